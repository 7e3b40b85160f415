"""FLAC wire encoding, CPU side: the host restatement audio.flac_frames against
the independent decoder of tests/flac_decode.py, the server routes on a stand-in engine, and the ABI."""

import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import flac_decode as fd
from pocket_tts_amd import GenerationParams
from pocket_tts_amd import _lib
from pocket_tts_amd.audio import (ENCODINGS, flac_choose, flac_frames, flac_stream_header, pcm_i16, read_wav,
                                  wav_bytes, wav_header, wire_bytes)
from pocket_tts_amd.serve import BatchScheduler, TTSService, create_app

GOLDEN = Path(__file__).parent / "golden"
SIZES = (16, 17, 255, 256, 257, 630, 640, 650, 1920, 3860, 4607, 4608, 4609, 11058)
SIGNALS = ("zeros", "constant", "alternating", "noise", "sine", "impulse", "speech")


def firsts(n):
    return (0, 127, 128, 2047, 2048, 65535, 65536, 2**21 - 1, 2**21, 2**26 - 1, 2**26, 2**31, 2**36 - 1 - n)


_speech = []


def speech():
    """2 s of tests/golden/ref.wav (48 kHz) as 16-bit samples, read once"""
    if not _speech:
        x, sr = read_wav(GOLDEN / "ref.wav")
        assert sr == 48000
        _speech.append(pcm_i16(x[0][48000:48000 + 96000]))
    return _speech[0]


def signal(name, n):
    i = np.arange(n)
    if name == "zeros":
        return np.zeros(n, np.int16)
    if name == "constant":
        return np.full(n, -1234, np.int16)
    if name == "alternating":
        return np.where(i % 2 == 0, 32767, -32767).astype(np.int16)
    if name == "noise":
        return np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)
    if name == "sine":
        return np.round(20000 * np.sin(2 * np.pi * 440 * i / 24000)).astype(np.int16)
    if name == "impulse":  # silence, one full-scale sample at the end: one long unary run
        return np.where(i == n - 1, 32767, 0).astype(np.int16)
    return speech()[1000:1000 + n].copy()


def subframe_kind(frame):
    """the subframe header byte of the frame at the start of `frame`"""
    _, first, n, _ = fd.decode_frame(frame, 0)
    nb = next(k for k, lim in enumerate((7, 11, 16, 21, 26, 31, 36), 1) if first < 1 << lim)
    return frame[4 + nb + (1 if n <= 256 else 2) + 1]


@pytest.mark.parametrize("name", SIGNALS)
def test_round_trip_every_size(name):
    for n in SIZES:
        s = signal(name, n)
        first = firsts(n)[SIZES.index(n) % 13]
        data = flac_frames(s, first, 24000)
        got, info = fd.decode_frames(data, 24000)
        assert np.array_equal(got, s), (name, n)
        assert [m for _, m, _ in info] == [min(4608, n - a) for a in range(0, n, 4608)]
        at = first
        for f0, m, size in info:
            assert f0 == at and size <= 17 + 2 * m, (name, n, f0, m, size)
            at += m
        kind = subframe_kind(data)
        if name in ("zeros", "constant"):
            assert kind == 0x00 and len(data) <= 19 * len(info)
        if name in ("alternating", "noise"):
            assert kind == 0x02, "VERBATIM"  # (alternating: order-4 sums pass 2^32)
        if name == "sine" and n >= 255:
            assert kind >> 4 == 1 and len(data) < 2 * n * 0.7, "FIXED, and smaller"


def test_first_sample_numbers_and_rates():
    s = signal("speech", 640)
    for first in firsts(640):
        got, info = fd.decode_frames(flac_frames(s, first, 8000), 8000)
        assert np.array_equal(got, s) and info[0][:2] == (first, 640)
    for rate in (8000, 16000, 24000, 44100, 48000):
        assert np.array_equal(fd.decode_frames(flac_frames(s, 5, rate), rate)[0], s)
    with pytest.raises(ValueError):
        flac_frames(s, 2**36 - 639, 8000)
    with pytest.raises(ValueError):
        flac_frames(s, 0, 22050)


def test_long_unary_run():
    """n = 4607 admits no partitioning: one parameter for silence and a full-scale impulse"""
    s = signal("impulse", 4607)
    pick = flac_choose(s.astype(np.int64))
    assert pick[0] == "fixed" and pick[1:3] == (0, 0) and list(pick[3]) == [3]
    data = flac_frames(s, 0, 48000)
    assert np.array_equal(fd.decode_frames(data, 48000)[0], s)
    assert 8191 // 8 < len(data) < 8191 // 8 + 4607 * 4 // 8 + 20  # the run of 65534 >> 3 zero bits is in there


def test_speech_beats_the_order_2_baseline():
    """on speech the rule's total is at most that of: order 2, one partition, the best k per block"""
    s = speech()
    total = base = 0
    for a in range(0, s.size, 3840):
        blk = s[a:a + 3840]
        frame = flac_frames(blk, a, 48000)
        got, info = fd.decode_frames(frame, 48000)
        assert np.array_equal(got, blk)
        e = np.diff(blk.astype(np.int64), 2)
        u = np.where(e >= 0, 2 * e, -2 * e - 1)
        bits = 8 + 32 + 6 + 4 + min(int((u >> k).sum()) + u.size * (k + 1) for k in range(15))
        hdr = 4 + (1 if a < 128 else 2 if a < 2048 else 3 if a < 65536 else 4) + 2 + 1  # the same header bytes
        base += hdr + -(-bits // 8) + 2
        total += len(frame)
    print(f"flac {total} bytes, order-2 baseline {base}, s16 {2 * s.size}: {total / (2 * s.size):.3f} vs "
          f"{base / (2 * s.size):.3f}")
    assert total <= base
    assert total < 0.6 * 2 * s.size


def test_header_and_rejections():
    h = flac_stream_header(44100, 123456789)
    assert len(h) == 42
    f = fd.parse_header(h)
    assert f == {"min_block": 16, "max_block": 4608, "min_frame": 0, "max_frame": 0, "rate": 44100, "channels": 1,
                 "bits": 16, "total": 123456789, "md5": 0}
    assert fd.parse_header(flac_stream_header(8000))["total"] == 0
    assert ENCODINGS[3] == "flac"
    for fn in (lambda: wire_bytes(np.zeros(4, np.float32), "flac"), lambda: wav_bytes(np.zeros(4, np.float32), 24000, "flac"),
               lambda: wav_header(8, 24000, "flac")):
        with pytest.raises(ValueError, match="flac"):
            fn()


def test_an_all_equal_block_is_immediate_and_a_block_is_fast():
    import time

    t0 = time.perf_counter()
    for _ in range(20):
        flac_frames(np.zeros(3840, np.int16), 0, 48000)
    assert (time.perf_counter() - t0) / 20 < 2e-3
    s = speech()[:3840]
    t0 = time.perf_counter()
    for _ in range(5):
        flac_frames(s, 0, 48000)
    assert (time.perf_counter() - t0) / 5 < 15e-3, "well under the naive prototype's 20-30 ms"


# ---------------------------------------------------------------- the ABI
def test_abi():
    L = _lib.lib()
    assert L.ptts_abi_version() == _lib.ABI_VERSION == 6
    assert C.sizeof(_lib.SlotOpts) == 24 and C.sizeof(_lib.SlotOpts2) == 40
    assert _lib.WIRE_FLAC == 4
    for name in ("ptts_flac_enable", "ptts_flac_bound", "ptts_flac_encode"):
        assert getattr(L, name).argtypes is not None
    assert [L.ptts_flac_bound(n) for n in (-1, 0, 1, 3860, 4608, 4609, 11058)] == \
        [0, 0, 19, 7737, 9233, 9252, 22167]
    assert L.ptts_wire_len(1920, 24000, _lib.WIRE_FLAC) == 0  # the size is not a function of n
    assert L.ptts_flac_enable(None, 1) != 0 and b"null engine" in L.ptts_last_error()


# ---------------------------------------------------------------- the server on a CPU stand-in
def utterance_frame(u, k):
    t = np.arange(1920) + 1920 * k
    return (0.5 * np.sin(t * (0.01 + 0.003 * u)) + 0.2 * np.sin(t * 0.21)).astype(np.float32)


class FlacFakeEngine:
    """Pipelined stand-in (frames one call late) with the wire surface at 24 kHz: a FLAC row yields,
    per frame, the frames of its 16-bit chunk, numbered on from the row's admission."""

    def __init__(self, max_slots=4, flac=True):
        self.max_slots, self.max_ctx, self.pipeline, self.wire, self.flac_enabled = max_slots, 10_000, True, True, flac
        self.rows, self.issued, self.pending, self.admitted = {}, [], None, []

    def open_many(self, slots, voices, ids_list, params_list):
        for s, ids, p in zip(slots, ids_list, params_list):
            rate, enc = p.wire()
            assert rate in (0, 24000), "the stand-in does not resample"
            self.rows[s] = {"u": int(ids[0]), "k": 0, "n": p.max_frames, "enc": ENCODINGS[enc - 1] if enc else None}
            self.admitted.append(self.rows[s]["enc"])

    def step_async(self, n):
        cur = {"pcm": np.zeros((n, 1920), np.float32), "valid": np.zeros(n, bool), "last": np.zeros(n, bool),
               "wire": [b""] * n}
        for s, st in list(self.rows.items()):
            if s >= n:
                continue
            cur["pcm"][s] = utterance_frame(st["u"], st["k"])
            cur["valid"][s] = True
            if st["enc"] == "flac":
                cur["wire"][s] = flac_frames(pcm_i16(cur["pcm"][s]), 1920 * st["k"], 24000)
            elif st["enc"]:
                cur["wire"][s] = wire_bytes(cur["pcm"][s], st["enc"])
            st["k"] += 1
            cur["last"][s] = st["k"] == st["n"]
            if cur["last"][s]:
                del self.rows[s]
        prev, self.pending = self.pending, cur
        out = {"pcm": np.zeros((n, 1920), np.float32), "valid": np.zeros(n, bool), "last": np.zeros(n, bool),
               "wire": [b""] * n}
        if prev is not None:
            m = min(n, prev["valid"].size)
            for key in ("pcm", "valid", "last"):
                out[key][:m] = prev[key][:m]
            out["wire"][:m] = prev["wire"][:m]
        self.issued = self.issued[-1:] + [out]

    def fetch(self, n, calls_back=0):
        o = self.issued[-1 - calls_back]
        return SimpleNamespace(pcm=o["pcm"], valid=o["valid"], last=o["last"])

    def fetch_wire(self, n, calls_back=0):
        return list(self.issued[-1 - calls_back]["wire"])

    def sync(self):
        pass


VOICE = SimpleNamespace(n_frames=10)


def samples(u, n_frames):
    return pcm_i16(np.concatenate([utterance_frame(u, k) for k in range(n_frames)]))


def test_http_flac_routes():
    from fastapi.testclient import TestClient

    eng = FlacFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=lambda s: [5] * len(s.split()))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        r = c.post("/stream", json={**body, "encoding": "flac"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
        h, s, info = fd.decode_stream(r.content)
        assert (h["rate"], h["total"]) == (24000, 0) and np.array_equal(s, samples(3, 4))
        assert [(a, n) for a, n, _ in info] == [(1920 * k, 1920) for k in range(4)]
        r = c.post("/generate", json={**body, "encoding": "flac", "sample_rate": 24000})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
        h, s, _ = fd.decode_stream(r.content)
        assert h["total"] == 4 * 1920 and np.array_equal(s, samples(3, 4))
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "flac"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
        h, s, _ = fd.decode_stream(r.content)
        assert h["total"] == 52 * 1920 and np.array_equal(s, samples(3, 52))
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "encoding": "flac"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
        assert eng.admitted == ["flac"] * 4
        # refusals: nothing is admitted
        assert c.post("/generate", json={"text": "One. Two.", "encoding": "flac", "long_form": True}).status_code == 400
        assert c.post("/stream", json={"text": "One. Two.", "encoding": "flac", "continuity": True}).status_code == 400
        assert c.post("/v1/audio/speech", json={"input": "One. Two.", "response_format": "flac",
                                                "long_form": True}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [1], "words": 1, "response_format": "flac",
                                                "encoding": "ulaw"}).status_code == 400
        assert c.post("/generate", json={**body, "encoding": "mp3"}).status_code == 400
        assert c.post("/stream", json={**body, "encoding": "mp3"}).status_code == 400
        assert eng.admitted == ["flac"] * 4
        # the other encodings are what they were
        r = c.post("/stream", json={**body, "encoding": "ulaw"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/PCMU"
    finally:
        sch.close()


def test_http_400_on_a_server_without_flac():
    from fastapi.testclient import TestClient

    eng = FlacFakeEngine(max_slots=2, flac=False)
    sch = BatchScheduler(eng)
    try:
        c = TestClient(create_app(TTSService(sch, {"alba": VOICE}, default_voice="alba")))
        body = {"token_ids": [3, 1, 2], "max_frames": 2}
        assert c.post("/generate", json={**body, "encoding": "flac"}).status_code == 400
        assert c.post("/stream", json={**body, "encoding": "flac"}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [3], "words": 1, "response_format": "flac"}).status_code == 400
        assert eng.admitted == []
        assert c.post("/generate", json={**body, "encoding": "alaw"}).status_code == 200
    finally:
        sch.close()


def test_params_carry_the_encoding():
    from pocket_tts_amd.engine import WIRE_ENCODINGS

    assert WIRE_ENCODINGS["flac"] == _lib.WIRE_FLAC
    p = GenerationParams(temp=0.0, max_frames=2)
    p.sample_rate, p.encoding = 8000, "flac"
    assert p.wire() == (8000, 4)
