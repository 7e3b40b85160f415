"""Wire formats on the host side (no GPU): the two G.711 rules (pinned values, CPython's audioop
where it exists), ptts_wire_len, the WAV headers of the three encodings parsed back, the size
handling of ptts_slot_opts, and the server with a CPU stand-in engine that implements fetch_wire:
requests with different formats share a batch and reach the client byte for byte, a request that
names no format gets exactly the bytes it got before, and unknown values get 400."""

import ctypes as C
import io
import struct
import wave
from math import gcd
from types import SimpleNamespace

import numpy as np
import pytest

from pocket_tts_amd import GenerationParams
from pocket_tts_amd.audio import lin2alaw, lin2ulaw, pcm_i16, pcm_i16_le_bytes, wav_bytes, wav_header, wire_bytes
from pocket_tts_amd.serve import BatchScheduler, TTSService, create_app

# s -> (mu-law, A-law)
PINNED = {0: (0xFF, 0xD5), -1: (0x7E, 0x55), 4: (0xFE, 0xD5), 100: (0xF2, 0xD3), 1000: (0xCE, 0xFA),
          -1000: (0x4E, 0x7A), 32767: (0x80, 0xAA), -32768: (0x00, 0x2A)}
CHUNKS = {8000: (630, 640, 650), 16000: (1270, 1280, 1290), 24000: (1920, 1920, 1920),
          44100: (3510, 3528, 3546), 48000: (3820, 3840, 3860)}
ALL = np.arange(-32768, 32768).astype(np.int16)


def test_g711_pinned_values():
    for s, (u, a) in PINNED.items():
        assert int(lin2ulaw(np.array([s], np.int16))[0]) == u, s
        assert int(lin2alaw(np.array([s], np.int16))[0]) == a, s


def test_g711_against_the_scalar_rule_on_all_inputs():
    """the vectorised rules of audio.py against the rule as the C header states it, value by value"""
    u_ends = [0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF]
    a_ends = [0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]
    u, a = [], []
    for s in ALL.tolist():
        v = s >> 2
        mask = 0x7F if v < 0 else 0xFF
        v = min(abs(v), 8159) + 33
        seg = next((k for k, e in enumerate(u_ends) if v <= e), 8)
        u.append((0x7F ^ mask) if seg == 8 else (((seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask))
        v, mask = (s >> 3, 0xD5) if s >= 0 else ((-s - 1) >> 3, 0x55)
        seg = next(k for k, e in enumerate(a_ends) if v <= e)
        a.append(((seg << 4) | ((v >> (1 if seg < 2 else seg)) & 15)) ^ mask)
    assert lin2ulaw(ALL).tolist() == u
    assert lin2alaw(ALL).tolist() == a


def test_g711_against_audioop():
    audioop = pytest.importorskip("audioop")  # in the standard library up to CPython 3.12
    raw = ALL.astype("<i2").tobytes()
    assert lin2ulaw(ALL).tobytes() == audioop.lin2ulaw(raw, 2)
    assert lin2alaw(ALL).tobytes() == audioop.lin2alaw(raw, 2)


def test_wire_bytes_rule():
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 0.99999, -0.00001], np.float32)
    assert pcm_i16(x).tolist() == [0, 16383, -16383, 32767, -32767, 32767, -32767, 32766, 0]
    assert wire_bytes(x, "pcm_s16le") == pcm_i16_le_bytes(x)
    assert wire_bytes(x, "ulaw") == lin2ulaw(pcm_i16(x)).tobytes()
    assert wire_bytes(x, "alaw") == lin2alaw(pcm_i16(x)).tobytes()
    with pytest.raises(ValueError):
        wire_bytes(x, "mp3")


def test_wire_len():
    from pocket_tts_amd import lib

    f = lib().ptts_wire_len
    for rate, (first, mid, last) in CHUNKS.items():
        per_frame = 1920 * rate // 24000
        assert first + mid + last == 3 * per_frame  # the table's chunks add up to the whole signal
        assert f(1920, rate, 1) == 2 * per_frame and f(1920, rate, 2) == per_frame == f(1920, rate, 3)
        assert f(3 * 1920, rate, 1) == 2 * 3 * per_frame
    assert f(1000, 8000, 2) == 334 and f(1001, 44100, 1) == 2 * -(-1001 * 147 // 80)  # ceil(n up / down)
    assert f(1920, 22050, 1) == 0 and f(1920, 8000, 0) == 0 and f(1920, 8000, 4) == 0 and f(-1, 8000, 1) == 0


def parse_wav(data):
    """-> (fmt fields, fmt chunk size, fact sample count or None, data bytes)"""
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    pos, fmt, fmt_size, fact, body = 12, None, None, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if cid == b"fmt ":
            fmt, fmt_size = struct.unpack_from("<HHIIHH", data, pos + 8), size
            if size == 18:
                assert struct.unpack_from("<H", data, pos + 24)[0] == 0  # cbSize
        elif cid == b"fact":
            fact = struct.unpack_from("<I", data, pos + 8)[0]
        elif cid == b"data":
            body = data[pos + 8:pos + 8 + size]
            assert len(body) == size
        pos += 8 + size + (size & 1)
    assert pos == len(data)
    return fmt, fmt_size, fact, body


@pytest.mark.parametrize("n", [480, 481])
def test_wav_headers_of_the_three_encodings(n):
    x = (0.4 * np.sin(np.arange(n) * 0.05)).astype(np.float32)
    fmt, size, fact, body = parse_wav(wav_bytes(x, 16000, "pcm_s16le"))
    assert (fmt, size, fact) == ((1, 1, 16000, 32000, 2, 16), 16, None) and body == pcm_i16_le_bytes(x)
    assert wav_bytes(x, 16000) == wav_bytes(x, 16000, "pcm_s16le")
    w = wave.open(io.BytesIO(wav_bytes(x, 16000)), "rb")
    assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, n)
    for enc, tag in (("ulaw", 7), ("alaw", 6)):
        data = wav_bytes(x, 8000, enc)
        fmt, size, fact, body = parse_wav(data)
        assert (fmt, size, fact) == ((tag, 1, 8000, 8000, 1, 8), 18, n)
        assert body == wire_bytes(x, enc) and len(data) % 2 == 0
        assert wav_bytes(wire_bytes(x, enc), 8000, enc) == data  # bytes the engine already encoded
        assert data.startswith(wav_header(n, 8000, enc))


def test_slot_opts_size_handling():
    """ptts_slots_open_opts reads entries `size` bytes apart and refuses a size that is no
    ptts_slot_opts of any version before it looks at anything else (so: testable without an
    engine); a size it accepts gets as far as the engine check."""
    from pocket_tts_amd import lib
    from pocket_tts_amd._lib import SlotOpts

    assert C.sizeof(SlotOpts) == 24 and SlotOpts.lsd_steps.offset == 8 and SlotOpts.wire_encoding.offset == 16
    L = lib()

    def call(opts):
        rc = L.ptts_slots_open_opts(None, len(opts), None, None, None, None, None, C.cast(opts, C.c_void_p))
        return rc, L.ptts_last_error().decode()

    for bad in (4, 8, 10, 13):
        rc, msg = call((SlotOpts * 1)(SlotOpts(bad, 0, 0, 0)))
        assert rc == 1 and "ptts_slot_opts.size" in msg, (bad, msg)
    rc, msg = call((SlotOpts * 2)(SlotOpts(24, 0, 0, 0), SlotOpts(16, 0, 0, 0)))
    assert rc == 1 and "differs" in msg
    for good in (0, 16, 24, 32):  # 0: this header's; 16: a header that ended at wire_rate; 32: a later one
        n = max(good, 24) // 8
        raw = (C.c_uint64 * (2 * n))()
        raw[0] = good
        raw[(good or 24) // 8] = good
        rc, msg = L.ptts_slots_open_opts(None, 2, None, None, None, None, None, C.cast(raw, C.c_void_p)), None
        assert rc == 1 and "null engine" in L.ptts_last_error().decode(), good
    assert L.ptts_slots_open_opts(None, 1, None, None, None, None, None, None) == 1  # NULL opts: defaults


# ---------------------------------------------------------------- the server on a CPU stand-in
def resample_f32(x, rate):
    """the resample_poly rule in numpy (f64 accumulation, rounded to f32 once)"""
    g = gcd(24000, rate)
    up, down = rate // g, 24000 // g
    if up == down:
        return np.asarray(x, np.float32)
    mr = max(up, down)
    half = 10 * mr
    L = 2 * half + 1
    k = np.arange(L, dtype=np.float64) - half
    h = np.sinc(k / mr) / mr * np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (k / half) ** 2))) / np.i0(5.0)
    h = ((h / h.sum()).astype(np.float32) * np.float32(up)).astype(np.float64)
    x = np.asarray(x, np.float64)
    n = len(x)
    a = np.arange(-(-n * up // down), dtype=np.int64) * down + half
    j = (a // up)[:, None] - np.arange(L // up + 2, dtype=np.int64)[None, :]
    idx = a[:, None] - j * up
    ok = (j >= 0) & (j < n) & (idx >= 0) & (idx < L)
    y = (np.where(ok, x[np.clip(j, 0, n - 1)], 0.0) * np.where(ok, h[np.clip(idx, 0, L - 1)], 0.0)).sum(axis=1)
    return y.astype(np.float32)


def utterance_frame(u, k):
    t = np.arange(1920) + 1920 * k
    return (0.5 * np.sin(t * (0.01 + 0.003 * u)) + 0.2 * np.sin(t * 0.21)).astype(np.float32)


class WireFakeEngine:
    """Pipelined stand-in (frames one call late) with the engine's wire surface: a row admitted with
    a format also yields, per frame, the chunk the streaming rule emits: after N samples every
    output whose filter support is complete, the rest with the last frame."""

    def __init__(self, max_slots=4, wire=True):
        self.max_slots, self.max_ctx, self.pipeline, self.wire = max_slots, 10_000, True, wire
        self.rows, self.issued, self.pending = {}, [], None
        self.admitted, self.wire_fetches = [], 0

    def open_many(self, slots, voices, ids_list, params_list):
        for s, ids, p in zip(slots, ids_list, params_list):
            rate, enc = p.wire()
            if (rate or enc) and not self.wire:
                raise RuntimeError("a wire format needs a wire-enabled engine")
            fmt = (rate or 24000, ("pcm_s16le", "ulaw", "alaw")[(enc or 1) - 1]) if rate or enc else None
            self.rows[s] = {"u": int(ids[0]), "k": 0, "n": p.max_frames, "fmt": fmt, "x": [], "sent": 0}
            self.admitted.append(fmt)

    def _chunk(self, st, last):
        rate, enc = st["fmt"]
        x = np.concatenate(st["x"])
        g = gcd(24000, rate)
        up, down = rate // g, 24000 // g
        half = 0 if up == down else 10 * max(up, down)
        N = len(x)
        end = -(-N * up // down) if last or up == down else (N * up - 1 - half) // down + 1
        y = resample_f32(x, rate)[st["sent"]:end]
        st["sent"] = end
        return wire_bytes(y, enc)

    def step_async(self, n):
        cur = {"pcm": np.zeros((n, 1920), np.float32), "valid": np.zeros(n, bool), "last": np.zeros(n, bool),
               "wire": [b""] * n}
        for s, st in list(self.rows.items()):
            if s >= n:
                continue
            cur["pcm"][s] = utterance_frame(st["u"], st["k"])
            cur["valid"][s] = True
            st["k"] += 1
            cur["last"][s] = st["k"] == st["n"]
            if st["fmt"]:
                st["x"].append(cur["pcm"][s].copy())
                cur["wire"][s] = self._chunk(st, cur["last"][s])
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
        self.wire_fetches += 1
        return list(self.issued[-1 - calls_back]["wire"])

    def sync(self):
        pass


VOICE = SimpleNamespace(n_frames=10)


def expected(u, n_frames, rate, enc):
    x = np.concatenate([utterance_frame(u, k) for k in range(n_frames)])
    return wire_bytes(resample_f32(x, rate), enc)


def test_scheduler_mixed_formats_share_a_batch():
    """six requests through four slots: four formats and two plain ones; the wire rows get their
    fetch_wire bytes untouched, chunk by chunk, the plain rows their float32 frames"""
    eng = WireFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    try:
        jobs = [(None, 3), ((8000, "ulaw"), 4), ((48000, "pcm_s16le"), 2), ((44100, "alaw"), 5), (None, 2),
                ((16000, "pcm_s16le"), 1), ((24000, "ulaw"), 3)]
        reqs = []
        for u, (fmt, n) in enumerate(jobs):
            p = GenerationParams(temp=0.0, eos_threshold=float("inf"), max_frames=n, seed=1)
            if fmt:
                p.sample_rate, p.encoding = fmt
            reqs.append(sch.submit([u + 1, 7], VOICE, p))
        for u, ((fmt, n), r) in enumerate(zip(jobs, reqs)):
            items = list(r.stream(timeout=10))
            assert len(items) == n
            if fmt is None:
                assert r.wire is None
                assert all(np.array_equal(f, utterance_frame(u + 1, k)) for k, f in enumerate(items))
                continue
            assert r.wire == fmt and all(isinstance(c, bytes) for c in items)
            per = 1 if fmt[1] != "pcm_s16le" else 2
            first, mid, last = CHUNKS[fmt[0]]
            sizes = [1920 * fmt[0] // 24000] if n == 1 else [first] + [mid] * (n - 2) + [last]
            assert [len(c) for c in items] == [s * per for s in sizes], (u, fmt)
            assert b"".join(items) == expected(u + 1, n, *fmt), (u, fmt)
    finally:
        sch.close()


def test_scheduler_skips_fetch_wire_without_wire_rows():
    eng = WireFakeEngine(max_slots=2)
    sch = BatchScheduler(eng)
    try:
        p = GenerationParams(temp=0.0, eos_threshold=float("inf"), max_frames=3, seed=1)
        assert len(list(sch.submit([1, 7], VOICE, p).stream(timeout=10))) == 3
        assert eng.wire_fetches == 0
    finally:
        sch.close()


def test_http_formats_defaults_and_400s():
    from fastapi.testclient import TestClient

    eng = WireFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=lambda s: [5] * len(s.split()))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        x = np.concatenate([utterance_frame(3, k) for k in range(4)])
        # a request without the new fields: today's bytes (the host rule on the float32 frames)
        r = c.post("/generate", json=body)
        assert r.status_code == 200 and r.content == wav_bytes(x)
        r = c.post("/stream", json=body)
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(x) and r.headers["content-type"] == "audio/pcm"
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm"})
        x52 = np.concatenate([utterance_frame(3, k) for k in range(52)])
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(x52)
        assert eng.admitted == [None, None, None] and eng.wire_fetches == 0
        # formats
        r = c.post("/stream", json={**body, "sample_rate": 8000, "encoding": "ulaw"})
        assert r.status_code == 200 and r.content == expected(3, 4, 8000, "ulaw")
        assert r.headers["content-type"] == "audio/PCMU"
        r = c.post("/stream", json={**body, "sample_rate": 48000})  # encoding defaults to 16-bit
        assert r.status_code == 200 and r.content == expected(3, 4, 48000, "pcm_s16le")
        r = c.post("/stream", json={**body, "encoding": "alaw"})  # rate defaults to 24 kHz
        assert r.status_code == 200 and r.content == expected(3, 4, 24000, "alaw")
        r = c.post("/generate", json={**body, "sample_rate": 16000, "encoding": "alaw"})
        fmt, size, fact, data = parse_wav(r.content)
        assert r.status_code == 200 and (fmt, size) == ((6, 1, 16000, 16000, 1, 8), 18)
        assert data == expected(3, 4, 16000, "alaw") and fact == len(data)
        r = c.post("/generate", json={**body, "sample_rate": 44100})
        w = wave.open(io.BytesIO(r.content), "rb")
        assert (w.getframerate(), w.getsampwidth(), w.getnframes()) == (44100, 2, 4 * 3528)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "ulaw"})
        assert r.status_code == 200 and r.content == expected(3, 52, 8000, "ulaw")
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "alaw",
                                             "sample_rate": 16000})
        assert r.status_code == 200 and r.content == expected(3, 52, 16000, "alaw")
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "sample_rate": 16000})
        assert parse_wav(r.content)[3] == expected(3, 52, 16000, "pcm_s16le")
        # refusals
        n_admitted = len(eng.admitted)
        for bad in ({"sample_rate": 22050}, {"encoding": "mp3"}, {"sample_rate": 0}, {"encoding": ""}):
            assert c.post("/generate", json={**body, **bad}).status_code == 400, bad
            assert c.post("/stream", json={**body, **bad}).status_code == 400, bad
        assert c.post("/v1/audio/speech", json={"token_ids": [1], "words": 1, "response_format": "ulaw",
                                                "encoding": "alaw"}).status_code == 400
        assert len(eng.admitted) == n_admitted
    finally:
        sch.close()


def test_http_400_on_a_server_without_wire():
    from fastapi.testclient import TestClient

    sch = BatchScheduler(WireFakeEngine(max_slots=2, wire=False))
    try:
        c = TestClient(create_app(TTSService(sch, {"alba": VOICE}, default_voice="alba")))
        body = {"token_ids": [3, 1, 2], "max_frames": 2}
        assert c.post("/generate", json=body).status_code == 200
        assert c.post("/generate", json={**body, "sample_rate": 8000}).status_code == 400
        assert c.post("/stream", json={**body, "encoding": "ulaw"}).status_code == 400
    finally:
        sch.close()
