"""Speech speed on the host: audio.tempo_wsola, the numpy restatement of the
rule the GPU tempo stage computes (tests/test_gpu_tempo.py pins the two to each other bit for
bit), its length and chunk-size functions, and the server's handling of `speed` on a CPU stand-in
engine with the engine's wire and tempo surface."""

import numpy as np
import pytest

from pocket_tts_amd import GenerationParams
from pocket_tts_amd.audio import (TEMPO_HS, TEMPO_R, pcm_i16_le_bytes, speed_permille, tempo_chunk_samples,
                                  tempo_hops_ready, tempo_len, tempo_window, tempo_wsola, wav_bytes, wire_bytes)
from pocket_tts_amd.serve import BatchScheduler, TTSService, create_app
from test_text_frontend import synthetic_tokenizer
from test_wire import VOICE, WireFakeEngine, utterance_frame

SPEEDS = [500, 800, 1250, 2000]


def test_tempo_len():
    for n in (0, 1, 2, 239, 240, 1919, 1920, 1921, 24000, 123457, 10**9 + 7):
        for sp in (500, 501, 730, 999, 1000, 1001, 1250, 1999, 2000):
            want = -(-n * 1000 // sp)
            assert tempo_len(n, sp) == want
            assert (want - 1) * sp < n * 1000 <= want * sp or n == 0


def test_speed_permille():
    assert speed_permille(None) == 0 and speed_permille(1.0) == 0 and speed_permille(1.0004) == 0
    assert speed_permille(0.5) == 500 and speed_permille(2) == 2000 and speed_permille(0.73) == 730
    for bad in (0.4994, 2.0006, 0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            speed_permille(bad)


def test_window_overlaps_to_one():
    w = tempo_window().astype(np.float64)
    assert w[0] == 0.0 and w[240] == 1.0
    assert np.abs(w[:240] + w[240:] - 1.0).max() < 1e-7


@pytest.mark.parametrize("sp", SPEEDS)
def test_periodic_signal_keeps_its_period(sp):
    """One random 120-sample period tiled to 2 s: every shifted window has the same energy, so by
    Cauchy-Schwarz the correlation is largest at a shift aligned with the period, and one lies
    within +-120; the output is then the periodic continuation itself (pitch kept, no seam), up to
    the zero-padded end."""
    per = (0.4 * np.random.default_rng(sp).uniform(-1, 1, 120)).astype(np.float32)
    x = np.tile(per, 400)
    y = tempo_wsola(x, sp)
    assert y.dtype == np.float32 and len(y) == tempo_len(len(x), sp)
    ref = np.tile(per, len(y) // 120 + 1)[:len(y)]
    err = float(np.abs(y - ref)[:-1200].max())
    print(f"sp {sp}: {len(y)} samples, max |y - periodic| {err:.3g}")
    assert err <= 1e-6


@pytest.mark.parametrize("sp", SPEEDS + [730, 1999])
def test_chunk_sizes_are_the_streams(sp):
    """The chunk-size function against a frame-by-frame run of the restatement; the frame-by-frame
    run against the whole-signal one; and the bound the engine's chunk slots are sized by."""
    rng = np.random.default_rng(1)
    for nfr in (1, 2, 7):
        x = (0.3 * rng.standard_normal(1920 * nfr)).astype(np.float32)
        chunks = tempo_wsola(x, sp, frame_len=1920)
        assert [len(c) for c in chunks] == [tempo_chunk_samples(f, sp, f == nfr - 1) for f in range(nfr)]
        assert np.array_equal(np.concatenate(chunks), tempo_wsola(x, sp))
        # a frame's chunk needs nothing of later frames: the stream so far, cut where it stands
        for f in range(nfr - 1):
            head = tempo_wsola(x[:1920 * (f + 1)], sp)[:tempo_hops_ready(1920 * (f + 1), sp) * TEMPO_HS]
            assert np.array_equal(head, np.concatenate(chunks[:f + 1]))
    for f in range(40):
        assert tempo_chunk_samples(f, sp, False) <= 1920 * 1000 // 500 + TEMPO_HS
        assert tempo_chunk_samples(f, sp, True) <= (1920 + TEMPO_R - 1) * 1000 // 500 + 1 <= 5528


# ---------------------------------------------------------------- the server on a CPU stand-in
class TempoFakeEngine(WireFakeEngine):
    """WireFakeEngine with the tempo surface: a row admitted with a speed (24 kHz rows only here)
    yields the chunks of the frame-by-frame run of tempo_wsola over its frames."""

    def __init__(self, max_slots=4, wire=True, tempo=True):
        super().__init__(max_slots, wire)
        self.tempo_enabled = tempo
        self.opts = []

    def open_many(self, slots, voices, ids_list, params_list):
        for p in params_list:
            if p.opts()[2] and not self.tempo_enabled:
                raise RuntimeError("a speed needs a tempo-enabled engine")
            self.opts.append(p.opts())
        super().open_many(slots, voices, ids_list, params_list)
        for s, p in zip(slots, params_list):
            self.rows[s]["sp"] = p.opts()[2]
            if p.opts()[2]:
                rate, enc = p.wire()
                self.rows[s]["fmt"] = (rate or 24000, ("pcm_s16le", "ulaw", "alaw")[(enc or 1) - 1])

    def _chunk(self, st, last):
        if not st.get("sp"):
            return super()._chunk(st, last)
        assert st["fmt"][0] == 24000
        if "chunks" not in st:  # the row's frames are known ahead (utterance_frame): one frame-by-frame run
            x = np.concatenate([utterance_frame(st["u"], k) for k in range(st["n"])])
            st["chunks"] = tempo_wsola(x, st["sp"], frame_len=1920)
        assert np.array_equal(st["x"][-1], utterance_frame(st["u"], len(st["x"]) - 1))
        return wire_bytes(st["chunks"][len(st["x"]) - 1], st["fmt"][1])


def frames(u, n):
    return np.concatenate([utterance_frame(u, k) for k in range(n)])


def test_http_speed():
    from fastapi.testclient import TestClient

    eng = TempoFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=lambda s: [5] * len(s.split()))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        x = frames(3, 4)
        # unset, and 1.0: the request of before (no opts at all, float32 frames, today's bytes)
        for extra in ({}, {"speed": 1.0}, {"speed": None}):
            r = c.post("/generate", json={**body, **extra})
            assert r.status_code == 200 and r.content == wav_bytes(x), extra
            r = c.post("/stream", json={**body, **extra})
            assert r.status_code == 200 and r.content == pcm_i16_le_bytes(x), extra
        assert eng.opts == [(0, 0, 0)] * 6 and eng.wire_fetches == 0
        # a speed alone: 24000 / pcm_s16le, the bytes of the rule over the row's frames
        r = c.post("/stream", json={**body, "speed": 1.25})
        want = pcm_i16_le_bytes(tempo_wsola(x, 1250))
        assert r.status_code == 200 and r.content == want and len(want) == 2 * tempo_len(len(x), 1250)
        assert eng.opts[-1] == (0, 0, 1250)
        r = c.post("/generate", json={**body, "speed": 0.5, "encoding": "ulaw"})
        assert r.status_code == 200 and r.content == wav_bytes(wire_bytes(tempo_wsola(x, 500), "ulaw"), 24000, "ulaw")
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "speed": 2.0})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(tempo_wsola(frames(3, 52), 2000))
        assert eng.opts[-1] == (0, 0, 2000)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "speed": 1.0})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(frames(3, 52)) and eng.opts[-1] == (0, 0, 0)
        # out of range: 400, nothing admitted
        n = len(eng.opts)
        for bad in (0.49, 2.01, 0, -1, 4.0):
            assert c.post("/generate", json={**body, "speed": bad}).status_code == 400, bad
            assert c.post("/stream", json={**body, "speed": bad}).status_code == 400, bad
            assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, "speed": bad}).status_code == 400
        assert len(eng.opts) == n
    finally:
        sch.close()


@pytest.mark.parametrize("wire,tempo", [(False, False), (True, False)])
def test_http_400_on_a_server_without_the_stage(wire, tempo):
    from fastapi.testclient import TestClient

    sch = BatchScheduler(TempoFakeEngine(max_slots=2, wire=wire, tempo=tempo))
    try:
        c = TestClient(create_app(TTSService(sch, {"alba": VOICE}, default_voice="alba")))
        body = {"token_ids": [3, 1, 2], "max_frames": 2}
        assert c.post("/generate", json=body).status_code == 200
        assert c.post("/generate", json={**body, "speed": 1.0}).status_code == 200
        assert c.post("/generate", json={**body, "speed": 1.5}).status_code == 400
        assert c.post("/stream", json={**body, "speed": 0.8}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, "speed": 0.8}).status_code == 400
    finally:
        sch.close()


def test_long_form_segments_carry_the_speed_and_pauses_keep_their_length():
    eng = TempoFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"v": VOICE}, default_voice="v", tokenizer=synthetic_tokenizer(), temp=0.0)
    try:
        text = "Hello there. [pause:100ms] And again."
        plain = svc.request(text=text, long_form=True, max_frames=2, encoding="pcm_s16le")
        a = list(plain.stream(timeout=20))
        fast = svc.request(text=text, long_form=True, max_frames=2, speed=2.0)
        b = list(fast.stream(timeout=20))
        assert fast.wire == (24000, "pcm_s16le")
        n_text = sum(1 for o in eng.opts if o[2] == 2000)
        assert n_text >= 2 and [o[2] for o in eng.opts] == [0] * n_text + [2000] * n_text
        silence = wire_bytes(np.zeros(2400, np.float32), "pcm_s16le")  # 100 ms at 24 kHz, whatever the speed
        assert silence in a and silence in b
        assert len(b"".join(b)) - len(silence) == (len(b"".join(a)) - len(silence)) // 2
    finally:
        sch.close()


def test_generation_params_opts():
    p = GenerationParams()
    assert p.opts() == (0, 0, 0)
    p.speed = 1.0
    assert p.opts() == (0, 0, 0)
    p.speed, p.sample_rate = 0.8, 8000
    assert p.opts() == (8000, 0, 800) and p.wire() == (8000, 0)
