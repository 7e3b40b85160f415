"""`volume_db` and `limit` on the server's routes, on the CPU stand-in engine of
serve.py: parsed on /generate, /stream and /v1/audio/speech, 400 where the request is invalid or the
server has no stage, the default format implied, carried by every long-form and continuity row, and
the request of before where unset or 0."""

from types import SimpleNamespace

import numpy as np
import pytest

from pocket_tts_amd.audio import level_limit, pcm_i16_le_bytes, wav_bytes, wire_bytes
from pocket_tts_amd.serve import BatchScheduler, StandInEngine, TTSService, create_app, stand_in_sample
from test_text_frontend import synthetic_tokenizer

VOICE = SimpleNamespace(n_frames=10)
CEILING_DB = -26.0  # the stand-in's samples are small: u = 3 is 0.0235 at frame 0, the ceiling 0.0501


def frames(u, n):
    return np.concatenate([np.full(1920, stand_in_sample(u, k), np.float32) for k in range(n)])


def service(level=True, **kw):
    eng = StandInEngine(max_slots=4, max_ctx=10_000, wire=level, level=level, level_ceiling_db=CEILING_DB)
    sch = BatchScheduler(eng)
    return eng, sch, TTSService(sch, {"alba": VOICE}, default_voice="alba", **kw)


def test_http_volume_on_the_three_routes():
    from fastapi.testclient import TestClient

    eng, sch, svc = service(tokenizer=lambda s: [5] * len(s.split()))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        x = frames(3, 4)
        # unset, 0, null, and limit false: the request of before (no opts, float32 frames, today's bytes)
        for extra in ({}, {"volume_db": 0}, {"volume_db": 0.0}, {"volume_db": None}, {"limit": False},
                      {"volume_db": 0.004, "limit": None}):
            r = c.post("/generate", json={**body, **extra})
            assert r.status_code == 200 and r.content == wav_bytes(x), extra
            r = c.post("/stream", json={**body, **extra})
            assert r.status_code == 200 and r.content == pcm_i16_le_bytes(x), extra
        assert all(p.level() == (0, 0) and p.opts() == (0, 0, 0) and p.volume_db is None and p.limit is False
                   for p in eng.params_log) and len(eng.params_log) == 12
        # a gain alone: 24000 / pcm_s16le implied, the bytes of the rule over the row's frames
        r = c.post("/stream", json={**body, "volume_db": 12})
        want = level_limit(x, 1200, -2600)
        assert np.abs(x * 10 ** 0.6).max() > 10 ** -1.3 >= np.abs(want).max()  # the limiter engaged
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(want)
        assert eng.params_log[-1].level() == (1200, 0) and eng.params_log[-1].opts() == (0, 0, 0)
        # limit alone, and with an encoding; hundredths of a dB
        r = c.post("/generate", json={**body, "limit": True, "encoding": "ulaw"})
        assert r.status_code == 200
        assert r.content == wav_bytes(wire_bytes(level_limit(x, 0, -2600), "ulaw"), 24000, "ulaw")
        assert eng.params_log[-1].level() == (0, 1) and eng.params_log[-1].opts() == (0, 2, 0)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm",
                                            "volume_db": -6.014})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(level_limit(frames(3, 52), -601, -2600))
        assert eng.params_log[-1].level() == (-601, 0)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "volume_db": 0})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(frames(3, 52))
        assert eng.params_log[-1].level() == (0, 0)
        # 400: out of range (nothing admitted); a wrong type never reaches the service
        n = len(eng.params_log)
        for bad in ({"volume_db": 24.01}, {"volume_db": -25}, {"volume_db": 1e9}):
            assert c.post("/generate", json={**body, **bad}).status_code == 400, bad
            assert c.post("/stream", json={**body, **bad}).status_code == 400, bad
            assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, **bad}).status_code == 400, bad
        for bad in ({"volume_db": "loud"}, {"volume_db": [1]}, {"limit": "perhaps"}, {"limit": 2}):
            assert c.post("/generate", json={**body, **bad}).status_code in (400, 422), bad
            assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, **bad}).status_code in (400, 422), bad
        assert len(eng.params_log) == n
        with pytest.raises(ValueError):
            svc.request(token_ids=[3, 1], max_frames=2, limit=2)
        with pytest.raises(ValueError):
            svc.request(token_ids=[3, 1], max_frames=2, volume_db=float("nan"))
        assert len(eng.params_log) == n
        # the edges that are valid
        assert c.post("/generate", json={**body, "volume_db": 24}).status_code == 200
        assert c.post("/generate", json={**body, "volume_db": -24, "limit": True}).status_code == 200
        assert eng.params_log[-1].level() == (-2400, 1)
    finally:
        sch.close()


def test_http_400_on_a_server_without_the_stage():
    from fastapi.testclient import TestClient

    eng, sch, svc = service(level=False)
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 2}
        assert c.post("/generate", json=body).status_code == 200
        assert c.post("/generate", json={**body, "volume_db": 0}).status_code == 200
        assert c.post("/generate", json={**body, "limit": False}).status_code == 200
        assert c.post("/generate", json={**body, "volume_db": 2}).status_code == 400
        assert c.post("/stream", json={**body, "limit": True}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, "volume_db": -2}).status_code == 400
        assert len(eng.params_log) == 3
    finally:
        sch.close()


def test_params_without_the_fields_are_the_parents():
    """what a request with neither field submits: every field the parent commit's GenerationParams had,
    with the values the parent submitted, and the new ones at their defaults"""
    eng, sch, svc = service()
    try:
        r = svc.request(token_ids=[3, 1, 2], max_frames=2, temperature=0.5, lsd_steps=1)
        list(r.stream(timeout=20))
        p = eng.params_log[-1]
        assert (p.temp, p.eos_threshold, p.noise_clamp, p.frames_after_eos, p.max_frames, p.seed, p.lsd_steps) == \
            (0.5, svc.eos_threshold, svc.noise_clamp, 3, 2, 1, 1)
        assert (p.sample_rate, p.encoding, p.speed, p.pitch, p.prefix_latents, p.keep_codec) == \
            (None, None, None, None, None, False)
        assert (p.volume_db, p.limit) == (None, False) and r.wire is None and r.level == (0, 0)
    finally:
        sch.close()


@pytest.mark.parametrize("continuity", [False, True])
def test_long_form_and_continuity_rows_carry_the_fields(continuity):
    eng, sch, svc = service(tokenizer=synthetic_tokenizer(), temp=0.0)
    try:
        text = "Hello there. [pause:100ms] And again."
        plain = svc.request(text=text, long_form=True, continuity=continuity, max_frames=2, encoding="pcm_s16le")
        a = list(plain.stream(timeout=20))
        n_text = len(eng.params_log)
        assert n_text >= 2 and all(p.level() == (0, 0) for p in eng.params_log)
        loud = svc.request(text=text, long_form=True, continuity=continuity, max_frames=2, volume_db=6, limit=True)
        b = list(loud.stream(timeout=20))
        assert loud.wire == (24000, "pcm_s16le")
        assert [p.level() for p in eng.params_log[n_text:]] == [(600, 1)] * n_text
        assert [bool(p.keep_codec) for p in eng.params_log[n_text:]] == [bool(p.keep_codec) for p in eng.params_log[:n_text]]
        silence = wire_bytes(np.zeros(2400, np.float32), "pcm_s16le")  # 100 ms at 24 kHz: host-made, untouched
        assert silence in a and silence in b
        assert len(b"".join(b)) == len(b"".join(a))  # the stage keeps every row's length
        assert b"".join(b) != b"".join(a)
    finally:
        sch.close()
