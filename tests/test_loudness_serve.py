"""`loudness_lufs` and `loudness` on the server's routes, voice calibration and GET /voices/NAME
(DESIGN.md section 27), on the CPU stand-in engine of serve.py, whose meter is the host rule
audio.LoudnessMeter over what a row's wire stage reads.

The stand-in's signal of utterance u is a staircase from (u % 128) * 256 / 32767: the K-weighting's
high-pass leaves the step at its start, which is what every reading here measures (about -61 LUFS for
the calibration sentence). The unmeasurable voice is that of a server with no tokenizer, which cannot
say the sentence."""

import base64
from types import SimpleNamespace

import numpy as np
import pytest

from pocket_tts_amd.audio import (level_limit, loudness_blocks, loudness_gain_cdb, loudness_integrated,
                                  pcm_i16_le_bytes, wav_bytes)
from pocket_tts_amd.serve import (CALIBRATION_SEED, CALIBRATION_TEXT, BatchScheduler, StandInEngine, TTSService,
                                  create_app, stand_in_sample)
from pocket_tts_amd.text import segment_request
from test_text_frontend import synthetic_tokenizer

VOICE = SimpleNamespace(n_frames=10)
CEILING_DB = -1.0
TOK = lambda s: [5] * len(s.split())  # noqa: E731


def frames(u, n):
    return np.concatenate([np.full(1920, stand_in_sample(u, k), np.float32) for k in range(n)])


def service(loud=True, level=True, tokenizer=TOK, **kw):
    eng = StandInEngine(max_slots=4, max_ctx=10_000, wire=loud or level, level=level, level_ceiling_db=CEILING_DB,
                        loud=loud)
    sch = BatchScheduler(eng)
    return eng, sch, TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=tokenizer, **kw)


def calibrated(tokenizer=TOK):
    """The stand-in voice's loudness by the host rule: the calibration sentence's frames."""
    ids, mgl, _ = segment_request(CALIBRATION_TEXT, tokenizer)
    return loudness_integrated(loudness_blocks(frames(int(ids[0]), mgl)))


def wav_clip_b64(seed=0):
    x = (0.1 * np.random.default_rng(seed).standard_normal(24000)).astype(np.float32)
    return base64.b64encode(wav_bytes(x)).decode()


def test_calibration_sentence_is_short():
    from pathlib import Path

    from pocket_tts_amd.text import load_tokenizer, prepare_text_prompt

    tok = load_tokenizer(str(Path(__file__).parent / "golden" / "reference_tokenizer.json"))
    assert len(tok(prepare_text_prompt(CALIBRATION_TEXT))) <= 50


def test_calibration_at_registration_and_lazily_for_a_clip():
    from fastapi.testclient import TestClient

    eng, sch, svc = service()
    try:
        want = calibrated()
        assert want is not None and -70 < want < -30
        # the voice the server started with: one metered row, the fixed seed, no gain, 24000 / pcm_s16le
        assert len(eng.params_log) == 1 and svc.voice_lufs == {"alba": want}
        p = eng.params_log[0]
        assert p.loudness and p.seed == CALIBRATION_SEED and p.level() == (0, 0) and p.opts() == (24000, 1, 0)
        assert (p.temp, p.eos_threshold, p.noise_clamp) == (svc.temp, svc.eos_threshold, svc.noise_clamp)
        c = TestClient(create_app(svc))
        r = c.get("/voices/alba")
        assert r.status_code == 200 and r.json() == {"name": "alba", "frames": 10, "loudness_lufs": want}
        assert c.get("/voices/nobody").status_code == 404
        assert c.get("/voices").json() == {"voices": ["alba"], "default": "alba"}  # as it was
        # POST /voices/NAME calibrates before it answers
        x = (0.1 * np.random.default_rng(1).standard_normal(24000)).astype(np.float32)
        assert c.post("/voices/bert", content=wav_bytes(x)).status_code == 200
        assert len(eng.params_log) == 2 and eng.params_log[1].loudness and eng.params_log[1].seed == CALIBRATION_SEED
        assert c.get("/voices/bert").json()["loudness_lufs"] == want
        # an inline clip: calibrated on first use of loudness_lufs, not again, and not without the field
        clip = wav_clip_b64()
        body = {"token_ids": [3, 1, 2], "max_frames": 2, "voice": clip}
        assert c.post("/generate", json=body).status_code == 200
        assert len(eng.params_log) == 3 and not eng.params_log[2].loudness
        for _ in range(2):
            r = c.post("/generate", json={**body, "loudness_lufs": -40})
            assert r.status_code == 200 and r.headers["X-Gain-dB"] == f"{loudness_gain_cdb(-40, want) / 100:.2f}"
        assert [bool(p.loudness) for p in eng.params_log[3:]] == [True, False, False]
    finally:
        sch.close()


def test_target_becomes_a_gain_on_the_three_routes():
    from fastapi.testclient import TestClient

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        cal = calibrated()
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        x = frames(3, 4)
        for target in (-40.0, -38.5, -16, -5):  # the last two clamp at +24 dB
            gain = max(-2400, min(2400, round(100 * (target - cal))))
            assert (gain == 2400) == (target > -30)
            want = level_limit(x, gain, round(100 * CEILING_DB))
            r = c.post("/generate", json={**body, "loudness_lufs": target})
            assert r.status_code == 200 and r.content == wav_bytes(pcm_i16_le_bytes(want), 24000, "pcm_s16le")
            assert r.headers["X-Gain-dB"] == f"{gain / 100:.2f}" and "X-Loudness-LUFS" not in r.headers
            assert eng.params_log[-1].level() == (gain, 1) and not eng.params_log[-1].loudness
            r = c.post("/stream", json={**body, "loudness_lufs": target})
            assert r.status_code == 200 and r.content == pcm_i16_le_bytes(want) and r.headers["X-Gain-dB"] == f"{gain / 100:.2f}"
            assert eng.params_log[-1].level() == (gain, 1)
            r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm",
                                                "loudness_lufs": target})
            assert r.status_code == 200 and r.headers["X-Gain-dB"] == f"{gain / 100:.2f}"
            assert r.content == pcm_i16_le_bytes(level_limit(frames(3, 52), gain, round(100 * CEILING_DB)))
            assert eng.params_log[-1].level() == (gain, 1)
    finally:
        sch.close()


@pytest.mark.parametrize("continuity", [False, True])
def test_every_long_form_row_carries_the_gain(continuity):
    eng, sch, svc = service(tokenizer=synthetic_tokenizer(), temp=0.0)
    try:
        cal = svc.voice_lufs["alba"]
        assert cal == calibrated(synthetic_tokenizer()) and cal is not None
        n0 = len(eng.params_log)
        text = "Hello there. [pause:100ms] And again."
        r = svc.request(text=text, long_form=True, continuity=continuity, max_frames=2, loudness_lufs=-40, loudness=True)
        out = list(r.stream(timeout=20))
        gain = loudness_gain_cdb(-40, cal)
        rows = eng.params_log[n0:]
        assert len(rows) >= 2 and [p.level() for p in rows] == [(gain, 1)] * len(rows) and all(p.loudness for p in rows)
        assert r.gain_db == gain / 100 and r.wire == (24000, "pcm_s16le")
        assert pcm_i16_le_bytes(np.zeros(2400, np.float32)) in out  # the pause: host-made silence, untouched
        # pooled over the segments: each row's gating blocks, gated once
        energy = [np.concatenate(it.loud_rows) for it in r.items if hasattr(it, "loud_rows")]
        assert len(energy) == len(rows) and r.loudness() == loudness_integrated(energy)
    finally:
        sch.close()


def test_metered_responses():
    from fastapi.testclient import TestClient

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 6}
        want = loudness_integrated(loudness_blocks(frames(3, 6)))
        assert want is not None
        r = c.post("/generate", json={**body, "loudness": True})
        assert r.status_code == 200 and r.content == wav_bytes(frames(3, 6)) and r.headers["X-Loudness-LUFS"] == f"{want:.2f}"
        assert eng.params_log[-1].loudness and eng.params_log[-1].level() == (0, 0)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "loudness": True})
        w52 = loudness_integrated(loudness_blocks(frames(3, 52)))
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(frames(3, 52)) and r.headers["X-Loudness-LUFS"] == f"{w52:.2f}"
        r = c.post("/generate", json={"token_ids": [3, 1, 2], "max_frames": 1, "loudness": True})  # 80 ms: no gating block
        assert r.status_code == 200 and r.headers["X-Loudness-LUFS"] == "none"
        # with a gain: the meter reads the level stage's output
        r = c.post("/generate", json={**body, "loudness": True, "volume_db": 6})
        lv = level_limit(frames(3, 6), 600, round(100 * CEILING_DB))
        assert r.headers["X-Loudness-LUFS"] == f"{loudness_integrated(loudness_blocks(lv)):.2f}"
        assert c.post("/stream", json={**body, "loudness": True}).status_code == 400
        assert c.post("/stream", json={**body, "loudness": False}).status_code == 200
    finally:
        sch.close()


def test_timestamps_json_carries_the_loudness():
    from fastapi.testclient import TestClient

    eng = StandInEngine(max_slots=4, max_ctx=10_000, wire=True, level=True, loud=True, align=True)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": VOICE}, default_voice="alba", tokenizer=synthetic_tokenizer(), temp=0.0)
    try:
        c = TestClient(create_app(svc))
        r = c.post("/generate", json={"text": "hello world good day", "max_frames": 6, "timestamps": True, "loudness": True})
        assert r.status_code == 200
        j = r.json()
        assert "words" in j and "loudness_lufs" in j
        assert r.headers["X-Loudness-LUFS"] == ("none" if j["loudness_lufs"] is None else f"{j['loudness_lufs']:.2f}")
        j = c.post("/generate", json={"text": "hello world good day", "max_frames": 6, "timestamps": True}).json()
        assert "loudness_lufs" not in j
    finally:
        sch.close()


def test_refusals():
    from fastapi.testclient import TestClient

    body = {"token_ids": [3, 1, 2], "max_frames": 2}
    speech = {"token_ids": [3, 1], "words": 1}
    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        n = len(eng.params_log)
        for bad in ({"loudness_lufs": -40.01}, {"loudness_lufs": -4.99}, {"loudness_lufs": 0}, {"loudness_lufs": 1e9},
                    {"loudness_lufs": -16, "volume_db": 3}, {"loudness_lufs": -16, "volume_db": 0}):
            assert c.post("/generate", json={**body, **bad}).status_code == 400, bad
            assert c.post("/stream", json={**body, **bad}).status_code == 400, bad
            assert c.post("/v1/audio/speech", json={**speech, **bad}).status_code == 400, bad
        for bad in ({"loudness_lufs": "loud"}, {"loudness": "yes please"}, {"loudness": 2}):
            assert c.post("/generate", json={**body, **bad}).status_code in (400, 422), bad
        with pytest.raises(ValueError):
            svc.request(token_ids=[3, 1], max_frames=2, loudness_lufs=float("nan"))
        assert len(eng.params_log) == n  # nothing was admitted
        assert c.post("/generate", json={**body, "loudness_lufs": -40}).status_code == 200  # the edges
        assert c.post("/generate", json={**body, "loudness_lufs": -5}).status_code == 200
    finally:
        sch.close()
    # a server without --loudness, and one without --volume
    for loud, level in ((False, True), (True, False), (False, False)):
        eng, sch, svc = service(loud=loud, level=level)
        try:
            c = TestClient(create_app(svc))
            assert svc.voice_lufs == ({"alba": calibrated()} if loud else {})
            n = len(eng.params_log)
            assert c.post("/generate", json={**body, "loudness_lufs": -30}).status_code == 400
            assert c.post("/stream", json={**body, "loudness_lufs": -30}).status_code == 400
            assert c.post("/v1/audio/speech", json={**speech, "loudness_lufs": -30}).status_code == 400
            assert c.post("/generate", json={**body, "loudness": True}).status_code == (200 if loud else 400)
            assert c.post("/generate", json={**body, "loudness": False}).status_code == 200
            assert len(eng.params_log) == n + 1 + int(loud)
            assert c.get("/voices/alba").json()["loudness_lufs"] == (calibrated() if loud else None)
        finally:
            sch.close()
    # a voice whose calibration is unmeasurable
    eng, sch, svc = service(tokenizer=None)
    try:
        c = TestClient(create_app(svc))
        assert svc.voice_lufs == {"alba": None} and not eng.params_log
        assert c.get("/voices/alba").json()["loudness_lufs"] is None
        r = c.post("/generate", json={**body, "loudness_lufs": -16})
        assert r.status_code == 400 and "unmeasurable" in r.json()["detail"]
        assert c.post("/stream", json={**body, "loudness_lufs": -16}).status_code == 400
        assert c.post("/generate", json=body).status_code == 200
    finally:
        sch.close()


def test_requests_without_the_fields_are_byte_identical():
    """The same requests on a server with the stage and on one without: the same bytes, the same
    headers but for none of the new ones, and the params of before."""
    from fastapi.testclient import TestClient

    got = []
    for loud in (False, True):
        eng, sch, svc = service(loud=loud)
        try:
            c = TestClient(create_app(svc))
            n = len(eng.params_log)
            out = [c.post("/generate", json={"token_ids": [3, 1, 2], "max_frames": 3}),
                   c.post("/stream", json={"token_ids": [3, 1, 2], "max_frames": 3, "loudness": None, "loudness_lufs": None}),
                   c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "volume_db": 3}),
                   c.post("/generate", json={"token_ids": [7, 1], "max_frames": 2, "encoding": "ulaw", "limit": True})]
            assert all(r.status_code == 200 for r in out)
            assert not any(h.lower() in ("x-gain-db", "x-loudness-lufs") for r in out for h in r.headers)
            assert not any(p.loudness for p in eng.params_log[n:]) and len(eng.params_log) == n + 4
            got.append([(r.content, r.headers["content-type"]) for r in out])
        finally:
            sch.close()
    assert got[0] == got[1]


def test_calibration_comes_last_and_once():
    """A request that is refused for another reason has not calibrated its clip; the refusal a
    request with a bad voice and another bad field gets is the other field's, as before; two first
    uses of one clip at once calibrate it once; /stream takes a clip with a target."""
    import threading

    from fastapi.testclient import TestClient

    eng, sch, svc = service()
    try:
        c = TestClient(create_app(svc))
        clip = wav_clip_b64(3)
        body = {"token_ids": [3, 1, 2], "max_frames": 2, "voice": clip, "loudness_lufs": -40}
        n = len(eng.params_log)
        for bad in ({"lsd_steps": 99}, {"speed": 9}, {"sample_rate": 12345}, {"max_frames": None}):
            assert c.post("/generate", json={**body, **bad}).status_code == 400, bad
        assert len(eng.params_log) == n and not svc.clip_lufs  # nothing ran
        r = c.post("/generate", json={"token_ids": [3, 1], "max_frames": 2, "voice": "nobody", "lsd_steps": 99})
        assert r.status_code == 400 and "lsd_steps" in r.json()["detail"]
        r = c.post("/generate", json={"token_ids": [3, 1], "max_frames": 2, "voice": "nobody"})
        assert r.status_code == 400 and "unknown voice" in r.json()["detail"]
        out = []
        ts = [threading.Thread(target=lambda: out.append(svc.request(token_ids=[3, 1, 2], max_frames=2, voice=clip,
                                                                      loudness_lufs=-40))) for _ in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(30)
        assert len(out) == 3 and len({r.gain_db for r in out}) == 1
        for r in out:
            r.wire_audio(timeout=20)
        assert sum(bool(p.loudness) for p in eng.params_log[n:]) == 1 and len(svc.clip_lufs) == 1
        r = c.post("/stream", json={**body, "voice": wav_clip_b64(4)})
        assert r.status_code == 200 and r.headers["X-Gain-dB"] == f"{out[0].gain_db:.2f}" and len(svc.clip_lufs) == 2
    finally:
        sch.close()
