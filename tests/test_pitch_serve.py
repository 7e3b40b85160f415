"""`pitch` on the server's routes, on CPU stand-in engines: parsed on
/generate, /stream and /v1/audio/speech, 400 where the request is invalid or the server has no
stage, carried by every long-form row, and byte-identical to today where unset or 0."""

import numpy as np
import pytest

from pocket_tts_amd.audio import (pcm_i16_le_bytes, pitch_len, pitch_plan, pitch_resample, tempo_len, tempo_wsola,
                                  wav_bytes, wire_bytes)
from pocket_tts_amd.serve import BatchScheduler, TTSService, create_app
from test_tempo import TempoFakeEngine, frames
from test_text_frontend import synthetic_tokenizer
from test_wire import VOICE, utterance_frame


class PitchFakeEngine(TempoFakeEngine):
    """TempoFakeEngine with the pitch surface: a row admitted with a pitch (24 kHz rows only here)
    yields the chunks of the streaming run of tempo_wsola at sp_w and pitch_resample over its frames."""

    def __init__(self, max_slots=4, wire=True, tempo=True, pitch=True):
        super().__init__(max_slots, wire, tempo)
        self.pitch_enabled = pitch
        self.cents = []

    def open_many(self, slots, voices, ids_list, params_list):
        for p in params_list:
            if p.cents() and not self.pitch_enabled:
                raise RuntimeError("a pitch needs a pitch-enabled engine")
            self.cents.append(p.cents())
        super().open_many(slots, voices, ids_list, params_list)
        for s, p in zip(slots, params_list):
            self.rows[s]["cents"] = p.cents()
            if p.cents():
                rate, enc = p.wire()
                self.rows[s]["fmt"] = (rate or 24000, ("pcm_s16le", "ulaw", "alaw")[(enc or 1) - 1])

    def _chunk(self, st, last):
        if not st.get("cents"):
            return super()._chunk(st, last)
        assert st["fmt"][0] == 24000
        if "chunks" not in st:
            st["chunks"] = host_chunks(st["u"], st["n"], st["sp"], st["cents"])
        return wire_bytes(st["chunks"][len(st["x"]) - 1], st["fmt"][1])


def host_chunks(u, n, sp, cents):
    """the per-frame chunks of the host rule over utterance u's n frames"""
    x = np.concatenate([utterance_frame(u, k) for k in range(n)])
    sp_w, step = pitch_plan(cents, sp)
    mid = [x[1920 * k:1920 * (k + 1)] for k in range(n)] if sp_w == 1000 else tempo_wsola(x, sp_w, frame_len=1920)
    return pitch_resample(np.concatenate(mid), step, [len(c) for c in mid])


def host_all(u, n, sp, cents):
    return np.concatenate(host_chunks(u, n, sp, cents))


def service(eng, **kw):
    sch = BatchScheduler(eng)
    return sch, TTSService(sch, {"alba": VOICE}, default_voice="alba", **kw)


def test_http_pitch_on_the_three_routes():
    from fastapi.testclient import TestClient

    eng = PitchFakeEngine(max_slots=4)
    sch, svc = service(eng, tokenizer=lambda s: [5] * len(s.split()))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 4}
        x = frames(3, 4)
        # unset, 0 and null: the request of before (no opts at all, float32 frames, today's bytes)
        for extra in ({}, {"pitch": 0}, {"pitch": 0.0}, {"pitch": None}):
            r = c.post("/generate", json={**body, **extra})
            assert r.status_code == 200 and r.content == wav_bytes(x), extra
            r = c.post("/stream", json={**body, **extra})
            assert r.status_code == 200 and r.content == pcm_i16_le_bytes(x), extra
        assert eng.cents == [0] * 8 and eng.opts == [(0, 0, 0)] * 8 and eng.wire_fetches == 0
        # a pitch alone: 24000 / pcm_s16le, the bytes of the rule over the row's frames
        r = c.post("/stream", json={**body, "pitch": 4})
        want = host_all(3, 4, 0, 400)
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(want)
        sp_w, step = pitch_plan(400, 0)
        assert len(want) == pitch_len(tempo_len(len(x), sp_w), step)
        assert eng.cents[-1] == 400 and eng.opts[-1] == (0, 0, 0)
        # with a speed and an encoding; the speed travels as the request's own, the engine plans sp_w
        r = c.post("/generate", json={**body, "pitch": -7, "speed": 0.8, "encoding": "ulaw"})
        assert r.status_code == 200
        assert r.content == wav_bytes(wire_bytes(host_all(3, 4, 800, -700), "ulaw"), 24000, "ulaw")
        assert eng.cents[-1] == -700 and eng.opts[-1] == (0, 2, 800)
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "pitch": 12})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(host_all(3, 52, 0, 1200))
        assert eng.cents[-1] == 1200
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1, 2], "words": 2, "response_format": "pcm", "pitch": 0})
        assert r.status_code == 200 and r.content == pcm_i16_le_bytes(frames(3, 52)) and eng.cents[-1] == 0
        # 400: out of range, and combinations with speed that leave WSOLA's range; nothing admitted
        n = len(eng.cents)
        for bad in ({"pitch": 12.01}, {"pitch": -13}, {"pitch": 7, "speed": 0.6}, {"pitch": -7, "speed": 1.8},
                    {"pitch": 12, "speed": 0.99}, {"pitch": -12, "speed": 1.01}):
            assert c.post("/generate", json={**body, **bad}).status_code == 400, bad
            assert c.post("/stream", json={**body, **bad}).status_code == 400, bad
            assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, **bad}).status_code == 400, bad
        assert len(eng.cents) == n
        # the edges that are valid
        assert c.post("/generate", json={**body, "pitch": 12, "speed": 2.0}).status_code == 200
        assert c.post("/generate", json={**body, "pitch": -12, "speed": 0.5}).status_code == 200
    finally:
        sch.close()


@pytest.mark.parametrize("wire,tempo,pitch", [(False, False, False), (True, False, False), (True, True, False)])
def test_http_400_on_a_server_without_the_stage(wire, tempo, pitch):
    from fastapi.testclient import TestClient

    sch, svc = service(PitchFakeEngine(max_slots=2, wire=wire, tempo=tempo, pitch=pitch))
    try:
        c = TestClient(create_app(svc))
        body = {"token_ids": [3, 1, 2], "max_frames": 2}
        assert c.post("/generate", json=body).status_code == 200
        assert c.post("/generate", json={**body, "pitch": 0}).status_code == 200
        assert c.post("/generate", json={**body, "pitch": 2}).status_code == 400
        assert c.post("/stream", json={**body, "pitch": -2}).status_code == 400
        assert c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, "pitch": 2}).status_code == 400
    finally:
        sch.close()


def test_long_form_rows_carry_the_pitch_and_pauses_keep_their_length():
    eng = PitchFakeEngine(max_slots=4)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"v": VOICE}, default_voice="v", tokenizer=synthetic_tokenizer(), temp=0.0)
    try:
        text = "Hello there. [pause:100ms] And again."
        plain = svc.request(text=text, long_form=True, max_frames=2, encoding="pcm_s16le")
        a = list(plain.stream(timeout=20))
        low = svc.request(text=text, long_form=True, max_frames=2, pitch=-5, speed=1.25)
        b = list(low.stream(timeout=20))
        assert low.wire == (24000, "pcm_s16le")
        n_text = sum(1 for v in eng.cents if v == -500)
        assert n_text >= 2 and eng.cents == [0] * n_text + [-500] * n_text
        assert [o[2] for o in eng.opts] == [0] * n_text + [1250] * n_text
        silence = wire_bytes(np.zeros(2400, np.float32), "pcm_s16le")  # 100 ms at 24 kHz, whatever the pitch
        assert silence in a and silence in b
        sp_w, step = pitch_plan(-500, 1250)
        per_row = pitch_len(tempo_len(2 * 1920, sp_w), step)
        assert len(b"".join(b)) - len(silence) == 2 * per_row * n_text
    finally:
        sch.close()
