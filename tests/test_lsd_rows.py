"""Per-utterance LSD step counts, the parts that need no GPU: the C boundary's new entry points on
a null engine, the request-level rules of the server (TTSService, /generate) over the stand-in
engine, and the unchanged ptts_gen_params marshalling."""

import ctypes as C

import numpy as np
import pytest

from pocket_tts_amd import GenerationParams
from pocket_tts_amd.serve import BatchScheduler, StandInEngine, TTSService, create_app


def test_new_entry_points_reject_a_null_engine():
    from pocket_tts_amd._lib import lib

    L = lib()
    p = GenerationParams(max_frames=2).to_c()
    ids = np.array([1, 2], np.int32)
    assert L.ptts_slot_open_ex(None, 0, None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 2, C.byref(p), 1) == 1
    assert b"null engine" in L.ptts_last_error()
    assert L.ptts_slots_open_ex(None, 0, None, None, None, None, None, None) == 1
    cap, run = C.c_int(-7), C.c_int(-7)
    assert L.ptts_lsd_steps(None, C.byref(cap), C.byref(run)) == 1
    assert (cap.value, run.value) == (-7, -7)


def test_generation_params_marshalling_is_unchanged():
    """lsd_steps travels beside ptts_gen_params (ptts_slot_open_ex), not inside it."""
    base = dict(temp=0.3, eos_threshold=-2.0, noise_clamp=1.5, frames_after_eos=4, max_frames=9, seed=77)
    a, b = GenerationParams(**base).to_c(), GenerationParams(**base, lsd_steps=3).to_c()
    assert GenerationParams(**base).lsd_steps is None
    assert C.sizeof(a) == C.sizeof(b) == 32
    assert bytes(a) == bytes(b)
    assert [f for f, _ in a._fields_] == ["temp", "eos_threshold", "noise_clamp", "frames_after_eos", "max_frames",
                                          "seed"]


class RecordingEngine(StandInEngine):
    """The stand-in engine, keeping the params of every admission (open_many as the scheduler calls it)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.admitted = []

    def open_many(self, slots, voices, ids_list, params_list):
        self.admitted += list(params_list)
        super().open_many(slots, voices, ids_list, params_list)


@pytest.fixture()
def service4():
    eng = RecordingEngine(max_slots=2)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": eng.voice_from_prompt(np.zeros((4, 1024), np.float32))}, default_voice="alba",
                     max_lsd_steps=4)
    yield svc, eng
    sch.close()


def test_service_accepts_counts_up_to_its_cap(service4):
    svc, eng = service4
    for n in (1, 4):
        req = svc.request(token_ids=[n, 7], max_frames=2, lsd_steps=n)
        assert len(list(req.stream(timeout=10))) == 2
        assert eng.admitted[-1].lsd_steps == n
    req = svc.request(token_ids=[9, 7], max_frames=1)  # no count of its own: the engine's default
    assert len(list(req.stream(timeout=10))) == 1
    assert eng.admitted[-1].lsd_steps is None
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match=r"\[1, 4\]"):
            svc.request(token_ids=[1], max_frames=1, lsd_steps=bad)
    assert len(eng.admitted) == 3


def test_generate_route_answers_200_and_400(service4):
    from fastapi.testclient import TestClient

    svc, eng = service4
    c = TestClient(create_app(svc))
    for n in (1, 4):
        r = c.post("/generate", json={"token_ids": [3, 1], "max_frames": 2, "lsd_steps": n})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        assert eng.admitted[-1].lsd_steps == n
    for bad in (0, 5):
        r = c.post("/generate", json={"token_ids": [3, 1], "max_frames": 2, "lsd_steps": bad})
        assert r.status_code == 400 and "[1, 4]" in r.text


def test_default_service_still_refuses_another_count():
    eng = RecordingEngine(max_slots=1)
    sch = BatchScheduler(eng)
    try:
        svc = TTSService(sch, {"alba": eng.voice_from_prompt(np.zeros((4, 1024), np.float32))}, default_voice="alba")
        assert svc.max_lsd_steps == 1
        with pytest.raises(ValueError, match="lsd_steps"):
            svc.request(token_ids=[1], max_frames=1, lsd_steps=4)
        assert len(list(svc.request(token_ids=[1], max_frames=1, lsd_steps=1).stream(timeout=10))) == 1
    finally:
        sch.close()
