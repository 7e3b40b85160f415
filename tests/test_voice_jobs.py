"""Voice jobs without a GPU: the C ABI surface, and the server's per-request voices (base64 WAV in
the `voice` field, POST /voices, the per-engine LRU cache) on the stand-in engine."""

import base64
import ctypes as C
import threading

import numpy as np
import pytest

from pocket_tts_amd.audio import wav_bytes
from pocket_tts_amd.serve import (BatchScheduler, MultiGpuScheduler, StandInEngine, TTSService, VoiceCache, clip_frames,
                                  create_app, voice_spec_audio, wav_wire_samples)

PTTS_ERR_INVALID = 1


# ------------------------------------------------------------------ C ABI
def test_abi_surface():
    from pocket_tts_amd._lib import SIGNATURES, lib

    L = lib()
    assert L.ptts_abi_version() == 6
    sig = {n: (r, a) for n, r, a in SIGNATURES}
    vp, ip = C.c_void_p, C.c_int
    assert sig["ptts_voice_job_start"] == (ip, [vp, vp, ip, ip, ip, ip, ip, C.POINTER(vp)])
    assert sig["ptts_voice_job_start_prompt"] == (ip, [vp, C.POINTER(C.c_float), ip, C.POINTER(vp)])
    assert sig["ptts_voice_ready"] == (ip, [vp, ip, C.POINTER(ip)])
    assert sig["ptts_voice_jobs_reserve"] == (ip, [vp, ip])
    for name in ("ptts_voice_job_start", "ptts_voice_job_start_prompt", "ptts_voice_ready", "ptts_voice_jobs_reserve"):
        assert getattr(L, name) is not None
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "pocket_tts.h").read_text()
    assert "#define PTTS_ABI_VERSION 6" in header
    assert "#define PTTS_SAMPLES_F32 0" in header and "#define PTTS_SAMPLES_S16 1" in header


def test_abi_null_safe_and_invalid_arguments_without_a_gpu():
    from pocket_tts_amd._lib import lib

    L = lib()
    ready = C.c_int(-1)
    assert L.ptts_voice_ready(None, 0, C.byref(ready)) == 0 and ready.value == 1  # no voice: no pending job
    ready = C.c_int(-1)
    assert L.ptts_voice_ready(None, 1, C.byref(ready)) == 0 and ready.value == 1
    assert L.ptts_voice_ready(None, 0, None) == PTTS_ERR_INVALID
    x = np.zeros(1920, np.float32)
    h = C.c_void_p(123)
    rc = L.ptts_voice_job_start(None, x.ctypes.data_as(C.c_void_p), x.size, 0, 24000, 0, 0, C.byref(h))
    assert rc == PTTS_ERR_INVALID and h.value is None and b"null engine" in L.ptts_last_error()
    assert L.ptts_voice_job_start(None, x.ctypes.data_as(C.c_void_p), x.size, 0, 24000, 0, 0, None) == PTTS_ERR_INVALID
    h = C.c_void_p(123)
    assert L.ptts_voice_job_start_prompt(None, x.ctypes.data_as(C.POINTER(C.c_float)), 1, C.byref(h)) == PTTS_ERR_INVALID
    assert h.value is None
    assert L.ptts_voice_job_start_prompt(None, None, 1, None) == PTTS_ERR_INVALID
    assert L.ptts_voice_jobs_reserve(None, 16) == PTTS_ERR_INVALID


# ------------------------------------------------------------------ helpers
def _clip(seconds=0.5, sr=16000, seed=0, channels=1):
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal((channels, int(seconds * sr)))).astype(np.float32)
    return wav_bytes(x if channels > 1 else x[0], sr)


def _b64(data):
    return base64.b64encode(data).decode()


def _service(slots=4, cache=64, **kw):
    eng = StandInEngine(max_slots=slots, max_ctx=512)
    sch = BatchScheduler(eng, voice_cache=cache)
    svc = TTSService(sch, {"alba": eng.voice_from_prompt(np.zeros((4, 1024), np.float32))}, default_voice="alba", **kw)
    return eng, sch, svc


BODY = {"token_ids": [3, 1, 2], "max_frames": 4}


def test_voice_spec_rule_and_wire_samples():
    wav = _clip()
    assert voice_spec_audio("data:audio/wav;base64," + _b64(wav)) == wav
    assert voice_spec_audio(_b64(wav)) == wav
    assert voice_spec_audio("A" * 50) is None  # voice.rs:180: raw base64 needs more than 100 characters
    assert voice_spec_audio("A" * 100) is None
    assert voice_spec_audio("hf://owner/repo/" + "a" * 120 + ".wav") is None  # ':' and '.' are not base64
    assert voice_spec_audio("/srv/voices/" + "a" * 120 + ".wav") is None
    with pytest.raises(ValueError):
        voice_spec_audio("data:audio/wav;base64,@@@@")
    x, sr = wav_wire_samples(wav)  # 16-bit PCM travels as int16
    assert x.dtype == np.int16 and sr == 16000 and x.size == 8000
    assert clip_frames(8000, 16000) == 7 and clip_frames(1920, 24000) == 1 and clip_frames(1921, 24000) == 2
    f = np.array([0.25, -0.7512345, 0.1], np.float32)
    import struct
    hdr = b"RIFF" + struct.pack("<I", 36 + 12) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 24000, 96000, 4, 32)
    y, _ = wav_wire_samples(hdr + b"data" + struct.pack("<I", 12) + f.tobytes())
    assert y.dtype == np.float32 and np.array_equal(y, f)


# ------------------------------------------------------------------ routes on the stand-in engine
def test_base64_voices_synthesise_and_bad_specs_are_refused():
    from fastapi.testclient import TestClient

    eng, sch, svc = _service(max_voice_seconds=2.0)
    try:
        c = TestClient(create_app(svc))
        wav = _clip()
        r = c.post("/generate", json={**BODY, "voice": "data:audio/wav;base64," + _b64(wav)})
        assert r.status_code == 200 and len(r.content) == 44 + 4 * 1920 * 2
        assert eng.voice_jobs == 1
        r = c.post("/stream", json={**BODY, "voice": _b64(_clip(seed=1))})  # raw base64
        assert r.status_code == 200 and len(r.content) == 4 * 1920 * 2
        assert eng.voice_jobs == 2
        r = c.post("/v1/audio/speech", json={"token_ids": [3, 1], "words": 1, "voice": _b64(wav)})
        assert r.status_code == 200 and eng.voice_jobs == 2  # the first clip again: from the cache
        assert c.post("/generate", json={**BODY, "voice": "A" * 50}).status_code == 400  # an unknown voice
        assert c.post("/generate", json={**BODY, "voice": _b64(_clip(channels=2))}).status_code == 400  # stereo
        assert c.post("/generate", json={**BODY, "voice": _b64(_clip(seconds=2.5))}).status_code == 400  # too long
        assert c.post("/generate", json={**BODY, "voice": _b64(b"RIFF" + b"\0" * 200)}).status_code == 400
        for spec in ("hf://kyutai/tts-voices/alba.wav", "/etc/passwd", "../voices/alba.wav", __file__,
                     "/tmp/" + "a" * 120 + ".wav"):
            r = c.post("/generate", json={**BODY, "voice": spec})
            assert r.status_code == 400 and "voice" in r.json()["detail"], spec
        assert eng.voice_jobs == 2
        assert c.post("/generate", json=BODY).status_code == 200  # the server still serves
    finally:
        sch.close()


def test_register_named_voice_at_run_time():
    from fastapi.testclient import TestClient
    from safetensors.numpy import save as st_save

    eng, sch, svc = _service()
    try:
        c = TestClient(create_app(svc))
        assert c.get("/voices").json() == {"voices": ["alba"], "default": "alba"}
        assert c.post("/generate", json={**BODY, "voice": "x"}).status_code == 400
        r = c.post("/voices/x", content=_clip(), headers={"content-type": "audio/wav"})
        assert r.status_code == 200 and r.json() == {"voice": "x", "frames": 7}
        assert c.get("/voices").json()["voices"] == ["alba", "x"]
        assert c.post("/generate", json={**BODY, "voice": "x"}).status_code == 200
        assert eng.voice_jobs == 1 and len(sch.voices) == 0  # owned by the registry, not by the LRU
        first = svc.voices["x"]
        prompt = st_save({"audio_prompt": np.zeros((1, 9, 1024), np.float32)})
        r = c.post("/voices/x", content=prompt)  # replaced, by a precomputed audio_prompt
        assert r.status_code == 200 and r.json()["frames"] == 9 and first.closed
        assert svc.voices["x"].n_frames == 9 and not svc.voices["x"].closed
        assert c.post("/generate", json={**BODY, "voice": "x"}).status_code == 200
        assert c.post("/voices/x", content=_clip(channels=2)).status_code == 400
        assert c.post("/voices/x", content=b"not a voice").status_code == 400
        assert c.post("/voices/bad name!", content=_clip()).status_code == 400
    finally:
        sch.close()


def test_concurrent_requests_with_one_new_clip_share_one_job():
    eng, sch, svc = _service(slots=8)
    eng.step_s = 0.002
    try:
        spec = _b64(_clip(seed=5))
        out, gate = [], threading.Barrier(6)

        def one():
            gate.wait()
            out.append(svc.request(token_ids=[3, 1], max_frames=3, voice=spec).audio(timeout=30).size)

        threads = [threading.Thread(target=one) for _ in range(6)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert out == [3 * 1920] * 6
        assert eng.voice_jobs == 1 and sch.voices.jobs == 1 and sch.voices.hits == 5
    finally:
        sch.close()


def test_lru_evicts_the_oldest_entry_at_capacity():
    eng, sch, svc = _service(cache=2)
    try:
        specs = [_b64(_clip(seed=s)) for s in range(3)]
        for s in specs[:2]:
            svc.request(token_ids=[3], max_frames=2, voice=s).audio(timeout=30)
        a, b = (sch.voices._d[k] for k in sch.voices.keys())
        svc.request(token_ids=[3], max_frames=2, voice=specs[0]).audio(timeout=30)  # a is the most recent now
        assert eng.voice_jobs == 2
        svc.request(token_ids=[3], max_frames=2, voice=specs[2]).audio(timeout=30)  # evicts b
        assert len(sch.voices) == 2 and b.closed and not a.closed and eng.voice_jobs == 3
        svc.request(token_ids=[3], max_frames=2, voice=specs[1]).audio(timeout=30)  # b's clip is cloned again
        assert eng.voice_jobs == 4 and a.closed
    finally:
        sch.close()
    cache = VoiceCache(0)  # capacity 0: nothing is kept past the admission
    assert len(cache) == 0


def test_multi_gpu_scheduler_clones_on_the_engine_it_routes_to():
    engines = [StandInEngine(max_slots=2, max_ctx=512, step_s=0.002) for _ in range(2)]  # the first is still busy
    multi = MultiGpuScheduler([BatchScheduler(e) for e in engines])
    voices = {"alba": [e.voice_from_prompt(np.zeros((4, 1024), np.float32)) for e in engines]}
    svc = TTSService(multi, voices, default_voice="alba")
    try:
        assert svc.max_ctx == 512
        spec = _b64(_clip(seed=9))
        reqs = [svc.request(token_ids=[3], max_frames=40, voice=spec) for _ in range(2)]  # least loaded: one each
        assert [r.audio(timeout=30).size for r in reqs] == [40 * 1920] * 2
        assert [getattr(e, "voice_jobs", 0) for e in engines] == [1, 1]  # the cache is per engine
        assert svc.register_voice("y", _clip(seed=3)) == 7
        assert len(svc.voices["y"]) == 2
        assert svc.request(token_ids=[3], max_frames=2, voice="y").audio(timeout=30).size == 2 * 1920
    finally:
        multi.close()


class _StrictEngine(StandInEngine):
    """A stand-in whose admission, like the real engine's, refuses a voice that was closed."""

    def open_many(self, slots, voices, ids_list, params_list):
        if any(getattr(v, "closed", False) for v in voices):
            raise ValueError("voice belongs to another engine")
        super().open_many(slots, voices, ids_list, params_list)


def test_replacing_a_voice_that_a_queued_request_holds_keeps_the_server_up():
    """Both slots busy, a third request naming `x` waits; `x` is replaced meanwhile. The waiting
    request is admitted with the voice it was given (closed only afterwards), and nothing stops."""
    eng = _StrictEngine(max_slots=2, max_ctx=512, step_s=0.002)
    sch = BatchScheduler(eng)
    svc = TTSService(sch, {"alba": eng.voice_from_prompt(np.zeros((4, 1024), np.float32))}, default_voice="alba")
    try:
        assert svc.register_voice("x", _clip(seed=1)) == 7
        first = svc.voices["x"]
        busy = [svc.request(token_ids=[3], max_frames=60, voice="x") for _ in range(2)]
        queued = svc.request(token_ids=[4], max_frames=3, voice="x")  # waits behind the full slots
        assert sch.load() == 3
        svc.register_voice("x", _clip(seed=2))  # returns while `queued` still waits
        assert svc.voices["x"] is not first and not first.closed  # held by the queued request
        assert queued.audio(timeout=30).size == 3 * 1920
        assert [r.audio(timeout=30).size for r in busy] == [60 * 1920] * 2
        assert svc.request(token_ids=[3], max_frames=2, voice="x").audio(timeout=30).size == 2 * 1920
        assert sch.running and first.closed and sch.retired == []  # closed once nothing queued held it
        # a voice closed behind the scheduler's back fails its own request only
        svc.voices["x"].close()
        with pytest.raises(Exception):
            svc.request(token_ids=[3], max_frames=2, voice="x").audio(timeout=30)
        assert sch.running
        assert svc.request(token_ids=[3], max_frames=2).audio(timeout=30).size == 2 * 1920
    finally:
        sch.close()


def test_scheduler_calls_taken_by_a_failing_pass_are_failed_not_left_hanging():
    """An admission that fails for another reason than a refused argument still stops the scheduler;
    a call() the same pass had taken is failed with it, not left waiting for ever."""
    from pocket_tts_amd import GenerationParams
    from pocket_tts_amd.serve import Request, _Call

    class HipError(RuntimeError):
        code = 2

    eng = StandInEngine(max_slots=2, max_ctx=512)

    def boom(*a):
        raise HipError("device lost")

    eng.open_many = boom
    sch = BatchScheduler(eng)
    try:
        req = Request(np.array([3], np.int32), eng.voice_from_prompt(np.zeros((4, 1024), np.float32)),
                      GenerationParams(max_frames=5))
        c = _Call(lambda: 1)
        with sch.cv:  # one pass takes both
            sch.waiting.append(req)
            sch.calls.append(c)
            sch.cv.notify()
        assert c.done.wait(timeout=10) and isinstance(c.error, RuntimeError) and c.result is None
        with pytest.raises(HipError):
            req.audio(timeout=10)
        with pytest.raises(RuntimeError):
            sch.call(lambda: 2)
    finally:
        sch.close()
