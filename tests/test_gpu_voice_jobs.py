"""Voice jobs (ptts_voice_job_start / _prompt): a clone enqueued on the engine's voice stream with
a workspace of its own, admissible at once, ordered against admission by an event.

Tolerances are the project's own: conditioning against the oracle at 1e-5 abs
(test_voice_frontend.py), latents / PCM at LAT_TOL / PCM_TOL (conftest.py). Shapes are the smallest
at which each path can go wrong: one frame, a partly filled last frame, the int16 ingest with the
2:1 polyphase rule, full chunks plus a remainder through the one-launch replicate, the rubato rule."""

import numpy as np
import pytest
from conftest import LAT_TOL, PCM_TOL, load_golden, load_ref_wav, pcm_err

pytestmark = pytest.mark.gpu

IDS = np.array([260, 2994, 262, 578, 682], np.int32)


def _pad_frames(y):
    pad = np.zeros((y.size + 1919) // 1920 * 1920, np.float32)
    pad[:y.size] = y
    return pad


def _ref13():
    """The first second of ref.wav (48 kHz int16): 24,000 samples at 24 kHz, 13 frames."""
    return np.ascontiguousarray(load_ref_wav()[:48000])


def _oracle_cond(oracle, x, sr, chunk=-1, rubato=False):
    from _oracle import resample, resample_septic

    x = np.asarray(x).reshape(-1)
    xf = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)
    y = xf if sr == 24000 else (resample_septic if rubato else resample)(xf, sr)
    return oracle.encode(_pad_frames(y), chunk)[0]


def _oracle_frames(oracle, cond, ids, n, ctx=512):
    s = oracle.new_state(ctx)
    s.prefill(cond)
    s.prefill_tokens(ids)
    out, lat = [], None
    for _ in range(n):
        ref = s.step(lat)
        lat = ref["latent"]
        out.append(ref)
    return out


def _params(n):
    import pocket_tts_amd as pt

    return pt.GenerationParams(temp=0.0, eos_threshold=float("inf"), max_frames=n)


def _check_generation(eng, oracle, voice, cond, slot=0, n=2):
    """n frames from `voice` on `slot` (rows 0 .. slot stepped) against the oracle prefilled with cond."""
    eng.open(slot, voice, IDS, _params(n))
    refs = _oracle_frames(oracle, cond, IDS, n)
    for i in range(n):
        r = eng.step(slot + 1)
        assert r.valid[slot], i
        err = float(np.abs(r.latents[slot] - refs[i]["latent"]).max())
        print(f"frame {i}: latent max |d| {err:.3g}, pcm max |d| {pcm_err(r.pcm[slot] - refs[i]['pcm']):.3g}")
        assert err <= LAT_TOL, (i, err)
        assert abs(float(r.eos_logits[slot]) - refs[i]["eos_logit"]) <= LAT_TOL, i
        assert pcm_err(r.pcm[slot] - refs[i]["pcm"]) <= PCM_TOL, i
    eng.close_slot(slot)


def _cases():
    rng = np.random.default_rng(11)
    d = load_golden("encoder_chunked_5f.safetensors")
    return {
        "one_frame_24k": (0.1 * rng.standard_normal(1920).astype(np.float32), 24000, 0, "poly", -1, 1),
        "padded_last_frame": (0.1 * rng.standard_normal(1920 * 3 + 7).astype(np.float32), 24000, 0, "poly", -1, 4),
        "ref_wav_i16_48k": (_ref13(), 48000, 0, "poly", -1, 13),
        "chunked_5f": (d["pcm"], 24000, int(d["meta"][2]), "poly", int(d["meta"][2]), 5),
        "rubato_48k": (0.2 * rng.standard_normal(2 * 3840 + 77).astype(np.float32), 48000, -1, "rubato", -1, 3),
        "five_frames_48k": (0.1 * rng.standard_normal(5 * 3840 - 100).astype(np.float32), 48000, 2, "poly", 2, 5),
    }


def test_sync_clone_between_jobs_leaves_job_workspace_alone(gpu_engine, oracle):
    """A synchronous clone runs the jobs' code in a transient workspace of its own. First in this
    file, so the engine's job workspace is the 2 frames reserved here: the 5-frame synchronous clone
    (two full chunks of 2 frames and a one-frame remainder) between two jobs, none of them waited
    for, is larger than it and must neither alias, free nor resize it."""
    cases = _cases()
    gpu_engine.reserve_voice_jobs(2)
    a = gpu_engine.voice_job(*cases["one_frame_24k"][:2])
    x, sr, chunk, rule, ochunk, frames = cases["five_frames_48k"]
    b = gpu_engine.voice_from_audio(x, sr, chunk, resampler=rule)
    assert b.ready() and b.n_frames == frames
    c = gpu_engine.voice_job(*cases["padded_last_frame"][:2])
    conds = [_oracle_cond(oracle, *cases["one_frame_24k"][:2]), _oracle_cond(oracle, x, sr, ochunk),
             _oracle_cond(oracle, *cases["padded_last_frame"][:2])]
    for name, v, cond in zip("abc", (a, b, c), conds):
        err = float(np.abs(v.conditioning() - cond).max())
        print(f"{name}: {v.n_frames} frames, conditioning max |d| {err:.3g}")
        assert err <= 1e-5, (name, err)
    for v, cond in zip((a, b, c), conds):
        _check_generation(gpu_engine, oracle, v, cond)
        v.close()


@pytest.mark.parametrize("case", ["one_frame_24k", "padded_last_frame", "ref_wav_i16_48k", "chunked_5f", "rubato_48k"])
def test_voice_job_matches_oracle(gpu_engine, oracle, case):
    x, sr, chunk, rule, ochunk, frames = _cases()[case]
    v = gpu_engine.voice_job(x, sr, chunk, resampler=rule)
    assert v.n_frames == frames  # valid as soon as the job is started
    cond = _oracle_cond(oracle, x, sr, ochunk, rubato=rule == "rubato")
    assert cond.shape[0] == frames
    got = v.conditioning()
    assert v.ready()
    err = float(np.abs(got - cond).max())
    print(f"{case}: conditioning max |d| {err:.3g}")
    assert err <= 1e-5, err
    if case == "chunked_5f":  # the reference's own fixture, and the chunk quirk is exercised
        d = load_golden("encoder_chunked_5f.safetensors")
        np.testing.assert_allclose(got, d["conditioning"], atol=1e-5)
        assert np.abs(got - _oracle_cond(oracle, x, sr, -1)).max() > 1e-4
    _check_generation(gpu_engine, oracle, v, cond)
    v.close()


def test_voice_job_int16_ingest_equals_float32(gpu_engine):
    x = _ref13()
    a = gpu_engine.voice_job(x, 48000)
    b = gpu_engine.voice_job(x.astype(np.float32) / np.float32(32768.0), 48000)
    c = gpu_engine.voice_from_audio(x.astype(np.float32) / np.float32(32768.0), 48000)
    ca, cb = a.conditioning(), b.conditioning()
    np.testing.assert_array_equal(ca, cb)
    np.testing.assert_array_equal(ca, c.conditioning())  # the job sees the synchronous call's numbers
    for v in (a, b, c):
        v.close()


def test_rubato_job_above_four_times_the_model_rate(gpu_engine):
    """The converted clip of the rubato rule is sized from the clip, not from the workspace: a
    192 kHz clip is accepted whatever was cloned before, as voice_from_audio accepts it."""
    x = (0.2 * np.random.default_rng(4).standard_normal(8 * 1920 + 40)).astype(np.float32)
    a = gpu_engine.voice_job(x, 192000, -1, resampler="rubato")
    b = gpu_engine.voice_from_audio(x, 192000, -1, resampler="rubato")
    assert a.n_frames == b.n_frames == 2
    np.testing.assert_array_equal(a.conditioning(), b.conditioning())
    a.close()
    b.close()


def _pipelined_run(oracle, with_job):
    """Rows 0-3 generate 12 frames on a pipelined engine (back_frames=2, 6 slots); after call 4,
    row 4 is admitted with a 13-frame voice: a job started right there and never waited for
    (with_job), or the same clip cloned synchronously before the first call."""
    import pocket_tts_amd as pt

    rng = np.random.default_rng(5)
    prompt = (0.11 * rng.standard_normal((6, 1024))).astype(np.float32)
    ids = [np.array([260, 2994, 262 + r, 578, 682][: 3 + r % 3], np.int32) for r in range(4)]
    eng = pt.Engine(device=0, max_slots=6, max_ctx=512, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=2)
    try:
        v0 = eng.voice_from_prompt(prompt)
        v4 = None if with_job else eng.voice_from_audio(_ref13().astype(np.float32) / np.float32(32768.0), 48000)
        eng.open_many([0, 1, 2, 3], [v0] * 4, ids, [_params(12)] * 4)
        frames = {r: [] for r in range(5)}
        for call in range(40):
            if call == 4:
                if with_job:
                    v4 = eng.voice_job(_ref13(), 48000)
                eng.open(4, v4, IDS, _params(6))  # same pass: no ready(), no host wait
            r = eng.step(6)
            for row in range(5):
                if r.valid[row]:
                    frames[row].append((r.latents[row].copy(), r.pcm[row].copy(), float(r.eos_logits[row])))
            if all(len(frames[row]) == 12 for row in range(4)) and len(frames[4]) == 6:
                break
        cond = v4.conditioning()
        v4.close()
        v0.close()
        return frames, cond
    finally:
        eng.close()


def test_admission_behind_pending_job_no_host_wait(oracle):
    with_job, cond = _pipelined_run(oracle, True)
    baseline, cond_sync = _pipelined_run(oracle, False)
    assert [len(with_job[r]) for r in range(5)] == [12, 12, 12, 12, 6]
    assert [len(baseline[r]) for r in range(5)] == [12, 12, 12, 12, 6]
    for row in range(4):  # the job touched nothing of theirs: bit-identical
        for i in range(12):
            np.testing.assert_array_equal(with_job[row][i][0], baseline[row][i][0])
            np.testing.assert_array_equal(with_job[row][i][1], baseline[row][i][1])
            assert with_job[row][i][2] == baseline[row][i][2]
    ocond = _oracle_cond(oracle, _ref13(), 48000)
    assert np.abs(cond - ocond).max() <= 1e-5
    np.testing.assert_array_equal(cond, cond_sync)
    refs = _oracle_frames(oracle, ocond, IDS, 6)
    for i in range(6):
        lat, pcm, eos = with_job[4][i]
        assert np.abs(lat - refs[i]["latent"]).max() <= LAT_TOL, i
        assert abs(eos - refs[i]["eos_logit"]) <= LAT_TOL, i
        assert pcm_err(pcm - refs[i]["pcm"]) <= PCM_TOL, i


def test_back_to_back_jobs_share_the_workspace_in_order(oracle):
    """3, 13 and 1 frames with no waits in between, on an engine that has reserved nothing: the
    second job grows the workspace under the first."""
    import pocket_tts_amd as pt

    rng = np.random.default_rng(17)
    clips = [(0.1 * rng.standard_normal(1920 * 3).astype(np.float32), 24000), (_ref13(), 48000),
             (0.1 * rng.standard_normal(1000).astype(np.float32), 24000)]
    eng = pt.Engine(device=0, max_slots=1, max_ctx=512, lsd_decode_steps=1, seed=0x5EED)
    try:
        voices = [eng.voice_job(x, sr) for x, sr in clips]
        assert [v.n_frames for v in voices] == [3, 13, 1]
        for v, (x, sr) in zip(voices, clips):
            err = float(np.abs(v.conditioning() - _oracle_cond(oracle, x, sr)).max())
            assert err <= 1e-5, (v.n_frames, err)
        # the caches too: generate from the first (written while the workspace was about to grow)
        _check_generation(eng, oracle, voices[0], _oracle_cond(oracle, *clips[0]))
        _check_generation(eng, oracle, voices[2], _oracle_cond(oracle, *clips[2]))
        for v in voices:
            v.close()
    finally:
        eng.close()


@pytest.mark.parametrize("rows", [21, 70, 300])
def test_prompt_job_matches_voice_from_prompt(gpu_engine, rows):
    """One size per GEMM path of the prefill (linear_split): <= 64 rows (register-resident weights),
    65 .. 255 (split-K slabs), >= 256 (whole-K tiles with the split tail: the job's own tail scratch
    and tickets)."""
    prompt = (0.11 * np.random.default_rng(rows).standard_normal((rows, 1024))).astype(np.float32)
    outs = []
    for make in (gpu_engine.voice_from_prompt, gpu_engine.voice_job_prompt):
        v = make(prompt)
        assert v.n_frames == rows
        gpu_engine.open(0, v, IDS, _params(3))
        outs.append([gpu_engine.step(1) for _ in range(3)])
        gpu_engine.close_slot(0)
        v.close()
    for a, b in zip(*outs):
        assert a.valid[0] and b.valid[0]
        assert np.abs(a.latents[0] - b.latents[0]).max() <= LAT_TOL
        assert abs(float(a.eos_logits[0]) - float(b.eos_logits[0])) <= LAT_TOL
        assert pcm_err(a.pcm[0] - b.pcm[0]) <= PCM_TOL


def test_voice_job_lifetime(gpu_engine, oracle):
    x = _ref13()
    v = gpu_engine.voice_job(x, 48000)
    v.close()  # pending: returns cleanly (waits for the job, frees the voice)
    assert v.handle is None
    w = gpu_engine.voice_job(x, 48000)
    gpu_engine.open(0, w, IDS, _params(2))
    w.close()  # evicted while slot 0 reads it: lives on until the slot lets go
    refs = _oracle_frames(oracle, _oracle_cond(oracle, x, 48000), IDS, 2)
    for i in range(2):
        r = gpu_engine.step(1)
        assert r.valid[0]
        assert np.abs(r.latents[0] - refs[i]["latent"]).max() <= LAT_TOL, i
        assert pcm_err(r.pcm[0] - refs[i]["pcm"]) <= PCM_TOL, i
    gpu_engine.close_slot(0)


def test_voice_job_argument_errors(gpu_engine, oracle):
    import ctypes as C

    from pocket_tts_amd import PocketTTSError
    from pocket_tts_amd._lib import check, lib

    x = np.zeros(1920, np.float32)
    with pytest.raises(PocketTTSError):
        gpu_engine.voice_job(x, 0)
    with pytest.raises(PocketTTSError):
        gpu_engine.voice_job(x[:0], 24000)
    with pytest.raises(PocketTTSError):
        gpu_engine.voice_job(np.zeros(1920 * 512, np.float32), 24000)  # max_ctx frames
    with pytest.raises(PocketTTSError):
        gpu_engine.voice_job_prompt(np.zeros((512, 1024), np.float32))
    with pytest.raises(PocketTTSError):
        gpu_engine.reserve_voice_jobs(512)
    h = C.c_void_p()
    with pytest.raises(PocketTTSError):  # unknown sample format
        check(lib().ptts_voice_job_start(gpu_engine.handle, x.ctypes.data_as(C.c_void_p), x.size, 7, 24000, 0, 0,
                                         C.byref(h)))
    assert h.value is None  # a rejected job returns no handle
    with pytest.raises(ValueError):
        gpu_engine.voice_job(x, 24000, resampler="sinc")
    # the engine still generates
    clip = 0.1 * np.random.default_rng(2).standard_normal(1920).astype(np.float32)
    gpu_engine.reserve_voice_jobs(16)
    v = gpu_engine.voice_job(clip, 24000)
    _check_generation(gpu_engine, oracle, v, _oracle_cond(oracle, clip, 24000))
    v.close()
