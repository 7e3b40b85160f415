"""Per-request volume (ptts_level_enable / ptts_slot_opts.gain_cdb, .limit): the
GPU level stage against its host restatement audio.level_limit, bit for bit. The whole-signal seam
first (Engine.level), then rows that differ in (gain, limit, speed, pitch, rate, encoding) in one
batch: a level row's chunks, concatenated, are the host pipeline over the row's own f32 frames
(tempo_wsola, pitch_resample, level_limit, Engine.resample, the numpy encoder / the FLAC decoder),
each frame's byte count is the chunk-size functions composed, and everything else equals an engine
without the stage, whose plan is the parent commit's (tests/golden/plan_ops_before_level.json).

The synthetic-weight PCM peaks near 0.053, so the engines' ceiling is -26 dBFS (0.0501): the test
asserts by the host rule that the limiter engages in every frame of every row with a gain >= 0.

Small engines: 8 slots, synthetic weights, temp 0, EOS off, 5 frames a row and one row of one."""

import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import flac_decode as fd
from test_gpu_tempo import signal
from test_gpu_wire import BYTES, INF, drive, expected_chunks, make_voice, np_encode, np_s16

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "plan_ops_before_level.json"
CEILING_CDB = -2600
SEAM_SIZES = [1, 126, 127, 253, 3 * 1920 + 7]
SEAM_PLANS = [(0, -100), (600, -100), (2400, 0), (-600, -2600)]  # (gain, ceiling) in hundredths of a dB
# (sample_rate, encoding, speed permille, cents, gain cdB, limit) per row; None: nothing at all. Row 1
# has a format only, row 2 `limit` only (24000 / 16 bit implied), row 5 a negative gain (pure gain
# through the stage), row 7 is the one-frame row.
ROWS = [None, (24000, "pcm_s16le", None, None, 0, False), (None, None, None, None, 0, True),
        (48000, "pcm_s16le", None, None, 200, False), (48000, "pcm_s16le", 600, -700, 200, False),
        (8000, "ulaw", 1250, None, -600, False), (16000, "flac", None, None, 200, False),
        (44100, "alaw", None, None, 0, True)]
FRAMES = [5, 5, 5, 5, 5, 5, 5, 1]
MODES = [(True, 1), (True, 4), (False, 1)]  # (pipeline, back_frames)


def in_stage(row):
    return bool(row) and (row[4] != 0 or row[5])


def params(max_frames, row, level=True):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1)
    if row:
        p.sample_rate, p.encoding = row[0], row[1]
        p.speed = None if row[2] is None else row[2] / 1000.0
        p.pitch = None if row[3] is None else row[3] / 100.0
        if level:
            p.volume_db, p.limit = row[4] / 100.0, row[5]
    return p


def engine(mode=(True, 1), level=True, slots=8):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=mode[0],
                     back_frames=mode[1], wire=True, tempo=True, flac=True, pitch=True, level=level,
                     level_ceiling_db=CEILING_CDB / 100.0)


def admit(eng, rows, frames, voice, slots=None, level=True):
    slots = list(range(len(rows))) if slots is None else slots
    rng = np.random.default_rng(5)
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], rows[i], level) for i in range(len(slots))])


def host_pipeline(eng, pcm_frames, row, last=True):
    """(samples at the wire rate, per-frame sample counts, the level stage's per-frame inputs) of a level
    row by the host rule over its f32 frames: tempo_wsola, pitch_resample, level_limit, Engine.resample.
    last=False: the frames are the first of a longer utterance (no frame is its last)."""
    from pocket_tts_amd.audio import (level_chunk_samples, level_limit, pitch_chunk_samples, pitch_plan, pitch_resample,
                                      tempo_chunk_samples, tempo_wsola)

    rate, _, sp, cents, gain, _ = row
    rate = rate or 24000
    sp_w, step = pitch_plan(cents, sp or 0) if cents else (sp or 1000, None)
    n = len(pcm_frames)
    x = np.concatenate(pcm_frames)
    y = x if sp_w == 1000 else tempo_wsola(x, sp_w)
    z = pitch_resample(y, step) if cents else y
    lv = level_limit(z, gain, CEILING_CDB)
    w = lv if rate == 24000 else eng.resample(lv, 24000, rate)
    g = np.gcd(24000, rate)
    up, down = rate // g, 24000 // g
    half = 10 * max(up, down)
    sizes, inputs, t_seen, p_seen, l_seen, out = [], [], 0, 0, 0, 0
    for f in range(n):
        end = last and f == n - 1
        t_next = t_seen + (1920 if sp_w == 1000 else tempo_chunk_samples(f, sp_w, end))
        p_next = p_seen + (pitch_chunk_samples(t_seen, t_next, step, end) if cents else t_next - t_seen)
        l_seen += level_chunk_samples(p_seen, p_next, end)
        inputs.append(z[p_seen:p_next])
        t_seen, p_seen = t_next, p_next
        if end:
            m = -(-l_seen * up // down)
        else:
            m = l_seen if rate == 24000 else (0 if l_seen == 0 else (l_seen * up - 1 - half) // down + 1)
        sizes.append(m - out)
        out = m
    if last:
        assert t_seen == len(y) and p_seen == len(z) and l_seen == len(lv) and out == len(w)
    return w, sizes, inputs


def share_over(x, gain):
    from pocket_tts_amd.audio import level_plan

    v, c = level_plan(gain, CEILING_CDB)
    return float((np.abs(v * np.asarray(x, np.float32)) > c).mean())


@pytest.fixture(scope="module")
def seam_engine():
    import pocket_tts_amd as pt

    eng = pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED)
    yield eng
    eng.close()


@pytest.mark.parametrize("gain,ceiling", SEAM_PLANS)
def test_seam_equals_the_host_rule(seam_engine, gain, ceiling):
    from pocket_tts_amd.audio import level_limit, level_plan

    v, c = level_plan(gain, ceiling)
    for n in SEAM_SIZES:
        x = signal(n, seed=n)
        a = np.abs(x)
        # a fifth of the samples over the ceiling, and a spike at the first and the last index
        x = x * np.float32(float(c) / float(v) / max(float(np.quantile(a, 0.8)), 1e-6))
        x[0], x[-1] = 4 * float(c) / float(v), -4 * float(c) / float(v)
        over = float((np.abs(v * x) > c).mean())
        if n >= 126:
            assert 0.01 <= over <= 0.5, (n, over)
        else:
            assert over > 0
        got = seam_engine.level(x, gain / 100.0, ceiling / 100.0)
        want, u, r, g = level_limit(x, gain, ceiling, detail=True)
        assert got.size == want.size == n and np.abs(want).max() <= c and (g < 1).any()
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"gain {gain} ceiling {ceiling}, n {n}: {bad.size} samples differ, first at {bad[0]}"


def test_seam_pure_gain(seam_engine):
    from pocket_tts_amd.audio import level_plan

    x = signal(3 * 1920 + 7, seed=3)
    for gain in (0, 600, -2400):
        v, _ = level_plan(gain, 0)
        got = seam_engine.level(0.1 * x, gain / 100.0, 0.0)
        assert np.array_equal(got.view(np.uint32), (v * (np.float32(0.1) * x)).astype(np.float32).view(np.uint32))


_PLAIN = {}


def plain_run(mode):
    """the batch on an engine without the level stage (the fields dropped): the reference of every
    output that must not depend on them, computed once per pass shape"""
    if mode not in _PLAIN:
        eng = engine(mode, level=False)
        try:
            admit(eng, ROWS, FRAMES, make_voice(eng), level=False)
            rec = []
            pcm, wire = drive(eng, 8, FRAMES, record=rec)
            _PLAIN[mode] = (pcm, wire, rec)
        finally:
            eng.close()
    return _PLAIN[mode]


@pytest.mark.parametrize("mode", MODES)
def test_level_rows_in_a_mixed_batch(mode):
    from pocket_tts_amd.audio import level_limit

    eng = engine(mode)
    try:
        admit(eng, ROWS, FRAMES, make_voice(eng))
        rec = []
        pcm, wire = drive(eng, 8, FRAMES, record=rec)
        ppcm, pwire, prec = plain_run(mode)
        # f32 PCM, flags, EOS logits and latents of every call: those of the engine without the stage
        assert len(rec) == len(prec)
        for a, b in zip(rec, prec):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        for b, row in enumerate(ROWS):
            assert len(pcm[b]) == FRAMES[b]
            if not in_stage(row):  # no level field: the bytes of the engine without the stage
                assert wire[b] == pwire[b], b
                if row:
                    assert [len(c) for c in wire[b]] == expected_chunks(row[0], row[1], FRAMES[b])
                continue
            assert wire[b] != pwire[b], b
            want, sizes, inputs = host_pipeline(eng, pcm[b], row)
            rate, enc, gain = row[0] or 24000, row[1] or "pcm_s16le", row[4]
            shares = [share_over(x, gain) for x in inputs]
            print(f"mode {mode} row {b} {row}: chunks {[len(c) for c in wire[b]]}, samples {sizes}, "
                  f"over the ceiling {[round(s, 4) for s in shares]}")
            if gain >= 0:  # the limiter engages in every frame, on both sides of every chunk boundary
                assert all(0.005 <= s <= 0.6 for s in shares), (b, shares)
            else:  # pure gain through the stage
                z = np.concatenate(inputs)
                y, u, r, g = level_limit(z, gain, CEILING_CDB, detail=True)
                assert (g == 1).all() and np.array_equal(y, u)
            if enc == "flac":  # the decoded samples instead of the byte count
                at = 0
                for chunk, size in zip(wire[b], sizes):
                    s, info = fd.decode_frames(chunk, rate) if chunk else (np.zeros(0, np.int16), [])
                    assert s.size == size and (not info or info[0][0] == at), (b, at, s.size, size)
                    assert np.array_equal(s, np_s16(want[at:at + size])), (b, at)
                    at += size
                assert at == len(want)
                continue
            assert [len(c) for c in wire[b]] == [s * BYTES[enc] for s in sizes], (b, row)
            got, ref = b"".join(wire[b]), np_encode(want, enc)
            assert len(got) == len(ref), (b, row, len(got), len(ref))
            if got != ref:
                g, w = np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8)
                bad = np.flatnonzero(g != w)
                raise AssertionError(f"row {b} {row}: {bad.size} bytes differ, first at {bad[0]}")
    finally:
        eng.close()


def test_plan_of_an_engine_without_the_stage_is_the_parents():
    """Engine.plan_ops(8) of engines that do not enable the stage: the text the parent commit returns
    (the fixture was written by the parent's library); an engine with the stage adds `level`."""
    import pocket_tts_amd as pt

    want = json.loads(GOLDEN.read_text())
    kinds = {"sequential": dict(pipeline=False),
             "pipelined_pair": dict(pipeline=True, back_frames=2),
             "pipelined_four_wire_tempo": dict(pipeline=True, back_frames=4, wire=True, tempo=True),
             "pipelined_four_wire_tempo_pitch_flac": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                          pitch=True, flac=True)}
    assert sorted(want) == sorted(kinds)
    for name, kw in kinds.items():
        eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, **kw)
        try:
            assert eng.plan_ops(8) == want[name], name
        finally:
            eng.close()
    eng = engine((True, 4))
    try:
        ops = eng.plan_ops(8)
        assert ops.index("pitch") + 1 == ops.index("level") == ops.index("wire") - 1
        assert [o for o in ops if o != "level"] == want["pipelined_four_wire_tempo_pitch_flac"]
    finally:
        eng.close()
    eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=4,
                    wire=True, level=True)  # independent of the tempo and pitch stages
    try:
        ops = eng.plan_ops(8)
        assert ops.index("level") == ops.index("wire") - 1 and "tempo" not in ops and "pitch" not in ops
    finally:
        eng.close()


def test_slot_cancelled_and_readmitted_with_another_gain():
    """One call in flight: slot 0 runs a +2 dB row, is cancelled after two delivered frames and
    re-admitted at once with +4 dB at 48 kHz while the old pass is unfetched. The new row starts from
    a zero count and an empty history: its bytes equal a fresh engine's. The old row's two chunks are
    the first 2 * 1920 - 126 samples of its own host rule."""
    old, new, nf = (24000, "pcm_s16le", None, None, 200, False), (48000, "pcm_s16le", None, None, 400, False), 4
    fresh = engine((True, 2), slots=1)
    try:
        admit(fresh, [new], [nf], make_voice(fresh))
        _, want = drive(fresh, 1, [nf])
    finally:
        fresh.close()
    eng = engine((True, 2), slots=1)
    try:
        v = make_voice(eng)
        admit(eng, [old], [8], v)
        old_pcm, old_wire, new_wire, phase = [], [], [], ["old"]

        def take():
            r, w = eng.fetch(1, calls_back=1), eng.fetch_wire(1, calls_back=1)
            if not r.valid[0]:
                assert w[0] == b""
            elif phase[0] == "old":
                old_pcm.append(r.pcm[0].copy())
                old_wire.append(w[0])
            else:
                new_wire.append(w[0])

        eng.step_async(1)
        for _ in range(32):
            if len(old_pcm) == 2:
                break
            eng.step_async(1)
            take()
        assert len(old_pcm) == 2
        eng.cancel_slots([0])  # with the pass over the row's later frames in flight
        phase[0] = "new"
        admit(eng, [new], [nf], v)
        for _ in range(32):
            if len(new_wire) == nf:
                break
            eng.step_async(1)
            take()
        assert new_wire == want[0]
        ref, sizes, _ = host_pipeline(eng, old_pcm, old, last=False)
        assert sizes == [1920 - 126, 1920] and [len(c) for c in old_wire] == [2 * s for s in sizes]
        assert b"".join(old_wire) == np_encode(ref[:sum(sizes)], "pcm_s16le")
    finally:
        eng.close()


def test_refusals_admit_nothing():
    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import WIRE_CHUNK_MAX_LEVEL, WIRE_CHUNK_MAX_TEMPO, check, lib, u8ptr

    no_stage = engine(level=False, slots=2)
    staged = engine(slots=2)
    try:
        # (engine, gain cdB, limit): out of range both ways, limit 2, no stage
        for eng, gain, limit in ((staged, 2401, False), (staged, -2401, False), (staged, 0, 2), (staged, 300, 2),
                                 (no_stage, 100, False), (no_stage, 0, True)):
            with pytest.raises(pt.PocketTTSError) as e:  # row 0 is a good row of the same call
                admit(eng, [(24000, "pcm_s16le", None, None, 0, False), (24000, "pcm_s16le", None, None, gain, limit)],
                      [2, 2], make_voice(eng))
            assert e.value.code == 1, (gain, limit)
            for _ in range(3):
                eng.step_async(2)
                assert not eng.fetch(2).valid.any(), (gain, limit)  # nothing was admitted
        with pytest.raises(pt.PocketTTSError) as e:  # after the first step
            check(lib().ptts_level_enable(no_stage.handle, 1, -100))
        assert e.value.code == 1
        for bad in (1, -4001):  # the ceiling's range
            with pytest.raises(ValueError):
                pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, wire=True, level=True,
                          level_ceiling_db=bad / 100.0)
            with pytest.raises(pt.PocketTTSError) as e:
                check(lib().ptts_level_enable(staged.handle, 1, bad))
            assert e.value.code == 1
        with pytest.raises(pt.PocketTTSError):  # not wire-enabled
            pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, level=True)
        # a level-enabled engine's chunk slots: the stride of ptts_fetch_wire
        buf, nb = np.zeros((2, WIRE_CHUNK_MAX_LEVEL), np.uint8), np.zeros(2, np.int32)
        with pytest.raises(pt.PocketTTSError):
            check(lib().ptts_fetch_wire(staged.handle, 0, 2, u8ptr(buf), WIRE_CHUNK_MAX_TEMPO,
                                        nb.ctypes.data_as(C.POINTER(C.c_int))))
        admit(staged, [(24000, "pcm_s16le", None, None, 100, True)], [2], make_voice(staged))  # a good one still admits
        _, wire = drive(staged, 1, [2])
        assert [len(c) for c in wire[0]] == [2 * (1920 - 126), 2 * (1920 + 126)]
    finally:
        no_stage.close()
        staged.close()


def test_tts_model_returns_level_bytes():
    """TTSModel.generate / generate_stream with volume_db / limit: bytes, the host rule over what
    generate returns without them (temp 0: the same PCM); 0 dB with no limit is the f32 result."""
    import pocket_tts_amd as pt
    from pocket_tts_amd.audio import level_limit

    eng = engine((True, 2), slots=1)
    try:
        m = pt.TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None)
        v = make_voice(eng)
        ids = np.array([260, 2994, 262, 578], np.int32)
        x = m.generate(ids, v, max_frames=4)
        assert x.dtype == np.float32 and x.shape == (1, 4 * 1920)
        same = m.generate(ids, v, max_frames=4, volume_db=0.0)
        assert isinstance(same, np.ndarray) and np.array_equal(same, x)
        got = m.generate(ids, v, max_frames=4, volume_db=2.0)
        want = level_limit(x[0], 200, CEILING_CDB)
        assert 0.005 <= share_over(x[0], 200) <= 0.6
        assert isinstance(got, bytes) and got == np_encode(want, "pcm_s16le")
        chunks = list(m.generate_stream(ids, v, max_frames=4, limit=True, encoding="ulaw"))
        assert [len(c) for c in chunks] == [1920 - 126, 1920, 1920, 1920 + 126]
        assert b"".join(chunks) == np_encode(level_limit(x[0], 0, CEILING_CDB), "ulaw")
    finally:
        eng.close()
