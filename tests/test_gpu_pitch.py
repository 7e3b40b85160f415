"""Per-request pitch (ptts_pitch_enable / ptts_slot_opts.pitch_cents): the GPU
pitch stage against its host restatement audio.pitch_resample, bit for bit. The whole-signal seam
first (Engine.pitch_resample), then rows that differ in (pitch, speed, rate, encoding) in one batch:
a pitch row's chunks, concatenated, are the host pipeline over the row's own f32 frames
(tempo_wsola at sp_w, pitch_resample, Engine.resample, the numpy encoder / the FLAC decoder), each
frame's byte count is the chunk-size function, and everything else equals an engine without the
stage, whose plan is the parent commit's (tests/golden/plan_ops_before_pitch.json).

Small engines: 8 slots, synthetic weights, temp 0, EOS off, 5 frames a row and one row of one."""

import json
from pathlib import Path

import numpy as np
import pytest

import flac_decode as fd
from test_gpu_tempo import signal
from test_gpu_wire import BYTES, INF, drive, expected_chunks, make_voice, np_encode, np_s16

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "plan_ops_before_pitch.json"
SEAM_CENTS = [-1200, -350, 1, 700, 1200]
# (sample_rate, encoding, speed permille, cents) per row; None: no format. Row 2 has a pitch and
# neither speed nor format (24000 / 16 bit implied), row 3 a speed and no pitch, row 1 a format
# only, row 0 nothing; row 7 (one frame) has sp_w = 1000: its resampler reads the PCM frames.
ROWS = [None, (24000, "pcm_s16le", None, None), (None, None, None, 400), (48000, "pcm_s16le", 800, None),
        (48000, "pcm_s16le", 600, -700), (8000, "ulaw", 1250, 700), (16000, "flac", None, -350),
        (44100, "alaw", 500, -1200)]
FRAMES = [5, 5, 5, 5, 5, 5, 5, 1]
MODES = [(True, 1), (True, 4), (False, 1)]  # (pipeline, back_frames)


def params(max_frames, row, pitch=True):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1)
    if row:
        p.sample_rate, p.encoding = row[0], row[1]
        p.speed = None if row[2] is None else row[2] / 1000.0
        p.pitch = None if row[3] is None or not pitch else row[3] / 100.0
    return p


def engine(mode=(True, 1), pitch=True, slots=8, wire=True, tempo=True):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=mode[0],
                     back_frames=mode[1], wire=wire, tempo=tempo, flac=wire, pitch=pitch)


def admit(eng, rows, frames, voice, slots=None, pitch=True):
    slots = list(range(len(rows))) if slots is None else slots
    rng = np.random.default_rng(5)
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], rows[i], pitch) for i in range(len(slots))])


def host_pipeline(eng, pcm_frames, row):
    """(samples at the wire rate, per-frame sample counts) of a pitch row by the host rule over its
    f32 frames: tempo_wsola at sp_w, pitch_resample, Engine.resample"""
    from pocket_tts_amd.audio import (pitch_chunk_samples, pitch_len, pitch_plan, pitch_resample, tempo_chunk_samples,
                                      tempo_len, tempo_wsola)

    rate, _, sp, cents = row
    rate = rate or 24000
    sp_w, step = pitch_plan(cents, sp or 0)
    n = len(pcm_frames)
    x = np.concatenate(pcm_frames)
    y = x if sp_w == 1000 else tempo_wsola(x, sp_w)
    z = pitch_resample(y, step)
    assert len(z) == pitch_len(len(y), step) == eng.pitch_len(tempo_len(len(x), sp_w), step)
    w = z if rate == 24000 else eng.resample(z, 24000, rate)
    g = np.gcd(24000, rate)
    up, down = rate // g, 24000 // g
    half = 10 * max(up, down)
    sizes, t_seen, seen, out = [], 0, 0, 0
    for f in range(n):
        last = f == n - 1
        t_next = t_seen + (1920 if sp_w == 1000 else tempo_chunk_samples(f, sp_w, last))
        seen += pitch_chunk_samples(t_seen, t_next, step, last)
        t_seen = t_next
        if last:
            m = -(-seen * up // down)
        else:
            m = seen if rate == 24000 else (0 if seen == 0 else (seen * up - 1 - half) // down + 1)
        sizes.append(m - out)
        out = m
    assert t_seen == len(y) and seen == len(z) and out == len(w)
    return w, sizes


@pytest.fixture(scope="module")
def seam_engine():
    eng = engine((False, 1), pitch=False, slots=1, wire=False, tempo=False)
    yield eng
    eng.close()


@pytest.mark.parametrize("cents", SEAM_CENTS)
def test_seam_equals_the_host_rule(seam_engine, cents):
    from pocket_tts_amd.audio import pitch_len, pitch_plan, pitch_resample, pitch_support

    step = pitch_plan(cents, 1000 if abs(cents) < 1200 else (2000 if cents > 0 else 500))[1]
    H = pitch_support(step)
    for n in (1, H, 2 * H + 1, 3 * 1920 + 7):
        x = signal(n, seed=n)
        got, want = seam_engine.pitch_resample(x, step), pitch_resample(x, step)
        assert len(got) == len(want) == pitch_len(n, step) == seam_engine.pitch_len(n, step), (cents, n)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{cents} cents, n {n}: {bad.size} samples differ, first at {bad[0]}"


def test_seam_identity(seam_engine):
    x = signal(3 * 1920 + 7, seed=3)
    got = seam_engine.pitch_resample(x, 1 << 20)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


_PLAIN = {}


def plain_run(mode):
    """the batch on an engine without the pitch stage (pitches dropped): the reference of every
    output that must not depend on pitch, computed once per pass shape"""
    if mode not in _PLAIN:
        eng = engine(mode, pitch=False)
        try:
            admit(eng, ROWS, FRAMES, make_voice(eng), pitch=False)
            rec = []
            pcm, wire = drive(eng, 8, FRAMES, record=rec)
            _PLAIN[mode] = (pcm, wire, rec)
        finally:
            eng.close()
    return _PLAIN[mode]


@pytest.mark.parametrize("mode", MODES)
def test_pitch_rows_in_a_mixed_batch(mode):
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
            if row is None or row[3] is None:  # no pitch: the bytes of the engine without the stage
                assert wire[b] == pwire[b], b
                if row and row[2] is None:
                    assert [len(c) for c in wire[b]] == expected_chunks(row[0], row[1], FRAMES[b])
                continue
            assert wire[b] != pwire[b], b
            want, sizes = host_pipeline(eng, pcm[b], row)
            rate, enc = row[0] or 24000, row[1] or "pcm_s16le"
            print(f"mode {mode} row {b} {row}: chunks {[len(c) for c in wire[b]]}, samples {sizes}")
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
    (the fixture was written by the parent's library); an engine with the stage adds `pitch`."""
    import pocket_tts_amd as pt

    want = json.loads(GOLDEN.read_text())
    kinds = {"sequential": dict(pipeline=False),
             "pipelined_pair": dict(pipeline=True, back_frames=2),
             "pipelined_four_wire_tempo": dict(pipeline=True, back_frames=4, wire=True, tempo=True)}
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
        assert ops.index("tempo") + 1 == ops.index("pitch") == ops.index("wire") - 1
        assert [o for o in ops if o != "pitch" and o != "flac"] == want["pipelined_four_wire_tempo"]
    finally:
        eng.close()


def test_slot_readmitted_with_another_pitch_and_cancel():
    """One call in flight: slot 0 runs a 4-frame row at +700 cents and is re-admitted at -1200 cents,
    48 kHz, while the pass over its last frame is unfetched; the new row starts from a zero count and
    its bytes equal a fresh engine's. Then the row is cancelled mid-utterance: no byte of it arrives."""
    old, new, nf = (8000, "ulaw", 1250, 700), (48000, "pcm_s16le", 700, -1200), 4
    fresh = engine((True, 2), slots=1)
    try:
        admit(fresh, [new], [nf], make_voice(fresh))
        _, want = drive(fresh, 1, [nf])
    finally:
        fresh.close()
    eng = engine((True, 2), slots=1)
    try:
        v = make_voice(eng)
        admit(eng, [old], [nf], v)
        old_pcm, old_wire, new_wire = [], [], []

        def take():
            r, w = eng.fetch(1, calls_back=1), eng.fetch_wire(1, calls_back=1)
            if not r.valid[0]:
                assert w[0] == b""
            elif len(old_pcm) < nf:
                old_pcm.append(r.pcm[0].copy())
                old_wire.append(w[0])
            else:
                new_wire.append(w[0])

        for k in range(nf + 1):
            eng.step_async(1)
            if k:
                take()
        assert len(old_pcm) < nf
        admit(eng, [new], [nf], v)
        for _ in range(32):
            if len(new_wire) == nf:
                break
            eng.step_async(1)
            take()
        assert len(old_pcm) == nf
        assert new_wire == want[0]
        assert b"".join(old_wire) == np_encode(host_pipeline(eng, old_pcm, old)[0], old[1])
        admit(eng, [new], [12], v)
        for _ in range(5):
            eng.step_async(1)
        eng.cancel_slots([0])
        for _ in range(10):
            eng.step_async(1)
            assert eng.fetch_wire(1) == [b""] and not eng.fetch(1).valid[0]
    finally:
        eng.close()


def test_refusals_admit_nothing():
    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import check, lib

    no_stage = engine(pitch=False, slots=2)
    staged = engine(slots=2)
    try:
        # (engine, speed permille, cents): out of range, sp_w out of range both ways, no stage
        for eng, sp, cents in ((staged, None, 1201), (staged, None, -1201), (staged, 600, 700), (staged, 1800, -700),
                               (no_stage, None, 100)):
            with pytest.raises(pt.PocketTTSError) as e:  # row 0 is a good row of the same call
                admit(eng, [(24000, "pcm_s16le", None, None), (24000, "pcm_s16le", sp, cents)], [2, 2], make_voice(eng))
            assert e.value.code == 1, (sp, cents)
            for _ in range(3):
                eng.step_async(2)
                assert not eng.fetch(2).valid.any(), (sp, cents)  # nothing was admitted
        with pytest.raises(pt.PocketTTSError) as e:  # after the first step
            check(lib().ptts_pitch_enable(no_stage.handle, 1))
        assert e.value.code == 1
        with pytest.raises(pt.PocketTTSError):  # not tempo-enabled
            engine(slots=1, tempo=False)
        admit(staged, [(24000, "pcm_s16le", None, 100)], [2], make_voice(staged))  # and a good one still admits
        _, wire = drive(staged, 1, [2])
        assert all(wire[0])
    finally:
        no_stage.close()
        staged.close()
