"""The loudness stage (ptts_loud_enable / ptts_slot_opts.loud) on the GPU against
its host restatement audio.loudness_blocks, bit for bit as f64. The whole-signal seam first
(Engine.loudness_blocks), then a batch of rows that differ in what the wire stage reads (a gain, a
speed and a pitch, nothing, and an unmetered row): a metered row's per-call energies are the host
rule over the row's own stage input, rebuilt from its f32 frames (tempo_wsola, pitch_resample,
level_limit), in the same per-frame groups; everything else equals an engine without the stage,
whose plan is the parent commit's (tests/golden/plan_ops_before_loud.json).

Small engines: 4 slots, synthetic weights, temp 0, EOS off, 8 frames a row."""

import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from test_gpu_tempo import signal
from test_gpu_wire import INF, make_voice

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "plan_ops_before_loud.json"
CEILING_CDB = -2600  # the synthetic-weight PCM peaks near 0.053: the limiter engages at +6 dB
SEAM_SIZES = [2399, 2400, 2401, 4831, 12000]
# (speed permille, cents, gain cdB, metered) per row
ROWS = [(None, None, 600, True), (800, 400, None, True), (None, None, None, True), (None, None, None, False)]
NF = 8
MODES = [1, 4]  # back_frames


def params(max_frames, row, loud=True):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=max_frames,
                         seed=1, sample_rate=24000, encoding="pcm_s16le")
    sp, cents, gain, metered = row
    p.speed = None if sp is None else sp / 1000.0
    p.pitch = None if cents is None else cents / 100.0
    p.volume_db = None if gain is None else gain / 100.0
    p.loudness = bool(loud and metered)
    return p


def engine(back_frames=1, loud=True, slots=4):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True,
                     back_frames=back_frames, wire=True, tempo=True, pitch=True, level=True,
                     level_ceiling_db=CEILING_CDB / 100.0, loud=loud)


def admit(eng, rows, frames, voice, slots=None, loud=True):
    slots = list(range(len(rows))) if slots is None else slots
    rng = np.random.default_rng(5)
    ids = [rng.integers(0, 4000, size=3 + b).astype(np.int32) for b in slots]
    eng.open_many(slots, [voice] * len(slots), ids, [params(frames[i], rows[i], loud) for i in range(len(slots))])


def drive(eng, B, frames, loud=True):
    """Step until every row's last frame is fetched. Per row: its f32 frames, wire chunks and
    per-frame energy arrays; and every call's raw outputs."""
    got = [0] * B
    pcm, wire, energy, rec = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)], []
    call = 0
    while any(got[b] < frames[b] for b in range(B)):
        assert call < 64, "the rows never finished"
        eng.step_async(B)
        r = eng.fetch(B)
        w = eng.fetch_wire(B)
        e = eng.fetch_loud(B) if loud else [np.zeros(0)] * B
        rec.append((r.pcm.copy(), r.valid.copy(), r.last.copy(), r.eos_logits.copy(), r.latents.copy(), list(w)))
        for b in range(B):
            if r.valid[b]:
                got[b] += 1
                pcm[b].append(r.pcm[b].copy())
                wire[b].append(w[b])
                energy[b].append(e[b])
            else:
                assert e[b].size == 0, (call, b)
        call += 1
    return pcm, wire, energy, rec


def stage_input(pcm_frames, row, last=True):
    """(the signal the wire stage reads for the row, its per-frame sample counts) by the host rules
    over the row's f32 frames."""
    from pocket_tts_amd.audio import (level_chunk_samples, level_limit, pitch_chunk_samples, pitch_plan,
                                      pitch_resample, tempo_chunk_samples, tempo_wsola)

    sp, cents, gain, _ = row
    sp_w, step = pitch_plan(cents, sp or 0) if cents else (sp or 1000, None)
    x = np.concatenate(pcm_frames)
    y = x if sp_w == 1000 else tempo_wsola(x, sp_w)
    z = pitch_resample(y, step) if cents else y
    out = level_limit(z, gain, CEILING_CDB) if gain is not None else z
    sizes, t_seen, p_seen = [], 0, 0
    for f in range(len(pcm_frames)):
        end = last and f == len(pcm_frames) - 1
        t_next = t_seen + (1920 if sp_w == 1000 else tempo_chunk_samples(f, sp_w, end))
        p_next = p_seen + (pitch_chunk_samples(t_seen, t_next, step, end) if cents else t_next - t_seen)
        sizes.append(level_chunk_samples(p_seen, p_next, end) if gain is not None else p_next - p_seen)
        t_seen, p_seen = t_next, p_next
    if last:
        assert sum(sizes) == out.size
    return out, sizes


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def seam_engine():
    import pocket_tts_amd as pt

    eng = pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED)
    yield eng
    eng.close()


@pytest.mark.parametrize("kind", ["noise", "sine", "step"])
def test_seam_equals_the_host_rule(seam_engine, kind):
    from pocket_tts_amd._lib import lib
    from pocket_tts_amd.audio import kweight_coeffs, loudness_blocks, loudness_tables

    c, pq = np.zeros((2, 5)), np.zeros((2, 2, 32))
    dp = C.POINTER(C.c_double)
    assert lib().ptts_loud_coeffs(c.ctypes.data_as(dp), pq.ctypes.data_as(dp)) == 0
    assert np.array_equal(bits(c), bits(kweight_coeffs(24000.0))) and np.array_equal(bits(pq), bits(loudness_tables(c)))
    for n in SEAM_SIZES:
        if kind == "noise":
            x = signal(n, seed=n)
        elif kind == "sine":
            x = (0.5 * np.sin(2 * np.pi * 997.0 * np.arange(n) / 24000.0)).astype(np.float32)
        else:
            x = np.ones(n, np.float32)
        got, want = seam_engine.loudness_blocks(x), loudness_blocks(x)
        assert got.size == want.size == n // 2400 == lib().ptts_loud_len(n)
        assert got.size == 0 or (want > 0).all()
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"{kind}, n {n}: {bad.size} energies differ, first at {bad[0]}: {got[bad[0]]!r} {want[bad[0]]!r}"


_PLAIN = {}


def plain_run(bf):
    if bf not in _PLAIN:
        eng = engine(bf, loud=False)
        try:
            admit(eng, ROWS, [NF] * 4, make_voice(eng), loud=False)
            _PLAIN[bf] = drive(eng, 4, [NF] * 4, loud=False)
        finally:
            eng.close()
    return _PLAIN[bf]


@pytest.mark.parametrize("bf", MODES)
def test_metered_rows_in_a_mixed_batch(bf):
    from pocket_tts_amd.audio import level_plan, loudness_blocks, loudness_integrated

    eng = engine(bf)
    try:
        admit(eng, ROWS, [NF] * 4, make_voice(eng))
        pcm, wire, energy, rec = drive(eng, 4, [NF] * 4)
        _, pwire, _, prec = plain_run(bf)
        assert len(rec) == len(prec)  # every other output of every call: the engine without the stage
        for a, b in zip(rec, prec):
            for x, y in zip(a[:5], b[:5]):
                assert np.array_equal(x, y)
            assert a[5] == b[5]
        assert wire == pwire
        for b, row in enumerate(ROWS):
            assert len(pcm[b]) == NF
            if not row[3]:
                assert all(e.size == 0 for e in energy[b]), b
                continue
            x, sizes = stage_input(pcm[b], row)
            if row[2] is not None:  # the limiter engaged: the meter reads the level stage's output
                v, c = level_plan(row[2], CEILING_CDB)
                assert 0.9 * c < np.abs(x).max() <= c < v * np.abs(np.concatenate(pcm[b])).max()
            want = loudness_blocks(x, chunks=sizes)
            whole = loudness_blocks(x)
            got = np.concatenate(energy[b])
            print(f"back_frames {bf} row {b} {row}: sizes {sizes}, blocks {[e.size for e in energy[b]]}, "
                  f"{loudness_integrated(got)} LUFS")
            assert whole.size == x.size // 2400 >= 6
            assert [e.size for e in energy[b]] == [w.size for w in want], b
            bad = np.flatnonzero(bits(got) != bits(whole))
            assert bad.size == 0, f"row {b} {row}: {bad.size} energies differ, first at {bad[0]}"
    finally:
        eng.close()


def test_slot_cancelled_and_readmitted_metered():
    """One call in flight: slot 0 runs a metered row, is cancelled after two delivered frames and
    re-admitted metered at once while the old pass is unfetched. The energies that arrive afterwards
    are those of the new utterance alone."""
    from pocket_tts_amd.audio import loudness_blocks

    old, new, nf = (None, None, 600, True), (None, None, None, True), 4
    eng = engine(2, slots=1)
    try:
        v = make_voice(eng)
        admit(eng, [old], [8], v)
        old_n, new_pcm, new_e, phase = [0], [], [], ["old"]

        def take():
            r, e = eng.fetch(1, calls_back=1), eng.fetch_loud(1, calls_back=1)
            if not r.valid[0]:
                assert e[0].size == 0
            elif phase[0] == "old":
                old_n[0] += 1
            else:
                new_pcm.append(r.pcm[0].copy())
                new_e.append(e[0])

        eng.step_async(1)
        for _ in range(32):
            if old_n[0] == 2:
                break
            eng.step_async(1)
            take()
        assert old_n[0] == 2
        eng.cancel_slots([0])  # with the pass over the row's later frames in flight
        phase[0] = "new"
        rng = np.random.default_rng(9)
        eng.open_many([0], [v], [rng.integers(0, 4000, size=5).astype(np.int32)], [params(nf, new)])
        for _ in range(32):
            if len(new_pcm) == nf:
                break
            eng.step_async(1)
            take()
        assert len(new_pcm) == nf
        x, sizes = stage_input(new_pcm, new)
        want = loudness_blocks(x, chunks=sizes)
        assert [e.size for e in new_e] == [w.size for w in want] and sum(e.size for e in new_e) == 3
        assert np.array_equal(bits(np.concatenate(new_e)), bits(np.concatenate(want)))
    finally:
        eng.close()


def test_refusals_admit_nothing_and_a_64_byte_struct_gets_no_meter():
    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import GenParams, SlotOpts5, SlotOpts6, check, lib

    no_stage = engine(loud=False, slots=2)
    staged = engine(slots=2)
    try:
        def raw_open(eng, loud_values, K=SlotOpts6):
            v = make_voice(eng)
            n = len(loud_values)
            ids = np.array([260, 2994, 262] * n, np.int32)
            nid = np.array([3] * n, np.int32)
            sl = np.arange(n, dtype=np.int32)
            vh = (C.c_void_p * n)(*[v.handle] * n)
            ps = (GenParams * n)(*[params(2, (None, None, None, False)).to_c() for _ in range(n)])
            rows = []
            for lv in loud_values:
                o = K(size=C.sizeof(K), lsd_steps=1, wire_rate=24000, wire_encoding=1)
                if K is SlotOpts6:
                    o.loud = lv
                rows.append(o)
            i32 = C.POINTER(C.c_int32)
            return lib().ptts_slots_open_opts(eng.handle, n, sl.ctypes.data_as(i32), vh, ids.ctypes.data_as(i32),
                                              nid.ctypes.data_as(i32), ps, C.cast((K * n)(*rows), C.c_void_p))

        for eng, lv in ((no_stage, 1), (staged, 2), (staged, -1)):  # row 0 is a good row of the same call
            assert raw_open(eng, [0, lv]) == 1, lv
            for _ in range(3):
                eng.step_async(2)
                assert not eng.fetch(2).valid.any(), lv  # nothing was admitted
        with pytest.raises(pt.PocketTTSError) as e:  # after the first step
            check(lib().ptts_loud_enable(no_stage.handle, 1))
        assert e.value.code == 1
        with pytest.raises(pt.PocketTTSError) as e:
            no_stage.fetch_loud(2)
        assert e.value.code == 1
        with pytest.raises(pt.PocketTTSError):  # not wire-enabled
            pt.Engine(device=0, max_slots=1, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, loud=True)
        # the 64-byte struct on the staged engine: admitted, no meter; then the 72-byte one: metered
        for K, blocks in ((SlotOpts5, 0), (SlotOpts6, 1)):
            assert raw_open(staged, [1], K) == 0
            n_blocks, frames = 0, 0
            for _ in range(16):
                staged.step_async(1)
                r = staged.fetch(1)
                n_blocks += staged.fetch_loud(1)[0].size
                frames += int(r.valid[0])
                if r.valid[0] and r.last[0]:
                    break
            assert frames == 2 and n_blocks == blocks, (K.__name__, frames, n_blocks)
    finally:
        no_stage.close()
        staged.close()


def test_plan_of_an_engine_without_the_stage_is_the_parents():
    """Engine.plan_ops(8) of engines that do not enable the stage: the text the parent commit returns
    (the fixture was written by the parent's library); an engine with the stage adds `loud`."""
    import pocket_tts_amd as pt

    want = json.loads(GOLDEN.read_text())
    kinds = {"sequential": dict(pipeline=False),
             "pipelined_pair": dict(pipeline=True, back_frames=2),
             "pipelined_four_wire_tempo": dict(pipeline=True, back_frames=4, wire=True, tempo=True),
             "pipelined_four_wire_tempo_pitch_level": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                           pitch=True, level=True),
             "pipelined_four_wire_tempo_pitch_flac": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                          pitch=True, flac=True)}
    assert sorted(want) == sorted(kinds)
    for name, kw in kinds.items():
        eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, **kw)
        try:
            assert eng.plan_ops(8) == want[name], name
        finally:
            eng.close()
    eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=4,
                    wire=True, tempo=True, pitch=True, level=True, loud=True)
    try:
        ops = eng.plan_ops(8)
        assert ops.index("level") + 1 == ops.index("loud") == ops.index("wire") - 1
        assert [o for o in ops if o != "loud"] == want["pipelined_four_wire_tempo_pitch_level"]
    finally:
        eng.close()
    eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=4,
                    wire=True, loud=True)  # independent of the other stages
    try:
        ops = eng.plan_ops(8)
        assert ops.index("loud") == ops.index("wire") - 1 and not {"tempo", "pitch", "level", "flac"} & set(ops)
    finally:
        eng.close()


def test_tts_model_measures_what_it_returns():
    """TTSModel.generate(.., measure_loudness=True): (audio, lufs); the audio is what generate returns
    without it, the loudness the host rule over that audio's stage input (here the f32 frames, and
    the level stage's output with a gain)."""
    import pocket_tts_amd as pt
    from pocket_tts_amd.audio import level_limit, loudness_blocks, loudness_integrated

    eng = engine(2, slots=1)
    try:
        m = pt.TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None)
        v = make_voice(eng)
        ids = np.array([260, 2994, 262, 578], np.int32)
        x = m.generate(ids, v, max_frames=6)
        got, lufs = m.generate(ids, v, max_frames=6, measure_loudness=True)
        assert isinstance(got, np.ndarray) and np.array_equal(got, x)
        want = loudness_integrated(loudness_blocks(x[0]))
        assert want is not None and lufs == want
        quiet, none = m.generate(ids, v, max_frames=1, measure_loudness=True)  # 1,920 samples: no block
        assert none is None and quiet.shape == (1, 1920)
        by, lufs6 = m.generate(ids, v, max_frames=6, volume_db=6.0, measure_loudness=True)
        assert isinstance(by, bytes) and by == m.generate(ids, v, max_frames=6, volume_db=6.0)
        assert lufs6 == loudness_integrated(loudness_blocks(level_limit(x[0], 600, CEILING_CDB)))
        assert lufs6 != lufs and lufs6 < lufs + 6.0  # the limiter (ceiling -26 dBFS) took more than the gain gave
    finally:
        eng.close()


def test_tts_model_loudness_target():
    """TTSModel.voice_loudness calibrates on the fixed sentence (once per voice), and
    generate(.., loudness_lufs=) applies target - voice loudness as the row's gain with the limiter on."""
    import pocket_tts_amd as pt
    from pocket_tts_amd.audio import level_limit, loudness_blocks, loudness_gain_cdb, loudness_integrated
    from test_gpu_wire import np_encode
    from test_text_frontend import synthetic_tokenizer

    eng = pt.Engine(device=0, max_slots=1, max_ctx=512, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=2,
                    wire=True, level=True, level_ceiling_db=-1.0, loud=True)
    try:
        m = pt.TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None,
                        tokenizer=synthetic_tokenizer())
        v = make_voice(eng)
        cal = m.voice_loudness(v)
        assert cal is not None and -60.0 < cal < -20.0 and m.voice_loudness(v) == cal
        ids = np.array([260, 2994, 262, 578], np.int32)
        x = m.generate(ids, v, max_frames=6)
        gain = loudness_gain_cdb(-30.0, cal)
        assert 0 < gain < 2400
        got, lufs = m.generate(ids, v, max_frames=6, loudness_lufs=-30.0, measure_loudness=True)
        want = level_limit(x[0], gain, -100)
        assert isinstance(got, bytes) and got == np_encode(want, "pcm_s16le")
        assert lufs == loudness_integrated(loudness_blocks(want))
        for bad in (dict(loudness_lufs=-40.5), dict(loudness_lufs=-4.0), dict(loudness_lufs=-16.0, volume_db=1.0)):
            with pytest.raises(ValueError):
                m.generate(ids, v, max_frames=2, **bad)
    finally:
        eng.close()


def test_voice_loudness_is_seeded_on_its_own():
    """At temp 0.7 the noise matters: the calibration row runs with CALIBRATION_SEED, so the value is
    the same whatever the model generated before, and it leaves the model's seed counter alone, so
    the calls after it (and a call with loudness_lufs, which calibrates first) return what they
    return without it."""
    import pocket_tts_amd as pt
    from pocket_tts_amd.audio import level_limit, loudness_gain_cdb
    from test_gpu_wire import np_encode
    from test_text_frontend import synthetic_tokenizer

    eng = pt.Engine(device=0, max_slots=1, max_ctx=512, lsd_decode_steps=1, seed=0x5EED, pipeline=True, back_frames=2,
                    wire=True, level=True, level_ceiling_db=-1.0, loud=True)
    try:
        def model():
            return pt.TTSModel(eng, temp=0.7, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None,
                               tokenizer=synthetic_tokenizer())

        v = make_voice(eng)
        ids = np.array([260, 2994, 262, 578], np.int32)
        plain = model()
        first, second = plain.generate(ids, v, max_frames=4), plain.generate(ids, v, max_frames=4)
        assert not np.array_equal(first, second)  # the seed counter matters at this temperature
        cal = plain.voice_loudness(v)  # after two calls
        assert cal is not None
        m = model()
        assert m.voice_loudness(v) == cal  # before any call: the same value
        assert np.array_equal(m.generate(ids, v, max_frames=4), first)  # and the first call's seed is the first
        assert np.array_equal(m.generate(ids, v, max_frames=4), second)
        m = model()  # a target calibrates first, and returns the first call's audio at the gain
        got = m.generate(ids, v, max_frames=4, loudness_lufs=-30.0)
        assert got == np_encode(level_limit(first[0], loudness_gain_cdb(-30.0, cal), -100), "pcm_s16le")
        assert np.array_equal(m.generate(ids, v, max_frames=4), second)
        # the value is kept with the Voice object: another voice has its own
        other = eng.voice_from_prompt((0.2 * np.random.default_rng(8).standard_normal((4, 1024))).astype(np.float32))
        assert m.voice_loudness(other) != cal and m.voice_loudness(v) == cal
    finally:
        eng.close()
