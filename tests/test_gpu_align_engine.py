"""The align stage in the engine (ptts_align_enable / ptts_slot_opts.align / ptts_fetch_align;
DESIGN.md section 26). Three rows over a 4-frame voice prefix, S = 5 and 12 tokens in the stage and a
third row (S = 7) outside it, 6 frames each, sequential, pipelined and with four-frame passes, with
one voice shared by the rows and with a voice per row.

Layer 0 against float64. Layer 0's q and k are functions of tensors a test can restate (no other
layer's are): the token embedding, input_linear, layer 0's norm1 and in_proj (tests/golden/synth.py)
and the inputs, i.e. the ids and the latents ptts_fetch returned (bos for the first frame). With
x = embed[id] (a key at position F + j) or x = W_in lat (the query of frame t at position F + S + t):
h = LN(x) w + b, (q | k) = W_qk h, rotated at the position, s_j = q . k_j / 8, softmax over the S text
keys, mean over the heads.

Bound: the form of tests/test_gpu_align.py,
    |a_j - ref_j| <= 4 mean_h p_hj (E_hj + sum_k p_hk E_hk) + 8 u,
    E_j = u sum_i |q_i k_ji| + (sum_i dq_i |k_ji| + sum_i |q_i| dk_ji) / 8 + 6 u + 3 u |s_j - max s|,
where dq and dk, the f32 engine's error on the rotated q and k, take the place of that model's
rtol(q). For a vector y = W h rotated at pos:
    dx_k = sqrt(32) u sum_m |W_in,km lat_m|                      (the query's input GEMM; 0 for a key)
    dh_k = |w_k| (36 u (1 + |hn_k|) + dx_k / sigma) + 2 u |h_k|,  hn = (x - mean) / sigma:
           the f32 mean and variance over 1024 terms (sqrt(1024) u = 32 u of the row's scale each,
           4 u for the subtraction, division and rsqrt), the input's error, the affine's two roundings
    dy_i = sum_k dh_k |W_ik| + (sqrt(1024) + 16) u sum_k |h_k W_ik|:  the 1024-term f32 dot, split in
           up to 16 slabs summed in f32
    d(rot y) per pair = dy_0 + dy_1 + the RoPE gate of tests/test_gpu_attention_core.py on (y_0, y_1).
Each case prints its worst err / bound.

Any layer: a fetched row sums to 1 within n 4 u and is zero past n (the fetch returns n floats; the
block's floats behind n are checked through the probe in tests/test_gpu_align.py); the row outside
the stage and every call without a valid frame return count 0. Every other output of every call,
wire bytes included, equals an engine without the stage bit for bit, and an engine that never enables
the stage builds the parent commit's plan (tests/golden/plan_ops_before_align.json)."""

import json
from pathlib import Path

import numpy as np
import pytest

from test_gpu_align import U, rope64, rope_tol

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "plan_ops_before_align.json"
SEED = 0x5EED
D, NH, LDIM = 1024, 16, 32
INF = float("inf")
S_ROWS = [5, 12, 7]
ALIGNED = [True, True, False]
FORMATS = [(24000, "pcm_s16le"), (8000, "ulaw"), None]
FRAMES = 6
MODES = [(False, 1), (True, 1), (True, 4)]  # (pipeline, back_frames)
L0 = "flow_lm.transformer.layers.0."


def ids_of(b):
    return np.random.default_rng(40 + b).integers(0, 4000, size=S_ROWS[b]).astype(np.int32)


def prompt(i):
    return (0.11 * np.random.default_rng(3 + i).standard_normal((4, 1024))).astype(np.float32)


def engine(mode, align, layer=0, heads=0xFFFF, slots=3):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=slots, max_ctx=64, lsd_decode_steps=1, seed=SEED, pipeline=mode[0],
                     back_frames=mode[1], wire=True, align=align, align_layer=layer, align_heads=heads)


def params(b, align, frames=FRAMES):
    from pocket_tts_amd import GenerationParams

    p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=frames, seed=1 + b)
    if FORMATS[b]:
        p.sample_rate, p.encoding = FORMATS[b]
    p.align = bool(align and ALIGNED[b])
    return p


def run(mode, align, per_row_voice, layer=0, heads=0xFFFF):
    """Every call's raw outputs, and per row the latents and alignment rows of its valid frames."""
    eng = engine(mode, align, layer, heads)
    try:
        voices = [eng.voice_from_prompt(prompt(b if per_row_voice else 0)) for b in range(3)] if per_row_voice \
            else [eng.voice_from_prompt(prompt(0))] * 3
        eng.open_many([0, 1, 2], voices, [ids_of(b) for b in range(3)], [params(b, align) for b in range(3)])
        rec, lat, rows = [], [[] for _ in range(3)], [[] for _ in range(3)]
        started, delay, call = 0, eng.frame_lag()[1], 0
        while any(len(x) < FRAMES for x in lat):
            assert call < 64, "the rows never finished"
            if started >= FRAMES and eng.pipeline:
                eng.flush_async(3)
            else:
                eng.step_async(3)
                started += call >= delay
            r, w = eng.fetch(3), eng.fetch_wire(3)
            a = eng.fetch_align(3) if align else [np.zeros(0, np.float32)] * 3
            rec.append((r.pcm.copy(), r.valid.copy(), r.last.copy(), r.eos_logits.copy(), r.latents.copy(), list(w)))
            for b in range(3):
                if r.valid[b]:
                    lat[b].append(r.latents[b].copy())
                    rows[b].append(a[b])
                else:
                    assert a[b].size == 0, (call, b)  # no valid frame: count 0
            call += 1
        return rec, lat, rows, [v.n_frames for v in voices]
    finally:
        eng.close()


_PLAIN = {}


def plain(mode, per_row_voice):
    key = (mode, per_row_voice)
    if key not in _PLAIN:
        _PLAIN[key] = run(mode, False, per_row_voice)[0]
    return _PLAIN[key]


def same_outputs(rec, prec):
    assert len(rec) == len(prec)
    for c, (x, y) in enumerate(zip(rec, prec)):
        for i in range(5):
            assert np.array_equal(x[i], y[i]), (c, i)
        assert x[5] == y[5], (c, "wire bytes")


# ---------------------------------------------------------------------------------------------
# layer 0 in float64, with the f32 engine's error carried along
# ---------------------------------------------------------------------------------------------
_W = {}


def weights():
    if not _W:
        import synth

        _W["embed"] = synth.synth_tensor(SEED, "flow_lm.conditioner.embed.weight", (4001, D)).astype(np.float64)
        _W["w_in"] = synth.synth_tensor(SEED, "flow_lm.input_linear.weight", (D, LDIM)).astype(np.float64)
        _W["bos"] = synth.synth_tensor(SEED, "flow_lm.bos_emb", (LDIM,)).astype(np.float64)
        _W["n1w"] = synth.synth_tensor(SEED, L0 + "norm1.weight", (D,)).astype(np.float64)
        _W["n1b"] = synth.synth_tensor(SEED, L0 + "norm1.bias", (D,)).astype(np.float64)
        qk = synth.synth_tensor(SEED, L0 + "self_attn.in_proj.weight", (3 * D, D)).astype(np.float64)
        _W["wq"], _W["wk"] = qk[:D], qk[D:2 * D]
    return _W


def project(x, dx, Wm, pos):
    """(rot y, d(rot y)) [NH][64] of y = Wm LN(x) rotated at pos (the module docstring's error terms)."""
    w = weights()
    mu, sig = x.mean(), np.sqrt(x.var() + 1e-5)
    hn = (x - mu) / sig
    h = hn * w["n1w"] + w["n1b"]
    dh = np.abs(w["n1w"]) * (36 * U * (1 + np.abs(hn)) + dx / sig) + 2 * U * np.abs(h)
    y = (Wm @ h).reshape(NH, 64)
    dy = (np.abs(Wm) @ dh + (32 + 16) * U * (np.abs(Wm) @ np.abs(h))).reshape(NH, 64)
    pair = np.repeat(dy[:, 0::2] + dy[:, 1::2], 2, axis=-1)
    return rope64(y, pos), pair + rope_tol(y, pos)


def layer0_reference(ids, F, lat_in, t):
    """(a [S], bound [S]) of frame t of a row with `ids` behind F voice rows, its backbone input lat_in."""
    w = weights()
    S = len(ids)
    K, dK = zip(*[project(w["embed"][ids[j]], 0.0, w["wk"], F + j) for j in range(S)])
    K, dK = np.stack(K, 1), np.stack(dK, 1)  # [NH][S][64]
    x = w["w_in"] @ lat_in
    dx = np.sqrt(32.0) * U * (np.abs(w["w_in"]) @ np.abs(lat_in))
    q, dq = project(x, dx, w["wq"], F + S + t)
    a = tol = 0.0
    for h in range(NH):
        s = K[h] @ q[h] / 8.0
        p = np.exp(s - s.max())
        p /= p.sum()
        E = U * (np.abs(K[h]) @ np.abs(q[h])) + (np.abs(K[h]) @ dq[h] + dK[h] @ np.abs(q[h])) / 8.0 + 6 * U \
            + 3 * U * np.abs(s - s.max())
        a = a + p
        tol = tol + p * (E + p @ E)
    return a / NH, 4.0 * tol / NH + 8 * U


@pytest.mark.parametrize("per_row_voice", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_layer0_rows_against_float64(mode, per_row_voice):
    rec, lat, rows, F = run(mode, True, per_row_voice, layer=0)
    same_outputs(rec, plain(mode, per_row_voice))
    w = weights()
    worst = 0.0
    for b in range(3):
        assert len(rows[b]) == FRAMES
        if not ALIGNED[b]:
            assert all(r.size == 0 for r in rows[b])
            continue
        ids = ids_of(b)
        for t in range(FRAMES):
            got = rows[b][t]
            assert got.size == S_ROWS[b], (b, t, got.size)
            lat_in = w["bos"] if t == 0 else lat[b][t - 1].astype(np.float64)
            ref, tol = layer0_reference(ids, F[b], lat_in, t)
            worst = max(worst, float((np.abs(got - ref) / tol).max()))
    print(f"mode {mode} per-row voice {per_row_voice}: worst err / bound {worst:.2e}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("mode", MODES)
def test_layer3_rows_are_distributions_and_nothing_else_moves(mode):
    rec, lat, rows, _ = run(mode, True, False, layer=3, heads=1 | 1 << 15)
    same_outputs(rec, plain(mode, False))
    for b in range(3):
        assert len(rows[b]) == FRAMES
        for r in rows[b]:
            if not ALIGNED[b]:
                assert r.size == 0
                continue
            assert r.size == S_ROWS[b] and np.all(r >= 0)
            assert abs(float(r.astype(np.float64).sum()) - 1.0) <= r.size * 4 * U


def test_cancelled_row_readmitted_with_another_length():
    """One call in flight: row 0 (S = 5) is cancelled after two delivered frames and re-admitted at
    once with S = 9 while the old pass is unfetched: no fetched row carries the old count, and the
    new rows equal a fresh engine's."""
    def admit(eng, v, S, frames):
        from pocket_tts_amd import GenerationParams

        p = GenerationParams(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=frames, seed=1)
        p.align = True
        eng.open_many([0], [v], [np.random.default_rng(S).integers(0, 4000, size=S).astype(np.int32)], [p])

    def collect(eng, n, out):
        for _ in range(32):
            if len(out) == n:
                return
            eng.step_async(1)
            r, a = eng.fetch(1, calls_back=1), eng.fetch_align(1, calls_back=1)
            if r.valid[0]:
                out.append(a[0])
            else:
                assert a[0].size == 0
        raise AssertionError("the row never delivered")

    nf = 4
    fresh = engine((True, 2), True, slots=1)
    try:
        admit(fresh, fresh.voice_from_prompt(prompt(0)), 9, nf)
        want = []
        fresh.step_async(1)
        collect(fresh, nf, want)
    finally:
        fresh.close()
    eng = engine((True, 2), True, slots=1)
    try:
        v = eng.voice_from_prompt(prompt(0))
        admit(eng, v, 5, 8)
        old, new = [], []
        eng.step_async(1)
        collect(eng, 2, old)
        assert [r.size for r in old] == [5, 5]
        eng.cancel_slots([0])  # with the pass over the row's later frames in flight
        admit(eng, v, 9, nf)
        collect(eng, nf, new)
        assert [r.size for r in new] == [9] * nf
        for x, y in zip(new, want):
            assert np.array_equal(x, y)
    finally:
        eng.close()


def test_plan_of_an_engine_without_the_stage_is_the_parents():
    """Engine.plan_ops(8) of engines that never enable the stage: the text the parent commit returns
    (the fixture was written by the parent's library); an engine with the stage adds one op behind
    its layer's attention, with its costs modelled."""
    import pocket_tts_amd as pt

    want = json.loads(GOLDEN.read_text())
    kinds = {"sequential": dict(pipeline=False),
             "pipelined_pair": dict(pipeline=True, back_frames=2),
             "pipelined_four_wire_tempo": dict(pipeline=True, back_frames=4, wire=True, tempo=True),
             "pipelined_four_wire_tempo_pitch_flac": dict(pipeline=True, back_frames=4, wire=True, tempo=True,
                                                          pitch=True, flac=True)}
    assert sorted(want) == sorted(kinds)
    for name, kw in kinds.items():
        eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=SEED, **kw)
        try:
            assert eng.plan_ops(8) == want[name], name
        finally:
            eng.close()
    eng = pt.Engine(device=0, max_slots=8, max_ctx=64, lsd_decode_steps=1, seed=SEED, pipeline=True, back_frames=2,
                    align=True, align_layer=4, align_heads=0x00F0)
    try:
        ops = eng.plan_ops(8)
        assert ops.index("flow.l4.align") == ops.index("flow.l4.attention") + 1
        assert [o for o in ops if o != "flow.l4.align"] == want["pipelined_pair"]
        cost = {n: (f, b) for n, f, b in eng.plan(8)}["flow.l4.align"]
        assert cost[1] > 0  # no row in the stage yet: the counts alone
    finally:
        eng.close()


def test_refusals_admit_nothing():
    import pocket_tts_amd as pt

    for layer, heads in [(6, 0xFFFF), (-1, 1), (0, 0), (0, 1 << 16)]:
        with pytest.raises(pt.PocketTTSError):
            engine((False, 1), True, layer=layer, heads=heads)
    eng = engine((False, 1), False)
    try:
        v = eng.voice_from_prompt(prompt(0))
        with pytest.raises(pt.PocketTTSError):  # no align stage
            eng.open_many([0], [v], [ids_of(0)], [params(0, True)])
        with pytest.raises(pt.PocketTTSError):
            eng.fetch_align(1)
        eng.open_many([0], [v], [ids_of(0)], [params(0, False)])
        assert eng.step(1).valid[0]
        from pocket_tts_amd._lib import check, lib
        with pytest.raises(pt.PocketTTSError):  # not after the first step
            check(lib().ptts_align_enable(eng.handle, 1, 0, 0xFFFF))
    finally:
        eng.close()
    eng = pt.Engine(device=0, max_slots=2, max_ctx=256, lsd_decode_steps=1, seed=SEED, align=True)
    try:
        v = eng.voice_from_prompt(prompt(0))
        from pocket_tts_amd import GenerationParams

        p = GenerationParams(temp=0.0, eos_threshold=INF, max_frames=2, seed=1)
        p.align = True
        long_ids = np.arange(129, dtype=np.int32)
        with pytest.raises(pt.PocketTTSError):  # more than PTTS_ALIGN_TOKENS ids: neither row is admitted
            eng.open_many([0, 1], [v, v], [ids_of(0), long_ids], [p, p])
        r = eng.step(2)
        assert not r.valid.any()
        eng.open_many([0], [v], [long_ids[:128]], [p])
        q = GenerationParams(temp=0.0, eos_threshold=INF, max_frames=2, seed=1)  # no align: the ABI's older entry points
        eng.open_many([1], [v], [ids_of(1)], [q])
        r, a = eng.step(2), eng.fetch_align(2)
        assert r.valid.all() and a[0].size == 128 and a[1].size == 0
    finally:
        eng.close()


def test_tts_model_returns_words():
    """TTSModel.generate / generate_parallel with timestamps: (audio, words), the audio that of the
    call without timestamps (temp 0), the words those of the text with times inside the audio; a
    pause shifts the words behind it by its samples."""
    import pocket_tts_amd as pt
    from pocket_tts_amd import align

    tok = pt.load_tokenizer(str(Path(__file__).parent / "golden" / "reference_tokenizer.json"))
    eng = pt.Engine(device=0, max_slots=2, max_ctx=256, lsd_decode_steps=1, seed=SEED, pipeline=True, back_frames=2,
                    align=True, align_layer=2, align_heads=0x0F0F)
    try:
        m = pt.TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=INF, noise_clamp=None, tokenizer=tok)
        v = eng.voice_from_prompt(prompt(0))
        text = "Hello, world! This is unbelievable."
        x = m.generate(text, v, max_frames=6)
        audio, words = m.generate(text, v, max_frames=6, timestamps=True)
        assert isinstance(audio, np.ndarray) and np.array_equal(audio, x) and x.shape == (1, 6 * 1920)
        assert [w["word"] for w in words] == ["Hello,", "world!", "This", "is", "unbelievable."]
        starts = [w["start"] for w in words]
        assert starts[0] == 0.0 and starts == sorted(starts) and all(w["start"] <= w["end"] <= 0.48 + 1e-9 for w in words)
        assert [w["word"] for w in align.timestamps(tok, tok(pt.prepare_text_prompt(text)), np.zeros((0, 13)))] == \
            [w["word"] for w in words]
        with pytest.raises(ValueError):
            m.generate(np.array([260, 2994], np.int32), v, max_frames=2, timestamps=True)  # ids carry no words
        long = "Hello there [pause:250ms] General Kenobi"
        y = m.generate_parallel(long, v, pauses=True)
        audio2, words2 = m.generate_parallel(long, v, pauses=True, timestamps=True)
        assert audio2.shape == y.shape  # (each call draws new seeds: the segments' lengths are what must agree)
        assert [w["word"] for w in words2] == ["Hello", "there.", "General", "Kenobi."]
        total = audio2.shape[-1] / 24000
        assert all(0.0 <= w["start"] <= w["end"] <= total + 1e-9 for w in words2)
        assert words2[2]["start"] >= words2[1]["end"] + 0.25 - 1e-9  # the pause's 6000 samples lie between them
    finally:
        eng.close()


def test_a_56_byte_slot_opts_behaves_as_before():
    """A caller built before `align` states size 56: on an align-enabled engine its row is admitted
    outside the stage (count 0 with every frame) and its frames are bit for bit those of the same
    row on an engine without the stage."""
    import ctypes as C

    from pocket_tts_amd._lib import SlotOpts4, check, lib

    def frames(align):
        eng = engine((False, 1), align, slots=1)
        try:
            v = eng.voice_from_prompt(prompt(0))
            ids = np.ascontiguousarray(ids_of(1))
            gp, n = params(2, False, 3).to_c(), C.c_int32(ids.size)
            o = SlotOpts4(C.sizeof(SlotOpts4))
            assert o.size == 56
            i32 = C.POINTER(C.c_int32)
            check(lib().ptts_slots_open_opts(eng.handle, 1, C.byref(C.c_int32(0)), (C.c_void_p * 1)(v.handle),
                                             ids.ctypes.data_as(i32), C.byref(n), C.byref(gp), C.addressof(o)))
            out = []
            for _ in range(3):
                r = eng.step(1)
                assert r.valid[0]
                if align:
                    assert eng.fetch_align(1)[0].size == 0
                out.append((r.pcm[0].copy(), r.latents[0].copy(), float(r.eos_logits[0]), bool(r.last[0])))
            return out
        finally:
            eng.close()

    for x, y in zip(frames(True), frames(False)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:]


def test_a_finished_row_leaves_the_stage():
    """Row 0 (2 frames) finishes while row 1 (5 frames) goes on and still steps it: once its last
    frame is fetched its table entry is cleared, so the align launch's modelled traffic falls to that
    of row 1 alone, and row 1's rows are those of the same batch in which row 0 runs on."""
    def scenario(frames0):
        eng = engine((True, 1), True, slots=2)
        try:
            v = eng.voice_from_prompt(prompt(0))
            eng.open_many([0, 1], [v, v], [ids_of(0), ids_of(1)], [params(0, True, frames0), params(1, True, 5)])
            cost = lambda: {n: b for n, _, b in eng.plan(2)}["flow.l0.align"]
            before, mid, got = cost(), None, [[], []]
            for call in range(12):
                eng.step_async(2)
                r, a = eng.fetch(2), eng.fetch_align(2)
                for b in range(2):
                    if r.valid[b]:
                        got[b].append(a[b])
                if len(got[1]) == 3 and mid is None:
                    mid = cost()  # row 1 in mid-utterance
                if len(got[1]) == 5:
                    break
            return before, mid, got
        finally:
            eng.close()

    both, one, got = scenario(2)
    assert [x.size for x in got[0]] == [5, 5] and [x.size for x in got[1]] == [12] * 5
    # the keys of row 0 (5 tokens x 16 heads x 256 B), its q slabs, RoPE row and output are gone,
    # row 1's (12 tokens) are still read
    assert both - one >= 16 * 256 * 5 and one >= 16 * 256 * 12
    both2, still, want = scenario(5)
    assert both2 == both == still and [x.size for x in want[0]] == [5] * 5
    for x, y in zip(got[1], want[1]):
        assert np.array_equal(x, y)
