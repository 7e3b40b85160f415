"""Rows admitted behind a teacher-forced latent prefix, and onto their slot's codec state
(ptts_slot_opts.prefix_latents / .n_prefix / .keep_codec).

The rule under test: a row admitted with prefix p[0 .. n) starts in the state of a row admitted
without one that then ran n steps with each sampled latent replaced by p[j] (ptts_slot_set_latent
after every step), those steps' outputs discarded; its counters count new frames only. The oracle
states exactly that: orc_step(latent_in=...) is the forced step. orc_step decodes the latent it
sampled itself, not the forced one, so the expected PCM never comes from the forced state: it is
orc_mimi_decode on a state of its own (fresh, or the one that decoded the slot's previous utterance).

Tolerances are the project's own against the oracle (conftest.py): latents and EOS logits 5e-5, PCM
2e-6 max abs per frame. Synthetic weights, 4 slots, a 5-frame voice."""

import ctypes as C

import numpy as np
import pytest
from _oracle import fp
from conftest import LAT_TOL, PCM_TOL, load_golden, pcm_err
from test_gpu_parity import _noise

pytestmark = pytest.mark.gpu

INF = float("inf")
F_VOICE = 5
CTX = 128
# the rows of test 1: (tokens, prefix frames, seed of ids and prefix); row 0's text + prefix is 26
# rows, across a 16-row group. Test 2 needs new-frame EOS logits 0 and 1 of row 0 that rise by more
# than 2e-3. Logit 0 depends on the inputs alone, and a unit-scale prefix mostly leaves it the highest,
# so the inputs' seed is the one of 0..7 with the lowest logit 0 on the CPU oracle (-0.372), and at
# temp 0.7 the first sampling seed tried, EOS_SEED = 0, has logit 1 at -0.260: a rise of 0.111.
ROW0_SEED = 4
EOS_SEED = 0
ROWS = [(7, 19, ROW0_SEED), (9, 16, 101), (7, 0, 102)]
ENGINES = [(False, 1), (True, 1), (True, 2)]


def params(**kw):
    from pocket_tts_amd import GenerationParams

    base = dict(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=4, seed=1)
    base.update(kw)
    return GenerationParams(**base)


def make_engine(pipeline, back_frames, **kw):
    import pocket_tts_amd as pt

    return pt.Engine(device=0, max_slots=4, max_ctx=CTX, lsd_decode_steps=1, seed=0x5EED, pipeline=pipeline,
                     back_frames=back_frames, **kw)


def prompt_of(row):
    d = load_golden("e2e_lsd1.safetensors")
    return (d["prompt"][:F_VOICE] * (1.0 + 0.07 * row)).astype(np.float32)


def row_inputs(S, n_prefix, seed):
    """Token ids and an arbitrary finite prefix (unit scale) from one seed."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 4000, size=S).astype(np.int32)
    return ids, rng.standard_normal((n_prefix, 32)).astype(np.float32)


def mimi_decode(oracle, state, latents):
    """orc_mimi_decode of each latent in sequence on `state` (advances its codec state)."""
    oracle.L.orc_mimi_decode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    out = np.zeros((len(latents), 1920), np.float32)
    for i, lat in enumerate(latents):
        oracle.L.orc_mimi_decode(oracle.m, state.s, fp(np.ascontiguousarray(lat, np.float32)), fp(out[i]))
    return out


def forced_run(oracle, prompt, ids, prefix, n_new, noise=None):
    """The rule on the oracle: prefill voice and tokens, one forced step per prefix latent (inputs
    bos, p[0], .., outputs discarded), then n_new free steps from p[-1]. noise(i): x_0 of new frame i."""
    s = oracle.new_state(CTX)
    s.prefill(prompt)
    if len(ids):
        s.prefill_tokens(ids)
    inp = None
    for p in prefix:
        s.step(inp)
        inp = p
    lat, eos = [], []
    for i in range(n_new):
        o = s.step(inp, noise=None if noise is None else noise(i))
        inp = o["latent"]
        lat.append(o["latent"])
        eos.append(o["eos_logit"])
    return np.array(lat), np.array(eos)


_CACHE: dict = {}


def expected(oracle, row, temp=0.0, seed=1):
    """(latents, EOS logits, fresh-codec PCM) of 4 new frames of ROWS[row]; computed once."""
    key = (row, temp, seed)
    if key not in _CACHE:
        S, n_pre, rs = ROWS[row]
        ids, pre = row_inputs(S, n_pre, rs)
        noise = None if temp == 0.0 else (lambda i: _noise(seed, i, temp, None))
        lat, eos = forced_run(oracle, prompt_of(row), ids, pre, 4, noise)
        _CACHE[key] = (lat, eos, mimi_decode(oracle, oracle.new_state(CTX), lat))
    return _CACHE[key]


class Run:
    """Steps rows [0, B) and files the frames of `rows` in order: per row the lists of latents, EOS
    logits, PCM frames and `last` flags."""

    def __init__(self, eng, B, rows):
        self.eng, self.B, self.rows = eng, B, list(rows)
        self.got = {b: dict(lat=[], eos=[], pcm=[], last=[]) for b in rows}
        self.done = set()

    def call(self):
        self.eng.step_async(self.B)
        r = self.eng.fetch(self.B)
        for b in self.rows:
            if r.valid[b] and b not in self.done:
                g = self.got[b]
                g["lat"].append(r.latents[b].copy())
                g["eos"].append(float(r.eos_logits[b]))
                g["pcm"].append(r.pcm[b].copy())
                g["last"].append(bool(r.last[b]))
                if r.last[b]:
                    self.done.add(b)

    def finish(self, max_calls=80):
        """Step until every row has returned its last frame."""
        for _ in range(max_calls):
            if len(self.done) == len(self.rows):
                return self.got
            self.call()
        raise AssertionError(f"rows {sorted(set(self.rows) - self.done)} did not finish in {max_calls} calls")


def collect(eng, B, rows):
    return Run(eng, B, rows).finish()


def check_frames(g, lat, eos, pcm, what):
    n = len(lat)
    assert len(g["lat"]) == n, (what, len(g["lat"]), n)
    for i in range(n):
        e_lat = float(np.abs(g["lat"][i] - lat[i]).max())
        e_eos = abs(g["eos"][i] - eos[i])
        e_pcm = pcm_err(g["pcm"][i] - pcm[i])
        print(f"{what} frame {i}: latent {e_lat:.3g} eos {e_eos:.3g} pcm {e_pcm:.3g}")
        assert e_lat <= LAT_TOL and e_eos <= LAT_TOL, (what, i, e_lat, e_eos)
        assert e_pcm <= PCM_TOL, (what, i, e_pcm)
    assert g["last"] == [False] * (n - 1) + [True], (what, g["last"])


def admit_rows(eng, rows, slots, **kw):
    voices, ids_l, ps = [], [], []
    for row in rows:
        S, n_pre, rs = ROWS[row]
        ids, pre = row_inputs(S, n_pre, rs)
        voices.append(eng.voice_from_prompt(prompt_of(row)))
        ids_l.append(ids)
        ps.append(params(prefix_latents=pre if n_pre else None, **kw))
    eng.open_many(slots, voices, ids_l, ps)
    return voices


@pytest.mark.parametrize("pipeline,back_frames,temp", [(p, b, 0.0) for p, b in ENGINES] + [(True, 2, 0.7)])
def test_prefix_equals_forced_steps(oracle, pipeline, back_frames, temp):
    """1. Three rows in one admission (prefixes of 19, 16 and 0 frames), 4 new frames each: latents,
    EOS logits and fresh-codec PCM equal the oracle's forced run. At temp 0.7 the oracle's noise is
    drawn at step indices 0..3: the noise stream is indexed from the first new frame."""
    seed = 77
    eng = make_engine(pipeline, back_frames)
    try:
        admit_rows(eng, [0, 1, 2], [2, 0, 1], temp=temp, seed=seed)
        got = collect(eng, 4, [2, 0, 1])
        for row, slot in zip([0, 1, 2], [2, 0, 1]):
            lat, eos, pcm = expected(oracle, row, temp, seed)
            check_frames(got[slot], lat, eos, pcm, f"row {row}")
    finally:
        eng.close()


def test_counters_count_new_frames(oracle):
    """2. Behind a 19-frame prefix: max_frames = 3 ends the row on its third NEW frame; and with a
    threshold between the oracle's new-frame logits 0 and 1 (temp 0.7; >= 1e-3 from both, 20x the
    logit tolerance), EOS is found at new frame 1 and frames_after_eos = 1 ends the row on new frame
    2, well inside max_frames = 8."""
    lat, eos, pcm = expected(oracle, 0)
    lat7, eos7, pcm7 = expected(oracle, 0, 0.7, EOS_SEED)
    S, n_pre, rs = ROWS[0]
    ids, pre = row_inputs(S, n_pre, rs)
    thr = 0.5 * (eos7[0] + eos7[1])
    assert eos7[0] <= thr - 1e-3 and eos7[1] >= thr + 1e-3, eos7
    eng = make_engine(False, 1)
    try:
        v = eng.voice_from_prompt(prompt_of(0))
        eng.open(1, v, ids, params(prefix_latents=pre, max_frames=3))
        check_frames(collect(eng, 2, [1])[1], lat[:3], eos[:3], pcm[:3], "max_frames 3")
        eng.open(1, v, ids, params(prefix_latents=pre, max_frames=8, eos_threshold=float(thr), frames_after_eos=1,
                                   temp=0.7, seed=EOS_SEED))
        check_frames(collect(eng, 2, [1])[1], lat7[:3], eos7[:3], pcm7[:3], "eos at new frame 1")
    finally:
        eng.close()


@pytest.mark.parametrize("back_frames", [1, 4])
def test_keep_codec_across_ring_wrap(oracle, back_frames):
    """3. Utterance A (17 frames = 272 Mimi positions, past the 250-position window; with 4-frame
    passes it ends in a partial pass), then B on the same slot with ids A ++ B, prefix = A's fetched
    latents and keep_codec: FlowLM outputs equal a fresh oracle state forced through A's latents, PCM
    equals orc_mimi_decode on the oracle state that decoded A. The same admission with keep_codec =
    0 equals the fresh-state PCM, which differs from the other by far more than the tolerance."""
    rng = np.random.default_rng(5)
    ids_a = rng.integers(0, 4000, size=7).astype(np.int32)
    ids_b = rng.integers(0, 4000, size=6).astype(np.int32)
    ids_ab = np.concatenate([ids_a, ids_b])
    prompt = prompt_of(0)
    eng = make_engine(True, back_frames)
    try:
        v = eng.voice_from_prompt(prompt)
        for keep in (1, 0):
            eng.open(0, v, ids_a, params(max_frames=17))
            a = collect(eng, 1, [0])[0]
            assert len(a["lat"]) == 17
            pre = np.array(a["lat"])
            # the oracle's A (orc_step decodes its own latents on its own codec state)
            sa = oracle.new_state(CTX)
            sa.prefill(prompt)
            sa.prefill_tokens(ids_a)
            inp = None
            for i in range(17):
                o = sa.step(inp)
                inp = o["latent"]
                np.testing.assert_allclose(a["lat"][i], o["latent"], atol=LAT_TOL)
                assert pcm_err(a["pcm"][i] - o["pcm"]) <= PCM_TOL, i
            lat, eos = forced_run(oracle, prompt, ids_ab, pre, 4)
            pcm_keep = mimi_decode(oracle, sa, lat)
            pcm_fresh = mimi_decode(oracle, oracle.new_state(CTX), lat)
            print("keep vs fresh PCM, max abs difference per frame:",
                  [f"{pcm_err(pcm_keep[i] - pcm_fresh[i]):.3g}" for i in range(4)])
            assert pcm_err(pcm_keep - pcm_fresh) > 100 * PCM_TOL
            eng.open(0, v, ids_ab, params(prefix_latents=pre, keep_codec=bool(keep)))
            b = collect(eng, 1, [0])[0]
            check_frames(b, lat, eos, pcm_keep if keep else pcm_fresh, f"keep_codec {keep}")
    finally:
        eng.close()


@pytest.mark.parametrize("pipeline,back_frames", [(False, 1), (True, 2)])
def test_neighbours_untouched(oracle, pipeline, back_frames):
    """4. Row 1 is mid-utterance when row 0 is admitted behind a 19-frame prefix: every frame of
    row 1 equals its own oracle run, and row 0 its forced run."""
    eng = make_engine(pipeline, back_frames)
    try:
        rng = np.random.default_rng(9)
        ids1 = rng.integers(0, 4000, size=11).astype(np.int32)
        v1 = eng.voice_from_prompt(prompt_of(3))
        eng.open(1, v1, ids1, params(max_frames=9))
        run = Run(eng, 2, [0, 1])
        for _ in range(3):  # row 1 alone
            run.call()
        admit_rows(eng, [0], [0])
        got = run.finish()
        lat1, eos1 = forced_run(oracle, prompt_of(3), ids1, [], 9)
        check_frames(got[1], lat1, eos1, mimi_decode(oracle, oracle.new_state(CTX), lat1), "neighbour")
        check_frames(got[0], *expected(oracle, 0), "prefix row")
    finally:
        eng.close()


def _raw_open(eng, slot, voice, ids, p, opts, stride):
    """ptts_slots_open_opts of one row with a hand-made opts entry."""
    from pocket_tts_amd import lib

    ids = np.ascontiguousarray(ids, np.int32)
    i32 = C.POINTER(C.c_int32)
    sl = (C.c_int32 * 1)(slot)
    nid = (C.c_int32 * 1)(ids.size)
    vh = (C.c_void_p * 1)(voice.handle)
    cp = p.to_c()
    return lib().ptts_slots_open_opts(eng.handle, 1, sl, vh, ids.ctypes.data_as(i32), nid, C.byref(cp),
                                      C.cast(opts, C.c_void_p))


def test_refusals(oracle):
    """5. Every PTTS_ERR_INVALID case admits nothing; keep_codec after a cancel, or with the last
    frame unfetched, is PTTS_ERR_STATE; a 24-byte-stride opts array behaves as no prefix."""
    from pocket_tts_amd._lib import PocketTTSError, SlotOpts, SlotOpts2

    S, n_pre, rs = ROWS[0]
    ids, pre = row_inputs(S, n_pre, rs)
    eng = make_engine(False, 1)
    try:
        v = eng.voice_from_prompt(prompt_of(0))
        assert C.sizeof(SlotOpts2) == 40 and SlotOpts2.prefix_latents.offset == 24 and SlotOpts2.keep_codec.offset == 36

        def idle():
            r = eng.step(4)
            assert not r.valid.any()

        bad = [
            SlotOpts2(40, 0, 0, 0, 0, pre.ctypes.data, -1, 0),  # n_prefix < 0
            SlotOpts2(40, 0, 0, 0, 0, None, 3, 0),              # a prefix with no pointer
            SlotOpts2(40, 0, 0, 0, 0, None, 0, 2),              # keep_codec outside {0, 1}
            SlotOpts2(40, 0, 0, 0, 0, None, 0, -1),
        ]
        for o in bad:
            assert _raw_open(eng, 0, v, ids, params(), (SlotOpts2 * 1)(o), 40) == 1, (o.n_prefix, o.keep_codec)
            idle()
        # capacity: F + S + n_prefix + max_frames <= max_ctx, at the bound and one past it
        room = CTX - F_VOICE - S - n_pre
        with pytest.raises(PocketTTSError) as ei:
            eng.open(0, v, ids, params(prefix_latents=pre, max_frames=room + 1))
        assert ei.value.code == 1
        idle()
        eng.open(0, v, ids, params(prefix_latents=pre, max_frames=room))
        assert eng.step(4).valid[0]
        # keep_codec with the utterance still running (its last frame unfetched), and after a cancel
        with pytest.raises(PocketTTSError) as ei:
            eng.open(0, v, ids, params(keep_codec=True))
        assert ei.value.code == 3
        assert eng.step(4).valid[0]  # the running utterance is untouched
        eng.cancel_slots([0])
        idle()
        with pytest.raises(PocketTTSError) as ei:
            eng.open(0, v, ids, params(keep_codec=True))
        assert ei.value.code == 3
        idle()
        # ... while a slot that was never used, and one whose last frame was fetched, admit it
        eng.open(3, v, ids, params(keep_codec=True, max_frames=1))
        r = eng.step(4)
        assert r.valid[3] and r.last[3]
        eng.open(3, v, ids, params(keep_codec=True, max_frames=1))
        assert eng.step(4).last[3]
        # after ptts_slot_close too
        eng.open(3, v, ids, params(max_frames=2))
        eng.close_slot(3)
        with pytest.raises(PocketTTSError) as ei:
            eng.open(3, v, ids, params(keep_codec=True))
        assert ei.value.code == 3
        idle()
        # the 24-byte struct of an older caller: the bytes behind it are not read as a prefix
        raw = (C.c_uint64 * 6)(24, 0, 0, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFF00000001, 0xFFFFFFFFFFFFFFFF)
        assert C.sizeof(SlotOpts) == 24
        assert _raw_open(eng, 1, v, ids, params(), raw, 24) == 0
        lat, eos = forced_run(oracle, prompt_of(0), ids, [], 4)
        check_frames(collect(eng, 4, [1])[1], lat, eos, mimi_decode(oracle, oracle.new_state(CTX), lat), "24-byte opts")
    finally:
        eng.close()


def test_previews_of_prefix_and_keep_rows(oracle):
    """5 (previews). With previews enabled a keep_codec row yields none, and a prefix row with a fresh
    codec yields one within the tolerance the preview tests use (PCM_TOL against the oracle)."""
    eng = make_engine(True, 2)
    try:
        eng.enable_preview(4)
        S, n_pre, rs = ROWS[0]
        ids, pre = row_inputs(S, n_pre, rs)
        v0, v1 = eng.voice_from_prompt(prompt_of(0)), eng.voice_from_prompt(prompt_of(1))
        ids1, pre1 = row_inputs(*ROWS[1])
        eng.open_many([0, 1], [v0, v1], [ids, ids1],
                      [params(prefix_latents=pre), params(prefix_latents=pre1, keep_codec=True)])
        got = collect(eng, 2, [0, 1])
        pv = dict(eng.fetch_previews(wait=True))
        assert sorted(pv) == [0], sorted(pv)
        lat, eos, pcm = expected(oracle, 0)
        assert pcm_err(pv[0] - pcm[0]) <= PCM_TOL
        check_frames(got[0], lat, eos, pcm, "prefix row")
        check_frames(got[1], *expected(oracle, 1), "keep_codec row on a never-used slot")
    finally:
        eng.close()


def test_tts_model_chain_matches_oracle(oracle):
    """TTSModel.generate_continued on the real engine: the second link's audio is the oracle's
    forced run through the first link's latents, decoded on from the state that decoded the first
    (an EOS threshold every logit exceeds: each link is its 5-frame tail after frame 0)."""
    from pocket_tts_amd import TTSModel
    from pocket_tts_amd.text import prepare_text_prompt
    from test_text_frontend import synthetic_tokenizer

    tok = synthetic_tokenizer()
    eng = make_engine(False, 1)
    try:
        m = TTSModel(eng, temp=0.0, lsd_decode_steps=1, eos_threshold=-INF, noise_clamp=None, tokenizer=tok)
        v = eng.voice_from_prompt(prompt_of(0))
        pcm_a, ca = m.generate_continued("Hello there.", v)
        pcm_b, cb = m.generate_continued("Good day.", v, ca)
        assert ca.latents.shape == (6, 32) and cb.latents.shape == (6, 32)
        assert ca.ids.tolist() == list(tok(prepare_text_prompt("Hello there.")))
        sa = oracle.new_state(CTX)
        sa.prefill(prompt_of(0))
        sa.prefill_tokens(ca.ids)
        inp = None
        for i in range(6):
            o = sa.step(inp)
            inp = o["latent"]
            assert pcm_err(pcm_a[0, 1920 * i:1920 * (i + 1)] - o["pcm"]) <= PCM_TOL, i
        lat, eos = forced_run(oracle, prompt_of(0), np.concatenate([ca.ids, cb.ids]), ca.latents, 6)
        pcm = mimi_decode(oracle, sa, lat)
        np.testing.assert_allclose(cb.latents, lat, atol=LAT_TOL)
        for i in range(6):
            assert pcm_err(pcm_b[0, 1920 * i:1920 * (i + 1)] - pcm[i]) <= PCM_TOL, i
    finally:
        eng.close()


def test_scheduler_chain_on_the_engine(oracle):
    """The server's scheduler on a pipelined engine with previews on: a continuity group of two
    segments and, beside it, a plain request. The group's audio is segment A, then segment B as the
    oracle's forced run through the latents the scheduler kept of A, decoded on from A's codec
    state; the plain request equals its own oracle run."""
    from pocket_tts_amd.serve import BatchScheduler

    rng = np.random.default_rng(21)
    ids_a = rng.integers(0, 4000, size=7).astype(np.int32)
    ids_b = rng.integers(0, 4000, size=9).astype(np.int32)
    ids_c = rng.integers(0, 4000, size=5).astype(np.int32)
    eng = make_engine(True, 2)
    sch = BatchScheduler(eng, preview_rows=4)
    try:
        v = eng.voice_from_prompt(prompt_of(0))
        with sch.cv:
            g = sch.submit_group([("text", ids_a, params(max_frames=5)), ("text", ids_b, params(max_frames=4))], v,
                                 continuity=True)
            plain = sch.submit(ids_c, v, params(max_frames=7))
        audio = g.audio(timeout=60).reshape(-1, 1920)
        other = plain.audio(timeout=60).reshape(-1, 1920)
        assert audio.shape[0] == 9 and other.shape[0] == 7
        a, b = g.segments
        assert b.slot == a.slot and b.params.keep_codec and len(a.lat) == 5
        sa = oracle.new_state(CTX)
        sa.prefill(prompt_of(0))
        sa.prefill_tokens(ids_a)
        inp = None
        for i in range(5):
            o = sa.step(inp)
            inp = o["latent"]
            np.testing.assert_allclose(a.lat[i], o["latent"], atol=LAT_TOL)
            assert pcm_err(audio[i] - o["pcm"]) <= PCM_TOL, i
        lat, eos = forced_run(oracle, prompt_of(0), np.concatenate([ids_a, ids_b]), np.array(a.lat), 4)
        pcm = mimi_decode(oracle, sa, lat)
        for i in range(4):
            assert pcm_err(audio[5 + i] - pcm[i]) <= PCM_TOL, i
        lat_c, _ = forced_run(oracle, prompt_of(0), ids_c, [], 7)
        pcm_c = mimi_decode(oracle, oracle.new_state(CTX), lat_c)
        for i in range(7):
            assert pcm_err(other[i] - pcm_c[i]) <= PCM_TOL, i
    finally:
        sch.close()
        eng.close()
