"""Per-utterance LSD Euler step counts in one batch (ptts_slot_open_ex / ptts_slots_open_ex,
GenerationParams.lsd_steps): an engine is created with a cap, every utterance chooses its own
count n in [1, cap] at admission, rows with different n share one batched step, and each row must
compute what a whole engine created at lsd_decode_steps = n would.

Every row is compared with its own oracle run at its own n (the oracle takes lsd_steps per step),
at the suite's fp32 gates (conftest.py: LAT_TOL 5e-5 on latents and EOS logits, PCM_TOL 2e-6 on
PCM), temp 0 and eos_threshold = inf as in the other parity tests."""

import numpy as np
import pytest
from conftest import LAT_TOL, PCM_TOL, load_golden, pcm_err, rms

pytestmark = pytest.mark.gpu

INF = float("inf")


def params(**kw):
    from pocket_tts_amd import GenerationParams

    base = dict(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=64, seed=1)
    base.update(kw)
    return GenerationParams(**base)


def check_step(r, row, d, i):
    """test_gpu_parity.check_step: one engine row against frame i of a reference fixture."""
    assert r.valid[row]
    assert abs(r.eos_logits[row] - d["eos_logit"][i]) <= LAT_TOL, (i, r.eos_logits[row], d["eos_logit"][i])
    np.testing.assert_allclose(r.latents[row], d["latent"][i], atol=LAT_TOL)
    diff = r.pcm[row] - d["pcm"][i]
    assert pcm_err(diff) <= PCM_TOL, (i, rms(diff), pcm_err(diff))


def check_row(r, b, o):
    """engine row b of a step result against its oracle step o"""
    assert r.valid[b], b
    assert abs(r.eos_logits[b] - o["eos_logit"]) <= LAT_TOL, (b, r.eos_logits[b], o["eos_logit"])
    np.testing.assert_allclose(r.latents[b], o["latent"], atol=LAT_TOL, err_msg=f"row {b}")
    assert pcm_err(r.pcm[b] - o["pcm"]) <= PCM_TOL, (b, pcm_err(r.pcm[b] - o["pcm"]))


class Rows:
    """The oracle side of a batch: per row its state, its own step count and its last latent."""

    def __init__(self, oracle, ctx):
        self.oracle, self.ctx = oracle, ctx
        self.s, self.n, self.lat, self.got = {}, {}, {}, {}

    def add(self, b, prompt, ids, n):
        s = self.oracle.new_state(self.ctx)
        s.prefill(prompt)
        s.prefill_tokens(ids)
        self.s[b], self.n[b], self.lat[b], self.got[b] = s, n, None, 0

    def check(self, r, rows=None):
        """every valid row of `r` (or exactly `rows`) against the next oracle step at the row's n"""
        for b in (rows if rows is not None else [b for b in self.s if r.valid[b]]):
            o = self.s[b].step(self.lat[b], lsd_steps=self.n[b])
            self.lat[b] = o["latent"]
            self.got[b] += 1
            check_row(r, b, o)


def test_reference_goldens_at_two_counts_on_one_engine():
    """One cap-2 engine: slot 0 opened with lsd_steps=2 equals the reference's e2e_lsd2 fixture step
    by step, then re-opened with lsd_steps=1 equals its e2e_lsd1 fixture (both made by the
    reference). The second run pays for one Euler step."""
    import pocket_tts_amd as pt

    d2, d1 = load_golden("e2e_lsd2.safetensors"), load_golden("e2e_lsd1.safetensors")
    eng = pt.Engine(device=0, max_slots=1, max_ctx=128, lsd_decode_steps=2, seed=0x5EED)
    try:
        assert eng.lsd_steps() == (2, 0)
        eng.open(0, eng.voice_from_prompt(d2["prompt"]), d2["text_ids"], params(max_frames=8, lsd_steps=2))
        for i in range(d2["latent"].shape[0]):
            check_step(eng.step(1), 0, d2, i)
        assert eng.lsd_steps() == (2, 2)
        n = d1["latent"].shape[0]
        eng.open(0, eng.voice_from_prompt(d1["prompt"]), d1["text_ids"], params(max_frames=n, lsd_steps=1))
        for i in range(n):
            r = eng.step(1)
            check_step(r, 0, d1, i)
            assert bool(r.last[0]) == (i == n - 1)
        assert eng.lsd_steps() == (2, 1)
    finally:
        eng.close()


def test_mixed_rows_persistent_chain(oracle):
    """B = 20 (two row groups of k_flow_head, the second ragged), cap 3, n_b = 1 + b % 3: every row
    of every step equals its oracle run at its own n; the launch runs 3 Euler steps."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(11)
    B, steps = 20, 3
    eng = pt.Engine(device=0, max_slots=B, max_ctx=64, lsd_decode_steps=3, seed=0x5EED)
    try:
        assert "head.chain" in eng.plan_ops(B)
        rows = Rows(oracle, 64)
        for b in range(B):
            F = 3 + (b % 5)
            prompt = (d["prompt"][:F] * (1.0 + 0.05 * b)).astype(np.float32)
            ids = rng.integers(0, 4000, size=2 + b % 3).astype(np.int32)
            n = 1 + b % 3
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(max_frames=steps, lsd_steps=n))
            rows.add(b, prompt, ids, n)
        for _ in range(steps):
            r = eng.step(B)
            assert r.valid.all()
            rows.check(r, range(B))
            assert eng.lsd_steps() == (3, 3)
    finally:
        eng.close()


def test_run_length_follows_the_open_rows(oracle):
    """Cap 3, 4 slots: rows 0/1 (n = 3) end after 2 frames, rows 2/3 (n = 1) after 6. Once only the
    n = 1 rows are open the step runs one Euler step (another front graph; the chain's counters
    re-armed by the longer launch); an n = 2 row admitted into a freed slot raises it to 2. Every
    row keeps matching its oracle across the switches."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(3)
    eng = pt.Engine(device=0, max_slots=4, max_ctx=128, lsd_decode_steps=3, seed=0x5EED)
    try:
        rows = Rows(oracle, 128)

        def admit(b, n, frames):
            prompt = (d["prompt"][: 4 + 2 * b] * (1.0 + 0.06 * b + 0.01 * n)).astype(np.float32)
            ids = rng.integers(0, 4000, size=3 + b).astype(np.int32)
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(max_frames=frames, lsd_steps=n))
            rows.add(b, prompt, ids, n)

        for b in range(4):
            admit(b, 3 if b < 2 else 1, 2 if b < 2 else 6)
        for i in range(2):
            r = eng.step(4)
            rows.check(r, range(4))
            assert eng.lsd_steps()[1] == 3
            assert bool(r.last[0]) == bool(r.last[1]) == (i == 1)
        r = eng.step(4)  # rows 0/1 have delivered their last frame: only n = 1 rows are open
        assert eng.lsd_steps()[1] == 1
        assert not r.valid[0] and not r.valid[1]
        rows.check(r, [2, 3])
        admit(0, 2, 3)
        for i in range(3):
            r = eng.step(4)
            assert eng.lsd_steps()[1] == 2
            assert not r.valid[1]
            rows.check(r, [0, 2, 3])
        assert r.last[0] and r.last[2] and r.last[3]
        assert rows.got == {0: 3, 1: 2, 2: 6, 3: 6}
        assert not eng.step(4).valid.any()
    finally:
        eng.close()


def test_default_count_is_the_cap(oracle):
    """Rows opened without a count of their own (GenerationParams.lsd_steps None, the admission
    calls as they were) run the engine's lsd_decode_steps = 3."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(9)
    eng = pt.Engine(device=0, max_slots=3, max_ctx=64, lsd_decode_steps=3, seed=0x5EED)
    try:
        rows = Rows(oracle, 64)
        for b in range(3):
            prompt = (d["prompt"][: 4 + b] * (1.0 + 0.08 * b)).astype(np.float32)
            ids = rng.integers(0, 4000, size=2 + b).astype(np.int32)
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(max_frames=2))
            rows.add(b, prompt, ids, 3)
        for _ in range(2):
            rows.check(eng.step(3), range(3))
            assert eng.lsd_steps() == (3, 3)
    finally:
        eng.close()


def test_mixed_rows_multi_launch_head(oracle):
    """B = 136 (past the persistent launch's 128 rows): the head's GEMM + row-reduce launches with
    the per-row Euler epilogue. n_b = 1 + b % 2, cap 2; probe rows 0 and 70 use n = 1, 135 n = 2."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(5)
    B, steps, probe = 136, 2, (0, 70, 135)
    eng = pt.Engine(device=0, max_slots=B, max_ctx=32, lsd_decode_steps=2, seed=0x5EED)
    try:
        assert "head.chain" not in eng.plan_ops(B)
        base = eng.voice_from_prompt(d["prompt"][:3])
        rows = Rows(oracle, 32)
        slots, vs, ids_l, ps = [], [], [], []
        for b in range(B):
            n = 1 + b % 2
            if b in probe:
                prompt = (d["prompt"][:4] * (1.0 + 0.1 * probe.index(b))).astype(np.float32)
                ids = rng.integers(0, 4000, size=3).astype(np.int32)
                v = eng.voice_from_prompt(prompt)
                rows.add(b, prompt, ids, n)
            else:
                v, ids = base, np.array([260, 261], np.int32)
            slots.append(b), vs.append(v), ids_l.append(ids), ps.append(params(max_frames=steps, lsd_steps=n))
        eng.open_many(slots, vs, ids_l, ps)
        assert {rows.n[b] for b in probe} == {1, 2}
        for _ in range(steps):
            r = eng.step(B)
            rows.check(r, probe)
            assert eng.lsd_steps() == (2, 2)
    finally:
        eng.close()


def test_mixed_rows_pipelined_pairs(oracle):
    """pipeline=True, back_frames=2: 4 rows with n = 1, 2, 2, 1 (cap 2), 6 frames each, the last
    ones delivered by flush calls. Every delivered frame equals its oracle's."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(17)
    frames = 6
    eng = pt.Engine(device=0, max_slots=4, max_ctx=128, lsd_decode_steps=2, seed=0x5EED, pipeline=True,
                    back_frames=2)
    try:
        rows = Rows(oracle, 128)
        vs, ids_l, ps = [], [], []
        for b, n in enumerate((1, 2, 2, 1)):
            prompt = (d["prompt"][: 5 + 2 * b] * (1.0 + 0.04 * b)).astype(np.float32)
            ids = rng.integers(0, 4000, size=3 + 2 * b).astype(np.int32)
            vs.append(eng.voice_from_prompt(prompt)), ids_l.append(ids)
            ps.append(params(max_frames=frames, lsd_steps=n))
            rows.add(b, prompt, ids, n)
        eng.open_many([0, 1, 2, 3], vs, ids_l, ps)
        lag, delay = eng.frame_lag()
        assert (lag, delay) == (3, 0)
        for _ in range(frames):
            rows.check(eng.step(4))
            assert eng.lsd_steps()[1] == 2
        for _ in range(lag):
            eng.flush_async(4)
            rows.check(eng.fetch(4))
        assert rows.got == {b: frames for b in range(4)}
    finally:
        eng.close()


def test_mixed_rows_int8(oracle):
    """weight_quant=1 (int8 codes in the FlowLM step GEMMs, the adaLN GEMM among them at M =
    lsd_run * B rows), cap 2, rows with n = 1 and n = 2, against the quantized oracle at
    tests/test_quantize.py's gates (LAT_TOL, PCM_TOL)."""
    import pocket_tts_amd as pt
    from _oracle import Oracle

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(21)
    eng = pt.Engine(device=0, max_slots=2, max_ctx=256, lsd_decode_steps=2, seed=0x5EED, weight_quant=1)
    try:
        rows = Rows(Oracle(0x5EED, 1), 256)
        for b, n in enumerate((1, 2)):
            prompt = (d["prompt"][: 6 + 2 * b] * (1 + 0.05 * b)).astype(np.float32)
            ids = rng.integers(0, 4000, size=3 + b).astype(np.int32)
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(max_frames=4, lsd_steps=n))
            rows.add(b, prompt, ids, n)
        for _ in range(4):
            rows.check(eng.step(2), range(2))
    finally:
        eng.close()


def test_count_outside_the_cap_is_refused(oracle):
    """lsd_steps of cap + 1 and of -1: PTTS_ERR_INVALID with a message, nothing admitted; the
    engine steps correctly afterwards."""
    import ctypes as C

    import pocket_tts_amd as pt
    from pocket_tts_amd._lib import lib

    d = load_golden("e2e_lsd1.safetensors")
    prompt, ids = d["prompt"][:5].astype(np.float32), np.array([260, 2994, 262], np.int32)
    eng = pt.Engine(device=0, max_slots=2, max_ctx=64, lsd_decode_steps=2, seed=0x5EED)
    try:
        v = eng.voice_from_prompt(prompt)
        for bad in (3, -1):
            with pytest.raises(pt.PocketTTSError, match="lsd_steps") as e:
                eng.open(0, v, ids, params(max_frames=2, lsd_steps=bad))
            assert e.value.code == 1
            with pytest.raises(pt.PocketTTSError, match="lsd_steps"):
                eng.open_many([0, 1], [v, v], [ids, ids], [params(max_frames=2), params(max_frames=2, lsd_steps=bad)])
        cp = params(max_frames=2).to_c()
        a = np.ascontiguousarray(ids)
        rc = lib().ptts_slot_open_ex(eng.handle, 0, v.handle, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size,
                                     C.byref(cp), 3)
        assert rc == 1 and b"lsd_steps" in lib().ptts_last_error()
        assert not eng.step(2).valid.any()  # nothing was admitted
        rows = Rows(oracle, 64)
        eng.open(1, v, ids, params(max_frames=2, lsd_steps=1))
        rows.add(1, prompt, ids, 1)
        for _ in range(2):
            r = eng.step(2)
            assert not r.valid[0]
            rows.check(r, [1])
    finally:
        eng.close()
