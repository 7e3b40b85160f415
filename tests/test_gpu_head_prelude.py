"""The flow head's prelude as one launch (`head.prelude`, k_head_prelude): cond | EOS on the whole-K
GEMM, silu(c + temb) handed to the adaLN GEMM inside the launch, the rows' noise, x0 and the
chain's emptied regions as side jobs. It runs on f32 engines for B <= 32 rows ahead of the
persistent chain; every other case keeps the four launches it replaces.

Synthetic weights (seed 0x5EED), max_ctx <= 64, 3 steps per case; every row is compared with its
own oracle run at the suite's fp32 gates (conftest.py: LAT_TOL on latents and EOS logits, PCM_TOL
on PCM)."""

import numpy as np
import pytest
from conftest import LAT_TOL, PCM_TOL, load_golden, pcm_err
from test_gpu_parity import _noise

pytestmark = pytest.mark.gpu

INF = float("inf")
OLD = ("head.cond_eos_gemm", "head.flow_cond", "head.ada_gemm", "head.ada_reduce")
STEPS = 3
TEMP, CLAMP = 0.7, 0.5  # the one sampled row of a batch


def params(**kw):
    from pocket_tts_amd import GenerationParams

    base = dict(temp=0.0, eos_threshold=INF, noise_clamp=None, frames_after_eos=3, max_frames=STEPS, seed=1)
    base.update(kw)
    return GenerationParams(**base)


def request(d, rng, b):
    """row b's own prompt and text"""
    prompt = (d["prompt"][: 3 + (b % 5)] * (1.0 + 0.05 * b)).astype(np.float32)
    ids = rng.integers(0, 4000, size=2 + b % 3).astype(np.int32)
    return prompt, ids


class Row:
    """The oracle side of one engine row: its state, step count, sampling and last latent."""

    def __init__(self, oracle, prompt, ids, n=1, hot_seed=None):
        self.s = oracle.new_state(64)
        self.s.prefill(prompt)
        self.s.prefill_tokens(ids)
        self.n, self.hot_seed, self.lat, self.i = n, hot_seed, None, 0

    def check(self, r, b):
        noise = None if self.hot_seed is None else _noise(self.hot_seed, self.i, TEMP, CLAMP)
        o = self.s.step(self.lat, noise=noise, lsd_steps=self.n)
        self.lat = o["latent"]
        self.i += 1
        e_eos = abs(float(r.eos_logits[b]) - o["eos_logit"])
        e_lat = float(np.abs(r.latents[b] - o["latent"]).max())
        e_pcm = pcm_err(r.pcm[b] - o["pcm"])
        assert r.valid[b], b
        assert e_eos <= LAT_TOL and e_lat <= LAT_TOL and e_pcm <= PCM_TOL, (b, self.i, e_eos, e_lat, e_pcm)


@pytest.mark.parametrize("lsd", [1, 3])
@pytest.mark.parametrize("B", [1, 17, 32])
def test_parity(oracle, B, lsd):
    """B = 1: one valid row in a 16-row tile; 17: a second tile with one valid row (the sampled
    one); 32: the full grid. lsd = 3 runs the consumers' loop over Euler steps with the weights
    held; at B = 17 the rows' own counts differ (n = 1 + b % 3: each row's own time embeddings),
    elsewhere every row runs the cap. All rows at temp 0 but the last (temp 0.7, clamp 0.5)."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(31)
    eng = pt.Engine(device=0, max_slots=B, max_ctx=64, lsd_decode_steps=lsd, seed=0x5EED)
    try:
        names = eng.plan_ops(B)
        assert "head.prelude" in names and "head.chain" in names
        rows = []
        for b in range(B):
            prompt, ids = request(d, rng, b)
            n = 1 + b % 3 if (lsd == 3 and B == 17) else lsd
            hot = 900 + b if b == B - 1 else None
            p = params(lsd_steps=n) if hot is None else params(lsd_steps=n, temp=TEMP, noise_clamp=CLAMP, seed=hot)
            eng.open(b, eng.voice_from_prompt(prompt), ids, p)
            rows.append(Row(oracle, prompt, ids, n, hot))
        for _ in range(STEPS):
            r = eng.step(B)
            for b in range(B):
                rows[b].check(r, b)
    finally:
        eng.close()


def test_plan():
    """head.prelude replaces the four launches for B <= 32 on an f32 engine only: B = 33 and the
    engines that stream weight codes (weight_quant, fp8_gemm) keep them, under their names."""
    import pocket_tts_amd as pt

    def split(eng, B):
        names = eng.plan_ops(B)
        return "head.prelude" in names, [n for n in OLD if n in names]

    eng = pt.Engine(device=0, max_slots=33, max_ctx=16, lsd_decode_steps=1, seed=0x5EED)
    try:
        for B in (1, 17, 32):
            assert split(eng, B) == (True, []), B
        assert split(eng, 33) == (False, list(OLD))
    finally:
        eng.close()
    for kw in (dict(fp8_gemm=True), dict(weight_quant=1)):
        eng = pt.Engine(device=0, max_slots=32, max_ctx=16, lsd_decode_steps=1, seed=0x5EED, **kw)
        try:
            assert split(eng, 32) == (False, list(OLD)), kw
        finally:
            eng.close()


def test_replay_rearms_the_handoff(oracle):
    """The launch replayed alone in a timing loop (each replay behind its prep) leaves its hand-off
    regions as a step finds them: the steps after it equal the oracle like the one before it.
    B = 5 at cap 2: two Euler steps' regions."""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(32)
    B = 5
    eng = pt.Engine(device=0, max_slots=B, max_ctx=64, lsd_decode_steps=2, seed=0x5EED)
    try:
        rows = []
        for b in range(B):
            prompt, ids = request(d, rng, b)
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(lsd_steps=2))
            rows.append(Row(oracle, prompt, ids, 2))
        for i in range(STEPS):
            if i == 1:
                assert eng.time_kernel(B, "head.prelude", reps=20) > 0
            r = eng.step(B)
            for b in range(B):
                rows[b].check(r, b)
    finally:
        eng.close()


def run_at(B, row, lsd=1):
    """latents and EOS logits of one fixed request at row `row` of B-row steps (the other rows hold
    requests of their own)"""
    import pocket_tts_amd as pt

    d = load_golden("e2e_lsd1.safetensors")
    rng = np.random.default_rng(33)
    eng = pt.Engine(device=0, max_slots=B, max_ctx=64, lsd_decode_steps=lsd, seed=0x5EED)
    try:
        for b in range(B):
            prompt, ids = request(d, rng, b + 1)
            if b == row:
                prompt, ids = d["prompt"][:6].astype(np.float32), np.array([260, 2994, 262], np.int32)
            eng.open(b, eng.voice_from_prompt(prompt), ids, params(temp=TEMP, noise_clamp=CLAMP, seed=77))
        out = [eng.step(B) for _ in range(STEPS)]
        return np.stack([r.latents[row] for r in out]), np.array([r.eos_logits[row] for r in out])
    finally:
        eng.close()


def test_row_result_depends_on_neither_batch_nor_row():
    """The same request at row 0 of a 1-row call and at row 19 of a 20-row call: bit-identical
    latents and EOS logits (fixed summation orders, no tile choice that depends on B)."""
    lat1, eos1 = run_at(1, 0)
    lat20, eos20 = run_at(20, 19)
    assert np.array_equal(lat1.view(np.uint32), lat20.view(np.uint32))
    assert np.array_equal(eos1.view(np.uint32), eos20.view(np.uint32))
