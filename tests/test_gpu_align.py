"""The align stage's kernel on its own (ptts_test_align: the product launcher align_step, k_align)
against a float64 softmax over the text keys, on operands the model never produces. On the synthetic
weights every softmax over the text is almost flat, so an engine run alone would hardly move the max
subtraction, the head mean or the masks.

What the kernel computes for row r = slot r with table entry {t0, n}, n >= 1, at position pos:
q_h = RoPE(sum of the q column's slabs in z order, at min(pos, cap - 1)), s_j = q_h . K_h[t0 + j] / 8
over the slot's own store, p_h = softmax_j s over j < n, a_j = mean over the heads of the mask.

Reference: the f32 slab sum in z order (the kernel's own order, exact to state), rotated in float64
by the angle the kernels form, theta = float32(pos) * float32(f_i), then everything in float64.

Bound (not tuned; the error model of tests/test_gpu_attention_core.py, restated). Per score of head h
    E_j = u sum_i |q_i k_ji|  +  sum_i rtol(q)_i |k_ji| / 8  +  6 u  +  3 u |s_j - max s|,   u = 2^-24:
the 64-term f32 dot (sqrt(64) roundings of u relative to sum |q_i k_i|, times 1/8), the RoPE gate of q
carried through the dot,
    rtol(q) per rotation pair = (|x0| + |x1|) (dtheta + 8 u),  dtheta = theta (a_i 2^-22 + 4 u) + theta 2 u,
    a_i = i ln(1e4) / 32
(the device's f_i = expf(i c) is off by a_i 2^-22 relative, expf and the reference's rounding 4 u, the
product pos f_i 2 u, cosf / sinf and the rotation's three roundings 8 u), the expf calls (6 u) and the
rounding of their arguments (3 u |s_j - max|). A perturbation e of the logits moves p_j by
p_j (e_j - sum_k p_k e_k), so
    |a_j - ref_j| <= 4 mean_h p_hj (E_hj + sum_k p_hk E_hk) + 8 u,
4 the project's usual margin, 8 u for the division, the head sum and the mean. Each test prints the
worst err / bound of its case.

Exact cases: equal scores give e_j = 1 for every key and a sum of n, so every a_j is the f32 quotient
1 / n (the masks select 1, 2 or 16 heads: the head mean is exact); a row with n == 0 comes back with
count 0 and its sentinel floats untouched; the floats behind n are zero."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ARG = np.arange(32) * (np.log(1e4) / 32)
FREQ = np.exp(-ARG).astype(np.float32)
NH, CAP, TOK = 16, 160, 128
SENTINEL = np.float32(-777.25)
MASKS = [1 << 3, 1 | 1 << 15, 0xFFFF]
NS = [1, 3, 64, 65, 128]
SLABS = [0, 1, 8, 16]  # 0: dense rows
KINDS = ["random", "equal", "spike", "span"]


@pytest.fixture(scope="module")
def eng():
    import pocket_tts_amd as pt

    e = pt.Engine(device=0, max_slots=1, max_ctx=64, seed=0x5EED)
    yield e
    e.close()


def angles(pos):
    return (np.asarray(pos, np.float32)[..., None] * FREQ).astype(np.float32).astype(np.float64)


def rope64(x, pos):
    x = np.asarray(x, np.float64)
    th = angles(pos)
    cs, sn = np.cos(th), np.sin(th)
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * cs - x[..., 1::2] * sn
    y[..., 1::2] = x[..., 0::2] * sn + x[..., 1::2] * cs
    return y


def rope_tol(x, pos):
    x = np.abs(np.asarray(x, np.float64))
    th = angles(pos)
    dth = th * (ARG * 2.0 ** -22 + 4 * U) + th * 2 * U
    return np.repeat((x[..., 0::2] + x[..., 1::2]) * (dth + 8 * U), 2, axis=-1)


def slab_sum(slabs):
    acc = np.zeros(slabs.shape[1:], np.float32)
    for z in range(slabs.shape[0]):
        acc = (acc + slabs[z]).astype(np.float32)
    return acc


def heads_of(mask):
    return [h for h in range(NH) if mask >> h & 1]


def reference(q32, K, qp, mask):
    """(a [n], bound [n]) of one row: q32 [NH][64] the f32 slab sums, K [NH][n][64] its text keys."""
    a = tol = 0.0
    hs = heads_of(mask)
    for h in hs:
        q, rt, k = rope64(q32[h], qp), rope_tol(q32[h], qp), K[h].astype(np.float64)
        s = k @ q / 8.0
        p = np.exp(s - s.max())
        p /= p.sum()
        E = U * (np.abs(k) @ np.abs(q)) + (np.abs(k) @ rt) / 8.0 + 6 * U + 3 * U * np.abs(s - s.max())
        a = a + p
        tol = tol + p * (E + p @ E)
    return a / len(hs), 4.0 * tol / len(hs) + 8 * U


def make_case(seed, n, S, t0, kind):
    """Three rows: row 0 and row 2 (at pos == cap) in the stage with n tokens from t0, row 1 not."""
    rng = np.random.default_rng(seed)
    pos = np.array([t0 + n + 3, 9, CAP], np.int32)
    tab = np.array([[t0, n], [4, 0], [t0, n]], np.int32)
    d = NH * 64
    q = rng.standard_normal((3, NH, 64)).astype(np.float32)
    kv = (0.5 * rng.standard_normal((3, 2, NH, CAP, 64))).astype(np.float32)
    qp = np.minimum(pos, CAP - 1)
    for r in (0, 2):
        spike = int(rng.integers(n))  # the same token in every head: the head mean keeps p -> 1
        for h in range(NH):
            qr = rope64(q[r, h], qp[r])
            qhat = qr / np.linalg.norm(qr)
            keys = kv[r, 0, h, t0:t0 + n]
            if kind == "equal":  # one vector for every key: bit-equal scores
                keys[:] = keys[0]
            elif kind == "spike":  # one key along q at 30 x the norm of the others: p -> 1
                keys[spike] = (30.0 * np.linalg.norm(keys, axis=1).max() * qhat).astype(np.float32)
            elif kind == "span":  # scores from -80 to 80
                sj = np.linspace(-80.0, 80.0, n) if n > 1 else np.array([80.0])
                noise = 0.05 * rng.standard_normal((n, 64))
                noise -= np.outer(noise @ qhat, qhat)
                keys[:] = (np.outer(sj * 8.0 / np.linalg.norm(qr), qhat) + noise).astype(np.float32)
    rows = np.zeros((3, 3 * d), np.float32)
    rows[:, :d] = q.reshape(3, d)
    rows[:, d:] = rng.standard_normal((3, 2 * d)).astype(np.float32)  # k | v columns: not read
    if S == 0:
        qkv = rows
    else:  # S slabs that sum (in f32, z order) to something near rows; the reference sums them itself
        parts = rng.standard_normal((S, 3, 3 * d)).astype(np.float32)
        parts[S - 1] = rows - parts[:S - 1].sum(axis=0, dtype=np.float32)
        qkv = parts
    return qkv, kv, pos, tab


def run_case(eng, n, S, t0, with_pre, mask, kind, seed):
    qkv, kv, pos, tab = make_case(seed, n, S, t0, kind)
    pre = None
    if with_pre:  # prefixes that claim the first text positions too, filled with large values
        rng = np.random.default_rng(seed + 1)
        pre = [(50.0 * rng.standard_normal((2, NH, t0 + 2, 64))).astype(np.float32) for _ in range(3)]
    out0 = np.full((3, 1 + TOK), SENTINEL, np.float32)
    cnt, rows = eng.test_align(qkv, kv, pos, tab, mask, out0, pre=pre)
    assert cnt.tolist() == [n, 0, n]
    assert np.array_equal(rows[1], out0[1, 1:]), "a row outside the stage had its floats written"
    q32 = (slab_sum(qkv) if S else qkv)[:, :NH * 64].reshape(3, NH, 64)
    worst = 0.0
    for r in (0, 2):
        assert np.all(rows[r, n:] == 0.0), "floats behind n"
        got = rows[r, :n].astype(np.float64)
        ref, tol = reference(q32[r], kv[r, 0][:, t0:t0 + n], min(int(pos[r]), CAP - 1), mask)
        ratio = np.abs(got - ref) / tol
        worst = max(worst, float(ratio.max()))
        assert np.all(got >= 0) and abs(got.sum() - 1.0) <= n * 4 * U
        if kind == "equal":
            assert np.all(rows[r, :n] == np.float32(1.0) / np.float32(n)), (r, rows[r, :n])
        if kind == "spike":
            assert got.max() >= 1.0 - 1e-6
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_align_rows_against_float64(eng, n, kind):
    """Every slab form for this (n, operands), with t0, the prefix tables and the head mask cycling
    so that each value of each meets every n and every operand kind across the module."""
    worst = 0.0
    for i, S in enumerate(SLABS):
        c = i + NS.index(n) + KINDS.index(kind)
        t0, with_pre, mask = (0, 5)[c % 2], bool((c // 2) % 2), MASKS[c % 3]
        w = run_case(eng, n, S, t0, with_pre, mask, kind, seed=1000 * n + 10 * i + KINDS.index(kind))
        print(f"n {n} {kind}: slabs {S} t0 {t0} pre {with_pre} mask {mask:#06x}: worst err / bound {w:.3f}")
        worst = max(worst, w)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("t0,with_pre", [(0, False), (0, True), (5, False), (5, True)])
def test_align_masks_and_prefix_tables(eng, mask, t0, with_pre):
    """The full cross of masks x t0 x prefix tables at the two-block size n = 65 (8 slabs)."""
    w = run_case(eng, 65, 8, t0, with_pre, mask, "random", seed=77 + t0 + mask % 13)
    print(f"mask {mask:#06x} t0 {t0} pre {with_pre}: worst err / bound {w:.3f}")
    assert w <= 1.0, w


def test_align_refusals(eng):
    import pocket_tts_amd as pt

    qkv, kv, pos, tab = make_case(1, 3, 0, 0, "random")
    out0 = np.zeros((3, 1 + TOK), np.float32)
    with pytest.raises(pt.PocketTTSError):  # no head of the mask among the 16
        eng.test_align(qkv, kv, pos, tab, 1 << 16, out0)
    bad = tab.copy()
    bad[0] = (CAP - 2, 3)  # text keys past the store
    with pytest.raises(pt.PocketTTSError):
        eng.test_align(qkv, kv, pos, bad, 1, out0)
    bad[0] = (0, TOK + 1)
    with pytest.raises(pt.PocketTTSError):
        eng.test_align(qkv, kv, pos, bad, 1, out0)
