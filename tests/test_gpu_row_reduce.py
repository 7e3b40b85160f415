"""The row reduce on its own (ptts_test_row_reduce: the product launcher row_reduce, unchanged)
against the float64 formula, on shapes and operand sets the model never runs:

    v = sum_z p[z] (+ bias); v = act(v); v *= gate; v += r; y = v
    h = LN(v) (biased variance, eps) (* ln_w + ln_b) (* (1 + mscale) + mshift)

The slabs and the bias / gate / residual operands of a launch are requested in one level, absent
ones from a stand-in address and dropped by a select: a wrong stand-in or a select on the wrong
flag shows as an operand applied (or missing) in full. M = 3; N = 512 (k_row_reduce4 outside the front part, k_row_reduce inside it), 1024 (with
the A-fragment copy Hfrag) and, without LayerNorm, 3072 (three column blocks); S = 1, 3, 8.

The bound is computed, not stated: four times the largest |f32 - f64| over the case's elements,
where f32 is the same formula evaluated with numpy in float32 in the kernel's summation order
(slabs in z order; a row's sums per float4 quad, then the wave's xor butterfly, then the four
waves pairwise), per output (y, h). The CPU test holds that evaluation itself to the bound and the
bound to a few roundings of the largest value."""

import itertools

import numpy as np
import pytest

M = 3
F32 = np.float32


def gelu(x, dt):
    c = dt.type
    return c(0.5) * x * (c(1.0) + np.tanh(c(0.7978845608028654) * (x + c(0.044715) * x * x * x)))


def block_sum(t, dt):
    """Sum of the row's per-thread values t [256] as block_sum() forms it: the xor butterfly of each
    64-lane wave, then (w0 + w1) + (w2 + w3)."""
    w = t.reshape(4, 64).astype(dt)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, lanes ^ o]).astype(dt)
    return ((w[0, 0] + w[1, 0]).astype(dt) + (w[2, 0] + w[3, 0]).astype(dt)).astype(dt)


def evaluate(c, dtype):
    """(y, h) of case c in `dtype`, in the kernel's order (for float64: the formula)."""
    dt = np.dtype(dtype)
    f = lambda a: None if a is None else a.astype(dt)
    p = f(c["p"])
    v = p[0]
    for z in range(1, p.shape[0]):
        v = (v + p[z]).astype(dt)
    if c["bias"] is not None:
        v = (v + f(c["bias"])).astype(dt)
    if c["act"]:
        v = gelu(v, dt).astype(dt)
    if c["gate"] is not None:
        v = (v * f(c["gate"])).astype(dt)
    if c["r"] is not None:
        v = (v + f(c["r"])).astype(dt)
    if not c["ln"]:
        return v, None
    n = v.shape[1]
    h = np.empty_like(v)
    for m in range(v.shape[0]):
        quads = v[m].reshape(-1, 4)
        t = np.zeros(256, dt)
        t[:n // 4] = ((quads[:, 0] + quads[:, 1]).astype(dt) + (quads[:, 2] + quads[:, 3]).astype(dt)).astype(dt)
        mean = (block_sum(t, dt) / dt.type(n)).astype(dt)
        d = (v[m] - mean).astype(dt)
        dq = (d * d).astype(dt).reshape(-1, 4)
        t = np.zeros(256, dt)
        t[:n // 4] = ((dq[:, 0] + dq[:, 1]).astype(dt) + (dq[:, 2] + dq[:, 3]).astype(dt)).astype(dt)
        den = np.sqrt((block_sum(t, dt) / dt.type(n)).astype(dt) + dt.type(c["eps"])).astype(dt)
        hh = (d / den).astype(dt)
        if c["ln_w"] is not None:
            hh = ((hh * f(c["ln_w"])).astype(dt) + f(c["ln_b"])).astype(dt)
        if c["mscale"] is not None:
            hh = ((hh * (dt.type(1.0) + f(c["mscale"])[m]).astype(dt)).astype(dt) + f(c["mshift"])[m]).astype(dt)
        h[m] = hh
    return v, h


def make_case(n, s, ops, act, ln, front, seed):
    rng = np.random.default_rng(seed)
    g = lambda *shape, scale=1.0, loc=0.0: (loc + scale * rng.standard_normal(shape)).astype(F32)
    c = dict(n=n, s=s, act=act, ln=ln, front=front, eps=1e-5, hfrag=bool(ln and n == 1024))
    c["p"] = g(s, M, n)
    c["bias"] = g(n) if "bias" in ops else None
    c["gate"] = g(M, n) if "gate" in ops else None
    c["r"] = g(M, n) if "r" in ops else None
    c["ln_w"] = g(n, scale=0.3, loc=1.0) if "affine" in ops else None
    c["ln_b"] = g(n, scale=0.3) if "affine" in ops else None
    c["mscale"] = g(M, n, scale=0.5) if "mod" in ops else None
    c["mshift"] = g(M, n) if "mod" in ops else None
    c["name"] = f"n{n}_S{s}_{'+'.join(ops) or 'plain'}_{'gelu' if act else 'id'}_{'ln' if ln else 'raw'}_f{front}"
    return c


ALL_LN = ("bias", "gate", "r", "affine", "mod")
ALL_RAW = ("bias", "gate", "r")


def cases():
    out, seed = [], 100
    for n, s in itertools.product((512, 1024), (1, 3, 8)):
        for front in ((0, 1) if n == 512 else (1,)):  # 512 outside the front part: k_row_reduce4
            out.append(make_case(n, s, ALL_LN, 1, 1, front, seed := seed + 1))
            out.append(make_case(n, s, (), 0, 1, front, seed := seed + 1))
    for op in ALL_LN:  # each operand alone
        out.append(make_case(1024, 3, (op,), 0, 1, 1, seed := seed + 1))
    out.append(make_case(1024, 3, (), 1, 1, 1, seed := seed + 1))  # GELU alone
    for s in (1, 3, 8):  # three column blocks, no LayerNorm
        out.append(make_case(3072, s, ALL_RAW, 1, 0, 1, seed := seed + 1))
        out.append(make_case(3072, s, (), 0, 0, 1, seed := seed + 1))
    for op in ALL_RAW:
        out.append(make_case(3072, 3, (op,), 0, 0, 1, seed := seed + 1))
    out.append(make_case(512, 3, ALL_RAW, 1, 0, 0, seed := seed + 1))  # k_row_reduce4 without statistics
    out.append(make_case(512, 3, (), 0, 0, 0, seed := seed + 1))
    return out


CASES = cases()


def reference(c):
    """(y64, h64, bound_y, bound_h, err of the f32 evaluation for y, for h)."""
    y64, h64 = evaluate(c, np.float64)
    y32, h32 = evaluate(c, np.float32)
    assert y32.dtype == np.float32 and (h32 is None or h32.dtype == np.float32)
    ey = float(np.abs(y32.astype(np.float64) - y64).max())
    eh = float(np.abs(h32.astype(np.float64) - h64).max()) if c["ln"] else 0.0
    return y64, h64, 4.0 * ey, 4.0 * eh, ey, eh


def afrag_index(row, k):
    """gemv_fk's A-fragment order (kernels.hip fk_afrag_index): the float index of (row, k)."""
    w, g, s, t, r = k >> 7, (k >> 5) & 3, k & 31, row >> 4, row & 15
    return ((((w * 2 + t) * 8 + (s >> 2)) * 64 + (g * 16 + r)) << 2) + (s & 3)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_float32_evaluation_passes_its_own_bound(c):
    """CPU: the float32 evaluation the bound comes from lies within it, and the bound is a few
    roundings of the largest value: at most 64 u per output (u = 2^-24; a slab sum of 8 terms,
    GELU's 8 operations with tanh, the gate and the residual; LayerNorm's mean, difference,
    division, affine and modulate), not a loose one."""
    y64, h64, by, bh, ey, eh = reference(c)
    assert ey <= by and eh <= bh
    assert by <= 4 * 64 * 2.0 ** -24 * np.abs(y64).max()
    if c["ln"]:
        assert 0.0 < bh <= 4 * 64 * 2.0 ** -24 * np.abs(h64).max()


@pytest.fixture(scope="module")
def eng():
    import pocket_tts_amd as pt

    e = pt.Engine(device=0, max_slots=1, max_ctx=64, seed=0x5EED)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_row_reduce_matches_fp64(eng, c):
    y64, h64, by, bh, _, _ = reference(c)
    y, h, hf = eng.test_row_reduce(c["p"], bias=c["bias"], gate=c["gate"], r=c["r"], act=c["act"], ln=bool(c["ln"]),
                                   eps=c["eps"], ln_w=c["ln_w"], ln_b=c["ln_b"], mscale=c["mscale"],
                                   mshift=c["mshift"], hfrag=c["hfrag"], front=bool(c["front"]))
    ey = float(np.abs(y.astype(np.float64) - y64).max())
    eh = float(np.abs(h.astype(np.float64) - h64).max()) if c["ln"] else 0.0
    print(f"{c['name']}: y err {ey:.3g} (bound {by:.3g}), h err {eh:.3g} (bound {bh:.3g})")
    assert np.isfinite(y).all() and ey <= by, (c["name"], "y", ey, by)
    if c["ln"]:
        assert np.isfinite(h).all() and eh <= bh, (c["name"], "h", eh, bh)
    else:
        assert h is None
    if c["hfrag"]:
        rows, ks = np.meshgrid(np.arange(M), np.arange(c["n"]), indexing="ij")
        idx = afrag_index(rows, ks)
        assert np.array_equal(hf[idx].view(np.uint32), h.view(np.uint32)), (c["name"], "hfrag differs from h")
        rest = np.ones(hf.size, bool)
        rest[idx.ravel()] = False
        assert not hf[rest].any(), (c["name"], "hfrag written outside the rows")
