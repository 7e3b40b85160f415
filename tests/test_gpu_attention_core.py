"""The attention path on its own (ptts_test_attention: the product launchers, unchanged) against a
float64 softmax attention, on operands the model never produces. End-to-end parity on the synthetic
weights leaves these kernels nearly untested: the weights give logits of sigma ~ 0.3, so every
softmax is almost flat (each of 250 keys weighs ~ 1/250) and the max subtraction, the online
rescale between key tiles, the waves' (m, l, o) merge and the mask edges hardly move the output.

Kinds: A = qkv_rope_append + attention (k_qkv_rope, k_attn16<RING>), B = attention16_qkv
(k_attn16<true, true>, RoPE and the ring append fused), C = attention_step_qkv (k_attn_decode_qkv
with the engine's rope_table). Every case is checked in two layers, so that RoPE rounding stays out
of the softmax gate.

RoPE and append. Stored K (and, kind A, the rotated Q) against the float64 rotation by the angle
the kernels form, theta = float32(pos) * float32(f_i), f_i = exp(-a_i), a_i = i ln(1e4) / 32. Gate
per rotation pair (x0, x1), both outputs:
    (|x0| + |x1|) * (dtheta + 8 u),   u = 2^-24,
    dtheta = theta * (a_i 2^-22 + 4 u) + theta * 2 u.
The device forms f_i = expf(float(i) * c) with c = -logf(1e4) * 2 / 64 in f32: c carries up to one
ulp (2^-23 relative), the product i * c half an ulp more, so the exponent is off by at most
a_i * (2^-23 + 2^-24) <= a_i 2^-22, which is the relative error of f_i; expf adds one ulp (2 u) and
the reference's own rounding of f_i to f32 half an ulp (u): 4 u with one u to spare. That relative
error times theta is position * ulp(f_i) in the issue's words. The f32 product pos * f_i rounds
once on each side (theta * 2 u), cosf / sinf are good to 2 ulp (4 u) and the two products and the
sum of a rotation round three times (3 u): 8 u with one to spare. Stored V and every store element
the call must not touch are bit-equal to the input (V of slab input: to the f32 sum in slab order).

Softmax and P V. O against the float64 attention over the store and the Q the device produced
(kind A) or the float64 rotation of q (B, C), mask kp <= qp and (window == 0 or qp - kp < window),
logits s_j = q . k_j / 8. First-order bound per output element d of a query with weights p_j:
    tol_d = 4 * ( sum_j p_j (E_j + sum_k p_k E_k) |v_jd - O_d|  +  sqrt(n + 8) u (sum_j p_j |v_jd| + |O_d|) )
    E_j = u sum_i |q_i k_ji|  [+ sum_i rtol(q)_i |k_ji| / 8 for B, C]  +  6 u + 3 u |s_j - max s|
A perturbation e_j of the logits moves O by sum_j p_j (e_j - sum_k p_k e_k) (v_j - O): the spread of V
under the weights. E_j holds the logit error of a 64-term f32 dot, sqrt(64) roundings of u relative
to sum |q_i k_i|, times 1/8 (and, where the reference rotates q itself, the RoPE gate rtol of q
carried through the dot); three expf of one ulp each (the tile's, the online rescale, the merge:
6 u) and the rounding of their three arguments (3 u |s_j - max|). The second term is the f32
accumulation of P V and of the denominator over n visible keys plus the 8-wave merge, sqrt(n + 8)
roundings relative to sum p |v|; weights under FLT_MIN = 2^-126, which f32 loses, add n max|v| 2^-126
(it matters only where a spike's V element is ~ 0). 4 is the project's usual margin. Achieved
errors are printed per test as the worst ratio err / tol (MI355X: RoPE <= 0.27 of its gate in every
kind, O <= 0.17 for A, 0.13 for B, 0.12 for C)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ARG = np.arange(32) * (np.log(1e4) / 32)
FREQ = np.exp(-ARG).astype(np.float32)
A, B, C = 0, 1, 2
SPIKE = 76.0  # logit of the spike key over a key orthogonal to the spike direction


@pytest.fixture(scope="module")
def eng():
    import pocket_tts_amd as pt

    e = pt.Engine(device=0, max_slots=1, max_ctx=64, seed=0x5EED)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------
def angles(pos):
    """theta [..., 32] as the kernels form it: float32(pos) * float32(f_i), rounded to f32."""
    return (np.asarray(pos, np.float32)[..., None] * FREQ).astype(np.float32).astype(np.float64)


def rope64(x, pos, inverse=False):
    """x [..., 64] rotated pairwise by theta(pos) in float64; pos broadcasts over x's leading axes."""
    x = np.asarray(x, np.float64)
    th = angles(pos)
    cs, sn = np.cos(th), np.sin(th) * (-1.0 if inverse else 1.0)
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * cs - x[..., 1::2] * sn
    y[..., 1::2] = x[..., 0::2] * sn + x[..., 1::2] * cs
    return y


def rope_tol(x, pos):
    """The RoPE gate of the module docstring for x [..., 64] at pos."""
    x = np.abs(np.asarray(x, np.float64))
    th = angles(pos)
    dth = th * (ARG * 2.0 ** -22 + 4 * U) + th * 2 * U
    return np.repeat((x[..., 0::2] + x[..., 1::2]) * (dth + 8 * U), 2, axis=-1)


def slab_sum(slabs):
    """f32 sum over the leading axis in slab order, from 0 (k_qkv_rope's loop, slab_sum())."""
    acc = np.zeros(slabs.shape[1:], np.float32)
    for z in range(slabs.shape[0]):
        acc = (acc + slabs[z]).astype(np.float32)
    return acc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# layouts: which rows go where. rows[r] = (slot, position) or None (a padding row of a table).
# ---------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, name, nh, cap, window, slots, *, rps=None, pos=None, p0=0, slot0=0, m=None, tab=None,
                 compact=False, pre=None, S=0):
        self.name, self.nh, self.cap, self.window, self.slots, self.S = name, nh, cap, window, slots, S
        self.rps, self.pos, self.p0, self.slot0, self.compact = rps, pos, p0, slot0, compact
        self.F = list(pre) if pre is not None else None
        if tab is not None:  # tab: [(slot, first position, rows)], each padded to whole 16-row groups
            padded = []
            for slot, first, n in tab:
                padded += [(slot, first + i) for i in range(n)]
                padded += [None] * (-n % 16)
            while padded and padded[-1] is None and not compact:
                padded.pop()  # a launch may end inside a group: no padding rows after the last token
            self.padded = padded
            self.rows = [r for r in padded if r is not None] if compact else padded
        else:
            self.padded = None
            self.rows = [(slot0 + r // rps, (pos[slot0 + r // rps] if pos is not None else p0) + r % rps)
                         for r in range(m)]
        self.m = len(self.rows)

    def pre_len(self, slot):
        return self.F[slot] if self.F is not None else 0

    def blocks(self):
        """Runs of rows of one slot at consecutive positions: [(first row, slot, first position, n)]."""
        out, r = [], 0
        while r < self.m:
            if self.rows[r] is None:
                r += 1
                continue
            slot, p = self.rows[r]
            n = 1
            while r + n < self.m and self.rows[r + n] == (slot, p + n):
                n += 1
            out.append((r, slot, p, n))
            r += n
        return out

    def call(self, eng, kind, qkv, kv0, pre):
        kw = dict(window=self.window, pre=pre)
        if self.padded is not None:
            enc = lambda rows: [-1 if r is None else r[0] << 16 | r[1] for r in rows]
            kw["tab"] = enc(self.rows)
            if self.compact:
                kw["ptab"] = enc(self.padded)
        else:
            kw.update(slot0=self.slot0, rps=self.rps, p0=self.p0, pos=self.pos)
        return eng.test_attention(kind, qkv, kv0, **kw)


# k_attn16 (16-key tiles over 8 waves; ntiles = ceil((kmax - kmin + 1) / 16)). Kind A.
A_LAYOUTS = [
    # qpos0 = 0 (query 0 sees one key; 1 tile, 7 waves idle) | 105 keys: 7 tiles, 15 rows; M % 16 = 15
    Layout("t1_t7", 2, 128, 0, 2, rps=16, pos=[0, 90], m=31, S=3),
    # cap not a power of two: k_attn16<false>; 126 keys: 8 tiles | 136: 9 tiles | one row; M % 16 = 1
    Layout("t8_t9_row1", 3, 160, 0, 3, rps=16, pos=[110, 120, 37], m=33),
    # two groups per slot: 250 keys (16 tiles) then 266 (17 tiles, the first group's appended keys
    # among them) | 15 rows from position 1
    Layout("t16_t17", 2, 288, 0, 2, rps=32, pos=[234, 1], m=47),
    # window 5: kmin = qpos0 - 4 | a ring (cap 64) wrapped 3 times with the wrap inside the pass
    Layout("w5", 2, 64, 5, 2, rps=16, pos=[0, 252], m=32),
    # window 16 on a ring of exactly window + 16 | one row at position 1000 (31 wraps)
    Layout("w16", 2, 32, 16, 2, rps=16, pos=[7, 1000], m=17),
    # window 17, cap not a power of two (no ring: positions stay below cap); kmin = 24, 0
    Layout("w17", 3, 96, 17, 2, rps=16, pos=[40, 13], m=31),
    # window 48 on a ring of 64 = window + 16, 62 wraps, the wrap inside the window | position 30
    Layout("w48", 2, 64, 48, 2, rps=16, pos=[3990, 30], m=32, S=16),
    # the product's Mimi ring: window 250 of 512, 17 tiles; 7 wraps with the wrap inside the window |
    # qpos0 = 249 = window - 1 (kmin = 0) | 15 rows from 0
    Layout("w250", 2, 512, 250, 3, rps=16, pos=[3684, 249, 0], m=47),
    # a multi-frame pass: 32 rows per slot, the second group's window holds the first group's rows;
    # the pass itself crosses the wrap (500 .. 531) | 5 wraps
    Layout("w250_pass", 2, 512, 250, 2, rps=32, pos=[500, 3000], m=64),
    # table form: slots out of order, -1 padding rows closing a group (1 row + 15, 15 rows + 1)
    Layout("tab", 2, 128, 0, 3, tab=[(2, 20, 16), (0, 5, 1), (1, 40, 15)], S=3),
    # compact table form (batched admission: qrow / orow) with shared prefixes of 1, 5 and 16 rows:
    # the groups' keys lie on both sides of the prefix boundary
    Layout("compact_pre", 2, 128, 0, 3, tab=[(0, 1, 17), (1, 5, 15), (2, 16, 16)], compact=True, pre=[1, 5, 16]),
    # prefixes of 17 and 33 rows and a slot without one (F = 0 under a prefix table)
    Layout("compact_pre2", 3, 96, 0, 3, tab=[(2, 0, 16), (0, 17, 16), (1, 33, 3)], compact=True, pre=[17, 33, 0]),
    # the single-utterance prefill: RowMap {slot, T, p0 = F} on slot 1, 20 rows (16 + 4) after 33 shared
    Layout("prefill_pre", 3, 96, 0, 2, rps=20, slot0=1, p0=33, m=20, pre=[5, 33], S=3),
]
# k_attn16<true, true> (kind B): 16 rows per slot on a power-of-two ring of >= window + 16; these
# run through kind A as well (equal stores and outputs)
B_LAYOUTS = [
    Layout("w5", 2, 32, 5, 2, rps=16, pos=[0, 30], m=32),
    Layout("w16", 2, 32, 16, 2, rps=16, pos=[7, 1000], m=17),
    Layout("w17", 3, 64, 17, 2, rps=16, pos=[40, 589], m=31),
    Layout("w48", 2, 64, 48, 2, rps=16, pos=[3990, 30], m=32),  # cap == window + 16 exactly
    Layout("w250", 2, 512, 250, 3, rps=16, pos=[3684, 249, 0], m=47),  # the product's 250 / 512
]


def c_layout(name, qps, S, pre=None, cap=512, nh=2):
    return Layout(name, nh, cap, 0, len(qps), rps=1, pos=list(qps), m=len(qps), S=S, pre=pre)


# k_attn_decode_qkv<4, 8> (kind C): 128 keys per round (4 waves x 8 loads x 4 keys), the new key
# from LDS; rows of different slots at different positions in one launch
C_QPS = [(0, 1, 3), (4, 5, 31), (32, 33, 127), (128, 129, 255), (256, 257, 511)]
C_LAYOUTS = [c_layout(f"qp{q[0]}_S{S}", q, S) for q in C_QPS for S in (1, 3, 16)]
# shared prefixes of 1, 5, 33, 130 rows with qp below, at and above them
C_LAYOUTS += [c_layout(f"pre{F}_S{S}", (F - 1, F, F + 1), S, pre=[F] * 3)
              for F, S in [(1, 1), (5, 3), (33, 16), (130, 3)]]
C_LAYOUTS += [c_layout("pre_mixed", (140, 2, 40), 3, pre=[130, 0, 33], nh=3)]

SIGMA = {"s0.3": 0.3, "s5": 5.0, "s40": 40.0}
SPOTS_AB = ["first", "last", "out", "in", "pre_last", "own_first"]
SPOTS_C = ["first", "last", "new", "future", "pre_last", "own_first"]


def spike_position(kind, lay, spot, slot, p, n):
    """The spike key's position in `slot`, whose rows sit at p .. p + n - 1 (None: no such spot)."""
    F, w = lay.pre_len(slot), lay.window
    c0 = min(8, n - 1)
    if spot == "first":  # the first key the slot's first query sees
        kp = max(0, p - w + 1) if w else 0
    elif spot == "last":  # kind C: the last cached key; A, B: the last row's own key
        kp = p - 1 if kind == C else p + n - 1
    elif spot == "new":  # kind C: the key this step appends (read from LDS)
        kp = p
    elif spot == "future":  # stale store content past the query: no effect
        kp = p + 1
    elif spot == "out":  # one position outside query c0's window (queries below c0 still see it); without a
        kp = p + c0 - w if w else p + n  # window: the stale row after the last key
    elif spot == "in":  # the oldest key inside query c0's window; without a window: row c0's own key
        kp = p + c0 - w + 1 if w else p + c0
    elif spot == "pre_last":
        kp = F - 1
    else:  # own_first: the slot's own first row after the prefix
        kp = F
    if w:  # a ring keeps the last cap positions: older ones are overwritten by the pass itself
        return kp if max(0, p + n - lay.cap) <= kp <= p + n - 1 else None
    return kp if 0 <= kp < lay.cap else None


def v_values(idx, nh):
    """Distinct large V rows: v[h][d] at store index / position idx, |v| <= 125 (251 is prime, so any
    251 consecutive keys differ in every dim)."""
    idx = np.asarray(idx)[..., None, None]
    h, d = np.arange(nh)[:, None], np.arange(64)[None, :]
    return ((7 * idx + 13 * h + 3 * d) % 251 - 125).astype(np.float64)


def build(kind, lay, family, seed):
    """Inputs of one case: the store and prefixes hold rotated keys of the family's scale, the rows'
    raw q / k are the inverse rotations of the wanted rotated vectors."""
    rng = np.random.default_rng(seed)
    nh, cap, m = lay.nh, lay.cap, lay.m
    s = np.sqrt(SIGMA.get(family, 0.3))  # logits q . k / 8 of N(0, s^2) elements: sigma = s^2
    Kst = rng.standard_normal((lay.slots, nh, cap, 64)) * s
    Vst = np.stack([np.moveaxis(v_values(np.arange(cap) + 29 * sl, nh), 0, 1) for sl in range(lay.slots)])
    Vst += 0.25 * rng.standard_normal(Kst.shape)
    pre = None
    if lay.F is not None:
        pre = [np.stack([rng.standard_normal((nh, F, 64)) * s,
                         np.moveaxis(v_values(np.arange(F) + 97 + 11 * sl, nh), 0, 1)
                         + 0.25 * rng.standard_normal((nh, F, 64))]) for sl, F in enumerate(lay.F)]
    live = [r for r in range(m) if lay.rows[r] is not None]
    rpos = np.array([lay.rows[r][1] if lay.rows[r] else 0 for r in range(m)])
    Qn = rng.standard_normal((m, nh, 64)) * (0.0 if family == "zero" else s)
    Kn = rng.standard_normal((m, nh, 64)) * s
    Vn = v_values(rpos % cap + 31, nh) + 0.25 * rng.standard_normal((m, nh, 64))
    spikes = {}  # slot -> position of its spike key
    if family.startswith("spike_"):
        amp = np.sqrt(8 * SPIKE)
        for r0, slot, p, n in lay.blocks():
            if slot in spikes:
                continue  # a slot's later blocks (table form: there are none) share its spike
            rows = [r for r in live if lay.rows[r][0] == slot]
            p, n = lay.rows[rows[0]][1], len(rows)
            w = rng.standard_normal((nh, 64))
            w /= np.linalg.norm(w, axis=-1, keepdims=True)
            Kst[slot] -= (Kst[slot] * w[:, None]).sum(-1, keepdims=True) * w[:, None]
            Kn[rows] -= (Kn[rows] * w).sum(-1, keepdims=True) * w
            if pre is not None and lay.F[slot]:
                pre[slot][0] -= (pre[slot][0] * w[:, None]).sum(-1, keepdims=True) * w[:, None]
            Qn[rows] += amp * w
            kp = spike_position(kind, lay, family[6:], slot, p, n)
            if kp is None:
                continue
            spikes[slot] = kp
            if p <= kp < p + n:  # one of the call's own rows (kind C: also below the prefix length)
                Kn[rows[kp - p]] += amp * w
            elif kp < lay.pre_len(slot):
                pre[slot][0][:, kp] += amp * w
            else:
                Kst[slot, :, kp % cap] += amp * w
    pos_b = rpos[:, None]
    raw = np.concatenate([rope64(Qn, pos_b, True), rope64(Kn, pos_b, True), Vn], axis=0)  # [3 m][nh][64]
    raw = raw.reshape(3, m, nh * 64).transpose(1, 0, 2).reshape(m, 3 * nh * 64).astype(np.float32)
    for r in range(m):
        if lay.rows[r] is None:
            raw[r] = 0.0
    if lay.S > 0:  # S partial slabs that sum (f32, slab order) to about the wanted rows
        slabs = (0.3 * np.abs(raw) * rng.standard_normal((lay.S,) + raw.shape)).astype(np.float32)
        slabs[-1] = 0.0
        slabs[-1] = raw - slab_sum(slabs)
        qkv, raw = slabs, slab_sum(slabs)
    else:
        qkv = raw
    kv0 = np.stack([Kst, Vst], axis=1).astype(np.float32)
    if pre is not None:
        pre = [p.astype(np.float32) for p in pre]
    q_raw, k_raw, v_raw = (raw[:, i * nh * 64:(i + 1) * nh * 64].reshape(m, nh, 64) for i in range(3))
    return dict(qkv=qkv, kv0=kv0, pre=pre, q=q_raw, k=k_raw, v=v_raw, pos=rpos, live=live, spikes=spikes)


# ---------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------
def check_rope_append(kind, lay, c, kv1, q_dev):
    """Layer 1: stored K and rotated Q against the float64 rotation, V and the rest of the store
    bit-equal. Returns the worst err / tol."""
    worst = 0.0
    touched = np.zeros(kv1.shape[:4], bool)
    for r in c["live"]:
        slot, pos = lay.rows[r]
        if kind == C and pos >= lay.cap:
            continue  # a finished row that filled its cache appends nothing
        i = pos % lay.cap
        assert not touched[slot, 0, 0, i], "layout appends two rows at one ring index"
        touched[slot, :, :, i] = True
        err = np.abs(kv1[slot, 0, :, i].astype(np.float64) - rope64(c["k"][r], pos))
        tol = rope_tol(c["k"][r], pos)
        assert (err <= tol).all(), (lay.name, "K", r, slot, pos, float(err.max()), float(tol.max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert np.array_equal(bits(kv1[slot, 1, :, i]), bits(c["v"][r])), (lay.name, "V", r, slot, pos)
    same = bits(kv1) == bits(c["kv0"])
    assert same[~touched].all(), (lay.name, "untouched store elements changed", np.argwhere(~same & ~touched[..., None])[:4])
    if q_dev is not None:
        q_dev = q_dev.reshape(-1, lay.nh, 64)
        for r in c["live"]:
            err = np.abs(q_dev[r].astype(np.float64) - rope64(c["q"][r], c["pos"][r]))
            tol = rope_tol(c["q"][r], c["pos"][r])
            assert (err <= tol).all(), (lay.name, "Q", r, float(err.max()), float(tol.max()))
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def ref_attention(kind, lay, c, kv1, q_dev):
    """Layer 2 reference: float64 attention of every live row over the store the device left (and the
    prefixes), with its bound. Returns (O [m][nh][64], tol [m][nh][64])."""
    nh, cap, w, m = lay.nh, lay.cap, lay.window, lay.m
    O, T = np.zeros((m, nh, 64)), np.zeros((m, nh, 64))
    kv = kv1.astype(np.float64)
    for r0, slot, p, n in lay.blocks():
        rows = np.arange(r0, r0 + n)
        qp = np.minimum(np.arange(p, p + n), cap - 1) if kind == C else np.arange(p, p + n)
        if q_dev is not None:
            Q, qt = q_dev.reshape(-1, nh, 64)[rows].astype(np.float64), 0.0
        else:
            Q, qt = rope64(c["q"][rows], qp[:, None]), rope_tol(c["q"][rows], qp[:, None])
        kmin, kmax = (max(0, p - w + 1) if w else 0), int(qp[-1])
        kps = np.arange(kmin, kmax + 1)
        K, V = kv[slot, 0][:, kps % cap], kv[slot, 1][:, kps % cap]  # [nh][keys][64]
        F = lay.pre_len(slot)
        if F:
            shared = kps < F
            if kind == C:
                shared &= kps != p  # the step's own key comes from its row, also below the prefix length
            pk = c["pre"][slot].astype(np.float64)
            K[:, shared], V[:, shared] = pk[0][:, kps[shared]], pk[1][:, kps[shared]]
        vis = (kps[None, :] <= qp[:, None]) & ((w == 0) | (qp[:, None] - kps[None, :] < w))  # [n][keys]
        s = np.einsum("rhd,hkd->hrk", Q, K) / 8.0
        E = U * np.einsum("rhd,hkd->hrk", np.abs(Q), np.abs(K))
        if q_dev is None:
            E += np.einsum("rhd,hkd->hrk", qt, np.abs(K)) / 8.0
        s = np.where(vis[None], s, -np.inf)
        smax = s.max(-1, keepdims=True)
        E = np.where(vis[None], E + 6 * U + 3 * U * np.abs(np.where(vis[None], s - smax, 0.0)), 0.0)
        pw = np.exp(s - smax)
        pw /= pw.sum(-1, keepdims=True)
        o = np.einsum("hrk,hkd->hrd", pw, V)
        spread = np.abs(V[:, None] - o[:, :, None])  # [nh][n][keys][64]
        t1 = np.einsum("hrk,hrkd->hrd", pw * (E + (pw * E).sum(-1, keepdims=True)), spread)
        t2 = np.sqrt(vis.sum(-1) + 8.0)[None, :, None] * U * (np.einsum("hrk,hkd->hrd", pw, np.abs(V)) + np.abs(o))
        t3 = kps.size * np.abs(V).max() * 2.0 ** -126  # weights below FLT_MIN are lost to f32
        O[rows], T[rows] = o.transpose(1, 0, 2), 4.0 * (t1 + t2 + t3).transpose(1, 0, 2)
        kp = c["spikes"].get(slot)
        if kp is not None:  # the family's own claim: a visible spike stands SPIKE - 16 over every other key
            j = kp - kmin
            for i in range(n):
                if 0 <= j < kps.size and vis[i, j]:
                    rest = np.delete(s[:, i], j, axis=-1)
                    assert rest.size == 0 or (s[:, i, j] - rest.max(-1) >= 60.0).all(), (lay.name, slot, kp)
                    assert (np.abs(o[:, i] - V[:, j]) <= 1e-9).all()  # it dominates: O is its V row
    return O, T


def run_case(eng, kind, lay, family, seed):
    """One launch, both layers. Returns (worst RoPE err / tol, worst O err / tol, worst |O err|, o, kv1)."""
    c = build(kind, lay, family, seed)
    o, kv1, q = lay.call(eng, kind, c["qkv"], c["kv0"], c["pre"])
    if q is not None and lay.compact:  # Q rows are the padded rows: take the tokens'
        q = q[[i for i, r in enumerate(lay.padded) if r is not None]]
    wr = check_rope_append(kind, lay, c, kv1, q)
    ref, tol = ref_attention(kind, lay, c, kv1, q)
    o3 = o.reshape(lay.m, lay.nh, 64).astype(np.float64)
    live = [r for r in c["live"] if not (kind == C and lay.rows[r][1] >= lay.cap)]
    err = np.abs(o3 - ref)[live]
    assert np.isfinite(o3[live]).all(), (lay.name, family)
    bad = err > tol[live]
    assert not bad.any(), (lay.name, family, "row/head/dim", np.argwhere(bad)[:4].tolist(), float(err[bad].max()),
                           float(tol[live][bad].min()))
    dead = [r for r in range(lay.m) if lay.rows[r] is None]
    assert not o3[dead].any(), (lay.name, "a padding row's output was written")
    return wr, float((err / np.maximum(tol[live], 1e-300)).max()), float(err.max()), o, kv1


def sweep(eng, kind, layouts, family):
    wr = wo = wa = 0.0
    for i, lay in enumerate(layouts):
        r, o, a, _, _ = run_case(eng, kind, lay, family, 1000 * kind + 17 * i + sum(map(ord, family)))
        wr, wo, wa = max(wr, r), max(wo, o), max(wa, a)
    print(f"kind {'ABC'[kind]} {family}: worst RoPE err/gate {wr:.3g}, worst O err/gate {wo:.3g}, worst |dO| {wa:.3g}")


@pytest.mark.parametrize("family", list(SIGMA) + ["zero"] + ["spike_" + s for s in SPOTS_AB])
def test_prefill_attention_matches_fp64(eng, family):
    """Kind A on every k_attn16 shape edge: 1, 7, 8, 9, 16, 17 key tiles, kmin off the tile grid,
    qpos0 = 0, groups of 1, 15, 16 rows (uniform and table form), windows 5 / 16 / 17 / 48 / 250,
    rings wrapped up to 62 times with the wrap inside the window, prefixes of 1 / 5 / 16 / 17 / 33
    rows, dense rows and 3 / 16 slabs."""
    sweep(eng, A, A_LAYOUTS + B_LAYOUTS, family)


@pytest.mark.parametrize("family", list(SIGMA) + ["zero"] + ["spike_" + s for s in SPOTS_AB])
def test_mimi_step_attention_matches_fp64(eng, family):
    """Kind B (RoPE and ring append fused): windows 5 .. 250, cap == window + 16 exactly (16 / 32,
    48 / 64) and the product's 250 / 512, wraps inside the window and inside the appended rows."""
    sweep(eng, B, B_LAYOUTS, family)


@pytest.mark.parametrize("family", list(SIGMA) + ["zero"] + ["spike_" + s for s in SPOTS_C])
def test_flow_step_attention_matches_fp64(eng, family):
    """Kind C: qp 0, 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, cap - 1, each with 1, 3
    and 16 slabs; prefixes of 1 / 5 / 33 / 130 rows with qp below, at and above them; three slots
    at different positions per launch."""
    sweep(eng, C, C_LAYOUTS, family)


def test_fused_and_unfused_mimi_paths_agree_bitwise(eng):
    """attention16_qkv (B) and qkv_rope_append + attention (A) run the same expressions on the same
    template, tile order included: equal stores and equal outputs on the same input."""
    for i, lay in enumerate(B_LAYOUTS):
        for family in ("s5", "spike_in"):
            c = build(B, lay, family, 40 + i)
            oa, kva, _ = lay.call(eng, A, c["qkv"], c["kv0"], None)
            ob, kvb, _ = lay.call(eng, B, c["qkv"], c["kv0"], None)
            assert np.array_equal(bits(kva), bits(kvb)), (lay.name, family, "stores differ")
            assert np.array_equal(bits(oa), bits(ob)), (lay.name, family, float(np.abs(oa - ob).max()))


def test_step_table_rope_equals_inline_rope_bitwise(eng):
    """K appended by the step kernel (cos / sin from rope_table) equals K appended by k_qkv_rope
    (inline expf / cosf / sinf) for the same row and position, V too; positions 0, 1 and cap - 1,
    1 and 16 slabs. The table's cos / sin always were the inline values; the rotation was not: the
    compiler fused x0 sn + x1 cs around the other product in the step kernel, and 15 to 26 of a
    row's 64 odd dims came out 1 ulp apart (up to 9 where the sum cancels). The step kernel now
    spells the fused form k_qkv_rope compiles to."""
    for S, qps in [(1, (0, 1, 511)), (16, (257, 5, 130))]:
        lc = c_layout("c", qps, S)
        # the same rows through kind A: each alone in a 16-row group of a table
        la = Layout("a", 2, 512, 0, 3, tab=[(s, qp, 1) for s, qp in enumerate(qps)], S=S)
        c = build(C, lc, "s5", 7 + S)
        _, kvc, _ = lc.call(eng, C, c["qkv"], c["kv0"], None)
        qkv_a = np.zeros((S, la.m, c["qkv"].shape[-1]), np.float32)
        qkv_a[:, [16 * s for s in range(3)]] = c["qkv"]
        _, kva, _ = la.call(eng, A, qkv_a, c["kv0"], None)
        assert check_rope_append(C, lc, c, kvc, None) <= 1.0
        assert np.array_equal(bits(kva), bits(kvc)), (S, qps)


def test_rope_append_positions(eng):
    """RoPE and append alone at positions 0, 1, cap - 1 and ring positions up to 4,000 (125 wraps of
    a 32-row ring), kinds A and B; the gate of the module docstring, V and the untouched store
    bit-equal."""
    for kind, lay in [(A, Layout("p_a", 3, 32, 16, 3, rps=16, pos=[0, 3984, 16], m=48)),  # 3984 + 15 = 3999
                      (B, Layout("p_b", 3, 32, 16, 3, rps=16, pos=[0, 3984, 16], m=48)),  # 16 + 15 = cap - 1
                      (A, Layout("p_a1", 2, 160, 0, 2, rps=16, pos=[1, 144], m=32))]:  # 144 + 15 = cap - 1
        c = build(kind, lay, "s5", 3)
        _, kv1, q = lay.call(eng, kind, c["qkv"], c["kv0"], None)
        print(f"{lay.name}: worst RoPE err/gate {check_rope_append(kind, lay, c, kv1, q):.3g}")


def test_finished_row_at_cap_appends_nothing(eng):
    """Kind C, qp == cap: a finished row that filled its cache is still stepped; its key must not
    land on position cap, which is the next head's (for the last head: the next slot's) position 0.
    The whole store is bit-equal for that slot; its neighbours append as usual."""
    lay = c_layout("full", (64, 64, 10), 3, cap=64, nh=3)
    c = build(C, lay, "s5", 11)
    o, kv1, _ = lay.call(eng, C, c["qkv"], c["kv0"], None)
    assert np.array_equal(bits(kv1[:2]), bits(c["kv0"][:2]))
    check_rope_append(C, lay, c, kv1, None)  # slot 2's append, everything else untouched
    assert np.isfinite(o).all()


def test_ring_too_small_for_the_fused_append_is_refused(eng):
    """attention16_qkv keeps its host checks: cap < window + 16 (and a cap that is no power of two)
    raises instead of evicting keys inside the window."""
    import pocket_tts_amd as pt

    for cap, window in [(64, 49), (32, 17), (96, 48)]:
        lay = Layout("small", 2, cap, window, 1, rps=16, pos=[0], m=16)
        c = build(B, lay, "s0.3", 1)
        with pytest.raises(pt.PocketTTSError, match="ring too small"):
            lay.call(eng, B, c["qkv"], c["kv0"], None)
    lay = Layout("rps", 2, 64, 16, 1, rps=32, pos=[0], m=32)
    c = build(B, lay, "s0.3", 1)
    with pytest.raises(pt.PocketTTSError, match="16 rows per slot"):
        lay.call(eng, B, c["qkv"], c["kv0"], None)
