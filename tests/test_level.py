"""The level rule on the host: the plan (ptts_level_plan, the library's host
function, through ctypes), the struct layout, the numpy restatement audio.level_limit with the
properties the rule promises, and its streaming form against the whole-signal form. No GPU: the
library is only loaded for its host functions."""

import ctypes as C
import math

import numpy as np
import pytest

from pocket_tts_amd._lib import SlotOpts3, SlotOpts4, lib
from pocket_tts_amd.audio import LEVEL_L, LEVEL_TAPS, level_cdb, level_chunk_samples, level_limit, level_plan

GAINS = [-2400, -601, 0, 1, 2400]
CEILINGS = [-4000, -100, 0]
SIZES = [1, 126, 127, 253, 5000]


def c_plan(gain_cdb, ceiling_cdb):
    v, c = C.c_float(0), C.c_float(0)
    rc = lib().ptts_level_plan(gain_cdb, ceiling_cdb, C.byref(v), C.byref(c))
    return rc, np.float32(v.value), np.float32(c.value)


def test_plan():
    for g in GAINS:
        for ce in CEILINGS:
            rc, v, c = c_plan(g, ce)
            assert rc == 0
            assert v == np.float32(10 ** (g / 2000)) and c == np.float32(10 ** (ce / 2000)), (g, ce)
            assert level_plan(g, ce) == (v, c)
    assert c_plan(0, 0)[1:] == (np.float32(1.0), np.float32(1.0))
    for g, ce in ((2401, -100), (-2401, -100), (0, 1), (0, -4001), (1 << 20, 0)):
        assert c_plan(g, ce)[0] == 1, (g, ce)
        with pytest.raises(ValueError):
            level_plan(g, ce)
    assert lib().ptts_level_plan(600, -100, None, None) == 0  # either pointer may be null
    v = C.c_float(0)
    assert lib().ptts_level_plan(600, -100, C.byref(v), None) == 0 and np.float32(v.value) == np.float32(10 ** 0.3)
    assert lib().ptts_level_plan(600, -100, None, C.byref(v)) == 0 and np.float32(v.value) == np.float32(10 ** -0.05)


def test_slot_opts_layout():
    assert C.sizeof(SlotOpts3) == 48 and C.sizeof(SlotOpts4) == 56
    assert SlotOpts4.pitch_cents.offset == 40 and SlotOpts4.reserved.offset == 44
    assert SlotOpts4.gain_cdb.offset == 48 and SlotOpts4.limit.offset == 52


def test_taps():
    assert LEVEL_TAPS.size == LEVEL_L + 1 == 127 and LEVEL_TAPS.sum() == 4096
    box = np.convolve(np.ones(64), np.ones(64))
    assert np.array_equal(LEVEL_TAPS, box)


def test_cdb():
    assert level_cdb(None) == 0 and level_cdb(0) == 0 and level_cdb(6) == 600 and level_cdb(-24) == -2400
    assert level_cdb(1.004) == 100 and level_cdb(-0.006) == -1
    for bad in (24.01, -24.01, math.inf, math.nan):
        with pytest.raises(ValueError):
            level_cdb(bad)


def test_identity():
    """peaks under the ceiling: g == 1 and y == f32(v x) exactly"""
    rng = np.random.default_rng(0)
    for n in SIZES:
        for g, ce in ((0, -100), (600, -100), (-601, -4000), (2400, 0)):
            v, c = level_plan(g, ce)
            x = rng.uniform(-1, 1, n).astype(np.float32) * np.float32(0.999 * float(c) / float(v))
            y, u, r, gg = level_limit(x, g, ce, detail=True)
            assert np.abs(u).max() <= c
            assert (gg == 1).all() and (r == 1).all()
            assert np.array_equal(y.view(np.uint32), (v * x).astype(np.float32).view(np.uint32)), (n, g, ce)


def adversarial(n, kind, rng):
    x = np.zeros(n, np.float32)
    if kind == "spikes":
        x += (0.01 * rng.standard_normal(n)).astype(np.float32)
        for i in (0, 1, n - 1):
            x[min(max(i, 0), n - 1)] = 1.0 if i != 1 else -1.0
    elif kind == "plateau":
        x += (0.05 * rng.standard_normal(n)).astype(np.float32)
        a = max(0, n // 2 - 150)
        x[a:a + 300] = 1.0
    elif kind == "alternating":
        x[:] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    elif kind == "noise":
        x[:] = (0.3 * rng.standard_normal(n)).astype(np.float32)
    return x


@pytest.mark.parametrize("kind", ["spikes", "plateau", "alternating", "noise"])
def test_peak_slope_window_clamp(kind):
    rng = np.random.default_rng(7)
    engaged = 0
    for n in SIZES:
        for g, ce in ((2400, -100), (0, -100), (600, -2600), (2400, 0)):
            x = adversarial(n, kind, rng)
            y, u, r, gg = level_limit(x, g, ce, detail=True)
            v, c = level_plan(g, ce)
            assert y.size == n and y.dtype == np.float32
            # peak: the output never leaves the ceiling, the gain never exceeds the instantaneous ratio
            assert np.abs(y).max() <= c, (kind, n, g, ce)
            assert (gg <= r).all(), (kind, n, g, ce)
            assert (gg > 0).all() and (gg <= 1).all()
            # slope: at most 1/64 per sample (one f32 rounding on top)
            if n > 1:
                assert np.abs(np.diff(gg.astype(np.float64))).max() <= 1 / 64 + 2.0 ** -23, (kind, n, g, ce)
            # window: g == 1 wherever no |u| > C lies within +-L
            over = np.flatnonzero(np.abs(u) > c)
            near = np.zeros(n, bool)
            for i in over:
                near[max(i - LEVEL_L, 0):i + LEVEL_L + 1] = True
            assert (gg[~near] == 1).all(), (kind, n, g, ce)
            assert np.array_equal(y[~near].view(np.uint32), u[~near].view(np.uint32))
            engaged += int(over.size > 0)
            # clamp: it moves a sample only by the rounding of g u
            before = np.abs(gg.astype(np.float64) * u.astype(np.float64))
            assert before.max() <= float(c) * (1 + 2.0 ** -22), (kind, n, g, ce, before.max())
            moved = np.flatnonzero((gg * u) != y)
            print(f"{kind} n {n} gain {g} ceiling {ce}: {over.size} over, clamp moved {moved.size}")
    assert engaged >= len(SIZES)  # the limiter did engage


@pytest.mark.parametrize("gain,ceiling", [(2400, -100), (600, -2600), (0, -100), (-601, -4000)])
def test_streaming_equals_the_whole_signal(gain, ceiling):
    rng = np.random.default_rng(gain & 0xFFFF)
    n = 2 * 1920 + 77
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x[0], x[-1], x[1000:1300] = 1.0, -1.0, 0.9
    whole = level_limit(x, gain, ceiling)
    assert whole.size == n
    ragged = [int(v) for v in rng.integers(0, 400, size=9)]
    for sizes in ([n], [1], [0, 1, 125, 0, 1920, 0], [1] * 260, [125, 0, 1, 126, 127], ragged, [1920, 1920], [0, 0]):
        sizes = sizes + [n - sum(sizes)] if sum(sizes) < n else sizes
        chunks = level_limit(x, gain, ceiling, chunks=sizes)
        assert len(chunks) == len(sizes)
        seen, want = 0, []
        for f, s in enumerate(sizes):
            want.append(level_chunk_samples(seen, seen + s, f == len(sizes) - 1))
            seen += s
        assert [len(c) for c in chunks] == want, sizes
        cat = np.concatenate(chunks)
        assert cat.size == n and np.array_equal(cat.view(np.uint32), whole.view(np.uint32)), sizes
    # chunk sizes of a plain row: 1920 - 126, 1920, 1920 + 126; a one-frame row emits everything at once
    assert [level_chunk_samples(1920 * f, 1920 * (f + 1), f == 2) for f in range(3)] == [1794, 1920, 2046]
    assert level_chunk_samples(0, 1920, True) == 1920 and level_chunk_samples(0, 100, False) == 0
    short = x[:100]  # a whole signal shorter than the look-ahead
    assert np.array_equal(level_limit(short, gain, ceiling, chunks=[100])[0], level_limit(short, gain, ceiling))
    with pytest.raises(ValueError):
        level_limit(x, gain, ceiling, chunks=[5])


def test_generation_params_level():
    from pocket_tts_amd import GenerationParams

    p = GenerationParams()
    assert p.level() == (0, 0) and p.opts() == (0, 0, 0) and p.cents() == 0
    p.volume_db = 0.0
    assert p.level() == (0, 0)
    p.volume_db = -6.5
    assert p.level() == (-650, 0) and p.opts() == (0, 0, 0)
    p.volume_db, p.limit = None, True
    assert p.level() == (0, 1)
