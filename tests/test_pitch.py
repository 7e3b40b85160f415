"""The pitch rule on the host: the plan (ptts_pitch_plan, the library's host
function, through ctypes), the numpy restatement audio.pitch_resample and its streaming form, and
the two tone conditions that the constants Z, P and beta are chosen by. No GPU: the library is only
loaded for its host functions."""

import ctypes as C
import math

import numpy as np
import pytest

from pocket_tts_amd._lib import fptr, lib
from pocket_tts_amd.audio import (PITCH_ONE, PITCH_P, PITCH_Z, pitch_chunk_samples, pitch_cq, pitch_emitted, pitch_len,
                                  pitch_plan, pitch_resample, pitch_support, pitch_table, tempo_len, tempo_wsola)

HALF_STEP = 1.0 / 65534.0  # half a step of the 16-bit wire (1 / 32767)
TONE_CENTS = [-1200, -700, -100, 100, 700, 1200]


def c_plan(cents, sp):
    w, st = C.c_int(0), C.c_uint32(0)
    rc = lib().ptts_pitch_plan(cents, sp, C.byref(w), C.byref(st))
    return rc, w.value, st.value


def test_plan():
    assert pitch_plan(0) == (1000, 1 << 20)
    assert pitch_plan(1200) == (500, 1 << 21)
    assert pitch_plan(-1200) == (2000, 1 << 19)
    for cents in range(-1200, 1201):
        sp_w, step = pitch_plan(cents, 1000)
        assert step == round(2 ** (cents / 1200) * 2 ** 20), cents
        assert sp_w == (1000 * 2 ** 20 + step // 2) // step, cents
    # sp_w follows from (step, speed) by the integer rule; outside [500, 2000]: invalid, both ways
    n_bad = 0
    for cents in (-1200, -701, -1, 1, 350, 1200):
        step = pitch_plan(cents, 1000)[1]
        for sp in (0, 500, 501, 707, 999, 1000, 1414, 1999, 2000):
            want = ((sp or 1000) * 2 ** 20 + step // 2) // step
            rc, w, st = c_plan(cents, sp)
            if 500 <= want <= 2000:
                assert (rc, w, st) == (0, want, step), (cents, sp)
                assert pitch_plan(cents, sp) == (want, step)
            else:
                n_bad += 1
                assert rc == 1, (cents, sp)
                with pytest.raises(ValueError):
                    pitch_plan(cents, sp)
    assert n_bad >= 8
    for cents, sp in ((1201, 1000), (-1201, 1000), (0, 499), (0, 2001), (100, -5)):
        assert c_plan(cents, sp)[0] == 1, (cents, sp)
    assert lib().ptts_pitch_plan(700, 1000, None, None) == 0  # either pointer may be null
    assert lib().ptts_pitch_len(1920, 1 << 20) == 1920 and lib().ptts_pitch_len(1921, 1 << 21) == 960
    assert lib().ptts_pitch_len(5, 1 << 18) == 0 and lib().ptts_pitch_len(-1, 1 << 20) == 0
    for n, step in ((0, 1 << 20), (1, 1 << 21), (7777, 699841), (1 << 30, 1571089)):
        assert lib().ptts_pitch_len(n, step) == pitch_len(n, step) == (n << 20) // step


def test_table():
    t, d = pitch_table()
    zp = PITCH_Z * PITCH_P
    assert t.size == zp + 2 and d.size == zp + 1 and t.dtype == d.dtype == np.float32
    assert t[0] == 1.0 and not t[PITCH_P:zp + 2:PITCH_P].any() and t[zp] == 0.0 and t[zp + 1] == 0.0
    assert np.array_equal(d, (t[1:].astype(np.float64) - t[:-1].astype(np.float64)).astype(np.float32))
    ct, cd = np.zeros(zp + 1, np.float32), np.zeros(zp + 1, np.float32)  # the table the engine uploads
    assert lib().ptts_pitch_table(fptr(ct), fptr(cd), zp + 1) == 0
    assert np.array_equal(ct.view(np.uint32), t[:zp + 1].view(np.uint32))
    assert np.array_equal(cd.view(np.uint32), d.view(np.uint32))
    assert lib().ptts_pitch_table(fptr(ct), fptr(cd), zp) == 1


def test_identity():
    rng = np.random.default_rng(0)
    for n in (1, 33, 1920, 5000):
        x = rng.standard_normal(n).astype(np.float32)
        y = pitch_resample(x, PITCH_ONE)
        assert y.size == n and np.array_equal(y.view(np.uint32), x.view(np.uint32))


def tone(freq_hz, n=24000):
    return (0.9 * np.sin(2 * np.pi * freq_hz * np.arange(n) / 24000.0)).astype(np.float32)


@pytest.mark.parametrize("cents", TONE_CENTS)
def test_passband(cents):
    """a 0.9 sine at 0.02, 0.3, 0.6 and 0.75 of c 12 kHz stays within half a 16-bit step of the
    analytic sine at m step / 2^20 (the inputs are the f64 sine rounded to f32: 2^-25 at most)"""
    step = pitch_plan(cents, 1000)[1]
    c = pitch_cq(step) / 2 ** 20
    for frac in (0.02, 0.3, 0.6, 0.75):
        f = frac * c * 12000.0
        y = pitch_resample(tone(f), step)
        m = np.arange(y.size)
        ref = 0.9 * np.sin(2 * np.pi * f * (m * step / 2 ** 20) / 24000.0)
        err = np.abs(y - ref)[400:-400].max()
        print(f"passband {cents} cents, {frac} of the cutoff ({f:.0f} Hz): {err:.3g}")
        assert err <= HALF_STEP, (cents, frac, err)


@pytest.mark.parametrize("cents", [c for c in TONE_CENTS if c > 0])
def test_stopband(cents):
    """a 0.9 sine at 1.25 c 12 kHz (where that is below 12 kHz) comes out below half a 16-bit step"""
    step = pitch_plan(cents, 1000)[1]
    f = 1.25 * (pitch_cq(step) / 2 ** 20) * 12000.0
    if f >= 12000.0:
        return  # (+100 cents: 14.2 kHz is no input tone)
    y = pitch_resample(tone(f), step)
    peak = np.abs(y)[400:-400].max()
    print(f"stopband {cents} cents ({f:.0f} Hz): {peak:.3g}")
    assert peak < HALF_STEP, (cents, peak)


@pytest.mark.parametrize("cents", [-1200, -350, 1, 700, 1200])
def test_streaming_equals_the_whole_signal(cents):
    step = pitch_plan(cents, 1000)[1]
    H = pitch_support(step)
    rng = np.random.default_rng(cents & 0xFFFF)
    x = (0.3 * rng.standard_normal(2 * 1920 + 77)).astype(np.float32)
    whole = pitch_resample(x, step)
    assert whole.size == pitch_len(x.size, step)
    ragged = [int(v) for v in rng.integers(0, 400, size=9)]
    for sizes in ([x.size], [0, 1, H, 1920, 0], [1] * (2 * H + 3), [H, 0, H, 1], ragged, [1920, 1920]):
        sizes = sizes + [x.size - sum(sizes)] if sum(sizes) < x.size else sizes
        chunks = pitch_resample(x, step, sizes)
        assert len(chunks) == len(sizes)
        n, want = 0, []
        for f, c in enumerate(sizes):
            want.append(pitch_chunk_samples(n, n + c, step, f == len(sizes) - 1))
            n += c
        assert [len(c) for c in chunks] == want, sizes
        cat = np.concatenate(chunks)
        assert cat.size == whole.size and np.array_equal(cat.view(np.uint32), whole.view(np.uint32)), sizes
    # the streaming rule: after n inputs (not the last frame) every m with (m step >> 20) + H <= n - 1
    for n in (0, 1, H, H + 1, 2 * H + 1, 1920, 5528):
        e = pitch_emitted(n, step)
        assert e == sum(1 for m in range(e + 3) if ((m * step) >> 20) + H <= n - 1)
        assert e <= pitch_len(n, step)
    # one signal of one chunk that is shorter than the support
    short = x[:H]
    assert np.array_equal(pitch_resample(short, step, [H])[0], pitch_resample(short, step))


@pytest.mark.parametrize("cents", [400, -700])
def test_composition_shifts_the_pitch_and_keeps_the_duration(cents):
    """A stationary 200 Hz sine through tempo_wsola(., sp_w) and pitch_resample: the FFT peak lies
    within one bin of 200 step / 2^20 Hz and the length is pitch_len(tempo_len(N, sp_w), step), which
    is N 1000 / sp up to the rounding of sp_w (at most 0.1 %) and the two integer roundings."""
    N = 24000
    x = (0.5 * np.sin(2 * np.pi * 200.0 * np.arange(N) / 24000.0)).astype(np.float32)
    for sp in (1000, 800):
        sp_w, step = pitch_plan(cents, sp)
        y = pitch_resample(tempo_wsola(x, sp_w), step)
        L = lib().ptts_pitch_len(lib().ptts_tempo_len(N, sp_w), step)
        assert y.size == L == pitch_len(tempo_len(N, sp_w), step)
        ideal = N * 1000.0 / sp
        print(f"{cents} cents at speed {sp}: sp_w {sp_w}, {L} samples against {ideal:.1f} ({(L / ideal - 1) * 100:+.4f} %)")
        assert abs(L / ideal - 1.0) <= 1e-3
        spec = np.abs(np.fft.rfft(y * np.hanning(y.size)))
        peak_hz = np.argmax(spec) * 24000.0 / y.size
        assert abs(peak_hz - 200.0 * step / 2 ** 20) <= 24000.0 / y.size, (peak_hz, 200.0 * step / 2 ** 20)


def test_generation_params_cents():
    from pocket_tts_amd import GenerationParams
    from pocket_tts_amd.audio import pitch_cents

    p = GenerationParams()
    assert p.cents() == 0 and p.opts() == (0, 0, 0)
    p.pitch = 0.0
    assert p.cents() == 0
    p.pitch = -3.5
    assert p.cents() == -350 and p.opts() == (0, 0, 0)
    assert pitch_cents(None) == 0 and pitch_cents(12) == 1200 and pitch_cents(-0.01) == -1
    for bad in (12.01, -12.01, math.inf, math.nan):
        with pytest.raises(ValueError):
            pitch_cents(bad)
