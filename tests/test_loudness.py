"""The host loudness rule (audio.kweight_coeffs / loudness_blocks /
loudness_integrated): ITU-R BS.1770 K-weighting at 24 kHz, 100 ms sub-blocks, 400 ms gating blocks,
absolute and relative gates. No GPU: the library is used for nothing here."""

import numpy as np
import pytest

from pocket_tts_amd.audio import (LoudnessMeter, kweight_coeffs, loudness_blocks, loudness_gain_cdb,
                                  loudness_integrated, loudness_tables)

FS = 24000


def sine(freq, amp, seconds):
    n = int(round(seconds * FS))
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / FS)).astype(np.float32)


def lufs(x):
    return loudness_integrated(loudness_blocks(x))


def test_coefficients_at_48k_are_the_standards_table():
    c = kweight_coeffs(48000.0)
    want = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                     [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])
    assert c.shape == (2, 5) and np.abs(c - want).max() <= 1e-12, np.abs(c - want).max()
    pq = loudness_tables(kweight_coeffs())
    a1, a2 = kweight_coeffs()[0][3:]
    assert pq.shape == (2, 2, 32) and pq[0, 0, 0] == -a1 and pq[0, 1, 0] == -a2


def test_calibration_sine_and_the_weighting_curve():
    ref = lufs(sine(997.0, 1.0, 5.0))
    print("997 Hz full scale:", ref)
    assert abs(ref - (-3.01)) <= 0.05, ref  # BS.1770's own calibration statement
    low = lufs(sine(20.0, 1.0, 5.0))
    print("20 Hz:", low)
    assert low <= ref - 10.0
    assert lufs(sine(100.0, 1.0, 5.0)) < ref < lufs(sine(4000.0, 1.0, 5.0))


def test_six_db_reads_six_lu():
    x = sine(997.0, 0.25, 5.0)
    v = np.float32(10.0 ** (6.0 / 20.0))
    d = lufs(v * x) - lufs(x)
    print("+6.00 dB reads", d)
    assert abs(d - 6.0) <= 0.01, d


def test_gating():
    loud, quiet = sine(997.0, 0.1, 2.0), sine(997.0, 1e-4, 2.0)
    both, alone = lufs(np.concatenate([loud, quiet])), lufs(loud)
    e = loudness_blocks(np.concatenate([loud, quiet]))
    B = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / 9600.0
    ungated = -0.691 + 10 * np.log10(B.mean())
    print("gated", both, "loud part alone", alone, "ungated", ungated)
    assert alone - 0.5 <= both <= alone
    assert both > ungated + 2.0
    assert lufs(np.zeros(2 * FS, np.float32)) is None
    assert lufs(sine(997.0, 0.5, 0.399)) is None and lufs(sine(997.0, 0.5, 0.4)) is not None
    # a response of several rows: the gating blocks are pooled and gated once
    assert loudness_integrated([loudness_blocks(loud), loudness_blocks(quiet)]) == pytest.approx(alone, abs=1e-9)
    assert loudness_integrated([np.zeros(3), np.zeros(0)]) is None


def test_streaming_equals_whole():
    x = (0.1 * np.random.default_rng(0).standard_normal(12000)).astype(np.float32)
    sizes = [1794, 1, 2046, 5728, 0, 2399, 32]
    assert sum(sizes) == x.size
    whole = loudness_blocks(x)
    chunks = loudness_blocks(x, chunks=sizes)
    assert whole.size == 5 and [c.size for c in chunks] == [0, 0, 1, 2, 0, 1, 1]
    assert np.array_equal(np.concatenate(chunks).view(np.uint64), whole.view(np.uint64))
    assert loudness_blocks(x[:2399]).size == 0 and loudness_blocks(x[:2400]).size == 1
    assert loudness_blocks(x[:2400])[0].view(np.uint64) == whole[0].view(np.uint64)
    m = LoudnessMeter()  # one sample at a time across a sub-block boundary
    got = [m.feed(x[i:i + 1]) for i in range(2395, 2405)]
    assert all(g.size == 0 for g in got)
    with pytest.raises(ValueError):
        loudness_blocks(x, chunks=[1, 2])


def test_segment_rule_against_the_plain_cascade():
    x = (0.1 * np.random.default_rng(1).standard_normal(12000)).astype(np.float32)
    c = kweight_coeffs()
    y = x.astype(np.float64)
    for bq in range(2):  # direct form I, sample by sample
        b0, b1, b2, a1, a2 = (float(v) for v in c[bq])
        out = np.zeros_like(y)
        x1 = x2 = y1 = y2 = 0.0
        for n, v in enumerate(y):
            r = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, float(v), y1, r
            out[n] = r
        y = out
    plain = (y * y).reshape(-1, 2400).sum(axis=1)
    rel = np.abs(loudness_blocks(x) / plain - 1.0).max()
    print("segment rule against the plain cascade:", rel)
    assert rel <= 1e-10


def test_gain_rule():
    assert loudness_gain_cdb(-16.0, -23.456) == 746 and loudness_gain_cdb(-16.0, -20.004) == 400
    assert loudness_gain_cdb(-5.0, -60.0) == 2400 and loudness_gain_cdb(-40.0, -3.0) == -2400
