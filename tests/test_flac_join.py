"""Joining FLAC segments, CPU side, no engine: ptts_flac_rebase and
ptts_flac_silence against the host restatement audio.flac_frames byte for byte, the inputs rebase
must refuse (with `out` untouched), and audio.FlacJoiner against the decoder of tests/flac_decode.py.

The acceptance rule: rebase(flac_frames(s, f, rate), index, d) == flac_frames(s, f + d, rate)."""

import ctypes as C

import numpy as np
import pytest

import flac_decode as fd
from pocket_tts_amd import _lib
from pocket_tts_amd.audio import (FLAC_BLOCK, FlacJoiner, flac_frames, flac_frames_index, flac_rebase, flac_silence,
                                  flac_stream_header)

SIZES = (1, 15, 16, 17, 256, 257, 4608, 11477)  # the block sizes, and one chunk of three frames
SIGNALS = ("noise", "constant", "alternating")
END = 1 << 36
# (f, delta): the number keeps its width ...
SAME = [(0, 0), (3, 100), (1000, 500), (1 << 20, (1 << 20) - 7), ((1 << 31) + 9, 1 << 33)]
# ... or crosses a width boundary upward: each one by one step, a frame that ends on it, and all at once
CROSS = [((1 << k) - 1, 1) for k in (7, 11, 16, 21, 26, 31)] + [((1 << k) - 3, 5) for k in (7, 11, 16, 21, 26, 31)] + \
        [(5, (1 << 31) + 12345)]


def signal(name, n):
    if name == "constant":
        return np.full(n, -1234, np.int16)
    if name == "alternating":
        return np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
    return np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)


def frames_at(s, first, rate, memo={}):
    """flac_frames_index(s, first, rate). The subframes do not depend on `first`, so the search runs once per
    signal: the frames at another `first` are those at 0 with the header and the CRC-16 redone by
    audio's own functions (test_memo_is_flac_frames pins that against flac_frames itself)."""
    from pocket_tts_amd.audio import flac_crc8, flac_crc16, flac_number
    key = (s.tobytes(), rate)
    if key not in memo:
        memo[key] = flac_frames_index(s, 0, rate)
    data, index = memo[key]
    if first == 0:
        return data, index
    out, at = [], 0
    for i, (size, bs) in enumerate(index):
        f = data[at:at + size]
        old = len(flac_number(i * FLAC_BLOCK))
        head = f[:4] + flac_number(first + i * FLAC_BLOCK) + f[4 + old:4 + old + (1 if bs <= 256 else 2)]
        head += bytes([flac_crc8(head)])
        body = f[4 + old + (1 if bs <= 256 else 2) + 1:-2]
        out.append(head + body + flac_crc16(head + body).to_bytes(2, "big"))
        at += size
    return b"".join(out), [(len(f), bs) for f, (_, bs) in zip(out, index)]


def raw_rebase(data, index, delta, cap=None, fill=0xAA):
    """ptts_flac_rebase itself: (status, out buffer, bytes written)"""
    idx = np.ascontiguousarray(np.asarray(index, np.int32).reshape(-1, 2))
    src = np.frombuffer(bytes(data), np.uint8).copy()
    cap = len(data) + 6 * idx.shape[0] if cap is None else cap
    out = np.full(len(data) + 6 * idx.shape[0] + 8, fill, np.uint8)
    n = C.c_int(-1)
    rc = _lib.lib().ptts_flac_rebase(src.ctypes.data_as(_lib.U8P), src.size, idx.ctypes.data_as(_lib.I32P), idx.shape[0],
                                     int(delta), out.ctypes.data_as(_lib.U8P), cap, C.byref(n))
    return rc, out, n.value


@pytest.mark.parametrize("n", (17, 257, 4609))
def test_memo_is_flac_frames(n):
    """the shortcut of frames_at is flac_frames at every width of the number"""
    s = signal("noise", n)
    for first in (0, 127, 128, 2047, 2048, 65536, 1 << 21, 1 << 26, 1 << 31, END - n):
        assert frames_at(s, first, 24000) == flac_frames_index(s, first, 24000), first
        assert frames_at(s, first, 24000)[0] == flac_frames(s, first, 24000)


@pytest.mark.parametrize("name", SIGNALS)
@pytest.mark.parametrize("n", SIZES)
def test_rebase_is_flac_frames_at_the_new_number(n, name):
    s = signal(name, n)
    rate = 48000 if n % 2 else 24000
    for f, d in SAME + CROSS + [(7, END - n - 7), (0, END - n), (END - n, 0)]:  # the last ones end at 2^36 exactly
        src, index = frames_at(s, f, rate)
        assert sum(a for a, _ in index) == len(src) and sum(bs for _, bs in index) == n
        want, _ = frames_at(s, f + d, rate)
        got = flac_rebase(src, index, d)
        assert got == want, (n, name, f, d)
        rc, out, nb = raw_rebase(src, index, d)
        assert rc == 0 and nb == len(want) and out[:nb].tobytes() == want and np.all(out[nb:] == 0xAA)


@pytest.mark.parametrize("n", (1, 16, 4608, 11477))
def test_one_sample_past_the_36_bit_number_is_refused(n):
    s = signal("noise", n)
    src, index = flac_frames_index(s, 7, 24000)
    assert flac_rebase(src, index, END - n - 7) == frames_at(s, END - n, 24000)[0]
    rc, out, _ = raw_rebase(src, index, END - n - 6)
    assert rc == 1 and "2^36" in _lib.lib().ptts_last_error().decode() and np.all(out == 0xAA)
    with pytest.raises(ValueError, match="2\\^36"):
        flac_rebase(src, index, END - n - 6)


def flipped(data, byte, bit=0):
    b = bytearray(data)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("n", (300, 11477))
def test_every_rejected_input_leaves_out_untouched(n):
    """n = 11477: the fault sits in the third frame, behind two that pass every check"""
    s = signal("noise", n)
    src, index = flac_frames_index(s, 5, 24000)
    last = len(src) - index[-1][0]  # where the last frame starts
    short = [(a, b) for a, b in index]
    short[-1] = (short[-1][0] - 1, short[-1][1])
    other = [(a, b) for a, b in index]
    other[-1] = (other[-1][0], other[-1][1] - 1)
    cases = {
        "sync": (flipped(src, last + 1, 3), index, 1000, None, "sync"),
        "header bit (CRC-8)": (flipped(src, last + 4, 1), index, 1000, None, "CRC-8"),
        "body bit (CRC-16)": (flipped(src, len(src) - 5, 6), index, 1000, None, "CRC-16"),
        "stored CRC-16": (flipped(src, len(src) - 1), index, 1000, None, "CRC-16"),
        "index sum": (src, short, 1000, None, "sum"),
        "index block size": (src, other, 1000, None, "block size"),
        "negative delta": (src, index, -1, None, "delta"),
        "short out_cap": (src, index, 1000, len(src) + 6 * len(index) - 1, "out_cap"),
    }
    for name, (data, idx, delta, cap, word) in cases.items():
        rc, out, nb = raw_rebase(data, idx, delta, cap)
        msg = _lib.lib().ptts_last_error().decode()
        assert rc == 1 and word in msg, (name, rc, msg)
        assert np.all(out == 0xAA) and nb == -1, name
    rc, out, nb = raw_rebase(src, index, 1000)  # and the untouched input passes
    assert rc == 0 and out[:nb].tobytes() == frames_at(s, 1005, 24000)[0]


@pytest.mark.parametrize("rate", (8000, 48000))
@pytest.mark.parametrize("n", (1, 16, 4608, 4609, 24000))
def test_silence_is_flac_frames_of_zeros(n, rate):
    bound = _lib.lib().ptts_flac_silence_bound(n)
    assert bound == 19 * -(-n // FLAC_BLOCK)
    for base in (0, (1 << 31) - 5):
        got = flac_silence(n, base, rate)
        assert got == flac_frames(np.zeros(n, np.int16), base, rate), (n, rate, base)
        assert len(got) <= bound
    worst = flac_silence(n, END - n, rate)  # seven bytes of number in every frame
    assert worst == flac_frames(np.zeros(n, np.int16), END - n, rate) and len(worst) <= bound
    assert n != FLAC_BLOCK or len(worst) == bound  # and two of block size: the bound is met
    with pytest.raises(ValueError):
        flac_silence(n, END - n + 1, rate)
    assert _lib.lib().ptts_flac_silence_bound(0) == 0 and flac_silence(0, 5, rate) == b""
    out, got = np.full(bound, 0xAA, np.uint8), C.c_long(-1)
    rc = _lib.lib().ptts_flac_silence(n, rate, 0, out.ctypes.data_as(_lib.U8P), bound - 1, C.byref(got))
    assert rc == 1 and np.all(out == 0xAA) and got.value == -1
    assert _lib.lib().ptts_flac_silence(n, 22050, 0, out.ctypes.data_as(_lib.U8P), bound, C.byref(got)) == 1


def test_joiner_makes_one_stream_of_segments_and_pauses():
    """Three segments of different lengths (chunks of one, two and three frames; the first ends in a
    block of 7 samples, which stays as it is inside the stream) with two pauses between them."""
    rate = 24000
    rng = np.random.default_rng(7)
    segs = [[1920, 1920, 7], [11477, 3000], [300]]  # the chunk sizes of each segment
    pauses = [4800, 13]
    j = FlacJoiner(rate)
    sent, want = [], []
    for i, sizes in enumerate(segs):
        at = 0
        for n in sizes:
            s = (2000 * rng.standard_normal(n)).astype(np.int16)
            data, index = flac_frames_index(s, at, rate)  # the row numbers from 0 of its own utterance
            sent.append(j.chunk(data, index))
            want.append(s)
            at += n
        if i < len(pauses):
            sent.append(j.pause(pauses[i]))
            want.append(np.zeros(pauses[i], np.int16))
        else:
            j.end_segment()
    want = np.concatenate(want)
    assert j.total == want.size == sum(map(sum, segs)) + sum(pauses)
    h, got, info = fd.decode_stream(flac_stream_header(rate, j.total) + b"".join(sent))
    assert h["total"] == j.total and h["rate"] == rate
    assert np.array_equal(got, want)
    at = 0
    for first, n, _ in info:  # contiguous from 0 (decode_stream asserts it too)
        assert first == at
        at += n
    assert at == j.total and 7 in [n for _, n, _ in info]
    assert sent[0] == flac_frames(want[:1920], 0, rate)  # the first segment passes through as it is
