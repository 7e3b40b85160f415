"""A small FLAC decoder for the tests, written from the format of DESIGN.md section 21 (RFC 9639's
mono 16-bit subset), not from the encoder: stream header, frame headers (sync, blocksize and rate
codes, the UTF-8-like sample number, CRC-8), CONSTANT / VERBATIM / FIXED subframes with partitioned
Rice codes of method 0, padding and CRC-16. Every check is an assertion."""

from __future__ import annotations

import numpy as np

RATES = {4: 8000, 5: 16000, 7: 24000, 9: 44100, 10: 48000}
# the fixed predictors: coefficients of s[i-1], s[i-2], ..
PREDICTORS = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def crc(data: bytes, poly: int, width: int) -> int:
    """Bit by bit: initial value 0, not reflected, no final XOR."""
    c, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for byte in data:
        c ^= byte << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly if c & top else c << 1) & mask
    return c


class Bits:
    def __init__(self, data: bytes, pos: int = 0):
        self.s = bin(int.from_bytes(b"\1" + data, "big"))[3:]  # one character per bit
        self.pos = 8 * pos

    def u(self, n: int) -> int:
        assert self.pos + n <= len(self.s), "stream cut short"
        v = int(self.s[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def i(self, n: int) -> int:
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        one = self.s.index("1", self.pos)
        q = one - self.pos
        self.pos = one + 1
        return q


def parse_header(data: bytes) -> dict:
    assert data[:4] == b"fLaC"
    assert data[4:8] == bytes([0x80, 0, 0, 0x22]), "one last STREAMINFO block of 34 bytes"
    b = Bits(data, 8)
    h = {"min_block": b.u(16), "max_block": b.u(16), "min_frame": b.u(24), "max_frame": b.u(24), "rate": b.u(20),
         "channels": b.u(3) + 1, "bits": b.u(5) + 1, "total": b.u(36), "md5": b.u(128)}
    assert b.pos == 8 * 42
    return h


def decode_frame(data: bytes, pos: int, rate: int | None = None):
    """One frame at byte `pos` -> (samples int64 [n], first_sample, n, byte length)."""
    b = Bits(data, pos)
    assert b.u(16) == 0xFFF9, "sync code and the variable-blocksize strategy"
    bs_code, rate_code = b.u(4), b.u(4)
    assert bs_code in (6, 7) and rate_code in RATES
    assert rate is None or RATES[rate_code] == rate
    assert b.u(8) == 0x08, "mono, 16 bit, reserved 0"
    lead = b.u(8)
    if lead < 0x80:
        first, nb = lead, 1
    else:
        nb = 8 - (lead ^ 0xFF).bit_length()  # leading ones
        assert 2 <= nb <= 7
        first = lead & (0x7F >> nb)
        for _ in range(nb - 1):
            c = b.u(8)
            assert c >> 6 == 2, "continuation byte"
            first = first << 6 | (c & 0x3F)
        assert first >= (0x80, 1 << 11, 1 << 16, 1 << 21, 1 << 26, 1 << 31)[nb - 2], "shortest form"
    n = b.u(8 if bs_code == 6 else 16) + 1
    assert (n <= 256) == (bs_code == 6), "blocksize code by the block's size"
    hdr_end = b.pos // 8
    assert b.u(8) == crc(data[pos:hdr_end], 0x07, 8), "CRC-8"
    assert b.u(1) == 0
    kind = b.u(6)
    assert b.u(1) == 0, "no wasted bits"
    if kind == 0:
        out = [b.i(16)] * n
    elif kind == 1:
        out = [b.i(16) for _ in range(n)]
    else:
        assert 8 <= kind <= 12, "FIXED of order 0..4"
        o = kind - 8
        out = [b.i(16) for _ in range(o)]
        assert b.u(2) == 0, "Rice with 4-bit parameters"
        p = b.u(4)
        assert n % (1 << p) == 0 and (n >> p) >= o
        for part in range(1 << p):
            k = b.u(4)
            assert k != 15, "no escape partitions"
            for _ in range((n >> p) - (o if part == 0 else 0)):
                q = b.unary()
                u = q << k | b.u(k)
                e = u >> 1 if u & 1 == 0 else -(u >> 1) - 1
                out.append(e + sum(c * out[-1 - j] for j, c in enumerate(PREDICTORS[o])))
    assert len(out) == n
    pad = -b.pos % 8
    assert b.u(pad) == 0, "zero bits to the byte boundary"
    end = b.pos // 8
    assert b.u(16) == crc(data[pos:end], 0x8005, 16), "CRC-16"
    s = np.array(out, np.int64)
    assert s.min() >= -32768 and s.max() <= 32767, "16-bit samples"
    return s, first, n, end + 2 - pos


def decode_frames(data: bytes, rate: int | None = None):
    """Back-to-back frames -> (samples int16, [(first_sample, n, byte length)])."""
    pos, parts, info = 0, [], []
    while pos < len(data):
        s, first, n, size = decode_frame(data, pos, rate)
        parts.append(s)
        info.append((first, n, size))
        pos += size
    assert pos == len(data)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int16), info


def decode_stream(data: bytes):
    """A whole stream -> (header fields, samples, frame infos); sample numbers must be contiguous from 0."""
    h = parse_header(data)
    s, info = decode_frames(data[42:], h["rate"])
    at = 0
    for first, n, _ in info:
        assert first == at, "sample numbers are contiguous from 0"
        assert n <= h["max_block"]
        at += n
    assert h["total"] in (0, at)
    return h, s, info
