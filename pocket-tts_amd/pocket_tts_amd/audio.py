"""Audio I/O of the voice-cloning front end, host side.

Mirrors crates/pocket-tts/src/audio.rs:
  * `read_wav` / `read_wav_from_bytes` (audio.rs:12-108, hound): RIFF/WAVE with integer PCM
    (8/16/24/32 bit, value / 2^(bits-1); 8-bit data is unsigned on disk) or IEEE float32, plain
    or WAVE_FORMAT_EXTENSIBLE; interleaved channels -> [channels, samples]; a data chunk cut short
    keeps the whole samples read so far (the reference accepts truncated files, audio.rs:33-49).
  * `pcm_i16_le_bytes` (audio.rs:110-146): clamp to [-1, 1], x 32767, truncate toward zero,
    channels interleaved.
  * `write_wav` / `wav_bytes` (audio.rs:148-185): 16-bit integer PCM RIFF/WAVE; with an encoding,
    also G.711 mu-law / A-law files (8 bits per sample, an 18-byte fmt chunk and a fact chunk).
  * `lin2ulaw` / `lin2alaw` / `wire_bytes`: the host restatement of the engine's wire stage
    encodings (include/pocket_tts.h, PTTS_WIRE_*): what the GPU writes, for tests and for rows
    that did not go through it.
  * `flac_stream_header` / `flac_frames`: the host restatement of the engine's FLAC stage
    (DESIGN.md section 21): the same blocks and the same choice rule, byte for byte.
  * `flac_rebase` / `flac_silence` / `FlacJoiner`: several rows and pauses as one FLAC stream
    (section 21.5), over the library's host-only ptts_flac_rebase / ptts_flac_silence.
  * `normalize_peak` (audio.rs:187-194).
Resampling to 24 kHz is not here: it runs on the GPU inside `ptts_voice_from_audio`
(the polyphase resampler of pocket-tts_amd/csrc/kernels.hip).
"""

from __future__ import annotations

import math
import struct
from pathlib import Path

import numpy as np

WAVE_FORMAT_PCM = 0x0001
WAVE_FORMAT_IEEE_FLOAT = 0x0003
WAVE_FORMAT_ALAW = 0x0006
WAVE_FORMAT_MULAW = 0x0007
WAVE_FORMAT_EXTENSIBLE = 0xFFFE
ENCODINGS = ("pcm_s16le", "ulaw", "alaw", "flac")  # by PTTS_WIRE_* - 1


class WavError(ValueError):
    pass


def read_wav_from_bytes(data: bytes) -> tuple[np.ndarray, int]:
    """-> (samples float32 [channels, n], sample_rate)."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise WavError("not a RIFF/WAVE file")
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        start = pos + 8
        if cid == b"fmt ":
            if size < 16:
                raise WavError("fmt chunk too short")
            tag, ch, sr, _, align, bits = struct.unpack_from("<HHIIHH", data, start)
            if tag == WAVE_FORMAT_EXTENSIBLE:
                if size < 40:
                    raise WavError("extensible fmt chunk too short")
                tag = struct.unpack_from("<H", data, start + 24)[0]  # first 2 bytes of the subformat GUID
            fmt = (tag, ch, sr, align, bits)
        elif cid == b"data":
            body = data[start:start + size]  # may be shorter than `size`: truncated file
            break
        pos = start + size + (size & 1)  # chunks are word aligned
    if fmt is None:
        raise WavError("missing fmt chunk")
    if body is None:
        raise WavError("missing data chunk")
    tag, ch, sr, align, bits = fmt
    if ch < 1:
        raise WavError("zero channels")
    width = (bits + 7) // 8
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits != 32:
            raise WavError(f"unsupported float width {bits}")
    elif tag != WAVE_FORMAT_PCM or bits not in (8, 16, 24, 32):
        raise WavError(f"unsupported WAV format tag {tag:#x} / {bits} bits")
    frame = width * ch
    n = len(body) // frame
    if n == 0 and len(body) > 0:
        raise WavError("truncated WAV data")
    raw = np.frombuffer(body[:n * frame], np.uint8).reshape(n * ch, width)
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        x = raw.copy().view("<f4").reshape(-1)
    elif bits == 8:
        x = (raw[:, 0].astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)
    else:
        v = np.zeros(n * ch, np.int64)
        for b in range(width):
            v |= raw[:, b].astype(np.int64) << (8 * b)
        sign = np.int64(1) << (bits - 1)
        v = (v ^ sign) - sign
        x = v.astype(np.float32) / np.float32(1 << (bits - 1))
    return np.ascontiguousarray(x.reshape(n, ch).T, np.float32), int(sr)


def read_wav(path) -> tuple[np.ndarray, int]:
    return read_wav_from_bytes(Path(path).read_bytes())


def pcm_i16_le_bytes(audio: np.ndarray) -> bytes:
    """audio [channels, n] (or [n] mono) -> interleaved little-endian int16."""
    a = np.asarray(audio, np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    x = np.clip(a.T, -1.0, 1.0) * np.float32(32767.0)
    return x.astype(np.int16).astype("<i2").tobytes()  # float -> int casts truncate toward zero


def pcm_i16(audio: np.ndarray) -> np.ndarray:
    """The 16-bit wire value of every sample: trunc(clip(x, -1, 1) * 32767) in float32."""
    x = np.clip(np.asarray(audio, np.float32), -1.0, 1.0) * np.float32(32767.0)
    return x.astype(np.int16)


def lin2ulaw(s: np.ndarray) -> np.ndarray:
    """G.711 mu-law code (uint8) of 16-bit samples: the rule of the engine's wire stage, equal to
    CPython's audioop.lin2ulaw(.., 2) on all 65,536 inputs."""
    v = np.asarray(s, np.int16).astype(np.int32) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8159) + 33
    seg = np.searchsorted(np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF]), v, side="left")
    code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | ((v >> (np.minimum(seg, 7) + 1)) & 15))
    return (code ^ mask).astype(np.uint8)


def lin2alaw(s: np.ndarray) -> np.ndarray:
    """G.711 A-law code (uint8) of 16-bit samples; equal to audioop.lin2alaw(.., 2) on all inputs."""
    s = np.asarray(s, np.int16).astype(np.int32)
    mask = np.where(s >= 0, 0xD5, 0x55)
    v = np.where(s >= 0, s >> 3, (-s - 1) >> 3)
    seg = np.searchsorted(np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]), v, side="left")
    code = (seg << 4) | ((v >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ mask).astype(np.uint8)


def wire_bytes(audio: np.ndarray, encoding: str = "pcm_s16le") -> bytes:
    """Mono float32 samples (already at the wire rate) -> the bytes of `encoding`."""
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding must be one of {list(ENCODINGS)}, got {encoding!r}")
    if encoding == "flac":
        raise ValueError("flac is a stream of frames, not a per-sample encoding: flac_stream_header + flac_frames")
    s = pcm_i16(np.asarray(audio, np.float32).reshape(-1))
    if encoding == "pcm_s16le":
        return s.astype("<i2").tobytes()
    return (lin2ulaw(s) if encoding == "ulaw" else lin2alaw(s)).tobytes()


def wav_header(n_data: int, sample_rate: int = 24000, encoding: str = "pcm_s16le", channels: int = 1) -> bytes:
    """RIFF/WAVE header in front of n_data bytes of `encoding`: format tag 1 (16-bit PCM, a 16-byte
    fmt chunk), or 7 (mu-law) / 6 (A-law) with 8 bits per sample, an 18-byte fmt chunk (cbSize 0)
    and a fact chunk holding the sample count per channel, as non-PCM formats require."""
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding must be one of {list(ENCODINGS)}, got {encoding!r}")
    if encoding == "flac":
        raise ValueError("a WAV file cannot carry flac: send the FLAC stream itself (flac_stream_header + frames)")
    ch = channels
    if encoding == "pcm_s16le":
        fmt = b"fmt " + struct.pack("<IHHIIHH", 16, WAVE_FORMAT_PCM, ch, sample_rate, sample_rate * 2 * ch, 2 * ch, 16)
        fact = b""
    else:
        tag = WAVE_FORMAT_MULAW if encoding == "ulaw" else WAVE_FORMAT_ALAW
        fmt = b"fmt " + struct.pack("<IHHIIHHH", 18, tag, ch, sample_rate, sample_rate * ch, ch, 8, 0)
        fact = b"fact" + struct.pack("<II", 4, n_data // ch)
    body = fmt + fact + b"data" + struct.pack("<I", n_data)
    return b"RIFF" + struct.pack("<I", 4 + len(body) + n_data + (n_data & 1)) + b"WAVE" + body


def wav_bytes(audio, sample_rate: int = 24000, encoding: str = "pcm_s16le") -> bytes:
    """A WAV file of `audio`: float32 samples [channels, n] or [n] (encoded here: 16-bit by
    pcm_i16_le_bytes, G.711 mono by wire_bytes), or bytes already in `encoding` (mono; what
    Engine.fetch_wire returned)."""
    if isinstance(audio, (bytes, bytearray, memoryview)):
        data, ch = bytes(audio), 1
    else:
        a = np.asarray(audio, np.float32)
        ch = 1 if a.ndim == 1 else a.shape[0]
        if encoding == "pcm_s16le":
            data = pcm_i16_le_bytes(a)
        else:
            if ch != 1:
                raise ValueError("G.711 output is mono")
            data = wire_bytes(a, encoding)
    return wav_header(len(data), sample_rate, encoding, ch) + data + (b"\0" if len(data) & 1 else b"")


def write_wav(path, audio: np.ndarray, sample_rate: int = 24000) -> None:
    Path(path).write_bytes(wav_bytes(audio, sample_rate))


# ---- FLAC: the host restatement of DESIGN.md section 21 (the GPU FLAC stage's format and rule)
FLAC_BLOCK = 4608  # samples per frame at most (the subset limit at <= 48 kHz)
FLAC_RATE_CODES = {8000: 4, 16000: 5, 24000: 7, 44100: 9, 48000: 10}


def wire_samples(n: int, rate: int, sp: int = 0, cents: int = 0) -> int:
    """Samples at `rate` of an utterance of n samples at 24 kHz (time-scaled first at a speed of sp
    permille, 0: none, and shifted by `cents`, 0: none): what its wire chunks add up to
    (ceil(n' rate / 24000))."""
    if cents:
        sp_w, step = pitch_plan(cents, sp)
        n = pitch_len(tempo_len(n, sp_w) if sp_w != 1000 else int(n), step)
    else:
        n = tempo_len(n, sp) if sp else int(n)
    return -(-n * int(rate) // 24000)


def flac_stream_header(rate: int, total_samples: int = 0) -> bytes:
    """`fLaC` and one STREAMINFO block (42 bytes): block sizes 16 .. 4608, frame sizes unknown, mono,
    16 bit, total_samples (0: unknown, for streams), no MD5."""
    if rate not in FLAC_RATE_CODES:
        raise ValueError(f"sample rate must be one of {sorted(FLAC_RATE_CODES)}")
    if not 0 <= total_samples < 1 << 36:
        raise ValueError("total_samples must fit 36 bits")
    word = (int(rate) << 44) | (0 << 41) | (15 << 36) | int(total_samples)
    info = struct.pack(">HH", 16, FLAC_BLOCK) + bytes(6) + word.to_bytes(8, "big") + bytes(16)
    return b"fLaC" + bytes([0x80, 0, 0, 0x22]) + info


def _crc_table(poly: int, bits: int) -> list[int]:
    top, mask, out = 1 << (bits - 1), (1 << bits) - 1, []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly if c & top else c << 1) & mask
        out.append(c)
    return out


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def flac_crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def flac_crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def flac_number(v: int) -> bytes:
    """The UTF-8-like code of a frame's first sample index, extended to 36 bits."""
    if v < 0x80:
        return bytes([v])
    nb = next(i for i, lim in enumerate((11, 16, 21, 26, 31, 36), 2) if v < 1 << lim)
    first = ((0xFF << (8 - nb)) & 0xFF) | (0 if nb == 7 else v >> (6 * (nb - 1)))
    return bytes([first] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(nb - 2, -1, -1)])


def flac_choose(s: np.ndarray):
    """The choice rule on one block (int64 samples): ("constant",), ("verbatim",) or
    ("fixed", order, partition order, parameters [2^p])."""
    n = s.size
    if np.all(s == s[0]):
        return ("constant",)
    best, pick = 8 + 16 * n, ("verbatim",)
    if n < 16:
        return pick
    pmax = min((n & -n).bit_length() - 1, 6)
    while (n >> pmax) < 16:
        pmax -= 1
    ks = np.arange(15, dtype=np.int64)[:, None]
    for o in range(5):
        e = np.diff(s, o) if o else s
        u = np.concatenate([np.zeros(o, np.int64), np.where(e >= 0, 2 * e, -2 * e - 1)])
        fine = (u[None, :] >> ks).reshape(15, 1 << pmax, -1).sum(axis=2)  # [k][finest partition]
        for p in range(pmax + 1):
            cnt = np.full(1 << p, n >> p, np.int64)
            cnt[0] -= o
            cost = fine.reshape(15, 1 << p, -1).sum(axis=2) + cnt[None, :] * (ks + 1)
            k = cost.argmin(axis=0)  # the first minimum: the lower k
            total = 8 + 16 * o + 6 + int((cost.min(axis=0) + 4).sum())
            if total < best:
                best, pick = total, ("fixed", o, p, k)
    return pick


def _flac_pack(fields_val, fields_nb, fields_skip) -> np.ndarray:
    """Bit fields (value, width <= 16, zero bits before it), in order -> the bits (uint8 0/1)."""
    val = np.asarray(fields_val, np.int64)
    nb = np.asarray(fields_nb, np.int64)
    skip = np.asarray(fields_skip, np.int64)
    end = np.cumsum(nb + skip)
    pos = end - nb  # where each field's value starts
    bits = np.zeros(int(end[-1]) if end.size else 0, np.uint8)
    for b in range(int(nb.max()) if nb.size else 0):
        m = nb > b
        bits[pos[m] + b] = (val[m] >> (nb[m] - 1 - b)) & 1
    return bits


def flac_frame(s: np.ndarray, first_sample: int, rate: int) -> bytes:
    """One FLAC frame of the block s (1 .. 4608 int16 samples) whose first sample has that index."""
    s = np.asarray(s, np.int16).astype(np.int64).reshape(-1)
    n = s.size
    if not 1 <= n <= FLAC_BLOCK:
        raise ValueError("a block holds 1 .. 4608 samples")
    head = bytes([0xFF, 0xF9, ((6 if n <= 256 else 7) << 4) | FLAC_RATE_CODES[rate], 0x08]) + flac_number(first_sample)
    head += bytes([n - 1]) if n <= 256 else struct.pack(">H", n - 1)
    head += bytes([flac_crc8(head)])
    pick = flac_choose(s)
    if pick[0] == "constant":
        body = bytes([0x00]) + struct.pack(">h", int(s[0]))
    elif pick[0] == "verbatim":
        body = bytes([0x02]) + s.astype(">i2").tobytes()
    else:
        _, o, p, k = pick
        e = np.diff(s, o) if o else s
        u = np.where(e >= 0, 2 * e, -2 * e - 1)
        i = np.arange(o, n)
        kk = k[i // (n >> p)]
        # per residual: an optional prefix (the method, partition order and first parameter, or a
        # partition's parameter), then u >> k zeros and the one bit with the k low bits
        pre_nb = np.where(i == o, 10, np.where(i % (n >> p) == 0, 4, 0))
        pre_val = np.where(i == o, (p << 4) | kk, kk)
        val = np.stack([pre_val, (1 << kk) | (u & ((1 << kk) - 1))], axis=1).reshape(-1)
        nb = np.stack([pre_nb, kk + 1], axis=1).reshape(-1)
        skip = np.stack([np.zeros_like(u), u >> kk], axis=1).reshape(-1)
        warm = s[:o] & 0xFFFF
        bits = _flac_pack(np.concatenate([[(8 | o) << 1], warm, val]), np.concatenate([[8], np.full(o, 16), nb]),
                          np.concatenate([np.zeros(1 + o, np.int64), skip]))
        body = np.packbits(bits).tobytes()  # zero bits to the byte boundary
    frame = head + body
    return frame + struct.pack(">H", flac_crc16(frame))


def flac_frames(samples_i16, first_sample: int, rate: int) -> bytes:
    """The FLAC frames of a chunk of 16-bit samples (blocks of 4,608, the last one shorter), the
    first of which has index first_sample in its stream: what the engine's FLAC stage writes for
    that chunk, byte for byte."""
    s = np.asarray(samples_i16, np.int16).reshape(-1)
    if rate not in FLAC_RATE_CODES:
        raise ValueError(f"sample rate must be one of {sorted(FLAC_RATE_CODES)}")
    if first_sample < 0 or first_sample + s.size > 1 << 36:
        raise ValueError("sample indices must fit 36 bits")
    return b"".join(flac_frame(s[a:a + FLAC_BLOCK], first_sample + a, rate) for a in range(0, s.size, FLAC_BLOCK))


def flac_frames_index(samples_i16, first_sample: int, rate: int) -> tuple[bytes, list[tuple[int, int]]]:
    """flac_frames with the chunk's frame index: (frames, [(byte length, block size) per frame]), what
    the FLAC stage writes beside the chunk (ptts_fetch_flac_index)."""
    s = np.asarray(samples_i16, np.int16).reshape(-1)
    frames = [flac_frames(s[a:a + FLAC_BLOCK], first_sample + a, rate) for a in range(0, s.size, FLAC_BLOCK)]
    return b"".join(frames), [(len(f), min(FLAC_BLOCK, s.size - a)) for f, a in zip(frames, range(0, s.size, FLAC_BLOCK))]


def flac_rebase(chunk: bytes, index, delta: int) -> bytes:
    """The frames of `chunk` (index: (byte length, block size) per frame) with every sample number
    raised by delta >= 0 and both CRCs renewed, the body bits untouched (ptts_flac_rebase; host only):
    flac_rebase(flac_frames(s, f, rate), index, d) == flac_frames(s, f + d, rate). ValueError for
    frames that do not verify against their CRCs or the index, and for numbers past 2^36."""
    import ctypes as C

    from ._lib import I32P, U8P, lib
    idx = np.ascontiguousarray(np.asarray(index, np.int32).reshape(-1, 2))
    src = np.frombuffer(bytes(chunk), np.uint8)
    out = np.zeros(max(src.size + 6 * idx.shape[0], 1), np.uint8)
    n = C.c_int(0)
    if lib().ptts_flac_rebase(src.ctypes.data_as(U8P), src.size, idx.ctypes.data_as(I32P), idx.shape[0], int(delta),
                              out.ctypes.data_as(U8P), out.size, C.byref(n)) != 0:
        raise ValueError(lib().ptts_last_error().decode(errors="replace"))
    return out[: n.value].tobytes()


def flac_silence(n: int, first_sample: int, rate: int) -> bytes:
    """n zero samples as CONSTANT frames in blocks of 4,608 (ptts_flac_silence; host only): equal to
    flac_frames(np.zeros(n, np.int16), first_sample, rate), without the search."""
    import ctypes as C

    from ._lib import U8P, lib
    out = np.zeros(max(int(lib().ptts_flac_silence_bound(int(n))), 1), np.uint8)
    got = C.c_long(0)
    if lib().ptts_flac_silence(int(n), int(rate), int(first_sample), out.ctypes.data_as(U8P), out.size, C.byref(got)) != 0:
        raise ValueError(lib().ptts_last_error().decode(errors="replace"))
    return out[: got.value].tobytes()


class FlacJoiner:
    """The segments of one response as one FLAC stream: every row numbers its
    frames from sample 0 of its own utterance, and this is the only place that knows where a segment
    starts. chunk() and pause() return the bytes to send behind flac_stream_header(rate); a segment's
    chunks go in order, end_segment() closes it (pause() does too). total: the samples so far."""

    def __init__(self, rate: int):
        if rate not in FLAC_RATE_CODES:
            raise ValueError(f"sample rate must be one of {sorted(FLAC_RATE_CODES)}")
        self.rate = int(rate)
        self.total = 0   # samples of everything returned so far
        self._base = 0   # where the open segment's sample 0 lies

    def chunk(self, data: bytes, index) -> bytes:
        """One chunk of the open segment with its frame index, renumbered to its place."""
        if not data:
            return b""
        out = flac_rebase(data, index, self._base) if self._base else bytes(data)
        self.total += sum(int(bs) for _, bs in index)
        return out

    def end_segment(self) -> None:
        """The next chunk is the first of another row: it starts where this one ends."""
        self._base = self.total

    def pause(self, n_samples: int) -> bytes:
        """n_samples of silence between two segments (closes the open one)."""
        self.end_segment()
        out = flac_silence(n_samples, self.total, self.rate) if n_samples > 0 else b""
        self.total += max(int(n_samples), 0)
        self._base = self.total
        return out


def normalize_peak(audio: np.ndarray) -> np.ndarray:
    a = np.asarray(audio, np.float32)
    m = float(np.abs(a).max()) if a.size else 0.0
    return (a * np.float32(1.0 / m)).astype(np.float32) if m > 0 else a.copy()


# ---- speech speed: the host restatement of DESIGN.md section 19 (the GPU tempo stage's rule)
TEMPO_W, TEMPO_HS, TEMPO_D = 480, 240, 120  # window, synthesis hop, search radius
TEMPO_R = TEMPO_D + TEMPO_HS + TEMPO_W  # hop k runs once a_k + TEMPO_R samples are in
TEMPO_SPEED_MIN, TEMPO_SPEED_MAX = 500, 2000  # permille


def speed_permille(speed) -> int:
    """A speed factor (1.0 = unchanged) as the integer permille the engine takes; 0 for None or 1.0.
    ValueError outside [0.5, 2.0]."""
    if speed is None:
        return 0
    f = float(speed)
    sp = round(f * 1000) if math.isfinite(f) else -1
    if not TEMPO_SPEED_MIN <= sp <= TEMPO_SPEED_MAX:
        raise ValueError(f"speed must be in [0.5, 2.0], got {speed!r}")
    return 0 if sp == 1000 else sp


def tempo_len(n: int, sp: int) -> int:
    """Samples of an n-sample utterance at speed sp (permille): ceil(n * 1000 / sp)."""
    return (int(n) * 1000 + int(sp) - 1) // int(sp)


def tempo_window() -> np.ndarray:
    """w[i] = 0.5 - 0.5 cos(2 pi i / W) in f64, rounded to f32."""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / TEMPO_W) for i in range(TEMPO_W)], np.float32)


def tempo_hops_ready(n: int, sp: int) -> int:
    """Hops a stream has run after n samples (not its last frame): the k with a_k + TEMPO_R <= n."""
    k = 0
    while k * TEMPO_HS * sp // 1000 + TEMPO_R <= n:
        k += 1
    return k


def tempo_chunk_samples(frame: int, sp: int, last: bool, frame_len: int = 1920) -> int:
    """Samples the tempo stage emits in frame `frame` (0-based) of a row at speed sp: a pure function
    of (frame, sp, last). The last frame emits the rest up to tempo_len of the utterance."""
    n0, n1 = frame * frame_len, (frame + 1) * frame_len
    before = tempo_hops_ready(n0, sp) * TEMPO_HS
    return (tempo_len(n1, sp) if last else tempo_hops_ready(n1, sp) * TEMPO_HS) - before


def tempo_wsola(x: np.ndarray, sp: int, frame_len: int | None = None):
    """WSOLA time-scaling of mono f32 PCM at 24 kHz by sp permille: tempo_len(len(x), sp) samples.
    Every product is f32 x f32 in f64 (exact), every sum runs in the stated order, so the GPU stage
    agrees bit for bit. frame_len: run frame by frame as the stream does (hop k as soon as
    a_k + TEMPO_R samples are in, the rest in the last frame) and return the list of chunks."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    sp = int(sp)
    if not TEMPO_SPEED_MIN <= sp <= TEMPO_SPEED_MAX:
        raise ValueError(f"speed must be in [{TEMPO_SPEED_MIN}, {TEMPO_SPEED_MAX}] permille, got {sp}")
    n = x.size
    W, HS, D = TEMPO_W, TEMPO_HS, TEMPO_D
    L = tempo_len(n, sp)
    hops = (L + HS - 1) // HS
    # zeros past the end: the furthest read is a_k + D + W or p_{k-1} + HS + W
    xd = np.concatenate([x.astype(np.float64), np.zeros(hops * HS * sp // 1000 + TEMPO_R + W + 1)])
    w = tempo_window().astype(np.float64)
    scan = [0] + [d for j in range(1, D + 1) for d in (-j, j)]
    y = np.zeros(hops * HS, np.float32)
    starts = np.arange(-D, D + 1)
    p_prev = 0
    for k in range(hops):
        if k == 0:
            p = 0
            y[:HS] = x[:HS] if n >= HS else xd[:HS].astype(np.float32)
        else:
            a = k * HS * sp // 1000
            t = xd[p_prev + HS: p_prev + HS + W]
            c = np.zeros(2 * D + 1)
            for q in range(4):
                acc = np.zeros(2 * D + 1)
                for i in range(120 * q, 120 * q + 120):  # ascending i, all shifts at once
                    acc += xd[a + starts + i] * t[i]
                c = acc if q == 0 else c + acc
            best = 0
            for d in scan[1:]:
                if c[d + D] > c[best + D]:
                    best = d
            p = a + best
            y[k * HS:(k + 1) * HS] = (w[:HS] * xd[p: p + HS] + w[HS:] * xd[p_prev + HS: p_prev + W]).astype(np.float32)
        p_prev = p
    y = y[:L]
    if frame_len is None:
        return y
    chunks, done, nfr = [], 0, (n + frame_len - 1) // frame_len
    for f in range(nfr):
        end = L if f == nfr - 1 else tempo_hops_ready((f + 1) * frame_len, sp) * HS
        chunks.append(y[done:end])
        done = end
    return chunks



# ---- pitch: the host restatement of DESIGN.md section 23 (the GPU pitch stage's rule)
PITCH_CENTS_MAX = 1200
PITCH_Z, PITCH_P, PITCH_BETA = 32, 512, 12.0  # zero crossings a side, table entries per crossing, Kaiser beta
PITCH_ONE = 1 << 20  # a step is Q20: input samples per output sample
_PITCH_TABLE = None


def pitch_cents(pitch) -> int:
    """A pitch shift in semitones as the integer cents the engine takes; 0 for None or 0.
    ValueError outside [-12, 12]."""
    if pitch is None:
        return 0
    f = float(pitch)
    c = round(100.0 * f) if math.isfinite(f) else PITCH_CENTS_MAX + 1
    if not -PITCH_CENTS_MAX <= c <= PITCH_CENTS_MAX:
        raise ValueError(f"pitch must be in [-12, 12] semitones, got {pitch!r}")
    return c


def pitch_plan(cents: int, sp: int = 0) -> tuple[int, int]:
    """(sp_w, step) of a pitch of `cents` at speed sp permille (0: 1000): the speed the WSOLA stage
    runs at and the resampler's Q20 step, from the library's ptts_pitch_plan (the single source of the
    rule). ValueError for an invalid request (cents outside [-1200, 1200], sp_w outside [500, 2000])."""
    import ctypes as C

    from ._lib import lib
    w, st = C.c_int(0), C.c_uint32(0)
    if lib().ptts_pitch_plan(int(cents), int(sp), C.byref(w), C.byref(st)) != 0:
        raise ValueError(f"pitch of {cents} cents at speed {sp or 1000} permille is outside the valid range "
                         "(cents in [-1200, 1200], speed / 2^(cents / 1200) in [0.5, 2.0])")
    return w.value, st.value


def pitch_cq(step: int) -> int:
    """The cutoff scale in Q20: min(2^20, floor(2^40 / step))."""
    return min(PITCH_ONE, (1 << 40) // int(step))


def pitch_support(step: int) -> int:
    """H: the one-sided support in input samples, ceil(Z 2^20 / cq) + 1."""
    cq = pitch_cq(step)
    return -(-(PITCH_Z << 20) // cq) + 1


def pitch_len(n: int, step: int) -> int:
    """Outputs of n inputs: floor(n 2^20 / step)."""
    return (int(n) << 20) // int(step)


def pitch_emitted(n: int, step: int) -> int:
    """Outputs a stream has emitted after n inputs (not its last frame): the m with
    (m step >> 20) + H <= n - 1, ceil((n - H) 2^20 / step)."""
    h = pitch_support(step)
    return -(-((int(n) - h) << 20) // int(step)) if n > h else 0


def pitch_chunk_samples(n_before: int, n_after: int, step: int, last: bool) -> int:
    """Samples the pitch stage emits in the frame that takes a row from n_before to n_after inputs: a
    pure function of the plan and the input counts. The last frame emits the rest up to pitch_len."""
    return (pitch_len(n_after, step) if last else pitch_emitted(n_after, step)) - pitch_emitted(n_before, step)


def _bessel_i0(x: np.ndarray) -> np.ndarray:
    """The power series of the library's bessel_i0, term by term in its order (terms past its stopping
    point do not change the f64 sum)."""
    x = np.asarray(x, np.float64)
    s, t, q = np.ones_like(x), np.ones_like(x), 0.25 * x * x
    for k in range(1, 500):
        t = t * (q / (float(k) * k))
        s = s + t
    return s


def pitch_table() -> tuple[np.ndarray, np.ndarray]:
    """(T, D): T[i] = f32(sinc(i / P) kaiser_beta(i / (P Z))) for 0 <= i <= Z P + 1, computed in f64,
    exactly 0 at the sinc's zeros and past Z P, T[0] = 1; D[i] = f32(T[i + 1] - T[i])."""
    global _PITCH_TABLE
    if _PITCH_TABLE is None:
        n = PITCH_Z * PITCH_P
        i = np.arange(1, n)
        r = i / float(PITCH_P * PITCH_Z)
        kais = _bessel_i0(PITCH_BETA * np.sqrt(1.0 - r * r)) / float(_bessel_i0(np.float64(PITCH_BETA)))
        sinc = np.array([math.sin(math.pi * (k / PITCH_P)) / (math.pi * (k / PITCH_P)) for k in range(1, n)])
        t = np.zeros(n + 2, np.float32)
        t[0] = 1.0
        t[1:n] = (sinc * kais).astype(np.float32)
        t[PITCH_P:n:PITCH_P] = 0.0
        d = (t[1:].astype(np.float64) - t[:-1].astype(np.float64)).astype(np.float32)
        _PITCH_TABLE = (t, d)
    return _PITCH_TABLE


def _pitch_outputs(buf: np.ndarray, base: int, n: int, m0: int, m1: int, step: int) -> np.ndarray:
    """Outputs m0 <= m < m1 of the signal whose sample j is buf[j - base] for base <= j < n (0 outside
    [0, n)): per output one ascending f64 chain over j = i0 - H .. i0 + H."""
    t, d = pitch_table()
    cq, h_side, zp = pitch_cq(step), pitch_support(step), PITCH_Z * PITCH_P
    m = np.arange(m0, m1, dtype=np.int64)
    pos = m * int(step)
    i0 = pos >> 20
    acc = np.zeros(m.size, np.float64)
    for k in range(-h_side, h_side + 1):
        j = i0 + k
        q = (np.abs(pos - (j << 20)) * cq) >> 20
        qp = q * PITCH_P
        ti = qp >> 20
        live = ti < zp
        tc = np.minimum(ti, zp - 1)
        fr = (qp & (PITCH_ONE - 1)).astype(np.float64) / float(PITCH_ONE)
        h = (t[tc].astype(np.float64) + d[tc].astype(np.float64) * fr).astype(np.float32)
        h[~live] = 0.0
        inside = (j >= 0) & (j >= base) & (j < n)
        u = np.where(inside, buf[np.clip(j - base, 0, max(buf.size - 1, 0))], np.float32(0.0)) if buf.size else \
            np.zeros(m.size, np.float32)
        acc += u.astype(np.float64) * h.astype(np.float64)
    return (acc * (cq / float(PITCH_ONE))).astype(np.float32)


def pitch_resample(x: np.ndarray, step: int, chunks=None):
    """The fractional resampler of the pitch stage: x (f32) read at step / 2^20 input samples per
    output sample, pitch_len(len(x), step) outputs. Every product is exact in f64 and every sum runs in
    the stated order, so the GPU stage agrees bit for bit. chunks: the sizes in which the input
    arrives (they sum to len(x); the last one is the row's last frame): run as the stream does,
    keeping only the last 2 H + 2 inputs between chunks, and return the list of output chunks."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    step = int(step)
    if not PITCH_ONE // 2 <= step <= PITCH_ONE * 2:
        raise ValueError(f"step must be in [2^19, 2^21], got {step}")
    if chunks is None:
        return _pitch_outputs(x, 0, x.size, 0, pitch_len(x.size, step), step)
    sizes = [int(c) for c in chunks]
    if sum(sizes) != x.size or any(c < 0 for c in sizes):
        raise ValueError("chunks must be non-negative and sum to len(x)")
    keep = 2 * pitch_support(step) + 2
    hist, n, e, out = np.zeros(0, np.float32), 0, 0, []
    for f, c in enumerate(sizes):
        buf = np.concatenate([hist, x[n:n + c]])
        base, n = n - hist.size, n + c
        e1 = pitch_len(n, step) if f == len(sizes) - 1 else pitch_emitted(n, step)
        out.append(_pitch_outputs(buf, base, n, e, e1, step))
        e, hist = e1, buf[-keep:]
    return out


# ---- level: the host restatement of DESIGN.md section 24 (the GPU level stage's rule)
LEVEL_L = 126  # samples of look-ahead (5.25 ms at 24 kHz)
LEVEL_GAIN_DB_MAX = 24.0
LEVEL_TAPS = (64 - np.abs(np.arange(LEVEL_L + 1) - 63)).astype(np.float64)  # a triangle: two 64-boxes convolved; sum 4096


def level_cdb(db, lo: float = -LEVEL_GAIN_DB_MAX, hi: float = LEVEL_GAIN_DB_MAX, name: str = "volume_db") -> int:
    """A level in dB as the integer hundredths of a dB the engine takes; 0 for None. ValueError
    outside [lo, hi]."""
    if db is None:
        return 0
    f = float(db)
    c = round(100.0 * f) if math.isfinite(f) else None
    if c is None or not round(100 * lo) <= c <= round(100 * hi):
        raise ValueError(f"{name} must be in [{lo:g}, {hi:g}] dB, got {db!r}")
    return c


def level_plan(gain_cdb: int, ceiling_cdb: int = -100) -> tuple[np.float32, np.float32]:
    """(v, C): the f32 gain and ceiling of (gain_cdb, ceiling_cdb), (float)pow(10, cdb / 2000), from the
    library's ptts_level_plan (the single source of the two floats). ValueError outside [-2400, 2400]
    and [-4000, 0]."""
    import ctypes as C

    from ._lib import lib
    v, c = C.c_float(0), C.c_float(0)
    if lib().ptts_level_plan(int(gain_cdb), int(ceiling_cdb), C.byref(v), C.byref(c)) != 0:
        raise ValueError(f"gain of {gain_cdb} cdB with a ceiling of {ceiling_cdb} cdB is outside the valid range "
                         "(gain in [-2400, 2400], ceiling in [-4000, 0])")
    return np.float32(v.value), np.float32(c.value)


def level_emitted(n: int) -> int:
    """Outputs a stream has emitted after n inputs (not its last frame): max(n - L, 0)."""
    return max(int(n) - LEVEL_L, 0)


def level_chunk_samples(seen_before: int, seen_after: int, last: bool) -> int:
    """Samples the level stage emits in the frame that takes a row from seen_before to seen_after
    inputs. The last frame emits the rest up to seen_after."""
    return (int(seen_after) if last else level_emitted(seen_after)) - level_emitted(seen_before)


def _level_outputs(u: np.ndarray, base: int, n0: int, n1: int, c: np.float32):
    """Outputs n0 <= n < n1 of the signal whose u[j] is u[j - base] for base <= j < base + len(u) and
    whose r is 1 everywhere else: (y, g, r) of those outputs."""
    L = LEVEL_L
    lo, hi = n0 - 2 * L, n1 + L  # r over [lo, hi), m over [lo, n1), g over [n0, n1)
    r = np.ones(hi - lo, np.float32)
    j0, j1 = max(lo, base), min(hi, base + u.size)
    if j1 > j0:
        a = np.abs(u[j0 - base:j1 - base])
        over = a > c
        r[j0 - lo:j1 - lo] = np.where(over, c / np.where(over, a, np.float32(1.0)), np.float32(1.0))
    m = np.lib.stride_tricks.sliding_window_view(r, L + 1).min(axis=1)  # m[i - lo], lo <= i < n1
    acc = np.zeros(n1 - n0, np.float64)
    for k in range(L + 1):  # ascending k, as the kernel sums
        acc += LEVEL_TAPS[k] * m[n0 - k - lo:n1 - k - lo].astype(np.float64)
    g = (acc / 4096.0).astype(np.float32)
    un = np.zeros(n1 - n0, np.float32)
    a0, a1 = max(n0, base), min(n1, base + u.size)
    if a1 > a0:
        un[a0 - n0:a1 - n0] = u[a0 - base:a1 - base]
    y = np.minimum(np.maximum(g * un, -c), c)
    return y, g, r[2 * L:2 * L + (n1 - n0)]


def level_limit(x: np.ndarray, gain_cdb: int, ceiling_cdb: int = -100, chunks=None, detail: bool = False):
    """The level stage's rule over a whole signal x (f32 at 24 kHz): u = v x, r = |u| > C ? C / |u| : 1
    (1 outside the signal), m[i] = min(r[i .. i + L]), g[n] = f32(sum_k w[k] m[n - k] / 4096) in f64 in
    ascending k, y = clamp(g u, -C, C); len(x) outputs. detail: (y, u, r, g) instead of y. Every product
    of the sum is exact and the sum runs in the stated order, so the GPU stage agrees bit for bit.
    chunks: the sizes in which the input arrives (they sum to len(x); the last one is the row's last
    frame): run as the stream does, keeping only the last 2 L values of u between chunks, and return
    the list of output chunks."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    v, c = level_plan(gain_cdb, ceiling_cdb)
    if chunks is None:
        u = v * x
        y, g, r = _level_outputs(u, 0, 0, x.size, c)
        return (y, u, r, g) if detail else y
    sizes = [int(s) for s in chunks]
    if sum(sizes) != x.size or any(s < 0 for s in sizes):
        raise ValueError("chunks must be non-negative and sum to len(x)")
    hist, n, out = np.zeros(0, np.float32), 0, []
    for f, s in enumerate(sizes):
        buf = np.concatenate([hist, v * x[n:n + s]])
        base, e0, n = n - hist.size, level_emitted(n), n + s
        e1 = n if f == len(sizes) - 1 else level_emitted(n)
        out.append(_level_outputs(buf, base, e0, e1, c)[0])
        hist = buf[-2 * LEVEL_L:] if buf.size else buf
    return out


# ---- loudness: the host restatement of DESIGN.md section 27 (the GPU loudness stage's rule)
LOUD_SUB = 2400  # samples of a sub-block (100 ms at 24 kHz)
LOUD_G = 32      # samples of a segment
_LOUD_SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)  # f0, G (dB), Q
_LOUD_HIGHPASS = (38.13547087602444, 0.5003270373238773)                  # f0, Q


def kweight_coeffs(fs: float = 24000.0) -> np.ndarray:
    """The K-weighting of ITU-R BS.1770 at sample rate fs: [2, 5] float64, the shelf then the
    high-pass, each (b0, b1, b2, a1, a2). At 48000 this is the standard's table; the engine uses
    24000 (ptts_loud_coeffs returns the same bits). Scalar libm calls only, each operation once."""
    fs = float(fs)
    f0, G, Q = _LOUD_SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = _LOUD_HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], np.float64)


def loudness_tables(c: np.ndarray) -> np.ndarray:
    """[2, 2, 32]: per biquad of c the correction tables p and q of section 27, the recursion
    v = (-a1 y1) - a2 y2 run from (y1, y2) = (1, 0) and from (0, 1)."""
    out = np.zeros((2, 2, LOUD_G), np.float64)
    for bq in range(2):
        a1, a2 = float(c[bq][3]), float(c[bq][4])
        for w, (y1, y2) in enumerate(((1.0, 0.0), (0.0, 1.0))):
            for i in range(LOUD_G):
                v = (-a1 * y1) - a2 * y2
                out[bq, w, i] = v
                y2, y1 = y1, v
    return out


def _loud_biquad(c, pq, x: np.ndarray, xs, ys):
    """One biquad over x (f64, a multiple of 32 samples starting on a segment boundary) by the three
    steps of section 27. xs = (x[-1], x[-2]), ys = (y[-1], y[-2]). Returns y."""
    b0, b1, b2, a1, a2 = (np.float64(v) for v in c)
    S = x.size // LOUD_G
    ext = np.concatenate([np.array([xs[1], xs[0]], np.float64), x])
    X = np.lib.stride_tricks.sliding_window_view(ext, LOUD_G + 2)[::LOUD_G]  # [S, 34]: x[-2], x[-1], x[0..31]
    z = np.zeros((S, LOUD_G), np.float64)
    z1 = np.zeros(S, np.float64)
    z2 = np.zeros(S, np.float64)
    for k in range(LOUD_G):  # the zero-state pass, all segments at once
        acc = b0 * X[:, k + 2] + b1 * X[:, k + 1]
        acc = acc + b2 * X[:, k]
        acc = acc - a1 * z1
        acc = acc - a2 * z2
        z[:, k] = acc
        z2, z1 = z1, acc
    p, q = pq
    p1, q1, p2, q2 = p[-1], q[-1], p[-2], q[-2]
    e1 = np.zeros(S + 1, np.float64)
    e2 = np.zeros(S + 1, np.float64)
    e1[0], e2[0] = ys
    za, zb = z[:, -1], z[:, -2]
    a, b = np.float64(ys[0]), np.float64(ys[1])
    for s in range(S):  # the chain: two values per segment
        a, b = (za[s] + p1 * a) + q1 * b, (zb[s] + p2 * a) + q2 * b
        e1[s + 1], e2[s + 1] = a, b
    y = (z + p[None, :] * e1[:S, None]) + q[None, :] * e2[:S, None]
    return y.reshape(-1)


class LoudnessMeter:
    """The streaming state of the loudness stage (section 27): feed() takes f32 samples in any chunk
    sizes and returns the energies of the sub-blocks they complete, bit for bit what the GPU stage
    reports for the same chunks, and what loudness_blocks gives for the whole signal."""

    def __init__(self):
        self.c = kweight_coeffs(24000.0)
        self.pq = loudness_tables(self.c)
        self.pend = np.zeros(0, np.float32)
        self.seen = 0
        self.f = [0.0] * 6  # x[-1], x[-2], shelf y[-1], y[-2], high-pass y[-1], y[-2]

    def feed(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        self.seen += x.size
        buf = np.concatenate([self.pend, x])
        nb = buf.size // LOUD_SUB
        self.pend = buf[nb * LOUD_SUB:]
        if nb == 0:
            return np.zeros(0, np.float64)
        w = buf[:nb * LOUD_SUB].astype(np.float64)
        f = self.f
        y1 = _loud_biquad(self.c[0], self.pq[0], w, (f[0], f[1]), (f[2], f[3]))
        y2 = _loud_biquad(self.c[1], self.pq[1], y1, (f[2], f[3]), (f[4], f[5]))
        self.f = [w[-1], w[-2], y1[-1], y1[-2], y2[-1], y2[-2]]
        sq = (y2 * y2).reshape(nb, LOUD_SUB // LOUD_G, LOUD_G)
        seg = np.zeros(sq.shape[:2], np.float64)
        for k in range(LOUD_G):  # a segment's 32 terms in ascending order
            seg = seg + sq[:, :, k]
        e = np.zeros(nb, np.float64)
        for s in range(seg.shape[1]):  # then the 75 segment sums in ascending order
            e = e + seg[:, s]
        return e


def loudness_blocks(x: np.ndarray, chunks=None):
    """The loudness stage's rule over a signal x (f32 at 24 kHz): the K-weighted energy sum of y^2 of
    each complete sub-block of 2,400 samples, float64 [len(x) // 2400]; samples behind the last
    complete sub-block are not measured. Every f64 operation is rounded once, in the order section
    27 states, so the GPU stage agrees bit for bit. chunks: the sizes in which the input arrives
    (they sum to len(x)): run as the stream does and return the list of per-chunk energy arrays,
    whose concatenation is the whole-signal result."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    m = LoudnessMeter()
    if chunks is None:
        return m.feed(x)
    sizes = [int(s) for s in chunks]
    if sum(sizes) != x.size or any(s < 0 for s in sizes):
        raise ValueError("chunks must be non-negative and sum to len(x)")
    out, n = [], 0
    for s in sizes:
        out.append(m.feed(x[n:n + s]))
        n += s
    return out


def loudness_integrated(energy) -> float | None:
    """Integrated loudness in LUFS (BS.1770 / EBU R128 gating) from sub-block energies: one array
    (one row), or a list of arrays (the rows of one response: each row's 400 ms gating blocks, four
    sub-blocks at 75 % overlap, are pooled and gated once). None: unmeasurable (no row with four
    sub-blocks, or the absolute gate at -70 keeps nothing)."""
    rows = [energy] if isinstance(energy, np.ndarray) or (len(energy) and np.isscalar(energy[0])) else list(energy)
    blocks = []
    for e in rows:
        e = np.asarray(e, np.float64).reshape(-1)
        if e.size >= 4:
            blocks.append((e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * LOUD_SUB))
    if not blocks:
        return None
    B = np.concatenate(blocks)
    B = B[B > 0.0]
    lk = lambda ms: -0.691 + 10.0 * np.log10(ms)  # noqa: E731
    B = B[lk(B) > -70.0]
    if B.size == 0:
        return None
    gate = lk(B.mean()) - 10.0
    B = B[lk(B) > gate]
    if B.size == 0:
        return None
    return float(lk(B.mean()))


def loudness_gain_cdb(target_lufs: float, voice_lufs: float) -> int:
    """The gain in hundredths of a dB that brings a voice calibrated at voice_lufs to target_lufs:
    round(100 (target - voice)), clamped to the level stage's [-2400, 2400]."""
    return int(max(-2400, min(2400, round(100.0 * (float(target_lufs) - float(voice_lufs))))))
