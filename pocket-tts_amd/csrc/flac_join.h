// Joining FLAC segments on the host: the frames of a chunk renumbered by a
// sample offset, and pause silence as CONSTANT frames. Plain C++: needs neither engine nor GPU.
#pragma once
#include <cstdint>

namespace ptts {

constexpr int FLAC_JOIN_BLOCK = 4608;         // kernels.h FLAC_BLOCK (capi.cpp asserts both)
constexpr int FLAC_JOIN_GROW = 6;             // a frame's coded number is 1 .. 7 bytes
constexpr int FLAC_SILENCE_FRAME = 19;        // 14 header, 1 subframe header, 2 sample, 2 CRC-16
constexpr long long FLAC_SAMPLES_END = 1LL << 36;
constexpr long flac_silence_bound(long long n) {  // bytes of n samples of silence, at most (0: n < 1)
  return n < 1 ? 0 : (long)((n + FLAC_JOIN_BLOCK - 1) / FLAC_JOIN_BLOCK) * FLAC_SILENCE_FRAME;
}

// The n_frames frames at `in` (index [n_frames][2]: byte length, block size) with every coded sample
// number moved up by delta, in its shortest form, and both CRCs renewed; the body bits untouched.
// Every check is made before the first byte of `out` is written. Returns null, or what is wrong.
const char* flac_rebase(const uint8_t* in, int n_bytes, const int* index, int n_frames, long long delta, uint8_t* out,
                        int out_cap, int* out_bytes);

// n zero samples at `rate` as CONSTANT frames in blocks of FLAC_JOIN_BLOCK, the last one shorter,
// the first sample numbered first_sample. Returns null, or what is wrong (nothing written then).
const char* flac_silence(long long n, int rate, long long first_sample, uint8_t* out, long out_cap, long* out_bytes);

}  // namespace ptts
