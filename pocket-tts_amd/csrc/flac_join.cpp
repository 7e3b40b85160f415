// Joining FLAC segments on the host (flac_join.h; the rule is DESIGN.md section 21.5).
#include "flac_join.h"

#include <cstring>

namespace ptts {
namespace {

// CRC-8 (0x07) and CRC-16 (0x8005) of section 21.1: initial value 0, not reflected
struct CrcTables {
  uint8_t c8[256];
  uint16_t c16[256];
  constexpr CrcTables() : c8(), c16() {
    for (int b = 0; b < 256; ++b) {
      unsigned a = (unsigned)b, c = (unsigned)b << 8;
      for (int i = 0; i < 8; ++i) {
        a = (a & 0x80u ? (a << 1) ^ 0x07u : a << 1) & 0xFFu;
        c = (c & 0x8000u ? (c << 1) ^ 0x8005u : c << 1) & 0xFFFFu;
      }
      c8[b] = (uint8_t)a;
      c16[b] = (uint16_t)c;
    }
  }
};
constexpr CrcTables CRC;

unsigned crc8(const uint8_t* p, int n) {
  unsigned c = 0;
  for (int i = 0; i < n; ++i) c = CRC.c8[c ^ p[i]];
  return c;
}
unsigned crc16(const uint8_t* p, long n) {
  unsigned c = 0;
  for (long i = 0; i < n; ++i) c = ((c << 8) & 0xFFFFu) ^ CRC.c16[(c >> 8) ^ p[i]];
  return c;
}
// a b mod x^16 + x^15 + x^2 + 1
unsigned mulmod(unsigned a, unsigned b) {
  unsigned r = 0;
  for (int i = 15; i >= 0; --i) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x18005u;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// c x^(8 m) mod the polynomial: what m more bytes behind a run do to its CRC (k_flac step 4)
unsigned shift_bytes(unsigned c, long m) {
  unsigned pw = 0x100u;
  for (; m > 0 && c; m >>= 1) {
    if (m & 1) c = mulmod(c, pw);
    pw = mulmod(pw, pw);
  }
  return c;
}

int number_bytes(long long v) {
  return v < (1LL << 7) ? 1 : v < (1LL << 11) ? 2 : v < (1LL << 16) ? 3 : v < (1LL << 21) ? 4
       : v < (1LL << 26) ? 5 : v < (1LL << 31) ? 6 : 7;
}
int put_number(long long v, uint8_t* o) {  // the UTF-8-like code extended to 36 bits; returns its bytes
  const int nb = number_bytes(v);
  if (nb == 1) {
    o[0] = (uint8_t)v;
    return 1;
  }
  o[0] = (uint8_t)(((0xFFu << (8 - nb)) & 0xFFu) | (unsigned)(nb == 7 ? 0 : v >> (6 * (nb - 1))));
  for (int i = nb - 2, at = 1; i >= 0; --i, ++at) o[at] = (uint8_t)(0x80u | (unsigned)((v >> (6 * i)) & 0x3F));
  return nb;
}
int rate_code(int rate) {
  return rate == 8000 ? 4 : rate == 16000 ? 5 : rate == 24000 ? 7 : rate == 44100 ? 9 : rate == 48000 ? 10 : -1;
}

struct Head {
  int nb;        // bytes of the coded number
  int len;       // bytes of the header, its CRC-8 included
  int block;     // the block size it states
  long long f;   // the coded number
};
// the header of section 21.1 at p (len bytes of frame); null, or what is wrong
const char* parse(const uint8_t* p, int len, Head* h) {
  if (len < 5) return "flac_rebase: a frame shorter than its header";
  if (p[0] != 0xFF || p[1] != 0xF9) return "flac_rebase: no frame sync (FF F9) at an index offset";
  const int bc = p[2] >> 4;
  if ((bc != 6 && bc != 7) || p[3] != 0x08) return "flac_rebase: not a frame header of section 21.1";
  const unsigned b0 = p[4];
  int nb = 0;
  while (nb < 8 && (b0 & (0x80u >> nb))) ++nb;  // leading one bits
  if (nb == 1 || nb == 8) return "flac_rebase: bad first byte of the coded number";
  if (nb == 0) nb = 1;
  const int hl = 4 + nb + (bc == 6 ? 1 : 2) + 1;
  if (len < hl + 1 + 2) return "flac_rebase: a frame shorter than its header";
  long long f = nb == 1 ? b0 : nb == 7 ? 0 : b0 & (0x7Fu >> nb);
  for (int i = 1; i < nb; ++i) {
    if ((p[4 + i] & 0xC0u) != 0x80u) return "flac_rebase: bad continuation byte in the coded number";
    f = f << 6 | (p[4 + i] & 0x3Fu);
  }
  h->nb = nb;
  h->len = hl;
  h->block = (bc == 6 ? p[4 + nb] : p[4 + nb] << 8 | p[5 + nb]) + 1;
  h->f = f;
  return nullptr;
}

}  // namespace

const char* flac_rebase(const uint8_t* in, int n_bytes, const int* index, int n_frames, long long delta, uint8_t* out,
                        int out_cap, int* out_bytes) {
  if (!in || !index || !out || !out_bytes || n_bytes < 0 || n_frames < 0) return "flac_rebase: null or negative argument";
  if (delta < 0) return "flac_rebase: delta must be >= 0";
  if (delta > FLAC_SAMPLES_END) return "flac_rebase: a sample number past 2^36";
  long long sum = 0;
  for (int i = 0; i < n_frames; ++i) {
    if (index[2 * i] < 1) return "flac_rebase: an index length below 1";
    sum += index[2 * i];
  }
  if (sum != n_bytes) return "flac_rebase: the index lengths do not sum to n_bytes";
  if ((long long)out_cap < (long long)n_bytes + (long long)FLAC_JOIN_GROW * n_frames)
    return "flac_rebase: out_cap must be >= n_bytes + 6 n_frames";
  // ---- every frame checked: nothing is written before the last one passes
  long at = 0;
  for (int i = 0; i < n_frames; ++i) {
    const uint8_t* p = in + at;
    const int len = index[2 * i];
    Head h;
    if (const char* err = parse(p, len, &h)) return err;
    if (crc8(p, h.len - 1) != p[h.len - 1]) return "flac_rebase: the header's CRC-8 does not verify";
    if (h.block != index[2 * i + 1]) return "flac_rebase: the header's block size differs from the index";
    if (crc16(p, len - 2) != (unsigned)(p[len - 2] << 8 | p[len - 1])) return "flac_rebase: the frame's CRC-16 does not verify";
    if (h.f + delta + h.block > FLAC_SAMPLES_END) return "flac_rebase: a sample number past 2^36";
    at += len;
  }
  // ---- the frames, renumbered. The CRC-16 is patched, not recomputed: with initial value 0,
  // CRC(header | body) = CRC(header) x^(8 body bytes) + CRC(body), so over the same body
  // CRC(new) = CRC(old) + (CRC(new header) + CRC(old header)) x^(8 body bytes)
  at = 0;
  long to = 0;
  for (int i = 0; i < n_frames; ++i) {
    const uint8_t* p = in + at;
    const int len = index[2 * i];
    Head h;
    (void)parse(p, len, &h);
    uint8_t* o = out + to;
    memcpy(o, p, 4);
    int hl = 4 + put_number(h.f + delta, o + 4);
    const int tail = h.len - 1 - 4 - h.nb;  // the block size bytes
    memcpy(o + hl, p + 4 + h.nb, tail);
    hl += tail;
    o[hl] = (uint8_t)crc8(o, hl);
    ++hl;
    const int body = len - h.len - 2;
    memcpy(o + hl, p + h.len, body);
    const unsigned crc = (unsigned)(p[len - 2] << 8 | p[len - 1]) ^ shift_bytes(crc16(o, hl) ^ crc16(p, h.len), body);
    o[hl + body] = (uint8_t)(crc >> 8);
    o[hl + body + 1] = (uint8_t)crc;
    at += len;
    to += hl + body + 2;
  }
  *out_bytes = (int)to;
  return nullptr;
}

const char* flac_silence(long long n, int rate, long long first_sample, uint8_t* out, long out_cap, long* out_bytes) {
  if (!out || !out_bytes || n < 0) return "flac_silence: null or negative argument";
  const int rc = rate_code(rate);
  if (rc < 0) return "flac_silence: sample_rate must be one of 8000, 16000, 24000, 44100, 48000";
  if (first_sample < 0 || n > FLAC_SAMPLES_END || first_sample > FLAC_SAMPLES_END - n)
    return "flac_silence: a sample number past 2^36";
  if (out_cap < flac_silence_bound(n)) return "flac_silence: out_cap must be >= ptts_flac_silence_bound(n)";
  long to = 0;
  for (long long off = 0; off < n; off += FLAC_JOIN_BLOCK) {
    const int bs = (int)(n - off < FLAC_JOIN_BLOCK ? n - off : FLAC_JOIN_BLOCK);
    uint8_t* o = out + to;
    int k = 0;
    o[k++] = 0xFF;
    o[k++] = 0xF9;
    o[k++] = (uint8_t)((bs <= 256 ? 6 : 7) << 4 | rc);
    o[k++] = 0x08;
    k += put_number(first_sample + off, o + k);
    if (bs > 256) o[k++] = (uint8_t)((bs - 1) >> 8);
    o[k++] = (uint8_t)(bs - 1);
    o[k] = (uint8_t)crc8(o, k);
    ++k;
    o[k++] = 0x00;  // CONSTANT
    o[k++] = 0x00;  // the sample, 16 bits
    o[k++] = 0x00;
    const unsigned crc = crc16(o, k);
    o[k++] = (uint8_t)(crc >> 8);
    o[k++] = (uint8_t)crc;
    to += k;
  }
  *out_bytes = to;
  return nullptr;
}

}  // namespace ptts
