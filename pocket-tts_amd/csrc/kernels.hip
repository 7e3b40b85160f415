// Device kernels of the Pocket TTS hot path, written for gfx950 (CDNA4, wave64).
//
// Reference semantics (ykevinc/pocket-tts, crates/pocket-tts/src):
//   GEMMs      <- candle Linear / Conv1d / ConvTranspose1d calls (transformer.rs:43-44,85;
//                 attention.rs:59-60,129,280; mlp.rs; conv.rs:90-136,219-267; seanet.rs)
//   attention  <- attention.rs:104-283 + sdpa.rs:36-280 (causal + context-window mask)
//   RoPE       <- rope.rs:18-60 (interleaved pairs)
//   flow head  <- mlp.rs:135-383, flow_lm.rs:7-22,98-164
//   Mimi front <- tts_model.rs:1033-1038, mimi.rs:8-37,143-157, conv.rs:315-346
#include "kernels.h"

#include <cmath>
#include <stdexcept>

#include "devfn.h"

namespace ptts {

// Measurement probes (PTTS_PROBES builds only, tools/): GemmArgs::probe bit 0 skips the MFMAs,
// bit 1 the operand loads of the tiled GEMMs (results wrong). A product build compiles them out.
#ifdef PTTS_PROBES
#define PTTS_PROBE(a) ((a).probe)
#else
#define PTTS_PROBE(a) 0
#endif

// Workgroups-per-CU cap of the launches issued while it is set (set_wg_cap; the engine sets it
// while capturing the back part of a pipelined step): dynamic LDS is reserved so that at most
// `cap` workgroups of a kernel share a CU, leaving room for the concurrently running front part.
// Per host thread: engines of one process (serve --gpus N threads) capture graphs concurrently.
static thread_local int g_wg_cap = 0;
void set_wg_cap(int cap) { g_wg_cap = cap; }
static thread_local int g_back_hi = 1;
void set_back_hi(int on) { g_back_hi = on; }
#ifdef PTTS_PROBES
__device__ int g_front_prio = 0;
void set_front_prio(int prio) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_front_prio), &prio, sizeof prio) != hipSuccess)
    throw std::runtime_error("set_front_prio failed");
}
__device__ int g_back_prio = 3;  // the product level (devfn.h back_prio)
__device__ int g_front_skip = 0;
void set_front_skip(int v) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_front_skip), &v, sizeof v) != hipSuccess)
    throw std::runtime_error("set_front_skip failed");
}
void set_back_prio(int prio) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_back_prio), &prio, sizeof prio) != hipSuccess)
    throw std::runtime_error("set_back_prio failed");
}
#else
void set_front_prio(int) {}  // product builds: no front priority
void set_back_prio(int) {}
void set_front_skip(int) {}
#endif
template <typename K>
static size_t cap_lds(K kernel, int cap) {
  if (cap <= 0) return 0;
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) != hipSuccess) return 0;
  const size_t need = 163840 / (cap + 1) + 16;  // cap + 1 workgroups no longer fit (160 KiB per CU)
  return need > fa.sharedSizeBytes ? need - fa.sharedSizeBytes : 0;
}


// Sum over S (<= 16) split-K slabs p[z * stride] in z order, every load issued before the first
// add (a runtime-bounded loop waited on each load in turn: one L2 round trip per slab).
__device__ __forceinline__ float slab_sum(const float* p, long stride, int S) {
  float v[16];
#pragma unroll
  for (int z = 0; z < 16; ++z) v[z] = z < S ? p[(long)z * stride] : 0.f;
  float acc = 0.f;
#pragma unroll
  for (int z = 0; z < 16; ++z)
    if (z < S) acc += v[z];
  return acc;
}

// =============================================================================================
// GEMM (see kernels.h). One 256-thread workgroup = 4 waves owns a 32x32 output tile; the
// tile's K chunks (32 wide) are dealt round-robin to the 4 waves, each wave accumulates with
// v_mfma_f32_32x32x2_f32 straight from registers (weights are read once per tile: the GEMV
// regime of the CDNA guide, no LDS staging), and the 4 partial tiles are summed through LDS.
//
// Fragment maps for v_mfma_f32_32x32x2_f32 (lane l, r = l & 31, h = l >> 5):
//   A[i = r][k = h], B[k = h][j = r], D reg g -> row (g&3) + 8*(g>>2) + 4*h, col r.
// Lane (r, h) loads 16 consecutive k of its A row and of its W row (k0 + 16h ... +15);
// MFMA #j of a chunk consumes element j of both, i.e. k-pair {k0 + j, k0 + 16 + j}.
// =============================================================================================
// Workgroup layouts (each wave accumulating one 32x32 tile; the TILE_GEMM rows of PTTS_TILES):
//   tile 0   "ksplit": WG tile 32x32, the tile's K chunks dealt round-robin to the 4 waves,
//            partial tiles summed through LDS (skinny M <= 32 GEMMs: more waves per tile)
//   tile 3   4x1 waves = WG tile 128x32 (each wave runs the whole K chain of its z-slice;
//            neighbours share W rows in L1/L2)
//   K-split variants of tile 0: 9 = 8 waves (2 per SIMD at one workgroup per CU),
//   10 = 4 waves with two chunks in flight, 17 = 8 waves, two chunks in flight.
// Epilogue of one output element v of GEMM row `row`, column `col` (S == 1 path): bias,
// activation, per-column scale, residual, ELU-out / dual store. Mode 1 maps row (b, q) to the
// output time row b*T_out + q*out_tstride + phase; `ident` (wave-uniform) marks the identity map
// (mode 0, or stride-1 single-phase convs) and skips the per-element division.
__device__ __forceinline__ void gemm_store(const GemmArgs& a, int row, int col, int phase, bool ident, float v) {
  if (a.bias) v += a.bias[col];
  if (a.act == ACT_GELU) v = gelu_tanh(v);
  else if (a.act == ACT_SILU) v = silu(v);
  long yrow = row;
  if (!ident) {
    const int b2 = row / a.Tq;
    const int q2 = row - b2 * a.Tq;
    yrow = (long)b2 * a.T_out + (long)q2 * a.out_tstride + phase;
  }
  if (a.rscale) v *= a.rscale[col];
  if (a.R) v += a.R[yrow * a.ldr + col];
  if (a.Y2) {
    a.Y[yrow * a.ldy + col] = v;
    a.Y2[yrow * a.ldy + col] = elu1(v);
  } else {
    a.Y[yrow * a.ldy + col] = a.elu_out ? elu1(v) : v;
  }
}
__device__ __forceinline__ bool gemm_ident(const GemmArgs& a, int mode, int phase) {
  return mode == 0 || (phase == 0 && a.out_tstride == 1 && a.T_out == a.Tq);
}

// Fast epilogue of NG accumulator values g = g0 .. g0+NG-1 of one in-bounds 32x32 tile
// (identity row map, no split-K; row of g = tm0 + (g&3) + 8(g>>2) + 4h, column tn0 + r). The
// column is fixed per lane, so bias / scale load once, row offsets are compile-time multiples of
// the leading dimensions, and the uniform options branch once per call instead of per element
// (the generic per-element path costs ~150 VALU per output, which dominated short-K tiles).
template <int NG>
__device__ __forceinline__ void gemm_store_fast(const GemmArgs& a, const float* acc, int g0, int tm0, int tn0, int h,
                                                int r) {
  const int col = tn0 + r;
  const long rb = (long)(tm0 + 4 * h);
  auto roff = [&](int k) { const int g = g0 + k; return (long)((g & 3) + 8 * (g >> 2)); };
  const float bcol = a.bias ? a.bias[col] : 0.f;
  float v[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) v[k] = acc[k] + bcol;
  if (a.act == ACT_GELU) {
#pragma unroll
    for (int k = 0; k < NG; ++k) v[k] = gelu_tanh(v[k]);
  } else if (a.act == ACT_SILU) {
#pragma unroll
    for (int k = 0; k < NG; ++k) v[k] = silu(v[k]);
  }
  if (a.rscale) {
    const float sc = a.rscale[col];
#pragma unroll
    for (int k = 0; k < NG; ++k) v[k] *= sc;
  }
  if (a.R) {
    const float* rp = a.R + rb * a.ldr + col;
    float rv[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) rv[k] = rp[roff(k) * a.ldr];
#pragma unroll
    for (int k = 0; k < NG; ++k) v[k] += rv[k];
  }
  float* yp = a.Y + rb * a.ldy + col;
  if (a.Y2) {
    float* y2 = a.Y2 + rb * a.ldy + col;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      yp[roff(k) * a.ldy] = v[k];
      y2[roff(k) * a.ldy] = elu1(v[k]);
    }
  } else if (a.elu_out) {
#pragma unroll
    for (int k = 0; k < NG; ++k) yp[roff(k) * a.ldy] = elu1(v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < NG; ++k) yp[roff(k) * a.ldy] = v[k];
  }
}
__device__ __forceinline__ void gemm_store_tile(const GemmArgs& a, const floatx16& acc, int tm0, int tn0, int h,
                                                int r) {
  float v[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) v[g] = acc[g];
  gemm_store_fast<16>(a, v, 0, tm0, tn0, h, r);
}

// XCD-aware tile order (speed only; any placement is correct). Workgroups are dealt round-robin
// to the 8 XCDs by linear id (MI355X_MICROARCH.md §Workgroup dispatch), so XCD x runs ids
// x, x + 8, ... Each XCD is given one block of the tile grid: the N tiles split into xcd_pn
// parts, the M tiles into 8 / xcd_pn, so an XCD reads 1/xcd_pn of the weights and
// xcd_pn/8 of the A rows, each once through its L2 (gemm() picks xcd_pn to minimise
// (8/pn) * |W| + pn * |A|: weight-heavy Mimi GEMMs and SEANet convs share weight tiles, the
// activation-heavy late SEANet stages share A row blocks). xcd_pn = 0, or a grid that does not
// split evenly: contiguous runs of T/8 tiles per XCD (x fastest); identity when T % 8 != 0 or
// when `on` is false.
__device__ __forceinline__ void xcd_tile(const GemmArgs& a, bool on, int& bx, int& by) {
  const int gx = gridDim.x, gy = gridDim.y, T = gx * gy;
  const int L = blockIdx.x + blockIdx.y * gx;
  const int pn = a.xcd_pn;
  if (on && (T & 7) == 0 && pn > 0) {
    const int pm = 8 / pn, xcd = L & 7, j = L >> 3, tnx = gx / pn;
    bx = (xcd % pn) * tnx + j % tnx;
    by = (xcd / pn) * (gy / pm) + j / tnx;
    return;
  }
  const int t = (on && (T & 7) == 0) ? (L & 7) * (T >> 3) + (L >> 3) : L;
  bx = t % gx;
  by = t / gx;
}

// LAYOUT: the id of a TILE_GEMM row of PTTS_TILES (kernels.h), which gives the waves per workgroup,
// WM x WN, the chunks in flight per wave (NBUF) and whether the waves split K
template <int MODE, int LAYOUT>
__global__ __launch_bounds__(tile_row(LAYOUT)->threads) void k_gemm(GemmArgs a) {
  if (a.front) front_prio();
  constexpr TileInfo T = *tile_row(LAYOUT);
  static_assert(T.family == TILE_GEMM, "k_gemm: not one of its tiles");
  constexpr bool KS = T.ksplit();
  constexpr int NW = T.threads / 64, PF = T.nbuf;
  __shared__ float red[KS ? NW * 16 * 64 : 1];
  const int lane = threadIdx.x & 63;
  // wave-uniform (SGPR) so that the chunk loop is a scalar loop: no exec-masked joins, and
  // the compiler can keep the next chunk's loads in flight across the MFMAs (counted vmcnt)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  constexpr int WM = T.wm, WN = T.wn;
  const int wm = KS ? 0 : wave / WN, wn = KS ? 0 : wave % WN;
  int bx, by;
  xcd_tile(a, true, bx, by);
  const int n0 = (bx * WN + wn) * 32, m0 = (by * WM + wm) * 32, z = blockIdx.z;
  const int nchunks = a.K >> 5;
  int cb = 0, ce = nchunks, phase = 0;
  if (MODE == 0) {
    cb = (int)((long)nchunks * z / a.S);
    ce = (int)((long)nchunks * (z + 1) / a.S);
  } else {
    phase = z;
  }
  // waves whose tile lies wholly outside W's padded rows or outside M have nothing to do
  // (wave-uniform; LAYOUT 0 never has such waves)
  const bool wave_live = n0 < a.Nw && m0 < a.M;
  const float* wrow = a.W + (long)phase * a.w_phase_stride + (long)(wave_live ? n0 + r : r) * a.K + 16 * h;
  const int m = m0 + r;
  const bool mvalid = m < a.M;
  const float* xrow = nullptr;
  const float *xb = nullptr, *hb = nullptr;  // conv: this row's batch base in X and in H (t = 0)
  int qs = 0;                                // conv: q * stride - P
  if (MODE == 0) {
    xrow = a.X + (long)(mvalid ? m : 0) * a.ldx + 16 * h;
  } else {
    const int mm = mvalid ? m : 0;
    const int bq = mm / a.Tq;
    qs = (mm - bq * a.Tq) * a.stride_in - a.P;
    xb = a.X + (long)bq * a.T_in * a.ldx + 16 * h;
    hb = a.H + ((long)bq * a.P + a.P) * a.cin + 16 * h;
  }

  // select, not branch: both candidate addresses are formed and one is picked per lane
  auto a_ptr = [&](int k0) -> const float* {
    if (MODE == 0) return xrow + k0;
    const int j = k0 / a.cin;  // wave-uniform (scalar)
    const int ci = k0 - j * a.cin;
    const int t = qs + j;
    const float* px = xb + t * a.ldx + ci;
    const float* ph = hb + t * a.cin + ci;
    return t >= 0 ? px : ph;
  };

  floatx16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;

  // Rows >= M were clamped to a valid row above: their garbage only reaches output rows that
  // are never stored, so the loads are unconditional (no exec-masked branches around them).
  (void)mvalid;
  constexpr bool elu = MODE == 2;  // compile-time: an if-converted ELU costs ~250 VALU per chunk
  auto load = [&](int cc, float4 (&A)[4], float4 (&Bv)[4]) {
    const float* ap = a_ptr(cc << 5);
    if (a.w_nt) {  // wave-uniform: the once-read weight stream with the non-temporal hint
      typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f4v w = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(wrow + (cc << 5) + 4 * i));
        Bv[i] = make_float4(w.x, w.y, w.z, w.w);
        A[i] = *reinterpret_cast<const float4*>(ap + 4 * i);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Bv[i] = *reinterpret_cast<const float4*>(wrow + (cc << 5) + 4 * i);
        A[i] = *reinterpret_cast<const float4*>(ap + 4 * i);
      }
    }
  };
  auto mma = [&](float4 (&A)[4], float4 (&Bv)[4]) {
    float af[16], bf[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[4 * i + 0] = A[i].x; af[4 * i + 1] = A[i].y; af[4 * i + 2] = A[i].z; af[4 * i + 3] = A[i].w;
      bf[4 * i + 0] = Bv[i].x; bf[4 * i + 1] = Bv[i].y; bf[4 * i + 2] = Bv[i].z; bf[4 * i + 3] = Bv[i].w;
    }
    if (elu) {
#pragma unroll
      for (int j = 0; j < 16; ++j) af[j] = elu1(af[j]);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
  };
  // rotating register sets: chunk c is multiplied while the next PF chunks are in flight
  float4 a0[4], b0[4], a1[4], b1[4];
  constexpr int CSTEP = KS ? NW : 1;
  int c = KS ? cb + wave : cb;
  if (!wave_live) c = ce;
  // The prefetch is unconditional (past the end it re-reads a valid chunk, never used), so no
  // control-flow join sits between a load and the MFMAs that must not wait for it.
  if (PF == 1) {
    // n chunks for this wave; loop body = two chunks with fixed register roles and no exits,
    // odd tail peeled (keeps the accumulator in place and the loads one chunk ahead)
    const int n = c < ce ? (ce - c + CSTEP - 1) / CSTEP : 0;
    const int clast = c + (n - 1) * CSTEP;
    auto chunk = [&](int i) { return i < n ? c + i * CSTEP : clast; };
    if (n > 0) {
      load(c, a0, b0);
      int i = 0;
      for (; i + 2 <= n; i += 2) {
        load(chunk(i + 1), a1, b1);
        mma(a0, b0);
        load(chunk(i + 2), a0, b0);
        mma(a1, b1);
      }
      if (i < n) mma(a0, b0);
    }
  } else {
    float4 a2[4], b2[4];
    if (c < ce) {
      load(c, a0, b0);
      load(c + CSTEP < ce ? c + CSTEP : c, a1, b1);
      for (;;) {  // invariant: a0 = chunk c, a1 = chunk c+CSTEP (if any), a2 free
        const int c1 = c + CSTEP, c2 = c + 2 * CSTEP, c3 = c + 3 * CSTEP, c4 = c + 4 * CSTEP;
        load(c2 < ce ? c2 : c, a2, b2);
        mma(a0, b0);
        if (c1 >= ce) break;
        load(c3 < ce ? c3 : c, a0, b0);
        mma(a1, b1);
        if (c2 >= ce) break;
        load(c4 < ce ? c4 : c, a1, b1);
        mma(a2, b2);
        if (c3 >= ce) break;
        c = c3;
      }
    }
  }

  const bool ident = gemm_ident(a, MODE, phase);
  auto store = [&](int g, float v) {
    const int row = m0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    const int col = n0 + r;
    if (row >= a.M || col >= a.N) return;
    if (a.partial) {
      a.partial[((long)z * a.M + row) * a.N + col] = v;
      return;
    }
    gemm_store(a, row, col, phase, ident, v);
  };
  if (KS) {
#pragma unroll
    for (int g = 0; g < 16; ++g) red[(wave * 16 + g) * 64 + lane] = acc[g];
    __syncthreads();
    constexpr int GPW = 16 / NW;  // output registers finished per wave
    float vs[GPW];
#pragma unroll
    for (int gg = 0; gg < GPW; ++gg) {
      const int g = wave * GPW + gg;
      float v = red[(0 * 16 + g) * 64 + lane];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += red[(w * 16 + g) * 64 + lane];
      vs[gg] = v;
    }
    if (ident && !a.partial && m0 + 32 <= a.M && n0 + 32 <= a.N) {
      gemm_store_fast<GPW>(a, vs, wave * GPW, m0, n0, h, r);
    } else {
#pragma unroll
      for (int gg = 0; gg < GPW; ++gg) store(wave * GPW + gg, vs[gg]);
    }
  } else if (wave_live) {
    if (ident && !a.partial && m0 + 32 <= a.M && n0 + 32 <= a.N) {
      gemm_store_tile(a, acc, m0, n0, h, r);
    } else {
#pragma unroll
      for (int g = 0; g < 16; ++g) store(g, acc[g]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA GEMM (the CDNA guide's 2-buffer global_load_lds structure): operand tiles go
// global -> LDS with global_load_lds_dwordx4 (one 1-KiB wave instruction = RPI rows of one
// BK-wide chunk; no VGPRs), two LDS buffers, one barrier per chunk: the DMA of chunk c+1 is in
// flight while chunk c is multiplied. LDS rows are unpadded and XOR-swizzled by 16-byte column
// (BK 32: col ^ ((row>>1)&7), BK 64: col ^ (row&15)) so the ds_read_b128 fragment reads are
// conflict-free; the swizzle is applied on the per-lane global SOURCE address (the DMA writes
// lane-linearly).  WG tile (32*WM) x (32*WN), 4 waves, each one 32x32 accumulator.
// Requires K % BK == 0 and, for convs, cin % BK == 0.
// ---------------------------------------------------------------------------------------------
template <int BK>
__device__ __forceinline__ int swz(int row) {
  return BK == 32 ? ((row >> 1) & 7) : (row & 15);
}

// One 16-byte-per-lane LDS-DMA (global_load_lds_dwordx4): lane l's 16 bytes land at
// lds_byte + 16*l. Issued through inline asm so hipcc neither counts it in vmcnt nor fences the
// ds_reads of the other buffer behind it (it cannot prove they do not alias); the caller drains
// it with an explicit `s_waitcnt vmcnt(0)` before the barrier that precedes reading it
// (cdna_hip_programming.md §5.7, M0 saved and restored inside the statement).
__device__ __forceinline__ void glds16(const float* gsrc, unsigned lds_byte) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_byte)
      : "memory");
}
// The same with the non-temporal hint (weights that one CU reads once per step: the decode's
// weight stream, MI355X_MICROARCH.md price row nt-weights).
__device__ __forceinline__ void glds16_nt(const float* gsrc, unsigned lds_byte) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_byte)
      : "memory");
}
// write-through (sc1) 16-byte store and L2-bypassing load: partial tiles handed between
// workgroups on different XCDs (each XCD has its own L2)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sc1_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
typedef unsigned int sc1_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void sc1_st(__amdgpu_buffer_rsrc_t r, int byte_off, float4 f) {
  const sc1_u32x4 v = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, byte_off, 0, 16);
}
__device__ __forceinline__ float4 sc1_ld(__amdgpu_buffer_rsrc_t r, int byte_off) {
  const sc1_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ unsigned lds_addr(const float* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) float*)(p);
}

// bf16x6 operand pieces (k_gemm_glds PREC 2). split3_frag: 8 f32 values -> their exact three-piece
// bf16 split by truncation (x0 = the upper 16 bits of x; r = x - x0 is exact (Sterbenz) with at
// most 16 significant bits; x1 = the upper 16 bits of r; x2 = r - x1 is exact with at most 8
// significant bits, so its lower 16 bits are zero): 4 VALU ops per value plus one v_perm_b32 per
// pair and piece. hm_frag: the hi and mid pieces of 8 pre-split W values (hm = hi << 16 | mid).
__device__ __forceinline__ void split3_frag(const float* x, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
  u32x4 h, m, l;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned u0 = __float_as_uint(x[2 * p]), u1 = __float_as_uint(x[2 * p + 1]);
    const float r0 = x[2 * p] - __uint_as_float(u0 & 0xffff0000u), r1 = x[2 * p + 1] - __uint_as_float(u1 & 0xffff0000u);
    const unsigned v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    h[p] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    m[p] = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    l[p] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
  }
  p0 = __builtin_bit_cast(bf16x8, h);
  p1 = __builtin_bit_cast(bf16x8, m);
  p2 = __builtin_bit_cast(bf16x8, l);
}
__device__ __forceinline__ void hm_frag(const float* w, bf16x8& p0, bf16x8& p1) {
  u32x4 h, m;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned e0 = __float_as_uint(w[2 * p]), e1 = __float_as_uint(w[2 * p + 1]);
    h[p] = __builtin_amdgcn_perm(e1, e0, 0x07060302u);
    m[p] = __builtin_amdgcn_perm(e1, e0, 0x05040100u);
  }
  p0 = __builtin_bit_cast(bf16x8, h);
  p1 = __builtin_bit_cast(bf16x8, m);
}

// s_waitcnt with only vmcnt = n (expcnt/lgkmcnt left at "no wait"), gfx9 simm16 encoding
#define PTTS_WAIT_VM(n) __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | (7 << 4) | (15 << 8))

// TMW x TNW: 32x32 accumulators per wave (register blocking: one A fragment feeds TNW MFMAs,
// one B fragment TMW), WG tile (32*WM*TMW) x (32*WN*TNW).
// MODE 1 with S > 1 (single-phase convs): z is a K slice and the tile goes to partial slab z.
// MINB: workgroups per CU the register allocation must allow (__launch_bounds__ min waves per
// SIMD = MINB). ILV: the DMAs of chunk c + NBUF - 1 are issued between the MFMAs of chunk c (one
// per 16 / IPW k-steps) instead of as a burst ahead of its fragment reads: an f32 MFMA leaves 56
// of its 64 issue cycles free, so the DMA issue (60-185 cycles each) hides behind the matrix pipe.
// PREC 1, bf16 (engine back_mfma = PTTS_BACK_BF16, a variant beside the f32 path): the same tiles,
// operands still f32 in HBM and LDS, rounded to bf16 (v_cvt_pk_bf16_f32, RNE) as the fragments are
// read, and multiplied on v_mfma_f32_32x32x16_bf16 with f32 accumulation: lane half h feeds
// elements j of MFMA q from its chunk columns 16h + 8q + j for A and B alike, so each chunk's 32 k
// are summed once (2 MFMAs per 32-k chunk instead of 16). The next chunk's DMAs are issued after
// the two MFMAs.
// PREC 2, bf16x6 (PTTS_BACK_F32X6): f32 products on the bf16 matrix pipe. Every f32 operand is the
// exact sum of three bf16 pieces, x = x0 + x1 + x2 (split3: |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|),
// and the tile sums the six products whose order is <= 2, a0 b0 + a0 b1 + a1 b0 + a0 b2 + a1 b1 +
// a2 b0: each piece product is exact, the dropped three are below 2^-24 |a b| together, so the
// result has f32 accuracy (test_gpu_gemm_core: error against fp64 no larger than the f32 MFMA
// tile's) at 6 bf16 MFMAs (32 cycles each) per 16 k instead of 8 f32 ones (64 cycles each). W
// comes pre-split from finalize (GemmArgs::Whm = hi | mid in W's f32 layout, Wlo = lo: one more
// 64-B LDS row per W row and chunk, its 16-B columns swizzled by (row >> 2) & 3 so the ds_read_b128
// of a 16-lane group hit distinct banks); A is split as its fragments are read (truncation:
// x0 = x & 0xffff0000, x1 = trunc(x - x0), x2 = x - x0 - x1, all exact).
template <int MODE, int WM, int WN, int BK, int NBUF, int TMW = 1, int TNW = 1, int MINB = 1, bool ILV = false,
          int PREC = 0>
__global__ __launch_bounds__(256, MINB) void k_gemm_glds(GemmArgs a) {
  if (a.front) front_prio();
  else if (a.back_hi) back_prio();
  constexpr bool BF16 = PREC == 1, X6 = PREC == 2;
  constexpr int TM = 32 * WM * TMW, TN = 32 * WN * TNW, ROWS = TM + TN;
  constexpr int CPR = BK / 4;        // 16-byte columns per LDS row
  constexpr int RPI = 64 / CPR;      // rows per 1-KiB wave instruction
  constexpr int NMAIN = ROWS / RPI;  // DMA instructions per chunk for the A and W rows
  constexpr int NLO = X6 ? TN / 16 : 0;  // ... for the W lo rows (64 B each: 16 per instruction)
  constexpr int NINS = NMAIN + NLO;  // DMA instructions per chunk (whole workgroup)
  static_assert(NINS % 4 == 0, "every wave issues the same number of DMAs per chunk");
  static_assert(!X6 || BK == 32, "bf16x6 tiles: BK 32");
  constexpr int IPW = NINS / 4;
  constexpr int DIST = NBUF - 1;     // chunks in flight ahead of the one being multiplied
  static_assert(NBUF >= 2 && NBUF <= 4, "counted waits below cover up to 3 chunks in flight");
  constexpr int BUF = ROWS * BK + (X6 ? TN * 16 : 0);  // floats per LDS buffer (A | W | W lo)
  __shared__ __attribute__((aligned(16))) float lds[NBUF * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, h = lane >> 5;
  int bx, by;
  int tail_u = -1;  // split tail: this workgroup's (tile, slice) unit among the remainder tiles
  if (ILV && MODE == 0 && a.tail_S > 0) {
    // 1-D grid: whole tiles first (contiguous runs of them per XCD), then tail_S units per
    // remainder tile
    const int L = blockIdx.x, F = a.tail_full;
    int t;
    if (L < F) {
      t = (F & 7) == 0 ? (L & 7) * (F >> 3) + (L >> 3) : L;
    } else {
      tail_u = L - F;
      t = F + tail_u / a.tail_S;
    }
    bx = t % a.tiles_n;
    by = t / a.tiles_n;
  } else {
    xcd_tile(a, true, bx, by);
  }
  const int n0 = bx * TN, m0 = by * TM, z = blockIdx.z;
  const int nchunks = a.K / BK;
  int cb = 0, ce = nchunks, phase = 0;
  if (MODE == 0 || a.S > 1) {
    cb = (int)((long)nchunks * z / a.S);
    ce = (int)((long)nchunks * (z + 1) / a.S);
  } else {
    phase = z;
  }
  if (tail_u >= 0) {
    const int zt = tail_u % a.tail_S;
    cb = (int)((long)nchunks * zt / a.tail_S);
    ce = (int)((long)nchunks * (zt + 1) / a.tail_S);
  }
  const float* Wp = (X6 ? reinterpret_cast<const float*>(a.Whm) : a.W) + (long)phase * a.w_phase_stride;
  const unsigned lds_base = lds_addr(lds);
  // this lane's DMA sources: instruction j = wave + 4*ins covers rows j*RPI .. +RPI-1, all of
  // them A rows or all of them W rows (TM % RPI == 0), so the A/W choice is wave-uniform.
  // Conv A rows keep two base pointers (activation X and history H, both at time index 0 and
  // this lane's column); a chunk picks one per lane with a select, never a branch.
  // bf16x6: instructions j >= NMAIN move W lo rows (16 per instruction, 4 lanes of 16 B each).
  const float* src_base[IPW];
  const float* src_hist[IPW];
  int src_qs[IPW];
#pragma unroll
  for (int ins = 0; ins < IPW; ++ins) {
    const int j = wave + 4 * ins;
    if (X6 && j >= NMAIN) {
      const int lrow = (j - NMAIN) * 16 + lane / 4;
      const int lcol = (lane % 4) ^ ((lrow >> 2) & 3);
      const int n = min(n0 + lrow, a.Nw - 1);
      src_base[ins] = reinterpret_cast<const float*>(a.Wlo + (long)phase * a.w_phase_stride + (long)n * a.K + 8 * lcol);
      continue;
    }
    const int row = (j < NINS ? j : 0) * RPI + lane / CPR;
    const int lcol = (lane % CPR) ^ swz<BK>(row);
    if ((j < NINS ? j : 0) * RPI < TM) {
      const int m = min(m0 + row, a.M - 1);  // rows >= M only feed output rows that are never stored
      if (MODE == 0) {
        src_base[ins] = a.X + (long)m * a.ldx + 4 * lcol;
      } else {
        const int bq = m / a.Tq;
        const int qq = m - bq * a.Tq;
        src_qs[ins] = qq * a.stride_in - a.P;
        src_base[ins] = a.X + (long)bq * a.T_in * a.ldx + 4 * lcol;
        src_hist[ins] = a.H + ((long)bq * a.P + a.P) * a.cin + 4 * lcol;
      }
    } else {
      const int n = min(n0 + row - TM, a.Nw - 1);
      src_base[ins] = Wp + (long)n * a.K + 4 * lcol;
    }
  }
  const long ldx = a.ldx, hld = a.cin;
  // source of this lane's 16 bytes for DMA instruction `ins` of this wave and chunk c
  auto dma_src = [&](int c, int ins) -> const float* {
    const int j = wave + 4 * ins;
    const int k0 = c * BK;
    if (X6 && j >= NMAIN)  // W lo row: bf16 elements
      return reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(src_base[ins]) + k0);
    if (MODE != 0 && j * RPI < TM) {
      const int tap = k0 / a.cin;  // scalar
      const int ci = k0 - tap * a.cin;
      const int t = src_qs[ins] + tap;
      const float* px = src_base[ins] + t * ldx + ci;
      const float* ph = src_hist[ins] + t * hld + ci;
      return t >= 0 ? px : ph;
    }
    return src_base[ins] + k0;
  };
  // DMA instruction `ins` of this wave from src into LDS buffer buf
  auto dma = [&](const float* src, int buf, int ins) {
    if (PTTS_PROBE(a) & 2) return;
    const int j = wave + 4 * ins;
    if (j >= NINS) return;  // wave-uniform
    // wave-uniform LDS base of this instruction; lane l -> + 16*l bytes
    const int off = X6 && j >= NMAIN ? buf * BUF + ROWS * BK + (j - NMAIN) * 256 : buf * BUF + j * RPI * BK;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(off * 4));
    if (a.w_nt && j * RPI >= TM) glds16_nt(src, dst);  // wave-uniform: a W row instruction
    else glds16(src, dst);
  };
  auto issue = [&](int c, int buf) {
#pragma unroll
    for (int ins = 0; ins < IPW; ++ins) dma(dma_src(c, ins), buf, ins);
  };
  static_assert(!ILV || (BK == 32 && IPW <= 16), "interleaved DMA issue: BK 32, at most one DMA per k-step");
  constexpr bool elu = MODE == 2;  // compile-time: an if-converted ELU costs ~250 VALU per chunk
  floatx16 acc[TMW][TNW];
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < TNW; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
  const int arow = 32 * TMW * wm + r, brow = TM + 32 * TNW * wn + r;
  for (int d = 0; d < DIST; ++d)
    if (cb + d < ce) issue(cb + d, d);
  for (int c = cb; c < ce; ++c) {
    {  // chunk c landed for this wave once only the younger chunks' DMAs remain outstanding
      const int younger = min(DIST - 1, ce - 1 - c);
      if (younger >= 2) PTTS_WAIT_VM(2 * IPW);
      else if (younger == 1) PTTS_WAIT_VM(IPW);
      else PTTS_WAIT_VM(0);
    }
    // every wave's DMAs of chunk c have landed, and every wave is done with chunk c-1's buffer,
    // which the DMA issued next (chunk c+DIST) overwrites
    __syncthreads();
    const bool pf = c + DIST < ce;
    const int pc = c + DIST, pbuf = (c + DIST - cb) % NBUF;
    if (!ILV && pf) issue(pc, pbuf);
    // ILV: the next chunk's DMA sources are formed here, ahead of this chunk's fragment reads, and
    // pinned (an empty asm that rewrites them), so no address arithmetic lands between the MFMAs:
    // with it there, the compiler reused the registers of queued MFMAs' operands for the address
    // (v_lshl_add_u64 right behind the MFMA that reads it) and tiles came out wrong
    const float* nsrc[IPW];
    if (ILV) {
#pragma unroll
      for (int ins = 0; ins < IPW; ++ins) {
        nsrc[ins] = dma_src(pf ? pc : c, ins);
        asm volatile("" : "+v"(nsrc[ins]));
      }
    }
    {
      const int buf = (c - cb) % NBUF;
#pragma unroll
      for (int half = 0; half < BK / 32; ++half) {
        float af[TMW][16], bf[TNW][16];
#pragma unroll
        for (int ii = 0; ii < TMW; ++ii) {
          const int row = arow + 32 * ii;
          const float* la = lds + buf * BUF + row * BK;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int lc = 8 * half + 4 * h + i;
            const float4 x = *reinterpret_cast<const float4*>(la + 4 * (lc ^ swz<BK>(row)));
            af[ii][4 * i + 0] = x.x; af[ii][4 * i + 1] = x.y; af[ii][4 * i + 2] = x.z; af[ii][4 * i + 3] = x.w;
          }
          if (elu) {
#pragma unroll
            for (int j = 0; j < 16; ++j) af[ii][j] = elu1(af[ii][j]);
          }
        }
#pragma unroll
        for (int jj = 0; jj < TNW; ++jj) {
          const int row = brow + 32 * jj;
          const float* lb = lds + buf * BUF + row * BK;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int lc = 8 * half + 4 * h + i;
            const float4 y = *reinterpret_cast<const float4*>(lb + 4 * (lc ^ swz<BK>(row)));
            bf[jj][4 * i + 0] = y.x; bf[jj][4 * i + 1] = y.y; bf[jj][4 * i + 2] = y.z; bf[jj][4 * i + 3] = y.w;
          }
        }
        if (BF16) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            bf16x8 ab[TMW], bb[TNW];
#pragma unroll
            for (int ii = 0; ii < TMW; ++ii) {
              floatx8 v;
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = af[ii][8 * q + j];
              ab[ii] = __builtin_convertvector(v, bf16x8);
            }
#pragma unroll
            for (int jj = 0; jj < TNW; ++jj) {
              floatx8 v;
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = bf[jj][8 * q + j];
              bb[jj] = __builtin_convertvector(v, bf16x8);
            }
#pragma unroll
            for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
              for (int jj = 0; jj < TNW; ++jj)
                acc[ii][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[ii], bb[jj], acc[ii][jj], 0, 0, 0);
          }
          if (ILV && pf) {
#pragma unroll
            for (int ins = 0; ins < IPW; ++ins) dma(nsrc[ins], pbuf, ins);
          }
        } else if (X6) {
          const float* llo = lds + buf * BUF + ROWS * BK;  // W lo rows, 16 floats (32 bf16) each
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            bf16x8 a0[TMW], a1[TMW], a2[TMW], b0[TNW], b1[TNW], b2[TNW];
#pragma unroll
            for (int ii = 0; ii < TMW; ++ii) split3_frag(&af[ii][8 * q], a0[ii], a1[ii], a2[ii]);
#pragma unroll
            for (int jj = 0; jj < TNW; ++jj) {
              hm_frag(&bf[jj][8 * q], b0[jj], b1[jj]);
              const int lrow = brow - TM + 32 * jj;
              const int lc = (2 * h + q) ^ ((lrow >> 2) & 3);
              b2[jj] = *reinterpret_cast<const bf16x8*>(llo + lrow * 16 + 4 * lc);
            }
#pragma unroll
            for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
              for (int jj = 0; jj < TNW; ++jj) {
                floatx16 t = acc[ii][jj];
                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[ii], b0[jj], t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[ii], b1[jj], t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ii], b2[jj], t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[ii], b0[jj], t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ii], b1[jj], t, 0, 0, 0);
                acc[ii][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[ii], b0[jj], t, 0, 0, 0);
              }
            if (ILV && pf && q == 0) {  // the next chunk's DMAs between the two halves
#pragma unroll
              for (int ins = 0; ins < IPW; ++ins) dma(nsrc[ins], pbuf, ins);
            }
          }
        } else if (!(PTTS_PROBE(a) & 1)) {
#pragma unroll
          for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
              for (int jj = 0; jj < TNW; ++jj)
                acc[ii][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ii][j], bf[jj][j], acc[ii][jj], 0, 0, 0);
            if (ILV && pf && ((j + 1) * IPW) / 16 != (j * IPW) / 16) dma(nsrc[(j * IPW) / 16], pbuf, (j * IPW) / 16);
          }
        } else if (ILV && pf) {
          issue(pc, pbuf);
        }
      }
    }
  }
  if (ILV && MODE == 0 && tail_u >= 0) {
    // split tail: publish this slice's partial tile (register order, 1 KB per float4 row of the
    // wave), count in; the last of the tile's tail_S slices sums them in slice order
    const int ti = tail_u / a.tail_S, zt = tail_u % a.tail_S;
    const auto rs = sc1_rsrc(a.tail_slab + (long)ti * a.tail_S * TM * TN);
    auto off = [&](int zz, int ii, int jj, int q) {
      return (((zz * 4 + wave) * TMW * TNW + ii * TNW + jj) * 4 + q) * 1024 + 16 * lane;
    };
#pragma unroll
    for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
      for (int jj = 0; jj < TNW; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          sc1_st(rs, off(zt, ii, jj, q),
                 make_float4(acc[ii][jj][4 * q], acc[ii][jj][4 * q + 1], acc[ii][jj][4 * q + 2], acc[ii][jj][4 * q + 3]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int last;
    if (tid == 0)
      last = __hip_atomic_fetch_add(a.tickets + ti, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.tail_S - 1;
    __syncthreads();
    if (!last) return;
    if (tid == 0) __hip_atomic_store(a.tickets + ti, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // keeps the slab loads below the ticket
    // slice order: t = P0 + P1 + ... ; one slice's 4 * TMW * TNW loads in flight at a time
    float4 t[TMW][TNW][4];
#pragma unroll
    for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
      for (int jj = 0; jj < TNW; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          t[ii][jj][q] = zt == 0 ? make_float4(acc[ii][jj][4 * q], acc[ii][jj][4 * q + 1], acc[ii][jj][4 * q + 2],
                                               acc[ii][jj][4 * q + 3])
                                 : sc1_ld(rs, off(0, ii, jj, q));
#pragma unroll 1
    for (int zz = 1; zz < a.tail_S; ++zz) {
      float4 v[TMW][TNW][4];
#pragma unroll
      for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
        for (int jj = 0; jj < TNW; ++jj)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            v[ii][jj][q] = zz == zt ? make_float4(acc[ii][jj][4 * q], acc[ii][jj][4 * q + 1], acc[ii][jj][4 * q + 2],
                                                  acc[ii][jj][4 * q + 3])
                                    : sc1_ld(rs, off(zz, ii, jj, q));
#pragma unroll
      for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
        for (int jj = 0; jj < TNW; ++jj)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            t[ii][jj][q].x += v[ii][jj][q].x;
            t[ii][jj][q].y += v[ii][jj][q].y;
            t[ii][jj][q].z += v[ii][jj][q].z;
            t[ii][jj][q].w += v[ii][jj][q].w;
          }
    }
#pragma unroll
    for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
      for (int jj = 0; jj < TNW; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[ii][jj][4 * q] = t[ii][jj][q].x;
          acc[ii][jj][4 * q + 1] = t[ii][jj][q].y;
          acc[ii][jj][4 * q + 2] = t[ii][jj][q].z;
          acc[ii][jj][4 * q + 3] = t[ii][jj][q].w;
        }
  }
  const bool ident = gemm_ident(a, MODE, phase);
#pragma unroll
  for (int ii = 0; ii < TMW; ++ii)
#pragma unroll
    for (int jj = 0; jj < TNW; ++jj) {
      const int tm0 = m0 + 32 * TMW * wm + 32 * ii, tn0 = n0 + 32 * TNW * wn + 32 * jj;
      if (ident && !a.partial && tm0 + 32 <= a.M && tn0 + 32 <= a.N) {
        gemm_store_tile(a, acc[ii][jj], tm0, tn0, h, r);
      } else {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = tm0 + (g & 3) + 8 * (g >> 2) + 4 * h;
          const int col = tn0 + r;
          if (row < a.M && col < a.N) {
            const float v = acc[ii][jj][g];
            if (a.partial) a.partial[((long)z * a.M + row) * a.N + col] = v;
            else gemm_store(a, row, col, phase, ident, v);
          }
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------
// Register-blocked K-split GEMM: each wave accumulates a (32*TM) x (32*TN) block (TM*TN
// 32x32 accumulators); one A fragment feeds TN MFMAs and one B fragment TM, so operand bytes per
// flop fall to (TM+TN)/(2*TM*TN) of the 32x32 tile's. The 4 waves split the K chunks of the
// workgroup tile and are summed through LDS; loads run one chunk ahead in an exit-free loop.
// LAYOUT 18: 32x64 per workgroup (TM 1, TN 2), 19: 64x32 (2, 1), 20: 64x64 (2, 2).
// ---------------------------------------------------------------------------------------------
template <int MODE, int TM, int TN>
__global__ __launch_bounds__(256) void k_gemm_rb(GemmArgs a) {
  if (a.back_hi) back_prio();
  __shared__ float red[4 * 16 * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  int bx, by;
  xcd_tile(a, true, bx, by);
  const int n0 = bx * 32 * TN, m0 = by * 32 * TM, z = blockIdx.z;
  const int nchunks = a.K >> 5;
  int cb = 0, ce = nchunks, phase = 0;
  if (MODE == 0) {
    cb = (int)((long)nchunks * z / a.S);
    ce = (int)((long)nchunks * (z + 1) / a.S);
  } else {
    phase = z;
  }
  const float* wrow[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = min(n0 + 32 * j + r, a.Nw - 1);
    wrow[j] = a.W + (long)phase * a.w_phase_stride + (long)n * a.K + 16 * h;
  }
  const float* xrow[TM];
  const float *xb[TM], *hb[TM];
  int qs[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int mm = min(m0 + 32 * i + r, a.M - 1);  // rows past M only feed unstored outputs
    if (MODE == 0) {
      xrow[i] = a.X + (long)mm * a.ldx + 16 * h;
    } else {
      const int bq = mm / a.Tq;
      qs[i] = (mm - bq * a.Tq) * a.stride_in - a.P;
      xb[i] = a.X + (long)bq * a.T_in * a.ldx + 16 * h;
      hb[i] = a.H + ((long)bq * a.P + a.P) * a.cin + 16 * h;
    }
  }
  auto a_ptr = [&](int i, int k0) -> const float* {
    if (MODE == 0) return xrow[i] + k0;
    const int j = k0 / a.cin;
    const int ci = k0 - j * a.cin;
    const int t = qs[i] + j;
    const float* px = xb[i] + t * a.ldx + ci;
    const float* ph = hb[i] + t * a.cin + ci;
    return t >= 0 ? px : ph;
  };
  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
  constexpr bool elu = MODE == 2;  // compile-time: an if-converted ELU costs ~250 VALU per chunk
  auto load = [&](int cc, float4 (&A)[TM][4], float4 (&Bv)[TN][4]) {
    if (PTTS_PROBE(a) & 2) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) A[i][q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) Bv[j][q] = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float* ap = a_ptr(i, cc << 5);
#pragma unroll
      for (int q = 0; q < 4; ++q) A[i][q] = *reinterpret_cast<const float4*>(ap + 4 * q);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) Bv[j][q] = *reinterpret_cast<const float4*>(wrow[j] + (cc << 5) + 4 * q);
  };
  auto mma = [&](float4 (&A)[TM][4], float4 (&Bv)[TN][4]) {
    float af[TM][16], bf[TN][16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        af[i][4 * q] = A[i][q].x; af[i][4 * q + 1] = A[i][q].y; af[i][4 * q + 2] = A[i][q].z; af[i][4 * q + 3] = A[i][q].w;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bf[j][4 * q] = Bv[j][q].x; bf[j][4 * q + 1] = Bv[j][q].y; bf[j][4 * q + 2] = Bv[j][q].z; bf[j][4 * q + 3] = Bv[j][q].w;
      }
    }
    if (elu) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) af[i][k] = elu1(af[i][k]);
    }
    if (PTTS_PROBE(a) & 1) return;
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][k], bf[j][k], acc[i][j], 0, 0, 0);
  };
  float4 a0[TM][4], b0[TN][4], a1[TM][4], b1[TN][4];
  {
    const int c = cb + wave;
    const int n = c < ce ? (ce - c + 3) / 4 : 0;
    const int clast = c + (n - 1) * 4;
    auto chunk = [&](int i) { return i < n ? c + i * 4 : clast; };
    if (n > 0) {
      load(c, a0, b0);
      int i = 0;
      for (; i + 2 <= n; i += 2) {
        load(chunk(i + 1), a1, b1);
        mma(a0, b0);
        load(chunk(i + 2), a0, b0);
        mma(a1, b1);
      }
      if (i < n) mma(a0, b0);
    }
  }
  // K-split sum over the 4 waves, one 32x32 accumulator at a time through LDS
  const bool ident = gemm_ident(a, MODE, phase);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if (i + j > 0) __syncthreads();
#pragma unroll
      for (int g = 0; g < 16; ++g) red[(wave * 16 + g) * 64 + lane] = acc[i][j][g];
      __syncthreads();
      float vs[4];
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int g = wave * 4 + gg;
        float v = red[(0 * 16 + g) * 64 + lane] + red[(1 * 16 + g) * 64 + lane];
        v += red[(2 * 16 + g) * 64 + lane];
        v += red[(3 * 16 + g) * 64 + lane];
        vs[gg] = v;
      }
      if (ident && !a.partial && m0 + 32 * i + 32 <= a.M && n0 + 32 * j + 32 <= a.N) {
        gemm_store_fast<4>(a, vs, wave * 4, m0 + 32 * i, n0 + 32 * j, h, r);
        continue;
      }
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int g = wave * 4 + gg;
        const int row = m0 + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h;
        const int col = n0 + 32 * j + r;
        if (row >= a.M || col >= a.N) continue;
        if (a.partial) {
          a.partial[((long)z * a.M + row) * a.N + col] = vs[gg];
          continue;
        }
        gemm_store(a, row, col, phase, ident, vs[gg]);
      }
    }
}

// ---------------------------------------------------------------------------------------------
// int8-weight split-K GEMM for the FlowLM step under weight_quant. The weights hold the
// reference's simulated quantization (QuantizedTensor::quantize, quantize.rs:66-90: data =
// clamp(round(x/scale)) * scale, in f32), so the f32 weight is rebuilt per element as
// float(q) * scale[n] - bit-for-bit the value the reference multiplies with - and only the
// int8 code is streamed from HBM: 4x fewer weight bytes on the weight-bound skinny GEMMs.
// Structure of LAYOUT 0: 4 waves on one 32 x (32*TN) tile, the tile's K chunks dealt
// round-robin to the waves (one chunk in flight ahead of the MFMAs), partial tiles summed
// through LDS into split-K slab z. Lane (r, h) reads the 16 codes k0+16h..+15 of row
// n0+32t+r with one 16-byte load; each A fragment feeds TN MFMAs.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float i8_to_f(unsigned d, int b) { return (float)((int)(d << (24 - 8 * b)) >> 24); }

template <int TN>
__global__ __launch_bounds__(256) void k_gemm_w8(GemmArgs a) {
  __shared__ float red[4 * 16 * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32 * TN, m0 = blockIdx.y * 32, z = blockIdx.z;
  const int nchunks = a.K >> 5;
  const int cb = (int)((long)nchunks * z / a.S), ce = (int)((long)nchunks * (z + 1) / a.S);
  // rows past M / N are clamped to valid ones: their results are never stored
  const float* xrow = a.X + (long)min(m0 + r, a.M - 1) * a.ldx + 16 * h;
  const int8_t* wrow[TN];
  float sc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int n = min(n0 + 32 * t + r, a.N - 1);
    wrow[t] = a.Wq + (long)n * a.K + 16 * h;
    sc[t] = a.wscale[n];
  }
  floatx16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;

  auto load = [&](int cc, float4 (&A)[4], uint4 (&Q)[TN]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) A[i] = *reinterpret_cast<const float4*>(xrow + (cc << 5) + 4 * i);
#pragma unroll
    for (int t = 0; t < TN; ++t) Q[t] = *reinterpret_cast<const uint4*>(wrow[t] + (cc << 5));
  };
  auto mma = [&](float4 (&A)[4], uint4 (&Q)[TN]) {
    float af[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[4 * i + 0] = A[i].x; af[4 * i + 1] = A[i].y; af[4 * i + 2] = A[i].z; af[4 * i + 3] = A[i].w;
    }
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const unsigned d[4] = {Q[t].x, Q[t].y, Q[t].z, Q[t].w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float w = i8_to_f(d[j >> 2], j & 3) * sc[t];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], w, acc[t], 0, 0, 0);
      }
    }
  };
  float4 a0[4], a1[4];
  uint4 q0[TN], q1[TN];
  const int c = cb + wave;
  const int n = c < ce ? (ce - c + 3) / 4 : 0;
  const int clast = c + (n - 1) * 4;
  auto chunk = [&](int i) { return i < n ? c + i * 4 : clast; };
  if (n > 0) {
    load(c, a0, q0);
    int i = 0;
    for (; i + 2 <= n; i += 2) {
      load(chunk(i + 1), a1, q1);
      mma(a0, q0);
      load(chunk(i + 2), a0, q0);
      mma(a1, q1);
    }
    if (i < n) mma(a0, q0);
  }
#pragma unroll
  for (int t = 0; t < TN; ++t) {
#pragma unroll
    for (int g = 0; g < 16; ++g) red[(wave * 16 + g) * 64 + lane] = acc[t][g];
    __syncthreads();
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      const int g = wave * 4 + gg;
      const float v = red[g * 64 + lane] + red[(16 + g) * 64 + lane] + red[(32 + g) * 64 + lane] +
                      red[(48 + g) * 64 + lane];
      const int row = m0 + (g & 3) + 8 * (g >> 2) + 4 * h;
      const int col = n0 + 32 * t + r;
      if (row < a.M && col < a.N) a.partial[((long)z * a.M + row) * a.N + col] = v;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_quant_codes(const float* W, const float* s, int N, int K, int8_t* q,
                                                     int* bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * K) return;
  const float sc = s[i / K], w = W[i];
  float c = sc > 0.f ? rintf(w / sc) : 0.f;
  c = fminf(fmaxf(c, -127.f), 127.f);
  q[i] = (int8_t)c;
  if (sc > 0.f && c * sc != w) atomicAdd(bad, 1);
}

void quant_codes(const float* W, const float* s, int N, int K, int8_t* q, int* bad, hipStream_t st) {
  const long n = (long)N * K;
  hipLaunchKernelGGL(k_quant_codes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, s, N, K, q, bad);
}

// ---------------------------------------------------------------------------------------------
// fp8 W8A8 split-K GEMM for the FlowLM step (ptts_engine_config.fp8_gemm; BASELINE configs[4]
// "fp8 MFMA GEMM path"). Not a reference numeric: the reference has no fp8 (quantize.rs is a
// simulated int8 grid), so this path is gated on accuracy against the f32 oracle.
//   W: OCP e4m3 codes [N][K], one scale per row (fp8_codes). A: the workgroup's K slice of its
//   32 rows is loaded once, each row's max |a| over the slice sets its scale (max/448), and the
//   e4m3 codes go to LDS. v_mfma_f32_32x32x16_fp8_fp8 then runs the slice: lane (r, h) supplies
//   the 16 bytes at k 32c+16h..+15 of A row r and of W row n as two 8-byte operands (A and B see
//   the same k permutation, so the dot products are unchanged). Products of two e4m3 values are
//   exact in f32; the slab value is acc * sa[row] * sw[col]. 4 waves deal the slice's 32-wide
//   chunks round-robin (W loads one chunk ahead) and are summed through LDS as in k_gemm_w8.
// ---------------------------------------------------------------------------------------------
constexpr int F8_LDA = FP8_KSLICE_MAX + 16;  // LDS row stride (bytes): 16-B skew between rows

template <int TN>
__global__ __launch_bounds__(256) void k_gemm_fp8(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sa8[32 * F8_LDA];
  __shared__ float sas[32];
  __shared__ float red[4 * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32 * TN, m0 = blockIdx.y * 32, z = blockIdx.z;
  const int nchunks = a.K >> 5;
  const int cb = (int)((long)nchunks * z / a.S), ce = (int)((long)nchunks * (z + 1) / a.S);
  const int ks = 32 * (ce - cb);  // slice length (<= FP8_KSLICE_MAX, host-checked)
  // ---- A slice: 8 threads per row, float4 j*8 + part; row max over the slice; e4m3 codes to LDS
  {
    const int row = tid >> 3, part = tid & 7;
    const bool live = m0 + row < a.M;
    const float* xr = a.X + (long)min(m0 + row, a.M - 1) * a.ldx + 32 * cb;
    constexpr int NJ = FP8_KSLICE_MAX / 32;
    float4 v[NJ];
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && 32 * j < ks) v[j] = *reinterpret_cast<const float4*>(xr + 4 * (8 * j + part));
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[j].x), fabsf(v[j].y)), fmaxf(fabsf(v[j].z), fabsf(v[j].w))));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
    const float inv = mx > 0.f ? 448.f / mx : 0.f;
    if (part == 0) sas[row] = mx / 448.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (32 * j < ks) {
        int q = __builtin_amdgcn_cvt_pk_fp8_f32(v[j].x * inv, v[j].y * inv, 0, false);
        q = __builtin_amdgcn_cvt_pk_fp8_f32(v[j].z * inv, v[j].w * inv, q, true);
        *reinterpret_cast<int*>(&sa8[row * F8_LDA + 4 * (8 * j + part)]) = q;
      }
    }
  }
  __syncthreads();
  const uint8_t* wrow[TN];
  float sc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int n = min(n0 + 32 * t + r, a.N - 1);
    wrow[t] = a.Wf8 + (long)n * a.K + 16 * h;
    sc[t] = a.wscale[n];
  }
  floatx16 acc[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;
  auto load = [&](int cc, uint4 (&Q)[TN]) {
#pragma unroll
    for (int t = 0; t < TN; ++t) Q[t] = *reinterpret_cast<const uint4*>(wrow[t] + (cc << 5));
  };
  auto mma = [&](int cc, uint4 (&Q)[TN]) {
    const uint4 A = *reinterpret_cast<const uint4*>(&sa8[r * F8_LDA + 32 * (cc - cb) + 16 * h]);
    const long a0 = (long)(((unsigned long)A.y << 32) | A.x), a1 = (long)(((unsigned long)A.w << 32) | A.z);
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const long b0 = (long)(((unsigned long)Q[t].y << 32) | Q[t].x);
      const long b1 = (long)(((unsigned long)Q[t].w << 32) | Q[t].z);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a0, b0, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a1, b1, acc[t], 0, 0, 0);
    }
  };
  uint4 q0[TN], q1[TN];
  const int c = cb + wave;
  const int n = c < ce ? (ce - c + 3) / 4 : 0;
  const int clast = c + (n - 1) * 4;
  auto chunk = [&](int i) { return i < n ? c + i * 4 : clast; };
  if (n > 0) {
    load(c, q0);
    int i = 0;
    for (; i + 2 <= n; i += 2) {
      load(chunk(i + 1), q1);
      mma(chunk(i), q0);
      load(chunk(i + 2), q0);
      mma(chunk(i + 1), q1);
    }
    if (i < n) mma(chunk(i), q0);
  }
#pragma unroll
  for (int t = 0; t < TN; ++t) {
#pragma unroll
    for (int g = 0; g < 16; ++g) red[(wave * 16 + g) * 64 + lane] = acc[t][g];
    __syncthreads();
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      const int g = wave * 4 + gg;
      const float v = red[g * 64 + lane] + red[(16 + g) * 64 + lane] + red[(32 + g) * 64 + lane] +
                      red[(48 + g) * 64 + lane];
      const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
      const int col = n0 + 32 * t + r;
      if (m0 + row < a.M && col < a.N) a.partial[((long)z * a.M + m0 + row) * a.N + col] = v * sas[row] * sc[t];
    }
    __syncthreads();
  }
}

// One workgroup per weight row: s = max|W[n][:]| / 448 (1 for an all-zero row), codes e4m3(W / s)
__global__ __launch_bounds__(256) void k_fp8_codes(const float* W, int K, uint8_t* q, float* s) {
  __shared__ float sh[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* w = W + (long)n * K;
  float mx = 0.f;
  for (int k = 4 * tid; k < K; k += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(w + k);
    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) sh[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  const float sc = mx > 0.f ? mx / 448.f : 1.f, inv = 1.f / sc;
  if (tid == 0) s[n] = sc;
  for (int k = 4 * tid; k < K; k += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(w + k);
    int c = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * inv, v.y * inv, 0, false);
    c = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * inv, v.w * inv, c, true);
    *reinterpret_cast<int*>(q + (long)n * K + k) = c;
  }
}

void fp8_codes(const float* W, int N, int K, uint8_t* q, float* s, hipStream_t st) {
  hipLaunchKernelGGL(k_fp8_codes, dim3((unsigned)N), dim3(256), 0, st, W, K, q, s);
}

// xcd_pn of a tile grid gx x gy (see xcd_tile): the split of the 8 XCDs over N and M tiles that
// moves the fewest operand bytes through the L2s, (8/pn) * |W| + pn * |A|; 0 when none divides.
static int choose_xcd_pn(const GemmArgs& a, int gx, int gy) {
  if (((long)gx * gy) % 8) return 0;
  const double wb = (double)a.N * a.K;
  const double ab = a.mode == 0 ? (double)a.M * a.K : (double)(a.M / a.Tq) * a.T_in * a.cin;
  int best = 0;
  double bc = 0;
  for (int pn : {8, 4, 2, 1}) {
    const int pm = 8 / pn;
    if (gx % pn || gy % pm) continue;
    const double c = pm * wb + pn * ab;
    if (!best || c < bc) best = pn, bc = c;
  }
  return best;
}
#ifdef PTTS_PROBES
static bool rr4_off() {  // PTTS_NO_RR4: the back part's 512-wide reduces one row per workgroup (A/B)
  static const bool v = getenv("PTTS_NO_RR4") != nullptr;
  return v;
}
static int back_probe() {
  static const int p = getenv("PTTS_BACK_PROBE") ? atoi(getenv("PTTS_BACK_PROBE")) : 0;
  return p;
}
static int front_probe() {  // the same probe on every uncapped launch (front part, prefill, ...)
  static const int p = getenv("PTTS_FRONT_PROBE") ? atoi(getenv("PTTS_FRONT_PROBE")) : 0;
  return p;
}
#else
static constexpr bool rr4_off() { return false; }
#endif
template <typename K>
static void launch_tiled(K kernel, dim3 grid, int threads, hipStream_t s, const GemmArgs& a) {
  GemmArgs b = a;
  b.xcd_pn = choose_xcd_pn(a, (int)grid.x, (int)grid.y);
  b.back_hi = g_back_hi;
#ifdef PTTS_PROBES
  b.probe = g_wg_cap > 0 ? back_probe() : front_probe();  // the cap is set exactly while the back part is captured
#endif
  hipLaunchKernelGGL(kernel, grid, dim3(threads), cap_lds(kernel, std::max(a.max_wg_per_cu, g_wg_cap)), s, b);
}

// Split tail (GemmArgs::tail_S): whole rounds of the CUs' workgroup slots (256 CUs x MINB) run
// whole tiles; the remaining tiles are cut into tail_S K slices that run as the last round.
static constexpr int NUM_CUS = 256;
template <typename K>
static void launch_split_tail(K kernel, int TM, int TN, int minb, hipStream_t s, const GemmArgs& a) {
  GemmArgs b = a;
  b.tiles_n = (a.N + TN - 1) / TN;
  const int tiles_m = (a.M + TM - 1) / TM, tiles = b.tiles_n * tiles_m, slots = NUM_CUS * minb;
  b.tail_full = tiles / slots * slots;
  const int rem = tiles - b.tail_full;
  if (rem == 0) {  // whole rounds: every workgroup takes a whole tile, the ordinary 2-D grid
    b.tail_S = 0;
    launch_tiled(kernel, dim3((unsigned)b.tiles_n, (unsigned)tiles_m, 1), 256, s, b);
    return;
  }
  b.tail_S = std::min(b.tail_S, a.K / 32);
  while (b.tail_S > 1 && (long)rem * b.tail_S * TM * TN > a.tail_cap) --b.tail_S;  // scratch-bound
  if (b.tail_S <= 1) {
    b.tail_S = 0;
    launch_tiled(kernel, dim3((unsigned)b.tiles_n, (unsigned)tiles_m, 1), 256, s, b);
    return;
  }
  if (rem > a.tickets_cap || !a.tail_slab || !a.tickets || a.S != 1)
    throw std::runtime_error("gemm: split tail needs its slab and tickets and S == 1");
  b.xcd_pn = 0;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(b.tail_full + rem * b.tail_S)), dim3(256),
                     cap_lds(kernel, a.max_wg_per_cu), s, b);
}

// One tile launch: the kernel instantiation, the grid and the threads all come from the tile's
// row of PTTS_TILES (kernels.h)
template <int MODE, int ID>
static void launch_tile(const GemmArgs& a, int grid_z, hipStream_t s) {
  constexpr TileInfo T = *tile_row(ID);
  const dim3 grid((a.N + T.tn() - 1) / T.tn(), (a.M + T.tm() - 1) / T.tm(), grid_z);
  if constexpr (T.family == TILE_GEMM) {
    launch_tiled((k_gemm<MODE, ID>), grid, T.threads, s, a);
  } else if constexpr (T.family == TILE_RB) {
    launch_tiled((k_gemm_rb<MODE, T.tmw, T.tnw>), grid, T.threads, s, a);
  } else {
    constexpr auto kernel = k_gemm_glds<MODE, T.wm, T.wn, T.bk, T.nbuf, T.tmw, T.tnw, T.minb, T.ilv, (int)T.ops>;
    if (T.split_weights() && (!a.Whm || !a.Wlo))
      throw std::runtime_error("gemm: bf16x6 layout without its split weights");
    if (MODE == 0 && T.split_tail() && a.tail_S > 0) launch_split_tail(kernel, T.tm(), T.tn(), T.minb, s, a);
    else launch_tiled(kernel, grid, T.threads, s, a);
  }
}

// a probe-only row expands to nothing in a product build
#define PTTS_TILE_IF_0(...) __VA_ARGS__
#ifdef PTTS_PROBES
#define PTTS_TILE_IF_1(...) __VA_ARGS__
#else
#define PTTS_TILE_IF_1(...)
#endif
template <int MODE>
static void gemm_launch(const GemmArgs& a, int grid_z, hipStream_t s) {
  switch (a.layout) {
#define PTTS_TILE_CASE(ID, FAM, WM, WN, BK, NBUF, TMW, TNW, MINB, ILV, OPS, THR, PROBE) \
  PTTS_TILE_IF_##PROBE(case ID: return launch_tile<MODE, ID>(a, grid_z, s);)
    PTTS_TILES(PTTS_TILE_CASE)
#undef PTTS_TILE_CASE
    default:
      throw std::runtime_error("gemm: tile layout " + std::to_string(a.layout) + " is not in this build");
  }
}

// split3 (kernels.h): round-to-nearest-even pieces, each remainder exact in f32
__global__ __launch_bounds__(256) void k_split3(const float* __restrict__ W, long n, unsigned* __restrict__ hm,
                                                unsigned short* __restrict__ lo) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float x = W[i];
    const __bf16 p0 = (__bf16)x;
    const float r = x - (float)p0;
    const __bf16 p1 = (__bf16)r;
    const __bf16 p2 = (__bf16)(r - (float)p1);
    hm[i] = (unsigned)__builtin_bit_cast(unsigned short, p0) << 16 | __builtin_bit_cast(unsigned short, p1);
    lo[i] = __builtin_bit_cast(unsigned short, p2);
  }
}
void split3(const float* W, long n, unsigned* hm, unsigned short* lo, hipStream_t s) {
  const long blocks = std::min<long>((n + 255) / 256, 4096);
  if (blocks > 0) hipLaunchKernelGGL(k_split3, dim3((unsigned)blocks), dim3(256), 0, s, W, n, hm, lo);
}

void gemm(const GemmArgs& a, int grid_z, hipStream_t s) {
  if (a.Wf8) {  // fp8 W8A8: 32x64 tiles
    hipLaunchKernelGGL((k_gemm_fp8<2>), dim3((a.N + 63) / 64, (a.M + 31) / 32, grid_z), dim3(256), 0, s, a);
    return;
  }
  if (a.Wq) {  // int8 weights: 32x64 tiles
    hipLaunchKernelGGL((k_gemm_w8<2>), dim3((a.N + 63) / 64, (a.M + 31) / 32, grid_z), dim3(256), 0, s, a);
    return;
  }
  // MODE 1 = implicit-GEMM conv, MODE 2 = the same with ELU applied to A on load
  if (a.mode == 0) gemm_launch<0>(a, grid_z, s);
  else if (a.elu_in) gemm_launch<2>(a, grid_z, s);
  else gemm_launch<1>(a, grid_z, s);
}

// =============================================================================================
// Skinny split-K GEMM with register-resident weights (see kernels.h). Packed layout, per
// (tile t, slice z, wave w): NV = kw / 8 groups of 64 float4, group j lane l = W[n][k..k+3] with
//   n = t * 32 * WN + (w % WN) * 32 + (l & 31),  k = z * ks + (w / WN) * kw + (l >> 5) * kw / 2 + 4 j,
// so lane l holds the B operand of v_mfma_f32_32x32x2f32 for the steps s = 0 .. kw/2 - 1 of its
// wave, k = base + (l >> 5) * kw / 2 + s (the two lane halves take the two k of a step from the two
// halves of the wave's k range: the MFMA K order is a permutation of the sum). A (X's slice) is
// read from LDS in the same order: lane l, row l & 31, the same k.
// =============================================================================================
__global__ void k_pack_gemv(const float* __restrict__ W, int N, int K, int wn, int kw, float* __restrict__ P) {
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;  // float4 index into P
  const long total4 = (long)N * K / 4;
  if (i4 >= total4) return;
  const int nv = kw / 8, ks = kw * (4 / wn), S = K / ks;
  const int lane = (int)(i4 & 63);
  long r = i4 >> 6;
  const int j = (int)(r % nv);
  r /= nv;
  const int w = (int)(r & 3);
  r >>= 2;
  const int z = (int)(r % S);
  const int t = (int)(r / S);
  const int n = t * 32 * wn + (w % wn) * 32 + (lane & 31);
  const int k = z * ks + (w / wn) * kw + (lane >> 5) * (kw / 2) + 4 * j;
  reinterpret_cast<float4*>(P)[i4] = *reinterpret_cast<const float4*>(W + (long)n * K + k);
}

// int8 weight codes (engines with weight_quant): code word -> the f32 weight quad float(q) * s
__device__ __forceinline__ float4 q8_quad(unsigned q, float sc) {
  return make_float4((float)(int)(signed char)(q & 0xff) * sc, (float)(int)(signed char)((q >> 8) & 0xff) * sc,
                     (float)(int)(signed char)((q >> 16) & 0xff) * sc, (float)((int)q >> 24) * sc);
}

// fp8 A operand: 8 f32 values * inv -> 8 e4m3 bytes (one MFMA operand)
__device__ __forceinline__ long f8_pack8(const float* v, float inv) {
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
  return (long)(((unsigned long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ long u32x2_long(unsigned lo, unsigned hi) {
  return (long)(((unsigned long)hi << 32) | lo);
}

// WQ: the weight form. 0 f32 fragments; 1 int8 codes of a quantized matrix (weight_quant: widened
// to the same f32 weights in registers); 2 e4m3 codes (fp8_gemm, W8A8: {4, 128} tiles only) - the
// 32 rows of the X slice quantized to e4m3 with one scale per (row, slice) = max |x| / 448 (every
// wave computes the same scales from the LDS slice), v_mfma_f32_32x32x16_fp8_fp8 over the slice
// (lane (r, h) supplies k 64 h + 8 s .. + 7 of step s for A and B alike), slab = acc * sa * sw.
template <int WN, int KW, int WQ = 0>
__global__ __launch_bounds__(256) void k_gemv(const float* __restrict__ X, long ldx, int M, int N,
                                              const float* __restrict__ P, float* __restrict__ partial,
                                              const uint32_t* __restrict__ P8, const float* __restrict__ scale) {
  static_assert(WQ != 2 || (WN == 4 && KW == 128), "fp8 gemv: {4, 128} tiles");
  constexpr bool Q8 = WQ == 1;
  front_prio();
  constexpr int WK = 4 / WN, KS = KW * WK, NV = KW / 8, LDA = KS + 4;  // +4: conflict-free b128 rows
  __shared__ __attribute__((aligned(16))) float sA[32 * LDA];
  __shared__ __attribute__((aligned(16))) float red[WK > 1 ? 4 * 16 * 64 : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x, z = blockIdx.y, S = gridDim.y, m0 = 32 * blockIdx.z;  // z: K slice; blockIdx.z: 32-row block
  // X's slice first (the LDS fill waits only for these loads), then every weight load
  constexpr int AV = 32 * KS / 4 / 256;  // float4 of X per thread
  float4 av[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const int e = tid + 256 * i, row = e / (KS / 4), c4 = e % (KS / 4);
    av[i] = m0 + row < M ? *reinterpret_cast<const float4*>(X + (long)(m0 + row) * ldx + (long)z * KS + 4 * c4)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v* wp = reinterpret_cast<const f4v*>(P) + (((long)t * S + z) * 4 + wave) * NV * 64 + lane;
  f4v w[WQ ? 1 : NV];
  u32x4 wq[WQ ? NV / 4 : 1];
  const int m = lane & 31, h = lane >> 5, wn = wave % WN, wk = wave / WN;
  const int n = t * 32 * WN + wn * 32 + m;
  if (WQ) {  // codes: NV / 4 16-B loads per lane (pack_q8 order)
    const u32x4* qp = reinterpret_cast<const u32x4*>(P8) + (((long)t * S + z) * 4 + wave) * (NV / 4) * 64 + lane;
#pragma unroll
    for (int j = 0; j < NV / 4; ++j)
      wq[j] = (front_skip() & 1) ? u32x4{0u, 0u, 0u, 0u} : __builtin_nontemporal_load(qp + j * 64);
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j)
      w[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + j * 64);  // once-read
  }
  const float sc = WQ ? scale[n] : 0.f;
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const int e = tid + 256 * i, row = e / (KS / 4), c4 = e % (KS / 4);
    *reinterpret_cast<float4*>(&sA[row * LDA + 4 * c4]) = av[i];
  }
  __syncthreads();
  const float* ar = &sA[m * LDA + wk * KW + h * (KW / 2)];
  floatx16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  if (WQ == 2) {  // ---- fp8 W8A8: this lane's 64 values of row m, the row scale, 8 fp8 MFMAs
    float xv[KW / 2];
#pragma unroll
    for (int j = 0; j < KW / 8; ++j) {
      const float4 a = *reinterpret_cast<const float4*>(ar + 4 * j);
      xv[4 * j] = a.x, xv[4 * j + 1] = a.y, xv[4 * j + 2] = a.z, xv[4 * j + 3] = a.w;
    }
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < KW / 2; ++j) mx = fmaxf(mx, fabsf(xv[j]));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float inv = mx > 0.f ? 448.f / mx : 0.f, sa = mx / 448.f;
#pragma unroll
    for (int st = 0; st < KW / 16; ++st) {
      const long a8 = f8_pack8(&xv[8 * st], inv);
      const u32x4 q = wq[st >> 1];
      const long b8 = (st & 1) ? u32x2_long(q[2], q[3]) : u32x2_long(q[0], q[1]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a8, b8, acc, 0, 0, 0);
    }
    // slab value acc * sa(row) * sw(column): the row of register g is (g & 3) + 8 (g >> 2) + 4 h
    float* out = partial + (long)z * M * N;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int rl = (g & 3) + 8 * (g >> 2) + 4 * h, row = m0 + rl;
      const float sar = __shfl(sa, rl, 64);
      if (row < M) out[(long)row * N + n] = acc[g] * sar * sc;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (front_skip() & 2) break;
    const float4 a = *reinterpret_cast<const float4*>(ar + 4 * j);
    float4 b;
    if (Q8) b = q8_quad(wq[j / 4][j % 4], sc);
    else b = make_float4(w[j].x, w[j].y, w[j].z, w[j].w);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  float* out = partial + (long)z * M * N;
  if (WK == 1) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = m0 + (g & 3) + 8 * (g >> 2) + 4 * h;
      if (row < M) out[(long)row * N + n] = acc[g];
    }
    return;
  }
  // WK > 1: the WK waves of column block c (waves c, c + WN, ..) hold partials over their k
  // ranges; the 16 * WN (block, register) outputs are dealt 4 * WN per wave and summed in k order
#pragma unroll
  for (int g = 0; g < 16; ++g) red[(wave * 16 + g) * 64 + lane] = acc[g];
  __syncthreads();
#pragma unroll
  for (int ff = 0; ff < 4 * WN; ++ff) {
    const int f = wave * 4 * WN + ff, c = f / 16, g = f % 16;
    float v = red[(c * 16 + g) * 64 + lane];
#pragma unroll
    for (int kk = 1; kk < WK; ++kk) v += red[((kk * WN + c) * 16 + g) * 64 + lane];
    const int row = m0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (row < M) out[(long)row * N + t * 32 * WN + c * 32 + m] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Whole-K skinny GEMM (kernels.h gemv_fk). Fragment orders, K = 1024, wave w (0..7) covering
// k = 128 w .. 128 w + 127, lane l = 16 g + c (g = l >> 4 the lane group, c = l & 15):
//   A: lane (g, r) of row tile t holds k = 128 w + 32 g + s, s = 0..31, for row 16 t + r, as 8 float4
//      j = s / 4: float4 index ((w * 2 + t) * 8 + j) * 64 + l  (FK_A_FLOATS floats for 32 rows)
//   W: lane (g, c) of column tile n0 / 16 holds k = 128 w + 32 g + s of column n0 + c:
//      float4 index ((n0 / 16 * 8 + w) * 8 + j) * 64 + l
// MFMA step s (16x16x4, lane group g supplies the step's k index g) sums k = 128 w + 32 g + s over
// g for both operands alike: each wave's 128 k are covered once (a permutation of the order).
__device__ __forceinline__ long fk_afrag_index(int row, int k) {  // float index into the A fragment
  const int w = k >> 7, g = (k >> 5) & 3, s = k & 31, t = row >> 4, r = row & 15;
  return ((((long)(w * 2 + t) * 8 + (s >> 2)) * 64 + (g * 16 + r)) << 2) + (s & 3);
}
__global__ void k_pack_gemv_fk(const float* __restrict__ W, int N, int K, float* __restrict__ P) {
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= (long)N * K / 4) return;
  const int l = (int)(i4 & 63), j = (int)((i4 >> 6) & 7), w = (int)((i4 >> 9) & 7);
  const int ct = (int)(i4 >> 12);
  const int n = ct * 16 + (l & 15), k = w * 128 + (l >> 4) * 32 + 4 * j;
  reinterpret_cast<float4*>(P)[i4] = *reinterpret_cast<const float4*>(W + (long)n * K + k);
}
__global__ __launch_bounds__(512) void k_gemv_fk(const float* __restrict__ A, int M, int N,
                                                 const float* __restrict__ P, const float* __restrict__ bias,
                                                 int act, float* __restrict__ Y, long ldy) {
  front_prio();
  __shared__ __attribute__((aligned(16))) float red[8 * 2 * 4 * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ct = blockIdx.x;
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v* wp = reinterpret_cast<const f4v*>(P) + ((long)(ct * 8 + w) * 8) * 64 + lane;
  const f4v* ap = reinterpret_cast<const f4v*>(A) + ((long)(w * 2) * 8) * 64 + lane;
  f4v b[8], a0[8], a1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    b[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + j * 64);  // once-read
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a0[j] = ap[j * 64];
    a1[j] = ap[(8 + j) * 64];
  }
  // every load in flight before the first MFMA (the scheduler otherwise sinks them next to their
  // use: a few loads in flight at a time, one round trip each)
  __builtin_amdgcn_sched_barrier(0);
  floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (front_skip() & 2) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j][e], b[j][e], c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j][e], b[j][e], c1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[((w * 2 + 0) * 4 + i) * 64 + lane] = c0[i];
    red[((w * 2 + 1) * 4 + i) * 64 + lane] = c1[i];
  }
  __syncthreads();
  // thread tid: row tile t, register i, lane ll (C map: column ll & 15, row (ll >> 4) * 4 + i)
  const int t = tid >> 8, i = (tid >> 6) & 3, ll = tid & 63;
  float v = red[((0 * 2 + t) * 4 + i) * 64 + ll];
#pragma unroll
  for (int ww = 1; ww < 8; ++ww) v += red[((ww * 2 + t) * 4 + i) * 64 + ll];
  const int row = 16 * t + (ll >> 4) * 4 + i, col = ct * 16 + (ll & 15);
  if (row < M) {
    if (bias) v += bias[col];
    if (act == ACT_GELU) v = gelu_tanh(v);
    Y[(long)row * ldy + col] = v;
  }
}

bool gemv_fk_supported(int M, int N, int K) { return M >= 1 && M <= 32 && K == FK_K && N % 16 == 0; }

void pack_gemv_fk(const float* W, int N, int K, float* packed, hipStream_t s) {
  if (!gemv_fk_supported(1, N, K)) throw std::runtime_error("pack_gemv_fk: unsupported shape");
  const long total4 = (long)N * K / 4;
  hipLaunchKernelGGL(k_pack_gemv_fk, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, W, N, K, packed);
}

void gemv_fk(const float* Afrag, int M, int N, const float* packed, const float* bias, int act, float* Y, long ldy,
             hipStream_t s) {
  if (!gemv_fk_supported(M, N, FK_K) || (act != ACT_NONE && act != ACT_GELU))
    throw std::runtime_error("gemv_fk: unsupported shape");
  hipLaunchKernelGGL(k_gemv_fk, dim3((unsigned)(N / 16)), dim3(512), cap_lds(k_gemv_fk, g_wg_cap), s, Afrag, M, N,
                     packed, bias, act, Y, ldy);
}

// ---------------------------------------------------------------------------------------------
// Fused FlowLM feed-forward of a step pass (kernels.h ffn_fused). Workgroup L (512 threads) is
// member i of group z, with all 16 members of a group on one XCD when workgroups are dealt to the
// XCDs round-robin (speed only: the hand-off is coherent across XCDs). Linear2 fragments (packed
// by pack_ffn2), float4 index (((z * 16 + i) * 8 + w) * 8 + j) * 64 + l: lane l of wave w holds
// W2[n][k .. k + 3], n = 64 i + 32 (w & 1) + (l & 31), k = 256 z + 64 (w >> 1) + 32 (l >> 5) + 4 j:
// the B operand of v_mfma_f32_32x32x2f32 for the wave's 32 steps (k-half l >> 5 as in k_gemv).
// The hand-off region of group z holds linear1's 32 x 256 outputs in the matching A order: float4
// (q * 8 + j) * 64 + l = U[row l & 31][64 q + 32 (l >> 5) + 4 j .. + 3].
// ---------------------------------------------------------------------------------------------
template <int NG>
__global__ void k_pack_ffn2(const float* __restrict__ W, float* __restrict__ P) {
  constexpr int MB = 256 / NG, CT = 1024 / MB / 32;  // members per group, 32-column tiles per member
  const long f = (long)blockIdx.x * 256 + threadIdx.x;  // float4 index into P
  if (f >= 1024L * 4096 / 4) return;
  const int l = (int)(f & 63), j = (int)((f >> 6) & 7), w = (int)((f >> 9) & 7);
  const long r = f >> 12;
  const int i = (int)(r % MB), z = (int)(r / MB);
  const int n = (1024 / MB) * i + 32 * (w % CT) + (l & 31), k = (4096 / NG) * z + 64 * (w / CT) + 32 * (l >> 5) + 4 * j;
  reinterpret_cast<float4*>(P)[f] = *reinterpret_cast<const float4*>(W + (long)n * 4096 + k);
}

// WQ as k_gemv: 0 f32, 1 int8 codes widened to f32, 2 e4m3 codes W8A8 on the fp8 MFMA - linear1:
// each wave quantizes its two 16-row A tiles over its 128 k (one scale per (row, wave), max |a| /
// 448 over the 4 lane groups of the row) and runs v_mfma_f32_16x16x32_fp8_fp8 (lane group g
// supplies k 128 w + 32 g + 8 s .. + 7 of step s for A and B alike); linear2: each wave its 32 rows
// over its 64-k part (lanes r, r + 32), v_mfma_f32_32x32x16_fp8_fp8; a wave's partial tile is
// scaled by its row scales before the cross-wave sums, the column scale applied after them.
template <int NG, int WQ = 0>
__global__ __launch_bounds__(512) void k_ffn_fused(const float* __restrict__ A, int M, const float* __restrict__ P1,
                                                   const float* __restrict__ P2, float* __restrict__ hand, int set,
                                                   float* __restrict__ P, int* err, const uint32_t* __restrict__ Q1,
                                                   const float* __restrict__ s1, const uint32_t* __restrict__ Q2,
                                                   const float* __restrict__ s2) {
  constexpr int MB = 256 / NG;        // members per group
  constexpr int CT = 1024 / MB / 32;  // linear2 32-column tiles per member
  constexpr int KG = 4096 / NG;       // linear2 K slice of a group = linear1 columns of the group
  front_prio();
  __shared__ __attribute__((aligned(16))) float red[8 * 16 * 64];  // phase 1: 8 x 2 x 4 x 64; phase 2: all
  __shared__ __attribute__((aligned(16))) float sU[32 * 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = blockIdx.x;
  int z, i;  // group (linear2 slice), member
  if (NG == 16) {  // a group's 16 members on one XCD (workgroups dealt round-robin; speed only)
    const int x = L & 7, jj = L >> 3;
    z = 2 * x + (jj >> 4);
    i = jj & 15;
  } else {  // contiguous members: progress needs only one group co-resident
    z = L / MB;
    i = L % MB;
  }
  const int ct = MB * z + i;  // linear1 column tile: columns 16 ct .. 16 ct + 15
  typedef float f4v __attribute__((ext_vector_type(4)));
  // every operand that does not depend on the hand-off, requested up front: linear1's weight and
  // A fragments (as k_gemv_fk), then linear2's weight fragment (used after the hand-off)
  const f4v* wp = reinterpret_cast<const f4v*>(P1) + ((long)(ct * 8 + w) * 8) * 64 + lane;
  const f4v* ap = reinterpret_cast<const f4v*>(A) + ((long)(w * 2) * 8) * 64 + lane;
  const f4v* w2p = reinterpret_cast<const f4v*>(P2) + ((long)((z * MB + i) * 8 + w) * 8) * 64 + lane;
  constexpr bool Q8 = WQ != 0;
  f4v b[Q8 ? 1 : 8], a0[8], a1[8], b2[Q8 ? 1 : 8];
  u32x4 q1[Q8 ? 2 : 1], q2[Q8 ? 2 : 1];
  if (Q8) {  // int8 / e4m3 codes (pack_q8 order): two 16-B loads per lane and matrix
    const u32x4* q1p = reinterpret_cast<const u32x4*>(Q1) + ((long)(ct * 8 + w) * 2) * 64 + lane;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      q1[j] = (front_skip() & 1) ? u32x4{0u, 0u, 0u, 0u} : __builtin_nontemporal_load(q1p + j * 64);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      b[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + j * 64);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a0[j] = ap[j * 64];
    a1[j] = ap[(8 + j) * 64];
  }
  if (Q8) {
    const u32x4* q2p = reinterpret_cast<const u32x4*>(Q2) + ((long)((z * MB + i) * 8 + w) * 2) * 64 + lane;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      q2[j] = (front_skip() & 1) ? u32x4{0u, 0u, 0u, 0u} : __builtin_nontemporal_load(q2p + j * 64);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      b2[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(w2p + j * 64);
  }
  // row scales of this lane's linear1 column and linear2 column (int8 codes)
  const float sc1 = Q8 ? s1[ct * 16 + (lane & 15)] : 0.f;
  const float sc2 = Q8 ? s2[(1024 / MB) * i + 32 * (w % CT) + (lane & 31)] : 0.f;
  __builtin_amdgcn_sched_barrier(0);
  // ---- linear1 + GELU (k_gemv_fk): two 16-row tiles, the 8 waves' partial tiles summed in LDS
  floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
  if (WQ == 2) {
    float x0[32], x1[32];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) x0[4 * j + e] = a0[j][e], x1[4 * j + e] = a1[j][e];
    float m0 = 0.f, m1 = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) m0 = fmaxf(m0, fabsf(x0[j])), m1 = fmaxf(m1, fabsf(x1[j]));
    m0 = fmaxf(m0, __shfl_xor(m0, 16, 64));
    m0 = fmaxf(m0, __shfl_xor(m0, 32, 64));
    m1 = fmaxf(m1, __shfl_xor(m1, 16, 64));
    m1 = fmaxf(m1, __shfl_xor(m1, 32, 64));
    const float i0 = m0 > 0.f ? 448.f / m0 : 0.f, i1 = m1 > 0.f ? 448.f / m1 : 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 q = q1[st >> 1];
      const long b8 = (st & 1) ? u32x2_long(q[2], q[3]) : u32x2_long(q[0], q[1]);
      c0 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8_pack8(&x0[8 * st], i0), b8, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8_pack8(&x1[8 * st], i1), b8, c1, 0, 0, 0);
    }
    // C register r of lane l: row (l >> 4) * 4 + r of the tile, whose scale lane that row holds
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rl = (lane >> 4) * 4 + r;
      c0[r] *= __shfl(m0, rl, 64) / 448.f;
      c1[r] *= __shfl(m1, rl, 64) / 448.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (front_skip() & 2) break;
      float4 bq;
      if (Q8) bq = q8_quad(q1[j / 4][j % 4], sc1);
      else bq = make_float4(b[j][0], b[j][1], b[j][2], b[j][3]);
      const float be[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j][e], be[e], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j][e], be[e], c1, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[((w * 2 + 0) * 4 + r) * 64 + lane] = c0[r];
    red[((w * 2 + 1) * 4 + r) * 64 + lane] = c1[r];
  }
  __syncthreads();
  {  // thread tid: row tile t, register r, lane ll (C map: column ll & 15, row (ll >> 4) * 4 + r)
    const int t = tid >> 8, r = (tid >> 6) & 3, ll = tid & 63;
    float v = red[((0 * 2 + t) * 4 + r) * 64 + ll];
#pragma unroll
    for (int ww = 1; ww < 8; ++ww) v += red[((ww * 2 + t) * 4 + r) * 64 + ll];
    const int row = 16 * t + (ll >> 4) * 4 + r;
    if (WQ == 2) v *= s1[ct * 16 + (ll & 15)];  // the e4m3 weight column's scale, after the wave sums
    sU[row * 16 + (ll & 15)] = row < M ? gelu_tanh(v) : 0.f;  // rows past M: handed off as 0
  }
  __syncthreads();
  const auto hr = sc1_rsrc(hand + (long)set * FFN_HAND_FLOATS + (long)z * 32 * KG);
  if (tid < 128) {  // publish: row m, columns 4 c4 .. 4 c4 + 3 of this tile = k_local 16 i + 4 c4
    const int m = tid & 31, c4 = tid >> 5;
    const int q = i >> 2, h = (i >> 1) & 1, j = 4 * (i & 1) + c4;
    const float4 v = *reinterpret_cast<const float4*>(&sU[m * 16 + 4 * c4]);
    fh_put(hr, (((q * 8 + j) * 64) + h * 32 + m) * 16, v);
  }
  // ---- linear2, slice z: wave w = (column tile w % CT, 64-k part q = w / CT); its A fragment is
  // linear1's output of the group's members 4 q .. 4 q + 3, swept until none is empty
  const int q = w / CT;
  float4 av[8];
  bool dead = false;
  {
#pragma unroll
    for (int j = 0; j < 8; ++j) av[j] = fh_ld(hr, ((q * 8 + j) * 64 + lane) * 16);
    unsigned spins = 0;
    while (true) {
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 8; ++j) ok &= !fh_empty(av[j]);
      if (__all(ok)) break;
      __builtin_amdgcn_s_sleep(1);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (fh_empty(av[j])) av[j] = fh_ld(hr, ((q * 8 + j) * 64 + lane) * 16);
      if (++spins > (1u << 20)) {
        if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dead = true;
        break;
      }
    }
  }
  (void)dead;
  floatx16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  if (WQ == 2) {
    float xv[32];
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[4 * j] = av[j].x, xv[4 * j + 1] = av[j].y, xv[4 * j + 2] = av[j].z, xv[4 * j + 3] = av[j].w;
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) mx = fmaxf(mx, fabsf(xv[j]));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float inv = mx > 0.f ? 448.f / mx : 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 q = q2[st >> 1];
      const long b8 = (st & 1) ? u32x2_long(q[2], q[3]) : u32x2_long(q[0], q[1]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(f8_pack8(&xv[8 * st], inv), b8, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] *= __shfl(mx, (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), 64) / 448.f;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (front_skip() & 2) break;
      float4 bq;
      if (Q8) bq = q8_quad(q2[j / 4][j % 4], sc2);
      else bq = make_float4(b2[j][0], b2[j][1], b2[j][2], b2[j][3]);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].x, bq.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].y, bq.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].z, bq.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j].w, bq.w, acc, 0, 0, 0);
    }
  }
  // the 8 / CT k parts of each column tile summed in k order; slab z of P
#pragma unroll
  for (int g = 0; g < 16; ++g) red[(w * 16 + g) * 64 + lane] = acc[g];
  __syncthreads();
  {
    float* out = P + (long)z * M * 1024;
#pragma unroll
    for (int rr = 0; rr < 2 * CT; ++rr) {
      const int f = tid + 512 * rr;  // (column tile c, register g, lane ll)
      const int c = f >> 10, g = (f >> 6) & 15, ll = f & 63;
      float v = red[((0 * CT + c) * 16 + g) * 64 + ll];
#pragma unroll
      for (int qq = 1; qq < 8 / CT; ++qq) v += red[((qq * CT + c) * 16 + g) * 64 + ll];
      const int row = (g & 3) + 8 * (g >> 2) + 4 * (ll >> 5);
      const int col = (1024 / MB) * i + 32 * c + (ll & 31);
      if (WQ == 2) v *= s2[col];  // the e4m3 weight column's scale, after the k-part sums
      if (row < M) out[(long)row * 1024 + col] = v;
    }
  }
  // empty this workgroup's float4s of the other set for the next launch
  if (tid < 128) {
    const int m = tid & 31, c4 = tid >> 5;
    const int qh = i >> 2, h = (i >> 1) & 1, j = 4 * (i & 1) + c4;
    const auto er = sc1_rsrc(hand + (long)(set ^ 1) * FFN_HAND_FLOATS + (long)z * 32 * KG);
    fh_st(er, (((qh * 8 + j) * 64) + h * 32 + m) * 16,
          make_float4(__uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u)));
  }
}

bool ffn_fused_supported(int M, int D, int FF) { return M >= 1 && M <= 32 && D == 1024 && FF == 4096; }

void pack_ffn2(const float* W2, int groups, float* packed, hipStream_t s) {
  if (groups == 16) hipLaunchKernelGGL(k_pack_ffn2<16>, dim3(1024 * 4096 / 4 / 256), dim3(256), 0, s, W2, packed);
  else if (groups == 8) hipLaunchKernelGGL(k_pack_ffn2<8>, dim3(1024 * 4096 / 4 / 256), dim3(256), 0, s, W2, packed);
  else throw std::runtime_error("pack_ffn2: 8 or 16 groups");
}

void ffn_fused(const float* Afrag, int M, const float* P1, const float* P2, int groups, float* hand, int set, float* P,
               int* err, hipStream_t s, const uint32_t* Q1, const float* s1, const uint32_t* Q2, const float* s2,
               bool fp8) {
  if (!ffn_fused_supported(M, 1024, 4096) || (set != 0 && set != 1) || (groups != 8 && groups != 16))
    throw std::runtime_error("ffn_fused: bad shape");
  if (!Q1 != !Q2 || (Q1 && (!s1 || !s2))) throw std::runtime_error("ffn_fused: int8 codes of both matrices, with scales");
  if (Q1 && fp8 && groups == 8)
    hipLaunchKernelGGL((k_ffn_fused<8, 2>), dim3(256), dim3(512), cap_lds(k_ffn_fused<8, 2>, g_wg_cap), s, Afrag, M, P1,
                       P2, hand, set, P, err, Q1, s1, Q2, s2);
  else if (Q1 && fp8)
    throw std::runtime_error("ffn_fused: fp8 codes with 8 groups only");
  else if (Q1 && groups == 8)
    hipLaunchKernelGGL((k_ffn_fused<8, 1>), dim3(256), dim3(512), cap_lds(k_ffn_fused<8, 1>, g_wg_cap), s, Afrag, M,
                       P1, P2, hand, set, P, err, Q1, s1, Q2, s2);
  else if (Q1)
    hipLaunchKernelGGL((k_ffn_fused<16, 1>), dim3(256), dim3(512), cap_lds(k_ffn_fused<16, 1>, g_wg_cap), s,
                       Afrag, M, P1, P2, hand, set, P, err, Q1, s1, Q2, s2);
  else if (groups == 16)
    hipLaunchKernelGGL(k_ffn_fused<16>, dim3(256), dim3(512), cap_lds(k_ffn_fused<16>, g_wg_cap), s, Afrag, M, P1, P2,
                       hand, set, P, err, nullptr, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL(k_ffn_fused<8>, dim3(256), dim3(512), cap_lds(k_ffn_fused<8>, g_wg_cap), s, Afrag, M, P1, P2,
                       hand, set, P, err, nullptr, nullptr, nullptr, nullptr);
}

__global__ void k_codes_to_f32(const int8_t* __restrict__ q, long n, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (float)q[i];
}
void codes_to_f32(const int8_t* q, long n, float* out, hipStream_t s) {
  const long blocks = std::min<long>((n + 255) / 256, 8192);
  if (blocks > 0) hipLaunchKernelGGL(k_codes_to_f32, dim3((unsigned)blocks), dim3(256), 0, s, q, n, out);
}
__global__ void k_codes_u8_to_f32(const uint8_t* __restrict__ q, long n, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (float)q[i];
}
void codes_u8_to_f32(const uint8_t* q, long n, float* out, hipStream_t s) {
  const long blocks = std::min<long>((n + 255) / 256, 8192);
  if (blocks > 0) hipLaunchKernelGGL(k_codes_u8_to_f32, dim3((unsigned)blocks), dim3(256), 0, s, q, n, out);
}
__global__ void k_pack_q8(const float* __restrict__ pf, long n16, int nj, uint32_t* __restrict__ q8) {
  const long gi = (long)blockIdx.x * 256 + threadIdx.x;  // u32x4 index
  if (gi >= n16) return;
  const int l = (int)(gi & 63);
  const long q = gi >> 6;
  const int J = (int)(q % (nj / 4));
  const long P = q / (nj / 4);
  u32x4 o;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const float4 f = reinterpret_cast<const float4*>(pf)[(P * nj + 4 * J + jj) * 64 + l];
    o[jj] = ((unsigned)(int)f.x & 0xffu) | (((unsigned)(int)f.y & 0xffu) << 8) | (((unsigned)(int)f.z & 0xffu) << 16) |
            ((unsigned)(int)f.w << 24);
  }
  reinterpret_cast<u32x4*>(q8)[gi] = o;
}
void pack_q8(const float* packed_codes, long n4, int nj, uint32_t* q8, hipStream_t s) {
  if (nj % 4 != 0 || n4 % ((long)nj * 64) != 0) throw std::runtime_error("pack_q8: bad shape");
  const long n16 = n4 / 4;
  hipLaunchKernelGGL(k_pack_q8, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, packed_codes, n16, nj, q8);
}

bool gemv_supported(GemvShape g, int N, int K) {
  const bool shape = (g.wn == 4 && g.kw == 128) || (g.wn == 1 && g.kw == 32) || (g.wn == 1 && g.kw == 64) ||
                     (g.wn == 2 && g.kw == 64);
  return shape && N % (32 * g.wn) == 0 && K % g.ks() == 0 && K / g.ks() <= 16;
}

void pack_gemv(const float* W, int N, int K, GemvShape g, float* packed, hipStream_t s) {
  if (!gemv_supported(g, N, K)) throw std::runtime_error("pack_gemv: unsupported shape");
  const long total4 = (long)N * K / 4;
  hipLaunchKernelGGL(k_pack_gemv, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, W, N, K, g.wn, g.kw,
                     packed);
}

void gemv_splitk(const float* X, long ldx, int M, int N, int K, const float* packed, GemvShape g, float* partial,
                 hipStream_t s, const uint32_t* q8, const float* scale, bool fp8) {
  if (M < 1 || M > 64 || !gemv_supported(g, N, K)) throw std::runtime_error("gemv_splitk: unsupported shape");
  if (q8 && (!scale || g.kw % 32 != 0)) throw std::runtime_error("gemv_splitk: int8 codes need scales, kw % 32 == 0");
  const dim3 grid((unsigned)(N / (32 * g.wn)), (unsigned)(K / g.ks()), (unsigned)((M + 31) / 32));
#define PTTS_GEMV(WN_, KW_)                                                                              \
  if (g.wn == WN_ && g.kw == KW_) {                                                                      \
    if (q8 && fp8 && WN_ == 4 && KW_ == 128)                                                             \
      hipLaunchKernelGGL((k_gemv<4, 128, 2>), grid, dim3(256), cap_lds(k_gemv<4, 128, 2>, g_wg_cap), s, X, ldx, M, \
                         N, packed, partial, q8, scale);                                                 \
    else if (q8 && !fp8)                                                                                 \
      hipLaunchKernelGGL((k_gemv<WN_, KW_, 1>), grid, dim3(256), cap_lds(k_gemv<WN_, KW_, 1>, g_wg_cap), s, X, \
                         ldx, M, N, packed, partial, q8, scale);                                         \
    else if (q8)                                                                                         \
      throw std::runtime_error("gemv_splitk: fp8 codes on {4, 128} tiles only");                        \
    else                                                                                                 \
      hipLaunchKernelGGL((k_gemv<WN_, KW_>), grid, dim3(256), cap_lds(k_gemv<WN_, KW_>, g_wg_cap), s, X, ldx, M, \
                         N, packed, partial, nullptr, nullptr);                                          \
    return;                                                                                              \
  }
  PTTS_GEMV(4, 128)
  PTTS_GEMV(2, 64)
  PTTS_GEMV(1, 64)
  PTTS_GEMV(1, 32)
#undef PTTS_GEMV
}

// =============================================================================================
// Row reduce + epilogue + LayerNorm/modulate. One workgroup per row.
// =============================================================================================

// One workgroup per (row, 1024-column block); each thread owns 4 consecutive columns (float4).
// The S partial slabs are summed in z order (deterministic) with 4 independent loads in flight.
__device__ __forceinline__ float act1(float x, int act) {
  return act == ACT_GELU ? gelu_tanh(x) : (act == ACT_SILU ? silu(x) : (act == ACT_ELU ? elu1(x) : x));
}

// Every load of a thread (its S slab float4s and the bias / gate / residual operands) is issued
// before the first add: one memory round trip. Absent operands are read from a valid stand-in
// address and dropped by a select (no branches around loads).
template <int SMAX>
__device__ __forceinline__ float4 rr_value(const RowReduceArgs& a, int m, int n) {
  const float* p = a.P + (long)m * a.N + n;
  const long zs = (long)a.M * a.N;
  float4 pz[SMAX];
#pragma unroll
  for (int z = 0; z < SMAX; ++z) pz[z] = *reinterpret_cast<const float4*>(p + (long)min(z, a.S - 1) * zs);
  const float4 bi = *reinterpret_cast<const float4*>((a.bias ? a.bias + n : p));
  const float4 ga = *reinterpret_cast<const float4*>((a.gate ? a.gate + (long)m * a.ldg + n : p));
  const float4 rr = *reinterpret_cast<const float4*>((a.R ? a.R + (long)m * a.ldr + n : p));
  float4 v = pz[0];
#pragma unroll
  for (int z = 1; z < SMAX; ++z)
    if (z < a.S) v = f4add(v, pz[z]);
  if (a.bias) v = f4add(v, bi);
  if (a.act != ACT_NONE) v = make_float4(act1(v.x, a.act), act1(v.y, a.act), act1(v.z, a.act), act1(v.w, a.act));
  if (a.gate) v = f4mul(v, ga);
  if (a.R) v = f4add(v, rr);
  return v;
}
// FlowHeadArgs::fhm float4 index of adaLN columns n .. n + 3 (n % 4 == 0) of row b of a batch of B
// rows at Euler step st, or -1 for a gate column: the columns are [shift | scale | gate] x 6
// ResBlocks, then [shift | scale] (final)
__device__ __forceinline__ long fhm_index(int st, int b, int B, int n) {
  const int RG = (B + 15) / 16;
  const int i = min(n / (3 * FH_D), FH_DEPTH), rem = n - i * 3 * FH_D;
  const int t = rem / FH_D, k = rem - t * FH_D;
  if (t >= 2) return -1;
  return (((((long)(st * RG + b / 16) * (FH_DEPTH + 1) + i) * 2 + t) * 8 + (k >> 6)) * 4 + ((k >> 4) & 3)) * 64 +
         (b & 15) + 16 * ((k >> 2) & 3);
}
__device__ __forceinline__ void rr_store(const RowReduceArgs& a, int m, int n, float4 v) {
  if (a.Y) *reinterpret_cast<float4*>(a.Y + (long)m * a.ldy + n) = v;
  if (a.fhm) {
    const int st = m / a.fhm_B;
    const long idx = fhm_index(st, m - st * a.fhm_B, a.fhm_B, n);
    if (idx >= 0) reinterpret_cast<float4*>(a.fhm)[idx] = v;
  }
  if (a.Y2) *reinterpret_cast<float4*>(a.Y2 + (long)m * a.ldy + n) = make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w));
  if (a.euler) {
    float4* e = reinterpret_cast<float4*>(a.euler + (long)m * 32 + n);
    const int nr = max(a.euler_st[m].lsd, 1);
    const float sc = 1.0f / (float)nr;
    const float4 c = *e;
    const float4 nx = make_float4(c.x + v.x * sc, c.y + v.y * sc, c.z + v.z * sc, c.w + v.w * sc);
    *e = a.euler_step < nr ? nx : c;  // a row past its own count keeps its latent
  }
}
// LayerNorm (+affine) (+modulate) of one row value quad, given the row mean and 1/den
__device__ __forceinline__ float4 rr_ln(const RowReduceArgs& a, int m, int n, float4 d, float den) {
  float4 hh = make_float4(d.x / den, d.y / den, d.z / den, d.w / den);
  if (a.ln_w)
    hh = f4add(f4mul(hh, *reinterpret_cast<const float4*>(a.ln_w + n)), *reinterpret_cast<const float4*>(a.ln_b + n));
  if (a.mshift) {
    const float4 sc = *reinterpret_cast<const float4*>(a.mscale + (long)m * a.ldm + n);
    const float4 sf = *reinterpret_cast<const float4*>(a.mshift + (long)m * a.ldm + n);
    hh = make_float4(hh.x * (1.0f + sc.x) + sf.x, hh.y * (1.0f + sc.y) + sf.y, hh.z * (1.0f + sc.z) + sf.z,
                     hh.w * (1.0f + sc.w) + sf.w);
  }
  return hh;
}

// Flow-head input projection of 4 columns n..n+3 of one row (cv: the row's 32 latent values),
// in one summation order for both of its callers (k_row_reduce's x0 side job, k_flow_head's
// later Euler steps); a NaN result is stored canonical (never the hand-off's empty pattern).
__device__ __forceinline__ float fh_dot4(float4 c, float4 w) { return (c.x * w.x + c.y * w.y) + (c.z * w.z + c.w * w.w); }
__device__ __forceinline__ float4 fh_inproj4(const float4 (&cv)[8], const float* in_w, const float* in_b, int n) {
  float acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float* w = in_w + (long)(n + q) * FH_L;
    float t = in_b[n + q];
#pragma unroll
    for (int j = 0; j < 8; ++j) t += fh_dot4(cv[j], *reinterpret_cast<const float4*>(w + 4 * j));
    acc[q] = t;
  }
  return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// x0 of Euler step 0 into hand-off region 0 ([RG][32][16][16] tiles; plain stores, read by the
// next launch), one output per thread i0, i0 + nthr, ...; the weight is read transposed (w_t
// [32][512], made at finalize) so each load instruction of a wave is one contiguous 256-B run
// column n of row b, whose 32 latent values are at c
__device__ __forceinline__ void fh_x0_one(const float* c, const float* w_t, const float* bias, float* hx, int b,
                                          int n) {
  float t = bias[n];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float4 cj = *reinterpret_cast<const float4*>(c + 4 * j);
    const float* w = w_t + (long)(4 * j) * FH_D + n;
    t += fh_dot4(cj, make_float4(w[0], w[FH_D], w[2 * FH_D], w[3 * FH_D]));
  }
  if (t != t) t = __uint_as_float(0x7FC00000u);  // never the hand-off's empty pattern
  hx[((long)((b >> 4) * 32 + (n >> 4))) * 256 + (b & 15) * 16 + (n & 15)] = t;
}
__device__ __forceinline__ void fh_x0_job(const float* cur, const float* w_t, const float* bias, float* hx, int B,
                                          long i0, long nthr) {
  for (long i = i0; i < (long)B * FH_D; i += nthr) {
    const int b = (int)(i / FH_D), n = (int)(i % FH_D);
    fh_x0_one(cur + (long)b * FH_L, w_t, bias, hx, b, n);
  }
}
__global__ void k_fh_x0(const float* cur, const float* w, const float* bias, float* hx, int B) {
  fh_x0_job(cur, w, bias, hx, B, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}
void flow_head_x0(const float* cur, const float* w_t, const float* bias, float* hx, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_fh_x0, dim3((B * FH_D + 255) / 256), dim3(256), 0, s, cur, w_t, bias, hx, B);
}

template <int SMAX>
__global__ __launch_bounds__(256) void k_row_reduce(RowReduceArgs a) {
  if (a.front) front_prio();
  __shared__ float sh[4];
  if (a.fill) {
    const long nthr = (long)gridDim.x * gridDim.y * 256;
    for (long i = ((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < a.fill_n4; i += nthr)
      reinterpret_cast<uint4*>(a.fill)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  }
  if (a.x0_hx)
    fh_x0_job(a.x0_cur, a.x0_w, a.x0_b, a.x0_hx, a.x0_B, ((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x,
              (long)gridDim.x * gridDim.y * 256);
  const int m = blockIdx.x;
  const int n0 = blockIdx.y * 1024 + 4 * threadIdx.x;
  const bool ok = n0 < a.N;
  const int n = ok ? n0 : 0;
  const float4 v = rr_value<SMAX>(a, m, n);
  if (ok) rr_store(a, m, n, v);
  if (!a.ln) return;  // LN rows are <= 1024 wide: gridDim.y == 1 (host-checked)
  const float s = ok ? (v.x + v.y) + (v.z + v.w) : 0.f;
  const float mean = block_sum(s, sh) / (float)a.N;
  const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
  const float q = ok ? (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w) : 0.f;
  const float den = sqrtf(block_sum(q, sh) / (float)a.N + a.eps);
  if (!ok) return;
  const float4 hv = rr_ln(a, m, n, d, den);
  *reinterpret_cast<float4*>(a.Hout + (long)m * a.ldh + n) = hv;
  if (a.Hfrag) *reinterpret_cast<float4*>(a.Hfrag + fk_afrag_index(m, n)) = hv;  // n % 4 == 0: one float4
}

// The same for the back part's 512-wide rows (Mimi d_model, SEANet conv0): FOUR rows per 512-thread
// workgroup, 128 threads per row, so a pass's 16 B rows fill the chip's one capped workgroup per
// CU in a single round instead of four (the one-row form left half of its 256 threads idle). A
// row's sums are its two waves' DPP sums, combined in LDS: the values, their order and every
// rounding are those of k_row_reduce (whose other two waves add zeros).
template <int SMAX>
__global__ __launch_bounds__(512) void k_row_reduce4(RowReduceArgs a) {
  if (a.front) front_prio();
  __shared__ float sh[2][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = tid >> 7;
  if (!a.ln) {  // no row statistics: elementwise over the 4 rows
    const int q = a.N >> 2;  // float4 per row
    for (int e = tid; e < 4 * q; e += 512) {
      const int mm = blockIdx.x * 4 + e / q, nn = 4 * (e % q);
      if (mm < a.M) rr_store(a, mm, nn, rr_value<SMAX>(a, mm, nn));
    }
    return;
  }
  const int m = blockIdx.x * 4 + r, n = 4 * (tid & 127);
  const bool ok = m < a.M;
  const float4 v = rr_value<SMAX>(a, ok ? m : a.M - 1, n);
  if (ok) rr_store(a, m, n, v);
  const float s = wave_sum(ok ? (v.x + v.y) + (v.z + v.w) : 0.f);
  if (lane == 0) sh[0][wave] = s;
  __syncthreads();
  const float mean = (sh[0][2 * r] + sh[0][2 * r + 1]) / 512.f;
  const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
  const float q = wave_sum(ok ? (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w) : 0.f);
  if (lane == 0) sh[1][wave] = q;
  __syncthreads();
  const float den = sqrtf((sh[1][2 * r] + sh[1][2 * r + 1]) / 512.f + a.eps);
  if (!ok) return;
  const float4 hv = rr_ln(a, m, n, d, den);
  *reinterpret_cast<float4*>(a.Hout + (long)m * a.ldh + n) = hv;
}

void row_reduce(const RowReduceArgs& a, hipStream_t s) {
  // (N = 512 only: the 2,048-wide reduce as 4 rows per workgroup, 4 float4 per thread, measured
  // slower than its one-row form, profiles/r04/row_reduce4_ab.txt)
  if (!a.front && a.N == 512 && !a.fill && !a.x0_hx && !a.fhm && !a.Hfrag && !rr4_off()) {
    const dim3 g4((a.M + 3) / 4);
    if (a.S <= 1) hipLaunchKernelGGL(k_row_reduce4<1>, g4, dim3(512), cap_lds(k_row_reduce4<1>, g_wg_cap), s, a);
    else if (a.S <= 2) hipLaunchKernelGGL(k_row_reduce4<2>, g4, dim3(512), cap_lds(k_row_reduce4<2>, g_wg_cap), s, a);
    else if (a.S <= 4) hipLaunchKernelGGL(k_row_reduce4<4>, g4, dim3(512), cap_lds(k_row_reduce4<4>, g_wg_cap), s, a);
    else if (a.S <= 8) hipLaunchKernelGGL(k_row_reduce4<8>, g4, dim3(512), cap_lds(k_row_reduce4<8>, g_wg_cap), s, a);
    else hipLaunchKernelGGL(k_row_reduce4<16>, g4, dim3(512), cap_lds(k_row_reduce4<16>, g_wg_cap), s, a);
    return;
  }
  dim3 grid(a.M, (a.N + 1023) / 1024);
  if (a.S <= 1) hipLaunchKernelGGL(k_row_reduce<1>, grid, dim3(256), cap_lds(k_row_reduce<1>, g_wg_cap), s, a);
  else if (a.S <= 2) hipLaunchKernelGGL(k_row_reduce<2>, grid, dim3(256), cap_lds(k_row_reduce<2>, g_wg_cap), s, a);
  else if (a.S <= 4) hipLaunchKernelGGL(k_row_reduce<4>, grid, dim3(256), cap_lds(k_row_reduce<4>, g_wg_cap), s, a);
  else if (a.S <= 8) hipLaunchKernelGGL(k_row_reduce<8>, grid, dim3(256), cap_lds(k_row_reduce<8>, g_wg_cap), s, a);
  else hipLaunchKernelGGL(k_row_reduce<16>, grid, dim3(256), cap_lds(k_row_reduce<16>, g_wg_cap), s, a);
}

// LayerNorm, one wave per row (N <= 1024, multiple of 64).
__global__ __launch_bounds__(256) void k_layernorm(const float* x, long ldx, float* y, long ldy, int M, int N,
                                                   const float* w, const float* b, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (long)row * ldx;
  float v[16];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = lane + 64 * i;
    v[i] = n < N ? xr[n] : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float d = v[i] - mean;
    q += (lane + 64 * i < N) ? d * d : 0.f;
  }
  const float den = sqrtf(wave_sum(q) / (float)N + eps);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = lane + 64 * i;
    if (n < N) y[(long)row * ldy + n] = (v[i] - mean) / den * w[n] + b[n];
  }
}
void layernorm(const float* x, long ldx, float* y, long ldy, int M, int N, const float* w, const float* b,
               float eps, hipStream_t s) {
  hipLaunchKernelGGL(k_layernorm, dim3((M + 3) / 4), dim3(256), cap_lds(k_layernorm, g_wg_cap), s, x, ldx, y, ldy, M, N, w, b, eps);
}

// =============================================================================================
// QKV (+ split-K reduce) -> RoPE -> KV append. One thread per (row, head, rotation pair).
// =============================================================================================

__global__ __launch_bounds__(256) void k_qkv_rope(const float* P, int S, const float* dense, int M, int nh,
                                                  RowMap mp, KvStore kv, float* Q) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int per_row = nh * 32;
  if (idx >= M * per_row) return;
  const int row = idx / per_row;
  const int rem = idx - row * per_row;
  const int hh = rem >> 5, i = rem & 31;
  const int d = nh * 64, ld = 3 * d;
  const int c = hh * 64 + 2 * i;
  float q0, q1, k0, k1, v0, v1;
  if (dense) {
    const float* pr = dense + (long)row * ld;
    q0 = pr[c]; q1 = pr[c + 1]; k0 = pr[d + c]; k1 = pr[d + c + 1]; v0 = pr[2 * d + c]; v1 = pr[2 * d + c + 1];
  } else {
    q0 = q1 = k0 = k1 = v0 = v1 = 0.f;
    for (int z = 0; z < S; ++z) {
      const float* pr = P + ((long)z * M + row) * ld;
      q0 += pr[c]; q1 += pr[c + 1]; k0 += pr[d + c]; k1 += pr[d + c + 1]; v0 += pr[2 * d + c]; v1 += pr[2 * d + c + 1];
    }
  }
  int slot, pos;
  row_slot_pos(mp, row, slot, pos);
  // rope.rs:9-16 inv_freq = exp(-ln(max_period) * 2i / head_dim); ts = offset + t
  const float freq = expf((float)i * (-logf(10000.0f) * 2.0f / 64.0f));
  const float ang = (float)pos * freq;
  const float cs = cosf(ang), sn = sinf(ang);
  const long qr = mp.qrow ? mp.qrow[row] : row;  // compact admission: the query's padded row
  Q[qr * d + c] = q0 * cs - q1 * sn;
  Q[qr * d + c + 1] = q0 * sn + q1 * cs;
  if (slot < 0) return;  // padding row of a batched admission
  float* kb = kv.base + (long)slot * kv.slot_stride + ((long)hh * kv.cap + (pos % kv.cap)) * 64 + 2 * i;
  float* vb = kv.base + (long)slot * kv.slot_stride + ((long)(nh + hh) * kv.cap + (pos % kv.cap)) * 64 + 2 * i;
  kb[0] = k0 * cs - k1 * sn;
  kb[1] = k0 * sn + k1 * cs;
  vb[0] = v0;
  vb[1] = v1;
}

void qkv_rope_append(const float* P, int S, const float* dense, int M, int nh, RowMap map, KvStore kv, float* Q,
                     hipStream_t s) {
  const int total = M * nh * 32;
  hipLaunchKernelGGL(k_qkv_rope, dim3((total + 255) / 256), dim3(256), cap_lds(k_qkv_rope, g_wg_cap), s, P, S, dense, M, nh, map, kv, Q);
}

// =============================================================================================
// Attention. Mask (sdpa.rs:128-171): key kp visible to query qp iff kp <= qp and (no window or
// qp-kp < window).
// =============================================================================================
// ---------------------------------------------------------------------------------------------
// 16-query attention on MFMA (Mimi decoder ring window: 16 upsampled positions per row, and the
// prefill / encoder groups): one workgroup per (16 consecutive rows of one slot, head), 16-key
// tiles dealt to 8 waves, online softmax per wave, waves merged through LDS.
// v_mfma_f32_16x16x4_f32 fragments (lane l, c = l & 15, G = l >> 4):
//   A[i][k] lane i + 16k, B[k][j] lane j + 16k, D reg g -> row 4G + g, col c.
// S^T = K Q^T: A = K (key c, dims 16G+s at step s), B = Q^T (query c, same dims) -> lane holds
// S[query c][key 4G+g]. O += P V: A = P (query c, key 4G+s at step s: the lane's own S^T regs,
// no transpose), B = V (key 4G+s, dim 4c+dt for output tile dt: one float4 per key) -> lane holds
// O[query 4G+g][dim 4c+dt]. The dot-product / key order permutations only reorder sums.
// ---------------------------------------------------------------------------------------------
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int A16_WAVES = 8;

// rope.rs:9-16: inv_freq = exp(-ln(max_period) * 2i / head_dim), angle = position * inv_freq
// (the same expressions as k_qkv_rope, so both paths rotate identically)
__device__ __forceinline__ void rope_cs(int pos, int i, float& cs, float& sn) {
  const float freq = expf((float)i * (-logf(10000.0f) * 2.0f / 64.0f));
  const float ang = (float)pos * freq;
  cs = cosf(ang);
  sn = sinf(ang);
}

// FUSE: Q is the dense QKV projection [M][3d] (Mimi decoder step) instead of rotated queries:
// the workgroup rotates its 16 rows' q and k (RoPE), appends k and v at their positions in the
// ring, and attends over the ring after a workgroup barrier (replaces the k_qkv_rope launch; the
// ring holds window + 16 positions, so the appended rows never evict a key inside the window).
template <bool RING, bool FUSE = false>
__global__ __launch_bounds__(64 * A16_WAVES) void k_attn16(const float* __restrict__ Q, int M, int nh, RowMap mp,
                                                          KvStore kv, int window, float* __restrict__ O) {
  __shared__ float s_m[A16_WAVES][16], s_l[A16_WAVES][16];
  __shared__ float s_o[A16_WAVES][16][65];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, G = lane >> 4;
  const int row0 = blockIdx.x * 16, head = blockIdx.y;
  int nrows = min(16, M - row0);
  if (mp.tab) {  // a slot's rows come first in its 16-row groups, padding rows after them
    int n = 0;
    for (int i = 0; i < nrows; ++i) n += mp.tab[row0 + i] >= 0;
    nrows = n;
  }
  if (nrows <= 0) return;  // whole group of padding (uniform over the workgroup)
  int slot, qpos0;
  row_slot_pos(mp, row0, slot, qpos0);
  const int kmax = qpos0 + nrows - 1;
  const int kmin = window > 0 ? max(0, qpos0 - window + 1) : 0;
  const int d = nh * 64;
  const KvHead kh = kv_head(kv, slot, nh, head);
  const float* kbase = kh.kb;
  const float* vbase = kh.vb;
  const int cmask = kv.cap - 1;
  auto kidx = [&](int kp) { return RING ? (kp & cmask) : kp; };
  // FlowLM prefill: keys below F come from the shared voice prefix (never in a wrapped ring)
  auto kaddr = [&](int kp) { return (FUSE || kp >= kh.F ? kbase + (long)kidx(kp) * 64 : kh.pk + (long)kp * 64); };
  auto vaddr = [&](int kp) { return (FUSE || kp >= kh.F ? vbase + (long)kidx(kp) * 64 : kh.pv + (long)kp * 64); };
  const int ntiles = (kmax - kmin + 16) / 16;
  float4 kf[4], vf[4];
  auto load = [&](int t) {
    const int kt = kmin + 16 * t;
    const float4* kr = reinterpret_cast<const float4*>(kaddr(min(kt + c, kmax)) + 16 * G);
#pragma unroll
    for (int i = 0; i < 4; ++i) kf[i] = kr[i];
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx)
      vf[sidx] = *reinterpret_cast<const float4*>(vaddr(min(kt + 4 * G + sidx, kmax)) + 4 * c);
  };
  // a wave whose first key tile holds only keys older than this step's appended rows issues its
  // loads now, so their latency overlaps the append below (the append never evicts a key of the
  // window: the ring holds window + 16 positions)
  const bool early = FUSE && wave < ntiles && kmin + 16 * wave + 15 < qpos0;
  if (early) load(wave);
  // Q^T fragment: query c (rows past nrows reuse the last row; never stored), dims 16G..16G+15
  float qf[16];
  if (FUSE) {
    const int ld = 3 * d;
    {  // append: thread (row r, rotation pair i) of the 16 x 32 (A16_WAVES = 8: 512 threads)
      const int r = threadIdx.x >> 5, i = threadIdx.x & 31;
      if (r < nrows) {
        const float* pr = Q + (long)(row0 + r) * ld + head * 64 + 2 * i;
        const float k0 = pr[d], k1 = pr[d + 1], v0 = pr[2 * d], v1 = pr[2 * d + 1];
        float cs, sn;
        rope_cs(qpos0 + r, i, cs, sn);
        float* kb = kv.base + (long)slot * kv.slot_stride + ((long)head * kv.cap + kidx(qpos0 + r)) * 64 + 2 * i;
        float* vb = kv.base + (long)slot * kv.slot_stride + ((long)(nh + head) * kv.cap + kidx(qpos0 + r)) * 64 + 2 * i;
        *reinterpret_cast<float2*>(kb) = make_float2(k0 * cs - k1 * sn, k0 * sn + k1 * cs);
        *reinterpret_cast<float2*>(vb) = make_float2(v0, v1);
      }
    }
    const int rq = min(c, nrows - 1);
    const float4* q4 = reinterpret_cast<const float4*>(Q + (long)(row0 + rq) * ld + head * 64 + 16 * G);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 t = q4[i];
      float cs, sn;
      rope_cs(qpos0 + rq, 8 * G + 2 * i, cs, sn);
      qf[4 * i] = t.x * cs - t.y * sn;
      qf[4 * i + 1] = t.x * sn + t.y * cs;
      rope_cs(qpos0 + rq, 8 * G + 2 * i + 1, cs, sn);
      qf[4 * i + 2] = t.z * cs - t.w * sn;
      qf[4 * i + 3] = t.z * sn + t.w * cs;
    }
    __syncthreads();  // the appended keys / values are read back by every wave below
  } else {
    const float4* q4 = reinterpret_cast<const float4*>(Q + (long)(row0 + min(c, nrows - 1)) * d + head * 64 + 16 * G);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 t = q4[i];
      qf[4 * i] = t.x; qf[4 * i + 1] = t.y; qf[4 * i + 2] = t.z; qf[4 * i + 3] = t.w;
    }
  }
  const int qp = qpos0 + c;  // this lane's query position (softmax side)
  float m = -INFINITY, l = 0.f;
  floatx4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (wave < ntiles && !early) load(wave);
  for (int t = wave; t < ntiles; t += A16_WAVES) {
    const int kt = kmin + 16 * t;
    float ka[16];
    float4 vc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ka[4 * i] = kf[i].x; ka[4 * i + 1] = kf[i].y; ka[4 * i + 2] = kf[i].z; ka[4 * i + 3] = kf[i].w;
      vc[i] = vf[i];
    }
    if (t + A16_WAVES < ntiles) load(t + A16_WAVES);  // next tile in flight during this one
    floatx4 st = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sidx = 0; sidx < 16; ++sidx) st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[sidx], qf[sidx], st, 0, 0, 0);
    float sc[4];
    float mt = -INFINITY;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kp = kt + 4 * G + g;
      const bool ok = kp <= kmax && kp <= qp && (window <= 0 || qp - kp < window);
      sc[g] = ok ? st[g] * 0.125f : -INFINITY;  // 1/sqrt(64) (attention.rs:191,229)
      mt = fmaxf(mt, sc[g]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float alpha = mn == -INFINITY ? 1.f : expf(m - mn);
    float p[4], ps = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      p[g] = sc[g] == -INFINITY ? 0.f : expf(sc[g] - mn);
      ps += p[g];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    // O rows are queries 4G+g: their rescale factors live in lanes 4G+g
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float a = __shfl(alpha, 4 * G + g, 64);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt][g] *= a;
    }
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[sidx], vc[sidx].x, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[sidx], vc[sidx].y, o[1], 0, 0, 0);
      o[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[sidx], vc[sidx].z, o[2], 0, 0, 0);
      o[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[sidx], vc[sidx].w, o[3], 0, 0, 0);
    }
  }
  if (G == 0) {
    s_m[wave][c] = m;
    s_l[wave][c] = l;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) s_o[wave][4 * G + g][4 * c + dt] = o[dt][g];
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * 64; e += 64 * A16_WAVES) {
    const int qi = e >> 6, dd = e & 63;
    if (qi >= nrows) continue;
    float M_ = -INFINITY;
#pragma unroll
    for (int w = 0; w < A16_WAVES; ++w) M_ = fmaxf(M_, s_m[w][qi]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < A16_WAVES; ++w) {
      const float ew = s_m[w][qi] == -INFINITY ? 0.f : expf(s_m[w][qi] - M_);
      num += s_o[w][qi][dd] * ew;
      den += s_l[w][qi] * ew;
    }
    const int orow = mp.orow ? mp.orow[row0 + qi] : row0 + qi;  // compact admission: the token's row
    if (orow >= 0) O[(long)orow * d + head * 64 + dd] = num / den;
  }
}

// ---------------------------------------------------------------------------------------------
// FlowLM step attention with the QKV split-K sum, RoPE and KV append fused in front (one launch
// instead of qkv_rope_append + a decode attention for the one-query-per-row step): the workgroup of (row, head)
// sums its 192 q|k|v columns over the S slabs, rotates q and k (rope.rs:18-60), appends k, v at
// the row's position and attends over the cached keys 0..pos-1 plus the new key from LDS.
// ---------------------------------------------------------------------------------------------

// Decode attention of the FlowLM step fused with the QKV slab sum, RoPE and KV append
// (attention.rs:104-283 with the single-query mask skip of sdpa.rs:3-18). One 256-thread
// workgroup per (row, head); the cached keys are dealt to the 4 waves 64 at a time.
// A 64-key block of K (and of V) is 16 KB contiguous, read with 16 fully coalesced 1-KB wave
// loads: load i gives lane l the 4 dims 4(l%16).. of key 4i + l/16. Scores: a 4-term dot with
// the matching q dims, summed over the 16-lane row with DPP, so lane l holds the score of key
// 4i + l/16 - exactly the key whose V dims it holds from V load i, so P.V needs no broadcast.
// The rows (l/16) are combined once per wave at the end. Each wave issues its first block's
// loads before the QKV/RoPE phase: the cached keys do not depend on this step's token.
// Load order: after the kernel arguments, one scalar level (the row's position, its prefix length
// and prefix pointer, read unconditionally from stand-in addresses where a table is absent) and
// one vector level (the wave's first key block, the QKV slabs and the RoPE row, all requested
// before the first wait); the only further levels are the next key blocks. SMAX: the slab count
// the fixed-trip slab loop is unrolled to (S <= SMAX).
template <int NW, int KQ, bool NT = false, int SMAX = 16, bool PRE = true>
__global__ __launch_bounds__(64 * NW) void k_attn_decode_qkv(const float* __restrict__ P, int S, int M, int nh, RowMap mp,
                                                         KvStore kv, const float* __restrict__ rope,
                                                         float* __restrict__ O) {
  front_prio();
  constexpr int BLK = 4 * KQ * NW;  // keys per round: NW waves x KQ loads of 4 keys
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) f4v* gf4p;  // global address space: no flat loads
  __shared__ float s_m[NW], s_l[NW];
  __shared__ __attribute__((aligned(16))) float s_o[NW][64];
  __shared__ __attribute__((aligned(16))) float s_qkv[3][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c4 = (lane & 15) * 4;  // key row within a load, first of my 4 dims
  const int row = blockIdx.x, head = blockIdx.y;
  // every kernel argument in scalar registers here: one argument load level (left alone, the
  // compiler reads the segment piecemeal, a few fields behind each branch)
  asm volatile("" ::"s"(P), "s"(S), "s"(M), "s"(nh), "s"(mp.slot0), "s"(mp.rps), "s"(mp.p0), "s"(mp.pos_arr),
               "s"(mp.tab), "s"(kv.base), "s"(kv.slot_stride), "s"(kv.cap), "s"(kv.pre), "s"(kv.pre_len),
               "s"(kv.layer), "s"(rope), "s"(O));
  // PRE: the launch has prefix tables (kv.pre != nullptr, the launcher's choice of instance)
  int slot, qp, F = 0;
  const float* pre = nullptr;
  if (mp.tab) {  // table form (not a step launch of the engine): the slot itself is a table entry
    row_slot_pos(mp, row, slot, qp);
    if (PRE && slot >= 0) {
      F = kv.pre_len[slot];
      pre = kv.pre[slot];
    }
  } else {  // uniform form: the table entries in one scalar level
    const int sr = __builtin_amdgcn_readfirstlane(row / mp.rps);
    slot = mp.slot0 + sr;
    // read through the constant address space: scalar loads (nothing in this launch writes the
    // tables; behind the argument pin the compiler would no longer prove that and go through
    // the vector memory path, a wait per entry)
    typedef const __attribute__((address_space(4))) int* cip;
    typedef const float* cfp;
    const int* none = reinterpret_cast<const int*>(P);  // stand-in where the table is absent
    const int pa = *(cip)(mp.pos_arr ? mp.pos_arr + slot : none);
    if (PRE) {
      F = *(cip)(kv.pre_len + slot);
      pre = *(const __attribute__((address_space(4))) cfp*)(kv.pre + slot);
    }
    qp = (mp.pos_arr ? pa : mp.p0) + (row - sr * mp.rps);
  }
  F = max(F, 0);
  // a finished row is still stepped (its frame is discarded): once it has filled the cache
  // (qp == cap) its key/value must not be appended, or position cap would spill into the next
  // head's (or, for the slot's last head, the next slot's) position 0
  const bool append = qp < kv.cap;
  qp = min(qp, kv.cap - 1);
  const int d = nh * 64, ld = 3 * d;
  float* kbase = kv.base + (long)slot * kv.slot_stride + (long)head * kv.cap * 64;
  float* vbase = kv.base + (long)slot * kv.slot_stride + (long)(nh + head) * kv.cap * 64;
  // positions < F live in the voice's rows (KvStore::pre); addresses as integers, so that the
  // per-element choice between the two bases stays one global load
  const uintptr_t kb_a = reinterpret_cast<uintptr_t>(kbase), vb_a = reinterpret_cast<uintptr_t>(vbase);
  const uintptr_t pk_a =
      F > 0 ? reinterpret_cast<uintptr_t>(pre + ((long)kv.layer * 2 * nh + head) * F * 64) : kb_a;
  const uintptr_t pv_a = F > 0 ? pk_a + (uintptr_t)((long)nh * F * 64) * sizeof(float) : vb_a;
  const int last = qp - 1;
  float4 k[KQ], v[KQ];
  // (Part of) a block in the shared voice prefix: cached loads, since every row of the voice reads
  // these lines. The row's own blocks are read once per step: non-temporal. max(.., 0): a wave
  // without keys yet (qp <= base) still requests position 0 of its rows and drops the values (no
  // branch around the first block's loads).
  auto load_cached = [&](int base) {
#pragma unroll
    for (int i = 0; i < KQ; ++i) {
      const int j = max(min(base + 4 * i + g, last), 0);
      const uintptr_t off = (uintptr_t)((long)j * 64 + c4) * sizeof(float);
      const f4v kk = *(gf4p)((j < F ? pk_a : kb_a) + off), vv = *(gf4p)((j < F ? pv_a : vb_a) + off);
      k[i] = make_float4(kk.x, kk.y, kk.z, kk.w);
      v[i] = make_float4(vv.x, vv.y, vv.z, vv.w);
    }
  };
  auto load_own = [&](int base) {
#pragma unroll
    for (int i = 0; i < KQ; ++i) {
      const uintptr_t off = (uintptr_t)((long)max(min(base + 4 * i + g, last), 0) * 64 + c4) * sizeof(float);
      const f4v kk = __builtin_nontemporal_load((gf4p)(kb_a + off));
      const f4v vv = __builtin_nontemporal_load((gf4p)(vb_a + off));
      k[i] = make_float4(kk.x, kk.y, kk.z, kk.w);
      v[i] = make_float4(vv.x, vv.y, vv.z, vv.w);
    }
  };
  auto load_none = [&]() {  // probe builds: front_skip bit 2
#pragma unroll
    for (int i = 0; i < KQ; ++i) k[i] = v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  // The first block's policy is the launch's, not the block's: a branch between two sets of loads
  // into the same registers makes the compiler wait for the one before issuing the other (the
  // never-taken edge between the arms). With prefix tables (PRE) the first blocks lie in the
  // prefix for all but short prefixes: cached; without them they are the row's own: non-temporal.
  int base = 4 * KQ * wave;
  if (front_skip() & 4) load_none();
  else if (PRE || !NT) load_cached(base);
  else load_own(base);
  auto load_block = [&](int base) {  // later blocks: the policy per block (wave-uniform branch)
    if (front_skip() & 4) load_none();
    else if (!NT || base < F) load_cached(base);
    else load_own(base);
  };
  // q | k | v column of this head (waves 0-2; wave 3 requests v's again and drops it): the slabs,
  // clamped to the last one, and this position's RoPE pair (table of rope_table()), all in the
  // level of the key block
  const int part = min(tid >> 6, 2);
  const float* pr = P + (long)row * ld + part * d + head * 64 + lane;
  const long zs = (long)M * ld;
  float pz[SMAX];
#pragma unroll
  for (int z = 0; z < SMAX; ++z) pz[z] = pr[(long)max(min(z, S - 1), 0) * zs];
  const float2 cssn = *reinterpret_cast<const float2*>(rope + (long)qp * 64 + 2 * (tid & 31));
  __builtin_amdgcn_sched_barrier(0);
  float qs = 0.f;  // summed over the slabs in z order (by every wave: a branch around the adds
                   // would take the loads with it, behind the barrier above)
#pragma unroll
  for (int z = 0; z < SMAX; ++z) qs = z < S ? qs + pz[z] : qs;
  if (tid < 192) s_qkv[part][lane] = qs;
  __syncthreads();
  if (tid < 64) {  // rotate the (2i, 2i+1) pairs of q (tid < 32) and k (tid >= 32)
    const int i = tid & 31, part = tid >> 5;
    const float cs = cssn.x, sn = cssn.y;
    const float x0 = s_qkv[part][2 * i], x1 = s_qkv[part][2 * i + 1];
    // Spelled as the fused form k_qkv_rope compiles to (one product rounded, the other fused), so
    // that a key rotates to the same bits whichever kernel appends it; left to the compiler, y1 fused
    // the other product here and odd dims came out an ulp apart (tests/test_gpu_attention_core.py).
    // One wave: all reads precede the writes.
    const float y0 = fmaf(x0, cs, -(x1 * sn)), y1 = fmaf(x1, cs, x0 * sn);
    s_qkv[part][2 * i] = y0;
    s_qkv[part][2 * i + 1] = y1;
    if (part == 1 && append) {
      kbase[(long)qp * 64 + 2 * i] = y0;
      kbase[(long)qp * 64 + 2 * i + 1] = y1;
    }
  } else if (tid < 128 && append) {
    vbase[(long)qp * 64 + lane] = s_qkv[2][lane];
  }
  __syncthreads();
  const float4 q = *reinterpret_cast<const float4*>(&s_qkv[0][c4]);
  float m = -INFINITY, l = 0.f;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  for (; base < qp; base += BLK) {  // cached keys 0 .. qp-1, block `base` already in registers
    float sc[KQ];
    float bm = -INFINITY;
#pragma unroll
    for (int i = 0; i < KQ; ++i) {
      const float part = q.x * k[i].x + q.y * k[i].y + q.z * k[i].z + q.w * k[i].w;
      const float t = row16_sum(part) * 0.125f;  // 1/sqrt(64) (attention.rs:191,229)
      sc[i] = base + 4 * i + g <= last ? t : -INFINITY;
      bm = fmaxf(bm, sc[i]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);
    const float alpha = expf(m - mn);
    float ps = 0.f;
    o.x *= alpha; o.y *= alpha; o.z *= alpha; o.w *= alpha;
#pragma unroll
    for (int i = 0; i < KQ; ++i) {
      const float p = expf(sc[i] - mn);  // 0 for masked keys
      ps += p;
      o.x += p * v[i].x; o.y += p * v[i].y; o.z += p * v[i].z; o.w += p * v[i].w;
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    if (base + BLK < qp) load_block(base + BLK);
  }
  // combine the 4 key rows (lanes l, l^16, l^32, l^48 hold the same dims)
  o.x += __shfl_xor(o.x, 16, 64); o.y += __shfl_xor(o.y, 16, 64);
  o.z += __shfl_xor(o.z, 16, 64); o.w += __shfl_xor(o.w, 16, 64);
  o.x += __shfl_xor(o.x, 32, 64); o.y += __shfl_xor(o.y, 32, 64);
  o.z += __shfl_xor(o.z, 32, 64); o.w += __shfl_xor(o.w, 32, 64);
  if (wave == 0) {  // the new key (position qp) from LDS
    const float sc = wave_sum(s_qkv[0][lane] * s_qkv[1][lane]) * 0.125f;
    const float mn = fmaxf(m, sc);
    const float alpha = expf(m - mn);
    const float p = expf(sc - mn);
    l = l * alpha + p;
    const float4 vn = *reinterpret_cast<const float4*>(&s_qkv[2][c4]);
    o.x = o.x * alpha + p * vn.x; o.y = o.y * alpha + p * vn.y;
    o.z = o.z * alpha + p * vn.z; o.w = o.w * alpha + p * vn.w;
    m = mn;
  }
  if (lane == 0) {
    s_m[wave] = m;
    s_l[wave] = l;
  }
  if (lane < 16) *reinterpret_cast<float4*>(&s_o[wave][c4]) = o;
  __syncthreads();
  if (wave == 0) {
    float Mx = s_m[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) Mx = fmaxf(Mx, s_m[w]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float e = s_m[w] == -INFINITY ? 0.f : expf(s_m[w] - Mx);
      num += s_o[w][lane] * e;
      den += s_l[w] * e;
    }
    O[(long)row * d + head * 64 + lane] = num / den;
  }
}

void attention_step_qkv(const float* P, int S, int M, int nh, RowMap map, KvStore kv, const float* rope, float* O,
                        hipStream_t s) {
  // 4 waves x 32 keys (128 keys per round; 116 VGPRs with prefix tables, 102 without, from the
  // code object's .vgpr_count; 158 before the load order of DESIGN section 25): in the pipelined
  // step the front part's attention shares each CU with a back-part workgroup, and this register
  // budget keeps two of its workgroups resident beside it. Steady step 0.690 -> 0.673 ms against 4 x 64 keys
  // (238 VGPRs, faster alone); 8 x 32, 4 x 48, 4 x 16, 2 x 64, 8 x 48 measured in between
  // (tools/sweep_env.sh). KV blocks are read once per step: non-temporal loads (-1.1 % step).
  if (S < 0 || S > 16) throw std::runtime_error("attention_step_qkv: 0 to 16 slabs");
  // instances: the slab loop's trip count (the step's QKV GEMM writes 8 slabs) x prefix tables
  const dim3 grid(M, nh), block(256);
  if (S <= 8 && kv.pre)
    hipLaunchKernelGGL((k_attn_decode_qkv<4, 8, true, 8, true>), grid, block, 0, s, P, S, M, nh, map, kv, rope, O);
  else if (S <= 8)
    hipLaunchKernelGGL((k_attn_decode_qkv<4, 8, true, 8, false>), grid, block, 0, s, P, S, M, nh, map, kv, rope, O);
  else if (kv.pre)
    hipLaunchKernelGGL((k_attn_decode_qkv<4, 8, true, 16, true>), grid, block, 0, s, P, S, M, nh, map, kv, rope, O);
  else
    hipLaunchKernelGGL((k_attn_decode_qkv<4, 8, true, 16, false>), grid, block, 0, s, P, S, M, nh, map, kv, rope, O);
}

__global__ __launch_bounds__(256) void k_rope_table(float* tab, int npos) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)npos * 32) return;
  const int pos = (int)(idx >> 5), i = (int)(idx & 31);
  const float freq = expf((float)i * (-logf(10000.0f) * 2.0f / 64.0f));
  const float ang = (float)pos * freq;
  tab[(long)pos * 64 + 2 * i] = cosf(ang);
  tab[(long)pos * 64 + 2 * i + 1] = sinf(ang);
}

void rope_table(float* tab, int npos, hipStream_t s) {
  hipLaunchKernelGGL(k_rope_table, dim3((unsigned)((npos * 32L + 255) / 256)), dim3(256), 0, s, tab, npos);
}

// ---------------------------------------------------------------------------------------------
// Word alignment: the step query's softmax over the row's text keys, for
// one layer, as a launch of its own behind that layer's step attention. One 256-thread workgroup
// per row; the selected heads are dealt to the 4 waves in rounds (the i-th selected head goes to
// wave i % 4 in round i / 4). A wave forms q_h as k_attn_decode_qkv does (slab sum in z order from
// 0, the fmaf RoPE form), reads its head's n keys with the same 1-KB wave loads (load i: lane l
// holds dims 4 (l % 16) .. of key 4 i + l / 16), and leaves the head's softmax row in LDS; the
// heads are then averaged in ascending head order. All loads are ordinary cached loads: the text
// keys are read again by this launch at every step of the utterance (and the slabs and the RoPE
// row were read by the attention launch right before), so the lines are wanted in L2.
// Every address is formed from clamped indices: an entry that does not fit the store counts 0.
// ---------------------------------------------------------------------------------------------
template <int SMAX>
__global__ __launch_bounds__(256) void k_align(AlignArgs a) {
  front_prio();
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) f4v* gf4p;
  __shared__ float s_sc[4][ALIGN_TOKENS];
  __shared__ float s_p[16][ALIGN_TOKENS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c4 = (lane & 15) * 4;
  const int row = blockIdx.x;
  const AlignEntry en = a.tab[row];
  const int cap = a.kv.cap, n = en.n, t0 = en.t0;
  float* orow = a.out + (long)row * ALIGN_ROW;
  if (n <= 0 || n > ALIGN_TOKENS || t0 < 0 || t0 > cap - n) {  // not in the stage (uniform)
    if (tid == 0) *reinterpret_cast<int*>(orow) = 0;
    return;
  }
  const unsigned mask = a.head_mask & (a.nh >= 32 ? ~0u : (1u << a.nh) - 1u);
  const int nsel = __popc(mask);
  const int qp = min(max(a.pos[row], 0), cap - 1);
  const int d = a.nh * 64, ld = 3 * d;
  const long zs = (long)a.M * ld;
  const float2 cssn = *reinterpret_cast<const float2*>(a.rope + (long)qp * 64 + 2 * (lane >> 1));
  for (int r0 = 0; r0 < nsel; r0 += 4) {
    const int idx = r0 + wave;  // this wave's head: the idx-th set bit of the mask
    int head = -1;
    {
      unsigned m = mask;
      for (int i = 0; i < idx && m; ++i) m &= m - 1;
      if (idx < nsel) head = __builtin_ctz(m);
    }
    if (head >= 0) {  // wave-uniform
      const float* pr = a.P + (long)row * ld + head * 64 + lane;
      float pz[SMAX];
#pragma unroll
      for (int z = 0; z < SMAX; ++z) pz[z] = pr[(long)max(min(z, a.S - 1), 0) * zs];
      float qs = 0.f;
#pragma unroll
      for (int z = 0; z < SMAX; ++z) qs = z < a.S ? qs + pz[z] : qs;
      // RoPE of the pair (2i, 2i+1), one dim per lane: y0 = fma(x0, c, -(x1 s)), y1 = fma(x1, c, x0 s)
      const float xo = __shfl_xor(qs, 1, 64);
      const float t = __fmul_rn(xo, cssn.y);
      const float qr = __fmaf_rn(qs, cssn.x, (lane & 1) ? t : -t);
      const float4 q = make_float4(__shfl(qr, c4, 64), __shfl(qr, c4 + 1, 64), __shfl(qr, c4 + 2, 64),
                                   __shfl(qr, c4 + 3, 64));
      const uintptr_t kb = reinterpret_cast<uintptr_t>(a.kv.base + (long)row * a.kv.slot_stride +
                                                       (long)head * cap * 64 + (long)t0 * 64);
      for (int base = 0; base < n; base += 32) {
        f4v k[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int j = min(base + 4 * i + g, n - 1);
          k[i] = *(gf4p)(kb + (uintptr_t)((long)j * 64 + c4) * sizeof(float));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float part = q.x * k[i].x + q.y * k[i].y + q.z * k[i].z + q.w * k[i].w;
          const float sc = row16_sum(part) * 0.125f;
          if ((lane & 15) == 0) s_sc[wave][base + 4 * i + g] = sc;  // base + 4 i + g < ALIGN_TOKENS
        }
      }
    }
    __syncthreads();
    if (head >= 0) {
      const float v0 = lane < n ? s_sc[wave][lane] : -INFINITY;
      const float v1 = lane + 64 < n ? s_sc[wave][lane + 64] : -INFINITY;
      const float mx = wave_max(fmaxf(v0, v1));  // n >= 1: finite
      const float e0 = lane < n ? expf(v0 - mx) : 0.f, e1 = lane + 64 < n ? expf(v1 - mx) : 0.f;
      const float sum = wave_sum(e0 + e1);
      s_p[head][lane] = e0 / sum;
      s_p[head][lane + 64] = e1 / sum;
    }
    __syncthreads();
  }
  if (tid < ALIGN_TOKENS) {
    float acc = 0.f;
    for (unsigned m = mask; m; m &= m - 1) acc += s_p[__builtin_ctz(m)][tid];  // ascending head order
    orow[1 + tid] = tid < n ? acc / (float)nsel : 0.f;
  }
  if (tid == 0) *reinterpret_cast<int*>(orow) = n;
}

void align_step(const AlignArgs& a, hipStream_t s) {
  if (a.S < 1 || a.S > 16) throw std::runtime_error("align_step: 1 to 16 slabs");
  if (a.M < 1 || a.nh < 1 || a.nh > 16 || !(a.head_mask & ((1u << a.nh) - 1u)))
    throw std::runtime_error("align_step: no row, or no head of the mask among the layer's");
  if (a.S <= 8) hipLaunchKernelGGL(k_align<8>, dim3(a.M), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_align<16>, dim3(a.M), dim3(256), 0, s, a);
}

void attention16_qkv(const float* qkv, int M, int nh, RowMap map, KvStore kv, int window, float* O, hipStream_t s) {
  if (map.tab != nullptr || map.rps != 16) throw std::runtime_error("attention16_qkv: needs 16 rows per slot");
  if ((kv.cap & (kv.cap - 1)) != 0 || kv.cap < window + 16)
    throw std::runtime_error("attention16_qkv: ring too small for the fused append");
  const dim3 grid((M + 15) / 16, nh);
  hipLaunchKernelGGL((k_attn16<true, true>), grid, dim3(64 * A16_WAVES), cap_lds(k_attn16<true, true>, g_wg_cap), s,
                     qkv, M, nh, map, kv, window, O);
}

void attention(const float* Q, int M, int nh, RowMap map, KvStore kv, int window, float* O, hipStream_t s) {
  if (kv.pre != nullptr && window > 0)
    throw std::runtime_error("attention: shared voice prefixes need the 16-row causal kernel");
  // 16-row groups never straddle slots (rows-per-slot is 16 or the whole group)
  const dim3 grid((M + 15) / 16, nh);
  if ((kv.cap & (kv.cap - 1)) == 0)
    hipLaunchKernelGGL(k_attn16<true>, grid, dim3(64 * A16_WAVES), cap_lds(k_attn16<true>, g_wg_cap), s, Q, M, nh, map, kv, window, O);
  else
    hipLaunchKernelGGL(k_attn16<false>, grid, dim3(64 * A16_WAVES), cap_lds(k_attn16<false>, g_wg_cap), s, Q, M, nh, map, kv, window, O);
}

// =============================================================================================
// Flow head prologue: cond_embed | out_eos reduce, EOS bookkeeping, adaLN inputs, x0 noise.
// =============================================================================================
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Standard normal for (seed, step, k, attempt): Box-Muller over two 24-bit uniforms.
__device__ float normal_at(unsigned long long seed, int step, int k, int attempt) {
  const unsigned long long base =
      mix64(seed * 0x9E3779B97F4A7C15ull + (unsigned long long)step * 0xD1B54A32D192ED03ull +
            (unsigned long long)(k * 64 + attempt) * 0x8CB92BA72F3D8DD7ull);
  const float u1 = ((float)(base >> 41) + 0.5f) * (1.0f / 8388608.0f);  // (0,1), exact in fp32
  const float u2 = (float)(mix64(base ^ 0x5851F42D4C957F2Dull) >> 40) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// element k of a row's x0 noise: N(0, sqrt(temp)), optionally truncated to |x| <= clamp
// (flow_lm.rs:39-65); 0 at temp 0
__device__ __forceinline__ float flow_noise(float temp, float clamp, unsigned long long seed, int step, int k) {
  float x0 = 0.f;
  if (temp > 0.f) {
    const float sd = sqrtf(temp);
    x0 = sd * normal_at(seed, step, k, 0);
    if (clamp > 0.f) {
      int att = 1;
      while (fabsf(x0) > clamp && att < 64) x0 = sd * normal_at(seed, step, k, att++);
      x0 = fminf(fmaxf(x0, -clamp), clamp);
    }
  }
  return x0;
}

__global__ __launch_bounds__(256) void k_flow_cond(const float* P, int S, int B, const float* bias, const float* temb,
                                                   int lsd, int lsd_cap, const SlotState* st, float* ysilu,
                                                   float* cur, float* eos_out) {
  front_prio();
  const int b = blockIdx.x, tid = threadIdx.x;
  const int NC = 513;  // cond_embed (512) | out_eos (1)
  // every load of the thread first (its two columns' slabs, thread 0's EOS slabs, the slot
  // state of the noise lanes), then the arithmetic: one memory round trip, not four
  const long zs = (long)B * NC;
  const float* p0 = P + (long)b * NC + tid;
  float v0[16], v1[16], ve[16];
#pragma unroll
  for (int z = 0; z < 16; ++z) {
    v0[z] = z < S ? p0[z * zs] : 0.f;
    v1[z] = z < S ? p0[z * zs + 256] : 0.f;
    ve[z] = (z < S && tid == 0) ? P[(long)b * NC + 512 + z * zs] : 0.f;
  }
  const SlotState& ss = st[b];
  const float temp = ss.temp, clamp = ss.noise_clamp;
  const unsigned long long seed = ss.seed;
  const int step = ss.step;
  // the row's own Euler step count: its time embeddings are rows temb_row0(n) .. + n - 1
  const int nrow = min(max(ss.lsd, 1), lsd_cap);
  const float* tn = temb + (long)temb_row0(nrow) * 512;
  const float b0 = bias[tid], b1 = bias[tid + 256], be = bias[512];
  float c0 = 0.f, c1 = 0.f, e = 0.f;
#pragma unroll
  for (int z = 0; z < 16; ++z)
    if (z < S) {
      c0 += v0[z];
      c1 += v1[z];
      e += ve[z];
    }
  c0 += b0;
  c1 += b1;
  for (int s = 0; s < lsd; ++s) {  // steps past the row's count repeat its last (finite, unused)
    const int ts = min(s, nrow - 1);
    ysilu[((long)s * B + b) * 512 + tid] = silu(tn[ts * 512 + tid] + c0);
    ysilu[((long)s * B + b) * 512 + tid + 256] = silu(tn[ts * 512 + tid + 256] + c1);
  }
  if (tid == 0) eos_out[b] = e + be;  // out_eos logit (flow_lm.rs:139-145); the EOS rule runs in front_commit
  if (tid < 32) cur[b * 32 + tid] = flow_noise(temp, clamp, seed, step, tid);
}

void flow_cond(const float* P, int S, int B, const float* bias, const float* temb, int lsd_run, int lsd_cap,
               const SlotState* st, float* ysilu, float* cur, float* eos_out, hipStream_t s) {
  if (S < 1 || S > FLOW_COND_MAX_SLABS) throw std::runtime_error("flow_cond: 1..16 split-K slabs");
  if (lsd_run < 1 || lsd_run > lsd_cap) throw std::runtime_error("flow_cond: lsd_run outside [1, cap]");
  hipLaunchKernelGGL(k_flow_cond, dim3(B), dim3(256), 0, s, P, S, B, bias, temb, lsd_run, lsd_cap, st, ysilu, cur,
                     eos_out);
}

// ---------------------------------------------------------------------------------------------
// Flow-head prelude in ONE launch (kernels.h head_prelude): cond | EOS GEMM, silu(c + temb), the
// adaLN GEMM, and the side jobs of k_flow_cond / the adaLN reduce (noise, x0, emptying the chain's
// regions). Workgroups 0 .. HP_PRODUCERS - 1 are producers, the HP_CONSUMERS after them consumers.
//
// Progress: a producer waits for nothing. A consumer waits only for producers, and workgroups are
// dispatched in index order, so whenever a consumer is resident every producer is resident or has
// finished: the launch completes however few workgroups fit on the device at once.
//
// Producer ct: columns 16 ct .. + 15 of cond | EOS over the whole K = 1024 exactly as k_gemv_fk
// (A in gemv_fk's fragment order, the weight packed by pack_gemv_fk); its epilogue adds the bias,
// writes the EOS logit (column 512) and, for every Euler step s of the launch, publishes
// y_s = silu(temb_row(s) + c) into hand-off region (s, row tile t) in the consumers' A-fragment
// order: float4 (kq * 8 + j) * 64 + 16 g + r = y_s[row 16 t + r][128 kq + 32 g + 4 j .. + 3]
// (data-as-flag, sc1 stores, a NaN stored canonical; rows past B as 0).
// Consumer cw: adaLN columns 64 cw .. + 63 over the whole K = 512. Wave w takes the 128-k range
// kq = w & 3 of the column tiles 2 (w >> 2) and 2 (w >> 2) + 1; its two weight fragments
// (pack_head_ada: float4 ((((cw * 8 + w) * 2 + c2) * 8 + j) * 64 + l = W[64 cw + 32 (w >> 2) +
// 16 c2 + (l & 15)][128 kq + 32 (l >> 4) + 4 j .. + 3]) are requested at the start and stay in
// registers for every Euler step and row tile. v_mfma_f32_16x16x4f32 sums k = 128 kq + 32 g + s
// over the lane groups g at step s for A and B alike; the 4 k ranges of a column tile are summed
// in LDS in kq order (a fixed order: a row's result depends on neither B nor its row index).
// ---------------------------------------------------------------------------------------------
__global__ void k_pack_head_ada(const float* __restrict__ W, float* __restrict__ P) {
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= (long)HP_NADA * FH_D / 4) return;
  const int l = (int)(i4 & 63), j = (int)((i4 >> 6) & 7), c2 = (int)((i4 >> 9) & 1), w = (int)((i4 >> 10) & 7);
  const int cw = (int)(i4 >> 13);
  const int n = 64 * cw + 32 * (w >> 2) + 16 * c2 + (l & 15), k = 128 * (w & 3) + 32 * (l >> 4) + 4 * j;
  reinterpret_cast<float4*>(P)[i4] = *reinterpret_cast<const float4*>(W + (long)n * FH_D + k);
}
void pack_head_ada(const float* W, float* packed, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_head_ada, dim3(HP_NADA * FH_D / 4 / 256), dim3(256), 0, s, W, packed);
}

__global__ __launch_bounds__(512) void k_head_prelude(HeadPreludeArgs a) {
  front_prio();
  __shared__ __attribute__((aligned(16))) float red[8 * 2 * 4 * 64];
  __shared__ __attribute__((aligned(16))) float sC[32 * 16];  // producer: c tile; consumer: the row's noise
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int RG = (a.B + 15) >> 4;
  typedef float f4v __attribute__((ext_vector_type(4)));
  const auto hr = sc1_rsrc(a.hand);
  if (blockIdx.x < HP_PRODUCERS) {
    const int ct = blockIdx.x;
    const f4v* wp = reinterpret_cast<const f4v*>(a.Pc) + ((long)(ct * 8 + w) * 8) * 64 + lane;
    const f4v* ap = reinterpret_cast<const f4v*>(a.A) + ((long)(w * 2) * 8) * 64 + lane;
    f4v b[8], a0[8], a1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      b[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + j * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a0[j] = ap[j * 64];
      a1[j] = ap[(8 + j) * 64];
    }
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the first MFMA (k_gemv_fk)
    floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (front_skip() & 2) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j][e], b[j][e], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j][e], b[j][e], c1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[((w * 2 + 0) * 4 + i) * 64 + lane] = c0[i];
      red[((w * 2 + 1) * 4 + i) * 64 + lane] = c1[i];
    }
    __syncthreads();
    {  // thread tid: row tile t, register i, lane ll (C map: column ll & 15, row (ll >> 4) * 4 + i)
      const int t = tid >> 8, i = (tid >> 6) & 3, ll = tid & 63;
      float v = red[((0 * 2 + t) * 4 + i) * 64 + ll];
#pragma unroll
      for (int ww = 1; ww < 8; ++ww) v += red[((ww * 2 + t) * 4 + i) * 64 + ll];
      const int row = 16 * t + (ll >> 4) * 4 + i, col = ct * 16 + (ll & 15);
      v += a.cbias[col];
      if (col == FH_D && row < a.B) a.eos_out[row] = v;  // out_eos logit; the EOS rule runs in front_commit
      sC[row * 16 + (ll & 15)] = v;
    }
    __syncthreads();
    if (ct < FH_D / 16 && tid < 128) {  // row m, columns k .. k + 3 of cond_embed
      const int m = tid & 31, c4 = tid >> 5, k = 16 * ct + 4 * c4;
      if ((m >> 4) < RG) {
        const bool live = m < a.B;
        const float4 c = *reinterpret_cast<const float4*>(&sC[m * 16 + 4 * c4]);
        // the row's own Euler step count: its time embeddings are rows temb_row0(n) .. + n - 1
        const int nrow = live ? min(max(a.st[m].lsd, 1), a.lsd_cap) : 1;
        const float* tn = a.temb + (long)temb_row0(nrow) * FH_D + k;
        const int off = (((k >> 7) * 8 + ((k >> 2) & 7)) * 64 + ((k >> 5) & 3) * 16 + (m & 15)) * 16;
        for (int s = 0; s < a.lsd; ++s) {  // steps past the row's count repeat its last (finite, unused)
          const float4 te = *reinterpret_cast<const float4*>(tn + (long)min(s, nrow - 1) * FH_D);
          float4 y = make_float4(silu(te.x + c.x), silu(te.y + c.y), silu(te.z + c.z), silu(te.w + c.w));
          if (!live) y = make_float4(0.f, 0.f, 0.f, 0.f);
          fh_put(hr, (s * RG + (m >> 4)) * (int)(HP_REGION_FLOATS * 4) + off, y);
        }
      }
    }
    return;
  }
  // ---- consumer
  const int cw = blockIdx.x - HP_PRODUCERS;
  const int kq = w & 3;
  const f4v* wp = reinterpret_cast<const f4v*>(a.Pa) + ((long)((cw * 8 + w) * 2) * 8) * 64 + lane;
  f4v b0[8], b1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    b0[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + j * 64);
    b1[j] = (front_skip() & 1) ? f4v{0.f, 0.f, 0.f, 0.f} : __builtin_nontemporal_load(wp + (8 + j) * 64);
  }
  __builtin_amdgcn_sched_barrier(0);
  // side jobs behind the weight request, through the wait for the producers: they depend on nothing
  // in this launch. Consumer 4 b + q: row b's noise, then columns 128 q .. + 127 of its x0 into the
  // chain's region 0; every consumer: its share of the chain's other regions, emptied
  if (cw < 4 * a.B) {
    const int b = cw >> 2, q = cw & 3;
    if (tid < FH_L) {
      const SlotState& ss = a.st[b];
      const float x0 = flow_noise(ss.temp, ss.noise_clamp, ss.seed, ss.step, tid);
      sC[tid] = x0;
      if (q == 0) a.cur[b * FH_L + tid] = x0;
    }
    __syncthreads();
    if (tid < 128) fh_x0_one(sC, a.x0_w, a.x0_b, a.x0_hx, b, 128 * q + tid);
  }
  for (long i = (long)cw * 512 + tid; i < a.fill_n4; i += (long)HP_CONSUMERS * 512)
    reinterpret_cast<uint4*>(a.fill)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  bool dead = false;
  for (int s = 0; s < a.lsd; ++s)
    for (int t = 0; t < RG; ++t) {
      // this wave's A fragment of region (s, t), swept until none of it is empty (fh_sweep); a
      // timeout sets *err and stops waiting for the rest of the launch
      const int aoff = (s * RG + t) * (int)(HP_REGION_FLOATS * 4) + (kq * 8 * 64 + lane) * 16;
      float4 av[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = fh_ld(hr, aoff + j * 64 * 16);
      unsigned spins = 0;
      while (!dead) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) ok &= !fh_empty(av[j]);
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (fh_empty(av[j])) av[j] = fh_ld(hr, aoff + j * 64 * 16);
        if (++spins > (1u << 20)) {
          if (lane == 0) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          dead = true;
        }
      }
      floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (front_skip() & 2) break;
        const float ae[4] = {av[j].x, av[j].y, av[j].z, av[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], b0[j][e], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], b1[j][e], c1, 0, 0, 0);
        }
      }
      __syncthreads();  // the tile before this one is read out of red (and the side job out of sC)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        red[((w * 2 + 0) * 4 + i) * 64 + lane] = c0[i];
        red[((w * 2 + 1) * 4 + i) * 64 + lane] = c1[i];
      }
      __syncthreads();
      if (tid < 256) {  // column tile ctl of the workgroup's 4, row r, columns 4 q4 .. + 3 of the tile
        const int ctl = tid >> 6, r = (tid >> 2) & 15, q4 = tid & 3;
        // C map: register r & 3 of lanes (r >> 2) * 16 + 4 q4 .. + 3: one aligned float4 of red
        const float* rp = red + (((ctl >> 1) * 4 * 2 + (ctl & 1)) * 4 + (r & 3)) * 64 + (r >> 2) * 16 + 4 * q4;
        float4 v = *reinterpret_cast<const float4*>(rp);
#pragma unroll
        for (int kk = 1; kk < 4; ++kk) v = f4add(v, *reinterpret_cast<const float4*>(rp + kk * 2 * 4 * 64));
        const int brow = 16 * t + r, n = 64 * cw + 16 * ctl + 4 * q4;
        if (brow < a.B) {
          v = f4add(v, *reinterpret_cast<const float4*>(a.abias + n));
          *reinterpret_cast<float4*>(a.mods + ((long)s * a.B + brow) * HP_NADA + n) = v;
          const long idx = fhm_index(s, brow, a.B, n);
          if (idx >= 0) reinterpret_cast<float4*>(a.fhm)[idx] = v;
        }
      }
    }
}

bool head_prelude_supported(int B, int lsd_run) { return B >= 1 && B <= 32 && lsd_run >= 1; }

void head_prelude(const HeadPreludeArgs& a, hipStream_t s) {
  if (!head_prelude_supported(a.B, a.lsd) || a.lsd > a.lsd_cap) throw std::runtime_error("head_prelude: bad shape");
  hipLaunchKernelGGL(k_head_prelude, dim3(HP_PRODUCERS + HP_CONSUMERS), dim3(512), cap_lds(k_head_prelude, g_wg_cap), s,
                     a);
}

// =============================================================================================
// Mimi front: denorm -> 1x1 quantizer -> depthwise ConvTrUpsample1d (k=32, s=16) -> LN.
// The transposed conv's overlap-add `partial` (conv.rs:202-267) equals qprev * W[:, 16 + r],
// so the kernel keeps the previous frame's quantized vector instead.
// =============================================================================================
// Denorm + quantizer 1x1 conv (mimi.rs:8-37) + depthwise ConvTrUpsample1d k32 s16
// (conv.rs:315-346: frame row r = q*w[r] + qprev*w[16+r], the overlap-add of the previous frame's
// tail) + norm1 of Mimi layer 0. One workgroup per (row b, 4 of the 16 output rows): 4x the
// workgroups of a per-row kernel, each loading only its rows' upsample taps, one LayerNorm row
// per wave. The pass's quantizer outputs go to a scratch (qprev_out [B][NFR_MAX][512]) and the commit
// moves the last valid frame's into the history, so the four workgroups of a row never race on
// it, and a row without a frame in the pass (or outside it) keeps its history unchanged.
struct QuantUpArgs {
  const float* latent[NFR_MAX];
  const FrameFlags* fl[NFR_MAX];
  int nfr;
  const float *emb_std, *emb_mean, *wq, *wup, *qprev_in;
  float* qprev_out;
  float *x, *h;
  const float *ln_w, *ln_b;
};
// grid (B, 4 nfr): rows 4 (y % 4).. of frame y / 4 of row b
__global__ __launch_bounds__(256) void k_quant_upsample(QuantUpArgs a) {
  __shared__ float sz[NFR_MAX][32];
  __shared__ float sx[4 * 512];
  const int b = blockIdx.x, f = blockIdx.y >> 2, r0 = (blockIdx.y & 3) * 4, tid = threadIdx.x;
  const int T = 16 * a.nfr;
  // every operand load of the thread's two channels is issued before the arithmetic
  float4 wqr[2][8], wur[2][2];
  float qpv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = tid + 256 * u;
#pragma unroll
    for (int i = 0; i < 8; ++i) wqr[u][i] = *reinterpret_cast<const float4*>(a.wq + c * 32 + 4 * i);
    wur[u][0] = *reinterpret_cast<const float4*>(a.wup + c * 32 + r0);
    wur[u][1] = *reinterpret_cast<const float4*>(a.wup + c * 32 + 16 + r0);
    qpv[u] = a.qprev_in[(long)b * 512 + c];
  }
  if (tid < 32 * a.nfr) {
    const int g = tid >> 5, k = tid & 31;
    sz[g][k] = a.latent[g][b * 32 + k] * a.emb_std[k] + a.emb_mean[k];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = tid + 256 * u;
    const float* wqf = reinterpret_cast<const float*>(wqr[u]);
    const float* w0 = reinterpret_cast<const float*>(&wur[u][0]);
    const float* w1 = reinterpret_cast<const float*>(&wur[u][1]);
    float q[NFR_MAX] = {};
#pragma unroll
    for (int g = 0; g < NFR_MAX; ++g)
      if (g < a.nfr) {
#pragma unroll
        for (int k = 0; k < 32; ++k) q[g] += wqf[k] * sz[g][k];
      }
    // frame f overlaps frame f - 1 (frame 0 the history); selects, no dynamic register indexing
    float cur = q[0], prev = qpv[u];
#pragma unroll
    for (int g = 1; g < NFR_MAX; ++g)
      if (f == g) cur = q[g], prev = q[g - 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = cur * w0[r] + prev * w1[r];
      sx[r * 512 + c] = v;
      a.x[((long)b * T + 16 * f + r0 + r) * 512 + c] = v;
    }
    if (blockIdx.y == 0) {
#pragma unroll
      for (int g = 0; g < NFR_MAX; ++g)
        if (g < a.nfr) a.qprev_out[((long)b * NFR_MAX + g) * 512 + c] = q[g];
    }
  }
  __syncthreads();
  const int lane = tid & 63, r = tid >> 6;  // one row per wave
  float v[8], sm = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = sx[r * 512 + lane + 64 * i];
    sm += v[i];
  }
  const float mean = wave_sum(sm) / 512.f;
  float qq = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) qq += (v[i] - mean) * (v[i] - mean);
  const float den = sqrtf(wave_sum(qq) / 512.f + 1e-5f);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = lane + 64 * i;
    a.h[((long)b * T + 16 * f + r0 + r) * 512 + n] = (v[i] - mean) / den * a.ln_w[n] + a.ln_b[n];
  }
}

void quant_upsample(const float* const latent[NFR_MAX], const FrameFlags* const fl[NFR_MAX], int nfr, int B, const float* emb_std,
                    const float* emb_mean, const float* wq, const float* wup, const float* qprev_in, float* qprev_out,
                    float* x, float* h, const float* ln_w, const float* ln_b, hipStream_t s) {
  if (nfr < 1 || nfr > NFR_MAX) throw std::runtime_error("quant_upsample: 1 to NFR_MAX frames");
  QuantUpArgs a{};
  for (int g = 0; g < NFR_MAX; ++g) {
    a.latent[g] = latent[g < nfr ? g : 0];
    a.fl[g] = fl[g < nfr ? g : 0];
  }
  a.nfr = nfr;
  a.emb_std = emb_std;
  a.emb_mean = emb_mean;
  a.wq = wq;
  a.wup = wup;
  a.qprev_in = qprev_in;
  a.qprev_out = qprev_out;
  a.x = x;
  a.h = h;
  a.ln_w = ln_w;
  a.ln_b = ln_b;
  hipLaunchKernelGGL(k_quant_upsample, dim3(B, 4 * nfr), dim3(256), cap_lds(k_quant_upsample, g_wg_cap), s, a);
}

// =============================================================================================
// Step commit: conv histories (last P input rows per slot), counters, next backbone input.
// =============================================================================================
// One workgroup per row: every history of the row (P x C floats each, C % 4 == 0) and its
// quantizer output, as float4 copies (the launch is one capped round: 32 workgroups, where a
// workgroup per (history, row) took two rounds of scalar copies).
__global__ __launch_bounds__(256) void k_commit(CommitArgs a) {
  const int b = blockIdx.x;
  if (a.fin_side) {  // every row (as the final conv computes every row): tile-boundary shares
    const int nx = a.fin_T / RESBLOCK_FIN_TT;
    for (int e = 2 + threadIdx.x; e < 2 * nx; e += 256)
      a.fin_pcm[(long)b * (a.fin_ld ? a.fin_ld : a.fin_T) + (e >> 1) * RESBLOCK_FIN_TT + (e & 1)] +=
          a.fin_side[(long)b * 2 * nx + e];
  }
  int nv = 0;  // valid frames: a prefix
  while (nv < a.nfr && a.flags[nv][b].valid) ++nv;
  if (nv == 0) return;
  for (int i = 0; i < a.nh; ++i) {
    const HistDesc& hd = a.h[i];
    const long n4 = (long)hd.P * hd.C / 4;
    const int tv = hd.T / a.nfr * nv;  // rows through the last valid frame
    const float4* src = reinterpret_cast<const float4*>(hd.src + ((long)b * hd.T + (tv - hd.P)) * hd.C);
    float4* dst = reinterpret_cast<float4*>(hd.dst + (long)b * hd.P * hd.C);
    if (hd.elu) {
      for (long e = threadIdx.x; e < n4; e += 256) {
        const float4 v = src[e];
        dst[e] = make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w));
      }
    } else {
      for (long e = threadIdx.x; e < n4; e += 256) dst[e] = src[e];
    }
  }
  // the overlap-add history of the next pass: the last valid frame's quantizer output
  if (threadIdx.x < 128)
    reinterpret_cast<float4*>(a.qprev + (long)b * 512)[threadIdx.x] =
        reinterpret_cast<const float4*>(a.qcur + ((long)b * NFR_MAX + nv - 1) * 512)[threadIdx.x];
  if (threadIdx.x == 0) a.mpos[b] += 16 * nv;
}

// x[m] = lat[m] W^T (K = 32) for the 4 columns n.. of this thread, and h[m] = LN(x[m]) (eps 1e-5)
// over the 256 threads of the workgroup (one row): flow_lm.rs:117 input_linear +
// transformer.rs:66-90 norm1 of layer 0. The weight arrives transposed, Wt [32][1024], so the 64
// lanes of a wave read one contiguous 1-KB run of Wt[k] per load. lat: the row's 32 inputs.
// input_linear4 is the projection alone (the prefill's latent-prefix rows, k_prefill_input).
// The operands that depend on nothing computed: this thread's 32 Wt quads and its LayerNorm
// affine quads, requested at kernel entry (input_ln_request) so that they travel with the
// caller's state loads instead of behind its barriers. A kernel without the projection (Wt ==
// nullptr) reads the stand-in address `alt` (>= 16 B, 16-B aligned) and drops the values.
struct InputLnOps {
  float4 wv[32], w4, b4;
};
__device__ __forceinline__ void input_linear_request(const float* __restrict__ Wt, const float* alt, float4 (&wv)[32]) {
  const int n = 4 * threadIdx.x;  // N = 1024
#pragma unroll
  for (int k = 0; k < 32; ++k) wv[k] = ldg4(Wt ? Wt + (long)k * 1024 + n : alt);
}
__device__ __forceinline__ void input_ln_request(const float* __restrict__ Wt, const float* __restrict__ lnw,
                                                 const float* __restrict__ lnb, const float* alt, InputLnOps& o) {
  const int n = 4 * threadIdx.x;
  input_linear_request(Wt, alt, o.wv);
  o.w4 = ldg4(Wt ? lnw + n : alt);
  o.b4 = ldg4(Wt ? lnb + n : alt);
}
__device__ __forceinline__ float4 input_linear4(const float* lat, const float4 (&wv)[32]) {
  float4 lv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) lv[j] = *reinterpret_cast<const float4*>(lat + 4 * j);
  float acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // same summation order as the row-major form: ((k0 k1) + (k2 k3)) per float4
      const float a0 = lv[j].x * (&wv[4 * j].x)[q], a1 = lv[j].y * (&wv[4 * j + 1].x)[q];
      const float a2 = lv[j].z * (&wv[4 * j + 2].x)[q], a3 = lv[j].w * (&wv[4 * j + 3].x)[q];
      t += (a0 + a1) + (a2 + a3);
    }
    acc[q] = t;
  }
  return make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__device__ __forceinline__ void input_ln_row(const float* lat, const InputLnOps& ops, float* __restrict__ xr,
                                             float* __restrict__ hr, float* sh) {
  const int n = 4 * threadIdx.x;  // N = 1024
  const float4 v = input_linear4(lat, ops.wv);
  *reinterpret_cast<float4*>(xr + n) = v;
  const float mean = block_sum((v.x + v.y) + (v.z + v.w), sh) / 1024.f;
  const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
  const float den = sqrtf(block_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w), sh) / 1024.f + 1e-5f);
  const float4 w4 = ops.w4, b4 = ops.b4;
  *reinterpret_cast<float4*>(hr + n) =
      make_float4(d.x / den * w4.x + b4.x, d.y / den * w4.y + b4.y, d.z / den * w4.z + b4.z, d.w / den * w4.w + b4.w);
}

// one 256-thread block per row: the EOS rule and frame flags (lane 0), the frame's latent, then
// the next step's x / h rows from the updated backbone input (the step's first launch, folded in)
__global__ __launch_bounds__(256) void k_front_commit(FrontCommitArgs a) {
  front_prio();
  __shared__ float s_lat[32];
  __shared__ float sh[4];
  const int b = blockIdx.x, t = threadIdx.x;
  SlotState& ss = a.st[b];
  const int valid = ss.active;
  const float e = a.eos[b];                       // loaded with `active`: one round trip
  const float cv = t < 32 ? a.cur[b * 32 + t] : 0.f;
  const float li = t < 32 ? a.lat_in[b * 32 + t] : 0.f;
  // the next step's projection weights and LN affine with the state loads: the same round trip
  // (they depend on nothing computed here; stand-in: cur's allocation, aligned down to 16 B)
  InputLnOps ops;
  input_ln_request(a.Wt, a.lnw, a.lnb, reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(a.cur) & ~(uintptr_t)15),
                   ops);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();  // every lane has read `active` before lane 0 updates the state
  if (t == 0) {
    FrameFlags f{0, 0};
    if (valid) {  // tts_model.rs:1055-1063 + map_while over 0..max_gen_len
      if (e > ss.eos_threshold && ss.eos_step < 0) ss.eos_step = ss.step;
      const bool tail = ss.eos_step >= 0 && ss.step >= ss.eos_step + ss.frames_after_eos;
      f.valid = 1;
      f.last = (tail || ss.step + 1 >= ss.max_frames) ? 1 : 0;
      ss.step += 1;
      a.fpos[b] += 1;
      if (f.last) ss.active = 0;
    }
    a.flags[b] = f;
    a.eos_out[b] = e;
    if (b == 0 && a.err_host)
      __hip_atomic_store(a.err_host, __hip_atomic_load(a.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (b == 0)
    for (int r = t; r < a.n_zero; r += 256) a.flags[a.B + r] = FrameFlags{0, 0};
  if (t < 32) {
    a.lat_out[b * 32 + t] = cv;
    if (valid) a.lat_in[b * 32 + t] = cv;
    s_lat[t] = valid ? cv : li;
  }
  if (!a.Wt) return;  // uniform
  __syncthreads();
  input_ln_row(s_lat, ops, a.x + (long)b * 1024, a.h + (long)b * 1024, sh);
}

void front_commit(const FrontCommitArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_front_commit, dim3(a.B), dim3(256), 0, s, a);
}

void step_commit(const CommitArgs& a, hipStream_t s) {
  for (int i = 0; i < a.nh; ++i)
    if (a.h[i].C % 4) throw std::runtime_error("step_commit: history channels must be a multiple of 4");
  hipLaunchKernelGGL(k_commit, dim3(a.B), dim3(256), cap_lds(k_commit, g_wg_cap), s, a);
}

__global__ __launch_bounds__(256) void k_slot_reset(ResetArgs a) {
  const int i = blockIdx.x, b = blockIdx.y;
  const int slot = a.slots[i];
  const int opt = a.opt_src ? a.opt_src[i] : 0;
  if (b < a.nb) {
    if (opt & RESET_KEEP_CODEC) return;  // the row decodes on from the state its slot ended on
    float* p = a.buf[b] + (long)slot * a.per_slot[b];
    for (long e = threadIdx.x; e < a.per_slot[b]; e += 256) p[e] = 0.f;
    return;
  }
  if (threadIdx.x < 32)
    a.lat_in[slot * 32 + threadIdx.x] = (opt & RESET_LAT_SRC) ? a.lat_src[i * 32 + threadIdx.x] : a.bos[threadIdx.x];
  if (threadIdx.x == 0) {
    a.st[slot] = a.st_src[i];
    a.fpos[slot] = a.fpos_src[i];
    if (!(opt & RESET_KEEP_CODEC)) a.mpos[slot] = 0;
    for (int q = 0; q < NHB_MAX; ++q)
      if (a.flags[q]) a.flags[q][slot] = FrameFlags{0, 0};
    if (a.wire_fmt) {
      a.wire_fmt[slot] = a.wire_src[i];
      a.wire_frames[slot] = 0;
    }
    if (a.tempo_sp) {
      a.tempo_sp[slot] = a.tempo_src[i];
      for (int q = 0; q < TEMPO_STATE; ++q) a.tempo_state[slot * TEMPO_STATE + q] = 0;
    }
    if (a.pitch_step) {
      a.pitch_step[slot] = a.pitch_src[i];
      for (int q = 0; q < PITCH_STATE; ++q) a.pitch_state[slot * PITCH_STATE + q] = 0;
    }
    if (a.level_gain) {
      a.level_gain[slot] = a.level_src[i];
      for (int q = 0; q < LEVEL_STATE; ++q) a.level_state[slot * LEVEL_STATE + q] = 0;
    }
    if (a.loud_state) {
      a.loud_state[slot * LOUD_STATE] = a.loud_src[i];
      a.loud_state[slot * LOUD_STATE + 1] = 0;
    }
  }
}

void slot_reset(const ResetArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_slot_reset, dim3(a.n, a.nb + 1), dim3(256), 0, s, a);
}

struct GatherArgs {
  const float* lat;
  const FrameFlags* flags;
  float* lat_out;
  FrameFlags* flags_out;
  int n;
  int idx[GATHER_MAX];
};

__global__ __launch_bounds__(64) void k_gather_preview(GatherArgs a) {
  const int i = blockIdx.x, t = threadIdx.x;
  const bool on = i < a.n;
  const int r = on ? a.idx[i] : 0;
  if (t < 32) a.lat_out[i * 32 + t] = on ? a.lat[(long)r * 32 + t] : 0.f;
  if (t == 32) a.flags_out[i] = on ? a.flags[r] : FrameFlags{0, 0};
}

void gather_preview(const float* lat, const FrameFlags* flags, const int* idx, int n, int P, float* lat_out,
                    FrameFlags* flags_out, hipStream_t s) {
  if (n < 0 || n > P || P < 1 || P > GATHER_MAX) throw std::runtime_error("gather_preview: 0 <= n <= P <= 8");
  GatherArgs a{lat, flags, lat_out, flags_out, n, {}};
  for (int i = 0; i < n; ++i) a.idx[i] = idx[i];
  hipLaunchKernelGGL(k_gather_preview, dim3(P), dim3(64), 0, s, a);
}

// =============================================================================================
// Time embeddings (once per engine / lsd_decode_steps): grid (step, embedder).
// =============================================================================================
__global__ __launch_bounds__(256) void k_time_embed(TimeEmbedWeights w, int n, float* tmp) {
  __shared__ float emb[256];
  __shared__ float h1[512];
  __shared__ float sh[4];
  const int i = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
  const float tau = (float)((double)(e == 0 ? i : i + 1) / (double)n);  // s = i/N, t = (i+1)/N
  if (tid < 128) {
    const float f = expf(-logf(10000.0f) * (float)tid / 128.0f);
    emb[tid] = cosf(tau * f);
    emb[128 + tid] = sinf(tau * f);
  }
  __syncthreads();
  for (int o = tid; o < 512; o += 256) {
    float acc = 0.f;
    for (int k = 0; k < 256; ++k) acc += w.l1w[e][o * 256 + k] * emb[k];
    h1[o] = silu(acc + w.l1b[e][o]);
  }
  __syncthreads();
  float v[2];
  for (int q = 0; q < 2; ++q) {
    const int o = tid + 256 * q;
    float acc = 0.f;
    for (int k = 0; k < 512; ++k) acc += w.l2w[e][o * 512 + k] * h1[k];
    v[q] = acc + w.l2b[e][o];
  }
  const float mean = block_sum(v[0] + v[1], sh) / 512.f;
  const float var = block_sum((v[0] - mean) * (v[0] - mean) + (v[1] - mean) * (v[1] - mean), sh) / 511.f;
  const float inv = 1.0f / sqrtf(var + 1e-5f);  // RMSNorm on unbiased variance (mlp.rs:18-26)
  for (int q = 0; q < 2; ++q) {
    const int o = tid + 256 * q;
    tmp[((long)e * n + i) * 512 + o] = v[q] * inv * w.alpha[e][o];
  }
}
__global__ void k_time_avg(const float* tmp, int n, float* out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < n * 512) out[idx] = (tmp[idx] + tmp[n * 512 + idx]) / 2.0f;
}
void time_embeddings(const TimeEmbedWeights& w, int n, float* tmp, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_time_embed, dim3(n, 2), dim3(256), 0, s, w, n, tmp);
  hipLaunchKernelGGL(k_time_avg, dim3((n * 512 + 255) / 256), dim3(256), 0, s, tmp, n, out);
}

// =============================================================================================
// Small helpers.
// =============================================================================================
__global__ void k_embed(const int* ids, int n, const float* table, int dim, float* out) {
  const int i = blockIdx.x;
  const float* src = table + (long)ids[i] * dim;
  for (int c = threadIdx.x; c < dim; c += blockDim.x) out[(long)i * dim + c] = src[c];
}
void embed_gather(const int* ids, int n, const float* table, int dim, float* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_embed, dim3(n), dim3(256), 0, s, ids, n, table, dim, out);
}

// Input rows of a prefill pass that holds latent-prefix rows (one 256-thread block per compact row):
// src[i] >= 0: the embedding row of that token, as k_embed; PREFILL_SRC_BOS: input_linear(bos);
// below it: input_linear of staged latent PREFILL_SRC_LAT0 - src[i] (the projection of
// input_ln_row, in its summation order: what a step computes from the same backbone input).
__global__ __launch_bounds__(256) void k_prefill_input(const int* __restrict__ src, const float* __restrict__ table,
                                                       const float* __restrict__ lat, const float* __restrict__ bos,
                                                       const float* __restrict__ Wt, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_lat[32];
  const int i = blockIdx.x, n = 4 * threadIdx.x;
  const int v = src[i];  // uniform over the block
  float4* dst = reinterpret_cast<float4*>(out + (long)i * 1024 + n);
  if (v >= 0) {
    *dst = *reinterpret_cast<const float4*>(table + (long)v * 1024 + n);
    return;
  }
  if (threadIdx.x < 32)
    s_lat[threadIdx.x] = v == PREFILL_SRC_BOS ? bos[threadIdx.x] : lat[(long)(PREFILL_SRC_LAT0 - v) * 32 + threadIdx.x];
  __syncthreads();
  float4 wv[32];
  input_linear_request(Wt, Wt, wv);
  *dst = input_linear4(s_lat, wv);
}
void prefill_input(const int* src, int n, const float* table, const float* lat, const float* bos, const float* Wt,
                   int dim, float* out, hipStream_t s) {
  if (dim != 1024) throw std::runtime_error("prefill_input: dim must be 1024");
  if (n > 0) hipLaunchKernelGGL(k_prefill_input, dim3(n), dim3(256), 0, s, src, table, lat, bos, Wt, out);
}

__global__ void k_copy2d(const float* src, long lds, float* dst, long ldd, int rows, int cols) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)rows * cols) return;
  const int r = (int)(idx / cols), c = (int)(idx % cols);
  dst[(long)r * ldd + c] = src[(long)r * lds + c];
}
void copy2d(const float* src, long lds, float* dst, long ldd, int rows, int cols, hipStream_t s) {
  const long total = (long)rows * cols;
  if (total > 0) hipLaunchKernelGGL(k_copy2d, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
}

// Final SEANet conv (64 -> 1, k=3) with ELU'd input and 2-row history: one thread per sample.
// One wave per (batch row, 64 consecutive outputs): lane c owns input channel c (cin == 64) and
// loads its channel of the 64 + k - 1 input rows with coalesced 256-B row reads (history rows for
// t < 0), applies ELU once per element, and the k-tap dot products are reduced across the wave.
// One wave per (batch row, 64 consecutive outputs). The 64 + k - 1 input rows (cin == 64; history
// rows for t < 0) are read with coalesced 256-B row loads, ELU'd once per element and transposed
// through a padded LDS tile (row stride 65: conflict-free column reads); lane t then forms output
// t as a plain k x cin dot product (weights broadcast from LDS).
// =============================================================================================
// Fused SEANet residual block of one decoder stage (seanet.rs:43-89; SEANetResnetBlock with one
// residual layer, kernel sizes [3, 1], true skip): per (utterance, time tile of TT rows)
//   v = elu(b3 + conv_k3(E))          E = elu(convtr output), the stage's k3 conv input; its two
//                                       rows before the frame come from the conv history HE
//   Y = elu(R + b1 + conv_k1(v))       R = the raw convtr output (skip); Y = the next stage's
//                                       (or the final conv's) ELU'd input
// The intermediate v never leaves the CU: it goes from the first GEMM's accumulators to LDS and
// is the second GEMM's A operand. Both GEMMs run on v_mfma_f32_32x32x2_f32 with A fragments read
// from LDS (rows padded by 16 B: conflict-free ds_read_b128) and W fragments straight from global
// memory (L2-resident; each lane one 64-B piece of a weight row), one K chunk ahead.
// Shapes (B = 32): stage 0 C 256 / H 128 / T 96, stage 1 128 / 64 / 480, stage 2 64 / 32 / 1920.
// =============================================================================================
template <int C, int H, int TT>
__global__ __launch_bounds__(256) void k_resblock(ResBlockArgs a) {
  if (a.back_hi) back_prio();
  constexpr int LDE = C + 4, LDV = H + 4;
  __shared__ __attribute__((aligned(16))) float sm[(TT + 2) * LDE + TT * LDV];
  float* sE = sm;
  float* sV = sm + (TT + 2) * LDE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * TT;
  // ---- E rows t0-2 .. t0+TT-1 (history rows for t < 0) into LDS: every load of the thread is
  // issued before the first LDS store (one memory round trip, not one per 256-thread sweep)
  constexpr int C4 = C / 4, NE = ((TT + 2) * C4 + 255) / 256;
  float4 ev[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = min(tid + 256 * i, (TT + 2) * C4 - 1);  // a clamped duplicate, never stored
    const int row = e / C4, c4 = e - row * C4;
    const int t = t0 - 2 + row;
    const float* src = t >= 0 ? a.E + ((long)b * a.T + t) * C : a.HE + ((long)b * 2 + (t + 2)) * C;
    ev[i] = *reinterpret_cast<const float4*>(src + 4 * c4);
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + 256 * i;
    if (e >= (TT + 2) * C4) break;
    const int row = e / C4, c4 = e - row * C4;
    float4 v = ev[i];
    if (a.e_raw && t0 - 2 + row >= 0) v = make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w));
    *reinterpret_cast<float4*>(sE + row * LDE + 4 * c4) = v;
  }
  __syncthreads();
  // ---- GEMM 1: v[TT][H] = E3[TT][3C] . W3[H][3C]^T, k = tap * C + c reads sE[i + tap][c]
  constexpr int MB = TT / 32, NB1 = H / 32, K1 = 3 * C / 32;
  for (int blk = wave; blk < MB * NB1; blk += 4) {
    const int mi = blk / NB1, ni = blk - mi * NB1;
    const float* wrow = a.W3 + (long)(32 * ni + r) * (3 * C) + 16 * h;
    floatx16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    // W fragments three chunks ahead (an L2 / MALL round trip is several chunks of MFMAs): a ring
    // of three register sets with fixed roles per unrolled step
    float4 w0[4], w1[4], w2[4];
    auto wload = [&](int kc, float4 (&w)[4]) {
      const int k = kc < K1 ? kc : K1 - 1;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = *reinterpret_cast<const float4*>(wrow + 32 * k + 4 * q);
    };
    auto step = [&](int kc, const float4 (&w)[4]) {
      const int k0 = 32 * kc + 16 * h, tap = k0 / C, c = k0 - tap * C;
      const float* ap = sE + (32 * mi + r + tap) * LDE + c;
      float af[16], bf[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(ap + 4 * q);
        af[4 * q] = x.x; af[4 * q + 1] = x.y; af[4 * q + 2] = x.z; af[4 * q + 3] = x.w;
        bf[4 * q] = w[q].x; bf[4 * q + 1] = w[q].y; bf[4 * q + 2] = w[q].z; bf[4 * q + 3] = w[q].w;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
    };
    static_assert(K1 % 3 == 0, "K1 = 3C/32 chunks: a multiple of 3 (the ring)");
    wload(0, w0);
    wload(1, w1);
    for (int kc = 0; kc < K1; kc += 3) {
      wload(kc + 2, w2);
      step(kc, w0);
      wload(kc + 3, w0);
      step(kc + 1, w1);
      wload(kc + 4, w1);
      step(kc + 2, w2);
    }
    const int col = 32 * ni + r;
    const float bias = a.b3[col];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = 32 * mi + (g & 3) + 8 * (g >> 2) + 4 * h;
      sV[row * LDV + col] = elu1(acc[g] + bias);
    }
  }
  __syncthreads();
  // ---- GEMM 2: Y[TT][C] = elu(R + b1 + v . W1[C][H]^T)
  constexpr int NB2 = C / 32, K2 = H / 32;
  for (int blk = wave; blk < MB * NB2; blk += 4) {
    const int mi = blk / NB2, ni = blk - mi * NB2;
    const float* wrow = a.W1 + (long)(32 * ni + r) * H + 16 * h;
    const int col = 32 * ni + r;
    const long base = ((long)b * a.T + t0) * C + col;
    float rv[16];  // the skip rows, requested ahead of the MFMAs that they do not depend on
#pragma unroll
    for (int g = 0; g < 16; ++g) rv[g] = a.R[base + (long)(32 * mi + (g & 3) + 8 * (g >> 2) + 4 * h) * C];
    floatx16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
#pragma unroll
    for (int kc = 0; kc < K2; ++kc) {
      const float* ap = sV + (32 * mi + r) * LDV + 32 * kc + 16 * h;
      float af[16], bf[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(ap + 4 * q);
        const float4 y = *reinterpret_cast<const float4*>(wrow + 32 * kc + 4 * q);
        af[4 * q] = x.x; af[4 * q + 1] = x.y; af[4 * q + 2] = x.z; af[4 * q + 3] = x.w;
        bf[4 * q] = y.x; bf[4 * q + 1] = y.y; bf[4 * q + 2] = y.z; bf[4 * q + 3] = y.w;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
    }
    const float bias = a.b1[col];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = 32 * mi + (g & 3) + 8 * (g >> 2) + 4 * h;
      const float y = elu1(acc[g] + bias + rv[g]);
      a.Y[base + (long)row * C] = y;
      if (C == 64 && a.fw) sE[row * LDE + col] = y;  // (sE is free: GEMM 1 is behind the barrier)
    }
  }
  if constexpr (C == 64) {
    if (!a.fw) return;  // uniform
    // ---- final conv (64 -> 1, k = 3) of this tile: out[t] = b + d0[t-2] + d1[t-1] + d2[t],
    // d_j[r] = w[j] . Y[r]. Rows -2, -1 (the utterance's first tile only) are the conv history.
    static_assert(TT == RESBLOCK_FIN_TT, "the side buffer is laid out for 128-row tiles");
    float* sD = sV;  // [3][TT + 2] (row r at index r + 2); sV is free once GEMM 2 is done
    __syncthreads();
    for (int e = tid; e < 2 * (TT + 2); e += 256) {
      const int r = e / 2 - 2, half = e & 1;  // two threads per row (adjacent lanes), 32 channels each
      const bool live = r >= 0 || t0 == 0;
      const float* yr = r >= 0 ? sE + r * LDE + 32 * half : a.fH + ((long)b * 2 + (live ? r + 2 : 0)) * 64 + 32 * half;
      float d[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4 y = *reinterpret_cast<const float4*>(yr + 4 * q);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float4 w = *reinterpret_cast<const float4*>(a.fw + j * 64 + 32 * half + 4 * q);
          d[j] += (y.x * w.x + y.y * w.y) + (y.z * w.z + y.w * w.w);
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        d[j] += __shfl_xor(d[j], 1, 64);
        if (half == 0) sD[j * (TT + 2) + r + 2] = live ? d[j] : 0.f;
      }
    }
    __syncthreads();
    const float fb = a.fb[0];
    const int nx = a.T / TT, x = blockIdx.x;
    if (tid < TT) {
      const int r = tid;
      const float d0 = sD[r], d1 = sD[(TT + 2) + r + 1], d2 = sD[2 * (TT + 2) + r + 2];
      // rows 0, 1 of a later tile: the terms from this tile's rows only (the rest via the side buffer)
      const float v = r >= 2 || t0 == 0 ? ((d0 + d1) + d2) + fb : (r == 0 ? d2 : d1 + d2) + fb;
      a.fout[(long)b * (a.fld ? a.fld : a.T) + t0 + r] = v;
    } else if (tid < TT + 2 && x + 1 < nx) {  // this tile's share of the next tile's rows 0, 1
      const int k = tid - TT;
      const float v = k == 0 ? sD[TT] + sD[(TT + 2) + TT + 1]  // d0[TT-2] + d1[TT-1]
                             : sD[TT + 1];                     // d0[TT-1]
      a.fside[((long)b * nx + x + 1) * 2 + k] = v;
    }
  }
}

void resblock(const ResBlockArgs& ra, hipStream_t s) {
  ResBlockArgs a = ra;
  a.back_hi = g_back_hi;
  // time tiles: stage 0 32 rows (96 workgroups), stage 1 96 (160), stage 2 128 (480) at B = 32
  if (a.C == 256 && a.T % 32 == 0)
    hipLaunchKernelGGL((k_resblock<256, 128, 32>), dim3(a.T / 32, a.B), dim3(256),
                       cap_lds(k_resblock<256, 128, 32>, g_wg_cap), s, a);
  else if (a.C == 128 && a.T % 96 == 0)
    hipLaunchKernelGGL((k_resblock<128, 64, 96>), dim3(a.T / 96, a.B), dim3(256),
                       cap_lds(k_resblock<128, 64, 96>, g_wg_cap), s, a);
  else if (a.C == 64 && a.T % 128 == 0 && (!a.fw || (a.fb && a.fH && a.fout && a.fside)))
    hipLaunchKernelGGL((k_resblock<64, 32, 128>), dim3(a.T / 128, a.B), dim3(256),
                       cap_lds(k_resblock<64, 32, 128>, g_wg_cap), s, a);
  else
    throw std::runtime_error("resblock: unsupported stage shape");
}

template <int KT>
__global__ __launch_bounds__(256) void k_conv_cout1(const float* X, const float* H, int B, int T, int cin,
                                                    const float* w, const float* bias, float* Y, int elu_in,
                                                    long ldy) {
  constexpr int P = KT - 1, ROWS = 64 + P;
  __shared__ float tile[4][ROWS][65];
  __shared__ float sw[KT * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < KT * 64; i += 256) sw[i] = w[i];
  const int blk = blockIdx.x * 4 + wave;
  const int nblk = (T + 63) / 64;
  const bool live = blk < B * nblk;
  const int b = live ? blk / nblk : 0, t0 = live ? (blk - b * nblk) * 64 : 0;
  const float* xb = X + (long)b * T * cin + lane;
  const float* hb = H + ((long)b * P + P) * cin + lane;
  float e[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {  // unconditional loads: rows past T re-read row T-1
    const int tt = min(t0 + i - P, T - 1);
    e[i] = tt >= 0 ? xb[(long)tt * cin] : hb[(long)tt * cin];
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) tile[wave][i][lane] = elu_in ? elu1(e[i]) : e[i];
  __syncthreads();
  float acc = 0.f;
#pragma unroll 8
  for (int c = 0; c < 64; ++c)
#pragma unroll
    for (int j = 0; j < KT; ++j) acc += sw[j * 64 + c] * tile[wave][lane + j][c];
  if (live && t0 + lane < T) Y[(long)b * ldy + t0 + lane] = acc + bias[0];
}

void conv_cout1(const float* X, const float* H, int B, int T, int cin, int k, const float* w, const float* bias,
                float* Y, int elu_in, hipStream_t s, long ldy) {
  const long waves = (long)B * ((T + 63) / 64);  // one lane per input channel: cin == 64, k == 3
  (void)k;
  hipLaunchKernelGGL(k_conv_cout1<3>, dim3((unsigned)((waves + 3) / 4)), dim3(256), cap_lds(k_conv_cout1<3>, g_wg_cap), s, X, H, B, T, cin, w, bias,
                     Y, elu_in, ldy > 0 ? ldy : (long)T);
}

// Encoder first conv (1 -> cout, k taps, zero history of k-1 samples): one thread per output.
__global__ __launch_bounds__(256) void k_conv_cin1(const float* X, int T, int cout, int k, const float* w,
                                                   const float* bias, float* Y) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)T * cout) return;
  const int t = (int)(idx / cout), co = (int)(idx % cout);
  float acc = 0.f;
  for (int j = 0; j < k; ++j) {
    const int tt = t + j - (k - 1);
    acc += (tt >= 0 ? X[tt] : 0.f) * w[co * k + j];
  }
  Y[idx] = acc + bias[co];
}
void conv_cin1(const float* X, int T, int cout, int k, const float* w, const float* bias, float* Y, hipStream_t s) {
  const long total = (long)T * cout;
  hipLaunchKernelGGL(k_conv_cin1, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, T, cout, k, w, bias, Y);
}

// ---------------------------------------------------------------------------------------------
// Polyphase resampler (see kernels.h), the one copy of the rule: resample() runs it on f32 samples,
// voice_ingest() on a clip in its wire format (f32, or int16: v / 32768, exact in f32), so the two
// agree bit for bit by construction. One workgroup per tile of 256 consecutive outputs, one lane
// per output: lanes of a wave walk consecutive outputs, so their input windows overlap and the x
// reads coalesce (2 or 4 B per sample); the taps (L floats, <= 64 KB) are staged once per
// workgroup in LDS. Each output touches only the ~L/up taps of its phase, accumulated in f64
// (scipy's f32 upfirdn differs by f32 rounding only). Zeros for n_out <= m < n_pad.
// up == down == 1 (launch-uniform; voice_ingest only): convert and pad, no taps.
__device__ __forceinline__ float ingest_load(const float* x, long j) { return x[j]; }
__device__ __forceinline__ float ingest_load(const short* x, long j) { return (float)x[j] * (1.0f / 32768.0f); }

// Output m of the rule: x[j] is read as x[j - xoff] (xoff = 0 for a whole signal; the wire stage
// holds a window of the signal in LDS), n_in = samples of the signal so far. The one tap loop of
// k_voice_ingest and k_wire: ascending j, f64 accumulation, rounded to f32 once.
template <typename T>
__device__ __forceinline__ float resample_out(const T* x, long xoff, long n_in, const float* h, int L, int up, int down,
                                              int half, long m) {
  const long a = m * down + half;  // h index of x[0]; x[j] pairs with h[a - j*up]
  const long jhi = min(a / up, n_in - 1);
  const long lo = a - (L - 1);
  const long jlo = max(lo <= 0 ? 0 : (lo + up - 1) / up, xoff);
  double acc = 0.0;
  for (long j = jlo; j <= jhi; ++j) acc += (double)ingest_load(x, j - xoff) * (double)h[a - j * up];
  return (float)acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_voice_ingest(const T* __restrict__ x, int n_in,
                                                      const float* __restrict__ taps, int L, int up, int down,
                                                      int half, int n_out, int n_pad, int use_lds,
                                                      float* __restrict__ y) {
  extern __shared__ float sh_taps[];
  const bool identity = up == 1 && down == 1;
  if (!identity && use_lds) {
    for (int i = threadIdx.x; i < L; i += blockDim.x) sh_taps[i] = taps[i];
    __syncthreads();
  }
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_pad) return;
  if (m >= n_out) {
    y[m] = 0.f;
    return;
  }
  if (identity) {
    y[m] = m < n_in ? ingest_load(x, m) : 0.f;
    return;
  }
  const float* h = use_lds ? sh_taps : taps;
  y[m] = resample_out(x, 0, (long)n_in, h, L, up, down, half, m);
}

namespace {
int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}
double bessel_i0(double x) {  // power series; converges in a few dozen terms for beta = 5
  double s = 1.0, t = 1.0;
  const double q = 0.25 * x * x;
  for (int k = 1; k < 500; ++k) {
    t *= q / ((double)k * k);
    s += t;
    if (t < 1e-17 * s) break;
  }
  return s;
}
}  // namespace

ResamplePlan resample_plan(int sr_from, int sr_to) {
  ResamplePlan p;
  const int g = gcd_int(sr_from, sr_to);
  p.up = sr_to / g;
  p.down = sr_from / g;
  p.half = 10 * std::max(p.up, p.down);  // resample_poly: half_len = 10 * max_rate
  p.L = 2 * p.half + 1;
  return p;
}

// firwin(L, 1/max_rate, window=("kaiser", 5.0)): windowed sinc normalised to unit DC gain,
// then cast to f32 and multiplied by `up` in f32, as resample_poly does for f32 input.
std::vector<float> resample_taps(const ResamplePlan& p) {
  std::vector<double> hd(p.L);
  const double fc = 1.0 / std::max(p.up, p.down), alpha = 0.5 * (p.L - 1), i0b = bessel_i0(5.0);
  double sum = 0.0;
  for (int i = 0; i < p.L; ++i) {
    const double v = fc * (i - alpha), r = (i - alpha) / alpha;
    const double sinc = v == 0.0 ? 1.0 : std::sin(M_PI * v) / (M_PI * v);
    hd[i] = fc * sinc * (bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b);
    sum += hd[i];
  }
  std::vector<float> h(p.L);
  for (int i = 0; i < p.L; ++i) h[i] = (float)(hd[i] / sum) * (float)p.up;
  return h;
}

void resample(const float* x, int n_in, const float* taps, const ResamplePlan& p, int n_out, int n_pad, float* y,
              hipStream_t s) {
  if (n_pad <= 0) return;
  const int use_lds = p.L <= 16384 ? 1 : 0;
  const size_t lds = use_lds ? sizeof(float) * (size_t)p.L : 0;
  // never with an identity plan here (the callers copy equal-rate input): the FIR branch
  hipLaunchKernelGGL(k_voice_ingest<float>, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), lds, s, x, n_in, taps, p.L,
                     p.up, p.down, p.half, n_out, n_pad, use_lds, y);
}

// ---------------------------------------------------------------------------------------------
// Voice-job ingest (see kernels.h): k_voice_ingest above on the clip's wire format.
void voice_ingest(const void* x, int fmt_s16, int n_in, const float* taps, const ResamplePlan& p, int n_out,
                  int n_pad, float* y, hipStream_t s) {
  if (n_pad <= 0) return;
  const int use_lds = !p.identity() && p.L <= 16384 ? 1 : 0;
  const size_t lds = use_lds ? sizeof(float) * (size_t)p.L : 0;
  const dim3 grid((unsigned)((n_pad + 255) / 256));
  if (fmt_s16)
    hipLaunchKernelGGL(k_voice_ingest<short>, grid, dim3(256), lds, s, (const short*)x, n_in, taps, p.L, p.up, p.down,
                       p.half, n_out, n_pad, use_lds, y);
  else
    hipLaunchKernelGGL(k_voice_ingest<float>, grid, dim3(256), lds, s, (const float*)x, n_in, taps, p.L, p.up, p.down,
                       p.half, n_out, n_pad, use_lds, y);
}

// ---------------------------------------------------------------------------------------------
// Wire stage (see kernels.h): the encodings, then the streaming kernel and the whole-signal one.
__device__ __forceinline__ int wire_s16(float x) {  // audio.rs:110-146: clamp, x 32767, truncate
  return (int)(fminf(fmaxf(x, -1.0f), 1.0f) * 32767.0f);
}
__device__ __forceinline__ unsigned wire_ulaw(int s) {
  int v = s >> 2;
  const unsigned mask = v < 0 ? 0x7Fu : 0xFFu;
  v = min(v < 0 ? -v : v, 8159) + 33;
  int seg = 0;
  while (seg < 8 && v > (0x3F << seg | ((1 << seg) - 1))) ++seg;  // 0x3F, 0x7F, .. 0x1FFF
  if (seg == 8) return 0x7Fu ^ mask;
  return (unsigned)((seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask;
}
__device__ __forceinline__ unsigned wire_alaw(int s) {
  const unsigned mask = s >= 0 ? 0xD5u : 0x55u;
  const int v = s >= 0 ? s >> 3 : (-s - 1) >> 3;  // <= 0xFFF: a segment always exists
  int seg = 0;
  while (seg < 7 && v > (0x1F << seg | ((1 << seg) - 1))) ++seg;  // 0x1F, 0x3F, .. 0xFFF
  return (unsigned)((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 15)) ^ mask;
}
// four consecutive samples -> 8 bytes (s16) or 4 bytes (G.711) at byte offset bytes_per * 4 g of
// dst, as dword stores; samples past the chunk's end arrive as 0.f (padding inside the chunk slot)
__device__ __forceinline__ void wire_store4(unsigned char* dst, long g, int enc, const float v[4]) {
  int s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = wire_s16(v[q]);
  if (enc == WIRE_S16) {
    const unsigned lo = ((unsigned)s[0] & 0xFFFFu) | ((unsigned)s[1] << 16);
    const unsigned hi = ((unsigned)s[2] & 0xFFFFu) | ((unsigned)s[3] << 16);
    reinterpret_cast<uint2*>(dst)[g] = make_uint2(lo, hi);
    return;
  }
  unsigned w = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) w |= (enc == WIRE_ULAW ? wire_ulaw(s[q]) : wire_alaw(s[q])) << (8 * q);
  reinterpret_cast<unsigned*>(dst)[g] = w;
}

// One workgroup per row walks the frames of the pass in order, so the row's history is read and
// written by this workgroup alone. LDS: the row's taps, and a window of the row's signal: the
// WIRE_TAIL samples before the frame | the frame. Output m needs x[j] for j >= (m down - half) /
// up, and the first output not yet emitted after N samples has m down + half >= N up: at most
// 2 half / up = 60 samples (8 kHz) before the frame. Two phases per frame: one output per lane
// into LDS (1,024 lanes: at most four tap chains in a row per lane and frame), then four outputs
// per lane encoded and stored as dwords. (With 256 lanes computing four outputs each, the launch
// took 59 / 85 us per four-frame pass of 32 rows at 8 / 48 kHz: the tap chain is latency bound.)
constexpr int WIRE_THREADS = 1024;
constexpr int WIRE_OUT_MAX = 3864;  // >= the largest piece's outputs, 3860 + 3 carried, and a multiple of 4
// A frame's input is (pointer, count): the PCM frame and 1920, or the row's tempo chunk. It is walked
// in pieces of at most 1920 samples (one piece for a PCM frame); a piece's outputs that do not fill
// a group of four are carried in s_y to the next piece, so every store stays a whole dword.
__global__ __launch_bounds__(WIRE_THREADS) void k_wire(WireArgs a) {
  __shared__ float s_taps[WIRE_TAPS_MAX];
  __shared__ __attribute__((aligned(16))) float s_x[WIRE_TAIL + 1920];
  __shared__ __attribute__((aligned(16))) float s_y[WIRE_OUT_MAX];
  const int b = blockIdx.x, t = threadIdx.x;
  const int fmt = a.fmt[b];
  const bool flac = (fmt & 0xFF) == WIRE_FLAC;  // uniform: 16-bit chunks, which k_flac encodes in place
  const int enc = flac ? WIRE_S16 : fmt & 0xFF, ri = fmt >> 8;
  int* cnt = a.counts + (long)b * a.out_frames;
  if (enc == WIRE_NONE || ri < 0 || ri >= WIRE_RATES) {  // uniform
    if (t < a.out_frames) cnt[t] = 0;
    return;
  }
  const WirePlan p = a.plan[ri];
  const bool identity = p.up == 1 && p.down == 1;
  if (!identity)
    for (int i = t; i < p.L; i += WIRE_THREADS) s_taps[i] = a.taps[p.tap_off + i];
  const int sp = a.tempo_sp ? a.tempo_sp[b] : 0;  // uniform: the row's input is its tempo chunk
  const unsigned pt = a.pitch_step ? a.pitch_step[b] : 0u;  // uniform: or its pitch chunk (behind the tempo stage)
  const unsigned lv = a.level_gain ? a.level_gain[b] : 0u;  // uniform: or its level chunk (behind both)
  const long cap = a.chunk / (enc == WIRE_S16 ? 2 : 1);  // samples a chunk slot holds
  long n = a.frames[b];  // input samples of the row received so far
  if (t < WIRE_TAIL) s_x[t] = n > 0 ? a.tail[(long)b * WIRE_TAIL + t] : 0.f;
  bool any = false;
  for (int f = 0; f < a.out_frames; ++f) {
    const FrameFlags fl = f < a.nfr ? a.flags[f][b] : FrameFlags{0, 0};
    if (!fl.valid) {  // uniform
      if (t == 0) cnt[f] = 0;
      continue;
    }
    any = true;
    const float* in = lv   ? a.lin + ((long)b * a.out_frames + f) * LEVEL_OUT_MAX
                      : pt ? a.pin + ((long)b * a.out_frames + f) * PITCH_OUT_MAX
                      : sp ? a.tin + ((long)b * a.out_frames + f) * TEMPO_OUT_MAX
                           : a.pcm + ((long)b * a.pcm_frames + f) * 1920;
    const int n_in = lv   ? min(max(a.lcnt[(long)b * a.out_frames + f], 0), LEVEL_OUT_MAX)
                     : pt ? min(max(a.pcnt[(long)b * a.out_frames + f], 0), PITCH_OUT_MAX)
                     : sp ? min(max(a.tcnt[(long)b * a.out_frames + f], 0), TEMPO_OUT_MAX)
                          : 1920;
    unsigned char* dst = a.out + ((long)b * a.out_frames + f) * a.chunk;
    long gbase = 0, total = 0;  // groups of four stored, samples of the chunk
    int rem = 0, done = 0;      // outputs carried in s_y[0, rem), inputs walked
    do {
      const int np = min(1920, n_in - done);
      const bool fin = done + np == n_in;
      __syncthreads();  // the previous piece's tail and carried outputs are in place
      const float4* src = reinterpret_cast<const float4*>(in + done);
      for (int i = t; 4 * i < np; i += WIRE_THREADS) reinterpret_cast<float4*>(s_x + WIRE_TAIL)[i] = src[i];
      __syncthreads();
      const long N0 = n, N1 = n + np;
      long m0 = N0, m1 = N1;
      if (!identity) {  // emitted(N) = floor((N up - 1 - half) / down) + 1 (0 before the first sample)
        m0 = N0 == 0 ? 0 : (N0 * p.up - 1 - p.half) / p.down + 1;
        m1 = fl.last && fin ? (N1 * p.up + p.down - 1) / p.down
                            : (N1 == 0 ? 0 : (N1 * p.up - 1 - p.half) / p.down + 1);
      }
      if (flac && a.first && done == 0 && t == 0) a.first[(long)b * a.out_frames + f] = (int)m0;
      // (never more: the chunk sizes of kernels.h)
      const long count = max(min(min(m1 - m0, (long)WIRE_OUT_MAX - rem), cap - 4 * gbase - rem), 0L);
      const long tot = rem + count;
      const long ng = fin ? (tot + 3) / 4 : tot / 4;
      for (long i = t; i < (fin ? 4 * ng : tot) - rem; i += WIRE_THREADS) {  // zeros pad the last dword
        const long m = m0 + i;
        float v = 0.f;
        if (i < count)
          v = identity ? s_x[WIRE_TAIL + (m - N0)]
                       : resample_out(s_x, N0 - WIRE_TAIL, N1, s_taps, p.L, p.up, p.down, p.half, m);
        s_y[rem + i] = v;
      }
      __syncthreads();
      for (long g = t; g < ng; g += WIRE_THREADS) {
        const float4 y4 = reinterpret_cast<const float4*>(s_y)[g];
        const float v[4] = {y4.x, y4.y, y4.z, y4.w};
        wire_store4(dst, gbase + g, enc, v);
      }
      if (fin) {
        total = 4 * gbase + tot;
      } else {  // uniform: the outputs past the last whole group move to the front of s_y
        const int left = (int)(tot - 4 * ng);
        const float v = t < left ? s_y[4 * ng + t] : 0.f;
        __syncthreads();
        if (t < left) s_y[t] = v;
        rem = left;
        gbase += ng;
      }
      n = N1;
      done += np;
      const float tv = t < WIRE_TAIL ? s_x[np + t] : 0.f;  // the last WIRE_TAIL samples of tail | piece
      __syncthreads();  // every lane has read the window
      if (t < WIRE_TAIL) s_x[t] = tv;
    } while (done < n_in);
    if (t == 0) cnt[f] = (int)total * (enc == WIRE_S16 ? 2 : 1);
  }
  if (!any) return;  // uniform
  if (t < WIRE_TAIL) a.tail[(long)b * WIRE_TAIL + t] = s_x[t];  // each lane wrote its own entry
  if (t == 0) a.frames[b] = (int)n;
}

void wire_stage(const WireArgs& a, hipStream_t s) {
  if (a.B < 1 || a.nfr < 1 || a.nfr > a.out_frames || a.out_frames > NFR_MAX || a.pcm_frames < a.nfr)
    throw std::runtime_error("wire_stage: bad pass shape");
  if (a.chunk < WIRE_CHUNK_MAX || a.chunk % 8 || (a.tempo_sp && (!a.tin || !a.tcnt || a.chunk < WIRE_CHUNK_MAX_TEMPO)) ||
      (a.pitch_step && (!a.tempo_sp || !a.pin || !a.pcnt)) ||
      (a.level_gain && (!a.lin || !a.lcnt || a.chunk < WIRE_CHUNK_MAX_LEVEL)))
    throw std::runtime_error("wire_stage: bad chunk slot");
  for (int r = 0; r < WIRE_RATES; ++r)
    if (a.plan[r].L > WIRE_TAPS_MAX || a.plan[r].L < 1 || 2 * a.plan[r].half > WIRE_TAIL * a.plan[r].up)
      throw std::runtime_error("wire_stage: plan outside the kernel's LDS window");
  hipLaunchKernelGGL(k_wire, dim3(a.B), dim3(WIRE_THREADS), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// FLAC stage (see kernels.h; the format and the choice rule are DESIGN.md section 21). Per block of
// at most FLAC_BLOCK samples, all in LDS: (1) sum the folded residuals' Rice costs per order, finest
// partition and parameter; (2) choose (order, partition order, parameters); (3) scan the code
// lengths over the workgroup and OR the codes into a zeroed bit buffer, whose words hold the
// stream's bytes big-endian; (4) CRC-16 as the XOR of per-lane run CRCs shifted by x^(8 bytes after);
// (5) byte-swapped dword stores. A frame starts at any byte, so the buffer starts at the dword that
// holds the frame's first byte and word 0 carries the bytes of the previous frame (`carry`).
constexpr int FLAC_THREADS = 1024, FLAC_PARTS = 64, FLAC_KS = 15, FLAC_ORDERS = 5;
constexpr int FLAC_SUMS = FLAC_ORDERS * FLAC_PARTS * FLAC_KS;
constexpr int FLAC_BITS_WORDS = (3 + FLAC_FRAME_OVERHEAD + 2 * FLAC_BLOCK + 3) / 4 + 2;
constexpr unsigned FLAC_COST_SAT = 1u << 24;  // > the verbatim cost of any block: 64 of them fit 32 bits
static_assert(FLAC_BITS_WORDS * 4 <= FLAC_SUMS * 8, "the bit buffer lives in the cost sums' LDS");
static_assert(8 + 16 * FLAC_BLOCK < FLAC_COST_SAT, "saturated partition costs change no decision");

// nbits <= 16 of val at bit `pos` of the stream held in buf (bit 31 of a word first)
__device__ __forceinline__ void flac_put(unsigned* buf, unsigned pos, int nbits, unsigned val) {
  const unsigned long long v = (unsigned long long)val << (64 - nbits - (int)(pos & 31));
  const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
  if ((pos >> 5) + 1 >= (unsigned)FLAC_BITS_WORDS) return;  // (never: a frame is at most 17 + 2 n bytes)
  if (hi) atomicOr(&buf[pos >> 5], hi);
  if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}
__device__ __forceinline__ unsigned flac_byte(const unsigned* buf, int y) {
  return (buf[y >> 2] >> (24 - 8 * (y & 3))) & 0xFFu;
}
// a b mod x^16 + x^15 + x^2 + 1
__device__ __forceinline__ unsigned flac_mulmod(unsigned a, unsigned b) {
  unsigned r = 0;
  for (int i = 15; i >= 0; --i) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x18005u;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// the residual of the fixed predictor of order o at sample i >= o
__device__ __forceinline__ int flac_residual(const short* s, int i, int o) {
  const int s0 = s[i];
  if (o == 0) return s0;
  const int s1 = s[i - 1];
  if (o == 1) return s0 - s1;
  const int s2 = s[i - 2];
  if (o == 2) return s0 - 2 * s1 + s2;
  const int s3 = s[i - 3];
  if (o == 3) return s0 - 3 * s1 + 3 * s2 - s3;
  return s0 - 4 * s1 + 6 * s2 - 4 * s3 + s[i - 4];
}
// the sum of v over each row of 16 lanes, in every lane of the row: four DPP rotations, no LDS
// round trip (a __shfl_xor tree costs one per step: 90 of them per order and segment were 75 % of
// the launch)
__device__ __forceinline__ unsigned flac_row_sum(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);  // row_ror:2
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);  // row_ror:1
  return v;
}
__device__ __forceinline__ unsigned flac_fold(int e) { return ((unsigned)e << 1) ^ (unsigned)(e >> 31); }
__device__ __forceinline__ int flac_number_bytes(long long v) {
  return v < (1LL << 7) ? 1 : v < (1LL << 11) ? 2 : v < (1LL << 16) ? 3 : v < (1LL << 21) ? 4
       : v < (1LL << 26) ? 5 : v < (1LL << 31) ? 6 : 7;
}

// The chunk s_x [n_total] (LDS) -> its frames at dst (dwords; may be the chunk's own global slot,
// which is not read here); returns their byte total. Called by every lane of a FLAC_THREADS workgroup.
// index (global, may be null): frame i's byte length and block size go to index[2 i], index[2 i + 1]
// for the ceil(n_total / FLAC_BLOCK) <= FLAC_CHUNK_FRAMES frames, from where the frame is stored.
__device__ int flac_chunk(const short* s_x, int n_total, int rc, long long first, unsigned* dst, int* index) {
  __shared__ unsigned long long s_sum[FLAC_SUMS];  // [order][finest partition][k], then prefix sums over partitions
  __shared__ unsigned s_pcost[FLAC_ORDERS][128];   // [order][(1 << p) - 1 + partition]: best cost, saturated
  __shared__ unsigned char s_pk[FLAC_ORDERS][128]; // and its parameter
  __shared__ unsigned s_cost[FLAC_ORDERS][7];
  __shared__ unsigned s_wsum[FLAC_THREADS / 64];
  __shared__ unsigned s_crc;
  unsigned* s_bits = reinterpret_cast<unsigned*>(s_sum);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  unsigned carry = 0;
  int boff = 0, total_bytes = 0;
  long wbase = 0;
  for (int off = 0; off < n_total; off += FLAC_BLOCK) {
    const short* s = s_x + off;
    const int n = min(FLAC_BLOCK, n_total - off);
    const int c = (n + FLAC_THREADS - 1) / FLAC_THREADS;  // consecutive samples per lane
    const int i0 = min(t * c, n), i1 = min(i0 + c, n);
    int diff = 0;
    for (int i = i0; i < i1; ++i) diff |= s[i] != s[0];
    __syncthreads();  // the previous block's stores have read the bit buffer
    for (int i = t; i < FLAC_SUMS; i += FLAC_THREADS) s_sum[i] = 0;
    if (t == 0) s_crc = 0;
    const bool varied = __syncthreads_or(diff) != 0;
    int pmax = -1;  // no candidate below 16 samples
    if (n >= 16) {
      pmax = min(__ffs(n) - 1, 6);
      while ((n >> pmax) < 16) --pmax;
    }
    int kind = 0, bo = 0, bp = 0;  // 0 CONSTANT, 1 VERBATIM, 2 FIXED
    if (varied) kind = 1;
    if (varied && pmax >= 0) {  // uniform
      // ---- (1) cost sums at the finest partitions. A segment is a run of samples inside one finest
      // partition (a whole one, or a 1 / S of it when there are fewer partitions than waves): at most
      // 288 samples, so a row's sum fits 32 bits. A wave strides over its segment, each row of 16
      // lanes reduces by DPP, and the rows' first lanes add into the partition's sums.
      const int P = 1 << pmax, psz = n >> pmax;
      const int S = P >= FLAC_THREADS / 64 ? 1 : FLAC_THREADS / 64 / P;
      for (int g = wv; g < P * S; g += FLAC_THREADS / 64) {  // uniform per wave
        const int j = g / S, r = g - j * S;
        const int a0 = j * psz + r * psz / S, a1 = j * psz + (r + 1) * psz / S;
#pragma unroll 1
        for (int o = 0; o < FLAC_ORDERS; ++o) {  // one order at a time: 15 sums in registers
          unsigned acc[FLAC_KS];
#pragma unroll
          for (int k = 0; k < FLAC_KS; ++k) acc[k] = 0;
          for (int i = max(a0, o) + lane; i < a1; i += 64) {  // the first o samples are warm-up
            const unsigned u = flac_fold(flac_residual(s, i, o));
#pragma unroll
            for (int k = 0; k < FLAC_KS; ++k) acc[k] += u >> k;
          }
#pragma unroll
          for (int k = 0; k < FLAC_KS; ++k) {
            const unsigned v = flac_row_sum(acc[k]);  // every lane holds the sum of its row of 16
            if ((lane & 15) == 0 && v) atomicAdd(&s_sum[(o * FLAC_PARTS + j) * FLAC_KS + k], (unsigned long long)v);
          }
        }
      }
      __syncthreads();
      if (t < FLAC_ORDERS * FLAC_KS) {  // inclusive prefix sums along the partitions: any partition is two reads
        const int o = t / FLAC_KS, k = t - o * FLAC_KS;
        unsigned long long run = 0;
        for (int j = 0; j < P; ++j) {
          run += s_sum[(o * FLAC_PARTS + j) * FLAC_KS + k];
          s_sum[(o * FLAC_PARTS + j) * FLAC_KS + k] = run;
        }
      }
      __syncthreads();
      // ---- (2) the best parameter of every partition of every (o, p), then the cost of every (o, p)
      if (t < FLAC_ORDERS * 128) {
        const int o = t >> 7, idx = t & 127;
        const int p = 31 - __clz(idx + 1), q = idx + 1 - (1 << p);
        if (idx < 127 && p <= pmax) {
          const int span = 1 << (pmax - p);
          const unsigned long long cnt = (unsigned)((n >> p) - (q == 0 ? o : 0));
          unsigned long long best = ~0ull;
          int bk = 0;
          for (int k = 0; k < FLAC_KS; ++k) {
            const unsigned long long sum = s_sum[(o * FLAC_PARTS + (q + 1) * span - 1) * FLAC_KS + k] -
                                           (q ? s_sum[(o * FLAC_PARTS + q * span - 1) * FLAC_KS + k] : 0ull);
            const unsigned long long cost = sum + cnt * (unsigned)(k + 1);
            if (cost < best) best = cost, bk = k;
          }
          best += 4;
          s_pcost[o][idx] = best < FLAC_COST_SAT ? (unsigned)best : FLAC_COST_SAT;
          s_pk[o][idx] = (unsigned char)bk;
        }
      }
      __syncthreads();
      if (t < FLAC_ORDERS * 7) {
        const int o = t / 7, p = t % 7;
        if (p <= pmax) {
          unsigned cost = 8 + 16 * o + 6;
          for (int q = 0; q < (1 << p); ++q) cost += s_pcost[o][(1 << p) - 1 + q];
          s_cost[o][p] = cost;
        }
      }
      __syncthreads();
      unsigned best = 8u + 16u * (unsigned)n;  // VERBATIM unless something is strictly cheaper
      for (int o = 0; o < FLAC_ORDERS; ++o)
        for (int p = 0; p <= pmax; ++p)
          if (s_cost[o][p] < best) best = s_cost[o][p], kind = 2, bo = o, bp = p;
    }
    __syncthreads();  // the sums are dead: their LDS becomes the bit buffer
    for (int i = t; i < FLAC_BITS_WORDS; i += FLAC_THREADS) s_bits[i] = i == 0 ? carry : 0u;
    __syncthreads();
    // ---- (3) header (lane 0), then the subframe's codes
    const long long v = first + off;
    const int nb = flac_number_bytes(v);
    const unsigned base = 8u * (unsigned)(boff + 4 + nb + (n <= 256 ? 1 : 2) + 1) + 8u;  // after the subframe header
    if (t == 0) {
      unsigned pos = 8u * (unsigned)boff, crc = 0;
      auto emit = [&](unsigned byte) {
        flac_put(s_bits, pos, 8, byte);
        pos += 8;
        crc ^= byte;
        for (int i = 0; i < 8; ++i) crc = (crc & 0x80u ? (crc << 1) ^ 0x07u : crc << 1) & 0xFFu;
      };
      emit(0xFFu);
      emit(0xF9u);
      emit(((n <= 256 ? 6u : 7u) << 4) | (unsigned)rc);
      emit(0x08u);
      if (nb == 1) {
        emit((unsigned)v);
      } else {
        emit(((0xFFu << (8 - nb)) & 0xFFu) | (unsigned)(nb == 7 ? 0 : v >> (6 * (nb - 1))));
        for (int i = nb - 2; i >= 0; --i) emit(0x80u | (unsigned)((v >> (6 * i)) & 0x3F));
      }
      if (n > 256) emit((unsigned)(n - 1) >> 8);
      emit((unsigned)(n - 1) & 0xFFu);
      const unsigned c8 = crc;
      emit(c8);
      flac_put(s_bits, pos, 8, kind == 0 ? 0u : kind == 1 ? 2u : (8u | (unsigned)bo) << 1);
      if (kind == 0) flac_put(s_bits, base, 16, (unsigned)s[0] & 0xFFFFu);
    }
    unsigned bits_end = base + 16;
    if (kind == 1) {
      for (int i = i0; i < i1; ++i) flac_put(s_bits, base + 16u * i, 16, (unsigned)s[i] & 0xFFFFu);
      bits_end = base + 16u * n;
    } else if (kind == 2) {
      const int pn = n >> bp;  // samples per partition
      const unsigned char* ks = &s_pk[bo][(1 << bp) - 1];
      unsigned mine = 0;
      for (int i = i0; i < i1; ++i) {
        if (i < bo) {
          mine += 16;
          continue;
        }
        const int k = ks[i / pn];
        mine += (flac_fold(flac_residual(s, i, bo)) >> k) + 1 + k + (i == bo ? 10 : i % pn == 0 ? 4 : 0);
      }
      unsigned incl = mine;  // exclusive scan of the lanes' bit counts over the workgroup
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
      }
      if (lane == 63) s_wsum[wv] = incl;
      __syncthreads();
      unsigned before = 0, all = 0;
      for (int w = 0; w < FLAC_THREADS / 64; ++w) {
        if (w < wv) before += s_wsum[w];
        all += s_wsum[w];
      }
      unsigned pos = base + before + incl - mine;
      for (int i = i0; i < i1; ++i) {
        if (i < bo) {
          flac_put(s_bits, pos, 16, (unsigned)s[i] & 0xFFFFu);
          pos += 16;
          continue;
        }
        const int k = ks[i / pn];
        if (i == bo) {  // 00 (Rice, 4-bit parameters) | partition order | the first parameter
          flac_put(s_bits, pos, 10, (unsigned)bp << 4 | (unsigned)k);
          pos += 10;
        } else if (i % pn == 0) {
          flac_put(s_bits, pos, 4, (unsigned)k);
          pos += 4;
        }
        const unsigned u = flac_fold(flac_residual(s, i, bo));
        pos += u >> k;  // the unary zeros are already there
        flac_put(s_bits, pos, k + 1, 1u << k | (u & ((1u << k) - 1)));
        pos += k + 1;
      }
      bits_end = base + all;
    }
    __syncthreads();
    // ---- (4) CRC-16 over bytes [boff, eb) of the buffer
    const int eb = min((int)((bits_end + 7) >> 3), boff + FLAC_FRAME_OVERHEAD - 2 + 2 * n);  // (never the bound)
    {
      const int len = eb - boff, run = (len + FLAC_THREADS - 1) / FLAC_THREADS;
      const int y0 = min(boff + t * run, eb), y1 = min(y0 + run, eb);
      unsigned crc = 0;
      for (int y = y0; y < y1; ++y) {
        crc ^= flac_byte(s_bits, y) << 8;
        for (int i = 0; i < 8; ++i) crc = (crc & 0x8000u ? (crc << 1) ^ 0x8005u : crc << 1) & 0xFFFFu;
      }
      unsigned pw = 0x100u;  // x^8, squared per bit of the byte count after the run
      for (int m = eb - y1; m > 0 && crc; m >>= 1) {
        if (m & 1) crc = flac_mulmod(crc, pw);
        pw = flac_mulmod(pw, pw);
      }
      for (int d = 32; d >= 1; d >>= 1) crc ^= __shfl_xor(crc, d);
      if (lane == 0 && crc) atomicXor(&s_crc, crc);
    }
    __syncthreads();
    if (t == 0) flac_put(s_bits, 8u * (unsigned)eb, 16, s_crc);
    __syncthreads();
    // ---- (5) the whole dwords leave; the rest is carried into the next frame's first word
    const int tb = eb + 2, nfull = tb >> 2;
    for (int w = t; w < nfull; w += FLAC_THREADS) dst[wbase + w] = __builtin_bswap32(s_bits[w]);
    carry = tb & 3 ? s_bits[nfull] : 0u;
    wbase += nfull;
    total_bytes += tb - boff;
    if (index && t == 0) {
      index[2 * (off / FLAC_BLOCK)] = tb - boff;
      index[2 * (off / FLAC_BLOCK) + 1] = n;
    }
    boff = tb & 3;
  }
  if (boff && t == 0) dst[wbase] = __builtin_bswap32(carry);  // zeros pad the last dword (inside the slot)
  return total_bytes;
}

__global__ __launch_bounds__(FLAC_THREADS) void k_flac(FlacArgs a) {
  __shared__ __attribute__((aligned(16))) short s_x[(FLAC_CHUNK_SAMPLES + 7) / 8 * 8];
  const int b = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
  const int fmt = a.fmt[b], ri = fmt >> 8;
  const long idx = (long)b * a.out_frames + f;
  // k_wire's 16-bit chunk (never more than the frames of which fit the slot: the chunk sizes of kernels.h)
  int n = 0;
  if ((fmt & 0xFF) == WIRE_FLAC && ri >= 0 && ri < WIRE_RATES)  // uniform
    n = min(min(a.counts[idx] / 2, (a.chunk - FLAC_CHUNK_FRAMES * FLAC_FRAME_OVERHEAD) / 2), FLAC_CHUNK_SAMPLES);
  if (t == 0) a.nframes[idx] = n > 0 ? (n + FLAC_BLOCK - 1) / FLAC_BLOCK : 0;  // no FLAC row, or no chunk: 0
  if (n <= 0) return;
  unsigned* slot = reinterpret_cast<unsigned*>(a.out + idx * a.chunk);
  for (int i = t; i < (n + 1) / 2; i += FLAC_THREADS) reinterpret_cast<unsigned*>(s_x)[i] = slot[i];
  __syncthreads();
  const int bytes = flac_chunk(s_x, n, flac_rate_code(ri), a.first[idx], slot, a.index + idx * (2 * FLAC_CHUNK_FRAMES));
  if (t == 0) a.counts[idx] = bytes;
}

void flac_stage(const FlacArgs& a, hipStream_t s) {
  if (a.B < 1 || a.out_frames < 1 || a.out_frames > NFR_MAX || !a.fmt || !a.first || !a.out || !a.counts ||
      !a.index || !a.nframes)
    throw std::runtime_error("flac_stage: bad pass shape");
  if (a.chunk < WIRE_CHUNK_MAX || a.chunk % 8 || a.chunk > WIRE_CHUNK_MAX_LEVEL)
    throw std::runtime_error("flac_stage: bad chunk slot");
  hipLaunchKernelGGL(k_flac, dim3(a.B, a.out_frames), dim3(FLAC_THREADS), 0, s, a);
}

__global__ __launch_bounds__(FLAC_THREADS) void k_flac_encode(const short* __restrict__ x, int n, int rc,
                                                              long long first, unsigned* out, int* n_bytes,
                                                              int* index) {
  __shared__ __attribute__((aligned(16))) short s_x[(FLAC_CHUNK_SAMPLES + 7) / 8 * 8];
  for (int i = threadIdx.x; i < n; i += FLAC_THREADS) s_x[i] = x[i];
  __syncthreads();
  const int bytes = flac_chunk(s_x, n, rc, first, out, index);
  if (threadIdx.x == 0) *n_bytes = bytes;
}
void flac_encode(const short* x, int n, int rate_index, long long first_sample, unsigned char* out, int* n_bytes,
                 int* index, hipStream_t s) {
  if (n < 1 || n > FLAC_CHUNK_SAMPLES || rate_index < 0 || rate_index >= WIRE_RATES || first_sample < 0 ||
      first_sample + n > (1LL << 36))
    throw std::runtime_error("flac_encode: bad chunk");
  hipLaunchKernelGGL(k_flac_encode, dim3(1), dim3(FLAC_THREADS), 0, s, x, n, flac_rate_code(rate_index), first_sample,
                     reinterpret_cast<unsigned*>(out), n_bytes, index);
}

// ---------------------------------------------------------------------------------------------
// Tempo stage (see kernels.h; the rule is DESIGN.md section 19). The hop functions are templates on
// how a sample is read: the streaming kernel's LDS window, or the whole signal in global memory.
// The streaming window lives in LDS with its four index phases apart: sample u of the window is at
// (u & 3) * TEMPO_WQ + (u >> 2), so lanes that read samples four apart (tempo_search: four shifts
// per lane) read consecutive words. quad(j, p): p[r][m * STRIDE] is x[j + 4 m + r].
constexpr int TEMPO_WQ = (TEMPO_HIST + 1920) / 4;  // 780 words per phase
struct TempoWindow {  // sample u of s is x[base + u]; n samples received so far (x reads 0 from n on)
  const float* s;
  long base, n;
  static constexpr int STRIDE = 1;
  __device__ __forceinline__ static int pos(int u) { return (u & 3) * TEMPO_WQ + (u >> 2); }
  __device__ __forceinline__ float raw(long j) const { return s[pos((int)(j - base))]; }
  __device__ __forceinline__ float operator()(long j) const { return j >= base && j < n ? raw(j) : 0.f; }
  __device__ __forceinline__ bool inside(long j, int len) const { return j >= base && j + len <= n; }
  __device__ __forceinline__ void quad(long j, const float* p[4]) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = s + pos((int)(j - base) + r);
  }
};
struct TempoSignal {
  const float* x;
  long n;
  static constexpr int STRIDE = 4;
  __device__ __forceinline__ float raw(long j) const { return x[j]; }
  __device__ __forceinline__ float operator()(long j) const { return j >= 0 && j < n ? x[j] : 0.f; }
  __device__ __forceinline__ bool inside(long j, int len) const { return j >= 0 && j + len <= n; }
  __device__ __forceinline__ void quad(long j, const float* p[4]) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = x + j + r;
  }
};
constexpr int TEMPO_THREADS = 1024;
constexpr int TEMPO_CAND = 2 * TEMPO_D + 1;       // 241 shifts
constexpr int TEMPO_QLEN = TEMPO_W / 4;           // 120 products per quarter
constexpr int TEMPO_NG = (TEMPO_CAND + 3) / 4;    // 61 groups of four consecutive shifts
static_assert(4 * TEMPO_NG <= TEMPO_THREADS && TEMPO_CAND <= 256 && TEMPO_QLEN % 4 == 0, "tempo_search's lanes");

// p_k of hop k >= 1. Lane q * 61 + g runs quarter q of the four shifts 4 g - D .. 4 g - D + 3: four
// independent 120-long f64 chains that share each template word and slide over one new signal
// word per product (964 lanes with one chain each took 5 us a hop: two LDS reads and two
// conversions per product, LDS bound; this takes a quarter of both). Each chain is still the
// ascending sum of its quarter. The quarters are added in order, and the largest sum wins, the
// earliest in the scan order 0, -1, +1, .. among equal ones. s_c [4 * TEMPO_CAND], s_v / s_r [256].
template <class X>
__device__ __forceinline__ long tempo_search(const X& x, long a, long pprev, double* s_c, double* s_v, int* s_r) {
  const int t = threadIdx.x;
  if (t < 4 * TEMPO_NG) {
    const int q = t / TEMPO_NG, c0 = 4 * (t - q * TEMPO_NG);
    const long xa = a + (c0 - TEMPO_D) + q * TEMPO_QLEN, ta = pprev + TEMPO_HS + q * TEMPO_QLEN;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    if (x.inside(xa, TEMPO_QLEN + 3) && x.inside(ta, TEMPO_QLEN)) {
      const float *xp[4], *tp[4];
      x.quad(xa + 3, xp);
      x.quad(ta, tp);
      double x0 = (double)x.raw(xa), x1 = (double)x.raw(xa + 1), x2 = (double)x.raw(xa + 2);
#pragma unroll 5
      for (int m = 0; m < TEMPO_QLEN / 4; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // product i = 4 m + r of the four chains
          const double x3 = (double)xp[r][m * X::STRIDE], tv = (double)tp[r][m * X::STRIDE];
          acc0 += x0 * tv;
          acc1 += x1 * tv;
          acc2 += x2 * tv;
          acc3 += x3 * tv;
          x0 = x1, x1 = x2, x2 = x3;
        }
      }
    } else {  // a window that crosses the utterance's end (zeros) or its start
      double x0 = (double)x(xa), x1 = (double)x(xa + 1), x2 = (double)x(xa + 2);
      for (int i = 0; i < TEMPO_QLEN; ++i) {
        const double x3 = (double)x(xa + 3 + i), tv = (double)x(ta + i);
        acc0 += x0 * tv;
        acc1 += x1 * tv;
        acc2 += x2 * tv;
        acc3 += x3 * tv;
        x0 = x1, x1 = x2, x2 = x3;
      }
    }
    double* c = s_c + q * TEMPO_CAND + c0;
    c[0] = acc0;  // (c0 <= 240: the first shift of a group always exists)
    if (c0 + 1 < TEMPO_CAND) c[1] = acc1;
    if (c0 + 2 < TEMPO_CAND) c[2] = acc2;
    if (c0 + 3 < TEMPO_CAND) c[3] = acc3;
  }
  __syncthreads();
  if (t < 256) {
    double v = -INFINITY;
    int r = 1 << 30;
    if (t < TEMPO_CAND) {
      v = ((s_c[t] + s_c[TEMPO_CAND + t]) + s_c[2 * TEMPO_CAND + t]) + s_c[3 * TEMPO_CAND + t];
      const int d = t - TEMPO_D;
      r = d == 0 ? 0 : d < 0 ? -2 * d - 1 : 2 * d;  // place in the scan order
    }
    s_v[t] = v;
    s_r[t] = r;
  }
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      const double v2 = s_v[t + h];
      const int r2 = s_r[t + h];
      if (v2 > s_v[t] || (v2 == s_v[t] && r2 < s_r[t])) {
        s_v[t] = v2;
        s_r[t] = r2;
      }
    }
    __syncthreads();
  }
  const int r = min(s_r[0], 2 * TEMPO_D);
  return a + (r == 0 ? 0 : (r & 1) ? -(r + 1) / 2 : r / 2);
}

// `count` output samples of hop k (the products are exact in f64: one rounding, to f32)
template <class X>
__device__ __forceinline__ void tempo_ola(const X& x, const float* w, long k, long p, long pprev, int count,
                                          float* out) {
  const int i = threadIdx.x;
  if (i >= count) return;
  out[i] = k == 0 ? x(p + i)
                  : (float)((double)w[i] * (double)x(p + i) +
                            (double)w[TEMPO_HS + i] * (double)x(pprev + TEMPO_HS + i));
}

__global__ __launch_bounds__(TEMPO_THREADS) void k_tempo(TempoArgs a) {
  __shared__ float s_x[4 * TEMPO_WQ];  // the window, by phase (TempoWindow)
  __shared__ float s_w[TEMPO_W];
  __shared__ double s_c[4 * TEMPO_CAND];
  __shared__ double s_v[256];
  __shared__ int s_r[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int sp = a.sp[b];
  int* cnt = a.counts + (long)b * a.out_frames;
  if (sp < TEMPO_SP_MIN || sp > TEMPO_SP_MAX) {  // uniform: a row without speed
    if (t < a.out_frames) cnt[t] = 0;
    return;
  }
  if (t < TEMPO_W) s_w[t] = a.win[t];
  int* st = a.state + (long)b * TEMPO_STATE;
  long nf = st[0], k = st[1], pprev = st[2];
  for (int i = t; i < TEMPO_HIST; i += TEMPO_THREADS)
    s_x[TempoWindow::pos(i)] = nf > 0 ? a.hist[(long)b * TEMPO_HIST + i] : 0.f;
  bool any = false;
  for (int f = 0; f < a.out_frames; ++f) {
    const FrameFlags fl = f < a.nfr ? a.flags[f][b] : FrameFlags{0, 0};
    if (!fl.valid) {  // uniform
      if (t == 0) cnt[f] = 0;
      continue;
    }
    any = true;
    __syncthreads();  // the history is in place
    const float4* src = reinterpret_cast<const float4*>(a.pcm + ((long)b * a.pcm_frames + f) * 1920);
    for (int i = t; i < 480; i += TEMPO_THREADS) {  // samples TEMPO_HIST + 4 i + r: word TEMPO_HIST / 4 + i of phase r
      const float4 v = src[i];
      s_x[0 * TEMPO_WQ + TEMPO_HIST / 4 + i] = v.x;
      s_x[1 * TEMPO_WQ + TEMPO_HIST / 4 + i] = v.y;
      s_x[2 * TEMPO_WQ + TEMPO_HIST / 4 + i] = v.z;
      s_x[3 * TEMPO_WQ + TEMPO_HIST / 4 + i] = v.w;
    }
    __syncthreads();
    const long N0 = nf * 1920, N = N0 + 1920;
    const TempoWindow x{s_x, N0 - TEMPO_HIST, N};
    const long L = (N * 1000 + sp - 1) / sp;
    float* out = a.out + ((long)b * a.out_frames + f) * TEMPO_OUT_MAX;
    int emitted = 0;
    for (;;) {  // uniform: the hops this frame completes
      const long ak = k * TEMPO_HS * sp / 1000;
      if (fl.last ? k * TEMPO_HS >= L : ak + TEMPO_R > N) break;
      const int count = fl.last ? (int)min((long)TEMPO_HS, L - k * TEMPO_HS) : TEMPO_HS;
      if (emitted + count > TEMPO_OUT_MAX) break;  // (never: the bound of kernels.h)
      const long p = k > 0 ? tempo_search(x, ak, pprev, s_c, s_v, s_r) : 0;
      tempo_ola(x, s_w, k, p, pprev, count, out + emitted);
      emitted += count;
      pprev = p;
      ++k;
    }
    if (t == 0) cnt[f] = emitted;
    nf += 1;
    __syncthreads();  // every lane has read the window
    // the window moves on by 1920 samples, 480 words of each phase (1920 >= TEMPO_HIST: disjoint)
    for (int i = t; i < TEMPO_HIST; i += TEMPO_THREADS) s_x[TempoWindow::pos(i)] = s_x[TempoWindow::pos(i) + 480];
  }
  if (!any) return;  // uniform
  for (int i = t; i < TEMPO_HIST; i += TEMPO_THREADS)  // own entries
    a.hist[(long)b * TEMPO_HIST + i] = s_x[TempoWindow::pos(i)];
  if (t == 0) {
    st[0] = (int)nf;
    st[1] = (int)k;
    st[2] = (int)pprev;
  }
}

void tempo_stage(const TempoArgs& a, hipStream_t s) {
  static_assert(TEMPO_HIST <= 1920 && TEMPO_HIST % 4 == 0 && TEMPO_OUT_MAX % 4 == 0, "k_tempo's window");
  if (a.B < 1 || a.nfr < 1 || a.nfr > a.out_frames || a.out_frames > NFR_MAX || a.pcm_frames < a.nfr)
    throw std::runtime_error("tempo_stage: bad pass shape");
  hipLaunchKernelGGL(k_tempo, dim3(a.B), dim3(TEMPO_THREADS), 0, s, a);
}

__global__ __launch_bounds__(TEMPO_THREADS) void k_tempo_whole(const float* __restrict__ xs, long n, int sp,
                                                              const float* __restrict__ win, float* __restrict__ y) {
  __shared__ float s_w[TEMPO_W];
  __shared__ double s_c[4 * TEMPO_CAND];
  __shared__ double s_v[256];
  __shared__ int s_r[256];
  const int t = threadIdx.x;
  if (t < TEMPO_W) s_w[t] = win[t];
  __syncthreads();
  const TempoSignal x{xs, n};
  const long L = (n * 1000 + sp - 1) / sp;
  long pprev = 0;
  for (long k = 0; k * TEMPO_HS < L; ++k) {
    const long ak = k * TEMPO_HS * sp / 1000;
    const int count = (int)min((long)TEMPO_HS, L - k * TEMPO_HS);
    const long p = k > 0 ? tempo_search(x, ak, pprev, s_c, s_v, s_r) : 0;
    tempo_ola(x, s_w, k, p, pprev, count, y + k * TEMPO_HS);
    pprev = p;
  }
}

long tempo_len(long n, int sp) { return (n * 1000 + sp - 1) / sp; }

std::vector<float> tempo_window() {
  std::vector<float> w(TEMPO_W);
  for (int i = 0; i < TEMPO_W; ++i) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / TEMPO_W));
  return w;
}

void tempo(const float* x, int n, int sp, const float* win, float* y, hipStream_t s) {
  if (n < 1 || sp < TEMPO_SP_MIN || sp > TEMPO_SP_MAX) throw std::runtime_error("tempo: bad arguments");
  hipLaunchKernelGGL(k_tempo_whole, dim3(1), dim3(TEMPO_THREADS), 0, s, x, (long)n, sp, win, y);
}

// ---------------------------------------------------------------------------------------------
// Pitch stage (see kernels.h; the rule is DESIGN.md section 23). The tap loop is a template on how a
// sample is read (the LDS window of the stream, or the whole signal), so the streaming stage and the
// seam are equal by construction. The prototype table (128 KB, shared by all rows, read-only) is
// read through the cache.
struct PitchWindow {  // sample j of the row is s[j - base], base <= j < n (0 outside [0, n))
  const float* s;
  long base, n;
  __device__ __forceinline__ float operator()(long j) const { return j >= base && j >= 0 && j < n ? s[j - base] : 0.f; }
};
struct PitchSignal {
  const float* __restrict__ x;
  long n;
  __device__ __forceinline__ float operator()(long j) const { return j >= 0 && j < n ? x[j] : 0.f; }
};

// Output m: one ascending f64 chain over j = i0 - H .. i0 + H. Taps outside the signal or past the
// table's support contribute u * 0 or 0 * h, which leaves the f64 sum as it is, so they are skipped.
// Every product (f32 x 20 bits, f32 x f32) is exact in f64: contraction cannot change a bit.
template <class X>
__device__ __forceinline__ float pitch_out(const X& x, const float2* __restrict__ tab, long m, unsigned step, long cq,
                                           int H) {
  const long pos = m * (long)step, i0 = pos >> 20;
  const long jlo = max(i0 - H, 0L), jhi = min(i0 + H, x.n - 1);
  double acc = 0.0;
#pragma unroll 4
  for (long j = jlo; j <= jhi; ++j) {
    const long dd = pos - j * (1L << 20);
    const long q = ((dd < 0 ? -dd : dd) * cq) >> 20;
    const long qp = q * PITCH_P, ti = qp >> 20;
    if (ti >= PITCH_Z * PITCH_P) continue;
    const float2 td = tab[ti];
    const double fr = (double)(qp & ((1L << 20) - 1)) * (1.0 / 1048576.0);
    const float h = (float)((double)td.x + (double)td.y * fr);
    acc += (double)x(j) * (double)h;
  }
  return (float)(acc * ((double)cq * (1.0 / 1048576.0)));
}

// One workgroup per row walks the pass's frames in order, so the row's state is touched by this
// workgroup alone. LDS: the last PITCH_HIST inputs | the frame's input (a PCM frame or a tempo
// chunk). Lanes take whole outputs: a chunk is up to PITCH_OUT_MAX independent chains of at most
// 2 H + 1 products, five or six per lane, whose table loads do not depend on the running sum.
constexpr int PITCH_THREADS = 1024;
__global__ __launch_bounds__(PITCH_THREADS) void k_pitch(PitchArgs a) {
  __shared__ __attribute__((aligned(16))) float s_x[PITCH_HIST + TEMPO_OUT_MAX];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned step = a.step[b];
  int* cnt = a.counts + (long)b * a.out_frames;
  if (step < PITCH_STEP_MIN || step > PITCH_STEP_MAX) {  // uniform: a row without pitch
    if (t < a.out_frames) cnt[t] = 0;
    return;
  }
  const long cq = pitch_cq(step);
  const int H = pitch_support(step);
  const int sp = a.tempo_sp[b];  // uniform: the row's input is its tempo chunk
  int* st = a.state + (long)b * PITCH_STATE;
  long n = st[0], e = st[1];  // inputs received, outputs emitted
  if (t < PITCH_HIST) s_x[t] = n > 0 ? a.hist[(long)b * PITCH_HIST + t] : 0.f;
  bool any = false;
  for (int f = 0; f < a.out_frames; ++f) {
    const FrameFlags fl = f < a.nfr ? a.flags[f][b] : FrameFlags{0, 0};
    if (!fl.valid) {  // uniform
      if (t == 0) cnt[f] = 0;
      continue;
    }
    any = true;
    const float* in = sp ? a.tin + ((long)b * a.out_frames + f) * TEMPO_OUT_MAX
                         : a.pcm + ((long)b * a.pcm_frames + f) * 1920;
    const int n_in = sp ? min(max(a.tcnt[(long)b * a.out_frames + f], 0), TEMPO_OUT_MAX) : 1920;
    __syncthreads();  // the history is in place
    for (int i = t; 4 * i < n_in; i += PITCH_THREADS)
      reinterpret_cast<float4*>(s_x + PITCH_HIST)[i] = reinterpret_cast<const float4*>(in)[i];
    __syncthreads();
    const long N1 = n + n_in;
    // emitted(N) = ceil((N - H) 2^20 / step): every m with (m step >> 20) + H <= N - 1
    long e1 = fl.last ? (N1 << 20) / step : (N1 > H ? (((N1 - H) << 20) + step - 1) / step : 0);
    e1 = min(max(e1, e), e + PITCH_OUT_MAX);  // (never more: the chunk bound of kernels.h)
    const int count = (int)(e1 - e);
    const PitchWindow x{s_x, n - PITCH_HIST, N1};
    float* out = a.out + ((long)b * a.out_frames + f) * PITCH_OUT_MAX;
    for (int i = t; i < count; i += PITCH_THREADS)
      out[i] = pitch_out(x, reinterpret_cast<const float2*>(a.tab), e + i, step, cq, H);
    if (t == 0) cnt[f] = count;
    const float hv = t < PITCH_HIST ? s_x[n_in + t] : 0.f;  // the last PITCH_HIST samples of history | input
    __syncthreads();  // every lane has read the window
    if (t < PITCH_HIST) s_x[t] = hv;
    n = N1;
    e = e1;
  }
  if (!any) return;  // uniform
  if (t < PITCH_HIST) a.hist[(long)b * PITCH_HIST + t] = s_x[t];  // each lane wrote its own entry
  if (t == 0) {
    st[0] = (int)n;
    st[1] = (int)e;
  }
}

void pitch_stage(const PitchArgs& a, hipStream_t s) {
  static_assert(TEMPO_OUT_MAX % 4 == 0 && TEMPO_OUT_MAX >= 1920 && PITCH_HIST >= 2 * PITCH_H_MAX, "k_pitch's window");
  if (a.B < 1 || a.nfr < 1 || a.nfr > a.out_frames || a.out_frames > NFR_MAX || a.pcm_frames < a.nfr)
    throw std::runtime_error("pitch_stage: bad pass shape");
  if (!a.step || !a.tempo_sp || !a.tin || !a.tcnt || !a.state || !a.hist || !a.tab || !a.out || !a.counts)
    throw std::runtime_error("pitch_stage: null argument");
  hipLaunchKernelGGL(k_pitch, dim3(a.B), dim3(PITCH_THREADS), 0, s, a);
}

__global__ __launch_bounds__(256) void k_pitch_whole(const float* __restrict__ xs, long n, unsigned step,
                                                     const float2* __restrict__ tab, long L, float* __restrict__ y) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= L) return;
  const PitchSignal x{xs, n};
  y[m] = pitch_out(x, tab, m, step, pitch_cq(step), pitch_support(step));
}

bool pitch_plan(int cents, int sp, int* sp_w, unsigned* step) {
  if (sp == 0) sp = 1000;
  if (cents < -PITCH_CENTS_MAX || cents > PITCH_CENTS_MAX || sp < TEMPO_SP_MIN || sp > TEMPO_SP_MAX) return false;
  const long st = std::llround(std::exp2((double)cents / 1200.0) * 1048576.0);
  const long w = (((long)sp << 20) + st / 2) / st;
  if (w < TEMPO_SP_MIN || w > TEMPO_SP_MAX) return false;
  if (sp_w) *sp_w = (int)w;
  if (step) *step = (unsigned)st;
  return true;
}

long pitch_len(long n, unsigned step) { return (n << 20) / step; }

// T[i] = f32(sinc(i / P) kaiser(i / (P Z))) in f64, exactly 0 at the sinc's zeros and past Z P;
// D[i] = f32(T[i + 1] - T[i]); interleaved (T[i], D[i]) so a tap is one 8-byte load
std::vector<float> pitch_table() {
  std::vector<float> T(PITCH_TAB + 1, 0.f);
  const double i0b = bessel_i0(PITCH_BETA);
  for (int i = 0; i < PITCH_Z * PITCH_P; ++i) {
    if (i == 0) {
      T[i] = 1.f;
      continue;
    }
    if (i % PITCH_P == 0) continue;
    const double v = (double)i / PITCH_P, r = (double)i / ((double)PITCH_P * PITCH_Z);
    T[i] = (float)(std::sin(M_PI * v) / (M_PI * v) * (bessel_i0(PITCH_BETA * std::sqrt(1.0 - r * r)) / i0b));
  }
  std::vector<float> tab(2 * (size_t)PITCH_TAB);
  for (int i = 0; i < PITCH_TAB; ++i) {
    tab[2 * i] = T[i];
    tab[2 * i + 1] = (float)((double)T[i + 1] - (double)T[i]);
  }
  return tab;
}

void pitch_resample(const float* x, int n, unsigned step, const float* tab, float* y, hipStream_t s) {
  if (n < 1 || step < PITCH_STEP_MIN || step > PITCH_STEP_MAX) throw std::runtime_error("pitch_resample: bad arguments");
  const long L = pitch_len(n, step);
  if (L < 1) return;
  hipLaunchKernelGGL(k_pitch_whole, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, x, (long)n, step,
                     reinterpret_cast<const float2*>(tab), L, y);
}

// ---------------------------------------------------------------------------------------------
// Level stage (see kernels.h; the rule is DESIGN.md section 24). One window function serves the
// streaming stage and the whole-signal seam, so they are equal by construction. The window holds u
// of W consecutive samples (0 outside the signal, where the rule says r = 1, which is what u = 0
// gives); outputs q0 <= q < q0 + count of it replace u[q] by y in place. It needs q0 >= LEVEL_L and
// q0 + count + LEVEL_L <= W: output q reads r[q - L .. q + L].
//   r: one lane per sample. m: the minimum over 127 by doubling in place (windows of 2, 4, .. 64,
// then two windows of 64 that overlap by one), each step read into registers, barrier, written.
//   g: 127 f64 multiply-adds per output in ascending k; every product (24 bits times an integer of
// at most 64) is exact, so contraction changes no bit.
constexpr int LEVEL_THREADS = 1024;
constexpr int LEVEL_PER_LANE = (LEVEL_WINDOW + LEVEL_THREADS - 1) / LEVEL_THREADS;  // 6
__device__ __forceinline__ void level_window(float* s_u, float* s_r, int W, int q0, int count, float C, int t) {
  for (int p = t; p < W; p += LEVEL_THREADS) {
    const float a = fabsf(s_u[p]);
    s_r[p] = a > C ? __fdiv_rn(C, a) : 1.0f;
  }
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < 7; ++step) {  // uniform
    const int sh = step < 6 ? 1 << step : 63;
    float v[LEVEL_PER_LANE];
#pragma unroll
    for (int i = 0; i < LEVEL_PER_LANE; ++i) {
      const int p = t + i * LEVEL_THREADS;
      v[i] = p < W ? fminf(s_r[p], p + sh < W ? s_r[p + sh] : 1.0f) : 1.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LEVEL_PER_LANE; ++i) {
      const int p = t + i * LEVEL_THREADS;
      if (p < W) s_r[p] = v[i];
    }
    __syncthreads();
  }
  // s_r[p] = min(r[p .. p + L]) (r = 1 past the window)
  for (int i = t; i < count; i += LEVEL_THREADS) {
    const int q = q0 + i;
    double acc = 0.0;
#pragma unroll 9
    for (int k = 0; k <= LEVEL_L; ++k) acc += (double)(64 - abs(k - 63)) * (double)s_r[q - k];
    const float g = (float)(acc * (1.0 / 4096.0));
    const float y = g * s_u[q];
    s_u[q] = fminf(fmaxf(y, -C), C);
  }
  __syncthreads();
}

// One workgroup per row walks the pass's frames in order, so the row's history is read and written
// by this workgroup alone. LDS: u of the last LEVEL_HIST samples | the frame's input | L zeros, and
// r / m of the same window. A frame that is not the last emits the outputs below N - L.
__global__ __launch_bounds__(LEVEL_THREADS) void k_level(LevelArgs a) {
  __shared__ __attribute__((aligned(16))) float s_u[LEVEL_WINDOW + 2];
  __shared__ __attribute__((aligned(16))) float s_r[LEVEL_WINDOW + 2];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned gb = a.gain[b];
  int* cnt = a.counts + (long)b * a.out_frames;
  if (gb == 0u) {  // uniform: a row that is not in the stage
    if (t < a.out_frames) cnt[t] = 0;
    return;
  }
  const float v = __uint_as_float(gb), C = a.ceiling;
  const int sp = a.tempo_sp ? a.tempo_sp[b] : 0;                // uniform: the row's input, as k_wire chooses it
  const unsigned pt = a.pitch_step ? a.pitch_step[b] : 0u;
  long n = a.state[(long)b * LEVEL_STATE];  // inputs received
  if (t < LEVEL_HIST) s_u[t] = n > 0 ? a.hist[(long)b * LEVEL_HIST + t] : 0.f;
  bool any = false;
  for (int f = 0; f < a.out_frames; ++f) {
    const FrameFlags fl = f < a.nfr ? a.flags[f][b] : FrameFlags{0, 0};
    if (!fl.valid) {  // uniform
      if (t == 0) cnt[f] = 0;
      continue;
    }
    any = true;
    const float* in = pt   ? a.pin + ((long)b * a.out_frames + f) * PITCH_OUT_MAX
                      : sp ? a.tin + ((long)b * a.out_frames + f) * TEMPO_OUT_MAX
                           : a.pcm + ((long)b * a.pcm_frames + f) * 1920;
    const int n_in = pt   ? min(max(a.pcnt[(long)b * a.out_frames + f], 0), PITCH_OUT_MAX)
                     : sp ? min(max(a.tcnt[(long)b * a.out_frames + f], 0), TEMPO_OUT_MAX)
                          : 1920;
    __syncthreads();  // the history is in place
    for (int i = t; 4 * i < n_in; i += LEVEL_THREADS) {  // u = v x (the slots are padded to four)
      const float4 x4 = reinterpret_cast<const float4*>(in)[i];
      reinterpret_cast<float4*>(s_u + LEVEL_HIST)[i] = make_float4(v * x4.x, v * x4.y, v * x4.z, v * x4.w);
    }
    __syncthreads();  // (a count that is no multiple of four: the zeros below overwrite the excess)
    if (t < LEVEL_L + 2) s_u[LEVEL_HIST + n_in + t] = 0.f;
    __syncthreads();
    const float hv = t < LEVEL_HIST ? s_u[n_in + t] : 0.f;  // the last LEVEL_HIST values of history | input
    const long N1 = n + n_in;
    const long e0 = max(n - LEVEL_L, 0L), e1 = fl.last ? N1 : max(N1 - LEVEL_L, 0L);
    const int count = (int)min(max(e1 - e0, 0L), (long)LEVEL_OUT_MAX);  // (never more: n_in + L)
    const int q0 = (int)(e0 - (n - LEVEL_HIST));  // L, or 2 L - n while the row has fewer than L inputs
    level_window(s_u, s_r, LEVEL_HIST + n_in + LEVEL_L, q0, count, C, t);
    float* out = a.out + ((long)b * a.out_frames + f) * LEVEL_OUT_MAX;
    for (int i = t; 4 * i < count; i += LEVEL_THREADS) {  // zeros pad the last group (inside the slot)
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = 4 * i + j < count ? s_u[q0 + 4 * i + j] : 0.f;
      reinterpret_cast<float4*>(out)[i] = make_float4(y[0], y[1], y[2], y[3]);
    }
    if (t == 0) cnt[f] = count;
    __syncthreads();  // every lane has read the window
    if (t < LEVEL_HIST) s_u[t] = hv;
    n = N1;
  }
  if (!any) return;  // uniform
  if (t < LEVEL_HIST) a.hist[(long)b * LEVEL_HIST + t] = s_u[t];  // each lane wrote its own entry
  if (t == 0) a.state[(long)b * LEVEL_STATE] = (int)n;
}

void level_stage(const LevelArgs& a, hipStream_t s) {
  if (a.B < 1 || a.nfr < 1 || a.nfr > a.out_frames || a.out_frames > NFR_MAX || a.pcm_frames < a.nfr)
    throw std::runtime_error("level_stage: bad pass shape");
  if (!a.pcm || !a.gain || !a.state || !a.hist || !a.out || !a.counts || (a.tempo_sp && (!a.tin || !a.tcnt)) ||
      (a.pitch_step && (!a.pin || !a.pcnt)) || !(a.ceiling > 0.f && a.ceiling <= 1.f))
    throw std::runtime_error("level_stage: bad argument");
  hipLaunchKernelGGL(k_level, dim3(a.B), dim3(LEVEL_THREADS), 0, s, a);
}

// the seam: a workgroup per LEVEL_TILE outputs, its window the 2 L samples before and L after them
constexpr int LEVEL_TILE = LEVEL_WINDOW - LEVEL_HIST - LEVEL_L;
__global__ __launch_bounds__(LEVEL_THREADS) void k_level_whole(const float* __restrict__ x, long n, float v, float C,
                                                               float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float s_u[LEVEL_WINDOW + 2];
  __shared__ __attribute__((aligned(16))) float s_r[LEVEL_WINDOW + 2];
  const int t = threadIdx.x;
  const long n0 = (long)blockIdx.x * LEVEL_TILE;
  const int count = (int)min((long)LEVEL_TILE, n - n0);
  const int W = LEVEL_HIST + count + LEVEL_L;
  for (int p = t; p < W; p += LEVEL_THREADS) {
    const long j = n0 - LEVEL_HIST + p;
    s_u[p] = j >= 0 && j < n ? v * x[j] : 0.f;
  }
  __syncthreads();
  level_window(s_u, s_r, W, LEVEL_HIST, count, C, t);
  for (int i = t; i < count; i += LEVEL_THREADS) y[n0 + i] = s_u[LEVEL_HIST + i];
}

bool level_plan(int gain_cdb, int ceiling_cdb, float* gain, float* ceiling) {
  if (gain_cdb < -LEVEL_GAIN_CDB_MAX || gain_cdb > LEVEL_GAIN_CDB_MAX || ceiling_cdb < LEVEL_CEIL_CDB_MIN || ceiling_cdb > 0)
    return false;
  if (gain) *gain = (float)std::pow(10.0, (double)gain_cdb / 2000.0);
  if (ceiling) *ceiling = (float)std::pow(10.0, (double)ceiling_cdb / 2000.0);
  return true;
}

void level(const float* x, long n, float gain, float ceiling, float* y, hipStream_t s) {
  if (n < 1 || !(gain > 0.f) || !(ceiling > 0.f && ceiling <= 1.f)) throw std::runtime_error("level: bad arguments");
  hipLaunchKernelGGL(k_level_whole, dim3((unsigned)((n + LEVEL_TILE - 1) / LEVEL_TILE)), dim3(LEVEL_THREADS), 0, s, x, n,
                     gain, ceiling, y);
}

// ---------------------------------------------------------------------------------------------
// Loudness stage (see kernels.h; the rule is DESIGN.md section 27). One block function serves the
// streaming stage and the whole-signal seam, so they are equal by construction. It takes nb <= 3
// sub-blocks of f32 samples from LDS, starting at a sub-block boundary of the row, and the six
// doubles of filter state at that boundary, and leaves the nb energies and the state at the end.
//   One lane per segment (at most 225 of 256) keeps its 32 samples in registers through both
// biquads: zero-state pass, correction, zero-state pass, correction, squares. Between them lane 0
// walks the chain of (e1, e2) over the segments from the last two zero-state values of each; the
// shelf's chain values are also the high-pass's x[n - 1], x[n - 2] at each segment start. The work is
// a few thousand dependent f64 operations; nothing here is bandwidth.
//   No operation may be contracted: the functions below state `fp contract(off)` and use plain
// operators (the __dmul_rn family is plain operators compiled elsewhere, which would not carry it).
constexpr int LOUD_THREADS = 256;
constexpr int LOUD_LANES = LOUD_BLOCKS_MAX * LOUD_SEGS;  // 225
static_assert(LOUD_LANES <= LOUD_THREADS, "a lane per segment of the largest window");
// the window in LDS: sample i at i + i / 32, so that lanes reading a segment each hit banks of their own
__device__ __forceinline__ int loud_at(int i) { return i + (i >> 5); }
constexpr int LOUD_WINDOW = LOUD_SUB - 1 + LOUD_IN_MAX;            // 8127 samples
constexpr int LOUD_WINDOW_LDS = LOUD_WINDOW + LOUD_WINDOW / 32 + 2;

// z[k] = ((((b0 x[k] + b1 x[k-1]) + b2 x[k-2]) - a1 z[k-1]) - a2 z[k-2]) with z = 0 before the segment
__device__ __forceinline__ void loud_zero_state(const double* c, double x1, double x2, double (&v)[LOUD_G]) {
#pragma clang fp contract(off)
  double z1 = 0.0, z2 = 0.0;
#pragma unroll
  for (int k = 0; k < LOUD_G; ++k) {
    const double x = v[k];
    double acc = c[0] * x + c[1] * x1;
    acc = acc + c[2] * x2;
    acc = acc - c[3] * z1;
    acc = acc - c[4] * z2;
    x2 = x1, x1 = x;
    z2 = z1, z1 = acc;
    v[k] = acc;
  }
}
// y[k] = (z[k] + p[k] e1) + q[k] e2
__device__ __forceinline__ void loud_correct(const double* p, const double* q, double e1, double e2, double (&v)[LOUD_G]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < LOUD_G; ++k) v[k] = (v[k] + p[k] * e1) + q[k] * e2;
}
// lane 0: e[s + 1] = y of the last two samples of segment s, from e[s] and that segment's zero-state values
__device__ __forceinline__ void loud_chain(const double* p, const double* q, const double* za, const double* zb,
                                           double* e1s, double* e2s, double e1, double e2, int S) {
#pragma clang fp contract(off)
  const double p1 = p[LOUD_G - 1], q1 = q[LOUD_G - 1], p2 = p[LOUD_G - 2], q2 = q[LOUD_G - 2];
  e1s[0] = e1, e2s[0] = e2;
#pragma unroll 5
  for (int s = 0; s < S; ++s) {
    const double n1 = (za[s] + p1 * e1) + q1 * e2;
    const double n2 = (zb[s] + p2 * e1) + q2 * e2;
    e1 = n1, e2 = n2;
    e1s[s + 1] = e1, e2s[s + 1] = e2;
  }
}

struct LoudLds {
  double za[LOUD_LANES], zb[LOUD_LANES];            // z[31], z[30] of each segment (one biquad at a time)
  double e1[2][LOUD_LANES + 1], e2[2][LOUD_LANES + 1];  // per biquad: y[-1], y[-2] at each segment start, and at the end
  double seg[LOUD_LANES];                           // sum of y^2 of each segment
  double f[LOUD_FILT];                              // the filter state at the window's start, then at its end
  double E[LOUD_BLOCKS_MAX];
};

// uniform: every lane of the workgroup calls it (barriers inside); 1 <= nb <= LOUD_BLOCKS_MAX
__device__ __forceinline__ void loud_window(const float* s_x, int nb, LoudLds& L, const LoudCoef& K, int t) {
  const int S = nb * LOUD_SEGS;
  const bool on = t < S;
  double v[LOUD_G];
  double x1 = 0.0, x2 = 0.0;
  double nx1 = 0.0, nx2 = 0.0;  // (lane S - 1: the inputs the next window starts behind)
  if (on) {
#pragma unroll
    for (int k = 0; k < LOUD_G; ++k) v[k] = (double)s_x[loud_at(t * LOUD_G + k)];
    x1 = t ? (double)s_x[loud_at(t * LOUD_G - 1)] : L.f[0];
    x2 = t ? (double)s_x[loud_at(t * LOUD_G - 2)] : L.f[1];
    nx1 = v[LOUD_G - 1], nx2 = v[LOUD_G - 2];
  }
#pragma unroll
  for (int bq = 0; bq < 2; ++bq) {
    if (on) {
      loud_zero_state(K.c[bq], x1, x2, v);
      L.za[t] = v[LOUD_G - 1], L.zb[t] = v[LOUD_G - 2];
    }
    __syncthreads();
    if (t == 0) loud_chain(K.pq[bq][0], K.pq[bq][1], L.za, L.zb, L.e1[bq], L.e2[bq], L.f[2 + 2 * bq], L.f[3 + 2 * bq], S);
    __syncthreads();
    if (on) {
      x1 = L.e1[bq][t], x2 = L.e2[bq][t];  // this biquad's outputs ahead of the segment: the next one's inputs
      loud_correct(K.pq[bq][0], K.pq[bq][1], x1, x2, v);
    }
  }
  if (on) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < LOUD_G; ++k) acc = acc + v[k] * v[k];
    L.seg[t] = acc;
  }
  __syncthreads();
  if (t < nb) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int s = 0; s < LOUD_SEGS; ++s) acc = acc + L.seg[t * LOUD_SEGS + s];
    L.E[t] = acc;
  }
  if (t == S - 1) L.f[0] = nx1, L.f[1] = nx2;
  if (t == 0) {
    L.f[2] = L.e1[0][S], L.f[3] = L.e2[0][S];
    L.f[4] = L.e1[1][S], L.f[5] = L.e2[1][S];
  }
  __syncthreads();
}

// One workgroup per row walks the pass's frames in order, so the row's state is read and written by
// this workgroup alone. LDS: the samples behind the row's last complete sub-block | the frame's input.
__global__ __launch_bounds__(LOUD_THREADS) void k_loud(LoudArgs a) {
  __shared__ float s_x[LOUD_WINDOW_LDS];
  __shared__ LoudLds L;
  const int b = blockIdx.x, t = threadIdx.x;
  LoudRecord* rec = a.out + (long)b * a.out_frames;
  if (a.state[(long)b * LOUD_STATE] == 0) {  // uniform: a row that is not metered
    if (t < a.out_frames) rec[t].n_blocks = 0;
    return;
  }
  const int sp = a.tempo_sp ? a.tempo_sp[b] : 0;  // uniform: the row's input, as k_wire chooses it
  const unsigned pt = a.pitch_step ? a.pitch_step[b] : 0u;
  const unsigned lv = a.level_gain ? a.level_gain[b] : 0u;
  long seen = a.state[(long)b * LOUD_STATE + 1];
  int np = (int)(seen % LOUD_SUB);  // samples behind the last complete sub-block
  for (int i = t; i < np; i += LOUD_THREADS) s_x[loud_at(i)] = a.pend[(long)b * LOUD_SUB + i];
  if (t < LOUD_FILT) L.f[t] = seen >= LOUD_SUB ? a.filt[(long)b * LOUD_FILT + t] : 0.0;
  bool any = false;
  for (int f = 0; f < a.out_frames; ++f) {
    const FrameFlags fl = f < a.nfr ? a.flags[f][b] : FrameFlags{0, 0};
    if (!fl.valid) {  // uniform
      if (t == 0) rec[f].n_blocks = 0;
      continue;
    }
    any = true;
    const float* in = lv   ? a.lin + ((long)b * a.out_frames + f) * LEVEL_OUT_MAX
                      : pt ? a.pin + ((long)b * a.out_frames + f) * PITCH_OUT_MAX
                      : sp ? a.tin + ((long)b * a.out_frames + f) * TEMPO_OUT_MAX
                           : a.pcm + ((long)b * a.pcm_frames + f) * 1920;
    const int n_in = lv   ? min(max(a.lcnt[(long)b * a.out_frames + f], 0), LEVEL_OUT_MAX)
                     : pt ? min(max(a.pcnt[(long)b * a.out_frames + f], 0), PITCH_OUT_MAX)
                     : sp ? min(max(a.tcnt[(long)b * a.out_frames + f], 0), TEMPO_OUT_MAX)
                          : 1920;
    for (int i = t; i < n_in; i += LOUD_THREADS) s_x[loud_at(np + i)] = in[i];
    __syncthreads();  // the window and the state are in place
    const int total = np + n_in, nb = total / LOUD_SUB;  // nb <= LOUD_BLOCKS_MAX: np < LOUD_SUB, n_in <= LOUD_IN_MAX
    if (nb > 0) {  // uniform
      loud_window(s_x, nb, L, a.k, t);
      if (t < nb) rec[f].e[t] = L.E[t];
      const int rem = total - nb * LOUD_SUB;
      constexpr int PER = (LOUD_SUB + LOUD_THREADS - 1) / LOUD_THREADS;
      float keep[PER];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int i = t + j * LOUD_THREADS;
        keep[j] = i < rem ? s_x[loud_at(nb * LOUD_SUB + i)] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int i = t + j * LOUD_THREADS;
        if (i < rem) s_x[loud_at(i)] = keep[j];
      }
      np = rem;
    } else {
      np = total;
    }
    if (t == 0) rec[f].n_blocks = nb;
    seen += n_in;
  }
  if (!any) return;  // uniform
  __syncthreads();
  for (int i = t; i < np; i += LOUD_THREADS) a.pend[(long)b * LOUD_SUB + i] = s_x[loud_at(i)];
  if (t < LOUD_FILT && seen >= LOUD_SUB) a.filt[(long)b * LOUD_FILT + t] = L.f[t];
  if (t == 0) a.state[(long)b * LOUD_STATE + 1] = (int)seen;
}

void loud_stage(const LoudArgs& a, hipStream_t s) {
  if (a.B < 1 || a.nfr < 1 || a.nfr > a.out_frames || a.out_frames > NFR_MAX || a.pcm_frames < a.nfr)
    throw std::runtime_error("loud_stage: bad pass shape");
  if (!a.pcm || !a.state || !a.pend || !a.filt || !a.out || (a.tempo_sp && (!a.tin || !a.tcnt)) ||
      (a.pitch_step && (!a.pin || !a.pcnt)) || (a.level_gain && (!a.lin || !a.lcnt)))
    throw std::runtime_error("loud_stage: bad argument");
  hipLaunchKernelGGL(k_loud, dim3(a.B), dim3(LOUD_THREADS), 0, s, a);
}

// the seam: one workgroup walks the signal in windows of three sub-blocks from a zero state
__global__ __launch_bounds__(LOUD_THREADS) void k_loud_whole(const float* __restrict__ x, long n_blocks, LoudCoef k,
                                                             double* __restrict__ energy) {
  __shared__ float s_x[LOUD_WINDOW_LDS];
  __shared__ LoudLds L;
  const int t = threadIdx.x;
  if (t < LOUD_FILT) L.f[t] = 0.0;
  for (long w = 0; w < n_blocks; w += LOUD_BLOCKS_MAX) {
    const int nb = (int)min((long)LOUD_BLOCKS_MAX, n_blocks - w);
    for (int i = t; i < nb * LOUD_SUB; i += LOUD_THREADS) s_x[loud_at(i)] = x[w * LOUD_SUB + i];
    __syncthreads();
    loud_window(s_x, nb, L, k, t);
    if (t < nb) energy[w + t] = L.E[t];
  }
}

void loud_coef(LoudCoef* k) {
#pragma clang fp contract(off)
  const double fs = 24000.0, pi = 3.141592653589793;
  {  // the shelf
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    k->c[0][0] = (Vh + Vb * K / Q + K * K) / a0;
    k->c[0][1] = 2.0 * (K * K - Vh) / a0;
    k->c[0][2] = (Vh - Vb * K / Q + K * K) / a0;
    k->c[0][3] = 2.0 * (K * K - 1.0) / a0;
    k->c[0][4] = (1.0 - K / Q + K * K) / a0;
  }
  {  // the high-pass
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
    k->c[1][0] = 1.0, k->c[1][1] = -2.0, k->c[1][2] = 1.0;
    k->c[1][3] = 2.0 * (K * K - 1.0) / a0;
    k->c[1][4] = (1.0 - K / Q + K * K) / a0;
  }
  for (int bq = 0; bq < 2; ++bq)
    for (int w = 0; w < 2; ++w) {  // p from (y1, y2) = (1, 0), q from (0, 1)
      double y1 = w == 0 ? 1.0 : 0.0, y2 = w == 0 ? 0.0 : 1.0;
      for (int i = 0; i < LOUD_G; ++i) {
        const double m1 = -k->c[bq][3] * y1, m2 = k->c[bq][4] * y2;
        const double v = m1 - m2;
        k->pq[bq][w][i] = v;
        y2 = y1, y1 = v;
      }
    }
}

void loud_blocks(const float* x, long n, const LoudCoef& k, double* energy, hipStream_t s) {
  if (n < LOUD_SUB) throw std::runtime_error("loud_blocks: no complete sub-block");
  hipLaunchKernelGGL(k_loud_whole, dim3(1), dim3(LOUD_THREADS), 0, s, x, n / LOUD_SUB, k, energy);
}

// whole-signal encode of n samples (already at the wire rate), four per lane
__global__ __launch_bounds__(256) void k_wire_encode(const float* __restrict__ x, long n, int enc,
                                                     unsigned char* __restrict__ out) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (4 * g >= n) return;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = 4 * g + q < n ? x[4 * g + q] : 0.f;
  wire_store4(out, g, enc, v);
}
void wire_encode(const float* x, long n, int enc, unsigned char* out, hipStream_t s) {
  if (n <= 0) return;
  if (enc != WIRE_S16 && enc != WIRE_ULAW && enc != WIRE_ALAW) throw std::runtime_error("wire_encode: encoding");
  hipLaunchKernelGGL(k_wire_encode, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, x, n, enc, out);
}

// dst[c][r][:] = src[c * chunk_stride + :] for c < nch, r < rows: the replicate padding of every
// encoder chunk's first row in one launch (ConvDownsample1d, conv.rs:116-123).
__global__ __launch_bounds__(256) void k_replicate_chunks(const float* __restrict__ src, long chunk_stride,
                                                          float* __restrict__ dst, int nch, int rows, int cols) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)nch * rows * cols) return;
  const int col = (int)(idx % cols), c = (int)(idx / ((long)rows * cols));
  dst[idx] = src[(long)c * chunk_stride + col];
}
void replicate_chunks(const float* src, long chunk_stride, float* dst, int nch, int rows, int cols, hipStream_t s) {
  const long total = (long)nch * rows * cols;
  if (total > 0)
    hipLaunchKernelGGL(k_replicate_chunks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, chunk_stride,
                       dst, nch, rows, cols);
}

// ---------------------------------------------------------------------------------------------
// rubato FastFixedIn / Septic (see kernels.h): the Lagrange weights of nodes -3..4 at frac as
// prefix x suffix products of (frac - node), each times 1 / prod_{m != j} (j - m) =
// (-1)^(7-j) / (j! (7-j)!); the sum over the 8 taps in tap order. The oracle's orc_resample_septic
// performs the same f32 operations in the same order (contraction off on both sides), so the two
// agree bit for bit; lanes of a wave read overlapping 8-sample windows (L1/L2 hits).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float septic_eval(const float* __restrict__ x, int n_in, int s, float f) {
#pragma clang fp contract(off)
  constexpr float inv_den[8] = {-1.f / 5040.f, 1.f / 720.f, -1.f / 240.f, 1.f / 144.f,
                                -1.f / 144.f,  1.f / 240.f, -1.f / 720.f, 1.f / 5040.f};
  float d[8], pre[8], suf[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) d[m] = f - (float)(m - 3);
  pre[0] = 1.f;
#pragma unroll
  for (int m = 1; m < 8; ++m) pre[m] = pre[m - 1] * d[m - 1];
  suf[7] = 1.f;
#pragma unroll
  for (int m = 6; m >= 0; --m) suf[m] = suf[m + 1] * d[m + 1];
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = s - 3 + j;
    const float v = (i >= 0 && i < n_in) ? x[i] : 0.f;
    acc = acc + v * ((pre[j] * suf[j]) * inv_den[j]);
  }
  return acc;
}

__global__ __launch_bounds__(256) void k_resample_septic(const float* __restrict__ x, int n_in,
                                                         const int* __restrict__ start,
                                                         const float* __restrict__ frac, int n_out, int n_pad,
                                                         float* __restrict__ y) {
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_pad) return;
  y[m] = m < n_out ? septic_eval(x, n_in, start[m], frac[m]) : 0.f;
}

long septic_schedule(long n, int sr_from, int sr_to, std::vector<int>* start, std::vector<float>* frac) {
  if (n <= 0 || sr_from <= 0 || sr_to <= 0) return 0;
  const double ratio = (double)sr_to / (double)sr_from;  // audio.rs:213
  const double t = 1.0 / ratio;                          // dt_ratio is 0 at a fixed ratio
  const double end = (double)(n - 9);                    // chunk_size - (POLYNOMIAL_LEN + 1)
  double idx = -4.0;                                     // last_index = -(POLYNOMIAL_LEN / 2)
  long cnt = 0;
  if (start) start->clear();
  if (frac) frac->clear();
  while (idx < end) {
    idx += t;
    const double fl = std::floor(idx);
    if (start) start->push_back((int)fl);
    if (frac) frac->push_back((float)(idx - fl));
    ++cnt;
  }
  return cnt;
}

void resample_septic(const float* x, int n_in, const int* start, const float* frac, int n_out, int n_pad, float* y,
                     hipStream_t s) {
  if (n_pad <= 0) return;
  hipLaunchKernelGGL(k_resample_septic, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, x, n_in, start, frac,
                     n_out, n_pad, y);
}

// =============================================================================================
// Flow-head chain in ONE persistent launch (mlp.rs:146-213, 370-383; flow_lm.rs:7-22): for every
// lsd Euler step, input projection -> 6 ResBlocks -> FinalLayer -> x += v / N. As separate
// launches this is 28 GEMM + row-reduce kernels of M = B rows x 512 (each ~1 MB of weights), a
// chain of launch gaps and HBM round trips. Here a grid of ceil(B/16) row groups x 32 column
// groups (16 rows x 16 output columns per workgroup, 8 waves splitting K = 512) runs the chain
// with in-launch hand-offs in which the data is its own flag (the tag-free form of the granule
// hand-off, cdna_hip_programming.md Guideline 16 R2):
//   every hand-off has its own region, filled with 0xFFFFFFFF (a NaN no arithmetic produces) by
//   the launch just ahead (k_row_reduce's side job in the adaLN reduce);
//   producer: the storing wave writes its 16x16 tile with sc1 (write-through) 16-B buffer stores
//             and moves on (no drain, no counter);
//   consumer: each wave sweeps its 16 rows x 64 columns with sc1 buffer loads and re-reads every
//             float4 that still holds the empty pattern (bounded spin) - a 4-byte word is read
//             either empty or final, so a word that is not empty is the producer's value.
// Each workgroup keeps its 16x16 tile of the residual stream x in registers for the whole chain;
// consumers rebuild the full rows (LayerNorm statistics need all 512 columns) from the published
// copy. Weights, LayerNorm affines and adaLN modulations do not depend on the chain and are
// loaded before each wait. The latent `cur` between Euler steps (lsd > 1) is handed off with a
// counter (sc1 stores, drain, agent-scope add); counters are zeroed at allocation and re-armed by
// the last workgroup to finish.
// v_mfma_f32_16x16x4_f32 fragments as in k_attn16: lane (c = l & 15, G = l >> 4) supplies
// A[row c][k] and B[k][col c] for k = 64*wave + FH_KJ*(s/4) + 4*G + s%4 at step s (FH_KJ below); D reg g -> row 4G+g, col c.
// =============================================================================================
constexpr int FH_WAVES = 8;  // FH_D, FH_L, FH_DEPTH: kernels.h
// k layout of a lane's 16 values: float4 j of lane group G holds k = 64 wave + FH_KJ j + 4 G ..+3,
// so the 4 lane groups of a row read 64 contiguous bytes per load instruction (16 rows x 64 B
// per instruction instead of 16 rows x four 16-B pieces 64 B apart). A and B use the same k
// order, so the MFMA sum is over the same products.
constexpr int FH_KJ = 16;
// consumer offsets of float4 j in a hand-off region: the 16 columns of j sit in the next column
// group's 16x16 tile, 1 KB on
constexpr int FH_SJ = 16 * 16 * 4;

__device__ __forceinline__ float4 f4ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
// consumer: this lane's 16 values of a region (byte offset `off`), re-read until none is empty.
// The loop condition is wave-uniform; a timeout sets *err and stops waiting for the rest of the
// launch (the frame is poisoned, fetch() reports it).
__device__ __forceinline__ void fh_sweep(__amdgpu_buffer_rsrc_t r, int off, float4 (&v)[4], int* err, bool& dead) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = fh_ld(r, off + FH_SJ * j);
  unsigned spins = 0;
  while (!dead) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok &= !fh_empty(v[j]);
    if (__all(ok)) break;
    __builtin_amdgcn_s_sleep(1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (fh_empty(v[j])) v[j] = fh_ld(r, off + FH_SJ * j);
    if (++spins > (1u << 20)) {
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      dead = true;
    }
  }
}

// LayerNorm (eps 1e-6, optional affine) + adaLN modulate (mlp.rs:29-58,135-137) of this lane's
// 16 values of row c. Row statistics in ONE workgroup barrier: each wave contributes its 64
// values' sum and squared deviations about their own mean, combined as M2 = sum_w [M2_w +
// 64 (mean_w - mean)^2] (Chan et al.'s pairwise update; the same two-pass variance, summed in a
// different order), in a fixed wave order.
// The affines (lnw, lnb: LDS, this lane's k range; nullptr for none) are read after the barrier,
// so the prologue's LDS fill needs no barrier of its own.
__device__ __forceinline__ void fh_ln(float4 (&v)[4], float (*s_st)[FH_WAVES][16], int wave, int c, int G,
                                      const float* lnw, const float* lnb, const float4 (&sc)[4],
                                      const float4 (&sf)[4]) {
  float s1 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s1 += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  s1 += __shfl_xor(s1, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  const float mw = s1 * (1.0f / 64.0f);
  float m2 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = v[j].x - mw, b = v[j].y - mw, d = v[j].z - mw, e = v[j].w - mw;
    m2 += (a * a + b * b) + (d * d + e * e);
  }
  m2 += __shfl_xor(m2, 16, 64);
  m2 += __shfl_xor(m2, 32, 64);
  if (G == 0) {
    s_st[0][wave][c] = s1;
    s_st[1][wave][c] = m2;
  }
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < FH_WAVES; ++w) tot += s_st[0][w][c];
  const float mean = tot / (float)FH_D;
  float q = 0.f;
#pragma unroll
  for (int w = 0; w < FH_WAVES; ++w) {
    const float dm = s_st[0][w][c] * (1.0f / 64.0f) - mean;
    q += s_st[1][w][c] + 64.0f * dm * dm;
  }
  const float rden = 1.0f / sqrtf(q / (float)FH_D + 1e-6f);  // one divide, then multiplies (<= 1 ulp apart)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float4 h = make_float4((v[j].x - mean) * rden, (v[j].y - mean) * rden, (v[j].z - mean) * rden,
                           (v[j].w - mean) * rden);
    if (lnw) h = f4add(f4mul(h, f4ld(lnw + FH_KJ * j)), f4ld(lnb + FH_KJ * j));
    v[j] = make_float4(h.x * (1.0f + sc[j].x) + sf[j].x, h.y * (1.0f + sc[j].y) + sf[j].y,
                       h.z * (1.0f + sc[j].z) + sf[j].z, h.w * (1.0f + sc[j].w) + sf[j].w);
  }
}
// 16 MFMA steps over this lane's k range, then the 8 wave partials summed in wave order; wave 0
// lane t returns the 16x16 tile's row t/4, columns 4(t%4)..+3
// (consecutive GEMMs alternate between two s_red buffers: no barrier is needed between wave 0's
// reads of one and the other waves' writes of the next)
__device__ __forceinline__ float4 fh_gemm(const float4 (&a)[4], const float4 (&b)[4], float (*s_red)[16][16],
                                          int wave, int c, int G, int lane) {
  // four independent accumulator chains (one per float4 of the lane's k range), summed after:
  // the dependent chain of 16 MFMAs was the phase's longest serial step
  floatx4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b[j].x, floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b[j].y, acc[j], 0, 0, 0);
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b[j].z, acc[j], 0, 0, 0);
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b[j].w, acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) s_red[wave][4 * G + g][c] = (acc[0][g] + acc[1][g]) + (acc[2][g] + acc[3][g]);
  __syncthreads();
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < FH_WAVES; ++w) r = f4add(r, f4ld(&s_red[w][lane >> 2][4 * (lane & 3)]));
  }
  return r;
}

// Operands of one phase, loaded a phase ahead of their use (non-publishing waves right after the
// current phase's payload loads, the publishing wave 0 right after its publish, so that neither
// the payload wait nor the publish drain waits for them): the lane's 16-k slice of one weight
// row, and for LayerNorm phases the adaLN scale / shift of the lane's row.
struct FhOps {
  float4 w[4], sc[4], sf[4];
  float4 e0, e1;  // wave 0 epilogue: bias | gate, bias
};

__global__ __launch_bounds__(64 * FH_WAVES) void k_flow_head(FlowHeadArgs a) {
  front_prio();
  __shared__ float s_st[2][FH_WAVES][16];
  __shared__ __attribute__((aligned(16))) float s_red2[2][FH_WAVES][16][16];
  __shared__ __attribute__((aligned(16))) float s_ln[FH_DEPTH][2][FH_D];  // ResBlock LayerNorm affines
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, G = lane >> 4;
  const int RG = (a.B + 15) / 16;
  // XCD-aware placement (speed only: blocks b and b + 8 are observed to share an XCD's L2): the
  // RG row groups of a column group sit on one XCD, so each weight fragment is fetched into that
  // L2 once and read by all RG of them (column groups 4x .. 4x+3 on XCD slot x)
  const int xs = blockIdx.x & 7, xr = blockIdx.x >> 3;
  const int rg = xr % RG, cg = 4 * xs + xr / RG;
  const int col0 = 16 * cg;
  const int arow = min(16 * rg + c, a.B - 1);  // A-operand row of this lane (clamped; rows >= B unused)
  const int k0 = 64 * wave + 4 * G;            // this lane's 16 k: k0 + FH_KJ j + 0..3, j < 4
  const int orow = 16 * rg + (lane >> 2);      // epilogue (wave 0): row, columns ocol..ocol+3
  const int ocol = col0 + 4 * (lane & 3);
  const int crow = min(orow, a.B - 1);
  const bool ostore = orow < a.B;
  const bool fin = cg < FH_L / 16;  // column groups 0 and 1 own the 32 latent columns
  // the epilogue row's own Euler step count and step size (wave 0 of the latent column groups),
  // loaded here with the launch's first operands: nothing of it waits behind a sweep. The step
  // loop's trip count stays a.lsd for every row (the hand-offs need every workgroup in every phase).
  const int n_row = fin && wave == 0 ? max(a.st[crow].lsd, 1) : 1;
  const float e_row = 1.0f / (float)n_row;
  const __amdgpu_buffer_rsrc_t hr = fh_rsrc(a.hx), cr = fh_rsrc(a.cur);
  int* cc = a.ctr + 4 * rg + 2;  // cur published (lsd > 1)
  const int rstride = RG * 16 * FH_D * 4;  // bytes per hand-off region
  // sweep / store byte offsets in a hand-off region ([RG][32][16][16]: tile (rg, cg) is one KB):
  // lane (c, G) of wave w reads row c, columns 16 (4w + j) + 4G..+3 of its row group; wave 0 lane
  // t stores its tile's row t/4, columns 4(t%4)..+3 at tile offset 16 t bytes
  const int aoff = (((rg * 32 + 4 * wave) * 16 + (arow - 16 * rg)) * 16 + 4 * G) * 4;
  const int ooff = ((rg * 32 + cg) * 256 + 4 * lane) * 4;
  int q = 0;   // next hand-off region
  int gi = 0;  // GEMMs done (s_red buffer parity)
  bool dead = false;
  float4 xo = make_float4(0.f, 0.f, 0.f, 0.f);  // wave 0: residual tile x[orow][ocol..+3]
  int sk = 0;
#ifdef PTTS_PROBES  // s_memrealtime stamps of workgroups 0-3 (tools/head_stamps.py)
#define FH_STAMP()                                                                     \
  if (a.dbg && tid == 0 && blockIdx.x < 4 && sk < 120) a.dbg[blockIdx.x * 128 + sk++] = __builtin_amdgcn_s_memrealtime()
#else
#define FH_STAMP() (void)sk
#endif
  // probe layout: [entry, x0 published, 6 x 8 ResBlock stamps, final: swept, done]
  FH_STAMP();

  // operand loaders (i: ResBlock, or FH_DEPTH for the FinalLayer)
  // fragment-packed matrix m (2i: w0 of ResBlock i, 2i + 1: its w2, 12: fin_w), this lane's float4 j
  const float* wpl = a.wp + ((long)cg * FH_WAVES + wave) * 4 * 256 + 4 * lane;
  auto wfrag = [&](int m, int j) { return f4ld(wpl + (long)m * (32 * FH_WAVES * 4 * 256) + j * 256); };
  auto load_ln_ops = [&](FhOps& o, const float* mods, int i, int stp) {
    if (i == FH_DEPTH && !fin) return;
    const float* mp = a.fhm + (((((long)(stp * RG + rg) * (FH_DEPTH + 1) + i) * 2) * 8 + wave) * 4 * 64 + lane) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o.w[j] = wfrag(2 * i, j);
      o.sf[j] = f4ld(mp + j * 256);
      o.sc[j] = f4ld(mp + 8 * 4 * 256 + j * 256);
    }
    if (wave == 0) o.e0 = f4ld((i < FH_DEPTH ? a.b0 + (long)i * a.blk : a.fin_b) + ocol);
  };
  auto load_mlp2_ops = [&](FhOps& o, const float* mods, int i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w[j] = wfrag(2 * i + 1, j);
    if (wave == 0) {
      o.e0 = f4ld(mods + (long)crow * a.ldm + (long)i * 3 * FH_D + 2 * FH_D + ocol);  // gate
      o.e1 = f4ld(a.b2 + (long)i * a.blk + ocol);
    }
  };
  FhOps p0, p2;  // operands of the next LayerNorm phase and the next mlp2 phase

  for (int st = 0; st < a.lsd; ++st) {
    const float* mods = a.mods + (long)st * a.B * a.ldm;
    // ---- input projection x = cur W_in^T + b_in (K = 32), one wave. At st = 0 it comes first:
    // its hand-off starts the chain, so its loads are not queued behind the prologue's
    // At st = 0 with x0_ready the launch ahead (the adaLN reduce) has stored x0 already: wave 0
    // only reads its residual tile back (the chain's prologue was 3.5-3.9 us of cold loads).
    if (st > 0) fh_wait(cc, 2 * st, a.err, dead);
    if (wave == 0 && st == 0 && a.x0_ready) {
      xo = fh_ld(hr, ooff);
    } else if (wave == 0) {
      float4 cv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) cv[j] = fh_ld(cr, (crow * FH_L + 4 * j) * 4);
      xo = fh_inproj4(cv, a.in_w, a.in_b, ocol);
      if (ostore) fh_put(hr, q * rstride + ooff, xo);
    }
    ++q;
    FH_STAMP();
    if (st == 0) {
      // the first phases' operands, then the ResBlock LayerNorm affines into LDS (first read
      // after the first LayerNorm's barrier)
      load_ln_ops(p0, mods, 0, st);
      load_mlp2_ops(p2, mods, 0);
#pragma unroll
      for (int i = 0; i < FH_DEPTH; ++i)
        if (tid < FH_D / 2) {  // threads 0..255: float4 (tid & 127) of lnw (tid < 128) or lnb
          const float* src = (tid < FH_D / 4 ? a.lnw : a.lnb) + (long)i * a.blk;
          reinterpret_cast<float4*>(&s_ln[i][tid < FH_D / 4 ? 0 : 1][0])[tid & (FH_D / 4 - 1)] =
              f4ld(src + 4 * (tid & (FH_D / 4 - 1)));
        }
    }
#pragma unroll 1
    for (int i = 0; i < FH_DEPTH; ++i) {
      // ---- h = modulate(LN(x)), u = silu(h W0^T + b0)
      float4 v[4];
      FH_STAMP();
      fh_sweep(hr, (q - 1) * rstride + aoff, v, a.err, dead);
      FH_STAMP();
      fh_ln(v, s_st, wave, c, G, &s_ln[i][0][k0], &s_ln[i][1][k0], p0.sc, p0.sf);
      FH_STAMP();
      float4 r = fh_gemm(v, p0.w, s_red2[gi++ & 1], wave, c, G, lane);
      FH_STAMP();
      if (wave != 0) load_ln_ops(p0, mods, i + 1, st);
      if (wave == 0) {
        const float4 bb = p0.e0;
        const float4 u = make_float4(silu(r.x + bb.x), silu(r.y + bb.y), silu(r.z + bb.z), silu(r.w + bb.w));
        if (ostore) fh_put(hr, q * rstride + ooff, u);
        load_ln_ops(p0, mods, i + 1, st);
      }
      FH_STAMP();
      ++q;
      // ---- x += gate * (u W2^T + b2)
      fh_sweep(hr, (q - 1) * rstride + aoff, v, a.err, dead);
      FH_STAMP();
      r = fh_gemm(v, p2.w, s_red2[gi++ & 1], wave, c, G, lane);
      FH_STAMP();
      if (wave != 0 && i + 1 < FH_DEPTH) load_mlp2_ops(p2, mods, i + 1);
      if (wave == 0) {
        xo = f4add(xo, f4mul(p2.e0, f4add(r, p2.e1)));
        if (ostore) fh_put(hr, q * rstride + ooff, xo);
        if (i + 1 < FH_DEPTH) load_mlp2_ops(p2, mods, i + 1);
      }
      FH_STAMP();
      ++q;
    }
    // ---- FinalLayer (mlp.rs:182-213): modulate(LN_noaffine(x)) W_f^T + b_f, Euler x += v / N
    const float* nmods = mods + (long)a.B * a.ldm;  // next Euler step's modulations
    const bool more = st + 1 < a.lsd;
    if (fin) {
      const int off = (crow * FH_L + ocol) * 4;
      float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (wave == 0) cv = fh_ld(cr, off);  // latent before this Euler step (read ahead of the sweep)
      float4 v[4];
      fh_sweep(hr, (q - 1) * rstride + aoff, v, a.err, dead);
      FH_STAMP();
      if (wave != 0 && more) load_mlp2_ops(p2, nmods, 0);
      fh_ln(v, s_st, wave, c, G, nullptr, nullptr, p0.sc, p0.sf);
      const float4 r = fh_gemm(v, p0.w, s_red2[gi++ & 1], wave, c, G, lane);
      if (wave != 0 && more) load_ln_ops(p0, nmods, 0, st + 1);
      if (wave == 0) {
        const float e = e_row;
        const float4 o = f4add(r, p0.e0);
        const float4 nx = make_float4(cv.x + o.x * e, cv.y + o.y * e, cv.z + o.z * e, cv.w + o.w * e);
        // a row past its own count keeps its latent (a select: the discarded update may be non-finite)
        if (ostore) fh_st(cr, off, st < n_row ? nx : cv);
        if (more) fh_publish(cc);
        FH_STAMP();
        if (more) {
          load_ln_ops(p0, nmods, 0, st + 1);
          load_mlp2_ops(p2, nmods, 0);
        }
      }
    } else if (more) {
      load_ln_ops(p0, nmods, 0, st + 1);
      load_mlp2_ops(p2, nmods, 0);
    }
  }
  // re-arm: the last workgroup to finish zeroes every counter (all waits are behind it); with one
  // Euler step no counter is used
  if (a.lsd > 1 && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int* done = a.ctr + 4 * RG;
    if (__hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
      for (int g = 0; g < 4 * RG; ++g) __hip_atomic_store(a.ctr + g, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// FlowLM input projection + the first layer's norm1 in one launch (flow_lm.rs:117 input_linear,
// transformer.rs:66-90 norm1): x[m] = lat[m] W^T (K = 32, no bias), h[m] = LN(x[m]) (eps 1e-5).
// One workgroup per row (input_ln_row). The step graphs fold this into k_front_commit of the step
// before; this launch refreshes every row after anything else wrote x / h or lat_in.
__global__ __launch_bounds__(256) void k_input_ln(const float* __restrict__ lat, const float* __restrict__ Wt,
                                                  const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                  float* __restrict__ x, float* __restrict__ h) {
  front_prio();
  __shared__ float sh[4];
  const int m = blockIdx.x;
  InputLnOps ops;
  input_ln_request(Wt, lnw, lnb, Wt, ops);
  __builtin_amdgcn_sched_barrier(0);  // all 34 in flight before the first product
  input_ln_row(lat + (long)m * 32, ops, x + (long)m * 1024, h + (long)m * 1024, sh);
}

void input_ln(const float* lat, const float* Wt, const float* lnw, const float* lnb, float* x, float* h, int M,
              hipStream_t s) {
  hipLaunchKernelGGL(k_input_ln, dim3(M), dim3(256), 0, s, lat, Wt, lnw, lnb, x, h);
}

__global__ void k_transpose(const float* src, int rows, int cols, float* dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  dst[(long)c * rows + r] = src[i];
}

void transpose(const float* src, int rows, int cols, float* dst, hipStream_t s) {
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(k_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, rows, cols, dst);
}


bool flow_head_fits(int B) { return B >= 1 && B <= 128; }

size_t flow_head_packed_floats() { return (size_t)2 * FH_DEPTH * FH_D * FH_D + (size_t)FH_L * FH_D; }

// dst float4 (((m * 32 + cg) * 8 + w) * 4 + j) * 64 + l = W_m[16 cg + (l & 15)][64 w + FH_KJ j +
// 4 (l >> 4) ..+3], W_m = w0 / w2 of ResBlock m / 2, or fin_w (m = 12, column groups 0-1)
__global__ void k_pack_flow_head(const float* w0, const float* w2, long blk, const float* fin_w, float4* dst,
                                 long n4) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const int l = (int)(e & 63), j = (int)((e >> 6) & 3), w = (int)((e >> 8) & 7), cg = (int)((e >> 11) & 31);
  const int m = (int)(e >> 16);
  const float* W = m == 2 * FH_DEPTH ? fin_w : (m & 1 ? w2 : w0) + (long)(m >> 1) * blk;
  dst[e] = *reinterpret_cast<const float4*>(W + (long)(16 * cg + (l & 15)) * FH_D + 64 * w + FH_KJ * j + 4 * (l >> 4));
}

void pack_flow_head(const float* w0, const float* w2, long blk, const float* fin_w, float* dst, hipStream_t s) {
  const long n4 = (long)flow_head_packed_floats() / 4;
  hipLaunchKernelGGL(k_pack_flow_head, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, w0, w2, blk, fin_w,
                     reinterpret_cast<float4*>(dst), n4);
}

int flow_head_grid(int B) { return (B + 15) / 16 * (FH_D / 16); }

int flow_head_max_resident(int dev) {
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_flow_head, 64 * FH_WAVES, 0) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return per_cu * cus;
}

void flow_head(const FlowHeadArgs& a, hipStream_t s) {
  if (!flow_head_fits(a.B)) throw std::runtime_error("flow_head: B out of range");
  hipLaunchKernelGGL(k_flow_head, dim3(flow_head_grid(a.B)), dim3(64 * FH_WAVES), 0, s, a);
}

#ifdef PTTS_PROBES
__global__ void k_stamp(unsigned long long* ring, unsigned* ctr, unsigned tag) {
  const unsigned i = atomicAdd(ctr, 1u);
  if (i < STAMP_CAP) {
    ring[2 * i] = tag;
    ring[2 * i + 1] = wall_clock64();
  }
}

void stamp(unsigned long long* ring, unsigned* ctr, unsigned tag, hipStream_t s) {
  hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, s, ring, ctr, tag);
}
#endif

}  // namespace ptts
