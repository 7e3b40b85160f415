// Device kernels of the Pocket TTS hot path (gfx950 / CDNA4), launch-side declarations.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace ptts {

// ---------------------------------------------------------------------------------------------
// GEMM: Y[M][N] = epilogue(A[M][K] . W[N][K]^T), fp32 in / fp32 accumulate on
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain). A is either a dense row-major matrix
// (mode 0) or the implicit im2col of a streaming conv1d over channels-last activations
// (mode 1): row m = (b, q), k = (tap j, ci) reads X[b][q*stride + j - P][ci], or the
// per-slot history H[b][P + t][ci] when that time index is negative (t < 0).
// W rows are padded to a multiple of 32; K must be a multiple of 32 (and cin % 32 == 0).
// grid = (ceil(N/32), ceil(M/32), S) ; S > 1 = split-K partial slabs (mode 0 only),
// or the transposed-conv phase index (mode 1).
enum Act : int { ACT_NONE = 0, ACT_GELU = 1, ACT_SILU = 2, ACT_ELU = 3 };

// ---------------------------------------------------------------------------------------------
// Row reduce / epilogue of a split-K GEMM, fused with residual, gate, LayerNorm and modulate:
//   v = sum_z P[z][m][n] (+bias[n]) ; v = act(v) ; v *= gate[m][n] ; v += R[m][n] ;
//   Y[m][n] = v ; (euler) cur[m][n] += v / n_m while euler_step < n_m (n_m: row m's lsd count)
//   if ln: h = LN(v)*w+b (or non-affine) ; h = h*(1+mscale[m][n]) + mshift[m][n] ; H[m][n] = h
struct SlotState;
struct RowReduceArgs {
  const float* P;
  int S, M, N;
  const float* bias;
  int act;
  const float* gate;  // [M][ldg] or nullptr
  long ldg;
  const float* R;  // residual [M][ldr] or nullptr (may alias Y)
  long ldr;
  float* Y;  // [M][ldy] or nullptr
  long ldy;
  float* Y2;  // also store elu(v) here ([M][ldy]), or nullptr (SEANet dual raw / ELU'd output)
  // cur [M][32] (N must be 32): Euler step euler_step of the flow head. Row m takes euler_st[m].lsd
  // steps of size 1 / lsd: cur += v / lsd while euler_step < lsd, cur kept (a select) from then on
  float* euler;
  const SlotState* euler_st;
  int euler_step;
  // LayerNorm of the final row (N <= 1024)
  int ln;
  const float* ln_w;
  const float* ln_b;
  float eps;
  const float* mshift;  // modulate (mlp.rs:135): [M][ldm] or nullptr
  const float* mscale;
  long ldm;
  float* Hout;
  long ldh;
  // side job: fill[0 .. 4 * fill_n4) = 0xFFFFFFFF (re-arms the flow-head hand-off regions in the
  // launch just ahead of k_flow_head), or nullptr
  float* fill;
  long fill_n4;
  // the adaLN reduce's second copy of the ResBlock / final shift and scale columns in k_flow_head's
  // fragment order (FlowHeadArgs::fhm) for a batch of fhm_B rows, or nullptr
  float* fhm;
  int fhm_B;
  // side job for k_flow_head's first hand-off: x0 = cur W_in^T + b_in (flow-head input projection,
  // mlp.rs:375) for x0_B rows, stored into hand-off region 0 in its tile layout, or nullptr;
  // x0_w is W_in transposed, [32][512]
  const float *x0_cur, *x0_w, *x0_b;
  float* x0_hx;
  int x0_B;
  int front;  // 1: a launch of the front part (issue priority, set_front_prio)
  // (ln, N == FK_K, M <= 32) also store the LayerNorm output in gemv_fk's A-fragment order, or nullptr
  float* Hfrag;
};
// ---------------------------------------------------------------------------------------------
// The GEMM tiles, one row per tile id (GemmArgs::layout). The ids are an interface and keep their
// values: PTTS_OVR, the tools' command lines and the records under profiles/ speak them. The
// bf16-operand twin of an f32 tile has its id + 100, the bf16x6 twin + 200.
//   family  the kernel: TILE_GEMM k_gemm (register operands), TILE_RB k_gemm_rb (register-blocked,
//           the 4 waves split K), TILE_GLDS k_gemm_glds (LDS-DMA)
//   WM WN   waves of the workgroup tile in M and N; TMW TNW 32x32 accumulators per wave; the tile
//           is 32 WM TMW x 32 WN TNW. A k_gemm tile with more waves than WM WN deals its K chunks
//           to them (ksplit)
//   BK      K chunk width: K (and a conv's cin) must be a multiple of it
//   NBUF    k_gemm_glds: LDS buffers; k_gemm: chunks in flight per wave
//   MINB    workgroups per CU the register allocation allows; ILV: DMA issue between the MFMAs
//   ops     operand kind (k_gemm_glds PREC); thr: threads per workgroup
//   probe   1: compiled only into -DPTTS_PROBES builds (tools/, PTTS_OVR sweeps)
// ---------------------------------------------------------------------------------------------
enum TileFamily : int { TILE_GEMM, TILE_RB, TILE_GLDS };
enum TileOps : int { OPS_F32 = 0, OPS_BF16 = 1, OPS_BF16X6 = 2 };
//  id   family     WM WN BK NBUF TMW TNW MINB ILV ops        thr probe
#define PTTS_TILES(X)                                                                                          \
  X(0,   TILE_GEMM, 1, 1, 32, 1, 1, 1, 1, 0, OPS_F32,    256, 0) /*  32 x  32 ksplit, 4 waves */              \
  X(3,   TILE_GEMM, 4, 1, 32, 1, 1, 1, 1, 0, OPS_F32,    256, 1) /* 128 x  32 */                              \
  X(9,   TILE_GEMM, 1, 1, 32, 1, 1, 1, 1, 0, OPS_F32,    512, 0) /*  32 x  32 ksplit, 8 waves */              \
  X(10,  TILE_GEMM, 1, 1, 32, 2, 1, 1, 1, 0, OPS_F32,    256, 1) /*  ... 4 waves, 2 chunks in flight */       \
  X(17,  TILE_GEMM, 1, 1, 32, 2, 1, 1, 1, 0, OPS_F32,    512, 1) /*  ... 8 waves, 2 chunks in flight */       \
  X(18,  TILE_RB,   1, 1, 32, 1, 1, 2, 1, 0, OPS_F32,    256, 0) /*  32 x  64 */                              \
  X(19,  TILE_RB,   1, 1, 32, 1, 2, 1, 1, 0, OPS_F32,    256, 1) /*  64 x  32 */                              \
  X(20,  TILE_RB,   1, 1, 32, 1, 2, 2, 1, 0, OPS_F32,    256, 0) /*  64 x  64 */                              \
  X(6,   TILE_GLDS, 2, 2, 32, 2, 1, 1, 1, 0, OPS_F32,    256, 0) /*  64 x  64 */                              \
  X(7,   TILE_GLDS, 1, 4, 32, 2, 1, 1, 1, 0, OPS_F32,    256, 0) /*  32 x 128 */                              \
  X(8,   TILE_GLDS, 2, 2, 64, 2, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  X(11,  TILE_GLDS, 2, 2, 32, 3, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  X(12,  TILE_GLDS, 2, 2, 32, 4, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  X(13,  TILE_GLDS, 1, 4, 32, 4, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  X(14,  TILE_GLDS, 4, 1, 32, 4, 1, 1, 1, 0, OPS_F32,    256, 0) /* 128 x  32 */                              \
  X(15,  TILE_GLDS, 2, 2, 64, 3, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  X(16,  TILE_GLDS, 1, 4, 64, 3, 1, 1, 1, 0, OPS_F32,    256, 1)                                              \
  /* register-blocked LDS-DMA tiles (per-wave TMW x TNW accumulators) */                                      \
  X(21,  TILE_GLDS, 2, 2, 32, 3, 2, 2, 1, 0, OPS_F32,    256, 1) /* 128 x 128 */                              \
  X(22,  TILE_GLDS, 2, 2, 32, 3, 1, 2, 1, 0, OPS_F32,    256, 1) /*  64 x 128 */                              \
  X(23,  TILE_GLDS, 2, 2, 32, 3, 2, 1, 1, 0, OPS_F32,    256, 0) /* 128 x  64 */                              \
  X(24,  TILE_GLDS, 4, 1, 32, 3, 2, 1, 1, 0, OPS_F32,    256, 1) /* 256 x  32 */                              \
  X(25,  TILE_GLDS, 4, 1, 32, 3, 1, 2, 1, 0, OPS_F32,    256, 1) /* 128 x  64 (waves stacked in M) */         \
  X(26,  TILE_GLDS, 2, 2, 32, 4, 2, 2, 1, 0, OPS_F32,    256, 1) /* 128 x 128, 4 buffers */                   \
  X(27,  TILE_GLDS, 1, 4, 32, 3, 2, 1, 1, 0, OPS_F32,    256, 1) /*  64 x 128 (waves side by side in N) */    \
  /* interleaved DMA issue (ILV) */                                                                           \
  X(30,  TILE_GLDS, 2, 2, 32, 3, 2, 2, 1, 1, OPS_F32,    256, 1) /* 128 x 128 */                              \
  X(31,  TILE_GLDS, 2, 2, 32, 2, 2, 2, 2, 1, OPS_F32,    256, 1) /* 128 x 128, 2 per CU */                    \
  X(32,  TILE_GLDS, 2, 2, 32, 3, 1, 1, 2, 1, OPS_F32,    256, 0) /*  64 x  64, 2 per CU (back part) */        \
  X(33,  TILE_GLDS, 2, 2, 32, 2, 1, 1, 2, 1, OPS_F32,    256, 1) /*  64 x  64, 2 buffers, 2 per CU */         \
  X(34,  TILE_GLDS, 2, 2, 32, 3, 2, 1, 1, 1, OPS_F32,    256, 0) /* 128 x  64 (prefill linear1) */            \
  X(35,  TILE_GLDS, 2, 2, 32, 2, 2, 1, 2, 1, OPS_F32,    256, 0) /* 128 x  64, 2 per CU (prefill) */          \
  X(36,  TILE_GLDS, 2, 2, 32, 3, 1, 2, 1, 1, OPS_F32,    256, 1) /*  64 x 128 */                              \
  X(37,  TILE_GLDS, 2, 2, 32, 4, 1, 1, 1, 1, OPS_F32,    256, 1) /*  64 x  64, 4 buffers */                   \
  X(38,  TILE_GLDS, 2, 2, 32, 4, 2, 2, 1, 1, OPS_F32,    256, 1) /* 128 x 128, 4 buffers */                   \
  X(39,  TILE_GLDS, 2, 2, 32, 3, 1, 2, 2, 1, OPS_F32,    256, 1) /*  64 x 128, 2 per CU */                    \
  /* bf16 operands (engine back_mfma = PTTS_BACK_BF16) */                                                     \
  X(130, TILE_GLDS, 2, 2, 32, 3, 2, 2, 1, 1, OPS_BF16,   256, 1)                                              \
  X(131, TILE_GLDS, 2, 2, 32, 2, 2, 2, 2, 1, OPS_BF16,   256, 0)                                              \
  X(132, TILE_GLDS, 2, 2, 32, 3, 1, 1, 2, 1, OPS_BF16,   256, 0)                                              \
  X(135, TILE_GLDS, 2, 2, 32, 2, 2, 1, 2, 1, OPS_BF16,   256, 0)                                              \
  X(136, TILE_GLDS, 2, 2, 32, 3, 1, 2, 1, 1, OPS_BF16,   256, 1)                                              \
  X(139, TILE_GLDS, 2, 2, 32, 3, 1, 2, 2, 1, OPS_BF16,   256, 1)                                              \
  /* bf16x6 f32 (engine back_mfma = PTTS_BACK_F32X6): W pre-split (GemmArgs::Whm, Wlo) */                      \
  X(230, TILE_GLDS, 2, 2, 32, 3, 2, 2, 1, 1, OPS_BF16X6, 256, 1)                                              \
  X(231, TILE_GLDS, 2, 2, 32, 2, 2, 2, 2, 1, OPS_BF16X6, 256, 1)                                              \
  X(232, TILE_GLDS, 2, 2, 32, 3, 1, 1, 2, 1, OPS_BF16X6, 256, 0)                                              \
  X(235, TILE_GLDS, 2, 2, 32, 2, 2, 1, 2, 1, OPS_BF16X6, 256, 0)                                              \
  X(236, TILE_GLDS, 2, 2, 32, 3, 1, 2, 1, 1, OPS_BF16X6, 256, 0)                                              \
  X(239, TILE_GLDS, 2, 2, 32, 3, 1, 2, 2, 1, OPS_BF16X6, 256, 0)

struct TileInfo {
  int id;
  TileFamily family;
  int wm, wn, bk, nbuf, tmw, tnw, minb;
  bool ilv;
  TileOps ops;
  int threads;
  bool probe;
  constexpr int tm() const { return 32 * wm * tmw; }
  constexpr int tn() const { return 32 * wn * tnw; }
  constexpr bool ksplit() const { return family == TILE_GEMM && threads / 64 > wm * wn; }
  constexpr bool lds_dma() const { return family == TILE_GLDS; }  // the tiles that may split a conv's K
  constexpr bool split_tail() const { return ilv && ops == OPS_F32; }  // GemmArgs::tail_S (dense)
  constexpr bool split_weights() const { return ops == OPS_BF16X6; }   // reads GemmArgs::Whm / Wlo
};
#define PTTS_TILE_ROW(ID, FAM, WM, WN, BK, NBUF, TMW, TNW, MINB, ILV, OPS, THR, PROBE) \
  {ID, FAM, WM, WN, BK, NBUF, TMW, TNW, MINB, ILV != 0, OPS, THR, PROBE != 0},
inline constexpr TileInfo TILES[] = {PTTS_TILES(PTTS_TILE_ROW)};
#undef PTTS_TILE_ROW
constexpr int TILE_TWIN_BF16 = 100, TILE_TWIN_BF16X6 = 200;  // id offsets of the operand twins
// the row of a tile id in the table (any build), or nullptr
constexpr const TileInfo* tile_row(int id) {
  for (const TileInfo& t : TILES)
    if (t.id == id) return &t;
  return nullptr;
}
// a twin differs from its f32 tile in the operand kind alone
constexpr bool tile_twins_match() {
  for (const TileInfo& t : TILES) {
    if (t.id < TILE_TWIN_BF16) continue;
    const TileInfo* f = tile_row(t.id % 100);
    if (!f || t.ops != (t.id >= TILE_TWIN_BF16X6 ? OPS_BF16X6 : OPS_BF16) || f->ops != OPS_F32 || f->family != t.family ||
        f->wm != t.wm || f->wn != t.wn || f->bk != t.bk || f->nbuf != t.nbuf || f->tmw != t.tmw || f->tnw != t.tnw ||
        f->minb != t.minb || f->ilv != t.ilv || f->threads != t.threads)
      return false;
  }
  return true;
}
static_assert(tile_twins_match(), "PTTS_TILES: a + 100 / + 200 row must repeat its f32 tile");
// ... in this build: nullptr for an unknown id, and for a probe-only tile in a product build
inline const TileInfo* tile_info(int id) {
  const TileInfo* t = tile_row(id);
#ifndef PTTS_PROBES
  if (t && t->probe) return nullptr;
#endif
  return t;
}
// The tiles the product selects (engine.cpp linear_split, back_tile)
constexpr int TILE_KSPLIT_4W = 0;      // 32 x 32, K dealt to 4 waves: the skinny default, B < 16 back part
constexpr int TILE_KSPLIT_8W = 9;      // ... to 8 waves (flow-head MLPs)
constexpr int TILE_RB_32x64 = 18;      // register-blocked K-split (SEANet residual convs)
constexpr int TILE_RB_64x64 = 20;
constexpr int TILE_GLDS_64x64 = 6;     // LDS-DMA, 2 buffers
constexpr int TILE_GLDS_32x128 = 7;    // FlowLM qkv / ff1, flow-head adaLN
constexpr int TILE_GLDS_128x32 = 14;
constexpr int TILE_GLDS_RB_128x64 = 23;
constexpr int TILE_ILV_64x64_2CU = 32;  // the back part's MFMA-bound GEMMs and convs
constexpr int TILE_ILV_128x64 = 34;     // prefill linear1
constexpr int TILE_ILV_128x64_2CU = 35;  // prefill
constexpr int TILE_ILV_128x128_2CU = 31;  // probe-only as f32; its bf16 twin ships

struct GemmArgs {
  int mode;    // 0 dense, 1 conv
  int layout;  // tile id: a row of PTTS_TILES above
  int M, N, K;
  int Nw;  // rows present in W (N rounded up to 32)
  // A operand
  const float* X;
  long ldx;
  const float* H;  // conv history [B][P][cin]
  int P, T_in, Tq, stride_in, cin, elu_in;
  // B operand
  const float* W;
  long w_phase_stride;  // floats between polyphase weight blocks (mode 1)
  // bf16x6 tiles (TileInfo::split_weights, ptts_engine_config.back_mfma = PTTS_BACK_F32X6): W split exactly
  // into three bf16 pieces, W = hi + mid + lo (split3): Whm[n][k] = hi << 16 | mid (the f32 layout
  // of W, 4 B per element), Wlo[n][k] = lo (2 B per element); same indexing as W
  const unsigned* Whm;
  const unsigned short* Wlo;
  // int8 B operand (weight_quant; mode 0, split-K slabs only): W[n][k] = float(Wq[n][k]) *
  // wscale[n], formed per element before the MFMA. Replaces W when non-null.
  const int8_t* Wq;
  const float* wscale;
  // fp8 W8A8 (ptts_engine_config.fp8_gemm; mode 0, split-K slabs only): W[n][k] ~= e4m3(Wf8[n][k])
  // * wscale[n]; the A rows are quantized to e4m3 in-kernel with one scale per (row, K slice)
  // and the tile runs on v_mfma_f32_32x32x16_fp8_fp8. Replaces W when non-null.
  const uint8_t* Wf8;
  // XCD placement of the tile grid (set by gemm(); speed only): the 8 XCDs split the N tiles
  // into xcd_pn parts and the M tiles into 8 / xcd_pn parts; 0 = contiguous runs of tiles
  int xcd_pn;
  // > 0: at most this many workgroups of the launch per CU (dynamic LDS reserved to enforce it),
  // leaving room on every CU for the concurrently running part of a pipelined step
  int max_wg_per_cu;
  // 1: the weight stream is read with non-temporal loads (once-read FlowLM step weights)
  int w_nt;
  // 1: a launch of the front part (FlowLM / flow head): its waves take the front issue priority
  int front;
  // 1: a back-part launch whose waves issue at priority 3 (set by the launcher from set_back_hi)
  int back_hi;
  // measurement probe, -DPTTS_PROBES builds only (tools/; PTTS_BACK_PROBE: back-part launches of a
  // pipelined step, PTTS_FRONT_PROBE: all other tiled launches; results are wrong): bit 0 skips
  // the MFMAs, bit 1 the operand loads of the K loop. Ignored by product builds.
  int probe;
  // split-K
  int S;
  float* partial;  // [S][M][N] when S > 1
  // split tail (dense, LDS-DMA ILV tiles, S == 1): the tiles that fill whole rounds of the CUs'
  // workgroup slots run over all of K; the remainder (fewer tiles than slots) is cut into tail_S
  // K slices, one workgroup each, whose partial tiles go to tail_slab [rem][tail_S][TM*TN]; the
  // last slice to finish (tickets[rem], zero between launches) sums them in slice order and
  // applies the epilogue. gemm() derives the split of the grid; capacities are checked.
  int tail_S;
  float* tail_slab;
  long tail_cap;  // floats in tail_slab
  int* tickets;
  int tickets_cap;
  int tail_full, tiles_n;  // set by gemm()
  // epilogue (S == 1)
  const float* bias;
  int act;
  const float* R;  // residual (same row mapping as Y), may alias Y
  long ldr;
  const float* rscale;  // per-column scale of the update (LayerScale) or nullptr
  float* Y;
  long ldy;
  int T_out, out_tstride;  // mode 1 output row = b*T_out + q*out_tstride + phase
  // ELU on the way out (SEANet: the consumer's ELU applied once by the producer, seanet.rs:298-305):
  // elu_out: Y = elu(v) (after the residual); Y2 != null: Y = v and Y2 = elu(v) (same indexing)
  int elu_out;
  float* Y2;
};
// A dense GEMM (mode 0) X [M][ldx] . W [N][K]^T on tile `layout`; split-K, the split tail and the
// epilogue are the caller's to add
inline GemmArgs dense_gemm(int layout, int M, int N, int K, const float* X, long ldx, const float* W) {
  GemmArgs a{};
  a.mode = 0;
  a.layout = layout;
  a.M = M;
  a.N = N;
  a.K = K;
  a.Nw = (N + 31) / 32 * 32;
  a.X = X;
  a.ldx = ldx;
  a.W = W;
  return a;
}
void gemm(const GemmArgs& a, int grid_z, hipStream_t s);
// Exact three-piece bf16 split of n f32 values (the B operand of the bf16x6 tiles): x = hi + mid
// + lo with every piece a bf16 (round to nearest even at each step; the remainders are exact in
// f32 and the last one is exact in bf16), stored as hm = bits(hi) << 16 | bits(mid) and lo.
void split3(const float* W, long n, unsigned* hm, unsigned short* lo, hipStream_t s);

// Skinny split-K GEMM (M <= 64 rows: the FlowLM step, small prefills; one 32-row block per
// grid z) with register-resident weights: the
// workgroup tile is 32 rows x 32*wn columns over a K slice of ks = kw * (4 / wn); wave w takes
// 32 columns (w % wn) and kw of the slice's k ((w / wn) * kw ..). Its weight fragment (kw * 32
// floats) comes from a copy packed in fragment order (pack_gemv: every load instruction reads 1
// contiguous KB), all of it requested at the start; the slice of X is staged in LDS. Output:
// partial slab z = blockIdx.y of P [S][M][N], S = K / ks.
struct GemvShape {
  int wn, kw;
  int ks() const { return kw * (4 / wn); }
};
bool gemv_supported(GemvShape g, int N, int K);
// Whole-K skinny GEMM for K = 1024, M <= 32 (the FlowLM step's linear1): Y = act(A W^T + bias),
// one 512-thread workgroup per 16 output columns, the 8 waves splitting K in 128-k ranges, each
// wave's weight fragment (pack_gemv_fk) AND its A fragment requested at the start: A comes in
// fragment order (FK_A_FLOATS floats, written by the row reduce ahead of it: RowReduceArgs::Hfrag),
// so every load instruction reads one contiguous KB. v_mfma_f32_16x16x4f32 over two 16-row tiles;
// the waves' partial tiles are summed through LDS in wave order and the epilogue (bias, GELU)
// writes Y: no split-K slabs and no reduce launch.
constexpr int FK_K = 1024;
constexpr long FK_A_FLOATS = 32L * FK_K;
bool gemv_fk_supported(int M, int N, int K);
void pack_gemv_fk(const float* W, int N, int K, float* packed, hipStream_t s);
void gemv_fk(const float* Afrag, int M, int N, const float* packed, const float* bias, int act, float* Y, long ldy,
             hipStream_t s);
// FlowLM feed-forward of a step pass in ONE launch (M <= 32; D = 1024, FF = 4096): linear1 + GELU as
// gemv_fk, then linear2 split over `groups` K slices into the partial slabs P [groups][M][D] (the
// following row reduce sums them). The 256 workgroups form the groups, one per linear2 slice (8
// groups of 32: the product; 16 of 16: probe builds): the members of group z produce linear1's
// columns of slice z (16 each) and hand them to each other through `hand` (data-as-flag, sc1
// stores / loads, in the MFMA A-fragment order of linear2), then each computes its linear2
// columns of slice z, its linear2
// weight fragment requested at the start beside linear1's. `hand` holds two sets of
// FFN_HAND_FLOATS floats: the launch uses set `set` (emptied, 0xFFFFFFFF, by the launch before)
// and empties the other one for the launch after. A hand-off wait that times out sets *err.
constexpr long FFN_HAND_FLOATS = 16L * 32 * 256;
bool ffn_fused_supported(int M, int D, int FF);
// groups: 16 (linear2 K slices of 256, 16 slabs) or 8 (slices of 512 with 32 members, 8 slabs)
void pack_ffn2(const float* W2, int groups, float* packed, hipStream_t s);  // linear2 [1024][4096] -> fragment order
// Q1 / Q2 (optional, weight_quant engines): linear1 / linear2 as int8 codes in pack_q8 order with
// their row scales s1 / s2 (float(q) * s == the quantized f32 weight, bit for bit, derive_int8):
// the codes are widened to f32 in registers, so the MFMA chain and the result are those of the f32
// fragments (P1 / P2 unused when the codes are given)
// fp8: Q1 / Q2 are e4m3 codes (fp8_codes) and both GEMMs run W8A8 on the fp8 MFMA (8 groups)
void ffn_fused(const float* Afrag, int M, const float* P1, const float* P2, int groups, float* hand, int set, float* P,
               int* err, hipStream_t s, const uint32_t* Q1 = nullptr, const float* s1 = nullptr,
               const uint32_t* Q2 = nullptr, const float* s2 = nullptr, bool fp8 = false);
void pack_gemv(const float* W, int N, int K, GemvShape g, float* packed, hipStream_t s);
// q8 / scale (optional): the weight as int8 codes in pack_q8 order + row scales, as for ffn_fused;
// fp8: the codes are e4m3 (fp8_codes) and the tile runs W8A8 on the fp8 MFMA ({4, 128} tiles)
void gemv_splitk(const float* X, long ldx, int M, int N, int K, const float* packed, GemvShape g, float* partial,
                 hipStream_t s, const uint32_t* q8 = nullptr, const float* scale = nullptr, bool fp8 = false);
// int8 codes of the register-resident GEMMs: a fragment-packed copy (pack_gemv / pack_gemv_fk /
// pack_ffn2 applied to the codes widened to f32, codes_to_f32) re-packed to one byte per element
// with a lane's four consecutive fragment groups in one 16-B load: u32x4 (P * NJ / 4 + J) * 64 + l
// holds the groups 4 J .. 4 J + 3 of f32 float4 index (P * NJ + j) * 64 + l (NJ: groups per lane
// and wave, a multiple of 4; n4 float4 in the f32 copy)
void codes_to_f32(const int8_t* q, long n, float* out, hipStream_t s);
void codes_u8_to_f32(const uint8_t* q, long n, float* out, hipStream_t s);  // fp8 codes as their byte values
void pack_q8(const float* packed_codes, long n4, int nj, uint32_t* q8, hipStream_t s);

// int8 codes of a quantized weight matrix: q[n][k] = W[n][k] / s[n] (exact integers in
// [-127, 127] for a blob packed by the quantizer); rows with s[n] == 0 get code 0. Any element
// with float(q) * s[n] != W[n][k] (bitwise) increments *bad.
void quant_codes(const float* W, const float* s, int N, int K, int8_t* q, int* bad, hipStream_t st);
// fp8 (OCP e4m3) codes of W [N][K] with one scale per row: s[n] = max|W[n][:]| / 448
void fp8_codes(const float* W, int N, int K, uint8_t* q, float* s, hipStream_t st);
constexpr int FP8_KSLICE_MAX = 512;  // K elements per split-K slice the fp8 GEMM stages in LDS

void row_reduce(const RowReduceArgs& a, hipStream_t s);

// LayerNorm over rows of width N (<= 1024), biased variance (candle_nn::LayerNorm).
void layernorm(const float* x, long ldx, float* y, long ldy, int M, int N, const float* w, const float* b,
               float eps, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Packed QKV (sum of S partials, or dense) -> RoPE(q,k) -> q to Q[M][d], k/v into the KV store.
// Row r belongs to slot = slot0 + r / rps at position pos = (pos_arr ? pos_arr[slot] : p0) + r % rps.
// KV layout per slot: base + slot*slot_stride + (kv*nh + h)*cap*64 + (pos % cap)*64.
// Row -> (slot, position). Uniform form: slot = slot0 + row / rps, position = (pos_arr ?
// pos_arr[slot] : p0) + row % rps. Table form (tab != nullptr, batched admission): tab[row] =
// slot << 16 | position, or -1 for a padding row (no KV write, output unused).
struct RowMap {
  int slot0, rps, p0;
  const int* pos_arr;
  const int* tab;
  // compact batched admission (slots_open): the GEMM / reduce rows are the tokens only (tab), while
  // the 16-query attention runs on slot-aligned 16-row groups with padding (ptab, mpad rows): qkv
  // rope writes query row r at padded row qrow[r], the attention writes padded row p's output at
  // row orow[p] (-1: padding, not written)
  const int* ptab = nullptr;
  int mpad = 0;
  const int* qrow = nullptr;
  const int* orow = nullptr;
};
// Shared voice prefixes (FlowLM cache): when `pre` is set, positions < pre_len[slot] of slot
// `slot` live in the voice's own cache pre[slot] ([NL][2][nh][F][64], F = pre_len[slot]; layer
// `layer` of it) instead of the slot's rows, so every utterance of one voice reads one copy.
struct KvStore {
  float* base;
  long slot_stride;
  int cap;
  const float* const* pre = nullptr;
  const int* pre_len = nullptr;
  int layer = 0;
};
void qkv_rope_append(const float* P, int S, const float* dense, int M, int nh, RowMap map, KvStore kv,
                     float* Q, hipStream_t s);

// Causal (optionally windowed) softmax attention for rows mapped as above; rows are processed
// in groups of 16 consecutive rows of one slot. O[M][nh*64].
// Mimi decoder step: RoPE + ring append of the dense QKV rows fused into the 16-row attention
void attention16_qkv(const float* qkv, int M, int nh, RowMap map, KvStore kv, int window, float* O, hipStream_t s);
void attention(const float* Q, int M, int nh, RowMap map, KvStore kv, int window, float* O, hipStream_t s);
// One-query-per-row step attention fused with the QKV slab sum, RoPE and KV append (positions
// must not wrap: FlowLM cache).
void attention_step_qkv(const float* P, int S, int M, int nh, RowMap map, KvStore kv, const float* rope, float* O,
                        hipStream_t s);
// RoPE table (rope.rs:9-60): tab[pos][2i] = cos(pos * f_i), tab[pos][2i+1] = sin(pos * f_i),
// f_i = exp(-ln(1e4) * 2i / 64), i < 32, pos < npos - the values the step kernels would compute.
void rope_table(float* tab, int npos, hipStream_t s);

// Word alignment: one layer's text-attention row per step row, from the
// operands the step attention of that layer has just read. Row r is slot r at position pos[r]. A
// slot with tab[r] = {t0, n}, n >= 1, gets, per head of head_mask, the softmax over j < n of
// (q_h . K_h[t0 + j]) / 8 with q_h the slab sum of its q column rotated at min(pos, cap - 1) (the
// attention kernel's q, bit for bit) and K_h the slot's own store (never KvStore::pre: text keys
// lie at positions >= F), and the mean of those rows over the selected heads. out row r: the int
// count n, then ALIGN_TOKENS floats (a[0..n), zeros behind). n == 0 (or an entry that does not fit
// the store): count 0, the floats are left alone.
constexpr int ALIGN_TOKENS = 128;
constexpr int ALIGN_ROW = 1 + ALIGN_TOKENS;  // 4-byte words per row of the alignment block
struct AlignEntry {
  int t0, n;
};
struct AlignArgs {
  const float* P;  // [S][M][3 nh 64] QKV slabs (S == 1: dense rows)
  int S, M, nh;
  const int* pos;  // [M] the rows' positions
  KvStore kv;      // the layer's store (pre / pre_len unused)
  const float* rope;
  const AlignEntry* tab;  // [M]
  unsigned head_mask;
  float* out;  // [M][ALIGN_ROW]
};
void align_step(const AlignArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Per-slot generation bookkeeping (device resident so the step can be replayed as a graph).
// The step is split into a FRONT part (FlowLM + flow head: produces this step's latent and
// frame flags, owns SlotState / FlowLM KV / positions) and a BACK part (Mimi decode of a frame
// produced by the front, owns the Mimi ring, conv histories and Mimi positions). They exchange
// frames through per-parity buffers, so the back part of frame k can run concurrently with the
// front part of frame k+1.
struct SlotState {
  int active;  // row still generating
  int step;    // generation step index within the segment
  int eos_step;
  int frames_after_eos, max_frames;
  float temp, eos_threshold, noise_clamp;
  unsigned long long seed;
  // the row's LSD Euler step count, 1 .. the engine's cap (0: a closed row; read as 1)
  int lsd;
};
struct FrameFlags {
  int valid;  // the front produced a frame for this row at this step
  int last;   // ... and it is the row's final frame (EOS tail reached or max_frames)
};

// After the cond_embed|out_eos split-K GEMM: c = sum + b, eos logit -> eos_out,
// y_s = silu(temb_n[min(s, n - 1)] + c) for each of the launch's lsd_run Euler steps, n = the
// row's own step count (SlotState::lsd, clamped to [1, lsd_cap]); x0 noise -> cur (reads SlotState
// only). temb holds the time embeddings of every count 1 .. lsd_cap, triangular: the rows of
// count n start at row temb_row0(n).
constexpr int FLOW_COND_MAX_SLABS = 16;  // k_flow_cond's unrolled slab loads
constexpr int temb_row0(int n) { return n * (n - 1) / 2; }
void flow_cond(const float* P, int S, int B, const float* bias, const float* temb, int lsd_run, int lsd_cap,
               const SlotState* st, float* ysilu, float* cur, float* eos_out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Flow-head chain (mlp.rs:146-213,370-383; flow_lm.rs:7-22) in one persistent launch: per lsd
// step, x = cur W_in^T + b_in; 6 ResBlocks x += gate * (silu(mod(LN(x)) W0^T + b0) W2^T + b2);
// cur += (mod(LN_noaffine(x)) W_f^T + b_f) / n_row while the step index < n_row, the row's own
// count (st[row].lsd <= lsd; every row runs all lsd steps of the launch, a finished row keeps its
// cur). mods [lsd][B][ldm] holds the adaLN shift |
// scale | gate of each block and the final shift | scale (mlp.rs:322-368). xp/up: [B][512]
// hand-off buffers; ctr: 4*ceil(B/16)+1 ints, zero before the first launch (the kernel re-arms
// them); err: set to 1 if a hand-off wait timed out. Requires 1 <= B <= 128 (flow_head_fits).
constexpr int FH_D = 512, FH_L = 32, FH_DEPTH = 6;
struct FlowHeadArgs {
  int B, lsd;  // lsd: Euler steps of this launch (launch-uniform; >= every row's own count)
  const SlotState* st;  // per row: its own count (SlotState::lsd)
  float* cur;
  const float* mods;
  long ldm;
  const float *in_w, *in_b;
  // ResBlock 0's tensors; block i's are at + i * blk floats (the packed blob's uniform stride)
  const float *lnw, *lnb, *w0, *b0, *w2, *b2;
  long blk;
  const float *fin_w, *fin_b;
  // the 13 chain matrices (w0 / w2 of each ResBlock, then fin_w) in fragment order
  // (pack_flow_head): every operand load instruction reads one contiguous KB
  const float* wp;
  // adaLN shift / scale in fragment order, float4 ((((((st RG + rg) 7 + i) 2 + t) 8 + w) 4 + j) 64 +
  // lane) for Euler step st, row group rg, ResBlock i (6: final layer), t 0 shift / 1 scale
  // (written by the adaLN reduce: RowReduceArgs::fhm); mods itself is read for the gates
  const float* fhm;
  // hand-off regions: 13 per Euler step (x0, then u_i, x_{i+1} per ResBlock), each
  // [ceil(B/16)][32 column groups][16 rows][16 columns] (one producer tile = one contiguous KB),
  // all 0xFFFFFFFF (empty) at launch
  float* hx;
  int x0_ready;  // 1: hand-off region 0 already holds x0 of Euler step 0 (the adaLN reduce's side job)
  int* ctr;
  int* err;
  unsigned long long* dbg;  // probe only: s_memrealtime stamps of workgroups 0-3, or nullptr
};
// ---------------------------------------------------------------------------------------------
// Flow-head prelude in one persistent launch (B <= 32 rows, f32 weights, ahead of flow_head): what
// the cond | EOS GEMM, flow_cond, the adaLN GEMM and the adaLN reduce compute, without slabs.
// HP_PRODUCERS workgroups run cond | EOS = A Wc^T + bc over the whole K as gemv_fk does (A: the
// out_norm rows in gemv_fk's fragment order, Pc: pack_gemv_fk of the NCOND_PAD x 1024 matrix),
// write the EOS logits and hand y_s = silu(temb_n[min(s, n - 1)] + c) (flow_cond's rule) of each
// of the lsd Euler steps to the HP_CONSUMERS workgroups through `hand` (data-as-flag, lsd x
// ceil(B / 16) regions of HP_REGION_FLOATS, all 0xFFFFFFFF at launch: emptied by the launch ahead).
// Each consumer holds 64 columns of the adaLN matrix over the whole K = 512 in registers
// (Pa: pack_head_ada) and writes mods [lsd][B][HP_NADA] = y W_ada^T + b_ada and the shift / scale
// columns' copy fhm (FlowHeadArgs::fhm). While they wait the consumers draw the rows' noise into
// cur, compute x0 = cur W_in^T + b_in into the chain's hand-off region 0 (x0_w: W_in transposed)
// and empty fill[0 .. 4 * fill_n4) (the chain's other regions). A hand-off wait that times out
// sets *err.
constexpr int HP_NCOND = 544, HP_NADA = (FH_DEPTH * 3 + 2) * FH_D;
constexpr int HP_PRODUCERS = HP_NCOND / 16, HP_CONSUMERS = HP_NADA / 64;
constexpr long HP_REGION_FLOATS = 16L * FH_D;
struct HeadPreludeArgs {
  int B, lsd, lsd_cap;
  const float *A, *Pc, *cbias, *temb;
  const SlotState* st;
  float *eos_out, *cur, *hand;
  const float *Pa, *abias;
  float *mods, *fhm;
  const float *x0_w, *x0_b;
  float* x0_hx;
  float* fill;
  long fill_n4;
  int* err;
};
bool head_prelude_supported(int B, int lsd_run);
void pack_head_ada(const float* W, float* packed, hipStream_t s);  // [HP_NADA][512] -> fragment order
void head_prelude(const HeadPreludeArgs& a, hipStream_t s);
// Launches issued while a cap > 0 is set reserve dynamic LDS so that at most `cap` workgroups of
// each kernel share a CU (0 = no cap). Per host thread; the engine sets it around graph capture.
void set_wg_cap(int cap);
// Issue priority of the back part's tile waves (k_gemm_glds outside the front part, k_gemm_rb,
// k_resblock) for the launches made on this host thread from now on: 1 (default) s_setprio 3,
// 0 none. Set while a back graph is captured (engine.cpp part_graph).
void set_back_hi(int on);
#ifdef PTTS_PROBES
// one {tag, s_memrealtime} record appended to a device ring (tools/stamps.py)
constexpr unsigned STAMP_CAP = 1u << 16;
void stamp(unsigned long long* ring, unsigned* ctr, unsigned tag, hipStream_t s);
#endif
// Issue priority of the front part's waves (s_setprio 0..3) when they share a SIMD with back-part
// waves: probe builds only (PTTS_FRONT_PRIO), for A/B runs; a no-op in product builds.
void set_front_prio(int prio);
void set_back_prio(int prio);  // probe builds only
void set_front_skip(int v);    // probe builds only
bool flow_head_fits(int B);
// x0 = cur W_in^T + b_in into hand-off region 0 as its own launch (the adaLN reduce's side job,
// for replaying k_flow_head alone)
void flow_head_x0(const float* cur, const float* w_t, const float* bias, float* hx, int B, hipStream_t s);
// fragment-order copy of the chain's matrices for FlowHeadArgs::wp: 12 * 512 * 512 + 32 * 512 floats
size_t flow_head_packed_floats();
void pack_flow_head(const float* w0, const float* w2, long blk, const float* fin_w, float* dst, hipStream_t s);
int flow_head_grid(int B);             // workgroups of one k_flow_head launch
int flow_head_max_resident(int dev);   // co-resident k_flow_head workgroups (occupancy x CUs)
// FlowLM input_linear (32 -> 1024, no bias) + layer-0 norm1: x = lat W^T, h = LN(x) (eps 1e-5).
void input_ln(const float* lat, const float* Wt, const float* lnw, const float* lnb, float* x, float* h, int M,
              hipStream_t s);
// dst [cols][rows] = src [rows][cols]^T
void transpose(const float* src, int rows, int cols, float* dst, hipStream_t s);
void flow_head(const FlowHeadArgs& a, hipStream_t s);

// End of the front part: EOS state machine (tts_model.rs:1055-1063), frame flags, the frame's
// latent / eos logit into the parity buffers, next backbone input, step / FlowLM position.
struct FrontCommitArgs {
  int B;
  SlotState* st;
  const float* eos;  // [B] this step's logits
  const float* cur;  // [B][32] this step's latent
  float* lat_in;     // [B][32] backbone input of the next step
  float* lat_out;    // [B][32] frame latent (parity buffer)
  float* eos_out;    // [B] frame eos logit (parity buffer)
  FrameFlags* flags; // [B] (parity buffer)
  int* fpos;         // FlowLM positions, += 1
  // the next step's input projection + layer-0 norm1 of every row (k_input_ln's x, h), from the
  // updated lat_in (Wt = input_linear transposed [32][1024])
  const float *Wt, *lnw, *lnb;
  float *x, *h;
  // side jobs of workgroup 0 (they used to be copy / fill nodes at the end of the front graph, a
  // blit launch on the step's critical chain): the hand-off timeout word err_dev -> err_host
  // (pinned host memory, a system-scope store) and zero flags for the rows B .. B + n_zero - 1
  // (multi-frame passes: a pass covers the largest row count of its frames)
  const int* err_dev;
  int* err_host;
  int n_zero;
};
void front_commit(const FrontCommitArgs& a, hipStream_t s);

// Frames per back-part pass (ptts_engine_config.back_frames: 1, 2, 4 or 8) and the front -> back
// hand-off buffers of the largest pass (three passes' worth: the front part may run two passes ahead)
constexpr int NFR_MAX = 8;
constexpr int NHB_MAX = 3 * NFR_MAX;

// Denorm + 1x1 quantizer conv + depthwise ConvTrUpsample1d (k32 s16) + LN of Mimi layer 0, for
// nfr (1 .. NFR_MAX; a partial pass may cover 3) consecutive frames of every row: latent[f] [B][32] -> x [B][16 nfr][512] (frame
// f at rows 16 f..), h = LN(x). The overlap-add history [B][512] is read from qprev_in (frame 0;
// frame f > 0 overlaps frame f - 1); the quantized rows of the pass go to qprev_out
// [B][NFR_MAX][512], and the commit copies the last valid frame's into the history (rows without a
// frame, or outside the pass, keep theirs).
void quant_upsample(const float* const latent[NFR_MAX], const FrameFlags* const fl[NFR_MAX], int nfr, int B, const float* emb_std,
                    const float* emb_mean, const float* wq, const float* wup, const float* qprev_in, float* qprev_out,
                    float* x, float* h, const float* ln_w, const float* ln_b, hipStream_t s);

// End of the back part, for rows with a valid frame: copy the last P rows of each conv input
// into its history and the last valid frame's quantizer output into the overlap-add history,
// advance the Mimi position. A launch over nfr frames (T rows per row of a
// buffer = nfr frames of T / nfr rows) commits through the row's last valid frame: its valid
// frames are a prefix (an utterance starts at a pass boundary and ends with its last frame).
struct HistDesc {
  const float* src;  // [B][T][C]
  float* dst;        // [B][P][C]
  int T, C, P;
  int elu = 0;  // dst = elu(src): the history of an ELU'd activation kept only raw (ResBlockArgs::e_raw)
};
struct CommitArgs {
  HistDesc h[10];
  int nh;
  int B;
  const FrameFlags* flags[NFR_MAX];  // frame f of the pass (f < nfr)
  int nfr;
  int* mpos;  // Mimi decoder positions, += 16 per committed frame
  const float* qcur;  // the pass's quantizer outputs [B][NFR_MAX][512] (quant_upsample)
  float* qprev;       // overlap-add history [B][512] <- qcur[b][last valid frame]
  // the fused final conv's tile-boundary shares (ResBlockArgs::fside): pcm[b][x * 128 + k] +=
  // fin_side[b][x][k], k < 2, for tiles x = 1 .. fin_T / 128 - 1 (fin_side == nullptr: none)
  float* fin_pcm = nullptr;
  const float* fin_side = nullptr;
  int fin_T = 0;
  long fin_ld = 0;  // fin_pcm's row stride (0: fin_T)
};
void step_commit(const CommitArgs& a, hipStream_t s);

// Admission reset of n slots (tts_model.rs:941 init_states per segment): zero the per-slot
// regions of up to 10 state buffers, backbone input = bos, SlotState / FlowLM / Mimi positions
// from the staged per-admission arrays (index i -> slots[i]). Rows admitted behind a latent prefix
// or onto their slot's codec state say so in opt_src[i].
constexpr int RESET_KEEP_CODEC = 1;  // leave buf[] and mpos of the row as they are
constexpr int RESET_LAT_SRC = 2;     // backbone input = lat_src[i] (the prefix's last latent), not bos
struct ResetArgs {
  float* buf[10];
  long per_slot[10];
  int nb;
  const int* slots;
  int n;
  float* lat_in;
  const float* bos;
  const SlotState* st_src;
  const int* fpos_src;
  FrameFlags* flags[NHB_MAX];  // every hand-off buffer: an undrained frame of the slot's previous
                         // utterance is discarded (null entries skipped)
  SlotState* st;
  int* fpos;
  int* mpos;
  // wire stage (null on an engine without it): the row's format from the staged array, no frames
  // received yet
  const int* wire_src = nullptr;
  int* wire_fmt = nullptr;
  int* wire_frames = nullptr;
  // tempo stage (null without it): the row's speed from the staged array, no frame, no hop yet
  const int* tempo_src = nullptr;
  int* tempo_sp = nullptr;
  int* tempo_state = nullptr;  // [max_slots][TEMPO_STATE]
  // pitch stage (null without it): the row's step from the staged array, no input, no output yet
  const unsigned* pitch_src = nullptr;
  unsigned* pitch_step = nullptr;
  int* pitch_state = nullptr;  // [max_slots][PITCH_STATE]
  // level stage (null without it): the row's gain bits from the staged array, no input yet
  const unsigned* level_src = nullptr;
  unsigned* level_gain = nullptr;
  int* level_state = nullptr;  // [max_slots][LEVEL_STATE]
  // loudness stage (null without it): the row's metered flag from the staged array, no sample yet
  const int* loud_src = nullptr;
  int* loud_state = nullptr;   // [max_slots][LOUD_STATE]
  // per-row RESET_* bits and staged backbone inputs [n][32] (null: no row of the admission has any)
  const int* opt_src = nullptr;
  const float* lat_src = nullptr;
};
void slot_reset(const ResetArgs& a, hipStream_t s);
// The first-frame preview pass's inputs, one launch: row i < n gets the latent and frame flags of
// row idx[i] of a hand-off buffer, rows n <= i < P zeros (no frame). idx travels in the kernel
// arguments (no host-to-device copy ahead of it).
constexpr int GATHER_MAX = 8;
void gather_preview(const float* lat, const FrameFlags* flags, const int* idx, int n, int P, float* lat_out,
                    FrameFlags* flags_out, hipStream_t s);

// TimestepEmbedder pair + RMSNorm + average (mlp.rs:76-133,296-319): out [n][512].
// tmp: scratch [2][n][512].
struct TimeEmbedWeights {
  const float* l1w[2];
  const float* l1b[2];
  const float* l2w[2];
  const float* l2b[2];
  const float* alpha[2];
};
void time_embeddings(const TimeEmbedWeights& w, int n, float* tmp, float* out, hipStream_t s);

// Token embedding gather: out[i] = table[ids[i]].
void embed_gather(const int* ids, int n, const float* table, int dim, float* out, hipStream_t s);
// The same for a prefill pass with latent-prefix rows (dim = 1024): src[i] >= 0 is a token id;
// PREFILL_SRC_BOS: out[i] = input_linear(bos); PREFILL_SRC_LAT0 - k: out[i] = input_linear(lat[k]),
// lat [*][32] staged latents, Wt the transposed input_linear weight [32][1024] (input_ln).
constexpr int PREFILL_SRC_BOS = -1, PREFILL_SRC_LAT0 = -2;
void prefill_input(const int* src, int n, const float* table, const float* lat, const float* bos, const float* Wt,
                   int dim, float* out, hipStream_t s);

// Strided copy: dst[r][c] = src[r][c] for rows x cols (used for small packing jobs).
void copy2d(const float* src, long lds, float* dst, long ldd, int rows, int cols, hipStream_t s);

// out[m] = sum_k x[m*ldx + k] * w[k] + b  (tiny GEMV column, e.g. the N=1 final conv)
// Streaming conv with Cout == 1: pcm[b][t] = bias + sum_{j,ci} elu(xin)[...] * w[j][ci] (Y's row
// stride ldy, 0: T).
void conv_cout1(const float* X, const float* H, int B, int T, int cin, int k, const float* w, const float* bias,
                float* Y, int elu_in, hipStream_t s, long ldy = 0);

// Fused SEANet residual block of one decoder stage (seanet.rs:43-89, kernels [3, 1], true skip):
// Y = elu(R + b1 + conv_k1(elu(b3 + conv_k3(E)))) over [B][T][C] channels-last rows, E's two rows
// before the frame from HE [B][2][C]. W3 [H][3][C] ([Cout][k][Cin]), W1 [C][H]. The intermediate
// stays in LDS. Stages: (C, H, T) = (256, 128, 96), (128, 64, 480), (64, 32, 1920).
struct ResBlockArgs {
  const float *E, *HE, *R, *W3, *b3, *W1, *b1;
  float* Y;
  int B, T, C;
  // stage 2 only (C == 64), optional: the final conv (64 -> 1, k = 3, seanet.rs:396-402) of the
  // tile's own rows in the epilogue, into fout [B][T]. A tile's first two outputs also need the
  // previous tile's last two rows: the tile stores its part of them, and its own two-row share of
  // the next tile's (fside [B][T / 128][2]) is added by the commit (CommitArgs::fin_*). The
  // utterance's first tile reads the conv history fH [B][2][64] instead.
  const float *fw = nullptr, *fb = nullptr, *fH = nullptr;
  float *fout = nullptr, *fside = nullptr;
  // E == R (the raw transposed-conv output): the k3 conv's input is elu(R), applied as the rows
  // enter LDS, so the transposed conv stores no ELU'd copy (HE stays ELU'd: the commit ELUs it)
  int e_raw = 0;
  int back_hi = 1;  // issue priority 3 (set by the launcher from set_back_hi)
  long fld = 0;     // fout's row stride (0: T; a pass block of more frames than this launch covers)
};
constexpr int RESBLOCK_FIN_TT = 128;  // stage-2 time tile (the side buffer's granularity)
void resblock(const ResBlockArgs& a, hipStream_t s);

// Encoder first conv (Cin == 1): Y[b][t][co] = bias[co] + sum_j w[co][j] * xpad[t + j], with
// the 6-sample zero history (constant padding, conv.py:90-108).
void conv_cin1(const float* X, int T, int cout, int k, const float* w, const float* bias, float* Y,
               hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Voice-prompt resampler: the polyphase FIR of scipy.signal.resample_poly (the Python reference's
// convert_audio, data/audio_utils.py:8-28; audio.rs:197-255 claims the same for Rust). Rates
// reduce by their gcd to up/down; taps h[0, L) with L = 2*half + 1, half = 10*max(up, down);
// y[m] = sum_j x[j] * h[m*down + half - j*up] for m < n_out, zeros for n_out <= m < n_pad.
struct ResamplePlan {
  int up = 1, down = 1, half = 0, L = 1;
  bool identity() const { return up == 1 && down == 1; }
  long out_len(long n) const { return (n * up + down - 1) / down; }
};
ResamplePlan resample_plan(int sr_from, int sr_to);
std::vector<float> resample_taps(const ResamplePlan& p);  // host FIR design (f32 taps x up)
void resample(const float* x, int n_in, const float* taps, const ResamplePlan& p, int n_out, int n_pad, float* y,
              hipStream_t s);

// Voice-job ingest: the clip in its wire format (mono f32, or mono int16 little-endian when
// fmt_s16: v / 32768, exact in f32) -> y [n_pad] in one launch: the kernel resample() runs,
// instantiated on the sample type (bit-equal to resample() on the converted samples by
// construction), zeros for n_out <= m < n_pad.
// An identity plan converts and pads (taps unused, may be null).
void voice_ingest(const void* x, int fmt_s16, int n_in, const float* taps, const ResamplePlan& p, int n_out,
                  int n_pad, float* y, hipStream_t s);
// ---------------------------------------------------------------------------------------------
// Wire stage: a row's f32 PCM at 24 kHz -> the bytes a client reads, inside the back part. Per row
// a format (encoding | rate index << 8; 0: none): 16-bit integer samples by the project's wire rule
// (audio.rs:110-185: trunc(clamp(x, -1, 1) * 32767) in f32), or the G.711 mu-law / A-law code of
// that 16-bit value, at one of WIRE_RATE_HZ. Rates other than 24 kHz resample by the rule above
// (the same tap loop as k_voice_ingest: one device function), streaming: after N samples of a row
// every output whose filter support is complete has been emitted, emitted(N) = floor((N up - 1 -
// half) / down) + 1, and the frame flagged `last` emits the rest up to N up / down, so a row's
// chunks concatenate to the whole-signal resample of its PCM, bit for bit. Per-row state: the
// frames received and the last WIRE_TAIL input samples; the admission reset (k_slot_reset) zeroes
// the count and writes the format.
constexpr int WIRE_NONE = 0, WIRE_S16 = 1, WIRE_ULAW = 2, WIRE_ALAW = 3;
// FLAC (below): k_wire treats the row as WIRE_S16 and records each chunk's first sample index
constexpr int WIRE_FLAC = 4;
constexpr int WIRE_RATES = 5;
constexpr int WIRE_RATE_HZ[WIRE_RATES] = {8000, 16000, 24000, 44100, 48000};
constexpr int WIRE_CHUNK_MAX = 8192;  // bytes per (row, frame) slot: 3860 16-bit samples at most
constexpr int WIRE_TAIL = 64;         // >= 2 half / up of every rate (60 at 8 kHz)
constexpr int WIRE_TAPS_MAX = 2944;   // >= L of every rate (2941 at 44.1 kHz)
struct WirePlan {
  int up, down, half, L, tap_off;  // tap_off: the rate's taps within WireArgs::taps
};
// On an engine with the tempo stage (below) a frame's input is the row's tempo chunk instead: `tin`
// [B][out_frames][TEMPO_OUT_MAX] and its sample counts `tcnt` for the rows whose tempo_sp is not 0,
// the PCM frame and 1920 for the others. The per-row state counts input samples, and a chunk longer
// than 1920 samples is walked in pieces of 1920 (the LDS window), so the emitted(N) rule is the same.
struct WireArgs {
  int B, nfr;               // rows, frames this pass decodes
  int pcm_frames;           // frames per row of the PCM block
  int out_frames;           // frames per row of `out` / `counts` (slots past nfr get count 0)
  const float* pcm;         // [B][pcm_frames][1920], after the commit
  const FrameFlags* flags[NFR_MAX];
  const int* fmt;           // [B]
  int* frames;              // [B] input samples of the row's utterance received so far
  float* tail;              // [B][WIRE_TAIL]
  const float* taps;
  WirePlan plan[WIRE_RATES];
  unsigned char* out;       // [B][out_frames][WIRE_CHUNK_MAX]
  int* counts;              // [B][out_frames] bytes of each chunk (0: no wire format or no frame)
  int chunk;                // bytes per (row, frame) slot of `out`: WIRE_CHUNK_MAX, _TEMPO or _LEVEL
  const int* tempo_sp = nullptr;  // [B] (null: no tempo stage)
  const float* tin = nullptr;
  const int* tcnt = nullptr;
  int* first = nullptr;     // [B][out_frames] (null: no FLAC stage) a WIRE_FLAC chunk's first output index
  // pitch stage (null without it): a row whose pitch_step is not 0 reads its pitch chunk instead,
  // `pin` [B][out_frames][PITCH_OUT_MAX] and its sample counts `pcnt`
  const unsigned* pitch_step = nullptr;  // [B]
  const float* pin = nullptr;
  const int* pcnt = nullptr;
  // level stage (null without it): a row whose level_gain is not 0 reads its level chunk instead,
  // `lin` [B][out_frames][LEVEL_OUT_MAX] and its sample counts `lcnt`
  const unsigned* level_gain = nullptr;  // [B]
  const float* lin = nullptr;
  const int* lcnt = nullptr;
};
void wire_stage(const WireArgs& a, hipStream_t s);
// n samples already at the wire rate -> n (G.711) or 2 n (16-bit) bytes; `out` holds the byte count
// rounded up to a multiple of 8
void wire_encode(const float* x, long n, int enc, unsigned char* out, hipStream_t s);

// Tempo stage: WSOLA time-scaling of a row's f32 PCM at 24 kHz by its speed
// sp (permille, [TEMPO_SP_MIN, TEMPO_SP_MAX]; 0: none), ahead of the wire stage. Hop k writes
// TEMPO_HS output samples from the segment at p_k = a_k + delta_k, a_k = floor(k Hs sp / 1000),
// delta_k the shift in [-D, D] that correlates best (f64, four ordered quarters of 120 products)
// with the continuation of the previous segment. Streaming: hop k runs in the first frame after
// which the row has a_k + TEMPO_R samples, the frame flagged `last` runs the rest up to
// tempo_len(N, sp), so a row's chunks concatenate to the whole-signal rule (tempo()) bit for bit.
// Per-row state: frames received, next hop, p of the last hop (tempo_state), and the last TEMPO_HIST
// input samples.
constexpr int TEMPO_W = 480, TEMPO_HS = 240, TEMPO_D = 120, TEMPO_R = TEMPO_D + TEMPO_HS + TEMPO_W;
constexpr int TEMPO_SP_MIN = 500, TEMPO_SP_MAX = 2000;
// input history: a pending hop has a_k > N - R, and reads no sample before
// min(a_k - D, p_{k-1} + Hs) >= a_k - (ceil(Hs SP_MAX / 1000) + D - Hs)
constexpr int TEMPO_BACK = (TEMPO_HS * TEMPO_SP_MAX + 999) / 1000 + TEMPO_D - TEMPO_HS;  // 360
constexpr int TEMPO_HIST = TEMPO_R + TEMPO_BACK;                                         // 1200
// samples of one chunk: the hops run before a last frame cover every a_k <= N_prev - R, so that
// frame emits < (1920 + R - 1) 1000 / sp + 1 <= 5519 (section 19); any other frame <= 3840 + Hs
constexpr int TEMPO_OUT_MAX = 5528;
constexpr int TEMPO_STATE = 4;  // ints per row: frames received, next hop k, p_{k-1}, unused
// bytes per (row, frame) slot on a tempo-enabled engine: 2 TEMPO_OUT_MAX + 21 samples at 48 kHz, 16 bit
constexpr int WIRE_CHUNK_MAX_TEMPO = 22528;
long tempo_len(long n, int sp);            // ceil(n 1000 / sp)
std::vector<float> tempo_window();         // [TEMPO_W] periodic Hann, f64 rounded to f32
struct TempoArgs {
  int B, nfr, pcm_frames, out_frames;      // as WireArgs
  const float* pcm;
  const FrameFlags* flags[NFR_MAX];
  const int* sp;                           // [B] speed (0: none)
  int* state;                              // [B][TEMPO_STATE]
  float* hist;                             // [B][TEMPO_HIST]
  const float* win;                        // [TEMPO_W]
  float* out;                              // [B][out_frames][TEMPO_OUT_MAX]
  int* counts;                             // [B][out_frames] samples of each chunk
};
void tempo_stage(const TempoArgs& a, hipStream_t s);
// whole signal: x [n] -> y [tempo_len(n, sp)], one workgroup, the hop functions of the stage
void tempo(const float* x, int n, int sp, const float* win, float* y, hipStream_t s);

// Pitch stage: a streaming fractional resampler between the tempo stage and
// the wire stage. A row with pitch `cents` has its PCM time-scaled by WSOLA at sp_w (pitch_plan) and
// then read at `step` / 2^20 input samples per output sample through a Kaiser-windowed sinc
// (PITCH_Z zero crossings a side, PITCH_P table entries per crossing, linear interpolation between
// entries, cutoff lowered to 1 / step when step > 2^20). Output m reads inputs i0 - H .. i0 + H,
// i0 = m step >> 20. Streaming: after N inputs every m with i0 + H <= N - 1 has been emitted, the
// frame flagged `last` emits the rest up to pitch_len(N, step), so a row's chunks concatenate to the
// whole-signal rule (pitch_resample()) bit for bit. Per-row state: step (0: none), inputs received,
// outputs emitted, the last PITCH_HIST inputs.
constexpr int PITCH_CENTS_MAX = 1200;
constexpr int PITCH_Z = 32, PITCH_P = 512;
constexpr double PITCH_BETA = 12.0;
constexpr int PITCH_TAB = PITCH_Z * PITCH_P + 1;          // (T[i], D[i]) pairs, 0 <= i <= Z P
constexpr unsigned PITCH_STEP_MIN = 1u << 19, PITCH_STEP_MAX = 1u << 21;
constexpr long pitch_cq(unsigned step) {                  // cutoff scale, Q20
  return (1L << 40) / step < (1L << 20) ? (1L << 40) / step : (1L << 20);
}
constexpr int pitch_support(unsigned step) {              // H: one-sided support in input samples
  return (int)((((long)PITCH_Z << 20) + pitch_cq(step) - 1) / pitch_cq(step)) + 1;
}
constexpr int PITCH_H_MAX = pitch_support(PITCH_STEP_MAX);  // 65
constexpr int PITCH_HIST = 2 * PITCH_H_MAX + 2;             // 132: the first pending output reads from N - 2 H on
// samples of one chunk: a last frame emits at most (tempo's last chunk + H) 2^20 / step, 5,588 over
// all valid (cents, speed) (section 23; pitch_enable recomputes it)
constexpr int PITCH_OUT_MAX = 5600;
constexpr int PITCH_STATE = 2;  // ints per row: inputs received, outputs emitted
static_assert(PITCH_HIST % 4 == 0 && PITCH_OUT_MAX % 4 == 0 && (2L * PITCH_OUT_MAX + 21) * 2 <= WIRE_CHUNK_MAX_TEMPO,
              "a pitch chunk at 48 kHz, 16 bit, fits the tempo-enabled chunk slot");
// host only: the WSOLA speed and the Q20 step of (cents, speed permille; 0: 1000); false: invalid
bool pitch_plan(int cents, int sp, int* sp_w, unsigned* step);
long pitch_len(long n, unsigned step);                    // floor(n 2^20 / step)
std::vector<float> pitch_table();                         // [PITCH_TAB][2]: T[i], D[i] = T[i+1] - T[i]
struct PitchArgs {
  int B, nfr, pcm_frames, out_frames;      // as WireArgs
  const float* pcm;
  const FrameFlags* flags[NFR_MAX];
  const unsigned* step;                    // [B] (0: none)
  const int* tempo_sp;                     // [B] the row's input is its tempo chunk (tin, tcnt) if not 0
  const float* tin;
  const int* tcnt;
  int* state;                              // [B][PITCH_STATE]
  float* hist;                             // [B][PITCH_HIST]
  const float* tab;                        // pitch_table()
  float* out;                              // [B][out_frames][PITCH_OUT_MAX]
  int* counts;                             // [B][out_frames] samples of each chunk
};
void pitch_stage(const PitchArgs& a, hipStream_t s);
// whole signal: x [n] -> y [pitch_len(n, step)], the tap loop of the stage
void pitch_resample(const float* x, int n, unsigned step, const float* tab, float* y, hipStream_t s);

// Level stage: a per-row gain and a look-ahead peak limiter between the pitch
// stage and the wire stage. With v the row's gain and C the engine's ceiling (f32, from level_plan):
// u[n] = v x[n]; r[n] = |u[n]| > C ? C / |u[n]| : 1 (1 outside the signal); m[i] = min(r[i .. i + L]);
// g[n] = (float)(sum_k w[k] m[n - k] / 4096), w[k] = 64 - |k - 63| for k = 0 .. L, summed in f64 in
// ascending k; y[n] = clamp(g[n] u[n], -C, C). Streaming: after N inputs a row has emitted the
// outputs below N - L, the frame flagged `last` emits the rest up to N, so a row's chunks
// concatenate to the whole-signal rule (level()) bit for bit. Per-row state: the gain's f32 bits
// (0: the row is not in the stage), the inputs received, the last LEVEL_HIST values of u.
constexpr int LEVEL_L = 126;                 // look-ahead in samples (5.25 ms); the taps are L + 1
constexpr int LEVEL_HIST = 2 * LEVEL_L;      // 252: the first pending output N - L reads r from N - 2 L on
constexpr int LEVEL_GAIN_CDB_MAX = 2400, LEVEL_CEIL_CDB_MIN = -4000;  // hundredths of a dB
// a frame's input is a PCM frame, a tempo chunk or a pitch chunk; its last frame emits L more
constexpr int LEVEL_IN_MAX = PITCH_OUT_MAX;
constexpr int LEVEL_OUT_MAX = LEVEL_IN_MAX + LEVEL_L + 2;  // 5728
constexpr int LEVEL_WINDOW = LEVEL_HIST + LEVEL_IN_MAX + LEVEL_L;  // 5978: history | input | L samples past it
constexpr int LEVEL_STATE = 1;  // ints per row: inputs received
// bytes per (row, frame) slot on a level-enabled engine: 2 LEVEL_OUT_MAX + 21 samples at 48 kHz, 16
// bit (a plain last frame: 2 (1920 + L) + 20 = 4,112 samples, above WIRE_CHUNK_MAX already)
constexpr int WIRE_CHUNK_MAX_LEVEL = 23552;
static_assert(LEVEL_IN_MAX >= TEMPO_OUT_MAX && LEVEL_IN_MAX >= 1920 && LEVEL_IN_MAX % 4 == 0 && LEVEL_OUT_MAX % 4 == 0 &&
                  LEVEL_HIST % 4 == 0 && LEVEL_OUT_MAX >= LEVEL_IN_MAX + LEVEL_L,
              "a level chunk holds the largest input chunk and the look-ahead");
static_assert((2L * LEVEL_OUT_MAX + 21) * 2 <= WIRE_CHUNK_MAX_LEVEL && WIRE_CHUNK_MAX_LEVEL % 8 == 0 &&
                  WIRE_CHUNK_MAX_LEVEL >= WIRE_CHUNK_MAX_TEMPO,
              "a level chunk at 48 kHz, 16 bit, fits the level-enabled chunk slot");
// host only: the f32 gain and ceiling of (gain_cdb, ceiling_cdb), (float)pow(10, cdb / 2000); false: out of range
bool level_plan(int gain_cdb, int ceiling_cdb, float* gain, float* ceiling);
struct LevelArgs {
  int B, nfr, pcm_frames, out_frames;      // as WireArgs
  const float* pcm;
  const FrameFlags* flags[NFR_MAX];
  const unsigned* gain;                    // [B] f32 bits of the row's gain (0: the row is not in the stage)
  float ceiling;
  // the row's input is its pitch chunk (pin, pcnt) if pitch_step is not 0, else its tempo chunk (tin,
  // tcnt) if tempo_sp is not 0, else the PCM frame (null: the engine has no such stage)
  const int* tempo_sp = nullptr;
  const float* tin = nullptr;
  const int* tcnt = nullptr;
  const unsigned* pitch_step = nullptr;
  const float* pin = nullptr;
  const int* pcnt = nullptr;
  int* state;                              // [B][LEVEL_STATE]
  float* hist;                             // [B][LEVEL_HIST]
  float* out;                              // [B][out_frames][LEVEL_OUT_MAX]
  int* counts;                             // [B][out_frames] samples of each chunk
};
void level_stage(const LevelArgs& a, hipStream_t s);
// whole signal: x [n] -> y [n], the window function of the stage
void level(const float* x, long n, float gain, float ceiling, float* y, hipStream_t s);

// Loudness stage: a BS.1770 meter beside the wire stage. It reads what k_wire
// reads for the row (PCM frame, tempo, pitch or level chunk), widens it to f64, runs the K-weighting
// (shelf, then high-pass; two biquads at 24 kHz) and writes the energy sum of y^2 of every complete
// sub-block of LOUD_SUB samples. Each biquad runs in segments of LOUD_G samples on the row's absolute
// sample index: a zero-state pass per segment, a sequential chain of two values per segment, a
// correction from the tables p and q. Every f64 operation is rounded once (no contraction) in the
// order section 27 states, so audio.loudness_blocks agrees bit for bit. Per-row state: the metered
// flag and the samples seen, the samples behind the last complete sub-block, six doubles (the last
// two inputs, shelf outputs and high-pass outputs at that sub-block's end).
constexpr int LOUD_SUB = 2400;       // samples of a sub-block (100 ms)
constexpr int LOUD_G = 32;           // samples of a segment
constexpr int LOUD_SEGS = LOUD_SUB / LOUD_G;  // 75
constexpr int LOUD_BLOCKS_MAX = 3;   // sub-blocks one chunk completes at most
constexpr int LOUD_IN_MAX = LEVEL_OUT_MAX;  // the largest chunk the wire stage reads
constexpr int LOUD_STATE = 2;        // ints per row: metered (0 / 1), samples seen
constexpr int LOUD_FILT = 6;         // doubles per row: x[-1], x[-2], shelf y[-1], y[-2], high-pass y[-1], y[-2]
static_assert(LOUD_SEGS * LOUD_G == LOUD_SUB, "a sub-block is a whole number of segments");
static_assert(LOUD_IN_MAX >= PITCH_OUT_MAX && LOUD_IN_MAX >= TEMPO_OUT_MAX && LOUD_IN_MAX >= 1920 &&
                  (LOUD_SUB - 1 + LOUD_IN_MAX) / LOUD_SUB == LOUD_BLOCKS_MAX,
              "a chunk completes at most three sub-blocks");
struct LoudCoef {
  double c[2][5];        // shelf, high-pass: b0 b1 b2 a1 a2
  double pq[2][2][LOUD_G];  // per biquad: p, q
};
struct LoudRecord {      // per (row, frame), in the pass block's head
  int n_blocks;          // 0 .. LOUD_BLOCKS_MAX
  int pad;
  double e[LOUD_BLOCKS_MAX];
};
static_assert(sizeof(LoudRecord) == 32, "a loudness record is 32 bytes");
// host only: the coefficients of section 27 at 24 kHz and their tables
void loud_coef(LoudCoef* k);
struct LoudArgs {
  int B, nfr, pcm_frames, out_frames;      // as WireArgs
  const float* pcm;
  const FrameFlags* flags[NFR_MAX];
  // the row's input, chosen as k_wire chooses it (null: the engine has no such stage)
  const int* tempo_sp = nullptr;
  const float* tin = nullptr;
  const int* tcnt = nullptr;
  const unsigned* pitch_step = nullptr;
  const float* pin = nullptr;
  const int* pcnt = nullptr;
  const unsigned* level_gain = nullptr;
  const float* lin = nullptr;
  const int* lcnt = nullptr;
  int* state;                              // [B][LOUD_STATE]
  float* pend;                             // [B][LOUD_SUB]
  double* filt;                            // [B][LOUD_FILT]
  LoudRecord* out;                         // [B][out_frames]
  LoudCoef k;
};
void loud_stage(const LoudArgs& a, hipStream_t s);
// whole signal: x [n] -> energy [n / LOUD_SUB], the block function of the stage
void loud_blocks(const float* x, long n, const LoudCoef& k, double* energy, hipStream_t s);

// FLAC stage: behind the wire stage, the 16-bit chunk of every WIRE_FLAC row
// becomes ceil(n / FLAC_BLOCK) FLAC frames (mono, 16 bit, fixed predictors of order 0..4, partitioned
// Rice codes, the exhaustive choice rule of section 21), written back to back over the chunk slot,
// and the chunk's count becomes their byte total. One workgroup per (row, frame slot); it holds the
// whole chunk in LDS before its first store, so encoding in place is safe. Integer arithmetic only.
constexpr int FLAC_BLOCK = 4608;                 // the subset limit at <= 48 kHz
constexpr int FLAC_FRAME_OVERHEAD = 17;          // 14 header, 1 subframe header, 2 CRC-16
constexpr int FLAC_CHUNK_FRAMES = 3;             // frames of a chunk, at most
// the slot bound above; the longest chunk is 11,058 of a tempo row, 11,196 of a pitch row (section 23),
// 11,448 of a level row behind the pitch stage (section 24)
constexpr int FLAC_CHUNK_SAMPLES = 2 * LEVEL_OUT_MAX + 21;
constexpr int flac_rate_code(int ri) { return ri == 0 ? 4 : ri == 1 ? 5 : ri == 2 ? 7 : ri == 3 ? 9 : 10; }  // by WIRE_RATE_HZ
constexpr long flac_bound(long n) {              // bytes of the frames of an n-sample chunk, at most
  return 2 * n + FLAC_FRAME_OVERHEAD * ((n + FLAC_BLOCK - 1) / FLAC_BLOCK);
}
static_assert(flac_bound(3860) <= WIRE_CHUNK_MAX, "a FLAC chunk fits the chunk slot");
static_assert(flac_bound(2 * PITCH_OUT_MAX + 21) <= WIRE_CHUNK_MAX_TEMPO && FLAC_CHUNK_SAMPLES <= FLAC_CHUNK_FRAMES * FLAC_BLOCK &&
                  2 * (2 * PITCH_OUT_MAX + 21) <= WIRE_CHUNK_MAX_TEMPO,
              "a FLAC chunk of a tempo row is at most three frames and fits the chunk slot");
static_assert(flac_bound(FLAC_CHUNK_SAMPLES) <= WIRE_CHUNK_MAX_LEVEL && 2 * FLAC_CHUNK_SAMPLES <= WIRE_CHUNK_MAX_LEVEL,
              "a FLAC chunk of a level row is at most three frames and fits the chunk slot");
static_assert(TEMPO_HS * WIRE_RATE_HZ[0] / 24000 >= 16, "the shortest non-last chunk (one tempo hop at 8 kHz) is a legal block");
struct FlacArgs {
  int B, out_frames;
  const int* fmt;           // [B] the wire formats
  const int* first;         // [B][out_frames] from k_wire
  unsigned char* out;       // the wire stage's chunk slots, encoded in place
  int* counts;              // [B][out_frames] in: bytes of the s16 chunk; out: bytes of its frames
  int chunk;
  // the frame index beside the chunk (section 21.5): each frame's byte length and block size, and the
  // chunk's frame count (0: the row is not FLAC, or the slot holds no chunk)
  int* index;               // [B][out_frames][FLAC_CHUNK_FRAMES][2]
  int* nframes;             // [B][out_frames]
};
void flac_stage(const FlacArgs& a, hipStream_t s);
// the stage's chunk encoder on n <= FLAC_CHUNK_SAMPLES samples (device pointers): frames into `out`
// (flac_bound(n) bytes rounded up to a multiple of 4), their byte total into *n_bytes, and (index
// not null) each frame's byte length and block size into index [ceil(n / FLAC_BLOCK)][2]
void flac_encode(const short* x, int n, int rate_index, long long first_sample, unsigned char* out, int* n_bytes,
                 int* index, hipStream_t s);

// dst [nch][rows][cols]: row r of chunk c = src[c * chunk_stride .. + cols) (each encoder chunk's
// first row replicated: the history of the chunked ConvDownsample1d), one launch over all chunks
void replicate_chunks(const float* src, long chunk_stride, float* dst, int nch, int rows, int cols, hipStream_t s);

// The Rust driver's resampler instead (audio.rs:197-255): rubato 0.14.1 FastFixedIn with
// PolynomialDegree::Septic, one process() call over the whole input (chunk = n). Its source is not
// in the reference; the published algorithm restated here: a read position idx starts at -4
// (half the 8-point window), advances by t = sr_from / sr_to in f64 before each output, and
// outputs continue while the position before the step is < n - 9; output m is the degree-7
// Lagrange polynomial through x[s-3 .. s+4] (zeros outside the input), s = floor(idx), at
// frac = (f32)(idx - s). septic_schedule() replays the f64 position walk on the host (count, and
// per output s and frac when the vectors are given); resample_septic() evaluates the outputs, one
// lane each, in a fixed f32 operation order (no contraction), zeros for n_out <= m < n_pad.
long septic_schedule(long n, int sr_from, int sr_to, std::vector<int>* start, std::vector<float>* frac);
void resample_septic(const float* x, int n_in, const int* start, const float* frac, int n_out, int n_pad, float* y,
                     hipStream_t s);

}  // namespace ptts
