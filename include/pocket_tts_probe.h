/* pocket_tts_probe.h - measurement and test hooks of libpocket_tts_hip.so.
 *
 * Not part of the drop-in boundary (include/pocket_tts.h): nothing in the reference corresponds
 * to these, and a reference-side binding never declares them. bench.py, the
 * GPU tests and tools/ use them to time single kernels of the step plan, list the plan with its
 * algorithmic costs, probe front/back overlap and test the GEMM core and the attention path on off-model operands. Same
 * conventions as pocket_tts.h (status codes, the thread-local last-error message).
 */
#ifndef POCKET_TTS_PROBE_H
#define POCKET_TTS_PROBE_H

#include "pocket_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook of the GEMM core (no reference counterpart): y = x w^T for x [m][k], w [n][k] (host
 * buffers) on the engine's device, with the tile of id `layout` (the table PTTS_TILES of
 * csrc/kernels.h: the f32 tiles, + 100 for their bf16-operand twins, + 200 for the bf16x6 ones);
 * splits > 1 writes the [splits][m][n] split-K partial slabs to y, tail_slices > 0 takes the
 * split-tail path. PTTS_ERR_INVALID, with a message, for a tile id that is not in this build,
 * tail_slices > 0 on a tile without the split tail, and a k that is not a multiple of the tile's
 * BK (ptts_gemm_tiles lists all three per tile). The tests run every shipped tile on shapes the
 * model never runs. */
int ptts_test_gemm(ptts_engine* e, int layout, int m, int n, int k, int splits, int tail_slices, const float* x,
                   const float* w, float* y);
/* The GEMM tiles of this build, one line per tile: "id<TAB>tm<TAB>tn<TAB>bk<TAB>operands<TAB>tail"
 * (tile M x N, K chunk, operands f32 | bf16 | bf16x6, tail 1 where tail_slices > 0 is served).
 * Needs no engine and no GPU. */
int ptts_gemm_tiles(char* buf, int buflen);
/* Test hook of the attention path (no reference counterpart): the product launchers, unchanged, on
 * host operands, so the tests can compare RoPE, the KV append and the softmax with fp64 on operands
 * the model never produces. kind PTTS_ATTN_PREFILL: qkv_rope_append + attention (FlowLM
 * prefill, Mimi multi-frame pass); PTTS_ATTN_MIMI_STEP: attention16_qkv (RoPE and ring append fused,
 * 16 rows per slot; cap < window + 16 is refused as in the product); PTTS_ATTN_FLOW_STEP:
 * attention_step_qkv with the engine's rope_table (one row per slot, window 0).
 *   qkv  [m][3 nh 64] dense rows (splits == 0) or [splits][m][3 nh 64] partial slabs;
 *   kv   [n_slots][2][nh][cap][64], in: the store before the call, out: after it;
 *   pre  optional shared prefixes, slot s's [2][nh][F_s][64] back to back, F_s = pre_len[s]
 *        (positions < F_s of slot s are read from it; window 0, not the Mimi step);
 *   rows -> (slot, position): uniform, slot = slot0 + row / rps at (pos ? pos[slot] : p0) + row % rps
 *        (16-row groups must not straddle slots), or, PREFILL only, tab [m] = slot << 16 | position
 *        with -1 padding rows closing a 16-row group; with ptab [mpad] as well, tab holds the tokens
 *        only and ptab the padded groups (the compact batched admission: Q is [mpad] rows);
 *   q    out, PREFILL only: the rotated queries [m or mpad][nh 64];  o  out [m][nh 64].
 * Every position must lie inside the store unless it is a ring (cap a power of two, window > 0). */
enum { PTTS_ATTN_PREFILL = 0, PTTS_ATTN_MIMI_STEP = 1, PTTS_ATTN_FLOW_STEP = 2 };
int ptts_test_attention(ptts_engine* e, int kind, int m, int nh, int cap, int window, int n_slots, int splits,
                        const float* qkv, float* kv, const float* pre, const int* pre_len, int slot0, int rps, int p0,
                        const int* pos, const int* tab, const int* ptab, int mpad, float* q, float* o);
/* Measurement: replay one named kernel of the step plan `reps` times between HIP events on
 * the engine stream; returns the average duration in microseconds. */
int ptts_time_kernel(ptts_engine* e, int n_rows, const char* name, int reps, double* avg_us);
/* The step plan for n_rows: one line per op, "name<TAB>flops<TAB>bytes" (algorithmic cost of one
 * launch; 0 where not modelled). */
int ptts_plan_ops(ptts_engine* e, int n_rows, char* buf, int buflen);

/* Measurement: the step plan split at the FlowLM/flow-head -> Mimi boundary, timed as two
 * graphs alone and launched together on two streams; us8 = {front, back, both, both with the
 * front on a high-priority stream, 0, 0, 0, 0} microseconds per step. Clobbers engine state
 * (timing only). */
int ptts_probe_overlap(ptts_engine* e, int n_rows, int reps, double* us8);

#ifdef __cplusplus
}
#endif
#endif
