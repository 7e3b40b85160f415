/* test_hooks.h - C-ABI test hooks of libpocket_tts_hip.so that live beside the library's sources,
 * not under include/: include/pocket_tts_probe.h holds a fixed list of hooks (tests/test_boundary.py
 * compares the header and the Python binding's signature table with it), so a hook added for one
 * kernel's test is declared here and bound by its caller (pocket_tts_amd.Engine.test_row_reduce, .test_align).
 * Same conventions as pocket_tts.h (status codes, the thread-local last-error message).
 */
#ifndef POCKET_TTS_TEST_HOOKS_H
#define POCKET_TTS_TEST_HOOKS_H

#include "pocket_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook of the row reduce (no reference counterpart): the product launcher row_reduce on host
 * operands (RowReduceArgs of kernels.h):
 *   v = sum_z p[z][m][n] (+ bias[n]); v = act(v) (0 none, 1 GELU); v *= gate[m][n]; v += r[m][n];
 *   y[m][n] = v;  with ln: h = LN(v) over the row (biased variance, eps) (* ln_w + ln_b)
 *   (* (1 + mscale[m][n]) + mshift[m][n]);  with hfrag (ln, n == 1024, m <= 32): h as well in the
 *   whole-K skinny GEMM's A-fragment order (32 x 1024 floats, rows >= m unwritten).
 * p [splits][m][n] (1 <= splits <= 16), n % 4 == 0, ln needs n <= 1024; bias / gate / r / ln_w with
 * ln_b / mscale with mshift may be NULL (absent); front != 0 marks a launch of the step's front part
 * (a 512-wide front row keeps the one-row kernel). y [m][n], h [m][n] (ln), hfrag [32][1024]. */
int ptts_test_row_reduce(ptts_engine* e, int m, int n, int splits, int act, int ln, float eps, int front,
                         const float* p, const float* bias, const float* gate, const float* r, const float* ln_w,
                         const float* ln_b, const float* mscale, const float* mshift, float* y, float* h,
                         float* hfrag);


/* Test hook of the align stage (no reference counterpart): the product launcher (k_align) on host
 * operands, in ptts_test_attention's PTTS_ATTN_FLOW_STEP form (pocket_tts_probe.h): row r is slot r.
 *   qkv  [m][3 nh 64] dense rows (splits == 0) or [splits][m][3 nh 64] partial slabs;
 *   kv   [m][2][nh][cap][64], read only;
 *   pre  optional shared prefixes as in ptts_test_attention (handed to the launcher as the engine
 *        hands them; the text keys are never read from them);
 *   pos  [m] the rows' positions (<= cap; the query rotates at min(pos, cap - 1));
 *   tab  [m][2] = {t0, n}: the first text position and the token count (n == 0: not in the stage);
 *   out  [m][1 + PTTS_ALIGN_TOKENS] 4-byte words, in and out: the int count, then the row (zeros
 *        behind n); a row with n == 0 gets count 0 and keeps its floats. */
int ptts_test_align(ptts_engine* e, int m, int nh, int cap, int splits, const float* qkv, const float* kv,
                    const float* pre, const int* pre_len, const int* pos, const int* tab, unsigned head_mask,
                    float* out);

#ifdef __cplusplus
}
#endif
#endif
