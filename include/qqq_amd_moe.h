/*
 * qqq_amd_moe.h -- C-ABI of the three ops of a mixture-of-experts MLP (exported by libqqq_amd.so, beside include/qqq_amd.h and the other
 * per-feature headers): the router's top-k with the sort of its (token, slot) pairs by expert, the grouped W4A8 GEMM over the routed rows,
 * and the weighted combine.  A token t with top_k experts makes the pairs p = t * top_k + j, j = 0 .. top_k - 1.
 *
 * qqq_moe_route
 *   logits   fp16 [T, E], row stride ld elements (ld >= E), 2-byte aligned: the router's output
 *   ids      int32 [T, top_k], w  f32 [T, top_k], offsets  int32 [E + 1], order  int32 [T * top_k]: outputs, 4-byte aligned
 *   Per row:  x[e] = float(logits[t, e]);  mx = max_e x[e];  u[e] = expf(x[e] - mx);  sum = the f32 sum of u (a lane's experts e = l,
 *   l + 64, l + 128, l + 192 ascending, then an xor butterfly over the 64 lanes);  the probability is prob[e] = u[e] / sum.  Slot j takes
 *   the largest u -- the largest prob: one positive divisor -- among the experts not taken by slots 0 .. j - 1, the LOWER index among
 *   equal ones: ids[t, j] = that expert, descending.  w[t, j] = u[ids[t, j]] / sum, an f32 division; with renorm != 0 it is
 *   prob[ids[t, j]] / (prob[ids[t, 0]] + ... + prob[ids[t, top_k - 1]]) with the row's sum cancelled: u[ids[t, j]] / (u[ids[t, 0]] + ... +
 *   u[ids[t, top_k - 1]]), the f32 sum in slot order and ONE f32 division (transformers' Qwen3MoeTopKRouter with norm_topk_prob; Mixtral's
 *   router always renormalises).
 *   A NaN u orders below every number, and taken experts are tracked by a flag, so a row of NaN or +-inf logits still gives top_k
 *   DISTINCT ids inside [0, E); its weights may be NaN.
 *   order[] lists the pairs p sorted by ids[p], pairs of one expert ascending in p (a stable counting sort); offsets[e] is the first
 *   position of expert e in order[], offsets[E] = T * top_k.  offsets and order are a pure function of ids: no atomic decides a position.
 *   Two launches: one wave per row, then ONE workgroup that sorts (chunks of 1024 pairs: ballots inside a wave, scans across waves and
 *   chunks).  Limits: 0 <= T, T * top_k <= 131072, 2 <= E <= 256, 1 <= top_k <= min(E, 16).
 *
 * qqq_moe_gemm
 *   xq       int8 [R, K] contiguous, 16-byte aligned;  s1  f32 [R]: per-token quantised activation rows
 *   B        int32 [E, K / 16, 2 N], s2  f32 [E, N], s3  fp16 [E, K / 128, N] or NULL (per-channel; group_size = -1): the experts' packed
 *            weights and scales stacked, every slice in exactly the layout and stored scale order qqq_w4a8_gemm reads; 16-byte aligned
 *   ids      int32 [P]: taken for the interface's symmetry and not read -- a pair's expert is where offsets[] puts it
 *   offsets  int32 [E + 1], order  int32 [P]: qqq_moe_route's;  P pairs
 *   D        fp16 [P, N] contiguous, 8-byte aligned, in PAIR order
 *   Pair p = order[i], offsets[e] <= i < offsets[e + 1], reads activation row p / a_div (a_div = top_k: the token's row, for gate | up;
 *   a_div = 1: the pair's own row, for down; R >= ceil(P / a_div)) and
 *       D[p, n] = fp16( ( float(sum_k xq[p / a_div, k] * Wq_e[k, n]) * s2[e, n] ) * s1[p / a_div] )
 *   with an exact int32 sum, two separate f32 multiplies and one rounding to fp16; Wq_e is expert e's int8 weight operand (16 * w4
 *   per-channel; per-group re-quantised from s3 with one packed-fp16 FMA as the dense kernels do).  Row p is bit for bit the row
 *   qqq_w4a8_gemm gives for that activation row against expert e's slices, whatever the other rows, their number or their order in
 *   order[].  A pair that order[] does not list is not written.  Any number of rows per expert, none included.
 *   One launch: a workgroup per (128-column strip, expert), no split-K across workgroups, no workspace; a workgroup whose expert has no
 *   rows leaves at once, the others walk the rows in passes of up to 64.  offsets[] are held inside [0, P] and pair indices inside [0, P),
 *   so garbage in them gives garbage rows of D and never an access outside the arrays.
 *   Limits: K a positive multiple of 128, N of 64, 1 <= E <= 256, 0 <= P <= 2097152, group_size in {-1, 128}, a_div >= 1.
 *
 * qqq_moe_combine
 *   y        fp16 [T * top_k, H] contiguous, 16-byte aligned;  w  f32 [T, top_k];  out  fp16 [T, H] contiguous, 16-byte aligned
 *       out[t, h] = fp16( (...((0.0f + w[t, 0] * float(y[t * top_k, h])) + w[t, 1] * float(y[t * top_k + 1, h])) + ...) )
 *   every product and every sum a separate f32 operation (no fused multiply-add), slot order, one rounding to fp16.  One launch.  A row's
 *   bits depend on that row alone.  Nothing is skipped: w = 0 against a NaN or inf y gives NaN.
 *   Limits: H a positive multiple of 8, 1 <= top_k <= 16, 0 <= T <= 1048576.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (safe under hipGraph capture),
 * no allocation, no state, nothing read on the host; the launch sizes depend on the shapes alone, so a captured step replays with other
 * routings.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad
 * arguments are rejected before any launch.  No tokens (T == 0, P == 0) is a no-op (NULL pointers allowed).
 */
#ifndef QQQ_AMD_MOE_H_
#define QQQ_AMD_MOE_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_moe_route(const void* logits, int ld, void* ids, void* w, void* offsets, void* order, int T, int E, int top_k, int renorm, int dev,
                  void* stream);

int qqq_moe_gemm(const void* xq, const void* s1, const void* B, const void* s2, const void* s3, const void* ids, const void* offsets,
                 const void* order, void* D, int P, int R, int E, int N, int K, int a_div, int group_size, int dev, void* stream);

int qqq_moe_combine(const void* y, const void* w, void* out, int T, int top_k, int H, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_MOE_H_ */
