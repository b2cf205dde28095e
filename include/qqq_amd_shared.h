/*
 * qqq_amd_shared.h -- C-ABI of the decode attention over the block-table (paged) KV cache for rows that share a prefix: the n completions of
 * one prompt (parallel sampling), whose block tables name the prompt's full blocks in common (exported by libqqq_amd.so, beside
 * include/qqq_amd_paged.h, whose pools, block tables and conventions these entry points share).
 *
 * A family is the set of rows of one call that were forked from one prompt; its members are siblings and adjacent.  The queries of up to
 * `pack` siblings ride in the 16-row MFMA tiles of qqq_decode_attn_paged's split kernel (up to four tiles, as for a verify chunk of
 * include/qqq_amd_verify.h), for the splits that lie wholly inside the keys they share: K and V of those splits are read once per KV head
 * and pack instead of once per row.  Every other split is computed per row.  For finite cache rows o_fp16, xq and s1 of every row are bit
 * for bit those of qqq_decode_attn_paged(_kv8) with the same b, kvh, max_len, tables and pos; with pack = 1, or when no row has a sibling,
 * the call is that call.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  b = 0 is a no-op.  The launch sizes depend on (b, h, kvh, max_len,
 * pack) alone, so a captured graph replays with other families, lengths and positions.
 */
#ifndef QQQ_AMD_SHARED_H_
#define QQQ_AMD_SHARED_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Two launches over an fp16 pool, the second one qqq_decode_attn's combine.  Every argument of qqq_decode_attn_paged, and
 *   family   int32 [b] in device memory: family[i] is the index of the first row of row i's family (a lone row names itself)
 *   shared   int64 [b] in device memory: the number of leading keys row i has in common with its family, the same on every member
 *            (0 for a lone row).  Rows of a family must hold equal table entries for their first shared / block_size blocks.
 *   pack     the number of sibling rows whose queries share one workgroup: pack >= 1 and (h / kvh) * pack <= 64
 * A family's rows fall into packs of `pack` consecutive rows counted from its first row; a family larger than pack reads its prefix once
 * per pack.  A split (the chunk of qqq_decode_attn_shared_plan) is taken jointly by the members of a pack whose pos is in [0, max_len) and
 * for which it lies inside the first min(shared[i], pos[i] + 1) keys; its blocks are read through the table row of the first such member.
 * A row with pos outside [0, max_len) writes nothing and does not disturb its siblings, wherever in its family or pack it stands; its
 * table row may hold anything.  Block ids that are read are clamped into [0, num_blocks).
 * A descriptor that makes no sense -- family[i] > i, a negative value, family[family[i]] != family[i], shared[i] > pos[i] + 1 (clamped per
 * member) or negative -- makes rows compute alone or share less; it never causes an access outside the arrays.
 * Shapes: the limits of qqq_decode_attn_paged.  Alignment: as there; family 4 bytes, shared 8 bytes.
 */
int qqq_decode_attn_paged_shared(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                 const void* pos, const void* family, const void* shared, int pack, float scale, void* o_fp16, void* xq,
                                 void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks,
                                 int block_size, int max_len, int dev, void* stream);

/*
 * The same over an int8 pool (k_scale, v_scale f32 [num_blocks, kvh, block_size], 4-byte aligned), with qqq_decode_attn_paged_kv8's
 * arithmetic.
 */
int qqq_decode_attn_paged_shared_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                     const void* block_table, int table_stride, const void* pos, const void* family, const void* shared,
                                     int pack, float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes,
                                     int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int dev, void* stream);

/*
 * Host only: the split plan of such a call on the calling thread's current device (256 compute units are assumed where there is none) --
 * qqq_decode_attn_paged's for (b, kvh, max_len): *chunk keys per split, a multiple of 128, and *splits = ceil(max_len / *chunk).  Split s
 * covers keys s * chunk ... (s + 1) * chunk - 1; it is taken jointly where (s + 1) * chunk <= shared.  QQQ_ERR_ARG for b < 1, a shape or
 * a pack the entry points refuse, or a NULL result pointer.
 */
int qqq_decode_attn_shared_plan(int b, int h, int kvh, int max_len, int pack, int* splits, int* chunk);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_SHARED_H_ */
