// qqq_lora.hip.h -- the batched LoRA op (include/qqq_amd_lora.h): fp16 low-rank adapters added to a W4A8 GEMM's output,
// the adapter of every token read from device memory.  One kernel, one launch.  Part of the single translation unit qqq_w4a8.hip.
//
//   qqq_lora_add_kernel<R>  grid (token tiles, column chunks): a workgroup of 8 waves owns 16 tokens and a chunk of the columns of ONE
//                           part (lora_chunk_width(): a multiple of 64, from the shapes alone; few tokens -> many chunks, many tokens ->
//                           one chunk per part).
//     shrink   for every DISTINCT slot of the tile (a wave-uniform loop over LDS) the workgroup computes h[r][token] = sum_k A[r][k] * xq[token][k]
//              for all 16 tokens with v_mfma_f32_16x16x32_f16: the adapter's rows are the MFMA's A operand, the tokens its B operand, xq
//              converted to fp16 (exact).  A wave takes the 128-wide k blocks  wave, wave + 8, ...: four MFMAs each, operands in the natural
//              order (lane group g holds k = 32 j + 8 g ... + 7 of MFMA j), so the four groups of a row read one 64-byte line of A per load.
//              A lane keeps the accumulators of the pass that is its own token's slot and discards the others; no barrier stands between
//              two passes.  Behind the last pass the eight waves' partial tiles meet in LDS once and are added in wave order, and h = s1 * sum.
//              Every workgroup of a token tile repeats the shrink of its part (the adapters live in L2): no intermediate in memory, no
//              second launch.
//     expand   a thread owns two adjacent columns: per token of the tile with a slot, the two rows of B (kept in registers while the slot
//              does not change), an f32 FMA chain over r against h (LDS broadcast), then y <- fp16(fma(scale, sum, float(y))), one 4-byte
//              read-modify-write.  A token without a slot is never touched.
//   What a row's bits depend on: its own xq, s1, y, and its slot's matrices -- the k split (a function of K), the wave order and the r
//   order are the same for every tile, every T and every chunking, a row's place in its tile only picks the MFMA column, and the rows of
//   other slots in a pass are computed and thrown away.
#ifndef QQQ_AMD_QQQ_LORA_HIP_H_
#define QQQ_AMD_QQQ_LORA_HIP_H_

static constexpr int LORA_NT = 512;
static constexpr int LORA_WAVES = LORA_NT / 64;
static constexpr int LORA_TILE = 16;            // tokens of a workgroup: the MFMA's columns
static constexpr int LORA_KBLOCK = 128;         // k of one wave iteration: four MFMAs of 32
static constexpr int LORA_TARGET_GROUPS = 128;  // workgroups a launch aims at when the tokens are few (each repeats the shrink of its tile)

typedef float lora_f4 __attribute__((ext_vector_type(4)));

struct qqq_lora_args {
  unsigned short* y;
  const signed char* xq;
  const float* s1;
  const _Float16* A;
  const _Float16* B;
  const float* scale;
  const int* slot;
  long long ldy, a_stride, b_stride;
  int T, N, K, S, P;
  int pc[4];    // part_cols, padded with N
  int chunk_w;  // columns of a chunk
};

// the columns of a chunk: a function of the shapes alone (the widest part split so that tiles * chunks reaches LORA_TARGET_GROUPS)
static inline int lora_chunk_width(const int T, const int P, const int* part_cols) {
  const int tiles = (T + LORA_TILE - 1) / LORA_TILE;
  int widest = 64;
  for (int p = 0; p < P; ++p) widest = part_cols[p + 1] - part_cols[p] > widest ? part_cols[p + 1] - part_cols[p] : widest;
  int per_part = (LORA_TARGET_GROUPS + tiles * P - 1) / (tiles * P);
  per_part = per_part < 1 ? 1 : per_part;
  const int share = (widest + per_part - 1) / per_part;
  return (share + 63) / 64 * 64;
}
static inline int lora_chunks(const int P, const int* part_cols, const int chunk_w) {
  int n = 0;
  for (int p = 0; p < P; ++p) n += (part_cols[p + 1] - part_cols[p] + chunk_w - 1) / chunk_w;
  return n;
}

// 8 int8 (two dwords, little endian) -> 8 fp16, exactly
__device__ __forceinline__ h8 lora_cvt8(const int lo, const int hi) {
  h8 o;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    o[b] = (_Float16)(int)(signed char)(lo >> (8 * b));
    o[4 + b] = (_Float16)(int)(signed char)(hi >> (8 * b));
  }
  return o;
}

template <int R>
__global__ __launch_bounds__(LORA_NT) void qqq_lora_add_kernel(const qqq_lora_args a) {
  constexpr int RB = (R + 15) / 16;  // 16-row blocks of the adapter's A (R = 8: one block, its upper half zero)
  __shared__ float part_s[LORA_WAVES][RB * 16][LORA_TILE];
  __shared__ __attribute__((aligned(16))) float h_s[LORA_TILE][R];
  __shared__ int slot_s[LORA_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * LORA_TILE;

  // the chunk's part and columns (workgroup-uniform)
  int p = 0, c = blockIdx.y;
  for (; p < a.P - 1; ++p) {
    const int lo = p == 0 ? a.pc[0] : a.pc[1], hi = p == 0 ? a.pc[1] : a.pc[2];
    const int chunks = (hi - lo + a.chunk_w - 1) / a.chunk_w;
    if (c < chunks) break;
    c -= chunks;
  }
  const int part_lo = p == 0 ? a.pc[0] : p == 1 ? a.pc[1] : a.pc[2];
  const int part_hi = p == 0 ? a.pc[1] : p == 1 ? a.pc[2] : a.pc[3];
  const int col0 = part_lo + c * a.chunk_w;
  const int col1 = col0 + a.chunk_w < part_hi ? col0 + a.chunk_w : part_hi;
  if (col0 >= col1) return;

  if (tid < LORA_TILE) {
    const int t = t0 + tid;
    int s = t < a.T ? a.slot[t] : -1;
    if (s < 0 || s >= a.S) s = -1;  // an index outside [0, S) never becomes an address
    slot_s[tid] = s;
  }
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int i = 0; i < LORA_TILE; ++i) any |= slot_s[i] >= 0;
  if (!any) return;  // (workgroup-uniform)

  // ---- shrink: one pass per distinct slot of the tile; a lane keeps the pass of its own token's slot, the waves meet once at the end
  const int row = lane & 15, g = lane >> 4;  // the lane's adapter row / token, and its k group
  const int tok = t0 + row;
  const bool tok_ok = tok < a.T;
  const int my_slot = slot_s[row];
  const signed char* xrow = a.xq + (long long)(tok_ok ? tok : 0) * a.K + 8 * g;
  lora_f4 keep[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) keep[rb] = lora_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int i = 0; i < LORA_TILE; ++i) {
    const int sa = slot_s[i];
    bool first = sa >= 0;
    for (int j = 0; j < i; ++j) first &= slot_s[j] != sa;
    if (!first) continue;  // (workgroup-uniform: slot_s is shared)
    const _Float16* Ap = a.A + (long long)sa * a.a_stride + ((long long)p * R + row) * a.K + 8 * g;
    lora_f4 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = lora_f4{0.f, 0.f, 0.f, 0.f};
    for (int kb = wave * LORA_KBLOCK; kb < a.K; kb += LORA_WAVES * LORA_KBLOCK) {
      // MFMA j of the block sums k = kb + 32 j + 8 g + (0 ... 7): the four k groups of a row read one 64-byte line per load
      h8 xf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int lo = 0, hi = 0;
        if (tok_ok && kb + 32 * j < a.K) {  // K is a multiple of 64: a block of 32 k is all inside or all outside
          lo = *reinterpret_cast<const int*>(xrow + kb + 32 * j);
          hi = *reinterpret_cast<const int*>(xrow + kb + 32 * j + 4);
        }
        xf[j] = lora_cvt8(lo, hi);
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        h8 af[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          af[j] = h8{0, 0, 0, 0, 0, 0, 0, 0};
          if (rb * 16 + row < R && kb + 32 * j < a.K) af[j] = *reinterpret_cast<const h8*>(Ap + (long long)rb * 16 * a.K + kb + 32 * j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[j], xf[j], acc[rb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) keep[rb] = my_slot == sa ? acc[rb] : keep[rb];  // the other slots' tokens discard this pass
  }
  // the accumulator tile: column (token) = lane & 15, row (r) = 4 * (lane >> 4) + register
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int e = 0; e < 4; ++e) part_s[wave][rb * 16 + 4 * g + e][row] = keep[rb][e];
  __syncthreads();
  for (int idx = tid; idx < RB * 16 * LORA_TILE; idx += LORA_NT) {
    const int r = idx / LORA_TILE, t = idx % LORA_TILE;
    float s = part_s[0][r][t];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) s += part_s[w][r][t];
    if (r < R && slot_s[t] >= 0) h_s[t][r] = a.s1[t0 + t] * s;  // (slot_s[t] >= 0 implies t0 + t < T)
  }
  __syncthreads();

  // ---- expand: two columns per thread, the tile's tokens in order
  const int pairs = (col1 - col0) >> 1;
  for (int cp = tid; cp < pairs; cp += LORA_NT) {
    const int n = col0 + 2 * cp;
    h8 b0[R / 8], b1[R / 8];
    float sc = 0.f;
    int held = -1;
#pragma unroll 1
    for (int i = 0; i < LORA_TILE; ++i) {
      const int sa = slot_s[i];
      if (sa < 0) continue;
      if (sa != held) {
        const h8* bp = reinterpret_cast<const h8*>(a.B + (long long)sa * a.b_stride + (long long)n * R);
#pragma unroll
        for (int q = 0; q < R / 8; ++q) {
          b0[q] = bp[q];
          b1[q] = bp[R / 8 + q];
        }
        sc = a.scale[sa];
        held = sa;
      }
      float s0 = 0.f, s1 = 0.f;
      const lora_f4* hp = reinterpret_cast<const lora_f4*>(&h_s[i][0]);
#pragma unroll
      for (int q = 0; q < R / 8; ++q) {
        const lora_f4 ha = hp[2 * q], hb = hp[2 * q + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 = fmaf((float)b0[q][e], ha[e], s0);
          s1 = fmaf((float)b1[q][e], ha[e], s1);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 = fmaf((float)b0[q][4 + e], hb[e], s0);
          s1 = fmaf((float)b1[q][4 + e], hb[e], s1);
        }
      }
      h2* yp = reinterpret_cast<h2*>(a.y + (long long)(t0 + i) * a.ldy + n);
      const h2 yv = *yp;
      h2 o;
      o[0] = (_Float16)fmaf(sc, s0, (float)yv[0]);
      o[1] = (_Float16)fmaf(sc, s1, (float)yv[1]);
      *yp = o;
    }
  }
}

static void lora_launch(const int R, const dim3 grid, hipStream_t stream, const qqq_lora_args& a) {
  switch (R) {
    case 8: hipLaunchKernelGGL(qqq_lora_add_kernel<8>, grid, dim3(LORA_NT), 0, stream, a); break;
    case 16: hipLaunchKernelGGL(qqq_lora_add_kernel<16>, grid, dim3(LORA_NT), 0, stream, a); break;
    case 32: hipLaunchKernelGGL(qqq_lora_add_kernel<32>, grid, dim3(LORA_NT), 0, stream, a); break;
    default: hipLaunchKernelGGL(qqq_lora_add_kernel<64>, grid, dim3(LORA_NT), 0, stream, a); break;
  }
}

#endif  // QQQ_AMD_QQQ_LORA_HIP_H_
