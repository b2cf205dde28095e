// qqq_hessian_grouped.hip.h -- the kernel of qqq_hessian_update_grouped (qqq_amd/quant/include/qqq_amd_hessian_grouped.h): the running
// Hessians of all E experts of a mixture-of-experts layer,
//   H_e <- f32(f32(alpha[e] H_e) + f32(beta[e] S_e)),  S_e = sum over the rows routed to e, in the order of order[], of x x^T,
// in ONE launch over (tile, expert) that gathers its rows through the sorted routing of qqq_moe_route.  Part of the single translation unit
// qqq_quant.hip, behind qqq_hessian.hip.h: the tile, the LDS layout, the operand read (hes_operand) and the epilogue's three roundings
// are the dense kernel's, which is what gives every H_e the dense op's bits.  DESIGN.md section 13 argues the choices.
//
//   qqq_hessian_grouped_kernel   one workgroup of four waves per (128 x 128 tile bi <= bj of the upper block triangle, expert e);
//                                E * nb (nb + 1) / 2 of them whatever the routing says.
//     split     the linear order runs through the TILES of one expert first (column by column, as the dense kernel), then to the next
//               expert; workgroup b runs on XCD b % 8 and every XCD takes one contiguous run of that order.  A run is a few whole
//               experts (or, with E < 8, a part of one): the workgroups that gather the same rows of X and read the same stretch of
//               order[] share one L2.  Inside an XCD the hardware hands the run out workgroup by workgroup as CUs come free, which
//               evens out experts of very different lengths; across XCDs the split is by workgroup count, blind to the lengths -- the
//               host does not read them.
//     empty     c_e == 0: the workgroup leaves on its two offsets, before it touches LDS or H.  c_e < 32 is one stage.
//     gather    a stage is 32 positions of order[].  A wave keeps the row indices of 64 positions (two stages), one per lane, from
//               one coalesced load: lane l of chunk k holds order[off + 64 k + l], clamped and divided by a_div into a row of X where
//               the chunk becomes current.  The raw indices of chunk k + 1 are loaded while chunk k is current -- at least one full
//               stage of MFMAs ahead of the first row address they give -- so the chain index -> address -> 16-byte loads costs its
//               latency once, in the prologue.  A thread takes its two rows' indices from the lanes that hold them (ds_bpermute: no
//               memory), then issues the dense kernel's two 16-byte loads per panel.  Positions >= c_e are zero-filled in LDS, never
//               loaded, and their indices never read.
//     staging, operands, waves, epilogue   the dense kernel's, word for word: two LDS buffers, one barrier a stage, ds_read_b64_tr_b16
//               -> v_mfma_f32_32x32x16_f16, the mirrored tile through LDS in the epilogue.  alpha[e] and beta[e] are read from device
//               memory once per workgroup.
#ifndef QQQ_AMD_QQQ_HESSIAN_GROUPED_HIP_H_
#define QQQ_AMD_QQQ_HESSIAN_GROUPED_HIP_H_

#pragma clang fp contract(off)

struct qqq_hessian_grouped_args {
  float* H;
  const _Float16* X;
  const int* offsets;
  const int* order;
  const float* alpha;
  const float* beta;
  long long lde, ldh, ldx;
  int P, R, n, a_div;
  int ntiles;  // nb (nb + 1) / 2 of one expert
  int work;    // E * ntiles (at most 256 * 32896)
};

__global__ __launch_bounds__(HES_NT) void qqq_hessian_grouped_kernel(const qqq_hessian_grouped_args a) {
  __shared__ __attribute__((aligned(16))) _Float16 stage[2][2][HES_TS * HES_LD];  // [buffer][row panel, column panel]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;

  // workgroup b runs on XCD b % 8: every XCD takes one contiguous run of the order (expert, tile of its triangle column by column)
  int e, bi, bj;
  {
    const int q = a.work >> 3, rr = a.work & 7;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int item = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    e = item / a.ntiles;
    fac_tri(item - e * a.ntiles, bi, bj);
  }
  int off = a.offsets[e], end = a.offsets[e + 1];
  off = off < 0 ? 0 : (off > a.P ? a.P : off);
  end = end < off ? off : (end > a.P ? a.P : end);
  const int cnt = end - off;
  if (cnt == 0) return;  // the expert was not chosen: nothing of LDS or H is touched

  const bool diag = bi == bj;
  const int np = diag ? 1 : 2;  // panels to stage

  // the row indices: lane l of chunk k holds position 64 k + l of the expert's stretch of order[]
  const int* ord = a.order + off;
  auto load_idx = [&](const int chunk) {
    const int i = 64 * chunk + lane;
    return i < cnt ? ord[i] : 0;
  };
  auto to_row = [&](int p) {  // a pair index inside [0, P), its row inside [0, R), whatever order[] holds
    p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);
    const int ar = a.a_div == 1 ? p : p / a.a_div;
    return ar >= a.R ? a.R - 1 : ar;
  };

  // staging: thread -> (row r0 and r0 + 16 of the stage, 16-byte chunk ch of the panel's 128 columns)
  const int r0 = tid >> 4, ch = tid & 15;
  const int colA = bi * HES_TILE + 8 * ch, colB = bj * HES_TILE + 8 * ch;
  const bool liveA = colA < a.n, liveB = colB < a.n;  // (n is a multiple of 64: a chunk is inside or outside as a whole)
  hes_u4 regs[2][2];
  auto fetch = [&](const int s, const int rows) {  // stage s: positions 32 s ... 32 s + 31, `rows` the row indices of chunk s / 2
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = r0 + 16 * h;
      const int ar = __shfl(rows, 32 * (s & 1) + r);  // (every lane takes part)
      const bool row = 32 * s + r < cnt;
      const _Float16* xr = a.X + (long long)ar * a.ldx;
      regs[0][h] = row && liveA ? *reinterpret_cast<const hes_u4*>(xr + colA) : hes_u4{0u, 0u, 0u, 0u};
      if (!diag) regs[1][h] = row && liveB ? *reinterpret_cast<const hes_u4*>(xr + colB) : hes_u4{0u, 0u, 0u, 0u};
    }
  };
  auto park = [&](const int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      for (int p = 0; p < np; ++p) *reinterpret_cast<hes_u4*>(&stage[buf][p][(r0 + 16 * h) * HES_LD + 8 * ch]) = regs[p][h];
  };

  hes_f16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;

  const int stages = (cnt + HES_TS - 1) / HES_TS;
  int cur = to_row(load_idx(0));  // chunk 0, the one dependent chain that nothing hides
  int ahead = load_idx(1);        // chunk 1, raw: it becomes current behind stage 1's barrier
  fetch(0, cur);
  park(0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1;
    if (s + 1 < stages) {
      if (s & 1) {  // stage s + 1 opens chunk (s + 1) / 2: its indices came in a stage ago; ask for the chunk behind it
        cur = to_row(ahead);
        ahead = load_idx((s + 1) / 2 + 1);
      }
      fetch(s + 1, cur);
    }
    const _Float16* pa = stage[buf][0];
    const _Float16* pb = stage[buf][diag ? 0 : 1];
#pragma unroll
    for (int k = 0; k < HES_TS; k += 16) {
      hes_h8 fa[2], fb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        fa[u] = hes_operand(pa, k, 64 * wr + 32 * u, lane);
        fb[u] = hes_operand(pb, k, 64 * wc + 32 * u, lane);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[u], fb[v], acc[u][v], 0, 0, 0);
    }
    if (s + 1 < stages) park(buf ^ 1);
    __syncthreads();  // the next stage is in place, and nobody reads this one any more
  }

  // epilogue: the dense kernel's, on expert e's matrix under its own factors.  An accumulator holds, in register r of lane l, row
  // 8 (r / 4) + 4 (l / 32) + r % 4 and column l % 32 of its block; every wave turns its blocks in 32 x 33 floats of the free staging buffers.
  float* He = a.H + (long long)e * a.lde;
  const float alpha = a.alpha[e], beta = a.beta[e];
  float* turn = reinterpret_cast<float*>(&stage[0][0][0]) + w * (32 * HES_TLD);
  const int lc = lane & 31, lh = lane >> 5;
  const bool read_h = alpha != 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i0 = bi * HES_TILE + 64 * wr + 32 * u, j0 = bj * HES_TILE + 64 * wc + 32 * v;  // (a block is inside n or outside as a whole)
      const bool live = i0 < a.n && j0 < a.n;
      if (live) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 8 * (r >> 2) + 4 * lh + (r & 3);
          float* hp = He + (long long)(i0 + i) * a.ldh + j0 + lc;
          const float scaled = beta * acc[u][v][r];
          const float kept = read_h ? alpha * *hp : 0.f;
          const float out = kept + scaled;
          *hp = out;
          if (!diag) turn[i * HES_TLD + lc] = scaled;
        }
      }
      if (!diag) {  // (uniform over the workgroup: the barriers are met by every wave)
        __syncthreads();
        if (live) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = 2 * r + lh;  // row j0 + j of the mirrored block takes column j of the block, along i
            float* hp = He + (long long)(j0 + j) * a.ldh + i0 + lc;
            const float kept = read_h ? alpha * *hp : 0.f;
            *hp = kept + turn[lc * HES_TLD + j];
          }
        }
        __syncthreads();
      }
    }
}

#endif  // QQQ_AMD_QQQ_HESSIAN_GROUPED_HIP_H_
