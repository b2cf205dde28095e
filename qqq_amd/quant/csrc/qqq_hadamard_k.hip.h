// qqq_hadamard_k.hip.h -- the Hadamard transform of matrix rows for blocks of n = K * 2^p columns: the Sylvester stages inside every
// sub-block of m = 2^p entries, then the K x K table that mixes the K sub-blocks (qqq_amd/quant/include_ext/qqq_amd_rotate_k.h states the
// bits).  Part of the single translation unit qqq_quant.hip, after qqq_hadamard.hip.h, whose loads, stores, register butterflies, LDS
// slots, sign flip and divide it uses as they are.
//
//   qqq_hadamard_k_kernel<T, VEC, LOG_TILE>   A workgroup of NT = 2^(LOG_TILE-3) threads owns GROUP whole blocks, numbered row by row
//       through the matrix: as many as fit NT runs at n <= 2048 (256 threads; the blocks may lie in different rows), one at n <= 4096
//       (512 threads) and at n <= 8192 (1024 threads, 72 KB of LDS).  A thread owns one RUN of 8 consecutive elements of that list of
//       blocks from the load to the store; n is a multiple of 8 except at m = 1 with K = 4 (mod 8), where the run is 4 elements and
//       no stage runs at all.  Threads past the group's last run, and the blocks past the matrix's last in the last workgroup, carry
//       zeros and store nothing.
//       The stages h = 1 ... m/2 are those of qqq_hadamard_kernel with log2 m in place of log2 n: sub-blocks start at multiples of
//       m in the group's list, so the same register butterflies and LDS trips apply (with m < 8 a run holds several sub-blocks and the
//       stages below m run in the registers alone).  The group then lies in LDS in its natural order, padded by one double per eight.
//       The mix: the group's n / 4 * GROUP TASKS are (four table rows 4q ... 4q+3, block, column c), c fastest, then the block, at
//       most two per thread.  A task reads its column's K partials v[k' m + c] from LDS, k' ascending, once each, and adds every one
//       into four accumulators under the four rows' signs: z = s(k,0) v[c] first (a flip, no add), then one f64 add per term -- the
//       header's order per output.  A table row is a 64-bit mask of its negative entries, built once per workgroup: the int8 table
//       is copied into LDS by all threads (K dependent byte loads from global memory by one thread per row cost more than the whole
//       mix at K = 40), and the first K threads pack their rows from it.  The flip of a term (shift, mask, shift, xor) costs four
//       vector instructions beside the add.  Where GROUP * m is a multiple of 64 (and m of 8: every shipped hidden size) the tasks of
//       a wave share q, so the masks are read into scalar registers and a term is ONE instruction, fma(v, +-1.0, z) with the
//       +-1.0 formed by scalar instructions: the product is exact and the fma rounds z +- v once, the bits of the flip and the add.
//       All tasks have read before any output is written (one barrier): the outputs replace the partials in place, and the threads
//       read their runs back, divide and store.
#ifndef QQQ_AMD_QQQ_HADAMARD_K_HIP_H_
#define QQQ_AMD_QQQ_HADAMARD_K_HIP_H_

#include "qqq_hadamard.hip.h"

#pragma clang fp contract(off)

static constexpr int HAD_K_MAX = 64;

struct qqq_hadamard_k_args {
  const void* X;
  void* Y;
  const signed char* sign;   // NULL: all +1
  const signed char* table;  // [K, K]
  long long ldx, ldy;
  long long blocks;          // blocks in the matrix: rows * blocks_per_row
  int blocks_per_row;        // cols / n
  int group;                 // blocks a workgroup owns
  int run;                   // 8, or 4 where n % 8 == 4 (m = 1 then)
  int n, K, m, log2m;
  int uniform;               // the 64 tasks of every wave share their table rows: m % 8 == 0 and group * m % 64 == 0
  double d;                  // (double)sqrtf((float)n)
  double rd;                 // 1 / d, correctly rounded (the host's divide)
};

// the padded LDS index of element idx of the group's list
__device__ __forceinline__ int had_pad(const int idx) { return idx + (idx >> 3); }

template <typename T, bool VEC, int LOG_TILE>
__global__ __launch_bounds__(1 << (LOG_TILE - 3)) void qqq_hadamard_k_kernel(const qqq_hadamard_k_args a) {
  constexpr int NT = 1 << (LOG_TILE - 3);
  __shared__ double tile[NT * (HAD_RUN + 1)];
  __shared__ unsigned long long rowmask[HAD_K_MAX];
  __shared__ unsigned int tab[HAD_K_MAX * HAD_K_MAX / 4];
  const int t = threadIdx.x;
  // the table's K * K bytes come in spread over the workgroup, so that the loads are in flight together (and with the matrix's)
  for (int e = t; e < a.K * a.K; e += NT) reinterpret_cast<signed char*>(tab)[e] = a.table[e];
  const int p = t * a.run;  // where the run starts in the group's list
  const int g = p / a.n;
  const int within = p - g * a.n;
  const long long blk = static_cast<long long>(blockIdx.x) * a.group + g;
  const bool live = g < a.group && blk < a.blocks;
  double v[HAD_RUN];
  T* yp = nullptr;
  if (live) {
    const long long row = blk / a.blocks_per_row;
    const long long col = (blk - row * a.blocks_per_row) * a.n + within;
    had_load<VEC>(static_cast<const T*>(a.X) + row * a.ldx + col, a.run, v);
    yp = static_cast<T*>(a.Y) + row * a.ldy + col;
    if (a.sign) {
      const signed char* s = a.sign + within;
      if (VEC) {  // the run's eight entries in one load (the host takes VEC only with an 8-byte aligned sign and runs of 8)
        const had_u2 w = *reinterpret_cast<const had_u2*>(s);
#pragma unroll
        for (int j = 0; j < HAD_RUN; ++j) v[j] = had_signed(v[j], (j < 4 ? w.x : w.y) >> (8 * (j & 3) + 7));
      } else {
#pragma unroll
        for (int j = 0; j < HAD_RUN; ++j)
          if (j < a.run) v[j] = had_signed(v[j], s[j] < 0);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = 0.0;
  }
  // h = 1, 2, 4 (those below m)
  if (a.log2m > 0) had_stage<0>(v);
  if (a.log2m > 1) had_stage<1>(v);
  if (a.log2m > 2) had_stage<2>(v);
  __syncthreads();
  if (t < a.K) {  // bit k' of row t: table[t][k'] is negative; four entries per word (K is a multiple of 4: a row starts a word)
    unsigned long long bits = 0;
    for (int w = 0; w < a.K >> 2; ++w) {
      const unsigned x = tab[t * (a.K >> 2) + w];
      bits |= static_cast<unsigned long long>(((x >> 7) & 1u) | ((x >> 14) & 2u) | ((x >> 21) & 4u) | ((x >> 28) & 8u)) << (4 * w);
    }
    rowmask[t] = bits;  // read after the next barrier
  }
  int base = 0;  // the list-index bits the register index holds now
  for (int done = 3; done < a.log2m; done += 3) {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) tile[had_slot(t, j, base)] = v[j];
    __syncthreads();
    base = done < LOG_TILE - 3 ? done : LOG_TILE - 3;
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = tile[had_slot(t, j, base)];
    __syncthreads();
    if (base + 0 >= done && base + 0 < a.log2m) had_stage<0>(v);
    if (base + 1 >= done && base + 1 < a.log2m) had_stage<1>(v);
    if (base + 2 >= done && base + 2 < a.log2m) had_stage<2>(v);
  }
  // the group in its natural order
  if (a.run == HAD_RUN) {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) tile[had_slot(t, j, base)] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN / 2; ++j) tile[had_pad(p + j)] = v[j];
  }
  __syncthreads();
  // the mix: at most two tasks of four outputs each per thread
  const int quads = a.K >> 2;
  const int tasks = a.group * quads * a.m;
  double z[2][4];
  int at[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int task = t + s * NT;
    at[s] = -1;
    if (task < tasks) {
      const int c = task & (a.m - 1);
      const int rest = task >> a.log2m;
      const int qv = rest / a.group;
      const int p0 = (rest - qv * a.group) * a.n + c;
      if (a.uniform) {
        // the 64 tasks of a wave share their four table rows: the signs live in scalar registers as +-1.0, and a term is one fma,
        // fma(x, +-1, z) = RN(z +- x): the bits of the flip and the add, zeros included
        const int q = __builtin_amdgcn_readfirstlane(qv);
        unsigned lo[4], hi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned long long w = rowmask[4 * q + r];
          lo[r] = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(w));
          hi[r] = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(w >> 32));
        }
        const int first = had_pad(p0), stride = a.m + (a.m >> 3);  // m is a multiple of 8: the padding moves in step
        // z starts as -0: fma(x, +-1, -0) = +-x for every x, zeros included, so the first term is the flip alone.  Four partials
        // are read ahead of their sixteen fmas (K is a multiple of 4): the LDS latency is paid once per four terms
#pragma unroll
        for (int r = 0; r < 4; ++r) z[s][r] = -0.0;
        for (int k = 0; k < a.K; k += 4) {
          double x[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = tile[first + (k + j) * stride];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const unsigned bit = ((k < 32 ? lo[r] : hi[r]) >> ((k & 31) + j)) & 1u;
              z[s][r] = __builtin_fma(x[j], __longlong_as_double(0x3ff0000000000000LL | (static_cast<long long>(bit) << 63)), z[s][r]);
            }
          }
        }
      } else {
        unsigned long long mk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mk[r] = rowmask[4 * qv + r];
        double x = tile[had_pad(p0)];
#pragma unroll
        for (int r = 0; r < 4; ++r) z[s][r] = had_signed(x, static_cast<unsigned>(mk[r]));
        for (int k = 1; k < a.K; ++k) {
          x = tile[had_pad(p0 + k * a.m)];
#pragma unroll
          for (int r = 0; r < 4; ++r) z[s][r] = z[s][r] + had_signed(x, static_cast<unsigned>(mk[r] >> k));
        }
      }
      at[s] = p0 + 4 * qv * a.m;
    }
  }
  __syncthreads();  // every partial has been read: the outputs take their places
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (at[s] >= 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[had_pad(at[s] + r * a.m)] = z[s][r];
    }
  __syncthreads();
  if (live) {
    float y[HAD_RUN];
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) y[j] = j < a.run ? static_cast<float>(had_div(tile[had_pad(p + j)], a.d, a.rd)) : 0.0f;
    had_store<VEC>(yp, a.run, y);
  }
}

#endif  // QQQ_AMD_QQQ_HADAMARD_K_HIP_H_
