// qqq_plan.h -- the dispatch planner of qqq_w4a8_gemm: which kernel family, tile shape and K split a call runs with.
// Pure host arithmetic over the problem size, the CU count and the scratch the caller gave: no HIP call, no HIP header -- it compiles on its
// own with the host compiler (tests/test_abi_cpu.py holds it to that), so a planner change can be tried without building a kernel.
// qqq_w4a8.hip includes it and wraps it in the C-ABI (qqq_w4a8_plan, qqq_w4a8_model_us, qqq_w4a8_gemm_ex2); every rate comes from qqq_rates.h.
#ifndef QQQ_AMD_QQQ_PLAN_H_
#define QQQ_AMD_QQQ_PLAN_H_

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qqq_amd.h"
#include "qqq_rates.h"

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The scratch a split K may use.  The reference guarantees max_par * 64 rows of C (int32, N wide) and N / 128 * max_par zeroed ints of workspace
// (include/qqq_amd.h); a call may come without either.
struct ScratchRoom {
  bool slabs;             // C is there and has rows: K slices as [m, n] slabs + a reduce launch (stream, column, tiled)
  bool have;              // ... and the workspace as well: the in-launch hand-offs (tickets in the workspace, deposits in C)
  long long cap_rows;     // rows of C we may use
  long long cap_tickets;  // ints of workspace we may use (0 without one)
  long long N;
  static ScratchRoom of(int max_par, bool have_C, bool have_ws, int N) {
    ScratchRoom r;
    r.cap_rows = (long long)(max_par > 0 ? max_par : 0) * 64;
    r.cap_tickets = have_ws ? (long long)(N / 128) * (max_par > 0 ? max_par : 0) : 0;
    r.slabs = have_C && r.cap_rows > 0;
    r.have = r.slabs && have_ws;
    r.N = N;
    return r;
  }
  // panel / wide: `ks` K slices of `tiles` tiles of rows x bn -- two ticket words per tile, one slot of rows x bn ints per tile and depositing
  // slice, all inside C (bn-wide strips may overhang N)
  bool fits(long long tiles, int rows, int bn, int ks) const {
    return have && 2 * tiles <= cap_tickets && tiles * rows * bn * (ks - 1) <= cap_rows * N;
  }
};

// What one call is planned for.  `cus`: the CUs the call may use -- qqq_w4a8_gemm_ex2 passes the count of the device it was given, capped by the
// reference's `sms` argument, and launches with the same number, so the plan and the launch grid can never disagree (the cost models' rounds of
// workgroups, the K splits that fill one round and the tile walk's grid all read it); qqq_w4a8_plan plans for the MI355X's 256.
struct PlanCtx {
  int M, N, K;
  bool grouped;
  int cus;
  ScratchRoom room;
};
static PlanCtx plan_ctx(int M, int N, int K, bool grouped, int cus, int max_par, bool have_C, bool have_ws) {
  return PlanCtx{M, N, K, grouped, cus > 0 ? cus : 256, ScratchRoom::of(max_par, have_C, have_ws, N)};
}

// tiled, in-launch split K: the tile-sized slots of C (rows x 256 ints) that `ks` slices can meet in -- at most ks - 1, one ticket per tile and slot
static int slot_count(const PlanCtx& c, int rows, int ks, bool slabs_only) {
  if (!c.room.slabs || ks < 2 || slabs_only) return 0;
  const long long tl = (long long)((c.M + rows - 1) / rows) * ((c.N + 255) / 256);
  long long S = c.room.cap_rows * c.room.N / (tl * rows * 256);
  if (S > ks - 1) S = ks - 1;
  while (S > 0 && tl * (1 + S) > c.room.cap_tickets) --S;
  return (int)S;
}

// ---- cost models (microseconds) used by the automatic dispatch; constants fitted to profiles/r02_dispatch_check*.txt ----
// tiled: rounds(tiles x ksplit over 256 CUs) x tile_time(rows, K / ksplit, rate(shape)) + split-K cost,
// per-shape rates (TOPS at large m) measured on MI355X.  Bigger tiles are more efficient per MFMA but quantise worse
// over the CUs; split-K fills idle CUs at the price of int32 partial-sum traffic.  Wave shapes per mode: per-channel
// keeps 64x128 wave tiles (least LDS traffic); per-group uses the column-owner shapes (258 / 130): every weight
// re-quantised once per workgroup.
static double tiled_estimate(const PlanCtx& c, bool slabs_only, int* bm_out, int* ks_out) {
  const int M = c.M, N = c.N, K = c.K;
  const bool grouped = c.grouped, have_scratch = c.room.slabs;
  const long long strips = (N + 255) / 256, cap_rows = c.room.cap_rows;
  // {several workgroups co-resident per CU, a single one} -- small tiles lose efficiency when alone on a CU
  const double rate256 = grouped ? 1950.0 : 2500.0;
  const double rate128[2] = {grouped ? 1360.0 : 2050.0, grouped ? 1320.0 : 1650.0};
  const double rate64[2] = {grouped ? 800.0 : 1560.0, grouped ? 650.0 : 1170.0};
  double best = 1e30;
  auto consider = [&](int rows, const double* rates, int code) {
    const long long tl = (long long)((M + rows - 1) / rows) * strips;
    const int ks_max = (tl < 192 && have_scratch) ? clampi((int)((256 + tl - 1) / tl), 1, (K / 128) / 4 > 0 ? (K / 128) / 4 : 1) : 1;
    for (int ks = 1; ks <= ks_max; ++ks) {
      const int S = slot_count(c, rows, ks, slabs_only);
      if (ks > 1 && S == 0 && (long long)ks * M > cap_rows) break;
      const double rate = (rows == 256) ? rates[0] : rates[(tl * ks <= 256) ? 1 : 0];
      const double tile_us = (double)rows * ((double)K / ks) * 131072.0 / (rate * 1e6) + 6.0;  // + prologue/epilogue
      double us = (double)((tl * ks + 255) / 256) * tile_us;
      if (ks > 1 && S > 0)  // every deposit is written once and read once (~4.2 TB/s chip-wide) + serial hops
        us += 3.0 + 2.0 * (ks - 1) * (double)tl * rows * 1024.0 / 4.2e6 + 3.0 * (double)((ks - 1 + S - 1) / S);
      else if (ks > 1) us += 5.0 + (double)ks * M * N * 8.0 / 3.0e6;  // slabs written + read at ~3 TB/s, + launch
      if (us < best) {
        best = us;
        *bm_out = code;
        *ks_out = ks;
      }
    }
  };
  consider(256, &rate256, grouped ? 258 : 256);
  consider(128, rate128, grouped ? 130 : 131);
  consider(64, rate64, 64);
  return best;
}

// 1 ... 32 tokens: the column kernel (one launch; every 32-column workgroup re-reads the m x K activations) against the stream kernel (K slices + reduce launch).
// Both are linear forms whose coefficients are GENERATED (qqq_rates.h, kQqqSmall; tools/fit_rates.py: least squares over the forced column / stream measurements of ten
// dispatch grids, 3 - 4 % mean error per form -- round 5's last re-measurement, taken with enough rotating weight copies that the Infinity Cache serves nobody):
//   column, per-channel: launch + the weights (c1 per MB) + the activations every workgroup reads again (c2 per 1e6 bytes, per round of 256 workgroups) + the serial depth
//   of a chip that is not full (c3 per 1000 k, scaled by the share of idle CUs: N = 3584, K = 18944 at decode 16.2 us where the bytes alone say 10.7);
//   per-group: bound by the re-quantiser -- g1 per 1000 k per round, flat up to 16 tokens, g2 for the second 16-token tile (growing as ((m - 16) / 16)^0.75) -- + the weights;
//   stream: a + b weight passes at 5 TB/s up to 16 tokens, a + c (m - 24) / 16 + b passes from 17; per mode.
static double column_small_estimate(const PlanCtx& c0) {
  const int M = c0.M, N = c0.N, K = c0.K, cus = c0.cus;  // (CUs of THIS call: the device's, or the `sms` cap)
  const bool grouped = c0.grouped;
  const int wgs = N / 32, rounds = (wgs + cus - 1) / cus;
  const double mb = (double)N * K / 2.0e6;
  if (!grouped) {
    const double* c = kQqqSmall.col_pc;
    const double idle = wgs < cus ? 1.0 - wgs / (double)cus : 0.0;
    return c[0] + c[1] * mb + c[2] * 1e-6 * (double)K * M * rounds + c[3] * 1e-3 * K * idle;
  }
  const double* g = kQqqSmall.col_g;
  const double r = rounds == 1 ? 1.0 : 0.92 * rounds;
  double us = g[0] + g[1] * 1e-3 * K * r + g[3] * mb;
  if (M > 16) us += g[2] * 1e-3 * K * r * pow((M - 16) / 16.0, 0.75);
  return us;
}
// stream, tune.ksplit = 0 up to 64 tokens: one workgroup per CU -- (strips x m-blocks = `base`) x K slices ~ the CUs, at least 2 steps of 64 k per wave
static int stream_auto_ksplit(int cus, long long base, bool one_tile, int KS, int waves) {
  int ks = (int)((cus + base / 2) / base);
  // a 257th workgroup is a second round (n = 11008: 86 strips x 3 slices) -- for the 4-wave bodies of <= 16 tokens as well (N = 7168, K = 20480:
  // 56 strips x 5 slices 25.5 us, x 4 slices 18.9; profiles/r04_stream_ksplit_wide_n.txt)
  if (ks > 1 && base * ks > cus) --ks;
  // up to 16 tokens (one 16-token tile, 4-wave bodies): 128 workgroups or more already pull the weights at the HBM's pace, a second K slice only adds the reduce
  // launch (N = 18944, K = 3584 at 16 tokens: 10.9 us unsplit, 14.9 in two slices; N = 16384, K = 4096: 11.5 / 12.7; profiles/r04_stream_ksplit_wide_n.txt)
  if (one_tile && base >= 128) ks = 1;
  return clampi(ks, 1, KS / (2 * waves) > 0 ? KS / (2 * waves) : 1);
}
static double stream_small_estimate(const PlanCtx& c) {
  const int M = c.M, N = c.N, K = c.K;
  const bool grouped = c.grouped;
  const double pb = (double)N * K / 2.0 / 5.0e6;
  const int gi = grouped ? 1 : 0;
  const double us = M <= 16 ? kQqqSmall.st16[gi][0] + kQqqSmall.st16[gi][1] * pb
                            : kQqqSmall.st32[gi][0] + kQqqSmall.st32[gi][1] * (M - 24) / 16.0 + kQqqSmall.st32[gi][2] * pb;
  if (!grouped) return us;
  // per-group a slice is also bound by its re-quantiser: 9.7 us + 2.1 us per 1000 k of the slice -- what a wide layer's unsplit strips pay
  // (N = 20480, K = 7168: 24.9 us against the column kernel's 21.1; profiles/r04_stream_ksplit_wide_n.txt).  The K split as make_plan picks it
  // (one 16-token tile and 4 waves up to 16 tokens, 32-token m-blocks and 8 waves above):
  const long long base = (long long)((N + 127) / 128) * (M <= 16 ? 1 : (M + 31) / 32);
  const int ks = stream_auto_ksplit(c.cus, base, M <= 16, K / 64, M <= 16 ? 4 : 8);
  const double requant = 9.7 + 2.1e-3 * (double)K / ks;
  return us > requant ? us : requant;
}

// stream, 65 ... 256 tokens (two to four 64-token m-blocks) on layers up to ~40 MB: the loop, not the weight stream, sets the time: a + b per 64-k step of a slice, per
// round of 256 workgroups (x 1.2 from the second round on), + for a K split the slabs and the reduce launch (s0 + s1 per MB of int32 slabs); one set of rates per mode,
// GENERATED (qqq_rates.h, kQqqSmall.stmid: 137 points per mode, 3 - 4 % mean error; round 4's hand fit -- 8.65 us + 0.153 per step, x 1.235 per-group, 2 + 0.4 per MB --
// read 4 - 8 % low on the cold re-measurement).  Returns the time and the split it is reached with -- "fill 256 workgroups" (the rule for <= 64 tokens) splits
// short-K layers that are better left whole (N = 8192, K = 3072 at 128 tokens: 19.4 us in two slices, 15.7 unsplit).
static double stream_mid_estimate(const PlanCtx& c0, int ks_cap, int* ks_out) {
  const int M = c0.M, N = c0.N, K = c0.K, cus = c0.cus;
  const bool grouped = c0.grouped;
  const long long base = (long long)((N + 127) / 128) * ((M + 63) / 64);
  const int KS = K / 64;
  // The SPLIT is chosen by round 4's hand-fitted rates (right at 44 of its 48 points), the PRICE of that split comes from the generated ones: the forced stream
  // kernel's plan then does not depend on the table, so the tool that fits the table from measurements of that plan reaches a fixed point in one pass.
  double best_rule = 1e30, price = 1e30;
  *ks_out = 1;
  const double* c = kQqqSmall.stmid[grouped ? 1 : 0];
  for (int ks = 1; ks <= 8 && ks <= ks_cap; ++ks) {
    if (ks > 1 && KS / ks < 8) break;  // (8-wave bodies: at least a step per wave)
    const double rounds = (double)((base * ks + cus - 1) / cus);
    const double steps = rounds * (rounds > 1.0 ? 1.2 : 1.0) * KS / ks, slab_mb = (double)M * N * 4.0 * ks / 1.0e6;
    const double rule = 8.65 + 0.153 * (grouped ? 1.235 : 1.0) * steps + (ks > 1 ? 2.0 + 0.4 * slab_mb : 0.0);
    if (rule < best_rule) {
      best_rule = rule;
      price = c[0] + c[1] * steps + (ks > 1 ? c[2] + c[3] * slab_mb : 0.0);
      *ks_out = ks;
    }
  }
  return price;
}

// stream: every 64-token m-block streams the whole weight matrix (the first from HBM, the others mostly from L2 /
// Infinity Cache), plus launch, LDS reduce and the separate split-K reduce launch
static double stream_estimate(const PlanCtx& c) {
  const int M = c.M, N = c.N, K = c.K;
  const bool grouped = c.grouped;
  double per_block = (double)N * K / 2.0 / 5.0e6;  // the weight matrix at ~5 TB/s
  if (per_block < 2.5) per_block = 2.5;
  const int mblocks = (M + 63) / 64;
  if (mblocks >= 2 && mblocks <= 4 && (double)N * K / 2.0 / 5.0e6 < 8.0) {
    // (only splits the plan can realise: slabs need C, and ksplit x M rows of it)
    int ks, ks_cap = c.room.slabs ? (int)(c.room.cap_rows / M < 8 ? c.room.cap_rows / M : 8) : 1;
    return stream_mid_estimate(c, ks_cap < 1 ? 1 : ks_cap, &ks);
  }
  // measured: 2 / 3 / 4 m-blocks take 1.85 / 3.2 / 3.3 weight passes
  // (one m-block: 16 / 32 / 48 / 64 tokens measured at 0.6 / 0.8 / 1.0 / 1.2 -- the 16-token tiles of a block share the weights
  //  in registers but not the MFMA / VALU time)
  const double passes = (mblocks == 1) ? 0.4 + 0.0125 * M : (mblocks == 2) ? 1.85 : (mblocks == 3) ? 3.2 : 3.3 + 0.8 * (mblocks - 4);
  // fixed part: 2 and 3 m-blocks in one round of workgroups measured at 10.6 (3 blocks: 18.0 / 25.0 / 68 us at 1.7 / 4.5 / 17.8 us
  // per pass; 2 blocks: 16.3 / 18.9 / 43.5; profiles/r02_dispatch_check_handoff.txt); more than 256 workgroups even unsplit
  // (n = 11008: 86 strips x 3) is a second round
  double us = ((mblocks == 2 || mblocks == 3) ? 10.6 : 9.0 + 2.0 * mblocks) + per_block * passes;
  if ((long long)((N + 127) / 128) * mblocks > c.cus) us *= 1.35;
  if (mblocks == 1 && M > 32) {
    // 33 ... 64 tokens: per token count a line in the weight bytes (no floor: the 8 MB layers sit ON the line), with a step where the fourth 16-token tile
    // starts (49 tokens); one form per mode, coefficients generated (qqq_rates.h, kQqqSmall.st64: 68 points per mode, 3 % mean error)
    const double pb = (double)N * K / 2.0 / 5.0e6;
    const double four = M > 48 ? 1.0 : 0.0;
    const double* f = kQqqSmall.st64[grouped ? 1 : 0];
    return f[0] + f[1] * M + f[2] * four + pb * (f[3] + f[4] * M + f[5] * four);
  }
  return grouped ? us * 1.15 : us;
}

// panel: all tokens of an m-block (16 ... 128) x bn-column strips x K slices.  Priced from the GENERATED table qqq_rates.h (tools/fit_rates.py: one
// linear form per (strip shape, m-block, mode), least squares over every forced panel variant of profiles/r05_dispatch_check_*.txt -- 2600 measurements, 2 ... 5 % mean
// error per group): us = rounds x (a + c [split] + d (slices - 2) + b x stages per workgroup).  Round 5 replaced the hand-fitted constants of rounds 2 - 4 here (they
// were 10 ... 35 % high once the uneven K slices had shortened the hand-off).
static double panel_estimate(const PlanCtx& c, int* bn_out, int* ks_out, int* cw_out, int* mt_out = nullptr) {
  const int M = c.M, N = c.N, K = c.K, cus = c.cus;
  const bool grouped = c.grouped;
  if (mt_out) *mt_out = 0;  // 0: the m-block the token count implies (16 / 32 / 64 / 128 rows)
  const int mt = (M <= 16) ? 1 : (M <= 32) ? 2 : (M <= 64) ? 4 : 8;
  const int mti = mt == 1 ? 0 : mt == 2 ? 1 : mt == 4 ? 2 : 3;
  const int rows = 16 * mt;
  const long long mblocks = (M + rows - 1) / rows;
  const int NST = (K / 64 + 1) / 2;
  double best = 1e30;
  for (int shape = 0; shape < 3; ++shape) {  // 128-column strips; 256-column strips; 256-column strips with 64 columns per wave (128-token m-blocks)
    if (shape == 2 && mt != 8) continue;
    const int bn = shape == 0 ? 128 : 256;
    const QqqPanelRate& r = kQqqPanelRates[shape][mti][grouped ? 1 : 0];
    if (r.b <= 0.0) continue;
    const long long tl = mblocks * ((N + bn - 1) / bn);
    for (int ks = 1; ks <= 4; ++ks) {
      if (ks > 1 && (!c.room.fits(tl, rows, bn, ks) || ks > NST / 4)) break;
      const double rounds = (double)((tl * ks + cus - 1) / cus);
      const double us = rounds * (r.a + (ks > 1 ? r.c : 0.0) + (ks > 2 ? r.d * (ks - 2) : 0.0) + r.b * (double)NST / ks);
      if (us < best) {
        best = us;
        *bn_out = bn;
        *ks_out = ks;
        *cw_out = shape == 2 ? 2 : 1;
      }
    }
  }
  // More than 64 tokens as SEVERAL 64-token m-blocks (round 5, profiles/r05_panel_feeder.txt): on layers whose 128-token tiles leave CUs idle or hold few
  // stages each, twice the workgroups of half the size finish sooner although every m-block streams the weights again (from L2 / the Infinity Cache) --
  // 4096 x 4096 at 128 / 256 / 512 tokens 13.1 / 15.2 / 18.4 us against 15.2 / 17.7 / 19.4, 4096 x 11008 and 11008 x 4096 at 128 tokens 18.3 / 18.5 against
  // 21.5 / 20.0, 8192 x 8192 21.3 against 22.1; not on the BASELINE layer (40.1 vs 35.4: the weights come from HBM twice) and not beyond one round of
  // workgroups (11008 x 4096 at 256 tokens 27.7 vs 23.3).  Priced with the 64-token form above; one round only.
  // (the form holds on narrow layers as well: 74 single-round points with N < 4096 in profiles/r05_dispatch_check_*.txt, mean error 3.9 %)
  if (mt == 8 && mt_out) {
    const long long mb4 = (M + 63) / 64, tl = mb4 * ((N + 127) / 128);
    for (int ks = 1; ks <= 4; ++ks) {
      if (tl * ks > cus) break;
      if (ks > 1 && (!c.room.fits(tl, 64, 128, ks) || ks > NST / 4)) break;
      // (rates GENERATED -- qqq_rates.h, kQqqSmall.panel64, tools/fit_rates.py: the single-round points of the column panel64 in profiles/r05_dispatch_check_*.txt,
      //  165 per mode, 2.5 - 2.7 % mean error: launch + fill + epilogue unsplit / split, us per stage, every further m-block a share of a weight pass at bw MB/us)
      const double* q = kQqqSmall.panel64[grouped ? 1 : 0];
      const double stage_us = ((double)NST / ks) * q[2];
      const double bytes_us = (1.0 + q[3] * (double)(mb4 - 1)) * ((double)N * K / 2.0e6) / q[4];
      const double us = (ks == 1 ? q[0] : q[1]) + (stage_us > bytes_us ? stage_us : bytes_us);
      if (us < best) {
        best = us;
        *bn_out = 128;
        *ks_out = ks;
        *cw_out = 1;
        *mt_out = 4;
      }
    }
  }
  return best;
}

// wide: three tile shapes, one tile per CU and round.  Fitted on one box after the LDS-DMA staging
// (profiles/r03_dispatch_check_wide3.txt): time = 3.7 + rounds * (fixed + hand-off + stages * t_stage * load), with
//   256 x 256 (mt 16, bn 256): fixed 12 us (first operands from HBM with every CU in its prologue at once ~4, epilogue ~7),
//                              1.25 us per 128-k stage (per-group 1.635: the re-quantiser of a lone wave is issue-bound);
//   256 x 128 (mt 16, bn 128): fixed 7, 0.70 (0.96) per stage: a weight operand still feeds 256 tokens, twice the LDS traffic
//                              per MFMA -- the shape that fills the chip from ~600 tokens, and per-group on 4096-wide layers;
//   128 x 256 (mt 8,  bn 256): fixed 7, 0.725 (1.17): twice the unpack / re-quantise work per MFMA.  (Round 4, cold A/B on six layer shapes at
//                              640 ... 2048 tokens, profiles/r04_wide_w8_vs_w128.txt: 256 x 128 is 1 ... 4.5 % ahead of 128 x 256 per-channel wherever the
//                              tile counts do not decide -- 0.72 / 0.71 had it the other way round.)
// Two K slices (256-token tiles): hand-off 15 us per 256 KiB of partial tile (kept in the XCD's L2 when its slices share one -- round 4 --,
// folded by the last arrival; 20 us written through).
// (w8: the call has the expanded int8 weights.  The loop is then the per-channel loop minus its unpack, with two more 16-byte
//  loads per step: priced like a per-channel call (load rule) with rates of its own -- the third column of kQqqWideRates, fitted from profiles/r06_w8_dispatch_check_main.txt.)
static double wide_estimate(const PlanCtx& c, int* ks_out, int* mt_out, int* bn_out, bool w8 = false) {
  const int M = c.M, N = c.N, K = c.K, cus = c.cus;
  bool grouped = c.grouped;
  *ks_out = 1;
  *mt_out = 16;
  *bn_out = 256;
  if ((long long)N * K / (w8 ? 1 : 2) >= (1ll << 32) || (K % 128) != 0) return 1e30;  // 32-bit offsets into the weights; whole stages
  if (w8) grouped = false;
  const int NST = K / 128;
  double best = 1e30;
  for (int shape = 0; shape < 3; ++shape) {
    const int mt = shape == 2 ? 8 : 16, bn = shape == 1 ? 128 : 256;
    const int rows = 16 * mt;
    const long long tl = (long long)((M + rows - 1) / rows) * ((N + bn - 1) / bn);
    // (round 5: fixed / t_stage / hand-off per shape and mode from the GENERATED table qqq_rates.h -- tools/fit_rates.py, least squares over every forced wide variant of
    //  profiles/r05_dispatch_check_*.txt, 2.3 ... 3.9 % mean error per group; the hand-fitted values above -- 12 / 7 us, 1.25 / 0.70 / 0.725 us per stage, 15 us per
    //  256 KiB -- are the history: the uneven K slices took the hand-off to 11-12.6)
    const QqqWideRate& wr = kQqqWideRates[shape][w8 ? 2 : grouped ? 1 : 0];  // (round 6: calls that have expanded weights are priced from a fit of their own)
    const double t_stage = wr.t_stage;
    const double fixed = wr.fixed;
    for (int ks = 1; ks <= (mt == 16 ? 2 : 1); ++ks) {
      if (ks > 1 && (!c.room.fits(tl, rows, bn, ks) || ks > NST / 4)) break;
      // rounds: workgroups of later rounds start as CUs free up, but the XCDs' queues drain unevenly -- close to the ceiling of
      // the ratio (288-344 tiles measured 1.7-1.8 rounds, 688 tiles 2.8-3).  A partly filled single round runs each tile
      // faster: the part is power-limited (half the CUs busy: 0.8 of the full-chip stage time, 0.85 per-group; then quadratic)
      const double x = (double)(tl * ks) / (double)cus;
      const double cx = (double)((tl * ks + cus - 1) / cus);
      const double rounds = x <= 1.0 ? 1.0 : cx - 0.3 * (cx - x);
      const double lo = grouped ? 0.85 : 0.80, rel = x <= 0.5 ? 0.0 : (x - 0.5) / 0.5;
      const double load = x <= 1.0 ? lo + (1.0 - lo) * rel * rel : 1.0;
      // (15 us per 256 KiB of partial tile since the deposits stay in the XCD's L2, 20-23 written through: profiles/r04_wide_xcd_local_deposits.txt)
      const double handoff = ks > 1 ? wr.handoff * (double)(rows * bn) / 65536.0 : 0.0;
      const double us = 3.7 + rounds * (fixed + handoff + ((double)NST / ks) * t_stage * load);
      if (us < best) {
        best = us;
        *ks_out = ks;
        *mt_out = mt;
        *bn_out = bn;
      }
    }
  }
  return best;
}

// panel, split K: stages the last slice gets on top of an even share (tune.skew = 0).  Measured (profiles/r05_uneven_k_slices.txt: N = 8192, K = 21760 at
// 64 / 128 / 256 tokens, both modes, and 4096 x 4096 at 128 / 256): the best skew makes the last slice's extra loop time -- skew stages, plus the
// skew / (ks - 1) stages every other slice is shorter by -- about the latency of a deposit (write-through drain + publish: ~1.6 us, + ~1.2 us per
// 64 KiB of partial tile): 4 stages at 128 tokens (37.3 -> 36.1 us; per-group 3: 45.5 -> 43.4), 3 in two slices (256 tokens: 56.9 -> 54.4).  Less than
// that is slower than even slices (the last slice arrives last but still waits), more only lengthens the longest slice.
static int panel_auto_skew(int mt, int bn, bool grouped, int ksplit) {
  const double t_stage = ((mt == 8 && bn == 128) ? 0.506 : 0.13 + 0.042 * mt) * (bn == 256 ? 1.9 : 1.0) * (grouped ? (mt == 8 ? 1.45 : 1.6) : 1.0);
  const double latency = 1.6 + 1.2 * (16.0 * mt * bn) / 16384.0;
  const int sk = (int)(latency / (t_stage * ksplit / (ksplit - 1.0)) + 0.5);
  return sk < 1 ? 1 : sk;
}
// stream, split K through arrival-order slots (tune.fused = 3): the skew of the slot protocol, in 64-k steps: the slices stream the matrix together in about N K / 2 / 5 TB/s, a deposit (8 ... 32 KiB written
// through, drained, counted) takes ~2 us
static int stream_auto_skew(int N, int K, int ksplit) {
  const double pass_us = (double)N * K / 2.0 / 5.0e6;
  const double t_step = pass_us * ksplit / (K / 64.0);
  const int sk = (int)(2.0 / (t_step * ksplit / (ksplit - 1.0)) + 0.5);
  return sk < 1 ? 1 : sk;
}
// wide, split K: the same rule with the wide kernel's deposits (a 256 x 256 partial tile goes through the LDS transposition and out as 256 KiB of
// row-major int32: ~20 us from the depositor's last MFMA to "complete", half of that for the 128-column tiles) and stage times (wide_estimate).
// Measured (profiles/r05_uneven_k_slices_wide.txt): N = 8192, K = 21760 per-group at 1024 tokens 173.1 -> 165.9 us (skew 6; 4: 167.6, 8: 167.0), per-channel
// two slices of 256 x 256 140.3 -> 133.2 (8); 256 x 128 tiles in two slices at 384 / 512 tokens 80.8 -> 76.4 / 85.6 -> 82.2 (6), per-group 512: 102.8 -> 98.6 (3-6);
// Llama-2-7B down_proj (4096 x 11008) at 1024 tokens 50.1 -> 48.6, per-group 62.3 -> 58.1 (3).
static int wide_auto_skew(int mt, int bn, bool grouped, int ksplit, bool w8 = false) {
  if (w8) grouped = false;
  const double t_stage = kQqqWideRates[(mt == 16 && bn == 256) ? 0 : (mt == 16) ? 1 : 2][w8 ? 2 : grouped ? 1 : 0].t_stage;
  const double latency = 20.0 * (16.0 * mt * bn) / 65536.0;
  const int sk = (int)(latency / (t_stage * ksplit / (ksplit - 1.0)) + 0.5);
  return sk < 1 ? 1 : sk;
}

// wide: the persistent tile walk needs whole tiles (no K split), a K range longer than its prefetch leads and at least one tile per
// workgroup of its grid (a multiple of 8: workgroup b lands on XCD b % 8)
static bool wide_chain_ok(const PlanCtx& c, long long tiles, int ksplit) {
  return ksplit == 1 && c.K / 128 >= 8 && tiles >= (long long)(c.cus & ~7) && (c.cus & ~7) >= 8;
}
// Automatic choice (profiles/r04_tile_walk_sweep.txt: plain vs walk over nine layer shapes x five token counts x both modes).
// A seam costs 5.5 us (per-group 7) where the plain grid pays 9 us between two tiles of a CU (epilogue 6.3 + relaunch 0.2 +
// prologue 2.6), and the walk's stage loop pays ~2-3 % for its per-stage bookkeeping: it wins where tiles are short and every CU
// gets more than one -- K <= 6144 (4096 / 5120-deep layers: +4 ... +8 % from two tiles per CU on; +9 ... +15 % on a slow box,
// profiles/r04_walk_zero_operands.txt).  At K = 8192 the sweep's box read it neutral (-1.4 ... +1.7 %), three other boxes +1 ... +6 %
// (profiles/r04_dispatch_check_mid_shapes.txt, r04_walk_larger_k.txt): on, since the end of round 4.  K = 11008: -3.6 ... +2 % box to box,
// K = 21760: -6 ... +1 %: off.  256 x 256 tiles only: the 128-column shape loses with it, the 128-token shape gains less.
static bool wide_chain_pays(const PlanCtx& c, long long tiles, int mt, int bn) {
  return mt == 16 && bn == 256 && c.K / 128 <= 64 && tiles > (long long)(c.cus & ~7);
}

// uneven K slices, the rule every family shares: tune.skew > 0 asks for that many stages, 0 takes the family's automatic rule, -1 keeps the slices
// even; never more than the room the slices' minimum length leaves, nor than the kernel argument's field holds
static int clamp_skew(int asked, int automatic, int room, int field_max) {
  int sk = asked > 0 ? asked : (asked == 0 ? automatic : 0);
  if (sk > room) sk = room;
  if (sk > field_max) sk = field_max;
  return sk > 0 ? sk : 0;
}

// The dispatch decision of one call, as plain data (pure host logic: also exported as qqq_w4a8_plan so
// that it can be inspected and tested without a GPU).
struct Plan {
  int kernel;  // 1 stream, 2 tiled, 3 column, 4 panel, 5 wide
  int ksplit;
  int fused;   // stream: 1 / 3 in-launch, 2 separate reduce.  tiled: 1 in-launch slots, 2 slabs + reduce
  int mt, waves, pf;      // stream
  int bm, stages, nslots, pw; // tiled
  int chain;                  // wide: 1 = persistent tile walk (one workgroup per CU walks its run of tiles)
  int skew;                   // panel: extra 128-k stages of the last K slice
  int w8;                     // wide: 1 = the loop reads the expanded int8 weights (the call has them)
  int exch;                   // wide, two K slices of 256-column tiles: 1 = exchange hand-off (each slice finishes one row half), even slices
};

// (t.w8: 1 = the call has the expanded int8 weights of its layer -- gemm_ex2 sets it from its W8 argument --, -1 = ignore them)
static Plan make_plan(const PlanCtx& c, qqq_tune_t t, double* est_out = nullptr) {
  const int M = c.M, N = c.N, K = c.K;
  const bool grouped = c.grouped;
  const ScratchRoom& room = c.room;
  const bool have_w8 = t.w8 > 0 && (long long)N * K < (1ll << 32) && (K % 128) == 0;
  Plan pl;
  memset(&pl, 0, sizeof(pl));
  double est = -1.0;  // the chosen family's modelled time (us) when the choice is the models' (automatic dispatch); -1 otherwise

  // ---- kernel choice (measured on MI355X, profiles/) ----
  // decode (m <= 16): the "column" kernel (32-column workgroups over all of K, no split-K, no reduce launch);
  // m <= 128: the HBM-bound "stream" kernel (128-column strips x K slices); above, LDS tiles.
  int kernel = t.kernel;
  const bool column_ok = (N % 64) == 0 && (K % 64) == 0;
  if (kernel == 0) {
    // measured (profiles/r01_tune_decode.txt, r02_decode_sweep.txt): every column workgroup re-reads the m x K
    // activations (per-lane 16-byte loads of 16 rows), so beyond m = 8 it only wins while that stays cheap -- but then
    // up to 32 tokens (two 16-token tiles per wave), where it saves the stream kernel's reduce launch: the two small cost models above
    // (beyond 512 column workgroups -- two rounds of the chip -- the stream kernel's one round of K slices wins even at decode:
    // N = 28672, K = 8192: 23.0 vs 25.3 us per-channel, 29.1 vs 30.4 per-group, profiles/r04_dispatch_check_shapes_before.txt)
    // (narrow layers -- the k / v projections of grouped-query attention, N = 1024 / 512: 32 / 16 column workgroups, 6.3 vs 8.8 us and 6.2 vs 9.4 us
    // at decode, profiles/r04_dispatch_check_merged.txt, r04_dispatch_check_qwen_mistral.txt; below that not measured)
    // (per-group up to 16 tokens the cap of three rounds holds as at decode: N = 22016, K = 4096 at 16 tokens 15.0 vs 17.3 us)
    // Per-group the column kernel is bound by its re-quantiser (time ~ K per round), so on long-K layers the stream kernel's K slices win even
    // at decode (N = 3584, K = 18944: 15.4 vs 19.4 us; N = 4096, K = 14336: 13.5 vs 15.8): the two small models decide from one token on.
    // (a tie goes to the column kernel -- one launch instead of two; 2 % is where the measured regret of the rule is smallest: 0.27 % mean over 238 points against 0.32 % without)
    const bool col_cheaper = column_small_estimate(c) < 1.02 * stream_small_estimate(c);
    const bool column = column_ok && N / 32 >= 16 && N / 32 <= ((M <= 8 || (grouped && M <= 16)) ? 768 : 512) &&
                        (grouped ? (M <= 32 && col_cheaper) : (M <= 8 || (M <= 32 && col_cheaper)));
    if (column) kernel = 3;
    else kernel = (M <= 128 || (K % 128) != 0) ? 1 : 2;
    if (column_ok && M <= 32) est = column ? column_small_estimate(c) : stream_small_estimate(c);
    // 17 ... 32 tokens: the panel kernel's 32-token m-blocks are a third candidate -- on very wide layers 256-column strips in two or three K slices beat both
    // (N = 20480, K = 7168 at 32 tokens: 21.7 us against 27.2 / 32.6; N = 28672 / 29568: 10 - 12 %; 10 of the 192 measured points, profiles/r05_dispatch_check_*.txt).
    // It has to be clearly ahead (5 %: the three models are each good to 3 - 4 %).  (Up to 16 tokens it won 3 of 116 measured points, and the one time the models
    // picked it there -- N = 20480, K = 7168 -- the clock said 20.2 us against the stream kernel's 16.6: not a candidate.)
    if (column_ok && M > 16 && M <= 32 && t.bm == 0 && t.mt == 0 && t.ksplit <= 0) {
      int pbn = 128, pks = 1, pcw = 1;
      const double e_panel = panel_estimate(c, &pbn, &pks, &pcw);
      if (e_panel < 0.95 * est) {
        kernel = 4;
        est = e_panel;
        t.bm = pbn;
        t.ksplit = pks;
      }
    }
    // Above the decode regime the family is picked by the three cost models.  The panel kernel is also the MFMA path
    // with LDS-shared activations for K % 128 == 64 at any m (the tiled kernel needs 128-k blocks).
    if (column_ok && !column && M > 32) {
      int pbn = 128, pks = 1, pcw = 1, pmt = 0;
      const double e_panel = ((long long)(M + 127) / 128 <= 65535) ? panel_estimate(c, &pbn, &pks, &pcw, &pmt) : 1e30;
      // (round 6: above 64 tokens the stream kernel is a candidate only where its GENERATED form prices it -- 2 ... 4 m-blocks on layers up to ~40 MB, kQqqSmall.stmid.  The
      //  regime beyond -- larger layers, five m-blocks and more -- was the last hand-fitted branch of the dispatcher (stream_estimate below its first return); in the 48 points of it
      //  that the committed grids measured the stream kernel is never more than 3 % ahead of the best panel / wide shape, and the plan never chose it: out of the automatic path.
      //  tune.kernel = 1 still runs it; qqq_w4a8_model_us still prices it.)
      const int s_mblocks = (M + 63) / 64;
      const bool stream_candidate = s_mblocks == 1 || (s_mblocks <= 4 && (double)N * K / 2.0 / 5.0e6 < 8.0);
      const double e_stream = (M <= 256 && stream_candidate) ? stream_estimate(c) : 1e30;
      // (the tiled family -- round 1's LDS-tiled 32x32x32 kernel -- is no longer a candidate of the automatic dispatch: in the 903 measured
      // dispatch points of round 4 it never won one (M = 4096: 585.9 vs 449.2 us).  It stays reachable through tune.kernel = 2 -- the
      // differential fuzzers' independent reference -- and as the fallback for packed weights beyond 4 GB, where the wide kernel's 32-bit
      // offsets end.)
      int wks = 1, wmt = 16, wbn = 256;
      const double e_wide = (M > 256) ? wide_estimate(c, &wks, &wmt, &wbn, have_w8) : 1e30;
      est = e_wide < e_panel ? e_wide : e_panel;
      if (e_stream < est) est = e_stream;
      if (e_wide < e_panel && e_wide < e_stream) {
        kernel = 5;
        // (the K split was costed for the model's own tile shape: a caller who pins mt / bm gets one slice unless it asks)
        if (t.mt == 0 && t.bm == 0) {
          t.mt = wmt;
          t.bm = wbn;
          if (t.ksplit <= 0) t.ksplit = wks;
        }
      } else if (e_panel <= e_stream) {
        kernel = 4;
        if (t.bm == 0 && t.pw == 0 && t.mt == 0 && pcw == 2) t.pw = 2;
        if (t.bm == 0 && t.mt == 0 && pmt) t.mt = pmt;  // several 64-token m-blocks instead of 128-token ones
        if (t.bm == 0) t.bm = pbn;
        if (t.ksplit <= 0) t.ksplit = pks;
      } else {
        kernel = 1;
      }
    }
  }
  if (est_out) *est_out = est;
  if ((kernel == 3 || kernel == 4 || kernel == 5) && !column_ok) kernel = 1;
  if (kernel == 5 && (K % 128) != 0) kernel = 4;                        // whole 128-k stages only
  if (kernel == 5 && (long long)N * K / 2 >= (1ll << 32)) kernel = 2;  // 32-bit offsets into the packed weights
  if (kernel == 2 && (K % 128) != 0) kernel = 1;
  pl.kernel = kernel;
  int ksplit = 1;

  if (kernel == 5) {
    // wide: 256 (mt = 8: 128) tokens x 256 columns per workgroup, 4 waves with 512 registers each; in-launch split-K with
    // one slot of C per depositing slice (row-major partial tiles) and two ticket words per tile
    pl.mt = (t.mt == 8) ? 8 : 16;                         // 16-token m-tiles per workgroup: 256- or 128-token tiles
    pl.bm = (t.bm == 128 && pl.mt == 16) ? 128 : 256;     // columns per workgroup: 64 or (256-token tiles only) 32 per wave
    // (128 x 128 tiles compile from the same template and were measured: 39 us at M=128 against the panel kernel's 36, 4 % ahead
    // of it only at 160-256 tokens in two K slices -- not instantiated; profiles/r03_wide_128x128.txt)
    pl.stages = 1;                                        // activation lead: the LDS-DMA of a stage is issued a full stage ahead
    // weight ring: 4 steps of 64 k in every mode.  The packed modes load a step as 8 dwords per lane, and a ring of 8 steps would pass the 63 loads vmcnt
    // counts (the depths measured before the dword loads, 4 against 8: profiles/r05_wide_ring_depth.txt).
    const bool big_tile = (pl.mt == 16 && pl.bm == 256);
    pl.w8 = have_w8 ? 1 : 0;
    pl.pf = 4;
    pl.pw = (t.pw == 4 || t.pw == 8 || t.pw == 16 || t.pw == 32) ? t.pw : 8;
    const int rows = 16 * pl.mt;
    const long long tl = (long long)((M + rows - 1) / rows) * ((N + pl.bm - 1) / pl.bm);
    ksplit = t.ksplit > 0 ? t.ksplit : 1;
    ksplit = clampi(ksplit, 1, (K / 128) / 4 > 0 ? (K / 128) / 4 : 1);
    if (ksplit > 255) ksplit = 255;  // the arrival word's ticket field is 8 bits (the XCC nibbles sit above it; they are used up to 6 slices)
    while (ksplit > 1 && !room.fits(tl, rows, pl.bm, ksplit)) --ksplit;
    pl.ksplit = ksplit;
    pl.fused = 1;
    pl.skew = 0;
    // two slices of 256-column tiles: the exchange hand-off (qqq_wide.hip.h) on request -- tune.fused bit 64.  Measured level with the classic fold over uneven
    // slices or up to 2 % behind it (N = 8192, K = 21760 at 768 / 1024 tokens, both modes, and 4096 x 11008: profiles/r06_wide_exchange_handoff.txt): either way the
    // tile's partial sums -- 33.5 MB chip-wide at 1024 tokens -- cross the fabric once out and once back at the chip's write bandwidth, which is what the hand-off costs.
    pl.exch = (ksplit == 2 && pl.bm == 256 && t.skew <= 0 && (t.fused & 64)) ? 1 : 0;
    if (ksplit > 1 && !pl.exch)  // uneven K slices: every slice keeps at least 4 stages
      pl.skew = clamp_skew(t.skew, wide_auto_skew(pl.mt, pl.bm, grouped, ksplit, pl.w8 != 0), K / 128 - 4 * ksplit, 63);
    // the persistent tile walk (t.glds: 1 = never, 2 = whenever it applies, 0 = automatic); its ring depth is the mode's default
    pl.chain = (t.glds != 1 && wide_chain_ok(c, tl, ksplit) && (t.glds == 2 || wide_chain_pays(c, tl, pl.mt, pl.bm))) ? 1 : 0;
    if (pl.chain && pl.w8 && !big_tile) pl.chain = 0;  // (the walk over expanded weights is instantiated for 256 x 256 tiles only)
    if (pl.chain) pl.pf = 4;
    return pl;
  }

  if (kernel == 4) {
    // panel: all tokens of an m-block (16*mt <= 128) x bn columns x a K slice per workgroup; in-launch split-K with one
    // slot of C per depositing slice and two ticket words per (m-block, strip) tile
    int mt = (t.mt == 1 || t.mt == 2 || t.mt == 4 || t.mt == 8) ? t.mt : (M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8);
    const int bn = (t.bm == 256) ? 256 : 128;
    const int waves = (bn == 256) ? 8 : (t.waves == 4 ? 4 : 8);
    const int rows = 16 * mt;
    const long long mblocks = (M + rows - 1) / rows, strips = (N + bn - 1) / bn;
    const int NST = (K / 64 + 1) / 2;
    ksplit = t.ksplit;
    if (ksplit <= 0) ksplit = clampi((int)(c.cus / (strips * mblocks)), 1, 4);  // never more than one round of workgroups (on the CUs this call may use)
    ksplit = clampi(ksplit, 1, NST / 4 > 0 ? NST / 4 : 1);
    while (ksplit > 1 && !room.fits(mblocks * strips, rows, bn, ksplit)) --ksplit;
    pl.mt = mt;
    pl.bm = bn;
    const bool cw2 = (t.pw == 2 && bn == 256 && mt == 8);
    pl.pf = (t.pf == 2 || t.pf == 3 || t.pf == 8) ? t.pf : (t.pf == 0 && bn == 256 && !cw2 ? 3 : 4);  // weight prefetch depth in stages
    if (pl.pf == 8 && mt > 4) pl.pf = 4;
    // activation prefetch depth in stages: 2 with the 4-deep weight ring (the 64-column shape: 14 registers of slack, no spill
    // with the four-buffer, barrier-every-other-stage ring, profiles/r02_panel_cw2.txt; the 32-column shapes: 1-4 % faster than
    // depth 4 on every shape measured, profiles/r02_panel_prefetch_depth.txt)
    pl.stages = (pl.pf == 4 && t.stages != 4) ? 2 : pl.pf;
    // 32-column sets per wave: 2 = 4 waves x 64 columns x 2 k-groups for the 256-column, 128-token shape
    pl.pw = (cw2 && pl.pf >= 3 && pl.pf <= 4 && (pl.stages == pl.pf || (pl.pf == 4 && pl.stages == 2))) ? 2 : 1;
    pl.waves = waves;
    pl.ksplit = ksplit;
    pl.fused = 1;
    // uneven K slices: every slice keeps at least 4 stages
    pl.skew = ksplit > 1 ? clamp_skew(t.skew, panel_auto_skew(mt, bn, grouped, ksplit), NST - 4 * ksplit, 63) : 0;
    return pl;
  }

  if (kernel == 3) {
    const int mt = (t.mt >= 1 && t.mt <= 2) ? t.mt : (M <= 16 ? 1 : 2);
    const int KS = K / 64;
    ksplit = t.ksplit > 0 ? t.ksplit : 1;  // a second launch costs more than idle CUs save (measured)
    ksplit = clampi(ksplit, 1, KS);
    if (!room.slabs) ksplit = 1;
    if (ksplit > 1 && (long long)ksplit * M > room.cap_rows) ksplit = (int)(room.cap_rows / M);
    if (ksplit < 1) ksplit = 1;
    pl.mt = mt;
    // sixteen waves per workgroup (the waves split K inside the workgroup) where the re-quantiser binds: per-group up to 8 tokens -2 ... -6 % on five layer shapes
    // (BASELINE layer at decode 23.5 -> 22.05 us); per-channel mixed (+4 % there), from 9 tokens level: eight (profiles/r05_column_16_waves.txt)
    pl.waves = mt == 1 && (t.waves == 16 || (t.waves == 0 && grouped && M <= 8)) ? 16 : 8;
    pl.pf = t.pf > 0 ? t.pf : 3;
    pl.ksplit = ksplit;
    pl.fused = 2;
    return pl;
  }

  if (kernel == 1) {
    // rows are processed in m-blocks of 16*MT (grid.z); every m-block re-reads the weights, so this
    // kernel is meant for m <= 64 (one m-block) but stays correct for any m.
    const int mt = (t.mt >= 1 && t.mt <= 4) ? t.mt : clampi((M + 15) / 16, 1, 4);
    const int mblocks = (M + 16 * mt - 1) / (16 * mt);
    const int strips = (N + 127) / 128;
    const int KS = K / 64;
    int waves = t.waves ? t.waves : (mt == 1 ? 4 : 8);
    if (waves != 4 && waves != 8 && waves != 16) waves = 8;
    if (waves == 16 && mt > 1) waves = 8;  // 1024-thread blocks cap VGPRs at 128: only the MT=1 body fits
    ksplit = t.ksplit;
    if (ksplit <= 0) {
      ksplit = stream_auto_ksplit(c.cus, (long long)strips * mblocks, mt == 1, KS, waves);
      // 65 ... 256 tokens on layers up to ~40 MB: the split the loop model is fastest with (see stream_mid_estimate)
      if (mt == 4 && mblocks >= 2 && mblocks <= 4 && (double)N * K / 2.0 / 5.0e6 < 8.0) stream_mid_estimate(c, KS / (2 * waves) > 0 ? KS / (2 * waves) : 1, &ksplit);
    }
    ksplit = clampi(ksplit, 1, KS);
    if (!room.slabs) ksplit = 1;
    if (ksplit > 1 && (long long)ksplit * M > room.cap_rows) ksplit = (int)(room.cap_rows / M);
    if (ksplit < 1) ksplit = 1;
    // how the slices meet: 2 = slabs + a reduce launch (tune.fused = 0: the in-launch forms are not measured yet), 1 / 3 in-launch on request
    int fused = t.fused & 3;  // (bits 2.. are the in-launch hand-off switches of the other families)
    if (fused == 0) fused = 2;
    // tickets: one int per (m-block, strip) for the fenced fold over the slabs (1), two for the slot protocol (3); the reference guarantees
    // n/128*max_par ints.  Slots (3): (ksplit - 1) tiles of 16*mt x 128 ints per (m-block, strip), inside the rows of C we may use.
    // (these hold whether or not C has rows to use: without them the call is one slice, and the form asked for stays in the plan)
    if (fused == 1 && (long long)mblocks * strips > room.cap_tickets) fused = 2;
    if (fused == 3 && (2ll * mblocks * strips > room.cap_tickets ||
                       (long long)mblocks * strips * (ksplit - 1) * (16ll * mt * 128) > room.cap_rows * (long long)N))
      fused = 2;
    // uneven slices, in 64-k steps; every slice keeps two steps per wave
    pl.skew = (fused == 3 && ksplit > 1) ? clamp_skew(t.skew, stream_auto_skew(N, K, ksplit), KS - 2 * waves * ksplit, 255) : 0;
    pl.mt = mt;
    pl.waves = waves;
    pl.pf = t.pf > 0 ? t.pf : (mt <= 2 ? 3 : 2);
    pl.ksplit = ksplit;
    pl.fused = fused;
    return pl;
  }

  // ---- tiled ----
  // Split-K comes in two forms.  In-launch (default when it fits): the K slices of a tile meet in tile-sized
  // int32 slots of C, tickets in `workspace`, the last arrival runs the epilogue -- needs one slot per tile
  // (<= max_par*64 rows of C) whatever ksplit is.  Slabs + separate reduce launch: ksplit full [m, n] slabs.
  const long long strips = (N + 255) / 256;
  const bool slabs_only = (t.fused & 3) == 2;
  int bm = t.bm;
  if (bm != 64 && bm != 128 && bm != 256 && bm != 258 && bm != 259 && bm != 130 && bm != 131) {
    int best_ks = 1;
    (void)tiled_estimate(c, slabs_only, &bm, &best_ks);
    if (t.ksplit <= 0) t.ksplit = best_ks;
  }
  // glds: 2 = register-staged, 1 = LDS-DMA ring with `stages` buffers; auto: the DMA ring pays at the
  // 8-wave 256-row tile, register staging is faster for the 4-wave tiles (measured)
  int stages;
  if (t.glds == 2) stages = 0;
  else if (t.glds == 1) stages = ((t.stages >= 2 && t.stages <= 4) || (t.stages == 5 && bm != 64 && bm != 128) || ((t.stages == 6 || t.stages == 7) && bm == 256)) ? t.stages : (bm >= 256 ? 3 : 4);
  else stages = (bm == 256) ? 7 : (bm == 258) ? 2 : (bm == 130) ? 4 : 0;  // measured best per shape (profiles/r01_tune_sweep_*.txt, r02_tiled_ns7.txt)
  if (bm >= 256 && stages == 4) stages = 3;
  const int bm_rows = (bm >= 256) ? 256 : (bm >= 128 ? 128 : bm);
  const long long tiles = (long long)((M + bm_rows - 1) / bm_rows) * strips;
  ksplit = t.ksplit;
  if (ksplit <= 0) {
    ksplit = tiles >= 192 ? 1 : (int)((256 + tiles - 1) / tiles);
    ksplit = clampi(ksplit, 1, (K / 128) / 4 > 0 ? (K / 128) / 4 : 1);
  }
  ksplit = clampi(ksplit, 1, K / 128);
  if (!room.slabs) ksplit = 1;
  const int nslots = slot_count(c, bm_rows, ksplit, slabs_only);
  if (nslots == 0 && ksplit > 1 && (long long)ksplit * M > room.cap_rows) ksplit = (int)(room.cap_rows / M);
  if (ksplit < 1) ksplit = 1;
  pl.bm = bm;
  pl.stages = stages;
  // Tile order: an XCD runs 32 workgroups at a time = (32 / PW) m-tiles x PW weight strips.  Per 128-k block a
  // strip costs 16 KB of L2 fill and an m-tile rows/2 KB, so 4 x 8 is the cheapest split for 256- and 128-row
  // tiles (measured M=4096: L2 miss traffic 892 -> 714 MB per launch, profiles/r01_hbm_traffic.txt), 8 x 4 for 64 rows.
  pl.pw = (t.pw == 4 || t.pw == 8 || t.pw == 16 || t.pw == 32) ? t.pw : (bm == 64 ? 4 : 8);
  pl.ksplit = ksplit;
  pl.nslots = ksplit > 1 ? nslots : 0;
  pl.fused = pl.nslots > 0 ? 1 : 2;
  return pl;
}

// ---- M split (rows are independent).  A token count one past a whole number of rounds of 256 x 256 tiles costs a partial extra round of the wide
// kernel: N = 8192, K = 21760: 4096 tokens 451 us, 4097 tokens 624 us -- and 464 us as 4096 + 1 tokens in two launches on the same stream; 2049 tokens
// 341 -> 240 us; N = 4096, K = 11008 at 4100 tokens 188 -> 134 us (profiles/r04_ragged_m.txt).  For the automatic dispatch, when the whole call is the
// wide kernel's: the rows that fill whole tiles (or whole rounds) go first, the remainder (at most 2048 tokens) follows as a call of its own, if the
// models price the pair at least 7 % below the single launch.  Returns the first launch's rows, 0 = no split.
// (the largest remainder that is tried; QQQ_AMD_SPLIT_CAP overrides it for measurements -- 512 against 4096 on five layer shapes, profiles/r04_ragged_m.txt:
// the larger remainders gain 5 ... 13 % wherever the models choose them and lose nowhere)
static int split_remainder_cap() {
  static const int cap = [] {
    const char* e = getenv("QQQ_AMD_SPLIT_CAP");
    if (!e) return 2048;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    return (end == e || *end != 0 || v <= 0 || v > (1 << 20)) ? 2048 : (int)v;  // not a positive number: the default, not "never split"
  }();
  return cap;
}
static int choose_split(const PlanCtx& c, const qqq_tune_t& t, const Plan& pl, const double est_whole) {
  if (t.split_m < 0 || t.kernel != 0 || t.mt != 0 || t.bm != 0 || t.ksplit > 0 || pl.kernel != 5 || est_whole <= 0.0) return 0;
  const int M = c.M, N = c.N, cus = c.cus;
  const int rows = 16 * pl.mt;
  const long long tiles_n = (N + pl.bm - 1) / pl.bm;
  int cand[3] = {(M / rows) * rows, 0, 0};
  const long long tiles = (long long)((M + rows - 1) / rows) * tiles_n;
  if (tiles > cus) cand[1] = (int)((tiles / cus) * cus / tiles_n) * rows;  // the m-blocks that whole rounds cover
  // ... and the whole rounds of 256 x 256 tiles, whatever shape the whole call was planned in (round 6: with the refitted rates 5000 tokens at the BASELINE layer are
  // planned as 256 x 128 tiles -- five full rounds, 598 us by the model -- whose own candidates do not contain 4096 + 904: 545 us, measured 560 against 620)
  const long long tiles256 = (long long)((M + 255) / 256) * ((N + 255) / 256);
  if (tiles256 > cus) cand[2] = (int)((tiles256 / cus) * cus / ((N + 255) / 256)) * 256;
  int best_m0 = 0;
  double best = 0.93 * est_whole;
  qqq_tune_t tn = t;
  tn.split_m = -1;
  for (int i = 0; i < 3; ++i) {
    const int M0 = cand[i];
    if (M0 <= 0 || M0 >= M || M - M0 > split_remainder_cap() || (i >= 1 && M0 == cand[0]) || (i == 2 && M0 == cand[1])) continue;
    double e0 = -1.0, er = -1.0;
    PlanCtx first = c, rest = c;
    first.M = M0;
    rest.M = M - M0;
    (void)make_plan(first, tn, &e0);
    (void)make_plan(rest, tn, &er);
    if (e0 > 0.0 && er > 0.0 && e0 + er < best) {
      best = e0 + er;
      best_m0 = M0;
    }
  }
  return best_m0;
}

// qqq_w4a8_plan: the decision for `c` in the fields of a qqq_tune_t (include/qqq_amd.h says which field means what on the way out)
static void plan_report(const PlanCtx& c, const qqq_tune_t& t, qqq_tune_t* plan_out) {
  double est = -1.0;
  const Plan pl = make_plan(c, t, &est);
  memset(plan_out, 0, sizeof(*plan_out));
  plan_out->split_m = choose_split(c, t, pl, est);
  plan_out->kernel = pl.kernel;
  plan_out->ksplit = pl.ksplit;
  plan_out->fused = pl.fused | (pl.kernel == 5 && pl.exch ? 64 : 0);
  plan_out->waves = pl.waves;
  plan_out->pf = pl.pf;
  plan_out->mt = pl.mt;
  plan_out->bm = pl.bm;
  plan_out->stages = pl.stages;
  plan_out->glds = pl.kernel == 2 ? (pl.stages == 0 ? 2 : 1) : pl.kernel == 5 ? (pl.chain ? 2 : 1) : 0;
  plan_out->nslots = pl.nslots;
  plan_out->pw = pl.pw;
  plan_out->skew = pl.skew;
  plan_out->w8 = pl.w8;
}

// qqq_w4a8_model_us: the cost models' price (us) of each family for one problem, exactly as make_plan evaluates them -- so that ONE tool
// (tools/cost_model_report.py) can hold every model against every committed measurement.  out[0] column, [1] stream, [2] panel, [3] wide; <= 0: not a
// candidate at this size.  (`c` as of a call that has C and a workspace.)
static void model_us(const PlanCtx& c, double out[4]) {
  const int M = c.M;
  for (int i = 0; i < 4; ++i) out[i] = -1.0;
  int bn = 0, ks = 0, cw = 0, mt = 0;
  if (M <= 32) {
    out[0] = column_small_estimate(c);
    out[1] = stream_small_estimate(c);
    if (M > 8) out[2] = panel_estimate(c, &bn, &ks, &cw);
    return;
  }
  if (M <= 256) out[1] = stream_estimate(c);
  out[2] = panel_estimate(c, &bn, &ks, &cw, &mt);
  if (M > 256) {
    const double w = wide_estimate(c, &ks, &mt, &bn);
    out[3] = w < 1e29 ? w : -1.0;
  }
}

#endif  // QQQ_AMD_QQQ_PLAN_H_
