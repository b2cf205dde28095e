// qqq_w4a8.hip -- MI355X (gfx950 / CDNA4) W4A8 GEMM kernels behind QQQ's `qqq_gemm` operator.
//
// Not a port of the reference CUDA kernel (csrc/qqq_gemm.cu): the only things shared with it are
// the DATA contracts -- the Marlin/QQQ packed int4 layout produced by QuantLinear.pack()
// (qlinear_marlin.py:147-262) and the arithmetic
//     D[m,n] = fp16_rn( (f32_rn(sum_k A[m,k] * Wq[k,n]) * s2[n]) * s1[m] )
// (csrc/qqq_gemm.cu:106-117, :146-151, :167-210, :695-700).  Everything else is designed for
// wave64 / MFMA / LDS:
//
//  * Packed layout, closed form: word B[kt][128*ng + 4*(4*c + kq) + jt] holds, for k-tile kt
//    (16 k) and 64-column group ng, the 4 consecutive k = 16*kt + 4*kq + r (r = 0..3) of the two
//    columns n = 64*ng + 16*jt + c + 8*b (b = 0,1).  Hence for a fixed (kt, ng, c) the 64
//    contiguous bytes [64*c, 64*c+64) of the 512-byte block are ALL 16 k of the 8 columns
//    {16*jt + 8*b + c}.  One lane that loads those 64 bytes owns complete MFMA operands
//    (16 int8 along k) for 8 columns: the unpack `q & 0xF0F0F0F0`, `(q << 4) & 0xF0F0F0F0`
//    doubles as the register transpose, no cross-lane traffic, every bit used exactly once.
//  * MFMA operand roles are swapped w.r.t. the textbook: the WEIGHTS are the MFMA "A" operand
//    (tile row i <-> weight column n), the ACTIVATIONS the "B" operand (tile column j <-> token m),
//    so that each lane ends up with 4 CONSECUTIVE n of one token: 8-byte fp16 stores, 16-byte
//    int32 partial-sum stores.  The integer dot products do not care about the k order inside
//    an operand as long as both operands use the same order ("k-slot freedom"), and the
//    packed order [kq][r] IS natural k order, so the activation operand is 16 contiguous bytes.
//
// Where things are (one translation unit: this file includes the rest):
//   qqq_common.hip.h   vector types, loads / stores, the split-K hand-off primitives; LaunchArgs and the dynamic-LDS helper of the launch tables
//   qqq_column.hip.h   "column" kernel: decode, m <= 8 and up to 32 tokens while m * K is small; 32 weight columns x all of K per workgroup, one launch
//   qqq_stream.hip.h   "stream" kernel: a few tens of tokens; weights HBM -> VGPR, waves and workgroups split K, int32 slabs in C
//   qqq_panel.hip.h    "panel" kernel: about 64 ... 1024 tokens; an m-block of up to 128 tokens x 128 / 256 columns x a K slice, in-launch split-K
//   qqq_wide.hip.h     "wide" kernel: from ~320 tokens up; 256 x 256 / 256 x 128 / 128 x 256 tiles, hand-placed loop, persistent tile walk, expanded weights
//   qqq_tiled.hip.h    "tiled" kernel: tune.kernel = 2 only -- the fuzzers' independent reference, the fallback beyond 4 GB of packed weights
//   qqq_small.hip.h    split-K reduce, dynamic quantiser, int4 packer / unpacker, int8 expander
//   qqq_act.hip.h, qqq_attn.hip.h, qqq_decode.hip.h   the decoder block's fused quantisers, RoPE + KV-cache write, split-K decode attention
//   qqq_kv8.hip.h      the int8 KV cache: the quantising RoPE / cache write and the decode split kernel that reads it
//   qqq_shared.hip.h   decode attention of sibling rows over a shared prefix of their block tables: joint splits, bit for bit the paged decode
//   qqq_paged.hip.h    the block-table (paged) KV cache, fp16 and int8: the cache writes by slot and the decode split kernels through a block table
//   qqq_prefill.hip.h  paged, ragged, causal prefill attention over the block pools (fp16 and int8) and the quantisation of its rows
//   qqq_sample.hip.h   the fused token sampler: temperature, top-k, top-p and the draw over a batch of fp16 logit rows, one launch
//   qqq_score.hip.h    the fused scoring kernel: a target token's log-probability and the argmax per fp16 logit row, one launch (the sampler's weights)
//   qqq_logprobs.hip.h the fused top-k log-probability kernel: a token's log-probability and rank and the k most probable tokens per row, one launch
//   qqq_step.hip.h     the decode loop's step: that sampler with an epilogue that advances each row's decode state on the device
//   qqq_penalty.hip.h  the repetition / presence / frequency penalty: fp16 logit rows rewritten in place from each row's token history, one launch
//   qqq_spec.hip.h     the speculative decode loop's step: draft_len + 1 draws per row by that sampler, the accept rule and the n-gram drafter
//   qqq_stop.hip.h     stop sequences, stop token ids and the minimum length: the ban in front of a sampler, the check behind a loop's step
//   qqq_guided.hip.h   guided decoding over a token automaton in device memory: the mask in front of a sampler, the advance behind a loop's step
//   qqq_lora.hip.h     the batched LoRA op: fp16 low-rank adapters added to a GEMM's output, every token's adapter read from device memory
//   each family's header ends with its launch table: the list of instantiations next to the template it instantiates
//   qqq_plan.h         the dispatch planner (make_plan, the cost models, the M split): pure host C++, no HIP; its rates are GENERATED into
//   qqq_rates.h        by tools/fit_rates.py and held against the committed measurements by tools/cost_model_report.py
//   this file          error state, the reference's shape validation, the CU-masked stream of `sms`, and the C-ABI entry points
//
// The accumulators are the reference's: per-channel weights enter as 16*w4 (high nibble of each
// byte) and pack() has pre-divided s_channel by 16; per-group weights are re-quantised to int8
// with ONE packed-fp16 FMA exactly like dequant_per_group (csrc/qqq_gemm.cu:167-210).

#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "qqq_common.hip.h"
#include "qqq_stream.hip.h"
#include "qqq_column.hip.h"
#include "qqq_panel.hip.h"
#include "qqq_tiled.hip.h"
#include "qqq_wide.hip.h"
#include "qqq_small.hip.h"
#include "qqq_act.hip.h"
#include "../../include/qqq_amd_act.h"
#include "qqq_attn.hip.h"
#include "../../include/qqq_amd_attn.h"
#include "qqq_decode.hip.h"
#include "../../include/qqq_amd_decode.h"
#include "qqq_kv8.hip.h"
#include "../../include/qqq_amd_kv8.h"
#include "qqq_paged.hip.h"
#include "../../include/qqq_amd_paged.h"
#include "qqq_qknorm.hip.h"
#include "../../include_ops/qqq_amd_qknorm.h"
#include "qqq_prefill.hip.h"
#include "../../include/qqq_amd_prefill.h"
#include "qqq_sample.hip.h"
#include "../../include/qqq_amd_sample.h"
#include "qqq_score.hip.h"
#include "../../include/qqq_amd_score.h"
#include "qqq_logprobs.hip.h"
#include "../../include/qqq_amd_logprobs.h"
#include "qqq_beam.hip.h"
#include "../../include/qqq_amd_beam.h"
#include "qqq_step.hip.h"
#include "../../include/qqq_amd_step.h"
#include "qqq_spec.hip.h"
#include "../../include/qqq_amd_spec.h"
#include "qqq_verify.hip.h"
#include "../../include/qqq_amd_verify.h"
#include "qqq_shared.hip.h"
#include "../../include/qqq_amd_shared.h"
#include "qqq_penalty.hip.h"
#include "../../include/qqq_amd_penalty.h"
#include "qqq_stop.hip.h"
#include "../../include/qqq_amd_stop.h"
#include "qqq_guided.hip.h"
#include "../../include/qqq_amd_guided.h"
#include "qqq_lora.hip.h"
#include "../../include/qqq_amd_lora.h"
#include "qqq_plan.h"

// ------------------------------------------------------------------------------------------
// host side: validation (mirrors the reference's), dispatch, C-ABI
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return QQQ_ERR_HIP;
}

struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev && dev >= 0) {
      changed = (hipSetDevice(dev) == hipSuccess);
    }
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

// reference: is_valid_config (csrc/qqq_gemm.cu:867-897)
static bool ref_valid_config(int thread_k, int thread_n, int num_threads, int n, int k) {
  if (thread_k == -1 || thread_n == -1 || num_threads == -1) return false;
  if (k % thread_k != 0 || n % thread_n != 0) return false;
  if (thread_k != 128 && thread_k != 64) return false;
  if (thread_n < 64 || thread_k < 64) return false;
  if (num_threads < 128) return false;
  return true;
}

// reference: determine_thread_config + the CALL_IF table (csrc/qqq_gemm.cu:847-865, :899-945,
// :1033-1036).  Returns 0 / ERR_PROB_SHAPE / ERR_KERN_SHAPE exactly when the reference does.
static int ref_shape_check(int m, int n, int k, int groupsize, int thread_k, int thread_n) {
  struct Cfg { int tk, tn, nt; };
  static const Cfg small_cfgs[4] = {{128, 128, 256}, {128, 64, 128}, {64, 256, 256}, {64, 128, 128}};
  static const Cfg large_cfgs[4] = {{64, 256, 256}, {128, 128, 256}, {64, 128, 128}, {128, 64, 128}};
  Cfg cfg = {-1, -1, -1};
  if (thread_k != -1 && thread_n != -1) {
    cfg = {thread_k, thread_n, 256};
  } else {
    const Cfg* list = (m <= 16) ? small_cfgs : large_cfgs;
    for (int i = 0; i < 4; ++i)
      if (ref_valid_config(list[i].tk, list[i].tn, list[i].nt, n, k)) {
        cfg = list[i];
        break;
      }
  }
  const int group_blocks = (groupsize == -1) ? -1 : groupsize / 16;
  if (!ref_valid_config(cfg.tk, cfg.tn, cfg.nt, n, k) || (group_blocks != -1 && group_blocks != 0 && k % group_blocks != 0) ||
      group_blocks == 0)
    return QQQ_ERR_PROB_SHAPE;
  if (m == 0 || n == 0 || k == 0) return QQQ_OK;
  const int nb = cfg.tn / 16, kb = cfg.tk / 16;
  const bool known = (nb == 8 && kb == 8 && cfg.nt == 256) || (nb == 16 && kb == 4 && cfg.nt == 256) ||
                     (nb == 8 && kb == 4 && cfg.nt == 128) || (nb == 4 && kb == 8 && cfg.nt == 128);
  if (!known || (group_blocks != -1 && group_blocks != 8)) return QQQ_ERR_KERN_SHAPE;
  return QQQ_OK;
}

// `sms` as a CU cap (the reference launches `sms` persistent threadblocks, csrc/qqq_gemm.cu:998, :1016-1036): the call's kernels run on a
// library-owned stream created with a CU mask of `sms` CUs, forked from and joined back into the caller's stream with two events -- the
// caller sees the usual stream order and `sms` CUs' worth of occupancy, the other CUs stay free for whatever else it runs (RCCL's kernels
// in the sharded sweep).
// The mask, as read off the hardware (tools/cu_mask_probe.py, profiles/r06_cu_mask_probe.txt): bit i is CU i / 8 of XCD
// i % 8 -- the bits are dealt round-robin over the XCDs --, and an XCD whose bits are ALL zero is not restricted at all.  So the FIRST `sms`
// bits are set (an even spread: sms / 8 CUs per XCD, the first sms % 8 XCDs one more), and the smallest cap that holds is 8 (one CU per
// XCD): 0 < sms < 8 runs on 8 CUs.  (Round 5 set every (CUs / sms)-th bit: sms = 64 enabled all of XCDs 3 and 7 and left the other six
// unrestricted -- no cap at all.)
// One stream + two events per (device, sms, caller stream) -- callers on independent streams do not serialise on one masked stream --, created
// on first use and kept for the life of the process (at most 64 entries; beyond that callers share the (device, sms) entry of the NULL stream);
// the fork / launch / join sequence of a call holds the entry's lock.  A call whose stream is being CAPTURED is not masked: kernel nodes carry
// no CU mask (a replayed graph is never capped), and pulling a shared library-owned stream into somebody's capture would make every other
// capped call on it part of that graph (or an error) until the capture ends.
struct MaskedStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex mu;
};
static int masked_cus(int sms) { return sms < 8 ? 8 : sms; }
static MaskedStream* masked_stream(int dev, int sms, int cus, hipStream_t caller) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, hipStream_t>, MaskedStream*> cache;
  std::lock_guard<std::mutex> lk(mu);
  if (cache.size() >= 64 && cache.find({dev, sms, caller}) == cache.end()) caller = nullptr;
  auto it = cache.find({dev, sms, caller});
  if (it != cache.end()) return it->second;
  uint32_t mask[16] = {};
  for (int i = 0; i < masked_cus(sms) && i < cus && i < 512; ++i) mask[i >> 5] |= 1u << (i & 31);
  MaskedStream* m = new MaskedStream;
  if (hipExtStreamCreateWithCUMask(&m->s, (uint32_t)((cus + 31) / 32), mask) != hipSuccess ||
      hipEventCreateWithFlags(&m->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->join, hipEventDisableTiming) != hipSuccess) {
    delete m;  // (a stream or event that was created stays with the runtime: this path is an out-of-resources error)
    return nullptr;
  }
  cache[{dev, sms, caller}] = m;
  return m;
}
// the fork into a masked stream, joined back into the caller's stream on EVERY way out of the call (error returns included: the caller's
// stream must not be left waiting on nothing, nor the masked stream's work un-ordered against what the caller enqueues next)
struct MaskedFork {
  MaskedStream* ms = nullptr;
  hipStream_t caller = nullptr;
  std::unique_lock<std::mutex> lock;
  hipError_t join() {
    if (!ms) return hipSuccess;
    hipError_t e = hipEventRecord(ms->join, ms->s);
    if (e == hipSuccess) e = hipStreamWaitEvent(caller, ms->join, 0);
    ms = nullptr;
    lock.unlock();
    return e;
  }
  ~MaskedFork() { (void)join(); }
};

// compute units of device `dev` (queried for THAT device, cached)
static int device_cus_of(int dev) {
  static int cus[64] = {};
  if (dev >= 0 && dev < 64 && cus[dev] > 0) return cus[dev];
  int n = 0;
  if (dev < 0 || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (dev >= 0 && dev < 64) cus[dev] = n;
  return n;
}
// process-wide switches read once from the environment: bit 4 = QQQ_AMD_NO_LOCAL_DEPOSITS=1 (as tune.fused | 16: split-K deposits are always
// written through -- the kill switch for the XCD-local hand-off, should a driver or partition mode change what HW_REG_XCC_ID / the L2 do)
static int handoff_env_flags() {
  static const int f = [] {
    const char* e = getenv("QQQ_AMD_NO_LOCAL_DEPOSITS");
    return (e && e[0] == '1') ? 4 : 0;
  }();
  return f;
}

// qqq_w4a8_plan / qqq_w4a8_model_us -- pure host logic, no HIP call -- plan for the MI355X's 256 CUs
extern "C" int qqq_w4a8_plan(int prob_m, int prob_n, int prob_k, int groupsize, int max_par, int have_scratch,
                             int have_workspace, const qqq_tune_t* tune, qqq_tune_t* plan_out) {
  g_err[0] = 0;
  if (!plan_out || prob_m <= 0 || prob_n <= 0 || prob_k <= 0) {
    snprintf(g_err, sizeof(g_err), "qqq_w4a8_plan: bad argument");
    return QQQ_ERR_ARG;
  }
  qqq_tune_t t;
  memset(&t, 0, sizeof(t));
  if (tune) t = *tune;
  plan_report(plan_ctx(prob_m, prob_n, prob_k, groupsize != -1, 256, max_par, have_scratch != 0, have_workspace != 0), t, plan_out);
  return QQQ_OK;
}

extern "C" int qqq_w4a8_model_us(int prob_m, int prob_n, int prob_k, int groupsize, int max_par, double* out) {
  g_err[0] = 0;
  if (!out || prob_m <= 0 || prob_n <= 0 || prob_k <= 0 || (prob_n % 64) != 0 || (prob_k % 64) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_w4a8_model_us: bad argument");
    return QQQ_ERR_ARG;
  }
  model_us(plan_ctx(prob_m, prob_n, prob_k, groupsize != -1, 256, max_par, true, true), out);
  return QQQ_OK;
}

extern "C" int qqq_w4a8_gemm_ex(const void* A, const void* B, void* C, void* D, const void* s1,
                                const void* s2, const void* s3, int prob_m, int prob_n, int prob_k,
                                void* workspace, int groupsize, int dev, void* stream, int thread_k,
                                int thread_n, int sms, int max_par, const qqq_tune_t* tune,
                                int32_t* acc_out, const void* bias) {
  return qqq_w4a8_gemm_ex2(A, B, C, D, s1, s2, s3, prob_m, prob_n, prob_k, workspace, groupsize, dev, stream, thread_k, thread_n, sms, max_par,
                           tune, acc_out, bias, nullptr);
}

extern "C" int qqq_w4a8_gemm_ex2(const void* A, const void* B, void* C, void* D, const void* s1,
                                 const void* s2, const void* s3, int prob_m, int prob_n, int prob_k,
                                 void* workspace, int groupsize, int dev, void* stream, int thread_k,
                                 int thread_n, int sms, int max_par, const qqq_tune_t* tune,
                                 int32_t* acc_out, const void* bias, const void* W8) {
  g_err[0] = 0;
  const int rc = ref_shape_check(prob_m, prob_n, prob_k, groupsize, thread_k, thread_n);
  if (rc != QQQ_OK) return rc;
  if (prob_m == 0 || prob_n == 0 || prob_k == 0) return QQQ_OK;  // reference :1002-1003
  if (!A || !B || !D || !s1 || !s2 || (groupsize != -1 && !s3)) {
    snprintf(g_err, sizeof(g_err), "null pointer argument");
    return QQQ_ERR_ARG;
  }
  // the kernels use 16-byte vector / LDS-DMA accesses on A, B, C, D, bias, acc_out, s3 and 8-byte loads on s2
  if ((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)D | (uintptr_t)bias | (uintptr_t)acc_out |
        (groupsize != -1 ? (uintptr_t)s3 : 0)) & 15) != 0 ||
      (((uintptr_t)s2) & 7) != 0 || (((uintptr_t)s1 | (uintptr_t)workspace) & 3) != 0 || (((uintptr_t)W8) & 15) != 0) {
    snprintf(g_err, sizeof(g_err), "misaligned pointer argument (A/B/C/D/s3/bias/acc_out/W8: 16 bytes, s2: 8, s1/workspace: 4)");
    return QQQ_ERR_ARG;
  }
  const bool grouped = groupsize != -1;
  qqq_tune_t t;
  memset(&t, 0, sizeof(t));
  if (tune) t = *tune;
  // the layer's expanded int8 weights (qqq_expand_int8): used where the plan is the wide kernel's; tune.w8 = -1 ignores them
  t.w8 = (W8 != nullptr && t.w8 >= 0) ? 1 : -1;
  const int M = prob_m, N = prob_n, K = prob_k;
  // the device this call runs on decides the CU count the plan AND the launch work with (not "the current device"); `sms`
  // (reference: the number of persistent threadblocks, -1 = every SM) caps it (a capped call used to be planned for a full chip)
  int cur_dev = dev;
  if (dev < 0) (void)hipGetDevice(&cur_dev);
  const int cus_dev = device_cus_of(cur_dev);
  const bool capped = sms > 0 && sms < cus_dev;
  const PlanCtx ctx = plan_ctx(M, N, K, grouped, capped ? masked_cus(sms) : cus_dev, max_par, C != nullptr, workspace != nullptr);
  if (handoff_env_flags() & 4) t.fused |= 16;  // QQQ_AMD_NO_LOCAL_DEPOSITS=1: every split-K deposit is written through
  double est = -1.0;
  const Plan pl = make_plan(ctx, t, &est);
  if (const int M0 = choose_split(ctx, t, pl, est)) {
    // two launches on the same stream, C / workspace shared (each launch leaves the workspace zero); K % 64 == 0 and N % 64 == 0 keep every
    // offset pointer 16-byte aligned
    qqq_tune_t tn = t;
    tn.split_m = -1;
    const int rc0 = qqq_w4a8_gemm_ex2(A, B, C, D, s1, s2, s3, M0, N, K, workspace, groupsize, dev, stream, thread_k, thread_n, sms, max_par, &tn,
                                      acc_out, bias, W8);
    if (rc0 != QQQ_OK) return rc0;
    return qqq_w4a8_gemm_ex2(static_cast<const int8_t*>(A) + (size_t)M0 * K, B, C, static_cast<_Float16*>(D) + (size_t)M0 * N,
                             static_cast<const float*>(s1) + M0, s2, s3, M - M0, N, K, workspace, groupsize, dev, stream, thread_k, thread_n, sms,
                             max_par, &tn, acc_out ? acc_out + (size_t)M0 * N : nullptr, bias, W8);
  }

  LaunchArgs a;
  a.A = static_cast<const int8_t*>(A);
  a.B = static_cast<const unsigned char*>(B);
  a.C = static_cast<int32_t*>(C);
  a.D = static_cast<_Float16*>(D);
  a.s1 = static_cast<const float*>(s1);
  a.s2 = static_cast<const float*>(s2);
  a.s3 = static_cast<const _Float16*>(s3);
  a.acc_out = acc_out;
  a.bias = static_cast<const _Float16*>(bias);
  a.tickets = static_cast<int*>(workspace);
  a.M = M;
  a.N = N;
  a.K = K;
  a.cus = ctx.cus;
  a.stream = static_cast<hipStream_t>(stream);
  a.skew = pl.skew;
  a.hflags = (pl.kernel == 2 || pl.kernel == 4 || pl.kernel == 5) ? ((t.fused >> 2) & (pl.kernel == 4 ? 15 : 7)) : 0;  // (panel: bit 3 = plain grid order, the slices of a tile NOT gathered on one XCD)
  if (pl.kernel == 5 && pl.exch) a.hflags |= 8;  // (wide: bit 3 = exchange hand-off of a two-slice split)
  if (pl.kernel == 5 && (t.fused & 128)) a.hflags |= 16;  // (wide, measurement: the two slices of a tile on neighbouring XCDs)

  DeviceGuard guard(dev);
  hipError_t e = hipSuccess;
  bool reduce_launch;
  if ((pl.kernel == 1 || pl.kernel == 3 || pl.kernel == 4) && (M + 16 * pl.mt - 1) / (16 * pl.mt) > 65535) {
    snprintf(g_err, sizeof(g_err), "m=%d exceeds the grid of the small-m kernels (forced by tune)", M);
    return QQQ_ERR_ARG;
  }
  // sms < CUs: the kernels of this call go to the CU-masked stream of (device, sms, caller stream), between a fork from and a join into `stream`
  MaskedFork mf;
  if (capped) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(a.stream, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    if (cap == hipStreamCaptureStatusNone) {
      MaskedStream* ms = masked_stream(cur_dev, sms, cus_dev, a.stream);
      if (!ms) {
        snprintf(g_err, sizeof(g_err), "sms=%d: could not create a CU-masked stream", sms);
        return QQQ_ERR_HIP;
      }
      mf.lock = std::unique_lock<std::mutex>(ms->mu);
      if ((e = hipEventRecord(ms->fork, a.stream)) != hipSuccess || (e = hipStreamWaitEvent(ms->s, ms->fork, 0)) != hipSuccess)
        return fail_hip(e, "fork into the CU-masked stream");
      mf.ms = ms;
      mf.caller = a.stream;
      a.stream = ms->s;
    }
  }
  if (pl.kernel == 5) {
    if (pl.w8) a.B = static_cast<const unsigned char*>(W8);  // the loop reads the expanded weights; s3 is not touched
    e = launch_wide(a, pl.w8 ? 2 : (grouped ? 1 : 0), pl.mt, pl.bm, pl.pf, pl.pw, pl.ksplit, pl.chain != 0);
    if (e != hipSuccess) return fail_hip(e, "qqq_wide_kernel launch");
    reduce_launch = false;
  } else if (pl.kernel == 4) {
    e = launch_panel(a, grouped, pl.mt, pl.bm, pl.waves, pl.pw, pl.pf, pl.stages, pl.ksplit);
    if (e != hipSuccess) return fail_hip(e, "qqq_panel_kernel launch");
    reduce_launch = false;
  } else if (pl.kernel == 3) {
    e = launch_column(a, grouped, pl.mt, pl.pf, pl.ksplit, pl.waves);
    if (e != hipSuccess) return fail_hip(e, "qqq_column_kernel launch");
    reduce_launch = pl.ksplit > 1;
  } else if (pl.kernel == 1) {
    // kernel arg: 0 = slabs only (separate reduce launch), 1 = in-launch over the slabs with release / acquire fences, 3 = in-launch through
    // arrival-order slots (the last arrival keeps its tile in LDS; uneven slices: skew in 64-k steps rides in bits 16.. of the K split)
    e = launch_stream(a, grouped, pl.mt, pl.waves, pl.pf, pl.ksplit | ((pl.fused == 3 && pl.ksplit > 1 ? pl.skew & 0xff : 0) << 16),
                      pl.ksplit > 1 ? (pl.fused == 1 ? 1 : (pl.fused == 3 ? 3 : 0)) : 0);
    if (e != hipSuccess) return fail_hip(e, "qqq_stream_kernel launch");
    reduce_launch = pl.ksplit > 1 && pl.fused != 1 && pl.fused != 3;
  } else {
    e = launch_tiled(a, grouped, pl.bm, pl.stages, pl.ksplit, pl.nslots, pl.pw);
    if (e != hipSuccess) return fail_hip(e, "qqq_tiled_kernel launch");
    reduce_launch = pl.ksplit > 1 && pl.nslots == 0;
  }
  if (reduce_launch) {
    const long long items = (long long)M * (N / 4);
    const int blocks = (int)((items + 63) / 64 > 8192 ? 8192 : (items + 63) / 64);
    hipLaunchKernelGGL(qqq_reduce_kernel, dim3(blocks), dim3(64), 0, a.stream, a.C, a.D, a.s1, a.s2,
                       a.acc_out, a.bias, M, N, pl.ksplit);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "qqq_reduce_kernel launch");
  }
  if ((e = mf.join()) != hipSuccess) return fail_hip(e, "join from the CU-masked stream");
  return QQQ_OK;
}

extern "C" int qqq_w4a8_gemm(const void* A, const void* B, void* C, void* D, const void* s1,
                             const void* s2, const void* s3, int prob_m, int prob_n, int prob_k,
                             void* workspace, int groupsize, int dev, void* stream, int thread_k,
                             int thread_n, int sms, int max_par) {
  return qqq_w4a8_gemm_ex(A, B, C, D, s1, s2, s3, prob_m, prob_n, prob_k, workspace, groupsize, dev,
                          stream, thread_k, thread_n, sms, max_par, nullptr, nullptr, nullptr);
}

// ---- the per-row activation quantisers: qqq_dynamic_quant (kernel in qqq_small.hip.h) and those of a decoder block (include/qqq_amd_act.h; kernels in
// qqq_act.hip.h).  One launch ladder: 1024 threads per row for few rows (<= 2 per CU) or long rows, 256 otherwise; VPT 16-byte vectors per thread
// cover the row -- up to 8 x 1024 x 8 = 65536 elements, which the entry points check before they come here.
template <template <int, int> class Launch, typename... Args>
static int act_launch(const char* what, int m, int k, hipStream_t st, Args... args) {
  const int nvec = k / 8;
  const int vpt = (nvec + 255) / 256;
  if ((m <= 512 || nvec > 2048) && vpt > 2) {
    const int v4 = (nvec + 1023) / 1024;
    if (v4 <= 2)
      Launch<2, 1024>::run(m, st, args...);
    else if (v4 <= 4)
      Launch<4, 1024>::run(m, st, args...);
    else
      Launch<8, 1024>::run(m, st, args...);
  } else if (vpt <= 2)
    Launch<2, 256>::run(m, st, args...);
  else if (vpt <= 4)
    Launch<4, 256>::run(m, st, args...);
  else
    Launch<8, 256>::run(m, st, args...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, what);
  return QQQ_OK;
}

template <int VPT, int NT>
struct DynamicQuantLaunch {
  static void run(int m, hipStream_t st, const _Float16* x, int8_t* xq, float* s1, int k) {
    hipLaunchKernelGGL((qqq_dynamic_quant_kernel<VPT, NT>), dim3(m), dim3(NT), 0, st, x, xq, s1, k);
  }
};

extern "C" int qqq_dynamic_quant(const void* x, void* xq, void* s1, int m, int k, int dev,
                                 void* stream) {
  g_err[0] = 0;
  if (m == 0 || k == 0) return QQQ_OK;
  if (!x || !xq || !s1 || (k % 8) != 0 || ((uintptr_t)x & 15) != 0 || ((uintptr_t)xq & 7) != 0 || ((uintptr_t)s1 & 3) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_dynamic_quant: bad argument (k must be a multiple of 8, x 16-byte / xq 8-byte aligned)");
    return QQQ_ERR_ARG;
  }
  if (k > 65536) {
    snprintf(g_err, sizeof(g_err), "qqq_dynamic_quant: k=%d too large (max 65536)", k);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  return act_launch<DynamicQuantLaunch>("qqq_dynamic_quant_kernel launch", m, k, static_cast<hipStream_t>(stream), static_cast<const _Float16*>(x),
                                        static_cast<int8_t*>(xq), static_cast<float*>(s1), k);
}

template <int VPT, int NT>
struct RmsnormQuantLaunch {
  static void run(int m, hipStream_t st, const _Float16* x, _Float16* r, const _Float16* w, float eps, _Float16* y, int8_t* xq, float* s1, int k) {
    hipLaunchKernelGGL((qqq_rmsnorm_quant_kernel<VPT, NT>), dim3(m), dim3(NT), 0, st, x, r, w, eps, y, xq, s1, k);
  }
};

template <int VPT, int NT>
struct SiluMulQuantLaunch {
  static void run(int m, hipStream_t st, const _Float16* g, int ldg, const _Float16* u, int ldu, _Float16* y, int8_t* xq, float* s1, int i) {
    hipLaunchKernelGGL((qqq_silu_mul_quant_kernel<VPT, NT>), dim3(m), dim3(NT), 0, st, g, ldg, u, ldu, y, xq, s1, i);
  }
};

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" int qqq_rmsnorm_quant(const void* x, void* residual, const void* weight, float eps, void* y, void* xq, void* s1, int m, int k,
                                 int dev, void* stream) {
  g_err[0] = 0;
  if (m >= 0 && k >= 0 && (m == 0 || k == 0)) return QQQ_OK;
  if (m < 0 || k < 0 || (k % 8) != 0 || k > 65536) {
    snprintf(g_err, sizeof(g_err), "qqq_rmsnorm_quant: bad shape m=%d k=%d (k must be a multiple of 8, at most 65536)", m, k);
    return QQQ_ERR_ARG;
  }
  if (!x || !weight || !xq || !s1 || misaligned(x, 16) || misaligned(weight, 16) || (residual && misaligned(residual, 16)) ||
      (y && misaligned(y, 16)) || misaligned(xq, 8) || misaligned(s1, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_rmsnorm_quant: bad argument (x / weight / xq / s1 must be non-NULL; x, weight, residual, y 16-byte, "
             "xq 8-byte, s1 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  return act_launch<RmsnormQuantLaunch>("qqq_rmsnorm_quant_kernel launch", m, k, static_cast<hipStream_t>(stream),
                                        static_cast<const _Float16*>(x), static_cast<_Float16*>(residual), static_cast<const _Float16*>(weight),
                                        eps, static_cast<_Float16*>(y), static_cast<int8_t*>(xq), static_cast<float*>(s1), k);
}

extern "C" int qqq_silu_mul_quant(const void* gate, int ld_gate, const void* up, int ld_up, void* y, void* xq, void* s1, int m, int i,
                                  int dev, void* stream) {
  g_err[0] = 0;
  if (m >= 0 && i >= 0 && (m == 0 || i == 0)) return QQQ_OK;
  if (m < 0 || i < 0 || (i % 8) != 0 || i > 65536) {
    snprintf(g_err, sizeof(g_err), "qqq_silu_mul_quant: bad shape m=%d i=%d (i must be a multiple of 8, at most 65536)", m, i);
    return QQQ_ERR_ARG;
  }
  if (ld_gate < i || ld_up < i || (ld_gate % 8) != 0 || (ld_up % 8) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_silu_mul_quant: bad row strides ld_gate=%d ld_up=%d (need >= i=%d and multiples of 8)", ld_gate, ld_up, i);
    return QQQ_ERR_ARG;
  }
  if (!gate || !up || !xq || !s1 || misaligned(gate, 16) || misaligned(up, 16) || (y && misaligned(y, 16)) || misaligned(xq, 8) ||
      misaligned(s1, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_silu_mul_quant: bad argument (gate / up / xq / s1 must be non-NULL; gate, up, y 16-byte, xq 8-byte, "
             "s1 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  return act_launch<SiluMulQuantLaunch>("qqq_silu_mul_quant_kernel launch", m, i, static_cast<hipStream_t>(stream),
                                        static_cast<const _Float16*>(gate), ld_gate, static_cast<const _Float16*>(up), ld_up,
                                        static_cast<_Float16*>(y), static_cast<int8_t*>(xq), static_cast<float*>(s1), i);
}

// ---- RoPE + KV-cache write of an attention block (include/qqq_amd_attn.h; kernel in qqq_attn.hip.h).  Grid x = token, grid y = blocks of
// ROPE_NT (head, 16-byte pair) items: at decode a Llama-2-7B layer (96 heads of 128) spreads over 6 workgroups instead of one.
static constexpr int ROPE_NT = 128;

extern "C" int qqq_rope_qkv(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                            int table_len, const void* pos, void* q_out, void* k_cache, void* v_cache, int b, int s, int h, int kvh, int d,
                            int cap, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || s < 0 || h < 0 || kvh < 0 || d < 0 || cap < 0 || table_len < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv: negative size (b=%d s=%d h=%d kvh=%d d=%d cap=%d table_len=%d)", b, s, h, kvh, d, cap,
             table_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0 || s == 0) return QQQ_OK;
  if ((long long)b * s > 0x7fffffffLL || h < 1 || kvh < 1 || h % kvh != 0 || d < 16 || d > 256 || d % 16 != 0 ||
      (long long)(h + 2LL * kvh) * d > (1LL << 20)) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv: bad shape b=%d s=%d h=%d kvh=%d d=%d (need b*s < 2^31, h %% kvh == 0, d a multiple of 16 "
             "in [16, 256], (h + 2 kvh) d <= 2^20)", b, s, h, kvh, d);
    return QQQ_ERR_ARG;
  }
  if (ld_q < h * d || ld_k < kvh * d || ld_v < kvh * d || ld_q % 8 || ld_k % 8 || ld_v % 8) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv: bad row strides ld_q=%d ld_k=%d ld_v=%d (need multiples of 8, >= h*d=%d / kvh*d=%d)", ld_q,
             ld_k, ld_v, h * d, kvh * d);
    return QQQ_ERR_ARG;
  }
  if (!q || !k || !v || !cos || !sin || !pos || !q_out || !k_cache || !v_cache || misaligned(q, 16) || misaligned(k, 16) ||
      misaligned(v, 16) || misaligned(cos, 16) || misaligned(sin, 16) || misaligned(pos, 8) || misaligned(q_out, 16) ||
      misaligned(k_cache, 16) || misaligned(v_cache, 16)) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv: bad argument (every pointer must be non-NULL; fp16 tensors 16-byte, pos 8-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  const int items = (h + 2 * kvh) * (d / 16);
  const long long limit = cap < table_len ? cap : table_len;
  hipLaunchKernelGGL((qqq_rope_qkv_kernel<ROPE_NT>), dim3(b * s, (items + ROPE_NT - 1) / ROPE_NT), dim3(ROPE_NT), 0,
                     static_cast<hipStream_t>(stream), static_cast<const _Float16*>(q), ld_q, static_cast<const _Float16*>(k), ld_k,
                     static_cast<const _Float16*>(v), ld_v, static_cast<const _Float16*>(cos), static_cast<const _Float16*>(sin),
                     static_cast<const long long*>(pos), limit, static_cast<_Float16*>(q_out), static_cast<_Float16*>(k_cache),
                     static_cast<_Float16*>(v_cache), s, h, kvh, d, cap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_rope_qkv_kernel launch");
  return QQQ_OK;
}

// ---- split-K decode attention (include/qqq_amd_decode.h; kernels in qqq_decode.hip.h).  Split count: about four 4-wave workgroups per
// CU over all (row, KV head) pairs -- the 16 waves a CU holds at the split kernel's 4 waves per SIMD, each with one 16 KB K/V block in
// flight -- at most DEC_MAX_SPLITS and one per DEC_ROUND keys of max_len; the workspace is sized for the bound alone, so it does not
// depend on the device.
static constexpr int DEC_MAX_SPLITS = 32;

static int decode_split_bound(int max_len) {
  const int by_len = (max_len + DEC_ROUND - 1) / DEC_ROUND;
  return by_len < DEC_MAX_SPLITS ? by_len : DEC_MAX_SPLITS;
}

static const char* decode_shape_error(int b, int h, int kvh, int d, int max_len) {
  if (b < 0 || h < 1 || kvh < 1 || h % kvh != 0 || h / kvh > DEC_GMAX || (d != 64 && d != 128) || (long long)h * d > 16384 ||
      b > 65535 || max_len < 1)
    return "bad shape";
  return nullptr;
}

extern "C" size_t qqq_decode_attn_workspace_bytes(int b, int h, int kvh, int d, int max_len) {
  if (b == 0 || decode_shape_error(b, h, kvh, d, max_len)) return 0;
  return (size_t)b * h * decode_split_bound(max_len) * (size_t)(d + 2) * sizeof(float);
}

template <int VPT>
static void decode_combine(int b, hipStream_t st, const float* wo, const float* wml, const long long* pos, long long limit, _Float16* o16,
                           int8_t* xq, float* s1, int h, int d, int chunk, int splits) {
  hipLaunchKernelGGL((qqq_decode_combine_kernel<VPT, DEC_COMBINE_NT>), dim3(b), dim3(DEC_COMBINE_NT), 0, st, wo, wml, pos, limit, o16, xq,
                     s1, h, d, chunk, splits);
}

// splits and keys per split of a call: the same for the fp16 and the int8 cache
static void decode_split_plan(int dev, int b, int kvh, int max_len, int* splits_out, int* chunk_out) {
  const int bk = b * kvh;
  int splits = (4 * device_cus_of(dev) + bk - 1) / bk;
  const int bound = decode_split_bound(max_len);
  splits = splits < 1 ? 1 : (splits > bound ? bound : splits);
  const int per = (max_len + splits - 1) / splits;
  const int chunk = (per + DEC_ROUND - 1) / DEC_ROUND * DEC_ROUND;
  *splits_out = (max_len + chunk - 1) / chunk;
  *chunk_out = chunk;
}

static int decode_combine_launch(int b, hipStream_t st, const float* wo, const float* wml, const long long* pp, long long limit, void* o_fp16,
                                 void* xq, void* s1, int h, int d, int chunk, int splits) {
  _Float16* o16 = static_cast<_Float16*>(o_fp16);
  int8_t* xqp = static_cast<int8_t*>(xq);
  float* s1p = static_cast<float*>(s1);
  const int nvec = h * d / 8;
  if (nvec <= DEC_COMBINE_NT)
    decode_combine<1>(b, st, wo, wml, pp, limit, o16, xqp, s1p, h, d, chunk, splits);
  else if (nvec <= 2 * DEC_COMBINE_NT)
    decode_combine<2>(b, st, wo, wml, pp, limit, o16, xqp, s1p, h, d, chunk, splits);
  else
    decode_combine<4>(b, st, wo, wml, pp, limit, o16, xqp, s1p, h, d, chunk, splits);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_decode_combine_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_decode_attn(const void* q, const void* k_cache, const void* v_cache, const void* pos, float scale, void* o_fp16, void* xq,
                               void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int cap, int max_len, int dev,
                               void* stream) {
  g_err[0] = 0;
  if (b < 0 || h < 0 || kvh < 0 || d < 0 || cap < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn: negative size (b=%d h=%d kvh=%d d=%d cap=%d max_len=%d)", b, h, kvh, d, cap, max_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0) return QQQ_OK;
  if (decode_shape_error(b, h, kvh, d, max_len) || max_len > cap) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn: bad shape b=%d h=%d kvh=%d d=%d cap=%d max_len=%d (need h %% kvh == 0, h / kvh <= %d, "
             "d 64 or 128, h*d <= 16384, b <= 65535, 1 <= max_len <= cap)", b, h, kvh, d, cap, max_len, DEC_GMAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn: no output (o_fp16 and xq / s1 are all NULL)");
    return QQQ_ERR_ARG;
  }
  if (!q || !k_cache || !v_cache || !pos || !workspace || (!xq) != (!s1) || misaligned(q, 16) || misaligned(k_cache, 16) ||
      misaligned(v_cache, 16) || misaligned(pos, 8) || misaligned(workspace, 16) || (o_fp16 && misaligned(o_fp16, 16)) ||
      (xq && misaligned(xq, 8)) || (s1 && misaligned(s1, 4))) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn: bad argument (q / caches / pos / workspace must be non-NULL, xq and s1 both given or "
             "both NULL; q, caches, o_fp16, workspace 16-byte, pos / xq 8-byte, s1 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn: workspace of %zu bytes, need %zu", workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int splits, chunk;
  decode_split_plan(dev, b, kvh, max_len, &splits, &chunk);
  float* wo = static_cast<float*>(workspace);
  float* wml = wo + (size_t)b * h * splits * d;
  const long long* pp = static_cast<const long long*>(pos);
  const long long limit = max_len;  // <= cap
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const _Float16* kp = static_cast<const _Float16*>(k_cache);
  const _Float16* vp = static_cast<const _Float16*>(v_cache);
  if (d == 64)
    hipLaunchKernelGGL((qqq_decode_split_kernel<64>), dim3(splits, kvh, b), dim3(DEC_WAVES * 64), 0, st, qp, kp, vp, pp, limit, scale_log2,
                       wo, wml, h, kvh, cap, chunk, splits);
  else
    hipLaunchKernelGGL((qqq_decode_split_kernel<128>), dim3(splits, kvh, b), dim3(DEC_WAVES * 64), 0, st, qp, kp, vp, pp, limit, scale_log2,
                       wo, wml, h, kvh, cap, chunk, splits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_decode_split_kernel launch");
  return decode_combine_launch(b, st, wo, wml, pp, limit, o_fp16, xq, s1, h, d, chunk, splits);
}

// ---- the int8 KV cache (include/qqq_amd_kv8.h; kernels in qqq_kv8.hip.h): qqq_rope_qkv's and qqq_decode_attn's launches with the
// quantising / int8-reading kernels; the decode call ends in the same combine kernel.
extern "C" int qqq_rope_qkv_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                                int table_len, const void* pos, void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                                int b, int s, int h, int kvh, int d, int cap, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || s < 0 || h < 0 || kvh < 0 || d < 0 || cap < 0 || table_len < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv_kv8: negative size (b=%d s=%d h=%d kvh=%d d=%d cap=%d table_len=%d)", b, s, h, kvh, d, cap,
             table_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0 || s == 0) return QQQ_OK;
  if ((long long)b * s > 0x7fffffffLL || h < 1 || kvh < 1 || h % kvh != 0 || (d != 64 && d != 128) ||
      (long long)(h + 2LL * kvh) * d > (1LL << 20)) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv_kv8: bad shape b=%d s=%d h=%d kvh=%d d=%d (need b*s < 2^31, h %% kvh == 0, d 64 or 128, "
             "(h + 2 kvh) d <= 2^20)", b, s, h, kvh, d);
    return QQQ_ERR_ARG;
  }
  if (ld_q < h * d || ld_k < kvh * d || ld_v < kvh * d || ld_q % 8 || ld_k % 8 || ld_v % 8) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv_kv8: bad row strides ld_q=%d ld_k=%d ld_v=%d (need multiples of 8, >= h*d=%d / kvh*d=%d)",
             ld_q, ld_k, ld_v, h * d, kvh * d);
    return QQQ_ERR_ARG;
  }
  if (!q || !k || !v || !cos || !sin || !pos || !q_out || !k_cache || !v_cache || !k_scale || !v_scale || misaligned(q, 16) ||
      misaligned(k, 16) || misaligned(v, 16) || misaligned(cos, 16) || misaligned(sin, 16) || misaligned(pos, 8) || misaligned(q_out, 16) ||
      misaligned(k_cache, 16) || misaligned(v_cache, 16) || misaligned(k_scale, 4) || misaligned(v_scale, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_rope_qkv_kv8: bad argument (every pointer must be non-NULL; fp16 tensors and the caches 16-byte, pos "
             "8-byte, the scales 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  const int items = (h + 2 * kvh) * (d / 16);
  const long long limit = cap < table_len ? cap : table_len;
  hipLaunchKernelGGL((qqq_kv8_rope_qkv_kernel<ROPE_NT>), dim3(b * s, (items + ROPE_NT - 1) / ROPE_NT), dim3(ROPE_NT), 0,
                     static_cast<hipStream_t>(stream), static_cast<const _Float16*>(q), ld_q, static_cast<const _Float16*>(k), ld_k,
                     static_cast<const _Float16*>(v), ld_v, static_cast<const _Float16*>(cos), static_cast<const _Float16*>(sin),
                     static_cast<const long long*>(pos), limit, static_cast<_Float16*>(q_out), static_cast<int8_t*>(k_cache),
                     static_cast<int8_t*>(v_cache), static_cast<float*>(k_scale), static_cast<float*>(v_scale), s, h, kvh, d, cap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_kv8_rope_qkv_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_decode_attn_kv8(const void* q, const void* k_cache, const void* v_cache, const void* k_scale, const void* v_scale,
                                   const void* pos, float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes,
                                   int b, int h, int kvh, int d, int cap, int max_len, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || h < 0 || kvh < 0 || d < 0 || cap < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_kv8: negative size (b=%d h=%d kvh=%d d=%d cap=%d max_len=%d)", b, h, kvh, d, cap,
             max_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0) return QQQ_OK;
  if (decode_shape_error(b, h, kvh, d, max_len) || max_len > cap) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_kv8: bad shape b=%d h=%d kvh=%d d=%d cap=%d max_len=%d (need h %% kvh == 0, h / kvh <= "
             "%d, d 64 or 128, h*d <= 16384, b <= 65535, 1 <= max_len <= cap)", b, h, kvh, d, cap, max_len, DEC_GMAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_kv8: no output (o_fp16 and xq / s1 are all NULL)");
    return QQQ_ERR_ARG;
  }
  if (!q || !k_cache || !v_cache || !k_scale || !v_scale || !pos || !workspace || (!xq) != (!s1) || misaligned(q, 16) ||
      misaligned(k_cache, 16) || misaligned(v_cache, 16) || misaligned(k_scale, 4) || misaligned(v_scale, 4) || misaligned(pos, 8) ||
      misaligned(workspace, 16) || (o_fp16 && misaligned(o_fp16, 16)) || (xq && misaligned(xq, 8)) || (s1 && misaligned(s1, 4))) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_kv8: bad argument (q / caches / scales / pos / workspace must be non-NULL, xq and s1 both "
             "given or both NULL; q, caches, o_fp16, workspace 16-byte, pos / xq 8-byte, s1 and the scales 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_kv8: workspace of %zu bytes, need %zu", workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int splits, chunk;
  decode_split_plan(dev, b, kvh, max_len, &splits, &chunk);
  float* wo = static_cast<float*>(workspace);
  float* wml = wo + (size_t)b * h * splits * d;
  const long long* pp = static_cast<const long long*>(pos);
  const long long limit = max_len;  // <= cap
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const int8_t* kp = static_cast<const int8_t*>(k_cache);
  const int8_t* vp = static_cast<const int8_t*>(v_cache);
  const float* ksp = static_cast<const float*>(k_scale);
  const float* vsp = static_cast<const float*>(v_scale);
  if (d == 64)
    hipLaunchKernelGGL((qqq_kv8_decode_split_kernel<64>), dim3(splits, kvh, b), dim3(DEC_WAVES * 64), 0, st, qp, kp, vp, ksp, vsp, pp, limit,
                       scale_log2, wo, wml, h, kvh, cap, chunk, splits);
  else
    hipLaunchKernelGGL((qqq_kv8_decode_split_kernel<128>), dim3(splits, kvh, b), dim3(DEC_WAVES * 64), 0, st, qp, kp, vp, ksp, vsp, pp, limit,
                       scale_log2, wo, wml, h, kvh, cap, chunk, splits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_kv8_decode_split_kernel launch");
  return decode_combine_launch(b, st, wo, wml, pp, limit, o_fp16, xq, s1, h, d, chunk, splits);
}

// ---- the block-table (paged) KV cache (include/qqq_amd_paged.h; kernels in qqq_paged.hip.h): the four launches above with a slot per
// token / a block table per row in place of the contiguous caches' (row, position) addresses.  One body per pair; `name` is the entry
// point's, kv8 selects the int8 pool with its scales.
static int paged_log2_block(int block_size) {  // log2 of a power of two in [16, 256], -1 otherwise
  for (int l = 4; l <= 8; ++l)
    if (block_size == (1 << l)) return l;
  return -1;
}

static int rope_qkv_paged(const char* name, bool kv8, const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v,
                          const void* cos, const void* sin, int table_len, const void* pos, const void* slots, void* q_out, void* k_pool,
                          void* v_pool, void* k_scale, void* v_scale, int m, int h, int kvh, int d, int num_blocks, int block_size, int dev,
                          void* stream) {
  g_err[0] = 0;
  if (m < 0 || h < 0 || kvh < 0 || d < 0 || num_blocks < 0 || block_size < 0 || table_len < 0) {
    snprintf(g_err, sizeof(g_err), "%s: negative size (m=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_len=%d)", name, m, h, kvh, d,
             num_blocks, block_size, table_len);
    return QQQ_ERR_ARG;
  }
  if (m == 0) return QQQ_OK;
  const int lbs = paged_log2_block(block_size);
  if (h < 1 || kvh < 1 || h % kvh != 0 || (d != 64 && d != 128) || (long long)(h + 2LL * kvh) * d > (1LL << 20) || lbs < 0 ||
      num_blocks < 1 || (long long)num_blocks * block_size > 0x7fffffffLL) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape m=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d (need h %% kvh == 0, d 64 or 128, "
             "(h + 2 kvh) d <= 2^20, block_size a power of two in [16, 256], num_blocks >= 1, num_blocks * block_size < 2^31)", name, m, h,
             kvh, d, num_blocks, block_size);
    return QQQ_ERR_ARG;
  }
  if (ld_q < h * d || ld_k < kvh * d || ld_v < kvh * d || ld_q % 8 || ld_k % 8 || ld_v % 8) {
    snprintf(g_err, sizeof(g_err), "%s: bad row strides ld_q=%d ld_k=%d ld_v=%d (need multiples of 8, >= h*d=%d / kvh*d=%d)", name, ld_q,
             ld_k, ld_v, h * d, kvh * d);
    return QQQ_ERR_ARG;
  }
  if (!q || !k || !v || !cos || !sin || !pos || !slots || !q_out || !k_pool || !v_pool || misaligned(q, 16) || misaligned(k, 16) ||
      misaligned(v, 16) || misaligned(cos, 16) || misaligned(sin, 16) || misaligned(pos, 8) || misaligned(slots, 8) ||
      misaligned(q_out, 16) || misaligned(k_pool, 16) || misaligned(v_pool, 16) ||
      (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (every pointer must be non-NULL; fp16 tensors and the pools 16-byte, pos / slots "
             "8-byte, the scales 4-byte aligned)", name);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  const int items = (h + 2 * kvh) * (d / 16);
  const dim3 grid(m, (items + ROPE_NT - 1) / ROPE_NT);
  const long long limit = table_len, nslots = (long long)num_blocks * block_size;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const _Float16 *qp = static_cast<const _Float16*>(q), *kp = static_cast<const _Float16*>(k), *vp = static_cast<const _Float16*>(v);
  const _Float16 *cp = static_cast<const _Float16*>(cos), *sp = static_cast<const _Float16*>(sin);
  const long long *pp = static_cast<const long long*>(pos), *slp = static_cast<const long long*>(slots);
  if (kv8)
    hipLaunchKernelGGL((qqq_paged_kv8_rope_qkv_kernel<ROPE_NT>), grid, dim3(ROPE_NT), 0, st, qp, ld_q, kp, ld_k, vp, ld_v, cp, sp, pp, limit,
                       slp, nslots, static_cast<_Float16*>(q_out), static_cast<int8_t*>(k_pool), static_cast<int8_t*>(v_pool),
                       static_cast<float*>(k_scale), static_cast<float*>(v_scale), h, kvh, d, lbs);
  else
    hipLaunchKernelGGL((qqq_paged_rope_qkv_kernel<ROPE_NT>), grid, dim3(ROPE_NT), 0, st, qp, ld_q, kp, ld_k, vp, ld_v, cp, sp, pp, limit, slp,
                       nslots, static_cast<_Float16*>(q_out), static_cast<_Float16*>(k_pool), static_cast<_Float16*>(v_pool), h, kvh, d, lbs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, kv8 ? "qqq_paged_kv8_rope_qkv_kernel launch" : "qqq_paged_rope_qkv_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_rope_qkv_paged(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                                  int table_len, const void* pos, const void* slots, void* q_out, void* k_pool, void* v_pool, int m, int h,
                                  int kvh, int d, int num_blocks, int block_size, int dev, void* stream) {
  return rope_qkv_paged("qqq_rope_qkv_paged", false, q, ld_q, k, ld_k, v, ld_v, cos, sin, table_len, pos, slots, q_out, k_pool, v_pool,
                        nullptr, nullptr, m, h, kvh, d, num_blocks, block_size, dev, stream);
}

extern "C" int qqq_rope_qkv_paged_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos,
                                      const void* sin, int table_len, const void* pos, const void* slots, void* q_out, void* k_pool,
                                      void* v_pool, void* k_scale, void* v_scale, int m, int h, int kvh, int d, int num_blocks,
                                      int block_size, int dev, void* stream) {
  return rope_qkv_paged("qqq_rope_qkv_paged_kv8", true, q, ld_q, k, ld_k, v, ld_v, cos, sin, table_len, pos, slots, q_out, k_pool, v_pool,
                        k_scale, v_scale, m, h, kvh, d, num_blocks, block_size, dev, stream);
}

// ---- Qwen3's per-head q / k RMSNorm in front of the rotation (include_ops/qqq_amd_qknorm.h; kernel in qqq_qknorm.hip.h): the four RoPE /
// cache-write launches above with one kernel template of their own.  One body for the four; `name` is the entry point's.  The static
// cache comes as (b, s, cap) with slots = nullptr, the pool as (m, num_blocks, block_size) with b = m, s = 1.
static int rope_qkv_norm(const char* name, bool paged, bool kv8, const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v,
                         const void* q_weight, const void* k_weight, float eps, const void* cos, const void* sin, int table_len,
                         const void* pos, const void* slots, void* q_out, void* k_dst, void* v_dst, void* k_scale, void* v_scale, int b,
                         int s, int h, int kvh, int d, int cap, int num_blocks, int block_size, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || s < 0 || h < 0 || kvh < 0 || d < 0 || cap < 0 || num_blocks < 0 || block_size < 0 || table_len < 0) {
    if (paged)
      snprintf(g_err, sizeof(g_err), "%s: negative size (m=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_len=%d)", name, b, h, kvh,
               d, num_blocks, block_size, table_len);
    else
      snprintf(g_err, sizeof(g_err), "%s: negative size (b=%d s=%d h=%d kvh=%d d=%d cap=%d table_len=%d)", name, b, s, h, kvh, d, cap,
               table_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0 || s == 0) return QQQ_OK;
  const int lbs = paged ? paged_log2_block(block_size) : 0;
  if ((long long)b * s > 0x7fffffffLL || h < 1 || kvh < 1 || h % kvh != 0 || (d != 64 && d != 128) ||
      (long long)(h + 2LL * kvh) * d > (1LL << 20) ||
      (paged && (lbs < 0 || num_blocks < 1 || (long long)num_blocks * block_size > 0x7fffffffLL))) {
    if (paged)
      snprintf(g_err, sizeof(g_err), "%s: bad shape m=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d (need h %% kvh == 0, d 64 or 128, "
               "(h + 2 kvh) d <= 2^20, block_size a power of two in [16, 256], num_blocks >= 1, num_blocks * block_size < 2^31)", name, b,
               h, kvh, d, num_blocks, block_size);
    else
      snprintf(g_err, sizeof(g_err), "%s: bad shape b=%d s=%d h=%d kvh=%d d=%d (need b*s < 2^31, h %% kvh == 0, d 64 or 128, "
               "(h + 2 kvh) d <= 2^20)", name, b, s, h, kvh, d);
    return QQQ_ERR_ARG;
  }
  if (ld_q < h * d || ld_k < kvh * d || ld_v < kvh * d || ld_q % 8 || ld_k % 8 || ld_v % 8) {
    snprintf(g_err, sizeof(g_err), "%s: bad row strides ld_q=%d ld_k=%d ld_v=%d (need multiples of 8, >= h*d=%d / kvh*d=%d)", name, ld_q,
             ld_k, ld_v, h * d, kvh * d);
    return QQQ_ERR_ARG;
  }
  if (!(eps >= 0.f) || eps > 3.0e38f) {
    snprintf(g_err, sizeof(g_err), "%s: bad eps %g (need a finite eps >= 0)", name, (double)eps);
    return QQQ_ERR_ARG;
  }
  if (!q || !k || !v || !q_weight || !k_weight || !cos || !sin || !pos || (paged && !slots) || !q_out || !k_dst || !v_dst ||
      misaligned(q, 16) || misaligned(k, 16) || misaligned(v, 16) || misaligned(q_weight, 16) || misaligned(k_weight, 16) ||
      misaligned(cos, 16) || misaligned(sin, 16) || misaligned(pos, 8) || (paged && misaligned(slots, 8)) || misaligned(q_out, 16) ||
      misaligned(k_dst, 16) || misaligned(v_dst, 16) ||
      (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (every pointer must be non-NULL; fp16 tensors, the norm weights and the %s 16-byte, "
             "pos%s 8-byte, the scales 4-byte aligned)", name, paged ? "pools" : "caches", paged ? " / slots" : "");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  const int items = (h + 2 * kvh) * (d / 16);
  const dim3 grid(b * s, (items + ROPE_NT - 1) / ROPE_NT);
  const long long limit = paged ? table_len : (cap < table_len ? cap : table_len);
  const long long nslots = (long long)num_blocks * block_size;
  const int where = paged ? lbs : cap;
  hipStream_t st = static_cast<hipStream_t>(stream);
#define QQQ_QKNORM_LAUNCH(PAGED, KV8)                                                                                                      \
  hipLaunchKernelGGL((qqq_rope_qkv_norm_kernel<ROPE_NT, PAGED, KV8>), grid, dim3(ROPE_NT), 0, st, static_cast<const _Float16*>(q), ld_q,   \
                     static_cast<const _Float16*>(k), ld_k, static_cast<const _Float16*>(v), ld_v,                                         \
                     static_cast<const _Float16*>(q_weight), static_cast<const _Float16*>(k_weight), eps,                                  \
                     static_cast<const _Float16*>(cos), static_cast<const _Float16*>(sin), static_cast<const long long*>(pos), limit,      \
                     static_cast<const long long*>(slots), nslots, static_cast<_Float16*>(q_out), k_dst, v_dst,                            \
                     static_cast<float*>(k_scale), static_cast<float*>(v_scale), s, h, kvh, d, where)
  if (paged && kv8)
    QQQ_QKNORM_LAUNCH(true, true);
  else if (paged)
    QQQ_QKNORM_LAUNCH(true, false);
  else if (kv8)
    QQQ_QKNORM_LAUNCH(false, true);
  else
    QQQ_QKNORM_LAUNCH(false, false);
#undef QQQ_QKNORM_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_rope_qkv_norm_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_rope_qkv_norm(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                                 const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos,
                                 void* q_out, void* k_cache, void* v_cache, int b, int s, int h, int kvh, int d, int cap, int dev,
                                 void* stream) {
  return rope_qkv_norm("qqq_rope_qkv_norm", false, false, q, ld_q, k, ld_k, v, ld_v, q_weight, k_weight, eps, cos, sin, table_len, pos,
                       nullptr, q_out, k_cache, v_cache, nullptr, nullptr, b, s, h, kvh, d, cap, 0, 0, dev, stream);
}

extern "C" int qqq_rope_qkv_norm_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                                     const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos,
                                     void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale, int b, int s, int h, int kvh,
                                     int d, int cap, int dev, void* stream) {
  return rope_qkv_norm("qqq_rope_qkv_norm_kv8", false, true, q, ld_q, k, ld_k, v, ld_v, q_weight, k_weight, eps, cos, sin, table_len, pos,
                       nullptr, q_out, k_cache, v_cache, k_scale, v_scale, b, s, h, kvh, d, cap, 0, 0, dev, stream);
}

extern "C" int qqq_rope_qkv_norm_paged(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                                       const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos,
                                       const void* slots, void* q_out, void* k_pool, void* v_pool, int m, int h, int kvh, int d,
                                       int num_blocks, int block_size, int dev, void* stream) {
  return rope_qkv_norm("qqq_rope_qkv_norm_paged", true, false, q, ld_q, k, ld_k, v, ld_v, q_weight, k_weight, eps, cos, sin, table_len,
                       pos, slots, q_out, k_pool, v_pool, nullptr, nullptr, m, 1, h, kvh, d, 0, num_blocks, block_size, dev, stream);
}

extern "C" int qqq_rope_qkv_norm_paged_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                                           const void* k_weight, float eps, const void* cos, const void* sin, int table_len,
                                           const void* pos, const void* slots, void* q_out, void* k_pool, void* v_pool, void* k_scale,
                                           void* v_scale, int m, int h, int kvh, int d, int num_blocks, int block_size, int dev,
                                           void* stream) {
  return rope_qkv_norm("qqq_rope_qkv_norm_paged_kv8", true, true, q, ld_q, k, ld_k, v, ld_v, q_weight, k_weight, eps, cos, sin, table_len,
                       pos, slots, q_out, k_pool, v_pool, k_scale, v_scale, m, 1, h, kvh, d, 0, num_blocks, block_size, dev, stream);
}

static int decode_attn_paged(const char* name, bool kv8, const void* q, const void* k_pool, const void* v_pool, const void* k_scale,
                             const void* v_scale, const void* block_table, int table_stride, const void* pos, float scale, void* o_fp16,
                             void* xq, void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks,
                             int block_size, int max_len, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || h < 0 || kvh < 0 || d < 0 || num_blocks < 0 || block_size < 0 || table_stride < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "%s: negative size (b=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d)", name,
             b, h, kvh, d, num_blocks, block_size, table_stride, max_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0) return QQQ_OK;
  const int lbs = paged_log2_block(block_size);
  if (decode_shape_error(b, h, kvh, d, max_len) || lbs < 0 || num_blocks < 1 || (long long)num_blocks * block_size > 0x7fffffffLL ||
      table_stride < 1 || max_len > (long long)table_stride * block_size) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape b=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d (need "
             "h %% kvh == 0, h / kvh <= %d, d 64 or 128, h*d <= 16384, b <= 65535, block_size a power of two in [16, 256], num_blocks >= 1, "
             "num_blocks * block_size < 2^31, 1 <= max_len <= table_stride * block_size)", name, b, h, kvh, d, num_blocks, block_size,
             table_stride, max_len, DEC_GMAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "%s: no output (o_fp16 and xq / s1 are all NULL)", name);
    return QQQ_ERR_ARG;
  }
  if (!q || !k_pool || !v_pool || !block_table || !pos || !workspace || (!xq) != (!s1) || misaligned(q, 16) || misaligned(k_pool, 16) ||
      misaligned(v_pool, 16) || misaligned(block_table, 4) || misaligned(pos, 8) || misaligned(workspace, 16) ||
      (o_fp16 && misaligned(o_fp16, 16)) || (xq && misaligned(xq, 8)) || (s1 && misaligned(s1, 4)) ||
      (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (q / pools / scales / block_table / pos / workspace must be non-NULL, xq and s1 both "
             "given or both NULL; q, pools, o_fp16, workspace 16-byte, pos / xq 8-byte, block_table, s1 and the scales 4-byte aligned)", name);
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "%s: workspace of %zu bytes, need %zu", name, workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int splits, chunk;
  decode_split_plan(dev, b, kvh, max_len, &splits, &chunk);
  float* wo = static_cast<float*>(workspace);
  float* wml = wo + (size_t)b * h * splits * d;
  const long long* pp = static_cast<const long long*>(pos);
  const long long limit = max_len;  // <= table_stride * block_size
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const int* tp = static_cast<const int*>(block_table);
  const dim3 grid(splits, kvh, b), block(DEC_WAVES * 64);
  if (kv8) {
    const int8_t *kp = static_cast<const int8_t*>(k_pool), *vp = static_cast<const int8_t*>(v_pool);
    const float *ksp = static_cast<const float*>(k_scale), *vsp = static_cast<const float*>(v_scale);
    if (d == 64)
      hipLaunchKernelGGL((qqq_paged_kv8_decode_split_kernel<64>), grid, block, 0, st, qp, kp, vp, ksp, vsp, tp, table_stride, pp, limit,
                         scale_log2, wo, wml, h, kvh, num_blocks, lbs, chunk, splits);
    else
      hipLaunchKernelGGL((qqq_paged_kv8_decode_split_kernel<128>), grid, block, 0, st, qp, kp, vp, ksp, vsp, tp, table_stride, pp, limit,
                         scale_log2, wo, wml, h, kvh, num_blocks, lbs, chunk, splits);
  } else {
    const _Float16 *kp = static_cast<const _Float16*>(k_pool), *vp = static_cast<const _Float16*>(v_pool);
    if (d == 64)
      hipLaunchKernelGGL((qqq_paged_decode_split_kernel<64>), grid, block, 0, st, qp, kp, vp, tp, table_stride, pp, limit, scale_log2, wo,
                         wml, h, kvh, num_blocks, lbs, chunk, splits);
    else
      hipLaunchKernelGGL((qqq_paged_decode_split_kernel<128>), grid, block, 0, st, qp, kp, vp, tp, table_stride, pp, limit, scale_log2, wo,
                         wml, h, kvh, num_blocks, lbs, chunk, splits);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, kv8 ? "qqq_paged_kv8_decode_split_kernel launch" : "qqq_paged_decode_split_kernel launch");
  return decode_combine_launch(b, st, wo, wml, pp, limit, o_fp16, xq, s1, h, d, chunk, splits);
}

extern "C" int qqq_decode_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                     const void* pos, float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes,
                                     int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int dev, void* stream) {
  return decode_attn_paged("qqq_decode_attn_paged", false, q, k_pool, v_pool, nullptr, nullptr, block_table, table_stride, pos, scale, o_fp16,
                           xq, s1, workspace, workspace_bytes, b, h, kvh, d, num_blocks, block_size, max_len, dev, stream);
}

extern "C" int qqq_decode_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                         const void* block_table, int table_stride, const void* pos, float scale, void* o_fp16, void* xq,
                                         void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks,
                                         int block_size, int max_len, int dev, void* stream) {
  return decode_attn_paged("qqq_decode_attn_paged_kv8", true, q, k_pool, v_pool, k_scale, v_scale, block_table, table_stride, pos, scale,
                           o_fp16, xq, s1, workspace, workspace_bytes, b, h, kvh, d, num_blocks, block_size, max_len, dev, stream);
}

// ---- the verify chunk's attention (include/qqq_amd_verify.h; kernels in qqq_verify.hip.h): decode_attn_paged's two launches for t tokens
// per batch row.  One body for the pair; `name` is the entry point's.
extern "C" size_t qqq_verify_attn_workspace_bytes(int b, int t, int h, int kvh, int d, int max_len) {
  if (b < 0 || t < 1 || t > VER_TMAX || (long long)b * t > 65535) return 0;
  return qqq_decode_attn_workspace_bytes(b * t, h, kvh, d, max_len);
}

template <int VPT>
static void verify_combine(int rows, hipStream_t st, const float* wo, const float* wml, const long long* start, long long limit, int t,
                           _Float16* o16, int8_t* xq, float* s1, int h, int d, int chunk, int splits) {
  hipLaunchKernelGGL((qqq_verify_combine_kernel<VPT, DEC_COMBINE_NT>), dim3(rows), dim3(DEC_COMBINE_NT), 0, st, wo, wml, start, limit, t,
                     o16, xq, s1, h, d, chunk, splits);
}

template <int D, int NQ, typename... Args>
static void verify_split(bool kv8, dim3 grid, hipStream_t st, const _Float16* q, const void* k_pool, const void* v_pool, const void* k_scale,
                         const void* v_scale, Args... rest) {
  if (kv8)
    hipLaunchKernelGGL((qqq_verify_kv8_split_kernel<D, NQ>), grid, dim3(DEC_WAVES * 64), 0, st, q, static_cast<const int8_t*>(k_pool),
                       static_cast<const int8_t*>(v_pool), static_cast<const float*>(k_scale), static_cast<const float*>(v_scale), rest...);
  else
    hipLaunchKernelGGL((qqq_verify_split_kernel<D, NQ>), grid, dim3(DEC_WAVES * 64), 0, st, q, static_cast<const _Float16*>(k_pool),
                       static_cast<const _Float16*>(v_pool), rest...);
}

template <int D, typename... Args>
static void verify_split_tiles(int rows, Args... args) {
  if (rows <= 16)
    verify_split<D, 1>(args...);
  else if (rows <= 32)
    verify_split<D, 2>(args...);
  else
    verify_split<D, 4>(args...);
}

static int verify_attn_paged(const char* name, bool kv8, const void* q, const void* k_pool, const void* v_pool, const void* k_scale,
                             const void* v_scale, const void* block_table, int table_stride, const void* start, float scale, void* o_fp16,
                             void* xq, void* s1, void* workspace, size_t workspace_bytes, int b, int t, int h, int kvh, int d,
                             int num_blocks, int block_size, int max_len, int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || t < 0 || h < 0 || kvh < 0 || d < 0 || num_blocks < 0 || block_size < 0 || table_stride < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "%s: negative size (b=%d t=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d)",
             name, b, t, h, kvh, d, num_blocks, block_size, table_stride, max_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0) return QQQ_OK;
  const int lbs = paged_log2_block(block_size);
  if (decode_shape_error(b, h, kvh, d, max_len) || t < 1 || t > VER_TMAX || (h / kvh) * t > VER_ROWS_MAX || (long long)b * t > 65535 ||
      lbs < 0 || num_blocks < 1 || (long long)num_blocks * block_size > 0x7fffffffLL || table_stride < 1 ||
      max_len > (long long)table_stride * block_size) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape b=%d t=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d (need "
             "h %% kvh == 0, h / kvh <= %d, d 64 or 128, h*d <= 16384, 1 <= t <= %d, (h / kvh) * t <= %d, b * t <= 65535, block_size a power "
             "of two in [16, 256], num_blocks >= 1, num_blocks * block_size < 2^31, 1 <= max_len <= table_stride * block_size)", name, b, t,
             h, kvh, d, num_blocks, block_size, table_stride, max_len, DEC_GMAX, VER_TMAX, VER_ROWS_MAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "%s: no output (o_fp16 and xq / s1 are all NULL)", name);
    return QQQ_ERR_ARG;
  }
  if (!q || !k_pool || !v_pool || !block_table || !start || !workspace || (!xq) != (!s1) || misaligned(q, 16) || misaligned(k_pool, 16) ||
      misaligned(v_pool, 16) || misaligned(block_table, 4) || misaligned(start, 8) || misaligned(workspace, 16) ||
      (o_fp16 && misaligned(o_fp16, 16)) || (xq && misaligned(xq, 8)) || (s1 && misaligned(s1, 4)) ||
      (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (q / pools / scales / block_table / start / workspace must be non-NULL, xq and s1 both "
             "given or both NULL; q, pools, o_fp16, workspace 16-byte, start / xq 8-byte, block_table, s1 and the scales 4-byte aligned)",
             name);
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, max_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "%s: workspace of %zu bytes, need %zu", name, workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int splits, chunk;
  decode_split_plan(dev, b, kvh, max_len, &splits, &chunk);  // b batch rows: the plan of the decode call each token is compared with
  const int rows = b * t;
  float* wo = static_cast<float*>(workspace);
  float* wml = wo + (size_t)rows * h * splits * d;
  const long long* sp = static_cast<const long long*>(start);
  const long long limit = max_len;  // <= table_stride * block_size
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const int* tp = static_cast<const int*>(block_table);
  const dim3 grid(splits, kvh, b);
  if (d == 64)
    verify_split_tiles<64>((h / kvh) * t, kv8, grid, st, qp, k_pool, v_pool, k_scale, v_scale, tp, table_stride, sp, limit, scale_log2, wo,
                           wml, h, kvh, t, num_blocks, lbs, chunk, splits);
  else
    verify_split_tiles<128>((h / kvh) * t, kv8, grid, st, qp, k_pool, v_pool, k_scale, v_scale, tp, table_stride, sp, limit, scale_log2, wo,
                            wml, h, kvh, t, num_blocks, lbs, chunk, splits);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, kv8 ? "qqq_verify_kv8_split_kernel launch" : "qqq_verify_split_kernel launch");
  _Float16* o16 = static_cast<_Float16*>(o_fp16);
  int8_t* xqp = static_cast<int8_t*>(xq);
  float* s1p = static_cast<float*>(s1);
  const int nvec = h * d / 8;
  if (nvec <= DEC_COMBINE_NT)
    verify_combine<1>(rows, st, wo, wml, sp, limit, t, o16, xqp, s1p, h, d, chunk, splits);
  else if (nvec <= 2 * DEC_COMBINE_NT)
    verify_combine<2>(rows, st, wo, wml, sp, limit, t, o16, xqp, s1p, h, d, chunk, splits);
  else
    verify_combine<4>(rows, st, wo, wml, sp, limit, t, o16, xqp, s1p, h, d, chunk, splits);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_verify_combine_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_verify_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                     const void* start, float scale, void* o_fp16, void* xq, void* s1, void* workspace,
                                     size_t workspace_bytes, int b, int t, int h, int kvh, int d, int num_blocks, int block_size, int max_len,
                                     int dev, void* stream) {
  return verify_attn_paged("qqq_verify_attn_paged", false, q, k_pool, v_pool, nullptr, nullptr, block_table, table_stride, start, scale,
                           o_fp16, xq, s1, workspace, workspace_bytes, b, t, h, kvh, d, num_blocks, block_size, max_len, dev, stream);
}

extern "C" int qqq_verify_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                         const void* block_table, int table_stride, const void* start, float scale, void* o_fp16, void* xq,
                                         void* s1, void* workspace, size_t workspace_bytes, int b, int t, int h, int kvh, int d,
                                         int num_blocks, int block_size, int max_len, int dev, void* stream) {
  return verify_attn_paged("qqq_verify_attn_paged_kv8", true, q, k_pool, v_pool, k_scale, v_scale, block_table, table_stride, start, scale,
                           o_fp16, xq, s1, workspace, workspace_bytes, b, t, h, kvh, d, num_blocks, block_size, max_len, dev, stream);
}

// ---- the decode attention of rows that share a prefix (include/qqq_amd_shared.h; kernels in qqq_shared.hip.h): decode_attn_paged's two
// launches, the first one with the family descriptors.  One body for the pair; `name` is the entry point's.
template <int D, int NQ, typename... Args>
static void shared_split(bool kv8, dim3 grid, hipStream_t st, const _Float16* q, const void* k_pool, const void* v_pool, const void* k_scale,
                         const void* v_scale, Args... rest) {
  if (kv8)
    hipLaunchKernelGGL((qqq_shared_kv8_split_kernel<D, NQ>), grid, dim3(DEC_WAVES * 64), 0, st, q, static_cast<const int8_t*>(k_pool),
                       static_cast<const int8_t*>(v_pool), static_cast<const float*>(k_scale), static_cast<const float*>(v_scale), rest...);
  else
    hipLaunchKernelGGL((qqq_shared_split_kernel<D, NQ>), grid, dim3(DEC_WAVES * 64), 0, st, q, static_cast<const _Float16*>(k_pool),
                       static_cast<const _Float16*>(v_pool), rest...);
}

template <int D, typename... Args>
static void shared_split_tiles(int rows, Args... args) {
  if (rows <= 16)
    shared_split<D, 1>(args...);
  else if (rows <= 32)
    shared_split<D, 2>(args...);
  else
    shared_split<D, 4>(args...);
}

extern "C" int qqq_decode_attn_shared_plan(int b, int h, int kvh, int max_len, int pack, int* splits, int* chunk) {
  g_err[0] = 0;
  if (!splits || !chunk || b < 1 || decode_shape_error(b, h, kvh, 64, max_len) || pack < 1 || (long long)(h / kvh) * pack > SHR_ROWS_MAX) {
    snprintf(g_err, sizeof(g_err), "qqq_decode_attn_shared_plan: bad argument b=%d h=%d kvh=%d max_len=%d pack=%d (need result pointers, "
             "1 <= b <= 65535, h %% kvh == 0, h / kvh <= %d, max_len >= 1, pack >= 1, (h / kvh) * pack <= %d)", b, h, kvh, max_len, pack,
             DEC_GMAX, SHR_ROWS_MAX);
    return QQQ_ERR_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  decode_split_plan(dev, b, kvh, max_len, splits, chunk);
  return QQQ_OK;
}

static int decode_attn_paged_shared(const char* name, bool kv8, const void* q, const void* k_pool, const void* v_pool, const void* k_scale,
                                    const void* v_scale, const void* block_table, int table_stride, const void* pos, const void* family,
                                    const void* shared, int pack, float scale, void* o_fp16, void* xq, void* s1, void* workspace,
                                    size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len,
                                    int dev, void* stream) {
  g_err[0] = 0;
  if (b < 0 || h < 0 || kvh < 0 || d < 0 || num_blocks < 0 || block_size < 0 || table_stride < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "%s: negative size (b=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d)", name,
             b, h, kvh, d, num_blocks, block_size, table_stride, max_len);
    return QQQ_ERR_ARG;
  }
  if (b == 0) return QQQ_OK;
  const int lbs = paged_log2_block(block_size);
  if (decode_shape_error(b, h, kvh, d, max_len) || pack < 1 || (long long)(h / kvh) * pack > SHR_ROWS_MAX || lbs < 0 || num_blocks < 1 ||
      (long long)num_blocks * block_size > 0x7fffffffLL || table_stride < 1 || max_len > (long long)table_stride * block_size) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape b=%d h=%d kvh=%d d=%d pack=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d (need "
             "h %% kvh == 0, h / kvh <= %d, d 64 or 128, h*d <= 16384, b <= 65535, pack >= 1, (h / kvh) * pack <= %d, block_size a power of "
             "two in [16, 256], num_blocks >= 1, num_blocks * block_size < 2^31, 1 <= max_len <= table_stride * block_size)", name, b, h,
             kvh, d, pack, num_blocks, block_size, table_stride, max_len, DEC_GMAX, SHR_ROWS_MAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "%s: no output (o_fp16 and xq / s1 are all NULL)", name);
    return QQQ_ERR_ARG;
  }
  if (!q || !k_pool || !v_pool || !block_table || !pos || !family || !shared || !workspace || (!xq) != (!s1) || misaligned(q, 16) ||
      misaligned(k_pool, 16) || misaligned(v_pool, 16) || misaligned(block_table, 4) || misaligned(pos, 8) || misaligned(family, 4) ||
      misaligned(shared, 8) || misaligned(workspace, 16) || (o_fp16 && misaligned(o_fp16, 16)) || (xq && misaligned(xq, 8)) ||
      (s1 && misaligned(s1, 4)) || (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (q / pools / scales / block_table / pos / family / shared / workspace must be non-NULL, "
             "xq and s1 both given or both NULL; q, pools, o_fp16, workspace 16-byte, pos / shared / xq 8-byte, block_table, family, s1 and "
             "the scales 4-byte aligned)", name);
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "%s: workspace of %zu bytes, need %zu", name, workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  if (pack == 1)  // nothing can be taken jointly: the plain call
    return decode_attn_paged(name, kv8, q, k_pool, v_pool, k_scale, v_scale, block_table, table_stride, pos, scale, o_fp16, xq, s1,
                             workspace, workspace_bytes, b, h, kvh, d, num_blocks, block_size, max_len, dev, stream);
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int splits, chunk;
  decode_split_plan(dev, b, kvh, max_len, &splits, &chunk);
  float* wo = static_cast<float*>(workspace);
  float* wml = wo + (size_t)b * h * splits * d;
  const long long* pp = static_cast<const long long*>(pos);
  const long long limit = max_len;  // <= table_stride * block_size
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const int* tp = static_cast<const int*>(block_table);
  const int* fp = static_cast<const int*>(family);
  const long long* shp = static_cast<const long long*>(shared);
  const dim3 grid(splits, kvh, b);
  if (d == 64)
    shared_split_tiles<64>((h / kvh) * pack, kv8, grid, st, qp, k_pool, v_pool, k_scale, v_scale, tp, table_stride, pp, limit, fp, shp, pack,
                           scale_log2, wo, wml, h, kvh, num_blocks, lbs, chunk, splits);
  else
    shared_split_tiles<128>((h / kvh) * pack, kv8, grid, st, qp, k_pool, v_pool, k_scale, v_scale, tp, table_stride, pp, limit, fp, shp, pack,
                            scale_log2, wo, wml, h, kvh, num_blocks, lbs, chunk, splits);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, kv8 ? "qqq_shared_kv8_split_kernel launch" : "qqq_shared_split_kernel launch");
  return decode_combine_launch(b, st, wo, wml, pp, limit, o_fp16, xq, s1, h, d, chunk, splits);
}

extern "C" int qqq_decode_attn_paged_shared(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                            const void* pos, const void* family, const void* shared, int pack, float scale, void* o_fp16,
                                            void* xq, void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d,
                                            int num_blocks, int block_size, int max_len, int dev, void* stream) {
  return decode_attn_paged_shared("qqq_decode_attn_paged_shared", false, q, k_pool, v_pool, nullptr, nullptr, block_table, table_stride, pos,
                                  family, shared, pack, scale, o_fp16, xq, s1, workspace, workspace_bytes, b, h, kvh, d, num_blocks,
                                  block_size, max_len, dev, stream);
}

extern "C" int qqq_decode_attn_paged_shared_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale,
                                                const void* v_scale, const void* block_table, int table_stride, const void* pos,
                                                const void* family, const void* shared, int pack, float scale, void* o_fp16, void* xq,
                                                void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d,
                                                int num_blocks, int block_size, int max_len, int dev, void* stream) {
  return decode_attn_paged_shared("qqq_decode_attn_paged_shared_kv8", true, q, k_pool, v_pool, k_scale, v_scale, block_table, table_stride,
                                  pos, family, shared, pack, scale, o_fp16, xq, s1, workspace, workspace_bytes, b, h, kvh, d, num_blocks,
                                  block_size, max_len, dev, stream);
}

// ---- the paged prefill attention (include/qqq_amd_prefill.h; kernels in qqq_prefill.hip.h): one attention launch over the packed batch's
// query tiles and one launch that quantises the rows it wrote.  One body for the pair; `name` is the entry point's.
static bool prefill_shape_error(int h, int kvh, int d) {
  return h < 1 || kvh < 1 || h % kvh != 0 || h / kvh > DEC_GMAX || (d != 64 && d != 128) || (long long)h * d > 16384;
}

extern "C" size_t qqq_prefill_attn_workspace_bytes(int m, int h, int d) {
  if (m <= 0 || h < 1 || (d != 64 && d != 128) || (long long)h * d > 16384) return 0;
  return (size_t)m * h * d * sizeof(_Float16);
}

template <int VPT>
static void prefill_quant(int m, hipStream_t st, const _Float16* o16, const int* cu, const long long* sp, long long limit, int8_t* xq,
                          float* s1, int b, int hd) {
  hipLaunchKernelGGL((qqq_prefill_quant_kernel<VPT, PF_QUANT_NT>), dim3(m), dim3(PF_QUANT_NT), 0, st, o16, cu, sp, limit, xq, s1, m, b, hd);
}

static int prefill_attn_paged(const char* name, bool kv8, const void* q, const void* k_pool, const void* v_pool, const void* k_scale,
                              const void* v_scale, const void* block_table, int table_stride, const void* cu_tokens, const void* start_pos,
                              float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int m, int b, int h,
                              int kvh, int d, int num_blocks, int block_size, int max_len, int dev, void* stream) {
  g_err[0] = 0;
  if (m < 0 || b < 0 || h < 0 || kvh < 0 || d < 0 || num_blocks < 0 || block_size < 0 || table_stride < 0 || max_len < 0) {
    snprintf(g_err, sizeof(g_err), "%s: negative size (m=%d b=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d)",
             name, m, b, h, kvh, d, num_blocks, block_size, table_stride, max_len);
    return QQQ_ERR_ARG;
  }
  if (m == 0 || b == 0) return QQQ_OK;
  const int lbs = paged_log2_block(block_size);
  if (prefill_shape_error(h, kvh, d) || b > 65535 || lbs < 0 || num_blocks < 1 || (long long)num_blocks * block_size > 0x7fffffffLL ||
      table_stride < 1 || max_len < 1 || max_len > (long long)table_stride * block_size) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape m=%d b=%d h=%d kvh=%d d=%d num_blocks=%d block_size=%d table_stride=%d max_len=%d (need "
             "h %% kvh == 0, h / kvh <= %d, d 64 or 128, h*d <= 16384, b <= 65535, block_size a power of two in [16, 256], num_blocks >= 1, "
             "num_blocks * block_size < 2^31, 1 <= max_len <= table_stride * block_size)", name, m, b, h, kvh, d, num_blocks, block_size,
             table_stride, max_len, DEC_GMAX);
    return QQQ_ERR_ARG;
  }
  if (!o_fp16 && !xq && !s1) {
    snprintf(g_err, sizeof(g_err), "%s: no output (o_fp16 and xq / s1 are all NULL)", name);
    return QQQ_ERR_ARG;
  }
  if (!q || !k_pool || !v_pool || !block_table || !cu_tokens || !start_pos || (!xq) != (!s1) || (!o_fp16 && !workspace) ||
      misaligned(q, 16) || misaligned(k_pool, 16) || misaligned(v_pool, 16) || misaligned(block_table, 4) || misaligned(cu_tokens, 4) ||
      misaligned(start_pos, 8) || (workspace && misaligned(workspace, 16)) || (o_fp16 && misaligned(o_fp16, 16)) ||
      (xq && misaligned(xq, 8)) || (s1 && misaligned(s1, 4)) ||
      (kv8 && (!k_scale || !v_scale || misaligned(k_scale, 4) || misaligned(v_scale, 4)))) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (q / pools / scales / block_table / cu_tokens / start_pos must be non-NULL, workspace "
             "too where o_fp16 is NULL, xq and s1 both given or both NULL; q, pools, o_fp16, workspace 16-byte, start_pos / xq 8-byte, "
             "cu_tokens, block_table, s1 and the scales 4-byte aligned)", name);
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_prefill_attn_workspace_bytes(m, h, d);
  if (!o_fp16 && workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "%s: workspace of %zu bytes, need %zu", name, workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tq = PF_ROWS / (h / kvh);  // tokens of a query tile
  const int nslots = m / tq + b;      // sequence i owns the slots from cu_tokens[i] / tq + i on: an upper bound of the tiles of any split of m
  const dim3 grid(nslots, kvh), block(PF_NT);
  const long long limit = max_len;
  const float scale_log2 = scale * 1.4426950408889634f;
  const _Float16* qp = static_cast<const _Float16*>(q);
  const float *ksp = static_cast<const float*>(k_scale), *vsp = static_cast<const float*>(v_scale);
  const int* tp = static_cast<const int*>(block_table);
  const int* cup = static_cast<const int*>(cu_tokens);
  const long long* spp = static_cast<const long long*>(start_pos);
  _Float16* o16 = static_cast<_Float16*>(o_fp16 ? o_fp16 : workspace);
  if (kv8) {
    if (d == 64)
      hipLaunchKernelGGL((qqq_prefill_attn_kernel<64, true>), grid, block, 0, st, qp, k_pool, v_pool, ksp, vsp, tp, table_stride, cup, spp,
                         limit, scale_log2, o16, m, b, h, kvh, num_blocks, lbs, nslots);
    else
      hipLaunchKernelGGL((qqq_prefill_attn_kernel<128, true>), grid, block, 0, st, qp, k_pool, v_pool, ksp, vsp, tp, table_stride, cup, spp,
                         limit, scale_log2, o16, m, b, h, kvh, num_blocks, lbs, nslots);
  } else {
    if (d == 64)
      hipLaunchKernelGGL((qqq_prefill_attn_kernel<64, false>), grid, block, 0, st, qp, k_pool, v_pool, ksp, vsp, tp, table_stride, cup, spp,
                         limit, scale_log2, o16, m, b, h, kvh, num_blocks, lbs, nslots);
    else
      hipLaunchKernelGGL((qqq_prefill_attn_kernel<128, false>), grid, block, 0, st, qp, k_pool, v_pool, ksp, vsp, tp, table_stride, cup, spp,
                         limit, scale_log2, o16, m, b, h, kvh, num_blocks, lbs, nslots);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_prefill_attn_kernel launch");
  if (!xq) return QQQ_OK;
  int8_t* xqp = static_cast<int8_t*>(xq);
  float* s1p = static_cast<float*>(s1);
  const int hd = h * d, nvec = hd / 8;
  if (nvec <= PF_QUANT_NT)
    prefill_quant<1>(m, st, o16, cup, spp, limit, xqp, s1p, b, hd);
  else if (nvec <= 2 * PF_QUANT_NT)
    prefill_quant<2>(m, st, o16, cup, spp, limit, xqp, s1p, b, hd);
  else
    prefill_quant<4>(m, st, o16, cup, spp, limit, xqp, s1p, b, hd);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_prefill_quant_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_prefill_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                      const void* cu_tokens, const void* start_pos, float scale, void* o_fp16, void* xq, void* s1,
                                      void* workspace, size_t workspace_bytes, int m, int b, int h, int kvh, int d, int num_blocks,
                                      int block_size, int max_len, int dev, void* stream) {
  return prefill_attn_paged("qqq_prefill_attn_paged", false, q, k_pool, v_pool, nullptr, nullptr, block_table, table_stride, cu_tokens,
                            start_pos, scale, o_fp16, xq, s1, workspace, workspace_bytes, m, b, h, kvh, d, num_blocks, block_size, max_len,
                            dev, stream);
}

extern "C" int qqq_prefill_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                          const void* block_table, int table_stride, const void* cu_tokens, const void* start_pos,
                                          float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int m,
                                          int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int dev, void* stream) {
  return prefill_attn_paged("qqq_prefill_attn_paged_kv8", true, q, k_pool, v_pool, k_scale, v_scale, block_table, table_stride, cu_tokens,
                            start_pos, scale, o_fp16, xq, s1, workspace, workspace_bytes, m, b, h, kvh, d, num_blocks, block_size, max_len,
                            dev, stream);
}

// ---- the fused token sampler (include/qqq_amd_sample.h; kernel in qqq_sample.hip.h): one launch, one workgroup per row, no workspace.
extern "C" int qqq_sample_tokens(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u,
                                 void* tokens, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_tokens: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_tokens: bad shape vocab=%d ld=%d (need 1 <= vocab <= %d, ld >= vocab, ld %% 8 == 0)", vocab, ld,
             SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (!logits || !temperature || !top_k || !top_p || !u || !tokens || misaligned(logits, 16) || misaligned(temperature, 4) ||
      misaligned(top_k, 4) || misaligned(top_p, 4) || misaligned(u, 4) || misaligned(tokens, 8)) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_tokens: bad argument (every pointer must be non-NULL; logits 16-byte, tokens 8-byte, "
             "temperature / top_k / top_p / u 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_sample_tokens_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const float*>(temperature), static_cast<const int*>(top_k),
                     static_cast<const float*>(top_p), static_cast<const float*>(u), static_cast<long long*>(tokens), vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_sample_tokens_kernel launch");
  return QQQ_OK;
}

// ---- the fused scoring kernel (include/qqq_amd_score.h; kernel in qqq_score.hip.h): one launch, one workgroup per row, no workspace.
extern "C" int qqq_token_logprobs(const void* logits, int ld, const void* targets, void* logprob, void* argmax, int rows, int vocab, int dev,
                                  void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 1048576) {
    snprintf(g_err, sizeof(g_err), "qqq_token_logprobs: rows=%d outside [0, 1048576]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_token_logprobs: bad shape vocab=%d ld=%d (need 1 <= vocab <= %d, ld >= vocab, ld %% 8 == 0)", vocab, ld,
             SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (!logits || !targets || !logprob || misaligned(logits, 16) || misaligned(targets, 8) || misaligned(logprob, 4) || misaligned(argmax, 8)) {
    snprintf(g_err, sizeof(g_err), "qqq_token_logprobs: bad argument (logits, targets and logprob must be non-NULL; logits 16-byte, targets and "
             "argmax 8-byte, logprob 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_token_logprobs_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const long long*>(targets), static_cast<float*>(logprob),
                     static_cast<long long*>(argmax), vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_token_logprobs_kernel launch");
  return QQQ_OK;
}

// ---- the fused top-k log-probability kernel (include/qqq_amd_logprobs.h; kernels in qqq_logprobs.hip.h): one launch, one workgroup
// per row, no workspace.  The checks the two entries share: shape, k, and the top-k pair.
static int topk_logprobs_check(const char* name, const void* logits, int ld, const void* top_ids, const void* top_logprobs, int k, int rows,
                               int vocab) {
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "%s: bad shape vocab=%d ld=%d (need 1 <= vocab <= %d, ld >= vocab, ld %% 8 == 0)", name, vocab, ld,
             SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (k < 0 || k > LGP_MAX_K || k > vocab) {
    snprintf(g_err, sizeof(g_err), "%s: k=%d outside [0, min(%d, vocab=%d)]", name, k, LGP_MAX_K, vocab);
    return QQQ_ERR_ARG;
  }
  if ((k == 0) != (top_ids == nullptr) || (k == 0) != (top_logprobs == nullptr)) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (top_ids and top_logprobs must be NULL exactly when k == 0; k=%d)", name, k);
    return QQQ_ERR_ARG;
  }
  if (!logits || misaligned(logits, 16) || misaligned(top_ids, 4) || misaligned(top_logprobs, 4)) {
    snprintf(g_err, sizeof(g_err), "%s: bad argument (logits must be non-NULL and 16-byte, top_ids and top_logprobs 4-byte aligned)", name);
    return QQQ_ERR_ARG;
  }
  return QQQ_OK;
}

extern "C" int qqq_topk_logprobs(const void* logits, int ld, const void* tokens, void* logprob, void* rank, void* top_ids, void* top_logprobs,
                                 int k, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_topk_logprobs: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  const int rc = topk_logprobs_check("qqq_topk_logprobs", logits, ld, top_ids, top_logprobs, k, rows, vocab);
  if (rc != QQQ_OK) return rc;
  if ((tokens == nullptr) != (logprob == nullptr) || (tokens == nullptr) != (rank == nullptr) || (!tokens && k == 0) ||
      misaligned(tokens, 8) || misaligned(logprob, 4) || misaligned(rank, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_topk_logprobs: bad argument (tokens, logprob and rank must be given or NULL together, and not NULL "
             "with k == 0; tokens 8-byte, logprob and rank 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_topk_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const long long*>(tokens), static_cast<float*>(logprob),
                     static_cast<int*>(rank), static_cast<int*>(top_ids), static_cast<float*>(top_logprobs), k, vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_topk_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_topk_logprobs_step(const void* logits, int ld, const void* out, int out_stride, const void* n_out, void* n_rec,
                                      void* logprob, void* rank, void* top_ids, void* top_logprobs, int cap, int k, int rows, int vocab,
                                      int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_topk_logprobs_step: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  const int rc = topk_logprobs_check("qqq_topk_logprobs_step", logits, ld, top_ids, top_logprobs, k, rows, vocab);
  if (rc != QQQ_OK) return rc;
  if (out_stride < 1 || cap < 1) {
    snprintf(g_err, sizeof(g_err), "qqq_topk_logprobs_step: bad shape out_stride=%d cap=%d (need both >= 1)", out_stride, cap);
    return QQQ_ERR_ARG;
  }
  if (!out || !n_out || !n_rec || !logprob || !rank || misaligned(out, 8) || misaligned(n_out, 4) || misaligned(n_rec, 4) ||
      misaligned(logprob, 4) || misaligned(rank, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_topk_logprobs_step: bad argument (out, n_out, n_rec, logprob and rank must be non-NULL; out 8-byte, "
             "everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_topk_step_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const long long*>(out), out_stride,
                     static_cast<const int*>(n_out), static_cast<int*>(n_rec), static_cast<float*>(logprob), static_cast<int*>(rank),
                     static_cast<int*>(top_ids), static_cast<float*>(top_logprobs), cap, k, vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_topk_step_kernel launch");
  return QQQ_OK;
}

// ---- the decode loop's sample-and-advance step (include/qqq_amd_step.h; kernel in qqq_step.hip.h): the sampler's launch with an epilogue.
extern "C" int qqq_sample_advance(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u,
                                  int u_stride, void* tick, void* ids, void* pos, void* slots, const void* block_table, int table_stride,
                                  void* remaining, const void* eos, void* out, int out_stride, void* n_out, int rows, int vocab,
                                  int block_size, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_advance: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_advance: bad shape vocab=%d ld=%d (need 1 <= vocab <= %d, ld >= vocab, ld %% 8 == 0)", vocab,
             ld, SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (block_size < 16 || block_size > 256 || (block_size & (block_size - 1)) || table_stride < 1 || out_stride < 1 || u_stride < 1) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_advance: bad shape block_size=%d table_stride=%d out_stride=%d u_stride=%d (need block_size a "
             "power of two in [16, 256] and every stride >= 1)", block_size, table_stride, out_stride, u_stride);
    return QQQ_ERR_ARG;
  }
  if (!logits || !temperature || !top_k || !top_p || !u || !tick || !ids || !pos || !slots || !block_table || !remaining || !eos || !out ||
      !n_out || misaligned(logits, 16) || misaligned(temperature, 4) || misaligned(top_k, 4) || misaligned(top_p, 4) || misaligned(u, 4) ||
      misaligned(tick, 4) || misaligned(ids, 8) || misaligned(pos, 8) || misaligned(slots, 8) || misaligned(block_table, 4) ||
      misaligned(remaining, 4) || misaligned(eos, 4) || misaligned(out, 8) || misaligned(n_out, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_sample_advance: bad argument (every pointer must be non-NULL; logits 16-byte, ids / pos / slots / out "
             "8-byte, everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_step_emit st;
  st.uu = static_cast<const float*>(u);
  st.u_stride = u_stride;
  st.tick = static_cast<int*>(tick);
  st.ids = static_cast<long long*>(ids);
  st.pos = static_cast<long long*>(pos);
  st.slots = static_cast<long long*>(slots);
  st.block_table = static_cast<const int*>(block_table);
  st.remaining = static_cast<int*>(remaining);
  st.eos = static_cast<const int*>(eos);
  st.out = static_cast<long long*>(out);
  st.n_out = static_cast<int*>(n_out);
  st.table_stride = table_stride;
  st.out_stride = out_stride;
  st.block_shift = __builtin_ctz((unsigned)block_size);
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_step_advance_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const float*>(temperature), static_cast<const int*>(top_k),
                     static_cast<const float*>(top_p), st, vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_step_advance_kernel launch");
  return QQQ_OK;
}

// ---- the speculative decode loop's verify-and-advance step (include/qqq_amd_spec.h; kernels in qqq_spec.hip.h): the sampler's launch over
// rows * (draft_len + 1) logits rows into the workspace, then one workgroup per row for the accept rule, the drafter and the next positions.
extern "C" size_t qqq_spec_advance_workspace_bytes(int rows, int draft_len) {
  if (rows < 1 || draft_len < 1 || draft_len > SPEC_MAX_DRAFT || (long long)rows * (draft_len + 1) > 65535) return 0;
  return (size_t)rows * (size_t)(draft_len + 1) * sizeof(long long);
}

extern "C" int qqq_spec_advance(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u,
                                int u_stride, void* tick, void* ids, void* pos, void* slots, void* start, const void* block_table,
                                int table_stride, void* remaining, const void* eos, void* hist, int hist_stride, void* hist_len,
                                void* n_out, void* n_acc, void* workspace, size_t workspace_bytes, int rows, int draft_len, int ngram_max,
                                int vocab, int block_size, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: rows=%d is negative", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (draft_len < 1 || draft_len > SPEC_MAX_DRAFT || ngram_max < 1 || ngram_max > SPEC_MAX_NGRAM) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: draft_len=%d outside [1, %d] or ngram_max=%d outside [1, %d]", draft_len,
             SPEC_MAX_DRAFT, ngram_max, SPEC_MAX_NGRAM);
    return QQQ_ERR_ARG;
  }
  const int group = draft_len + 1;
  if ((long long)rows * group > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: rows=%d times draft_len + 1 = %d exceeds 65535 logits rows", rows, group);
    return QQQ_ERR_ARG;
  }
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: bad shape vocab=%d ld=%d (need 1 <= vocab <= %d, ld >= vocab, ld %% 8 == 0)", vocab, ld,
             SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (block_size < 16 || block_size > 256 || (block_size & (block_size - 1)) || table_stride < 1 || hist_stride < 1 || u_stride < group) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: bad shape block_size=%d table_stride=%d hist_stride=%d u_stride=%d (need block_size a "
             "power of two in [16, 256], table_stride and hist_stride >= 1, u_stride >= draft_len + 1 = %d)", block_size, table_stride,
             hist_stride, u_stride, group);
    return QQQ_ERR_ARG;
  }
  if (!logits || !temperature || !top_k || !top_p || !u || !tick || !ids || !pos || !slots || !start || !block_table || !remaining || !eos ||
      !hist || !hist_len || !n_out || !n_acc || !workspace || misaligned(logits, 16) || misaligned(temperature, 4) || misaligned(top_k, 4) ||
      misaligned(top_p, 4) || misaligned(u, 4) || misaligned(tick, 4) || misaligned(ids, 8) || misaligned(pos, 8) || misaligned(slots, 8) ||
      misaligned(start, 8) || misaligned(block_table, 4) || misaligned(remaining, 4) || misaligned(eos, 4) || misaligned(hist, 4) ||
      misaligned(hist_len, 4) || misaligned(n_out, 4) || misaligned(n_acc, 4) || misaligned(workspace, 8)) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: bad argument (every pointer must be non-NULL; logits 16-byte, ids / pos / slots / "
             "start / workspace 8-byte, everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_spec_advance_workspace_bytes(rows, draft_len);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "qqq_spec_advance: workspace of %zu bytes, %zu needed (qqq_spec_advance_workspace_bytes)", workspace_bytes,
             need);
    return QQQ_ERR_ARG;
  }
  qqq_spec_draw dr;
  dr.uu = static_cast<const float*>(u);
  dr.tick = static_cast<const int*>(tick);
  dr.tokens = static_cast<long long*>(workspace);
  dr.u_stride = u_stride;
  dr.group = group;
  qqq_spec_state st;
  st.tokens = static_cast<const long long*>(workspace);
  st.tick = static_cast<int*>(tick);
  st.ids = static_cast<long long*>(ids);
  st.pos = static_cast<long long*>(pos);
  st.slots = static_cast<long long*>(slots);
  st.start = static_cast<long long*>(start);
  st.block_table = static_cast<const int*>(block_table);
  st.remaining = static_cast<int*>(remaining);
  st.eos = static_cast<const int*>(eos);
  st.hist = static_cast<int*>(hist);
  st.hist_len = static_cast<int*>(hist_len);
  st.n_out = static_cast<int*>(n_out);
  st.n_acc = static_cast<int*>(n_acc);
  st.table_stride = table_stride;
  st.hist_stride = hist_stride;
  st.block_shift = __builtin_ctz((unsigned)block_size);
  st.draft_len = draft_len;
  st.ngram_max = ngram_max;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_spec_draw_kernel, dim3(rows * group), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, static_cast<const float*>(temperature), static_cast<const int*>(top_k),
                     static_cast<const float*>(top_p), dr, vocab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_spec_draw_kernel launch");
  hipLaunchKernelGGL(qqq_spec_advance_kernel, dim3(rows), dim3(SPEC_NT), 0, static_cast<hipStream_t>(stream), st);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_spec_advance_kernel launch");
  return QQQ_OK;
}

// ---- the repetition / presence / frequency penalty (include/qqq_amd_penalty.h; kernel in qqq_penalty.hip.h): one launch, one workgroup per
// row, in front of a sampler; the workspace is zero on entry and left zero.
extern "C" size_t qqq_penalize_logits_workspace_bytes(int rows, int vocab) {
  if (rows < 1 || rows > 65535 || vocab < 1 || vocab > SMP_MAX_VOCAB) return 0;
  return (size_t)rows * (size_t)vocab * sizeof(unsigned);
}

extern "C" int qqq_penalize_logits(void* logits, int ld, const void* ids, const void* pos, int group, void* seen, int seen_stride,
                                   const void* n_prompt, const void* repetition, const void* presence, const void* frequency,
                                   void* workspace, size_t workspace_bytes, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_penalize_logits: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (group < 1 || group > PEN_MAX_GROUP || (long long)rows * group > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_penalize_logits: group=%d outside [1, %d], or rows=%d times group exceeds 65535 logits rows", group,
             PEN_MAX_GROUP, rows);
    return QQQ_ERR_ARG;
  }
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || seen_stride < 1 || seen_stride > PEN_MAX_SEEN) {
    snprintf(g_err, sizeof(g_err), "qqq_penalize_logits: bad shape vocab=%d ld=%d seen_stride=%d (need 1 <= vocab <= %d, ld >= vocab, "
             "1 <= seen_stride < 2^30)", vocab, ld, seen_stride, SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (!logits || !ids || !pos || !seen || !n_prompt || !repetition || !presence || !frequency || !workspace || misaligned(logits, 2) ||
      misaligned(ids, 8) || misaligned(pos, 8) || misaligned(seen, 4) || misaligned(n_prompt, 4) || misaligned(repetition, 4) ||
      misaligned(presence, 4) || misaligned(frequency, 4) || misaligned(workspace, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_penalize_logits: bad argument (every pointer must be non-NULL; logits 2-byte, ids / pos 8-byte, "
             "everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_penalize_logits_workspace_bytes(rows, vocab);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "qqq_penalize_logits: workspace of %zu bytes, %zu needed (qqq_penalize_logits_workspace_bytes)",
             workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_penalize_logits_kernel, dim3(rows), dim3(PEN_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned short*>(logits), ld, static_cast<const long long*>(ids), static_cast<const long long*>(pos), group,
                     static_cast<int*>(seen), seen_stride, static_cast<const int*>(n_prompt), static_cast<const float*>(repetition),
                     static_cast<const float*>(presence), static_cast<const float*>(frequency), static_cast<unsigned*>(workspace), vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_penalize_logits_kernel launch");
  return QQQ_OK;
}

// ---- stop sequences, stop token ids and the minimum length (include/qqq_amd_stop.h; kernels in qqq_stop.hip.h): one launch
// each, one wave per logits row / per row, no workspace.
extern "C" int qqq_ban_tokens(void* logits, int ld, const void* n_out, int base, const void* min_new, const void* eos, const void* ban_ids,
                              int n_ban, int group, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_ban_tokens: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (group < 1 || group > STOP_MAX_GROUP || (long long)rows * group > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_ban_tokens: group=%d outside [1, %d], or rows=%d times group exceeds 65535 logits rows", group,
             STOP_MAX_GROUP, rows);
    return QQQ_ERR_ARG;
  }
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || n_ban < 0 || n_ban > STOP_MAX) {
    snprintf(g_err, sizeof(g_err), "qqq_ban_tokens: bad shape vocab=%d ld=%d n_ban=%d (need 1 <= vocab <= %d, ld >= vocab, 0 <= n_ban <= %d)",
             vocab, ld, n_ban, SMP_MAX_VOCAB, STOP_MAX);
    return QQQ_ERR_ARG;
  }
  if (!logits || !n_out || !min_new || !eos || (n_ban == 0) != (ban_ids == nullptr) || misaligned(logits, 2) || misaligned(n_out, 4) ||
      misaligned(min_new, 4) || misaligned(eos, 4) || misaligned(ban_ids, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_ban_tokens: bad argument (logits, n_out, min_new and eos must be non-NULL, ban_ids NULL exactly when "
             "n_ban == 0; logits 2-byte, everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const int total = rows * group;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_ban_tokens_kernel, dim3((total + STOP_WAVES - 1) / STOP_WAVES), dim3(STOP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned short*>(logits), ld, static_cast<const int*>(n_out), base, static_cast<const int*>(min_new),
                     static_cast<const int*>(eos), static_cast<const int*>(ban_ids), n_ban, group, total, vocab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_ban_tokens_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_stop_check(const void* tokens, int token_bytes, int tok_stride, const void* base, const void* first, const void* n_out,
                              const void* stop_ids, int stop_stride, const void* stop_len, int n_stop, const void* end_ids, int n_end,
                              const void* eos, const void* min_new, void* n_seen, void* n_trim, void* stop_hit, void* ids, void* pos, void* slots, void* start,
                              void* remaining, int group, int rows, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_stop_check: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (group < 1 || group > STOP_MAX_GROUP) {
    snprintf(g_err, sizeof(g_err), "qqq_stop_check: group=%d outside [1, %d]", group, STOP_MAX_GROUP);
    return QQQ_ERR_ARG;
  }
  if ((token_bytes != 4 && token_bytes != 8) || tok_stride < 1 || n_stop < 0 || n_stop > STOP_MAX || stop_stride < 1 ||
      stop_stride > STOP_MAX || n_end < 0 || n_end > STOP_MAX) {
    snprintf(g_err, sizeof(g_err), "qqq_stop_check: bad shape token_bytes=%d tok_stride=%d n_stop=%d stop_stride=%d n_end=%d (need token_bytes "
             "4 or 8, tok_stride >= 1, 0 <= n_stop <= %d, 1 <= stop_stride <= %d, 0 <= n_end <= %d)", token_bytes, tok_stride, n_stop,
             stop_stride, n_end, STOP_MAX, STOP_MAX, STOP_MAX);
    return QQQ_ERR_ARG;
  }
  if (!tokens || !base || !n_out || !min_new || !n_seen || !n_trim || !stop_hit || !ids || !pos || !slots || !remaining ||
      (n_stop == 0) != (stop_ids == nullptr) || (n_stop == 0) != (stop_len == nullptr) || (n_end == 0) != (end_ids == nullptr) ||
      misaligned(tokens, token_bytes) || misaligned(base, 4) || misaligned(first, 4) || misaligned(n_out, 4) || misaligned(stop_ids, 4) ||
      misaligned(stop_len, 4) || misaligned(end_ids, 4) || misaligned(eos, 4) || misaligned(min_new, 4) || misaligned(n_seen, 4) || misaligned(n_trim, 4) ||
      misaligned(stop_hit, 4) || misaligned(ids, 8) || misaligned(pos, 8) || misaligned(slots, 8) || misaligned(start, 8) ||
      misaligned(remaining, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_stop_check: bad argument (every pointer but first, eos and start must be non-NULL; stop_ids and stop_len "
             "NULL exactly when n_stop == 0, end_ids when n_end == 0; tokens token_bytes-aligned, ids / pos / slots / start 8-byte, "
             "everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_stop_state st;
  st.tokens = tokens;
  st.base = static_cast<const int*>(base);
  st.first = static_cast<const int*>(first);
  st.n_out = static_cast<const int*>(n_out);
  st.stop_ids = static_cast<const int*>(stop_ids);
  st.stop_len = static_cast<const int*>(stop_len);
  st.end_ids = static_cast<const int*>(end_ids);
  st.eos = static_cast<const int*>(eos);
  st.min_new = static_cast<const int*>(min_new);
  st.n_seen = static_cast<int*>(n_seen);
  st.n_trim = static_cast<int*>(n_trim);
  st.stop_hit = static_cast<int*>(stop_hit);
  st.ids = static_cast<long long*>(ids);
  st.pos = static_cast<long long*>(pos);
  st.slots = static_cast<long long*>(slots);
  st.start = static_cast<long long*>(start);
  st.remaining = static_cast<int*>(remaining);
  st.token_bytes = token_bytes;
  st.tok_stride = tok_stride;
  st.stop_stride = stop_stride;
  st.n_stop = n_stop;
  st.n_end = n_end;
  st.group = group;
  st.rows = rows;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_stop_check_kernel, dim3((rows + STOP_WAVES - 1) / STOP_WAVES), dim3(STOP_NT), 0, static_cast<hipStream_t>(stream),
                     st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_stop_check_kernel launch");
  return QQQ_OK;
}

// ---- guided decoding (include/qqq_amd_guided.h; kernels in qqq_guided.hip.h): one launch each, a row's columns over several
// workgroups / one wave per row, no workspace.
extern "C" int qqq_fsm_mask(void* logits, int ld, const void* state, const void* eos, const void* remaining, const void* offsets,
                            const void* tokens, const void* accept, int n_states, int n_edges, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_mask: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (vocab < 1 || vocab > SMP_MAX_VOCAB || ld < vocab || n_states < 1 || n_edges < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_mask: bad shape vocab=%d ld=%d n_states=%d n_edges=%d (need 1 <= vocab <= %d, ld >= vocab, "
             "n_states >= 1, n_edges >= 0)", vocab, ld, n_states, n_edges, SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (!logits || !state || !offsets || !accept || (n_edges == 0) != (tokens == nullptr) || misaligned(logits, 2) || misaligned(state, 4) ||
      misaligned(eos, 4) || misaligned(remaining, 4) || misaligned(offsets, 4) || misaligned(tokens, 4) || misaligned(accept, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_mask: bad argument (logits, state, offsets and accept must be non-NULL, tokens NULL exactly when "
             "n_edges == 0; logits 2-byte, everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const int width = fsm_mask_width(rows, vocab);
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_fsm_mask_kernel, dim3((vocab + width - 1) / width, rows), dim3(FSM_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned short*>(logits), ld, static_cast<const int*>(state), static_cast<const int*>(eos),
                     static_cast<const int*>(remaining), static_cast<const int*>(offsets), static_cast<const int*>(tokens),
                     static_cast<const int*>(accept), n_states, n_edges, vocab, width);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_fsm_mask_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_fsm_advance(const void* out, int out_stride, const void* n_out, void* n_fsm, void* state, const void* eos,
                               const void* offsets, const void* tokens, const void* next, const void* accept, int n_states, int n_edges,
                               void* ids, void* pos, void* slots, void* remaining, int rows, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 0 || rows > 65535) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_advance: rows=%d outside [0, 65535]", rows);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (out_stride < 1 || n_states < 1 || n_edges < 0) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_advance: bad shape out_stride=%d n_states=%d n_edges=%d (need out_stride >= 1, n_states >= 1, "
             "n_edges >= 0)", out_stride, n_states, n_edges);
    return QQQ_ERR_ARG;
  }
  if (!out || !n_out || !n_fsm || !state || !offsets || !accept || !ids || !pos || !slots || !remaining ||
      (n_edges == 0) != (tokens == nullptr) || (n_edges == 0) != (next == nullptr) || misaligned(out, 8) || misaligned(n_out, 4) ||
      misaligned(n_fsm, 4) || misaligned(state, 4) || misaligned(eos, 4) || misaligned(offsets, 4) || misaligned(tokens, 4) ||
      misaligned(next, 4) || misaligned(accept, 4) || misaligned(ids, 8) || misaligned(pos, 8) || misaligned(slots, 8) ||
      misaligned(remaining, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_fsm_advance: bad argument (every pointer but eos must be non-NULL, tokens and next NULL exactly when "
             "n_edges == 0; out, ids, pos and slots 8-byte, everything else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_fsm_advance_args a;
  a.out = static_cast<const long long*>(out);
  a.n_out = static_cast<const int*>(n_out);
  a.n_fsm = static_cast<int*>(n_fsm);
  a.state = static_cast<int*>(state);
  a.eos = static_cast<const int*>(eos);
  a.offsets = static_cast<const int*>(offsets);
  a.tokens = static_cast<const int*>(tokens);
  a.next = static_cast<const int*>(next);
  a.accept = static_cast<const int*>(accept);
  a.ids = static_cast<long long*>(ids);
  a.pos = static_cast<long long*>(pos);
  a.slots = static_cast<long long*>(slots);
  a.remaining = static_cast<int*>(remaining);
  a.out_stride = out_stride;
  a.n_states = n_states;
  a.n_edges = n_edges;
  a.rows = rows;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_fsm_advance_kernel, dim3((rows + FSM_WAVES - 1) / FSM_WAVES), dim3(FSM_NT), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_fsm_advance_kernel launch");
  return QQQ_OK;
}

// ---- batched LoRA (include/qqq_amd_lora.h; kernel in qqq_lora.hip.h): one launch, a workgroup per 16 tokens and column
// chunk, no workspace.
extern "C" int qqq_lora_add(void* y, int ldy, const void* xq, const void* s1, const void* A, size_t a_stride, const void* B, size_t b_stride,
                            const void* scale, const void* slot, const void* part_cols_host, int P, int T, int N, int K, int R, int S, int dev,
                            void* stream) {
  g_err[0] = 0;
  const int* part_cols = static_cast<const int*>(part_cols_host);
  if (T < 0 || T > 1048576) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: T=%d outside [0, 1048576]", T);
    return QQQ_ERR_ARG;
  }
  if (T == 0) return QQQ_OK;
  if (R != 8 && R != 16 && R != 32 && R != 64) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: R=%d is not one of 8, 16, 32, 64", R);
    return QQQ_ERR_ARG;
  }
  if (N < 64 || K < 64 || N % 64 != 0 || K % 64 != 0 || S < 1 || P < 1 || P > 3 || ldy < N || ldy % 2 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: bad shape N=%d K=%d S=%d P=%d ldy=%d (need N and K positive multiples of 64, S >= 1, "
             "1 <= P <= 3, ldy >= N and even)", N, K, S, P, ldy);
    return QQQ_ERR_ARG;
  }
  if (!part_cols) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: part_cols must be non-NULL (P + 1 ints in host memory)");
    return QQQ_ERR_ARG;
  }
  bool cols_ok = part_cols[0] == 0 && part_cols[P] == N;
  for (int p = 0; p < P; ++p) cols_ok = cols_ok && part_cols[p] % 64 == 0 && part_cols[p] >= 0 && part_cols[p + 1] > part_cols[p];
  if (!cols_ok) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: part_cols must ascend strictly from 0 to N=%d in multiples of 64 (P=%d: %d, %d, %d, %d)", N, P,
             part_cols[0], part_cols[1], P > 1 ? part_cols[2] : -1, P > 2 ? part_cols[3] : -1);
    return QQQ_ERR_ARG;
  }
  if (a_stride < (size_t)P * R * K || a_stride % 8 != 0 || b_stride < (size_t)N * R || b_stride % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: bad slot stride a_stride=%zu b_stride=%zu (need multiples of 8 elements, a_stride >= "
             "P * R * K = %zu, b_stride >= N * R = %zu)", a_stride, b_stride, (size_t)P * R * K, (size_t)N * R);
    return QQQ_ERR_ARG;
  }
  if (!y || !xq || !s1 || !A || !B || !scale || !slot || misaligned(y, 4) || misaligned(xq, 16) || misaligned(s1, 4) || misaligned(A, 16) ||
      misaligned(B, 16) || misaligned(scale, 4) || misaligned(slot, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_lora_add: bad argument (every pointer must be non-NULL; xq, A and B 16-byte, everything else 4-byte "
             "aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_lora_args a;
  a.y = static_cast<unsigned short*>(y);
  a.xq = static_cast<const signed char*>(xq);
  a.s1 = static_cast<const float*>(s1);
  a.A = static_cast<const _Float16*>(A);
  a.B = static_cast<const _Float16*>(B);
  a.scale = static_cast<const float*>(scale);
  a.slot = static_cast<const int*>(slot);
  a.ldy = ldy;
  a.a_stride = (long long)a_stride;
  a.b_stride = (long long)b_stride;
  a.T = T;
  a.N = N;
  a.K = K;
  a.S = S;
  a.P = P;
  for (int p = 0; p < 4; ++p) a.pc[p] = p <= P ? part_cols[p] : N;
  a.chunk_w = lora_chunk_width(T, P, part_cols);
  const dim3 grid((T + LORA_TILE - 1) / LORA_TILE, lora_chunks(P, part_cols, a.chunk_w));
  DeviceGuard guard(dev);
  lora_launch(R, grid, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_lora_add_kernel launch");
  return QQQ_OK;
}

// ---- beam search (include/qqq_amd_beam.h; kernels in qqq_beam.hip.h): the step behind a pass's logits -- a workgroup per row into the
// workspace, then a wave per prompt that merges -- and the block copies of a cache reorder.
extern "C" size_t qqq_beam_step_workspace_bytes(int rows, int num_beams) {
  if (num_beams < 1 || num_beams > BEAM_MAX || rows < 1 || rows > 65535 || rows % num_beams != 0) return 0;
  return sizeof(int) * 2 * (size_t)rows * (size_t)(2 * num_beams);
}

extern "C" int qqq_beam_step(const void* logits, int ld, const void* cum, const void* live, void* cand_score, void* cand_logprob,
                             void* cand_parent, void* cand_token, void* next_ids, void* next_parent, void* next_cum, void* next_live,
                             void* workspace, size_t workspace_bytes, int num_beams, int eos, int rows, int vocab, int dev, void* stream) {
  g_err[0] = 0;
  if (num_beams < 1 || num_beams > BEAM_MAX) {
    snprintf(g_err, sizeof(g_err), "qqq_beam_step: num_beams=%d outside [1, %d]", num_beams, BEAM_MAX);
    return QQQ_ERR_ARG;
  }
  if (rows < 0 || rows > 65535 || rows % num_beams != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_beam_step: rows=%d outside [0, 65535] or no multiple of num_beams=%d", rows, num_beams);
    return QQQ_ERR_ARG;
  }
  if (rows == 0) return QQQ_OK;
  if (vocab < 2 * num_beams || vocab > SMP_MAX_VOCAB || ld < vocab || ld % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_beam_step: bad shape vocab=%d ld=%d (need 2 * num_beams = %d <= vocab <= %d, ld >= vocab, ld %% 8 == 0)",
             vocab, ld, 2 * num_beams, SMP_MAX_VOCAB);
    return QQQ_ERR_ARG;
  }
  if (!logits || !cum || !live || !cand_score || !cand_logprob || !cand_parent || !cand_token || !next_ids || !next_parent || !next_cum ||
      !next_live || !workspace || misaligned(logits, 16) || misaligned(cum, 4) || misaligned(live, 4) || misaligned(cand_score, 4) ||
      misaligned(cand_logprob, 4) || misaligned(cand_parent, 4) || misaligned(cand_token, 4) || misaligned(next_ids, 8) ||
      misaligned(next_parent, 4) || misaligned(next_cum, 4) || misaligned(next_live, 4) || misaligned(workspace, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_beam_step: bad argument (every pointer must be non-NULL; logits 16-byte, next_ids 8-byte, everything "
             "else 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const size_t need = qqq_beam_step_workspace_bytes(rows, num_beams);
  if (workspace_bytes < need) {
    snprintf(g_err, sizeof(g_err), "qqq_beam_step: workspace of %zu bytes, %zu needed (qqq_beam_step_workspace_bytes)", workspace_bytes, need);
    return QQQ_ERR_ARG;
  }
  const size_t cands = (size_t)rows * (size_t)(2 * num_beams);
  qqq_beam_args a;
  a.cum = static_cast<const float*>(cum);
  a.live = static_cast<const int*>(live);
  a.cand_score = static_cast<float*>(cand_score);
  a.cand_logprob = static_cast<float*>(cand_logprob);
  a.cand_parent = static_cast<int*>(cand_parent);
  a.cand_token = static_cast<int*>(cand_token);
  a.next_ids = static_cast<long long*>(next_ids);
  a.next_parent = static_cast<int*>(next_parent);
  a.next_cum = static_cast<float*>(next_cum);
  a.next_live = static_cast<int*>(next_live);
  int* ws_ids = static_cast<int*>(workspace);
  float* ws_lp = reinterpret_cast<float*>(ws_ids + cands);
  a.ws_ids = ws_ids;
  a.ws_lp = ws_lp;
  a.B = num_beams;
  a.eos = eos;
  a.prompts = rows / num_beams;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_beam_rows_kernel, dim3(rows), dim3(SMP_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(logits), ld, a.live, ws_ids, ws_lp, 2 * num_beams, vocab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_beam_rows_kernel launch");
  hipLaunchKernelGGL(qqq_beam_merge_kernel, dim3((a.prompts + BEAM_WAVES - 1) / BEAM_WAVES), dim3(BEAM_NT), 0,
                     static_cast<hipStream_t>(stream), a);
  e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_beam_merge_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_copy_blocks(const void* pools, int n_pools, const void* src, const void* dst, int n, size_t block_bytes, int num_blocks,
                               int dev, void* stream) {
  g_err[0] = 0;
  if (n < 0 || n > 65535 * 16) {
    snprintf(g_err, sizeof(g_err), "qqq_copy_blocks: n=%d outside [0, %d]", n, 65535 * 16);
    return QQQ_ERR_ARG;
  }
  if (n == 0) return QQQ_OK;
  if (n_pools < 1 || n_pools > 65535 || num_blocks < 1 || block_bytes < 16 || block_bytes % 16 != 0 || block_bytes / 16 > 0xffffffffull) {
    snprintf(g_err, sizeof(g_err), "qqq_copy_blocks: bad shape n_pools=%d num_blocks=%d block_bytes=%zu (need 1 <= n_pools <= 65535, "
             "num_blocks >= 1, block_bytes a positive multiple of 16)", n_pools, num_blocks, block_bytes);
    return QQQ_ERR_ARG;
  }
  if (!pools || !src || !dst || misaligned(pools, 8) || misaligned(src, 4) || misaligned(dst, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_copy_blocks: bad argument (pools, src and dst must be non-NULL; pools 8-byte, src and dst 4-byte "
             "aligned)");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_copy_blocks_kernel, dim3(n, n_pools), dim3(COPY_NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const void* const*>(pools), static_cast<const int*>(src), static_cast<const int*>(dst),
                     (unsigned)(block_bytes / 16), num_blocks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_copy_blocks_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_quantlinear_forward(const void* x, void* xq, void* s1, const void* B, void* C, void* D,
                                       const void* s2, const void* s3, int m, int n, int k, void* workspace,
                                       int groupsize, int dev, void* stream, int max_par, const void* bias) {
  const int rc = qqq_dynamic_quant(x, xq, s1, m, k, dev, stream);
  if (rc != QQQ_OK) return rc;
  return qqq_w4a8_gemm_ex(xq, B, C, D, s1, s2, s3, m, n, k, workspace, groupsize, dev, stream, -1, -1, -1, max_par,
                          nullptr, nullptr, bias);
}

extern "C" int qqq_quantlinear_forward2(const void* x, void* xq, void* s1, const void* B, void* C, void* D,
                                        const void* s2, const void* s3, int m, int n, int k, void* workspace,
                                        int groupsize, int dev, void* stream, int max_par, const void* bias, const void* W8) {
  const int rc = qqq_dynamic_quant(x, xq, s1, m, k, dev, stream);
  if (rc != QQQ_OK) return rc;
  return qqq_w4a8_gemm_ex2(xq, B, C, D, s1, s2, s3, m, n, k, workspace, groupsize, dev, stream, -1, -1, -1, max_par,
                           nullptr, nullptr, bias, W8);
}

// ---- load-time expansion of per-group weights (opt-in): B + s3 -> W8, once per layer; see qqq_small.hip.h for the layout
extern "C" int qqq_expand_int8(const void* B, const void* s3, void* W8, int k, int n, int groupsize, int dev, void* stream) {
  g_err[0] = 0;
  if (k == 0 || n == 0) return QQQ_OK;
  const bool grouped = groupsize != -1;
  if (!B || (grouped && !s3) || !W8 || (grouped && groupsize != 128) || k < 0 || n < 0 || (k % 128) != 0 || (n % 64) != 0 || (k / 64) > 65535 ||
      (long long)n * k >= (1ll << 32) || (((uintptr_t)B | (uintptr_t)W8) & 15) != 0 || (grouped && ((uintptr_t)s3 & 3) != 0)) {
    snprintf(g_err, sizeof(g_err), "qqq_expand_int8: need groupsize -1 or 128, k %% 128 == 0, n %% 64 == 0, n * k < 4 GiB, 16-byte aligned B / W8");
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  if (grouped)
    hipLaunchKernelGGL(qqq_expand_int8_kernel<true>, dim3(n / 64, k / 64), dim3(128), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned*>(B), static_cast<const _Float16*>(s3), static_cast<v4u*>(W8), n);
  else
    hipLaunchKernelGGL(qqq_expand_int8_kernel<false>, dim3(n / 64, k / 64), dim3(128), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned*>(B), static_cast<const _Float16*>(nullptr), static_cast<v4u*>(W8), n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_expand_int8_kernel launch");
  return QQQ_OK;
}

// ---- int4 packer / unpacker: device buffers go through the HIP kernels, host buffers through the
// same closed form on the CPU (a thread per slice of k-tiles).  Offline format conversion, not part of the GEMM path.
template <bool PACK>
static void pack_host_range(const int8_t* codes_in, int8_t* codes_out, const unsigned* B_in, unsigned* B_out, int n,
                            int grouped, int kt0, int kt1) {
  int pb[8], pr[8];
  for (int p = 0; p < 8; ++p) qqq_nibble_coords(p, grouped != 0, pb[p], pr[p]);
  const size_t row_words = 2 * (size_t)n;
  for (int kt = kt0; kt < kt1; ++kt)
    for (int ng = 0; ng < n / 64; ++ng)
      for (int wi = 0; wi < 128; ++wi) {
        const int c = wi >> 4, kq = (wi >> 2) & 3, jt = wi & 3;
        const size_t widx = (size_t)kt * row_words + 128 * (size_t)ng + wi;
        if constexpr (PACK) {
          unsigned w = 0;
          for (int p = 0; p < 8; ++p)
            w |= ((unsigned)codes_in[(size_t)(16 * kt + 4 * kq + pr[p]) * n + 64 * ng + 16 * jt + 8 * pb[p] + c] & 0xFu)
                 << (4 * p);
          B_out[widx] = w;
        } else {
          const unsigned w = B_in[widx];
          for (int p = 0; p < 8; ++p) {
            const int u = (int)((w >> (4 * p)) & 0xFu);
            codes_out[(size_t)(16 * kt + 4 * kq + pr[p]) * n + 64 * ng + 16 * jt + 8 * pb[p] + c] =
                (int8_t)((grouped || u < 8) ? u : u - 16);
          }
        }
      }
}

template <bool PACK>
static int pack_entry(const void* src, void* dst, int k, int n, int grouped, int on_device, int dev, void* stream) {
  g_err[0] = 0;
  if (k == 0 || n == 0) return QQQ_OK;
  if (!src || !dst || k < 0 || n < 0 || (k % 16) != 0 || (n % 64) != 0 || (k / 16) > 65535 ||
      ((uintptr_t)src & 7) != 0 || ((uintptr_t)dst & 7) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_%spack_int4: need k %% 16 == 0 (k <= 1048560), n %% 64 == 0, 8-byte aligned buffers",
             PACK ? "" : "un");
    return QQQ_ERR_ARG;
  }
  if (on_device) {
    DeviceGuard guard(dev);
    const dim3 grid(n / 64, k / 16);
    if constexpr (PACK)
      hipLaunchKernelGGL(qqq_pack_int4_kernel, grid, dim3(128), 0, static_cast<hipStream_t>(stream),
                         static_cast<const int8_t*>(src), static_cast<unsigned*>(dst), n, grouped);
    else
      hipLaunchKernelGGL(qqq_unpack_int4_kernel, grid, dim3(128), 0, static_cast<hipStream_t>(stream),
                         static_cast<const unsigned*>(src), static_cast<int8_t*>(dst), n, grouped);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, PACK ? "qqq_pack_int4_kernel launch" : "qqq_unpack_int4_kernel launch");
    return QQQ_OK;
  }
  const int kts = k / 16;
  unsigned hw = std::thread::hardware_concurrency();
  int nthr = (int)(hw ? hw : 1);
  if (nthr > 32) nthr = 32;
  if ((long long)k * n < (1 << 20)) nthr = 1;
  if (nthr > kts) nthr = kts;
  auto work = [&](int t) {
    const int kt0 = (int)((long long)kts * t / nthr), kt1 = (int)((long long)kts * (t + 1) / nthr);
    pack_host_range<PACK>(static_cast<const int8_t*>(src), static_cast<int8_t*>(dst), static_cast<const unsigned*>(src),
                          static_cast<unsigned*>(dst), n, grouped, kt0, kt1);
  };
  if (nthr == 1) {
    work(0);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < nthr; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
  }
  return QQQ_OK;
}

extern "C" int qqq_pack_int4(const void* codes, void* B, int k, int n, int grouped, int on_device, int dev, void* stream) {
  return pack_entry<true>(codes, B, k, n, grouped, on_device, dev, stream);
}

extern "C" int qqq_unpack_int4(const void* B, void* codes, int k, int n, int grouped, int on_device, int dev, void* stream) {
  return pack_entry<false>(B, codes, k, n, grouped, on_device, dev, stream);
}

extern "C" int qqq_amd_abi_version(void) { return QQQ_AMD_ABI_VERSION; }
extern "C" const char* qqq_amd_last_error(void) { return g_err; }

#ifdef QQQ_PANEL_TRACE
// measurement builds only (see qqq_panel.hip.h): where the panel kernel's phase clocks go
extern "C" int qqq_trace_set(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(qqq_trace_buf), &p, sizeof p); }
#endif
