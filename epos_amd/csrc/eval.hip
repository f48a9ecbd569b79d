// Evaluation reductions (include/epos_hip.h, "Evaluation"; DESIGN.md, "Evaluation"): the
// per-pixel confusion matrix of a ground-truth label map against the predicted one
// (eval_utils.py:52-87 of the reference), and per-object fragment hit counts.
//
// Everything is an integer sum, so the tables do not depend on the launch order and
// tests/helpers/eval_ref.py equals them exactly. Both kernels ADD into their tables: the caller
// clears them once per evaluation and accumulates over every batch without a host round trip.
//
// Counting scheme of both kernels: a workgroup owns a contiguous share of the pixels, counts
// into a private table of 32-bit counters in LDS, and at the end adds every non-zero cell to the
// 64-bit table in global memory with one atomic each (`bad`: one per wavefront). A share is at
// most 2^14 (confusion) or 2^16 (fragment hits) pixels, so a 32-bit counter cannot wrap.
// Confusion matrices of more than CONF_LDS_MAX_CLS classes do not fit a private table: their
// pixels go to the global table directly, one 64-bit atomic per distinct cell and wavefront
// step.
#include "common.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int EVAL_THREADS = 256;
// 128 x 128 32-bit counters = 64 KB, the LDS a launch gets without asking for more
constexpr int CONF_LDS_MAX_CLS = 128;
constexpr int64_t CONF_SHARE_MIN = 1024, CONF_SHARE_MAX = int64_t(1) << 14;
constexpr int64_t CONF_TARGET_BLOCKS = 256;        // one workgroup per CU before shares grow
constexpr int64_t FRAG_SHARE_MIN = 256, FRAG_SHARE_MAX = int64_t(1) << 16;
constexpr int64_t FRAG_TARGET_BLOCKS = 1024;
constexpr int FRAG_MAX_OBJS = 4095;                // 3 * (O + 1) counters = 48 KB of LDS
constexpr int64_t EVAL_MAX_PIXELS = int64_t(1) << 40;

// pixels per workgroup: P spread over `target` workgroups, in whole passes of the workgroup,
// within [lo, hi]
inline int64_t pixel_share(int64_t P, int64_t target, int64_t lo, int64_t hi) {
  const int64_t s = round_up(ceil_div(P, target), EVAL_THREADS);
  return s < lo ? lo : s > hi ? hi : s;
}

__device__ __forceinline__ void add_u64(int64_t* p, unsigned v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v));
}

// cell index of a pixel, -1 = skipped (ignored), -2 = outside the table
__device__ __forceinline__ int conf_cell(int32_t g, int64_t q, int num_cls, int ignore_label) {
  if (g == ignore_label) return -1;
  if (g < 0 || g >= num_cls || q < 0 || q >= num_cls) return -2;
  return g * num_cls + static_cast<int>(q);
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(EVAL_THREADS) void confusion_kernel(
    const int32_t* __restrict__ gt, const int64_t* __restrict__ pred, int64_t P, int64_t share,
    int num_cls, int ignore_label, int64_t* cm, int64_t* bad) {
  extern __shared__ unsigned conf_tab[];          // LDS_TABLE: [num_cls * num_cls]
  const int cells = num_cls * num_cls;
  if (LDS_TABLE)
    for (int i = threadIdx.x; i < cells; i += EVAL_THREADS) conf_tab[i] = 0u;
  __syncthreads();
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * share;
  const int64_t p1 = p0 + share < P ? p0 + share : P;
  unsigned n_bad = 0;
  const int lane = threadIdx.x & 63;
  for (int64_t base = p0; base < p1; base += EVAL_THREADS) {   // the same trips for every lane
    const int64_t p = base + threadIdx.x;
    const int cell = p < p1 ? conf_cell(gt[p], pred[p], num_cls, ignore_label) : -1;
    if (cell == -2) ++n_bad;
    if (LDS_TABLE) {
      if (cell >= 0) atomicAdd(&conf_tab[cell], 1u);
    } else {
      // the lanes of a wavefront that hit one cell send one atomic between them; `todo` is the
      // same in every lane, so the loop does not diverge
      unsigned long long todo = __ballot(cell >= 0);
      while (todo) {
        const int src = __ffsll(static_cast<long long>(todo)) - 1;
        const int lead = __shfl(cell, src);
        const unsigned long long peers = __ballot(cell == lead);
        if (lane == src) add_u64(cm + lead, static_cast<unsigned>(__popcll(peers)));
        todo &= ~peers;
      }
    }
  }
  // the whole 64 KB of LDS may be the table: `bad` is summed over each wavefront in registers
  n_bad = wave_sum(n_bad);
  if (lane == 0 && n_bad) add_u64(bad, n_bad);
  __syncthreads();
  if (LDS_TABLE)
    for (int i = threadIdx.x; i < cells; i += EVAL_THREADS) {
      const unsigned v = conf_tab[i];
      if (v) add_u64(cm + i, v);
    }
}

// A NaN compares as -inf, so it never beats a number.
__device__ __forceinline__ void take(float v, int f, float& best, int& arg) {
  v = v == v ? v : -INFINITY;
  if (v > best || (v == best && f < arg)) { best = v; arg = f; }
}

// L lanes share one pixel, each reading four consecutive confidences per step (one 16-byte
// load when VEC), so a wavefront takes 64 / L pixels at a time: 4 at F = 64, 64 at F <= 4.
// Background, ignored and out-of-range pixels read no confidence.
template <bool VEC>
__global__ __launch_bounds__(EVAL_THREADS) void frag_hits_kernel(
    const int32_t* __restrict__ gt_obj, const int32_t* __restrict__ gt_frag,
    const int64_t* __restrict__ pred_obj, const float* __restrict__ conf, int64_t P,
    int64_t share, int num_objs, int num_frags, int ignore_label, int L, int64_t* counts) {
  extern __shared__ unsigned frag_tab[];          // [(num_objs + 1) * 3]
  const int cells = (num_objs + 1) * 3;
  for (int i = threadIdx.x; i < cells; i += EVAL_THREADS) frag_tab[i] = 0u;
  __syncthreads();
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * share;
  const int64_t p1 = p0 + share < P ? p0 + share : P;
  const int sub = threadIdx.x % L;                // L is a power of two <= 64
  const int per_pass = EVAL_THREADS / L;
  for (int64_t base = p0; base < p1; base += per_pass) {   // uniform trip count: shuffles below
    const int64_t p = base + threadIdx.x / L;
    int o = 0;
    if (p < p1) {
      o = gt_obj[p];
      if (o == ignore_label || o < 1 || o > num_objs) o = 0;
    }
    float best = -INFINITY;
    int arg = 0x7fffffff;
    if (o) {
      const float* row = conf + (p * num_objs + (o - 1)) * num_frags;
      for (int f = 4 * sub; f < num_frags; f += 4 * L) {
        if (VEC) {
          const float4 v = *reinterpret_cast<const float4*>(row + f);
          take(v.x, f, best, arg);
          take(v.y, f + 1, best, arg);
          take(v.z, f + 2, best, arg);
          take(v.w, f + 3, best, arg);
        } else {
          for (int k = 0; k < 4 && f + k < num_frags; ++k) take(row[f + k], f + k, best, arg);
        }
      }
    }
    for (int d = 1; d < L; d <<= 1) {             // butterfly inside the pixel's L lanes
      const float ob = __shfl_xor(best, d);
      const int oa = __shfl_xor(arg, d);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (o && sub == 0) {
      const bool hit = arg == gt_frag[p];
      atomicAdd(&frag_tab[3 * o], 1u);
      if (hit) atomicAdd(&frag_tab[3 * o + 1], 1u);
      if (hit && pred_obj && pred_obj[p] == o) atomicAdd(&frag_tab[3 * o + 2], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += EVAL_THREADS) {
    const unsigned v = frag_tab[i];
    if (v) add_u64(counts + i, v);
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_eval_lds_max_cls(void) { return CONF_LDS_MAX_CLS; }

extern "C" int epos_eval_confusion(const int32_t* gt_label, const int64_t* pred_label, int64_t P,
                                   int num_cls, int ignore_label, int64_t* cm, int64_t* bad,
                                   void* stream) {
  EPOS_REQUIRE(P >= 0 && P <= EVAL_MAX_PIXELS, "P must be in 0..2^40");
  EPOS_REQUIRE(num_cls >= 1 && num_cls <= 256, "num_cls must be in 1..256");
  if (P == 0) return EPOS_OK;
  EPOS_REQUIRE(gt_label && pred_label && cm && bad, "null pointer");
  const int64_t share = pixel_share(P, CONF_TARGET_BLOCKS, CONF_SHARE_MIN, CONF_SHARE_MAX);
  const dim3 grid(static_cast<unsigned>(ceil_div(P, share)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_cls <= CONF_LDS_MAX_CLS) {
    const size_t lds = sizeof(unsigned) * num_cls * num_cls;
    hipLaunchKernelGGL(confusion_kernel<true>, grid, dim3(EVAL_THREADS), lds, s, gt_label,
                       pred_label, P, share, num_cls, ignore_label, cm, bad);
  } else {
    hipLaunchKernelGGL(confusion_kernel<false>, grid, dim3(EVAL_THREADS), 0, s, gt_label,
                       pred_label, P, share, num_cls, ignore_label, cm, bad);
  }
  return launch_status("confusion_kernel");
}

extern "C" int epos_eval_frag_hits(const int32_t* gt_obj_label, const int32_t* gt_frag_label,
                                   const int64_t* pred_obj_label, const float* pred_frag_conf,
                                   int64_t P, int num_objs, int num_frags, int ignore_label,
                                   int64_t* counts, void* stream) {
  EPOS_REQUIRE(P >= 0 && P <= EVAL_MAX_PIXELS, "P must be in 0..2^40");
  EPOS_REQUIRE(num_objs >= 1 && num_objs <= FRAG_MAX_OBJS, "num_objs must be in 1..4095");
  EPOS_REQUIRE(num_frags >= 1 && num_frags <= 256, "num_frags must be in 1..256");
  if (P == 0) return EPOS_OK;
  EPOS_REQUIRE(gt_obj_label && gt_frag_label && pred_frag_conf && counts, "null pointer");
  int L = 1;
  while (4 * L < num_frags) L <<= 1;              // 1..64 lanes per pixel
  const int64_t share = pixel_share(P, FRAG_TARGET_BLOCKS, FRAG_SHARE_MIN, FRAG_SHARE_MAX);
  const dim3 grid(static_cast<unsigned>(ceil_div(P, share)));
  const size_t lds = sizeof(unsigned) * 3 * (num_objs + 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = num_frags % 4 == 0 && reinterpret_cast<uintptr_t>(pred_frag_conf) % 16 == 0;
  if (vec) {
    hipLaunchKernelGGL(frag_hits_kernel<true>, grid, dim3(EVAL_THREADS), lds, s, gt_obj_label,
                       gt_frag_label, pred_obj_label, pred_frag_conf, P, share, num_objs,
                       num_frags, ignore_label, L, counts);
  } else {
    hipLaunchKernelGGL(frag_hits_kernel<false>, grid, dim3(EVAL_THREADS), lds, s, gt_obj_label,
                       gt_frag_label, pred_obj_label, pred_frag_conf, P, share, num_objs,
                       num_frags, ignore_label, L, counts);
  }
  return launch_status("frag_hits_kernel");
}
