// What the loss reduction (loss.hip), its gradient (loss_grad.hip) and the logits layers' weight
// and input gradients (heads_wgrad.hip, heads_dgrad.hip) share, each rule stated once: the
// limits and entry checks, the class of a pixel, the row scheme -- L lanes share a pixel's row,
// each lane adds its own values in index order, the lanes' partial sums are added in a
// butterfly --, what phase one leaves of a pixel, and the value of one gradient element: fp64
// on the fp32 values, one product for s_k, rounded to float last. A foreground pixel carries knn
// slots (fragment, weight): the k nearest fragments of include/epos_hip.h, "k nearest fragments".
#pragma once
#include <math.h>

#include <initializer_list>

#include "common.h"

namespace epos {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_OBJS = 4095, LOSS_MAX_FRAGS = 256;
constexpr int64_t LOSS_MAX_PIXELS = int64_t(1) << 31;
constexpr int64_t LOSS_MAX_BLOCKS = (int64_t(1) << 31) - 1;
constexpr int HEADS_MAX_K = 1024;            // feature channels of the logits layers
// fragments per foreground pixel, at most (include/epos_hip.h, "k nearest fragments")
constexpr int LOSS_MAX_KNN = EPOS_LOSS_MAX_KNN;

// classes of a pixel slot in LDS besides 0..O
constexpr int CODE_IGNORED = -1, CODE_BAD = -2, CODE_NONE = -3;

// lanes per pixel: 1 for F <= 4, else the power of two with 2L < F <= 4L (1..64)
inline int loss_lanes(int num_frags) {
  int L = 1;
  while (4 * L < num_frags) L <<= 1;
  return L;
}

// `share` = pixels per workgroup of the launch that follows
inline int check_loss_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags,
                           int64_t share) {
  const char* msg = nullptr;
  if (B < 0) msg = "B must be >= 0";
  else if (P < 0 || P > LOSS_MAX_PIXELS) msg = "P must be in 0..2^31";
  else if (num_objs < 1 || num_objs > LOSS_MAX_OBJS) msg = "num_objs must be in 1..4095";
  else if (num_frags < 1 || num_frags > LOSS_MAX_FRAGS) msg = "num_frags must be in 1..256";
  else if (B > 0 && P > 0 && ceil_div(P, share) > LOSS_MAX_BLOCKS / B)
    msg = "B * workgroups per image must be below 2^31";
  else if (B > 65535) msg = "B must be <= 65535";
  if (!msg) return EPOS_OK;
  set_error("%s: %s", fn, msg);
  return EPOS_E_INVALID;
}

// 1 <= knn <= min(F, LOSS_MAX_KNN); F is checked before
inline int check_knn(const char* fn, int knn, int num_frags) {
  if (knn >= 1 && knn <= LOSS_MAX_KNN && knn <= num_frags) return EPOS_OK;
  set_error("%s: knn must be in 1..min(num_frags, %d)", fn, LOSS_MAX_KNN);
  return EPOS_E_INVALID;
}

// check_loss_dims and the limit of K, for the entries that read or write the features
inline int check_heads_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags,
                            int64_t share, int K) {
  const int rc = check_loss_dims(fn, B, P, num_objs, num_frags, share);
  if (rc != EPOS_OK) return rc;
  if (K < 1 || K > HEADS_MAX_K) {
    set_error("%s: K must be in 1..1024", fn);
    return EPOS_E_INVALID;
  }
  return EPOS_OK;
}

// EPOS_E_INVALID when an output starts at an input pointer; null pointers are skipped
inline int check_no_alias(const char* fn, std::initializer_list<const void*> inputs,
                          std::initializer_list<const void*> outputs) {
  for (const void* in : inputs)
    for (const void* out : outputs)
      if (in && in == out) {
        set_error("%s: %s output buffer starts at an input pointer", fn,
                  outputs.size() == 1 ? "the" : "an");
        return EPOS_E_INVALID;
      }
  return EPOS_OK;
}

// The kernels of the family are compiled for SLOTS = 1 and SLOTS = LOSS_MAX_KNN slots per pixel:
// with one slot knn is the constant 1 and the code is what it was before there were slots.
template <int SLOTS>
__device__ __forceinline__ int slots_of(int knn) { return SLOTS == 1 ? 1 : knn; }
// the launch for knn: SLOTS = 1 or LOSS_MAX_KNN
#define EPOS_FOR_SLOTS(knn, LAUNCH)                  \
  do {                                               \
    if ((knn) == 1) { LAUNCH(1); }                   \
    else { LAUNCH(::epos::LOSS_MAX_KNN); }           \
  } while (0)

// The class of pixel p: 0..O, CODE_IGNORED or CODE_BAD; the ignore rule first. The knn slots
// f[j], wgt[j] are read for a foreground pixel only; the arrays are indexed by unrolled loops
// alone, so they stay in registers.
template <int SLOTS>
__device__ __forceinline__ int pixel_class(const int32_t* __restrict__ gt_obj,
                                           const int32_t* __restrict__ gt_frag,
                                           const float* __restrict__ gt_weight, int64_t p,
                                           int num_objs, int num_frags, int ignore_label, int knn,
                                           int (&f)[SLOTS], float (&wgt)[SLOTS]) {
  int g = gt_obj[p];
  if (g == ignore_label) {
    g = CODE_IGNORED;
  } else if (g < 0 || g > num_objs) {
    g = CODE_BAD;
  } else if (g > 0) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
      if (j >= knn) continue;
      f[j] = gt_frag[p * knn + j];
      wgt[j] = gt_weight[p * knn + j];
      // !(w > 0) is true for a NaN; an infinite weight is refused as well
      bad |= f[j] < 0 || f[j] >= num_frags || !(wgt[j] > 0.f) || wgt[j] == INFINITY;
#pragma unroll
      for (int i = 0; i < j; ++i) bad |= f[i] == f[j];       // two slots, one fragment
    }
    if (bad) g = CODE_BAD;
  }
  return g;
}

// The class alone
template <int SLOTS>
__device__ __forceinline__ int pixel_class(const int32_t* __restrict__ gt_obj,
                                           const int32_t* __restrict__ gt_frag,
                                           const float* __restrict__ gt_weight, int64_t p,
                                           int num_objs, int num_frags, int ignore_label,
                                           int knn) {
  int f[SLOTS];
  float wgt[SLOTS];
  return pixel_class<SLOTS>(gt_obj, gt_frag, gt_weight, p, num_objs, num_frags, ignore_label,
                            knn, f, wgt);
}

// The lane's part of a row of n values: four consecutive values per step, steps 4 * L apart
// (one 16-byte load per whole quad when VEC). fn(value) is called in index order.
template <bool VEC, typename Fn>
__device__ __forceinline__ void for_lane_values(const float* __restrict__ row, int n, int sub,
                                                int L, Fn fn) {
  for (int c = 4 * sub; c < n; c += 4 * L) {
    if (VEC && c + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(row + c);
      fn(v.x); fn(v.y); fn(v.z); fn(v.w);
    } else {
      for (int k = 0; k < 4 && c + k < n; ++k) fn(row[c + k]);
    }
  }
}

// m = max x and s = sum_c exp(x_c - m) of the row the L lanes of a pixel share; every lane of
// the L takes part (inactive pixels with active = false: they read nothing) and every lane
// holds the result. The lanes' partial sums are added in a butterfly, each lane's own values
// in index order.
template <bool VEC>
__device__ __forceinline__ void row_max_sum(const float* __restrict__ row, int n, bool active,
                                            int sub, int L, double& md, double& s) {
  float m = -INFINITY;
  if (active) for_lane_values<VEC>(row, n, sub, L, [&](float v) { m = fmaxf(m, v); });
  for (int d = 1; d < L; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  md = static_cast<double>(m);
  const double mm = md;
  double acc = 0.0;
  if (active)
    for_lane_values<VEC>(row, n, sub, L,
                         [&](float v) { acc += exp(static_cast<double>(v) - mm); });
  for (int d = 1; d < L; d <<= 1) acc += __shfl_xor(acc, d);
  s = acc;
}

// Where the F fragment logits of foreground pixel p (of the whole batch) and object g start;
// three times that, its localisation values
__device__ __forceinline__ int64_t frag_row_offset(int64_t p, int num_objs, int g,
                                                   int num_frags) {
  return (p * num_objs + (g - 1)) * num_frags;
}

// What phase one leaves of a pixel: its class, fragments and weights (pixel_class), m and S of
// its object row (class >= 0) and of its fragment row (class > 0)
template <int SLOTS>
struct PixelRows {
  int code, frag[SLOTS];
  float wgt[SLOTS];
  double m_obj, s_obj, m_frag, s_frag;       // m is an fp32 value
};

// Phase one of pixel p for the L lanes that share it (all of them call, `valid` or not: the
// shuffles of row_max_sum); a row that is not wanted is not read and leaves m = S = 0.
template <int SLOTS, bool VEC_OBJ, bool VEC_FRAG>
__device__ __forceinline__ PixelRows<SLOTS> pixel_rows(
    const float* __restrict__ obj_logits, int64_t ld_obj, const float* __restrict__ frag_logits,
    const int32_t* __restrict__ gt_obj, const int32_t* __restrict__ gt_frag,
    const float* __restrict__ gt_weight, int64_t p, bool valid, int num_objs, int num_frags,
    int ignore_label, int knn, bool want_obj, bool want_frag, int sub, int L) {
  PixelRows<SLOTS> r = {CODE_NONE, {}, {}, 0.0, 0.0, 0.0, 0.0};     // slots: 0, 0.f
  if (valid)
    r.code = pixel_class<SLOTS>(gt_obj, gt_frag, gt_weight, p, num_objs, num_frags,
                                ignore_label, knn, r.frag, r.wgt);
  if (want_obj)
    row_max_sum<VEC_OBJ>(obj_logits + (r.code >= 0 ? p * ld_obj : 0), num_objs + 1, r.code >= 0,
                         sub, L, r.m_obj, r.s_obj);
  if (want_frag)
    row_max_sum<VEC_FRAG>(
        frag_logits + (r.code > 0 ? frag_row_offset(p, num_objs, r.code, num_frags) : 0),
        num_frags, r.code > 0, sub, L, r.m_frag, r.s_frag);
  return r;
}

// Phase one of a share of N pixels at most, in LDS
template <int N, int SLOTS>
struct ShareRows {
  double s_obj[N], s_frag[N];                // S of the two rows
  float m_obj[N], m_frag[N];                 // m of the two rows
  float wgt[N][SLOTS];
  int code[N], frag[N][SLOTS];

  __device__ __forceinline__ void put(int i, const PixelRows<SLOTS>& r, int knn) {
    code[i] = r.code;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
      if (j >= knn) continue;
      frag[i][j] = r.frag[j];
      wgt[i][j] = r.wgt[j];
    }
    m_obj[i] = static_cast<float>(r.m_obj);
    s_obj[i] = r.s_obj;
    m_frag[i] = static_cast<float>(r.m_frag);
    s_frag[i] = r.s_frag;
  }
};

// u_k: what arrives at loss k, directly and through the total; 1.0 without upstream
__device__ __forceinline__ double upstream_factor(const double* __restrict__ upstream, int k) {
  return upstream ? upstream[k] + upstream[3] : 1.0;
}

// s_k of image b = scales[b,k] * u_k, one product
__device__ __forceinline__ double task_factor(const double* __restrict__ scales, int64_t b,
                                              int k, double u_k) {
  return scales[b * 3 + k] * u_k;
}

// d loss / d x of one element of a softmax row with maximum m and sum S
__device__ __forceinline__ float softmax_grad(float x, double m, double S, bool target,
                                              double s_k) {
  const double pr = exp(static_cast<double>(x) - m) / S;
  return static_cast<float>(s_k * (pr - (target ? 1.0 : 0.0)));
}

// softmax_grad with knn assigned fragments: the probability counts once per slot, target is
// true for each of the pixel's fragments. knn == 1.0 gives softmax_grad's bytes: 1.0 * pr is pr.
__device__ __forceinline__ float softmax_grad_knn(float x, double m, double S, bool target,
                                                  double s_k, double knn) {
  const double pr = exp(static_cast<double>(x) - m) / S;
  return static_cast<float>(s_k * (knn * pr - (target ? 1.0 : 0.0)));
}

// c is one of the knn fragments at f
__device__ __forceinline__ bool is_slot(const int* f, int knn, int c) {
  bool hit = false;
  for (int j = 0; j < knn; ++j) hit |= f[j] == c;
  return hit;
}

// The Huber term of one localisation component, d = q - t ...
__device__ __forceinline__ double huber1(double d) {
  const double a = fabs(d);
  return a <= 1.0 ? 0.5 * d * d : a - 0.5;
}

// ... and its derivative, knee included: |d| <= 1 gives d
__device__ __forceinline__ float huber_grad(float q, float t, float wgt, double s_2) {
  const double d = static_cast<double>(q) - static_cast<double>(t);
  const double cl = d > 1.0 ? 1.0 : d < -1.0 ? -1.0 : d;
  return static_cast<float>(s_2 * (static_cast<double>(wgt) * cl));
}

}  // namespace epos
