// What the loss reduction (loss.hip) and its gradient (loss_grad.hip) share: the limits, the
// class of a pixel, and the row scheme -- L lanes share a pixel's row, each lane adds its own
// values in index order, the lanes' partial sums are added in a butterfly.
#pragma once
#include <math.h>

#include "common.h"

namespace epos {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_OBJS = 4095, LOSS_MAX_FRAGS = 256;
constexpr int64_t LOSS_MAX_PIXELS = int64_t(1) << 31;
constexpr int64_t LOSS_MAX_BLOCKS = (int64_t(1) << 31) - 1;

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

// The class of pixel p: 0..O, CODE_IGNORED or CODE_BAD; the ignore rule first. f and wgt are
// read for a foreground pixel only.
__device__ __forceinline__ int pixel_class(const int32_t* __restrict__ gt_obj,
                                           const int32_t* __restrict__ gt_frag,
                                           const float* __restrict__ gt_weight, int64_t p,
                                           int num_objs, int num_frags, int ignore_label, int& f,
                                           float& wgt) {
  int g = gt_obj[p];
  if (g == ignore_label) {
    g = CODE_IGNORED;
  } else if (g < 0 || g > num_objs) {
    g = CODE_BAD;
  } else if (g > 0) {
    f = gt_frag[p];
    wgt = gt_weight[p];
    // !(w > 0) is true for a NaN; an infinite weight is refused as well
    if (f < 0 || f >= num_frags || !(wgt > 0.f) || wgt == INFINITY) g = CODE_BAD;
  }
  return g;
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

}  // namespace epos
