// Reductions over the 64 lanes of a wavefront: the xor butterfly at distances 32, 16, 8, 4,
// 2, 1, after which every lane holds the result. ALL 64 lanes must take part. For a
// floating-point sum that order is part of the result (the fitting kernels' oracles and the
// softmax tests pin it), so it is written down here once. T = float, double, int, int64_t,
// unsigned. LANES < 64 (a power of two): the same inside each aligned group of LANES lanes,
// from distance LANES/2 down.
//
// Not here, on purpose: the butterflies over a pixel's L lanes in loss.hip and eval.hip (L is
// a run-time value; they walk 1 -> L/2, which loss.hip's sums pin), the arg-reductions that
// carry a payload with the value (corresp.hip's projection, mesh_project.hip, eval.hip's
// fragment argmax: their tie rules are their own) and reduce_scatter32 (fit_lo.h: 32
// sums at once, halving the set per level).
#pragma once
#include <type_traits>

#include "common.h"

namespace epos {
namespace {

template <int LANES, typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, LANES));
  return v;
}

template <int LANES = 64, typename T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce<LANES>(v, [](T a, T b) { return a + b; });
}

// float: fmaxf (one v_max_f32 per level; a NaN loses to a number). Every other type, and
// wave_min: by comparison, so a lane's own NaN stays and an incoming one never wins.
template <int LANES = 64, typename T>
__device__ __forceinline__ T wave_max(T v) {
  return wave_reduce<LANES>(v, [](T a, T b) {
    if constexpr (std::is_same<T, float>::value) return fmaxf(a, b);
    else return b > a ? b : a;
  });
}

template <int LANES = 64, typename T>
__device__ __forceinline__ T wave_min(T v) {
  return wave_reduce<LANES>(v, [](T a, T b) { return b < a ? b : a; });
}

}  // namespace
}  // namespace epos
