// Pooled correspondence rows -> slot, for the kernels that are launched over `capacity` rows
// and find their work on the device (corresp_order.hip, mesh_project.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace epos {

__device__ __forceinline__ int64_t clamp_row(int64_t v, int64_t cap) {
  return v < 0 ? 0 : v > cap ? cap : v;
}

// The segment (slot) that holds pooled row g: the last s with seg[s] <= g. Empty slots
// share their bound with a neighbour and are never returned. seg[0] <= g < seg[S] (clamped).
__device__ __forceinline__ int find_slot(const int64_t* __restrict__ seg, int S, int64_t cap,
                                         int64_t g) {
  int lo = 0, hi = S;                  // answer in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clamp_row(seg[mid], cap) <= g) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace epos
