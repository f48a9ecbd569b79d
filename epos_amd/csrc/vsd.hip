// VSD counts (include/epos_hip.h, "VSD"; DESIGN.md, "VSD"): per (ground truth, estimate) pair
// the pixel counts that the Visible Surface Discrepancy of BOP'19 is made of -- the two
// rendered masks, their visibility masks against the test depth image, the intersection and
// union of those, and for every tau the intersection pixels whose normalised distance
// difference reaches it.
//
// Per pixel everything is fp64 from + - * / sqrt without FMA (the build sets
// -ffp-contract=off) in the order the header writes down, and every output is an integer count.
// A result is therefore a function of the input alone, never of the grid, the row split or the
// arrival order of the atomics, and tests/helpers/vsd_ref.py equals it exactly.
//
// One launch on the caller's stream after a clear of the counters: a grid of (pairs x
// VSD_BANDS) workgroups of four wavefronts. Row r of a pair's window belongs to wavefront
// r mod (VSD_BANDS * 4) of the pair; a wavefront walks its rows 64 pixels at a time, so the
// three loads are coalesced along x. Each lane keeps its 6 + n_taus counters in registers;
// they are summed over the wavefront by shuffles, over the workgroup through LDS, and every
// non-zero sum goes to the pair's row with one 64-bit atomic add.
#include <math.h>

#include "common.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int VSD_THREADS = 256;
constexpr int VSD_WAVES = VSD_THREADS / 64;
#ifndef EPOS_VSD_BANDS
#define EPOS_VSD_BANDS 8                           // tools/bench_vsd.py times other values
#endif
constexpr int VSD_BANDS = EPOS_VSD_BANDS;          // workgroups per pair
constexpr int VSD_ROW_STEP = VSD_BANDS * VSD_WAVES;  // rows of a window walked side by side
constexpr int VSD_MAX_TAUS = 16;
constexpr int VSD_FIXED = 6;                       // counters in front of the per-tau ones
constexpr int VSD_MAX_COUNTERS = VSD_FIXED + VSD_MAX_TAUS;

struct VsdTaus {
  double v[VSD_MAX_TAUS];
};

__global__ __launch_bounds__(VSD_THREADS) void vsd_counts_kernel(
    const float* __restrict__ depth_test, const float* __restrict__ depth_model, int h, int w,
    const EposVsdPair* __restrict__ pairs, double delta, VsdTaus taus, int n_taus,
    int64_t* counts) {
  __shared__ unsigned red[VSD_WAVES][VSD_MAX_COUNTERS];
  const int pair = blockIdx.x / VSD_BANDS, band = blockIdx.x % VSD_BANDS;
  const EposVsdPair& pr = pairs[pair];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x0 = pr.x0, x1 = pr.x1, y1 = pr.y1;
  const int64_t hw = static_cast<int64_t>(h) * w;
  const float* T = depth_test + pr.image * hw;
  const float* G = depth_model + pr.gt_inst * hw;
  const bool has_est = pr.est_inst >= 0;
  const float* E = depth_model + (has_est ? pr.est_inst : 0) * hw;
  const double fx = pr.fx, fy = pr.fy, cx = pr.cx, cy = pr.cy, diameter = pr.diameter;

  // a lane sees fewer than h * w < 2^31 pixels: 32 bits hold every one of its counters
  unsigned c[VSD_FIXED] = {0u, 0u, 0u, 0u, 0u, 0u};
  unsigned ge[VSD_MAX_TAUS];
#pragma unroll
  for (int k = 0; k < VSD_MAX_TAUS; ++k) ge[k] = 0u;

  for (int y = pr.y0 + band * VSD_WAVES + wave; y < y1; y += VSD_ROW_STEP) {
    const double ry = ((static_cast<double>(y) + 0.5) - cy) / fy;
    const double ry2 = ry * ry;
    const int64_t row = static_cast<int64_t>(y) * w;
    for (int x = x0 + lane; x < x1; x += 64) {
      const double zt = static_cast<double>(T[row + x]);
      const double zg = static_cast<double>(G[row + x]);
      const double ze = has_est ? static_cast<double>(E[row + x]) : 0.0;
      const bool mask_g = zg > 0.0, mask_e = ze > 0.0;
      if (!(mask_g || mask_e)) continue;           // no counter moves
      const bool missing = !(zt > 0.0);
      const double rx = ((static_cast<double>(x) + 0.5) - cx) / fx;
      const double s = sqrt((rx * rx + ry2) + 1.0);
      const double dt = zt * s, dg = zg * s, de = ze * s;
      const bool vis_g = mask_g && (missing || dg - dt <= delta);
      const bool vis_e = mask_e && (missing || de - dt <= delta || vis_g);
      const bool inter = vis_g && vis_e;
      c[0] += mask_g;
      c[1] += vis_g;
      c[2] += mask_e;
      c[3] += vis_e;
      c[4] += inter;
      c[5] += (vis_g || vis_e);
      if (inter) {
        const double d = fabs(dg - de) / diameter;
#pragma unroll
        for (int k = 0; k < VSD_MAX_TAUS; ++k)
          if (k < n_taus) ge[k] += (d >= taus.v[k]);
      }
    }
  }

#pragma unroll
  for (int k = 0; k < VSD_FIXED; ++k) {
    const unsigned v = wave_sum(c[k]);
    if (lane == 0) red[wave][k] = v;
  }
#pragma unroll
  for (int k = 0; k < VSD_MAX_TAUS; ++k) {
    const unsigned v = wave_sum(ge[k]);
    if (lane == 0) red[wave][VSD_FIXED + k] = v;
  }
  __syncthreads();
  const int n_counters = VSD_FIXED + n_taus;
  if (static_cast<int>(threadIdx.x) < n_counters) {
    unsigned long long v = 0;
    for (int wv = 0; wv < VSD_WAVES; ++wv) v += red[wv][threadIdx.x];
    if (v)
      atomicAdd(reinterpret_cast<unsigned long long*>(
                    counts + static_cast<int64_t>(pair) * n_counters + threadIdx.x), v);
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_vsd_max_taus(void) { return VSD_MAX_TAUS; }
extern "C" int epos_vsd_row_bands(void) { return VSD_ROW_STEP; }

extern "C" int epos_vsd_counts(const float* depth_test, int n_images, const float* depth_model,
                               int n_inst, int h, int w, const EposVsdPair* pairs,
                               EposVsdPair* pairs_dev, int n_pairs, double delta,
                               const double* taus, int n_taus, int64_t* counts, void* stream) {
  EPOS_REQUIRE(n_pairs >= 0, "n_pairs must be >= 0");
  EPOS_REQUIRE(n_taus >= 1 && n_taus <= VSD_MAX_TAUS, "n_taus must be in 1..16");
  EPOS_REQUIRE(isfinite(delta), "delta must be finite");
  EPOS_REQUIRE(n_images >= 0 && n_inst >= 0 && h >= 0 && w >= 0, "negative size");
  // two ints cannot overflow an int64; the third factor is compared, not multiplied in
  const int64_t hw = static_cast<int64_t>(h) * w, lim = (int64_t(1) << 31) - 1;
  EPOS_REQUIRE(hw <= lim, "h * w must be < 2^31");
  EPOS_REQUIRE(hw == 0 || n_inst <= lim / hw, "n_inst * h * w must be < 2^31");
  if (n_pairs == 0) return EPOS_OK;
  EPOS_REQUIRE(depth_test && depth_model && pairs && pairs_dev && taus && counts,
               "null pointer");
  EPOS_REQUIRE(static_cast<int64_t>(n_pairs) * VSD_BANDS < (int64_t(1) << 31),
               "n_pairs * workgroups per pair must be < 2^31");
  VsdTaus tv;
  for (int k = 0; k < VSD_MAX_TAUS; ++k) tv.v[k] = k < n_taus ? taus[k] : 0.0;
  for (int i = 0; i < n_pairs; ++i) {
    const EposVsdPair& p = pairs[i];
    EPOS_REQUIRE(p.image >= 0 && p.image < n_images, "image outside [0, n_images)");
    EPOS_REQUIRE(p.gt_inst >= 0 && p.gt_inst < n_inst, "gt_inst outside [0, n_inst)");
    EPOS_REQUIRE(p.est_inst >= -1 && p.est_inst < n_inst,
                 "est_inst is neither -1 nor inside [0, n_inst)");
    EPOS_REQUIRE(p.x0 >= 0 && p.x0 <= p.x1 && p.x1 <= w, "window outside [0, w] or x1 < x0");
    EPOS_REQUIRE(p.y0 >= 0 && p.y0 <= p.y1 && p.y1 <= h, "window outside [0, h] or y1 < y0");
    EPOS_REQUIRE(isfinite(p.diameter) && p.diameter > 0.0, "diameter must be finite and > 0");
    EPOS_REQUIRE(isfinite(p.fx) && p.fx != 0.0 && isfinite(p.fy) && p.fy != 0.0,
                 "fx and fy must be finite and non-zero");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = check_hip(hipMemcpyAsync(pairs_dev, pairs, sizeof(EposVsdPair) * n_pairs,
                                    hipMemcpyHostToDevice, s), "pair table upload");
  if (rc != EPOS_OK) return rc;
  rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * n_pairs * (VSD_FIXED + n_taus), s),
                 "counter clear");
  if (rc != EPOS_OK) return rc;
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(n_pairs) * VSD_BANDS));
  hipLaunchKernelGGL(vsd_counts_kernel, grid, dim3(VSD_THREADS), 0, s, depth_test, depth_model,
                     h, w, pairs_dev, delta, tv, n_taus, counts);
  return launch_status("vsd_counts_kernel");
}
