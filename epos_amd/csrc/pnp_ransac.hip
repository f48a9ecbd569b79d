// Wavefront-parallel multi-instance PnP-RANSAC for gfx950 -- replaces the pyprogressivex.
// find6DPoses call of scripts/infer.py:470-488 (the un-vendored danini/progressive-x C++ module).
// Algorithm definition: DESIGN.md "Pose fitting" (P3P minimal solver, MSAC quality, Gauss-Newton
// local optimisation of the best hypothesis, spatial-coherence labelling, sequential multi-
// instance with Tanimoto / coverage tests, joint refinement). ONE translation unit: the stages
// are in fit_work.h, fit_p3p.h, fit_lo.h, fit_label.h and fit_pearl.h; the per-round kernels that
// tie them together, the workspace, the launch sequence and the C entry points are here.
// Mapping to the hardware (one call = one launch sequence over all slots = (image, object)
// pairs of a step; everything stays on the device, DESIGN.md (f) has the measurements):
//   * ransac_init: per-call state, the sweeps' position-ordered candidate stream (static
//     geometry) and the candidate window of every tile of 64 row-sorted points.
//   Per proposal round (max_k rounds, + 2 retries in a multi-instance search):
//   * ransac_hypotheses: ONE HYPOTHESIS SET PER WAVEFRONT. The 64 lanes compute the
//     (wave-uniform) P3P solve redundantly, then stride over the slot's correspondences; the
//     MSAC sums are reduced in a canonical order (64 strided partials, xor butterfly).
//     Grid = (max_iters / 4, slots).
//   * ransac_select_lo: FOUR workgroups per slot. Deterministic arg-max over the hypothesis
//     table, then the Gauss-Newton refits on the inliers: one pass over the points per refit
//     (score of the candidate + the 27 normal-equation sums of the step from it), 1024
//     strided partials in the oracle's canonical tree -- a reduce-scatter butterfly per wave,
//     a fence-free agent-scope hand-off between the workgroups, a pivot-free 6 x 6 solve by
//     every thread; last, the fixed-point residual table the labelling starts from.
//   * ransac_gc_scan (first sweep) / ransac_gc_delta (further sweeps): the spatial-coherence
//     labelling on the 5-D neighbourhood graph. Scan: sixteen waves per tile walk the tile's
//     window with the candidate in SCALAR registers (s_load), exact integer counters. Delta:
//     only the candidates the previous sweep flipped are revisited. (ransac_gc_sweep: the
//     LDS-staged predecessor, kept as EPOS_FIT_SCAN=0 and as ransac_nb_build, which writes
//     the neighbour lists the joint refinement walks.)
//   * ransac_refit_accept: refits on the labelled set (same machinery as select_lo), the
//     instance acceptance tests on inlier bitsets (ballot + popcount), stable in-place
//     compaction of the still-unexplained correspondences by the whole workgroup.
//   * pearl_*: joint refinement of multi-instance slots (labels over all instances).
// Arithmetic is fp64 (the reference hands f64 arrays to progressive-x) using only + - * / sqrt,
// compiled with -ffp-contract=off: reproducible run to run and identical to a scalar evaluation
// in the same canonical order.
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include "fit_work.h"
#include "fit_p3p.h"
#include "fit_lo.h"
#include "fit_label.h"
#include "fit_pearl.h"

namespace epos {
namespace {

// A proposal round of slot s failed (no model, too few inliers, Tanimoto / coverage): single-
// instance search stops; the multi-instance search retries with fresh samples while the samples
// drawn since the last success have not reached confidence `conf` of having hit an instance as
// large as the last accepted one (DESIGN.md "Pose fitting").
__device__ void round_failed(int s, const Work& w, const EposFitParams& prm, int want,
                             int k, int64_t n_active) {
  const int tries = ++w.tries[s];
  bool stop = want == 1;
  if (!stop) {
    const int64_t ref = k == 0 ? prm.min_point_number : w.last_new[s];
    if (ref >= n_active) {
      stop = true;
    } else {
      const double r = static_cast<double>(ref) / static_cast<double>(n_active);
      stop = !(powi(1.0 - r * r * r, static_cast<int64_t>(tries) * prm.max_iters) >
               1.0 - prm.conf);
    }
  }
  if (stop) w.done[s] = 1;
}

__global__ __launch_bounds__(256) void ransac_init(const double* __restrict__ xy_all,
                                                   const double* __restrict__ xyz_all,
                                                   const int64_t* slot_base, int S,
                                                   Work w, int32_t* labels,
                                                   int32_t* num_models,
                                                   int min_pts, int64_t n_capacity, int n_lo,
                                                   int build_nb, int build_geo, double rad) {
  const int s = blockIdx.x;
  const bool first = blockIdx.y == 0;        // gridDim.y workgroups share the slot's rows
  if (first) {
    for (int i = threadIdx.x; i < n_lo; i += blockDim.x)
      w.lo_cnt[static_cast<int64_t>(s) * n_lo + i] = 0u;
    if (threadIdx.x == 0) w.nb_ok[s] = build_nb;
    if (s == 0 && threadIdx.x == 0) *w.lo_timeout = 0;
  }
  const int64_t base = slot_base[s];
  // A slot whose rows would end beyond the pooled arrays (the correspondence stage
  // raised its overflow flag and wrote nothing there) is fitted as EMPTY: no kernel of
  // this stage then touches a row >= n_capacity. The host reports the overflow.
  const int64_t n = slot_base[s + 1] <= n_capacity ? slot_base[s + 1] - base : 0;
  for (int64_t i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.y) {
    w.active[base + i] = static_cast<int32_t>(i);
    labels[base + i] = -1;
    if (build_geo) {                  // static geometry of the sweeps' candidate stream
      const int64_t o = w.yorder ? w.yorder[base + i] : i;
      double* g = w.geo + 4 * (base + i);
      g[0] = xy_all[2 * (base + o)]; g[1] = xy_all[2 * (base + o) + 1];
      g[2] = xyz_all[3 * (base + o)]; g[3] = xyz_all[3 * (base + o) + 1];
    }
  }
  if (build_geo) {
    // The candidate window of every tile of 64 positions -- the positions whose image row
    // can hold a neighbour of a point of the tile -- depends on the geometry only: found
    // here once per call (one wavefront per tile, 64-ary searches over the sorted rows: three
    // dependent loads per side) instead of by every sweep.
    const int lane = threadIdx.x & 63;
    const int64_t wave = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.y) * (blockDim.x >> 6);
    const int32_t* yo = w.yorder ? w.yorder + base : nullptr;
    const double* ys = xy_all + 2 * base + 1;
    int32_t* win = w.win + 2 * (base / 64 + s);
    for (int64_t tile = wave; tile * 64 < n; tile += waves) {
      const int64_t pos0 = tile * 64;
      const int64_t last = pos0 + 63 < n ? pos0 + 63 : n - 1;
      const double ylo = ys[2 * (yo ? yo[pos0] : pos0)] - rad;
      const double yhi = ys[2 * (yo ? yo[last] : last)] + rad;
      for (int side = 0; side < 2; ++side) {
        // side 0: first position in [0, pos0] with y >= ylo; side 1: first position in
        // [last + 1, n] with y > yhi   (y is non-decreasing along the sorted order)
        int64_t lo = side ? last + 1 : 0, hi = side ? n : pos0;
        while (hi - lo > 0) {
          const int64_t step = (hi - lo + 63) / 64;
          const int64_t q = lo + lane * step;
          bool pred = false;
          if (q < hi) {
            const double yq = ys[2 * (yo ? yo[q] : q)];
            pred = side ? yq > yhi : yq >= ylo;
          }
          const unsigned long long b = __ballot(pred);
          if (!b) {                 // no probe at or beyond the bound: it lies after the last
            const int64_t tv = (hi - lo - 1) / step;
            lo = lo + tv * step + 1;
          } else {                  // the bound lies in (probe[first - 1], probe[first]]
            const int f = __ffsll(static_cast<long long>(b)) - 1;
            const int64_t qf = lo + static_cast<int64_t>(f) * step;
            lo = f == 0 ? lo : lo + static_cast<int64_t>(f - 1) * step + 1;
            hi = qf;
          }
        }
        if (lane == 0) win[2 * tile + side] = static_cast<int32_t>(lo);
      }
    }
  }
  if (first && threadIdx.x == 0) {
    w.n_active[s] = static_cast<int32_t>(n);
    num_models[s] = 0;
    w.done[s] = (n < min_pts || n < 3) ? 1 : 0;      // infer.py:420-422
    w.state[s] = 0;
    w.tries[s] = 0;
    w.last_new[s] = min_pts;
  }
}

__global__ __launch_bounds__(256) void ransac_hypotheses(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const double* __restrict__ Ks,
    const uint64_t* __restrict__ seeds, const int32_t* __restrict__ max_models,
    const int32_t* __restrict__ num_models, EposFitParams prm, int max_k, int round,
    Work w) {
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int it = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (it >= prm.max_iters) return;
  double* hs = w.hyp_score + (static_cast<int64_t>(s) * prm.max_iters + it) * MAX_SOL;
  int ns = 0;
  if (!w.done[s]) {
    const int64_t base = slot_base[s];
    const double* xy = xy_all + 2 * base;
    const double* xyz = xyz_all + 3 * base;
    const int32_t* active = w.active + base;
    const int64_t n_active = w.n_active[s];
    const int64_t n = slot_base[s + 1] - base;
    double K[9];
    for (int i = 0; i < 9; ++i) K[i] = Ks[s * 9 + i];
    int64_t m = n_active;
    if (prm.use_prosac) {
      m = (n_active * static_cast<int64_t>(it + 1) + prm.max_iters - 1) / prm.max_iters;
      if (m < prm.min_point_number) m = prm.min_point_number;
      if (m < 3) m = 3;
      if (m > n_active) m = n_active;
    }
    FIT_TRACE(0, s == 0 && it == 0 && lane == 0);
    int64_t smp[3];
    sample3(seeds[s], static_cast<uint32_t>(round), static_cast<uint32_t>(it), m, smp);
    double f[9], X[9], p2[6];
    for (int j = 0; j < 3; ++j) {
      const int32_t p = active[smp[j]];
      bearing(K, xy + 2 * p, f + 3 * j);
      for (int d = 0; d < 3; ++d) X[3 * j + d] = xyz[3 * p + d];
      p2[2 * j] = xy[2 * p]; p2[2 * j + 1] = xy[2 * p + 1];
    }
    const double area = 0.5 * fabs((p2[2] - p2[0]) * (p2[5] - p2[1]) -
                                   (p2[3] - p2[1]) * (p2[4] - p2[0]));
    if (!(area < prm.min_triangle_area)) {
      double sols[MAX_SOL * 12];
      FIT_TRACE(0, s == 0 && it == 0 && lane == 0);
      ns = p3p(f, X, sols);
      FIT_TRACE(0, s == 0 && it == 0 && lane == 0);
      const double thr2 = prm.threshold * prm.threshold;
      double* hp = w.hyp_pose + (static_cast<int64_t>(s) * prm.max_iters + it) * MAX_SOL * 12;
      int32_t* hc = w.hyp_count + (static_cast<int64_t>(s) * prm.max_iters + it) * MAX_SOL;
      double sc[MAX_SOL];
      int cnt[MAX_SOL];
      // while nothing has been removed the active list is the identity (ransac_init): the
      // scoring passes then index the points directly -- one dependent load per item less
      score_poses(sols, ns, K, xy, xyz, n_active == n ? nullptr : active, n_active, thr2, lane,
                  sc, cnt);
#pragma unroll
      for (int q = 0; q < MAX_SOL; ++q) {
        if (q < ns) {
          if (lane == 0) { hs[q] = sc[q]; hc[q] = cnt[q]; }
#pragma unroll
          for (int e = 0; e < 12; ++e)
            if (lane == e) hp[q * 12 + e] = sols[12 * q + e];
        }
      }
    }
  }
  if (lane == 0)
    for (int q = ns; q < MAX_SOL; ++q) hs[q] = -1.0;     // no hypothesis
  FIT_TRACE(0, s == 0 && it == 0 && lane == 0);
}

// ---- round, step 2: best hypothesis (with the RANSAC confidence bound) + local
// optimisation (i) + the residual table and thresholded labels of the labelling step.
__global__ __launch_bounds__(256) void ransac_select_lo(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const double* __restrict__ Ks,
    const int32_t* __restrict__ max_models, EposFitParams prm, int max_k, int round,
    Work w, const int32_t* __restrict__ num_models, const int32_t* __restrict__ labels_all,
    int lo_launch, int n_lo) {
  __shared__ double s_score[256];
  __shared__ int s_index[256];
  __shared__ LoLds s_lo;
  // LO_G workgroups per slot (blockIdx.x = g: siblings are adjacent in dispatch order);
  // all of them take every decision from the same data, workgroup 0 writes the state
  const int s = blockIdx.y;
  const int g = blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0 && g == 0) w.state[s] = 0;
  FIT_TRACE(1, s == 0 && g == 0 && t == 0);
  if (w.done[s]) return;                                   // uniform over the slot
  const int want = clamp_want(max_models[s], max_k);
  const int k = num_models[s];
  const Slot sl = slot_of(slot_base, s, w, xy_all, xyz_all);
  int32_t* active = w.active + sl.base;
  const int64_t n_active = w.n_active[s];
  if (k >= want || round >= fit_rounds(want) ||
      n_active < prm.min_point_number || n_active < 3) {
    if (t == 0 && g == 0) w.done[s] = 1;
    return;
  }
  const int nh = prm.max_iters * MAX_SOL;
  const double* hs = w.hyp_score + static_cast<int64_t>(s) * nh;
  const int32_t* hcnt = w.hyp_count + static_cast<int64_t>(s) * nh;
  if (prm.proposal_engine_conf < 1.0) {
    // sequential semantics of the termination bound: the best among the hypotheses
    // drawn before (1 - w^3)^it <= 1 - conf (sequential semantics)
    if (t == 0) {
      double best = -1.0;
      int best_i = 0x7fffffff, best_c = 0;
      for (int it = 0; it < prm.max_iters; ++it) {
        if (it > 0 && best > 0.0) {
          const double r = static_cast<double>(best_c) / static_cast<double>(n_active);
          if (powi(1.0 - r * r * r, it) <= 1.0 - prm.proposal_engine_conf) break;
        }
        for (int q = 0; q < MAX_SOL; ++q) {
          const double v = hs[it * MAX_SOL + q];
          if (v > best) { best = v; best_i = it * MAX_SOL + q; best_c = hcnt[best_i]; }
        }
      }
      s_score[0] = best; s_index[0] = best_i;
    }
    __syncthreads();
  } else {
    // ---- arg-max over the hypothesis table (ties -> lowest index) ----
    double best = -1.0;
    int best_i = 0x7fffffff;
    for (int i = t; i < nh; i += 256) {
      const double v = hs[i];
      if (v > best) { best = v; best_i = i; }
    }
    // (max score, lowest index) is associative and commutative: any reduction order gives
    // the same winner -- a butterfly per wave, then the four wave winners through LDS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double v = __shfl_xor(best, off, 64);
      const int vi = __shfl_xor(best_i, off, 64);
      if (v > best || (v == best && vi < best_i)) { best = v; best_i = vi; }
    }
    if ((t & 63) == 0) { s_score[t >> 6] = best; s_index[t >> 6] = best_i; }
    __syncthreads();
    best = s_score[0]; best_i = s_index[0];
#pragma unroll
    for (int g2 = 1; g2 < 4; ++g2) {
      const double v = s_score[g2];
      const int vi = s_index[g2];
      if (v > best || (v == best && vi < best_i)) { best = v; best_i = vi; }
    }
    __syncthreads();
    if (t == 0) { s_score[0] = best; s_index[0] = best_i; }
    __syncthreads();
  }
  double best_score = s_score[0];
  const int bi = s_index[0];
  int best_count = best_score > 0.0 ? hcnt[bi] : 0;
  FIT_TRACE(1, s == 0 && g == 0 && t == 0);
  if (!(best_score > 0.0) || best_count < 3) {             // uniform
    if (t == 0 && g == 0) round_failed(s, w, prm, want, k, n_active);
    return;
  }
  LoSync sy = lo_sync_of(w, s, g, lo_launch, n_lo);
#ifdef EPOS_FIT_TRACE
  sy.trace = s == 0 && g == 0;
#endif
  const Camera cam = camera_of(Ks, s, prm);
  double pose[12];
  for (int i = 0; i < 12; ++i) pose[i] = w.hyp_pose[(static_cast<int64_t>(s) * nh + bi) * 12 + i];
  // ---- local optimisation (i): the whole workgroup sums, every thread steps ----
  orthonormalize(pose);
  const int32_t* idx = n_active == sl.n ? nullptr : active;   // identity while nothing is removed
  lo_refine<true, 1>(pose, &best_score, &best_count, sl, cam, idx, n_active, t, sy, &s_lo,
                     nullptr, prm.lo_iters, s == 0 && g == 0 && t == 0);
  if (g == 0) {
    if (t < 12) w.cur_pose[s * 12 + t] = pose[t];
    if (t == 0) { w.cur_score[s] = best_score; w.cur_count[s] = best_count; }
  }
  if (!gc_enabled(prm)) { if (t == 0 && g == 0) w.state[s] = 2; return; }
  // ---- residual table (2^-20 fixed point of min(e^2 / (1.5 tau)^2, 1)) and the
  //      thresholded labelling the sweeps start from; 2 = not active. A correspondence is
  //      active iff no accepted instance explains it yet (labels < 0: ransac_refit_accept
  //      labels exactly the ones it removes from the active list), so every point is
  //      decided by the one thread that owns it -- the workgroups of the slot share the rows
  uint8_t* lab = w.lab_a + sl.base;
  int32_t* gq = w.gq + sl.base;
  const int32_t* labels = labels_all + sl.base;
  const double tthr = 1.5 * prm.threshold, tthr2 = tthr * tthr;
  GcDyn* dyn = w.dyn_a + sl.base;
  for (int64_t p = static_cast<int64_t>(g) * 256 + t; p < sl.n; p += 256 * LO_G) {
    const int64_t pos = sl.ypos ? sl.ypos[p] : p;
    GcDyn dn;
    dn.Z = sl.xyz[3 * p + 2]; dn.q = GC_Q; dn.out = 1;
    if (labels[p] >= 0) {
      lab[p] = 2;
      dn.Z = __builtin_huge_val(); dn.q = 0; dn.out = 0;
      dyn[pos] = dn;
      continue;
    }
    double e2, Xc[3], r[2];
    if (reproj(pose, cam.K, sl.xy + 2 * p, sl.xyz + 3 * p, &e2, Xc, r)) {
      gq[p] = GC_Q; lab[p] = 0; dyn[pos] = dn;
      continue;
    }
    double d = e2 / tthr2;
    if (!(d < 1.0)) d = 1.0;
    dn.q = static_cast<int32_t>(d * static_cast<double>(GC_Q));
    dn.out = e2 < cam.thr2 ? 0 : 1;
    gq[p] = dn.q;
    lab[p] = e2 < cam.thr2 ? 1 : 0;
    dyn[pos] = dn;
  }
  if (t == 0 && g == 0) w.state[s] = 1;
  FIT_TRACE(1, s == 0 && g == 0 && t == 0);
}

// ---- round, step 4: local optimisation (ii) on the labelled inliers, the instance
// acceptance tests, labelling + removal of the explained correspondences.
__global__ __launch_bounds__(256) void ransac_refit_accept(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const double* __restrict__ Ks,
    const int32_t* __restrict__ max_models, EposFitParams prm, int max_k, Work w,
    const uint8_t* __restrict__ lab_all, double* poses, double* scores,
    int32_t* num_models, int32_t* labels_all, int lo_launch, int n_lo) {
  const int s = blockIdx.y;
  const int g = blockIdx.x;          // LO_G workgroups refit together; workgroup 0 accepts
  const int t = threadIdx.x;
  const int state = w.state[s];
  FIT_TRACE(2, s == 0 && g == 0 && t == 0);
  if (state == 0) return;                                  // uniform over the slot
  const int want = clamp_want(max_models[s], max_k);
  const int k = num_models[s];
  const Slot sl = slot_of(slot_base, s, w, xy_all, xyz_all);
  const int64_t n = sl.n;
  int32_t* active = w.active + sl.base;
  const int64_t n_active = w.n_active[s];
  __shared__ LoLds s_lo;
  __shared__ int s_inl[4], s_new[4];
  const int lane = t & 63, wave = t >> 6;
  int32_t* labels = labels_all + sl.base;
  const Camera cam = camera_of(Ks, s, prm);
  double pose[12];
  for (int i = 0; i < 12; ++i) pose[i] = w.cur_pose[s * 12 + i];
  double best_score = w.cur_score[s];
  int best_count = w.cur_count[s];
  if (state == 1) {
    // the first step on the labelled set starts from the accepted pose (its score is
    // known); from then on each pass scores a candidate and steps from it
    LoSync sy = lo_sync_of(w, s, g, lo_launch, n_lo);
    const int32_t* idx = n_active == n ? nullptr : active;
    lo_refine<false, 2>(pose, &best_score, &best_count, sl, cam, idx, n_active, t, sy, &s_lo,
                        lab_all + sl.base, prm.lo_iters, s == 0 && g == 0 && t == 0);
  }
  // A hand-off that timed out (a sibling workgroup was not scheduled for ~0.5 s: never seen,
  // but then the sums -- and everything derived from them -- are garbage) is reported, not
  // hidden: the slot's instance count becomes -1 and the host entry points raise.
  if (__hip_atomic_load(w.lo_timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
    if (g == 0 && t == 0) { num_models[s] = -1; w.done[s] = 1; }
    return;
  }
  if (g != 0) return;          // the siblings only helped with the sums
  FIT_TRACE(2, s == 0 && t == 0);
  if (best_count < prm.min_point_number) {
    if (t == 0) round_failed(s, w, prm, want, k, n_active);
    return;
  }
  // ---- inliers over ALL correspondences of the slot -> bitset (chunk c: wave c % 4);
  //      four chunks per trip: their loads are issued together (one dependent round trip
  //      per trip instead of per chunk -- this loop is latency, not arithmetic)
  const int64_t words = (n + 63) / 64;
  const int64_t wbase = sl.base / 64 + s;
  uint64_t* cur = w.inl_bits + static_cast<int64_t>(k) * w.words_total + wbase;
  int n_inl = 0, n_new = 0;
  for (int64_t c0 = wave; c0 < words; c0 += 16) {
    double x2[4][2], x3[4][3];
    int32_t lb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = (c0 + 4 * u) * 64 + lane;
      const int64_t ic = i < n ? i : n - 1;
      x2[u][0] = sl.xy[2 * ic]; x2[u][1] = sl.xy[2 * ic + 1];
      x3[u][0] = sl.xyz[3 * ic]; x3[u][1] = sl.xyz[3 * ic + 1]; x3[u][2] = sl.xyz[3 * ic + 2];
      lb[u] = labels[ic];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = c0 + 4 * u;
      if (c >= words) break;                               // wave-uniform
      const int64_t i = c * 64 + lane;
      bool inl = false;
      double e2, Xc[3], r[2];
      if (i < n && !reproj(pose, cam.K, x2[u], x3[u], &e2, Xc, r)) inl = e2 < cam.thr2;
      const bool fresh = inl && lb[u] < 0;
      const uint64_t bits = __ballot(inl);
      n_inl += __popcll(bits);
      n_new += __popcll(__ballot(fresh));
      if (lane == 0) cur[c] = bits;
    }
  }
  __shared__ int s_ok;
  __shared__ int s_keep[4][4];
  if (lane == 0) { s_inl[wave] = n_inl; s_new[wave] = n_new; }
  __threadfence_block();
  __syncthreads();
  FIT_TRACE(2, s == 0 && t == 0);
  n_inl = s_inl[0] + s_inl[1] + s_inl[2] + s_inl[3];
  n_new = s_new[0] + s_new[1] + s_new[2] + s_new[3];
  if (wave == 0) {                                         // the acceptance tests
    bool ok = n_inl > 0;
    for (int j = 0; j < k && ok; ++j) {
      const uint64_t* pj = w.inl_bits + static_cast<int64_t>(j) * w.words_total + wbase;
      int inter = 0, uni = 0;
      for (int64_t c = lane; c < words; c += 64) {
        const uint64_t a = cur[c], b = pj[c];
        inter += __popcll(a & b);
        uni += __popcll(a | b);
      }
      inter = wave_sum(inter);
      uni = wave_sum(uni);
      if (static_cast<double>(inter) >= prm.max_tanimoto_similarity * static_cast<double>(uni)) ok = false;
    }
    if (ok && static_cast<double>(n_new) < prm.min_coverage * static_cast<double>(n_inl)) ok = false;
    if (lane == 0) s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  FIT_TRACE(2, s == 0 && t == 0);
  if (!s_ok) { if (t == 0) round_failed(s, w, prm, want, k, n_active); return; }
  // ---- accept: write the pose, label + remove its inliers. Stable compaction of the
  //      active list IN PLACE by the whole workgroup, 1024 entries per trip: every entry
  //      of the trip is read before any is written, and a trip only writes below its own
  //      start + what it kept (positions that have all been read).
  if (t < 12) poses[(static_cast<int64_t>(s) * max_k + k) * 12 + t] = pose[t];
  if (t == 0) scores[static_cast<int64_t>(s) * max_k + k] = best_score;
  if (k + 1 >= want) {
    // the slot's LAST instance: nobody reads its active list again, so the compaction (a
    // dependent gather per entry) is skipped -- the unexplained inliers are labelled
    // straight from the bitset, coalesced. (Every inlier that is still unlabelled IS
    // active: the two sets are kept identical by the compaction below.)
    for (int64_t i = t; i < n; i += 256)
      if (((cur[i >> 6] >> (i & 63)) & 1ull) && labels[i] < 0) labels[i] = k;
    if (t == 0) {
      w.tries[s] = 0;
      w.last_new[s] = n_new;
      num_models[s] = k + 1;
      w.done[s] = 1;
    }
    FIT_TRACE(2, s == 0 && t == 0);
    return;
  }
  int64_t wpos = 0;
  for (int64_t c0 = 0; c0 < n_active; c0 += 1024) {
    int32_t pv[4];
    bool keep[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = c0 + u * 256 + t;
      pv[u] = i < n_active ? active[i] : 0;
    }
    uint64_t cw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cw[u] = cur[pv[u] >> 6];
    int rank[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = c0 + u * 256 + t;
      const bool inl = i < n_active && ((cw[u] >> (pv[u] & 63)) & 1ull);
      if (inl) labels[pv[u]] = k;
      keep[u] = i < n_active && !inl;
      const uint64_t kb = __ballot(keep[u]);
      rank[u] = __popcll(kb & ((1ull << lane) - 1ull));
      if (lane == 0) s_keep[u][wave] = __popcll(kb);
    }
    __syncthreads();                       // every entry of the trip has been read
    int total = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int g2 = 0; g2 < 4; ++g2) total += s_keep[u][g2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int off = 0;
#pragma unroll
      for (int uu = 0; uu < 4; ++uu)
#pragma unroll
        for (int g2 = 0; g2 < 4; ++g2)
          if (uu * 4 + g2 < u * 4 + wave) off += s_keep[uu][g2];
      if (keep[u]) active[wpos + off + rank[u]] = pv[u];
    }
    wpos += total;
    __syncthreads();                       // s_keep is reused by the next trip
  }
  if (t == 0) {
    w.n_active[s] = static_cast<int32_t>(wpos);
    w.tries[s] = 0;
    w.last_new[s] = n_new;
    num_models[s] = k + 1;
    if (k + 1 >= want) w.done[s] = 1;
  }
  FIT_TRACE(2, s == 0 && t == 0);
}

// cooperating launches per call: select + refit of every round (max_k + 2 rounds at most)
int lo_launches(int max_k) { return 2 * (max_k + 2); }

// The workspace of one call: every buffer of Work, carved in this order from 256-byte
// aligned offsets. base != null: fills w's pointers and words_total; base == null: w is not
// touched. Returns the bytes the buffers take (epos_fit_workspace_bytes).
int64_t carve_work(char* base, int S, int64_t n_cap, int max_iters, int max_k, Work& w) {
  int64_t off = 0;
  auto take = [&](auto*& ptr, int64_t bytes) {
    if (base) ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + off);
    off = (off + bytes + 255) / 256 * 256;
  };
  const int64_t nh = static_cast<int64_t>(S) * max_iters * MAX_SOL;
  const int64_t words_total = n_cap / 64 + S + 2;
  if (base) w.words_total = words_total;
  take(w.hyp_score, nh * 8);
  take(w.hyp_pose, nh * 12 * 8);
  take(w.hyp_count, nh * 4);
  take(w.active, (n_cap + 1) * 4);
  take(w.n_active, (S + 1) * 4);
  take(w.done, (S + 1) * 4);
  take(w.inl_bits, words_total * (max_k + 1) * 8);
  take(w.cur_pose, (S + 1) * 12 * 8);
  take(w.cur_score, (S + 1) * 8);
  take(w.cur_count, (S + 1) * 4);
  take(w.state, (S + 1) * 4);
  take(w.tries, (S + 1) * 4);
  take(w.last_new, (S + 1) * 4);
  take(w.gq, (n_cap + 1) * 4);
  take(w.lab_a, n_cap + 1);
  take(w.lab_b, n_cap + 1);
  take(w.lo_cnt, static_cast<int64_t>(S + 1) * lo_launches(max_k) * 4);
  take(w.lo_data, static_cast<int64_t>(S + 1) * 2 * LO_G * 4 * LO_NV * 8);
  take(w.lo_timeout, 8);
  take(w.nb_cnt, (n_cap + 1) * NB_W * 2);
  take(w.nb_pool, (n_cap + 1) * NB_W * NB_SUB * 2);
  take(w.nb_ok, (S + 1) * 4);
  take(w.geo, (n_cap + 1) * 32);
  take(w.dyn_a, (n_cap + 1) * 16);
  take(w.dyn_b, (n_cap + 1) * 16);
  take(w.win, words_total * 2 * 4);
  take(w.acc, (n_cap + 1) * 16);
  take(w.flip_a, n_cap + 1);
  take(w.flip_b, n_cap + 1);
  take(w.pearl_pose, (S + 1) * PEARL_MAX_K * 12 * 8);
  take(w.pearl_acc, (S + 1) * 4 * PEARL_BINS * 8);
  take(w.pearl_state, (S + 1) * 4);
  take(w.pearl_moved, (S + 1) * 4);
  take(w.lab_c, n_cap + 1);
  take(w.pearl_dt, (n_cap + 1) * PEARL_DT * 4);
  return off;
}

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Enqueues the whole fitting stage. yorder / ypos [device, n_capacity] or null: the
// y-sorted order of every slot's correspondences and its inverse (slot-local indices);
// null = the slots are already sorted by image row (epos_corr_fill's raster order).
int find6d_enqueue(const double* xy, const double* xyz, const int64_t* slot_base, int S,
                   int64_t n_capacity, const double* Ks, const int32_t* max_models,
                   const uint64_t* seeds, const EposFitParams* p, int32_t max_k, void* work,
                   double* poses, double* scores, int32_t* num_models, int32_t* labels,
                   const int32_t* yorder, const int32_t* ypos, hipStream_t st) {
  Work w;
  carve_work(static_cast<char*>(work), S, n_capacity, p->max_iters, max_k, w);
  w.yorder = yorder; w.ypos = ypos;
  static const unsigned spin_max = [] {      // EPOS_FIT_SPIN_MAX=0: every hand-off that has to
    const char* e = getenv("EPOS_FIT_SPIN_MAX");   // wait at all gives up (tests of the error path)
    return e ? static_cast<unsigned>(strtoul(e, nullptr, 10)) : LO_SPIN_MAX;
  }();
  w.lo_spin_max = spin_max;
  const int n_lo = lo_launches(max_k);
  const bool gc = gc_enabled(*p);
  // The binary sweeps scan the windows with the candidates in scalar registers (ransac_gc_scan,
  // then ransac_gc_delta): that costs less than walking neighbour lists, so the lists are built
  // only for the joint refinement, whose passes gather per point. EPOS_FIT_SCAN=0 runs the LDS-
  // staged sweeps instead, which walk the lists too: building them (one sweep's worth of pair
  // tests) then pays from a call's third neighbourhood pass on. EPOS_FIT_NB_LISTS=0: no lists,
  // every pass scans windows. EPOS_FIT_DELTA=0: every sweep is a full scan.
  static const int use_nb = env_int("EPOS_FIT_NB_LISTS", 1);
  static const int use_scan = env_int("EPOS_FIT_SCAN", 1);
  static const int use_delta = env_int("EPOS_FIT_DELTA", 1);
  const bool refine = max_k >= 2 && p->pearl_iters > 0;      // the joint refinement may run
  const bool nb_pays = use_scan ? refine : fit_rounds(max_k) * p->gc_sweeps > 2;
  const int build_nb = gc && use_nb && GC_W == NB_W &&     // lists are laid out per wave
                       nb_pays ? 1 : 0;
  const int64_t per_slot = ceil_div(n_capacity, S > 0 ? S : 1);
  const dim3 hgrid(static_cast<unsigned>(ceil_div(p->max_iters, 4)), S);
  // joint refinement kernels: one wavefront per point and pass
  // (512 .. 2048 workgroups per slot measure the same at C4's size; 128 is 30 % slower)
  const dim3 pgrid(static_cast<unsigned>(per_slot < 8192 ? ceil_div(per_slot, 4) < 64 ? 64 : ceil_div(per_slot, 4) : 2048), S);
  // labelling sweeps: one workgroup per tile of 64 points (grid-stride beyond 512 tiles)
  const int64_t tiles = ceil_div(per_slot, 64);
  const dim3 sgrid(static_cast<unsigned>(tiles < 1 ? 1 : tiles > 512 ? 512 : tiles), S);
  // ---- one proposal round ----
  const auto enqueue_round = [&](int round) -> int {
    hipLaunchKernelGGL(ransac_hypotheses, hgrid, dim3(256), 0, st, xy, xyz, slot_base, Ks, seeds,
                       max_models, num_models, *p, max_k, round, w);
    int rc = launch_status("ransac_hypotheses");
    if (rc) return rc;
    hipLaunchKernelGGL(ransac_select_lo, dim3(LO_G, S), dim3(256), 0, st, xy, xyz, slot_base,
                       Ks, max_models, *p, max_k, round, w, num_models, labels, 2 * round, n_lo);
    rc = launch_status("ransac_select_lo");
    if (rc) return rc;
    const uint8_t* lab_final = w.lab_a;
    for (int sw = 0; gc && sw < p->gc_sweeps; ++sw) {
      const uint8_t* in = (sw & 1) ? w.lab_b : w.lab_a;
      uint8_t* out = (sw & 1) ? w.lab_a : w.lab_b;
      if (use_scan && sw > 0 && use_delta)
        hipLaunchKernelGGL(ransac_gc_delta, sgrid, dim3(256), 0, st, slot_base, *p, w,
                           reinterpret_cast<const GcGeo*>(w.geo), w.dyn_a,
                           (sw & 1) ? w.flip_a : w.flip_b, (sw & 1) ? w.flip_b : w.flip_a,
                           in, out);
      else if (use_scan)
        hipLaunchKernelGGL(ransac_gc_scan,
                           dim3(static_cast<unsigned>(ceil_div(sgrid.x, GS_P)), S), dim3(GS_T),
                           0, st, slot_base, *p, w, reinterpret_cast<const GcGeo*>(w.geo),
                           (sw & 1) ? w.dyn_b : w.dyn_a, (sw & 1) ? w.dyn_a : w.dyn_b, in,
                           out, (sw & 1) ? w.flip_b : w.flip_a);
      else
        hipLaunchKernelGGL(ransac_gc_sweep<false>, sgrid, dim3(GC_T), 0, st, xy, xyz,
                           slot_base, *p, w, in, out);
      rc = launch_status("ransac_gc_sweep");
      if (rc) return rc;
      lab_final = out;
    }
    hipLaunchKernelGGL(ransac_refit_accept, dim3(LO_G, S), dim3(256), 0, st, xy, xyz,
                       slot_base, Ks, max_models, *p, max_k, w, lab_final, poses, scores,
                       num_models, labels, 2 * round + 1, n_lo);
    return launch_status("ransac_refit_accept");
  };
  // ---- one iteration of the joint refinement (pearl_setup admits a slot only with gc_sweeps
  // >= 1). The sweeps' labels live in position order (lab_a / lab_b); the last sweep also writes
  // them in index order (lab_c) for the refit and the commit; the first yields the energy before.
  const auto enqueue_pearl_iteration = [&]() -> int {
    hipLaunchKernelGGL(pearl_begin, pgrid, dim3(256), 0, st, slot_base, num_models, w, labels);
    const dim3 dgrid(static_cast<unsigned>(pgrid.x < 4 ? 1 : pgrid.x / 4), S);
    // One launch per case of Work::nb_ok; the slots of the other case leave at once. The
    // window-walk case is the rare one -- a sub-list overflowed -- and gets the small grid:
    // its launch is ~2 us of empty workgroups otherwise.
    const dim3 fgrid(pgrid.x < 256 ? pgrid.x : 256, S);
    hipLaunchKernelGGL(pearl_data, dgrid, dim3(256), 0, st, xy, xyz, slot_base, Ks, num_models,
                       *p, max_k, w, poses, 0);
    const uint8_t* lab_final = w.lab_a;
    for (int sw = 0; sw < p->gc_sweeps; ++sw) {
      const uint8_t* in = (sw & 1) ? w.lab_b : w.lab_a;
      uint8_t* out = (sw & 1) ? w.lab_a : w.lab_b;
      uint8_t* idx_out = sw + 1 == p->gc_sweeps ? w.lab_c : nullptr;
      hipLaunchKernelGGL(pearl_sweep<true>, pgrid, dim3(256), 0, st, xy, xyz, slot_base,
                         num_models, *p, w, in, out, sw == 0 ? 1 : 0, idx_out);
      hipLaunchKernelGGL(pearl_sweep<false>, fgrid, dim3(256), 0, st, xy, xyz, slot_base,
                         num_models, *p, w, in, out, sw == 0 ? 1 : 0, idx_out);
      lab_final = out;
    }
    hipLaunchKernelGGL(pearl_refit, dim3(S, PEARL_MAX_K), dim3(256), 0, st, xy, xyz, slot_base, Ks,
                       num_models, *p, max_k, w, poses, w.lab_c);
    hipLaunchKernelGGL(pearl_data, dgrid, dim3(256), 0, st, xy, xyz, slot_base, Ks, num_models,
                       *p, max_k, w, poses, 1);
    hipLaunchKernelGGL(pearl_energy<true>, pgrid, dim3(256), 0, st, xy, xyz, slot_base,
                       num_models, *p, w, lab_final, 1);
    hipLaunchKernelGGL(pearl_energy<false>, fgrid, dim3(256), 0, st, xy, xyz, slot_base,
                       num_models, *p, w, lab_final, 1);
    hipLaunchKernelGGL(pearl_commit, dim3(S), dim3(256), 0, st, slot_base, num_models, *p,
                       max_k, w, poses, w.lab_c, labels);
    return launch_status("pearl");
  };
  hipLaunchKernelGGL(ransac_init, dim3(S, 24), dim3(256), 0, st, xy, xyz, slot_base, S, w, labels,
                     num_models, p->min_point_number, n_capacity, n_lo, build_nb, gc ? 1 : 0,
                     p->neighborhood_ball_radius);
  int rc = launch_status("ransac_init");
  if (rc) return rc;
  if (build_nb) {       // the neighbourhood graph, once: neither labels nor rounds change it
    hipLaunchKernelGGL(ransac_gc_sweep<true>, sgrid, dim3(GC_T), 0, st, xy, xyz, slot_base, *p,
                       w, nullptr, nullptr);
    rc = launch_status("ransac_nb_build");
    if (rc) return rc;
  }
  for (int round = 0; round < fit_rounds(max_k) && !rc; ++round) rc = enqueue_round(round);
  if (rc || !(refine && gc)) return rc;
  hipLaunchKernelGGL(pearl_setup, dim3(static_cast<unsigned>(ceil_div(S, 64))), dim3(64), 0, st,
                     num_models, *p, w, S);
  for (int it = 0; it < p->pearl_iters && !rc; ++it) rc = enqueue_pearl_iteration();
  return rc;
}

// the ranges both entry points accept; fn: the entry point's name for the error text; all: the
// host entry's one text for every range
int validate_fit_params(const char* fn, const EposFitParams* p, int32_t max_k, const char* all) {
  const char* msg =
      !(max_k >= 1 && p->max_iters >= 1) ? "max_k and max_iters must be >= 1"
      : !(p->gc_sweeps >= 0 && p->gc_sweeps <= 16) ? "gc_sweeps must be in [0, 16]"
      : !(p->pearl_iters >= 0 && p->pearl_iters <= 8) ? "pearl_iters must be in [0, 8]" : nullptr;
  if (msg) set_error("%s: %s", fn, all ? all : msg);
  return msg ? EPOS_E_INVALID : EPOS_OK;
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" void epos_fit_params_default(EposFitParams* p) {
  // scripts/infer.py:76-120 (flag defaults) and :470-488 (call).
  p->threshold = 4.0;
  p->neighborhood_ball_radius = 20.0;
  p->spatial_coherence_weight = 0.1;
  p->scaling_from_millimeters = 0.1;
  p->max_tanimoto_similarity = 0.9;
  p->conf = 0.5;
  p->proposal_engine_conf = 1.0;
  p->min_coverage = 0.5;
  p->min_triangle_area = 0.0;
  p->max_iters = 400;
  p->min_point_number = 6;
  p->max_model_number = 1;
  p->max_model_number_for_optimization = 5;
  p->use_prosac = 0;
  p->lo_iters = 8;
  p->gc_sweeps = 2;
  p->pearl_iters = 2;
}

extern "C" int64_t epos_fit_workspace_bytes(int S, int64_t n_capacity,
                                            const EposFitParams* p, int32_t max_k) {
  if (!p || S < 0 || n_capacity < 0 || max_k < 1) return EPOS_E_INVALID;
  Work unused;
  return carve_work(nullptr, S, n_capacity, p->max_iters, max_k, unused);
}

extern "C" int epos_find6d_poses_device_ordered(
    const double* xy, const double* xyz, const int64_t* slot_base, int S,
    int64_t n_capacity, const double* Ks, const int32_t* max_models,
    const uint64_t* seeds, const EposFitParams* p, int32_t max_k, void* work,
    double* poses, double* scores, int32_t* num_models, int32_t* labels,
    void* stream, const int32_t* yorder, const int32_t* ypos) {
  EPOS_REQUIRE(xy && xyz && slot_base && Ks && max_models && seeds && p && work &&
               poses && scores && num_models && labels, "null pointer");
  EPOS_REQUIRE(!yorder == !ypos, "yorder and ypos: both or neither");
  if (const int bad = validate_fit_params(__func__, p, max_k, nullptr)) return bad;
  if (S == 0) return EPOS_OK;
  return find6d_enqueue(xy, xyz, slot_base, S, n_capacity, Ks, max_models, seeds, p, max_k,
                        work, poses, scores, num_models, labels, yorder, ypos,
                        static_cast<hipStream_t>(stream));
}

extern "C" int epos_find6d_poses_device(
    const double* xy, const double* xyz, const int64_t* slot_base, int S,
    int64_t n_capacity, const double* Ks, const int32_t* max_models,
    const uint64_t* seeds, const EposFitParams* p, int32_t max_k, void* work,
    double* poses, double* scores, int32_t* num_models, int32_t* labels,
    void* stream) {
  return epos_find6d_poses_device_ordered(xy, xyz, slot_base, S, n_capacity, Ks, max_models,
                                          seeds, p, max_k, work, poses, scores, num_models,
                                          labels, stream, nullptr, nullptr);
}

extern "C" int epos_find6d_poses(const double* xy, const double* xyz, int64_t n,
                                 const double* K, const EposFitParams* p,
                                 uint64_t seed, double* poses_out,
                                 int32_t* labels_out, double* scores_out,
                                 int32_t max_k) {
  EPOS_REQUIRE(K && p && poses_out && scores_out && (n == 0 || (xy && xyz && labels_out)),
               "null pointer");
  EPOS_REQUIRE(max_k >= 1, "max_k must be >= 1");
  for (int64_t i = 0; i < n; ++i) labels_out[i] = -1;
  if (n < p->min_point_number || n < 3) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("epos_find6d_poses: no HIP device (there is no CPU fallback)");
    return EPOS_E_NODEVICE;
  }
  if (const int bad = validate_fit_params(
          __func__, p, max_k, "max_iters >= 1, gc_sweeps in [0, 16], pearl_iters in [0, 8]")) return bad;
  const int64_t wbytes = epos_fit_workspace_bytes(1, n, p, max_k);
  const int64_t sizes[] = {n * 16, n * 24, 16, 72, 8, 8, wbytes,
                           static_cast<int64_t>(max_k) * 96,
                           static_cast<int64_t>(max_k) * 8, 8, n * 4, n * 4, n * 4};
  constexpr int ND = 13;
  char* d[ND] = {0};
  int rc = EPOS_OK;
  for (int i = 0; i < ND && !rc; ++i)
    rc = check_hip(hipMalloc(reinterpret_cast<void**>(&d[i]), sizes[i] + 8), "hipMalloc");
  int32_t k = 0;
  // The caller's order is kept (PROSAC samples from a prefix of it); the neighbourhood
  // windows of the spatial-coherence step walk the correspondences in image-row order
  // through this permutation (stable sort by y) and its inverse.
  int32_t* yorder = static_cast<int32_t*>(malloc(sizeof(int32_t) * static_cast<size_t>(n) * 2));
  if (!yorder) { set_error("epos_find6d_poses: out of host memory"); rc = EPOS_E_INVALID; }
  if (!rc) {
    int32_t* ypos = yorder + n;
    for (int64_t i = 0; i < n; ++i) yorder[i] = static_cast<int32_t>(i);
    std::stable_sort(yorder, yorder + n, [&](int32_t a, int32_t b) {
      return xy[2 * static_cast<int64_t>(a) + 1] < xy[2 * static_cast<int64_t>(b) + 1];
    });
    for (int64_t i = 0; i < n; ++i) ypos[yorder[i]] = static_cast<int32_t>(i);
    rc = check_hip(hipMemcpy(d[11], yorder, n * 4, hipMemcpyHostToDevice), "copy yorder");
    if (!rc) rc = check_hip(hipMemcpy(d[12], ypos, n * 4, hipMemcpyHostToDevice), "copy ypos");
  }
  free(yorder);
  if (!rc) {
    const int64_t sb[2] = {0, n};
    const int32_t mm = clamp_want(p->max_model_number, max_k);
    rc = check_hip(hipMemcpy(d[0], xy, n * 16, hipMemcpyHostToDevice), "copy xy");
    if (!rc) rc = check_hip(hipMemcpy(d[1], xyz, n * 24, hipMemcpyHostToDevice), "copy xyz");
    if (!rc) rc = check_hip(hipMemcpy(d[2], sb, 16, hipMemcpyHostToDevice), "copy base");
    if (!rc) rc = check_hip(hipMemcpy(d[3], K, 72, hipMemcpyHostToDevice), "copy K");
    if (!rc) rc = check_hip(hipMemcpy(d[4], &mm, 4, hipMemcpyHostToDevice), "copy mm");
    if (!rc) rc = check_hip(hipMemcpy(d[5], &seed, 8, hipMemcpyHostToDevice), "copy seed");
    if (!rc)
      rc = find6d_enqueue(
          reinterpret_cast<double*>(d[0]), reinterpret_cast<double*>(d[1]),
          reinterpret_cast<int64_t*>(d[2]), 1, n, reinterpret_cast<double*>(d[3]),
          reinterpret_cast<int32_t*>(d[4]), reinterpret_cast<uint64_t*>(d[5]), p,
          max_k, d[6], reinterpret_cast<double*>(d[7]),
          reinterpret_cast<double*>(d[8]), reinterpret_cast<int32_t*>(d[9]),
          reinterpret_cast<int32_t*>(d[10]), reinterpret_cast<int32_t*>(d[11]),
          reinterpret_cast<int32_t*>(d[12]), nullptr);
    if (!rc) rc = check_hip(hipDeviceSynchronize(), "sync");
    if (!rc) rc = check_hip(hipMemcpy(&k, d[9], 4, hipMemcpyDeviceToHost), "copy k");
    if (!rc && k < 0) {
      set_error("epos_find6d_poses: a hand-off between cooperating workgroups timed out");
      rc = EPOS_E_INTERNAL;
    }
    if (!rc && k > 0) {
      rc = check_hip(hipMemcpy(poses_out, d[7], static_cast<size_t>(k) * 96, hipMemcpyDeviceToHost), "copy poses");
      if (!rc) rc = check_hip(hipMemcpy(scores_out, d[8], static_cast<size_t>(k) * 8, hipMemcpyDeviceToHost), "copy scores");
    }
    if (!rc) rc = check_hip(hipMemcpy(labels_out, d[10], n * 4, hipMemcpyDeviceToHost), "copy labels");
  }
  for (int i = 0; i < ND; ++i)
    if (d[i]) (void)hipFree(d[i]);
  return rc ? rc : k;
}

#ifdef EPOS_FIT_TRACE
extern "C" int epos_debug_fit_trace(unsigned long long* out /*[8][32]*/, int* n8, int reset) {
  int rc = static_cast<int>(hipMemcpyFromSymbol(out, HIP_SYMBOL(epos::g_fit_trace), 8 * 32 * 8));
  rc |= static_cast<int>(hipMemcpyFromSymbol(n8, HIP_SYMBOL(epos::g_fit_trace_n), 32));
  if (reset) {
    const int z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rc |= static_cast<int>(hipMemcpyToSymbol(HIP_SYMBOL(epos::g_fit_trace_n), z, 32));
  }
  return rc;
}
#endif

#ifdef EPOS_GC_STATS
extern "C" int epos_debug_gc_stats(unsigned long long* out4, int reset) {
  int rc = static_cast<int>(hipMemcpyFromSymbol(out4, HIP_SYMBOL(epos::g_gc_stats), 32));
  if (reset) {
    const unsigned long long z[4] = {0, 0, 0, 0};
    rc |= static_cast<int>(hipMemcpyToSymbol(HIP_SYMBOL(epos::g_gc_stats), z, 32));
  }
  return rc;
}
#endif
