// Pose fitting (pnp_ransac.hip), what every stage shares: the constants, the RNG, the small
// algebra, reprojection and MSAC scoring, the FIT_TRACE stamps, the workspace (Work) and the
// view of one slot that a kernel fills at its top. Included first, after common.h and wave.h;
// fit_p3p.h, fit_lo.h, fit_label.h and fit_pearl.h follow in that order, all in ONE unit.
#pragma once

#include "common.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int MAX_SOL = 4;

// ------------------------------------------------------------------ RNG --
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t draw(uint64_t seed, uint32_t round,
                                         uint32_t it, uint32_t k, uint64_t n) {
  const uint64_t u =
      mix64(mix64(seed ^ mix64((static_cast<uint64_t>(round) << 32) | it)) + k);
  return __umul64hi(u, n);
}
__device__ __forceinline__ void sample3(uint64_t seed, uint32_t round, uint32_t it,
                                        int64_t m, int64_t* s) {
  int64_t a = static_cast<int64_t>(draw(seed, round, it, 0, m));
  int64_t b = static_cast<int64_t>(draw(seed, round, it, 1, m - 1));
  int64_t c = static_cast<int64_t>(draw(seed, round, it, 2, m - 2));
  if (b >= a) b += 1;
  const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
  if (c >= lo) c += 1;
  if (c >= hi) c += 1;
  s[0] = a; s[1] = b; s[2] = c;
}

// --------------------------------------------------------- small algebra --
__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// symmetric 3x3 packed as {00, 01, 02, 11, 12, 22}
__device__ __forceinline__ void sym_adj(const double* s, double* b) {
  b[0] = s[3] * s[5] - s[4] * s[4];
  b[1] = s[2] * s[4] - s[1] * s[5];
  b[2] = s[1] * s[4] - s[2] * s[3];
  b[3] = s[0] * s[5] - s[2] * s[2];
  b[4] = s[1] * s[2] - s[0] * s[4];
  b[5] = s[0] * s[3] - s[1] * s[1];
}
__device__ __forceinline__ double sym_det(const double* s, const double* adj) {
  return s[0] * adj[0] + s[1] * adj[1] + s[2] * adj[2];
}
__device__ __forceinline__ double sym_inner(const double* a, const double* b) {
  return a[0] * b[0] + a[3] * b[3] + a[5] * b[5] +
         2.0 * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4]);
}
__device__ __forceinline__ double sym_quad(const double* s, const double* v) {
  return s[0] * v[0] * v[0] + s[3] * v[1] * v[1] + s[5] * v[2] * v[2] +
         2.0 * (s[1] * v[0] * v[1] + s[2] * v[0] * v[2] + s[4] * v[1] * v[2]);
}
__device__ __forceinline__ double sym_at(const double* s, int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  // (0,0)->0 (0,1)->1 (0,2)->2 (1,1)->3 (1,2)->4 (2,2)->5
  return s[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
}

// -------------------------------------------------------------- scoring --
// returns true if behind the camera; else e2 / Xc / r are set
__device__ __forceinline__ bool reproj(const double* pose, const double* K,
                                       const double* xy, const double* xyz,
                                       double* e2, double* Xc, double* r) {
  Xc[0] = pose[0] * xyz[0] + pose[1] * xyz[1] + pose[2] * xyz[2] + pose[9];
  Xc[1] = pose[3] * xyz[0] + pose[4] * xyz[1] + pose[5] * xyz[2] + pose[10];
  Xc[2] = pose[6] * xyz[0] + pose[7] * xyz[1] + pose[8] * xyz[2] + pose[11];
  if (!(Xc[2] > 0.0)) return true;
  const double iz = 1.0 / Xc[2];               // the only division per point
  const double px = (K[0] * Xc[0] + K[1] * Xc[1]) * iz + K[2];
  const double py = (K[4] * Xc[1]) * iz + K[5];
  r[0] = px - xy[0];
  r[1] = py - xy[1];
  *e2 = r[0] * r[0] + r[1] * r[1];
  return false;
}

constexpr int PF = 4;           // items fetched together per lane / thread

// PF correspondences of one lane's strided partial (items i0, i0 + stride, ...): all
// index loads first, then all point loads (unconditional, from clamped positions), so
// that the gathers of PF items are in flight together.
struct PointBatch {
  double x2[PF][2], x3[PF][3];
  bool ok[PF];
  int32_t p[PF];
  __device__ __forceinline__ void load(const double* xy, const double* xyz,
                                       const int32_t* idx, int64_t i0, int stride,
                                       int64_t m) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int64_t i = i0 + static_cast<int64_t>(u) * stride;
      ok[u] = i < m;
      p[u] = idx ? idx[ok[u] ? i : i0] : static_cast<int32_t>(ok[u] ? i : i0);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      x2[u][0] = xy[2 * p[u]]; x2[u][1] = xy[2 * p[u] + 1];
      x3[u][0] = xyz[3 * p[u]]; x3[u][1] = xyz[3 * p[u] + 1]; x3[u][2] = xyz[3 * p[u] + 2];
    }
  }
};

// MSAC scores + inlier counts of `ns` (<= 4) poses over idx[0..m) in ONE pass over
// the correspondences (wave-wide; results uniform). Each pose's sum keeps the
// canonical order: 64 strided per-lane partials, then the xor butterfly.
__device__ void score_poses(const double* poses, int ns, const double* K,
                            const double* xy, const double* xyz, const int32_t* idx,
                            int64_t m, double thr2, int lane, double* score,
                            int* count) {
  const double inv_thr2 = 1.0 / thr2;
  double acc[MAX_SOL] = {0.0, 0.0, 0.0, 0.0};
  int cnt[MAX_SOL] = {0, 0, 0, 0};
  // PF items of this lane's partial are fetched together (index -> point is a dependent
  // gather: without this the loop is one memory round trip per item) and then consumed
  // in the canonical order i, i + 64, ...
  for (int64_t i0 = lane; i0 < m; i0 += 64 * PF) {
    PointBatch pb;
    pb.load(xy, xyz, idx, i0, 64, m);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (!pb.ok[u]) continue;
#pragma unroll
      for (int q = 0; q < MAX_SOL; ++q) {
        if (q < ns) {                                      // wave-uniform
          double e2, Xc[3], r[2];
          if (!reproj(poses + 12 * q, K, pb.x2[u], pb.x3[u], &e2, Xc, r) && e2 < thr2) {
            acc[q] += 1.0 - e2 * inv_thr2;
            ++cnt[q];
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MAX_SOL; ++q) {
    if (q < ns) {
      count[q] = wave_sum(cnt[q]);
      score[q] = wave_sum(acc[q]);
    }
  }
}

__device__ void bearing(const double* K, const double* xy, double* f) {
  const double y = (xy[1] - K[5]) / K[4];
  const double x = (xy[0] - K[2] - K[1] * y) / K[0];
  const double n = sqrt(x * x + y * y + 1.0);
  f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}

#ifdef EPOS_FIT_TRACE   // tools/fit_trace.py: time stamps (100 MHz) of slot 0's first workgroup
__device__ unsigned long long g_fit_trace[8][32];
__device__ int g_fit_trace_n[8];
#define FIT_TRACE(K, COND)                                                      \
  do {                                                                          \
    if (COND) {                                                                 \
      const int i_ = g_fit_trace_n[K];                                          \
      if (i_ < 32) { g_fit_trace[K][i_] = wall_clock64(); g_fit_trace_n[K] = i_ + 1; } \
    }                                                                           \
  } while (0)
#else
#define FIT_TRACE(K, COND) do { } while (0)
#endif

// What a sweep needs of a candidate besides its static geometry. An inactive correspondence
// carries Z = +inf: its 5-D distance to anything is +inf, so it fails `d2 <= r2` without a
// label test.
struct __attribute__((aligned(16))) GcDyn {
  double Z;
  int32_t q;            // fixed-point residual
  int32_t out;          // 1: currently labelled outlier
};

// Raw sums of a full scan over a point's window, the point itself included: the number of
// neighbours, of neighbours labelled outlier, and the neighbours' fixed-point residuals.
struct __attribute__((aligned(16))) GcAcc {
  uint32_t deg, n0;
  unsigned long long S;
};

struct Work {
  double* hyp_score;     // [S][iters][4]
  double* hyp_pose;      // [S][iters][4][12]
  int32_t* hyp_count;    // [S][iters][4]
  int32_t* active;       // [N] local indices, pooled by slot_base
  int32_t* n_active;     // [S]
  int32_t* done;         // [S]
  uint64_t* inl_bits;    // [max_k][words_total]
  int64_t words_total;
  // proposal state between the kernels of one round
  double* cur_pose;      // [S][12]
  double* cur_score;     // [S]
  int32_t* cur_count;    // [S]
  int32_t* state;        // [S] 0: nothing to do, 1: label + refit, 2: refit / accept only
  int32_t* tries;        // [S] failed proposals since the last accepted instance
  int32_t* last_new;     // [S] newly explained points of the last accepted instance
  int32_t* gq;           // [N] fixed-point truncated residuals of the labelling
  uint8_t* lab_a;        // [N] labels, ping
  uint8_t* lab_b;        // [N] labels, pong
  uint8_t* lab_c;        // [N] joint refinement: the last sweep's labels in INDEX order
  int32_t* pearl_dt;     // [N][PEARL_DT] joint refinement: data terms of every point and label
  const int32_t* yorder; // [N] correspondences of a slot sorted by image y (or null:
  const int32_t* ypos;   //     they already are), and the inverse permutation
  // the sweeps' candidate stream, per POSITION of the row-sorted order (ransac_gc_scan):
  double* geo;           // [N][4] x, y, X, Y -- written once per call by ransac_init
  int32_t* win;          // [words_total][2] candidate window of every tile of 64 positions
  GcAcc* acc;            // [N] raw neighbour sums of the last full scan (self included)
  int8_t* flip_a;        // [N] label change of the last sweep per position: +1 became
  int8_t* flip_b;        //     outlier, -1 became inlier, 0 unchanged / not active (ping, pong)
  GcDyn* dyn_a;          // [N] Z (+inf: not active), residual, "labelled outlier": ping
  GcDyn* dyn_b;          //     pong (a sweep reads one and writes the other)
  // neighbour lists of the 5-D graph (built once per call: the graph depends on neither
  // labels nor rounds), per POSITION of the row-sorted order
  uint16_t* nb_cnt;      // [N][GC_W] entries of the point's GC_W sub-lists
  int16_t* nb_pool;      // [N][GC_W][NB_SUB] position deltas
  int32_t* nb_ok;        // [S] 1: lists complete; 0: overflow -> the sweeps scan windows
  // cooperative local optimisation (LO_G workgroups per slot)
  unsigned* lo_cnt;      // [S][lo_launches(max_k)] arrival counters, zeroed by ransac_init
  double* lo_data;       // [S][2][LO_G * 4][LO_NV] wave sums, double buffered
  int32_t* lo_timeout;   // [1] sticky: a workgroup gave up waiting for its siblings
  unsigned lo_spin_max;  // polls before that happens (LO_SPIN_MAX; EPOS_FIT_SPIN_MAX: tests)
  // joint refinement
  double* pearl_pose;            // [S][8][12] candidate poses
  unsigned long long* pearl_acc; // [S][4][PEARL_BINS] data / smoothness sums before, after (exact)
  int32_t* pearl_state;          // [S] 1: refining
  int32_t* pearl_moved;          // [S]
};

constexpr int GC_Q = 1 << 20;          // fixed point of the labelling energies
constexpr int PEARL_DT = 9;            // = PEARL_MAX_K + 1 columns of Work::pearl_dt
constexpr double LO_MIN_GAIN = 1e-6;   // relative MSAC gain below which the refits stop

// b^e by binary exponentiation (multiplications only: every implementation of the
// stage gets the same bits)
__device__ __forceinline__ double powi(double b, int64_t e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r = r * b;
    b = b * b;
    e >>= 1;
  }
  return r;
}

// ---- rules the host and the kernels both apply --------------------------------------------
// instances a slot may get: its own wish, capped by (or, if negative, replaced by) max_k
__host__ __device__ __forceinline__ int clamp_want(int max_models, int max_k) {
  return max_models < 0 || max_models > max_k ? max_k : max_models;
}
// proposal rounds: a multi-instance (Progressive-X) search may retry a failed proposal twice
__host__ __device__ __forceinline__ int fit_rounds(int max_k) { return max_k + (max_k > 1 ? 2 : 0); }
// the spatial-coherence term acts; sweeps = false leaves the sweep count to the caller
__host__ __device__ __forceinline__ bool gc_enabled(const EposFitParams& prm, bool sweeps = true) {
  return (!sweeps || prm.gc_sweeps > 0) && prm.spatial_coherence_weight > 0.0 &&
         prm.neighborhood_ball_radius > 0.0;
}

// ---- one slot, as a kernel sees it: filled once at the kernel's top. Rows [base, base + n)
// of the pooled arrays; xy / xyz at its first row (null in the kernels that read the position-
// ordered stream); yorder / ypos: its row-sorted order and the inverse (null: sorted already).
struct Slot { int64_t base, n; const double *xy, *xyz; const int32_t *yorder, *ypos; };
__device__ __forceinline__ Slot slot_of(const int64_t* slot_base, int s, const Work& w) {
  const int64_t base = slot_base[s];
  return {base, slot_base[s + 1] - base, nullptr, nullptr,
          w.yorder ? w.yorder + base : nullptr, w.ypos ? w.ypos + base : nullptr};
}
__device__ __forceinline__ Slot slot_of(const int64_t* slot_base, int s, const Work& w,
                                        const double* xy_all, const double* xyz_all) {
  Slot sl = slot_of(slot_base, s, w);
  sl.xy = xy_all + 2 * sl.base; sl.xyz = xyz_all + 3 * sl.base;
  return sl;
}
// the slot's camera and the squared inlier threshold
struct Camera { double K[9], thr2; };
__device__ __forceinline__ Camera camera_of(const double* Ks, int s, const EposFitParams& prm) {
  Camera c;
  for (int i = 0; i < 9; ++i) c.K[i] = Ks[s * 9 + i];
  c.thr2 = prm.threshold * prm.threshold;
  return c;
}
// the 5-D neighbourhood: smoothness weight, radius, (millimetre scale)^2, radius^2
struct Ball { double lam, rad, s2, r2; };
__device__ __forceinline__ Ball ball_of(const EposFitParams& prm) {
  const double rad = prm.neighborhood_ball_radius;
  return {prm.spatial_coherence_weight, rad,
          prm.scaling_from_millimeters * prm.scaling_from_millimeters, rad * rad};
}

}  // namespace
}  // namespace epos
