// Pose errors (include/epos_hip.h, "Pose errors"; DESIGN.md, "Pose errors"): MSSD, MSPD, ADD
// and ADI of (estimate, ground truth) pairs over pooled model vertices and symmetry sets.
//
// Everything is fp64 from + - * / sqrt without FMA (the build sets -ffp-contract=off), every
// 3-term sum runs left to right with the translation added last, and every reduction has a
// shape that the header fixes (sums) or that does not matter (max, min). A result is therefore
// a function of the input alone and tests/helpers/pose_error_ref.py equals it bit for bit.
//
// Four launches on the caller's stream:
//   pose_add_kernel       one workgroup per pair: ADD, and +inf into the two min cells
//   pose_adi_kernel       (want_adi) one workgroup per pair: ADI, estimate-side points tiled
//                         through LDS
//   pose_ms_kernel        one workgroup per (pair, group of MS_GROUP_SYMS symmetries): the max
//                         over the vertices of each of its symmetries, for both errors at once
//                         (the estimate-side point and its projection are shared), folded into
//                         the pair's min with a 64-bit unsigned atomic min on the bits of the
//                         non-negative double
//   pose_finish_kernel    the one sqrt of MSSD and MSPD
#include "common.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int PE_THREADS = 256;          // also the 256 partial sums of the header's sum shape
constexpr int PE_WAVES = PE_THREADS / 64;
constexpr int MS_GROUP_SYMS = 8;         // symmetries a workgroup of pose_ms_kernel owns
constexpr int ADI_TILE = PE_THREADS;     // estimate-side points per LDS tile

__device__ __forceinline__ double inf_f64() { return __longlong_as_double(0x7ff0000000000000LL); }

struct Rigid {
  double r[9], t[3];
};

// R' = R_g R_s, t' = R_g t_s + t_g; s = 12 numbers: R_s row-major, then t_s
__device__ __forceinline__ void compose(const double* Rg, const double* tg, const double* s,
                                        Rigid& o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o.r[3 * i + j] = (Rg[3 * i] * s[j] + Rg[3 * i + 1] * s[3 + j]) + Rg[3 * i + 2] * s[6 + j];
    o.t[i] = ((Rg[3 * i] * s[9] + Rg[3 * i + 1] * s[10]) + Rg[3 * i + 2] * s[11]) + tg[i];
  }
}

__device__ __forceinline__ void apply(const double* r, const double* t, double x, double y,
                                      double z, double& ox, double& oy, double& oz) {
  ox = ((r[0] * x + r[1] * y) + r[2] * z) + t[0];
  oy = ((r[3] * x + r[4] * y) + r[5] * z) + t[1];
  oz = ((r[6] * x + r[7] * y) + r[8] * z) + t[2];
}

__device__ __forceinline__ double sq3(double dx, double dy, double dz) {
  return (dx * dx + dy * dy) + dz * dz;
}

// The header's sum shape: part[j] holds p_j; p_j += p_{j+128}, then 64, ... 1; returns p_0 to
// every thread.
__device__ __forceinline__ double tree_sum(double* part, double p) {
  part[threadIdx.x] = p;
  for (int s = PE_THREADS / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < s) part[threadIdx.x] += part[threadIdx.x + s];
  }
  __syncthreads();
  return part[0];
}

__global__ __launch_bounds__(PE_THREADS) void pose_add_kernel(
    const double* __restrict__ verts, const double* __restrict__ syms,
    const EposPosePair* __restrict__ pairs, double* __restrict__ err) {
  __shared__ double part[PE_THREADS];
  const EposPosePair& pr = pairs[blockIdx.x];
  const int n = pr.n_verts;
  const double* X = verts + 3 * static_cast<int64_t>(pr.vert_base);
  Rigid g;
  compose(pr.R_g, pr.t_g, syms + 12 * static_cast<int64_t>(pr.sym_base), g);
  double p = 0.0;
  for (int v = threadIdx.x; v < n; v += PE_THREADS) {
    const double x = X[3 * v], y = X[3 * v + 1], z = X[3 * v + 2];
    double ex, ey, ez, gx, gy, gz;
    apply(pr.R_e, pr.t_e, x, y, z, ex, ey, ez);
    apply(g.r, g.t, x, y, z, gx, gy, gz);
    p += sqrt(sq3(ex - gx, ey - gy, ez - gz));
  }
  const double total = tree_sum(part, p);
  if (threadIdx.x == 0) {
    double* e = err + 4 * static_cast<int64_t>(blockIdx.x);
    e[0] = inf_f64();
    e[1] = inf_f64();
    e[2] = total / static_cast<double>(n);
  }
}

__global__ __launch_bounds__(PE_THREADS) void pose_adi_kernel(
    const double* __restrict__ verts, const double* __restrict__ syms,
    const EposPosePair* __restrict__ pairs, double* __restrict__ err) {
  __shared__ double tx[ADI_TILE], ty[ADI_TILE], tz[ADI_TILE];
  __shared__ double part[PE_THREADS];
  const EposPosePair& pr = pairs[blockIdx.x];
  const int n = pr.n_verts;
  const double* X = verts + 3 * static_cast<int64_t>(pr.vert_base);
  Rigid g;
  compose(pr.R_g, pr.t_g, syms + 12 * static_cast<int64_t>(pr.sym_base), g);
  double p = 0.0;
  for (int row = 0; row < n; row += PE_THREADS) {      // the same trips for every thread
    const int v = row + threadIdx.x;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (v < n) apply(g.r, g.t, X[3 * v], X[3 * v + 1], X[3 * v + 2], gx, gy, gz);
    double best = inf_f64();
    for (int t0 = 0; t0 < n; t0 += ADI_TILE) {
      __syncthreads();                                 // the previous tile has been read
      const int w = t0 + threadIdx.x;
      if (w < n)
        apply(pr.R_e, pr.t_e, X[3 * w], X[3 * w + 1], X[3 * w + 2], tx[threadIdx.x],
              ty[threadIdx.x], tz[threadIdx.x]);
      __syncthreads();
      const int cnt = n - t0 < ADI_TILE ? n - t0 : ADI_TILE;
#pragma unroll 4
      for (int k = 0; k < cnt; ++k) {
        const double d = sq3(tx[k] - gx, ty[k] - gy, tz[k] - gz);
        best = d < best ? d : best;
      }
    }
    if (v < n) p += sqrt(best);
  }
  const double total = tree_sum(part, p);
  if (threadIdx.x == 0)
    err[4 * static_cast<int64_t>(blockIdx.x) + 3] = total / static_cast<double>(n);
}

__global__ __launch_bounds__(PE_THREADS) void pose_ms_kernel(
    const double* __restrict__ verts, const double* __restrict__ syms,
    const EposPosePair* __restrict__ pairs, int groups_per_pair, double* err) {
  __shared__ double tr[MS_GROUP_SYMS][12];                   // composed R', t' of the group
  __shared__ double red[PE_WAVES][2 * MS_GROUP_SYMS];
  const int pair = blockIdx.x / groups_per_pair;
  const int s0 = (blockIdx.x % groups_per_pair) * MS_GROUP_SYMS;
  const EposPosePair& pr = pairs[pair];
  if (s0 >= pr.n_sym) return;                                // uniform over the workgroup
  const int n_here = pr.n_sym - s0 < MS_GROUP_SYMS ? pr.n_sym - s0 : MS_GROUP_SYMS;
  if (threadIdx.x < MS_GROUP_SYMS) {
    // a partial group repeats its first symmetry: a duplicate changes no min
    const int s = s0 + (static_cast<int>(threadIdx.x) < n_here ? threadIdx.x : 0);
    Rigid g;
    compose(pr.R_g, pr.t_g, syms + 12 * (static_cast<int64_t>(pr.sym_base) + s), g);
#pragma unroll
    for (int k = 0; k < 9; ++k) tr[threadIdx.x][k] = g.r[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tr[threadIdx.x][9 + k] = g.t[k];
  }
  __syncthreads();
  const int n = pr.n_verts;
  const double* X = verts + 3 * static_cast<int64_t>(pr.vert_base);
  const double fx = pr.fx, fy = pr.fy, cx = pr.cx, cy = pr.cy;
  double m3[MS_GROUP_SYMS], m2[MS_GROUP_SYMS];
#pragma unroll
  for (int k = 0; k < MS_GROUP_SYMS; ++k) m3[k] = m2[k] = 0.0;   // the errors are >= +0
  for (int v = threadIdx.x; v < n; v += PE_THREADS) {
    const double x = X[3 * v], y = X[3 * v + 1], z = X[3 * v + 2];
    double ex, ey, ez;
    apply(pr.R_e, pr.t_e, x, y, z, ex, ey, ez);
    const double ue = (fx * ex) / ez + cx, ve = (fy * ey) / ez + cy;
#pragma unroll
    for (int k = 0; k < MS_GROUP_SYMS; ++k) {
      double gx, gy, gz;
      apply(tr[k], tr[k] + 9, x, y, z, gx, gy, gz);
      const double d3 = sq3(ex - gx, ey - gy, ez - gz);
      m3[k] = d3 > m3[k] ? d3 : m3[k];
      const double ug = (fx * gx) / gz + cx, vg = (fy * gy) / gz + cy;
      const double du = ue - ug, dv = ve - vg;
      const double d2 = (ez <= 0.0 || gz <= 0.0) ? inf_f64() : du * du + dv * dv;
      m2[k] = d2 > m2[k] ? d2 : m2[k];
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < MS_GROUP_SYMS; ++k) {
    const double a = wave_max(m3[k]), b = wave_max(m2[k]);
    if (lane == 0) {
      red[wave][k] = a;
      red[wave][MS_GROUP_SYMS + k] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) {                                     // 0: MSSD, 1: MSPD
    double best = inf_f64();
    for (int k = 0; k < MS_GROUP_SYMS; ++k) {
      double m = red[0][threadIdx.x * MS_GROUP_SYMS + k];
      for (int w = 1; w < PE_WAVES; ++w) {
        const double o = red[w][threadIdx.x * MS_GROUP_SYMS + k];
        m = o > m ? o : m;
      }
      best = m < best ? m : best;
    }
    // non-negative doubles order as their bit patterns do
    atomicMin(reinterpret_cast<unsigned long long*>(err + 4 * static_cast<int64_t>(pair) +
                                                     threadIdx.x),
              static_cast<unsigned long long>(__double_as_longlong(best)));
  }
}

__global__ __launch_bounds__(PE_THREADS) void pose_finish_kernel(double* err, int n_pairs) {
  const int i = blockIdx.x * PE_THREADS + threadIdx.x;       // one thread per min cell
  if (i < 2 * n_pairs) {
    double* e = err + 4 * static_cast<int64_t>(i >> 1) + (i & 1);
    *e = sqrt(*e);
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_pose_error_group_syms(void) { return MS_GROUP_SYMS; }
extern "C" int epos_pose_error_adi_tile(void) { return ADI_TILE; }

extern "C" int epos_pose_errors_f64(const double* verts, int64_t n_verts_total,
                                    const double* syms, int64_t n_syms_total,
                                    const EposPosePair* pairs, EposPosePair* pairs_dev,
                                    int n_pairs, int want_adi, double* err, void* stream) {
  EPOS_REQUIRE(n_pairs >= 0, "n_pairs must be >= 0");
  EPOS_REQUIRE(n_verts_total >= 0 && n_syms_total >= 0, "negative pool size");
  if (n_pairs == 0) return EPOS_OK;
  EPOS_REQUIRE(verts && syms && pairs && pairs_dev && err, "null pointer");
  int max_sym = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const EposPosePair& p = pairs[i];
    EPOS_REQUIRE(p.n_verts >= 1, "n_verts must be >= 1");
    EPOS_REQUIRE(p.n_sym >= 1, "n_sym must be >= 1");
    EPOS_REQUIRE(p.vert_base >= 0 && int64_t(p.vert_base) + p.n_verts <= n_verts_total,
                 "vert_base + n_verts outside the pooled vertices");
    EPOS_REQUIRE(p.sym_base >= 0 && int64_t(p.sym_base) + p.n_sym <= n_syms_total,
                 "sym_base + n_sym outside the pooled symmetries");
    if (p.n_sym > max_sym) max_sym = p.n_sym;
  }
  const int64_t groups = ceil_div(max_sym, MS_GROUP_SYMS);
  EPOS_REQUIRE(groups * n_pairs < (int64_t(1) << 31), "n_pairs * symmetry groups must be < 2^31");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = check_hip(hipMemcpyAsync(pairs_dev, pairs, sizeof(EposPosePair) * n_pairs,
                                          hipMemcpyHostToDevice, s), "pair table upload");
  if (rc != EPOS_OK) return rc;
  const dim3 block(PE_THREADS), per_pair(static_cast<unsigned>(n_pairs));
  hipLaunchKernelGGL(pose_add_kernel, per_pair, block, 0, s, verts, syms, pairs_dev, err);
  if (want_adi)
    hipLaunchKernelGGL(pose_adi_kernel, per_pair, block, 0, s, verts, syms, pairs_dev, err);
  hipLaunchKernelGGL(pose_ms_kernel, dim3(static_cast<unsigned>(groups * n_pairs)), block, 0, s,
                     verts, syms, pairs_dev, static_cast<int>(groups), err);
  const dim3 cells(static_cast<unsigned>(ceil_div(2 * int64_t(n_pairs), PE_THREADS)));
  hipLaunchKernelGGL(pose_finish_kernel, cells, block, 0, s, err, n_pairs);
  return launch_status("pose_errors");
}
