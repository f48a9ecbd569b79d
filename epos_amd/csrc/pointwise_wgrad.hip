// The weight gradient of a 1x1 conv layer with a frozen batch norm: S = A^T G and g = the column
// sums of G in fp64 on the matrix pipe, then the checkpoint-shaped fp32 gradients from them
// (include/epos_hip.h, "Pointwise weight gradient"; DESIGN.md, "Losses", "Decoder layer
// gradients").
//
//   pw_wgrad_kernel        a workgroup of four waves owns a 128 x 128 block of S and ONE row
//                          range of M; a wave owns 64 x 64 of it as sixteen 16x16 accumulators
//                          of v_mfma_f64_16x16x4_f64. A lane loads 16 bytes of a row of A and 16
//                          of the same row of G per step (four rows a step, sixteen lanes a
//                          row), the fp16 pairs of a pre-split A being exactly those 16 bytes:
//                          element e of a lane's quad belongs to accumulator column / row e, so
//                          a 16x16 tile holds every FOURTH row and column of the wave's 64 x 64.
//                          No LDS, no barrier; the loads run two steps ahead of the MFMAs. The
//                          waves whose block starts at k = 0 also add their G values per lane:
//                          the column sums.
//   pw_wgrad_sum_kernel    with more than one row range: adds the ranges' slabs in range order.
//   pw_wgrad_close_kernel  epos_pointwise_wgrad_close_f32: dW, dgamma and dbeta (or dW, db).
//
// Every sum over rows is taken in fp64 from +0.0; which rows a range holds depends on (M, K, N)
// only; no atomics: the same bytes in every run. -ffp-contract=off.
#include "h2_scale.h"

namespace epos {
namespace {

constexpr int WG_THREADS = 256;
constexpr int WG_TILE = 128;                  // a workgroup's block of S, both ways
constexpr int WG_TARGET = 256;                // workgroups to aim for: one per compute unit

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { A_SCALAR = 0, A_VEC = 1, A_H2 = 2 };

struct Ranges {
  int64_t rows;                               // per range, a multiple of 4
  int64_t count;
  int64_t blocks;                             // 128 x 128 blocks of S
};

// A function of (M, K, N) only: the cut decides the order of the sums
Ranges ranges_for(int64_t M, int64_t K, int64_t N) {
  Ranges r;
  r.blocks = ceil_div(K, WG_TILE) * ceil_div(N, WG_TILE);
  int64_t want = WG_TARGET / r.blocks;
  if (want < 1) want = 1;
  const int64_t most = ceil_div(M, 128);     // a range is worth its slab from 128 rows on
  if (want > most) want = most;
  r.rows = round_up(ceil_div(M, want), 4);
  r.count = ceil_div(M, r.rows);
  return r;
}

// Four consecutive values of a row, as fp64: columns col .. col + 3, zeros past `cols` and for a
// row that is not there. VEC needs cols % 4 == 0 and 16-byte aligned rows.
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* row, bool row_ok, int col, int cols) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (VEC) {
    if (row_ok && col < cols) v = *reinterpret_cast<const float4*>(row + col);
  } else {
    if (row_ok) {
      if (col < cols) v.x = row[col];
      if (col + 1 < cols) v.y = row[col + 1];
      if (col + 2 < cols) v.z = row[col + 2];
      if (col + 3 < cols) v.w = row[col + 3];
    }
  }
  return v;
}

__device__ __forceinline__ void widen(float4 v, double (&d)[4]) {
  d[0] = static_cast<double>(v.x);
  d[1] = static_cast<double>(v.y);
  d[2] = static_cast<double>(v.z);
  d[3] = static_cast<double>(v.w);
}

// [hi(c..c+3) | mid(c..c+3)] -> (hi + mid 2^-11) inv, exact in fp64
__device__ __forceinline__ void widen_h2(float4 raw, double inv, double (&d)[4]) {
  const h2_f16x2 h01 = __builtin_bit_cast(h2_f16x2, raw.x);
  const h2_f16x2 h23 = __builtin_bit_cast(h2_f16x2, raw.y);
  const h2_f16x2 m01 = __builtin_bit_cast(h2_f16x2, raw.z);
  const h2_f16x2 m23 = __builtin_bit_cast(h2_f16x2, raw.w);
  const double hi[4] = {static_cast<double>(h01.x), static_cast<double>(h01.y),
                        static_cast<double>(h23.x), static_cast<double>(h23.y)};
  const double mid[4] = {static_cast<double>(m01.x), static_cast<double>(m01.y),
                         static_cast<double>(m23.x), static_cast<double>(m23.y)};
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = (hi[e] + mid[e] * (1.0 / 2048.0)) * inv;
}

template <int AMODE, bool VG>
__global__ __launch_bounds__(WG_THREADS) void pw_wgrad_kernel(
    const float* __restrict__ A, int64_t lda, const float* __restrict__ G, int64_t ldg,
    int64_t M, int K, int N, int64_t range_rows, int n_blocks, const unsigned* __restrict__ amax,
    const unsigned* __restrict__ amax2, float gain, float bias, double* __restrict__ S_out,
    double* __restrict__ g_out, int64_t slab_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int kb = blockIdx.x / n_blocks, nb = blockIdx.x % n_blocks;
  const int k0 = kb * WG_TILE + 64 * (wave >> 1);
  const int n0 = nb * WG_TILE + 64 * (wave & 1);
  if (k0 >= K || n0 >= N) return;             // the whole wave: there is no barrier below
  const int64_t m0 = static_cast<int64_t>(blockIdx.y) * range_rows;
  const int64_t m1 = m0 + range_rows < M ? m0 + range_rows : M;
  double inv = 1.0;
  if constexpr (AMODE == A_H2) {
    float s, inv_s;
    h2_scale(amax, amax2, gain, bias, lane, s, inv_s);
    inv = static_cast<double>(inv_s);
  }
  const int ka = k0 + 4 * c, na = n0 + 4 * c;
  const bool sum_g = k0 == 0;

  f64x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  double gs[4] = {0.0, 0.0, 0.0, 0.0};

  const int64_t steps = (m1 - m0 + 3) / 4;
  auto load_a = [&](int64_t step) {
    const int64_t p = m0 + 4 * step + q;
    return load_quad<AMODE != A_SCALAR>(A + p * lda, p < m1, ka, K);
  };
  auto load_g = [&](int64_t step) {
    const int64_t p = m0 + 4 * step + q;
    return load_quad<VG>(G + p * ldg, p < m1, na, N);
  };
  float4 a_0 = load_a(0), g_0 = load_g(0);
  float4 a_1 = load_a(1), g_1 = load_g(1);
  for (int64_t step = 0; step < steps; ++step) {
    const float4 a_2 = load_a(step + 2), g_2 = load_g(step + 2);
    double av[4], gv[4];
    if constexpr (AMODE == A_H2) widen_h2(a_0, inv, av);
    else widen(a_0, av);
    widen(g_0, gv);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], gv[j], acc[i][j], 0, 0, 0);
    if (sum_g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) gs[j] += gv[j];
    }
    a_0 = a_1; g_0 = g_1;
    a_1 = a_2; g_1 = g_2;
  }

  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register. Tile (i, j) holds
  // S[k0 + 4 * row + i][n0 + 4 * column + j].
  double* S_slab = S_out + blockIdx.y * slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int k = k0 + 4 * (q + 4 * reg) + i;
      if (k >= K) continue;
      double* row = S_slab + static_cast<int64_t>(k) * N;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (na + j < N) row[na + j] = acc[i][j][reg];
    }
  if (sum_g) {
    double* g_slab = g_out + blockIdx.y * slab_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {             // the four row groups, in their order
      const double t0 = __shfl(gs[j], c, 64), t1 = __shfl(gs[j], c + 16, 64);
      const double t2 = __shfl(gs[j], c + 32, 64), t3 = __shfl(gs[j], c + 48, 64);
      const double t = ((t0 + t1) + t2) + t3;
      if (q == 0 && na + j < N) g_slab[na + j] = t;
    }
  }
}

// S and g = the sum of the ranges' slabs [K * N | N], in range order, from +0.0
__global__ __launch_bounds__(WG_THREADS) void pw_wgrad_sum_kernel(
    const double* __restrict__ slabs, int64_t slab_stride, int64_t count, int64_t kn, int64_t n,
    double* __restrict__ S, double* __restrict__ g) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * WG_THREADS + threadIdx.x;
  if (i >= kn + n) return;
  double t = 0.0;
  for (int64_t r = 0; r < count; ++r) t += slabs[r * slab_stride + i];
  if (i < kn) S[i] = t;
  else g[i - kn] = t;
}

// 16 columns a workgroup, 16 threads a column: each takes every 16th k, ascending; the 16
// partial sums of W S are added in their order.
__global__ __launch_bounds__(WG_THREADS) void pw_wgrad_close_kernel(
    const double* __restrict__ S, const double* __restrict__ g, const float* __restrict__ W,
    int K, int N, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ var, double eps, float* __restrict__ dW,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double part[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + tx;
  const bool bn = gamma != nullptr;
  double scale = 1.0, rstd = 1.0, dot = 0.0;
  if (col < N) {
    if (bn) {
      const double sd = sqrt(static_cast<double>(var[col]) + eps);
      rstd = 1.0 / sd;
      scale = static_cast<double>(static_cast<float>(static_cast<double>(gamma[col]) / sd));
    }
    for (int k = ty; k < K; k += 16) {
      const int64_t at = static_cast<int64_t>(k) * N + col;
      const double s = S[at];
      // + 0.0: a negative scale leaves +0.0 where S is +0.0
      dW[at] = static_cast<float>(bn ? scale * s + 0.0 : s);
      if (bn) dot += static_cast<double>(W[at]) * s;
    }
  }
  part[ty][tx] = dot;
  __syncthreads();
  if (ty != 0 || col >= N) return;
  const double gc = g[col];
  dbeta[col] = static_cast<float>(gc);
  if (!bn) return;
  double t = 0.0;
  for (int i = 0; i < 16; ++i) t += part[i][tx];
  dgamma[col] = static_cast<float>(rstd * (t - static_cast<double>(mean[col]) * gc) + 0.0);
}

bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_pointwise_wgrad_workspace_bytes(int64_t M, int K, int N) {
  EPOS_REQUIRE(M >= 1 && K >= 1 && N >= 1, "M, K and N must be positive");
  const Ranges r = ranges_for(M, K, N);
  if (r.count <= 1) return 0;
  return r.count * 8 * (static_cast<int64_t>(K) * N + N);
}

extern "C" int64_t epos_pointwise_wgrad_range_rows(int64_t M, int K, int N) {
  EPOS_REQUIRE(M >= 1 && K >= 1 && N >= 1, "M, K and N must be positive");
  return ranges_for(M, K, N).rows;
}

extern "C" int epos_pointwise_wgrad_f32(const EposPointwiseWgradArgs* args, void* stream) {
  EPOS_REQUIRE(args, "null args");
  const EposPointwiseWgradArgs& a = *args;
  EPOS_REQUIRE(a.M >= 1 && a.K >= 1 && a.N >= 1, "M, K and N must be positive");
  EPOS_REQUIRE(a.M <= (int64_t{1} << 40), "M too large");
  EPOS_REQUIRE(a.lda >= a.K, "lda must be >= K");
  EPOS_REQUIRE(a.ldg >= a.N, "ldg must be >= N");
  EPOS_REQUIRE(a.A && a.G && a.S && a.g, "null pointer");
  EPOS_REQUIRE(al(a.A, 4) && al(a.G, 4) && al(a.S, 8) && al(a.g, 8),
               "A and G must be 4-byte aligned, S and g 8-byte aligned");
  if (a.a_presplit) {
    EPOS_REQUIRE(a.a_amax, "a pre-split A needs its absmax slot (a_amax)");
    EPOS_REQUIRE(a.K % 4 == 0 && a.lda % 4 == 0 && al16(a.A),
                 "a pre-split A needs K % 4 == 0, lda % 4 == 0 and 16-byte aligned rows");
  }
  const Ranges r = ranges_for(a.M, a.K, a.N);
  const int64_t kn = static_cast<int64_t>(a.K) * a.N;
  EPOS_REQUIRE(r.count <= 1 || (a.workspace && al(a.workspace, 8)),
               "the workspace must be given, 8-byte aligned");
  EPOS_REQUIRE(r.blocks <= 0x7fffffff && r.count <= 65535, "too many blocks");
  const bool va = a.K % 4 == 0 && a.lda % 4 == 0 && al16(a.A);
  const bool vg = a.N % 4 == 0 && a.ldg % 4 == 0 && al16(a.G);
  const int mode = a.a_presplit ? A_H2 : va ? A_VEC : A_SCALAR;
  double* S_out = a.S;
  double* g_out = a.g;
  int64_t stride = 0;
  if (r.count > 1) {
    S_out = static_cast<double*>(a.workspace);
    g_out = S_out + kn;
    stride = kn + a.N;
  }
  const dim3 grid(static_cast<unsigned>(r.blocks), static_cast<unsigned>(r.count));
  const int n_blocks = static_cast<int>(ceil_div(a.N, WG_TILE));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* A = static_cast<const float*>(a.A);
#define EPOS_WGRAD_LAUNCH(MODE, VG)                                                              \
  hipLaunchKernelGGL((pw_wgrad_kernel<MODE, VG>), grid, dim3(WG_THREADS), 0, s, A, a.lda, a.G,   \
                     a.ldg, a.M, a.K, a.N, r.rows, n_blocks, a.a_amax, a.a_amax2, a.a_gain,      \
                     a.a_bias, S_out, g_out, stride)
  if (mode == A_H2) { if (vg) EPOS_WGRAD_LAUNCH(A_H2, true); else EPOS_WGRAD_LAUNCH(A_H2, false); }
  else if (mode == A_VEC) {
    if (vg) EPOS_WGRAD_LAUNCH(A_VEC, true); else EPOS_WGRAD_LAUNCH(A_VEC, false);
  } else {
    if (vg) EPOS_WGRAD_LAUNCH(A_SCALAR, true); else EPOS_WGRAD_LAUNCH(A_SCALAR, false);
  }
#undef EPOS_WGRAD_LAUNCH
  int rc = launch_status("pw_wgrad_kernel");
  if (rc != EPOS_OK || r.count <= 1) return rc;
  hipLaunchKernelGGL(pw_wgrad_sum_kernel, dim3(blocks_for(kn + a.N, WG_THREADS)),
                     dim3(WG_THREADS), 0, s, static_cast<const double*>(a.workspace), stride,
                     r.count, kn, static_cast<int64_t>(a.N), a.S, a.g);
  return launch_status("pw_wgrad_sum_kernel");
}

extern "C" int epos_pointwise_wgrad_close_f32(const double* S, const double* g, const float* W,
                                              int K, int N, const float* gamma,
                                              const float* moving_mean,
                                              const float* moving_variance, double eps, float* dW,
                                              float* dgamma, float* dbeta, void* stream) {
  EPOS_REQUIRE(K >= 1 && N >= 1, "K and N must be positive");
  EPOS_REQUIRE(S && g && dW && dbeta, "null pointer");
  const bool bn = gamma != nullptr;
  if (bn) {
    EPOS_REQUIRE(W && moving_mean && moving_variance && dgamma,
                 "with a batch norm W, moving_mean, moving_variance and dgamma are needed");
    EPOS_REQUIRE(eps >= 0.0 && eps == eps, "eps must be a non-negative number");
  } else {
    EPOS_REQUIRE(!moving_mean && !moving_variance && !dgamma,
                 "without gamma there is no batch norm: moving_mean, moving_variance and "
                 "dgamma must be NULL");
  }
  EPOS_REQUIRE(al(S, 8) && al(g, 8) && al(dW, 4) && al(dbeta, 4), "misaligned pointer");
  hipLaunchKernelGGL(pw_wgrad_close_kernel, dim3(blocks_for(N, 16)), dim3(WG_THREADS), 0,
                     static_cast<hipStream_t>(stream), S, g, W, K, N, gamma, moving_mean,
                     moving_variance, eps, dW, dgamma, dbeta);
  return launch_status("pw_wgrad_close_kernel");
}
