// The input gradient of a 1x1 conv layer with a folded batch norm: D = mask (.) (G Wf^T) in fp64
// on the matrix pipe, rounded to fp32 once (include/epos_hip.h, "Pointwise input gradient";
// DESIGN.md, "Losses", "Backward through decoder_conv1").
//
//   pw_dgrad_fold_kernel  the workspace: Wf[k,c] = fl32(W[k,c] scale_c) widened to fp64, rows k
//                         padded to a multiple of 64 and columns c to a multiple of 16 with
//                         +0.0, so that the GEMM loads its weights without a bounds check.
//   pw_dgrad_kernel       a wave owns 32 rows x 64 columns of D as eight 16x16 accumulators of
//                         v_mfma_f64_16x16x4_f64 (64 rows measured 1.3 times the time at the
//                         workload, profiles/r28/); M is the parallel dimension, there is no
//                         split over c. A lane loads 16 bytes of a row of G (four consecutive c)
//                         and 32 bytes of a row of the workspace per tile and step of sixteen c:
//                         element e of the quads is reduction step e, so both operands come
//                         straight from their row-major layouts. Tile j of a wave holds the
//                         columns k = k0 + 4 * column + j: a lane ends up with FOUR consecutive
//                         k of a row and stores them, and reads the mask for them, with 16 bytes
//                         -- the fp16 pairs of a pre-split mask being exactly those 16 bytes.
//                         No LDS, no barrier; the loads run one step ahead of the MFMAs.
//
// One fp64 accumulator per (p, k) from +0.0, the c in an order the shape fixes; no atomics: the
// same bytes in every run and for a row at any position of M. -ffp-contract=off.
#include "h2_scale.h"

namespace epos {
namespace {

constexpr int DG_THREADS = 256;
// 16-row blocks of a wave's tile. 2 is what the library ships and the only value the tests
// run; -DEPOS_DGRAD_ROW_BLOCKS=4 (64 rows) is the build profiles/r28/ compares it with.
#ifndef EPOS_DGRAD_ROW_BLOCKS
#define EPOS_DGRAD_ROW_BLOCKS 2
#endif
constexpr int DG_RB = EPOS_DGRAD_ROW_BLOCKS;   // 16-row blocks of a wave's tile
constexpr int DG_ROWS = 16 * DG_RB;           // a wave's block of D: DG_ROWS rows ...
constexpr int DG_TILE = 64;                   // ... of 64 columns
constexpr int DG_STEP = 16;                   // values of c per step: four MFMAs a tile

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

enum { MASK_NONE = 0, MASK_F32 = 1, MASK_H2 = 2 };

int64_t padded_k(int K) { return round_up(K, DG_TILE); }
int64_t padded_n(int N) { return round_up(N, DG_STEP); }

__global__ __launch_bounds__(DG_THREADS) void pw_dgrad_fold_kernel(
    const float* __restrict__ W, int K, int N, const float* __restrict__ gamma,
    const float* __restrict__ var, double eps, double* __restrict__ Wd, int64_t kp, int64_t np) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * DG_THREADS + threadIdx.x;
  if (i >= kp * np) return;
  const int64_t k = i / np, c = i % np;
  double v = 0.0;
  if (k < K && c < N) {
    float w = W[k * N + c];
    if (gamma != nullptr) {
      const double sd = sqrt(static_cast<double>(var[c]) + eps);
      const float scale = static_cast<float>(static_cast<double>(gamma[c]) / sd);
      w = w * scale;                          // one fp32 product, as the forward's fold
    }
    v = static_cast<double>(w);
  }
  Wd[i] = v;
}

// Four consecutive values of a row: columns col .. col + 3, zeros past `cols` and for a row that
// is not there. VEC needs cols % 4 == 0 and 16-byte aligned rows.
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

// [hi(k..k+3) | mid(k..k+3)] -> hi + mid 2^-11, exact in fp64: only its sign is used
__device__ __forceinline__ void pair_values(float4 raw, double (&d)[4]) {
  const h2_f16x2 h01 = __builtin_bit_cast(h2_f16x2, raw.x);
  const h2_f16x2 h23 = __builtin_bit_cast(h2_f16x2, raw.y);
  const h2_f16x2 m01 = __builtin_bit_cast(h2_f16x2, raw.z);
  const h2_f16x2 m23 = __builtin_bit_cast(h2_f16x2, raw.w);
  d[0] = static_cast<double>(h01.x) + static_cast<double>(m01.x) * (1.0 / 2048.0);
  d[1] = static_cast<double>(h01.y) + static_cast<double>(m01.y) * (1.0 / 2048.0);
  d[2] = static_cast<double>(h23.x) + static_cast<double>(m23.x) * (1.0 / 2048.0);
  d[3] = static_cast<double>(h23.y) + static_cast<double>(m23.y) * (1.0 / 2048.0);
}

struct Operands {
  float4 g[DG_RB];                            // the row blocks of the wave
  f64x2 w[4][2];                              // the four tiles' weights, steps (0,1) and (2,3)
};

template <bool VG>
__global__ __launch_bounds__(DG_THREADS) void pw_dgrad_kernel(
    const float* __restrict__ G, int64_t ldg, const double* __restrict__ Wd, int64_t np,
    int64_t M, int K, int N, int k_blocks, const float* __restrict__ mask, int64_t ldm,
    int mask_mode, bool vec_mask, float* __restrict__ D, int64_t ldd, bool vec_d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = static_cast<int64_t>(blockIdx.x) * (DG_THREADS / 64) + wave;
  const int64_t p0 = tile / k_blocks * DG_ROWS;
  if (p0 >= M) return;                        // the whole wave: there is no barrier below
  const int k0 = static_cast<int>(tile % k_blocks) * DG_TILE;

  const float* g_row[DG_RB];
  bool g_ok[DG_RB];
  const double* w_row[4];
#pragma unroll
  for (int i = 0; i < DG_RB; ++i) {
    const int64_t p = p0 + 16 * i + n;
    g_ok[i] = p < M;
    g_row[i] = G + (g_ok[i] ? p : 0) * ldg;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) w_row[j] = Wd + static_cast<int64_t>(k0 + 4 * n + j) * np + 4 * q;

  auto load = [&](int64_t step, Operands& o) {
    const int c = static_cast<int>(step) * DG_STEP + 4 * q;
#pragma unroll
    for (int i = 0; i < DG_RB; ++i) o.g[i] = load_quad<VG>(g_row[i], g_ok[i], c, N);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f64x2* w = reinterpret_cast<const f64x2*>(w_row[j] + step * DG_STEP);
      o.w[j][0] = w[0];
      o.w[j][1] = w[1];
    }
  };

  f64x4 acc[DG_RB][4];
#pragma unroll
  for (int i = 0; i < DG_RB; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t steps = np / DG_STEP;
  Operands cur, next;
  load(0, cur);
  next = cur;
  for (int64_t step = 0; step < steps; ++step) {
    // the workspace holds a whole step behind the last one only when there is one
    if (step + 1 < steps) load(step + 1, next);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double gv[DG_RB], wv[4];
#pragma unroll
      for (int i = 0; i < DG_RB; ++i) {
        const float4 g = cur.g[i];
        gv[i] = static_cast<double>(e == 0 ? g.x : e == 1 ? g.y : e == 2 ? g.z : g.w);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = cur.w[j][e >> 1][e & 1];
#pragma unroll
      for (int i = 0; i < DG_RB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(gv[i], wv[j], acc[i][j], 0, 0, 0);
    }
    cur = next;
  }

  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register. Tile (i, j) holds
  // D[p0 + 16 i + row][k0 + 4 * column + j]: the lane's four tiles j are four consecutive k.
  const int k = k0 + 4 * n;
  if (k >= K) return;
#pragma unroll
  for (int i = 0; i < DG_RB; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t p = p0 + 16 * i + q + 4 * reg;
      if (p >= M) continue;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = static_cast<float>(acc[i][j][reg]);
      if (mask_mode != MASK_NONE) {
        const float* m_row = mask + p * ldm;
        if (mask_mode == MASK_H2) {
          double m[4];
          pair_values(*reinterpret_cast<const float4*>(m_row + k), m);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = m[j] <= 0.0 ? 0.f : v[j];
        } else {
          const float4 m = vec_mask ? load_quad<true>(m_row, true, k, K)
                                    : load_quad<false>(m_row, true, k, K);
          // columns past K read as 0 and are not stored
          v[0] = m.x <= 0.f ? 0.f : v[0];
          v[1] = m.y <= 0.f ? 0.f : v[1];
          v[2] = m.z <= 0.f ? 0.f : v[2];
          v[3] = m.w <= 0.f ? 0.f : v[3];
        }
      }
      float* d_row = D + p * ldd;
      if (vec_d) {
        *reinterpret_cast<float4*>(d_row + k) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < K) d_row[k + j] = v[j];
      }
    }
}

bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_pointwise_dgrad_workspace_bytes(int K, int N) {
  EPOS_REQUIRE(K >= 1 && N >= 1 && K <= 1024 && N <= 1024, "K and N must be in 1..1024");
  return 8 * padded_k(K) * padded_n(N);
}

extern "C" int epos_pointwise_dgrad_f32(const EposPointwiseDgradArgs* args, void* stream) {
  EPOS_REQUIRE(args, "null args");
  const EposPointwiseDgradArgs& a = *args;
  EPOS_REQUIRE(a.M >= 1 && a.K >= 1 && a.N >= 1, "M, K and N must be positive");
  EPOS_REQUIRE(a.K <= 1024 && a.N <= 1024, "K and N must be in 1..1024");
  EPOS_REQUIRE(a.M <= (int64_t{1} << 33), "M too large");
  EPOS_REQUIRE(a.ldg >= a.N, "ldg must be >= N");
  EPOS_REQUIRE(a.ldd >= a.K, "ldd must be >= K");
  EPOS_REQUIRE(a.G && a.W && a.D && a.workspace, "null pointer");
  EPOS_REQUIRE(!a.mask || a.ldm >= a.K, "ldm must be >= K");
  EPOS_REQUIRE((a.gamma != nullptr) == (a.moving_variance != nullptr),
               "gamma and moving_variance are given together or not at all");
  EPOS_REQUIRE(!a.gamma || (a.eps >= 0.0 && a.eps == a.eps), "eps must be a non-negative number");
  EPOS_REQUIRE(al(a.G, 4) && al(a.W, 4) && al(a.D, 4) && al(a.mask, 4) && al(a.gamma, 4) &&
               al(a.moving_variance, 4) && al16(a.workspace),
               "G, W, D, mask, gamma and moving_variance must be 4-byte aligned, the workspace "
               "16-byte aligned");
  const bool h2 = a.mask && a.mask_h2;
  EPOS_REQUIRE(!h2 || (a.K % 4 == 0 && a.ldm % 4 == 0 && al16(a.mask)),
               "a pre-split mask needs K % 4 == 0, ldm % 4 == 0 and 16-byte aligned rows");
  EPOS_REQUIRE(static_cast<const void*>(a.D) != static_cast<const void*>(a.G) &&
               static_cast<const void*>(a.D) != a.mask, "D may not start at G or at mask");
  const int64_t kp = padded_k(a.K), np = padded_n(a.N);
  const int k_blocks = static_cast<int>(kp / DG_TILE);
  const int64_t tiles = ceil_div(a.M, DG_ROWS) * k_blocks;
  const int64_t blocks = ceil_div(tiles, DG_THREADS / 64);
  EPOS_REQUIRE(blocks <= 0x7fffffff, "too many blocks");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* Wd = static_cast<double*>(a.workspace);
  hipLaunchKernelGGL(pw_dgrad_fold_kernel, dim3(blocks_for(kp * np, DG_THREADS)),
                     dim3(DG_THREADS), 0, s, a.W, a.K, a.N, a.gamma, a.moving_variance, a.eps, Wd,
                     kp, np);
  const int rc = launch_status("pw_dgrad_fold_kernel");
  if (rc != EPOS_OK) return rc;
  const bool vg = a.N % 4 == 0 && a.ldg % 4 == 0 && al16(a.G);
  const bool vd = a.K % 4 == 0 && a.ldd % 4 == 0 && al16(a.D);
  const bool vm = a.mask && a.K % 4 == 0 && a.ldm % 4 == 0 && al16(a.mask);
  const int mode = !a.mask ? MASK_NONE : h2 ? MASK_H2 : MASK_F32;
  const float* mask = static_cast<const float*>(a.mask);
#define EPOS_DGRAD_LAUNCH(VG)                                                                    \
  hipLaunchKernelGGL((pw_dgrad_kernel<VG>), dim3(static_cast<unsigned>(blocks)),                 \
                     dim3(DG_THREADS), 0, s, a.G, a.ldg, Wd, np, a.M, a.K, a.N, k_blocks, mask,  \
                     a.ldm, mode, vm, a.D, a.ldd, vd)
  if (vg) EPOS_DGRAD_LAUNCH(true); else EPOS_DGRAD_LAUNCH(false);
#undef EPOS_DGRAD_LAUNCH
  return launch_status("pw_dgrad_kernel");
}
