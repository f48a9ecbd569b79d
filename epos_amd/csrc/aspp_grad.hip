// The backward pass through ASPP's fan-out (include/epos_hip.h, "ASPP gradients"; DESIGN.md,
// "Losses", "Backward through ASPP").
//
//   pool_sum_kernel        the adjoint of the image-pooling broadcast, g[b,c] = sum_p D[b,p,c],
//                          over ONE range of an image's pixels: a thread owns four consecutive
//                          channels and every PS-th pixel of the range (the slots of
//                          dw_wgrad_kernel), one fp64 sum per channel; the slots' sums are then
//                          added in slot order through LDS.
//   pool_sum_close_kernel  with more than one range: adds the ranges' slabs in range order.
//   join_kernel            the gradient at a tensor that feeds several branches, in one pass over
//                          the output: plain terms, the mirrored taps of up to four depthwise
//                          terms, a per-image term and the ReLU mask, one fp64 accumulator per
//                          element in a fixed order. Partitions of the same elements (pixel-
//                          major; channel slices of 32 or 64, one, two or four pixels a
//                          thread): the bytes do not depend on it.
//
// No atomics: the same bytes in every run. -ffp-contract=off.
#include "common.h"

namespace epos {
namespace {

constexpr int AG_THREADS = 256;
constexpr int64_t POOL_MIN_RANGE = 64;        // pixels: below that a slab costs more than it saves
constexpr int64_t POOL_RANGES = 64;           // ranges an image is cut into at most
constexpr int POOL_QUADS = 16;                // channel quads a workgroup owns at most
constexpr int XCDS = 8;                       // workgroup b and b + XCDS share an L2 (observed)

// A function of P only: the cut decides the order of the sums
int64_t pool_range(int64_t P) {
  const int64_t r = ceil_div(P, POOL_RANGES);
  return r < POOL_MIN_RANGE ? POOL_MIN_RANGE : r;
}

// out_f (count == 1): g itself, rounded; out_d: slab [b][range][C] in fp64
__global__ __launch_bounds__(AG_THREADS) void pool_sum_kernel(
    const float* __restrict__ D, int64_t ldd, int64_t P, int C, int64_t range, int q_wide,
    int slots, float* __restrict__ out_f, int64_t ldg, double* __restrict__ out_d) {
  __shared__ double part[AG_THREADS][4];
  const int tid = threadIdx.x;
  const int qi = tid % q_wide, slot = tid / q_wide;
  const int c = 4 * (blockIdx.x * q_wide + qi);
  const bool active = slot < slots && c < C;
  const int64_t b = blockIdx.z;
  const int64_t p0 = static_cast<int64_t>(blockIdx.y) * range;
  const int64_t p1 = p0 + range < P ? p0 + range : P;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (active) {
    const float* src = D + b * P * ldd + c;
    for (int64_t p = p0 + slot; p < p1; p += slots) {
      const float4 d = *reinterpret_cast<const float4*>(src + p * ldd);
      acc[0] += static_cast<double>(d.x);
      acc[1] += static_cast<double>(d.y);
      acc[2] += static_cast<double>(d.z);
      acc[3] += static_cast<double>(d.w);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[tid][e] = acc[e];
  __syncthreads();
  if (!active || slot != 0) return;
  double s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s[e] = 0.0;
    for (int k = 0; k < slots; ++k) s[e] += part[k * q_wide + qi][e];
  }
  if (out_f != nullptr) {
    *reinterpret_cast<float4*>(out_f + b * ldg + c) =
        make_float4(static_cast<float>(s[0]), static_cast<float>(s[1]), static_cast<float>(s[2]),
                    static_cast<float>(s[3]));
  } else {
    double* dst = out_d + (b * gridDim.y + blockIdx.y) * C + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = s[e];
  }
}

// g[b,c] = fl32(the sum of the ranges' slabs in range order, from +0.0)
__global__ __launch_bounds__(AG_THREADS) void pool_sum_close_kernel(
    const double* __restrict__ slabs, int64_t count, int C, int64_t total,
    float* __restrict__ g, int64_t ldg) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * AG_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / C;
  const int c = static_cast<int>(i - b * C);
  const double* src = slabs + b * count * C + c;
  double s = 0.0;
  for (int64_t r = 0; r < count; ++r) s += src[r * C];
  g[b * ldg + c] = static_cast<float>(s);
}

// a += w * d for a tap that is there, w already in fp64 (the conversion is exact); one that is
// not adds +0.0 (never 0 * d)
__device__ __forceinline__ void tap4_if(double (&a)[4], const double (&w)[4], float4 d, bool ok) {
  const double p0 = w[0] * static_cast<double>(d.x);
  const double p1 = w[1] * static_cast<double>(d.y);
  const double p2 = w[2] * static_cast<double>(d.z);
  const double p3 = w[3] * static_cast<double>(d.w);
  a[0] += ok ? p0 : 0.0;
  a[1] += ok ? p1 : 0.0;
  a[2] += ok ? p2 : 0.0;
  a[3] += ok ? p3 : 0.0;
}

// Four channels (c..c+3) of the NPIX pixels i0, i0 + step, ... (those below P): the whole sum,
// the rounding, the mask and the store of each. The pixels share what does not depend on the
// pixel -- a tap's weights, converted to fp64 once, and its offset, which is the same for the
// whole wave; every element keeps its own accumulator and its own order.
template <int NPIX>
__device__ __forceinline__ void join_elements(const EposAsppJoinArgs& a, int64_t i0,
                                              int64_t step, int64_t P, int c) {
  int64_t i[NPIX];
  bool live[NPIX];
  int x[NPIX], y[NPIX];
  double acc[NPIX][4];
#pragma unroll
  for (int n = 0; n < NPIX; ++n) {
    i[n] = i0 + n * step;
    live[n] = i[n] < P;
    if (!live[n]) i[n] = i0;                  // loaded from a pixel that is there, not stored
    x[n] = static_cast<int>(i[n] % a.W);
    y[n] = static_cast<int>(i[n] / a.W % a.H);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[n][e] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < a.n_plain) {
#pragma unroll
      for (int n = 0; n < NPIX; ++n) {
        const float4 e =
            *reinterpret_cast<const float4*>(a.plain[j].E + i[n] * a.plain[j].lde + c);
        acc[n][0] += static_cast<double>(e.x);
        acc[n][1] += static_cast<double>(e.y);
        acc[n][2] += static_cast<double>(e.z);
        acc[n][3] += static_cast<double>(e.w);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < a.n_dw) {
      const float* D = a.dw[t].D + c;
      const float* w9c = a.dw[t].w9c + c;
      const int64_t ldd = a.dw[t].ldd;
      const int64_t rate = a.dw[t].rate;
      // every tap is loaded, one outside the image from the pixel itself, and then not added:
      // no load sits under a branch
      float4 dv[NPIX][9];
      bool ok[NPIX][9];
#pragma unroll
      for (int n = 0; n < NPIX; ++n) {
        const float* at = D + i[n] * ldd;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int64_t yy = y[n] - (ky - 1) * rate;
          const bool oky = yy >= 0 && yy < a.H;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int64_t xx = x[n] - (kx - 1) * rate;
            const int tap = 3 * ky + kx;
            ok[n][tap] = oky && xx >= 0 && xx < a.W;
            const int64_t back = ((ky - 1) * rate * a.W + (kx - 1) * rate) * ldd;   // uniform
            dv[n][tap] = *reinterpret_cast<const float4*>(at - (ok[n][tap] ? back : 0));
          }
        }
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float4 w = *reinterpret_cast<const float4*>(w9c + static_cast<int64_t>(tap) * a.C);
        const double wd[4] = {static_cast<double>(w.x), static_cast<double>(w.y),
                              static_cast<double>(w.z), static_cast<double>(w.w)};
#pragma unroll
        for (int n = 0; n < NPIX; ++n) tap4_if(acc[n], wd, dv[n][tap], ok[n][tap]);
      }
    }
  }
  const int64_t hw = static_cast<int64_t>(a.H) * a.W;
  const double div = static_cast<double>(a.pool_div);
#pragma unroll
  for (int n = 0; n < NPIX; ++n) {
    if (a.Pool != nullptr) {
      const float4 p = *reinterpret_cast<const float4*>(a.Pool + i[n] / hw * a.ldp + c);
      acc[n][0] += static_cast<double>(p.x) / div;
      acc[n][1] += static_cast<double>(p.y) / div;
      acc[n][2] += static_cast<double>(p.z) / div;
      acc[n][3] += static_cast<double>(p.w) / div;
    }
    float4 v = make_float4(static_cast<float>(acc[n][0]), static_cast<float>(acc[n][1]),
                           static_cast<float>(acc[n][2]), static_cast<float>(acc[n][3]));
    if (a.Y != nullptr) {
      const float4 m = *reinterpret_cast<const float4*>(a.Y + i[n] * a.ldy + c);
      v.x = m.x <= 0.f ? 0.f : v.x;
      v.y = m.y <= 0.f ? 0.f : v.y;
      v.z = m.z <= 0.f ? 0.f : v.z;
      v.w = m.w <= 0.f ? 0.f : v.w;
    }
    if (live[n]) *reinterpret_cast<float4*>(a.dX + i[n] * a.ldx + c) = v;
  }
}

// Pixel-major: consecutive threads along the channel axis, all channels of a pixel together
// (dw_dgrad_kernel's partition). A tap's neighbours are rate * W * C floats away: no reuse
// before the whole tensor has gone by.
__global__ __launch_bounds__(AG_THREADS) void join_pixel_kernel(const EposAsppJoinArgs a,
                                                                int64_t total, int64_t P) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * AG_THREADS + threadIdx.x;
  if (g >= total) return;
  const int quads = a.C / 4;
  join_elements<1>(a, g / quads, 0, P, 4 * static_cast<int>(g % quads));
}

// Channel slices: a workgroup owns Q quads (Q = 8: one 128-byte line a pixel) of NPIX * 256 / Q
// consecutive pixels, a thread NPIX of them, 256 / Q apart. The workgroups of a slice are dealt
// to ONE XCD -- workgroup ids that are congruent mod 8 -- and follow each other there, so that a
// slice of every operand (H W 16 Q bytes an image) stays in that XCD's L2 while its nine taps
// are read. For speed only: where the dispatcher deals differently the bytes are the same.
template <int Q, int NPIX>
__global__ __launch_bounds__(AG_THREADS) void join_slice_kernel(const EposAsppJoinArgs a,
                                                                int64_t P, int slices,
                                                                int64_t units) {
  constexpr int PIX = AG_THREADS / Q;
  const int64_t id = blockIdx.x;
  const int xcd = static_cast<int>(id % XCDS);
  const int64_t j = id / XCDS;
  const int64_t slice = (j / units) * XCDS + xcd;
  if (slice >= slices) return;
  const int64_t unit = j % units;
  const int tid = threadIdx.x;
  const int c = 4 * (static_cast<int>(slice) * Q + tid % Q);
  const int64_t i = unit * (PIX * NPIX) + tid / Q;
  if (c >= a.C || i >= P) return;
  join_elements<NPIX>(a, i, PIX, P, c);
}

int check_shape(const char* fn, int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1 || C < 1) {
    set_error("%s: %s", fn, "B, H, W and C must be positive");
    return EPOS_E_INVALID;
  }
  if (C % 4 != 0) {
    set_error("%s: %s", fn, "C must be a multiple of 4");
    return EPOS_E_INVALID;
  }
  if (H > (1 << 30) || W > (1 << 30) || static_cast<int64_t>(B) * H * W > (int64_t{1} << 40)) {
    set_error("%s: %s", fn, "too many pixels");
    return EPOS_E_INVALID;
  }
  return EPOS_OK;
}

int check_pool(const char* fn, int B, int64_t P, int C) {
  if (B < 1 || P < 1 || C < 1) {
    set_error("%s: %s", fn, "B, P and C must be positive");
    return EPOS_E_INVALID;
  }
  if (C % 4 != 0) {
    set_error("%s: %s", fn, "C must be a multiple of 4");
    return EPOS_E_INVALID;
  }
  if (B > 65535 || P > (int64_t{1} << 40) || B * P > (int64_t{1} << 40)) {
    set_error("%s: %s", fn, "too many pixels");
    return EPOS_E_INVALID;
  }
  return EPOS_OK;
}

template <int Q, int NPIX>
int launch_slices(const EposAsppJoinArgs& a, int64_t P, hipStream_t s) {
  const int64_t slices = ceil_div(a.C / 4, Q);
  const int64_t units = ceil_div(P, NPIX * (AG_THREADS / Q));
  const int64_t blocks = round_up(slices, XCDS) * units;
  if (blocks > 0x7fffffff) {
    set_error("%s: %s", "epos_aspp_join_dgrad_f32", "too many blocks");
    return EPOS_E_INVALID;
  }
  hipLaunchKernelGGL((join_slice_kernel<Q, NPIX>), dim3(static_cast<unsigned>(blocks)), dim3(AG_THREADS),
                     0, s, a, P, static_cast<int>(slices), units);
  return launch_status("join_slice_kernel");
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_pool_broadcast_dgrad_range_pixels(int B, int64_t P, int C) {
  const int rc = check_pool(__func__, B, P, C);
  if (rc != EPOS_OK) return rc;
  return pool_range(P);
}

extern "C" int64_t epos_pool_broadcast_dgrad_workspace_bytes(int B, int64_t P, int C) {
  const int rc = check_pool(__func__, B, P, C);
  if (rc != EPOS_OK) return rc;
  const int64_t count = ceil_div(P, pool_range(P));
  return count <= 1 ? 0 : 8 * count * B * C;
}

extern "C" int epos_pool_broadcast_dgrad_f32(const float* D, int64_t ldd, float* g, int64_t ldg,
                                             int B, int64_t P, int C, void* workspace,
                                             void* stream) {
  const int rc0 = check_pool(__func__, B, P, C);
  if (rc0 != EPOS_OK) return rc0;
  EPOS_REQUIRE(ldd >= C && ldd % 4 == 0, "ldd must be >= C and a multiple of 4");
  EPOS_REQUIRE(ldg >= C && ldg % 4 == 0, "ldg must be >= C and a multiple of 4");
  EPOS_REQUIRE(D && g, "null pointer");
  EPOS_REQUIRE(al16(D) && al16(g), "D and g must be 16-byte aligned");
  EPOS_REQUIRE(static_cast<const void*>(g) != D, "g may not start at D");
  const int64_t range = pool_range(P);
  const int64_t count = ceil_div(P, range);
  EPOS_REQUIRE(count <= 1 || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
               "the workspace must be given, 8-byte aligned");
  const int quads = C / 4;
  const int q_wide = quads < POOL_QUADS ? quads : POOL_QUADS;
  const int slots = AG_THREADS / q_wide;
  const int64_t q_blocks = ceil_div(quads, q_wide);
  EPOS_REQUIRE(q_blocks <= 0x7fffffff && count <= 65535, "too many blocks");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* slabs = static_cast<double*>(workspace);
  hipLaunchKernelGGL(pool_sum_kernel,
                     dim3(static_cast<unsigned>(q_blocks), static_cast<unsigned>(count),
                          static_cast<unsigned>(B)),
                     dim3(AG_THREADS), 0, s, D, ldd, P, C, range, q_wide, slots,
                     count <= 1 ? g : nullptr, ldg, slabs);
  const int rc = launch_status("pool_sum_kernel");
  if (rc != EPOS_OK || count <= 1) return rc;
  const int64_t total = static_cast<int64_t>(B) * C;
  hipLaunchKernelGGL(pool_sum_close_kernel, dim3(blocks_for(total, AG_THREADS)), dim3(AG_THREADS),
                     0, s, slabs, count, C, total, g, ldg);
  return launch_status("pool_sum_close_kernel");
}

extern "C" int epos_aspp_join_dgrad_f32(const EposAsppJoinArgs* args, void* stream) {
  EPOS_REQUIRE(args, "null args");
  const EposAsppJoinArgs& a = *args;
  const int rc0 = check_shape(__func__, a.B, a.H, a.W, a.C);
  if (rc0 != EPOS_OK) return rc0;
  EPOS_REQUIRE(a.n_dw >= 0 && a.n_dw <= 4, "n_dw must be in 0..4");
  EPOS_REQUIRE(a.n_plain >= 0 && a.n_plain <= 2, "n_plain must be in 0..2");
  EPOS_REQUIRE(a.n_dw + a.n_plain > 0 || a.Pool, "at least one term must be present");
  EPOS_REQUIRE(a.dX, "null pointer");
  EPOS_REQUIRE(a.ldx >= a.C && a.ldx % 4 == 0, "ldx must be >= C and a multiple of 4");
  EPOS_REQUIRE(al16(a.dX), "every pointer must be 16-byte aligned");
  for (int t = 0; t < a.n_dw; ++t) {
    EPOS_REQUIRE(a.dw[t].D && a.dw[t].w9c, "null pointer");
    EPOS_REQUIRE(a.dw[t].rate >= 1 && a.dw[t].rate <= (1 << 20), "rate must be >= 1");
    EPOS_REQUIRE(a.dw[t].ldd >= a.C && a.dw[t].ldd % 4 == 0,
                 "ldd must be >= C and a multiple of 4");
    EPOS_REQUIRE(al16(a.dw[t].D) && al16(a.dw[t].w9c), "every pointer must be 16-byte aligned");
    EPOS_REQUIRE(a.dX != a.dw[t].D, "dX may not start at an input");
  }
  for (int j = 0; j < a.n_plain; ++j) {
    EPOS_REQUIRE(a.plain[j].E, "null pointer");
    EPOS_REQUIRE(a.plain[j].lde >= a.C && a.plain[j].lde % 4 == 0,
                 "lde must be >= C and a multiple of 4");
    EPOS_REQUIRE(al16(a.plain[j].E), "every pointer must be 16-byte aligned");
    EPOS_REQUIRE(a.dX != a.plain[j].E, "dX may not start at an input");
  }
  if (a.Pool) {
    EPOS_REQUIRE(a.ldp >= a.C && a.ldp % 4 == 0, "ldp must be >= C and a multiple of 4");
    EPOS_REQUIRE(a.pool_div >= 1, "pool_div must be >= 1");
    EPOS_REQUIRE(al16(a.Pool), "every pointer must be 16-byte aligned");
    EPOS_REQUIRE(a.dX != a.Pool, "dX may not start at an input");
  }
  if (a.Y) {
    EPOS_REQUIRE(a.ldy >= a.C && a.ldy % 4 == 0, "ldy must be >= C and a multiple of 4");
    EPOS_REQUIRE(al16(a.Y), "every pointer must be 16-byte aligned");
    EPOS_REQUIRE(a.dX != a.Y, "dX may not start at an input");
  }
  EPOS_REQUIRE(a.partition >= 0 && a.partition <= EPOS_ASPP_JOIN_SLICE32X4,
               "unknown partition");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t P = static_cast<int64_t>(a.B) * a.H * a.W;
  const int partition = a.partition == 0 ? EPOS_ASPP_JOIN_SHIPPED : a.partition;
  if (partition == EPOS_ASPP_JOIN_SLICE32) return launch_slices<8, 1>(a, P, s);
  if (partition == EPOS_ASPP_JOIN_SLICE64) return launch_slices<16, 1>(a, P, s);
  if (partition == EPOS_ASPP_JOIN_SLICE32X2) return launch_slices<8, 2>(a, P, s);
  if (partition == EPOS_ASPP_JOIN_SLICE32X4) return launch_slices<8, 4>(a, P, s);
  const int64_t total = P * (a.C / 4);
  const int64_t blocks = ceil_div(total, AG_THREADS);
  EPOS_REQUIRE(blocks <= 0x7fffffff, "too many blocks");
  hipLaunchKernelGGL(join_pixel_kernel, dim3(static_cast<unsigned>(blocks)), dim3(AG_THREADS), 0,
                     s, a, total, P);
  return launch_status("join_pixel_kernel");
}
