// The backward pass of a 3x3 depthwise layer with a frozen batch norm, stride 1, TF 'SAME'
// padding (include/epos_hip.h, "Depthwise gradients"; DESIGN.md, "Losses", "Backward through
// decoder_conv1").
//
//   dw_wgrad_kernel      T[tap,c] = sum X(tap) D and t[c] = sum D over ONE range of pixels. A
//                        thread owns four consecutive channels and every PS-th pixel of the range
//                        (PS = 256 / min(C / 4, 16) pixel slots a workgroup, which owns at most
//                        64 channels): ten fp64 sums per channel in registers, the products
//                        exact. The slots' sums are then added in slot order through LDS.
//   dw_wgrad_sum_kernel  with more than one range: adds the ranges' slabs in range order.
//   dw_dgrad_kernel      dX = the nine taps of D, mirrored, times the folded weights: a thread
//                        owns four channels of one pixel, one fp64 accumulator each, the taps in
//                        ascending order, rounded once; the ReLU mask of the layer below.
//
// The checkpoint-shaped gradients come from epos_pointwise_wgrad_close_f32 with K = 9: there is
// no closing kernel here. No atomics: the same bytes in every run. -ffp-contract=off.
#include "common.h"

namespace epos {
namespace {

constexpr int DW_THREADS = 256;
constexpr int64_t DW_MIN_RANGE = 64;          // pixels: below that a slab costs more than it saves
constexpr int64_t DW_TARGET = 1024;           // workgroups to aim for: four per compute unit
constexpr int DW_QUADS = 16;                  // channel quads a workgroup owns at most

// A function of (B, H, W, C) only: the cut decides the order of the sums
int64_t range_for(int64_t P, int C) {
  const int64_t q_blocks = ceil_div(C / 4, DW_QUADS);
  int64_t want = DW_TARGET / q_blocks;
  if (want < 1) want = 1;
  int64_t r = ceil_div(P, want);
  return r < DW_MIN_RANGE ? DW_MIN_RANGE : r;
}

// a += x * d for a tap that is there; one that is not adds +0.0, which changes no byte of a sum
// that started from +0.0 -- not 0 * d, which a non-finite d would turn into a NaN
__device__ __forceinline__ void add4_if(double (&a)[4], float4 x, float4 d, bool ok) {
  const double p0 = static_cast<double>(x.x) * static_cast<double>(d.x);
  const double p1 = static_cast<double>(x.y) * static_cast<double>(d.y);
  const double p2 = static_cast<double>(x.z) * static_cast<double>(d.z);
  const double p3 = static_cast<double>(x.w) * static_cast<double>(d.w);
  a[0] += ok ? p0 : 0.0;
  a[1] += ok ? p1 : 0.0;
  a[2] += ok ? p2 : 0.0;
  a[3] += ok ? p3 : 0.0;
}

__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ D, int64_t ldd, int H,
    int W, int C, int rate, int64_t P, int64_t range, int q_wide, int slots,
    double* __restrict__ T_out, double* __restrict__ t_out, int64_t slab_stride) {
  __shared__ double part[DW_THREADS][4];
  const int tid = threadIdx.x;
  const int qi = tid % q_wide, slot = tid / q_wide;
  const int c = 4 * (blockIdx.x * q_wide + qi);
  const bool active = slot < slots && c < C;
  const int64_t i0 = static_cast<int64_t>(blockIdx.y) * range;
  const int64_t i1 = i0 + range < P ? i0 + range : P;

  double acc[10][4];
#pragma unroll
  for (int v = 0; v < 10; ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[v][e] = 0.0;

  if (active && i0 + slot < i1) {
    // (x, y) of the slot's first pixel, then stepped along: no 64-bit division per pixel
    int x = static_cast<int>((i0 + slot) % W);
    int y = static_cast<int>((i0 + slot) / W % H);
    for (int64_t i = i0 + slot; i < i1; i += slots) {
      const float4 d = *reinterpret_cast<const float4*>(D + i * ldd + c);
      // every tap is loaded, one in the padding from the pixel itself, and then not added:
      // loads under a branch would be waited for one by one
      float4 xv[9];
      bool ok[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + (ky - 1) * rate;
        const bool oky = yy >= 0 && yy < H;   // the same image: a tap never leaves it
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = x + (kx - 1) * rate;
          const int tap = 3 * ky + kx;
          ok[tap] = oky && xx >= 0 && xx < W;
          const int64_t at =
              ok[tap] ? i + static_cast<int64_t>((ky - 1) * rate) * W + (kx - 1) * rate : i;
          xv[tap] = *reinterpret_cast<const float4*>(X + at * ldx + c);
        }
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) add4_if(acc[tap], xv[tap], d, ok[tap]);
      acc[9][0] += static_cast<double>(d.x);
      acc[9][1] += static_cast<double>(d.y);
      acc[9][2] += static_cast<double>(d.z);
      acc[9][3] += static_cast<double>(d.w);
      x += slots;
      if (x >= W) {
        const int rows = x / W;
        x -= rows * W;
        y = (y + rows) % H;
      }
    }
  }

  double* T_slab = T_out + blockIdx.y * slab_stride;
  double* t_slab = t_out + blockIdx.y * slab_stride;
  for (int v = 0; v < 10; ++v) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) part[tid][e] = acc[v][e];
    __syncthreads();
    if (active && slot == 0) {
      double* dst = v < 9 ? T_slab + static_cast<int64_t>(v) * C + c : t_slab + c;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double s = 0.0;
        for (int k = 0; k < slots; ++k) s += part[k * q_wide + qi][e];
        dst[e] = s;
      }
    }
  }
}

// T and t = the sum of the ranges' slabs [9 * C | C], in range order, from +0.0
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_sum_kernel(
    const double* __restrict__ slabs, int64_t slab_stride, int64_t count, int64_t tc, int64_t c,
    double* __restrict__ T, double* __restrict__ t) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * DW_THREADS + threadIdx.x;
  if (i >= tc + c) return;
  const double* src = slabs + i;
  double s = 0.0;
  int64_t r = 0;
  for (; r + 16 <= count; r += 16) {          // sixteen loads in flight, added in range order
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = src[(r + u) * slab_stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; r < count; ++r) s += src[r * slab_stride];
  if (i < tc) T[i] = s;
  else t[i - tc] = s;
}

__global__ __launch_bounds__(DW_THREADS) void dw_dgrad_kernel(
    const float* __restrict__ D, int64_t ldd, const float* __restrict__ w9c,
    const float* __restrict__ Y, int64_t ldy, float* __restrict__ dX, int64_t ldx, int H, int W,
    int C, int rate, int64_t total) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * DW_THREADS + threadIdx.x;
  if (g >= total) return;
  const int quads = C / 4;
  const int c = 4 * static_cast<int>(g % quads);
  const int64_t i = g / quads;
  const int x = static_cast<int>(i % W);
  const int y = static_cast<int>(i / W % H);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  // as in dw_wgrad_kernel: every tap loaded, one outside the image from the pixel itself and not
  // added (+0.0 changes no byte of the sum)
  float4 dv[9];
  bool ok[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = y - (ky - 1) * rate;
    const bool oky = yy >= 0 && yy < H;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = x - (kx - 1) * rate;
      const int tap = 3 * ky + kx;
      ok[tap] = oky && xx >= 0 && xx < W;
      const int64_t at =
          ok[tap] ? i - static_cast<int64_t>((ky - 1) * rate) * W - (kx - 1) * rate : i;
      dv[tap] = *reinterpret_cast<const float4*>(D + at * ldd + c);
    }
  }
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
    add4_if(acc, *reinterpret_cast<const float4*>(w9c + static_cast<int64_t>(tap) * C + c),
            dv[tap], ok[tap]);
  float4 v = make_float4(static_cast<float>(acc[0]), static_cast<float>(acc[1]),
                         static_cast<float>(acc[2]), static_cast<float>(acc[3]));
  if (Y != nullptr) {
    const float4 m = *reinterpret_cast<const float4*>(Y + i * ldy + c);
    v.x = m.x <= 0.f ? 0.f : v.x;
    v.y = m.y <= 0.f ? 0.f : v.y;
    v.z = m.z <= 0.f ? 0.f : v.z;
    v.w = m.w <= 0.f ? 0.f : v.w;
  }
  *reinterpret_cast<float4*>(dX + i * ldx + c) = v;
}

bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

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

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_depthwise_wgrad_range_pixels(int B, int H, int W, int C) {
  const int rc = check_shape(__func__, B, H, W, C);
  if (rc != EPOS_OK) return rc;
  return range_for(static_cast<int64_t>(B) * H * W, C);
}

extern "C" int64_t epos_depthwise_wgrad_workspace_bytes(int B, int H, int W, int C) {
  const int rc = check_shape(__func__, B, H, W, C);
  if (rc != EPOS_OK) return rc;
  const int64_t P = static_cast<int64_t>(B) * H * W;
  const int64_t count = ceil_div(P, range_for(P, C));
  return count <= 1 ? 0 : count * 8 * 10 * static_cast<int64_t>(C);
}

extern "C" int epos_depthwise_wgrad_f32(const EposDepthwiseWgradArgs* args, void* stream) {
  EPOS_REQUIRE(args, "null args");
  const EposDepthwiseWgradArgs& a = *args;
  const int rc0 = check_shape(__func__, a.B, a.H, a.W, a.C);
  if (rc0 != EPOS_OK) return rc0;
  EPOS_REQUIRE(a.stride == 1, "stride must be 1");
  EPOS_REQUIRE(a.rate >= 1 && a.rate <= (1 << 20), "rate must be >= 1");
  EPOS_REQUIRE(a.ldx >= a.C && a.ldx % 4 == 0, "ldx must be >= C and a multiple of 4");
  EPOS_REQUIRE(a.ldd >= a.C && a.ldd % 4 == 0, "ldd must be >= C and a multiple of 4");
  EPOS_REQUIRE(a.X && a.D && a.T && a.t, "null pointer");
  EPOS_REQUIRE(al16(a.X) && al16(a.D) && al(a.T, 8) && al(a.t, 8),
               "X and D must be 16-byte aligned, T and t 8-byte aligned");
  const int64_t P = static_cast<int64_t>(a.B) * a.H * a.W;
  const int64_t range = range_for(P, a.C);
  const int64_t count = ceil_div(P, range);
  EPOS_REQUIRE(count <= 1 || (a.workspace && al(a.workspace, 8)),
               "the workspace must be given, 8-byte aligned");
  const int quads = a.C / 4;
  const int q_wide = quads < DW_QUADS ? quads : DW_QUADS;
  const int slots = DW_THREADS / q_wide;
  const int64_t q_blocks = ceil_div(quads, q_wide);
  EPOS_REQUIRE(count <= 65535 && q_blocks <= 0x7fffffff, "too many blocks");
  const int64_t tc = 9 * static_cast<int64_t>(a.C);
  double* T_out = a.T;
  double* t_out = a.t;
  int64_t stride = 0;
  if (count > 1) {
    T_out = static_cast<double*>(a.workspace);
    t_out = T_out + tc;
    stride = tc + a.C;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dw_wgrad_kernel,
                     dim3(static_cast<unsigned>(q_blocks), static_cast<unsigned>(count)),
                     dim3(DW_THREADS), 0, s, a.X, a.ldx, a.D, a.ldd, a.H, a.W, a.C, a.rate, P,
                     range, q_wide, slots, T_out, t_out, stride);
  const int rc = launch_status("dw_wgrad_kernel");
  if (rc != EPOS_OK || count <= 1) return rc;
  hipLaunchKernelGGL(dw_wgrad_sum_kernel, dim3(blocks_for(tc + a.C, DW_THREADS)),
                     dim3(DW_THREADS), 0, s, static_cast<const double*>(a.workspace), stride,
                     count, tc, static_cast<int64_t>(a.C), a.T, a.t);
  return launch_status("dw_wgrad_sum_kernel");
}

extern "C" int epos_depthwise_dgrad_f32(const float* D, int64_t ldd, const float* w9c,
                                        const float* Y, int64_t ldy, float* dX, int64_t ldx,
                                        int B, int H, int W, int C, int rate, void* stream) {
  const int rc0 = check_shape(__func__, B, H, W, C);
  if (rc0 != EPOS_OK) return rc0;
  EPOS_REQUIRE(rate >= 1 && rate <= (1 << 20), "rate must be >= 1");
  EPOS_REQUIRE(ldd >= C && ldd % 4 == 0, "ldd must be >= C and a multiple of 4");
  EPOS_REQUIRE(ldx >= C && ldx % 4 == 0, "ldx must be >= C and a multiple of 4");
  EPOS_REQUIRE(D && w9c && dX, "null pointer");
  EPOS_REQUIRE(!Y || (ldy >= C && ldy % 4 == 0), "ldy must be >= C and a multiple of 4");
  EPOS_REQUIRE(al16(D) && al16(w9c) && al16(Y) && al16(dX),
               "D, w9c, Y and dX must be 16-byte aligned");
  EPOS_REQUIRE(dX != D, "dX may not start at D");
  const int64_t total = static_cast<int64_t>(B) * H * W * (C / 4);
  const int64_t blocks = ceil_div(total, DW_THREADS);
  EPOS_REQUIRE(blocks <= 0x7fffffff, "too many blocks");
  hipLaunchKernelGGL(dw_dgrad_kernel, dim3(static_cast<unsigned>(blocks)), dim3(DW_THREADS), 0,
                     static_cast<hipStream_t>(stream), D, ldd, w9c, Y, ldy, dX, ldx, H, W, C, rate,
                     total);
  return launch_status("dw_dgrad_kernel");
}
