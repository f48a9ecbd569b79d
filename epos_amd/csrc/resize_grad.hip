// The adjoint of the align-corners bilinear resize (include/epos_hip.h, "Resize input gradient";
// DESIGN.md, "Losses", "Backward through the decoder"): the gradient that crosses
// decoder/resize, from the decoder's size down to the encoder's.
//
//   resize_dgrad_kernel  gather form: a thread owns four channels of ONE SOURCE pixel and adds,
//                        in fp64 from +0.0, the output pixels whose taps name that pixel, rows
//                        ascending and columns ascending within a row, each weighted by
//                        wy(yo, yi) wx(xo, xi); rounded to fp32 once; the ReLU mask of the layer
//                        that produced the source.
//
// Which output pixels those are is asked of the forward's own fp32 expressions (bilinear_sample,
// nhwc.h): o -> min(floor(o s), in - 1) and o -> min(ceil(o s), in - 1) do not decrease with o, so
// the outputs of a source index are one interval, found by two binary searches over those very
// expressions -- no division by s, whose rounding would disagree with the forward where fp32
// moved a sample into the neighbouring cell. No atomics, no workspace: the same bytes in every
// run. -ffp-contract=off.
#include "common.h"

namespace epos {
namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_BATCH = 4;            // loads of one output row in flight before they are added

struct Axis {                          // one axis of the forward: in -> out, align_corners
  int in, out;
  float s;
};

// the forward's taps and weight of output index o (bilinear_sample)
__device__ __forceinline__ int tap0(const Axis& a, int o) {
  return min(static_cast<int>(floorf(static_cast<float>(o) * a.s)), a.in - 1);
}
__device__ __forceinline__ int tap1(const Axis& a, int o) {
  return min(static_cast<int>(ceilf(static_cast<float>(o) * a.s)), a.in - 1);
}

// the weight of source index i on output index o, in fp64 from the forward's fp32 fraction:
// [i0 == i](1 - l) + [i1 == i] l, exactly 1 where both taps name i
__device__ __forceinline__ double weight(const Axis& a, int o, int i) {
  const float f = static_cast<float>(o) * a.s;
  const int i0 = min(static_cast<int>(floorf(f)), a.in - 1);
  const int i1 = min(static_cast<int>(ceilf(f)), a.in - 1);
  const double l = static_cast<double>(f - static_cast<float>(i0));
  if (i0 == i1) return i0 == i ? 1.0 : 0.0;
  return i0 == i ? 1.0 - l : (i1 == i ? l : 0.0);
}

// [lo, hi]: the output indices with tap0 == i or tap1 == i (empty: lo > hi). tap1 - tap0 <= 1, so
// every o with tap1(o) >= i and tap0(o) <= i has one of them equal to i.
__device__ __forceinline__ void footprint(const Axis& a, int i, int* lo_out, int* hi_out) {
  int lo = 0, hi = a.out;              // the first o with tap1(o) >= i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tap1(a, mid) >= i) hi = mid;
    else lo = mid + 1;
  }
  *lo_out = lo;
  hi = a.out;                          // the first o with tap0(o) > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tap0(a, mid) > i) hi = mid;
    else lo = mid + 1;
  }
  *hi_out = lo - 1;
}

__device__ __forceinline__ void add_if(double (&acc)[4], double w, float4 d, bool ok) {
  // a slot past the footprint adds +0.0, which changes no byte of a sum that started from +0.0
  // -- not 0 * d, which a non-finite d would turn into a NaN
  const double p0 = w * static_cast<double>(d.x);
  const double p1 = w * static_cast<double>(d.y);
  const double p2 = w * static_cast<double>(d.z);
  const double p3 = w * static_cast<double>(d.w);
  acc[0] += ok ? p0 : 0.0;
  acc[1] += ok ? p1 : 0.0;
  acc[2] += ok ? p2 : 0.0;
  acc[3] += ok ? p3 : 0.0;
}

__global__ __launch_bounds__(RG_THREADS) void resize_dgrad_kernel(
    const float* __restrict__ D, int64_t ldd, const float* __restrict__ Y, int64_t ldy,
    float* __restrict__ dX, int64_t ldx, Axis ay, Axis ax, int C, int64_t total) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * RG_THREADS + threadIdx.x;
  if (g >= total) return;
  const int quads = C / 4;
  const int c = 4 * static_cast<int>(g % quads);
  const int64_t i = g / quads;                         // the source pixel, (b, yi, xi) order
  const int xi = static_cast<int>(i % ax.in);
  const int yi = static_cast<int>(i / ax.in % ay.in);
  const int64_t b = i / ax.in / ay.in;
  int ylo, yhi, xlo, xhi;
  footprint(ay, yi, &ylo, &yhi);
  footprint(ax, xi, &xlo, &xhi);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (xlo <= xhi) {
    for (int yo = ylo; yo <= yhi; ++yo) {
      const double wy = weight(ay, yo, yi);
      const float* row = D + (b * ay.out + yo) * ax.out * ldd + c;
      for (int x0 = xlo; x0 <= xhi; x0 += RG_BATCH) {
        // RG_BATCH loads in flight, one past the footprint from its last pixel and not added
        float4 d[RG_BATCH];
        double w[RG_BATCH];
        bool ok[RG_BATCH];
#pragma unroll
        for (int u = 0; u < RG_BATCH; ++u) {
          ok[u] = x0 + u <= xhi;
          const int xo = ok[u] ? x0 + u : xhi;
          d[u] = *reinterpret_cast<const float4*>(row + static_cast<int64_t>(xo) * ldd);
          w[u] = wy * weight(ax, xo, xi);
        }
#pragma unroll
        for (int u = 0; u < RG_BATCH; ++u) add_if(acc, w[u], d[u], ok[u]);
      }
    }
  }
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

// scale = (in - 1) / (out - 1) as a float, 0 for out == 1: align_corners_scale of nhwc.h
float scale_of(int in, int out) {
  return out > 1 ? static_cast<float>(in - 1) / static_cast<float>(out - 1) : 0.f;
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_resize_bilinear_dgrad_f32(const float* D, int64_t ldd, const float* Y,
                                              int64_t ldy, float* dX, int64_t ldx, int B, int Hi,
                                              int Wi, int Ho, int Wo, int C, void* stream) {
  EPOS_REQUIRE(B >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 && C >= 1,
               "B, Hi, Wi, Ho, Wo and C must be positive");
  EPOS_REQUIRE(C % 4 == 0, "C must be a multiple of 4");
  // below 2^22 every index and every tap is an exact float
  EPOS_REQUIRE(Hi <= (1 << 22) && Wi <= (1 << 22) && Ho <= (1 << 22) && Wo <= (1 << 22) &&
                   static_cast<int64_t>(B) * Hi * Wi <= (int64_t{1} << 40) &&
                   static_cast<int64_t>(B) * Ho * Wo <= (int64_t{1} << 40),
               "too many pixels");
  EPOS_REQUIRE((Hi > 1 || Ho == 1) && (Wi > 1 || Wo == 1),
               "a source of one row or column broadcasts: its adjoint is a sum, not this entry");
  EPOS_REQUIRE(ldd >= C && ldd % 4 == 0, "ldd must be >= C and a multiple of 4");
  EPOS_REQUIRE(ldx >= C && ldx % 4 == 0, "ldx must be >= C and a multiple of 4");
  EPOS_REQUIRE(D && dX, "null pointer");
  EPOS_REQUIRE(!Y || (ldy >= C && ldy % 4 == 0), "ldy must be >= C and a multiple of 4");
  EPOS_REQUIRE(al16(D) && al16(Y) && al16(dX), "D, Y and dX must be 16-byte aligned");
  EPOS_REQUIRE(dX != D, "dX may not start at D");
  EPOS_REQUIRE(dX != Y, "dX may not start at Y");
  const int64_t total = static_cast<int64_t>(B) * Hi * Wi * (C / 4);
  const int64_t blocks = ceil_div(total, RG_THREADS);
  EPOS_REQUIRE(blocks <= 0x7fffffff, "too many blocks");
  const Axis ay = {Hi, Ho, scale_of(Hi, Ho)};
  const Axis ax = {Wi, Wo, scale_of(Wi, Wo)};
  hipLaunchKernelGGL(resize_dgrad_kernel, dim3(static_cast<unsigned>(blocks)), dim3(RG_THREADS),
                     0, static_cast<hipStream_t>(stream), D, ldd, Y, ldy, dX, ldx, ay, ax, C,
                     total);
  return launch_status("resize_dgrad_kernel");
}
