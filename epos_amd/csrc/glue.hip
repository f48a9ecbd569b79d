// Glue layers of the network, NHWC, fp32 and the bf16 mode from one template each: bilinear
// resize (align_corners), 3x3 stride-2 'SAME' max pool (net_resnet_v1_beta.py:190), spatial
// subsampling (slim resnet_utils.subsample, the identity shortcut of a strided unit) and the
// ResNet unit's final relu(a + b). One thread = one channel pack (nhwc.h) of one output pixel:
// 4 channels in fp32, 8 in bf16, 16 bytes either way; consecutive threads walk the channel
// axis first (coalesced), then pixels; 256 threads per workgroup.
#include "nhwc.h"

namespace epos {
namespace {

// SP = source pack, DP = destination pack (same channel count): fp32 -> fp32, bf16 -> bf16, and
// fp32 -> bf16 (the bf16 mode resizes the fp32 image-pooling branch). The arithmetic is fp32
// in all three (bilinear_sample), then one rounding per stored bf16 value.
template <class SP, class DP>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(
    const typename SP::elem* X, int64_t ldx, typename DP::elem* Y, int64_t ldy, int Hi, int Wi,
    int Ho, int Wo, int cn, float sy, float sx, int64_t total) {
  static_assert(SP::n == DP::n, "one thread reads the channels it writes");
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const Pixel p = decode_pixel<DP::n>(id, cn, Ho, Wo);
  const BilinearSrc<typename SP::elem> src = {X, ldx, Hi, Wi, sy, sx};
  float o[DP::n];
  bilinear_sample<SP>(src, p.b, p.yo, p.xo, p.c, o);
  DP::store(Y + pixel_offset(p, Ho, Wo, ldy), o);
}

template <class P>
__global__ __launch_bounds__(256) void maxpool3x3_s2_kernel(
    const typename P::elem* X, int64_t ldx, typename P::elem* Y, int64_t ldy, int Hi, int Wi,
    int Ho, int Wo, int cn, int pad_y, int pad_x, int64_t total) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const Pixel p = decode_pixel<P::n>(id, cn, Ho, Wo);
  const typename P::elem* xb = X + static_cast<int64_t>(p.b) * Hi * Wi * ldx + p.c;
  float m[P::n];
#pragma unroll
  for (int e = 0; e < P::n; ++e) m[e] = -INFINITY;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yi = p.yo * 2 - pad_y + ky;
    if (yi < 0 || yi >= Hi) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xi = p.xo * 2 - pad_x + kx;
      if (xi < 0 || xi >= Wi) continue;
      float v[P::n];
      P::load(xb + (static_cast<int64_t>(yi) * Wi + xi) * ldx, v);
#pragma unroll
      for (int e = 0; e < P::n; ++e) m[e] = fmaxf(m[e], v[e]);
    }
  }
  P::store(Y + pixel_offset(p, Ho, Wo, ldy), m);   // a maximum of bf16 values: exact
}

template <class P>
__global__ __launch_bounds__(256) void subsample_kernel(
    const typename P::elem* X, int64_t ldx, typename P::elem* Y, int64_t ldy, int Hi, int Wi,
    int Ho, int Wo, int cn, int factor, int64_t total) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const Pixel p = decode_pixel<P::n>(id, cn, Ho, Wo);
  using vec = typename P::vec;                     // a copy of the pack's bits
  *reinterpret_cast<vec*>(Y + pixel_offset(p, Ho, Wo, ldy)) = *reinterpret_cast<const vec*>(
      X + ((static_cast<int64_t>(p.b) * Hi + p.yo * factor) * Wi + p.xo * factor) * ldx + p.c);
}

template <class P>
__global__ __launch_bounds__(256) void add_relu_kernel(const typename P::elem* A,
                                                       const typename P::elem* B,
                                                       typename P::elem* Y, int64_t packs) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= packs) return;
  float a[P::n], b[P::n];
  P::load(A + P::n * i, a);
  P::load(B + P::n * i, b);
#pragma unroll
  for (int e = 0; e < P::n; ++e) a[e] = fmaxf(a[e] + b[e], 0.f);
  P::store(Y + P::n * i, a);
}

// What every map launcher refuses, under the name `fn` of its entry point: N = channels per
// thread; need_al0, need_al1 = the pointers that must be 16-byte aligned (the bf16 entries ask
// it of their bf16 tensors, the fp32 entries of none).
int check_maps(const char* fn, const void* X, int64_t ldx, const void* Y, int64_t ldy, int B,
               int Hi, int Wi, int C, int N, const void* need_al0 = nullptr,
               const void* need_al1 = nullptr) {
  const char* msg = nullptr;
  if (!X || !Y) msg = "null pointer";
  else if (C % N || ldx % N || ldy % N) msg = "C, ldx, ldy must be multiples of 4 (bf16: 8)";
  else if (!al16(need_al0) || !al16(need_al1)) msg = "bf16 tensors must be 16-byte aligned";
  else if (B < 1 || Hi < 1 || Wi < 1 || C < 1) msg = "empty map";
  else if (ldx < C || ldy < C) msg = "ldx, ldy >= C";
  if (!msg) return EPOS_OK;
  set_error("%s: %s", fn, msg);
  return EPOS_E_INVALID;
}

// TF 'SAME' for a window of 3 at stride 2: out = ceil(in / 2); the padding in front is half of
// what the windows overhang, rounded down (the odd one goes behind).
struct Same { int out, pad; };
Same same_3x3_s2(int in) {
  const int out = (in + 1) / 2, t = (out - 1) * 2 + 3 - in;
  return {out, t > 0 ? t / 2 : 0};
}

template <class SP, class DP>
int resize(const typename SP::elem* X, int64_t ldx, typename DP::elem* Y, int64_t ldy, int B,
           int Hi, int Wi, int Ho, int Wo, int C, void* stream) {
  const int cn = C / DP::n;
  const int64_t total = static_cast<int64_t>(B) * Ho * Wo * cn;
  hipLaunchKernelGGL((resize_bilinear_kernel<SP, DP>), dim3(blocks_for(total, 256)), dim3(256),
                     0, static_cast<hipStream_t>(stream), X, ldx, Y, ldy, Hi, Wi, Ho, Wo, cn,
                     align_corners_scale(Hi, Ho), align_corners_scale(Wi, Wo), total);
  return launch_status("resize_bilinear_kernel");
}

template <class P>
int maxpool(const typename P::elem* X, int64_t ldx, typename P::elem* Y, int64_t ldy, int B,
            int Hi, int Wi, int C, void* stream) {
  const Same y = same_3x3_s2(Hi), x = same_3x3_s2(Wi);
  const int cn = C / P::n;
  const int64_t total = static_cast<int64_t>(B) * y.out * x.out * cn;
  hipLaunchKernelGGL(maxpool3x3_s2_kernel<P>, dim3(blocks_for(total, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), X, ldx, Y, ldy, Hi, Wi, y.out, x.out, cn,
                     y.pad, x.pad, total);
  return launch_status("maxpool3x3_s2_kernel");
}

template <class P>
int subsample(const typename P::elem* X, int64_t ldx, typename P::elem* Y, int64_t ldy, int B,
              int Hi, int Wi, int C, int factor, void* stream) {
  const int Ho = (Hi - 1) / factor + 1, Wo = (Wi - 1) / factor + 1;
  const int cn = C / P::n;
  const int64_t total = static_cast<int64_t>(B) * Ho * Wo * cn;
  hipLaunchKernelGGL(subsample_kernel<P>, dim3(blocks_for(total, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), X, ldx, Y, ldy, Hi, Wi, Ho, Wo, cn,
                     factor, total);
  return launch_status("subsample_kernel");
}

template <class P>
int add_relu(const char* fn, const typename P::elem* A, const typename P::elem* B,
             typename P::elem* Y, int64_t n, bool need_al, void* stream) {
  const char* msg = nullptr;
  if (!A || !B || !Y) msg = "null pointer";
  else if (n < 0 || n % P::n) msg = "n must be a multiple of 4 (bf16: 8)";
  else if (need_al && !(al16(A) && al16(B) && al16(Y))) msg = "16-byte aligned";
  if (msg) {
    set_error("%s: %s", fn, msg);
    return EPOS_E_INVALID;
  }
  if (n == 0) return EPOS_OK;
  hipLaunchKernelGGL(add_relu_kernel<P>, dim3(blocks_for(n / P::n, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), A, B, Y, n / P::n);
  return launch_status("add_relu_kernel");
}

using F32 = F32Pack<4>;

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_resize_bilinear_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int B,
                                        int Hi, int Wi, int Ho, int Wo, int C, void* stream) {
  EPOS_REQUIRE(Ho >= 1 && Wo >= 1, "empty map");
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 4)) return rc;
  return resize<F32, F32>(X, ldx, Y, ldy, B, Hi, Wi, Ho, Wo, C, stream);
}

// x_f32: X holds fp32 (read by scalar loads, so only Y and a bf16 X need the alignment)
extern "C" int epos_resize_bilinear_bf16(const void* X, int64_t ldx, int x_f32, uint16_t* Y,
                                         int64_t ldy, int B, int Hi, int Wi, int Ho, int Wo,
                                         int C, void* stream) {
  EPOS_REQUIRE(Ho >= 1 && Wo >= 1, "empty map");
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 8, Y, x_f32 ? nullptr : X))
    return rc;
  if (x_f32)
    return resize<F32ScalarPack, Bf16Pack>(static_cast<const float*>(X), ldx, Y, ldy, B, Hi, Wi,
                                           Ho, Wo, C, stream);
  return resize<Bf16Pack, Bf16Pack>(static_cast<const uint16_t*>(X), ldx, Y, ldy, B, Hi, Wi, Ho,
                                    Wo, C, stream);
}

extern "C" int epos_maxpool3x3_s2_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int B,
                                      int Hi, int Wi, int C, void* stream) {
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 4)) return rc;
  return maxpool<F32>(X, ldx, Y, ldy, B, Hi, Wi, C, stream);
}

extern "C" int epos_maxpool3x3_s2_bf16(const uint16_t* X, int64_t ldx, uint16_t* Y,
                                       int64_t ldy, int B, int Hi, int Wi, int C, void* stream) {
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 8, X, Y)) return rc;
  return maxpool<Bf16Pack>(X, ldx, Y, ldy, B, Hi, Wi, C, stream);
}

extern "C" int epos_subsample_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int B,
                                  int Hi, int Wi, int C, int factor, void* stream) {
  EPOS_REQUIRE(factor >= 1, "factor >= 1");
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 4)) return rc;
  return subsample<F32>(X, ldx, Y, ldy, B, Hi, Wi, C, factor, stream);
}

extern "C" int epos_subsample_bf16(const uint16_t* X, int64_t ldx, uint16_t* Y, int64_t ldy,
                                   int B, int Hi, int Wi, int C, int factor, void* stream) {
  EPOS_REQUIRE(factor >= 1, "factor >= 1");
  if (int rc = check_maps(__func__, X, ldx, Y, ldy, B, Hi, Wi, C, 8, X, Y)) return rc;
  return subsample<Bf16Pack>(X, ldx, Y, ldy, B, Hi, Wi, C, factor, stream);
}

extern "C" int epos_add_relu_f32(const float* A, const float* B, float* Y, int64_t n,
                                 void* stream) {
  return add_relu<F32>(__func__, A, B, Y, n, false, stream);
}

extern "C" int epos_add_relu_bf16(const uint16_t* A, const uint16_t* B, uint16_t* Y, int64_t n,
                                  void* stream) {
  return add_relu<Bf16Pack>(__func__, A, B, Y, n, true, stream);
}
