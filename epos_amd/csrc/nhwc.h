// NHWC channel packs: what one thread moves along the channel axis (the contiguous axis of
// NHWC) -- 16 bytes where pitch and base allow it, so a wave moves 1 KiB per instruction -- with
// the pixel decode and the bilinear sampler that the glue kernels (glue.hip), the multi-scale
// merge (resize_merge.hip) and the layer kernels of layers.hip and bf16.hip share.
#pragma once
#include "common.h"

namespace epos {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- fp32 x 4 as a float4 value (kernels that compute on float4) -------------------------
__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void st4(float* p, float4 v) {
  *reinterpret_cast<float4*>(p) = v;
}

// ---- bf16: round to nearest even, a NaN stays a (quiet) NaN ------------------------------
__host__ __device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}
__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return static_cast<uint32_t>(f2bf(a)) | (static_cast<uint32_t>(f2bf(b)) << 16);
}
// 8 bf16 (16 bytes) <-> 8 floats
__device__ __forceinline__ void ld8(const uint16_t* p, float* v) {
  const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(q[i] << 16);
    v[2 * i + 1] = __uint_as_float(q[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void st8(uint16_t* p, const float* v) {
  u32x4 q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pack2(v[2 * i], v[2 * i + 1]);
  *reinterpret_cast<u32x4*>(p) = q;
}

// ---- packs: n channels of element type elem <-> float[n]; vec = the pack as one access ----
template <int V> struct F32Vec;
template <> struct F32Vec<1> { using T = float; };
template <> struct F32Vec<2> { using T = float2; };
template <> struct F32Vec<4> { using T = float4; };

template <int V>                       // V = 4, 2 or 1 floats in one load / store
struct F32Pack {
  using elem = float;
  using vec = typename F32Vec<V>::T;
  static constexpr int n = V;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const vec t = *reinterpret_cast<const vec*>(p);
    const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = f[i];
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    vec t;
    float* f = reinterpret_cast<float*>(&t);
#pragma unroll
    for (int i = 0; i < V; ++i) f[i] = v[i];
    *reinterpret_cast<vec*>(p) = t;
  }
};

struct Bf16Pack {                      // 8 bf16 in one 16-byte access
  using elem = uint16_t;
  using vec = u32x4;
  static constexpr int n = 8;
  static __device__ __forceinline__ void load(const uint16_t* p, float* v) { ld8(p, v); }
  static __device__ __forceinline__ void store(uint16_t* p, const float* v) { st8(p, v); }
};

struct F32ScalarPack {                 // 8 floats by scalar loads: no alignment asked of p
  using elem = float;
  static constexpr int n = 8;
  static __device__ __forceinline__ void load(const float* p, float* v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[i];
  }
};

// ---- work item id -> (image, output row, output column, first channel of pack id % cn) -----
struct Pixel {
  int b, yo, xo, c;
};
template <int N>
__device__ __forceinline__ Pixel decode_pixel(int64_t id, int cn, int Ho, int Wo) {
  Pixel p;
  p.c = static_cast<int>(id % cn) * N;
  int64_t pix = id / cn;
  p.xo = static_cast<int>(pix % Wo);
  pix /= Wo;
  p.yo = static_cast<int>(pix % Ho);
  p.b = static_cast<int>(pix / Ho);
  return p;
}
__device__ __forceinline__ int64_t pixel_offset(const Pixel& p, int H, int W, int64_t ld) {
  return ((static_cast<int64_t>(p.b) * H + p.yo) * W + p.xo) * ld + p.c;
}

// ---- bilinear resize, align_corners=True ------------------------------------------------
// scale = (in - 1) / (out - 1) as a float (TF resize_bilinear_op.cc, align_corners)
inline float align_corners_scale(int in, int out) {
  return out > 1 ? static_cast<float>(in - 1) / static_cast<float>(out - 1) : 0.f;
}
template <class E>
struct BilinearSrc {                   // one source map [B, Hi, Wi, C] at pitch ldx
  const E* X;
  int64_t ldx;
  int32_t Hi, Wi;
  float sy, sx;                        // align_corners_scale to the output size
};

// One source's value at output pixel (b, yo, xo), channels [c, c + P::n), in TF's arithmetic
// order: f = o * scale, taps floor(f) and ceil(f), weight f - floor(f), the two lerps along x
// as a + (b - a) * w, then the one along y; no contraction (the library is built with
// -ffp-contract=off). Every entry point that resizes goes through here, so they agree bit for
// bit. The upper tap needs its clamp (ceil of the last coordinate can round past in - 1); the
// lower one is <= in - 1 for every in < 2^23 and is clamped all the same, so that no load
// leaves the map whatever the sizes.
template <class P>
__device__ __forceinline__ void bilinear_sample(const BilinearSrc<typename P::elem>& src, int b,
                                                int yo, int xo, int c, float* out) {
  const float fy = static_cast<float>(yo) * src.sy;
  const float fx = static_cast<float>(xo) * src.sx;
  const int y0 = min(static_cast<int>(floorf(fy)), src.Hi - 1);
  const int x0 = min(static_cast<int>(floorf(fx)), src.Wi - 1);
  const int y1 = min(static_cast<int>(ceilf(fy)), src.Hi - 1);
  const int x1 = min(static_cast<int>(ceilf(fx)), src.Wi - 1);
  const float ly = fy - static_cast<float>(y0), lx = fx - static_cast<float>(x0);
  const typename P::elem* xb = src.X + static_cast<int64_t>(b) * src.Hi * src.Wi * src.ldx + c;
  float tl[P::n], tr[P::n], bl[P::n], br[P::n];
  P::load(xb + (static_cast<int64_t>(y0) * src.Wi + x0) * src.ldx, tl);
  P::load(xb + (static_cast<int64_t>(y0) * src.Wi + x1) * src.ldx, tr);
  P::load(xb + (static_cast<int64_t>(y1) * src.Wi + x0) * src.ldx, bl);
  P::load(xb + (static_cast<int64_t>(y1) * src.Wi + x1) * src.ldx, br);
#pragma unroll
  for (int i = 0; i < P::n; ++i) {
    const float top = tl[i] + (tr[i] - tl[i]) * lx;
    const float bot = bl[i] + (br[i] - bl[i]) * lx;
    out[i] = top + (bot - top) * ly;
  }
}

}  // namespace epos
