// Multi-scale inference (model.py:515-626): bilinear resize (align_corners=True) of up to
// eight sources to one output size, merged elementwise by max or mean -- one launch per head.
// S = 1 is a plain resize at any channel count (the per-scale input images, C = 3).
#include "common.h"

namespace epos {
namespace {

constexpr int kMaxSrc = 8;

struct ResizeSrcK {
  const float* X;
  int64_t ldx;
  int32_t Hi, Wi;
  float sy, sx;
};

struct ResizeSrcsK {
  ResizeSrcK s[kMaxSrc];
};

template <int V>
struct VecT;
template <>
struct VecT<1> { using T = float; };
template <>
struct VecT<2> { using T = float2; };
template <>
struct VecT<4> { using T = float4; };

template <int V>
__device__ __forceinline__ void load_v(const float* p, float* v) {
  const typename VecT<V>::T t = *reinterpret_cast<const typename VecT<V>::T*>(p);
  const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
  for (int i = 0; i < V; ++i) v[i] = f[i];
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
  typename VecT<V>::T t;
  float* f = reinterpret_cast<float*>(&t);
#pragma unroll
  for (int i = 0; i < V; ++i) f[i] = v[i];
  *reinterpret_cast<typename VecT<V>::T*>(p) = t;
}

// One source's contribution at (b, yo, xo), channels [c, c + W): TF's align_corners
// arithmetic in the order of resize_bilinear_kernel (csrc/layers.hip), no contraction.
template <int W>
__device__ __forceinline__ void sample(const ResizeSrcK& src, int b, int yo, int xo, int c,
                                       float* out) {
#pragma clang fp contract(off)
  const float fy = static_cast<float>(yo) * src.sy;
  const float fx = static_cast<float>(xo) * src.sx;
  // (lo <= in - 1 always holds for in < 2^23; the min only keeps the loads in bounds)
  const int y0 = min(static_cast<int>(floorf(fy)), src.Hi - 1);
  const int x0 = min(static_cast<int>(floorf(fx)), src.Wi - 1);
  const int y1 = min(static_cast<int>(ceilf(fy)), src.Hi - 1);
  const int x1 = min(static_cast<int>(ceilf(fx)), src.Wi - 1);
  const float ly = fy - static_cast<float>(y0), lx = fx - static_cast<float>(x0);
  const float* xb = src.X + static_cast<int64_t>(b) * src.Hi * src.Wi * src.ldx + c;
  float tl[W], tr[W], bl[W], br[W];
  load_v<W>(xb + (static_cast<int64_t>(y0) * src.Wi + x0) * src.ldx, tl);
  load_v<W>(xb + (static_cast<int64_t>(y0) * src.Wi + x1) * src.ldx, tr);
  load_v<W>(xb + (static_cast<int64_t>(y1) * src.Wi + x0) * src.ldx, bl);
  load_v<W>(xb + (static_cast<int64_t>(y1) * src.Wi + x1) * src.ldx, br);
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const float top = tl[i] + (tr[i] - tl[i]) * lx;
    const float bot = bl[i] + (br[i] - bl[i]) * lx;
    out[i] = top + (bot - top) * ly;
  }
}

template <int W>
__device__ __forceinline__ void resize_merge_at(const ResizeSrcsK& srcs, int S, int merge,
                                                float* Y, int64_t ldy, int b, int yo, int xo,
                                                int Ho, int Wo, int c) {
#pragma clang fp contract(off)
  float acc[W], v[W];
  sample<W>(srcs.s[0], b, yo, xo, c, acc);
  for (int s = 1; s < S; ++s) {
    sample<W>(srcs.s[s], b, yo, xo, c, v);
    if (merge == EPOS_MERGE_MAX) {
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = fmaxf(acc[i], v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] + v[i];       // source order
    }
  }
  if (merge == EPOS_MERGE_MEAN && S > 1) {
    const float n = static_cast<float>(S);
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = acc[i] / n;
  }
  store_v<W>(Y + ((static_cast<int64_t>(b) * Ho + yo) * Wo + xo) * ldy + c, acc);
}

// Block = 256 threads on one output row (b, yo): `chunks` blocks per row, a row's pixels
// laid out as tpp = cv + tail threads each -- cv vectors of V channels, then `tail` single
// channels (C % V). Consecutive threads read consecutive vectors of one source pixel.
template <int V>
__global__ __launch_bounds__(256) void resize_merge_kernel(ResizeSrcsK srcs, int S, int merge,
                                                           float* Y, int64_t ldy, int Ho,
                                                           int Wo, int cv, int tail,
                                                           int chunks) {
  const int row = blockIdx.x / chunks;
  const unsigned t = (blockIdx.x - row * chunks) * 256u + threadIdx.x;
  const unsigned tpp = static_cast<unsigned>(cv + tail);
  const unsigned xo = t / tpp;
  if (xo >= static_cast<unsigned>(Wo)) return;
  const int j = static_cast<int>(t - xo * tpp);
  const int b = row / Ho, yo = row - b * Ho;
  if (j < cv)
    resize_merge_at<V>(srcs, S, merge, Y, ldy, b, yo, xo, Ho, Wo, j * V);
  else
    resize_merge_at<1>(srcs, S, merge, Y, ldy, b, yo, xo, Ho, Wo, cv * V + (j - cv));
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_resize_merge_f32(const EposResizeSrc* srcs, int S, float* Y, int64_t ldy,
                                     int B, int Ho, int Wo, int C, int merge, void* stream) {
  EPOS_REQUIRE(srcs && Y, "null pointer");
  EPOS_REQUIRE(S >= 1 && S <= kMaxSrc, "S must be in [1, 8]");
  EPOS_REQUIRE(C >= 1 && ldy >= C, "C >= 1 and ldy >= C");
  EPOS_REQUIRE(B >= 0 && Ho >= 0 && Wo >= 0, "negative size");
  EPOS_REQUIRE(merge == EPOS_MERGE_MAX || merge == EPOS_MERGE_MEAN, "unknown merge");
  ResizeSrcsK k = {};
  // the widest vector (4, 2 or 1 floats) that every row pitch and base pointer allows
  int V = (ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0) ? 4
          : (ldy % 2 == 0 && (reinterpret_cast<uintptr_t>(Y) & 7) == 0) ? 2 : 1;
  for (int s = 0; s < S; ++s) {
    const EposResizeSrc& src = srcs[s];
    EPOS_REQUIRE(src.X, "null source pointer");
    EPOS_REQUIRE(src.Hi >= 1 && src.Wi >= 1, "source size must be >= 1");
    EPOS_REQUIRE(src.ldx >= C, "ldx >= C");
    const uintptr_t a = reinterpret_cast<uintptr_t>(src.X);
    if (V == 4 && !(src.ldx % 4 == 0 && (a & 15) == 0)) V = 2;
    if (V == 2 && !(src.ldx % 2 == 0 && (a & 7) == 0)) V = 1;
    k.s[s].X = src.X;
    k.s[s].ldx = src.ldx;
    k.s[s].Hi = src.Hi;
    k.s[s].Wi = src.Wi;
    // scale = (in - 1) / (out - 1) as a float (resize_bilinear_op.cc, align_corners)
    k.s[s].sy = Ho > 1 ? static_cast<float>(src.Hi - 1) / static_cast<float>(Ho - 1) : 0.f;
    k.s[s].sx = Wo > 1 ? static_cast<float>(src.Wi - 1) / static_cast<float>(Wo - 1) : 0.f;
  }
  if (static_cast<int64_t>(B) * Ho * Wo == 0) return EPOS_OK;
  const int cv = C / V, tail = C % V;
  const int64_t row_threads = static_cast<int64_t>(Wo) * (cv + tail);
  EPOS_REQUIRE(row_threads < (int64_t(1) << 31), "output row too wide");
  const int64_t chunks = ceil_div(row_threads, 256);
  const int64_t blocks = chunks * B * Ho;
  // a grid holds fewer than 2^32 work-items (blocks * 256)
  EPOS_REQUIRE(blocks * 256 < (int64_t(1) << 32), "output too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ch = static_cast<int>(chunks);
  if (V == 4)
    hipLaunchKernelGGL(resize_merge_kernel<4>, dim3(blocks), dim3(256), 0, st, k, S, merge, Y,
                       ldy, Ho, Wo, cv, tail, ch);
  else if (V == 2)
    hipLaunchKernelGGL(resize_merge_kernel<2>, dim3(blocks), dim3(256), 0, st, k, S, merge, Y,
                       ldy, Ho, Wo, cv, tail, ch);
  else
    hipLaunchKernelGGL(resize_merge_kernel<1>, dim3(blocks), dim3(256), 0, st, k, S, merge, Y,
                       ldy, Ho, Wo, cv, tail, ch);
  return launch_status("resize_merge_kernel");
}
