// Multi-scale inference (model.py:515-626): bilinear resize (align_corners=True) of up to
// eight sources to one output size, merged elementwise by max or mean -- one launch per head.
// S = 1 is a plain resize at any channel count (the per-scale input images, C = 3).
#include "nhwc.h"

namespace epos {
namespace {

constexpr int kMaxSrc = 8;

struct ResizeSrcsK {
  BilinearSrc<float> s[kMaxSrc];
};

// One output pack: the sources' values (bilinear_sample, nhwc.h) merged in source order.
template <int W>
__device__ __forceinline__ void resize_merge_at(const ResizeSrcsK& srcs, int S, int merge,
                                                float* Y, int64_t ldy, int b, int yo, int xo,
                                                int Ho, int Wo, int c) {
#pragma clang fp contract(off)
  using P = F32Pack<W>;
  float acc[W], v[W];
  bilinear_sample<P>(srcs.s[0], b, yo, xo, c, acc);
  for (int s = 1; s < S; ++s) {
    bilinear_sample<P>(srcs.s[s], b, yo, xo, c, v);
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
  P::store(Y + ((static_cast<int64_t>(b) * Ho + yo) * Wo + xo) * ldy + c, acc);
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
    k.s[s].sy = align_corners_scale(src.Hi, Ho);
    k.s[s].sx = align_corners_scale(src.Wi, Wo);
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
