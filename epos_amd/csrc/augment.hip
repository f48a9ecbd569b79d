// Training-time image augmentation on the device (include/epos_hip.h, "Augmentation";
// DESIGN.md, "Losses", "Augmentation"): brightness, contrast, saturation, hue, Gaussian blur,
// Gaussian noise and a baseline-JPEG round trip, in place on f32 [B,h,w,3] images in [0,255].
//
// One image's ops are cut into stages on the host: a run of pointwise ops is ONE pass (the
// affine of a contrast op opens such a run, its channel means come from the sum stage in front
// of it), a blur is a row and a column pass, a JPEG round trip a block pass (colour transform,
// chroma downsampling, DCT, quantisation and back, per 16x16 MCU through LDS) and a pixel pass
// (chroma upsampling, colour transform back). Stage s of every image of a chunk of up to 8
// images goes into the same launches (the image is the grid's y), so the number of launches
// does not depend on B up to 8. The per-image tables travel as kernel arguments: nothing is
// uploaded and nothing waits. No floating-point atomics: the same bytes in every run and at
// every position of a batch.
#include <math.h>

#include <cmath>

#include "common.h"

namespace epos {
namespace {

constexpr int MAX_OPS = 8;       // ops per image
constexpr int CHUNK = 8;         // images per launch
constexpr int SUM_BLOCKS = 64;   // partial sums per image of a contrast mean
constexpr int MAX_R = 32;        // blur radius
constexpr int THREADS = 256;

enum StageType { ST_POINTWISE = 0, ST_SUM, ST_BLUR, ST_JPEG, ST_TYPES };
enum { F_ACTIVE = 1, F_IN255 = 2, F_OUT255 = 4 };

struct PwOp { int32_t kind; float a; uint32_t key_lo, key_hi; };
struct PwImage { int32_t n, flags; PwOp ops[MAX_OPS]; };
struct PwArgs { PwImage img[CHUNK]; };
struct SumArgs { int32_t flags[CHUNK]; };
struct BlurImage { int32_t flags, R; float w[MAX_R + 1]; };
struct BlurArgs { BlurImage img[CHUNK]; };
struct JpegArgs { int32_t flags[CHUNK]; int32_t quality[CHUNK]; double T[64]; };

// per-image workspace: the partial sums, the blur's intermediate image, the JPEG planes
struct Layout { int64_t partials, tmp, planes, total; };
Layout layout(int h, int w) {
  Layout l;
  int64_t H16 = round_up(h, 16), W16 = round_up(w, 16);
  l.partials = 0;
  l.tmp = round_up(SUM_BLOCKS * 3 * sizeof(double), 256);
  l.planes = l.tmp + round_up(int64_t(h) * w * 3 * sizeof(float), 256);
  l.total = l.planes + round_up(H16 * W16 * 3 / 2, 256);
  return l;
}

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// ---- colour: the hexcone HSV, h in [0,1), h = 0 where max = min
__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float& h, float& s,
                                           float& v) {
  float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  float d = mx - mn;
  v = mx;
  s = mx > 0.f ? d / mx : 0.f;
  if (d == 0.f) { h = 0.f; return; }
  float t;
  if (mx == r) t = (g - b) / d;
  else if (mx == g) t = (b - r) / d + 2.f;
  else t = (r - g) / d + 4.f;
  t = t / 6.f;
  h = t - floorf(t);
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float& r, float& g,
                                           float& b) {
  float h6 = h * 6.f;
  float fi = floorf(h6);
  float f = h6 - fi;
  int i = static_cast<int>(fi) % 6;
  if (i < 0) i += 6;
  float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// ---- Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1,
                                              uint32_t r[4]) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
    uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
    c1 = uint32_t(p1); c3 = uint32_t(p0); c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// Box-Muller on (ra, rb): the radius in fp64 ((ra >> 8) + 0.5 needs 25 bits), the angle in fp32
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
  double u1 = (double(ra >> 8) + 0.5) * (1.0 / 16777216.0);
  float rad = static_cast<float>(sqrt(-2.0 * log(u1)));
  float u2 = float(rb >> 8) * (1.f / 16777216.f);
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

// ---- stage: a run of pointwise ops. One thread = 4 pixels = 12 values = 3 Philox counters.
__global__ __launch_bounds__(THREADS) void augment_pointwise_kernel(
    float* images, int64_t n_vals, const char* work, int64_t work_stride, PwArgs args, int vec) {
  const int b = blockIdx.y;
  const int flags = args.img[b].flags;
  if (!(flags & F_ACTIVE)) return;
  const int n_ops = args.img[b].n;
  float* img = images + b * n_vals;
  __shared__ float mean[3];
  if (n_ops > 0 && args.img[b].ops[0].kind == EPOS_AUG_CONTRAST) {
    // the closing pass of the mean: the partials in their order, by every workgroup alike
    if (threadIdx.x < 3) {
      const double* part = reinterpret_cast<const double*>(work + b * work_stride);
      double s = 0.0;
      for (int k = 0; k < SUM_BLOCKS; ++k) s += part[k * 3 + threadIdx.x];
      mean[threadIdx.x] = static_cast<float>(s / double(n_vals / 3));
    }
    __syncthreads();
  }
  const int64_t g = int64_t(blockIdx.x) * THREADS + threadIdx.x;
  const int64_t first = g * 12;
  if (first >= n_vals) return;
  const int count = static_cast<int>(n_vals - first < 12 ? n_vals - first : 12);
  float v[12];
  if (vec && count == 12) {
    const float4* p = reinterpret_cast<const float4*>(img + first);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float4 q = p[k];
      v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = k < count ? img[first + k] : 0.f;
  }
  if (flags & F_IN255) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = v[k] / 255.f;
  }
  for (int o = 0; o < n_ops; ++o) {
    const int kind = args.img[b].ops[o].kind;
    const float a = args.img[b].ops[o].a;
    if (kind == EPOS_AUG_BRIGHTNESS) {
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] = clip01(v[k] + a);
    } else if (kind == EPOS_AUG_CONTRAST) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        float m = mean[k % 3];
        v[k] = clip01((v[k] - m) * a + m);
      }
    } else if (kind == EPOS_AUG_SATURATION || kind == EPOS_AUG_HUE) {
#pragma unroll
      for (int k = 0; k < 12; k += 3) {
        float h, s, val;
        rgb_to_hsv(v[k], v[k + 1], v[k + 2], h, s, val);
        if (kind == EPOS_AUG_SATURATION) {
          s = clip01(s * a);
        } else {
          h = h + a;
          h = h - floorf(h);
          if (h >= 1.f) h = 0.f;
        }
        hsv_to_rgb(h, s, val, v[k], v[k + 1], v[k + 2]);
        v[k] = clip01(v[k]); v[k + 1] = clip01(v[k + 1]); v[k + 2] = clip01(v[k + 2]);
      }
    } else if (kind == EPOS_AUG_NOISE) {
      const uint32_t k0 = args.img[b].ops[o].key_lo, k1 = args.img[b].ops[o].key_hi;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        uint32_t r[4];
        philox4x32_10(static_cast<uint32_t>(g * 3 + q), k0, k1, r);
        float z[4];
        box_muller(r[0], r[1], z[0], z[1]);
        box_muller(r[2], r[3], z[2], z[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * q + k] = clip01(v[4 * q + k] + a * z[k]);
      }
    }
  }
  if (flags & F_OUT255) {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = v[k] * 255.f;
  }
  if (vec && count == 12) {
    float4* p = reinterpret_cast<float4*>(img + first);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2],
                                                   v[4 * k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < count) img[first + k] = v[k];
  }
}

// ---- stage: the channel sums of a contrast op, fp64. Workgroup k of SUM_BLOCKS sums the
// pixels [k * per, (k + 1) * per); a thread its pixels in rising order; then the wave butterfly
// and the four waves in their order.
__global__ __launch_bounds__(THREADS) void augment_channel_sums_kernel(
    const float* images, int64_t n_vals, char* work, int64_t work_stride, SumArgs args) {
  const int b = blockIdx.y;
  const int flags = args.flags[b];
  if (!(flags & F_ACTIVE)) return;
  const float* img = images + b * n_vals;
  const int64_t npix = n_vals / 3;
  const int64_t per = (npix + SUM_BLOCKS - 1) / SUM_BLOCKS;
  const int64_t p0 = blockIdx.x * per;
  const int64_t p1 = p0 + per < npix ? p0 + per : npix;
  const bool in255 = flags & F_IN255;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t p = p0 + threadIdx.x; p < p1; p += THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x = img[p * 3 + c];
      if (in255) x = x / 255.f;
      s[c] += double(x);
    }
  }
  __shared__ double part[THREADS / 64][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; ++c) part[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int k = 0; k < THREADS / 64; ++k) t += part[k][threadIdx.x];
    reinterpret_cast<double*>(work + b * work_stride)[blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// ---- stage: blur. BORDER_REFLECT_101; R <= n - 1, so one reflection lands inside.
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// ROWS: image -> tmp along x; else tmp -> image along y.
template <bool ROWS>
__global__ __launch_bounds__(THREADS) void augment_blur_kernel(
    float* images, int64_t n_vals, int h, int w, char* work, int64_t work_stride,
    int64_t tmp_offset, BlurArgs args) {
  const int b = blockIdx.y;
  const int flags = args.img[b].flags;
  if (!(flags & F_ACTIVE)) return;
  const int R = args.img[b].R;
  __shared__ float wt[MAX_R + 1];
  if (threadIdx.x <= R) wt[threadIdx.x] = args.img[b].w[threadIdx.x];
  __syncthreads();
  const int64_t i = int64_t(blockIdx.x) * THREADS + threadIdx.x;
  if (i >= n_vals) return;
  float* img = images + b * n_vals;
  float* tmp = reinterpret_cast<float*>(work + b * work_stride + tmp_offset);
  const float* src = ROWS ? img : tmp;
  float* dst = ROWS ? tmp : img;
  const int c = static_cast<int>(i % 3);
  const int64_t p = i / 3;
  const int x = static_cast<int>(p % w), y = static_cast<int>(p / w);
  const bool in255 = ROWS && (flags & F_IN255);
  float acc = 0.f;
  for (int k = -R; k <= R; ++k) {
    int64_t at = ROWS ? (int64_t(y) * w + reflect101(x + k, w)) * 3 + c
                      : (int64_t(reflect101(y + k, h)) * w + x) * 3 + c;
    float t = src[at];
    if (in255) t = t / 255.f;
    acc += wt[k < 0 ? -k : k] * t;
  }
  if (!ROWS && (flags & F_OUT255)) acc = acc * 255.f;
  dst[i] = acc;
}

// ---- stage: the JPEG round trip
__device__ const uint8_t kLuma[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__device__ const uint8_t kChroma[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

constexpr int fix16(double c) { return static_cast<int>(c * 65536.0 + 0.5); }

// One workgroup = one 16x16 MCU: thread t = pixel (t / 16, t % 16), clamped to the image
// (padding by replication). Blocks 0..3 = Y (row-major 2x2), 4 = Cb, 5 = Cr. T[u*8+x] =
// C(u)/2 cos((2x+1) u pi / 16): F = T f T^t, f = T^t F T, each as two passes in fp64.
__global__ __launch_bounds__(THREADS) void augment_jpeg_blocks_kernel(
    const float* images, int64_t n_vals, int h, int w, char* work, int64_t work_stride,
    int64_t planes_offset, JpegArgs args) {
  const int b = blockIdx.y;
  const int flags = args.flags[b];
  if (!(flags & F_ACTIVE)) return;
  const float* img = images + b * n_vals;
  const int W16 = (w + 15) / 16 * 16, H16 = (h + 15) / 16 * 16;
  const int mcus_x = W16 / 16;
  const int my = blockIdx.x / mcus_x, mx = blockIdx.x % mcus_x;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  __shared__ double f[6 * 64];
  __shared__ double g[6 * 64];
  __shared__ double Ts[64];
  __shared__ int cbs[16][17], crs[16][17];
  __shared__ int qt[2][64];
  {
    int y = my * 16 + ty, x = mx * 16 + tx;
    y = y < h ? y : h - 1;
    x = x < w ? x : w - 1;
    const float* px = img + (int64_t(y) * w + x) * 3;
    int rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = px[c];
      if (flags & F_IN255) v = v / 255.f;
      float q = floorf(v * 255.5f);
      rgb[c] = q >= 255.f ? 255 : (q > 0.f ? static_cast<int>(q) : 0);
    }
    const int R = rgb[0], G = rgb[1], B = rgb[2];
    int Y = (fix16(.299) * R + fix16(.587) * G + fix16(.114) * B + 32768) >> 16;
    cbs[ty][tx] = (-fix16(.16874) * R - fix16(.33126) * G + fix16(.5) * B + (128 << 16) +
                   32767) >> 16;
    crs[ty][tx] = (fix16(.5) * R - fix16(.41869) * G - fix16(.08131) * B + (128 << 16) +
                   32767) >> 16;
    f[((ty >> 3) * 2 + (tx >> 3)) * 64 + (ty & 7) * 8 + (tx & 7)] = double(Y - 128);
  }
  if (t < 64) Ts[t] = args.T[t];
  if (t < 128) {
    const int q = args.quality[b];
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    const int base = t < 64 ? kLuma[t] : kChroma[t - 64];
    int d = (base * scale + 50) / 100;
    qt[t >> 6][t & 63] = d < 1 ? 1 : (d > 255 ? 255 : d);
  }
  __syncthreads();
  if (t < 128) {
    const int cy = (t >> 3) & 7, cx = t & 7, bias = (cx & 1) ? 2 : 1;
    int (*pl)[17] = t < 64 ? cbs : crs;
    // below the image the last chroma ROW is replicated, not the mean of replicated pixels
    const int last = (h + 1) / 2 - 1 - my * 8;
    const int sy = cy < last ? cy : last;
    int s = (pl[2 * sy][2 * cx] + pl[2 * sy][2 * cx + 1] + pl[2 * sy + 1][2 * cx] +
             pl[2 * sy + 1][2 * cx + 1] + bias) >> 2;
    f[(4 + (t >> 6)) * 64 + cy * 8 + cx] = double(s - 128);
  }
  __syncthreads();
  for (int i = t; i < 384; i += THREADS) {       // g[y][u] = sum_x f[y][x] T[u][x]
    const int blk = i >> 6, y = (i >> 3) & 7, u = i & 7;
    double s = 0.0;
#pragma unroll
    for (int x = 0; x < 8; ++x) s += f[blk * 64 + y * 8 + x] * Ts[u * 8 + x];
    g[i] = s;
  }
  __syncthreads();
  for (int i = t; i < 384; i += THREADS) {       // F[v][u] = sum_y T[v][y] g[y][u]; quantise
    const int blk = i >> 6, v = (i >> 3) & 7, u = i & 7;
    double s = 0.0;
#pragma unroll
    for (int y = 0; y < 8; ++y) s += g[blk * 64 + y * 8 + u] * Ts[v * 8 + y];
    const double d = double(qt[blk >= 4][v * 8 + u]);
    const double level = floor(fabs(s) / d + 0.5) * d;
    f[i] = s < 0.0 ? -level : level;
  }
  __syncthreads();
  for (int i = t; i < 384; i += THREADS) {       // g[v][x] = sum_u F[v][u] T[u][x]
    const int blk = i >> 6, v = (i >> 3) & 7, x = i & 7;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += f[blk * 64 + v * 8 + u] * Ts[u * 8 + x];
    g[i] = s;
  }
  __syncthreads();
  uint8_t* planeY = reinterpret_cast<uint8_t*>(work + b * work_stride + planes_offset);
  uint8_t* planeC = planeY + int64_t(H16) * W16;
  const int CW = W16 / 2, CH = H16 / 2;
  for (int i = t; i < 384; i += THREADS) {       // f'[y][x] = sum_v T[v][y] g[v][x]
    const int blk = i >> 6, y = (i >> 3) & 7, x = i & 7;
    double s = 0.0;
#pragma unroll
    for (int v = 0; v < 8; ++v) s += g[blk * 64 + v * 8 + x] * Ts[v * 8 + y];
    s = rint(s + 128.0);
    const uint8_t out = static_cast<uint8_t>(s < 0.0 ? 0.0 : (s > 255.0 ? 255.0 : s));
    if (blk < 4) {
      planeY[int64_t(my * 16 + (blk >> 1) * 8 + y) * W16 + mx * 16 + (blk & 1) * 8 + x] = out;
    } else {
      planeC[int64_t(blk - 4) * CH * CW + int64_t(my * 8 + y) * CW + mx * 8 + x] = out;
    }
  }
}

// One thread = one pixel: the "fancy" h2v2 triangle upsampling of the ceil(h/2) x ceil(w/2)
// chroma samples, then YCbCr -> RGB.
__global__ __launch_bounds__(THREADS) void augment_jpeg_pixels_kernel(
    float* images, int64_t n_vals, int h, int w, const char* work, int64_t work_stride,
    int64_t planes_offset, JpegArgs args) {
  const int b = blockIdx.y;
  const int flags = args.flags[b];
  if (!(flags & F_ACTIVE)) return;
  const int64_t p = int64_t(blockIdx.x) * THREADS + threadIdx.x;
  if (p >= n_vals / 3) return;
  const int x = static_cast<int>(p % w), y = static_cast<int>(p / w);
  const int W16 = (w + 15) / 16 * 16, H16 = (h + 15) / 16 * 16;
  const int CW = W16 / 2, CH = H16 / 2, cw = (w + 1) / 2, ch = (h + 1) / 2;
  const uint8_t* planeY = reinterpret_cast<const uint8_t*>(work + b * work_stride +
                                                           planes_offset);
  const uint8_t* planeC = planeY + int64_t(H16) * W16;
  const int Y = planeY[int64_t(y) * W16 + x];
  const int cy = y >> 1, cx = x >> 1;
  int far = (y & 1) ? cy + 1 : cy - 1;
  if (far < 0 || far >= ch) far = cy;
  const int side = (x & 1) ? cx + 1 : cx - 1;
  const bool edge = side < 0 || side >= cw;
  int c2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint8_t* pl = planeC + int64_t(k) * CH * CW;
    const uint8_t* near_row = pl + int64_t(cy) * CW;
    const uint8_t* far_row = pl + int64_t(far) * CW;
    const int cur = 3 * near_row[cx] + far_row[cx];
    const int round = (x & 1) ? 7 : 8;
    if (edge) {
      c2[k] = (4 * cur + round) >> 4;
    } else {
      const int other = 3 * near_row[side] + far_row[side];
      c2[k] = (3 * cur + other + round) >> 4;
    }
  }
  const int cb = c2[0] - 128, cr = c2[1] - 128;
  int rgb[3];
  rgb[0] = Y + ((fix16(1.402) * cr + 32768) >> 16);
  rgb[1] = Y + ((-fix16(.34414) * cb - fix16(.71414) * cr + 32768) >> 16);
  rgb[2] = Y + ((fix16(1.772) * cb + 32768) >> 16);
  float* px = images + b * n_vals + p * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int v = rgb[c] < 0 ? 0 : (rgb[c] > 255 ? 255 : rgb[c]);
    float o = float(v) / 255.f;
    if (flags & F_OUT255) o = o * 255.f;
    px[c] = o;
  }
}

// ---- host: one image's ops as stages
struct Stage {
  int type;
  int flags;
  int n_ops;                 // ST_POINTWISE
  PwOp ops[MAX_OPS];
  int R;                     // ST_BLUR
  float w[MAX_R + 1];
  int quality;               // ST_JPEG
};
struct Program { int n; Stage st[2 * MAX_OPS + 1]; };

// ksize = round_half_even(8 sigma + 1) | 1 (the default rounding mode: to nearest even)
int blur_radius(double sigma) {
  int64_t ksize = static_cast<int64_t>(nearbyint(sigma * 8.0 + 1.0)) | 1;
  return static_cast<int>((ksize - 1) / 2);
}

bool is_noop(const EposAugmentOp& op) {
  if (op.kind == EPOS_AUG_NONE) return true;
  return op.kind == EPOS_AUG_BLUR && (op.a == 0.f || blur_radius(op.a) == 0);
}

void compile(const EposAugmentOp* ops, int n_ops, Program* prog) {
  prog->n = 0;
  Stage cur;
  cur.type = ST_POINTWISE;
  cur.n_ops = 0;
  auto flush = [&]() {
    if (cur.n_ops) prog->st[prog->n++] = cur;
    cur.n_ops = 0;
  };
  for (int i = 0; i < n_ops; ++i) {
    const EposAugmentOp& op = ops[i];
    if (is_noop(op)) continue;
    if (op.kind == EPOS_AUG_BLUR) {
      flush();
      Stage& s = prog->st[prog->n++];
      s.type = ST_BLUR;
      s.R = blur_radius(op.a);
      const double sigma = op.a;
      double e[MAX_R + 1], sum = 0.0;
      for (int k = 0; k <= s.R; ++k) e[k] = exp(-double(k) * k / (2.0 * sigma * sigma));
      for (int k = -s.R; k <= s.R; ++k) sum += e[k < 0 ? -k : k];
      for (int k = 0; k <= MAX_R; ++k) s.w[k] = k <= s.R ? static_cast<float>(e[k] / sum) : 0.f;
    } else if (op.kind == EPOS_AUG_JPEG) {
      flush();
      Stage& s = prog->st[prog->n++];
      s.type = ST_JPEG;
      s.quality = static_cast<int>(op.a);
    } else {
      if (op.kind == EPOS_AUG_CONTRAST) {
        flush();
        prog->st[prog->n++].type = ST_SUM;
      }
      PwOp& o = cur.ops[cur.n_ops++];
      o.kind = op.kind; o.a = op.a; o.key_lo = op.key_lo; o.key_hi = op.key_hi;
    }
  }
  flush();
  // the image is in [0,255] until the first stage that writes it, and again after the last
  bool in255 = true;
  for (int s = 0; s < prog->n; ++s) {
    prog->st[s].flags = F_ACTIVE | (in255 ? F_IN255 : 0) | (s == prog->n - 1 ? F_OUT255 : 0);
    if (prog->st[s].type != ST_SUM) in255 = false;
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_augment_workspace_bytes(int B, int h, int w) {
  EPOS_REQUIRE(B >= 0 && h >= 1 && w >= 1, "B >= 0, h >= 1 and w >= 1 are required");
  EPOS_REQUIRE(int64_t(h) * w * 3 < (int64_t(1) << 31), "an image of 2^31 values or more");
  return B * layout(h, w).total;
}

extern "C" int epos_augment_f32(float* images, int B, int h, int w, const EposAugmentOp* ops,
                                int n_ops, void* work, void* stream) {
  EPOS_REQUIRE(B >= 0 && h >= 1 && w >= 1, "B >= 0, h >= 1 and w >= 1 are required");
  EPOS_REQUIRE(int64_t(h) * w * 3 < (int64_t(1) << 31), "an image of 2^31 values or more");
  EPOS_REQUIRE(n_ops >= 0 && n_ops <= MAX_OPS, "n_ops must lie in 0..8");
  if (B == 0 || n_ops == 0) return EPOS_OK;
  EPOS_REQUIRE(images && ops, "null images or ops");
  EPOS_REQUIRE((reinterpret_cast<uintptr_t>(images) & 3) == 0, "images not 4-byte aligned");
  bool need_work = false;
  for (int64_t i = 0; i < int64_t(B) * n_ops; ++i) {
    const EposAugmentOp& op = ops[i];
    EPOS_REQUIRE(op.kind >= EPOS_AUG_NONE && op.kind <= EPOS_AUG_JPEG, "unknown op kind");
    if (op.kind == EPOS_AUG_NONE) continue;
    EPOS_REQUIRE(std::isfinite(op.a), "an op parameter that is not finite");
    if (op.kind == EPOS_AUG_BLUR) {
      EPOS_REQUIRE(op.a >= 0.f, "blur: negative sigma");
      EPOS_REQUIRE(op.a <= 8.25f, "blur: radius above 32");
      const int R = blur_radius(op.a);
      EPOS_REQUIRE(R <= MAX_R, "blur: radius above 32");
      EPOS_REQUIRE(R <= (h < w ? h : w) - 1, "blur: radius above min(h, w) - 1");
    } else if (op.kind == EPOS_AUG_NOISE) {
      EPOS_REQUIRE(op.a >= 0.f, "noise: negative sigma");
    } else if (op.kind == EPOS_AUG_JPEG) {
      EPOS_REQUIRE(op.a >= 1.f && op.a <= 100.f && op.a == floorf(op.a),
                   "jpeg: quality must be an integer in 1..100");
    }
    if (!is_noop(op) && (op.kind == EPOS_AUG_BLUR || op.kind == EPOS_AUG_JPEG ||
                         op.kind == EPOS_AUG_CONTRAST)) need_work = true;
  }
  EPOS_REQUIRE(!need_work || work, "null workspace");
  EPOS_REQUIRE(!need_work || al16(work), "workspace not 16-byte aligned");

  hipStream_t s = static_cast<hipStream_t>(stream);
  const Layout lay = layout(h, w);
  const int64_t n_vals = int64_t(h) * w * 3;
  const int vec = al16(images) && n_vals % 4 == 0;
  JpegArgs jpeg;
  bool have_T = false;
  Program prog[CHUNK];
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    int max_stages = 0;
    for (int b = 0; b < nb; ++b) {
      compile(ops + int64_t(b0 + b) * n_ops, n_ops, &prog[b]);
      if (prog[b].n > max_stages) max_stages = prog[b].n;
    }
    float* img0 = images + b0 * n_vals;
    char* work0 = static_cast<char*>(work) + b0 * lay.total;
    for (int st = 0; st < max_stages; ++st) {
      bool present[ST_TYPES] = {false, false, false, false};
      for (int b = 0; b < nb; ++b)
        if (st < prog[b].n) present[prog[b].st[st].type] = true;
      if (present[ST_POINTWISE]) {
        PwArgs a;
        for (int b = 0; b < CHUNK; ++b) {
          a.img[b].n = 0;
          a.img[b].flags = 0;
          for (int o = 0; o < MAX_OPS; ++o) a.img[b].ops[o] = PwOp{0, 0.f, 0u, 0u};
          if (b < nb && st < prog[b].n && prog[b].st[st].type == ST_POINTWISE) {
            const Stage& g = prog[b].st[st];
            a.img[b].n = g.n_ops;
            a.img[b].flags = g.flags;
            for (int o = 0; o < g.n_ops; ++o) a.img[b].ops[o] = g.ops[o];
          }
        }
        dim3 grid(blocks_for(ceil_div(n_vals, 12), THREADS), nb);
        hipLaunchKernelGGL(augment_pointwise_kernel, grid, dim3(THREADS), 0, s, img0, n_vals,
                           work0, lay.total, a, vec);
        int rc = launch_status("augment_pointwise_kernel");
        if (rc) return rc;
      }
      if (present[ST_SUM]) {
        SumArgs a;
        for (int b = 0; b < CHUNK; ++b)
          a.flags[b] = (b < nb && st < prog[b].n && prog[b].st[st].type == ST_SUM)
                           ? prog[b].st[st].flags : 0;
        hipLaunchKernelGGL(augment_channel_sums_kernel, dim3(SUM_BLOCKS, nb), dim3(THREADS), 0,
                           s, img0, n_vals, work0, lay.total, a);
        int rc = launch_status("augment_channel_sums_kernel");
        if (rc) return rc;
      }
      if (present[ST_BLUR]) {
        BlurArgs a;
        for (int b = 0; b < CHUNK; ++b) {
          a.img[b].flags = 0;
          a.img[b].R = 0;
          for (int k = 0; k <= MAX_R; ++k) a.img[b].w[k] = 0.f;
          if (b < nb && st < prog[b].n && prog[b].st[st].type == ST_BLUR) {
            const Stage& g = prog[b].st[st];
            a.img[b].flags = g.flags;
            a.img[b].R = g.R;
            for (int k = 0; k <= MAX_R; ++k) a.img[b].w[k] = g.w[k];
          }
        }
        dim3 grid(blocks_for(n_vals, THREADS), nb);
        hipLaunchKernelGGL(augment_blur_kernel<true>, grid, dim3(THREADS), 0, s, img0, n_vals,
                           h, w, work0, lay.total, lay.tmp, a);
        int rc = launch_status("augment_blur_kernel<rows>");
        if (rc) return rc;
        hipLaunchKernelGGL(augment_blur_kernel<false>, grid, dim3(THREADS), 0, s, img0, n_vals,
                           h, w, work0, lay.total, lay.tmp, a);
        rc = launch_status("augment_blur_kernel<columns>");
        if (rc) return rc;
      }
      if (present[ST_JPEG]) {
        if (!have_T) {
          const double pi = 3.14159265358979323846;
          for (int u = 0; u < 8; ++u)
            for (int x = 0; x < 8; ++x)
              jpeg.T[u * 8 + x] = 0.5 * (u == 0 ? sqrt(0.5) : 1.0) *
                                  cos((2 * x + 1) * u * pi / 16.0);
          have_T = true;
        }
        for (int b = 0; b < CHUNK; ++b) {
          const bool on = b < nb && st < prog[b].n && prog[b].st[st].type == ST_JPEG;
          jpeg.flags[b] = on ? prog[b].st[st].flags : 0;
          jpeg.quality[b] = on ? prog[b].st[st].quality : 50;
        }
        const int mcus = static_cast<int>(ceil_div(h, 16) * ceil_div(w, 16));
        hipLaunchKernelGGL(augment_jpeg_blocks_kernel, dim3(mcus, nb), dim3(THREADS), 0, s,
                           img0, n_vals, h, w, work0, lay.total, lay.planes, jpeg);
        int rc = launch_status("augment_jpeg_blocks_kernel");
        if (rc) return rc;
        dim3 grid(blocks_for(n_vals / 3, THREADS), nb);
        hipLaunchKernelGGL(augment_jpeg_pixels_kernel, grid, dim3(THREADS), 0, s, img0, n_vals,
                           h, w, work0, lay.total, lay.planes, jpeg);
        rc = launch_status("augment_jpeg_pixels_kernel");
        if (rc) return rc;
      }
    }
  }
  return EPOS_OK;
}
