// Mesh renderer: a batched z-buffered triangle rasteriser and the ground-truth fields built
// from its images (include/epos_hip.h, "Mesh renderer"; DESIGN.md, "Renderer").
//
// Everything here is a defined function of the input, not of the launch: vertices are
// transformed in fp64 with a fixed operation order (no FMA: the library is built with
// -ffp-contract=off), snapped to 1/256 pixel, coverage is decided by exact integer edge
// functions with a top-left rule, and the visible surface of a pixel is the minimum of a 64-bit
// key (fp32 depth bits, face index) taken with an unsigned atomic min, which does not depend
// on the order of arrival. tests/helpers/render_ref.py restates it in numpy; the two agree bit
// for bit.
//
// Work distribution of the raster pass: one lane per triangle. A triangle whose screen-clipped
// bounding box holds at most RASTER_LANE_MAX_PIXELS sample points is walked by its own lane;
// the larger ones are taken one after the other by the whole wavefront, whose 64 lanes share
// the box out among them (every lane repeats the triangle's set-up, which is a few dozen
// operations, instead of receiving it through cross-lane moves). Both paths evaluate the same
// expressions, so which one a triangle takes changes nothing in the result.
#include "common.h"

namespace epos {
namespace {

constexpr int RASTER_LANE_MAX_PIXELS = 256;  // bounding box samples one lane walks alone
constexpr int RASTER_THREADS = 256;          // faces per workgroup and chunk
constexpr int RASTER_BLOCKS_PER_INST = 64;   // workgroups striding over one instance's faces
constexpr int SUBPIX = 256;                  // snapping grid: 1/256 pixel
constexpr int64_t COORD_LIMIT = int64_t(1) << 31;  // |snapped coordinate| >= this: dropped
constexpr int64_t FAST_LIMIT = int64_t(1) << 29;   // below: edge products fit 64 bits
constexpr double SHADE_AMBIENT = 0.3, SHADE_DIFFUSE = 0.7;

// exact value of a wide edge function as a double: the high and the low 64-bit halves are
// converted separately and added (one rounding each; exact below 2^53). render_ref.py does
// the same on Python integers.
__device__ __forceinline__ double to_f64(int64_t v) { return static_cast<double>(v); }
__device__ __forceinline__ double to_f64(__int128 v) {
  const int64_t hi = static_cast<int64_t>(v >> 64);
  const uint64_t lo = static_cast<uint64_t>(v);
  return static_cast<double>(hi) * 18446744073709551616.0 + static_cast<double>(lo);
}

struct Tri {
  int64_t x[3], y[3];     // snapped image coordinates, 1/256 pixel
  double z[3];            // camera depth
  double cam[3][3];       // camera-space vertices (shading)
  int32_t vi[3];          // pooled vertex indices
  int x0, x1, y0, y1;     // screen-clipped bounding box in pixels, inclusive (empty: x1 < x0)
  bool ok, wide;
};

// Camera-space vertex, projection, snapping. false: behind `near` or out of the coordinate
// range (the triangle is dropped whole).
__device__ __forceinline__ bool project_vertex(const double* __restrict__ X,
                                               const EposRenderInst& in, double near,
                                               double* cam, int64_t* sx, int64_t* sy) {
  const double* R = in.R;
  cam[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + in.t[0];
  cam[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + in.t[1];
  cam[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + in.t[2];
  if (!(cam[2] >= near)) return false;
  const double u = in.fx * cam[0] / cam[2] + in.cx;
  const double v = in.fy * cam[1] / cam[2] + in.cy;
  const double su = rint(u * SUBPIX), sv = rint(v * SUBPIX);
  if (!(fabs(su) < 2147483648.0) || !(fabs(sv) < 2147483648.0)) return false;
  *sx = static_cast<int64_t>(su);
  *sy = static_cast<int64_t>(sv);
  return true;
}

__device__ __forceinline__ void setup_tri(const double* __restrict__ verts,
                                          const int32_t* __restrict__ faces, int64_t n_verts,
                                          int64_t n_faces_total, const EposRenderInst& in,
                                          int f, int h, int w, double near, Tri* t) {
  t->ok = false;
  t->x0 = 0; t->x1 = -1; t->y0 = 0; t->y1 = -1;
  const int64_t fi = static_cast<int64_t>(in.face_base) + f;
  if (f < 0 || in.face_base < 0 || in.vert_base < 0 || fi >= n_faces_total) return;
  int64_t xmin = COORD_LIMIT, xmax = -COORD_LIMIT, ymin = COORD_LIMIT, ymax = -COORD_LIMIT;
  int64_t amax = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t local = faces[3 * fi + k];
    const int64_t vi = static_cast<int64_t>(in.vert_base) + local;
    if (local < 0 || vi >= n_verts) return;
    t->vi[k] = static_cast<int32_t>(vi);
    if (!project_vertex(verts + 3 * vi, in, near, t->cam[k], &t->x[k], &t->y[k])) return;
    t->z[k] = t->cam[k][2];
    xmin = t->x[k] < xmin ? t->x[k] : xmin; xmax = t->x[k] > xmax ? t->x[k] : xmax;
    ymin = t->y[k] < ymin ? t->y[k] : ymin; ymax = t->y[k] > ymax ? t->y[k] : ymax;
    const int64_t ax = t->x[k] < 0 ? -t->x[k] : t->x[k], ay = t->y[k] < 0 ? -t->y[k] : t->y[k];
    amax = ax > amax ? ax : amax; amax = ay > amax ? ay : amax;
  }
  t->wide = amax >= FAST_LIMIT;
  // pixel x is sampled at 256 x + 128: first / last sample inside [min, max]
  int64_t x0 = (xmin - SUBPIX / 2 + SUBPIX - 1) >> 8, x1 = (xmax - SUBPIX / 2) >> 8;
  int64_t y0 = (ymin - SUBPIX / 2 + SUBPIX - 1) >> 8, y1 = (ymax - SUBPIX / 2) >> 8;
  x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
  x1 = x1 > w - 1 ? w - 1 : x1; y1 = y1 > h - 1 ? h - 1 : y1;
  t->x0 = static_cast<int>(x0); t->y0 = static_cast<int>(y0);
  t->x1 = x1 < x0 ? static_cast<int>(x0) - 1 : static_cast<int>(x1);
  t->y1 = y1 < y0 ? static_cast<int>(y0) - 1 : static_cast<int>(y1);
  t->ok = true;
}

// The three edge functions of a triangle at one sample point, oriented so that the inside is
// positive, and the top-left rule for points exactly on an edge. I = int64_t when every
// |coordinate| < 2^29 (products below 2^62), __int128 otherwise: both are exact.
template <typename I>
struct Edges {
  I dx[3], dy[3];         // oriented edge vectors; edge k runs from vertex k+1 to vertex k+2
  int64_t ax[3], ay[3];
  bool tl[3];
  bool empty;

  __device__ __forceinline__ void init(const Tri& t) {
    const I area2 = static_cast<I>(t.x[1] - t.x[0]) * static_cast<I>(t.y[2] - t.y[0]) -
                    static_cast<I>(t.y[1] - t.y[0]) * static_cast<I>(t.x[2] - t.x[0]);
    empty = area2 == 0;
    const bool flip = area2 < 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a = (k + 1) % 3, b = (k + 2) % 3;
      const int64_t ex = t.x[b] - t.x[a], ey = t.y[b] - t.y[a];
      dx[k] = flip ? -static_cast<I>(ex) : static_cast<I>(ex);
      dy[k] = flip ? -static_cast<I>(ey) : static_cast<I>(ey);
      ax[k] = t.x[a]; ay[k] = t.y[a];
      // y points down: dy < 0 is a left edge, dy == 0 && dx > 0 a top edge
      tl[k] = dy[k] < 0 || (dy[k] == 0 && dx[k] > 0);
    }
  }

  // true: the sample of pixel (px, py) is covered; e[k] = weight of vertex k (sum = |area2|)
  __device__ __forceinline__ bool at(int px, int py, I* e) const {
    const int64_t sx = static_cast<int64_t>(px) * SUBPIX + SUBPIX / 2;
    const int64_t sy = static_cast<int64_t>(py) * SUBPIX + SUBPIX / 2;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      e[k] = dx[k] * static_cast<I>(sy - ay[k]) - dy[k] * static_cast<I>(sx - ax[k]);
      in = in && (e[k] > 0 || (e[k] == 0 && tl[k]));
    }
    return in;
  }
};

// b_k / z_k for the three vertices and their sum (1 / depth), in fp64
template <typename I>
__device__ __forceinline__ double inv_depth(const I* e, const double* z, double* q) {
  const double s = to_f64(e[0] + e[1] + e[2]);
  q[0] = to_f64(e[0]) / s / z[0];
  q[1] = to_f64(e[1]) / s / z[1];
  q[2] = to_f64(e[2]) / s / z[2];
  return q[0] + q[1] + q[2];
}

template <typename I>
__device__ __forceinline__ void raster_pixel(const Edges<I>& ed, const Tri& t, int px, int py,
                                             uint32_t face, unsigned long long* row) {
  I e[3];
  if (!ed.at(px, py, e)) return;
  double q[3];
  const float z = static_cast<float>(1.0 / inv_depth(e, t.z, q));
  const unsigned long long key =
      (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | face;
  // the stored key only ever decreases: a plain look saves the atomic where it cannot win
  if (key < __hip_atomic_load(row + px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(row + px, key);
}

// lane_id < 0: this lane walks the whole box; otherwise the 64 lanes share it
template <typename I>
__device__ __forceinline__ void raster_tri(const Tri& t, uint32_t face,
                                           unsigned long long* img, int w, int lane_id) {
  Edges<I> ed;
  ed.init(t);
  if (ed.empty) return;
  const int bw = t.x1 - t.x0 + 1;
  const int64_t n = static_cast<int64_t>(bw) * (t.y1 - t.y0 + 1);
  const int64_t first = lane_id < 0 ? 0 : lane_id, step = lane_id < 0 ? 1 : 64;
  for (int64_t i = first; i < n; i += step) {
    const int py = t.y0 + static_cast<int>(i / bw), px = t.x0 + static_cast<int>(i % bw);
    raster_pixel(ed, t, px, py, face, img + static_cast<int64_t>(py) * w);
  }
}

__global__ __launch_bounds__(256) void fill_keys_kernel(unsigned long long* keys, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += stride)
    keys[i] = ~0ull;
}

__global__ __launch_bounds__(RASTER_THREADS) void raster_kernel(
    const double* __restrict__ verts, const int32_t* __restrict__ faces, int64_t n_verts,
    int64_t n_faces_total, const EposRenderInst* __restrict__ insts, int h, int w, double near,
    unsigned long long* keys) {
  const int inst = blockIdx.x / RASTER_BLOCKS_PER_INST;
  const int blk = blockIdx.x % RASTER_BLOCKS_PER_INST;
  const EposRenderInst in = insts[inst];
  const int nf = in.n_faces;
  const int lane = threadIdx.x & 63;
  unsigned long long* img = keys + static_cast<int64_t>(inst) * h * w;
  // the trip count is the same for every lane of the workgroup: the ballots below see all 64
  for (int64_t f0 = static_cast<int64_t>(blk) * RASTER_THREADS; f0 < nf;
       f0 += static_cast<int64_t>(RASTER_BLOCKS_PER_INST) * RASTER_THREADS) {
    const int64_t f = f0 + threadIdx.x;
    Tri t;
    t.ok = false; t.wide = false; t.x0 = t.y0 = 0; t.x1 = t.y1 = -1;
    if (f < nf) setup_tri(verts, faces, n_verts, n_faces_total, in, static_cast<int>(f), h, w,
                          near, &t);
    const int64_t box = t.ok ? static_cast<int64_t>(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
    const bool large = box > RASTER_LANE_MAX_PIXELS;
    if (box > 0 && !large) {
      if (t.wide) raster_tri<__int128>(t, static_cast<uint32_t>(f), img, w, -1);
      else raster_tri<int64_t>(t, static_cast<uint32_t>(f), img, w, -1);
    }
    uint64_t todo = __ballot(large);
    while (todo) {
      const int src = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      const int fl = static_cast<int>(f0) + (static_cast<int>(threadIdx.x) & ~63) + src;
      Tri tw;
      setup_tri(verts, faces, n_verts, n_faces_total, in, fl, h, w, near, &tw);
      if (tw.wide) raster_tri<__int128>(tw, static_cast<uint32_t>(fl), img, w, lane);
      else raster_tri<int64_t>(tw, static_cast<uint32_t>(fl), img, w, lane);
    }
  }
}

template <typename I>
__device__ __forceinline__ void weights_at(const Tri& t, int px, int py, double* q,
                                           double* den) {
  Edges<I> ed;
  ed.init(t);
  I e[3];
  ed.at(px, py, e);
  *den = inv_depth(e, t.z, q);
}

__global__ __launch_bounds__(256) void resolve_kernel(
    const unsigned long long* __restrict__ keys, const double* __restrict__ verts,
    const int32_t* __restrict__ faces, const uint8_t* __restrict__ colors, int64_t n_verts,
    int64_t n_faces_total, const EposRenderInst* __restrict__ insts, int n_inst, int h, int w,
    double near, float* depth, int32_t* face, float* local_pos, uint8_t* color) {
  const int64_t total = static_cast<int64_t>(n_inst) * h * w;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const unsigned long long key = keys[i];
  const int inst = static_cast<int>(i / (static_cast<int64_t>(h) * w));
  const int pix = static_cast<int>(i % (static_cast<int64_t>(h) * w));
  const int py = pix / w, px = pix % w;
  float d = 0.f, lp[3] = {0.f, 0.f, 0.f};
  int32_t fo = -1;
  uint8_t c[3] = {0, 0, 0};
  if (key != ~0ull) {
    const EposRenderInst in = insts[inst];
    const int f = static_cast<int>(key & 0xffffffffu);
    Tri t;
    setup_tri(verts, faces, n_verts, n_faces_total, in, f, h, w, near, &t);
    if (t.ok && f < in.n_faces) {
      d = __uint_as_float(static_cast<uint32_t>(key >> 32));
      fo = f;
      if (local_pos || color) {
        double q[3], den;
        if (t.wide) weights_at<__int128>(t, px, py, q, &den);
        else weights_at<int64_t>(t, px, py, q, &den);
        if (local_pos) {
#pragma unroll
          for (int k = 0; k < 3; ++k)
            lp[k] = static_cast<float>((q[0] * verts[3 * int64_t(t.vi[0]) + k] +
                                        q[1] * verts[3 * int64_t(t.vi[1]) + k] +
                                        q[2] * verts[3 * int64_t(t.vi[2]) + k]) / den);
        }
        if (color) {
          // headlight: ambient + diffuse * cos^2 of the angle between the camera-space face
          // normal and the optical axis (no square root: every operation is exactly rounded)
          double a[3], b[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            a[k] = t.cam[1][k] - t.cam[0][k];
            b[k] = t.cam[2][k] - t.cam[0][k];
          }
          const double nx = a[1] * b[2] - a[2] * b[1], ny = a[2] * b[0] - a[0] * b[2],
                       nz = a[0] * b[1] - a[1] * b[0];
          const double n2 = nx * nx + ny * ny + nz * nz;
          const double light = n2 > 0.0 ? SHADE_AMBIENT + SHADE_DIFFUSE * (nz * nz / n2)
                                        : SHADE_AMBIENT;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double base = (q[0] * colors[3 * int64_t(t.vi[0]) + k] +
                                 q[1] * colors[3 * int64_t(t.vi[1]) + k] +
                                 q[2] * colors[3 * int64_t(t.vi[2]) + k]) / den;
            double v = floor(base * light + 0.5);
            v = v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v;      // NaN: 255 is not taken, 0 is
            c[k] = static_cast<uint8_t>(v == v ? v : 0.0);
          }
        }
      }
    }
  }
  if (depth) depth[i] = d;
  if (face) face[i] = fo;
  if (local_pos) { local_pos[3 * i] = lp[0]; local_pos[3 * i + 1] = lp[1]; local_pos[3 * i + 2] = lp[2]; }
  if (color) { color[3 * i] = c[0]; color[3 * i + 1] = c[1]; color[3 * i + 2] = c[2]; }
}

constexpr int GT_MAX_KNN = EPOS_LOSS_MAX_KNN;     // slots per pixel, at most

// SLOTS = 1 (knn is then the constant 1: the kernel as it was before there were slots) or
// GT_MAX_KNN
template <int SLOTS>
__global__ __launch_bounds__(256) void gt_fields_kernel(
    const float* __restrict__ depth, const float* __restrict__ local_pos,
    const uint8_t* __restrict__ masks, const int32_t* __restrict__ obj_ids, int n_inst, int h,
    int w, const double* __restrict__ centers, const double* __restrict__ sizes, int num_objs,
    int num_frags, int knn_arg, int32_t* obj_label, int32_t* inst_out, int32_t* frag_label,
    float* frag_loc, float* frag_weight) {
  const int knn = SLOTS == 1 ? 1 : knn_arg;
  const int64_t hw = static_cast<int64_t>(h) * w;
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= hw) return;
  int win = -1;
  if (masks) {                       // from the last to the first: the first hit keeps the pixel
    for (int n = n_inst - 1; n >= 0; --n) {
      const int o = obj_ids[n];
      if (o >= 1 && o <= num_objs && masks[n * hw + p] && depth[n * hw + p] > 0.f) {
        win = n;
        break;
      }
    }
  } else {                           // nearest; ties to the higher index
    float best = 0.f;
    for (int n = 0; n < n_inst; ++n) {
      const int o = obj_ids[n];
      const float d = depth[n * hw + p];
      if (o >= 1 && o <= num_objs && d > 0.f && (win < 0 || d <= best)) {
        win = n;
        best = d;
      }
    }
  }
  // slot j: the j-th nearest centre, ascending distance, ties to the lower index. The arrays
  // are indexed by unrolled loops alone, so they stay in registers.
  int32_t ol = 0, fl[SLOTS];
  double bd[SLOTS];
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) { fl[j] = 0; bd[j] = INFINITY; }
  double x = 0.0, y = 0.0, z = 0.0;
  const double* c = centers;
  if (win >= 0) {
    ol = obj_ids[win];
    const float* xyz = local_pos + 3 * (win * hw + p);
    x = xyz[0]; y = xyz[1]; z = xyz[2];
    c = centers + static_cast<int64_t>(ol - 1) * num_frags * 3;
    for (int f = 0; f < num_frags; ++f) {
      const double dx = x - c[3 * f], dy = y - c[3 * f + 1], dz = z - c[3 * f + 2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      // insert in front of the first slot that is farther; from the last slot down, so a slot
      // takes its neighbour's value before that one changes
#pragma unroll
      for (int j = SLOTS - 1; j >= 0; --j) {
        if (j >= knn) continue;
        const int below = j > 0 ? j - 1 : 0;
        if (j > 0 && d2 < bd[below]) { bd[j] = bd[below]; fl[j] = fl[below]; }
        else if (d2 < bd[j]) { bd[j] = d2; fl[j] = f; }
      }
    }
  }
  if (obj_label) obj_label[p] = ol;
  if (inst_out) inst_out[p] = win;
#pragma unroll
  for (int j = 0; j < SLOTS; ++j) {
    if (j >= knn) continue;
    float loc[3] = {0.f, 0.f, 0.f}, wt = 0.f;
    if (win >= 0) {
      const double s = sizes[static_cast<int64_t>(ol - 1) * num_frags + fl[j]];
      loc[0] = static_cast<float>((x - c[3 * fl[j]]) / s);
      loc[1] = static_cast<float>((y - c[3 * fl[j] + 1]) / s);
      loc[2] = static_cast<float>((z - c[3 * fl[j] + 2]) / s);
      wt = 1.f;
    }
    const int64_t e = p * knn + j;
    if (frag_label) frag_label[e] = fl[j];
    if (frag_loc) {
      frag_loc[3 * e] = loc[0];
      frag_loc[3 * e + 1] = loc[1];
      frag_loc[3 * e + 2] = loc[2];
    }
    if (frag_weight) frag_weight[e] = wt;
  }
}

// pixels of one call (all instances): one lane per pixel in the resolve pass, so the grid stays
// below 2^23 workgroups and the lane count below 2^32
constexpr int64_t RENDER_MAX_PIXELS = int64_t(1) << 31;

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_render_lane_max_pixels(void) { return RASTER_LANE_MAX_PIXELS; }

extern "C" int epos_render_raster(const double* verts, int64_t n_verts, const int32_t* faces,
                                  int64_t n_faces, const EposRenderInst* insts, int n_inst,
                                  int h, int w, double near, uint64_t* keys, void* stream) {
  EPOS_REQUIRE(n_inst >= 0 && h >= 0 && w >= 0 && n_verts >= 0 && n_faces >= 0,
               "negative size");
  EPOS_REQUIRE(near > 0.0, "near must be > 0");
  EPOS_REQUIRE(h <= 32768 && w <= 32768 && n_inst <= (1 << 20), "image or batch too large");
  const int64_t total = static_cast<int64_t>(n_inst) * h * w;
  if (total == 0) return EPOS_OK;
  EPOS_REQUIRE(keys && insts, "null pointer");
  EPOS_REQUIRE(total < RENDER_MAX_PIXELS, "image or batch too large");
  const bool no_mesh = n_faces == 0 || n_verts == 0;
  EPOS_REQUIRE(no_mesh || (verts && faces), "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t fb = ceil_div(total, 256);
  hipLaunchKernelGGL(fill_keys_kernel, dim3(static_cast<unsigned>(fb < 4096 ? fb : 4096)),
                     dim3(256), 0, s, reinterpret_cast<unsigned long long*>(keys), total);
  int rc = launch_status("fill_keys_kernel");
  if (rc != EPOS_OK || no_mesh) return rc;
  hipLaunchKernelGGL(raster_kernel, dim3(static_cast<unsigned>(n_inst) * RASTER_BLOCKS_PER_INST),
                     dim3(RASTER_THREADS), 0, s, verts, faces, n_verts, n_faces, insts, h, w,
                     near, reinterpret_cast<unsigned long long*>(keys));
  return launch_status("raster_kernel");
}

extern "C" int epos_render_resolve(const uint64_t* keys, const double* verts, int64_t n_verts,
                                   const int32_t* faces, int64_t n_faces,
                                   const uint8_t* colors, const EposRenderInst* insts,
                                   int n_inst, int h, int w, double near, float* depth,
                                   int32_t* face, float* local_pos, uint8_t* color,
                                   void* stream) {
  EPOS_REQUIRE(n_inst >= 0 && h >= 0 && w >= 0 && n_verts >= 0 && n_faces >= 0,
               "negative size");
  EPOS_REQUIRE(near > 0.0, "near must be > 0");
  EPOS_REQUIRE(h <= 32768 && w <= 32768 && n_inst <= (1 << 20), "image or batch too large");
  const int64_t total = static_cast<int64_t>(n_inst) * h * w;
  if (total == 0) return EPOS_OK;
  EPOS_REQUIRE(total < RENDER_MAX_PIXELS, "image or batch too large");
  EPOS_REQUIRE(keys && insts && verts && faces, "null pointer");
  EPOS_REQUIRE(!color || colors, "colour output without vertex colours");
  hipLaunchKernelGGL(resolve_kernel, dim3(static_cast<unsigned>(ceil_div(total, 256))),
                     dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(keys), verts, faces, colors,
                     n_verts, n_faces, insts, n_inst, h, w, near, depth, face, local_pos,
                     color);
  return launch_status("resolve_kernel");
}

namespace {

// epos_gt_fields_knn, refusing in the name of the entry that was called
int gt_fields(const char* fn, const float* depth, const float* local_pos, const uint8_t* masks,
              const int32_t* obj_ids, int n_inst, int h, int w, const double* centers,
              const double* sizes, int num_objs, int num_frags, int knn, int32_t* obj_label,
              int32_t* instance, int32_t* frag_label, float* frag_loc, float* frag_weight,
              void* stream) {
  EPOS_REQUIRE_FN(fn, n_inst >= 0 && h >= 0 && w >= 0, "negative size");
  EPOS_REQUIRE_FN(fn, num_objs >= 1, "num_objs must be >= 1");
  EPOS_REQUIRE_FN(fn, num_frags >= 1 && num_frags <= 256, "num_frags must be in 1..256");
  EPOS_REQUIRE_FN(fn, knn >= 1 && knn <= GT_MAX_KNN && knn <= num_frags,
                  "knn must be in 1..min(num_frags, EPOS_LOSS_MAX_KNN)");
  EPOS_REQUIRE_FN(fn, h <= 32768 && w <= 32768 && n_inst <= (1 << 20), "image or batch too large");
  const int64_t hw = static_cast<int64_t>(h) * w;
  if (hw == 0) return EPOS_OK;
  EPOS_REQUIRE_FN(fn, centers && sizes, "null pointer");
  EPOS_REQUIRE_FN(fn, n_inst == 0 || (depth && local_pos && obj_ids), "null pointer");
  const dim3 grid(static_cast<unsigned>(ceil_div(hw, 256)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (knn == 1)
    hipLaunchKernelGGL(gt_fields_kernel<1>, grid, dim3(256), 0, s, depth, local_pos, masks,
                       obj_ids, n_inst, h, w, centers, sizes, num_objs, num_frags, knn,
                       obj_label, instance, frag_label, frag_loc, frag_weight);
  else
    hipLaunchKernelGGL(gt_fields_kernel<GT_MAX_KNN>, grid, dim3(256), 0, s, depth, local_pos,
                       masks, obj_ids, n_inst, h, w, centers, sizes, num_objs, num_frags, knn,
                       obj_label, instance, frag_label, frag_loc, frag_weight);
  return launch_status("gt_fields_kernel");
}

}  // namespace

extern "C" int epos_gt_fields(const float* depth, const float* local_pos, const uint8_t* masks,
                              const int32_t* obj_ids, int n_inst, int h, int w,
                              const double* centers, const double* sizes, int num_objs,
                              int num_frags, int32_t* obj_label, int32_t* instance,
                              int32_t* frag_label, float* frag_loc, float* frag_weight,
                              void* stream) {
  return gt_fields(__func__, depth, local_pos, masks, obj_ids, n_inst, h, w, centers, sizes,
                   num_objs, num_frags, 1, obj_label, instance, frag_label, frag_loc, frag_weight,
                   stream);
}

extern "C" int epos_gt_fields_knn(const float* depth, const float* local_pos,
                                  const uint8_t* masks, const int32_t* obj_ids, int n_inst, int h,
                                  int w, const double* centers, const double* sizes, int num_objs,
                                  int num_frags, int knn, int32_t* obj_label, int32_t* instance,
                                  int32_t* frag_label, float* frag_loc, float* frag_weight,
                                  void* stream) {
  return gt_fields(__func__, depth, local_pos, masks, obj_ids, n_inst, h, w, centers, sizes,
                   num_objs, num_frags, knn, obj_label, instance, frag_label, frag_loc,
                   frag_weight, stream);
}
