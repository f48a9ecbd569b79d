// The weight and bias gradients of the three logits layers, taken from the features and the
// raw logits without ever forming the dense logit gradients, and the momentum step
// (include/epos_hip.h, "Weight gradients"; DESIGN.md, "Losses", "Weight gradients").
//
//   wgrad_rows_kernel   pixel-parallel: S of the object row and of the foreground pixel's
//                       fragment row, and m of the object row, from the function epos_loss_grads
//                       takes them with (loss_rows.h, pixel_rows), to the workspace: 20 bytes per
//                       pixel.
//   wgrad_frag_kernel   a workgroup owns (object g, a slice of ks feature indices, a pixel
//                       range) of the fragment and the localisation head. It walks its range of
//                       every image, compacts the pixels of class g with ballots, and takes them
//                       in batches:
//                       the batch's F gradient values per pixel and its feature slice go to LDS,
//                       a thread keeps the fp64 sums of (k, up to four columns) in registers; the
//                       three localisation values per pixel go to an fp64 table [F][3][ks] in LDS
//                       that one thread per (k, component, f mod FS) adds to in batch order.
//   wgrad_obj_kernel    a workgroup owns (16 feature indices, 8 columns, a pixel range) of the
//                       object head: 32 pixel lanes x 8 columns, a lane adds every 32nd pixel of
//                       the range in order, the 32 lanes are added in lane order at the end.
//
//   wgrad_close_kernel  adds the R partial slabs in range order and rounds to f32, once.
//
// The bias gradient is the row k == K of the same sums with a feature of 1.0. An image's pixels
// are cut into R fixed ranges of epos_heads_wgrad_range_pixels consecutive pixels; a workgroup
// of the two head kernels owns range r of EVERY image, in image order, and writes its fp64 sums
// to slab r of the workspace [R][K+1][N], N = O+1 + 4*O*F; small images have R = 1 and no
// slabs: the head kernels round and write the outputs themselves. Every sum is that of one
// thread, or of a fixed sequence of threads and slabs, in a fixed order -- no atomics, the same
// bytes in every run. fp64 on the fp32 values, -ffp-contract=off; the logit gradients that are
// multiplied with the features are softmax_grad and huber_grad of loss_rows.h, the functions
// epos_loss_grads writes its outputs with. With knn slots per pixel ("k nearest fragments") a
// batch holds knn (fragment, weight, three localisation gradients) per pixel; the slots of a
// pixel name different fragments, so a cell of the localisation table still takes a pixel once.
#include "loss_rows.h"

namespace epos {
namespace {

constexpr int WG_KS = 16;                    // feature indices per slice (fewer for F > 64)
constexpr int WG_BATCH = 64;                 // pixels per batch, at most
constexpr int WG_DF = 4096;                  // floats of a batch's fragment gradients
constexpr int WG_LOC = 3072;                 // doubles of the localisation table: ks * F * 3
constexpr int WG_SCAN = 4;                   // labels per thread and scan step
constexpr int WG_RING = 2048;                // >= WG_BATCH - 1 + WG_SCAN * LOSS_THREADS
constexpr int64_t WG_ROWS_PIXELS = 256;      // pixels per workgroup of wgrad_rows_kernel
constexpr int OBJ_COLS = 8, OBJ_LANES = LOSS_THREADS / OBJ_COLS, OBJ_UNROLL = 4;
constexpr int WG_MAX_RANGES = 8;             // ranges per image, at most
constexpr int64_t WG_MIN_RANGE = 1024;       // pixels per range, at least, when there are two

// N = O+1 + 4*O*F, the columns of a slab row: those of the object, the fragment and the
// localisation head
__host__ __device__ inline int64_t slab_cols(int64_t O1, int64_t OF) { return O1 + 4 * OF; }

// Ranges per image: up to 8 of at least max(1024, 8 (K+1)) pixels -- the R slabs of
// 8 (K+1) N bytes then stay below a quarter of the dense gradients' 4 P N -- and one range for
// the smallest heads (N < 10), where 20 bytes per pixel are most of the dense size already.
inline int wgrad_ranges(int64_t P, int num_objs, int num_frags, int K) {
  const int64_t N = slab_cols(num_objs + 1, int64_t(num_objs) * num_frags);
  const int64_t least = 8 * (int64_t(K) + 1) > WG_MIN_RANGE ? 8 * (int64_t(K) + 1) : WG_MIN_RANGE;
  const int64_t R = N < 10 ? 1 : P / least;
  return R < 1 ? 1 : R > WG_MAX_RANGES ? WG_MAX_RANGES : static_cast<int>(R);
}

// feature indices per slice of the fragment kernel: ks * F * 3 <= WG_LOC, and a thread's
// columns cl + (256 / ks) * j, j < 4, cover F
inline int frag_ks(int num_frags) { return num_frags <= 64 ? 16 : num_frags <= 128 ? 8 : 4; }
inline int frag_batch(int num_frags) {
  const int n = WG_DF / num_frags;
  return n < WG_BATCH ? n : WG_BATCH;
}

int check_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags, int K) {
  return check_heads_dims(fn, B, P, num_objs, num_frags, WG_ROWS_PIXELS, K);
}

// Where the sum of feature row kq (kq == K: the bias row) and column col of a head of `width`
// columns goes when there are no slabs: dW[kq, col] or db[col]; null for kq > K and for an
// output that is not asked for
__device__ __forceinline__ float* out_cell(int64_t kq, int K, float* dW, float* db,
                                           int64_t width, int64_t col) {
  if (kq < K) return dW ? dW + kq * width + col : nullptr;
  return kq == K && db ? db + col : nullptr;
}

// One finished sum: to cell [kq][n0 + col] of the workgroup's slab of N columns when there are
// slabs, else rounded to its output
__device__ __forceinline__ void store_sum(double sum, int64_t kq, int K, double* slab, int64_t N,
                                          int64_t n0, float* dW, float* db, int64_t width,
                                          int64_t col) {
  if (slab) {
    if (kq <= K) slab[kq * N + n0 + col] = sum;
  } else if (float* out = out_cell(kq, K, dW, db, width, col)) {
    *out = static_cast<float>(sum);
  }
}

template <int SLOTS>
__global__ __launch_bounds__(LOSS_THREADS) void wgrad_rows_kernel(
    const float* __restrict__ obj_logits, int64_t ld_obj, const float* __restrict__ frag_logits,
    const int32_t* __restrict__ gt_obj, const int32_t* __restrict__ gt_frag,
    const float* __restrict__ gt_weight, int64_t n_pix, int num_objs, int num_frags,
    int ignore_label, int knn_arg, int L, bool want_obj, bool want_frag, double* __restrict__ s_obj,
    double* __restrict__ s_frag, float* __restrict__ m_obj) {
  const int knn = slots_of<SLOTS>(knn_arg);
  const int sub = threadIdx.x % L;                           // L is a power of two <= 64
  const int per_pass = LOSS_THREADS / L;
  const int64_t p0 = blockIdx.x * WG_ROWS_PIXELS;
  for (int base = 0; base < WG_ROWS_PIXELS; base += per_pass) {   // uniform: shuffles below
    const int64_t p = p0 + base + threadIdx.x / L;
    const PixelRows<SLOTS> r = pixel_rows<SLOTS, false, false>(
        obj_logits, ld_obj, frag_logits, gt_obj, gt_frag, gt_weight, p, p < n_pix, num_objs,
        num_frags, ignore_label, knn, want_obj, want_frag, sub, L);
    if (p < n_pix && sub == 0) {
      if (want_obj) {
        s_obj[p] = r.s_obj;
        m_obj[p] = static_cast<float>(r.m_obj);              // m is an fp32 value
      }
      if (want_frag) s_frag[p] = r.s_frag;
    }
  }
}

template <int SLOTS>
struct FragShared {
  double loc[WG_LOC];                 // [f][component][k of the slice]
  float df[WG_DF];                    // [pixel of the batch][F]
  float a[WG_BATCH * WG_KS];          // [pixel of the batch][k of the slice]
  float dl[WG_BATCH * SLOTS * 3];     // [pixel of the batch][slot][component]
  double s_frag[WG_BATCH];
  int64_t pixel[WG_BATCH];            // pixel of the whole batch of images
  float m_frag[WG_BATCH], wgt[WG_BATCH][SLOTS];
  int frag[WG_BATCH][SLOTS];
  uint32_t ring[WG_RING];             // pixels of class g of the current image, in order
  int count[WG_SCAN][LOSS_THREADS / 64];
};

template <int SLOTS>
__global__ __launch_bounds__(LOSS_THREADS) void wgrad_frag_kernel(
    const float* __restrict__ A, int64_t lda, int K, const float* __restrict__ frag_logits,
    const float* __restrict__ frag_loc, const int32_t* __restrict__ gt_obj,
    const int32_t* __restrict__ gt_frag, const float* __restrict__ gt_loc,
    const float* __restrict__ gt_weight, int B, int64_t P, int num_objs, int num_frags,
    int ignore_label, int knn_arg, const double* __restrict__ scales,
    const double* __restrict__ upstream, const double* __restrict__ s_frag, int ks,
    int slice0, int batch, int64_t range,
    double* __restrict__ slabs, float* __restrict__ dW_frag, float* __restrict__ db_frag,
    float* __restrict__ dW_loc, float* __restrict__ db_loc) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ FragShared<SLOTS> sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = blockIdx.y + 1;                              // the object, 1..O
  const int k0 = (slice0 + blockIdx.x) * ks;                 // k == K is the bias row
  const int F = num_frags;
  const bool want_frag = dW_frag || db_frag, want_loc = dW_loc || db_loc;
  const int k = t % ks, cl = t / ks, lanes = LOSS_THREADS / ks;
  // localisation: thread (k, component, fs) adds the pixels with f % FS == fs, in batch order
  const int FS = LOSS_THREADS / (ks * 3);
  const int loc_k = t % ks, loc_c = (t / ks) % 3, loc_fs = t / (ks * 3);
  // range blockIdx.z of every image
  const int64_t r0 = blockIdx.z * range;
  const int64_t r1 = r0 + range < P ? r0 + range : P;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (want_loc)
    for (int e = t; e < ks * F * 3; e += LOSS_THREADS) sh.loc[e] = 0.0;
  const double u1 = upstream_factor(upstream, 1), u2 = upstream_factor(upstream, 2);
  const double kd = static_cast<double>(knn);
  __syncthreads();

  for (int b = 0; b < B; ++b) {
    const int64_t img = static_cast<int64_t>(b) * P;
    const double s1 = task_factor(scales, b, 1, u1), s2 = task_factor(scales, b, 2, u2);
    uint32_t head = 0, tail = 0;                             // uniform
    for (int64_t base = r0;; base += WG_SCAN * LOSS_THREADS) {
      const bool more = base < r1;
      if (more) {
        bool match[WG_SCAN];
        uint64_t mask[WG_SCAN];
#pragma unroll
        for (int j = 0; j < WG_SCAN; ++j) {
          const int64_t pp = base + j * LOSS_THREADS + t;
          match[j] = pp < r1 && pixel_class<SLOTS>(gt_obj, gt_frag, gt_weight, img + pp, num_objs,
                                                  F, ignore_label, knn) == g;
          mask[j] = __ballot(match[j]);
          if (lane == 0) sh.count[j][wave] = __popcll(mask[j]);
        }
        __syncthreads();
        uint32_t at = tail;
#pragma unroll
        for (int j = 0; j < WG_SCAN; ++j) {
          for (int w = 0; w < LOSS_THREADS / 64; ++w) {
            if (w == wave && match[j]) {
              const uint32_t pos = at + __popcll(mask[j] & ((uint64_t(1) << lane) - 1));
              sh.ring[pos % WG_RING] = static_cast<uint32_t>(base + j * LOSS_THREADS + t);
            }
            at += sh.count[j][w];
          }
        }
        tail = at;
        __syncthreads();
      }
      // whole batches; what is left of the image when its labels are through
      while (tail - head >= static_cast<uint32_t>(batch) || (!more && tail != head)) {
        const int n = tail - head < static_cast<uint32_t>(batch) ? static_cast<int>(tail - head)
                                                                  : batch;
        {                                                    // four threads per pixel: m
          const int i = t >> 2, sub = t & 3;
          const bool valid = i < n;
          int64_t p = 0;
          float m = -INFINITY;
          if (valid) {
            p = img + sh.ring[(head + i) % WG_RING];
            if (want_frag) {
              const float* row = frag_logits + frag_row_offset(p, num_objs, g, F);
              for (int c = sub; c < F; c += 4) m = fmaxf(m, row[c]);
            }
          }
          m = fmaxf(m, __shfl_xor(m, 1));
          m = fmaxf(m, __shfl_xor(m, 2));
          if (valid && sub == 0) {
            sh.pixel[i] = p;
            sh.m_frag[i] = m;
            sh.s_frag[i] = want_frag ? s_frag[p] : 0.0;
            for (int j = 0; j < knn; ++j) {
              sh.frag[i][j] = gt_frag[p * knn + j];
              sh.wgt[i][j] = gt_weight[p * knn + j];
            }
          }
        }
        __syncthreads();
        if (want_frag) {
          for (int e = t; e < n * F; e += LOSS_THREADS) {
            const int i = e / F, c = e - i * F;
            sh.df[e] = softmax_grad_knn(
                frag_logits[frag_row_offset(sh.pixel[i], num_objs, g, F) + c],
                static_cast<double>(sh.m_frag[i]), sh.s_frag[i], is_slot(sh.frag[i], knn, c), s1,
                kd);
          }
        }
        if (want_loc) {
          for (int e = t; e < n * knn * 3; e += LOSS_THREADS) {
            const int ij = e / 3, c = e - ij * 3;            // ij = i * knn + j
            const int i = ij / knn, j = ij - i * knn;
            const int64_t p = sh.pixel[i];
            sh.dl[e] = huber_grad(
                frag_loc[(frag_row_offset(p, num_objs, g, F) + sh.frag[i][j]) * 3 + c],
                gt_loc[(p * knn + j) * 3 + c], sh.wgt[i][j], s2);
          }
        }
        for (int e = t; e < n * ks; e += LOSS_THREADS) {
          const int i = e / ks, kq = k0 + (e - i * ks);
          sh.a[e] = kq < K ? A[sh.pixel[i] * lda + kq] : kq == K ? 1.f : 0.f;
        }
        __syncthreads();
        if (want_frag) {
          for (int i = 0; i < n; ++i) {
            const double av = static_cast<double>(sh.a[i * ks + k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int c = cl + lanes * j;
              if (c < F) acc[j] += av * static_cast<double>(sh.df[i * F + c]);
            }
          }
        }
        if (want_loc && loc_fs < FS) {
          // a pixel's slots name different fragments: it adds to a cell at most once
          for (int i = 0; i < n; ++i) {
            for (int j = 0; j < knn; ++j) {
              const int f = sh.frag[i][j];
              if (f % FS == loc_fs)
                sh.loc[(f * 3 + loc_c) * ks + loc_k] +=
                    static_cast<double>(sh.a[i * ks + loc_k]) *
                    static_cast<double>(sh.dl[(i * knn + j) * 3 + loc_c]);
            }
          }
        }
        __syncthreads();
        head += n;
      }
      if (!more) break;
    }
  }

  const int kq = k0 + k;
  const int64_t OF = static_cast<int64_t>(num_objs) * F;
  const int64_t N = slab_cols(num_objs + 1, OF);
  double* __restrict__ slab = slabs ? slabs + blockIdx.z * (static_cast<int64_t>(K) + 1) * N
                                    : nullptr;
  if (want_frag) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cl + lanes * j;
      if (c >= F) continue;
      store_sum(acc[j], kq, K, slab, N, num_objs + 1, dW_frag, db_frag, OF,
                static_cast<int64_t>(g - 1) * F + c);
    }
  }
  if (want_loc) {
    const int64_t OF3 = OF * 3;
    for (int e = t; e < ks * F * 3; e += LOSS_THREADS) {
      const int fc = e / ks, kk = k0 + (e - fc * ks);
      const int64_t col = static_cast<int64_t>(g - 1) * F * 3 + fc;
      // store_sum's cases written out: the sum lies in LDS and is read only where it is stored
      // (taken by value it is read for every cell; profiles/r25/)
      if (slab) {
        if (kk <= K) slab[kk * N + (num_objs + 1) + OF + col] = sh.loc[e];
      } else if (kk < K) {
        if (dW_loc) dW_loc[kk * OF3 + col] = static_cast<float>(sh.loc[e]);
      } else if (kk == K && db_loc) {
        db_loc[col] = static_cast<float>(sh.loc[e]);
      }
    }
  }
}

template <int SLOTS>
__global__ __launch_bounds__(LOSS_THREADS) void wgrad_obj_kernel(
    const float* __restrict__ A, int64_t lda, int K, const float* __restrict__ obj_logits,
    int64_t ld_obj, const int32_t* __restrict__ gt_obj, const int32_t* __restrict__ gt_frag,
    const float* __restrict__ gt_weight, int B, int64_t P, int num_objs, int num_frags,
    int ignore_label, int knn_arg, const double* __restrict__ scales,
    const double* __restrict__ upstream, const double* __restrict__ s_obj,
    const float* __restrict__ m_obj, int slice0,
    int64_t range, double* __restrict__ slabs, float* __restrict__ dW_obj,
    float* __restrict__ db_obj) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ double part[OBJ_LANES][OBJ_COLS][WG_KS];
  const int t = threadIdx.x;
  const int cc = t % OBJ_COLS, pl = t / OBJ_COLS;
  const int O1 = num_objs + 1;
  const int c = blockIdx.y * OBJ_COLS + cc;
  const int k0 = (slice0 + blockIdx.x) * WG_KS;              // k == K is the bias row
  const double u0 = upstream_factor(upstream, 0);
  // range blockIdx.z of every image
  const int64_t r0 = blockIdx.z * range;
  const int64_t r1 = r0 + range < P ? r0 + range : P;
  double acc[WG_KS];
#pragma unroll
  for (int kk = 0; kk < WG_KS; ++kk) acc[kk] = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t img = static_cast<int64_t>(b) * P;
    const double s0 = task_factor(scales, b, 0, u0);
    for (int64_t base = r0; base < r1; base += OBJ_LANES * OBJ_UNROLL) {
      int code[OBJ_UNROLL];
      float x[OBJ_UNROLL], m[OBJ_UNROLL];
      double s[OBJ_UNROLL];
      // the loads of the four pixels first: they do not wait for one another
#pragma unroll
      for (int j = 0; j < OBJ_UNROLL; ++j) {
        const int64_t pp = base + j * OBJ_LANES + pl;
        code[j] = CODE_NONE;
        x[j] = m[j] = 0.f;
        s[j] = 1.0;
        if (pp < r1 && c < O1) {
          const int64_t p = img + pp;
          code[j] = pixel_class<SLOTS>(gt_obj, gt_frag, gt_weight, p, num_objs, num_frags,
                                       ignore_label, knn);
          if (code[j] >= 0) {
            x[j] = obj_logits[p * ld_obj + c];
            m[j] = m_obj[p];
            s[j] = s_obj[p];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < OBJ_UNROLL; ++j) {
        if (code[j] < 0) continue;
        const int64_t p = img + base + j * OBJ_LANES + pl;
        const double dv = static_cast<double>(
            softmax_grad(x[j], static_cast<double>(m[j]), s[j], c == code[j], s0));
        const float* __restrict__ a = A + p * lda;
#pragma unroll
        for (int kk = 0; kk < WG_KS; ++kk) {
          const int kq = k0 + kk;
          const float av = kq < K ? a[kq] : kq == K ? 1.f : 0.f;
          acc[kk] += static_cast<double>(av) * dv;
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < WG_KS; ++kk) part[pl][cc][kk] = acc[kk];
  __syncthreads();
  if (t < OBJ_COLS * WG_KS) {
    const int oc = t / WG_KS, kk = t % WG_KS;
    const int col = blockIdx.y * OBJ_COLS + oc, kq = k0 + kk;
    double sum = 0.0;
    for (int l = 0; l < OBJ_LANES; ++l) sum += part[l][oc][kk];       // lanes in order
    if (col < O1) {
      const int64_t N = slab_cols(O1, int64_t(num_objs) * num_frags);
      double* slab = slabs ? slabs + blockIdx.z * (static_cast<int64_t>(K) + 1) * N : nullptr;
      store_sum(sum, kq, K, slab, N, 0, dW_obj, db_obj, O1, col);
    }
  }
}

// out[k,n] = fl32(sum_r slab[r][k][n]), the ranges in order from 0.0; the columns of a row are
// those of the object, the fragment and the localisation head, the row k == K is the bias
__global__ __launch_bounds__(LOSS_THREADS) void wgrad_close_kernel(
    const double* __restrict__ slabs, int R, int K, int O1, int64_t OF,
    float* __restrict__ dW_obj, float* __restrict__ db_obj, float* __restrict__ dW_frag,
    float* __restrict__ db_frag, float* __restrict__ dW_loc, float* __restrict__ db_loc) {
  const int64_t N = slab_cols(O1, OF);
  const int64_t e = static_cast<int64_t>(blockIdx.x) * LOSS_THREADS + threadIdx.x;
  if (e >= (static_cast<int64_t>(K) + 1) * N) return;
  const int64_t k = e / N, n = e - k * N;
  float* dW;
  float* db;
  int64_t col, width;
  if (n < O1) { dW = dW_obj; db = db_obj; col = n; width = O1; }
  else if (n < O1 + OF) { dW = dW_frag; db = db_frag; col = n - O1; width = OF; }
  else { dW = dW_loc; db = db_loc; col = n - O1 - OF; width = 3 * OF; }
  float* out = out_cell(k, K, dW, db, width, col);
  if (!out) return;                               // not asked for: its slab columns hold nothing
  double sum = 0.0;
  for (int r = 0; r < R; ++r) sum += slabs[(r * (static_cast<int64_t>(K) + 1)) * N + e];
  *out = static_cast<float>(sum);
}

// One update, each operation rounded once (-ffp-contract=off: no FMA)
__device__ __forceinline__ void momentum_update(float& w, float& a, float grad, float lr,
                                                float momentum, float weight_decay,
                                                float grad_mult) {
  const float g = grad_mult * (grad + weight_decay * w);
  a = momentum * a + g;
  w = w - lr * a;
}

// `head` scalar elements in front of the 16-byte body of `quads` float4, `tail` behind it
__global__ __launch_bounds__(LOSS_THREADS) void momentum_step_kernel(
    float* __restrict__ w, float* __restrict__ accum, const float* __restrict__ grad, int64_t n,
    int head, int64_t quads, float lr, float momentum, float weight_decay, float grad_mult) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * LOSS_THREADS + threadIdx.x;
  if (i < quads) {
    const int64_t e = head + 4 * i;
    float4 wv = *reinterpret_cast<const float4*>(w + e);
    float4 av = *reinterpret_cast<const float4*>(accum + e);
    const float4 gv = *reinterpret_cast<const float4*>(grad + e);
    momentum_update(wv.x, av.x, gv.x, lr, momentum, weight_decay, grad_mult);
    momentum_update(wv.y, av.y, gv.y, lr, momentum, weight_decay, grad_mult);
    momentum_update(wv.z, av.z, gv.z, lr, momentum, weight_decay, grad_mult);
    momentum_update(wv.w, av.w, gv.w, lr, momentum, weight_decay, grad_mult);
    *reinterpret_cast<float4*>(w + e) = wv;
    *reinterpret_cast<float4*>(accum + e) = av;
  }
  const int64_t body_end = head + 4 * quads;
  if (i < head) momentum_update(w[i], accum[i], grad[i], lr, momentum, weight_decay, grad_mult);
  if (i < n - body_end)
    momentum_update(w[body_end + i], accum[body_end + i], grad[body_end + i], lr, momentum,
                    weight_decay, grad_mult);
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_heads_wgrad_range_pixels(int64_t P, int num_objs, int num_frags, int K) {
  if (check_dims(__func__, 1, P, num_objs, num_frags, K) != EPOS_OK) return EPOS_E_INVALID;
  return ceil_div(P, wgrad_ranges(P, num_objs, num_frags, K));
}

extern "C" int64_t epos_heads_wgrad_workspace_bytes(int B, int64_t P, int num_objs,
                                                    int num_frags, int K) {
  if (check_dims(__func__, B, P, num_objs, num_frags, K) != EPOS_OK) return EPOS_E_INVALID;
  const int R = wgrad_ranges(P, num_objs, num_frags, K);
  const int64_t N = slab_cols(num_objs + 1, int64_t(num_objs) * num_frags);
  return 20 * (static_cast<int64_t>(B) * P) + (R > 1 ? R * 8 * (int64_t(K) + 1) * N : 0);
}

namespace {

// epos_heads_wgrad_knn_f32, refusing in the name of the entry that was called
int heads_wgrad(const char* fn, const float* A, int64_t lda, int K, const float* obj_logits,
                int64_t ld_obj, const float* frag_logits, const float* frag_loc,
                const int32_t* gt_obj, const int32_t* gt_frag, const float* gt_loc,
                const float* gt_weight, int B, int64_t P, int num_objs, int num_frags,
                int ignore_label, int knn, const double* scales, const double* upstream,
                void* workspace, float* dW_obj, float* db_obj, float* dW_frag, float* db_frag,
                float* dW_loc, float* db_loc, void* stream) {
  const int rc = check_dims(fn, B, P, num_objs, num_frags, K);
  if (rc != EPOS_OK) return rc;
  const int rk = check_knn(fn, knn, num_frags);
  if (rk != EPOS_OK) return rk;
  EPOS_REQUIRE_FN(fn, lda >= K, "lda must be >= K");
  EPOS_REQUIRE_FN(fn, ld_obj >= num_objs + 1, "ld_obj must be >= num_objs + 1");
  const bool want_obj = dW_obj || db_obj, want_frag = dW_frag || db_frag,
             want_loc = dW_loc || db_loc;
  if (!want_obj && !want_frag && !want_loc) return EPOS_OK;
  const int64_t n_pix = static_cast<int64_t>(B) * P;
  if (n_pix > 0) {
    EPOS_REQUIRE_FN(fn, A && obj_logits && frag_logits && frag_loc && gt_obj && gt_frag && gt_loc &&
                 gt_weight && scales && workspace, "null pointer");
    EPOS_REQUIRE_FN(fn, reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                 "workspace must be 8-byte aligned");
  }
  const int alias = check_no_alias(fn, {A, obj_logits, frag_logits, frag_loc, gt_obj, gt_frag,
                                              gt_loc, gt_weight, scales, upstream, workspace},
                                   {dW_obj, db_obj, dW_frag, db_frag, dW_loc, db_loc});
  if (alias != EPOS_OK) return alias;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_pix == 0) B = 0;                          // no pixel: the kernels write zeros
  // workspace: the R slabs f64 [R][K+1][N] when R > 1, S of the object rows f64 [B*P], S of the
  // fragment rows f64 [B*P], m of the object rows f32 [B*P]
  const int R = B ? wgrad_ranges(P, num_objs, num_frags, K) : 1;
  const int64_t range = ceil_div(P, R);
  const int64_t OF = static_cast<int64_t>(num_objs) * num_frags;
  const int64_t cells = (int64_t(K) + 1) * slab_cols(num_objs + 1, OF);      // of a slab
  double* slabs = R > 1 ? static_cast<double*>(workspace) : nullptr;
  double* s_obj = static_cast<double*>(workspace);
  if (slabs) s_obj += R * cells;
  double* s_frag = s_obj ? s_obj + n_pix : nullptr;
  float* m_obj = s_obj ? reinterpret_cast<float*>(s_frag + n_pix) : nullptr;
  if (n_pix > 0 && (want_obj || want_frag)) {
    const dim3 grid(static_cast<unsigned>(ceil_div(n_pix, WG_ROWS_PIXELS)));
#define EPOS_WGRAD_ROWS(SLOTS)                                                                 \
  hipLaunchKernelGGL(wgrad_rows_kernel<SLOTS>, grid, dim3(LOSS_THREADS), 0, s, obj_logits,     \
                     ld_obj, frag_logits, gt_obj, gt_frag, gt_weight, n_pix, num_objs,         \
                     num_frags, ignore_label, knn, loss_lanes(num_frags), want_obj, want_frag, \
                     s_obj, s_frag, m_obj)
    EPOS_FOR_SLOTS(knn, EPOS_WGRAD_ROWS);
#undef EPOS_WGRAD_ROWS
    const int st = launch_status("wgrad_rows_kernel");
    if (st != EPOS_OK) return st;
  }
  if (want_obj) {
    // without dW only the slice that holds the bias row k == K
    const int slices = static_cast<int>(ceil_div(K + 1, WG_KS));
    const int slice0 = dW_obj ? 0 : K / WG_KS;
    const dim3 grid(slices - slice0, static_cast<unsigned>(ceil_div(num_objs + 1, OBJ_COLS)), R);
#define EPOS_WGRAD_OBJ(SLOTS)                                                                  \
  hipLaunchKernelGGL(wgrad_obj_kernel<SLOTS>, grid, dim3(LOSS_THREADS), 0, s, A, lda, K,       \
                     obj_logits, ld_obj, gt_obj, gt_frag, gt_weight, B, P, num_objs,           \
                     num_frags, ignore_label, knn, scales, upstream, s_obj, m_obj, slice0,     \
                     range, slabs, dW_obj, db_obj)
    EPOS_FOR_SLOTS(knn, EPOS_WGRAD_OBJ);
#undef EPOS_WGRAD_OBJ
    const int st = launch_status("wgrad_obj_kernel");
    if (st != EPOS_OK) return st;
  }
  if (want_frag || want_loc) {
    const int ks = frag_ks(num_frags);
    const int slices = static_cast<int>(ceil_div(K + 1, ks));
    const int slice0 = (dW_frag || dW_loc) ? 0 : K / ks;
    const dim3 grid(slices - slice0, num_objs, R);
#define EPOS_WGRAD_FRAG(SLOTS)                                                                 \
  hipLaunchKernelGGL(wgrad_frag_kernel<SLOTS>, grid, dim3(LOSS_THREADS), 0, s, A, lda, K,      \
                     frag_logits, frag_loc, gt_obj, gt_frag, gt_loc, gt_weight, B, P,          \
                     num_objs, num_frags, ignore_label, knn, scales, upstream, s_frag, ks,     \
                     slice0, frag_batch(num_frags), range, slabs, dW_frag, db_frag, dW_loc,    \
                     db_loc)
    EPOS_FOR_SLOTS(knn, EPOS_WGRAD_FRAG);
#undef EPOS_WGRAD_FRAG
    const int st = launch_status("wgrad_frag_kernel");
    if (st != EPOS_OK) return st;
  }
  if (slabs) {
    hipLaunchKernelGGL(wgrad_close_kernel, dim3(static_cast<unsigned>(ceil_div(cells,
                       LOSS_THREADS))), dim3(LOSS_THREADS), 0, s, slabs, R, K, num_objs + 1, OF,
                       dW_obj, db_obj, dW_frag, db_frag, dW_loc, db_loc);
    const int st = launch_status("wgrad_close_kernel");
    if (st != EPOS_OK) return st;
  }
  return EPOS_OK;
}

}  // namespace

extern "C" int epos_heads_wgrad_f32(const float* A, int64_t lda, int K, const float* obj_logits,
                                    int64_t ld_obj, const float* frag_logits,
                                    const float* frag_loc, const int32_t* gt_obj,
                                    const int32_t* gt_frag, const float* gt_loc,
                                    const float* gt_weight, int B, int64_t P, int num_objs,
                                    int num_frags, int ignore_label, const double* scales,
                                    const double* upstream, void* workspace, float* dW_obj,
                                    float* db_obj, float* dW_frag, float* db_frag, float* dW_loc,
                                    float* db_loc, void* stream) {
  return heads_wgrad(__func__, A, lda, K, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj,
                     gt_frag, gt_loc, gt_weight, B, P, num_objs, num_frags, ignore_label, 1,
                     scales, upstream, workspace, dW_obj, db_obj, dW_frag, db_frag, dW_loc,
                     db_loc, stream);
}

extern "C" int epos_heads_wgrad_knn_f32(const float* A, int64_t lda, int K,
                                        const float* obj_logits, int64_t ld_obj,
                                        const float* frag_logits, const float* frag_loc,
                                        const int32_t* gt_obj, const int32_t* gt_frag,
                                        const float* gt_loc, const float* gt_weight, int B,
                                        int64_t P, int num_objs, int num_frags, int ignore_label,
                                        int knn, const double* scales, const double* upstream,
                                        void* workspace, float* dW_obj, float* db_obj,
                                        float* dW_frag, float* db_frag, float* dW_loc,
                                        float* db_loc, void* stream) {
  return heads_wgrad(__func__, A, lda, K, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj,
                     gt_frag, gt_loc, gt_weight, B, P, num_objs, num_frags, ignore_label, knn,
                     scales, upstream, workspace, dW_obj, db_obj, dW_frag, db_frag, dW_loc,
                     db_loc, stream);
}

extern "C" int epos_momentum_step_f32(float* w, float* accum, const float* grad, int64_t n,
                                      float lr, float momentum, float weight_decay,
                                      float grad_mult, void* stream) {
  EPOS_REQUIRE(n >= 0, "n must be >= 0");
  if (n == 0) return EPOS_OK;
  EPOS_REQUIRE(w && accum && grad, "null pointer");
  EPOS_REQUIRE(n <= (int64_t(1) << 38), "n must be <= 2^38");
  const uintptr_t aw = reinterpret_cast<uintptr_t>(w), aa = reinterpret_cast<uintptr_t>(accum),
                  ag = reinterpret_cast<uintptr_t>(grad);
  EPOS_REQUIRE(aw % 4 == 0 && aa % 4 == 0 && ag % 4 == 0, "pointers must be 4-byte aligned");
  // a 16-byte body where the three arrays reach a 16-byte boundary together; else all scalar
  int head = 0;
  int64_t quads = 0;
  if (aw % 16 == aa % 16 && aw % 16 == ag % 16) {
    head = static_cast<int>((4 - (aw >> 2 & 3)) & 3);
    if (head > n) head = static_cast<int>(n);
    quads = (n - head) / 4;
  }
  const int64_t tail = n - head - 4 * quads;
  int64_t items = quads > tail ? quads : tail;
  if (items < head) items = head;
  const dim3 grid(static_cast<unsigned>(ceil_div(items, LOSS_THREADS)));
  hipLaunchKernelGGL(momentum_step_kernel, grid, dim3(LOSS_THREADS), 0,
                     static_cast<hipStream_t>(stream), w, accum, grad, n, head, quads, lr,
                     momentum, weight_decay, grad_mult);
  return launch_status("momentum_step_kernel");
}
