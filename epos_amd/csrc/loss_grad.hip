// The derivative of the three training losses with respect to the three logit tensors
// (include/epos_hip.h, "Losses"; DESIGN.md, "Losses", "Gradients"), and the reduction of the
// tables of epos_loss_terms to the batch's loss values and the per-image gradient factors.
//
//   loss_reduce_kernel  one workgroup, no floating-point atomics: a thread per image (mean) or
//                       per object (pooled) in rounds of 256, one thread adds each round's
//                       results in index order.
//   loss_grads_kernel   a workgroup owns a contiguous share of the pixels of ONE image.
//                       Phase one is the forward's (loss_rows.h, pixel_rows): the pixel's
//                       class, m and S of its two rows and where its active rows start go to
//                       LDS. Phase two streams the share's contiguous spans of d_frag and d_loc
//                       in 16-byte nontemporal stores: zeros, except for the quads that touch a
//                       foreground pixel's row (F values of share * O * F, 3 of share * O * F * 3).
//
// Every output element is written by exactly one thread from values that depend on its own
// pixel only: no atomics, the same bytes in every run and at every position of every batch.
// fp64 on the fp32 values, -ffp-contract=off (no FMA): an element's value is softmax_grad or
// huber_grad of loss_rows.h, which heads_wgrad.hip and heads_dgrad.hip call as well. With knn
// slots per pixel ("k nearest fragments") a foreground pixel has one row of F logit gradients
// (softmax_grad_knn) and knn rows of three localisation gradients; the entries without knn are
// knn = 1.
#include "loss_rows.h"

namespace epos {
namespace {

// Pixels per workgroup: a 120 x 160 head in shares of 16 is 1200 workgroups per image, 4.7 per
// CU, each with 344 KB to write at O = 21, F = 64; at F = 64 (L = 16) phase one is one pass.
// The share bounds the LDS (44 bytes per pixel) and keeps a span's element index in 32 bits:
// 64 * 4095 * 256 * 3 < 2^31.
constexpr int64_t GRAD_SHARE_MIN = 16, GRAD_SHARE_MAX = 64;
constexpr int64_t GRAD_TARGET_BLOCKS = 2048;
constexpr int NO_ROW = -1;
constexpr int REDUCE_THREADS = 256;

typedef float lg_f32x4 __attribute__((ext_vector_type(4)));

// a function of P only (never of B, O or F)
inline int64_t grad_share(int64_t P) {
  const int64_t s = round_up(ceil_div(P, GRAD_TARGET_BLOCKS), 16);
  return s < GRAD_SHARE_MIN ? GRAD_SHARE_MIN : s > GRAD_SHARE_MAX ? GRAD_SHARE_MAX : s;
}

int check_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags) {
  return check_loss_dims(fn, B, P, num_objs, num_frags, grad_share(P));
}

// P_b, n_b and the three sums of image b, objects added in index order
__device__ __forceinline__ void image_sums(const double* __restrict__ sums,
                                           const int64_t* __restrict__ counts, int64_t b, int O1,
                                           int64_t& pixels, int64_t& n_fg, double s[3]) {
  pixels = counts[b * O1 * 2 + 1];
  n_fg = 0;
  s[0] = s[1] = s[2] = 0.0;
  for (int g = 0; g < O1; ++g) {
    const int64_t c = counts[(b * O1 + g) * 2];
    pixels += c;
    s[0] += sums[(b * O1 + g) * 3];
    if (g >= 1) {
      n_fg += c;
      s[1] += sums[(b * O1 + g) * 3 + 1];
      s[2] += sums[(b * O1 + g) * 3 + 2];
    }
  }
}

template <int SLOTS>
__global__ __launch_bounds__(REDUCE_THREADS) void loss_reduce_kernel(
    const double* __restrict__ sums, const int64_t* __restrict__ counts, int B, int O1,
    double w_obj, double w_cls, double w_loc, int reduction, int knn_arg,
    double* __restrict__ values, double* __restrict__ scales) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ double part[REDUCE_THREADS][4];
  __shared__ int64_t cnt[REDUCE_THREADS][2];
  __shared__ double pooled[3];
  const int t = threadIdx.x;
  if (reduction == EPOS_LOSS_MEAN) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};          // thread 0's
    for (int b0 = 0; b0 < B; b0 += REDUCE_THREADS) {
      const int b = b0 + t;
      if (b < B) {
        int64_t pixels, n_fg;
        double s[3];
        image_sums(sums, counts, b, O1, pixels, n_fg, s);
        // the mean first, the weight last (loss.image_losses)
        part[t][0] = pixels ? w_obj * (s[0] / static_cast<double>(pixels)) : 0.0;
        // n_b * knn rows in the two fragment means
        part[t][1] = n_fg ? w_cls * (s[1] / static_cast<double>(n_fg * knn)) : 0.0;
        part[t][2] = n_fg ? w_loc * (s[2] / static_cast<double>(3 * n_fg * knn)) : 0.0;
        part[t][3] = (part[t][0] + part[t][1]) + part[t][2];
        scales[3 * b] = pixels ? w_obj / static_cast<double>(pixels * B) : 0.0;
        scales[3 * b + 1] = n_fg ? w_cls / static_cast<double>(n_fg * knn * B) : 0.0;
        scales[3 * b + 2] = n_fg ? w_loc / static_cast<double>(3 * n_fg * knn * B) : 0.0;
      }
      __syncthreads();
      if (t == 0) {
        const int n = B - b0 < REDUCE_THREADS ? B - b0 : REDUCE_THREADS;
        for (int j = 0; j < n; ++j)                // images in order
          for (int k = 0; k < 4; ++k) acc[k] += part[j][k];
      }
      __syncthreads();
    }
    if (t == 0)
      for (int k = 0; k < 4; ++k) values[k] = acc[k] / static_cast<double>(B);
    return;
  }
  // pooled: per object the images in order, then the objects in order
  double s[3] = {0.0, 0.0, 0.0};                   // thread 0's
  int64_t pixels = 0, n_fg = 0;
  for (int g0 = 0; g0 < O1; g0 += REDUCE_THREADS) {
    const int g = g0 + t;
    if (g < O1) {
      double tot[3] = {0.0, 0.0, 0.0};
      int64_t n = 0, ign = 0;
      for (int64_t b = 0; b < B; ++b) {
        for (int k = 0; k < 3; ++k) tot[k] += sums[(b * O1 + g) * 3 + k];
        n += counts[(b * O1 + g) * 2];
        if (g == 0) ign += counts[b * O1 * 2 + 1];
      }
      for (int k = 0; k < 3; ++k) part[t][k] = tot[k];
      cnt[t][0] = n;
      cnt[t][1] = ign;
    }
    __syncthreads();
    if (t == 0) {
      const int n = O1 - g0 < REDUCE_THREADS ? O1 - g0 : REDUCE_THREADS;
      for (int j = 0; j < n; ++j) {
        s[0] += part[j][0];
        pixels += cnt[j][0] + cnt[j][1];
        if (g0 + j >= 1) {
          s[1] += part[j][1];
          s[2] += part[j][2];
          n_fg += cnt[j][0];
        }
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const double v0 = pixels ? w_obj * (s[0] / static_cast<double>(pixels)) : 0.0;
    const double v1 = n_fg ? w_cls * (s[1] / static_cast<double>(n_fg * knn)) : 0.0;
    const double v2 = n_fg ? w_loc * (s[2] / static_cast<double>(3 * n_fg * knn)) : 0.0;
    values[0] = v0;
    values[1] = v1;
    values[2] = v2;
    values[3] = (v0 + v1) + v2;
    pooled[0] = pixels ? w_obj / static_cast<double>(pixels) : 0.0;
    pooled[1] = n_fg ? w_cls / static_cast<double>(n_fg * knn) : 0.0;
    pooled[2] = n_fg ? w_loc / static_cast<double>(3 * n_fg * knn) : 0.0;
  }
  __syncthreads();
  for (int64_t j = t; j < int64_t(3) * B; j += REDUCE_THREADS) scales[j] = pooled[j % 3];
}

// What phase one leaves of a share's pixels, and where each pixel's active rows start inside
// its O * F (O * F * 3) values, or NO_ROW: the `start` of fill_span. One row of F logits, one
// row of three localisation values per slot.
template <int SLOTS>
struct GradRows : ShareRows<GRAD_SHARE_MAX, SLOTS> {
  int row_frag[GRAD_SHARE_MAX], row_loc[GRAD_SHARE_MAX][SLOTS];
};

// Writes the n floats at `out`, a share's part of one output: element e belongs to pixel
// e / row of the share and is number r = e % row of it. A pixel has `ns` starts
// start[pixel * stride + j], all NO_ROW or none; the element is value(pixel, j, r - start) for
// the j with 0 <= r - start < len (the rows of a pixel do not overlap) and +0.0 everywhere else.
// Up to three scalar elements in front of the first 16-byte boundary and three behind the
// last, 16-byte nontemporal stores between: the data is written once and not read here again.
template <typename Fn>
__device__ __forceinline__ void fill_span(float* __restrict__ out, uint32_t n, uint32_t row,
                                          const int* start, int stride, int ns, int len,
                                          Fn value) {
  auto elem = [&](uint32_t i, uint32_t r) -> float {
    if (start[i * stride] == NO_ROW) return 0.f;
    for (int j = 0; j < ns; ++j) {
      const int c = static_cast<int>(r) - start[i * stride + j];
      if (c >= 0 && c < len) return value(i, j, c);
    }
    return 0.f;
  };
  uint32_t head = (4 - static_cast<uint32_t>((reinterpret_cast<uintptr_t>(out) >> 2) & 3)) & 3;
  if (head > n) head = n;
  const uint32_t quads = (n - head) / 4;
  if (threadIdx.x < 6) {
    const uint32_t e = threadIdx.x < 3 ? threadIdx.x : head + 4 * quads + (threadIdx.x - 3);
    if (threadIdx.x < 3 ? e < head : e < n) out[e] = elem(e / row, e % row);
  }
  constexpr uint32_t STEP = 4 * LOSS_THREADS;
  const uint32_t step_i = STEP / row, step_r = STEP % row;
  uint32_t e = head + 4 * threadIdx.x;
  uint32_t i = e / row, r = e % row;
  for (uint32_t q = threadIdx.x; q < quads; q += LOSS_THREADS) {
    // e + 3 < n here, so i and every pixel the quad reaches are pixels of the share
    lg_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    bool touches = r + 3 >= row;                             // crosses into the next pixel
    if (start[i * stride] != NO_ROW)
      for (int j = 0; j < ns; ++j) {
        const int st = start[i * stride + j];
        touches |= static_cast<int>(r) + 3 >= st && static_cast<int>(r) < st + len;
      }
    if (touches) {
      uint32_t ii = i, rr = r;
      float a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = elem(ii, rr);
        if (++rr == row) { rr = 0; ++ii; }
      }
      v = lg_f32x4{a[0], a[1], a[2], a[3]};
    }
    __builtin_nontemporal_store(v, reinterpret_cast<lg_f32x4*>(out + e));
    e += STEP;
    i += step_i;
    r += step_r;
    if (r >= row) { r -= row; ++i; }
  }
}

template <int SLOTS, bool VEC_OBJ, bool VEC_FRAG>
__global__ __launch_bounds__(LOSS_THREADS) void loss_grads_kernel(
    const float* __restrict__ obj_logits, int64_t ld_obj, const float* __restrict__ frag_logits,
    const float* __restrict__ frag_loc, const int32_t* __restrict__ gt_obj,
    const int32_t* __restrict__ gt_frag, const float* __restrict__ gt_loc,
    const float* __restrict__ gt_weight, int64_t P, int64_t share, int64_t blocks_per_image,
    int num_objs, int num_frags, int ignore_label, int knn_arg, int L,
    const double* __restrict__ scales, const double* __restrict__ upstream,
    float* __restrict__ d_obj, int64_t ld_dobj,
    float* __restrict__ d_frag, float* __restrict__ d_loc) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ GradRows<SLOTS> sh;
  const int64_t image = blockIdx.x / blocks_per_image;
  const int64_t p0 = (blockIdx.x % blocks_per_image) * share;
  const int64_t p1 = p0 + share < P ? p0 + share : P;
  const int n_here = static_cast<int>(p1 - p0);              // 1..GRAD_SHARE_MAX
  const int64_t pix0 = image * P + p0;                       // pixel of the whole batch
  const int O1 = num_objs + 1;
  const uint32_t OF = static_cast<uint32_t>(num_objs) * num_frags;
  const int sub = threadIdx.x % L;                           // L is a power of two <= 64
  const int per_pass = LOSS_THREADS / L;
  for (int base = 0; base < n_here; base += per_pass) {     // uniform trip count: shuffles below
    const int i = base + threadIdx.x / L;
    // nothing but d_frag needs m, S of the fragment row
    const PixelRows<SLOTS> r = pixel_rows<SLOTS, VEC_OBJ, VEC_FRAG>(
        obj_logits, ld_obj, frag_logits, gt_obj, gt_frag, gt_weight, pix0 + i, i < n_here,
        num_objs, num_frags, ignore_label, knn, d_obj != nullptr, d_frag != nullptr, sub, L);
    if (i < n_here && sub == 0) {
      sh.put(i, r, knn);
      sh.row_frag[i] = r.code > 0 ? (r.code - 1) * num_frags : NO_ROW;
#pragma unroll
      for (int j = 0; j < SLOTS; ++j)
        if (j < knn)
          sh.row_loc[i][j] = r.code > 0 ? 3 * ((r.code - 1) * num_frags + r.frag[j]) : NO_ROW;
    }
  }
  __syncthreads();
  double s[3];
  for (int k = 0; k < 3; ++k) s[k] = task_factor(scales, image, k, upstream_factor(upstream, k));

  if (d_obj) {
    for (int t = threadIdx.x; t < n_here * O1; t += LOSS_THREADS) {
      const int i = t / O1, c = t - i * O1;
      const int g = sh.code[i];
      float v = 0.f;
      if (g >= 0)
        v = softmax_grad(obj_logits[(pix0 + i) * ld_obj + c], static_cast<double>(sh.m_obj[i]),
                         sh.s_obj[i], c == g, s[0]);
      d_obj[(pix0 + i) * ld_dobj + c] = v;
    }
  }
  if (d_frag) {
    const int64_t span = pix0 * OF;
    const double kd = static_cast<double>(knn);
    fill_span(d_frag + span, static_cast<uint32_t>(n_here) * OF, OF, sh.row_frag, 1, 1, num_frags,
              [&](uint32_t i, int, int c) {
                return softmax_grad_knn(
                    frag_logits[span + static_cast<int64_t>(i) * OF + sh.row_frag[i] + c],
                    static_cast<double>(sh.m_frag[i]), sh.s_frag[i],
                    is_slot(sh.frag[i], knn, c), s[1], kd);
              });
  }
  if (d_loc) {
    const int64_t span = pix0 * OF * 3;
    fill_span(d_loc + span, static_cast<uint32_t>(n_here) * OF * 3, OF * 3, &sh.row_loc[0][0],
              SLOTS, knn, 3, [&](uint32_t i, int j, int k) {
                return huber_grad(
                    frag_loc[span + static_cast<int64_t>(i) * OF * 3 + sh.row_loc[i][j] + k],
                    gt_loc[((pix0 + i) * knn + j) * 3 + k], sh.wgt[i][j], s[2]);
              });
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

namespace {

// epos_loss_reduce_knn, refusing in the name of the entry that was called
int loss_reduce(const char* fn, const double* sums, const int64_t* counts, int B, int num_objs,
                double w_obj, double w_cls, double w_loc, int reduction, int knn, double* values,
                double* scales, void* stream) {
  EPOS_REQUIRE_FN(fn, B >= 0, "B must be >= 0");
  EPOS_REQUIRE_FN(fn, num_objs >= 1 && num_objs <= LOSS_MAX_OBJS, "num_objs must be in 1..4095");
  EPOS_REQUIRE_FN(fn, reduction == EPOS_LOSS_MEAN || reduction == EPOS_LOSS_POOLED,
               "reduction must be EPOS_LOSS_MEAN or EPOS_LOSS_POOLED");
  EPOS_REQUIRE_FN(fn, knn >= 1 && knn <= LOSS_MAX_KNN, "knn must be in 1..EPOS_LOSS_MAX_KNN");
  if (B == 0) return EPOS_OK;
  EPOS_REQUIRE_FN(fn, sums && counts && values && scales, "null pointer");
#define EPOS_REDUCE_LAUNCH(SLOTS)                                                              \
  hipLaunchKernelGGL(loss_reduce_kernel<SLOTS>, dim3(1), dim3(REDUCE_THREADS), 0,              \
                     static_cast<hipStream_t>(stream), sums, counts, B, num_objs + 1, w_obj,   \
                     w_cls, w_loc, reduction, knn, values, scales)
  EPOS_FOR_SLOTS(knn, EPOS_REDUCE_LAUNCH);
#undef EPOS_REDUCE_LAUNCH
  return launch_status("loss_reduce_kernel");
}

}  // namespace

extern "C" int epos_loss_reduce(const double* sums, const int64_t* counts, int B, int num_objs,
                                double w_obj, double w_cls, double w_loc, int reduction,
                                double* values, double* scales, void* stream) {
  return loss_reduce(__func__, sums, counts, B, num_objs, w_obj, w_cls, w_loc, reduction, 1,
                     values, scales, stream);
}

extern "C" int epos_loss_reduce_knn(const double* sums, const int64_t* counts, int B,
                                    int num_objs, double w_obj, double w_cls, double w_loc,
                                    int reduction, int knn, double* values, double* scales,
                                    void* stream) {
  return loss_reduce(__func__, sums, counts, B, num_objs, w_obj, w_cls, w_loc, reduction, knn,
                     values, scales, stream);
}

extern "C" int64_t epos_loss_grad_share_pixels(int64_t P, int num_objs, int num_frags) {
  if (check_dims(__func__, 1, P, num_objs, num_frags) != EPOS_OK) return EPOS_E_INVALID;
  return P == 0 ? 0 : grad_share(P);
}

namespace {

// epos_loss_grads_knn, refusing in the name of the entry that was called
int loss_grads(const char* fn, const float* obj_logits, int64_t ld_obj, const float* frag_logits,
               const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
               const float* gt_loc, const float* gt_weight, int B, int64_t P, int num_objs,
               int num_frags, int ignore_label, int knn, const double* scales,
               const double* upstream, float* d_obj, int64_t ld_dobj, float* d_frag,
               float* d_loc, void* stream) {
  const int rc = check_dims(fn, B, P, num_objs, num_frags);
  if (rc != EPOS_OK) return rc;
  const int rk = check_knn(fn, knn, num_frags);
  if (rk != EPOS_OK) return rk;
  EPOS_REQUIRE_FN(fn, ld_obj >= num_objs + 1, "ld_obj must be >= num_objs + 1");
  EPOS_REQUIRE_FN(fn, ld_dobj >= num_objs + 1, "ld_dobj must be >= num_objs + 1");
  if (B == 0 || P == 0) return EPOS_OK;
  EPOS_REQUIRE_FN(fn, obj_logits && frag_logits && frag_loc && gt_obj && gt_frag && gt_loc &&
               gt_weight && scales, "null pointer");
  if (!d_obj && !d_frag && !d_loc) return EPOS_OK;
  const int alias = check_no_alias(fn, {obj_logits, frag_logits, frag_loc, gt_obj, gt_frag,
                                              gt_loc, gt_weight, scales, upstream},
                                   {d_obj, d_frag, d_loc});
  if (alias != EPOS_OK) return alias;
  const int64_t share = grad_share(P);
  const int64_t per_image = ceil_div(P, share);
  const int L = loss_lanes(num_frags);            // 1..64 lanes per pixel
  // 16-byte loads where every row starts on a 16-byte boundary
  const bool vec_obj = ld_obj % 4 == 0 && reinterpret_cast<uintptr_t>(obj_logits) % 16 == 0;
  const bool vec_frag = num_frags % 4 == 0 && reinterpret_cast<uintptr_t>(frag_logits) % 16 == 0;
  const dim3 grid(static_cast<unsigned>(B * per_image));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define EPOS_GRAD_LAUNCH(SLOTS, VO, VF)                                                        \
  hipLaunchKernelGGL((loss_grads_kernel<SLOTS, VO, VF>), grid, dim3(LOSS_THREADS), 0, s,       \
                     obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,       \
                     gt_weight, P, share, per_image, num_objs, num_frags, ignore_label, knn, L, \
                     scales, upstream, d_obj, ld_dobj, d_frag, d_loc)
#define EPOS_GRAD_VEC(SLOTS)                                       \
  if (vec_obj && vec_frag) EPOS_GRAD_LAUNCH(SLOTS, true, true);    \
  else if (vec_obj) EPOS_GRAD_LAUNCH(SLOTS, true, false);          \
  else if (vec_frag) EPOS_GRAD_LAUNCH(SLOTS, false, true);         \
  else EPOS_GRAD_LAUNCH(SLOTS, false, false)
  EPOS_FOR_SLOTS(knn, EPOS_GRAD_VEC);
#undef EPOS_GRAD_VEC
#undef EPOS_GRAD_LAUNCH
  return launch_status("loss_grads_kernel");
}

}  // namespace

extern "C" int epos_loss_grads(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                               const float* frag_loc, const int32_t* gt_obj,
                               const int32_t* gt_frag, const float* gt_loc,
                               const float* gt_weight, int B, int64_t P, int num_objs,
                               int num_frags, int ignore_label, const double* scales,
                               const double* upstream, float* d_obj, int64_t ld_dobj,
                               float* d_frag, float* d_loc, void* stream) {
  return loss_grads(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                    gt_weight, B, P, num_objs, num_frags, ignore_label, 1, scales, upstream,
                    d_obj, ld_dobj, d_frag, d_loc, stream);
}

extern "C" int epos_loss_grads_knn(const float* obj_logits, int64_t ld_obj,
                                   const float* frag_logits, const float* frag_loc,
                                   const int32_t* gt_obj, const int32_t* gt_frag,
                                   const float* gt_loc, const float* gt_weight, int B, int64_t P,
                                   int num_objs, int num_frags, int ignore_label, int knn,
                                   const double* scales, const double* upstream, float* d_obj,
                                   int64_t ld_dobj, float* d_frag, float* d_loc, void* stream) {
  return loss_grads(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                    gt_weight, B, P, num_objs, num_frags, ignore_label, knn, scales, upstream,
                    d_obj, ld_dobj, d_frag, d_loc, stream);
}
