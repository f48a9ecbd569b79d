// The input gradient of the three logits layers: dL/d decoder_out from the raw logits and the
// transposed weights, without ever forming the dense logit gradients (include/epos_hip.h,
// "Input gradient"; DESIGN.md, "Losses", "Input gradient").
//
//   heads_dgrad_kernel  a workgroup owns DG_SHARE consecutive pixels of ONE image. Phase one is
//                       epos_loss_grads' (loss_rows.h, pixel_rows): the pixel's class, m and S
//                       of its two rows go to LDS. Phase two is a gather-GEMV per pixel: a wave
//                       takes every fourth pixel of the share; its lanes compute the pixel's
//                       active logit gradients 64 at a time, one per lane, with the functions
//                       epos_loss_grads rounds them with (loss_rows.h, softmax_grad and
//                       huber_grad); each value is then broadcast from its lane and multiplied
//                       with its row of the transposed weights, a lane holding the fp64 sums of
//                       its own feature indices k in registers. The row is rounded and stored
//                       once, 16 bytes per lane where the layout allows.
//
// Every output row is computed by one wave from its own pixel, the weights and s_k only, one
// accumulator per (pixel, k), the active columns in the stated order: no workspace, no atomics,
// the same bytes in every run, at every position of every batch and for every alignment.
// fp64 on the fp32 values, -ffp-contract=off. With knn slots per pixel ("k nearest fragments")
// the three localisation columns of every slot follow, the slots by ascending fragment.
#include "loss_rows.h"

namespace epos {
namespace {

constexpr int64_t DG_SHARE = 16;             // pixels per workgroup, four per wave
constexpr int DG_WAVES = LOSS_THREADS / 64;

int check_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags, int K) {
  return check_heads_dims(fn, B, P, num_objs, num_frags, DG_SHARE, K);
}

// The value lane `src` holds, in every lane; src is the same in all lanes
__device__ __forceinline__ float from_lane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// A lane's feature indices: k = (lane + 64 j) * KV + i, j < J, i < KV. KV == 4 needs K % 4 == 0
// and 16-byte aligned rows, so that a quad is inside K whenever its first index is.
template <int KV, int J>
__device__ __forceinline__ void add_row(double (&acc)[J * KV], const float* __restrict__ row,
                                        int K, int lane, double dv) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = (lane + 64 * j) * KV;
    if (k >= K) continue;
    if constexpr (KV == 4) {
      const float4 w = *reinterpret_cast<const float4*>(row + k);
      acc[4 * j] += dv * static_cast<double>(w.x);
      acc[4 * j + 1] += dv * static_cast<double>(w.y);
      acc[4 * j + 2] += dv * static_cast<double>(w.z);
      acc[4 * j + 3] += dv * static_cast<double>(w.w);
    } else {
      acc[j] += dv * static_cast<double>(row[k]);
    }
  }
}

// acc += sum_{e < n} d_e * rows[e], ascending e; lane e holds d_e (n <= 64, the same in all lanes).
// One row per step: taking 4, 8 or 16 rows' loads ahead of their additions cost occupancy and
// measured 1.2, 1.4 and 1.9 times the time at C2 (profiles/r24/).
template <int KV, int J>
__device__ __forceinline__ void add_rows(double (&acc)[J * KV], const float* __restrict__ rows,
                                         int64_t ldwt, int n, int K, int lane, float dv) {
  for (int e = 0; e < n; ++e)
    add_row<KV, J>(acc, rows + e * ldwt, K, lane, static_cast<double>(from_lane(dv, e)));
}

template <int SLOTS, int KV, int J>
__global__ __launch_bounds__(LOSS_THREADS) void heads_dgrad_kernel(
    const float* __restrict__ obj_logits, int64_t ld_obj, const float* __restrict__ frag_logits,
    const float* __restrict__ frag_loc, const int32_t* __restrict__ gt_obj,
    const int32_t* __restrict__ gt_frag, const float* __restrict__ gt_loc,
    const float* __restrict__ gt_weight, int64_t P, int64_t blocks_per_image, int num_objs,
    int num_frags, int ignore_label, int knn_arg, int L, const double* __restrict__ scales,
    const double* __restrict__ upstream, const float* __restrict__ Wt_obj,
    const float* __restrict__ Wt_frag, const float* __restrict__ Wt_loc, int64_t ldwt, int K,
    const float* Y, int64_t ldy, float* dX, int64_t ldx) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ ShareRows<DG_SHARE, SLOTS> sh;
  const int64_t image = blockIdx.x / blocks_per_image;
  const int64_t p0 = (blockIdx.x % blocks_per_image) * DG_SHARE;
  const int64_t p1 = p0 + DG_SHARE < P ? p0 + DG_SHARE : P;
  const int n_here = static_cast<int>(p1 - p0);              // 1..DG_SHARE
  const int64_t pix0 = image * P + p0;                       // pixel of the whole batch
  const int O1 = num_objs + 1, F = num_frags;
  const int sub = threadIdx.x % L;                           // L is a power of two <= 64
  const int per_pass = LOSS_THREADS / L;
  for (int base = 0; base < n_here; base += per_pass) {     // uniform trip count: shuffles below
    const int i = base + threadIdx.x / L;
    const PixelRows<SLOTS> r = pixel_rows<SLOTS, false, false>(
        obj_logits, ld_obj, frag_logits, gt_obj, gt_frag, gt_weight, pix0 + i, i < n_here,
        num_objs, F, ignore_label, knn, true, true, sub, L);
    if (i < n_here && sub == 0) sh.put(i, r, knn);
  }
  __syncthreads();
  double s[3];
  for (int k = 0; k < 3; ++k) s[k] = task_factor(scales, image, k, upstream_factor(upstream, k));

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < n_here; i += DG_WAVES) {
    const int64_t p = pix0 + i;
    const int g = __builtin_amdgcn_readfirstlane(sh.code[i]);          // the wave's pixel
    double acc[J * KV];
#pragma unroll
    for (int a = 0; a < J * KV; ++a) acc[a] = 0.0;
    if (g >= 0) {
      const double m = static_cast<double>(sh.m_obj[i]), S = sh.s_obj[i];
      for (int c0 = 0; c0 < O1; c0 += 64) {                  // the object head, 64 columns a time
        const int c = c0 + lane;
        float dv = 0.f;
        if (c < O1) dv = softmax_grad(obj_logits[p * ld_obj + c], m, S, c == g, s[0]);
        add_rows<KV, J>(acc, Wt_obj + c0 * ldwt, ldwt, O1 - c0 < 64 ? O1 - c0 : 64, K, lane, dv);
      }
    }
    if (g > 0) {
      const int64_t row0 = static_cast<int64_t>(g - 1) * F;  // the pixel's row of O * F
      const int64_t frag_row = frag_row_offset(p, num_objs, g, F);
      const double m = static_cast<double>(sh.m_frag[i]), S = sh.s_frag[i];
      // one slot: its fragment in a scalar register, as before there were slots
      const int f0 = __builtin_amdgcn_readfirstlane(sh.frag[i][0]);
      for (int c0 = 0; c0 < F; c0 += 64) {                   // the fragment head
        const int c = c0 + lane;
        float dv = 0.f;
        if (c < F) {
          if constexpr (SLOTS == 1)
            dv = softmax_grad(frag_logits[frag_row + c], m, S, c == f0, s[1]);
          else
            dv = softmax_grad_knn(frag_logits[frag_row + c], m, S, is_slot(sh.frag[i], knn, c),
                                  s[1], static_cast<double>(knn));
        }
        add_rows<KV, J>(acc, Wt_frag + (row0 + c0) * ldwt, ldwt, F - c0 < 64 ? F - c0 : 64, K,
                        lane, dv);
      }
      // the three localisation values of every slot, the slots by ascending fragment (they
      // name different fragments): the columns in ascending order
      int f = -1;
      for (int a = 0; a < knn; ++a) {
        int next = F, slot = 0;
        if constexpr (SLOTS == 1) {
          next = f0;
        } else {
          for (int j = 0; j < knn; ++j) {
            const int fj = __builtin_amdgcn_readfirstlane(sh.frag[i][j]);
            if (fj > f && fj < next) { next = fj; slot = j; }
          }
        }
        f = next;
        float dv = 0.f;
        if (lane < 3)
          dv = huber_grad(frag_loc[(frag_row + f) * 3 + lane],
                          gt_loc[(p * knn + slot) * 3 + lane], sh.wgt[i][slot], s[2]);
        add_rows<KV, J>(acc, Wt_loc + (row0 + f) * 3 * ldwt, ldwt, 3, K, lane, dv);
      }
    }
    // an ignored or bad pixel: the sums are still +0.0
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int k = (lane + 64 * j) * KV;
      if (k >= K) continue;
      if constexpr (KV == 4) {
        float4 v = make_float4(static_cast<float>(acc[4 * j]), static_cast<float>(acc[4 * j + 1]),
                               static_cast<float>(acc[4 * j + 2]),
                               static_cast<float>(acc[4 * j + 3]));
        if (Y) {
          const float4 y = *reinterpret_cast<const float4*>(Y + p * ldy + k);
          if (y.x <= 0.f) v.x = 0.f;
          if (y.y <= 0.f) v.y = 0.f;
          if (y.z <= 0.f) v.z = 0.f;
          if (y.w <= 0.f) v.w = 0.f;
        }
        *reinterpret_cast<float4*>(dX + p * ldx + k) = v;
      } else {
        float v = static_cast<float>(acc[j]);
        if (Y && Y[p * ldy + k] <= 0.f) v = 0.f;
        dX[p * ldx + k] = v;
      }
    }
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

namespace {

// epos_heads_dgrad_knn_f32, refusing in the name of the entry that was called
int heads_dgrad(const char* fn, const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
                const float* gt_loc, const float* gt_weight, int B, int64_t P, int num_objs,
                int num_frags, int ignore_label, int knn, const double* scales,
                const double* upstream, const float* Wt_obj, const float* Wt_frag,
                const float* Wt_loc, int64_t ldwt, int K, const float* Y, int64_t ldy, float* dX,
                int64_t ldx, void* stream) {
  const int rc = check_dims(fn, B, P, num_objs, num_frags, K);
  if (rc != EPOS_OK) return rc;
  const int rk = check_knn(fn, knn, num_frags);
  if (rk != EPOS_OK) return rk;
  EPOS_REQUIRE_FN(fn, ldx >= K, "ldx must be >= K");
  EPOS_REQUIRE_FN(fn, ldwt >= K, "ldwt must be >= K");
  EPOS_REQUIRE_FN(fn, !Y || ldy >= K, "ldy must be >= K");
  EPOS_REQUIRE_FN(fn, ld_obj >= num_objs + 1, "ld_obj must be >= num_objs + 1");
  if (B == 0 || P == 0) return EPOS_OK;
  EPOS_REQUIRE_FN(fn, obj_logits && frag_logits && frag_loc && gt_obj && gt_frag && gt_loc &&
               gt_weight && scales && Wt_obj && Wt_frag && Wt_loc && dX, "null pointer");
  const int alias = check_no_alias(fn, {obj_logits, frag_logits, frag_loc, gt_obj, gt_frag,
                                              gt_loc, gt_weight, scales, upstream, Wt_obj, Wt_frag,
                                              Wt_loc, Y}, {dX});
  if (alias != EPOS_OK) return alias;
  const int64_t per_image = ceil_div(P, DG_SHARE);
  const int L = loss_lanes(num_frags);            // 1..64 lanes per pixel, as epos_loss_grads
  // 16 bytes per lane where every row of the weights, of Y and of dX starts on a 16-byte boundary
  const bool vec = K % 4 == 0 && ldwt % 4 == 0 && ldx % 4 == 0 && al16(Wt_obj) &&
                   al16(Wt_frag) && al16(Wt_loc) && al16(dX) && (!Y || (ldy % 4 == 0 && al16(Y)));
  const int groups = static_cast<int>(ceil_div(K, vec ? 256 : 64));   // of 64 lanes
  const dim3 grid(static_cast<unsigned>(B * per_image));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define EPOS_DGRAD_LAUNCH(SLOTS, KV, J)                                                        \
  hipLaunchKernelGGL((heads_dgrad_kernel<SLOTS, KV, J>), grid, dim3(LOSS_THREADS), 0, s,       \
                     obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,       \
                     gt_weight, P, per_image, num_objs, num_frags, ignore_label, knn, L,       \
                     scales, upstream, Wt_obj, Wt_frag, Wt_loc, ldwt, K, Y, ldy, dX, ldx)
#define EPOS_DGRAD_WIDTH(SLOTS)                           \
  if (vec) {                                              \
    if (groups <= 1) EPOS_DGRAD_LAUNCH(SLOTS, 4, 1);      \
    else if (groups <= 2) EPOS_DGRAD_LAUNCH(SLOTS, 4, 2); \
    else EPOS_DGRAD_LAUNCH(SLOTS, 4, 4);                  \
  } else {                                                \
    if (groups <= 1) EPOS_DGRAD_LAUNCH(SLOTS, 1, 1);      \
    else if (groups <= 4) EPOS_DGRAD_LAUNCH(SLOTS, 1, 4); \
    else EPOS_DGRAD_LAUNCH(SLOTS, 1, 16);                 \
  }
  EPOS_FOR_SLOTS(knn, EPOS_DGRAD_WIDTH);
#undef EPOS_DGRAD_WIDTH
#undef EPOS_DGRAD_LAUNCH
  return launch_status("heads_dgrad_kernel");
}

}  // namespace

extern "C" int epos_heads_dgrad_f32(const float* obj_logits, int64_t ld_obj,
                                    const float* frag_logits, const float* frag_loc,
                                    const int32_t* gt_obj, const int32_t* gt_frag,
                                    const float* gt_loc, const float* gt_weight, int B, int64_t P,
                                    int num_objs, int num_frags, int ignore_label,
                                    const double* scales, const double* upstream,
                                    const float* Wt_obj, const float* Wt_frag,
                                    const float* Wt_loc, int64_t ldwt, int K, const float* Y,
                                    int64_t ldy, float* dX, int64_t ldx, void* stream) {
  return heads_dgrad(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                     gt_weight, B, P, num_objs, num_frags, ignore_label, 1, scales, upstream,
                     Wt_obj, Wt_frag, Wt_loc, ldwt, K, Y, ldy, dX, ldx, stream);
}

extern "C" int epos_heads_dgrad_knn_f32(const float* obj_logits, int64_t ld_obj,
                                        const float* frag_logits, const float* frag_loc,
                                        const int32_t* gt_obj, const int32_t* gt_frag,
                                        const float* gt_loc, const float* gt_weight, int B,
                                        int64_t P, int num_objs, int num_frags, int ignore_label,
                                        int knn, const double* scales, const double* upstream,
                                        const float* Wt_obj, const float* Wt_frag,
                                        const float* Wt_loc, int64_t ldwt, int K, const float* Y,
                                        int64_t ldy, float* dX, int64_t ldx, void* stream) {
  return heads_dgrad(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                     gt_weight, B, P, num_objs, num_frags, ignore_label, knn, scales, upstream,
                     Wt_obj, Wt_frag, Wt_loc, ldwt, K, Y, ldy, dX, ldx, stream);
}
