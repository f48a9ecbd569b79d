// The three training losses as per-image, per-object sums (include/epos_hip.h, "Losses";
// DESIGN.md, "Losses"): object cross-entropy, fragment cross-entropy and the fragment
// localisation Huber loss of epos_lib/loss.py:99-303, from the RAW logits of the dense heads.
//
// Two launches, no floating-point atomic anywhere:
//   loss_terms_kernel   a workgroup owns a contiguous share of the pixels of ONE image. L lanes
//                       share a pixel's row (the scheme of frag_hits_kernel, csrc/eval.hip); the
//                       pixel's three terms and its class go to LDS. Then one thread per table
//                       cell walks the share IN PIXEL ORDER and adds the terms of its class, and
//                       the workgroup writes its whole row of the workspace.
//   loss_close_kernel   one thread per output cell adds the rows of an image's workgroups in
//                       workgroup order and WRITES sums / counts / bad.
// The share depends on P alone, so an image's partial sums -- and with them its output bytes --
// are the same in every run and at every position of every batch.
//
// fp64 on the fp32 values, -ffp-contract=off (no FMA). Background, ignored and bad pixels read
// no fragment value; a foreground pixel reads its object's F logits and 3 localisation values.
// The class of a pixel, m and S of a row and the Huber term are loss_rows.h's, next to their
// derivatives. With knn slots per pixel ("k nearest fragments") the two fragment terms are the
// sums over the slots, in order, of the one-slot terms; epos_loss_terms is knn = 1.
#include "loss_rows.h"

namespace epos {
namespace {

constexpr int64_t LOSS_SHARE_MIN = 64, LOSS_SHARE_MAX = 1024;
// per image: a workgroup of a 120 x 160 head makes four passes over its 64 pixels at F = 64,
// each a chain of dependent loads, so short shares and many workgroups hide more of them
// (shares of 128: 0.098 instead of 0.055 ms at B = 1, profiles/r19/)
constexpr int64_t LOSS_TARGET_BLOCKS = 1024;
constexpr int CLOSE_DEPTH = 16;                    // partial tables whose loads are in flight

// pixels per workgroup: a function of P only (never of B)
inline int64_t loss_share(int64_t P) {
  const int64_t s = round_up(ceil_div(P, LOSS_TARGET_BLOCKS), 64);
  return s < LOSS_SHARE_MIN ? LOSS_SHARE_MIN : s > LOSS_SHARE_MAX ? LOSS_SHARE_MAX : s;
}

// 8-byte words of one workgroup's workspace row: sums f64 [O+1,3], counts i64 [O+1,2], bad
inline int64_t loss_row_words(int num_objs) { return int64_t(num_objs + 1) * 5 + 1; }

// ce = log(sum_c exp(x_c - m)) + (m - x_t) of the row the L lanes of a pixel share; every lane
// of the L takes part (inactive pixels with active = false: they read nothing), lane sub == 0
// of an active pixel holds the result. The lanes' partial sums are added in a butterfly, each
// lane's own values in index order.
template <bool VEC>
__device__ __forceinline__ double row_cross_entropy(const float* __restrict__ row, int n,
                                                    int target, bool active, int sub, int L) {
  double md, s;
  row_max_sum<VEC>(row, n, active, sub, L, md, s);
  if (!active || sub != 0) return 0.0;
  return log(s) + (md - static_cast<double>(row[target]));
}

template <int SLOTS, bool VEC_OBJ, bool VEC_FRAG>
__global__ __launch_bounds__(LOSS_THREADS) void loss_terms_kernel(
    const float* __restrict__ obj_logits, int64_t ld_obj, const float* __restrict__ frag_logits,
    const float* __restrict__ frag_loc, const int32_t* __restrict__ gt_obj,
    const int32_t* __restrict__ gt_frag, const float* __restrict__ gt_loc,
    const float* __restrict__ gt_weight, int64_t P, int64_t share, int64_t blocks_per_image,
    int num_objs, int num_frags, int ignore_label, int knn_arg, int L,
    double* __restrict__ ws) {
  const int knn = slots_of<SLOTS>(knn_arg);
  __shared__ double term[3 * LOSS_SHARE_MAX];
  __shared__ int code[LOSS_SHARE_MAX];
  const int64_t image = blockIdx.x / blocks_per_image;
  const int64_t p0 = (blockIdx.x % blocks_per_image) * share;
  const int64_t p1 = p0 + share < P ? p0 + share : P;
  const int n_here = static_cast<int>(p1 - p0);
  const int sub = threadIdx.x % L;                // L is a power of two <= 64
  const int per_pass = LOSS_THREADS / L;
  for (int base = 0; base < n_here; base += per_pass) {     // uniform trip count: shuffles below
    const int i = base + threadIdx.x / L;
    const int64_t p = image * P + p0 + i;         // pixel of the whole batch
    int g = CODE_NONE, f[SLOTS];
    float wgt[SLOTS];
    if (i < n_here)
      g = pixel_class<SLOTS>(gt_obj, gt_frag, gt_weight, p, num_objs, num_frags, ignore_label,
                             knn, f, wgt);
    const double ce_obj = row_cross_entropy<VEC_OBJ>(obj_logits + p * ld_obj, num_objs + 1, g,
                                                     g >= 0, sub, L);
    const int64_t frag_row = g > 0 ? frag_row_offset(p, num_objs, g, num_frags) : 0;
    double m_frag, s_frag;
    row_max_sum<VEC_FRAG>(frag_logits + frag_row, num_frags, g > 0, sub, L, m_frag, s_frag);
    if (i < n_here && sub == 0) {
      double ce_frag = 0.0, hub = 0.0;
      if (g > 0) {
        // the slots in order, each summand as with one slot
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
          if (j >= knn) continue;
          ce_frag += log(s_frag) + (m_frag - static_cast<double>(frag_logits[frag_row + f[j]]));
          const float* q = frag_loc + (frag_row + f[j]) * 3;
          const float* t = gt_loc + (p * knn + j) * 3;
          const double h0 = huber1(static_cast<double>(q[0]) - static_cast<double>(t[0]));
          const double h1 = huber1(static_cast<double>(q[1]) - static_cast<double>(t[1]));
          const double h2 = huber1(static_cast<double>(q[2]) - static_cast<double>(t[2]));
          hub += static_cast<double>(wgt[j]) * ((h0 + h1) + h2);
        }
      }
      code[i] = g;
      term[3 * i] = ce_obj;
      term[3 * i + 1] = ce_frag;
      term[3 * i + 2] = hub;
    }
  }
  __syncthreads();
  // one thread per cell (class, term): the share's pixels of that class, in pixel order
  double* row = ws + static_cast<int64_t>(blockIdx.x) * (int64_t(num_objs + 1) * 5 + 1);
  int64_t* cnt = reinterpret_cast<int64_t*>(row + 3 * (num_objs + 1));
  const int cells = 3 * (num_objs + 1);
  for (int cell = threadIdx.x; cell < cells; cell += LOSS_THREADS) {
    const int cls = cell / 3, k = cell - 3 * cls;
    double acc = 0.0;
    int64_t n = 0, n_ign = 0, n_bad = 0;
    for (int i = 0; i < n_here; ++i) {
      const int c = code[i];
      if (c == cls) { acc += term[3 * i + k]; ++n; }
      n_ign += c == CODE_IGNORED;
      n_bad += c == CODE_BAD;
    }
    row[cell] = acc;
    if (k == 0) {
      cnt[2 * cls] = n;
      cnt[2 * cls + 1] = cls == 0 ? n_ign : 0;
      if (cls == 0) cnt[2 * (num_objs + 1)] = n_bad;
    }
  }
}

// cell < 3 (O+1): a sum (fp64 add); the other cells are integers
__global__ __launch_bounds__(LOSS_THREADS) void loss_close_kernel(
    const double* __restrict__ ws, int64_t blocks_per_image, int num_objs,
    double* __restrict__ sums, int64_t* __restrict__ counts, int64_t* __restrict__ bad) {
  const int64_t words = int64_t(num_objs + 1) * 5 + 1;
  const int64_t cell = static_cast<int64_t>(blockIdx.x) * LOSS_THREADS + threadIdx.x;
  if (cell >= words) return;
  const int64_t image = blockIdx.y;
  const double* src = ws + image * blocks_per_image * words + cell;
  const int n_sums = 3 * (num_objs + 1);
  if (cell < n_sums) {
    // CLOSE_DEPTH loads at a time, then their additions in workgroup order: the order of the
    // sum is that of the plain loop, only the loads do not wait for one another
    double acc = 0.0;
    for (int64_t j0 = 0; j0 < blocks_per_image; j0 += CLOSE_DEPTH) {
      double v[CLOSE_DEPTH];
#pragma unroll
      for (int k = 0; k < CLOSE_DEPTH; ++k)
        v[k] = j0 + k < blocks_per_image ? src[(j0 + k) * words] : 0.0;
#pragma unroll
      for (int k = 0; k < CLOSE_DEPTH; ++k)
        if (j0 + k < blocks_per_image) acc += v[k];
    }
    sums[image * n_sums + cell] = acc;
  } else {
    const int64_t* isrc = reinterpret_cast<const int64_t*>(src);
    int64_t acc = 0;
#pragma unroll 8
    for (int64_t j = 0; j < blocks_per_image; ++j) acc += isrc[j * words];
    if (cell == words - 1) bad[image] = acc;
    else counts[image * 2 * (num_objs + 1) + (cell - n_sums)] = acc;
  }
}

int check_dims(const char* fn, int B, int64_t P, int num_objs, int num_frags) {
  return check_loss_dims(fn, B, P, num_objs, num_frags, loss_share(P));
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_loss_share_pixels(int64_t P, int num_objs, int num_frags) {
  if (check_dims(__func__, 1, P, num_objs, num_frags) != EPOS_OK) return EPOS_E_INVALID;
  return P == 0 ? 0 : loss_share(P);
}

extern "C" int64_t epos_loss_workspace_bytes(int B, int64_t P, int num_objs, int num_frags) {
  if (check_dims(__func__, B, P, num_objs, num_frags) != EPOS_OK) return EPOS_E_INVALID;
  if (B == 0 || P == 0) return 0;
  return B * ceil_div(P, loss_share(P)) * loss_row_words(num_objs) * 8;
}

namespace {

// epos_loss_terms_knn, refusing in the name of the entry that was called
int loss_terms(const char* fn, const float* obj_logits, int64_t ld_obj, const float* frag_logits,
               const float* frag_loc, const int32_t* gt_obj, const int32_t* gt_frag,
               const float* gt_loc, const float* gt_weight, int B, int64_t P, int num_objs,
               int num_frags, int ignore_label, int knn, void* workspace, double* sums,
               int64_t* counts, int64_t* bad, void* stream) {
  const int rc = check_dims(fn, B, P, num_objs, num_frags);
  if (rc != EPOS_OK) return rc;
  const int rk = check_knn(fn, knn, num_frags);
  if (rk != EPOS_OK) return rk;
  EPOS_REQUIRE_FN(fn, ld_obj >= num_objs + 1, "ld_obj must be >= num_objs + 1");
  if (B == 0 || P == 0) return EPOS_OK;
  EPOS_REQUIRE_FN(fn, obj_logits && frag_logits && frag_loc && gt_obj && gt_frag && gt_loc &&
               gt_weight && workspace && sums && counts && bad, "null pointer");
  EPOS_REQUIRE_FN(fn, reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                  "workspace must be 8-byte aligned");
  const int64_t share = loss_share(P);
  const int64_t per_image = ceil_div(P, share);
  const int L = loss_lanes(num_frags);            // 1..64 lanes per pixel
  // 16-byte loads where every row starts on a 16-byte boundary
  const bool vec_obj = ld_obj % 4 == 0 && reinterpret_cast<uintptr_t>(obj_logits) % 16 == 0;
  const bool vec_frag = num_frags % 4 == 0 && reinterpret_cast<uintptr_t>(frag_logits) % 16 == 0;
  const dim3 grid(static_cast<unsigned>(B * per_image));
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace);
#define EPOS_LOSS_LAUNCH(SLOTS, VO, VF)                                                        \
  hipLaunchKernelGGL((loss_terms_kernel<SLOTS, VO, VF>), grid, dim3(LOSS_THREADS), 0, s,       \
                     obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,       \
                     gt_weight, P, share, per_image, num_objs, num_frags, ignore_label, knn, L, \
                     ws)
#define EPOS_LOSS_VEC(SLOTS)                                       \
  if (vec_obj && vec_frag) EPOS_LOSS_LAUNCH(SLOTS, true, true);    \
  else if (vec_obj) EPOS_LOSS_LAUNCH(SLOTS, true, false);          \
  else if (vec_frag) EPOS_LOSS_LAUNCH(SLOTS, false, true);         \
  else EPOS_LOSS_LAUNCH(SLOTS, false, false)
  EPOS_FOR_SLOTS(knn, EPOS_LOSS_VEC);
#undef EPOS_LOSS_VEC
#undef EPOS_LOSS_LAUNCH
  const int st = launch_status("loss_terms_kernel");
  if (st != EPOS_OK) return st;
  const dim3 cgrid(static_cast<unsigned>(ceil_div(loss_row_words(num_objs), LOSS_THREADS)),
                   static_cast<unsigned>(B));
  hipLaunchKernelGGL(loss_close_kernel, cgrid, dim3(LOSS_THREADS), 0, s, ws, per_image, num_objs,
                     sums, counts, bad);
  return launch_status("loss_close_kernel");
}

}  // namespace

extern "C" int epos_loss_terms(const float* obj_logits, int64_t ld_obj, const float* frag_logits,
                               const float* frag_loc, const int32_t* gt_obj,
                               const int32_t* gt_frag, const float* gt_loc,
                               const float* gt_weight, int B, int64_t P, int num_objs,
                               int num_frags, int ignore_label, void* workspace, double* sums,
                               int64_t* counts, int64_t* bad, void* stream) {
  return loss_terms(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                    gt_weight, B, P, num_objs, num_frags, ignore_label, 1, workspace, sums,
                    counts, bad, stream);
}

extern "C" int epos_loss_terms_knn(const float* obj_logits, int64_t ld_obj,
                                   const float* frag_logits, const float* frag_loc,
                                   const int32_t* gt_obj, const int32_t* gt_frag,
                                   const float* gt_loc, const float* gt_weight, int B, int64_t P,
                                   int num_objs, int num_frags, int ignore_label, int knn,
                                   void* workspace, double* sums, int64_t* counts, int64_t* bad,
                                   void* stream) {
  return loss_terms(__func__, obj_logits, ld_obj, frag_logits, frag_loc, gt_obj, gt_frag, gt_loc,
                    gt_weight, B, P, num_objs, num_frags, ignore_label, knn, workspace, sums,
                    counts, bad, stream);
}
