// Softmax over rows of G <= 256 consecutive floats, in place (model.py:677-683): the dense
// rows of epos_softmax_groups_f32 and the rows of the given (image, object) slots of
// epos_softmax_slots_f32 (sparse-head mode). ONE kernel template over (row form, row
// addresser) and one rule that picks the form (softmax_launch): what a row computes depends on
// the form alone, so dense and sparse-head runs give the same bits by construction.
#include "common.h"
#include "wave.h"

namespace epos {
namespace {

// Streaming (non-temporal) or plain 16-byte accesses.
typedef float sm_f32x4 __attribute__((ext_vector_type(4)));
template <bool STREAM>
__device__ __forceinline__ float4 ld4(const float* p) {
  const sm_f32x4* q = reinterpret_cast<const sm_f32x4*>(p);
  const sm_f32x4 v = STREAM ? __builtin_nontemporal_load(q) : *q;
  return make_float4(v[0], v[1], v[2], v[3]);
}
template <bool STREAM>
__device__ __forceinline__ void st4(float* p, float4 v) {
  const sm_f32x4 o = {v.x, v.y, v.z, v.w};
  if (STREAM) __builtin_nontemporal_store(o, reinterpret_cast<sm_f32x4*>(p));
  else *reinterpret_cast<sm_f32x4*>(p) = o;
}

// ------------------------------------------------------------------ the two row functions --
// A row of 4 * LANES values held by LANES consecutive lanes x float4 (lane l of the group holds
// values 4l..4l+3): max / sum by in-lane pairs first, then the xor butterfly over the LANES
// lanes from LANES/2 down to 1. All 64 lanes must take part.
template <int LANES>
__device__ __forceinline__ float4 softmax_vec4(float4 v) {
  const float m = wave_max<LANES>(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
  v.x = expf(v.x - m); v.y = expf(v.y - m); v.z = expf(v.z - m); v.w = expf(v.w - m);
  const float s = wave_sum<LANES>((v.x + v.y) + (v.z + v.w));
  return make_float4(v.x / s, v.y / s, v.z / s, v.w / s);
}

// v[0..N) combined as a balanced tree: v0 | op(v0, v1) | op(op(v0, v1), op(v2, v3)).
template <int N, typename Op>
__device__ __forceinline__ float in_lane(const float* v, Op op) {
  if constexpr (N == 1) return v[0];
  else return op(in_lane<N / 2>(v, op), in_lane<N / 2>(v + N / 2, op));
}

// A row of G <= 64 * NV values at x, one wave: lane l owns values l + 64k, k < NV (those < G;
// a missing one is -inf for the max and 0 for the sum); max / sum in-lane first, then over
// the wave. NV = 1 is one value per lane: nothing is combined in-lane. All 64 lanes must
// take part.
template <int NV>
__device__ __forceinline__ void softmax_strided(float* x, int G, int lane) {
  float v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lane + 64 * k < G ? x[lane + 64 * k] : -INFINITY;
  const float m = wave_max(in_lane<NV>(v, [](float a, float b) { return fmaxf(a, b); }));
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lane + 64 * k < G ? expf(v[k] - m) : 0.f;
  const float s = wave_sum(in_lane<NV>(v, [](float a, float b) { return a + b; }));
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (lane + 64 * k < G) x[lane + 64 * k] = v[k] / s;
}

// ------------------------------------------------------------------------ row addressers --
// Dense rows: row r at X + r * G. The dense fragment-confidence head is 103 MB at C2 (413 MB
// with F = 256): read once, written once, re-read only sparsely by the correspondence stage --
// streaming (non-temporal) accesses in the float4 forms keep it from sweeping the Infinity
// Cache.
struct DenseRows {
  static constexpr bool STREAM = true;
  typedef int64_t Index;
  Index n;
  __device__ __forceinline__ float* at(float* X, int64_t r, int G) const { return X + r * G; }
};
// The rows of the (image, object) slots (one slot per blockIdx.y), n = P pixels each: row of
// pixel p at X + ((img * P + p) * O + obj - 1) * F. Plain accesses (the streaming forms were
// measured on the dense heads: profiles/r07/README.md).
struct SlotRows {
  static constexpr bool STREAM = false;
  typedef int Index;
  Index n;
  const EposCorrSlot* __restrict__ slots;
  int O;
  __device__ __forceinline__ float* at(float* X, int p, int F) const {
    const int img = slots[blockIdx.y].image, obj = slots[blockIdx.y].obj_id;
    return X + ((static_cast<int64_t>(img) * n + p) * O + (obj - 1)) * F;
  }
};

// The row form: VEC = 16 or 64 is softmax_vec4<VEC> on rows of G == 4 * VEC floats, 16-byte
// aligned; VEC = 0 is softmax_strided<NV> on rows of any G <= 64 * NV. Four waves per
// workgroup, one row per wave -- but VEC = 16 (G == 64, the fragment axis): FOUR rows per wave,
// a quarter of the waves and fewer shuffle levels than one value per lane. Past the last row a
// wave that owns one row leaves (wave-uniform); a lane of a wave that shares rows takes row 0
// instead, still takes part in the shuffles and stores nothing.
template <int VEC, int NV, typename Rows>
__global__ __launch_bounds__(256) void softmax_kernel(float* X, Rows rows, int G) {
  constexpr int ROWS_PER_WAVE = VEC ? 64 / VEC : 1;
  const int lane = threadIdx.x & 63;
  typedef typename Rows::Index Index;
  const Index r = (static_cast<Index>(blockIdx.x) * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE +
                  (VEC ? lane / VEC : 0);
  const bool on = r < rows.n;
  if (ROWS_PER_WAVE == 1 && !on) return;                     // wave-uniform
  if constexpr (VEC != 0) {
    float* x = rows.at(X, on ? r : 0, 4 * VEC) + (lane & (VEC - 1)) * 4;
    const float4 y = softmax_vec4<VEC>(ld4<Rows::STREAM>(x));
    if (on) st4<Rows::STREAM>(x, y);
  } else {
    softmax_strided<NV>(rows.at(X, r, G), G, lane);
  }
}

template <int VEC, int NV, typename Rows>
int launch_form(float* X, const Rows& rows, unsigned grid_y, int G, void* stream,
                const char* name) {
  const unsigned grid_x = static_cast<unsigned>(ceil_div(rows.n, VEC == 16 ? 16 : 4));
  hipLaunchKernelGGL((softmax_kernel<VEC, NV, Rows>), dim3(grid_x, grid_y), dim3(256), 0,
                     static_cast<hipStream_t>(stream), X, rows, G);
  return launch_status(name);
}

// The form for (G, alignment of the base), the same for both addressers.
template <typename Rows>
int softmax_launch(float* X, const Rows& rows, unsigned grid_y, int G, void* stream) {
#define EPOS_SM_LAUNCH(VEC, NV)                                                          \
  launch_form<VEC, NV>(X, rows, grid_y, G, stream,                                       \
                       std::is_same<Rows, DenseRows>::value                              \
                           ? "softmax_kernel<" #VEC ", " #NV ", DenseRows>"              \
                           : "softmax_kernel<" #VEC ", " #NV ", SlotRows>")
  const bool aligned = (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  if (G > 64) return G == 256 && aligned ? EPOS_SM_LAUNCH(64, 0) : EPOS_SM_LAUNCH(0, 4);
  return G == 64 && aligned ? EPOS_SM_LAUNCH(16, 0) : EPOS_SM_LAUNCH(0, 1);
#undef EPOS_SM_LAUNCH
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_softmax_groups_f32(float* X, int64_t n_groups, int G,
                                       void* stream) {
  EPOS_REQUIRE(X, "null pointer");
  EPOS_REQUIRE(G >= 1 && G <= 256, "G must be in [1, 256]");
  if (n_groups == 0) return EPOS_OK;
  return softmax_launch(X, DenseRows{n_groups}, 1, G, stream);
}

extern "C" int epos_softmax_slots_f32(float* X, const EposCorrSlot* slots, int S,
                                      int P, int O, int F, void* stream) {
  EPOS_REQUIRE(X && slots, "null pointer");
  EPOS_REQUIRE(F >= 1 && F <= 256, "F must be in [1, 256]");
  if (S == 0 || P == 0) return EPOS_OK;
  return softmax_launch(X, SlotRows{P, slots, O}, S, F, stream);
}
