// Device weight packer (include/epos_hip.h, "Weight update"): fp32 [K][ldw] matrices on the
// device into the three layouts the pointwise GEMMs read -- the plain fp32 tile order
// (pointwise_gemm.hip), the three-piece bf16 split (pointwise_gemm_split.hip) and the fp16
// pairs with per-column power-of-two scales (pointwise_gemm_h2.hip) -- and the zero-padded
// bias, byte for byte what the host packers write. The logits layers' trainer
// (epos_amd/heads_train.py) hands its updated weights back to a built plan through it.
//
// Two kernels, both one workgroup per (problem, tile of 128 columns):
//   pack_check_kernel  the acceptance rule of the host fp16-pair packer (finite weights, the
//                      column scale within 2^+-100, the self-check of the split) -> one status
//                      word per problem, OR-ed with integer atomics;
//   pack_write_kernel  returns at once when ANY status word of the call is set (all or
//                      nothing); otherwise walks K in steps of 16 rows: the step's 16 x 128
//                      values go through LDS once (row-wise, coalesced loads) and leave as the
//                      lane-major 16-byte fragments of every wanted layout -- each wave writes
//                      whole 1 KB pieces contiguously.
// fp32 subnormals are kept (the library is built without flush-to-zero), every piece is
// rounded as on the host (-ffp-contract=off: no product is fused).
#include "h2_scale.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_BN = 128;            // columns per tile: BN == SP_BN == H2_BN
constexpr int PK_BK = 16;             // rows per step: SP_BK == H2_BK; the plain layout pads K to 32
constexpr int PK_ROW = PK_BN + 4;     // floats per staged row
constexpr int PK_CHUNK = 32;          // problems per launch (kernel arguments: 2.5 KB)
constexpr int PK_MAX = 256;           // problems per call

typedef unsigned pk_u32x4 __attribute__((ext_vector_type(4)));

struct PackProb {
  const float* W;        // column col0 of row 0
  const float* bias;     // bias[col0]
  float* plain;
  pk_u32x4* split;
  pk_u32x4* h2;
  float* bias_pad;
  int64_t ldw;
  int K, N;
  int index;             // of the problem in the call: its status word
  int pad0;
};

struct PackChunk {
  PackProb p[PK_CHUNK];
  int tile_start[PK_CHUNK + 1];
  int count;
};

// workgroup -> (problem, column tile)
__device__ __forceinline__ int locate(const PackChunk& g, int& tn) {
  const int b = static_cast<int>(blockIdx.x);
  int i = 0;
  while (i + 1 < g.count && b >= g.tile_start[i + 1]) ++i;
  tn = b - g.tile_start[i];
  return i;
}

// max |w| of the tile's columns, as bits (a NaN or Inf is the largest), into cmax[PK_BN].
// Lane pairs share a column: rows k and k + 1 of 32 columns per wave load (two 128-byte
// lines); the pair is folded by wave_max<2>. K is even.
__device__ __forceinline__ void tile_col_max(const PackProb& p, int n0, unsigned* cmax) {
  const int t = static_cast<int>(threadIdx.x);
  const int c = t >> 1, n = n0 + c;
  unsigned m = 0;
  if (n < p.N) {
    const float* src = p.W + n + static_cast<int64_t>(t & 1) * p.ldw;
    for (int k = 0; k < p.K; k += 2)
      m = max(m, __float_as_uint(src[static_cast<int64_t>(k) * p.ldw]) & 0x7fffffffu);
  }
  m = wave_max<2>(m);
  if ((t & 1) == 0) cmax[c] = m;
  __syncthreads();
}

// The host packer's column scale 2^e from the column maximum: frexpf(cmax) = f * 2^x with f in
// [0.5, 1) gives e = 15 - x; x = E - 126 for the biased exponent E of a normal maximum (a
// subnormal one has x <= -126: refused). An all-zero column has e = 0. false = refused.
__device__ __forceinline__ bool col_scale(unsigned bits, int& e) {
  e = 0;
  if (!(__uint_as_float(bits) <= 3.0e38f)) return false;
  if (bits == 0u) return true;
  const int E = static_cast<int>(bits >> 23);
  if (E == 0) return false;
  e = 141 - E;
  return e <= 100 && e >= -100;
}
__device__ __forceinline__ float pow2f(int e) {          // -126 <= e <= 127
  return __uint_as_float(static_cast<unsigned>(e + 127) << 23);
}

// the host packer's self-check of one scaled weight: |hi + mid 2^-11 - t| <= max(2^-22 |t|, 2^-36)
__device__ __forceinline__ bool pair_ok(float w, float s) {
  if (w == 0.f) return true;
  const float t = w * s;
  const float hi = static_cast<float>(static_cast<_Float16>(t));
  const float mid = static_cast<float>(static_cast<_Float16>((t - hi) * 2048.f));
  const double err = fabs((static_cast<double>(hi) + static_cast<double>(mid) / 2048.0) -
                          static_cast<double>(t));
  const double tol = fmax(fabs(static_cast<double>(t)) * 0x1p-22, 0x1p-36);
  return err <= tol;
}

__global__ __launch_bounds__(PK_THREADS) void pack_check_kernel(PackChunk g, int32_t* status) {
  __shared__ unsigned cmax[PK_BN];
  int tn;
  const PackProb& p = g.p[locate(g, tn)];
  if (!p.h2) return;                         // never refused
  const int t = static_cast<int>(threadIdx.x);
  const int n0 = tn * PK_BN;
  tile_col_max(p, n0, cmax);
  const int c = t >> 1, n = n0 + c;
  int e;
  int bad = !col_scale(cmax[c], e);
  if (!bad && n < p.N) {
    const float s = pow2f(e);
    const float* src = p.W + n + static_cast<int64_t>(t & 1) * p.ldw;
    for (int k = 0; k < p.K; k += 2)
      bad |= !pair_ok(src[static_cast<int64_t>(k) * p.ldw], s);
  }
  if (__syncthreads_or(bad) && t == 0) atomicOr(status + p.index, 1);
}

__device__ __forceinline__ unsigned pack16(unsigned lo, unsigned hi) {
  return (lo >> 16) | (hi & 0xffff0000u);
}

__global__ __launch_bounds__(PK_THREADS) void pack_write_kernel(PackChunk g,
                                                                const int32_t* status,
                                                                int count_all) {
  __shared__ float tile[PK_BK][PK_ROW];
  __shared__ unsigned cmax[PK_BN];
  __shared__ float scale[PK_BN];
  const int t = static_cast<int>(threadIdx.x);
  // all or nothing: one refused problem anywhere in the call and nobody writes
  int refused = 0;
  for (int i = t; i < count_all; i += PK_THREADS) refused |= status[i];
  if (__syncthreads_or(refused)) return;
  int tn;
  const PackProb& p = g.p[locate(g, tn)];
  const int K = p.K, N = p.N;
  const int n0 = tn * PK_BN;
  const int64_t tiles_n = (N + PK_BN - 1) / PK_BN, npad = tiles_n * PK_BN;
  const int nks = (K + PK_BK - 1) / PK_BK;              // steps of the split / fp16-pair layouts
  const int nks_plain = (K + 31) / 32 * 2;              // the plain layout pads K to 32
  if (p.h2) {
    tile_col_max(p, n0, cmax);
    if (t < PK_BN) {
      int e;
      (void)col_scale(cmax[t], e);                      // accepted by pack_check_kernel
      scale[t] = pow2f(e);
      // the inverse scales behind the fragments, 1.0 for the padding columns
      float* inv = reinterpret_cast<float*>(p.h2 + tiles_n * nks * (PK_BK * PK_BN * 4 / 16));
      inv[n0 + t] = pow2f(-e);
    }
  }
  if (p.bias_pad && t < PK_BN) p.bias_pad[n0 + t] = n0 + t < N ? p.bias[n0 + t] : 0.f;
  const int wave = t >> 6, ln = t & 63;
  for (int ks = 0; ks < nks_plain; ++ks) {
    __syncthreads();                                    // the last step's reads; scale[]
    {
      const int c = t & (PK_BN - 1), n = n0 + c;
#pragma unroll
      for (int i = 0; i < PK_BK / 2; ++i) {
        const int r = (t >> 7) + 2 * i, k = ks * PK_BK + r;
        tile[r][c] = (k < K && n < N) ? p.W[static_cast<int64_t>(k) * p.ldw + n] : 0.f;
      }
    }
    __syncthreads();
    if (p.plain) {
      const int c = t & (PK_BN - 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ql = (t >> 7) + 2 * i;
        const float4 v = make_float4(tile[ql * 4][c], tile[ql * 4 + 1][c], tile[ql * 4 + 2][c],
                                     tile[ql * 4 + 3][c]);
        *reinterpret_cast<float4*>(p.plain + ((static_cast<int64_t>(ks) * 4 + ql) * npad +
                                              n0 + c) * 4) = v;
      }
    }
    if (ks >= nks || !(p.split || p.h2)) continue;
    // wave = block of 32 columns; a lane holds 8 consecutive k of one column
    const int c = wave * 32 + (ln & 31), kb = (ln >> 5) * 8;
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = tile[kb + j][c];
    const int64_t frag = (static_cast<int64_t>(tn) * nks + ks) * 4 + wave;
    if (p.split) {
      // w = hi + mid + lo exactly, each piece the upper 16 bits of what is left
      unsigned hb[8], mb[8], lb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        hb[j] = __float_as_uint(w[j]);
        const float r1 = w[j] - __uint_as_float(hb[j] & 0xffff0000u);
        mb[j] = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(mb[j] & 0xffff0000u);
        lb[j] = __float_as_uint(r2);
      }
      pk_u32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = pack16(hb[2 * i], hb[2 * i + 1]);
      p.split[(frag * 3 + 0) * 64 + ln] = v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = pack16(mb[2 * i], mb[2 * i + 1]);
      p.split[(frag * 3 + 1) * 64 + ln] = v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = pack16(lb[2 * i], lb[2 * i + 1]);
      p.split[(frag * 3 + 2) * 64 + ln] = v;
    }
    if (p.h2) {
      const float s = scale[c];
      pk_u32x4 hi, mid;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned h, m;
        h2_split_pair(w[2 * i], w[2 * i + 1], s, h, m);
        hi[i] = h;
        mid[i] = m;
      }
      p.h2[(frag * 2 + 0) * 64 + ln] = hi;
      p.h2[(frag * 2 + 1) * 64 + ln] = mid;
    }
  }
}

}  // namespace
}  // namespace epos

extern "C" int epos_pack_weights_device_f32(const EposWeightPackArgs* args, int count,
                                            int32_t* status, void* stream) {
  using namespace epos;
  EPOS_REQUIRE(args, "null problem table");
  EPOS_REQUIRE(count >= 0 && count <= PK_MAX, "count must be in 0..256");
  if (count == 0) return EPOS_OK;
  EPOS_REQUIRE(status, "null status");
  EPOS_REQUIRE((reinterpret_cast<uintptr_t>(status) & 3) == 0, "status must be 4-byte aligned");
  bool any_h2 = false;
  for (int i = 0; i < count; ++i) {
    const EposWeightPackArgs& a = args[i];
    EPOS_REQUIRE(a.K >= 4 && a.K <= 1024 && (a.K & 3) == 0,
                 "K must be a multiple of 4 in 4..1024");
    EPOS_REQUIRE(a.N >= 1 && a.N <= (1 << 24), "N must be in 1..2^24");
    EPOS_REQUIRE(a.col0 >= 0 && a.ldw <= (int64_t(1) << 31) && a.col0 + a.N <= a.ldw,
                 "need 0 <= col0 and col0 + N <= ldw <= 2^31");
    EPOS_REQUIRE(a.W, "null W");
    EPOS_REQUIRE(a.bias || !a.bias_pad, "bias_pad needs bias");
    EPOS_REQUIRE((reinterpret_cast<uintptr_t>(a.W) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.bias) & 3) == 0,
                 "W and bias must be 4-byte aligned");
    EPOS_REQUIRE(al16(a.plain) && al16(a.split) && al16(a.h2) &&
                     (reinterpret_cast<uintptr_t>(a.bias_pad) & 3) == 0,
                 "plain, split and h2 must be 16-byte aligned, bias_pad 4-byte aligned");
    any_h2 = any_h2 || a.h2;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = check_hip(hipMemsetAsync(status, 0, sizeof(int32_t) * count, s), "status clear");
  if (rc) return rc;
  // every check launch of the call goes in front of its first write launch
  for (int pass = any_h2 ? 0 : 1; pass < 2; ++pass)
    for (int first = 0; first < count; first += PK_CHUNK) {
      PackChunk g;
      g.count = count - first < PK_CHUNK ? count - first : PK_CHUNK;
      g.tile_start[0] = 0;
      bool h2 = false;
      for (int i = 0; i < g.count; ++i) {
        const EposWeightPackArgs& a = args[first + i];
        PackProb& p = g.p[i];
        p.W = a.W + a.col0;
        p.bias = a.bias ? a.bias + a.col0 : nullptr;
        p.plain = a.plain;
        p.split = static_cast<pk_u32x4*>(a.split);
        p.h2 = static_cast<pk_u32x4*>(a.h2);
        p.bias_pad = a.bias_pad;
        p.ldw = a.ldw;
        p.K = a.K;
        p.N = a.N;
        p.index = first + i;
        p.pad0 = 0;
        h2 = h2 || a.h2;
        g.tile_start[i + 1] = g.tile_start[i] + static_cast<int>(ceil_div(a.N, PK_BN));
      }
      for (int i = g.count; i < PK_CHUNK; ++i) {
        g.p[i] = PackProb();
        g.tile_start[i + 1] = g.tile_start[g.count];
      }
      const dim3 grid(static_cast<unsigned>(g.tile_start[g.count]));
      if (pass == 0) {
        if (!h2) continue;
        hipLaunchKernelGGL(pack_check_kernel, grid, dim3(PK_THREADS), 0, s, g, status);
        rc = launch_status("pack_check_kernel");
      } else {
        hipLaunchKernelGGL(pack_write_kernel, grid, dim3(PK_THREADS), 0, s, g, status, count);
        rc = launch_status("pack_write_kernel");
      }
      if (rc) return rc;
    }
  return EPOS_OK;
}
