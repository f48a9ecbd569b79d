// Kernels of the bf16 inference mode (EposNet(precision='bf16'), include/epos_hip.h):
// bf16 activations, bf16 x bf16 products on the matrix cores (v_mfma_f32_32x32x16_bf16) with
// fp32 accumulation, fp32 epilogues, one round-to-nearest-even per stored value.
//
//   * pointwise GEMM (grouped, 1..8 problems per launch): the 1x1 convs, the dense convs after
//     epos_im2col_bf16, the logits;
//   * depthwise 3x3, im2col, global mean (bilinear resize, max-pool, subsample, add + ReLU:
//     glue.hip; the bf16 conversions and 16-byte packs: nhwc.h).
#include <stdlib.h>

#include "nhwc.h"

namespace epos {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// Pointwise GEMM. The product is computed transposed, C^T = W^T A^T, so that the MFMA's
// accumulator gives a lane one output ROW m (its column, lane & 31) and runs of four
// consecutive output channels n in its registers: the epilogue stores 8 (bf16) or 16 (fp32)
// bytes at a time with no transpose. Fragments (v_mfma_f32_32x32x16_bf16):
//   MFMA A operand (32 rows i = n, 16 k): lane (r, h) holds W[k0 + 8h + j][n0 + r], j < 8 --
//     8 consecutive k of one column, contiguous in the packed layout [k/8][Npad][8];
//   MFMA B operand (16 k, 32 cols j = m): lane (r, h) holds A[row(m0 + r)][k0 + 8h + j] --
//     8 consecutive elements of an activation row.
// Workgroup = 4 waves = a 128 (n) x 128 (m) tile; wave (wn, wm) owns 64 x 64 = 2 x 2 MFMA tiles.
// Staging as in the fp16-pair kernel: every 32-deep K step of the workgroup's A rows (128 x 64 B)
// and W columns (4 x 128 x 16 B) comes in by LDS-DMA (global_load_lds_dwordx4, 8 + 8 wave
// instructions, 2 + 2 per wave) into one of two LDS buffers while the MFMAs run on the other;
// every A row and W column is fetched once per workgroup and shared by its waves. The K tail
// (K % 32 in {8, 16, 24}): the 16-byte pieces of A at and past K are taken from a zero piece of
// the packed weights (W is zero-padded to a multiple of 32 in K), so the columns of A at and
// past K are never read.
// ---------------------------------------------------------------------------
constexpr int G_BN = 128, G_BM = 128, G_BK = 32, G_MAXP = 8;
constexpr int G_TILE = G_BM * G_BK;           // bf16 elements per staged A (or W) tile: 8 KB

struct GemmGroup {
  EposPointwiseBf16Args p[G_MAXP];
  int tile_start[G_MAXP + 1];
  int tiles_n[G_MAXP];
  int npad[G_MAXP];
  int count;
};

typedef __attribute__((address_space(3))) void lds_void;

// one wave instruction: 64 lanes x 16 bytes -> LDS [dst, dst + 1024), lane-linear
__device__ __forceinline__ void glds16(const uint16_t* src, uint16_t* dst) {
  __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src),
                                   (lds_void*)(dst), 16, 0, 0);
}

__device__ __forceinline__ void mma_step(f32x16 (&acc)[2][2], const bf16x8& w0,
                                         const bf16x8& w1, const bf16x8& a0,
                                         const bf16x8& a1) {
  acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, a0, acc[0][0], 0, 0, 0);
  acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, a1, acc[0][1], 0, 0, 0);
  acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, a0, acc[1][0], 0, 0, 0);
  acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, a1, acc[1][1], 0, 0, 0);
}

__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmGroup g) {
  // [buffer][A | W][G_TILE]: A as [row 0..127][4 pieces of 8 k], W as [k/8 0..3][n 0..127][8]
  __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][G_TILE];
  // XCD-aware order: workgroup i runs on XCD i % 8; the bijective remap gives each XCD a
  // contiguous run of tiles, so the column tiles of one row block (same A rows) share an L2
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int q = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int bid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + orig / 8;
  int pi = 0;
  while (pi + 1 < g.count && bid >= g.tile_start[pi + 1]) ++pi;
  const EposPointwiseBf16Args& p = g.p[pi];
  const int t = bid - g.tile_start[pi];
  const int tn = t % g.tiles_n[pi], tm = t / g.tiles_n[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int M = p.M, N = p.N, K = p.K;
  const int nb = tn * G_BN, mb = tm * G_BM;
  const int n0 = nb + (wave & 1) * 64;
  const int m0 = mb + (wave >> 1) * 64;
  // a wave whose whole sub-tile lies past M or N still stages and meets every barrier
  const bool active = n0 < N && m0 < M;
  const int64_t npad = g.npad[pi];
  const int64_t ws8 = npad * 8;                 // elements per k/8 group of the packed W
  const int k32 = (K + G_BK - 1) / G_BK * G_BK;
  const uint16_t* zero = p.Wp + static_cast<int64_t>(k32 / 8 - 1) * ws8;   // used iff K % 32
  // this lane's staging pieces: A rows (mb + 16 qa + lane / 4), piece lane % 4, for qa =
  // 2 wave + {0, 1}; W group qw / 2, columns nb + 64 (qw % 2) + lane, for qw = 2 wave + {0, 1}
  const int piece = lane & 3;
  const uint16_t* asrc[2];
  const uint16_t* wsrc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qa = 2 * wave + u;
    int m = mb + 16 * qa + (lane >> 2);
    m = m < M ? m : M - 1;                      // rows past M: staged, computed, never stored
    int64_t row = m;
    if (p.sub > 1) {
      const int hw = p.Ho * p.Wo;
      const int b = m / hw, rem = m - b * hw;
      const int y = rem / p.Wo, x = rem - y * p.Wo;
      row = (static_cast<int64_t>(b) * p.Hi + static_cast<int64_t>(y) * p.sub) * p.Wi +
            static_cast<int64_t>(x) * p.sub;
    }
    asrc[u] = p.A + row * p.lda + piece * 8;
    wsrc[u] = p.Wp + (static_cast<int64_t>(qa >> 1) * npad + nb + 64 * (qa & 1) + lane) * 8;
  }
  auto stage = [&](int k0, int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int qa = 2 * wave + u;
      const uint16_t* a = k0 + piece * 8 < K ? asrc[u] + k0 : zero;
      glds16(a, &lds[buf][0][qa * 512]);
      glds16(wsrc[u] + static_cast<int64_t>(k0 / 8) * ws8, &lds[buf][1][qa * 512]);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;

  const int arow0 = (wave >> 1) * 64 + r;       // this lane's A rows in the tile: + 32 i
  const int wcol0 = (wave & 1) * 64 + r;        // its W columns: + 32 j
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int k0 = 0, buf = 0; k0 < k32; k0 += G_BK, buf ^= 1) {
    if (k0 + G_BK < k32) stage(k0 + G_BK, buf ^ 1);
    if (active) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int pc = 2 * s + h;                 // the 8-k piece of this lane in k16 step s
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&lds[buf][0][(arow0 * 4 + pc) * 8]);
        const bf16x8 a1 =
            *reinterpret_cast<const bf16x8*>(&lds[buf][0][((arow0 + 32) * 4 + pc) * 8]);
        const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(&lds[buf][1][(pc * 128 + wcol0) * 8]);
        const bf16x8 w1 =
            *reinterpret_cast<const bf16x8*>(&lds[buf][1][(pc * 128 + wcol0 + 32) * 8]);
        mma_step(acc, w0, w1, a0, a1);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;

  // ---- epilogue: acc[j][i][4g + q] = C^T[n0 + 32j + 8g + 4h + q][m0 + 32i + r]
  const bool f32 = p.c_f32 != 0;
  const int esz = f32 ? 4 : 2;
  const bool vec = (p.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(p.C) & (4 * esz - 1)) == 0 &&
                   (!p.bias || (reinterpret_cast<uintptr_t>(p.bias) & 15) == 0) &&
                   (!p.R || ((p.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(p.R) & 7) == 0));
  const bool relu = p.relu != 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + i * 32 + r;
    if (m >= M) continue;
    const uint16_t* rrow = p.R ? p.R + static_cast<int64_t>(m) * p.ldr : nullptr;
    char* crow = static_cast<char*>(p.C) + static_cast<int64_t>(m) * p.ldc * esz;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int n = n0 + 32 * j + 8 * gq + 4 * h;
        if (n >= N) continue;
        float v[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) v[qq] = acc[j][i][4 * gq + qq];
        if (vec && n + 3 < N) {
          if (p.bias) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
            v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
          }
          if (rrow) {
            const uint2 rv = *reinterpret_cast<const uint2*>(rrow + n);
            v[0] += bf2f(rv.x & 0xffffu); v[1] += bf2f(rv.x >> 16);
            v[2] += bf2f(rv.y & 0xffffu); v[3] += bf2f(rv.y >> 16);
          }
          if (relu) {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) v[qq] = fmaxf(v[qq], 0.f);
          }
          if (f32) {
            f32x4* dst = reinterpret_cast<f32x4*>(crow) + n / 4;
            const f32x4 o = {v[0], v[1], v[2], v[3]};
            if (p.c_stream) __builtin_nontemporal_store(o, dst);
            else *dst = o;
          } else {
            uint2 o;
            o.x = pack2(v[0], v[1]);
            o.y = pack2(v[2], v[3]);
            *reinterpret_cast<uint2*>(crow + static_cast<int64_t>(n) * 2) = o;
          }
        } else {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int nn = n + qq;
            if (nn >= N) break;
            float x = v[qq];
            if (p.bias) x += p.bias[nn];
            if (rrow) x += bf2f(rrow[nn]);
            if (relu) x = fmaxf(x, 0.f);
            if (f32) reinterpret_cast<float*>(crow)[nn] = x;
            else reinterpret_cast<uint16_t*>(crow)[nn] = f2bf(x);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Depthwise 3x3: one thread = one output pixel x 8 channels (16-byte loads and stores);
// consecutive threads walk the channel axis first.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depthwise3x3_bf16_kernel(EposDepthwiseBf16Args p,
                                                                int c8n, int64_t total) {
  EPOS_SET_PRIO(DW_PRIO);
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const Pixel o = decode_pixel<8>(id, c8n, p.Ho, p.Wo);
  const int pad = p.rate;      // SAME (stride 1) and fixed_padding + VALID (stride 2) agree
  float acc[8];
  {
    const float4 b0 = *reinterpret_cast<const float4*>(p.bias + o.c);
    const float4 b1 = *reinterpret_cast<const float4*>(p.bias + o.c + 4);
    acc[0] = b0.x; acc[1] = b0.y; acc[2] = b0.z; acc[3] = b0.w;
    acc[4] = b1.x; acc[5] = b1.y; acc[6] = b1.z; acc[7] = b1.w;
  }
  const uint16_t* xb = p.X + static_cast<int64_t>(o.b) * p.Hi * p.Wi * p.ldx + o.c;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yi = o.yo * p.stride - pad + ky * p.rate;
    if (yi < 0 || yi >= p.Hi) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xi = o.xo * p.stride - pad + kx * p.rate;
      if (xi < 0 || xi >= p.Wi) continue;
      float v[8];
      ld8(xb + (static_cast<int64_t>(yi) * p.Wi + xi) * p.ldx, v);
      const float* w = p.w9c + (ky * 3 + kx) * p.C + o.c;
      const float4 w0 = *reinterpret_cast<const float4*>(w);
      const float4 w1 = *reinterpret_cast<const float4*>(w + 4);
      const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = p.relu_in ? fmaxf(v[e], 0.f) : v[e];
        acc[e] = fmaf(xv, wv[e], acc[e]);
      }
    }
  }
  if (p.relu_out) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaxf(acc[e], 0.f);
  }
  st8(p.Y + pixel_offset(o, p.Ho, p.Wo, p.ldy), acc);
}

// ---------------------------------------------------------------------------
// im2col: one thread = 8 consecutive columns of one row of col (one 16-byte store). A bf16
// source with C % 8 == 0 reads the 8 columns as one 16-byte load (they share a tap).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void im2col_bf16_kernel(EposIm2colBf16Args p, int q,
                                                          int64_t total) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const Pixel o = decode_pixel<8>(id, q, p.Ho, p.Wo);      // c = the first of the 8 columns
  const int col0 = o.c, xo = o.xo, yo = o.yo, b = o.b;
  const int64_t m = id / q;
  const int kkc = p.k * p.k * p.C;
  const int y0 = yo * p.stride - p.pad, x0 = xo * p.stride - p.pad;
  uint16_t* dst = p.col + m * p.ldcol + col0;
  float v[8];
  if (p.x_bf16 && (p.C & 7) == 0) {
    if (col0 < kkc) {
      const int tap = col0 / p.C, c = col0 - tap * p.C;
      const int ky = tap / p.k, kx = tap - ky * p.k;
      const int yi = y0 + ky * p.rate, xi = x0 + kx * p.rate;
      if (yi >= 0 && yi < p.Hi && xi >= 0 && xi < p.Wi) {
        const uint16_t* src = static_cast<const uint16_t*>(p.X) +
            ((static_cast<int64_t>(b) * p.Hi + yi) * p.Wi + xi) * p.ldx + c;
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
        return;
      }
    }
    *reinterpret_cast<u32x4*>(dst) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const float m0 = p.mean_rgb[0], m1 = p.mean_rgb[1], m2 = p.mean_rgb[2];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = col0 + j;
    float e = 0.f;
    if (col < kkc) {
      const int tap = col / p.C, c = col - tap * p.C;
      const int ky = tap / p.k, kx = tap - ky * p.k;
      const int yi = y0 + ky * p.rate, xi = x0 + kx * p.rate;
      if (yi >= 0 && yi < p.Hi && xi >= 0 && xi < p.Wi) {
        const int64_t off = ((static_cast<int64_t>(b) * p.Hi + yi) * p.Wi + xi) * p.ldx + c;
        if (p.x_bf16) {
          e = bf2f(static_cast<const uint16_t*>(p.X)[off]);
        } else {
          e = static_cast<const float*>(p.X)[off];
          if (p.preprocess == EPOS_PREPROCESS_UNIT_RANGE) {
            e = (2.0f / 255.0f) * e - 1.0f;                        // feature.py:171-174
          } else if (p.preprocess == EPOS_PREPROCESS_SUB_MEAN) {   // feature.py:157-165
            e = e - (c == 0 ? m0 : c == 1 ? m1 : c == 2 ? m2 : 0.f);
          }
        }
      }
    }
    v[j] = e;
  }
  st8(dst, v);
}

// Global mean into fp32: block = (image, 64 channels); 8 channel groups x 32 row phases;
// fixed-order LDS reduction (deterministic).
__global__ __launch_bounds__(256) void global_avg_pool_bf16_kernel(
    const uint16_t* X, int64_t ldx, float* Y, int HW, int C) {
  __shared__ float part[32][64];
  const int b = blockIdx.y;
  const int cg = threadIdx.x & 7, phase = threadIdx.x >> 3;
  const int c = blockIdx.x * 64 + cg * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const uint16_t* xb = X + static_cast<int64_t>(b) * HW * ldx + c;
    for (int r = phase; r < HW; r += 32) {
      float v[8];
      ld8(xb + static_cast<int64_t>(r) * ldx, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[phase][cg * 8 + e] = s[e];
  __syncthreads();
  if (threadIdx.x < 64 && blockIdx.x * 64 + static_cast<int>(threadIdx.x) < C) {
    float t = part[0][threadIdx.x];
    for (int i = 1; i < 32; ++i) t += part[i][threadIdx.x];
    Y[static_cast<int64_t>(b) * C + blockIdx.x * 64 + threadIdx.x] = t / static_cast<float>(HW);
  }
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int64_t epos_pack_pointwise_weights_bf16(const float* W, int K, int N, uint16_t* dst) {
  if (K < 1 || N < 1) {
    set_error("epos_pack_pointwise_weights_bf16: K, N must be >= 1");
    return EPOS_E_INVALID;
  }
  const int64_t k32 = round_up(K, 32), npad = round_up(N, 128);
  const int64_t total = k32 * npad;
  if (!dst) return total;
  if (!W) {
    set_error("epos_pack_pointwise_weights_bf16: null W");
    return EPOS_E_INVALID;
  }
  for (int64_t kg = 0; kg < k32 / 8; ++kg)
    for (int64_t n = 0; n < npad; ++n)
      for (int j = 0; j < 8; ++j) {
        const int64_t k = kg * 8 + j;
        dst[(kg * npad + n) * 8 + j] = (k < K && n < N) ? f2bf(W[k * N + n]) : 0;
      }
  return total;
}

extern "C" int epos_pointwise_conv_bf16(const EposPointwiseBf16Args* args, int count,
                                        void* stream) {
  EPOS_REQUIRE(args && count >= 1 && count <= G_MAXP, "1..8 problems");
  GemmGroup g;
  g.count = count;
  int tiles = 0;
  for (int i = 0; i < count; ++i) {
    const EposPointwiseBf16Args& a = args[i];
    EPOS_REQUIRE(a.A && a.Wp && a.C, "null pointer");
    EPOS_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "empty problem");
    EPOS_REQUIRE(a.K % 8 == 0 && a.lda % 8 == 0 && a.lda >= a.K,
                 "K and lda must be multiples of 8, lda >= K");
    EPOS_REQUIRE(al16(a.A), "A must be 16-byte aligned");
    EPOS_REQUIRE(a.ldc >= a.N && (!a.R || a.ldr >= a.N), "ldc / ldr must be >= N");
    EPOS_REQUIRE(a.sub >= 1, "sub must be >= 1");
    EPOS_REQUIRE(a.sub == 1 || (a.Ho > 0 && a.Wo > 0 && a.Hi > 0 && a.Wi > 0 &&
                                (a.Ho - 1) * a.sub < a.Hi && (a.Wo - 1) * a.sub < a.Wi &&
                                a.M % (a.Ho * a.Wo) == 0),
                 "sub > 1 needs Ho, Wo, Hi, Wi with M = B * Ho * Wo");
    g.p[i] = a;
    g.npad[i] = static_cast<int>(round_up(a.N, 128));
    g.tiles_n[i] = static_cast<int>(ceil_div(a.N, G_BN));
    g.tile_start[i] = tiles;
    const int64_t t = static_cast<int64_t>(g.tiles_n[i]) * ceil_div(a.M, G_BM);
    EPOS_REQUIRE(tiles + t < (1ll << 31), "problem too large");
    tiles += static_cast<int>(t);
  }
  for (int i = count; i <= G_MAXP; ++i) g.tile_start[i] = tiles;
  hipLaunchKernelGGL(gemm_bf16_kernel, dim3(tiles), dim3(256), 0,
                     static_cast<hipStream_t>(stream), g);
  return launch_status("gemm_bf16_kernel");
}

extern "C" int epos_depthwise3x3_bf16(const EposDepthwiseBf16Args* a, void* stream) {
  EPOS_REQUIRE(a && a->X && a->Y && a->w9c && a->bias, "null pointer");
  EPOS_REQUIRE(a->C % 8 == 0 && a->ldx % 8 == 0 && a->ldy % 8 == 0 && a->ldx >= a->C &&
               a->ldy >= a->C, "C, ldx, ldy must be multiples of 8");
  EPOS_REQUIRE(al16(a->X) && al16(a->Y) && al16(a->w9c) && al16(a->bias), "16-byte alignment");
  EPOS_REQUIRE(a->stride == 1 || a->stride == 2, "stride 1 or 2");
  EPOS_REQUIRE(a->rate >= 1, "rate >= 1");
  const int eho = a->stride == 1 ? a->Hi : (a->Hi - 1) / 2 + 1;
  const int ewo = a->stride == 1 ? a->Wi : (a->Wi - 1) / 2 + 1;
  EPOS_REQUIRE(a->Ho == eho && a->Wo == ewo, "Ho / Wo do not match stride");
  const int c8n = a->C / 8;
  const int64_t total = static_cast<int64_t>(a->B) * a->Ho * a->Wo * c8n;
  if (total <= 0) return EPOS_OK;
  hipLaunchKernelGGL(depthwise3x3_bf16_kernel, dim3(blocks_for(total, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), *a, c8n, total);
  return launch_status("depthwise3x3_bf16_kernel");
}

extern "C" int epos_im2col_bf16(const EposIm2colBf16Args* a, void* stream) {
  EPOS_REQUIRE(a && a->X && a->col, "null pointer");
  EPOS_REQUIRE(a->k >= 1 && a->C >= 1 && a->stride >= 1 && a->rate >= 1 && a->pad >= 0,
               "bad geometry");
  EPOS_REQUIRE(a->ldcol % 8 == 0 && a->ldcol >= static_cast<int64_t>(a->k) * a->k * a->C,
               "ldcol must be a multiple of 8 and >= k*k*C");
  EPOS_REQUIRE(al16(a->col), "col must be 16-byte aligned");
  EPOS_REQUIRE(!a->x_bf16 || a->preprocess == EPOS_PREPROCESS_NONE,
               "a bf16 source takes no preprocessing");
  EPOS_REQUIRE(!a->x_bf16 || (a->C % 8 != 0) || (a->ldx % 8 == 0 && al16(a->X)),
               "bf16 source with C % 8 == 0 needs ldx % 8 == 0 and 16-byte alignment");
  EPOS_REQUIRE(a->preprocess >= EPOS_PREPROCESS_NONE && a->preprocess <= EPOS_PREPROCESS_SUB_MEAN,
               "unknown preprocess mode");
  const int q = static_cast<int>(a->ldcol / 8);
  const int64_t total = static_cast<int64_t>(a->B) * a->Ho * a->Wo * q;
  if (total <= 0) return EPOS_OK;
  hipLaunchKernelGGL(im2col_bf16_kernel, dim3(blocks_for(total, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), *a, q, total);
  return launch_status("im2col_bf16_kernel");
}

extern "C" int epos_global_avg_pool_bf16(const uint16_t* X, int64_t ldx, float* Y, int B,
                                         int HW, int C, void* stream) {
  EPOS_REQUIRE(X && Y, "null pointer");
  EPOS_REQUIRE(C % 8 == 0 && ldx % 8 == 0 && al16(X), "C, ldx multiples of 8");
  EPOS_REQUIRE(B >= 1 && HW >= 1 && C >= 1, "empty map");
  EPOS_REQUIRE(ldx >= C, "ldx >= C");
  hipLaunchKernelGGL(global_avg_pool_bf16_kernel, dim3(blocks_for(C, 64), B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), X, ldx, Y, HW, C);
  return launch_status("global_avg_pool_bf16_kernel");
}
