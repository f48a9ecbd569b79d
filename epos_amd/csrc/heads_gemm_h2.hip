// The dense logits heads on the fp16 matrix pipe: an A-stationary form of the fp16-pair GEMM
// (pointwise_gemm_h2.hip) for the grouped head problems -- one A shared by every problem of
// the group (the decoder output), K = 256, fp32 A with a scale from the absmax slot, packed
// fp16-pair W, bias, no residual / ReLU / absmax publish. Round 10.
//
// Why a kernel of its own: at K = 256 the generic kernel's 128 x 128 workgroup spends about
// half its life outside the K loop (set-up ~2.2 us, loop 8.7 us, epilogue ~5 us; the r04
// timeline), and every (M, N) tile re-reads its 128 x 256 fp32 A block into LDS and splits it
// again -- 44 times per A element at C2.
//
// Structure.
//  * Work item = one 128-row PANEL of A x a RANGE of consecutive 64-column N tiles of the
//    group (the tiles of all problems laid end to end: tile0[]). A workgroup (4 waves, a wave
//    owns 32 rows) loads its panel ONCE into registers and splits it once: per lane 16 K steps
//    x {hi, mid} x 4 dwords = 128 VGPRs, exactly the MFMA A operands of the generic kernel.
//  * Only W is streamed: one 1 KB LDS-DMA piece per wave and K step (the 4 KB half of the
//    packed 128-column stage image that holds the tile's 64 columns) into an 8-stage ring,
//    7 steps ahead; the ring runs on across tile boundaries, so the first W stages of tile
//    j + 1 are in flight while tile j's epilogue runs. The per-column epilogue operands
//    (inverse weight scale, bias: 2 x 64 floats) ride the same ring as two dword LDS-DMA
//    pieces per wave, issued with tile j + 1's first W piece into a per-wave, per-parity slot.
//  * Epilogue: (acc + corr * 2^-11) is staged through the wave's own LDS rows (not part of
//    the ring: no barrier), then x cn, x inv_a, + bias and 128-bit BUFFER stores (streaming
//    when c_stream): a row out of the matrix or a column >= N gets an out-of-range offset and
//    is dropped by the hardware, so every lane issues the same number of stores per tile and
//    the ring's counted waits can leave them in flight: the waits of the next tile's first
//    six K steps count the tile's 8 stores (HD_S_MIN; the element-wise path of an unaligned
//    problem -- the 22-column object head -- issues 32, more than counted: it waits longer,
//    never too short). The stores of tile j therefore drain under tile j + 1's MFMAs.
//  * Two workgroups per CU (LDS 74 KB each, <= 256 registers per wave): while one is in its
//    epilogue or its A load, the other one's MFMAs run.
//
// Work items and balance (host, choose_range): items of one XCD (blockIdx % 8) share a
// contiguous eighth of the panels and walk the N ranges range-major, so that the W range in
// use (range x 64 KB) and the XCD's panels (C2: 19 x 128 KB) both stay in its 4 MB L2. The
// range length R minimises ceil(items per XCD / 64 slots) x (R + 1) (one tile's worth of
// set-up per item) over R in [4, 32]. C2 (M 19 200, N 22 + 1 344 + 4 032 = 85 tiles, P = 150
// panels, at most 19 per XCD): R = 9, 10 ranges, 190 items per XCD on 64 slots (2.97 rounds of
// 9 tiles). F = 256 (337 tiles): R = 17, 20 ranges, 380 items per XCD (5.94 rounds). C4 (M
// 24 300, 190 panels): R = 11, 8 ranges, 192 items (3.0 rounds).
//
// Bits: identical to pointwise_gemm_h2_f32 by construction -- the same scale (h2_scale) and
// split (h2_split_pair) of A, the same A / W operand layouts, the same three
// v_mfma_f32_32x32x16_f16 per column block and K step in ascending K into the same
// accumulators in the same order (corr += ah * bm, corr += am * bh, acc += ah * bh), and the
// same element-wise epilogue: fma(corr, 2^-11, acc) * cn * inv_a + bias. An element's value
// does not depend on the tile or workgroup that computes it. tests/test_gpu_heads.py and, per
// launch regime, tests/test_gpu_heads_regimes.py hold the two kernels to equal bit patterns;
// epos_heads_gemm_plan (heads_plan below) tells them that this kernel is the one that ran.
//
// Resources (hipcc -O3 -Rpass-analysis=kernel-resource-usage, profiles/r10/): 252 VGPRs, no
// AGPRs, 0 bytes of scratch, 75 776 B of LDS: two workgroups = two waves per SIMD. Measured:
// 182 us per launch at C2 (the generic kernel: 203), 642 at F = 256 (778); profiles/r10/.
#include "h2_scale.h"
#include "pointwise_gemm.h"

namespace epos {
namespace {

typedef _Float16 hd_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned hd_u32x4 __attribute__((ext_vector_type(4)));

constexpr int HD_BM = 128, HD_BN = 64, HD_BK = 16;
constexpr int HD_K = 256;
constexpr int HD_NKS = HD_K / HD_BK;                 // 16 K steps per tile
constexpr int HD_NS = 8;                             // ring stages (a power of two, divides 16)
constexpr int HD_LA = HD_NS - 1;                     // K steps issued ahead
constexpr int HD_STAGE = 4 * 1024;                   // W: 2 column blocks x {hi, mid} x 1 KB
constexpr int HD_RING = HD_NS * HD_STAGE;            // 32 KB
constexpr int HD_OPS = 2 * 4 * 1024;                 // [parity][wave]: cn[64] | bias[64] (1 KB)
constexpr int HD_EPR = HD_BN + 4;                    // floats per staged epilogue row
constexpr int HD_EPI = 4 * 32 * HD_EPR * 4;          // 34 KB: a wave stages its 32 x 64 block
constexpr int HD_LDS = HD_RING + HD_OPS + HD_EPI;    // 75776 B: two workgroups per CU
constexpr int HD_S_MIN = 8;                          // stores per lane and tile (lower bound)
constexpr unsigned HD_OOB = 0x80000000u;             // buffer offset beyond any record count
static_assert(HD_NKS % HD_NS == 0, "stage of a K step = its index mod HD_NS");
static_assert(HD_LA - 2 + 2 + HD_S_MIN <= 63, "vmcnt is a 6-bit counter");

struct HeadsArgs {
  EposPointwiseArgs p[MAX_GROUP];
  int tile0[MAX_GROUP + 1];     // first 64-column tile of problem i in a panel's tile list
  int count;
  int nt;                       // tiles per panel (sum over the problems)
  int panels;                   // ceil(M / 128)
  int range;                    // tiles per work item
  int nr;                       // ranges per panel
  const float* zero_chunk;      // 16+ zero bytes in device memory
};

template <int... I, class F>
__device__ __forceinline__ void hd_static_for(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N> __device__ __forceinline__ void hd_wait_vm_lgkm0() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" : : "n"(N) : "memory");
}
// one wave-instruction: 64 lanes x 4 B (per-lane source) -> LDS [lds_dst, lds_dst + 256)
__device__ __forceinline__ void glds4_v_m0(const float* gsrc, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
               : : "v"(gsrc), "s"(lds_dst) : "memory", "m0");
}

// Where tile t of a panel's tile list lies: its problem, W stage images, epilogue operands.
struct HdTile {
  const float* w;       // the tile's 4 KB W piece of K step 0 (+ 8 KB per K step)
  const float* cn;      // 64 inverse column scales (padded to a multiple of 128 columns)
  const float* bias;    // nullptr: no bias
  int n0, N, pi;
};
__device__ __forceinline__ HdTile hd_tile(const HeadsArgs* gp, int t) {
  int pi = 0;
#pragma unroll
  for (int i = 1; i < MAX_GROUP; ++i)
    if (i < gp->count && t >= gp->tile0[i]) pi = i;
  const EposPointwiseArgs& q = gp->p[pi];
  const int tl = t - gp->tile0[pi];
  const int tn128 = (q.N + 127) >> 7;
  const char* wh = static_cast<const char*>(q.Wh);
  HdTile r;
  r.w = reinterpret_cast<const float*>(wh + static_cast<int64_t>(tl >> 1) * HD_NKS * 8192 +
                                       (tl & 1) * 4096);
  r.cn = reinterpret_cast<const float*>(wh + static_cast<int64_t>(tn128) * HD_NKS * 8192) +
         tl * HD_BN;
  r.bias = q.bias;
  r.n0 = tl * HD_BN;
  r.N = q.N;
  r.pi = pi;
  return r;
}

__device__ __forceinline__ void hd_mfma(const hd_u32x4& a, const hd_u32x4& b, f32x16& c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hd_f16x8, a),
                                             __builtin_bit_cast(hd_f16x8, b), c, 0, 0, 0);
}

__global__ __launch_bounds__(256, 2) void heads_gemm_h2_f32(HeadsArgs ga_) {
  (void)ga_;
  const HeadsArgs* __restrict__ gp = (const HeadsArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int l31 = lane & 31, h = lane >> 5;

  // ---- work item: XCD x = blockIdx % 8 owns panels [p_lo, p_hi), range-major
  int panel, t0, t1;
  {
    const int raw = blockIdx.x, x = raw & 7, k = raw >> 3;
    const int P = gp->panels;
    const int p_lo = (x * P) >> 3, p_hi = ((x + 1) * P) >> 3;
    const int px = p_hi - p_lo;
    if (k >= px * gp->nr) return;
    const int r = k / px;
    panel = p_lo + (k - r * px);
    t0 = r * gp->range;
    t1 = t0 + gp->range < gp->nt ? t0 + gp->range : gp->nt;
  }
  const EposPointwiseArgs& pa = gp->p[0];           // A, M, lda, scale: common to the group
  const int M = pa.M;
  const int m0 = panel * HD_BM;
  const float* zero_chunk = gp->zero_chunk;

  unsigned am_raw = 0, am_raw2 = 0;
  h2_scale_load(pa.a_amax, pa.a_amax2, lane, am_raw, am_raw2);

  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) float*)smem));
  const unsigned w_voff = static_cast<unsigned>(wave * 1024 + lane * 16);
  const unsigned w_dst = lds0 + wave_u * 1024;
  const unsigned ops_dst = lds0 + HD_RING + wave_u * 1024;

  // W piece of K step kq of tile `ti` into ring stage `slot`
  auto issue_w = [&](const HdTile& ti, int kq, int slot) {
    glds16_s_m0(w_voff, uniform_ptr(ti.w + kq * (8192 / 4)), w_dst + slot * HD_STAGE);
  };
  // epilogue operands of tile `ti` into parity slot `par` (two pieces)
  auto issue_ops = [&](const HdTile& ti, int par) {
    glds4_v_m0(ti.cn + lane, ops_dst + par * 4096);
    const int n = ti.n0 + lane;
    const float* b = (ti.bias && n < ti.N) ? ti.bias + n : zero_chunk;
    glds4_v_m0(b, ops_dst + par * 4096 + 256);
  };

  HdTile cur = hd_tile(gp, t0);
  HdTile nxt = hd_tile(gp, t0 + 1 < t1 ? t0 + 1 : t0);   // a duplicate at the end: the
                                                          // pieces per step stay uniform
  // ---- A panel: rows m0 + 32 wave + l31 (clamped), k = 16 ks + 8 h + 0..7, loaded once
  hd_u32x4 ah[HD_NKS], am[HD_NKS];
  float inv_a;
  {
    int m = m0 + wave * 32 + l31;
    m = m < M ? m : M - 1;
    const float* arow = pa.A + static_cast<int64_t>(m) * pa.lda + 8 * h;
    float4 xa[2 * HD_NKS];
#pragma unroll
    for (int ks = 0; ks < HD_NKS; ++ks) {
      xa[2 * ks] = *reinterpret_cast<const float4*>(arow + ks * HD_BK);
      xa[2 * ks + 1] = *reinterpret_cast<const float4*>(arow + ks * HD_BK + 4);
    }
    // prologue of the W ring: K steps 0 .. LA-1 of the first tile (+ its epilogue operands,
    // which travel with K step 0) -- the same pieces in the same order as the steady state
    issue_w(cur, 0, 0);
    issue_ops(cur, 0);
#pragma unroll
    for (int q = 1; q < HD_LA; ++q) issue_w(cur, q, q);
    float sa_v, inv_a_v;
    h2_scale_finish(am_raw, am_raw2, pa.a_gain, pa.a_bias, sa_v, inv_a_v);
    const float sa = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sa_v)));
    inv_a = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(inv_a_v)));
#pragma unroll
    for (int ks = 0; ks < HD_NKS; ++ks)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 x4 = xa[2 * ks + (u >> 1)];
        const float x0 = (u & 1) ? x4.z : x4.x, x1 = (u & 1) ? x4.w : x4.y;
        unsigned hh, mm;
        h2_split_pair(x0, x1, sa, hh, mm);
        ah[ks][u] = hh;
        am[ks][u] = mm;
      }
  }

  // W of K step 0 landed: younger are its epilogue operands (2) and K steps 1 .. LA-1
  hd_wait_vm_lgkm0<2 + HD_LA - 1>();
  __builtin_amdgcn_s_barrier();
  const int b_off = lane * 4;                       // + (cb * 2 + piece) * 256 floats
  hd_u32x4 bp[2][2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int pc = 0; pc < 2; ++pc)
      bp[cb][pc] = *reinterpret_cast<const hd_u32x4*>(smem + b_off + (cb * 2 + pc) * 256);

  float* ws = smem + (HD_RING + HD_OPS) / 4 + wave * 32 * HD_EPR;
  const int c4 = lane & 15, r0 = lane >> 4;          // row phase: 16 float4 per row, 4 rows

  for (int tt = t0; tt < t1; ++tt) {
    const bool first = tt == t0;
    const int par = (tt - t0) & 1;
    f32x16 acc[2], corr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[j][r] = 0.f; corr[j][r] = 0.f; }

    // K step ks of this tile (global step g = 16 tile + ks). At its top, W(g + 1) must have
    // landed. Younger than that piece on this wave's counter: the pieces of steps g-5 .. g-1
    // (one each, +2 operand pieces in the step that issues a tile's K step 0: ks = 9, seen
    // from ks = 10..14), the two operand pieces issued right behind W(g + 1) itself (ks = 15),
    // and -- for ks <= 5, unless this is the work item's first tile -- the previous tile's
    // stores (at least HD_S_MIN).
    auto step = [&](auto ks_tag) {
      constexpr int ks = decltype(ks_tag)::value;
      constexpr int younger = (HD_LA - 2) + (ks >= 10 ? 2 : 0);
      static_assert(HD_LA == 7, "the counts above are written for 7 steps ahead");
      if constexpr (ks <= 5) {
        if (first) hd_wait_vm_lgkm0<younger>();
        else hd_wait_vm_lgkm0<younger + HD_S_MIN>();
      } else {
        hd_wait_vm_lgkm0<younger>();
      }
      __builtin_amdgcn_s_barrier();
      constexpr int s1 = (ks + 1) % HD_NS;
      hd_u32x4 nb[2][2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc)
          nb[cb][pc] = *reinterpret_cast<const hd_u32x4*>(smem + s1 * (HD_STAGE / 4) + b_off +
                                                          (cb * 2 + pc) * 256);
      __builtin_amdgcn_sched_barrier(0);
      // the generic kernel's order (pointwise_gemm_h2.hip, tile2): per accumulator
      // corr += ah * bm, corr += am * bh; acc += ah * bh
      hd_mfma(ah[ks], bp[0][1], corr[0]);
      __builtin_amdgcn_sched_barrier(0);
      {   // W of step g + LA into the stage of step g - 1 (read in step g - 2, before the
          // barrier of step g - 1)
        constexpr int q = ks + HD_LA;
        constexpr int slot = q % HD_NS;
        if constexpr (q < HD_NKS) issue_w(cur, q, slot);
        else issue_w(nxt, q - HD_NKS, slot);
      }
      __builtin_amdgcn_sched_barrier(0);
      hd_mfma(ah[ks], bp[1][1], corr[1]);
      if constexpr (ks + HD_LA == HD_NKS) {
        __builtin_amdgcn_sched_barrier(0);
        issue_ops(nxt, par ^ 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      hd_mfma(am[ks], bp[0][0], corr[0]);
      hd_mfma(am[ks], bp[1][0], corr[1]);
      hd_mfma(ah[ks], bp[0][0], acc[0]);
      hd_mfma(ah[ks], bp[1][0], acc[1]);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) { bp[cb][0] = nb[cb][0]; bp[cb][1] = nb[cb][1]; }
    };
    hd_static_for(std::make_integer_sequence<int, HD_NKS>{}, step);

    // ---- epilogue: stage acc + corr * 2^-11 (element-wise as the generic kernel)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ws[((r & 3) + 8 * (r >> 2) + 4 * h) * HD_EPR + j * 32 + l31] =
            __builtin_fmaf(corr[j][r], 0x1p-11f, acc[j][r]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const float* ops = smem + (HD_RING + par * 4096) / 4 + wave * 256;
    const float4 cn4 = *reinterpret_cast<const float4*>(ops + c4 * 4);
    const float4 b4 = *reinterpret_cast<const float4*>(ops + 64 + c4 * 4);
    float4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = *reinterpret_cast<const float4*>(ws + (r0 + 4 * i) * HD_EPR + c4 * 4);
      v[i].x = v[i].x * cn4.x * inv_a + b4.x;
      v[i].y = v[i].y * cn4.y * inv_a + b4.y;
      v[i].z = v[i].z * cn4.z * inv_a + b4.z;
      v[i].w = v[i].w * cn4.w * inv_a + b4.w;
    }
    const EposPointwiseArgs& q = gp->p[cur.pi];
    const int rows = M - m0 < HD_BM ? M - m0 : HD_BM;
    const int64_t ldc = q.ldc;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        q.C + static_cast<int64_t>(m0) * ldc, 0, static_cast<int>(rows * ldc * 4), 0x00020000);
    const int n = cur.n0 + c4 * 4;
    const unsigned row0 = static_cast<unsigned>(wave * 32 + r0);
    const bool vec = (ldc & 3) == 0 && (cur.N & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(q.C) & 15) == 0;
    // out-of-range lanes: the offset's top bit set (>= 2^31 > any record count). Opaque to
    // the compiler, which otherwise splits a select of offsets into two exec-masked stores
    // behind branches -- and the number of stores a wave issues must not depend on the data
    auto opaque = [](unsigned x) { asm volatile("" : "+v"(x)); return x; };
    if (vec) {
      const unsigned oob = n < cur.N ? 0u : HD_OOB;
      const unsigned nb4 = static_cast<unsigned>(n) * 4u;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int off = static_cast<int>(
            opaque(((row0 + 4 * i) * static_cast<unsigned>(ldc) * 4u + nb4) | oob));
        if (q.c_stream)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hd_u32x4, v[i]), rsrc, off, 0, 2);
        else
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hd_u32x4, v[i]), rsrc, off, 0, 0);
      }
    } else {
      // element-wise stores (N or ldc not a multiple of 4, e.g. the 22-column object head)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float e4[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned oob = n + e < cur.N ? 0u : HD_OOB;
          const int off = static_cast<int>(opaque(
              (((row0 + 4 * i) * static_cast<unsigned>(ldc) + static_cast<unsigned>(n + e)) * 4u) |
              oob));
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e4[e]), rsrc, off, 0, 0);
        }
      }
    }
    cur = nxt;
    nxt = hd_tile(gp, tt + 2 < t1 ? tt + 2 : t1 - 1);
  }
  // nothing of the ring may still be landing in LDS when the workgroup's LDS is handed on
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// R (tiles per work item): fewest estimated rounds x item length, one tile of set-up per item
int choose_range(int nt, int panels, int cus) {
  const int slots = cus > 8 ? cus * 2 / 8 : 1;      // workgroups per XCD at a time
  const int pmax = (panels + 7) / 8;
  int best = nt < 4 ? nt : 4;
  int64_t best_cost = -1;
  for (int r = 4; r <= 32; ++r) {
    const int rr = r < nt ? r : nt;
    const int64_t nr = (nt + rr - 1) / rr;
    const int64_t rounds = (pmax * nr + slots - 1) / slots;
    const int64_t cost = rounds * (rr + 1);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = rr; }
    if (rr == nt) break;
  }
  return best;
}

int device_cus() {
  static int cus[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  int n = __atomic_load_n(&cus[dev], __ATOMIC_RELAXED);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
    n = 256;
  __atomic_store_n(&cus[dev], n, __ATOMIC_RELAXED);
  return n;
}

}  // namespace

// The group this kernel takes (besides h2_eligible): one A for every problem (same pointer,
// lda, M, scale slots), K = 256, 1x1 rows (sub 1), fp32 A, no residual / ReLU / output
// absmax / column sums, a bound for A, and W packed for the fp16-pair kernel.
bool heads_eligible(const EposPointwiseArgs* args, int count) {
  if (count < 1 || count > MAX_GROUP) return false;
  const EposPointwiseArgs& a0 = args[0];
  if (!a0.a_amax) return false;
  for (int i = 0; i < count; ++i) {
    const EposPointwiseArgs& a = args[i];
    if (a.A != a0.A || a.lda != a0.lda || a.M != a0.M || a.K != HD_K || a.sub != 1 ||
        a.R || a.relu || a.relu_in || a.a_presplit || a.c_amax || a.col_sums || !a.Wh ||
        a.a_amax != a0.a_amax || a.a_amax2 != a0.a_amax2 || a.a_gain != a0.a_gain ||
        a.a_bias != a0.a_bias || a.N < 1 || a.M < 1 || a.ldc < a.N ||
        a.ldc > (1LL << 20) ||                        // 128 rows x ldc x 4 B: a 32-bit range
        (reinterpret_cast<uintptr_t>(a.Wh) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(a.bias) & 3) != 0)
      return false;
  }
  return true;
}

namespace {

// The one routine behind the launch and the plan query (epos_heads_gemm_plan): false = the
// group falls back to the grouped GEMM; otherwise g holds the kernel's arguments but for
// zero_chunk, and `blocks` the grid. cus = 0: the current device's count.
bool heads_fill(const EposPointwiseArgs* args, int count, int cus, HeadsArgs& g, int& blocks) {
  if (!h2_eligible(args, count) || !heads_eligible(args, count)) return false;
  g.count = count;
  int nt = 0;
  for (int i = 0; i < count; ++i) {
    g.p[i] = args[i];
    g.tile0[i] = nt;
    nt += static_cast<int>(ceil_div(args[i].N, HD_BN));
  }
  for (int i = count; i <= MAX_GROUP; ++i) g.tile0[i] = nt;
  g.nt = nt;
  g.panels = static_cast<int>(ceil_div(args[0].M, HD_BM));
  g.range = choose_range(nt, g.panels, cus > 0 ? cus : device_cus());
  g.nr = static_cast<int>(ceil_div(nt, g.range));
  int items = 0;                                     // the largest XCD's item count
  for (int x = 0; x < 8; ++x) {
    const int px = ((x + 1) * g.panels >> 3) - (x * g.panels >> 3);
    items = px * g.nr > items ? px * g.nr : items;
  }
  blocks = 8 * items;
  return true;
}

}  // namespace

bool heads_takes(const EposPointwiseArgs* args, int count) {
  return h2_eligible(args, count) && heads_eligible(args, count);
}

int heads_plan(const EposPointwiseArgs* args, int count, int cus, int32_t* plan) {
  HeadsArgs g = {};
  int blocks = 0;
  if (!heads_fill(args, count, cus, g, blocks)) return 0;
  if (plan) {
    plan[0] = g.nt; plan[1] = g.panels; plan[2] = g.range; plan[3] = g.nr; plan[4] = blocks;
  }
  return 1;
}

int launch_heads_h2(const EposPointwiseArgs* args, int count, const float* zero_chunk,
                    hipStream_t s) {
  HeadsArgs g = {};
  int blocks = 0;
  if (!heads_fill(args, count, 0, g, blocks)) {
    set_error("launch_heads_h2: not a group of the dense-heads kernel");
    return EPOS_E_INVALID;
  }
  g.zero_chunk = zero_chunk;
  if (blocks <= 0) return EPOS_OK;
  static LdsAttrOnce once;
  const int rc = ensure_dynamic_lds(once, reinterpret_cast<const void*>(heads_gemm_h2_f32),
                                    HD_LDS, "hipFuncSetAttribute(heads_gemm_h2_f32)");
  if (rc) return rc;
  hipLaunchKernelGGL(heads_gemm_h2_f32, dim3(blocks), dim3(256), HD_LDS, s, g);
  return launch_status("heads_gemm_h2_f32");
}

}  // namespace epos
