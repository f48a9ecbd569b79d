// Pose fitting, the spatial-coherence labelling: the 5-D neighbourhood (distance, neighbour
// lists, for_each_neighbour), the binary relabelling rule, and the three sweeps over it --
// ransac_gc_sweep (LDS-staged; as ransac_nb_build it writes the lists), ransac_gc_scan and
// ransac_gc_delta. Included after fit_work.h (Work, Slot, Ball, GcDyn, GcAcc, FIT_TRACE).
#pragma once

namespace epos {
namespace {

// ---- round, step 3 (gc_sweeps launches): one synchronous relabelling sweep of the spatial-
// coherence energy (GC-RANSAC labelling): per point, over its neighbours on the 5-D
// graph (their image rows are within tau_d), the degree / residual sum / outlier-labelled
// neighbours in integers (exact, order independent), then the cheaper label.

// squared 5-D distance from the coordinate differences (pixels; millimetres scaled by s2)
__device__ __forceinline__ double gc_dist2(double dx, double dy, double dX, double dY,
                                           double dZ, double s2) {
  return (dx * dx + dy * dy) + s2 * ((dX * dX + dY * dY) + dZ * dZ);
}
__device__ __forceinline__ bool gc_neighbours(const Slot& sl, const Ball& ball, int32_t a, int32_t b) {
  const double *xy = sl.xy, *xyz = sl.xyz;
  const double dx = xy[2 * a] - xy[2 * b], dy = xy[2 * a + 1] - xy[2 * b + 1];
  const double dX = xyz[3 * a] - xyz[3 * b], dY = xyz[3 * a + 1] - xyz[3 * b + 1],
               dZ = xyz[3 * a + 2] - xyz[3 * b + 2];
  return gc_dist2(dx, dy, dX, dY, dZ, ball.s2) <= ball.r2;
}

// The binary relabelling rule: 1 (inlier) iff that label is the cheaper one for a point with
// fixed-point residual qp whose dg neighbours (itself not among them) hold z0 outlier labels
// and residuals summing to Ss. u, T: the data and smoothness terms' differences (exact).
__device__ __forceinline__ int gc_decide(int64_t qp, int64_t dg, int64_t z0, int64_t Ss,
                                         double lam) {
  const int64_t T = 2 * static_cast<int64_t>(GC_Q) * z0 - (dg * qp + Ss);
  const int64_t u = qp < GC_Q ? -2 * (static_cast<int64_t>(GC_Q) - qp)
                              : 2 * static_cast<int64_t>(GC_Q);
  const double val = (1.0 - lam) * static_cast<double>(u) + lam * static_cast<double>(T);
  return val < 0.0 ? 1 : 0;
}
// The same for the raw sums of a full window scan, in which the point (at x, y, X, Y, Z;
// out_prev: 1 if labelled outlier) met itself: taken out again by the same test on itself.
__device__ __forceinline__ int gc_decide_without_self(double x, double y, double X, double Y,
                                                      double Z, const Ball& ball, int64_t deg,
                                                      int64_t n0, int64_t S, int64_t qp, int64_t out_prev) {
  const int64_t self = gc_dist2(x - x, y - y, X - X, Y - Y, Z - Z, ball.s2) <= ball.r2 ? 1 : 0;
  return gc_decide(qp, deg - self, n0 - self * out_prev, S - self * qp, ball.lam);
}

// a slot's neighbour lists (null cnt: not available, scan the window)
constexpr int NB_W = 4;            // sub-lists per point (= waves of a sweep workgroup)
constexpr int NB_SUB = 160;        // entries per sub-list: 640 neighbours per point
struct NbLists {
  const uint16_t* cnt;
  const int16_t* pool;
};
__device__ __forceinline__ NbLists nb_lists_of(const Work& w, int s, const Slot& sl) {
  NbLists nl = {nullptr, nullptr};
  if (w.nb_ok[s]) { nl.cnt = w.nb_cnt + sl.base * NB_W; nl.pool = w.nb_pool + sl.base * (NB_W * NB_SUB); }
  return nl;
}

// Visits every ACTIVE neighbour of point p (slot-local index): f(q, valid), q = the
// neighbour's POSITION in the row-sorted order (its index if the slot is not sorted) -- f is
// called by every lane of the wave, `valid` says whether the lane holds a neighbour (q is a
// safe position otherwise), so that f's own loads are unconditional and can be in flight
// together. Callers keep what they look up per neighbour in position order: a neighbour is
// then one list entry and one nearby byte, no order look-up. Wave-wide.
// LISTS: the slot's neighbour lists are complete (Work::nb_ok) -- the caller's kernel is
// instantiated once per case, because the window walk of the other case (fp64 distance
// tests) costs the list walk three of eight waves per SIMD if both sit in one kernel.
template <bool LISTS, typename F>
__device__ __forceinline__ void for_each_neighbour(const Slot& sl, const Ball& ball, int32_t p,
                                                   int lane, const NbLists& nl, F f) {
  const int64_t pos = sl.ypos ? sl.ypos[p] : p;
  if constexpr (LISTS) {     // the slot's neighbour lists are complete: walk the point's
    // One quarter-wave per sub-list, two entries per lane and trip: count -> list entries ->
    // f's loads = THREE dependent round trips for up to 128 neighbours.
    static_assert(NB_W == 4, "one quarter-wave per sub-list");
    const int q = lane >> 4, l16 = lane & 15;
    const int cntq = nl.cnt[pos * NB_W + q];
    const int16_t* lst = nl.pool + (pos * NB_W + q) * NB_SUB;
    int cmax = cntq;                                   // wave-uniform trip count
    cmax = max(cmax, __shfl_xor(cmax, 16, 64));
    cmax = max(cmax, __shfl_xor(cmax, 32, 64));
    for (int i0 = 0; i0 < cmax; i0 += 32) {
      const int ia = i0 + l16, ib = ia + 16;
      const bool va = ia < cntq, vb = ib < cntq;
      const int64_t pa = pos + (va ? lst[ia] : 0), pb = pos + (vb ? lst[ib] : 0);
      f(pa, va);
      f(pb, vb);
    }
    return;
  }
  const double yp = sl.xy[2 * p + 1];
  for (int dir = 0; dir < 2; ++dir) {
    for (int64_t j0 = dir ? pos + 1 : pos - 1; dir ? j0 < sl.n : j0 >= 0; j0 += dir ? 64 : -64) {
      const int64_t j = dir ? j0 + lane : j0 - lane;
      const bool in = dir ? j < sl.n : j >= 0;
      int32_t o = 0;
      bool near = false;
      if (in) {
        o = sl.yorder ? sl.yorder[j] : static_cast<int32_t>(j);
        near = !(fabs(yp - sl.xy[2 * o + 1]) > ball.rad);
      }
      if (!__any(near)) break;            // sorted by y: nothing further can be in range
      f(in ? j : pos, near && gc_neighbours(sl, ball, p, o));
    }
  }
}

// One workgroup per TILE of 64 consecutive points of the row-sorted order. The points of
// a tile share one candidate window (all correspondences whose image row is within tau_d
// of the tile's rows: a contiguous range of the sorted order, found by two binary
// searches); the window streams through LDS in chunks of GC_T candidates and each thread
// tests its point (t & 63) against its wave's share of the chunk (t >> 6) -- all 64 lanes of a
// wave read the SAME candidate: LDS broadcasts, no bank conflicts. Per pair: the 5-D
// distance in fp64 and three integer counters (exact, order independent).
// 256 threads per tile: 1024 (16 waves share a tile's window) is 20 % faster for one
// image at a time (fitting 0.55 vs 0.66 ms) but costs throughput with several images in
// flight (310 vs 320 images/s, same box: the large workgroups displace GEMM workgroups)
#ifdef EPOS_GC_STATS              // tools/gc_stats.py: tiles visited, candidates streamed
__device__ unsigned long long g_gc_stats[4];
#endif
struct GcCand {
  double x, y, X, Y, Z;
  int32_t q;          // fixed-point residual
  int32_t ol;         // slot-local index | label << 30
};
constexpr int GC_T = 256;             // threads per tile workgroup
constexpr int GC_W = GC_T / 64;       // waves: each takes every GC_W-th candidate
// BUILD = true (ransac_nb_build, once per call, right after ransac_init): the same tiles and
// windows, but instead of relabelling every found neighbour is appended to the point's list
// -- GC_W sub-lists of NB_SUB entries per point, sub-list g written by the wave that tests
// every GC_W-th candidate from g on; position deltas, 2 bytes each. The sweeps of every
// round and the joint refinement walk those lists (100-300 gathers per point on EPOS's
// many-to-many sets) instead of repeating ~1 100 pair tests per point and sweep; results are
// the same integers. A slot in which some sub-list does not fit (more than NB_SUB entries, a
// delta beyond 16 bits) keeps nb_ok = 0 and its sweeps scan the windows as before.
template <bool BUILD>
__global__ __launch_bounds__(GC_T) void ransac_gc_sweep(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, EposFitParams prm, Work w,
    const uint8_t* __restrict__ lab_in_all, uint8_t* __restrict__ lab_out_all) {
  const int s = blockIdx.y;
  if (BUILD ? w.done[s] != 0 : w.state[s] != 1) return;
  // one 48-byte record per candidate = three ds_read_b128 (separate arrays serialise the
  // reads of a candidate behind one another: profiles/r03/gc_sweep_ablation.txt)
  __shared__ __attribute__((aligned(16))) GcCand c_rec[GC_T];
  __shared__ int64_t s_win[2];
  __shared__ int s_deg[GC_W][64], s_n0[GC_W][64];
  __shared__ int64_t s_S[GC_W][64];
  __shared__ int s_cnt4[GC_W];
  const int t = threadIdx.x, pt = t & 63, sub = t >> 6;
  const Slot sl = slot_of(slot_base, s, w, xy_all, xyz_all);
  const Ball ball = ball_of(prm);
  const uint8_t* lab_in = BUILD ? nullptr : lab_in_all + sl.base;
  uint8_t* lab_out = BUILD ? nullptr : lab_out_all + sl.base;
  const int32_t* gq = w.gq + sl.base;
  uint16_t* nb_cnt = w.nb_cnt + sl.base * GC_W;
  int16_t* nb_pool = w.nb_pool + sl.base * (GC_W * NB_SUB);
  const bool use_lists = !BUILD && w.nb_ok[s] != 0;        // uniform over the slot
  for (int64_t tile = blockIdx.x; tile * 64 < sl.n; tile += gridDim.x) {
    const int64_t pos0 = tile * 64;
    const int64_t pos = pos0 + pt;
    const bool valid = pos < sl.n;
    const int32_t p = valid ? (sl.yorder ? sl.yorder[pos] : static_cast<int32_t>(pos)) : 0;
    const uint8_t lp = BUILD ? 0 : (valid ? lab_in[p] : 2);
    const bool act = BUILD ? valid : lp != 2;
    int deg = 0, n0 = 0;
    int64_t S = 0;
    if (use_lists) {
      // ---- the point's neighbour list: this wave walks the sub-list it wrote ----------
      if (valid && act) {
        const int cntp = nb_cnt[pos * GC_W + sub];
        const int16_t* lst = nb_pool + (pos * GC_W + sub) * NB_SUB;
        for (int i0 = 0; i0 < cntp; i0 += 4) {
          int32_t o[4];
          int ok4[4], lo4[4], q4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int i = i0 + u;
            ok4[u] = i < cntp;
            const int64_t op = pos + lst[ok4[u] ? i : 0];
            o[u] = sl.yorder ? sl.yorder[op] : static_cast<int32_t>(op);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) { lo4[u] = lab_in[o[u]]; q4[u] = gq[o[u]]; }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int nb = ok4[u] & static_cast<int>(lo4[u] != 2);
            deg += nb;
            S += nb ? q4[u] : 0;
            n0 += nb & static_cast<int>(lo4[u] == 0);
          }
        }
      }
    } else {
    const double px = sl.xy[2 * p], py = sl.xy[2 * p + 1];
    const double pX = sl.xyz[3 * p], pY = sl.xyz[3 * p + 1], pZ = sl.xyz[3 * p + 2];
    int nlist = 0;                 // BUILD: entries in this thread's sub-list
    bool ovf = false;
    {
      // window of sorted positions whose row can hold a neighbour of a point of the tile:
      // GC_T-ary searches (every thread probes one position per step: two or three
      // dependent loads instead of the ~13 of a binary search by one thread)
      const int64_t last = pos0 + 63 < sl.n ? pos0 + 63 : sl.n - 1;
      const int32_t pf = sl.yorder ? sl.yorder[pos0] : static_cast<int32_t>(pos0);
      const int32_t pl = sl.yorder ? sl.yorder[last] : static_cast<int32_t>(last);
      const double ylo = sl.xy[2 * pf + 1] - ball.rad, yhi = sl.xy[2 * pl + 1] + ball.rad;
      for (int side = 0; side < 2; ++side) {
        // side 0: first position in [0, pos0] with y >= ylo; side 1: first position in
        // [last + 1, n] with y > yhi   (y is non-decreasing along the sorted order)
        int64_t lo = side ? last + 1 : 0, hi = side ? sl.n : pos0;
        while (hi - lo > 0) {
          const int64_t step = (hi - lo + GC_T - 1) / GC_T;
          const int64_t q = lo + static_cast<int64_t>(t) * step;
          bool pred = false;                       // "position q is at or beyond the bound"
          if (q < hi) {
            const int32_t o = sl.yorder ? sl.yorder[q] : static_cast<int32_t>(q);
            const double yq = sl.xy[2 * o + 1];
            pred = side ? yq > yhi : yq >= ylo;
          }
          // first thread whose probe satisfies the predicate (monotone along t)
          const unsigned long long b = __ballot(pred);
          if ((t & 63) == 0) s_cnt4[t >> 6] = b ? (t + __ffsll(static_cast<long long>(b)) - 1) : GC_T;
          __syncthreads();
          int first = GC_T;
#pragma unroll
          for (int g = 0; g < GC_W; ++g) first = s_cnt4[g] < first ? s_cnt4[g] : first;
          __syncthreads();
          if (first == GC_T) {       // no probe at or beyond the bound: it lies after the
            const int64_t tv = (hi - lo - 1) / step;            // last probe made
            lo = lo + tv * step + 1;
          } else {                  // the bound lies in (probe[first - 1], probe[first]]
            const int64_t qf = lo + static_cast<int64_t>(first) * step;
            lo = first == 0 ? lo : lo + static_cast<int64_t>(first - 1) * step + 1;
            hi = qf;
          }
        }
        if (t == 0) s_win[side] = lo;
      }
    }
    __syncthreads();
    const int64_t wlo = s_win[0], whi = s_win[1];
#ifdef EPOS_GC_STATS
    if (t == 0) {
      atomicAdd(&g_gc_stats[0], 1ull);
      atomicAdd(&g_gc_stats[1], static_cast<unsigned long long>(whi - wlo));
      atomicAdd(&g_gc_stats[2], static_cast<unsigned long long>(sl.n));
    }
#endif
    for (int64_t c0 = wlo; c0 < whi; c0 += GC_T) {
      const int64_t c = c0 + t;
      if (c < whi) {
        const int32_t o = sl.yorder ? sl.yorder[c] : static_cast<int32_t>(c);
        GcCand r;
        r.x = sl.xy[2 * o]; r.y = sl.xy[2 * o + 1];
        r.X = sl.xyz[3 * o]; r.Y = sl.xyz[3 * o + 1]; r.Z = sl.xyz[3 * o + 2];
        r.q = BUILD ? 0 : gq[o];
        r.ol = o | (static_cast<int32_t>(BUILD ? 0 : lab_in[o]) << 30);
        c_rec[t] = r;
      }
      __syncthreads();
      const int cnt = whi - c0 < GC_T ? static_cast<int>(whi - c0) : GC_T;
      // branch-free, four candidates per trip: their twelve 16-byte LDS reads (wave-uniform
      // addresses: broadcasts) are issued together from clamped positions, the tests are
      // arithmetic (early-outs between dependent LDS reads ran at ~1500 cycles per candidate).
      for (int j0 = sub; j0 < cnt; j0 += 4 * GC_W) {
        GcCand r[4];
        int okj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * GC_W;
          okj[u] = j < cnt;
          r[u] = c_rec[okj[u] ? j : sub];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int lo_ = (r[u].ol >> 30) & 3;
          const int32_t co = r[u].ol & 0x3fffffff, cq = r[u].q;
          const double dx = px - r[u].x, dy = py - r[u].y;
          const double dX = pX - r[u].X, dY = pY - r[u].Y, dZ = pZ - r[u].Z;
          const int nb = okj[u] & static_cast<int>(act) & static_cast<int>(lo_ != 2) &
                         static_cast<int>(co != p) &
                         static_cast<int>(gc_dist2(dx, dy, dX, dY, dZ, ball.s2) <= ball.r2);
          if (BUILD) {
            if (nb) {              // position of the candidate: c0 + j
              const int64_t dl = c0 + (j0 + u * GC_W) - pos;
              if (nlist < NB_SUB && dl >= -32768 && dl <= 32767)
                nb_pool[(pos * GC_W + sub) * NB_SUB + nlist] = static_cast<int16_t>(dl);
              else
                ovf = true;
              ++nlist;
            }
          } else {
            deg += nb;
            S += nb ? cq : 0;
            n0 += nb & static_cast<int>(lo_ == 0);
          }
        }
      }
      __syncthreads();
    }
    if (BUILD) {
      if (valid) nb_cnt[pos * GC_W + sub] = static_cast<uint16_t>(ovf ? 0 : nlist);
      if (__any(valid && ovf) && pt == 0)
        __hip_atomic_store(w.nb_ok + s, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      continue;
    }
    }   // !use_lists
    s_deg[sub][pt] = deg; s_n0[sub][pt] = n0; s_S[sub][pt] = S;
    __syncthreads();
    if (sub == 0 && valid) {
      if (!act) {
        lab_out[p] = 2;
      } else {
        int64_t dg = 0, z0 = 0, Ss = 0;
#pragma unroll
        for (int g = 0; g < GC_W; ++g) { dg += s_deg[g][pt]; z0 += s_n0[g][pt]; Ss += s_S[g][pt]; }
        lab_out[p] = static_cast<uint8_t>(gc_decide(gq[p], dg, z0, Ss, ball.lam));
      }
    }
    __syncthreads();
  }
}

// ---- the same sweep with the candidates in SCALAR registers (round 3). A candidate is the
// same for all points of a tile, so it does not belong in vector registers or LDS at all:
// every wave walks a contiguous share (1 / GS_W) of the window through s_load (32 bytes of
// static geometry from w.geo + 16 bytes of GcDyn per candidate, position ordered) and the
// fifteen fp64 operations of the distance take the candidate's fields as SGPR operands. No
// staging through LDS, no barriers inside the window, no per-candidate index arithmetic; "not
// active" is Z = +inf instead of a label test, the point itself is counted like any other
// candidate and taken out once at the end, the residual sum runs in 32 bits per block of
// GS_BLOCK candidates. The scalar cache streams poorly (every line is a miss to L2 and few
// misses are in flight: GS_P = 1 ran at ~0.5 bytes per ns and CU pair), so a lane holds
// GS_P points -- a workgroup covers GS_P adjacent tiles, whose windows are nearly the same
// rows -- and every loaded candidate is tested GS_P times. The waves' partial counts meet in
// LDS by integer atomics (exact, order free). Same integers as ransac_gc_sweep<false>
// (tests/test_gpu_fit_lists.py runs both).
constexpr int GS_W = 16;                 // waves per workgroup: shares of the window
constexpr int GS_P = 1;                  // points per lane: adjacent tiles per workgroup
constexpr int GS_T = GS_W * 64;
constexpr int GS_BLOCK = 2048;           // 2048 x 2^20 < 2^32: the 32-bit sum cannot wrap

__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

struct __attribute__((aligned(32))) GcGeo { double x, y, X, Y; };
typedef double GsGeoV __attribute__((ext_vector_type(4)));      // x, y, X, Y
typedef int32_t GsDynV __attribute__((ext_vector_type(4)));     // Z (two words), q, out

__global__ __launch_bounds__(GS_T) void ransac_gc_scan(
    const int64_t* __restrict__ slot_base, EposFitParams prm, Work w,
    const GcGeo* __restrict__ geo_all, const GcDyn* __restrict__ dyn_in_all,
    GcDyn* __restrict__ dyn_out_all, const uint8_t* __restrict__ lab_in_all,
    uint8_t* __restrict__ lab_out_all, int8_t* __restrict__ flip_out_all) {
  const int s = blockIdx.y;
  if (w.state[s] != 1) return;
  __shared__ unsigned s_deg[GS_P * 64], s_n0[GS_P * 64];
  __shared__ unsigned long long s_S[GS_P * 64];
  const int t = threadIdx.x, pt = t & 63;
  const int sub = __builtin_amdgcn_readfirstlane(t >> 6);
  const Slot sl = slot_of(slot_base, s, w);
  const Ball ball = ball_of(prm);
  const GcGeo* __restrict__ geo = geo_all + sl.base;
  const GcDyn* __restrict__ dyn_in = dyn_in_all + sl.base;
  GcDyn* __restrict__ dyn_out = dyn_out_all + sl.base;
  const uint8_t* lab_in = lab_in_all + sl.base;
  uint8_t* lab_out = lab_out_all + sl.base;
  int8_t* __restrict__ flip_out = flip_out_all + sl.base;
  const GsGeoV* __restrict__ gv = reinterpret_cast<const GsGeoV*>(geo);
  const GsDynV* __restrict__ dv = reinterpret_cast<const GsDynV*>(dyn_in);
  const int64_t clast = sl.n - 1;
  const int64_t tiles = (sl.n + 63) / 64;
  FIT_TRACE(3, s == 0 && blockIdx.x == 0 && t == 0);
  for (int64_t grp = blockIdx.x; grp * GS_P < tiles; grp += gridDim.x) {
    const int64_t tile0 = grp * GS_P;
    const int64_t tile1 = tile0 + GS_P - 1 < tiles - 1 ? tile0 + GS_P - 1 : tiles - 1;
    const int64_t pos0 = tile0 * 64;
    // the group's candidate window: first tile's lower bound .. last tile's upper bound
    // (found once per call by ransac_init; the bounds are monotone along the order)
    const int32_t* wn = w.win + 2 * (sl.base / 64 + s);
    const int64_t wlo = uniform64(wn[2 * tile0]), whi = uniform64(wn[2 * tile1 + 1]);
    for (int i = t; i < GS_P * 64; i += GS_T) { s_deg[i] = 0u; s_n0[i] = 0u; s_S[i] = 0ull; }
#ifdef EPOS_GC_STATS
    if (t == 0) {
      atomicAdd(&g_gc_stats[0], 1ull);
      atomicAdd(&g_gc_stats[1], static_cast<unsigned long long>(whi - wlo));
      atomicAdd(&g_gc_stats[2], static_cast<unsigned long long>(sl.n));
    }
#endif
    double px[GS_P], py[GS_P], pX[GS_P], pY[GS_P], pZ[GS_P];
    uint32_t deg[GS_P], n0[GS_P], S32[GS_P];
    unsigned long long S[GS_P];
#pragma unroll
    for (int j = 0; j < GS_P; ++j) {
      const int64_t pos = pos0 + j * 64 + pt;
      const int64_t posc = pos < sl.n ? pos : clast;
      const GsGeoV mg = gv[posc];
      const GsDynV md = dv[posc];
      px[j] = mg.x; py[j] = mg.y; pX[j] = mg.z; pY[j] = mg.w;
      pZ[j] = __builtin_bit_cast(double, md.xy);
      deg[j] = 0; n0[j] = 0; S32[j] = 0; S[j] = 0;
    }
    __syncthreads();                                 // the LDS counters are zero
    FIT_TRACE(3, s == 0 && blockIdx.x == 0 && t == 0);
    const int64_t chunk = (whi - wlo + GS_W - 1) / GS_W;
    const int64_t ca = wlo + sub * chunk;
    const int64_t cb = ca + chunk < whi ? ca + chunk : whi;
// one candidate: its geometry (x, y, X, Y) and dynamic record (Z | q, out) arrive as whole
// 32- and 16-byte scalar loads and are tested against the lane's GS_P points
#define EPOS_GS_TEST(G, D)                                                                \
    {                                                                                     \
      const double cZ = __builtin_bit_cast(double, (D).xy);                               \
      _Pragma("unroll") for (int j = 0; j < GS_P; ++j) {                                  \
        const double dx = px[j] - (G).x, dy = py[j] - (G).y;                              \
        const double dX = pX[j] - (G).z, dY = pY[j] - (G).w, dZ = pZ[j] - cZ;             \
        const uint32_t nb = gc_dist2(dx, dy, dX, dY, dZ, ball.s2) <= ball.r2 ? 1u : 0u;   \
        deg[j] += nb;                                                                     \
        S32[j] += __umul24(nb, static_cast<uint32_t>((D).z));                             \
        n0[j] += __umul24(nb, static_cast<uint32_t>((D).w));                              \
      }                                                                                   \
    }
    for (int64_t c0 = ca; c0 < cb; c0 += GS_BLOCK) {
      const int64_t c1 = c0 + GS_BLOCK < cb ? c0 + GS_BLOCK : cb;
      int64_t c = c0;
      // two candidates in flight while two are tested (reads past the block are clamped to
      // the slot and never tested)
      GsGeoV ga0 = gv[c < clast ? c : clast], ga1 = gv[c + 1 < clast ? c + 1 : clast];
      GsDynV da0 = dv[c < clast ? c : clast], da1 = dv[c + 1 < clast ? c + 1 : clast];
      for (; c + 4 <= c1; c += 4) {
        const GsGeoV gb0 = gv[c + 2], gb1 = gv[c + 3];
        const GsDynV db0 = dv[c + 2], db1 = dv[c + 3];
        EPOS_GS_TEST(ga0, da0)
        EPOS_GS_TEST(ga1, da1)
        const int64_t e0 = c + 4 < clast ? c + 4 : clast, e1 = c + 5 < clast ? c + 5 : clast;
        ga0 = gv[e0]; ga1 = gv[e1]; da0 = dv[e0]; da1 = dv[e1];
        EPOS_GS_TEST(gb0, db0)
        EPOS_GS_TEST(gb1, db1)
      }
      if (c < c1) {                       // up to three left: ga0 / ga1 hold c, c + 1
        EPOS_GS_TEST(ga0, da0)
        if (c + 1 < c1) EPOS_GS_TEST(ga1, da1)
        if (c + 2 < c1) { const GsGeoV g2 = gv[c + 2]; const GsDynV d2_ = dv[c + 2]; EPOS_GS_TEST(g2, d2_) }
      }
#pragma unroll
      for (int j = 0; j < GS_P; ++j) { S[j] += S32[j]; S32[j] = 0; }
    }
#undef EPOS_GS_TEST
    FIT_TRACE(3, s == 0 && blockIdx.x == 0 && t == 0);
#pragma unroll
    for (int j = 0; j < GS_P; ++j) {
      atomicAdd(&s_deg[j * 64 + pt], deg[j]);
      atomicAdd(&s_n0[j * 64 + pt], n0[j]);
      atomicAdd(&s_S[j * 64 + pt], S[j]);
    }
    __syncthreads();
    // wave j (when there are fewer waves than tiles: j, j + GS_W, ...) decides tile j
    for (int j = sub; j < GS_P; j += GS_W) {
      const int64_t pos = pos0 + j * 64 + pt;
      if (pos >= sl.n) continue;
      const GsGeoV mg = gv[pos];
      const GsDynV md = dv[pos];
      const int32_t p = sl.yorder ? sl.yorder[pos] : static_cast<int32_t>(pos);
      const double mZ = __builtin_bit_cast(double, md.xy);
      GcDyn nd;
      nd.Z = mZ; nd.q = md.z; nd.out = 0;
      int8_t flip = 0;
      GcAcc raw;
      raw.deg = s_deg[j * 64 + pt]; raw.n0 = s_n0[j * 64 + pt]; raw.S = s_S[j * 64 + pt];
      w.acc[sl.base + pos] = raw;
      if (lab_in[p] == 2) {
        lab_out[p] = 2;
      } else {
        // the point met itself in the window
        const int inl = gc_decide_without_self(mg.x, mg.y, mg.z, mg.w, mZ, ball, s_deg[j * 64 + pt],
                                               s_n0[j * 64 + pt], s_S[j * 64 + pt], md.z, md.w);
        lab_out[p] = static_cast<uint8_t>(inl);
        nd.out = 1 - inl;
        flip = static_cast<int8_t>(nd.out - md.w);
      }
      dyn_out[pos] = nd;
      flip_out[pos] = flip;
    }
    __syncthreads();
    FIT_TRACE(3, s == 0 && blockIdx.x == 0 && t == 0);
  }
}

// ---- every FURTHER sweep of a round: the labels changed only at the positions the previous
// sweep flipped, and of a point's three sums only the count of outlier-labelled neighbours
// depends on labels at all. So the sweep after a full scan tests every point against the
// FLIPPED candidates of its window alone (typically a few percent of it):
//   raw_n0' = raw_n0 + sum over flipped neighbours of (+1: became outlier, -1: became inlier)
// -- integers, hence the same labels as another full scan (tests/test_gpu_fit_lists.py). One
// workgroup per tile: the window's flip bytes are read in chunks of 256 positions, the
// flipped candidates of a chunk are compacted into LDS with their geometry, wave g tests
// entries g, g + 4, ...
struct GdCand { double x, y, X, Y, Z; int32_t sign, pad; };

__global__ __launch_bounds__(256) void ransac_gc_delta(
    const int64_t* __restrict__ slot_base, EposFitParams prm, Work w,
    const GcGeo* __restrict__ geo_all, const GcDyn* __restrict__ dyn_all,
    const int8_t* __restrict__ flip_in_all, int8_t* __restrict__ flip_out_all,
    const uint8_t* __restrict__ lab_in_all, uint8_t* __restrict__ lab_out_all) {
  const int s = blockIdx.y;
  if (w.state[s] != 1) return;
  __shared__ __attribute__((aligned(16))) GdCand s_list[256];
  __shared__ int s_wcnt[4];
  __shared__ int s_dn0[64];
  const int t = threadIdx.x, pt = t & 63, sub = t >> 6;
  const Slot sl = slot_of(slot_base, s, w);
  const Ball ball = ball_of(prm);
  const GcGeo* __restrict__ geo = geo_all + sl.base;
  const GcDyn* __restrict__ dyn = dyn_all + sl.base;       // Z and q: the round's dyn_a
  const int8_t* __restrict__ flip_in = flip_in_all + sl.base;
  int8_t* __restrict__ flip_out = flip_out_all + sl.base;
  const uint8_t* lab_in = lab_in_all + sl.base;
  uint8_t* lab_out = lab_out_all + sl.base;
  GcAcc* acc = w.acc + sl.base;
  FIT_TRACE(5, s == 0 && blockIdx.x == 0 && t == 0);
  for (int64_t tile = blockIdx.x; tile * 64 < sl.n; tile += gridDim.x) {
    const int64_t pos = tile * 64 + pt;
    const bool valid = pos < sl.n;
    const int64_t posc = valid ? pos : sl.n - 1;
    const GcGeo me = geo[posc];
    const GcDyn md = dyn[posc];
    const int32_t* wn = w.win + 2 * (sl.base / 64 + s + tile);
    const int64_t wlo = wn[0], whi = wn[1];
    if (t < 64) s_dn0[t] = 0;
    int dn0 = 0;
    for (int64_t c0 = wlo; c0 < whi; c0 += 256) {
      const int64_t c = c0 + t;
      const int f = c < whi ? flip_in[c] : 0;
      const unsigned long long b = __ballot(f != 0);
      if (pt == 0) s_wcnt[sub] = __popcll(b);
      __syncthreads();                               // also: the list of the last chunk is done
      int off = 0, cnt = 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) { off += g < sub ? s_wcnt[g] : 0; cnt += s_wcnt[g]; }
      if (f != 0) {
        const GcGeo cg = geo[c];
        GdCand e;
        e.x = cg.x; e.y = cg.y; e.X = cg.X; e.Y = cg.Y; e.Z = dyn[c].Z; e.sign = f; e.pad = 0;
        s_list[off + __popcll(b & ((1ull << pt) - 1ull))] = e;
      }
      __syncthreads();
      for (int e = sub; e < cnt; e += 4) {
        const GdCand r = s_list[e];
        const double dx = me.x - r.x, dy = me.y - r.y;
        const double dX = me.X - r.X, dY = me.Y - r.Y, dZ = md.Z - r.Z;
        dn0 += gc_dist2(dx, dy, dX, dY, dZ, ball.s2) <= ball.r2 ? r.sign : 0;
      }
      __syncthreads();
    }
    if (dn0 != 0) atomicAdd(&s_dn0[pt], dn0);
    __syncthreads();
    if (sub == 0 && valid) {
      const int32_t p = sl.yorder ? sl.yorder[pos] : static_cast<int32_t>(pos);
      const int prev = lab_in[p];
      int8_t flip = 0;
      if (prev == 2) {
        lab_out[p] = 2;
      } else {
        GcAcc raw = acc[pos];
        raw.n0 = static_cast<uint32_t>(static_cast<int>(raw.n0) + s_dn0[pt]);
        acc[pos] = raw;                                // the next sweep continues from here
        const int out_prev = 1 - prev;                 // label 1 = inlier
        const int inl = gc_decide_without_self(me.x, me.y, me.X, me.Y, md.Z, ball, raw.deg, raw.n0,
                                               raw.S, md.q, out_prev);
        lab_out[p] = static_cast<uint8_t>(inl);
        flip = static_cast<int8_t>((1 - inl) - out_prev);
      }
      flip_out[pos] = flip;
    }
    __syncthreads();
  }
  FIT_TRACE(5, s == 0 && blockIdx.x == 0 && t == 0);
}

}  // namespace
}  // namespace epos
