// Pose fitting, the local optimisation: the 6 x 6 solve, the canonical sums of one or LO_G
// cooperating workgroups (LoSync, lo_combine), one Gauss-Newton pass (lo_pass) and the refit
// loop over it (lo_refine). Included after fit_work.h (reproj, PointBatch, Work, FIT_TRACE).
#pragma once

namespace epos {
namespace {

// ------------------------------------------------- local optimisation --
__device__ void orthonormalize(double* R) {
  const double n0 = sqrt(dot3(R, R));
  for (int j = 0; j < 3; ++j) R[j] /= n0;
  const double d = dot3(R, R + 3);
  for (int j = 0; j < 3; ++j) R[3 + j] -= d * R[j];
  const double n1 = sqrt(dot3(R + 3, R + 3));
  for (int j = 0; j < 3; ++j) R[3 + j] /= n1;
  cross3(R, R + 3, R + 6);
}

// Gaussian elimination WITHOUT pivoting, the arithmetic of the C definition's solve6
// operation for operation: H = J^T J is symmetric positive (semi)definite, so that is stable,
// and one reciprocal per pivot serves the column and the back-substitution. Every index is a
// compile-time constant so that the 6 x 7 system stays in registers (an indexed form goes
// through scratch memory: ~300 dependent private loads and stores per thread and pass).
__device__ int solve6(const double* H /*[36]*/, const double* g, double* x) {
  double A[6][7], inv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) A[i][j] = H[i * 6 + j];
    A[i][6] = -g[i];
  }
  bool bad = false;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    bad = bad || !(A[c][c] > 1e-300);
    inv[c] = 1.0 / A[c][c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double fct = A[r][c] * inv[c];
#pragma unroll
      for (int j = c + 1; j < 7; ++j) A[r][j] -= fct * A[c][j];
    }
  }
  if (bad) return 1;
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double sacc = A[i][6];
#pragma unroll
    for (int j = i + 1; j < 6; ++j) sacc -= A[i][j] * x[j];
    x[i] = sacc * inv[i];
  }
  return 0;
}

// ---- sums of the local optimisation ------------------------------------------------------
// Canonical order over P = 256 * G strided partials (partial q takes items q, q + P, ...):
// the xor butterfly inside each group of 64, (w0 + w1) + (w2 + w3) inside each group of 256,
// then (W0 + W1) + (W2 + W3) over the G = 4 groups of 256 (G = 1: the group of 256 alone).
// G = 1 is one 256-thread workgroup (joint refinement). G = LO_G = 4 (round 3): FOUR
// workgroups per slot, workgroup g owning partials [256 g, 256 g + 256): each pass of a refit
// is a latency-bound sweep over the slot's correspondences (a dependent gather and ~250 fp64
// operations per item), so four workgroups on four CUs shorten it almost four-fold; the
// sixteen wave sums meet in global memory (the fence-free agent-scope hand-off of lo_combine)
// and every workgroup combines them in the same order, so all of them continue with
// identical values and identical control flow. The siblings of a slot have adjacent block
// indices, i.e. the same position in their XCDs' dispatch order: whenever one of them is
// resident the others are or are about to be; the spin is bounded anyway (lo_timeout).
constexpr int LO_G = 4;
constexpr int LO_NV = 32;            // doubles per wave row (27 sums, score, count)
constexpr unsigned LO_SPIN_MAX = 1u << 24;

struct LoSync {
  int trace = 0;        // EPOS_FIT_TRACE: this workgroup stamps the phases of its passes
  unsigned* cnt;        // this launch's counter of the slot (null: single workgroup)
  double* data;         // [2][LO_G * 4][LO_NV]
  int32_t* timeout;
  unsigned spin_max;    // polls before a workgroup gives up on its siblings (Work::lo_spin_max)
  int g;                // workgroup index within the slot
  unsigned epoch;       // exchanges done so far in this launch
};
// workgroup g of slot s in the cooperating launch number lo_launch (of n_lo) of the call
__device__ __forceinline__ LoSync lo_sync_of(const Work& w, int s, int g, int lo_launch, int n_lo) {
  return {0, w.lo_cnt + static_cast<int64_t>(s) * n_lo + lo_launch,
          w.lo_data + static_cast<int64_t>(s) * (2 * LO_G * 4 * LO_NV), w.lo_timeout,
          w.lo_spin_max, g, 0u};
}

// The wave sums of up to 32 quantities at once. A butterfly per quantity (wave_sum:
// xor 32, 16, ... 1, every lane ends with the total) moves 6 x 2 words per quantity; here the
// first five levels HALVE the set instead -- at the level of xor-distance d a lane keeps the
// quantities whose next index bit equals its own bit d and receives its partner's copies of
// exactly those -- so 16 + 8 + 4 + 2 + 1 + 1 values cross lanes instead of 6 x 32. Every
// quantity is still summed over the same pairs in the same order (a + b == b + a bit for
// bit), i.e. the canonical tree of the oracle's tree64. Lane l ends with the total of
// quantity lo_owned(l).
__device__ __forceinline__ int lo_owned(int lane) {        // bits 5..1 of the lane, reversed
  return ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2) |
         (((lane >> 2) & 1) << 3) | (((lane >> 1) & 1) << 4);
}
__device__ __forceinline__ double reduce_scatter32(double (&a)[32], int lane) {
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int off = 32 >> k;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < (16 >> k); ++i) {
      const double keep = up ? a[2 * i + 1] : a[2 * i];
      const double send = up ? a[2 * i] : a[2 * i + 1];
      a[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  return a[0] + __shfl_xor(a[0], 1, 64);
}

// val: the total over this WAVE of quantity lo_owned(lane) (reduce_scatter32). Returns the
// canonical totals in comb[0..nv) (LDS, valid for every thread after the call). s_rows:
// LDS [4][LO_NV].
__device__ void lo_combine(LoSync& sy, double val, int nv, int t, double* s_rows,
                           double* comb) {
  const int lane = t & 63, wave = t >> 6;
  const int own = lo_owned(lane);
  const bool writer = (lane & 1) == 0 && own < nv;
  if (sy.cnt == nullptr) {                       // one workgroup: through LDS only
    if (writer) s_rows[wave * LO_NV + own] = val;
    __syncthreads();
    if (t < nv)
      comb[t] = (s_rows[t] + s_rows[LO_NV + t]) + (s_rows[2 * LO_NV + t] + s_rows[3 * LO_NV + t]);
    __syncthreads();
    return;
  }
  // The exchanged words are written and read by AGENT-SCOPE ATOMIC stores / loads (sc1: they
  // are coherent across the XCDs' L2s by themselves), so the hand-off needs no release /
  // acquire fence -- on this part a fence is a write-back / invalidate of the whole L2,
  // which costs microseconds while other streams' GEMMs keep it dirty: every storing wave
  // waits for its stores to complete, the workgroup meets, ONE relaxed ticket, relaxed
  // polling, and the reads are issued after the poll returned (they depend on it).
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(sy.data) +
                            (sy.epoch & 1u) * (LO_G * 4 * LO_NV);
  if (writer)
    __hip_atomic_store(buf + (sy.g * 4 + wave) * LO_NV + own,
                       __builtin_bit_cast(unsigned long long, val), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains
  __syncthreads();
  if (t == 0) {
    __hip_atomic_fetch_add(sy.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = LO_G * (sy.epoch + 1u);
    unsigned spins = 0;
    while (__hip_atomic_load(sy.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      // a hand-off of this launch has already timed out (the call will report
      // num_models = -1): do not spin the full budget again at every later exchange
      if ((spins & 255u) == 255u &&
          __hip_atomic_load(sy.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        break;
      if (++spins > sy.spin_max) {
        __hip_atomic_store(sy.timeout, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (t < nv) {
    double W[LO_G];
#pragma unroll
    for (int g = 0; g < LO_G; ++g) {
      const unsigned long long* r = buf + (g * 4) * LO_NV + t;
      double r4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        r4[q] = __builtin_bit_cast(double, __hip_atomic_load(r + q * LO_NV, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
      W[g] = (r4[0] + r4[1]) + (r4[2] + r4[3]);
    }
    comb[t] = (W[0] + W[1]) + (W[2] + W[3]);
  }
  __syncthreads();
  ++sy.epoch;
}

struct LoLds {                 // LDS of a local-optimisation workgroup
  double rows[4 * LO_NV];
  double comb[LO_NV];
};

// One pass over the correspondences idx[0..m) (idx == nullptr: 0..m) that yields
//   * SCORE: the MSAC score and inlier count of `pose` at thr2,
//   * the Gauss-Newton step from `pose` on its members -- lab == nullptr: the inliers at
//     thr2; otherwise the points with lab[p] == sel (fixed membership, full weight) --
//     as the next pose (returns 1 when the normal equations are singular / non-finite).
// One pass per refit: the step of an accepted candidate is already there when the next
// refit starts. All sums in the canonical order of lo_combine (G = 1 or LO_G workgroups).
template <bool SCORE>
__device__ int lo_pass(const double* pose, const double* K, const double* xy,
                       const double* xyz, const int32_t* idx, int64_t m, double thr2, int t,
                       LoSync& sy, LoLds* lds, const uint8_t* lab, int sel, double* score,
                       int* count, double* next) {
  const int G = sy.cnt ? LO_G : 1;
  const int stride = 256 * G;
  const double inv_thr2 = 1.0 / thr2;
  double acc[32];
#pragma unroll
  for (int v = 0; v < 32; ++v) acc[v] = 0.0;
  int cnt = 0;
  FIT_TRACE(4, sy.trace && t == 0);
  for (int64_t i0 = static_cast<int64_t>(sy.g) * 256 + t; i0 < m;
       i0 += static_cast<int64_t>(stride) * PF) {
    PointBatch pb;
    pb.load(xy, xyz, idx, i0, stride, m);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (!pb.ok[u]) continue;
      double e2, Xc[3], r[2];
      if (reproj(pose, K, pb.x2[u], pb.x3[u], &e2, Xc, r)) continue;
      const bool inl = e2 < thr2;
      if (SCORE && inl) { acc[27] += 1.0 - e2 * inv_thr2; ++cnt; }
      if (lab ? lab[pb.p[u]] != sel : !inl) continue;
      const double iz = 1.0 / Xc[2];
      const double a0 = K[0] * iz, a1 = K[1] * iz,
                   a2 = -(K[0] * Xc[0] + K[1] * Xc[1]) * iz * iz;
      const double b1 = K[4] * iz, b2 = -(K[4] * Xc[1]) * iz * iz;
      double J0[6], J1[6];
      // Xc(w) = Xc - [Xc]x w: row . (-[Xc]x)  (sign fixed in round 2)
      J0[0] = -a1 * Xc[2] + a2 * Xc[1];
      J0[1] = a0 * Xc[2] - a2 * Xc[0];
      J0[2] = -a0 * Xc[1] + a1 * Xc[0];
      J0[3] = a0; J0[4] = a1; J0[5] = a2;
      J1[0] = -b1 * Xc[2] + b2 * Xc[1];
      J1[1] = -b2 * Xc[0];
      J1[2] = b1 * Xc[0];
      J1[3] = 0.0; J1[4] = b1; J1[5] = b2;
      int v = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) { acc[v] += J0[a] * J0[b] + J1[a] * J1[b]; ++v; }
#pragma unroll
      for (int a = 0; a < 6; ++a) { acc[v] += J0[a] * r[0] + J1[a] * r[1]; ++v; }
    }
  }
  constexpr int NV = SCORE ? 29 : 27;
  FIT_TRACE(4, sy.trace && t == 0);
  if (SCORE) acc[28] = static_cast<double>(cnt);     // exact in any order: counts < 2^31
  const double mine = reduce_scatter32(acc, t & 63);
  FIT_TRACE(4, sy.trace && t == 0);
  lo_combine(sy, mine, NV, t, lds->rows, lds->comb);
  FIT_TRACE(4, sy.trace && t == 0);
  const double* tot = lds->comb;
  if (SCORE) {
    *score = tot[27];
    *count = static_cast<int>(tot[28]);
  }
  double H[36], g[6], x[6];
  {
    int v = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) { H[a * 6 + b] = tot[v]; H[b * 6 + a] = tot[v]; ++v; }
#pragma unroll
    for (int a = 0; a < 6; ++a) g[a] = tot[v++];
  }
  __syncthreads();               // every thread has read the totals: comb may be reused
  if (solve6(H, g, x)) return 1;
  double qw = 1.0, qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  double dR[9];
  dR[0] = 1.0 - 2.0 * (qy * qy + qz * qz); dR[1] = 2.0 * (qx * qy - qz * qw); dR[2] = 2.0 * (qx * qz + qy * qw);
  dR[3] = 2.0 * (qx * qy + qz * qw); dR[4] = 1.0 - 2.0 * (qx * qx + qz * qz); dR[5] = 2.0 * (qy * qz - qx * qw);
  dR[6] = 2.0 * (qx * qz - qy * qw); dR[7] = 2.0 * (qy * qz + qx * qw); dR[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      next[i * 3 + j] = dR[i * 3] * pose[j] + dR[i * 3 + 1] * pose[3 + j] + dR[i * 3 + 2] * pose[6 + j];
    next[9 + i] = dR[i * 3] * pose[9] + dR[i * 3 + 1] * pose[10] + dR[i * 3 + 2] * pose[11] + x[3 + i];
  }
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 12; ++i) bad = bad || !(next[i] == next[i]);
  FIT_TRACE(4, sy.trace && t == 0);
  return bad ? 1 : 0;
}

// The refits of one proposal, in place: a first pass steps from `pose` (SCORE_FIRST: and
// rescores it; otherwise its score and count are the known ones), then up to lo_iters passes
// that score the candidate and step from it. A candidate is kept iff it scores higher; the loop
// ends when the relative gain falls to LO_MIN_GAIN. Members: as in lo_pass, sel = 1. TRACE_ROW
// / stamp: the calling kernel's FIT_TRACE row and whether this thread stamps.
template <bool SCORE_FIRST, int TRACE_ROW>
__device__ __forceinline__ void lo_refine(double* pose, double* best_score, int* best_count,
                                          const Slot& sl, const Camera& cam,
                                          const int32_t* idx, int64_t m, int t, LoSync& sy,
                                          LoLds* lds, const uint8_t* lab, int lo_iters,
                                          bool stamp) {
  double cand[12];
  FIT_TRACE(TRACE_ROW, stamp);
  int fail = lo_pass<SCORE_FIRST>(pose, cam.K, sl.xy, sl.xyz, idx, m, cam.thr2, t, sy, lds, lab,
                                  1, best_score, best_count, cand);
  FIT_TRACE(TRACE_ROW, stamp);
  for (int li = 0; li < lo_iters && !fail; ++li) {
    double sc, cand2[12];
    int cnt;
    const int fail2 = lo_pass<true>(cand, cam.K, sl.xy, sl.xyz, idx, m, cam.thr2, t, sy, lds,
                                    lab, 1, &sc, &cnt, cand2);
    FIT_TRACE(TRACE_ROW, stamp);
    if (!(sc > *best_score)) break;
    const double gain = sc - *best_score;
    *best_score = sc; *best_count = cnt;
    for (int i = 0; i < 12; ++i) { pose[i] = cand[i]; cand[i] = cand2[i]; }
    fail = fail2;
    if (!(gain > LO_MIN_GAIN * sc)) break;        // converged: further steps are noise
  }
}

}  // namespace
}  // namespace epos
