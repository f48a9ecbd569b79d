// Pose fitting, the joint refinement of multi-instance slots: labels over all instances by
// synchronous sweeps of a Potts energy, one Gauss-Newton refit per instance, kept iff the
// energy dropped. Included after fit_lo.h (lo_pass, LoSync) and fit_label.h (the neighbour
// lists and for_each_neighbour).
#pragma once

namespace epos {
namespace {

// ------------------------------------------------ joint refinement (PEARL's role) --
// For slots with 2 <= k <= max_model_number_for_optimization accepted instances, over
// ALL correspondences of the slot: labels {0..k-1, k = outlier}; data term
// D_p(m) = min(e_pm^2 / (1.5 tau)^2, 1), D_p(outlier) = (tau / 1.5 tau)^2; degree-
// normalised Potts smoothness (a point pays lambda times the fraction of its neighbours
// with another label); everything in 2^-20 fixed point (exact integer sums: order
// independent). One iteration = gc_sweeps synchronous relabelling sweeps + one Gauss-Newton
// refit of every instance on its points, kept iff the energy dropped.
constexpr int PEARL_MAX_K = 8;
static_assert(PEARL_DT == PEARL_MAX_K + 1, "one data-term column per label incl. the outlier");
constexpr int PEARL_BINS = 64;    // bins per energy sum (the workgroups' atomics spread over them)
static_assert(4 * PEARL_BINS == 256, "pearl_begin zeroes the bins with one 256-thread workgroup");

__device__ __forceinline__ int64_t pearl_data_term(const double* pose, const double* K,
                                                   const double* xy2, const double* xyz3,
                                                   double tthr2) {
  double e2, Xc[3], r[2];
  if (reproj(pose, K, xy2, xyz3, &e2, Xc, r)) return GC_Q;
  double d = e2 / tthr2;
  if (!(d < 1.0)) d = 1.0;
  return static_cast<int64_t>(d * static_cast<double>(GC_Q));
}

__global__ void pearl_setup(const int32_t* num_models, EposFitParams prm, Work w, int S) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int k = num_models[s];
  w.pearl_state[s] = (k >= 2 && k <= PEARL_MAX_K && k <= prm.max_model_number_for_optimization &&
                      gc_enabled(prm, false) && prm.gc_sweeps >= 1) ? 1 : 0;
}

// The degree-normalised Potts term: the FRACTION of a point's `deg` neighbours that hold
// another label (`other` of them), in 2^-20 fixed point. With lists deg <= NB_W * NB_SUB = 640:
// the numerator stays below 2^29 and a 32-bit division gives the same integer.
template <bool LISTS>
__device__ __forceinline__ int64_t potts_fraction(int other, int deg) {
  static_assert(static_cast<int64_t>(GC_Q) * NB_W * NB_SUB < (1ll << 31), "32-bit quotient");
  if (deg <= 0) return 0;
  if constexpr (LISTS)
    return static_cast<int64_t>(static_cast<uint32_t>(GC_Q * other) / static_cast<uint32_t>(deg));
  return (static_cast<int64_t>(GC_Q) * other) / deg;
}

// A workgroup's share of the slot's energy sums `first` (data) and `first` + 1 (smoothness) of
// Work::pearl_acc (0, 1: before the refit; 2, 3: after): the threads with `adds` meet in LDS,
// then ONE pair of global atomics, spread over PEARL_BINS addresses (pearl_commit adds them).
__device__ __forceinline__ void pearl_publish(const Work& w, int s, int first, bool adds,
                                              unsigned long long data, unsigned long long smooth) {
  __shared__ unsigned long long s_sum[2];
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0ull;
  __syncthreads();
  if (adds) {
    atomicAdd(&s_sum[0], data);
    atomicAdd(&s_sum[1], smooth);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_sum[threadIdx.x] != 0ull)
    atomicAdd(&w.pearl_acc[(s * 4 + first + threadIdx.x) * PEARL_BINS +
                           (blockIdx.x & (PEARL_BINS - 1))], s_sum[threadIdx.x]);
}

__global__ __launch_bounds__(256) void pearl_begin(const int64_t* slot_base,
                                                   const int32_t* num_models, Work w,
                                                   const int32_t* labels_all) {
  const int s = blockIdx.y;
  if (!w.pearl_state[s]) return;
  const int64_t base = slot_base[s], n = slot_base[s + 1] - base;
  const int k = num_models[s];
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int32_t l = labels_all[base + i];
    const int64_t pos = w.ypos ? w.ypos[base + i] : i;       // the sweeps' labels: position order
    w.lab_a[base + pos] = static_cast<uint8_t>(l >= 0 && l < k ? l : k);
  }
  if (blockIdx.x == 0) w.pearl_acc[s * (4 * PEARL_BINS) + threadIdx.x] = 0ull;   // 4 x 64 bins
  if (blockIdx.x == 0 && threadIdx.x == 0) w.pearl_moved[s] = 0;
}

// Data terms of every point of a slot against the k poses (which = 0: the accepted ones,
// 1: the candidates of pearl_refit) -> Work::pearl_dt, one thread per point. The sweeps and
// the energy pass then only walk neighbours: the fp64 reprojection inside them, one point per
// wave, idles 61 of 64 lanes and costs the walk three of eight waves per SIMD (profiles/r04).
__global__ __launch_bounds__(256) void pearl_data(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const double* __restrict__ Ks,
    const int32_t* __restrict__ num_models, EposFitParams prm, int max_k, Work w,
    const double* __restrict__ poses, int which) {
  const int s = blockIdx.y;
  if (!w.pearl_state[s]) return;
  if (which == 1 && !w.pearl_moved[s]) return;
  const int64_t base = slot_base[s], n = slot_base[s + 1] - base;
  const int k = num_models[s];
  const double* pp = which ? w.pearl_pose + static_cast<int64_t>(s) * PEARL_MAX_K * 12
                           : poses + static_cast<int64_t>(s) * max_k * 12;
  const Camera cam = camera_of(Ks, s, prm);
  const double tthr = 1.5 * prm.threshold, tthr2 = tthr * tthr;
  const int32_t d_out = static_cast<int32_t>(
      static_cast<int64_t>((cam.thr2 / tthr2) * static_cast<double>(GC_Q)));
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * 256) {
    int32_t* row = w.pearl_dt + (base + p) * PEARL_DT;
    for (int m = 0; m < k; ++m)
      row[m] = static_cast<int32_t>(
          pearl_data_term(pp + 12 * m, cam.K, xy_all + 2 * (base + p), xyz_all + 3 * (base + p), tthr2));
    row[k] = d_out;
  }
}

// which = 0: energy of (accepted poses, lab) -> acc[0..1]; 1: of (candidate poses, lab).
// `lab_all`: labels in POSITION order; the data terms come from Work::pearl_dt (pearl_data
// with the same `which` runs before this launch).
template <bool LISTS>
__global__ __launch_bounds__(256) void pearl_energy(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const int32_t* __restrict__ num_models,
    EposFitParams prm, Work w, const uint8_t* __restrict__ lab_all, int which) {
  const int s = blockIdx.y;
  if (!w.pearl_state[s] || (w.nb_ok[s] != 0) != LISTS) return;
  if (which == 1 && !w.pearl_moved[s]) return;
  const int lane = threadIdx.x & 63;
  const Slot sl = slot_of(slot_base, s, w, xy_all, xyz_all);
  const Ball ball = ball_of(prm);
  const uint8_t* lab = lab_all + sl.base;
  const int k = num_models[s];
  const NbLists nl = nb_lists_of(w, s, sl);
  // Only as many workgroups take part as give every wave ~2 points (the grid is sized for the
  // pool's capacity): with one point and one pair of atomics per wave the 130 000 same-address
  // 64-bit atomics of a C4 image serialised at ~7 ns each, 0.93 ms per launch (profiles/r03).
  const int64_t want = (sl.n + 7) / 8;
  const int wgs = static_cast<int>(want < 1 ? 1 : want < gridDim.x ? want : gridDim.x);
  if (static_cast<int>(blockIdx.x) >= wgs) return;
  const int nwaves = wgs * 4;
  unsigned long long data = 0, smooth = 0;
  for (int64_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < sl.n; p += nwaves) {
    const int lp = lab[sl.ypos ? sl.ypos[p] : p];
    const int64_t dterm = w.pearl_dt[(sl.base + p) * PEARL_DT + (lp < k ? lp : k)];
    int diff = 0, deg = 0;
    for_each_neighbour<LISTS>(sl, ball, static_cast<int32_t>(p), lane, nl,
                              [&](int64_t q, bool valid) {
                                const int lo = lab[q];
                                deg += valid;
                                diff += valid && lo != lp;
                              });
    diff = wave_sum(diff);
    deg = wave_sum(deg);
    if (lane == 0) {
      smooth += static_cast<unsigned long long>(potts_fraction<LISTS>(diff, deg));
      data += static_cast<unsigned long long>(dterm);
    }
  }
  pearl_publish(w, s, 2 * which, lane == 0, data, smooth);
}

template <bool LISTS>
__global__ __launch_bounds__(256) void pearl_sweep(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const int32_t* __restrict__ num_models,
    EposFitParams prm, Work w, const uint8_t* __restrict__ lab_in_all,
    uint8_t* __restrict__ lab_out_all, int with_energy, uint8_t* __restrict__ lab_idx_all) {
  // lab_in / lab_out: labels in POSITION order (row-sorted; what the neighbour walk indexes);
  // lab_idx_all (the last sweep of an iteration, else null): the same labels in index order
  // for pearl_refit / pearl_commit. Data terms: Work::pearl_dt (pearl_data runs before).
  // with_energy (the FIRST sweep of an iteration): the energy of (poses, lab_in) -- the
  // "before" of pearl_commit's comparison -- falls out of this pass: a point's disagreeing
  // neighbours are deg - cnt[its label] and its data term is one of the k + 1 this pass
  // evaluates anyway (two pearl_energy launches per call less; same integers, same bins).
  const int s = blockIdx.y;
  if (!w.pearl_state[s] || (w.nb_ok[s] != 0) != LISTS) return;
  const int lane = threadIdx.x & 63;
  const Slot sl = slot_of(slot_base, s, w, xy_all, xyz_all);
  const Ball ball = ball_of(prm);
  const uint8_t* lab_in = lab_in_all + sl.base;
  uint8_t* lab_out = lab_out_all + sl.base;
  const int k = num_models[s];
  const NbLists nl = nb_lists_of(w, s, sl);
  const int nwaves = gridDim.x * 4;
  unsigned long long e_data = 0, e_smooth = 0;
  for (int64_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < sl.n; p += nwaves) {
    // Lane m (m <= k) owns label m: its data term, then (after the walk) its cost.
    const int64_t pos = sl.ypos ? sl.ypos[p] : p;
    const int lp = lab_in[pos];
    const int ml = lane <= k ? lane : k;
    const int64_t D = w.pearl_dt[(sl.base + p) * PEARL_DT + ml];
    int deg = 0, mine = 0;
    if constexpr (LISTS) {
      // at most 640 neighbours: the nine label counts ride in three words, ten bits each
      // (a third of the registers and of the wave reductions; the sums are the same integers)
      static_assert(NB_W * NB_SUB < 1024 && PEARL_MAX_K + 1 <= 9, "three 10-bit fields per word");
      unsigned pk[3] = {0u, 0u, 0u};
      for_each_neighbour<true>(sl, ball, static_cast<int32_t>(p), lane, nl,
                               [&](int64_t q, bool valid) {
                                 const unsigned l = lab_in[q];
                                 const unsigned wd = l / 3u, sh = 10u * (l - 3u * wd);
                                 const unsigned one = valid && l <= PEARL_MAX_K ? 1u << sh : 0u;
#pragma unroll
                                 for (int i = 0; i < 3; ++i) pk[i] += wd == i ? one : 0u;
                               });
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pk[i] = wave_sum(pk[i]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int c = static_cast<int>((pk[i] >> (10 * j)) & 1023u);
          deg += c;
          mine = lane == 3 * i + j ? c : mine;
        }
      }
    } else {
      int cnt[PEARL_MAX_K + 1];
#pragma unroll
      for (int m = 0; m <= PEARL_MAX_K; ++m) cnt[m] = 0;
      for_each_neighbour<false>(sl, ball, static_cast<int32_t>(p), lane, nl,
                                [&](int64_t q, bool valid) {
                                  const int l = lab_in[q];
                                  const int lo = valid ? l : -1;
#pragma unroll
                                  for (int m = 0; m <= PEARL_MAX_K; ++m) cnt[m] += lo == m;
                                });
#pragma unroll
      for (int m = 0; m <= PEARL_MAX_K; ++m) {
        cnt[m] = wave_sum(cnt[m]);
        deg += cnt[m];
        mine = lane == m ? cnt[m] : mine;
      }
    }
    // lane m: the cost of label m
    const int64_t sm = potts_fraction<LISTS>(deg - mine, deg);
    const double c = (1.0 - ball.lam) * static_cast<double>(D) + ball.lam * static_cast<double>(sm);
    int best = 0;
    double best_c = __shfl(c, 0, 64);
    for (int m = 1; m <= k; ++m) {                      // k is uniform; first minimum wins
      const double cm = __shfl(c, m, 64);
      if (cm < best_c) { best = m; best_c = cm; }
    }
    if (lane == 0) {
      lab_out[pos] = static_cast<uint8_t>(best);
      if (lab_idx_all) lab_idx_all[sl.base + p] = static_cast<uint8_t>(best);
    }
    if (with_energy && (lane == lp || (lane == k && lp >= k)) && lane <= k) {
      e_data += static_cast<unsigned long long>(D);
      e_smooth += static_cast<unsigned long long>(sm);
    }
  }
  if (with_energy)                // as pearl_energy(which = 0); the lanes that own labels add
    pearl_publish(w, s, 0, lane <= PEARL_MAX_K && (e_data | e_smooth) != 0ull, e_data, e_smooth);
}

__global__ __launch_bounds__(256) void pearl_refit(
    const double* __restrict__ xy_all, const double* __restrict__ xyz_all,
    const int64_t* __restrict__ slot_base, const double* __restrict__ Ks,
    const int32_t* __restrict__ num_models, EposFitParams prm, int max_k, Work w,
    const double* __restrict__ poses, const uint8_t* __restrict__ lab_all) {
  const int s = blockIdx.x;
  if (!w.pearl_state[s]) return;
  const int t = threadIdx.x;
  __shared__ LoLds s_lo;
  __shared__ int s_cnt[4];
  LoSync sy;                         // one workgroup: the sums stay in LDS
  sy.cnt = nullptr; sy.data = nullptr; sy.timeout = nullptr; sy.spin_max = 0; sy.g = 0; sy.epoch = 0;
  const int64_t base = slot_base[s], n = slot_base[s + 1] - base;
  const double* xy = xy_all + 2 * base;
  const double* xyz = xyz_all + 3 * base;
  const uint8_t* lab = lab_all + base;
  const int k = num_models[s];
  double K[9];
  for (int i = 0; i < 9; ++i) K[i] = Ks[s * 9 + i];
  const double thr2 = prm.threshold * prm.threshold;
  // one workgroup per (slot, model): the refits of a slot's models are independent
  const int m = blockIdx.y;
  if (m >= k) return;
  {
    double pose[12], next[12];
    for (int i = 0; i < 12; ++i) pose[i] = poses[(static_cast<int64_t>(s) * max_k + m) * 12 + i];
    int c = 0;
    for (int64_t i = t; i < n; i += 256) c += lab[i] == m;
    c = wave_sum(c);
    if ((t & 63) == 0) s_cnt[t >> 6] = c;
    __syncthreads();
    c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
    bool ok = false;
    if (c >= prm.min_point_number)                         // uniform
      ok = !lo_pass<false>(pose, K, xy, xyz, nullptr, n, thr2, t, sy, &s_lo, lab, m, nullptr,
                           nullptr, next);
    if (t < 12) w.pearl_pose[(static_cast<int64_t>(s) * PEARL_MAX_K + m) * 12 + t] =
        ok ? next[t] : pose[t];
    if (t == 0 && ok) atomicOr(&w.pearl_moved[s], 1);         // zeroed by pearl_begin
  }
}

__global__ __launch_bounds__(256) void pearl_commit(const int64_t* slot_base,
                                                    const int32_t* num_models,
                                                    EposFitParams prm, int max_k, Work w,
                                                    double* poses, const uint8_t* lab_all,
                                                    int32_t* labels_all) {
  const int s = blockIdx.x;
  if (!w.pearl_state[s]) return;
  const int t = threadIdx.x;
  const int k = num_models[s];
  const double lam = prm.spatial_coherence_weight;
  unsigned long long a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned long long v = 0;
    for (int b = 0; b < PEARL_BINS; ++b) v += w.pearl_acc[(s * 4 + q) * PEARL_BINS + b];
    a[q] = v;
  }
  const double e_before = (1.0 - lam) * static_cast<double>(static_cast<int64_t>(a[0])) +
                          lam * static_cast<double>(static_cast<int64_t>(a[1]));
  const double e_after = (1.0 - lam) * static_cast<double>(static_cast<int64_t>(a[2])) +
                         lam * static_cast<double>(static_cast<int64_t>(a[3]));
  const bool keep = w.pearl_moved[s] && e_after < e_before;   // uniform
  __syncthreads();
  if (!keep) { if (t == 0) w.pearl_state[s] = 0; return; }
  const int64_t base = slot_base[s], n = slot_base[s + 1] - base;
  for (int i = t; i < k * 12; i += 256)
    poses[static_cast<int64_t>(s) * max_k * 12 + i] =
        w.pearl_pose[static_cast<int64_t>(s) * PEARL_MAX_K * 12 + i];
  for (int64_t i = t; i < n; i += 256) {
    const int l = lab_all[base + i];
    labels_all[base + i] = l < k ? l : -1;
  }
}

}  // namespace
}  // namespace epos
