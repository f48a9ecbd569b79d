// project_to_surface for the pooled correspondence rows, in place, through a mesh index
// (the stage between epos_corr_fill and the ordering / fitting stages when the pipeline is
// built with project_to_surface=True). Same result as the exhaustive sweep of corresp.hip
// (project_to_mesh_kernel), bit for bit: every face that is evaluated runs the same
// closest_on_triangle, the winner is the minimum of (d2, original face index), and a subtree is
// skipped only when a lower bound of EVERY d2 the sweep could compute below it is strictly
// greater than the best d2 so far ("Mesh index": why the bound holds in floating
// point, which faces stay out of the tree, which queries sweep everything).
//
// One wavefront per row, as in the sweep. The index (epos_amd/mesh_index.py) is an implicit
// 64-ary tree: at an inner node lane j bounds child j (one coalesced load of the group's six
// box planes), at a leaf lane j evaluates face j. No stack in memory: per level one 64-bit
// mask of the children still to visit (wave-uniform) and one bound per lane, in registers;
// the level is wave-uniform, so selecting among them is scalar control flow. Children are
// taken in ascending order of their bound (ties: lowest lane), so the first leaf reached is
// the nearest one and most of the others fall to the bound.
#include "common.h"
#include "closest_tri.h"
#include "slot_search.h"
#include "wave.h"

namespace epos {
namespace {

constexpr int MP_LEVELS = 4;           // box levels of EposMeshRec
constexpr int MP_BLOCKS = 4096;        // workgroups of 4 waves; the waves stride over the rows

// Squared distance from p to box `lane` of a group (6 x 64 doubles: lo xyz, hi xyz), with the
// operations of the d2 of a face -- differences, squares, (x + y) + z -- so that rounding is
// monotone between the two: a computed closest point inside the box cannot give a smaller d2.
__device__ __forceinline__ double box_bound(const double* __restrict__ g, int lane,
                                            const double* p) {
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double below = g[k * 64 + lane] - p[k], above = p[k] - g[(3 + k) * 64 + lane];
    const double d = below > above ? below : above;
    e[k] = d > 0.0 ? d : 0.0;
  }
  return e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
}

#define MP_SEL(l, x) ((l) == 0 ? x##0 : (l) == 1 ? x##1 : (l) == 2 ? x##2 : x##3)
#define MP_SET(l, x, v)                                                         \
  do {                                                                          \
    if ((l) == 0) x##0 = (v); else if ((l) == 1) x##1 = (v);                    \
    else if ((l) == 2) x##2 = (v); else x##3 = (v);                             \
  } while (0)

__global__ __launch_bounds__(256) void project_rows_kernel(
    double* coord_3d, const int64_t* __restrict__ slot_base,
    const EposCorrSlot* __restrict__ slots, int S, int64_t cap,
    const EposMeshRec* __restrict__ recs, int num_objs, const double* __restrict__ geom,
    const int32_t* __restrict__ fids, int32_t* face_idx, int32_t* visited) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(
      static_cast<int>(blockIdx.x) * 4 + static_cast<int>(threadIdx.x >> 6));
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * 4;
  const int64_t end = clamp_row(slot_base[S], cap);
  for (int64_t r = clamp_row(slot_base[0], cap) + wave; r < end; r += nwaves) {
    const int s = find_slot(slot_base, S, cap, r);
    const int obj = slots[s].obj_id;
    if (obj < 1 || obj > num_objs) continue;
    const EposMeshRec& m = recs[obj - 1];
    const int nf = m.nf, nleaf = m.nleaf, top = m.top;
    if (nf <= 0 || top < 0 || top >= MP_LEVELS) continue;
    const double p[3] = {coord_3d[3 * r], coord_3d[3 * r + 1], coord_3d[3 * r + 2]};
    // far-field queries take every leaf (the error argument of the bound needs the query
    // within a known distance of the mesh); NaN coordinates compare false and land here too
    const bool near_mesh = p[0] >= m.near_lo[0] && p[0] <= m.near_hi[0] &&
                           p[1] >= m.near_lo[1] && p[1] <= m.near_hi[1] &&
                           p[2] >= m.near_lo[2] && p[2] <= m.near_hi[2];
    const double* __restrict__ tri = geom + m.tri_off;
    const int32_t* __restrict__ fid = fids + m.fid_off;

    double mine = INFINITY, bq[3] = {0.0, 0.0, 0.0};    // this lane's best face
    int32_t bf = nf;
    double best = INFINITY;                             // wave-uniform: min of `mine`
    int nvis = 0;

    auto sweep_block = [&](int blk) {
      const int32_t f = fid[static_cast<int64_t>(blk) * 64 + lane];
      if (f >= 0) {
        const double* t = tri + static_cast<int64_t>(blk) * 576 + lane;
        const double a[3] = {t[0], t[64], t[128]};
        const double b[3] = {t[192], t[256], t[320]};
        const double c[3] = {t[384], t[448], t[512]};
        double q[3];
        closest_on_triangle(p, a, b, c, q);
        const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        // (d2, f) lexicographic: faces are not met in index order here. inf never wins.
        if (d2 < mine || (d2 == mine && d2 < INFINITY && f < bf)) {
          mine = d2; bf = f; bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2];
        }
      }
      best = wave_min(mine);
      ++nvis;
    };

    for (int i = 0; i < m.nalways; ++i) sweep_block(nleaf + i);

    if (nleaf > 0) {
      double bnd0 = 0.0, bnd1 = 0.0, bnd2 = 0.0, bnd3 = 0.0;
      uint64_t pend0 = 0, pend1 = 0, pend2 = 0, pend3 = 0;
      int grp0 = 0, grp1 = 0, grp2 = 0, grp3 = 0;
      int lvl = top;
      bool load = true;
      for (;;) {
        if (load) {
          const int g = MP_SEL(lvl, grp);
          const int cnt = m.count[lvl] - g * 64;        // children of this group (<= 64 used)
          double b = 0.0;
          if (lane < cnt && near_mesh)
            b = box_bound(geom + m.box_off[lvl] + static_cast<int64_t>(g) * 384, lane, p);
          const uint64_t pd = __ballot(lane < cnt && !(b > best));
          MP_SET(lvl, bnd, b);
          MP_SET(lvl, pend, pd);
        }
        uint64_t pd = MP_SEL(lvl, pend);
        int j = -1;
        if (pd) {
          const double b = MP_SEL(lvl, bnd);
          const bool todo = (pd >> lane) & 1;
          const double mb = wave_min(todo ? b : INFINITY);
          // ascending bounds: once the smallest exceeds the best, so do the others
          if (!(mb > best)) j = __ffsll(static_cast<long long>(__ballot(todo && b == mb))) - 1;
        }
        if (j < 0) {                                    // node done
          if (lvl == top) break;
          ++lvl;
          load = false;
          continue;
        }
        pd &= ~(1ull << j);
        MP_SET(lvl, pend, pd);
        const int child = MP_SEL(lvl, grp) * 64 + j;
        if (lvl == 0) {
          sweep_block(child);
          load = false;
        } else {
          --lvl;
          MP_SET(lvl, grp, child);
          load = true;
        }
      }
    }

    int64_t wf = bf;                                    // the sweep's final reduction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_xor(mine, off, 64);
      const int64_t of = __shfl_xor(wf, off, 64);
      const double o0 = __shfl_xor(bq[0], off, 64), o1 = __shfl_xor(bq[1], off, 64),
                   o2 = __shfl_xor(bq[2], off, 64);
      if (ob < mine || (ob == mine && of < wf)) {
        mine = ob; wf = of; bq[0] = o0; bq[1] = o1; bq[2] = o2;
      }
    }
    if (lane == 0) {
      coord_3d[3 * r] = bq[0]; coord_3d[3 * r + 1] = bq[1]; coord_3d[3 * r + 2] = bq[2];
      if (face_idx) face_idx[r] = static_cast<int32_t>(wf);
      if (visited) visited[r] = nvis;
    }
  }
}

#undef MP_SEL
#undef MP_SET

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_project_rows_to_mesh_f64(double* coord_3d, const int64_t* slot_base,
                                             const EposCorrSlot* slots, int S,
                                             int64_t capacity, const EposMeshRec* recs,
                                             int num_objs, const double* geom,
                                             const int32_t* face_ids, int32_t* face_idx,
                                             int32_t* visited, void* stream) {
  EPOS_REQUIRE(S >= 0 && capacity >= 0, "S and capacity must be >= 0");
  if (S == 0 || capacity == 0) return EPOS_OK;
  EPOS_REQUIRE(coord_3d && slot_base && slots && recs && geom && face_ids, "null pointer");
  EPOS_REQUIRE(num_objs > 0, "empty mesh table");
  const int64_t blocks = ceil_div(capacity, 4);
  hipLaunchKernelGGL(project_rows_kernel,
                     dim3(static_cast<unsigned>(blocks < MP_BLOCKS ? blocks : MP_BLOCKS)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), coord_3d, slot_base,
                     slots, S, capacity, recs, num_objs, geom, face_ids, face_idx, visited);
  return launch_status("project_rows_kernel");
}
