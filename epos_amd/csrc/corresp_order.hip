// Confidence order, truncation and row-order permutation of the pooled correspondences, on
// the device (the stage between epos_corr_fill and the fitting kernels when use_prosac or
// max_correspondences is set; scripts/infer.py:425-440 does this per object with np.argsort).
//
// Everything is a segmented sort of UNIQUE 64-bit keys, run twice on the same machinery:
//   1. key = (conf, descending) << 32 | slot-local row   -> the confidence order
//      (identity slots get key = row: already sorted, the passes move nothing);
//   2. key = y group << 32 | position in the kept list -> yorder (and ypos, its inverse):
//      the stable sort by coord_2d y of epos_find6d_poses. The y group of a row is the first
//      row of its slot with the same y (one binary search: a slot's rows come in raster
//      order, so y is non-decreasing along them). px_id cannot serve: epos_corr_fill writes
//      the index among the MASKED pixels there, which says nothing about the image row.
// Unique keys make the permutation a function of the keys alone: no stability argument, and
// any correct sort gives the same bits.
//
// The host never learns a row count, so every launch is sized from `capacity` and finds its
// work on the device: a workgroup sorts one tile of ORDER_TILE keys of one slot in LDS
// (bitonic network over the next power of two of the tile's fill), then log2(capacity /
// ORDER_TILE) merge passes double the run length, one thread per key: with unique keys a
// key's place in the merged pair is its index in its own run plus its rank in the sibling
// run (one binary search). The first launch leaves the longest slot and the longest kept
// list in the workspace; a pass whose runs already span them has nothing to merge and leaves
// at once (so slots of at most ORDER_TILE rows cost the tile sort alone), and every kernel
// works out from those two numbers which of the two key buffers holds the current keys.
// Workgroups beyond the rows that exist leave after one load.
//
// Slot bounds are clamped to [0, capacity]: after an overflow of epos_corr_fill (the
// pipeline raises at collect()) nothing at or beyond `capacity` is read and nothing beyond
// the kept rows is written.
#include "common.h"
#include "slot_search.h"

namespace epos {
namespace {

constexpr int ORDER_TILE = 4096;       // keys per workgroup of the LDS sort (32 KB)
constexpr int ORDER_T = 512;           // its threads
constexpr int ORDER_B = 256;           // threads of the per-row kernels

// float -> uint32 whose unsigned order is the float's DESCENDING order
__device__ __forceinline__ uint32_t desc_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// Merge passes that have work for segments of at most `longest` keys.
__device__ __forceinline__ int passes_for(int64_t longest) {
  int c = 0;
  for (int64_t run = ORDER_TILE; run < longest; run *= 2) ++c;
  return c;
}

// The two key buffers and info = {longest slot, longest kept list}. Sort 0 (confidence) starts
// in a; sort 1 (rows) starts in the buffer sort 0 did NOT end in.
struct KeyBufs {
  uint64_t* a;
  uint64_t* b;
  const int64_t* info;
  __device__ uint64_t* start(int sort) const {
    return sort == 0 || (passes_for(info[0]) & 1) ? a : b;
  }
  __device__ uint64_t* other(const uint64_t* p) const { return p == a ? b : a; }
  // where the keys of `sort` are after `done` of its passes
  __device__ uint64_t* at(int sort, int done) const {
    uint64_t* p = start(sort);
    return (done & 1) ? other(p) : p;
  }
  __device__ uint64_t* result(int sort) const { return at(sort, passes_for(info[sort])); }
};

__device__ __forceinline__ int64_t kept_rows(int64_t n, int64_t max_corr) {
  return max_corr > 0 && n > max_corr ? max_corr : n;
}

// Launch 1: the confidence keys of every row; the first thread also writes slot_base_out and
// info = {longest slot, longest kept list}.
__global__ __launch_bounds__(ORDER_B) void order_conf_keys(
    const float* __restrict__ conf, const int64_t* __restrict__ slot_base, int S, int64_t cap,
    int64_t max_corr, int always_sort, uint64_t* __restrict__ keys,
    int64_t* __restrict__ slot_base_out, int64_t* __restrict__ info) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * ORDER_B + threadIdx.x;
  if (g == 0) {
    int64_t acc = 0, longest = 0;
    for (int s = 0; s < S; ++s) {
      slot_base_out[s] = acc;
      const int64_t lo = clamp_row(slot_base[s], cap), hi = clamp_row(slot_base[s + 1], cap);
      const int64_t n = hi > lo ? hi - lo : 0;
      if (n > longest) longest = n;
      acc += kept_rows(n, max_corr);
    }
    slot_base_out[S] = acc;
    info[0] = longest;
    info[1] = kept_rows(longest, max_corr);
  }
  if (g < clamp_row(slot_base[0], cap) || g >= clamp_row(slot_base[S], cap)) return;
  const int s = find_slot(slot_base, S, cap, g);
  const int64_t lo = clamp_row(slot_base[s], cap), hi = clamp_row(slot_base[s + 1], cap);
  const int64_t n = hi - lo;
  const uint64_t row = static_cast<uint64_t>(g - lo);
  const bool apply = always_sort || (max_corr > 0 && n > max_corr);
  keys[g] = apply ? (static_cast<uint64_t>(desc_bits(conf[g])) << 32) | row : row;
}

// Sorts every tile of ORDER_TILE keys of every segment in place. Workgroup b owns the b-th
// tile in (segment, tile) order; there are at most capacity / ORDER_TILE + S of them.
__global__ __launch_bounds__(ORDER_T) void order_tile_sort(const int64_t* __restrict__ seg, int S,
                                                           int64_t cap, KeyBufs kb, int sort) {
  __shared__ uint64_t sk[ORDER_TILE];
  int64_t b = blockIdx.x;
  int64_t first = 0;
  int count = 0;
  for (int s = 0; s < S; ++s) {
    const int64_t lo = clamp_row(seg[s], cap), hi = clamp_row(seg[s + 1], cap);
    const int64_t n = hi > lo ? hi - lo : 0;
    const int64_t tiles = (n + ORDER_TILE - 1) / ORDER_TILE;
    if (b < tiles) {
      first = lo + b * ORDER_TILE;
      const int64_t left = hi - first;
      count = left < ORDER_TILE ? static_cast<int>(left) : ORDER_TILE;
      break;
    }
    b -= tiles;
  }
  if (count < 2) return;               // no such tile, or nothing to order
  uint64_t* keys = kb.start(sort);
  int m = 2;
  while (m < count) m <<= 1;           // <= ORDER_TILE
  for (int i = threadIdx.x; i < m; i += ORDER_T)
    sk[i] = i < count ? keys[first + i] : ~0ull;     // pads sort behind every key
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (m >> 1); t += ORDER_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint64_t a = sk[i], c = sk[i + j];
        const bool up = (i & k) == 0;
        if ((a > c) == up) { sk[i] = c; sk[i + j] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < count; i += ORDER_T) keys[first + i] = sk[i];
}

// Merge pass number `pass` of a sort: runs of `run` keys (sorted, per segment) become runs
// of 2 * run. Nothing to do (and nothing moved) once the runs span the longest segment.
__global__ __launch_bounds__(ORDER_B) void order_merge_pass(const int64_t* __restrict__ seg, int S,
                                                            int64_t cap, int64_t run, int pass,
                                                            KeyBufs kb, int sort) {
  if (run >= kb.info[sort]) return;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * ORDER_B + threadIdx.x;
  if (g < clamp_row(seg[0], cap) || g >= clamp_row(seg[S], cap)) return;
  const uint64_t* __restrict__ in = kb.at(sort, pass);
  uint64_t* __restrict__ out = kb.at(sort, pass + 1);
  const int s = find_slot(seg, S, cap, g);
  const int64_t lo = clamp_row(seg[s], cap), n = clamp_row(seg[s + 1], cap) - lo;
  const int64_t i = g - lo;
  const uint64_t key = in[g];
  const int64_t r = i / run;
  const int64_t own = r * run;                       // first index of the key's run
  const int64_t sib = (r ^ 1) * run;                 // ... of the sibling run
  if (sib >= n) { out[g] = key; return; }            // last run of an odd count: as it is
  const int64_t sib_end = sib + run < n ? sib + run : n;
  const uint64_t* q = in + lo;
  int64_t a = sib, e = sib_end;                      // keys of the sibling run below `key`
  while (a < e) {
    const int64_t mid = (a + e) >> 1;
    if (q[mid] < key) a = mid + 1; else e = mid;
  }
  const int64_t pair = own < sib ? own : sib;
  out[lo + pair + (i - own) + (a - sib)] = key;
}

// The kept rows in confidence order: src_row, the gathered coordinates, and the row-order
// keys of the second sort.
__global__ __launch_bounds__(ORDER_B) void order_gather(
    KeyBufs kb, const double* __restrict__ coord_2d, const double* __restrict__ coord_3d,
    const int64_t* __restrict__ slot_base, const int64_t* __restrict__ slot_base_out, int S,
    int64_t cap, double* __restrict__ coord_2d_out, double* __restrict__ coord_3d_out,
    int32_t* __restrict__ src_row_out) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * ORDER_B + threadIdx.x;
  if (g >= clamp_row(slot_base_out[S], cap)) return;
  const uint64_t* __restrict__ sorted = kb.result(0);
  uint64_t* __restrict__ keys_out = kb.start(1);
  const int s = find_slot(slot_base_out, S, cap, g);
  const int64_t j = g - slot_base_out[s];
  const int64_t lo = clamp_row(slot_base[s], cap), n = clamp_row(slot_base[s + 1], cap) - lo;
  const int64_t r = static_cast<int64_t>(sorted[lo + j] & 0xffffffffull);
  const int64_t src = lo + r;
  const double y = coord_2d[2 * src + 1];
  src_row_out[g] = static_cast<int32_t>(r);
  coord_2d_out[2 * g] = coord_2d[2 * src];
  coord_2d_out[2 * g + 1] = y;
  coord_3d_out[3 * g] = coord_3d[3 * src];
  coord_3d_out[3 * g + 1] = coord_3d[3 * src + 1];
  coord_3d_out[3 * g + 2] = coord_3d[3 * src + 2];
  // y group: the first row of the slot whose y is not below this row's
  const double* ys = coord_2d + 2 * lo + 1;
  int64_t a = 0, e = n;
  while (a < e) {
    const int64_t mid = (a + e) >> 1;
    if (ys[2 * mid] < y) a = mid + 1; else e = mid;
  }
  keys_out[g] = (static_cast<uint64_t>(a) << 32) | static_cast<uint64_t>(j);
}

__global__ __launch_bounds__(ORDER_B) void order_perm(KeyBufs kb,
                                                      const int64_t* __restrict__ slot_base_out,
                                                      int S, int64_t cap,
                                                      int32_t* __restrict__ yorder,
                                                      int32_t* __restrict__ ypos) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * ORDER_B + threadIdx.x;
  if (g >= clamp_row(slot_base_out[S], cap)) return;
  const uint64_t* __restrict__ sorted = kb.result(1);
  const int s = find_slot(slot_base_out, S, cap, g);
  const int64_t base = slot_base_out[s];
  const int64_t o = static_cast<int64_t>(sorted[g] & 0xffffffffull);
  yorder[g] = static_cast<int32_t>(o);
  ypos[base + o] = static_cast<int32_t>(g - base);
}

// Tile sort + merge passes of sort 0 / 1 over segments of at most `longest` keys (the bound
// the host knows; the passes beyond the longest segment there is leave at once).
int sort_segments(const int64_t* seg, int S, int64_t cap, int64_t longest, const KeyBufs& kb,
                  int sort, hipStream_t st) {
  const unsigned tiles = static_cast<unsigned>(ceil_div(cap, ORDER_TILE) + S);
  const unsigned rows = static_cast<unsigned>(ceil_div(cap, ORDER_B));
  hipLaunchKernelGGL(order_tile_sort, dim3(tiles), dim3(ORDER_T), 0, st, seg, S, cap, kb, sort);
  int rc = launch_status("order_tile_sort");
  int pass = 0;
  for (int64_t run = ORDER_TILE; !rc && run < longest; run *= 2, ++pass) {
    hipLaunchKernelGGL(order_merge_pass, dim3(rows), dim3(ORDER_B), 0, st, seg, S, cap, run, pass,
                       kb, sort);
    rc = launch_status("order_merge_pass");
  }
  return rc;
}

}  // namespace
}  // namespace epos

using namespace epos;

extern "C" int epos_corr_order_tile_rows(void) { return ORDER_TILE; }

extern "C" int64_t epos_corr_order_workspace_bytes(int S, int64_t capacity) {
  if (S < 0 || capacity < 0) return EPOS_E_INVALID;
  return 2 * round_up(capacity * 8, 256) + 512;      // two key buffers, info, alignment
}

extern "C" int epos_corr_order_by_conf(
    const float* conf, const int64_t* px_id, const double* coord_2d, const double* coord_3d,
    const int64_t* slot_base, int S, int64_t capacity, int W, int64_t max_corr, int always_sort,
    void* work, int64_t* slot_base_out, double* coord_2d_out, double* coord_3d_out,
    int32_t* src_row_out, int32_t* yorder, int32_t* ypos, void* stream) {
  EPOS_REQUIRE(S >= 0 && capacity >= 0, "S and capacity must be >= 0");
  EPOS_REQUIRE(capacity < (int64_t{1} << 31), "slot-local rows are int32: capacity < 2^31");
  EPOS_REQUIRE(slot_base && slot_base_out, "null slot_base / slot_base_out");
  EPOS_REQUIRE(capacity == 0 || (conf && px_id && coord_2d && coord_3d && work && coord_2d_out &&
                                 coord_3d_out && src_row_out && yorder && ypos),
               "null pointer");
  EPOS_REQUIRE(capacity == 0 || W >= 1, "W must be >= 1");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (S == 0 || capacity == 0)         // nothing is kept: every bound is 0
    return check_hip(hipMemsetAsync(slot_base_out, 0, sizeof(int64_t) * (S + 1), st),
                     "clear slot_base_out");
  char* wp = static_cast<char*>(work);
  wp += (256 - reinterpret_cast<uintptr_t>(wp) % 256) % 256;
  const int64_t kbytes = round_up(capacity * 8, 256);
  int64_t* info = reinterpret_cast<int64_t*>(wp + 2 * kbytes);
  const KeyBufs kb = {reinterpret_cast<uint64_t*>(wp), reinterpret_cast<uint64_t*>(wp + kbytes),
                      info};
  const unsigned rows = static_cast<unsigned>(ceil_div(capacity, ORDER_B));
  hipLaunchKernelGGL(order_conf_keys, dim3(rows), dim3(ORDER_B), 0, st, conf, slot_base, S,
                     capacity, max_corr, always_sort, kb.a, slot_base_out, info);
  int rc = launch_status("order_conf_keys");
  if (rc) return rc;
  rc = sort_segments(slot_base, S, capacity, capacity, kb, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(order_gather, dim3(rows), dim3(ORDER_B), 0, st, kb, coord_2d, coord_3d,
                     slot_base, slot_base_out, S, capacity, coord_2d_out, coord_3d_out,
                     src_row_out);
  rc = launch_status("order_gather");
  if (rc) return rc;
  // a kept list is at most max_corr rows long: its sort needs no pass beyond that
  const int64_t longest = max_corr > 0 && max_corr < capacity ? max_corr : capacity;
  rc = sort_segments(slot_base_out, S, capacity, longest, kb, 1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(order_perm, dim3(rows), dim3(ORDER_B), 0, st, kb, slot_base_out, S,
                     capacity, yorder, ypos);
  return launch_status("order_perm");
}
