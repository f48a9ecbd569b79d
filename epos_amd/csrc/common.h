// Helpers shared by the translation units of libepos_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/epos_hip.h"

namespace epos {

void set_error(const char* fmt, ...);

inline int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return EPOS_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return EPOS_E_HIP_BASE - static_cast<int>(e);
}

inline int launch_status(const char* kernel) {
  return check_hip(hipGetLastError(), kernel);
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int64_t ceil_div(int64_t x, int64_t m) { return (x + m - 1) / m; }
// workgroups of `threads` for `total` work items
inline unsigned blocks_for(int64_t total, int threads) {
  return static_cast<unsigned>(ceil_div(total, threads));
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f),
                     fmaxf(v.w, 0.f));
}

// Issue priority of the depthwise kernels' waves: when such a wave shares a SIMD with a GEMM
// wave of another image in flight it gets the issue slots first -- it is short and mostly
// waits for memory, the GEMM wave loses nothing it could use. Same-box A/Bs of round 5
// (profiles/r05/ab_dw_setprio.txt, ab_wave_priorities.txt): priority 1-3 vs 0 = +0.6 % end to
// end; the same for the other helper kernels (softmax, resize, correspondences) and for the
// fitting kernels: no effect, not kept. Wave priority only: nothing about results changes.
constexpr int DW_PRIO = 3;
#define EPOS_SET_PRIO(p) do { if ((p) > 0) __builtin_amdgcn_s_setprio(p); } while (0)

#define EPOS_REQUIRE(cond, msg)                  \
  do {                                           \
    if (!(cond)) {                               \
      ::epos::set_error("%s: %s", __func__, msg); \
      return EPOS_E_INVALID;                     \
    }                                            \
  } while (0)

// EPOS_REQUIRE in the name of the entry `fn`: an entry and its _knn sibling share one body
#define EPOS_REQUIRE_FN(fn, cond, msg)           \
  do {                                           \
    if (!(cond)) {                               \
      ::epos::set_error("%s: %s", fn, msg);      \
      return EPOS_E_INVALID;                     \
    }                                            \
  } while (0)

}  // namespace epos
