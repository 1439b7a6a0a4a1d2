// ac_hbm_plan.hpp -- the launch plan of the HBM-resident AC kernels k_ac_lu_hbm<W> / k_ac_adj_hbm<W> (ac_lu.hip), as host-only arithmetic
// (the manner of lds_layout.hpp and lu_transpose.hpp): no HIP, no handle.  tests/test_ac_hbm_plan_cpu.py compiles it with the host compiler.
//
// The kernels keep what k_ac_lu keeps in LDS -- the complex factors and three complex n-vectors, 16 (nnz_lu + 3 n) bytes per system
// (lds_layout.hpp: lds_ac, the same regions in the same order) -- in a workspace in global memory.  A workspace belongs to a WAVE, not to a
// system: the grid is sized by the device, wave g of n_waves handles systems g, g + n_waves, ... of the launch and reuses its one
// workspace, so the handle's footprint is bounded however many systems a launch has.
//   n_waves = min(n_sys, CUs x k),  k the largest of 8, 4, 2, 1 with n_waves x per-system bytes <= AC_WORK_BYTES
// (k waves per compute unit: 8 is two per SIMD).  When not even one wave per compute unit fits, n_waves is what does fit.  A system whose
// own workspace exceeds AC_WORK_BYTES is refused.  A non-zero wave cap of the caller replaces CUs x k and is taken as given: the caller
// asked for that many workspaces.  wpb -- waves per workgroup -- is 1, 2, 4 or 8; 0 gives the plan's choice of 4 (a workgroup per SIMD
// quartet; the waves never meet at a workgroup barrier, so wpb only shapes the grid).
#pragma once
#include <stddef.h>

// A design cap on the handle's footprint, like AC_CHUNK_BYTES (api.hip): NOT a tuned value.  Nothing was measured to choose it
#define AC_WORK_BYTES ((size_t)256 << 20)
#define AC_HBM_WPB 4       // the plan's choice of waves per workgroup

namespace cadnip {

struct AcHbmPlan { int wpb = 0, n_waves = 0; size_t work_bytes = 0; };   // wpb 0: refused, nothing may be launched

// bytes of one system's (= one wave's) workspace
inline size_t ac_hbm_system_bytes(int nnz_lu, int n) { return 16 * ((size_t)nnz_lu + 3 * (size_t)n); }

// ... of k_ac_sens_hbm: a fourth complex n-vector (lds_layout.hpp: lds_ac_sens)
inline size_t ac_sens_hbm_system_bytes(int nnz_lu, int n) { return 16 * ((size_t)nnz_lu + 4 * (size_t)n); }

// the plan for workspaces of `per` bytes each
inline AcHbmPlan ac_hbm_plan_bytes(size_t per, long n_sys, int wpb_req, int max_waves, int n_cu) {
  AcHbmPlan none, p;
  if (per == 0 || n_sys <= 0 || max_waves < 0 || n_cu <= 0) return none;
  if (wpb_req != 0 && wpb_req != 1 && wpb_req != 2 && wpb_req != 4 && wpb_req != 8) return none;
  if (per > AC_WORK_BYTES) return none;
  size_t waves;
  if (max_waves > 0) waves = (size_t)max_waves;
  else {
    int k = 8;
    while (k > 1 && (size_t)n_cu * k * per > AC_WORK_BYTES && (size_t)n_sys * per > AC_WORK_BYTES) k >>= 1;
    waves = (size_t)n_cu * k;
    if (waves * per > AC_WORK_BYTES) waves = AC_WORK_BYTES / per;        // >= 1: per <= AC_WORK_BYTES
  }
  if ((size_t)n_sys < waves) waves = (size_t)n_sys;
  p.wpb = wpb_req ? wpb_req : AC_HBM_WPB;
  p.n_waves = (int)waves;
  p.work_bytes = waves * per;
  return p;
}

inline AcHbmPlan ac_hbm_plan(int nnz_lu, int n, long n_sys, int wpb_req, int max_waves, int n_cu) {
  if (nnz_lu <= 0 || n <= 0) return AcHbmPlan();
  return ac_hbm_plan_bytes(ac_hbm_system_bytes(nnz_lu, n), n_sys, wpb_req, max_waves, n_cu);
}

}  // namespace cadnip
