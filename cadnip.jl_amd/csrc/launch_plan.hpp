// launch_plan.hpp -- THE launch plan of the LDS-resident kernels: what a fused launch runs (f2_choose) and what launch_factor_solve runs
// (lu_choose), as pure functions of facts about the handle (PlanFacts) and of the diagnostic switches as values (F2Switches, LuSwitches).
// Host-only: plain C++, no HIP, no handle type, no getenv (tests/test_launch_plan_cpu.py compiles it with the host compiler and walks the
// truth tables).  fused2.hip: fused2_plan and lu_f2.hip: lu_f2_plan gather the facts -- building tables and block descriptors on the way --,
// read the switches from the environment and call these; lds_layout.hpp is the map of the LDS block whose bytes the rules count.
#pragma once
#include "lds_layout.hpp"
#include "src_cache.hpp"

namespace cadnip {

enum F2Mode { F2_TRAN, F2_DC, F2_STEP };
enum F2Steps { F2_STEPS_NONE, F2_STEPS_1, F2_STEPS_TEAM2, F2_STEPS_TEAM4 };   // the step list a fused launch stages (FusedState: steps1, team[0], team[1])

struct StepFacts { int present = 0, len = 0, n_steps[3] = {0, 0, 0}; };   // one StepList: uploaded or not, 64-bit words, steps pre-core / post-core / forward-only
struct BlockFacts { int type = -1, mos1_plain = 0; };
// Everything the two planners read from a handle, as plain numbers (flags: 0 / 1)
struct PlanFacts {
  int B = 0, n = 0;
  int n_cu = 0;               // compute units of the device: asked once per handle, at its first plan of either kind
  int nb = 0;                 // non-empty device blocks of the circuit
  int va_ext = 0, analyzed = 0;
  int tables = 0;             // the packed tables exist (fused2_tables; what follows is meaningful only then)
  int delayed = 0;            // delayed stamps are set (cadnip_tran_set_delay)
  int homotopy = 0;           // a homotopy is in force: h->homotopy, gshunt != 0 or srcFact < 1
  // FusedState: the linear-solve program and the table ranges (32-bit words)
  int lu_words = 0, nc = 0, n_pre = 0, n_post = 0, lu_len = 0, lean_lo = 0, lean_end = 0, full_len = 0, loadpos_off = 0;
  // ... and the block list (fused2_blocks; filled when the circuit passed f2_circuit_fits): blk [n_blk], the facts f2_shape_ok takes
  int par_words = 0, n_blk = 0;
  int src_blk = -1, src_type = -1, src_count = 0, rc_type = -1, rc_count = 0, dev_type = -1, dev_plain = 0, dev_count = 0;
  BlockFacts blk[F2_MAX_BLOCKS];   // (in the handle's order, not the descriptors': the lean rule does not care)
  StepFacts steps1, steps4, team[2];
  int lu_plain_threads = 0;   // lu_choose only: threads of k_lu (kernels.hip: lu_plain_threads)
};

// The diagnostic switches, each SW_UNSET or the number the variable holds (atoi)
#define SW_UNSET (-2147483647 - 1)
struct F2Switches {           // CADNIP_F2_...
  int nodirect = SW_UNSET;    // set (to anything): the assembled residual, variant 2
  int team = SW_UNSET;        // 0 | 2 | 4: forces the team width
  int wpb = SW_UNSET;         // caps the sweep kernel's waves per workgroup
  int steps_packed = SW_UNSET;   // set (to anything): the kernel decodes the packed step words
  int src_cache = SW_UNSET, fixed = SW_UNSET, shape = SW_UNSET;   // 0: without the source cache / the fixed form / the shape form
};
struct LuSwitches {           // CADNIP_LU_..., read for kernel CADNIP_LUK_AUTO only
  int plain = SW_UNSET;       // set (to anything): k_lu
  int steps = SW_UNSET;       // 0 | 1: forces the choice of k_lu_steps
  int wpi = SW_UNSET;         // 4: k_lu_f2_mw, another number: not
  int f2s = SW_UNSET;         // 0: keeps the pass program
};
inline bool sw_is_zero(int s) { return s == 0; }   // (SW_UNSET is not 0)

// ---- the fused kernels -----------------------------------------------------------------------------------------------------------
// The lean device set: linear elements, sources, plain sp_mos1 ...
inline bool f2_type_lean(int type, int mos1_plain) {
  const bool heavy = type == CADNIP_DEV_DIODE || type == CADNIP_DEV_DIODECAP || type == CADNIP_DEV_SIMPLEMOS || type == CADNIP_DEV_BVSOURCE ||
                     type == CADNIP_DEV_BISOURCE || type == CADNIP_DEV_VA || (type == CADNIP_DEV_MOS1 && !mos1_plain);
  return !heavy;
}
// ... and its linear solve runs from step descriptors staged in LDS: a circuit whose steps do not fit beside the tables and eight
// instances (long dependency chains: an RC ladder has one step per section) takes the full variant, whose pass program is compact
inline bool f2_lean(const PlanFacts& f) {
  for (int i = 0; i < f.n_blk; ++i)
    if (!f2_type_lean(f.blk[i].type, f.blk[i].mos1_plain)) return false;
  return f.steps1.present && lds_bytes(lds_sweep((size_t)0, f.lean_end - f.lean_lo, f.steps1.len, f.lu_words, f.n, 0, 8)) <= LDS_BUDGET;
}
// The circuit can be addressed by the fused kernels at all: at most F2_MAX_BLOCKS blocks, and one instance beside the FULL table has to fit,
// whichever range the chosen kernel stages (findings).  The block descriptors are built for such a circuit only
inline bool f2_circuit_fits(const PlanFacts& f) {
  return f.nb <= F2_MAX_BLOCKS && lds_bytes(lds_sweep((size_t)0, f.full_len, 0, f.lu_words, f.n, 0, 1)) <= LDS_BUDGET;
}

struct F2CallOpts { int newton_mode, max_order, step_rule, use_pcnr; };   // of the transient call the plan is for: what f2_fixed_ok reads
// What a fused launch would run.  rc != CADNIP_OK: the fused kernels do not apply now; !circuit_ok: they never apply to this circuit / Newton mode
struct F2Choice {
  int rc = CADNIP_OK; bool circuit_ok = false;
  int nw = 0;                 // team kernel k_fteam<nw>; 0: sweep kernel k_fused2<wpb, dc, var>
  int var = 0, wpb = 0, grid = 0; size_t shmem = 0;
  int tab_lo = 0, tab_len = 0;          // staged table range (32-bit words)
  F2Steps step_list = F2_STEPS_NONE;    // step descriptors staged behind it (none: the pass program of the full table)
  bool step_predec = false, keep_factors = false;
  int src_words = 0;
  bool fixed = false, shape = false;
};

// The one place that decides what a fused launch runs.  topt: null = no transient call (the fixed form is then never chosen)
inline F2Choice f2_choose(const PlanFacts& f, const F2Switches& sw, F2Mode mode, int newton_mode, const F2CallOpts* topt) {
  F2Choice p;
  p.rc = CADNIP_BADARG;
  // external generated models exist in the per-op stamping kernel only; an un-analyzed handle is the entry points' CADNIP_NOTREADY
  if (f.va_ext || !f.analyzed) return p;
  if (!f.tables) return p;                              // (the tables cannot address the circuit)
  if (!f2_circuit_fits(f)) return p;
  // every device type emits its residual directly (devices.hpp, Rn); CADNIP_F2_NODIRECT=1 selects the assembled form
  // r = J u + C beta - b instead (diagnostic: the two must agree)
  const bool direct = sw.nodirect == SW_UNSET, circuit_lean = f2_lean(f), lean = direct && circuit_lean;
  // IDA-style Jacobian reuse (Newton mode 1) and the single step exist in the lean direct-residual variant only: a circuit with other
  // device types (diodes, behavioural sources, sp_mos1 with series resistances, built-in Verilog-A modules ...) takes the per-op kernels
  p.keep_factors = mode != F2_DC && (newton_mode || mode == F2_STEP);
  if (p.keep_factors && !lean) return p;
  // delayed stamps (cadnip_tran_set_delay) and their history ring exist beside the per-op kernels only (delay.hip); DC ignores them
  if (mode == F2_TRAN && f.delayed) return p;
  p.circuit_ok = true;
  if (f.homotopy) return p;                             // homotopies run on the per-op path
  p.var = !direct ? 2 : circuit_lean ? 0 : 1;
  p.tab_len = f.full_len;
  if (lean) { p.tab_lo = f.lean_lo; p.tab_len = f.lean_end - f.lean_lo; }   // the lean kernels stage [permutations | stamp and node tables] only
  // Few instances: a team of waves per instance (fused_team_kernel.hpp) -- the latency of ONE transient is what counts when the batch
  // cannot fill the chip.  Transient, direct residuals, lean device set.  CADNIP_F2_TEAM = 0 | 2 | 4 forces the choice (diagnostic, tests).
  if (mode != F2_DC && lean) {
    // at most one instance per CU: a team of four waves (one per SIMD); at most two: teams of two waves, two workgroups per CU (their LDS allows it);
    // beyond that the sweep kernel's one wave per instance
    int nw = f.B <= f.n_cu ? 4 : f.B <= 2 * f.n_cu ? 2 : 0;
    if (sw.team != SW_UNSET) nw = sw.team >= 4 ? 4 : sw.team >= 2 ? 2 : 0;
    if (mode == F2_STEP) nw = 4;
    const StepFacts& T = f.team[nw / 4];
    const size_t shmem = lds_bytes(lds_team((size_t)0, p.tab_len, nw ? T.len : 0, f.lu_words, f.n, f.par_words, nw));
    if (nw && T.present && shmem <= LDS_BUDGET) {
      size_t wg_per_cu = LDS_BUDGET / shmem;
      if (wg_per_cu > (size_t)(16 / nw)) wg_per_cu = (size_t)(16 / nw);
      if (wg_per_cu < 1) wg_per_cu = 1;
      const int resident = f.n_cu * (int)wg_per_cu;
      p.nw = nw; p.step_list = nw == 4 ? F2_STEPS_TEAM4 : F2_STEPS_TEAM2; p.shmem = shmem; p.grid = f.B < resident ? f.B : resident; p.rc = CADNIP_OK;
      return p;
    }
  }
  if (mode == F2_STEP) return p;                        // (no team kernel for this circuit: the caller takes the per-op kernels)
  // waves (= instances) per workgroup: 8 (two waves per SIMD) when they fit into LDS; fewer when the whole batch is then
  // still resident in one generation with a workgroup on every CU -- a wave runs about 20 % faster with half as many
  // neighbours on its CU (1024 instances: 4 per workgroup on 256 CUs, 57.7 M iterations/s, against 48.1 M as 8 x 128)
  if (lean) p.step_list = F2_STEPS_1;   // the lean variant's linear solve runs from step descriptors (f2_build_steps) staged behind the tables
  const int steps_len = p.step_list == F2_STEPS_1 ? f.steps1.len : 0;
  auto bytes = [&](int wpb) { return lds_bytes(lds_sweep((size_t)0, p.tab_len, steps_len, f.lu_words, f.n, 0, wpb)); };
  int wpb = 8;
  if (sw.wpb != SW_UNSET) wpb = sw.wpb >= 8 ? 8 : sw.wpb >= 4 ? 4 : sw.wpb >= 2 ? 2 : 1;   // diagnostic: cap the waves per workgroup
  while (wpb > 1 && (bytes(wpb) > LDS_BUDGET || f.n_cu * (wpb / 2) >= f.B)) wpb >>= 1;
  if (bytes(wpb) > LDS_BUDGET) return p;
  // resident workgroups only: the instances beyond them are handed out by the in-kernel queue as waves become free
  const int wg_per_cu = sweep_wg_per_cu(bytes(wpb), wpb);
  // The step descriptors are staged pre-decoded (lds_layout.hpp: lds_step_predecode) when every word of a work array has a 16-bit byte
  // offset and the flag bytes fit without costing a resident instance: neither wpb nor the workgroups per CU may change for them.  Otherwise,
  // and under CADNIP_F2_STEPS_PACKED=1 (diagnostic, tests: the two decodes must agree to the bit), the kernel decodes the packed words.
  size_t shmem = bytes(wpb);
  if (p.step_list != F2_STEPS_NONE && lds_steps_predec_ok(f.lu_words, f.n) && sw.steps_packed == SW_UNSET) {
    const size_t pd = lds_bytes(lds_sweep((size_t)0, p.tab_len, lds_sweep_desc_words(steps_len, true), f.lu_words, f.n, 0, wpb));
    if (pd <= LDS_BUDGET && sweep_wg_per_cu(pd, wpb) == wg_per_cu) { p.step_predec = true; shmem = pd; }
  }
  // Transient launches of the direct-residual variants keep the segment each pinned source is on in LDS (src_cache.hpp), under the same rule: the
  // region may cost neither a wave per workgroup (wpb stands as chosen above) nor a workgroup per CU.  Otherwise, and under CADNIP_F2_SRC_CACHE=0
  // (diagnostic, tests: bit-identical results either way), every new time point evaluates its sources from global memory as before.
  if (mode == F2_TRAN && direct && f.src_blk >= 0 && !sw_is_zero(sw.src_cache)) {
    const int cw = src_cache_words(f.src_count), dw = p.step_list != F2_STEPS_NONE ? lds_sweep_desc_words(steps_len, p.step_predec) : 0;
    if (src_cache_fits(p.tab_len, dw, f.lu_words, f.n, wpb, cw)) {
      p.src_words = cw;
      shmem = lds_bytes(lds_sweep((size_t)0, p.tab_len, dw, f.lu_words, f.n, 0, wpb, cw));
    }
  }
  // The default transient call on a lean circuit takes the fixed form of variant 0 (k_fused2<wpb, false, 3>: the call's switches are compile-time
  // constants there); f2_fixed_ok is the list of what that kernel assumes.  CADNIP_F2_FIXED=0 (diagnostic, tests: bit-identical results either
  // way) keeps the generic kernel, and so do CADNIP_F2_STEPS_PACKED=1 and CADNIP_F2_SRC_CACHE=0 through step_predec / src_words.
  p.fixed = topt && f2_fixed_ok(mode == F2_TRAN, p.var == 0, topt->newton_mode, p.step_predec, p.src_words, f.n, f.nc, topt->max_order, topt->step_rule,
                                topt->use_pcnr, !sw_is_zero(sw.fixed));
  // ... and of the fixed form its shape form (k_fused2<wpb, false, 4>) when the circuit's block list is a CMOS cell's: voltage sources, one pass of
  // plain sp_mos1, capacitors -- f2_shape_ok is the list.  CADNIP_F2_SHAPE=0 (diagnostic, tests: bit-identical results either way) keeps variant 3.
  // (its sp_mos1 lanes address u by 16-bit byte offsets from W: lds_m1pin_ok)
  p.shape = f2_shape_ok(p.fixed, f.n_blk, f.src_type, f.src_count, f.rc_type, f.rc_count, f.dev_type, f.dev_plain, f.dev_count, !sw_is_zero(sw.shape)) &&
            lds_m1pin_ok(f.lu_words, f.n);
  const int groups = (f.B + wpb - 1) / wpb, resident = f.n_cu * wg_per_cu;
  p.wpb = wpb; p.shmem = shmem; p.grid = groups < resident ? groups : resident; p.rc = CADNIP_OK;
  return p;
}

// ---- the per-op refactor + solve (lu_f2.hip: launch_factor_solve) -------------------------------------------------------------------
// kernel: CADNIP_LUK_*, -1: the forced kernel does not apply.  The first six members are what cadnip_factor_solve reports (info [6])
struct LuPlan { int kernel, wpb, wpi, nc, pre, post, tab_lo, tab_len; size_t shmem; };   // wpb, wpi: waves per workgroup / per instance; pre, post: steps or passes before / after the dense core
// k_lu without a look at the tables: forced, CADNIP_LU_PLAIN set (diagnostic: the kernels must agree), or a Jacobian that is not fused (J from d_J)
inline bool lu_takes_plain(const LuSwitches& sw, bool fuse, int kernel) {
  return !fuse || kernel == CADNIP_LUK_PLAIN || (kernel == CADNIP_LUK_AUTO && sw.plain != SW_UNSET);
}
// THE plan of launch_factor_solve: which kernel runs and with what geometry.  kernel: CADNIP_LUK_AUTO (the choice below, switches included) or
// one forced kernel (switches and batch rules ignored, the LDS limits kept; W of k_lu_f2s / k_lu_f2 still from B).  When no program kernel
// applies, auto runs k_lu
inline LuPlan lu_choose(const PlanFacts& f, const LuSwitches& sw, bool fuse, int kernel) {
  const bool any = kernel == CADNIP_LUK_AUTO;
  const LuPlan none{-1, 0, 0, 0, 0, 0, 0, 0, 0};
  const int plain_waves = f.lu_plain_threads / 64;
  const LuPlan plain{CADNIP_LUK_PLAIN, plain_waves, plain_waves, 0, 0, 0, 0, 0, 0};
  if (lu_takes_plain(sw, fuse, kernel)) return plain;
  const LuPlan other = any ? plain : none;
  if (!f.tables) return other;                          // (only the linear-solve prefix of the tables has to fit: the LDS limits below)
  auto bytes = [&](int tab_len, int desc_len, bool consts, int waves) { return lds_bytes(lds_lu((size_t)0, tab_len, desc_len, f.lu_words, f.n, consts, 0, waves)); };
  // at most two instances per CU: the straight-line steps of a team of four waves per instance (k_lu_steps).  CADNIP_LU_STEPS = 0 | 1 forces the choice
  if (any || kernel == CADNIP_LUK_STEPS4) {
    const bool steps = !any || (sw.steps != SW_UNSET ? sw.steps != 0 : f.B <= 2 * f.n_cu);
    if (steps && f.steps4.present && bytes(0, 0, true, 1) <= LDS_BUDGET) return LuPlan{CADNIP_LUK_STEPS4, 4, 4, f.nc, f.steps4.n_steps[0], f.steps4.n_steps[1], 0, 0, bytes(0, 0, true, 1)};
    if (!any) return none;
  }
  // a few instances of a circuit with many passes: several waves per instance (k_lu_f2_mw).  CADNIP_LU_WPI forces 1 / 4 (diagnostic)
  if (any || kernel == CADNIP_LUK_F2MW) {
    const int wpi = !any ? 4 : sw.wpi != SW_UNSET ? sw.wpi : (f.B * 4 <= f.n_cu && f.n_pre + f.n_post >= 32 ? 4 : 1);
    if (wpi == 4 && bytes(f.lu_len, 0, false, 1) <= LDS_BUDGET) return LuPlan{CADNIP_LUK_F2MW, 4, 4, f.nc, f.n_pre, f.n_post, 0, f.lu_len, bytes(f.lu_len, 0, false, 1)};
    if (!any) return none;
  }
  // many instances: one wave each, 8 per workgroup unless fewer still put a workgroup on every CU
  int wpb = 8;
  while (wpb > 1 && f.B < f.n_cu * wpb / 2) wpb >>= 1;
  // ... on the step program when its descriptors fit beside eight work arrays (CADNIP_LU_F2S = 0 keeps the passes); staged: the table from the load map on
  if (f.steps1.present && (any ? !sw_is_zero(sw.f2s) : kernel == CADNIP_LUK_F2S)) {
    const int lo = f.loadpos_off & ~3;
    if (bytes(f.lu_len - lo, f.steps1.len, true, 8) <= LDS_BUDGET)
      return LuPlan{CADNIP_LUK_F2S, wpb, 1, f.nc, f.steps1.n_steps[0], f.steps1.n_steps[1], lo, f.lu_len - lo, bytes(f.lu_len - lo, f.steps1.len, true, wpb)};
  }
  if (!any && kernel != CADNIP_LUK_F2) return none;
  while (wpb > 1 && bytes(f.lu_len, 0, false, wpb) > LDS_BUDGET) wpb >>= 1;
  if (bytes(f.lu_len, 0, false, wpb) > LDS_BUDGET) return other;
  return LuPlan{CADNIP_LUK_F2, wpb, 1, f.nc, f.n_pre, f.n_post, 0, f.lu_len, bytes(f.lu_len, 0, false, wpb)};
}

}  // namespace cadnip
