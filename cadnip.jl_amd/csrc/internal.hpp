// internal.hpp -- handle layout shared by the kernel, symbolic and driver translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/cadnip_hip.h"
#include "stamp_plan.hpp"   // StampShape
#include "ac_hbm_plan.hpp"  // AcHbmPlan
#include "delay_plan.hpp"   // DelayPlan
#include "tran_sens_plan.hpp"
#include "launch_plan.hpp"  // PlanFacts, F2Mode, F2Choice
// rows of the derived sp_mos1 parameter card (devices.hpp: enum M1_*) that cadnip_set_params inspects
#define CADNIP_MOS1_PAR_OXCAP 8
#define CADNIP_MOS1_PAR_GD 30
#define CADNIP_MOS1_PAR_GS 31

#define HIP_TRY(expr)                                                     \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      cadnip::set_last_error(#expr, _e);                                  \
      return CADNIP_HIPERROR;                                             \
    }                                                                     \
  } while (0)

namespace cadnip {

void set_last_error(const char* what, hipError_t e);

// host-side result of the symbolic phase (symbolic.cpp)
struct LUProgram {
  int n = 0;
  int n_blocks = 0;                    // CADNIP_LU_ORDER=klu: diagonal blocks of the block triangular form (0: the Markowitz search was used)
  std::vector<int> rperm, cperm;       // pivot k uses original row rperm[k], column cperm[k]
  std::vector<char> unit;              // pivot k is the stamped constant 1 (a charge / limit row's own diagonal): no division by it
  int nnz_lu = 0;
  // LU stored row-major in permuted indices; row i occupies [lu_rowptr[i], lu_rowptr[i+1]) with sorted columns
  std::vector<int> lu_rowptr, lu_col, lu_diag;   // lu_diag[i] = position of U(i,i)
  std::vector<int> load_src, load_dst;           // J csr position -> LU position
  // entry-wise left-looking factorisation program, entries sorted by dependency level
  std::vector<int> ent_pos, ent_diag, ent_ptr;   // ent_diag = -1 for U entries, else position of the pivot
  std::vector<int> term_a, term_b;               // LU positions: acc -= lu[a]*lu[b]
  std::vector<int> lev_ptr;                      // factor levels -> ranges of entries
  // triangular solves, row-wise gather, rows sorted by level
  std::vector<int> fwd_rows, fwd_lev_ptr, bwd_rows, bwd_lev_ptr;
};

// device-local unknowns for the leaf-first pivot order (symbolic.cpp): charges [q_begin, lim_begin), limits [lim_begin, n);
// unit_ok[i]: the diagonal of unknown i is one constant stamp (no C part, a single G slot)
struct LULeaves { int q_begin = -1, lim_begin = -1; const unsigned char* unit_ok = nullptr; bool first = false; };   // first: pivot the leaves before everything else (diagnostic, CADNIP_LU_LEAF_FIRST=1)

static inline unsigned long long pack4(unsigned a, unsigned b, unsigned c, unsigned d) {
  return (unsigned long long)(a & 0xFFFFu) | ((unsigned long long)(b & 0xFFFFu) << 16) | ((unsigned long long)(c & 0xFFFFu) << 32) | ((unsigned long long)(d & 0xFFFFu) << 48);
}

// ---- linear-solve program of the fused kernel (f2_program.cpp) ----
struct F2Program {
  int nc = 0, lu_words = 0, dn0 = 0;       // core size, words before the rhs (sparse + dense), first dense word
  std::vector<int> posW;                   // LU pattern position -> W offset
  std::vector<unsigned long long> lanes, passes;          // lane descriptors, pass descriptors (pre-dense passes, then post-dense)
  std::vector<unsigned> terms;
  int n_pre = 0, n_post = 0, n_fwd = 0;    // (n_fwd: forward substitution alone, on kept factors: behind the other two lists)
  double cost = 0;                         // issue-slot estimate used to choose nc
};

struct F2Ent { int pos, dg, lvl; std::vector<int> a, b; std::vector<int> tl; int dl = -1; };   // tl / dl: level at which term t's factors / the pivot are final

bool f2_build_program(const LUProgram& P, int n, int nc, F2Program& G);

// the same program laid out for a team of nw waves per instance (f2_program.cpp: f2_build_team; fused_team_kernel.hpp)
struct F2Team {
  int nw = 0, nc = 0, lu_words = 0, dn0 = 0;
  int n_steps[3] = {0, 0, 0};              // steps of the pre-core, post-core and forward-only (kept factors) lists
  std::vector<int> posW;                   // as F2Program::posW (same layout for the same nc)
  std::vector<unsigned long long> desc;    // [step][nw * 64 lanes] packed word offsets into W (f2_program.cpp: f2_build_team)
};
bool f2_build_team(const LUProgram& P, int n, int nc, int nw, F2Team& T);
// ... for one wave per instance: list-scheduled steps of 64 lanes with up to three terms per lane, 16-byte descriptors (two words per lane in `desc`)
bool f2_build_steps(const LUProgram& P, int n, int nc, int nw, F2Team& T);

struct DeviceBlock {
  int type, count, n_nodes, n_ipar, n_par;
  int g_base, c_base, b_base, n_g, n_c, n_b;
  int* d_nodes = nullptr;
  std::vector<int> h_nodes;  // host copy (the fused kernel keeps an int16 copy in LDS)
  double* d_cache = nullptr; int n_cache = 0;   // generated external model: [B][n_cache][count] results of its setup pass (bias-independent statements)
  int va_model = -1;         // CADNIP_DEV_VA: the block's model id (ipar row 0)
  int va_tl = 0;             // generated external model: lanes per device when evaluated with one derivative direction per lane (16 / 32; stamp_csr.hip)
  bool mos1_plain = false;   // sp_mos1 block: every instance has gd = gs = OxideCap = 0 (set by cadnip_set_params)
  int* d_ipar = nullptr;
  double* d_par = nullptr;   // [B][n_par][count]
  // the stamping kernel's plan (stamp_plan.hpp; uploaded by stamp_csr.hip: build_stamp_plan): devices per tile, tiles per instance, and the
  // tables in device memory.  plan[0]: the general plan; plan[1]: the lane-pair plan of an sp_mos1 block (mos1_plain: fewer live rows),
  // empty for every other type -- the launch picks the one that matches the parameters in force
  int sp_cs = 0, sp_chunks = 0;
  struct PlanSet { StampShape shape; int *tptr = nullptr, *info = nullptr; uint4* rec = nullptr; unsigned short* rowoff = nullptr; };
  PlanSet plan[2];
};

struct ProfEntry { const char* name; double ms = 0; int64_t calls = 0; };

// step descriptors of one linear-solve program in device memory (f2_program.cpp: f2_build_steps / f2_build_team)
struct StepList { unsigned long long* d = nullptr; int len = 0, n_steps[3] = {0, 0, 0}; };   // len: 64-bit words; n_steps: pre-core, post-core, forward-only (kept factors)

// Everything the LDS-resident kernels (fused Newton kernels, program LU) keep per handle; built on demand by fused2.hip, rebuilt when the
// LU program changes (`dirty`) or cadnip_set_params changed a block (`blk_dirty`)
struct FusedState {
  bool dirty = true, blk_dirty = true;
  // packed structure tables (fused2.hip: f2_prepare) and the linear-solve program they belong to
  unsigned int* d_tab = nullptr;
  int off[16] = {0};          // section offsets in 32-bit words
  int lu_len = 0;             // 32-bit words of the linear-solve prefix (entry program, load map, permutations): what the program LU stages
  int lean_lo = 0, lean_end = 0;   // the words [lo, end) the lean kernels stage (permutations, stamp tables, node tables)
  int full_len = 0;           // words the full-table kernels stage
  int lu_words = 0, nc = 0, dn0 = 0, n_pre = 0, n_post = 0, n_fwd = 0;
  std::vector<int> nodes_off; // per device block: offset (int16 units) of its node table inside the NODES section
  StepList steps1;            // one wave per instance (lean sweep kernel, k_lu_f2s): three-term list-scheduled steps, two words per lane
  StepList steps4;            // ... for a team of four waves, read from global memory (k_lu_steps)
  StepList team[2];           // team kernel: teams of 2 (three-term steps) / 4 waves (one-term level-aligned steps)
  // device-block descriptors and the facts of their list (fused2.hip: fused2_blocks)
  void* d_blk = nullptr;
  int n_blk = 0, rc_blk = -1, src_blk = -1;   // first capacitor / resistor block, first independent-source block of the list
  int src_count = 0;          // devices of block src_blk (the first 64 are pinned to lanes and may have their segment cached: src_cache.hpp)
  // the block list as lds_layout.hpp: f2_shape_ok reads it: types and counts of the two pinned blocks and of the one block beside them (of a
  // list of three; a type of -1: no such block)
  int src_type = -1, rc_type = -1, rc_count = 0, dev_type = -1, dev_plain = 0, dev_count = 0;
  int par_words = 0;          // team kernel: doubles of the LDS-staged sp_mos1 parameter rows of one instance
  // buffers of the launches
  int* d_queue = nullptr;     // dynamic instance queue
  double* d_lufac = nullptr; size_t lufac_cap = 0;   // Newton mode 1: kept factors of the non-resident instances [B][lu_words]
  int n_cu = 0;               // compute units of the device (queried by the handle's first launch plan, fused2.hip: plan_facts; MI355X: 256)
  void release();             // frees every device buffer; the next use builds everything again
};

// One transfer buffer of the AC sweeps' pool; cap_bytes reads 0 until an allocation stands (api.hip: ac_reserve)
struct AcSlot { void* p = nullptr; size_t cap_bytes = 0; };
enum { AC_MAX_IN = 8, AC_MAX_OUT = 7 };    // the most a family transfers: the sensitivity sweep's inputs, the Arnoldi sweep's outputs
// The device buffers of the running sweep's transfers, in the order its entry point lists them (the launchers below name each family's
// order); null: a transfer this call does not make
struct AcIo {
  void *in[AC_MAX_IN], *out[AC_MAX_OUT];
  const double* din(int i) const { return (const double*)in[i]; }
  const int* iin(int i) const { return (const int*)in[i]; }
  double* dout(int o) const { return (double*)out[o]; }
  int* iout(int o) const { return (int*)out[o]; }
};

// AC sweeps (ac_lu.hip; api.hip: ac_sweep): the pivot lists of the complex factorisation -- the rows whose diagonal is final after the load
// (list 0) / after factor level l (list l + 1); ~row marks a constant-1 pivot (LUProgram::unit) -- and ONE pool of transfer buffers for all
// six families.  Only one sweep runs at a time, between an idle stream and a drained one, so slot i is whatever the running sweep's i-th
// input / output is: grown on demand to that transfer's bytes, never shrunk, holding whatever the last sweep left (every family's kernel
// writes every word it downloads).  A handle's resident transfer memory is its largest sweep's, not the sum over the families it has run
struct AcState {
  bool dirty = true;                       // the LU program changed: the pivot lists are built again
  int *d_piv_rows = nullptr, *d_piv_lev_ptr = nullptr;
  unsigned char* d_nodiag = nullptr;       // [n] 1 = a voltage node whose diagonal is not in the pattern: its gmin lives in the residuals only
  AcSlot in[AC_MAX_IN], out[AC_MAX_OUT];   // the pool: uploaded whole once per call / one chunk of systems, downloaded per chunk
  // the adjoint families: the transposed-solve tables of the LU program (lu_transpose.hpp), built with the pivot lists under `dirty` but
  // only once an adjoint path is asked for (`adj_ready`)
  bool adj_ready = false;
  int *d_t_colptr = nullptr, *d_t_pos = nullptr, *d_t_row = nullptr, *d_t_diag = nullptr;
  int *d_ut_rows = nullptr, *d_ut_lev_ptr = nullptr, *d_lt_rows = nullptr, *d_lt_lev_ptr = nullptr;
  int *d_a_colptr = nullptr, *d_a_row = nullptr, *d_a_pos = nullptr;
  int n_ut_lev = 0, n_lt_lev = 0;
  // HBM-resident form (k_ac_hbm; cadnip_ac_set_memory, ac_hbm_plan.hpp): the setting, the persistent waves' workspace
  // (grown on demand like the pool, released with the handle) and what the last AC / adjoint call ran (cadnip_ac_plan_info)
  int memory = CADNIP_AC_LDS, max_waves = 0;
  double* d_work = nullptr; size_t cap_work = 0;   // cap_work: bytes
  int n_cu = 0;                                    // compute units of the device (queried by the first HBM plan)
  int64_t last[4] = {CADNIP_AC_LDS, 0, 0, 0};      // memory, n_waves, work_bytes, lds_bytes
  // the overlay (cadnip_ac_set_overlay; ac_lu.hip: AcOvl): positions, their inverse map over the CSR pattern, the values [B][F][ovl_n] complex
  // and the grid the table was made for -- a solve under it must name the same grid, bit for bit.  ovl_n == 0: none is set
  int ovl_n = 0;
  std::vector<double> ovl_omega;
  int *d_ovl_pos = nullptr, *d_ovl_map = nullptr;
  double* d_ovl_val = nullptr;
  template <class F> void each_adjoint_buffer(F f) {
    f((void**)&d_t_colptr); f((void**)&d_t_pos); f((void**)&d_t_row); f((void**)&d_t_diag); f((void**)&d_ut_rows); f((void**)&d_ut_lev_ptr);
    f((void**)&d_lt_rows); f((void**)&d_lt_lev_ptr); f((void**)&d_a_colptr); f((void**)&d_a_row); f((void**)&d_a_pos);
  }
};

// Transport delays in the transient (cadnip_tran_set_delay; delay.hip, delay_plan.hpp): the plan's tables, the per-instance terms and the
// history ring, all in device memory.  n_term == 0: no spec is set -- nothing is allocated and cadnip_tran_run launches nothing new
struct DelayState {
  int n_pos = 0, n_term = 0, n_taps = 0, n_rows = 0, depth = 0;
  double tau_min = 0.0, t0 = 0.0;   // smallest delay of the batch (the step clamp); start of the run in flight
  int *d_pos = nullptr, *d_taps = nullptr, *d_rows = nullptr, *d_row_ptr = nullptr, *d_term_tap = nullptr;
  unsigned char* d_row_store = nullptr;     // [n_rows] 1 = no device stamps this row of b: the kernel stores, and the run clears it at its end
  double *d_tau = nullptr, *d_w = nullptr, *d_W = nullptr;               // [B][n_term] in the plan's grouped order; [B][n_pos]
  double *d_hist_t = nullptr, *d_hist_v = nullptr, *d_v_init = nullptr;  // [B][depth], [B][n_taps][depth], [B][n_taps]
  int *d_head = nullptr, *d_count = nullptr;                              // [B] ring head and count
  template <class F> void each_buffer(F f) {
    f((void**)&d_pos); f((void**)&d_taps); f((void**)&d_rows); f((void**)&d_row_ptr); f((void**)&d_term_tap); f((void**)&d_row_store);
    f((void**)&d_tau); f((void**)&d_w); f((void**)&d_W); f((void**)&d_hist_t); f((void**)&d_hist_v); f((void**)&d_v_init);
    f((void**)&d_head); f((void**)&d_count);
  }
};

// Transient parameter sensitivities (cadnip_tran_set_sens; tran_sens.hip, tran_sens_plan.hpp): the group table, the sensitivity history and
// output, and the snapshot of the bases' controller state that one stage works from.  n_group == 0: no spec is set -- nothing is allocated
// and cadnip_tran_run launches nothing new
struct SensState {
  int n_group = 0, K = 0, nh = 0, n_save = 0, n_obs = 0;
  bool inited = false;                            // cadnip_tran_sens_init has run since the last transient
  int *d_members = nullptr, *d_slot_of = nullptr; // [n_group][2 + 2 K]; [B] group * (2 + 2 K) + member, -1 = in no group
  double* d_delta = nullptr;                      // [n_group][K]
  double *d_hist = nullptr, *d_out = nullptr;     // [n_group][K][nh][n] newest first; [n_group][K][n_save][n_obs]
  double *d_snap = nullptr, *d_alpha = nullptr;   // [n_group][4] t, h, hprev, hpp before the update; [n_group][4] a0 .. a3 of the accepted step
  int *d_snap_i = nullptr, *d_accept = nullptr, *d_flag = nullptr;   // [n_group][3] nhist, order, save_idx; [n_group]; [n_group]
  long long* d_snap_cnt = nullptr;                // [n_group] accepted-step counter before the update
  template <class F> void each_buffer(F f) {
    f((void**)&d_members); f((void**)&d_slot_of); f((void**)&d_delta); f((void**)&d_hist); f((void**)&d_out); f((void**)&d_snap); f((void**)&d_alpha);
    f((void**)&d_snap_i); f((void**)&d_accept); f((void**)&d_flag); f((void**)&d_snap_cnt);
  }
};

}  // namespace cadnip

struct CadnipHandle {
  int device = 0;
  hipStream_t stream = nullptr;
  int B = 0;
  // structure (host copies kept for the symbolic phase)
  int n = 0, n_nodes = 0, n_currents = 0, n_charges = 0, n_limits = 0, nnz = 0;
  std::vector<int> h_rowptr, h_colidx, h_to_ref;
  std::vector<int> h_g_ptr, h_g_slots, h_c_ptr, h_c_slots, h_b_ptr, h_b_slots;   // gather lists: the fused kernel's tables invert them (fused2.hip)
  int ns_g = 0, ns_c = 0, ns_b = 0, ns = 0;
  std::vector<cadnip::DeviceBlock> blocks;
  std::vector<double> h_limit_init;
  CadnipSpec spec{1, 1e-12, 0.0, 1.0};
  int initjct = 0;
  // device: structure
  int *d_rowptr = nullptr, *d_colidx = nullptr, *d_to_ref = nullptr;
  int *d_g_ptr = nullptr, *d_g_slots = nullptr, *d_c_ptr = nullptr, *d_c_slots = nullptr, *d_b_ptr = nullptr, *d_b_slots = nullptr;
  unsigned char* d_diag_flag = nullptr;   // [nnz] 1 where the entry is G[i,i] of a voltage node
  int* d_long_rows = nullptr;   // rows with more than LONG_LIST entries (kernels.hip: k_residual_long)
  int n_long_rows = 0;
  double* d_dump = nullptr;     // non-null only inside cadnip_get_contributions: [B][ns] staged contributions (stamp_csr.hip)
  unsigned* d_prep = nullptr;   // words the stamping kernels do not store themselves (stamp_csr.hip: k_stamp_prep)
  int n_prep = 0, n_prep_atomic = 0;   // the first n_prep_atomic words are rewritten before every restamp
  bool prep_stale = true;              // unstamped node diagonals may still hold a gshunt of an earlier restamp
  double* d_wave = nullptr;
  double* d_limit_init = nullptr;
  // per-instance homotopy parameters of the DC fallback chain (solve.jl:720-850); equal to spec.gshunt / spec.srcFact
  // except while cadnip_dc_run walks an instance through gshunt / source stepping
  double *d_gshunt = nullptr, *d_srcfact = nullptr;
  std::vector<double> held_gshunt, held_srcfact;   // what upload_homotopy (their only writer) last put there; empty = nothing known
  bool homotopy = false;     // some instance has gshunt != 0 or srcFact < 1: the fused kernel (no homotopy terms) must not run
  // device: per-instance state [B][..]
  double *d_u = nullptr, *d_du = nullptr, *d_t = nullptr, *d_gamma = nullptr;
  double *d_G = nullptr, *d_C = nullptr, *d_b = nullptr, *d_J = nullptr, *d_resid = nullptr, *d_delta = nullptr;
  double *d_limit_w = nullptr, *d_LU = nullptr, *d_tmp = nullptr;
  int* d_flags = nullptr;        // [B] per-instance status bits (1 = singular pivot, 2 = non-finite)
  int* d_active = nullptr;       // [B] 1 = instance takes part in the next launches
  int* d_nonfinite = nullptr;    // [B] raised by the assemble kernels when a stamped value is NaN / Inf
  int* d_cold = nullptr;         // [B] 1 = the instance's DC solve is a cold start: initjct (armed per launch) applies to it (solve.jl:615-625: iszero(u0))
  // LU
  bool analyzed = false;
  cadnip::LUProgram lu;
  int *d_load_src = nullptr, *d_load_dst = nullptr, *d_ent_pos = nullptr, *d_ent_diag = nullptr, *d_ent_ptr = nullptr;
  int *d_term_a = nullptr, *d_term_b = nullptr, *d_lev_ptr = nullptr;
  int *d_lu_rowptr = nullptr, *d_lu_col = nullptr, *d_lu_diag = nullptr, *d_rperm = nullptr, *d_cperm = nullptr;
  int *d_fwd_rows = nullptr, *d_fwd_lev_ptr = nullptr, *d_bwd_rows = nullptr, *d_bwd_lev_ptr = nullptr;
  std::vector<unsigned char> leaf_unit_ok;   // per unknown: its diagonal is one constant G stamp, no C stamp (leaf-first pivot order, symbolic.cpp)
  cadnip::LULeaves leaves;    // charge / limit ranges of the unknown layout [V | I | q | lim]
  bool va_ext = false;        // the circuit uses an external generated model (va_generated_ext.hpp): not compiled into the fused kernel
  cadnip::FusedState f2;      // the LDS-resident kernels' tables, step lists and buffers (fused2.hip, lu_f2.hip)
  cadnip::AcState ac;         // AC sweep: pivot lists and transfer buffers (ac_lu.hip; released with the handle's other buffers in cadnip_destroy)
  cadnip::DelayState dly;     // transient: delayed stamps and their history ring (delay.hip; released in cadnip_destroy)
  cadnip::SensState sns;     // transient: parameter sensitivities (tran_sens.hip; released in cadnip_destroy)
  // driver state (allocated lazily)
  struct Driver* drv = nullptr;
  // profiling
  bool prof_on = false;
  std::vector<cadnip::ProfEntry> prof;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // pinned scratch
  int* h_pinned = nullptr;
  int* d_pinned = nullptr;
  // mapped pinned staging area of the host-pointer entry points (api.hip: stage_up / stage_down / stage_finish): small transfers are moved
  // by a copy KERNEL on the stream that reads / writes the staging area across the bus; large ones are blocking copies
  char* h_stage = nullptr; char* d_stage = nullptr; size_t stage_bytes = 0, stage_off = 0;   // (d_stage: the same memory as the device sees it)
  struct PendingDown { void* dst; const void* src; size_t bytes; };
  // cadnip_newton_step: the launch sequence of one call as an instantiated HIP graph per variant (refresh or not); `graph_epoch` moves whenever
  // something a captured kernel argument depends on changes (spec, parameters' structure, LU program): a stale graph is captured again
  struct StepGraph { hipGraphExec_t exec = nullptr; unsigned long long epoch = 0, warmed = 0; };
  StepGraph step_graph[4];      // per-op: no refresh / refresh; fused: no refresh / refresh
  unsigned long long graph_epoch = 1;
  std::vector<PendingDown> stage_pending;   // the same words as the device sees them: small results are PUBLISHED there by a kernel (driver.hip: k_publish_int), not copied
};

namespace cadnip {
// symbolic.cpp
// KLU's ordering (klu_order.cpp): column sequence, the maximum transversal's row per column, block boundaries; false = structurally singular
bool klu_style_order(int n, const std::vector<int>& rowptr, const std::vector<int>& colidx, std::vector<int>& colorder, std::vector<int>& match_row, std::vector<int>& block_ptr);
int lu_analyze(int n, const std::vector<int>& rowptr, const std::vector<int>& colidx, const std::vector<double>& vals,
               double pivot_tol, bool sample, LUProgram& out, std::string& err, const LULeaves* leaves = nullptr);
// kernels.hip launchers (all asynchronous on h->stream)
int launch_rebuild(CadnipHandle* h);                       // stamp_csr.hip: one stamp + reduce kernel per device type at (d_u, d_t)
int build_stamp_plan(CadnipHandle* h, const CadnipStructure* s);   // stamp_csr.hip, once per structure
int launch_stamp_block(CadnipHandle* h, int block);                // stamp_csr.hip: the stamping kernel of one device block
int launch_residual(CadnipHandle* h, const double* d_du);  // d_resid = C du + G u - b
int launch_jacobian(CadnipHandle* h);                      // d_J = G + gamma C
int launch_factor(CadnipHandle* h, bool fuse_jacobian);    // LU of J (or of G + gamma C)
int launch_solve(CadnipHandle* h, const double* d_rhs, double* d_x);
// k_lu with the name of its profile class (lu_f2.hip runs it as one of launch_factor_solve's kernels); threads: lu_plain_threads with the same do_factor (whole waves, 64 .. 1024: else CADNIP_BADARG)
int lu_plain_threads(const CadnipHandle* h, bool do_factor);
int launch_lu(CadnipHandle* h, const char* name, int do_factor, int do_solve, bool fuse_jacobian, const double* d_rhs, double* d_x, int threads);
// lu_f2.hip.  kernel: CADNIP_LUK_* (auto: the drivers' choice); info [6] (optional): what ran (cadnip_factor_solve).  dry: choose, fill info,
// launch nothing.  A forced kernel that does not apply: CADNIP_BADARG
int launch_factor_solve(CadnipHandle* h, bool fuse_jacobian, const double* d_rhs, double* d_x, int kernel = CADNIP_LUK_AUTO, int* info = nullptr,
                        bool dry = false);
int upload_lu(CadnipHandle* h);
// ac_lu.hip: the launch plan of k_ac<W, S> for n_sys systems -- wpb_req 0: the plan's choice (CADNIP_AC_WPB overrides it), else 1 / 2 / 4 / 8.
// wpb 0: an invalid request, or the work arrays of wpb_req (of one, for 0) systems exceed LDS_BUDGET
struct AcPlan { int wpb = 0; size_t shmem = 0; };
AcPlan ac_lu_plan(const CadnipHandle* h, long n_sys, int wpb_req, bool sens = false);   // sens: of the families with four n-vectors (AcSensSys, AcArnoldiSys), 16 (nnz(L+U) + 4 n) bytes per system
// the home of a call's work arrays under the handle's setting (h->ac.memory) and its plan: memory CADNIP_AC_LDS -> lds, CADNIP_AC_HBM -> hbm
// (ac_hbm_plan.hpp, on the device's compute units and h->ac.max_waves); -1: refused -- an invalid wpb, or the circuit fits neither
struct AcLaunch {
  int memory = -1; AcPlan lds; AcHbmPlan hbm;
  int wpb() const { return memory == CADNIP_AC_HBM ? hbm.wpb : lds.wpb; }
  int workgroups(long n_sys) const { return memory == CADNIP_AC_HBM ? (hbm.n_waves + hbm.wpb - 1) / hbm.wpb : (int)((n_sys + lds.wpb - 1) / lds.wpb); }
};
AcLaunch ac_launch_plan(CadnipHandle* h, long n_sys, int wpb_req, bool sens = false);
// the pivot lists of the current LU program, on demand; adjoint: the transposed-solve tables (lu_transpose.hpp) as well
int ac_lu_prepare(CadnipHandle* h, bool adjoint = false);
// The launchers of the six families: systems [s0, s0 + n_sys) of the call's grid (s = b * n_freq + f) under the plan p, inputs read from and
// outputs written (from index 0) to the buffers of io.  `in:` / `out:` name the order of io's slots; an output the caller does not want is null.
// in: omega, b_ac [B][n].  out: x, berr, flags
int launch_ac_lu(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_freq, long s0, int n_sys, double gmin);
// A^T x = c through AcAdjSys (needs ac_lu_prepare(h, true)).  in: omega, c [B][n], pairs [n_pairs][2].  out: h[k] = x[p_k] - x[n_k], x (optional), berr, flags
int launch_ac_adjoint(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_pairs);
// A x_k = b_k for n_rhs columns per instance through AcLuMultiSys (one factorisation per system).  in: omega, rhs [B][n_rhs][n], pairs (none with
// n_pairs == 0).  out: per (system, column) h (none with n_pairs == 0), x (optional; required with n_pairs == 0), berr, flags
int launch_ac_multi(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_rhs, int n_pairs);
// ... of A^T x_k = c_k through AcAdjMultiSys (needs ac_lu_prepare(h, true)): the slots of launch_ac_multi
int launch_ac_adjoint_multi(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_rhs, int n_pairs);
// the n_base x n_freq grid of cadnip_ac_sens (b an index into the base list) through AcSensSys (needs ac_lu_prepare(h, true); p must come from
// ac_launch_plan(.., sens = true)); n_par columns, pair: the output pair.  in: omega, base [NB], plus [NB][n_par], minus, scale, b_ac [NB][n],
// db [NB][n_par][n] (optional: zeros), c [n].  out: y, s, x and lambda (optional), berr [2], flags [n_par]
int launch_ac_sens(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_base, int n_par, const int* pair);
// the B x n_shift grid of cadnip_ac_arnoldi through AcArnoldiSys (p must come from ac_launch_plan(.., sens = true): the same four n-vectors); m
// steps, breakdown tolerance tol.  in: omega, b_ac [B][n], pairs (none with n_pairs == 0).  out: H, l (none with n_pairs == 0), V, beta, meff, berr, flags
int launch_ac_arnoldi(CadnipHandle* h, const AcLaunch& p, const AcIo& io, int n_shift, long s0, int n_sys, double gmin, int m, double tol, int n_pairs);
// delay.hip: the transient's delayed stamps (cadnip_tran_set_delay), asynchronous on h->stream.  The driver passes its own per-instance arrays:
// status (0 = running), t (accepted time), u0 (newest accepted vector [B][n])
void delay_release(CadnipHandle* h);                                       // frees everything; no spec is set afterwards
int launch_delay_init(CadnipHandle* h, double t0);                         // v_init and the first ring entry (t0, u[tap]) from h->d_u
int launch_delay_apply(CadnipHandle* h, int* d_status);                    // G -= W, b[row] -= sum w ud(col, tcur - tau) where the rebuild stamped; ends an instance whose look-up overflows
int launch_delay_record(CadnipHandle* h, const double* d_t, const double* d_u0, int* d_status);   // appends accepted points
int launch_delay_clear(CadnipHandle* h);                                   // zeroes the rows of b that only k_delay_apply writes
// tran_sens.hip: the transient's sensitivity stage (cadnip_tran_set_sens), asynchronous on h->stream; t: the arguments of the run's controller kernels
struct TranArgs;
void sens_release(CadnipHandle* h);                                        // frees everything; no spec is set afterwards
int launch_sens_begin(CadnipHandle* h, const TranArgs& t);                 // after k_tran_init: parks every member but the bases, writes s(t0) to the save points at or before t0
int launch_sens_snapshot(CadnipHandle* h, const TranArgs& t);              // before k_tran_update: the bases' step in flight
int launch_sens_stage(CadnipHandle* h, const TranArgs& t);                 // after k_tran_update: gather, restamp, residual, right-hand sides, one LU launch, record
int upload_homotopy(CadnipHandle* h, const double* gshunt /* [B] or null = spec */, const double* srcfact /* [B] or null = spec */);
int restore_masks(CadnipHandle* h, bool cold);   // api.hip: d_active (and with `cold` d_cold, first) back to all ones, as blocking copies: every instance takes part again
int launch_calib_copy(CadnipHandle* h, long n, int reps);
#define TRY_RC(x) do { int _rc_ = (x); if (_rc_) return _rc_; } while (0)
struct MultiCopy { struct Seg { unsigned* dst; const unsigned* src; size_t words; }; Seg seg[8]; int n = 0;
  void add(void* dst, const void* src, size_t bytes) { seg[n].dst = (unsigned*)dst; seg[n].src = (const unsigned*)src; seg[n].words = bytes / 4; ++n; } };
int dev_multi_async(CadnipHandle* h, const MultiCopy& m, bool to_host);   // kernels.hip: up to 8 word copies / clears (src = null) in one launch
int launch_norm2(CadnipHandle* h, const double* d_x, double* d_out);      // kernels.hip: per-instance 2-norm
int dev_zero_async(CadnipHandle* h, void* p, size_t bytes);               // kernels.hip: zero-fill as a kernel on the handle's stream (ordered with the other kernels)
int dev_copy_async(CadnipHandle* h, void* dst, const void* src, size_t bytes, bool to_host);   // kernels.hip: word copy as a kernel on the handle's stream
int launch_negate(CadnipHandle* h, double* d_x, long n);
struct TranArgs;                                                          // tran_ctrl.hpp
int launch_fused2_rounds(CadnipHandle* h, const TranArgs& t, int rounds); // fused2.hip
// one Newton iteration in the team kernel (fused2.hip): device-visible pointers (device memory or mapped pinned host memory) of its inputs and outputs;
// gamma_keep / t_keep: device arrays that also receive the caller's gamma / t (the handle's state stays what the per-op entry points would leave)
struct FusedStepIO { const double *u, *du, *gamma, *t; double *gamma_keep, *t_keep, *delta, *resid, *norm; int* flags; int reps = 1, skip = 0; };   // reps / skip: measurement (cadnip_debug_step_time)
int launch_fused_step(CadnipHandle* h, int refresh, const FusedStepIO& io);
int launch_va_setup(CadnipHandle* h, DeviceBlock& b);                        // stamp_csr.hip: the setup pass of a generated external model's block
int fused2_tables(CadnipHandle* h);                                        // builds the packed tables on demand; CADNIP_OK: they exist
// The facts both launch planners read (launch_plan.hpp), gathered from the handle.  tables: build the packed tables first if need be; blocks:
// and, for a circuit the fused kernels can address, the block descriptors.  Once the tables exist the device is asked for its compute units,
// at the handle's first such call (a handle that is refused before, or takes k_lu whatever the tables hold, makes no HIP call here as before).
// Returns the failure of that query or of the descriptors' upload
int plan_facts(CadnipHandle* h, bool tables, bool blocks, PlanFacts& f);
// What a fused launch would run (fused2.hip: fused2_plan; launch_plan.hpp: f2_choose decides).  rc != CADNIP_OK: the fused kernels do not apply now, and launch_fused2_* return
// rc; !circuit_ok: they never apply to this circuit / Newton mode -- the drivers take the per-op kernels (still on the GPU) instead
struct F2Plan : F2Choice {             // what launch_plan.hpp: f2_choose chose, and ...
  const StepList* steps = nullptr;      // ... the step list it named: the descriptors staged behind the tables (null: the pass program of the full table)
};
// topt: the transient options of the call the plan is for (null: none -- the fixed form is then never chosen)
F2Plan fused2_plan(CadnipHandle* h, F2Mode mode, int newton_mode, const TranArgs* topt = nullptr);
int launch_fused2_dc(CadnipHandle* h, const TranArgs& t, int rounds, double abstol, int maxiters, int use_pcnr, int mode, int initjct, int* d_dcstate);
struct ProfScope {
  CadnipHandle* h; int idx;
  ProfScope(CadnipHandle* h, const char* name);
  ~ProfScope();
};
}  // namespace cadnip
