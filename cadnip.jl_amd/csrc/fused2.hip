// fused2.hip -- host side of the fused Newton kernels: the packed structure tables, the launch plan and the launchers.
//
// The kernels keep all the Newton rounds of a launch on the chip: the circuit *structure* (tables, step descriptors) resident in LDS and
// shared by the workgroup, each instance's Jacobian, right-hand side, solution and BDF history term resident in LDS, the step controller's
// scalars in registers; HBM is touched for device parameters, the predictor / history vectors and the outputs.  lds_layout.hpp is the map
// of that LDS block for every kernel; launch_plan.hpp (f2_choose, through fused2_plan() below) decides which kernel runs and with what:
//   * sweep kernel k_fused2<WPB, DC, VAR> (fused2_kernel.hpp): WPB instances per workgroup, one 64-lane wave each, waves never wait for
//     each other.  VAR 0, the benchmark's kernel: lean device set (linear elements, sources, plain sp_mos1), every device emits its residual
//     directly (devices.hpp, Rn), the linear solve runs from list-scheduled step descriptors staged behind the lean range of the tables.
//     VAR 3: VAR 0 with the default transient call's switches fixed at compile time (lds_layout.hpp: f2_fixed_ok), taken whenever they hold.
//     VAR 4: VAR 3 with the circuit's block list fixed as well -- voltage sources, one pass of plain sp_mos1, capacitors: a CMOS cell
//     (lds_layout.hpp: f2_shape_ok) --, taken whenever the list has that shape.
//     VAR 1: direct residuals for every device type, the linear solve as the pass program of the full table.  VAR 2 (diagnostic,
//     CADNIP_F2_NODIRECT=1): the assembled residual r = J u + C beta - b from a J*u pass over the resident matrix.
//   * team kernel k_fteam<NW, STEP> (fused_team_kernel.hpp): 2 or 4 waves share one instance when the batch cannot fill the chip; STEP
//     mode is one Newton iteration for cadnip_newton_step_fused.
// In every variant stamps accumulate straight into J = G + a0*C at their LU positions (no slot buffer, no G / C), branch-free: a slot whose
// row or column is ground goes to a per-lane trash word.  Refactorisation, forward and back substitution are one entry-wise program
// W[pos] = (W[pos] - sum_k W[a_k]*W[b_k]) [/ W[piv]] over W = [ LU | rhs ] (f2_program.cpp).
// Summation order inside an nz differs from the per-op path (slot-major instead of COO order), so results agree with it to rounding
// (1e-13 relative), not bit for bit; the per-op path remains the reference ABI.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "fused_team_kernel.hpp"

namespace cadnip {

// ---- host side: build the packed tables once per (structure, LU program) ------------------------------------
struct F2Tables {
  std::vector<unsigned> data;   // 32-bit words
  int off[S_NSEC];
  void begin(int which) { if (data.size() & 1) data.push_back(0); off[which] = (int)data.size(); }
  void add16(const std::vector<int>& v) {
    for (size_t i = 0; i < v.size(); i += 2) data.push_back((unsigned)(v[i] & 0xFFFF) | ((i + 1 < v.size() ? (unsigned)(v[i + 1] & 0xFFFF) : 0u) << 16));
  }
  void add32(unsigned x) { data.push_back(x); }
  void add64(u64 x) { data.push_back((unsigned)x); data.push_back((unsigned)(x >> 32)); }
};

// one step list: built by `build`, uploaded; left empty (d = null) when the program does not exist for this circuit or the upload fails
template <class Build>
static void upload_steps(StepList& L, int lu_words, Build&& build) {
  if (L.d) (void)hipFree(L.d);
  L = StepList();
  F2Team TM;
  const size_t bytes = (build(TM) && TM.lu_words == lu_words) ? TM.desc.size() * sizeof(unsigned long long) : 0;
  if (!bytes || hipMalloc((void**)&L.d, bytes) != hipSuccess) { L.d = nullptr; return; }
  if (hipMemcpy(L.d, TM.desc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(L.d); L.d = nullptr; return; }
  L.len = (int)TM.desc.size();
  for (int li = 0; li < 3; ++li) L.n_steps[li] = TM.n_steps[li];
}

static bool f2_prepare(CadnipHandle* h, F2Tables& T) {
  const LUProgram& P = h->lu;
  FusedState& S = h->f2;
  const std::vector<int>&g_ptr = h->h_g_ptr, &g_slots = h->h_g_slots, &c_ptr = h->h_c_ptr, &c_slots = h->h_c_slots, &b_ptr = h->h_b_ptr, &b_slots = h->h_b_slots;
  const int n = h->n;
  if (n >= 32767) return false;
  // core size: the cheapest of {0, 8, 12, 16}; CADNIP_F2_NC forces one (diagnostic)
  F2Program G;
  {
    bool any = false;
    const char* force = getenv("CADNIP_F2_NC");
    for (int nc : {0, 8, 12, F2_NCMAX}) {
      if (nc > n || (force && atoi(force) != nc)) continue;
      F2Program C;
      if (!f2_build_program(P, n, nc, C)) continue;
      if (!any || C.cost < G.cost) { G = std::move(C); any = true; }
    }
    if (!any) return false;
  }
  const int y0 = G.lu_words, trash0 = G.lu_words + n;                 // W offsets
  if (trash0 + F2_TRASH >= 65535) return false;
  S.lu_words = G.lu_words; S.nc = G.nc; S.dn0 = G.dn0; S.n_pre = G.n_pre; S.n_post = G.n_post; S.n_fwd = G.n_fwd;
  std::vector<int> pinv(n), qinv(n);
  for (int k = 0; k < n; ++k) { pinv[P.rperm[k]] = k; qinv[P.cperm[k]] = k; }
  std::vector<int> dst(h->nnz, 0);
  for (size_t k = 0; k < P.load_src.size(); ++k) dst[P.load_src[k]] = G.posW[P.load_dst[k]];
  // slot -> W offset.  A slot that no nz gathers (ground row / column) goes to the trash word of its lane.
  std::vector<int> gs(h->ns_g, -1), cpos(h->ns_c, -1), crow(h->ns_c, 0), ccol(h->ns_c, 0), br(h->ns_b, -1);
  for (int i = 0; i < n; ++i)
    for (int e = h->h_rowptr[i]; e < h->h_rowptr[i + 1]; ++e) {
      for (int p = g_ptr[e]; p < g_ptr[e + 1]; ++p) gs[g_slots[p]] = dst[e];
      for (int p = c_ptr[e]; p < c_ptr[e + 1]; ++p) { cpos[c_slots[p]] = dst[e]; crow[c_slots[p]] = y0 + pinv[i]; ccol[c_slots[p]] = h->h_colidx[e]; }
    }
  for (int i = 0; i < n; ++i) for (int p = b_ptr[i]; p < b_ptr[i + 1]; ++p) br[b_slots[p]] = y0 + pinv[i];
  // the lane that writes slot s of a block is ((s - base) % count) % 64
  std::vector<int> lane_g(h->ns_g, 0), lane_c(h->ns_c, 0), lane_b(h->ns_b, 0);
  for (auto& b : h->blocks) {
    if (b.count == 0) continue;
    for (int s = 0; s < b.n_g * b.count; ++s) lane_g[b.g_base + s] = (s % b.count) & 63;
    for (int s = 0; s < b.n_c * b.count; ++s) lane_c[b.c_base + s] = (s % b.count) & 63;
    for (int s = 0; s < b.n_b * b.count; ++s) lane_b[b.b_base + s] = (s % b.count) & 63;
  }
  for (int s = 0; s < h->ns_g; ++s) if (gs[s] < 0) gs[s] = trash0 + lane_g[s];
  for (int s = 0; s < h->ns_b; ++s) if (br[s] < 0) br[s] = trash0 + lane_b[s];
  // ---- section order: [pass program, load map | permutations] = the prefix the per-op program LU (lu_f2.hip) stages; [permutations | stamp
  // tables, node tables] = the range the lean kernels stage (their linear solve runs from step descriptors, fused2_kernel.hpp: run_steps);
  // the J*u list of the assembled-residual variant last.  Range boundaries are multiples of 4 words (16-byte copies, aligned work arrays).
  auto pad4 = [&]() { while (T.data.size() & 3) T.data.push_back(0); };
  T.begin(S_ENT); for (u64 wv : G.lanes) T.add64(wv);
  T.begin(S_TERM); for (unsigned t : G.terms) T.add32(t);
  T.begin(S_LEV); for (u64 wv : G.passes) T.add64(wv);
  T.add64(0); T.add64(0);   // two empty passes: the kernel reads pass descriptors two ahead
  T.begin(S_LOADPOS); T.add16(dst);                 // csr entry -> W word: the per-op program LU loads J = G + gamma C through it
  pad4();
  S.lean_lo = (int)T.data.size();
  std::vector<int> qoff(n);
  for (int j = 0; j < n; ++j) qoff[j] = y0 + qinv[j];
  T.begin(S_QINV); T.add16(qoff);
  {
    std::vector<int> rowoff(n);                       // unknown index -> rhs word of its row (direct residuals, devices.hpp Rn)
    for (int i = 0; i < n; ++i) rowoff[i] = y0 + pinv[i];
    T.begin(S_ROWOF); T.add16(rowoff);
  }
  pad4();
  S.lu_len = (int)T.data.size();
  T.begin(S_GPOS); T.add16(gs);
  T.begin(S_CDESC);
  for (int s = 0; s < h->ns_c; ++s) {
    if (cpos[s] < 0) T.add64(pack4(trash0 + lane_c[s], trash0 + lane_c[s], 0, 0));
    else T.add64(pack4(cpos[s], crow[s], ccol[s], 0));
  }
  T.begin(S_BROW); T.add16(br);
  T.begin(S_NODES);
  S.nodes_off.clear();
  {
    std::vector<int> all;
    for (auto& b : h->blocks) { S.nodes_off.push_back((int)all.size()); all.insert(all.end(), b.h_nodes.begin(), b.h_nodes.end()); }
    T.add16(all);
  }
  pad4();
  S.lean_end = (int)T.data.size();
  T.begin(S_NZ);
  {
    // J*u adds every entry's product into its row with an LDS atomic, 64 entries per instruction.  In CSR order a long
    // row would put up to 64 same-address atomics into one instruction; ordered by (position within the row, row) the
    // entries of one instruction belong to different rows.
    std::vector<std::pair<int, int>> order;   // (rank in row, csr entry)
    for (int i = 0; i < n; ++i) for (int e = h->h_rowptr[i]; e < h->h_rowptr[i + 1]; ++e) order.push_back({e - h->h_rowptr[i], e});
    std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first < y.first; });
    std::vector<int> row_of(h->nnz);
    for (int i = 0; i < n; ++i) for (int e = h->h_rowptr[i]; e < h->h_rowptr[i + 1]; ++e) row_of[e] = i;
    for (auto& oe : order) { const int e = oe.second; T.add64(pack4(dst[e], y0 + pinv[row_of[e]], h->h_colidx[e], 0)); }
  }
  pad4();                                          // the work arrays behind the tables stay 16-byte aligned
  S.full_len = (int)T.data.size();                 // what the full-table kernels copy to LDS ends here
  // ---- the same program as straight-line steps (f2_program.cpp).  One wave per instance, lean variant: list-scheduled steps with three
  // terms per lane, staged in LDS; for a team of four waves: the per-op step LU (lu_f2.hip: k_lu_steps), read from global memory; the team
  // kernel (fused_team_kernel.hpp), staged in LDS: three-term steps for teams of two, one-term level-aligned steps for teams of four
  upload_steps(S.steps1, G.lu_words, [&](F2Team& TM) { return f2_build_steps(P, n, G.nc, 1, TM); });
  upload_steps(S.steps4, G.lu_words, [&](F2Team& TM) { return f2_build_steps(P, n, G.nc, 4, TM); });
  upload_steps(S.team[0], G.lu_words, [&](F2Team& TM) { return f2_build_steps(P, n, G.nc, 2, TM); });
  upload_steps(S.team[1], G.lu_words, [&](F2Team& TM) { return f2_build_team(P, n, G.nc, 4, TM); });
  return true;
}

struct F2DcOpts { double abstol; int maxiters, use_pcnr, mode, initjct; int* dcstate; };
struct F2StepOpts { int refresh; double *resid, *norm; int reps, skip; };   // cadnip_newton_step_fused: one Newton iteration in the team kernel (STEP mode)

void FusedState::release() {
  void* ptrs[] = {d_tab, steps1.d, steps4.d, team[0].d, team[1].d, d_blk, d_queue, d_lufac};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  d_tab = nullptr; steps1 = steps4 = team[0] = team[1] = StepList(); d_blk = nullptr; d_queue = nullptr; d_lufac = nullptr; lufac_cap = 0;
  dirty = blk_dirty = true;
}

// Build (or rebuild) the structure tables; CADNIP_BADARG if the circuit cannot be expressed in them (16-bit offsets)
int fused2_tables(CadnipHandle* h) {
  FusedState& S = h->f2;
  if (!h->analyzed) return CADNIP_NOTREADY;
  if (S.d_tab && !S.dirty) return CADNIP_OK;
  S.release();
  F2Tables T;
  if (!f2_prepare(h, T)) return CADNIP_BADARG;
  HIP_TRY(hipMalloc((void**)&S.d_tab, T.data.size() * sizeof(unsigned)));
  HIP_TRY(hipMemcpy(S.d_tab, T.data.data(), T.data.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  for (int i = 0; i < S_NSEC; ++i) S.off[i] = T.off[i];
  S.dirty = false;
  return CADNIP_OK;
}

// device-block descriptors of the fused kernels: rebuilt when the tables were, or when cadnip_set_params changed a block (sp_mos1 pairing)
// (whether the list stays within the lean device set: launch_plan.hpp, f2_lean)
static int fused2_blocks(CadnipHandle* h) {
  { int rc = fused2_tables(h); if (rc) return rc; }
  FusedState& S = h->f2;
  if (S.blk_dirty || !S.d_blk) {
    F2Block hb[F2_MAX_BLOCKS];
    int nb = 0;
    for (size_t bi = 0; bi < h->blocks.size() && nb < F2_MAX_BLOCKS; ++bi) {
      auto& b = h->blocks[bi];
      if (b.count == 0) continue;
      hb[nb++] = F2Block{b.d_ipar, b.d_par, b.type, b.count, b.n_par, b.g_base, b.c_base, b.b_base, S.nodes_off[bi], b.mos1_plain ? 1 : 0, -1};
    }
    // the heaviest device type first
    for (int i = 0; i < nb; ++i)
      for (int j = i + 1; j < nb; ++j)
        if ((hb[j].type == CADNIP_DEV_MOS1) > (hb[i].type == CADNIP_DEV_MOS1)) { F2Block tmp = hb[i]; hb[i] = hb[j]; hb[j] = tmp; }
    auto first_of = [&](int ta, int tb) { for (int i = 0; i < nb; ++i) if (hb[i].type == ta || hb[i].type == tb) return i; return -1; };
    S.rc_blk = first_of(CADNIP_DEV_CAPACITOR, CADNIP_DEV_RESISTOR);
    S.src_blk = first_of(CADNIP_DEV_VSOURCE, CADNIP_DEV_ISOURCE);
    S.src_count = S.src_blk >= 0 ? hb[S.src_blk].count : 0;
    S.src_type = S.src_blk >= 0 ? hb[S.src_blk].type : -1;
    S.rc_type = S.rc_blk >= 0 ? hb[S.rc_blk].type : -1;
    S.rc_count = S.rc_blk >= 0 ? hb[S.rc_blk].count : 0;
    S.dev_type = -1; S.dev_plain = 0; S.dev_count = 0;
    if (nb == 3 && S.src_blk >= 0 && S.rc_blk >= 0) {       // a list of three: the block beside the two pinned ones
      const F2Block& D = hb[3 - S.src_blk - S.rc_blk];
      S.dev_type = D.type; S.dev_plain = D.mos1_plain; S.dev_count = D.count;
    }
    S.n_blk = nb;
    // team kernel (fused_team_kernel.hpp): the parameter rows of the lane-paired sp_mos1 blocks are staged in LDS
    // ... of what the register-resident first pass over the first block does not cover (more than 32 MOSFETs, several blocks)
    S.par_words = 0;
    { bool first = true;
      for (int i = 0; i < nb; ++i)
        if (hb[i].type == CADNIP_DEV_MOS1 && hb[i].mos1_plain) {
          if (!first || hb[i].count > 32) { hb[i].lds_par = S.par_words; S.par_words += hb[i].n_par * hb[i].count; }
          first = false;
        } }
    if (!S.d_blk) HIP_TRY(hipMalloc((void**)&S.d_blk, sizeof(hb)));
    HIP_TRY(hipStreamSynchronize(h->stream));               // no launch in flight may still read the old descriptors
    HIP_TRY(hipMemcpy(S.d_blk, hb, sizeof(F2Block) * (size_t)nb, hipMemcpyHostToDevice));
    S.blk_dirty = false;
  }
  return CADNIP_OK;
}

// ---- the launch plan: launch_plan.hpp decides (f2_choose, lu_choose); what follows gathers what it reads and carries its effects out ----
// compute units of the device: asked once per handle, when a plan first gets as far as a rule that reads them
static int device_cus(CadnipHandle* h) {
  FusedState& S = h->f2;
  if (S.n_cu > 0) return CADNIP_OK;
  int cu = 0;
  const hipError_t e = hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, h->device);
  if (e != hipSuccess || cu <= 0) { set_last_error("hipDeviceGetAttribute", e); return CADNIP_HIPERROR; }
  S.n_cu = cu;
  return CADNIP_OK;
}

static StepFacts step_facts(const StepList& L) { StepFacts s; s.present = L.d != nullptr; s.len = L.len; for (int i = 0; i < 3; ++i) s.n_steps[i] = L.n_steps[i]; return s; }

int plan_facts(CadnipHandle* h, bool tables, bool blocks, PlanFacts& f) {
  FusedState& S = h->f2;
  f.B = h->B; f.n = h->n;
  for (auto& b : h->blocks) f.nb += b.count > 0;
  f.va_ext = h->va_ext; f.analyzed = h->analyzed; f.delayed = h->dly.n_term > 0;
  f.homotopy = h->homotopy || h->spec.gshunt != 0.0 || h->spec.srcFact < 1.0;
  f.tables = tables && fused2_tables(h) == CADNIP_OK;
  if (!f.tables) return CADNIP_OK;                        // (no rule reads further, and no HIP call has been made)
  TRY_RC(device_cus(h));
  f.n_cu = S.n_cu;
  f.lu_words = S.lu_words; f.nc = S.nc; f.n_pre = S.n_pre; f.n_post = S.n_post;
  f.lu_len = S.lu_len; f.lean_lo = S.lean_lo; f.lean_end = S.lean_end; f.full_len = S.full_len; f.loadpos_off = S.off[S_LOADPOS];
  f.steps1 = step_facts(S.steps1); f.steps4 = step_facts(S.steps4); f.team[0] = step_facts(S.team[0]); f.team[1] = step_facts(S.team[1]);
  if (!blocks || !f2_circuit_fits(f)) return CADNIP_OK;
  TRY_RC(fused2_blocks(h));
  f.par_words = S.par_words; f.n_blk = S.n_blk;
  f.src_blk = S.src_blk; f.src_type = S.src_type; f.src_count = S.src_count; f.rc_type = S.rc_type; f.rc_count = S.rc_count;
  f.dev_type = S.dev_type; f.dev_plain = S.dev_plain; f.dev_count = S.dev_count;
  int nb = 0;                                             // (the handle's order; fused2_blocks sorts its copy)
  for (auto& b : h->blocks)
    if (b.count > 0 && nb < F2_MAX_BLOCKS) f.blk[nb++] = BlockFacts{b.type, b.mos1_plain ? 1 : 0};
  return CADNIP_OK;
}

// The diagnostic switches CADNIP_F2_NODIRECT / _TEAM / _WPB / _STEPS_PACKED / _SRC_CACHE / _FIXED / _SHAPE, read at every plan: tests change
// them between simulators of one process (CADNIP_F2_NC: f2_prepare, where the tables are built; CADNIP_F2_DEBUG prints the plan, launch_fused2)
static int env_switch(const char* name) { const char* e = getenv(name); return e ? atoi(e) : SW_UNSET; }
static F2Switches f2_switches() {
  return F2Switches{env_switch("CADNIP_F2_NODIRECT"), env_switch("CADNIP_F2_TEAM"), env_switch("CADNIP_F2_WPB"), env_switch("CADNIP_F2_STEPS_PACKED"),
                    env_switch("CADNIP_F2_SRC_CACHE"), env_switch("CADNIP_F2_FIXED"), env_switch("CADNIP_F2_SHAPE")};
}

F2Plan fused2_plan(CadnipHandle* h, F2Mode mode, int newton_mode, const TranArgs* topt) {
  F2Plan p;
  PlanFacts f;
  if (int rc = plan_facts(h, !h->va_ext && h->analyzed, true, f)) { p.rc = rc; return p; }
  const F2CallOpts co = topt ? F2CallOpts{topt->newton_mode, topt->max_order, topt->step_rule, topt->use_pcnr} : F2CallOpts{};
  static_cast<F2Choice&>(p) = f2_choose(f, f2_switches(), mode, newton_mode, topt ? &co : nullptr);
  FusedState& S = h->f2;
  p.steps = p.step_list == F2_STEPS_1 ? &S.steps1 : p.step_list == F2_STEPS_TEAM2 ? &S.team[0] : p.step_list == F2_STEPS_TEAM4 ? &S.team[1] : nullptr;
  return p;
}

static int launch_fused2(CadnipHandle* h, const TranArgs& t, int rounds, const F2DcOpts* dc, const F2StepOpts* step = nullptr) {
  const F2Plan p = fused2_plan(h, dc ? F2_DC : step ? F2_STEP : F2_TRAN, t.newton_mode, dc || step ? nullptr : &t);
  if (p.rc) return p.rc;
  ProfScope ps(h, dc ? "fused2_dc" : step ? "fused_step" : "fused2_newton");
  FusedState& S = h->f2;
  F2Args f{};
  f.n_blk = S.n_blk; f.rc_blk = S.rc_blk; f.src_blk = S.src_blk;
  f.blk = (const F2Block*)S.d_blk;
  f.wave = h->d_wave;
  f.tab = S.d_tab;
  for (int i = 0; i < S_NSEC; ++i) f.off[i] = S.off[i];
  f.tab_len = p.tab_len; f.tab_lo = p.tab_lo;
  f.n = h->n; f.nnz = h->nnz; f.nnz_lu = S.lu_words;
  f.n_pre = S.n_pre; f.n_post = S.n_post; f.nc = S.nc; f.dn0 = S.dn0; f.n_fwd = S.n_fwd;
  if (p.steps) { f.team_desc = p.steps->d; f.team_desc_len = p.steps->len; f.ts_pre = p.steps->n_steps[0]; f.ts_post = p.steps->n_steps[1]; f.ts_fwd = p.steps->n_steps[2]; }
  f.step_predec = p.step_predec ? 1 : 0;
  f.src_words = p.src_words;
  f.step_refresh = step ? step->refresh : 0; f.step_resid = step ? step->resid : nullptr; f.step_norm = step ? step->norm : nullptr;
  f.step_reps = step ? step->reps : 1; f.step_skip = step ? step->skip : 0;
  if (p.keep_factors) {       // the kept factors of instances that are not resident live in HBM
    const size_t need = (size_t)h->B * S.lu_words;
    if (need > S.lufac_cap) {
      if (S.d_lufac) (void)hipFree(S.d_lufac);
      S.d_lufac = nullptr; S.lufac_cap = 0;
      HIP_TRY(hipMalloc((void**)&S.d_lufac, need * sizeof(double)));
      S.lufac_cap = need;
    }
    f.lufac = S.d_lufac;
  }
  f.rounds = rounds; f.B = h->B; f.t = t; f.cold = h->d_cold;
  f.dc_mode = 1;
  if (dc) { f.dc_abstol = dc->abstol; f.dc_maxiters = dc->maxiters; f.dc_pcnr = dc->use_pcnr; f.dc_mode = dc->mode; f.dc_initjct = dc->initjct; f.dcstate = dc->dcstate; }
  if (!S.d_queue) HIP_TRY(hipMalloc((void**)&S.d_queue, sizeof(int)));
  TRY_RC(dev_zero_async(h, S.d_queue, sizeof(int)));
  f.queue = S.d_queue;
  const bool debug = getenv("CADNIP_F2_DEBUG") != nullptr;
  if (p.nw) {
    f.par_words = S.par_words;
    if (debug) fprintf(stderr, "[cadnip f2] team of %d waves: B %d n_cu %d grid %d shmem %zu rounds %d nc %d steps %d+%d / %d\n", p.nw, h->B, S.n_cu, p.grid, p.shmem, rounds, S.nc, f.ts_pre, f.ts_post, f.ts_fwd);
    if (step) TRY_RC(fteam_launch_step(std::min(h->B, S.n_cu), p.shmem, h->stream, f));   // (one workgroup per CU, whatever p.grid allows)
    else TRY_RC(fteam_launch(p.nw, p.grid, p.shmem, h->stream, f));
  } else {
    const size_t tab_b = (size_t)p.tab_len / 2 * 8, desc_b = (size_t)lds_sweep_desc_words(f.team_desc_len, p.step_predec) * 8;
    if (debug) fprintf(stderr, "[cadnip f2] B %d n_cu %d wpb %d grid %d shmem %zu (tables %zu, steps %zu, per instance %zu) rounds %d nc %d passes %d+%d steps %d+%d / %d (%s) variant %d src-cache %d shape %d fixed %d\n", h->B, S.n_cu, p.wpb, p.grid, p.shmem, tab_b, desc_b, (p.shmem - tab_b - desc_b) / p.wpb, rounds, S.nc, S.n_pre, S.n_post, f.ts_pre, f.ts_post, f.ts_fwd, p.step_predec ? "pre-decoded" : "packed", p.var, p.src_words, p.shape ? 1 : 0, p.fixed ? 1 : 0);
    TRY_RC(p.shape ? f2_launch_variant<4>(p.wpb, dc != nullptr, p.grid, p.shmem, h->stream, f)
         : p.fixed ? f2_launch_variant<3>(p.wpb, dc != nullptr, p.grid, p.shmem, h->stream, f)
         : p.var == 0 ? f2_launch_variant<0>(p.wpb, dc != nullptr, p.grid, p.shmem, h->stream, f)
         : p.var == 1 ? f2_launch_variant<1>(p.wpb, dc != nullptr, p.grid, p.shmem, h->stream, f)
                      : f2_launch_variant<2>(p.wpb, dc != nullptr, p.grid, p.shmem, h->stream, f));
  }
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

int launch_fused2_rounds(CadnipHandle* h, const TranArgs& t, int rounds) { return launch_fused2(h, t, rounds, nullptr); }

// one Newton iteration of every instance in the team kernel (STEP mode): residual -> io.resid / io.norm (optional), Newton step -> io.delta,
// io.flags[inst] = 1 on a failed solve (the caller clears them); CADNIP_BADARG when the circuit has no team kernel (not lean, too large for LDS)
int launch_fused_step(CadnipHandle* h, int refresh, const FusedStepIO& io) {
  TranArgs t;
  memset(&t, 0, sizeof(t));
  t.u = (double*)io.u; t.du = (double*)io.du; t.delta = io.delta; t.limit_w = h->d_limit_w; t.tcur = (double*)io.t; t.gamma = (double*)io.gamma; t.active = h->d_active; t.flags = io.flags;
  t.t = io.t_keep; t.h = io.gamma_keep;                   // (STEP mode: where the caller's times / leading coefficients are also kept)
  t.B = h->B; t.n = h->n; t.n_limits = h->n_limits;
  F2StepOpts so{refresh, io.resid, io.norm, io.reps > 0 ? io.reps : 1, io.skip};
  return launch_fused2(h, t, 1 << 30, nullptr, &so);
}

int launch_fused2_dc(CadnipHandle* h, const TranArgs& t, int rounds, double abstol, int maxiters, int use_pcnr, int mode, int initjct, int* d_dcstate) {
  F2DcOpts dc{abstol, maxiters, use_pcnr, mode, initjct, d_dcstate};
  return launch_fused2(h, t, rounds, &dc);
}

}  // namespace cadnip
