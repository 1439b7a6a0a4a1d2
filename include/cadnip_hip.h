/*
 * cadnip_hip.h -- C ABI of libcadnip_hip.so, the MI355X (gfx950) replacement for the
 * CPU hot path of Cadnip.jl's transient analysis (reference: /root/reference/src/mna).
 *
 * Every entry point names the reference interface it replaces (file:line relative to
 * /root/reference).  The reference-side binding (Julia `ccall`) is shown in
 * INTEGRATION.md and shipped as source in cadnip.jl_amd/julia/CadnipHIP.jl.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; all indices are 0-based int32;
 *     all values are IEEE fp64.
 *   - every function returns a CadnipStatus (0 = ok); nothing throws across the ABI.
 *     The Julia shim maps CADNIP_SINGULAR -> LinearAlgebra.SingularException and
 *     CADNIP_NONFINITE -> DomainError so `_dc_solve_with_fallbacks`
 *     (src/mna/solve.jl:887-897) keeps working.
 *   - a handle owns all device memory; the caller owns every host array it passes.
 *     `*_host` arguments are host pointers (copied over PCIe inside the call);
 *     `cadnip_dev_ptr` exposes the handle's device buffers for zero-copy callers.
 *   - one handle = one (structure, GPU, HIP stream); handles are independent.
 *   - `n_instances` > 1 batches sweep points / Monte-Carlo instances that share one
 *     structure (CircuitSweep, src/sweeps.jl:387-424); all per-instance arrays are laid
 *     out instance-major: x[inst * n + i].
 */
#ifndef CADNIP_HIP_H
#define CADNIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CADNIP_OK = 0,
  CADNIP_BADARG = 1,
  CADNIP_SINGULAR = 2,   /* zero / non-finite pivot in some instance (KLU: SingularException) */
  CADNIP_NONFINITE = 3,  /* non-finite stamp value (reference: DomainError from device math) */
  CADNIP_HIPERROR = 4,
  CADNIP_NOTREADY = 5,   /* e.g. factor before analyze */
  CADNIP_NOCONV = 6      /* driver: some instance did not converge / step size underflow */
} CadnipStatus;

/* Device types: one stamping kernel per type (src/mna/devices.jl `stamp!` methods and the
 * Verilog-A stamp pattern src/vasim.jl:3319-3521). */
typedef enum {
  CADNIP_DEV_RESISTOR = 0,   /* devices.jl:498-510   nodes p,n        par: g=1/r                */
  CADNIP_DEV_CAPACITOR = 1,  /* devices.jl:531-534   nodes p,n        par: c                    */
  CADNIP_DEV_INDUCTOR = 2,   /* devices.jl:569-586   nodes p,n,I      par: l                    */
  CADNIP_DEV_VSOURCE = 3,    /* devices.jl:619-663   nodes p,n,I      par: dc,scale  ipar: wave */
  CADNIP_DEV_ISOURCE = 4,    /* devices.jl:698-737   nodes p,n        par: dc,scale  ipar: wave */
  CADNIP_DEV_VCVS = 5,       /* devices.jl:760-775   nodes op,on,ip,in,I          par: gain     */
  CADNIP_DEV_VCCS = 6,       /* devices.jl:797-808   nodes op,on,ip,in            par: gm       */
  CADNIP_DEV_CCVS = 7,       /* devices.jl:824-849   nodes op,on,ip,in,Iin,Iout   par: rm       */
  CADNIP_DEV_CCCS = 8,       /* devices.jl:865-881   nodes op,on,ip,in,Iin        par: gain     */
  CADNIP_DEV_DIODE = 9,      /* devices.jl:1370-1428 nodes p,n,lim    par: Is,nVt,vcrit  ipar: limit flag */
  CADNIP_DEV_DIODECAP = 10,  /* devices.jl:1558-1602 nodes p,n        par: Is,nVt,Cj0,Vj,m      */
  CADNIP_DEV_SIMPLEMOS = 11, /* devices.jl:1667-1749 nodes d,g,s      par: Vth,K,lambda,Cgd,Cgs */
  CADNIP_DEV_MOS1 = 12,      /* models/VADistillerModels.jl/va/mos1.va via vasim.jl:3319-3521;
                                nodes d,g,s,b,d_int,s_int,lim[4],q[4]; par: CADNIP_MOS1_NPAR derived
                                (setup+temp hoisted, mos1.va:695-897) values; ipar: flags       */
  CADNIP_DEV_BVSOURCE = 13,  /* devices.jl:1079-1102 BehavioralVoltageSource  nodes p,n,I   par: scale   ipar: program off,len */
  CADNIP_DEV_BISOURCE = 14,  /* devices.jl:1118-1131 BehavioralCurrentSource  nodes p,n     par: scale   ipar: program off,len */
  CADNIP_DEV_VA = 15,        /* generated Verilog-A module (src/vasim.jl:2993-3985 generate_mna_stamp_method_nterm): nodes = ports, internal
                              * nodes, one charge unknown per branch (-1 = none); par = module parameters, temperature [K], mfactor,
                              * gmin; ipar: model id (position in the list the library was generated from), voltage-dependent-charge
                              * bit mask.  One block per module; slot layout: cadnip.jl_amd/va/frontend.py */
  CADNIP_DEV_NTYPES = 16
} CadnipDeviceType;

#define CADNIP_MOS1_NPAR 36

typedef enum { CADNIP_WAVE_DC = 0, CADNIP_WAVE_PWL = 1, CADNIP_WAVE_PULSE = 2, CADNIP_WAVE_SIN = 3 } CadnipWaveKind;

/* Behavioural sources: `value_fn(get_voltage)` of the reference is a Julia closure; across the C ABI it is a
 * postfix program of doubles stored in wave_data[off .. off+len): opcode [operands].  The value is evaluated at the
 * current iterate and stamped as a fixed source (no Jacobian entries), exactly as devices.jl:1079-1131 does. */
typedef enum CadnipBsrcOp {
  CADNIP_BOP_CONST = 0,   /* + value                     */
  CADNIP_BOP_V = 1,       /* + unknown index p, n (-1 = ground): pushes u[p] - u[n] */
  CADNIP_BOP_TIME = 2,
  CADNIP_BOP_ADD = 10, CADNIP_BOP_SUB = 11, CADNIP_BOP_MUL = 12, CADNIP_BOP_DIV = 13, CADNIP_BOP_POW = 14,
  CADNIP_BOP_MIN = 15, CADNIP_BOP_MAX = 16,
  CADNIP_BOP_NEG = 20, CADNIP_BOP_EXP = 21, CADNIP_BOP_LOG = 22, CADNIP_BOP_SQRT = 23, CADNIP_BOP_ABS = 24,
  CADNIP_BOP_TANH = 25, CADNIP_BOP_SIN = 26, CADNIP_BOP_COS = 27
} CadnipBsrcOp;
#define CADNIP_BSRC_MAX_STACK 16

/* One block per device type.  Node / ipar arrays are shared by all instances (structure);
 * parameters are per instance and set with cadnip_set_params.
 *   nodes[k * count + d]  : unknown index (0-based) read/written by device d's k-th node
 *                           slot, -1 = ground
 *   ipar[k * count + d]   : integer parameters (wave kind, offset/length into wave_data, flags)
 *   slot ids              : device d's k-th G stamp owns slot  g_base + k*count + d  of the
 *                           per-instance slot buffer (likewise C, b); limit_w index
 *                           lim_base + k*count + d is written by limiting devices. */
typedef struct {
  int32_t type;      /* CadnipDeviceType */
  int32_t count;
  int32_t n_nodes;   const int32_t* nodes;
  int32_t n_ipar;    const int32_t* ipar;
  int32_t n_par;     /* doubles per device per instance */
  int32_t g_base, c_base, b_base; /* first slot of this block in the G / C / b slot ranges */
  int32_t n_g, n_c, n_b;          /* slots per device */
} CadnipDeviceBlock;

/* Fixed structure of one circuit == the reference's CompiledStructure
 * (src/mna/precompile.jl:75-124), in CSR and with slot->nz gather lists instead of the
 * positional COO->nz maps (value_only.jl:395-478). */
typedef struct {
  int32_t n, n_nodes, n_currents, n_charges, n_limits;
  /* unified G u C pattern (precompile.jl:413-421), CSR, column indices sorted */
  int32_t nnz;
  const int32_t* rowptr;    /* [n+1] */
  const int32_t* colidx;    /* [nnz] */
  const int32_t* to_ref_nz; /* [nnz] position of CSR entry k in the reference's CSC nzval order */
  /* device blocks */
  int32_t n_blocks;
  const CadnipDeviceBlock* blocks;
  int32_t n_wave_data; const double* wave_data; /* PWL (t,y) tables etc. */
  /* slot -> nz gather lists, each list in the reference's COO (stamp) order so that the
   * floating-point summation order equals `nzval[map[pos]] += v` (value_only.jl:414-418) */
  int32_t ns_g, ns_c, ns_b;
  const int32_t* g_ptr; const int32_t* g_slots; /* [nnz+1], [..] */
  const int32_t* c_ptr; const int32_t* c_slots;
  const int32_t* b_ptr; const int32_t* b_slots; /* [n+1],  [..]  deferred b (precompile.jl:508-515) */
  const int32_t* diag_nz;   /* [n_nodes] CSR position of G[i,i] or -1 (precompile.jl:451-467) */
  const double*  limit_init;/* [n_limits] (precompile.jl:119-123) */
} CadnipStructure;

/* MNASpec scalars (src/mna/solve.jl:57-70).  temp is per instance (corner sweeps); the
 * temperature dependence of device parameters is hoisted into the per-instance parameter
 * blocks, so only mode / gmin / gshunt / srcFact reach the kernels. */
typedef struct {
  int32_t mode;      /* 0 = :dcop, 1 = :tran, 2 = :tranop */
  double gmin, gshunt, srcFact;
} CadnipSpec;

typedef struct CadnipHandle CadnipHandle;

/* ---- lifetime -------------------------------------------------------------------------
 * replaces compile_structure + create_workspace (precompile.jl:312-443, 193-222) */
int cadnip_create(const CadnipStructure* s, int32_t n_instances, int32_t device, CadnipHandle** out);
void cadnip_destroy(CadnipHandle* h);
int cadnip_set_params(CadnipHandle* h, int32_t block, const double* par_host /* [B][n_par][count] */);
int cadnip_set_spec(CadnipHandle* h, const CadnipSpec* spec);
int cadnip_set_initjct(CadnipHandle* h, int32_t on);            /* DirectStampContext.initjct, value_only.jl:93-95 */

/* ---- the three hot-path callbacks ------------------------------------------------------
 * cadnip_rebuild   == fast_rebuild!(ws, u, t)                  precompile.jl:493-537
 * cadnip_residual  == fast_residual!(resid, du, u, ws, t)      precompile.jl:546-557
 * cadnip_jacobian  == fast_jacobian!(J, du, u, ws, gamma, t)   precompile.jl:568-585
 * Unlike the reference, residual and jacobian do NOT restamp: they reuse the stamps of the
 * last cadnip_rebuild (the reference restamps the whole circuit in each, precompile.jl:548,572).
 * u_host/du_host: [B][n]; t_host: [B] (instances may sit at different times); gamma_host: [B]. */
int cadnip_rebuild(CadnipHandle* h, const double* u_host, const double* t_host);
int cadnip_residual(CadnipHandle* h, const double* du_host, const double* u_host, double* resid_host);
int cadnip_jacobian(CadnipHandle* h, const double* gamma_host, double* J_ref_nz_host /* may be NULL */);
/* fast_jacobian!(J::Matrix, ...) of a structure compiled with dense = true (precompile.jl:588-603; the form the reference's canonical boundary
 * test drives, test/mna/audio_integration.jl:505-520): J = G + gamma C as a dense matrix per instance, [B][n * n] in Julia's column-major
 * layout (J[i, j] at j * n + i), structural zeros written as 0.  Meant for the small systems that test uses (n^2 words per instance). */
int cadnip_jacobian_dense(CadnipHandle* h, const double* gamma_host, double* J_dense_host);
/* ODE-form callbacks (mass matrix C constant; used by the reference with FBDF / QNDF / Rodas):
 *   cadnip_ode_rhs      == rhs!(du, u, p, t):  restamp at (u, t), du = b - G u      src/mna/solve.jl:2241-2248
 *   cadnip_ode_jacobian == jac!(J, u, p, t):   restamp at (u, t), J = -G            src/mna/solve.jl:2251-2276
 * J comes back in the reference's CSC nzval order (jac_prototype = -cs.G, solve.jl:2285); the mass matrix is
 * cadnip_get_GCb's C.  u_host NULL = reuse the stamps of the last rebuild. */
int cadnip_ode_rhs(CadnipHandle* h, const double* u_host, const double* t_host, double* du_host);
int cadnip_ode_jacobian(CadnipHandle* h, const double* u_host, const double* t_host, double* J_ref_nz_host);
/* operating-point read-out: the per-device contributions of one restamp at the handle's current u / t,
 * [B][ns_g + ns_c + ns_b] in CadnipStructure's slot layout (G slots, then C, then b; slot (k, dev) of a block at
 * base + k * count + dev).  Terminal currents and small-signal variables are sums over them (context.jl:1200-1342). */
int cadnip_get_contributions(CadnipHandle* h, double* slots_host);
/* parity / debug read-back in the reference's CSC nzval order (any pointer may be NULL) */
int cadnip_get_GCb(CadnipHandle* h, double* G_ref_nz, double* C_ref_nz, double* b, double* limit_w);

/* ---- sparse LU == KLU at src/sweeps.jl:600 (IDA linear_solver=:KLU) and
 * src/mna/solve.jl:612-613,667-670 (LinearSolve KLUFactorization, symbolic reused) ----------
 * cadnip_analyze: host symbolic phase, once: threshold-Markowitz pivot order chosen on the
 *   current J of instance `sample_instance`, symbolic fill, level schedules.
 * cadnip_factor : numeric refactor of J for every instance on the GPU with the static pivot
 *   order; returns CADNIP_SINGULAR if any instance hit a bad pivot (flags via cadnip_get_flags).
 * cadnip_solve  : x = J^-1 rhs per instance. */
int cadnip_analyze(CadnipHandle* h, int32_t sample_instance);
/* same, on caller-supplied sample values (CSR order of CadnipStructure.colidx), e.g. the element-wise
 * max |J| over several operating points so that the static pivot order suits all of them */
int cadnip_analyze_values(CadnipHandle* h, const double* J_csr_host);
int cadnip_factor(CadnipHandle* h);
int cadnip_solve(CadnipHandle* h, const double* rhs_host, double* x_host);

/* The per-op refactor + solve of the drivers (x = (G + gamma C)^-1 rhs on the G / C of the last cadnip_rebuild) with a chosen kernel:
 * plain launches, for testing every kernel of that step.  gamma [B], rhs [B][n]; x [B][n] holds the initial contents on entry (what an
 * inactive instance returns) and the solutions on return; active [B] may be NULL (all active) and is reset to all ones before returning;
 * flags [B] receives the per-instance flags (bit 0: zero / non-finite pivot or non-finite solution).  A forced kernel that does not apply
 * to this circuit (no program, tables beyond LDS) returns CADNIP_BADARG and launches nothing.  info [6]: kernel run, waves per workgroup,
 * waves per instance, dense core size nc, and the steps (k_lu_steps, k_lu_f2s) or passes (k_lu_f2_mw, k_lu_f2) before and after the core
 * (zeros for k_lu). */
enum {
  CADNIP_LUK_AUTO = 0,     /* the drivers' choice (csrc/lu_f2.hip: launch_factor_solve_f2), CADNIP_LU_* environment switches included */
  CADNIP_LUK_STEPS4 = 1,   /* k_lu_steps<4>: straight-line steps, four waves per instance */
  CADNIP_LUK_F2MW = 2,     /* k_lu_f2_mw<4>: the pass program, four waves per instance */
  CADNIP_LUK_F2S = 3,      /* k_lu_f2s<W>: straight-line steps, one wave per instance, W instances per workgroup */
  CADNIP_LUK_F2 = 4,       /* k_lu_f2<W>: the pass program, one wave per instance */
  CADNIP_LUK_PLAIN = 5     /* k_lu, fused Jacobian: level by level on the LU program */
};
int cadnip_factor_solve(CadnipHandle* h, const double* gamma_host, const double* rhs_host, const int32_t* active_host, int32_t kernel,
                        double* x_host, int32_t* flags_host, int32_t* info);

/* One Newton iteration of the DAE form in one call -- what a host integrator that keeps the nonlinear loop to itself (IDA behind the Julia
 * shim: residual!, then jacobian! + klu_refactor when it decides on a set-up, then klu_solve; src/mna/precompile.jl:546-585,
 * src/mna/solve.jl:2138-2160, src/sweeps.jl:600) otherwise does with five entry points and five synchronisations:
 *   resid = C du + G u - b at (u, t)          [cadnip_rebuild, cadnip_residual]
 *   refresh != 0: J = G + gamma C, refactored  [cadnip_jacobian, cadnip_factor]; 0: the factors of the last refreshing call are used
 *   delta = J^-1 resid                         [cadnip_solve]
 * with the same kernels in the same order (the results are the same doubles as the five calls'), one staged upload, one staged download,
 * one synchronisation; the launch sequence is an instantiated HIP graph, replayed while the handle's configuration stays as it is.
 * u, du, delta, resid: [B][n]; gamma, t, resid_norm: [B].  t_host NULL = times unchanged; gamma_host may be NULL when refresh == 0;
 * resid_norm_host (||resid||_2 per instance) and resid_host are optional.  CADNIP_NONFINITE / CADNIP_SINGULAR as the separate calls. */
int cadnip_newton_step(CadnipHandle* h, const double* u_host, const double* du_host, const double* gamma_host, const double* t_host, int32_t refresh,
                       double* delta_host, double* resid_norm_host, double* resid_host);
/* The same iteration in ONE kernel (the fused team kernel, csrc/fused_team_kernel.hpp): stamping, residual, refactorisation or kept factors,
 * solve.  Same arguments; the results agree with cadnip_newton_step to rounding (the devices add into an LDS-resident work array in
 * another order), not bit for bit.  CADNIP_BADARG for circuits the team kernel does not run (device types outside linear elements /
 * sources / plain sp_mos1, tables beyond LDS, external generated models, homotopy in force): use cadnip_newton_step there.  The stamps use
 * the transient device mode (a DAE residual is a transient's). */
int cadnip_newton_step_fused(CadnipHandle* h, const double* u_host, const double* du_host, const double* gamma_host, const double* t_host, int32_t refresh,
                             double* delta_host, double* resid_norm_host, double* resid_host);
int cadnip_lu_stats(CadnipHandle* h, int32_t* nnz_lu, int32_t* n_terms, int32_t* n_levels, int32_t* n_fwd_levels, int32_t* n_bwd_levels);
/* the handle's current pivot order: pivot k uses original row rperm[k] and column cperm[k] ([n] each); CADNIP_NOTREADY before an analysis */
int cadnip_lu_order(CadnipHandle* h, int32_t* rperm, int32_t* cperm);

/* ---- AC sweep == the frequency loop of ac!, src/ac.jl:113-170 (there: one dense (G + jw C) \ b_ac per frequency) -----------------
 * x[b][f] = (G[b] + gmin on the voltage-node diagonals + j omega[f] C[b])^-1 b_ac[b] on the G / C of the last cadnip_rebuild and the handle's
 * current pivot order: B * n_freq independent complex sparse systems, one wave each (csrc/ac_lu.hip), factorisation, solve, one step of
 * iterative refinement and the componentwise backward error berr = max_i |b - A x|_i / (|A| |x| + |b|)_i of the returned x.
 * gmin of a node whose diagonal is not in the pattern enters the residuals (refinement, berr) and not the factors.
 * Complex values are interleaved (re, im) doubles.  flags bit 0: zero / non-finite pivot or non-finite solution of that system (reported,
 * never raised: the call still returns CADNIP_OK).  wpb: systems per workgroup, 0 = the launch plan's choice, else 1, 2, 4 or 8.
 * info: W that ran, LDS bytes of a workgroup, systems, workgroups.  CADNIP_BADARG -- and nothing launched -- without an analysis, with
 * n_freq <= 0, an invalid wpb, or when the work arrays of W systems, 16 (nnz(L+U) + 3 n) bytes each, exceed the 160 KB of LDS.  Large
 * sweeps run in chunks of at most 64 MiB of solution, so the handle's output buffers stay bounded. */
int cadnip_ac_solve(CadnipHandle* h, int32_t n_freq, const double* omega /* [F] */, double gmin, const double* bac_host /* [B][n][2] */,
                    int32_t wpb, double* x_host /* [B][F][n][2] */, double* berr_host /* [B][F] */, int32_t* flags_host /* [B][F] */,
                    int32_t* info /* [4] */);
/* The adjoint sweep of noise!, src/noise.jl:150-188 (there: one dense transpose(G + jw C) \ e_out per frequency): x[b][f] solves
 * A^T x = c[b] with the same A, pivot order and factors as cadnip_ac_solve -- the triangular solves and the residual run over columns
 * (csrc/lu_transpose.hpp) -- with one refinement step and berr = max_j |c - A^T x|_j / (|A^T| |x| + |c|)_j.  Returned are the n_pairs probe
 * differences h[b][f][k] = x[p_k] - x[n_k] (pairs[k] = {p_k, n_k}; -1 = ground, which contributes 0) and, with x_host non-NULL, x itself.
 * flags, wpb, info and the chunking (here 16 (n_pairs + n [x wanted]) bytes of device output per system) as cadnip_ac_solve.
 * CADNIP_BADARG -- and nothing launched -- also with n_pairs < 1 or a pair index outside [-1, n). */
int cadnip_ac_adjoint(CadnipHandle* h, int32_t n_freq, const double* omega /* [F] */, double gmin, const double* c_host /* [B][n][2] */,
                      int32_t n_pairs, const int32_t* pairs /* [K][2], -1 = ground */, int32_t wpb, double* h_host /* [B][F][K][2] */,
                      double* x_host /* [B][F][n][2] or NULL */, double* berr_host /* [B][F] */, int32_t* flags_host /* [B][F] */,
                      int32_t* info /* [4] */);
/* Many right-hand sides per factorisation (the columns of a network's Y matrix, the responses to several sources; SPICE's .net / .tf):
 * x[b][f][k] = A^-1 b[b][k] for the n_rhs columns of instance b, with the same A, pivot order and factors as cadnip_ac_solve.  Each of the
 * B * n_freq systems is factored ONCE by its wave (csrc/ac_lu.hip: k_ac_lu_multi); the solve, the refinement step and the backward error then
 * run per column, statement for statement as in cadnip_ac_solve: column k is bit-identical to that call with b[.][k] as its bac_host.
 * Returned per (b, f, k): the n_pairs probe differences h = x[p_j] - x[n_j] (pairs as cadnip_ac_adjoint; n_pairs may be 0), x itself with
 * x_host non-NULL, berr, and flags -- bit 0: a zero / non-finite pivot of system (b, f), set in all its columns, or a non-finite solution of
 * that column.  wpb, info, cadnip_ac_set_memory and cadnip_ac_plan_info as cadnip_ac_solve; chunks of at most 64 MiB of device output,
 * 16 n_rhs (n_pairs + n [x wanted]) bytes per system (a single system beyond that runs as a chunk of one).  CADNIP_BADARG -- and nothing
 * launched -- also with n_rhs < 1, n_pairs < 0, n_pairs == 0 without x_host (nothing to return) or a pair index outside [-1, n). */
int cadnip_ac_solve_multi(CadnipHandle* h, int32_t n_freq, const double* omega /* [F] */, double gmin, int32_t n_rhs,
                          const double* b_host /* [B][K][n][2] */, int32_t n_pairs, const int32_t* pairs /* [n_pairs][2], -1 = ground */,
                          int32_t wpb, double* h_host /* [B][F][K][n_pairs][2] */, double* x_host /* [B][F][K][n][2] or NULL */,
                          double* berr_host /* [B][F][K] */, int32_t* flags_host /* [B][F][K] */, int32_t* info /* [4] */);
/* Many adjoint right-hand sides per factorisation (the noise of several outputs, the noise correlation matrix of an N-port; SPICE's .net with
 * .noise): x[b][f][k] solves A^T x = c[b][k] for the n_rhs columns of instance b, with the same A, pivot order and factors as cadnip_ac_adjoint.
 * Each of the B * n_freq systems is factored ONCE by its wave (csrc/ac_lu.hip: k_ac_adj_multi); the transposed solve, the refinement step and
 * the backward error then run per column in the very statements of cadnip_ac_adjoint: column k is bit-identical to that call with c[.][k] as
 * its c_host -- h, x, berr and the flag, in LDS and in device memory, for every wpb.  Everything else -- what is returned per (b, f, k), the
 * flags (a bad pivot of a system flags all its columns), wpb, info, cadnip_ac_set_memory, cadnip_ac_plan_info, the chunks of at most 64 MiB of
 * device output with 16 n_rhs (n_pairs + n [x wanted]) bytes per system, and every CADNIP_BADARG -- exactly as cadnip_ac_solve_multi. */
int cadnip_ac_adjoint_multi(CadnipHandle* h, int32_t n_freq, const double* omega /* [F] */, double gmin, int32_t n_rhs,
                            const double* c_host /* [B][K][n][2] */, int32_t n_pairs, const int32_t* pairs /* [n_pairs][2], -1 = ground */,
                            int32_t wpb, double* h_host /* [B][F][K][n_pairs][2] */, double* x_host /* [B][F][K][n][2] or NULL */,
                            double* berr_host /* [B][F][K] */, int32_t* flags_host /* [B][F][K] */, int32_t* info /* [4] */);
/* AC sensitivities (SPICE's .SENS on an AC sweep; the gradient of a sizing or yield loop): per system (b, f) -- b an index into the list
 * `base` of n_base instances, NOT every instance of the handle -- the response y = x[p] - x[n] of A x = bac[b] (pair = {p, n}; -1 = ground)
 * and its derivatives with respect to n_par parameters from ONE factorisation (csrc/ac_lu.hip: k_ac_sens):
 *   s[b][f][k] = lambda^T (db[b][k] - (dG + j omega[f] dC) x),   A^T lambda = c,
 * with dG = (G[plus[b][k]] - G[minus[b][k]]) scale[b][k] and dC likewise: the derivatives of G and C are differences of the stamps of
 * perturbed instances that sit in the same handle (their G / C of the last cadnip_rebuild), taken entry by entry on the device; gmin
 * cancels in them.  For a central difference p_k +- delta: scale = 1 / (2 delta), db = (b_ac(p_k + delta) - b_ac(p_k - delta)) / (2 delta);
 * db_host NULL means zeros.  c is one [n] column for all systems, e_p - e_n for the derivative of y.  A, the pivot order, the factors, the
 * solves, the refinement steps and the backward errors are those of cadnip_ac_solve and cadnip_ac_adjoint: x (hence y) and lambda are
 * bit-identical to those calls on instance base[b].  berr: {forward, adjoint}.  flags, one word per (b, f, k): bit 0 a zero / non-finite
 * pivot or a non-finite x or lambda of system (b, f), set in all its columns; bit 1 a non-finite s[b][f][k].  With x_host non-NULL x and
 * lambda come back as well.  wpb, info, cadnip_ac_set_memory and cadnip_ac_plan_info as cadnip_ac_solve, except that a system keeps a
 * fourth n-vector: 16 (nnz(L+U) + 4 n) bytes, in LDS and in a wave's workspace.  Chunks of at most 64 MiB of device output,
 * 16 (1 + n_par + 2 n [x wanted]) bytes per system.  CADNIP_BADARG -- nothing launched, nothing written, no plan recorded -- without an
 * analysis, with n_freq <= 0, n_base < 1, n_par < 1, an instance index outside [0, B), a pair index outside [-1, n), p == n == -1, an
 * invalid wpb, or when the memory setting refuses the work arrays. */
int cadnip_ac_sens(CadnipHandle* h, int32_t n_freq, const double* omega /* [F] */, double gmin, int32_t n_base, const int32_t* base /* [NB] */,
                   int32_t n_par, const int32_t* plus /* [NB][K] */, const int32_t* minus /* [NB][K] */, const double* scale /* [NB][K] */,
                   const double* bac_host /* [NB][n][2] */, const double* db_host /* [NB][K][n][2] or NULL */, const double* c_host /* [n][2] */,
                   const int32_t* pair /* [2], -1 = ground */, int32_t wpb, double* y_host /* [NB][F][2] */, double* s_host /* [NB][F][K][2] */,
                   double* x_host /* [NB][F][2][n][2]: x, lambda; or NULL */, double* berr_host /* [NB][F][2] */,
                   int32_t* flags_host /* [NB][F][K] */, int32_t* info /* [4] */);
/* Pole-zero analysis: shift-invert Arnoldi on the descriptor system (E, A) = (C, -G) of an AC solution.  Per system (b, s) -- instance b, shift
 * j omega[s] on the imaginary axis -- with A = G[b] + gmin + j omega[s] C[b], the matrix, pivot order and factors of cadnip_ac_solve, the wave
 * (csrc/ac_lu.hip: k_ac_arnoldi) builds an orthonormal basis of the Krylov space of K = A^-1 C started at r = A^-1 b[b]:
 *   beta = ||r||_2, v_0 = r / beta;   for j = 0 .. m-1:  w = A^-1 (C v_j), two passes of modified Gram-Schmidt against v_0 .. v_j with
 *   H[i][j] the sum of the two coefficients <v_i, w> (v_i conjugated), H[j+1][j] = ||w||_2 after them, v_{j+1} = w / H[j+1][j].
 * So C V_m = A V_{m+1} H, the eigenvalues theta of H[:m_eff][:m_eff] give the poles p = j omega[s] - 1 / theta nearest the shift, and with
 * l[j][p] = v_j[p_p] - v_j[n_p] (unconjugated; pairs as cadnip_ac_adjoint, n_pairs may be 0) the transfer function to probe p is
 * l^T (I + (s - j omega[s]) H)^-1 beta e_1.  Every one of the m_eff + 1 columns is the column of cadnip_ac_solve -- solve, one refinement step,
 * backward error -- and r is bit-identical to that call's x for (b, omega[s]).  Breakdown: when the norm after the two passes is at most
 * breakdown_tol times the norm before them (or that norm is 0) at step j, the space has closed: m_eff = j + 1, H[j+1][j] = 0 and the system
 * is finished; otherwise m_eff = m.  Layouts: H (m+1) x m, row-major, zero beyond m_eff; l m x n_pairs, zero beyond m_eff; V (with v_host
 * non-NULL) (m+1) x n, rows that hold no vector zero; berr the worst backward error of the system's columns (a NaN stays).  flags: bit 0 a
 * zero / non-finite pivot or a non-finite word of H, beta or l; bit 1 beta zero or non-finite (m_eff = 0, no step made); bit 2 breakdown --
 * informational, not an error.  Flags, never traps: the call returns CADNIP_OK.  Dot products and norms are per-lane sums in index order and
 * a fixed butterfly: every output is bit-identical for wpb 1 / 2 / 4 / 8 and between LDS and device memory.  wpb, info, cadnip_ac_set_memory
 * and cadnip_ac_plan_info as cadnip_ac_sens (four n-vectors: 16 (nnz(L+U) + 4 n) bytes per system); the basis lives in device memory in both
 * homes.  Chunks of at most 64 MiB of device output, 16 ((m+1) m + m n_pairs + (m+1) n) bytes per system, the basis counted whether asked for or
 * not (a single system beyond that runs as a chunk of one).  CADNIP_BADARG -- nothing launched, nothing written, no plan recorded -- without
 * an analysis, with n_shift <= 0, m < 1, m > n, breakdown_tol outside (0, 1), n_pairs < 0, a pair index outside [-1, n), an invalid wpb, or
 * when the memory setting refuses the work arrays. */
int cadnip_ac_arnoldi(CadnipHandle* h, int32_t n_shift, const double* omega /* [S] */, double gmin, const double* b_host /* [B][n][2] */, int32_t m,
                      double breakdown_tol, int32_t n_pairs, const int32_t* pairs /* [n_pairs][2], -1 = ground */, int32_t wpb,
                      double* H_host /* [B][S][m+1][m][2] */, double* beta_host /* [B][S] */, int32_t* meff_host /* [B][S] */,
                      double* l_host /* [B][S][m][n_pairs][2]; NULL with n_pairs = 0 */, double* v_host /* [B][S][m+1][n][2] or NULL */,
                      double* berr_host /* [B][S] */, int32_t* flags_host /* [B][S] */, int32_t* info /* [4] */);

/* Where the AC and adjoint sweeps keep a system's work arrays -- a handle setting, LDS by default: every call exactly as without it.
 *   CADNIP_AC_LDS   in LDS (k_ac_lu / k_ac_adj): one wave per system, refused beyond 160 KB as described above,
 *   CADNIP_AC_HBM   in a workspace in device memory (k_ac_lu_hbm / k_ac_adj_hbm): the same arithmetic -- bit-identical results where both
 *                   apply -- by persistent waves; wave g of n_waves handles systems g, g + n_waves, ... of a launch in its one workspace
 *                   of 16 (nnz(L+U) + 3 n) bytes, so the handle's footprint is bounded (csrc/ac_hbm_plan.hpp: n_waves = min(systems,
 *                   compute units x k), k the largest of 8, 4, 2, 1 that keeps the workspace within 256 MiB),
 *   CADNIP_AC_AUTO  LDS when its launch plan accepts the circuit (and the wpb asked for), else HBM.
 * max_waves > 0 replaces compute units x k; 0: the plan's choice.  Under HBM, wpb is waves per workgroup (0: 4), info[1] (LDS bytes) is 0 and
 * info[3] the workgroups launched; a system whose own workspace exceeds 256 MiB is CADNIP_BADARG.  An unknown mode or max_waves < 0 is
 * CADNIP_BADARG and leaves the setting as it was. */
#define CADNIP_AC_LDS 0
#define CADNIP_AC_HBM 1
#define CADNIP_AC_AUTO 2
int cadnip_ac_set_memory(CadnipHandle* h, int32_t mode, int32_t max_waves);
/* A sparse complex addend per system on the A of the AC sweeps -- a handle setting, none by default: every call exactly as without it.
 * While it is set, system (b, f) of cadnip_ac_solve, cadnip_ac_adjoint, cadnip_ac_solve_multi and cadnip_ac_adjoint_multi is
 *   A = G[b] + gmin on the voltage-node diagonals + j omega[f] C[b] + D[b][f],
 * D non-zero at the n_ovl CSR positions pos[] (distinct, in [0, nnz), in the order of the structure's rowptr / colidx; the same for the
 * whole batch) with the values val[b][f][o] (interleaved re, im).  This is how an element that is neither a G nor a C enters an AC
 * analysis: a transport delay tau on a stamp w is the addend (e^{-j omega tau} - 1) w.  The caller computes the values; the kernels
 * (csrc/ac_lu.hip: k_ac_lu_ovl, k_ac_adj_ovl, k_ac_lu_multi_ovl, k_ac_adj_multi_ovl and their _hbm forms) add them wherever A is formed --
 * in the load, in both residuals and in the |A| of the backward error -- so factors, refinement and berr belong to one matrix, and the
 * results stay bit-identical for wpb 1 / 2 / 4 / 8, between LDS and device memory, and between the multi calls' columns and the
 * single-column calls.  The setting names its grid: while it is set, the four calls require their own n_freq / omega to equal the
 * setting's bit for bit (CADNIP_BADARG otherwise, nothing launched), so a table is never applied to other frequencies; cadnip_ac_sens and
 * cadnip_ac_arnoldi are CADNIP_BADARG while it is set (A is then not a (G, C) pencil).  A non-finite value is not an argument error: it
 * surfaces as flag bit 0 of its own system.  The values are copied to the device: the arrays may be released after the call.
 * n_ovl = 0 clears the setting (the other arguments are not read).  CADNIP_BADARG -- the previous setting stays in force -- with
 * n_ovl < 0, a position outside [0, nnz) or named twice, n_freq <= 0, or a table (16 B n_freq n_ovl bytes) beyond 256 MiB. */
int cadnip_ac_set_overlay(CadnipHandle* h, int32_t n_ovl, const int32_t* pos /* [n_ovl] */, int32_t n_freq, const double* omega /* [F] */,
                          const double* val /* [B][F][n_ovl][2] */);
/* of the last cadnip_ac_solve / cadnip_ac_adjoint call that launched: the memory used (CADNIP_AC_LDS / CADNIP_AC_HBM), n_waves and work_bytes of
 * its largest launch (0 under LDS), LDS bytes of a workgroup (0 under HBM) */
int cadnip_ac_plan_info(CadnipHandle* h, int64_t out[4]);

/* ---- host drivers (Newton loop + step controller; stand-in for IDA / _dc_pcnr_newton) ----
 * The loops run on the host and launch the kernels above on the handle's stream; the
 * per-instance convergence / step decisions are evaluated on the device (one lane-group
 * per instance) so that B desynchronised instances need no per-iteration PCIe traffic. */
/* CadnipDCOpts::cold_start = CADNIP_DC_COLD_ZERO: a cold start from the all-zero state whose start point is made on the device -- u_host is
 * output only, nothing of it is read or uploaded.  Honoured when `participate` is NULL; with a mask it means 1 and u_host is read as ever,
 * because masked rows must come back untouched. */
#define CADNIP_DC_COLD_ZERO 2
typedef struct {
  double abstol;          /* ||G u - b||_2 < abstol      solve.jl:640 (1e-10 dc!, 1e-9 CedarTranOp) */
  int32_t maxiters;       /* solve.jl:600 */
  int32_t use_pcnr;       /* PCNR corrector u[lim] = limit_w  solve.jl:682-688 */
  int32_t cold_start;     /* non-zero: seed limit vars + initjct  solve.jl:615-625; CADNIP_DC_COLD_ZERO: that, from zeros made on the device */
  int32_t use_stepping;   /* gshunt / source stepping fallbacks solve.jl:909-925 */
  int32_t fused;          /* non-zero: the first attempt (PCNR / Newton at the handle's spec) runs in the fused kernel
                             (csrc/fused2.hip, DC mode); the fallback homotopies always use the per-op kernels */
  const int32_t* participate; /* [B] or NULL (= everyone): instances with 0 sit the run out -- their u is left as it is and they
                             report converged = 0.  dc!(cs) continuation solves a sweep in stages (sweeps.jl:511-532): the
                             points of a stage start from converged neighbours of the earlier stages */
} CadnipDCOpts;

typedef struct {
  double t0, t1;
  double reltol;
  const double* abstol;     /* [n] per-unknown absolute tolerance (state_abstol, build.jl:276-283) */
  const double* err_mask;   /* [n] 1 = unknown takes part in the local-error test, 0 = excluded; NULL = all.
                               The driver's default excludes algebraic unknowns (V-source currents jump at
                               source breakpoints), i.e. it tests the differential unknowns -- the columns of C
                               (cf. detect_differential_vars, solve.jl:2041-2058, and IDA's suppressalg) */
  double h0;                /* initial step (<=0: automatic) */
  double hmin, hmax;        /* hmax <= 0: (t1-t0)/50 */
  int32_t max_newton;       /* IDA max_nonlinear_iters = 10, sweeps.jl:600 */
  int32_t max_order;        /* 1 = backward Euler only, 2 = variable-step BDF2 (default), 3 = variable-step BDF3 where four accepted points exist
                             * (the reference's IDA goes to 5, src/sweeps.jl:600; orders restart at 1 on every source breakpoint) */
  int32_t use_pcnr;         /* apply the PCNR corrector inside transient Newton */
  double newton_tol;        /* weighted-RMS norm of the Newton update that counts as converged */
  int32_t n_break; const double* breaks; /* sorted tstops from source breakpoints (solve.jl:1847-1960) */
  int32_t n_save;  const double* save_t; /* sorted output times (saveat) */
  int32_t n_obs;   const int32_t* obs;   /* unknown indices to record; n_obs = 0 -> all n */
  int64_t max_iterations;   /* safety bound on lock-step Newton launches */
  int32_t fused;            /* non-zero = fused per-instance Newton kernel, 0 = one kernel per op.  The fused kernel is chosen by batch size: one wave per
                               instance for sweeps (csrc/fused2_kernel.hpp), a team of four waves per instance for batches of at most one instance per
                               compute unit (csrc/fused_team_kernel.hpp: a single transient's latency).  A circuit the fused kernel cannot run -- too
                               large for LDS, an external generated model, or newton_mode 1 with device types outside its lean set (diodes, behavioural
                               sources, sp_mos1 with series resistances, built-in Verilog-A modules) -- runs on the per-op kernels instead, and so does
                               every run of a handle with a delay spec (cadnip_tran_set_delay) */
  int32_t newton_mode;      /* 0 = full Newton, converged when the weighted update norm < newton_tol (every round restamps and refactors);
                               1 = the nonlinear iteration as IDA runs it (the reference's integrator, src/sweeps.jl:600): refactor on a setup
                               only (first round, a0 outside [0.6, 1/0.6] of its last setup value, 20 steps, failure on a stale Jacobian), kept factors in between, rate-based
                               convergence test ss ||delta|| <= 0.33.  The fused kernel keeps the factors; the per-op kernels refactor every round (their
                               factors live in LDS for one launch) and take the convergence test only */
  int32_t step_rule;        /* step size after the error test.  0 = the classical controller: factor 0.9 err^(-1/(k+1)) in [0.2, 2] after an accepted step, in
                               [0.1, 0.9] after a rejected one.  1 = IDA's rule (ida.c: IDACompleteStep / IDASetEta, the reference's integrator, src/sweeps.jl:600):
                               eta = 1 / ((2 err)^(1/(k+1)) + 1e-4); the step DOUBLES when eta >= 2, shrinks by max(0.5, min(0.9, eta)) when eta <= 1 and
                               otherwise STAYS (fewer rejected steps, and a constant step keeps the kept factors of newton_mode 1 valid); after a failed
                               error test the factor is 0.9 eta in [0.25, 0.9] */
} CadnipTranOpts;

typedef struct {
  int64_t newton_iters;     /* == sol.stats.nnonliniter summed over instances */
  int64_t steps_accepted, steps_rejected, newton_failures;
  int64_t launches;         /* lock-step Newton launches */
  int32_t n_failed;         /* instances that did not reach t1 / did not converge */
  double  wall_seconds;     /* host wall clock of the driver loop (device-synchronised) */
} CadnipRunStats;

/* u_host [B][n]: in = initial guess (zeros = cold start), out = solution; converged_host [B] */
/* What the fallback chain of the last cadnip_dc_run did: one entry per (instance, Newton run) in execution order.
 * stage 0 = PCNR (or plain Newton when use_pcnr is off), 1 = plain Newton, 2 = gshunt stepping (value = the rung's gshunt),
 * 3 = source stepping (value = srcFact); ok = the run converged; iters = its Newton solves.  Arrays of cadnip_dc_log_size
 * entries; any pointer may be NULL.  (The reference reports the same through @debug lines, solve.jl:887-927.) */
int32_t cadnip_dc_log_size(CadnipHandle* h);
int cadnip_dc_log_get(CadnipHandle* h, int32_t* inst, int32_t* stage, double* value, int32_t* ok, int64_t* iters);
int cadnip_dc_run(CadnipHandle* h, const CadnipDCOpts* o, double* u_host, int32_t* converged_host, CadnipRunStats* st);
/* Transport delays in the transient -- a handle setting, none by default: the time-domain sibling of cadnip_ac_set_overlay.  A term t is
 * a delayed stamp: its own contribution w[b][t] to G at the CSR position pos[term_pos[t]] = (term_row[t], term_col[t]) multiplies not
 * u[col] at the trial time tn but u[col](tn - tau[b][t]).  While a spec is set, every Newton round of cadnip_tran_run solves
 *   G_tran = G - W,   W[pos] = sum of w over the terms at pos;     b_tran[row] = b[row] - sum over the row's terms of w ud(col, tn - tau)
 * (csrc/delay.hip: k_delay_apply between the restamp and the residual; csrc/delay_plan.hpp holds the look-up).  ud(col, tq) is the start
 * state of the run for tq <= t0, else the LINEAR interpolant of the two accepted points that bracket tq, read from a ring of `depth`
 * accepted points per instance in device memory (k_delay_record appends one per accepted step); a tq at or beyond the newest point takes
 * the newest value.  The run clamps h0 and hmax to the smallest tau of the batch, so tq never falls inside the step in flight.  A tq later
 * than t0 but older than the oldest point kept is not extrapolated: that instance stops with status CADNIP_TRAN_DELAY_OVERFLOW, the
 * others run on.  Such a run uses the per-op kernels whatever CadnipTranOpts::fused says; DC (fused DC included) ignores the spec, as an
 * absdelay without history does.  depth: 0 = 1024.  The arrays are copied: they may be released after the call.
 * spec == NULL or n_term == 0 clears the setting and frees its memory.  CADNIP_BADARG -- the previous setting stays in force -- with an
 * index out of range, a position named twice, a term whose (row, col) is not the coordinate of its position, a tau that is not a
 * positive finite number, depth < 0 or == 1, or a ring beyond 256 MiB (8 B (n_taps + 1) depth bytes; n_taps: the distinct term_col).
 * An instance that ended with CADNIP_TRAN_DELAY_OVERFLOW is ended by k_delay_apply in the middle of a round's launch: its saved outputs,
 * counters and state are those of its last accepted step, but its G and b in device memory (cadnip_get_GCb before the next
 * cadnip_rebuild) may hold a mix of G and G - W, b and b_tran -- other threads of that launch read the status without synchronisation. */
#define CADNIP_TRAN_DELAY_OVERFLOW (-4)
typedef struct {
  int32_t n_pos;  const int32_t* pos;        /* [n_pos] CSR positions in [0, nnz), distinct */
  int32_t n_term; const int32_t* term_pos;   /* [n_term] index into pos[] */
  const int32_t* term_row;                   /* [n_term] row of b that receives the term */
  const int32_t* term_col;                   /* [n_term] unknown whose delayed value it multiplies */
  const double* tau;                         /* [B][n_term] seconds, > 0 */
  const double* w;                           /* [B][n_term] the stamp's own contribution to G */
  int32_t depth;                             /* accepted points kept per instance; 0 = 1024 */
} CadnipDelaySpec;
int cadnip_tran_set_delay(CadnipHandle* h, const CadnipDelaySpec* spec);
/* The plan the handle built from the spec in force -- the sizes k_delay_init / k_delay_apply / k_delay_record index by:
 * out = {n_pos (distinct positions), n_rows (distinct delayed rows of b), n_taps (distinct term_col), n_term, depth}; all zero without a spec */
int cadnip_tran_delay_info(CadnipHandle* h, int32_t out[5]);
/* Parameter sensitivities of the transient, forward (direct, staggered) method -- a handle setting, none by default.  The resident batch is
 * laid out in groups of 2 + 2 K instances: members[g] = {base, twin, p_0 + delta_0, p_0 - delta_0, p_1 + delta_1, ...}.  The caller has given
 * the twin the base's parameters and member 2 + 2 k / 3 + 2 k the base's with parameter k moved by +- delta[g][k] (cadnip_set_params).  Only
 * the bases integrate: cadnip_tran_run parks every other member (status 1, never active in the time loop; its rows of the per-instance
 * arrays are scratch, its rows of out_host / per_inst_host mean nothing) and, after each round's step controller, runs one stage for the
 * groups whose base has just ACCEPTED a step (csrc/tran_sens.hip; arithmetic in csrc/tran_sens_plan.hpp):
 *   (G + a0 C) s_k,n = -(F(p_k + delta_k) - F(p_k - delta_k)) / (2 delta_k) - C sum_{j >= 1} a_j s_k,n-j,    F = C u' + G u - b
 * with G, C restamped on the twin at the accepted point (u_n, t_n), F on the +- members at the same (u_n, u'_n, t_n), a_j the BDF
 * coefficients of the accepted step, and all K systems of all accepting groups solved in one launch of the per-op LU.  One defect pass
 * follows, because G + a0 C need not be the Jacobian of F (a capacitance that depends on u but is stamped into C): the +- members are
 * restamped at (u_n +- delta_k s_k, u'_n +- delta_k s'_k) as well, the difference of their residuals over 2 delta_k -- the total central
 * difference along the trajectory, zero for the exact s_k -- is solved on the same matrix and subtracted.  s_k = du_n/dp_k is
 * the exact derivative of the discrete trajectory on the step sequence the run took (up to the central difference in p); it takes no part
 * in the error test or the step choice, and the bases' states, counters and statuses are bit for bit those of the run without the setting.
 * Save points are interpolated with the weights the states get.  A group whose solve met a bad pivot or a non-finite value gets flag 1
 * and NaN from that step on; its states run on.  Such a run uses the per-op kernels whatever CadnipTranOpts::fused says.
 * nh: history depth, 3, or 4 for runs with max_order >= 3; n_save / n_obs: those of the runs to come (cadnip_tran_run answers
 * CADNIP_BADARG to other values, or to a max_order that does not fit nh, and CADNIP_NOTREADY without a cadnip_tran_sens_init since the
 * last run).  The arrays are copied.  spec == NULL or n_group == 0 clears the setting and frees its memory.  CADNIP_BADARG -- the previous
 * setting stays in force -- with a member index outside [0, B), an instance named twice, a delta that is not a positive finite number, nh
 * other than 3 / 4, n_obs outside [1, n], history plus output beyond 256 MiB (8 n_group K (nh n + n_save n_obs) bytes), or while a delay
 * spec is set; cadnip_tran_set_delay is refused likewise while this setting stands. */
typedef struct {
  int32_t n_group, K;
  const int32_t* members;   /* [n_group][2 + 2 K] instance indices */
  const double* delta;      /* [n_group][K] parameter steps, > 0 */
  int32_t nh, n_save, n_obs;
} CadnipSensSpec;
int cadnip_tran_set_sens(CadnipHandle* h, const CadnipSensSpec* spec);
/* s(t0) of every group, before each cadnip_tran_run.  zero != 0: s = 0 (the start state was given).  Otherwise the handle's current state
 * is an operating point and s = -G^-1 d(G u - b)/dp there, by the same stage with every a_j = 0: call it after the :tranop cadnip_dc_run and
 * before the mode is switched (needs cadnip_analyze*). */
int cadnip_tran_sens_init(CadnipHandle* h, int32_t zero);
/* results of the last run: out_s [n_group][K][n_save][n_obs], flags [n_group] (either may be NULL) */
int cadnip_tran_sens_get(CadnipHandle* h, double* out_s, int32_t* flags);
/* the sizes the kernels index by: out = {n_group, K, members per group, nh, n_save, n_obs}; all zero without a spec */
int cadnip_tran_sens_info(CadnipHandle* h, int32_t out[6]);
/* starts from the handle's current state u (e.g. left by cadnip_dc_run in :tranop mode);
 * out_host [B][n_save][n_obs]; per_inst_host [B][4] = {newton_iters, accepted, rejected, status}; status 1 = reached t1, -1 / -2 = the step
 * fell below hmin after a failed error test / Newton iteration, CADNIP_TRAN_DELAY_OVERFLOW = see cadnip_tran_set_delay */
int cadnip_tran_run(CadnipHandle* h, const CadnipTranOpts* o, double* out_host, int64_t* per_inst_host, CadnipRunStats* st);

/* per-instance integrator state after / during a run: time reached, current step size, order */
int cadnip_tran_state(CadnipHandle* h, double* t_host, double* h_host, int32_t* order_host);

/* ---- misc -------------------------------------------------------------------------------- */
typedef enum { CADNIP_BUF_U = 0, CADNIP_BUF_G = 1, CADNIP_BUF_C = 2, CADNIP_BUF_B = 3, CADNIP_BUF_J = 4,
               CADNIP_BUF_RESID = 5, CADNIP_BUF_SLOTS = 6, CADNIP_BUF_LU = 7, CADNIP_BUF_FLAGS = 8 } CadnipBuffer;
void* cadnip_dev_ptr(CadnipHandle* h, int32_t which);  /* device pointer of a handle-owned buffer */
void* cadnip_stream(CadnipHandle* h);                  /* hipStream_t the handle launches on */
int cadnip_set_u(CadnipHandle* h, const double* u_host);
int cadnip_get_u(CadnipHandle* h, double* u_host);
int cadnip_get_flags(CadnipHandle* h, int32_t* flags_host /* [B] */);
int cadnip_sync(CadnipHandle* h);
/* timing of the kernels launched since the last reset, measured with hipEvents on the handle's
 * stream: names[i] (static strings), ms[i] total, calls[i]; returns number of entries */
int cadnip_profile_enable(CadnipHandle* h, int32_t on);
int cadnip_profile_read(CadnipHandle* h, int32_t max_entries, const char** names, double* ms, int64_t* calls);
const char* cadnip_version(void);
/* PMC calibration aid (MI355X_MICROARCH.md, HBM section: FETCH_SIZE / WRITE_SIZE must be calibrated on a known
 * byte count in the kernel's own access width): streams n_doubles fp64 values src -> dst with 8 B per lane,
 * `reps` times, through a kernel named k_calib_copy_f64.  Known traffic: 8*n_doubles read + 8*n_doubles written per rep. */
/* measurement aid: `reps` back-to-back launches of the stamping kernel of device block `block` (< 0: all blocks = one restamp)
 * at the handle's current u / t, timed with HIP events on the handle's stream */
int cadnip_debug_stamp_time(CadnipHandle* h, int32_t block, int32_t reps, double* ms_total);
/* diagnostic: one Newton iteration of the team kernel (STEP mode) repeated `reps` times at the resident state, phases left out by `skip`
 * (1 stamping, 2 adding the waves' private sums, 4 linear-solve steps, 8 dense core); tools/team_phases.py */
int cadnip_debug_step_time(CadnipHandle* h, int32_t refresh, int32_t reps, int32_t skip, double* ms_total);
int cadnip_debug_copy(CadnipHandle* h, int64_t n_doubles, int32_t reps);

/* ---- host-only helpers (no GPU needed): run the symbolic phase on any CSR matrix and read the
 * resulting program back; used by the CPU test-suite to validate the LU program --------------- */
typedef struct CadnipHostLU CadnipHostLU;
typedef enum { CADNIP_LU_RPERM = 0, CADNIP_LU_CPERM, CADNIP_LU_ROWPTR, CADNIP_LU_COL, CADNIP_LU_DIAG, CADNIP_LU_LOAD_SRC,
               CADNIP_LU_LOAD_DST, CADNIP_LU_ENT_POS, CADNIP_LU_ENT_DIAG, CADNIP_LU_ENT_PTR, CADNIP_LU_TERM_A, CADNIP_LU_TERM_B,
               CADNIP_LU_LEV_PTR, CADNIP_LU_FWD_ROWS, CADNIP_LU_FWD_LEV_PTR, CADNIP_LU_BWD_ROWS, CADNIP_LU_BWD_LEV_PTR,
               CADNIP_LU_NARRAYS } CadnipLUArray;
/* sample != 0: `vals` is a composite magnitude sample (as cadnip_analyze_values takes), not one state's Jacobian: a
 * numerically singular sample is re-analysed on magnitudes instead of being reported (csrc/symbolic.cpp) */
int cadnip_host_lu_analyze(int32_t n, const int32_t* rowptr, const int32_t* colidx, const double* vals, double pivot_tol, int32_t sample, CadnipHostLU** out);
/* ... with the leaf-first pivot order a handle uses (csrc/symbolic.cpp): unknowns [q_begin, lim_begin) are charge states, [lim_begin, n)
 * limit variables (the reference's layout [V | I | q | lim], src/mna/context.jl); unit_ok[i] != 0: the diagonal of unknown i is one
 * constant stamp.  q_begin < 0: plain Markowitz search (as cadnip_host_lu_analyze). */
int cadnip_host_lu_analyze_leaves(int32_t n, const int32_t* rowptr, const int32_t* colidx, const double* vals, double pivot_tol, int32_t sample,
                                  int32_t q_begin, int32_t lim_begin, const uint8_t* unit_ok, CadnipHostLU** out);
int32_t cadnip_host_lu_size(const CadnipHostLU* lu, int32_t which);
int32_t cadnip_host_lu_blocks(const CadnipHostLU* lu);   /* diagonal blocks of the block triangular form when KLU's ordering was used (csrc/klu_order.cpp), 0 = Markowitz search */
int cadnip_host_lu_get(const CadnipHostLU* lu, int32_t which, int32_t* dst);
void cadnip_host_lu_free(CadnipHostLU* lu);
/* The tables of the TRANSPOSED solve through the same factors (csrc/lu_transpose.hpp; the adjoint kernel k_ac_adj follows them): built by
 * this call, then read with cadnip_host_lu_size / _get under the indices below.  COLPTR / POS / ROW / DIAG: the column view of L\U;
 * UT_* / LT_*: the level schedules of U^T z = y (forward) and L^T w = z (backward); A_*: the column view of the CSR pattern. */
typedef enum { CADNIP_LUT_COLPTR = 32, CADNIP_LUT_POS, CADNIP_LUT_ROW, CADNIP_LUT_DIAG, CADNIP_LUT_UT_ROWS, CADNIP_LUT_UT_LEV_PTR,
               CADNIP_LUT_LT_ROWS, CADNIP_LUT_LT_LEV_PTR, CADNIP_LUT_A_COLPTR, CADNIP_LUT_A_ROW, CADNIP_LUT_A_POS } CadnipLUTArray;
int cadnip_host_lu_transpose(CadnipHostLU* lu);

/* The fused kernel's linear-solve program for core size nc (0, 8, 12 or 16; csrc/f2_program.cpp), built from a host LU:
 * arrays POSW (int32: LU pattern position -> work-array offset), LANES / PASSES (uint64 descriptors), TERMS (uint32) and
 * META (int32: nc, lu_words, dn0, n_pre, n_post).  cadnip_host_f2_get copies raw bytes; _size returns the element count. */
typedef struct CadnipHostF2 CadnipHostF2;
typedef enum { CADNIP_F2_POSW = 0, CADNIP_F2_LANES, CADNIP_F2_PASSES, CADNIP_F2_TERMS, CADNIP_F2_META, CADNIP_F2_NARRAYS } CadnipF2Array;
int cadnip_host_f2_build(const CadnipHostLU* lu, int32_t nc, CadnipHostF2** out);
int32_t cadnip_host_f2_size(const CadnipHostF2* prog, int32_t which);
int cadnip_host_f2_get(const CadnipHostF2* prog, int32_t which, void* dst);
int cadnip_host_f2_team_steps(const CadnipHostLU* lu, int32_t nc, int32_t nw, int32_t* out4);   /* steps of the team layout (pre, post, forward-only) and its descriptor words */
/* The same program as straight-line steps (csrc/f2_program.cpp): nw = 1 -- the one-wave layout of the fused sweep kernel (list-scheduled steps of 64
 * lanes, three terms per lane, 16-byte descriptors = two uint64 per lane), nw = 2 / 4 -- the team layouts (8-byte descriptors), nw = 12 / 14 -- the
 * three-term layout for teams of 2 / 4 waves (the per-op step LU).  out4 = steps of the
 * pre-core, post-core and forward-only lists and the number of uint64 words; dst (may be NULL) receives the words. */
int cadnip_host_f2_steps(const CadnipHostLU* lu, int32_t nc, int32_t nw, int32_t* out4, uint64_t* dst);
void cadnip_host_f2_free(CadnipHostF2* prog);

#ifdef __cplusplus
}
#endif
#endif /* CADNIP_HIP_H */
