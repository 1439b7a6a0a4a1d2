// ac_lu.hip -- the AC frequency sweep (src/ac.jl:113-170: x = (G + jw C)^-1 b_ac at the DC point) as a batched complex sparse LU.  The
// B instances x F frequencies of a sweep are S = B F independent systems with ONE pattern and ONE pivot order: one 64-lane wave per system
// (b, f), W systems per workgroup, all synchronisation wave-level (as k_lu_f2, lu_f2.hip).  Per system the complex factors and three complex
// n-vectors live in LDS (lds_layout.hpp: lds_ac); the index tables of the plain LUProgram (symbolic.cpp) are shared by every system and are
// read from global memory -- they stay in L2.  The wave
//   1. loads A = G[b] + gmin [node diagonals] + j w_f C[b] through load_dst (fill positions zeroed first).  A voltage node whose diagonal is
//      not in the pattern (a node that only source and inductor branches touch) has no word for its gmin: the factors leave it out, the
//      residuals of steps 4 and 5 carry it (`nodiag`), so the refinement step corrects for it -- to O((gmin |A^-1|)^2) -- and the backward
//      error is measured against the same A the host path solves,
//   2. factors entry-wise, level by level: lu[pos] = (lu[pos] - sum lu[a] lu[b]) [* 1 / piv].  The reciprocal of a pivot is taken ONCE per
//      row, in place, when the row's diagonal is final (the pivot lists of ac_lu_prepare): nothing reads a diagonal entry but the entries
//      that divide by it, and those sit in later levels.  Constant-1 pivots (LUProgram::unit) take no division: their word is set to 1,
//   3. solves for b_ac[b] (forward, backward),
//   4. refines once: r = b - A x from the G and C arrays in HBM (not from the factors), solve, x += correction,
//   5. recomputes r and the componentwise backward error max_i |r_i| / (|A| |x| + |b|)_i, 0 / 0 = 0 (tests/lu_ref.py with complex moduli),
//   6. stores x (interleaved re, im), berr and the flag (bit 0: zero / non-finite pivot or non-finite solution -- a flag, never a trap).
// Every multiply-add is an explicit fma: the W instantiations compute the same doubles.
// There are TWO kernels, both generic in a system type S (the structs named *Sys below): k_ac<W, S> keeps the work arrays in LDS, and
// k_ac_hbm<W, S> (cadnip_ac_set_memory) runs the same steps -- the same __device__ functions -- with them in a per-wave workspace in global
// memory, for circuits beyond the LDS budget: persistent waves, planned by ac_hbm_plan.hpp.  One launcher, ac_launch, starts either.  A
// system type holds the family's arguments, says whether its layout has a fourth n-vector, and runs one system; the families are
//   AcLuSys (cadnip_ac_solve): the steps above;  AcAdjSys (cadnip_ac_adjoint): A^T x = c with the same factors,
//   AcLuMultiSys (cadnip_ac_solve_multi): steps 1 and 2 once per system and steps 3 to 6 for each of K right-hand sides;  AcAdjMultiSys
//   (cadnip_ac_adjoint_multi): the same for K adjoint right-hand sides,
//   AcSensSys (cadnip_ac_sens): one forward and one adjoint column per system and, from the two solutions, K bilinear forms over the stamps
//   of perturbed instances -- the response and its K parameter derivatives from one factorisation,
//   AcArnoldiSys (cadnip_ac_arnoldi): factor at a shift j w_s and run m Arnoldi steps of A^-1 C there -- m + 1 columns with the same factors,
//   each right-hand side C times the previous solution, kept in the wave: the pole-zero analysis.
// The first four take the overlay as a type parameter: AcLuSys<AcOvl> (cadnip_ac_set_overlay) is AcLuSys<AcNoOvl> with a sparse complex
// addend D[b][f] on A -- delayed stamps, e^{-j w tau} -- added wherever A is formed: steps 1, 4 and 5 (struct AcOvl below).
// The ABI header, DESIGN.md, the tools and the tests call the families k_ac_lu, k_ac_adj, k_ac_lu_multi, k_ac_adj_multi, k_ac_sens and
// k_ac_arnoldi, with _hbm for the form in global memory and _ovl for AcOvl; ac_launch times them under those names ("ac_lu", "ac_lu_hbm", ...).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <vector>
#include "internal.hpp"
#include "tran_ctrl.hpp"
#include "lds_layout.hpp"
#include "lu_transpose.hpp"
#include "ac_hbm_plan.hpp"

namespace cadnip {

struct AcArgs {
  const double *G, *C, *omega, *bac; const unsigned char *diag_flag, *nodiag; double gmin;
  double *x, *berr; int* flags;
  const int *rowptr, *colidx, *load_dst, *ent_pos, *ent_diag, *ent_ptr, *term_a, *term_b, *lev_ptr;
  const int *lu_rowptr, *lu_col, *lu_diag, *rperm, *cperm, *fwd_rows, *fwd_lev_ptr, *bwd_rows, *bwd_lev_ptr;
  const int *piv_rows, *piv_lev_ptr;
  int n, nnz, nnz_lu, n_lev, n_fwd_lev, n_bwd_lev, n_freq, n_sys;
  long s0;
};

// acc - a b
__device__ __forceinline__ double2 cmsub(double2 acc, double2 a, double2 b) {
  return make_double2(fma(-a.x, b.x, fma(a.y, b.y, acc.x)), fma(-a.x, b.y, fma(-a.y, b.x, acc.y)));
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)); }
// 1 / p, scaled by the power of two of max(|re|, |im|): |p|^2 neither overflows nor underflows.  p = 0 / non-finite: the caller has flagged it
__device__ __forceinline__ double2 crecip(double2 p) {
  int e;
  (void)frexp(fmax(fabs(p.x), fabs(p.y)), &e);
  const double a = ldexp(p.x, -e), b = ldexp(p.y, -e);            // max(|a|, |b|) in [0.5, 1)
  const double d = fma(a, a, b * b);
  return make_double2(ldexp(a / d, -e), ldexp(-b / d, -e));
}
__device__ __forceinline__ double cabs2(double2 a) { return hypot(a.x, a.y); }

// The overlay (cadnip_ac_set_overlay): a sparse complex addend D[b][f] on A -- a delayed stamp's e^{-j w tau} is neither a G nor a C.  It is
// non-zero at n CSR positions pos[] shared by the whole batch (distinct; map[nnz] is the inverse, -1 = none), with the values of system
// (b, f) at val + (b n_freq + f) n: indexed by the system's own (inst, fi), so a chunk seam cannot shift it.  The host computes the values;
// the kernels only add them.  The overlay is a compile-time policy of every function that forms an entry of A -- the load, the two
// residuals and, through them, the backward error's |A| -- so the factors, the refinement step and berr belong to ONE matrix.  AcNoOvl is
// empty: the kernels without overlay are the statements they were.  The addend is added component by component to the entry ac_entry
// forms, in the load and in the residuals alike: the same doubles in both, whatever W and wherever the work arrays live.
struct AcNoOvl {
  static constexpr bool on = false;
  __device__ __forceinline__ AcNoOvl at(int, int, int) const { return *this; }
};
struct AcOvl {
  static constexpr bool on = true;
  const int *pos, *map; const double2* val; int n;
  __device__ __forceinline__ AcOvl at(int inst, int fi, int n_freq) const { AcOvl o = *this; o.val = val + ((size_t)inst * n_freq + fi) * n; return o; }
};

// A at CSR position e of instance-local G / C; o: the overlay of the system (AcOvl::at), or none
template <class O = AcNoOvl>
__device__ __forceinline__ double2 ac_entry(const AcArgs& a, const double* G, const double* C, double om, int e, const O& o = O()) {
  double2 v = make_double2(G[e] + (a.diag_flag[e] ? a.gmin : 0.0), om * C[e]);
  if constexpr (O::on) {
    const int k = o.map[e];
    if (k >= 0) { const double2 d = o.val[k]; v = make_double2(v.x + d.x, v.y + d.y); }
  }
  return v;
}

// How the lanes of a wave order their accesses to the work arrays between two steps: a level's lanes read words that OTHER lanes of the wave
// stored in an earlier level.  The steps below are generic in it, so the LDS and the HBM kernels run the same statements on the same doubles.
struct AcInLds {                                               // work arrays in LDS: the wave-scope fence of every LDS-resident kernel
  static __device__ __forceinline__ void sync() { CADNIP_WAVE_SYNC(); }
};
// Work arrays in global memory: the fence the fused kernel uses for words "read back by other lanes of this wave" (fused2_kernel.hpp:
// history_to_memory), then the wave barrier.  Why workgroup scope suffices on gfx950, from the memory model (LLVM AMDGPU: scopes are
// inclusive, gfx942 code sequences): a wave's workspace is written and read by the lanes of that ONE wave and by nobody else -- no other
// wave, no other workgroup, not the host (which reads x / berr / flags after the kernel's end, a system-scope release of its own).  Writer
// and reader therefore always sit in the same workgroup, the smallest named scope that is guaranteed to contain both, and a release-acquire
// fence at that scope orders the accesses of any two threads inside it.  What it costs: the release half waits for the wave's outstanding
// stores (vmcnt(0)) -- they have gone through the compute unit's write-through vector L1 -- before a later load issues; the acquire half
// needs no cache invalidate, because the waves of a workgroup (we never build threadgroup-split code) share that one L1, and a wave
// trivially shares it with itself.  A wider scope would add L1 invalidates / L2 write-backs for readers that do not exist.  For the
// compiler the fence pins every global access to its side and forbids keeping a loaded word in a register across it.
struct AcInHbm {
  static __device__ __forceinline__ void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
};

// Steps 1 and 2 of every kernel -- load A into lu, factor in place -- so that AcLuSys and AcAdjSys hold the same doubles by construction.
// Returns 1 in the lanes that met a zero / non-finite pivot.
template <class M, class O = AcNoOvl>
__device__ __forceinline__ int ac_load_factor(const AcArgs& a, double2* lu, const double* G, const double* C, double om, int lane, const O& o = O()) {
  int bad = 0;
  // ---- 1. load
  for (int p = lane; p < a.nnz_lu; p += 64) lu[p] = make_double2(0.0, 0.0);
  M::sync();
  for (int e = lane; e < a.nnz; e += 64) lu[a.load_dst[e]] = ac_entry(a, G, C, om, e);
  M::sync();
  if constexpr (O::on) {                                       // the overlay's pass: distinct positions, one lane each
    for (int k = lane; k < o.n; k += 64) { double2* w = lu + a.load_dst[o.pos[k]]; const double2 v = *w, d = o.val[k]; *w = make_double2(v.x + d.x, v.y + d.y); }
    M::sync();
  }
  // ---- 2. factor; the pivots of list l are final before level l runs (list 0: after the load)
  auto pivots = [&](int l) {
    const int k1 = a.piv_lev_ptr[l + 1];
    for (int k = a.piv_lev_ptr[l] + lane; k < k1; k += 64) {
      const int i = a.piv_rows[k], dp = a.lu_diag[i < 0 ? ~i : i];
      if (i < 0) { lu[dp] = make_double2(1.0, 0.0); continue; }
      const double2 pv = lu[dp];
      if ((pv.x == 0.0 && pv.y == 0.0) || !isfinite(pv.x) || !isfinite(pv.y)) bad = 1;
      lu[dp] = crecip(pv);
    }
    M::sync();
  };
  pivots(0);
  for (int lev = 0; lev < a.n_lev; ++lev) {
    const int e1 = a.lev_ptr[lev + 1];
    for (int e = a.lev_ptr[lev] + lane; e < e1; e += 64) {
      const int pos = a.ent_pos[e], t1 = a.ent_ptr[e + 1], dg = a.ent_diag[e];
      double2 acc = lu[pos];
      for (int t = a.ent_ptr[e]; t < t1; ++t) acc = cmsub(acc, lu[a.term_a[t]], lu[a.term_b[t]]);
      if (dg >= 0) acc = cmul(acc, lu[dg]);
      lu[pos] = acc;
    }
    M::sync();
    pivots(lev + 1);
  }
  return bad;
}

// The work arrays of one system, in LDS or in the wave's workspace in global memory: region w of `waves` over `base`, in lds_ac's layout or
// -- FOUR: the families that keep a fourth n-vector xf -- in lds_ac_sens's (lds_layout.hpp; size_t offsets).  The one place that picks a layout
struct AcWork { double2 *lu, *x, *r, *y, *xf; };
template <bool FOUR>
__device__ __forceinline__ AcWork ac_work(double* base, int nnz_lu, int n, int w, int waves) {
  if constexpr (FOUR) {
    const LdsAcSens<double*> L = lds_ac_sens(base, nnz_lu, n, w, waves);
    return AcWork{(double2*)L.lu, (double2*)L.x, (double2*)L.r, (double2*)L.y, (double2*)L.xf};
  } else {
    const LdsAc<double*> L = lds_ac(base, nnz_lu, n, w, waves);
    return AcWork{(double2*)L.lu, (double2*)L.x, (double2*)L.r, (double2*)L.y, nullptr};
  }
}

// ---- 3. / 4. y := A^-1 y through the factors (y in pivot-row order on entry, pivot-column order on return)
template <class M>
__device__ __forceinline__ void ac_solve(const AcArgs& a, const double2* lu, double2* y, int lane) {
  for (int lev = 0; lev < a.n_fwd_lev; ++lev) {
    const int r1 = a.fwd_lev_ptr[lev + 1];
    for (int q = a.fwd_lev_ptr[lev] + lane; q < r1; q += 64) {
      const int i = a.fwd_rows[q], p1 = a.lu_diag[i];
      double2 acc = y[i];
      for (int p = a.lu_rowptr[i]; p < p1; ++p) acc = cmsub(acc, lu[p], y[a.lu_col[p]]);
      y[i] = acc;
    }
    M::sync();
  }
  for (int lev = 0; lev < a.n_bwd_lev; ++lev) {
    const int r1 = a.bwd_lev_ptr[lev + 1];
    for (int q = a.bwd_lev_ptr[lev] + lane; q < r1; q += 64) {
      const int i = a.bwd_rows[q], dp = a.lu_diag[i], p1 = a.lu_rowptr[i + 1];
      double2 acc = y[i];
      for (int p = dp + 1; p < p1; ++p) acc = cmsub(acc, lu[p], y[a.lu_col[p]]);
      y[i] = cmul(acc, lu[dp]);                               // the diagonal word holds 1 / pivot
    }
    M::sync();
  }
}

// r = b - A x, one row per lane; with DEN the backward error of the wave's rows is returned
template <class M, bool DEN, class O = AcNoOvl>
__device__ __forceinline__ double ac_residual(const AcArgs& a, const double* G, const double* C, double om, const double2* bac, const double2* x,
                                              double2* r, int lane, const O& o = O()) {
  const double gmin = a.gmin;
  double worst = 0.0;
  for (int i = lane; i < a.n; i += 64) {
    const double2 bi = bac[i];
    double2 acc = bi;
    double den = DEN ? cabs2(bi) : 0.0;
    const int p1 = a.rowptr[i + 1];
    for (int p = a.rowptr[i]; p < p1; ++p) {
      const double2 av = ac_entry(a, G, C, om, p, o), xv = x[a.colidx[p]];
      acc = cmsub(acc, av, xv);
      if (DEN) den = fma(cabs2(av), cabs2(xv), den);
    }
    if (a.nodiag[i]) {                                        // gmin of a node diagonal outside the pattern
      const double2 xv = x[i];
      acc = cmsub(acc, make_double2(gmin, 0.0), xv);
      if (DEN) den = fma(gmin, cabs2(xv), den);
    }
    r[i] = acc;
    if (DEN) {
      const double num = cabs2(acc);
      const double q = num == 0.0 ? 0.0 : num / den;
      worst = (q > worst || q != q) ? q : worst;              // a NaN stays
    }
  }
  M::sync();
  return worst;
}

// the wave's backward error from its lanes' figures: the largest, and a NaN stays a NaN
__device__ __forceinline__ double ac_wave_berr(double worst) {
  int nan = worst != worst;
  if (nan) worst = 0.0;
  for (int off = 32; off >= 1; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off));
  return wave_any(nan) ? __builtin_nan("") : worst;
}
// the two status words of (system, column) ls of the launch: berr of the wave and the flag
__device__ __forceinline__ void ac_store_status(const AcArgs& a, int ls, double worst, int bad, int lane) {
  worst = ac_wave_berr(worst);
  bad = wave_any(bad);
  if (lane == 0) { a.berr[ls] = worst; a.flags[ls] = bad ? 1 : 0; }
}
// ---- 6. the stores of (system, column) lk of the launch from the solution x in the work arrays: x itself when the caller asked for it
// (a.x), the probe differences h[k] = x[p_k] - x[n_k] of the call's pairs (-1: ground, contributes 0; lanes striding over the pairs) and
// the status words.  bad: what the lanes know so far; a non-finite word of x adds to it
__device__ __forceinline__ void ac_store_column(const AcArgs& a, const double2* x, const int* pairs, double* h, int n_pairs, size_t lk, double worst, int bad,
                                                int lane) {
  const int n = a.n;
  double2* xo = a.x ? (double2*)a.x + lk * n : nullptr;
  for (int i = lane; i < n; i += 64) { const double2 v = x[i]; if (!isfinite(v.x) || !isfinite(v.y)) bad = 1; if (xo) xo[i] = v; }
  double2* ho = (double2*)h + lk * n_pairs;
  for (int k = lane; k < n_pairs; k += 64) {
    const int p = pairs[2 * k], q = pairs[2 * k + 1];
    const double2 xp = p >= 0 ? x[p] : make_double2(0.0, 0.0), xn = q >= 0 ? x[q] : make_double2(0.0, 0.0);
    ho[k] = make_double2(xp.x - xn.x, xp.y - xn.y);
  }
  ac_store_status(a, (int)lk, worst, bad, lane);
}

// What a system function derives from its index ls in the launch: system s0 + ls of the grid is (row, fi) -- row the instance, or, MAPPED
// (the sensitivity family), an index into the list `base` of instances -- and with it the G and C of the instance, the frequency and the
// overlay's values of that (instance, frequency)
template <class O>
struct AcSysCtx { int row, inst, fi; const double *G, *C; double om; O o; };
template <bool MAPPED = false, class O = AcNoOvl>
__device__ __forceinline__ AcSysCtx<O> ac_sys_ctx(const AcArgs& a, int ls, const O& ovl = O(), const int* base = nullptr) {
  const long s = a.s0 + ls;
  const int row = (int)(s / a.n_freq), fi = (int)(s - (long)row * a.n_freq), inst = MAPPED ? base[row] : row;
  return AcSysCtx<O>{row, inst, fi, a.G + (size_t)inst * a.nnz, a.C + (size_t)inst * a.nnz, a.omega[fi], ovl.at(inst, fi, a.n_freq)};
}

// Steps 3 to 5 of ONE column: A x = bac through the factors in lu, the refinement step and the backward error of the wave's rows (returned).
// x is left in wk.x, visible to every lane.  Shared by AcLuSys, AcLuMultiSys and AcSensSys: the same statements on the same doubles in the
// same x / r / y.  Every word of x, r and y is written before it is read, so a column leaves nothing to the next one
template <class M, class O = AcNoOvl>
__device__ __forceinline__ double ac_lu_column(const AcArgs& a, const AcWork& wk, const double* G, const double* C, double om, const double2* bac, int lane,
                                               const O& o = O()) {
  const int n = a.n;
  double2 *lu = wk.lu, *x = wk.x, *r = wk.r, *y = wk.y;
  for (int i = lane; i < n; i += 64) y[i] = bac[a.rperm[i]];
  M::sync();
  ac_solve<M>(a, lu, y, lane);
  for (int i = lane; i < n; i += 64) x[a.cperm[i]] = y[i];
  M::sync();
  (void)ac_residual<M, false>(a, G, C, om, bac, x, r, lane, o);
  for (int i = lane; i < n; i += 64) y[i] = r[a.rperm[i]];
  M::sync();
  ac_solve<M>(a, lu, y, lane);
  for (int i = lane; i < n; i += 64) { const int j = a.cperm[i]; const double2 xv = x[j], dv = y[i]; x[j] = make_double2(xv.x + dv.x, xv.y + dv.y); }
  M::sync();
  // ---- 5. backward error
  return ac_residual<M, true>(a, G, C, om, bac, x, r, lane, o);
}

// Steps 1 to 6 for system ls of the launch, by one wave, in the work arrays wk.  Everything a system leaves behind is in wk, and every word of
// wk is written before it is read: lu by step 1, y / x / r by the full-length loops of ac_lu_column -- a wave may run system after system in one wk
template <class M, class O = AcNoOvl>
__device__ __forceinline__ void ac_lu_system(const AcArgs& a, int ls, const AcWork& wk, int lane, const O& ovl = O()) {
  const int n = a.n;
  const AcSysCtx<O> s = ac_sys_ctx(a, ls, ovl);
  const double2* x = wk.x;
  const double2* bac = (const double2*)a.bac + (size_t)s.inst * n;
  int bad = ac_load_factor<M>(a, wk.lu, s.G, s.C, s.om, lane, s.o);
  const double worst = ac_lu_column<M>(a, wk, s.G, s.C, s.om, bac, lane, s.o);
  // ---- 6. store
  double2* xo = (double2*)a.x + (size_t)ls * n;
  for (int i = lane; i < n; i += 64) { const double2 v = x[i]; if (!isfinite(v.x) || !isfinite(v.y)) bad = 1; xo[i] = v; }
  ac_store_status(a, ls, worst, bad, lane);
}

// A system type: the arguments of a family (base(): their AcArgs), `four`: its layout keeps the fourth n-vector, run<M>: one system under
// the memory policy M, and `fenced`: in global memory, run() already ends in the fence the wave's next system needs (k_ac_hbm)
template <class O>
struct AcLuSys {
  AcArgs a; O ovl;
  static constexpr bool four = false, fenced = false;
  __host__ __device__ const AcArgs& base() const { return a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_lu_system<M>(a, ls, wk, lane, ovl); }
};

// ---- the adjoint family: A^T x = c with the same factors (noise.jl:150-188: one adjoint solve per frequency serves every noise source) --------
// Steps 1 and 2 as AcLuSys (ac_load_factor).  Then, through the tables of lu_transpose.hpp (M = A[rperm][:, cperm] = L U, so M^T = U^T L^T and
// the permutations swap roles):
//   3. y[j] = c[cperm[j]];  U^T z = y forward, L^T w = z backward, both a gather per unknown over its COLUMN of L\U, level by level, in place
//      in y;  x[rperm[i]] = w[i].  The diagonal word holds 1 / pivot (1 for constant-1 pivots),
//   4. one refinement step with r = c - A^T x from G and C in HBM over the column view of the CSR pattern; gmin sits on diagonals, so the
//      diag_flag entries and the `nodiag` nodes carry it exactly as in the plain residual,
//   5. the componentwise backward error max_j |r_j| / (|A^T| |x| + |c|)_j, 0 / 0 = 0, a NaN stays,
//   6. stores: h[k] = x[p_k] - x[n_k] for the K probe pairs of the call (-1: ground, contributes 0), lanes striding over K; berr; the flag
//      (bit 0 as AcLuSys); x itself when the caller asked for it.
// Everything is a gather and every multiply-add an explicit fma: no atomics, no workgroup barrier, the W instantiations compute the same doubles.
struct AcAdjArgs {
  AcArgs a;                                 // a.bac: c [B][n]; a.x: x out (null: not wanted); a.berr / a.flags: this kernel's outputs
  const int *t_colptr, *t_pos, *t_row, *t_diag, *ut_rows, *ut_lev_ptr, *lt_rows, *lt_lev_ptr, *a_colptr, *a_row, *a_pos;
  const int* pairs; double* h;
  int n_ut_lev, n_lt_lev, n_pairs;
};

// ---- 3. / 4. y := M^-T y (y in pivot-column order on entry, pivot-row order on return)
template <class M>
__device__ __forceinline__ void ac_adj_solve(const AcAdjArgs& t, const double2* lu, double2* y, int lane) {
  for (int lev = 0; lev < t.n_ut_lev; ++lev) {
    const int r1 = t.ut_lev_ptr[lev + 1];
    for (int q = t.ut_lev_ptr[lev] + lane; q < r1; q += 64) {
      const int j = t.ut_rows[q], p0 = t.t_colptr[j], pd = p0 + t.t_diag[j];
      double2 acc = y[j];
      for (int p = p0; p < pd; ++p) acc = cmsub(acc, lu[t.t_pos[p]], y[t.t_row[p]]);
      y[j] = cmul(acc, lu[t.t_pos[pd]]);                      // the diagonal word holds 1 / pivot
    }
    M::sync();
  }
  for (int lev = 0; lev < t.n_lt_lev; ++lev) {
    const int r1 = t.lt_lev_ptr[lev + 1];
    for (int q = t.lt_lev_ptr[lev] + lane; q < r1; q += 64) {
      const int j = t.lt_rows[q], p1 = t.t_colptr[j + 1];
      double2 acc = y[j];
      for (int p = t.t_colptr[j] + t.t_diag[j] + 1; p < p1; ++p) acc = cmsub(acc, lu[t.t_pos[p]], y[t.t_row[p]]);
      y[j] = acc;
    }
    M::sync();
  }
}

// r = c - A^T x, one column of A per lane; with DEN the backward error of the wave's columns is returned
template <class M, bool DEN, class O = AcNoOvl>
__device__ __forceinline__ double ac_adj_residual(const AcAdjArgs& t, const double* G, const double* C, double om, const double2* c, const double2* x,
                                                  double2* r, int lane, const O& o = O()) {
  const AcArgs& a = t.a;
  const double gmin = a.gmin;
  double worst = 0.0;
  for (int j = lane; j < a.n; j += 64) {
    const double2 cj = c[j];
    double2 acc = cj;
    double den = DEN ? cabs2(cj) : 0.0;
    const int p1 = t.a_colptr[j + 1];
    for (int p = t.a_colptr[j]; p < p1; ++p) {
      const double2 av = ac_entry(a, G, C, om, t.a_pos[p], o), xv = x[t.a_row[p]];
      acc = cmsub(acc, av, xv);
      if (DEN) den = fma(cabs2(av), cabs2(xv), den);
    }
    if (a.nodiag[j]) {                                        // gmin of a node diagonal outside the pattern
      const double2 xv = x[j];
      acc = cmsub(acc, make_double2(gmin, 0.0), xv);
      if (DEN) den = fma(gmin, cabs2(xv), den);
    }
    r[j] = acc;
    if (DEN) {
      const double num = cabs2(acc);
      const double q = num == 0.0 ? 0.0 : num / den;
      worst = (q > worst || q != q) ? q : worst;              // a NaN stays
    }
  }
  M::sync();
  return worst;
}

// Steps 3 to 6 of ONE adjoint column: A^T x = c through the factors in lu, the refinement step, the backward error (ac_adj_solve_column: steps
// 3 to 5, x left in wk.x, the backward error of the wave's columns returned) and the stores of (system, column) lk of the launch -- h, berr,
// the flag, x when asked for.  `bad`: what ac_load_factor returned for the system.  Shared by AcAdjSys (one column per system, lk = ls),
// AcAdjMultiSys and -- the solve -- AcSensSys: the same statements on the same doubles in the same x / r / y.  Every word of x, r and y is
// written before it is read, so a column leaves nothing to the next one
template <class M, class O = AcNoOvl>
__device__ __forceinline__ double ac_adj_solve_column(const AcAdjArgs& t, const AcWork& wk, const double* G, const double* C, double om, const double2* c, int lane,
                                                      const O& o = O()) {
  const AcArgs& a = t.a;
  const int n = a.n;
  double2 *lu = wk.lu, *x = wk.x, *r = wk.r, *y = wk.y;
  for (int j = lane; j < n; j += 64) y[j] = c[a.cperm[j]];
  M::sync();
  ac_adj_solve<M>(t, lu, y, lane);
  for (int i = lane; i < n; i += 64) x[a.rperm[i]] = y[i];
  M::sync();
  (void)ac_adj_residual<M, false>(t, G, C, om, c, x, r, lane, o);
  for (int j = lane; j < n; j += 64) y[j] = r[a.cperm[j]];
  M::sync();
  ac_adj_solve<M>(t, lu, y, lane);
  for (int i = lane; i < n; i += 64) { const int k = a.rperm[i]; const double2 xv = x[k], dv = y[i]; x[k] = make_double2(xv.x + dv.x, xv.y + dv.y); }
  M::sync();
  // ---- 5. backward error
  return ac_adj_residual<M, true>(t, G, C, om, c, x, r, lane, o);
}

template <class M, class O = AcNoOvl>
__device__ __forceinline__ void ac_adj_column(const AcAdjArgs& t, const AcWork& wk, const double* G, const double* C, double om, const double2* c,
                                              size_t lk, int bad, int lane, const O& o = O()) {
  const double worst = ac_adj_solve_column<M>(t, wk, G, C, om, c, lane, o);
  ac_store_column(t.a, wk.x, t.pairs, t.h, t.n_pairs, lk, worst, bad, lane);
}

// Steps 1 to 6 of the adjoint system ls of the launch; what ac_lu_system says about wk holds here word for word
template <class M, class O = AcNoOvl>
__device__ __forceinline__ void ac_adj_system(const AcAdjArgs& t, int ls, const AcWork& wk, int lane, const O& ovl = O()) {
  const AcArgs& a = t.a;
  const AcSysCtx<O> s = ac_sys_ctx(a, ls, ovl);
  const double2* c = (const double2*)a.bac + (size_t)s.inst * a.n;
  const int bad = ac_load_factor<M>(a, wk.lu, s.G, s.C, s.om, lane, s.o);
  ac_adj_column<M>(t, wk, s.G, s.C, s.om, c, (size_t)ls, bad, lane, s.o);
}

template <class O>
struct AcAdjSys {
  AcAdjArgs t; O ovl;
  static constexpr bool four = false, fenced = false;
  __host__ __device__ const AcArgs& base() const { return t.a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_adj_system<M>(t, ls, wk, lane, ovl); }
};

// ---- the multi-column kernel: A x_k = b_k for the K right-hand sides of an instance against ONE factorisation per system (cadnip_ac_solve_multi:
// the columns of a network's Y matrix, the responses to several sources) -------------------------------------------------------------------------
// Steps 1 and 2 once per system (ac_load_factor).  Then, per column k = 0 .. K-1, steps 3 to 5 of ac_lu_system word for word -- the same
// statements on the same doubles, in the same x / r / y, so column k holds what AcLuSys gives with b_k as its b_ac -- and the stores of step 6:
// x when the caller asked for it, the probe differences h[j] = x[p_j] - x[n_j] (pairs as AcAdjSys: -1 = ground, contributes 0), berr, the flag
// (bit 0: a zero / non-finite pivot of the system -- in all its K columns -- or a non-finite solution of THIS column).  Every word of x, r
// and y is written before it is read inside a column, as in ac_lu_system, so a column leaves nothing to the next one; the M::sync() that ends
// a column puts its last reads of x (the stores) before the next column's writes.  No atomics, no workgroup barrier.
struct AcMultiArgs {
  AcArgs a;                                 // a.x: x out [systems][K][n] (null: not wanted); a.berr / a.flags: [systems][K]; a.bac is not read
  const double* rhs; long rhs_stride;       // b [B][K][n] complex; complex words from one instance to the next (K n)
  const int* pairs; double* h;              // [n_pairs][2]; h out [systems][K][n_pairs] complex
  int n_rhs, n_pairs;
};

template <class M, class O = AcNoOvl>
__device__ __forceinline__ void ac_multi_system(const AcMultiArgs& t, int ls, const AcWork& wk, int lane, const O& ovl = O()) {
  const AcArgs& a = t.a;
  const AcSysCtx<O> s = ac_sys_ctx(a, ls, ovl);
  const int bad_pivot = ac_load_factor<M>(a, wk.lu, s.G, s.C, s.om, lane, s.o);
  for (int k = 0; k < t.n_rhs; ++k) {
    const double2* bac = (const double2*)t.rhs + (size_t)s.inst * t.rhs_stride + (size_t)k * a.n;
    const size_t lk = (size_t)ls * t.n_rhs + k;               // (system, column) of the launch: within int (api.hip bounds a launch's output)
    const double worst = ac_lu_column<M>(a, wk, s.G, s.C, s.om, bac, lane, s.o);
    ac_store_column(a, wk.x, t.pairs, t.h, t.n_pairs, lk, worst, bad_pivot, lane);
    M::sync();                                                 // the last reads of this column's x before the next column's (next system's) words
  }
}

// fenced: every system has a column (n_rhs >= 1: launch_ac_multi), and a column ends in M::sync() after its last read of the work arrays --
// the very fence k_ac_hbm would add.  The same holds for AcAdjMultiSys
template <class O>
struct AcLuMultiSys {
  AcMultiArgs t; O ovl;
  static constexpr bool four = false, fenced = true;
  __host__ __device__ const AcArgs& base() const { return t.a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_multi_system<M>(t, ls, wk, lane, ovl); }
};

// ---- the multi-column adjoint kernel: A^T x_k = c_k for the K columns of an instance against ONE factorisation per system (cadnip_ac_adjoint_multi:
// the noise of several outputs, the noise correlation matrix of an N-port) ------------------------------------------------------------------------
// Steps 1 and 2 once per system (ac_load_factor).  Then, per column k = 0 .. K-1, ac_adj_column -- the very function AcAdjSys runs, so column k
// holds what AcAdjSys gives with c_k as its c -- with the stores indexed by (system, column) as in ac_multi_system.  Flag bit 0: a zero /
// non-finite pivot of the system -- in all its K columns -- or a non-finite solution of THIS column.  The M::sync() that ends a column puts its
// last reads of x (the stores) before the next column's writes.  No atomics, no workgroup barrier.
struct AcAdjMultiArgs {
  AcAdjArgs t;                              // t.a.x: x out [systems][K][n] (null: not wanted); t.h: [systems][K][n_pairs]; t.a.berr / t.a.flags: [systems][K]; t.a.bac is not read
  const double* rhs; long rhs_stride;       // c [B][K][n] complex; complex words from one instance to the next (K n)
  int n_rhs;
};

template <class M, class O = AcNoOvl>
__device__ __forceinline__ void ac_adj_multi_system(const AcAdjMultiArgs& u, int ls, const AcWork& wk, int lane, const O& ovl = O()) {
  const AcArgs& a = u.t.a;
  const AcSysCtx<O> s = ac_sys_ctx(a, ls, ovl);
  const int bad_pivot = ac_load_factor<M>(a, wk.lu, s.G, s.C, s.om, lane, s.o);
  for (int k = 0; k < u.n_rhs; ++k) {
    const double2* c = (const double2*)u.rhs + (size_t)s.inst * u.rhs_stride + (size_t)k * a.n;
    const size_t lk = (size_t)ls * u.n_rhs + k;               // (system, column) of the launch: within int (api.hip bounds a launch's output)
    ac_adj_column<M>(u.t, wk, s.G, s.C, s.om, c, lk, bad_pivot, lane, s.o);
    M::sync();                                                 // the last reads of this column's x before the next column's (next system's) words
  }
}

template <class O>
struct AcAdjMultiSys {
  AcAdjMultiArgs u; O ovl;
  static constexpr bool four = false, fenced = true;
  __host__ __device__ const AcArgs& base() const { return u.t.a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_adj_multi_system<M>(u, ls, wk, lane, ovl); }
};

// ---- the sensitivity kernel: the response y = x[p] - x[n] of A x = b_ac and its derivatives with respect to K parameters from ONE factorisation
// per system (cadnip_ac_sens; SPICE's .SENS on an AC sweep).  With the adjoint solution A^T lambda = c, c = e_p - e_n,
//   dy/dp_k = lambda^T (db/dp_k - (dG/dp_k + j w dC/dp_k) x),
// and the parameter derivatives of G and C are central differences of the stamps of two perturbed instances of the SAME resident batch.  A
// system is (b, f) with b running over a LIST of base instances (u.base), not over the handle's instances.  The wave runs
//   1. / 2.  ac_load_factor on the base instance's G and C,
//   3.  the forward column (ac_lu_column: x is what AcLuSys gives for that instance), copied into the fourth vector xf, which outlives
//   4.  the adjoint column for c in the same x / r / y (ac_adj_solve_column: lambda is what AcAdjSys gives),
//   5.  s_k = sum_i lambda_i db_k[i] - sum_e lambda[row(e)] ((G+[e] - G-[e]) + j w (C+[e] - C-[e])) scale[b][k] xf[col(e)], k = 0 .. K-1, with
//       G+ / C+ the arrays of instance plus[b][k], G- / C- those of minus[b][k]: the differences are taken entry by entry from the handle's
//       device arrays -- no derivative array exists anywhere.  gmin sits in both and cancels.  The lanes stride over i and over the entries
//       (through the column view of the pattern, which carries an entry's row: a_row / a_pos of lu_transpose.hpp -- a fixed permutation of
//       the CSR positions), keep one partial sum each, and wave_sum (tran_ctrl.hpp) adds the 64,
//   6.  stores y, s[K], berr (forward, adjoint), one flag per column -- bit 0: zero / non-finite pivot or non-finite x or lambda of the SYSTEM,
//       in all its columns; bit 1: non-finite s_k -- and x, lambda when the caller asked for them.
// Every multiply-add is an explicit fma and the lane -> entry map does not depend on W or on where the work arrays live: the W instantiations
// and the HBM variant compute the same doubles.  No atomics, no workgroup barrier.
struct AcSensArgs {
  AcAdjArgs t;                              // t.a.bac: b_ac [NB][n]; t.a.x: x, lambda out [systems][2][n] (null: not wanted); t.a.berr: [systems][2]; t.a.flags: [systems][K]
  const int *base, *plus, *minus;           // [NB]; [NB][K]; [NB][K] instance indices
  const double *scale, *db, *c;             // [NB][K]; [NB][K][n] complex (null: zeros); [n] complex
  double *y, *s;                            // [systems] complex; [systems][K] complex
  int n_par, p, q;                          // K; the output pair (-1: ground)
};

// acc + a b
__device__ __forceinline__ double2 cmadd(double2 acc, double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, fma(-a.y, b.y, acc.x)), fma(a.x, b.y, fma(a.y, b.x, acc.y)));
}

template <class M>
__device__ __forceinline__ void ac_sens_system(const AcSensArgs& u, int ls, const AcWork& wk, int lane) {
  const AcAdjArgs& t = u.t;
  const AcArgs& a = t.a;
  const int n = a.n, K = u.n_par;
  const AcSysCtx<AcNoOvl> s = ac_sys_ctx<true>(a, ls, AcNoOvl(), u.base);
  const int bl = s.row;
  const double *G = s.G, *C = s.C;
  const double om = s.om;
  const double2* x = wk.x;
  double2* xf = wk.xf;
  const double2* bac = (const double2*)a.bac + (size_t)bl * n;
  const double2* c = (const double2*)u.c;
  int bad = ac_load_factor<M>(a, wk.lu, G, C, om, lane);
  // ---- 3. the forward column; x goes to xf
  const double berr_f = ac_wave_berr(ac_lu_column<M>(a, wk, G, C, om, bac, lane));
  double2* xo = a.x ? (double2*)a.x + (size_t)ls * 2 * n : nullptr;
  for (int i = lane; i < n; i += 64) { const double2 v = x[i]; if (!isfinite(v.x) || !isfinite(v.y)) bad = 1; xf[i] = v; if (xo) xo[i] = v; }
  M::sync();                                                   // xf for every lane; the last reads of x before the adjoint column's words
  // ---- 4. the adjoint column; lambda stays in x
  const double berr_a = ac_wave_berr(ac_adj_solve_column<M>(t, wk, G, C, om, c, lane));
  for (int i = lane; i < n; i += 64) { const double2 v = x[i]; if (!isfinite(v.x) || !isfinite(v.y)) bad = 1; if (xo) xo[n + i] = v; }
  bad = wave_any(bad);
  if (lane == 0) {
    const double2 xp = u.p >= 0 ? xf[u.p] : make_double2(0.0, 0.0), xn = u.q >= 0 ? xf[u.q] : make_double2(0.0, 0.0);
    ((double2*)u.y)[ls] = make_double2(xp.x - xn.x, xp.y - xn.y);
    a.berr[2 * (size_t)ls] = berr_f; a.berr[2 * (size_t)ls + 1] = berr_a;
  }
  // ---- 5. / 6. the bilinear forms
  for (int k = 0; k < K; ++k) {
    const size_t bk = (size_t)bl * K + k, lk = (size_t)ls * K + k;   // lk: within int (api.hip bounds a launch's output)
    const double *Gp = a.G + (size_t)u.plus[bk] * a.nnz, *Gm = a.G + (size_t)u.minus[bk] * a.nnz;
    const double *Cp = a.C + (size_t)u.plus[bk] * a.nnz, *Cm = a.C + (size_t)u.minus[bk] * a.nnz;
    const double sc = u.scale[bk];
    double2 acc = make_double2(0.0, 0.0);
    if (u.db) {
      const double2* db = (const double2*)u.db + bk * n;
      for (int i = lane; i < n; i += 64) acc = cmadd(acc, x[i], db[i]);
    }
    for (int q = lane; q < a.nnz; q += 64) {
      const int e = t.a_pos[q];
      const double2 dA = make_double2((Gp[e] - Gm[e]) * sc, (om * (Cp[e] - Cm[e])) * sc);
      acc = cmsub(acc, x[t.a_row[q]], cmul(dA, xf[a.colidx[e]]));
    }
    const double re = wave_sum(acc.x), im = wave_sum(acc.y);
    if (lane == 0) {
      ((double2*)u.s)[lk] = make_double2(re, im);
      a.flags[lk] = (bad ? 1 : 0) | ((!isfinite(re) || !isfinite(im)) ? 2 : 0);
    }
  }
}

struct AcSensSys {
  AcSensArgs u;
  static constexpr bool four = true, fenced = false;
  __host__ __device__ const AcArgs& base() const { return u.t.a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_sens_system<M>(u, ls, wk, lane); }
};

// ---- the Arnoldi family: an orthonormal basis of the Krylov space of K = A^-1 C started at A^-1 b_ac, A = G + gmin + j w_s C at the SHIFT
// j w_s, from ONE factorisation per system (cadnip_ac_arnoldi: poles, zeros and a reduced model of the descriptor system (C, -G) -- the
// eigenvalues theta of K are the poles p = j w_s - 1 / theta).  A system is (instance b, shift s).  The wave runs
//   1. / 2.  ac_load_factor at w_s,
//   3.  the start vector: x = A^-1 b_ac[b] by ac_lu_column (x is what AcLuSys gives for (b, w_s)), beta = ||x||_2, v_0 = x / beta.  beta zero
//       or non-finite: flag bit 1, m_eff = 0, no step,
//   4.  for j = 0 .. m-1: t = C[b] v_j (CSR rows, real C times complex v_j, one row per lane, into the fourth vector); w = A^-1 t by
//       ac_lu_column (solve, refinement, backward error, as every column of this file); nu_0 = ||w||_2; two passes of modified Gram-Schmidt
//       against v_0 .. v_j, H[i][j] the sum of the two passes' <v_i, w> (v_i conjugated); nu_1 = ||w||_2.  nu_0 = 0 or nu_1 <= tol nu_0: the
//       space has closed -- m_eff = j + 1, H[j+1][j] = 0, flag bit 2 (informational), the system is finished.  Else H[j+1][j] = nu_1 and
//       v_{j+1} = w / nu_1; without a breakdown m_eff = m,
//   5.  stores: H ((m+1) x m, zero beyond m_eff), beta, m_eff, the unconjugated probe projections l[j][p] = v_j[p_p] - v_j[n_p] (pairs as
//       AcAdjSys, zero beyond m_eff), berr -- the worst of the m_eff + 1 columns, a NaN stays --, the flag (bit 0: zero / non-finite pivot or a
//       non-finite word of H, beta or l; bits 1 and 2 as above), and the basis V ((m+1) x n; rows that hold no vector are zero).
// Where the vectors live.  w is ac_lu_column's x and is orthogonalised and normalised IN PLACE there, so the current v_j sits in a work
// array (LDS, or the wave's workspace) under the memory policy M, and everything that reads a vector ACROSS lanes -- the product C v_j
// through colidx, the probe differences -- reads that copy, behind M::sync().  The basis itself does not fit LDS next to the factors
// (16 (m+1) n bytes per system): it lives in global memory in both variants, in the launch's V buffer at the system's own index.  Its words are
// accessed by index k = lane, lane + 64, ... only -- written when a vector is normalised, read back by the dot products and the updates of
// the Gram-Schmidt passes -- so every lane reads only words it wrote itself: program order of one thread orders them, and the LDS kernel
// needs no global-memory fence (the HBM kernel's fences belong to its work arrays, as everywhere in this file).  H and l are written by the
// lane that read them (lane 0: the second pass adds to the word the first pass wrote) or once, at the end, where no vector was.
// Reductions: per-lane partial sums over k = lane, lane + 64, ... in index order, explicit fma, then the xor butterfly of ac_store_status --
// every lane holds the same double, whatever W and wherever the work arrays live.  No atomics, no workgroup barrier.
struct AcArnArgs {
  AcArgs a;                                 // a.bac: b_ac [B][n]; a.x is not used; a.berr / a.flags: [systems]
  const int* pairs;                         // [n_pairs][2]
  double *H, *beta, *l, *V;                 // [systems][m+1][m] complex; [systems]; [systems][m][n_pairs] complex; [systems][m+1][n] complex
  int* meff;                                // [systems]
  double tol; int m, n_pairs;
};

__device__ __forceinline__ double ac_wave_add(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// ||x||_2 over the lane's words k = lane, lane + 64, ...
__device__ __forceinline__ double ac_wave_norm(const double2* x, int n, int lane) {
  double p = 0.0;
  for (int k = lane; k < n; k += 64) { const double2 v = x[k]; p = fma(v.x, v.x, fma(v.y, v.y, p)); }
  return sqrt(ac_wave_add(p));
}

template <class M>
__device__ __forceinline__ void ac_arnoldi_system(const AcArnArgs& u, int ls, const AcWork& wk, int lane) {
  const AcArgs& a = u.a;
  const int n = a.n, m = u.m, P = u.n_pairs;
  const AcSysCtx<AcNoOvl> s = ac_sys_ctx(a, ls);
  const double *G = s.G, *C = s.C;
  const double om = s.om;
  double2 *x = wk.x, *t = wk.xf;
  const double2* bac = (const double2*)a.bac + (size_t)s.inst * n;
  double2* Ho = (double2*)u.H + (size_t)ls * (m + 1) * m;
  double2* lo = (double2*)u.l + (size_t)ls * m * P;
  double2* Vo = (double2*)u.V + (size_t)ls * (m + 1) * n;
  int bad = ac_load_factor<M>(a, wk.lu, G, C, om, lane);
  int flag = 0, meff = 0, nvec = 0;                              // nvec: rows of V that hold a vector
  // v_j := x / nrm in x and in row j of V; its probe projections
  auto take_vector = [&](int j, double nrm) {
    for (int k = lane; k < n; k += 64) { const double2 v = x[k]; const double2 q = make_double2(v.x / nrm, v.y / nrm); x[k] = q; Vo[(size_t)j * n + k] = q; }
    M::sync();                                                   // v_j for every lane
    if (j < m) for (int p = lane; p < P; p += 64) {
      const int pp = u.pairs[2 * p], pn = u.pairs[2 * p + 1];
      const double2 xp = pp >= 0 ? x[pp] : make_double2(0.0, 0.0), xn = pn >= 0 ? x[pn] : make_double2(0.0, 0.0);
      const double2 d = make_double2(xp.x - xn.x, xp.y - xn.y);
      if (!isfinite(d.x) || !isfinite(d.y)) bad = 1;
      lo[(size_t)j * P + p] = d;
    }
  };
  // ---- 3. the start vector
  double worst = ac_lu_column<M>(a, wk, G, C, om, bac, lane);
  const double beta = ac_wave_norm(x, n, lane);
  if (!isfinite(beta)) bad = 1;
  if (!(beta > 0.0) || !isfinite(beta)) flag = 2;
  else {
    take_vector(0, beta);
    nvec = 1; meff = m;
    // ---- 4. the steps
    for (int j = 0; j < m; ++j) {
      for (int i = lane; i < n; i += 64) {
        double2 acc = make_double2(0.0, 0.0);
        const int p1 = a.rowptr[i + 1];
        for (int p = a.rowptr[i]; p < p1; ++p) { const double c = C[p]; const double2 v = x[a.colidx[p]]; acc = make_double2(fma(c, v.x, acc.x), fma(c, v.y, acc.y)); }
        t[i] = acc;
      }
      M::sync();                                                 // t complete; the last reads of v_j in x before the column's words
      const double wj = ac_lu_column<M>(a, wk, G, C, om, t, lane);
      worst = (wj > worst || wj != wj) ? wj : worst;             // a NaN stays
      const double nu0 = ac_wave_norm(x, n, lane);
      for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i <= j; ++i) {
          const double2* vi = Vo + (size_t)i * n;
          double re = 0.0, im = 0.0;
          for (int k = lane; k < n; k += 64) {
            const double2 v = vi[k], w = x[k];
            re = fma(v.x, w.x, fma(v.y, w.y, re)); im = fma(v.x, w.y, fma(-v.y, w.x, im));
          }
          const double2 h = make_double2(ac_wave_add(re), ac_wave_add(im));
          for (int k = lane; k < n; k += 64) x[k] = cmsub(x[k], h, vi[k]);
          if (lane == 0) {
            double2 hs = h;
            if (pass) { const double2 h0 = Ho[(size_t)i * m + j]; hs = make_double2(h0.x + h.x, h0.y + h.y); }
            if (!isfinite(hs.x) || !isfinite(hs.y)) bad = 1;
            Ho[(size_t)i * m + j] = hs;
          }
        }
      const double nu1 = ac_wave_norm(x, n, lane);
      if (nu0 == 0.0 || nu1 <= u.tol * nu0) { meff = j + 1; flag |= 4; break; }
      if (!isfinite(nu1)) bad = 1;
      if (lane == 0) Ho[(size_t)(j + 1) * m + j] = make_double2(nu1, 0.0);
      take_vector(j + 1, nu1);
      nvec = j + 2;
    }
  }
  // ---- 5. the words no step wrote, and the status
  for (int e = lane; e < (m + 1) * m; e += 64) { const int i = e / m, j = e - i * m; if (j >= meff || i > j + 1 || (i == j + 1 && i >= nvec)) Ho[e] = make_double2(0.0, 0.0); }
  for (int e = lane + meff * P; e < m * P; e += 64) lo[e] = make_double2(0.0, 0.0);
  for (size_t e = (size_t)nvec * n + lane; e < (size_t)(m + 1) * n; e += 64) Vo[e] = make_double2(0.0, 0.0);
  worst = ac_wave_berr(worst);
  bad = wave_any(bad);
  if (lane == 0) { u.beta[ls] = beta; u.meff[ls] = meff; a.berr[ls] = worst; a.flags[ls] = flag | (bad ? 1 : 0); }
}

struct AcArnoldiSys {
  AcArnArgs u;
  static constexpr bool four = true, fenced = false;
  __host__ __device__ const AcArgs& base() const { return u.a; }
  template <class M> __device__ __forceinline__ void run(int ls, const AcWork& wk, int lane) const { ac_arnoldi_system<M>(u, ls, wk, lane); }
};

// ---- the two kernels.  Every family above runs through them: 10 system types (AcSensSys and AcArnoldiSys have no overlay form: their
// entry points refuse) x 2 homes x W = 1, 2, 4, 8, instantiated by ac_launch below.  Same launch plans, same layout, same lane order in
// both homes; no workgroup barrier, no atomics.
// Work arrays in LDS: one system per wave, W per workgroup
template <int W, class S>
__global__ void __launch_bounds__(64 * W) k_ac(S sys) {
  extern __shared__ double sm[];
  const AcArgs& a = sys.base();
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ls = blockIdx.x * W + w;                           // system of this wave inside the launch
  if (ls >= a.n_sys) return;                                   // the tail workgroup: no workgroup barrier anywhere below
  sys.template run<AcInLds>(ls, ac_work<S::four>((double*)sm, a.nnz_lu, a.n, w, W), lane);
}

// The HBM-resident form: the same steps with the work arrays in the wave's workspace in global memory (ac_hbm_plan.hpp).  Persistent
// waves: wave g of n_waves handles systems g, g + n_waves, ... of the launch in its one workspace -- region g of the family's layout over
// `work`, contiguous per wave, so a level's lanes touch neighbouring words.  The loop bound is the only tail handling: a wave beyond
// n_waves (the last workgroup when wpb does not divide n_waves) has no workspace and no system.  No workgroup barrier.
// Every system ends with the fence that puts its last reads of the work arrays (x; xf / t where there are four) before the next system's
// words.  A family whose run() already ends in exactly that fence says so (S::fenced) and gets no second one: the distinction is kept, not
// flattened, so that each family's instructions are the ones it had with a kernel of its own.
struct AcHbmArgs { double* work; int n_waves; };

template <int W, class S>
__global__ void __launch_bounds__(64 * W) k_ac_hbm(S sys, AcHbmArgs m) {
  const AcArgs& a = sys.base();
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.x * W + w, end = g < m.n_waves ? a.n_sys : 0;
  const AcWork wk = ac_work<S::four>(m.work, a.nnz_lu, a.n, g, m.n_waves);
  for (int ls = g; ls < end; ls += m.n_waves) {
    sys.template run<AcInHbm>(ls, wk, lane);
    if constexpr (!S::fenced) AcInHbm::sync();
  }
}


// The launch plan -- the one place that sizes the LDS block and picks W, and the only reader of CADNIP_AC_WPB.  A compute unit holds
// min(32 waves, LDS_BUDGET / block) workgroups' worth of systems: the plan takes the W with the most resident systems (ties: the largest),
// then halves it while the launch would not put a workgroup on half of the 256 compute units.
AcPlan ac_lu_plan(const CadnipHandle* h, long n_sys, int wpb_req, bool sens) {
  AcPlan none;
  if (!h->analyzed || n_sys <= 0) return none;
  auto bytes = [&](int wpb) {
    return sens ? lds_bytes(lds_ac_sens((size_t)0, h->lu.nnz_lu, h->n, 0, wpb)) : lds_bytes(lds_ac((size_t)0, h->lu.nnz_lu, h->n, 0, wpb));
  };
  if (wpb_req == 0) if (const char* e = getenv("CADNIP_AC_WPB")) wpb_req = atoi(e);
  if (wpb_req != 0) {
    if ((wpb_req != 1 && wpb_req != 2 && wpb_req != 4 && wpb_req != 8) || bytes(wpb_req) > LDS_BUDGET) return none;
    AcPlan p; p.wpb = wpb_req; p.shmem = bytes(wpb_req);
    return p;
  }
  if (bytes(1) > LDS_BUDGET) return none;
  int best = 1; size_t best_res = 0;
  for (int wpb = 1; wpb <= 8; wpb *= 2) {
    if (bytes(wpb) > LDS_BUDGET) break;
    const size_t res = std::min<size_t>(32, (LDS_BUDGET / bytes(wpb)) * wpb);
    if (res >= best_res) { best = wpb; best_res = res; }
  }
  while (best > 1 && n_sys < 128L * best) best >>= 1;
  AcPlan p; p.wpb = best; p.shmem = bytes(best);
  return p;
}

// Where the work arrays of a call live (cadnip_ac_set_memory) and the plan of that home: LDS -- ac_lu_plan alone, as ever; HBM -- the plan of
// ac_hbm_plan.hpp on this device's compute units; AUTO -- LDS when ac_lu_plan accepts the circuit, else HBM.  memory < 0: refused.
// sens: the plan of the families whose systems keep a fourth n-vector (AcSensSys, AcArnoldiSys)
AcLaunch ac_launch_plan(CadnipHandle* h, long n_sys, int wpb_req, bool sens) {
  AcLaunch L;
  AcState& A = h->ac;
  if (!h->analyzed || n_sys <= 0) return L;
  if (A.memory != CADNIP_AC_HBM) {
    L.lds = ac_lu_plan(h, n_sys, wpb_req, sens);
    if (L.lds.wpb > 0) { L.memory = CADNIP_AC_LDS; return L; }
    if (A.memory == CADNIP_AC_LDS) return L;
  }
  if (A.n_cu <= 0) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cu = 0;
    A.n_cu = cu > 0 ? cu : 256;
  }
  L.hbm = sens ? ac_hbm_plan_bytes(ac_sens_hbm_system_bytes(h->lu.nnz_lu, h->n), n_sys, wpb_req, A.max_waves, A.n_cu)
               : ac_hbm_plan(h->lu.nnz_lu, h->n, n_sys, wpb_req, A.max_waves, A.n_cu);
  if (L.hbm.wpb > 0) L.memory = CADNIP_AC_HBM;
  return L;
}

// the waves' workspace, grown like the other AC buffers: kept by the handle, released with it
static int ac_work_reserve(CadnipHandle* h, size_t bytes) {
  AcState& A = h->ac;
  if (A.cap_work >= bytes) return CADNIP_OK;
  if (A.d_work) { (void)hipFree(A.d_work); A.d_work = nullptr; }
  A.cap_work = 0;
  HIP_TRY(hipMalloc((void**)&A.d_work, bytes));
  A.cap_work = bytes;
  return CADNIP_OK;
}

namespace {
template <class T> int ac_upload(T** p, const std::vector<T>& v) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  HIP_TRY(hipMalloc((void**)p, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIP_TRY(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return CADNIP_OK;
}
}  // namespace

// the transposed-solve tables of the current LU program (lu_transpose.hpp) into AcState
static int ac_adjoint_tables(CadnipHandle* h) {
  AcState& A = h->ac;
  LUTranspose T;
  lu_transpose_build(h->lu, h->h_rowptr, h->h_colidx, T);
  TRY_RC(ac_upload(&A.d_t_colptr, T.t_colptr)); TRY_RC(ac_upload(&A.d_t_pos, T.t_pos)); TRY_RC(ac_upload(&A.d_t_row, T.t_row));
  TRY_RC(ac_upload(&A.d_t_diag, T.t_diag)); TRY_RC(ac_upload(&A.d_ut_rows, T.ut_rows)); TRY_RC(ac_upload(&A.d_ut_lev_ptr, T.ut_lev_ptr));
  TRY_RC(ac_upload(&A.d_lt_rows, T.lt_rows)); TRY_RC(ac_upload(&A.d_lt_lev_ptr, T.lt_lev_ptr));
  TRY_RC(ac_upload(&A.d_a_colptr, T.a_colptr)); TRY_RC(ac_upload(&A.d_a_row, T.a_row)); TRY_RC(ac_upload(&A.d_a_pos, T.a_pos));
  A.n_ut_lev = (int)T.ut_lev_ptr.size() - 1; A.n_lt_lev = (int)T.lt_lev_ptr.size() - 1;
  A.adj_ready = true;
  return CADNIP_OK;
}

int ac_lu_prepare(CadnipHandle* h, bool adjoint) {
  if (!h->analyzed) return CADNIP_NOTREADY;
  if (!h->ac.dirty) return adjoint && !h->ac.adj_ready ? ac_adjoint_tables(h) : CADNIP_OK;
  h->ac.adj_ready = false;                                     // tables of the previous program
  const LUProgram& P = h->lu;
  const int n_lev = (int)P.lev_ptr.size() - 1;
  // the factor level that computes each position (-1: final as loaded); a diagonal is only ever read as a pivot, by entries of later levels
  std::vector<int> lev_of(P.nnz_lu, -1);
  for (int l = 0; l < n_lev; ++l) for (int e = P.lev_ptr[l]; e < P.lev_ptr[l + 1]; ++e) lev_of[P.ent_pos[e]] = l;
  std::vector<int> ptr(n_lev + 2, 0), rows(h->n);
  for (int i = 0; i < h->n; ++i) ++ptr[lev_of[P.lu_diag[i]] + 2];
  for (int l = 1; l < n_lev + 2; ++l) ptr[l] += ptr[l - 1];
  std::vector<int> at(ptr.begin(), ptr.end() - 1);
  for (int i = 0; i < h->n; ++i) rows[at[lev_of[P.lu_diag[i]] + 1]++] = (!P.unit.empty() && P.unit[i]) ? ~i : i;
  if (!h->ac.d_nodiag) {
    std::vector<unsigned char> nd(h->n, 0);
    for (int i = 0; i < h->n_nodes; ++i) {
      nd[i] = 1;
      for (int p = h->h_rowptr[i]; p < h->h_rowptr[i + 1]; ++p) if (h->h_colidx[p] == i) nd[i] = 0;
    }
    TRY_RC(ac_upload(&h->ac.d_nodiag, nd));
  }
  TRY_RC(ac_upload(&h->ac.d_piv_rows, rows));
  TRY_RC(ac_upload(&h->ac.d_piv_lev_ptr, ptr));
  h->ac.dirty = false;
  return adjoint ? ac_adjoint_tables(h) : CADNIP_OK;
}

// the arguments every family shares: the handle's tables, the call's grid and -- the first input of every sweep -- omega; the family's
// launcher points b_ac and the outputs at its own slots of io
static AcArgs ac_args(CadnipHandle* h, const AcIo& io, int n_freq, long s0, int n_sys, double gmin) {
  const LUProgram& P = h->lu;
  AcArgs a{};
  a.G = h->d_G; a.C = h->d_C; a.omega = io.din(0); a.diag_flag = h->d_diag_flag; a.nodiag = h->ac.d_nodiag; a.gmin = gmin;
  a.rowptr = h->d_rowptr; a.colidx = h->d_colidx; a.load_dst = h->d_load_dst; a.ent_pos = h->d_ent_pos; a.ent_diag = h->d_ent_diag;
  a.ent_ptr = h->d_ent_ptr; a.term_a = h->d_term_a; a.term_b = h->d_term_b; a.lev_ptr = h->d_lev_ptr;
  a.lu_rowptr = h->d_lu_rowptr; a.lu_col = h->d_lu_col; a.lu_diag = h->d_lu_diag; a.rperm = h->d_rperm; a.cperm = h->d_cperm;
  a.fwd_rows = h->d_fwd_rows; a.fwd_lev_ptr = h->d_fwd_lev_ptr; a.bwd_rows = h->d_bwd_rows; a.bwd_lev_ptr = h->d_bwd_lev_ptr;
  a.piv_rows = h->ac.d_piv_rows; a.piv_lev_ptr = h->ac.d_piv_lev_ptr;
  a.n = h->n; a.nnz = h->nnz; a.nnz_lu = P.nnz_lu; a.n_lev = (int)P.lev_ptr.size() - 1;
  a.n_fwd_lev = (int)P.fwd_lev_ptr.size() - 1; a.n_bwd_lev = (int)P.bwd_lev_ptr.size() - 1;
  a.n_freq = n_freq; a.n_sys = n_sys; a.s0 = s0;
  return a;
}

// the handle's overlay (cadnip_ac_set_overlay) as the system types take it; n == 0: none is set, the AcNoOvl forms run
static AcOvl ac_ovl(const CadnipHandle* h) { return AcOvl{h->ac.d_ovl_pos, h->ac.d_ovl_map, (const double2*)h->ac.d_ovl_val, h->ac.ovl_n}; }

// The one launch of every family: the systems of `sys` in the home and under the plan of L, timed under the family's name for that home
template <class S>
static int ac_launch(CadnipHandle* h, const AcLaunch& L, const char* name_lds, const char* name_hbm, const S& sys) {
  const int n_sys = sys.base().n_sys;
  if (L.memory == CADNIP_AC_HBM) {
    const AcHbmPlan& p = L.hbm;
    if (p.n_waves <= 0 || p.n_waves > n_sys) return CADNIP_BADARG;
    TRY_RC(ac_work_reserve(h, p.work_bytes));
    ProfScope ps(h, name_hbm);
    const AcHbmArgs m{h->ac.d_work, p.n_waves};
    const int grid = (p.n_waves + p.wpb - 1) / p.wpb;
    TRY_RC(with_wpb(p.wpb, [&](auto W) { hipLaunchKernelGGL((k_ac_hbm<decltype(W)::value, S>), dim3(grid), dim3(64 * W.value), 0, h->stream, sys, m); return CADNIP_OK; }));
    HIP_TRY(hipGetLastError());
    return CADNIP_OK;
  }
  const AcPlan& p = L.lds;
  ProfScope ps(h, name_lds);
  const int grid = (n_sys + p.wpb - 1) / p.wpb;
  TRY_RC(with_wpb(p.wpb, [&](auto W) { return lds_launch(k_ac<decltype(W)::value, S>, grid, 64 * W.value, p.shmem, h->stream, sys); }));
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

// ... of a family with an overlay form: Sys<AcOvl> when the handle has one set, else Sys<AcNoOvl>, the statements without
template <template <class> class Sys, class Args>
static int ac_launch_ovl(CadnipHandle* h, const AcLaunch& L, const char* name_lds, const char* name_hbm, const Args& args) {
  const AcOvl v = ac_ovl(h);
  return v.n > 0 ? ac_launch(h, L, name_lds, name_hbm, Sys<AcOvl>{args, v}) : ac_launch(h, L, name_lds, name_hbm, Sys<AcNoOvl>{args, {}});
}

int launch_ac_lu(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_freq, long s0, int n_sys, double gmin) {
  if (L.memory < 0 || n_sys <= 0 || h->ac.dirty) return CADNIP_BADARG;
  AcArgs a = ac_args(h, io, n_freq, s0, n_sys, gmin);
  a.bac = io.din(1); a.x = io.dout(0); a.berr = io.dout(1); a.flags = io.iout(2);
  return ac_launch_ovl<AcLuSys>(h, L, "ac_lu", "ac_lu_hbm", a);
}

// the transposed-solve tables over ac_args
static AcAdjArgs ac_adj_args(CadnipHandle* h, const AcIo& io, int n_freq, long s0, int n_sys, double gmin) {
  AcState& A = h->ac;
  AcAdjArgs t{};
  t.a = ac_args(h, io, n_freq, s0, n_sys, gmin);
  t.t_colptr = A.d_t_colptr; t.t_pos = A.d_t_pos; t.t_row = A.d_t_row; t.t_diag = A.d_t_diag;
  t.ut_rows = A.d_ut_rows; t.ut_lev_ptr = A.d_ut_lev_ptr; t.lt_rows = A.d_lt_rows; t.lt_lev_ptr = A.d_lt_lev_ptr;
  t.a_colptr = A.d_a_colptr; t.a_row = A.d_a_row; t.a_pos = A.d_a_pos;
  t.n_ut_lev = A.n_ut_lev; t.n_lt_lev = A.n_lt_lev;
  return t;
}

int launch_ac_adjoint(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_pairs) {
  AcState& A = h->ac;
  if (L.memory < 0 || n_sys <= 0 || n_pairs <= 0 || A.dirty || !A.adj_ready) return CADNIP_BADARG;
  AcAdjArgs t = ac_adj_args(h, io, n_freq, s0, n_sys, gmin);
  t.a.bac = io.din(1); t.pairs = io.iin(2); t.n_pairs = n_pairs;
  t.h = io.dout(0); t.a.x = io.dout(1); t.a.berr = io.dout(2); t.a.flags = io.iout(3);
  return ac_launch_ovl<AcAdjSys>(h, L, "ac_adj", "ac_adj_hbm", t);
}

int launch_ac_multi(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_rhs, int n_pairs) {
  if (L.memory < 0 || n_sys <= 0 || n_rhs < 1 || n_pairs < 0 || (n_pairs == 0 && !io.out[1]) || h->ac.dirty) return CADNIP_BADARG;
  AcMultiArgs t{};
  t.a = ac_args(h, io, n_freq, s0, n_sys, gmin);
  t.rhs = io.din(1); t.rhs_stride = (long)n_rhs * h->n; t.pairs = io.iin(2); t.n_rhs = n_rhs; t.n_pairs = n_pairs;
  t.h = io.dout(0); t.a.x = io.dout(1); t.a.berr = io.dout(2); t.a.flags = io.iout(3);
  return ac_launch_ovl<AcLuMultiSys>(h, L, "ac_lu_multi", "ac_lu_multi_hbm", t);
}

int launch_ac_adjoint_multi(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_rhs, int n_pairs) {
  AcState& A = h->ac;
  if (L.memory < 0 || n_sys <= 0 || n_rhs < 1 || n_pairs < 0 || (n_pairs == 0 && !io.out[1]) || A.dirty || !A.adj_ready) return CADNIP_BADARG;
  AcAdjMultiArgs u{};
  u.t = ac_adj_args(h, io, n_freq, s0, n_sys, gmin);
  u.rhs = io.din(1); u.rhs_stride = (long)n_rhs * h->n; u.t.pairs = io.iin(2); u.n_rhs = n_rhs; u.t.n_pairs = n_pairs;
  u.t.h = io.dout(0); u.t.a.x = io.dout(1); u.t.a.berr = io.dout(2); u.t.a.flags = io.iout(3);
  return ac_launch_ovl<AcAdjMultiSys>(h, L, "ac_adj_multi", "ac_adj_multi_hbm", u);
}

int launch_ac_sens(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_freq, long s0, int n_sys, double gmin, int n_base, int n_par, const int* pair) {
  AcState& A = h->ac;
  if (L.memory < 0 || n_sys <= 0 || n_base < 1 || n_par < 1 || !pair || A.dirty || !A.adj_ready) return CADNIP_BADARG;
  AcSensArgs u{};
  u.t = ac_adj_args(h, io, n_freq, s0, n_sys, gmin);
  u.base = io.iin(1); u.plus = io.iin(2); u.minus = io.iin(3); u.scale = io.din(4); u.t.a.bac = io.din(5); u.db = io.din(6); u.c = io.din(7);
  u.y = io.dout(0); u.s = io.dout(1); u.t.a.x = io.dout(2); u.t.a.berr = io.dout(3); u.t.a.flags = io.iout(4);
  u.n_par = n_par; u.p = pair[0]; u.q = pair[1];
  return ac_launch(h, L, "ac_sens", "ac_sens_hbm", AcSensSys{u});
}

int launch_ac_arnoldi(CadnipHandle* h, const AcLaunch& L, const AcIo& io, int n_shift, long s0, int n_sys, double gmin, int m, double tol, int n_pairs) {
  if (L.memory < 0 || n_sys <= 0 || m < 1 || m > h->n || !(tol > 0.0 && tol < 1.0) || n_pairs < 0 || h->ac.dirty) return CADNIP_BADARG;
  AcArnArgs u{};
  u.a = ac_args(h, io, n_shift, s0, n_sys, gmin);
  u.a.bac = io.din(1); u.pairs = io.iin(2); u.tol = tol; u.m = m; u.n_pairs = n_pairs;
  u.H = io.dout(0); u.l = io.dout(1); u.V = io.dout(2); u.beta = io.dout(3); u.meff = io.iout(4); u.a.berr = io.dout(5); u.a.flags = io.iout(6);
  return ac_launch(h, L, "ac_arnoldi", "ac_arnoldi_hbm", AcArnoldiSys{u});
}

}  // namespace cadnip

