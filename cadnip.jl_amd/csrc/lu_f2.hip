// lu_f2.hip -- per-op refactor + solve (launch_factor_solve: the KLU step of a per-op Newton round, sweeps.jl:600 /
// solve.jl:667-670) executed with the fused kernel's entry program: J = G + gamma C scattered into a work array in LDS, the
// unified factor / forward / backward program of f2_program.cpp run on it (the dense core in registers), x gathered back.
// Four kernels, which differ in the shape of their loop and in where the program lives:
//   k_lu_f2<W>     the pass program (lane-packed entries, term lists), one wave per instance, W instances per workgroup sharing ONE
//                  copy of the tables in LDS; descriptor and first term of the next pass prefetched
//   k_lu_f2s<W>    the step program (straight-line steps of three terms per lane), otherwise the same; descriptors staged in LDS
//   k_lu_f2_mw<4>  the pass program, four waves per instance: the passes of a level dealt round-robin to the waves
//   k_lu_steps<4>  the step program, four waves per instance: descriptors prefetched from global memory, only W in LDS
// What they share is written once: the team (LuTeam), the load (lu_load), one step (step_open / step_finish), the dense core's
// dispatch (DENSE_CORE, fused2_kernel.hpp), the store and the flag rule (lu_store), the arguments (LuArgs).  The entry of a pass is
// written out in both pass kernels (see k_lu_f2_mw).
// launch_plan.hpp: lu_choose chooses among them and k_lu (kernels.hip: level by level on the LU program, factors in LDS or HBM), which also serves
// what this program cannot do: factor-only / solve-only (the callback ABI's cadnip_factor / cadnip_solve keep the factors in HBM).
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdlib.h>
#include "fused2_kernel.hpp"

namespace cadnip {

struct LuArgs {
  const unsigned* tab; int off[S_NSEC];          // the packed tables in global memory, section offsets in words
  int tab_len, tab_lo;                           // the words [tab_lo, tab_lo + tab_len) are staged in LDS (k_lu_steps: none)
  const uint4* steps; int steps_len;             // the step program (f2_build_steps), 16-byte lane descriptors; len in 64-bit words
  int n_pre, n_post;                             // passes or steps before / after the dense core
  const double *G, *C, *gamma, *rhs; double* x;
  const int* active; int* flags;
  int B, n, nnz, lu_words, nc, dn0;
};

// The threads that work on one instance: one wave (NW = 1, whatever the workgroup holds) or a workgroup of NW waves
template <int NW> struct LuTeam {
  static constexpr int NT = 64 * NW;
  const int lane, idx;                           // idx: 0 .. NT - 1
  __device__ __forceinline__ explicit LuTeam(int tid) : lane(tid & 63), idx(NW == 1 ? tid & 63 : tid) {}
  __device__ __forceinline__ void sync() const { if constexpr (NW == 1) CADNIP_WAVE_SYNC(); else __syncthreads(); }
};

// W := 0 [, the steps' constant words], J = G + gamma C at its L\U positions (every pattern entry has its own word: plain stores),
// rhs in pivot-row order.  loadpos: csr entry -> W word, rowof: unknown -> rhs word (LDS or global copies of the table sections)
template <bool CONSTS, class Team>
__device__ __forceinline__ void lu_load(const LuArgs& f, int inst, const Team& t, double* W, int nW, const u16* loadpos, const u16* rowof) {
  for (int i = t.idx; i < (nW >> 1); i += Team::NT) ((double2*)W)[i] = make_double2(0.0, 0.0);   // nW is even (f2_program.cpp)
  if (CONSTS && t.idx == 0) { W[nW] = 0.0; W[nW + 1] = 1.0; }                                    // (f2_build_steps)
  t.sync();
  const double* G = f.G + (size_t)inst * f.nnz;
  const double* C = f.C + (size_t)inst * f.nnz;
  const double gam = f.gamma[inst];
  for (int e = t.idx; e < f.nnz; e += Team::NT) W[loadpos[e]] = G[e] + gam * C[e];   // coalesced reads of the CSR arrays
  const double* rhs = f.rhs + (size_t)inst * f.n;
  for (int i = t.idx; i < f.n; i += Team::NT) W[rowof[i]] = rhs[i];
  t.sync();
}

// x gathered through qinv (unknown -> solution word); a non-finite solution or a bad pivot (`bad`, any lane) raises flag bit 0
template <class Team>
__device__ __forceinline__ void lu_store(const LuArgs& f, int inst, const Team& t, const double* W, const u16* qinv, int bad) {
  double* x = f.x + (size_t)inst * f.n;
  for (int i = t.idx; i < f.n; i += Team::NT) { const double v = W[qinv[i]]; if (!isfinite(v)) bad = 1; x[i] = v; }
  if (wave_any(bad) && t.lane == 0) atomicOr(&f.flags[inst], 1);
}

// One straight-line step of a lane from its 16-byte descriptor (f2_build_steps): word offsets of the entry, its pivot and the factors of
// three multiply-add terms, a flag in every field's top bit -- and the eight values.  (Two functions: k_lu_f2s requests its next
// descriptor between them, behind the operands in the LDS queue.)
struct StepEntry { double* pp; double piv, a0v, b0v, a1v, b1v, a2v, b2v, acc0; };
__device__ __forceinline__ StepEntry step_open(double* W, const uint4 D) {
  StepEntry e;
  e.pp = W + (D.x & 0x7FFFu);
  e.piv = W[(D.x >> 16) & 0x7FFFu];
  e.a0v = W[D.y & 0x7FFFu]; e.b0v = W[(D.y >> 16) & 0x7FFFu];
  e.a1v = W[D.z & 0x7FFFu]; e.b1v = W[(D.z >> 16) & 0x7FFFu];
  e.a2v = W[D.w & 0x7FFFu]; e.b2v = W[(D.w >> 16) & 0x7FFFu];
  e.acc0 = *e.pp;
  return e;
}
// ... finished: the three terms, the sums over the lane group, the division with the pivot test, the store -- to the entry, or to the lane's
// trash word where the lane does not lead its group.  UNIFORM_FLAGS: skip the sums beyond the step's widest group and the division of a
// step without one (both flags are the same in every lane: k_lu_f2s); else all four sums and the division always (a lane without a pivot
// divides by the constant 1: k_lu_steps)
template <bool UNIFORM_FLAGS>
__device__ __forceinline__ void step_finish(double* W, const uint4 D, const StepEntry& e, unsigned trash_w, int& bad) {
  unsigned maxlg = 4, div = 1;
  if constexpr (UNIFORM_FLAGS) {
    const unsigned fz = __builtin_amdgcn_readfirstlane(D.z), fw = __builtin_amdgcn_readfirstlane(D.w);
    maxlg = ((fz >> 15) & 1u) | ((fz >> 30) & 2u) | ((fw >> 13) & 4u);
    div = fw >> 31;
  }
  const unsigned lg = (D.x >> 31) | ((D.y >> 14) & 2u) | ((D.y >> 29) & 4u);
  double part = fma(e.a2v, e.b2v, fma(e.a1v, e.b1v, e.a0v * e.b0v));
  if (maxlg >= 1) { const double o = dpp_f64<0xB1>(part); part += lg >= 1 ? o : 0.0; }
  if (maxlg >= 2) { const double o = dpp_f64<0x4E>(part); part += lg >= 2 ? o : 0.0; }
  if (maxlg >= 3) { const double o = dpp_f64<0x141>(part); part += lg >= 3 ? o : 0.0; }
  if (maxlg >= 4) { const double o = dpp_f64<0x140>(part); part += lg >= 4 ? o : 0.0; }
  double acc = e.acc0 - part;
  if (div) {
    if (e.piv == 0.0 || !isfinite(e.piv)) bad = 1;
    acc = fast_div(acc, e.piv);
  }
  *((D.x & 0x8000u) ? e.pp : W + trash_w) = acc;
}

// The pass program, one wave per instance.  Software pipeline: the lane descriptor and the first term of pass p + 1 and the pass
// descriptor of pass p + 2 are requested while pass p runs
template <int WPB>
__global__ void __launch_bounds__(64 * WPB) k_lu_f2(LuArgs f) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), n = f.n;
  {
    const uint2* src = (const uint2*)f.tab;
    uint2* dst = (uint2*)sm;
    for (int i = tid; i < f.tab_len / 2; i += 64 * WPB) dst[i] = src[i];
  }
  __syncthreads();
  const int inst = blockIdx.x * WPB + w;
  if (inst >= f.B || !f.active[inst]) return;
  const unsigned* tab = (const unsigned*)sm;
  const LdsLu<double*> L = lds_lu((double*)sm, f.tab_len, 0, f.lu_words, n, false, w, WPB);
  double* W = L.W;
  const u16* loadpos = (const u16*)(tab + f.off[S_LOADPOS]);
  const u64* laned = (const u64*)(tab + f.off[S_ENT]);
  const unsigned* term = tab + f.off[S_TERM];
  // pass descriptors are wave-uniform: scalar loads from the table's copy in global memory (fused2_kernel.hpp)
  typedef const __attribute__((address_space(4))) u64* PassPtr;
  const PassPtr passd = (PassPtr)(const u64*)(f.tab + f.off[S_LEV]);
  const u16* qinv = (const u16*)(tab + f.off[S_QINV]);
  const u16* rowof = (const u16*)(tab + f.off[S_ROWOF]);
  const LuTeam<1> team(tid);
  lu_load<false>(f, inst, team, W, L.nW, loadpos, rowof);
  int bad = 0;
  auto run_passes = [&](const int p_first, const int p_count) {
    if (p_count <= 0) return;
    u64 pd = passd[p_first], pd1 = passd[p_first + 1];
    u64 D;
    unsigned T0;
    {
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pd), hi = __builtin_amdgcn_readfirstlane((unsigned)(pd >> 32));
      const int T = hi & 0x7F;
      D = laned[lo + (lane < T ? lane : T - 1)];
      T0 = term[(unsigned)(D >> 32) & 0xFFFFu];
    }
    for (int pi = p_first; pi < p_first + p_count; ++pi) {
      const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(pd >> 32));
      const int T = hi & 0x7F, maxlg = (hi >> 8) & 7, hasdiv = (hi >> 11) & 1, fence = (hi >> 12) & 1, multi = (hi >> 13) & 1;
      const bool act = lane < T;
      const unsigned pos = (unsigned)D & 0xFFFFu, dg = (unsigned)(D >> 16) & 0xFFFFu, t0 = (unsigned)(D >> 32) & 0xFFFFu;
      const unsigned dhi = (unsigned)(D >> 48);
      const int nt = act ? (int)(dhi & 0xFFu) : 0, lg = (dhi >> 8) & 7;
      const bool leader = act && ((dhi >> 12) & 1u);
      const double acc0 = W[pos];
      double piv = W[dg == NOPOS ? pos : dg];
      const double av = W[T0 & 0xFFFFu], bv = W[T0 >> 16];
      const unsigned lo1 = __builtin_amdgcn_readfirstlane((unsigned)pd1), hi1 = __builtin_amdgcn_readfirstlane((unsigned)(pd1 >> 32));
      const int T1 = hi1 & 0x7F;
      const u64 Dn = laned[lo1 + (lane < T1 ? lane : (T1 > 0 ? T1 - 1 : 0))];
      const u64 pd2 = passd[pi + 2];
      double part = nt > 0 ? av * bv : 0.0;
      const unsigned T0n = term[(unsigned)(Dn >> 32) & 0xFFFFu];
      if (multi)
        for (int t = 1; t < nt; ++t) { const unsigned tm = term[t0 + t]; part = fma(W[tm & 0xFFFFu], W[tm >> 16], part); }
      if (maxlg >= 1) { const double o = dpp_f64<0xB1>(part); part += lg >= 1 ? o : 0.0; }
      if (maxlg >= 2) { const double o = dpp_f64<0x4E>(part); part += lg >= 2 ? o : 0.0; }
      if (maxlg >= 3) { const double o = dpp_f64<0x141>(part); part += lg >= 3 ? o : 0.0; }
      if (maxlg >= 4) { const double o = dpp_f64<0x140>(part); part += lg >= 4 ? o : 0.0; }
      double acc = acc0 - part;
      if (hasdiv) {
        if (dg == NOPOS) piv = 1.0;
        else if (act && (piv == 0.0 || !isfinite(piv))) bad = 1;
        acc = fast_div(acc, piv);
      }
      if (leader) W[pos] = acc;
      if (fence) CADNIP_WAVE_SYNC();
      D = Dn; T0 = T0n; pd = pd1; pd1 = pd2;
    }
  };
  run_passes(0, f.n_pre);
  if (f.nc > 0) {
    DENSE_CORE(0, f.nc, W, f.dn0, f.lu_words + n - f.nc, lane, bad, false);
    CADNIP_WAVE_SYNC();
  }
  run_passes(f.n_pre, f.n_post);
  lu_store(f, inst, team, W, qinv, bad);
}

// The same kernel on the fused sweep kernel's STEP program (f2_program.cpp: f2_build_steps; fused2_kernel.hpp: run_steps): straight-line
// steps with three terms per lane, list-scheduled -- 7 + 6 steps instead of 9 + 8 passes on the flip-flop, and no term lists.  Staged in LDS:
// the load map and the permutations of the table, the step descriptors, the instances' work arrays.  Taken when the descriptors fit (a long
// dependency chain has one step per link: the pass program is the compact form).
template <int WPB>
__global__ void __launch_bounds__(64 * WPB) k_lu_f2s(LuArgs f) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), n = f.n;
  {
    const uint2* src = (const uint2*)(f.tab + f.tab_lo);
    uint2* dst = (uint2*)sm;
    for (int i = tid; i < f.tab_len / 2; i += 64 * WPB) dst[i] = src[i];
    const uint2* s2 = (const uint2*)f.steps;
    uint2* d2 = (uint2*)lds_lu((double*)sm, f.tab_len, f.steps_len, f.lu_words, n, true, w, WPB).desc;
    for (int i = tid; i < f.steps_len; i += 64 * WPB) d2[i] = s2[i];
  }
  __syncthreads();
  const int inst = blockIdx.x * WPB + w;
  if (inst >= f.B || !f.active[inst]) return;
  const unsigned* tab = (const unsigned*)sm;
  const LdsLu<double*> L = lds_lu((double*)sm, f.tab_len, f.steps_len, f.lu_words, n, true, w, WPB);
  const uint4* tdesc = (const uint4*)L.desc;
  double* W = L.W;
  const u16* loadpos = (const u16*)(tab + (f.off[S_LOADPOS] - f.tab_lo));
  const u16* qinv = (const u16*)(tab + (f.off[S_QINV] - f.tab_lo));
  const u16* rowof = (const u16*)(tab + (f.off[S_ROWOF] - f.tab_lo));
  const LuTeam<1> team(tid);
  lu_load<true>(f, inst, team, W, L.nW, loadpos, rowof);
  int bad = 0;
  const unsigned trash_w = (unsigned)(f.lu_words + n + lane);
  auto run_steps = [&](const int s_first, const int s_count) {
    if (s_count <= 0) return;
    const uint4* dp = tdesc + (size_t)s_first * 64 + lane;
    uint4 D = dp[0];
    for (int si = 0; si < s_count; ++si) {
      const StepEntry e = step_open(W, D);
      const uint4 Dn = dp[(size_t)(si + 1) * 64];
      step_finish<true>(W, D, e, trash_w, bad);
      D = Dn;
    }
    CADNIP_WAVE_SYNC();
  };
  run_steps(0, f.n_pre);
  if (f.nc > 0) {
    DENSE_CORE(0, f.nc, W, f.dn0, f.lu_words + n - f.nc, lane, bad, false);
    CADNIP_WAVE_SYNC();
  }
  run_steps(f.n_pre, f.n_post);
  lu_store(f, inst, team, W, qinv, bad);
}

// Few instances (a single transient, a handful of corners): one wave per instance leaves the chip empty and walks the passes one after
// the other -- the ring oscillator of BASELINE.json's config 5 (n = 371) has 105 of them in 46 dependency levels.  Here WPI waves share
// one instance: the passes of a level are dealt round-robin to the waves (they touch different entries and read only earlier levels), a
// workgroup barrier closes the level, the dense core is wave 0's.  No software pipeline: with so few waves the kernel is latency-bound anyway.
template <int WPI>
__global__ void __launch_bounds__(64 * WPI) k_lu_f2_mw(LuArgs f) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), n = f.n;
  {
    const uint2* src = (const uint2*)f.tab;
    uint2* dst = (uint2*)sm;
    for (int i = tid; i < f.tab_len / 2; i += 64 * WPI) dst[i] = src[i];
  }
  const int inst = blockIdx.x;
  if (inst >= f.B || !f.active[inst]) return;                 // (uniform over the workgroup: nobody is left waiting at a barrier)
  const unsigned* tab = (const unsigned*)sm;
  const LdsLu<double*> L = lds_lu((double*)sm, f.tab_len, 0, f.lu_words, n, false, 0, 1);
  double* W = L.W;
  const u16* loadpos = (const u16*)(tab + f.off[S_LOADPOS]);
  const u64* laned = (const u64*)(tab + f.off[S_ENT]);
  const unsigned* term = tab + f.off[S_TERM];
  typedef const __attribute__((address_space(4))) u64* PassPtr;
  const PassPtr passd = (PassPtr)(const u64*)(f.tab + f.off[S_LEV]);
  const u16* qinv = (const u16*)(tab + f.off[S_QINV]);
  const u16* rowof = (const u16*)(tab + f.off[S_ROWOF]);
  const LuTeam<WPI> team(tid);
  lu_load<false>(f, inst, team, W, L.nW, loadpos, rowof);   // (its first barrier: the tables are staged)
  int bad = 0;
  auto run_passes = [&](const int p_first, const int p_count) {
    int in_level = 0;
    for (int pi = p_first; pi < p_first + p_count; ++pi) {
      const u64 pd = passd[pi];
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pd), hi = __builtin_amdgcn_readfirstlane((unsigned)(pd >> 32));
      const int T = hi & 0x7F, maxlg = (hi >> 8) & 7, hasdiv = (hi >> 11) & 1, fence = (hi >> 12) & 1;
      if (in_level % WPI == w && T > 0) {
        // (the same entry text as k_lu_f2's, on purpose: through shared functions the two uniform branches of this loop came out with
        // the opposite sense and the kernel measured 0.1 us slower on the flip-flop at B = 1100 -- DESIGN.md section 5)
        const bool act = lane < T;
        const u64 D = laned[lo + (act ? lane : T - 1)];
        const unsigned pos = (unsigned)D & 0xFFFFu, dg = (unsigned)(D >> 16) & 0xFFFFu, t0 = (unsigned)(D >> 32) & 0xFFFFu;
        const unsigned dhi = (unsigned)(D >> 48);
        const int nt = act ? (int)(dhi & 0xFFu) : 0, lg = (dhi >> 8) & 7;
        const bool leader = act && ((dhi >> 12) & 1u);
        const double acc0 = W[pos];
        double piv = W[dg == NOPOS ? pos : dg];
        double part = 0.0;
        for (int t = 0; t < nt; ++t) { const unsigned tm = term[t0 + t]; part = fma(W[tm & 0xFFFFu], W[tm >> 16], part); }
        if (maxlg >= 1) { const double o = dpp_f64<0xB1>(part); part += lg >= 1 ? o : 0.0; }
        if (maxlg >= 2) { const double o = dpp_f64<0x4E>(part); part += lg >= 2 ? o : 0.0; }
        if (maxlg >= 3) { const double o = dpp_f64<0x141>(part); part += lg >= 3 ? o : 0.0; }
        if (maxlg >= 4) { const double o = dpp_f64<0x140>(part); part += lg >= 4 ? o : 0.0; }
        double acc = acc0 - part;
        if (hasdiv) {
          if (dg == NOPOS) piv = 1.0;
          else if (act && (piv == 0.0 || !isfinite(piv))) bad = 1;
          acc = fast_div(acc, piv);
        }
        if (leader) W[pos] = acc;
      }
      ++in_level;
      if (fence) { __syncthreads(); in_level = 0; }
    }
  };
  run_passes(0, f.n_pre);
  if (f.nc > 0) {
    if (w == 0) DENSE_CORE(0, f.nc, W, f.dn0, f.lu_words + n - f.nc, lane, bad, false);
    __syncthreads();
  }
  run_passes(f.n_pre, f.n_post);
  lu_store(f, inst, team, W, qinv, bad);
}

// The same refactor + solve as straight-line STEPS for a team of four waves per instance (f2_program.cpp: f2_build_steps with nw = 4):
// every thread owns one 16-byte descriptor per step; steps are list-scheduled (an entry runs in the first step behind its operands' last
// writers that has a lane group free), a barrier closes each.  The descriptors are per thread: they are fetched from global memory a CHUNK
// of steps ahead into registers (the loads of chunk c + 1 are in flight while chunk c runs), nothing of the program lives in LDS -- only
// the work array does, and the load map and the permutations are read from the table in global memory -- so a circuit whose tables do not
// fit beside it (the PSP103 ring: 87 steps x 256 threads; 116 with one term per lane and level-aligned steps) runs here all the same.
// For few instances -- where k_lu_f2's one wave per instance walks 100+ passes alone.
#define LU_CHUNK 8
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_lu_steps(LuArgs f) {
  constexpr int NT = 64 * NW;
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), n = f.n;
  const int inst = blockIdx.x;
  if (inst >= f.B || !f.active[inst]) return;                 // (uniform over the workgroup)
  const LdsLu<double*> L = lds_lu((double*)sm, 0, 0, f.lu_words, n, true, 0, 1);
  double* W = L.W;
  // this thread's descriptors of the first chunk: requested before the matrix is loaded
  const uint4* dp = f.steps + tid;
  uint4 cur[LU_CHUNK], nxt[LU_CHUNK];
  const int n_steps = f.n_pre + f.n_post;
#pragma unroll
  for (int k = 0; k < LU_CHUNK; ++k) cur[k] = dp[(size_t)(k < n_steps ? k : 0) * NT];
  const LuTeam<NW> team(tid);
  lu_load<true>(f, inst, team, W, L.nW, (const u16*)(f.tab + f.off[S_LOADPOS]), (const u16*)(f.tab + f.off[S_ROWOF]));
  int bad = 0;
  const unsigned trash_w = (unsigned)(f.lu_words + n + lane);
  // chunks of LU_CHUNK steps; the dense core sits between step n_pre - 1 and step n_pre
  for (int c0 = 0; c0 < n_steps; c0 += LU_CHUNK) {
#pragma unroll
    for (int k = 0; k < LU_CHUNK; ++k) { const int sidx = c0 + LU_CHUNK + k; nxt[k] = dp[(size_t)(sidx < n_steps ? sidx : 0) * NT]; }
#pragma unroll
    for (int k = 0; k < LU_CHUNK; ++k) {
      const int sidx = c0 + k;
      if (sidx == f.n_pre && f.nc > 0) {                     // (uniform)
        if (w == 0) DENSE_CORE(0, f.nc, W, f.dn0, f.lu_words + n - f.nc, lane, bad, false);
        __syncthreads();
      }
      if (sidx < n_steps) { step_finish<false>(W, cur[k], step_open(W, cur[k]), trash_w, bad); __syncthreads(); }
    }
#pragma unroll
    for (int k = 0; k < LU_CHUNK; ++k) cur[k] = nxt[k];
  }
  if (f.n_post == 0 && f.nc > 0) {                            // (no step behind the core: it has not run yet)
    if (w == 0) DENSE_CORE(0, f.nc, W, f.dn0, f.lu_words + n - f.nc, lane, bad, false);
    __syncthreads();
  }
  lu_store(f, inst, team, W, (const u16*)(f.tab + f.off[S_QINV]), bad);
}

// The plan of launch_factor_solve: launch_plan.hpp decides (lu_choose); here its facts are gathered -- the tables built unless k_lu runs whatever
// they hold -- and CADNIP_LU_PLAIN / _STEPS / _WPI / _F2S read, at every call and only where they count: a forced kernel ignores them.  This
// sits in the per-op Newton loop, where the choice used to cost two to four getenv calls depending on how far it got: the four are read in
// ONE pass over the environment (the first entry of a name counts, as for getenv), so that no batch size pays more look-ups than before
extern "C" char** environ;
static LuSwitches lu_switches() {
  static const char* const names[4] = {"PLAIN=", "STEPS=", "WPI=", "F2S="};
  int v[4] = {SW_UNSET, SW_UNSET, SW_UNSET, SW_UNSET};
  for (char** e = environ; e && *e; ++e) {
    if (strncmp(*e, "CADNIP_LU_", 10)) continue;
    for (int i = 0; i < 4; ++i) {
      const size_t nl = strlen(names[i]);
      if (v[i] == SW_UNSET && !strncmp(*e + 10, names[i], nl)) v[i] = atoi(*e + 10 + nl);
    }
  }
  return LuSwitches{v[0], v[1], v[2], v[3]};
}
static int lu_f2_plan(CadnipHandle* h, bool fuse, int kernel, LuPlan& p) {
  const LuSwitches sw = kernel == CADNIP_LUK_AUTO ? lu_switches() : LuSwitches();
  PlanFacts f;
  TRY_RC(plan_facts(h, !lu_takes_plain(sw, fuse, kernel), false, f));
  f.lu_plain_threads = lu_plain_threads(h, true);
  p = lu_choose(f, sw, fuse, kernel);
  return CADNIP_OK;
}

// the arguments of the program kernel of plan p
static LuArgs lu_args(const CadnipHandle* h, const LuPlan& p, const double* d_rhs, double* d_x) {
  const FusedState& S = h->f2;
  const StepList& steps = p.kernel == CADNIP_LUK_STEPS4 ? S.steps4 : S.steps1;
  const bool stepped = p.kernel == CADNIP_LUK_STEPS4 || p.kernel == CADNIP_LUK_F2S;
  LuArgs f{};
  f.tab = S.d_tab; for (int i = 0; i < S_NSEC; ++i) f.off[i] = S.off[i];
  f.tab_lo = p.tab_lo; f.tab_len = p.tab_len;
  if (stepped) { f.steps = (const uint4*)steps.d; f.steps_len = steps.len; }
  f.G = h->d_G; f.C = h->d_C; f.gamma = h->d_gamma; f.rhs = d_rhs; f.x = d_x; f.active = h->d_active; f.flags = h->d_flags;
  f.B = h->B; f.n = h->n; f.nnz = h->nnz; f.lu_words = S.lu_words; f.n_pre = p.pre; f.n_post = p.post; f.nc = S.nc; f.dn0 = S.dn0;
  return f;
}

// refactor of G + gamma C (fuse; else of d_J) followed by the solve.  kernel: CADNIP_LUK_*; a forced kernel needs the fused Jacobian, and one
// that does not apply is CADNIP_BADARG with nothing launched.  info [6] (optional): kernel, waves per workgroup, waves per instance, nc, steps
// or passes before / after the dense core (zeros for k_lu).  dry: choose and fill info, launch nothing
int launch_factor_solve(CadnipHandle* h, bool fuse, const double* d_rhs, double* d_x, int kernel, int* info, bool dry) {
  if (kernel < CADNIP_LUK_AUTO || kernel > CADNIP_LUK_PLAIN || (kernel != CADNIP_LUK_AUTO && !fuse)) return CADNIP_BADARG;
  if (!h->analyzed) return CADNIP_NOTREADY;
  LuPlan p;
  TRY_RC(lu_f2_plan(h, fuse, kernel, p));
  if (p.kernel < 0) return CADNIP_BADARG;
  if (info) { info[0] = p.kernel; info[1] = p.wpb; info[2] = p.wpi; info[3] = p.nc; info[4] = p.pre; info[5] = p.post; }
  if (dry) return CADNIP_OK;
  if (p.kernel == CADNIP_LUK_PLAIN) return launch_lu(h, "lu_factor_solve", 1, 1, fuse, d_rhs, d_x, 64 * p.wpb);
  ProfScope ps(h, "lu_factor_solve");
  const LuArgs f = lu_args(h, p, d_rhs, d_x);
  const int grid = p.wpi > 1 ? h->B : (h->B + p.wpb - 1) / p.wpb;   // a workgroup per instance, or per wpb instances
  if (p.kernel == CADNIP_LUK_STEPS4) TRY_RC(lds_launch(k_lu_steps<4>, grid, 256, p.shmem, h->stream, f));
  else if (p.kernel == CADNIP_LUK_F2MW) TRY_RC(lds_launch(k_lu_f2_mw<4>, grid, 256, p.shmem, h->stream, f));
  else if (p.kernel == CADNIP_LUK_F2S) TRY_RC(with_wpb(p.wpb, [&](auto W) { return lds_launch(k_lu_f2s<decltype(W)::value>, grid, 64 * W.value, p.shmem, h->stream, f); }));
  else TRY_RC(with_wpb(p.wpb, [&](auto W) { return lds_launch(k_lu_f2<decltype(W)::value>, grid, 64 * W.value, p.shmem, h->stream, f); }));
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

}  // namespace cadnip
