// lds_layout.hpp -- THE map of the dynamic LDS block of every LDS-resident kernel (k_fused2, k_fteam, k_lu_*, k_ac).  The kernels take their
// pointers from it and the launchers their `shmem`: nobody else adds up table, descriptor or work-array words.  Plain C++ behind the
// __host__ __device__ markers (tests/test_lds_layout.py compiles it with the host compiler).
//
// Every function is generic in the base P: with the kernel's `extern __shared__ double sm[]` it returns the region pointers, with
// (size_t)0 on the host the same regions as offsets in doubles, `end` being the size of the block (lds_bytes).  Alignment: the staged
// tables are a multiple of 4 32-bit words (fused2.hip: pad4), a step list a multiple of 128 words (16 bytes per lane), lu_words + n is even
// (f2_program.cpp) -- so every work array W (cleared as double2) and every descriptor area (read as uint4) starts on 16 bytes.
#pragma once
#include <stddef.h>
#include "../../include/cadnip_hip.h"   // device type codes (f2_shape_ok)
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <type_traits>
#define LDS_HD __host__ __device__ __forceinline__
#else
#define LDS_HD inline
#endif

#define F2_TRASH 64        // per-instance trash words (one per lane) that absorb stamps into ground rows / columns
#define F2_MAX_BLOCKS 32   // device blocks of one circuit (one per built-in type, one per Verilog-A module); more: per-op path
#define LDS_BUDGET ((size_t)160 * 1024)   // LDS of a gfx950 compute unit = the most one workgroup may ask for
#define LDS_OPTIN ((size_t)64 * 1024)     // above this a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize raised (lds_launch)

namespace cadnip {

// one work array: L\U entries (lu_words) | rhs in pivot-row order (n) | trash words; the part a Newton round clears
LDS_HD int lds_work_words(int lu_words, int n) { return lu_words + n + F2_TRASH; }
#define LDS_CONSTS 2       // the step programs' constant words 0.0, 1.0 directly behind the trash words (f2_build_steps / f2_build_team)

// ---- the sweep kernel's PRE-DECODED step descriptors.  f2_build_steps packs a lane's step as eight 15-bit WORD offsets into W with a flag in
// every field's top bit (x: entry | pivot, y: a0 | b0, z: a1 | b1, w: a2 | b2; f2_program.cpp).  That format stays what the host builds and
// what k_lu_f2s / k_lu_steps / k_fteam read; k_fused2 converts it once per launch, while it stages the descriptors, into eight 16-bit BYTE
// offsets from the instance's W -- an operand address is one add of a 16-bit half -- with no flag among them:
//   * a lane that does not lead its group gets its own trash word as its entry, so every lane stores to its entry unconditionally;
//   * the lane's group width and the step's two uniform flags go to one byte per lane and step behind the descriptors:
//     bits 4-6 log2 of the lane group's width, bit 3 "an entry of this step divides", bits 0-2 log2 of the step's widest group --
//     `lg >= k` is `byte >= 16 k`, one compare against an inline constant.
// Byte offsets need every word of W | consts below 8192: lds_steps_predec_ok; the launch plan (launch_plan.hpp: f2_choose) decides.
struct StepPredec { unsigned x, y, z, w, flags; };
LDS_HD StepPredec lds_step_predecode(unsigned x, unsigned y, unsigned z, unsigned w, unsigned trash_word) {
  StepPredec r;
  r.x = ((x & 0x8000u) ? (x & 0x7FFFu) : trash_word) << 3 | ((x >> 16) & 0x7FFFu) << 19;
  r.y = (y & 0x7FFF7FFFu) << 3; r.z = (z & 0x7FFF7FFFu) << 3; r.w = (w & 0x7FFF7FFFu) << 3;
  const unsigned lg = (x >> 31) | ((y >> 14) & 2u) | ((y >> 29) & 4u);
  const unsigned maxlg = ((z >> 15) & 1u) | ((z >> 30) & 2u) | ((w >> 13) & 4u);
  r.flags = lg << 4 | (w >> 31) << 3 | maxlg;
  return r;
}
LDS_HD bool lds_steps_predec_ok(int lu_words, int n) { return lu_words + n + F2_TRASH + LDS_CONSTS <= 8192; }
// ---- the sweep kernel's FIXED form (k_fused2<WPB, false, 3>, fused2_kernel.hpp): the lean transient kernel with every switch of the default
// call a compile-time constant.  THE list of what that kernel assumes; a launch that misses one condition takes the generic variant 0, which
// computes the same to the bit.  `enabled`: CADNIP_F2_FIXED is not 0 (diagnostic, tests; launch_plan.hpp: f2_choose is handed it and calls this).
LDS_HD bool f2_fixed_ok(bool tran, bool lean, int newton_mode, bool step_predec, int src_words, int n, int nc, int max_order, int step_rule,
                        int use_pcnr, bool enabled) {
  return tran && lean && newton_mode == 1 && step_predec && src_words > 0 && n <= 256 && nc == 8 && max_order <= 2 && step_rule == 0 &&
         use_pcnr == 0 && enabled;
}
// ---- ... and its SHAPE form (k_fused2<WPB, false, 4>): the fixed form with the circuit's block list fixed as well, to what every CMOS-cell
// characterisation deck has -- voltage sources, plain sp_mos1 transistors, capacitors, nothing else.  THE list of what that kernel assumes beyond
// f2_fixed_ok (`fixed`); a launch that misses one condition takes variant 3 (or 0), which computes the same to the bit.  The facts come from the
// block list of fused2.hip: fused2_blocks -- n_blk blocks, of which src_* is the pinned source block (F2Args::src_blk), rc_* the pinned
// capacitor / resistor block (F2Args::rc_blk) and dev_* the remaining one (a type of -1: there is no such block).  With three blocks, one of them
// the first of the source types and another the first of the R / C types, each is the only one of its kind.  The counts: a pinned block of at
// most 64 has one device per lane and nothing left for the block loop; 32 lane-paired sp_mos1 devices are one pass of a wave.
// `enabled`: CADNIP_F2_SHAPE is not 0 (diagnostic, tests; f2_choose is handed it and calls this).
LDS_HD bool f2_shape_ok(bool fixed, int n_blk, int src_type, int src_count, int rc_type, int rc_count, int dev_type, int dev_plain, int dev_count,
                        bool enabled) {
  return fixed && n_blk == 3 && src_type == CADNIP_DEV_VSOURCE && src_count <= 64 && rc_type == CADNIP_DEV_CAPACITOR && rc_count <= 64 &&
         dev_type == CADNIP_DEV_MOS1 && dev_plain != 0 && dev_count <= 32 && enabled;
}
// ---- ... and the words the shape form PINS for its sp_mos1 lanes (fused2_kernel.hpp; devices.hpp: M1PairView).  A lane serves one device and one
// junction side for a whole launch, so what the circuit alone decides is resolved once, as 16-bit halves like the pinned capacitor / source words:
//   * an operand -- a terminal voltage, a limit or charge unknown -- as the BYTE offset of its word of u from the instance's W (u lies behind
//     W | consts, lds_sweep); ground (node < 0) is the constant word 0.0, so that reading a voltage is one unconditional read of the same 0.0;
//   * a residual target as the WORD of W that `rowof` names for the unknown; ground is the lane's trash word.
// Byte offsets of u need W | consts | u below 8192 words: lds_m1pin_ok (one more condition of the shape form; launch_plan.hpp: f2_choose).
LDS_HD bool lds_m1pin_ok(int lu_words, int n) { return lds_work_words(lu_words, n) + LDS_CONSTS + n <= 8192; }
LDS_HD unsigned lds_m1pin_operand(int node, int lu_words, int n) {
  const int nW = lds_work_words(lu_words, n);
  return (unsigned)(node < 0 ? nW : nW + LDS_CONSTS + node) << 3;
}
template <class T> LDS_HD unsigned lds_m1pin_row(const T* rowof, int node, unsigned trash_word) { return node < 0 ? trash_word : (unsigned)rowof[node]; }
// 64-bit words of the descriptor area: desc_len as uploaded (two per lane and step), plus one flag byte per lane and step when pre-decoded
LDS_HD int lds_sweep_desc_words(int desc_len, bool predec) { return desc_len + (predec ? desc_len / 16 : 0); }

// sweep kernel k_fused2<WPB>: tables | step descriptors (lean variant; desc_len = lds_sweep_desc_words) | WPB x [ W | consts | u | beta | src ]; W, u, beta,
// src: of instance w.  src: the source segment cache (src_cache.hpp: src_cache_words doubles, an even number; 0 = the launch runs without it)
template <class P> struct LdsSweep { P desc, W, u, beta, end; int nW, per; P src; };   // nW, per: doubles of one work array / one instance
template <class P> LDS_HD LdsSweep<P> lds_sweep(P base, int tab_len, int desc_len, int lu_words, int n, int w, int wpb, int src_words = 0) {
  LdsSweep<P> L;
  L.nW = lds_work_words(lu_words, n);
  L.per = L.nW + LDS_CONSTS + 2 * n + src_words;
  L.desc = base + tab_len / 2;
  L.W = L.desc + desc_len + (size_t)w * L.per;
  L.u = L.W + L.nW + LDS_CONSTS; L.beta = L.u + n; L.src = L.beta + n;
  L.end = L.desc + desc_len + (size_t)wpb * L.per;
  return L;
}

// team kernel k_fteam<NW>: tables | W | consts | red [NW][4] | u | beta | sp_mos1 parameter rows (rounded up to even) | step descriptors |
// NW - 1 private copies of W
template <class P> struct LdsTeam { P W, red, u, beta, par, desc, priv, end; int nW; };
template <class P> LDS_HD LdsTeam<P> lds_team(P base, int tab_len, int desc_len, int lu_words, int n, int par_words, int nw) {
  LdsTeam<P> L;
  L.nW = lds_work_words(lu_words, n);
  L.W = base + tab_len / 2;
  L.red = L.W + L.nW + LDS_CONSTS; L.u = L.red + 4 * nw; L.beta = L.u + n; L.par = L.beta + n;
  L.desc = L.par + ((par_words + 1) & ~1); L.priv = L.desc + desc_len;
  L.end = L.priv + (nw ? (size_t)(nw - 1) * L.nW : 0);
  return L;
}

// refactor + solve kernels k_lu_*: tables | step descriptors | waves x [ W | consts (step programs only) ]; W: of wave w.  k_lu_f2_mw and
// k_lu_steps keep one work array per workgroup (waves = 1), k_lu_steps stages neither tables nor descriptors
template <class P> struct LdsLu { P desc, W, end; int nW, per; };
template <class P> LDS_HD LdsLu<P> lds_lu(P base, int tab_len, int desc_len, int lu_words, int n, bool consts, int w, int waves) {
  LdsLu<P> L;
  L.nW = lds_work_words(lu_words, n);
  L.per = L.nW + (consts ? LDS_CONSTS : 0);
  L.desc = base + tab_len / 2;
  L.W = L.desc + desc_len + (size_t)w * L.per;
  L.end = L.desc + desc_len + (size_t)waves * L.per;
  return L;
}
// AC kernel k_ac<W, S> (ac_lu.hip), three-vector families: W x [ complex L\U factors (nnz_lu) | x: rhs / solution (n) | r: residual (n) | y: correction, the solves' work
// vector (n) ], every value an interleaved (re, im) pair of doubles -- 16 (nnz_lu + 3 n) bytes per system, each region on 16 bytes.  No
// tables: the index arrays are read from global memory.  Regions of system w of the workgroup
template <class P> struct LdsAc { P lu, x, r, y, end; int per; };   // per: doubles of one system
template <class P> LDS_HD LdsAc<P> lds_ac(P base, int nnz_lu, int n, int w, int wpb) {
  LdsAc<P> L;
  L.per = 2 * (nnz_lu + 3 * n);
  L.lu = base + (size_t)w * L.per;
  L.x = L.lu + 2 * (size_t)nnz_lu; L.r = L.x + 2 * (size_t)n; L.y = L.r + 2 * (size_t)n;
  L.end = base + (size_t)wpb * L.per;
  return L;
}
// ... four-vector families (AcSensSys, AcArnoldiSys): lds_ac's regions in lds_ac's order, then xf (n): the forward solution, which has to outlive the adjoint
// column that runs in x / r / y -- 16 (nnz_lu + 4 n) bytes per system
template <class P> struct LdsAcSens { P lu, x, r, y, xf, end; int per; };   // per: doubles of one system
template <class P> LDS_HD LdsAcSens<P> lds_ac_sens(P base, int nnz_lu, int n, int w, int wpb) {
  LdsAcSens<P> L;
  L.per = 2 * (nnz_lu + 4 * n);
  L.lu = base + (size_t)w * L.per;
  L.x = L.lu + 2 * (size_t)nnz_lu; L.r = L.x + 2 * (size_t)n; L.y = L.r + 2 * (size_t)n; L.xf = L.y + 2 * (size_t)n;
  L.end = base + (size_t)wpb * L.per;
  return L;
}
template <class L> LDS_HD size_t lds_bytes(const L& l) { return (size_t)l.end * 8; }   // of a layout taken from base (size_t)0

#ifdef __HIPCC__
void set_last_error(const char* what, hipError_t e);   // api.hip (declared here too: this header stands alone, whatever includes it first)
// launch `kernel` with `shmem` bytes of dynamic LDS, opting in to more than LDS_OPTIN first
template <class K, class... A>
static int lds_launch(K kernel, int grid, int threads, size_t shmem, hipStream_t stream, const A&... args) {
  if (shmem > LDS_OPTIN)
    if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)) {
      set_last_error("hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize)", e);
      return CADNIP_HIPERROR;
    }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), shmem, stream, args...);
  return CADNIP_OK;
}
// the kernels are instantiated for 1, 2, 4, 8 waves per workgroup: fn(std::integral_constant<int, W>) for the one that matches
template <class F>
static int with_wpb(int wpb, F&& fn) {
  return wpb == 8 ? fn(std::integral_constant<int, 8>()) : wpb == 4 ? fn(std::integral_constant<int, 4>())
       : wpb == 2 ? fn(std::integral_constant<int, 2>()) : fn(std::integral_constant<int, 1>());
}
#endif

}  // namespace cadnip
