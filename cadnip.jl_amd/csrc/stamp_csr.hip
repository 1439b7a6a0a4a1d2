// stamp_csr.hip -- the per-op stamping kernels: one kernel per device type that evaluates the devices AND reduces their
// contributions into the CSR arrays G, C and b.  ≡ reset_direct_stamp! + the builder pass + the deferred-b / srcFact /
// gshunt steps of fast_rebuild! (/root/reference/src/mna/precompile.jl:493-537, value_only.jl:238-261, 395-478).
//
// One 64-lane wave owns a *tile*: one chunk of (up to 64) devices of one type, for one sweep instance (several instances when
// the type has few devices).  Phases of a tile:
//   1. stamp   -- every lane evaluates its device (coalesced reads of its parameter rows, node voltages from the instance's
//                 u) and stages its per-element contributions in LDS, slot-major ([slot][device]: conflict-free writes).
//   2. reduce  -- segmented reduction in LDS: the tile's *targets* (the CSR entries of G / C and the rows of b that receive
//                 anything from this chunk, in CSR order) are dealt to the lanes; a lane sums its target's staged
//                 contributions in the reference's COO order (nzval[map[pos]] += v, value_only.jl:414-418, addition for
//                 addition) and writes ONE value to HBM.  Consecutive lanes write consecutive CSR positions.  A target
//                 with more than five contributions (node diagonals, supply rails) is reduced as a 5-ary tree over
//                 consecutive runs of its list: partial sums go to LDS scratch words and are combined on the next level,
//                 so no lane ever walks a long list alone (one lane summing the 120 stamps of a rail made the whole wave
//                 wait 40 k cycles).
// No slot buffer in HBM, no separate assemble pass, no zero-fill of G / C / b: a target whose contributions all come from
// one tile is stored; a target that an earlier kernel of the stream has already stored is read-modify-written (kernels of a
// stream run in order, and within this kernel the tile is its only writer); only a target that receives contributions from
// several tiles of the SAME kernel -- a boundary between tiles, e.g. a supply rail fed by every chunk of a large circuit --
// is accumulated with a global fp64 atomic, on a word that k_stamp_prep has pre-set when no earlier kernel stores it.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "stamp_csr_kernel.hpp"   // CsrStampArgs, LdsOut, k_stamp_csr<TYPE, EXT>
#include "stamp_plan.hpp"         // the plan the kernel follows and its launch geometry (host only)

namespace cadnip {

// Pre-set words: (a) targets accumulated with atomics whose first contributions come from that same kernel, (b) diagonal
// entries of voltage nodes that no device stamps into G (a node held by capacitors only): they carry gshunt alone.
struct PrepArgs { const unsigned* words; int n_words; const unsigned char* diag_flag; const double* gshunt; const int* active; double *G, *C, *b; int B, n, nnz; };
__global__ void __launch_bounds__(256) k_stamp_prep(PrepArgs a) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)a.B * a.n_words) return;
  const int inst = (int)(tid / a.n_words);
  if (!a.active[inst]) return;
  const unsigned w = a.words[tid - (long)inst * a.n_words];
  const unsigned e = w & 0x0FFFFFFFu, arr = (w >> 28) & 3u;
  double v = 0.0;
  if (arr == 0u && a.diag_flag[e]) v = a.gshunt[inst];
  double* dst = arr == 0u ? a.G + (size_t)inst * a.nnz + e : arr == 1u ? a.C + (size_t)inst * a.nnz + e : a.b + (size_t)inst * a.n + e;
  *dst = v;
}

// ------------------------------------------------------------------------------------------
// host: the plan (stamp_plan.hpp), built and uploaded once per structure (cadnip_create)
// ------------------------------------------------------------------------------------------
static_assert(sizeof(StampRec) == sizeof(uint4) && offsetof(StampRec, x) == offsetof(uint4, x) && offsetof(StampRec, y) == offsetof(uint4, y) &&
              offsetof(StampRec, z) == offsetof(uint4, z) && offsetof(StampRec, w) == offsetof(uint4, w), "a record is one uint4 of the kernel");

template <class D, class T> static int upload_vec(D** p, const std::vector<T>& v) {
  static_assert(sizeof(D) == sizeof(T), "element types of the same layout");
  HIP_TRY(hipMalloc((void**)p, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIP_TRY(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return CADNIP_OK;
}

static StampBlock stamp_block_of(const DeviceBlock& b) { return StampBlock{b.type, b.count, b.n_g, b.n_c, b.n_b, b.g_base, b.c_base, b.b_base, b.va_tl}; }

// (every pointer lands in the handle as soon as it is allocated: cadnip_destroy releases a handle whose build failed half way)
int build_stamp_plan(CadnipHandle* h, const CadnipStructure* s) {
  std::vector<StampBlock> blocks;
  for (const DeviceBlock& b : h->blocks) blocks.push_back(stamp_block_of(b));
  StampPlans plans;
  TRY_RC(stamp_plan_build(*s, blocks, plans));
  for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
    DeviceBlock& b = h->blocks[bi];
    b.sp_cs = plans.block[bi].tiling.cs; b.sp_chunks = plans.block[bi].tiling.chunks;
    for (int v = 0; v < 2; ++v) {
      const StampPlan& P = plans.block[bi].plan[v];
      if (P.empty()) continue;
      DeviceBlock::PlanSet& D = b.plan[v];
      D.shape = P;
      TRY_RC(upload_vec(&D.tptr, P.tptr));
      TRY_RC(upload_vec(&D.info, P.info));
      TRY_RC(upload_vec(&D.rec, P.rec));
      if (!P.rowoff.empty()) TRY_RC(upload_vec(&D.rowoff, P.rowoff));
    }
  }
  h->n_prep_atomic = plans.n_prep_atomic;
  h->n_prep = (int)plans.prep.size();
  if (h->n_prep) TRY_RC(upload_vec(&h->d_prep, plans.prep));
  return CADNIP_OK;
}

// The external generated models: one translation unit each (va_ext/<module>.hip, written by va/hipgen.py) with the model's own
// instantiation of k_stamp_csr and of its setup kernel; reached through these tables (model id - CADNIP_VA_NBUILTIN).
#define X(i, nm) int va_ext_stamp_launch_##nm(const CsrStampArgs&, unsigned, size_t, hipStream_t); int va_ext_setup_launch_##nm(const VaSetupArgs&, hipStream_t);
CADNIP_VA_EXT_LIST(X)
#undef X
typedef int (*VaExtStampFn)(const CsrStampArgs&, unsigned, size_t, hipStream_t);
typedef int (*VaExtSetupFn)(const VaSetupArgs&, hipStream_t);
#define X(i, nm) va_ext_stamp_launch_##nm,
static const VaExtStampFn VA_EXT_STAMP[CADNIP_VA_NEXT + 1] = {CADNIP_VA_EXT_LIST(X) nullptr};
#undef X
#define X(i, nm) va_ext_setup_launch_##nm,
static const VaExtSetupFn VA_EXT_SETUP[CADNIP_VA_NEXT + 1] = {CADNIP_VA_EXT_LIST(X) nullptr};
#undef X

int launch_va_setup(CadnipHandle* h, DeviceBlock& b) {
  if (b.n_cache <= 0 || !b.d_cache) return CADNIP_OK;
  const int ext = b.va_model - CADNIP_VA_NBUILTIN;
  if (ext < 0 || ext >= CADNIP_VA_NEXT) return CADNIP_BADARG;
  VaSetupArgs a{b.d_nodes, b.d_ipar, b.d_par, h->d_wave, b.d_cache, h->B, b.count, b.n_par, b.n_cache, h->spec.mode};
  int rc = VA_EXT_SETUP[ext](a, h->stream);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

template <int TYPE>
static int launch_stamp_csr_pass(CadnipHandle* h, DeviceBlock& b, bool dump_only) {
  const int nslots = b.n_g + b.n_c + b.n_b;
  const bool pair = TYPE == CADNIP_DEV_MOS1 && b.mos1_plain;
  const DeviceBlock::PlanSet& P = b.plan[pair ? 1 : 0];   // the plan in force
  static const size_t lds_pad = getenv("CADNIP_SC_PAD") ? (size_t)atol(getenv("CADNIP_SC_PAD")) : 0;        // experiments: occupancy as a function of the LDS request
  const StampGeom g = stamp_geometry(stamp_block_of(b), StampTiling{b.sp_cs, b.sp_chunks}, P.shape, h->B, h->n, pair, dump_only, lds_pad);
  CsrStampArgs a{b.d_nodes, b.d_ipar, b.d_par, h->d_wave, h->d_u, h->d_t, h->d_active, h->d_cold, h->d_G, h->d_C, h->d_b, h->d_limit_w, h->d_nonfinite,
                 h->d_diag_flag, h->d_gshunt, h->d_srcfact, P.tptr, P.info, P.rec,
                 h->B, b.count, h->n, h->nnz, b.n_par, b.n_g, b.n_c, b.n_b, b.sp_cs, b.sp_chunks, g.ipw, g.lpd, h->spec.mode, h->initjct,
                 stamp_packs(TYPE) ? 1 : 0, P.shape.levels, P.shape.scratch, g.u_lds,
                 b.d_cache, b.n_cache, dump_only ? h->d_dump : nullptr, h->ns, b.g_base, h->ns_g + b.c_base, h->ns_g + h->ns_c + b.b_base,
                 dump_only ? nullptr : P.rowoff, g.rows, dump_only ? 1 : 0};
  if (getenv("CADNIP_SC_DEBUG")) fprintf(stderr, "[cadnip stamp] type %d count %d cs %d chunks %d ipw %d lpd %d slots %d rows %d scratch %d tile_words %zu shmem %zu grid %u levels %d u_lds %d%s\n",
                                         TYPE, b.count, b.sp_cs, b.sp_chunks, g.ipw, g.lpd, nslots, g.rows, P.shape.scratch, g.tile_words, g.shmem, g.grid, P.shape.levels, g.u_lds, dump_only ? " (read-out pass)" : "");
  if (TYPE == CADNIP_DEV_VA && b.va_tl) {           // external model: its own kernel (va_ext/<module>.hip)
    const int ext = b.va_model - CADNIP_VA_NBUILTIN;
    if (ext < 0 || ext >= CADNIP_VA_NEXT) return CADNIP_BADARG;
    return VA_EXT_STAMP[ext](a, g.grid, g.shmem, h->stream);
  }
  return launch_stamp_kernel<TYPE>(a, g.grid, g.shmem, h->stream);
}

// The stamping pass of one block; with the operating-point read-out armed (cadnip_get_contributions), a second pass that stages every
// slot -- also those no target reads: the current into a grounded terminal is one of them -- and writes them out instead of reducing.
template <int TYPE>
static int launch_stamp_csr_t(CadnipHandle* h, DeviceBlock& b) {
  int rc = launch_stamp_csr_pass<TYPE>(h, b, false);
  if (!rc && h->d_dump) rc = launch_stamp_csr_pass<TYPE>(h, b, true);
  return rc;
}

// device type -> its profile name and the launcher of its kernel instantiation, in the order of CadnipDeviceType
struct StampType { int type; const char* prof; int (*launch)(CadnipHandle*, DeviceBlock&); };
#define ROW(T, NAME) {T, NAME, launch_stamp_csr_t<T>}
static const StampType STAMP_TYPES[] = {
    ROW(CADNIP_DEV_RESISTOR, "stamp_resistor"), ROW(CADNIP_DEV_CAPACITOR, "stamp_capacitor"), ROW(CADNIP_DEV_INDUCTOR, "stamp_inductor"),
    ROW(CADNIP_DEV_VSOURCE, "stamp_vsource"), ROW(CADNIP_DEV_ISOURCE, "stamp_isource"), ROW(CADNIP_DEV_VCVS, "stamp_vcvs"), ROW(CADNIP_DEV_VCCS, "stamp_vccs"),
    ROW(CADNIP_DEV_CCVS, "stamp_ccvs"), ROW(CADNIP_DEV_CCCS, "stamp_cccs"), ROW(CADNIP_DEV_DIODE, "stamp_diode"), ROW(CADNIP_DEV_DIODECAP, "stamp_diodecap"),
    ROW(CADNIP_DEV_SIMPLEMOS, "stamp_simplemos"), ROW(CADNIP_DEV_MOS1, "stamp_mos1"), ROW(CADNIP_DEV_BVSOURCE, "stamp_bvsource"),
    ROW(CADNIP_DEV_BISOURCE, "stamp_bisource"), ROW(CADNIP_DEV_VA, "stamp_va")};
#undef ROW
static_assert(sizeof(STAMP_TYPES) / sizeof(STAMP_TYPES[0]) == CADNIP_DEV_NTYPES, "one row per device type");
static const StampType* stamp_type(int type) {
  return type >= 0 && type < CADNIP_DEV_NTYPES && STAMP_TYPES[type].type == type ? &STAMP_TYPES[type] : nullptr;
}

// one stamping kernel alone (bench.py times it back to back for the stamp-kernel roofline line)
int launch_stamp_block(CadnipHandle* h, int block) {
  if (block < 0 || block >= (int)h->blocks.size() || h->blocks[block].count == 0) return CADNIP_BADARG;
  const StampType* t = stamp_type(h->blocks[block].type);
  return t ? t->launch(h, h->blocks[block]) : CADNIP_BADARG;
}

int launch_rebuild(CadnipHandle* h) {
  // the pre-set pass runs when some word is accumulated with atomics from scratch; the unstamped node diagonals carry
  // gshunt alone, so they are rewritten only while a homotopy is on and once after it has been switched off
  const bool prep_now = h->n_prep_atomic > 0 || (h->n_prep > 0 && (h->homotopy || h->spec.gshunt != 0.0 || h->prep_stale));
  h->prep_stale = h->n_prep > h->n_prep_atomic && (h->homotopy || h->spec.gshunt != 0.0);
  if (prep_now) {
    ProfScope ps(h, "stamp_prep");
    PrepArgs p{h->d_prep, h->n_prep, h->d_diag_flag, h->d_gshunt, h->d_active, h->d_G, h->d_C, h->d_b, h->B, h->n, h->nnz};
    const long total = (long)h->B * h->n_prep;
    hipLaunchKernelGGL(k_stamp_prep, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, p);
  }
  for (auto& blk : h->blocks) {
    if (blk.count == 0) continue;
    const StampType* t = stamp_type(blk.type);
    if (!t) return CADNIP_BADARG;
    ProfScope ps(h, t->prof);
    TRY_RC(t->launch(h, blk));
  }
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

}  // namespace cadnip

#ifdef CADNIP_TRACE
extern "C" int cadnip_debug_stamp_trace(unsigned long long* sum8, unsigned long long* cnt, int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return CADNIP_HIPERROR;
  if (hipMemcpyFromSymbol(sum8, HIP_SYMBOL(cadnip::g_sc_sum), 8 * sizeof(unsigned long long)) != hipSuccess) return CADNIP_HIPERROR;
  if (hipMemcpyFromSymbol(cnt, HIP_SYMBOL(cadnip::g_sc_cnt), sizeof(unsigned long long)) != hipSuccess) return CADNIP_HIPERROR;
  if (reset) { unsigned long long z[9] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(cadnip::g_sc_sum), z, 64); (void)hipMemcpyToSymbol(HIP_SYMBOL(cadnip::g_sc_cnt), z, 8); }
  return CADNIP_OK;
}
#endif
