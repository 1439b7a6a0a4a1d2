// stamp_plan.hpp -- the plan that the per-op stamping kernel k_stamp_csr executes (stamp_csr_kernel.hpp; design: stamp_csr.hip), as
// host-only combinatorics: tile geometry, packed row offsets, reduction records and their 5-ary trees, the step list, the pre-set words
// of k_stamp_prep, and the launch geometry.  The kernel does no index arithmetic of its own; everything it follows is decided here.
// No HIP, no handle: stamp_csr.hip describes the handle's blocks (StampBlock), calls stamp_plan_build once per structure and uploads
// the vectors; its launcher sizes every launch with stamp_geometry.  tests/test_stamp_plan_cpu.py compiles this header with the host
// compiler, interprets the tables the way the kernel's reduce loop does and holds them against the digests of the tables the
// library uploaded before the header existed.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <vector>
#include "../../include/cadnip_hip.h"

namespace cadnip {

// ---- the record encoding, shared with the kernel ---------------------------------------------------------------------------
// target word: bits 30-31 mode, bits 28-29 array (0 G, 1 C, 2 b), bits 0-27 index -- the CSR position / row, or for TGT_PARTIAL the
// LDS scratch word of the tile (relative to the tile)
enum { TGT_STORE = 0, TGT_RMW = 1, TGT_ATOMIC = 2, TGT_PARTIAL = 3 };
constexpr unsigned TGT_MODE_SHIFT = 30, TGT_ARR_SHIFT = 28, TGT_INDEX_MASK = 0x0FFFFFFFu;
constexpr unsigned tgt_word(unsigned mode, unsigned arr, unsigned index) { return (mode << TGT_MODE_SHIFT) | (arr << TGT_ARR_SHIFT) | index; }
// record = {target word, count | off0 << 16, off1 | off2 << 16, off3 | off4 << 16}: up to five operands (word offsets into the tile)
// inline; an operand slot that is not used reads the tile's zero word; count 0 = padding inside a step (writes nothing)
struct StampRec { unsigned x, y, z, w; };
// record classes: 0 / 1 / 2 = sole writer of a word of G / C / b (TGT_STORE), 3 = partial sum into LDS scratch, 4 = the rest
// (TGT_RMW, TGT_ATOMIC), 5 = a step of padding alone (an empty level still fences)
constexpr int N_CLS = 5;
constexpr int CLS_PARTIAL = 3, CLS_SHARED = 4, CLS_PAD = 5;
constexpr int tgt_class(unsigned word) {
  return (word >> TGT_MODE_SHIFT) == TGT_PARTIAL ? CLS_PARTIAL : (word >> TGT_MODE_SHIFT) == TGT_STORE ? (int)((word >> TGT_ARR_SHIFT) & 3u) : CLS_SHARED;
}
constexpr int STEP_W = 128;   // records per reduction step (two per lane); every step is homogeneous in (level, class)
// step-info word: class | STEP_NEW_LEVEL on the first step of every level above 0 (the partial sums below it are complete)
constexpr int STEP_CLS_MASK = 0xFF, STEP_NEW_LEVEL = 0x100;

// ---- sp_mos1: slots whose value is zero whatever the parameters ------------------------------------------------------------
// Slot indices follow the stamp order of stamp_mos1 (devices.hpp): G = 12 g_lim entries | 6 branch rows (d, g, s, b, d_int, s_int) of
// 6 columns each (same order) | 4 charge rows (q_g, q_b, q_dint, q_sint) of 7 (the unit diagonal, then -CS dq per column);
// C = 4 charge-state entries | 4 charge rows of 6 columns (dq: the linear form); b = 6 branch rows | 4 charge rows.
constexpr int MOS1_N_G = 76, MOS1_N_C = 28, MOS1_N_B = 10;
enum { MOS1_COL_D = 0, MOS1_COL_G, MOS1_COL_S, MOS1_COL_B, MOS1_COL_DINT, MOS1_COL_SINT, MOS1_N_COL };
constexpr int mos1_g_branch(int br, int col) { return 12 + MOS1_N_COL * br + col; }            // dI(br) / dV(col)
constexpr int mos1_g_charge(int r, int col) { return 48 + (MOS1_N_COL + 1) * r + 1 + col; }    // -CS dq(r) / dV(col)   (gq[1 + col])
constexpr int mos1_c_charge(int r, int col) { return 4 + MOS1_N_COL * r + col; }               // dq(r) / dV(col)
constexpr int mos1_b_branch(int br) { return br; }
// ... always: no charge depends on the external d and s terminals (dq[0] = dq[2] = 0);
// ... on the lane-pair path (stamp_mos1_pair: gd = gs = OxideCap = 0) also the KCL rows of the external d, g, s terminals (Ir[0..2] = 0:
// their G rows and b entries) and, in the rows of b, d_int, s_int, the d and s columns
static_assert(mos1_g_charge(0, MOS1_COL_D) == 48 + 1 && mos1_g_charge(3, MOS1_COL_S) == 48 + 7 * 3 + 3 && mos1_c_charge(3, MOS1_COL_S) == 4 + 6 * 3 + 2 &&
              mos1_g_branch(0, 0) == 12 && mos1_g_branch(2, 5) == 29 && mos1_g_branch(5, MOS1_COL_S) == 12 + 6 * 5 + 2 && mos1_g_charge(3, 5) == MOS1_N_G - 1 &&
              mos1_c_charge(3, 5) == MOS1_N_C - 1, "sp_mos1 slot order (devices.hpp: stamp_mos1)");

// ---- inputs ----------------------------------------------------------------------------------------------------------------
// what the plan reads of a device block (the gather lists and sizes come from the CadnipStructure itself; its ranges are checked by
// cadnip_create).  va_tl: lanes per device of a generated external model (0: none)
struct StampBlock { int type, count, n_g, n_c, n_b, g_base, c_base, b_base, va_tl; };

// ---- outputs ---------------------------------------------------------------------------------------------------------------
struct StampTiling { int cs = 0, chunks = 0; };                  // devices per tile, tiles per instance
struct StampShape { int rows = 0, levels = 1, scratch = 0; };    // staged rows of a tile, levels of the deepest tree, scratch words (zero word included)
struct StampPlan : StampShape {
  std::vector<int> tptr, info;             // [chunks + 1] step range of every chunk | per step: class | STEP_NEW_LEVEL
  std::vector<StampRec> rec;               // STEP_W records per step
  std::vector<unsigned short> rowoff;      // [n_g + n_c + n_b] word offset of every slot's row inside a tile; empty: one row per slot, in order
  bool empty() const { return tptr.empty(); }
};
// plan[0]: the general plan; plan[1]: the lane-pair plan of an sp_mos1 block (fewer live rows), empty for every other type.  Both
// are empty for a block without devices.
struct StampBlockPlan { StampTiling tiling; StampPlan plan[2]; };
struct StampPlans {
  std::vector<StampBlockPlan> block;
  // words k_stamp_prep pre-sets: the first n_prep_atomic are accumulated with atomics and stored by nobody first, the rest are node
  // diagonals of G that no device stamps (they carry gshunt alone); word = array << 28 | index
  std::vector<unsigned> prep; int n_prep_atomic = 0;
};

// types whose plan packs its rows (k_stamp_csr: REMAP): many slots, many of them without a target.  The small types keep one row
// per slot, addressed arithmetically
constexpr bool stamp_packs(int type) { return type == CADNIP_DEV_MOS1 || type == CADNIP_DEV_VA; }

namespace stamp_plan_detail {

constexpr unsigned short ROW_ZERO = 0xFFFEu, ROW_NONE = 0xFFFFu;   // a slot that is structurally zero | a slot no target reads
constexpr unsigned OFF_ZERO = 0xFFFFu;     // operand that reads the tile's zero word: a structural zero or an unused slot of a record (patched once the
                                           // scratch words are counted; real offsets stay below 65535)
struct Src { unsigned short slot, ldev; };                            // a contribution: slot of the block (G, C, b slots in one range), device within its chunk
struct Target { int chunk; unsigned word; size_t first, count; };     // its contributions [first, first + count) in `src`, in gather-list order
struct BlockTargets { std::vector<char> live; std::vector<Target> tgt; std::vector<Src> src; };

// Rows of a tile.  A tile stages [row][device]; only the slots that some target reads need a row of their own (a stamp into a ground
// row / column has no target, nor has the unused form -- charge state or linear -- of a reactive branch): they are packed, every other
// slot writes into one shared trash row, and a slot whose value is structurally zero is read from the tile's zero word.  Fewer rows =
// less LDS per wave = more waves per CU: the kernel's duration follows its occupancy.
inline int rows_of(const StampBlock& b, int cs, const std::vector<char>& live, bool pair, std::vector<unsigned short>& row, StampPlan& P) {
  row.assign(live.size(), ROW_NONE);
  for (size_t k = 0; k < live.size(); ++k) if (live[k]) row[k] = 0;
  auto zero = [&](int k) { if (row[(size_t)k] != ROW_NONE) row[(size_t)k] = ROW_ZERO; };
  if (b.type == CADNIP_DEV_MOS1) {
    if (b.n_g != MOS1_N_G || b.n_c != MOS1_N_C || b.n_b != MOS1_N_B) return CADNIP_BADARG;
    for (int r = 0; r < 4; ++r)
      for (int col : {MOS1_COL_D, MOS1_COL_S}) { zero(mos1_g_charge(r, col)); zero(b.n_g + mos1_c_charge(r, col)); }
    if (pair) {
      for (int br = 0; br < 3; ++br) {
        for (int col = 0; col < MOS1_N_COL; ++col) zero(mos1_g_branch(br, col));
        zero(b.n_g + b.n_c + mos1_b_branch(br));
      }
      for (int br = 3; br < 6; ++br) for (int col : {MOS1_COL_D, MOS1_COL_S}) zero(mos1_g_branch(br, col));
    }
  }
  if (!stamp_packs(b.type)) {                           // one row per slot, no table
    for (size_t k = 0; k < row.size(); ++k) row[k] = (unsigned short)k;
    P.rows = (int)row.size();
    return CADNIP_OK;
  }
  int rows = 0;
  for (auto& r : row) if (r == 0) r = (unsigned short)rows++;
  P.rows = rows + 1;                                    // + the trash row
  if ((size_t)P.rows * cs > 65000) return CADNIP_BADARG;   // 16-bit staging offsets
  P.rowoff.resize(row.size());
  for (size_t k = 0; k < row.size(); ++k) P.rowoff[k] = (unsigned short)((row[k] >= ROW_ZERO ? rows : row[k]) * cs);
  return CADNIP_OK;
}

// Records and steps of one block.  A target with more than five contributions becomes a 5-ary tree: level-0 records sum consecutive
// runs of five staged words into scratch words of the tile, the next level combines five of those, ... until one record is left, which
// carries the target's real destination.  Records are grouped per chunk and level; steps are runs of STEP_W records within one
// (level, class), a short last step of a group padded with count-0 records that sum the zero word and write nothing.
inline int records_of(const BlockTargets& T, const std::vector<unsigned short>& row, const StampTiling& t, StampPlan& P) {
  const int stage_words = P.rows * t.cs;
  struct Rec { int chunk, level, cls; StampRec r; };
  std::vector<Rec> recs;
  std::vector<int> scratch_used((size_t)t.chunks, 0);
  int n_levels = 1;
  auto pack = [](unsigned word, const unsigned* o, unsigned cnt) {
    unsigned v[5] = {OFF_ZERO, OFF_ZERO, OFF_ZERO, OFF_ZERO, OFF_ZERO};
    for (unsigned i = 0; i < cnt; ++i) v[i] = o[i];
    return StampRec{word, cnt | (v[0] << 16), v[1] | (v[2] << 16), v[3] | (v[4] << 16)};
  };
  std::vector<unsigned> cur, next;
  for (const Target& tg : T.tgt) {
    cur.clear();
    for (size_t i = tg.first; i < tg.first + tg.count; ++i) {
      const unsigned short r = row[T.src[i].slot];
      cur.push_back(r == ROW_ZERO ? OFF_ZERO : (unsigned)(unsigned short)(r * t.cs + T.src[i].ldev));
    }
    int level = 0;
    while (cur.size() > 5) {
      next.clear();
      for (size_t i = 0; i < cur.size(); i += 5) {
        const unsigned cnt = (unsigned)std::min<size_t>(5, cur.size() - i);
        if (cnt == 1) { next.push_back(cur[i]); continue; }             // a lone tail word moves up as it is
        const unsigned so = (unsigned)(stage_words + scratch_used[(size_t)tg.chunk]++);
        recs.push_back(Rec{tg.chunk, level, CLS_PARTIAL, pack(tgt_word(TGT_PARTIAL, 0, so), &cur[i], cnt)});
        next.push_back(so);
      }
      cur.swap(next);
      ++level;
    }
    recs.push_back(Rec{tg.chunk, level, tgt_class(tg.word), pack(tg.word, cur.data(), (unsigned)cur.size())});
    n_levels = std::max(n_levels, level + 1);
  }
  int n_scratch = 0;
  for (int u : scratch_used) n_scratch = std::max(n_scratch, u);
  n_scratch += 1;                                                         // + the tile's zero word (its last word)
  if ((stage_words + n_scratch) & 1) n_scratch += 1;                      // tiles stay 16-byte aligned (zeroing uses 16-byte stores)
  if ((size_t)stage_words + n_scratch >= 65535) return CADNIP_BADARG;
  const unsigned zo = (unsigned)(stage_words + n_scratch - 1);
  auto fix = [&](unsigned half) { return half == OFF_ZERO ? zo : half; };
  for (Rec& rc : recs) {
    StampRec& r = rc.r;
    r.y = (r.y & 0xFFFFu) | (fix(r.y >> 16) << 16);
    r.z = fix(r.z & 0xFFFFu) | (fix(r.z >> 16) << 16);
    r.w = fix(r.w & 0xFFFFu) | (fix(r.w >> 16) << 16);
  }
  std::stable_sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) { return x.chunk != y.chunk ? x.chunk < y.chunk : x.level != y.level ? x.level < y.level : x.cls < y.cls; });
  const StampRec padrec{0u, zo << 16, zo | (zo << 16), zo | (zo << 16)};
  P.tptr.assign((size_t)t.chunks + 1, 0);
  size_t k = 0;
  for (int c = 0; c < t.chunks; ++c) {
    P.tptr[(size_t)c] = (int)P.info.size();
    for (int l = 0; l < n_levels; ++l) {
      bool first_of_level = l > 0;
      for (int cls = 0; cls < N_CLS; ++cls) {
        size_t k1 = k;
        while (k1 < recs.size() && recs[k1].chunk == c && recs[k1].level == l && recs[k1].cls == cls) ++k1;
        for (size_t p = k; p < k1; p += STEP_W) {
          P.info.push_back(cls | (first_of_level ? STEP_NEW_LEVEL : 0));
          first_of_level = false;
          for (size_t j = p; j < p + STEP_W; ++j) P.rec.push_back(j < k1 ? recs[j].r : padrec);
        }
        k = k1;
      }
      if (first_of_level) { P.info.push_back(CLS_PAD | STEP_NEW_LEVEL); P.rec.insert(P.rec.end(), (size_t)STEP_W, padrec); }   // an empty level still fences
    }
  }
  P.tptr[(size_t)t.chunks] = (int)P.info.size();
  P.levels = n_levels; P.scratch = n_scratch;
  return CADNIP_OK;
}

}  // namespace stamp_plan_detail

// Everything the stamping kernels of a structure follow, or the error code: CADNIP_BADARG for a gather list that names a slot no block
// owns and for a block beyond the 16-bit staging offsets.
inline int stamp_plan_build(const CadnipStructure& s, const std::vector<StampBlock>& blocks, StampPlans& out) {
  using namespace stamp_plan_detail;
  const size_t nb = blocks.size();
  out = StampPlans();
  out.block.resize(nb);
  std::vector<BlockTargets> T(nb);
  // tile geometry per block
  for (size_t bi = 0; bi < nb; ++bi) {
    const StampBlock& b = blocks[bi];
    if (b.count == 0) continue;
    const int nslots = b.n_g + b.n_c + b.n_b;
    int cs = b.type == CADNIP_DEV_MOS1 ? 32 : 64;                       // sp_mos1: room for two lanes per device
    if (b.type == CADNIP_DEV_VA && b.va_tl) cs = 64 / b.va_tl;           // external models: 16 or 32 direction lanes per device (va_runtime.hpp)
    while (cs > 1 && (size_t)cs * nslots * 8 > 96 * 1024) cs >>= 1;     // big generated models: smaller chunks
    if ((size_t)cs * nslots > 65535) return CADNIP_BADARG;              // 16-bit staging offsets
    StampTiling& t = out.block[bi].tiling;
    if (b.count <= cs) { t.cs = b.count; t.chunks = 1; }
    else { t.cs = cs; t.chunks = (b.count + cs - 1) / cs; }
    T[bi].live.assign((size_t)nslots, 0);
  }
  // the targets of every tile: the contributions of each entry of G and C and each row of b, in COO order, grouped by tile
  const int* ptrs[3] = {s.g_ptr, s.c_ptr, s.b_ptr};
  const int* slots[3] = {s.g_slots, s.c_slots, s.b_slots};
  const int n_tgt[3] = {s.nnz, s.nnz, s.n};
  const int totals[3] = {s.ns_g, s.ns_c, s.ns_b};
  std::vector<unsigned> prep_orphan;
  std::vector<char> is_diag((size_t)s.nnz, 0);
  for (int i = 0; i < s.n_nodes; ++i) if (s.diag_nz[i] >= 0 && s.diag_nz[i] < s.nnz) is_diag[(size_t)s.diag_nz[i]] = 1;
  struct Owner { int blk, slot, dev; };                  // slot of an array -> (block, slot of the block, device); blocks own disjoint ranges
  struct Contrib { int blk, chunk; Src src; };
  std::vector<Owner> own;
  std::vector<Contrib> cl;
  std::vector<int> order;
  for (int arr = 0; arr < 3; ++arr) {
    own.assign((size_t)totals[arr], Owner{-1, 0, 0});
    for (size_t bi = 0; bi < nb; ++bi) {
      const StampBlock& b = blocks[bi];
      if (b.count == 0) continue;
      const int base = arr == 0 ? b.g_base : arr == 1 ? b.c_base : b.b_base, nk = arr == 0 ? b.n_g : arr == 1 ? b.n_c : b.n_b;
      const int k0 = arr == 0 ? 0 : arr == 1 ? b.n_g : b.n_g + b.n_c;
      if (base < 0 || (size_t)base + (size_t)nk * b.count > own.size()) return CADNIP_BADARG;
      for (int k = 0; k < nk; ++k) for (int d = 0; d < b.count; ++d) own[(size_t)base + (size_t)k * b.count + d] = Owner{(int)bi, k0 + k, d};
    }
    for (int e = 0; e < n_tgt[arr]; ++e) {
      cl.clear();
      for (int p = ptrs[arr][e]; p < ptrs[arr][e + 1]; ++p) {
        const int sl = slots[arr][p];
        if (sl < 0 || sl >= totals[arr] || own[(size_t)sl].blk < 0) return CADNIP_BADARG;        // a gather list names a slot no block owns
        const Owner& o = own[(size_t)sl];
        const int cs = out.block[(size_t)o.blk].tiling.cs;
        T[(size_t)o.blk].live[(size_t)o.slot] = 1;
        cl.push_back(Contrib{o.blk, o.dev / cs, Src{(unsigned short)o.slot, (unsigned short)(o.dev % cs)}});
      }
      if (cl.empty()) {
        // a G entry nobody stamps stays zero for ever -- unless it is a node diagonal, which carries gshunt
        if (arr == 0 && is_diag[(size_t)e]) prep_orphan.push_back((unsigned)e);
        continue;
      }
      // group by tile (block, chunk) in launch order; inside a tile the COO order is kept
      order.resize(cl.size());
      for (size_t i = 0; i < cl.size(); ++i) order[i] = (int)i;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cl[x].blk != cl[y].blk ? cl[x].blk < cl[y].blk : cl[x].chunk < cl[y].chunk; });
      const int first_blk = cl[order[0]].blk;
      for (size_t i = 0; i < order.size();) {
        const int blk = cl[order[i]].blk, chunk = cl[order[i]].chunk;
        BlockTargets& bt = T[(size_t)blk];
        size_t j = i;
        const size_t first = bt.src.size();
        while (j < order.size() && cl[order[j]].blk == blk && cl[order[j]].chunk == chunk) bt.src.push_back(cl[order[j++]].src);
        // does another tile of the same kernel contribute too?
        const bool shared_in_kernel = (i > 0 && cl[order[i - 1]].blk == blk) || (j < order.size() && cl[order[j]].blk == blk);
        const unsigned mode = shared_in_kernel ? TGT_ATOMIC : (blk == first_blk ? TGT_STORE : TGT_RMW);
        if (mode == TGT_ATOMIC && blk == first_blk && i == 0) out.prep.push_back(tgt_word(0, (unsigned)arr, (unsigned)e));   // nobody stores it first
        bt.tgt.push_back(Target{chunk, tgt_word(mode, (unsigned)arr, (unsigned)e), first, j - i});
        i = j;
      }
    }
  }
  out.n_prep_atomic = (int)out.prep.size();
  out.prep.insert(out.prep.end(), prep_orphan.begin(), prep_orphan.end());
  // per block: targets grouped by chunk (stable: array, then CSR position); rows and records per variant
  std::vector<unsigned short> row;
  for (size_t bi = 0; bi < nb; ++bi) {
    const StampBlock& b = blocks[bi];
    if (b.count == 0) continue;
    std::stable_sort(T[bi].tgt.begin(), T[bi].tgt.end(), [](const Target& x, const Target& y) { return x.chunk < y.chunk; });
    for (int pair = 0; pair < (b.type == CADNIP_DEV_MOS1 ? 2 : 1); ++pair) {
      StampPlan& P = out.block[bi].plan[pair];
      int rc = rows_of(b, out.block[bi].tiling.cs, T[bi].live, pair != 0, row, P);
      if (!rc) rc = records_of(T[bi], row, out.block[bi].tiling, P);
      if (rc) return rc;
    }
  }
  return CADNIP_OK;
}

// ---- the launch geometry of one stamping pass (the analogue of launch_plan.hpp / ac_lu_plan) ------------------------------------
// pair: the lane-pair path of an sp_mos1 block (plan[1]); readout: the operating-point read-out pass, which stages every slot in a
// row of its own; pad: extra LDS bytes (experiments: occupancy as a function of the LDS request).
// The dynamic LDS block, as the kernel carves it: ipw tiles (staged rows + tree scratch) | 3 scalars per instance | u of the tile's
// instances when u_lds | the slots' row offsets (16 bit each, rounded up to 8 bytes).
struct StampGeom { int lpd, rows, ipw, u_lds; size_t tile_words, shmem; unsigned grid; };
inline StampGeom stamp_geometry(const StampBlock& b, const StampTiling& t, const StampShape& p, int B, int n, bool pair, bool readout, size_t pad) {
  StampGeom g;
  const int nslots = b.n_g + b.n_c + b.n_b;
  g.lpd = pair ? 2 : (b.type == CADNIP_DEV_VA && b.va_tl) ? b.va_tl : 1;      // lanes per device
  g.rows = readout ? nslots : p.rows;
  g.ipw = 1;                                                                  // instances per wave
  if (t.chunks == 1) g.ipw = std::min(8, std::max(1, 64 / (b.count * g.lpd)));   // (a wave reduces its instances one after the other: few per wave)
  g.tile_words = (size_t)g.rows * t.cs + p.scratch;
  while (g.ipw > 1 && (size_t)g.ipw * g.tile_words * 8 > 64 * 1024) --g.ipw;
  g.u_lds = (size_t)g.ipw * n * 8 <= 16 * 1024 ? 1 : 0;                       // small circuits: the unknowns of the tile's instances are staged in LDS
  g.shmem = ((size_t)g.ipw * g.tile_words + 3 * (size_t)g.ipw + (g.u_lds ? (size_t)g.ipw * n : 0)) * 8 + (((size_t)nslots * 2 + 7) & ~(size_t)7) + pad;
  g.grid = (unsigned)t.chunks * (unsigned)((B + g.ipw - 1) / g.ipw);
  return g;
}

}  // namespace cadnip
