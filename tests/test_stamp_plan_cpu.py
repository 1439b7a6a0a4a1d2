"""csrc/stamp_plan.hpp -- the plan the per-op stamping kernel k_stamp_csr executes, and its launch geometry -- on the CPU: the header is
compiled with the host compiler and fed the structures of the stamping test circuits through ctypes (no HIP library is loaded).

(a) a Python interpreter of the plan that follows the kernel's reduce loop tile by tile reproduces the exact sum of every gather list;
(b) the leaves of every target's tree, left to right, are its tile's contributions in gather-list order ("addition for addition");
(c) STORE / RMW / ATOMIC and the pre-set words are what the launch order demands; (d) the step list has the shape the kernel relies
on; (e) rows; (f) the launch geometry against the kernel's carving, written out below once as the record of what it was; (g) refusals;
(h) injected faults are rejected; (i) the tables are byte for byte those the library uploaded before the header existed
(tests/golden/stamp_plan_digests.json, recorded from the earlier build_plan_variant wrapped in a host harness)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import benchmarks as bm, hip, structure as S
from tests.circuits import ALL_STAMP, CHAIN_STAMP, TILED_STAMP, rc_charge, tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
DIGESTS = os.path.join(GOLD, "stamp_plan_digests.json")

SHIM = r"""
#include <string.h>
#include "stamp_plan.hpp"
#include "va_generated.hpp"      // (host part: CADNIP_VA_NBUILTIN and the external models' lanes per device, as api.hip reads them)
using namespace cadnip;
struct Built { std::vector<StampBlock> blocks; StampPlans plans; };
extern "C" {
int sp_va_lanes(int model) {
  static const int tl[] = {CADNIP_VA_EXT_TL_LANES 0};
  return model >= CADNIP_VA_NBUILTIN && model < CADNIP_VA_NBUILTIN + CADNIP_VA_NEXT ? tl[model - CADNIP_VA_NBUILTIN] : 0;
}
int sp_const(int i) {
  const int c[] = {STEP_W, N_CLS, TGT_STORE, TGT_RMW, TGT_ATOMIC, TGT_PARTIAL, (int)TGT_MODE_SHIFT, (int)TGT_ARR_SHIFT, (int)TGT_INDEX_MASK, STEP_CLS_MASK,
                   STEP_NEW_LEVEL, CLS_PARTIAL, CLS_SHARED, CLS_PAD, (int)sizeof(StampRec)};
  return c[i];
}
void* sp_build(const CadnipStructure* s, const int* va_tl, int* rc) {
  Built* b = new Built();
  for (int i = 0; i < s->n_blocks; ++i) {
    const CadnipDeviceBlock& sb = s->blocks[i];
    b->blocks.push_back(StampBlock{sb.type, sb.count, sb.n_g, sb.n_c, sb.n_b, sb.g_base, sb.c_base, sb.b_base, va_tl[i]});
  }
  *rc = stamp_plan_build(*s, b->blocks, b->plans);
  if (*rc) { delete b; return nullptr; }
  return b;
}
void sp_free(void* p) { delete (Built*)p; }
// out: cs, chunks, rows, levels, scratch, bytes of tptr, info, rec, rowoff; 0: the block has no such plan
int sp_scalars(void* p, int blk, int v, int* out) {
  const StampBlockPlan& bp = ((Built*)p)->plans.block[blk];
  const StampPlan& P = bp.plan[v];
  if (P.empty()) return 0;
  out[0] = bp.tiling.cs; out[1] = bp.tiling.chunks; out[2] = P.rows; out[3] = P.levels; out[4] = P.scratch;
  out[5] = (int)(P.tptr.size() * sizeof(int)); out[6] = (int)(P.info.size() * sizeof(int)); out[7] = (int)(P.rec.size() * sizeof(StampRec));
  out[8] = (int)(P.rowoff.size() * sizeof(unsigned short));
  return 1;
}
int sp_table(void* p, int blk, int v, int which, void* dst) {
  const StampPlan& P = ((Built*)p)->plans.block[blk].plan[v];
  if (P.empty()) return 0;
  if (which == 0) memcpy(dst, P.tptr.data(), P.tptr.size() * sizeof(int));
  if (which == 1) memcpy(dst, P.info.data(), P.info.size() * sizeof(int));
  if (which == 2) memcpy(dst, P.rec.data(), P.rec.size() * sizeof(StampRec));
  if (which == 3) memcpy(dst, P.rowoff.data(), P.rowoff.size() * sizeof(unsigned short));
  return 1;
}
void sp_prep(void* p, int* n, unsigned* dst) {
  const StampPlans& P = ((Built*)p)->plans;
  n[0] = (int)P.prep.size(); n[1] = P.n_prep_atomic;
  if (dst && !P.prep.empty()) memcpy(dst, P.prep.data(), P.prep.size() * sizeof(unsigned));
}
// out: lpd, rows, ipw, u_lds, tile_words, shmem, grid
void sp_geometry(void* p, int blk, int v, int B, int n, int readout, int pad, long long* out) {
  Built* b = (Built*)p;
  const StampGeom g = stamp_geometry(b->blocks[blk], b->plans.block[blk].tiling, b->plans.block[blk].plan[v], B, n, v != 0, readout != 0, (size_t)pad);
  out[0] = g.lpd; out[1] = g.rows; out[2] = g.ipw; out[3] = g.u_lds; out[4] = (long long)g.tile_words; out[5] = (long long)g.shmem; out[6] = g.grid;
}
}
"""

TABLES = ("tptr", "info", "rec", "rowoff")
BADARG = 1
MOS1, VA = hip.type_id("MOS1"), 15


def load_plan_lib(path):
    L = C.CDLL(path)
    L.sp_build.restype = C.c_void_p
    L.sp_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sp_free.argtypes = [C.c_void_p]
    L.sp_scalars.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sp_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.sp_prep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp_plan")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    L = load_plan_lib(so)
    L.sp_geometry.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    return L


def orphan_circuit():
    """(tests/test_gpu_stamp_kernels.py: _orphan_diag_circuit) one node that only a capacitor touches: its G diagonal carries gshunt alone"""
    return tiled(rc_charge(), 1, cap_node="cq")


def _circuits():
    out = {}
    for name, (mk, params) in dict(ALL_STAMP, **TILED_STAMP, **CHAIN_STAMP).items():
        out[name] = (lambda mk=mk, params=params: cj.discover(mk(), params))
    out["dff_generated"] = lambda: cj.discover(bm.dff_circuit(generated=True), {"vdd": 5.0})
    out["orphan"] = lambda: cj.discover(orphan_circuit(), {})
    out["psp103_ring"] = lambda: S.load_structure(os.path.join(GOLD, "psp103_ring.npz"))[0]
    return out


CIRCUITS = _circuits()
# (the 16 x 16 multiplier c6288 is left out: its structure alone takes 10 s to discover on the CPU)
_ST = {}


def structure(name):
    if name not in _ST:
        _ST[name] = CIRCUITS[name]()
    return _ST[name]


def va_lanes(st, lanes_of):
    """lanes per device of every block: the generated external models' table (va_generated_ext.hpp) by the block's model id (ipar row 0)"""
    return [lanes_of(int(np.asarray(b.ipar)[0][0])) if b.type.startswith("VA:") and b.count else 0 for b in st.blocks]


class Plan:
    """The tables of one structure as the device would receive them."""

    def __init__(self, L, st, lanes, sc=None):
        self.st = st
        s, keep = sc if sc is not None else hip.structure_c(st)
        tl = (C.c_int * max(1, len(lanes)))(*lanes)
        rc = C.c_int(0)
        h = L.sp_build(C.addressof(s), tl, C.addressof(rc))
        self.rc = rc.value
        self.blocks = []          # per block: [variant 0, variant 1] dicts or None
        if not h:
            return
        for bi in range(len(st.blocks)):
            vs = []
            for v in (0, 1):
                out = (C.c_int * 9)()
                if not L.sp_scalars(h, bi, v, out):
                    vs.append(None)
                    continue
                d = dict(zip(("cs", "chunks", "rows", "levels", "scratch"), out[:5]))
                for w, (nm, dt) in enumerate(zip(TABLES, (np.int32, np.int32, np.uint32, np.uint16))):
                    a = np.zeros(out[5 + w] // np.dtype(dt).itemsize, dtype=dt)
                    if a.size:
                        L.sp_table(h, bi, v, w, a.ctypes.data_as(C.c_void_p))
                    d[nm] = a.reshape(-1, 4) if nm == "rec" else a
                vs.append(d)
            self.blocks.append(vs)
        n = (C.c_int * 2)()
        L.sp_prep(h, n, None)
        self.prep = np.zeros(n[0], dtype=np.uint32)
        if n[0]:
            L.sp_prep(h, n, self.prep.ctypes.data_as(C.c_void_p))
        self.n_prep_atomic = n[1]
        L.sp_free(h)

    def digests(self):
        out = {"n_prep": int(self.prep.size), "n_prep_atomic": int(self.n_prep_atomic), "d_prep": hashlib.sha256(self.prep.tobytes()).hexdigest()}
        for bi, vs in enumerate(self.blocks):
            for v, d in enumerate(vs):
                if d is None:
                    continue
                e = {k: int(d[k]) for k in ("cs", "chunks", "rows", "levels", "scratch")}
                for nm in TABLES:
                    e[nm] = [int(d[nm].nbytes), hashlib.sha256(d[nm].tobytes()).hexdigest()]
                out["block%d/%s" % (bi, "pair" if v else "general")] = e
        return out


_PLANS = {}


def plan(lib, name):
    if name not in _PLANS:
        st = structure(name)
        _PLANS[name] = Plan(lib, st, va_lanes(st, lib.sp_va_lanes))
        assert _PLANS[name].rc == 0, name
    return _PLANS[name]


# ---- what the structure says, independently of the plan ---------------------------------------------------------------------
def mos1_zero_slots(blk, pair):
    """Block slots (G, C, b slots in one range) of sp_mos1 that are zero whatever the parameters, from the stamp order of stamp_mos1
    (devices.hpp): G = 12 g_lim | 6 branch rows x 6 columns (d g s b d_int s_int) | 4 charge rows x (1 + 6); C = 4 | 4 charge rows x 6;
    b = 6 branch rows | 4.  No charge depends on V(d), V(s); on the lane-pair path (gd = gs = 0) the rows of the external d, g, s carry
    nothing and no row has an entry in the d / s columns."""
    z = set()
    for r in range(4):
        for col in (0, 2):
            z.add(48 + 7 * r + 1 + col)
            z.add(blk.n_g + 4 + 6 * r + col)
    if pair:
        z |= {12 + 6 * br + col for br in range(3) for col in range(6)} | {blk.n_g + blk.n_c + br for br in range(3)}
        z |= {12 + 6 * br + col for br in range(3, 6) for col in (0, 2)}
    return z


def contributions(st):
    """Per array (G, C, b): for every gather-list position the owning block, the block slot, the device; and the entry it belongs to."""
    out = []
    for arr, (ptr, slots) in enumerate(((st.g_ptr, st.g_slots), (st.c_ptr, st.c_slots), (st.b_ptr, st.b_slots))):
        ptr, s = np.asarray(ptr), np.asarray(slots, dtype=np.int64)
        blk, kk, dev = np.full(s.size, -1), np.zeros(s.size, dtype=np.int64), np.zeros(s.size, dtype=np.int64)
        for bi, b in enumerate(st.blocks):
            if not b.count:
                continue
            base, nk, k0 = ((b.g_base, b.n_g, 0), (b.c_base, b.n_c, b.n_g), (b.b_base, b.n_b, b.n_g + b.n_c))[arr]
            m = (s >= base) & (s < base + nk * b.count)
            blk[m], kk[m], dev[m] = bi, k0 + (s[m] - base) // b.count, (s[m] - base) % b.count
        assert np.all(blk >= 0)
        out.append(dict(ptr=ptr, slots=s, blk=blk, kk=kk, dev=dev, ent=np.repeat(np.arange(ptr.size - 1), np.diff(ptr))))
    return out


def decode(word):
    return int(word) >> 30, (int(word) >> 28) & 3, int(word) & 0x0FFFFFFF


class Rejected(AssertionError):
    pass


def check(cond, *what):
    if not cond:
        raise Rejected(what)


def interpret(st, P, pair, symbolic=False):
    """The launches of one rebuild in order -- pre-set words, then the blocks in order, their chunks in order -- each tile staged and reduced
    the way k_stamp_csr does it: steps in order, the level fence where the flag is set, (((a0 + a1) + a2) + a3) + a4, class 3 writes scratch,
    unused operands read the zero word.  Slot contents are integers (the named structural zeros of sp_mos1 are 0), so every sum is exact.
    Words the kernel never defines (the trash row, scratch before its level is complete, rows of lanes without a device) hold NaN.
    Returns G, C, b (entries nobody writes keep the sentinel) and, per (array, entry, block, chunk), the leaves of the target's tree when
    ``symbolic``.  Checks (c) modes and (d) shape on the way."""
    con = contributions(st)
    rng = np.random.default_rng(7)
    SENT = -7.0
    out = [np.full(st.nnz, SENT), np.full(st.nnz, SENT), np.full(st.n, SENT)]
    for w in P.prep:
        _, arr, e = decode(w)
        out[arr][e] = 0.0                                     # (gshunt = 0)
    finals, leaves = {}, {}
    for bi, blk in enumerate(st.blocks):
        if not blk.count:
            continue
        d = P.blocks[bi][1 if (pair and blk.type == "MOS1") else 0]
        cs, chunks, rows, scratch = d["cs"], d["chunks"], d["rows"], d["scratch"]
        nslots = blk.n_g + blk.n_c + blk.n_b
        packs = blk.type == "MOS1" or blk.type.startswith("VA:")
        stage = rows * cs
        tile_words = stage + scratch
        zero_off = tile_words - 1
        # (d) shape
        check(d["tptr"].size == chunks + 1 and d["tptr"][0] == 0 and d["tptr"][-1] == d["info"].size and np.all(np.diff(d["tptr"]) >= 0), "tptr", bi)
        check(d["rec"].shape[0] == 128 * d["info"].size, "rec size", bi)
        check(tile_words % 2 == 0 and tile_words < 65535, "tile words", bi)
        check((d["rowoff"].size == nslots) if packs else (d["rowoff"].size == 0 and rows == nslots), "rowoff", bi)
        rowoff = d["rowoff"].astype(np.int64) if packs else np.arange(nslots) * cs
        zeros = mos1_zero_slots(blk, pair) if blk.type == "MOS1" else set()
        val = rng.integers(1, 1 << 20, size=(nslots, blk.count)).astype(np.float64)
        for k in zeros:
            val[k, :] = 0.0
        for a in range(3):                                    # the exact sums this block owes every entry
            c = con[a]
            m = c["blk"] == bi
            blk_sum = np.zeros(out[a].size)
            np.add.at(blk_sum, c["ent"][m], val[c["kk"][m], c["dev"][m]])
            d.setdefault("_owed", {})[a] = (blk_sum, np.bincount(c["ent"][m], minlength=out[a].size) > 0)
        got = [np.zeros(o.size) for o in out]
        for chunk in range(chunks):
            ndev = min(cs, blk.count - chunk * cs)
            tile = np.full(tile_words, np.nan)
            if packs:
                tile[:stage] = 0.0                            # zero_first (the scratch words too; NaN here: stricter)
            for k in range(nslots):
                tile[rowoff[k]:rowoff[k] + ndev] = val[k, chunk * cs:chunk * cs + ndev]
            if packs:
                tile[(rows - 1) * cs:stage] = np.nan          # the trash row: whatever was written last
            tile[zero_off] = 0.0
            sym = {}
            if symbolic:
                for k in range(nslots):
                    if packs and rowoff[k] == (rows - 1) * cs:
                        continue
                    for ld in range(ndev):
                        sym[int(rowoff[k]) + ld] = ((k, ld),)
                sym[zero_off] = ()
            s0, s1 = int(d["tptr"][chunk]), int(d["tptr"][chunk + 1])
            level, pending, prev, written = 0, [], None, set()
            flags = d["info"][s0:s1] & 0x100
            check(s1 == s0 or not flags[0], "no fence before level 0", bi, chunk)
            check(int(np.count_nonzero(flags)) == d["levels"] - 1, "one flagged step per level above 0", bi, chunk)
            for q in range(s0, s1):
                info = int(d["info"][q])
                cls = info & 0xFF
                if info & 0x100:
                    for off, v, sy in pending:
                        tile[off] = v
                        written.add(off)
                        if symbolic:
                            sym[off] = sy
                    pending, level, prev = [], level + 1, None
                check(prev is None or cls >= prev, "classes of a level in order", bi, q)
                prev = cls
                R = d["rec"][q * 128:(q + 1) * 128].astype(np.int64)
                cnt = R[:, 1] & 0xFFFF
                offs = np.stack([R[:, 1] >> 16, R[:, 2] & 0xFFFF, R[:, 2] >> 16, R[:, 3] & 0xFFFF, R[:, 3] >> 16], axis=1)
                check(np.all(offs < tile_words), "offset inside the tile", bi, q)
                check(np.all(cnt <= 5), "count", bi, q)
                check(np.all(offs[np.arange(5)[None, :] >= cnt[:, None]] == zero_off), "unused operands read the zero word", bi, q)
                if cls >= 5:
                    check(np.all(cnt == 0) and (info & 0x100), "a padding step is an empty level's fence", bi, q)
                    continue
                on = cnt > 0
                check(on.any(), "a step has a record", bi, q)
                used = offs[np.arange(5)[None, :] < cnt[:, None]]
                check(all(int(o) in written for o in used[(used >= stage) & (used < zero_off)]), "scratch read before a lower level wrote it", bi, q)
                a5 = tile[offs]
                acc = (((a5[:, 0] + a5[:, 1]) + a5[:, 2]) + a5[:, 3]) + a5[:, 4]
                md, arr, e = R[:, 0] >> 30, (R[:, 0] >> 28) & 3, R[:, 0] & 0x0FFFFFFF
                # every record of the step has the step's class
                rc = np.where(md == 3, 3, np.where(md == 0, arr, 4))
                check(np.all(rc[on] == cls), "step homogeneous in class", bi, q)
                for i in np.nonzero(on)[0]:
                    v = acc[i]
                    sy = sum((sym.get(int(o), (("?",),)) for o in offs[i, :cnt[i]]), ()) if symbolic else None
                    if cls == 3:
                        check(stage <= e[i] < zero_off, "scratch word", bi, q)
                        pending.append((int(e[i]), v, sy))
                        continue
                    key = (int(arr[i]), int(e[i]), bi, chunk)
                    check(key not in finals, "one final record per word and tile", key)
                    finals[key] = int(md[i])
                    if symbolic:
                        leaves[key] = sy
                    dst = out[int(arr[i])]
                    if cls < 3:
                        dst[e[i]] = v                         # STORE
                    else:
                        check(md[i] in (1, 2), "mode", key)
                        dst[e[i]] += v                        # RMW | ATOMIC
                    got[int(arr[i])][e[i]] += v
        for a in range(3):
            owed, feeds = d["_owed"][a]
            check(np.array_equal(got[a][feeds], owed[feeds]) and np.all(got[a][~feeds] == 0), "block sums", bi, a)
    # (a) every entry is the sum of its gather list; untouched where nobody stamps; orphan diagonals = the words behind n_prep_atomic
    total = [np.zeros(o.size) for o in out]
    for bi, blk in enumerate(st.blocks):
        if blk.count:
            d = P.blocks[bi][1 if (pair and blk.type == "MOS1") else 0]
            for a in range(3):
                total[a] += d["_owed"][a][0]
    orphans = set()
    dn = np.asarray(st.diag_nz)[:st.n_nodes]
    for a in range(3):
        empty = np.diff(con[a]["ptr"]) == 0
        check(np.array_equal(out[a][~empty], total[a][~empty]), "entry sums", a)
        exp = np.full(out[a].size, SENT)
        if a == 0:
            orphans = {int(p) for p in dn if p >= 0 and empty[p]}
            exp[list(orphans)] = 0.0
        check(np.array_equal(out[a][empty], exp[empty]), "entries nobody stamps", a)
    check({decode(w)[1:] for w in P.prep[P.n_prep_atomic:]} == {(0, p) for p in orphans} and P.prep.size - P.n_prep_atomic == len(orphans), "orphans")
    # (c) modes
    tiles = {}
    for a in range(3):
        c = con[a]
        chunk = c["dev"] // np.array([P.blocks[b][0]["cs"] if P.blocks[b][0] else 1 for b in range(len(st.blocks))])[c["blk"]]
        for key in set(zip([a] * c["ent"].size, c["ent"].tolist(), c["blk"].tolist(), chunk.tolist())):
            tiles.setdefault(key[:2], []).append(key[2:])
    check(set(finals) == {w + t for w, ts in tiles.items() for t in ts}, "a final record per contributing tile")
    prep_atomic = {decode(w)[1:] for w in P.prep[:P.n_prep_atomic]}
    for w, ts in tiles.items():
        first = min(t[0] for t in ts)
        for b, ch in ts:
            shared = sum(1 for t in ts if t[0] == b) > 1
            check(finals[w + (b, ch)] == (2 if shared else 0 if b == first else 1), "mode", w, b, ch)
        check((w in prep_atomic) == (sum(1 for t in ts if t[0] == first) > 1), "pre-set", w)
    check(len(prep_atomic) == P.n_prep_atomic)
    return out, leaves


def check_order(st, P, pair, leaves):
    """(b) the leaves of every target's tree, read left to right, are its tile's contributions in gather-list order; a contribution that
    is a named structural zero reads the zero word (no leaf)."""
    con = contributions(st)
    exp = {}
    for a in range(3):
        c = con[a]
        for p in range(c["slots"].size):
            bi = int(c["blk"][p])
            blk = st.blocks[bi]
            d = P.blocks[bi][1 if (pair and blk.type == "MOS1") else 0]
            key = (a, int(c["ent"][p]), bi, int(c["dev"][p]) // d["cs"])
            lst = exp.setdefault(key, [])
            if not (blk.type == "MOS1" and int(c["kk"][p]) in mos1_zero_slots(blk, pair)):
                lst.append((int(c["kk"][p]), int(c["dev"][p]) % d["cs"]))
    check(set(exp) == set(leaves), "targets")
    for key, lst in exp.items():
        check(tuple(lst) == leaves[key], "order", key)


SMALL = [n for n in CIRCUITS if n not in ("chain200", "chain520")]


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_interpreted_plan_sums_every_gather_list(lib, name):
    """(a), (c), (d) -- on both sp_mos1 variants"""
    st, P = structure(name), plan(lib, name)
    for pair in (False, True):
        if pair and not any(b.type == "MOS1" and b.count for b in st.blocks):
            continue
        interpret(st, P, pair)


@pytest.mark.parametrize("name", SMALL)
def test_tree_leaves_are_the_contributions_in_gather_order(lib, name):
    """(b) (the 200- and 520-stage chains repeat chain40's tiles; their trees are held by (a) and (i))"""
    st, P = structure(name), plan(lib, name)
    for pair in (False, True):
        if pair and not any(b.type == "MOS1" and b.count for b in st.blocks):
            continue
        check_order(st, P, pair, interpret(st, P, pair, symbolic=True)[1])


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_rows(lib, name):
    """(e) a slot with a target has a row of its own or is a named structural zero; every other slot maps to the trash row; the lane-pair
    plan's live rows are a subset of the general plan's; the flip-flop stages 53 rows on the lane-pair path, 80 on the general one."""
    st, P = structure(name), plan(lib, name)
    con = contributions(st)
    for bi, blk in enumerate(st.blocks):
        if not blk.count:
            assert P.blocks[bi] == [None, None]
            continue
        nslots = blk.n_g + blk.n_c + blk.n_b
        live = np.zeros(nslots, bool)
        for a in range(3):
            live[con[a]["kk"][con[a]["blk"] == bi]] = True
        assert (P.blocks[bi][1] is not None) == (blk.type == "MOS1")
        own = []
        for v, d in enumerate(P.blocks[bi]):
            if d is None:
                continue
            cs, rows = d["cs"], d["rows"]
            assert cs == (blk.count if d["chunks"] == 1 else cs) and d["chunks"] == -(-blk.count // cs)
            if not (blk.type == "MOS1" or blk.type.startswith("VA:")):
                assert d["rowoff"].size == 0 and rows == nslots
                continue
            zeros = mos1_zero_slots(blk, v == 1) if blk.type == "MOS1" else set()
            ro = d["rowoff"].astype(int)
            mine = np.array([live[k] and k not in zeros for k in range(nslots)])
            assert np.all(ro[~mine] == (rows - 1) * cs)
            assert sorted(ro[mine]) == [r * cs for r in range(rows - 1)]              # packed: one row each, no gaps
            assert np.all(np.diff(ro[mine]) > 0)                                     # in slot order
            own.append(set(np.nonzero(mine)[0]))
        if len(own) == 2:
            assert own[1] <= own[0]
    if name == "dff":
        mos = [P.blocks[bi] for bi, b in enumerate(st.blocks) if b.type == "MOS1"][0]
        assert (mos[1]["rows"], mos[0]["rows"]) == (53, 80)


def kernel_extent(nslots, n, cs, ipw, tile_words, u_lds):
    """Bytes of dynamic LDS that k_stamp_csr's carving reaches, as the kernel spells it: lds | ipw tiles | inst_par [ipw][3] | u_tile [ipw][n]
    when u_lds | rowoff [nslots] of 16 bits -- the launcher reserves the table rounded up to 8 bytes."""
    inst_par = ipw * tile_words
    u_tile = inst_par + 3 * ipw
    rowoff = u_tile + (ipw * n if u_lds else 0)
    return rowoff * 8 + ((nslots * 2 + 7) & ~7)


@pytest.mark.parametrize("name", ["dff", "dff_generated", "chain17", "chain40", "chain200", "va_zoo_x33", "psp103_ring", "linear_zoo_x65", "orphan"])
def test_geometry(lib, name):
    """(f) the relations tests/test_gpu_stamp_kernels.py (_reduce_launches) asserts from the debug line, and shmem against the kernel's carving"""
    st, P = structure(name), plan(lib, name)
    lanes = va_lanes(st, lib.sp_va_lanes)
    s, keep = hip.structure_c(st)
    tl = (C.c_int * len(lanes))(*lanes)
    rc = C.c_int(0)
    h = lib.sp_build(C.addressof(s), tl, C.addressof(rc))
    assert h and rc.value == 0
    cut = []
    for bi, blk in enumerate(st.blocks):
        if not blk.count:
            continue
        nslots = blk.n_g + blk.n_c + blk.n_b
        for v, d in enumerate(P.blocks[bi]):
            if d is None:
                continue
            for B in (1, 7, 65, 300):
                for readout in (0, 1):
                    for pad in (0, 4096):
                        o = (C.c_longlong * 7)()
                        lib.sp_geometry(h, bi, v, B, st.n, readout, pad, o)
                        lpd, rows, ipw, u_lds, tile_words, shmem, grid = list(o)
                        assert lpd == (2 if v else lanes[bi] if lanes[bi] else 1)
                        assert rows == (nslots if readout else d["rows"]) and tile_words == rows * d["cs"] + d["scratch"]
                        assert u_lds == (ipw * st.n * 8 <= 16 * 1024)
                        ipw0 = min(8, max(1, 64 // (blk.count * lpd))) if d["chunks"] == 1 else 1
                        assert 1 <= ipw <= ipw0 and (ipw == ipw0 or (ipw + 1) * tile_words * 8 > 64 * 1024)
                        assert ipw == 1 or ipw * tile_words * 8 <= 64 * 1024
                        assert grid == d["chunks"] * -(-B // ipw)
                        assert shmem == kernel_extent(nslots, st.n, d["cs"], ipw, tile_words, u_lds) + pad
                        if ipw < ipw0:
                            cut.append((blk.type, readout, ipw0, ipw))
    lib.sp_free(h)
    if name == "dff_generated":      # the read-out pass of the generated flip-flop: 2 x 30 x 192 words exceed 64 KB, one instance per wave
        assert ("VA:va_mos1l", 1, 2, 1) in cut and not any(c[1] == 0 for c in cut), cut


def test_encoding_constants(lib):
    assert [lib.sp_const(i) for i in range(15)] == [128, 5, 0, 1, 2, 3, 30, 28, 0x0FFFFFFF, 0xFF, 0x100, 3, 4, 5, 16]


def one_block(L, type_id, count, n_g, live, fan=1, tl=0):
    """Return code for a structure of one block of `count` devices with `n_g` G slots each; the first `live` slots (device 0) feed
    live / fan entries of G, `fan` slots each."""
    s = hip.StructureC()
    blocks = (hip.DeviceBlockC * 1)()
    b = blocks[0]
    b.type, b.count, b.n_g, b.n_c, b.n_b = type_id, count, n_g, 0, 0
    nnz = live // fan
    g_ptr = np.ascontiguousarray(np.arange(nnz + 1) * fan, dtype=np.int32)
    g_slots = np.ascontiguousarray(np.arange(live) * count, dtype=np.int32)
    zeros, none = np.zeros(nnz + 1, dtype=np.int32), np.array([-1], dtype=np.int32)
    s.n, s.n_nodes, s.nnz, s.n_blocks, s.blocks = 1, 1, nnz, 1, blocks
    s.ns_g, s.ns_c, s.ns_b = n_g * count, 0, 0
    s.g_ptr, s.g_slots, s.c_ptr, s.c_slots, s.b_ptr, s.b_slots = (hip._ip(a) for a in (g_ptr, g_slots, zeros, zeros, zeros, zeros))
    s.diag_nz = hip._ip(none)
    rc = C.c_int(0)
    h = L.sp_build(C.addressof(s), (C.c_int * 1)(tl), C.addressof(rc))
    if h:
        L.sp_free(h)
    return rc.value


def unowned_slot(L, st, lanes):
    """Return code when the first gather list of G names a slot behind every block's range."""
    s, keep = hip.structure_c(st)
    s.ns_g += 1
    [k for k in keep if isinstance(k, dict)][0]["g_slots"][0] = s.ns_g - 1
    return Plan(L, st, lanes, sc=(s, keep)).rc


def test_refusals(lib):
    """(g) CADNIP_BADARG, as before, for a gather list naming a slot no block owns and for a block over each 16-bit staging limit: slots x
    devices of a chunk above 65535 (chunks halve above 96 KB, so only a single device gets there); packed rows x devices above 65000;
    a tile (staged words + scratch) of 65535 words or more."""
    st = structure("divider")
    assert unowned_slot(lib, st, va_lanes(st, lib.sp_va_lanes)) == BADARG
    for args, rc in REFUSALS:
        assert one_block(lib, *args) == rc, args


# (type, devices, G slots per device, live slots, slots per entry) -> return code (the earlier builder's, recorded with the digests)
REFUSALS = [((hip.type_id("R"), 1, 65000, 1), 0),                    # one row per slot: 65000 staged words + 2 of scratch
            ((hip.type_id("R"), 1, 65536, 1), BADARG),               # cs x slots > 65535
            ((hip.type_id("R"), 1, 65535, 1), BADARG),               # passes that; the tile has 65535 + 2 words
            ((VA, 1, 65000, 64999), 0),                              # packed: 64999 live rows + the trash row = 65000
            ((VA, 1, 65000, 65000), BADARG),                         # 65001 rows
            ((VA, 1, 64000, 64000), 0),
            ((VA, 1, 64000, 64000, 64000), BADARG)]                  # one entry fed by all of them: 15999 scratch words of its 5-ary tree, the tile check


def _faulty(P, mutate):
    import copy
    Q = copy.copy(P)
    Q.blocks = [[None if d is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items() if k != "_owed"} for d in vs] for vs in P.blocks]
    Q.prep = P.prep.copy()
    mutate(Q)
    return Q


@pytest.mark.parametrize("fault", ["swap_operands", "rmw_to_store", "drop_level_flag", "drop_prep_word"])
def test_injected_faults_are_rejected(lib, fault):
    """(h) the shim's output patched: two operands of a record swapped (b), a read-modify-write turned into a store (a / c), a level fence
    dropped (a: the level above reads scratch that is not complete), a pre-set word dropped (a)."""
    # chain17: two chunks of sp_mos1 -- atomics, a three-level tree on the supply rail; nonlinear_zoo: a later block adds to the resistors' diagonals
    name = "nonlinear_zoo" if fault == "rmw_to_store" else "chain17"
    st, P = structure(name), plan(lib, name)
    mos = next((bi for bi, b in enumerate(st.blocks) if b.type == "MOS1"), None)
    later = [bi for bi, b in enumerate(st.blocks) if b.count and bi > 0]

    def mutate(Q):
        if fault == "swap_operands":
            d = Q.blocks[mos][0]
            i = next(i for i in range(d["rec"].shape[0]) if (d["rec"][i, 1] & 0xFFFF) >= 3 and (d["rec"][i, 2] & 0xFFFF) != (d["rec"][i, 2] >> 16))
            z = int(d["rec"][i, 2])
            d["rec"][i, 2] = ((z & 0xFFFF) << 16) | (z >> 16)
        elif fault == "rmw_to_store":
            for bi in later:
                d = Q.blocks[bi][0]
                hit = np.nonzero(((d["rec"][:, 0] >> 30) == 1) & ((d["rec"][:, 1] & 0xFFFF) > 0))[0]
                if hit.size:
                    d["rec"][hit[0], 0] &= np.uint32(0x3FFFFFFF)
                    return
            raise AssertionError("no RMW record")
        elif fault == "drop_level_flag":
            d = Q.blocks[mos][0]
            q = np.nonzero(d["info"] & 0x100)[0][0]
            d["info"][q] &= ~0x100
        else:
            assert Q.n_prep_atomic > 0
            Q.prep = Q.prep[1:]
            Q.n_prep_atomic -= 1
    Q = _faulty(P, mutate)
    with pytest.raises(Rejected):
        check_order(st, Q, False, interpret(st, Q, False, symbolic=True)[1])
    # the unpatched plan passes the same call
    check_order(st, P, False, interpret(st, P, False, symbolic=True)[1])


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_tables_are_those_of_the_earlier_builder(lib, name):
    """(i) sizes and SHA-256 of every table, per block and variant, against the record taken from the library's earlier build_plan_variant"""
    with open(DIGESTS) as f:
        want = json.load(f)[name]
    assert plan(lib, name).digests() == want
