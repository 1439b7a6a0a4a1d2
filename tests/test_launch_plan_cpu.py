"""csrc/launch_plan.hpp: f2_choose and lu_choose are THE launch plans of the LDS-resident kernels, pure functions of facts about the handle
(PlanFacts) and of the diagnostic switches as values.  Host-only: the header is compiled with the host compiler behind a ctypes shim, as
tests/test_f2_fixed_cpu.py does, and the truth tables are walked from ONE good fact set -- the benchmark's flip-flop as its plan lines
describe it (n = 235, a core of 8, 9 + 8 passes, 7 + 6 steps, 15 984 bytes of lean tables, seven sources, 30 plain sp_mos1 devices) on a
device of 256 compute units -- varying one thing per case.  The LDS thresholds are computed with the header's own lds_sweep / lds_team /
lds_lu through the shim, and each rule is asked at the last lu_words that passes and at the first that fails (lu_words + n is even, so
lu_words moves in steps of 2).

Two conditions of the plan cannot fail where the plan asks them, and the tests say so instead of pretending: lds_steps_predec_ok and
lds_m1pin_ok need a work array of 8192 words, and a circuit is lean -- which both presuppose -- only while EIGHT instances fit into 160 KB
(under 2 560 words each).  They are asked directly, at their own boundary and at the largest lean circuit."""
import ctypes as C
import subprocess

import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "launch_plan.hpp"
using namespace cadnip;
extern "C" {
int t_sizeof_facts() { return (int)sizeof(PlanFacts); }
int t_unset() { return SW_UNSET; }
int t_max_blocks() { return F2_MAX_BLOCKS; }
long long t_budget() { return (long long)LDS_BUDGET; }
void t_f2_choose(const PlanFacts* f, const int* s, int mode, int newton_mode, const int* o, long long* out) {
  const F2Switches sw{s[0], s[1], s[2], s[3], s[4], s[5], s[6]};
  F2CallOpts co{};
  if (o) co = F2CallOpts{o[0], o[1], o[2], o[3]};
  const F2Choice p = f2_choose(*f, sw, (F2Mode)mode, newton_mode, o ? &co : nullptr);
  const long long v[] = {p.rc, p.circuit_ok, p.nw, p.var, p.wpb, p.grid, (long long)p.shmem, p.tab_lo, p.tab_len, p.step_list, p.step_predec,
                         p.keep_factors, p.src_words, p.fixed, p.shape};
  for (int i = 0; i < 15; ++i) out[i] = v[i];
}
void t_lu_choose(const PlanFacts* f, const int* s, int fuse, int kernel, long long* out) {
  const LuPlan p = lu_choose(*f, LuSwitches{s[0], s[1], s[2], s[3]}, fuse != 0, kernel);
  const long long v[] = {p.kernel, p.wpb, p.wpi, p.nc, p.pre, p.post, p.tab_lo, p.tab_len, (long long)p.shmem};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
}
int t_lean(const PlanFacts* f) { return f2_lean(*f); }
long long t_sweep(int tab_len, int desc_len, int lu_words, int n, int wpb, int src_words) { return (long long)lds_bytes(lds_sweep((size_t)0, tab_len, desc_len, lu_words, n, 0, wpb, src_words)); }
long long t_team(int tab_len, int desc_len, int lu_words, int n, int par_words, int nw) { return (long long)lds_bytes(lds_team((size_t)0, tab_len, desc_len, lu_words, n, par_words, nw)); }
long long t_lu(int tab_len, int desc_len, int lu_words, int n, int consts, int waves) { return (long long)lds_bytes(lds_lu((size_t)0, tab_len, desc_len, lu_words, n, consts != 0, 0, waves)); }
int t_desc_words(int len, int predec) { return lds_sweep_desc_words(len, predec != 0); }
int t_wg_per_cu(long long bytes, int wpb) { return sweep_wg_per_cu((size_t)bytes, wpb); }
int t_cache_words(int count) { return src_cache_words(count); }
int t_cache_fits(int tab_len, int dw, int lu_words, int n, int wpb, int sw) { return src_cache_fits(tab_len, dw, lu_words, n, wpb, sw); }
int t_predec_ok(int lu_words, int n) { return lds_steps_predec_ok(lu_words, n); }
int t_m1pin_ok(int lu_words, int n) { return lds_m1pin_ok(lu_words, n); }
}
"""

TRAN, DC, STEP = 0, 1, 2
OK, BADARG = 0, 1
NONE, STEPS1, TEAM2, TEAM4 = 0, 1, 2, 3
AUTO, STEPS4, F2MW, F2S, F2, PLAIN = range(6)
R, CAP, VSRC, DIODE, DIODECAP, SMOS, MOS1, BV, BI, VA = 0, 1, 3, 9, 10, 11, 12, 13, 14, 15     # CADNIP_DEV_* (include/cadnip_hip.h)
HEAVY = (DIODE, DIODECAP, SMOS, BV, BI, VA)


class StepFacts(C.Structure):
    _fields_ = [("present", C.c_int), ("len", C.c_int), ("n_steps", C.c_int * 3)]


class BlockFacts(C.Structure):
    _fields_ = [("type", C.c_int), ("mos1_plain", C.c_int)]


SCALARS = ["B", "n", "n_cu", "nb", "va_ext", "analyzed", "tables", "delayed", "homotopy", "lu_words", "nc", "n_pre", "n_post", "lu_len", "lean_lo",
           "lean_end", "full_len", "loadpos_off", "par_words", "n_blk", "src_blk", "src_type", "src_count", "rc_type", "rc_count", "dev_type",
           "dev_plain", "dev_count"]


class PlanFacts(C.Structure):
    _fields_ = [(k, C.c_int) for k in SCALARS] + [("blk", BlockFacts * 32), ("steps1", StepFacts), ("steps4", StepFacts), ("team", StepFacts * 2),
                                                  ("lu_plain_threads", C.c_int)]


# The flip-flop.  Tables: [entry program, load map | permutations | stamp and node tables | J*u list]; step lists in 64-bit words
GOOD = dict(B=1100, n=235, n_cu=256, nb=3, va_ext=0, analyzed=1, tables=1, delayed=0, homotopy=0, lu_words=1111, nc=8, n_pre=9, n_post=8,
            lu_len=6236, lean_lo=6000, lean_end=9996, full_len=12176, loadpos_off=5452, par_words=0, n_blk=3, src_blk=1, src_type=VSRC,
            src_count=7, rc_type=CAP, rc_count=40, dev_type=MOS1, dev_plain=1, dev_count=30, lu_plain_threads=64,
            blk=[(MOS1, 1), (VSRC, 0), (CAP, 0)],
            steps1=(1, 2432, (7, 6, 5)), steps4=(1, 9728, (7, 5, 5)), team0=(1, 4608, (7, 5, 5)), team1=(1, 4864, (7, 6, 5)))
DEFAULT_CALL = (1, 2, 0, 0)        # Newton mode 1, max_order 2, step rule 0, no PCNR: the default transient call
F2_SW = ["nodirect", "team", "wpb", "steps_packed", "src_cache", "fixed", "shape"]
LU_SW = ["plain", "steps", "wpi", "f2s"]
F2_OUT = ["rc", "circuit_ok", "nw", "var", "wpb", "grid", "shmem", "tab_lo", "tab_len", "steps", "step_predec", "keep_factors", "src_words", "fixed", "shape"]
LU_OUT = ["kernel", "wpb", "wpi", "nc", "pre", "post", "tab_lo", "tab_len", "shmem"]


def facts(**kw):
    d = dict(GOOD, **kw)
    f = PlanFacts()
    for k in SCALARS + ["lu_plain_threads"]:
        setattr(f, k, d[k])
    for i in range(32):
        f.blk[i].type, f.blk[i].mos1_plain = -1, 0
    for i, (ty, plain) in enumerate(d["blk"]):
        f.blk[i].type, f.blk[i].mos1_plain = ty, plain
    for dst, key in ((f.steps1, "steps1"), (f.steps4, "steps4"), (f.team[0], "team0"), (f.team[1], "team1")):
        dst.present, dst.len = d[key][0], d[key][1]
        for i in range(3):
            dst.n_steps[i] = d[key][2][i]
    return f


class Plan(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    lib = C.CDLL(lib)
    for fn in ("t_budget", "t_sweep", "t_team", "t_lu"):
        getattr(lib, fn).restype = C.c_longlong
    lib.t_wg_per_cu.argtypes = [C.c_longlong, C.c_int]
    assert lib.t_sizeof_facts() == C.sizeof(PlanFacts) and lib.t_max_blocks() == 32
    unset = lib.t_unset()

    def f2(mode=TRAN, newton_mode=0, call=None, sw=None, **kw):
        s = (C.c_int * 7)(*[(sw or {}).get(k, unset) for k in F2_SW])
        assert not set(sw or {}) - set(F2_SW)
        out = (C.c_longlong * 15)()
        lib.t_f2_choose(C.byref(facts(**kw)), s, mode, newton_mode, None if call is None else (C.c_int * 4)(*call), out)
        return Plan(zip(F2_OUT, out))

    def lu(kernel=AUTO, fuse=1, sw=None, **kw):
        s = (C.c_int * 4)(*[(sw or {}).get(k, unset) for k in LU_SW])
        assert not set(sw or {}) - set(LU_SW)
        out = (C.c_longlong * 9)()
        lib.t_lu_choose(C.byref(facts(**kw)), s, fuse, kernel, out)
        return Plan(zip(LU_OUT, out))

    lib.f2, lib.lu, lib.BUDGET = f2, lu, lib.t_budget()
    return lib


def last_ok(cond, start=1, stop=30001):
    """the last lu_words (odd, as n is) from `start` up for which cond holds, cond being true at `start` and false somewhere below `stop`"""
    assert cond(start)
    for lw in range(start, stop, 2):
        if not cond(lw + 2):
            return lw
    raise AssertionError("the condition never fails")


TEAM_OFF = {"team": 0}


# ---- the fused plan: the batch rules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nw,wpb", [(256, 4, 0), (257, 2, 0), (512, 2, 0), (513, 0, 4), (1024, 0, 4), (1025, 0, 8)])
def test_batch_boundaries(L, B, nw, wpb):
    p = L.f2(B=B, newton_mode=1)
    assert (p.rc, p.circuit_ok, p.nw, p.wpb) == (OK, 1, nw, wpb), p
    assert p.steps == {4: TEAM4, 2: TEAM2, 0: STEPS1}[nw] and p.var == 0 and p.keep_factors == 1
    assert (p.tab_lo, p.tab_len) == (6000, 3996)


def test_team_switch(L):
    assert L.f2(B=256, sw=TEAM_OFF).wpb == 1 and L.f2(B=256, sw=TEAM_OFF).nw == 0
    assert L.f2(B=512, sw=TEAM_OFF).wpb == 2
    for v, nw in ((2, 2), (3, 2), (4, 4), (9, 4), (1, 0)):
        for B in (1, 1100, 5000):
            assert L.f2(B=B, sw={"team": v}).nw == nw, (v, B)


@pytest.mark.parametrize("asked,got", [(1, 1), (2, 2), (3, 2), (4, 4), (8, 8), (9, 8), (0, 1)])
def test_wpb_switch_clamps(L, asked, got):
    p = L.f2(B=4096, sw={"wpb": asked})
    assert (p.rc, p.wpb) == (OK, got), p
    assert L.f2(B=513, sw={"wpb": asked}).wpb == min(got, 4)       # the cap never widens what the batch rule gives


def test_step_mode(L):
    for B in (1, 300, 5000):
        p = L.f2(mode=STEP, B=B, sw={"team": 0} if B == 300 else None)
        assert (p.rc, p.nw, p.steps, p.keep_factors) == (OK, 4, TEAM4, 1), p       # a team of four whatever the batch and the switch
    p = L.f2(mode=STEP, B=1, team1=(0, 0, (0, 0, 0)))
    assert (p.rc, p.circuit_ok, p.nw) == (BADARG, 1, 0), p
    # ... nor when the team's block exceeds the LDS of a CU.  Four work arrays always fit where the lean rule's eight instances do, so it is
    # the team's step list (one-term steps: the longest of the four lists; 128 words per step) that is grown here, not lu_words
    fits = lambda steps: L.t_team(3996, 128 * steps, 1111, 235, 0, 4) <= L.BUDGET
    steps = max(s for s in range(38, 400) if fits(s))
    assert fits(steps) and not fits(steps + 1)
    p = L.f2(mode=STEP, B=1, team1=(1, 128 * steps, (7, 6, 5)))
    assert (p.rc, p.nw, p.shmem) == (OK, 4, L.t_team(3996, 128 * steps, 1111, 235, 0, 4)), p
    p = L.f2(mode=STEP, B=1, team1=(1, 128 * (steps + 1), (7, 6, 5)))
    assert (p.rc, p.circuit_ok, p.nw) == (BADARG, 1, 0), p
    p = L.f2(mode=TRAN, B=1, newton_mode=1, team1=(1, 128 * (steps + 1), (7, 6, 5)))      # a transient then takes the sweep kernel
    assert (p.rc, p.nw, p.wpb) == (OK, 0, 1), p


def test_dc_never_a_team(L):
    for B in (1, 256, 300, 1100):
        for sw in (None, {"team": 4}):
            p = L.f2(mode=DC, B=B, sw=sw)
            assert (p.rc, p.nw, p.keep_factors, p.steps, p.src_words) == (OK, 0, 0, STEPS1, 0), p
    assert L.f2(mode=DC, B=1, newton_mode=1).keep_factors == 0


NOT_LEAN = dict(blk=[(MOS1, 1), (VSRC, 0), (DIODE, 0)])


def test_refusals(L):
    # kept factors (Newton mode 1, the single step) exist in the lean variant only
    for kw in (dict(mode=TRAN, newton_mode=1), dict(mode=STEP)):
        p = L.f2(**dict(kw, **NOT_LEAN))
        assert (p.rc, p.circuit_ok) == (BADARG, 0), p
        p = L.f2(sw={"nodirect": 1}, **kw)
        assert (p.rc, p.circuit_ok) == (BADARG, 0), p
    assert L.f2(mode=TRAN, newton_mode=0, **NOT_LEAN).rc == OK and L.f2(mode=DC, newton_mode=1, **NOT_LEAN).rc == OK
    p = L.f2(delayed=1)
    assert (p.rc, p.circuit_ok) == (BADARG, 0), p
    assert L.f2(mode=DC, delayed=1).rc == OK
    p = L.f2(homotopy=1)
    assert (p.rc, p.circuit_ok) == (BADARG, 1), p
    for kw in (dict(va_ext=1), dict(analyzed=0), dict(tables=0), dict(nb=33)):
        for mode in (TRAN, DC, STEP):
            p = L.f2(mode=mode, **kw)
            assert (p.rc, p.circuit_ok) == (BADARG, 0), (kw, p)
    assert L.f2(nb=32).rc == OK


def test_variants(L):
    p = L.f2(**NOT_LEAN)
    assert (p.rc, p.var, p.steps, p.tab_lo, p.tab_len, p.step_predec) == (OK, 1, NONE, 0, 12176, 0), p
    p = L.f2(sw={"nodirect": 1})
    assert (p.rc, p.var, p.steps, p.tab_lo, p.tab_len, p.nw, p.src_words) == (OK, 2, NONE, 0, 12176, 0, 0), p
    assert L.f2(B=1, sw={"nodirect": 0}).var == 2 and L.f2(B=1, sw={"nodirect": 0}).nw == 0      # set to anything


# ---- the fused plan: the LDS rules -------------------------------------------------------------------------------------------------------
def test_full_table_and_wpb_by_lds(L):
    """the full-table variant at 4096 instances: 8 waves per workgroup while they fit, then 4, 2, 1, and no fused kernel at all once one
    instance beside the full table is too much (the same bound for a lean circuit, whichever range it stages)"""
    for wpb in (8, 4, 2, 1):
        lw = last_ok(lambda w: L.t_sweep(12176, 0, w, 235, wpb, 0) <= L.BUDGET)
        p = L.f2(mode=DC, B=4096, lu_words=lw, **NOT_LEAN)
        assert (p.rc, p.wpb, p.shmem) == (OK, wpb, L.t_sweep(12176, 0, lw, 235, wpb, 0)), p
        p = L.f2(mode=DC, B=4096, lu_words=lw + 2, **NOT_LEAN)
        assert (p.rc, p.wpb) == ((OK, wpb // 2) if wpb > 1 else (BADARG, 0)), p
        if wpb == 1:
            assert p.circuit_ok == 0
            q = L.f2(B=1, lu_words=lw + 2, steps1=(1, 128, (1, 1, 1)), team1=(1, 128, (1, 1, 1)))
            assert (q.rc, q.circuit_ok) == (BADARG, 0), q


def test_lean_rule(L):
    f = lambda **kw: L.t_lean(C.byref(facts(**kw)))
    assert f()
    for ty in HEAVY:
        assert not f(blk=[(ty, 0)], n_blk=1), ty
        assert not f(blk=[(MOS1, 1), (VSRC, 0), (CAP, 0), (ty, 1)], n_blk=4), ty
    assert f(blk=[(MOS1, 1)], n_blk=1) and not f(blk=[(MOS1, 0)], n_blk=1)
    assert f(blk=[(t, 0) for t in range(9)], n_blk=9)            # every linear element and source
    assert not f(steps1=(0, 2432, (7, 6, 5)))
    lw = last_ok(lambda w: L.t_sweep(3996, 2432, w, 235, 8, 0) <= L.BUDGET)
    assert f(lu_words=lw) and not f(lu_words=lw + 2)
    assert L.f2(B=1, mode=DC, lu_words=lw).var == 0 and L.f2(B=1, mode=DC, lu_words=lw + 2).var == 1     # at any batch size
    # the two conditions that presuppose a lean circuit hold at the largest one; their own boundaries lie far beyond it
    assert L.t_predec_ok(lw, 235) and L.t_m1pin_ok(lw, 235)
    assert L.t_predec_ok(8192 - 66 - 235, 235) and not L.t_predec_ok(8192 - 66 - 235 + 1, 235)
    assert L.t_m1pin_ok(8192 - 66 - 470, 235) and not L.t_m1pin_ok(8192 - 66 - 470 + 1, 235)


def _window(L, admits, **kw):
    """the first lu_words from the good one up at which `admits` turns false while the circuit is still lean; a shorter step list than the
    flip-flop's leaves room for that below the lean rule's own bound"""
    lean = lambda w: L.t_lean(C.byref(facts(lu_words=w, **kw)))
    lw = GOOD["lu_words"]
    while lean(lw + 2) and not (admits(lw) and not admits(lw + 2)):
        lw += 2
    assert lean(lw + 2) and admits(lw) and not admits(lw + 2), "no boundary inside the lean range"
    return lw


SHORT = dict(steps1=(1, 1024, (3, 3, 2)))


def test_predecoded_steps_may_not_cost_a_workgroup(L):
    def admits(w, wpb=1):
        packed, pd = L.t_sweep(3996, 1024, w, 235, wpb, 0), L.t_sweep(3996, L.t_desc_words(1024, 1), w, 235, wpb, 0)
        return pd <= L.BUDGET and L.t_wg_per_cu(pd, wpb) == L.t_wg_per_cu(packed, wpb)
    lw = _window(L, admits, **SHORT)
    kw = dict(B=9, mode=DC, sw=TEAM_OFF, **SHORT)
    p, q = L.f2(lu_words=lw, **kw), L.f2(lu_words=lw + 2, **kw)
    assert (p.wpb, p.step_predec, p.shmem) == (1, 1, L.t_sweep(3996, L.t_desc_words(1024, 1), lw, 235, 1, 0)), p
    assert (q.wpb, q.step_predec, q.shmem) == (1, 0, L.t_sweep(3996, 1024, lw + 2, 235, 1, 0)), q
    assert p.grid == q.grid == 9
    r = L.f2(lu_words=lw, B=9, mode=DC, sw={"team": 0, "steps_packed": 1}, **SHORT)
    assert (r.step_predec, r.shmem) == (0, L.t_sweep(3996, 1024, lw, 235, 1, 0)), r
    assert L.f2(B=9, mode=DC, sw=TEAM_OFF, **NOT_LEAN).step_predec == 0


def test_source_cache(L):
    cw = L.t_cache_words(7)
    assert cw == 36
    dw = L.t_desc_words(1024, 1)
    lw = _window(L, lambda w: L.t_cache_fits(3996, dw, w, 235, 1, cw) and L.t_wg_per_cu(L.t_sweep(3996, dw, w + 2, 235, 1, 0), 1) == L.t_wg_per_cu(L.t_sweep(3996, 1024, w + 2, 235, 1, 0), 1), **SHORT)
    kw = dict(B=9, sw=TEAM_OFF, **SHORT)
    p, q = L.f2(lu_words=lw, **kw), L.f2(lu_words=lw + 2, **kw)
    assert (p.step_predec, p.src_words, p.shmem) == (1, cw, L.t_sweep(3996, dw, lw, 235, 1, cw)), p
    assert (q.step_predec, q.src_words, q.shmem) == (1, 0, L.t_sweep(3996, dw, lw + 2, 235, 1, 0)), q
    assert L.f2(B=9, sw=TEAM_OFF).src_words == cw
    assert L.f2(B=9, sw={"team": 0, "src_cache": 0}).src_words == 0 and L.f2(B=9, sw={"team": 0, "src_cache": 1}).src_words == cw
    assert L.f2(B=9, sw=TEAM_OFF, src_blk=-1).src_words == 0
    assert L.f2(B=9, sw=TEAM_OFF, src_count=70).src_words == 320      # the 64 pinned lanes
    assert L.f2(B=9, sw=TEAM_OFF, **NOT_LEAN).src_words == cw         # every direct-residual variant


def test_fixed_and_shape(L):
    p = L.f2(call=DEFAULT_CALL, newton_mode=1)
    assert (p.rc, p.var, p.fixed, p.shape) == (OK, 0, 1, 1), p
    assert L.f2(newton_mode=1).fixed == 0 and L.f2(newton_mode=1).shape == 0                  # no transient call named
    p = L.f2(call=DEFAULT_CALL, newton_mode=1, sw={"fixed": 0})
    assert (p.fixed, p.shape) == (0, 0), p
    p = L.f2(call=DEFAULT_CALL, newton_mode=1, sw={"shape": 0})
    assert (p.fixed, p.shape) == (1, 0), p
    assert L.f2(call=DEFAULT_CALL, newton_mode=1, sw={"fixed": 1, "shape": 1}).shape == 1
    for kw in (dict(call=(0, 2, 0, 0)), dict(call=(1, 3, 0, 0)), dict(sw={"steps_packed": 1}), dict(sw={"src_cache": 0}), dict(nc=12)):
        assert L.f2(**dict(dict(call=DEFAULT_CALL, newton_mode=1), **kw)).fixed == 0, kw
    for kw in (dict(dev_plain=0), dict(dev_count=33), dict(n_blk=4, blk=GOOD["blk"] + [(R, 0)]), dict(rc_count=65)):
        p = L.f2(call=DEFAULT_CALL, newton_mode=1, **kw)
        assert (p.fixed, p.shape) == (1, 0), (kw, p)


def test_grid_is_the_smaller_of_the_batch_and_the_resident_workgroups(L):
    assert L.f2(B=1100).grid == 138 and L.f2(B=1100).wpb == 8           # ceil(1100 / 8) < 256 x 1
    assert L.f2(B=4096).grid == 256
    p = L.f2(B=2048, sw={"wpb": 1})                                      # three workgroups of one wave per CU by LDS
    assert (p.wpb, p.grid) == (1, 256 * L.t_wg_per_cu(p.shmem, 1)) and L.t_wg_per_cu(p.shmem, 1) == 3
    assert L.f2(B=700, sw={"wpb": 1}).grid == 700
    assert L.f2(B=300).grid == 300 and L.f2(B=300).nw == 2              # teams of two: two workgroups per CU
    assert L.f2(B=1100, sw={"team": 2}).grid == 512
    assert L.f2(B=1100, sw={"team": 4}).grid == 256
    assert L.f2(B=1100, sw={"team": 4}).shmem == L.t_team(3996, 4864, 1111, 235, 0, 4)


# ---- the plan of the per-op refactor + solve -----------------------------------------------------------------------------------------
NO_STEPS4 = dict(steps4=(0, 0, (0, 0, 0)))
MANY_PASSES = dict(n_pre=20, n_post=12, **NO_STEPS4)


def test_lu_batch_rules(L):
    p = L.lu(B=512)
    assert (p.kernel, p.wpb, p.wpi, p.nc, p.pre, p.post, p.shmem) == (STEPS4, 4, 4, 8, 7, 5, L.t_lu(0, 0, 1111, 235, 1, 1)), p
    assert L.lu(B=513).kernel == F2S
    p = L.lu(B=64, **MANY_PASSES)
    assert (p.kernel, p.wpb, p.wpi, p.pre, p.post, p.tab_len, p.shmem) == (F2MW, 4, 4, 20, 12, 6236, L.t_lu(6236, 0, 1111, 235, 0, 1)), p
    assert L.lu(B=64, **dict(MANY_PASSES, n_post=11)).kernel == F2S
    assert L.lu(B=65, **MANY_PASSES).kernel == F2S
    assert L.lu(B=64, n_pre=20, n_post=12).kernel == STEPS4            # the steps of a team come first


@pytest.mark.parametrize("B,wpb", [(255, 1), (256, 2), (511, 2), (512, 4), (1023, 4), (1024, 8)])
def test_lu_waves_per_workgroup(L, B, wpb):
    p = L.lu(B=B, **NO_STEPS4)
    assert (p.kernel, p.wpb, p.wpi, p.pre, p.post) == (F2S, wpb, 1, 7, 6), p
    assert (p.tab_lo, p.tab_len, p.shmem) == (5452, 784, L.t_lu(784, 2432, 1111, 235, 1, wpb)), p
    q = L.lu(kernel=F2, B=B)
    assert (q.kernel, q.wpb, q.pre, q.post, q.tab_len, q.shmem) == (F2, wpb, 9, 8, 6236, L.t_lu(6236, 0, 1111, 235, 0, wpb)), q


def test_lu_f2s_by_the_eight_instance_fit(L):
    lw = last_ok(lambda w: L.t_lu(784, 2432, w, 235, 1, 8) <= L.BUDGET)
    for B in (600, 4096):                      # (eight instances whatever the workgroup holds)
        assert L.lu(B=B, lu_words=lw).kernel == F2S and L.lu(B=B, lu_words=lw + 2).kernel == F2
    assert L.lu(kernel=F2S, lu_words=lw).kernel == F2S and L.lu(kernel=F2S, lu_words=lw + 2).kernel == -1
    # ... and the pass program halves its workgroup by LDS, down to k_lu
    for wpb in (8, 4, 2, 1):
        lw = last_ok(lambda w: L.t_lu(6236, 0, w, 235, 0, wpb) <= L.BUDGET)
        assert L.lu(B=4096, lu_words=lw, sw={"f2s": 0}).wpb == wpb
        p = L.lu(B=4096, lu_words=lw + 2, sw={"f2s": 0})
        assert (p.kernel, p.wpb) == ((F2, wpb // 2) if wpb > 1 else (PLAIN, 1)), p
        if wpb == 1:
            assert L.lu(kernel=F2, B=4096, lu_words=lw).kernel == F2 and L.lu(kernel=F2, B=4096, lu_words=lw + 2).kernel == -1


def test_lu_forced_kernels(L):
    for B in (1, 4096):
        assert L.lu(kernel=STEPS4, B=B).kernel == STEPS4 and L.lu(kernel=STEPS4, B=B, **NO_STEPS4).kernel == -1
        assert L.lu(kernel=F2MW, B=B).kernel == F2MW and L.lu(kernel=F2MW, B=B, lu_len=400000).kernel == -1
        assert L.lu(kernel=F2S, B=B).kernel == F2S and L.lu(kernel=F2S, B=B, steps1=(0, 0, (0, 0, 0))).kernel == -1
        assert L.lu(kernel=F2, B=B).kernel == F2 and L.lu(kernel=F2, B=B, lu_len=400000).kernel == -1
        p = L.lu(kernel=PLAIN, B=B, lu_plain_threads=256)
        assert (p.kernel, p.wpb, p.wpi, p.nc, p.pre, p.post) == (PLAIN, 4, 4, 0, 0, 0), p
        for k in (STEPS4, F2MW, F2S, F2):
            assert L.lu(kernel=k, B=B, tables=0).kernel == -1
            assert L.lu(kernel=k, B=B, sw=dict(plain=1, steps=0, wpi=1, f2s=0)).kernel == k       # a forced kernel ignores the switches
        assert L.lu(kernel=PLAIN, B=B, tables=0).kernel == PLAIN and L.lu(B=B, tables=0).kernel == PLAIN
    lw = last_ok(lambda w: L.t_lu(0, 0, w, 235, 1, 1) <= L.BUDGET)
    assert L.lu(kernel=STEPS4, lu_words=lw).kernel == STEPS4 and L.lu(kernel=STEPS4, lu_words=lw + 2).kernel == -1
    assert L.lu(B=1, lu_words=lw + 2).kernel == PLAIN


def test_lu_switches_and_the_unfused_jacobian(L):
    assert L.lu(B=4096, sw={"plain": 0}).kernel == PLAIN                 # set to anything
    assert L.lu(B=64, sw={"steps": 0}).kernel == F2S and L.lu(B=4096, sw={"steps": 1}).kernel == STEPS4
    assert L.lu(B=4096, sw={"wpi": 4}).kernel == F2MW
    assert L.lu(B=64, sw={"wpi": 1}, **MANY_PASSES).kernel == F2S
    assert L.lu(B=4096, sw={"f2s": 0}).kernel == F2 and L.lu(B=4096, sw={"f2s": 1}).kernel == F2S
    for B in (1, 4096):
        p = L.lu(B=B, fuse=0, lu_plain_threads=1024)
        assert (p.kernel, p.wpb, p.wpi) == (PLAIN, 16, 16), p


def test_one_device_size_scales_every_rule(L):
    """128 compute units: the team rules, the sweep kernel's halving, and the three batch rules of the LU plan all move with it"""
    kw = dict(n_cu=128)
    assert [L.f2(B=B, **kw).nw for B in (128, 129, 256, 257)] == [4, 2, 2, 0]
    assert [L.f2(B=B, **kw).wpb for B in (257, 512, 513)] == [4, 4, 8]
    assert L.f2(B=4096, **kw).grid == 128 and L.f2(B=200, **kw).grid == 200
    assert L.lu(B=256, **kw).kernel == STEPS4 and L.lu(B=257, **kw).kernel == F2S
    assert L.lu(B=32, **dict(MANY_PASSES, **kw)).kernel == F2MW and L.lu(B=33, **dict(MANY_PASSES, **kw)).kernel == F2S
    assert [L.lu(B=B, **dict(NO_STEPS4, **kw)).wpb for B in (127, 128, 255, 256, 511, 512)] == [1, 2, 2, 4, 4, 8]


def test_the_flip_flops_recorded_plans(L):
    """GOOD is consistent with the flip-flop's recorded plans.  Its table and step-list sizes were WORKED OUT FROM the `[cadnip f2]` lines of
    tests/golden/launch_plans.json (bytes of tables, steps and one instance; the teams' shmem), so agreement of a single line is by
    construction and proves nothing about the device.  What this does check: that one fact set fits all 24 lines and 24 factor_solve infos
    at once -- four batch sizes, both team settings, three calls, six kernels -- under the header's rules, and that GOOD stays the flip-flop
    should the fixture be recorded again.  The comparison with the device is tests/test_gpu_launch_plan.py's."""
    import json
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")) as f:
        doc = json.load(f)
    assert doc["n_cu"] == GOOD["n_cu"]
    seen = 0
    for B in (1, 300, 513, 1100):
        for team, sw in (("team_unset", None), ("team_0", TEAM_OFF)):
            rec = doc["cases"]["dff/%d" % B][team]
            for call, kw in (("dc", dict(mode=DC)), ("tran0", dict(mode=TRAN, newton_mode=0, call=(0, 2, 0, 0))),
                             ("tran1", dict(mode=TRAN, newton_mode=1, call=DEFAULT_CALL))):
                (line,) = rec[call]
                p = L.f2(B=B, sw=sw, **kw)
                num = lambda key: int(re.search(r"\b%s (\d+)" % key, line).group(1))
                m = re.search(r"team of (\d) waves", line)
                if m:
                    assert (p.nw, p.grid, p.shmem) == (int(m.group(1)), num("grid"), num("shmem")), (line, p)
                else:
                    assert (p.nw, p.wpb, p.grid, p.shmem, p.var, p.src_words, p.shape, p.fixed) == \
                        (0, num("wpb"), num("grid"), num("shmem"), num("variant"), num("src-cache"), num("shape"), num("fixed")), (line, p)
                    assert p.step_predec == ("(pre-decoded)" in line)
                seen += 1
    assert seen == 24
    # ... and lu_choose the ``info`` of factor_solve, for kernel "auto" and every forced kernel
    names = ("auto", "steps4", "mw4", "f2s", "f2", "plain")
    for B in (1, 300, 513, 1100):
        for k, name in enumerate(names):
            info, p = doc["cases"]["dff/%d" % B]["factor_solve"][name], L.lu(kernel=k, B=B)
            assert (names[p.kernel], p.wpb, p.wpi, p.nc, p.pre, p.post) == tuple(info[x] for x in ("kernel", "wpb", "wpi", "nc", "n_pre", "n_post")), (B, name, p)
