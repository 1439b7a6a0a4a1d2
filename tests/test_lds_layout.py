"""csrc/lds_layout.hpp is the one map of the dynamic LDS block of the LDS-resident kernels (k_fused2, k_fteam, k_lu_*): the kernels carve
their pointers from it, the launchers size the block with it.  This host-only check compiles the header with the host compiler and holds it
against the closed-form expressions the kernels and launch sites spelled out by hand before the header existed (written out literally
below, once, as the record of what the layout was): regions do not overlap, what is accessed as double2 / uint4 starts on 16 bytes, and
the totals are the old ones."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")

SHIM = r"""
#include "lds_layout.hpp"
using namespace cadnip;
typedef long long i64;
extern "C" {
i64 t_const(int i) { return i == 0 ? (i64)F2_TRASH : i == 1 ? (i64)LDS_BUDGET : (i64)LDS_OPTIN; }
void t_sweep(int tab, int desc, int lu, int n, int w, int wpb, i64* o) {
  const LdsSweep<size_t> L = lds_sweep((size_t)0, tab, desc, lu, n, w, wpb);
  o[0] = L.desc; o[1] = L.W; o[2] = L.u; o[3] = L.beta; o[4] = L.end; o[5] = L.nW; o[6] = L.per; o[7] = lds_bytes(L);
}
void t_team(int tab, int desc, int lu, int n, int par, int nw, i64* o) {
  const LdsTeam<size_t> L = lds_team((size_t)0, tab, desc, lu, n, par, nw);
  o[0] = L.W; o[1] = L.red; o[2] = L.u; o[3] = L.beta; o[4] = L.par; o[5] = L.desc; o[6] = L.priv; o[7] = L.end; o[8] = L.nW; o[9] = lds_bytes(L);
}
void t_lu(int tab, int desc, int lu, int n, int consts, int w, int waves, i64* o) {
  const LdsLu<size_t> L = lds_lu((size_t)0, tab, desc, lu, n, consts != 0, w, waves);
  o[0] = L.desc; o[1] = L.W; o[2] = L.end; o[3] = L.nW; o[4] = L.per; o[5] = lds_bytes(L);
}
}
"""


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    d = tmp_path_factory.mktemp("lds_layout")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    L.t_const.restype = ctypes.c_longlong

    def call(fn, *args):
        out = (ctypes.c_longlong * 10)()
        getattr(L, fn)(*[ctypes.c_int(a) for a in args], out)
        return list(out)
    L.call = call
    return L


# (lu_words, n): lu_words + n is even (f2_program.cpp pads the L\U words), which is what keeps every work array on 16 bytes.
# The flip-flop's real program (n = 235, 1091 L\U words), the smallest circuit, one at the tables' 16-bit limit, a ladder
SIZES = [(1091, 235), (1, 1), (3, 1), (2, 2), (32000, 32766), (6000, 2000)]
# staged table words (multiples of 4: fused2.hip pad4; 4096 / 9728: the flip-flop's lean range / full table) and step-list words
# (multiples of 128 = 64 lanes x 16 bytes; 2432: the flip-flop's 19 steps)
TABS = [0, 4, 4096, 9728, 40004]
DESCS = [0, 128, 2432, 128 * 300]
PARS = [0, 1, 7, 30 * 33, 30 * 33 + 1]          # sp_mos1 parameter rows: odd counts are rounded up to even
TRASH = 64


def disjoint_and_aligned(regions, end, aligned):
    """regions: name -> (start, length) in doubles; they tile [0, end) without overlap; `aligned` start on 16 bytes (even doubles)"""
    spans = sorted((s, s + ln, k) for k, (s, ln) in regions.items() if ln > 0)
    for (s0, e0, k0), (s1, e1, k1) in zip(spans, spans[1:]):
        assert e0 <= s1, (k0, k1)
    assert all(s >= 0 and e <= end for s, e, _ in spans)
    assert sum(e - s for s, e, _ in spans) == end           # nothing unaccounted for: the host reserves exactly what the kernel carves
    for k in aligned:
        assert regions[k][0] % 2 == 0, k


def test_constants(lay):
    assert lay.t_const(0) == TRASH and lay.t_const(1) == 160 * 1024 and lay.t_const(2) == 64 * 1024


def test_sweep_layout(lay):
    for (lu, n), tab, desc, wpb in itertools.product(SIZES, TABS, DESCS, (1, 2, 4, 8)):
        nW, per = lu + n + TRASH, lu + 3 * n + TRASH + 2
        regions = {"tab": (0, tab // 2), "desc": (tab // 2, desc)}
        for w in range(wpb):
            o_desc, W, u, beta, end, o_nW, o_per, nbytes = lay.call("t_sweep", tab, desc, lu, n, w, wpb)[:8]
            # k_fused2 as it carved by hand: W = sm + tab_dbl + desc_dbl + w * per; us = W + nW + 2; betas = us + n
            assert (o_desc, W, u, beta, o_nW, o_per) == (tab // 2, tab // 2 + desc + w * per, tab // 2 + desc + w * per + nW + 2,
                                                        tab // 2 + desc + w * per + nW + 2 + n, nW, per)
            # the launch sites: (tab_dbl + desc_dbl + wpb * per) * 8, per = lu_words + 3 n + F2_TRASH + 2
            assert nbytes == (tab // 2 + desc + wpb * (lu + 3 * n + TRASH + 2)) * 8 and end * 8 == nbytes
            regions.update({"W%d" % w: (W, nW), "c%d" % w: (W + nW, 2), "u%d" % w: (u, n), "beta%d" % w: (beta, n)})
        disjoint_and_aligned(regions, end, ["desc"] + ["W%d" % w for w in range(wpb)])


def test_team_layout(lay):
    for (lu, n), tab, desc, par, nw in itertools.product(SIZES, TABS, DESCS, PARS, (2, 4)):
        nW = lu + n + TRASH
        W, red, u, beta, parc, o_desc, priv, end, o_nW, nbytes = lay.call("t_team", tab, desc, lu, n, par, nw)
        par_even = (par + 1) & ~1
        # k_fteam as it carved by hand: W | 2 constants | red [NW][4] | u | beta | par (even) | descriptors | (NW - 1) private copies
        assert (W, red, u, beta, parc, o_desc, priv, o_nW) == (tab // 2, tab // 2 + nW + 2, tab // 2 + nW + 2 + 4 * nw, tab // 2 + nW + 2 + 4 * nw + n,
                                                              tab // 2 + nW + 2 + 4 * nw + 2 * n, tab // 2 + nW + 2 + 4 * nw + 2 * n + par_even,
                                                              tab // 2 + nW + 2 + 4 * nw + 2 * n + par_even + desc, nW)
        # the launch site: (tab_dbl + per + 4 nw + even(par_words) + desc_len + (nw - 1) (lu_words + n + F2_TRASH)) * 8, per as in the sweep kernel
        assert nbytes == (tab // 2 + (lu + 3 * n + TRASH + 2) + 4 * nw + par_even + desc + (nw - 1) * (lu + n + TRASH)) * 8 and end * 8 == nbytes
        regions = {"tab": (0, tab // 2), "W": (W, nW), "c": (W + nW, 2), "red": (red, 4 * nw), "u": (u, n), "beta": (beta, n),
                   "par": (parc, par_even), "desc": (o_desc, desc), "priv": (priv, (nw - 1) * nW)}
        disjoint_and_aligned(regions, end, ["W", "desc", "priv"])


def test_lu_layout(lay):
    # k_lu_steps: the work array and the constants alone; k_lu_f2_mw: tables + one work array
    for lu, n in SIZES:
        assert lay.call("t_lu", 0, 0, lu, n, 1, 0, 1)[:6] == [0, 0, lu + n + TRASH + 2, lu + n + TRASH, lu + n + TRASH + 2, (lu + n + TRASH + 2) * 8]
        for tab in TABS:
            assert lay.call("t_lu", tab, 0, lu, n, 0, 0, 1)[:6] == [tab // 2, tab // 2, tab // 2 + lu + n + TRASH, lu + n + TRASH, lu + n + TRASH,
                                                                   (tab // 2 + lu + n + TRASH) * 8]
    # k_lu_f2s (descriptors staged, constants) and k_lu_f2 (neither)
    for (lu, n), tab, desc, consts, wpb in itertools.product(SIZES, TABS, DESCS, (0, 1), (1, 2, 4, 8)):
        if not consts and desc:
            continue
        nW = lu + n + TRASH
        per = nW + (2 if consts else 0)
        regions = {"tab": (0, tab // 2), "desc": (tab // 2, desc)}
        for w in range(wpb):
            o_desc, W, end, o_nW, o_per, nbytes = lay.call("t_lu", tab, desc, lu, n, consts, w, wpb)[:6]
            # by hand: k_lu_f2s W = sm + tab_len / 2 + steps_len + w * (nW + 2); k_lu_f2 W = sm + tab_len / 2 + w * nW
            assert (o_desc, W, o_nW, o_per) == (tab // 2, tab // 2 + desc + w * per, nW, per)
            # the launch sites: (tabs + desc + wpb * (per + 2)) * 8 and (tab_dbl + wpb * per) * 8, per = lu_words + n + F2_TRASH
            assert nbytes == ((tab // 2 + desc + wpb * (lu + n + TRASH + 2)) * 8 if consts else (tab // 2 + wpb * (lu + n + TRASH)) * 8) and end * 8 == nbytes
            regions.update({"W%d" % w: (W, nW), "c%d" % w: (W + nW, per - nW)})
        disjoint_and_aligned(regions, end, ["desc"] + ["W%d" % w for w in range(wpb)])
