"""csrc/lds_layout.hpp: the two packing rules of the words the sweep kernel's shape form pins for its sp_mos1 lanes (csrc/devices.hpp:
M1PairView) -- lds_m1pin_operand (node -> 16-bit byte offset from the instance's W of its word of u, ground -> the constant word 0.0) and
lds_m1pin_row (node -> the W word `rowof` names, ground -> the lane's trash word) -- held, with the host compiler, against the table walk
they replace: volt(u, node) = node < 0 ? 0.0 : u[node], read from a work area laid out by lds_sweep, and Rn's
node < 0 ? trash : rowof[node].  lds_m1pin_ok is the condition under which every offset fits 16 bits."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "lds_layout.hpp"
using namespace cadnip;
extern "C" {
int m_consts() { return LDS_CONSTS; }
int m_ok(int lu, int n) { return lds_m1pin_ok(lu, n) ? 1 : 0; }
unsigned m_operand(int node, int lu, int n) { return lds_m1pin_operand(node, lu, n); }
unsigned m_row(const unsigned short* rowof, int node, unsigned trash) { return lds_m1pin_row(rowof, node, trash); }
// what the kernel's read does: the double at W + offset, W being instance w's work array inside a block laid out by lds_sweep
double m_read(const double* block, int tab, int desc, int lu, int n, int w, int wpb, int src_words, unsigned off) {
  const LdsSweep<const double*> L = lds_sweep(block, tab, desc, lu, n, w, wpb, src_words);
  return *(const double*)((const char*)L.W + off);
}
// the layout itself, as offsets in doubles: W, nW, u, beta, end
void m_layout(int tab, int desc, int lu, int n, int w, int wpb, int src_words, long long* o) {
  const LdsSweep<size_t> L = lds_sweep((size_t)0, tab, desc, lu, n, w, wpb, src_words);
  o[0] = L.W; o[1] = L.nW; o[2] = L.u; o[3] = L.beta; o[4] = L.end;
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("m1pin")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    L = ctypes.CDLL(so)
    L.m_operand.restype = ctypes.c_uint
    L.m_row.restype = ctypes.c_uint
    L.m_read.restype = ctypes.c_double
    L.m_read.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_uint]
    L.m_row.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint]
    return L


def _layout(lib, tab, desc, lu, n, w, wpb, src):
    o = (ctypes.c_longlong * 5)()
    lib.m_layout(tab, desc, lu, n, w, wpb, src, o)
    return dict(zip(("W", "nW", "u", "beta", "end"), o))


# (lu_words, n, staged table words, descriptor words, waves per workgroup, source cache words): the flip-flop's program, a tiny circuit, an inverter-sized one
SMALL = [(1091, 235, 4096, 2432 + 2432 // 16, 8, 6), (3, 1, 4, 0, 1, 0), (40, 22, 128, 128, 2, 2)]


@pytest.mark.parametrize("lu,n,tab,desc,wpb,src", SMALL)
def test_operand_reads_what_volt_reads(lib, lu, n, tab, desc, wpb, src):
    assert lib.m_ok(lu, n) == 1
    lay = _layout(lib, tab, desc, lu, n, 0, wpb, src)
    rng = np.random.default_rng(lu + n)
    block = rng.standard_normal(lay["end"]) + 3.0            # no word of the block is 0.0 by chance
    for w in range(wpb):
        lw = _layout(lib, tab, desc, lu, n, w, wpb, src)
        block[lw["W"] + lw["nW"]], block[lw["W"] + lw["nW"] + 1] = 0.0, 1.0    # the constant words, as the kernel's entry sets them
    ptr = block.ctypes.data_as(ctypes.c_void_p)
    for w in range(wpb):
        lw = _layout(lib, tab, desc, lu, n, w, wpb, src)
        u = block[lw["u"]:lw["u"] + n]                       # this instance's unknowns
        offs = [lib.m_operand(node, lu, n) for node in range(-1, n)]
        assert all(o % 8 == 0 and o <= 0xFFFF for o in offs) and len(set(offs)) == n + 1
        for node, off in zip(range(-1, n), offs):
            want = 0.0 if node < 0 else u[node]              # devices.hpp: volt(u, node)
            assert lib.m_read(ptr, tab, desc, lu, n, w, wpb, src, off) == want, (w, node)
        # the same word of beta lies 8 n bytes on (M1PairView::beta): du = a0 u + beta reads both
        for node in (0, n - 1):
            assert lib.m_read(ptr, tab, desc, lu, n, w, wpb, src, lib.m_operand(node, lu, n) + 8 * n) == block[lw["beta"] + node]
    assert lib.m_operand(-1, lu, n) == 8 * (lu + n + 64) and lib.m_consts() == 2     # ground: the word 0.0 directly behind the 64 trash words


@pytest.mark.parametrize("n", [1, 22, 235])
def test_row_is_the_table_walk(lib, n):
    rng = np.random.default_rng(n)
    rowof = rng.permutation(n).astype(np.uint16) + np.uint16(1091)       # unknown -> rhs word, in pivot order behind the L\U words
    ptr = rowof.ctypes.data_as(ctypes.c_void_p)
    for lane in (0, 63):
        trash = 1091 + n + lane
        for node in range(-1, n):
            want = trash if node < 0 else int(rowof[node])   # fused2_kernel.hpp: AccumOutT::Rn
            assert lib.m_row(ptr, node, trash) == want
        assert lib.m_row(ptr, -1, trash) not in set(rowof.tolist())


def test_offsets_at_the_16_bit_limit(lib):
    n = 256
    lu = 8192 - 2 - 64 - 2 * n                               # W | consts | u end exactly at word 8192
    assert lib.m_ok(lu, n) == 1 and lib.m_ok(lu + 2, n) == 0 and lib.m_ok(lu, n + 1) == 0
    assert lib.m_operand(n - 1, lu, n) == 8 * 8191 == 0xFFF8             # the last unknown: the largest 16-bit multiple of 8
    assert lib.m_operand(0, lu, n) == 8 * (8192 - n) and lib.m_operand(-1, lu, n) == 8 * (8192 - n - 2)
    packed = lib.m_operand(n - 2, lu, n) | lib.m_operand(n - 1, lu, n) << 16   # two to a register, as the kernel packs them
    assert packed & 0xFFFF == 8 * 8190 and packed >> 16 == 8 * 8191
    # one word more and the last offset would need 17 bits: that is what lds_m1pin_ok refuses
    assert lib.m_operand(n - 1, lu + 2, n) > 0xFFFF
    # rows and trash words are words of W below 8192 whenever the steps are pre-decoded; 16 bits hold any of them
    rowof = np.array([8191], dtype=np.uint16)
    assert lib.m_row(rowof.ctypes.data_as(ctypes.c_void_p), 0, 8127) == 8191 and lib.m_row(rowof.ctypes.data_as(ctypes.c_void_p), -1, 8127) == 8127
