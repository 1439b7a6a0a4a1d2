"""The sensitivity kernel's share of csrc/lds_layout.hpp and csrc/ac_hbm_plan.hpp, compiled with the host compiler as tests/test_lds_layout.py
and tests/test_ac_hbm_plan_cpu.py compile those headers: lds_ac_sens is lds_ac's map with a fourth n-vector behind it -- 16 (nnz_lu + 4 n)
bytes per system, every region on 16 bytes -- and ac_hbm_plan_bytes is ac_hbm_plan's rule for a per-system size given in bytes."""
import ctypes
import subprocess

import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "lds_layout.hpp"
#include "ac_hbm_plan.hpp"
using namespace cadnip;
typedef long long i64;
extern "C" {
void t_sens(int nnz_lu, int n, int w, int wpb, i64* o) {
  const LdsAcSens<size_t> L = lds_ac_sens((size_t)0, nnz_lu, n, w, wpb);
  o[0] = (i64)L.lu; o[1] = (i64)L.x; o[2] = (i64)L.r; o[3] = (i64)L.y; o[4] = (i64)L.xf; o[5] = (i64)L.end; o[6] = L.per; o[7] = (i64)lds_bytes(L);
}
void t_ac(int nnz_lu, int n, int w, int wpb, i64* o) {
  const LdsAc<size_t> L = lds_ac((size_t)0, nnz_lu, n, w, wpb);
  o[0] = (i64)L.lu; o[1] = (i64)L.x; o[2] = (i64)L.r; o[3] = (i64)L.y; o[4] = (i64)L.end;
}
i64 t_per(int nnz_lu, int n) { return (i64)ac_sens_hbm_system_bytes(nnz_lu, n); }
void t_plan_bytes(i64 per, i64 n_sys, int wpb, int max_waves, int n_cu, i64* o) {
  const AcHbmPlan p = ac_hbm_plan_bytes((size_t)per, (long)n_sys, wpb, max_waves, n_cu);
  o[0] = p.wpb; o[1] = p.n_waves; o[2] = (i64)p.work_bytes;
}
void t_plan(int nnz_lu, int n, i64 n_sys, int wpb, int max_waves, int n_cu, i64* o) {
  const AcHbmPlan p = ac_hbm_plan(nnz_lu, n, (long)n_sys, wpb, max_waves, n_cu);
  o[0] = p.wpb; o[1] = p.n_waves; o[2] = (i64)p.work_bytes;
}
}
"""
CAP = 256 << 20


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("ac_sens_layout")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    lib = ctypes.CDLL(lib)
    lib.t_per.restype = ctypes.c_longlong

    def call(fn, n_out, *args):
        o = (ctypes.c_longlong * n_out)()
        getattr(lib, fn)(*args, o)
        return tuple(o)
    lib.call = call
    return lib


def test_the_fourth_vector_sits_behind_lds_ac_s_regions(L):
    i = ctypes.c_int
    for nnz_lu, n in ((14, 6), (1091, 235), (6408, 2204), (1, 1)):
        per = 2 * (nnz_lu + 4 * n)                                # doubles
        assert L.t_per(i(nnz_lu), i(n)) == 16 * (nnz_lu + 4 * n)
        for wpb in (1, 2, 4, 8):
            for w in range(wpb):
                lu, x, r, y, xf, end, got_per, nbytes = L.call("t_sens", 8, i(nnz_lu), i(n), i(w), i(wpb))
                assert got_per == per and lu == w * per and end == wpb * per and nbytes == 16 * wpb * (nnz_lu + 4 * n)
                assert (x - lu, r - x, y - r, xf - y) == (2 * nnz_lu, 2 * n, 2 * n, 2 * n) and xf + 2 * n == lu + per     # regions tile the system
                assert all(v % 2 == 0 for v in (lu, x, r, y, xf))                                                       # 16-byte starts
                a = L.call("t_ac", 5, i(nnz_lu), i(n), i(0), i(1))
                assert (x - lu, r - lu, y - lu) == (a[1], a[2], a[3]) and a[4] == per - 2 * n                            # lds_ac, then n more


def test_the_plan_takes_the_per_system_size(L):
    i, q = ctypes.c_int, ctypes.c_longlong
    many = 1 << 20
    for nnz_lu, n in ((14, 6), (1091, 235), (6408, 2204)):
        per3, per4 = 16 * (nnz_lu + 3 * n), 16 * (nnz_lu + 4 * n)
        for n_sys in (1, 3, 2048, many):
            for wpb in (0, 1, 2, 4, 8, 3):
                for cap in (0, 2):
                    assert L.call("t_plan_bytes", 3, q(per3), q(n_sys), i(wpb), i(cap), i(256)) == L.call("t_plan", 3, i(nnz_lu), i(n), q(n_sys), i(wpb), i(cap), i(256))
        wpb, waves, nbytes = L.call("t_plan_bytes", 3, q(per4), q(many), i(0), i(0), i(256))
        assert wpb == 4 and nbytes == waves * per4 <= CAP and waves in (256 * 8, 256 * 4, 256 * 2, 256)
        assert waves == next(256 * k for k in (8, 4, 2, 1) if 256 * k * per4 <= CAP)
    assert L.call("t_plan_bytes", 3, q(CAP + 16), q(5), i(0), i(0), i(256)) == (0, 0, 0)         # a system beyond the cap
    assert L.call("t_plan_bytes", 3, q(0), q(5), i(0), i(0), i(256)) == (0, 0, 0)
    assert L.call("t_plan_bytes", 3, q(CAP), q(5), i(0), i(0), i(256)) == (4, 1, CAP)            # what fits
