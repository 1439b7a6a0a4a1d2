"""csrc/ac_hbm_plan.hpp is the launch plan of the HBM-resident AC kernels (k_ac_lu_hbm / k_ac_adj_hbm, csrc/ac_lu.hip): how many persistent
waves a launch gets, hence how large the handle's workspace grows.  Host-only arithmetic, compiled here with the host compiler as
tests/test_lds_layout.py compiles its header, and held against the rule written out below:
  n_waves = min(n_sys, CUs x k), k the largest of 8, 4, 2, 1 with n_waves x 16 (nnz_lu + 3 n) <= AC_WORK_BYTES = 256 MiB
(what fits, when not even k = 1 does); a non-zero wave cap replaces CUs x k; wpb is 1, 2, 4 or 8, 0 meaning 4; a system beyond the cap and
every invalid request are refused (wpb 0 in the result)."""
import ctypes
import subprocess

import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "ac_hbm_plan.hpp"
using namespace cadnip;
typedef long long i64;
extern "C" {
i64 t_cap() { return (i64)AC_WORK_BYTES; }
i64 t_per(int nnz_lu, int n) { return (i64)ac_hbm_system_bytes(nnz_lu, n); }
void t_plan(int nnz_lu, int n, i64 n_sys, int wpb, int max_waves, int n_cu, i64* o) {
  const AcHbmPlan p = ac_hbm_plan(nnz_lu, n, (long)n_sys, wpb, max_waves, n_cu);
  o[0] = p.wpb; o[1] = p.n_waves; o[2] = (i64)p.work_bytes;
}
}
"""
CAP = 256 << 20
CUS = 256                                   # an MI355X


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("ac_hbm_plan")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    L.t_cap.restype = L.t_per.restype = ctypes.c_longlong
    assert L.t_cap() == CAP

    def call(nnz_lu, n, n_sys, wpb=0, max_waves=0, n_cu=CUS):
        o = (ctypes.c_longlong * 3)()
        L.t_plan(ctypes.c_int(nnz_lu), ctypes.c_int(n), ctypes.c_longlong(n_sys), ctypes.c_int(wpb), ctypes.c_int(max_waves), ctypes.c_int(n_cu), o)
        assert L.t_per(nnz_lu, n) == 16 * (nnz_lu + 3 * n)
        return tuple(o)
    return call


def rule(nnz_lu, n, n_sys, max_waves=0, n_cu=CUS):
    """The rule of the module docstring, literally."""
    per = 16 * (nnz_lu + 3 * n)
    if max_waves:
        return min(n_sys, max_waves)
    for k in (8, 4, 2, 1):
        if min(n_sys, n_cu * k) * per <= CAP:
            return min(n_sys, n_cu * k)
    return min(n_sys, CAP // per)


def test_the_k_ladder_on_both_sides_of_the_cap(plan):
    # per system 16 (nnz_lu + 3 n) bytes; n = 1000 throughout, nnz_lu chosen so that CUs x k workspaces sit just inside / just outside 256 MiB
    n, many = 1000, 1 << 20
    for k in (8, 4, 2, 1):
        fits = CAP // (CUS * k) // 16 - 3 * n                   # the largest nnz_lu with CUs x k x per <= CAP
        assert CUS * k * 16 * (fits + 3 * n) <= CAP < CUS * k * 16 * (fits + 1 + 3 * n)
        assert plan(fits, n, many) == (4, CUS * k, CUS * k * 16 * (fits + 3 * n))
        below = k // 2
        want = CUS * below if below else CAP // (16 * (fits + 1 + 3 * n))      # k = 1 does not fit either: what does
        assert plan(fits + 1, n, many) == (4, want, want * 16 * (fits + 1 + 3 * n)) and want * 16 * (fits + 1 + 3 * n) <= CAP
        assert plan(fits, n, many)[1] == rule(fits, n, many) and plan(fits + 1, n, many)[1] == rule(fits + 1, n, many)
    # the circuits of the tests: the flip-flop (1091, 235) takes the full 8 waves per compute unit; chain200 (6408, 2204: 208 KB a system,
    # 417 MiB for 2048 of them) takes 4
    for nnz_lu, n, k in ((1091, 235, 8), (14, 6, 8), (6408, 2204, 4)):
        assert plan(nnz_lu, n, many) == (4, CUS * k, CUS * k * 16 * (nnz_lu + 3 * n))
    # few systems never push k down: the ladder looks at the waves the launch would really have
    big = CAP // 16 // 100 - 3 * n                               # 100 of them fit, CUs x 1 do not
    assert plan(big, n, 100) == (4, 100, 100 * 16 * (big + 3 * n)) and plan(big, n, 101)[1] == rule(big, n, 101) == 100


def test_fewer_systems_than_compute_units(plan):
    for n_sys in (1, 2, 21, 255, 256, 257, 2047, 2048, 2049):
        wpb, n_waves, work = plan(1091, 235, n_sys)
        assert (wpb, n_waves, work) == (4, min(n_sys, 2048), min(n_sys, 2048) * 16 * (1091 + 3 * 235))
    assert plan(1091, 235, 21, n_cu=2) == (4, 16, 16 * 16 * (1091 + 3 * 235))          # a small device: CUs x 8
    for n_sys in (0, -1):
        assert plan(1091, 235, n_sys) == (0, 0, 0)


def test_the_wave_cap_replaces_cus_times_k(plan):
    per = 16 * (1091 + 3 * 235)
    assert plan(1091, 235, 21, max_waves=1) == (4, 1, per)
    assert plan(1091, 235, 21, max_waves=3) == (4, 3, 3 * per)
    assert plan(1091, 235, 21, max_waves=64) == (4, 21, 21 * per)                      # never more waves than systems
    assert plan(1091, 235, 1 << 20, max_waves=5000) == (4, 5000, 5000 * per)           # beyond CUs x 8: the caller's figure
    assert plan(1091, 235, 21, max_waves=-1) == (0, 0, 0)


def test_waves_per_workgroup(plan):
    for wpb in (1, 2, 4, 8):
        assert plan(1091, 235, 21, wpb=wpb) == (wpb, 21, 21 * 16 * (1091 + 3 * 235))
    assert plan(1091, 235, 21, wpb=0)[0] == 4
    for wpb in (3, 16, -1, 5, 64):
        assert plan(1091, 235, 21, wpb=wpb) == (0, 0, 0)


def test_a_system_larger_than_the_cap_is_refused(plan):
    n = 1000
    last = CAP // 16 - 3 * n                                     # per == CAP exactly: one wave
    assert plan(last, n, 10) == (4, 1, CAP)
    assert plan(last + 1, n, 10) == (0, 0, 0) and plan(last + 1, n, 10, max_waves=1) == (0, 0, 0)
    assert plan(0, n, 10) == (0, 0, 0) and plan(10, 0, 10) == (0, 0, 0) and plan(10, 10, 10, n_cu=0) == (0, 0, 0)


def test_work_bytes_is_a_size_t_product(plan):
    # 16 (nnz_lu + 3 n) x n_waves beyond 2^32 -- reachable only through the caller's own wave cap; the plan's own choice stays within 256 MiB
    nnz_lu, n, waves = 3_000_000, 100_000, 100
    per = 16 * (nnz_lu + 3 * n)
    assert per * waves > 1 << 32 and per <= CAP
    assert plan(nnz_lu, n, 1000, max_waves=waves) == (4, waves, per * waves)
    assert plan(nnz_lu, n, 1000) == (4, CAP // per, (CAP // per) * per)
    # ... and a per-system size whose 32-bit product with 16 alone would wrap: 16 x 2^28 = 2^32
    assert plan((1 << 28) - 3, 1, 1) == (0, 0, 0)
