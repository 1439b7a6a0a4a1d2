"""csrc/lds_layout.hpp: f2_fixed_ok is THE list of what the fixed form of the sweep kernel (k_fused2<WPB, false, 3>) assumes; fused2_plan
launches that kernel only when it returns true.  Host-only: the header is compiled with the host compiler, as tests/test_lds_layout.py does,
and the truth table is walked -- all conditions met gives true, every single violated condition gives false."""
import ctypes
import subprocess

import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "lds_layout.hpp"
extern "C" int t_fixed_ok(int tran, int lean, int newton_mode, int step_predec, int src_words, int n, int nc, int max_order, int step_rule,
                          int use_pcnr, int enabled) {
  return cadnip::f2_fixed_ok(tran != 0, lean != 0, newton_mode, step_predec != 0, src_words, n, nc, max_order, step_rule, use_pcnr, enabled != 0) ? 1 : 0;
}
"""

# the default transient call on the flip-flop (n = 235, core of 8, a source cache of some words)
GOOD = dict(tran=1, lean=1, newton_mode=1, step_predec=1, src_words=10, n=235, nc=8, max_order=2, step_rule=0, use_pcnr=0, enabled=1)
ORDER = list(GOOD)


@pytest.fixture(scope="module")
def ok(tmp_path_factory):
    d = tmp_path_factory.mktemp("f2_fixed")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    return lambda **kw: bool(L.t_fixed_ok(*[ctypes.c_int(dict(GOOD, **kw)[k]) for k in ORDER]))


def test_all_conditions_met(ok):
    assert ok()
    # the bounds themselves are inside: 256 unknowns, order 1, the smallest cache
    assert ok(n=256) and ok(n=1) and ok(max_order=1) and ok(src_words=1)


@pytest.mark.parametrize("violated", [
    dict(tran=0), dict(lean=0), dict(newton_mode=0), dict(newton_mode=2), dict(step_predec=0), dict(src_words=0), dict(n=257), dict(n=1000),
    dict(nc=0), dict(nc=12), dict(nc=16), dict(max_order=3), dict(step_rule=1), dict(use_pcnr=1), dict(enabled=0)],
    ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_single_violation_is_refused(ok, violated):
    assert not ok(**violated)
