"""csrc/lds_layout.hpp: f2_shape_ok is THE list of what the shape form of the sweep kernel (k_fused2<WPB, false, 4>) assumes beyond the fixed
form: a block list of three -- the pinned voltage sources (at most 64), the pinned capacitors (at most 64), one plain sp_mos1 block of at
most 32 devices.  fused2_plan launches that kernel only when it returns true.  Host-only, built like tests/test_f2_fixed_cpu.py: the header
is compiled with the host compiler and the truth table is walked -- all conditions met gives true, every single violated condition false."""
import ctypes
import subprocess

import pytest

from tests.test_lds_layout import CSRC

SHIM = r"""
#include "lds_layout.hpp"
extern "C" int t_shape_ok(int fixed, int n_blk, int src_type, int src_count, int rc_type, int rc_count, int dev_type, int dev_plain, int dev_count,
                          int enabled) {
  return cadnip::f2_shape_ok(fixed != 0, n_blk, src_type, src_count, rc_type, rc_count, dev_type, dev_plain, dev_count, enabled != 0) ? 1 : 0;
}
extern "C" int t_code(int which) {
  const int c[] = {CADNIP_DEV_RESISTOR, CADNIP_DEV_CAPACITOR, CADNIP_DEV_VSOURCE, CADNIP_DEV_ISOURCE, CADNIP_DEV_MOS1, CADNIP_DEV_DIODE};
  return c[which];
}
"""

ORDER = ["fixed", "n_blk", "src_type", "src_count", "rc_type", "rc_count", "dev_type", "dev_plain", "dev_count", "enabled"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("f2_shape")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    T = dict(zip(["resistor", "capacitor", "vsource", "isource", "mos1", "diode"], [L.t_code(i) for i in range(6)]))
    # the flip-flop of the benchmark: 7 voltage sources, 61 capacitors, 30 plain sp_mos1
    good = dict(fixed=1, n_blk=3, src_type=T["vsource"], src_count=7, rc_type=T["capacitor"], rc_count=61, dev_type=T["mos1"], dev_plain=1,
                dev_count=30, enabled=1)
    return (lambda **kw: bool(L.t_shape_ok(*[ctypes.c_int(dict(good, **kw)[k]) for k in ORDER]))), T


def test_all_conditions_met(shim):
    ok, _ = shim
    assert ok()
    # the bounds themselves are inside
    assert ok(src_count=64) and ok(rc_count=64) and ok(dev_count=32)
    assert ok(src_count=64, rc_count=64, dev_count=32)
    assert ok(src_count=1) and ok(rc_count=1) and ok(dev_count=1)


VIOLATIONS = {
    "fixed_form_off": lambda T: dict(fixed=0),
    "n_blk_2": lambda T: dict(n_blk=2),
    "n_blk_4": lambda T: dict(n_blk=4),
    "source_type_isource": lambda T: dict(src_type=T["isource"]),
    "source_count_65": lambda T: dict(src_count=65),
    "rc_type_resistor": lambda T: dict(rc_type=T["resistor"]),
    "capacitor_count_65": lambda T: dict(rc_count=65),
    "mos1_count_33": lambda T: dict(dev_count=33),
    "mos1_not_plain": lambda T: dict(dev_plain=0),
    "third_block_diode": lambda T: dict(dev_type=T["diode"]),
    "third_block_resistor": lambda T: dict(dev_type=T["resistor"]),
    "third_block_missing": lambda T: dict(dev_type=-1),
    "no_source_block": lambda T: dict(src_type=-1),
    "no_rc_block": lambda T: dict(rc_type=-1),
    "disabled": lambda T: dict(enabled=0),
}


@pytest.mark.parametrize("violated", sorted(VIOLATIONS))
def test_single_violation_is_refused(shim, violated):
    ok, T = shim
    assert not ok(**VIOLATIONS[violated](T))
