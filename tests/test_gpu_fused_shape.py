"""The SHAPE form of the sweep kernel (csrc/fused2_kernel.hpp: k_fused2<WPB, false, 4>; csrc/lds_layout.hpp: f2_shape_ok): the fixed form
(variant 3) with the circuit's block list fixed as well -- the pinned voltage sources (<= 64), the pinned capacitors (<= 64) and one plain
sp_mos1 block of one lane-pair pass (<= 32), nothing else: no block loop, no type tests, no second pinned device per lane.  It holds the same
statements in the same order, so it must return what variant 3 returns, bit for bit; CADNIP_F2_SHAPE=0 keeps variant 3 (fused2.hip:
fused2_plan), and the plan line of CADNIP_F2_DEBUG=1 says which of the two a launch took (`shape 0|1`, in front of `fixed 0|1`).

The flip-flop of tests/test_gpu_fused_steps.py, 0 - 700 ns, Newton mode 1, with the helpers of tests/test_gpu_fused_fixed.py: the span crosses
every clock edge, an instance takes about 1 920 Newton rounds and a launch hands out 1 024 per wave, so every run crosses a launch seam --
controller state, history and kept factors (`lufac`) are stored by one launch and picked up by the next.  Workgroup widths 2, 4 and 8 run at
that file's batch sizes; width 1 runs one instance more than the device holds resident waves, so that one wave picks a second instance up
from the queue.  The near misses are the flip-flop with one thing added that the shape form does not cover -- a resistor to ground, a current
source, two buffers (34 MOSFETs), four more capacitors (65); they run 0 - 120 ns (both edges of the first clock pulse) and must take the same
kernel with the switch unset and at 0, `shape 0` on every plan line (NEAR below says which kernel that is for each)."""
import re

import numpy as np
import pytest

from cadnip_jl_amd import benchmarks as bm
from tests.test_gpu_fused_steps import BATCH, _setup, _env, CASES
from tests.test_gpu_fused_steps import _close_simulators  # noqa: F401  (module fixture: closes the simulators _setup cached)
from tests.test_gpu_fused_fixed import _run, _same

pytestmark = pytest.mark.gpu

NEAR_TSPAN = (0.0, 1.2e-7)


def _dff_resistor():
    c = bm.dff_circuit()
    c.R("RQ", "Q_tmp", "0", 1e6)                         # a fourth block
    return c


def _dff_isource():
    c = bm.dff_circuit()
    c.I("IQ", "Q_tmp", "0", dc=1e-6)                     # a fourth block, of the other source type
    return c


def _dff_34_fets():
    c = bm.dff_circuit()
    for k, (i, o) in enumerate((("Q", "B1"), ("B1", "B2"))):   # two buffers behind Q: 30 + 4 sp_mos1, beyond one lane-pair pass
        c.MOS1("X_bn%d" % k, o, i, "VSS", "VPW", bm.NFET_06V0, w=3.6e-07, l=6e-07)
        c.MOS1("X_bp%d" % k, o, i, "VDD", "VNW", bm.PFET_06V0, w=4.95e-07, l=5e-07)
    return c


def _dff_65_caps():
    c = bm.dff_circuit()
    for nd in ("D_neg", "net0", "net7", "Q_neg"):       # 61 + 4 capacitors: a second device on lane 0
        c.C("Cx_" + nd, nd, "0", 1e-15)
    return c


# name: (circuit, Newton mode, the variant its plan line names).  34 sp_mos1 are 265 unknowns: the lean tables, the steps and eight such instances
# do not fit the LDS of a compute unit, so fused2_blocks does not call the circuit lean and under Newton mode 1 the driver gives it the per-op
# kernels -- no sweep kernel, no plan line.  That case therefore runs under full Newton, where the sweep kernel's full-table variant takes it.
NEAR = {"resistor": (_dff_resistor, 1, 0), "isource": (_dff_isource, 1, 0), "fets34": (_dff_34_fets, 0, 1), "caps65": (_dff_65_caps, 1, 0)}
for _nm, (_mk, _, _) in NEAR.items():
    CASES.setdefault("dff_" + _nm, (_mk, {"vdd": 5.0}, ("vdd", 4.5, 5.5), NEAR_TSPAN))


def _field(plan, key):
    got = {int(re.search(r"\b%s (\d+)" % key, ln).group(1)) for ln in plan}
    assert len(got) == 1, plan
    return got.pop()


def _check_plan(plan, shape, wpb=None, variant=0):
    assert plan and all("variant %d" % variant in ln for ln in plan), plan
    assert _field(plan, "shape") == shape, plan
    if wpb is not None:
        assert _field(plan, "wpb") == wpb, plan


def _resident_plus_one(monkeypatch, capfd):
    """One flip-flop more than the waves k_fused2<1> keeps resident: workgroups per CU by the LDS block of a plan line (fused2.hip: fused2_plan)"""
    import torch
    _env(monkeypatch, 1)
    _, plan = _run(_setup("dff", BATCH[1]), capfd, newton_mode=1)
    per_cu = min((160 * 1024) // _field(plan, "shmem"), 32)
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu + 1


@pytest.mark.parametrize("wpb", [1, 2, 4, 8])
def test_shape_matches_fixed_to_the_bit(wpb, monkeypatch, capfd):
    B = _resident_plus_one(monkeypatch, capfd) if wpb == 1 else BATCH[wpb]
    _env(monkeypatch, wpb)
    monkeypatch.delenv("CADNIP_F2_SHAPE", raising=False)
    ctx = _setup("dff", B)
    got, plan = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan, 1, wpb)
    assert _field(plan, "fixed") == 1
    assert len(plan) >= 2, plan                       # the launch seam is crossed
    if wpb == 1:
        assert _field(plan, "grid") == B - 1, plan    # one instance waits in the queue
    monkeypatch.setenv("CADNIP_F2_SHAPE", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan0, 0, wpb)
    assert _field(plan0, "fixed") == 1 and _field(plan0, "grid") == _field(plan, "grid")
    assert len(plan0) == len(plan)
    assert np.all(ref[1][:, 0] > 1024), ref[1][:, 0].min()   # every instance ran beyond one launch's budget of rounds
    assert np.all(np.isfinite(ref[0])) and np.ptp(ref[0]) > 0.1
    assert _same(got, ref)


@pytest.mark.parametrize("name", sorted(NEAR))
def test_near_miss_takes_the_fixed_form(name, monkeypatch, capfd):
    _env(monkeypatch, 1)
    monkeypatch.delenv("CADNIP_F2_SHAPE", raising=False)
    _, newton_mode, variant = NEAR[name]
    ctx = _setup("dff_" + name, BATCH[1])
    got, plan = _run(ctx, capfd, newton_mode=newton_mode)
    _check_plan(plan, 0, variant=variant)
    monkeypatch.setenv("CADNIP_F2_SHAPE", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=newton_mode)
    _check_plan(plan0, 0, variant=variant)
    assert plan0 == plan                              # the same kernel ran, on the same plan
    assert np.all(np.isfinite(ref[0])) and np.ptp(ref[0]) > 0.1
    assert _same(got, ref)


def test_without_the_fixed_form_there_is_no_shape_form(monkeypatch, capfd):
    _env(monkeypatch, 1)
    monkeypatch.delenv("CADNIP_F2_SHAPE", raising=False)
    ctx = _setup("dff", BATCH[1])
    got, plan = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan, 1, 1)
    monkeypatch.setenv("CADNIP_F2_FIXED", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan0, 0, 1)
    assert _field(plan0, "fixed") == 0
    assert _same(got, ref)
