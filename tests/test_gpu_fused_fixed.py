"""The FIXED form of the sweep kernel (csrc/fused2_kernel.hpp: k_fused2<WPB, false, 3>; csrc/lds_layout.hpp: f2_fixed_ok): variant 0 with
the default transient call's switches -- Newton mode 1, pre-decoded steps, source cache, core of 8, no PCNR, max_order <= 2, step_rule 0,
n <= 256 -- as compile-time constants.  It holds the same statements in the same order, so it must return what the generic variant 0
returns, bit for bit; CADNIP_F2_FIXED=0 keeps the generic kernel (fused2.hip: fused2_plan), and the plan line of CADNIP_F2_DEBUG=1 says
which of the two a launch took (`fixed 0|1`; the family stays `variant 0`).

The flip-flop of tests/test_gpu_fused_steps.py, 0 - 700 ns, Newton mode 1, at that file's four batch sizes (k_fused2<1 | 2 | 4 | 8>, the team
kernel switched off).  An instance takes about 1 920 Newton rounds and a launch hands out 1 024 per wave, so every run crosses a launch
seam: controller state, history and kept factors are stored by one launch and picked up by the next."""
import re

import numpy as np
import pytest

from tests import circuits as tc
from tests.test_gpu_fused_steps import BATCH, _setup, _env, CASES
from tests.test_gpu_fused_steps import _close_simulators  # noqa: F401  (module fixture: closes the simulators _setup cached)

pytestmark = pytest.mark.gpu

CASES.setdefault("rc_charge", (tc.rc_charge, {}, None, (0.0, 3e-3)))   # three unknowns: no dense core (core size 0)


def _run(ctx, capfd, **opts):
    """One fused transient from the shared DC state: outputs, per-instance counters, the final state and the plan lines of its launches."""
    sim = ctx["sim"]
    sim.h.set_u(ctx["u0"])
    capfd.readouterr()
    out, per, stats = sim.h.tran_run(ctx["tspan"][0], ctx["tspan"][1], ctx["atol"], 1e-4, breaks=ctx["breaks"], save_t=ctx["ts"], obs=ctx["obs"],
                                     fused=1, **opts)
    u = sim.h.get_u()
    plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[cadnip f2] B ")]
    assert stats["n_failed"] == 0
    return (out, per, u), plan


def _check_plan(plan, fixed, wpb=None):
    assert plan and all("variant 0" in ln and ln.rstrip().endswith(" fixed %d" % fixed) for ln in plan), plan
    if wpb is not None:
        assert {int(re.search(r"wpb (\d+)", ln).group(1)) for ln in plan} == {wpb}, plan


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("wpb", [1, 2, 4, 8])
def test_fixed_matches_generic_to_the_bit(wpb, monkeypatch, capfd):
    _env(monkeypatch, wpb)
    ctx = _setup("dff", BATCH[wpb])
    got, plan = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan, 1, wpb)
    assert len(plan) >= 2, plan                       # the launch seam is crossed
    monkeypatch.setenv("CADNIP_F2_FIXED", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan0, 0, wpb)
    assert len(plan0) == len(plan)
    assert np.all(ref[1][:, 0] > 1024), ref[1][:, 0].min()   # every instance ran beyond one launch's budget of rounds
    assert _same(got, ref)


@pytest.mark.parametrize("opts", [dict(newton_mode=1, max_order=3), dict(newton_mode=1, step_rule=1), dict(newton_mode=1, use_pcnr=True), dict(newton_mode=0)],
                         ids=["max_order3", "step_rule1", "pcnr", "full_newton"])
def test_ineligible_call_takes_the_generic_form(opts, monkeypatch, capfd):
    _env(monkeypatch, 1)
    ctx = _setup("dff", BATCH[1])
    got, plan = _run(ctx, capfd, **opts)
    _check_plan(plan, 0)
    monkeypatch.setenv("CADNIP_F2_FIXED", "0")
    ref, plan0 = _run(ctx, capfd, **opts)
    _check_plan(plan0, 0)
    assert _same(got, ref)


def test_ineligible_circuit_takes_the_generic_form(monkeypatch, capfd):
    """tests/circuits.py: rc_charge is lean (a source, a resistor, a capacitor) but has three unknowns, too few for a dense core of 8."""
    _env(monkeypatch, 1)
    ctx = _setup("rc_charge", 9)
    got, plan = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan, 0)
    assert " nc 0 " in plan[0], plan
    monkeypatch.setenv("CADNIP_F2_FIXED", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan0, 0)
    assert _same(got, ref)
