"""Transients of every GPU launch path against textbook BDF on a forced step grid (tests/tran_ref.py): a reference that takes nothing from
the product or from oracle/cpu_port.cpp but the circuit description and the three-line rule of the grid.

Every other transient pin of the suite compares a GPU path with the port, whose controller is a copy of csrc/tran_ctrl.hpp: a wrong
variable-step BDF2 / BDF3 coefficient, start-up order or save-time interpolant would sit on both sides.  Here the step controller's
decisions are switched off (``err_mask`` all zero, ``breaks=()``), so the grid is known in advance, and the reference restates the
discretisation (Lagrange definition, exact rational node differences), the equations (the literal oracle), the solve (dense, pivoted,
refined) and the interpolants.  Cases, grids, tolerances and why Newton mode 1 has windows of its own: tests/tran_exact_cases.py;
tests/test_tran_ref_cpu.py holds the port to 1e-10 on the same inputs.

Launch paths (the forcing of tests/test_gpu_tran_parity.py): fused = 0 the per-op kernels; 1 with CADNIP_F2_TEAM = 0 ``k_fused2`` (with
Newton mode 1 and max_order 2 the fixed form that bench.py times; max_order 3 takes the generic form); 3 / 5 the team kernel with 2 / 4 waves.

Measured on the first green run (worst relative error over instances, unknowns and save times; bound 1e-9): see DESIGN.md section 3."""
import numpy as np
import pytest

from cadnip_jl_amd import api
from tests import tran_exact_cases as X

pytestmark = pytest.mark.gpu
REL_TOL = X.REL_TOL_GPU      # 1e-9: tests/test_gpu_tran_parity.REL_TOL

PATHS = [0, 1, 3, 5]


def _params():
    out = []
    for c in X.CASES.values():
        dff = c.name.startswith("dff")
        for k in c.orders:
            for B in ((3,) if len(c.points) == 3 else (3, 9)):
                for fused in ([0, 1, 5] if dff else PATHS):
                    out.append(pytest.param(c.name, k, B, fused, id="%s-order%d-B%d-fused%d" % (c.name, k, B, fused)))
    return out


@pytest.mark.parametrize("name,order,B,fused", _params())
def test_transient_on_a_forced_grid_matches_textbook_bdf(name, order, B, fused, monkeypatch):
    if fused:
        monkeypatch.setenv("CADNIP_F2_TEAM", str(fused - 1 if fused > 1 else 0))
    case = X.CASES[name]
    points = case.points[:B]
    ts, on = case.save_times()
    grid, orders = case.schedule(order)
    refs = {i: X.reference(name, order, i).sample(ts) for i in case.checked if i < B}     # once per process, shared by the paths

    sim = api.BatchSimulator(api.MNACircuit(case.make(), {"vdd": 5.0} if "vdd" in points[0] else {}), points)
    st = sim.st
    sim.analyze()
    sim.h.set_spec(mode="tran")
    sim.h.set_u(np.array([X.start_state(case, i) for i in range(B)]))
    out, per, stats = sim.h.tran_run(case.t0, case.t1, case.tau, case.tau, breaks=(), save_t=ts, obs=None, h0=case.h0, hmax=case.hmax,
                                     max_newton=case.max_newton, max_order=order, use_pcnr=False, newton_tol=1.0, fused=fused,
                                     err_mask=np.zeros(st.n), newton_mode=case.mode, step_rule=0)
    t_end, _, ord_end = sim.h.tran_state()
    sim.close()

    assert stats["n_failed"] == 0
    # neither fewer nor more steps than the schedule: a Newton failure or a rejection would leave the grid
    assert np.all(per[:, 1] == case.n_steps) and np.all(per[:, 2] == 0) and stats["newton_failures"] == 0, (per.tolist(), stats)
    assert np.all(t_end == case.t1) and np.all(ord_end == orders[-1]), (t_end, ord_end)
    assert out.shape == (B, len(ts), st.n)
    worst_on = worst_off = 0.0
    for i, R in refs.items():
        e = X.rel_err(out[i], R)
        worst_on, worst_off = max(worst_on, float(e[on].max())), max(worst_off, float(e[~on].max()))
    print("%s order %d B %d fused %d: worst error on grid %.2e, off grid %.2e" % (name, order, B, fused, worst_on, worst_off))
    assert worst_on <= REL_TOL, (name, order, B, fused, worst_on)
    assert worst_off <= REL_TOL, (name, order, B, fused, worst_off)
