"""Transients with transport delays on the GPU (cadnip_tran_set_delay; csrc/delay.hip, csrc/delay_plan.hpp): the per-op path with the two
delay kernels against the textbook delay-differential reference (tests/tran_delay_ref.py) on a forced step grid, the history ring's
capacity and overflow rule, and the product API (``api.tran(..., delays="history")``) against closed forms.

Forced grid, as tests/test_gpu_tran_exact.py: ``err_mask`` all zero, ``breaks=()``, explicit ``h0`` and ``hmax`` <= the smallest delay, so
the steps are tran_ref.schedule's; bound 1e-9, the project's bound for a GPU path against the textbook reference (worst relative error
over instances, unknowns and save times, |ref| floored at 1).  Every case runs with fused = False and fused = True: a handle with a delay
spec runs per-op whatever ``fused`` says, so the two are equal to the bit.

Measured on the first green run (worst error, bound 1e-9): see DESIGN.md section 9."""
import functools

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip, netlist
from tests import tran_delay_cases as K
from tests import tran_delay_ref as DR
from tests import tran_exact_cases as X
from tests import tran_ref as TR

pytestmark = pytest.mark.gpu
REL_TOL = X.REL_TOL_GPU
TD = K.TD


CASES = {"buffer": K.buffer_case, "line": K.line_case, "inverter": K.inverter_case, "ghf": K.ghf_case}


_tau_tol, _params, _save_times = K.tau_tol, K.case_params, K.save_times


def _set_delay(sim, depth=0):
    """the spec of the simulator's circuit on its handle and the pivot order of G - W: what BatchSimulator.tran does under delays="history" """
    spec = sim.delay_spec()
    sim.h.tran_set_delay(depth=depth, **spec)
    sim.analyze_delayed(spec, 0.0)


@functools.lru_cache(maxsize=None)
def _gpu_run(name, order, fused, depth=0, taus=None):
    """(out [B, S, n], per, start states): the case on the GPU on its forced grid"""
    case = CASES[name]()
    points = case["points"] if taus is None else [{"tau": t} for t in taus]
    sim = api.BatchSimulator(api.MNACircuit(case["make"](), case["base"]), points)
    try:
        sim.analyze()
        if case["start"] == "dc":
            u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
            assert np.all(conv)
        else:
            u0 = np.zeros((sim.B, sim.st.n))
        sim.h.set_spec(mode="tran")
        sim.h.set_u(u0)
        _set_delay(sim, depth)
        tol = _tau_tol(case)
        out, per, stats = sim.h.tran_run(0.0, float(TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], order)[0][-1]), tol, tol, breaks=(),
                                         save_t=_save_times(case, order), h0=case["h0"], hmax=case["hmax"], max_newton=25, max_order=order,
                                         newton_tol=1.0, fused=fused, err_mask=np.zeros(sim.st.n))
        return out, per, u0
    finally:
        sim.close()


@functools.lru_cache(maxsize=None)
def _reference(name, order, i):
    case = CASES[name]()
    deq = DR.DelayedEquations(case["make"](), _params(case, i), case["points"][i].get("temp", 27.0))
    grid, orders = TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], order)
    u0 = _gpu_run(name, order, False)[2][i]
    return DR.integrate(deq, u0, grid, orders).sample(_save_times(case, order))


@pytest.mark.parametrize("name,order", [("buffer", 2), ("buffer", 3), ("line", 2), ("inverter", 2), ("ghf", 2), ("ghf", 3)])
def test_forced_grid_matches_the_delay_differential_reference(name, order):
    case = CASES[name]()
    out, per, _ = _gpu_run(name, order, False)
    assert np.all(per[:, 3] == 1) and np.all(per[:, 1] == case["n_steps"]) and np.all(per[:, 2] == 0), per.tolist()
    worst = 0.0
    for i in range(len(case["points"])):
        ref = _reference(name, order, i)
        assert np.max(np.abs(ref)) <= case["umax"] and np.max(np.abs(ref)) > 0.1
        worst = max(worst, float(np.max(X.rel_err(out[i], ref))))
    print("%s order %d: worst error %.2e" % (name, order, worst))
    assert worst <= REL_TOL, (name, order, worst)
    # fused = True: the same per-op run, to the bit
    out_f, per_f, _ = _gpu_run(name, order, True)
    assert np.array_equal(out_f, out) and np.array_equal(per_f, per)


def test_ring_of_eight_serves_delays_of_up_to_six_steps_to_the_bit():
    out, per, _ = _gpu_run("buffer", 2, False)
    out8, per8, _ = _gpu_run("buffer", 2, False, depth=8)
    assert np.array_equal(out8, out) and np.array_equal(per8, per)


def test_ring_overflow_stops_its_instance_and_nothing_else():
    """depth 4, a delay of 12 final steps at instance 1 only: its look-up falls off the ring as soon as it leaves the pre-history; instances
    0 and 2 (3 and 2.3 steps: four points suffice) are what they are beside a healthy instance 1"""
    hmax = TD / 16
    taus = (3 * hmax, 12 * hmax, 2.3 * hmax)
    out, per, _ = _gpu_run("buffer", 2, False, depth=0, taus=taus)
    assert np.all(per[:, 3] == 1)
    out4, per4, _ = _gpu_run("buffer", 2, False, depth=4, taus=taus)
    assert per4[:, 3].tolist() == [1, hip.TRAN_DELAY_OVERFLOW, 1]
    for i in (0, 2):
        assert np.array_equal(out4[i], out[i]) and np.array_equal(per4[i], per[i])
    assert 0 < per4[1, 1] < per[1, 1]                      # it ran through its pre-history, not to the end


def test_spec_validation_and_clearing():
    case = K.buffer_case()
    sim = api.BatchSimulator(api.MNACircuit(case["make"](), case["base"]), case["points"])
    try:
        good = sim.delay_spec()
        sim.h.tran_set_delay(**good)
        bad_tau = good["tau"].copy()
        bad_tau[1, 0] = 0.0
        for change in (dict(tau=bad_tau), dict(term_col=good["term_col"] + 1), dict(pos=good["pos"] + sim.st.nnz), dict(term_pos=good["term_pos"] + 1)):
            with pytest.raises(hip.CadnipError, match="BADARG"):
                sim.h.tran_set_delay(**dict(good, **change))
        with pytest.raises(hip.CadnipError, match="BADARG"):
            sim.h.tran_set_delay(depth=1, **good)
        with pytest.raises(ValueError):
            sim.h.tran_set_delay(**dict(good, tau=good["tau"][:2]))
        sim.h.tran_clear_delay()
        sim.h.tran_clear_delay()
    finally:
        sim.close()


# ---- the product API, error control on ---------------------------------------------------------------------------------------------------------
LINE_TA, LINE_TB = 0.25 * TD, 0.75 * TD
LINE_SAVE = np.linspace(0.0, 6 * TD, 49)


@pytest.mark.parametrize("rs,rl", [(30.0, 100.0), (50.0, None)], ids=["mismatched", "matched-open"])
def test_api_line_follows_the_lattice_diagram(rs, rl):
    """algebraic and linear, kink images are break points: 1e-9 of the 1 V swing at the save times"""
    mc = api.MNACircuit(K.line(K.pwl_ramp(LINE_TA, LINE_TB), rs, rl), {"td": TD})
    sol = api.tran(mc, (0.0, 6 * TD), saveat=LINE_SAVE, delays="history")
    assert sol.retcode == "Success" and sol.run_stats["delay_breaks"] == 15 and not sol.run_stats["delay_breaks_truncated"]
    near, far = K.lattice(lambda t: K.ramp(t, LINE_TA, LINE_TB), LINE_SAVE, rs, rl, TD)
    e1, e2 = float(np.max(np.abs(sol["p1"] - near))), float(np.max(np.abs(sol["p2"] - far)))
    print("api line rs %g rl %s: near %.2e far %.2e" % (rs, rl, e1, e2))
    assert e1 <= 1e-9 and e2 <= 1e-9


def test_api_buffer_follows_its_closed_form():
    ta, tb, tau = 0.5 * TD, 1.5 * TD, 0.75 * TD
    mc = api.MNACircuit(K.buffer(K.pwl_ramp(ta, tb)), {"tau": tau})
    ts = np.array([1.5, 2.0, 2.25, 3.0, 4.0, 6.0]) * TD
    # hmax: the controller's first step after every break point (four of them here) is an untested backward-Euler step of a tenth of the step
    # before it; its local error h^2 v'' / 2 with v'' = 2 / TD^2 is (h / TD)^2, which at the default hmax = span / 50 (h = 0.012 TD: 1.4e-4)
    # is more than 1e-3 of the first sample (0.058).  With hmax = TD / 32 it is 1e-5.
    sol = api.tran(mc, (0.0, 6 * TD), abstol=1e-9, reltol=1e-6, saveat=ts, delays="history", hmax=TD / 32)
    assert sol.retcode == "Success"
    exact = K.buffer_out(ts, ta, tb, tau)
    assert np.allclose(sol["out"], exact, rtol=1e-3), (sol["out"], exact)


def test_a_deck_with_a_line_gives_the_samples_of_the_circuit_form():
    deck = "* line\nVS s 0 PWL(0 0 0.25n 0 0.75n 1 1 1)\nRS s p1 30\nT1 p1 0 p2 0 Z0=50 TD=1n\nRL p2 0 100\n"
    c, _ = netlist.read_spice(deck)
    ts = np.linspace(0.0, 6e-9, 25)
    a = api.tran(api.MNACircuit(c, {}), (0.0, 6e-9), saveat=ts, delays="history")
    b = api.tran(api.MNACircuit(K.line(("pwl", [0.0, 0.25e-9, 0.75e-9, 1.0], [0.0, 0.0, 1.0, 1.0]), 30.0, 100.0, 1e-9), {}), (0.0, 6e-9), saveat=ts,
                 delays="history")
    assert a.retcode == b.retcode == "Success"
    assert np.array_equal(a["p1"], b["p1"]) and np.array_equal(a["p2"], b["p2"]) and np.max(np.abs(a["p2"])) > 0.7


def test_a_circuit_without_delays_is_untouched_by_the_keyword():
    c = cj.Circuit()
    c.V("v1", "vin", "0", dc=0.0, wave=("pwl", [0.0, 1e-9], [0.0, 5.0]))
    c.R("r1", "vin", "out", 1e3)
    c.C("c1", "out", "0", 1e-6)
    ts = np.linspace(0.0, 2e-3, 9)
    a = api.tran(api.MNACircuit(c), (0.0, 2e-3), abstol=1e-9, reltol=1e-6, saveat=ts)
    b = api.tran(api.MNACircuit(c), (0.0, 2e-3), abstol=1e-9, reltol=1e-6, saveat=ts, delays="history", delay_depth=16)
    assert np.array_equal(a.u, b.u) and a.stats == b.stats and "delay_breaks" not in b.run_stats


def test_a_sweep_over_td_returns_one_solution_per_point():
    mc = api.MNACircuit(K.line(K.pwl_ramp(LINE_TA, LINE_TB), 30.0, 100.0), {"td": TD})
    tds = [TD, 1.5 * TD, 2 * TD]
    res = api.tran(api.CircuitSweep(mc, api.Sweep(td=tds)), (0.0, 6 * TD), saveat=LINE_SAVE, delays="history")
    assert len(res) == 3 and res.stats["delay_breaks"] > 0
    for (pt, sol), td in zip(res, tds):
        assert sol.retcode == "Success" and pt["td"] == td
        near, far = K.lattice(lambda t: K.ramp(t, LINE_TA, LINE_TB), LINE_SAVE, 30.0, 100.0, td)
        assert np.max(np.abs(sol["p2"] - far)) <= 1e-9 and np.max(np.abs(sol["p1"] - near)) <= 1e-9
