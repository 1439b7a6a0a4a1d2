"""Transport delays in the CPU port (oracle/cpu_port.cpp: port_set_delay), pinned without a GPU:

(a) forced grid (the settings of tests/test_gpu_tran_delay._gpu_run: ``err_mask`` zero, ``breaks=()``, explicit ``h0`` and ``hmax``,
    ``newton_tol=1``, ``max_newton=25``): the port against the textbook delay-differential reference (tests/tran_delay_ref.integrate) at
    tran_exact_cases.REL_TOL_PORT = 1e-10 -- buffer (orders 2, 3), ghf (2), the line into the inverter (2);
(b) the depth rule: ``depth = delay_need`` is the unbounded run to the bit, one less ends with status -4, and a delay of twelve steps on two
    kept points ends at the first look-up that leaves the pre-history;
(c) the conditions under which tests/test_gpu_tran_delay_port.py means something -- rejected steps, break-point landings, Newton
    failures, look-ups across more than one interval of the history -- established with the port alone on the error-controlled cases
    (tests/tran_delay_cases.ec_case), so that they cannot silently lapse;
(d) what port_set_delay refuses, and that the port refuses a step beyond its smallest delay (it does not clamp: the caller does).

Measured: worst error against the reference 4.4e-16 .. 2.3e-15; the counts of (c) are in the asserts' messages."""
import functools

import numpy as np
import pytest

import cadnip_jl_amd as cj
from tests import port_util as PU
from tests import tran_delay_cases as K
from tests import tran_delay_ref as DR
from tests import tran_exact_cases as X
from tests import tran_ref as TR

TD = K.TD
CASES = {"buffer": K.buffer_case, "inverter": K.inverter_case, "ghf": K.ghf_case}
VSCALE = {"buffer": 1.0, "ghf": 1.0, "inverter": 5.0}


@functools.lru_cache(maxsize=None)
def _start(name, i):
    case = CASES[name]()
    params, temp = K.case_params(case, i), case["points"][i].get("temp", 27.0)
    if case["start"] == "dc":
        return PU.dense_dc_start(case["make"](), params, temp)
    return np.zeros(cj.discover(case["make"](), params).n)


def _forced(name, order, i, depth=0, tau=None):
    """(out, stats, accepted times) of instance i of a forced-grid case on the port"""
    case = CASES[name]()
    params, temp = K.case_params(case, i), case["points"][i].get("temp", 27.0)
    if tau is not None:
        params = dict(params, tau=tau)
    st, port, _ = PU.make_port_delayed(case["make"](), params, temp, VSCALE[name], depth)
    try:
        grid = TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], order)[0]
        tol = K.tau_tol(case)
        out, _, stats, trace = port.tran(_start(name, i), 0.0, float(grid[-1]), tol, tol, breaks=(), save_t=K.save_times(case, order), err_mask=np.zeros(st.n),
                                         h0=case["h0"], hmax=case["hmax"], max_newton=25, max_order=order, newton_tol=1.0, use_pcnr=False, trace_cap=case["n_steps"] + 1)
        return out, stats, trace
    finally:
        port.close()


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [("buffer", 2), ("buffer", 3), ("ghf", 2), ("inverter", 2)])
def test_forced_grid_port_matches_the_delay_differential_reference(name, order):
    case = CASES[name]()
    grid, orders = TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], order)
    worst = 0.0
    for i, pt in enumerate(case["points"]):
        out, stats, trace = _forced(name, order, i)
        assert (stats["status"], stats["accepted"], stats["rejected"], stats["newton_failures"]) == (1, case["n_steps"], 0, 0), stats
        assert np.array_equal(trace, grid[1:])                                    # the port took the scheduled grid, to the bit
        deq = DR.DelayedEquations(case["make"](), K.case_params(case, i), pt.get("temp", 27.0))
        ref = DR.integrate(deq, _start(name, i), grid, orders).sample(K.save_times(case, order))
        assert 0.1 < np.max(np.abs(ref)) <= case["umax"]
        worst = max(worst, float(np.max(X.rel_err(out, ref))))
    print("%s order %d: port against the reference, worst error %.2e" % (name, order, worst))
    assert worst <= X.REL_TOL_PORT, (name, order, worst)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 2])
def test_depth_of_delay_need_is_the_unbounded_run_and_one_less_overflows(i):
    """buffer, tau = 3 and 2.3 final steps: the look-ups of the constant-step phase reach three points back"""
    out, stats, _ = _forced("buffer", 2, i)
    need = stats["delay_need"]
    assert stats["status"] == 1 and need >= 3, stats
    out_d, stats_d, _ = _forced("buffer", 2, i, depth=need)
    assert np.array_equal(out_d, out) and stats_d["status"] == 1 and stats_d["delay_need"] == need
    assert (stats_d["newton_iters"], stats_d["accepted"]) == (stats["newton_iters"], stats["accepted"])
    _, stats_s, _ = _forced("buffer", 2, i, depth=need - 1)
    assert stats_s["status"] == -4 and 0 < stats_s["accepted"] < stats["accepted"], stats_s


def test_two_kept_points_end_a_long_delay_at_the_first_look_up_past_the_pre_history():
    case = K.buffer_case()
    tau = 12 * case["hmax"]
    grid = TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], 2)[0]
    pre = int(np.sum(grid[1:] - tau <= 0.0))                   # the steps whose look-up is still the start value
    _, stats, trace = _forced("buffer", 2, 1, depth=2, tau=tau)
    assert stats["status"] == -4 and stats["accepted"] == pre and trace[-1] == grid[pre], (stats, pre)
    _, free, _ = _forced("buffer", 2, 1, tau=tau)               # unbounded: the same delay runs through
    assert free["status"] == 1 and free["delay_need"] >= 12


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ec(name):
    """[(stats, number of break points landed on)] per point of an error-controlled case, and the batch's clamped hmax"""
    case = K.ec_case(name)
    circ = case["make"]()
    pts = [K.ec_point(case, i) for i in range(len(case["points"]))]
    st = cj.discover(circ, pts[0][0])
    hb = min(case["hmax"], PU.batch_tau_min(st, circ, [p for p, _ in pts]))
    breaks = PU.ec_breaks(st, circ, [p for p, _ in pts], case)
    ts = PU.ec_save_times(case, breaks)
    res = []
    for p, temp in pts:
        u0 = PU.dense_dc_start(circ, p, temp) if case["start"] == "dc" else np.zeros(st.n)
        for order in ([case["max_order"]] if isinstance(case["max_order"], int) else case["max_order"]):
            _, stats, trace = PU.port_ec_run(case, circ, p, temp, u0, hb, breaks, ts, max_order=order, trace_cap=100000)
            res.append((stats, len(set(trace.tolist()) & set(breaks))))
    return res, hb, breaks


@pytest.mark.parametrize("name", ["buffer_sin", "buffer_sin_five", "buffer_sin_depth", "ghf", "ghf_five", "line_inverter_breaks", "line_inverter_tight_newton"])
def test_every_instance_runs_through_and_looks_across_more_than_one_interval(name):
    res, _, _ = _ec(name)
    print(name, [(s["newton_iters"], s["accepted"], s["rejected"], s["newton_failures"], s["delay_need"], landed) for s, landed in res])
    for s, _ in res:
        assert s["status"] == 1 and s["delay_need"] >= 3, s
        assert 100 <= s["accepted"] <= 400, s                      # "a few hundred steps": the GPU tests stay quick


def test_buffer_sin_rejects_steps_and_its_clamp_binds():
    res, hb, _ = _ec("buffer_sin")
    assert max(s["rejected"] for s, _ in res) >= 1, [s for s, _ in res]
    # the clamp binds: with the case's own hmax the controller of the instance with the smallest delay steps past it, which the port refuses
    case = K.ec_case("buffer_sin")
    assert hb == TD / 32 < case["hmax"]
    p, temp = K.ec_point(case, 1)
    n = cj.discover(case["make"](), p).n
    with pytest.raises(ValueError, match="smallest delay"):
        PU.port_ec_run(case, case["make"](), p, temp, np.zeros(n), case["hmax"], [], PU.ec_save_times(case, []))


def test_line_inverter_lands_on_breaks_and_iterates():
    res, _, breaks = _ec("line_inverter_breaks")
    assert len(breaks) >= 3
    for s, landed in res:
        assert landed >= 3, (landed, breaks)
        assert s["newton_iters"] > 2 * s["accepted"], s


def test_line_inverter_with_three_newton_rounds_fails_and_recovers():
    res, _, _ = _ec("line_inverter_tight_newton")
    assert K.ec_case("line_inverter_tight_newton")["max_newton"] == 3
    for s, _ in res:
        assert s["newton_failures"] >= 1 and s["status"] == 1, s


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------
def test_set_delay_refuses_what_it_cannot_place_and_clears():
    case = K.buffer_case()
    circ, params = case["make"](), K.case_params(case, 0)
    st, port = PU.make_port(circ, params)
    try:
        (r, c, w, tau), = DR.delayed_terms(st, circ, params)
        port.set_delay([(r, c, w, tau)])
        missing = next(j for j in range(st.n) if j not in st.colidx[st.rowptr[r]:st.rowptr[r + 1]])
        for bad in ([(r, missing, w, tau)], [(r, c, w, 0.0)], [(r, c, w, float("inf"))], [(st.n, c, w, tau)]):
            with pytest.raises(ValueError):
                port.set_delay(bad)
        with pytest.raises(ValueError):
            port.set_delay([(r, c, w, tau)], depth=-1)
        # cleared: the transient is the undelayed one again (the E source acts at once)
        port.set_delay([])
        PU.analyze_port(st, port, 1.0)
        kw = dict(save_t=[TD], err_mask=np.zeros(st.n), h0=TD / 64, hmax=TD / 16, newton_tol=1.0, use_pcnr=False)
        a = port.tran(np.zeros(st.n), 0.0, TD, 1e-11, 1e-11, **kw)
        port.set_delay([(r, c, w, tau)])
        port.set_delay([])
        b = port.tran(np.zeros(st.n), 0.0, TD, 1e-11, 1e-11, **kw)
        assert np.array_equal(a[0], b[0]) and b[2]["delay_need"] == 0 and np.max(np.abs(a[0])) > 0.1
    finally:
        port.close()
