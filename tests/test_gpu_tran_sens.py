"""Forward parameter sensitivities of the transient on the GPU (csrc/tran_sens.hip; cadnip_tran_set_sens, api.tran(..., sens=)).

(a) Forced grid (the conventions of tests/tran_exact_cases.py: ``err_mask`` zero, ``breaks=()``, exact-double grids, save times on and off
    the grid): the stage against ``direct_dense`` of tests/tran_sens_ref.py -- the same recursion in dense extended-precision numpy on the
    literal oracle's equations, at the same parameter steps -- as scaled sensitivities p ds/dp with ``rel_err`` of tran_exact_cases.  Bound:
    REL_TOL_GPU, the project's 1e-9; differencing residuals in double arithmetic costs less (tran_sens_ref.AMP, measured on the CPU).
(b) Error control with break points: the time loop is undisturbed (states, counters, statuses bit for bit those of the run without
    ``sens``), and a group's sensitivities do not depend on the batch around it.
(c) Group and block indexing: 131 groups of 4, 5 groups of 6, against the closed form of the backward-Euler recursion.
(d) Error-controlled RC against the closed form of the continuous problem, bounded by the state's own discretisation error.
(e) Handle hygiene: set, clear, set again; refusals keep the previous setting; a run after the setting is gone equals a fresh handle's."""
import numpy as np
import pytest

from cadnip_jl_amd import api, hip
from tests import tran_exact_cases as X
from tests import tran_sens_cases as K
from tests import tran_sens_ref as SR

pytestmark = pytest.mark.gpu
REL_TOL = X.REL_TOL_GPU


def _groups(G, k):
    per = 2 + 2 * k
    return np.arange(G * per, dtype=np.int32).reshape(G, per), per


def _forced_run(name, order, B, make=None, points=None, sens=None, max_order=None):
    """the forced-grid run of B points of a case on the expanded batch: (out [B, n_save, n], s [B, K, n_save, n], flags, per, stats, ts, on)"""
    case = K.CASES[name]
    points = case.points[:B] if points is None else points
    sens = K.SENS[name] if sens is None else sens
    mc = api.MNACircuit((make or case.make)(), K.DEFAULTS[name])
    ts, on = case.save_times()
    _, _, steps, expanded, per = api.sens_prepare(mc, points, sens, SR.REL_STEP, (case.t0, case.t1))
    members, per_ = _groups(len(points), len(sens))
    assert per == per_
    sim = api.BatchSimulator(mc, expanded)
    try:
        st = sim.st
        sim.analyze()
        start = np.zeros((len(points), st.n)) if case.start == "zero" else np.array([X.start_state(case, i) for i in range(len(points))])
        sim.h.set_spec(mode="tranop")
        sim.h.set_u(np.repeat(start, per, axis=0))
        sim.h.tran_set_sens(members, steps, len(ts), None, order)
        sim.h.tran_sens_init(zero=case.start == "zero")
        sim.h.set_spec(mode="tran")
        out, pi, stats = sim.h.tran_run(case.t0, case.t1, case.tau, case.tau, breaks=(), save_t=ts, obs=None, h0=case.h0, hmax=case.hmax,
                                        max_newton=case.max_newton, max_order=order, use_pcnr=False, newton_tol=1.0, fused=1,
                                        err_mask=np.zeros(st.n), newton_mode=0, step_rule=0)
        s, flags = sim.h.tran_sens_get()
    finally:
        sim.close()
    base = members[:, 0]
    return out[base], s, flags, pi, stats, ts, on, base


def _forced_params():
    return [pytest.param(c.name, k, id="%s-order%d" % (c.name, k)) for c in K.CASES.values() for k in c.orders]


@pytest.mark.parametrize("name,order", _forced_params())
def test_sensitivities_on_a_forced_grid_match_the_dense_recursion(name, order):
    case = K.CASES[name]
    B = len(case.points)
    out, s, flags, pi, stats, ts, on, base = _forced_run(name, order, B)
    assert stats["n_failed"] == 0 and not flags.any()
    # the bases walk the schedule, every parked member stands still with status 1 (fused = 1 was asked for: the per-op kernels ran all the same)
    parked = np.setdiff1d(np.arange(pi.shape[0]), base)
    assert np.all(pi[base, 1] == case.n_steps) and np.all(pi[base, 2] == 0) and np.all(pi[base, 3] == 1), pi[base].tolist()
    assert np.all(pi[parked, :3] == 0) and np.all(pi[parked, 3] == 1)
    grid, _ = case.schedule(order)
    for i in case.checked:
        e_u = float(X.rel_err(out[i], K.trajectory(name, order, i).sample(ts)).max())
        ref = SR.sample(grid, K.direct(name, order, i), ts)
        sc = K.scales_of(name, i)[:, None, None]
        e = X.rel_err(s[i] * sc, ref * sc)
        e_on, e_off = float(e[:, on].max()), float(e[:, ~on].max())
        print("%s order %d instance %d: states %.2e, scaled sensitivities on grid %.2e, off grid %.2e (max |p ds/dp| %.3g)"
              % (name, order, i, e_u, e_on, e_off, np.abs(ref * sc).max()))
        assert e_u <= REL_TOL, (name, order, i, e_u)
        assert e_on <= REL_TOL, (name, order, i, e_on)
        assert e_off <= REL_TOL, (name, order, i, e_off)


# ---- (b) error control, break points ------------------------------------------------------------------------------------------------------
EC_POINTS = [{"R": 1e3, "C": 1e-6, "V": 5.0}, {"R": 3e3, "C": 1e-6, "V": 2.0}, {"R": 1e3, "C": 0.2e-6, "V": 4.0}]     # tau = 1, 3, 0.2 ms
EC_TSPAN = (0.0, 2.5e-3)
EC_SAVE = np.linspace(0.0, 2.5e-3, 41)
EC_KW = dict(initializealg="uic", warmup_dt=1e-7, max_order=2)


def _ec_run(sim, sens):
    kw = dict(EC_KW)
    if sens:
        kw["sens"] = sens
    return sim.tran(EC_TSPAN, 1e-9, 1e-6, EC_SAVE, **kw)


@pytest.fixture(scope="module")
def ec_runs():
    mc = api.MNACircuit(K.rc_pulse(), K.RC_DEFAULTS)
    sim = api.BatchSimulator(mc, EC_POINTS)
    try:
        sim.analyze()
        plain = _ec_run(sim, None)
        with_s = _ec_run(sim, ["R", "C"])
        sample = sim.pivot_sample
    finally:
        sim.close()
    alone = []
    for pt in EC_POINTS:
        one = api.BatchSimulator(mc, [pt])
        try:
            one.analyze(sample=sample)
            alone.append(_ec_run(one, ["R", "C"]))
        finally:
            one.close()
    return plain, with_s, alone


def test_the_time_loop_is_undisturbed(ec_runs):
    (out0, per0, st0), (out1, per1, st1), _ = ec_runs
    assert "sens" not in st0 and st1["sens_params"] == 2
    assert np.all(per0[:, 3] == 1) and per0[:, 2].sum() > 0 and len(set(per0[:, 1].tolist())) == 3     # rejections happen, three different step sequences
    assert np.array_equal(out0, out1)
    assert np.array_equal(per0, per1)
    assert np.all(np.isfinite(st1["sens"])) and not st1["sens_flag"].any() and np.abs(st1["sens"]).max() > 0


def test_a_group_does_not_depend_on_the_batch_around_it(ec_runs):
    _, (out1, per1, st1), alone = ec_runs
    for i, (out_a, per_a, st_a) in enumerate(alone):
        assert np.array_equal(out_a[0], out1[i]) and np.array_equal(per_a[0], per1[i])
        assert np.array_equal(st_a["sens"][0], st1["sens"][i]), i


# ---- (c) group and block indexing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sens", [(131, ["C"]), (5, ["C", "V"])], ids=["B131-K1", "B5-K2"])
def test_group_and_block_indexing(B, sens):
    """Every group of a large batch against the closed form.  F is linear in C and in V, so the central differences in them are exact (first
    solve and defect pass alike: (C + d)(u' + d s') - (C - d)(u' - d s') = 2 d (u' + C s')) and the stage gives the derivative itself."""
    case = K.CASES["rc"]
    points = [{"R": 1e3 * (1.0 + i / 131.0), "C": 1e-6 * (1.0 + (i % 7) / 7.0), "V": 5.0 - (i % 3)} for i in range(B)]
    out, s, flags, pi, stats, ts, on, base = _forced_run("rc", 1, B, points=points, sens=sens)
    assert stats["n_failed"] == 0 and not flags.any() and s.shape[:2] == (B, len(sens))
    grid, _ = case.schedule(1)
    v, _, dC, dV = K.be_closed_form(points, grid)
    j = api.discover(case.make(), points[0]).index_of("out")
    at = np.searchsorted(grid, ts[on])
    assert np.array_equal(grid[at], ts[on])
    assert float(X.rel_err(out[:, on, j], v[:, at].astype(float)).max()) <= REL_TOL
    for k, nm in enumerate(sens):
        p = np.array([pt[nm] for pt in points])[:, None]
        ref = {"C": dC, "V": dV}[nm][:, at].astype(float)
        e = float(X.rel_err(s[:, k, on, j] * p, ref * p).max())
        print("B %d, d/d%s: worst scaled error over all groups %.2e" % (B, nm, e))
        assert e <= REL_TOL, (B, nm, e)


# ---- (d) error-controlled RC against the continuous closed form -----------------------------------------------------------------------------
# worst |v(out) - V (1 - exp(-t / RC))| over the save times of api.tran on the RC charge circuit (R = 1 kOhm, C = 1 uF, V = 5 V, 0 .. 3 ms,
# abstol 1e-9, reltol 1e-5, "uic" from zero) -- measured on the transient as it stood before this stage existed; the bases of a run with
# ``sens`` repeat that run bit for bit (test_the_time_loop_is_undisturbed).  Measured 6.914685e-04 (91 accepted steps, one rejected); with
# ``sens`` the same run gave R dv/dR 9.669e-04 and C dv/dC 9.668e-04 against their closed forms
E_STATE = 6.92e-4


def test_error_controlled_rc_against_the_closed_form():
    p = K.RC_DEFAULTS
    tau = p["R"] * p["C"]
    ts = np.linspace(0.0, 3e-3, 31)
    sol = api.tran(api.MNACircuit(K.rc_param(), p), (0.0, 3e-3), abstol=1e-9, reltol=1e-5, saveat=ts, initializealg="uic", warmup_dt=1e-7,
                   sens=["R", "C"])
    assert sol.retcode == "Success" and sol.sens_flag == 0 and sol.sens_params == ["R", "C"] and sol.sens.shape == (2, ts.size, sol.st.n)
    x = ts / tau
    e_state = float(np.abs(sol["out"] - p["V"] * (1.0 - np.exp(-x))).max())
    # R dv/dR = C dv/dC = -V (t / tau) exp(-t / tau)
    ref = -p["V"] * x * np.exp(-x)
    e_r = float(np.abs(p["R"] * sol.sensitivity("out", "R") - ref).max())
    e_c = float(np.abs(p["C"] * sol.sensitivity("out", "C") - ref).max())
    print("error-controlled rc: state %.3e (recorded %r), R dv/dR %.3e, C dv/dC %.3e" % (e_state, E_STATE, e_r, e_c))
    assert e_state <= E_STATE
    assert e_r <= 16 * E_STATE and e_c <= 16 * E_STATE


# ---- (e) handle hygiene ---------------------------------------------------------------------------------------------------------------------
def test_handle_hygiene():
    case = K.CASES["rc"]
    mc = api.MNACircuit(case.make(), K.RC_DEFAULTS)
    ts, _ = case.save_times()
    run = lambda h, n: h.tran_run(case.t0, case.t1, 1e-9, 1e-6, breaks=(), save_t=ts, h0=case.h0, hmax=case.hmax, max_order=2, fused=0)

    def fresh(points):
        sim = api.BatchSimulator(mc, points)
        sim.analyze()
        sim.h.set_spec(mode="tran")
        sim.h.set_u(np.zeros((len(points), sim.st.n)))
        return sim

    _, _, steps1, exp1, per1 = api.sens_prepare(mc, [K.RC_POINTS[0]] * 2, ["R"], SR.REL_STEP, (case.t0, case.t1))
    _, _, steps2, exp2, per2 = api.sens_prepare(mc, [K.RC_POINTS[0]], ["R", "C", "V"], SR.REL_STEP, (case.t0, case.t1))
    assert len(exp1) == len(exp2) == 8
    sim = fresh(exp1)
    ref = fresh(exp1)
    try:
        h, n = sim.h, sim.st.n
        zero = dict(n_group=0, K=0, per=0, nh=0, n_save=0, n_obs=0)
        assert h.tran_sens_info() == zero
        h.tran_set_sens(_groups(2, 1)[0], steps1, len(ts))
        assert h.tran_sens_info() == dict(n_group=2, K=1, per=4, nh=3, n_save=len(ts), n_obs=n)
        # refusals keep the setting: an index out of range, an instance in two groups, a step that is not positive and finite, results beyond 256 MiB
        bad = _groups(2, 1)[0].copy()
        bad[1, 3] = 8
        twice = _groups(2, 1)[0].copy()
        twice[1, 0] = 0
        for mem, dl, n_save in ((bad, steps1, len(ts)), (twice, steps1, len(ts)), (_groups(2, 1)[0], steps1 * 0.0, len(ts)),
                                (_groups(2, 1)[0], steps1 * np.inf, len(ts)), (_groups(2, 1)[0], steps1, 1 << 26)):
            with pytest.raises(hip.CadnipError) as ei:
                h.tran_set_sens(mem, dl, n_save)
            assert ei.value.code == hip.BADARG and h.tran_sens_info()["n_group"] == 2
        # the two settings exclude each other, in both orders
        rp, ci = np.asarray(sim.st.rowptr), np.asarray(sim.st.colidx)
        row0 = int(np.searchsorted(rp, 0, side="right") - 1)
        delay = dict(pos=[0], term_pos=[0], term_row=[row0], term_col=[int(ci[0])], tau=[1e-3], w=[0.0])
        with pytest.raises(hip.CadnipError):
            h.tran_set_delay(**delay)
        h.tran_clear_sens()
        assert h.tran_sens_info() == zero
        h.tran_set_delay(**delay)
        with pytest.raises(hip.CadnipError):
            h.tran_set_sens(_groups(2, 1)[0], steps1, len(ts))
        h.tran_clear_delay()
        # a run needs s(t0), and the sizes the spec was made for
        h.tran_set_sens(_groups(2, 1)[0], steps1, len(ts))
        with pytest.raises(hip.CadnipError) as ei:
            run(h, n)
        assert ei.value.code == hip.NOTREADY
        h.tran_sens_init(zero=True)
        out_s, per_s, _ = run(h, n)
        s1, f1 = h.tran_sens_get()
        assert s1.shape == (2, 1, len(ts), n) and not f1.any() and np.array_equal(s1[0], s1[1]) and np.abs(s1).max() > 0
        # another K on the same handle (the parameters of the instances are set again to match)
        h.set_params(api.pack_params(sim.st, mc.circuit, *_par_arrays(mc, exp2), len(exp2), gmin=mc.spec.gmin, tnom_c=mc.spec.tnom))
        h.tran_set_sens(_groups(1, 3)[0], steps2, len(ts))
        assert h.tran_sens_info() == dict(n_group=1, K=3, per=8, nh=3, n_save=len(ts), n_obs=n)
        h.set_u(np.zeros((8, n)))
        h.tran_sens_init(zero=True)
        run(h, n)
        s2, f2 = h.tran_sens_get()
        assert s2.shape == (1, 3, len(ts), n) and not f2.any() and np.array_equal(s2[0, 0], s1[0, 0])
        # with the setting gone the handle is a fresh one's equal
        h.tran_clear_sens()
        h.set_params(api.pack_params(sim.st, mc.circuit, *_par_arrays(mc, exp1), len(exp1), gmin=mc.spec.gmin, tnom_c=mc.spec.tnom))
        h.set_u(np.zeros((8, n)))
        out_a, per_a, _ = run(h, n)
        out_b, per_b, _ = run(ref.h, n)
        assert np.array_equal(out_a, out_b) and np.array_equal(per_a, per_b)
        assert np.array_equal(out_s[0], out_b[0]) and np.array_equal(per_s[0], per_b[0])
    finally:
        sim.close()
        ref.close()


def _par_arrays(mc, points):
    """(params {name: [B]}, temps [B]) of a point list, as BatchSimulator lays them out"""
    params = {k: np.array([float(pt.get(k, v)) for pt in points]) for k, v in mc.params.items()}
    return params, np.array([float(pt.get("temp", mc.spec.temp)) for pt in points])
