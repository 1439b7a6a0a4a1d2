"""One Newton update of every kernel form against the oracle (tests/newton_probe_ref.py; the same probes on the CPU port:
tests/test_newton_probe_cpu.py).  The fused kernels stamp, factor and update inside one kernel, so their Jacobian cannot be read; every other
pin they have compares converged results, which a wrong Jacobian entry leaves where they are.  Here `dc_run(maxiters=1)` and a one-step
`tran_run` perform exactly one update u1 = u0 - J(u0)^-1 F(u0), and delta = u0 - u1 is held to the componentwise backward error bound of the
reference module -- the per-op kernels (`fused=0`) as the control under the same bound as every fused form.

Every case asserts the form it claims from the plan line of CADNIP_F2_DEBUG=1 (`variant`, `wpb`, `shape`, `fixed`; the team kernel's line
names its waves; the per-op path prints none) and prints the form, the worst backward ratio and the forward error against u0 - delta_ref
(information only).

Forms.  Lean circuits, by the plan's own ruling (csrc/fused2.hip: fused2_blocks): the inverter, the flip-flop and linear_zoo -- its linear
builtins are all in the lean device set, so it runs variant 0 and the team kernel, not variant 1.  DC probe (modes dcop and tranop, three
states, use_pcnr 0 and 1): per-op; k_fused2<w, true, 0> on the lean circuits, <.., 1> on the others, <.., 2> (CADNIP_F2_NODIRECT=1) on the inverter and `nonlinear`.  Transient probe (three states x three step sizes): per-op in Newton
modes 0 and 1; the sweep kernel (CADNIP_F2_TEAM=0) as variant 0 in modes 0 and 1 (CADNIP_F2_FIXED=0 under mode 1), variant 3 (flip-flop, mode
1, CADNIP_F2_SHAPE=0), variant 4 (flip-flop, mode 1, default), variant 1 (the other circuits, mode 0), variant 2; the team kernel with 2 and 4
waves in both modes on the lean circuits.  B = 9 (one wave per workgroup) everywhere, and the inverter also at B = 1100 (eight waves per
workgroup, the in-kernel queue): the nine corners tiled, every instance checked.

use_pcnr = 1 on a circuit with limit unknowns.  A PCNR run of one solve never converges (no residual test after the last solve), so the DC
chain (csrc/dc_chain.hpp) goes on to stage 1 -- plain Newton from the caller's start point on the per-op kernels -- and `take_all` replaces
stage 0's end state by stage 1's.  What dc_run returns there is the plain per-op update, whatever `fused` says; it is checked as that, and
the run log must show stage 0 in the claimed kernel (one solve, not converged) and stage 1 (one solve).  The PCNR overwrite of the limit
slots is therefore not visible from this call; it is checked on the port, whose `dc` has no chain.  (On the circuits without limit unknowns
there is no stage 1 and use_pcnr changes nothing.)

Counters of the transient probe: one Newton iteration, one accepted step, no rejection, status 1 (per[:, 3] is the instance's status, done),
no Newton failure in the run's totals."""
import numpy as np
import pytest

from cadnip_jl_amd import api
from tests import newton_probe_ref as NP
from tests.test_gpu_fused_shape import _field, _check_plan

pytestmark = pytest.mark.gpu

WIDE = 1100           # tests/test_gpu_fused_steps.BATCH[8]: the smallest batch that keeps eight waves per workgroup on 256 compute units
_sims = {}


@pytest.fixture(scope="module", autouse=True)
def _close_simulators():
    yield
    for sim in _sims.values():
        sim.close()
    _sims.clear()


def _sim(name, B):
    if (name, B) not in _sims:
        pts = NP.points(name)
        sim = api.BatchSimulator(api.MNACircuit(NP.make(name), NP.params_of(pts[0])), [pts[i % NP.N_CORNERS] for i in range(B)])
        sim.analyze()
        _sims[(name, B)] = sim
    return _sims[(name, B)]


# form: (fused, environment, plan): plan = None (per-op: no plan line), ("team", waves) or ("sweep", variant, shape, fixed)
def _sweep(variant, shape=0, fixed=0, **env):
    e = {"CADNIP_F2_TEAM": "0"}
    e.update(env)
    return (1, e, ("sweep", variant, shape, fixed))


FORMS = {
    "per-op": (0, {}, None),
    "v0": _sweep(0, CADNIP_F2_FIXED="0"),
    "v1": _sweep(1),
    "v2": _sweep(2, CADNIP_F2_NODIRECT="1"),
    "v3": _sweep(0, 0, 1, CADNIP_F2_SHAPE="0"),          # the fixed form: family `variant 0`, fixed 1
    "v4": _sweep(0, 1, 1),                               # the shape form: shape 1 fixed 1
    "team2": (1, {"CADNIP_F2_TEAM": "2"}, ("team", 2)),
    "team4": (1, {"CADNIP_F2_TEAM": "4"}, ("team", 4)),
}
SWITCHES = ("CADNIP_F2_TEAM", "CADNIP_F2_WPB", "CADNIP_F2_NODIRECT", "CADNIP_F2_FIXED", "CADNIP_F2_SHAPE", "CADNIP_F2_STEPS_PACKED", "CADNIP_F2_SRC_CACHE")


def _enter(form, monkeypatch):
    fused, env, plan = FORMS[form]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("CADNIP_F2_DEBUG", "1")
    return fused, plan


def _assert_form(lines, plan, wpb):
    """the plan lines of one call against the form the case claims"""
    if plan is None:
        assert not lines, lines
    elif plan[0] == "team":
        assert lines and all(ln.startswith("[cadnip f2] team of %d waves:" % plan[1]) for ln in lines), lines
    else:
        assert lines and all(ln.startswith("[cadnip f2] B ") for ln in lines), lines
        _check_plan(lines, plan[2], wpb, variant=plan[1])
        assert _field(lines, "fixed") == plan[3], lines


def _plan_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[cadnip f2]")]


DC_CASES = [(n, 9, "per-op") for n in NP.CIRCUITS] + [(n, 9, "v0") for n in NP.LEAN] + [(n, 9, "v1") for n in NP.NON_LEAN] + \
    [("inverter", 9, "v2"), ("nonlinear", 9, "v2")] + [("inverter", WIDE, f) for f in ("per-op", "v0", "v2")]


@pytest.mark.parametrize("name,B,form", DC_CASES, ids=["%s-%d-%s" % c for c in DC_CASES])
def test_dc_probe(name, B, form, monkeypatch, capfd):
    fused, plan = _enter(form, monkeypatch)
    sim = _sim(name, B)
    st = sim.st
    worst = (0.0, None, 0.0)
    for probe in [p for p in NP.PROBES if p[0] == "dc"]:
        u0 = NP.start_states(name, probe, B)
        for pcnr in (0, 1):
            sim.h.set_spec(mode=probe[1])
            capfd.readouterr()
            u1, conv, stats = sim.h.dc_run(u0, abstol=1e-300, maxiters=1, use_pcnr=bool(pcnr), cold_start=False, use_stepping=False, fused=fused)
            lines = _plan_lines(capfd)
            _assert_form(lines, plan, 8 if B == WIDE else 1)
            assert not conv.any() and stats["n_failed"] == B
            log = sim.h.dc_log()
            chained = bool(pcnr) and st.n_limits > 0
            want = [(i, 0, False, 1) for i in range(B)] + ([(i, 1, False, 1) for i in range(B)] if chained else [])
            assert [(i, stg, ok, it) for i, stg, _, ok, it in log] == want, log[:4]
            r, where, fwd, _ = NP.check_batch(name, probe, u1, pcnr=False)
            worst = (max(worst[0], r), (probe[1], probe[2], pcnr) + where if r >= worst[0] else worst[1], max(worst[2], fwd))
            assert r <= 1.0, (name, form, probe, pcnr, r, where, NP.unknown_name(st, where[1]))
    print("DC probe        %-18s B %4d %-7s worst backward ratio %.3g at (mode, state, pcnr, instance, row) %s, forward error %.3g"
          % (name, B, form, worst[0], worst[1], worst[2]))


def _tran_cases():
    c = [(n, 9, "per-op", m) for n in NP.CIRCUITS for m in (0, 1)] + [("inverter", WIDE, "per-op", 0)]
    c += [(n, 9, "v0", m) for n in NP.LEAN for m in (0, 1)] + [("inverter", WIDE, "v0", m) for m in (0, 1)]
    c += [("dff", 9, "v3", 1), ("dff", 9, "v4", 1)]
    c += [(n, 9, "v1", 0) for n in NP.NON_LEAN]
    c += [("inverter", 9, "v2", 0), ("nonlinear", 9, "v2", 0), ("inverter", WIDE, "v2", 0)]
    c += [(n, 9, f, m) for n in NP.LEAN for f in ("team2", "team4") for m in (0, 1)]
    return c


TRAN_CASES = _tran_cases()


@pytest.mark.parametrize("name,B,form,newton_mode", TRAN_CASES, ids=["%s-%d-%s-mode%d" % c for c in TRAN_CASES])
def test_transient_probe(name, B, form, newton_mode, monkeypatch, capfd):
    fused, plan = _enter(form, monkeypatch)
    sim = _sim(name, B)
    st = sim.st
    worst = (0.0, None, 0.0)
    for probe in [p for p in NP.PROBES if p[0] == "tran"]:
        h = probe[3]
        u0 = NP.start_states(name, probe, B)
        sim.h.set_u(u0)
        capfd.readouterr()
        out, per, stats = sim.h.tran_run(NP.T0, NP.T0 + h, 1e30, 1.0, breaks=(), save_t=[NP.T0 + h], h0=h, hmax=h, max_newton=3, newton_tol=1.0,
                                         err_mask=np.zeros(st.n), use_pcnr=False, fused=fused, newton_mode=newton_mode, max_order=2)
        _assert_form(_plan_lines(capfd), plan, 8 if B == WIDE else 1)
        assert stats["n_failed"] == 0 and stats["newton_failures"] == 0
        assert np.array_equal(per, np.tile([1, 1, 0, 1], (B, 1))), per[:4]
        u1 = sim.h.get_u()
        r, where, fwd, _ = NP.check_batch(name, probe, u1)
        worst = (max(worst[0], r), (probe[2], h) + where if r >= worst[0] else worst[1], max(worst[2], fwd))
        assert r <= 1.0, (name, form, newton_mode, probe, r, where, NP.unknown_name(st, where[1]))
    print("transient probe %-18s B %4d %-7s Newton mode %d worst backward ratio %.3g at (state, h, instance, row) %s, forward error %.3g"
          % (name, B, form, newton_mode, worst[0], worst[1], worst[2]))
