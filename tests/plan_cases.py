"""The launch plans of a small matrix of circuits, batch sizes and calls, as the library itself reports them: the `[cadnip f2]` lines of
CADNIP_F2_DEBUG=1 (csrc/fused2.hip: launch_fused2) and the ``info`` of ``Handle.factor_solve``.  tools/make_plan_fixtures.py records them
into tests/golden/launch_plans.json; tests/test_gpu_launch_plan.py runs the same matrix and compares literally.

Per (circuit, B) one simulator: factor_solve with kernel "auto" and every forced kernel, then -- with CADNIP_F2_TEAM unset and 0 -- a fused DC
solve, a fused transient over a span of a few steps under Newton modes 0 and 1, and one fused Newton step.  A call the library refuses is
recorded as its status code; a call that takes the per-op kernels prints no line and is recorded as an empty list.  The lines of one call are
recorded once each, in the order of their first appearance (every launch of a call prints the same line)."""
import contextlib
import os
import sys
import tempfile

import numpy as np

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, benchmarks as bm, hip
from cadnip_jl_amd.structure import expand_breakpoints
from tests import circuits as tc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
SWITCHES = ["CADNIP_F2_" + s for s in ("NODIRECT", "TEAM", "WPB", "STEPS_PACKED", "SRC_CACHE", "FIXED", "SHAPE", "NC", "M1_EARLY")] + \
           ["CADNIP_LU_" + s for s in ("PLAIN", "STEPS", "WPI", "F2S")]
BATCHES = (1, 300, 513, 1100)
TEAMS = (None, "0")


def rc_ladder(sections=120):
    """one step of the linear solve per section: the step list does not fit beside eight instances, the circuit loses the lean variant"""
    c = cj.Circuit("rc ladder %d" % sections)
    c.V("v1", "n0", "0", dc=0.0, wave=("pwl", [0.0, 1e-8, 2e-8], [0.0, 0.0, 1.0]))
    for k in range(sections):
        c.R("r%d" % k, "n%d" % k, "n%d" % (k + 1), 100.0 + k)
        c.C("c%d" % k, "n%d" % (k + 1), "0", 1e-12)
    return c


# name: (circuit factory, default parameters, swept parameter or None, span of the transient)
CIRCUITS = {
    "inverter": (bm.inverter_circuit, {"vdd": 5.0}, "vdd", (0.0, 5e-9)),
    "dff": (bm.dff_circuit, {"vdd": 5.0}, "vdd", (0.0, 5e-9)),
    "diode": (tc.diode_rectifier, {}, None, (0.0, 1e-7)),
    "ladder": (rc_ladder, {}, None, (0.0, 3e-8)),
}
CASES = [(name, B) for name in CIRCUITS for B in BATCHES]


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@contextlib.contextmanager
def _plan_lines(into):
    """the library's `[cadnip f2]` lines (written to file descriptor 2 by C code) of the calls inside"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            lines = [ln for ln in f.read().decode().splitlines() if ln.startswith("[cadnip f2]")]
            into.extend(dict.fromkeys(lines))


def _call(fn):
    """the plan lines of one call, or the status code with which the library refused it"""
    lines = []
    try:
        with _plan_lines(lines):
            fn()
    except hip.CadnipError as e:
        return {"refused": int(e.code)}
    return lines


def _points(swept, B):
    rng = np.random.default_rng(B)
    temps = -40.0 + 165.0 * rng.random(B)
    vdd = 4.5 + rng.random(B)
    return [dict({"temp": float(t)}, **({swept: float(v)} if swept else {})) for v, t in zip(vdd, temps)]


def record(name, B):
    """the plans of one (circuit, B); leaves the environment as it found it"""
    mk, params, swept, tspan = CIRCUITS[name]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES + ["CADNIP_F2_DEBUG"]}
    os.environ["CADNIP_F2_DEBUG"] = "1"
    sim = api.BatchSimulator(api.MNACircuit(mk(), params), _points(swept, B))
    try:
        st, h = sim.st, sim.h
        sim.analyze()
        u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
        assert np.all(conv), (name, B)
        h.set_spec(mode="tran")
        h.rebuild(u0, 0.0)
        out = {"factor_solve": {}}
        for k in hip.LU_KERNELS:
            try:
                out["factor_solve"][k] = h.factor_solve(np.full(B, 1e9), np.ones((B, st.n)), kernel=k)[2]
            except hip.CadnipError as e:
                out["factor_solve"][k] = {"refused": int(e.code)}
        atol = st.state_abstol(vntol=1e-6, iabstol=1e-9, chgtol=1e-6)
        breaks = expand_breakpoints(st.breakpoints, tspan)
        ts = np.linspace(tspan[0], tspan[1], 3)

        def tran(newton_mode):
            h.set_spec(mode="tran")
            h.set_u(u0)
            h.tran_run(tspan[0], tspan[1], atol, 1e-4, breaks=breaks, save_t=ts, obs=[0], fused=1, newton_mode=newton_mode)

        for team in TEAMS:
            if team is None:
                os.environ.pop("CADNIP_F2_TEAM", None)
            else:
                os.environ["CADNIP_F2_TEAM"] = team
            got = {"dc": _call(lambda: sim.dc(abstol=1e-9, mode="tranop", fused=True))}
            got["tran0"] = _call(lambda: tran(0))
            got["tran1"] = _call(lambda: tran(1))
            h.set_spec(mode="tran")
            got["step"] = _call(lambda: h.newton_step(u0, np.zeros_like(u0), 1e9, 0.0, fused=True))
            out["team_unset" if team is None else "team_" + team] = got
        return out
    finally:
        sim.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
