"""The sweep kernel's linear solve from PRE-DECODED step descriptors (csrc/lds_layout.hpp: lds_step_predecode; fused2_kernel.hpp:
run_steps_pd): k_fused2 converts the packed descriptors while it stages them -- byte offsets, per-lane trash entries for the lanes that do
not lead their group, one flag byte per lane and step -- and runs the same arithmetic on the same words.

Per instance the fused transient is held to the CPU port (tests/port_util.py): the same Newton, accepted-step and rejected-step counts and
every recorded unknown within the 1e-9 relative bound of tests/test_gpu_tran_parity.py (REL_TOL there, relative to max(|value|, 1)).
Circuits: the inverter and chain17 of tests/circuits.py and the flip-flop at B = 9; CADNIP_F2_WPB = 1, 2, 4, 8; Newton modes 0 and 1.
CADNIP_F2_WPB caps the waves per workgroup and the plan halves them while a workgroup per compute unit still holds the batch, so the
inverter and chain17 run at the smallest batch that keeps the requested width on a 256-CU device (9, 300, 700, 1100 instances; a smaller
device only takes a wider workgroup than asked for earlier); the flip-flop at B = 9 runs k_fused2<1> on nine workgroups whatever the cap.

The plan line of CADNIP_F2_DEBUG=1 is read back.  It shows that the inverter and chain17 of tests/circuits.py do NOT reach the step
program: the plan (fused2.hip: fused2_blocks decides what is lean) gives them the full-table variant with its pass program under full
Newton, and the driver the per-op kernels under Newton mode 1.  They stay as the cases that were asked
for -- held to the port like the others -- and the benchmark's inverter (cadnip_jl_amd.benchmarks.inverter_circuit, lean) is added at the
same four batch sizes, so that k_fused2<1 | 2 | 4 | 8> do run from pre-decoded descriptors; for it and for the flip-flop the plan line must
name the lean variant and the pre-decoded form."""
import re

import numpy as np
import pytest

from cadnip_jl_amd import api, benchmarks as bm
from cadnip_jl_amd.structure import expand_breakpoints
from tests import circuits as tc
from tests.port_util import make_port, analyze_port
from tests.test_gpu_tran_parity import REL_TOL, ABSTOL

pytestmark = pytest.mark.gpu

# name: (circuit factory, default parameters, swept parameter and its range, time span)
CASES = {
    "inverter": (tc.ALL_STAMP["inverter"][0], {}, None, (0.0, 1e-7)),
    "chain17": (tc.CHAIN_STAMP["chain17"][0], {"vdd": 1.0}, ("vdd", 0.9, 1.1), (0.0, 1e-7)),
    "dff": (bm.dff_circuit, {"vdd": 5.0}, ("vdd", 4.5, 5.5), bm.DFF_TSPAN),
    "bench_inverter": (bm.inverter_circuit, {"vdd": 5.0}, ("vdd", 4.5, 5.5), (0.0, 4e-7)),
}
LEAN = ("dff", "bench_inverter")      # circuits the plan gives the sweep kernel's lean variant, the one that runs from step descriptors
BATCH = {1: 9, 2: 300, 4: 700, 8: 1100}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _close_simulators():
    yield
    for ctx in _cache.values():
        ctx["sim"].close()
    _cache.clear()


def _points(name, B):
    _, _, swept, _ = CASES[name]
    rng = np.random.default_rng(B)
    temps = -40.0 + 165.0 * rng.random(B)
    if swept is None:
        return [{"temp": float(t)} for t in temps]
    key, lo, hi = swept
    return [{key: float(v), "temp": float(t)} for v, t in zip(lo + (hi - lo) * rng.random(B), temps)]


def _setup(name, B):
    """One simulator per (circuit, batch): DC start states, save times and the port's reference runs are computed once and shared."""
    if (name, B) in _cache:
        return _cache[(name, B)]
    mk, params, swept, tspan = CASES[name]
    circ = mk()
    pts = _points(name, B)
    sim = api.BatchSimulator(api.MNACircuit(circ, params), pts)
    st = sim.st
    sim.analyze()
    u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
    assert np.all(conv)
    ctx = dict(sim=sim, st=st, circ=circ, pts=pts, u0=u0, tspan=tspan, ts=np.linspace(tspan[0], tspan[1], 15), obs=list(range(st.n_nodes)),
               atol=st.state_abstol(**ABSTOL), breaks=expand_breakpoints(st.breakpoints, tspan), refs={}, vscale=sim.vscale())
    sim.h.set_spec(mode="tran")
    _cache[(name, B)] = ctx
    return ctx


def _port_ref(name, ctx, i, newton_mode):
    """(newton_mode: the port's -- 1 mirrors the fused kernels' Jacobian reuse, 2 the per-op kernels, which refactor every round)"""
    if (i, newton_mode) not in ctx["refs"]:
        _, params, swept, tspan = CASES[name]
        pt = ctx["pts"][i]
        p = dict(params)
        if swept is not None:
            p[swept[0]] = pt[swept[0]]
        pst, port = make_port(ctx["circ"], p, pt["temp"], "tran")
        analyze_port(pst, port, ctx["vscale"])
        ref, _, rst, _ = port.tran(ctx["u0"][i], tspan[0], tspan[1], ctx["atol"], 1e-4, breaks=ctx["breaks"], save_t=ctx["ts"], obs=ctx["obs"],
                                   err_mask=pst.differential_mask(), use_pcnr=False, newton_mode=newton_mode)
        port.close()
        assert rst["status"] == 1
        ctx["refs"][(i, newton_mode)] = (ref, rst)
    return ctx["refs"][(i, newton_mode)]


def _run(ctx, newton_mode, capfd):
    """One fused transient from the shared DC state; returns outputs, per-instance counters and the plan lines the launches printed."""
    sim = ctx["sim"]
    sim.h.set_u(ctx["u0"])
    capfd.readouterr()
    out, per, stats = sim.h.tran_run(ctx["tspan"][0], ctx["tspan"][1], ctx["atol"], 1e-4, breaks=ctx["breaks"], save_t=ctx["ts"], obs=ctx["obs"],
                                     fused=1, newton_mode=newton_mode)
    plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[cadnip f2]")]
    assert stats["n_failed"] == 0
    return out, per, plan


def _env(monkeypatch, wpb):
    monkeypatch.setenv("CADNIP_F2_TEAM", "0")            # one wave per instance at every batch size: the sweep kernel
    monkeypatch.setenv("CADNIP_F2_WPB", str(wpb))
    monkeypatch.setenv("CADNIP_F2_DEBUG", "1")


def _check_plan(plan, wpb_max, fmt):
    assert plan and all("variant 0" in ln and "(%s)" % fmt in ln for ln in plan), plan
    got = {int(re.search(r"wpb (\d+)", ln).group(1)) for ln in plan}
    assert len(got) == 1 and got.pop() <= wpb_max, plan


@pytest.mark.parametrize("newton_mode", [0, 1])
@pytest.mark.parametrize("wpb", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["inverter", "chain17", "dff", "bench_inverter"])
def test_predecoded_steps_match_port(name, wpb, newton_mode, monkeypatch, capfd):
    """Counts equal to the port's and 1e-9 on every node, at every workgroup width; on the lean circuits from the pre-decoded descriptors."""
    _env(monkeypatch, wpb)
    B = 9 if name == "dff" else BATCH[wpb]
    ctx = _setup(name, B)
    out, per, plan = _run(ctx, newton_mode, capfd)
    if name in LEAN:
        _check_plan(plan, wpb, "pre-decoded")
    else:
        assert not any("(pre-decoded)" in ln for ln in plan), plan      # (the full-table variant has no step descriptors)
    # no plan line: the driver gave a circuit outside the lean device set the per-op kernels (Newton mode 1), whose policy is the port's mode 2
    port_mode = newton_mode if plan or not newton_mode else 2
    for i in (range(B) if name == "dff" else sorted({0, B // 2, B - 1})):
        ref, rst = _port_ref(name, ctx, i, port_mode)
        err = np.max(np.abs(out[i] - ref) / np.maximum(np.abs(ref), 1.0))
        print(name, "wpb", wpb, "mode", newton_mode, "instance", i, "gpu", per[i, :3].tolist(), "port", (rst["newton_iters"], rst["accepted"], rst["rejected"]), "err", err)
        assert (per[i, 0], per[i, 1], per[i, 2]) == (rst["newton_iters"], rst["accepted"], rst["rejected"]), (ctx["pts"][i], per[i], rst)
        assert err <= REL_TOL, (ctx["pts"][i], err)


@pytest.mark.parametrize("newton_mode", [0, 1])
@pytest.mark.parametrize("name,B", [("dff", 9), ("bench_inverter", 9), ("bench_inverter", 1100)])
def test_packed_decode_is_kept_and_agrees_to_the_bit(name, B, newton_mode, monkeypatch, capfd):
    """fused2_plan refuses the pre-decoded form when a word of the work array has no 16-bit byte offset (lu_words + n + 66 > 8192) or when
    the flag bytes (1/16 of the descriptors) would cost a resident instance; the kernel then decodes the packed words as before.  None of
    tests/circuits.py: ALL_STAMP qualifies at any workgroup width: the largest of them is the flip-flop (work array of under 2 000
    words; 6 KB of LDS to spare beside eight instances against 1.2 KB of flag bytes), the others have work arrays of a few hundred words.  So the packed decode is
    forced with the plan's diagnostic switch CADNIP_F2_STEPS_PACKED=1 -- on the flip-flop (k_fused2<1>, nine workgroups) and on the
    benchmark's inverter (k_fused2<1> and, at 1100 instances, k_fused2<8> with the in-kernel queue) -- and the two decodes must produce
    the same doubles and the same counters."""
    _env(monkeypatch, 8)
    ctx = _setup(name, B)
    out, per, plan = _run(ctx, newton_mode, capfd)
    _check_plan(plan, 8, "pre-decoded")
    monkeypatch.setenv("CADNIP_F2_STEPS_PACKED", "1")
    out_p, per_p, plan_p = _run(ctx, newton_mode, capfd)
    _check_plan(plan_p, 8, "packed")
    assert np.array_equal(out, out_p) and np.array_equal(per, per_p)
