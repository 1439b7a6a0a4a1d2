"""The register view of the sweep kernel's shape form (csrc/devices.hpp: M1PairView; csrc/fused2_kernel.hpp: k_fused2<WPB, false, 4>): a lane of
the sp_mos1 pass holds its operand offsets and residual words for the launch and its device's parameters for as long as the instance is
resident.  Variant 3 (CADNIP_F2_SHAPE=0) reads all of that from the tables and from memory in every round; the two must agree bit for bit on
the observed waveform, the per-instance counters and the final states.

tests/test_gpu_fused_shape.py holds the two forms together already.  What this file adds is aimed at the view:
  * every instance has its own temperature as well as its own supply (a Vdd x temp corner grid, sweep_shard.rank_points), so the sp_mos1
    parameter rows differ from instance to instance -- asserted on the packed blocks -- and a view that is not reloaded when a wave picks up
    another instance computes something else.  The flip-flop, 0 - 700 ns, Newton mode 1: one instance more than the waves k_fused2<1> keeps
    resident (one wave takes a second instance from the queue), and 16 instances at width 8 (every instance runs beyond the 1 024 rounds of a
    launch, so each is stored at the seam and resumed by whichever wave gets it);
  * the benchmark's inverter: two MOSFETs, so 60 lanes have no device, and the NMOS source and bulk are ground -- the ground operand (the
    constant word 0.0) and the ground residual word (the lane's trash word); 0 - 250 ns covers a rising and a falling input edge.
(A flip-flop with one more inverter, 32 MOSFETs and 250 unknowns, would fill every lane of the pass, but it does not reach the sweep kernel under
Newton mode 1: the driver gives it the per-op kernels, no plan line -- as the 34-MOSFET one of tests/test_gpu_fused_shape.py.)"""
import numpy as np
import pytest

from cadnip_jl_amd import api, benchmarks as bm
from cadnip_jl_amd.structure import expand_breakpoints, pack_params
from cadnip_jl_amd.sweep_shard import rank_points
from tests.test_gpu_tran_parity import ABSTOL
from tests.test_gpu_fused_steps import _env
from tests.test_gpu_fused_fixed import _run
from tests.test_gpu_fused_shape import _field, _check_plan, _resident_plus_one
from tests.test_gpu_fused_steps import _close_simulators  # noqa: F401  (module fixture: closes the simulators _resident_plus_one caches there)

pytestmark = pytest.mark.gpu


# name: (circuit factory, time span)
CIRCUITS = {"dff": (bm.dff_circuit, bm.DFF_TSPAN), "inverter": (bm.inverter_circuit, (0.0, 2.5e-7))}
_sims = {}


@pytest.fixture(scope="module", autouse=True)
def _close_own_simulators():
    yield
    for ctx in _sims.values():
        ctx["sim"].close()
    _sims.clear()


def _corner_points(B):
    """B points of a Vdd x temp corner grid (32 supplies per temperature), spread so that even a few points cover two temperatures"""
    pts, _ = rank_points(max(64, 32 * ((B + 31) // 32)), 0, 1)
    pts = pts[::len(pts) // B][:B]
    assert len(pts) == B and len({p["temp"] for p in pts}) >= 2 and len({p["vdd"] for p in pts}) >= 2
    return pts


def _setup(name, B):
    if (name, B) in _sims:
        return _sims[(name, B)]
    mk, tspan = CIRCUITS[name]
    circ = mk()
    sim = api.BatchSimulator(api.MNACircuit(circ, {"vdd": 5.0}), _corner_points(B))
    st = sim.st
    sim.analyze()
    u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
    assert np.all(conv)
    ctx = dict(sim=sim, st=st, u0=u0, tspan=tspan, ts=np.linspace(tspan[0], tspan[1], 15), obs=list(range(st.n_nodes)),
               atol=st.state_abstol(**ABSTOL), breaks=expand_breakpoints(st.breakpoints, tspan))
    sim.h.set_spec(mode="tran")
    _sims[(name, B)] = ctx
    return ctx


def _mos1_rows_differ(sim):
    """The packed sp_mos1 parameter rows of two instances at different temperatures -- [B, n_par, count], the 34 derived parameters first -- are not
    the same numbers"""
    packed = pack_params(sim.st, sim.mc.circuit, sim.params, sim.temps, sim.B, gmin=sim.mc.spec.gmin, tnom_c=sim.mc.spec.tnom)
    (rows,) = [a for blk, a in zip(sim.st.blocks, packed) if blk.type == "MOS1"]
    temps = np.asarray(sim.temps, dtype=float)
    i, j = 0, int(np.flatnonzero(temps != temps[0])[0])
    return rows.shape[1] >= 34 and not np.array_equal(rows[i, :34], rows[j, :34])


def _both_forms(ctx, capfd, monkeypatch, wpb=None, seam=False):
    monkeypatch.delenv("CADNIP_F2_SHAPE", raising=False)
    got, plan = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan, 1, wpb)
    monkeypatch.setenv("CADNIP_F2_SHAPE", "0")
    ref, plan0 = _run(ctx, capfd, newton_mode=1)
    _check_plan(plan0, 0, wpb)
    assert len(plan0) == len(plan) and _field(plan0, "grid") == _field(plan, "grid")
    if seam:
        assert len(plan) >= 2, plan
        assert np.all(ref[1][:, 0] > 1024), ref[1][:, 0].min()   # every instance ran beyond one launch's budget of rounds
    assert np.all(np.isfinite(ref[0])) and np.ptp(ref[0]) > 0.1
    for k, what in enumerate(("waveform", "per-instance counters", "final states")):
        assert np.array_equal(got[k], ref[k]), what
    return plan


def test_queue_pickup_reloads_the_view(monkeypatch, capfd):
    B = _resident_plus_one(monkeypatch, capfd)
    _env(monkeypatch, 1)
    ctx = _setup("dff", B)
    assert _mos1_rows_differ(ctx["sim"])
    plan = _both_forms(ctx, capfd, monkeypatch, wpb=1, seam=True)
    assert _field(plan, "grid") == B - 1, plan        # one instance waits in the queue


def test_launch_seam_reloads_the_view(monkeypatch, capfd):
    _env(monkeypatch, 8)
    ctx = _setup("dff", 16)
    assert _mos1_rows_differ(ctx["sim"])
    _both_forms(ctx, capfd, monkeypatch, seam=True)


def test_grounded_terminals_and_idle_lanes(monkeypatch, capfd):
    _env(monkeypatch, 2)
    ctx = _setup("inverter", 4)
    assert _mos1_rows_differ(ctx["sim"])
    _both_forms(ctx, capfd, monkeypatch)
