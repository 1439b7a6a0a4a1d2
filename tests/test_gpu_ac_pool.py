"""The AC sweeps' shared transfer-buffer pool (csrc/api.hip: ac_sweep; AcState::in / out): slot i of the pool is whatever the running sweep's
i-th transfer is, so a buffer may hold another family's bytes, at another size, when a sweep starts.  Nothing a call returns may depend on
that.  On ONE handle a fixed interleaved sequence makes every slot grow, shrink and change owner; every output of every call is held TO THE
BIT (64-bit patterns: ``same`` of tests/test_gpu_ac_multi.py; flags and info included) against the same call made as the FIRST call of a
fresh handle, whose buffers are newly allocated and zeroed.  The handles are built as tests/test_gpu_ac_lu.py builds its cases
(butterworth: n = 6, B = 1; the flip-flop: B = 3), at the cached case's DC point and pivot sample, never the cached handle itself."""
import numpy as np
import pytest

from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import noise_ref as N
from tests import test_gpu_ac_adjoint as TA
from tests import test_gpu_ac_lu as T
from tests.test_gpu_ac_multi import same

pytestmark = pytest.mark.gpu
GMIN = T.GMIN


def fresh(name):
    """a new handle in the state of T.case(name).h: same instances, same G / C (to the bit), same pivot order"""
    c = T.case(name)
    _, base, pts, _ = R.CASES[name]
    sim = api.BatchSimulator(api.MNACircuit(c.circ, dict(base), api.MNASpec(mode="dcop")), pts if pts != [{}] else None)
    sim.h.set_spec(mode="dcop")
    sim.h.rebuild(c.u, 0.0)
    G, Cm, _, _ = sim.h.get_GCb()
    to_ref = np.asarray(c.st.to_ref_nz)
    assert np.array_equal(G[:, to_ref], c.G) and np.array_equal(Cm[:, to_ref], c.C)
    sim.h.analyze_values(c.sample_ref)
    return sim


def equal(got, ref):
    """every output of a call: floating-point arrays on their bit patterns, integer arrays, None and the info dictionary by value"""
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        if r is None or isinstance(r, dict):
            ok = g == r
        elif r.dtype.kind in "fc":
            ok = same(g, r)
        else:
            ok = g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r)
        if not ok:
            return False
    return True


class Calls:
    """the calls of the sequence for one case, each a function of the handle"""

    def __init__(self, name):
        c = T.case(name)
        self.name = name
        n, B = c.st.n, c.B
        om5 = np.concatenate([[0.0], c.om[:: max(1, len(c.om) // 4)][:4]])
        om2 = om5[1:3]
        assert len(om5) == 5
        b3 = np.zeros((B, 3, n), complex)
        b3[:, 0] = c.bac
        b3[:, 1, c.st.n_nodes // 2] = 1.0
        b3[:, 2, c.st.n_nodes] = 1.0
        pairs, e, out = TA.all_pairs(n), N.e_out(name, c.st), N.output_index(name, c.st)
        db = np.random.default_rng(7).standard_normal((1, 2, n)) * (1 + 0.5j)
        if B == 3:
            sens = dict(base=[1], plus=[[2, 0]], minus=[[0, 2]], scale=[[0.7, 0.7]])
        else:
            sens = dict(base=[0], plus=[[0, 0]], minus=[[0, 0]], scale=[[0.7, 0.7]])

        def hbm(call):
            def run(h):
                h.ac_set_memory("hbm", 2)
                try:
                    return call(h)
                finally:
                    h.ac_set_memory("lds")
            return run

        self.om5, self.om2, self.bac, self.n = om5, om2, c.bac, n
        self.call = {
            "plain5": lambda h: h.ac_solve(om5, GMIN, c.bac),
            "arnoldi3": lambda h: h.ac_arnoldi(om5, GMIN, c.bac, 3, [(out, -1), (-1, out)], want_v=True),
            "multi": lambda h: h.ac_solve_multi(om5, GMIN, b3, pairs, 0, True),
            "adjoint1": lambda h: h.ac_adjoint(om5, GMIN, e, [(out, -1)], want_x=False),
            "plain2": lambda h: h.ac_solve(om2, GMIN, c.bac),
            "sens": lambda h: h.ac_sens(om5, GMIN, sens["base"], sens["plus"], sens["minus"], sens["scale"], c.bac[sens["base"]], e, (out, -1), db, 0, True),
            "adjoint_hbm": hbm(lambda h: h.ac_adjoint(om2, GMIN, e, pairs, want_x=True)),
            "adjoint_multi": lambda h: h.ac_adjoint_multi(om5, GMIN, b3, pairs, 0, True),
            "arnoldi6": lambda h: h.ac_arnoldi(om2[:1], GMIN, c.bac, 6, [(out, -1)], want_v=True),
        }
        self.ref = {}

    def reference(self, key):
        """the call as the first AC call of a fresh handle, once"""
        if key not in self.ref:
            sim = fresh(self.name)
            try:
                self.ref[key] = self.call[key](sim.h)
            finally:
                sim.close()
        return self.ref[key]


_CALLS = {}


def calls(name):
    if name not in _CALLS:
        _CALLS[name] = Calls(name)
    return _CALLS[name]


SEQUENCE = ["plain5", "arnoldi3", "multi", "adjoint1", "plain2", "sens", "adjoint_hbm", "adjoint_multi", "plain5"]


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_an_interleaved_sequence_on_one_handle_is_the_fresh_handles_to_the_bit(name):
    k = calls(name)
    sim = fresh(name)
    try:
        for step, key in enumerate(SEQUENCE):
            got = k.call[key](sim.h)
            assert equal(got, k.reference(key)), (step, key)
        assert sim.h.ac_plan_info()["memory"] == "lds"
        # the six families ran: plain, adjoint, multi, adjoint-multi, sensitivity, Arnoldi; the plain sweep saw its slots larger, smaller and
        # owned by every other family in between
        x5 = k.reference("plain5")[0]
        assert x5.shape[1] == 5 and k.reference("plain2")[0].shape[1] == 2 and k.reference("adjoint1")[1] is None
        assert k.reference("adjoint_hbm")[4]["lds_bytes"] == 0 and k.reference("arnoldi3")[4].shape[2:] == (4, k.n)
    finally:
        sim.close()


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_a_refused_call_leaves_the_next_call_unchanged(name):
    """refusals come before anything is touched: an invalid wpb, a family the overlay excludes, a grid that is not the overlay's"""
    k = calls(name)
    sim = fresh(name)
    try:
        h = sim.h
        assert equal(k.call["multi"](h), k.reference("multi"))
        with pytest.raises(hip.CadnipError) as e:
            h.ac_solve(k.om5, GMIN, k.bac, 3)
        assert e.value.code == hip.BADARG
        h.ac_set_overlay([0], k.om5, np.zeros((5, 1), complex))
        try:
            for call in (k.call["plain2"], k.call["arnoldi3"], k.call["sens"]):
                with pytest.raises(hip.CadnipError) as e:
                    call(h)
                assert e.value.code == hip.BADARG
        finally:
            h.ac_clear_overlay()
        assert equal(k.call["plain5"](h), k.reference("plain5"))
        assert equal(k.call["multi"](h), k.reference("multi"))
    finally:
        sim.close()


def test_a_breakdown_after_a_larger_call_shows_no_stale_columns():
    """butterworth at m = n = 6: the Krylov space closes at step 4 (tests/test_gpu_ac_arnoldi.py), so H, l and V have words no step writes --
    after a larger Arnoldi call without a breakdown (5 shifts, m = 3) and a multi sweep on the same handle, they are the fresh handle's zeros"""
    k = calls("butterworth")
    sim = fresh("butterworth")
    try:
        for key in ("arnoldi3", "multi", "arnoldi6"):
            assert equal(k.call[key](sim.h), k.reference(key)), key
        H, beta, meff, l, V, berr, flags, info = k.reference("arnoldi6")
        H3, _, meff3 = k.reference("arnoldi3")[:3]
        assert np.all(meff3[:, 1:] == 3) and H3.size > H.size                      # the larger call ran its three steps
        me = int(meff[0, 0])
        assert 1 <= me < 6 and flags[0, 0] == 4
        assert not H[0, 0, :, me:].any() and not l[0, 0, me:].any() and not V[0, 0, me:].any() and V[0, 0, :me].any()
    finally:
        sim.close()
