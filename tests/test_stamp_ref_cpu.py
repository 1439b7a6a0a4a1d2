"""The per-contribution stamping reference (tests/stamp_ref.py) on the CPU: it reproduces the oracle's fast_rebuild bit for bit, its
entry lists line up with the Structure's gather lists slot for slot, and its per-entry bound catches faults that the array-wide
tolerance of tests/test_gpu_parity.py lets through."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from tests import stamp_ref as R
from tests.circuits import ALL_STAMP, CHAIN_STAMP, TILED_STAMP

CASES = dict(ALL_STAMP, **TILED_STAMP, **CHAIN_STAMP)


def _state(st, seed, name):
    rng = np.random.default_rng(seed)
    return rng.random(st.n) * (5.0 if name.startswith(("dff", "chain", "inverter")) else 2.0) - 0.5


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_contributions_reproduce_the_oracle(name):
    mk, params = CASES[name]
    circ = mk()
    o = R.OracleStamper(circ, params)
    st = o.st
    for seed, t, gsh, sf in ((1, 0.0, 0.0, 1.0), (2, 3e-7, 1e-3, 0.3)):
        ref = o.rebuild(_state(st, seed, name), t, gshunt=gsh, srcFact=sf)
        # the k-th oracle contribution of an entry is the k-th slot of the Structure's gather list
        assert np.array_equal(ref.pg, st.g_ptr) and np.array_equal(ref.pc, st.c_ptr) and np.array_equal(ref.pb, st.b_ptr), name
        assert len(ref.vg) == len(st.g_slots) and len(ref.vc) == len(st.c_slots) and len(ref.vb) == len(st.b_slots)
        # summed in COO order (+ gshunt, * srcFact) they are the oracle's arrays, bit for bit
        assert np.array_equal(R.coo_sums(ref.vg, ref.pg, extra=ref.gdiag), ref.G), name
        assert np.array_equal(R.coo_sums(ref.vc, ref.pc), ref.C), name
        assert np.array_equal(R.coo_sums(ref.vb, ref.pb, scale=sf), ref.b), name
        # and the oracle's own arrays pass the per-entry check against the exact sums
        for c in R.check_stamp(ref.G, ref.C, ref.b, ref):
            assert c.ok, (name, c)


def test_exact_sums_and_bounds():
    """check_sums against math.fsum on a cancelling sum, the empty-entry rule and the gamma bound's edge."""
    vals = np.array([1e16, 1.0, -1e16, 3.0, 0.5, -0.25])
    ptr = np.array([0, 3, 3, 6])
    ex = R.fsum_entries(vals, ptr)
    assert list(ex) == [1.0, 0.0, 3.25]
    assert R.check_sums(np.array([1.0, 0.0, 3.25]), vals, ptr).ok
    assert not R.check_sums(np.array([1.0, 1e-300, 3.25]), vals, ptr).ok       # an entry with no contribution is exactly 0
    S = 2e16 + 1.0
    tol = float(R.gamma(4)) * S
    assert R.check_sums(np.array([1.0 + 0.9 * tol, 0.0, 3.25]), vals, ptr).ok
    assert not R.check_sums(np.array([1.0 + 1.2 * tol, 0.0, 3.25]), vals, ptr).ok
    # gshunt on a diagonal: an entry with no stamp carries gshunt alone
    assert R.check_sums(np.array([1.0, 1e-3, 3.25]), vals, ptr, extra=np.array([0.0, 1e-3, 0.0])).ok
    assert not R.check_sums(np.array([1.0, 0.0, 3.25]), vals, ptr, extra=np.array([0.0, 1e-3, 0.0])).ok
    assert R.jacobian_ok(np.array([[1.0 + 2.0 ** -52]]), np.array([[1.0]]), np.array([[2.0 ** -52]]), [1.0])


def _dff_trial1():
    """The flip-flop at the state of trial 1 of test_gpu_parity.test_rebuild_matches_oracle (seed 42, u in [-0.5, 1.5], tran, t = 0)."""
    mk, params = ALL_STAMP["dff"]
    o = R.OracleStamper(mk(), params)
    rng = np.random.default_rng(42)
    rng.random(o.st.n)
    rng.random(o.st.n)
    u = rng.random(o.st.n) * 2 - 0.5
    return o, o.rebuild(u, 0.0), u


def _parity_close(a, b):
    from tests.test_gpu_parity import _close
    return _close(a, b)


@pytest.mark.parametrize("fault", ["drop_gmin", "scale_small_g", "drop_mos1_b"])
def test_per_entry_check_catches_what_the_array_tolerance_misses(fault):
    o, ref, u = _dff_trial1()
    st = o.st
    G, b = ref.G.copy(), ref.b.copy()
    gmin = o.cs.spec.gmin
    tg, tb = R.slot_types(st, "g"), R.slot_types(st, "b")
    if fault == "drop_gmin":
        # a junction's conductance carries gmin (va_mos1_ref.py: MOS1gbd / MOS1gbs); drop it on the smallest G entry fed by sp_mos1
        mos = np.zeros(st.nnz, dtype=bool)
        mos[np.repeat(np.arange(st.nnz), np.diff(st.g_ptr))[tg[st.g_slots] == "MOS1"]] = True
        e = np.nonzero(mos & (G != 0))[0]
        e = e[np.argmin(np.abs(G[e]))]
        G[e] -= gmin
    elif fault == "scale_small_g":
        # (a contribution below 1e-4 max|G|: the largest under 1e-6 max|G|, so that 1e-6 of it is still under _close's 1e-12 max|G|)
        small = np.nonzero((np.abs(ref.vg) > 0) & (np.abs(ref.vg) < 1e-6 * np.max(np.abs(G))))[0]
        p = small[np.argmax(np.abs(ref.vg[small]))]
        vg = ref.vg.copy()
        vg[p] *= 1 + 1e-6
        G = R.coo_sums(vg, ref.pg, extra=ref.gdiag)
    else:
        # (the largest sp_mos1 b contribution under 1e-12 max|b|: _close's absolute tolerance on b)
        p = np.nonzero((tb[st.b_slots] == "MOS1") & (ref.vb != 0) & (np.abs(ref.vb) < 1e-12 * np.max(np.abs(b))))[0]
        p = p[np.argmax(np.abs(ref.vb[p]))]
        vb = ref.vb.copy()
        vb[p] = 0.0
        b = R.coo_sums(vb, ref.pb)
    assert not np.array_equal(G, ref.G) or not np.array_equal(b, ref.b)
    # the array-wide tolerance of test_gpu_parity accepts the fault ...
    assert _parity_close(G, ref.G) and _parity_close(b, ref.b)
    # ... the per-entry check does: the summation bound alone, and the tolerance the GPU tests use (test_gpu_parity._per_entry,
    # tests/test_gpu_stamp_kernels.py: rho per slot on its own scale)
    for kw in ({}, dict(rho=R.RHO, st=st, u=u)):
        cg, cc, cb = R.check_stamp(G, ref.C, b, ref, **kw)
        assert cc.ok and not (cg.ok and cb.ok), (fault, kw.keys(), cg, cb)
    assert all(c.ok for c in R.check_stamp(ref.G, ref.C, ref.b, ref, rho=R.RHO, st=st, u=u))


def test_slot_tolerance_is_relative():
    """The slot check of tests/test_gpu_stamp_kernels.py at the deployed tolerance: on the flip-flop at trial 1 every contribution that
    is at least 1e-3 of its scale (a device's larger conductances, capacitances and currents) is rejected when changed by 1e-6 of
    itself, and doubling any contribution above 1e-15 of its scale is rejected."""
    o, ref, u = _dff_trial1()
    st = o.st
    sc = R.slot_scales(st, ref, u)
    for which, vals, slots in (("g", ref.vg, st.g_slots), ("c", ref.vc, st.c_slots), ("b", ref.vb, st.b_slots)):
        rho = R.rho_of(st, which, slots, R.RHO)
        q = R.slot_ratio(vals * (1 + 1e-6), vals, sc[which]) / rho
        live = (vals != 0) & (np.abs(vals) >= 1e-3 * sc[which])
        assert live.sum() > 0 and np.all(q[live] > 1), (which, int(np.sum(q[live] <= 1)))
        big = np.abs(vals) > 1e-15 * sc[which]
        assert np.all(R.slot_ratio(2 * vals, vals, sc[which])[big] > rho[big]), which
        assert np.all(R.slot_ratio(vals, vals, sc[which]) == 0)


def test_dff_trial1_entries_are_mostly_below_the_array_tolerance():
    """The gap the per-entry check closes: at trial 1 the largest |G| of the flip-flop is 1 (the supplies' incidence entries) and the
    largest |b| is 5 V, so _close is an absolute tolerance of 1e-12 on G and 5e-12 on b -- above 1e8 ulp for the junction and
    channel conductances below 1e-4 and for 102 of the 107 non-zero b rows."""
    o, ref, u = _dff_trial1()
    G, b = ref.G, ref.b
    nzG, nzb = G[G != 0], b[b != 0]
    assert np.max(np.abs(G)) == 1.0 and np.max(np.abs(b)) == 5.0
    assert np.sum(np.abs(nzG) < 1e-4) >= 50 and np.sum(np.abs(nzb) < 5e-4) >= 100
