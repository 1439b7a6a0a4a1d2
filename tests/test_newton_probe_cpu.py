"""The single-Newton-update probes (tests/newton_probe_ref.py) without a GPU: the reference meets its own bound, its states pin at least
80 % of every circuit's Jacobian entries, the CPU port performs the two probes as exactly one update -- one Newton solve in the DC call; one
accepted step and one iteration in the transient call -- and passes the bound the GPU paths are held to, and the bound rejects a Jacobian
entry that is off by 1e-3 and two swapped partials of an sp_mos1.

Conditioning (kappa_inf of J at corner 0, printed by the first test).  Transient probes: at most 1.3e6 on the flip-flop and 3e4 on the
other circuits but linear_zoo, whose J reaches 2e13 at h = 2^-42 (L / h = 4.4e9 beside unit incidence entries).  DC probes (J = G in dcop
and tranop): the flip-flop reaches 1.5e12 at these states (gmin-only paths to its storage nodes), above 1e10; every other circuit stays
below 5e5.  The check is a backward error and holds there all the same.

What the read-out costs.  A probe returns u1 = fl(u0 - delta), so delta = u0 - u1 is known to u |u1| only (u = 2^-53).  Where an update is
small beside its unknown -- an inductor current of 0.5 mA that one C-dominated step moves by 1e-10 A -- the exact delta_ref, rounded into
u1 and read back, misses the bound without the read-out's term (newton_probe_ref: the last term of the bound) by four orders of magnitude
on linear_zoo; with it the rounded delta_ref stays below 1 everywhere (worst: 0.85, linear_zoo, h = 2^-42, the inductor's row).  The first
test prints both figures."""
import numpy as np
import pytest

from tests import newton_probe_ref as NP
from tests import stamp_ref as SR
from tests.port_util import make_port, analyze_port

LD = np.longdouble


_ports = {}


def _port(name, i, mode):
    if (name, i, mode) not in _ports:
        pt = NP.points(name)[i]
        st, port = make_port(NP.make(name), NP.params_of(pt), pt["temp"], mode)
        analyze_port(st, port, NP.vscale(name))
        _ports[(name, i, mode)] = (st, port)
    return _ports[(name, i, mode)]


@pytest.fixture(scope="module", autouse=True)
def _close_ports():
    yield
    for _, port in _ports.values():
        port.close()
    _ports.clear()


def port_probe(name, i, probe, pcnr=False, newton_mode=0):
    """u1 of one probe on the CPU port, with the assertion that it was exactly one Newton update."""
    kind, mode, s, h = probe
    ref = NP.reference(name, i, probe)
    st, port = _port(name, i, mode)
    if kind == "dc":
        u1, ok, iters = port.dc(ref.u0, abstol=1e-300, maxiters=1, use_pcnr=pcnr, cold_start=False)
        assert not ok and iters == 1, (name, i, probe, ok, iters)
        return u1
    out, u1, stats, _ = port.tran(ref.u0, NP.T0, NP.T0 + h, 1e30, 1.0, breaks=(), save_t=[NP.T0 + h], h0=h, hmax=h, max_newton=3, newton_tol=1.0,
                                  err_mask=np.zeros(st.n), use_pcnr=False, newton_mode=newton_mode, max_order=2)
    got = (stats["status"], stats["accepted"], stats["newton_iters"], stats["rejected"], stats["newton_failures"])
    assert got == (1, 1, 1, 0, 0), (name, i, probe, stats)
    assert np.array_equal(out[0], u1)
    return u1


@pytest.mark.parametrize("name", NP.CIRCUITS)
def test_reference_meets_its_own_bound(name):
    """(a) delta_ref itself, and delta_ref as a probe would return it (rounded into u1 = fl(u0 - delta_ref))."""
    from tests.lu_ref import cond_inf
    worst, worst_rt, bare, kmax = 0.0, 0.0, 0.0, {"dc": 0.0, "tran": 0.0}
    for i in range(NP.N_CORNERS):
        for probe in NP.PROBES:
            r = NP.reference(name, i, probe)
            assert np.all(np.isfinite(np.asarray(r.delta, dtype=np.float64)))
            worst = max(worst, float(np.max(r.ratios(r.delta))))
            u1 = r.u0 - np.asarray(r.delta, dtype=np.float64)
            worst_rt = max(worst_rt, r.check(u1)[0])
            bare = max(bare, float(np.max(r.ratios(r.u0.astype(LD) - u1.astype(LD), readout=False))))
            if i == 0:
                kmax[probe[0]] = max(kmax[probe[0]], cond_inf(r.J))
    print("%-18s delta_ref ratio %.3g, through u1 %.3g (without the read-out's term: %.3g); kappa_inf(J) at corner 0: DC %.2g, transient %.2g"
          % (name, worst, worst_rt, bare, kmax["dc"], kmax["tran"]))
    assert worst < 1e-3 and worst_rt < 1.0


@pytest.mark.parametrize("name", NP.CIRCUITS)
def test_states_pin_the_jacobian(name):
    """(b) the coverage cap: at least 80 % of the structurally non-zero entries are pinned by some probe."""
    pinned, pat, _ = NP.coverage(name)
    n_pin, n_all = int(pinned.sum()), int(pat.sum())
    print("%-18s pinned %d of %d entries (%.1f %%)" % (name, n_pin, n_all, 100.0 * n_pin / n_all))
    for ln in NP.unpinned_report(name):
        print("   unpinned:", ln)
    assert n_all == NP.structure(name).nnz
    assert n_pin >= NP.PIN_CAP * n_all


@pytest.mark.parametrize("name", NP.CIRCUITS)
def test_port_performs_one_update_within_the_bound(name):
    """(c) both probes on the CPU port -- DC with and without PCNR, transient in the port's three Newton modes (2 is the per-op kernels'
    reading of mode 1) -- are one update each and pass the bound."""
    worst = {}
    for i in range(NP.N_CORNERS):
        for probe in NP.PROBES:
            ref = NP.reference(name, i, probe)
            for opt in ((False, True) if probe[0] == "dc" else (0, 1, 2)):
                pc = probe[0] == "dc" and opt
                u1 = port_probe(name, i, probe, pcnr=pc, newton_mode=0 if probe[0] == "dc" else opt)
                r, row, fwd, lim = ref.check(u1, pcnr=pc)
                key = "DC, PCNR %d" % opt if probe[0] == "dc" else "transient, Newton mode %d" % opt
                if r >= worst.get(key, (-1.0,))[0]:
                    worst[key] = (r, fwd, lim, i, probe, NP.unknown_name(ref.st, row))
                assert r <= 1.0, (name, i, probe, opt, r, NP.unknown_name(ref.st, row))
                assert lim <= 1.0, (name, i, probe, opt, lim)
    for key, (r, fwd, lim, i, probe, row) in sorted(worst.items()):
        print("%-18s port %-24s worst backward ratio %.3g (corner %d, state %d, h %s, row %s), forward %.3g, limit slots %.3g"
              % (name, key, r, i, probe[2], probe[3], row, fwd, lim))


def _faulty_update(ref, J):
    """u1 = fl(u0 - delta) with delta solved from the matrix J in place of J_ref: by the reference's own solver, so that what fails the
    check is the fault and not a solver's noise (a plain float64 solve leaves 1e-22 A in the flip-flop's ammeter row, whose bound is 0).  A
    matrix that the fault made singular returns a non-finite state, which fails."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            d = np.asarray(NP.solve(J, ref.F), dtype=np.float64)
        except (np.linalg.LinAlgError, ValueError):
            d = np.full(ref.st.n, np.nan)
    return ref.u0 - d


@pytest.mark.parametrize("name", NP.CIRCUITS)
def test_a_wrong_entry_fails_the_check(name):
    """(d) a seeded sample of 100 pinned entries (all of them where a circuit has fewer): one entry of J scaled by 1 + 1e-3, the update solved
    with that matrix, fails the check in the probe that pins the entry -- and the same solve with the right matrix passes."""
    pinned, _, witness = NP.coverage(name)
    idx = np.argwhere(pinned)
    rng = np.random.default_rng(20240607)
    pick = idx[rng.permutation(len(idx))[:100]]
    low = np.inf
    for i, j in pick:
        ref = NP.witness_ref(name, witness[i, j])
        assert ref.check(_faulty_update(ref, ref.J))[0] <= 1.0
        Jf = ref.J.copy()
        Jf[i, j] *= LD(1.0 + 1e-3)
        r = ref.check(_faulty_update(ref, Jf))[0]
        low = min(low, r)
        assert r > 1.0, (name, NP.unknown_name(ref.st, i), NP.unknown_name(ref.st, j), r)
    print("%-18s %d faulty entries, smallest ratio of a faulty update %.3g" % (name, len(pick), low))


def _mos1_pairs(st, ref):
    """Per sp_mos1 device: [(row, col_a, col_b, J_a, J_b)] of its own contributions to two entries of one row (J = G + a0 C parts)."""
    dev_g, dev_c = SR.slot_devices(st, "g")[st.g_slots], SR.slot_devices(st, "c")[st.c_slots]
    ty = SR.slot_types(st, "g")[st.g_slots]
    ent_g, ent_c = np.repeat(np.arange(st.nnz), np.diff(st.g_ptr)), np.repeat(np.arange(st.nnz), np.diff(st.c_ptr))
    rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
    cols = np.asarray(st.colidx)
    out = {}
    for d in np.unique(dev_g[ty == "MOS1"]):
        part = np.zeros(st.nnz, dtype=LD)
        np.add.at(part, ent_g[dev_g == d], ref.stamp.vg[dev_g == d].astype(LD))
        np.add.at(part, ent_c[dev_c == d], LD(ref.a0) * ref.stamp.vc[dev_c == d].astype(LD))
        touched = np.zeros(st.nnz, dtype=bool)
        touched[ent_g[dev_g == d]] = True
        touched[ent_c[dev_c == d]] = True
        prs = []
        for r in np.unique(rows[touched]):
            e = np.nonzero(touched & (rows == r))[0]
            prs += [(int(r), int(cols[a]), int(cols[b]), part[a], part[b]) for k, a in enumerate(e) for b in e[k + 1:]]
        out[int(d)] = prs
    return out


@pytest.mark.parametrize("name", ["inverter", "dff", "meyer_inverter_rd"])
def test_swapped_mos1_partials_fail_the_check(name):
    """(d) two partials of one sp_mos1 swapped in J (the device's own contributions to two entries of one row change places).  A swap is
    visible to a probe if PIN_LEVEL |(J_a - J_b)(delta_a - delta_b)| exceeds the row's bound at delta_ref -- the pinning condition applied
    to what the swap changes in the row's product; every device must have a visible swap, and every visible one (a seeded sample of at most
    100) must fail the check."""
    st = NP.structure(name)
    vis = []
    seen = set()
    for i in (0, 1, 2):
        for k, probe in enumerate(NP.PROBES):
            ref = NP.reference(name, i, probe)
            bd = ref.bound(ref.delta)
            for d, prs in _mos1_pairs(st, ref).items():
                for r, ca, cb, ja, jb in prs:
                    if r >= ref.lim0 or ja == jb:
                        continue
                    if LD(NP.PIN_LEVEL) * abs((ja - jb) * (ref.delta[ca] - ref.delta[cb])) > bd[r]:
                        vis.append((i, k, d, r, ca, cb, ja, jb))
                        seen.add(d)
    devs = set(_mos1_pairs(st, NP.reference(name, 0, NP.PROBES[0])))
    assert seen == devs, (name, sorted(devs - seen))
    rng = np.random.default_rng(7)
    low = np.inf
    for q in rng.permutation(len(vis))[:100]:
        i, k, d, r, ca, cb, ja, jb = vis[q]
        ref = NP.reference(name, i, NP.PROBES[k])
        Jf = ref.J.copy()
        Jf[r, ca] += jb - ja
        Jf[r, cb] += ja - jb
        ratio = ref.check(_faulty_update(ref, Jf))[0]
        low = min(low, ratio)
        assert ratio > 1.0, (name, d, NP.unknown_name(st, r), NP.unknown_name(st, ca), NP.unknown_name(st, cb), ratio)
    print("%-18s %d sp_mos1 devices, %d visible swaps, smallest ratio of a swapped update %.3g" % (name, len(devs), len(vis), low))
