"""The per-op stamping kernels (csrc/stamp_csr.hip: k_stamp_prep, k_stamp_csr<TYPE>), the residual kernels and the Jacobian kernels
entry by entry against the per-contribution reference of tests/stamp_ref.py, on circuits that reach every launch path (DESIGN.md
section 5, "Stamping coverage").

(a) reduction: G, C, b of a rebuild against the exact sums of the same rebuild's own per-device contributions (get_contributions),
    gamma_{k+1} bound per entry -- independent of the device math;
(b) device evaluation: every contribution slot against the oracle's, |s - r| <= RHO * scale + FLOOR (stamp_ref.slot_scales);
(c) end to end: G, C, b against the oracle's exact sums, gamma_{k+1} S_ref plus the slots' allowances;
(d) consumers: residual row by row (k_residual_lds, k_residual, k_residual_long), J = G + gamma C bit for bit, dense J, ODE forms;
(e) modes and state sequences; (f) single-writer words bit for bit across rebuilds and batch sizes.
Every case asserts the launch geometry it claims from the CADNIP_SC_DEBUG line of each stamping launch."""
import re

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import hip
from tests import stamp_ref as R
from tests.circuits import ALL_STAMP, CHAIN_STAMP, TILED_STAMP, tiled

pytestmark = pytest.mark.gpu

CASES = dict(ALL_STAMP, **TILED_STAMP, **CHAIN_STAMP)
MULTI = dict(TILED_STAMP, **CHAIN_STAMP)
RHO = R.RHO
DBG = re.compile(r"\[cadnip stamp\] type (\d+) count (\d+) cs (\d+) chunks (\d+) ipw (\d+) lpd (\d+) slots (\d+) rows (\d+) scratch (\d+) "
                 r"tile_words (\d+) shmem (\d+) grid (\d+) levels (\d+) u_lds (\d+)( \(read-out pass\))?")
KEYS = ("type", "count", "cs", "chunks", "ipw", "lpd", "slots", "rows", "scratch", "tile_words", "shmem", "grid", "levels", "u_lds")


def _launches(capfd):
    out = []
    for line in capfd.readouterr().err.splitlines():
        m = DBG.search(line)
        if m:
            d = dict(zip(KEYS, map(int, m.groups()[:-1])))
            d["readout"] = m.group(15) is not None
            out.append(d)
    return out


def _blocks(st):
    return [b for b in st.blocks if b.count]


def _reduce_launches(st, launches, B):
    """The reducing launches of one rebuild, matched to the structure's blocks; each one's geometry re-derived from the plan's rules."""
    red = [d for d in launches if not d["readout"]][-len(_blocks(st)):]
    assert len(red) == len(_blocks(st)), (len(red), len(_blocks(st)))
    for blk, d in zip(_blocks(st), red):
        assert d["count"] == blk.count and d["type"] == hip.type_id(blk.type)
        assert d["chunks"] == -(-blk.count // d["cs"]) and (d["chunks"] == 1) == (blk.count == d["cs"])
        assert d["u_lds"] == (d["ipw"] * st.n * 8 <= 16 * 1024)
        ipw0 = min(8, max(1, 64 // (blk.count * d["lpd"]))) if d["chunks"] == 1 else 1
        assert d["ipw"] <= ipw0 and (d["ipw"] == ipw0 or (d["ipw"] + 1) * d["tile_words"] * 8 > 64 * 1024), d
        assert d["grid"] == d["chunks"] * -(-B // d["ipw"])
        d["block"] = blk
    return red


def _atomic_targets(st, blk, cs):
    """Targets of G, C and b that receive contributions from more than one chunk (dev // cs) of this block: fp64 atomics."""
    n = 0
    for which, ptr, slots, base, nk in (("g", st.g_ptr, st.g_slots, blk.g_base, blk.n_g), ("c", st.c_ptr, st.c_slots, blk.c_base, blk.n_c),
                                        ("b", st.b_ptr, st.b_slots, blk.b_base, blk.n_b)):
        ent = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        s = np.asarray(slots)
        own = (s >= base) & (s < base + nk * blk.count)
        chunk = ((s[own] - base) % blk.count) // cs
        e = ent[own]
        if e.size:
            lo = np.full(len(ptr) - 1, 1 << 30)
            hi = np.full(len(ptr) - 1, -1)
            np.minimum.at(lo, e, chunk)
            np.maximum.at(hi, e, chunk)
            n += int(np.sum(hi > lo))
    return n


# types whose every target is private to one device (each entry involves the device's own branch current): no target is shared
PRIVATE = {"V", "E", "H", "L", "F", "BV"}


def _sim(name, B, mode="tran"):
    mk, params = CASES[name]
    circ = mk()
    st = cj.discover(circ, params)
    h = hip.Handle(st, B)
    # (up to 60 C: at 100 C the oracle's charge detection finds va_mos_inverter_x65's junction charges bias-independent -- another structure)
    temps = np.linspace(-40.0, 60.0, B) if B > 1 else np.array([27.0])
    pp = {k: float(v) * (1.0 + 0.1 * np.linspace(-1, 1, B)) for k, v in params.items()}
    h.set_params(cj.pack_params(st, circ, pp, temps, B))
    h.set_spec(mode=mode)
    return circ, params, st, h, temps, pp


def _states(st, name, B, seed):
    rng = np.random.default_rng(seed)
    vs = 5.0 if name.startswith(("dff", "chain", "inverter")) else 1.0
    u = (rng.random((B, st.n)) * 2 - 0.5) * vs
    if name.startswith("chain"):          # logic levels along the chain (vin = 5 V: n0 high, n1 low, ...), +-0.1 V
        lv = np.array([5.0 if nm == "vdd" else 5.0 * (1 - int(nm[1:]) % 2) for nm in st.node_names])
        u[:, :st.n_nodes] = lv[None, :] + 0.2 * (rng.random((B, st.n_nodes)) - 0.5)
    return u, rng.random(B) * 1e-6


def _csr(st, A):
    return np.asarray(A)[..., st.to_ref_nz]


def _check_reduction(st, h, u, t, gshunt=0.0, srcFact=1.0):
    """get_contributions (read-out pass + reduction) then get_GCb: every entry within gamma_{k+1} of the exact sum of its own slots;
    a second plain rebuild writes the same single-writer words bit for bit."""
    Sg, Sc, Sb = h.get_contributions()
    G, Cm, b, lw = h.get_GCb()
    gd = R.gshunt_terms(st, gshunt)
    checks = (R.check_sums(_csr(st, G), Sg[:, st.g_slots], st.g_ptr, extra=gd, what="G"),
              R.check_sums(_csr(st, Cm), Sc[:, st.c_slots], st.c_ptr, what="C"),
              R.check_sums(b, Sb[:, st.b_slots], st.b_ptr, scale=srcFact, what="b"))
    for c in checks:
        assert c.ok, c
    h.rebuild(u, t)
    G2, C2, b2, lw2 = h.get_GCb()
    assert np.array_equal(lw2, lw)
    return (G, Cm, b), (G2, C2, b2), (Sg, Sc, Sb), checks


def _single_writer(st, blocks_cs):
    """Masks (G, C in reference order; b) of the words that one tile writes: no atomics there."""
    multi = {0: np.zeros(st.nnz, bool), 1: np.zeros(st.nnz, bool), 2: np.zeros(st.n, bool)}
    for arr, (ptr, slots) in enumerate(((st.g_ptr, st.g_slots), (st.c_ptr, st.c_slots), (st.b_ptr, st.b_slots))):
        ent = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        s = np.asarray(slots)
        for blk, cs in blocks_cs:
            base, nk = (blk.g_base, blk.n_g) if arr == 0 else (blk.c_base, blk.n_c) if arr == 1 else (blk.b_base, blk.n_b)
            own = (s >= base) & (s < base + nk * blk.count)
            if not own.any():
                continue
            chunk = ((s[own] - base) % blk.count) // cs
            lo = np.full(len(ptr) - 1, 1 << 30); hi = np.full(len(ptr) - 1, -1)
            np.minimum.at(lo, ent[own], chunk); np.maximum.at(hi, ent[own], chunk)
            multi[arr] |= hi > lo
    inv = np.argsort(st.to_ref_nz)            # reference order position -> CSR entry
    return ~multi[0][inv], ~multi[1][inv], ~multi[2]


def _bs(name):
    return (1, 7, 65) if name == "chain520" else (1, 7, 65, 300)     # (chain520 at B = 300: 36 M contribution words)


@pytest.mark.parametrize("name,B", [(n, B) for n in CASES for B in _bs(n)])
def test_reduction_matches_the_exact_sum_of_its_own_contributions(name, B, monkeypatch, capfd):
    monkeypatch.setenv("CADNIP_SC_DEBUG", "1")
    circ, params, st, h, temps, pp = _sim(name, B)
    u, t = _states(st, name, B, seed=B)
    capfd.readouterr()
    h.rebuild(u, t)
    red = _reduce_launches(st, _launches(capfd), B)
    # the geometry this case is here for
    by = {d["block"].type: d for d in red}
    if name in MULTI:
        for d in red:
            if d["chunks"] > 1 and d["block"].type not in PRIVATE:
                assert _atomic_targets(st, d["block"], d["cs"]) >= 1, (name, d["block"].type)
        if name in TILED_STAMP:
            assert all(d["chunks"] >= 2 for d in red if d["block"].type != "C" or name != "va_zoo_x33"), [(d["block"].type, d["chunks"]) for d in red]
    if name == "chain16":
        assert by["MOS1"]["chunks"] == 1 and by["MOS1"]["cs"] == 32
    if name == "chain17":
        assert by["MOS1"]["chunks"] == 2
    if name == "chain40" and B >= 8:
        assert by["V"]["ipw"] == 8 and by["V"]["u_lds"] == 0
    if name == "chain200":
        assert by["MOS1"]["chunks"] == 13 and by["MOS1"]["u_lds"] == 0
    if name in ("chain200", "chain520"):
        assert by["MOS1"]["levels"] >= 3
    (G, Cm, b), (G2, C2, b2), _, _ = _check_reduction(st, h, u, t)
    sw = _single_writer(st, [(d["block"], d["cs"]) for d in red])
    assert np.array_equal(G2[:, sw[0]], G[:, sw[0]]) and np.array_equal(C2[:, sw[1]], Cm[:, sw[1]]) and np.array_equal(b2[:, sw[2]], b[:, sw[2]])
    h.close()
    # (f) single-writer words do not depend on the batch: instance B - 1 restamped alone
    if B > 1:
        i = B - 1
        st1 = cj.discover(circ, params)
        h1 = hip.Handle(st1, 1)
        h1.set_params(cj.pack_params(st1, circ, {k: v[i:i + 1] for k, v in pp.items()}, temps[i:i + 1], 1))
        h1.set_spec(mode="tran")
        h1.rebuild(u[i:i + 1], t[i:i + 1])
        G1, C1, b1, _ = h1.get_GCb()
        h1.close()
        assert np.array_equal(G1[0, sw[0]], G2[i, sw[0]]) and np.array_equal(C1[0, sw[1]], C2[i, sw[1]]) and np.array_equal(b1[0, sw[2]], b2[i, sw[2]])


@pytest.mark.parametrize("name", list(CASES))
def _physical_states(st, h, name, B):
    """States the solver meets: the DC operating point of the circuit (dc_run, tranop) with +-0.1 V on the node voltages, a state along a
    transient from it, and (the flip-flop) the extreme random state of test_gpu_parity.  The 200- and 520-stage chains, whose DC does
    not converge from zero, keep their logic levels +-0.1 V (_states); other circuits keep random states."""
    u, t = _states(st, name, B, seed=11)
    if not name.startswith(("dff", "chain")):
        return u, t
    from cadnip_jl_amd.structure import expand_breakpoints
    h.set_spec(mode="tranop")
    h.rebuild(np.zeros((B, st.n)), 0.0)
    h.jacobian(np.full(B, 1e9))
    h.analyze()
    udc, conv, _ = h.dc_run(abstol=1e-9)
    if name in ("chain200", "chain520"):
        h.set_spec(mode="tran")
        return u, t
    assert conv[0], name
    h.set_spec(mode="tran")
    t1 = 2.05e-7 if name.startswith("dff") else 1e-9
    out, _, stats = h.tran_run(0.0, t1, st.state_abstol(vntol=1e-6, iabstol=1e-9, chgtol=1e-6), 1e-4,
                               breaks=expand_breakpoints(st.breakpoints, (0.0, t1)), save_t=[t1], fused=0)
    rng = np.random.default_rng(12)
    u = udc.copy()
    u[0, :st.n_nodes] += 0.2 * (rng.random(st.n_nodes) - 0.5)
    t = np.zeros(B)
    u[1], t[1] = out[0, 0, :], t1
    if name.startswith("dff"):
        u[2] = np.random.default_rng(3).random(st.n) * 5.0          # the extreme state of test_gpu_parity
    return u, t


@pytest.mark.parametrize("name", list(CASES))
def test_device_evaluation_and_end_to_end_against_the_oracle(name, monkeypatch, capfd):
    """(b) slot by slot, (c) entry by entry end to end, on three instances with their own temperatures, parameters and states: each
    contribution within RHO of its own scale (stamp_ref.slot_scales: |r| plus the device's largest non-unit contribution for G and C;
    |r| plus the device's largest b and its companion products in the row for b)."""
    B = 3
    circ, params, st, h, temps, pp = _sim(name, B)
    u, t = _physical_states(st, h, name, B)
    h.set_spec(mode="tran")
    h.rebuild(u, t)
    Sg, Sc, Sb = h.get_contributions()
    G, Cm, b, lw = h.get_GCb()
    h.close()
    worst, bad_all = {}, []
    for i in range(B):
        o = R.OracleStamper(circ, {k: float(v[i]) for k, v in pp.items()}, temp=float(temps[i]), st=st)
        ref = o.rebuild(u[i], float(t[i]))
        sc = R.slot_scales(st, ref, u[i])
        for which, S, slots, vals in (("g", Sg, st.g_slots, ref.vg), ("c", Sc, st.c_slots, ref.vc), ("b", Sb, st.b_slots, ref.vb)):
            # |s - r| <= RHO * scale + FLOOR, reported as the ratio of the two sides
            err = np.abs(S[i, slots] - vals)
            allow = R.rho_of(st, which, slots, RHO) * sc[which] + R.floor_of(st, which, slots)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err == 0, 0.0, np.inf))
            ty = R.slot_types(st, which)[slots]
            for tname in set(ty):
                m = ty == tname
                key = "%s/%s" % (tname, which)
                worst[key] = max(worst.get(key, 0.0), float(np.max(q[m])))
                worst[key + " abs"] = max(worst.get(key + " abs", 0.0), float(np.max(err[m])))
            bad = np.nonzero(q > 1)[0]
            bad_all += [(i, which, ty[p], float(q[p]), float(S[i, slots[p]]), float(vals[p])) for p in bad[:3]]
        for c in R.check_stamp(_csr(st, G)[i], _csr(st, Cm)[i], b[i], ref, rho=RHO, st=st, u=u[i]):
            if not c.ok:
                bad_all.append((i, c))
    print("worst slot error / allowance", name, {k: float("%.3g" % v) for k, v in sorted(worst.items())})
    assert not bad_all, (name, bad_all[:8])


@pytest.mark.parametrize("name", ["dff", "linear_zoo_x65", "chain40", "chain520", "va_mos_inverter_x65"])
@pytest.mark.parametrize("rows_kernel", [False, True])
def test_consumers_entry_by_entry(name, rows_kernel, monkeypatch):
    """(d) residual row by row against long double (k_residual_lds; with CADNIP_RESIDUAL_ROWS k_residual; k_residual_long on rows above
    512 entries), J = G + gamma C bit for bit (fused or unfused), the dense J, and the ODE forms' rhs and Jacobian."""
    if rows_kernel:
        monkeypatch.setenv("CADNIP_RESIDUAL_ROWS", "1")
    B = 3
    circ, params, st, h, temps, pp = _sim(name, B)
    long_rows = int(np.max(np.diff(st.rowptr))) > 512
    lds_path = not rows_kernel and not long_rows and (2 * st.nnz + 2 * st.n) * 8 <= 96 * 1024
    assert long_rows == (name == "chain520")
    assert lds_path == (not rows_kernel and name != "chain520")
    u, t = _states(st, name, B, seed=5)
    rng = np.random.default_rng(6)
    du = (rng.random((B, st.n)) - 0.5) * 1e6
    h.rebuild(u, t)
    G, Cm, b, _ = h.get_GCb()
    r = h.residual(du, u)
    c = R.residual_check(r, G, Cm, b, u, du, st)
    assert c.ok, (name, c)
    gam = np.array([1e7, 3.3e9, 1e12])
    J = h.jacobian(gam)
    assert R.jacobian_ok(J, G, Cm, gam), name
    if st.n <= 300:
        Jd = h.jacobian_dense(gam)
        rows, cols = np.asarray(st.ref_rowval), np.repeat(np.arange(st.n), np.diff(st.ref_colptr))
        assert np.array_equal(Jd[:, rows, cols], J)
        mask = np.ones((st.n, st.n), bool); mask[rows, cols] = False
        assert np.all(Jd[:, mask] == 0.0)
    # the ODE forms restamp: checked against their own restamp's G and b (words summed with atomics may differ in the last bits)
    du_ode = h.ode_rhs(u, t)
    G3, C3, b3, _ = h.get_GCb()
    c = R.residual_check(-du_ode, G3, C3, b3, u, np.zeros_like(u), st)
    assert c.ok, (name, "ode_rhs", c)
    Jo = h.ode_jacobian(u, t)
    assert np.array_equal(Jo, -h.get_GCb()[0])
    h.close()


def _orphan_diag_circuit():
    """An RC charge with one node that only a capacitor touches (its G diagonal: gshunt alone, k_stamp_prep), one chunk per type: no
    atomics, so k_stamp_prep runs only while gshunt is on and once after (prep_stale)."""
    from tests.circuits import rc_charge
    return tiled(rc_charge(), 1, cap_node="cq")


def _check_all(st, h, u, t, gshunt=0.0, srcFact=1.0):
    h.rebuild(u, t)
    (G, Cm, b), _, _, checks = _check_reduction(st, h, u, t, gshunt, srcFact)
    empty_g = np.diff(st.g_ptr)[np.argsort(st.to_ref_nz)] == 0
    diag = np.zeros(st.nnz, bool)
    dn = np.asarray(st.diag_nz)
    diag[dn[dn >= 0]] = True
    diag = diag[np.argsort(st.to_ref_nz)]
    assert np.all(G[:, empty_g & ~diag] == 0.0) and np.all(G[:, empty_g & diag] == gshunt)
    assert np.all(Cm[:, np.diff(st.c_ptr)[np.argsort(st.to_ref_nz)] == 0] == 0.0) and np.all(b[:, np.diff(st.b_ptr) == 0] == 0.0)
    return G, Cm, b


@pytest.mark.parametrize("name", ["dff", "orphan", "chain40"])
def test_modes_gshunt_srcfact_and_state_sequences(name, monkeypatch):
    """(e) tran / dcop / tranop and initjct against the oracle; gshunt 1e-3 then 0 (unstamped diagonals back to exactly 0); srcFact 0.3;
    and a rebuild after dc_run (per-op and fused), tran_run and factor_solve on the same handle: every entry still within its bound and
    every entry without a contribution exactly 0 -- no other kernel has left data in G, C or b."""
    B = 3
    if name == "orphan":
        circ, params = _orphan_diag_circuit(), {}
    else:
        circ, params = CASES[name][0](), CASES[name][1]
    st = cj.discover(circ, params)
    assert name != "orphan" or any(st.diag_nz[i] >= 0 and st.g_ptr[st.diag_nz[i] + 1] == st.g_ptr[st.diag_nz[i]] for i in range(st.n_nodes))
    h = hip.Handle(st, B)
    temps = np.array([-20.0, 27.0, 100.0])
    h.set_params(cj.pack_params(st, circ, {k: np.full(B, float(v)) for k, v in params.items()}, temps, B))
    u, t = _states(st, name, B, seed=9)
    for mode in ("tran", "dcop", "tranop"):
        h.set_spec(mode=mode)
        for initjct in ((False, True) if mode == "tranop" else (False,)):
            h.set_initjct(initjct)
            uu = np.zeros_like(u) if initjct else u
            h.rebuild(uu, t)
            G, Cm, b = _check_all(st, h, uu, t)
            h.set_initjct(False)
            for i in (0, 2):
                ref = R.OracleStamper(circ, params, mode=mode, temp=float(temps[i]), st=st).rebuild(uu[i], float(t[i]), initjct=initjct)
                for c in R.check_stamp(_csr(st, G)[i], _csr(st, Cm)[i], b[i], ref, rho=RHO, st=st, u=uu[i]):
                    assert c.ok, (name, mode, initjct, i, c)
    h.set_spec(mode="tran")
    for gsh, sf in ((1e-3, 1.0), (0.0, 1.0), (0.0, 0.3), (0.0, 1.0)):
        h.set_spec(gshunt=gsh, srcFact=sf)
        h.rebuild(u, t)
        G, Cm, b = _check_all(st, h, u, t, gshunt=gsh, srcFact=sf)
        ref = R.OracleStamper(circ, params, temp=float(temps[1]), st=st).rebuild(u[1], float(t[1]), gshunt=gsh, srcFact=sf)
        for c in R.check_stamp(_csr(st, G)[1], _csr(st, Cm)[1], b[1], ref, rho=RHO, st=st, u=u[1]):
            assert c.ok, (name, gsh, sf, c)
    h.set_spec(gshunt=0.0, srcFact=1.0)
    # other kernels on the same handle, then a plain rebuild
    h.rebuild(u, t)
    h.jacobian(np.full(B, 1e9))
    h.analyze()
    h.dc_run(abstol=1e-9)
    _check_all(st, h, u, t)
    if name == "dff":
        h.dc_run(abstol=1e-9, fused=True)
        _check_all(st, h, u, t)
    h.tran_run(0.0, 2e-9, st.state_abstol(vntol=1e-6, iabstol=1e-9, chgtol=1e-6), 1e-3, save_t=[2e-9])
    _check_all(st, h, u, t)
    h.set_spec(mode="tran")
    h.rebuild(u, t)
    h.factor_solve(np.full(B, 1e9), np.ones((B, st.n)))
    _check_all(st, h, u, t)
    h.close()


def test_c6288_reduction_at_one_instance(monkeypatch, capfd):
    """The 16 x 16 multiplier (10 112 sp_mos1, n = 75 908): 316 chunks, supply rails summed from every chunk by atomics after deep
    5-ary trees -- the G target with 43 456 contributions and the b row with 14 656 -- each within gamma_{k+1} of its exact sum."""
    from cadnip_jl_amd import api
    from tools.c6288 import deck
    monkeypatch.setenv("CADNIP_SC_DEBUG", "1")
    sim = api.BatchSimulator(api.MNACircuit(deck(0xBEEF, 0x1234), {}, api.MNASpec(mode="tran")), [{}])
    st, h = sim.st, sim.h
    assert int(np.max(np.diff(st.g_ptr))) == 43456 and int(np.max(np.diff(st.b_ptr))) == 14656
    u = np.random.default_rng(1).random((1, st.n)) * 1.2
    capfd.readouterr()
    h.rebuild(u, 0.0)
    red = _reduce_launches(st, _launches(capfd), 1)
    mos = [d for d in red if d["block"].type == "MOS1"][0]
    assert mos["chunks"] == 316 and mos["levels"] >= 4 and _atomic_targets(st, mos["block"], mos["cs"]) >= 1
    _check_reduction(st, h, u, np.zeros(1))
    sim.close()


def test_generated_model_tiles_cut_to_64k(monkeypatch, capfd):
    """The flip-flop with the generated level-1 MOSFET (va_mos1l: 192 slots per device, 30 devices in one chunk, two instances per wave).
    The read-out pass stages every slot: 2 x 30 x 192 words exceed 64 KB, so the limit cuts its waves to one instance; the reducing
    pass (packed rows) keeps two.  The reduction of the one against the contributions of the other, at B = 1, 7 and 65."""
    from cadnip_jl_amd import benchmarks as bm
    monkeypatch.setenv("CADNIP_SC_DEBUG", "1")
    circ = bm.dff_circuit(generated=True)
    st = cj.discover(circ, {"vdd": 5.0})
    for B in (1, 7, 65):
        h = hip.Handle(st, B)
        h.set_params(cj.pack_params(st, circ, {"vdd": np.linspace(4.5, 5.5, B)}, np.linspace(-40.0, 125.0, B), B))
        h.set_spec(mode="tran")
        u, t = _states(st, "dff", B, seed=B)
        h.rebuild(u, t)
        capfd.readouterr()
        _check_reduction(st, h, u, t)
        launches = _launches(capfd)
        red = _reduce_launches(st, launches, B)
        va = [d for d in red if d["block"].type == "VA:va_mos1l"][0]
        assert va["chunks"] == 1 and va["ipw"] == 2 == min(8, 64 // va["count"]), va
        ro = [d for d in launches if d["readout"] and d["type"] == va["type"]][0]
        assert ro["rows"] == ro["slots"] == 192 and ro["ipw"] == 1 and 2 * ro["tile_words"] * 8 > 64 * 1024, ro
        assert ro["grid"] == B and ro["u_lds"] == 1
        h.close()


@pytest.mark.parametrize("fixture", ["nmos_card", "bsim4_nmos", "ring"])
def test_external_models_reduction(fixture, monkeypatch, capfd):
    """PSP103 and BSIM4 (generated external models, one kernel each, 16 or 32 lanes per device): the reduction at B = 1, 7 and 65, with
    the launch geometry of every block (the ring: 18 devices, 4 per chunk of 16-lane groups, 5 chunks)."""
    from tests.test_gpu_psp103 import _sim as psim
    monkeypatch.setenv("CADNIP_SC_DEBUG", "1")
    for B in (1, 7, 65):
        st, x, sim = psim(fixture, B=B)
        h = sim.h
        u = np.random.default_rng(B).random((B, st.n)) * 1.2
        capfd.readouterr()
        h.rebuild(u, 0.0)
        red = _reduce_launches(st, _launches(capfd), B)
        va = [d for d in red if d["block"].type.startswith("VA:")]
        assert va and all(d["lpd"] in (16, 32) and d["cs"] == min(d["count"], 64 // d["lpd"]) for d in va), va
        _check_reduction(st, h, u, np.zeros(B))
        sim.close()
