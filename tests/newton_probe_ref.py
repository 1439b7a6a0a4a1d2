"""Reference of the single-Newton-update probes (tests/test_newton_probe_cpu.py: the CPU port; tests/test_gpu_newton_probe.py: the per-op
kernels and every form of the fused kernels).  Nothing here comes from a kernel.

Two existing calls perform exactly one Newton update from a given state u0:

* DC probe (J = G).  ``dc_run(u0, abstol=1e-300, maxiters=1, cold_start=False, use_stepping=False)``: round 0 stamps at u0, finds the norm
  above abstol, solves and updates; round 1 ends with status -3 before anything else changes u.  u1 = u0 - G(u0)^-1 (G(u0) u0 - b(u0)); with
  PCNR the limit slots of u1 are then overwritten by limit_w(u0).
* Transient probe (J = G + C / h).  ``tran_run(t0, t0 + h, abstol=1e30, reltol=1, h0=hmax=h, newton_tol=1, err_mask=0, max_order=2)`` after
  ``set_u(u0)``: with one history point the predictor is u0 and a0 = 1 / h, with h a power of two du = a0 u0 + beta is exactly 0, with atol = 1e30
  the weighted update norm is ~0 and round 0 converges in both Newton modes, the error test is off (nhist < 2) and tn >= t1 ends the run:
  one accepted step, one Newton iteration.  u1 = u0 - (G + C / h)^-1 (G u0 - b), everything stamped at (u0, t0 + h).

The reference: stamps from stamp_ref.OracleStamper in the probe's mode, summed in long double; J_ref and F_ref in long double; delta_ref by
lu_ref.refined_solve; limit values the oracle's limit_w.  The check is a backward error (kappa(J) reaches 1e6 and more, a forward tolerance
would be loose or flaky): with delta = u0 - u1 from the code under test, every row i must meet

    |F_ref - J_ref delta|_i <= OMEGA (|J_ref| |delta| + |F_ref|)_i + sum_j E_J[i, j] |delta_j| + E_F[i] + u sum_j |J_ref[i, j]| |u1_j|

OMEGA = 1e-12 (test_gpu_lu_kernels.OMEGA), E_J = E_G + E_C / h, E_F[i] = sum_j E_G[i, j] |u0_j| + E_b[i], and E_G, E_C, E_b the entrywise
bounds of the stamping tests (stamp_ref.stamp_bounds with stamp_ref.RHO: gamma_{k+1} S plus the RHO / FLOOR allowances of the slots).  A row
with 0 <= 0 passes.

The last term is the read-out's, not the solver's (u = 2^-53).  A probe returns u1 = fl(u0 - delta): one rounding of at most u |u1_j| per
unknown, which the difference u0 - u1 hands back as an error of delta, whatever computed delta.  Where an update is small beside its unknown
-- linear_zoo's inductor current of 0.5 mA, which a step of 2^-42 s moves by 1e-10 A past L / h = 4.4e9 -- that rounding alone, on the exact
delta_ref, is four orders of magnitude above the first three terms (tests/test_newton_probe_cpu.py prints the figure per circuit: every
other circuit's rounded delta_ref passes without the term).  Beside a node voltage of 5 V that the smallest perturbation moves by 0.05 V it
is u 5 / (OMEGA 0.05) = 1e-2 of OMEGA |J| |delta|.

Two details of the reference's own solve (`solve`, `dc_point`): the flip-flop has a 0 V ammeter source whose node row reads -I = 0.  The
dense DC solve leaves 1e-35 A in I, the refinement 1e-41 A; against a row bound of OMEGA times that, both are errors of 1e5 .. 1e11 bounds.
So DC-point values below 1e-30 are set to 0, and a row with a single entry fixes its unknown exactly, delta_j = F_i / J_ij.

States.  Uniformly random unknowns are unusable (junctions volts into forward bias: kappa 1e45 and beyond).  A state is the circuit's tranop DC
point (port_util.dense_dc_start: dense Newton on the oracle port's stamps) plus a uniform perturbation of +-0.05, +-0.3 or +-1.0 V on the node
voltages; branch currents and charge unknowns stay at the DC point; the limit slots are the oracle's limit_w at the perturbed state.

A limit unknown's column holds its own row's unit diagonal only (devices_ref.limit; `reference` asserts it), so under PCNR, where the limit
slots of u1 are limit_w and their Newton update is lost, every other row is checked as it stands and the limit rows are replaced by the
comparison of the slots with the oracle's limit_w (allowance: stamp_ref.RHO's default times max(1, max |limit_w|), as test_gpu_parity holds
limit_w)."""
import functools
import zlib

import numpy as np

from cadnip_jl_amd import benchmarks as bm
from tests import circuits as tc
from tests import lu_ref as LR
from tests import stamp_ref as SR
from tests.tran_exact_cases import INV_CORNERS

LD = np.longdouble
OMEGA = 1e-12                                   # tests/test_gpu_lu_kernels.OMEGA
AMPS = (0.05, 0.3, 1.0)                         # V, uniform perturbation of the node voltages around the DC point: one state each
HS = (2.0 ** -30, 2.0 ** -36, 2.0 ** -42)       # s: G-comparable, mixed, C-dominated
T0 = 0.0                                        # a multiple of every h: t0 + h is exact
REFINE_STEPS = 6                                # of lu_ref.refined_solve: kappa u = 1e-4 per step at kappa = 1e12, down to long double
NOISE = 1e-30                                   # V, A, C: below it a DC-point value is the dense solve's rounding noise
PIN_LEVEL = 1e-4                                # an entry is pinned where 1e-4 |J_ij delta_ref_j| exceeds its row's bound
PIN_CAP = 0.8                                   # share of a circuit's structurally non-zero entries that must be pinned

# (kind, mode, state, h): both DC modes at every state; every step size at every state
PROBES = tuple(("dc", mode, s, None) for mode in ("dcop", "tranop") for s in range(len(AMPS))) + \
    tuple(("tran", "tran", s, h) for s in range(len(AMPS)) for h in HS)


def _factories():
    from tests import test_gpu_tran_parity as TP
    return {"inverter": bm.inverter_circuit, "dff": bm.dff_circuit, "nonlinear": TP._nonlinear_tran, "diode_limited": tc.diode_rectifier,
            "behavioral": tc.behavioral, "meyer_inverter_rd": TP._meyer_inverter, "linear_zoo": tc.linear_zoo}


# lean: what csrc/fused2.hip (fused2_blocks) gives the sweep kernel's lean variant 0 and the team kernel -- the two CMOS circuits and
# linear_zoo, whose linear builtins are all in the lean device set; the others take the full-table variant 1
SUPPLY = ("inverter", "dff")                    # circuits with a `vdd` parameter
LEAN = SUPPLY + ("linear_zoo",)
NON_LEAN = ("nonlinear", "diode_limited", "behavioral", "meyer_inverter_rd")
CIRCUITS = LEAN + NON_LEAN
N_CORNERS = len(INV_CORNERS)


def make(name):
    return _factories()[name]()


def points(name):
    """Nine distinct corners: (vdd, temp) of tran_exact_cases.INV_CORNERS (all inside the range that file documents) where the circuit
    has a supply parameter, its nine temperatures elsewhere."""
    if name in SUPPLY:
        return [{"vdd": v, "temp": t} for v, t in INV_CORNERS]
    return [{"temp": t} for _, t in INV_CORNERS]


def params_of(pt):
    return {k: v for k, v in pt.items() if k != "temp"}


def vscale(name):
    """BatchSimulator.vscale's rule on the probe's points (the scale of analyze's random samples), without a device."""
    v = [abs(float(x)) for pt in points(name) for x in params_of(pt).values()] + [1.0]
    for d in make(name).devices:
        if d.type == "V":
            dc = d.params.get("dc", 0.0)
            if not hasattr(dc, "name"):
                v.append(abs(float(dc)))
            if d.wave is not None and d.wave[0] == "pwl":
                v.append(max(abs(float(y)) for y in d.wave[2]))
    return max(v)


@functools.lru_cache(maxsize=None)
def structure(name):
    import cadnip_jl_amd as cj
    return cj.discover(make(name), params_of(points(name)[0]))


@functools.lru_cache(maxsize=None)
def stamper(name, i, mode):
    pt = points(name)[i]
    return SR.OracleStamper(make(name), params_of(pt), mode=mode, temp=pt["temp"], st=structure(name))


@functools.lru_cache(maxsize=None)
def dc_point(name, i):
    from tests.port_util import dense_dc_start
    pt = points(name)[i]
    u = dense_dc_start(make(name), params_of(pt), pt["temp"])
    # what the dense solve leaves in an unknown whose value is 0 (1e-35 A in the flip-flop's 0 V ammeter source) is rounding noise of that
    # solve, not a state: as an exact 0 the row reads 0 = 0
    return np.where(np.abs(u) < NOISE, 0.0, u)


def probe_time(probe):
    return 0.0 if probe[0] == "dc" else T0 + probe[3]


class Ref:
    """One probe of one instance: u0, J (dense, long double), F, delta_ref, the bound's E_J (dense) and E_F, the oracle's limit_w."""

    def __init__(self, st, u0, J, F, EJ, EF, limit_w, stamp=None, a0=0.0):
        self.st, self.u0, self.J, self.F, self.EJ, self.EF, self.limit_w = st, u0, J, F, EJ, EF, limit_w
        self.stamp, self.a0 = stamp, a0            # the oracle's contributions and 1 / h (0 in a DC probe): J = G + a0 C
        self.delta = solve(J, F)
        self.absJ = np.abs(J)
        self.lim0 = st.n - st.n_limits

    def bound(self, delta, readout=True):
        """the row bounds at an update delta; readout=False: without the read-out's term (a figure of the CPU test, never a check)"""
        d = np.abs(np.asarray(delta, dtype=LD))
        bd = LD(OMEGA) * (self.absJ @ d + np.abs(self.F)) + self.EJ @ d + self.EF
        if readout:
            bd = bd + LD(SR.U) * (self.absJ @ np.abs(self.u0.astype(LD) - np.asarray(delta, dtype=LD)))
        return bd

    def ratios(self, delta, J=None, readout=True):
        """per row |F - J delta| / bound (0 where both are 0); ``J``: another matrix in the residual (the sensitivity test's faulty one)"""
        d = np.asarray(delta, dtype=LD)
        res = np.abs(self.F - (self.J if J is None else J) @ d)
        bd = self.bound(d, readout)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.asarray(np.where(res == 0, LD(0), res / np.where(bd > 0, bd, LD(1e-300))), dtype=np.float64)

    def check(self, u1, pcnr=False):
        """(worst backward ratio, its row, forward error against u0 - delta_ref, worst limit-slot ratio) of an updated state u1.
        pcnr: the limit slots of u1 hold limit_w; their rows leave the backward check and the slots are compared with the oracle's."""
        u1 = np.asarray(u1, dtype=np.float64)
        delta = self.u0.astype(LD) - u1.astype(LD)
        live = np.ones(self.st.n, dtype=bool)
        lim = 0.0
        if pcnr and self.st.n_limits:
            live[self.lim0:] = False
            delta[self.lim0:] = 0          # the limit columns are zero in every live row
            lim = float(np.max(np.abs(u1[self.lim0:] - self.limit_w))) / (SR.RHO["default"] * max(1.0, float(np.max(np.abs(self.limit_w)))))
        if not np.all(np.isfinite(u1)):
            return np.inf, -1, np.inf, lim
        r = np.where(live, self.ratios(delta), 0.0)
        fwd = float(np.max(np.abs(np.asarray(delta - self.delta, dtype=np.float64))[live]))
        return float(np.max(r)), int(np.argmax(r)), fwd, lim


def dense(st, vals):
    rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
    return LR.dense(vals, rows, np.asarray(st.colidx, dtype=np.int64), st.n)


def perturbed(name, i, s):
    """The DC point with the node voltages moved by AMPS[s] * uniform(-1, 1) (seeded by circuit, corner and state)."""
    st = structure(name)
    u = dc_point(name, i).copy()
    rng = np.random.default_rng([zlib.crc32(name.encode()), i, s])
    u[:st.n_nodes] += AMPS[s] * (2.0 * rng.random(st.n_nodes) - 1.0)
    return u


@functools.lru_cache(maxsize=None)
def reference(name, i, probe):
    """The Ref of instance i of a circuit under one of PROBES, computed once per process."""
    kind, mode, s, h = probe
    st = structure(name)
    o = stamper(name, i, mode)
    t = probe_time(probe)
    u0 = perturbed(name, i, s)
    if st.n_limits:
        u0[st.n - st.n_limits:] = o.rebuild(u0, t).limit_w
    ref = o.rebuild(u0, t)
    (G, EG), (Cm, EC), (b, Eb) = SR.stamp_bounds(ref, rho=SR.RHO, st=st, u=u0)
    a0 = LD(0) if kind == "dc" else LD(1) / LD(h)
    Gd, EGd = dense(st, G), dense(st, EG)
    J, EJ = Gd + a0 * dense(st, Cm), EGd + a0 * dense(st, EC)
    ul = u0.astype(LD)
    F, EF = Gd @ ul - b, EGd @ np.abs(ul) + Eb
    L = st.n_limits
    if L:
        assert not np.any(J[:st.n - L, st.n - L:]), "a limit unknown outside its own row"
    return Ref(st, u0, J, F, EJ, EF, ref.limit_w.copy(), ref, float(a0))


def start_states(name, probe, B=N_CORNERS):
    """[B, n] u0 of a batch that tiles the nine corners."""
    return np.stack([reference(name, i % N_CORNERS, probe).u0 for i in range(B)])


def check_batch(name, probe, u1, pcnr=False):
    """Every instance of an updated batch [B, n] (instance i is corner i % 9) against its reference: the worst (backward ratio, (instance, row),
    forward error, limit ratio)."""
    worst, where, fwd, lim = 0.0, None, 0.0, 0.0
    for i, row in enumerate(np.asarray(u1)):
        r, k, f, l = reference(name, i % N_CORNERS, probe).check(row, pcnr)
        if r > worst or where is None:
            worst, where = max(worst, r), (i, k)
        fwd, lim = max(fwd, f), max(lim, l)
    return worst, where, fwd, lim


def pattern_mask(name):
    st = structure(name)
    return dense(st, np.ones(st.nnz)) != 0


@functools.lru_cache(maxsize=None)
def coverage(name):
    """(pinned [n, n] bool, structural [n, n] bool, witness [n, n] int): entry (i, j) is pinned if in at least one probe of the circuit (any
    corner) PIN_LEVEL |J_ij delta_ref_j| > bound_i at delta_ref -- from the reference alone; witness = corner * len(PROBES) + probe number of
    the first probe that pins it, -1 without one."""
    pat = pattern_mask(name)
    witness = np.full(pat.shape, -1, dtype=np.int64)
    for i in range(N_CORNERS):
        for k, probe in enumerate(PROBES):
            r = reference(name, i, probe)
            bd = r.bound(r.delta)
            hit = pat & (LD(PIN_LEVEL) * r.absJ * np.abs(r.delta)[None, :] > bd[:, None])
            witness[hit & (witness < 0)] = i * len(PROBES) + k
    return witness >= 0, pat, witness


def witness_ref(name, w):
    return reference(name, int(w) // len(PROBES), PROBES[int(w) % len(PROBES)])


def unknown_name(st, k):
    names = list(st.node_names) + list(st.current_names) + list(st.charge_names) + list(st.limit_names)
    return names[k]


def entry_slots(st, i, j):
    """The device slots that stamp entry (i, j): [(array, block type, local slot number)]."""
    out = []
    e = [q for q in range(st.rowptr[i], st.rowptr[i + 1]) if st.colidx[q] == j]
    for which, ptr, slots in (("g", st.g_ptr, st.g_slots), ("c", st.c_ptr, st.c_slots)):
        for q in e:
            for sl in np.asarray(slots)[ptr[q]:ptr[q + 1]]:
                for blk in st.blocks:
                    base, nk = (blk.g_base, blk.n_g) if which == "g" else (blk.c_base, blk.n_c)
                    if blk.count and base <= sl < base + nk * blk.count:
                        out.append((which, blk.type, int((sl - base) // blk.count)))
    return out


def unpinned_report(name):
    """The unpinned structural entries by the device slots behind them: one line per slot signature with the number of entries and one example
    (row and column names)."""
    st = structure(name)
    pinned, pat, _ = coverage(name)
    groups = {}
    for i, j in np.argwhere(pat & ~pinned):
        sig = ", ".join("%s %s[%d]" % (t, w, k) for w, t, k in sorted(set(entry_slots(st, int(i), int(j)))))
        groups.setdefault(sig, []).append((unknown_name(st, i), unknown_name(st, j)))
    return ["%s  %3d x  %s   e.g. (%s, %s)" % ((name, len(v), sig) + v[0]) for sig, v in sorted(groups.items())]


def solve(J, F):
    """delta of J delta = F as the reference solves it: lu_ref.refined_solve to long double, then the rows with one entry, which fix their
    unknown by themselves: delta_j = F_i / J_ij -- exactly 0 where F_i is (the flip-flop's 0 V ammeter source: -I = 0), where the refinement
    leaves the long-double noise of the other rows (1e-41 A)."""
    delta = LR.refined_solve(J, F, steps=REFINE_STEPS)
    for i in np.nonzero(np.count_nonzero(J, axis=1) == 1)[0]:
        j = int(np.nonzero(J[i])[0][0])
        delta[j] = F[i] / J[i, j]
    return delta
