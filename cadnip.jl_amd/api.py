"""Reference-shaped user API on top of the GPU hot path.

Mirrors the surface a Cadnip.jl user touches on this path -- same names, argument meaning and
result layout -- so that tests read like the reference's own:

    MNASpec, MNACircuit, alter                       /root/reference/src/mna/solve.jl:57-70, 1585-1597, 1719-1732
    dc(circuit) / tran(circuit, tspan)               /root/reference/src/sweeps.jl:450-455, 588-665   (dc! / tran!)
    Sweep, ProductSweep, TandemSweep, SerialSweep    /root/reference/src/sweeps.jl:150-330
    CircuitSweep, SweepResult, dc(cs), tran(cs)      /root/reference/src/sweeps.jl:387-424, 477-532, 692-707
    solution layout [V | I | q*1e12 | v_lim], sol[name]   /root/reference/src/mna/build.jl:39-51, 421-457

Differences forced by the target: a ``MNACircuit`` wraps a flattened device table instead of a
generated Julia builder; ``tran``/``dc`` over a ``CircuitSweep`` integrate all sweep points as
one resident batch on the GPU instead of the reference's serial loop (sweeps.jl:696-703);
temperature is a per-point axis (``temp`` key), which the reference can only reach through an
outer loop over ``MNASpec``.
"""
import itertools
from dataclasses import dataclass, field, replace
from typing import Any, Dict, List, Optional

import numpy as np

from .circuit import Circuit
from .structure import Structure, discover, expand_breakpoints, pack_params


@dataclass(frozen=True)
class MNASpec:
    temp: float = 27.0
    mode: str = "tran"
    time: float = 0.0
    gmin: float = 1e-12
    gshunt: float = 0.0
    srcFact: float = 1.0
    tnom: float = 27.0
    abstol: float = 1e-12
    reltol: float = 1e-3
    vntol: float = 1e-6
    iabstol: float = 1e-12


def with_mode(spec, mode):
    return replace(spec, mode=mode)


def with_temp(spec, temp):
    return replace(spec, temp=float(temp))


@dataclass(frozen=True)
class MNACircuit:
    circuit: Circuit
    params: Dict[str, float] = field(default_factory=dict)
    spec: MNASpec = MNASpec()


def alter(c: MNACircuit, spec: Optional[MNASpec] = None, **params) -> MNACircuit:
    """solve.jl:1719-1732: new circuit with some parameters (or the spec) replaced."""
    p = dict(c.params)
    for k, v in params.items():
        if k not in p:
            raise KeyError("unknown circuit parameter %r" % k)
        p[k] = v
    return MNACircuit(c.circuit, p, spec if spec is not None else c.spec)


# ------------------------------------------------------------------------------------------------
# sweeps (sweeps.jl:150-330)
# ------------------------------------------------------------------------------------------------
class Sweep:
    def __init__(self, **axes):
        if len(axes) != 1:
            raise ValueError("Sweep takes exactly one name=values axis; combine with ProductSweep/TandemSweep")
        (self.name, vals), = axes.items()
        self.values = list(vals)

    def __iter__(self):
        return ({self.name: v} for v in self.values)

    def __len__(self):
        return len(self.values)


class ProductSweep:
    """Cartesian product, first axis fastest (Base.Iterators.product, sweeps.jl:272)."""

    def __init__(self, *sweeps, **axes):
        self.sweeps = list(sweeps) + [Sweep(**{k: v}) for k, v in axes.items()]

    def __iter__(self):
        lists = [list(s) for s in self.sweeps]
        for combo in itertools.product(*reversed(lists)):
            d = {}
            for part in reversed(combo):
                d.update(part)
            yield d

    def __len__(self):
        return int(np.prod([len(s) for s in self.sweeps]))


class TandemSweep:
    def __init__(self, *sweeps, **axes):
        self.sweeps = list(sweeps) + [Sweep(**{k: v}) for k, v in axes.items()]
        if len({len(s) for s in self.sweeps}) > 1:
            raise ValueError("TandemSweep axes must have equal lengths")

    def __iter__(self):
        for parts in zip(*self.sweeps):
            d = {}
            for p in parts:
                d.update(p)
            yield d

    def __len__(self):
        return len(self.sweeps[0]) if self.sweeps else 0


class SerialSweep:
    def __init__(self, *sweeps):
        self.sweeps = list(sweeps)

    def __iter__(self):
        return itertools.chain(*self.sweeps)

    def __len__(self):
        return sum(len(s) for s in self.sweeps)


class CircuitSweep:
    """sweeps.jl:387-424.  Sweep keys name circuit parameters; the extra key ``temp`` sweeps
    MNASpec.temp."""

    def __init__(self, circuit: MNACircuit, iterator):
        self.circuit = circuit
        self.iterator = iterator
        for pt in iterator:
            for k in pt:
                if k != "temp" and k not in circuit.params:
                    raise KeyError("sweep variable %r is not a circuit parameter" % k)

    def points(self):
        return list(self.iterator)

    def __len__(self):
        return len(self.iterator)


class SweepResult:
    """sweeps.jl:477-487: iterates (params, solution) pairs."""

    def __init__(self, points, solutions):
        self.points = points
        self.solutions = solutions

    def __iter__(self):
        return iter(zip(self.points, self.solutions))

    def __len__(self):
        return len(self.points)

    def __getitem__(self, i):
        return self.solutions[i]


# ------------------------------------------------------------------------------------------------
# solutions
# ------------------------------------------------------------------------------------------------
class DCSolution:
    """solve.jl:156-166; name lookup in the reference's order -- nodes, currents, charges, limits, then device terminal
    currents ``i_<device>_<terminal>`` and operating-point variables ``<device>_<var>`` (solve.jl:234-250, test/opinfo.jl)."""

    def __init__(self, st: Structure, x, converged, op=None):
        self.st = st
        self.x = np.asarray(x)
        self.converged = bool(converged)
        self.op = dict(op or {})
        self.node_names = st.node_names
        self.current_names = st.current_names
        self.charge_names = st.charge_names
        self.limit_names = st.limit_names
        self.n_nodes = st.n_nodes

    def __getitem__(self, name):
        try:
            return float(self.x[self.st.index_of(name)])
        except KeyError:
            if name in self.op:
                return self.op[name]
            raise

    def terminal_currents(self):
        return {k: v for k, v in self.op.items() if k.startswith("i_")}

    def op_vars(self):
        return {k: v for k, v in self.op.items() if not k.startswith("i_")}

    def keys(self):
        return list(self.st.node_names) + list(self.st.current_names) + list(self.op)

    def __contains__(self, name):
        return name in self.op or name in self.st.node_names or name in self.st.current_names


class TranSolution:
    """What the path hands back: states at the requested ``saveat`` times plus solver statistics
    (sol.t, sol[name], sol(t), sol.stats.nnonliniter as in benchmarks/vacask/ring/cedarsim/runme.jl:74-76)."""

    def __init__(self, st, t, u, stats, retcode):
        self.st = st
        self.t = np.asarray(t)
        self.u = np.asarray(u)          # [n_save, n]
        self.stats = stats
        self.retcode = retcode
        # tran(..., sens=[names]): d u / d p_k at the save times [K, n_save, n], the names, the parameter steps of the central differences
        # [K] and the flag (1: a sensitivity solve met a bad pivot or a non-finite value, NaN from that step on); None / empty without it
        self.sens, self.sens_params, self.sens_steps, self.sens_flag = None, [], None, 0

    def __getitem__(self, name):
        return self.u[:, self.st.index_of(name)]

    def sensitivity(self, name, param):
        """d ``name`` / d ``param`` at the save times [n_save], of a run asked for with ``sens=``."""
        if self.sens is None or param not in self.sens_params:
            raise KeyError("no sensitivity with respect to %r was computed (tran(..., sens=[...]))" % (param,))
        return self.sens[self.sens_params.index(param)][:, self.st.index_of(name)]

    def __call__(self, t, name=None):
        cols = self.u if name is None else self.u[:, self.st.index_of(name)]
        if cols.ndim == 1:
            return float(np.interp(t, self.t, cols))
        return np.array([np.interp(t, self.t, cols[:, j]) for j in range(cols.shape[1])])


def nameat(sol, name, t):
    """solve.jl:347-353"""
    return sol(t, name)


# ------------------------------------------------------------------------------------------------
# batched simulator
# ------------------------------------------------------------------------------------------------
def clip_sample(J, headroom=1e6):
    """|J| of one or more sample Jacobians ([.., nnz]) for the symbolic phase, each sample clipped to ``headroom`` times
    the median of its non-zero magnitudes (non-finite entries count as the cap).  A random probe point can forward-bias
    an exponential junction by volts: its conductance (1e30 and more) would swamp every other entry of the sample, and
    the pivot search -- which eliminates numerically -- would see a singular matrix where only the probe was absurd."""
    a = np.abs(np.atleast_2d(np.asarray(J, dtype=float)))
    out = np.empty_like(a)
    for i, row in enumerate(a):
        fin = np.isfinite(row)
        nz = row[fin & (row > 0)]
        cap = headroom * float(np.median(nz)) if nz.size else 0.0
        r = np.where(fin, row, cap)
        out[i] = np.minimum(r, cap) if nz.size else 0.0
    return out


class BatchSimulator:
    """One structure, B resident sweep instances on one GPU."""

    @classmethod
    def from_packed(cls, st: Structure, packed, spec: Optional[MNASpec] = None, device: int = 0, vscale: float = 1.0):
        """A simulator from a ready structure and packed per-instance parameter blocks (``pack_params`` output, one array
        [B, n_par, count] per block) -- e.g. loaded with ``structure.load_structure`` on a machine that holds the library's generated
        model code but not the model's Verilog-A source."""
        from . import hip
        self = cls.__new__(cls)
        spec = spec or MNASpec()
        self.mc, self.points, self.st = None, None, st
        self.B = int(np.asarray(packed[0]).shape[0])
        self.params, self.temps = {}, np.full(self.B, spec.temp)
        self._vscale = float(vscale)
        self.device = device
        self.h = hip.Handle(st, self.B, device)
        self.h.set_params([np.ascontiguousarray(p, dtype=np.float64) for p in packed])
        self.h.set_spec(mode=spec.mode if spec.mode in ("dcop", "tran", "tranop") else "tran", gmin=spec.gmin, gshunt=spec.gshunt, srcFact=spec.srcFact)
        self._analyzed = False
        return self

    def __init__(self, mc: MNACircuit, points: Optional[List[Dict[str, Any]]] = None, device: int = 0, st: Optional[Structure] = None):
        from . import hip
        self.mc = mc
        points = points if points else [{}]
        self.points = points
        B = len(points)
        self.B = B
        params = {k: np.full(B, float(v)) for k, v in mc.params.items()}
        temps = np.full(B, mc.spec.temp)
        for i, pt in enumerate(points):
            for k, v in pt.items():
                if k == "temp":
                    temps[i] = float(v)
                else:
                    params[k][i] = float(v)
        self.params, self.temps = params, temps
        p0 = {k: float(v[0]) for k, v in params.items()}
        self.st = st if st is not None else discover(mc.circuit, p0)
        self.device = device
        self.h = hip.Handle(self.st, B, device)
        self.h.set_params(pack_params(self.st, mc.circuit, params, temps, B, gmin=mc.spec.gmin, tnom_c=mc.spec.tnom))
        self.h.set_spec(mode=mc.spec.mode if mc.spec.mode in ("dcop", "tran", "tranop") else "tran",
                        gmin=mc.spec.gmin, gshunt=mc.spec.gshunt, srcFact=mc.spec.srcFact)
        self._analyzed = False

    def close(self):
        self.h.close()

    def vscale(self):
        if self.mc is None:
            return self._vscale
        v = [abs(float(np.max(np.abs(self.params[k])))) for k in self.params] + [1.0]
        for d in self.mc.circuit.devices:
            if d.type == "V":
                dc = d.params.get("dc", 0.0)
                if not hasattr(dc, "name"):
                    v.append(abs(float(dc)))
                if d.wave is not None and d.wave[0] == "pwl":
                    v.append(max(abs(float(y)) for y in d.wave[2]))
        return max(v)

    def analyze(self, gamma=1e9, n_samples=6, seed=1234, sample=None):
        """Symbolic LU phase on the element-wise max |G + gamma*C| over several operating points
        (cold start with initjct, zero, and random points) and over ALL instances of the handle, so the static pivot order suits all.
        Each sample is clipped (``clip_sample``) before it enters the max.  The order therefore belongs to the batch: a subset of
        its points analysed on its own may get another one and then agrees with the batch to rounding, not bit for bit;
        ``sample`` (the ``pivot_sample`` of another simulator of the same structure) reuses that simulator's order."""
        if sample is not None:
            self.pivot_sample = np.array(sample, dtype=float)
            self.h.analyze_values(self.pivot_sample)
            self._analyzed = True
            return
        rng = np.random.default_rng(seed)
        st, h = self.st, self.h
        vs = self.vscale()
        acc = np.zeros(st.nnz)
        for k in range(n_samples):
            if k == 0:
                u = np.zeros(st.n)
                u[st.n - st.n_limits:] = st.limit_init
                h.set_initjct(True)
            elif k == 1:
                u = np.zeros(st.n)
            else:
                u = (rng.random(st.n) * 1.2 - 0.1) * vs
                u[st.n_nodes:st.n_nodes + st.n_currents] = 0.0
            h.rebuild(u, 0.0)
            h.set_initjct(False)
            J = h.jacobian(gamma)
            acc = np.maximum(acc, np.max(clip_sample(J), axis=0))
        h.analyze_values(acc)
        self.pivot_sample = acc
        self._analyzed = True

    def analyze_at(self, u, t=0.0, gamma=0.0, instance=0):
        """Symbolic LU phase on the Jacobian ``G + gamma*C`` of one state -- KLU's first ``klu_factor``: the pivot order of
        the matrix the solver is about to meet (e.g. the first transient steps from a given start state, gamma = 1 / h).
        For circuits whose composite sample (``analyze``) does not yield a usable order."""
        uu = np.broadcast_to(np.asarray(u, dtype=float), (self.B, self.st.n)) if np.ndim(u) == 1 else np.asarray(u, dtype=float)
        self.h.rebuild(uu, t)
        self.h.analyze_values(self.h.jacobian(gamma)[instance])
        self._analyzed = True

    def dc(self, u0=None, abstol=1e-10, maxiters=100, mode="dcop", fused=False, participate=None, cold_start=None):
        self.h.set_spec(mode=mode)
        if not self._analyzed:
            self.analyze()
        return self.h.dc_run(u0, abstol=abstol, maxiters=maxiters, use_pcnr=True, cold_start=(u0 is None) if cold_start is None else cold_start,
                             fused=fused, participate=participate)

    def operating_points(self, u, mode="dcop"):
        """Terminal currents and op variables of every instance at the states ``u`` (opinfo.py): one restamp with the
        per-device contributions read back."""
        from . import opinfo
        self.h.set_spec(mode=mode)
        self.h.set_u(u)
        Sg, Sc, Sb = self.h.get_contributions()
        packed = pack_params(self.st, self.mc.circuit, self.params, self.temps, self.B, gmin=self.mc.spec.gmin, tnom_c=self.mc.spec.tnom)
        return [opinfo.operating_point(self.st, np.asarray(u)[i], Sg[i], Sb[i], packed, i) for i in range(self.B)]

    def dc_continuation(self, abstol=1e-10, maxiters=100, mode="dcop", fused=False, serial=False):
        """dc!(cs; continuation=true) (sweeps.jl:489-532) for a resident batch.  The reference walks the sweep serially and
        starts every point from the last CONVERGED solution.  Here the sweep is solved in 1 + ceil(log2 B) batch stages
        (``continuation_stages``): point 0 cold, then the midpoints, quarter points, ... each started from the nearest
        converged point of the earlier stages at a lower index (the reference's direction), else the nearest converged
        one at all, else cold; a point that failed is never a starting guess (sweeps.jl:522-524).  For a circuit with ONE
        operating point continuation changes the path Newton takes, not where it lands (test/sweep.jl:332-345).  A circuit with
        several (a latch, a Schmitt trigger, the flip-flop itself) is different: the reference's strictly serial chain i - 1 -> i
        follows one branch of the hysteresis, while a seed from B / 2 points away can land on another.  ``serial=True`` is that
        chain: B stages of one point each, every point started from its converged predecessor (B launches instead of log2 B --
        the price of following a branch).  Returns (u, converged, stats)."""
        st = self.st
        u = np.zeros((self.B, st.n))
        conv = np.zeros(self.B, dtype=bool)
        solved = np.zeros(self.B, dtype=bool)
        total = {"newton_iters": 0, "stages": 0, "cold_points": 0}
        for stage in ([[i] for i in range(self.B)] if serial else continuation_stages(self.B)):
            start = np.zeros((self.B, st.n))
            mask = np.zeros(self.B, dtype=bool)
            mask[stage] = True
            good = np.flatnonzero(solved & conv)
            for i in stage:
                j = seed_for(i, good)
                if j is None:
                    total["cold_points"] += 1                    # zeros: dc_run seeds the limit variables and arms initjct for it
                else:
                    start[i] = u[j]
            start[~mask] = u[~mask]
            ui, ci, stats = self.dc(start, abstol=abstol, maxiters=maxiters, mode=mode, fused=fused, participate=mask, cold_start=True)
            u[mask], conv[mask] = ui[mask], ci[mask]
            solved |= mask
            total["newton_iters"] += stats["newton_iters"]
            total["stages"] += 1
        return u, conv, total

    def tran(self, tspan, abstol, reltol, saveat, initializealg="tranop", u0=None, warmup_dt=1e-12, delays="refuse", delay_depth=0, sens=None,
             sens_rel_step=1e-4, **kw):
        """``initializealg``: "tranop" = CedarTranOp, a DC solve in :tranop mode at t0 (dcop.jl:160-212); "uic" = CedarUICOp
        (dcop.jl:109-151, 304-411): no DC solve -- the run starts from ``u0`` (zeros by default) and the integrator's first
        steps, backward Euler from ``warmup_dt``, relax the algebraic constraints (for oscillators and for circuits whose
        static operating point Newton does not find).

        ``delays``: what to do with delayed controlled sources and transmission lines.  "refuse" (the default, and for now the only
        behaviour a caller gets without asking: flipping it is a later change): NotImplementedError.  "history": the terms of
        ``ac_delay_overlay`` go to the handle (``hip.Handle.tran_set_delay``), which integrates with the delayed values read from a ring
        of ``delay_depth`` (0 = 1024) accepted points per instance, linearly interpolated; the steps are clamped to the smallest delay,
        the source break points are propagated through the delays (``delay_breakpoints``; stats["delay_breaks"] /
        ["delay_breaks_truncated"]), and the run uses the per-op kernels whatever ``fused`` says.  A delay that is not positive and
        finite at any point is a ValueError.  A circuit without a delayed element runs exactly as without the keyword.

        ``sens``: names of circuit parameters, or "temp", each once -- the forward (direct) sensitivities d u / d p_k of the trajectory on
        the step sequence the run takes (``_tran_sens``; csrc/tran_sens.hip).  They take no part in the error test or the step choice:
        states, counters and statuses are bit for bit those of the run without the keyword on the same pivot order (the composite sample
        of ``analyze``, taken here if no order has been chosen yet).  stats then carries "sens" [B, K, n_save, n_obs], "sens_steps" [B, K],
        "sens_flag" [B], "sens_names" and "sens_params" = K.  Without ``sens`` nothing new is called and no instance is added."""
        st = self.st
        if initializealg not in ("tranop", "uic"):
            raise ValueError("initializealg must be 'tranop' or 'uic'")
        if delays not in ("refuse", "history"):
            raise ValueError("delays must be 'refuse' or 'history'")
        breaks = expand_breakpoints(st.breakpoints, tspan)
        if sens is not None:
            return self._tran_sens(tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, sens, sens_rel_step, kw)
        if self.mc is not None and has_delay(self.mc.circuit):
            if delays == "refuse":
                refuse_delay(self.mc.circuit, "tran", "a transient needs the delayed quantity's history: ask for it with delays=\"history\" "
                             "(without it a delay-differential integrator is not built into the call)")
            return self._tran_delayed(tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, delay_depth, breaks, kw)
        return self._tran(tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, kw)

    def _tran_delayed(self, tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, delay_depth, breaks, kw):
        """the run of ``tran`` under delays="history": spec on the handle, propagated break points, spec off again"""
        spec = self.delay_spec()
        breaks, n_new, truncated = delay_breakpoints(breaks, spec["tau"], tspan)
        self.h.tran_set_delay(depth=delay_depth, **spec)
        restore = []
        try:
            # the initialisation (a DC solve on G, delays ignored) keeps the order it has; the time loop solves G - W and gets its own
            out, per, stats = self._tran(tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, kw,
                                         before_run=lambda: restore.append(self.analyze_delayed(spec, tspan[0])))
        finally:
            self.h.tran_clear_delay()
            if restore:
                self.h.analyze_values(restore[0])
        stats["delay_breaks"], stats["delay_breaks_truncated"] = n_new, truncated
        return out, per, stats

    def _tran_sens(self, tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, sens, rel_step, kw):
        """the run of ``tran`` with ``sens``: every point becomes a group base | twin | p_k + delta_k | p_k - delta_k of one resident batch
        (``sens_expand``) on a handle of its own with this simulator's pivot order; only the bases are initialised and integrate"""
        if self.mc is None:
            raise ValueError("tran: sens needs the circuit description; a simulator made from packed parameters has none")
        names, values, steps, expanded, per = sens_prepare(self.mc, self.points, sens, rel_step, tspan)
        if not self._analyzed or getattr(self, "pivot_sample", None) is None:
            self.analyze()
        G, K = len(self.points), len(names)
        members = np.arange(G * per, dtype=np.int32).reshape(G, per)
        is_base = np.zeros(G * per, dtype=bool)
        is_base[members[:, 0]] = True
        obs = kw.get("obs")
        n_obs = self.st.n if obs is None or len(obs) == 0 else len(obs)
        if isinstance(u0, np.ndarray) and u0.ndim == 2:
            u0 = np.repeat(u0, per, axis=0)
        inner = BatchSimulator(self.mc, expanded, self.device, st=self.st)
        try:
            inner.analyze(sample=self.pivot_sample)
            inner.h.tran_set_sens(members, steps, len(saveat), n_obs, kw.get("max_order", 2))
            out, per_inst, stats = inner._tran(tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, kw, participate=is_base,
                                               after_init=lambda: inner.h.tran_sens_init(zero=initializealg == "uic"))
            s, flag = inner.h.tran_sens_get()
        finally:
            inner.close()
        stats.update(sens=s, sens_steps=steps, sens_values=values, sens_flag=flag, sens_names=names, sens_params=K)
        return out[is_base], per_inst[is_base], stats

    def delay_spec(self):
        """The delayed stamps of the circuit at the simulator's points as ``hip.Handle.tran_set_delay`` takes them, from the one pure function
        (``ac_delay_overlay`` without a grid): {pos, term_pos, term_row, term_col, tau [B, T], w [B, T]}.  A delay that is not positive and
        finite at any point is a ValueError."""
        ovl = ac_delay_overlay(self.st, self.mc.circuit, self.params, omegas=(), B=self.B)
        tau = np.array([t for _, t, _ in ovl.terms]).T.reshape(self.B, len(ovl.terms))
        w = np.array([wt for _, _, wt in ovl.terms]).T.reshape(self.B, len(ovl.terms))
        if not np.all(np.isfinite(tau) & (tau > 0.0)):
            raise ValueError("tran: every delay must be positive and finite at every point (a zero delay is no delay: leave it out of the circuit)")
        o = np.array([k for k, _, _ in ovl.terms], dtype=np.int64)
        return dict(pos=ovl.pos, term_pos=o, term_row=ovl.rows[o], term_col=ovl.cols[o], tau=tau, w=w)

    def analyze_delayed(self, spec, t=0.0):
        """Symbolic LU phase for the matrix a delayed transient solves, G - W + a0 C (``spec``: ``delay_spec()``).  The composite sample of
        ``analyze`` holds the delayed stamps as if they were coefficients of the present state, and a pivot chosen on one of them -- the gain
        entry of a line's E elements is the largest of its row -- is an exact zero in G - W.  So the sample is taken again with what is LEFT
        at the delayed positions once W is gone (measured on the stamps at the handle's current state, which is preserved); a position only
        delayed stamps fill enters as zero and is never a pivot.  Returns the sample that was in force (``h.analyze_values`` of it restores
        the order)."""
        u = self.h.get_u()
        if getattr(self, "pivot_sample", None) is None:
            self.analyze()
        base = np.array(self.pivot_sample, dtype=float)
        to_ref = np.asarray(self.st.to_ref_nz)
        W = np.zeros((self.B, len(spec["pos"])))
        for k, o in enumerate(spec["term_pos"]):
            W[:, o] += spec["w"][:, k]
        self.h.rebuild(u, t)
        G = self.h.get_GCb()[0][:, to_ref]
        csr = base[to_ref]
        csr[spec["pos"]] = np.max(np.abs(G[:, spec["pos"]] - W), axis=0)
        sample = base.copy()
        sample[to_ref] = csr
        self.h.analyze_values(sample)
        self.h.set_u(u)
        self._analyzed = True
        return base

    def _tran(self, tspan, abstol, reltol, saveat, initializealg, u0, warmup_dt, breaks, kw, before_run=lambda: None, participate=None,
              after_init=lambda: None):
        """``participate`` (mask [B], None = all): who gets the tranop DC solve; ``after_init``: called with the start state on the handle,
        before the mode is switched to the transient's"""
        st = self.st
        if initializealg == "uic":
            if isinstance(u0, dict):          # {unknown name: value}: the usual .IC form
                start = np.zeros((self.B, st.n))
                for name, value in u0.items():
                    start[:, st.index_of(name)] = value
            else:
                start = np.zeros((self.B, st.n)) if u0 is None else np.broadcast_to(np.asarray(u0, dtype=float), (self.B, st.n)).copy()
            if not self._analyzed:     # pivot order from the Jacobian the first steps will meet (h = warmup_dt)
                self.analyze_at(start, t=tspan[0], gamma=1.0 / (10.0 * warmup_dt))
            self.h.set_u(start)
            after_init()
            self.h.set_spec(mode="tran")
            kw.setdefault("h0", warmup_dt)
            before_run()
            out, per, stats = self.h.tran_run(tspan[0], tspan[1], abstol, reltol, breaks=breaks, save_t=saveat, **kw)
            stats["dc_newton_iters"] = 0
            return out, per, stats
        if not self._analyzed:
            self.analyze()
        u0_, conv, dcs = self.dc(abstol=1e-9, mode="tranop", fused=bool(kw.get("fused", False)), participate=participate)
        if participate is not None:
            conv = conv | ~np.asarray(participate, dtype=bool)
        if not np.all(conv):
            raise RuntimeError("transient initialisation (CedarTranOp) failed for %d instance(s)" % int((~conv).sum()))
        after_init()
        self.h.set_spec(mode="tran")
        before_run()
        out, per, stats = self.h.tran_run(tspan[0], tspan[1], abstol, reltol, breaks=breaks, save_t=saveat, **kw)
        stats["dc_newton_iters"] = dcs["newton_iters"]
        return out, per, stats


def continuation_stages(n):
    """Index sets of the staged continuation: [0], then for stride s = 2^k (largest first) the indices i = s (mod 2s): each
    lies midway between two indices of the earlier stages, and i - s is always among them."""
    if n <= 0:
        return []
    stages = [[0]]
    s = 1
    while s < n:
        s *= 2
    s //= 2
    while s >= 1:
        idx = list(range(s, n, 2 * s))
        if idx:
            stages.append(idx)
        s //= 2
    return stages


def seed_for(i, good):
    """the converged point a staged-continuation point starts from: the nearest one below it, else the nearest at all"""
    good = np.asarray(good)
    if good.size == 0:
        return None
    below = good[good < i]
    if below.size:
        return int(below[-1])
    return int(good[np.argmin(np.abs(good - i))])


def structure_classes(mc: MNACircuit, points):
    """Partition sweep points by circuit STRUCTURE (unknowns, pattern, slot maps): a sweep may move a parameter across a
    value that changes it -- a series resistance reaching zero collapses an internal node (mos1.va:716-721,
    vasim.jl:3537-3553), a junction capacitance reaching zero removes a charge unknown (contrib.jl:214-257).  The reference
    rebuilds every point from scratch; here every class gets its own resident batch.  Discovery runs once per distinct
    value tuple of the parameters that device MODEL cards refer to (sweeping a source value or the temperature never
    changes the structure).  Returns [(point indices, Structure)]."""
    from .circuit import Param
    model_pars = sorted({v.name for d in mc.circuit.devices if d.model for v in d.model.values() if isinstance(v, Param)})
    classes, by_key, sig_class = [], {}, {}
    for i, pt in enumerate(points):
        p = dict(mc.params)
        p.update({k: v for k, v in pt.items() if k != "temp"})
        key = tuple(float(p[k]) for k in model_pars)
        if key not in by_key:
            st = discover(mc.circuit, {k: float(v) for k, v in p.items()})
            sig = st.signature()
            if sig not in sig_class:
                sig_class[sig] = len(classes)
                classes.append(([], st))
            by_key[key] = sig_class[sig]
        classes[by_key[key]][0].append(i)
    return classes


def _resolve_abstol(abstol, st):
    """_resolve_abstol (sweeps.jl:626): per-class NamedTuple -> vector via state_abstol."""
    if isinstance(abstol, dict):
        return st.state_abstol(**abstol)
    return np.broadcast_to(np.asarray(abstol, dtype=float), (st.n,)).copy()


def dc(target, u0=None, device=0, continuation=True):
    """dc!(circuit) / dc!(cs::CircuitSweep; continuation=true) -- sweeps.jl:450-455, 489-532.  Goes through
    with_mode(:dcop), which keeps only temp+mode of the spec (solve.jl:1976-1989).  A sweep is partitioned by structure
    (``structure_classes``); each class is one resident batch, solved with the staged continuation (``continuation=True``), with the
    reference's strictly serial chain point i - 1 -> point i (``continuation="serial"``: the choice for circuits with several DC
    solutions, whose branch a sweep is meant to follow -- see ``BatchSimulator.dc_continuation``), or as independent cold solves
    (``continuation=False``)."""
    if isinstance(target, CircuitSweep):
        mc = target.circuit
        mc = MNACircuit(mc.circuit, mc.params, MNASpec(temp=mc.spec.temp, mode="dcop"))
        pts = target.points()
        sols = [None] * len(pts)
        for idx, st in structure_classes(mc, pts):
            sim = BatchSimulator(mc, [pts[i] for i in idx], device, st=st)
            try:
                u, conv, _ = sim.dc_continuation(serial=continuation == "serial") if continuation else sim.dc()
                ops = sim.operating_points(u)
                for k, i in enumerate(idx):
                    sols[i] = DCSolution(sim.st, u[k], conv[k], ops[k])
            finally:
                sim.close()
        return SweepResult(pts, sols)
    mc = MNACircuit(target.circuit, target.params, MNASpec(temp=target.spec.temp, mode="dcop"))
    sim = BatchSimulator(mc, None, device)
    try:
        u, conv, _ = sim.dc(u0=u0)
        return DCSolution(sim.st, u[0], conv[0], sim.operating_points(u)[0])
    finally:
        sim.close()


class ACSol:
    """ac!'s result (src/ac.jl:75-82): the system linearised at the DC point -- G (with gmin on the voltage-node diagonals), C, the
    excitation b_ac -- plus the DC solution and the frequency grid in hertz.  ``sol[name]`` is the complex response of a node
    voltage or a branch current over the grid (ac.jl name-based access); ``freqresp(name, omegas)`` evaluates at angular
    frequencies (ac.jl:185-215); ``magnitude_db`` / ``phase_deg`` as in ac.jl:228-273."""

    def __init__(self, st, G, C, b_ac, dc_x, freqs, delay=None):
        self.st, self.G, self.C, self.b_ac, self.dc_x, self.freqs = st, G, C, b_ac, dc_x, np.asarray(freqs, dtype=float)
        self.delay = delay       # None, or omega -> the n x n addend of the circuit's delayed elements (AcDelayOverlay.of): A = G + j w C + delay(w)
        self._cache = {}
        self.stats = {}          # ac(..., solver="gpu" | "auto"): what the batched GPU sweep did (``ac_gpu_sweep``); empty on the host path

    def _solve(self, omegas):
        key = tuple(np.asarray(omegas, dtype=float))
        if key not in self._cache:
            self._cache[key] = np.array([np.linalg.solve(ac_matrix(self.G, self.C, w, self.delay), self.b_ac) for w in key]) if len(key) else np.zeros((0, self.st.n), complex)
        return self._cache[key]

    def freqresp(self, name, omegas):
        return self._solve(omegas)[:, self.st.index_of(name)]

    def __getitem__(self, name):
        return self.freqresp(name, 2.0 * np.pi * self.freqs)

    def magnitude_db(self, name, freqs=None):
        r = self[name] if freqs is None else self.freqresp(name, 2.0 * np.pi * np.asarray(freqs, dtype=float))
        return 20.0 * np.log10(np.abs(r))

    def phase_deg(self, name, freqs=None):
        r = self[name] if freqs is None else self.freqresp(name, 2.0 * np.pi * np.asarray(freqs, dtype=float))
        return np.degrees(np.angle(r))


def acdec(points_per_decade, fstart, fstop):
    """SPICE ``.ac dec``: logarithmic grid with ``points_per_decade`` points per decade from fstart to fstop (hertz)."""
    n = int(np.floor(np.log10(fstop / fstart) * points_per_decade + 1e-9)) + 1
    return fstart * 10.0 ** (np.arange(n) / points_per_decade)


def rhs_ac(st, circuit, params):
    """get_rhs_ac (build.jl:169-190): V sources stamp their ``ac`` value on their branch row (devices.jl:659), I sources +ac into p
    and -ac into n (devices.jl:728-729)."""
    from .circuit import resolve
    b = np.zeros(st.n, dtype=complex)
    for d in circuit.devices:
        if d.type not in ("V", "I"):
            continue
        ac = complex(resolve(d.params.get("ac", 0.0), params))
        if ac == 0:
            continue
        if d.type == "V":
            b[st.index_of("I_" + d.name)] += ac
        else:
            for nm, sgn in ((d.nodes[0], 1.0), (d.nodes[1], -1.0)):
                if nm not in ("0", "gnd", "gnd!"):
                    b[st.index_of(nm)] += sgn * ac
    return b


# A GPU system is accepted when its componentwise backward error is at most AC_BERR_MAX; otherwise (or when its flag is set) the host's dense
# solve replaces it.  Measured, not chosen: 16 x the largest backward error np.linalg.solve -- the reference path -- itself leaves over the
# systems of the AC test circuits (tests/ac_ref.py CASES, on the CPU port's G, C at the DC points), and not below 64 eps.  16 is what this
# project grants another summation order (tests/test_gpu_lu_kernels.py).  The measurement gave 1.0: the unrefined dense solve is normwise
# stable (6e-17 on every system) but leaves rows of the flip-flop whose terms are all of order 1e-19 -- switched-off transistors at 1 kHz --
# with a residual as large as the terms themselves.  At 16 the gate therefore only rejects non-finite or grossly wrong rows (singular
# pivots are caught by the flag); the kernel's own rows measure 2e-16.  DESIGN.md section 6.
AC_BERR_MAX = max(16 * 1.0, 64 * float(np.finfo(np.float64).eps))


def ac_pivot_sample(st, G_csr, C_csr, omegas, gmin):
    """The sample the GPU sweep's pivot order is analysed on ([nnz], the structure's CSR order): element-wise maximum over the instances
    ([B, nnz]) of |G| + w_g |C| with gmin on the voltage-node diagonals, w_g the geometric mean of the non-zero grid frequencies."""
    w = np.asarray(omegas, dtype=float)
    w = w[w > 0]
    wg = float(np.exp(np.mean(np.log(w)))) if w.size else 0.0
    s = np.max(np.abs(np.atleast_2d(G_csr)) + wg * np.abs(np.atleast_2d(C_csr)), axis=0)
    d = np.asarray(st.diag_nz)[:st.n_nodes]
    s[d[d >= 0]] += gmin
    return s


# ---- delayed controlled sources (Circuit.E/G/H/F(..., delay=), Circuit.T) in the frequency domain ------------------------------------------
# The stamps of a controlled source that carry its gain: type -> (parameter, {G slot of structure.PROGRAMS: d stamp / d parameter}), from
# csrc/devices.hpp (stamp_vcvs, stamp_vccs, stamp_ccvs, stamp_cccs).  A delay tau multiplies exactly these by e^{-j w tau}.
DELAY_STAMPS = {"E": ("gain", {4: -1.0, 5: 1.0}), "G": ("gm", {0: -1.0, 1: 1.0, 2: 1.0, 3: -1.0}), "H": ("rm", {8: -1.0}), "F": ("gain", {4: -1.0, 5: 1.0})}


def has_delay(circuit):
    """does the circuit hold a delayed controlled source (a transmission line is made of them)?"""
    return any("delay" in d.params for d in circuit.devices)


def refuse_delay(circuit, what, why):
    """the analyses that cannot take a delayed element say so before any device work"""
    if has_delay(circuit):
        raise NotImplementedError("%s: the circuit has a delayed controlled source or a transmission line; %s" % (what, why))


class AcDelayOverlay:
    """What the delayed elements of a circuit add to A(w) = G + j w C at a batch of points: D[b](w), non-zero at the CSR positions ``pos`` [O]
    (ascending; ``rows`` / ``cols`` their coordinates), D[b](w)[pos[o]] = sum over the delayed stamps t at that position of
    (e^{-j w tau_t[b]} - 1) w_t[b], with w_t the stamp's own contribution to G.  ``val`` [B, F, O] is the table on the grid ``omegas`` the
    overlay was made for -- what hip.Handle.ac_set_overlay takes; ``values(omegas)`` evaluates it on any grid, ``dense(b, omega)`` gives the
    n x n addend of point b at one frequency, and ``of(b)`` that as a function of omega alone."""

    def __init__(self, n, pos, rows, cols, terms, B, omegas):
        self.n, self.pos, self.rows, self.cols, self.terms, self.B = n, pos, rows, cols, terms, B
        self.omegas = np.asarray(omegas, dtype=float).ravel()
        self.val = self.values(self.omegas)

    def values(self, omegas):
        w = np.asarray(omegas, dtype=float).ravel()
        val = np.zeros((self.B, w.size, len(self.pos)), dtype=complex)
        for o, tau, wt in self.terms:
            x = w[None, :] * tau[:, None]
            val[:, :, o] += (-2.0 * np.sin(0.5 * x) ** 2 - 1j * np.sin(x)) * wt[:, None]      # e^{-jx} - 1 without the cancellation at small x
        return val

    def dense(self, b, omega):
        D = np.zeros((self.n, self.n), dtype=complex)
        D[self.rows, self.cols] = self.values([omega])[b, 0]
        return D

    def of(self, b):
        return lambda omega: self.dense(b, omega)


def ac_delay_overlay(st, circuit, params, omegas=(), B=None):
    """The one place that turns delayed elements into numbers -- pure host code, shared by the dense host solves, the redo rows of the GPU
    gates and the GPU sweeps (which hand ``pos`` / ``val`` to the overlay kernels): circuit, structure and point parameters (name -> a
    number or one value per point; ``B``: the number of points when no parameter tells) in, an AcDelayOverlay out, or None for a circuit without a delayed element.  The table is computed here,
    not on the device: it is B x F x a handful of entries, needs sin / cos of arguments that must agree with the host path's to the bit, and
    the kernels stay ignorant of what produced it."""
    from .circuit import resolve
    from .opinfo import _index
    if not has_delay(circuit):
        return None
    B = int(B) if B is not None else max([np.size(v) for v in params.values()] + [1])
    info = {d["name"]: d for d in st.opinfo}
    at, terms = {}, []
    for d in circuit.devices:
        if "delay" not in d.params:
            continue
        if d.type not in DELAY_STAMPS:
            raise NotImplementedError("a delay on a %s element" % d.type)
        par, slots = DELAY_STAMPS[d.type]
        oi = info[d.name]
        gl = [_index(st, t) for t in oi["nodes"]]
        tau = np.broadcast_to(np.asarray(resolve(d.params["delay"], params), dtype=float), (B,))
        gain = np.broadcast_to(np.asarray(resolve(d.params[par], params), dtype=float), (B,))
        for stream, k, rl, cl in oi["prog"]:
            if stream != "G" or k not in slots or gl[rl] < 0 or gl[cl] < 0:
                continue
            terms.append(((gl[rl], gl[cl]), tau, slots[k] * gain))
            at.setdefault((gl[rl], gl[cl]), None)
    rowptr, colidx = np.asarray(st.rowptr), np.asarray(st.colidx)
    csr = lambda r, c: int(rowptr[r] + np.flatnonzero(colidx[rowptr[r]:rowptr[r + 1]] == c)[0])
    coords = sorted(at, key=lambda rc: csr(*rc))
    o_of = {rc: o for o, rc in enumerate(coords)}
    return AcDelayOverlay(st.n, np.array([csr(*rc) for rc in coords], dtype=np.int32), np.array([rc[0] for rc in coords], dtype=np.int64),
                          np.array([rc[1] for rc in coords], dtype=np.int64), [(o_of[rc], tau, wt) for rc, tau, wt in terms], B, omegas)


def ac_matrix(G, C, omega, delay=None):
    """A(w) of the dense host solves: G + j w C, plus the delayed elements' addend when there is one (``delay``: omega -> n x n)"""
    A = G + 1j * omega * C
    return A if delay is None else A + delay(omega)


class _ac_overlay_of:
    """the handle's overlay for one sweep, as a ``with`` block (``_ac_gated_launch``); None makes no call at all"""

    def __init__(self, h, ovl):
        self.h, self.ovl = h, ovl

    def __enter__(self):
        if self.ovl is not None:
            self.h.ac_set_overlay(self.ovl.pos, self.ovl.omegas, self.ovl.val)

    def __exit__(self, *exc):
        if self.ovl is not None:
            self.h.ac_clear_overlay()


def _overlay_sample(sample_csr, ovl):
    """the pivot sample of a sweep under an overlay: max_f |D| joins the sample at the overlay's positions"""
    if ovl is not None and ovl.val.size:
        sample_csr = np.array(sample_csr)
        sample_csr[ovl.pos] += np.max(np.abs(ovl.val), axis=(0, 1))
    return sample_csr


AC_MEMORIES = ("lds", "hbm", "auto")


def _ac_memory(memory):
    if memory not in AC_MEMORIES:
        raise ValueError("memory must be 'lds', 'hbm' or 'auto'")
    return memory


def _ac_solver(solver):
    if solver not in ("host", "gpu", "auto"):
        raise ValueError("solver must be 'host', 'gpu' or 'auto'")
    return solver


def _ac_stats(**more):
    """what the GPU sweeps of one call count into (``_ac_gated_launch``), plus the analysis' own keys"""
    return dict({"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}, **more)


class _ac_memory_of:
    """the handle's AC memory setting for one sweep, as a ``with`` block (``_ac_gated_launch``).  "lds" -- the default -- makes no call of its
    own: the sweep is call for call what it was, under the setting of a new handle; "hbm" / "auto" are set for the block and LDS restored after it."""

    def __init__(self, h, memory):
        self.h, self.memory = h, memory

    def __enter__(self):
        if self.memory != "lds":
            self.h.ac_set_memory(self.memory)

    def __exit__(self, *exc):
        if self.memory != "lds":
            self.h.ac_set_memory("lds")


def ac_analyze_pivots(h, st, G_ref, C_ref, omegas, gmin, overlay=None):
    """Re-analyse the handle's pivot order for a small-signal sweep: ``ac_pivot_sample`` of the class (``G_ref`` / ``C_ref`` [B, nnz]: the
    handle's get_GCb) on the grid, joined by the overlay's max_f |D|, handed to ``analyze_values`` in the reference order it takes."""
    to_ref = np.asarray(st.to_ref_nz)
    sample_ref = np.empty(st.nnz)
    sample_ref[to_ref] = _overlay_sample(ac_pivot_sample(st, np.asarray(G_ref)[:, to_ref], np.asarray(C_ref)[:, to_ref], omegas, gmin), overlay)
    h.analyze_values(sample_ref)


def _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, overlay, call, rejected, n_systems, fallback="host solve"):
    """The one way a small-signal sweep reaches the GPU, and the one gate its results pass: the pivot order is re-analysed
    (``ac_analyze_pivots``), then ``call(h)`` makes the ONE kernel call -- a Handle method whose tuple ends in (berr, flags, info) -- under the
    memory setting and the overlay of the sweep, and ``rejected(berr, flags)`` gives the boolean mask of the systems the caller must solve
    again on the host.  ``stats`` is updated: gpu_systems / host_systems by the mask, max_berr over the accepted systems, wpb, and memory --
    what the launch used.  Returns (what ``call`` returned, the mask).  A circuit the memory setting refuses (CADNIP_BADARG) raises with
    solver="gpu"; with "auto" ``n_systems`` are counted as host systems, stats["fallback"] says why and None is returned."""
    from . import hip
    ac_analyze_pivots(h, st, G_ref, C_ref, omegas, gmin, overlay)
    try:
        with _ac_memory_of(h, memory), _ac_overlay_of(h, overlay):
            got = call(h)
            used = h.ac_plan_info()["memory"] if memory != "lds" else "lds"
    except hip.CadnipError as e:
        if solver == "auto" and e.code == hip.BADARG:
            stats["host_systems"] += n_systems
            stats["fallback"] = "the circuit's work arrays exceed the AC kernel's LDS budget: " + fallback
            return None
        raise
    berr, flags, info = got[-3:]
    redo = rejected(berr, flags)
    kept = berr[~redo]
    stats["gpu_systems"] += int((~redo).sum())
    stats["host_systems"] += int(redo.sum())
    stats["max_berr"] = max(stats["max_berr"], float(kept.max()) if kept.size else 0.0)
    stats["wpb"] = info["wpb"]
    stats["memory"] = used
    return got, redo


def probe_differences(x, pairs):
    """x[p] - x[n] along the first axis of ``x`` for the (p, n) rows of ``pairs``, -1 = ground"""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    at = lambda j: np.where((j >= 0).reshape((-1,) + (1,) * (np.ndim(x) - 1)), x[j], 0.0)
    return at(pr[:, 0]) - at(pr[:, 1])


def pair_column(n, pair):
    """the column e_p - e_n of an output pair of unknown indices (-1 = ground)"""
    e = np.zeros(n, dtype=complex)
    for j, sgn in zip(pair, (1.0, -1.0)):
        if j >= 0:
            e[j] += sgn
    return e


def dense_of_ref(st, nz, gmin=None):
    """one instance's values in reference order (a row of get_GCb) as a dense n x n matrix; ``gmin`` joins the voltage-node diagonals"""
    import scipy.sparse as sp
    A = sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
    if gmin is not None:
        A[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
    return A


def ac_gpu_sweep(h, st, sols, G_ref, C_ref, omegas, gmin, solver, stats, memory="lds", overlay=None):
    """The frequency sweep of one structure class on the GPU: ``h`` (a hip.Handle holding the restamp at the DC points) re-analyses its
    pivot order on ``ac_pivot_sample`` and solves all points x all frequencies in ONE ``ac_solve`` call; every ACSol of ``sols`` gets the
    rows of its point into its cache under the key ``tuple(omegas)``.  A system whose flag is set or whose backward error exceeds
    AC_BERR_MAX is solved again by the host's dense solve, which replaces the GPU row.  ``stats`` (shared by the call) is updated:
    gpu_systems / host_systems, max_berr over the accepted GPU rows, wpb (``_ac_gated_launch``).  A circuit that does not fit the launch plan raises with
    solver="gpu"; with "auto" nothing is cached -- the sols solve on the host on demand -- and stats["fallback"] says why.
    ``memory``: where the kernel keeps a system's work arrays (hip.Handle.ac_set_memory) -- "lds" (the default; DESIGN section 9 has
    the figures and leaves another default to a later change): circuits beyond the LDS budget are refused as above; "hbm": a workspace in device memory, so
    such a circuit is solved on the GPU; "auto": LDS where the circuit fits, else HBM.  stats["memory"] is what the launch used.
    ``overlay``: the AcDelayOverlay of the class on ``omegas`` (the sols then carry its ``of(k)`` as their ``delay``), or None: it is set on
    the handle for the call and cleared after it, and its max_f |D| joins the pivot sample."""
    _ac_memory(memory)
    omegas = np.asarray(omegas, dtype=float)
    B, F = len(sols), omegas.size
    key = tuple(omegas)
    if F == 0:
        for s in sols:
            s._cache[key] = np.zeros((0, st.n), complex)
        return
    got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, overlay,
                           lambda h: h.ac_solve(omegas, gmin, np.array([s.b_ac for s in sols])),
                           lambda berr, flags: (flags != 0) | ~(berr <= AC_BERR_MAX), B * F)
    if got is None:
        return
    (x, _, _, _), redo = got
    for k, s in enumerate(sols):
        rows = np.array(x[k])
        for f in np.flatnonzero(redo[k]):
            rows[f] = np.linalg.solve(ac_matrix(s.G, s.C, omegas[f], s.delay), s.b_ac)
        s._cache[key] = rows


def _ac_target(target):
    """(sweep?, the circuit in dcop mode, the sweep points) of an AC-family call"""
    sweep = isinstance(target, CircuitSweep)
    mc0 = target.circuit if sweep else target
    mc = MNACircuit(mc0.circuit, mc0.params, MNASpec(temp=mc0.spec.temp, mode="dcop", gmin=mc0.spec.gmin))
    return sweep, mc, target.points() if sweep else [{}]


def _ac_classes(sweep, mc, pts, gmin, device, what):
    """The linearisation ``ac``, ``network``, ``noise``, ``network_noise`` and ``pz`` share, one structure class at a time: a resident batch per class, its DC operating points, the
    restamp at them, and per point the dense G (``gmin`` on the voltage-node diagonals) and C.  Yields (sim, st, idx, G, C, lin) with G / C the
    handle's get_GCb ([B, nnz]) and lin = [(point index, G dense, C dense, point parameters, DC solution)]; the batch is closed when the
    consumer moves on -- or closes the generator."""
    for idx, st in structure_classes(mc, pts) if sweep else [(list(range(1)), None)]:
        sim = BatchSimulator(mc, [pts[i] for i in idx] if sweep else None, device, st=st)
        try:
            st = sim.st
            u, conv, _ = sim.dc()
            if not np.all(conv):
                raise RuntimeError("%s: the DC operating point did not converge for %d point(s)" % (what, int((~conv).sum())))
            sim.h.rebuild(u, 0.0)
            G, C, _, _ = sim.h.get_GCb()
            yield sim, st, idx, G, C, [(i, dense_of_ref(st, G[k], gmin), dense_of_ref(st, C[k]), {kk: float(v[k]) for kk, v in sim.params.items()}, u[k].copy())
                                       for k, i in enumerate(idx)]
        finally:
            sim.close()


def source_rhs(st, circuit, name):
    """The excitation of ONE independent source at unit magnitude, whatever its ``ac`` value: a V source's branch row gets 1, an I source puts
    +1 into p and -1 into n (as ``rhs_ac``).  The name is matched as ``noise(..., input=)`` matches it (as written, then in lower case)."""
    d = next((d for d in circuit.devices if d.type in ("V", "I") and d.name == name), None) or \
        next((d for d in circuit.devices if d.type in ("V", "I") and d.name.lower() == name.lower()), None)
    if d is None:
        raise ValueError("%s is not an independent source of the circuit" % name)
    b = np.zeros(st.n, dtype=complex)
    if d.type == "V":
        b[port_rows(st, [d.name])[0]] = 1.0
    else:
        for nm, sgn in ((d.nodes[0], 1.0), (d.nodes[1], -1.0)):
            if nm not in ("0", "gnd", "gnd!"):
                b[st.index_of(nm)] += sgn
    return b


def port_rows(st, ports):
    """The branch rows I_<V> of the voltage sources named in ``ports``, resolved as ``noise_indices`` resolves ``input``; ValueError for a name
    that is not an independent voltage source."""
    rows = []
    for nm in ports:
        cand = [c for c in ("I_" + nm, "I_" + nm.lower()) if c in st.current_names]
        if not cand:
            raise ValueError("network: port %s is not an independent voltage source (no current variable I_%s)" % (nm, nm))
        rows.append(st.n_nodes + st.current_names.index(cand[0]))
    if len(set(rows)) != len(rows):
        raise ValueError("network: a port is named twice")
    return rows


def ac_multi_gpu_sweep(h, st, Gd, Cd, G_ref, C_ref, omegas, gmin, rhs, pairs, want_x, solver, stats, memory="lds", overlay=None):
    """K excitations per point against ONE factorisation per (point, frequency), on the GPU: ``h`` (holding the restamp at the DC points)
    re-analyses its pivot order on ``ac_pivot_sample`` -- as ``ac_gpu_sweep`` -- and solves points x frequencies x the K columns of ``rhs``
    ([K, n]) in ONE ``ac_solve_multi`` call.  Returns (h [B, F, K, P] for the probe ``pairs`` or None, x [B, F, K, n] or None without
    ``want_x``).  The gate is ``ac_gpu_sweep``'s, per column: a column whose flag is set or whose backward error exceeds AC_BERR_MAX is solved
    again by the host's dense solve on ``Gd`` / ``Cd`` (per point; gmin on the node diagonals).  ``stats`` counts columns as systems.  A
    circuit the memory home refuses raises with solver="gpu"; with "auto" None is returned and stats["fallback"] says why.  ``overlay`` as
    for ``ac_gpu_sweep``: the redo solves add its ``dense(b, w)``."""
    _ac_memory(memory)
    omegas = np.asarray(omegas, dtype=float)
    rhs = np.asarray(rhs, dtype=complex)
    B, F, K = len(Gd), omegas.size, rhs.shape[0]
    stats["rhs"] = K
    got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, overlay,
                           lambda h: h.ac_solve_multi(omegas, gmin, rhs, pairs, 0, want_x),
                           lambda berr, flags: (flags != 0) | ~(berr <= AC_BERR_MAX), B * F * K)
    if got is None:
        return None
    (hh, x, _, _, _), redo = got
    for b, f, k in zip(*np.nonzero(redo)):
        xh = np.linalg.solve(ac_matrix(Gd[b], Cd[b], omegas[f], overlay and overlay.of(b)), rhs[k])
        if x is not None:
            x[b, f, k] = xh
        if hh is not None:
            hh[b, f, k] = probe_differences(xh, pairs)
    return hh, x


def ac(target, freqs=(), gmin=1e-12, device=0, solver="host", memory="lds", sources=None):
    """ac!(circuit, freqs; gmin) -- src/ac.jl:113-170.  The DC operating point and the restamp at it run on the GPU (cadnip_dc_run,
    cadnip_rebuild: the linearisation IS the stamping); G gets ``gmin`` on the voltage-node diagonals (assemble_G(ctx; gshunt=gmin),
    ac.jl:127).  The frequency sweep is the reference's own dense ``(jw C + G)^-1 b_ac`` on the host: n is a circuit's size, not a
    batch dimension.  A CircuitSweep returns one ACSol per point (one resident batch per structure class).
    ``solver``: "host" (default) as above; "gpu" solves the grid of every point on the device as well -- points x frequencies complex
    sparse systems in one batched kernel per structure class (``ac_gpu_sweep``) -- and fills the ACSols' caches for the grid, so ``sol[name]``,
    ``magnitude_db`` and ``phase_deg`` read GPU results while ``freqresp`` at other frequencies still solves on the host; ``sol.stats`` =
    {"gpu_systems", "host_systems", "max_berr", "wpb", "memory"} of the call.  "gpu" raises for a circuit too large for the kernel, "auto"
    takes the host path for it and says so in ``stats``.
    ``memory`` (ignored with solver="host"): "lds" (default) keeps a system's work arrays in LDS -- "too large" is then 160 KB; "hbm" keeps
    them in device memory and "auto" does so where LDS refuses, so such a circuit is solved on the GPU (``ac_gpu_sweep``).  The default
    stays "lds": DESIGN section 9 has the measured figures and leaves making "auto" the default to a later change.
    ``sources`` (default None: the call is exactly what it is without the keyword): a list of names of independent sources.  The result is
    then, per point, a dict name -> ACSol whose excitation is that source ALONE at unit magnitude (``source_rhs``; the circuit's ``ac=``
    values are ignored): the separate responses from one DC solve and one restamp, and with a GPU solver from one factorisation per (point,
    frequency) serving all of them (``ac_multi_gpu_sweep``; ``stats`` then counts columns as systems and has "rhs": the number of sources).
    A circuit with delayed controlled sources or transmission lines (``Circuit.E/G/H/F(..., delay=)``, ``Circuit.T``) is solved as
    A(w) = G + j w C + D(w) on every path -- ``ac_delay_overlay`` computes D, the host solves add it, the GPU sweeps hand it to the overlay
    kernels -- and so are ``network``, ``noise`` and ``network_noise``; the ACSols then carry ``delay``."""
    from contextlib import closing
    _ac_solver(solver), _ac_memory(memory)
    stats = _ac_stats()
    sweep, mc, pts = _ac_target(target)
    sols = [None] * len(pts)
    omegas = 2.0 * np.pi * np.asarray(freqs, dtype=float)
    with closing(_ac_classes(sweep, mc, pts, gmin, device, "ac")) as classes:
        for sim, st, idx, G, C, lin in classes:
            ovl = ac_delay_overlay(st, mc.circuit, sim.params, omegas, sim.B)
            if sources is None:
                for k, (i, Gd, Cd, p_i, u_i) in enumerate(lin):
                    sols[i] = ACSol(st, Gd, Cd, rhs_ac(st, mc.circuit, p_i), u_i, freqs, ovl and ovl.of(k))
                if solver != "host":
                    ac_gpu_sweep(sim.h, st, [sols[i] for i in idx], G, C, omegas, gmin, solver, stats, memory, ovl)
                continue
            rhs = np.array([source_rhs(st, mc.circuit, nm) for nm in sources]).reshape(len(sources), st.n)
            for k, (i, Gd, Cd, p_i, u_i) in enumerate(lin):
                sols[i] = {nm: ACSol(st, Gd, Cd, rhs[j], u_i, freqs, ovl and ovl.of(k)) for j, nm in enumerate(sources)}
            if solver != "host" and omegas.size and len(sources):
                got = ac_multi_gpu_sweep(sim.h, st, [l[1] for l in lin], [l[2] for l in lin], G, C, omegas, gmin, rhs, None, True, solver, stats, memory, ovl)
                if got is not None:
                    for k, i in enumerate(idx):
                        for j, nm in enumerate(sources):
                            sols[i][nm]._cache[tuple(omegas)] = np.array(got[1][k, :, j])
    if solver != "host":
        for s in sols:
            for a in (s.values() if isinstance(s, dict) else [s]):
                a.stats = stats
    return SweepResult(pts, sols) if sweep else sols[0]


class NetworkSol:
    """``network``'s result: the N-port admittance matrix of a circuit linearised at its DC point, over a grid in hertz.  ``y`` [F, P, P]
    complex with y[f, i, j] the current INTO port i per volt at port j, the other ports shorted; ``z`` = inv(y) per frequency (a singular y
    raises numpy's LinAlgError -- from ``z`` only); ``s`` the scattering matrix for the reference impedances ``z0`` (a scalar, or one real
    value per port): (I - z0 y)(I + z0 y)^-1, and with unequal impedances the power-wave form F (I - Z0 y)(I + Z0 y)^-1 F^-1 with
    Z0 = diag(z0), F = diag(1 / (2 sqrt(z0_i))).  ``s_db(i, j)`` is 20 log10 |s[:, i, j]| (ports by index or by name).  ``dc_x`` is the DC
    solution, ``stats`` what a GPU solver did (as ``ACSol.stats``, columns counted as systems, plus "rhs")."""

    def __init__(self, freqs, ports, y, z0=50.0, dc_x=None):
        self.freqs, self.ports, self.dc_x = np.asarray(freqs, dtype=float), list(ports), dc_x
        P = len(self.ports)
        self.y = np.ascontiguousarray(np.asarray(y, dtype=complex).reshape(len(self.freqs), P, P))
        z = np.asarray(z0, dtype=float)
        if z.ndim > 1 or (z.ndim == 1 and z.size != P) or not np.all(z > 0):
            raise ValueError("z0 must be a positive scalar or one positive value per port")
        self.z0 = float(z) if z.ndim == 0 else z.copy()
        self.stats = {}

    @property
    def z(self):
        return np.linalg.inv(self.y)

    @property
    def s(self):
        P = len(self.ports)
        z0 = np.broadcast_to(np.asarray(self.z0, dtype=float), (P,))
        eye, zy = np.eye(P), z0[:, None] * self.y                    # Z0 y
        s = (eye - zy) @ np.linalg.inv(eye + zy)
        f = 1.0 / (2.0 * np.sqrt(z0))
        return s if np.all(z0 == z0[0]) else (f[:, None] * s) / f[None, :]

    def _port(self, i):
        return self.ports.index(i) if isinstance(i, str) else int(i)

    def s_db(self, i, j):
        return 20.0 * np.log10(np.abs(self.s[:, self._port(i), self._port(j)]))


def network_solve(st, G, C, ports, freqs, z0=50.0, dc_x=None, delay=None):
    """The host path of ``network`` on dense G (gmin already on the voltage-node diagonals) and C: per frequency ONE dense LU serves the P
    columns -- column j has 1 on the branch row of port j's source and 0 elsewhere -- and y[f, i, j] = -x_j[I_<Vi>]: a V source's branch
    current flows from + through the source to -, so the current into the port from outside is its negative."""
    freqs = np.asarray(freqs, dtype=float)
    rows = port_rows(st, ports)
    E = np.zeros((st.n, len(rows)), dtype=complex)
    E[rows, np.arange(len(rows))] = 1.0
    y = np.zeros((len(freqs), len(rows), len(rows)), dtype=complex)
    for fi, f in enumerate(freqs):
        y[fi] = -np.linalg.solve(ac_matrix(G, C, 2.0 * np.pi * f, delay), E)[rows]
    return NetworkSol(freqs, ports, y, z0, dc_x)


def network(target, ports, freqs, z0=50.0, gmin=1e-12, device=0, solver="host", memory="lds"):
    """The N-port small-signal parameters of a circuit (SPICE's .net / .sp): ``ports`` names P independent voltage sources, port i is its
    source's (+, -) node pair.  The circuit is linearised at its DC point exactly as by ``ac`` (the same code); column j of the admittance
    matrix is the response to 1 V on port j's source with every other port AC-shorted by its own source -- the ``ac=`` values of the circuit
    are ignored.  Returns a NetworkSol (``y``, ``z``, ``s``, ``s_db``), or for a CircuitSweep a SweepResult of them.  A port that is not an
    independent voltage source raises ValueError.
    ``solver``: "host" (default) -- dense solves, one LU per frequency serving all P columns (``network_solve``); "gpu" -- one
    ``ac_solve_multi`` call per structure class: each (point, frequency) system is factored once on the device for its P columns, and only
    the P x P port currents per system come back (``ac_multi_gpu_sweep``: the gate of ``ac_gpu_sweep`` per column, a rejected column is solved
    again on the host); "auto" -- as "gpu", with the host path for a circuit the memory home refuses.  ``memory`` as for ``ac``.
    ``stats`` = {"gpu_systems", "host_systems", "max_berr", "wpb", "memory", "rhs"} with columns counted as systems."""
    from contextlib import closing
    _ac_solver(solver), _ac_memory(memory)
    ports = list(ports)
    freqs = np.asarray(freqs, dtype=float)
    omegas = 2.0 * np.pi * freqs
    stats = _ac_stats()
    sweep, mc, pts = _ac_target(target)
    sols = [None] * len(pts)
    with closing(_ac_classes(sweep, mc, pts, gmin, device, "network")) as classes:
        for sim, st, idx, G, C, lin in classes:
            rows = port_rows(st, ports)
            ovl = ac_delay_overlay(st, mc.circuit, sim.params, omegas, sim.B)
            got = None
            if solver != "host" and freqs.size and rows:
                rhs = np.zeros((len(rows), st.n), dtype=complex)
                rhs[np.arange(len(rows)), rows] = 1.0
                got = ac_multi_gpu_sweep(sim.h, st, [l[1] for l in lin], [l[2] for l in lin], G, C, omegas, gmin, rhs, [(r, -1) for r in rows], False,
                                         solver, stats, memory, ovl)
            for k, (i, Gd, Cd, p_i, u_i) in enumerate(lin):
                if got is None:
                    sols[i] = network_solve(st, Gd, Cd, ports, freqs, z0, u_i, ovl and ovl.of(k))
                else:
                    sols[i] = NetworkSol(freqs, ports, -np.swapaxes(got[0][k], 1, 2), z0, u_i)      # h[f, column j, port i] -> y[f, i, j]
    if solver != "host":
        for s in sols:
            s.stats = stats
    return SweepResult(pts, sols) if sweep else sols[0]


# ---- noise! (src/noise.jl) ---------------------------------------------------------------------------------------------------------------
K_BOLTZMANN, Q_ELEMENTARY = 1.380649e-23, 1.602176634e-19


class NoiseSol:
    """noise!'s result (src/noise.jl:31-40): output-referred noise PSD over a grid in hertz, per-source contributions (device names in lower
    case), and -- when an input source was named -- the input -> output gain and the input-referred PSD.  ``ns["onoise"]``, ``ns["inoise"]``,
    ``ns[source]`` as in noise.jl:239-253."""

    def __init__(self, freqs, output, onoise, contributions, temp, input, gain, inoise):
        self.freqs, self.output, self.onoise, self.contributions = freqs, output, onoise, contributions
        self.temp, self.input, self.gain, self.inoise = temp, input, gain, inoise
        self.stats = {}          # noise(..., solver="gpu" | "auto"): what the batched GPU sweep did (``noise_solve_gpu``); empty on the host path

    def __getitem__(self, name):
        if name == "onoise":
            return self.onoise
        if name == "inoise":
            if self.input is None:
                raise KeyError("NoiseSol: no input-referred noise -- call noise(circuit, output, freqs, input=...)")
            return self.inoise
        if name in self.contributions:
            return self.contributions[name]
        raise KeyError("NoiseSol: unknown key %r (have onoise, inoise and the sources %s)" % (name, sorted(self.contributions)))


def total_noise(ns, referred="output"):
    """band-integrated RMS noise sqrt(int S df) by the trapezoidal rule (noise.jl:258-276)"""
    if referred not in ("output", "input"):
        raise ValueError("total_noise: referred must be 'output' or 'input', got %r" % (referred,))
    psd = ns["onoise"] if referred == "output" else ns["inoise"]
    fs = ns.freqs
    if len(fs) < 2:
        return float(np.sqrt(psd[0] if len(fs) == 1 else 0.0))
    return float(np.sqrt(np.sum(0.5 * (psd[:-1] + psd[1:]) * np.diff(fs))))


def noise_psd(src, temp_c, f):
    """one-sided PSD of a registered source (context.jl:179-189): thermal 4kT a, shot 2q a, white a, flicker a / f^b"""
    kind, a, b = src[2], src[3], src[4]
    if kind == "thermal":
        return 4.0 * K_BOLTZMANN * (float(temp_c) + 273.15) * a
    if kind == "shot":
        return 2.0 * Q_ELEMENTARY * a
    if kind == "white":
        return a
    return a / float(f) ** b


def noise_sources(st, circuit, params, u, temp_c=27.0, gmin=1e-12):
    """The noise sources of ``circuit`` at the solution ``u`` (one instance, [n]): (p, n, kind, a, b, name) with global unknown indices
    (-1 = ground).  What the reference's devices register while the builder runs at the DC point (context.jl:1017-1127): resistors their
    thermal noise 4kT/R (devices.jl:498-503), diodes the shot noise of their junction current and, with KF > 0, its flicker noise
    (devices.jl:1393-1443, 1582-1585), SimpleMOSFETs their channel thermal and flicker noise (devices.jl:1718-1732), instances of
    Verilog-A modules one source per white_noise / flicker_noise call of the contributions they execute (vasim.jl:2856-2893; evaluated by
    va/host_eval.py at the node voltages of ``u``: needs the model source)."""
    from .circuit import resolve
    from .opinfo import _index
    from . import va
    num = lambda v: float(np.asarray(resolve(v, params)).flat[0])
    out = []
    info = {d["name"]: d for d in st.opinfo}
    for d in circuit.devices:
        gl = [_index(st, t) for t in info[d.name]["nodes"]]
        name = d.name.lower()
        if d.type == "R":
            out.append((gl[0], gl[1], "thermal", 1.0 / num(d.params["r"]), 0.0, name))
        elif d.type in ("D", "DCAP"):
            v = (u[gl[0]] if gl[0] >= 0 else 0.0) - (u[gl[1]] if gl[1] >= 0 else 0.0)
            nVt = num(d.params["n"]) * num(d.params["Vt"])
            xarg = v / nVt
            i0 = num(d.params["Is"]) * ((np.exp(80.0) * (1.0 + (xarg - 80.0)) - 1.0) if xarg > 80.0 else (np.exp(xarg) - 1.0))
            out.append((gl[0], gl[1], "shot", abs(i0), 0.0, name))
            kf = num(d.params.get("KF", 0.0))
            if kf > 0:                           # devices.jl:1435-1443: KF |I0|^AF / f^FFE, under the device's own name like its shot noise
                out.append((gl[0], gl[1], "flicker", kf * abs(i0) ** num(d.params.get("AF", 1.0)), num(d.params.get("FFE", 1.0)), name))
        elif d.type.startswith("VA:"):
            mod = va.get(d.type[3:])[1]
            given = {k: num(v) for k, v in d.model.items()}
            par = va.host_eval.defaults(mod, given)
            V = [u[g] if g >= 0 else 0.0 for g in gl[:mod.n_nodes]]
            vold = [(V[p] if p >= 0 else 0.0) - (V[n] if n >= 0 else 0.0) for p, n in mod.limit_branches]   # at the solution the limit unknowns sit on their probes

            def on_noise(a, b, fn, pwr, expo, label, gl=gl, name=name):
                nm = ("%s_%s" % (name, label.lower())) if label else name
                out.append((gl[a] if a >= 0 else -1, gl[b] if b >= 0 else -1, "white" if fn == "white_noise" else "flicker", pwr, expo, nm))
            va.host_eval.evaluate(mod, V, par, temp_c + 273.15, num(d.params.get("m", 1.0)), gmin, vold=vold, given=set(d.model), mode="dcop", on_noise=on_noise)
        elif d.type == "MOS1":
            # the hand-written sp_mos1 device: its sources are those of the model text it transcribes (models/VADistillerModels.jl/va/mos1.va:
            # rd / rs thermal, channel thermal, flicker), evaluated by the host evaluator on that text at the solution
            mod = va.get("sp_mos1")[1]
            given = {k: num(v) for k, v in d.model.items()}
            par = va.host_eval.defaults(mod, given)
            V = [u[g] if g >= 0 else 0.0 for g in gl[:mod.n_nodes]]           # d, g, s, b, d_int, s_int: the module's node order
            vold = [(V[p] if p >= 0 else 0.0) - (V[n] if n >= 0 else 0.0) for p, n in mod.limit_branches]

            def on_noise(a, b, fn, pwr, expo, label, gl=gl, name=name):
                nm = ("%s_%s" % (name, label.lower())) if label else name
                out.append((gl[a] if a >= 0 else -1, gl[b] if b >= 0 else -1, "white" if fn == "white_noise" else "flicker", pwr, expo, nm))
            va.host_eval.evaluate(mod, V, par, temp_c + 273.15, num(d.params.get("m", 1.0)), gmin, vold=vold, given=set(d.model), mode="dcop", on_noise=on_noise)
        elif d.type == "SMOS":
            # SimpleMOSFET (devices.jl:1667-1732): channel thermal noise 4kT (2/3) gm between drain and source where the device conducts,
            # flicker noise KF |Ids|^AF / f^FFE when KF > 0 -- gm and Ids of the square law at the operating point
            vat = lambda k: u[gl[k]] if gl[k] >= 0 else 0.0
            vgs, vds = vat(1) - vat(2), vat(0) - vat(2)
            vth, kk, lam = num(d.params["Vth"]), num(d.params["K"]), num(d.params["lambda"])
            if vgs <= vth:
                ids = gm = 0.0
            elif vds <= vgs - vth:
                ids, gm = kk * ((vgs - vth) * vds - vds ** 2 / 2), kk * vds
            else:
                ids, gm = kk / 2 * (vgs - vth) ** 2 * (1 + lam * vds), kk * (vgs - vth) * (1 + lam * vds)
            if gm > 0:
                out.append((gl[0], gl[2], "thermal", 2.0 / 3.0 * gm, 0.0, name))
            kf = num(d.params.get("KF", 0.0))
            if kf > 0 and ids != 0.0:
                out.append((gl[0], gl[2], "flicker", kf * abs(ids) ** num(d.params.get("AF", 1.0)), num(d.params.get("FFE", 1.0)), name))
    return out


def noise_indices(st, output, input=None):
    """(out_idx, in_idx or None): the output unknown and the branch row of the input source, with noise!'s own errors"""
    names = list(st.node_names) + list(st.current_names)
    if output in ("gnd", "0"):
        raise KeyError("noise: the output cannot be ground")
    if output not in names:
        raise KeyError("noise: unknown output %s (nodes %s, currents %s)" % (output, st.node_names, st.current_names))
    out_idx = names.index(output)
    in_idx = None
    if input is not None:
        cand = [nm for nm in ("I_" + input, "I_" + input.lower()) if nm in st.current_names]
        if not cand:
            raise KeyError("noise: input source %s is not an independent voltage source (no current variable I_%s)" % (input, input))
        in_idx = st.n_nodes + st.current_names.index(cand[0])
    return out_idx, in_idx


def noise_solve(st, G, C, sources, output, freqs, input=None, temp_c=27.0, adjoint=None, delay=None):
    """noise.jl:150-188 on dense G (gmin already on the voltage-node diagonals) and C: one adjoint solve per frequency,
    S_out(f) = sum_k |x_adj[p_k] - x_adj[n_k]|^2 S_k(f); the same adjoint gives the gain from the input source's branch row.
    ``adjoint``: None -- the dense solve here -- or (index, H): the probe differences H[f, index[(p, n)]] = x_adj[p] - x_adj[n] of this
    point, solved elsewhere (``noise_solve_gpu``) for every source's (p, n) and for (in_idx, -1); the weighting and the sums are the same
    statements in the same source order either way."""
    freqs = np.asarray(freqs, dtype=float)
    if freqs.size == 0:
        raise ValueError("noise(circuit, output, freqs=...) needs a non-empty grid in hertz (e.g. acdec(20, 1, 1e6))")
    out_idx, in_idx = noise_indices(st, output, input)
    e_out = np.zeros(st.n, dtype=complex)
    e_out[out_idx] = 1.0
    onoise = np.zeros(len(freqs))
    contributions = {s[5]: np.zeros(len(freqs)) for s in sources}
    gain = np.zeros(len(freqs), dtype=complex) if input is not None else np.zeros(0, dtype=complex)
    inoise = np.zeros(len(freqs)) if input is not None else np.zeros(0)
    for fi, f in enumerate(freqs):
        if adjoint is None:
            x_adj = np.linalg.solve((1j * 2.0 * np.pi * f * C + G).T if delay is None else ac_matrix(G, C, 2.0 * np.pi * f, delay).T, e_out)
        for s in sources:
            if adjoint is None:
                Hk = (x_adj[s[0]] if s[0] >= 0 else 0.0) - (x_adj[s[1]] if s[1] >= 0 else 0.0)
            else:
                Hk = adjoint[1][fi, adjoint[0][(s[0], s[1])]]
            c = abs(Hk) ** 2 * noise_psd(s, temp_c, f)
            onoise[fi] += c
            contributions[s[5]][fi] += c
        if input is not None:
            H = x_adj[in_idx] if adjoint is None else adjoint[1][fi, adjoint[0][(in_idx, -1)]]
            gain[fi] = H
            inoise[fi] = np.inf if H == 0 else onoise[fi] / abs(H) ** 2
    return NoiseSol(freqs, output, onoise, contributions, temp_c, input, gain, inoise)


# The adjoint sweep's gate, as AC_BERR_MAX above and measured the same way on the TRANSPOSED systems: 16 x the largest componentwise backward
# error np.linalg.solve(A.T, e_out) -- the host path's solve -- leaves over the noise test systems (tests/ac_ref.py CASES on the CPU port's
# G, C at the DC points, e_out at the output nodes of tests/noise_ref.py), and not below 64 eps.
# The measurement gave 1.45e-15 (linear_zoo at 1 Hz; the flip-flop 6.8e-16, the Butterworth filter 8.0e-16, the inverter 1.2e-16), held
# here rounded up to two digits: a gate of 2.4e-14.  Unlike the plain systems' b_ac, e_out at an output node leaves no row whose terms all
# vanish, so the dense solve's componentwise figure stays near eps and the gate is a real one; the static-order adjoint solve measures at most
# 2.1e-16 on the same systems.  tests/test_lu_transpose_cpu.py repeats the measurement.  DESIGN.md section 6.
NOISE_BERR_MEASURED = 1.5e-15
NOISE_BERR_MAX = max(16 * NOISE_BERR_MEASURED, 64 * float(np.finfo(np.float64).eps))


def noise_probe_pairs(source_lists, in_idx=None):
    """The probe pairs of a structure class: the distinct (p, n) over all its points' sources in order of first appearance, plus
    (in_idx, -1) for the gain.  Returns (pairs [K, 2] int32, {(p, n): k})."""
    index = {}
    for srcs in source_lists:
        for s in srcs:
            index.setdefault((int(s[0]), int(s[1])), len(index))
    if in_idx is not None:
        index.setdefault((int(in_idx), -1), len(index))
    return np.array(list(index), dtype=np.int32).reshape(-1, 2), index


def noise_solve_gpu(h, st, G_ref, C_ref, Gd, Cd, source_lists, output, freqs, input=None, temps=27.0, gmin=1e-12, solver="gpu", stats=None,
                    memory="lds", overlay=None):
    """The adjoint sweep of one structure class on the GPU, reachable without ``noise_sources``: ``h`` (a hip.Handle holding the restamp at the
    DC points; ``G_ref`` / ``C_ref`` [B, nnz] are its get_GCb) re-analyses its pivot order on ``ac_pivot_sample`` and solves all points x all
    frequencies in ONE ``ac_adjoint`` call for the class's probe pairs; ``Gd`` / ``Cd`` (dense, gmin on the node diagonals) and
    ``source_lists`` are per point.  A system whose flag is set or whose backward error exceeds NOISE_BERR_MAX is solved again by the host's
    dense adjoint solve.  The PSD weighting and the sums are ``noise_solve``'s.  Returns one NoiseSol per point; ``stats`` (shared by the call)
    is updated as by ``ac_gpu_sweep``.  A circuit that does not fit the launch plan raises with solver="gpu"; with "auto" the points are
    solved on the host and stats["fallback"] says why.  ``memory``: "lds" (the default; DESIGN section 9 has the figures and leaves
    another default to a later change), "hbm" or "auto", as for ``ac_gpu_sweep``: with the latter two a circuit beyond the LDS budget is solved on the GPU;
    stats["memory"] is what the launch used."""
    _ac_memory(memory)
    freqs = np.asarray(freqs, dtype=float)
    if freqs.size == 0:
        raise ValueError("noise(circuit, output, freqs=...) needs a non-empty grid in hertz (e.g. acdec(20, 1, 1e6))")
    if stats is None:
        stats = _ac_stats()
    B, F = len(Gd), freqs.size
    temps = np.broadcast_to(np.asarray(temps, dtype=float), (B,))
    out_idx, in_idx = noise_indices(st, output, input)
    omegas = 2.0 * np.pi * freqs
    pairs, index = noise_probe_pairs(source_lists, in_idx)
    H = None                                             # stays None where the host solves: no pairs, or the fallback of "auto"
    if len(pairs) == 0:                                  # no source and no input: nothing to probe, the sums are empty
        stats["host_systems"] += B * F
    else:
        e_out = pair_column(st.n, (out_idx, -1))
        got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, overlay,
                               lambda h: h.ac_adjoint(omegas, gmin, e_out, pairs),
                               lambda berr, flags: (flags != 0) | ~(berr <= NOISE_BERR_MAX), B * F)
        if got is not None:
            H = np.array(got[0][0])
            for k, f in zip(*np.nonzero(got[1])):
                x_adj = np.linalg.solve(ac_matrix(Gd[k], Cd[k], omegas[f], overlay and overlay.of(k)).T, e_out)
                H[k, f] = probe_differences(x_adj, pairs)
    sols = [noise_solve(st, Gd[k], Cd[k], source_lists[k], output, freqs, input, float(temps[k]), adjoint=None if H is None else (index, H[k]),
                        delay=overlay and overlay.of(k)) for k in range(B)]
    for s in sols:
        s.stats = stats
    return sols


def noise(target, output, freqs, input=None, gmin=1e-12, device=0, solver="host", memory="lds"):
    """noise!(circuit, output; freqs, input, gmin) -- src/noise.jl:118-190.  As for ``ac``: the DC operating point and the restamp at it run on the
    GPU; the sources are collected on the host at that point (noise_sources) and the adjoint sweep is the reference's own dense solve.
    A CircuitSweep returns one NoiseSol per point (one resident batch per structure class).
    ``solver``: "host" (default) as above; "gpu" solves the adjoint systems of every point on the device as well -- points x frequencies
    transposed complex sparse systems in one batched kernel per structure class (``noise_solve_gpu``), for the probe pairs the class's
    sources need -- while the PSD weighting stays in numpy; ``ns.stats`` = {"gpu_systems", "host_systems", "max_berr", "wpb"} of the call.
    "gpu" raises for a circuit too large for the kernel, "auto" takes the host path for it and says so in ``stats["fallback"]``.
    ``memory`` (ignored with solver="host"): "lds" (default), "hbm" or "auto" as for ``ac`` -- with "hbm" / "auto" a circuit beyond the
    160 KB of LDS is solved on the GPU; ``stats["memory"]`` says which ran.  The default stays "lds": DESIGN section 9 has the measured
    figures and leaves making "auto" the default to a later change.
    ``output`` as a list of names (a string is exactly the call above): the result is then, per point, a dict name -> NoiseSol from one DC solve
    and one restamp; the host path runs ``noise_solve`` once per output, a GPU solver makes ONE ``ac_adjoint_multi`` call per structure class
    -- one factorisation per (point, frequency) serving every output (``noise_multi_solve_gpu``; ``stats`` then counts columns as systems and
    has "rhs": the number of outputs).  Each NoiseSol equals the single-output call's to the bit."""
    from contextlib import closing
    _ac_solver(solver), _ac_memory(memory)
    if len(freqs) == 0:
        raise ValueError("noise(circuit, output, freqs=...) needs a non-empty grid in hertz (e.g. acdec(20, 1, 1e6))")
    stats = _ac_stats()
    sweep, mc, pts = _ac_target(target)
    sols = [None] * len(pts)
    outputs = None if isinstance(output, str) else list(output)
    if outputs is not None and (not outputs or len(set(outputs)) != len(outputs)):
        raise ValueError("noise: output as a list needs at least one name, each once")
    with closing(_ac_classes(sweep, mc, pts, gmin, device, "noise")) as classes:
        for sim, st, idx, G, C, lin in classes:
            Gd, Cd = [l[1] for l in lin], [l[2] for l in lin]
            temps = [float(pts[i].get("temp", mc.spec.temp)) for i in idx]
            srcs = [noise_sources(st, mc.circuit, p_i, u_i, temps[k], mc.spec.gmin) for k, (i, _, _, p_i, u_i) in enumerate(lin)]
            ovl = ac_delay_overlay(st, mc.circuit, sim.params, 2.0 * np.pi * np.asarray(freqs, dtype=float), sim.B)
            host = lambda k, o: noise_solve(st, Gd[k], Cd[k], srcs[k], o, freqs, input, temps[k], delay=ovl and ovl.of(k))
            if outputs is not None:
                if solver == "host":
                    got = [{o: host(k, o) for o in outputs} for k in range(len(idx))]
                else:
                    got = noise_multi_solve_gpu(sim.h, st, G, C, Gd, Cd, srcs, outputs, freqs, input, temps, gmin, solver, stats, memory, ovl)
            elif solver == "host":
                got = [host(k, output) for k in range(len(idx))]
            else:
                got = noise_solve_gpu(sim.h, st, G, C, Gd, Cd, srcs, output, freqs, input, temps, gmin, solver, stats, memory, ovl)
            for k, i in enumerate(idx):
                sols[i] = got[k]
    return SweepResult(pts, sols) if sweep else sols[0]


def adjoint_multi_gpu_sweep(h, st, Gd, Cd, G_ref, C_ref, omegas, gmin, cols, pairs, solver, stats, memory="lds", overlay=None):
    """K adjoint right-hand sides per point against ONE factorisation per (point, frequency), on the GPU -- the transposed counterpart of
    ``ac_multi_gpu_sweep``: ``h`` re-analyses its pivot order on ``ac_pivot_sample`` and solves A^T x = cols[k] for points x frequencies x the
    K columns of ``cols`` ([K, n]) in ONE ``ac_adjoint_multi`` call.  Returns the probe differences H [B, F, K, P] for ``pairs``.  The gate is
    ``noise_solve_gpu``'s, per column: a column whose flag is set or whose backward error exceeds NOISE_BERR_MAX is solved again by the host's
    dense adjoint solve on ``Gd`` / ``Cd``.  ``stats`` counts columns as systems and carries "rhs" and "memory".  A circuit the memory home
    refuses raises with solver="gpu"; with "auto" None is returned and stats["fallback"] says why."""
    _ac_memory(memory)
    omegas = np.asarray(omegas, dtype=float)
    cols = np.asarray(cols, dtype=complex)
    B, F, K = len(Gd), omegas.size, cols.shape[0]
    stats["rhs"] = K
    got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, overlay,
                           lambda h: h.ac_adjoint_multi(omegas, gmin, cols, pairs),
                           lambda berr, flags: (flags != 0) | ~(berr <= NOISE_BERR_MAX), B * F * K)
    if got is None:
        return None
    H, redo = got[0][0], got[1]
    for b, f, k in zip(*np.nonzero(redo)):
        x_adj = np.linalg.solve(ac_matrix(Gd[b], Cd[b], omegas[f], overlay and overlay.of(b)).T, cols[k])
        H[b, f, k] = probe_differences(x_adj, pairs)
    return H


def noise_multi_solve_gpu(h, st, G_ref, C_ref, Gd, Cd, source_lists, outputs, freqs, input=None, temps=27.0, gmin=1e-12, solver="gpu", stats=None,
                          memory="lds", overlay=None):
    """``noise_solve_gpu`` for several outputs: column j of ONE ``ac_adjoint_multi`` call is e_out of ``outputs[j]``, the probe pairs are those of
    the single-output call (``noise_probe_pairs``), and the weighting is ``noise_solve``'s per output.  Returns one dict output -> NoiseSol per
    point; the kernel's columns are bit-identical to the single-column kernel's, so each NoiseSol equals ``noise_solve_gpu``'s for that output."""
    freqs = np.asarray(freqs, dtype=float)
    if freqs.size == 0:
        raise ValueError("noise(circuit, output, freqs=...) needs a non-empty grid in hertz (e.g. acdec(20, 1, 1e6))")
    if stats is None:
        stats = _ac_stats()
    B, F, K = len(Gd), freqs.size, len(outputs)
    temps = np.broadcast_to(np.asarray(temps, dtype=float), (B,))
    idxs = [noise_indices(st, o, input) for o in outputs]
    pairs, index = noise_probe_pairs(source_lists, idxs[0][1])
    host = lambda k, o, adj=None: noise_solve(st, Gd[k], Cd[k], source_lists[k], o, freqs, input, float(temps[k]), adjoint=adj,
                                              delay=overlay and overlay.of(k))
    H = None
    stats["rhs"] = K
    if len(pairs):
        cols = np.zeros((K, st.n), dtype=complex)
        cols[np.arange(K), [i[0] for i in idxs]] = 1.0
        H = adjoint_multi_gpu_sweep(h, st, Gd, Cd, G_ref, C_ref, 2.0 * np.pi * freqs, gmin, cols, pairs, solver, stats, memory, overlay)
    else:                                                # no source and no input: nothing to probe, the sums are empty
        stats["host_systems"] += B * F * K
    sols = [{o: host(k, o, None if H is None else (index, H[k, :, j])) for j, o in enumerate(outputs)} for k in range(B)]
    for d in sols:
        for s in d.values():
            s.stats = stats
    return sols


# ---- the noise of N-ports (SPICE's .net with .noise; Spectre's sp with donoise=yes) -------------------------------------------------------
T0 = 290.0            # K: the standard source temperature of a noise figure (IEEE)


class NetworkNoiseSol(NetworkSol):
    """``network_noise``'s result: a NetworkSol (``y``, ``z``, ``s``, ``s_db``) with the noise of the same ports.  ``cy`` [F, P, P] is the
    one-sided correlation matrix of the ports' short-circuit noise currents in A^2 / Hz (Hermitian, positive semidefinite),
    ``cy_by_source`` {source name: [F, P, P]} its parts (their sum is ``cy``), ``temp`` the circuit temperature in degrees Celsius.
    For a two-port -- port 0 the input, port 1 the output -- the noise parameters against T0 = 290 K, all linear ratios unless named ``_db``:
    ``ca`` [F, 2, 2] the chain-form correlation matrix of the input-referred noise voltage and current (M cy M^H, M = [[0, B], [1, D]],
    B = -1 / y21, D = -y11 / y21), ``rn`` = ca00 / (4 k T0) in ohms, ``yopt`` the optimum source admittance, ``gamma_opt`` its reflection
    coefficient for z0 of port 0, ``nfmin``, ``nf(zs)`` the noise factor for a source impedance ``zs`` (default: z0 of port 0; a scalar or
    one value per frequency), ``nf_db`` / ``nfmin_db``.  With another number of ports these raise ValueError.  Where y21 == 0 the chain form
    does not exist: the figures are inf / nan there."""

    def __init__(self, freqs, ports, y, cy, cy_by_source, temp, z0=50.0, dc_x=None):
        super().__init__(freqs, ports, y, z0, dc_x)
        self.cy, self.cy_by_source, self.temp = cy, cy_by_source, temp

    def _two_port(self):
        if len(self.ports) != 2:
            raise ValueError("the noise parameters (ca, rn, yopt, gamma_opt, nfmin, nf) are those of a two-port; this network has %d port(s)" % len(self.ports))

    @property
    def ca(self):
        self._two_port()
        with np.errstate(divide="ignore", invalid="ignore"):
            y11, y21 = self.y[:, 0, 0], self.y[:, 1, 0]
            M = np.zeros((len(self.freqs), 2, 2), dtype=complex)
            M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = -1.0 / y21, 1.0, -y11 / y21
            return M @ self.cy @ np.conj(np.swapaxes(M, 1, 2))

    @property
    def rn(self):
        return self.ca[:, 0, 0].real / (4.0 * K_BOLTZMANN * T0)

    @property
    def yopt(self):
        ca = self.ca
        with np.errstate(divide="ignore", invalid="ignore"):
            b = ca[:, 0, 1].imag / ca[:, 0, 0].real
            return np.sqrt(np.maximum(ca[:, 1, 1].real / ca[:, 0, 0].real - b * b, 0.0)) + 1j * b      # ca is positive semidefinite: below 0 is rounding

    @property
    def gamma_opt(self):
        y0 = 1.0 / float(np.broadcast_to(np.asarray(self.z0, dtype=float), (2,))[0])
        yo = self.yopt
        with np.errstate(divide="ignore", invalid="ignore"):
            return (y0 - yo) / (y0 + yo)

    @property
    def nfmin(self):
        ca = self.ca
        with np.errstate(invalid="ignore"):
            return 1.0 + (ca[:, 0, 1].real + ca[:, 0, 0].real * self.yopt.real) / (2.0 * K_BOLTZMANN * T0)

    def nf(self, zs=None):
        ca = self.ca
        if zs is None:
            zs = float(np.broadcast_to(np.asarray(self.z0, dtype=float), (2,))[0])
        zs = np.broadcast_to(np.asarray(zs, dtype=complex), (len(self.freqs),))
        z = np.stack([np.ones(len(self.freqs), dtype=complex), np.conj(zs)], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1.0 + np.einsum("fi,fij,fj->f", np.conj(z), ca, z).real / (4.0 * K_BOLTZMANN * T0 * zs.real)

    def nf_db(self, zs=None):
        return 10.0 * np.log10(self.nf(zs))

    @property
    def nfmin_db(self):
        return 10.0 * np.log10(self.nfmin)


def network_noise_pairs(rows, source_lists):
    """The probe pairs of a structure class's network noise: ``noise_probe_pairs`` of its sources -- the transfers T[i, s] -- and (row_j, -1)
    for the port rows -- the admittances.  Returns (pairs [K, 2] int32, {(p, n): k})."""
    _, index = noise_probe_pairs(source_lists)
    for r in rows:
        index.setdefault((int(r), -1), len(index))
    return np.array(list(index), dtype=np.int32).reshape(-1, 2), index


def network_noise_solve(st, G, C, sources, ports, freqs, z0=50.0, temp_c=27.0, dc_x=None, adjoint=None, delay=None):
    """The host path of ``network_noise`` on dense G (gmin already on the voltage-node diagonals) and C: per frequency ONE dense LU of A^T serves
    the P adjoint columns -- column i solves A^T l_i = e_row_i with row_i the branch row of port i's source.  From them y[f, i, j] = -l_i[row_j]
    and the transfer of noise source s to the short-circuit current of port i, T[i, s] = l_i[p_s] - l_i[n_s];
    cy[f] = sum_s S_s(f) T[:, s] T[:, s]^H with S_s = noise_psd(s, temp_c, f).
    ``adjoint``: None -- the dense solve here -- or (index, H): the probe differences H[f, i, index[(p, n)]] = l_i[p] - l_i[n] of this point,
    solved elsewhere (``network_noise_gpu``) for every source's (p, n) and for (row_j, -1); the weighting and the sums are the same
    statements in the same source order either way."""
    freqs = np.asarray(freqs, dtype=float)
    rows = port_rows(st, ports)
    P = len(rows)
    if adjoint is None:
        pairs, index = network_noise_pairs(rows, [sources])
        E = np.zeros((st.n, P), dtype=complex)
        E[rows, np.arange(P)] = 1.0
    else:
        index = adjoint[0]
    at_rows = [index[(r, -1)] for r in rows]
    y = np.zeros((len(freqs), P, P), dtype=complex)
    cy = np.zeros((len(freqs), P, P), dtype=complex)
    by_source = {s[5]: np.zeros((len(freqs), P, P), dtype=complex) for s in sources}
    for fi, f in enumerate(freqs):
        if adjoint is None:
            lam = np.linalg.solve((1j * 2.0 * np.pi * f * C + G).T if delay is None else ac_matrix(G, C, 2.0 * np.pi * f, delay).T, E)                       # [n, P]: column i is l_i
            Hf = probe_differences(lam, pairs).T
        else:
            Hf = adjoint[1][fi]                                                              # [P, pairs]
        y[fi] = -Hf[:, at_rows]
        for s in sources:
            T = Hf[:, index[(s[0], s[1])]]
            c = noise_psd(s, temp_c, f) * np.outer(T, np.conj(T))
            cy[fi] += c
            by_source[s[5]][fi] += c
    return NetworkNoiseSol(freqs, ports, y, cy, by_source, temp_c, z0, dc_x)


def network_noise_gpu(h, st, G_ref, C_ref, Gd, Cd, source_lists, ports, freqs, z0=50.0, temps=27.0, gmin=1e-12, solver="gpu", stats=None,
                      memory="lds", dc_x=None, overlay=None):
    """The P adjoint columns of one structure class on the GPU, shaped like ``noise_solve_gpu``: ``h`` (holding the restamp at the DC points)
    solves all points x frequencies x ports in ONE ``ac_adjoint_multi`` call (``adjoint_multi_gpu_sweep``: one factorisation per (point,
    frequency), the gate NOISE_BERR_MAX per column, a rejected column solved again by the host's dense adjoint solve) for the class's probe
    pairs (``network_noise_pairs``); the PSD weighting is ``network_noise_solve``'s.  Returns one NetworkNoiseSol per point (``dc_x``: their
    DC solutions, per point).  A circuit the memory home refuses raises with solver="gpu"; with "auto" the points are solved on the host."""
    _ac_memory(memory)
    freqs = np.asarray(freqs, dtype=float)
    if stats is None:
        stats = _ac_stats()
    B = len(Gd)
    temps = np.broadcast_to(np.asarray(temps, dtype=float), (B,))
    rows = port_rows(st, ports)
    pairs, index = network_noise_pairs(rows, source_lists)
    H = None
    if freqs.size and rows:
        cols = np.zeros((len(rows), st.n), dtype=complex)
        cols[np.arange(len(rows)), rows] = 1.0
        H = adjoint_multi_gpu_sweep(h, st, Gd, Cd, G_ref, C_ref, 2.0 * np.pi * freqs, gmin, cols, pairs, solver, stats, memory, overlay)
    sols = [network_noise_solve(st, Gd[k], Cd[k], source_lists[k], ports, freqs, z0, float(temps[k]), None if dc_x is None else dc_x[k],
                                None if H is None else (index, H[k]), overlay and overlay.of(k)) for k in range(B)]
    for s in sols:
        s.stats = stats
    return sols


def network_noise(target, ports, freqs, z0=50.0, gmin=1e-12, device=0, solver="host", memory="lds"):
    """The noise of an N-port beside its small-signal parameters (SPICE's .net with .noise): ``ports`` as for ``network``, the linearisation as
    for ``ac`` (the same code), the noise sources per point as for ``noise`` (``noise_sources`` at the point's temperature).  Returns a
    NetworkNoiseSol -- ``y`` / ``z`` / ``s`` as ``network``'s, ``cy`` the correlation matrix of the ports' short-circuit noise currents and,
    for a two-port, ``nfmin``, ``rn``, ``yopt`` / ``gamma_opt`` and ``nf(zs)`` -- or for a CircuitSweep a SweepResult of them.  All of it comes
    from P adjoint solves per frequency: A^T l_i = e_row_i for the branch row of port i's source.  A port that is not an independent voltage
    source raises ValueError.
    ``solver``: "host" (default) -- one dense LU of A^T per frequency serving the P columns (``network_noise_solve``); "gpu" -- one
    ``ac_adjoint_multi`` call per structure class, each (point, frequency) system factored once on the device for its P columns
    (``network_noise_gpu``); "auto" -- as "gpu", with the host path for a circuit the memory home refuses.  ``memory`` as for ``ac``.
    ``stats`` = {"gpu_systems", "host_systems", "max_berr", "wpb", "memory", "rhs"} with columns counted as systems."""
    from contextlib import closing
    _ac_solver(solver), _ac_memory(memory)
    ports = list(ports)
    freqs = np.asarray(freqs, dtype=float)
    stats = _ac_stats()
    sweep, mc, pts = _ac_target(target)
    sols = [None] * len(pts)
    with closing(_ac_classes(sweep, mc, pts, gmin, device, "network_noise")) as classes:
        for sim, st, idx, G, C, lin in classes:
            port_rows(st, ports)
            temps = [float(pts[i].get("temp", mc.spec.temp)) for i in idx]
            srcs = [noise_sources(st, mc.circuit, p_i, u_i, temps[k], mc.spec.gmin) for k, (i, Gd, Cd, p_i, u_i) in enumerate(lin)]
            ovl = ac_delay_overlay(st, mc.circuit, sim.params, 2.0 * np.pi * freqs, sim.B)
            if solver == "host":
                got = [network_noise_solve(st, Gd, Cd, srcs[k], ports, freqs, z0, temps[k], u_i, None, ovl and ovl.of(k))
                       for k, (i, Gd, Cd, p_i, u_i) in enumerate(lin)]
            else:
                got = network_noise_gpu(sim.h, st, G, C, [l[1] for l in lin], [l[2] for l in lin], srcs, ports, freqs, z0, temps, gmin, solver,
                                        stats, memory, [l[4] for l in lin], ovl)
            for k, i in enumerate(idx):
                sols[i] = got[k]
    return SweepResult(pts, sols) if sweep else sols[0]


class SensSol:
    """``sensitivity``'s result for one point: the response ``y`` [F] of the output over the grid ``freqs`` (hertz) and its derivatives ``dy``
    [F, K] with respect to the K ``params`` (names; ``values`` their values at the point, "temp" in degrees Celsius; ``steps`` the
    central-difference steps delta_k the stamps were differenced with).  ``dc_value`` is the output at the DC operating point and ``dc_dy``
    [K] its derivative (u+[out] - u-[out]) / (2 delta), a by-product of the perturbed DC solves.  ``normalized(k)`` = p_k dy[:, k];
    ``dmag(k)`` = d|y| / dp_k = Re(conj(y) dy) / |y|; ``dphase(k)`` = d arg(y) / dp_k = Im(dy / y) in radians (k: an index or a name).
    ``stats``: what a GPU solver did, as ``ACSol.stats`` plus "params"; empty on the host path."""

    def __init__(self, freqs, params, values, steps, y, dy, dc_value, dc_dy):
        self.freqs, self.params = np.asarray(freqs, dtype=float), list(params)
        self.values, self.steps = np.asarray(values, dtype=float), np.asarray(steps, dtype=float)
        self.y, self.dy = np.asarray(y, dtype=complex), np.asarray(dy, dtype=complex)
        self.dc_value, self.dc_dy = float(dc_value), np.asarray(dc_dy, dtype=float)
        self.stats = {}

    def _k(self, k):
        return self.params.index(k) if isinstance(k, str) else int(k)

    def normalized(self, k):
        k = self._k(k)
        return self.values[k] * self.dy[:, k]

    def dmag(self, k):
        return np.real(np.conj(self.y) * self.dy[:, self._k(k)]) / np.abs(self.y)

    def dphase(self, k):
        return np.imag(self.dy[:, self._k(k)] / self.y)


def sens_output(st, output):
    """(p, n) unknown indices (-1 = ground) of ``sensitivity``'s output: a name -- resolved as ``noise_indices`` resolves it -- against ground,
    or a (p, n) pair of names of which one may be ground.  ValueError for anything that is not an unknown."""
    names = [output] if isinstance(output, str) else list(output)
    if len(names) not in (1, 2) or not all(isinstance(nm, str) for nm in names):
        raise ValueError("sensitivity: output must be a name or a (p, n) pair of names")
    idx = []
    for nm in names:
        try:
            idx.append(-1 if len(names) == 2 and nm in ("gnd", "0") else noise_indices(st, nm)[0])
        except KeyError as e:
            raise ValueError("sensitivity: " + str(e.args[0])) from None
    if len(idx) == 1:
        idx.append(-1)
    if idx[0] == idx[1]:
        raise ValueError("sensitivity: the output pair names one unknown twice")
    return idx[0], idx[1]


def sensitivity_solve(st, Gd, Cd, b, dG, dC, db, out, omegas):
    """The host path of ``sensitivity``, in dense numpy: with A = G + j w C (``Gd`` with gmin on the voltage-node diagonals, ``Cd``), A x = b and
    the adjoint A^T lambda = e_p - e_n for ``out`` = (p, n) (-1 = ground),
        y = x[p] - x[n],   dy/dp_k = lambda^T (db_k - (dG_k + j w dC_k) x)
    per angular frequency of ``omegas`` -- one factorisation serving the response and all K derivatives.  ``dG`` / ``dC`` [K, n, n] are the
    parameter derivatives of G and C (``sensitivity``: central differences of the stamps of perturbed points), ``db`` [K, n] that of the
    excitation or None for zeros.  Returns (y [F], dy [F, K])."""
    import scipy.linalg as sla
    omegas = np.asarray(omegas, dtype=float).ravel()
    dG, dC = np.asarray(dG, dtype=float), np.asarray(dC, dtype=float)
    K, n = dG.shape[0], st.n
    e = pair_column(n, out)
    b = np.asarray(b, dtype=complex)
    y, dy = np.zeros(omegas.size, dtype=complex), np.zeros((omegas.size, K), dtype=complex)
    for f, w in enumerate(omegas):
        lu = sla.lu_factor(Gd + 1j * w * Cd)
        x, lam = sla.lu_solve(lu, b), sla.lu_solve(lu, e, trans=1)
        y[f] = e @ x
        for k in range(K):
            rhs = -((dG[k] + 1j * w * dC[k]) @ x)
            if db is not None:
                rhs = rhs + db[k]
            dy[f, k] = lam @ rhs
    return y, dy


def sens_gpu_sweep(h, st, G_ref, C_ref, base, plus, minus, scale, bac, out, db, omegas, gmin, solver, stats, host, memory="lds"):
    """The responses and derivatives of one structure class on the GPU: ``h`` (holding the restamp of the expanded batch; ``G_ref`` / ``C_ref``
    [B, nnz] its get_GCb) re-analyses its pivot order on ``ac_pivot_sample`` over all instances -- as ``ac_gpu_sweep`` -- and runs base points x
    frequencies systems in ONE ``ac_sens`` call: ``base`` [NB], ``plus`` / ``minus`` [NB, K] instance indices, ``scale`` [NB, K], ``bac``
    [NB, n], ``out`` the (p, n) output pair, ``db`` [NB, K, n] or None.  A system with a flag set in any column, a forward backward error
    above AC_BERR_MAX or an adjoint one above NOISE_BERR_MAX is solved again by the host: ``host(a)`` gives base a's solver, angular
    frequencies -> (y [F'], s [F', K]) (``sensitivity_solve``).  Returns [(y [F], s [F, K])] per base and updates ``stats`` as ``ac_gpu_sweep``
    does.  A circuit the memory setting refuses raises with solver="gpu"; with "auto" None is returned and stats["fallback"] says why."""
    _ac_memory(memory)
    omegas = np.asarray(omegas, dtype=float)
    got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, None,
                           lambda h: h.ac_sens(omegas, gmin, base, plus, minus, scale, bac, pair_column(st.n, out), out, db),
                           lambda berr, flags: flags.any(axis=2) | ~(berr[:, :, 0] <= AC_BERR_MAX) | ~(berr[:, :, 1] <= NOISE_BERR_MAX),
                           len(base) * omegas.size)
    if got is None:
        return None
    y, s, redo = np.array(got[0][0]), np.array(got[0][1]), got[1]
    for a in np.flatnonzero(redo.any(axis=1)):
        ff = np.flatnonzero(redo[a])
        y[a, ff], s[a, ff] = host(a)(omegas[ff])
    return [(y[a], s[a]) for a in range(len(base))]


def sens_expand(mc, pts, params, rel_step, twin=False):
    """The perturbed batch of ``sensitivity`` and of ``tran(..., sens=)``: point i -> expanded points i * per + [0 | 1 + 2 k | 2 + 2 k] =
    base | p_k + delta_k | p_k - delta_k (``twin``: a second copy of the base behind it, everything after it one further), with delta_k =
    rel_step |p_k| (rel_step when p_k == 0; rel_step (T + 273.15) for "temp").  Returns (values [P, K], steps [P, K], expanded, per)."""
    K = len(params)
    per = 1 + int(bool(twin)) + 2 * K
    values, steps, expanded = np.zeros((len(pts), K)), np.zeros((len(pts), K)), []
    for i, pt in enumerate(pts):
        expanded.append(dict(pt))
        if twin:
            expanded.append(dict(pt))
        for k, nm in enumerate(params):
            v = float(pt.get(nm, mc.spec.temp if nm == "temp" else mc.params.get(nm)))
            d = rel_step * (v + 273.15) if nm == "temp" else rel_step * abs(v) if v != 0 else rel_step
            values[i, k], steps[i, k] = v, d
            for sgn in (1.0, -1.0):
                q = dict(pt)
                q[nm] = v + sgn * d
                expanded.append(q)
    return values, steps, expanded, per


def sens_breaks(mc, point, tspan):
    """the source break points inside ``tspan`` of the circuit at ``point``.  Source waveforms hold plain numbers today, so no parameter
    moves them; ``sens_prepare`` compares base and variant all the same, and a waveform that learns to take a Param is caught there"""
    from .structure import wave_breakpoints
    specs = [wave_breakpoints(d.wave) for d in mc.circuit.devices if d.wave is not None]
    return expand_breakpoints([b for b in specs if b is not None], tspan)


def sens_prepare(mc, pts, sens, rel_step, tspan):
    """Everything ``tran(..., sens=)`` refuses, before any device work, and the expanded batch: (names, values, steps, expanded, per).
    ValueError: an empty list, a name twice, a name that is neither a circuit parameter nor "temp", a rel_step that is not positive, a
    step that changes the structure of the circuit or moves a source break point (the derivative on a frozen grid does not exist there).
    NotImplementedError: a delayed element (its history would need a sensitivity ring of its own) or a behavioural source (its stamp
    carries no Jacobian entries, so G is not dF/du)."""
    names = [sens] if isinstance(sens, str) else list(sens)
    if not names or len(set(names)) != len(names):
        raise ValueError("tran: sens needs at least one parameter name, each once")
    for nm in names:
        if nm != "temp" and nm not in mc.params:
            raise ValueError("tran: %s is not a parameter of the circuit (parameters: %s, or \"temp\")" % (nm, sorted(mc.params)))
    if not rel_step > 0:
        raise ValueError("tran: sens_rel_step must be positive")
    if has_delay(mc.circuit):
        raise NotImplementedError("tran: sens with a delayed element (%s) is not built: the delayed value's own sensitivity would need a history ring"
                                  % ", ".join(d.name for d in mc.circuit.devices if "delay" in d.params))
    bsrc = [d.name for d in mc.circuit.devices if d.type in ("BV", "BI")]
    if bsrc:
        raise NotImplementedError("tran: sens with a behavioural source (%s) is not built: its stamp carries no Jacobian entries, so G is not dF/du there"
                                  % ", ".join(bsrc))
    values, steps, expanded, per = sens_expand(mc, pts, names, rel_step, twin=True)
    cls_of = {}
    for ci, (members, _) in enumerate(structure_classes(mc, expanded)):
        for j in members:
            cls_of[j] = ci
    if len({cls_of[i * per] for i in range(len(pts))}) > 1:
        raise ValueError("tran: sens needs every point of the sweep to share one structure (its unknowns and its pattern)")
    for i in range(len(pts)):
        base_breaks = sens_breaks(mc, expanded[i * per], tspan)
        for k, nm in enumerate(names):
            for j in (i * per + 2 + 2 * k, i * per + 3 + 2 * k):
                if cls_of[j] != cls_of[i * per]:
                    raise ValueError("tran: a step of %g in %s at point %d changes the structure of the circuit (its unknowns or its pattern): "
                                     "the derivative does not exist there" % (steps[i, k], nm, i))
                if not np.array_equal(sens_breaks(mc, expanded[j], tspan), base_breaks):
                    raise ValueError("tran: a step of %g in %s at point %d moves a source break point: the derivative of the trajectory on a "
                                     "frozen step grid does not exist there" % (steps[i, k], nm, i))
    return names, values, steps, expanded, per


def sensitivity(target, output, params, freqs, rel_step=1e-4, gmin=1e-12, device=0, solver="host", memory="lds"):
    """Small-signal sensitivities (SPICE's .SENS on an AC sweep): the response y of ``output`` over ``freqs`` (hertz) as ``ac`` gives it, and
    dy/dp_k for every parameter of ``params`` -- names of circuit parameters, or "temp" -- from ONE factorisation per (point, frequency): with
    the adjoint solve A^T lambda = e_out, dy/dp_k = lambda^T (db/dp_k - (dG/dp_k + j w dC/dp_k) x).  ``output``: a node or current name, or
    a (p, n) pair of names (``sens_output``).  Returns a SensSol, or for a CircuitSweep a SweepResult of them.
    The parameter derivatives of G, C and b are central differences of the STAMPS: every point expands to 1 + 2 K instances of one resident
    batch -- the base, then p_k + delta_k, p_k - delta_k for each k -- with delta_k = rel_step |p_k| (rel_step when p_k == 0; rel_step
    (T + 273.15) for "temp").  The bases are solved as ``ac`` solves them; the perturbed instances then start from their base's solution
    (seeded as ``dc_continuation`` seeds points, so a multi-stable circuit stays on its branch), all must converge, and one restamp at
    those points linearises everything, the moved operating point included.  The variants of a point must keep its structure: a step that
    changes it (a series resistance leaving zero) raises ValueError naming the parameter.
    ``solver``: "host" (default) -- ``sensitivity_solve`` in dense numpy; "gpu" -- one ``ac_sens`` call per structure class: the kernel
    differences the perturbed instances' G and C in place on the device and returns K + 1 numbers per system (csrc/ac_lu.hip: k_ac_sens); a
    system with a flag set, a forward backward error above AC_BERR_MAX or an adjoint one above NOISE_BERR_MAX is redone by the host path;
    "auto" -- as "gpu", with the host path for a circuit the memory home refuses.  ``memory`` as for ``ac``.  ``stats`` =
    {"gpu_systems", "host_systems", "max_berr", "wpb", "memory", "params"}.  Several outputs: call once per output."""
    _ac_solver(solver), _ac_memory(memory)
    params = [params] if isinstance(params, str) else list(params)
    if not params or len(set(params)) != len(params):
        raise ValueError("sensitivity: params needs at least one parameter name, each once")
    freqs = np.asarray(freqs, dtype=float).ravel()
    if freqs.size == 0:
        raise ValueError("sensitivity(circuit, output, params, freqs) needs a non-empty grid in hertz (e.g. acdec(20, 1, 1e6))")
    if not rel_step > 0:
        raise ValueError("sensitivity: rel_step must be positive")
    sweep, mc, pts = _ac_target(target)
    refuse_delay(mc.circuit, "sensitivity", "the bilinear forms over perturbed stamps do not know e^{-j w tau}, and its derivative with respect to tau is not built")
    for nm in params:
        if nm != "temp" and nm not in mc.params:
            raise ValueError("sensitivity: %s is not a parameter of the circuit (parameters: %s, or \"temp\")" % (nm, sorted(mc.params)))
    K, omegas = len(params), 2.0 * np.pi * freqs
    # the perturbed batch: point i -> instances i (1 + 2 K) + [0 | 1 + 2 k | 2 + 2 k] = base | p_k + delta | p_k - delta
    values, steps, expanded, per = sens_expand(mc, pts, params, rel_step)
    cls_of = {}
    classes = structure_classes(mc, expanded)
    for ci, (members, st) in enumerate(classes):
        for j in members:
            cls_of[j] = ci
    for i in range(len(pts)):
        for k, nm in enumerate(params):
            if cls_of[i * per + 1 + 2 * k] != cls_of[i * per] or cls_of[i * per + 2 + 2 * k] != cls_of[i * per]:
                raise ValueError("sensitivity: a step of %g in %s at point %d changes the structure of the circuit (its unknowns or its pattern): "
                                 "the derivative does not exist there" % (steps[i, k], nm, i))
    outs = [sens_output(st, output) for _, st in classes]
    stats = _ac_stats(params=K)
    sols = [None] * len(pts)
    for (members, st), out in zip(classes, outs):
        bases = [j for j in members if j % per == 0]
        if not bases:
            continue
        inst = {j: m for m, j in enumerate(j for b in bases for j in range(b, b + per))}      # expanded index -> instance of this batch
        sim = BatchSimulator(mc, [expanded[j] for j in inst], device, st=st)
        try:
            B, NB = sim.B, len(bases)
            base = np.array([inst[b] for b in bases], dtype=np.int32)
            plus = np.array([[inst[b + 1 + 2 * k] for k in range(K)] for b in bases], dtype=np.int32)
            minus = np.array([[inst[b + 2 + 2 * k] for k in range(K)] for b in bases], dtype=np.int32)
            is_base = np.zeros(B, dtype=bool)
            is_base[base] = True
            u, conv, _ = sim.dc(participate=is_base)
            if not np.all(conv[is_base]):
                raise RuntimeError("sensitivity: the DC operating point did not converge for %d point(s)" % int((~conv[is_base]).sum()))
            start = np.array(u)
            start[~is_base] = np.repeat(u[base], 2 * K, axis=0)                                # every variant from its base's solution
            uv, cv, _ = sim.dc(start, participate=~is_base, cold_start=True)
            if not np.all(cv[~is_base]):
                raise RuntimeError("sensitivity: the DC operating point of %d perturbed instance(s) did not converge" % int((~cv[~is_base]).sum()))
            u[~is_base] = uv[~is_base]
            sim.h.rebuild(u, 0.0)
            G, C, _, _ = sim.h.get_GCb()
            dense = lambda nz: dense_of_ref(st, nz)
            par_of = lambda m: {kk: float(v[m]) for kk, v in sim.params.items()}
            scale = np.array([[1.0 / (2.0 * steps[b // per, k]) for k in range(K)] for b in bases])
            bac = np.array([rhs_ac(st, mc.circuit, par_of(m)) for m in base])
            db = np.array([[(rhs_ac(st, mc.circuit, par_of(plus[a, k])) - rhs_ac(st, mc.circuit, par_of(minus[a, k]))) * scale[a, k] for k in range(K)]
                           for a in range(NB)])
            if not db.any():
                db = None
            val = lambda m: (u[m, out[0]] if out[0] >= 0 else 0.0) - (u[m, out[1]] if out[1] >= 0 else 0.0)

            def host(a):
                dG = np.array([(dense(G[plus[a, k]]) - dense(G[minus[a, k]])) * scale[a, k] for k in range(K)])
                dC = np.array([(dense(C[plus[a, k]]) - dense(C[minus[a, k]])) * scale[a, k] for k in range(K)])
                return lambda om: sensitivity_solve(st, dense_of_ref(st, G[base[a]], gmin), dense(C[base[a]]), bac[a], dG, dC, None if db is None else db[a], out, om)

            got = None if solver == "host" else sens_gpu_sweep(sim.h, st, G, C, base, plus, minus, scale, bac, out, db, omegas, gmin, solver, stats, host, memory)
            if got is None:
                got = [host(a)(omegas) for a in range(NB)]
            for a, b in enumerate(bases):
                i = b // per
                dc_dy = np.array([(val(plus[a, k]) - val(minus[a, k])) * scale[a, k] for k in range(K)])
                sols[i] = SensSol(freqs, params, values[i], steps[i], got[a][0], got[a][1], val(base[a]), dc_dy)
                if solver != "host":
                    sols[i].stats = stats
        finally:
            sim.close()
    return SweepResult(pts, sols) if sweep else sols[0]


def subsystem(ac, name):
    """subsystem(ac, name) -- src/ac.jl:358-388: the single-output descriptor system E x' = A x + B u, y = C x + D u of an ACSol as the tuple
    (A, E, B, C_row, D) = (-G, C, b_ac[:, None], e_name^T, 0) -- what a control-systems package takes.  Ground is not an unknown: ValueError."""
    if getattr(ac, "delay", None) is not None:
        raise NotImplementedError("subsystem: the circuit has a delayed controlled source or a transmission line; A(w) = G + j w C + D(w) is not a "
                                  "descriptor system (E, A, B, C, D)")
    if name in ("0", "gnd", "gnd!"):
        raise ValueError("subsystem: ground is not an unknown of the system")
    try:
        i = ac.st.index_of(name)
    except KeyError as e:
        raise ValueError("subsystem: " + str(e.args[0])) from None
    c = np.zeros((1, ac.st.n))
    c[0, i] = 1.0
    return -np.asarray(ac.G, dtype=float), np.asarray(ac.C, dtype=float), np.asarray(ac.b_ac, dtype=complex)[:, None], c, np.zeros((1, 1))


# A Ritz value theta of A^-1 C whose modulus is below PZ_THETA_TOL times the largest one belongs to the infinite eigenvalues of the pencil (the
# null space of C: algebraic unknowns) and gives no pole.  Measured with the numpy port (tests/pz_ref.py) over the circuits of
# tests/test_pz_cpu.py, on Krylov spaces that closed: the smallest genuine |theta| / max |theta| is 1.4e-2 (the eight-section ladder), the
# largest spurious one 6.3e-16 -- the geometric middle of the gap
PZ_THETA_TOL = 3e-9
# A dense pencil's eigenvalue alpha / beta (both matrices scaled to unit norm) is infinite when |beta| <= PZ_INF_TOL |alpha|: QZ leaves the
# infinite ones at |beta| of the order of the unit roundoff, and a finite pole 1e9 times beyond ||G|| / ||C|| is not one a circuit has
PZ_INF_TOL = 1e-9
# A Ritz pair is accepted as a pole when its residual estimate |h_{m+1,m}| |e_m^T y| / |theta| is at most this; after a breakdown the estimate is
# 0.  The square root of the unit roundoff: a converged pair, to the first order at which the estimate means anything
PZ_RESID_MAX = 1.5e-8
# the relative perturbation of the probe row with which ``pz_solve`` tells the zeros of a reduced model from the images of its zeros at infinity:
# those move by at least its square root (1e-5), a genuine zero is kept when it moves by less than a hundredth of that
PZ_ZERO_PROBE = 1e-10
# two accepted poles from different shifts closer than this (relative to the larger modulus) are one pole: the one with the smaller estimate stays
PZ_MERGE_TOL = 1e-6


def _finite_eigs(M0, M1):
    """The finite s with det(M0 + s M1) = 0 through scipy.linalg.eig in homogeneous form, each matrix scaled to unit norm: an eigenvalue
    alpha / beta is infinite when |beta| <= PZ_INF_TOL |alpha| there."""
    import scipy.linalg as sla
    M0, M1 = np.asarray(M0, dtype=complex), np.asarray(M1, dtype=complex)
    n0, n1 = np.linalg.norm(M0), np.linalg.norm(M1)
    if n0 == 0.0 or n1 == 0.0:
        return np.zeros(0, dtype=complex)
    ab = sla.eig(-M0 / n0, M1 / n1, right=False, homogeneous_eigvals=True)
    keep = np.abs(ab[1]) > PZ_INF_TOL * np.abs(ab[0])
    return ab[0][keep] / ab[1][keep] * (n0 / n1)


def _no_pencil(what, delay):
    if delay is not None:
        raise NotImplementedError("%s: with a delayed element (G + s C + D(s)) is not a matrix pencil; its poles and zeros are those of a "
                                  "transcendental equation" % what)


def poles_dense(G, C, delay=None):
    """The finite generalized eigenvalues of (-G, C): every finite pole of (G + s C)^-1 -- the host path of ``pz`` and the tests' reference.
    ``delay``: an ACSol's ``delay``; anything but None is refused (NotImplementedError)."""
    _no_pencil("poles_dense", delay)
    return _finite_eigs(G, C)


def zeros_dense(G, C, b, c, delay=None):
    """The finite transmission zeros of c^T (G + s C)^-1 b: the finite generalized eigenvalues of the bordered pencil [[G, -b], [c^T, 0]] +
    s [[C, 0], [0, 0]].  ``delay`` as for ``poles_dense``."""
    _no_pencil("zeros_dense", delay)
    n = len(b)
    M0, M1 = np.zeros((n + 1, n + 1), dtype=complex), np.zeros((n + 1, n + 1), dtype=complex)
    M0[:n, :n], M0[:n, n], M0[n, :n] = G, -np.asarray(b), np.asarray(c)
    M1[:n, :n] = C
    return _finite_eigs(M0, M1)


def arnoldi_host(G, C, b, omega0, m, c, breakdown_tol=None):
    """The host implementation of cadnip_ac_arnoldi's algorithm for one system, dense: A = G + j omega0 C, r = A^-1 b, m steps of K = A^-1 C
    with two passes of modified Gram-Schmidt and the kernel's breakdown test.  ``c`` [P, n]: the probe rows.  Returns (H [m+1, m], beta,
    m_eff, l [m, P]) as the kernel lays them out."""
    import scipy.linalg as sla
    from . import hip
    tol = hip.AC_BREAKDOWN_TOL if breakdown_tol is None else breakdown_tol
    n = len(b)
    c = np.asarray(c, dtype=complex).reshape(-1, n)
    H, l = np.zeros((m + 1, m), dtype=complex), np.zeros((m, c.shape[0]), dtype=complex)
    lu = sla.lu_factor(np.asarray(G) + 1j * omega0 * np.asarray(C))
    r = sla.lu_solve(lu, np.asarray(b, dtype=complex))
    beta = float(np.linalg.norm(r))
    if not (beta > 0.0 and np.isfinite(beta)):
        return H, beta, 0, l
    V = [r / beta]
    l[0] = c @ V[0]
    m_eff = m
    for j in range(m):
        w = sla.lu_solve(lu, np.asarray(C) @ V[j])
        nu0 = np.linalg.norm(w)
        for _ in range(2):
            for i in range(j + 1):
                h = np.vdot(V[i], w)
                w = w - h * V[i]
                H[i, j] += h
        nu1 = np.linalg.norm(w)
        if nu0 == 0.0 or nu1 <= tol * nu0:
            m_eff = j + 1
            break
        H[j + 1, j] = nu1
        V.append(w / nu1)
        if j + 1 < m:
            l[j + 1] = c @ V[j + 1]
    return H, beta, m_eff, l


class PZSol:
    """``pz``'s result for one point.  ``poles`` / ``zeros``: complex, in rad/s; ``gain``: the transfer function at s = 0; ``pole_resid`` /
    ``pole_shift``: per pole its residual estimate and the shift that found it (0 / nan on the dense host path); ``reduced(shift)`` ->
    (H [m_eff, m_eff], beta, l [m_eff]) of that shift, from which T(s) = l^T (I + (s - j omega_0) H)^-1 beta e_1 (``transfer``, s in rad/s);
    ``dc_x``: the DC solution; ``stats``: ``ACSol.stats``' keys plus "order", "shifts", "breakdowns".  A shift is named as the caller gave
    it: an angular frequency to ``pz_solve``, hertz to ``pz`` (``shift_scale`` = 2 pi there)."""

    def __init__(self, poles, zeros, gain, pole_resid, pole_shift, models, dc_x=None):
        self.poles, self.zeros, self.gain = np.asarray(poles, dtype=complex), np.asarray(zeros, dtype=complex), complex(gain)
        self.pole_resid, self.pole_shift = np.asarray(pole_resid, dtype=float), np.asarray(pole_shift, dtype=float)
        self._models, self.dc_x, self.stats, self.shift_scale = dict(models), dc_x, {}, 1.0

    def _in_hertz(self, shifts_hz, omegas):
        name = {float(w): float(f) for f, w in zip(shifts_hz, omegas)}
        self._models = {name[w]: v for w, v in self._models.items()}
        self.pole_shift = np.array([name[float(w)] for w in self.pole_shift], dtype=float)
        self.shift_scale = 2.0 * np.pi

    def reduced(self, shift):
        return self._models[float(shift)]

    def transfer(self, s, shift=None):
        key = float(shift) if shift is not None else min(self._models, key=abs)
        H, beta, l = self._models[key]
        w0 = key * self.shift_scale
        e1 = np.zeros(H.shape[0], dtype=complex)
        e1[0] = beta
        return np.array([l @ np.linalg.solve(np.eye(H.shape[0]) + (sv - 1j * w0) * H, e1) for sv in np.atleast_1d(np.asarray(s, dtype=complex))])


def pz_solve(st, G, C, b, out, shifts, order, arnoldi=None):
    """The matrix-level worker of ``pz`` for one point: ``G`` (gmin on the node diagonals), ``C`` dense, ``b`` the excitation, ``out`` a (p, n)
    pair of unknown indices (-1 = ground), ``shifts`` angular frequencies omega_0 of the shifts j omega_0, ``order`` the Arnoldi steps m (at most
    n).  ``arnoldi(omega_0) -> (H, beta, m_eff, l)`` supplies the reduction of a shift (l [m, 1] for the one probe pair) and defaults to
    ``arnoldi_host``.  Per shift: the Ritz values theta of H[:m_eff, :m_eff] give poles j omega_0 - 1 / theta with the residual estimate
    |h_{m_eff+1, m_eff}| |e^T y| / |theta| (0 after a breakdown); theta below PZ_THETA_TOL max |theta| are the infinite eigenvalues and dropped;
    poles whose estimate is at most PZ_RESID_MAX are accepted and merged across the shifts (PZ_MERGE_TOL).  Zeros: the finite eigenvalues of
    the reduced pencil [[I + (s - s_0) H, -beta e_1], [l^T, 0]] of the first shift whose space closed (else of the first shift), beyond
    1 / (PZ_THETA_TOL max |theta|) from the shift dropped.  The gain is the reduced model of the shift nearest 0 at s = 0 (exact for shift 0).
    Returns (PZSol, breakdowns)."""
    n = len(b)
    m = min(int(order), n)
    c = pair_column(n, out)
    if arnoldi is None:
        arnoldi = lambda w0: arnoldi_host(G, C, b, w0, m, c[None])
    cand, models, closed, breakdowns = [], {}, [], 0
    for w0 in (float(w) for w in shifts):
        H, beta, m_eff, l = arnoldi(w0)
        m_eff = int(m_eff)
        H, l = np.asarray(H), np.asarray(l).reshape(H.shape[1], -1)[:, 0]
        Hm = H[:m_eff, :m_eff]
        models[w0] = (Hm, float(beta), l[:m_eff])
        if m_eff == 0:
            continue
        sub = abs(H[m_eff, m_eff - 1])
        if sub == 0.0:
            breakdowns += 1
            closed.append(w0)
        theta, Y = np.linalg.eig(Hm)
        big = np.max(np.abs(theta))
        for k in np.flatnonzero(np.abs(theta) > PZ_THETA_TOL * big):
            y = Y[:, k] / np.linalg.norm(Y[:, k])
            cand.append((1j * w0 - 1.0 / theta[k], sub * abs(y[-1]) / abs(theta[k]), w0))
    poles = []
    for p, res, w0 in sorted((c_ for c_ in cand if c_[1] <= PZ_RESID_MAX), key=lambda c_: c_[1]):
        if not any(abs(p - q[0]) <= PZ_MERGE_TOL * max(abs(p), abs(q[0])) for q in poles):
            poles.append((p, res, w0))
    poles.sort(key=lambda q: (abs(q[0]), q[0].imag))
    zeros, gain = np.zeros(0, dtype=complex), 0.0
    live = [w for w in models if models[w][0].shape[0]]
    if live:
        wz = closed[0] if closed else live[0]
        Hm, beta, l = models[wz]
        k = Hm.shape[0]
        def reduced_zeros(lv):
            M0, M1 = np.zeros((k + 1, k + 1), dtype=complex), np.zeros((k + 1, k + 1), dtype=complex)
            M0[:k, :k], M0[0, k], M0[k, :k] = np.eye(k), -beta, lv
            M1[:k, :k] = Hm
            return _finite_eigs(M0, M1)
        sig = reduced_zeros(l)
        big = np.max(np.abs(np.linalg.eigvals(Hm)))
        sig = sig[np.abs(sig) * (PZ_THETA_TOL * big) < 1.0]
        # a transfer function of relative degree k > 1 has a k-fold zero at infinity, which the reduced pencil returns as k values on a circle of
        # radius eps^(-1/k) -- not large.  They are told apart by what makes them: a perturbation of relative size d moves them by d^(1/k), a
        # genuine zero by d times its condition number
        moved = reduced_zeros(l * (1.0 + PZ_ZERO_PROBE * (-1.0) ** np.arange(k)))
        if sig.size:
            near = np.min(np.abs(sig[:, None] - moved[None, :]), axis=1) if moved.size else np.full(sig.size, np.inf)
            sig = sig[near <= np.sqrt(PZ_ZERO_PROBE) * 1e-2 * np.abs(sig)]
        zeros = 1j * wz + sig
        zeros = zeros[np.argsort(np.abs(zeros))]
        wg = min(live, key=abs)
        Hm, beta, l = models[wg]
        e1 = np.zeros(Hm.shape[0], dtype=complex)
        e1[0] = beta
        gain = l @ np.linalg.solve(np.eye(Hm.shape[0]) - 1j * wg * Hm, e1)
    sol = PZSol([q[0] for q in poles], zeros, gain, [q[1] for q in poles], [q[2] for q in poles], models)
    return sol, breakdowns


def pz_gpu_sweep(h, st, G_ref, C_ref, rhs, out, omegas, m, gmin, solver, stats, memory="lds"):
    """The Arnoldi reductions of one structure class on the GPU: ``h`` (holding the restamp at the DC points) re-analyses its pivot order on
    ``ac_pivot_sample`` over the shifts -- as ``ac_gpu_sweep`` -- and runs points x shifts systems of ``m`` steps in ONE ``ac_arnoldi`` call
    with the probe pair ``out``.  Returns (H [B, S, m+1, m], beta, m_eff, l [B, S, m, 1], redo [B, S]) -- ``redo``: flag bit 0 or 1 set, or
    a backward error above AC_BERR_MAX: the caller reduces that system on the host -- and updates ``stats`` as ``ac_gpu_sweep`` does.  A
    circuit the memory home refuses raises with solver="gpu"; with "auto" None is returned and stats["fallback"] says why."""
    _ac_memory(memory)
    omegas = np.asarray(omegas, dtype=float)
    got = _ac_gated_launch(h, st, G_ref, C_ref, omegas, gmin, solver, stats, memory, None,
                           lambda h: h.ac_arnoldi(omegas, gmin, rhs, m, [out]),
                           lambda berr, flags: ((flags & 3) != 0) | ~(berr <= AC_BERR_MAX), len(rhs) * omegas.size, fallback="host Arnoldi")
    if got is None:
        return None
    (H, beta, meff, l, _, _, _, _), redo = got
    return H, beta, meff, l, redo


def pz(target, output, input=None, shifts=(0.0,), order=16, gmin=1e-12, device=0, solver="host", memory="lds"):
    """Pole-zero analysis of the circuit linearised at its DC operating point (SPICE's .pz; the poles / zeros one takes from the reference's
    ``subsystem`` through a descriptor-systems package): the finite poles of (G + s C)^-1, the zeros and the DC gain of the transfer function
    from ``input`` to ``output``.  ``output``: a name or a (p, n) pair (``sens_output``); ``input``: None -- the circuit's ``ac=`` excitation
    (``rhs_ac``) -- or the name of an independent source (``source_rhs``).  A CircuitSweep returns one PZSol per point.
    ``solver``: "host" (default) -- the dense pencils per point (``poles_dense``, ``zeros_dense``): EVERY finite pole, O(n^3) per point; "gpu" --
    shift-invert Arnoldi of ``order`` steps at the ``shifts`` (hertz, on the imaginary axis): the pivot order is re-analysed on
    ``ac_pivot_sample`` over the shift list and ONE ``ac_arnoldi`` call per structure class runs points x shifts systems
    (csrc/ac_lu.hip: k_ac_arnoldi); ``pz_solve`` turns the reductions into the poles nearest the shifts that converged.  A system whose flag
    bit 0 or 1 is set or whose backward error exceeds AC_BERR_MAX is reduced again by ``arnoldi_host`` and counted in ``stats``
    ("host_systems").  "gpu" raises for a circuit the memory setting refuses; "auto" takes the host Arnoldi for it and says so in
    ``stats["fallback"]``.  ``memory`` as ``ac``.  ``stats`` = ``ACSol.stats``' keys plus "order", "shifts", "breakdowns" (systems whose Krylov
    space closed before ``order`` steps: their poles are exact)."""
    from contextlib import closing
    _ac_solver(solver), _ac_memory(memory)
    omegas = 2.0 * np.pi * np.asarray(shifts, dtype=float).ravel()
    if solver != "host" and (omegas.size == 0 or int(order) < 1):
        raise ValueError("pz: at least one shift and one Arnoldi step")
    sweep, mc, pts = _ac_target(target)
    refuse_delay(mc.circuit, "pz", "(G + s C + D(s)) is not a matrix pencil, so neither the dense eigenvalue path nor the Arnoldi kernel applies")
    stats = _ac_stats(order=int(order), shifts=int(omegas.size), breakdowns=0)
    sols = [None] * len(pts)
    with closing(_ac_classes(sweep, mc, pts, gmin, device, "pz")) as classes:
        for sim, st, idx, G, C, lin in classes:
            out = sens_output(st, output)
            c = pair_column(st.n, out)
            rhs = [rhs_ac(st, mc.circuit, p_i) if input is None else source_rhs(st, mc.circuit, input) for _, _, _, p_i, _ in lin]
            if solver == "host":
                for (i, Gd, Cd, p_i, u_i), b in zip(lin, rhs):
                    sols[i] = PZSol(poles_dense(Gd, Cd), zeros_dense(Gd, Cd, b, c), c @ np.linalg.solve(Gd.astype(complex), b), [], [], {}, u_i)
                    sols[i].pole_resid, sols[i].pole_shift = np.zeros(len(sols[i].poles)), np.full(len(sols[i].poles), np.nan)
                continue
            m = min(int(order), st.n)
            got = pz_gpu_sweep(sim.h, st, G, C, np.array(rhs), out, omegas, m, gmin, solver, stats, memory)
            for k, ((i, Gd, Cd, p_i, u_i), b) in enumerate(zip(lin, rhs)):
                def arnoldi(w0, k=k, Gd=Gd, Cd=Cd, b=b):
                    s = int(np.flatnonzero(omegas == w0)[0])
                    if got is None or got[4][k, s]:
                        return arnoldi_host(Gd, Cd, b, w0, m, c[None])
                    return got[0][k, s], got[1][k, s], got[2][k, s], got[3][k, s]
                sols[i], nb = pz_solve(st, Gd, Cd, b, out, omegas, m, arnoldi)
                sols[i].dc_x = u_i
                sols[i]._in_hertz(np.asarray(shifts, dtype=float).ravel(), omegas)
                stats["breakdowns"] += nb
    if solver != "host":
        for s in sols:
            s.stats = stats
    return SweepResult(pts, sols) if sweep else sols[0]


TRAN_RETCODES = {1: "Success", -4: "DelayHistoryOverflow"}      # per-instance status of cadnip_tran_run -> TranSolution.retcode; anything else: "Failure"


def delay_breakpoints(breaks, taus, tspan, max_points=100000):
    """Source break points propagated through transport delays: a kink of a source at t_b reappears at t_b + sum k_i tau_i wherever a delayed
    element passes it on, so those times join the stop list.  ``breaks``: the sorted stop times inside ``tspan``
    (``structure.expand_breakpoints``); the start of the run, where every source leaves its DC value, is a seed as well.  ``taus``: the
    delays of all terms at all points -- the break list is global, so the images are taken over the distinct values of all instances.
    Generated breadth-first, by number of delays added, until nothing new falls inside ``tspan`` or the total reaches ``max_points`` (the
    cap of ``expand_breakpoints``); sorted and deduplicated by that function's 4-ulp rule.  Returns (stop times, number added, truncated)."""
    import bisect
    import math
    t0, t1 = float(tspan[0]), float(tspan[1])
    near = lambda a, b: abs(a - b) <= 4 * max(math.ulp(a), math.ulp(b))

    def dedupe(ts):
        out = []
        for t in sorted(ts):
            if not out or not near(out[-1], t):
                out.append(t)
        return out

    def known(ts, t):
        k = bisect.bisect_left(ts, t)
        return any(0 <= j < len(ts) and near(ts[j], t) for j in (k - 1, k))

    taus = sorted({float(x) for x in np.ravel(taus)})
    pts = dedupe(float(b) for b in breaks)
    n_base, level, truncated = len(pts), [t0] + pts, False
    while level and taus and not truncated:
        new = [t for t in dedupe(t + tau for t in level for tau in taus if t0 < t + tau < t1) if not known(pts, t)]
        if len(pts) + len(new) > max_points:
            new, truncated = new[:max(max_points - len(pts), 0)], True
        pts = dedupe(pts + new)
        level = new
    return pts, len(pts) - n_base, truncated


def _check_delays(target):
    """every delay of the circuit at every point of the target is a positive finite number, or ValueError -- before any device work"""
    from .circuit import resolve
    mc = target.circuit if isinstance(target, CircuitSweep) else target
    pts = target.points() if isinstance(target, CircuitSweep) else [{}]
    for d in mc.circuit.devices:
        if "delay" not in d.params:
            continue
        for pt in pts:
            p = dict(mc.params)
            p.update({k: v for k, v in pt.items() if k != "temp"})
            tau = float(resolve(d.params["delay"], p))
            if not (np.isfinite(tau) and tau > 0.0):
                raise ValueError("tran: the delay of %s is %r at the point %r; every delay must be positive and finite (a zero delay is no delay: "
                                 "leave it out of the circuit)" % (d.name, tau, pt))


def tran(target, tspan, abstol=1e-10, reltol=1e-8, saveat=None, device=0, **kw):
    """tran!(circuit, tspan) / tran!(cs::CircuitSweep, tspan) -- sweeps.jl:588-665, 692-707.

    A circuit with delayed controlled sources or transmission lines (``Circuit.E/G/H/F(..., delay=)``, ``Circuit.T``, ``TD=`` in a deck) is
    refused (NotImplementedError) unless the call says ``delays="history"``: then the handle keeps a history ring of ``delay_depth``
    accepted points per instance and integrates the delay-differential system (``BatchSimulator.tran``).  "refuse"
    stays the default for now -- flipping it is a later change.  An instance whose delayed look-up fell off the ring has retcode
    "DelayHistoryOverflow".

    ``sens=[names]`` (circuit parameters or "temp", each once; ``sens_rel_step=1e-4``): the forward sensitivities of the trajectory with
    respect to those parameters, on the step sequence the run takes (``BatchSimulator.tran``): ``sol.sens``
    [K, n_save, n], ``sol.sens_params``, ``sol.sens_steps``, ``sol.sens_flag``, ``sol.sensitivity(name, param)``; a CircuitSweep gives one
    such result per point, and stats["sens_params"] is K.  What is refused, before any device work: ``sens_prepare``."""
    if kw.get("sens") is not None:
        mc_ = target.circuit if isinstance(target, CircuitSweep) else target
        sens_prepare(mc_, target.points() if isinstance(target, CircuitSweep) else [{}], kw["sens"], kw.get("sens_rel_step", 1e-4),
                     (float(tspan[0]), float(tspan[1])))
    if kw.get("delays", "refuse") not in ("refuse", "history"):
        raise ValueError("delays must be 'refuse' or 'history'")
    if kw.get("delays", "refuse") == "refuse":
        refuse_delay((target.circuit if isinstance(target, CircuitSweep) else target).circuit, "tran",
                     "a transient needs the delayed quantity's history: ask for it with delays=\"history\" (without it a delay-differential integrator is not built into the call)")
    else:
        _check_delays(target)
    tspan = (float(tspan[0]), float(tspan[1]))
    if saveat is None:
        saveat = np.linspace(tspan[0], tspan[1], 501)
    saveat = np.asarray(saveat, dtype=float)
    if isinstance(target, CircuitSweep):
        sim = BatchSimulator(target.circuit, target.points(), device)
    else:
        sim = BatchSimulator(target, None, device)
    try:
        out, per, stats = sim.tran(tspan, _resolve_abstol(abstol, sim.st), reltol, saveat, **kw)
        sens = {k: stats.pop(k) for k in ("sens", "sens_steps", "sens_values", "sens_flag", "sens_names") if k in stats}
        sols = []
        for i in range(sim.B):
            s = {"nnonliniter": int(per[i, 0]), "naccept": int(per[i, 1]), "nreject": int(per[i, 2])}
            sols.append(TranSolution(sim.st, saveat, out[i], s, TRAN_RETCODES.get(int(per[i, 3]), "Failure")))
            if sens:
                sols[-1].sens, sols[-1].sens_params = sens["sens"][i], list(sens["sens_names"])
                sols[-1].sens_steps, sols[-1].sens_flag = sens["sens_steps"][i], int(sens["sens_flag"][i])
        if isinstance(target, CircuitSweep):
            res = SweepResult(target.points(), sols)
            res.stats = stats
            return res
        sols[0].run_stats = stats
        return sols[0]
    finally:
        sim.close()
