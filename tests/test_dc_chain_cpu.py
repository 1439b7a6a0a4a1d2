"""csrc/dc_chain.hpp is the DC fallback chain of cadnip_dc_run as host-only policy: stages, ladders, participation, log.  This host-only
check compiles it with the host compiler and gives it a runner that calls the oracle's own Newton functions (oracle/mna_ref.py:
dc_pcnr_newton / dc_newton_plain) per instance, with the homotopy terms the chain asked for.  The oracle's chain
(tests/dc_chain_util.oracle_chain) runs the very same functions, so there is no rounding between the two: logs are equal rung for rung
and solutions bit for bit.  This is where the ladder semantics are pinned; tests/test_gpu_dc_fallbacks.py holds the device plumbing
under the chain to the same oracle end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import mna_ref as M
from oracle.netlist_ref import make_builder
from tests.dc_chain_util import oracle_chain, same_ladder
from tests.test_gpu_dc_fallbacks import CASES, _rectifier_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")

SHIM = r"""
#include "dc_chain.hpp"
using namespace cadnip;
typedef int (*runner_t)(int stage, int use_pcnr, int cold_start, int fused, const int* part, const double* u, const double* gshunt,
                        const double* srcFact, int* status, double* R, long long* iters);
static std::vector<DCLogEntry> g_log;
extern "C" {
// out: total Newton solves, n_failed, direct, log entries
int t_chain(int B, int n, int use_pcnr, int cold_start, int fused, int use_stepping, int has_limits, double gshunt, double srcFact,
            const int* participate, double* u, int* converged, runner_t cb, long long* out) {
  g_log.clear();
  std::vector<double> ends((size_t)B * n);
  auto runner = [&](const DCRun& r) {
    if (int rc = cb(r.stage, r.use_pcnr, r.cold_start, r.fused, r.part, r.u, r.gshunt, r.srcFact, r.status, ends.data(), r.iters)) return rc;
    std::copy(ends.begin(), ends.end(), r.dest());
    return 0;
  };
  const DCChainOpts o{use_pcnr, cold_start, fused, use_stepping, has_limits != 0, gshunt, srcFact, participate};
  DCChainResult res;
  const int rc = dc_chain(o, B, n, u, converged, runner, g_log, res);
  out[0] = res.iters; out[1] = res.n_failed; out[2] = res.direct; out[3] = (long long)g_log.size();
  return rc;
}
void t_log(int* inst, int* stage, double* value, int* ok, long long* iters) {
  for (size_t k = 0; k < g_log.size(); ++k) { inst[k] = g_log[k].inst; stage[k] = g_log[k].stage; value[k] = g_log[k].value; ok[k] = g_log[k].ok; iters[k] = g_log[k].iters; }
}
}
"""

_I, _D, _L = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_longlong)
RUNNER = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I, _D, _D, _D, _I, _D, _L)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("dc_chain")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    L = C.CDLL(so)
    L.t_chain.argtypes = [C.c_int] * 7 + [C.c_double, C.c_double, _I, _D, _I, RUNNER, _L]
    L.t_log.restype = None
    return L


def _instance(circ, params=None):
    b = make_builder(circ.to_dicts(params or {}))
    spec = M.MNASpec(mode="dcop")
    ctx = M.build_with_detection(b, {}, spec)
    cs = M.compile_structure(b, {}, spec, ctx=ctx)
    return cs, M.create_workspace(cs, ctx=ctx)


class Chain:
    """One dc_chain call on a batch of oracle instances [(cs, ws)]: u, conv, per-instance logs, the runner calls as (stage, part)."""

    def __init__(self, lib, insts, u0=None, participate=None, use_stepping=True, abstol=1e-10, maxiters=100):
        B, n = len(insts), insts[0][0].n
        assert all(cs.n == n for cs, _ in insts)
        spec = insts[0][0].spec
        self.calls, errors, done = [], [], set()

        def runner(stage, use_pcnr, cold_start, fused, part, u, gshunt, srcFact, status, R, iters):
            try:
                p = [int(part[i]) for i in range(B)]
                self.calls.append((stage, p))
                # never an empty run, never a finished or a masked instance
                assert any(p) and not any(p[i] and i in done for i in range(B))
                assert participate is None or not any(p[i] and not participate[i] for i in range(B))
                assert (use_pcnr, cold_start, fused) == ((1, 1, 0) if stage == 0 else (0, 0, 0))
                start, ends = np.ctypeslib.as_array(u, (B, n)), np.ctypeslib.as_array(R, (B, n))
                for i in range(B):
                    if not p[i]:
                        continue
                    cs, ws = insts[i]
                    cs_run = cs.with_spec(cs.spec.replace(gshunt=gshunt[i], srcFact=srcFact[i]))
                    newton = M.dc_pcnr_newton if use_pcnr and cs.n_limits > 0 else M.dc_newton_plain
                    with np.errstate(all="ignore"):
                        un, ok, it = newton(cs_run, ws, start[i].copy(), abstol, maxiters)
                    status[i], iters[i] = (1 if ok else -3), it
                    ends[i] = un
                    if ok and (stage <= 1 or (stage == 2 and gshunt[i] == spec.gshunt) or (stage == 3 and srcFact[i] >= 1.0)):
                        done.add(i)                      # solved at the circuit's own spec: it has left the chain
                return 0
            except BaseException as e:      # ctypes swallows what a callback raises: kept, raised again after the call
                errors.append(e)
                return 99

        self.u = np.zeros((B, n)) if u0 is None else np.array(u0, dtype=float).reshape(B, n)
        conv = np.full(B, -1, dtype=np.int32)
        pm = None if participate is None else np.ascontiguousarray(participate, dtype=np.int32)
        out = np.zeros(4, dtype=np.int64)
        self.rc = lib.t_chain(B, n, 1, 1, 0, int(use_stepping), int(insts[0][0].n_limits > 0), spec.gshunt, spec.srcFact,
                              None if pm is None else pm.ctypes.data_as(_I), self.u.ctypes.data_as(_D), conv.ctypes.data_as(_I), RUNNER(runner),
                              out.ctypes.data_as(_L))
        if errors:
            raise errors[0]
        assert self.rc == 0
        self.iters, self.n_failed, self.direct, k = (int(v) for v in out)
        inst, stage, ok = (np.zeros(max(k, 1), dtype=np.int32) for _ in range(3))
        val, it = np.zeros(max(k, 1)), np.zeros(max(k, 1), dtype=np.int64)
        lib.t_log(inst.ctypes.data_as(_I), stage.ctypes.data_as(_I), val.ctypes.data_as(_D), ok.ctypes.data_as(_I), it.ctypes.data_as(_L))
        self.log = [(int(inst[j]), int(stage[j]), float(val[j]), bool(ok[j]), int(it[j])) for j in range(k)]
        self.per = [[e[1:] for e in self.log if e[0] == i] for i in range(B)]
        self.conv = [bool(c) for c in conv]
        assert self.n_failed == sum(1 for i in range(B) if not self.conv[i] and (participate is None or participate[i]))


_cache = {}


def _oracle_case(name):
    """(instance, oracle result) of a CASES entry, computed once"""
    if name not in _cache:
        mk, kw, _, _ = CASES[name]
        cs, ws = _instance(mk())
        _cache[name] = ((cs, ws), oracle_chain(cs, ws, np.zeros(cs.n), **kw))
    return _cache[name]


def _oracle_sweep(limit):
    """(instances, oracle results, options) of the rectifier sweeps of tests/test_gpu_dc_fallbacks.py, computed once"""
    if limit not in _cache:
        vins, kw = ([5.0, 0.8, 500.0, 0.7, 3.0, 0.5], dict(maxiters=10)) if limit else ([0.5, 8.0, 5.0, 2.0], {})
        insts = [_instance(_rectifier_sweep(limit), {"vin": v}) for v in vins]
        _cache[limit] = (insts, [oracle_chain(cs, ws, np.zeros(cs.n), **kw) for cs, ws in insts], kw)
    return _cache[limit]


def _same_as_oracle(got, i, ref):
    u_ref, ok_ref, log_ref = ref
    assert got.conv[i] == ok_ref
    assert same_ladder(got.per[i], log_ref), (i, got.per[i], log_ref)
    if ok_ref:
        assert np.array_equal(got.u[i], u_ref)


@pytest.mark.parametrize("name", list(CASES))
def test_chain_matches_oracle_rung_for_rung(lib, name):
    _, kw, expect_ok, stages = CASES[name]
    inst, ref = _oracle_case(name)
    assert ref[1] == expect_ok and sorted({e[0] for e in ref[2]}) == list(stages)
    got = Chain(lib, [inst], **kw)
    _same_as_oracle(got, 0, ref)
    assert got.iters == sum(e[3] for e in ref[2]) and got.n_failed == (0 if expect_ok else 1) and not got.direct
    assert [s for s, _ in got.calls] == [e[0] for e in got.per[0]]            # one runner call per log entry


@pytest.mark.parametrize("limit", [True, False])
def test_batch_points_walk_their_own_ladders(lib, limit):
    """Every point's log is the log of that point alone -- the hopeless 8 V point's 55 runs included -- and dropping points from the
    batch leaves the others' logs and solutions as they are."""
    insts, ref, kw = _oracle_sweep(limit)
    if limit:
        assert all(r[1] for r in ref) and [max(e[0] for e in r[2]) for r in ref] == [0, 2, 0, 1, 0, 1]
        keep = [0, 2, 3, 4]
    else:
        assert [r[1] for r in ref] == [True, False, True, True] and len(ref[1][2]) == 55 and {e[0] for e in ref[1][2]} == {1, 2, 3}
        keep = [0, 2, 3]
    got = Chain(lib, insts, **kw)
    for i, r in enumerate(ref):
        _same_as_oracle(got, i, r)
    assert got.iters == sum(e[3] for r in ref for e in r[2]) and got.n_failed == sum(not r[1] for r in ref) and not got.direct
    alone = Chain(lib, [insts[1]], **kw)                                      # the hardest point by itself
    assert alone.per[0] == got.per[1] and alone.conv[0] == got.conv[1] and np.array_equal(alone.u[0], got.u[1])
    fewer = Chain(lib, [insts[i] for i in keep], **kw)
    for k, i in enumerate(keep):
        assert fewer.per[k] == got.per[i] and fewer.conv[k] == got.conv[i] and np.array_equal(fewer.u[k], got.u[i])


def test_masked_instances_sit_the_call_out(lib):
    insts, ref, kw = _oracle_sweep(True)
    B, n = len(insts), insts[0][0].n
    mask = [1, 0, 1, 1, 0, 1]
    u0 = np.zeros((B, n))
    u0[1], u0[4] = 0.25, -1.5                                                 # theirs to keep
    got = Chain(lib, insts, u0=u0, participate=mask, **kw)
    full = Chain(lib, insts, **kw)
    for i in range(B):
        if mask[i]:
            assert got.per[i] == full.per[i] and got.conv[i] and np.array_equal(got.u[i], full.u[i])
        else:
            assert got.per[i] == [] and not got.conv[i] and np.array_equal(got.u[i], u0[i])
    assert got.n_failed == 0 and not got.direct
    nobody = Chain(lib, insts, u0=u0, participate=[0] * B, **kw)              # nothing to run: the runner is not called
    assert nobody.calls == [] and nobody.log == [] and nobody.conv == [False] * B and np.array_equal(nobody.u, u0) and nobody.n_failed == 0


def test_everybody_solved_by_the_first_run_is_direct(lib):
    insts, ref, kw = _oracle_sweep(True)
    easy = [0, 2, 4]                                                          # 5 V, 500 V, 3 V: PCNR converges
    got = Chain(lib, [insts[i] for i in easy], **kw)
    assert got.direct and got.calls == [(0, [1, 1, 1])] and got.conv == [True] * 3 and got.n_failed == 0
    for k, i in enumerate(easy):
        _same_as_oracle(got, k, ref[i])
    masked = Chain(lib, [insts[i] for i in easy], participate=[1, 1, 1], **kw)   # with a mask the general path delivers the same
    assert not masked.direct and len(masked.calls) == 1 and masked.per == got.per and np.array_equal(masked.u, got.u) and masked.conv == got.conv


@pytest.mark.parametrize("name", ["rect_nolimit", "rect_5_iterations"])
def test_without_stepping_the_chain_ends_after_stage_1(lib, name):
    _, kw, _, _ = CASES[name]
    (cs, ws), _ = _oracle_case(name)
    ref = oracle_chain(cs, ws, np.zeros(cs.n), use_stepping=False, **kw)
    assert not ref[1] and {e[0] for e in ref[2]} <= {0, 1}
    got = Chain(lib, [(cs, ws)], use_stepping=False, **kw)
    _same_as_oracle(got, 0, ref)
    assert got.n_failed == 1 and got.iters == sum(e[3] for e in ref[2])
    assert np.array_equal(got.u[0], ref[0])                                   # left with the state of its last run, as the oracle is
