"""csrc/dc_chain.hpp, the zero start (cold_start = 2, CADNIP_DC_COLD_ZERO) and the uninitialised end-state buffer.  Host only, in the
manner of tests/test_dc_chain_cpu.py: the header is compiled with the host compiler and its runner calls the oracle's Newton functions.

  * cold_start = 2 without a mask: the chain reads nothing of `u` (here filled with NaN) and hands the runner a null start state for the
    first run; everything it reports equals, bit for bit, the cold_start = 1 run on explicit zeros -- when the first run solves everybody,
    when some instance falls through to stage 1, when some instance goes on to the ladders.
  * with a mask, 2 is 1: `u` is read, masked rows come back untouched.
  * the chain's end-state buffer R is not initialised.  The poisoned build fills it with NaN (CADNIP_DC_CHAIN_POISON), and its runner writes
    the rows of the run's participants only and sets every other row of R to NaN again on every run: a read of a row the current run did
    not write -- never written, or stale from an earlier run -- would put NaN into the results."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import mna_ref as M
from tests.test_dc_chain_cpu import _instance, _oracle_sweep
from tests.test_gpu_dc_fallbacks import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")

SHIM = r"""
#include "dc_chain.hpp"
using namespace cadnip;
// u: null on the first run of a zero start
typedef int (*runner_t)(int stage, int use_pcnr, int cold_start, int fused, const int* part, const double* u, const double* gshunt,
                        const double* srcFact, int* status, double* ends, long long* iters);
static std::vector<DCLogEntry> g_log;
extern "C" {
// out: total Newton solves, n_failed, direct, log entries
int t_chain(int B, int n, int use_pcnr, int cold_start, int fused, int use_stepping, int has_limits, double gshunt, double srcFact,
            const int* participate, double* u, int* converged, runner_t cb, long long* out) {
  g_log.clear();
  std::vector<double> ends((size_t)B * n);
  auto runner = [&](const DCRun& r) {
    if (int rc = cb(r.stage, r.use_pcnr, r.cold_start, r.fused, r.part, r.u, r.gshunt, r.srcFact, r.status, ends.data(), r.iters)) return rc;
    double* dst = r.dest();
    for (int i = 0; i < B; ++i) {
      if (r.part[i]) std::copy(ends.begin() + (size_t)i * n, ends.begin() + (size_t)(i + 1) * n, dst + (size_t)i * n);
#ifdef CADNIP_DC_CHAIN_POISON
      else if (dst == r.R) std::fill(dst + (size_t)i * n, dst + (size_t)(i + 1) * n, std::numeric_limits<double>::quiet_NaN());
#endif
    }
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
def libs(tmp_path_factory):
    """the shim as it is, and with the chain's end-state buffer poisoned"""
    d = tmp_path_factory.mktemp("dc_chain_zero")
    src = str(d / "shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    out = {}
    for name, flags in (("plain", []), ("poison", ["-DCADNIP_DC_CHAIN_POISON"])):
        so = str(d / ("libshim_%s.so" % name))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src] + flags)
        L = C.CDLL(so)
        L.t_chain.argtypes = [C.c_int] * 7 + [C.c_double, C.c_double, _I, _D, _I, RUNNER, _L]
        L.t_log.restype = None
        out[name] = L
    return out


class Chain:
    """One dc_chain call on a batch of oracle instances [(cs, ws)] with the given cold_start and `u` as handed in."""

    def __init__(self, lib, insts, cold_start, u, participate=None, abstol=1e-10, maxiters=100):
        B, n = len(insts), insts[0][0].n
        spec = insts[0][0].spec
        zero = cold_start == 2 and participate is None
        self.calls, errors = [], []

        def runner(stage, use_pcnr, cold, fused, part, u_run, gshunt, srcFact, status, R, iters):
            try:
                p = [int(part[i]) for i in range(B)]
                self.calls.append((stage, p))
                assert any(p) and (participate is None or not any(p[i] and not participate[i] for i in range(B)))
                # stage 0 of a zero start: cold_start 2 and no start state; everything else is told 1 / 0 and given one
                assert (use_pcnr, cold, fused) == ((1, 2 if zero else 1, 0) if stage == 0 else (0, 0, 0))
                assert bool(u_run) == (not (zero and stage == 0))
                start = np.ctypeslib.as_array(u_run, (B, n)) if u_run else np.zeros((B, n))
                ends = np.ctypeslib.as_array(R, (B, n))
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
                return 0
            except BaseException as e:      # ctypes swallows what a callback raises: kept, raised again after the call
                errors.append(e)
                return 99

        self.u = np.array(u, dtype=float).reshape(B, n)
        conv = np.full(B, -1, dtype=np.int32)
        pm = None if participate is None else np.ascontiguousarray(participate, dtype=np.int32)
        out = np.zeros(4, dtype=np.int64)
        rc = lib.t_chain(B, n, 1, cold_start, 0, 1, int(insts[0][0].n_limits > 0), spec.gshunt, spec.srcFact,
                         None if pm is None else pm.ctypes.data_as(_I), self.u.ctypes.data_as(_D), conv.ctypes.data_as(_I), RUNNER(runner),
                         out.ctypes.data_as(_L))
        if errors:
            raise errors[0]
        assert rc == 0
        self.iters, self.n_failed, self.direct, k = (int(v) for v in out)
        inst, stage, ok = (np.zeros(max(k, 1), dtype=np.int32) for _ in range(3))
        val, it = np.zeros(max(k, 1)), np.zeros(max(k, 1), dtype=np.int64)
        lib.t_log(inst.ctypes.data_as(_I), stage.ctypes.data_as(_I), val.ctypes.data_as(_D), ok.ctypes.data_as(_I), it.ctypes.data_as(_L))
        self.log = [(int(inst[j]), int(stage[j]), float(val[j]), bool(ok[j]), int(it[j])) for j in range(k)]
        self.conv = [int(c) for c in conv]

    def same_as(self, other):
        # (array_equal with equal_nan: an unsolved instance's last state may hold non-finite words, the same ones in both)
        return (self.log == other.log and np.array_equal(self.u, other.u, equal_nan=True) and self.conv == other.conv
                and (self.iters, self.n_failed, self.direct) == (other.iters, other.n_failed, other.direct))


_ref = {}


def _batch(name):
    """(instances, options, the cold_start = 1 run on explicit zeros with the plain shim -- made by the first test that asks, then shared)"""
    if name in CASES:
        mk, kw, _, _ = CASES[name]
        return [_instance(mk())], kw
    insts, _, kw = _oracle_sweep(True)                      # rectifier, 10 iterations: 5 V, 0.8 V, 500 V, 0.7 V, 3 V, 0.5 V
    pick = {"stage0_solves_all": [0, 2, 4], "one_falls_to_stage1": [0, 3, 4], "one_goes_to_the_ladders": [0, 1, 2, 3, 4, 5]}[name]
    return [insts[i] for i in pick], kw


def _reference(libs, name):
    if name not in _ref:
        insts, kw = _batch(name)
        _ref[name] = Chain(libs["plain"], insts, 1, np.zeros((len(insts), insts[0][0].n)), **kw)
    return _ref[name]


def _garbage(insts):
    return np.full((len(insts), insts[0][0].n), np.nan)


SITUATIONS = {"stage0_solves_all": {0}, "one_falls_to_stage1": {0, 1}, "one_goes_to_the_ladders": {0, 1, 2}}


@pytest.mark.parametrize("name", list(SITUATIONS) + list(CASES))
def test_zero_start_equals_cold_start_on_explicit_zeros(libs, name):
    insts, kw = _batch(name)
    ref = _reference(libs, name)
    if name in SITUATIONS:
        assert {e[1] for e in ref.log} == SITUATIONS[name] and ref.direct == (name == "stage0_solves_all") and ref.n_failed == 0
    else:
        assert max(e[1] for e in ref.log) == max(CASES[name][3]) >= 2 and ref.n_failed == (0 if CASES[name][2] else 1)
    got = Chain(libs["plain"], insts, 2, _garbage(insts), **kw)
    assert got.same_as(ref), (got.log, ref.log)
    assert got.calls == ref.calls


def test_with_a_mask_the_zero_start_is_a_cold_start_that_reads_u(libs):
    insts, kw = _batch("one_goes_to_the_ladders")
    B, n = len(insts), insts[0][0].n
    mask = [1, 0, 1, 1, 0, 1]
    u0 = np.zeros((B, n))
    u0[1], u0[4] = 0.25, -1.5                                                 # theirs to keep
    ref = Chain(libs["plain"], insts, 1, u0, participate=mask, **kw)
    got = Chain(libs["plain"], insts, 2, u0, participate=mask, **kw)          # (the runner checks: told 1, given u)
    assert got.same_as(ref) and got.calls == ref.calls and not got.direct
    full = _reference(libs, "one_goes_to_the_ladders")
    for i in range(B):
        if mask[i]:
            assert got.conv[i] == 1 and np.array_equal(got.u[i], full.u[i])
        else:
            assert got.conv[i] == 0 and np.array_equal(got.u[i], u0[i]) and not any(e[0] == i for e in got.log)


@pytest.mark.parametrize("name", ["one_goes_to_the_ladders", "bi_quadratic", "masked"])
def test_no_row_of_the_end_state_buffer_is_read_before_its_run_wrote_it(libs, name):
    if name == "masked":
        insts, kw = _batch("one_goes_to_the_ladders")
        u0 = np.zeros((len(insts), insts[0][0].n))
        u0[1], u0[4] = 0.25, -1.5
        args = dict(participate=[1, 0, 1, 1, 0, 1], **kw)
        ref = Chain(libs["plain"], insts, 1, u0, **args)
        got = Chain(libs["poison"], insts, 1, u0, **args)
    else:
        insts, kw = _batch(name)
        ref = _reference(libs, name)
        got = Chain(libs["poison"], insts, 2, _garbage(insts), **kw)
    assert got.same_as(ref)
    assert ref.n_failed == 0 and np.all(np.isfinite(got.u))
