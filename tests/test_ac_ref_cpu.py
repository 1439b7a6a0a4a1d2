"""Host-only checks of the AC sweep's references (tests/ac_ref.py) and of the product's merge logic (api.ac_gpu_sweep) with a stub in place of
the GPU handle: the refined dense reference against the Butterworth filter's transfer function, reference and static-order solve against each
other on the CPU port's inverter and flip-flop systems, the backward-error function's sensitivity, the measurement behind api.AC_BERR_MAX."""
import numpy as np
import pytest

from cadnip_jl_amd import api, hip
from tests import ac_ref as R

EPS = R.EPS
GMIN = 1e-12
_CASE = {}


def case(name):
    if name not in _CASE:
        st, G, C, bac, om = R.port_case(name)
        rp, cp = R.order_of(st, R.pivot_sample(st, G, C, om, GMIN))
        _CASE[name] = (st, G, C, bac, om, rp, cp)
    return _CASE[name]


def test_reference_reproduces_the_butterworth_transfer_function():
    st, G, C, bac, om, rp, cp = case("butterworth")
    H = R.butterworth_h(om)
    vout = st.index_of("vout")
    # gmin = 0: the transfer function knows no shunt conductances (1e-12 S on the 1 ohm nodes is a 2e-12 relative change of the response)
    for solve in (lambda A, b: R.refined_solve_c(A, b), lambda A, b: R.static_order_solve_c(A, b, rp, cp)):
        got = np.array([solve(R.system(st, G[0], C[0], w, 0.0), bac[0])[vout] for w in om])
        assert np.max(np.abs(got - H) / np.abs(H)) <= 1e-12


@pytest.mark.parametrize("name", ["inverter", "dff"])
def test_reference_and_static_order_solve_agree_on_the_port_matrices(name):
    st, G, C, bac, om, rp, cp = case(name)
    for b in range(G.shape[0]):
        for w in om[:: max(1, len(om) // 7)]:
            A = R.system(st, G[b], C[b], w, GMIN)
            xr, xs = R.refined_solve_c(A, bac[b]), R.static_order_solve_c(A, bac[b], rp, cp)
            assert R.backward_error_c(A, xr, bac[b]) <= 4 * EPS
            assert R.backward_error_c(A, xs, bac[b]) <= api.AC_BERR_MAX / 16        # no system of these cases is exempt from the forward check
            assert np.max(np.abs(xs - xr)) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xr))


def test_backward_error_rejects_a_perturbed_entry():
    st, G, C, bac, om, rp, cp = case("butterworth")
    A = R.system(st, G[0], C[0], om[30], GMIN)
    x = R.refined_solve_c(A, bac[0])
    assert R.backward_error_c(A, x, bac[0]) <= 4 * EPS
    k = int(np.argmax(np.abs(x)))
    y = x.copy()
    y[k] *= 1.0 + 1e-9
    assert R.backward_error_c(A, y, bac[0]) > 1e-10
    assert R.backward_error_c(np.zeros((2, 2)), np.zeros(2), np.zeros(2)) == 0.0         # 0 / 0 = 0


def test_ac_berr_max_is_sixteen_times_the_dense_solve_s_own_backward_error():
    """The measurement api.AC_BERR_MAX states: the largest componentwise backward error np.linalg.solve leaves over the systems of the test
    circuits, times 16, not below 64 eps."""
    worst = 0.0
    for name in R.CASES:
        st, G, C, bac, om, _, _ = case(name)
        for b in range(G.shape[0]):
            for w in om:
                A = R.system(st, G[b], C[b], w, GMIN)
                worst = max(worst, R.backward_error_c(A, np.linalg.solve(A, bac[b]), bac[b]))
    assert api.AC_BERR_MAX == max(16 * round(worst, 2), 64 * EPS), worst


class StubHandle:
    """Handle.analyze_values / ac_solve of the merge test: the static-order CPU solve, with chosen rows spoiled."""

    def __init__(self, st, G, C, rp_cp, spoil, fit=True):
        self.st, self.G, self.C, self.order, self.spoil, self.fit, self.samples, self.calls = st, G, C, rp_cp, spoil, fit, [], 0

    def analyze_values(self, sample_ref):
        self.samples.append(np.asarray(sample_ref)[self.st.to_ref_nz])

    def ac_solve(self, omega, gmin, b_ac, wpb=0):
        self.calls += 1
        if not self.fit:
            raise hip.CadnipError(hip.BADARG, "cadnip_ac_solve")
        B, F, n = len(self.G), len(omega), self.st.n
        x, berr, flags = np.zeros((B, F, n), complex), np.zeros((B, F)), np.zeros((B, F), dtype=np.int32)
        for b in range(B):
            for f, w in enumerate(omega):
                A = R.system(self.st, self.G[b], self.C[b], w, gmin)
                x[b, f] = R.static_order_solve_c(A, b_ac[b], *self.order)
                berr[b, f] = R.backward_error_c(A, x[b, f], b_ac[b])
        for (b, f), kind in self.spoil.items():
            x[b, f] = 123.0
            if kind == "flag":
                flags[b, f] = 1
            elif kind == "nan":
                berr[b, f] = np.nan
            else:
                berr[b, f] = 2 * api.AC_BERR_MAX
        return x, berr, flags, dict(wpb=4, lds_bytes=0, systems=B * F, workgroups=0)


def _sols(st, G, C, bac, freqs):
    to_ref = np.asarray(st.to_ref_nz)
    G_ref, C_ref = np.empty_like(G), np.empty_like(C)
    G_ref[:, to_ref], C_ref[:, to_ref] = G, C
    sols = []
    for b in range(len(G)):
        Gd = R.dense_csr(st, G[b])
        Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += GMIN
        sols.append(api.ACSol(st, Gd, R.dense_csr(st, C[b]), bac[b], np.zeros(st.n), freqs))
    return sols, G_ref, C_ref


def test_merge_keeps_gpu_rows_and_replaces_flagged_ones_by_the_host_solve():
    st, G, C, bac, om, rp, cp = case("inverter")
    freqs = om[:5] / (2 * np.pi)
    omegas = 2.0 * np.pi * freqs
    spoil = {(0, 1): "flag", (1, 0): "berr", (2, 4): "nan"}
    stub = StubHandle(st, G, C, (rp, cp), spoil)
    sols, G_ref, C_ref = _sols(st, G, C, bac, freqs)
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
    api.ac_gpu_sweep(stub, st, sols, G_ref, C_ref, omegas, GMIN, "gpu", stats)
    assert stub.calls == 1 and np.array_equal(stub.samples[0], R.pivot_sample(st, G, C, omegas, GMIN))
    assert stats["gpu_systems"] == 12 and stats["host_systems"] == 3 and stats["wpb"] == 4 and 0 < stats["max_berr"] <= 4 * EPS
    vout = st.index_of("vout")
    for b, s in enumerate(sols):
        assert list(s._cache) == [tuple(omegas)]
        got = s["vout"]
        for f, w in enumerate(omegas):
            A = s.G + 1j * w * s.C
            if (b, f) in spoil:
                assert got[f] == np.linalg.solve(A, s.b_ac)[vout]                         # the host row, bit for bit
            else:
                assert got[f] == R.static_order_solve_c(A, s.b_ac, rp, cp)[vout]          # the stub's row, untouched
        assert np.array_equal(s.magnitude_db("vout"), 20.0 * np.log10(np.abs(got)))
        other = s.freqresp("vout", [3.0])                                                 # another frequency: the host, and a second cache entry
        assert other[0] == np.linalg.solve(s.G + 3.0j * s.C, s.b_ac)[vout] and len(s._cache) == 2


def test_merge_when_the_circuit_does_not_fit_and_on_an_empty_grid():
    st, G, C, bac, om, rp, cp = case("inverter")
    freqs = om[:2] / (2 * np.pi)
    omegas = 2.0 * np.pi * freqs
    sols, G_ref, C_ref = _sols(st, G, C, bac, freqs)
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
    api.ac_gpu_sweep(StubHandle(st, G, C, (rp, cp), {}, fit=False), st, sols, G_ref, C_ref, omegas, GMIN, "auto", stats)
    assert stats["gpu_systems"] == 0 and stats["host_systems"] == 6 and "fallback" in stats and all(not s._cache for s in sols)
    assert sols[0]["vout"][0] == np.linalg.solve(sols[0].G + 1j * omegas[0] * sols[0].C, sols[0].b_ac)[st.index_of("vout")]
    with pytest.raises(hip.CadnipError):
        api.ac_gpu_sweep(StubHandle(st, G, C, (rp, cp), {}, fit=False), st, sols, G_ref, C_ref, omegas, GMIN, "gpu", dict(stats))
    stub = StubHandle(st, G, C, (rp, cp), {})
    empty, _, _ = _sols(st, G, C, bac, ())
    api.ac_gpu_sweep(stub, st, empty, G_ref, C_ref, np.zeros(0), GMIN, "gpu", stats)
    assert stub.calls == 0 and not stub.samples and len(empty[0]["vout"]) == 0                # an empty grid launches nothing
    with pytest.raises(ValueError):
        api.ac(None, solver="fpga")
