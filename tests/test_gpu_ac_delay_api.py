"""Delayed controlled sources and transmission lines through the product API with solver="gpu": ``ac`` on the delayed buffer, ``ac`` and
``network`` on the line, ``noise`` (one output and a list) and ``network_noise`` on the line between matched noisy resistors -- against the
closed forms of tests/ac_delay_ref.py, in every memory home.  The bound of each figure is 16 x what the dense host path measures against
the same closed form (ac_delay_ref.HOST_MEASURED, re-measured by tests/test_ac_delay_cpu.py) and not below 64 eps.  No system of these
circuits may fall back to the host."""
import numpy as np
import pytest

from cadnip_jl_amd import api
from tests import ac_delay_ref as D

pytestmark = pytest.mark.gpu


class GpuBackend:
    """the product API with a GPU solver; gmin = 0 as in the host measurement"""

    def __init__(self, memory):
        self.memory, self.stats = memory, []

    def _target(self, circ, base, pts):
        mc = api.MNACircuit(circ, dict(base))
        return mc if pts == [{}] else api.CircuitSweep(mc, pts)

    def _list(self, res, pts):
        sols = [res] if pts == [{}] else [res[i] for i in range(len(pts))]
        for s in sols:
            self.stats.append((s if not isinstance(s, dict) else next(iter(s.values()))).stats)
        return sols

    def ac(self, circ, base, pts, freqs):
        return self._list(api.ac(self._target(circ, base, pts), freqs, gmin=0.0, solver="gpu", memory=self.memory), pts)

    def network(self, circ, base, pts, ports, freqs, z0):
        return self._list(api.network(self._target(circ, base, pts), ports, freqs, z0=z0, gmin=0.0, solver="gpu", memory=self.memory), pts)

    def noise(self, circ, base, pts, output, freqs):
        return self._list(api.noise(self._target(circ, base, pts), output, freqs, gmin=0.0, solver="gpu", memory=self.memory), pts)

    def network_noise(self, circ, base, pts, ports, freqs, z0):
        return self._list(api.network_noise(self._target(circ, base, pts), ports, freqs, z0=z0, gmin=0.0, solver="gpu", memory=self.memory), pts)


@pytest.mark.parametrize("memory", ["lds", "hbm", "auto"])
def test_the_gpu_path_meets_the_closed_forms(memory):
    be = GpuBackend(memory)
    got = D.closed_form_errors(be)
    for key, err in got.items():
        print("%s memory %s: gpu path against the closed form %.3g, bound %.3g (host path %.3g)" % (key, memory, err, D.closed_form_bound(key), D.HOST_MEASURED[key]))
    assert len(be.stats) == 1 + 5 * len(D.TL_PTS)
    for st in be.stats:
        assert st["host_systems"] == 0 and st["gpu_systems"] > 0 and st["memory"] == ("hbm" if memory == "hbm" else "lds"), st
    for key, err in got.items():
        assert err <= D.closed_form_bound(key), (key, err)


def test_a_list_of_outputs_is_the_single_output_call():
    mc = api.MNACircuit(D.tline_noise(), {"td": D.TL_TDS[1]})
    one = api.noise(mc, "p2", D.TL_FREQS, gmin=0.0, solver="gpu")
    many = api.noise(mc, ["p1", "p2"], D.TL_FREQS, gmin=0.0, solver="gpu")
    assert np.array_equal(many["p2"]["onoise"], one["onoise"]) and np.array_equal(many["p2"]["ra"], one["ra"])
    assert many["p2"].stats["host_systems"] == 0 and many["p2"].stats["rhs"] == 2
    kt2 = 2.0 * D.KT * D.Z0
    assert np.max(np.abs(many["p1"]["onoise"] - kt2)) <= D.closed_form_bound("tline_noise") * kt2        # the near end: the same by symmetry
