"""csrc/lds_layout.hpp: lds_step_predecode -- the conversion k_fused2 applies to every lane's step descriptor while it stages the step
program -- on the CPU: the header is compiled with the host compiler and fed the flip-flop's and chain17's step programs (f2_build_steps,
through cadnip_host_lu_analyze; no GPU).  For every lane of every step, padding step included: the new 16-bit fields are the byte offsets
of exactly the words the packed 15-bit fields name; a lane that does not lead its group gets its own trash word as its entry; the flag
byte carries the lane's group width, the step's widest group and the division bit unchanged; and every offset fits 16 bits where
lds_steps_predec_ok says so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cadnip_jl_amd import benchmarks as bm, hip
from tests import circuits as tc
from tests.port_util import make_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")

SHIM = r"""
#include "lds_layout.hpp"
using namespace cadnip;
extern "C" {
// words: [lanes][4] packed 32-bit words (x, y, z, w); out: [lanes][5] pre-decoded x, y, z, w, flags
void pd_convert(const unsigned* words, int lanes, int trash0, unsigned* out) {
  for (int i = 0; i < lanes; ++i) {
    const StepPredec p = lds_step_predecode(words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3], (unsigned)(trash0 + (i & 63)));
    out[5 * i] = p.x; out[5 * i + 1] = p.y; out[5 * i + 2] = p.z; out[5 * i + 3] = p.w; out[5 * i + 4] = p.flags;
  }
}
int pd_ok(int lu_words, int n) { return lds_steps_predec_ok(lu_words, n) ? 1 : 0; }
int pd_desc_words(int desc_len, int predec) { return lds_sweep_desc_words(desc_len, predec != 0); }
int pd_trash() { return F2_TRASH; }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_predecode")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    return C.CDLL(so)


def _program(name):
    if name == "dff":
        circ, params = bm.dff_circuit(), {"vdd": 5.0}
    else:
        mk, params = tc.CHAIN_STAMP["chain17"]
        circ = mk()
    st, port = make_port(circ, params)
    u = np.random.default_rng(11).random(st.n) * float(params["vdd"]) * (5.0 if name != "dff" else 1.0)
    G, Cm, b, lw = port.rebuild(u, 2.005e-7)
    port.close()
    return st, G + 1e9 * Cm


@pytest.mark.parametrize("nc", [0, 8])
@pytest.mark.parametrize("name", ["dff", "chain17"])
def test_predecoded_fields_address_the_same_words(lib, name, nc):
    st, J = _program(name)
    P = hip.host_lu_analyze(st.n, np.asarray(st.rowptr), np.asarray(st.colidx), J, f2_nc=nc, leaves=hip.leaves_of(st))
    lu_words = int(P["f2"]["meta"][1])
    (n_pre, n_post, n_fwd), words = P["steps"][1]              # one wave per instance, three terms per lane: what k_fused2 stages
    w32 = np.ascontiguousarray(np.asarray(words, dtype=np.uint64)).view(np.uint32).reshape(-1, 4)
    lanes = w32.shape[0]
    assert lanes == 64 * (n_pre + n_post + n_fwd + 1)          # (the padding step the kernel prefetches)
    assert lib.pd_ok(lu_words, st.n) == 1 and lib.pd_ok(8192 - st.n - 66 + 1, st.n) == 0 and lib.pd_ok(8192 - st.n - 66, st.n) == 1
    assert lib.pd_desc_words(2 * lanes, 0) == 2 * lanes and lib.pd_desc_words(2 * lanes, 1) == 2 * lanes + lanes // 8
    trash0 = lu_words + st.n
    out = np.zeros((lanes, 5), dtype=np.uint32)
    lib.pd_convert(w32.ctypes.data_as(C.c_void_p), lanes, trash0, out.ctypes.data_as(C.c_void_p))
    old = np.stack([w32[:, k // 2] >> (16 * (k % 2)) & 0xFFFF for k in range(8)], axis=1).astype(np.int64)     # entry, pivot, a0, b0, a1, b1, a2, b2
    new = np.stack([out[:, k // 2] >> (16 * (k % 2)) & 0xFFFF for k in range(8)], axis=1).astype(np.int64)
    word, flag = old & 0x7FFF, old >> 15
    lane = np.arange(lanes) & 63
    assert np.all(new % 8 == 0) and np.all(new // 8 < lu_words + st.n + lib.pd_trash() + 2)
    assert np.array_equal(new[:, 1:] // 8, word[:, 1:])                                   # pivot and the six operands: the same words
    leader = flag[:, 0] == 1
    assert np.array_equal(new[leader, 0] // 8, word[leader, 0])                           # a leader's entry: the same word
    assert np.array_equal(new[~leader, 0] // 8, trash0 + lane[~leader])                   # everybody else: the lane's own trash word
    lg = flag[:, 1] | flag[:, 2] << 1 | flag[:, 3] << 2
    maxlg = flag[:, 4] | flag[:, 5] << 1 | flag[:, 6] << 2
    assert np.array_equal(out[:, 4] >> 4, lg) and np.array_equal(out[:, 4] & 7, maxlg) and np.array_equal(out[:, 4] >> 3 & 1, flag[:, 7])
    assert out[:, 4].max() < 256 and leader.sum() > 0 and lg.max() >= 1                   # one byte; the programs have lane groups wider than one
