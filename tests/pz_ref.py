"""References of the pole-zero tests (tests/test_pz_cpu.py, tests/test_gpu_ac_arnoldi.py, tests/test_gpu_pz.py): a numpy port of the algorithm
of k_ac_arnoldi (csrc/ac_lu.hip) -- complex128, np.linalg's LU as the solve, two passes of modified Gram-Schmidt, the kernel's breakdown test --
that also records the norm ratio of every step; the circuits of those tests with their systems on the CPU port; the figures the tests measure
(the breakdown gap, the theta gap, the Arnoldi relation, orthogonality, pole errors).  Nothing here calls cadnip_jl_amd.api's own Arnoldi."""
import numpy as np
import scipy.linalg as sla

import cadnip_jl_amd as cj
from cadnip_jl_amd import api
from tests import ac_ref as R

EPS = R.EPS
GMIN = 1e-12


def rc_ladder(sections, r=1e3, c=1e-9):
    """V - (R - C to ground) x sections: `sections` distinct real poles, no finite zero to the last node."""
    circ = cj.Circuit("rc ladder %d" % sections)
    circ.V("vin", "n0", "0", dc=0.0, ac=1.0)
    for k in range(sections):
        circ.R("r%d" % (k + 1), "n%d" % k, "n%d" % (k + 1), r * (1.0 + 0.25 * k))
        circ.C("c%d" % (k + 1), "n%d" % (k + 1), "0", c / (1.0 + 0.5 * k))
    return circ


def lead_lag():
    """vin - Rs - a - (R1 || C1) - out - R2 - ground, the lead-lag network: one pole -(1 / R1 + 1 / (Rs + R2)) / C1 = -1.009e5 and ONE
    finite zero -1 / (R1 C1) = -1e4.  No capacitor loop and no capacitor across the source: the system has index 1."""
    circ = cj.Circuit("lead-lag")
    circ.V("vin", "in", "0", dc=0.0, ac=1.0)
    circ.R("rs", "in", "a", 1e2)
    circ.R("r1", "a", "out", 1e4)
    circ.C("c1", "a", "out", 1e-8)
    circ.R("r2", "out", "0", 1e3)
    return circ


# name -> (circuit, output node): the linear circuits of the pole-zero tests
LINEAR = {
    "butterworth": (lambda: cj.netlist.read_spice(R.BUTTERWORTH)[0], "vout"),
    "ladder4": (lambda: rc_ladder(4), "n4"),
    "ladder8": (lambda: rc_ladder(8), "n8"),
    "leadlag": (lead_lag, "out"),
}
# the output unknown of the MOS cases of ac_ref.CASES
MOS_OUT = {"inverter": "vout", "dff": "Q_neg"}


def linear_system(name):
    """(st, G dense with gmin on the node diagonals, C dense, b_ac, c = e_out) of a LINEAR circuit, on the CPU port at the zero state."""
    from tests.port_util import make_port, analyze_port
    mk, out = LINEAR[name]
    circ = mk()
    st, port = make_port(circ, {}, 27.0, "dcop")
    analyze_port(st, port, 1.0)
    G, C, _, _ = port.rebuild(np.zeros(st.n), 0.0)
    port.close()
    c = np.zeros(st.n)
    c[st.index_of(out)] = 1.0
    return st, R.system(st, G, C, 0.0, GMIN).real, R.dense_csr(st, np.asarray(C, dtype=float)), api.rhs_ac(st, circ, {}), c


def arnoldi_port(G, C, b, w0, m, tol, c=None):
    """The kernel's algorithm in numpy for one system.  Returns dict(H [m+1, m], beta, m_eff, l [m, P], V [m+1, n], flag, ratios): ratios[j]
    = nu_1 / nu_0 of step j, for every step made (the breakdown step included)."""
    n = len(b)
    A = np.asarray(G) + 1j * w0 * np.asarray(C)
    lu = sla.lu_factor(A)
    cc = np.zeros((0, n)) if c is None else np.asarray(c, dtype=complex).reshape(-1, n)
    H, V, l = np.zeros((m + 1, m), complex), np.zeros((m + 1, n), complex), np.zeros((m, cc.shape[0]), complex)
    r = sla.lu_solve(lu, np.asarray(b, dtype=complex))
    beta = float(np.linalg.norm(r))
    out = dict(H=H, beta=beta, m_eff=0, l=l, V=V, flag=0, ratios=[])
    if not (beta > 0 and np.isfinite(beta)):
        out["flag"] = 2
        return out
    V[0] = r / beta
    l[0] = cc @ V[0]
    out["m_eff"] = m
    for j in range(m):
        w = sla.lu_solve(lu, np.asarray(C) @ V[j])
        nu0 = np.linalg.norm(w)
        for _ in range(2):
            for i in range(j + 1):
                h = np.vdot(V[i], w)
                w = w - h * V[i]
                H[i, j] += h
        nu1 = np.linalg.norm(w)
        out["ratios"].append(nu1 / nu0 if nu0 > 0 else 0.0)
        if nu0 == 0 or nu1 <= tol * nu0:
            out["m_eff"], out["flag"] = j + 1, 4
            break
        H[j + 1, j] = nu1
        V[j + 1] = w / nu1
        if j + 1 < m:
            l[j + 1] = cc @ V[j + 1]
    return out


def krylov_dimension(G, C, b, w0, m):
    """The dimension of span{r, K r, ..., K^m r}, K = A^-1 C, r = A^-1 b, from the dense pencil, without any orthogonalisation: the distinct
    finite eigenvalues p of (-G, C) whose left eigenvector y sees the excitation (y^H b != 0: the pole has a residue in (G + s C)^-1 b), plus
    the length of the chain r_N, K r_N, ... of the rest of r, which lies in the generalised null space of K (the infinite eigenvalues: K is
    nilpotent there, and the chain ends after as many steps as the differentiation index of the excitation's path)."""
    G, C = np.asarray(G, dtype=float), np.asarray(C, dtype=float)
    A = G + 1j * w0 * C
    r = np.linalg.solve(A, np.asarray(b, dtype=complex))
    K = np.linalg.solve(A, C.astype(complex))
    n0, n1 = np.linalg.norm(G), np.linalg.norm(C)
    ab, Y, X = sla.eig(-G / n0, C / n1, left=True, right=True, homogeneous_eigvals=True)
    fin = np.abs(ab[1]) > 1e-9 * np.abs(ab[0])
    rN, reached = r.copy(), []
    for k in np.flatnonzero(fin):
        p = ab[0][k] / ab[1][k] * (n0 / n1)
        x, z = X[:, k], Y[:, k].conj() @ A                      # z K = theta z, theta = 1 / (j w0 - p)
        comp = (z @ r) / (z @ x)
        if abs(comp) * np.linalg.norm(x) > 1e-9 * np.linalg.norm(r):
            rN = rN - comp * x
            if not any(abs(p - q) <= 1e-6 * abs(q) for q in reached):
                reached.append(p)
    chain, v, kn = 0, rN, np.linalg.norm(K, 2)
    scale = np.linalg.norm(r)
    while chain < len(b) and np.linalg.norm(v) > 1e-9 * scale:
        chain, scale, v = chain + 1, kn * np.linalg.norm(v), K @ v
    return min(len(reached) + chain, m + 1)


def relation_error(G, C, w0, H, V, m_eff):
    """The componentwise Arnoldi-relation figure max |A V_{m_eff+1} Hbar - C V_{m_eff}| / (|A| |V| |Hbar| + |C| |V|), 0 / 0 = 0, in long double."""
    CLD = R.CLD
    A = (np.asarray(G) + 1j * w0 * np.asarray(C)).astype(CLD)
    Cl = np.asarray(C).astype(CLD)
    Vt, Hb = V[:m_eff + 1].T.astype(CLD), H[:m_eff + 1, :m_eff].astype(CLD)
    num = np.abs(A @ (Vt @ Hb) - Cl @ Vt[:, :m_eff])
    den = np.abs(A) @ (np.abs(Vt) @ np.abs(Hb)) + np.abs(Cl) @ np.abs(Vt[:, :m_eff])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(num == 0, np.longdouble(0), num / den)
    return float(np.max(q)) if q.size else 0.0


def orthogonality_error(V, nvec):
    Q = V[:nvec]
    return float(np.max(np.abs(Q.conj() @ Q.T - np.eye(nvec)))) if nvec else 0.0


def n_vectors(m, m_eff, flag):
    """rows of V that hold a vector: m_eff after a breakdown (v_{m_eff} does not exist), m + 1 without, 0 when beta was refused"""
    return 0 if flag & 2 else m_eff if flag & 4 else m + 1


def match_error(found, ref, w0=None):
    """per found pole: the distance to the nearest reference pole relative to |p - j w0| (w0 [len(found)] or a scalar; None: relative to |p|)"""
    found, ref = np.asarray(found, dtype=complex), np.asarray(ref, dtype=complex)
    if found.size == 0:
        return np.zeros(0)
    d = np.min(np.abs(found[:, None] - ref[None, :]), axis=1)
    base = np.abs(found - (0.0 if w0 is None else 1j * np.asarray(w0, dtype=float)))
    return d / base
