"""References of the sensitivity tests (tests/test_sensitivity_cpu.py, tests/test_gpu_ac_sens.py, tests/test_gpu_sensitivity.py): the DIRECT
form of the derivative of y = e^T x, A x = b -- dy/dp = e^T A^-1 (db - dA x), one extended-precision solve per parameter -- which the adjoint
form lambda^T (db - dA x) of api.sensitivity_solve and of k_ac_sens (csrc/ac_lu.hip) must reproduce, the bound d_s that holds the two
together, and the systems of tests/ac_ref.py at arbitrary points on the CPU port."""
import numpy as np

from cadnip_jl_amd import api
from tests import ac_ref as R

EPS = R.EPS
CLD = R.CLD


def e_pair(n, pair):
    e = np.zeros(n, dtype=complex)
    for j, sgn in zip(pair, (1.0, -1.0)):
        if j >= 0:
            e[j] += sgn
    return e


def direct_form(A, b, dA, db, pair):
    """(s [K], x_ref, lambda_ref, w [K, n]): s_k = e^T refined_solve_c(A, w_k), w_k = db_k - dA_k x_ref, with x_ref and lambda_ref refined
    dense solves of A x = b and A^T lambda = e.  The products with dA run in complex long double."""
    n = A.shape[0]
    e = e_pair(n, pair)
    x = R.refined_solve_c(A, b)
    lam = R.refined_solve_c(A.T, e)
    K = len(dA)
    w = np.zeros((K, n), dtype=complex)
    s = np.zeros(K, dtype=complex)
    for k in range(K):
        wl = -(np.asarray(dA[k]).astype(CLD) @ x.astype(CLD))
        if db is not None:
            wl = wl + np.asarray(db[k]).astype(CLD)
        w[k] = wl.astype(complex)
        s[k] = complex((e.astype(CLD) @ R.refined_solve_c(A, w[k]).astype(CLD)))
    return s, x, lam, w


def d_s(A, x, lam, dA_k, w_k):
    """The bound on |s_adjoint - s_direct| of one column, from the forward bounds this project holds its solves to (tests/test_gpu_ac_lu.py,
    tests/test_gpu_ac_adjoint.py): d_x = 16 cond_inf(A) eps max|x| on every component of x, d_lambda = 16 cond_inf(A^T) eps max|lambda| on
    every component of lambda.  s = lambda^T w with w = db - dA x:  an error of d_lambda per lambda_i moves s by at most d_lambda sum|w|, an
    error of d_x per x_j by at most d_x sum_i |lambda_i| sum_j |dA_ij|, and the two sums of products themselves -- n-term dot products, the
    rows of dA x and the final one, in another order than the reference's -- by 16 n eps sum_i |lambda_i| |w_i|."""
    n = A.shape[0]
    d_x = 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(x))
    d_lam = 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(lam))
    absw = np.abs(w_k)
    return d_lam * np.sum(absw) + d_x * np.sum(np.abs(lam) * np.sum(np.abs(dA_k), axis=1)) + 16 * n * EPS * np.sum(np.abs(lam) * absw)


def port_points(name, points):
    """ac_ref.port_case at arbitrary points of the case's circuit: (st, G [B, nnz], C [B, nnz], b_ac [B, n], u [B, n]) on the CPU port, CSR
    order, each point a cold DC solve of its own."""
    from tests.port_util import make_port, analyze_port
    mk, base, _, _ = R.CASES[name]
    circ = mk()
    Gs, Cs, bs, us, st = [], [], [], [], None
    for pt in points:
        p = dict(base)
        p.update({k: v for k, v in pt.items() if k != "temp"})
        st, port = make_port(circ, p, pt.get("temp", 27.0), "dcop")
        vs = [abs(float(v)) for v in p.values()] + [abs(float(d.params["dc"])) for d in circ.devices
                                                    if d.type == "V" and not hasattr(d.params.get("dc", 0.0), "name")] + [1.0]
        analyze_port(st, port, max(vs))
        u, ok, _ = port.dc(abstol=1e-13)
        assert ok, (name, pt)
        G, C, _, _ = port.rebuild(u, 0.0)
        port.close()
        Gs.append(G), Cs.append(C), bs.append(api.rhs_ac(st, circ, p)), us.append(u)
    return st, np.array(Gs), np.array(Cs), np.array(bs), np.array(us)


def dense_G(st, G_csr, gmin):
    G = R.dense_csr(st, np.asarray(G_csr, dtype=float))
    G[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
    return G
