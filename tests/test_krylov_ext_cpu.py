"""MINRES, QMR and CGNR on the host (no GPU): the numpy restatements of tests/krylov_ext_ref.py against plain line-by-line
transliterations of src/solver/minres.rs:60-219, qmr.rs:61-166 and cgnr.rs:77-208 (serial inner products, bit for bit), the reference's
behaviour as written pinned, the textbook extensions' convergence, and the host transpose's order contract."""
import math

import numpy as np
import pytest

from oracle import oracle as O
import krylov_ext_ref as R

SER = O.Reduce.serial()


# ----------------------------------------------------------------------------- line-by-line transliterations (Python floats)
def _mv(a, x):
    y = []
    for i in range(a.nrows):
        s = 0.0
        for k in range(int(a.row_ptr[i]), int(a.row_ptr[i + 1])):
            s = s + float(a.vals[k]) * x[int(a.col_idx[k])]
        y.append(s)
    return y


def _dot(x, y):
    acc = 0.0
    for u, v in zip(x, y):
        acc = acc + u * v
    return acc


def _norm(x):
    return math.sqrt(_dot(x, x))


def _check(res, res0, i, tol, mx):
    rel = res / res0 if res0 != 0.0 else (math.nan if res == 0.0 or res != res else math.copysign(math.inf, res))
    return rel <= tol or i >= mx


def t_minres(a, b, x, tol, mx):
    n = len(b)
    r = _mv(a, x)
    r = [b[i] - r[i] for i in range(n)]
    beta1 = _norm(r)
    if beta1 == 0.0:
        return [0.0] * n, 0, True, beta1, []
    v_prev = [0.0] * n; v = [ri / beta1 for ri in r]; w_prev = [0.0] * n; w = [0.0] * n
    x_out = [0.0] * n; x_best = list(x_out); phi_min = abs(beta1)
    beta = beta1; c_prev = 1.0; s_prev = 0.0; rho_bar = beta1; phi = beta1
    st = (0, beta1, False); hist = []
    for j in range(1, mx + 1):
        v_next = _mv(a, v)
        alpha = _dot(v, v_next)
        v_next = [v_next[i] - alpha * v[i] - beta * v_prev[i] for i in range(n)]
        beta_next = _norm(v_next)
        if beta_next == 0.0:
            break
        v_next = [q / beta_next for q in v_next]
        delta, epsilon = (0.0, 0.0) if j == 1 else (s_prev * beta, -c_prev * beta)
        rho = math.sqrt(rho_bar * rho_bar + alpha * alpha)
        c = rho_bar / rho if rho != 0.0 else 1.0
        s = alpha / rho if rho != 0.0 else 0.0
        phi_next = c * phi; phi_bar = -s * phi
        if rho == 0.0:
            break                                            # (x_out's update is never returned)
        w_new = [v[i] / rho for i in range(n)] if j == 1 else [(v[i] - delta * w[i] - epsilon * w_prev[i]) / rho for i in range(n)]
        x_out = [x_out[i] + phi_next * w_new[i] for i in range(n)]
        w_prev = w; w = w_new; v_prev = v; v = v_next
        beta = beta_next; phi = phi_next; rho_bar = -s * beta_next; c_prev = c; s_prev = s
        if abs(phi_bar) < phi_min:
            phi_min = abs(phi_bar); x_best = list(x_out)
        hist.append(abs(phi_bar))
        stop = _check(abs(phi_bar), beta1, j, tol, mx)
        st = (j, abs(phi_bar), stop)
        if stop:
            break
    return x_best, st[0], st[2], phi_min, hist


def t_qmr(a, b, x, tol, mx):
    n = len(b)
    r = _mv(a, x)
    r = [b[i] - r[i] for i in range(n)]
    r_tld = list(r); x_j = list(x)
    norm_r0 = _norm(r)
    st = [0, norm_r0, False]; hist = []
    rho = _dot(r_tld, r)
    if rho == 0.0:
        return x_j, 0, True, _norm(r), []
    res_norm = norm_r0
    p = p_tld = None
    for j in range(mx):
        if j == 0:
            p = list(r); p_tld = list(r_tld)
        else:
            rho_prev = rho
            rho = _dot(r_tld, r)
            if rho == 0.0:
                break
            beta = rho / rho_prev
            p = [r[i] + beta * p[i] for i in range(n)]
            p_tld = [r_tld[i] + beta * p_tld[i] for i in range(n)]
        v = _mv(a, p)
        sigma = _dot(p_tld, v)
        if sigma == 0.0:
            break
        alpha = rho / sigma
        s = [r[i] - alpha * v[i] for i in range(n)]
        t = _mv(a, s)
        tds = _dot(t, s); tdt = _dot(t, t)
        omega = tds / tdt if tdt != 0.0 else 0.0
        x_j = [x_j[i] + alpha * p[i] + omega * s[i] for i in range(n)]
        r = [s[i] - omega * t[i] for i in range(n)]
        t = _mv(a, x_j)
        t = [b[i] - t[i] for i in range(n)]
        res_norm = _norm(t)
        hist.append(res_norm)
        stop = _check(res_norm, norm_r0, j + 1, tol, mx)
        st = [j + 1, res_norm, stop]
        if stop:
            return x_j, j + 1, True, res_norm, hist
    return x_j, st[0], st[2], res_norm, hist


def t_cgnr(a, b, x, tol, mx, cgne=False):
    n = len(b)
    xk = list(x)
    tmp = _mv(a, xk)
    r = [b[i] - tmp[i] for i in range(n)]
    z = _mv(a, r)
    p = list(z)
    rz = _dot(z, z)
    res0 = _norm(r)
    st = (0, res0, False); hist = []
    for i in range(1, mx + 1):
        ap = _mv(a, p)                                       # CGNE: at_p
        at_ap = _mv(a, ap)                                   # CGNE: ap
        den = _dot(at_ap, at_ap)
        alpha = rz / den if den != 0.0 else (math.nan if rz == 0.0 or rz != rz else math.copysign(math.inf, rz))
        xk = [xk[k] + alpha * p[k] for k in range(n)]
        r = [r[k] - alpha * ap[k] for k in range(n)]
        z = _mv(a, r)
        rz_new = _dot(z, z)
        res_norm = _norm(r)
        hist.append(res_norm)
        stop = _check(res_norm, res0, i, tol, mx)
        st = (i, res_norm, stop)
        if stop:
            break
        beta = rz_new / rz
        p = [z[k] + beta * p[k] for k in range(n)]
        rz = rz_new
    return xk, st[0], st[2], st[1], hist


def _same(res, t):
    x, it, conv, fin, hist = t
    assert res.iterations == it and res.converged == conv
    assert float(res.final_residual) == fin or (math.isnan(fin) and math.isnan(res.final_residual))
    assert np.array_equal(np.array(res.history, dtype=float), np.array(hist, dtype=float), equal_nan=True)
    assert np.array_equal(res.x, np.array(x, dtype=float), equal_nan=True)


def _small_cases():
    rng = np.random.default_rng(7)
    nonsym = rng.standard_normal((12, 12)) + 6.0 * np.eye(12)
    sym = nonsym + nonsym.T
    return [("tridiag", O.Csr.from_dense(O.tridiag(10, -1.0, 2.0, -1.0), keep_zeros=False)),
            ("sym", O.Csr.from_dense(sym, keep_zeros=False)),
            ("nonsym", O.Csr.from_dense(nonsym, keep_zeros=False)),
            ("convdiff", O.stencil7(3, "convdiff"))]


@pytest.mark.parametrize("name,a", _small_cases())
@pytest.mark.parametrize("method", ["minres", "qmr", "cgnr"])
def test_restatement_matches_transliteration(method, name, a):
    n = a.nrows
    b = a.spmv(np.linspace(0.5, 1.5, n))
    fn = {"minres": t_minres, "qmr": t_qmr, "cgnr": t_cgnr}[method]
    for tol, mx in ((1e-8, 60), (1e-30, 7), (1e-2, 60), (1e-8, 0)):
        x0 = np.linspace(-1.0, 1.0, n)
        res = R.SOLVERS[method](a, b, x0, tol, mx, SER)
        _same(res, fn(a, list(b), list(x0), tol, mx))
    # b = A x0: beta_1 = 0 (MINRES), rho_0 = 0 (QMR), 0 / 0 (CGNR)
    x0 = np.linspace(-1.0, 1.0, n)
    bb = a.spmv(x0)
    _same(R.SOLVERS[method](a, bb, x0, 1e-8, 5, SER), fn(a, list(bb), list(x0), 1e-8, 5))


def test_cgne_is_cgnr():
    a = O.Csr.from_dense(O.tridiag(10, -1.0, 2.0, -1.0), keep_zeros=False)
    b = a.spmv(np.linspace(0.5, 1.5, 10))
    _same(R.cgnr(a, b, np.zeros(10), 1e-8, 40, SER), t_cgnr(a, list(b), [0.0] * 10, 1e-8, 40, cgne=True))


def test_minres_identity_breakdown():
    a = O.Csr.from_dense(np.eye(6), keep_zeros=False)
    b = np.arange(1.0, 7.0)
    res = R.minres(a, b, np.zeros(6), 1e-8, 10, SER)
    assert res.iterations == 0 and not res.converged and res.history == []     # beta_next == 0 before stats is touched
    assert np.array_equal(res.x, np.zeros(6))                                   # x_best never moved
    _same(res, t_minres(a, list(b), [0.0] * 6, 1e-8, 10))


def test_minres_as_written_estimate_is_not_the_residual():
    # minres.rs: |phi_bar| reaches the tolerance while the true residual stays near ||b|| (1-D Laplacian)
    for n in (50, 400):
        a = O.Csr.from_dense(O.tridiag(n, -1.0, 2.0, -1.0), keep_zeros=False)
        b = np.ones(n)
        res = R.minres(a, b, np.zeros(n), 1e-8, 2 * n, SER)
        assert res.converged and res.final_residual <= 1e-8 * np.linalg.norm(b)
        true_rel = np.linalg.norm(b - a.spmv(res.x)) / np.linalg.norm(b)
        assert true_rel > 0.5


def test_cgnr_as_written_does_not_converge():
    n = 50
    a = O.Csr.from_dense(O.tridiag(n, -1.0, 2.0, -1.0), keep_zeros=False)
    b = np.ones(n)
    res = R.cgnr(a, b, np.zeros(n), 1e-8, 500, SER)
    assert res.iterations == 500                              # the cap: reported converged, like Convergence::check
    assert np.linalg.norm(b - a.spmv(res.x)) > 1e-3 * np.linalg.norm(b)


def _shifted_poisson(N):
    a = O.stencil7(N, "poisson")
    v = a.vals.copy()
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v[a.col_idx == rows] -= 1.0                                   # Poisson - I: symmetric indefinite
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


def test_minres_textbook_converges_on_indefinite():
    a = _shifted_poisson(8)
    ev = np.linalg.eigvalsh(a.to_dense())
    assert ev[0] < 0.0 < ev[-1]
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    tol = 1e-8
    res = R.minres_textbook(a, b, np.zeros(a.nrows), tol, 300, SER)
    assert res.converged and res.iterations < 300
    assert np.linalg.norm(b - a.spmv(res.x)) <= 10 * tol * np.linalg.norm(b)
    # |phi_bar| is the true residual norm up to rounding
    assert abs(res.final_residual - np.linalg.norm(b - a.spmv(res.x))) <= 1e-6 * np.linalg.norm(b)


def test_minres_textbook_identity_is_exact():
    a = O.Csr.from_dense(np.eye(6), keep_zeros=False)
    b = np.arange(1.0, 7.0)
    res = R.minres_textbook(a, b, np.zeros(6), 1e-30, 10, SER)
    assert res.iterations == 1 and res.converged and res.final_residual == 0.0
    assert np.allclose(res.x, b, rtol=1e-15, atol=0)


def test_cgnr_textbook_converges_on_convdiff():
    a = O.stencil7(8, "convdiff")
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    tol = 1e-8
    res = R.cgnr(a, b, np.zeros(a.nrows), tol, 1000, SER, textbook=True)
    assert res.converged and res.iterations < 1000
    assert np.linalg.norm(b - a.spmv(res.x)) <= 10 * tol * np.linalg.norm(b)


def _dense_t(a):
    d = np.zeros((a.ncols, a.nrows))
    for i in range(a.nrows):
        for k in range(a.row_ptr[i], a.row_ptr[i + 1]):
            d[a.col_idx[k], i] += a.vals[k]
    return d


def test_transpose_order_contract():
    rng = np.random.default_rng(3)
    # ragged rows, empty rows and columns, a rectangular shape
    rp = np.array([0, 3, 3, 4, 8, 8, 9], dtype=np.int64)
    ci = np.array([0, 4, 6, 2, 0, 1, 4, 6, 3], dtype=np.int64)
    va = rng.standard_normal(9)
    a = O.Csr(6, 8, rp, ci, va)
    t = R.transpose(a)
    assert (t.nrows, t.ncols) == (8, 6)
    assert np.array_equal(t.row_ptr, [0, 2, 3, 4, 5, 7, 7, 9, 9])
    assert np.array_equal(t.col_idx, [0, 3, 3, 2, 5, 0, 3, 0, 3])
    assert np.array_equal(t.vals, va[[0, 4, 5, 3, 8, 1, 6, 2, 7]])
    assert np.array_equal(t.to_dense(), a.to_dense().T)
    # unsorted rows and duplicate entries: ascending row, then the row's stored order
    rp = np.array([0, 3, 5], dtype=np.int64)
    ci = np.array([2, 0, 2, 1, 0], dtype=np.int64)
    va = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    u = O.Csr(2, 3, rp, ci, va, check=False)
    tu = R.transpose(u)
    assert np.array_equal(tu.row_ptr, [0, 2, 3, 5])
    assert np.array_equal(tu.col_idx, [0, 1, 1, 0, 0])
    assert np.array_equal(tu.vals, [2.0, 5.0, 4.0, 1.0, 3.0])
    assert np.array_equal(_dense_t(u), np.array([[2.0, 5.0], [0.0, 4.0], [4.0, 0.0]]))
    # random matrices: A^T x by the transpose equals the column sums in ascending row order, bit for bit
    for seed in range(5):
        g = np.random.default_rng(seed)
        m, n = int(g.integers(1, 40)), int(g.integers(1, 40))
        d = g.standard_normal((m, n)) * (g.random((m, n)) < 0.2)
        a = O.Csr.from_dense(d, keep_zeros=False)
        x = g.standard_normal(m)
        y = R.transpose(a).spmv(x)
        ref = np.zeros(n)
        for j in range(n):
            s = 0.0
            for i in range(m):
                if d[i, j] != 0.0:
                    s = s + d[i, j] * x[i]
            ref[j] = s
        assert np.array_equal(y, ref)
