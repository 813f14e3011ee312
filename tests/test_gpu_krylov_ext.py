"""MINRES, QMR, CGNR (as written and textbook) and the transposed SpMV on the device, bit for bit against tests/krylov_ext_ref.py in the
library's reduction order (kryst_amd/csrc/minres_qmr_cgnr.hip, transpose.hip)."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import krylov_ext_ref as R

pytestmark = pytest.mark.gpu

CLASSES = {
    "minres": lambda tol, mx: K.MinresSolver(tol, mx),
    "qmr": lambda tol, mx: K.QmrSolver(tol, mx),
    "cgnr": lambda tol, mx: K.CgnrSolver(tol, mx),
    "minres_textbook": lambda tol, mx: K.MinresSolver(tol, mx).with_textbook(),
    "cgnr_textbook": lambda tol, mx: K.CgnrSolver(tol, mx).with_textbook(),
}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    T, V, F = K.reduce_spec()
    return O.Reduce.tiled(T, V, F)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def check(res, st, s, x, nan_ok=False):
    assert st.iterations == res.iterations and st.converged == res.converged
    assert st.final_residual == res.final_residual or (nan_ok and np.isnan(st.final_residual) and np.isnan(res.final_residual))
    assert np.array_equal(np.array(s.residual_history), np.array(res.history, dtype=float), equal_nan=nan_ok)
    assert np.array_equal(x, res.x, equal_nan=nan_ok)


def shifted_poisson(N):
    a = O.stencil7(N, "poisson")
    v = a.vals.copy()
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v[a.col_idx == rows] -= 1.0
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


# ----------------------------------------------------------------------------- transposed SpMV
def _random_csr(g, m, n, density):
    d = g.standard_normal((m, n)) * (g.random((m, n)) < density)
    return O.Csr.from_dense(d, keep_zeros=False)


def test_spmv_transpose_bits(ctx):
    g = np.random.default_rng(11)
    cases = [_random_csr(g, 37, 53, 0.15), _random_csr(g, 300, 120, 0.05), _random_csr(g, 1000, 1000, 0.01)]
    # ragged with empty rows and columns, rectangular
    cases.append(O.Csr(6, 8, [0, 3, 3, 4, 8, 8, 9], [0, 4, 6, 2, 0, 1, 4, 6, 3], g.standard_normal(9)))
    cases += [O.stencil7(10, k) for k in ("poisson", "convdiff", "aniso", "varcoef")]
    for a in cases:
        at = R.transpose(a)
        x = g.standard_normal(a.nrows)
        want = at.spmv(x)
        for make in ("u64", "i32"):
            if make == "u64":
                d = to_dev(ctx, a)
            else:
                d = K.CsrMatrix.from_csr_i32(a.nrows, a.ncols, a.row_ptr, a.col_idx.astype(np.int32), a.vals, ctx=ctx)
            xv = ctx.vec(x)
            y1 = d.spmv_transpose(xv).to_host()
            y2 = d.spmv_transpose(xv).to_host()                 # second call: the cached A^T
            assert np.array_equal(y1, want) and np.array_equal(y2, want)
            assert np.array_equal(d.spmv_transpose(x), want)      # host arrays
    # the generator's stencils: every storage form of A^T (A^T of a symmetric stencil is A)
    for kind in ("poisson", "convdiff", "aniso", "varcoef"):
        for N in (8, 33):
            a = O.stencil7(N, kind)
            d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
            x = np.linspace(-1.0, 2.0, a.nrows)
            assert np.array_equal(d.spmv_transpose(x), R.transpose(a).spmv(x))


def _transpose_bits(ctx, a, g):
    x = g.standard_normal(a.nrows)
    want = R.transpose(a).spmv(x)
    for make in ("u64", "i32"):
        if make == "u64":
            d = to_dev(ctx, a)
        else:
            d = K.CsrMatrix.from_csr_i32(a.nrows, a.ncols, a.row_ptr, a.col_idx.astype(np.int32), a.vals, ctx=ctx)
        y = d.spmv_transpose(ctx.vec(x)).to_host()
        assert y.shape == want.shape and np.array_equal(y.view(np.int64), want.view(np.int64)), make


def test_spmv_transpose_long_columns(ctx):
    """columns of 33, 100 and 5 000 entries: csr_transpose sorts segments longer than 32 by heapsort (one thread per segment), whatever
    order the atomic fill left them in"""
    g = np.random.default_rng(21)
    m = 6000
    lens = [33, 100, 5000, 32, 1, 0, 257]
    rows = np.concatenate([g.choice(m, k, replace=False) for k in lens])
    cols = np.concatenate([np.full(k, c) for c, k in enumerate(lens)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=rp[1:])
    a = O.Csr(m, len(lens), rp, cols, g.standard_normal(len(cols)))
    _transpose_bits(ctx, a, g)


def test_spmv_transpose_more_than_1024_scan_blocks(ctx):
    """3 x 2 200 000 with empty columns at both ends: 1 075 scan blocks of 2 048 columns, so tr_scan_top_kernel's threads take more
    than one block sum each"""
    g = np.random.default_rng(22)
    nc, lo, hi = 2_200_000, 100, 2_200_000 - 100
    r0 = np.arange(lo, hi, 2); r1 = np.arange(lo, hi, 3); r2 = np.sort(g.choice(np.arange(lo, hi), 400_000, replace=False))
    ci = np.concatenate([r0, r1, r2])
    rp = np.array([0, len(r0), len(r0) + len(r1), len(ci)], dtype=np.int64)
    a = O.Csr(3, nc, rp, ci, g.standard_normal(len(ci)))
    _transpose_bits(ctx, a, g)


def test_spmv_transpose_errors(ctx):
    a = O.Csr(3, 5, [0, 2, 3, 4], [0, 4, 1, 2], [1.0, 2.0, 3.0, 4.0])
    d = to_dev(ctx, a)
    with pytest.raises(K.KError) as e:
        d.spmv_transpose(ctx.vec(np.ones(5)))                   # x must have nrows entries
    assert e.value.code == 102
    with pytest.raises(K.KError) as e:
        d.spmv_transpose(ctx.vec(np.ones(3)), ctx.vec(np.ones(3)))   # y must have ncols entries
    assert e.value.code == 102
    assert np.array_equal(d.spmv_transpose(np.array([1.0, 1.0, 1.0])), R.transpose(a).spmv(np.ones(3)))


# ----------------------------------------------------------------------------- the five solvers, bit for bit
@pytest.mark.parametrize("kind,N", [("convdiff", 8), ("poisson", 12), ("aniso", 10)])
@pytest.mark.parametrize("method", list(CLASSES))
def test_bit_exact(ctx, rs, method, kind, N):
    a = O.stencil7(N, kind)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    d = to_dev(ctx, a)
    for tol, mx in ((1e-8, 300), (1e-30, 7), (1e-2, 300)):
        x0 = np.linspace(-1.0, 1.0, a.nrows)
        res = R.SOLVERS[method](a, b, x0, tol, mx, rs)
        s = CLASSES[method](tol, mx)
        xv, bv = ctx.vec(x0), ctx.vec(b)
        st = s.solve(d, K.Jacobi().setup(d), bv, xv)            # pc is ignored by all five
        check(res, st, s, xv.to_host(), nan_ok=method == "cgnr")
    if method in ("minres", "qmr", "cgnr"):                     # host-array form
        x0 = np.linspace(-1.0, 1.0, a.nrows)
        res = R.SOLVERS[method](a, b, x0, 1e-8, 50, rs)
        s = CLASSES[method](1e-8, 50); x = x0.copy()
        check(res, s.solve(d, None, b, x), s, x, nan_ok=method == "cgnr")


def test_breakdowns(ctx, rs):
    # MINRES on the identity: beta_next = 0 at once
    a = O.Csr.from_dense(np.eye(40), keep_zeros=False); d = to_dev(ctx, a)
    b = np.linspace(1.0, 2.0, 40)
    for method in CLASSES:
        res = R.SOLVERS[method](a, b, np.zeros(40), 1e-8, 10, rs)
        s = CLASSES[method](1e-8, 10); xv = ctx.vec(np.zeros(40))
        check(res, s.solve(d, None, ctx.vec(b), xv), s, xv.to_host(), nan_ok=True)
    # b = A x0: beta_1 = 0, rho_0 = 0, CGNR's 0 / 0 (NaNs compared as equal); max_iters = 0
    a = O.stencil7(6, "convdiff"); d = to_dev(ctx, a)
    x0 = np.linspace(-1.0, 1.0, a.nrows); b = a.spmv(x0)
    for method in CLASSES:
        res = R.SOLVERS[method](a, b, x0, 1e-8, 5, rs)
        s = CLASSES[method](1e-8, 5); xv = ctx.vec(x0)
        check(res, s.solve(d, None, ctx.vec(b), xv), s, xv.to_host(), nan_ok=True)
        b2 = a.spmv(np.ones(a.nrows))
        res = R.SOLVERS[method](a, b2, x0, 1e-8, 0, rs)
        s = CLASSES[method](1e-8, 0); xv = ctx.vec(x0)
        check(res, s.solve(d, None, ctx.vec(b2), xv), s, xv.to_host())


def test_kspcontext_and_sessions(ctx, rs):
    a = O.stencil7(8, "convdiff"); d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows)); x0 = np.linspace(-1.0, 1.0, a.nrows)
    for kind, method in ((K.SolverKind.Qmr, "qmr"), (K.SolverKind.Minres, "minres"), (K.SolverKind.Cgnr, "cgnr")):
        x1 = x0.copy(); st1 = K.KspContext(kind, d, None, 1e-8, 40).solve_context(b, x1)
        s = CLASSES[method](1e-8, 40); x2 = x0.copy(); st2 = s.solve(d, None, b, x2)
        assert (st1.iterations, st1.converged) == (st2.iterations, st2.converged)
        assert st1.final_residual == st2.final_residual or np.isnan(st1.final_residual)
        assert np.array_equal(x1, x2, equal_nan=True)
    K_STEPS = 9
    for method in CLASSES:
        res = R.SOLVERS[method](a, b, x0, 1e-30, K_STEPS, rs)
        bv, xv = ctx.vec(b), ctx.vec(x0)
        with K.Session(method, d, None, bv, xv, 1e-30, K_STEPS) as ss:
            ss.step(4); ss.step(K_STEPS - 4)
            st = ss.end()
        assert st.iterations == res.iterations == K_STEPS and st.converged == res.converged
        assert st.final_residual == res.final_residual or np.isnan(res.final_residual)
        assert np.array_equal(np.array(ss.residual_history), np.array(res.history, dtype=float), equal_nan=True)
        assert np.array_equal(xv.to_host(), res.x, equal_nan=True)


def test_cgne_binds_to_cgnr(ctx):
    a = O.stencil7(6, "aniso"); d = to_dev(ctx, a)
    b = a.spmv(np.ones(a.nrows))
    x1 = np.zeros(a.nrows); s1 = K.CgnrSolver(1e-8, 30); st1 = s1.solve(d, None, b, x1)
    x2 = np.zeros(a.nrows); s2 = K.CgneSolver(1e-8, 30); st2 = s2.solve(d, None, b, x2)
    assert st1.iterations == st2.iterations and np.array_equal(x1, x2) and s1.residual_history == s2.residual_history


# ----------------------------------------------------------------------------- textbook properties
def test_minres_textbook_indefinite_32(ctx):
    a = shifted_poisson(32); d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    tol = 1e-8
    s = K.MinresSolver(tol, 2000).with_textbook(); xv = ctx.vec(np.zeros(a.nrows))
    st = s.solve(d, None, ctx.vec(b), xv)
    assert st.converged and st.iterations < 2000
    assert np.linalg.norm(b - a.spmv(xv.to_host())) <= 10 * tol * np.linalg.norm(b)


@pytest.mark.parametrize("N", [8, 12, 24])
def test_minres_textbook_vs_cg(ctx, N):
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    a = O.stencil7(N, "poisson")
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    s = K.MinresSolver(1e-8, 1000).with_textbook(); st = s.solve(d, None, ctx.vec(b), ctx.vec(np.zeros(a.nrows)))
    c = K.CgSolver(1e-8, 1000); sc = c.solve(d, None, ctx.vec(b), ctx.vec(np.zeros(a.nrows)))
    assert st.converged and abs(st.iterations - sc.iterations) <= 2


def test_cgnr_textbook_convdiff_16(ctx):
    a = O.stencil7(16, "convdiff"); d = K.CsrMatrix.stencil7(16, "convdiff", ctx=ctx)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    tol = 1e-8
    s = K.CgnrSolver(tol, 3000).with_textbook(); xv = ctx.vec(np.zeros(a.nrows))
    st = s.solve(d, None, ctx.vec(b), xv)
    assert st.converged and st.iterations < 3000
    assert np.linalg.norm(b - a.spmv(xv.to_host())) <= 10 * tol * np.linalg.norm(b)


@pytest.mark.parametrize("method,kind", [("minres_textbook", "poisson"), ("cgnr_textbook", "convdiff")])
def test_large_128(ctx, rs, method, kind):
    N = 128
    a = O.stencil7(N, kind); d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows)); x0 = np.linspace(-1.0, 1.0, a.nrows)
    res = R.SOLVERS[method](a, b, x0, 1e-30, 20, rs)
    s = CLASSES[method](1e-30, 20); xv = ctx.vec(x0)
    check(res, s.solve(d, None, ctx.vec(b), xv), s, xv.to_host())
