"""DenseMatrix, LuSolver and QrSolver on the GPU against the numpy restatement of DESIGN.md section 4.12 (tests/dense_ref.py), bit for bit."""
import os
import subprocess
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import dense_ref as R
import dense_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, TAIL, TILE = 4096, 128, 256                       # what kryst_lu_info must report (test_info_reports_the_thresholds)
SIZES = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 257, 300, 1024)
THRESHOLD_SIZES = (TAIL - 1, TAIL, TAIL + 1, TILE - 1, TILE, TILE + 1,        # n at the thresholds ...
                   TAIL + TILE, TAIL + TILE + 1, TAIL + TILE + 2)             # ... and the first trailing block (n - 1 rows) at the tile edge
LU_SIZES = tuple(sorted(set(SIZES + THRESHOLD_SIZES)))
QR_SIZES = tuple(n for n in LU_SIZES if n <= 300 + 1) + (385, 1024)


def _families(n):
    """Every family up to the threshold sizes.  At 1024 the restatement costs 6 s per matrix on the host, so three families there: random
    data, the one whose pivots are all off the diagonal and the one with ties everywhere."""
    return DC.FAMILIES if n <= 512 else ("normal", "zero_diag", "ties")


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture
def tail_hook(monkeypatch):
    def set_tail(v):
        if v is None:
            monkeypatch.delenv("KRYST_DENSE_TAIL", raising=False)
        else:
            monkeypatch.setenv("KRYST_DENSE_TAIL", str(v))
    return set_tail


def test_info_reports_the_thresholds(ctx, tail_hook):
    tail_hook(None)
    assert K.LuSolver(ctx).info() == {"cap": CAP, "tail": TAIL, "tile": TILE, "n": -1}
    tail_hook(0)
    assert K.LuSolver(ctx).info()["tail"] == 0


@pytest.mark.parametrize("n", LU_SIZES)
def test_lu_bit_for_bit(ctx, tail_hook, n):
    """kryst_lu_export (permutations, factors) and x equal the restatement bit for bit, with the in-LDS tail on and forced off."""
    for kind in _families(n):
        rp, cp, f, xref = DC.lu_ref(kind, n)
        a = K.DenseMatrix.from_numpy(DC.matrix(kind, n), ctx=ctx)
        for tail in (None, 0):
            tail_hook(tail)
            lu = K.LuSolver(ctx)
            x = np.full(n, 7.0)
            st = lu.solve(a, None, DC.rhs(n), x)
            assert (st.iterations, st.final_residual, st.converged) == (1, 0.0, True)
            grp, gcp, gf = lu.factors()
            tag = (kind, n, tail)
            assert np.array_equal(grp, rp) and np.array_equal(gcp, cp), tag
            assert np.array_equal(gf, f), tag
            assert np.array_equal(x, xref), tag


def test_lu_tie_rule(ctx, tail_hook):
    """Ties go to the smaller row, then the smaller column: the hand-written matrices of test_dense_cpu.py (their pivot sequences are
    worked out there) and matrices whose every step ties n - s times inside ONE row, across all column tiles of the scan, of the step
    kernel (n - 1 > 8 column tiles, more than one row tile) and of the in-LDS tail."""
    mats = list(DC.TIE_MATRICES) + [DC.row_ties(n) for n in (9, 100, 300, 700)]
    for m in mats:
        n = m.shape[0]
        rp, cp, f = R.lu_factor(m)
        if n >= 9:                                                       # by construction: columns in order, rows by rank, no fill
            assert np.array_equal(cp, np.arange(n)) and np.array_equal(np.abs(np.diag(f)), np.arange(n, 0, -1.0)) and not np.tril(f, -1).any()
        b = DC.rhs(n)
        a = K.DenseMatrix.from_numpy(m, ctx=ctx)
        for tail in (None, 0, 5):
            tail_hook(tail)
            lu = K.LuSolver(ctx)
            x = np.zeros(n)
            lu.solve(a, None, b, x)
            grp, gcp, gf = lu.factors()
            assert np.array_equal(grp, rp) and np.array_equal(gcp, cp) and np.array_equal(gf, f), (n, tail)
            assert np.array_equal(x, R.lu_solve(rp, cp, f, b)), (n, tail)


@pytest.mark.parametrize("n", QR_SIZES)
def test_qr_bit_for_bit(ctx, tail_hook, n):
    for kind in (DC.FAMILIES if n <= 301 else ("normal",)):
        a = K.DenseMatrix.from_numpy(DC.matrix(kind, n), ctx=ctx)
        for tail in (None, 0):
            tail_hook(tail)
            x = np.full(n, 7.0)
            st = K.QrSolver().solve(a, None, DC.rhs(n), x)
            assert (st.iterations, st.final_residual, st.converged) == (1, 0.0, True)
            assert np.array_equal(x, DC.qr_ref(kind, n)), (kind, n, tail)


def test_reference_3x3(ctx):
    """direct_lu.rs:150-192: both solvers on [[2,1,1],[1,3,2],[1,0,0]] x = [4,5,6] -> [6,15,-23] within the reference's 1e-10."""
    a = K.DenseMatrix.from_raw(3, 3, [2.0, 1.0, 1.0, 1.0, 3.0, 0.0, 1.0, 2.0, 0.0], ctx=ctx)
    b = np.array([4.0, 5.0, 6.0])
    for solver in (K.LuSolver(ctx), K.QrSolver()):
        x = np.zeros(3)
        solver.solve(a, None, b, x)
        assert np.abs(x - [6.0, 15.0, -23.0]).max() <= 1e-10


def test_solve_cached(ctx, tail_hook):
    tail_hook(None)
    n = 200
    lu = K.LuSolver(ctx)
    with pytest.raises(K.KError) as e:                                   # nothing cached yet
        lu.solve_cached(np.ones(n))
    assert e.value.code == 2
    rp, cp, f, xref = DC.lu_ref("normal", n)
    a = K.DenseMatrix.from_numpy(DC.matrix("normal", n), ctx=ctx)
    x = np.zeros(n)
    lu.solve(a, None, DC.rhs(n), x)
    assert np.array_equal(x, xref)
    for k in (1, 2, 3):
        b = DC.rhs(n, k=k)
        assert np.array_equal(lu.solve_cached(b), R.lu_solve(rp, cp, f, b)), k
    bad = K.DenseMatrix.from_numpy(DC.repeated_row(), ctx=ctx)
    x = np.zeros(bad.nrows())
    with pytest.raises(K.KError) as e:
        lu.solve(bad, None, np.ones(bad.nrows()), x)
    assert e.value.code == 5
    with pytest.raises(K.KError) as e:                                   # the failed factorization left nothing behind
        lu.solve_cached(np.ones(n))
    assert e.value.code == 2


def _expect(ref, call, x, sentinel):
    """`call` fills x; it must end like the restatement's outcome `ref`, x untouched on an error."""
    if ref[0] == "ok":
        call()
        assert np.array_equal(x, ref[1], equal_nan=True)
        return
    with pytest.raises(K.KError) as e:
        call()
    if ref[0] == "zero":
        assert e.value.code == 5 and e.value.row == ref[1]
    else:
        assert e.value.code == 1
    assert np.array_equal(x, sentinel)


@pytest.mark.parametrize("tail", (None, 0))
def test_zero_pivot_and_nonfinite_matrix(ctx, tail_hook, tail):
    tail_hook(tail)
    cases = [DC.repeated_row(), DC.zero_column(6, 3)]
    big = DC.matrix("normal", 200); big[150, :] = big[20, :]            # the zero pivot arrives in the tail (or in the last launches)
    cases.append(big)
    for bad in (np.nan, np.inf, -np.inf):
        for n, (i, j) in ((5, (1, 2)), (300, (299, 0))):
            m = DC.matrix("normal", n); m[i, j] = bad
            cases.append(m)
    for m in cases:
        n = m.shape[0]
        a = K.DenseMatrix.from_numpy(m, ctx=ctx)
        b = DC.rhs(n)
        sentinel = np.full(n, 123.0)
        x = sentinel.copy()
        _expect(DC.outcome(R.lu, m, b), lambda: K.LuSolver(ctx).solve(a, None, b, x), x, sentinel)
        x = sentinel.copy()
        _expect(DC.outcome(R.qr_solve, m, b), lambda: K.QrSolver().solve(a, None, b, x), x, sentinel)
        xd = ctx.vec(sentinel)                                          # the device-vector entry point
        ref = DC.outcome(R.lu, m, b)
        if ref[0] == "ok":
            K.LuSolver(ctx).solve(a, None, ctx.vec(b), xd)
            assert np.array_equal(xd.to_host(), ref[1])
        else:
            with pytest.raises(K.KError):
                K.LuSolver(ctx).solve(a, None, ctx.vec(b), xd)
            assert np.array_equal(xd.to_host(), sentinel)
    assert DC.outcome(R.lu, cases[0], np.ones(7)) == ("zero", 6) and DC.outcome(R.qr_solve, cases[1], np.ones(6)) == ("zero", 3)
    assert DC.outcome(R.lu, big, np.ones(200)) == ("zero", 199)


def test_nonfinite_and_signed_zero_rhs(ctx):
    n = 70
    m = DC.matrix("normal", n)
    a = K.DenseMatrix.from_numpy(m, ctx=ctx)
    rp, cp, f, _ = DC.lu_ref("normal", n)
    lu = K.LuSolver(ctx)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        b = DC.rhs(n, k=k); b[3 * k + 1] = bad
        x = np.zeros(n)
        lu.solve(a, None, b, x)
        ref = R.lu_solve(rp, cp, f, b)
        assert np.array_equal(x, ref, equal_nan=True) and np.array_equal(np.signbit(x)[~np.isnan(x)], np.signbit(ref)[~np.isnan(ref)])
        x = np.zeros(n)
        K.QrSolver().solve(a, None, b, x)
        ref = R.qr_solve(m, b)
        assert np.array_equal(x, ref, equal_nan=True) and np.array_equal(np.signbit(x)[~np.isnan(x)], np.signbit(ref)[~np.isnan(ref)])
    z = np.zeros(n); z[5] = -0.0
    x = np.ones(n)
    lu.solve(a, None, z, x)
    ref = R.lu_solve(rp, cp, f, z)
    assert np.array_equal(x, ref) and np.array_equal(np.signbit(x), np.signbit(ref))


def test_argument_errors(ctx):
    sentinel = np.full(3, 123.0)
    rect = K.DenseMatrix.from_numpy(np.ones((3, 4)), ctx=ctx)
    for solver in (K.LuSolver(ctx), K.QrSolver()):
        x = sentinel.copy()
        with pytest.raises(K.KError) as e:
            solver.solve(rect, None, np.ones(3), x)
        assert e.value.code == 102 and np.array_equal(x, sentinel)
    n = CAP + 1                                                          # above the cap: the identity, densified on the device
    eye = K.CsrMatrix.from_csr(n, n, np.arange(n + 1), np.arange(n), np.ones(n), ctx=ctx)
    a = K.DenseMatrix.from_csr(eye)
    assert a.shape == (n, n)
    b, xd = ctx.vec(np.ones(n)), ctx.vec(np.full(n, 123.0))
    for solver in (K.LuSolver(ctx), K.QrSolver()):
        with pytest.raises(K.KError) as e:
            solver.solve(a, None, b, xd)
        assert e.value.code == 6
    assert np.array_equal(xd.to_host(), np.full(n, 123.0))
    sq = K.DenseMatrix.from_numpy(DC.matrix("normal", 5), ctx=ctx)
    with pytest.raises(K.KError) as e:                                   # vector length
        K.LuSolver(ctx).solve(sq, None, ctx.vec(np.ones(6)), ctx.vec(np.ones(6)))
    assert e.value.code == 102
    with pytest.raises(K.KError) as e:                                   # matvec refuses x and y in one vector
        v = ctx.vec(np.ones(5))
        sq.matvec(v, v)
    assert e.value.code == 102


def test_b_is_x(ctx):
    for n in (5, 200):
        m = DC.matrix("normal", n)
        a = K.DenseMatrix.from_numpy(m, ctx=ctx)
        b = DC.rhs(n)
        v = ctx.vec(b)
        K.LuSolver(ctx).solve(a, None, v, v)
        assert np.array_equal(v.to_host(), DC.lu_ref("normal", n)[3])
        v = ctx.vec(b)
        K.QrSolver().solve(a, None, v, v)
        assert np.array_equal(v.to_host(), DC.qr_ref("normal", n))
        lu = K.LuSolver(ctx)
        w = ctx.vec(n)
        lu.solve(a, None, ctx.vec(b), w)
        v = ctx.vec(b)
        lu.solve_cached(v, v)
        assert np.array_equal(v.to_host(), w.to_host())


@pytest.mark.parametrize("shape", ((64, 64), (63, 65), (65, 63), (257, 257), (256, 259), (258, 255), (1, 7), (7, 1)))
def test_dense_matvec(ctx, shape):
    """Bit-identical to the oracle's SpMV of Csr.from_dense (every entry stored: the reference's dense row loop term by term)."""
    rng = np.random.default_rng([shape[0], shape[1]])
    m = rng.standard_normal(shape)
    x = rng.standard_normal(shape[1])
    a = K.DenseMatrix.from_numpy(m, ctx=ctx)
    assert a.shape == shape and np.array_equal(a.to_numpy(), m)
    y = a.matvec(x)
    assert np.array_equal(y, O.Csr.from_dense(m).spmv(x))
    assert np.array_equal(y, R.matvec(m, x))
    xv = ctx.vec(x).poison_padding()                                     # what lies behind the vector's end does not matter
    assert np.array_equal(a.matvec(xv).to_host(), y)
    raw = K.DenseMatrix.from_raw(shape[0], shape[1], m.T.ravel(), ctx=ctx)              # column-major storage: data[i + j * nrows]
    assert np.array_equal(raw.to_numpy(), m)


@pytest.mark.parametrize("N", (4, 6))
def test_from_csr(ctx, N):
    a_o = O.stencil7(N)
    a = K.CsrMatrix.from_csr(a_o.nrows, a_o.ncols, a_o.row_ptr, a_o.col_idx, a_o.vals, ctx=ctx)
    dense = np.zeros((a_o.nrows, a_o.ncols))
    for i in range(a_o.nrows):
        lo, hi = int(a_o.row_ptr[i]), int(a_o.row_ptr[i + 1])
        dense[i, np.asarray(a_o.col_idx[lo:hi], dtype=np.int64)] = a_o.vals[lo:hi]
    got = K.DenseMatrix.from_csr(a).to_numpy()
    assert np.array_equal(got, dense) and not np.signbit(got[got == 0.0]).any()      # absent entries are +0.0


def test_device_lu_against_cg(ctx):
    """CG on the CsrMatrix against LuSolver on its dense form: the 6^3 Poisson operator, within the reference's 1e-6
    (tests/solver_iterative.rs:33-50)."""
    a_o = O.stencil7(6)
    n = a_o.nrows
    a = K.CsrMatrix.from_csr(n, n, a_o.row_ptr, a_o.col_idx, a_o.vals, ctx=ctx)
    b = np.random.default_rng(6).random(n)
    x_cg = np.zeros(n)
    st = K.CgSolver(1e-8, 1000).solve(a, None, b, x_cg)
    assert st.converged
    x_lu = np.zeros(n)
    K.LuSolver(ctx).solve(K.DenseMatrix.from_csr(a), None, b, x_lu)
    assert np.abs(x_cg - x_lu).max() <= 1e-6


def test_cpp_mirror_dense():
    """tests/cpp/test_dense_mirror.cpp: the reference's two 3 x 3 tests (direct_lu.rs:150-192) through include/kryst_hip.hpp."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_dense_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_DENSE_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
