"""The dense direct solvers without a GPU: the numpy restatement of DESIGN.md section 4.12 (tests/dense_ref.py) against known answers and
error bounds that do not come from the code under test, and the host twins (kryst_host_dense_*) bit for bit against the restatement."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import dense_ref as R
import dense_cases as DC

U = 2.0 ** -53
ACC_SIZES = (1, 2, 5, 63, 64, 65, 257, 300, 512)
ACC_FAMILIES = ("normal", "diag_dominant", "graded")
A3 = np.array([[2.0, 1.0, 1.0], [1.0, 3.0, 2.0], [1.0, 0.0, 0.0]])        # direct_lu.rs:150-192
B3 = np.array([4.0, 5.0, 6.0])
X3 = np.array([6.0, 15.0, -23.0])


# ---------------------------------------------------------------- the restatement: known answers
def test_restatement_reference_3x3():
    assert np.abs(R.lu(A3, B3) - X3).max() <= 1e-10
    assert np.abs(R.qr_solve(A3, B3) - X3).max() <= 1e-10


def test_restatement_exact_cases():
    b = np.array([3.0, -5.0, 7.0, 0.5])
    assert np.array_equal(R.lu(np.eye(4), b), b)
    d = np.array([2.0, -4.0, 0.5, 8.0])
    rp, cp, f = R.lu_factor(np.diag(d))
    assert list(rp) == [3, 1, 0, 2] and list(cp) == [3, 1, 0, 2]            # by |d| descending: 8, -4, 2, 0.5
    assert np.array_equal(f, np.diag([8.0, -4.0, 2.0, 0.5]))
    assert np.array_equal(R.lu_solve(rp, cp, f, b), b / d)
    perm = np.array([2, 0, 3, 1])
    p = np.zeros((4, 4)); p[np.arange(4), perm] = 1.0                        # (P x)[i] = x[perm[i]]
    x = np.empty(4); x[perm] = b
    assert np.array_equal(R.lu(p, b), x)
    rp, cp, f = R.lu_factor(p)
    assert np.array_equal(f, np.eye(4))
    # Householder QR of a matrix whose reflectors are exact: the identity (alpha = -1, v = 2 e_s, vv = 4) and a diagonal of powers of two
    assert np.array_equal(R.qr_solve(np.eye(4), b), b)
    assert np.array_equal(R.qr_solve(np.diag(d), b), b / d)
    assert np.array_equal(R.matvec(np.diag(d), b), d * b)


def test_restatement_pivot_sequence_with_ties():
    """Ties go to the smaller row, then the smaller column (the row-by-row scan); the sequences are worked out by hand."""
    # step 0: every |entry| is 1 -> (0, 0).  l = (1, -1); trailing block [[2, -2], [0, 2]]: 2 three times -> (1, 1); last pivot 2 - 0 * (-2)
    a = np.array([[1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0]])
    rp, cp, f = R.lu_factor(a)
    assert list(rp) == [0, 1, 2] and list(cp) == [0, 1, 2]
    assert np.array_equal(f, [[1.0, -1.0, 1.0], [1.0, 2.0, -2.0], [-1.0, 0.0, 2.0]])
    # step 1 meets |2| at (1, 2) and at (2, 1): the row-by-row scan takes (1, 2), a column-by-column scan would take (2, 1)
    a = np.array([[4.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.0, 2.0, 1.0]])
    rp, cp, f = R.lu_factor(a)
    assert list(rp) == [0, 1, 2] and list(cp) == [0, 2, 1]
    assert np.array_equal(f, [[4.0, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 0.5, 1.5]])
    # step 0: the first 2 in scan order is (0, 1).  After it the trailing block is [[1.5, 1, 1.5], [1, -1, 1], [0, 0, -3]] -> (3, 3);
    # then [[-1, 1], [1, 1.5]] -> (3, 3); the last step has one entry
    a = np.array([[1.0, 2.0, 2.0, 1.0], [2.0, 1.0, 2.0, 2.0], [2.0, 2.0, 1.0, 2.0], [1.0, 2.0, 2.0, -2.0]])
    rp, cp, f = R.lu_factor(a)
    assert list(rp) == [0, 3, 1, 2] and list(cp) == [1, 3, 0, 2]
    assert list(np.diag(f)[:3]) == [2.0, -3.0, 1.5]


def test_restatement_errors():
    a = DC.repeated_row()
    with pytest.raises(R.ZeroPivot) as e:
        R.lu_factor(a)
    assert e.value.step == a.shape[0] - 1                    # rank n - 1, exact arithmetic: the last trailing block is the zero
    with pytest.raises(R.ZeroPivot) as e:
        R.qr_solve(np.array([[1.0, 0.0], [2.0, 0.0]]), np.ones(2))
    assert e.value.step == 1
    for bad in (np.nan, np.inf, -np.inf):
        m = np.eye(3); m[1, 2] = bad
        with pytest.raises(R.FactorError):
            R.lu_factor(m)
        with pytest.raises(R.FactorError):
            R.qr_solve(m, np.ones(3))


# ---------------------------------------------------------------- the restatement: accuracy
@pytest.mark.parametrize("n", ACC_SIZES)
def test_lu_backward_error_theorem(n):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 9.4: |P b - (P A Q)(Q^T x)| <= gamma_3n |L||U||Q^T x| componentwise,
    gamma_k = k u / (1 - k u), with the computed factors; the residual in extended precision."""
    LD = np.longdouble
    g = 3 * n * U / (1.0 - 3 * n * U)
    for kind in ACC_FAMILIES:
        a, b = DC.matrix(kind, n), DC.rhs(n)
        rp, cp, f = R.lu_factor(a)
        x = R.lu_solve(rp, cp, f, b)
        lo, up = np.tril(f, -1) + np.eye(n), np.triu(f)
        res = np.abs(b[rp].astype(LD) - a[np.ix_(rp, cp)].astype(LD) @ x[cp].astype(LD))
        bound = g * (np.abs(lo).astype(LD) @ (np.abs(up).astype(LD) @ np.abs(x[cp]).astype(LD)))
        ratio = float((res / np.where(bound > 0, bound, 1)).max())
        print(f"n={n} {kind}: largest |residual| / bound = {ratio:.3f}")
        assert np.all(res <= bound), (kind, ratio)


def _eta(a, x, b):
    LD = np.longdouble
    r = np.abs(b.astype(LD) - a.astype(LD) @ x.astype(LD)).max()
    return float(r / (np.abs(a).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


@pytest.mark.parametrize("n", ACC_SIZES)
def test_qr_backward_error_against_lapack(n):
    """eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) of the restatement's QR against numpy.linalg.solve's on the same input:
    another elimination order moves eta by a small factor (10), and n u is the floor below which the ratio of two errors is noise."""
    for kind in ACC_FAMILIES:
        a, b = DC.matrix(kind, n), DC.rhs(n)
        e_qr, e_la = _eta(a, R.qr_solve(a, b), b), _eta(a, np.linalg.solve(a, b), b)
        print(f"n={n} {kind}: eta qr {e_qr:.3e} lapack {e_la:.3e} ratio {e_qr / max(e_la, 1e-300):.2f} eta / (n u) {e_qr / (n * U):.3f}")
        assert e_qr <= max(10.0 * e_la, n * U), (kind, e_qr, e_la)


# ---------------------------------------------------------------- the host twins
@pytest.mark.parametrize("n", (1, 2, 3, 5, 64, 65, 300))
def test_host_twins_bit_identical(n):
    for kind in DC.FAMILIES:
        a, b = DC.matrix(kind, n), DC.rhs(n)
        rp, cp, f, x = DC.lu_ref(kind, n)
        hrp, hcp, hf = K.host_dense_lu(a)
        assert np.array_equal(hrp, rp) and np.array_equal(hcp, cp), kind
        assert np.array_equal(hf, f), kind
        assert np.array_equal(K.host_dense_lu_solve(hrp, hcp, hf, b), x), kind
        if n <= 65 or kind == "normal":
            assert np.array_equal(K.host_dense_qr_solve(a, b), DC.qr_ref(kind, n)), kind


def test_host_twins_tie_rule():
    """The smaller row, then the smaller column: the hand-written tie matrices and matrices that tie inside one row at every step."""
    for m in list(DC.TIE_MATRICES) + [DC.row_ties(n) for n in (9, 100, 300)]:
        n = m.shape[0]
        rp, cp, f = R.lu_factor(m)
        if n >= 9:
            assert np.array_equal(cp, np.arange(n)) and np.array_equal(np.abs(np.diag(f)), np.arange(n, 0, -1.0)) and not np.tril(f, -1).any()
        hrp, hcp, hf = K.host_dense_lu(m)
        assert np.array_equal(hrp, rp) and np.array_equal(hcp, cp) and np.array_equal(hf, f), n


def test_host_twins_reference_3x3():
    rp, cp, f = K.host_dense_lu(A3)
    assert np.abs(K.host_dense_lu_solve(rp, cp, f, B3) - X3).max() <= 1e-10
    assert np.abs(K.host_dense_qr_solve(A3, B3) - X3).max() <= 1e-10


def test_host_twins_in_place_and_nonfinite_rhs():
    n = 9
    a = DC.matrix("normal", n)
    rp, cp, f = K.host_dense_lu(a)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        b = DC.rhs(n, k=k); b[k + 1] = bad
        ref = R.lu_solve(rp, cp, f, b)
        assert np.array_equal(K.host_dense_lu_solve(rp, cp, f, b), ref, equal_nan=True)
        assert np.array_equal(np.signbit(K.host_dense_lu_solve(rp, cp, f, b)), np.signbit(ref))
        x = b.copy()
        K.host_dense_lu_solve(rp, cp, f, x, x)                               # b is x
        assert np.array_equal(x, ref, equal_nan=True)
        assert np.array_equal(K.host_dense_qr_solve(a, b), R.qr_solve(a, b), equal_nan=True)
    z = np.zeros(n); z[3] = -0.0
    assert np.array_equal(np.signbit(K.host_dense_lu_solve(rp, cp, f, z)), np.signbit(R.lu_solve(rp, cp, f, z)))


def test_host_twins_errors():
    a = DC.repeated_row()
    n = a.shape[0]
    with pytest.raises(R.ZeroPivot) as ref:
        R.lu_factor(a)
    with pytest.raises(K.KError) as e:
        K.host_dense_lu(a)
    assert e.value.code == 5 and e.value.row == ref.value.step
    sentinel = np.full(n, 123.0)
    # QR: reflections do not keep two equal rows equal, so the repeated row need not give an exact zero; whatever the restatement does
    # with it the twin does too.  A zero column stays exactly zero: step k stops on it.
    for m in (a, DC.zero_column(6, 3)):
        nn = m.shape[0]
        ref = DC.outcome(R.qr_solve, m, np.ones(nn))
        x = sentinel[:nn].copy()
        if ref[0] == "ok":
            assert np.array_equal(K.host_dense_qr_solve(m, np.ones(nn), x), ref[1])
        else:
            with pytest.raises(K.KError) as e:
                K.host_dense_qr_solve(m, np.ones(nn), x)
            assert e.value.code == 5 and e.value.row == ref[1] and np.array_equal(x, sentinel[:nn])
    assert DC.outcome(R.qr_solve, DC.zero_column(6, 3), np.ones(6)) == ("zero", 3)
    m = np.eye(4); m[2, 1] = np.nan
    with pytest.raises(K.KError) as e:
        K.host_dense_lu(m)
    assert e.value.code == 1
    x = sentinel[:4].copy()
    with pytest.raises(K.KError) as e:
        K.host_dense_qr_solve(m, np.ones(4), x)
    assert e.value.code == 1 and np.array_equal(x, sentinel[:4])
    with pytest.raises(K.KError) as e:
        K.host_dense_lu(np.ones((3, 4)))
    assert e.value.code == 102
    x = sentinel[:3].copy()
    with pytest.raises(K.KError) as e:
        K.host_dense_qr_solve(np.ones((3, 4)), np.ones(3), x)
    assert e.value.code == 102 and np.array_equal(x, sentinel[:3])


# ---------------------------------------------------------------- the reference's cross-checks (tests/solver_iterative.rs:33-77), seeded
def test_reference_cg_vs_direct_on_spd():
    n = 10
    rng = np.random.default_rng(20)
    m = rng.random((n, n))
    a = m.T @ m + np.eye(n)
    b = rng.random(n)
    res = O.solve("cg", O.Csr.from_dense(a), b, tol=1e-8, max_iters=1000)
    assert res.converged
    rp, cp, f = K.host_dense_lu(a)
    assert np.abs(res.x - K.host_dense_lu_solve(rp, cp, f, b)).max() <= 1e-6


def test_reference_gmres_vs_direct_on_nonsymmetric():
    n = 10
    rng = np.random.default_rng(21)
    a = rng.random((n, n))
    b = rng.random(n)
    res = O.solve("gmres", O.Csr.from_dense(a), b, tol=1e-8, max_iters=1000, restart=100)
    assert res.converged
    assert np.abs(res.x - K.host_dense_qr_solve(a, b)).max() <= 1e-6
