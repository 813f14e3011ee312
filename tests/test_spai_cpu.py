"""The SPAI set-up without a GPU: the numpy restatement (tests/spai_ref.py) against the reference's own known answers
(approxinv.rs:382-442) and against the full n-row least squares, and the public surface (SparsityPattern, Spai, PC.ApproxInv, the two C
entry points in the ctypes table)."""
import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import spai_ref as R


def _setup_dense(dense, pat, tol):
    a = O.Csr.from_dense(dense, keep_zeros=False)
    ptr, idx = R.manual_ptr_idx(pat)
    (rp, ci, va), _ = R.setup(a, ptr, idx, tol)
    return [[(int(ci[e]), float(va[e])) for e in range(rp[i], rp[i + 1])] for i in range(a.nrows)]


def test_known_answer_diagonal():                       # approxinv.rs:382-394
    inv = _setup_dense(np.diag([2.0, 3.0, 4.0]), [[0], [1], [2]], 1e-12)
    assert [len(r) for r in inv] == [1, 1, 1] and [r[0][0] for r in inv] == [0, 1, 2]
    for got, want in zip([r[0][1] for r in inv], [0.5, 1.0 / 3.0, 0.25]):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))


def test_known_answer_two_by_two():                     # approxinv.rs:396-424
    A = np.array([[4.0, 1.0], [2.0, 3.0]])
    inv = _setup_dense(A, [[0, 1], [0, 1]], 1e-12)
    M = np.zeros((2, 2))
    for i, row in enumerate(inv):
        assert [c for c, _ in row] == [0, 1]             # ascending columns
        for c, v in row:
            M[i, c] = v
    # the reference's assertion as written: y = M x against [[0.375, -0.125], [-0.25, 0.5]] x with assert_relative_eq!(epsilon = 2.5e-1)
    x = np.array([1.0, 2.0])
    y, y_expected = M @ x, np.array([[0.375, -0.125], [-0.25, 0.5]]) @ x
    for a_, b_ in zip(y, y_expected):
        assert abs(a_ - b_) <= 2.5e-1 or abs(a_ - b_) <= 2.5e-1 * max(abs(a_), abs(b_))
    # ... which that matrix passes only through the loose epsilon: the full pattern gives A^-1 itself
    assert np.allclose(M, np.linalg.inv(A), rtol=0, atol=1e-15)


def test_known_answer_identity():                       # approxinv.rs:426-442
    inv = _setup_dense(np.eye(4), [[0], [1], [2], [3]], 1e-12)
    assert inv == [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)]]


def test_drop_is_strict_and_rows_ascend():
    # M = diag(1/d) = (0.5, 0.25, 0.125): an entry equal to tol is dropped (strict >)
    d = np.array([2.0, 4.0, 8.0])
    inv = _setup_dense(np.diag(d), [[0], [1], [2]], 0.25)
    assert inv == [[(0, 0.5)], [], []]
    # j not in I_j: column 0's pattern {1} of a diagonal operator gives m = 0, dropped even at tol = 0
    inv = _setup_dense(np.diag(d), [[1], [1], [2]], 0.0)
    assert inv[1] == [(1, 0.25)] and inv[0] == [] and inv[2] == [(2, 0.125)]


@pytest.mark.parametrize("seed", range(8))
def test_reduced_equals_full_least_squares(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 60))
    dense = np.where(rng.random((n, n)) < 0.12, rng.standard_normal((n, n)), 0.0)
    dense[np.arange(n), np.arange(n)] += 4.0
    a = O.Csr.from_dense(dense, keep_zeros=False)
    col = R.column_lists(*R.csc(a.row_ptr, a.col_idx, a.vals, n))
    for j in range(n):
        J = rng.choice(n, size=int(rng.integers(1, 6)), replace=False)
        J = np.union1d(J, [j]) if rng.random() < 0.7 else J              # sometimes j is not in the pattern at all
        Js, I, Ah, e = R.reduced_problem(j, J, col)
        m = R.solve_column(Ah, e)
        full = np.linalg.lstsq(dense[:, Js], np.eye(n)[:, j], rcond=None)[0]
        assert np.max(np.abs(m - full)) <= 1e-13 * max(1.0, np.max(np.abs(full)))
        assert np.array_equal(I, np.unique(np.nonzero(dense[:, Js])[0]))    # I_j: the stored rows of the columns J_j


def test_csc_rows_ascend():
    rng = np.random.default_rng(5)
    dense = np.where(rng.random((40, 40)) < 0.2, 1.0 + rng.random((40, 40)), 0.0)
    a = O.Csr.from_dense(dense, keep_zeros=False)
    cp, cr, cv = R.csc(a.row_ptr, a.col_idx, a.vals, 40)
    for k in range(40):
        assert np.array_equal(cr[cp[k]:cp[k + 1]], np.nonzero(dense[:, k])[0])
        assert np.array_equal(cv[cp[k]:cp[k + 1]], dense[cr[cp[k]:cp[k + 1]], k])


def test_public_surface():
    for name in ("kryst_pc_spai", "kryst_pc_spai_export"):
        assert name in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["kryst_pc_spai"][1]) == 7 and len(_ffi.SIGNATURES["kryst_pc_spai_export"][1]) == 5
    assert issubclass(K.Spai, K._Pc) and hasattr(K.Spai, "export")
    p = K.PC.ApproxInv(K.SparsityPattern.Operator, 1e-12, 10)
    assert p.kind == "ApproxInv" and p.params["tol"] == 1e-12 and p.params["max_iter"] == 10
    assert "ApproxInv" not in K.PC.__doc__.split("raise")[0].split("(")[-1]      # no longer listed as unsupported
    assert K.SparsityPattern.Auto.kind == 1 and K.SparsityPattern.Operator.kind == 2
    m = K.SparsityPattern.Manual([[3, 1], [], [0]])
    assert m.kind == 0 and list(m.ptr) == [0, 2, 2, 3] and list(m.idx) == [3, 1, 0]
    m = K.SparsityPattern.Manual((np.array([0, 1, 3]), np.array([2, 0, 1])))
    assert list(m.ptr) == [0, 1, 3] and list(m.idx) == [2, 0, 1]
    s = K.Spai([[0], [1]], 1e-3, 5, 1, 100, 8, 1, 0, False, False)              # ApproxInv::new's ten arguments
    assert s.pattern.kind == 0 and s.tol == 1e-3 and s.max_iter == 5


def test_pattern_argument_checks():
    with pytest.raises(K.KError) as e:
        K.SparsityPattern.Manual((np.array([0, 4]), np.array([1, 2])))           # ptr and idx disagree
    assert e.value.code == 102
    with pytest.raises(K.KError):
        K.SparsityPattern.Manual((np.array([1, 2]), np.array([1])))              # ptr[0] != 0
    with pytest.raises(K.KError):
        K.Spai((np.array([0, 3]), np.array([0])), 1e-12)
