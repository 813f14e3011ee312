"""Block Jacobi without a GPU: the numpy restatement of the set-up (tests/bjacobi_ref.py) pinned independently of the device, and the
public surface (PC.BlockJacobi, BlockJacobi, the three C entry points in the ctypes table)."""
import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
import bjacobi_ref as R


@pytest.mark.parametrize("b", [1, 2, 3, 5, 8, 13, 16, 31, 33, 64])
def test_restatement_inverts(b):
    rng = np.random.default_rng(b)
    B = rng.standard_normal((40, b, b))
    B[:, np.arange(b), np.arange(b)] = 0.0 if b > 1 else 1.0        # zero diagonals: off-diagonal pivots (b > 1)
    Bi, zp = R.gauss_jordan(B)
    assert np.all(zp == -1)
    for k in range(len(B)):
        want = np.linalg.inv(B[k])
        cond = np.linalg.cond(B[k])
        assert np.max(np.abs(Bi[k] - want)) <= 64 * b * np.finfo(float).eps * cond * np.max(np.abs(want))


def test_restatement_tie_rule():
    # all entries +-1: every candidate ties, so the first in row-major order over unpivoted rows and columns is taken at each step
    B = np.array([[[1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0]]])
    Bi, zp = R.gauss_jordan(B)
    assert zp[0] == -1
    assert np.allclose(Bi[0] @ B[0], np.eye(3))
    # the same in pure Python, step by step, with the strict ">" scan written out
    T = [row[:] for row in B[0].tolist()]
    piv, rec = set(), []
    for _ in range(3):
        best, p, q = -1.0, 0, 0
        for i in range(3):
            for j in range(3):
                if i not in piv and j not in piv and abs(T[i][j]) > best:
                    best, p, q = abs(T[i][j]), i, j
        T[p], T[q] = T[q], T[p]
        rec.append((p, q)); piv.add(q)
        pivinv = 1.0 / T[q][q]; T[q][q] = 1.0
        T[q] = [v * pivinv for v in T[q]]
        for m in range(3):
            if m != q:
                f = T[m][q]; T[m][q] = 0.0
                T[m] = [T[m][l] - T[q][l] * f for l in range(3)]
    assert rec[0] == (0, 0)                                          # the first of the nine ties
    for p, q in reversed(rec):
        for row in T:
            row[p], row[q] = row[q], row[p]
    assert np.array_equal(np.array(T), Bi[0])


def test_restatement_zero_pivot_position():
    B = np.zeros((3, 4, 4))
    B[0] = np.eye(4)
    B[1] = np.diag([2.0, 3.0, 0.0, 0.0])                             # positions 0, 1 pivot, then the remaining 2x2 is zero
    B[2, 0, 1] = 1.0; B[2, 1, 0] = 1.0; B[2, 3, 3] = 1.0             # position 2 is never pivotable
    Bi, zp = R.gauss_jordan(B)
    assert list(zp) == [-1, 2, 2]
    assert np.array_equal(Bi[0], np.eye(4))


def test_restatement_apply_is_the_spmv_order():
    rng = np.random.default_rng(9)
    Bi = rng.standard_normal((5, 6, 6))
    rg = rng.standard_normal((5, 6))
    z = R.apply_pinned(Bi, rg)
    for k in range(5):
        for i in range(6):
            s = 0.0
            for j in range(6):
                s = s + Bi[k, i, j] * rg[k, j]
            assert z[k, i] == s


def test_public_surface():
    assert callable(K.PC.BlockJacobi) and K.PC.BlockJacobi([[0, 1]]).kind == "BlockJacobi"
    assert issubclass(K.BlockJacobi, K._Pc) and callable(K.BlockJacobi.uniform) and hasattr(K.BlockJacobi, "inverse_csr")
    for name in ("kryst_pc_block_jacobi", "kryst_pc_block_jacobi_uniform", "kryst_pc_block_jacobi_export"):
        assert name in _ffi.SIGNATURES
    assert "BlockJacobi" not in K.PC.__doc__.split("raise")[0].split("(")[-1]          # no longer listed as unsupported


def test_blocks_argument_forms():
    pc = K.BlockJacobi([[3, 1], [], [0]])
    assert list(pc.ptr) == [0, 2, 2, 3] and list(pc.idx) == [3, 1, 0]
    pc = K.BlockJacobi((np.array([0, 2, 3]), np.array([5, 4, 1])))
    assert list(pc.ptr) == [0, 2, 3] and list(pc.idx) == [5, 4, 1]
    assert K.BlockJacobi.uniform(8).bsize == 8
    with pytest.raises(K.KError):
        K.BlockJacobi((np.array([0, 4]), np.array([1, 2])))
