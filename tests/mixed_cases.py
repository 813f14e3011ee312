"""Matrices and vectors of the mixed-precision tests, shared by the CPU tier (tests/test_mixed_cpu.py: the restatement alone) and the GPU
tier (tests/test_gpu_mixed.py: the library against the restatement, bit for bit)."""
import numpy as np

from oracle import oracle as O

OUTER_TOL, INNER_TOL, INNER_CAP, OUTER_CAP = 1e-10, 1e-6, 2000, 30


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rhs(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n)


def vec32(n, seed=11):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ---- the operators of the convergence cases: name -> (operator, uses Jacobi)
def poisson12():
    return O.stencil7(12, "poisson")


def aniso16():
    return O.stencil7(16, "aniso")


def varcoef12():
    return O.stencil7(12, "varcoef")


REFINE_CASES = {"poisson12": (poisson12, False), "aniso16": (aniso16, False), "varcoef12-jacobi": (varcoef12, True)}


def hilbert(n):
    i = np.arange(n)
    return O.Csr.from_dense(1.0 / (i[:, None] + i[None, :] + 1.0))


def singular_when_lowered():
    """[[1, 1 - 2^-30], [1 - 2^-30, 1]]: SPD in fp64, all ones -- singular -- once its values are rounded to fp32"""
    e = 1.0 - 2.0 ** -30
    return O.Csr.from_dense(np.array([[1.0, e], [e, 1.0]]))


def indefinite():
    """diag(1, -1, 2, ...) plus a weak coupling: p.Ap turns negative at once for b = e_2"""
    n = 40
    d = np.where(np.arange(n) % 2 == 1, -1.0, 1.0) * (1.0 + np.arange(n) / n)
    m = np.diag(d) + 0.01 * (np.eye(n, k=1) + np.eye(n, k=-1))
    return O.Csr.from_dense(m, keep_zeros=False)


def zero_diagonal():
    """an SPD-looking tridiagonal operator whose row 5 stores no diagonal entry: Jacobi's inverse is 0 there (jacobi.rs:53-73)"""
    n = 64
    m = 4.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    m[5, 5] = 0.0
    return O.Csr.from_dense(m, keep_zeros=False)


# ---- SpMV shapes
def _random_csr(nrows, ncols, lengths, seed):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ci = np.empty(rp[-1], dtype=np.int64)
    for i, ln in enumerate(lengths):
        ci[rp[i]:rp[i + 1]] = np.sort(rng.choice(ncols, size=ln, replace=False))
    va = rng.standard_normal(rp[-1]) * np.exp(rng.uniform(-3, 3, rp[-1]))
    return O.Csr(nrows, ncols, rp, ci, va)


def ragged():
    """3000 rows x 6000 columns: empty rows, one row of 5000 entries (three LDS windows), row starts at every residue of 8 entries"""
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 14, 3000)
    lengths[rng.integers(0, 3000, 300)] = 0
    lengths[1500] = 5000
    lengths[0] = 0
    a = _random_csr(3000, 6000, lengths, 4)
    assert set((a.row_ptr[:-1][lengths > 0] % 8).tolist()) == set(range(8)) and (lengths == 0).sum() > 100
    return a


def one_row():
    return _random_csr(1, 50, np.array([9]), 5)


def banded1025():
    n = 1025
    m = np.zeros((n, n))
    for k in (-3, -1, 0, 1, 3):
        m += np.diag(np.full(n - abs(k), 1.0 / (1 + abs(k))), k)
    return O.Csr.from_dense(m, keep_zeros=False)


def nonsquare():
    return _random_csr(700, 1300, np.random.default_rng(6).integers(1, 20, 700), 7)


def tiny_products():
    """values and operands of about 1e-20: every product is of the order 1e-40 and lands on an fp32 subnormal"""
    a = _random_csr(300, 300, np.random.default_rng(8).integers(1, 6, 300), 9)
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, np.sign(a.vals) * 1e-20 * (1.0 + np.abs(a.vals) % 1.0))


SPMV_OPERATORS = {"poisson12": poisson12, "varcoef12": varcoef12, "ragged": ragged, "one_row": one_row, "banded1025": banded1025,
                  "nonsquare": nonsquare}


def special32(n, seed=13):
    """fp32 input with NaN, +-inf, -0.0 and subnormals sprinkled in"""
    x = vec32(n, seed)
    rng = np.random.default_rng(seed + 1)
    idx = rng.permutation(n)
    k = max(1, n // 9)
    x[idx[0:k]] = np.nan
    x[idx[k:2 * k]] = np.inf
    x[idx[2 * k:3 * k]] = -np.inf
    x[idx[3 * k:4 * k]] = -0.0
    x[idx[4 * k:5 * k]] = np.float32(1e-41)
    return x
