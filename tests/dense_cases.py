"""Seeded dense test matrices shared by test_dense_cpu.py and test_gpu_dense.py, and the restatement's answers for them (computed once)."""
import functools
import numpy as np

import dense_ref as R

FAMILIES = ("normal", "zero_diag", "graded", "ties", "scaled_perm")


def matrix(kind, n, seed=0):
    rng = np.random.default_rng([seed, n, sum(map(ord, kind))])
    if kind == "normal":
        return rng.standard_normal((n, n))
    if kind == "diag_dominant":                       # uniform + n I
        return rng.uniform(-1.0, 1.0, (n, n)) + n * np.eye(n)
    if kind == "zero_diag":                           # every pivot is off the diagonal
        a = rng.standard_normal((n, n))
        np.fill_diagonal(a, 0.0)
        if n == 1:
            a[0, 0] = 1.5                             # (a 1 x 1 zero matrix is singular)
        return a
    if kind == "graded":                              # rows graded over 10^12
        return rng.standard_normal((n, n)) * (10.0 ** rng.uniform(-6.0, 6.0, (n, 1)))
    if kind == "ties":                                # entries from {-1, 0, 1}: ties everywhere (in a row too), exact arithmetic to begin with
        return _ties(n, seed).copy()
    if kind == "scaled_perm":
        a = np.zeros((n, n))
        a[np.arange(n), rng.permutation(n)] = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-20, 21, n)
        return a
    raise KeyError(kind)


_LU_OF_TIES = {}


@functools.lru_cache(maxsize=None)
def _ties(n, seed):
    """The first draw of an n x n matrix with entries from {-1, 0, 1} that the restatement's LU factors without a zero pivot (such a
    matrix is singular with a probability that matters at small n only).  Its factors are kept for lu_ref."""
    rng = np.random.default_rng([seed, n, 7141])
    for _ in range(200):
        a = rng.integers(-1, 2, (n, n)).astype(np.float64)
        try:
            _LU_OF_TIES[(n, seed)] = R.lu_factor(a)
            return a
        except R.ZeroPivot:
            continue
    raise RuntimeError("no regular {-1, 0, 1} matrix drawn")


# Hand-written integer matrices whose pivot sequences are worked out in test_dense_cpu.py: ties between rows, inside a row, and (1, 2)
# against (2, 1), which a column-by-column scan would settle the other way.
TIE_MATRICES = (
    np.array([[1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0]]),
    np.array([[4.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.0, 2.0, 1.0]]),
    np.array([[1.0, 2.0, 2.0, 1.0], [2.0, 1.0, 2.0, 2.0], [2.0, 2.0, 1.0, 2.0], [1.0, 2.0, 2.0, -2.0]]),
)


def row_ties(n, seed=0):
    """A row-permuted upper triangle whose row of rank i holds n - i entries +-(n - i) in the columns i .. n - 1.  Step s finds its maximum
    n - s times in ONE row, across every column tile of the trailing block, so only the smaller-column half of the tie rule decides; the
    column it must take holds nothing below the pivot, so every multiplier is 0, nothing changes and the next step looks the same."""
    rng = np.random.default_rng([seed, n, 90210])
    u = np.triu(rng.choice([-1.0, 1.0], (n, n))) * np.arange(n, 0, -1.0)[:, None]
    return u[rng.permutation(n)]


def rhs(n, seed=0, k=0):
    return np.random.default_rng([seed, n, 977 + k]).standard_normal(n)


def repeated_row(n=7):
    """An integer matrix whose row 4 repeats row 1: elimination is exact, so both factorizations meet an exactly zero pivot / column."""
    a = np.random.default_rng(41).integers(-3, 4, (n, n)).astype(np.float64) + 5.0 * np.eye(n)
    a[4, :] = a[1, :]
    return a


def zero_column(n=6, k=3):
    """Column k is zero and stays exactly zero under every reflection and elimination step: QR stops at step k with a zero column."""
    a = np.random.default_rng(43).standard_normal((n, n))
    a[:, k] = 0.0
    return a


def outcome(fn, *args):
    """("ok", x) | ("zero", step) | ("factor",) of a restatement call."""
    try:
        return ("ok", fn(*args))
    except R.ZeroPivot as e:
        return ("zero", e.step)
    except R.FactorError:
        return ("factor",)


@functools.lru_cache(maxsize=None)
def lu_ref(kind, n):
    """(row_perm, col_perm, factors, x) of the restatement for matrix(kind, n) and rhs(n)."""
    a = matrix(kind, n)
    rp, cp, f = _LU_OF_TIES[(n, 0)] if kind == "ties" else R.lu_factor(a)
    return rp, cp, f, R.lu_solve(rp, cp, f, rhs(n))


@functools.lru_cache(maxsize=None)
def qr_ref(kind, n):
    return R.qr_solve(matrix(kind, n), rhs(n))
