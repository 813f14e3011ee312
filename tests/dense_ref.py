"""numpy restatement of the dense direct solvers' arithmetic contract, written from the contract and not from the
kernels: fp64, every product, sum, difference and quotient rounded on its own (numpy never fuses), loops vectorised only across elements
that do not depend on each other.  The host twins (kryst_host_dense_*) and the device (LuSolver / QrSolver) must reproduce it bit for bit."""
import functools
import numpy as np


def _quiet(f):
    """NaN / Inf in the data are part of what is restated: no warnings about them."""
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


class ZeroPivot(Exception):
    def __init__(self, step):
        super().__init__(f"zero pivot at step {step}")
        self.step = step


class FactorError(Exception):
    pass


@_quiet
def matvec(a, x):
    """y[i] = +0.0, then y[i] = y[i] + a[i][j] * x[j] for ascending j (all rows at once)."""
    a = np.asarray(a, dtype=np.float64)
    y = np.zeros(a.shape[0])
    for j in range(a.shape[1]):
        y = y + a[:, j] * x[j]
    return y


def pivot_scan(w, s):
    """Row by row (i ascending, j ascending inside a row) over i, j >= s; a later entry replaces the current one only if strictly greater.
    The first entry is the current one to begin with, so a NaN there is never replaced; a NaN elsewhere never wins."""
    t = np.abs(w[s:, s:]).ravel()                 # C order = the scan order
    if np.isnan(t[0]):
        k = 0
    else:
        k = int(np.argmax(np.where(np.isnan(t), -1.0, t)))       # argmax returns the FIRST largest: strictly-greater replacement
    m = w.shape[0] - s
    return s + k // m, s + k % m


@_quiet
def lu_factor(a):
    """-> (row_perm, col_perm, factors): L strictly below the diagonal, U on and above, in the permuted frame."""
    w = np.array(a, dtype=np.float64, order="F")
    n = w.shape[0]
    assert w.shape == (n, n)
    if not np.all(np.isfinite(w)):
        raise FactorError("non-finite entry")
    rp, cp = np.arange(n), np.arange(n)
    for s in range(n):
        p, q = pivot_scan(w, s)
        if w[p, q] == 0.0:
            raise ZeroPivot(s)
        if not np.isfinite(w[p, q]):
            raise FactorError(f"non-finite pivot at step {s}")
        w[[s, p], :] = w[[p, s], :]; rp[[s, p]] = rp[[p, s]]
        w[:, [s, q]] = w[:, [q, s]]; cp[[s, q]] = cp[[q, s]]
        w[s + 1:, s] = w[s + 1:, s] / w[s, s]                                   # true division
        w[s + 1:, s + 1:] = w[s + 1:, s + 1:] - np.outer(w[s + 1:, s], w[s, s + 1:])     # one product, one difference per element
    return rp, cp, w


@_quiet
def back_sweep(f, y):
    for j in range(len(y) - 1, -1, -1):
        y[j] = y[j] / f[j, j]
        y[:j] = y[:j] - f[:j, j] * y[j]
    return y


@_quiet
def lu_solve(rp, cp, f, b):
    n = len(rp)
    y = np.array(b, dtype=np.float64)[rp]
    for j in range(n):
        y[j + 1:] = y[j + 1:] - f[j + 1:, j] * y[j]
    back_sweep(f, y)
    x = np.empty(n)
    x[cp] = y
    return x


def lu(a, b):
    rp, cp, f = lu_factor(a)
    return lu_solve(rp, cp, f, b)


@_quiet
def qr_solve(a, b):
    w = np.array(a, dtype=np.float64)
    n = w.shape[0]
    assert w.shape == (n, n)
    if not np.all(np.isfinite(w)):
        raise FactorError("non-finite entry")
    w = np.hstack([w, np.array(b, dtype=np.float64).reshape(n, 1)])              # c rides along as one more column
    for s in range(n):
        ss = 0.0
        for i in range(s, n):
            ss = ss + w[i, s] * w[i, s]
        nrm = np.sqrt(ss)
        if nrm == 0.0:
            raise ZeroPivot(s)
        alpha = -nrm if w[s, s] >= 0.0 else nrm
        v = w[s:, s].copy()
        v[0] = w[s, s] - alpha
        vv = 0.0
        for i in range(n - s):
            vv = vv + v[i] * v[i]
        if vv == 0.0:
            raise ZeroPivot(s)
        t = np.zeros(n - s)                                                      # the columns j > s and c, all at once
        for i in range(n - s):
            t = t + v[i] * w[s + i, s + 1:]
        t = (2.0 * t) / vv
        w[s:, s + 1:] = w[s:, s + 1:] - np.outer(v, t)
        w[s, s] = alpha
    c = w[:, n].copy()
    return back_sweep(w[:, :n], c)
