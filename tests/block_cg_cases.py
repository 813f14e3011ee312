"""Fixtures of the block CG tests, shared by the CPU tier (test_block_cg_cpu.py: the restatement against a plain implementation, the true
residuals, the pivot margins, the scalar step) and the GPU tier (test_gpu_block_cg.py: the device against the restatement, bit for bit).

Everything here is numpy and the oracle; nothing touches the device.  References are computed once (lru_cache) and never modified."""
import functools

import numpy as np

from oracle import oracle as O
import block_cg_ref as R

WIDTHS = (2, 4, 8)
TOL, CAP = 1e-8, 200
PCS = (None, "identity", "jacobi")
# (name, N, kind): 7-point Poisson at 8^3 (exactly one tile), 9^3 and 12^3; the symmetric variable-coefficient 7-point operator at 12^3, the
# kind that carries the CSR-DIA streams
FIXTURES = (("poisson8", 8, "poisson"), ("poisson9", 9, "poisson"), ("poisson12", 12, "poisson"), ("varcoef12", 12, "varcoef"))
NAMES = tuple(f[0] for f in FIXTURES)
_BY_NAME = {f[0]: f for f in FIXTURES}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def operator(name):
    _, N, kind = _BY_NAME[name]
    return O.stencil7(N, kind)


def kind_of(name):
    return _BY_NAME[name][1:]


@functools.lru_cache(maxsize=None)
def rhs(name, m=8):
    """right-hand sides uniform in [0, 1) from a fixed seed, (n, m)"""
    a = operator(name)
    return np.random.default_rng(0xB10C + a.nrows).random((a.nrows, m))


@functools.lru_cache(maxsize=None)
def guesses(name, m=8):
    a = operator(name)
    return np.random.default_rng(77 + a.nrows).standard_normal((a.nrows, m))


@functools.lru_cache(maxsize=None)
def inv_diag(name):
    return O.Pc.jacobi(operator(name)).inv_diag.copy()


def weights(name, pc):
    return inv_diag(name) if pc == "jacobi" else None


@functools.lru_cache(maxsize=None)
def reference(name, k, pc, tol=TOL, max_iters=CAP, guess=False, alias=False):
    """the restatement on the first k columns; pc None and "identity" are the same computation"""
    b = rhs(name)[:, :k]
    x0 = b if alias else guesses(name)[:, :k] if guess else None
    return R.solve(operator(name), b, x0=x0, d=weights(name, pc), tol=tol, max_iters=max_iters)


@functools.lru_cache(maxsize=None)
def single_counts(name, k, pc):
    """iterations of single CG / Jacobi-PCG per column, to the same tolerance in the norm block CG watches (PCG: Natural, sqrt|r.z|)"""
    a, b = operator(name), rhs(name)[:, :k]
    out = []
    for j in range(k):
        if pc == "jacobi":
            r = O.solve("pcg", a, np.ascontiguousarray(b[:, j]), pc=O.Pc.jacobi(a), tol=TOL, max_iters=CAP, norm_type=2, rs=R.rs())
        else:
            r = O.solve("cg", a, np.ascontiguousarray(b[:, j]), tol=TOL, max_iters=CAP, rs=R.rs())
        out.append(r.iterations)
    return out


# ---------------------------------------------------------------------------------------------------------------- ways of ending
@functools.lru_cache(maxsize=None)
def shifted_poisson8():
    """A - 3 I: indefinite"""
    a = operator("poisson8")
    vals = a.vals.copy()
    for i in range(a.nrows):
        lo, hi = a.row_ptr[i], a.row_ptr[i + 1]
        vals[lo:hi][a.col_idx[lo:hi] == i] -= 3.0
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals)


@functools.lru_cache(maxsize=None)
def negative_diagonal_poisson8():
    """Poisson with entry (0, 0) = -1e-3: the Jacobi weights hold -1000, which makes the weighted residual Gram's first diagonal entry negative"""
    a = operator("poisson8")
    vals = a.vals.copy()
    lo, hi = a.row_ptr[0], a.row_ptr[1]
    vals[lo:hi][a.col_idx[lo:hi] == 0] = -1e-3
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals)


@functools.lru_cache(maxsize=None)
def tridiag3():
    return O.Csr.from_dense(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 2.0]]), keep_zeros=False)


def breakdown_cases():
    """name -> (operator, B (n, 4), jacobi?, expected status, expected iteration); the initial guesses (breakdown_reference) are nonzero and keep the
    residual block's defect: the duplicate columns share a guess, the zero column starts from zero, the indefinite case from a constant"""
    b = rhs("poisson8")[:, :4]
    dup = b.copy(); dup[:, 2] = dup[:, 0]
    zero = b.copy(); zero[:, 1] = 0.0
    neg = b.copy(); neg[0, :] = 1.0
    return {
        "duplicate": (operator("poisson8"), dup, False, R.SOLVE_ERROR, 0),
        "zero_column": (operator("poisson8"), zero, False, R.SOLVE_ERROR, 0),
        "n3_k4": (tridiag3(), np.random.default_rng(3).random((3, 4)), False, R.SOLVE_ERROR, 0),
        "indefinite": (shifted_poisson8(), b, False, R.INDEFINITE_MATRIX, 1),
        "negative_jacobi": (negative_diagonal_poisson8(), neg, True, R.INDEFINITE_PC, 0),
    }


@functools.lru_cache(maxsize=None)
def breakdown_reference(name):
    a, b, jac, _, _ = breakdown_cases()[name]
    g = np.random.default_rng(5).standard_normal(b.shape)
    if name == "duplicate":
        g[:, 2] = g[:, 0]
    if name == "zero_column":
        g[:, 1] = 0.0
    if name == "indefinite":
        g[:] = 0.25                     # a smooth start: the first directions already see the negative end of the spectrum
    return g, R.solve(a, b, x0=g, d=O.Pc.jacobi(a).inv_diag.copy() if jac else None, tol=TOL, max_iters=CAP)


# ---------------------------------------------------------------------------------------------------------------- Gram inputs
GRAM_SIZES = (1, 127, 128, 511, 512, 513, 1025, 531441)


def gram_inputs(n, k):
    g = np.random.default_rng(1000 * k + n % 9973)
    return g.standard_normal((n, k)), g.standard_normal((n, k)), g.uniform(0.5, 2.0, n)


def special_column(kind, n):
    if kind == "nan":
        return np.full(n, np.nan)
    if kind == "inf":
        v = np.ones(n); v[::3] = np.inf
        return v
    if kind == "negzero":
        return np.full(n, -0.0)
    v = np.full(n, 5e-324); v[::2] = -2.5e-310
    return v
