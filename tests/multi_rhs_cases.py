"""Case builders for the multiple-right-hand-side tests, shared by the CPU tier (test_multi_rhs_cpu.py: the fixtures checked on the oracle
alone) and the GPU tier (test_gpu_multi_rhs.py: batched calls against the single-vector calls and the oracle, bit for bit).

Everything here is numpy and the oracle; nothing touches the device."""
import functools

import numpy as np

from oracle import oracle as O

SPEC = (256, 2, 1024)            # the published reduce spec (kryst_reduce_spec): threads per tile, elements per thread, threads of the final fold
WIDTHS = (2, 4, 8)


def rs():
    return O.Reduce.tiled(*SPEC)


# ------------------------------------------------------------------------------------------------ packing (what MultiVec.from_numpy / to_numpy do)
def pack_colmajor(a, ld=None):
    """(n, m) array -> flat buffer with column j at [j * ld, j * ld + n), ld >= n; the gaps hold NaN so that nobody reads them unnoticed"""
    a = np.asarray(a, dtype=np.float64)
    n, m = a.shape
    ld = n if ld is None else ld
    assert ld >= n
    buf = np.full(ld * m, np.nan)
    for j in range(m):
        buf[j * ld:j * ld + n] = a[:, j]
    return buf


def unpack_colmajor(buf, n, m, ld=None):
    ld = n if ld is None else ld
    return np.stack([buf[j * ld:j * ld + n] for j in range(m)], axis=1) if m else np.empty((n, 0))


def interleave(a):
    """the device layout: element (i, j) at i * m + j"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).ravel()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ------------------------------------------------------------------------------------------------ operators for the SpMM
def _csr(nrows, ncols, rows):
    """rows: list of (sorted unique column array, value array)"""
    rp = np.zeros(nrows + 1, dtype=np.int64)
    for i, (c, _) in enumerate(rows):
        rp[i + 1] = rp[i] + len(c)
    ci = np.concatenate([c for c, _ in rows]).astype(np.int64) if rp[-1] else np.zeros(0, dtype=np.int64)
    va = np.concatenate([v for _, v in rows]).astype(np.float64) if rp[-1] else np.zeros(0)
    return O.Csr(nrows, ncols, rp, ci, va)


def banded(n, seed=11):
    """n x n, up to five diagonals (-7, -1, 0, +1, +3) with random values: n = 1, 127, 128, 511, 512, 513, 1025 cross every tile / wave edge"""
    g = np.random.default_rng(seed + n)
    rows = []
    for i in range(n):
        c = np.array(sorted({j for j in (i - 7, i - 1, i, i + 1, i + 3) if 0 <= j < n}), dtype=np.int64)
        rows.append((c, g.standard_normal(len(c))))
    return _csr(n, n, rows)


def ragged(n=2003, seed=5):
    """about 2 000 rows of 0 .. 40 entries at random columns; every seventh row and a run of 130 rows (a whole wave's slice) are empty"""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cnt = 0 if (i % 7 == 3 or 1024 <= i < 1154) else int(g.integers(1, 41))
        c = np.sort(g.choice(n, size=cnt, replace=False)).astype(np.int64)
        rows.append((c, g.standard_normal(cnt)))
    return _csr(n, n, rows)


def long_rows(seed=6):
    """600 x 3200: rows 101 (the second row of its lane) and 514 hold 3 000 entries each -- several LDS windows -- between short rows"""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(600):
        if i in (101, 514):
            c = np.sort(g.choice(3200, size=3000, replace=False)).astype(np.int64)
        else:
            c = np.sort(g.choice(3200, size=int(g.integers(0, 5)), replace=False)).astype(np.int64)
        rows.append((c, g.standard_normal(len(c))))
    return _csr(600, 3200, rows)


def rectangular(seed=7):
    """700 x 300, 1 .. 9 entries per row"""
    g = np.random.default_rng(seed)
    rows = []
    for _ in range(700):
        c = np.sort(g.choice(300, size=int(g.integers(1, 10)), replace=False)).astype(np.int64)
        rows.append((c, g.standard_normal(len(c))))
    return _csr(700, 300, rows)


SPMM_OPERATORS = {
    **{f"banded{n}": functools.partial(banded, n) for n in (1, 127, 128, 511, 512, 513, 1025)},
    "ragged": ragged, "long_rows": long_rows, "rect700x300": rectangular,
    **{f"stencil{N}_{kind}": functools.partial(O.stencil7, N, kind) for N in (8, 12, 16) for kind in ("poisson", "convdiff")},
}


def xcols(n, k, seed=21):
    return np.random.default_rng(seed + 131 * k + n).standard_normal((n, k))


def oracle_spmm(a, x):
    return np.stack([a.spmv(np.ascontiguousarray(x[:, j])) for j in range(x.shape[1])], axis=1)


SPECIAL_COLUMNS = ("nan", "inf", "negzero", "denormal")


def special_column(kind, n):
    if kind == "nan":
        return np.full(n, np.nan)
    if kind == "inf":
        v = np.ones(n); v[::3] = np.inf; v[1::5] = -np.inf
        return v
    if kind == "negzero":
        return np.full(n, -0.0)
    v = np.full(n, 5e-324); v[::2] = -2.5e-310
    return v


# ------------------------------------------------------------------------------------------------ solver fixtures
TOL, CAP = 1e-8, 200
ERR_INDEFINITE_MATRIX, ERR_INDEFINITE_PC = 3, 4


@functools.lru_cache(maxsize=None)
def block600():
    """A = diag(T, -T), T = tridiag(-1, 2, -1) of 300 rows: 600 rows cross a tile edge, one half is indefinite"""
    n = 300
    t = O.tridiag(n, -1.0, 2.0, -1.0)
    a = np.zeros((2 * n, 2 * n))
    a[:n, :n] = t
    a[n:, n:] = -t
    return O.Csr.from_dense(a, keep_zeros=False)


@functools.lru_cache(maxsize=None)
def block600_columns():
    """the eight right-hand sides of the issue, (600, 8)"""
    n = 300
    a = block600()
    u = O.splitmix64_uniform
    z = np.zeros(n)
    c3 = u(0xB10C + 2, 2 * n).copy(); c3[n:] *= 1e-3
    c6 = u(0xB10C + 5, n)
    cols = [a.spmv(np.concatenate([np.ones(n), z])),                     # A 1 on the first block
            np.concatenate([z, u(0xB10C + 1, n)]),                       # random on the second (negative definite) block
            c3,                                                          # random, the second block x 1e-3
            np.zeros(2 * n),                                             # zero
            np.concatenate([np.sin(np.pi * np.arange(1, n + 1) / (n + 1)), z]),   # the first block's lowest eigenvector
            np.concatenate([c6, z]),                                     # random on the first block
            np.concatenate([c6[::-1] * 1e6, z]),                         # the same reversed x 1e6
            u(0x5EED, 2 * n)]                                            # fully random
    return np.stack(cols, axis=1)


# (status, iterations, converged) per column, what the CPU oracle gives with the tiled reduce (asserted in test_multi_rhs_cpu.py)
BLOCK600_EXPECT = {
    "cg": [(0, 150, True), (3, 1, False), (3, 6, False), (3, 1, False), (0, 1, True), (0, 200, True), (0, 200, True), (3, 2, False)],
    "pcg": [(0, 150, True), (3, 1, False), (0, 200, True), (3, 1, False), (0, 1, True), (0, 200, True), (0, 200, True), (4, 1, False)],
}

# (N, kind, method, pc)
STENCIL_CASES = [(8, "poisson", "cg", None), (8, "poisson", "pcg", "jacobi"), (8, "aniso", "pcg", "jacobi"),
                 (12, "poisson", "cg", None), (12, "poisson", "pcg", "jacobi"), (12, "aniso", "pcg", "jacobi")]


@functools.lru_cache(maxsize=None)
def stencil(N, kind):
    return O.stencil7(N, kind)


@functools.lru_cache(maxsize=None)
def stencil_columns(N, kind, m=8):
    """A 1 plus m - 1 splitmix columns, column j scaled by 10^(j - 3)"""
    a = stencil(N, kind)
    return np.stack([a.spmv(np.ones(a.nrows))] + [O.splitmix64_uniform(0x5EED + j, a.nrows) * 10.0 ** (j - 3) for j in range(1, m)], axis=1)


def guesses(n, m, seed=77):
    """x0 != 0, another one per column"""
    return np.random.default_rng(seed).standard_normal((n, m))


def oracle_pc(a, pc):
    return {None: lambda a: None, "identity": lambda a: O.Pc.identity(), "jacobi": O.Pc.jacobi}[pc](a)


def oracle_columns(method, a, b, x0=None, pc=None, tol=TOL, max_iters=CAP, norm_type=1):
    """the reference per column: a list of oracle Results (code, iterations, final_residual, converged, history, x; x = x0 on an error)"""
    out = []
    opc = oracle_pc(a, pc)
    for j in range(b.shape[1]):
        start = None if x0 is None else np.ascontiguousarray(x0[:, j])
        r = O.solve(method, a, np.ascontiguousarray(b[:, j]), x0=start, pc=opc, tol=tol, max_iters=max_iters, norm_type=norm_type, rs=rs(),
                    raise_on_error=False)
        if r.code != 0:                                   # on Err the reference never reaches `*x = ...`
            r.x = np.zeros(a.nrows) if start is None else start.copy()
        out.append(r)
    return out
