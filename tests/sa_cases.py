"""Operators shared by the AMG and SPAI tests: the 27-point box operator, a graph Laplacian with a hub row, Poisson with Dirichlet
identity rows and stored zeros, and a diagonal matrix."""
import numpy as np

from oracle import oracle as O


def op27(N, seed):
    """A nonsymmetric 27-point box operator on an N^3 grid: off-diagonals -U(0.5, 1.5), diagonal 27 + U(0, 1)."""
    rng = np.random.default_rng(seed)
    n = N ** 3
    r = np.arange(n)
    i, j, k = r % N, (r // N) % N, r // (N * N)
    cols, vals = [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                ok = (i + di >= 0) & (i + di < N) & (j + dj >= 0) & (j + dj < N) & (k + dk >= 0) & (k + dk < N)
                c = np.where(ok, r + di + N * (dj + N * dk), -1)
                v = 27.0 + rng.random(n) if (di, dj, dk) == (0, 0, 0) else -(0.5 + rng.random(n))
                cols.append(c); vals.append(v)
    C = np.stack(cols, 1); V = np.stack(vals, 1)
    keep = C >= 0
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(1), out=rp[1:])
    return O.Csr(n, n, rp, C[keep], V[keep])


def _sym_csr(n, ei, ej, w, diag):
    """symmetric CSR from undirected edges (i, j, w), duplicates merged, plus the diagonal; columns ascending."""
    r = np.concatenate([ei, ej, np.arange(n)])
    c = np.concatenate([ej, ei, np.arange(n)])
    v = np.concatenate([-w, -w, diag])
    key = r * n + c
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    u, first = np.unique(key, return_index=True)
    vs = np.zeros(len(u))
    for q in range(int(np.max(np.diff(np.append(first, len(key)))))):   # merge duplicates left to right
        idx = first + q
        ok = idx < np.append(first[1:], len(key))
        vs[ok] = vs[ok] + v[idx[ok]]
    rows, cols = u // n, u % n
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return O.Csr(n, n, rp, cols, vs)


def graph_laplacian(n, seed, hub=1000, shift=1.0):
    """weighted graph Laplacian + shift I: irregular degrees (1 to about 12 random neighbours a node) and node 0 joined to `hub` others,
    weights U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    deg = rng.geometric(0.3, n).clip(1, 12)
    ei = np.repeat(np.arange(n), deg)
    ej = rng.integers(0, n, len(ei))
    hj = rng.choice(np.arange(1, n), hub, replace=False)
    ei = np.concatenate([ei, np.zeros(hub, dtype=np.int64)]); ej = np.concatenate([ej, hj])
    keep = ei != ej
    ei, ej = ei[keep], ej[keep]
    w = 0.5 + rng.random(len(ei))
    wsum = np.zeros(n)
    np.add.at(wsum, ei, w); np.add.at(wsum, ej, w)
    return _sym_csr(n, ei, ej, w, wsum + shift)


def dirichlet_poisson(N):
    """Poisson N^3 whose boundary rows are identity rows; every coupling to or from a boundary node is kept as a stored 0.0."""
    a = O.stencil7(N)
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    idx = lambda r: (r % N, (r // N) % N, r // (N * N))
    bnd = np.zeros(a.nrows, dtype=bool)
    for t in idx(np.arange(a.nrows)):
        bnd |= (t == 0) | (t == N - 1)
    v = a.vals.copy()
    diag = a.col_idx == rows
    v[(bnd[rows] | bnd[a.col_idx]) & ~diag] = 0.0
    v[bnd[rows] & diag] = 1.0
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


def diagonal(n, seed=0):
    d = 1.0 + np.random.default_rng(seed).random(n)
    return O.Csr(n, n, np.arange(n + 1), np.arange(n), d)
