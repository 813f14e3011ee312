"""numpy restatement of additive Schwarz (src/preconditioner/asm.rs; kryst_amd/csrc/asm.hip).

Set-up: the uniform partition of asm.rs:46-56 with the reference's `capacity()` quirk; each index set sorted ascending (block Jacobi's
deviation 2); growth by `overlap` layers of the symmetrised graph of A (the labelled extension: row i's neighbours are the stored columns
of rows i of A and of A^T, i excluded); the owner of every row (the last un-grown set that contains it); the explicit inverses through
bjacobi_ref.gauss_jordan.  Apply: every subdomain's product from +0.0 in ascending j, each `*` and `+` rounded on its own, then z = 0 and
z[g] = z[g] + x_k in ascending subdomain order (asm.rs:77, :93-97); RAS keeps only the owner's product (0.0 + x).  The device gives these
bits."""
import numpy as np
import scipy.sparse as sp

import bjacobi_ref as BR

MAX_ROWS = 128


def uniform_parts(n, capacity):
    """asm.rs:46-56: p = max(capacity, 1) parts of chunk = ceil(n / p) rows, part i = [i chunk, min((i + 1) chunk, n)); trailing parts may
    be empty (an empty Rust range)."""
    p = max(int(capacity), 1)
    chunk = (n + p - 1) // p
    return [np.arange(min(i * chunk, n), min((i + 1) * chunk, n), dtype=np.int64) for i in range(p)]


def sorted_sets(sets):
    return [np.sort(np.asarray(g, dtype=np.int64).ravel()) for g in sets]


def adjacency_dense(n, row_ptr, col):
    """The symmetrised graph by brute force: D[i, j] when j is stored in row i or i in row j, i != j."""
    D = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr, dtype=np.int64)))
    D[rows, np.asarray(col, dtype=np.int64)] = True
    D |= D.T
    np.fill_diagonal(D, False)
    return D


def grow_dense(n, row_ptr, col, sets, overlap):
    D = adjacency_dense(n, row_ptr, col)
    out = []
    for g in sorted_sets(sets):
        m = np.zeros(n, dtype=bool)
        m[g] = True
        for _ in range(overlap):
            m = m | D[m].any(axis=0)
        out.append(np.nonzero(m)[0].astype(np.int64))
    return out


def grow(n, row_ptr, col, sets, overlap):
    """grow_dense through the sparse symmetrised pattern (operators too large for a dense n x n)."""
    rows = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr, dtype=np.int64)))
    S = sp.csr_matrix((np.ones(len(rows)), (rows, np.asarray(col, dtype=np.int64))), shape=(n, n))
    S = (S + S.T).tocsr()
    out = []
    for g in sorted_sets(sets):
        cur = g
        for _ in range(overlap):
            cur = np.union1d(cur, S[cur].indices).astype(np.int64)
        out.append(cur)
    return out


def owners(n, sets):
    own = np.full(n, -1, dtype=np.int64)
    for k, g in enumerate(sets):
        own[np.asarray(g, dtype=np.int64)] = k
    return own


def tiles(row_ptr, col, val, gs, chunk=1024):
    """Gauss-Jordan inverses of the sorted sets' matrices (bjacobi_ref.gauss_jordan, in chunks of equal size) -> (inv list, zero_pos list)"""
    inv, zp = [None] * len(gs), [-1] * len(gs)
    by = {}
    for k, g in enumerate(gs):
        by.setdefault(len(g), []).append(k)
    for b, ks in by.items():
        if b == 0:
            for k in ks:
                inv[k] = np.zeros((0, 0))
            continue
        for s in range(0, len(ks), chunk):
            part = ks[s:s + chunk]
            Bi, z = BR.gauss_jordan(np.stack([BR.block_matrix(row_ptr, col, val, gs[k]) for k in part]))
            for t, k in enumerate(part):
                inv[k], zp[k] = Bi[t], int(z[t])
    return inv, zp


def setup(a, sets=None, capacity=0, overlap=0, variant="as_written"):
    """-> (gs: the grown sorted sets, owner: last un-grown set per row, inv, zero_pos)"""
    n = a.nrows
    base = sorted_sets(uniform_parts(n, capacity) if sets is None or len(sets) == 0 else sets)
    own = owners(n, base)
    gs = base if variant == "as_written" else grow(n, a.row_ptr, a.col_idx, base, overlap)
    inv, zp = tiles(a.row_ptr, a.col_idx, a.vals, gs)
    return gs, own, inv, zp


class Apply:
    """z = M r of the restated preconditioner, vectorised over subdomains of equal size with the pinned order of every sum."""

    def __init__(self, n, gs, inv, owner=None, restricted=False):
        self.n = n
        lens = np.array([len(g) for g in gs], dtype=np.int64)
        self.off = np.zeros(len(gs) + 1, dtype=np.int64)
        np.cumsum(lens, out=self.off[1:])
        self.rows = np.concatenate(gs).astype(np.int64) if len(gs) else np.zeros(0, dtype=np.int64)
        self.groups = []
        for b in np.unique(lens):
            if b == 0:
                continue
            ks = np.nonzero(lens == b)[0]
            P = self.off[ks][:, None] + np.arange(b)[None, :]
            self.groups.append((np.stack([inv[k] for k in ks]), self.rows[P], P))
        if restricted:                         # each row with an owner: 0.0 + its position in the owner's grown set
            r = np.nonzero(owner >= 0)[0]
            o = owner[r]
            pos = np.array([self.off[k] + np.searchsorted(gs[k], row) for k, row in zip(o, r)], dtype=np.int64)
            self.passes = [(r, pos)]
        else:                                  # the t-th subdomain (ascending) of each row in pass t
            order = np.argsort(self.rows, kind="stable")
            srt = self.rows[order]
            first = np.searchsorted(srt, srt, side="left")
            rank = np.empty(len(order), dtype=np.int64)
            rank[order] = np.arange(len(order)) - first
            self.passes = [(self.rows[rank == t], np.nonzero(rank == t)[0]) for t in range(int(rank.max()) + 1 if len(rank) else 0)]

    def __call__(self, r):
        r = np.asarray(r, dtype=np.float64)
        X = np.empty(len(self.rows))
        for Bi, G, P in self.groups:
            X[P] = BR.apply_pinned(Bi, r[G])
        z = np.zeros(self.n)
        for rows, pos in self.passes:
            z[rows] = z[rows] + X[pos]
        return z


def apply_loop(n, gs, inv, r, owner=None, restricted=False):
    """The same apply written out as asm.rs:77-119 does it, one subdomain after another (small cases)."""
    z = np.zeros(n)
    xs = []
    for g, B in zip(gs, inv):
        x = np.zeros(len(g))
        for j in range(len(g)):
            x = x + B[:, j] * r[g[j]]
        xs.append(x)
    if restricted:
        for row in np.nonzero(owner >= 0)[0]:
            k = owner[row]
            z[row] = 0.0 + xs[k][np.searchsorted(gs[k], row)]
        return z
    for g, x in zip(gs, xs):
        for j, gi in enumerate(g):
            z[gi] = z[gi] + x[j]
    return z
