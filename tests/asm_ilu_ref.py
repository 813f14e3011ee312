"""Restatement of additive Schwarz with ILU(0) subdomain solves (kryst_amd/csrc/asm_ilu.hip), composed from the
oracle: the sets, growth and owners of asm_ref; S_k = A[g_k, g_k] in the sorted order of g_k with every stored entry kept (explicit zeros
included) and the columns outside g_k dropped; the oracle's own `Pc.ilup0(S_k)` / `Pc.ilu0_true(S_k)` and their apply (tri_apply with
divide_diag = 1); the combine of asm_ref.apply_loop: z = 0, then z[g] = z[g] + x_k in ascending subdomain order, RAS 0.0 + x of the owner.
The device gives these bits."""
import numpy as np

from oracle import oracle as O
import asm_ref as A

MAX_ROWS = 16384
MODES = {"ilup0": O.Pc.ilup0, "ilu0": O.Pc.ilu0_true}


def submatrix(a, g):
    """S = A[g, g] for a sorted index set g -> O.Csr in local indices (stored order kept: ascending columns)"""
    g = np.asarray(g, dtype=np.int64)
    b = len(g)
    rp = np.asarray(a.row_ptr, dtype=np.int64)
    lens = rp[g + 1] - rp[g]
    src = np.repeat(rp[g] - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(int(lens.sum()))
    rows = np.repeat(np.arange(b), lens)
    cols = np.asarray(a.col_idx, dtype=np.int64)[src]
    pos = np.minimum(np.searchsorted(g, cols), max(b - 1, 0))
    keep = g[pos] == cols if b else np.zeros(0, dtype=bool)
    sp = np.zeros(b + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=b), out=sp[1:])
    return O.Csr(b, b, sp, pos[keep], np.asarray(a.vals, dtype=np.float64)[src][keep])


def block_diagonal(a, gs):
    """A with every entry outside the blocks gs x gs dropped (disjoint contiguous parts that cover all rows)"""
    part = np.empty(a.nrows, dtype=np.int64)
    for k, g in enumerate(gs):
        part[g] = k
    rp = np.asarray(a.row_ptr, dtype=np.int64)
    rows = np.repeat(np.arange(a.nrows), np.diff(rp))
    cols = np.asarray(a.col_idx, dtype=np.int64)
    keep = part[rows] == part[cols]
    out = np.zeros(a.nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=a.nrows), out=out[1:])
    return O.Csr(a.nrows, a.nrows, out, cols[keep], np.asarray(a.vals, dtype=np.float64)[keep])


def factor_values(pc):
    """the factors on S's pattern as one array: l_ij below the diagonal, u_ij on and above it"""
    s = pc.a
    rows = np.repeat(np.arange(s.nrows), np.diff(np.asarray(s.row_ptr, dtype=np.int64)))
    return np.where(np.asarray(s.col_idx, dtype=np.int64) < rows, pc.lfac, pc.ufac)


def levels(s, w):
    """every row's level (from 1) in the forward and in the backward sweep over the kept (non-zero) entries"""
    n = s.nrows
    rp, col = np.asarray(s.row_ptr, dtype=np.int64), np.asarray(s.col_idx, dtype=np.int64)
    ll, lu = np.ones(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    for i in range(n):
        c, v = col[rp[i]:rp[i + 1]], w[rp[i]:rp[i + 1]]
        d = c[(c < i) & (v != 0.0)]
        if len(d):
            ll[i] = 1 + ll[d].max()
    for i in range(n - 1, -1, -1):
        c, v = col[rp[i]:rp[i + 1]], w[rp[i]:rp[i + 1]]
        d = c[(c > i) & (v != 0.0)]
        if len(d):
            lu[i] = 1 + lu[d].max()
    return ll, lu


def combine_loop(n, gs, xs, owner=None, restricted=False):
    """the combine of asm_ref.apply_loop, one subdomain after another"""
    z = np.zeros(n)
    if restricted:
        for row in np.nonzero(owner >= 0)[0]:
            k = owner[row]
            z[row] = 0.0 + xs[k][np.searchsorted(gs[k], row)]
        return z
    for g, x in zip(gs, xs):
        for j, gi in enumerate(g):
            z[gi] = z[gi] + x[j]
    return z


class Setup:
    """sets (given or uniform), growth, owners, the oracle's factorisation of every submatrix"""

    def __init__(self, a, sets=None, capacity=0, overlap=0, variant="as_written", mode="ilu0"):
        self.n = a.nrows
        base = A.sorted_sets(A.uniform_parts(a.nrows, capacity) if sets is None or len(sets) == 0 else sets)
        self.owner = A.owners(a.nrows, base)
        self.gs = base if variant == "as_written" else A.grow(a.nrows, a.row_ptr, a.col_idx, base, overlap)
        self.restricted = variant == "restricted"
        self.subs = [submatrix(a, g) for g in self.gs]
        self.pcs = [MODES[mode](s) if s.nrows else None for s in self.subs]
        # the combine, pass by pass: the t-th subdomain (ascending) of each row in pass t (asm_ref.Apply)
        rows = np.concatenate(self.gs).astype(np.int64) if len(self.gs) else np.zeros(0, dtype=np.int64)
        self.off = np.zeros(len(self.gs) + 1, dtype=np.int64)
        np.cumsum([len(g) for g in self.gs], out=self.off[1:])
        if self.restricted:
            r = np.nonzero(self.owner >= 0)[0]
            pos = np.array([self.off[k] + np.searchsorted(self.gs[k], row) for k, row in zip(self.owner[r], r)], dtype=np.int64)
            self.passes = [(r, pos)]
        else:
            order = np.argsort(rows, kind="stable")
            srt = rows[order]
            rank = np.empty(len(order), dtype=np.int64)
            rank[order] = np.arange(len(order)) - np.searchsorted(srt, srt, side="left")
            self.passes = [(rows[rank == t], np.nonzero(rank == t)[0]) for t in range(int(rank.max()) + 1 if len(rank) else 0)]

    def products(self, r):
        r = np.asarray(r, dtype=np.float64)
        return [pc.apply(r[g]) if pc is not None else np.zeros(0) for g, pc in zip(self.gs, self.pcs)]

    def __call__(self, r):
        xs = self.products(r)
        X = np.concatenate(xs) if xs else np.zeros(0)
        z = np.zeros(self.n)
        for rows, pos in self.passes:
            z[rows] = z[rows] + X[pos]
        return z

    def apply_loop(self, r):
        return combine_loop(self.n, self.gs, self.products(r), self.owner, self.restricted)
