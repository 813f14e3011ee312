"""numpy restatement of the block Jacobi set-up (kryst_amd/csrc/block_jacobi.hip), vectorised over blocks.

Every step is the same IEEE operation, in the same order, as the device kernel: the block matrix from the sorted index set, Gauss-Jordan
with full pivoting in the textbook `gaussj` order (pivot = the first maximum of |B| over unpivoted rows and columns in row-major order),
each `*` and `-` rounded on its own, then the column swaps undone from the last step to the first.  The tiles it gives are therefore the
device's tiles bit for bit, and the CSR matrix M built from them turns the oracle's ApproxInv preconditioner (z = kro_spmv(M, r)) into
block Jacobi."""
import numpy as np


def gauss_jordan(B):
    """B: (nb, b, b) float64 -> (Binv (nb, b, b), zero_pos (nb,)): zero_pos[k] = -1, or the smallest position of block k not yet pivoted
    when its chosen pivot is 0 (its Binv rows are then meaningless)."""
    B = np.array(B, dtype=np.float64, copy=True)
    nb, b = B.shape[0], B.shape[1]
    ar = np.arange(nb)
    pivoted = np.zeros((nb, b), dtype=bool)
    alive = np.ones(nb, dtype=bool)
    zero_pos = np.full(nb, -1, dtype=np.int64)
    rows = np.zeros((nb, b), dtype=np.int64)
    cols = np.zeros((nb, b), dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(b):
            A = np.where(pivoted[:, :, None] | pivoted[:, None, :], -1.0, np.abs(B))
            k = np.argmax(A.reshape(nb, -1), axis=1)          # first maximum in row-major order = the strict ">" scan
            p, q = k // b, k % b
            newly = alive & (B[ar, p, q] == 0.0)
            zero_pos[newly] = np.argmin(pivoted[newly], axis=1)
            alive &= ~newly
            go = alive
            B2 = B.copy()
            rp, rq = B[ar, p, :].copy(), B[ar, q, :].copy()
            B2[ar, p, :] = rq
            B2[ar, q, :] = rp
            pivinv = 1.0 / B2[ar, q, q]
            B2[ar, q, q] = 1.0
            B2[ar, q, :] = B2[ar, q, :] * pivinv[:, None]
            rowq = B2[ar, q, :].copy()
            f = B2[ar, :, q].copy()
            Bz = B2.copy()
            Bz[ar, :, q] = 0.0
            upd = Bz - rowq[:, None, :] * f[:, :, None]
            upd[ar, q, :] = rowq
            B = np.where(go[:, None, None], upd, B)
            rows[go, s], cols[go, s] = p[go], q[go]
            pivoted[ar[go], q[go]] = True
        for s in range(b - 1, -1, -1):
            r_s, c_s = rows[:, s], cols[:, s]
            cr, cc = B[ar, :, r_s].copy(), B[ar, :, c_s].copy()
            B[ar, :, r_s] = cc
            B[ar, :, c_s] = cr
    return B, zero_pos


def block_matrix(row_ptr, col, val, g):
    """B[i][j] = A(g[i], g[j]) if stored, else +0.0 (g sorted ascending)."""
    b = len(g)
    B = np.zeros((b, b))
    for i, r in enumerate(g):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        c = np.asarray(col[lo:hi], dtype=np.int64)
        pos = np.searchsorted(g, c)
        ok = (pos < b) & (g[np.minimum(pos, b - 1)] == c)
        B[i, pos[ok]] = np.asarray(val[lo:hi])[ok]
    return B


def uniform_blocks(n, bsize):
    return [np.arange(s, min(s + bsize, n), dtype=np.int64) for s in range(0, n, bsize)]


def tiles_of(row_ptr, col, val, blocks):
    """Restated tiles of the (sorted) blocks, inverted in groups of equal size -> (list of Binv, list of zero_pos)."""
    gs = [np.sort(np.asarray(g, dtype=np.int64)) for g in blocks]
    inv = [None] * len(gs)
    zp = [-1] * len(gs)
    by_size = {}
    for k, g in enumerate(gs):
        by_size.setdefault(len(g), []).append(k)
    for b, ks in by_size.items():
        if b == 0:
            for k in ks:
                inv[k] = np.zeros((0, 0))
            continue
        Bs = np.stack([block_matrix(row_ptr, col, val, gs[k]) for k in ks])
        Bi, z = gauss_jordan(Bs)
        for t, k in enumerate(ks):
            inv[k], zp[k] = Bi[t], int(z[t])
    return gs, inv, zp


def tiles_uniform(row_ptr, col, val, n, bsize):
    """The contiguous form without a Python loop over blocks: the full blocks through one scatter, the short last block on its own."""
    nfull = n // bsize
    out = []
    rp = np.asarray(row_ptr, dtype=np.int64)
    c = np.asarray(col, dtype=np.int64)
    v = np.asarray(val, dtype=np.float64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    if nfull:
        B = np.zeros((nfull, bsize, bsize))
        m = (r // bsize == c // bsize) & (r < nfull * bsize)
        B[r[m] // bsize, r[m] % bsize, c[m] % bsize] = v[m]
        Bi, z = gauss_jordan(B)
        out.append((Bi, z))
    if n % bsize:
        g = np.arange(nfull * bsize, n, dtype=np.int64)
        Bi, z = gauss_jordan(block_matrix(rp, c, v, g)[None])
        out.append((Bi, z))
    inv = [t for Bi, _ in out for t in Bi]
    zp = [int(x) for _, z in out for x in z]
    return uniform_blocks(n, bsize), inv, zp


def m_ref(n, gs, inv):
    """M as CSR (row_ptr, col, val): row g[i] of the last block containing it holds (g[j], Binv[i][j]) for all j; other rows empty."""
    owner = np.full(n, -1, dtype=np.int64)
    pos = np.full(n, -1, dtype=np.int64)
    for k, g in enumerate(gs):
        owner[g] = k
        pos[g] = np.arange(len(g))
    lens = np.array([len(gs[k]) if k >= 0 else 0 for k in owner], dtype=np.int64)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.empty(rp[-1], dtype=np.int64)
    va = np.empty(rp[-1], dtype=np.float64)
    for r in np.nonzero(owner >= 0)[0]:
        k, i = owner[r], pos[r]
        ci[rp[r]:rp[r + 1]] = gs[k]
        va[rp[r]:rp[r + 1]] = inv[k][i, :]
    return rp, ci, va


def m_ref_uniform(n, bsize, inv):
    """m_ref for the contiguous form, vectorised."""
    rows = np.arange(n, dtype=np.int64)
    k = rows // bsize
    lo = k * bsize
    lens = np.minimum(bsize, n - lo)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rp[1:])
    nfull = n // bsize
    ci = np.empty(rp[-1], dtype=np.int64)
    va = np.empty(rp[-1], dtype=np.float64)
    if nfull:
        T = np.stack(inv[:nfull])                              # (nfull, b, b): row i of block k
        ci[:nfull * bsize * bsize] = (np.arange(nfull * bsize)[:, None] // bsize * bsize + np.arange(bsize)[None, :]).ravel()
        va[:nfull * bsize * bsize] = T.reshape(-1)
    if n % bsize:
        g = np.arange(nfull * bsize, n)
        t = inv[-1]
        ci[nfull * bsize * bsize:] = np.tile(g, len(g))
        va[nfull * bsize * bsize:] = t.reshape(-1)
    return rp, ci, va


def apply_pinned(Binv, rg):
    """Binv (nb, b, b), rg (nb, b) = r|_g -> z|_g (nb, b) in the pinned order: from +0.0, ascending j, each product added on its own."""
    s = np.zeros(rg.shape)
    for j in range(rg.shape[1]):
        s = s + Binv[:, :, j] * rg[:, j][:, None]
    return s


def stencil7_rows(N, kind, rows):
    """Rows `rows` of the oracle's 7-point operator (oracle.stencil7, kinds poisson / aniso) as CSR with global columns, without forming
    the whole operator (the full-size test takes 4 096 blocks of the 512^3 operator)."""
    if kind == "poisson":
        coef = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
    elif kind == "aniso":
        cx, cy, cz = 1.0, 1.0, 0.01
        coef = np.array([-cz, -cy, -cx, 2.0 * (cx + cy + cz), -cx, -cy, -cz])
    else:
        raise ValueError(kind)
    rows = np.asarray(rows, dtype=np.int64)
    N2 = N * N
    i = rows % N; j = (rows // N) % N; k = rows // N2
    offs = np.array([-N2, -N, -1, 0, 1, N, N2], dtype=np.int64)
    valid = np.stack([k > 0, j > 0, i > 0, np.ones_like(i, bool), i < N - 1, j < N - 1, k < N - 1], axis=1)
    cols = rows[:, None] + offs[None, :]
    vals = np.broadcast_to(coef, cols.shape)
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(valid.sum(axis=1), out=rp[1:])
    return rp, cols[valid], vals[valid]
