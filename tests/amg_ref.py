"""numpy restatement of AMG as written (src/preconditioner/amg.rs; kryst_amd/csrc/amg_setup.cpp and amg.hip).

`amg_new_dense` is a line-by-line dense transliteration of AMG::new (:73-118) with its helpers (:447-818).  The reference forms the
coarse operator with faer's dense product, whose summation order is faer's own; the restatement fixes it as the library does:
(R A) P, every entry summed over the inner index in ascending order from 0.0.  `vcycle` restates apply_recursive (:200-250) on CSR
levels with oracle.Csr.spmv (ascending stored columns, separate mul and add: the device SpMV's arithmetic) and the reference's
element-wise expressions, so it gives the device's bits on the same hierarchy.  `pcg` restates PcgSolver::solve (pcg.rs) with the
preconditioner's z carried from one apply to the next, as the reference's solver holds it."""
import numpy as np

from oracle import oracle as O


# --------------------------------------------------------------------------- set-up, dense (amg.rs:73-818)

def diag_inverse(m):                                   # :139-170
    d = np.diag(m).copy()
    return np.where(np.abs(d) < 1e-14, 0.0, 1.0 / np.where(d == 0.0, 1.0, d))


def adaptive_threshold(a, base):                       # :447-498
    n = a.shape[0]
    s = 0.0
    for i in range(n):
        mx = 0.0
        for j in range(n):
            if j != i:
                mx = max(mx, abs(a[i, j]))
        s += mx / abs(a[i, i]) if abs(a[i, i]) > 1e-14 else 0.0
    avg = s / n if n else 1.0
    return base * (1.0 + max(avg, 0.5))


def strength(a, thr):                                  # :605-658
    n = a.shape[0]
    s = np.zeros((n, n))
    for i in range(n):
        aii = abs(a[i, i])
        for j in range(n):
            if i == j:
                continue
            ajj = abs(a[j, j])
            if aii > 1e-14 and ajj > 1e-14:
                st = abs(a[i, j]) / np.sqrt(aii * ajj)
                if st > thr:
                    s[i, j] = st
    return s


def pairwise(s):                                       # :707-747
    n = s.shape[0]
    agg = [None] * n
    visited = [False] * n
    aid = 0
    for i in range(n):
        if visited[i]:
            continue
        best, nb = 0.0, None
        for j in range(n):
            if i != j and not visited[j] and s[i, j] > best:
                best, nb = s[i, j], j
        agg[i] = aid; visited[i] = True
        if nb is not None:
            agg[nb] = aid; visited[nb] = True
        aid += 1
    return agg


def coarse_graph(s, agg):                              # :752-771
    nc = max(agg) + 1
    g = np.zeros((nc, nc))
    for i in range(s.shape[0]):
        for j in range(s.shape[1]):
            if s[i, j] != 0.0:
                g[agg[i], agg[j]] += s[i, j]
    return g


def matmul_ordered(x, y):
    """x @ y with every entry summed over the inner index in ascending order from 0.0 (numpy's matmul may block or fuse)."""
    out = np.zeros((x.shape[0], y.shape[1]))
    for k in range(x.shape[1]):
        out = out + np.multiply.outer(x[:, k], y[k, :])
    return out


def amg_new_dense(a, max_levels, base):
    """AMG::new(a, max_levels, base_threshold) -> list of levels {A, P, R, dinv, agg, threshold} (P / R / agg None on the last)."""
    levels = []
    cur = np.array(a, dtype=np.float64)
    cur_d = diag_inverse(cur)
    for _ in range(max_levels):
        n = cur.shape[0]
        if n <= 10:
            break
        thr = adaptive_threshold(cur, base)
        s = strength(cur, thr)
        first = pairwise(s)
        second = pairwise(coarse_graph(s, first))
        agg = np.array([second[f] for f in first])
        nc = int(agg.max()) + 1
        p0 = np.zeros((n, nc))
        p0[np.arange(n), agg] = 1.0
        r = p0.T.copy()
        p = p0.copy()
        smooth_interpolation(p, cur, 0.5)
        minimize_energy(p)
        coarse = matmul_ordered(matmul_ordered(r, cur), p)
        levels.append(dict(A=cur, P=p, R=r, dinv=cur_d, agg=agg, threshold=thr))
        cur = coarse
        cur_d = diag_inverse(cur)
    levels.append(dict(A=cur, P=None, R=None, dinv=cur_d, agg=None, threshold=None))
    return levels


def smooth_interpolation(p, m, weight):                # :502-525
    for j in range(min(p.shape[1], m.shape[1])):
        for i in range(min(p.shape[0], m.shape[0])):
            p[i, j] -= weight * m[i, j]


def minimize_energy(p):                                # :529-565
    for i in range(p.shape[0]):
        ss = 0.0
        for v in p[i]:
            ss += v * v
        nf = np.sqrt(ss) if abs(ss) > 1e-14 else 1.0
        p[i] = p[i] / nf


# --------------------------------------------------------------------------- apply (amg.rs:171-312)

def to_csr(m):
    return O.Csr.from_dense(m, keep_zeros=False)


def csr_levels(levels):
    """dense levels -> CSR levels (stored entries only) for `vcycle`."""
    out = []
    for L in levels:
        out.append(dict(A=to_csr(L["A"]), P=None if L["P"] is None else to_csr(L["P"]),
                        R=None if L["R"] is None else to_csr(L["R"]), dinv=np.asarray(L["dinv"], dtype=np.float64)))
    return out


def solve_direct(a, r):                                # :254-312
    n = len(r)
    x = np.zeros(n); res = r.copy(); p = res.copy()
    sdot = lambda u, v: O.dot(u, v, O.SERIAL)
    rr_new = sdot(res, res)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(n):
            ap = a.spmv(p)
            alpha = np.float64(rr_new) / np.float64(sdot(p, ap))
            x = x + alpha * p
            res = res - alpha * ap
            rr_old = rr_new
            rr_new = sdot(res, res)
            if np.sqrt(rr_new) < 1e-10:
                break
            beta = np.float64(rr_new) / np.float64(rr_old)
            p = res + beta * p
    return x


def smooth(a, dinv, r, z, iters):                      # :174-196
    for _ in range(iters):
        t = a.spmv(z)
        t = r - t
        z = z + dinv * t
    return z


def vcycle(levels, r, z, level=0, nu_pre=1, nu_post=1, coarse=None):
    """apply_recursive(level, r, z) (:200-250) -> the new z.  `coarse(r) -> z` solves on the last level (default: solve_direct)."""
    L = levels[level]
    if level + 1 == len(levels):
        return solve_direct(L["A"], r) if coarse is None else coarse(r)
    a, dinv = L["A"], L["dinv"]
    z = smooth(a, dinv, r, np.array(z, dtype=np.float64), nu_pre)
    az = r - a.spmv(z)
    rc = L["R"].spmv(az)
    zc = vcycle(levels, rc, np.zeros(len(rc)), level + 1, nu_pre, nu_post, coarse)
    z = z + L["P"].spmv(zc)
    return smooth(a, dinv, r, z, nu_post)


# --------------------------------------------------------------------------- PCG with the AMG apply (pcg.rs)

def pcg(a, levels, b, tol, max_iters, rs, apply=None):
    """PcgSolver::solve with norm Unpreconditioned -> (x, iterations, code, history); code 0, 3 (IndefiniteMatrix) or 4
    (IndefinitePreconditioner).  `apply(r, z) -> z` is the preconditioner (default: the as-written V-cycle on `levels`)."""
    n = len(b)
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    if apply is None:
        apply = lambda r, z: vcycle(levels, r, z)
    x = np.zeros(n)
    r = b - a.spmv(x)
    z = apply(r, np.zeros(n))
    p = z.copy()
    rz = dot(r, z)
    hist = [np.sqrt(dot(r, r))]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        res0 = np.sqrt(abs(rz))
        for i in range(max_iters):
            ap = a.spmv(p)
            pap = dot(p, ap)
            if not pap > 0.0:
                if pap <= 0.0:
                    return x, i + 1, 3, hist
            alpha = rz / pap
            x = x + alpha * p
            r = r - alpha * ap
            z = apply(r, z)
            rz_new = dot(r, z)
            res = np.sqrt(dot(r, r))
            hist.append(res)
            if res / res0 <= tol or i + 1 >= max_iters:
                return x, i + 1, 0, hist
            beta = rz_new / rz
            if beta < 0.0:                             # indefinite-preconditioner exit
                return x, i + 1, 4, hist
            p = z + beta * p
            rz = rz_new
    return x, max_iters, 0, hist


# --------------------------------------------------------------------------- smoothed aggregation (labelled extension; amg.hip sa_*)

def sa_key(i):
    """the hashed MIS priority: (hash32(i) << 32) | i"""
    h = np.asarray(i, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = (h * np.uint32(0x9E3779B1)).astype(np.uint32)
        h ^= h >> np.uint32(16); h = (h * np.uint32(0x85EBCA6B)).astype(np.uint32)
        h ^= h >> np.uint32(13); h = (h * np.uint32(0xC2B2AE35)).astype(np.uint32)
        h ^= h >> np.uint32(16)
    return (h.astype(np.uint64) << np.uint64(32)) | np.asarray(i, dtype=np.uint64)


def sa_aggregates(a, theta=0.0, with_roots=False):
    """distance-2 MIS with hashed priorities, root neighbourhoods, then leftover attachment; singletons numbered after the roots.
    with_roots: -> (agg, roots), roots[g] the root row of aggregate g < len(roots)."""
    n = a.nrows
    rp = np.asarray(a.row_ptr); ci = np.asarray(a.col_idx); va = np.asarray(a.vals)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n); dm = ci == rows; d[rows[dm]] = va[dm]
    strong = (ci != rows) & (np.abs(va) > theta * np.sqrt(np.abs(d[rows] * d[ci])))
    sr, sc = rows[strong], ci[strong]
    key = sa_key(np.arange(n))
    state = np.zeros(n, dtype=np.int8)

    def nbmax(v):
        out = v.copy(); np.maximum.at(out, sr, v[sc]); return out

    def nbany(v):
        out = v.copy(); np.logical_or.at(out, sr, v[sc]); return out

    while True:
        m2 = nbmax(nbmax(np.where(state == 0, key, np.uint64(0))))
        state[(state == 0) & (m2 == key)] = 1
        f2 = nbany(nbany(state == 1))
        state[(state == 0) & f2] = 2
        if not np.any(state == 0):
            break
    roots = np.flatnonzero(state == 1)
    rid = -np.ones(n, dtype=np.int64); rid[roots] = np.arange(len(roots))

    def first_with(src):                       # per row: src of the first strong neighbour (stored order) with src >= 0
        out = -np.ones(n, dtype=np.int64)
        for i in range(n):
            for k in range(rp[i], rp[i + 1]):
                if strong[k] and src[ci[k]] >= 0:
                    out[i] = src[ci[k]]; break
        return out

    a1 = np.where(state == 1, rid, first_with(np.where(state == 1, rid, -1)))
    a2 = np.where(a1 >= 0, a1, first_with(a1))
    left = np.flatnonzero(a2 < 0)
    a2[left] = len(roots) + np.arange(len(left))
    return (a2, roots) if with_roots else a2


def sa_level(a, theta=0.0):
    """one SA level in dense numpy -> (agg, P, R, A_c, omega D^-1)."""
    A = a.to_dense(); n = A.shape[0]
    agg = sa_aggregates(a, theta)
    nc = int(agg.max()) + 1
    size = np.bincount(agg, minlength=nc)
    p0 = np.zeros((n, nc)); p0[np.arange(n), agg] = 1.0 / np.sqrt(size[agg].astype(float))
    d = np.diag(A)
    rho = np.max(np.abs(A).sum(axis=1) / np.abs(d))
    omega = 4.0 / (3.0 * rho)
    P = p0 - (omega / d)[:, None] * (A @ p0)
    return agg, P, P.T.copy(), P.T @ (A @ P), omega / d


# --------------------------------------------------------------------------- smoothed aggregation, operation by operation (amg.hip sa_level)
# Every SA kernel runs one thread per row in a fixed order and the library is built with -ffp-contract=off, so the restatement below
# follows sa_diag_kernel, sa_p0_kernel, sa_spgemm_kernel, sa_smooth_kernel and csr_transpose with the same IEEE operations in the same
# order and gives the device's bits.  Row sums run in rounds over the position inside the row (never np.sum / np.add.reduceat, whose
# association is not the kernels').

def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _ordered_row_sums(rp, terms):
    """per row: 0.0 + terms[rp[i]] + terms[rp[i] + 1] + ... (left to right, one rounding per add)."""
    n = len(rp) - 1
    ln = np.diff(rp)
    s = np.zeros(n)
    for p in range(int(ln.max()) if n else 0):
        live = np.flatnonzero(ln > p)
        s[live] = s[live] + terms[rp[live] + p]
    return s


def spgemm_ordered(ap, ac, av, bp, bc, bv, chunk=1 << 22):
    """C = A B as sa_spgemm_kernel forms it -> (cp, cc, cv): row i of C holds the union of the columns of the rows of B that row i of A
    selects, ascending; each entry is 0.0 + a_ik b_hj + ... over the ascending stored positions k of A's row (B's rows strictly
    ascending).  Products are single IEEE multiplies; the sums run in rounds over the position inside the group."""
    ap = np.asarray(ap, dtype=np.int64); ac = np.asarray(ac, dtype=np.int64); av = np.asarray(av, dtype=np.float64)
    bp = np.asarray(bp, dtype=np.int64); bc = np.asarray(bc, dtype=np.int64); bv = np.asarray(bv, dtype=np.float64)
    n = len(ap) - 1
    arow = _rows_of(ap)
    plen = np.diff(bp)[ac]                                  # products per stored entry of A
    ncb = int(bc.max()) + 1 if len(bc) else 1
    cnt = np.zeros(n, dtype=np.int64)
    cols, vals = [], []
    r0 = 0
    while r0 < n:                                           # chunks of whole rows of A, about `chunk` products each
        k0 = ap[r0]
        cum = np.cumsum(plen[k0:])
        r1 = r0 + 1
        if r1 < n:
            kcut = k0 + int(np.searchsorted(cum, chunk, side="right"))
            r1 = max(r1, int(np.searchsorted(ap, kcut, side="right")) - 1)
        k1 = ap[r1]
        ks = np.arange(k0, k1, dtype=np.int64)
        pl = plen[k0:k1]
        tot = int(pl.sum())
        rep = np.repeat(ks, pl)                             # the A position of every product, ascending
        start = np.repeat(np.cumsum(pl) - pl, pl)
        h = np.repeat(bp[ac[ks]], pl) + (np.arange(tot, dtype=np.int64) - start)
        row = arow[rep]
        key = (row - r0) * ncb + bc[h]
        order = np.argsort(key, kind="stable")              # by (row, column); inside a group the A positions stay ascending
        key = key[order]
        prod = av[rep[order]] * bv[h[order]]
        newg = np.ones(tot, dtype=bool)
        newg[1:] = key[1:] != key[:-1]
        gid = np.cumsum(newg) - 1
        gstart = np.flatnonzero(newg)
        t = np.arange(tot, dtype=np.int64) - gstart[gid]     # position inside the group: the round that adds it
        s = np.zeros(len(gstart))
        o2 = np.argsort(t.astype(np.int32), kind="stable")
        tb = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=int(t.max()) + 1 if tot else 0))])
        for q in range(len(tb) - 1):
            sl = o2[tb[q]:tb[q + 1]]
            s[gid[sl]] = s[gid[sl]] + prod[sl]
        gkey = key[gstart]
        cnt[r0:r1] = np.bincount(gkey // ncb, minlength=r1 - r0)
        cols.append(gkey % ncb); vals.append(s)
        r0 = r1
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=cp[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return cp, cat(cols, np.int64), cat(vals, np.float64)


def transpose_sorted(rp, ci, cv, ncols):
    """csr_transpose: row j of the result lists column j of the input, rows ascending -> (tp, tc, tv)."""
    rows = _rows_of(np.asarray(rp, dtype=np.int64))
    ci = np.asarray(ci, dtype=np.int64)
    order = np.lexsort((rows, ci))
    tp = np.zeros(ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=ncols), out=tp[1:])
    return tp, rows[order], np.asarray(cv, dtype=np.float64)[order]


class SaZeroDiagonal(ValueError):
    pass


def sa_level_ordered(a, theta=0.0):
    """one SA level as amg.hip's sa_level forms it -> dict(agg, nc, rho, omega, dinv (1/d), wdinv (the exported omega D^-1), p0,
    AP0, P, R, AP, Ac), the matrices as oracle.Csr."""
    n = a.nrows
    rp = np.asarray(a.row_ptr, dtype=np.int64); ci = np.asarray(a.col_idx, dtype=np.int64); va = np.asarray(a.vals, dtype=np.float64)
    rows = _rows_of(rp)
    # sa_diag_kernel: d_i the last stored diagonal entry, s_i = 0.0 + |a_ik| over ascending positions, rho = max s_i / |d_i|
    d = np.zeros(n)
    dm = np.flatnonzero(ci == rows)
    d[rows[dm]] = va[dm]                                    # ascending positions: the last assignment wins, as in the kernel
    if np.any(d == 0.0):
        raise SaZeroDiagonal(int(np.flatnonzero(d == 0.0)[0]))
    s = _ordered_row_sums(rp, np.abs(va))
    rho = np.max(s / np.abs(d))
    omega = 4.0 / (3.0 * rho)
    dinv = 1.0 / d
    agg, roots = sa_aggregates(a, theta, with_roots=True)
    agg = np.asarray(agg, dtype=np.int64)
    nc = int(agg.max()) + 1 if n else 0
    size = np.bincount(agg, minlength=nc)
    p0 = 1.0 / np.sqrt(size[agg].astype(np.float64))       # sa_p0_kernel
    # A P0, then sa_smooth_kernel: p = (J == agg_i ? p0_i : 0.0) - (omega * dinv_i) * (A P0)_iJ
    cp, cc, cv = spgemm_ordered(rp, ci, va, np.arange(n + 1), agg, p0)
    ap0 = O.Csr(n, nc, cp, cc, cv.copy(), check=False)
    crow = _rows_of(cp)
    w = omega * dinv
    pv = np.where(cc == agg[crow], p0[crow], 0.0) - w[crow] * cv
    P = O.Csr(n, nc, cp, cc, pv, check=False)
    Rm = O.Csr(nc, n, *transpose_sorted(cp, cc, pv, nc), check=False)
    AP = O.Csr(n, nc, *spgemm_ordered(rp, ci, va, cp, cc, pv), check=False)
    Ac = O.Csr(nc, nc, *spgemm_ordered(Rm.row_ptr, Rm.col_idx, Rm.vals, AP.row_ptr, AP.col_idx, AP.vals), check=False)
    return dict(agg=agg, roots=roots, nc=nc, rho=rho, omega=omega, d=d, dinv=dinv, wdinv=omega * dinv, p0=p0, AP0=ap0, P=P, R=Rm, AP=AP, Ac=Ac)


def sa_hierarchy(a, max_levels=10, theta=0.0):
    """sa_build: coarsen while n > 64 and lv < max_levels; a level with n_c > 0.8 n is dropped (stalled) and its A is the coarsest.
    -> list of levels dict(A, P, R, dinv (exported: omega D^-1; zeros on the last level), agg, stalled (last level only), lvl (the
    sa_level_ordered dict))."""
    levels = []
    cur = a
    lv = 0
    while True:
        n = cur.nrows
        last = lv >= max_levels or n <= 64
        o = None if last else sa_level_ordered(cur, theta)
        stalled = o is not None and float(o["nc"]) > 0.8 * float(n)
        if last or stalled:
            levels.append(dict(A=cur, P=None, R=None, dinv=np.zeros(n), agg=None, stalled=stalled, lvl=o))
            return levels
        levels.append(dict(A=cur, P=o["P"], R=o["R"], dinv=o["wdinv"], agg=o["agg"], stalled=False, lvl=o))
        cur = o["Ac"]
        lv += 1


def sa_coarse_block_jacobi(a):
    """the coarsest level's solve: block Jacobi of min(64, n) rows on A (kryst_pc_block_jacobi_uniform) -> (apply(r) -> z, M as Csr)."""
    import bjacobi_ref as B
    n = a.nrows
    b = min(64, max(n, 1))
    _, inv, _ = B.tiles_uniform(a.row_ptr, a.col_idx, a.vals, n, b)
    m = O.Csr(n, n, *B.m_ref_uniform(n, b, inv), check=False)
    return O.Pc.approx_inverse(m).apply, m


def sa_apply(levels, nu_pre=2, nu_post=2, coarse=None):
    """the SA preconditioner on a hierarchy -> apply(r, z=None) -> z: z starts from zero whatever it holds, then the V-cycle with block
    Jacobi on the coarsest level."""
    if coarse is None:
        coarse = sa_coarse_block_jacobi(levels[-1]["A"])[0]
    return lambda r, z=None: vcycle(levels, np.asarray(r, dtype=np.float64), np.zeros(len(r)), 0, nu_pre, nu_post, coarse)


def vcycle_longdouble(levels, r, nu_pre, nu_post, m_coarse, absval=False):
    """the SA V-cycle (z from zero) on the same hierarchy in np.longdouble, the coarsest solve z = M r with the block-Jacobi matrix
    m_coarse.  absval: every operator and r by its absolute value and every subtraction an addition -- the magnitude that bounds the
    rounding error of the double V-cycle."""
    import scipy.sparse as sp
    f = np.abs if absval else (lambda v: v)
    mat = lambda c: sp.csr_matrix((f(np.asarray(c.vals, dtype=np.longdouble)), np.asarray(c.col_idx), np.asarray(c.row_ptr)),
                                  shape=(c.nrows, c.ncols))
    sub = (lambda x, y: x + y) if absval else (lambda x, y: x - y)
    ops = [dict(A=mat(L["A"]), P=None if L["P"] is None else mat(L["P"]), R=None if L["R"] is None else mat(L["R"]),
                dinv=f(np.asarray(L["dinv"], dtype=np.longdouble))) for L in levels]
    M = mat(m_coarse)

    def cycle(l, r):
        L = ops[l]
        if l + 1 == len(ops):
            return M @ r
        z = np.zeros(len(r), dtype=np.longdouble)
        for _ in range(nu_pre):
            z = z + L["dinv"] * sub(r, L["A"] @ z)
        zc = cycle(l + 1, L["R"] @ sub(r, L["A"] @ z))
        z = z + L["P"] @ zc
        for _ in range(nu_post):
            z = z + L["dinv"] * sub(r, L["A"] @ z)
        return z
    return cycle(0, f(np.asarray(r, dtype=np.longdouble)))
