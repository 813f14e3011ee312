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


def vcycle(levels, r, z, level=0, nu_pre=1, nu_post=1):
    """apply_recursive(level, r, z) (:200-250) -> the new z."""
    L = levels[level]
    if level + 1 == len(levels):
        return solve_direct(L["A"], r)
    a, dinv = L["A"], L["dinv"]
    z = smooth(a, dinv, r, np.array(z, dtype=np.float64), nu_pre)
    az = r - a.spmv(z)
    rc = L["R"].spmv(az)
    zc = vcycle(levels, rc, np.zeros(len(rc)), level + 1, nu_pre, nu_post)
    z = z + L["P"].spmv(zc)
    return smooth(a, dinv, r, z, nu_post)


# --------------------------------------------------------------------------- PCG with the AMG apply (pcg.rs)

def pcg(a, levels, b, tol, max_iters, rs):
    """PcgSolver::solve with norm Unpreconditioned -> (x, iterations, code, history); code 0, 3 (IndefiniteMatrix) or 4
    (IndefinitePreconditioner)."""
    n = len(b)
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    x = np.zeros(n)
    r = b - a.spmv(x)
    z = vcycle(levels, r, np.zeros(n))
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
            z = vcycle(levels, r, z)
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


def sa_aggregates(a, theta=0.0):
    """distance-2 MIS with hashed priorities, root neighbourhoods, then leftover attachment; singletons numbered after the roots."""
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
    return a2


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
