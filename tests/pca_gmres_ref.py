"""numpy restatements of PcaGmresSolver (src/solver/pca_gmres.rs:99-312): the as-written form and the labelled s-step extension,
operation for operation in the order of kryst_amd/csrc/pca_gmres.hip, with every inner product taken by oracle.dot in the given
reduction order (Reduce.tiled(*reduce_spec()) for the device's bits, Reduce.serial() for a line-by-line reading of the reference)."""
import numpy as np

from oracle import oracle as O

F = np.float64
EPS = F(np.finfo(np.float64).eps)


class ArgError(Exception):
    """the device returns KRYST_ERR_ARG"""


class Unsupported(Exception):
    """the device returns KRYST_UNSUPPORTED"""


class Result:
    def __init__(self, x, iterations, final_residual, converged, history, cycles=None):
        self.x, self.iterations, self.final_residual, self.converged = x, iterations, final_residual, converged
        self.history = np.array(history, dtype=float)
        self.cycles = cycles or []
        self.events = []

    def __repr__(self):
        return f"Result(iterations={self.iterations}, final_residual={self.final_residual!r}, converged={self.converged})"


def _sqrt(v):
    return F(np.sqrt(F(v)))


def _givens(h, g, cs, sn, col):
    """pca_gmres.rs:238-262"""
    for i in range(col):
        temp = cs[i] * h[i, col] + sn[i] * h[i + 1, col]
        h[i + 1, col] = -sn[i] * h[i, col] + cs[i] * h[i + 1, col]
        h[i, col] = temp
    h_kk, h_k1k = h[col, col], h[col + 1, col]
    r = _sqrt(h_kk * h_kk + h_k1k * h_k1k)
    if abs(r) < EPS:
        cs[col], sn[col] = F(1.0), F(0.0)
    else:
        cs[col], sn[col] = h_kk / r, h_k1k / r
    h[col, col] = cs[col] * h_kk + sn[col] * h_k1k
    h[col + 1, col] = F(0.0)
    temp = cs[col] * g[col] + sn[col] * g[col + 1]
    g[col + 1] = -sn[col] * g[col] + cs[col] * g[col + 1]
    g[col] = temp


def as_written(a, b, x=None, pc=None, side=1, restart=30, block_size=1, tol=1e-8, max_iters=100, rs=O.SERIAL):
    """pca_gmres.rs:99-312 with the default features.  x is ignored (:107).  Raises ArgError where the device returns KRYST_ERR_ARG."""
    R, s = int(restart), int(block_size)
    if R < 1 or s < 1:
        raise ArgError("restart = 0 or block_size = 0")
    n_outer = (max_iters + R - 1) // R                                   # :120
    if s >= 2 and R >= 2 and n_outer >= 1:
        raise ArgError("block_size >= 2 with restart >= 2")
    right = side == 2 and pc is not None
    dot = lambda u, v: F(O.dot(u, v, rs))
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=float)
        n = len(b)
        xk = np.zeros(n)                                                 # :107
        r0 = b - a.spmv(xk)                                              # :108-113
        beta = _sqrt(dot(r0, r0))
        res0 = beta
        st = [0, beta, False]
        hist = []
        iteration = 0
        for _ in range(n_outer):
            V = [r0 / beta]                                              # :124
            h = np.zeros((R + 1, R)); g = np.zeros(R + 1); g[0] = beta
            cs = np.zeros(R); sn = np.zeros(R)
            j = 0
            while j < R:                                                 # t = min(s, m - j) = 1
                w = a.spmv(V[j])                                         # :145 / :151
                if right:
                    w = pc.apply(w)                                      # :152-156
                for i in range(j + 1):
                    h[i, j] = dot(V[i], w)                               # :177, :210
                nrm = _sqrt(dot(w, w))                                   # :225
                h[j + 1, j] = nrm
                inv = F(1.0) / nrm                                       # :227
                V.append(w * inv)
                _givens(h, g, cs, sn, j)
                gnorm = abs(g[j + 1])                                    # :266
                iteration += 1
                hist.append(gnorm)
                conv = (gnorm / res0 <= tol) or iteration >= max_iters   # Convergence::check
                st = [iteration, gnorm, conv]
                if conv:
                    break
                j += 1
            m = j                                                        # :277
            y = np.zeros(R)
            for i in range(m - 1, -1, -1):                               # :280-286
                acc = g[i]
                for k in range(i + 1, m):
                    acc = acc - h[i, k] * y[k]
                if abs(h[i, i]) > EPS:
                    y[i] = acc / h[i, i]
            for i in range(m):                                           # :289-295
                xk = xk + y[i] * V[i]
            r0 = b - a.spmv(xk)                                          # :298-302
            beta = _sqrt(dot(r0, r0))
            st[1] = beta
            st[2] = bool(beta <= tol * res0)                             # :304
            if st[2] or iteration >= max_iters:
                break
    return Result(xk, st[0], st[1], bool(st[2]), hist)


def _chol(G, k, S, test=None):
    """upper Cholesky column by column; test(c, d) -> False ends the factor at column c (returns the columns kept)"""
    Rm = np.zeros((S, S))
    keep = k
    for c in range(k):
        for r in range(c):
            v = G[r, c]
            for i in range(r):
                v = v - Rm[i, r] * Rm[i, c]
            Rm[r, c] = v / Rm[r, r]
        d = G[c, c]
        for i in range(c):
            d = d - Rm[i, c] * Rm[i, c]
        if test is not None and not test(c, d):
            Rm[:c, c] = 0.0
            keep = c
            break
        Rm[c, c] = _sqrt(d)
    return Rm, keep


def sstep(a, b, x=None, pc=None, side=2, restart=30, block_size=5, tol=1e-8, max_iters=100, rs=O.SERIAL):
    """the labelled extension: s-step GMRES(restart), right preconditioned, BCGS2 + CholQR2 (pca_gmres.hip, part 2).  cycles holds,
    per restart cycle, the basis Q, the unrotated Hessenberg matrix Hu and the number of columns m, for the Arnoldi checks."""
    R, S = int(restart), int(block_size)
    if R < 1 or S < 1 or S > 16:
        raise ArgError("restart or block_size out of range")
    if side not in (0, 1, 2):
        raise ArgError("side")
    if side == 1 and pc is not None:
        raise Unsupported("left preconditioning")
    M = (lambda v: pc.apply(v)) if (side == 2 and pc is not None) else (lambda v: v)
    dot = lambda u, v: F(O.dot(u, v, rs))
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=float)
        n = len(b)
        xk = np.zeros(n) if x is None else np.array(x, dtype=float)
        r0 = b - a.spmv(xk)
        beta = _sqrt(dot(r0, r0))
        res0 = beta
        it, final, conv = 0, beta, False
        hist, cycles, events = [], [], []
        if beta == 0.0:
            return Result(xk, 0, beta, True, hist)
        if max_iters <= 0:
            return Result(xk, 0, beta, False, hist)
        while True:
            Q = [r0 / beta]
            H = np.zeros((R + 1, R)); Hu = np.zeros((R + 1, R)); g = np.zeros(R + 1); g[0] = beta
            cs = np.zeros(R); sn = np.zeros(R)
            ysc = np.zeros(R + 1)
            j, m = 0, R
            while True:
                s_eff = min(S, R - j, max_iters - it)
                # block generation
                W, nu2, nu = [], [], []
                inp = Q[j]
                for c in range(s_eff):
                    wc = a.spmv(M(inp))
                    W.append(wc)
                    d = dot(wc, wc)
                    nu2.append(d); nu.append(_sqrt(d))
                    if c + 1 < s_eff:
                        inp = wc / nu[c]
                nb = j + 1
                # BCGS2
                C1 = np.array([[dot(Q[i], W[k]) for k in range(s_eff)] for i in range(nb)])
                for k in range(s_eff):
                    for i in range(nb):
                        W[k] = W[k] - C1[i, k] * Q[i]
                C2 = np.array([[dot(Q[i], W[k]) for k in range(s_eff)] for i in range(nb)])
                for k in range(s_eff):
                    for i in range(nb):
                        W[k] = W[k] - C2[i, k] * Q[i]
                # CholQR, first pass with the column test
                G1 = np.zeros((s_eff, s_eff))
                for p in range(s_eff):
                    for q in range(p, s_eff):
                        G1[p, q] = dot(W[p], W[q])
                R1, keep = _chol(G1, s_eff, S, lambda c, d: bool(np.isfinite(d) and d > 1e-12 * nu2[c]))
                X = []
                for c in range(keep):
                    xc = W[c]
                    for r in range(c):
                        xc = xc - X[r] * R1[r, c]
                    X.append(xc / R1[c, c])
                G2 = np.zeros((max(keep, 1), max(keep, 1)))
                for p in range(keep):
                    for q in range(p, keep):
                        G2[p, q] = dot(X[p], X[q])
                R2, _ = _chol(G2, keep, S)
                k = keep
                ncols = k if k > 0 else 1
                if k == 0:
                    events.append(("happy", j))
                elif k < s_eff:
                    events.append(("truncate", j, k, s_eff))

                def Y(l, cc):
                    if l <= j:
                        return C1[l, cc] + C2[l, cc]
                    if k == 0:
                        return F(0.0)
                    a_ = l - j - 1
                    acc = F(0.0)
                    for i in range(a_, cc + 1):
                        acc = acc + R2[a_, i] * R1[i, cc]
                    return acc

                stop = False
                for cc in range(ncols):
                    col = j + cc
                    for l in range(col + 2):
                        Hu[l, col] = Y(l, cc)
                    if cc > 0:
                        nuv = nu[cc - 1]
                        tdiag = ysc[col] / nuv
                        for l in range(col + 2):
                            v = Hu[l, col]
                            for i in range(col):
                                v = v - (ysc[i] / nuv) * Hu[l, i]
                            Hu[l, col] = v / tdiag
                    if cc + 1 < ncols:
                        for l in range(col + 2):
                            ysc[l] = Y(l, cc)
                    H[:col + 2, col] = Hu[:col + 2, col]
                    _givens(H, g, cs, sn, col)
                    it += 1
                    res = abs(g[col + 1])
                    hist.append(res)
                    final = res
                    conv = bool(res <= tol * res0)
                    if conv or it >= max_iters or k == 0:
                        stop, m = True, col + 1
                        break
                # pass E: the new basis vectors
                for c in range(keep):
                    qc = X[c]
                    for r in range(c):
                        qc = qc - Q[j + 1 + r] * R2[r, c]
                    Q.append(qc / R2[c, c])
                if stop:
                    break
                j += ncols
                if j >= R:
                    m = R
                    break
            cycles.append({"Q": np.array(Q).T.copy(), "Hu": Hu.copy(), "m": m})
            y = np.zeros(R + 1)
            for i in range(m - 1, -1, -1):
                acc = g[i]
                for kk in range(i + 1, m):
                    acc = acc - H[i, kk] * y[kk]
                y[i] = acc / H[i, i]
            t = np.zeros(n)
            for i in range(m):
                t = t + y[i] * Q[i]
            xk = xk + M(t)
            r0 = b - a.spmv(xk)
            beta = _sqrt(dot(r0, r0))
            final = beta
            conv = bool(beta <= tol * res0)
            if conv or it >= max_iters:
                break
    res = Result(xk, it, final, conv, hist, cycles)
    res.events = events
    return res
