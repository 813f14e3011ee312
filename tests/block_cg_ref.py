"""Block CG (Dubrulle's retooled block CG, BCGrQ, with a Cholesky-QR of a K x K Gram matrix) restated in numpy: the reference of the block CG tests.

Two implementations:

  solve()        the restatement, in the operation order kryst_amd/csrc/bcg_logic.h and block_cg.hip write down -- every K x K step in scalar loops
                 on Python floats (IEEE doubles, one rounding per operation, nothing fused), every Gram entry the oracle's tiled inner product,
                 every row product summed from 0.0 in ascending order over the structurally nonzero terms.  The GPU tier compares against it bit
                 for bit; the CPU tier compares kryst_host_bcg_step with step().
  solve_plain()  the same method with numpy.linalg and no fixed order, to check the restatement against.

Multivectors are (n, K) arrays; d is the Jacobi inv_diag (or None: no preconditioner / Identity, no multiply at all)."""
import collections
import math

import numpy as np

from oracle import oracle as O

SPEC = (256, 2, 1024)
RANK_TOL = 2.0 ** -26
OK, SOLVE_ERROR, INDEFINITE_MATRIX, INDEFINITE_PC = 0, 2, 3, 4
GRAM_RES, GRAM_ST = 0, 1
STEP_INIT, STEP_ALPHA, STEP_BETA = 0, 1, 2


def rs():
    return O.Reduce.tiled(*SPEC)


# ---------------------------------------------------------------------------------------------------------------- passes over the multivectors
def spmm(a, x):
    return np.stack([a.spmv(np.ascontiguousarray(x[:, j])) for j in range(x.shape[1])], axis=1)


def gram(u, v, d=None):
    """entry (a, b), a <= b: the tiled inner product over u(i, a) * v(i, b), or u(i, a) * (d_i * v(i, b)); the lower triangle is the mirror"""
    k = u.shape[1]
    g = np.zeros((k, k))
    r = rs()
    w = v if d is None else d[:, None] * v
    for a in range(k):
        ua = np.ascontiguousarray(u[:, a])
        for b in range(a, k):
            g[a, b] = g[b, a] = O.dot(ua, np.ascontiguousarray(w[:, b]), r)
    return g


def row_product(u, m, lo=None, hi=None):
    """(U M)(i, j) from 0.0, adding U(i, l) * M[l][j] for l ascending over lo(j) .. hi(j) (default: every l)"""
    n, k = u.shape
    out = np.zeros((n, k))
    for j in range(k):
        acc = np.zeros(n)
        for l in range(0 if lo is None else lo(j), k if hi is None else hi(j) + 1):
            acc = acc + u[:, l] * m[l][j]
        out[:, j] = acc
    return out


# ---------------------------------------------------------------------------------------------------------------- the K x K steps, scalar loops
def chol(g, gram_kind):
    """-> (code, U, margin): upper U with U^T U = g in the fixed order, the pivot rule, and the smallest s / g[j][j] seen (inf when none)"""
    k = len(g)
    u = [[0.0] * k for _ in range(k)]
    margin = math.inf
    for j in range(k):
        gjj = float(g[j][j])
        s = gjj
        for l in range(j):
            s = s - u[l][j] * u[l][j]
        if gram_kind == GRAM_ST:
            if not (gjj > 0.0) or not (s > 0.0):
                return INDEFINITE_MATRIX, u, margin
        elif gjj < 0.0:
            return INDEFINITE_PC, u, margin
        if not (s > RANK_TOL * gjj):
            return SOLVE_ERROR, u, margin
        margin = min(margin, s / gjj)
        ujj = math.sqrt(s)
        u[j][j] = ujj
        for i in range(j + 1, k):
            t = float(g[j][i])
            for l in range(j):
                t = t - u[l][j] * u[l][i]
            u[j][i] = t / ujj
    return OK, u, margin


def upper_inverse(u):
    """back substitution, column by column, j ascending; within a column i = j - 1 down to 0"""
    k = len(u)
    v = [[0.0] * k for _ in range(k)]
    for j in range(k):
        v[j][j] = 1.0 / u[j][j]
        for i in range(j - 1, -1, -1):
            s = 0.0
            for l in range(i + 1, j + 1):
                s = s + u[i][l] * v[l][j]
            v[i][j] = (0.0 - s) / u[i][i]
    return v


def gamma(v):
    k = len(v)
    g = [[0.0] * k for _ in range(k)]
    for a in range(k):
        for b in range(a, k):
            s = 0.0
            for l in range(b, k):
                s = s + v[a][l] * v[b][l]
            g[a][b] = g[b][a] = s
    return g


def full_times_upper(gam, c):
    k = len(c)
    out = [[0.0] * k for _ in range(k)]
    for a in range(k):
        for j in range(k):
            s = 0.0
            for l in range(j + 1):
                s = s + gam[a][l] * c[l][j]
            out[a][j] = s
    return out


def upper_times_upper(phi, c):
    k = len(c)
    out = [[0.0] * k for _ in range(k)]
    for a in range(k):
        for j in range(a, k):
            s = 0.0
            for l in range(a, j + 1):
                s = s + phi[a][l] * c[l][j]
            out[a][j] = s
    return out


def column_norms(c):
    k = len(c)
    res = []
    for j in range(k):
        s = 0.0
        for l in range(j + 1):
            s = s + c[l][j] * c[l][j]
        res.append(math.sqrt(s))
    return res


Step = collections.namedtuple("Step", "code c out1 out2 res margin")


def step(kind, g, c=None):
    """kryst_host_bcg_step restated.  INIT: c = chol(g), out1 = c^-1, res.  ALPHA: out1 = Gamma, out2 = Gamma c.  BETA: out1 = Phi, out2 = Phi^-1,
    c <- Phi c, res.  After a breakdown only `code` (and margin) mean anything."""
    g = [[float(x) for x in row] for row in np.asarray(g)]
    c = None if c is None else [[float(x) for x in row] for row in np.asarray(c)]
    if kind == STEP_INIT:
        code, cc, margin = chol(g, GRAM_RES)
        if code:
            return Step(code, None, None, None, None, margin)
        return Step(OK, cc, upper_inverse(cc), None, column_norms(cc), margin)
    if kind == STEP_ALPHA:
        code, u, margin = chol(g, GRAM_ST)
        if code:
            return Step(code, c, None, None, None, margin)
        gam = gamma(upper_inverse(u))
        return Step(OK, c, gam, full_times_upper(gam, c), None, margin)
    code, phi, margin = chol(g, GRAM_RES)
    if code:
        return Step(code, c, None, None, None, margin)
    cn = upper_times_upper(phi, c)
    return Step(OK, cn, phi, upper_inverse(phi), column_norms(cn), margin)


# ---------------------------------------------------------------------------------------------------------------- the solve
Result = collections.namedtuple("Result", "status iterations final_residual converged history x margin")


def solve(a, b, x0=None, d=None, tol=1e-8, max_iters=200):
    """-> Result: status (one code for the block), iterations, final_residual[K], converged[K], history (K lists), x (x0 after a breakdown),
    margin (the smallest s / G[j][j] any Cholesky pivot of the run saw)"""
    b = np.asarray(b, dtype=np.float64)
    n, k = b.shape
    x_in = np.zeros((n, k)) if x0 is None else np.array(x0, dtype=np.float64)
    x = x_in.copy()
    hist = [[] for _ in range(k)]

    def broke(code, it, res, margin):
        return Result(code, it, list(res), [False] * k, hist, x_in.copy(), margin)

    r = b - spmm(a, x)
    st = step(STEP_INIT, gram(r, r, d))
    margin = st.margin
    if st.code:
        return broke(st.code, 0, [0.0] * k, margin)
    c, res0 = st.c, st.res
    upper = dict(lo=None, hi=lambda j: j)
    q = row_product(r, st.out1, **upper)
    s = q.copy() if d is None else d[:, None] * q
    res = list(res0)
    for j in range(k):
        hist[j].append(res[j])
    if max_iters <= 0:
        return Result(OK, 0, res, [False] * k, hist, x, margin)
    it = 0
    while True:
        t = spmm(a, s)
        sa = step(STEP_ALPHA, gram(s, t), c)
        margin = min(margin, sa.margin)
        if sa.code:
            return broke(sa.code, it + 1, res, margin)
        gam, m1 = sa.out1, sa.out2
        x = x + row_product(s, m1)
        qn = q - row_product(t, gam)
        sb = step(STEP_BETA, gram(qn, qn, d), c)
        margin = min(margin, sb.margin)
        if sb.code:
            return broke(sb.code, it + 1, res, margin)
        c, phi, phinv, res = sb.c, sb.out1, sb.out2, list(sb.res)
        it += 1
        for j in range(k):
            hist[j].append(res[j])
        conv = [res[j] / res0[j] <= tol for j in range(k)]
        if all(conv) or it >= max_iters:
            return Result(OK, it, res, [cj or it >= max_iters for cj in conv], hist, x, margin)
        q = row_product(qn, phinv, **upper)
        dq = q if d is None else d[:, None] * q
        # (S Phi^T)(i, j) = sum_{l = j .. K-1} S(i, l) * Phi[j][l]
        phit = [[phi[jj][l] for jj in range(k)] for l in range(k)]
        s = dq + row_product(s, phit, lo=lambda j: j, hi=None)


def solve_plain(a, b, x0=None, d=None, tol=1e-8, max_iters=200):
    """the same method with numpy.linalg: -> (iterations, x, final residual norms)"""
    b = np.asarray(b, dtype=np.float64)
    n, k = b.shape
    x = np.zeros((n, k)) if x0 is None else np.array(x0, dtype=np.float64)
    w = (lambda v: v) if d is None else (lambda v: d[:, None] * v)
    r = b - spmm(a, x)
    c = np.linalg.cholesky(r.T @ w(r)).T
    q = np.linalg.solve(c.T, r.T).T
    s = w(q)
    res0 = np.linalg.norm(c, axis=0)
    res = res0
    it = 0
    while it < max_iters:
        t = spmm(a, s)
        gam = np.linalg.inv(s.T @ t)
        x = x + s @ (gam @ c)
        qn = q - t @ gam
        phi = np.linalg.cholesky(qn.T @ w(qn)).T
        c = phi @ c
        res = np.linalg.norm(c, axis=0)
        it += 1
        if np.all(res / res0 <= tol):
            break
        q = np.linalg.solve(phi.T, qn.T).T
        s = w(q) + s @ phi.T
    return it, x, res
