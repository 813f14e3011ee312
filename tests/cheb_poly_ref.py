"""Restatement of the Chebyshev polynomial preconditioner and its spectrum estimate (kryst_amd/csrc/cheb_poly.hip, host_spectrum.cpp;
DESIGN.md section 4.15), operation by operation: numpy array expressions round every operation on its own, like the library built with
-ffp-contract=off, and the host scalars are Python floats (IEEE double).

  scalars / apply            section 1: theta, delta, sigma, rho_k, c1_k, c2_k; d_0, res_k, d_k, z_k
  jacobi_w                   Jacobi's inv_diag as kryst_pc_jacobi forms it (jacobi.rs:69-71)
  lanczos / gershgorin       section 3, the dots in the library's published order (O.dot with the tiled Reduce)
  tridiag_extreme_eigs       the bisection with Sturm counts of kryst_host_tridiag_extreme_eigs
  default_bounds, make_apply what ChebyshevPoly.setup does with an estimate; closures for amg_ref.pcg and krylov_pc_ref.gmres
"""
import math
import sys

import numpy as np

from oracle import oracle as O

DBL_MIN, EPS = sys.float_info.min, sys.float_info.epsilon


class IndefiniteDiagonal(Exception):
    def __init__(self, row):
        super().__init__(f"IndefiniteDiagonal({row})")
        self.row = row


def scalars(m, lo, hi):
    """-> (theta, [c1_1 .. c1_m], [c2_1 .. c2_m])"""
    lo, hi = float(lo), float(hi)
    theta = (hi + lo) / 2.0
    delta = (hi - lo) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [], []
    for _ in range(m):
        rho_k = 1.0 / (2.0 * sigma - rho)
        c1.append(rho_k * rho)
        c2.append((2.0 * rho_k) / delta)
        rho = rho_k
    return theta, c1, c2


def jacobi_w(a):
    """inv_diag[i] = 1 / a_ii where the stored diagonal (the last one, if a row repeats it) is non-zero, else 0.0"""
    d = np.zeros(a.nrows)
    rows = np.repeat(np.arange(a.nrows, dtype=np.int64), np.diff(a.row_ptr))
    on = np.flatnonzero(a.col_idx == rows)
    d[rows[on]] = 0.0 + a.vals[on] * 1.0                       # (ascending positions: the last stored one stays)
    w = np.zeros(a.nrows)
    nz = d != 0.0
    with np.errstate(all="ignore"):
        w[nz] = 1.0 / d[nz]
    return w


def apply(a, r, m, lo, hi, w=None):
    """z_m of section 1; w None: no scaling (no multiplication at all)"""
    r = np.asarray(r, dtype=np.float64)
    theta, c1, c2 = scalars(m, lo, hi)
    with np.errstate(all="ignore"):
        d = (r if w is None else w * r) / theta
        z = d.copy()
        res = r
        for k in range(m):
            y = a.spmv(d)
            res = res - y
            t = res if w is None else w * res
            d = c1[k] * d + c2[k] * t
            z = z + d
    return z


def make_apply(a, m, lo, hi, w=None, two_args=False):
    """apply(r) for krylov_pc_ref.gmres, apply(r, z) for amg_ref.pcg"""
    if two_args:
        return lambda r, z: apply(a, r, m, lo, hi, w)
    return lambda r: apply(a, r, m, lo, hi, w)


# ------------------------------------------------------------------------------------------------ the tridiagonal eigenvalues
def _sturm_count(a, b, pivmin, x):
    c = 0
    q = a[0] - x
    if abs(q) < pivmin:
        q = -pivmin
    if q < 0.0:
        c += 1
    for i in range(1, len(a)):
        bb = b[i - 1] * b[i - 1]
        try:
            quo = bb / q
        except ZeroDivisionError:                              # (pivmin keeps q away from zero; kept for the shape of IEEE)
            quo = math.copysign(math.inf, bb) * math.copysign(1.0, q)
        q = (a[i] - x) - quo
        if abs(q) < pivmin:
            q = -pivmin
        if q < 0.0:
            c += 1
    return c


def _bisect(a, b, pivmin, want, lo, hi):
    while True:
        mid = lo * 0.5 + hi * 0.5
        if not (lo < mid < hi):
            return lo, hi
        if _sturm_count(a, b, pivmin, mid) >= want:
            hi = mid
        else:
            lo = mid


def tridiag_extreme_eigs(alpha, beta):
    a = [float(v) for v in alpha]
    k = len(a)
    b = [float(v) for v in beta][:k - 1]
    if not all(math.isfinite(v) for v in a + b):
        return math.nan, math.nan
    if k == 1:
        return a[0], a[0]
    gl = gu = bmax = 0.0
    for i in range(k):
        off = (abs(b[i - 1]) if i > 0 else 0.0) + (abs(b[i]) if i + 1 < k else 0.0)
        lo_i, up_i = a[i] - off, a[i] + off
        if i == 0 or lo_i < gl:
            gl = lo_i
        if i == 0 or up_i > gu:
            gu = up_i
        if i + 1 < k:
            bb = b[i] * b[i]
            if bb > bmax:
                bmax = bb
    pivmin = DBL_MIN * (bmax if bmax > 1.0 else 1.0)
    tnorm = abs(gl) if abs(gl) > abs(gu) else abs(gu)
    widen = (2.0 * tnorm) * EPS * float(k) + 2.0 * pivmin
    gl = gl - widen
    gu = gu + widen
    tmin = _bisect(a, b, pivmin, 1, gl, gu)[0]
    tmax = _bisect(a, b, pivmin, k, gl, gu)[1]
    return tmin, tmax


def tridiag_dense(alpha, beta):
    k = len(alpha)
    t = np.diag(np.asarray(alpha, dtype=np.float64))
    for i in range(k - 1):
        t[i, i + 1] = t[i + 1, i] = beta[i]
    return t


# ------------------------------------------------------------------------------------------------ the estimate
def checked_w(a):
    w = jacobi_w(a)
    with np.errstate(all="ignore"):
        bad = np.flatnonzero(~((w > 0.0) & np.isfinite(w)))
    if len(bad):
        raise IndefiniteDiagonal(int(bad[0]))
    return w


def gershgorin(a, w=None):
    """max_i((sum_k |a_ik|) * w_i), the row sums from 0.0 in stored order; a NaN wins"""
    ln = np.diff(a.row_ptr)
    s = np.zeros(a.nrows)
    terms = np.abs(a.vals)
    with np.errstate(all="ignore"):
        for p in range(int(ln.max()) if a.nrows else 0):
            live = np.flatnonzero(ln > p)
            s[live] = s[live] + terms[a.row_ptr[live] + p]
        if w is not None:
            s = s * w
    return float("nan") if np.isnan(s).any() else float(s.max())


def lanczos(a, steps, seed, rs, w=None):
    """-> (alpha, beta) of steps_done = len(alpha) entries each"""
    n = a.nrows
    dot = lambda u, v: float(O.dot(u, v, rs))                   # noqa: E731
    s = None if w is None else np.sqrt(w)
    u = O.splitmix64_uniform(seed, n)
    alpha, beta = [], []
    with np.errstate(all="ignore"):
        q = u / math.sqrt(dot(u, u))
        q_prev = None
        for j in range(min(steps, n)):
            if s is None:
                t = a.spmv(q)
            else:
                t = s * a.spmv(s * q)
            al = dot(q, t)
            t = t - al * q
            if j > 0:
                t = t - beta[j - 1] * q_prev
            tt = dot(t, t)
            be = math.sqrt(tt) if tt >= 0.0 else math.nan
            alpha.append(al); beta.append(be)
            if be == 0.0 or not math.isfinite(be):
                break
            q_prev, q = q, t / be
    return np.array(alpha), np.array(beta)


def estimate(a, rs, jacobi=True, steps=10, seed=0x5EED):
    w = checked_w(a) if jacobi else None
    g = gershgorin(a, w)
    al, be = lanczos(a, steps, seed, rs, w)
    tmin, tmax = tridiag_extreme_eigs(al, be)
    return {"alpha": al, "beta": be, "steps_done": len(al), "theta_min": tmin, "theta_max": tmax, "gershgorin": g}


def default_bounds(est, ratio=30.0, safety=1.1):
    hi = min(float(safety) * est["theta_max"], est["gershgorin"])
    return hi / float(ratio), hi
