"""numpy restatements of MINRES, QMR and CGNR as written (src/solver/minres.rs:60-219, qmr.rs:61-166, cgnr.rs:77-132), of the two
labelled extensions (textbook MINRES, Paige & Saunders 1975; textbook CGNR, Saad section 8.3) and of the host transpose
(kryst_amd/csrc/minres_qmr_cgnr.hip, transpose.hip).

Inner products go through oracle.dot / oracle.norm in the association order `rs` (Reduce.tiled(*K.reduce_spec()) for the device,
Reduce.serial() for the line-by-line transliterations), SpMVs through oracle.Csr.spmv.  Element-wise expressions keep the reference's
order; numpy never contracts a*b+c.  Each solver returns Res(x, iterations, converged, final_residual, history), history being the
value passed to Convergence::check each iteration (the device records the same)."""
import numpy as np

from oracle import oracle as O


class Res:
    def __init__(self, x, iterations, converged, final_residual, history):
        self.x, self.iterations, self.converged, self.final_residual, self.history = x, iterations, converged, final_residual, history


def check(res, res0, i, tol, max_iters):
    """Convergence::check (src/utils/convergence.rs:18-34) -> (stop, converged)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.float64(res) / np.float64(res0)
    conv = bool(rel <= tol) or i >= max_iters
    return conv


def transpose(a):
    """A^T as an oracle.Csr: row j lists column j of A in ascending row order; entries of one row of A keep their stored order
    (a row that holds column j twice contributes both, in stored order).  Works on unsorted and duplicate-entry rows too."""
    rp = np.asarray(a.row_ptr, dtype=np.int64)
    ci = np.asarray(a.col_idx, dtype=np.int64)
    rows = np.repeat(np.arange(a.nrows, dtype=np.int64), np.diff(rp))
    order = np.argsort(ci, kind="stable")                       # stable: ascending row, then stored order inside a row
    tp = np.zeros(a.ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=a.ncols), out=tp[1:])
    return O.Csr(a.ncols, a.nrows, tp, rows[order], np.asarray(a.vals, dtype=np.float64)[order], check=False)


def minres(a, b, x0, tol, max_iters, rs):
    """minres.rs:60-219 as written."""
    n = len(b)
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    r = b - a.spmv(x0)
    beta1 = np.sqrt(dot(r, r))
    if beta1 == 0.0:
        return Res(np.zeros(n), 0, True, beta1, [])
    v_prev = np.zeros(n); v = r / beta1
    w_prev = np.zeros(n); w = np.zeros(n)
    x_out = np.zeros(n); x_best = x_out.copy()
    phi_min = abs(beta1)
    beta = beta1; c_prev = 1.0; s_prev = 0.0; rho_bar = beta1; phi = beta1
    it, conv, hist = 0, False, []
    for j in range(1, max_iters + 1):
        v_next = a.spmv(v)
        alpha = dot(v, v_next)
        v_next = v_next - alpha * v - beta * v_prev
        beta_next = np.sqrt(dot(v_next, v_next))
        if beta_next == 0.0:
            break
        v_next = v_next / beta_next
        if j == 1:
            delta = 0.0; epsilon = 0.0
        else:
            delta = s_prev * beta; epsilon = -c_prev * beta
        rho = np.sqrt(rho_bar * rho_bar + alpha * alpha)
        c = rho_bar / rho if rho != 0.0 else 1.0
        s = alpha / rho if rho != 0.0 else 0.0
        phi_next = c * phi
        phi_bar = -s * phi
        with np.errstate(divide="ignore", invalid="ignore"):
            w_new = v / rho if j == 1 else (v - delta * w - epsilon * w_prev) / rho
        x_out = x_out + phi_next * w_new
        if rho == 0.0:
            break
        w_prev = w; w = w_new; v_prev = v; v = v_next
        beta = beta_next; phi = phi_next; rho_bar = -s * beta_next; c_prev = c; s_prev = s
        if abs(phi_bar) < phi_min:
            phi_min = abs(phi_bar); x_best = x_out.copy()
        hist.append(abs(phi_bar))
        stop = check(abs(phi_bar), beta1, j, tol, max_iters)
        it, conv = j, stop
        if stop:
            break
    return Res(x_best, it, conv, phi_min, hist)


def minres_textbook(a, b, x0, tol, max_iters, rs):
    """Unpreconditioned MINRES (Paige & Saunders 1975) from x0; stop on |phi_bar_k| / beta_1 <= tol or the cap; beta_{k+1} = 0 exact."""
    n = len(b)
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    x = np.array(x0, dtype=np.float64)
    r = b - a.spmv(x)
    beta1 = np.sqrt(dot(r, r))
    if beta1 == 0.0:
        return Res(x, 0, True, beta1, [])
    v_prev = np.zeros(n); v = r / beta1
    w_prev = np.zeros(n); w = np.zeros(n)
    c_prev = c = 1.0; s_prev = s = 0.0; eta = beta1; beta = beta1
    it, conv, fin, hist = 0, False, beta1, []
    for k in range(1, max_iters + 1):
        p = a.spmv(v)
        alpha = dot(v, p)
        p = p - alpha * v - beta * v_prev
        bn = np.sqrt(dot(p, p))
        gbar = c * alpha - c_prev * s * beta
        delta = s * alpha + c_prev * c * beta
        epsilon = s_prev * beta
        gamma = np.sqrt(gbar * gbar + bn * bn)              # sqrt, not hypot: the device rounds the same way
        cn = gbar / gamma; sn = bn / gamma
        coef = cn * eta
        eta = -sn * eta
        w_new = (v - epsilon * w_prev - delta * w) / gamma
        x = x + coef * w_new
        res = abs(eta)
        hist.append(res)
        stop = check(res, beta1, k, tol, max_iters)
        it, conv, fin = k, stop, res
        if bn == 0.0:
            conv = True
            break
        if stop:
            break
        with np.errstate(divide="ignore", invalid="ignore"):
            v_next = p / bn
        w_prev = w; w = w_new; v_prev = v; v = v_next
        c_prev = c; c = cn; s_prev = s; s = sn; beta = bn
    return Res(x, it, conv, fin, hist)


def qmr(a, b, x0, tol, max_iters, rs):
    """qmr.rs:61-166 as written (the unread A^T p_tld is left out)."""
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    x = np.array(x0, dtype=np.float64)
    r = b - a.spmv(x)
    r_tld = r.copy()
    norm_r0 = np.sqrt(dot(r, r))
    it, conv, fin, hist = 0, False, norm_r0, []
    rho = dot(r_tld, r)
    if rho == 0.0:
        return Res(x, 0, True, np.sqrt(dot(r, r)), [])
    res_norm = norm_r0
    p = p_tld = None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(max_iters):
            if j == 0:
                p = r.copy(); p_tld = r_tld.copy()
            else:
                rho_prev = rho
                rho = dot(r_tld, r)
                if rho == 0.0:
                    break
                beta = rho / rho_prev
                p = r + beta * p
                p_tld = r_tld + beta * p_tld
            v = a.spmv(p)
            sigma = dot(p_tld, v)
            if sigma == 0.0:
                break
            alpha = rho / sigma
            s = r - alpha * v
            t = a.spmv(s)
            t_dot_s = dot(t, s); t_dot_t = dot(t, t)
            omega = t_dot_s / t_dot_t if t_dot_t != 0.0 else 0.0
            x = x + alpha * p + omega * s
            r = s - omega * t
            t = b - a.spmv(x)
            res_norm = np.sqrt(dot(t, t))
            hist.append(res_norm)
            stop = check(res_norm, norm_r0, j + 1, tol, max_iters)
            it, conv, fin = j + 1, stop, res_norm
            if stop:
                conv = True
                break
    return Res(x, it, conv, fin, hist)


def cgnr(a, b, x0, tol, max_iters, rs, textbook=False):
    """cgnr.rs:77-132 as written (CgneSolver :153-208 is the same), or textbook CGNR (Saad section 8.3) with A^T = transpose(a)."""
    dot = lambda u, v: np.float64(O.dot(u, v, rs))
    at = transpose(a) if textbook else a
    x = np.array(x0, dtype=np.float64)
    r = b - a.spmv(x)
    z = at.spmv(r)
    p = z.copy()
    rz = dot(z, z)
    res0 = np.sqrt(dot(r, r))
    it, conv, fin, hist = 0, False, res0, []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(1, max_iters + 1):
            ap = a.spmv(p)
            if textbook:
                alpha = rz / dot(ap, ap)
            else:
                at_ap = a.spmv(ap)
                alpha = rz / dot(at_ap, at_ap)
            x = x + alpha * p
            r = r - alpha * ap
            z = at.spmv(r)
            rz_new = dot(z, z)
            res_norm = np.sqrt(dot(r, r))
            hist.append(res_norm)
            stop = check(res_norm, res0, i, tol, max_iters)
            it, conv, fin = i, stop, res_norm
            if stop:
                break
            beta = rz_new / rz
            p = z + beta * p
            rz = rz_new
    return Res(x, it, conv, fin, hist)


SOLVERS = {
    "minres": minres,
    "qmr": qmr,
    "cgnr": cgnr,
    "minres_textbook": minres_textbook,
    "cgnr_textbook": lambda a, b, x0, tol, mx, rs: cgnr(a, b, x0, tol, mx, rs, textbook=True),
}
