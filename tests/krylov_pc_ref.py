"""numpy restatements of preconditioned GMRES(m) (src/solver/gmres.rs:216-402, left and right as written) and of right-preconditioned
BiCGStab (bicgstab.rs:69-293 with the labelled extension of kryst_bicgstab_rpc_solve_dev: M^-1 p and M^-1 s feed the SpMVs and the update
of x) that take the preconditioner as a callable `apply(r) -> z` and every inner product through oracle.dot in the given reduction order:
what amg_ref.pcg is for PCG, for preconditioners the C oracle has no form of (tests/sor_ref.py).  Pinned on the CPU against the C oracle
with the Jacobi apply (tests/test_sor_cpu.py)."""
import numpy as np

from oracle import oracle as O

F = np.float64
EPS = 1e-14                        # gmres.rs:233
DBL_EPS = float(np.finfo(np.float64).eps)


def _givens(h, g, cs, sn, j):      # gmres.rs:154-176
    for i in range(j):
        temp = cs[i] * h[i, j] + sn[i] * h[i + 1, j]
        h[i + 1, j] = -sn[i] * h[i, j] + cs[i] * h[i + 1, j]
        h[i, j] = temp
    h_kk, h_k1k = h[j, j], h[j + 1, j]
    r = F(np.sqrt(h_kk * h_kk + h_k1k * h_k1k))
    if abs(r) < EPS:
        cs[j], sn[j] = 1.0, 0.0
    else:
        cs[j], sn[j] = h_kk / r, h_k1k / r
    h[j, j] = cs[j] * h_kk + sn[j] * h_k1k
    h[j + 1, j] = 0.0
    temp = cs[j] * g[j] + sn[j] * g[j + 1]
    g[j + 1] = -sn[j] * g[j] + cs[j] * g[j + 1]
    g[j] = temp


def _back_substitution(h, g, m):   # gmres.rs:180-192
    y = np.zeros(m)
    for i in reversed(range(m)):
        y[i] = g[i]
        for j in range(i + 1, m):
            y[i] = y[i] - h[i, j] * y[j]
        y[i] = y[i] / h[i, i] if abs(h[i, i]) > EPS else 0.0
    return y


def gmres(a, apply, side, b, restart, tol, max_iters, rs):
    """gmres.rs:216-402 with a preconditioner, side "left" or "right", x0 = 0 -> (x, iterations, final_residual, converged, history);
    history: |g[j + 1]| after every rotation (the reference keeps none)."""
    dot = lambda u, v: F(O.dot(u, v, rs))
    norm = lambda u: F(np.sqrt(dot(u, u)))

    def mgs2(z, basis, h, j):      # the double modified Gram-Schmidt (:286-298, :318-330)
        for i in range(j + 1):
            h[i, j] = dot(z, basis[i])
            z = z - h[i, j] * basis[i]
        for i in range(j + 1):
            tmp = dot(z, basis[i])
            h[i, j] = h[i, j] + tmp
            z = z - tmp * basis[i]
        return z

    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=float)
        xk = np.zeros(len(b))
        r0 = b - a.spmv(xk)                                           # :221-227
        beta = norm(r0)
        res0 = beta
        iterations, final_residual, converged = 0, beta, False
        hist = []
        iteration = 0
        for outer in range(-(-max_iters // restart)):                 # :231
            v, zb = [], []
            r0_norm = beta
            if side == "left":                                        # :239-246
                v.append(r0 / r0_norm)
                zb.append(apply(v[0]))
            else:                                                     # :247-260
                z0 = apply(r0)
                r0_norm = norm(z0)
                v.append(z0 / r0_norm)
                zb.append(apply(v[0]))
                beta = r0_norm
            h = np.zeros((restart + 1, restart)); g = np.zeros(restart + 1)
            g[0] = r0_norm
            cs, sn = np.zeros(restart), np.zeros(restart)
            m = 0
            for j in range(restart):
                iteration += 1
                if side == "left":                                    # :279-307
                    z = mgs2(apply(a.spmv(v[j])), zb, h, j)
                    h[j + 1, j] = norm(z)
                    if abs(h[j + 1, j]) < EPS:
                        break
                    v.append(z / h[j + 1, j])
                    zb.append(v[-1].copy())
                else:                                                 # :308-343
                    w = mgs2(a.spmv(apply(v[j])), v, h, j)
                    h[j + 1, j] = norm(w)
                    if abs(h[j + 1, j]) < EPS:
                        break
                    v.append(w / h[j + 1, j])
                    zb.append(apply(v[-1]))
                _givens(h, g, cs, sn, j)                              # :347
                res_norm = abs(g[j + 1])
                hist.append(res_norm)
                stop = bool(res_norm / res0 <= tol) or iteration >= max_iters
                iterations, final_residual, converged = iteration, res_norm, stop
                m = j + 1
                if stop:
                    break
            y = _back_substitution(h, g, m)                           # :358-361
            basis = zb if side == "right" else v                      # :363-386
            for j in range(m):
                xk = xk + y[j] * basis[j]
            r0 = b - a.spmv(xk)                                       # :388-391
            beta = norm(r0)
            final_residual = beta                                     # :393
            converged = bool(beta < tol * res0)                       # :394
            if converged or iteration >= max_iters:
                break
    return xk, iterations, float(final_residual), converged, np.array(hist)


def bicgstab_rpc(a, apply, b, tol, max_iters, rs):
    """bicgstab.rs:69-293 with x0 = 0 and the right-preconditioned extension: v = A (M^-1 p), t = A (M^-1 s),
    x = x + alpha M^-1 p + omega M^-1 s.  `tol` is absolute, as written.  -> (x, iterations, final_residual, converged, history)"""
    dot = lambda u, v: F(O.dot(u, v, rs))
    with np.errstate(all="ignore"):
        b = np.asarray(b, dtype=float)
        x = np.zeros(len(b))
        r = b - a.spmv(x)
        r_hat = r.copy()
        rho_prev = alpha = omega_prev = F(1.0)
        v = np.zeros(len(b))
        p = r.copy()
        res0 = F(np.sqrt(dot(r, r)))
        stats = (0, float(res0), False)
        hist = [res0]
        if res0 <= tol:
            return x, 0, float(res0), True, np.array(hist)
        for i in range(1, max_iters + 1):
            rho = dot(r_hat, r)
            if abs(rho) < DBL_EPS:
                break
            beta = F(0.0) if i == 1 else (rho / rho_prev) * (alpha / omega_prev)
            p = r + beta * (p - omega_prev * v)
            ph = apply(p)
            v = a.spmv(ph)
            alpha_den = dot(r_hat, v)
            if abs(alpha_den) < DBL_EPS:
                break
            alpha = rho / alpha_den
            s = r - alpha * v
            s_norm = F(np.sqrt(dot(s, s)))
            if s_norm <= tol:
                x = x + alpha * ph
                hist.append(s_norm)
                return x, i, float(s_norm), True, np.array(hist)
            sh = apply(s)
            t = a.spmv(sh)
            omega_num = dot(t, s)
            omega_den = dot(t, t)
            if abs(omega_den) < DBL_EPS:
                break
            omega = omega_num / omega_den
            x = x + alpha * ph + omega * sh
            r = s - omega * t
            r_norm = F(np.sqrt(dot(r, r)))
            stats = (i, float(r_norm), bool(r_norm <= tol))
            hist.append(r_norm)
            if r_norm <= tol or abs(omega) < DBL_EPS:
                break
            rho_prev, omega_prev = rho, omega
    return x, stats[0], stats[1], stats[2], np.array(hist)
