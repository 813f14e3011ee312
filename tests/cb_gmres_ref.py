"""The numpy restatement of compressed-basis GMRES (kryst_amd/csrc/gmres_cb.hip), on top of the CPU oracle.
TEST INFRASTRUCTURE ONLY.

The Krylov basis is a list of arrays in the storage type: `store` rounds once where the library stores a basis vector (v_0 = r / beta and
v_{j+1} = z / h[j+1][j]), `wide` widens exactly what was stored at every later use (the operand of the next SpMV / preconditioner apply,
B_i of every Gram-Schmidt link and dot, the x update).  Everything else is fp64: the oracle's own `spmv`, `dot` with the library's tree
(RS64) and preconditioner applies, numpy expressions with separate multiply and add, Python floats for the small least-squares problem.
The loop is written against gmres.rs:216-402 side None (through arnoldi :65-105, as oracle/kryst_oracle.c restates it), plus textbook
right preconditioning: Arnoldi on A M^-1 from the true residual, only V kept, x += M^-1 (sum_j y_j V_j, ascending j from zero)."""
import numpy as np

from oracle import oracle as O
from mixed_ref import F32, F64, RS64, Out, store as store32, wide

SIDE_NONE, SIDE_RIGHT = 0, 2
EPS = 1e-14                                                             # gmres.rs:233


def store64(v):
    """the control: nothing is rounded"""
    return np.array(v, dtype=F64)


STORES = {"f32": store32, "f64": store64}


def _givens(h, g, cs, sn, j):
    """apply_givens_and_update_g (gmres.rs:154-176); h[i][k] Python floats"""
    for i in range(j):
        temp = cs[i] * h[i][j] + sn[i] * h[i + 1][j]
        h[i + 1][j] = -sn[i] * h[i][j] + cs[i] * h[i + 1][j]
        h[i][j] = temp
    h_kk, h_k1k = h[j][j], h[j + 1][j]
    r = float(np.sqrt(F64(h_kk * h_kk + h_k1k * h_k1k)))
    if abs(r) < EPS:
        cs[j], sn[j] = 1.0, 0.0
    else:
        cs[j], sn[j] = float(F64(h_kk) / F64(r)), float(F64(h_k1k) / F64(r))
    h[j][j] = cs[j] * h_kk + sn[j] * h_k1k
    h[j + 1][j] = 0.0
    temp = cs[j] * g[j] + sn[j] * g[j + 1]
    g[j + 1] = -sn[j] * g[j] + cs[j] * g[j + 1]
    g[j] = temp


def _back(h, g, m):
    """back_substitution (gmres.rs:180-192)"""
    y = [0.0] * len(g)
    for i in range(m - 1, -1, -1):
        s = g[i]
        for k in range(i + 1, m):
            s = s - h[i][k] * y[k]
        y[i] = float(F64(s) / F64(h[i][i])) if abs(h[i][i]) > EPS else 0.0
    return y


def _norm(v, rs):
    return float(np.sqrt(F64(O.dot(v, v, rs))))


def cbgmres(a, b, x0, pc=None, side=SIDE_RIGHT, restart=30, tol=1e-8, max_iters=1000, basis="f32", rs=RS64, store=None):
    """kryst_cbgmres_solve_dev.  a: oracle Csr; pc: oracle Pc or None (then side is None, as in the library); basis "f32" | "f64" picks
    `store` unless one is given.  -> Out(x, iterations, final_residual, converged, history, basis = the stored vectors of the last cycle)"""
    store = STORES[basis] if store is None else store
    if pc is None:
        side = SIDE_NONE
    assert side in (SIDE_NONE, SIDE_RIGHT) and restart >= 1
    with np.errstate(all="ignore"):
        b = wide(b)
        xk = wide(x0).copy()                                            # :219
        r0 = b - a.spmv(xk)                                             # :221-226
        beta = _norm(r0, rs)                                            # :227
        res0 = beta                                                     # :228
        out = Out(x=xk.copy(), iterations=0, final_residual=beta, converged=False, history=[], basis=[])
        n_outer = (max_iters + restart - 1) // restart                  # :231
        iteration = 0
        for _ in range(n_outer):                                        # :234
            r0_norm = beta                                              # :238
            V = [store(r0 / F64(r0_norm))]                              # :242 / :263 -- on either side: the TRUE residual
            h = [[0.0] * restart for _ in range(restart + 1)]           # :268
            g = [0.0] * (restart + 1)
            g[0] = r0_norm                                              # :270
            cs, sn = [0.0] * restart, [0.0] * restart
            m, happy = 0, False
            for j in range(restart):                                    # :276
                iteration += 1                                          # :277
                vj = wide(V[j])
                z = a.spmv(pc.apply(vj)) if side == SIDE_RIGHT else a.spmv(vj)      # arnoldi :79-81 / w = M^-1 v_j, z = A w
                for sweep in range(2):                                  # double modified Gram-Schmidt (:83-96)
                    for i in range(j + 1):
                        bi = wide(V[i])
                        d = F64(O.dot(z, bi, rs))
                        h[i][j] = float(d) if sweep == 0 else h[i][j] + float(d)
                        t = d * bi
                        z = z - t
                hj1 = _norm(z, rs)                                      # :97
                h[j + 1][j] = hj1
                if abs(hj1) < EPS:                                      # :98-101 returns true, no push, Givens still applied
                    happy = True
                else:
                    V.append(store(z / F64(hj1)))                       # :102-103
                _givens(h, g, cs, sn, j)                                # :347
                res_norm = abs(g[j + 1])                                # :348
                rel = F64(res_norm) / F64(res0)                         # Convergence::check (convergence.rs:18-34)
                conv = bool(rel <= tol) or iteration >= max_iters
                out.iterations, out.final_residual, out.converged = iteration, res_norm, conv
                out.history.append(res_norm)
                m = j + 1                                               # :351
                if conv or happy:                                       # :352-354
                    break
            y = _back(h, g, m)                                          # :357-360
            if side == SIDE_RIGHT:
                u = np.zeros(a.nrows)
                for k in range(m):
                    t = F64(y[k]) * wide(V[k])
                    u = u + t
                xk = xk + pc.apply(u)
            else:
                for k in range(m):                                      # :362-386
                    t = F64(y[k]) * wide(V[k])
                    xk = xk + t
            r0 = b - a.spmv(xk)                                         # :388-391
            beta = _norm(r0, rs)                                        # :392
            out.final_residual = beta                                   # :394
            out.converged = bool(beta < tol * res0)                     # :395
            out.basis = V
            if out.converged or iteration >= max_iters:                 # :396-398
                break
        out.x = xk
        return out
