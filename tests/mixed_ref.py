"""The numpy restatement of the mixed-precision contract, on top of the CPU oracle.  TEST INFRASTRUCTURE ONLY.

fp32 is a storage format: every array that the library keeps in fp32 is a float32 array here; every operation widens it (astype(float64),
exact), runs the oracle's own fp64 `spmv` / `dot` or a numpy expression with separate multiply and add, and rounds once with
astype(float32) where the library stores.  Inner products of fp32-stored vectors use the oracle's tiled fold at T = 256, V = 4 (RS32); the
outer fp64 work of the refinement uses the library's fp64 tree (RS64).  The loops are written against cg.rs / pcg.rs with the exits of
kryst_amd/csrc/cg_logic.h."""
import numpy as np

from oracle import oracle as O

F32, F64 = np.float32, np.float64
OK, INDEFINITE_MATRIX, INDEFINITE_PC, UNSUPPORTED = 0, 3, 4, 6
SPEC32 = (256, 4, 1024)
RS32 = O.Reduce.tiled(T=256, V=4, F=1024)
RS64 = O.Reduce.tiled(T=256, V=2, F=1024)
TINY32 = float(np.finfo(np.float32).tiny)


def wide(v):
    return np.ascontiguousarray(v, dtype=F64)


def store(v):
    """the one rounding of a store"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, dtype=F64).astype(F32)


def round_f32(values):
    """-> (float32 array, changed, tiny, overflow): values the rounding changed, nonzero values that became zero or fp32-subnormal, finite
    values that became +-inf (the lowering is refused when there is one).  A NaN stays a NaN and counts as nothing."""
    v = np.asarray(values, dtype=F64).ravel()
    out = store(v)
    back = out.astype(F64)
    ok = ~np.isnan(v)
    changed = int(np.count_nonzero(ok & (back != v)))
    tiny = int(np.count_nonzero(ok & (v != 0.0) & (np.abs(out) < TINY32)))
    overflow = int(np.count_nonzero(np.isfinite(v) & np.isinf(out)))
    return out, changed, tiny, overflow


class Lowered:
    """CsrMatrix.lower(): the operator with fp32-stored values"""

    def __init__(self, a):
        self.vals32, self.changed, self.tiny, overflow = round_f32(a.vals)
        if overflow:
            raise O.KrylovError(UNSUPPORTED)
        self.nrows, self.ncols = a.nrows, a.ncols
        self.wide = O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, self.vals32.astype(F64), check=False)
        self.info = {"changed": self.changed, "tiny": self.tiny, "rows": a.nrows}

    def spmv(self, x32):
        assert x32.dtype == F32
        with np.errstate(all="ignore"):
            return store(self.wide.spmv(wide(x32)))


def dot32(x32, y32, rs=RS32):
    assert x32.dtype == F32 and y32.dtype == F32
    return F64(O.dot(wide(x32), wide(y32), rs))


class Out:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check(res, res0, i, tol, max_iters):
    """Convergence::check (convergence.rs:18-34)"""
    with np.errstate(all="ignore"):
        rel = F64(res) / F64(res0)
    return bool(rel <= tol) or i >= max_iters


def cg32(a32, b32, x32, tol, max_iters, rs=RS32, watch=None):
    """kryst_cg32_solve_dev: cg.rs:114-288 with norm type Preconditioned / Unpreconditioned (both (r, r)).  watch(i, ap, x, r, p), if
    given, sees the stored vectors of iteration i after its x and r updates (p: the direction the iteration used)"""
    with np.errstate(all="ignore"):
        x = x32.copy()
        r = store(wide(b32) - wide(a32.spmv(x)))                        # cg.rs:120-125
        p = r.copy()                                                    # :126
        rsq = dot32(r, r, rs)                                           # :127
        res0 = np.sqrt(rsq)
        out = Out(code=OK, x=x32.copy(), iterations=0, final_residual=float(res0), converged=False, history=[float(np.sqrt(rsq))])
        if max_iters <= 0:
            return out
        for i in range(1, max_iters + 1):
            ap = a32.spmv(p)                                            # :143-144
            pap = dot32(p, ap, rs)
            if pap <= 0.0:                                              # :168-174
                out.iterations, out.final_residual, out.converged, out.code = i, float(np.sqrt(rsq)), False, INDEFINITE_MATRIX
                return out
            alpha = rsq / pap                                           # :175
            x = store(wide(x) + alpha * wide(p))                        # :207-209
            r = store(wide(r) - alpha * wide(ap))                       # :210-212
            if watch is not None:
                watch(i, ap, x, r, p)
            rsq_new = dot32(r, r, rs)                                   # :223
            res = np.sqrt(rsq_new)
            if rsq_new / rsq < 0.0:                                     # :254-259
                out.iterations, out.final_residual, out.converged, out.code = i, float(res), False, INDEFINITE_PC
                return out
            out.history.append(float(res))
            conv = _check(res, res0, i, tol, max_iters)
            out.iterations, out.final_residual, out.converged = i, float(res), conv
            if conv:
                break
            beta = rsq_new / rsq                                        # :270
            p = store(wide(r) + beta * wide(p))                         # :274-276
            rsq = rsq_new
        out.x = x
        return out


def pcg32(a32, inv_diag, b32, x32, tol, max_iters, norm_type=1, rs=RS32):
    """kryst_pcg32_solve_dev: pcg.rs:114-222; inv_diag: the fp64 Jacobi values (rounded to fp32 once here) or None (z == r)"""
    with np.errstate(all="ignore"):
        d32 = None if inv_diag is None else store(inv_diag)

        def apply(r):
            return r if d32 is None else store(wide(d32) * wide(r))      # jacobi.rs:84-86

        def second(r, z):
            return dot32(z, z, rs) if norm_type == 0 else dot32(r, r, rs)

        x = x32.copy()
        r = store(wide(b32) - wide(a32.spmv(x)))
        z = apply(r)
        p = z.copy()
        rz = dot32(r, z, rs)                                            # :133
        res0 = np.sqrt(np.abs(rz))                                      # :134
        normq = second(r, z)
        out = Out(code=OK, x=x32.copy(), iterations=0, final_residual=float(res0), converged=False, history=[float(np.sqrt(normq))])
        if max_iters <= 0:
            return out
        for i in range(1, max_iters + 1):
            ap = a32.spmv(p)
            pap = dot32(p, ap, rs)
            if pap <= 0.0:                                              # :162-172
                out.iterations, out.final_residual, out.converged, out.code = i, float(np.sqrt(normq)), False, INDEFINITE_MATRIX
                return out
            alpha = rz / pap                                            # :173
            x = store(wide(x) + alpha * wide(p))
            r = store(wide(r) - alpha * wide(ap))
            z = apply(r)
            rz_new = dot32(r, z, rs)                                    # :188
            normq = second(r, z)
            res = np.sqrt(normq)
            out.history.append(float(res))
            conv = _check(res, res0, i, tol, max_iters)
            out.iterations, out.final_residual, out.converged = i, float(res), conv
            if conv:
                break
            beta = rz_new / rz                                          # :206
            if beta < 0.0:                                              # :208-213
                out.converged, out.code = False, INDEFINITE_PC
                return out
            p = store(wide(z) + beta * wide(p))
            rz = rz_new
        out.x = x
        return out


def refine(a, a32, inv_diag, b, x0, outer_tol, max_outer, inner_tol, inner_max, rs64=RS64, rs32=RS32):
    """kryst_refine_solve_dev.  a: the fp64 oracle operator; a32: Lowered(a); inv_diag: None (inner CG) or the fp64 Jacobi values (inner
    Jacobi-PCG).  -> Out(code, x, iterations, final_residual, converged, history, inner_iterations, rejected)"""
    with np.errstate(all="ignore"):
        b = wide(b)
        x = wide(x0).copy()
        r = b - a.spmv(x)
        rho = np.sqrt(F64(O.dot(r, r, rs64)))
        rho0 = rho
        out = Out(code=OK, x=x.copy(), iterations=0, final_residual=float(rho0), converged=False, history=[float(rho0)],
                  inner_iterations=[], rejected=False)
        if max_outer <= 0 or rho0 == 0.0:
            out.converged = True
            return out
        for k in range(1, max_outer + 1):
            r32 = store(r / rho)
            c0 = np.zeros(a.nrows, dtype=F32)
            inner = cg32(a32, r32, c0, inner_tol, inner_max, rs32) if inv_diag is None else \
                pcg32(a32, inv_diag, r32, c0, inner_tol, inner_max, 1, rs32)
            out.inner_iterations.append(inner.iterations)
            if inner.code != OK:
                out.code, out.iterations, out.final_residual, out.converged = inner.code, k - 1, float(rho), False
                out.x = wide(x0).copy()
                return out
            xn = x + rho * wide(inner.x)
            rn = b - a.spmv(xn)
            rho_new = np.sqrt(F64(O.dot(rn, rn, rs64)))
            out.history.append(float(rho_new))
            if not (rho_new < rho):
                out.iterations, out.final_residual, out.converged, out.rejected = k, float(rho), False, True
                break
            x, r, rho = xn, rn, rho_new
            conv = _check(rho, rho0, k, outer_tol, max_outer)
            out.iterations, out.final_residual, out.converged = k, float(rho), conv
            if conv:
                break
        out.x = x
        return out
