#!/usr/bin/env python3
"""SPAI set-up measurements: one JSON line per case on stdout.

  spai_only.py setup N           the set-up with the operator's pattern on the N^3 Poisson / anisotropic / convection-diffusion operators:
                                 wall ms of the whole synchronous call (host perf_counter around it, the stream synchronised before and
                                 after; not HIP events), the first set-up and four more on the same operator, nnz(M) against nnz(A)
  spai_only.py apply N           kryst_bench_pc_apply of the SPAI preconditioner (Poisson, operator pattern, tol 1e-12) against
                                 kryst_bench_spmv of A in the plain CSR form (KRYST_SPMV_COMPRESS=0, the form of value_sec8d), 20 applies each
  spai_only.py solve N           time to solution (set-up + solve, tol 1e-8): config 5's operator (anisotropic) with right-preconditioned
                                 BiCGStab and true ILU(0) / SPAI / Jacobi; config 3's operator (convection-diffusion) with GMRES(30), 600
                                 iterations, Jacobi / SPAI (left, as config 3, and right)

Bytes of one apply (plain CSR, M with A's pattern): 12 nnz (col + val) + 4 n (row_ptr) + 8 n (r, once when cached) + 8 n (z)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import kryst_amd as K
from kryst_amd import _ffi

PEAK = 8.0e12
OP = K.SparsityPattern.Operator


def nnz_of(a):
    v = C.c_int64()
    _ffi.check(_ffi.lib().kryst_csr_shape(a.h, None, None, C.byref(v)))
    return v.value


def m_nnz(pc):
    v = C.c_int64()
    _ffi.check(_ffi.lib().kryst_pc_spai_export(pc.h, C.byref(v), None, None, None))
    return v.value


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def setup_cases(N):
    ctx = K.Context(0)
    for kind in ("poisson", "aniso", "convdiff"):
        a = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        nnz_a = nnz_of(a)
        pc, ms1 = timed(lambda: K.Spai(OP, 1e-12).setup(a), ctx)
        rp_nnz = m_nnz(pc)
        later = []
        for _ in range(4):
            del pc
            pc, ms = timed(lambda: K.Spai(OP, 1e-12).setup(a), ctx)
            later.append(round(ms, 2))
        print(json.dumps({"case": "setup", "N": N, "kind": kind, "setup_ms_first": round(ms1, 2), "setup_ms_later": later,
                          "setup_ms_median": sorted(later)[len(later) // 2], "nnz_A": nnz_a, "nnz_M": rp_nnz}), flush=True)
        del pc, a


def apply_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    nnz = nnz_of(a)
    pc = K.Spai(OP, 1e-12).setup(a)
    r = ctx.vec(n).fill_splitmix(3)
    z = ctx.vec(n)
    byts = 12 * nnz + 4 * n + 16 * n
    ms_pc = sorted(pc.bench_apply(r, z, reps=20) for _ in range(3))[1]
    os.environ["KRYST_SPMV_COMPRESS"] = "0"
    ms_a = sorted(a.bench_spmv(r, z, fused_dots=0, reps=20) for _ in range(3))[1]
    del os.environ["KRYST_SPMV_COMPRESS"]
    for name, ms in (("spai_apply", ms_pc), ("spmv_A_plain_csr", ms_a)):
        print(json.dumps({"case": name, "N": N, "ms": round(ms, 4), "bytes": byts, "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 3)}), flush=True)
    print(json.dumps({"case": "apply_ratio", "N": N, "spai_over_spmv": round(ms_pc / ms_a, 4)}), flush=True)


def solve_cases(N):
    ctx = K.Context(0)

    def run(config, kind, pc_name, make_pc, make_solver, abs_tol):
        a = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        n = a.nrows()
        b = a.spmv(ctx.vec(n).fill(1.0))
        bn = K.norm(b)
        pc, setup_ms = timed(lambda: make_pc(a), ctx)
        best = None
        for _ in range(2):                                     # the first solve also sizes the solver's work arena
            s = make_solver(1e-8 * bn if abs_tol else 1e-8)
            x = ctx.vec(n)
            try:
                st, ms = timed(lambda: s.solve(a, pc, b, x), ctx)
            except K.KError as e:                              # not converged within the iteration limit
                st, ms = e.stats, None
                ctx.synchronize()
            if best is None or (ms is not None and (best[1] is None or ms < best[1])):
                best = (st, ms)
        st, ms = best
        print(json.dumps({"case": config, "N": N, "pc": pc_name, "iterations": st.iterations, "converged": bool(st.converged),
                          "final_residual": st.final_residual, "setup_ms": round(setup_ms, 2),
                          "solve_ms": None if ms is None else round(ms, 2),
                          "total_ms": None if ms is None else round(setup_ms + ms, 2)}), flush=True)
        del pc, a

    bicg = lambda t: K.BiCgStabRightPcSolver(t, 3000)
    for name, mk in (("true_ilu0", lambda a: K.TrueIlu0().setup(a)), ("spai", lambda a: K.Spai(OP, 1e-12).setup(a)),
                     ("jacobi", lambda a: K.Jacobi().setup(a))):
        run("config5_bicgstab_rpc_aniso", "aniso", name, mk, bicg, True)
    for side in (K.Preconditioning.Left, K.Preconditioning.Right):
        gm = lambda t, side=side: K.GmresSolver(30, t, 600).with_preconditioning(side)
        for name, mk in (("jacobi", lambda a: K.Jacobi().setup(a)), ("spai", lambda a: K.Spai(OP, 1e-12).setup(a))):
            run(f"config3_gmres30_{side.name.lower()}_convdiff", "convdiff", name, mk, gm, False)


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    {"setup": setup_cases, "apply": apply_cases, "solve": solve_cases}[mode](N)
