#!/usr/bin/env python3
"""Chebyshev polynomial preconditioner measurements: one JSON line per case on stdout.

  cheb_poly_only.py apply N    N^3 Poisson, degree 4, Jacobi scaling: the apply (kryst_bench_pc_apply, 10 back-to-back applies per sample, five
                               alternating rounds, median) in the fused and the unfused form on the plain CSR arrays (KRYST_SPMV_COMPRESS=0
                               at creation; KRYST_CHEB_POLY_FUSE picks the form) and in the unfused form on the operator's default
                               encoding; the byte model and its share of 8 TB/s
  cheb_poly_only.py pcg N      PCG to 1e-8, b = A 1: ChebyshevPoly(4) with estimated bounds against Jacobi, alternating; iterations, seconds
  cheb_poly_only.py gmres N    convection-diffusion, GMRES(30) right to 1e-8 (at most 600 iterations): ChebyshevPoly(4) against Jacobi
  cheb_poly_only.py trace N    three applies of each form and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run

Bytes per row and step (section 4.15): fused 12 nnz/n + 4 + 8 + 48 (+ 8 scaled); unfused 12 nnz/n + 4 + 16 for the plain SpMV (CSR-P16:
2 + 16) plus 64 (+ 8 scaled) for the pass; the first pass d_0 = (w r) / theta adds 24 per row."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K

PEAK = 8.0e12
DEGREE = 4


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, time.perf_counter() - t0


def with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def forms(ctx, N, bounds):
    """name -> (operator, preconditioner, modelled bytes per apply)"""
    plain = with_env({"KRYST_SPMV_COMPRESS": "0"}, lambda: K.CsrMatrix.stencil7(N, "poisson", ctx=ctx))
    dflt = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n, nnzr = plain.nrows(), plain.nnz / plain.nrows()
    mk = lambda a: K.ChebyshevPoly(DEGREE, *bounds).setup(a)                                                   # noqa: E731
    out = {
        "fused_plain": (plain, with_env({"KRYST_SPMV_COMPRESS": "0", "KRYST_CHEB_POLY_FUSE": "1"}, lambda: mk(plain)),
                        n * (DEGREE * (12 * nnzr + 4 + 8 + 56) + 24)),
        "unfused_plain": (plain, with_env({"KRYST_SPMV_COMPRESS": "0", "KRYST_CHEB_POLY_FUSE": "0"}, lambda: mk(plain)),
                          n * (DEGREE * (12 * nnzr + 4 + 16 + 72) + 24)),
        "unfused_default": (dflt, mk(dflt), n * (DEGREE * ((2 if dflt.encoding()[0] == "csr-p16" else 12 * nnzr + 4) + 16 + 72) + 24)),
    }
    assert out["fused_plain"][1].info()["fused"] and not out["unfused_plain"][1].info()["fused"] and not out["unfused_default"][1].info()["fused"]
    return out


def run_form(name, a, pc, fn):
    """the plain forms run with the plain kernel selected, as at their creation"""
    return with_env({"KRYST_SPMV_COMPRESS": "0"}, fn) if name.endswith("plain") else fn()


def apply_cases(N):
    ctx = K.Context(0)
    f = forms(ctx, N, (0.06, 2.0))
    n = f["fused_plain"][0].nrows()
    r, z = ctx.vec(n).fill_splitmix(3), ctx.vec(n)
    samples = {k: [] for k in f}
    for _ in range(5):
        for name, (a, pc, _) in f.items():
            samples[name].append(run_form(name, a, pc, lambda: pc.bench_apply(r, z, reps=10)))
    for name, (a, pc, byts) in f.items():
        ms = sorted(samples[name])[2]
        print(json.dumps({"case": "apply", "N": N, "form": name, "degree": DEGREE, "encoding": a.encoding()[0] if name == "unfused_default" else "csr",
                          "apply_ms": round(ms, 4), "min_ms": round(min(samples[name]), 4), "max_ms": round(max(samples[name]), 4),
                          "model_bytes": int(byts), "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 4), "sources": K._ffi.source_sha16()}), flush=True)


def trace_cases(N):
    ctx = K.Context(0)
    f = forms(ctx, N, (0.06, 2.0))
    n = f["fused_plain"][0].nrows()
    r, z = ctx.vec(n).fill_splitmix(3), ctx.vec(n)
    for name, (a, pc, _) in f.items():
        for _ in range(3):
            run_form(name, a, pc, lambda: pc.apply(r, z))
    ctx.synchronize()
    print(json.dumps({"case": "trace", "N": N, "applies_per_form": 3}), flush=True)


def solve_cases(N, kind, make_solver, label):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    n = a.nrows()
    bv = a.spmv(ctx.vec(n).fill(1.0))
    pcs = {}
    for name, mk in (("chebyshev_poly_4", lambda: K.ChebyshevPoly(DEGREE).setup(a)), ("jacobi", lambda: K.Jacobi().setup(a))):
        pc, setup_s = timed(mk, ctx)
        pcs[name] = (pc, setup_s)
    best = {}
    for _ in range(3):                                         # alternating; the first round also sizes the solver's work arena
        for name, (pc, setup_s) in pcs.items():
            xv = ctx.vec(n).fill(0.0)
            s = make_solver()
            try:
                st, sec = timed(lambda: s.solve(a, pc, bv, xv), ctx)
            except K.KError as e:                              # not converged within the cap: the stats ride on the error
                st, sec = e.stats, float("nan")
            if name not in best or sec < best[name][1]:
                best[name] = (st, sec)
    for name, (st, sec) in best.items():
        pc, setup_s = pcs[name]
        row = {"case": label, "N": N, "pc": name, "encoding": a.encoding()[0], "iterations": st.iterations, "converged": bool(st.converged),
               "final_residual": st.final_residual, "setup_s": round(setup_s, 4), "solve_s": round(sec, 5), "sources": K._ffi.source_sha16()}
        if name == "chebyshev_poly_4":
            row.update({k: pc.info()[k] for k in ("lambda_min", "lambda_max", "fused")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    if mode == "apply":
        apply_cases(N)
    elif mode == "trace":
        trace_cases(N)
    elif mode == "pcg":
        solve_cases(N, "poisson", lambda: K.PcgSolver(1e-8, 20000), "pcg_poisson")
    elif mode == "gmres":
        solve_cases(N, "convdiff", lambda: K.GmresSolver(30, 1e-8, 600).with_preconditioning(K.Preconditioning.Right), "gmres30_right_convdiff")
    else:
        sys.exit(f"unknown mode {mode}")
