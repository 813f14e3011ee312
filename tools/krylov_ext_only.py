#!/usr/bin/env python3
"""MINRES / QMR / CGNR (as written and textbook) stepping sessions and the transposed SpMV on a 7-point Poisson operator, one JSON line
per measurement (profiles/krylov_ext/).  Like bench.py, iterations are timed through a session: W warm-up steps, then K steps between two
stream synchronisations, host clock.  KRYST_SPMV_COMPRESS=0 in the environment selects plain CSR.

usage: krylov_ext_only.py solve [grid=256] [steps=50] [methods=minres_textbook,cgnr_textbook,minres,qmr,cgnr]
       krylov_ext_only.py spmv  [grid=256] [reps=50]      (A^T set-up time, then kryst_spmv_transpose against kryst_spmv)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K


def form():
    return "plain-csr" if os.environ.get("KRYST_SPMV_COMPRESS") == "0" else "default"


def solve(grid, steps, methods):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
    n = a.nrows()
    b = a.spmv(ctx.vec(n).fill(1.0))
    if any(m.endswith("textbook") and m.startswith("cgnr") for m in methods):
        t0 = time.perf_counter(); a.spmv_transpose(ctx.vec(n).fill(1.0)); ctx.synchronize()
        print(json.dumps({"what": "at_setup_in_solve_run", "grid": grid, "form": form(), "s": time.perf_counter() - t0}), flush=True)
    warm = 5
    for m in methods:
        x = ctx.vec(n)
        with K.Session(m, a, None, b, x, tol=0.0, max_iters=warm + steps) as s:
            s.step(warm); ctx.synchronize()
            t0 = time.perf_counter()
            s.step(steps); ctx.synchronize()
            dt = time.perf_counter() - t0
            st = s.end()
        print(json.dumps({"what": "solve", "method": m, "grid": grid, "form": form(), "encoding": a.encoding()[0], "steps": steps,
                          "iterations": st.iterations, "it_per_s": steps / dt}), flush=True)


def spmv(grid, reps):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
    n = a.nrows()
    x = ctx.vec(n).fill(1.0); y = ctx.vec(n)
    ctx.synchronize()
    t0 = time.perf_counter(); a.spmv_transpose(x, y); ctx.synchronize()
    setup = time.perf_counter() - t0
    out = {"what": "spmv", "grid": grid, "form": form(), "encoding": a.encoding()[0], "at_setup_s": setup}
    for name, f in (("forward", lambda: a.spmv(x, y)), ("transpose", lambda: a.spmv_transpose(x, y))):
        for _ in range(3):
            f()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        ctx.synchronize()
        out[name + "_ms"] = (time.perf_counter() - t0) / reps * 1e3
    out["transpose_over_forward"] = out["transpose_ms"] / out["forward_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "solve"
    grid = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    if what == "spmv":
        spmv(grid, int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    else:
        steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
        methods = (sys.argv[4] if len(sys.argv) > 4 else "minres_textbook,cgnr_textbook,minres,qmr,cgnr").split(",")
        solve(grid, steps, methods)
