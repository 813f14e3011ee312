#!/usr/bin/env python3
"""SOR / SSOR measurements: one JSON line per case on stdout.

  sor_only.py apply N     N^3 Poisson: the SSOR apply as written and in the red-black order (kryst_bench_pc_apply, 20 back-to-back
                          applies), passes per sweep, the bytes model and its fraction of 8 TB/s; beside them the two yardsticks on the
                          same operator: the ILU(0) apply and two SpMVs (the operator's own encoding, and plain CSR: the sweep's bytes)
  sor_only.py pcg N       PCG to 1e-8 on the N^3 Poisson operator with SSOR as written, red-black SSOR, Jacobi and ILU(0): iterations,
                          set-up ms, solve ms, iterations per second

Bytes per sweep and row of a 7-point operator: row pointer 4, row id 4, seven columns and values 84, inv_diag 8, x 8, y written 8 and six
neighbours of x or y gathered (counted once each: 8) = 124; the coloured order adds the position 4 and the entry order 28 = 156.  The SSOR
apply is two sweeps."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K

PEAK = 8.0e12
BYTES_ROW = {"as_written": 124, "red_black": 156}


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def red_black(N):
    r = np.arange(N ** 3, dtype=np.int64)
    return (r % N + (r // N) % N + r // (N * N)) % 2


def make(order, N):
    s = K.Sor(1.0, 1, 1, K.MatSorType.SYMMETRIC_SWEEP, 0.0)
    return s.with_colors(red_black(N)) if order == "red_black" else s


def apply_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    r = ctx.vec(n).fill_splitmix(3)
    z = ctx.vec(n)
    for order in os.environ.get("SOR_ONLY_ORDERS", "as_written,red_black").split(","):
        pc, setup_ms = timed(lambda: make(order, N).setup(a), ctx)
        ms = sorted(pc.bench_apply(r, z, reps=20) for _ in range(5))[2]
        byts = 2 * BYTES_ROW[order] * n
        print(json.dumps({"case": "apply", "N": N, "pc": "ssor_" + order, **pc.info(), "setup_ms": round(setup_ms, 2), "apply_ms": round(ms, 4),
                          "bytes_per_row_per_sweep": BYTES_ROW[order], "TBps": round(byts / ms / 1e9, 3),
                          "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 4)}), flush=True)
        del pc
    pc, setup_ms = timed(lambda: K.TrueIlu0().setup(a), ctx)
    ms = sorted(pc.bench_apply(r, z, reps=20) for _ in range(5))[2]
    print(json.dumps({"case": "apply", "N": N, "pc": "ilu0", "form": pc.ilu_info()["form"], "setup_ms": round(setup_ms, 2), "apply_ms": round(ms, 4)}), flush=True)
    del pc
    ms = sorted(a.bench_spmv(r, z, fused_dots=0, reps=20) for _ in range(5))[2]
    print(json.dumps({"case": "apply", "N": N, "pc": "two_spmv", "encoding": a.encoding()[0], "apply_ms": round(2 * ms, 4)}), flush=True)
    # the yardstick with the sweep's bytes: the same operator through the plain-CSR kernel (KRYST_SPMV_COMPRESS=0, bench.py's value_sec8d)
    os.environ["KRYST_SPMV_COMPRESS"] = "0"
    ms = sorted(a.bench_spmv(r, z, fused_dots=0, reps=20) for _ in range(5))[2]
    os.environ.pop("KRYST_SPMV_COMPRESS")
    print(json.dumps({"case": "apply", "N": N, "pc": "two_spmv_plain_csr", "apply_ms": round(2 * ms, 4)}), flush=True)


def pcg_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    bv = a.spmv(ctx.vec(n).fill(1.0))
    pcs = (("ssor_as_written", lambda: make("as_written", N).setup(a)), ("ssor_red_black", lambda: make("red_black", N).setup(a)),
           ("jacobi", lambda: K.Jacobi().setup(a)), ("ilu0", lambda: K.TrueIlu0().setup(a)))
    for name, mk in pcs:
        pc, setup_ms = timed(mk, ctx)
        for rep in range(2):                                   # the first solve also sizes the solver's work arena
            xv = ctx.vec(n).fill(0.0)
            s = K.PcgSolver(1e-8, 20000)
            st, ms = timed(lambda: s.solve(a, pc, bv, xv), ctx)
        print(json.dumps({"case": "pcg_poisson", "N": N, "pc": name, "iterations": st.iterations, "converged": st.converged,
                          "final_residual": st.final_residual, "setup_ms": round(setup_ms, 2), "solve_ms": round(ms, 2),
                          "iterations_per_s": round(st.iterations / (ms * 1e-3), 1)}), flush=True)
        del pc


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    {"apply": apply_cases, "pcg": pcg_cases}[mode](N)
