#!/usr/bin/env python3
"""Block Jacobi measurements: one JSON line per case on stdout.

  bjacobi_only.py apply N        contiguous b in {4, 8, 16, 32, 64} and one overlapping index-set form on the N^3 Poisson operator: set-up ms,
                                 apply ms (kryst_bench_pc_apply, 20 back-to-back applies), the bytes model and its fraction of 8 TB/s
  bjacobi_only.py pcg N          PCG on the anisotropic N^3 operator, Jacobi against block Jacobi b in {8, 16, 64}: iterations, set-up ms,
                                 solve ms (tol 1e-8, device vectors)

Bytes per apply, contiguous form: 8 sum_k b_k^2 (tiles) + 8 n (r) + 8 n (z).  Index-set form: 8 sum b_k^2 + 4 sum b_k (indices)
+ 8 sum b_k (r gathered) + 4 sum b_k (owner test) + 8 n (z)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K

PEAK = 8.0e12


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def apply_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    r = ctx.vec(n).fill_splitmix(3)
    z = ctx.vec(n)
    for b in (4, 8, 16, 32, 64):
        pc, setup_ms = timed(lambda: K.BlockJacobi.uniform(b).setup(a), ctx)
        _, setup2_ms = timed(lambda: K.BlockJacobi.uniform(b).setup(a), ctx)       # second set-up: allocation warm
        ms = pc.bench_apply(r, z, reps=20)
        full, last = divmod(n, b)
        byts = 8 * (full * b * b + last * last) + 16 * n
        print(json.dumps({"case": "apply_uniform", "N": N, "b": b, "setup_ms": round(setup_ms, 3), "setup_ms_2nd": round(setup2_ms, 3),
                          "apply_ms": round(ms, 4), "bytes": byts, "TBps": round(byts / ms / 1e9, 3),
                          "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 3)}), flush=True)
        del pc
    # index sets: blocks of 8 rows that start every 6 rows (each overlaps the next by 2 rows), handed over in descending order
    starts = np.arange(0, n - 8 + 1, 6, dtype=np.int64)
    idx = (starts[:, None] + np.arange(7, -1, -1, dtype=np.int64)[None, :]).ravel()
    ptr = np.arange(0, len(idx) + 1, 8, dtype=np.int64)
    pc, setup_ms = timed(lambda: K.BlockJacobi((ptr, idx)).setup(a), ctx)
    ms = pc.bench_apply(r, z, reps=20)
    s = len(idx)
    byts = 8 * len(starts) * 64 + 4 * s + 8 * s + 4 * s + 8 * n
    print(json.dumps({"case": "apply_index_sets_overlap", "N": N, "b": 8, "stride": 6, "nblocks": len(starts), "setup_ms": round(setup_ms, 3),
                      "apply_ms": round(ms, 4), "bytes": byts, "TBps": round(byts / ms / 1e9, 3),
                      "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 3)}), flush=True)


def pcg_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "aniso", ctx=ctx)
    n = a.nrows()
    bv = a.spmv(ctx.vec(n).fill(1.0))
    for name, mk in (("jacobi", lambda: K.Jacobi().setup(a)),) + tuple(
            (f"block_jacobi_b{b}", (lambda b=b: K.BlockJacobi.uniform(b).setup(a))) for b in (8, 16, 64)):
        pc, setup_ms = timed(mk, ctx)
        for rep in range(2):                                   # the first solve also sizes the solver's work arena
            xv = ctx.vec(n).fill(0.0)
            s = K.PcgSolver(1e-8, 20000)
            st, ms = timed(lambda: s.solve(a, pc, bv, xv), ctx)
        print(json.dumps({"case": "pcg_aniso", "N": N, "pc": name, "iterations": st.iterations, "converged": st.converged,
                          "final_residual": st.final_residual, "setup_ms": round(setup_ms, 3), "solve_ms": round(ms, 2),
                          "total_ms": round(setup_ms + ms, 2), "ms_per_iteration": round(ms / max(st.iterations, 1), 4)}), flush=True)
        del pc


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    {"apply": apply_cases, "pcg": pcg_cases}[mode](N)
