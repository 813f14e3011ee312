#!/usr/bin/env python3
"""Several right-hand sides at once, measured: one JSON line per case on stdout (and appended to --out FILE).

  multi_rhs_only.py spmm  N [--op poisson|band]   kryst_spmm at K = 2, 4, 8 against K back-to-back kryst_spmv calls on the same operator
  multi_rhs_only.py solve N [--op poisson|band]   batched CG and Jacobi-PCG at K = 2, 4, 8 against K single solves, at fixed iteration counts
  multi_rhs_only.py trace N [--op poisson|band]   one batched CG solve (K = 8) and eight single ones, once each, no timing: what to run under
                                                  `rocprofv3 --kernel-trace --stats -- python3 tools/multi_rhs_only.py trace N` (a run of its own)

Everything runs in one process on plain CSR (KRYST_SPMV_COMPRESS=0 is set here, before the operator exists: the yardstick is the
single-vector path on the same arrays) and the two sides ALTERNATE, repetition by repetition; REPS repetitions after WARM warm-ups,
medians reported.  spmm: each repetition sits between two hipEvents on the compute stream (Context.timer_start / timer_stop).  solve:
wall clock around the whole call (it ends with the host reading the results), at IT and 3 IT iterations with tol = 0; the time of one
iteration is the difference of the two medians over 2 IT, which leaves out what a call costs besides its iterations.

Operators on an N^3 grid's worth of rows: `poisson`, the 7-point stencil; `band`, a non-stencil operator -- seven entries per row, the
diagonal 8 and six at offsets -3g, -2g, -g, +g, +2g, +3g (g = N^2 / 4) each jittered by a random 0 .. g - 1, values -U(0, 0.5): no two
rows share a pattern, so no compressed form applies.

Bytes (the kernel's own, what it must move once): SpMM 12 nnz + 4 (n + 1) + 16 n K; a batched CG iteration 12 nnz + 4 (n + 1) + 96 n K
(SpMM with the fused (p, Ap): P read twice, AP written; update: p, Ap, x, r read, x, r written; direction: r, p read, p written); Jacobi-PCG
12 nnz + 4 (n + 1) + 8 n + 112 n K.  frac_8TBps = bytes / time / 8e12."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["KRYST_SPMV_COMPRESS"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K

PEAK = 8.0e12
WIDTHS = (2, 4, 8)
WARM, REPS = 5, 50
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def band(N, ctx):
    n = N ** 3
    g = max(N * N // 4, 2)
    rng = np.random.default_rng(1234)
    base = np.array([-3 * g, -2 * g, -g, 0, g, 2 * g, 3 * g], dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    jit = rng.integers(0, g, size=(n, 7), dtype=np.int64)
    jit[:, 3] = 0
    cols = rows[:, None] + base[None, :] + jit
    vals = -0.5 * rng.random((n, 7))
    vals[:, 3] = 8.0
    valid = (cols >= 0) & (cols < n)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(valid.sum(axis=1), out=rp[1:])
    return K.CsrMatrix.from_csr_i32(n, n, rp, cols[valid].astype(np.int32), vals[valid], ctx=ctx)


def operator(name, N, ctx):
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx) if name == "poisson" else band(N, ctx)
    assert a.encoding()[0] == "csr", a.encoding()
    return a


def alternate(sides, reps=REPS, warm=WARM):
    """sides: name -> callable returning the milliseconds of one repetition; -> name -> (median, min)"""
    for _ in range(warm):
        for f in sides.values():
            f()
    got = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            got[k].append(f())
    return {k: (statistics.median(v), min(v)) for k, v in got.items()}


def spmm_cases(name, N):
    ctx = K.Context(0)
    a = operator(name, N, ctx)
    n, nnz = a.nrows(), a.nnz
    x1, y1 = ctx.vec(n).fill_splitmix(3), ctx.vec(n)
    for k in WIDTHS:
        xm, ym = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
        for j in range(k):
            xm.set_column(j, ctx.vec(n).fill_splitmix(3 + j))

        def many():
            ctx.timer_start()
            a.spmm(xm, ym)
            return ctx.timer_stop()

        def singles():
            ctx.timer_start()
            for _ in range(k):
                a.spmv(x1, y1)
            return ctx.timer_stop()

        r = alternate({"spmm": many, "spmv_x_k": singles})
        byts = 12 * nnz + 4 * (n + 1) + 16 * n * k
        bytes1 = 12 * nnz + 4 * (n + 1) + 16 * n
        emit({"case": "spmm", "op": name, "N": N, "n": n, "nnz": nnz, "K": k, "reps": REPS, "warmups": WARM,
              "spmm_ms": round(r["spmm"][0], 5), "spmm_ms_min": round(r["spmm"][1], 5),
              "k_spmv_ms": round(r["spmv_x_k"][0], 5), "k_spmv_ms_min": round(r["spmv_x_k"][1], 5),
              "ratio_k_spmv_over_spmm": round(r["spmv_x_k"][0] / r["spmm"][0], 3), "byte_ceiling_ratio": round(k * bytes1 / byts, 3),
              "spmm_bytes": byts, "spmm_frac_8TBps": round(byts / (r["spmm"][0] * 1e-3) / PEAK, 4),
              "spmv_frac_8TBps": round(k * bytes1 / (r["spmv_x_k"][0] * 1e-3) / PEAK, 4),
              "columns_per_s_spmm": round(k / (r["spmm"][0] * 1e-3), 1), "columns_per_s_spmv": round(k / (r["spmv_x_k"][0] * 1e-3), 1),
              "sources": K._ffi.source_sha16()})
        del xm, ym


def solve_cases(name, N, it):
    ctx = K.Context(0)
    a = operator(name, N, ctx)
    n, nnz = a.nrows(), a.nnz
    jac = K.Jacobi().setup(a)
    b1 = a.spmv(ctx.vec(n).fill(1.0))
    reps = REPS
    for method, cls, pc in (("cg", K.CgSolver, None), ("pcg_jacobi", K.PcgSolver, jac)):
        for k in WIDTHS:
            bm, xm = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
            for j in range(k):
                bm.set_column(j, b1 if j == 0 else ctx.vec(n).fill_splitmix(11 + j))
            zero = ctx.vec(n)
            xv = ctx.vec(n)
            med = {}
            for iters in (it, 3 * it):
                def many():
                    for j in range(k):
                        xm.set_column(j, zero)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    res = cls(0.0, iters).solve_many(a, pc, bm, xm)
                    ms = (time.perf_counter() - t0) * 1e3
                    assert all(not isinstance(r, K.KError) and r.iterations == iters for r in res), res
                    return ms

                def singles():
                    total = 0.0
                    for j in range(k):
                        xv.fill(0.0)
                        bj = bm.column(j)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        st = cls(0.0, iters).solve(a, pc, bj, xv)
                        total += (time.perf_counter() - t0) * 1e3
                        assert st.iterations == iters
                    return total

                med[iters] = alternate({"many": many, "singles": singles}, reps=reps)
            t_many = (med[3 * it]["many"][0] - med[it]["many"][0]) / (2 * it)             # ms per batched iteration (k columns)
            t_single = (med[3 * it]["singles"][0] - med[it]["singles"][0]) / (2 * it)     # ms per iteration of k single solves
            byts = 12 * nnz + 4 * (n + 1) + (96 * n * k if method == "cg" else 8 * n + 112 * n * k)
            emit({"case": "solve", "op": name, "N": N, "n": n, "nnz": nnz, "method": method, "K": k, "reps": reps, "warmups": WARM, "iterations": [it, 3 * it],
                  "many_ms": {str(i): round(med[i]["many"][0], 4) for i in med}, "k_singles_ms": {str(i): round(med[i]["singles"][0], 4) for i in med},
                  "ms_per_iteration_many": round(t_many, 5), "ms_per_iteration_k_singles": round(t_single, 5),
                  "column_iterations_per_s_many": round(k / (t_many * 1e-3), 1), "column_iterations_per_s_single": round(k / (t_single * 1e-3), 1),
                  "ratio_k_singles_over_many": round(t_single / t_many, 3), "iteration_bytes": byts,
                  "iteration_frac_8TBps": round(byts / (t_many * 1e-3) / PEAK, 4), "sources": K._ffi.source_sha16()})
            del bm, xm


def trace_case(name, N, it):
    ctx = K.Context(0)
    a = operator(name, N, ctx)
    n, k = a.nrows(), 8
    bm, xm = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
    for j in range(k):
        bm.set_column(j, ctx.vec(n).fill_splitmix(11 + j))
    for _ in range(2):                                     # the first solve also sizes the work arena
        for j in range(k):
            xm.set_column(j, ctx.vec(n))
        K.CgSolver(0.0, it).solve_many(a, None, bm, xm)
        for j in range(k):
            K.CgSolver(0.0, it).solve(a, None, bm.column(j), ctx.vec(n))
    ctx.synchronize()
    emit({"case": "trace", "op": name, "N": N, "K": k, "iterations": it, "solves_of_each_kind": 2})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("spmm", "solve", "trace"))
    ap.add_argument("N", type=int)
    ap.add_argument("--op", default="poisson", choices=("poisson", "band"))
    ap.add_argument("--it", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT = args.out
    if args.mode == "spmm":
        spmm_cases(args.op, args.N)
    elif args.mode == "solve":
        solve_cases(args.op, args.N, args.it)
    else:
        trace_case(args.op, args.N, args.it)
