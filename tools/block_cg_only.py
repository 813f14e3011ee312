#!/usr/bin/env python3
"""Block CG measured against the routes it competes with: one JSON line per case on stdout (and appended to --out FILE).

  block_cg_only.py N [--op poisson|varcoef] [--pc none|jacobi] [--k 2,4,8] [--reps R] [--cap ITERS] [--phase-iters P]

Time to tolerance 1e-8 for K right-hand sides uniform in [0, 1) (splitmix64, one seed per column), x0 = 0, by three routes on the operator's
default encoding (the 7-point operator streams CSR-P16, `varcoef` CSR-DIA), in ONE process with the routes ALTERNATING, repetition by repetition:

  block    BlockCgSolver.solve_block            one Krylov space for the K columns
  many     CgSolver / PcgSolver.solve_many      K recurrences that share the matrix read
  singles  CgSolver / PcgSolver.solve, K times  the fast single path

Wall clock around each call (a call ends with the host reading the results); medians over --reps repetitions after one warm-up pass of
--warm-iters iterations per route (which also sizes the work arena).  Without a preconditioner every route stops on ||r||_2 / ||r0||_2 <= tol;
with Jacobi block CG watches the M^-1 norm and the other two the 2-norm (solve_many has no Natural norm) -- the same test on the 7-point operator,
whose diagonal is constant, and one within sqrt(max d / min d) on `varcoef`.

Each new kernel's share: a block solve of --phase-iters iterations at tol = 0 runs under the library's phase timing (events between launches);
phase_ms_per_iteration holds spmv (the SpMM), blas1 (mgram_kernel), blas1_residual (bcg_update_kernel), blas1_direction (bcg_direction_kernel)
and reduce (the folds with the scalar steps), kernel_frac_8TBps each pass's own bytes over its time over 8e12.

Per-iteration figures: ms per block iteration = block_ms / iterations.  Bytes a block iteration must move once, per row, K columns wide
(8 K B per multivector pass; matrix bytes `mat` per row: 2 B on CSR-P16 read through the plain CSR arrays by the SpMM -- 88 B --, 56 + 4 B on CSR-DIA):
  spmm  16 K + mat      gram  16 K      update  48 K (+ 8 Jacobi)      direction  32 K (+ 8 Jacobi)      => 112 K + mat (+ 16)
block_frac_8TBps = those bytes / (ms per block iteration) / 8e12, folds and scalar steps included in the time.

  block_cg_only.py N --fuse-ab ITERS [...]     the A/B of KRYST_BCG_FUSE_GRAM (Gram(S, T) by mgram_kernel, or in the SpMM's epilogue) instead"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K

PEAK = 8.0e12
TOL = 1e-8
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def run(N, op, pcname, widths, reps, cap, warm_iters, phase_iters):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, op, ctx=ctx)
    n = a.nrows()
    pc = K.Jacobi().setup(a) if pcname == "jacobi" else None
    single_cls = K.PcgSolver if pc is not None else K.CgSolver
    norm = K.CgNormType.Unpreconditioned
    cols = [ctx.vec(n).fill_splitmix(0xB10C + j) for j in range(max(widths))]
    zero = ctx.vec(n)
    xv = ctx.vec(n)
    for k in widths:
        bm, xm = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
        for j in range(k):
            bm.set_column(j, cols[j])
        info = {}

        def reset():
            for j in range(k):
                xm.set_column(j, zero)
            ctx.synchronize()

        def block(tol=TOL, iters=cap):
            reset()
            t0 = time.perf_counter()
            res = K.BlockCgSolver(tol, iters).solve_block(a, pc, bm, xm)
            ms = (time.perf_counter() - t0) * 1e3
            assert all(not isinstance(r, K.KError) for r in res), res
            info["block"] = [r.iterations for r in res]
            info["block_hit_cap"] = any(r.iterations >= iters for r in res)
            return ms

        def many(tol=TOL, iters=cap):
            reset()
            t0 = time.perf_counter()
            res = single_cls(tol, iters).with_norm(norm).solve_many(a, pc, bm, xm)
            ms = (time.perf_counter() - t0) * 1e3
            assert all(not isinstance(r, K.KError) for r in res), res
            info["many"] = [r.iterations for r in res]
            return ms

        def singles(tol=TOL, iters=cap):
            total, its = 0.0, []
            for j in range(k):
                xv.fill(0.0)
                ctx.synchronize()
                t0 = time.perf_counter()
                st = single_cls(tol, iters).with_norm(norm).solve(a, pc, cols[j], xv)
                total += (time.perf_counter() - t0) * 1e3
                its.append(st.iterations)
            info["singles"] = its
            return total

        sides = {"block": block, "many": many, "singles": singles}
        for f in sides.values():
            f(0.0, warm_iters)
        got = {name: [] for name in sides}
        for _ in range(reps):
            for name, f in sides.items():
                got[name].append(f())
        med = {name: statistics.median(v) for name, v in got.items()}
        assert not info["block_hit_cap"] and max(info["many"] + info["singles"]) < cap, "a route ended at the cap: not a time to tolerance"
        its = info["block"][0]
        mat = 60 if a.encoding()[0] == "csr-dia" else 88
        jb = 8 if pc is not None else 0
        ctx.phase_timing_begin()
        block(0.0, phase_iters)
        ph = {name: ms / phase_iters for name, ms in ctx.phase_timing_end().items() if ms > 0.0}
        own = {"spmv": 16 * k + mat, "blas1": 16 * k, "blas1_residual": 48 * k + jb, "blas1_direction": 32 * k + jb}
        frac = {name: round(own[name] * n / (ph[name] * 1e-3) / PEAK, 4) for name in own if name in ph}
        row_bytes = 112 * k + mat + (16 if pc is not None else 0)
        ms_it = med["block"] / max(its, 1)
        emit({"case": "block_cg", "op": op, "N": N, "n": n, "encoding": a.encoding()[0], "pc": pcname, "K": k, "tol": TOL, "cap": cap, "reps": reps,
              "warm_iters": warm_iters,
              "block_iterations": its, "many_iterations": info["many"], "single_iterations": info["singles"],
              "block_ms": round(med["block"], 3), "many_ms": round(med["many"], 3), "k_singles_ms": round(med["singles"], 3),
              "all_ms": {name: [round(x, 3) for x in v] for name, v in got.items()},
              "singles_over_block": round(med["singles"] / med["block"], 3), "many_over_block": round(med["many"] / med["block"], 3),
              "iteration_ratio_max_single_over_block": round(max(info["singles"]) / max(its, 1), 3),
              "ms_per_block_iteration": round(ms_it, 5), "block_iteration_bytes": row_bytes * n,
              "block_frac_8TBps": round(row_bytes * n / (ms_it * 1e-3) / PEAK, 4),
              "phase_ms_per_iteration": {name: round(ms, 5) for name, ms in ph.items()}, "kernel_frac_8TBps": frac,
              "ms_per_single_iteration_all_columns": round(med["singles"] / max(sum(info["singles"]), 1) * k, 5),
              "sources": K._ffi.source_sha16()})
        del bm, xm


def fuse_ab(N, op, pcname, widths, reps, iters):
    """Gram(S, T) by mgram_kernel behind a plain SpMM (KRYST_BCG_FUSE_GRAM=0) against the SpMM's epilogue arm (=1): block solves of `iters`
    iterations at tol = 0, the two settings alternating in one process, medians of the wall clock"""
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, op, ctx=ctx)
    n = a.nrows()
    pc = K.Jacobi().setup(a) if pcname == "jacobi" else None
    zero = ctx.vec(n)
    for k in widths:
        bm, xm = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
        for j in range(k):
            bm.set_column(j, ctx.vec(n).fill_splitmix(0xB10C + j))

        def side(flag, its):
            def f():
                os.environ["KRYST_BCG_FUSE_GRAM"] = flag
                for j in range(k):
                    xm.set_column(j, zero)
                ctx.synchronize()
                t0 = time.perf_counter()
                res = K.BlockCgSolver(0.0, its).solve_block(a, pc, bm, xm)
                ms = (time.perf_counter() - t0) * 1e3
                assert all(not isinstance(r, K.KError) and r.iterations == its for r in res), res
                return ms
            return f

        med = {}
        for its in (iters, 3 * iters):                      # the time of an iteration: the difference of the two medians over 2 * iters
            sides = {"unfused": side("0", its), "fused": side("1", its)}
            for f in sides.values():
                f()
            got = {name: [] for name in sides}
            for _ in range(reps):
                for name, f in sides.items():
                    got[name].append(f())
            med[its] = {name: statistics.median(v) for name, v in got.items()}
        os.environ.pop("KRYST_BCG_FUSE_GRAM", None)
        per = {name: (med[3 * iters][name] - med[iters][name]) / (2 * iters) for name in ("unfused", "fused")}
        emit({"case": "fuse_ab", "op": op, "N": N, "n": n, "encoding": a.encoding()[0], "pc": pcname, "K": k, "reps": reps, "iterations": [iters, 3 * iters],
              "ms": {str(i): {name: round(v, 3) for name, v in med[i].items()} for i in med},
              "ms_per_iteration_unfused": round(per["unfused"], 5), "ms_per_iteration_fused": round(per["fused"], 5),
              "unfused_over_fused": round(per["unfused"] / per["fused"], 4), "sources": K._ffi.source_sha16()})
        del bm, xm


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int)
    ap.add_argument("--op", default="poisson", choices=("poisson", "varcoef"))
    ap.add_argument("--pc", default="none", choices=("none", "jacobi"))
    ap.add_argument("--k", default="2,4,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=20000)
    ap.add_argument("--warm-iters", type=int, default=5)
    ap.add_argument("--phase-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fuse-ab", type=int, default=0, metavar="ITERS", help="A/B of KRYST_BCG_FUSE_GRAM at ITERS and 3 ITERS iterations instead of the routes")
    args = ap.parse_args()
    OUT = args.out
    if args.fuse_ab > 0:
        fuse_ab(args.N, args.op, args.pc, [int(x) for x in args.k.split(",")], args.reps, args.fuse_ab)
        sys.exit(0)
    run(args.N, args.op, args.pc, [int(x) for x in args.k.split(",")], args.reps, args.cap, args.warm_iters, args.phase_iters)
