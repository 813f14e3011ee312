#!/usr/bin/env python3
"""Additive Schwarz with ILU(0) subdomain solves, measured: one JSON line per case on stdout.

  asm_ilu_only.py apply N   N^3 Poisson; boxes of 8^3, 16^3 and 24^3 points, as written and RAS with one layer: set-up ms (first call and
                            repeat), apply ms (median of seven timings after two warm-ups, each between hipEvents: kryst_bench_pc_apply),
                            sizes, levels, the bytes model and its fraction of 8 TB/s.  Beside them, in the same process: the global
                            ILU(0) apply, the dense-tile additive Schwarz apply on 4x4x2 boxes, and two SpMVs.
  asm_ilu_only.py solve N   N^3 Poisson to 1e-8: PCG (as written) and left GMRES(30) (RAS, one layer) on 16^3 boxes against global
                            ILU(0), block Jacobi on 4x4x2 boxes and Jacobi: iterations, set-up ms, solve ms.

Bytes per apply: 10 per entry of the padded level layouts (8 value + 2 column), per subdomain row 4 (index) + 8 (r gathered) + 8 (order,
two sweeps) + 8 (diagonal) + 16 (X written and read), 4 per map entry, 8 n (z); the level tables are 16 bytes per level and subdomain."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K

PEAK = 8.0e12
BOXES = (8, 16, 24)
VARIANTS = (("as_written", 0), ("restricted", 1))


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def median_ms(fn):
    for _ in range(2):
        fn()
    return statistics.median(fn() for _ in range(7))


def make(variant, overlap, boxes, mode="ilu0"):
    p = K.AdditiveSchwarz(overlap, boxes)
    p = p.restricted() if variant == "restricted" else p.with_overlap() if variant == "grown" else p
    return p.with_sub_ilu(mode) if mode else p


def apply_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    r = ctx.vec(n).fill_splitmix(3)
    z = ctx.vec(n)
    for box in BOXES:
        sets = K.AdditiveSchwarz.grid_boxes(N, (box, box, box))
        for variant, overlap in VARIANTS:
            try:
                pc, setup_ms = timed(lambda: make(variant, overlap, sets).setup(a), ctx)
            except K.KError as e:                                           # 24^3 boxes with one layer: 17 280 rows, over the cap
                print(json.dumps({"case": "apply", "N": N, "box": box, "variant": variant, "overlap": overlap, "error": str(e)}), flush=True)
                continue
            del pc
            pc, setup2_ms = timed(lambda: make(variant, overlap, sets).setup(a), ctx)
            ms = median_ms(lambda: pc.bench_apply(r, z, reps=3))
            inf = pc.info()
            m = n if variant == "restricted" else inf["ext_rows"]
            byts = 10 * inf["layout_entries"] + (4 + 8 + 8 + 8 + 16) * inf["ext_rows"] + 4 * m + 8 * n
            print(json.dumps({"case": "apply", "N": N, "box": box, "variant": variant, "overlap": overlap, **inf,
                              "setup_ms": round(setup_ms, 2), "setup_ms_repeat": round(setup2_ms, 2), "apply_ms": round(ms, 4), "bytes": byts,
                              "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 4),
                              "us_per_level": round(1e3 * ms / max(2 * inf["max_levels"], 1), 3)}), flush=True)
            del pc
    ilu, ms_setup = timed(lambda: K.TrueIlu0().setup(a), ctx)
    print(json.dumps({"case": "global_ilu0_apply", "N": N, "setup_ms": round(ms_setup, 2),
                      "apply_ms": round(median_ms(lambda: ilu.bench_apply(r, z, reps=3)), 4), "form": ilu.ilu_info()["form"]}), flush=True)
    del ilu
    dense, ms_setup = timed(lambda: K.AdditiveSchwarz(0, K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))).setup(a), ctx)
    print(json.dumps({"case": "dense_tile_asm_apply", "N": N, "box": "4x4x2", "setup_ms": round(ms_setup, 2),
                      "apply_ms": round(median_ms(lambda: dense.bench_apply(r, z, reps=3)), 4)}), flush=True)
    del dense

    def two_spmv():
        ctx.timer_start()
        a.spmv(r, z)
        a.spmv(r, z)
        return ctx.timer_stop()
    print(json.dumps({"case": "two_spmv", "N": N, "ms": round(median_ms(two_spmv), 4)}), flush=True)


def solve_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    sets = K.AdditiveSchwarz.grid_boxes(N, (16, 16, 16))
    small = K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))
    bv = a.spmv(ctx.vec(n).fill(1.0))
    pcs = (("sub_ilu0_as_written", lambda: make("as_written", 0, sets).setup(a)), ("sub_ilu0_ras1", lambda: make("restricted", 1, sets).setup(a)),
           ("global_ilu0", lambda: K.TrueIlu0().setup(a)), ("block_jacobi_4x4x2", lambda: K.BlockJacobi(small).setup(a)),
           ("jacobi", lambda: K.Jacobi().setup(a)))
    for solver in ("pcg", "gmres30_left"):
        for name, mk in pcs:
            if name == ("sub_ilu0_ras1" if solver == "pcg" else "sub_ilu0_as_written"):   # RAS is not symmetric: GMRES only; as written: PCG only
                continue
            pc, setup_ms = timed(mk, ctx)
            for rep in range(2):                                            # the first solve also sizes the solver's work arena
                xv = ctx.vec(n).fill(0.0)
                s = K.PcgSolver(1e-8, 20000) if solver == "pcg" else K.GmresSolver(30, 1e-8, 20000).with_preconditioning(K.Preconditioning.Left)
                try:
                    st, ms = timed(lambda: s.solve(a, pc, bv, xv), ctx)
                except K.KError as e:
                    st, ms = e.stats, float("nan")
            print(json.dumps({"case": "solve_poisson", "N": N, "solver": solver, "pc": name, "iterations": st.iterations, "converged": bool(st.converged),
                              "final_residual": st.final_residual, "setup_ms": round(setup_ms, 2), "solve_ms": round(ms, 2),
                              "ms_per_iteration": round(ms / max(st.iterations, 1), 4)}), flush=True)
            del pc


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    {"apply": apply_cases, "solve": solve_cases}[mode](N)
