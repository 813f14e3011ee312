#!/usr/bin/env python3
"""Additive Schwarz measurements: one JSON line per case on stdout.

  asm_only.py apply N     N^3 Poisson, 4x4x2 boxes: as written (overlap 0), grown and RAS with overlap 1: set-up ms (first call and
                          repeat), apply ms (kryst_bench_pc_apply, 20 back-to-back applies), the bytes model and its fraction of 8 TB/s
  asm_only.py pcg N       PCG to 1e-8 on the N^3 Poisson operator: ASM as written and grown (overlap 1) on the 4x4x2 boxes against block
                          Jacobi on the same boxes, Jacobi and ILU(0): iterations, set-up ms, solve ms

Bytes per apply: 8 sum b_k^2 (tiles) + 4 sum b_k (indices) + 8 sum b_k (r gathered) + 16 sum b_k (X written and read) + 4 sum b_k (map)
+ 8 n (z); RAS reads 4 n map entries instead of 4 sum b_k."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K
from kryst_amd import _ffi

PEAK = 8.0e12
CASES = (("as_written", 0), ("grown", 1), ("restricted", 1))


def timed(fn, ctx):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def make(variant, overlap, boxes):
    p = K.AdditiveSchwarz(overlap, boxes)
    return p.with_overlap() if variant == "grown" else p.restricted() if variant == "restricted" else p


def sizes(pc):
    ptr = np.zeros(pc.info()["nsub"] + 1, dtype=np.int64)
    K.check(K.lib().kryst_pc_asm_export(pc.h, ptr.ctypes.data_as(_ffi.c_i64p), None, None, None))
    b = np.diff(ptr)
    return int(b.sum()), int((b * b).sum()), int(b.max())


def apply_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    boxes = K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))
    r = ctx.vec(n).fill_splitmix(3)
    z = ctx.vec(n)
    for variant, overlap in CASES:
        pc, setup_ms = timed(lambda: make(variant, overlap, boxes).setup(a), ctx)
        del pc
        pc, setup2_ms = timed(lambda: make(variant, overlap, boxes).setup(a), ctx)
        ms = pc.bench_apply(r, z, reps=20)
        sb, sb2, bmax = sizes(pc)
        byts = 8 * sb2 + 4 * sb + 8 * sb + 16 * sb + (4 * n if variant == "restricted" else 4 * sb) + 8 * n
        print(json.dumps({"case": "apply", "N": N, "variant": variant, "overlap": overlap, "nsub": len(boxes[0]) - 1, "sum_b": sb,
                          "max_b": bmax, "setup_ms": round(setup_ms, 2), "setup_ms_repeat": round(setup2_ms, 2), "apply_ms": round(ms, 4),
                          "bytes": byts, "TBps": round(byts / ms / 1e9, 3), "frac_8TBps": round(byts / (ms * 1e-3) / PEAK, 3)}), flush=True)
        del pc


def pcg_cases(N):
    ctx = K.Context(0)
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    n = a.nrows()
    boxes = K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))
    bv = a.spmv(ctx.vec(n).fill(1.0))
    pcs = (("asm_as_written", lambda: make("as_written", 0, boxes).setup(a)), ("asm_overlap1", lambda: make("grown", 1, boxes).setup(a)),
           ("block_jacobi_boxes", lambda: K.BlockJacobi(boxes).setup(a)), ("jacobi", lambda: K.Jacobi().setup(a)),
           ("ilu0", lambda: K.TrueIlu0().setup(a)))
    for name, mk in pcs:
        pc, setup_ms = timed(mk, ctx)
        for rep in range(2):                                   # the first solve also sizes the solver's work arena
            xv = ctx.vec(n).fill(0.0)
            s = K.PcgSolver(1e-8, 20000)
            st, ms = timed(lambda: s.solve(a, pc, bv, xv), ctx)
        print(json.dumps({"case": "pcg_poisson", "N": N, "pc": name, "iterations": st.iterations, "converged": st.converged,
                          "final_residual": st.final_residual, "setup_ms": round(setup_ms, 2), "solve_ms": round(ms, 2),
                          "total_ms": round(setup_ms + ms, 2), "ms_per_iteration": round(ms / max(st.iterations, 1), 4)}), flush=True)
        del pc


if __name__ == "__main__":
    mode, N = sys.argv[1], int(sys.argv[2])
    {"apply": apply_cases, "pcg": pcg_cases}[mode](N)
