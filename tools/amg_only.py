"""AMG measurements on one GPU: set-up time, levels and operator complexity of smoothed aggregation (Amg().with_textbook()), the
V-cycle's milliseconds, and PCG+SA against CG and Jacobi-PCG on the same Poisson operator (b = ones, rtol 1e-8; the operator's default
storage form).  One JSON line per measurement.  `python tools/amg_only.py --sizes 256 512 [--solve]`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K  # noqa: E402


def timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = f()
    ctx.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ctx = K.Context(0)
    for N in args.sizes:
        a = K.CsrMatrix.stencil7(N, ctx=ctx)
        setups = []
        for _ in range(3):
            pc, t = timed(ctx, lambda: K.Amg(25).with_textbook().setup(a))
            setups.append(t)
        info = pc.info()
        r = ctx.vec(a.nrows()).fill(1.0)
        z = ctx.vec(a.nrows())
        ms = pc.bench_apply(r, z, reps=args.reps)
        print(json.dumps({"what": "sa_setup", "N": N, "setup_s": setups, "levels": info["rows"], "nnz": info["nnz"],
                          "operator_complexity": info["operator_complexity"], "vcycle_ms": ms, "encoding": a.encoding()}), flush=True)
        if not args.solve:
            continue
        b = np.ones(a.nrows())
        for name, mk in (("pcg_sa", lambda: K.Amg(25).with_textbook().setup(a)), ("cg", None), ("pcg_jacobi", lambda: K.Jacobi().setup(a))):
            x = np.zeros(a.nrows())
            def run():
                p = mk() if mk else None
                s = K.PcgSolver(1e-8, 5000) if p is not None else K.CgSolver(1e-8, 5000)
                return s.solve(a, p, b, x)
            st, t = timed(ctx, run)
            print(json.dumps({"what": name, "N": N, "iterations": st.iterations, "converged": st.converged, "seconds_incl_setup": t,
                              "encoding": a.encoding()}), flush=True)


if __name__ == "__main__":
    main()
