"""PCA-GMRES measurements on one GPU.  One JSON line per measurement.
  --mode rate:    GMRES(30) + Jacobi on 7-point Poisson, b = A*ones, exactly 60 iterations per timed solve (tol = 0, as bench.py's
                  gmres30_jacobi): GmresSolver Right and LeftTextbook, and the s-step extension for each --s
  --mode config3: convection-diffusion 256^3, restart 30, Jacobi, to a true relative residual of 1e-8 (s-step, Right) against
                  GmresSolver LeftTextbook
`python tools/pca_gmres_only.py --mode rate --sizes 256 512 --s 1 2 4 5 6 8`"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K  # noqa: E402


def timed_solve(ctx, make, a, pc, b, reps):
    out = []
    for _ in range(reps):
        x = ctx.vec(a.nrows())
        s = make()
        ctx.synchronize()
        t0 = time.perf_counter()
        st = s.solve(a, pc, b, x)
        ctx.synchronize()
        out.append((time.perf_counter() - t0, st, x))
    return out


def forms(svals, restart, tol, max_iters):
    P = K.Preconditioning
    f = [("gmres_right", lambda: K.GmresSolver(restart, tol, max_iters).with_preconditioning(P.Right)),
         ("gmres_left_textbook", lambda: K.GmresSolver(restart, tol, max_iters).with_preconditioning(P.LeftTextbook))]
    for s in svals:
        f.append((f"sstep_s{s}", (lambda s=s: K.PcaGmresSolver(restart, 1, s, tol, max_iters).with_preconditioning(P.Right).with_textbook())))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["rate", "config3"], default="rate")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--s", type=int, nargs="+", default=[1, 2, 4, 5, 6, 8])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = K.Context(0)
    if args.mode == "rate":
        for N in args.sizes:
            a = K.CsrMatrix.stencil7(N, ctx=ctx)
            b = a.spmv(ctx.vec(a.nrows()).fill(1.0))
            pc = K.Jacobi().setup(a)
            for name, make in forms(args.s, 30, 0.0, 60):
                runs = timed_solve(ctx, make, a, pc, b, args.reps + 1)[1:]        # the first solve warms up
                ts = sorted(t for t, _, _ in runs)
                st = runs[0][1]
                print(json.dumps({"workload": f"gmres30_jacobi_poisson7_{N}^3", "form": name, "iterations": st.iterations,
                                  "iterations_per_s": st.iterations / ts[len(ts) // 2], "solve_seconds": ts, "final_residual": st.final_residual}),
                      flush=True)
    else:
        for N in args.sizes:
            a = K.CsrMatrix.stencil7(N, "convdiff", ctx=ctx)
            b = a.spmv(ctx.vec(a.nrows()).fill(1.0))
            bn = K.norm(b)
            pc = K.Jacobi().setup(a)
            for name, make in forms(args.s, 30, 1e-8, 3000)[1:]:
                (t, st, x), = timed_solve(ctx, make, a, pc, b, 1)
                ax = a.spmv(x)
                res = float(np.linalg.norm(b.to_host() - ax.to_host()) / bn)
                print(json.dumps({"workload": f"config3_gmres30_jacobi_convdiff7_{N}^3", "form": name, "iterations": st.iterations,
                                  "converged": bool(st.converged), "true_relative_residual": res, "solve_seconds": t,
                                  "iterations_per_s": st.iterations / t}), flush=True)


if __name__ == "__main__":
    main()
