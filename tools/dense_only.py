"""Factor + solve time of the dense direct solvers (LuSolver, QrSolver) between two hipEvents on the compute
stream: warm-up runs, then the median of repeated runs, nothing else on the stream.  LU is timed with the in-LDS tail on (default) and
off (KRYST_DENSE_TAIL=0), the two alternating run by run.  One JSON line per (solver, n), beside the model it is read against: sum over the steps of 16 (n - s)^2 bytes
at 8 TB/s plus n kernel boundaries at 1.45 - 1.9 us.

    python tools/dense_only.py [--sizes 512,1024,2048,4096] [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K


def model_ms(n):
    stream = sum(16.0 * (n - s) ** 2 for s in range(n)) / 8.0e12 * 1e3
    return {"stream_ms": round(stream, 3), "boundaries_ms": [round(n * 1.45e-3, 3), round(n * 1.9e-3, 3)]}


def timed(ctx, call, warmup, reps):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_start()
        call()
        out.append(ctx.timer_stop())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = K.Context(0)
    lines = []
    for n in [int(v) for v in args.sizes.split(",")]:
        rng = np.random.default_rng(n)
        a = K.DenseMatrix.from_numpy(rng.standard_normal((n, n)), ctx=ctx)
        b, x = ctx.vec(rng.standard_normal(n)), ctx.vec(n)
        lu, qr = K.LuSolver(ctx), K.QrSolver()
        runs = {"lu": [], "lu_no_tail": []}
        for rep in range(-args.warmup, args.reps):                  # the A/B alternates inside one process
            for name, tail in (("lu", None), ("lu_no_tail", "0")):
                if tail is None:
                    os.environ.pop("KRYST_DENSE_TAIL", None)
                else:
                    os.environ["KRYST_DENSE_TAIL"] = tail
                ms = timed(ctx, lambda: lu.solve(a, None, b, x), 0, 1)
                if rep >= 0:
                    runs[name] += ms
        os.environ.pop("KRYST_DENSE_TAIL", None)
        lu.solve(a, None, b, x)
        runs["lu_solve_cached"] = timed(ctx, lambda: lu.solve_cached(b, x), args.warmup, args.reps)
        runs["qr"] = timed(ctx, lambda: qr.solve(a, None, b, x), args.warmup, max(3, args.reps // 2) if n >= 4096 else args.reps)
        for name, ms in runs.items():
            rec = {"solver": name, "n": n, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                   "max_ms": round(max(ms), 4), "runs": len(ms), "model": model_ms(n), "sources": K._ffi.source_sha16(("dense.hip", "dense.h"))}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
