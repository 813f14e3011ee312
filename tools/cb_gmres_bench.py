#!/usr/bin/env python3
"""Compressed-basis GMRES against GmresSolver, all in one process, alternating (results: profiles/cb_gmres/).

  --mode rate    GmresSolver side None, CbGmresSolver f64 (the control) and CbGmresSolver f32 in turn, tol = 0 so that every solve does
                 exactly --iters iterations; without a preconditioner and with Jacobi (Right; there GmresSolver's as-written Right arm
                 runs beside them for orientation -- it keeps Z and is another algorithm).  One warm-up round, then --batches rounds;
                 one JSON line per (grid, operator, pc) with the median iterations/s, the batch spread and the ratios.
  --mode count   iterations of f32 against f64 to --tol (default 1e-10), one JSON line per (grid, operator, pc).
  --mode links   reads the kernel totals of a separate `rocprofv3 --kernel-trace --stats -- python tools/cb_gmres_bench.py --mode rate
                 --sizes N --batches 1` run (--stats FILE, the *_kernel_stats.csv) and prints, per link kernel, calls, total time and the
                 achieved TB/s on the model bytes of a link: 32 B per row with an fp64 basis (z read and written, B_i, B_next), 24 B with fp32.

usage: cb_gmres_bench.py --mode rate --sizes 256 512 [--restart 30] [--iters 60] [--batches 3] [--kinds convdiff poisson]"""
import argparse, csv, json, os, re, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def links_per_solve(restart, iters):
    """2 (j + 1) links in step j of a cycle"""
    full, rest = divmod(iters, restart)
    return full * restart * (restart + 1) + rest * (rest + 1)


def solvers(K, restart, tol, iters, pc):
    P = K.Preconditioning
    side = P.Right if pc else P.NoPc
    out = {"gmres": lambda: K.GmresSolver(restart, tol, iters).with_preconditioning(side),
           "cb_f64": lambda: K.CbGmresSolver(restart, tol, iters).with_basis("f64").with_preconditioning(side),
           "cb_f32": lambda: K.CbGmresSolver(restart, tol, iters).with_basis("f32").with_preconditioning(side)}
    return out


def timed(ctx, make, a, pc, b, n):
    s = make()
    x = ctx.vec(n)
    ctx.synchronize(); t0 = time.perf_counter()
    st = s.solve(a, pc, b, x)
    ctx.synchronize(); dt = time.perf_counter() - t0
    return st, s, dt


def run(args):
    import kryst_amd as K
    ctx = K.Context(0)
    for N in args.sizes:
        for kind in args.kinds:
            a = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
            n = a.nrows()
            b = a.spmv(ctx.vec(n).fill(1.0))
            for pcname in args.pcs:
                pc = K.Jacobi().setup(a) if pcname == "jacobi" else None
                if args.mode == "count":
                    rec = {"mode": "count", "grid": N, "operator": kind, "pc": pcname, "restart": args.restart, "tol": args.tol}
                    for name in ("cb_f64", "cb_f32"):
                        st, s, dt = timed(ctx, solvers(K, args.restart, args.tol, args.max_iters, pc)[name], a, pc, b, n)
                        rec[name] = {"iterations": st.iterations, "converged": bool(st.converged), "final_residual": st.final_residual, "seconds": dt}
                    print(json.dumps(rec), flush=True)
                    continue
                f = solvers(K, args.restart, 0.0, args.iters, pc)
                rates = {k: [] for k in f}
                for batch in range(args.batches + 1):                   # round 0 warms up (allocations, first launches)
                    for name, make in f.items():
                        st, s, dt = timed(ctx, make, a, pc, b, n)
                        assert st.iterations == args.iters, (name, st.iterations)
                        if batch:
                            rates[name].append(st.iterations / dt)
                med = {k: statistics.median(v) for k, v in rates.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in rates.items()}
                rec = {"mode": "rate", "grid": N, "operator": kind, "pc": pcname, "restart": args.restart, "iterations": args.iters,
                       "links_per_solve": links_per_solve(args.restart, args.iters), "batches": args.batches,
                       "iterations_per_sec": {k: round(v, 2) for k, v in med.items()},
                       "batch_rates": {k: [round(r, 2) for r in v] for k, v in rates.items()},
                       "spread": {k: round(v, 4) for k, v in spread.items()},
                       "f32_over_f64": round(med["cb_f32"] / med["cb_f64"], 4), "f32_over_gmres": round(med["cb_f32"] / med["gmres"], 4),
                       "f64_over_gmres": round(med["cb_f64"] / med["gmres"], 4)}
                print(json.dumps(rec), flush=True)
            del a


def links(args):
    """kernel totals -> TB/s of the link kernels on their model bytes"""
    n = args.sizes[0] ** 3
    rows = list(csv.DictReader(open(args.stats)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        m = re.search(r"(CbLinkOp<(?:true|false), (?:float|double)>|MgsLinkOp<(?:true|false)>)", name)
        if not m:
            continue
        calls = int(r.get("Calls") or r.get("Count"))
        total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or r.get("Total"))
        per_row = 24 if "float" in m.group(1) else 32
        print(json.dumps({"mode": "links", "grid": args.sizes[0], "kernel": m.group(1), "calls": calls, "total_ms": round(total_ns / 1e6, 3),
                          "us_per_link": round(total_ns / 1e3 / calls, 2), "model_bytes_per_row": per_row,
                          "tb_per_s": round(calls * n * per_row / total_ns / 1e3, 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["rate", "count", "links"], default="rate")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256])
    ap.add_argument("--kinds", nargs="+", default=["convdiff", "poisson"])
    ap.add_argument("--pcs", nargs="+", default=["none", "jacobi"])
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iters", type=int, default=6000)
    ap.add_argument("--stats")
    args = ap.parse_args()
    links(args) if args.mode == "links" else run(args)
