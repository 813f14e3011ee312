#!/usr/bin/env python3
"""Several right-hand sides on the diagonal (CSR-DIA) encoding, measured: one JSON line per case on stdout (and
appended to --out FILE).  The operator is the variable-coefficient 7-point stencil on an N^3 grid, created under the defaults, so that its own
SpMV streams CSR-DIA.

  multi_rhs_dia.py spmm  N    kryst_spmm at K = 2, 4, 8 through spmm_dia_kernel (KRYST_SPMM_FORM=dia) against both yardsticks: K back-to-back
                              kryst_spmv calls on CSR-DIA (what a user gets without solve_many) and spmm_rows_kernel (KRYST_SPMM_FORM=plain)
  multi_rhs_dia.py knobs N    the diagonal kernel alone, A/B: KRYST_SPMM_BLOCKS_PER_CU = 1 / 2 / 4 / 8 and KRYST_SPMM_DIA_NT = 1 / 0
  multi_rhs_dia.py solve N    batched CG and Jacobi-PCG at K = 2, 4, 8 under dia and under plain against K single solves, at fixed iteration counts

Method (section 4.14's): one process; the sides ALTERNATE window by window after a warm-up; a window is at least --window seconds of work
(spmm: repetitions between two hipEvents on the compute stream, the operand rotating over three copies so that it never sits in the Infinity
Cache; solve: wall clock around whole calls that end with the host reading the results); the median over the windows is reported, and beside
it the SPREAD of each side, (max - min) / median over its windows.  A ratio counts as a win or a loss only beyond the spreads of its two
sides, which `verdict` applies; inside them it is "level".  solve: every side runs at IT and at 3 IT iterations with tol = 0, and the time
of one iteration is the difference of the two medians over 2 IT, which leaves out what a call costs besides its iterations.

Bytes (the kernel's own, what it must move once), D = 7: the diagonal SpMM (8 D + 16 K) n; spmm_rows_kernel 12 nnz + 4 (n + 1) + 16 n K;
kryst_spmv on CSR-DIA (8 D + 16) n.  frac_8TBps = bytes / time / 8e12."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K

PEAK = 8.0e12
WIDTHS = (2, 4, 8)
D = 7
OUT = None
WINDOW = 0.5
WINDOWS = 5


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def operator(N, ctx):
    a = K.CsrMatrix.stencil7(N, "varcoef", ctx=ctx)
    assert a.encoding()[0] == "csr-dia", a.encoding()
    return a


class Env:
    """the settings of one side, in force while it runs"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def alternate(sides, windows=WINDOWS, warm=1):
    """sides: name -> callable returning the milliseconds per unit of work of one window; -> name -> {median, min, max, spread}"""
    for _ in range(warm):
        for f in sides.values():
            f()
    got = {k: [] for k in sides}
    for _ in range(windows):
        for k, f in sides.items():
            got[k].append(f())
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in got.items()}


def verdict(ratio, spread_a, spread_b):
    """ratio = yardstick time / time of the side under test"""
    band = spread_a + spread_b
    return "win" if ratio > 1.0 + band else "loss" if ratio < 1.0 - band else "level"


def summary(r):
    return {k: round(v, 5) for k, v in r.items()}


def spmm_window(ctx, launch, reps):
    """-> a callable: `reps` launches between two events, milliseconds per launch"""
    def f():
        ctx.timer_start()
        for i in range(reps):
            launch(i)
        return ctx.timer_stop() / reps
    return f


def calibrate(ctx, launch):
    """repetitions that fill a window"""
    for i in range(3):
        launch(i)
    ctx.timer_start()
    for i in range(5):
        launch(i)
    per = ctx.timer_stop() / 5
    return max(5, int(math.ceil(WINDOW * 1e3 / per)))


def operands(ctx, n, k):
    xs = [K.MultiVec(ctx, n, k) for _ in range(3)]
    for c, xm in enumerate(xs):
        for j in range(k):
            xm.set_column(j, ctx.vec(n).fill_splitmix(3 + j + 17 * c))
    return xs, K.MultiVec(ctx, n, k)


def spmm_cases(N):
    ctx = K.Context(0)
    a = operator(N, ctx)
    n, nnz = a.nrows(), a.nnz
    x1 = [ctx.vec(n).fill_splitmix(3 + 17 * c) for c in range(3)]
    y1 = ctx.vec(n)
    for k in WIDTHS:
        xs, ym = operands(ctx, n, k)

        def side(form):
            def launch(i):
                a.spmm(xs[i % 3], ym)

            def f():
                with Env(KRYST_SPMM_FORM=form):
                    assert a.spmm_kernel(k) == form
                    return spmm_window(ctx, launch, reps[form])()
            return launch, f

        def singles_launch(i):
            for j in range(k):
                a.spmv(x1[(i + j) % 3], y1)

        reps = {}
        sides = {}
        for form in ("dia", "plain"):
            launch, f = side(form)
            with Env(KRYST_SPMM_FORM=form):
                reps[form] = calibrate(ctx, launch)
            sides[form] = f
        reps["singles"] = calibrate(ctx, singles_launch)
        sides["singles"] = spmm_window(ctx, singles_launch, reps["singles"])
        r = alternate(sides)
        t = {s: r[s]["median"] for s in r}
        bytes_dia, bytes_plain, bytes_single = (8 * D + 16 * k) * n, 12 * nnz + 4 * (n + 1) + 16 * n * k, k * (8 * D + 16) * n
        ratio_s, ratio_p = t["singles"] / t["dia"], t["plain"] / t["dia"]
        emit({"case": "spmm", "op": "varcoef", "N": N, "n": n, "nnz": nnz, "K": k, "windows": WINDOWS, "window_s": WINDOW, "reps_per_window": reps,
              "dia_ms": summary(r["dia"]), "plain_ms": summary(r["plain"]), "k_spmv_ms": summary(r["singles"]),
              "ratio_k_spmv_over_dia": round(ratio_s, 3), "verdict_against_k_spmv": verdict(ratio_s, r["singles"]["spread"], r["dia"]["spread"]),
              "ratio_plain_over_dia": round(ratio_p, 3), "verdict_against_plain": verdict(ratio_p, r["plain"]["spread"], r["dia"]["spread"]),
              "byte_ceiling_ratio": round(bytes_single / bytes_dia, 3),
              "dia_frac_8TBps": round(bytes_dia / (t["dia"] * 1e-3) / PEAK, 4), "plain_frac_8TBps": round(bytes_plain / (t["plain"] * 1e-3) / PEAK, 4),
              "spmv_frac_8TBps": round(bytes_single / (t["singles"] * 1e-3) / PEAK, 4), "sources": K._ffi.source_sha16()})
        del xs, ym


def knob_cases(N):
    ctx = K.Context(0)
    a = operator(N, ctx)
    n = a.nrows()
    settings = {"bpc2": {"KRYST_SPMM_BLOCKS_PER_CU": "2"}, "bpc1": {"KRYST_SPMM_BLOCKS_PER_CU": "1"}, "bpc4": {"KRYST_SPMM_BLOCKS_PER_CU": "4"},
                "bpc8": {"KRYST_SPMM_BLOCKS_PER_CU": "8"}, "plain_loads": {"KRYST_SPMM_BLOCKS_PER_CU": "2", "KRYST_SPMM_DIA_NT": "0"}}
    for k in WIDTHS:
        xs, ym = operands(ctx, n, k)

        def launch(i):
            a.spmm(xs[i % 3], ym)

        with Env(KRYST_SPMM_FORM="dia"):
            assert a.spmm_kernel(k) == "dia"
            reps = calibrate(ctx, launch)
            sides = {}
            for name, kv in settings.items():
                def f(kv=kv):
                    with Env(**kv):
                        return spmm_window(ctx, launch, reps)()
                sides[name] = f
            r = alternate(sides)
        base = r["bpc2"]                                    # the shipped setting: 2 workgroups per compute unit, nontemporal value loads
        emit({"case": "knobs", "op": "varcoef", "N": N, "n": n, "K": k, "windows": WINDOWS, "window_s": WINDOW, "reps_per_window": reps,
              **{f"{name}_ms": summary(r[name]) for name in r},
              **{f"ratio_bpc2_over_{name}": round(base["median"] / r[name]["median"], 3) for name in r if name != "bpc2"},
              **{f"verdict_{name}": verdict(base["median"] / r[name]["median"], base["spread"], r[name]["spread"]) for name in r if name != "bpc2"},
              "sources": K._ffi.source_sha16()})
        del xs, ym


def solve_cases(N, windows):
    ctx = K.Context(0)
    a = operator(N, ctx)
    n, nnz = a.nrows(), a.nnz
    jac = K.Jacobi().setup(a)
    b1 = a.spmv(ctx.vec(n).fill(1.0))
    for method, cls, pc in (("cg", K.CgSolver, None), ("pcg_jacobi", K.PcgSolver, jac)):
        for k in WIDTHS:
            bm, xm = K.MultiVec(ctx, n, k), K.MultiVec(ctx, n, k)
            for j in range(k):
                bm.set_column(j, b1 if j == 0 else ctx.vec(n).fill_splitmix(11 + j))
            bcols = [bm.column(j) for j in range(k)]
            zero, xv = ctx.vec(n), ctx.vec(n)

            def many(form, iters):
                def f():
                    for j in range(k):
                        xm.set_column(j, zero)
                    with Env(KRYST_SPMM_FORM=form):
                        assert a.spmm_kernel(k) == form
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        res = cls(0.0, iters).solve_many(a, pc, bm, xm)
                        ms = (time.perf_counter() - t0) * 1e3
                    assert all(not isinstance(r, K.KError) and r.iterations == iters for r in res), res
                    return ms
                return f

            def singles(iters):
                def f():
                    total = 0.0
                    for j in range(k):
                        xv.fill(0.0)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        st = cls(0.0, iters).solve(a, pc, bcols[j], xv)
                        total += (time.perf_counter() - t0) * 1e3
                        assert st.iterations == iters
                    return total
                return f

            # iterations that fill a window on the fastest side: from one call of 10 (after one that sizes the work arena)
            many("dia", 10)()
            it = max(10, int(math.ceil(WINDOW * 1e3 / (many("dia", 10)() / 10.0))))
            med = {}
            for iters in (it, 3 * it):
                med[iters] = alternate({"dia": many("dia", iters), "plain": many("plain", iters), "singles": singles(iters)}, windows=windows)
            per = {s: (med[3 * it][s]["median"] - med[it][s]["median"]) / (2 * it) for s in ("dia", "plain", "singles")}      # ms per iteration of k columns
            spread = {s: max(med[it][s]["spread"], med[3 * it][s]["spread"]) for s in per}
            ratio_s, ratio_p = per["singles"] / per["dia"], per["plain"] / per["dia"]
            emit({"case": "solve", "op": "varcoef", "N": N, "n": n, "nnz": nnz, "method": method, "K": k, "windows": windows, "iterations": [it, 3 * it],
                  "call_ms": {s: {str(i): summary(med[i][s]) for i in med} for s in per},
                  "ms_per_iteration": {s: round(per[s], 5) for s in per}, "spread": {s: round(spread[s], 4) for s in per},
                  "column_iterations_per_s": {s: round(k / (per[s] * 1e-3), 1) for s in per},
                  "ratio_k_singles_over_dia": round(ratio_s, 3), "verdict_against_k_singles": verdict(ratio_s, spread["singles"], spread["dia"]),
                  "ratio_plain_over_dia": round(ratio_p, 3), "verdict_against_plain": verdict(ratio_p, spread["plain"], spread["dia"]),
                  "sources": K._ffi.source_sha16()})
            del bm, xm, bcols


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("spmm", "knobs", "solve"))
    ap.add_argument("N", type=int)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per window (at least 0.5 for a figure that is reported)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT, WINDOW, WINDOWS = args.out, args.window, args.windows
    if args.mode == "spmm":
        spmm_cases(args.N)
    elif args.mode == "knobs":
        knob_cases(args.N)
    else:
        solve_cases(args.N, args.windows)
