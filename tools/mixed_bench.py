#!/usr/bin/env python3
"""Mixed precision, measured: one JSON line per case on stdout (and appended to --out FILE).  One GPU, one process.

  mixed_bench.py spmv   N [--op poisson|varcoef|band]   kryst_spmv32 against the plain-CSR fp64 kryst_spmv, each as a fraction of 8 TB/s on its own bytes
  mixed_bench.py rate   N [--op ...]                    CG32 / PCG32 iterations per second against fp64 CG / Jacobi-PCG on plain CSR and on the
                                                        operator's default encoding, at the same capped iteration counts
  mixed_bench.py refine N [--op ...] [--reps R]         time to tolerance: RefinementSolver (outer 1e-10, inner 1e-6) against fp64 CG / Jacobi-PCG to
                                                        1e-10 on plain CSR and on the default encoding: outer steps, total inner iterations, ms
  mixed_bench.py pspmv  N                               the row-pattern lowering (CsrMatrix.lower("pattern")): kryst_spmv32 per kernel -- plain, pattern,
                                                        pattern-stage with runs of 1 and of 2 tiles -- against the fp64 kryst_spmv on the default encoding
  mixed_bench.py prate  N                               CG32 / PCG32 it/s on the pattern-lowered and on the plain-lowered operator against fp64 CG /
                                                        Jacobi-PCG on the default encoding (CSR-P16 for the stencil operators)
  mixed_bench.py prefine N [--reps R]                   RefinementSolver.with_form("pattern") and ("plain") against fp64 CG on the default encoding
  mixed_bench.py dspmv  N [--op varcoef|poisson]        the diagonal lowering (CsrMatrix.lower("dia")): kryst_spmv32 on the plain arrays and on the fp32
                                                        streams -- as shipped, with plain instead of nontemporal value loads, with 1 / 2 / 4 workgroups
                                                        per compute unit -- against the fp64 kryst_spmv on CSR-DIA (spmv_dia_kernel).  poisson is created
                                                        under KRYST_SPMV_DIA=2 so that it keeps streams
  mixed_bench.py drate  N [--op varcoef]                CG32 / PCG32 it/s on the dia-lowered and on the plain-lowered operator against fp64 CG /
                                                        Jacobi-PCG on CSR-DIA
  mixed_bench.py drefine N [--op varcoef] [--reps R]    RefinementSolver.with_form("dia") and ("plain") against fp64 CG / Jacobi-PCG on CSR-DIA

The versions ALTERNATE inside the process after a warm-up; every timed window lasts at least half a second (spmv: a run of launches between
two hipEvents; rate: the difference of two solves at IT and 3 IT iterations with tol = 0, wall clock, IT sized from a calibration solve so that
2 IT iterations take >= 0.6 s; refine: whole solves, wall clock, lowering and first-use allocations taken out by a warm-up call).  Medians.

Bytes, from shapes: fp64 plain-CSR SpMV 12 nnz + 4 (n + 1) + 16 n; spmv32 8 nnz + 4 (n + 1) + 8 n; CSR-P16 18 n in fp64 and 10 n in fp32; CSR-DIA with D
diagonals (8 D + 16) n in fp64 and (4 D + 8) n in fp32.  `band`: the non-stencil operator of
tools/multi_rhs_only.py (seven entries per row at jittered offsets, no two rows alike: no compressed form applies)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import kryst_amd as K

PEAK = 8.0e12
WINDOW_S = 0.5
OUT = None


def emit(rec):
    rec["sources"] = K._ffi.source_sha16()
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


def use(plain):
    """which form of the operator the fp64 SpMV streams from now on: plain CSR (KRYST_SPMV_COMPRESS=0) or the library's own choice -- the
    knob is read per launch outside a solve and once per solve inside one"""
    if plain:
        os.environ["KRYST_SPMV_COMPRESS"] = "0"
    else:
        os.environ.pop("KRYST_SPMV_COMPRESS", None)


def operator(name, N, ctx, dia=False):
    """dia: created under KRYST_SPMV_DIA=2, so that an operator with a more compact form keeps CSR-DIA streams as well"""
    if dia:
        os.environ["KRYST_SPMV_DIA"] = "2"
    try:
        return band(N, ctx) if name == "band" else K.CsrMatrix.stencil7(N, name, ctx=ctx)
    finally:
        os.environ.pop("KRYST_SPMV_DIA", None)


def encoding(a, plain):
    use(plain)
    e = a.encoding()[0]
    assert not plain or e == "csr", e
    return e


def alternate(sides, reps):
    got = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            got[k].append(f())
    return {k: statistics.median(v) for k, v in got.items()}


# ---------------------------------------------------------------------------------------------------------------- SpMV
def spmv_case(name, N, reps):
    ctx = K.Context(0)
    a = operator(name, N, ctx)
    a32 = a.lower()
    n, nnz = a.nrows(), a.nnz
    encoding(a, True)                                      # plain CSR for the whole case
    x, y = ctx.vec(n).fill_splitmix(3), ctx.vec(n)
    x32, y32 = K.DeviceVec32.from_f64(x), K.DeviceVec32(ctx, n)

    def window(fn, launches):
        ctx.timer_start()
        for _ in range(launches):
            fn()
        return ctx.timer_stop() / launches

    f64, f32 = (lambda: a.spmv(x, y)), (lambda: a32.spmv(x32, y32))
    count = {}
    for k, fn in (("fp64", f64), ("fp32", f32)):
        window(fn, 20)
        count[k] = max(20, int(math.ceil(WINDOW_S * 1.2 / (window(fn, 50) * 1e-3))))
    r = alternate({"fp64": lambda: window(f64, count["fp64"]), "fp32": lambda: window(f32, count["fp32"])}, reps)
    b64, b32 = 12 * nnz + 4 * (n + 1) + 16 * n, 8 * nnz + 4 * (n + 1) + 8 * n
    emit({"case": "spmv", "op": name, "N": N, "n": n, "nnz": nnz, "windows": reps, "launches_per_window": count, "info": a32.info,
          "spmv_fp64_plain_csr_ms": round(r["fp64"], 5), "spmv32_ms": round(r["fp32"], 5),
          "bytes_fp64": b64, "bytes_fp32": b32, "bytes_per_row_fp64": round(b64 / n, 2), "bytes_per_row_fp32": round(b32 / n, 2),
          "fp64_frac_8TBps": round(b64 / (r["fp64"] * 1e-3) / PEAK, 4), "fp32_frac_8TBps": round(b32 / (r["fp32"] * 1e-3) / PEAK, 4),
          "time_ratio_fp64_over_fp32": round(r["fp64"] / r["fp32"], 3), "byte_ratio_fp64_over_fp32": round(b64 / b32, 3)})


# ---------------------------------------------------------------------------------------------------------------- iteration rate
def rate_case(name, N, reps):
    ctx = K.Context(0)
    plain = dflt = operator(name, N, ctx)                   # one operator, streamed in either form
    a32 = plain.lower()
    n = plain.nrows()
    default_encoding = encoding(dflt, False)
    b = plain.spmv(ctx.vec(n).fill(1.0))
    b32 = K.DeviceVec32.from_f64(b)
    x, x32 = ctx.vec(n), K.DeviceVec32(ctx, n)
    zero32 = np.zeros(n, dtype=np.float32)
    for method, cls64, cls32 in (("cg", K.CgSolver, K.Cg32Solver), ("pcg_jacobi", K.PcgSolver, K.Pcg32Solver)):
        pcs = {"plain": K.Jacobi().setup(plain), "default": K.Jacobi().setup(dflt)} if method != "cg" else {"plain": None, "default": None}

        def timed(kind, iters):
            use(kind == "fp64_plain")
            if kind == "fp32":
                x32.upload(zero32)
            else:
                x.fill(0.0)
            ctx.synchronize()
            t0 = time.perf_counter()
            if kind == "fp32":
                st = cls32(0.0, iters).solve(a32, pcs["plain"], b32, x32)
            else:
                st = cls64(0.0, iters).solve(plain if kind == "fp64_plain" else dflt, pcs["plain" if kind == "fp64_plain" else "default"], b, x)
            return time.perf_counter() - t0, st.iterations

        rec = {"case": "rate", "op": name, "N": N, "n": n, "method": method, "windows": reps, "default_encoding": default_encoding}
        kinds = ("fp32", "fp64_plain", "fp64_default")
        its, lo, hi = {}, {k: [] for k in kinds}, {k: [] for k in kinds}
        for kind in kinds:                                   # calibration: IT such that 2 IT iterations take >= 0.6 s
            timed(kind, 10)
            per = max((timed(kind, 60)[0] - timed(kind, 20)[0]) / 40, 1e-6)
            its[kind] = max(20, int(math.ceil(0.3 / per)))
        for _ in range(reps):                                # the versions alternate
            for kind in kinds:
                lo[kind].append(timed(kind, its[kind]))
                hi[kind].append(timed(kind, 3 * its[kind]))
        for kind in kinds:
            t_lo, t_hi = statistics.median(t for t, _ in lo[kind]), statistics.median(t for t, _ in hi[kind])
            n_lo, n_hi = lo[kind][0][1], hi[kind][0][1]      # (a solve whose residual reaches exactly 0 ends before its cap: counted as run)
            rec[kind + "_iterations"] = [n_lo, n_hi]
            rec[kind + "_window_s"] = round(t_hi - t_lo, 4)
            # (no rate when both solves ended at the same iteration: a grid too small for a half-second window)
            rec[kind + "_iterations_per_s"] = round((n_hi - n_lo) / (t_hi - t_lo), 2) if n_hi > n_lo and t_hi > t_lo else None
        for other in ("fp64_plain", "fp64_default"):
            if rec["fp32_iterations_per_s"] and rec[other + "_iterations_per_s"]:
                rec["ratio_fp32_over_" + other] = round(rec["fp32_iterations_per_s"] / rec[other + "_iterations_per_s"], 3)
        emit(rec)


# ---------------------------------------------------------------------------------------------------------------- time to tolerance
def refine_case(name, N, reps, jacobi):
    ctx = K.Context(0)
    a = operator(name, N, ctx)                             # one operator, streamed in either form
    n = a.nrows()
    default_encoding = encoding(a, False)
    encoding(a, True)
    b = a.spmv(ctx.vec(n).fill_splitmix(7))
    x = ctx.vec(n)
    cap = 20000
    pc = K.Jacobi().setup(a) if jacobi else None
    fp64 = K.PcgSolver if jacobi else K.CgSolver
    ref = K.RefinementSolver(1e-10, 40).with_inner(1e-6, cap)
    ref.lowered(a)                                         # (the lowering is made once per operator: not part of a solve's time)
    rec = {"case": "refine", "op": name, "N": N, "n": n, "inner": "pcg_jacobi" if jacobi else "cg", "outer_tol": 1e-10, "inner_tol": 1e-6,
           "runs": reps, "default_encoding": default_encoding, "lowering": ref.lowered(a).info}

    def run_refine(plain):
        use(plain)
        x.fill(0.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        st = ref.solve(a, pc, b, x)
        ms = (time.perf_counter() - t0) * 1e3
        rec["refine_" + ("plain" if plain else "default")] = {
            "outer_steps": st.iterations, "inner_iterations": st.inner_iterations, "total_inner": sum(st.inner_iterations),
            "converged": st.converged, "final_over_first": ref.residual_history[-1] / ref.residual_history[0]}
        ref.clear_history()
        return ms

    def run_fp64(plain):
        use(plain)
        x.fill(0.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        st = fp64(1e-10, cap).solve(a, pc, b, x)
        ms = (time.perf_counter() - t0) * 1e3
        rec["fp64_" + ("plain" if plain else "default")] = {"iterations": st.iterations, "converged": st.converged}
        return ms

    # warm-up: first-use allocations (the work arena, the reduction scratch) on both paths
    warm = K.RefinementSolver(1e-10, 1).with_inner(1e-6, 5)
    warm._lowered.update(ref._lowered)
    warm.solve(a, pc, b, ctx.vec(n))
    fp64(0.0, 5).solve(a, pc, b, ctx.vec(n))
    ms = alternate({"refine_plain": lambda: run_refine(True), "fp64_plain": lambda: run_fp64(True),
                    "refine_default": lambda: run_refine(False), "fp64_default": lambda: run_fp64(False)}, reps)
    for k, v in ms.items():
        rec[k]["ms"] = round(v, 2)
    for form in ("plain", "default"):
        rec["time_ratio_fp64_over_refine_" + form] = round(ms["fp64_" + form] / ms["refine_" + form], 3)
    emit(rec)



# ---------------------------------------------------------------------------------------------------------------- the row-pattern and the diagonal lowering
# form: "pattern" (pspmv / prate / prefine) or "dia" (dspmv / drate / drefine)
SPMV32_KNOBS = ("KRYST_SPMV32_FORM", "KRYST_SPMV32_STAGE", "KRYST_SPMV32_STAGE_T", "KRYST_SPMV32_DIA_NT", "KRYST_SPMV32_BLOCKS_PER_CU")
SPMV32_KERNELS = {
    "pattern": {"fp32_plain": ({"KRYST_SPMV32_FORM": "plain"}, "plain"), "fp32_pattern": ({"KRYST_SPMV32_STAGE": "0"}, "pattern"),
                "fp32_stage_t1": ({"KRYST_SPMV32_STAGE_T": "1"}, "pattern-stage"), "fp32_stage_t2": ({"KRYST_SPMV32_STAGE_T": "2"}, "pattern-stage")},
    "dia": {"fp32_plain": ({"KRYST_SPMV32_FORM": "plain"}, "plain"), "fp32_dia": ({}, "dia"),
            "fp32_dia_plain_loads": ({"KRYST_SPMV32_DIA_NT": "0"}, "dia"), "fp32_dia_nontemporal": ({"KRYST_SPMV32_DIA_NT": "1"}, "dia"),
            "fp32_dia_bpc1": ({"KRYST_SPMV32_BLOCKS_PER_CU": "1"}, "dia"), "fp32_dia_bpc2": ({"KRYST_SPMV32_BLOCKS_PER_CU": "2"}, "dia"),
            "fp32_dia_bpc4": ({"KRYST_SPMV32_BLOCKS_PER_CU": "4"}, "dia")}}


def yardstick(a, form):
    """the fp64 encoding the case is measured against, for the whole case: the operator's own, or CSR-DIA (spmv_dia_kernel) for the diagonal form"""
    if form != "dia":
        return encoding(a, False)
    os.environ["KRYST_SPMV_COMPRESS"] = "1"
    e = a.encoding()[0]
    assert e == "csr-dia", e
    return e


def knobs32(env):
    for k in SPMV32_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


def pspmv_case(name, N, reps, form="pattern"):
    ctx = K.Context(0)
    a = operator(name, N, ctx, dia=form == "dia")
    a32 = a.lower(form)
    n, nnz = a.nrows(), a.nnz
    enc = yardstick(a, form)
    D = a.encoding()[1] if form == "dia" else 0
    x, y = ctx.vec(n).fill_splitmix(3), ctx.vec(n)
    x32, y32 = K.DeviceVec32.from_f64(x), K.DeviceVec32(ctx, n)
    knobs32({})
    staged = a32.encoding() == "pattern-stage"

    def window(fn, launches, env):
        knobs32(env)
        ctx.timer_start()
        for _ in range(launches):
            fn()
        return ctx.timer_stop() / launches

    sides = {"fp64_default": ((lambda: a.spmv(x, y)), {})}
    for k, (env, kernel) in SPMV32_KERNELS[form].items():
        if kernel != "pattern-stage" or staged:
            knobs32(env)
            assert a32.encoding() == kernel, (k, a32.encoding())
            sides[k] = ((lambda: a32.spmv(x32, y32)), env)
    count = {}
    for k, (fn, env) in sides.items():
        window(fn, 20, env)
        count[k] = max(20, int(math.ceil(WINDOW_S * 1.2 / (window(fn, 50, env) * 1e-3))))
    r = alternate({k: (lambda k=k: window(sides[k][0], count[k], sides[k][1])) for k in sides}, reps)
    knobs32({})
    nbytes = {"fp64_default": 18 * n if enc == "csr-p16" else (8 * D + 16) * n if form == "dia" else None, "fp32_plain": 8 * nnz + 4 * (n + 1) + 8 * n}
    rec = {"case": form[0] + "spmv", "op": name, "N": N, "n": n, "nnz": nnz, "windows": reps, "launches_per_window": count, "fp64_encoding": enc,
           "fp64_pattern_info": a.pattern_info(), "default_kernel": a32.encoding()}
    if form == "dia":
        rec["diagonals"] = D
    for k in sides:
        b = nbytes.get(k, (4 * D + 8) * n if form == "dia" else 10 * n)
        rec[k + "_ms"] = round(r[k], 5)
        if b:
            rec[k + "_bytes_per_row"] = round(b / n, 2)
            rec[k + "_frac_8TBps"] = round(b / (r[k] * 1e-3) / PEAK, 4)
        if k != "fp64_default":
            rec["time_ratio_fp64_over_" + k] = round(r["fp64_default"] / r[k], 3)
    emit(rec)


def prate_case(name, N, reps, form="pattern"):
    ctx = K.Context(0)
    a = operator(name, N, ctx, dia=form == "dia")
    fp32_form = "fp32_" + form
    lowered = {fp32_form: a.lower(form), "fp32_plain": a.lower()}
    n = a.nrows()
    enc = yardstick(a, form)
    knobs32({})
    b = a.spmv(ctx.vec(n).fill(1.0))
    b32 = K.DeviceVec32.from_f64(b)
    x, x32 = ctx.vec(n), K.DeviceVec32(ctx, n)
    zero32 = np.zeros(n, dtype=np.float32)
    for method, cls64, cls32 in (("cg", K.CgSolver, K.Cg32Solver), ("pcg_jacobi", K.PcgSolver, K.Pcg32Solver)):
        pc = K.Jacobi().setup(a) if method != "cg" else None

        def timed(kind, iters):
            if kind == "fp64_default":
                x.fill(0.0)
            else:
                x32.upload(zero32)
            ctx.synchronize()
            t0 = time.perf_counter()
            st = cls64(0.0, iters).solve(a, pc, b, x) if kind == "fp64_default" else cls32(0.0, iters).solve(lowered[kind], pc, b32, x32)
            return time.perf_counter() - t0, st.iterations

        rec = {"case": form[0] + "rate", "op": name, "N": N, "n": n, "method": method, "windows": reps, "fp64_encoding": enc,
               fp32_form + "_kernel": lowered[fp32_form].encoding()}
        kinds = (fp32_form, "fp32_plain", "fp64_default")
        its, lo, hi = {}, {k: [] for k in kinds}, {k: [] for k in kinds}
        for kind in kinds:
            timed(kind, 10)
            per = max((timed(kind, 60)[0] - timed(kind, 20)[0]) / 40, 1e-6)
            its[kind] = max(20, int(math.ceil(0.3 / per)))
        for _ in range(reps):
            for kind in kinds:
                lo[kind].append(timed(kind, its[kind]))
                hi[kind].append(timed(kind, 3 * its[kind]))
        for kind in kinds:
            t_lo, t_hi = statistics.median(t for t, _ in lo[kind]), statistics.median(t for t, _ in hi[kind])
            n_lo, n_hi = lo[kind][0][1], hi[kind][0][1]
            rec[kind + "_iterations"] = [n_lo, n_hi]
            rec[kind + "_window_s"] = round(t_hi - t_lo, 4)
            rec[kind + "_iterations_per_s"] = round((n_hi - n_lo) / (t_hi - t_lo), 2) if n_hi > n_lo and t_hi > t_lo else None
        for kind in (fp32_form, "fp32_plain"):
            if rec[kind + "_iterations_per_s"] and rec["fp64_default_iterations_per_s"]:
                rec["ratio_" + kind + "_over_fp64_default"] = round(rec[kind + "_iterations_per_s"] / rec["fp64_default_iterations_per_s"], 3)
        emit(rec)


def prefine_case(name, N, reps, jacobi, form="pattern"):
    ctx = K.Context(0)
    a = operator(name, N, ctx, dia=form == "dia")
    n = a.nrows()
    enc = yardstick(a, form)
    knobs32({})
    b = a.spmv(ctx.vec(n).fill_splitmix(7))
    x = ctx.vec(n)
    cap = 20000
    pc = K.Jacobi().setup(a) if jacobi else None
    fp64 = K.PcgSolver if jacobi else K.CgSolver
    refs = {f: K.RefinementSolver(1e-10, 40).with_inner(1e-6, cap).with_form(f) for f in (form, "plain")}
    rec = {"case": form[0] + "refine", "op": name, "N": N, "n": n, "inner": "pcg_jacobi" if jacobi else "cg", "outer_tol": 1e-10, "inner_tol": 1e-6,
           "runs": reps, "fp64_encoding": enc, "kernels": {f: r.lowered(a).encoding() for f, r in refs.items()}}

    def run_refine(form):
        ref = refs[form]
        x.fill(0.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        st = ref.solve(a, pc, b, x)
        ms = (time.perf_counter() - t0) * 1e3
        rec["refine_" + form] = {"outer_steps": st.iterations, "inner_iterations": st.inner_iterations, "total_inner": sum(st.inner_iterations),
                                 "converged": st.converged, "final_over_first": ref.residual_history[-1] / ref.residual_history[0]}
        ref.clear_history()
        return ms

    def run_fp64():
        x.fill(0.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        st = fp64(1e-10, cap).solve(a, pc, b, x)
        ms = (time.perf_counter() - t0) * 1e3
        rec["fp64_default"] = {"iterations": st.iterations, "converged": st.converged}
        return ms

    for f, r in refs.items():                              # warm-up: first-use allocations on every path
        warm = K.RefinementSolver(1e-10, 1).with_inner(1e-6, 5).with_form(f)
        warm._lowered.update(r._lowered)
        warm.solve(a, pc, b, ctx.vec(n))
    fp64(0.0, 5).solve(a, pc, b, ctx.vec(n))
    ms = alternate({"refine_" + form: lambda: run_refine(form), "fp64_default": run_fp64, "refine_plain": lambda: run_refine("plain")}, reps)
    for k, v in ms.items():
        rec[k]["ms"] = round(v, 2)
    for f in (form, "plain"):
        rec["time_ratio_fp64_over_refine_" + f] = round(ms["fp64_default"] / ms["refine_" + f], 3)
    emit(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("spmv", "rate", "refine", "pspmv", "prate", "prefine", "dspmv", "drate", "drefine"))
    ap.add_argument("N", type=int)
    ap.add_argument("--op", default="poisson", choices=("poisson", "varcoef", "band"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jacobi", action="store_true", help="refine: Jacobi-PCG inside and as the fp64 yardstick (default for varcoef)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT = args.out
    if args.mode == "spmv":
        spmv_case(args.op, args.N, args.reps)
    elif args.mode == "rate":
        rate_case(args.op, args.N, args.reps)
    elif args.mode in ("pspmv", "dspmv"):
        pspmv_case(args.op, args.N, args.reps, "dia" if args.mode[0] == "d" else "pattern")
    elif args.mode in ("prate", "drate"):
        prate_case(args.op, args.N, args.reps, "dia" if args.mode[0] == "d" else "pattern")
    elif args.mode in ("prefine", "drefine"):
        prefine_case(args.op, args.N, args.reps, args.jacobi or args.op == "varcoef", "dia" if args.mode[0] == "d" else "pattern")
    else:
        refine_case(args.op, args.N, args.reps, args.jacobi or args.op == "varcoef")
