"""CG / PCG iterations per second with x updated in BATCHES (KRYST_CG_X_BATCH = m <= 32: x += alpha_i p_i for m iterations in one pass, XBatchOp) against
the fused form that updates x every iteration (m = 1) and the unfused form, interleaved in ONE process on one operator instance.  Every form is
timed over whole batches: the warm-up and the timed stretch are multiples of its m, the timed stretch at least 4 m iterations.
XS_LIST: the ways a batch is paid (KRYST_CG_X_SLICE: 0 = all rows every m-th iteration, 1 = one slice of the rows per iteration), each m > 1 with each.
usage: [XB_LIST=1,8,12,16,24,32] [XS_LIST=0,1] [SOLVERS=cg,pcg] cg_xbatch_ab.py [grid=512] [steps=192] [rounds=3]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K
grid = int(sys.argv[1]) if len(sys.argv) > 1 else 512
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 192
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
MS = [int(v) for v in os.environ.get("XB_LIST", "1,8,12,16,24,32").split(",")]
XS = [int(v) for v in os.environ.get("XS_LIST", "0,1").split(",")]
SOLVERS = os.environ.get("SOLVERS", "cg,pcg").split(",")
ctx = K.Context(0)
a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
n = a.nrows()
b = a.spmv(ctx.vec(n).fill(1.0))
pcj = K.Jacobi().setup(a)
forms = [("unfused", 1, {"KRYST_CG_FUSE_P": "0", "KRYST_CG_X_BATCH": "1", "KRYST_CG_X_SLICE": "0"})] + \
        [(f"fused x-batch {m}" + (" in slices" if xs else ""), m, {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_T": "4", "KRYST_CG_X_BATCH": str(m), "KRYST_CG_X_SLICE": str(xs)})
         for m in MS for xs in (XS if m > 1 else [0])]
res = {}
for method, pc in (("cg", None), ("pcg", pcj)):
    if method not in SOLVERS:
        continue
    for rnd in range(rounds):
        for name, m, env in forms:
            for k, v in env.items():
                os.environ[k] = v
            warm = -(-16 // m) * m                                   # whole batches before the clock starts ...
            timed = -(-max(steps, 4 * m) // m) * m                   # ... and under it
            x = ctx.vec(n)
            with K.Session(method, a, pc, b, x, tol=0.0, max_iters=warm + timed) as s:
                s.step(warm); ctx.synchronize()
                t0 = time.perf_counter(); s.step(timed); ctx.synchronize(); dt = time.perf_counter() - t0
                st = s.end()
            res.setdefault((method, name), []).append((timed / dt, timed, st.iterations, st.final_residual, float(x.to_host()[n // 3])))
            del x
    for name, m, _ in forms:
        v = res[(method, name)]
        rate = [x[0] for x in v]
        # (forms of different m run different iteration counts: the residual and x are comparable between forms that ran the same number)
        print(json.dumps({"grid": grid, "solver": method, "form": name, "timed_iterations": v[0][1], "iterations_per_s": [round(r, 1) for r in rate],
                          "mean": round(sum(rate) / len(rate), 1), "spread": round(max(rate) - min(rate), 1),
                          "iterations": v[0][2], "final_residual": v[0][3], "x_probe": v[0][4],
                          "same_every_round": all(x[2:] == v[0][2:] for x in v)}), flush=True)
