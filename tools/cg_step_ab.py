"""CG iterations per second with the recompute residual pass taking the leg values as kernel arguments (KRYST_SPMV_LEG_VALUES=1) against the per-entry
table look-ups (=0), interleaved in ONE process on one operator instance (the knob is read per launch), with the fused form, its marching mode and the
recompute-Ap residual pass forced (KRYST_CG_FUSE_P=1, KRYST_SPMV_FUSE_MARCH=1, KRYST_CG_RECOMPUTE_AP=1) so that the smaller grids take them too.  The
final residual of the two forms must be the same bits.
usage: cg_step_ab.py [grids=512,256,384] [steps=60] [rounds=3]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K
grids = [int(g) for g in (sys.argv[1] if len(sys.argv) > 1 else "512,256,384").split(",")]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ctx = K.Context(0)
os.environ["KRYST_CG_FUSE_P"] = "1"
os.environ["KRYST_SPMV_FUSE_MARCH"] = "1"
os.environ["KRYST_CG_RECOMPUTE_AP"] = "1"
forms = [("table", "0"), ("leg_values", "1")]
for grid in grids:
    a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
    n = a.nrows()
    b = a.spmv(ctx.vec(n).fill(1.0))
    res, infos = {}, {}
    for rnd in range(rounds):
        for name, m in forms:
            os.environ["KRYST_SPMV_LEG_VALUES"] = m
            infos[name] = a.leg_values_info()
            x = ctx.vec(n)
            with K.Session("cg", a, None, b, x, tol=0.0, max_iters=10 + steps) as s:
                s.step(10); ctx.synchronize()
                t0 = time.perf_counter(); s.step(steps); ctx.synchronize(); dt = time.perf_counter() - t0
                st = s.end()
            res.setdefault(name, []).append((steps / dt, st.final_residual))
            del x
    for name, _ in forms:
        v = res[name]
        print(json.dumps({"grid": grid, "form": name, "march_info": a.fuse_march_info(), "leg_values_info": infos[name], "iterations_per_s": [round(x[0], 1) for x in v],
                          "mean": round(sum(x[0] for x in v) / len(v), 1), "spread": round(max(x[0] for x in v) - min(x[0] for x in v), 1),
                          "final_residual": v[0][1], "same_residual_as_table": v[0][1] == res["table"][0][1]}), flush=True)
    print(json.dumps({"grid": grid, "leg_values_over_table": round(sum(x[0] for x in res["leg_values"]) / sum(x[0] for x in res["table"]), 4)}), flush=True)
    del a, b
