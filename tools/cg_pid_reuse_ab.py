"""CG iterations per second with the marching kernels keeping repeated row-pattern ids in registers (KRYST_SPMV_PID_REUSE=1) against loading them at
every plane (=0), interleaved in ONE process on one operator instance (the knob is read per launch), with the fused form, its marching mode and the
recompute-Ap residual pass forced (KRYST_CG_FUSE_P=1, KRYST_SPMV_FUSE_MARCH=1, KRYST_CG_RECOMPUTE_AP=1 unless given) so that the smaller grids take
them too.  The final residual of the two forms must be the same bits.
usage: cg_pid_reuse_ab.py [grids=512,256,384] [steps=60] [rounds=3] [recompute_ap=1]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K
grids = [int(g) for g in (sys.argv[1] if len(sys.argv) > 1 else "512,256,384").split(",")]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ctx = K.Context(0)
os.environ["KRYST_CG_FUSE_P"] = "1"
os.environ["KRYST_SPMV_FUSE_MARCH"] = "1"
os.environ["KRYST_CG_RECOMPUTE_AP"] = sys.argv[4] if len(sys.argv) > 4 else "1"
forms = [("reload", "0"), ("reuse", "1")]
for grid in grids:
    a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
    n = a.nrows()
    b = a.spmv(ctx.vec(n).fill(1.0))
    os.environ["KRYST_SPMV_PID_REUSE"] = "1"
    info = a.fuse_march_info()
    res = {}
    for rnd in range(rounds):
        for name, m in forms:
            os.environ["KRYST_SPMV_PID_REUSE"] = m
            x = ctx.vec(n)
            with K.Session("cg", a, None, b, x, tol=0.0, max_iters=10 + steps) as s:
                s.step(10); ctx.synchronize()
                t0 = time.perf_counter(); s.step(steps); ctx.synchronize(); dt = time.perf_counter() - t0
                st = s.end()
            res.setdefault(name, []).append((steps / dt, st.final_residual))
            del x
    for name, _ in forms:
        v = res[name]
        print(json.dumps({"grid": grid, "form": name, "march_info": info, "iterations_per_s": [round(x[0], 1) for x in v], "mean": round(sum(x[0] for x in v) / len(v), 1),
                          "final_residual": v[0][1], "same_residual_as_reload": v[0][1] == res["reload"][0][1]}), flush=True)
    print(json.dumps({"grid": grid, "reuse_over_reload": round(sum(x[0] for x in res["reuse"]) / sum(x[0] for x in res["reload"]), 4)}), flush=True)
    del a, b
