"""CG iterations per second of several forms of the marching kernels, interleaved in ONE process on one operator instance (the knobs are read per
launch), with the fused form, its marching mode and the recompute-Ap residual pass forced (KRYST_CG_FUSE_P=1, KRYST_SPMV_FUSE_MARCH=1,
KRYST_CG_RECOMPUTE_AP=1) so that the smaller grids take them too.  A form is NAME:KNOB=VALUE[,KNOB=VALUE ...]; the first one is the base.  The final
residual of every form must be the base's bits.  The project's rule is printed per form against the base: every run above every run, and the means
apart by at least twice the larger spread (max - min).
usage: cg_forms_ab.py FORMS [grids=512] [steps=60] [rounds=3]     e.g.  cg_forms_ab.py "T4:KRYST_SPMV_FUSE_T=4;T2:KRYST_SPMV_FUSE_T=2" 512,384,256"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K
forms = []
for spec in sys.argv[1].split(";"):
    name, _, knobs = spec.partition(":")
    forms.append((name, dict(kv.split("=", 1) for kv in knobs.split(",") if kv)))
grids = [int(g) for g in (sys.argv[2] if len(sys.argv) > 2 else "512").split(",")]
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 60
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ctx = K.Context(0)
os.environ["KRYST_CG_FUSE_P"] = "1"
os.environ["KRYST_SPMV_FUSE_MARCH"] = "1"
os.environ["KRYST_CG_RECOMPUTE_AP"] = "1"
for grid in grids:
    a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
    n = a.nrows()
    b = a.spmv(ctx.vec(n).fill(1.0))
    res, infos = {}, {}
    for rnd in range(rounds):
        for name, knobs in forms:
            for k, v in knobs.items():
                os.environ[k] = v
            infos[name] = a.fuse_march_info()
            x = ctx.vec(n)
            with K.Session("cg", a, None, b, x, tol=0.0, max_iters=10 + steps) as s:
                s.step(10); ctx.synchronize()
                t0 = time.perf_counter(); s.step(steps); ctx.synchronize(); dt = time.perf_counter() - t0
                st = s.end()
            res.setdefault(name, []).append((steps / dt, st.final_residual))
            del x
    base = [x[0] for x in res[forms[0][0]]]
    for name, knobs in forms:
        v = [x[0] for x in res[name]]
        spread = max(v) - min(v)
        line = {"grid": grid, "form": name, "knobs": knobs, "march_info": infos[name], "iterations_per_s": [round(x, 1) for x in v],
                "mean": round(sum(v) / len(v), 1), "spread": round(spread, 1), "final_residual": res[name][0][1],
                "same_residual_as_base": all(x[1] == res[forms[0][0]][0][1] for x in res[name])}
        if name != forms[0][0]:
            gap = sum(v) / len(v) - sum(base) / len(base)
            line["over_base"] = round(sum(v) / sum(base), 4)
            line["gain_by_the_rule"] = bool(min(v) > max(base) and gap >= 2 * max(spread, max(base) - min(base)))
        print(json.dumps(line), flush=True)
    del a, b
