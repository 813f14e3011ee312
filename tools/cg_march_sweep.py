"""Sweep of the marching mode's knobs in one process: planes per segment S x tiles per strip T x resident workgroups per CU (LDS padding), each
against the un-marched kernel measured beside it (best of two 60-iteration stretches of a CG session).
usage: cg_march_sweep.py [grid=512] [steps=60] [S=32,64,86,128] [wg=0,2]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kryst_amd as K
grid = int(sys.argv[1]) if len(sys.argv) > 1 else 512
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
segs = (sys.argv[3] if len(sys.argv) > 3 else "32,64,86,128").split(",")
wgs = (sys.argv[4] if len(sys.argv) > 4 else "0,2").split(",")
ctx = K.Context(0)
a = K.CsrMatrix.stencil7(grid, "poisson", ctx=ctx)
n = a.nrows()
b = a.spmv(ctx.vec(n).fill(1.0))
os.environ["KRYST_CG_FUSE_P"] = "1"
def run(env):
    for k, v in env.items():
        os.environ[k] = v
    best = 0.0
    for _ in range(2):
        x = ctx.vec(n)
        with K.Session("cg", a, None, b, x, tol=0.0, max_iters=10 + steps) as s:
            s.step(10); ctx.synchronize()
            t0 = time.perf_counter(); s.step(steps); ctx.synchronize(); dt = time.perf_counter() - t0
            s.end()
        best = max(best, steps / dt)
    return round(best, 1)
for T in ("4", "2"):
    print(json.dumps({"grid": grid, "form": "un-marched", "T": int(T), "it_s": run({"KRYST_SPMV_FUSE_MARCH": "0", "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_WG_PER_CU": "0"})}), flush=True)
    for S in segs:
        for wg in wgs:
            print(json.dumps({"grid": grid, "form": "marching", "T": int(T), "S": int(S), "wg_per_cu": int(wg),
                              "it_s": run({"KRYST_SPMV_FUSE_MARCH": "1", "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_SEG": S, "KRYST_SPMV_FUSE_WG_PER_CU": wg})}), flush=True)
    print(json.dumps({"grid": grid, "form": "un-marched", "T": int(T), "it_s": run({"KRYST_SPMV_FUSE_MARCH": "0", "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_WG_PER_CU": "0"})}), flush=True)
