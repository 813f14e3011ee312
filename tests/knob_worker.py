"""One fresh process for the settings that the sources read once per process (tests/knob_cases.py: per_process).

usage: knob_worker.py <out.npz>.  The environment of the process IS the profile: the parent (tests/test_gpu_knobs.py) sets the four
*_BLOCKS_PER_CU settings and KRYST_NO_ARENA before it starts this script.  Runs the solvers of knob_cases.WORKER_CASES on convdiff
operators and writes, per case, (iterations, converged, final_residual), the residual history and x.  It compares nothing: the parent
holds the references.  A flushed line before every stage, so that a failure names the stage it died in."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import kryst_amd as K                                      # noqa: E402
import knob_cases as KC                                    # noqa: E402

PCN = K.Preconditioning
TOL = KC.WORKER_TOL

SOLVERS = {
    "gmres5_right_jacobi": (lambda mx: K.GmresSolver(5, TOL, mx).with_preconditioning(PCN.Right), "solve"),
    "fgmres5_classical": (lambda mx: K.FgmresSolver(TOL, mx, 5).with_orthog(K.Orthog.Classical), "solve_flex"),
    "fgmres5_modified": (lambda mx: K.FgmresSolver(TOL, mx, 5).with_orthog(K.Orthog.Modified), "solve_flex"),
    "pca5_right_jacobi": (lambda mx: K.PcaGmresSolver(5, 2, 1, TOL, mx).with_preconditioning(PCN.Right), "solve"),
    "sstep3_5_right_jacobi": (lambda mx: K.PcaGmresSolver(5, 1, 3, TOL, mx).with_preconditioning(PCN.Right).with_textbook(), "solve"),
}


def stage(what):
    print("[knob worker] " + what, flush=True)


def main():
    out_path = sys.argv[1]
    names = sorted({k for env in KC.PROFILES.values() for k in env})
    out = {"profile_env": np.array([f"{k}={os.environ[k]}" for k in names if k in os.environ])}
    stage("context; " + ", ".join(out["profile_env"]))
    ctx = K.Context(0)
    ops = {}
    for solver, N, mx in KC.WORKER_CASES:
        if N not in ops:
            stage(f"operator convdiff {N}^3")
            d = K.CsrMatrix.stencil7(N, "convdiff", ctx=ctx)
            ops[N] = (d, d.spmv(np.ones(N ** 3)), K.Jacobi().setup(d))
        d, b, pc = ops[N]
        stage(f"solve {solver} at {N}^3, at most {mx} iterations")
        make, call = SOLVERS[solver]
        s = make(mx)
        x = np.zeros(N ** 3)
        st = getattr(s, call)(d, pc, b, x)
        key = f"{solver}_{N}"
        out[key + "__stats"] = np.array([st.iterations, float(st.converged), st.final_residual])
        out[key + "__hist"] = np.array(s.residual_history, dtype=float)
        out[key + "__x"] = x
    ctx.synchronize()
    np.savez(out_path, **out)
    stage("done")


if __name__ == "__main__":
    main()
