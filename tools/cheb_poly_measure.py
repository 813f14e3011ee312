#!/usr/bin/env python3
"""Runs the measurements of DESIGN.md section 4.15 (tools/cheb_poly_only.py), one child process per step, each under its own time limit;
the first step that fails, faults or runs out of time ends the run (nothing more is started on the GPU) and is reported with its exit status.

  cheb_poly_measure.py OUTDIR [step ...]      steps: apply256 apply512 pcg64 pcg256 pcg512 gmres256 trace256   (default: all, in this order)

OUTDIR/<step>.jsonl receives the step's JSON lines, OUTDIR/<step>.log its stderr; trace256 runs under `rocprofv3 --kernel-trace --stats`, a
run of its own, and leaves the profiler's files in OUTDIR/trace256/."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY = os.path.join(ROOT, "tools", "cheb_poly_only.py")
STEPS = {                    # name -> (mode, N, seconds allowed)
    "apply256": ("apply", 256, 240), "apply512": ("apply", 512, 480),
    "pcg64": ("pcg", 64, 120), "pcg256": ("pcg", 256, 300), "pcg512": ("pcg", 512, 600),
    "gmres256": ("gmres", 256, 420), "trace256": ("trace", 256, 420),
}


def main():
    out = sys.argv[1]
    names = sys.argv[2:] or list(STEPS)
    os.makedirs(out, exist_ok=True)
    for name in names:
        mode, n, limit = STEPS[name]
        cmd = [sys.executable, ONLY, mode, str(n)]
        if mode == "trace":
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(out, name), "--"] + cmd
        print(f"[cheb_poly_measure] {name}: {' '.join(cmd)} (limit {limit} s)", flush=True)
        with open(os.path.join(out, name + ".jsonl"), "w") as so, open(os.path.join(out, name + ".log"), "w") as se:
            try:
                rc = subprocess.run(cmd, stdout=so, stderr=se, timeout=limit, cwd=ROOT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
        sys.stdout.write(open(os.path.join(out, name + ".jsonl")).read())
        if rc != 0:
            sys.stdout.write(open(os.path.join(out, name + ".log")).read()[-3000:])
            print(f"[cheb_poly_measure] {name} ended with status {rc}: stopping here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
