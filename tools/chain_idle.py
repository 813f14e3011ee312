#!/usr/bin/env python3
"""Where a CG iteration's time goes BETWEEN its kernels, from a rocprofv3 --kernel-trace CSV of tools/cg_only.py: over the stretch from the first to
the last fused SpMV launch, per iteration, the time each kernel runs, the time in which no kernel at all runs, the time in which no kernel of the
dependent chain (fused SpMV, fold, residual pass, fold) runs, and the mean gap at each kind of boundary.  The trace has one start and one end stamp
per launch: it cannot show how many workgroups of a launch are resident at a given moment.
usage: chain_idle.py <dir with *_kernel_trace.csv>"""
import collections, csv, glob, sys

f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))), key=lambda r: r[0])


def short(name):
    for key, s in (("spmv_pattern_fuse_kernel", "fused"), ("cg_recompute_residual_kernel", "residual"), ("CgAlphaLogic", "fold_alpha"), ("CgBetaLogic", "fold_beta"),
                   ("PcgAlphaLogic", "fold_alpha"), ("PcgBetaLogic", "fold_beta"), ("XBatch", "xbatch")):
        if key in name:
            return s
    return "other"


CHAIN = ("fused", "residual", "fold_alpha", "fold_beta")
fused = [i for i, r in enumerate(rows) if short(r[2]) == "fused"]
if len(fused) < 3:
    sys.exit("no fused SpMV launches in the trace")
win = rows[fused[0]:fused[-1]]                              # iterations 2 .. last - 1, whole
iters = len(fused) - 1
t0, t1 = win[0][0], rows[fused[-1]][0]


def union(spans):
    busy, end = 0, t0
    for s, e in sorted(spans):
        s, e = max(s, end), min(e, t1)
        if e > s:
            busy += e - s; end = e
    return busy


per = collections.defaultdict(lambda: [0, 0])
for s, e, n in win:
    k = short(n); per[k][0] += 1; per[k][1] += e - s
gaps = collections.defaultdict(list)
for (s0, e0, n0), (s1, e1, n1) in zip(win, win[1:] + [rows[fused[-1]]]):
    gaps[(short(n0), short(n1))].append(s1 - e0)
busy_all = union([(s, e) for s, e, _ in win])
busy_chain = union([(s, e) for s, e, n in win if short(n) in CHAIN])
span = t1 - t0
print(f"trace {f.split('/')[-1]}: {iters} iterations, {span / iters / 1e3:.1f} us per iteration")
for k, (c, t) in sorted(per.items(), key=lambda kv: -kv[1][1]):
    print(f"  {k:10s} {c:5d} launches  {t / c / 1e3:9.1f} us per launch  {t / iters / 1e3:8.1f} us per iteration")
print(f"  no kernel at all running:       {(span - busy_all) / iters / 1e3:7.1f} us per iteration")
print(f"  no kernel of the chain running: {(span - busy_chain) / iters / 1e3:7.1f} us per iteration (the x pass counts as such time)")
for (a, b), v in sorted(gaps.items()):
    print(f"  gap {a:10s} -> {b:10s} {len(v):4d} x  mean {sum(v) / len(v) / 1e3:7.2f} us  (negative: the two overlap)")
