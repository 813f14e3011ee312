#!/usr/bin/env python3
"""The compiler's register, scratch and spill figures of the marching instances of spmv_fuse.hip (spmv_pattern_fuse_kernel<.., MARCH = true, ..>,
cg_recompute_residual_kernel<..>) for gfx950: a device-only cross-compile with -Rpass-analysis=kernel-resource-usage, no GPU needed.
usage: resource_usage.py [csrc directory = this tree's] [label]"""
import os, re, subprocess, sys, tempfile
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "kryst_amd", "csrc")
label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with tempfile.TemporaryDirectory() as tmp:
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I/opt/rocm/include", "-x", "hip",
                        "--cuda-device-only", "-c", "spmv_fuse.hip", "-o", os.path.join(tmp, "o"), "-Rpass-analysis=kernel-resource-usage"],
                       cwd=src, capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr[-4000:])
kernels, cur = [], None
for line in r.stderr.splitlines():
    m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
    if not m: continue
    key, _, val = m.group(1).partition(": ")
    if key == "Function Name": cur = {"name": val}; kernels.append(cur)
    elif cur is not None: cur[key.strip()] = val
names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in kernels), capture_output=True, text=True).stdout.splitlines()
print(label)
for k, full in zip(kernels, names):
    short = re.sub(r"^void kr::|\(.*$", "", full)
    march = re.match(r"spmv_pattern_fuse_kernel<\d, \d, \d+, (true|false), true", short)
    if not (march or short.startswith("cg_recompute_residual_kernel")): continue
    print(f"{short:78s} VGPRs {int(k['VGPRs']):3d}  SGPRs {int(k['TotalSGPRs']):3d}  scratch {k['ScratchSize [bytes/lane]']} B/lane  "
          f"spills {int(k['SGPRs Spill']) + int(k['VGPRs Spill'])}  waves/SIMD possible {k['Occupancy [waves/SIMD]']}")
