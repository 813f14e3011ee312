"""The host bookkeeping of x paid in slices (kryst_amd/csrc/cg_logic.h: XSlices), without a GPU.

tests/cpp/test_x_slices.cpp is a stand-alone program that includes only that struct and drives random sequences of advance / flush / advance for
batch lengths 1, 2, 3, 7, 8, 31, 32 and 0, 1, 5, 31, 32, 33, 64, 1000 tiles against a model of the ring of direction vectors.  It asserts that every
(tile, iteration <= last enqueued) is applied exactly once and in ascending order per tile, that no launch carries more than m updates, that no
launch reads a ring slot an already enqueued iteration has overwritten, and that empty slices launch nothing.  Built here with AddressSanitizer
and UBSan and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x_slices_bookkeeping(tmp_path):
    exe = str(tmp_path / "test_x_slices")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it runs whatever else the loader brings along)
                         os.path.join(ROOT, "tests", "cpp", "test_x_slices.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "x slices ok" in r.stdout, r.stdout[-2000:]
