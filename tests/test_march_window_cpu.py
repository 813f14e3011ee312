"""The window map of the marching kernels (kryst_amd/csrc/march_window.h), without a GPU.

tests/cpp/test_march_window.cpp is a stand-alone program that includes only that header and runs the map over every even line length n from 4 to
512, strips of T = 2, 4 and 8 tiles and workgroups of 256 and 512 threads.  It asserts that every pair of the window is requested by exactly one
(lane, request), that request k of a lane is the pair of rows of its own tile k, that no LDS offset leaves the window (the buffer it marks is
exactly as long as the window) and that every lane issues ceil((R + 2 n) / (2 threads)) requests.  Built here with AddressSanitizer and UBSan and
run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_window_map(tmp_path):
    exe = str(tmp_path / "test_march_window")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it runs whatever else the loader brings along)
                         os.path.join(ROOT, "tests", "cpp", "test_march_window.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "march window ok" in r.stdout, r.stdout[-2000:]
