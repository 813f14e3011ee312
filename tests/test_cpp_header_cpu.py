"""Compile-time properties of include/kryst_hip.hpp (no GPU, nothing runs): every class that owns a library handle is move-only.  A copy
of such an object would hand the same handle to its destroy function twice; the property is checked by the compiler, never provoked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every DevicePc kind; the operators, multivector and LU object
PC_KINDS = ["DevicePc", "Jacobi", "Ilu0", "Ilup", "Ilut", "TrueIlu0", "IdentityPC", "ApproxInv", "BlockJacobi", "AdditiveSchwarz", "Sor", "Amg",
            "Spai", "Chebyshev", "ChebyshevPoly"]
OTHER_OWNERS = ["Context", "HipCsrMatrix", "HipDenseMatrix", "MultiVec", "LuSolver", "HipCsrMatrix32"]
# what the header returns by value (BlockJacobi::uniform, from_csr / stencil7, from_raw / from_csr, from_columns) or stores by value after a
# move (ApproxInv's operator), and the preconditioners, which a caller keeps in containers
MOVABLE = PC_KINDS + ["HipCsrMatrix", "HipDenseMatrix", "MultiVec", "HipCsrMatrix32"]


def unit():
    lines = ['#include <type_traits>', '#include "kryst_hip.hpp"', "using namespace kryst;"]
    for t in PC_KINDS + OTHER_OWNERS:
        lines.append(f'static_assert(!std::is_copy_constructible<{t}>::value, "{t} is copy-constructible");')
        lines.append(f'static_assert(!std::is_copy_assignable<{t}>::value, "{t} is copy-assignable");')
    for t in MOVABLE:
        lines.append(f'static_assert(std::is_move_constructible<{t}>::value, "{t} is not move-constructible");')
    # move assignment replaces (and destroys) the handle held: the kinds without a by-value operator member have it
    for t in [k for k in PC_KINDS if k != "ApproxInv"]:
        lines.append(f'static_assert(std::is_move_assignable<{t}>::value, "{t} is not move-assignable");')
    lines.append("BlockJacobi by_value() { return BlockJacobi::uniform(8); }")
    lines.append("int main() { return 0; }")
    return "\n".join(lines) + "\n"


def test_handle_owners_are_move_only(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to check the header")
    src = tmp_path / "move_only.cpp"
    src.write_text(unit())
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
