"""Block CG, the CPU tier: the numpy restatement (tests/block_cg_ref.py) against a plain numpy.linalg implementation and against what it must
deliver, on the fixtures of the GPU tier (tests/block_cg_cases.py); the library's scalar step on the host (kryst_host_bcg_step) against the
restatement's, bit for bit; the new symbols; and the scalar step as a stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
import block_cg_cases as BC
import block_cg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, k, pc) for name in BC.NAMES for k in BC.WIDTHS for pc in (None, "jacobi")]
bits = BC.bits


@pytest.mark.parametrize("name,k,pc", CASES)
def test_restatement_against_the_plain_implementation(name, k, pc):
    a, b = BC.operator(name), BC.rhs(name)[:, :k]
    ref = BC.reference(name, k, pc)
    assert ref.status == 0 and all(ref.converged) and ref.iterations < BC.CAP
    its, x, res = R.solve_plain(a, b, d=BC.weights(name, pc), tol=BC.TOL, max_iters=BC.CAP)
    assert its == ref.iterations, (its, ref.iterations)
    for j in range(k):
        assert np.linalg.norm(ref.x[:, j] - x[:, j]) <= 1e-10 * np.linalg.norm(x[:, j]), (name, k, pc, j)
    assert np.allclose(res, ref.final_residual, rtol=1e-6)
    assert all(len(h) == ref.iterations + 1 for h in ref.history) and [h[-1] for h in ref.history] == ref.final_residual


@pytest.mark.parametrize("name,k,pc", CASES)
def test_true_residual_of_the_restatement(name, k, pc):
    """||b_j - A x_j||_2 <= 1.001 * tol * sqrt(max d / min d) * ||b_j - A x0_j||_2: the square root is the gap between the M^-1 norm the
    iteration watches and the 2-norm (1 without Jacobi), the 1.001 room for the drift of the recurrence (near 1e-13)"""
    a, b = BC.operator(name), BC.rhs(name)[:, :k]
    ref = BC.reference(name, k, pc)
    d = BC.weights(name, pc)
    gap = 1.0 if d is None else float(np.sqrt(d.max() / d.min()))
    true = np.linalg.norm(b - R.spmm(a, ref.x), axis=0)
    start = np.linalg.norm(b, axis=0)                                          # x0 = 0
    for j in range(k):
        assert true[j] <= 1.001 * BC.TOL * gap * start[j], (name, k, pc, j, true[j] / start[j])


@pytest.mark.parametrize("name,k,pc", CASES)
def test_pivot_margin_and_iteration_counts(name, k, pc):
    ref = BC.reference(name, k, pc)
    assert ref.margin >= 0.05, ref.margin                                       # a healthy run stays far from KRYST_BCG_RANK_TOL = 2^-26
    single = BC.single_counts(name, k, pc)
    assert ref.iterations <= max(single), (ref.iterations, single)             # one shared Krylov space never costs more iterations


def test_variants_of_the_restatement():
    """what the GPU tier also runs: x0 != 0, x0 = b, caps; a cap reports converged = true as Convergence::check does"""
    name, k = "poisson9", 4
    full = BC.reference(name, k, None)
    for cap in (0, 1, 2, 5):
        r = BC.reference(name, k, None, max_iters=cap)
        assert r.status == 0 and r.iterations == cap and all(len(h) == cap + 1 for h in r.history)
        assert r.converged == ([True] * k if cap else [False] * k)
        assert all(h == f[:cap + 1] for h, f in zip(r.history, full.history))
    g = BC.reference(name, k, "jacobi", guess=True)
    al = BC.reference(name, k, None, alias=True)
    assert g.status == 0 and al.status == 0 and all(g.converged) and all(al.converged)
    assert g.margin >= 0.05 and al.margin >= 0.05


@pytest.mark.parametrize("name", list(BC.breakdown_cases()))
def test_each_way_of_ending_on_the_restatement(name):
    a, b, jac, status, it = BC.breakdown_cases()[name]
    g, ref = BC.breakdown_reference(name)
    assert (ref.status, ref.iterations) == (status, it), (ref.status, ref.iterations)
    assert np.array_equal(bits(ref.x), bits(g)) and ref.converged == [False] * b.shape[1]
    assert all(len(h) == (1 if it else 0) for h in ref.history)


# ---------------------------------------------------------------------------------------------------------------- the scalar step on the host
def as_array(m):
    return np.array(m, dtype=np.float64)


def compare_step(kind, g, c=None):
    want = R.step(kind, g, c)
    code, cc, o1, o2, res = K.host_bcg_step(kind, g, c)
    assert code == want.code, (kind, code, want.code)
    if code:
        return code
    if kind == R.STEP_INIT:
        pairs = [(cc, want.c), (o1, want.out1), (res, want.res)]
    elif kind == R.STEP_ALPHA:
        pairs = [(o1, want.out1), (o2, want.out2), (cc, want.c)]
    else:
        pairs = [(cc, want.c), (o1, want.out1), (o2, want.out2), (res, want.res)]
    for got, ref in pairs:
        assert np.array_equal(bits(got), bits(as_array(ref))), (kind, got, ref)
    return 0


def spd(k, gen, scale=1.0):
    m = gen.standard_normal((k + 3, k)) * scale
    return m.T @ m


@pytest.mark.parametrize("k", BC.WIDTHS)
def test_host_step_equals_the_restatement_bit_for_bit(k):
    gen = np.random.default_rng(40 + k)
    for rep in range(20):
        scales = 10.0 ** gen.integers(-6, 7, k) if rep % 2 else np.ones(k)    # columns that differ in scale by 1e+-6
        g0 = spd(k, gen) * np.outer(scales, scales)
        assert compare_step(R.STEP_INIT, g0) == 0
        c = as_array(R.step(R.STEP_INIT, g0).c)
        assert compare_step(R.STEP_ALPHA, spd(k, gen), c) == 0
        assert compare_step(R.STEP_BETA, spd(k, gen, 0.3), c) == 0
    # Gram matrices of a real run
    name = "varcoef12"
    a, b, d = BC.operator(name), BC.rhs(name)[:, :k], BC.inv_diag(name)
    g = R.gram(b, b, d)
    assert compare_step(R.STEP_INIT, g) == 0
    st = R.step(R.STEP_INIT, g)
    q = R.row_product(b, st.out1, hi=lambda j: j)
    s = d[:, None] * q
    assert compare_step(R.STEP_ALPHA, R.gram(s, R.spmm(a, s)), as_array(st.c)) == 0


@pytest.mark.parametrize("k", BC.WIDTHS)
def test_host_step_breakdowns(k):
    gen = np.random.default_rng(50 + k)
    c = as_array(R.step(R.STEP_INIT, spd(k, gen)).c)
    dep = spd(k, gen); dep[:, k - 1] = dep[:, 0]; dep[k - 1, :] = dep[0, :]; dep[k - 1, k - 1] = dep[0, 0]      # an exactly dependent pair
    assert compare_step(R.STEP_INIT, dep) == R.SOLVE_ERROR and compare_step(R.STEP_BETA, dep, c) == R.SOLVE_ERROR
    zero = spd(k, gen); zero[:, 1] = 0.0; zero[1, :] = 0.0                                                        # a zero column
    assert compare_step(R.STEP_INIT, zero) == R.SOLVE_ERROR and compare_step(R.STEP_ALPHA, zero, c) == R.INDEFINITE_MATRIX
    assert compare_step(R.STEP_ALPHA, -spd(k, gen), c) == R.INDEFINITE_MATRIX                                     # an indefinite Gram matrix
    ind = spd(k, gen); ind[k - 1, k - 1] = -ind[k - 1, k - 1]
    assert compare_step(R.STEP_ALPHA, ind, c) == R.INDEFINITE_MATRIX
    nan = spd(k, gen); nan[0, k - 1] = np.nan
    assert compare_step(R.STEP_ALPHA, nan, c) == R.INDEFINITE_MATRIX
    neg = spd(k, gen); neg[k - 1, k - 1] = -1.0                                                                   # a negative weighted diagonal
    assert compare_step(R.STEP_INIT, neg) == R.INDEFINITE_PC and compare_step(R.STEP_BETA, neg, c) == R.INDEFINITE_PC
    nearly = spd(k, gen); nearly[:, k - 1] = nearly[:, 0] * (1.0 + 1e-9); nearly[k - 1, :] = nearly[:, k - 1]
    nearly[k - 1, k - 1] = nearly[0, 0] * (1.0 + 1e-9) ** 2                                                      # dependent to 1e-9: below 2^-26
    assert compare_step(R.STEP_INIT, nearly) == R.SOLVE_ERROR
    lib = K.lib()
    z = np.zeros(64)
    p = z.ctypes.data_as(_ffi.c_dp)
    assert lib.kryst_host_bcg_step(3, 4, p, p, p, p, p) == 102 and lib.kryst_host_bcg_step(0, 3, p, p, p, p, p) == 102
    assert lib.kryst_host_bcg_step(0, 4, None, p, p, p, p) == 102


# ---------------------------------------------------------------------------------------------------------------- the interface
NEW_SYMBOLS = ("kryst_bcg_solve_multi_dev", "kryst_bcg_solve_multi", "kryst_host_bcg_step", "kryst_bench_mvec_gram")


def test_new_symbols_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "kryst_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib = K.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint32_t\s+" + s + r"\s*\(", header), s
        assert re.search(r"\bpub fn " + s + r"\s*\(", rust), s
        assert s in _ffi.SIGNATURES, s
        assert getattr(lib, s) is not None                                      # (an AttributeError here: the library does not export it)
    assert re.search(r"^#define KRYST_BCG_RANK_TOL 0x1p-26\b", header, re.M) and R.RANK_TOL == float.fromhex("0x1p-26")
    assert hasattr(K, "BlockCgSolver") and hasattr(K.BlockCgSolver, "solve_block")
    logic = open(os.path.join(ROOT, "kryst_amd", "csrc", "bcg_logic.h")).read()
    assert "#define KRYST_BCG_RANK_TOL" not in logic and "KRYST_BCG_RANK_TOL * gjj" in logic       # one definition, in the public header


def test_scalar_step_under_the_sanitizers(tmp_path):
    """tests/cpp/test_bcg_logic_san.cpp: bcg_logic.h's host side and a small main, built with AddressSanitizer and UBSan and run directly"""
    exe = str(tmp_path / "test_bcg_logic_san")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                         os.path.join(ROOT, "tests", "cpp", "test_bcg_logic_san.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "bcg logic ok" in r.stdout, r.stdout[-2000:]
