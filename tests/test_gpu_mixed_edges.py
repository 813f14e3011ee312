"""The fp32 path at window edges, with dirty padding and at the ends of the fp32 range, against the numpy restatement of the contract
(tests/mixed_ref.py).  The rule of tests/test_gpu_mixed.py holds: everything is compared bit for bit on integer views, no tolerance.  One
exception, where a NaN can arise (the overflow and non-finite cases of part d): there `nonfinite_cases.same_ieee` -- NaNs at the same
positions, every other value the same in all bits; sign and payload of a NaN made by inf - inf differ between host and device and the
contract does not define them.  Fixtures: tests/mixed_edge_cases.py (their properties are asserted in tests/test_mixed_edges_cpu.py).

a. spmv32 on every general operator, into a NaN-filled y          d. fp32 subnormals, flushes, overflow, inf / NaN / -0.0 in whole solves
b. the fused (p, Ap) partial on ragged SPD operators               e. more tiles than workgroups, on an operator whose tiles differ
c. every operand with poisoned padding                             f. the C++ mirror"""
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import mixed_cases as MC
import mixed_edge_cases as E
import mixed_ref as R
from nonfinite_cases import same_ieee

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
b32, b64 = MC.bits32, MC.bits64
UNPRE, PRE = K.CgNormType.Unpreconditioned, K.CgNormType.Preconditioned
POISONS32 = [None, np.float32(3e38)]               # the quiet NaN 0x7FC00000, and a finite value
POISONS64 = [None, 1e300]


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec32() == R.SPEC32
    return K.Context(0)


def upload(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def same32(a, b):
    return a.shape == b.shape and np.array_equal(b32(a), b32(b))


def same64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(b64(a), b64(b))


def nan_filled(ctx, n):
    return K.DeviceVec32(ctx, np.full(n, np.nan, np.float32))


def poisoned32(v, value):
    """the fp32 vector with its padding set to `value` -- and the proof that the hook did something"""
    n = len(v)
    assert v.padding_dirty() == 0
    v.poison_padding(value)
    assert v.padding_dirty() == -(-n // 1024) * 1024 + 1024 - n, (n, v.padding_dirty())
    return v


def poisoned64(v, value):
    n = len(v)
    assert v.padding_dirty() == 0
    v.poison_padding(value)
    assert v.padding_dirty() == -(-n // 512) * 512 + 512 - n, (n, v.padding_dirty())
    return v


def run32(solver, d32, pc, b, x0, same_vector=False, poison=False, value=None):
    """-> (code, stats, history, x after the call, b after the call)"""
    ctx = d32.ctx
    bv = K.DeviceVec32(ctx, b)
    xv = bv if same_vector else K.DeviceVec32(ctx, x0)
    if poison:
        poisoned32(bv, value)
        if not same_vector:
            poisoned32(xv, value)
    solver.clear_history()
    try:
        stats, code = solver.solve(d32, pc, bv, xv), 0
    except K.KError as e:
        if e.stats is None:
            raise
        stats, code = e.stats, e.code
    return code, stats, list(solver.residual_history), xv.to_host(), bv.to_host()


def assert_solve(got, ref, what, nan_can_arise=False):
    code, stats, hist, x = got[:4]
    assert code == ref.code, (what, code, ref.code)
    assert (stats.iterations, stats.converged) == (ref.iterations, ref.converged), (what, stats, ref.iterations, ref.converged)
    if nan_can_arise:
        assert same_ieee([stats.final_residual], [ref.final_residual]), (what, stats.final_residual, ref.final_residual)
        assert same_ieee(hist, ref.history), (what, hist, ref.history)
        assert same_ieee(x, ref.x), (what, int(np.sum(b32(x) != b32(ref.x))))
    else:
        assert same64([stats.final_residual], [ref.final_residual]), (what, stats.final_residual, ref.final_residual)
        assert same64(hist, ref.history), (what, len(hist), len(ref.history))
        assert same32(x, ref.x), (what, int(np.sum(b32(x) != b32(ref.x))))


def assert_same_run(got, clean, what):
    """a run on poisoned vectors against the same call on clean ones"""
    assert got[0] == clean[0] and (got[1].iterations, got[1].converged) == (clean[1].iterations, clean[1].converged), what
    assert same64([got[1].final_residual], [clean[1].final_residual]) and same64(got[2], clean[2]) and same32(got[3], clean[3]), what


# ------------------------------------------------------------------------------------------------------------- a. spmv32
@pytest.mark.parametrize("name", list(E.GENERAL_OPERATORS))
def test_spmv32_on_window_edges(ctx, name):
    a = E.GENERAL_OPERATORS[name]()
    ref = R.Lowered(a)
    d32 = upload(ctx, a).lower()
    assert d32.info == ref.info
    for operand in (MC.vec32, MC.special32):
        x = operand(a.ncols)
        want = ref.spmv(x)
        xv = K.DeviceVec32(ctx, x)
        y = nan_filled(ctx, a.nrows)                                            # every row must be stored, an empty one as +0.0
        d32.spmv(xv, y)
        got = y.to_host()
        assert same32(got, want), (name, operand.__name__, int(np.sum(b32(got) != b32(want))), np.flatnonzero(b32(got) != b32(want))[:8])
        assert y.padding_dirty() == 0                                           # ... and nothing behind the last row
        yp = poisoned32(nan_filled(ctx, a.nrows), None)
        d32.spmv(xv, yp)
        assert same32(yp.to_host(), want), (name, operand.__name__, "y poisoned")        # (what the padding holds now is unspecified)
    if a.nnz == 0:
        assert not b32(want).any()                                              # +0.0, the sign included


# ------------------------------------------------------------------------------------------------------------- b. the fused partial
@pytest.mark.parametrize("name", list(E.SPD_OPERATORS))
def test_fused_partial_on_ragged_operators(ctx, name):
    a = E.SPD_OPERATORS[name]()
    n = a.nrows
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    pc, inv = K.Jacobi().setup(d), O.Pc.jacobi(a).inv_diag
    b = R.store(MC.rhs(n))
    zero = np.zeros(n, np.float32)
    for start, x0 in (("zero", zero), ("guess", MC.vec32(n, seed=5))):
        for cap in (1, 2, 7):                                                   # tolerance 1e-30: a fixed number of iterations
            ref = R.cg32(ref32, b, x0, 1e-30, cap)
            assert ref.code == R.OK and ref.iterations == cap
            assert_solve(run32(K.Cg32Solver(1e-30, cap), d32, None, b, x0), ref, (name, start, cap, "cg32"))
            for nt in (UNPRE, PRE):
                ref = R.pcg32(ref32, inv, b, x0, 1e-30, cap, int(nt))
                assert ref.code == R.OK and ref.iterations == cap
                assert_solve(run32(K.Pcg32Solver(1e-30, cap).with_norm(nt), d32, pc, b, x0), ref, (name, start, cap, "pcg32", nt))
    ref = R.cg32(ref32, b, zero, 1e-5, 400)
    assert ref.code == R.OK and 5 < ref.iterations < 400
    assert_solve(run32(K.Cg32Solver(1e-5, 400), d32, None, b, zero), ref, (name, "cg32 to 1e-5"))
    ref = R.pcg32(ref32, inv, b, zero, 1e-5, 400, int(UNPRE))
    assert ref.code == R.OK and 2 < ref.iterations < 400
    assert_solve(run32(K.Pcg32Solver(1e-5, 400), d32, pc, b, zero), ref, (name, "pcg32 to 1e-5"))


# ------------------------------------------------------------------------------------------------------------- c. dirty padding
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3077])
def test_dot32_with_poisoned_padding(ctx, n):
    x, y = MC.vec32(n, seed=n), MC.vec32(n, seed=n + 1)
    clean = (K.dot32(K.DeviceVec32(ctx, x), K.DeviceVec32(ctx, y)), K.dot32(K.DeviceVec32(ctx, x), K.DeviceVec32(ctx, x)))
    assert same64(clean, [R.dot32(x, y), R.dot32(x, x)])
    for value in POISONS32:
        xv, yv = poisoned32(K.DeviceVec32(ctx, x), value), poisoned32(K.DeviceVec32(ctx, y), value)
        assert same64([K.dot32(xv, yv), K.dot32(xv, xv)], clean), (n, value)
        assert same32(xv.to_host(), x) and same32(yv.to_host(), y)


PADDING_SPMV = {"holes": E.holes, "partial_last_quad1": lambda: E.partial_last_quad(1), "partial_last_quad2": lambda: E.partial_last_quad(2),
                "partial_last_quad3": lambda: E.partial_last_quad(3), "banded1025": MC.banded1025}


@pytest.mark.parametrize("name", list(PADDING_SPMV))
def test_spmv32_with_poisoned_padding(ctx, name):
    a = PADDING_SPMV[name]()
    ref, d32 = R.Lowered(a), upload(ctx, a).lower()
    x = MC.vec32(a.ncols)
    want = ref.spmv(x)
    assert same32(d32.spmv(K.DeviceVec32(ctx, x), nan_filled(ctx, a.nrows)).to_host(), want)
    for value in POISONS32:
        xv, yv = poisoned32(K.DeviceVec32(ctx, x), value), poisoned32(nan_filled(ctx, a.nrows), value)
        d32.spmv(xv, yv)
        assert same32(yv.to_host(), want) and same32(xv.to_host(), x), (name, value)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3077])
def test_conversions_with_poisoned_padding(ctx, n):
    d = MC.rhs(n, seed=n) * np.exp(np.random.default_rng(n).uniform(-100, 100, n))       # overflows, underflows and subnormals in fp32
    x = MC.special32(n) if n > 8 else MC.vec32(n)
    for p32, p64 in zip(POISONS32, POISONS64):
        src = poisoned64(ctx.vec(d), p64)
        dst = poisoned32(nan_filled(ctx, n), p32)
        assert same32(K.DeviceVec32.from_f64(src, dst).to_host(), R.store(d)) and same64(src.to_host(), d)
        src = poisoned32(K.DeviceVec32(ctx, x), p32)
        dst = poisoned64(ctx.vec(np.full(n, np.nan)), p64)
        w = src.to_f64(dst).to_host()
        finite = ~np.isnan(x)
        assert same64(w[finite], x.astype(np.float64)[finite]) and np.array_equal(np.isnan(w), np.isnan(x)) and same32(src.to_host(), x)


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_solves_with_poisoned_padding(ctx, n):
    a = E.thinned_band(n)
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    inv = O.Pc.jacobi(a).inv_diag
    b, x0 = R.store(MC.rhs(n)), MC.vec32(n, seed=5)
    tol, cap = 1e-5, 200
    cases = [("cg32", lambda: K.Cg32Solver(tol, cap), None, lambda xs: R.cg32(ref32, b, xs, tol, cap)),
             ("pcg32 none", lambda: K.Pcg32Solver(tol, cap), None, lambda xs: R.pcg32(ref32, None, b, xs, tol, cap, 1)),
             ("pcg32 identity", lambda: K.Pcg32Solver(tol, cap), K.IdentityPc().setup(d), lambda xs: R.pcg32(ref32, None, b, xs, tol, cap, 1)),
             ("pcg32 jacobi", lambda: K.Pcg32Solver(tol, cap), K.Jacobi().setup(d), lambda xs: R.pcg32(ref32, inv, b, xs, tol, cap, 1)),
             ("pcg32 jacobi, preconditioned norm", lambda: K.Pcg32Solver(tol, cap).with_norm(PRE), K.Jacobi().setup(d),
              lambda xs: R.pcg32(ref32, inv, b, xs, tol, cap, 0))]
    for what, make, pc, restate in cases:
        for same_vector in (False, True):
            ref = restate(b if same_vector else x0)
            assert ref.code == R.OK and ref.iterations > 3
            clean = run32(make(), d32, pc, b, x0, same_vector)
            assert_solve(clean, ref, (n, what, same_vector, "clean"))
            for value in POISONS32:
                got = run32(make(), d32, pc, b, x0, same_vector, poison=True, value=value)
                assert_solve(got, ref, (n, what, same_vector, value))
                assert_same_run(got, clean, (n, what, same_vector, value))
                assert same_vector or same32(got[4], b), (n, what, value, "b was written")


def test_refinement_with_poisoned_padding(ctx):
    a = MC.poisson12()
    d = upload(ctx, a)
    b, x0 = MC.rhs(a.nrows), MC.rhs(a.nrows, seed=9)
    ref = R.refine(a, R.Lowered(a), None, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.code == R.OK and ref.converged and ref.iterations >= 2
    for value in [False] + POISONS64:
        bv, xv = ctx.vec(b), ctx.vec(x0)
        if value is not False:
            poisoned64(bv, value); poisoned64(xv, value)
        s = K.RefinementSolver(MC.OUTER_TOL, MC.OUTER_CAP).with_inner(MC.INNER_TOL, MC.INNER_CAP)
        stats = s.solve(d, None, bv, xv)
        assert (stats.iterations, stats.converged, stats.inner_iterations) == (ref.iterations, ref.converged, ref.inner_iterations), value
        assert same64([stats.final_residual], [ref.final_residual]) and same64(s.residual_history, ref.history), value
        assert same64(xv.to_host(), ref.x) and same64(bv.to_host(), b), value


# ------------------------------------------------------------------------------------------------------------- d. the ends of the fp32 range
def both_solvers(ctx, a, b, x0, what, nan_can_arise, cap=E.RANGE_CAP):
    """CG32 and Jacobi-PCG32 for exactly `cap` iterations unless the restatement leaves earlier; -> the two restated results"""
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    assert d32.info == ref32.info
    ref = R.cg32(ref32, b, x0, 1e-30, cap)
    assert_solve(run32(K.Cg32Solver(1e-30, cap), d32, None, b, x0), ref, (what, "cg32"), nan_can_arise)
    refp = R.pcg32(ref32, O.Pc.jacobi(a).inv_diag, b, x0, 1e-30, cap, 1)
    assert_solve(run32(K.Pcg32Solver(1e-30, cap), d32, K.Jacobi().setup(d), b, x0), refp, (what, "pcg32 jacobi"), nan_can_arise)
    return ref, refp


def test_whole_solves_at_the_ends_of_the_fp32_range(ctx):
    a = MC.poisson12()
    n = a.nrows
    zero = np.zeros(n, np.float32)
    for case, e in E.RANGE_EXPONENTS.items():
        b = R.store(MC.rhs(n) * 2.0 ** e)
        overflow = case == "overflow"                                            # (the conditions on these inputs: tests/test_mixed_edges_cpu.py)
        ref, refp = both_solvers(ctx, a, b, zero, case, nan_can_arise=overflow)
        assert (ref.code, ref.iterations, ref.converged) == (R.OK, E.RANGE_CAP, True) and np.isnan(ref.x).all() == overflow, case
        assert refp.iterations >= 1                                              # (Jacobi's p = r / 6 keeps the first Ap below the overflow)
    # one +inf, one NaN in b
    for bad in (np.inf, np.nan):
        b = R.store(MC.rhs(n))
        b[n // 3] = bad
        both_solvers(ctx, a, b, zero, ("b holds", bad), nan_can_arise=True)
    # signed zeros through every pass: x0 = -0.0 everywhere, b = 0
    ref, refp = both_solvers(ctx, a, zero, np.full(n, -0.0, np.float32), "signed zeros", nan_can_arise=True)
    assert np.signbit(ref.x).all() and np.signbit(refp.x).all()
    # one stored +inf (the lowering accepts it), off the diagonal
    vals = a.vals.copy()
    k = int(a.row_ptr[n // 2])
    assert a.col_idx[k] != n // 2
    vals[k] = np.inf
    both_solvers(ctx, O.Csr(n, n, a.row_ptr, a.col_idx, vals), R.store(MC.rhs(n)), zero, "a stored +inf", nan_can_arise=True)


# ------------------------------------------------------------------------------------------------------------- e. more tiles than workgroups
def test_tile_stride_loops_on_an_operator_whose_tiles_differ(ctx, monkeypatch):
    monkeypatch.setenv("KRYST_SPMV32_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("KRYST_EW32_BLOCKS_PER_CU", "1")
    a = E.thinned_band(E.BIG_BAND_ROWS)
    n = a.nrows
    assert (n + 1023) // 1024 == 264          # more than one workgroup per compute unit of a 256-CU device: every loop takes a second trip somewhere
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    x = MC.vec32(n)
    y = nan_filled(ctx, n)
    d32.spmv(K.DeviceVec32(ctx, x), y)
    want = ref32.spmv(x)
    assert same32(y.to_host(), want), int(np.sum(b32(y.to_host()) != b32(want)))
    assert same64([K.dot32(K.DeviceVec32(ctx, x), y)], [R.dot32(x, want)])
    b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
    ref = R.cg32(ref32, b, zero, 1e-30, 3)
    assert ref.iterations == 3
    assert_solve(run32(K.Cg32Solver(1e-30, 3), d32, None, b, zero), ref, "cg32")
    ref = R.pcg32(ref32, O.Pc.jacobi(a).inv_diag, b, zero, 1e-30, 3, 1)
    assert ref.iterations == 3
    assert_solve(run32(K.Pcg32Solver(1e-30, 3), d32, K.Jacobi().setup(d), b, zero), ref, "pcg32 jacobi")


# ------------------------------------------------------------------------------------------------------------- f. the C++ mirror
def test_cpp_mixed_mirror():
    """tests/cpp/test_mixed_mirror.cpp: HipCsrMatrix32 and RefinementSolver of include/kryst_hip.hpp on the reference's 2 x 2 case
    (cg.rs:310-323) and a 64-row tridiagonal operator."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_mixed_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_MIXED_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
