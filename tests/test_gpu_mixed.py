"""Mixed precision on the GPU: fp32-stored vectors and operator, CG32 / PCG32 and the fp64 iterative refinement, against the numpy
restatement of the contract (tests/mixed_ref.py).  One rule, no tolerance: everything -- y, x, every residual-history entry, iteration
counts, final_residual, converged, the status -- is compared bit for bit on integer views.  Fixtures: tests/mixed_cases.py (their behaviour
under the restatement alone is asserted in tests/test_mixed_cpu.py)."""
import os

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import mixed_cases as MC
import mixed_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG, UNSUPPORTED = 102, 6
b32, b64 = MC.bits32, MC.bits64


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec32() == R.SPEC32 and K.reduce_spec() == (256, 2, 1024)
    return K.Context(0)


def upload(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def same32(a, b):
    return a.shape == b.shape and np.array_equal(b32(a), b32(b))


def same64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(b64(a), b64(b))


# ------------------------------------------------------------------------------------------------------------- 1. vectors and dot32
SIZES = [1, 1023, 1024, 1025, 3 * 1024 + 5]


@pytest.mark.parametrize("n", SIZES)
def test_vector_round_trips(ctx, n):
    x = MC.special32(n) if n > 8 else MC.vec32(n)
    v = K.DeviceVec32(ctx, x)
    assert same32(v.to_host(), x)                                                # upload / download move the bits
    w = v.to_f64().to_host()
    assert same64(w[~np.isnan(x)], x.astype(np.float64)[~np.isnan(x)]) and np.array_equal(np.isnan(w), np.isnan(x))
    d = MC.rhs(n, seed=n) * np.exp(np.random.default_rng(n).uniform(-100, 100, n))          # overflows, underflows and subnormals in fp32
    r = K.DeviceVec32.from_f64(ctx.vec(d)).to_host()
    assert same32(r, R.store(d))
    assert same32(K.DeviceVec32.from_f64(v.to_f64()).to_host()[~np.isnan(x)], x[~np.isnan(x)])


@pytest.mark.parametrize("n", SIZES + [1024 * R.SPEC32[2] + 1025])
def test_dot32(ctx, n):
    x, y = MC.vec32(n, seed=n), MC.vec32(n, seed=n + 1)
    xv, yv = K.DeviceVec32(ctx, x), K.DeviceVec32(ctx, y)
    assert same64([K.dot32(xv, yv)], [R.dot32(x, y)])
    assert same64([K.dot32(xv, xv)], [R.dot32(x, x)])


def test_dot32_with_special_values(ctx):
    n = 2500
    x = MC.special32(n)
    y = MC.vec32(n, seed=2)
    for u, v in ((x, y), (np.where(np.isnan(x), np.float32(1e-41), x), y), (np.full(n, 1e-30, np.float32), np.full(n, 1e-30, np.float32))):
        assert same64([K.dot32(K.DeviceVec32(ctx, u), K.DeviceVec32(ctx, v))], [R.dot32(u, v)])
    with pytest.raises(K.KError) as e:
        K.dot32(K.DeviceVec32(ctx, 5), K.DeviceVec32(ctx, 6))
    assert e.value.code == ERR_ARG


# ------------------------------------------------------------------------------------------------------------- 2. lowering and spmv32
@pytest.mark.parametrize("name", list(MC.SPMV_OPERATORS))
def test_spmv32(ctx, name):
    a = MC.SPMV_OPERATORS[name]()
    ref = R.Lowered(a)
    d32 = upload(ctx, a).lower()
    assert d32.info == ref.info
    assert (d32.nrows(), d32.ncols()) == (a.nrows, a.ncols)
    for x in (MC.vec32(a.ncols), MC.special32(a.ncols)):
        y = d32.spmv(K.DeviceVec32(ctx, x)).to_host()
        want = ref.spmv(x)
        assert same32(y, want), (name, int(np.sum(b32(y) != b32(want))))
        full = K.DeviceVec32(ctx, np.full(a.nrows, np.nan, np.float32))          # every row is stored, the empty ones as +0.0
        y = d32.spmv(K.DeviceVec32(ctx, x), full).to_host()
        assert same32(y, want), (name, "into a NaN-filled y", int(np.sum(b32(y) != b32(want))))
    assert same32(d32.spmv(MC.vec32(a.ncols)), ref.spmv(MC.vec32(a.ncols)))       # host arrays round-trip


def test_spmv32_products_on_fp32_subnormals(ctx):
    a = MC.tiny_products()
    ref = R.Lowered(a)
    d32 = upload(ctx, a).lower()
    assert d32.info == ref.info
    x = (MC.vec32(a.ncols) * np.float32(1e-20)).astype(np.float32)
    y = d32.spmv(K.DeviceVec32(ctx, x)).to_host()
    tiny = np.finfo(np.float32).tiny
    assert same32(y, ref.spmv(x)) and np.count_nonzero((y != 0) & (np.abs(y) < tiny)) > a.nrows // 2      # subnormals are kept
    # values that leave the fp32 range of normal numbers when they are lowered
    small = O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals * 1e-20)
    d_small = upload(ctx, small).lower()
    assert d_small.info == R.Lowered(small).info and d_small.info["tiny"] == small.nnz


def test_spmv32_leaves_its_source_alone_and_refuses_bad_operands(ctx):
    a = MC.banded1025()
    d = upload(ctx, a)
    d32 = d.lower()
    x = MC.vec32(a.ncols)
    want = d32.spmv(K.DeviceVec32(ctx, x)).to_host()
    x64 = MC.rhs(a.ncols)
    y64 = d.spmv(ctx.vec(x64)).to_host()
    del d                                                                      # no lifetime tie to the fp64 operator
    assert same32(d32.spmv(K.DeviceVec32(ctx, x)).to_host(), want) and same64(y64, a.spmv(x64))
    xv = K.DeviceVec32(ctx, x)
    for bad_x, bad_y in ((xv, xv), (K.DeviceVec32(ctx, 7), K.DeviceVec32(ctx, a.nrows)), (xv, K.DeviceVec32(ctx, 7))):
        with pytest.raises(K.KError) as e:
            d32.spmv(bad_x, bad_y)
        assert e.value.code == ERR_ARG
    assert same32(xv.to_host(), x)


def test_lower_refusals(ctx):
    a = MC.banded1025()
    # a row-partitioned operator, made on this one rank
    dd = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)
    with pytest.raises(K.KError) as e:
        dd.lower()
    assert e.value.code == UNSUPPORTED
    vals = a.vals.copy()
    vals[17] = -1e39
    with pytest.raises(K.KError) as e:
        K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals, ctx=ctx).lower()
    assert e.value.code == UNSUPPORTED
    vals[17] = np.inf                                                          # an infinity is not an overflow
    assert K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals, ctx=ctx).lower().info == R.Lowered(O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals)).info


# ------------------------------------------------------------------------------------------------------------- 3. CG32 / PCG32
def run32(solver, d32, pc, b, x0, same_vector=False):
    """-> (code, stats, history, x after the call)"""
    bv = K.DeviceVec32(d32.ctx, b)
    xv = bv if same_vector else K.DeviceVec32(d32.ctx, x0)
    solver.clear_history()
    try:
        stats, code = solver.solve(d32, pc, bv, xv), 0
    except K.KError as e:
        if e.stats is None:
            raise
        stats, code = e.stats, e.code
    return code, stats, list(solver.residual_history), xv.to_host()


def assert_solve(got, ref, what):
    code, stats, hist, x = got
    assert code == ref.code, (what, code, ref.code)
    assert (stats.iterations, stats.converged) == (ref.iterations, ref.converged), (what, stats, ref.iterations, ref.converged)
    assert same64([stats.final_residual], [ref.final_residual]), what
    assert same64(hist, ref.history), (what, len(hist), len(ref.history))
    assert same32(x, ref.x), (what, int(np.sum(b32(x) != b32(ref.x))))


@pytest.mark.parametrize("name", list(MC.REFINE_CASES))
@pytest.mark.parametrize("start", ["zero", "guess", "b_is_x"])
def test_cg32_and_pcg32(ctx, name, start):
    make, jacobi = MC.REFINE_CASES[name]
    a = make()
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    b = R.store(MC.rhs(a.nrows))
    x0 = {"zero": np.zeros(a.nrows, np.float32), "guess": MC.vec32(a.nrows, seed=5), "b_is_x": b}[start]
    tol, cap = 1e-5, 400
    if jacobi:
        pc = K.Jacobi().setup(d)
        for nt in (K.CgNormType.Unpreconditioned, K.CgNormType.Preconditioned):
            ref = R.pcg32(ref32, O.Pc.jacobi(a).inv_diag, b, x0, tol, cap, int(nt))
            assert ref.code == 0 and 5 < ref.iterations < cap
            assert_solve(run32(K.Pcg32Solver(tol, cap).with_norm(nt), d32, pc, b, x0, start == "b_is_x"), ref, (name, start, nt))
        ref = R.pcg32(ref32, None, b, x0, tol, cap, 1)
        for none in (None, K.IdentityPc().setup(d)):
            assert_solve(run32(K.Pcg32Solver(tol, cap), d32, none, b, x0, start == "b_is_x"), ref, (name, start, "identity"))
    else:
        ref = R.cg32(ref32, b, x0, tol, cap)
        assert ref.code == 0 and 5 < ref.iterations < cap
        assert_solve(run32(K.Cg32Solver(tol, cap), d32, None, b, x0, start == "b_is_x"), ref, (name, start))
        assert_solve(run32(K.Cg32Solver(tol, cap), d32, K.Jacobi().setup(d), b, x0, start == "b_is_x"), ref, (name, start, "pc ignored"))


def test_solve32_cap_zero_iterations_and_host_arrays(ctx):
    a = MC.poisson12()
    d32, ref32 = upload(ctx, a).lower(), R.Lowered(a)
    b, x0 = R.store(MC.rhs(a.nrows)), MC.vec32(a.nrows, seed=5)
    for cap in (0, 1, 7):
        ref = R.cg32(ref32, b, x0, 1e-12, cap)
        assert ref.iterations == cap and ref.converged == (cap > 0)               # the cap reports converged (convergence.rs:18-34)
        assert_solve(run32(K.Cg32Solver(1e-12, cap), d32, None, b, x0), ref, cap)
        refp = R.pcg32(ref32, None, b, x0, 1e-12, cap, 0)
        assert_solve(run32(K.Pcg32Solver(1e-12, cap).with_norm(K.CgNormType.Preconditioned), d32, None, b, x0), refp, cap)
    x = x0.copy()
    s = K.Cg32Solver(1e-12, 7)
    stats = s.solve(d32, None, b, x)
    assert stats.iterations == 7 and same32(x, R.cg32(ref32, b, x0, 1e-12, 7).x)


def test_solve32_indefinite_matrix_and_zero_diagonal(ctx):
    a = MC.indefinite()
    d = upload(ctx, a)
    d32, ref32 = d.lower(), R.Lowered(a)
    b = np.zeros(a.nrows, np.float32)
    b[1] = 1.0
    x0 = np.zeros(a.nrows, np.float32)
    ref = R.cg32(ref32, b, x0, 1e-8, 50)
    assert ref.code == R.INDEFINITE_MATRIX and ref.iterations == 1
    assert_solve(run32(K.Cg32Solver(1e-8, 50), d32, None, b, x0), ref, "cg32 indefinite")
    refp = R.pcg32(ref32, None, b, x0, 1e-8, 50)
    assert refp.code == R.INDEFINITE_MATRIX
    assert_solve(run32(K.Pcg32Solver(1e-8, 50), d32, None, b, x0), refp, "pcg32 indefinite")
    # later in the solve: a start that is not an eigenvector
    b2 = R.store(MC.rhs(a.nrows, seed=3))
    ref2 = R.cg32(ref32, b2, x0, 1e-8, 50)
    assert_solve(run32(K.Cg32Solver(1e-8, 50), d32, None, b2, x0), ref2, "cg32 indefinite, random b")
    z = MC.zero_diagonal()
    dz = upload(ctx, z)
    inv = O.Pc.jacobi(z).inv_diag
    assert inv[5] == 0.0
    bz = R.store(MC.rhs(z.nrows, seed=4))
    refz = R.pcg32(R.Lowered(z), inv, bz, np.zeros(z.nrows, np.float32), 1e-6, 40)
    assert_solve(run32(K.Pcg32Solver(1e-6, 40), dz.lower(), K.Jacobi().setup(dz), bz, np.zeros(z.nrows, np.float32)), refz, "zero diagonal")


def test_cg32_past_one_fold_chunk(ctx):
    N = 104
    rp, ci, va = K.host_stencil7(N, "poisson")
    a = O.Csr(N ** 3, N ** 3, rp, ci, va, check=False)
    assert (a.nrows + 1023) // 1024 > R.SPEC32[2]                                 # more tile partials than one fold chunk holds
    d32, ref32 = upload(ctx, a).lower(), R.Lowered(a)
    b = R.store(MC.rhs(a.nrows))
    x0 = np.zeros(a.nrows, np.float32)
    ref = R.cg32(ref32, b, x0, 1e-12, 10)
    assert ref.iterations == 10
    assert_solve(run32(K.Cg32Solver(1e-12, 10), d32, None, b, x0), ref, "104^3")


def test_solve32_refusals(ctx):
    a = MC.poisson12()
    d = upload(ctx, a)
    d32 = d.lower()
    b, x0 = R.store(MC.rhs(a.nrows)), MC.vec32(a.nrows, seed=5)

    def refused(solver, op32, pc, bb=b, xx=x0, code=UNSUPPORTED):
        bv, xv = K.DeviceVec32(ctx, bb), K.DeviceVec32(ctx, xx)
        solver.clear_history()
        with pytest.raises(K.KError) as e:
            solver.solve(op32, pc, bv, xv)
        assert e.value.code == code and solver.residual_history == [] and same32(xv.to_host(), xx)     # nothing written

    refused(K.Pcg32Solver(1e-6, 10), d32, K.Ilu0().setup(d))
    for cls in (K.Cg32Solver, K.Pcg32Solver):
        refused(cls(1e-6, 10).with_norm(K.CgNormType.Natural), d32, None)
        refused(cls(1e-6, 10).with_norm(K.CgNormType.NoNorm), d32, None)
        refused(cls(1e-6, 10).with_radius(1.0), d32, None)
        refused(cls(1e-6, 10).with_obj_target(-1.0), d32, None)
        ns = MC.nonsquare()
        refused(cls(1e-6, 10), upload(ctx, ns).lower(), None, MC.vec32(ns.nrows), MC.vec32(ns.nrows, seed=1))
        refused(cls(1e-6, 10), d32, None, b[:-1], x0[:-1], code=ERR_ARG)


# ------------------------------------------------------------------------------------------------------------- 4. refinement
def run_refine(ctx, d, pc, b, x0, tol, max_outer, inner_tol, inner_cap):
    s = K.RefinementSolver(tol, max_outer).with_inner(inner_tol, inner_cap)
    xv = ctx.vec(x0)
    try:
        stats, code = s.solve(d, pc, ctx.vec(b), xv), 0
    except K.KError as e:
        if e.stats is None:
            raise
        stats, code = e.stats, e.code
    return code, stats, list(s.residual_history), xv.to_host()


def assert_refine(got, ref, what):
    code, stats, hist, x = got
    assert code == ref.code, (what, code, ref.code)
    assert (stats.iterations, stats.converged, stats.inner_iterations) == (ref.iterations, ref.converged, ref.inner_iterations), \
        (what, stats, stats.inner_iterations, ref.iterations, ref.converged, ref.inner_iterations)
    assert same64([stats.final_residual], [ref.final_residual]), what
    assert same64(hist, ref.history), (what, hist, ref.history)
    assert same64(x, ref.x), (what, int(np.sum(b64(x) != b64(ref.x))))


@pytest.mark.parametrize("compress", ["default", "0"])
@pytest.mark.parametrize("name", list(MC.REFINE_CASES))
def test_refinement_reaches_the_fp64_tolerance(ctx, monkeypatch, name, compress):
    if compress == "0":
        monkeypatch.setenv("KRYST_SPMV_COMPRESS", "0")
    else:
        monkeypatch.delenv("KRYST_SPMV_COMPRESS", raising=False)
    make, jacobi = MC.REFINE_CASES[name]
    a = make()
    d = upload(ctx, a)
    if compress == "0":
        assert d.encoding()[0] == "csr"
    print(name, compress, d.encoding())
    b, x0 = MC.rhs(a.nrows), np.zeros(a.nrows)
    ref = R.refine(a, R.Lowered(a), O.Pc.jacobi(a).inv_diag if jacobi else None, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.code == 0 and ref.converged and not ref.rejected
    got = run_refine(ctx, d, K.Jacobi().setup(d) if jacobi else None, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert_refine(got, ref, (name, compress))
    assert O.norm(b - a.spmv(got[3])) <= MC.OUTER_TOL * O.norm(b)
    if not jacobi:                                                             # Identity takes the inner CG too
        assert_refine(run_refine(ctx, d, K.IdentityPc().setup(d), b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP), ref, (name, "identity"))


def test_refinement_exits(ctx):
    # a rejected step
    for n in (8, 9, 10):
        h = MC.hilbert(n)
        ref = R.refine(h, R.Lowered(h), None, np.ones(n), np.zeros(n), MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
        if ref.rejected:
            break
    assert ref.rejected
    assert_refine(run_refine(ctx, upload(ctx, h), None, np.ones(n), np.zeros(n), MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP), ref, "rejected")
    # an inner error: the lowering is singular
    s = MC.singular_when_lowered()
    ds = upload(ctx, s)
    assert ds.lower().info["changed"] == 2
    x0 = np.array([0.5, -0.5])
    ref = R.refine(s, R.Lowered(s), None, np.array([1.0, -1.0]), x0, 1e-10, 10, MC.INNER_TOL, 50)
    assert ref.code == R.INDEFINITE_MATRIX and ref.iterations == 0
    assert_refine(run_refine(ctx, ds, None, np.array([1.0, -1.0]), x0, 1e-10, 10, MC.INNER_TOL, 50), ref, "inner error")
    # max_iters = 0, rho0 = 0, the outer cap
    a = MC.poisson12()
    d, a32 = upload(ctx, a), R.Lowered(a)
    b, x0 = MC.rhs(a.nrows), MC.rhs(a.nrows, seed=9)
    assert_refine(run_refine(ctx, d, None, b, x0, 1e-10, 0, MC.INNER_TOL, 50), R.refine(a, a32, None, b, x0, 1e-10, 0, MC.INNER_TOL, 50), "max_iters 0")
    zero = np.zeros(a.nrows)
    assert_refine(run_refine(ctx, d, None, zero, zero, 1e-10, 5, MC.INNER_TOL, 50), R.refine(a, a32, None, zero, zero, 1e-10, 5, MC.INNER_TOL, 50), "rho0 = 0")
    ref = R.refine(a, a32, None, b, x0, 1e-30, 2, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.iterations == 2 and ref.converged
    assert_refine(run_refine(ctx, d, None, b, x0, 1e-30, 2, MC.INNER_TOL, MC.INNER_CAP), ref, "outer cap")
    # the inner cap cuts every inner solve short
    ref = R.refine(a, a32, None, b, x0, 1e-10, 4, MC.INNER_TOL, 5)
    assert ref.inner_iterations[0] == 5
    assert_refine(run_refine(ctx, d, None, b, x0, 1e-10, 4, MC.INNER_TOL, 5), ref, "inner cap")


def test_refinement_refusals(ctx):
    a = MC.poisson12()
    d = upload(ctx, a)
    b, x0 = MC.rhs(a.nrows), MC.rhs(a.nrows, seed=9)
    s = K.RefinementSolver(1e-10, 5)
    xv = ctx.vec(x0)
    with pytest.raises(K.KError) as e:
        s.solve(d, K.Ilu0().setup(d), ctx.vec(b), xv)
    assert e.value.code == UNSUPPORTED and same64(xv.to_host(), x0) and s.residual_history == []
    # a lowered operator of another shape
    other = upload(ctx, MC.banded1025())
    s._lowered[id(d)] = (d, other.lower())
    with pytest.raises(K.KError) as e:
        s.solve(d, None, ctx.vec(b), xv)
    assert e.value.code == ERR_ARG and same64(xv.to_host(), x0)
    # the lowered operator is made once per operator
    s2 = K.RefinementSolver(1e-10, 5)
    assert s2.lowered(d) is s2.lowered(d) and s2.lowered(d) is not s2.lowered(other)
