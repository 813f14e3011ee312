"""Operands that share storage: which overlaps the C ABI refuses and which it defines (include/kryst_hip.h states both next to the entry
points).

REFUSED with KRYST_ERR_ARG before any launch, the vector unchanged bit for bit: x == y in kryst_spmv / kryst_spmv_transpose, r == z in
kryst_pc_apply / kryst_bench_pc_apply / kryst_apply_chebyshev -- one rule for every preconditioner kind (the reference's
apply(&self, r: &V, z: &mut V) cannot alias; the SPAI and block-Jacobi applies are products, the sync-free ILU solves arm z with a sentinel
and would spin on the r they destroyed, ASM and AMG read r after the first writes to z).  An unguarded in-place apply is never run here.

DEFINED: kryst_axpy / kryst_aypx with x == y, kryst_sub in every aliasing, kryst_dot(v, v), kryst_vec_copy(v, v) (nothing is done), and
every *_solve_dev / stepping session with b and x the same vector: x0 = b, the solvers iterate on a copy and write x once at the end."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import krylov_ext_ref as KR
from nonfinite_cases import same_ieee

pytestmark = pytest.mark.gpu

ERR_ARG = 102
PCN = K.Preconditioning


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def refused(f, v, data):
    with pytest.raises(K.KError) as e:
        f()
    assert e.value.code == ERR_ARG, e.value
    assert np.array_equal(bits(v.to_host()), bits(data)), "a refused call changed its operand"


# ------------------------------------------------------------------------------------------------ refused
PC_KINDS = {
    "identity": lambda d: K.IdentityPc().setup(d),
    "jacobi": lambda d: K.Jacobi().setup(d),
    "ilu0-as-written": lambda d: K.Ilu0().setup(d),
    "ilu0-textbook": lambda d: K.TrueIlu0().setup(d),
    "ilup1": lambda d: K.Ilup(1).setup(d),
    "ilut": lambda d: K.Ilut(3, 1e-12).setup(d),
    "chebyshev": lambda d: K.ChebyshevPc(3, 0.2, 11.9).setup(d),
    "spai": lambda d: K.Spai(K.SparsityPattern.Operator, 1e-12).setup(d),
    "block-jacobi-uniform": lambda d: K.BlockJacobi.uniform(8).setup(d),
    "block-jacobi-index-sets": lambda d: K.BlockJacobi([np.arange(k, min(k + 40, d.nrows())) for k in range(0, d.nrows(), 40)]).setup(d),
    "asm": lambda d: K.AdditiveSchwarz(0, K.AdditiveSchwarz.grid_boxes(8), None).setup(d),
    "asm-restricted": lambda d: K.AdditiveSchwarz(1, K.AdditiveSchwarz.grid_boxes(8, (2, 2, 2)), None).restricted().setup(d),
    "sor": lambda d: K.Sor(1.5, 2, 1, K.MatSorType.SYMMETRIC_SWEEP | K.MatSorType.LOCAL_FORWARD_SWEEP, 0.0).setup(d),
    "amg-as-written": lambda d: K.Amg(10, 0.1).setup(d),
    "amg-smoothed-aggregation": lambda d: K.Amg(1).with_textbook(0.0).setup(d),
}


@pytest.mark.parametrize("kind", list(PC_KINDS))
def test_an_apply_in_place_is_refused_for_every_kind(ctx, kind):
    a = O.stencil7(8, "convdiff")
    d = to_dev(ctx, a)
    pc = PC_KINDS[kind](d)
    r = O.splitmix64_uniform(5, a.nrows) - 0.5
    v = ctx.vec(r)
    refused(lambda: pc.apply(v, v), v, r)
    refused(lambda: pc.bench_apply(v, v, 1), v, r)
    # the object is as it was: an apply into another vector gives what a fresh object gives
    z = pc.apply(v, ctx.vec(np.zeros(a.nrows))).to_host()
    assert np.array_equal(bits(z), bits(PC_KINDS[kind](d).apply(ctx.vec(r), ctx.vec(np.zeros(a.nrows))).to_host()))
    assert np.array_equal(bits(v.to_host()), bits(r))


def test_apply_chebyshev_and_the_products_in_place_are_refused(ctx):
    a = O.stencil7(8, "convdiff")
    d = to_dev(ctx, a)
    r = O.splitmix64_uniform(6, a.nrows) - 0.5
    v = ctx.vec(r)
    for m in (0, 1, 5):
        refused(lambda: K.apply_chebyshev(d, v, v, 0.2, 11.9, m), v, r)
    refused(lambda: d.spmv(v, v), v, r)
    refused(lambda: d.spmv_transpose(v, v), v, r)


@pytest.mark.parametrize("n", [1, 511, 513])
def test_a_vector_copied_onto_itself_is_left_alone(ctx, n):
    x = np.random.default_rng(n).standard_normal(n); x[-1] = -0.0
    v = ctx.vec(x)
    assert v.copy_from(v) is v and np.array_equal(bits(v.to_host()), bits(x))


# ------------------------------------------------------------------------------------------------ defined: BLAS-1
SPECIAL = ((np.inf, np.nan), (-0.0, -np.inf), (5e-324, 1.7976931348623157e308), (np.nan, -5e-324), (0.25, -0.75))
ALPHAS = (np.inf, np.nan, -0.0, 0.37)


@pytest.mark.parametrize("n", [1, 511, 513])
def test_pointwise_kernels_and_dot_with_operands_that_share_storage(ctx, rs, n):
    """the special values of test_pointwise_kernels_and_dot_on_special_values in the first and the last element"""
    rng = np.random.default_rng(n)
    x0, y0 = rng.standard_normal(n), rng.standard_normal(n)
    for first, last in SPECIAL:
        x = x0.copy(); x[0] = first; x[-1] = last
        y = y0.copy(); y[-1] = -0.0
        with np.errstate(all="ignore"):
            for al in ALPHAS:
                v = ctx.vec(x)
                K.axpy(al, v, v)
                assert same_ieee(v.to_host(), x + al * x), ("axpy", n, al, first)
                v = ctx.vec(x)
                K.aypx(al, v, v)
                assert same_ieee(v.to_host(), x + al * x), ("aypx", n, al, first)
            dx, dy = ctx.vec(x), ctx.vec(y)
            assert same_ieee(K.sub(dx, dy, dx).to_host(), x - y), ("sub, out = a", n, first)
            dx = ctx.vec(x)
            assert same_ieee(K.sub(dx, dy, dy).to_host(), x - y), ("sub, out = b", n, first)
            out = ctx.vec(np.full(n, np.nan))
            assert same_ieee(K.sub(dx, dx, out).to_host(), x - x), ("sub, a = b", n, first)
            assert same_ieee(K.sub(dx, dx, dx).to_host(), x - x), ("sub, out = a = b", n, first)
            dx = ctx.vec(x)
            assert same_ieee([K.dot(dx, dx)], [O.dot(x, x, rs)]), ("dot(v, v)", n, first)
            assert np.array_equal(bits(dx.to_host()), bits(x))


# ------------------------------------------------------------------------------------------------ defined: solves with b == x
def _oracle(method, **kw):
    return lambda a, b, opc, rs: O.solve(method, a, b, x0=b, pc=opc, tol=1e-9, max_iters=40, rs=rs, **kw)


# name: (reference from x0 = b, device solver, operator kind, device pc, oracle pc)
SOLVES = {
    "cg": (_oracle("cg"), lambda: K.CgSolver(1e-9, 40), "poisson", None, None),
    "pcg-jacobi": (_oracle("pcg"), lambda: K.PcgSolver(1e-9, 40), "poisson", K.Jacobi, O.Pc.jacobi),
    "bicgstab": (_oracle("bicgstab"), lambda: K.BiCgStabSolver(1e-9, 40), "convdiff", None, None),
    "gmres-right-ilu": (_oracle("gmres", restart=12, side=2), lambda: K.GmresSolver(12, 1e-9, 40).with_preconditioning(PCN.Right), "convdiff",
                        K.TrueIlu0, O.Pc.ilu0_true),
    "fgmres": (_oracle("fgmres", restart=16), lambda: K.FgmresSolver(1e-9, 40, 16), "convdiff", K.Jacobi, O.Pc.jacobi),
    "tfqmr": (_oracle("tfqmr"), lambda: K.TfqmrSolver(1e-9, 40), "convdiff", None, None),
    "minres": (lambda a, b, opc, rs: KR.SOLVERS["minres"](a, b, b, 1e-9, 40, rs), lambda: K.MinresSolver(1e-9, 40), "poisson", None, None),
}


@pytest.mark.parametrize("N", [9, 8])
@pytest.mark.parametrize("name", list(SOLVES))
def test_a_solve_with_b_and_x_in_one_vector(ctx, rs, name, N):
    ref_fn, make, kind, kpc, opc = SOLVES[name]
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    ref = ref_fn(a, b, opc(a) if opc else None, rs)
    assert ref.iterations > 0
    v = ctx.vec(b)
    s = make()
    st = getattr(s, "solve_flex" if name == "fgmres" else "solve")(d, kpc().setup(d) if kpc else None, v, v)
    assert (st.iterations, bool(st.converged)) == (ref.iterations, bool(ref.converged)), (name, st, ref.iterations)
    assert np.array_equal(bits(s.residual_history), bits(ref.history)), (name, "history")
    assert np.array_equal(bits(v.to_host()), bits(ref.x)), (name, "the vector does not hold x")


@pytest.mark.parametrize("N", [9, 8])
def test_a_cg_stepping_session_with_b_and_x_in_one_vector(ctx, rs, N):
    a = O.stencil7(N)
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    steps = (2, 5, 1)
    ref = O.solve("cg", a, b, x0=b, tol=1e-30, max_iters=sum(steps), rs=rs)
    v = ctx.vec(b)
    with K.Session("cg", d, None, v, v, tol=1e-30, max_iters=1000) as sess:
        for q in steps:
            sess.step(q)
        st = sess.end()
    assert st.iterations == ref.iterations and np.array_equal(bits(sess.residual_history), bits(ref.history))
    assert np.array_equal(bits(v.to_host()), bits(ref.x))
