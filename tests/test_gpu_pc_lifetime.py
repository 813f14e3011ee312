"""What a preconditioner object owns and for how long (kryst_amd/csrc/pc.h): one sizeless object (Identity, the Chebyshev stub) serves
operators of different sizes, because the vector length travels with every apply and not with the object; a set-up that fails mid-way
releases what it took and the next set-up of that kind is right; an object with host index arrays (index-set block Jacobi, additive
Schwarz) is reusable across solves.  Every comparison is bit for bit, against the same solver without a preconditioner or against the
kind's restatement (bjacobi_ref / asm_ref / sor_ref / spai_ref / the oracle), with the helpers of the per-kind test files."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import asm_ref as A
import device_memory as DM
import sor_ref as S
import bjacobi_ref as BR
import pca_gmres_ref as PR
from test_gpu_block_jacobi import sets_ref
from test_gpu_spai import check_values

pytestmark = pytest.mark.gpu

STUB_MESSAGE = "Chebyshev preconditioner requires matrix argument; use apply_chebyshev free function."   # chebyshev.rs:69


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


SOLVERS = {          # name -> (a fresh solver, the name of the method that runs it with a preconditioner)
    "pcg": lambda: (K.PcgSolver(1e-8, 300), "solve"),
    "gmres_left": lambda: (K.GmresSolver(5, 1e-8, 300).with_preconditioning(K.Preconditioning.Left), "solve"),
    "gmres_right": lambda: (K.GmresSolver(5, 1e-8, 300).with_preconditioning(K.Preconditioning.Right), "solve"),
    "fgmres": lambda: (K.FgmresSolver(1e-8, 300, 5), "solve_flex"),
    "bicgstab_rpc": lambda: (K.BiCgStabRightPcSolver(1e-8, 300), "solve"),       # (its tolerance is absolute)
}


def _run(ctx, name, d, pc, b):
    """-> (status code, iterations, converged, final residual, history, x) of one solve from x = 0.25 on device vectors"""
    s, method = SOLVERS[name]()
    xv = K.DeviceVec(ctx, np.full(len(b), 0.25))
    code = 0
    try:
        st = getattr(s, method)(d, pc, K.DeviceVec(ctx, b), xv)
    except K.KError as e:
        code, st = e.code, e.stats
    return code, st.iterations, st.converged, st.final_residual, np.array(s.residual_history), xv.to_host()


def _same(u, v):
    return u[:4] == v[:4] and np.array_equal(u[4], v[4]) and np.array_equal(u[5], v[5])


# ------------------------------------------------------------------------------------------------ 1. one sizeless object, two sizes
def test_sizeless_preconditioners_serve_operators_of_different_sizes(ctx):
    ops = [O.stencil7(N, "poisson") for N in (8, 9)]                      # 512 rows: exactly one tile; 729: a tile and a partial one
    assert [a.nrows for a in ops] == [512, 729]
    devs = [to_dev(ctx, a) for a in ops]
    rhs = [a.spmv(np.linspace(0.5, 1.5, a.nrows)) for a in ops]
    ident = K.IdentityPc().setup(devs[0])                                 # (setup takes the context from the operator, nothing else)
    stub = K.Chebyshev(3).setup(devs[0])
    plain = [{name: _run(ctx, name, d, None, b) for name in SOLVERS} for d, b in zip(devs, rhs)]   # the reference, computed once
    for p in plain:
        assert all(v[1] > 1 for v in p.values())
    for round_ in range(2):
        for k in (0, 1):
            d, b, n = devs[k], rhs[k], ops[k].nrows
            r = np.random.default_rng(10 * round_ + k).standard_normal(n)
            r[::5] = -0.0
            z = ident.apply(r)
            assert np.array_equal(z, r) and np.array_equal(np.signbit(z), np.signbit(r))
            for name in SOLVERS:
                assert _same(_run(ctx, name, d, ident, b), plain[k][name]), (round_, n, name)
            # the stub fails every call with the reference's message and leaves x alone ...
            with pytest.raises(K.KError) as e:
                stub.apply(r)
            assert e.value.code == 2 and STUB_MESSAGE in str(e.value)
            for name in SOLVERS:
                s, method = SOLVERS[name]()
                xv = K.DeviceVec(ctx, np.full(n, 0.25))
                with pytest.raises(K.KError) as e:
                    getattr(s, method)(d, stub, K.DeviceVec(ctx, b), xv)
                assert e.value.code == 2 and STUB_MESSAGE in str(e.value), name
                assert np.array_equal(xv.to_host(), np.full(n, 0.25)), name
            # ... and the next Identity solve, on the other size, is still exact
            o = 1 - k
            assert _same(_run(ctx, "pcg", devs[o], ident, rhs[o]), plain[o]["pcg"]), (round_, n)


# ------------------------------------------------------------------------------------------------ 2. failed set-ups, reuse, the pool
def _with_singular_leading_block(a):
    """the operator with rows 0 and 1 made [[1, -1], [-1, 1]] on {0, 1}: u_11 = 1 - (-1)(-1) / 1 = 0 exactly (ILU(0): zero pivot at row 1),
    and every block or subdomain that holds rows 0 and 1 and no other neighbour of theirs inside is singular"""
    v = a.vals.copy()
    for i, j, x in ((0, 0, 1.0), (0, 1, -1.0), (1, 0, -1.0), (1, 1, 1.0)):
        k = a.row_ptr[i] + int(np.nonzero(a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]] == j)[0][0])
        v[k] = x
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


def _err(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_failed_setups_release_and_objects_are_reusable(ctx):
    a = O.stencil7(8, "poisson")
    n = a.nrows
    assert n == 512
    d = to_dev(ctx, a)
    bad = _with_singular_leading_block(a)
    dbad = to_dev(ctx, bad)
    r = np.random.default_rng(7).standard_normal(n)
    ctx.trim()                                                            # the pool starts empty
    pair = [[0, 1]] + [list(range(s, min(s + 8, n))) for s in range(2, n, 8)]

    # ILU(0): u_11 = 0
    e = _err(lambda: K.TrueIlu0().setup(dbad))
    assert e.code == 5 and e.row == 1
    assert np.array_equal(K.TrueIlu0().setup(d).apply(r), O.Pc.ilu0_true(a).apply(r))

    # block Jacobi (index sets): block 0 = {0, 1} is singular, after every index stream has been uploaded
    e = _err(lambda: K.BlockJacobi(pair).setup(dbad))
    gs, inv, zp = BR.tiles_of(bad.row_ptr, bad.col_idx, bad.vals, pair)
    assert e.code == 5 and zp[0] >= 0 and e.row == gs[0][zp[0]]
    assert np.array_equal(K.BlockJacobi(pair).setup(d).apply(r), O.Pc.approx_inverse(sets_ref(a, pair)).apply(r))

    # additive Schwarz: the same subdomain
    e = _err(lambda: K.AdditiveSchwarz(0, pair).setup(dbad))
    tinv, tzp = A.tiles(bad.row_ptr, bad.col_idx, bad.vals, A.sorted_sets(pair))
    assert e.code == 5 and tzp[0] >= 0 and e.row == A.sorted_sets(pair)[0][tzp[0]]
    gs_ref, own_ref, inv_ref, zp_ref = A.setup(a, pair)
    assert all(z == -1 for z in zp_ref)
    assert np.array_equal(K.AdditiveSchwarz(0, pair).setup(d).apply(r), A.Apply(n, gs_ref, inv_ref)(r))

    # SOR: a_ii + fshift = 6 - 6 = 0 in every row; the lowest is named
    T = K.MatSorType
    e = _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, -6.0).setup(d))
    assert e.code == 5 and e.row == 0
    want = S.Plan(a, 0.0, None, False).apply(r, 1.5, 2, int(T.SYMMETRIC_SWEEP))
    assert np.array_equal(K.Sor(1.5, 2, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d).apply(r), want)

    # SPAI: an index repeated within a pattern column is an argument error (KRYST_ERR_ARG; no row is documented for it: the row query
    # belongs to KRYST_ZERO_PIVOT alone).  The set-up after it is held against the restatement as test_gpu_spai.py does: the pattern exactly,
    # the values to rounding (another least-squares solver); the bit-for-bit comparison that follows is of the APPLY, with the M the device
    # itself exported, not an independent reference of the set-up
    ok = [[j] for j in range(n)]
    assert _err(lambda: K.Spai([[3, 5, 3]] + ok[1:], 1e-9).setup(d)).code == 102
    pc = K.Spai(K.SparsityPattern.Operator, 1e-9).setup(d)
    m = check_values(pc, a, a.row_ptr, a.col_idx, 1e-9)
    assert np.array_equal(pc.apply(r), O.Pc.approx_inverse(m).apply(r))
    del pc

    # one object, many solves: the index arrays on the host and the device state behind the handle are the same ones every time
    b = a.spmv(np.linspace(0.5, 1.5, n))
    over = [list(range(s, min(s + 8, n))) for s in range(0, n, 6)]        # blocks of 8 every 6 rows: they overlap
    made = {"block_jacobi": lambda: K.BlockJacobi(over).setup(d), "asm": lambda: K.AdditiveSchwarz(0, over).setup(d)}
    objs = {k: f() for k, f in made.items()}
    for k, pc in objs.items():
        first = _run(ctx, "pcg", d, pc, b)
        assert first[1] > 1, k
        for _ in range(2):
            assert _same(_run(ctx, "pcg", d, pc, b), first), k
        fresh = made[k]()
        assert _same(_run(ctx, "gmres_right", d, pc, b), _run(ctx, "gmres_right", d, fresh, b)), k
        assert _same(_run(ctx, "pcg", d, pc, b), first), k
        del fresh
    objs.clear()                                                          # the objects are destroyed last
    del pc


# ------------------------------------------------------------------------------------------------ 3. the device memory comes back
def test_setups_and_failed_setups_give_back_their_device_memory(ctx):
    """Every kind's set-up, a failed one included, returns what it allocated: the device's free memory (hipMemGetInfo) after a round of
    failed and successful set-ups, applies and destroys, with the context's pool trimmed, is what it was before that round.  The library has
    no query for the bytes its pool holds, so the figure is the driver's.  64^3 rows: the pooled kinds' blocks (ILU, additive Schwarz, SOR)
    are over the pool's 1 MiB threshold, so they take the pool_free path; block Jacobi, Jacobi-like vectors and SPAI's M take hipFree.  The
    first round is not measured: it loads the kernels and whatever else the runtime allocates once."""
    a = O.stencil7(64, "poisson")
    n = a.nrows
    d = to_dev(ctx, a)
    dbad = to_dev(ctx, _with_singular_leading_block(a))
    rv, zv = K.DeviceVec(ctx, np.random.default_rng(3).standard_normal(n)), K.DeviceVec(ctx, n)
    pair = [[0, 1]] + [list(range(s, min(s + 8, n))) for s in range(2, n, 8)]
    T = K.MatSorType
    failing = [lambda: K.TrueIlu0().setup(dbad), lambda: K.BlockJacobi(pair).setup(dbad), lambda: K.AdditiveSchwarz(0, pair).setup(dbad),
               lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, -6.0).setup(d)]
    working = [lambda: K.TrueIlu0().setup(d), lambda: K.BlockJacobi(pair).setup(d), lambda: K.AdditiveSchwarz(0, pair).setup(d),
               lambda: K.Sor(1.5, 2, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d), lambda: K.Spai(K.SparsityPattern.Operator, 1e-9).setup(d),
               lambda: K.Jacobi().setup(d), lambda: K.ChebyshevPc(3, 0.5, 12.0).setup(d)]

    def round_():
        for f in failing:
            assert _err(f).code == 5
        for f in working:
            pc = f()
            pc.apply(rv, zv)
            del pc                                                        # destroyed here: CPython drops the last reference
        ctx.synchronize()

    free_bytes = lambda: DM.free_bytes(ctx)                             # (tests/device_memory.py: the figure of every memory test)

    free_bytes()                                                          # (the first query brings its own runtime state)
    round_()
    ctx.trim()
    before = free_bytes()
    round_()
    # no solve ran since the trim, so there is no work arena: what trim releases now is what the destroyed objects put into the pool --
    # at least additive Schwarz's product vector (one double per subdomain row) and its tiles (8 doubles per row)
    released = ctx.trim()
    assert released >= 8 * n + 64 * n, released
    assert free_bytes() == before


# ------------------------------------------------------------------------------------------------ 4. the restarted solvers' scaffold
PCN = K.Preconditioning
RESTARTED = {        # name -> a fresh solver; every one of them applies the preconditioner it is given
    "gmres_left": lambda: K.GmresSolver(5, 1e-8, 40).with_preconditioning(PCN.Left),
    "gmres_right": lambda: K.GmresSolver(5, 1e-8, 40).with_preconditioning(PCN.Right),
    "gmres_left_textbook": lambda: K.GmresSolver(5, 1e-8, 40).with_preconditioning(PCN.LeftTextbook),
    "fgmres": lambda: K.FgmresSolver(1e-8, 40, 5),
    "pca_gmres_right": lambda: K.PcaGmresSolver(5, 1, 1, 1e-8, 40).with_preconditioning(PCN.Right),
    "sstep_right": lambda: K.PcaGmresSolver(5, 1, 3, 1e-8, 40).with_preconditioning(PCN.Right).with_textbook(),
}


def test_restarted_solvers_reject_a_preconditioner_of_another_size(ctx):
    """A sized preconditioner launches over its own n: one built on another operator is an argument error (KRYST_ERR_ARG, what PCG
    answers), raised before any device work, and x comes back as it went in.  The sizeless Identity still serves both operators."""
    ops = [O.stencil7(N, "poisson") for N in (8, 9)]
    assert [a.nrows for a in ops] == [512, 729]
    devs = [to_dev(ctx, a) for a in ops]
    jac = [K.Jacobi().setup(d) for d in devs]
    ident = K.IdentityPc().setup(devs[0])
    for k in (0, 1):
        a, d, n = ops[k], devs[k], ops[k].nrows
        bv = K.DeviceVec(ctx, a.spmv(np.linspace(0.5, 1.5, n)))
        x_in = np.random.default_rng(k).standard_normal(n)
        for name, make in RESTARTED.items():
            xv = K.DeviceVec(ctx, x_in)
            with pytest.raises(K.KError) as e:
                make().solve(d, jac[1 - k], bv, xv)
            assert e.value.code == 102, (n, name)
            assert np.array_equal(xv.to_host(), x_in), (n, name)
            xv = K.DeviceVec(ctx, x_in)
            st = make().solve(d, ident, bv, xv)
            assert st.iterations > 1 and np.all(np.isfinite(xv.to_host())), (n, name)


@pytest.mark.parametrize("restart", [1, 2, 7, 33])
def test_restarted_solvers_small_arrays_at_odd_restarts(ctx, restart):
    """H, g, the rotations, y, the state struct, the gate word and the pointer tables of a solve are slices of one allocation
    (restart_common.h: SmallArena).  At these restart values (and s-step blocks of 1, 3 and 16) every slice has an odd element count, so a
    wrong slice size or alignment moves a neighbour: each whole solve is bit for bit its oracle's -- history, iteration count and x."""
    rs = O.Reduce.tiled(*K.reduce_spec())
    a = O.stencil7(8, "convdiff")
    assert a.nrows == 512
    d = to_dev(ctx, a)
    b = a.spmv(np.ones(a.nrows))
    x0 = np.linspace(-0.5, 0.5, a.nrows)
    kpc, opc = K.Jacobi().setup(d), O.Pc.jacobi(a)

    def same(ref, st, s, x):
        assert (st.iterations, st.converged, st.final_residual) == (ref.iterations, ref.converged, ref.final_residual), (st, ref)
        assert np.array_equal(np.array(s.residual_history), ref.history) and np.array_equal(x, ref.x)

    for side in (PCN.NoPc, PCN.Left, PCN.Right, PCN.LeftTextbook):
        pcs = (None, None) if side == PCN.NoPc else (kpc, opc)
        ref = O.solve("gmres", a, b, x0=x0, pc=pcs[1], tol=1e-8, max_iters=40, restart=restart, side=int(side), rs=rs)
        s = K.GmresSolver(restart, 1e-8, 40).with_preconditioning(side)
        x = x0.copy()
        same(ref, s.solve(d, pcs[0], b, x), s, x)
    ref = PR.as_written(a, b, pc=opc, side=int(PCN.Right), restart=restart, tol=1e-8, max_iters=40, rs=rs)
    s = K.PcaGmresSolver(restart, 1, 1, 1e-8, 40).with_preconditioning(PCN.Right)
    x = x0.copy()
    same(ref, s.solve(d, kpc, b, x), s, x)
    for sb in (1, 3, 16):
        ref = PR.sstep(a, b, x=x0, pc=opc, side=2, restart=restart, block_size=sb, tol=1e-8, max_iters=40, rs=rs)
        s = K.PcaGmresSolver(restart, 1, sb, 1e-8, 40).with_preconditioning(PCN.Right).with_textbook()
        x = x0.copy()
        same(ref, s.solve(d, kpc, b, x), s, x)
