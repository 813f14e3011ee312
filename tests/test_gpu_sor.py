"""SOR / SSOR and the coloured order (src/preconditioner/sor.rs; kryst_amd/csrc/sor.hip) against the restatement tests/sor_ref.py, bit for
bit: applies for every flag combination, its and omega on random sparse operators and on the stencil operators up to 96^3 through every
operator constructor, the coloured order (red-black, the distance-2 colouring, a random vector), whole PCG solves through amg_ref.pcg,
KspContext and stepping sessions, the pay-off against Jacobi as iteration counts, and the error paths."""
import itertools
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import sor_ref as S
import amg_ref as AR

pytestmark = pytest.mark.gpu

T = K.MatSorType
FLAGS = {"lower": T.APPLY_LOWER, "upper": T.APPLY_UPPER, "symmetric": T.SYMMETRIC_SWEEP}
CASES = list(itertools.product(FLAGS, (False, True), (0, 1, 3), (1.0, 1.5, 0.3)))


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    t, v, f = K.reduce_spec()
    return O.Reduce.tiled(t, v, f)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def random_sparse(n, seed, density=0.06):
    """unsymmetric, rows without off-diagonal entries, negative and tiny values"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) * (rng.random((n, n)) < density)
    m[rng.random((n, n)) < 0.01] = 1e-300
    m[rng.random((n, n)) < 0.01] = -3e-17
    m[rng.choice(n, max(n // 10, 1), replace=False), :] = 0.0
    np.fill_diagonal(m, rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 4.0, n))
    return O.Csr.from_dense(m, keep_zeros=False)


def red_black(N):
    r = np.arange(N ** 3)
    return (r % N + (r // N) % N + r // (N * N)) % 2


def check_matrix_of_cases(ctx, a, d, seed, colors=None, cases=CASES):
    x = np.random.default_rng(seed).standard_normal(a.nrows)
    x[::7] = -0.0
    plans = {e: S.Plan(a, 0.0, colors, e) for e in (False, True)}
    for flag, eis, its, omega in cases:
        sym = FLAGS[flag] | (T.EISENSTAT if eis else 0) | T.LOCAL_FORWARD_SWEEP
        ctx.poison_lds()
        pc = K.Sor(omega, its, 1, sym, 0.0).with_colors(colors).setup(d)
        got = pc.apply(x)
        want = plans[eis].apply(x, omega, its, int(sym))
        assert np.array_equal(got, want), (flag, eis, its, omega, int(np.sum(got != want)))
        inf = pc.info()
        assert inf["rows"] == a.nrows
        assert 0 <= inf["workgroups_forward"] <= 256 and 0 <= inf["workgroups_backward"] <= 256
        assert inf["passes_forward"] == (plans[eis].passes(True) if sym & T.APPLY_LOWER else 0)
        assert inf["passes_backward"] == (plans[eis].passes(False) if sym & T.APPLY_UPPER else 0)
    return plans


# ------------------------------------------------------------------------------------------------ applies, as written
def test_reference_cases_on_the_device(ctx):
    """tests/preconditioner_sor.rs: identity, tridiag(5, -1, 4, -1) forward, SSOR finite"""
    x = np.ones(5)
    eye = to_dev(ctx, O.Csr.from_dense(np.eye(5), keep_zeros=False))
    assert np.array_equal(K.Sor(1.0, 1, 1, T.APPLY_LOWER, 0.0).setup(eye).apply(x), x)
    dt = O.tridiag(5, -1.0, 4.0, -1.0)
    tri = to_dev(ctx, O.Csr.from_dense(dt, keep_zeros=False))
    y = K.Sor(1.0, 1, 1, T.APPLY_LOWER, 0.0).setup(tri).apply(x)
    expected = np.zeros(5)
    for i in range(5):
        expected[i] = (x[i] + (expected[i - 1] if i > 0 else 0.0) + (x[i + 1] if i + 1 < 5 else 0.0)) / 4.0
    assert np.all(np.abs(y - expected) < 1e-12) and np.array_equal(y, S.apply_loop(dt, S.setup(dt), x, 1.0, 1, S.APPLY_LOWER))
    ys = K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(tri).apply(x)
    assert np.all(np.isfinite(ys)) and np.array_equal(ys, S.apply_loop(dt, S.setup(dt), x, 1.0, 1, S.SYMMETRIC_SWEEP))
    assert np.array_equal(K.PC.Ssor().build(tri).apply(x), ys)


@pytest.mark.parametrize("n,seed", [(1, 0), (37, 1), (200, 2), (3000, 3)])
def test_apply_random_sparse(ctx, n, seed):
    a = random_sparse(n, seed, density=0.06 if n <= 200 else 0.002)
    d = to_dev(ctx, a)
    check_matrix_of_cases(ctx, a, d, seed)
    if n <= 200:                                                       # the literal loops once more, directly
        dm = S.dense(a)
        x = np.random.default_rng(seed).standard_normal(n)
        for sym in (S.APPLY_UPPER, S.SYMMETRIC_SWEEP | S.EISENSTAT):
            assert np.array_equal(K.Sor(1.5, 3, 1, sym, 0.25).setup(d).apply(x), S.apply_loop(dm, S.setup(dm, 0.25), x, 1.5, 3, sym))


@pytest.mark.parametrize("kind", ["poisson", "varcoef"])
@pytest.mark.parametrize("N", [8, 32, 96])
def test_apply_stencil(ctx, N, kind):
    """N = 96: n = 884 736, past one fold chunk; 3N - 2 grid-barrier separated passes per sweep"""
    a = O.stencil7(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    plans = check_matrix_of_cases(ctx, a, d, N)
    assert plans[False].passes(True) == plans[False].passes(False) == 3 * N - 2


@pytest.mark.parametrize("kind", ["poisson", "aniso", "convdiff", "varcoef"])
def test_every_operator_constructor(ctx, kind):
    """the sweep reads the plain CSR arrays every operator keeps, whatever encoding its SpMV uses"""
    N = 12
    a = O.stencil7(N, kind)
    x = np.random.default_rng(12).standard_normal(a.nrows)
    want = S.Plan(a).apply(x, 1.5, 2, S.SYMMETRIC_SWEEP)
    ops = [K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx),
           K.CsrMatrix.from_csr_i32(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx),
           K.CsrMatrix.stencil7(N, kind, ctx=ctx)]
    encodings = set()
    for d in ops:
        encodings.add(d.encoding()[0])
        ctx.poison_lds()
        assert np.array_equal(K.Sor(1.5, 2, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d).apply(x), want)
    b = random_sparse(500, 77, density=0.01)                           # a general operator: another encoding again
    db = to_dev(ctx, b)
    encodings.add(db.encoding()[0])
    xb = np.random.default_rng(3).standard_normal(500)
    assert np.array_equal(K.Sor(0.3, 2, 1, T.SYMMETRIC_SWEEP, 0.0).setup(db).apply(xb), S.Plan(b).apply(xb, 0.3, 2, S.SYMMETRIC_SWEEP))
    assert len(encodings) >= 2, encodings


def test_device_vectors_and_repeated_applies(ctx):
    a = O.stencil7(10, "varcoef")
    d = to_dev(ctx, a)
    pc = K.Sor(1.2, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d)
    p = S.Plan(a)
    rng = np.random.default_rng(4)
    z = K.DeviceVec(ctx, np.full(a.nrows, np.nan))                      # the apply does not read what y held
    for _ in range(3):
        x = rng.standard_normal(a.nrows)
        pc.apply(K.DeviceVec(ctx, x), z)
        assert np.array_equal(z.to_host(), p.apply(x, 1.2, 1, S.SYMMETRIC_SWEEP))
    zz = pc.apply(np.full(a.nrows, -0.0))
    assert np.all(zz == 0.0)
    up = K.Sor(1.2, 2, 1, T.APPLY_UPPER, 0.0).setup(d)                  # backward only: starts from y = +0.0, whatever y held
    x = rng.standard_normal(a.nrows)
    up.apply(K.DeviceVec(ctx, x), z)
    assert np.array_equal(z.to_host(), p.apply(x, 1.2, 2, S.APPLY_UPPER))


# ------------------------------------------------------------------------------------------------ the coloured order
def test_coloured_red_black(ctx):
    for N, kind in ((8, "poisson"), (32, "varcoef")):
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        rb = red_black(N)
        cases = CASES if N == 8 else [c for c in CASES if c[2] == 1]
        plans = check_matrix_of_cases(ctx, a, d, N, colors=rb, cases=cases)
        assert plans[False].passes(True) == plans[False].passes(False) == 2
        if N == 8:                                                     # by definition: the loops on the permuted dense matrix
            x = np.random.default_rng(1).standard_normal(a.nrows)
            got = K.PC.Multicolor(rb, omega=1.5, its=2).build(d).apply(x)
            assert np.array_equal(got, S.apply_permuted(S.dense(a), x, rb, 1.5, 2, S.SYMMETRIC_SWEEP))


def test_coloured_distance2_and_random(ctx):
    N = 10
    a = O.stencil7(N, "aniso")
    d = to_dev(ctx, a)
    c2 = K.color_graph(d)
    assert np.array_equal(c2, K.color_graph(a))
    ncol = int(c2.max()) + 1
    plans = check_matrix_of_cases(ctx, a, d, 5, colors=c2)
    assert 7 <= ncol and plans[False].passes(True) <= ncol and plans[False].passes(False) <= ncol
    rnd = np.random.default_rng(6).integers(0, 9, a.nrows)
    check_matrix_of_cases(ctx, a, d, 6, colors=rnd)
    b = random_sparse(300, 41, density=0.02)                           # unsymmetric pattern, arbitrary colours
    cb = np.random.default_rng(7).integers(0, 4, 300)
    check_matrix_of_cases(ctx, b, to_dev(ctx, b), 7, colors=cb)
    x = np.random.default_rng(8).standard_normal(300)
    assert np.array_equal(K.Sor(0.3, 3, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(cb).setup(to_dev(ctx, b)).apply(x),
                          S.apply_permuted(S.dense(b), x, cb, 0.3, 3, S.SYMMETRIC_SWEEP))
    one = K.Sor(1.5, 2, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(np.zeros(300, dtype=int)).setup(to_dev(ctx, b)).apply(x)
    assert np.array_equal(one, S.Plan(b).apply(x, 1.5, 2, S.SYMMETRIC_SWEEP))


# ------------------------------------------------------------------------------------------------ whole solves
def _pcg_both(ctx, rs, a, d, pc, M, b, tol, max_iters):
    xr, it, code, hist = AR.pcg(a, None, b, tol, max_iters, rs, apply=lambda r, z: M(r))
    assert code == 0
    s = K.PcgSolver(tol, max_iters)
    x = np.zeros(a.nrows)
    try:
        st = s.solve(d, pc, b, x)
    except K.KError as e:                      # not converged within max_iters: the stats ride on the error
        st = e.stats
    assert st.iterations == it
    assert np.array_equal(np.array(s.residual_history), np.array(hist))
    assert np.array_equal(x, xr)
    return it


# PCG on Poisson 32^3, b = 1, tol 1e-8, from the restatement on the CPU (amg_ref.pcg with sor_ref.Plan / 1 / diag)
SSOR_ITERATIONS_32, JACOBI_ITERATIONS_32 = 46, 81


@pytest.mark.parametrize("handoff", ["poll", "ticket"])
def test_pcg_ssor_32(ctx, rs, handoff, monkeypatch):
    monkeypatch.setenv("KRYST_FOLD_POLL", "1" if handoff == "poll" else "0")
    N = 32
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    p = S.Plan(a)
    it = _pcg_both(ctx, rs, a, d, K.PC.Ssor().build(d), lambda r: p.apply(r, 1.0, 1, S.SYMMETRIC_SWEEP), np.ones(a.nrows), 1e-8, 400)
    assert it == SSOR_ITERATIONS_32


@pytest.mark.parametrize("handoff", ["poll", "ticket"])
def test_pcg_ssor_96_past_one_fold_chunk(ctx, rs, handoff, monkeypatch):
    monkeypatch.setenv("KRYST_FOLD_POLL", "1" if handoff == "poll" else "0")
    N = 96
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    assert a.nrows == 884736
    p = S.Plan(a)
    _pcg_both(ctx, rs, a, d, K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d), lambda r: p.apply(r, 1.0, 1, S.SYMMETRIC_SWEEP),
              a.spmv(np.linspace(0.5, 1.5, a.nrows)), 1e-8, 25)


def test_pcg_multicolor_32(ctx, rs):
    N = 32
    a = O.stencil7(N, "varcoef")
    d = K.CsrMatrix.stencil7(N, "varcoef", ctx=ctx)
    rb = red_black(N)
    p = S.Plan(a, colors=rb)
    _pcg_both(ctx, rs, a, d, K.PC.Multicolor(rb).build(d), lambda r: p.apply(r, 1.0, 1, S.SYMMETRIC_SWEEP), np.ones(a.nrows), 1e-8, 400)


def test_pays_off_against_jacobi(ctx, rs):
    """the condition, not a time: on Poisson 32^3 at 1e-8 PCG + SSOR needs fewer iterations than PCG + Jacobi.  The as-written omega = 1
    symmetric sweep is not a symmetric operator (one symmetric Gauss-Seidel step from the initial guess x), PCG converges with it all
    the same."""
    N = 32
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    b = np.ones(N ** 3)
    its = {}
    for name, pc in (("ssor", K.PC.Ssor().build(d)), ("jacobi", K.PC.Jacobi().build(d))):
        its[name] = K.PcgSolver(1e-8, 400).solve(d, pc, b, np.zeros(N ** 3)).iterations
    assert (its["ssor"], its["jacobi"]) == (SSOR_ITERATIONS_32, JACOBI_ITERATIONS_32)
    assert its["ssor"] < its["jacobi"]


def test_ksp_context_and_session(ctx, rs):
    N = 16
    a = O.stencil7(N, "aniso")
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    pc = K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d)
    p = S.Plan(a)
    M = lambda r, z: p.apply(r, 1.0, 1, S.SYMMETRIC_SWEEP)
    x1 = np.zeros(a.nrows)
    st1 = K.PcgSolver(1e-8, 300).solve(d, pc, b, x1)
    x2 = np.zeros(a.nrows)
    st2 = K.KspContext(K.SolverKind.Pcg, d, pc=pc, tol=1e-8, max_it=300).solve_context(b, x2)
    assert (st1.iterations, st1.final_residual) == (st2.iterations, st2.final_residual) and np.array_equal(x1, x2)
    xr, it, code, hist = AR.pcg(a, None, b, 1e-8, 300, rs, apply=M)
    assert st1.iterations == it and np.array_equal(x1, xr)
    steps = 9
    xr, it, code, hist = AR.pcg(a, None, b, 1e-30, steps, rs, apply=M)
    xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    with K.Session("pcg", d, pc, K.DeviceVec(ctx, b), xv, tol=1e-30, max_iters=steps) as sess:
        sess.step(steps)
        st = sess.end()
        h = sess.residual_history
    assert st.iterations == it == steps
    assert np.array_equal(np.array(h), np.array(hist)) and np.array_equal(xv.to_host(), xr)


def _stats(fn):
    try:
        return fn()
    except K.KError as e:                      # not converged within max_iters: the stats ride on the error
        assert e.stats is not None, e
        return e.stats


@pytest.mark.parametrize("solver,max_iters", [("gmres_left", 45), ("gmres_right", 45), ("gmres_left", 30), ("bicgstab_rpc", 12)])
def test_forward_sweep_under_gmres_and_bicgstab(ctx, rs, solver, max_iters):
    """the forward sweep as the preconditioner of the unsymmetric solvers on the variable-coefficient operator, bit for bit against
    tests/krylov_pc_ref.py (pinned to the C oracle on the CPU) with sor_ref's apply: iterations, final residual, history and x.  The
    as-written forward sweep applied to a residual is (D + L)^-1 (I - U) r; M^-1 A is then indefinite and restarted GMRES stalls with
    it, so the runs are cut off after a fixed number of iterations (GMRES: inside the second restart cycle, and
    at a cycle's end): a stall is no obstacle to comparing bits.  BiCgStabSolver itself ignores its preconditioner, as the reference
    does; the right-preconditioned extension is the one that takes it."""
    import krylov_pc_ref as KR
    N = 16
    a = O.stencil7(N, "varcoef")
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    pc = K.Sor(1.0, 1, 1, T.APPLY_LOWER, 0.0).setup(d)
    p = S.Plan(a)
    M = lambda r: p.apply(r, 1.0, 1, S.APPLY_LOWER)
    x = np.zeros(a.nrows)
    if solver == "bicgstab_rpc":
        tol = 1e-12 * float(np.linalg.norm(b))
        xr, it, fr, conv, hist = KR.bicgstab_rpc(a, M, b, tol, max_iters, rs)
        s = K.BiCgStabRightPcSolver(tol, max_iters)
    else:
        side = "left" if solver == "gmres_left" else "right"
        xr, it, fr, conv, hist = KR.gmres(a, M, side, b, 30, 1e-12, max_iters, rs)
        s = K.GmresSolver(30, 1e-12, max_iters).with_preconditioning(K.Preconditioning.Left if side == "left" else K.Preconditioning.Right)
    assert it == max_iters and np.all(np.isfinite(xr)) and np.all(np.isfinite(hist))
    st = _stats(lambda: s.solve(d, pc, b, x))
    assert (st.iterations, st.final_residual, bool(st.converged)) == (it, fr, conv)
    assert np.array_equal(np.array(s.residual_history), hist)
    assert np.array_equal(x, xr)
    if solver != "bicgstab_rpc":                                       # KspContext: the same bits
        kind = K.SolverKind.GmresLeft if solver == "gmres_left" else K.SolverKind.GmresRight
        x2 = np.zeros(a.nrows)
        st2 = _stats(lambda: K.KspContext(kind, d, pc=pc, tol=1e-12, max_it=max_iters, restart=30).solve_context(b, x2))
        assert (st2.iterations, st2.final_residual) == (it, fr) and np.array_equal(x2, xr)


def test_apply_large_unsymmetric_against_the_literal_loops(ctx):
    """n = 3000, unsymmetric, many levels: the device against the dense loops themselves (not the level-by-level restatement, which
    shares the idea of a schedule with the device), for the sweeps whose schedule carries anti-dependencies and for EISENSTAT"""
    a = random_sparse(3000, 3, density=0.002)
    d = to_dev(ctx, a)
    dm = S.dense(a)
    inv = S.setup(dm)
    x = np.random.default_rng(33).standard_normal(3000)
    for omega, its, sym in ((1.5, 1, S.SYMMETRIC_SWEEP), (0.3, 2, S.APPLY_UPPER), (1.0, 1, S.SYMMETRIC_SWEEP | S.EISENSTAT)):
        pc = K.Sor(omega, its, 1, sym, 0.0).setup(d)
        assert pc.info()["passes_backward"] > 3
        assert np.array_equal(pc.apply(x), S.apply_loop(dm, inv, x, omega, its, sym)), (omega, its, sym)
    cb = np.random.default_rng(34).integers(0, 6, 3000)
    got = K.Sor(1.5, 1, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(cb).setup(d).apply(x)
    assert np.array_equal(got, S.apply_permuted(dm, x, cb, 1.5, 1, S.SYMMETRIC_SWEEP))


# ------------------------------------------------------------------------------------------------ errors
def _err(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_errors(ctx):
    a = O.stencil7(6, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    dz = np.diag([2.0, 1.0, 3.0, 0.0, 5.0, 0.0])
    dz[3, 1] = 1.0; dz[1, 2] = -1.0
    z = to_dev(ctx, O.Csr.from_dense(dz, keep_zeros=False))                # rows 3 and 5: no stored diagonal
    e = _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(z))
    assert e.code == 5 and e.row == 3
    e = _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, -2.0).setup(z))   # the shift makes row 0 the first zero
    assert e.code == 5 and e.row == 0
    x = np.arange(1.0, 7.0)
    assert np.array_equal(K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.5).setup(z).apply(x),
                          S.apply_loop(dz, S.setup(dz, 0.5), x, 1.0, 1, S.SYMMETRIC_SWEEP))
    assert _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(np.zeros(n - 1, dtype=int)).setup(d)).code == 102
    assert _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(np.full(n, -1)).setup(d)).code == 102
    assert _err(lambda: K.Sor(1.0, -1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d)).code == 102
    rect = K.CsrMatrix.from_csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0], ctx=ctx)
    assert _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(rect)).code == 102
    dd = K.CsrMatrix.from_csr_dist(ctx, n, [0, n], a.row_ptr, a.col_idx, a.vals)
    assert _err(lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(dd)).code == 6
    pc = K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).setup(d)
    v = K.DeviceVec(ctx, np.ones(n))
    assert _err(lambda: pc.apply(v, v)).code == 102                       # the sweeps cannot run in place
    assert _err(lambda: pc.apply(np.ones(n + 1))).code == 102
    pc._free()                                                            # use after destroy
    assert _err(lambda: pc.apply(np.ones(n))).code == 2
    assert _err(lambda: pc.info()).code == 2
    b = O.stencil7(5, "varcoef")                                          # a second setup on a new operator replaces the first
    db = to_dev(ctx, b)
    pc.setup(d)
    pc.setup(db)
    xb = np.random.default_rng(2).standard_normal(b.nrows)
    assert np.array_equal(pc.apply(xb), S.Plan(b).apply(xb, 1.0, 1, S.SYMMETRIC_SWEEP))
    assert _err(lambda: pc.apply(np.ones(n))).code == 102
