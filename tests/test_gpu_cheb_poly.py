"""The Chebyshev polynomial preconditioner and its spectrum estimate (kryst_amd/csrc/cheb_poly.hip) against the
restatement tests/cheb_poly_ref.py, everything compared on uint64 views: the apply in its fused and unfused forms on operators that cross
every tile, wave and window edge, special input, poisoned padding, a one-rank distributed operator, the Lanczos coefficients and the
bounds made of them, whole PCG / GMRES solves through amg_ref.pcg and krylov_pc_ref.gmres, and the error paths."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import amg_ref as AR
import cheb_poly_ref as CP
import krylov_pc_ref as KR
import multi_rhs_cases as MR
import nonfinite_cases as C

pytestmark = pytest.mark.gpu

PLAIN = {"KRYST_SPMV_COMPRESS": "0", "KRYST_SPMV_DIA": "0"}
DEGREES = (0, 1, 2, 3, 5)
LO, HI = 0.07, 2.3                      # explicit bounds of the apply tests: any 0 < lo < hi gives a polynomial to compare
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same(u, v):
    return bool(np.array_equal(bits(u), bits(v)))


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def to_dist(ctx, a):
    return K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)


def setenv(monkeypatch, env):
    for k in PLAIN:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def long_row_square(n=1200, seed=9):
    """rows 101 (the second row of its lane) and 514 hold 1 000 entries each -- more than one wave window of 896 -- between short rows"""
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cnt = 1000 if i in (101, 514) else int(g.integers(0, 5))
        c = np.union1d(g.choice(n, size=cnt, replace=False), [i]).astype(np.int64)
        v = g.standard_normal(len(c))
        v[c == i] = 3.0 + g.random()
        rows.append((c, v))
    return MR._csr(n, n, rows)


def one_by_one():
    return O.Csr(1, 1, [0, 1], [0], [2.5])


OPERATORS = {
    "stencil7-8": lambda: O.stencil7(8),                     # 512 rows: exactly one tile
    "banded-513": lambda: MR.banded(513),                    # one tile and one row
    "n1": one_by_one,
    "ragged-2003": MR.ragged,                                # empty rows, no diagonal in most rows (w = 0.0 there)
    "long-rows-1200": long_row_square,
    "banded-1025": lambda: MR.banded(1025),
}


@pytest.fixture(scope="module")
def cases(rs):
    """name -> (operator, r, w, {(jacobi, degree): the restatement's z}), computed once"""
    out = {}
    for name, make in OPERATORS.items():
        a = make()
        r = np.random.default_rng(len(name)).standard_normal(a.nrows)
        r[::7] = -0.0
        w = CP.jacobi_w(a)
        out[name] = (a, r, w, {(j, m): CP.apply(a, r, m, LO, HI, w if j else None) for j in (False, True) for m in DEGREES})
    return out


# ------------------------------------------------------------------------------------------------ the apply, both forms
@pytest.mark.parametrize("name", list(OPERATORS))
def test_apply_fused_unfused_and_distributed_equal_the_restatement(ctx, cases, monkeypatch, name):
    a, r, w, want = cases[name]
    forms = set()
    for label, env, make, fused in (("plain", PLAIN, to_dev, True), ("default", {}, to_dev, None), ("one-rank distributed", {}, to_dist, False)):
        setenv(monkeypatch, env)
        d = make(ctx, a)
        for jac in (False, True):
            for m in DEGREES:
                ctx.poison_lds()
                pc = K.ChebyshevPoly(m, LO, HI, jacobi=jac).setup(d)
                inf = pc.info()
                assert (inf["degree"], inf["jacobi"], inf["lambda_min"], inf["lambda_max"]) == (m, jac, LO, HI)
                if fused is not None:
                    assert inf["fused"] == fused, (label, d.encoding())
                assert inf["fused"] == (label != "one-rank distributed" and d.encoding()[0] == "csr")
                forms.add(inf["fused"])
                got = pc.apply(r)
                assert same(got, want[(jac, m)]), (label, jac, m, int(np.sum(bits(got) != bits(want[(jac, m)]))))
                assert same(pc.apply(r), got)                            # its buffers carry nothing from one apply to the next
    assert forms == {True, False}


def test_one_tile_stencil_plain_is_fused_and_default_form_is_not(ctx, cases, monkeypatch):
    a, r, w, want = cases["stencil7-8"]
    setenv(monkeypatch, PLAIN)
    plain = K.CsrMatrix.stencil7(8, "poisson", ctx=ctx)
    p1 = K.ChebyshevPoly(5, LO, HI).setup(plain)
    assert plain.encoding()[0] == "csr" and p1.info()["fused"]
    z1 = p1.apply(r)
    setenv(monkeypatch, {})
    dflt = K.CsrMatrix.stencil7(8, "poisson", ctx=ctx)
    p2 = K.ChebyshevPoly(5, LO, HI).setup(dflt)
    assert dflt.encoding()[0] != "csr" and not p2.info()["fused"]
    z2 = p2.apply(r)
    assert same(z1, z2) and same(z1, want[(True, 5)])
    assert same(K.PC.ChebyshevPoly(5, LO, HI).build(dflt).apply(r), z1)


def test_fused_step_in_the_slab_order_of_the_tiles(ctx, monkeypatch):
    """what the fused kernel runs at 512^3: the plain kernel's slab order of the tiles (empty slots included), on the 100 x 250 x 6 box of
    test_spmv_slab_order_of_the_tiles_bit_exact with its lowered thresholds; the same bits as in the natural order"""
    import scipy.sparse as sp
    e = lambda n: sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])      # noqa: E731
    pat = (sp.kron(sp.identity(6), sp.kron(sp.identity(250), e(100))) + sp.kron(sp.identity(6), sp.kron(e(250), sp.identity(100))) +
           sp.kron(e(6), sp.identity(25000))).tocsr()
    pat.sort_indices()
    rng = np.random.default_rng(77)
    a = O.Csr(pat.shape[0], pat.shape[1], pat.indptr, pat.indices, rng.standard_normal(pat.nnz))
    setenv(monkeypatch, PLAIN)
    monkeypatch.setenv("KRYST_SPMV_ORDER", "2"); monkeypatch.setenv("KRYST_SPMV_ORDER_MIN_PLANE", "8192")
    d = to_dev(ctx, a)
    assert d.encoding()[0] == "csr" and d.tile_order()["in_use"], d.tile_order()
    r = rng.standard_normal(a.nrows)
    w = CP.jacobi_w(a)
    for jac, m in ((True, 3), (False, 1)):
        pc = K.ChebyshevPoly(m, LO, HI, jacobi=jac).setup(d)
        assert pc.info()["fused"]
        want = CP.apply(a, r, m, LO, HI, w if jac else None)
        monkeypatch.setenv("KRYST_SPMV_ORDER", "2")
        assert d.tile_order()["in_use"] and same(pc.apply(r), want)
        monkeypatch.setenv("KRYST_SPMV_ORDER", "0")              # read per launch: the same object in the natural order
        assert not d.tile_order()["in_use"] and same(pc.apply(r), want)


def test_device_vectors_r_is_never_written_and_z_is_not_read(ctx, cases, monkeypatch):
    a, r, w, want = cases["banded-1025"]
    for env in (PLAIN, {}):
        setenv(monkeypatch, env)
        d = to_dev(ctx, a)
        pc = K.ChebyshevPoly(3, LO, HI).setup(d)
        rv = K.DeviceVec(ctx, r)
        zv = K.DeviceVec(ctx, np.full(a.nrows, np.nan))
        assert pc.apply(rv, zv) is zv
        assert same(zv.to_host(), want[(True, 3)]) and same(rv.to_host(), r)


def test_destroyed_in_any_order_relative_to_the_operator(ctx, cases):
    a, r, w, want = cases["banded-513"]
    for first in ("operator", "preconditioner"):
        d = to_dev(ctx, a)
        pc = K.ChebyshevPoly(2, LO, HI).setup(d)
        assert same(pc.apply(r), want[(True, 2)])
        if first == "operator":
            pc._a = None
            K.lib().kryst_csr_destroy(d.h); d.h = None
            pc._free()
        else:
            pc._free()
            del d
    d = to_dev(ctx, a)
    assert same(K.ChebyshevPoly(2, LO, HI).setup(d).apply(r), want[(True, 2)])


# ------------------------------------------------------------------------------------------------ special input, poisoned padding
@pytest.mark.parametrize("form", ["fused", "unfused"])
def test_special_input(ctx, monkeypatch, form):
    """r holding NaN, +-inf, -0.0, denormals and the largest double (nonfinite_cases.POISON) at the first, last and middle row and across a tile
    edge: NaNs at the same places, every other entry the same 64 bits"""
    a = MR.banded(1025)
    w = CP.jacobi_w(a)
    setenv(monkeypatch, PLAIN if form == "fused" else {})
    d = to_dev(ctx, a) if form == "fused" else to_dist(ctx, a)
    clean = C.clean_r(a.nrows)
    for rows in ([0, 1024, 512, 511, 513, 300, 700], [5, 6, 7, 8, 9, 10, 11], [1018, 1019, 1020, 1021, 1022, 1023, 1024]):
        for shift in range(0, 7, 3):
            r = C.poisoned(clean, rows, C.POISON[shift:] + C.POISON[:shift])
            for jac in (False, True):
                for m in (0, 1, 3):
                    pc = K.ChebyshevPoly(m, LO, HI, jacobi=jac).setup(d)
                    assert pc.info()["fused"] == (form == "fused")
                    got, want = pc.apply(r), CP.apply(a, r, m, LO, HI, w if jac else None)
                    assert C.same_ieee(got, want), (rows, shift, jac, m)
                    assert np.isnan(want).any() and not np.isnan(want).all()


@pytest.mark.parametrize("poison", [QNAN, 1e300], ids=["qnan", "1e300"])
@pytest.mark.parametrize("n", [1, 511, 512, 513])
def test_poisoned_padding(ctx, monkeypatch, n, poison):
    """quiet NaN and 1e300 behind r and z (the rule of tests/test_gpu_padding.py): the first n results are those of clean vectors and of the
    restatement"""
    a = MR.banded(n)
    w = CP.jacobi_w(a)
    r = np.random.default_rng(n).standard_normal(n)
    pad = -(-n // 512) * 512 + 512 - n
    for env, make in ((PLAIN, to_dev), ({}, to_dist)):
        setenv(monkeypatch, env)
        d = make(ctx, a)
        for jac in (False, True):
            for m in (0, 1, 4):
                pc = K.ChebyshevPoly(m, LO, HI, jacobi=jac).setup(d)
                want = CP.apply(a, r, m, LO, HI, w if jac else None)
                for p in (None, poison):
                    rv, zv = ctx.vec(r), ctx.vec(np.full(n, np.nan))
                    if p is not None:
                        rv.poison_padding(p); zv.poison_padding(p)
                        assert rv.padding_dirty() == pad and zv.padding_dirty() == pad
                    pc.apply(rv, zv)
                    assert same(zv.to_host(), want), (n, jac, m, p, pc.info()["fused"])
                    assert same(rv.to_host(), r)


# ------------------------------------------------------------------------------------------------ the spectrum estimate
def symmetrised_ragged(shift=None):
    import scipy.sparse as sp
    a = MR.ragged()
    m = sp.csr_matrix((a.vals, a.col_idx, a.row_ptr), shape=(a.nrows, a.nrows))
    m = (m + m.T).tocsr()
    if shift is not None:
        m = (m + sp.diags(np.asarray(abs(m).sum(axis=1)).ravel() + shift)).tocsr()
    m.sort_indices()
    return O.Csr(a.nrows, a.nrows, m.indptr, m.indices, m.data)


def diagonal_matrix(n=700):
    """entries 4^k: w, its square root and s a s = 1 are exact, so S = I, t = q and alpha_0 = dot(q, q)"""
    return O.Csr(n, n, np.arange(n + 1), np.arange(n), 4.0 ** (np.arange(n) % 6))


def huge_diagonal(n=700):
    return O.Csr(n, n, np.arange(n + 1), np.arange(n), np.linspace(0.5, 4.0, n) * 1e200)


ESTIMATES = {                                                  # name -> (operator, jacobi, steps, seed)
    "poisson-8-jacobi": (lambda: O.stencil7(8), True, 10, 0x5EED),
    "poisson-8-none": (lambda: O.stencil7(8), False, 10, 0x5EED),
    "ragged-symmetrised-none": (symmetrised_ragged, False, 10, 0x5EED),
    "ragged-symmetrised-dominant-jacobi": (lambda: symmetrised_ragged(0.5), True, 64, 7),
    "diagonal-jacobi": (diagonal_matrix, True, 10, 1),         # seed 1: dot(q_0, q_0) rounds to 1.0, so t = q - 1.0 q = 0 and beta_0 = 0: one step
    "huge-diagonal-none": (huge_diagonal, False, 10, 0x5EED),  # dot(t, t) overflows: beta_0 = inf, one step
    "one-row": (one_by_one, True, 10, 0x5EED),                 # min(steps, n) = 1
    "poisson-81-jacobi": (lambda: O.stencil7(81), True, 3, 0x5EED),   # 531 441 rows: past one fold chunk of 524 288
}


@pytest.mark.parametrize("name", list(ESTIMATES))
def test_estimate_equals_the_restatement(ctx, rs, name):
    make, jac, steps, seed = ESTIMATES[name]
    a = make()
    d = K.CsrMatrix.stencil7(81, "poisson", ctx=ctx) if name == "poisson-81-jacobi" else to_dev(ctx, a)
    want = CP.estimate(a, rs, jac, steps, seed)
    try:
        got = K.estimate_spectrum(d, jac, steps, seed)
        code = 0
    except K.KError as e:                                      # an indefinite T: the coefficients are not returned through the exception
        got, code = None, e.code
    if name == "ragged-symmetrised-none":
        print(name, want["theta_min"], want["theta_max"], code)
    assert (code == 0) == (want["theta_max"] > 0.0), (code, want["theta_max"])
    if got is not None:
        assert got["steps_done"] == want["steps_done"]
        for key in ("alpha", "beta", "theta_min", "theta_max", "gershgorin"):
            assert same(got[key], want[key]), (key, got[key], want[key])
    if name == "diagonal-jacobi":
        assert want["steps_done"] == 1 and want["beta"][0] == 0.0 and want["theta_max"] == want["alpha"][0] == 1.0
    if name == "huge-diagonal-none":
        assert want["steps_done"] == 1 and want["beta"][0] == np.inf and np.isfinite(want["theta_max"])
    if name == "one-row":
        assert want["steps_done"] == 1
    if name == "poisson-81-jacobi":
        assert want["steps_done"] == 3 and a.nrows > 524288


def test_default_bounds_are_made_of_the_estimate(ctx, rs):
    a = O.stencil7(8)
    d = to_dev(ctx, a)
    lo, hi = CP.default_bounds(CP.estimate(a, rs))
    pc = K.ChebyshevPoly(4).setup(d)
    inf = pc.info()
    assert same([inf["lambda_min"], inf["lambda_max"]], [lo, hi]) and pc.estimate["steps_done"] == 10
    lo2, hi2 = CP.default_bounds(CP.estimate(a, rs, False, 7, 99), 12.0, 1.3)
    inf = K.ChebyshevPoly(4, jacobi=False, steps=7, ratio=12.0, safety=1.3, seed=99).setup(d).info()
    assert same([inf["lambda_min"], inf["lambda_max"]], [lo2, hi2])
    inf = K.ChebyshevPoly(4, lambda_max=3.0).setup(d).info()             # one bound given: the other follows it
    assert (inf["lambda_min"], inf["lambda_max"]) == (3.0 / 30.0, 3.0)


# ------------------------------------------------------------------------------------------------ whole solves
def _stats(fn):
    try:
        return fn()
    except K.KError as e:
        assert e.stats is not None
        return e.stats


@pytest.mark.parametrize("kind,N,form", [("poisson", 8, "plain"), ("poisson", 8, "default"), ("aniso", 16, "plain"), ("aniso", 16, "default")])
def test_pcg_equals_the_numpy_solver_over_apply(ctx, rs, monkeypatch, kind, N, form):
    """degree 4, default bounds, tol 1e-8; the cap of 500 is far beyond the 13 - 20 iterations taken, so the `done` gate of every kernel of the
    apply is exercised by the launches the solver has enqueued ahead"""
    setenv(monkeypatch, PLAIN if form == "plain" else {})
    a = O.stencil7(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    b = a.spmv(np.ones(a.nrows))
    pc = K.ChebyshevPoly(4).setup(d)
    assert pc.info()["fused"] == (form == "plain")
    w = CP.jacobi_w(a)
    lo, hi = CP.default_bounds(CP.estimate(a, rs))
    xr, it, code, hist = AR.pcg(a, None, b, 1e-8, 500, rs, apply=CP.make_apply(a, 4, lo, hi, w, two_args=True))
    assert code == 0 and 3 < it < 40
    s = K.PcgSolver(1e-8, 500)
    x = np.zeros(a.nrows)
    st = s.solve(d, pc, b, x)
    assert st.iterations == it and bool(st.converged)
    assert same(s.residual_history, hist) and same(x, xr)
    x2 = np.zeros(a.nrows)
    st2 = K.KspContext(K.SolverKind.Pcg, d, pc=pc, tol=1e-8, max_it=500).solve_context(b, x2)
    assert st2.iterations == it and same(x2, xr)
    if N == 16:                                                          # what it is for: 20 iterations against Jacobi's 79
        xj = np.zeros(a.nrows)
        itj = K.PcgSolver(1e-8, 500).solve(d, K.Jacobi().setup(d), b, xj).iterations
        assert 2 * it <= itj, (it, itj)


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("form", ["plain", "default"])
def test_gmres_equals_the_numpy_solver_over_apply(ctx, rs, monkeypatch, side, form):
    setenv(monkeypatch, PLAIN if form == "plain" else {})
    a = O.stencil7(8, "convdiff")
    d = K.CsrMatrix.stencil7(8, "convdiff", ctx=ctx)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    lo, hi = 0.06, 2.0
    pc = K.ChebyshevPoly(2, lo, hi).setup(d)
    assert pc.info()["fused"] == (form == "plain")
    M = CP.make_apply(a, 2, lo, hi, CP.jacobi_w(a))
    # (restarted GMRES as written stalls on this operator with Jacobi too: the run is cut off inside its fifth cycle, which is no obstacle to comparing bits)
    xr, it, fr, conv, hist = KR.gmres(a, M, side, b, 10, 1e-8, 45, rs)
    assert it == 45 and np.all(np.isfinite(hist))
    s = K.GmresSolver(10, 1e-8, 45).with_preconditioning(K.Preconditioning.Left if side == "left" else K.Preconditioning.Right)
    x = np.zeros(a.nrows)
    st = _stats(lambda: s.solve(d, pc, b, x))
    assert (st.iterations, bool(st.converged)) == (it, conv) and same(st.final_residual, fr)
    assert same(s.residual_history, hist) and same(x, xr)


def test_fgmres_and_bicgstab_take_it(ctx, rs):
    a = O.stencil7(8, "convdiff")
    d = K.CsrMatrix.stencil7(8, "convdiff", ctx=ctx)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    pc = K.ChebyshevPoly(2, 0.06, 2.0).setup(d)
    M = CP.make_apply(a, 2, 0.06, 2.0, CP.jacobi_w(a))
    atol = 1e-8 * float(np.linalg.norm(b))
    xr, it, fr, conv, hist = KR.bicgstab_rpc(a, M, b, atol, 200, rs)
    s = K.BiCgStabRightPcSolver(atol, 200)
    x = np.zeros(a.nrows)
    st = _stats(lambda: s.solve(d, pc, b, x))
    assert st.iterations == it and same(s.residual_history, hist) and same(x, xr)
    x = np.zeros(a.nrows)
    st = K.FgmresSolver(1e-8, 200, 10).solve_flex(d, pc, b, x)
    assert bool(st.converged) and np.linalg.norm(b - a.spmv(x)) <= 1e-6 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------------------ errors
def _err(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_errors(ctx):
    a = O.stencil7(8)
    n = a.nrows
    d = to_dev(ctx, a)
    rect = K.CsrMatrix.from_csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0], ctx=ctx)
    assert _err(lambda: K.ChebyshevPoly(2, 0.1, 2.0).setup(rect)).code == 102
    assert _err(lambda: K.estimate_spectrum(rect)).code == 102
    for deg in (-1, 65):
        assert _err(lambda: K.ChebyshevPoly(deg, 0.1, 2.0).setup(d)).code == 102
    assert K.ChebyshevPoly(64, 0.1, 2.0).setup(d).info()["degree"] == 64
    for lo, hi in ((0.0, 2.0), (-0.5, 2.0), (2.0, 2.0), (3.0, 2.0), (np.nan, 2.0), (0.1, np.nan), (0.1, np.inf), (-np.inf, 2.0)):
        assert _err(lambda: K.ChebyshevPoly(2, lo, hi).setup(d)).code == 102, (lo, hi)
    for steps in (0, -3, 65):
        assert _err(lambda: K.estimate_spectrum(d, True, steps)).code == 102
    assert K.estimate_spectrum(d, True, 64)["steps_done"] == 64
    # a one-rank distributed operator: bounds must be passed
    dd = to_dist(ctx, a)
    assert _err(lambda: K.estimate_spectrum(dd)).code == 6
    assert _err(lambda: K.ChebyshevPoly(2).setup(dd)).code == 6
    assert not K.ChebyshevPoly(2, 0.1, 2.0).setup(dd).info()["fused"]
    # Jacobi scaling and a diagonal the estimate cannot use: status 4 and the lowest such row
    for bad, row in ((0.0, 37), (-6.0, 300), (np.inf, 511), (np.nan, 0), (5e-324, 100)):
        vals = a.vals.copy()
        k = int(a.row_ptr[row]) + int(np.flatnonzero(a.col_idx[a.row_ptr[row]:a.row_ptr[row + 1]] == row)[0])
        vals[k] = bad
        if row == 300:
            vals[int(a.row_ptr[400]) + int(np.flatnonzero(a.col_idx[a.row_ptr[400]:a.row_ptr[401]] == 400)[0])] = 0.0   # a second, later one
        bd = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, vals, ctx=ctx)
        for fn in (lambda: K.estimate_spectrum(bd), lambda: K.ChebyshevPoly(3).setup(bd)):
            e = _err(fn)
            assert e.code == 4 and e.row == row and K.lib().kryst_hip_last_error_row() == row, (bad, e.code, e.row)
        with pytest.raises(CP.IndefiniteDiagonal) as ie:
            CP.checked_w(O.Csr(n, n, a.row_ptr, a.col_idx, vals))
        assert ie.value.row == row
    missing = O.Csr(3, 3, [0, 2, 3, 5], [0, 1, 0, 1, 2], [2.0, -1.0, -1.0, -1.0, 2.0])       # row 1 stores no diagonal
    e = _err(lambda: K.estimate_spectrum(to_dev(ctx, missing)))
    assert e.code == 4 and e.row == 1
    # without scaling the diagonal is not looked at; a negative definite operator is IndefiniteMatrix, a non-finite entry FactorError
    neg = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, -a.vals, ctx=ctx)
    assert _err(lambda: K.estimate_spectrum(neg, False)).code == 3
    vals = a.vals.copy(); vals[5] = np.inf
    assert _err(lambda: K.estimate_spectrum(K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, vals, ctx=ctx), False)).code == 1
    # r aliasing z is refused before any launch
    pc = K.ChebyshevPoly(2, 0.1, 2.0).setup(d)
    v = K.DeviceVec(ctx, np.ones(n))
    assert _err(lambda: pc.apply(v, v)).code == 102 and same(v.to_host(), np.ones(n))
    # the info call knows its own kind only; the as-written Chebyshev objects are what they were
    jac = K.Jacobi().setup(d)
    assert K.lib().kryst_pc_chebyshev_poly_info(jac.h, None, None, None, None, None) == 102
    assert _err(lambda: K.Chebyshev(3).setup(d).apply(np.ones(n))).code == 2
    assert _err(lambda: K.PC.Chebyshev(3).build(d).apply(np.ones(n))).code == 2
