"""Additive Schwarz with ILU(0) subdomain solves (kryst_amd/csrc/asm_ilu.hip) against the restatement that composes the
oracle on submatrices (tests/asm_ilu_ref.py), bit for bit: the exported sets, owners, factor entries and levels, the shapes that break a
level-scheduled kernel, applies of the three variants, whole solves, RAS convergence and the error paths."""
import numpy as np
import pytest
import scipy.sparse as sp

import kryst_amd as K
from oracle import oracle as O
import asm_ref as A
import asm_ilu_ref as R
import amg_ref as AR
import nonfinite_cases as C

pytestmark = pytest.mark.gpu

MODES = ("ilup0", "ilu0")
VARIANTS = {"as_written": lambda p: p, "grown": lambda p: p.with_overlap(), "restricted": lambda p: p.restricted()}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def make(overlap, sets, variant, mode, nparts=None):
    return VARIANTS[variant](K.AdditiveSchwarz(overlap, sets, nparts)).with_sub_ilu(mode)


def boxes(N, box):
    ptr, idx = K.AdditiveSchwarz.grid_boxes(N, box)
    return [idx[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]


def from_scipy(m):
    m = m.tocsr()
    m.sort_indices()
    return O.Csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)


def check_setup(pc, ref, levels=True):
    """the device's exported set-up against the restatement: sets, owners, the submatrices' patterns, factor values, both levels of every row"""
    ptr, idx, owner, fac = pc.export()
    assert len(fac) == len(ref.gs) and np.array_equal(owner, ref.owner)
    nl = nu = 0
    for k, (g, s, p, f) in enumerate(zip(ref.gs, ref.subs, ref.pcs, fac)):
        assert np.array_equal(idx[ptr[k]:ptr[k + 1]], g), k
        if p is None:
            assert len(f["col"]) == 0
            continue
        assert np.array_equal(f["row_ptr"], s.row_ptr) and np.array_equal(f["col"], s.col_idx), k
        w = R.factor_values(p)
        assert np.array_equal(f["val"], w), k
        rows = np.repeat(np.arange(s.nrows), np.diff(s.row_ptr))
        nl += int(((s.col_idx < rows) & (w != 0.0)).sum()); nu += int(((s.col_idx > rows) & (w != 0.0)).sum())
        if levels:
            ll, lu = R.levels(s, w)
            assert np.array_equal(f["lev_l"], ll) and np.array_equal(f["lev_u"], lu), k
    inf = pc.info()
    assert (inf["nsub"], inf["ext_rows"], inf["max_rows"]) == (len(ref.gs), sum(len(g) for g in ref.gs), max([len(g) for g in ref.gs] + [0]))
    assert (inf["nnz_l"], inf["nnz_u"], inf["cap"]) == (nl, nu, K.AdditiveSchwarz.SUB_ILU_MAX_ROWS)
    assert inf["lds_bytes"] == 8 * max(inf["max_rows"], 1)


def check_apply(ctx, pc, ref, seed=0, n_vec=2):
    rng = np.random.default_rng(seed)
    for _ in range(n_vec):
        r = rng.standard_normal(ref.n)
        r[::5] = -0.0
        ctx.poison_lds()
        z = pc.apply(r)
        assert np.array_equal(z, ref(r))
        assert np.array_equal(np.signbit(z), np.signbit(ref(r)))


def dominant(m):
    """the sparse matrix m with a dominating diagonal"""
    m = sp.csr_matrix(m)
    m = m - sp.diags(m.diagonal())
    return (m + sp.diags(np.asarray(abs(m).sum(axis=1)).ravel() + 1.0)).tocsr()


# ------------------------------------------------------------------------------------------------ set-up
def _sized_case(seed):
    """2 000 rows, random unsymmetric couplings within +-40 rows and a few anywhere; unsorted subdomains of 1, 7, 64, 65, 300 and 1 100 rows:
    row 1999 is in no set, rows 1100 .. 1163 are in two sets, rows 1100 .. 1106 in three"""
    n = 2000
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 6)
    cols = np.clip(np.where(rng.random(len(rows)) < 0.1, rng.integers(0, n, len(rows)), rows + rng.integers(-40, 41, len(rows))), 0, n - 1)
    m = sp.csr_matrix((rng.uniform(-1.0, 1.0, len(rows)), (rows, cols)), shape=(n, n))
    m.sum_duplicates()
    a = from_scipy(dominant(m))
    sets = [rng.permutation(np.arange(0, 1100)), rng.permutation(np.arange(1100, 1400)), rng.permutation(np.arange(1100, 1164)),
            rng.permutation(np.arange(1100, 1107)), rng.permutation(np.arange(1400, 1465)), np.array([1998]),
            rng.permutation(np.arange(1465, 1998))]
    return a, sets


@pytest.mark.parametrize("variant", ["as_written", "restricted"])
@pytest.mark.parametrize("mode", MODES)
def test_setup_every_size(ctx, mode, variant):
    a, sets = _sized_case(11)
    assert sorted(len(g) for g in sets)[:6] == [1, 7, 64, 65, 300, 533] and max(len(g) for g in sets) == 1100
    count = np.zeros(a.nrows, dtype=int)
    for g in sets:
        count[g] += 1
    assert count[1999] == 0 and (count == 2).any() and (count == 3).any()
    d = to_dev(ctx, a)
    ref = R.Setup(a, sets, overlap=0, variant=variant, mode=mode)
    ctx.poison_lds()
    pc = make(0, sets, variant, mode).setup(d)
    check_setup(pc, ref)
    check_apply(ctx, pc, ref)
    z = pc.apply(np.ones(a.nrows))
    assert z[1999] == 0.0 and not np.signbit(z[1999])


@pytest.mark.parametrize("mode", MODES)
def test_uniform_parts_empty_trailing_part_and_more_subdomains_than_workgroups(ctx, mode):
    a = O.stencil7(13, "convdiff")                                          # 2 197 rows
    d = to_dev(ctx, a)
    n = a.nrows
    for p, grown in ((n + 2, False), (40, True), (7, False)):               # n + 2: one row each, two empty parts, more than 8 x 256 workgroups
        parts = A.uniform_parts(n, p)
        assert len(parts) == p and (p != n + 2 or (len(parts[-1]) == 0 and p > 2048))
        variant = "grown" if grown else "as_written"
        ref = R.Setup(a, None, capacity=p, overlap=1, variant=variant, mode=mode)
        pc = make(1, None, variant, mode, nparts=p).setup(d)
        check_setup(pc, ref, levels=(p != n + 2))
        check_apply(ctx, pc, ref, seed=p, n_vec=1)


# ------------------------------------------------------------------------------------------------ shapes that break a level-scheduled kernel
def _shape(name):
    """-> (operator, sets)"""
    rng = np.random.default_rng(5)
    if name == "tridiagonal-300":                                           # 300 levels of one row, in both sweeps
        a = O.Csr.from_dense(O.tridiag(340, -1.0, 2.5, -0.5), keep_zeros=False)
        return a, [rng.permutation(np.arange(20, 320)), np.arange(0, 20)]
    if name == "wide-level-1100":                                           # diagonal plus a few couplings: one level wider than any workgroup
        n = 1200
        m = sp.lil_matrix((n, n))
        for i, j in ((5, 2), (700, 3), (1099, 1098), (2, 900), (400, 800), (800, 1050)):
            m[i, j] = -0.75
        a = from_scipy(dominant(m))
        return a, [rng.permutation(np.arange(0, 1100)), np.arange(1100, 1200)]
    if name == "dense-40":                                                  # long rows: 39 entries in the last row of L and the first of U
        m = rng.uniform(-1.0, 1.0, (60, 60)) * (rng.random((60, 60)) < 0.1)
        m[10:50, 10:50] = rng.uniform(-1.0, 1.0, (40, 40))
        a = from_scipy(dominant(sp.csr_matrix(m)))
        return a, [rng.permutation(np.arange(10, 50)), np.arange(0, 10), np.arange(50, 60)]
    if name == "stored-zeros":                                              # explicit zeros: in the pattern of the factorisation, in no sweep
        a = O.stencil7(7, "varcoef")
        v = a.vals.copy()
        rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
        v[(rng.random(len(v)) < 0.25) & (rows != a.col_idx)] = 0.0
        assert (v == 0.0).sum() > 100
        return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v), A.uniform_parts(a.nrows, 3)
    if name == "sizes-100x":                                                # 10 rows next to 1 000 rows
        a = O.stencil7(11, "convdiff")
        return a, [np.arange(1000, 1010), rng.permutation(np.arange(0, 1000)), np.arange(1010, a.nrows)]
    raise KeyError(name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tridiagonal-300", "wide-level-1100", "dense-40", "stored-zeros", "sizes-100x"])
def test_shapes(ctx, name, mode):
    a, sets = _shape(name)
    d = to_dev(ctx, a)
    ref = R.Setup(a, sets, mode=mode)
    ctx.poison_lds()
    pc = make(0, sets, "as_written", mode).setup(d)
    check_setup(pc, ref)
    _, _, _, fac = pc.export()
    if name == "tridiagonal-300":
        assert fac[0]["lev_l"].max() == 300 and fac[0]["lev_u"].max() == 300 and pc.info()["max_levels"] == 300
    if name == "wide-level-1100":
        assert np.bincount(fac[0]["lev_l"])[1] > 1024 and np.bincount(fac[0]["lev_u"])[1] > 1024
    check_apply(ctx, pc, ref, seed=len(name))


def test_absent_diagonal_ilup0(ctx):
    """row 9 stores no diagonal and nothing below the diagonal in column 9 is non-zero: Ilup(0) sets up, and the backward sweep does not
    divide in that row (ilup.rs:160-164)"""
    a = O.stencil7(4, "poisson")
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v = a.vals.copy()
    v[(a.col_idx == 9) & (rows > 9)] = 0.0
    keep = ~((rows == 9) & (a.col_idx == 9))
    rp = np.zeros(a.nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=a.nrows), out=rp[1:])
    a = O.Csr(a.nrows, a.ncols, rp, a.col_idx[keep], v[keep])
    sets = [np.arange(0, 32)[::-1], np.arange(32, 64)]
    ref = R.Setup(a, sets, mode="ilup0")
    pc = make(0, sets, "as_written", "ilup0").setup(to_dev(ctx, a))
    check_setup(pc, ref)
    check_apply(ctx, pc, ref)


# ------------------------------------------------------------------------------------------------ applies
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("box", [(6, 6, 6), (4, 4, 2)])
@pytest.mark.parametrize("kind", ["poisson", "convdiff", "varcoef"])
def test_applies_12(ctx, kind, box, mode):
    N = 12
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    sets = [g[::-1] for g in boxes(N, box)]
    for variant, overlap in (("as_written", 1), ("grown", 1), ("grown", 2), ("restricted", 1), ("restricted", 2)):
        ref = R.Setup(a, sets, overlap=overlap, variant=variant, mode=mode)
        ctx.poison_lds()
        pc = make(overlap, sets, variant, mode).setup(d)
        ptr, idx, owner, _ = pc.export()
        assert all(np.array_equal(idx[ptr[k]:ptr[k + 1]], g) for k, g in enumerate(ref.gs)) and np.array_equal(owner, ref.owner)
        check_apply(ctx, pc, ref, seed=overlap, n_vec=1)


@pytest.mark.parametrize("variant", ["as_written", "grown", "restricted"])
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_and_signed_zero_vectors(ctx, mode, variant):
    """+-inf, NaN, -0.0, the denormals and the largest double in r: NaNs where the restatement has them, the same bits everywhere else"""
    N = 8
    a = O.stencil7(N, "convdiff")
    d = to_dev(ctx, a)
    sets = boxes(N, (4, 4, 4))
    ref = R.Setup(a, sets, overlap=1, variant=variant, mode=mode)
    pc = make(1, sets, variant, mode).setup(d)
    clean = C.clean_r(a.nrows)
    for rows in ([0], [a.nrows - 1], list(range(3, a.nrows, 37)), list(sets[3][:7])):
        r = C.poisoned(clean, rows)
        with np.errstate(all="ignore"):
            want = ref(r)
        ctx.poison_lds()
        assert C.same_ieee(pc.apply(r), want), rows
    zz = pc.apply(np.full(a.nrows, -0.0))
    assert np.all(zz == 0.0) and not np.signbit(zz).any()


@pytest.mark.parametrize("poison", [None, 1e300])
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_vector_padding(ctx, mode, poison):
    """the result depends on the first n elements of r only (DeviceVec.poison_padding: a quiet NaN by default, and a finite 1e300)"""
    for N in (8, 9):                                                        # 512 rows: the over-read lands in the extra tile; 729: in the last tile
        a = O.stencil7(N, "varcoef")
        d = to_dev(ctx, a)
        sets = boxes(N, (4, 4, 3))
        ref = R.Setup(a, sets, overlap=1, variant="restricted", mode=mode)
        pc = make(1, sets, "restricted", mode).setup(d)
        r = np.random.default_rng(N).standard_normal(a.nrows)
        rv, zv = ctx.vec(r), ctx.vec(np.full(a.nrows, np.nan))
        rv.poison_padding(poison); zv.poison_padding(poison)
        assert rv.padding_dirty() == -(-a.nrows // 512) * 512 + 512 - a.nrows
        pc.apply(rv, zv)
        assert np.array_equal(zv.to_host(), ref(r))


# ------------------------------------------------------------------------------------------------ whole solves
def _pcg_both(ctx, rs, a, d, pc, M, b, tol, max_iters):
    xr, it, code, hist = AR.pcg(a, None, b, tol, max_iters, rs, apply=lambda r, z: M(r))
    assert code == 0
    s = K.PcgSolver(tol, max_iters)
    x = np.zeros(a.nrows)
    st = s.solve(d, pc, b, x)
    assert st.iterations == it
    assert np.array_equal(np.array(s.residual_history), np.array(hist))
    assert np.array_equal(x, xr)
    return it


@pytest.mark.parametrize("variant", ["as_written", "grown"])
@pytest.mark.parametrize("mode", MODES)
def test_pcg_16(ctx, rs, mode, variant):
    N = 16
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    sets = boxes(N, (8, 8, 4))
    ref = R.Setup(a, sets, overlap=1, variant=variant, mode=mode)
    pc = make(1, sets, variant, mode).setup(d)
    it = _pcg_both(ctx, rs, a, d, pc, ref, np.ones(a.nrows), 1e-8, 400)
    assert it > 5


def test_ksp_context_and_session(ctx, rs):
    N = 16
    a = O.stencil7(N, "aniso")
    d = to_dev(ctx, a)
    sets = boxes(N, (8, 8, 8))
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    ref = R.Setup(a, sets, mode="ilu0")
    pc = K.AdditiveSchwarz(0, sets).with_sub_ilu("ilu0").setup(d)
    x1 = np.zeros(a.nrows)
    st1 = K.PcgSolver(1e-8, 300).solve(d, pc, b, x1)
    x2 = np.zeros(a.nrows)
    st2 = K.KspContext(K.SolverKind.Pcg, d, pc=pc, tol=1e-8, max_it=300).solve_context(b, x2)
    assert (st1.iterations, st1.final_residual) == (st2.iterations, st2.final_residual) and np.array_equal(x1, x2)
    x3 = np.zeros(a.nrows)
    pw = K.PC.AdditiveSchwarz(0, sets, sub="ilu0").build(d)
    st3 = K.KspContext(K.SolverKind.Pcg, d, pc=pw, tol=1e-8, max_it=300).solve_context(b, x3)
    xr, it, code, hist = AR.pcg(a, None, b, 1e-8, 300, rs, apply=lambda r, z: ref(r))
    assert st3.iterations == st1.iterations == it and np.array_equal(x3, xr) and np.array_equal(x1, xr)
    steps = 9
    xr, it, code, hist = AR.pcg(a, None, b, 1e-30, steps, rs, apply=lambda r, z: ref(r))
    xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    with K.Session("pcg", d, pc, K.DeviceVec(ctx, b), xv, tol=1e-30, max_iters=steps) as sess:
        sess.step(steps)
        st = sess.end()
        h = sess.residual_history
    assert st.iterations == it == steps
    assert np.array_equal(np.array(h), np.array(hist)) and np.array_equal(xv.to_host(), xr)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("method", ["pcg", "gmres_left", "gmres_right", "bicgstab_rpc"])
def test_uniform_parts_follow_the_oracle(ctx, rs, method, mode):
    """contiguous parts: the preconditioner is the oracle's own ILU of the block-diagonal matrix, so O.solve gives iterations, history and x"""
    N = 14
    a = O.stencil7(N, "poisson" if method == "pcg" else "convdiff")
    d = to_dev(ctx, a)
    parts = 6
    pc = K.AdditiveSchwarz(0, None, parts).with_sub_ilu(mode).setup(d)
    opc = R.MODES[mode](R.block_diagonal(a, A.uniform_parts(a.nrows, parts)))
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x = np.zeros(a.nrows)
    tol, max_iters = 1e-8, 300
    if method == "pcg":
        res = O.solve("pcg", a, b, pc=opc, tol=tol, max_iters=max_iters, rs=rs)
        s = K.PcgSolver(tol, max_iters); st = s.solve(d, pc, b, x)
    elif method.startswith("gmres"):
        side = O.SIDE_LEFT if method == "gmres_left" else O.SIDE_RIGHT
        res = O.solve("gmres", a, b, pc=opc, tol=tol, max_iters=max_iters, restart=20, side=side, rs=rs, raise_on_error=False)
        s = K.GmresSolver(20, tol, max_iters).with_preconditioning(K.Preconditioning.Left if method == "gmres_left" else K.Preconditioning.Right)
        try:
            st = s.solve(d, pc, b, x)
        except K.KError as e:                  # not converged within max_iters: the stats ride on the error
            st = e.stats
    else:
        atol = tol * float(np.linalg.norm(b))
        res = O.solve("bicgstab_rpc", a, b, pc=opc, tol=atol, max_iters=max_iters, rs=rs)
        s = K.BiCgStabRightPcSolver(atol, max_iters); st = s.solve(d, pc, b, x)
    assert (st.iterations, st.converged, st.final_residual) == (res.iterations, res.converged, res.final_residual)
    assert np.array_equal(np.array(s.residual_history), res.history) and np.array_equal(x, res.x)
    assert res.iterations > 3


@pytest.mark.parametrize("solver", ["gmres_left", "bicgstab_rpc", "fgmres"])
def test_ras_converges(ctx, solver):
    """RAS is not symmetric: left GMRES, FGMRES and BiCGStab reach a true relative residual of 1e-8 on the convection-diffusion operator"""
    N = 20
    a = O.stencil7(N, "convdiff")
    d = to_dev(ctx, a)
    pc = K.AdditiveSchwarz(1, boxes(N, (10, 10, 10))).restricted().with_sub_ilu("ilu0").setup(d)
    assert pc.info()["max_rows"] == 10 ** 3 + 3 * 10 ** 2                   # a corner box and one layer of the 7-point graph: three faces
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x = np.zeros(a.nrows)
    if solver == "gmres_left":
        st = K.GmresSolver(30, 1e-12, 1000).with_preconditioning(K.Preconditioning.Left).solve(d, pc, b, x)
    elif solver == "fgmres":
        st = K.FgmresSolver(1e-10, 600, 30).solve_flex(d, pc, b, x)
    else:
        st = K.BiCgStabRightPcSolver(1e-11 * float(np.linalg.norm(b)), 600).solve(d, pc, b, x)
    assert np.linalg.norm(b - a.spmv(x)) / np.linalg.norm(b) <= 1e-8, (solver, st.iterations)


# ------------------------------------------------------------------------------------------------ errors
def _code(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


@pytest.mark.parametrize("mode", MODES)
def test_zero_pivot_reports_the_first_failing_subdomain_and_the_row_of_a(ctx, mode):
    """subdomains 1, 2 and 3 of five fail: the diagonals of their first rows (10, 20, 30: no entry of their own below the diagonal inside
    the subdomain, so no elimination changes them) are stored as 0.0, and the next row has an entry in that column"""
    a = O.Csr.from_dense(O.tridiag(50, -1.0, 2.5, -0.5), keep_zeros=False)
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v = a.vals.copy()
    for row in (10, 20, 30):
        v[(rows == row) & (a.col_idx == row)] = 0.0
    a = O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)
    sets = [np.arange(0, 10), np.arange(10, 20)[::-1], np.arange(20, 30), np.arange(30, 40), np.arange(40, 50)]
    with pytest.raises(O.KrylovError) as oe:
        R.Setup(a, sets, mode=mode)
    R.Setup(a, [sets[0], sets[4]], mode=mode)                               # the other two factorise
    e = _code(lambda: make(0, sets, "as_written", mode).setup(to_dev(ctx, a)))
    assert e.code == oe.value.code == (5 if mode == "ilu0" else 2) and "row 10" in str(e) and "subdomain 1" in str(e)
    if mode == "ilu0":
        assert e.row == 10
    s1 = R.submatrix(a, np.arange(10, 20))                                  # what the global factorisation returns for the same submatrix
    g = _code(lambda: (K.TrueIlu0() if mode == "ilu0" else K.Ilup(0)).setup(to_dev(ctx, s1)))
    assert g.code == e.code and "row 0" in str(g)


def test_the_cap(ctx):
    """16 385 rows are refused with the cap in the message, before and after growth; 16 384 rows set up and apply"""
    n = 16500
    cap = K.AdditiveSchwarz.SUB_ILU_MAX_ROWS
    assert cap == 16384 == R.MAX_ROWS
    # couplings at distance 128 keep the levels few: rows i and i - 128
    m = (sp.diags([-np.ones(n - 128), 2.5 * np.ones(n), -0.5 * np.ones(n - 128)], [-128, 0, 128])).tocsr()
    a = from_scipy(m)
    d = to_dev(ctx, a)
    e = _code(lambda: make(0, [np.arange(cap + 1)], "as_written", "ilu0").setup(d))
    assert e.code == 6 and "16384" in str(e)
    e = _code(lambda: make(1, [np.arange(cap)], "grown", "ilu0").setup(d))    # grows to 16 384 + 116 rows
    assert e.code == 6 and "16384" in str(e) and "subdomain 0" in str(e)
    sets = [np.arange(cap)[::-1], np.arange(cap, n)]
    ref = R.Setup(a, sets, mode="ilu0")
    pc = make(0, sets, "as_written", "ilu0").setup(d)
    inf = pc.info()
    assert inf["max_rows"] == cap and inf["lds_bytes"] == 8 * cap and inf["max_levels"] == 128
    check_apply(ctx, pc, ref, n_vec=1)


def test_errors(ctx, monkeypatch):
    a = O.stencil7(8, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    sets = boxes(8, (4, 4, 4))
    e = _code(lambda: K.AdditiveSchwarz(0, sets).with_sub_ilu(0).setup(d))   # KRYST_ILU_KRYST_COMPAT
    assert e.code == 6
    assert _code(lambda: K.AdditiveSchwarz(0, sets).with_sub_ilu(3).setup(d)).code == 102
    assert _code(lambda: K.AdditiveSchwarz(0, None, 4).with_sub_ilu(0).setup(d)).code == 6
    with pytest.raises(K.KError):
        K.AdditiveSchwarz(0, sets).with_sub_ilu("ilut")
    assert _code(lambda: make(0, [[0, 1], [n]], "as_written", "ilu0").setup(d)).code == 102
    assert _code(lambda: make(0, [[3, 5, 3]], "as_written", "ilu0").setup(d)).code == 102
    assert _code(lambda: make(-1, [[3]], "grown", "ilu0").setup(d)).code == 102
    dd = K.CsrMatrix.from_csr_dist(ctx, n, [0, n], a.row_ptr, a.col_idx, a.vals)
    assert _code(lambda: make(0, [[0]], "as_written", "ilu0").setup(dd)).code == 6
    monkeypatch.setenv("KRYST_ASM_MEM_LIMIT_MB", "0")
    e = _code(lambda: make(0, sets, "as_written", "ilu0").setup(d))
    assert e.code == 100 and "bytes" in str(e) and any(ch.isdigit() for ch in str(e))
    monkeypatch.delenv("KRYST_ASM_MEM_LIMIT_MB")
    pc = make(0, sets, "as_written", "ilu0").setup(d)                       # the context is still usable
    ref = R.Setup(a, sets, mode="ilu0")
    check_apply(ctx, pc, ref, n_vec=1)
    dense = K.AdditiveSchwarz(0, boxes(8, (4, 4, 2))).setup(d)              # info / export dispatch on the kind; the C entry points refuse the other
    assert set(dense.info()) == {"nsub", "ext_rows", "max_rows"} and len(dense.export()[3]) == 16 * 32 * 32
    v = np.zeros(10, dtype=np.int64)
    lib = K.lib()
    assert lib.kryst_pc_asm_ilu_info(dense.h, v.ctypes.data_as(K._ffi.c_i64p), 10) == 102
    assert lib.kryst_pc_asm_ilu_export(dense.h, None, None, None, None, None, None, None, None, None) == 102
    assert lib.kryst_pc_asm_info(pc.h, None, None, None) == 102
    assert lib.kryst_pc_asm_export(pc.h, None, None, None, None) == 102
    jac = K.Jacobi().setup(d)
    assert lib.kryst_pc_asm_ilu_info(jac.h, v.ctypes.data_as(K._ffi.c_i64p), 10) == 102
    z = make(0, [[], []], "as_written", "ilu0").setup(d).apply(np.ones(n))   # empty subdomains: every row uncovered
    assert np.all(z == 0.0)
