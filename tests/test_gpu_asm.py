"""Additive Schwarz (src/preconditioner/asm.rs; kryst_amd/csrc/asm.hip) against the numpy restatement (tests/asm_ref.py), bit for bit:
tiles for every subdomain size class, grown index sets and owners, applies of all three variants, whole PCG solves through
amg_ref.pcg, KspContext and stepping sessions, RAS under GMRES and BiCGStab, and the error paths."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import asm_ref as A
import amg_ref as AR
import bjacobi_ref as BR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    T, V, F = K.reduce_spec()
    return O.Reduce.tiled(T, V, F)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def exported(pc):
    """-> (sets, owner, tiles as row-major b x b arrays) of the device set-up"""
    ptr, idx, owner, t = pc.export()
    gs = [idx[ptr[k]:ptr[k + 1]].astype(np.int64) for k in range(len(ptr) - 1)]
    inv, o = [], 0
    for g in gs:
        b = len(g)
        inv.append(t[o:o + b * b].reshape(b, b).T)       # column-major tiles
        o += b * b
    return gs, owner.astype(np.int64), inv


def boxes(N, box):
    ptr, idx = K.AdditiveSchwarz.grid_boxes(N, box)
    return [idx[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]


VARIANTS = {"as_written": lambda p: p, "grown": lambda p: p.with_overlap(), "restricted": lambda p: p.restricted()}


def make(overlap, sets, variant, nparts=None):
    return VARIANTS[variant](K.AdditiveSchwarz(overlap, sets, nparts))


# ------------------------------------------------------------------------------------------------ tiles
def _dense_case(b, seed, tie=False):
    """n = b + 40 rows: a random dense b x b block with a zero diagonal (off-diagonal pivots) on rows 0..b-1, a random sparse rest"""
    n = b + 40
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.2)
    B = rng.standard_normal((b, b))
    if b > 1:
        np.fill_diagonal(B, 0.0)
    D[:b, :b] = B
    D[b:, b:] += np.diag(np.full(40, 8.0))
    if tie:                                          # the first pivot is a tie between row 10 (wave 0) and row 70 (wave 1)
        D[10, 20] = 9.5
        D[70, 30] = -9.5
    return O.Csr.from_dense(D, keep_zeros=False)


@pytest.mark.parametrize("b", [1, 7, 64, 65, 96, 128])
def test_tiles_every_size(ctx, b):
    a = _dense_case(b, b)
    d = to_dev(ctx, a)
    rng = np.random.default_rng(b + 1)
    sets = [rng.permutation(b), rng.permutation(np.arange(b, b + 40))[:7], rng.permutation(np.arange(b // 2, b + 20))]
    gs_ref, own_ref, inv_ref, zp = A.setup(a, sets)
    assert all(z == -1 for z in zp)
    ctx.poison_lds()
    pc = K.AdditiveSchwarz(0, sets).setup(d)
    gs, own, inv = exported(pc)
    assert all(np.array_equal(u, v) for u, v in zip(gs, gs_ref)) and np.array_equal(own, own_ref)
    assert all(np.array_equal(u, v) for u, v in zip(inv, inv_ref))
    r = rng.standard_normal(a.nrows)
    ctx.poison_lds()
    assert np.array_equal(pc.apply(r), A.apply_loop(a.nrows, gs_ref, inv_ref, r))


@pytest.mark.parametrize("b", [96, 128])
def test_pivot_tie_across_the_waves(ctx, b):
    a = _dense_case(b, 1000 + b, tie=True)
    d = to_dev(ctx, a)
    g = np.arange(b)
    B = BR.block_matrix(a.row_ptr, a.col_idx, a.vals, g)
    assert np.argmax(np.abs(B).ravel()) == 10 * b + 20 and abs(B[70, 30]) == abs(B[10, 20])
    Bi, zp = BR.gauss_jordan(B[None])
    pc = K.AdditiveSchwarz(0, [g[::-1]]).setup(d)
    assert zp[0] == -1 and np.array_equal(exported(pc)[2][0], Bi[0])


# ------------------------------------------------------------------------------------------------ growth
def _nonsym(n, seed):
    rng = np.random.default_rng(seed)
    m = np.diag(np.full(n, 6.0))
    for i in range(n):
        m[i, (i + rng.integers(1, n)) % n] = -1.0
    return O.Csr.from_dense(m, keep_zeros=False)


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("kind", ["poisson", "aniso", "varcoef", "nonsym"])
def test_grown_sets_and_owners(ctx, kind, overlap):
    if kind == "nonsym":
        a = _nonsym(400, overlap)
        rng = np.random.default_rng(overlap)
        sets = [rng.choice(400, 5, replace=False) for _ in range(60)]
    else:
        a = O.stencil7(8, kind)
        sets = [g[::-1] for g in boxes(8, (2, 2, 2))]
    d = to_dev(ctx, a)
    want = A.grow(a.nrows, a.row_ptr, a.col_idx, sets, overlap)
    assert max(len(g) for g in want) <= A.MAX_ROWS
    for variant in ("grown", "restricted"):
        gs, own, inv = exported(make(overlap, sets, variant).setup(d))
        assert len(gs) == len(want) and all(np.array_equal(u, v) for u, v in zip(gs, want))
        assert np.array_equal(own, A.owners(a.nrows, A.sorted_sets(sets)))
    gs, _, _ = exported(make(overlap, sets, "as_written").setup(d))       # as written: overlap ignored
    assert all(np.array_equal(u, v) for u, v in zip(gs, A.sorted_sets(sets)))


def _dense_blocks(nb, bsz, seed):
    """nb dense, diagonally dominant blocks of bsz rows, and one extra entry per row anywhere: rows of bsz + 1 stored entries"""
    n = nb * bsz
    rng = np.random.default_rng(seed)
    m = np.zeros((n, n))
    for k in range(nb):
        m[k * bsz:(k + 1) * bsz, k * bsz:(k + 1) * bsz] = rng.uniform(-1.0, 1.0, (bsz, bsz))
    m[np.arange(n), rng.integers(0, n, n)] = 0.5
    m[np.arange(n), np.arange(n)] = 2.0 * bsz
    return O.Csr.from_dense(m, keep_zeros=False)


def test_growth_in_several_merge_rounds(ctx):
    """wide rows: each subdomain's layer has more than 2048 candidates (with repeats), so the merge in LDS takes several rounds"""
    a = _dense_blocks(10, 50, 7)
    d = to_dev(ctx, a)
    rng = np.random.default_rng(8)
    sets = [rng.choice(np.arange(k * 50, (k + 1) * 50), 30, replace=False) for k in range(10)]
    deg = np.diff(a.row_ptr) + np.bincount(a.col_idx, minlength=a.nrows)          # stored entries of row i of A and of A^T
    assert min(int(deg[g].sum()) for g in sets) > 2048
    want = A.grow(a.nrows, a.row_ptr, a.col_idx, sets, 1)
    assert max(len(g) for g in want) <= A.MAX_ROWS and min(len(g) for g in want) > 64
    pc = make(1, sets, "grown").setup(d)
    gs, own, inv = exported(pc)
    assert all(np.array_equal(u, v) for u, v in zip(gs, want))
    ref, zp = A.tiles(a.row_ptr, a.col_idx, a.vals, want)
    assert all(z == -1 for z in zp) and all(np.array_equal(u, v) for u, v in zip(inv, ref))
    r = rng.standard_normal(a.nrows)
    assert np.array_equal(pc.apply(r), A.Apply(a.nrows, want, ref)(r))


def test_uniform_parts_and_growth(ctx):
    a = O.stencil7(6, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    for p in (0, 1, 3, n, n + 2):
        if p in (0, 1):                                                    # one subdomain of 216 rows: over the cap
            with pytest.raises(K.KError) as e:
                K.AdditiveSchwarz(0, None, p).setup(d)
            assert e.value.code == 6
            continue
        pc = K.AdditiveSchwarz(0, None, p).setup(d)
        gs, own, inv = exported(pc)
        want = A.uniform_parts(n, p)
        assert pc.info()["nsub"] == max(p, 1) and all(np.array_equal(u, v) for u, v in zip(gs, want))
    pc = K.AdditiveSchwarz(1, [], 54).with_overlap().setup(d)
    gs, own, inv = exported(pc)
    want = A.grow(n, a.row_ptr, a.col_idx, A.uniform_parts(n, 54), 1)
    assert all(np.array_equal(u, v) for u, v in zip(gs, want))


# ------------------------------------------------------------------------------------------------ applies
def _mixed_sets(N, seed):
    """unsorted, overlapping subdomains that leave rows uncovered: boxes with a few dropped, shifted copies, a permuted random subset"""
    rng = np.random.default_rng(seed)
    bx = boxes(N, (3, 3, 2))
    keep = [rng.permutation(g) for k, g in enumerate(bx) if k % 5 != 2]
    extra = [rng.permutation(g[: len(g) // 2] + 1) for g in bx[::4] if g.max() + 1 < N ** 3]
    return keep + extra


@pytest.mark.parametrize("variant", ["as_written", "grown", "restricted"])
@pytest.mark.parametrize("kind,N", [("varcoef", 10), ("convdiff", 9)])
def test_apply_index_sets(ctx, variant, kind, N):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    sets = _mixed_sets(N, N)
    gs, own, inv, zp = A.setup(a, sets, overlap=1, variant=variant)
    cov = np.zeros(a.nrows, bool)
    for g in sets:
        cov[g] = True
    assert not cov.all() and sum(len(g) for g in sets) > cov.sum() and all(z == -1 for z in zp)
    ctx.poison_lds()
    pc = make(1, sets, variant).setup(d)
    M = A.Apply(a.nrows, gs, inv, own, restricted=(variant == "restricted"))
    rng = np.random.default_rng(5)
    r = rng.standard_normal(a.nrows)
    r[::5] = -0.0
    ctx.poison_lds()
    z = pc.apply(r)
    assert np.array_equal(z, M(r))
    assert np.array_equal(z, A.apply_loop(a.nrows, gs, inv, r, own, restricted=(variant == "restricted")))
    zz = pc.apply(np.full(a.nrows, -0.0))
    assert np.all(zz == 0.0) and not np.signbit(zz).any()
    ptr = np.zeros(len(sets) + 1, dtype=np.int64)                         # the (ptr, idx) form gives the same preconditioner
    np.cumsum([len(g) for g in sets], out=ptr[1:])
    assert np.array_equal(make(1, (ptr, np.concatenate(sets)), variant).setup(d).apply(r), z)


def test_reference_identity(ctx):
    """asm.rs:125-137 on the device: the 4x4 identity, subdomains [0, 1] and [2, 3]"""
    d = to_dev(ctx, O.Csr.from_dense(np.eye(4), keep_zeros=True))
    r = np.array([1.0, 2.0, 3.0, 4.0])
    assert np.array_equal(K.AdditiveSchwarz(0, [[0, 1], [2, 3]]).setup(d).apply(r), r)
    assert np.array_equal(K.PC.AdditiveSchwarz(0, [[0, 1], [2, 3]]).build(d).apply(r), r)


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


@pytest.mark.parametrize("variant,overlap", [("as_written", 0), ("as_written", 1), ("grown", 1)])
def test_pcg_32(ctx, rs, variant, overlap):
    N = 32
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    sets = boxes(N, (4, 4, 2))
    pc = make(overlap, sets, variant).setup(d)
    gs, own, inv = exported(pc)
    want = A.sorted_sets(sets) if variant == "as_written" else A.grow(a.nrows, a.row_ptr, a.col_idx, sets, overlap)
    assert all(np.array_equal(u, v) for u, v in zip(gs, want))
    sample = np.random.default_rng(32).choice(len(gs), 48, replace=False)    # the tiles of a sample against the restatement
    ref, zp = A.tiles(a.row_ptr, a.col_idx, a.vals, [gs[k] for k in sample])
    assert all(np.array_equal(inv[k], t) for k, t in zip(sample, ref))
    it = _pcg_both(ctx, rs, a, d, pc, A.Apply(a.nrows, gs, inv), np.ones(a.nrows), 1e-8, 400)
    assert it > 5


def test_pcg_96_past_one_fold_chunk(ctx, rs):
    N = 96
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    ptr, idx = K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))
    pc = K.AdditiveSchwarz(0, (ptr, idx)).setup(d)
    gs, own, inv = exported(pc)
    assert a.nrows == 884736 and len(gs) == 27648
    sample = np.random.default_rng(96).choice(len(gs), 64, replace=False)
    ref, zp = A.tiles(a.row_ptr, a.col_idx, a.vals, [np.sort(idx[ptr[k]:ptr[k + 1]]) for k in sample])
    assert all(np.array_equal(inv[k], t) for k, t in zip(sample, ref))
    _pcg_both(ctx, rs, a, d, pc, A.Apply(a.nrows, gs, inv), a.spmv(np.linspace(0.5, 1.5, a.nrows)), 1e-8, 40)


def test_ksp_context_and_session(ctx, rs):
    N = 16
    a = O.stencil7(N, "aniso")
    d = to_dev(ctx, a)
    sets = boxes(N, (4, 4, 2))
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    pc = K.AdditiveSchwarz(1, sets).with_overlap().setup(d)
    x1 = np.zeros(a.nrows)
    st1 = K.PcgSolver(1e-8, 300).solve(d, pc, b, x1)
    x2 = np.zeros(a.nrows)
    st2 = K.KspContext(K.SolverKind.Pcg, d, pc=pc, tol=1e-8, max_it=300).solve_context(b, x2)
    assert (st1.iterations, st1.final_residual) == (st2.iterations, st2.final_residual) and np.array_equal(x1, x2)
    x3 = np.zeros(a.nrows)                                                 # PC.AdditiveSchwarz: as written
    pw = K.PC.AdditiveSchwarz(1, sets).build(d)
    st3 = K.KspContext(K.SolverKind.Pcg, d, pc=pw, tol=1e-8, max_it=300).solve_context(b, x3)
    gs, own, inv = exported(pw)
    assert all(np.array_equal(u, v) for u, v in zip(gs, A.sorted_sets(sets)))
    xr, it, code, hist = AR.pcg(a, None, b, 1e-8, 300, rs, apply=lambda r, z: A.Apply(a.nrows, gs, inv)(r))
    assert st3.iterations == it and np.array_equal(x3, xr)
    steps = 11
    gs, own, inv = exported(pc)
    xr, it, code, hist = AR.pcg(a, None, b, 1e-30, steps, rs, apply=lambda r, z: A.Apply(a.nrows, gs, inv)(r))
    xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    with K.Session("pcg", d, pc, K.DeviceVec(ctx, b), xv, tol=1e-30, max_iters=steps) as sess:
        sess.step(steps)
        st = sess.end()
        h = sess.residual_history
    assert st.iterations == it == steps
    assert np.array_equal(np.array(h), np.array(hist)) and np.array_equal(xv.to_host(), xr)


@pytest.mark.parametrize("solver", ["gmres_left", "bicgstab_rpc", "fgmres"])
def test_ras_converges(ctx, solver):
    """RAS is not symmetric: GMRES, FGMRES and BiCGStab reach a true relative residual of 1e-8 on the convection-diffusion operator.
    (Right-preconditioned GMRES as written re-normalises by ||M^-1 r|| at every restart and stalls here, as it does with other
    preconditioners: DESIGN.md section 4.10.)"""
    N = 20
    a = O.stencil7(N, "convdiff")
    d = to_dev(ctx, a)
    pc = K.AdditiveSchwarz(1, boxes(N, (4, 4, 2))).restricted().setup(d)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x = np.zeros(a.nrows)
    if solver == "gmres_left":
        st = K.GmresSolver(30, 1e-12, 1000).with_preconditioning(K.Preconditioning.Left).solve(d, pc, b, x)
    elif solver == "fgmres":
        st = K.FgmresSolver(1e-10, 600, 30).solve_flex(d, pc, b, x)
    else:
        st = K.BiCgStabRightPcSolver(1e-11 * float(np.linalg.norm(b)), 600).solve(d, pc, b, x)
    assert np.linalg.norm(b - a.spmv(x)) / np.linalg.norm(b) <= 1e-8, (solver, st.iterations)


def _ras_matrix(n, gs, own, inv):
    """RAS as the CSR matrix M with z = M r: row `row` holds (g_o[j], Binv_o[i][j]) of its owner o, ascending j; rows without one are empty.
    Its row sums from 0.0 in stored order are the products kernel's sums, and 0.0 + x = x for them (x is never -0.0)."""
    rp = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for row in range(n):
        o = own[row]
        if o >= 0:
            i = int(np.searchsorted(gs[o], row))
            cols.append(gs[o]); vals.append(inv[o][i, :])
        rp[row + 1] = rp[row] + (len(gs[o]) if o >= 0 else 0)
    return O.Csr(n, n, rp, np.concatenate(cols), np.concatenate(vals))


@pytest.mark.parametrize("kind", ["convdiff", "varcoef"])
def test_ras_right_gmres_follows_the_oracle(ctx, rs, kind):
    """GMRES(30) right-preconditioned with RAS, bit for bit against the oracle's right-preconditioned GMRES with RAS given as explicit
    inverse rows: iterations, history and x.  (As written, right GMRES stops on its own measure of the residual, well above a true
    relative residual of 1e-8 with any preconditioner -- profiles/asm/gmres_right_convdiff20.txt -- so convergence itself is checked with
    left GMRES, FGMRES and BiCGStab above.)"""
    N = 16
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    pc = K.AdditiveSchwarz(1, boxes(N, (4, 4, 2))).restricted().setup(d)
    gs, own, inv = exported(pc)
    m = _ras_matrix(a.nrows, gs, own, inv)
    r = np.random.default_rng(6).standard_normal(a.nrows)
    assert np.array_equal(pc.apply(r), O.Pc.approx_inverse(m).apply(r))
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    res = O.solve("gmres", a, b, pc=O.Pc.approx_inverse(m), tol=1e-10, max_iters=300, restart=30, side=O.SIDE_RIGHT, rs=rs,
                  raise_on_error=False)
    s = K.GmresSolver(30, 1e-10, 300).with_preconditioning(K.Preconditioning.Right)
    x = np.zeros(a.nrows)
    try:
        st = s.solve(d, pc, b, x)
    except K.KError as e:                      # not converged within max_iters: the stats ride on the error
        st = e.stats
    assert (st.iterations, st.converged, st.final_residual) == (res.iterations, res.converged, res.final_residual)
    assert np.array_equal(np.array(s.residual_history), res.history) and np.array_equal(x, res.x)
    assert res.iterations > 5

# ------------------------------------------------------------------------------------------------ errors
def _code(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_errors(ctx, monkeypatch):
    a = O.stencil7(8, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    e = _code(lambda: K.AdditiveSchwarz(2, boxes(8, (4, 4, 4))).with_overlap().setup(d))   # 64 rows grow to 112, then past 128
    assert e.code == 6 and "subdomain 0" in str(e) and "128" in str(e)
    assert _code(lambda: K.AdditiveSchwarz(0, [list(range(129))]).setup(d)).code == 6
    assert _code(lambda: K.AdditiveSchwarz(0, [[0, 1], [n]]).setup(d)).code == 102
    assert _code(lambda: K.AdditiveSchwarz(0, [[-1]]).setup(d)).code == 102
    assert _code(lambda: K.AdditiveSchwarz(0, [[3, 5, 3]]).setup(d)).code == 102
    assert _code(lambda: K.AdditiveSchwarz(-1, [[3]]).with_overlap().setup(d)).code == 102
    dense = np.diag(np.full(20, 4.0))                                    # subdomain 1 is singular
    dense[11, 10:14] = [1.0, 2.0, 3.0, 4.0]
    dense[12, 10:14] = [1.0, 2.0, 3.0, 4.0]
    s = O.Csr.from_dense(dense, keep_zeros=False)
    sets = [[0, 1], [13, 12, 11, 10], [11, 12]]
    e = _code(lambda: K.AdditiveSchwarz(0, sets).setup(to_dev(ctx, s)))
    inv, zp = A.tiles(s.row_ptr, s.col_idx, s.vals, A.sorted_sets(sets))
    assert e.code == 5 and zp[0] == -1 and zp[1] >= 0 and e.row == A.sorted_sets(sets)[1][zp[1]]
    bad = a.vals.copy(); bad[a.row_ptr[7]] = np.nan
    dn = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, bad, ctx=ctx)
    assert a.col_idx[a.row_ptr[7]] == 6 and _code(lambda: K.AdditiveSchwarz(0, [[7, 6]]).setup(dn)).code == 1
    rect = K.CsrMatrix.from_csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0], ctx=ctx)
    assert _code(lambda: K.AdditiveSchwarz(0, [[0]]).setup(rect)).code == 102
    dd = K.CsrMatrix.from_csr_dist(ctx, n, [0, n], a.row_ptr, a.col_idx, a.vals)
    assert _code(lambda: K.AdditiveSchwarz(0, [[0]]).setup(dd)).code == 6
    # over-size: 8 boxes of 64 rows need 8 x 64^2 x 8 bytes of tiles alone; with no device memory allowed the set-up stops before it
    # allocates anything -> KRYST_ERR_HIP with the byte count in the message
    monkeypatch.setenv("KRYST_ASM_MEM_LIMIT_MB", "0")
    e = _code(lambda: K.AdditiveSchwarz(0, boxes(8, (4, 4, 4))).setup(d))
    assert e.code == 100 and "bytes" in str(e)
    monkeypatch.delenv("KRYST_ASM_MEM_LIMIT_MB")
    pc = K.AdditiveSchwarz(0, boxes(8, (4, 4, 4))).setup(d)              # the context is still usable
    r = np.random.default_rng(1).standard_normal(n)
    gs, own, inv = exported(pc)
    assert np.array_equal(pc.apply(r), A.apply_loop(n, gs, inv, r))
    z = K.AdditiveSchwarz(0, [[], []]).setup(d).apply(np.ones(n))        # empty subdomains: every row uncovered
    assert np.all(z == 0.0)


def test_pooled_storage_does_not_reject_a_set_up(ctx, monkeypatch):
    """the memory check counts blocks kept by the device pool as available: a destroyed preconditioner's tiles (2 MiB, kept by the
    pool) would otherwise make a 3 MiB allowance look like 1 MiB to a set-up that needs 2.2 MB"""
    a = O.stencil7(16, "poisson")
    d = to_dev(ctx, a)
    sets = boxes(16, (4, 4, 4))                                           # 64 subdomains of 64 rows: 8 x 64 x 64^2 bytes of tiles
    r = np.random.default_rng(2).standard_normal(a.nrows)
    pc = K.AdditiveSchwarz(0, sets).setup(d)
    want = pc.apply(r)
    pc._free()                                                            # the tile block goes to the pool
    monkeypatch.setenv("KRYST_ASM_MEM_LIMIT_MB", "3")
    pc = K.AdditiveSchwarz(0, sets).setup(d)
    assert np.array_equal(pc.apply(r), want)
    pc._free()
    monkeypatch.setenv("KRYST_ASM_MEM_LIMIT_MB", "2")                     # below the need even with the pool empty
    e = _code(lambda: K.AdditiveSchwarz(0, sets).setup(d))
    assert e.code == 100 and "bytes" in str(e)
