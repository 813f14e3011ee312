"""Block Jacobi (BlockJacobi, src/preconditioner/block_jacobi.rs; kryst_amd/csrc/block_jacobi.hip) against the numpy restatement of its
set-up (tests/bjacobi_ref.py) and, through it, against the oracle: with M_ref = the restated block inverse as CSR, block Jacobi IS the
oracle's ApproxInv preconditioner (z = kro_spmv(M_ref, r)), so tiles, applies and whole solves are compared bit for bit."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import bjacobi_ref as R

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


def uniform_ref(a, bsize):
    gs, inv, zp = R.tiles_uniform(a.row_ptr, a.col_idx, a.vals, a.nrows, bsize)
    assert all(z == -1 for z in zp)
    return O.Csr(a.nrows, a.nrows, *R.m_ref_uniform(a.nrows, bsize, inv))


def sets_ref(a, blocks):
    gs, inv, zp = R.tiles_of(a.row_ptr, a.col_idx, a.vals, blocks)
    assert all(z == -1 for z in zp)
    return O.Csr(a.nrows, a.nrows, *R.m_ref(a.nrows, gs, inv))


def same_csr(pc, m):
    rp, ci, va = pc.inverse_csr()
    return np.array_equal(rp, m.row_ptr) and np.array_equal(ci.astype(np.int64), m.col_idx) and np.array_equal(va, m.vals)


def random_r(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


# ------------------------------------------------------------------------------------------------ tiles and applies
@pytest.mark.parametrize("kind,N", [("poisson", 8), ("aniso", 13), ("convdiff", 16), ("varcoef", 20), ("poisson", 32)])
@pytest.mark.parametrize("bsize", [1, 2, 3, 7, 8, 16, 33, 64])
def test_uniform_tiles_and_apply(ctx, kind, N, bsize):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    m = uniform_ref(a, bsize)
    ctx.poison_lds()
    pc = K.BlockJacobi.uniform(bsize).setup(d)
    assert same_csr(pc, m)
    r = random_r(a.nrows, N * 100 + bsize)
    ctx.poison_lds()
    assert np.array_equal(pc.apply(r), O.Pc.approx_inverse(m).apply(r))


@pytest.mark.parametrize("kind,N", [("poisson", 12), ("aniso", 16), ("varcoef", 10)])
def test_uniform_one_is_jacobi(ctx, kind, N):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    r = random_r(a.nrows, 3)
    z = K.BlockJacobi.uniform(1).setup(d).apply(r)
    assert np.array_equal(z, K.Jacobi().setup(d).apply(r))
    assert np.array_equal(z, O.Pc.jacobi(a).apply(r))


def _zero_diag_operator(n, bsize, seed):
    """Random nonsymmetric operator: dense random blocks on the block diagonal with a ZERO diagonal (every block of more than one row
    needs off-diagonal pivots), some entries between blocks, some explicitly stored zeros."""
    rng = np.random.default_rng(seed)
    dense = np.zeros((n, n))
    for s in range(0, n, bsize):
        e = min(s + bsize, n)
        blk = rng.standard_normal((e - s, e - s))
        if e - s > 1:
            np.fill_diagonal(blk, 0.0)
        dense[s:e, s:e] = blk
    far = rng.random((n, n)) < 0.02
    dense[far] = rng.standard_normal(int(far.sum()))
    keep = dense != 0.0
    keep |= (rng.random((n, n)) < 0.01)                 # explicit zeros: stored, count as entries
    np.fill_diagonal(keep, True)                        # the diagonal is stored -- as 0.0 inside every block
    rows, cols = np.nonzero(keep)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return O.Csr(n, n, rp, cols, dense[rows, cols])


@pytest.mark.parametrize("n,bsize", [(200, 5), (300, 16), (257, 64), (190, 32)])
def test_tiles_with_offdiagonal_pivots(ctx, n, bsize):
    a = _zero_diag_operator(n, bsize, n + bsize)
    d = to_dev(ctx, a)
    m = uniform_ref(a, bsize)
    pc = K.BlockJacobi.uniform(bsize).setup(d)
    assert same_csr(pc, m)
    r = random_r(n, 11)
    assert np.array_equal(pc.apply(r), O.Pc.approx_inverse(m).apply(r))
    # the index-set form with the same (shuffled) blocks gives the same preconditioner
    rng = np.random.default_rng(n)
    blocks = [rng.permutation(np.arange(s, min(s + bsize, n))) for s in range(0, n, bsize)]
    pcs = K.BlockJacobi(blocks).setup(d)
    assert same_csr(pcs, m)
    assert np.array_equal(pcs.apply(r), O.Pc.approx_inverse(m).apply(r))


def _index_sets(n, seed, count=60):
    """Unsorted index sets of mixed sizes 0..64 that overlap and leave rows uncovered."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 65, count)
    sizes[:3] = (0, 64, 1)
    blocks = [rng.choice(n, size=int(s), replace=False) for s in sizes]
    return blocks


@pytest.mark.parametrize("kind,N,seed", [("poisson", 10, 1), ("convdiff", 12, 2), ("varcoef", 9, 3)])
def test_index_sets_unsorted_overlapping_uncovered(ctx, kind, N, seed):
    a = O.stencil7(N, kind)
    # a diagonally dominant operator keeps every sub-block nonsingular
    d = to_dev(ctx, a)
    blocks = _index_sets(a.nrows, seed)
    covered = np.zeros(a.nrows, bool)
    for g in blocks:
        covered[g] = True
    assert not covered.all() and sum(len(g) for g in blocks) > covered.sum()     # uncovered rows and overlaps
    m = sets_ref(a, blocks)
    ctx.poison_lds()
    pc = K.BlockJacobi(blocks).setup(d)
    assert same_csr(pc, m)
    r = random_r(a.nrows, seed)
    ctx.poison_lds()
    z = pc.apply(r)
    assert np.array_equal(z, O.Pc.approx_inverse(m).apply(r))
    assert np.all(z[~covered] == 0.0) and not np.any(np.signbit(z[~covered]))
    # the (ptr, idx) form and PC.BlockJacobi give the same preconditioner
    ptr = np.zeros(len(blocks) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in blocks], out=ptr[1:])
    assert same_csr(K.BlockJacobi((ptr, np.concatenate(blocks))).setup(d), m)
    assert same_csr(K.PC.BlockJacobi(blocks).build(d), m)


# ------------------------------------------------------------------------------------------------ whole solves
def _check(res, st, hist, x):
    assert (st.iterations, st.converged) == (res.iterations, res.converged)
    assert st.final_residual == res.final_residual
    assert np.array_equal(np.array(hist), res.history)
    assert np.array_equal(x, res.x)


SOLVES = ["pcg", "gmres_left", "gmres_right", "fgmres", "bicgstab_rpc"]


def _solve_both(ctx, rs, method, a, d, kpc, m, b, tol, max_iters):
    opc = O.Pc.approx_inverse(m)
    x = np.zeros(a.nrows)
    if method == "pcg":
        res = O.solve("pcg", a, b, pc=opc, tol=tol, max_iters=max_iters, rs=rs)
        s = K.PcgSolver(tol, max_iters); st = s.solve(d, kpc, b, x)
    elif method.startswith("gmres"):
        side = O.SIDE_LEFT if method == "gmres_left" else O.SIDE_RIGHT
        res = O.solve("gmres", a, b, pc=opc, tol=tol, max_iters=max_iters, restart=20, side=side, rs=rs)
        s = K.GmresSolver(20, tol, max_iters).with_preconditioning(K.Preconditioning.Left if method == "gmres_left" else K.Preconditioning.Right)
        st = s.solve(d, kpc, b, x)
    elif method == "fgmres":
        res = O.solve("fgmres", a, b, pc=opc, tol=tol, max_iters=max_iters, restart=20, rs=rs)
        s = K.FgmresSolver(tol, max_iters, 20); st = s.solve_flex(d, kpc, b, x)
    else:
        atol = tol * float(np.linalg.norm(b))                                  # BiCGStab's tolerance is absolute (bicgstab.rs)
        res = O.solve("bicgstab_rpc", a, b, pc=opc, tol=atol, max_iters=max_iters, rs=rs)
        s = K.BiCgStabRightPcSolver(atol, max_iters); st = s.solve(d, kpc, b, x)
    _check(res, st, s.residual_history, x)
    return res


@pytest.mark.parametrize("method", SOLVES)
@pytest.mark.parametrize("kind,N,bsize", [("poisson", 16, 8), ("aniso", 24, 16), ("convdiff", 20, 7), ("varcoef", 32, 64),
                                          ("aniso", 64, 8)])
def test_solves_bit_exact(ctx, rs, method, kind, N, bsize):
    if method == "pcg" and kind == "convdiff":
        pytest.skip("PCG needs a symmetric operator")
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    m = uniform_ref(a, bsize)
    pc = K.BlockJacobi.uniform(bsize).setup(d)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    res = _solve_both(ctx, rs, method, a, d, pc, m, b, 1e-8, 300)
    assert res.iterations > 1


@pytest.mark.parametrize("method", ["pcg", "gmres_right", "bicgstab_rpc"])
def test_solves_index_sets(ctx, rs, method):
    a = O.stencil7(16, "poisson")
    d = to_dev(ctx, a)
    rng = np.random.default_rng(4)
    perm = rng.permutation(a.nrows)
    blocks = [perm[s:s + 24] for s in range(0, a.nrows, 24)]        # every row covered once, blocks of scattered rows
    m = sets_ref(a, blocks)
    pc = K.BlockJacobi(blocks).setup(d)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    _solve_both(ctx, rs, method, a, d, pc, m, b, 1e-8, 300)


def test_solve_aniso_128_b16(ctx, rs):
    a = O.stencil7(128, "aniso")
    d = to_dev(ctx, a)
    m = uniform_ref(a, 16)
    pc = K.BlockJacobi.uniform(16).setup(d)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    _solve_both(ctx, rs, "pcg", a, d, pc, m, b, 1e-8, 400)


@pytest.mark.parametrize("kind", [K.SolverKind.Pcg, K.SolverKind.GmresRight])
def test_ksp_context(ctx, rs, kind):
    a = O.stencil7(20, "aniso")
    d = to_dev(ctx, a)
    blocks = R.uniform_blocks(a.nrows, 20)
    m = sets_ref(a, blocks)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    ksp = K.KspContext(kind, d, pc=K.PC.BlockJacobi(blocks).build(d), tol=1e-8, max_it=300, restart=20)
    x = np.zeros(a.nrows)
    st = ksp.solve_context(b, x)
    if kind == K.SolverKind.Pcg:
        res = O.solve("pcg", a, b, pc=O.Pc.approx_inverse(m), tol=1e-8, max_iters=300, rs=rs)
    else:
        res = O.solve("gmres", a, b, pc=O.Pc.approx_inverse(m), tol=1e-8, max_iters=300, restart=20, side=O.SIDE_RIGHT, rs=rs)
    assert (st.iterations, st.converged, st.final_residual) == (res.iterations, res.converged, res.final_residual)
    assert np.array_equal(x, res.x)


def test_stepping_session(ctx, rs):
    a = O.stencil7(24, "aniso")
    d = to_dev(ctx, a)
    m = uniform_ref(a, 8)
    pc = K.BlockJacobi.uniform(8).setup(d)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    steps = 17
    res = O.solve("pcg", a, b, pc=O.Pc.approx_inverse(m), tol=1e-30, max_iters=steps, rs=rs, raise_on_error=False)
    xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    with K.Session("pcg", d, pc, K.DeviceVec(ctx, b), xv, tol=1e-30, max_iters=steps) as sess:
        sess.step(steps)
        st = sess.end()
        hist = sess.residual_history
    assert st.iterations == res.iterations == steps
    assert np.array_equal(np.array(hist), res.history)
    assert np.array_equal(xv.to_host(), res.x)


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_256_aniso_pcg_100(ctx, rs):
    N = 256
    a = O.stencil7(N, "aniso")
    d = K.CsrMatrix.stencil7(N, "aniso", ctx=ctx)
    m = uniform_ref(a, 8)
    pc = K.BlockJacobi.uniform(8).setup(d)
    b = a.spmv(np.ones(a.nrows))
    res = O.solve("pcg", a, b, pc=O.Pc.approx_inverse(m), tol=1e-30, max_iters=100, rs=rs, raise_on_error=False)
    s = K.PcgSolver(1e-30, 100)
    x = np.zeros(a.nrows)
    try:
        st = s.solve(d, pc, b, x)
    except K.KError as e:                  # not converged within 100 iterations: the same status as the oracle's
        st = e.stats
    assert st.iterations == res.iterations == 100
    assert np.array_equal(np.array(s.residual_history), res.history)
    assert np.array_equal(x, res.x)


def test_full_size_512_apply_sampled_blocks(ctx):
    N, bsize = 512, 8
    n = N ** 3
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    pc = K.BlockJacobi.uniform(bsize).setup(d)
    rv = ctx.vec(n).fill_splitmix(0x5EED)
    zv = pc.apply(rv)
    r, z = rv.to_host(), zv.to_host()
    ks = np.sort(np.random.default_rng(512).choice(n // bsize, 4096, replace=False))
    rows = (ks[:, None] * bsize + np.arange(bsize)[None, :]).ravel()
    rp, ci, va = R.stencil7_rows(N, "poisson", rows)
    # the rows' CSR with the columns of other rows: the block matrix takes the entries inside the block only
    B = np.zeros((len(ks), bsize, bsize))
    r_of = np.repeat(np.arange(len(rows)), np.diff(rp))
    inblk = (ci // bsize) == (rows[r_of] // bsize)
    B[r_of[inblk] // bsize, r_of[inblk] % bsize, ci[inblk] % bsize] = va[inblk]
    Bi, zp = R.gauss_jordan(B)
    assert np.all(zp == -1)
    want = R.apply_pinned(Bi, r[rows].reshape(len(ks), bsize))
    assert np.array_equal(z[rows].reshape(len(ks), bsize), want)


# ------------------------------------------------------------------------------------------------ errors
def _code(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_errors(ctx):
    a = O.stencil7(6, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    assert _code(lambda: K.BlockJacobi([[0, 1], [n]]).setup(d)).code == 102            # index out of range
    assert _code(lambda: K.BlockJacobi([[-1]]).setup(d)).code == 102
    assert _code(lambda: K.BlockJacobi([[3, 5, 3]]).setup(d)).code == 102             # repeated within a block
    e = _code(lambda: K.BlockJacobi([list(range(65))]).setup(d))                        # more than 64 rows
    assert e.code == 6 and "64" in str(e)
    assert _code(lambda: K.BlockJacobi.uniform(65).setup(d)).code == 6
    assert _code(lambda: K.BlockJacobi.uniform(0).setup(d)).code == 102
    # singular block: rows 10..13 of an operator whose rows 11 and 12 are equal inside the block
    dense = np.diag(np.full(20, 4.0))
    dense[11, 10:14] = [1.0, 2.0, 3.0, 4.0]
    dense[12, 10:14] = [1.0, 2.0, 3.0, 4.0]
    s = O.Csr.from_dense(dense, keep_zeros=False)
    ds = to_dev(ctx, s)
    blocks = [[0, 1], [13, 12, 11, 10]]
    e = _code(lambda: K.BlockJacobi(blocks).setup(ds))
    gs, inv, zp = R.tiles_of(s.row_ptr, s.col_idx, s.vals, blocks)
    assert e.code == 5 and zp[0] == -1 and zp[1] >= 0 and e.row == gs[1][zp[1]]
    dense = np.diag(np.full(20, 4.0))
    dense[10, 10:12] = [1.0, 2.0]
    dense[11, 10:12] = [1.0, 2.0]                      # block 5 of the contiguous form with 2 rows per block
    s = O.Csr.from_dense(dense, keep_zeros=False)
    e = _code(lambda: K.BlockJacobi.uniform(2).setup(to_dev(ctx, s)))
    gs, inv, zp = R.tiles_uniform(s.row_ptr, s.col_idx, s.vals, 20, 2)
    k = next(k for k, p in enumerate(zp) if p >= 0)
    assert e.code == 5 and k == 5 and e.row == gs[k][zp[k]]
    # an all-zero block: the first position
    z = O.Csr.from_dense(np.diag([1.0, 0.0, 0.0, 1.0]), keep_zeros=False)
    e = _code(lambda: K.BlockJacobi([[3], [2, 1]]).setup(to_dev(ctx, z)))
    assert e.code == 5 and e.row == 1
    # NaN inside a block
    bad = a.vals.copy(); bad[a.row_ptr[7]] = np.nan
    dn = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, bad, ctx=ctx)
    assert _code(lambda: K.BlockJacobi.uniform(8).setup(dn)).code == 1
    assert _code(lambda: K.BlockJacobi([[7, 1]]).setup(dn)).code == 1
    # non-square operator
    rect = K.CsrMatrix.from_csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0], ctx=ctx)
    assert _code(lambda: K.BlockJacobi.uniform(1).setup(rect)).code == 102
    assert _code(lambda: K.BlockJacobi([[0]]).setup(rect)).code == 102
    # a one-rank distributed operator
    dd = K.CsrMatrix.from_csr_dist(ctx, n, [0, n], a.row_ptr, a.col_idx, a.vals)
    assert _code(lambda: K.BlockJacobi.uniform(4).setup(dd)).code == 6
    # empty blocks do nothing; every row uncovered gives z = 0
    pc = K.BlockJacobi([[], []]).setup(d)
    zz = pc.apply(np.ones(n))
    assert np.all(zz == 0.0)
