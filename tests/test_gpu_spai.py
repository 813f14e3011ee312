"""The SPAI set-up on the device (ApproxInv::setup, src/preconditioner/approxinv.rs:123-264; kryst_amd/csrc/spai.hip) against the numpy
restatement (tests/spai_ref.py) and, through the exported M, against the oracle: with M = the device's inverse rows, the preconditioner IS
the oracle's ApproxInv(M) (z = kro_spmv(M, r)), so applies and whole solves are compared bit for bit.  The set-up values themselves come
from a different least-squares solver (Householder QR against LAPACK's), so they are compared to a tolerance, and the tolerances tol of
the drop are chosen so that no value lies near them: the drop sets are then identical."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import bjacobi_ref as BR
import spai_ref as R
from sa_cases import op27

pytestmark = pytest.mark.gpu

OP = K.SparsityPattern.Operator


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
    rp, ci, va = pc.export()
    return O.Csr(len(rp) - 1, len(rp) - 1, rp, ci.astype(np.int64), va)


def check_values(pc, a, pptr, pidx, tol):
    """The exported M has the restatement's pattern exactly and its values within 1e-11 of each column's max |m_j|."""
    (rp, ci, va), cols = R.setup(a, pptr, pidx, tol)
    allv = np.concatenate([m for _, m in cols.values()] + [np.zeros(0)])
    near = np.abs(np.abs(allv) - tol) <= 1e-6 * tol
    assert not near.any(), "tol lies too close to a reference value: choose another"
    m = exported(pc)
    assert np.array_equal(m.row_ptr, rp) and np.array_equal(m.col_idx, ci)
    scale = np.zeros(a.nrows)
    for j, (_, mj) in cols.items():
        scale[j] = np.max(np.abs(mj)) if len(mj) else 0.0
    assert np.all(np.abs(m.vals - va) <= 1e-11 * scale[ci])
    return m


def random_sparse(n, seed, density=0.02):
    rng = np.random.default_rng(seed)
    dense = np.where(rng.random((n, n)) < density, rng.standard_normal((n, n)), 0.0)
    dense[np.arange(n), np.arange(n)] += 4.0
    return O.Csr.from_dense(dense, keep_zeros=False)


def random_pattern(n, seed, empty=0.1, own=0.6, maxlen=6):
    """Unsorted columns of 0..maxlen random rows: some empty, j itself only in some of them."""
    rng = np.random.default_rng(seed)
    pat = []
    for j in range(n):
        if rng.random() < empty:
            pat.append([]); continue
        c = set(rng.choice(n, size=int(rng.integers(1, maxlen + 1)), replace=False).tolist())
        if rng.random() < own:
            c.add(j)
        else:
            c.discard(j)
        c = list(c); rng.shuffle(c)
        pat.append(c)
    return pat


# ------------------------------------------------------------------------------------------------ 1. set-up values
@pytest.mark.parametrize("kind,N", [("poisson", 8), ("aniso", 12), ("convdiff", 16), ("varcoef", 10), ("poisson", 32), ("convdiff", 32)])
def test_values_operator_pattern(ctx, kind, N):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    ctx.poison_lds()
    pc = K.Spai(OP, 1e-9).setup(d)
    m = check_values(pc, a, a.row_ptr, a.col_idx, 1e-9)
    assert m.nnz == a.nnz


@pytest.mark.parametrize("N,seed", [(6, 1), (9, 2)])
def test_values_27_point(ctx, N, seed):
    a = op27(N, seed)
    d = to_dev(ctx, a)
    ctx.poison_lds()
    pc = K.Spai(OP, 1e-10).setup(d)
    check_values(pc, a, a.row_ptr, a.col_idx, 1e-10)


@pytest.mark.parametrize("n,seed", [(300, 3), (1000, 4)])
def test_values_random_nonsymmetric(ctx, n, seed):
    a = random_sparse(n, seed, density=6.0 / n)
    d = to_dev(ctx, a)
    pc = K.Spai(OP, 1e-10).setup(d)
    check_values(pc, a, a.row_ptr, a.col_idx, 1e-10)
    pat = random_pattern(n, seed)
    ptr, idx = R.manual_ptr_idx(pat)
    ctx.poison_lds()
    pcm = K.Spai(K.SparsityPattern.Manual(pat), 1e-10).setup(d)
    check_values(pcm, a, ptr, idx, 1e-10)


@pytest.mark.parametrize("kind,N,seed", [("poisson", 10, 5), ("convdiff", 12, 6)])
def test_values_manual_stencil(ctx, kind, N, seed):
    # empty columns, columns without j, and columns two grid steps wide (|J| up to 13)
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    n = a.nrows
    rng = np.random.default_rng(seed)
    pat = []
    for j in range(n):
        u = rng.random()
        if u < 0.1:
            pat.append([])
        elif u < 0.2:
            pat.append([(j + 1) % n])
        else:
            row = a.col_idx[a.row_ptr[j]:a.row_ptr[j + 1]]
            far = [c for c in (j - 2, j + 2, j - 2 * N, j + 2 * N, j - 2 * N * N, j + 2 * N * N) if 0 <= c < n]
            pat.append(list(rng.permutation(np.concatenate([row, far]))))
    ptr, idx = R.manual_ptr_idx(pat)
    pc = K.Spai(K.SparsityPattern.Manual(pat), 1e-9).setup(d)
    check_values(pc, a, ptr, idx, 1e-9)


@pytest.mark.parametrize("wide", [40, 64])
def test_values_wide_columns(ctx, wide):
    # a column of 33..64 pattern entries: one column per workgroup, and at 64 a workgroup of two waves (barriers across waves); the other
    # columns take the operator's pattern.  Tridiagonal nonsymmetric operator: the wide column's I has wide + 2 rows.
    n = 200
    dense = np.diag(np.full(n, 4.0)) + np.diag(np.full(n - 1, -1.0), 1) + np.diag(np.full(n - 1, -0.5), -1)
    a = O.Csr.from_dense(dense, keep_zeros=False)
    d = to_dev(ctx, a)
    pat = [a.col_idx[a.row_ptr[j]:a.row_ptr[j + 1]].tolist() for j in range(n)]
    pat[100] = list(range(100 - wide // 2, 100 - wide // 2 + wide))[::-1]
    pat[7] = list(range(0, 40))
    ptr, idx = R.manual_ptr_idx(pat)
    ctx.poison_lds()
    pc = K.Spai(K.SparsityPattern.Manual(pat), 1e-10).setup(d)
    check_values(pc, a, ptr, idx, 1e-10)


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("kind", ["poisson", "convdiff"])
def test_determinism_64(ctx, kind):
    d = K.CsrMatrix.stencil7(64, kind, ctx=ctx)
    m1 = K.Spai(OP, 1e-12).setup(d).export()
    ctx.poison_lds()
    m2 = K.Spai(OP, 1e-12).setup(d).export()
    for x, y in zip(m1, m2):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ------------------------------------------------------------------------------------------------ 3. apply and solves, bit for bit
@pytest.mark.parametrize("kind,N", [("poisson", 16), ("aniso", 24), ("convdiff", 20), ("varcoef", 32)])
def test_apply_bit_exact(ctx, kind, N):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    pc = K.Spai(OP, 1e-12).setup(d)
    m = exported(pc)
    r = np.random.default_rng(N).standard_normal(a.nrows)
    ctx.poison_lds()
    assert np.array_equal(pc.apply(r), O.Pc.approx_inverse(m).apply(r))
    # the given-rows ApproxInv over the same M applies the same bits
    inv_rows = [list(zip(m.col_idx[m.row_ptr[i]:m.row_ptr[i + 1]].tolist(), m.vals[m.row_ptr[i]:m.row_ptr[i + 1]].tolist())) for i in range(a.nrows)]
    assert np.array_equal(K.ApproxInv(inv_rows, ctx=ctx).apply(r), pc.apply(r))


def _check(res, st, hist, x):
    assert (st.iterations, st.converged) == (res.iterations, res.converged)
    assert st.final_residual == res.final_residual
    assert np.array_equal(np.array(hist), res.history)
    assert np.array_equal(x, res.x)


def _solve_both(rs, method, a, d, kpc, m, b, tol, max_iters):
    opc = O.Pc.approx_inverse(m)
    x = np.zeros(a.nrows)
    if method == "pcg":
        res = O.solve("pcg", a, b, pc=opc, tol=tol, max_iters=max_iters, rs=rs)
        s = K.PcgSolver(tol, max_iters); st = s.solve(d, kpc, b, x)
    elif method == "gmres_right":
        res = O.solve("gmres", a, b, pc=opc, tol=tol, max_iters=max_iters, restart=20, side=O.SIDE_RIGHT, rs=rs)
        s = K.GmresSolver(20, tol, max_iters).with_preconditioning(K.Preconditioning.Right)
        st = s.solve(d, kpc, b, x)
    else:
        atol = tol * float(np.linalg.norm(b))                                  # BiCGStab's tolerance is absolute (bicgstab.rs)
        res = O.solve("bicgstab_rpc", a, b, pc=opc, tol=atol, max_iters=max_iters, rs=rs)
        s = K.BiCgStabRightPcSolver(atol, max_iters); st = s.solve(d, kpc, b, x)
    _check(res, st, s.residual_history, x)
    return res


@pytest.mark.parametrize("method,kind,N", [(m, k, N) for m in ("pcg", "bicgstab_rpc", "gmres_right")
                                            for k, N in (("poisson", 16), ("aniso", 24), ("convdiff", 20))
                                            if not (m == "pcg" and k == "convdiff")])            # (PCG needs a symmetric operator)
def test_solves_bit_exact(ctx, rs, method, kind, N):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    pc = K.Spai(OP, 1e-12).setup(d)
    m = exported(pc)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    res = _solve_both(rs, method, a, d, pc, m, b, 1e-8, 400)
    assert res.iterations > 1


def test_solve_manual_pattern_random(ctx, rs):
    a = random_sparse(400, 9, density=6.0 / 400)
    d = to_dev(ctx, a)
    pat = [sorted(set(a.col_idx[a.row_ptr[j]:a.row_ptr[j + 1]].tolist()) | {(j + 7) % 400}) for j in range(400)]
    pc = K.Spai(K.SparsityPattern.Manual(pat), 1e-12).setup(d)
    m = exported(pc)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    _solve_both(rs, "gmres_right", a, d, pc, m, b, 1e-10, 300)
    _solve_both(rs, "bicgstab_rpc", a, d, pc, m, b, 1e-10, 300)


@pytest.mark.parametrize("kind", [K.SolverKind.Bicgstab, K.SolverKind.GmresRight])
def test_ksp_context(ctx, rs, kind):
    a = O.stencil7(20, "convdiff")
    d = to_dev(ctx, a)
    pc = K.PC.ApproxInv(OP, 1e-12, 10).build(d)
    m = exported(pc)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    ksp = K.KspContext(kind, d, pc=pc, tol=1e-8, max_it=300, restart=20)
    x = np.zeros(a.nrows)
    st = ksp.solve_context(b, x)
    if kind == K.SolverKind.Bicgstab:
        res = O.solve("bicgstab", a, b, pc=O.Pc.approx_inverse(m), tol=1e-8, max_iters=300, rs=rs)
    else:
        res = O.solve("gmres", a, b, pc=O.Pc.approx_inverse(m), tol=1e-8, max_iters=300, restart=20, side=O.SIDE_RIGHT, rs=rs)
    assert (st.iterations, st.converged, st.final_residual) == (res.iterations, res.converged, res.final_residual)
    assert np.array_equal(x, res.x)


def test_stepping_session(ctx, rs):
    a = O.stencil7(24, "aniso")
    d = to_dev(ctx, a)
    pc = K.Spai(OP, 1e-12).setup(d)
    m = exported(pc)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    steps = 13
    res = O.solve("pcg", a, b, pc=O.Pc.approx_inverse(m), tol=1e-30, max_iters=steps, rs=rs, raise_on_error=False)
    xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    with K.Session("pcg", d, pc, K.DeviceVec(ctx, b), xv, tol=1e-30, max_iters=steps) as sess:
        sess.step(steps)
        st = sess.end()
        hist = sess.residual_history
    assert st.iterations == res.iterations == steps
    assert np.array_equal(np.array(hist), res.history)
    assert np.array_equal(xv.to_host(), res.x)


# ------------------------------------------------------------------------------------------------ 4. reference semantics and errors
def _code(fn):
    with pytest.raises(K.KError) as e:
        fn()
    return e.value


def test_errors(ctx):
    a = O.stencil7(6, "poisson")
    d = to_dev(ctx, a)
    n = a.nrows
    ok = [[j] for j in range(n)]
    assert _code(lambda: K.Spai(K.SparsityPattern.Auto, 1e-12).setup(d)).code == 6             # approxinv.rs:127-133
    assert _code(lambda: K.PC.ApproxInv(K.SparsityPattern.Auto, 1e-12, 10).build(d)).code == 6
    assert _code(lambda: K.Spai(ok[:-1], 1e-12).setup(d)).code == 102                            # pat.len() != n
    assert _code(lambda: K.Spai(ok + [[0]], 1e-12).setup(d)).code == 102
    assert _code(lambda: K.Spai(ok[:-1] + [[n]], 1e-12).setup(d)).code == 102                    # out of range
    assert _code(lambda: K.Spai([[-1]] + ok[1:], 1e-12).setup(d)).code == 102
    assert _code(lambda: K.Spai([[3, 5, 3]] + ok[1:], 1e-12).setup(d)).code == 102              # repeated within a column
    e = _code(lambda: K.Spai([list(range(65))] + ok[1:], 1e-12).setup(d))                       # more than 64 pattern entries
    assert e.code == 6 and "64" in str(e)
    # a structurally singular column: column 2 of the operator stores nothing, so A[:, {0, 2}] has a zero column
    s = O.Csr.from_dense(np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0], [0, 0, 0, 1.0]]), keep_zeros=False)
    e = _code(lambda: K.Spai([[0], [1], [0, 2], [3]], 1e-12).setup(to_dev(ctx, s)))
    assert e.code == 1 and "column 2" in str(e)
    # two columns with their only entries in one row: rank 1 (the second Householder column is empty)
    s = O.Csr.from_dense(np.array([[1.0, 2.0, 0], [0, 0, 0], [0, 0, 1.0]]), keep_zeros=False)
    e = _code(lambda: K.Spai([[0], [0, 1], [2]], 1e-12).setup(to_dev(ctx, s)))
    assert e.code == 1 and "column 1" in str(e)
    # the operator's pattern of a singular operator: row 1 stores columns {0, 1}, both columns have their entries in row 0 only
    assert _code(lambda: K.Spai(OP, 1e-12).setup(to_dev(ctx, O.Csr(3, 3, [0, 2, 4, 5], [0, 1, 0, 1, 2], [1.0, 2.0, 0.0, 0.0, 1.0])))).code == 1
    # NaN in A[I, J]
    bad = a.vals.copy(); bad[a.row_ptr[7]] = np.nan
    dn = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, bad, ctx=ctx)
    assert _code(lambda: K.Spai(OP, 1e-12).setup(dn)).code == 1
    # non-square; a one-rank distributed operator
    rect = K.CsrMatrix.from_csr(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0], ctx=ctx)
    assert _code(lambda: K.Spai(OP, 1e-12).setup(rect)).code == 102
    dd = K.CsrMatrix.from_csr_dist(ctx, n, [0, n], a.row_ptr, a.col_idx, a.vals)
    assert _code(lambda: K.Spai(OP, 1e-12).setup(dd)).code == 6


def test_caps(ctx):
    # the operator's pattern with a row of 65 entries: refused on the device before any column is solved
    n = 100
    dense = np.eye(n) * 4.0
    dense[10, :65] = 1.0
    dense[10, 10] = 4.0
    d = to_dev(ctx, O.Csr.from_dense(dense, keep_zeros=False))
    e = _code(lambda: K.Spai(OP, 1e-12).setup(d))
    assert e.code == 6 and "column 10" in str(e)
    # |I_j| > 128 with fewer than 64 pattern entries: refused by the column kernel
    a = random_sparse(600, 11, density=12.0 / 600)
    da = to_dev(ctx, a)
    cp, cr, cv = R.csc(a.row_ptr, a.col_idx, a.vals, 600)
    pat = [[j] for j in range(600)]
    pat[5] = list(range(0, 600, 25))                              # 24 columns of ~13 rows each: |I| > 128
    assert len(np.unique(np.concatenate([cr[cp[k]:cp[k + 1]] for k in pat[5]]))) > 128
    e = _code(lambda: K.Spai(pat, 1e-12).setup(da))
    assert e.code == 6 and "column 5" in str(e)
    # empty patterns: M = 0
    pc = K.Spai([[] for _ in range(600)], 1e-12).setup(da)
    rp, ci, va = pc.export()
    assert rp[-1] == 0 and np.all(pc.apply(np.ones(600)) == 0.0)


# ------------------------------------------------------------------------------------------------ 5. full size
def test_full_size_256_poisson_sampled_columns(ctx):
    N = 256
    n = N ** 3
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    pc = K.Spai(OP, 1e-12).setup(d)
    rp, ci, va = pc.export()
    assert rp[-1] == 7 * n - 6 * N * N                       # nnz(M) == nnz(A): every entry of the 7-point pattern is kept
    js = np.sort(np.random.default_rng(256).choice(n, 4096, replace=False))
    js = np.union1d(js, [0, n - 1, N * N * (N // 2) + N // 2])

    def col(k):                                              # the operator is symmetric: column k = row k
        r, c, v = BR.stencil7_rows(N, "poisson", [k])
        return c, v
    for j in js:
        J, I, Ah, e = R.reduced_problem(int(j), col(int(j))[0], col)
        m = R.solve_column(Ah, e)
        got = np.empty(len(J))
        for q, i in enumerate(J):                            # M[i, j] from row i of the exported CSR
            lo, hi = rp[i], rp[i + 1]
            p = lo + np.searchsorted(ci[lo:hi], j)
            assert p < hi and ci[p] == j
            got[q] = va[p]
        assert np.all(np.abs(got - m) <= 1e-11 * np.max(np.abs(m)))
