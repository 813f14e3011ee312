"""Block CG on the GPU (kryst_bcg_solve_multi_dev, kryst_bench_mvec_gram, BlockCgSolver) against the numpy restatement of its operation order
(tests/block_cg_ref.py), bit for bit: x, the iteration count, every residual-history entry, final_residual, converged and the status.  Every
comparison is made on uint64 views.  Fixtures and references: tests/block_cg_cases.py (checked without a GPU in test_block_cg_cpu.py)."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import block_cg_cases as BC
import block_cg_ref as R
import multi_rhs_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, UNSUPPORTED = 102, 6
bits = BC.bits


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec() == R.SPEC
    return K.Context(0)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def upload(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def device_operator(ctx, name):
    N, kind = BC.kind_of(name)
    return K.CsrMatrix.stencil7(N, kind, ctx=ctx)                    # carries its compressed forms (CSR-P16 / CSR-DIA)


def make_pc(d, pc):
    return {None: lambda: None, "identity": lambda: K.IdentityPc().setup(d), "jacobi": lambda: K.Jacobi().setup(d)}[pc]()


# ---------------------------------------------------------------------------------------------------------------- 1. the Gram pass
@pytest.mark.parametrize("n", BC.GRAM_SIZES)
def test_gram_against_the_restatement(ctx, n):
    for k in BC.WIDTHS:
        u, v, d = BC.gram_inputs(n, k)
        um, vm, dv = K.MultiVec.from_numpy(u, ctx=ctx), K.MultiVec.from_numpy(v, ctx=ctx), ctx.vec(d)
        want = {False: R.gram(u, v), True: R.gram(u, v, d)}
        want_uu = R.gram(u, u, d)
        for value in ("clean", None, 1e300):                         # NaN and 1e300 in the padding of both multivectors
            if value != "clean":
                um.poison_padding(value); vm.poison_padding(value)
            assert same(K.mvec_gram(um, vm), want[False]), (n, k, value)
            assert same(K.mvec_gram(um, vm, dv), want[True]), (n, k, value, "weighted")
            assert same(K.mvec_gram(um, um, dv), want_uu), (n, k, value, "U against U")


@pytest.mark.parametrize("kind", ("nan", "inf", "negzero", "denormal"))
def test_a_special_column_poisons_its_own_row_and_column_only(ctx, kind):
    n = 1025
    for k in BC.WIDTHS:
        u, v, d = BC.gram_inputs(n, k)
        j = k - 1 if kind in ("nan", "negzero") else 1
        us, vs = u.copy(), v.copy()
        us[:, j] = BC.special_column(kind, n); vs[:, j] = BC.special_column(kind, n)
        plain = K.mvec_gram(K.MultiVec.from_numpy(u, ctx=ctx), K.MultiVec.from_numpy(v, ctx=ctx), ctx.vec(d))
        got = K.mvec_gram(K.MultiVec.from_numpy(us, ctx=ctx), K.MultiVec.from_numpy(vs, ctx=ctx), ctx.vec(d))
        assert same(got, R.gram(us, vs, d)), (kind, k)
        touched = np.zeros((k, k), dtype=bool); touched[j, :] = True; touched[:, j] = True
        assert np.array_equal(bits(got)[~touched], bits(plain)[~touched]), (kind, k)
        # (the upper triangle holds U(:, a) . V(:, b) for a <= b and the lower mirrors it: row and column j are exactly the entries that see column j)
        if kind in ("nan", "inf"):
            assert not np.isfinite(got[touched]).all() and np.isfinite(got[~touched]).all()
        if kind == "nan":
            assert np.isnan(got[touched]).all()


# ---------------------------------------------------------------------------------------------------------------- 2. block solves
Col = collections.namedtuple("Col", "status iterations final_residual converged hist_len history x")


def block_solve(ctx, d, pc, b, x0, tol=BC.TOL, cap=BC.CAP, hist_cap=None, alias=False, edit=None, expect_rc=0, poison=None):
    """kryst_bcg_solve_multi_dev, raw"""
    k = b.shape[1]
    bm = K.MultiVec.from_numpy(b, ctx=ctx)
    xm = bm if alias else K.MultiVec.from_numpy(x0, ctx=ctx)
    if poison is not None:
        bm.poison_padding(poison[0]); xm.poison_padding(poison[0])
    prm = _ffi.Params(tol, cap, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    if edit:
        edit(prm)
    hist_cap = cap + 8 if hist_cap is None else hist_cap
    st, code, hlen = (_ffi.Stats * k)(), (C.c_int32 * k)(*([-99] * k)), (C.c_int64 * k)(*([-99] * k))
    hist = np.full((k, max(hist_cap, 1)), -99.0)
    rc = K.lib().kryst_bcg_solve_multi_dev(bm.h, xm.h, d.h, pc.h if pc is not None else None, C.byref(prm), st, code,
                                           hist.ctypes.data_as(_ffi.c_dp), hist_cap, hlen)
    assert rc == expect_rc, (rc, K.lib().kryst_hip_last_error())
    xs = xm.to_numpy()
    if rc != 0:
        return list(code), list(hlen), hist, xs
    assert (hist[:, hist_cap:] == -99.0).all()
    return [Col(code[j], st[j].iterations, st[j].final_residual, bool(st[j].converged), hlen[j], hist[j, :min(hlen[j], hist_cap)].copy(), xs[:, j].copy())
            for j in range(k)]


def from_reference(ref):
    k = len(ref.history)
    return [Col(ref.status, ref.iterations, ref.final_residual[j], bool(ref.converged[j]), len(ref.history[j]), np.array(ref.history[j]), ref.x[:, j])
            for j in range(k)]


def assert_columns(got, want, label, hist_cap=None):
    assert len(got) == len(want), label
    for j, (g, w) in enumerate(zip(got, want)):
        lab = (label, j)
        assert (g.status, g.iterations, g.converged, g.hist_len) == (w.status, w.iterations, w.converged, w.hist_len), (lab, g[:5], w[:5])
        assert same([g.final_residual], [w.final_residual]), (lab, g.final_residual, w.final_residual)
        wh = w.history if hist_cap is None else w.history[:hist_cap]
        assert same(g.history, wh), (lab, "history", g.history[:4], wh[:4])
        assert same(g.x, w.x), (lab, "x", int(np.sum(bits(g.x) != bits(w.x))))


@pytest.mark.parametrize("name", BC.NAMES)
@pytest.mark.parametrize("pc", BC.PCS)
def test_block_solves_against_the_restatement(ctx, name, pc):
    d = device_operator(ctx, name)
    dpc = make_pc(d, pc)
    for k in BC.WIDTHS:
        b = BC.rhs(name)[:, :k]
        want = from_reference(BC.reference(name, k, pc))
        assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b)), want, f"{name} k={k} pc={pc}")


@pytest.mark.parametrize("pc", (None, "jacobi"))
def test_plain_and_dia_spmm_give_the_same_bits(ctx, pc, monkeypatch):
    name = "varcoef12"
    d = device_operator(ctx, name)
    dpc = make_pc(d, pc)
    for k in BC.WIDTHS:
        b = BC.rhs(name)[:, :k]
        want = from_reference(BC.reference(name, k, pc))
        kernels = set()
        for form in ("plain", "dia"):
            monkeypatch.setenv("KRYST_SPMM_FORM", form)
            kernel = C.c_int32(-1)
            K.check(K.lib().kryst_spmm_kernel(d.h, k, C.byref(kernel)))
            kernels.add(kernel.value)
            assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b)), want, f"{name} k={k} pc={pc} KRYST_SPMM_FORM={form}")
        assert kernels == {0, 1}                                     # both kernels ran


@pytest.mark.parametrize("pc", (None, "jacobi"))
def test_solve_variants(ctx, pc):
    name, k = "poisson9", 4
    d = device_operator(ctx, name)
    dpc = make_pc(d, pc)
    b, g = BC.rhs(name)[:, :k], BC.guesses(name)[:, :k]
    # x0 != 0, with NaN and 1e300 in the padding of B and X
    want = from_reference(BC.reference(name, k, pc, guess=True))
    assert_columns(block_solve(ctx, d, dpc, b, g), want, "x0 != 0")
    for value in (None, 1e300):
        assert_columns(block_solve(ctx, d, dpc, b, g, poison=(value,)), want, f"x0 != 0, padding {value}")
    # B and X the same multivector: x0 = b, and it holds x afterwards
    assert_columns(block_solve(ctx, d, dpc, b, None, alias=True), from_reference(BC.reference(name, k, pc, alias=True)), "B is X")
    # caps: 0, 1, 2 and one hit mid-run (converged = true as Convergence::check reports it)
    for cap in (0, 1, 2, 5):
        ref = BC.reference(name, k, pc, max_iters=cap)
        assert ref.iterations == cap and ref.converged == [cap > 0] * k
        assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b), cap=cap), from_reference(ref), f"max_iters={cap}")
    # history buffers shorter than the history: hist_len still counts every push, the slices do not run into each other
    full = from_reference(BC.reference(name, k, pc))
    assert full[0].hist_len > 3
    assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b), hist_cap=3), full, "hist_cap=3", hist_cap=3)
    assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b), hist_cap=0), full, "hist_cap=0", hist_cap=0)
    # NULL outputs are allowed
    bm, xm = K.MultiVec.from_numpy(b, ctx=ctx), K.MultiVec(ctx, b.shape[0], k)
    prm = _ffi.Params(BC.TOL, BC.CAP, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    assert K.lib().kryst_bcg_solve_multi_dev(bm.h, xm.h, d.h, dpc.h if dpc is not None else None, C.byref(prm), None, None, None, 0, None) == 0
    assert same(xm.to_numpy(), np.stack([c.x for c in full], axis=1))


@pytest.mark.parametrize("name", list(BC.breakdown_cases()))
def test_each_way_of_ending(ctx, name):
    a, b, jac, status, it = BC.breakdown_cases()[name]
    g, ref = BC.breakdown_reference(name)
    assert (ref.status, ref.iterations) == (status, it)
    d = upload(ctx, a)
    dpc = K.Jacobi().setup(d) if jac else None
    got = block_solve(ctx, d, dpc, b, g)
    assert_columns(got, from_reference(ref), name)
    assert all(same(c.x, g[:, j]) for j, c in enumerate(got))       # X is bitwise untouched


@pytest.fixture(scope="module")
def big():
    """81^3 = 531 441 rows > 524 288: the folds run their second stage.  The reference is computed once."""
    N, cap, k = 81, 3, 8
    a = O.stencil7(N)
    b = np.random.default_rng(81).random((a.nrows, k))
    d = O.Pc.jacobi(a).inv_diag.copy()
    return N, cap, b, {None: R.solve(a, b, tol=BC.TOL, max_iters=cap), "jacobi": R.solve(a, b, d=d, tol=BC.TOL, max_iters=cap)}


@pytest.mark.parametrize("fuse", ("0", "1"))
def test_gram_in_the_spmm_epilogue_gives_the_same_bits(ctx, fuse, monkeypatch):
    """KRYST_BCG_FUSE_GRAM: Gram(S, T) by mgram_kernel behind a plain SpMM (0) or in the epilogue of spmm_rows_kernel / spmm_dia_kernel (1)"""
    monkeypatch.setenv("KRYST_BCG_FUSE_GRAM", fuse)
    for name, form in (("poisson9", "plain"), ("poisson12", "plain"), ("varcoef12", "plain"), ("varcoef12", "dia")):
        monkeypatch.setenv("KRYST_SPMM_FORM", form)
        d = device_operator(ctx, name)
        for pc in (None, "jacobi"):
            dpc = make_pc(d, pc)
            for k in BC.WIDTHS:
                b = BC.rhs(name)[:, :k]
                assert_columns(block_solve(ctx, d, dpc, b, np.zeros_like(b)), from_reference(BC.reference(name, k, pc)), f"{name} {form} k={k} pc={pc} fuse={fuse}")


@pytest.mark.parametrize("handoff", ("poll", "ticket"))
def test_past_one_fold_chunk(ctx, big, handoff, monkeypatch):
    N, cap, b, refs = big
    monkeypatch.delenv("KRYST_FOLD_POLL", raising=False)
    if handoff == "ticket":
        monkeypatch.setenv("KRYST_FOLD_POLL", "0")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    for pc in (None, "jacobi"):
        ref = refs[pc]
        assert ref.status == 0 and ref.iterations == cap and all(ref.converged)
        for fuse in ("0", "1"):
            monkeypatch.setenv("KRYST_BCG_FUSE_GRAM", fuse)
            assert_columns(block_solve(ctx, d, make_pc(d, pc), b, np.zeros_like(b), cap=cap), from_reference(ref), f"81^3 pc={pc} {handoff} fuse={fuse}")


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_outputs_untouched(ctx):
    name, k = "poisson8", 4
    a, b = BC.operator(name), BC.rhs(name)[:, :k]
    d = device_operator(ctx, name)
    x0 = BC.guesses(name)[:, :k]
    jac, ilu = K.Jacobi().setup(d), K.Ilu0().setup(d)

    def refused(pc, code, op=None, **kw):
        status, hlen, hist, xs = block_solve(ctx, d if op is None else op, pc, b, x0, expect_rc=code, **kw)
        assert status == [-99] * k and hlen == [-99] * k and (hist == -99.0).all() and same(xs, x0), (code, kw)

    refused(ilu, UNSUPPORTED)                                                   # a preconditioner other than Identity / Jacobi
    dd = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)      # a row-partitioned operator on this one rank
    refused(None, UNSUPPORTED, op=dd)
    refused(jac, UNSUPPORTED, op=dd)
    for pc in (None, jac):
        refused(pc, UNSUPPORTED, edit=lambda p: setattr(p, "norm_type", 2))
        refused(pc, UNSUPPORTED, edit=lambda p: setattr(p, "norm_type", 3))
        refused(pc, UNSUPPORTED, edit=lambda p: (setattr(p, "has_radius", 1), setattr(p, "radius", 1.0)))
        refused(pc, UNSUPPORTED, edit=lambda p: (setattr(p, "has_obj_target", 1), setattr(p, "obj_target", -1.0)))
        refused(pc, ERR_ARG, cap=-1)
    lib = K.lib()
    prm = _ffi.Params(BC.TOL, 10, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    bm = K.MultiVec.from_numpy(b, ctx=ctx)
    for xm in (K.MultiVec(ctx, a.nrows, 2), K.MultiVec(ctx, a.nrows + 1, 4)):   # shapes that do not match
        assert lib.kryst_bcg_solve_multi_dev(bm.h, xm.h, d.h, None, C.byref(prm), None, None, None, 0, None) == ERR_ARG
    # k = 3 exists nowhere: not as a multivector, not in the host twin
    st, code, hlen = (_ffi.Stats * 3)(), (C.c_int32 * 3)(), (C.c_int64 * 3)()
    bh, xh = MC.pack_colmajor(b[:, :3]), MC.pack_colmajor(x0[:, :3])
    keep = xh.copy()
    for kk in (3, 1, 16):
        assert lib.kryst_bcg_solve_multi(bh.ctypes.data_as(_ffi.c_dp), xh.ctypes.data_as(_ffi.c_dp), a.nrows, kk, a.nrows, d.h, None, C.byref(prm), st, code,
                                         None, 0, hlen) == ERR_ARG
    assert same(xh, keep)
    # the Gram hook: mismatched shapes
    with pytest.raises(K.KError) as e:
        K.mvec_gram(bm, K.MultiVec(ctx, a.nrows, 2))
    assert e.value.code == ERR_ARG
    # the class: no single-vector form, no solve_many; B a MultiVec and X an array is an argument error
    s = K.BlockCgSolver(1e-8, 10)
    for call in (lambda: s.solve(d, None, b[:, 0], x0[:, 0].copy()), lambda: s.solve_many(d, None, b, x0.copy())):
        with pytest.raises(K.KError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    with pytest.raises(K.KError) as e:
        s.solve_block(d, None, bm, x0.copy())
    assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 4. the Python class, the host twin
@pytest.mark.parametrize("pc", (None, "jacobi"))
def test_solve_block_with_any_number_of_columns(ctx, pc):
    name = "poisson12"
    a = BC.operator(name)
    d = device_operator(ctx, name)
    dpc = make_pc(d, pc)
    b15 = np.random.default_rng(15).random((a.nrows, 15))
    w = None if pc is None else BC.inv_diag(name)
    for m in (3, 7, 15):                                             # 3 -> 2 + 1, 7 -> 4 + 2 + 1, 15 -> 8 + 4 + 2 + 1
        b = b15[:, :m]
        s = K.BlockCgSolver(BC.TOL, BC.CAP)
        xs = np.zeros((a.nrows, m))
        res = s.solve_block(d, dpc, b, xs)
        assert len(res) == m == len(s.residual_histories)
        at = 0
        for width in K.split_widths(m):
            cols = list(range(at, at + width))
            if width == 1:                                           # the leftover column: CgSolver / PcgSolver, as solve() gives it
                one = (K.CgSolver if pc is None else K.PcgSolver)(BC.TOL, BC.CAP)
                xj = np.zeros(a.nrows)
                stj = one.solve(d, dpc, np.ascontiguousarray(b[:, at]), xj)
                assert (res[at].iterations, res[at].converged) == (stj.iterations, stj.converged)
                assert same([res[at].final_residual], [stj.final_residual]) and same(s.residual_histories[at], one.residual_history) and same(xs[:, at], xj)
            else:
                ref = R.solve(a, b[:, cols], d=w, tol=BC.TOL, max_iters=BC.CAP)
                got = [Col(0, res[j].iterations, res[j].final_residual, bool(res[j].converged), len(s.residual_histories[j]),
                           np.array(s.residual_histories[j]), xs[:, j].copy()) for j in cols]
                assert_columns(got, from_reference(ref), f"solve_block m={m} columns {cols}")
            at += width
    # a block that breaks down leaves its columns of X alone and reports the error per column; the other blocks are solved
    b = b15[:, :6].copy(); b[:, 5] = b[:, 4]
    xs = np.full((a.nrows, 6), 0.5)
    s = K.BlockCgSolver(BC.TOL, BC.CAP)
    res = s.solve_block(d, dpc, b, xs)
    assert all(not isinstance(r, K.KError) for r in res[:4]) and all(isinstance(r, K.KError) and r.code == R.SOLVE_ERROR for r in res[4:])
    assert (xs[:, 4:] == 0.5).all() and not (xs[:, :4] == 0.5).all()


def test_the_host_twin_with_ld_greater_than_n(ctx):
    name, k, pc = "varcoef12", 4, "jacobi"
    a, b, g = BC.operator(name), BC.rhs(name)[:, :k], BC.guesses(name)[:, :k]
    d = device_operator(ctx, name)
    dpc = make_pc(d, pc)
    n, ld = a.nrows, a.nrows + 11
    bh, xh = MC.pack_colmajor(b, ld), MC.pack_colmajor(g, ld)
    prm = _ffi.Params(BC.TOL, BC.CAP, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    st, code, hlen = (_ffi.Stats * k)(), (C.c_int32 * k)(), (C.c_int64 * k)()
    hist = np.zeros((k, BC.CAP + 8))
    K.check(K.lib().kryst_bcg_solve_multi(bh.ctypes.data_as(_ffi.c_dp), xh.ctypes.data_as(_ffi.c_dp), n, k, ld, d.h, dpc.h, C.byref(prm), st, code,
                                          hist.ctypes.data_as(_ffi.c_dp), BC.CAP + 8, hlen))
    xs = MC.unpack_colmajor(xh, n, k, ld)
    got = [Col(code[j], st[j].iterations, st[j].final_residual, bool(st[j].converged), hlen[j], hist[j, :hlen[j]].copy(), xs[:, j]) for j in range(k)]
    assert_columns(got, from_reference(BC.reference(name, k, pc, guess=True)), "host twin")
    assert np.isnan(xh[n:ld]).all()                                  # the gap between two host columns is not written


# ---------------------------------------------------------------------------------------------------------------- 5. the C++ mirror
def test_cpp_block_cg_mirror():
    """tests/cpp/test_block_cg_mirror.cpp: BlockCgSolver::solve_block of include/kryst_hip.hpp against the C interface's host twin."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_block_cg_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_BLOCK_CG_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
