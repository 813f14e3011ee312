"""Several right-hand sides at once: kryst_mvec_t, kryst_spmm and the batched CG / Jacobi-PCG, on the GPU.

One rule, no tolerance: column j of a batched call is, bit for bit, what the single-vector call returns for column j -- y, x, the
iteration count, every residual-history entry, final_residual, converged and the status -- and what the oracle computes with the tiled
reduce.  Every comparison is made on uint64 views, so NaNs compare as bits too.  Fixtures: tests/multi_rhs_cases.py (their per-column
behaviour is asserted on the oracle alone in tests/test_multi_rhs_cpu.py)."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import multi_rhs_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, UNSUPPORTED = 102, 6
bits = MC.bits


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec() == MC.SPEC
    return K.Context(0)


def upload(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. SpMM against SpMV
def spmv_columns(ctx, d, x):
    return np.stack([d.spmv(ctx.vec(np.ascontiguousarray(x[:, j]))).to_host() for j in range(x.shape[1])], axis=1)


@pytest.mark.parametrize("name", list(MC.SPMM_OPERATORS))
def test_spmm_equals_spmv_per_column(ctx, name):
    a = MC.SPMM_OPERATORS[name]()
    d = upload(ctx, a)
    x8 = MC.xcols(a.ncols, 8)
    want = spmv_columns(ctx, d, x8)
    assert same(want, MC.oracle_spmm(a, x8)), name
    for k in MC.WIDTHS:
        y = d.spmm(K.MultiVec.from_numpy(x8[:, :k], ctx=ctx)).to_numpy()
        assert y.shape == (a.nrows, k)
        for j in range(k):
            assert same(y[:, j], want[:, j]), (name, k, j, int(np.sum(bits(y[:, j]) != bits(want[:, j]))))


def test_spmm_is_the_same_on_an_operator_with_a_compressed_form(ctx, monkeypatch):
    N = 16
    monkeypatch.delenv("KRYST_SPMV_COMPRESS", raising=False)
    packed = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    assert packed.encoding()[0] == "csr-p16"
    x8 = MC.xcols(N ** 3, 8)
    want = spmv_columns(ctx, packed, x8)                       # through the CSR-P16 kernel
    got_packed = {k: packed.spmm(K.MultiVec.from_numpy(x8[:, :k], ctx=ctx)).to_numpy() for k in MC.WIDTHS}
    monkeypatch.setenv("KRYST_SPMV_COMPRESS", "0")
    plain = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    assert plain.encoding()[0] == "csr"
    assert same(spmv_columns(ctx, plain, x8), want)
    assert same(want, MC.oracle_spmm(O.stencil7(N), x8))
    for k in MC.WIDTHS:
        got_plain = plain.spmm(K.MultiVec.from_numpy(x8[:, :k], ctx=ctx)).to_numpy()
        assert same(got_plain, want[:, :k]) and same(got_packed[k], want[:, :k]), k


# ---------------------------------------------------------------------------------------------------------------- 2. column isolation
def test_special_columns_do_not_leak_into_their_neighbours(ctx):
    a = MC.ragged()
    d = upload(ctx, a)
    plain = MC.xcols(a.ncols, 8, seed=3)
    special = plain.copy()
    where = {1: "nan", 3: "inf", 4: "negzero", 6: "denormal"}
    for j, kind in where.items():
        special[:, j] = MC.special_column(kind, a.ncols)
    y_plain = d.spmm(K.MultiVec.from_numpy(plain, ctx=ctx)).to_numpy()
    y_special = d.spmm(K.MultiVec.from_numpy(special, ctx=ctx)).to_numpy()
    own = spmv_columns(ctx, d, special)
    for j in range(8):
        if j in where:
            assert same(y_special[:, j], own[:, j]), where[j]              # the special column is its own spmv, NaN payloads included
        else:
            assert same(y_special[:, j], y_plain[:, j]), j                  # an ordinary column never sees its neighbours
    nonempty = np.diff(a.row_ptr) > 0
    assert np.isnan(y_special[nonempty, 1]).all() and not np.isnan(y_special[:, [0, 2, 5, 7]]).any()
    # the same with two and four columns: a NaN column beside an ordinary one
    for k in (2, 4):
        ys = d.spmm(K.MultiVec.from_numpy(special[:, :k], ctx=ctx)).to_numpy()
        assert same(ys[:, 0], y_plain[:, 0]) and same(ys[:, 1], own[:, 1])


# ---------------------------------------------------------------------------------------------------------------- 3. padding, aliasing
@pytest.mark.parametrize("n", [513, 1000])
def test_results_do_not_depend_on_the_padding(ctx, n):
    a = MC.banded(n)
    d = upload(ctx, a)
    for k in MC.WIDTHS:
        x = MC.xcols(n, k, seed=9)
        xm, ym = K.MultiVec.from_numpy(x, ctx=ctx), K.MultiVec(ctx, n, k)
        assert xm.padding_dirty() == 0 and ym.padding_dirty() == 0           # zero at creation, and an upload writes rows < n only
        clean = d.spmm(xm, ym).to_numpy()
        assert same(clean, MC.oracle_spmm(a, x))
        pad = ((n + 511) // 512 * 512 + 512 - n) * k
        for value in (None, 1e300):
            xm.poison_padding(value); ym.poison_padding(value)
            assert xm.padding_dirty() == pad and ym.padding_dirty() == pad
            assert same(d.spmm(xm, ym).to_numpy(), clean), (n, k, value)
            assert same(xm.to_numpy(), x)                                     # rows < n are untouched by the hook


def test_spmm_refuses_aliased_and_mismatched_operands(ctx):
    a = MC.banded(513)
    d = upload(ctx, a)
    x = MC.xcols(513, 4)
    xm = K.MultiVec.from_numpy(x, ctx=ctx)
    for other, why in ((xm, "X and Y the same"), (K.MultiVec(ctx, 513, 2), "k differs"), (K.MultiVec(ctx, 512, 4), "rows differ")):
        with pytest.raises(K.KError) as e:
            d.spmm(xm, other)
        assert e.value.code == ERR_ARG, why
    with pytest.raises(K.KError) as e:
        d.spmm(K.MultiVec(ctx, 512, 4), K.MultiVec(ctx, 513, 4))
    assert e.value.code == ERR_ARG
    assert same(xm.to_numpy(), x)                                             # refused before any launch
    # a row-partitioned operator, made on this one rank: its columns are local indices and halo slots, which this kernel does not know
    dd = K.CsrMatrix.from_csr_dist(ctx, 513, [0, 513], a.row_ptr, a.col_idx, a.vals)
    y0 = MC.xcols(513, 4, seed=2)
    ym = K.MultiVec.from_numpy(y0, ctx=ctx)
    with pytest.raises(K.KError) as e:
        dd.spmm(xm, ym)
    assert e.value.code == UNSUPPORTED
    assert same(ym.to_numpy(), y0) and same(xm.to_numpy(), x)
    for k in (0, 1, 3, 5, 16):
        with pytest.raises(K.KError) as e:
            K.MultiVec(ctx, 10, k)
        assert e.value.code == ERR_ARG, k


# ---------------------------------------------------------------------------------------------------------------- 4. transfers, columns
@pytest.mark.parametrize("n,k", [(1, 2), (700, 4), (1025, 8)])
def test_upload_download_and_column_access(ctx, n, k):
    a = MC.xcols(n, k, seed=33)
    a[::3, 0] = -0.0
    lib = K.lib()
    mv = K.MultiVec(ctx, n, k)
    up = MC.pack_colmajor(a, n + 7)                                            # ld > n, NaN in the gaps
    K.check(lib.kryst_mvec_upload(mv.h, up.ctypes.data_as(_ffi.c_dp), n + 7))
    assert same(mv.to_numpy(), a) and mv.padding_dirty() == 0
    down = np.full((n + 3) * k, -7.0)
    K.check(lib.kryst_mvec_download(mv.h, down.ctypes.data_as(_ffi.c_dp), n + 3))
    assert same(MC.unpack_colmajor(down, n, k, n + 3), a)
    assert all((down[j * (n + 3) + n:(j + 1) * (n + 3)] == -7.0).all() for j in range(k))      # the gaps of the host buffer stay as they were
    assert lib.kryst_mvec_upload(mv.h, up.ctypes.data_as(_ffi.c_dp), n - 1) == ERR_ARG
    nn, kk = C.c_int64(), C.c_int32()
    K.check(lib.kryst_mvec_shape(mv.h, C.byref(nn), C.byref(kk)))
    assert (nn.value, kk.value) == (n, k) == mv.shape
    for order in ("C", "F"):                                                   # from_numpy takes either memory order
        assert same(K.MultiVec.from_numpy(np.array(a, order=order), ctx=ctx).to_numpy(), a)
    for j in range(k):
        assert same(mv.column(j).to_host(), a[:, j])
    v = np.random.default_rng(k).standard_normal(n)
    mv.set_column(k - 1, ctx.vec(v))
    a[:, k - 1] = v
    assert same(mv.to_numpy(), a)
    for bad in (-1, k):
        assert lib.kryst_mvec_get_column(mv.h, bad, ctx.vec(n).h) == ERR_ARG
    assert lib.kryst_mvec_set_column(mv.h, 0, ctx.vec(n + 1).h) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 5. batched CG / PCG
Col = collections.namedtuple("Col", "status iterations final_residual converged hist_len history x")
SOLVER = {"cg": K.CgSolver, "pcg": K.PcgSolver}
UNPREC = K.CgNormType.Unpreconditioned


def make_pc(d, pc):
    return {None: lambda: None, "identity": lambda: K.IdentityPc().setup(d), "jacobi": lambda: K.Jacobi().setup(d)}[pc]()


def single_columns(ctx, method, d, pc, b, x0, tol=MC.TOL, cap=MC.CAP, norm=UNPREC):
    """kryst_cg_solve_dev / kryst_pcg_solve_dev on every column"""
    out = []
    for j in range(b.shape[1]):
        s = SOLVER[method](tol, cap).with_norm(norm)
        bv, xv = ctx.vec(np.ascontiguousarray(b[:, j])), ctx.vec(np.ascontiguousarray(x0[:, j]))
        try:
            st, code = s.solve(d, pc, bv, xv), 0
        except K.KError as e:
            st, code = e.stats, e.code
        out.append(Col(code, st.iterations, st.final_residual, bool(st.converged), len(s.residual_history), np.array(s.residual_history), xv.to_host()))
    return out


def batched(ctx, method, d, pc, b, x0, tol=MC.TOL, cap=MC.CAP, norm=UNPREC, hist_cap=None, alias=False, edit=None, expect_rc=0):
    """kryst_cg_solve_multi_dev / kryst_pcg_solve_multi_dev, raw"""
    k = b.shape[1]
    bm = K.MultiVec.from_numpy(b, ctx=ctx)
    xm = bm if alias else K.MultiVec.from_numpy(x0, ctx=ctx)
    prm = _ffi.Params(tol, cap, 0, 1, int(norm), 0, 0, 0.0, 0, 0.0, 0)
    if edit:
        edit(prm)
    hist_cap = cap + 8 if hist_cap is None else hist_cap
    st, code, hlen = (_ffi.Stats * k)(), (C.c_int32 * k)(*([-99] * k)), (C.c_int64 * k)(*([-99] * k))
    hist = np.full((k, max(hist_cap, 1)), -99.0)
    rc = getattr(K.lib(), f"kryst_{method}_solve_multi_dev")(bm.h, xm.h, d.h, pc.h if pc is not None else None, C.byref(prm), st, code,
                                                             hist.ctypes.data_as(_ffi.c_dp), hist_cap, hlen)
    assert rc == expect_rc, (rc, K.lib().kryst_hip_last_error())
    xs = xm.to_numpy()
    if rc != 0:
        return list(code), list(hlen), hist, xs
    assert (hist[:, hist_cap:] == -99.0).all()
    return [Col(code[j], st[j].iterations, st[j].final_residual, bool(st[j].converged), hlen[j], hist[j, :min(hlen[j], hist_cap)].copy(), xs[:, j].copy())
            for j in range(k)]


def from_oracle(res):
    return [Col(r.code, r.iterations, r.final_residual, bool(r.converged), len(r.history), np.asarray(r.history), r.x) for r in res]


def assert_columns(got, want, label, hist_cap=None):
    assert len(got) == len(want), label
    for j, (g, w) in enumerate(zip(got, want)):
        lab = (label, j)
        assert (g.status, g.iterations, g.converged, g.hist_len) == (w.status, w.iterations, w.converged, w.hist_len), (lab, g[:5], w[:5])
        assert same([g.final_residual], [w.final_residual]), (lab, g.final_residual, w.final_residual)
        wh = w.history if hist_cap is None else w.history[:hist_cap]
        assert same(g.history, wh), (lab, "history")
        assert same(g.x, w.x), (lab, "x", int(np.sum(bits(g.x) != bits(w.x))))


def groups(m, k):
    return [list(range(at, at + k)) for at in range(0, m - k + 1, k)]


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_block600_every_exit_in_one_batch(ctx, method, pc):
    a, b = MC.block600(), MC.block600_columns()
    d = upload(ctx, a)
    dpc = make_pc(d, pc)
    x0 = np.zeros_like(b)
    ref = from_oracle(MC.oracle_columns(method, a, b, pc=pc))
    assert [(r.status, r.iterations, r.converged) for r in ref] == MC.BLOCK600_EXPECT[method]
    one = single_columns(ctx, method, d, dpc, b, x0)
    assert_columns(one, ref, f"{method}: single calls against the oracle")
    for k in MC.WIDTHS:
        for cols in groups(8, k):
            got = batched(ctx, method, d, dpc, b[:, cols], x0[:, cols])
            assert_columns(got, [one[j] for j in cols], f"{method} k={k} columns {cols}")
    got8 = batched(ctx, method, d, dpc, b, x0)
    for j, g in enumerate(got8):
        if g.status != 0:
            assert not g.x.any(), j                                            # x is not written back for a column that ended in an error
    # any number of columns through solve_many: 3 -> 2 + 1, 7 -> 4 + 2 + 1, 15 -> 8 + 4 + 2 + 1
    for m in (3, 7, 15):
        pick = [(3 * i + 1) % 8 for i in range(m)]
        s = SOLVER[method](MC.TOL, MC.CAP)
        xs = np.zeros((600, m))
        res = s.solve_many(d, dpc, b[:, pick], xs)
        assert len(res) == m == len(s.residual_histories)
        got = [Col(r.code if isinstance(r, K.KError) else 0, (r.stats if isinstance(r, K.KError) else r).iterations,
                   (r.stats if isinstance(r, K.KError) else r).final_residual, bool((r.stats if isinstance(r, K.KError) else r).converged),
                   len(h), np.array(h), xs[:, i].copy()) for i, (r, h) in enumerate(zip(res, s.residual_histories))]
        assert_columns(got, [one[j] for j in pick], f"{method} solve_many m={m}")


@pytest.mark.parametrize("N,kind,method,pc", MC.STENCIL_CASES)
def test_stencil_columns_that_stop_at_different_iterations(ctx, N, kind, method, pc):
    a, b = MC.stencil(N, kind), MC.stencil_columns(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)                                  # carries its compressed forms: the single calls stream those
    dpc = make_pc(d, pc)
    x0 = np.zeros_like(b)
    ref = from_oracle(MC.oracle_columns(method, a, b, pc=pc))
    assert len({r.iterations for r in ref}) > 1
    one = single_columns(ctx, method, d, dpc, b, x0)
    assert_columns(one, ref, "single calls against the oracle")
    for k, cols in ((8, list(range(8))), (4, [0, 1, 2, 3]), (2, [0, 5])):
        assert_columns(batched(ctx, method, d, dpc, b[:, cols], x0[:, cols]), [one[j] for j in cols], f"{method} {kind} N={N} k={k}")


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi"), ("pcg", "identity"), ("pcg", None)])
def test_caps_and_history_buffers(ctx, method, pc):
    N, kind = 8, "poisson"
    a, b = MC.stencil(N, kind), MC.stencil_columns(N, kind)[:, :4]
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    dpc = make_pc(d, pc)
    x0 = MC.guesses(a.nrows, 4)
    for cap in (0, 1, 2, 9):
        ref = from_oracle(MC.oracle_columns(method, a, b, x0=x0, pc=pc, max_iters=cap))
        assert all(r.hist_len == cap + 1 for r in ref)
        got = batched(ctx, method, d, dpc, b, x0, cap=cap)
        assert_columns(got, ref, f"{method} pc={pc} max_iters={cap}")
        assert_columns(got, single_columns(ctx, method, d, dpc, b, x0, cap=cap), f"{method} pc={pc} max_iters={cap} (single)")
    # hist_cap = 3 with more pushes than that: hist_len still counts every push, the slices do not run into each other
    ref = from_oracle(MC.oracle_columns(method, a, b, x0=x0, pc=pc, max_iters=9))
    assert_columns(batched(ctx, method, d, dpc, b, x0, cap=9, hist_cap=3), ref, f"{method} hist_cap=3", hist_cap=3)
    assert_columns(batched(ctx, method, d, dpc, b, x0, cap=9, hist_cap=0), ref, f"{method} hist_cap=0", hist_cap=0)
    # the norm the history records: Preconditioned
    prec = K.CgNormType.Preconditioned
    ref = from_oracle(MC.oracle_columns(method, a, b, x0=x0, pc=pc, norm_type=int(prec)))
    assert_columns(batched(ctx, method, d, dpc, b, x0, norm=prec), ref, f"{method} pc={pc} Preconditioned norm")


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_initial_guesses_aliasing_and_the_host_twin(ctx, method, pc):
    N, kind = 12, "aniso" if method == "pcg" else "poisson"
    a, b = MC.stencil(N, kind), MC.stencil_columns(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
    dpc = make_pc(d, pc)
    x0 = MC.guesses(a.nrows, 8)
    ref = from_oracle(MC.oracle_columns(method, a, b, x0=x0, pc=pc))
    for k in MC.WIDTHS:
        assert_columns(batched(ctx, method, d, dpc, b[:, :k], x0[:, :k]), ref[:k], f"{method} x0 != 0, k={k}")
    # B and X the same multivector: x0 = b, and the multivector holds x afterwards
    ref_b = from_oracle(MC.oracle_columns(method, a, b, x0=b, pc=pc))
    assert_columns(batched(ctx, method, d, dpc, b[:, :4], None, alias=True), ref_b[:4], f"{method} B is X")
    # the block matrix with x0 != 0: the columns that end in an error keep their guess
    a6, b6 = MC.block600(), MC.block600_columns()
    d6 = upload(ctx, a6)
    g6 = MC.guesses(600, 8, seed=5) * 1e-3
    g6[300:] = 0.0                                                             # (a guess on the indefinite half would end every column at once)
    ref6 = from_oracle(MC.oracle_columns(method, a6, b6, x0=g6, pc=pc))
    assert any(r.status != 0 for r in ref6) and any(r.status == 0 for r in ref6)
    got6 = batched(ctx, method, d6, make_pc(d6, pc), b6, g6)
    assert_columns(got6, ref6, f"{method} block600 with guesses")
    # host arrays, column-major with ld > n
    k, n, ld = 4, 600, 611
    bh, xh = MC.pack_colmajor(b6[:, :k], ld), MC.pack_colmajor(g6[:, :k], ld)
    prm = _ffi.Params(MC.TOL, MC.CAP, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    st, code, hlen = (_ffi.Stats * k)(), (C.c_int32 * k)(), (C.c_int64 * k)()
    hist = np.zeros((k, MC.CAP + 8))
    dpc6 = make_pc(d6, pc)
    K.check(getattr(K.lib(), f"kryst_{method}_solve_multi")(bh.ctypes.data_as(_ffi.c_dp), xh.ctypes.data_as(_ffi.c_dp), n, k, ld, d6.h,
                                                            dpc6.h if dpc6 is not None else None, C.byref(prm), st, code,
                                                            hist.ctypes.data_as(_ffi.c_dp), MC.CAP + 8, hlen))
    xs = MC.unpack_colmajor(xh, n, k, ld)
    host = [Col(code[j], st[j].iterations, st[j].final_residual, bool(st[j].converged), hlen[j], hist[j, :hlen[j]].copy(), xs[:, j]) for j in range(k)]
    assert_columns(host, ref6[:k], f"{method} host twin")
    assert np.isnan(xh[n:ld]).all()                                            # the gap between two host columns is not written


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_past_one_fold_chunk(ctx, method, pc, monkeypatch):
    """531 441 rows > 524 288: the inner products' two-level fold runs its second stage, in both hand-offs"""
    N, cap = 81, 3
    a = O.stencil7(N)
    assert a.nrows > 512 * 1024
    b = np.stack([a.spmv(np.ones(a.nrows))] + [O.splitmix64_uniform(0x5EED + j, a.nrows) * 10.0 ** (j - 3) for j in range(1, 8)], axis=1)
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    dpc = make_pc(d, pc)
    x0 = np.zeros_like(b)
    ref = from_oracle(MC.oracle_columns(method, a, b, pc=pc, max_iters=cap))
    assert all(r.iterations == cap and r.converged for r in ref)
    assert_columns(single_columns(ctx, method, d, dpc, b[:, :2], x0[:, :2], cap=cap), ref[:2], "single calls against the oracle")
    for form in ("1", "0"):
        monkeypatch.setenv("KRYST_FOLD_POLL", form)
        assert_columns(batched(ctx, method, d, dpc, b, x0, cap=cap), ref, f"{method} N=81 k=8 KRYST_FOLD_POLL={form}")


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched(ctx):
    N = 8
    a, b = MC.stencil(N, "poisson"), MC.stencil_columns(N, "poisson")[:, :4]
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    x0 = MC.guesses(a.nrows, 4)
    jac, ilu = K.Jacobi().setup(d), K.Ilu0().setup(d)

    def refused(method, pc, code, op=None, **kw):
        status, hlen, hist, xs = batched(ctx, method, d if op is None else op, pc, b, x0, expect_rc=code, **kw)
        assert status == [-99] * 4 and hlen == [-99] * 4 and (hist == -99.0).all() and same(xs, x0), (method, code, kw)

    refused("pcg", ilu, UNSUPPORTED)                                            # a preconditioner other than Identity / Jacobi
    dd = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)      # a row-partitioned operator on this one rank
    refused("cg", None, UNSUPPORTED, op=dd)
    refused("pcg", jac, UNSUPPORTED, op=dd)
    refused("pcg", None, UNSUPPORTED, op=dd)
    for method, pc in (("cg", None), ("pcg", jac)):
        refused(method, pc, UNSUPPORTED, norm=K.CgNormType.Natural)
        refused(method, pc, UNSUPPORTED, norm=K.CgNormType.NoNorm)
        refused(method, pc, UNSUPPORTED, edit=lambda p: (setattr(p, "has_radius", 1), setattr(p, "radius", 1.0)))
        refused(method, pc, UNSUPPORTED, edit=lambda p: (setattr(p, "has_obj_target", 1), setattr(p, "obj_target", -1.0)))
        refused(method, pc, ERR_ARG, cap=-1)
    # shapes that do not match
    lib = K.lib()
    prm = _ffi.Params(MC.TOL, 10, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
    bm = K.MultiVec.from_numpy(b, ctx=ctx)
    for xm in (K.MultiVec(ctx, a.nrows, 2), K.MultiVec(ctx, a.nrows + 1, 4)):
        assert lib.kryst_cg_solve_multi_dev(bm.h, xm.h, d.h, None, C.byref(prm), None, None, None, 0, None) == ERR_ARG
    # CG ignores pc like the single call (cg.rs:115): ILU0 is accepted there and changes nothing
    assert_columns(batched(ctx, "cg", d, ilu, b, x0), batched(ctx, "cg", d, None, b, x0), "cg ignores pc")
    # k = 3 exists nowhere: not as a multivector, not in the host twin
    st, code, hlen = (_ffi.Stats * 3)(), (C.c_int32 * 3)(), (C.c_int64 * 3)()
    bh, xh = MC.pack_colmajor(b[:, :3]), MC.pack_colmajor(x0[:, :3])
    keep = xh.copy()
    assert lib.kryst_cg_solve_multi(bh.ctypes.data_as(_ffi.c_dp), xh.ctypes.data_as(_ffi.c_dp), a.nrows, 3, a.nrows, d.h, None, C.byref(prm), st, code,
                                    None, 0, hlen) == ERR_ARG
    assert same(xh, keep)
    # a solver without a batched form
    with pytest.raises(K.KError) as e:
        K.BiCgStabSolver(1e-8, 10).solve_many(d, None, b, x0.copy())
    assert e.value.code == UNSUPPORTED
    # B a MultiVec and X an array (or the other way round): an argument error, not an AttributeError
    for bb, xx in ((bm, x0.copy()), (b, K.MultiVec.from_numpy(x0, ctx=ctx))):
        with pytest.raises(K.KError) as e:
            K.CgSolver(1e-8, 10).solve_many(d, None, bb, xx)
        assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 7. the C++ mirror
def test_cpp_multi_mirror():
    """tests/cpp/test_multi_mirror.cpp: two columns of the reference's 2 x 2 CG case (cg.rs:310-323) through include/kryst_hip.hpp."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_multi_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_MULTI_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
