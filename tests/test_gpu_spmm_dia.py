"""Several right-hand sides on the diagonal (CSR-DIA) encoding: spmm_dia_kernel under kryst_spmm and the batched CG / Jacobi-PCG, on the GPU.

The rule of tests/test_gpu_multi_rhs.py, no tolerance: column j of a batched call is, bit for bit, what the single-vector call returns for
column j, and what the oracle computes.  Every comparison is made on uint64 views.  `spmm_kernel(k)` is asserted before a product or a solve,
so that no case passes because the other kernel ran: "dia" under KRYST_SPMM_FORM=dia on every operator that holds the streams, "plain" under
KRYST_SPMM_FORM=plain.  Fixtures: tests/spmm_dia_cases.py (their properties: tests/test_spmm_dia_cpu.py); the helpers that run and compare
batched solves are those of tests/test_gpu_multi_rhs.py."""
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import mixed_dia_cases as D
import multi_rhs_cases as MC
import spmm_dia_cases as S
import test_gpu_multi_rhs as T
from nonfinite_cases import same_ieee

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 102
bits, same = MC.bits, T.same
KNOBS = ("KRYST_SPMM_FORM", "KRYST_SPMM_BLOCKS_PER_CU", "KRYST_SPMM_DIA_NT", "KRYST_SPMV_COMPRESS", "KRYST_SPMV_DIA", "KRYST_FOLD_POLL")
# the widths at which KRYST_SPMM_FORM=auto takes the diagonal kernel on an operator whose own SpMV streams CSR-DIA
AUTO_DIA_WIDTHS = (2, 4, 8)
# created under KRYST_SPMV_DIA=2: operators with a handful of distinct values take a more compact form by default and would keep no streams
UNDER_DIA_2 = S.CONSTANT_COEFFICIENTS + ("tridiag1", "tridiag3")


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec() == MC.SPEC
    return K.Context(0)


def create(ctx, monkeypatch, a, dia=None):
    """the device operator, created under KRYST_SPMV_DIA=`dia` (None: the defaults)"""
    with monkeypatch.context() as m:
        m.delenv("KRYST_SPMV_DIA", raising=False)
        if dia is not None:
            m.setenv("KRYST_SPMV_DIA", dia)
        return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


_ops = {}


def device_operator(ctx, monkeypatch, name):
    if name not in _ops:
        _ops[name] = create(ctx, monkeypatch, S.operator(name), "2" if name in UNDER_DIA_2 else None)
    return _ops[name]


def enter(monkeypatch, form):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if form is not None:
        monkeypatch.setenv("KRYST_SPMM_FORM", form)


def spmm(ctx, d, x, want_kernel):
    assert d.spmm_kernel(x.shape[1]) == want_kernel, (d.spmm_kernel(x.shape[1]), want_kernel)
    return d.spmm(K.MultiVec.from_numpy(x, ctx=ctx)).to_numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. SpMM against SpMV and the oracle
@pytest.mark.parametrize("name", list(S.OPERATORS))
def test_spmm_dia_equals_spmv_per_column(ctx, monkeypatch, name):
    a, x8 = S.operator(name), S.xcols8(name)
    d = device_operator(ctx, monkeypatch, name)
    enter(monkeypatch, None)
    want = T.spmv_columns(ctx, d, x8)
    eq = same_ieee if name == "special_values" else same                      # stored inf and NaN: host and device make different default NaNs
    assert eq(want, S.want8(name)), name
    for k in S.WIDTHS:
        enter(monkeypatch, "dia")
        y = spmm(ctx, d, x8[:, :k], "dia")                                      # fails on a library without the kernel and the hook
        assert y.shape == (a.nrows, k)
        for j in range(k):
            assert same(y[:, j], want[:, j]), (name, k, j, int(np.sum(bits(y[:, j]) != bits(want[:, j]))))
        enter(monkeypatch, "plain")
        assert same(spmm(ctx, d, x8[:, :k], "plain"), y), (name, k)


def test_the_choice(ctx, monkeypatch):
    enter(monkeypatch, None)
    # an operator whose own SpMV streams CSR-DIA: auto takes the diagonal kernel for the widths that cleared the bar
    d = device_operator(ctx, monkeypatch, "varcoef12")
    assert d.encoding()[0] == "csr-dia"
    x8 = S.xcols8("varcoef12")
    for k in S.WIDTHS:
        enter(monkeypatch, None)
        auto = "dia" if k in AUTO_DIA_WIDTHS else "plain"
        y = spmm(ctx, d, x8[:, :k], auto)
        assert same(y, S.want8("varcoef12")[:, :k])
        for word, kernel in (("auto", auto), ("plain", "plain"), ("dia", "dia"), ("diagonal", auto)):
            enter(monkeypatch, word)
            assert same(spmm(ctx, d, x8[:, :k], kernel), y), (k, word)
        # with CSR-DIA switched off for the SpMV the streams are still there: auto follows the SpMV, dia does not
        enter(monkeypatch, None)
        monkeypatch.setenv("KRYST_SPMV_DIA", "0")
        assert d.encoding()[0] != "csr-dia" and d.spmm_kernel(k) == "plain"
        monkeypatch.setenv("KRYST_SPMM_FORM", "dia")
        assert d.spmm_kernel(k) == "dia"
    # a constant-coefficient operator that was given streams beside its row patterns: the SpMV streams the patterns, so auto stays plain
    enter(monkeypatch, None)
    p = device_operator(ctx, monkeypatch, "five_point")
    assert p.encoding()[0] != "csr-dia"
    assert [p.spmm_kernel(k) for k in S.WIDTHS] == ["plain"] * 3
    # no streams: `dia` falls back to the plain kernel without an error
    s = D.sparse_diagonals()
    x = MC.xcols(s.ncols, 8)
    for dia in (None, "2"):
        ds = create(ctx, monkeypatch, s, dia)
        for form in (None, "dia"):
            enter(monkeypatch, form)
            for k in S.WIDTHS:
                assert same(spmm(ctx, ds, x[:, :k], "plain"), MC.oracle_spmm(s, x[:, :k])), (dia, form, k)
    # a width that does not exist
    enter(monkeypatch, "dia")
    for k in (0, 1, 3, 16):
        with pytest.raises(K.KError) as e:
            d.spmm_kernel(k)
        assert e.value.code == ERR_ARG, k
    # a row-partitioned operator, made on this one rank: never the diagonal kernel, and kryst_spmm refuses it as before
    a = S.operator("tridiag1025")
    dd = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)
    assert dd.spmm_kernel(4) == "plain"
    with pytest.raises(K.KError) as e:
        dd.spmm(K.MultiVec.from_numpy(MC.xcols(a.ncols, 4), ctx=ctx))
    assert e.value.code == T.UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- 2. nothing leaks
@pytest.mark.parametrize("name", list(S.HOLES))
def test_special_columns_do_not_leak_into_their_neighbours(ctx, monkeypatch, name):
    a = S.operator(name)
    d = device_operator(ctx, monkeypatch, name)
    plain = S.xcols8(name)
    special = S.with_special_columns(plain, S.SPECIAL_AT)
    enter(monkeypatch, None)
    own = T.spmv_columns(ctx, d, special)
    enter(monkeypatch, "dia")
    for k in (4, 8):
        y_plain, y_special = spmm(ctx, d, plain[:, :k], "dia"), spmm(ctx, d, special[:, :k], "dia")
        assert same(y_plain, S.want8(name)[:, :k])
        for j in range(k):
            if j in S.SPECIAL_AT:
                assert same(y_special[:, j], own[:, j]), (name, k, S.SPECIAL_AT[j])        # the special column is its own spmv
            else:
                assert same(y_special[:, j], y_plain[:, j]), (name, k, j)                   # an ordinary column never sees its neighbours
        nonempty = np.diff(a.row_ptr) > 0
        assert np.isnan(y_special[nonempty, 1]).all() and not np.isnan(y_special[:, [0, 2]]).any()


@pytest.mark.parametrize("name", ["far", "nonsquare", "tridiag513"])
def test_results_do_not_depend_on_the_padding(ctx, monkeypatch, name):
    """absent entries of the last rows address X's padding rows (`far`: rows beyond the allocation, clamped into it); Y's padding is not written"""
    a = S.operator(name)
    d = device_operator(ctx, monkeypatch, name)
    enter(monkeypatch, "dia")
    for k in S.WIDTHS:
        x, want = S.xcols8(name)[:, :k], S.want8(name)[:, :k]
        xm, ym = K.MultiVec.from_numpy(x, ctx=ctx), K.MultiVec(ctx, a.nrows, k)
        assert d.spmm_kernel(k) == "dia" and xm.padding_dirty() == 0 and ym.padding_dirty() == 0
        assert same(d.spmm(xm, ym).to_numpy(), want), (name, k)
        xpad, ypad = (S.mvec_rows(a.ncols) - a.ncols) * k, (S.mvec_rows(a.nrows) - a.nrows) * k
        for value in (None, 1e300):
            xm.poison_padding(value)
            assert xm.padding_dirty() == xpad and ym.padding_dirty() == 0
            assert same(d.spmm(xm, ym).to_numpy(), want), (name, k, value, "X poisoned")
            assert ym.padding_dirty() == 0                                      # nothing was written behind Y's last row
            ym.poison_padding(value)
            assert same(d.spmm(xm, ym).to_numpy(), want), (name, k, value, "X and Y poisoned")
            assert ym.padding_dirty() == ypad and same(xm.to_numpy(), x)
            ym = K.MultiVec(ctx, a.nrows, k)


@pytest.mark.parametrize("name", list(S.HOLES))
def test_absent_entries_never_see_their_operand(ctx, monkeypatch, name):
    """NaN, +inf and -inf in every column exactly at the rows of X that only absent entries address: a lane's 16-byte loads cover them all the same"""
    a = S.operator(name)
    d = device_operator(ctx, monkeypatch, name)
    assert D.unread_elements(a).tolist() == S.HOLES[name]
    for k in S.WIDTHS:
        for x in S.poisoned_columns(a.ncols, k, S.HOLES[name]):
            want = MC.oracle_spmm(a, x)
            assert np.isfinite(want).all()
            enter(monkeypatch, "dia")
            assert same(spmm(ctx, d, x, "dia"), want), (name, k)


# ---------------------------------------------------------------------------------------------------------------- 3. the fused dot
def solve_many_columns(method, d, dpc, b, pick):
    s = T.SOLVER[method](MC.TOL, MC.CAP)
    xs = np.zeros((b.shape[0], len(pick)))
    res = s.solve_many(d, dpc, b[:, pick], xs)
    assert len(res) == len(pick) == len(s.residual_histories)
    return [T.Col(r.code if isinstance(r, K.KError) else 0, (r.stats if isinstance(r, K.KError) else r).iterations,
                  (r.stats if isinstance(r, K.KError) else r).final_residual, bool((r.stats if isinstance(r, K.KError) else r).converged),
                  len(h), np.array(h), xs[:, i].copy()) for i, (r, h) in enumerate(zip(res, s.residual_histories))]


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
@pytest.mark.parametrize("name", list(S.SOLVE_OPERATORS))
def test_batched_solves_on_the_diagonal_kernel(ctx, monkeypatch, name, method, pc):
    b = S.solve_columns(name)
    d = device_operator(ctx, monkeypatch, name)
    enter(monkeypatch, "dia")
    assert [d.spmm_kernel(k) for k in S.WIDTHS] == ["dia"] * 3
    dpc = T.make_pc(d, pc)
    x0 = np.zeros_like(b)
    ref = T.from_oracle(S.solve_reference(name, method, pc))
    one = T.single_columns(ctx, method, d, dpc, b, x0)
    T.assert_columns(one, ref, f"{name} {method}: single calls against the oracle")
    for k, cols in ((8, list(range(8))), (4, [0, 1, 2, 3]), (4, [4, 5, 6, 7]), (2, [0, 5]), (2, [6, 7])):
        T.assert_columns(T.batched(ctx, method, d, dpc, b[:, cols], x0[:, cols]), [one[j] for j in cols], f"{name} {method} k={k} columns {cols}")
    for m in (3, 7, 15):
        pick = [(3 * i + 1) % 8 for i in range(m)]
        T.assert_columns(solve_many_columns(method, d, dpc, b, pick), [one[j] for j in pick], f"{name} {method} solve_many m={m}")
    # the same bits from the plain kernel
    enter(monkeypatch, "plain")
    assert d.spmm_kernel(8) == "plain"
    T.assert_columns(T.batched(ctx, method, d, dpc, b, x0), one, f"{name} {method} k=8, plain kernel")


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_block600_every_exit_on_the_diagonal_kernel(ctx, monkeypatch, method, pc):
    """diag(T, -T): three diagonals whose off-diagonal streams have a hole where the two blocks meet; with its four distinct values the operator
    keeps streams only when it is created under KRYST_SPMV_DIA=2"""
    a, b = MC.block600(), MC.block600_columns()
    assert D.offsets(a).tolist() == [-1, 0, 1] and D.fill_rule(a)[0] <= D.fill_rule(a)[1] and S.interior_absent(a) == 2
    d = create(ctx, monkeypatch, a, "2")
    enter(monkeypatch, "dia")
    assert [d.spmm_kernel(k) for k in S.WIDTHS] == ["dia"] * 3
    dpc = T.make_pc(d, pc)
    x0 = np.zeros_like(b)
    ref = T.from_oracle(MC.oracle_columns(method, a, b, pc=pc))
    assert [(r.status, r.iterations, r.converged) for r in ref] == MC.BLOCK600_EXPECT[method]
    one = T.single_columns(ctx, method, d, dpc, b, x0)
    T.assert_columns(one, ref, f"{method}: single calls against the oracle")
    for k in S.WIDTHS:
        for cols in T.groups(8, k):
            T.assert_columns(T.batched(ctx, method, d, dpc, b[:, cols], x0[:, cols]), [one[j] for j in cols], f"{method} k={k} columns {cols}")
    for j, g in enumerate(T.batched(ctx, method, d, dpc, b, x0)):
        if g.status != 0:
            assert not g.x.any(), j                                            # x is not written back for a column that ended in an error
    for m in (3, 7, 15):
        pick = [(3 * i + 1) % 8 for i in range(m)]
        T.assert_columns(solve_many_columns(method, d, dpc, b, pick), [one[j] for j in pick], f"{method} solve_many m={m}")


# ---------------------------------------------------------------------------------------------------------------- 4. past one fold chunk
@pytest.fixture(scope="module")
def varcoef81(ctx):
    d = K.CsrMatrix.stencil7(81, "varcoef", ctx=ctx)
    n = 81 ** 3
    b = np.stack([O.splitmix64_uniform(0x5EED + j, n) * 10.0 ** (j - 1) for j in range(2)], axis=1)
    return d, b


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_past_one_fold_chunk(ctx, monkeypatch, varcoef81, method, pc):
    """531 441 rows > 524 288: 1038 tile partials per column, so the two-level fold runs its second stage and the capped grid strides"""
    d, b = varcoef81
    cap = 5
    assert b.shape[0] > 512 * 1024
    enter(monkeypatch, None)
    assert d.encoding()[0] == "csr-dia"
    dpc = T.make_pc(d, pc)
    x0 = np.zeros_like(b)
    one = T.single_columns(ctx, method, d, dpc, b, x0, cap=cap)
    assert all(c.iterations == cap and c.status == 0 for c in one)
    for form in ("1", "0"):
        enter(monkeypatch, "dia")
        monkeypatch.setenv("KRYST_FOLD_POLL", form)
        assert d.spmm_kernel(2) == "dia"
        T.assert_columns(T.batched(ctx, method, d, dpc, b, x0, cap=cap), one, f"{method} N=81 k=2 KRYST_FOLD_POLL={form}")


def test_spmm_past_the_capped_grid(ctx, monkeypatch, varcoef81):
    """1 038 tiles: at 1, 2 and 4 workgroups per compute unit the grid is capped below that on any device of up to 259 compute units and every
    workgroup strides; at 8 it is not capped on a device of 130 or more.  Neither the cap nor the kind of value load changes a bit."""
    d, _ = varcoef81
    x8 = MC.xcols(81 ** 3, 8)
    enter(monkeypatch, None)
    want = T.spmv_columns(ctx, d, x8)
    assert -(-81 ** 3 // S.TILE) == 1038
    for knob, values in ((None, (None,)), ("KRYST_SPMM_BLOCKS_PER_CU", ("1", "2", "4", "8")), ("KRYST_SPMM_DIA_NT", ("0",))):
        for v in values:
            enter(monkeypatch, "dia")
            if knob:
                monkeypatch.setenv(knob, v)
            for k in S.WIDTHS:
                assert same(spmm(ctx, d, x8[:, :k], "dia"), want[:, :k]), (knob, v, k)


# ---------------------------------------------------------------------------------------------------------------- 5. the C++ mirror
def test_cpp_spmm_dia_mirror():
    """tests/cpp/test_spmm_dia_mirror.cpp: HipCsrMatrix::spmm_kernel(k) of include/kryst_hip.hpp on a 1500-row tridiagonal operator"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_spmm_dia_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for k in KNOBS:
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_SPMM_DIA_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
