"""Multiple right-hand sides, the CPU tier: how columns are cut into multivectors, the packing, and the fixtures of test_gpu_multi_rhs.py
checked on the oracle alone -- if a fixture changes so that all of its columns behave alike, a test here fails, without a GPU."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import multi_rhs_cases as MC


def test_split_widths():
    want = {1: [1], 2: [2], 3: [2, 1], 4: [4], 5: [4, 1], 6: [4, 2], 7: [4, 2, 1], 8: [8], 9: [8, 1], 10: [8, 2], 11: [8, 2, 1], 12: [8, 4],
            13: [8, 4, 1], 14: [8, 4, 2], 15: [8, 4, 2, 1], 16: [8, 8], 17: [8, 8, 1], 64: [8] * 8}
    for m, w in want.items():
        got = K.split_widths(m)
        assert got == w, (m, got)
        assert sum(got) == m and all(x in (8, 4, 2, 1) for x in got) and got.count(1) <= 1          # no padding column, at most one single
        assert got == sorted(got, reverse=True)
    assert K.split_widths(0) == []
    with pytest.raises(ValueError):
        K.split_widths(-1)


@pytest.mark.parametrize("n,m,ld", [(1, 2, 1), (5, 3, 5), (5, 3, 9), (513, 8, 520), (0, 4, 0)])
def test_colmajor_packing_round_trips(n, m, ld):
    a = np.random.default_rng(n + m).standard_normal((n, m))
    a[::2, ::2] = -0.0
    for src in (np.ascontiguousarray(a), np.asfortranarray(a)):                      # either memory order
        buf = MC.pack_colmajor(src, ld)
        assert len(buf) == ld * m
        back = MC.unpack_colmajor(buf, n, m, ld)
        assert back.shape == (n, m) and np.array_equal(MC.bits(back), MC.bits(a))
        if ld > n and n:
            assert np.isnan(buf[n:ld]).all()                                         # the gap between two columns is not data
    il = MC.interleave(a)
    assert all(il[i * m + j] == a[i, j] for i in range(0, n, max(1, n // 7)) for j in range(m))
    assert np.array_equal(MC.bits(np.asfortranarray(a).ravel(order="F")), MC.bits(MC.pack_colmajor(a)))     # ld = n: numpy's own column-major


def test_spmm_operators_have_the_shapes_the_kernel_must_survive():
    ops = {k: f() for k, f in MC.SPMM_OPERATORS.items()}
    assert [ops[f"banded{n}"].nrows for n in (1, 127, 128, 511, 512, 513, 1025)] == [1, 127, 128, 511, 512, 513, 1025]
    rg = ops["ragged"]
    lens = np.diff(rg.row_ptr)
    assert 1900 < rg.nrows < 2100 and rg.nrows % 512 != 0 and (lens == 0).sum() > 300 and (lens[1024:1154] == 0).all() and lens.max() > 30
    lr = ops["long_rows"]
    ll = np.diff(lr.row_ptr)
    assert ll[101] == 3000 and ll[514] == 3000 and ll.max() == 3000 and np.median(ll) <= 4
    assert (ops["rect700x300"].nrows, ops["rect700x300"].ncols) == (700, 300)
    assert [ops[f"stencil{N}_poisson"].nrows for N in (8, 12, 16)] == [512, 1728, 4096]
    for kind in MC.SPECIAL_COLUMNS:
        assert len(MC.special_column(kind, 9)) == 9
    assert np.signbit(MC.special_column("negzero", 3)).all() and np.isnan(MC.special_column("nan", 3)).all()
    d = MC.special_column("denormal", 4)
    assert (d != 0).all() and (np.abs(d) < 2.3e-308).all()


@pytest.mark.parametrize("method,pc", [("cg", None), ("pcg", "jacobi")])
def test_block600_outcomes_on_the_oracle(method, pc):
    a, b = MC.block600(), MC.block600_columns()
    assert a.nrows == 600 and b.shape == (600, 8) and not b[:, 3].any()
    res = MC.oracle_columns(method, a, b, pc=pc)
    got = [(r.code, r.iterations, r.converged) for r in res]
    assert got == MC.BLOCK600_EXPECT[method], got
    assert res[3].final_residual == 0.0 and len(res[3].history) == 1              # the zero column: IndefiniteMatrix at once, residual 0
    assert len(res[0].history) == 151 and len(res[5].history) == 201              # one batch: a column frozen at 1 beside one that runs 200
    codes = {r.code for r in res}
    assert codes == ({0, MC.ERR_INDEFINITE_MATRIX} if method == "cg" else {0, MC.ERR_INDEFINITE_MATRIX, MC.ERR_INDEFINITE_PC})
    assert res[5].converged and res[5].final_residual / res[5].history[0] > MC.TOL   # the cap's `converged = true` is the reference's quirk


@pytest.mark.parametrize("N,kind,method,pc", MC.STENCIL_CASES)
def test_stencil_columns_do_not_all_stop_together(N, kind, method, pc):
    a, b = MC.stencil(N, kind), MC.stencil_columns(N, kind)
    res = MC.oracle_columns(method, a, b, pc=pc)
    its = [r.iterations for r in res]
    assert all(r.code == 0 and r.converged for r in res) and max(its) < MC.CAP, its
    assert len(set(its)) > 1, its
    assert [float(np.log10(np.abs(b[:, j]).max())) for j in (1, 7)] == pytest.approx([-2, 4], abs=0.1)      # the scales 10^(j - 3)
