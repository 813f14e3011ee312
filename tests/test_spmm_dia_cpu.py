"""The fixtures of the diagonal SpMM tests (tests/spmm_dia_cases.py) have the properties they are there for, the column-wise restatement of
the kernel's contract is the oracle's SpMV on every column, and the Python binding carries the new hook.  No GPU."""
import numpy as np
import pytest

import mixed_dia_cases as D
import multi_rhs_cases as MC
import spmm_dia_cases as S
from nonfinite_cases import same_ieee

bits = MC.bits


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. the fixtures
def test_every_operator_satisfies_the_fill_rule_and_has_its_diagonals():
    assert set(S.DIAGONALS) == set(S.OPERATORS) and set(D.OPERATORS) < set(S.OPERATORS)
    for name in S.OPERATORS:
        a = S.operator(name)
        used, allowed = D.fill_rule(a)
        assert used <= allowed, (name, used, allowed)
        assert len(D.offsets(a)) == S.DIAGONALS[name] <= D.DIA_MAX, name
    for name in S.SOLVE_OPERATORS:
        a = S.operator(name)
        used, allowed = D.fill_rule(a)
        assert used <= allowed and len(D.offsets(a)) in (3, 7), name
    for n in (511, 512, 513):
        assert S.operator(f"tridiag{n}").nrows == n
    # every batch shape of the kernel: 1, 2, 3, 4, 5, 6, 7, 8, 9, 11 and 27 diagonals -- the exact instantiations (3, 5, 7, 9), one batch with a
    # tail (1, 2, 6), whole batches (4, 8) and several batches with a tail (11 = 8 + 3 = 4 + 4 + 3, 27 = 8 + 8 + 8 + 3, odd: a tail at 2 per batch)
    assert sorted(set(S.DIAGONALS.values())) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 27]
    # the operator that has no diagonal form
    used, allowed = D.fill_rule(D.sparse_diagonals())
    assert used > allowed


def test_the_set_reaches_every_path_of_the_kernel():
    tiles = {name: S.clamped_tiles(S.operator(name)) for name in S.OPERATORS}
    ntiles = {name: -(-S.operator(name).nrows // S.TILE) for name in S.OPERATORS}
    # the clamped path (r0 + dia_min < 0) and, in the same operator, tiles on the fast path
    assert tiles["far"] == [0, 1, 2, 3] and ntiles["far"] == 32                # offsets +-2000: four tiles clamp at the bottom
    assert tiles["varcoef12"] == [0] and ntiles["varcoef12"] == 4
    assert tiles["tridiag513"] == [0] and ntiles["tridiag513"] == 2 and tiles["tridiag512"] == [0] and ntiles["tridiag512"] == 1
    assert tiles["nonsquare"] == [] and tiles["band2"] == [] and tiles["tridiag1"] == []      # no diagonal below the main one: fast path only
    assert any(t for t in tiles.values()) and any(len(t) < ntiles[name] for name, t in tiles.items())
    # rows whose absent entry points at or beyond the allocated rows of X: only the clamp at mvec_rows - 2 keeps those loads inside
    a = S.operator("far")
    assert S.mvec_rows(a.ncols) == 16896
    beyond = S.rows_pointing_beyond(a)
    assert beyond.tolist() == list(range(14896, 16000))
    assert all(len(S.rows_pointing_beyond(S.operator(name))) == 0 for name in S.OPERATORS if name != "far")
    # ... elsewhere an absent entry of the last rows points into X's padding rows
    a = S.operator("varcoef12")
    assert a.ncols <= a.nrows - 1 + 144 < S.mvec_rows(a.ncols) and S.mvec_rows(a.ncols) == 2560
    a = S.operator("nonsquare")                                                # none of its entries is clipped: 1299 + 100 < 1400
    assert a.nrows - 1 + 100 < a.ncols and S.mvec_rows(a.ncols) == 2048 and S.interior_absent(a) == 0
    # absent entries in the interior
    for name, holes in S.HOLES.items():
        assert S.interior_absent(S.operator(name)) > 0, name
        assert D.unread_elements(S.operator(name)).tolist() == holes, name
    assert S.interior_absent(S.operator("tridiag1025")) == 0 and S.interior_absent(S.operator("far")) == 0
    assert S.interior_absent(S.operator("varcoef12")) > 0                      # a grid operator's faces: the neighbour across a line's end


def test_mvec_rows():
    assert [S.mvec_rows(n) for n in (1, 511, 512, 513, 1300, 1400)] == [1024, 1024, 1024, 1536, 2048, 2048]


# ---------------------------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("name", list(S.OPERATORS))
def test_the_column_wise_fold_is_the_oracle(name):
    a = S.operator(name)
    eq = same_ieee if name == "special_values" else same                      # stored inf and NaN: a NaN's sign and payload do not count
    got = S.fold_columns(a, S.xcols8(name))
    assert eq(got, S.want8(name)), (name, int(np.sum(bits(got) != bits(S.want8(name)))))
    if a.ncols > 8:
        x = S.with_special_columns(S.xcols8(name), S.SPECIAL_AT)
        got, want = S.fold_columns(a, x), MC.oracle_spmm(a, x)
        for j in range(8):
            assert (same_ieee if j in S.SPECIAL_AT or name == "special_values" else same)(got[:, j], want[:, j]), (name, j)
            if j not in S.SPECIAL_AT:
                assert same(want[:, j], S.want8(name)[:, j])                  # an ordinary column is what it was


def test_the_fold_skips_what_absent_entries_point_at():
    for name, holes in S.HOLES.items():
        a = S.operator(name)
        clean = S.fold_columns(a, S.xcols8(name)[:, :2])
        for x in S.poisoned_columns(a.ncols, 2, holes):
            y = S.fold_columns(a, x)
            assert np.isfinite(y).all() and same(y, MC.oracle_spmm(a, x)), name
        assert np.isfinite(clean).all()


def test_solver_fixtures_stop_at_different_iterations():
    level = []
    for name in S.SOLVE_OPERATORS:
        for method, pc in (("cg", None), ("pcg", "jacobi")):
            ref = S.solve_reference(name, method, pc)
            assert len(ref) == 8 and all(r.code == 0 and r.converged and 30 < r.iterations < MC.CAP for r in ref), (name, method)
            if len({r.iterations for r in ref}) == 1:
                level.append((name, method))
    assert level == [("tridiag_spd1023", "pcg")]                              # the one case whose eight columns all take 41 iterations


# ---------------------------------------------------------------------------------------------------------------- 3. the new names
def test_the_new_names():
    import kryst_amd as K
    from kryst_amd import _ffi
    assert "kryst_spmm_kernel" in _ffi.SIGNATURES and hasattr(K.lib(), "kryst_spmm_kernel")
    assert K.CsrMatrix.SPMM_KERNELS == ("plain", "dia") and callable(K.CsrMatrix.spmm_kernel)
