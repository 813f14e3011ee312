"""The fixtures of the fp32 row-pattern tests (tests/mixed_pattern_cases.py) have the properties they are there for, the rounding of a pattern
table is the rounding of the CSR values, and the header and the built library carry the new entry points.  No GPU."""
import os

import numpy as np
import pytest

import mixed_pattern_cases as P
import mixed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    return {name: make() for name, (make, _) in P.OPERATORS.items()}


def test_every_operator_is_a_pattern_matrix(ops):
    for name, a in ops.items():
        rows, ids = P.distinct_rows(a)
        assert len(rows) <= 512, (name, len(rows))                              # KR_PMAX
        base_of = P.bases(rows)
        padded = sum(-(-len(rows[b]) // 8) * 8 for b in set(base_of.values()))
        assert padded <= 2048, (name, padded)                                   # KR_TMAX
        assert len(ids) == a.nrows


def test_line_lengths_decide_the_staged_kernel(ops):
    want = {"poisson16": 16, "poisson12": 12, "poisson18": 18, "box16x16x20": 16, "poisson16_holes": 16}
    for name, a in ops.items():
        n = P.line_length(a)
        assert n == want.get(name, 0), (name, n)
        staged = n >= 8 and n % 4 == 0
        assert (P.OPERATORS[name][1] == "pattern-stage") == staged, (name, n)
    assert P.line_length(ops["poisson18"]) % 4 == 2
    # tiles: 16^3 is 4 whole fp32 tiles, 12^3 ends in a partial one, the box has 5
    assert ops["poisson16"].nrows == 4 * P.TILE32 and ops["poisson12"].nrows % P.TILE32 == 704 and ops["box16x16x20"].nrows == 5 * P.TILE32


def test_which_quads_share_a_base(ops):
    share = {name: P.quads_sharing_a_base(a) for name, a in ops.items()}
    for name in ("poisson16", "poisson12", "poisson18", "box16x16x20", "tridiag1025", "five_point", "long_row", "wide"):
        assert share[name].all(), name                                          # boundary rows are sub-sequences of the interior row
    assert share["box27"].any() and not share["box27"].all()                    # a base of 27 entries has no sub-patterns: boundary rows stand alone
    assert not share["period2"][:-1].any() and not share["period3"][:-1].any()  # unrelated stencils side by side: the per-row walk
    # period 3: a quad starts at every phase, so every mix of the three bases occurs
    a = ops["period3"]
    assert {tuple((np.arange(4 * q, 4 * q + 4) % 3).tolist()) for q in range(a.nrows // 4)} == {(0, 1, 2, 0), (1, 2, 0, 1), (2, 0, 1, 2)}
    assert share["special_values"].any() and not share["special_values"].all()  # the changed rows are bases of their own
    assert share["empty_rows"].all()                                            # an empty row is a sub-sequence of anything
    # bases longer than 16 entries: the 27-point interior row and the 40-entry row
    assert max(len(r) for r in P.distinct_rows(ops["box27"])[0]) == 27 and max(len(r) for r in P.distinct_rows(ops["long_row"])[0]) == 40


def test_entries_before_x0_and_in_the_last_columns(ops):
    """a quad's gather for entry e starts at column 4t + off_e: it starts before x[0] where the quad's first rows lack the entry, and reaches
    into the last three columns (or past them, into the padding) at the other end"""
    for name in ("tridiag1025", "poisson16", "poisson18", "five_point", "box27"):
        a = ops[name]
        rows, ids = P.distinct_rows(a)
        base_of = P.bases(rows)
        first = rows[base_of[int(ids[0])]]                                      # the base of quad 0
        assert min(o for o, _ in first) < 0, name                               # ... has an entry whose gather starts before x[0]
        assert a.col_idx[a.row_ptr[0]] == 0                                     # ... which row 0 does not store
        q = 4 * ((a.nrows - 1) // 4)                                            # the last quad
        last = rows[base_of[int(ids[q])]]
        assert q + 3 + max(o for o, _ in last) >= a.ncols - 3, name
    for name, holes in (("tridiag_holes", P.TRIDIAG_HOLES), ("poisson16_holes", P.POISSON_HOLES)):
        a = ops[name]
        rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
        readers = rows[np.isin(a.col_idx, holes)]                               # rows that read a poisoned element: none, or the row itself
        assert 0 in holes and a.ncols - 1 in holes
        assert (len(readers) == 0) if name == "tridiag_holes" else (sorted(readers.tolist()) == sorted(holes))
        for x in P.poison_at(a.ncols, holes):
            seen = np.flatnonzero(~np.isfinite(R.Lowered(a).spmv(x)))           # nothing else may see the poisoned elements
            assert seen.tolist() == sorted(set(readers.tolist())), name


def test_shapes_of_the_other_fixtures(ops):
    assert ops["wide"].nrows < ops["wide"].ncols and ops["tall"].nrows > ops["tall"].ncols
    assert (np.diff(ops["tall"].row_ptr)[:100] == 0).all() and (np.diff(ops["tall"].row_ptr)[-50:] == 1).all()
    assert (np.diff(ops["empty_rows"].row_ptr) == 0).sum() == 206
    v = ops["special_values"].vals
    assert np.signbit(v[7]) and v[7] == 0.0 and np.isinf(v[100]) and np.isnan(v[1501])
    r32, changed, tiny, overflow = R.round_f32(v)
    assert overflow == 0 and tiny == 3 and r32[2500] == 0.0 and np.signbit(r32[2500]) and 0.0 < r32[2000] < R.TINY32 and r32[30] == 1.0
    a = ops["period3"]
    dense = a.to_dense()
    assert np.array_equal(dense, dense.T) and np.linalg.eigvalsh(dense).min() > 0.5


def test_rounding_the_table_is_rounding_the_values(ops):
    """the lowered table: every distinct (offset, value) row rounded entry by entry.  Expanded back through the ids it must be, bit for bit,
    mixed_ref.round_f32 of the CSR values"""
    for name, a in ops.items():
        rows, ids = P.distinct_rows(a)
        table = [R.store(np.array([v for _, v in r], dtype=np.uint64).view(np.float64)) for r in rows]
        expanded = np.concatenate([table[int(p)] for p in ids] + [np.zeros(0, np.float32)])
        want = R.round_f32(a.vals)[0]
        assert np.array_equal(expanded.view(np.uint32), want.view(np.uint32)), name


def test_two_fp64_values_that_round_to_one_fp32_value():
    a = P.twins()
    rows, _ = P.distinct_rows(a)
    interior = [r for r in rows if len(r) == 3]
    assert len(interior) == 2                                                   # two patterns in fp64 ...
    t = [R.store(np.array([v for _, v in r], dtype=np.uint64).view(np.float64)) for r in interior]
    assert np.array_equal(t[0].view(np.uint32), t[1].view(np.uint32))           # ... one row in fp32
    x = np.random.default_rng(3).standard_normal(a.ncols).astype(np.float32)
    ones = P.banded(a.nrows, a.ncols, [[(-1, 1.0), (0, 3.0), (1, 1.0)]], 1)
    assert np.array_equal(R.Lowered(a).spmv(x).view(np.uint32), R.Lowered(ones).spmv(x).view(np.uint32))


def test_header_and_library_export_the_new_symbols():
    import kryst_amd as K
    from kryst_amd import _ffi
    h = open(os.path.join(ROOT, "include", "kryst_hip.h")).read()
    for nm in ("kryst_csr32_lower_form", "kryst_csr32_encoding"):
        assert nm + "(" in h and nm in _ffi.SIGNATURES and hasattr(K.lib(), nm), nm
    for word in ("KRYST_CSR32_PLAIN 0", "KRYST_CSR32_AUTO 1", "KRYST_CSR32_PATTERN 2"):
        assert "#define " + word in h
    hpp = open(os.path.join(ROOT, "include", "kryst_hip.hpp")).read()
    assert "kryst_csr32_lower_form" in hpp and "std::string encoding() const" in hpp
    assert K.CsrMatrix32.FORMS == {"plain": 0, "auto": 1, "pattern": 2} and K.CsrMatrix32.KERNELS == ("plain", "pattern", "pattern-stage")
    assert hasattr(K.RefinementSolver, "with_form") and K.RefinementSolver(1e-10, 3).form == "plain"
