"""The fixtures of the fp32 diagonal tests (tests/mixed_dia_cases.py) have the properties they are there for, rounding a diagonal stream entry
by entry is the rounding of the CSR values, the fp32 absent marker is what the header says it is, and the header, the C++ mirror, the Rust
binding and the Python binding carry the new names.  No GPU."""
import os
import re

import numpy as np
import pytest

import mixed_dia_cases as D
import mixed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    return {name: make() for name, make in D.OPERATORS.items()}


def test_diagonals_offsets_and_the_fill_rule(ops):
    assert set(D.DIAGONALS) == set(ops)
    for name, a in ops.items():
        offs = D.offsets(a)
        assert len(offs) == D.DIAGONALS[name] <= D.DIA_MAX, (name, len(offs))
        used, allowed = D.fill_rule(a)
        assert used <= allowed, (name, used, allowed)
        lo, hi = D.dia_min_max(a)
        assert lo == min(0, offs[0]) and hi == max(0, offs[-1])
        assert (np.diff(a.col_idx) > 0)[np.setdiff1d(np.arange(len(a.col_idx) - 1), a.row_ptr[1:-1] - 1)].all(), name      # ascending columns in a row
    want = {"tridiag1": [0], "tridiag3": [-1, 0, 1], "five_point": [-16, -1, 0, 1, 16], "nine_point": [-17, -16, -15, -1, 0, 1, 15, 16, 17],
            "varcoef12": [-144, -12, -1, 0, 1, 12, 144], "varbox16x16x20": [-256, -16, -1, 0, 1, 16, 256], "band11": list(range(-5, 6)),
            "far": [-2000, 0, 2000], "nonsquare": [0, 37, 100]}
    for name, offs in want.items():
        assert D.offsets(ops[name]).tolist() == offs, name
    # the arithmetic of the fill rule, as worked out by hand
    assert D.fill_rule(ops["five_point"]) == (1280, 1432.0)
    assert D.fill_rule(ops["nine_point"]) == (2304, 2444.5)
    assert D.fill_rule(ops["varcoef12"]) == (12096, 12700.0)
    assert D.fill_rule(ops["box27"]) == (216000, 219565.0)
    assert D.fill_rule(ops["far"]) == (48000, 49564.0)
    # small 27-point boxes fail it: 27 n^3 <= 1.125 (3 n - 2)^3 + 64 holds from n = 18 on (the 10^3 box of the row-pattern tests has no such form)
    for n, passes in ((10, False), (17, False), (18, True)):
        used, allowed = D.fill_rule(D.P.box(n, n, n, D.P.TAPS27))
        assert (used <= allowed) == passes, (n, used, allowed)
    # batches: 1 diagonal in a batch of 4; 11 in batches of 8 with a tail of 3; 2 / 4 / 6 in batches of 4, 8 in one of 8; 27 in 8 + 8 + 8 + 3
    assert {name: D.DIAGONALS[name] for name in ("band2", "band4", "band6", "band8", "band11", "box27")} == \
        {"band2": 2, "band4": 4, "band6": 6, "band8": 8, "band11": 11, "box27": 27}
    assert 11 % 8 == 3 and 27 % 8 == 3 and ops["band11"].nrows == 2049


def test_the_operators_of_the_refusals():
    """the band of the row-pattern refusal test SATISFIES the fill rule (5 * 2000 = 10000 <= 1.125 * 9966 + 64 = 11275.75) and has far more than
    256 distinct values, so under the defaults it is given diagonal streams; the operator that really fails the rule is sparse_diagonals()"""
    a = D.refusal_band()
    assert len(a.vals) == 9966 and D.fill_rule(a) == (10000, 11275.75) and len(np.unique(a.vals)) > 256
    s = D.sparse_diagonals()
    used, allowed = D.fill_rule(s)
    assert D.offsets(s).tolist() == [-9, -4, 0, 3, 8] and used == 10000 and used > allowed


def test_all_values_of_the_tridiagonal_operators_are_distinct(ops):
    for n in (1, 3, 1023, 1024, 1025, 2049):
        a = ops[f"tridiag{n}"]
        assert a.nrows == n and len(a.vals) == 3 * n - 2 and len(np.unique(a.vals)) == len(a.vals)
        assert len(np.unique(R.round_f32(a.vals)[0])) == len(a.vals)            # ... after the rounding too
    for name, make in D.SOLVE_OPERATORS.items():
        a = make()
        dense_ok = a.nrows <= 2000
        if dense_ok:
            m = a.to_dense()
            assert np.array_equal(m, m.T) and np.linalg.eigvalsh(m).min() > 0.0, name
    box = D.varbox(16, 16, 20)
    rows = np.repeat(np.arange(box.nrows), np.diff(box.row_ptr))
    order = np.lexsort((rows, box.col_idx))                                     # (col, row) order = the transpose's (row, col) order
    assert np.array_equal(box.col_idx[order], rows) and np.array_equal(box.vals[order], box.vals)       # symmetric
    assert (box.spmv(np.ones(box.nrows)) >= -1e-12).all() and box.spmv(np.ones(box.nrows)).max() >= 1.0   # diagonally dominant, strictly at the faces


def test_which_tiles_start_before_x0(ops):
    assert D.clamped_tiles(ops["varcoef12"]) == [0] and -(-ops["varcoef12"].nrows // D.TILE32) == 2          # tile 1 is on the fast path
    assert D.clamped_tiles(ops["varbox16x16x20"]) == [0] and ops["varbox16x16x20"].nrows == 5 * D.TILE32
    assert D.clamped_tiles(ops["far"]) == [0, 1] and -(-ops["far"].nrows // D.TILE32) == 16
    assert D.clamped_tiles(ops["box27"]) == [0] and D.clamped_tiles(ops["tridiag2049"]) == [0] and D.clamped_tiles(ops["band11"]) == [0]
    assert D.clamped_tiles(ops["nonsquare"]) == [] and D.clamped_tiles(ops["band2"]) == []                    # no diagonal below the main one
    assert D.clamped_tiles(ops["tridiag1"]) == []


def test_which_rows_point_beyond_the_allocation_of_x(ops):
    a = ops["far"]
    assert D.xcap(a.ncols) == 17408
    beyond = D.rows_pointing_beyond(a)
    assert beyond.tolist() == list(range(15408, 16000)) and beyond[-1] + 2000 == 17999
    for name in ops:
        if name != "far":
            assert len(D.rows_pointing_beyond(ops[name])) == 0, name            # elsewhere an absent entry points into the padding at most
    # ... which it does: the last row's upper neighbours lie in [ncols, xcap)
    a = ops["varcoef12"]
    assert a.ncols <= a.nrows - 1 + 144 < D.xcap(a.ncols)


def test_rounding_the_streams_is_rounding_the_values(ops):
    for name, a in ops.items():
        s32, refused = D.streams32(a)
        assert refused == 0, name
        present = s32 != D.ABSENT32
        assert present.sum() == len(a.vals), name
        offs = D.offsets(a)
        rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
        back = s32[np.searchsorted(offs, a.col_idx - rows), rows]               # the stream entries in CSR order
        assert np.array_equal(back, R.round_f32(a.vals)[0].view(np.uint32)), name
    # the special values: the ordinary NaN stays a NaN that is not the marker, -0.0 keeps its sign, 1e-50 becomes a present zero
    v = R.round_f32(ops["special_values"].vals)[0]
    assert np.isnan(v[1501]) and v[1501:1502].view(np.uint32)[0] == 0x7FC00000 and np.signbit(v[7]) and v[2500] == 0.0 and np.isinf(v[100])


def test_the_marker():
    m = np.array([D.ABSENT32], dtype=np.uint32)
    assert np.isnan(m.view(np.float32)[0]) and (m[0] >> 22) & 1 == 1 and m[0] >> 31 == 0                     # a quiet NaN
    canonical = R.store(np.array([np.nan, -np.nan, np.inf - np.inf])).view(np.uint32)
    assert D.ABSENT32 not in canonical.tolist() and int(D.ABSENT32) & 0x3FFFFF != 0                         # a payload (float) of the canonical NaN lacks
    assert R.store(np.array([D.ABSENT64]).view(np.float64)).view(np.uint32)[0] != D.ABSENT32                # not even the fp64 marker rounds onto it
    # the stored NaNs that do: refused
    for which in (0, 1):
        a = D.marker_twin(which)
        assert np.isnan(a.vals[1501])
        assert R.store(a.vals[1501:1502]).view(np.uint32)[0] == D.ABSENT32
        assert D.streams32(a)[1] == 1
        assert R.Lowered(a).info["rows"] == 1025                                # the plain lowering takes it


def test_unread_elements(ops):
    assert D.unread_elements(ops["tridiag_holes"]).tolist() == D.TRIDIAG_HOLES
    assert D.unread_elements(ops["varcoef12_holes"]).tolist() == D.VARCOEF_HOLES
    for name, holes in (("tridiag_holes", D.TRIDIAG_HOLES), ("varcoef12_holes", D.VARCOEF_HOLES)):
        a = ops[name]
        for x in D.poison_at(a.ncols, holes):
            assert np.isfinite(R.Lowered(a).spmv(x)).all(), name                # nothing sees the poisoned elements


def test_the_new_names():
    import kryst_amd as K
    h = open(os.path.join(ROOT, "include", "kryst_hip.h")).read()
    assert "#define KRYST_CSR32_DIA 3" in h
    assert re.search(r"#define KRYST_CSR32_DIA_ABSENT_BITS 0x%08Xu" % int(D.ABSENT32), h)
    assert K.lib().kryst_hip_abi_version() == 6                               # an opt-in form: the ABI version stays
    hpp = open(os.path.join(ROOT, "include", "kryst_hip.hpp")).read()
    assert "Dia = KRYST_CSR32_DIA" in hpp and '"dia"' in hpp
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub const KRYST_CSR32_DIA: i32 = 3;" in rs and "Dia = KRYST_CSR32_DIA" in rs
    assert "pub const KRYST_CSR32_DIA_ABSENT_BITS: u32 = 0x7FD1_A0D1;" in rs
    assert K.CsrMatrix32.FORMS_EXT == {"dia": 3} and K.CsrMatrix32.KERNELS_EXT == ("dia",) and K.CsrMatrix32.DIA_ABSENT_BITS == int(D.ABSENT32)
    assert K.CsrMatrix32.FORMS == {"plain": 0, "auto": 1, "pattern": 2} and K.CsrMatrix32.KERNELS == ("plain", "pattern", "pattern-stage")
    assert K.CsrMatrix32.form_code("dia") == 3 and K.CsrMatrix32.form_code("pattern") == 2
    with pytest.raises(K.KError) as e:
        K.CsrMatrix32.form_code("dia32")
    assert e.value.code == 102
    assert K.RefinementSolver(1e-10, 3).with_form("dia").form == "dia"
    with pytest.raises(K.KError):
        K.RefinementSolver(1e-10, 3).with_form("diagonal")
    mk = open(os.path.join(ROOT, "kryst_amd", "csrc", "Makefile")).read()
    assert "mixed_dia.hip" in mk
