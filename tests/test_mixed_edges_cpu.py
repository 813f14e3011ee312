"""No GPU: the fixtures of tests/mixed_edge_cases.py have the properties they are there for, for every window size in WINDOWS, and the
inputs of the range tests do to the restatement (tests/mixed_ref.py) what tests/test_gpu_mixed_edges.py relies on.  These are conditions
on the inputs: when a generator change breaks one, the generator is changed back, not the condition."""
import numpy as np
import pytest

import mixed_cases as MC
import mixed_edge_cases as E
import mixed_ref as R

WAVE = E.WAVE


def wave_of_row(a):
    return np.arange(a.nrows) // WAVE


def test_wave_runs():
    rp = np.concatenate([[0], np.cumsum(np.arange(600) % 3)])
    runs = E.wave_runs(rp)
    assert runs.shape == (3, 2) and runs.tolist() == [[rp[0], rp[256]], [rp[256], rp[512]], [rp[512], rp[600]]]
    assert E.wave_runs(np.zeros(1025, dtype=np.int64)).shape == (4, 2)
    assert E.wave_bases(np.array([0, 7] + [7] * 255 + [9]))[1] == 4


@pytest.mark.parametrize("w", E.WINDOWS)
def test_runs_at_window_edges(w):
    a = E.runs_at_window_edges()
    runs = E.wave_runs(a.row_ptr)
    lens = set((runs[:, 1] - runs[:, 0]).tolist())
    assert {w - 1, w, w + 1, 2 * w, 2 * w + 1} <= lens
    assert set((runs[:, 0] % 4).tolist()) == {0, 1, 2, 3}
    base = E.wave_bases(a.row_ptr)[wave_of_row(a)]
    ends_on_boundary = (a.row_ptr[1:] == base + w) & (E.row_lengths(a) > 0)
    assert ends_on_boundary.any()
    assert a.nrows == WAVE * len(E.EDGE_RUNS) and 2000 < a.nrows < 5000


@pytest.mark.parametrize("w", E.WINDOWS)
def test_straddlers(w):
    a = E.straddlers()
    rp, ln = a.row_ptr, E.row_lengths(a)
    runs, bases = E.wave_runs(rp), E.wave_bases(rp)
    # one row crosses every boundary inside its wave's run
    i = int(np.argmax(ln))
    g = i // WAVE
    inside = bases[g] + w * np.arange(1, (runs[g, 1] - bases[g]) // w + 2)
    inside = inside[(inside > runs[g, 0]) & (inside < runs[g, 1])]
    assert len(inside) >= 3 and (rp[i] < inside).all() and (inside < rp[i + 1]).all()
    # ... and spans at least three windows of 4096 entries
    assert ln[i] >= 3 * 4096 and (rp[i + 1] - 1 - bases[g]) // 4096 - (rp[i] - bases[g]) // 4096 + 1 >= 3
    # rows of 1, 2 and 3 entries whose first entry is the last one before a boundary
    rel = rp[:-1] + 1 - bases[wave_of_row(a)]
    for short in (1, 2, 3):
        assert ((ln == short) & (rel > 0) & (rel % w == 0)).any(), short
    # exactly W and W + 1 entries from residue 3
    for exact in (w, w + 1):
        assert ((ln == exact) & (rp[:-1] % 4 == 3)).any(), exact
    assert a.nrows % E.TILE != 0 and ln[-1] > 0


def test_one_row_of_four():
    a = E.one_row_of_four()
    ln = E.row_lengths(a)
    i = np.arange(a.nrows)
    for r in range(4):
        wrong = np.concatenate([[0], np.cumsum((ln > 0) != (i % 4 == r))])
        starts = np.flatnonzero(wrong[WAVE:] - wrong[:-WAVE] == 0)
        assert len(starts) > 0, r
        s = int(starts[0])
        live = ln[s:s + WAVE][ln[s:s + WAVE] > 0]
        assert set(live.tolist()) == set(range(1, 10))
        assert np.array_equal(np.diff(live) % 9, np.ones(len(live) - 1))              # they cycle


def test_holes_and_empty_operators():
    a = E.holes()
    ln = E.row_lengths(a)
    assert a.nrows == 4 * 1024 + 300
    empty = np.zeros(a.nrows, dtype=bool)
    empty[256:512] = empty[2048:3072] = empty[0] = empty[-1] = True
    assert np.array_equal(ln == 0, empty) and ln.max() <= 8
    runs = E.wave_runs(a.row_ptr)
    assert runs[1, 0] == runs[1, 1] and (runs[8:12, 0] == runs[8:12, 1]).all() and (np.delete(runs[:, 1] - runs[:, 0], [1, 8, 9, 10, 11]) > 0).all()
    z = E.all_empty()
    assert (z.nrows, z.nnz) == (1500, 0)


def test_partial_last_quad_and_last_column():
    for residue in (1, 2, 3):
        a = E.partial_last_quad(residue)
        assert a.nnz % 4 == residue and E.row_lengths(a)[-1] > 0
    s = E.single_entry()
    assert (s.nrows, s.ncols, s.nnz) == (1, 1, 1)
    for ncols in (1, 1023, 1025):
        a = E.last_column(ncols)
        assert a.ncols == ncols and (E.row_lengths(a) > 0).all()
        assert (a.col_idx[a.row_ptr[:-1]] == 0).all() and (a.col_idx[a.row_ptr[1:] - 1] == ncols - 1).all()
    assert E.row_lengths(E.last_column(1025)).max() > 2


def triplets(a):
    rows = np.repeat(np.arange(a.nrows), E.row_lengths(a))
    return rows, a.col_idx, a.vals


def assert_spd_by_dominance(a):
    rows, cols, vals = triplets(a)
    order = np.lexsort((rows, cols))                                                     # the transpose, in row-major order
    assert np.array_equal(cols[order], rows) and np.array_equal(rows[order], cols) and np.array_equal(vals[order], vals)
    off = rows != cols
    diag = np.zeros(a.nrows)
    diag[rows[~off]] = vals[~off]
    assert (~off).sum() == a.nrows and (diag > np.bincount(rows[off], np.abs(vals[off]), a.nrows)).all()
    assert np.abs(vals[off]).max() <= 1.1 + 1e-12


def converges(a):
    b = R.store(MC.rhs(a.nrows))
    ref = R.cg32(R.Lowered(a), b, np.zeros(a.nrows, np.float32), 1e-5, 400)
    assert ref.code == R.OK and ref.converged and 5 < ref.iterations < 400, (ref.code, ref.iterations)
    return ref.iterations


def test_arrow3000():
    a = E.arrow3000()
    assert_spd_by_dominance(a)
    ln = E.row_lengths(a)
    assert a.nrows == 3000 and ln[0] == 3000 and ln[1:].max() <= 25 and ln[1:].min() >= 2
    run0 = E.wave_runs(a.row_ptr)[0]
    assert run0[1] - run0[0] > max(E.WINDOWS)                                            # (the row alone: two windows of 2048, six of 512)
    assert converges(a) < 100


def test_dense_rows_across_a_tile():
    a = E.dense_rows_across_a_tile()
    assert_spd_by_dominance(a)
    ln = E.row_lengths(a)
    assert a.nrows == 2500 and E.DENSE_ROWS[0] < 1024 <= E.DENSE_ROWS[-1]
    assert (ln[E.DENSE_ROWS] > 650).all() and (ln[E.DENSE_ROWS] < 760).all() and np.delete(ln, E.DENSE_ROWS).max() < 40
    runs = E.wave_runs(a.row_ptr)
    assert runs[3, 1] - runs[3, 0] > max(E.WINDOWS) and runs[4, 1] - runs[4, 0] > max(E.WINDOWS)
    converges(a)


@pytest.mark.parametrize("n", [1023, 1024, 1025, E.BIG_BAND_ROWS])
def test_thinned_band(n):
    a = E.thinned_band(n)
    assert a.nrows == n
    assert_spd_by_dominance(a)
    rows, cols, _ = triplets(a)
    assert set(np.unique(np.abs(rows - cols)).tolist()) == {0, *E.BAND_OFFSETS}
    ln = E.row_lengths(a)
    assert len(np.unique(ln)) >= 6 and np.count_nonzero(np.diff(ln)) > n // 2           # the lengths vary from row to row
    tiles = np.add.reduceat(ln, np.arange(0, n, E.TILE))
    assert n < 2048 or len(np.unique(tiles[:-1])) > len(tiles) // 4                     # ... and so do the tiles
    converges(a)
    if n == E.BIG_BAND_ROWS:
        assert len(tiles) == 264 > 256


# ---- the ends of the fp32 range (tests/test_gpu_mixed_edges.py, part d)
def watch_range(e):
    a = MC.poisson12()
    n = a.nrows
    b = R.store(MC.rhs(n) * 2.0 ** e)
    seen = []
    ref = R.cg32(R.Lowered(a), b, np.zeros(n, np.float32), 1e-30, E.RANGE_CAP, watch=lambda i, ap, x, r, p: seen.append((i, ap.copy(), x.copy(), r.copy(), p.copy())))
    return n, b, ref, seen


def subnormal(v):
    return int(np.count_nonzero((v != 0) & (np.abs(v) < R.TINY32)))


def test_range_subnormal():
    n, b, ref, seen = watch_range(E.RANGE_EXPONENTS["subnormal"])
    assert ref.code == R.OK and ref.iterations == E.RANGE_CAP and len(seen) == E.RANGE_CAP
    assert subnormal(b) > n // 2
    for i, ap, x, r, p in seen:
        assert min(subnormal(r), subnormal(p), subnormal(x)) > n // 2, (i, subnormal(r), subnormal(p), subnormal(x))
    assert ref.history[-1] < ref.history[0]


def test_range_flushing():
    e = E.RANGE_EXPONENTS["flushing"]
    n, b, ref, seen = watch_range(e)
    flushed = int(np.count_nonzero((MC.rhs(n) != 0) & (b == 0)))
    assert flushed >= 1 and subnormal(b) == n - flushed
    assert ref.code == R.OK and ref.iterations == E.RANGE_CAP
    assert ref.history[-1] < ref.history[0]                                              # the relative residual still falls


def test_range_overflow():
    n, b, ref, seen = watch_range(E.RANGE_EXPONENTS["overflow"])
    assert np.isfinite(b).all()
    first_ap = seen[0][1]
    assert np.isinf(first_ap).sum() >= 1 and not np.isnan(first_ap).any()
    # the iteration of the overflow: p.Ap = +inf, alpha = 0, and 0 * inf makes r NaN where Ap overflowed; (r, r) is NaN from there, so is
    # beta, and every vector of every later iteration is NaN in every element
    assert np.array_equal(np.isnan(seen[0][3]), np.isinf(first_ap))
    for i, ap, x, r, p in seen[1:]:
        assert np.isnan(r).all() and np.isnan(p).all() and np.isnan(x).all(), i
    assert (ref.code, ref.iterations, ref.converged) == (R.OK, E.RANGE_CAP, True)        # the cap reports converged (convergence.rs:18-34)
    assert np.isnan(ref.x).all() and np.isnan(ref.history[1:]).all()


def test_range_control():
    n, b, ref, seen = watch_range(E.RANGE_EXPONENTS["control"])
    assert subnormal(b) == 0 and (b != 0).all() and np.isfinite(b).all()
    for i, ap, x, r, p in seen:
        for v in (ap, x, r, p):
            assert np.isfinite(v).all() and subnormal(v) == 0
    assert ref.code == R.OK and ref.iterations == E.RANGE_CAP
