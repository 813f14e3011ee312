"""Operators that put the fp32 SpMV's window logic on its edges, shared by the CPU tier (tests/test_mixed_edges_cpu.py: every property
named here is asserted there, on the generators alone) and the GPU tier (tests/test_gpu_mixed_edges.py: the library against
tests/mixed_ref.py, bit for bit).  Generators only, vectorised numpy.

The vocabulary.  A WAVE is a group of 256 consecutive rows aligned to 256 (four of them make a 1024-row tile); its RUN is the stretch
[k0, k1) of stored entries of its rows; the wave streams its run through a window of W entries that starts at k0 & ~3, so the window
BOUNDARIES of a wave are (k0 & ~3) + j W, j = 1, 2, ...  Every property is stated for every W in WINDOWS, not only the kernel's current
size."""
import numpy as np

from oracle import oracle as O

WINDOWS = (512, 1024, 2048, 4096)
WAVE, TILE = 256, 1024


def wave_runs(row_ptr):
    """-> int64 array (number of waves, 2): (k0, k1), the first and the past-the-last entry of every group of 256 rows"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    n = len(rp) - 1
    starts = np.arange(0, n, WAVE)
    return np.stack([rp[starts], rp[np.minimum(starts + WAVE, n)]], axis=1)


def wave_bases(row_ptr):
    """the window origin k0 & ~3 of every wave"""
    return wave_runs(row_ptr)[:, 0] & ~np.int64(3)


def row_lengths(a):
    return np.diff(a.row_ptr)


# ---- building blocks
def _values(rng, nnz):
    return rng.standard_normal(nnz) * np.exp(rng.uniform(-3, 3, nnz))


def _from_lengths(ncols, lengths, seed):
    """a general operator with the given row lengths: row i holds the columns o_i + k s_i, k < length, o_i and s_i random"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.min(initial=0) >= 0 and lengths.max(initial=0) <= ncols
    n = len(lengths)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    max_stride = np.maximum(1, (ncols - 1) // np.maximum(lengths - 1, 1))
    stride = rng.integers(1, max_stride + 1)
    offset = rng.integers(0, ncols - (np.maximum(lengths, 1) - 1) * stride)
    rows = np.repeat(np.arange(n), lengths)
    k = np.arange(rp[-1]) - rp[rows]
    ci = offset[rows] + k * stride[rows]
    return O.Csr(n, ncols, rp, ci, _values(rng, rp[-1]))


def _spread(rng, total, nrows, cuts=()):
    """`nrows` random row lengths that sum to `total`; every offset in `cuts` (0 < cut < total) is a row end that follows a non-empty row"""
    cuts = sorted(set(int(c) for c in cuts if 0 < c < total))
    free = rng.integers(0, total + 1, nrows - 1 - 2 * len(cuts))
    forced = [c for cut in cuts for c in (cut - 1 - int(rng.integers(0, min(cut, 6))), cut)]      # (an earlier end just below: the row is short)
    ends = np.sort(np.concatenate([free, np.array(forced, dtype=np.int64), [total]]))
    return np.diff(np.concatenate([[0], ends]))


# ---- general operators
EDGE_RUNS = sorted({r for w in WINDOWS for r in (w - 1, w, w + 1, 2 * w, 2 * w + 1)})


def runs_at_window_edges():
    """One wave per run length in EDGE_RUNS (W - 1, W, W + 1, 2 W, 2 W + 1 for every W), the waves' k0 at every residue of 4, and in every
    wave a non-empty row that ends exactly on each first boundary (k0 & ~3) + W inside its run."""
    rng = np.random.default_rng(101)
    order = [512, 511, 1023, 513, 2047, 1024, 1025, 4095, 2048, 2049, 4096, 4097, 8193, 8192]     # k0 % 4 = 0 0 3 2 3 2 2 3 2 2 3 3 0 1
    assert sorted(order) == EDGE_RUNS
    lengths, k0 = [], 0
    for run in order:
        lengths.append(_spread(rng, run, WAVE, [w - (k0 & 3) for w in WINDOWS]))
        k0 += run
    return _from_lengths(6000, np.concatenate(lengths), 102)


def straddlers():
    """Rows across window boundaries.  Wave 0: one row of 13 000 entries that crosses every boundary, of every W, inside its wave's run
    (it spans four windows of 4096 entries).  Wave 1: rows of 1, 2 and 3 entries whose first entry is the last one before the boundary
    (k0 & ~3) + j 4096, j = 1, 2, 3 -- a boundary of every W at once.  Waves 2 and 3: for every W a row of exactly W and one of exactly
    W + 1 entries, each starting at an entry index of residue 3.  77 more short rows end the matrix inside a tile."""
    rng = np.random.default_rng(111)
    # wave 0: short rows (fewer than 512 entries in all on either side), the long row in the middle
    head, tail = rng.integers(0, 3, 100), rng.integers(0, 3, 155)
    lengths = [head, [13000], tail]
    k = int(head.sum() + 13000 + tail.sum())
    # wave 1
    base = k & ~3
    marks, taken = [], []
    for j, ln in ((1, 1), (2, 2), (3, 3)):
        first = base + j * 4096 - 1 - k                      # offset of the short row's first entry within the wave's run
        marks += [first, first + ln]
        taken += list(range(first, first + ln + 1))          # (no other row may end at, or inside, the short row)
    total = 3 * 4096 + 700
    free = rng.choice(np.setdiff1d(np.arange(1, total), taken), WAVE - 1 - len(marks), replace=False)
    ends = np.sort(np.concatenate([free, marks, [total]]))
    lengths.append(np.diff(np.concatenate([[0], ends])))
    k += total
    # waves 2 and 3
    for group in (WINDOWS[:2], WINDOWS[2:]):
        part = []
        for w in group:
            for ln in (w, w + 1):
                pad = (3 - k) % 4 or 4                       # a short row in front moves the start to residue 3
                part += [pad, ln]
                k += pad + ln
        filler = rng.integers(0, 7, WAVE - len(part))
        k += int(filler.sum())
        lengths += [part, filler]
    lengths.append(rng.integers(0, 7, 77))
    lengths[-1][-1] = 3
    return _from_lengths(14000, np.concatenate([np.asarray(x, dtype=np.int64) for x in lengths]), 112)


def one_row_of_four():
    """Four stretches of 320 rows; in stretch r only the rows with i % 4 == r hold entries, their lengths cycling through 1..9"""
    n = 4 * 320
    i = np.arange(n)
    live = (i % 4) == (i // 320)
    lengths = np.zeros(n, dtype=np.int64)
    lengths[live] = np.arange(live.sum()) % 9 + 1
    return _from_lengths(2000, lengths, 121)


def holes():
    """4 x 1024 + 300 rows: the wave of rows 256..511 and the tile of rows 2048..3071 are empty, so are the first and the last row;
    every other row holds 1..8 entries"""
    n = 4 * TILE + 300
    lengths = np.random.default_rng(131).integers(1, 9, n)
    lengths[256:512] = 0
    lengths[2048:3072] = 0
    lengths[0] = lengths[-1] = 0
    return _from_lengths(5000, lengths, 132)


def all_empty():
    return O.Csr(1500, 1500, np.zeros(1501, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))


def partial_last_quad(residue):
    """nnz % 4 == residue (1, 2, 3) with a non-empty last row: the last 16-byte load of the stream reaches past nnz"""
    lengths = np.random.default_rng(140 + residue).integers(0, 8, 300)
    lengths[-1] = 1
    lengths[-1] += (residue - lengths.sum()) % 4
    return _from_lengths(400, lengths, 145 + residue)


def single_entry():
    return O.Csr(1, 1, [0, 1], [0], [1.5])


def last_column(ncols):
    """every row holds column 0 and column ncols - 1 (one entry when they are the same), and up to 5 columns between them"""
    rng = np.random.default_rng(150 + ncols)
    n = 700
    mid = rng.integers(0, 6, n) if ncols > 8 else np.zeros(n, dtype=np.int64)
    ends = 1 if ncols == 1 else 2
    lengths = mid + ends
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = np.repeat(np.arange(n), lengths)
    k = np.arange(rp[-1]) - rp[rows]
    # between the ends: distinct ascending columns 1 + k * stride + jitter-free offset
    stride = (ncols - 2) // 6 if ncols > 8 else 1
    ci = np.where(k == 0, 0, np.where(k == lengths[rows] - 1, ncols - 1, 1 + (k - 1) * stride + rng.integers(0, max(stride, 1), rp[-1])))
    return O.Csr(n, ncols, rp, ci, _values(rng, rp[-1]))


GENERAL_OPERATORS = {
    "runs_at_window_edges": runs_at_window_edges, "straddlers": straddlers, "one_row_of_four": one_row_of_four, "holes": holes,
    "all_empty": all_empty, "partial_last_quad1": lambda: partial_last_quad(1), "partial_last_quad2": lambda: partial_last_quad(2),
    "partial_last_quad3": lambda: partial_last_quad(3), "single_entry": single_entry, "last_column1": lambda: last_column(1),
    "last_column1023": lambda: last_column(1023), "last_column1025": lambda: last_column(1025),
}


# ---- symmetric positive definite operators: pattern B + B^T, values of order one, a strictly dominant diagonal
def _spd_from_pairs(n, lo, hi, off, diag_extra):
    """the symmetric operator with off-diagonal entries a[lo, hi] = a[hi, lo] = off (lo < hi, pairs distinct) and the diagonal
    row-sum of |off| + diag_extra"""
    assert (lo < hi).all()
    rowsum = np.bincount(lo, np.abs(off), n) + np.bincount(hi, np.abs(off), n)
    rows = np.concatenate([lo, hi, np.arange(n)])
    cols = np.concatenate([hi, lo, np.arange(n)])
    vals = np.concatenate([off, off, rowsum + diag_extra])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return O.Csr(n, n, rp, cols[order], vals[order], check=n < 100000)


def _distinct_pairs(n, i, j):
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    key = np.unique((lo * n + hi)[lo != hi])
    return key // n, key % n


def arrow3000():
    """row and column 0 dense (3000 entries: two windows of 2048, six of 512), about a dozen entries in every other row"""
    n = 3000
    rng = np.random.default_rng(161)
    i = np.repeat(np.arange(1, n), 5)
    lo, hi = _distinct_pairs(n, np.concatenate([np.zeros(n - 1, dtype=np.int64), i]), np.concatenate([np.arange(1, n), rng.integers(1, n, len(i))]))
    return _spd_from_pairs(n, lo, hi, rng.uniform(-1.0, 1.0, len(lo)), 1.0 + rng.uniform(0.0, 50.0, n))


DENSE_ROWS = np.arange(1019, 1031)


def dense_rows_across_a_tile():
    """n = 2500; rows and columns 1019..1030 hold about 700 entries each (820 draws with repeats): the run of the wave of rows 768..1023 is far beyond a window and
    the block lies across the tile boundary at row 1024"""
    n = 2500
    rng = np.random.default_rng(171)
    i = np.concatenate([np.repeat(DENSE_ROWS, 820), np.repeat(np.arange(n), 3)])
    j = np.concatenate([rng.integers(0, n, 820 * len(DENSE_ROWS)), rng.integers(0, n, 3 * n)])
    lo, hi = _distinct_pairs(n, i, j)
    return _spd_from_pairs(n, lo, hi, rng.uniform(-1.0, 1.0, len(lo)), 1.0 + rng.uniform(0.0, 1.0, n))


BAND_OFFSETS = (1, 2, 5, 37, 724)


def _mix(x):
    """splitmix64's finaliser on uint64"""
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def thinned_band(n):
    """offsets +-1, +-2, +-5, +-37, +-724; the pair (i, i + o) is kept (3 in 4) or dropped by a hash of i and o, so the row lengths vary
    from row to row; values in -(0.1 .. 1.1), the diagonal row-sum + 1 + a hash fraction.  Any n > 724."""
    assert n > max(BAND_OFFSETS)
    los, his, offs = [], [], []
    with np.errstate(over="ignore"):
        for t, o in enumerate(BAND_OFFSETS):
            i = np.arange(n - o, dtype=np.uint64)
            h = _mix(i * np.uint64(8) + np.uint64(t))
            keep = (h & np.uint64(3)) != 0
            los.append(i[keep].astype(np.int64))
            his.append(i[keep].astype(np.int64) + o)
            offs.append(-(0.1 + ((h[keep] >> np.uint64(8)) % np.uint64(1000)).astype(np.float64) / 1000.0))
        extra = 1.0 + (_mix(np.arange(n, dtype=np.uint64) * np.uint64(8) + np.uint64(7)) % np.uint64(1000)).astype(np.float64) / 1000.0
    return _spd_from_pairs(n, np.concatenate(los), np.concatenate(his), np.concatenate(offs), extra)


SPD_OPERATORS = {"arrow3000": arrow3000, "dense_rows_across_a_tile": dense_rows_across_a_tile, "thinned_band1023": lambda: thinned_band(1023),
                 "thinned_band1024": lambda: thinned_band(1024), "thinned_band1025": lambda: thinned_band(1025)}
BIG_BAND_ROWS = 270000


# ---- the ends of the fp32 range inside whole solves: poisson12, b = store(rhs * 2^e), x0 = 0, tolerance 1e-30, 12 iterations
RANGE_EXPONENTS = {"subnormal": -140, "flushing": -147, "overflow": 124, "control": 120}
RANGE_CAP = 12
