"""Operators and vectors of the fp32 row-pattern (CSR-P16) tests, described on the host.  tests/test_mixed_pattern_cpu.py asserts that each
has the property it is there for; tests/test_gpu_mixed_pattern.py runs the library on them against tests/mixed_ref.py, bit for bit.

The fp32 tile is 1024 rows and lane t owns rows 4t .. 4t+3 (a "quad"); a row's BASE is the longest row whose (col - row, value) sequence
contains its own, and a quad whose rows share a base is served by one 16-byte gather per entry."""
import numpy as np

from oracle import oracle as O

QUAD, TILE32 = 4, 1024


def _csr(nrows, ncols, cols, vals, keep):
    """rows of a fixed candidate list: cols / vals are nrows x k, keep says which candidates exist (stored order = candidate order)"""
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return O.Csr(nrows, ncols, rp, cols[keep].astype(np.int64), np.ascontiguousarray(vals[keep], dtype=np.float64))


def box(nx, ny, nz, taps):
    """taps: (di, dj, dk, value), x fastest; a tap exists where the neighbour lies in the box.  Stored in ascending column order."""
    n = nx * ny * nz
    idx = np.arange(n)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    taps = sorted(taps, key=lambda t: t[0] + nx * (t[1] + ny * t[2]))
    cols = np.stack([idx + t[0] + nx * (t[1] + ny * t[2]) for t in taps], axis=1)
    keep = np.stack([(i + t[0] >= 0) & (i + t[0] < nx) & (j + t[1] >= 0) & (j + t[1] < ny) & (k + t[2] >= 0) & (k + t[2] < nz) for t in taps], axis=1)
    vals = np.tile(np.array([t[3] for t in taps], dtype=np.float64), (n, 1))
    return _csr(n, n, cols, vals, keep)


TAPS7 = [(0, 0, -1, -1.0), (0, -1, 0, -1.0), (-1, 0, 0, -1.0), (0, 0, 0, 6.0), (1, 0, 0, -1.0), (0, 1, 0, -1.0), (0, 0, 1, -1.0)]
TAPS5 = [(0, -1, 0, -1.0), (-1, 0, 0, -1.0), (0, 0, 0, 4.0), (1, 0, 0, -1.0), (0, 1, 0, -1.0)]
TAPS27 = [(di, dj, dk, 26.5 if (di, dj, dk) == (0, 0, 0) else -1.0 / (1 + abs(di) + abs(dj) + abs(dk)))
          for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)]


def poisson(nx, ny=None, nz=None):
    return box(nx, ny or nx, nz or nx, TAPS7)


def banded(nrows, ncols, row_kinds, period):
    """row i takes row_kinds[i % period]: a list of (col - row, value); an entry exists where its column lies in [0, ncols)"""
    k = max(len(r) for r in row_kinds)
    cols = np.zeros((nrows, k), dtype=np.int64); vals = np.zeros((nrows, k)); keep = np.zeros((nrows, k), dtype=bool)
    idx = np.arange(nrows)
    for kind, entries in enumerate(row_kinds):
        rows = idx[idx % period == kind]
        for e, (off, v) in enumerate(entries):
            cols[rows, e] = rows + off; vals[rows, e] = v
            keep[rows, e] = (rows + off >= 0) & (rows + off < ncols)
    return _csr(nrows, ncols, cols, vals, keep)


def tridiag(n):
    return banded(n, n, [[(-1, -1.0), (0, 2.5), (1, -1.0)]], 1)


def long_row():
    """one 40-entry row repeated 1500 times (non-square, so that no row is clipped): a base longer than 16 entries, 5 trips of the entry loop"""
    return banded(1500, 1500 + 117, [[(3 * j, (-1.0) ** j * (1.0 + j / 7.0)) for j in range(40)]], 1)


def period2():
    """even rows (-7, 0, 7), odd rows (-2, -1, 0, 1, 2): no quad shares a base"""
    return banded(2050, 2050, [[(-7, -1.0), (0, 4.0), (7, -1.25)], [(-2, 0.5), (-1, -1.5), (0, 5.0), (1, -1.75), (2, 0.25)]], 2)


def period3():
    """SPD, three unrelated rows in turn: (i, i + 3) coupled with a weight that depends on i % 3, (i, i + 1) coupled where i % 3 == 0.  A quad
    starts at every phase of the period."""
    w, u = (-1.0, -0.75, -0.5), -0.625
    return banded(2051, 2051, [[(-3, w[0]), (0, 4.0), (1, u), (3, w[0])], [(-3, w[1]), (-1, u), (0, 5.0), (3, w[1])], [(-3, w[2]), (0, 6.0), (3, w[2])]], 3)


def empty_rows():
    """a tridiagonal operator whose every fifth row stores nothing"""
    a = banded(1030, 1030, [[(-1, -1.0), (0, 2.5), (1, -1.0)]] * 4 + [[]], 5)
    assert (np.diff(a.row_ptr) == 0).sum() == 206
    return a


def wide():
    """1300 x 1400, every row the same three entries"""
    return banded(1300, 1400, [[(0, 1.5), (37, -0.5), (100, 0.25)]], 1)


def tall():
    """1500 x 1300, more rows than x has elements: the first 100 rows are empty, the next 100 and the last 100 clipped"""
    return banded(1500, 1300, [[(-200, 1.0), (-150, -2.0), (-100, 0.5)]], 1)


def with_values(a, changes):
    vals = a.vals.copy()
    for k, v in changes.items():
        vals[k] = v
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, vals, check=False)


SPECIAL_VALUES = {7: -0.0, 100: np.inf, 1501: np.nan, 2000: 1e-40, 2500: -1e-50, 3000: 2.0 ** -140, 30: 1.0 + 2.0 ** -30}


def special_values():
    """stored -0.0, +inf and NaN, values that become fp32-subnormal (1e-40, 2^-140) or zero (1e-50), one that rounds to 1.0"""
    return with_values(tridiag(1025), SPECIAL_VALUES)


def twins():
    """rows 3q store 1.0 off the diagonal, the others 1 + 2^-30: two fp64 patterns that are ONE row once rounded to fp32"""
    e = 1.0 + 2.0 ** -30
    return banded(1100, 1100, [[(-1, 1.0), (0, 3.0), (1, 1.0)], [(-1, e), (0, 3.0), (1, e)], [(-1, e), (0, 3.0), (1, e)]], 3)


def drop_columns(a, cols, keep_diagonal=False):
    """`a` without every entry that lies in one of `cols`: nothing reads those elements of x any more (keep_diagonal: nothing but the row
    of the same number -- the staged kernel takes operators whose every row stores its diagonal)"""
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    keep = ~np.isin(a.col_idx, cols) | (keep_diagonal & (rows == a.col_idx))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=a.nrows))]).astype(np.int64)
    return O.Csr(a.nrows, a.ncols, rp, a.col_idx[keep], a.vals[keep])


TRIDIAG_HOLES = [0, 5, 6, 514, 1023, 1024]
POISSON_HOLES = [0, 3, 16, 255, 256, 1023, 1024, 2050, 4092, 4095]


def tridiag_holes():
    return drop_columns(tridiag(1025), TRIDIAG_HOLES)


def poisson16_holes():
    return drop_columns(poisson(16), POISSON_HOLES, keep_diagonal=True)


def poison_at(n, holes, seed=21):
    """three fp32 vectors with NaN / +inf / -inf exactly at `holes`"""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
        x[holes] = bad
        out.append(x)
    return out


# name -> (constructor, the kernel its pattern lowering must report by default)
OPERATORS = {
    "poisson16": (lambda: poisson(16), "pattern-stage"),                       # n = 16: staged; 4 fp32 tiles
    "poisson12": (lambda: poisson(12), "pattern-stage"),                       # staged; the last tile is partial
    "poisson18": (lambda: poisson(18), "pattern"),                             # n % 4 = 2
    "box16x16x20": (lambda: poisson(16, 16, 20), "pattern-stage"),
    "tridiag1": (lambda: tridiag(1), "pattern"), "tridiag3": (lambda: tridiag(3), "pattern"), "tridiag1023": (lambda: tridiag(1023), "pattern"),
    "tridiag1024": (lambda: tridiag(1024), "pattern"), "tridiag1025": (lambda: tridiag(1025), "pattern"), "tridiag2049": (lambda: tridiag(2049), "pattern"),
    "five_point": (lambda: box(24, 45, 1, TAPS5), "pattern"),
    "box27": (lambda: box(10, 10, 10, TAPS27), "pattern"),
    "long_row": (long_row, "pattern"),
    "period2": (period2, "pattern"), "period3": (period3, "pattern"),
    "empty_rows": (empty_rows, "pattern"),
    "wide": (wide, "pattern"), "tall": (tall, "pattern"),
    "special_values": (special_values, "pattern"),
    "twins": (twins, "pattern"),
    "tridiag_holes": (tridiag_holes, "pattern"), "poisson16_holes": (poisson16_holes, "pattern-stage"),
}
SOLVE_OPERATORS = ["poisson16", "poisson18", "period3"]
SETTINGS = {"default": {}, "stage0": {"KRYST_SPMV32_STAGE": "0"}, "plain": {"KRYST_SPMV32_FORM": "plain"}}


def expected_kernel(default, setting):
    if setting == "plain":
        return "plain"
    return "pattern" if setting == "stage0" else default


# ---- host description of the row-pattern form ----
def distinct_rows(a):
    """-> (list of distinct rows as tuples of (col - row, value bits), id per row)"""
    seen, ids = {}, np.empty(a.nrows, dtype=np.int64)
    bits = np.ascontiguousarray(a.vals, dtype=np.float64).view(np.uint64)
    for i in range(a.nrows):
        s, e = int(a.row_ptr[i]), int(a.row_ptr[i + 1])
        key = (tuple((a.col_idx[s:e] - i).tolist()), tuple(bits[s:e].tolist()))
        ids[i] = seen.setdefault(key, len(seen))
    rows = [list(zip(k[0], k[1])) for k in seen]
    return rows, ids


def _subsequence(short, long):
    it = iter(long)
    return all(any(x == y for y in it) for x in short)


def bases(rows):
    """the base of every distinct row, as the library assigns it: longest rows first, a row of at most 16 entries joins the first base of at
    most 16 entries that contains it as a sub-sequence"""
    order = sorted(range(len(rows)), key=lambda p: -len(rows[p]))
    found, base_of = [], {}
    for p in order:
        hit = None
        if len(rows[p]) <= 16:
            hit = next((b for b in found if len(rows[b]) <= 16 and len(rows[b]) >= len(rows[p]) and _subsequence(rows[p], rows[b])), None)
        if hit is None:
            found.append(p); hit = p
        base_of[p] = hit
    return base_of


def quads_sharing_a_base(a):
    """-> boolean per quad: the (existing) rows 4q .. 4q+3 have one base"""
    rows, ids = distinct_rows(a)
    base_of = bases(rows)
    b = np.array([base_of[int(p)] for p in ids])
    nq = -(-a.nrows // QUAD)
    return np.array([len(set(b[QUAD * q:QUAD * q + QUAD].tolist())) == 1 for q in range(nq)])


def line_length(a):
    """n when every base is (far, -n, -1, 0, +1, +n, far) with one n, else 0"""
    rows, _ = distinct_rows(a)
    base_of = bases(rows)
    n = set()
    for b in set(base_of.values()):
        offs = [o for o, _ in rows[b]]
        if len(offs) != 7 or offs[2:5] != [-1, 0, 1] or offs[1] != -offs[5]:
            return 0
        n.add(offs[5])
    return n.pop() if len(n) == 1 else 0
