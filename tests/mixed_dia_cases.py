"""Operators and vectors of the fp32 diagonal (CSR-DIA) tests, described on the host.  tests/test_mixed_dia_cpu.py asserts that each has the
property it is there for; tests/test_gpu_mixed_dia.py runs the library on them against tests/mixed_ref.py, bit for bit.

The form: one value stream per distinct (col - row) offset, in ascending offset order (the stored order of rows with ascending columns); an entry
a row does not store is ABSENT (a NaN payload).  The library builds it when D <= 32 and D * nrows <= 1.125 * nnz + 64 (csr_create.hip: build_dia).
The fp32 tile is 1024 rows, lane t owns rows 4t .. 4t+3, and a vector of n elements has ceil(n / 1024) * 1024 + 1024 allocated floats."""
import numpy as np

from oracle import oracle as O
import mixed_pattern_cases as P
import mixed_ref as R

TILE32 = 1024
DIA_MAX = 32
ABSENT64 = np.uint64(0x7FF8D1A0D1A0D1A0)            # KR_DIA_ABSENT: "no entry here" in an fp64 stream
ABSENT32 = np.uint32(0x7FD1A0D1)                    # KRYST_CSR32_DIA_ABSENT_BITS
# a stored double NaN whose (float) has the marker's bits: the top 23 payload bits are the marker's (quiet and signalling twin)
MARKER_TWINS = (np.uint64(0x7FFA341A20000000), np.uint64(0x7FF2341A20000001))


def xcap(ncols):
    return -(-ncols // TILE32) * TILE32 + TILE32


def _distinct(n, k, seed):
    """n x k values of both signs in 1 <= |v| < 2, all distinct (and still distinct once rounded to fp32: they are more than 2^-23 apart)"""
    rng = np.random.default_rng(seed)
    v = (1.0 + np.arange(n * k) / (n * k + 1.0) + rng.uniform(0.0, 1e-7, n * k)) * np.where(rng.random(n * k) < 0.5, -1.0, 1.0)
    assert len(np.unique(v)) == n * k
    return rng.permutation(v).reshape(n, k)


def band(nrows, ncols, offsets, seed=3):
    """every row stores the entries of `offsets` (ascending) that lie in [0, ncols); all values distinct"""
    offsets = np.array(sorted(offsets), dtype=np.int64)
    idx = np.arange(nrows)
    cols = idx[:, None] + offsets[None, :]
    return P._csr(nrows, ncols, cols, _distinct(nrows, len(offsets), seed), (cols >= 0) & (cols < ncols))


def tridiag(n):
    return band(n, n, (-1, 0, 1), seed=n)


def tridiag_spd(n):
    """symmetric, strictly diagonally dominant, a distinct weight on every edge: the tridiagonal operator of the solver tests"""
    w = 0.5 + np.random.default_rng(n).random(n + 1)
    idx = np.arange(n)
    cols = idx[:, None] + np.array([-1, 0, 1])[None, :]
    vals = np.stack([-w[idx], w[idx] + w[idx + 1] + 0.25, -w[idx + 1]], axis=1)
    return P._csr(n, n, cols, vals, (cols >= 0) & (cols < n))


def varbox(nx, ny, nz, seed=17):
    """variable-coefficient diffusion on an nx x ny x nz box (x fastest): edge (r, r + stride) has weight 0.5 + U, off-diagonals are -w, the
    diagonal is the sum of the six incident weights with 1.0 for a neighbour outside the box.  SPD, 7 diagonals, no two rows alike."""
    n = nx * ny * nz
    w = 0.5 + np.random.default_rng(seed).random((3, n))                 # w[d][r]: edge (r, r + strides[d])
    idx = np.arange(n)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    strides = (1, nx, nx * ny)
    lo = (i > 0, j > 0, k > 0)
    hi = (i + 1 < nx, j + 1 < ny, k + 1 < nz)
    wlo = [np.where(lo[d], w[d][np.maximum(idx - strides[d], 0)], 1.0) for d in range(3)]
    whi = [np.where(hi[d], w[d], 1.0) for d in range(3)]
    diag = wlo[0] + whi[0] + wlo[1] + whi[1] + wlo[2] + whi[2]
    offs = np.array([-strides[2], -strides[1], -1, 0, 1, strides[1], strides[2]])
    vals = np.stack([-wlo[2], -wlo[1], -wlo[0], diag, -whi[0], -whi[1], -whi[2]], axis=1)
    keep = np.stack([lo[2], lo[1], lo[0], np.ones(n, dtype=bool), hi[0], hi[1], hi[2]], axis=1)
    return P._csr(n, n, idx[:, None] + offs[None, :], vals, keep)


TAPS9 = [(di, dj, 0, 8.5 if (di, dj) == (0, 0) else -1.0 / (1 + abs(di) + abs(dj))) for dj in (-1, 0, 1) for di in (-1, 0, 1)]
FAR_OFFSETS, FAR_ROWS = (-2000, 0, 2000), 16000
TRIDIAG_HOLES = [0, 5, 6, 514, 1023, 1024]
VARCOEF_HOLES = [0, 3, 143, 144, 1023, 1024, 1727]
SPECIAL_VALUES = {7: -0.0, 100: np.inf, 1501: np.nan, 2000: 1e-40, 2500: -1e-50, 3000: 2.0 ** -140, 30: 1.0 + 2.0 ** -30}


def special_values():
    """stored -0.0, +inf and an ordinary NaN, values that become fp32-subnormal (1e-40, 2^-140) or zero (1e-50), one that rounds to 1.0"""
    return P.with_values(tridiag(1025), SPECIAL_VALUES)


def marker_twin(which):
    """a stored NaN whose rounding to fp32 has the absent marker's bits"""
    return P.with_values(tridiag(1025), {1501: np.array([MARKER_TWINS[which]]).view(np.float64)[0]})


def refusal_band():
    """the 2000-row band of tests/test_gpu_mixed_pattern.py::test_refusals: 2000 distinct rows, offsets (-9, -4, 0, 3, 8), a few entries left out"""
    rng = np.random.default_rng(31)
    n = 2000
    cols = np.clip(np.arange(n)[:, None] + np.array([-9, -4, 0, 3, 8])[None, :], 0, n - 1)
    keep = np.ones((n, 5), dtype=bool); keep[:9, :2] = False; keep[-8:, 3:] = False
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    return O.Csr(n, n, rp, cols[keep], rng.standard_normal(int(rp[-1])))


def sparse_diagonals():
    """the same five offsets, the four outer ones stored in every second row only: 5 * 2000 > 1.125 * nnz + 64, so no diagonal form is built"""
    a = band(2000, 2000, (-9, -4, 0, 3, 8), seed=5)
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    keep = (rows % 2 == 0) | (a.col_idx == rows)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=a.nrows))]).astype(np.int64)
    return O.Csr(a.nrows, a.ncols, rp, a.col_idx[keep], a.vals[keep])


def nonsquare():
    """1300 x 1400, every row the same three offsets, none clipped"""
    return band(1300, 1400, (0, 37, 100), seed=9)


# name -> constructor.  Every one satisfies the fill rule (tests/test_mixed_dia_cpu.py)
OPERATORS = {
    "tridiag1": lambda: tridiag(1), "tridiag3": lambda: tridiag(3), "tridiag1023": lambda: tridiag(1023), "tridiag1024": lambda: tridiag(1024),
    "tridiag1025": lambda: tridiag(1025), "tridiag2049": lambda: tridiag(2049),
    "five_point": lambda: P.box(16, 16, 1, P.TAPS5),
    "nine_point": lambda: P.box(16, 16, 1, TAPS9),
    "varcoef12": lambda: O.stencil7(12, "varcoef"),
    "varbox16x16x20": lambda: varbox(16, 16, 20),
    "band11": lambda: band(2049, 2049, range(-5, 6)),
    "band2": lambda: band(1500, 1500, (0, 3)), "band4": lambda: band(1500, 1500, (-2, 0, 1, 5)),
    "band6": lambda: band(1500, 1500, (-7, -2, -1, 0, 1, 2)), "band8": lambda: band(1500, 1500, (-9, -4, -1, 0, 1, 2, 6, 11)),
    "box27": lambda: P.box(20, 20, 20, P.TAPS27),
    "far": lambda: band(FAR_ROWS, FAR_ROWS, FAR_OFFSETS),
    "nonsquare": nonsquare,
    "special_values": special_values,
    "tridiag_holes": lambda: P.drop_columns(tridiag(1025), TRIDIAG_HOLES),
    "varcoef12_holes": lambda: P.drop_columns(O.stencil7(12, "varcoef"), VARCOEF_HOLES),
}
# D of each
DIAGONALS = {"tridiag1": 1, "tridiag3": 3, "tridiag1023": 3, "tridiag1024": 3, "tridiag1025": 3, "tridiag2049": 3, "five_point": 5, "nine_point": 9,
             "varcoef12": 7, "varbox16x16x20": 7, "band11": 11, "band2": 2, "band4": 4, "band6": 6, "band8": 8, "box27": 27, "far": 3,
             "nonsquare": 3, "special_values": 3, "tridiag_holes": 3, "varcoef12_holes": 7}
SOLVE_OPERATORS = {"varcoef12": lambda: O.stencil7(12, "varcoef"), "varbox16x16x20": lambda: varbox(16, 16, 20),
                   "tridiag_spd1023": lambda: tridiag_spd(1023), "tridiag_spd1024": lambda: tridiag_spd(1024), "tridiag_spd1025": lambda: tridiag_spd(1025)}
SETTINGS = {"default": ({}, "dia"), "plain": ({"KRYST_SPMV32_FORM": "plain"}, "plain"), "word": ({"KRYST_SPMV32_FORM": "dia"}, "dia")}


# ---- host description of the diagonal form ----
def offsets(a):
    """the distinct (col - row) offsets, ascending: the diagonals in stored order"""
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    return np.unique(a.col_idx - rows)


def dia_min_max(a):
    offs = offsets(a)
    return min(0, int(offs.min())), max(0, int(offs.max()))


def fill_rule(a):
    """-> (D * nrows, 1.125 * nnz + 64)"""
    return len(offsets(a)) * a.nrows, 1.125 * len(a.vals) + 64.0


def streams64(a):
    """D x nrows uint64: the bits of the fp64 streams, ABSENT64 where a row does not store the diagonal"""
    offs = offsets(a)
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    out = np.full((len(offs), a.nrows), ABSENT64, dtype=np.uint64)
    out[np.searchsorted(offs, a.col_idx - rows), rows] = np.ascontiguousarray(a.vals, dtype=np.float64).view(np.uint64)
    return out


def streams32(a):
    """the lowered streams, entry by entry: an absent entry becomes the fp32 marker, every other (float)v.
    -> (D x nrows uint32, the number of present entries that round onto the marker)"""
    s64 = streams64(a)
    present = s64 != ABSENT64
    s32 = R.store(s64.view(np.float64)).view(np.uint32).copy()
    refused = int(np.count_nonzero(present & (s32 == ABSENT32)))
    s32[~present] = ABSENT32
    return s32, refused


def clamped_tiles(a):
    """the 1024-row tiles whose lowest diagonal would start before x[0]: they take the per-element path"""
    lo = dia_min_max(a)[0]
    return [q for q in range(-(-a.nrows // TILE32)) if q * TILE32 + lo < 0]


def rows_pointing_beyond(a):
    """rows with an (absent) entry whose column lies at or beyond the allocation of x"""
    idx = np.arange(a.nrows)
    return idx[idx + dia_min_max(a)[1] >= xcap(a.ncols)]


def unread_elements(a):
    """elements of x that no stored entry reads"""
    return np.setdiff1d(np.arange(a.ncols), a.col_idx)


def poison_at(n, where, seed=21):
    return P.poison_at(n, where, seed)
