"""The operators of tests/test_gpu_chunked_folds.py checked on the host: what the 5-point helper builds, and that the sizes there span the
tile and chunk counts they are chosen for (tiles of T * V = 512 rows, chunks of F = 1024 tiles: O.Reduce.tiled's defaults, which are the
library's kryst_reduce_spec)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
import chunked_cases as CC


def _scipy(a):
    return sp.csr_matrix((a.vals, a.col_idx, a.row_ptr), shape=(a.nrows, a.ncols))


@pytest.mark.parametrize("n", [1, 723, 724, 725, 1449, 5000, CC.SIZES["B"][0]])
def test_five_point_structure(n):
    m = CC.M
    for name, (c, d) in CC.VARIANTS.items():
        a = CC.variant(n, name)
        rp, ci = a.row_ptr, a.col_idx
        # every row in strictly ascending column order, columns in range
        rows = np.repeat(np.arange(n), np.diff(rp))
        starts = np.zeros(a.nnz, bool); starts[rp[:-1][np.diff(rp) > 0]] = True
        assert np.all((np.diff(ci) > 0) | starts[1:]), name
        assert ci.min() >= 0 and ci.max() < n
        # the couplings: i +- 1 inside the line, i +- m inside [0, n), nothing else; the values
        off = ci - rows
        assert set(np.unique(off).tolist()) <= {-m, -1, 0, 1, m}
        assert np.all(rows[off == 1] // m == (rows[off == 1] + 1) // m) and np.all(rows[off == -1] // m == (rows[off == -1] - 1) // m)
        i = np.arange(n)
        want = 1 + (i >= m) + (i + m < n) + (i % m != 0) + (((i + 1) % m != 0) & (i + 1 < n))
        assert np.array_equal(np.diff(rp), want), name
        assert np.array_equal(a.vals[off == 0], d + 0.01 * O.splitmix64_uniform(CC.SEED, n))
        assert np.all(a.vals[off < 0] == -1.0 - c) and np.all(a.vals[off > 0] == -1.0 + c)
        if c == 0.0:
            s = _scipy(a)
            assert (s != s.T).nnz == 0, name


def test_five_point_symmetric_variant_is_positive_definite_at_a_small_size():
    a = _scipy(CC.variant(3 * CC.M + 17, "sym")).toarray()
    assert np.linalg.eigvalsh(a).min() > 0.0


@pytest.mark.parametrize("name", ["A", "B", "C", "S"])
def test_sizes_span_the_tile_and_chunk_counts(name):
    n, tiles, chunks = CC.SIZES[name]
    rs = O.Reduce.tiled()
    T, V, F = rs.c.T, rs.c.V, rs.c.F
    assert (T * V, F) == (512, 1024)
    assert CC.tiles_and_chunks(n, T, V, F) == (tiles, chunks)
    if name != "S":
        a = CC.variant(n, "sym")
        assert a.nrows == n and len(a.row_ptr) - 1 == n
        # the tail: A fills its one chunk exactly, B's second chunk is one tile of one row, C's last chunk one tile of 36 rows
        last_tile_rows = n - (tiles - 1) * T * V
        tiles_in_last_chunk = tiles - (chunks - 1) * F
        assert (last_tile_rows, tiles_in_last_chunk) == {"A": (512, 1024), "B": (1, 1), "C": (36, 1)}[name]
