"""Operators of arbitrary length for the multi-chunk fold tests (tests/test_gpu_chunked_folds.py, tests/test_chunked_folds_cpu.py).

A 2-D 5-point operator on lines of M = 724 rows (not a multiple of the 512-row tile), cut to n rows: row i couples to i +- 1 inside its
line (i // M equal) and to i +- M where that column lies in [0, n); diagonal d + 0.01 u_i with u = splitmix64_uniform(seed, n),
off-diagonals -1 + c above the diagonal and -1 - c below it.  c = 0 is a principal submatrix of an SPD matrix (d = 4: the diagonal
dominates weakly), so SPD for every n."""
import numpy as np

from oracle import oracle as O

M = 724
SEED = 0xC4A7

# name: (n, tiles, chunks) with tiles of 512 rows and chunks of 1024 tiles (the library's fold, kryst_reduce_spec)
SIZES = {
    "A": (524288, 1024, 1),              # one full chunk: the last size without stage 2 of the fold
    "B": (524289, 1025, 2),              # the second chunk is one tile of one row
    "C": (1572900, 3073, 4),             # the last chunk is one tile of 36 rows
    "S": (96 ** 3, 1728, 2),             # stencil7(96): device-generated operator
}

VARIANTS = {                             # (c, d)
    "sym": (0.0, 4.0),
    "nonsym": (0.3, 4.0),
    "dom_sym": (0.0, 6.0),
    "dom_nonsym": (0.3, 6.0),
}


def tiles_and_chunks(n, T=256, V=2, F=1024):
    tiles = -(-n // (T * V))
    return tiles, (-(-tiles // F) if tiles > F else 1)


def five_point(n, c, d, m=M, seed=SEED):
    """The operator above as an oracle.Csr (rows in ascending column order)."""
    i = np.arange(n, dtype=np.int64)
    cols = i[:, None] + np.array([-m, -1, 0, 1, m], dtype=np.int64)[None, :]
    valid = np.stack([i >= m, i % m != 0, np.ones(n, bool), ((i + 1) % m != 0) & (i + 1 < n), i + m < n], axis=1)
    lo, up = -1.0 - c, -1.0 + c
    vals = np.empty((n, 5))
    vals[:, 0] = lo; vals[:, 1] = lo; vals[:, 3] = up; vals[:, 4] = up
    vals[:, 2] = d + 0.01 * O.splitmix64_uniform(seed, n)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(valid.sum(axis=1), out=rp[1:])
    return O.Csr(n, n, rp, cols[valid], vals[valid])


def variant(n, name):
    c, d = VARIANTS[name]
    return five_point(n, c, d)


def rhs(n):
    return O.splitmix64_uniform(0xB0B, n) - 0.25
