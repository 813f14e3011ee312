"""Which kernel an SpMV launch takes, pinned through the query hooks (spmv.h: tile_kernel / staged_form and the plans of spmv_fuse.hip).

Every storage form gives the same bits, so a slip in the choice passes every parity test and shows only as a speed loss at some size.  This
file asks the hooks the Python layer exposes -- encoding(), tile_order()["in_use"], pattern_info() and fuse_march_info() -- on the smallest
operators that reach every branch of the choice, under the defaults and under every setting the choice reads, one at a time (the settings
are read per launch, so one operator answers all of them).

EXPECTED is a literal: the answers of the commit BEFORE the choice was gathered into one place (when the form cascade was written out three
times and the staged-form condition five times), recorded on an MI355X and pasted here.  The code under test never generates its own
expectations; a change of a default or a threshold has to change this table by hand.
"""
import numpy as np
import pytest

import kryst_amd as K

pytestmark = pytest.mark.gpu

# (None: the defaults) -- applied one at a time
SETTINGS = [None] + [(k, v) for k, vs in (
    ("KRYST_SPMV_COMPRESS", "0123"), ("KRYST_SPMV_KERNEL", "3"), ("KRYST_SPMV_DIA", "02"), ("KRYST_SPMV_STAGE", "0"), ("KRYST_SPMV_STAGE_UFAR", "0"),
    ("KRYST_SPMV_ORDER", "02"), ("KRYST_CG_FUSE_P", "01"), ("KRYST_SPMV_FUSE_MARCH", "01"), ("KRYST_SPMV_FUSE_T", "24"), ("KRYST_CG_X_BATCH", "18"),
    ("KRYST_CG_RECOMPUTE_AP", "01"), ("KRYST_CG_FUSE_MIN_BYTES", "1")) for v in vs]


def label(setting):
    return "default" if setting is None else "%s=%s" % setting


def _host(ctx, m):
    m = m.tocsr(); m.sort_indices()
    return K.CsrMatrix.from_csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data, ctx=ctx)


def _many_offsets(ctx):
    """600 rows of five random columns: far more than 256 distinct (col - row) offsets -- plain CSR only"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(600), 5)
    m = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, rng.integers(0, 600, len(rows)))), shape=(600, 600))
    m.sum_duplicates()
    return _host(ctx, m)


def _band40(ctx):
    """1 500 rows, the 40 offsets -20 .. 19 (more diagonals than CSR-DIA takes), random values (no value dictionary, no row patterns): CSR-D8"""
    import scipy.sparse as sp
    rng = np.random.default_rng(6)
    n = 1500
    return _host(ctx, sp.diags([rng.standard_normal(n - abs(o)) for o in range(-20, 20)], list(range(-20, 20)), shape=(n, n)))


def _slab_box(ctx):
    """the 128 x 128 x 7 box of test_spmv_slab_order_of_the_tiles_bit_exact (values from a set of three), which gets a slab order of its tiles
    once KRYST_SPMV_ORDER_MIN_PLANE is lowered to 8192 at creation"""
    import scipy.sparse as sp
    rng = np.random.default_rng(77)
    ni, nj, nk = 128, 128, 7
    e = lambda n: sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])      # noqa: E731
    pat = (sp.kron(sp.identity(nk), sp.kron(sp.identity(nj), e(ni))) + sp.kron(sp.identity(nk), sp.kron(e(nj), sp.identity(ni))) +
           sp.kron(e(nk), sp.identity(nj * ni))).tocsr()
    pat.sort_indices()
    pat.data = rng.choice([-1.0, 6.0, 0.5], pat.nnz)
    return _host(ctx, pat)


OPERATORS = {
    "poisson16": lambda ctx: K.CsrMatrix.stencil7(16, "poisson", ctx=ctx),       # a tile spans two planes: no march
    "poisson32": lambda ctx: K.CsrMatrix.stencil7(32, "poisson", ctx=ctx),       # a plane of 1 024 rows: marches only with KRYST_SPMV_FUSE_T=2
    "poisson40": lambda ctx: K.CsrMatrix.stencil7(40, "poisson", ctx=ctx),       # a plane of 1 600 rows: not a whole strip
    "poisson64": lambda ctx: K.CsrMatrix.stencil7(64, "poisson", ctx=ctx),       # two strips at T = 4
    "varcoef21": lambda ctx: K.CsrMatrix.stencil7(21, "varcoef", ctx=ctx),       # CSR-DIA
    "many-offsets": _many_offsets,
    "band40": _band40,
    "slab-box": _slab_box,
}


def answers(d):
    """(encoding, tile_order info[3], pattern_info info[0..3], fuse_march_info info[0..6]) under the current settings"""
    p, f = d.pattern_info(), d.fuse_march_info()
    return (d.encoding()[0], int(d.tile_order()["in_use"]),
            (int(p["line"]), int(p["uniform_far"]), int(p["interior_first"]), int(p["staged"])),
            (int(f["eligible"]), int(f["on"]), int(f["T"]), int(f["strips"]), int(f["S"]), int(f["segments"]), int(f["recompute_ap"])))


# operator -> the answers in the order of SETTINGS
EXPECTED = {
    "poisson16": [
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # default
        ('csr', 0, (16, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (16, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d16', 0, (16, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-p16', 0, (16, 1, -1, 0), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 2, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-p16', 0, (16, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "poisson32": [
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # default
        ('csr', 0, (32, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (32, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d16', 0, (32, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-p16', 0, (32, 1, -1, 0), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-p16', 0, (32, 1, -1, 1), (1, 0, 2, 1, 4, 8, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-p16', 0, (32, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "poisson40": [
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # default
        ('csr', 0, (40, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (40, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d16', 0, (40, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-p16', 0, (40, 1, -1, 0), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 2, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-p16', 0, (40, 1, -1, 1), (0, 0, 4, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "poisson64": [
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # default
        ('csr', 0, (64, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (64, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d16', 0, (64, 1, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_DIA=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_DIA=2
        ('csr-p16', 0, (64, 1, -1, 0), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 1, 4, 2, 4, 16, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 2, 4, 4, 16, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-p16', 0, (64, 1, -1, 1), (1, 0, 4, 2, 4, 16, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-p16', 0, (64, 1, -1, 1), (1, 1, 4, 2, 4, 16, 1)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "varcoef21": [
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # default
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-dia', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "many-offsets": [
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # default
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "band40": [
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # default
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
    "slab-box": [
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # default
        ('csr', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=0
        ('csr-d8', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=1
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=2
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_COMPRESS=3
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_KERNEL=3
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_DIA=2
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_STAGE_UFAR=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=0
        ('csr-d16', 1, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_ORDER=2
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_P=1
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_MARCH=1
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=2
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_SPMV_FUSE_T=4
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=1
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_X_BATCH=8
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=0
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_RECOMPUTE_AP=1
        ('csr-d16', 0, (0, 0, -1, 0), (0, 0, 0, 0, 0, 0, 0)),  # KRYST_CG_FUSE_MIN_BYTES=1
    ],
}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.mark.parametrize("name", list(OPERATORS))
def test_the_choice_is_the_recorded_one(ctx, name, monkeypatch):
    monkeypatch.setenv("KRYST_SPMV_ORDER_MIN_PLANE", "8192")            # (read at creation only)
    d = OPERATORS[name](ctx)
    assert len(EXPECTED[name]) == len(SETTINGS)
    wrong = []
    for setting, want in zip(SETTINGS, EXPECTED[name]):
        with monkeypatch.context() as mp:
            if setting is not None:
                mp.setenv(*setting)
            got = answers(d)
        print(name, label(setting), got)
        if got != want:
            wrong.append((label(setting), got, want))
    assert not wrong, wrong
