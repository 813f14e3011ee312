"""Shared cases of the non-finite / signed-zero tests (test_nonfinite_cpu.py: references only; test_gpu_nonfinite.py: the device).

A case is an operator made of two halves WITHOUT coupling (a box cut at a k-plane, or a block-diagonal matrix of two operators), a
preconditioner on it, and right-hand sides `r` poisoned in ONE half with +-inf, NaN, -0.0, the denormals and the largest double.  A
poisoned entry of a connected triangular factor reaches every row of its half, so the expected output is NaN there and FINITE in the
other half -- bit for bit what the same apply gives on the clean `r`.  That second fact follows from the block structure alone, not from
any reference.  The couplings across the cut are either absent or (ILU family: `!= T::zero()` keeps them out of the factors) STORED AS
0.0: a form that multiplied such an entry instead of skipping it would be right on finite data and give 0 * inf = NaN here.

Importable without a GPU: `dev` factories take the product module as an argument and are only called by the GPU tier."""
import functools

import numpy as np

from oracle import oracle as O
import asm_ref as A
import bjacobi_ref as BR
import sor_ref as S

# the ready flag of the sync-free / wavefront triangular solves (ilu.hip, tri_wave.h, tri_box.h, tri_quad.h): never used as an input here --
# an input NaN with exactly these bits is indistinguishable from "not written yet" and ends in the documented give-up path
TRI_SENTINEL_BITS = 0xFFF8DEADBEEFCAFE
POISON = (np.inf, -np.inf, np.nan, -0.0, 5e-324, -5e-324, 1.7976931348623157e308)
assert all(np.float64(v).view(np.uint64) != TRI_SENTINEL_BITS for v in POISON)


def same_ieee(got, want):
    """NaNs at the same positions (payload and sign of a NaN do not count: host and device make different default NaNs), everywhere else
    the same 64 bits: signed zeros, the sign of an infinity and denormals all count."""
    got = np.ascontiguousarray(got, dtype=np.float64); want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]))


def poisoned(r, rows, values=POISON):
    """A copy of r with r[rows[i]] = values[i mod len(values)]."""
    out = np.array(r, dtype=np.float64, copy=True)
    vals = np.array(values, dtype=np.float64)
    assert not (vals.view(np.uint64) == np.uint64(TRI_SENTINEL_BITS)).any()
    rows = np.asarray(rows, dtype=np.int64)
    out[rows] = vals[np.arange(len(rows)) % len(vals)]
    return out


def clean_r(n, seed=1):
    return O.splitmix64_uniform(seed, n) - 0.5


def row_set(lo, hi):
    """Rows of [lo, hi): the first (empty lower part: level 0 of the forward solve; for lo = 0 the column every ELL padding slot names), the
    last (nothing depends on it in the forward solve), the middle (the middle of a dependency level of a grid), and the first and last row
    of the first 512-row tile that lies wholly inside."""
    rows = [lo, hi - 1, (lo + hi) // 2]
    t0 = -(-lo // 512) * 512
    if t0 + 511 < hi:
        rows += [t0, t0 + 511]
    return sorted(set(rows))


# ------------------------------------------------------------------------------------------------ operators of two uncoupled halves
def box_operator(rng, Ni, Nj, Nk, keep, drop=0.0, unsym=True, zeros=0.0):
    """A stencil operator inside the 3 x 3 x 3 cube on an Ni x Nj x Nk box, natural ordering: `keep(dk, dj, di)` selects the couplings (27-point: all),
    a fraction `drop` of the couplings is removed at random, the values are random (unsymmetric), the diagonal dominates."""
    import scipy.sparse as sp
    n = Ni * Nj * Nk
    idx = np.arange(n)
    i, j, k = idx % Ni, (idx // Ni) % Nj, idx // (Ni * Nj)
    rows, cols, vals = [], [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if (dk, dj, di) == (0, 0, 0) or not keep(dk, dj, di):
                    continue
                ok = (i + di >= 0) & (i + di < Ni) & (j + dj >= 0) & (j + dj < Nj) & (k + dk >= 0) & (k + dk < Nk)
                if drop > 0.0:
                    ok &= rng.random(n) >= drop
                r = idx[ok]
                rows.append(r); cols.append(r + di + Ni * dj + Ni * Nj * dk)
                v = -rng.uniform(0.2, 1.0, len(r)) if unsym else -np.ones(len(r))
                if zeros > 0.0:
                    v[rng.random(len(v)) < zeros] = 0.0                    # stored zeros: part of the pattern, never kept in a factor
                vals.append(v)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    dsum = np.ones(n)
    np.add.at(dsum, rows, np.abs(vals))
    m = sp.coo_matrix((np.concatenate([vals, dsum]), (np.concatenate([rows, idx]), np.concatenate([cols, idx]))), shape=(n, n)).tocsr()
    m.sort_indices()
    assert zeros == 0.0 or (m.data == 0.0).any()                           # the zeros are stored
    return O.Csr(n, n, m.indptr, m.indices, m.data)


def _with_cut(a, cut):
    a.cut = int(cut)
    return a


def cut_plane(a, plane_rows, kcut, zeros):
    """The operator `a` on a box in natural ordering (plane_rows rows per k-plane) without the couplings between planes kcut - 1 and kcut:
    removed (zeros=False) or stored as 0.0 (zeros=True)."""
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    cross = (rows // plane_rows < kcut) != (a.col_idx // plane_rows < kcut)
    assert cross.any()
    if zeros:
        v = a.vals.copy(); v[cross] = 0.0
        return _with_cut(O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v), plane_rows * kcut)
    keep = ~cross
    rp = np.zeros(a.nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=a.nrows), out=rp[1:])
    return _with_cut(O.Csr(a.nrows, a.ncols, rp, a.col_idx[keep], a.vals[keep]), plane_rows * kcut)


def block_diag(a, b, zeros):
    """diag(a, b); zeros=True: every row also stores one 0.0 in the other block (row i of a at column na + i mod nb, row i of b at column i mod na)."""
    na, nb = a.nrows, b.nrows
    rp, ci, va = [0], [], []
    for i in range(na):
        c = a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]].tolist(); v = a.vals[a.row_ptr[i]:a.row_ptr[i + 1]].tolist()
        if zeros:
            c.append(na + i % nb); v.append(0.0)
        ci += c; va += v; rp.append(len(ci))
    for i in range(nb):
        c = (b.col_idx[b.row_ptr[i]:b.row_ptr[i + 1]] + na).tolist(); v = b.vals[b.row_ptr[i]:b.row_ptr[i + 1]].tolist()
        if zeros:
            c.insert(0, i % na); v.insert(0, 0.0)
        ci += c; va += v; rp.append(len(ci))
    return _with_cut(O.Csr(na + nb, na + nb, rp, ci, va), na)


def lap_box(Ni, Nj, Nk):
    """The 7-point operator of test_structured_grid_triangular_solve_bit_exact on an Ni x Nj x Nk box (unsymmetric, direction weights 1, 0.7, 0.3)."""
    import scipy.sparse as sp

    def lap(n, w):
        return sp.diags([-w * np.ones(n - 1), 2 * w * np.ones(n), -0.5 * w * np.ones(n - 1)], [-1, 0, 1])
    m = (sp.kron(sp.eye(Nk), sp.kron(sp.eye(Nj), lap(Ni, 1.0))) + sp.kron(sp.eye(Nk), sp.kron(lap(Nj, 0.7), sp.eye(Ni)))
         + sp.kron(lap(Nk, 0.3), sp.kron(sp.eye(Nj), sp.eye(Ni)))).tocsr()
    m.sort_indices(); m.eliminate_zeros()
    return O.Csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)


def random_dominant(n, seed, density=0.05):
    """The random CSR-factor operator of test_triangular_solve_forms_bit_exact (irregular levels, rows longer than an ELL row)."""
    rng = np.random.default_rng(seed)
    dense = rng.random((n, n)) * (rng.random((n, n)) < density) + np.diag(5.0 + rng.random(n))
    return O.Csr.from_dense(dense, keep_zeros=False)


def deep_narrow(n, free, seed):
    """One half of the deep, narrow factor of test_narrow_level_runs_of_a_deep_factor_bit_exact: `free` independent rows, then rows of nine
    entries within +-300 rows, one in ten anywhere in the half, fifty rows of ~30 entries; diagonally dominant."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(free, n), 9)
    near = rows + rng.integers(-300, 301, len(rows))
    far = rng.integers(0, n, len(rows))
    cols = np.clip(np.where(rng.random(len(rows)) < 0.1, far, near), 0, n - 1)
    m = sp.csr_matrix((rng.uniform(-1.0, 1.0, len(rows)), (rows, cols)), shape=(n, n)); m.sum_duplicates()
    dr = rng.choice(np.arange(free, n), 50, replace=False)
    extra = sp.csr_matrix((rng.uniform(-1.0, 1.0, 50 * 24), (np.repeat(dr, 24), np.clip(np.repeat(dr, 24) + rng.integers(-2000, 2001, 50 * 24), 0, n - 1))), shape=(n, n))
    m = (m + extra).tocsr(); m.sum_duplicates()
    m = m - sp.diags(m.diagonal()) + sp.diags(np.asarray(abs(m).sum(axis=1)).ravel() + 1.0)
    m = m.tocsr(); m.sort_indices(); m.eliminate_zeros()
    return O.Csr(n, n, m.indptr, m.indices, m.data)


ALL27 = lambda dk, dj, di: True                                            # noqa: E731


@functools.lru_cache(maxsize=None)
def operator(name, zeros):
    """The two-halves operators by name; `zeros`: the couplings across the cut are stored as 0.0 instead of being absent."""
    if name == "grid24":                                                   # ELL factors (3 entries per row), 70 levels, 27 tiles
        return cut_plane(O.stencil7(24, "aniso"), 24 * 24, 12, zeros)
    if name == "grid17":
        return cut_plane(O.stencil7(17, "convdiff"), 17 * 17, 8, zeros)
    if name == "rand300":                                                  # CSR factors, irregular levels
        return block_diag(random_dominant(300, 77), random_dominant(300, 78), zeros)
    if name == "grid9x2":                                                  # Ilup(2): fill-in, long rows
        return block_diag(O.stencil7(9, "convdiff"), O.stencil7(9, "convdiff"), zeros)
    if name == "tri700":                                                   # 350 + 350 levels of one row
        return cut_plane(O.Csr.from_dense(O.tridiag(700, -1.0, 2.5, -0.5), keep_zeros=False), 350, 1, zeros)
    if name == "deep":                                                     # 2 x 20 000 rows, hundreds of narrow levels
        return block_diag(deep_narrow(20000, 1500, 2024), deep_narrow(20000, 1500, 2025), zeros)
    if name == "deep-wide-first":                                          # 3 000 independent rows first: a level kernel of its own, then the run
        return block_diag(deep_narrow(20000, 3000, 2026), deep_narrow(20000, 3000, 2027), zeros)
    if name == "box27-41x30x19":                                           # 13 entries per factor row: chains of two virtual rows
        rng = np.random.default_rng(3)
        return cut_plane(box_operator(rng, 41, 30, 19, ALL27), 41 * 30, 9, zeros)
    if name == "lap23x17x9":                                               # sides no multiple of the 8 x 8 / 16 x 16 line blocks
        return cut_plane(lap_box(23, 17, 9), 23 * 17, 4, zeros)
    if name == "lap34x16x32":                                              # whole 16 x 16 blocks (the 64-byte result groups of tri_quad.h)
        return cut_plane(lap_box(34, 16, 32), 34 * 16, 16, zeros)
    if name == "box27-17x9x10":
        return cut_plane(box_operator(np.random.default_rng(27), 17, 9, 10, ALL27), 17 * 9, 5, zeros)
    if name == "box27-13x12x11-holes":                                     # couplings missing and stored zeros INSIDE the halves too: not "regular"
        return cut_plane(box_operator(np.random.default_rng(28), 13, 12, 11, ALL27, drop=0.1, zeros=0.1), 13 * 12, 5, zeros)
    raise KeyError(name)


def half_poisonings(a):
    """[(label, rows to poison, mask of the rows that must equal the clean apply bit for bit)]: one half at a time"""
    out = []
    for label, lo, hi in (("low", 0, a.cut), ("high", a.cut, a.nrows)):
        clean = np.ones(a.nrows, dtype=bool); clean[lo:hi] = False
        out.append((label, row_set(lo, hi), clean))
    return out


def dense_half_poisonings(a):
    """every other row of one half (m = 0 copies r: only the poisoned rows themselves are non-finite) and the half's edges"""
    out = []
    for label, lo, hi in (("low", 0, a.cut), ("high", a.cut, a.nrows)):
        clean = np.ones(a.nrows, dtype=bool); clean[lo:hi] = False
        out.append((label, sorted(set(range(lo, hi, 2)) | {hi - 1}), clean))
    return out


class Case:
    """id; env: the settings that select the form; op() -> oracle Csr; ref(a) -> r |-> z on the CPU; dev(K, d) -> a set-up device
    preconditioner (anything with .apply(r, z)); poisonings(a) -> [(label, rows, clean mask)]; form: what ilu_info must report, before and after;
    dev_ref(pc): the GPU tier's reference where it is made from the device's own set-up."""

    def __init__(self, id, op, ref, dev, poisonings=half_poisonings, env=None, form=None, dev_ref=None, min_levels=0):
        self.id, self.op, self.ref, self.dev, self.poisonings, self.env, self.form = id, op, ref, dev, poisonings, dict(env or {}), form
        self.min_levels = min_levels        # ilu_info must report more dependency levels than this in both factors: only runs of narrow levels
                                            # go to the one-workgroup run kernels (no entry point names the kernel an apply launched)
        self.dev_ref = dev_ref              # pc -> r |-> z: a reference built from what the device set up (SPAI: the exported M)

    def __repr__(self):
        return self.id


# ------------------------------------------------------------------------------------------------ ILU family
ILU_KINDS = {
    "true": (lambda K: K.TrueIlu0(), O.Pc.ilu0_true),
    "compat": (lambda K: K.Ilu0(), O.Pc.ilu0_compat),
    "ilup0": (lambda K: K.Ilup(0), O.Pc.ilup0),
    "ilup1": (lambda K: K.Ilup(1), lambda a: O.Pc.ilup(a, 1)),
    "ilup2": (lambda K: K.Ilup(2), lambda a: O.Pc.ilup(a, 2)),
    "ilut": (lambda K: K.Ilut(3, 1e-12), lambda a: O.Pc.ilut(a, 3, 1e-12)),
}


@functools.lru_cache(maxsize=None)
def _ilu_ref(opname, zeros, kind):
    return ILU_KINDS[kind][1](operator(opname, zeros))


def _ilu(id, opname, kind, env, form, min_levels=0):
    out = []
    # Ilut eliminates nothing and keeps three entries per row: a poisoned row reaches few others, so every other row of the half is poisoned
    poisonings = dense_half_poisonings if kind == "ilut" else half_poisonings
    for zeros in (False, True):
        out.append(Case(f"{id}-{kind}-{'zeros' if zeros else 'absent'}", functools.partial(operator, opname, zeros),
                        lambda a, o=opname, z=zeros, k=kind: _ilu_ref(o, z, k).apply,
                        lambda K, d, k=kind: ILU_KINDS[k][0](K).setup(d), poisonings=poisonings, env=env, form=form, min_levels=min_levels))
    return out


def ilu_cases():
    c = []
    lv = {"KRYST_ILU_GRID": "0", "KRYST_ILU_BOX": "0"}
    for sf in ("0", "1"):                                                  # one launch per level / the sync-free single launch
        e = dict(lv, KRYST_ILU_SYNCFREE=sf)
        c += _ilu(f"levels-sf{sf}-ell", "grid24", "true", e, "level-ordered")
        if sf == "0":                                                      # without the run kernels every level is one tri_level_ell_kernel launch (ell_row)
            c += _ilu("levels-sf0-ell-level-kernel", "grid24", "true", dict(e, KRYST_ILU_RUN_FREE="0"), "level-ordered")
        c += _ilu(f"levels-sf{sf}-csr", "rand300", "compat", e, "level-ordered")
        c += _ilu(f"levels-sf{sf}-longrows", "grid9x2", "ilup2", e, "level-ordered")
        c += _ilu(f"levels-sf{sf}-onerow", "tri700", "ilup0", e, "level-ordered")
        c += _ilu(f"levels-sf{sf}-fill", "rand300", "ilut", e, "level-ordered")
        c += _ilu(f"levels-sf{sf}-fill", "grid9x2", "ilup1", e, "level-ordered")
    for pipe in ("free8", "free4", "free1", "free8-wide-first-level", "1", "0"):       # the one-workgroup run kernels of narrow levels
        e = {"KRYST_ILU_SYNCFREE": "0"}
        if pipe.startswith("free"):
            e.update(KRYST_ILU_RUN_FREE="1", KRYST_ILU_FREE_WAVES=pipe[4])
        else:
            e.update(KRYST_ILU_RUN_FREE="0", KRYST_ILU_RUN_PIPE=pipe)
        c += _ilu(f"run-{pipe}", "deep-wide-first" if pipe.endswith("first-level") else "deep", "true", e, "level-ordered", min_levels=200)
    for tune in ("16897", "513", "8705"):                                  # chains of virtual rows through the LDS ring, all three loop forms
        c += _ilu(f"free-tune{tune}", "box27-41x30x19", "true", {"KRYST_ILU_BOX": "0", "KRYST_ILU_FREE_TUNE": tune}, "level-ordered")
    for path, e, form in (("quad", {"KRYST_ILU_GRID": "1", "KRYST_ILU_WAVE": "2"}, "grid"), ("1", {"KRYST_ILU_GRID": "1", "KRYST_ILU_WAVE": "1"}, "grid"),
                          ("wave0", {"KRYST_ILU_GRID": "1", "KRYST_ILU_WAVE": "0"}, "grid"), ("0", {"KRYST_ILU_GRID": "0", "KRYST_ILU_WAVE": "2"}, "box")):       # without the grid kernels a 7-point box is a box operator
        for opname in ("lap23x17x9", "lap34x16x32"):
            for kind in ("true", "compat"):
                c += _ilu(f"grid-{path}-{opname}", opname, kind, e, form)
    for f, v, form in (("wave", "2", "box wavefront"), ("box", "1", "box planes"), ("levels", "0", "level-ordered")):
        for opname in ("box27-17x9x10", "box27-13x12x11-holes"):
            for kind in ("true", "compat"):
                c += _ilu(f"box-{f}-{opname}", opname, kind, {"KRYST_ILU_BOX": v}, form)
    for kind in ("true", "compat", "ilup0"):
        c += _ilu("planes", "grid17", kind, {"KRYST_ILU_PLANES": "1"}, "grid 8x8")
        # (the setting is read by every apply and sends it to tri_plane_kernel; ilu_info names the form the factors were laid out for, and
        # "grid planes" only after a give-up -- so a fall-back would still change it)
    return c


# ------------------------------------------------------------------------------------------------ Jacobi, Chebyshev
@functools.lru_cache(maxsize=None)
def jacobi_operator():
    """stencil7(9, convdiff) with a diagonal stored as 0.0 (row 5) and a missing one (row 7): the inverse is 0.0 there (jacobi.rs:69-71)"""
    a = O.stencil7(9, "convdiff")
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v = a.vals.copy()
    v[(rows == 5) & (a.col_idx == 5)] = 0.0
    keep = ~((rows == 7) & (a.col_idx == 7))
    rp = np.zeros(a.nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=a.nrows), out=rp[1:])
    return O.Csr(a.nrows, a.ncols, rp, a.col_idx[keep], v[keep])


def pointwise_poisonings(a):
    """every third row and the edges; rows 5 and 7 (inverse 0.0) get +inf and -inf: 0 * inf = NaN is what the reference does"""
    rows = [5, 7] + sorted((set(range(0, a.nrows, 3)) | {a.nrows - 1, 511, 512}) - {5, 7})
    clean = np.ones(a.nrows, dtype=bool); clean[rows] = False
    return [("thirds", rows, clean)]


def jacobi_cases():
    return [Case("jacobi-zero-and-missing-diagonal", jacobi_operator, lambda a: O.Pc.jacobi(a).apply, lambda K, d: K.Jacobi().setup(d),
                 poisonings=pointwise_poisonings)]


class _Cheb:
    def __init__(self, K, d, m):
        self.K, self.d, self.m = K, d, m

    def apply(self, r, z):
        return self.K.apply_chebyshev(self.d, r, z, 0.2, 11.9, self.m)


def chebyshev_cases():
    op = lambda: block_diag(O.stencil7(8), O.stencil7(8), False)           # noqa: E731  (1 024 rows: the cut is a tile boundary)
    return [Case(f"chebyshev-m{m}", op, lambda a, m=m: (lambda r: O.apply_chebyshev(a, r, 0.2, 11.9, m)), lambda K, d, m=m: _Cheb(K, d, m),
                 poisonings=dense_half_poisonings) for m in (0, 1, 5)]


# ------------------------------------------------------------------------------------------------ block Jacobi, additive Schwarz, SPAI
def _approx_inverse(rp, ci, va, n):
    m = O.Csr(n, n, rp, ci, va)
    pc = O.Pc.approx_inverse(m)
    return lambda r: pc.apply(r)


def _block_poisonings(blocks_of, stride):
    """rows: the last row first (+inf: the ragged last block), row 0, a tile's edges, then every stride-th row; clean: the rows of blocks
    without a poisoned row, and rows in no block"""
    def f(a):
        n = a.nrows
        first = [n - 1, 0, 511, 512]
        rows = first + sorted(set(range(stride, n, stride)) - set(first))
        hit = np.zeros(n, dtype=bool); hit[rows] = True
        clean = np.ones(n, dtype=bool)
        owner = {}
        for g in blocks_of(a):
            for row in g:
                owner[int(row)] = g                                        # the last block that contains a row decides it
        for row, g in owner.items():
            clean[row] = not hit[np.asarray(g, dtype=np.int64)].any()
        return [("scattered", rows, clean)]
    return f


def _index_blocks(n):
    """unsorted index sets of 0 .. 64 rows that overlap and leave rows uncovered (test_index_sets_unsorted_overlapping_uncovered)"""
    rng = np.random.default_rng(1)
    sizes = rng.integers(0, 65, 40); sizes[:3] = (0, 64, 1)
    return [rng.choice(n, size=int(s), replace=False) for s in sizes]


def block_jacobi_cases():
    op = lambda: O.stencil7(9, "convdiff")                                 # noqa: E731  729 rows: 8 | 728, 64 leaves a block of 25 rows
    c = []
    for b in (1, 8, 64):
        def ref(a, b=b):
            gs, inv, zp = BR.tiles_uniform(a.row_ptr, a.col_idx, a.vals, a.nrows, b)
            return _approx_inverse(*BR.m_ref_uniform(a.nrows, b, inv), a.nrows)
        c.append(Case(f"block-jacobi-uniform{b}", op, ref, lambda K, d, b=b: K.BlockJacobi.uniform(b).setup(d),
                      poisonings=_block_poisonings(lambda a, b=b: BR.uniform_blocks(a.nrows, b), {1: 3, 8: 24, 64: 200}[b])))

    def ref_sets(a):
        gs, inv, zp = BR.tiles_of(a.row_ptr, a.col_idx, a.vals, _index_blocks(a.nrows))
        return _approx_inverse(*BR.m_ref(a.nrows, gs, inv), a.nrows)
    c.append(Case("block-jacobi-index-sets", op, ref_sets, lambda K, d: K.BlockJacobi(_index_blocks(d.nrows())).setup(d),
                  poisonings=_block_poisonings(lambda a: _index_blocks(a.nrows), 400)))
    return c


def _asm_sets(N=9):
    """boxes of 3 x 3 x 2 points with every fifth dropped (uncovered rows), and shifted half copies (rows owned by two subdomains), unsorted"""
    rng = np.random.default_rng(N)
    r = np.arange(N ** 3)
    box_of = (r % N) // 3 + 3 * (((r // N) % N) // 3 + 3 * ((r // (N * N)) // 2))
    bx = [r[box_of == k] for k in range(int(box_of.max()) + 1)]
    keep = [rng.permutation(g) for k, g in enumerate(bx) if k % 5 != 2]
    extra = [rng.permutation(g[: len(g) // 2] + 1) for g in bx[::4] if g.max() + 1 < N ** 3]
    return keep + extra


ASM_VARIANTS = (("as_written", 0), ("grown", 1), ("restricted", 0), ("restricted", 1))


def _asm_setup(a, variant, overlap):
    return A.setup(a, _asm_sets(), overlap=overlap, variant=variant)


def _asm_poisonings(variant, overlap):
    def f(a):
        n = a.nrows
        gs, own, inv, zp = _asm_setup(a, variant, overlap)
        count = np.zeros(n, dtype=np.int64)
        for g in gs:
            count[g] += 1
        shared = int(np.flatnonzero(count >= 2)[0])                        # a row in two subdomains
        rows = sorted({shared, 0, n - 1, 511, 512} | set(range(3, n, n if variant == "grown" else 45)))    # grown sets reach ~300 rows around a row: the five named rows only
        hit = np.zeros(n, dtype=bool); hit[rows] = True
        bad = [bool(hit[g].any()) for g in gs]
        clean = np.ones(n, dtype=bool)
        if variant == "restricted":
            for row in np.flatnonzero(own >= 0):
                clean[row] = not bad[own[row]]
        else:
            for g, b in zip(gs, bad):
                if b:
                    clean[g] = False
        return [("scattered", rows, clean)]
    return f


def asm_cases():
    op = lambda: O.stencil7(9, "convdiff")                                 # noqa: E731
    c = []
    for variant, overlap in ASM_VARIANTS:
        def ref(a, variant=variant, overlap=overlap):
            gs, own, inv, zp = _asm_setup(a, variant, overlap)
            assert all(z == -1 for z in zp)
            M = A.Apply(a.nrows, gs, inv, own, restricted=(variant == "restricted"))

            def apply(r):
                with np.errstate(all="ignore"):
                    return M(r)
            return apply

        def dev(K, d, variant=variant, overlap=overlap):
            p = K.AdditiveSchwarz(overlap, _asm_sets(), None)
            p = {"as_written": p, "grown": p.with_overlap() if variant == "grown" else p, "restricted": p.restricted() if variant == "restricted" else p}[variant]
            return p.setup(d)
        c.append(Case(f"asm-{variant}-overlap{overlap}", op, ref, dev, poisonings=_asm_poisonings(variant, overlap)))
    return c


@functools.lru_cache(maxsize=None)
def spai_operator():
    return block_diag(O.stencil7(6, "convdiff"), O.stencil7(6, "convdiff"), False)


def spai_cases():
    """Spai(pattern of A, 1e-12): the apply is z = M r.  The device's M agrees with spai_ref's to rounding only (another least-squares
    solver), so the GPU tier takes its reference from the exported M; the conditions of the CPU tier depend on M's pattern alone."""
    import spai_ref as SP

    def ref(a):
        (rp, ci, va), _ = SP.setup(a, a.row_ptr, a.col_idx, 1e-12)
        return _approx_inverse(rp, ci, va, a.nrows)

    def dev_ref(pc):
        rp, ci, va = pc.export()
        return _approx_inverse(rp, ci.astype(np.int64), va, len(rp) - 1)
    return [Case("spai-operator-pattern", spai_operator, ref, lambda K, d: K.Spai(K.SparsityPattern.Operator, 1e-12).setup(d),
                 poisonings=dense_half_poisonings, dev_ref=dev_ref)]


# ------------------------------------------------------------------------------------------------ SOR / SSOR
SOR_FLAGS = {"lower": S.APPLY_LOWER, "upper": S.APPLY_UPPER, "symmetric": S.SYMMETRIC_SWEEP}


def sor_stored_loop(a, x, omega, its, sym, fshift=0.0):
    """sor.rs:124-170 on Python floats over the STORED entries of each row in ascending column (the device's
    restatement; the dense walk of the reference also multiplies the absent entries, +0.0 * x_j, which is NaN for a non-finite x_j)."""
    n = a.nrows
    rp = [int(v) for v in a.row_ptr]; ci = [int(v) for v in a.col_idx]; va = [float(v) for v in a.vals]
    inv = []
    for i in range(n):
        d = 0.0
        for k in range(rp[i], rp[i + 1]):
            if ci[k] == i:
                d = va[k]
        inv.append(1.0 / (d + fshift))
    x = [float(v) for v in x]
    y = [0.0] * n
    mul = lambda p, q: float(np.float64(p) * np.float64(q))               # noqa: E731  (inf * 0 without a Python exception)
    for _ in range(its):
        if sym & S.APPLY_LOWER:
            for i in range(n):
                sigma = 0.0
                for k in range(rp[i], rp[i + 1]):
                    if ci[k] < i:
                        sigma = sigma + mul(va[k], y[ci[k]])
                if not sym & S.EISENSTAT:
                    for k in range(rp[i], rp[i + 1]):
                        if ci[k] > i:
                            sigma = sigma + mul(va[k], x[ci[k]])
                y[i] = mul(x[i] - sigma, inv[i])
        if sym & S.APPLY_UPPER:
            for i in range(n - 1, -1, -1):
                sigma = 0.0
                for k in range(rp[i], rp[i + 1]):
                    if ci[k] > i:
                        sigma = sigma + mul(va[k], y[ci[k]])
                if not sym & S.EISENSTAT:
                    for k in range(rp[i], rp[i + 1]):
                        if ci[k] < i:
                            sigma = sigma + mul(va[k], y[ci[k]])
                y[i] = mul(1.0 - omega, x[i]) + mul(omega, mul(x[i] - sigma, inv[i]))
    return np.array(y)


def sor_random(n, seed, density=0.06):
    """test_gpu_sor.random_sparse: unsymmetric, rows without off-diagonal entries, negative and tiny values"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) * (rng.random((n, n)) < density)
    m[rng.random((n, n)) < 0.01] = 1e-300
    m[rng.random((n, n)) < 0.01] = -3e-17
    m[rng.choice(n, max(n // 10, 1), replace=False), :] = 0.0
    np.fill_diagonal(m, rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 4.0, n))
    return O.Csr.from_dense(m, keep_zeros=False)


@functools.lru_cache(maxsize=None)
def sor_operator(name):
    if name == "random":                                                   # unsymmetric pattern: the anti-dependencies of a backward sweep
        return block_diag(sor_random(200, 2), sor_random(200, 3), False)
    return cut_plane(O.stencil7(12, "convdiff"), 144, 6, False)            # 1 728 rows: two workgroups, 34 levels as written


def sor_colors(name, a):
    if name == "natural":
        return None
    if name == "red-black":
        r = np.arange(a.nrows)
        return (r % 12 + (r // 12) % 12 + r // 144) % 2
    return _multicolour("grid")


@functools.lru_cache(maxsize=None)
def _multicolour(_):
    return S.color_graph_csr(sor_operator("grid"))                         # coloring.rs restated in Python (distance-2 greedy): no product code in a reference


SOR_CASES = [("random", "natural"), ("grid", "natural"), ("grid", "red-black"), ("grid", "multicolour")]


def sor_cases():
    c = []
    for opname, order in SOR_CASES:
        for flag, bits in SOR_FLAGS.items():
            def ref(a, order=order, opname=opname, bits=bits):
                plan = S.Plan(a, 0.0, sor_colors(order, a), False)
                return lambda r: plan.apply(r, 1.5, 2, bits)

            def dev(K, d, order=order, opname=opname, bits=bits):
                a = sor_operator(opname)
                return K.Sor(1.5, 2, 1, K.MatSorType(bits) | K.MatSorType.LOCAL_FORWARD_SWEEP, 0.0).with_colors(sor_colors(order, a)).setup(d)
            # a coloured or one-directional sweep carries a value a few rows only: every other row of the half is poisoned on the grid
            c.append(Case(f"sor-{opname}-{order}-{flag}", functools.partial(sor_operator, opname), ref, dev,
                          poisonings=half_poisonings if opname == "random" else dense_half_poisonings))
    return c


# ------------------------------------------------------------------------------------------------ AMG
@functools.lru_cache(maxsize=None)
def amg_sa_operator():
    """2 x 16^3 rows, 795 coarse points: the smallest cube pair at which the one coarsest-level block that holds coarse points of both
    halves leaves 30 % of all rows out of reach (15^3: 31 %, 14^3 and below: under 30 %)"""
    return block_diag(O.stencil7(16), O.stencil7(16), False)


def _bool_mv(c, t):
    """which rows of the CSR operator c have a stored entry in a marked column"""
    rows = np.repeat(np.arange(c.nrows), np.diff(c.row_ptr))
    out = np.zeros(c.nrows, dtype=bool)
    out[rows[t[c.col_idx]]] = True
    return out


def sa_taint(levels, tr, nu_pre=2, nu_post=2, level=0):
    """The rows a marked r can reach in the smoothed-aggregation V-cycle, from the PATTERNS of A, P, R alone (z from zero; damped Jacobi
    z += w D^-1 (r - A z); the coarsest level block Jacobi of 64 contiguous rows, whose dense tiles couple a whole block)."""
    L = levels[level]
    n = L["A"].nrows
    if level + 1 == len(levels):
        b = min(64, max(n, 1))
        out = np.zeros(n, dtype=bool)
        for s0 in range(0, n, b):
            out[s0:s0 + b] = tr[s0:s0 + b].any()
        return out
    tz = np.zeros(n, dtype=bool)
    for _ in range(nu_pre):
        tz = tz | tr | _bool_mv(L["A"], tz)
    tzc = sa_taint(levels, _bool_mv(L["R"], tr | _bool_mv(L["A"], tz)), nu_pre, nu_post, level + 1)
    tz = tz | _bool_mv(L["P"], tzc)
    for _ in range(nu_post):
        tz = tz | tr | _bool_mv(L["A"], tz)
    return tz


@functools.lru_cache(maxsize=None)
def _sa_levels():
    import amg_ref as R
    return R.sa_hierarchy(amg_sa_operator(), 1, 0.0)


def _sa_poisonings(a):
    """every fourth row of one half; clean: what the V-cycle cannot reach from there (the two halves share no aggregate, but one 64-row
    block of the coarsest level's block Jacobi holds coarse points of both)"""
    out = []
    for label, lo, hi in (("low", 0, a.cut), ("high", a.cut, a.nrows)):
        rows = sorted(set(range(lo, hi, 4)) | {lo, hi - 1})
        t = np.zeros(a.nrows, dtype=bool); t[rows] = True
        out.append((label, rows, ~sa_taint(_sa_levels(), t)))
    return out


def amg_cases():
    """Smoothed aggregation on two levels (a labelled extension: z from zero).  AMG as written ends in CG on the coarsest level, whose inner
    products reach every row: its cases are tests of their own (test_nonfinite_cpu.py, test_gpu_nonfinite.py)."""
    import amg_ref as R

    def ref(a):
        levels = _sa_levels()
        assert len(levels) == 2 and levels[1]["A"].nrows > 64
        f = R.sa_apply(levels)

        def apply(r):
            with np.errstate(all="ignore"):
                return f(r)
        return apply
    return [Case("amg-sa-two-levels", amg_sa_operator, ref, lambda K, d: K.Amg(1).with_textbook(0.0).setup(d), poisonings=_sa_poisonings)]


def apply_cases():
    """every case of the GPU tier whose reference needs no device"""
    return ilu_cases() + jacobi_cases() + chebyshev_cases() + block_jacobi_cases() + asm_cases() + sor_cases() + amg_cases()
