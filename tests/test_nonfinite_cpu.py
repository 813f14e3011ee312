"""Non-finite and signed-zero right-hand sides, CPU tier: the references that test_gpu_nonfinite.py compares the device with.

1. The C oracle's Jacobi, ILU(0) as written / textbook, Ilup(p), Ilut and apply_chebyshev on poisoned `r` against plain Python-float
   transcriptions (test_oracle_independent.py, written from the Rust source), by `same_ieee`; the numpy restatements without a C form
   (bjacobi_ref, asm_ref, sor_ref) against their own loop forms.  The oracle is built with `-O2 -ffp-contract=off -fno-fast-math` and no
   value-changing floating-point flag (oracle/Makefile; asserted below), so inf / NaN / signed zeros follow IEEE 754 in it.
2. For every case of the GPU tier the reference ALONE must leave at least 30 % of the output rows finite and make at least 10 % non-finite:
   a case whose expected output is all NaN (or all finite) would prove little.
3. The rows of the un-poisoned half are bit for bit those of the same apply on the clean `r` -- a consequence of the block structure of
   the operators (nonfinite_cases.py), asserted here for the references and in the GPU tier for the device.

Two places where "as written" walks a DENSE row are restated over the stored entries by the oracle and the device (kryst_oracle.c:
tri_apply): Ilu0::apply (ilu.rs:109-119) and Sor::apply (sor.rs:131-166).  On finite data the absent terms are
+-0 products that change nothing; on a non-finite operand they are 0 * inf = NaN in EVERY row.  That is pinned below as what it is, a
labelled deviation: the restatements skip what is not stored (and, in the ILU family, what is stored as zero: `!= T::zero()`)."""
import os

import numpy as np
import pytest

from oracle import oracle as O
import asm_ref as A
import bjacobi_ref as BR
import sor_ref as S
import spai_ref as SP
import nonfinite_cases as C
import test_oracle_independent as TI
from nonfinite_cases import same_ieee, poisoned, clean_r, POISON

CASES = C.apply_cases() + C.spai_cases()


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_same_ieee_counts_signed_zeros_infinities_and_denormals_but_no_nan_payload():
    a = np.array([0.0, np.inf, 5e-324, np.nan, 1.0])
    assert same_ieee(a, a.copy())
    other_nan = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    b = a.copy(); b[3] = other_nan
    assert same_ieee(a, b)                                                  # payload and sign of a NaN do not count
    for i, v in ((0, -0.0), (1, -np.inf), (2, -5e-324), (2, 0.0), (3, 1.0), (4, np.nan)):
        b = a.copy(); b[i] = v
        assert not same_ieee(a, b), (i, v)
    assert not same_ieee(a, a[:4])


def test_poisoned_cycles_through_the_values_and_never_makes_the_ready_flag():
    r = np.zeros(20) + 1.0
    p = poisoned(r, [3, 4, 5, 6, 7, 8, 9, 0])
    assert np.array_equal(p[[3, 4, 5, 6, 7, 8, 9, 0]].view(np.uint64), np.array(POISON + (np.inf,)).view(np.uint64))
    assert np.array_equal(np.delete(p, [3, 4, 5, 6, 7, 8, 9, 0]), np.ones(12)) and np.array_equal(r, np.ones(20))
    sentinel = np.array([C.TRI_SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
    with pytest.raises(AssertionError):
        poisoned(r, [1], values=(sentinel,))


def test_the_oracle_is_built_without_value_changing_floating_point_flags():
    """-ffp-contract=off (no fused multiply-add), -fno-fast-math, and none of the flags that let the compiler assume finite operands or
    ignore signed zeros: the oracle's inf / NaN / -0.0 results are IEEE 754's."""
    flags = open(os.path.join(os.path.dirname(O.__file__), "Makefile")).read()
    cflags = [ln for ln in flags.splitlines() if ln.startswith("CFLAGS")]
    assert len(cflags) == 1 and "-ffp-contract=off" in cflags[0] and "-fno-fast-math" in cflags[0]
    for bad in ("-ffast-math", "-Ofast", "-ffinite-math-only", "-fno-signed-zeros", "-funsafe-math-optimizations", "-fassociative-math", "-freciprocal-math"):
        assert bad not in flags, bad


# ------------------------------------------------------------------------------------------------ 1. the oracle against Python floats
def csr_rows(a):
    return [(a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]].tolist(), a.vals[a.row_ptr[i]:a.row_ptr[i + 1]].tolist()) for i in range(a.nrows)]


def csr_matvec(a, x):                                                       # sparse.rs:56-68: y_i = 0; y_i += v * x[j] over the stored entries
    y = []
    for cols, vals in a:
        s = 0.0
        for j, v in zip(cols, vals):
            s = s + v * x[j]
        y.append(s)
    return y


def ilu0_apply_over_nonzeros(f, x):
    """Ilu0::apply (ilu.rs:105-122) with the terms whose factor entry is zero left out -- the oracle's restatement (kryst_oracle.c: tri_apply)."""
    y = list(x)
    n = len(x)
    for i in range(n):
        for j in range(i):
            if f.l[i][j] != 0.0:
                y[i] = y[i] - f.l[i][j] * y[j]
    for i in reversed(range(n)):
        for j in range(i + 1, n):
            if f.u[i][j] != 0.0:
                y[i] = y[i] - f.u[i][j] * y[j]
    return y


def true_ilu0_apply(a, r):
    """Textbook ILU(0) in IKJ order on the pattern of a (dense lists; zeros of the pattern are entries), then L y = r, U z = y with the
    division -- the labelled extension behind TrueIlu0.  Stored zeros of the FACTORS are skipped in the solves."""
    n = len(a)
    w = [list(row) for row in a]
    pat = [[a[i][j] != 0.0 for j in range(n)] for i in range(n)]
    for i in range(n):
        for k in range(i):
            if pat[i][k]:
                w[i][k] = w[i][k] / w[k][k]
                for j in range(k + 1, n):
                    if pat[i][j] and pat[k][j]:
                        w[i][j] = w[i][j] - w[i][k] * w[k][j]
    y = [0.0] * n
    for i in range(n):
        s = r[i]
        for j in range(i):
            if pat[i][j] and w[i][j] != 0.0:
                s = s - w[i][j] * y[j]
        y[i] = s
    z = [0.0] * n
    for i in reversed(range(n)):
        s = y[i]
        for j in range(i + 1, n):
            if pat[i][j] and w[i][j] != 0.0:
                s = s - w[i][j] * z[j]
        z[i] = s / w[i][i]
    return z


def _two_blocks(rng, n1, n2):
    """dense lists of a block-diagonal, diagonally dominant operator of n1 + n2 rows, sparse inside the blocks"""
    n = n1 + n2
    m = np.zeros((n, n))
    for lo, hi in ((0, n1), (n1, n)):
        b = rng.uniform(-1.0, 1.0, (hi - lo, hi - lo))
        b[rng.random(b.shape) < 0.6] = 0.0
        m[lo:hi, lo:hi] = b
    m += np.diag(np.abs(m).sum(axis=1) + 1.0)
    return m.tolist()


def test_oracle_preconditioners_on_poisoned_r_equal_the_python_float_transcriptions(monkeypatch):
    rng = np.random.default_rng(2718)
    a = _two_blocks(rng, 9, 8)
    n = len(a)
    sparse = O.Csr.from_dense(np.array(a), keep_zeros=False)
    assert not np.isnan(O.Pc.ilu0_true(sparse).apply(np.ones(n))).any()
    rows_of = csr_rows(sparse)
    checked = 0
    for lo, hi in ((0, 9), (9, n)):
        for shift in range(len(POISON)):
            rows = [lo, hi - 1, (lo + hi) // 2]
            r = poisoned(rng.standard_normal(n), rows, POISON[shift:] + POISON[:shift])
            rl = r.tolist()
            want = {
                "jacobi": (O.Pc.jacobi(sparse).apply(r), TI.Jacobi(a).apply(rl)),
                "ilu0 as written": (O.Pc.ilu0_compat(sparse).apply(r), ilu0_apply_over_nonzeros(TI.Ilu0(a), rl)),
                "ilu0 textbook": (O.Pc.ilu0_true(sparse).apply(r), true_ilu0_apply(a, rl)),
                "ilup0": (O.Pc.ilup0(sparse).apply(r), TI.Ilup(a, 0).apply(rl)),
                "ilup(2)": (O.Pc.ilup(sparse, 2).apply(r), TI.Ilup(a, 2).apply(rl)),
                "ilut": (O.Pc.ilut(sparse, 3, 1e-3).apply(r), TI.Ilut(a, 3, 1e-3).apply(rl)),
            }
            with monkeypatch.context() as mp:
                mp.setattr(TI, "matvec", csr_matvec)                        # apply_chebyshev on the CSR operator (sparse.rs), not the dense row loop
                for m in (0, 1, 5):
                    want[f"chebyshev {m}"] = (O.apply_chebyshev(sparse, r, 0.5, 7.5, m), TI.apply_chebyshev(rows_of, rl, 0.5, 7.5, m))
            for name, (got, ref) in want.items():
                assert same_ieee(got, np.array(ref)), (name, lo, shift)
                other = np.ones(n, dtype=bool); other[lo:hi] = False
                assert np.isfinite(got[other]).all(), (name, lo, shift)
                checked += 1
    assert checked == 2 * 7 * 9


def test_a_zero_or_missing_diagonal_times_infinity_is_nan_in_jacobi():
    """jacobi.rs:69-71 stores 0.0 for a zero diagonal and :84-86 multiplies by it: 0 * inf = NaN, 0 * -1 = -0.0"""
    a2 = O.Csr(3, 3, [0, 1, 2, 4], [1, 1, 0, 2], [2.0, 0.0, 1.0, 4.0])      # row 0: no diagonal; row 1: a stored zero
    got = O.Pc.jacobi(a2).apply(np.array([np.inf, -1.0, -0.0]))
    assert same_ieee(got, np.array([np.nan, -0.0, -0.0]))
    dense = [[0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 4.0]]
    assert same_ieee(got, np.array(TI.Jacobi(dense).apply([np.inf, -1.0, -0.0])))


def test_the_dense_walks_of_the_reference_give_nan_in_every_row():
    """The labelled deviation of the module docstring, pinned: Ilu0::apply and Sor::apply as written multiply the absent entries too."""
    rng = np.random.default_rng(5)
    a = _two_blocks(rng, 6, 6)
    r = rng.standard_normal(12); r[0] = np.inf
    assert np.isnan(TI.Ilu0(a).apply(r.tolist())).all()                     # inf in row 0: y[i] - 0 * inf for every i > 0, then back up
    sp = O.Csr.from_dense(np.array(a), keep_zeros=False)
    assert np.isfinite(O.Pc.ilu0_compat(sp).apply(r)[6:]).all()
    d = np.array(a)
    with np.errstate(all="ignore"):
        assert np.isnan(S.apply_loop(d, S.setup(d), r, 1.5, 1, S.SYMMETRIC_SWEEP)).all()
    assert np.isfinite(S.Plan(sp).apply(r, 1.5, 1, S.SYMMETRIC_SWEEP)[6:]).all()


def test_numpy_restatements_on_poisoned_r_equal_their_loop_forms():
    """bjacobi_ref (through the oracle's ApproxInv on M) against apply_pinned block by block, asm_ref.Apply against asm.rs's loop, sor_ref.Plan
    against the loops of sor.rs over the stored entries, spai_ref's M against a dense M r in stored order."""
    rng = np.random.default_rng(31)
    # block Jacobi, b = 8 with a ragged last block
    a = O.stencil7(5, "convdiff")
    n = a.nrows
    r = poisoned(rng.standard_normal(n), [0, 9, 17, 33, 64, 70, n - 1])
    gs, inv, zp = BR.tiles_uniform(a.row_ptr, a.col_idx, a.vals, n, 8)
    z = O.Pc.approx_inverse(O.Csr(n, n, *BR.m_ref_uniform(n, 8, inv))).apply(r)
    with np.errstate(all="ignore"):
        want = np.concatenate([BR.apply_pinned(t[None], r[g][None])[0] for g, t in zip(gs, inv)])
    assert same_ieee(z, want) and np.isnan(z).any() and np.isfinite(z).any()
    # additive Schwarz, every variant
    a = O.stencil7(9, "convdiff")
    for variant, overlap in C.ASM_VARIANTS:
        gs, own, inv, zp = A.setup(a, C._asm_sets(), overlap=overlap, variant=variant)
        _, rows, _ = C._asm_poisonings(variant, overlap)(a)[0]
        r = poisoned(clean_r(a.nrows), rows)
        with np.errstate(all="ignore"):
            got = A.Apply(a.nrows, gs, inv, own, restricted=(variant == "restricted"))(r)
            want = A.apply_loop(a.nrows, gs, inv, r, own, restricted=(variant == "restricted"))
        assert same_ieee(got, want), (variant, overlap)
    # SOR: natural order on the unsymmetric random operator and the cut grid, every direction
    for name in ("random", "grid-small"):
        a = C.sor_operator("random") if name == "random" else C.cut_plane(O.stencil7(6, "convdiff"), 36, 3, False)
        for label, rows, _ in C.half_poisonings(a):
            r = poisoned(clean_r(a.nrows), rows)
            for bits in C.SOR_FLAGS.values():
                assert same_ieee(S.Plan(a).apply(r, 1.5, 2, bits), C.sor_stored_loop(a, r, 1.5, 2, bits)), (name, label, bits)
    # the coloured order: by definition the loops on the permuted operator
    a = C.cut_plane(O.stencil7(6, "convdiff"), 36, 3, False)
    colors = np.random.default_rng(6).integers(0, 4, a.nrows)
    o = S.order_of(colors)
    rows_p = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    import scipy.sparse as sp
    m = sp.csr_matrix((a.vals, (rows_p, a.col_idx)), shape=(a.nrows, a.nrows))[o][:, o].tocsr(); m.sort_indices()
    ap = O.Csr(a.nrows, a.nrows, m.indptr, m.indices, m.data)
    r = poisoned(clean_r(a.nrows), C.half_poisonings(a)[1][1])
    yp = C.sor_stored_loop(ap, r[o], 1.5, 2, S.SYMMETRIC_SWEEP)
    y = np.zeros(a.nrows); y[o] = yp
    assert same_ieee(S.Plan(a, 0.0, colors).apply(r, 1.5, 2, S.SYMMETRIC_SWEEP), y)
    # SPAI: z = M r over the stored entries of M
    a = C.spai_operator()
    (rp, ci, va), _ = SP.setup(a, a.row_ptr, a.col_idx, 1e-12)
    mm = O.Csr(a.nrows, a.nrows, rp, ci, va)
    r = poisoned(clean_r(a.nrows), C.dense_half_poisonings(a)[0][1])
    assert same_ieee(O.Pc.approx_inverse(mm).apply(r), np.array(csr_matvec(csr_rows(mm), r.tolist())))


def test_amg_as_written_on_poisoned_r_and_z_equals_its_dense_restatement():
    """amg_ref.vcycle on the CSR levels against the same recursion on the DENSE levels of amg_new_dense (every entry stored), with r AND
    the incoming z poisoned (amg.rs:211 starts the finest level from z).  Finite special values (-0.0, denormals): bit for bit.
    Non-finite ones: CG on the coarsest level (amg.rs:254-312) folds every row into its inner products, so EVERY row is NaN -- by
    construction no case of AMG as written can leave 30 % of the rows finite; the smoothed-aggregation case (block Jacobi on the coarsest
    level) carries that condition, and this one is pinned as what it is."""
    import amg_ref as R
    a = O.stencil7(4, "convdiff")
    n = a.nrows
    dense_levels = R.amg_new_dense(a.to_dense(), 10, 0.1)
    assert len(dense_levels) >= 2
    sparse = R.csr_levels(dense_levels)
    full = [dict(A=O.Csr.from_dense(L["A"], keep_zeros=True), P=None if L["P"] is None else O.Csr.from_dense(L["P"], keep_zeros=True),
                 R=None if L["R"] is None else O.Csr.from_dense(L["R"], keep_zeros=True), dinv=np.asarray(L["dinv"], dtype=np.float64)) for L in dense_levels]
    r0, z0 = clean_r(n, 1), clean_r(n, 2)
    rows = [0, n - 1, n // 2, 7, 8]
    tame = (-0.0, 5e-324, -5e-324)
    with np.errstate(all="ignore"):
        for r, z in ((r0, z0), (poisoned(r0, rows, tame), z0), (r0, poisoned(z0, rows, tame)), (poisoned(r0, rows, tame), poisoned(z0, rows[::-1], tame))):
            got = R.vcycle(sparse, r, z)
            assert np.isfinite(got).all() and np.array_equal(got.view(np.uint64), R.vcycle(full, r, z).view(np.uint64))
        for r, z in ((poisoned(r0, rows), z0), (r0, poisoned(z0, rows)), (poisoned(r0, rows), poisoned(z0, rows))):
            got = R.vcycle(sparse, r, z)
            assert np.isnan(got).all() and same_ieee(got, R.vcycle(full, r, z))


# ------------------------------------------------------------------------------------------------ 2. and 3. every case of the GPU tier
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_leaves_one_half_finite_and_equal_to_the_clean_apply(case):
    a = case.op()
    ref = case.ref(a)
    n = a.nrows
    r0 = clean_r(n)
    z0 = ref(r0)
    assert np.isfinite(z0).all()
    for label, rows, clean in case.poisonings(a):
        z = ref(poisoned(r0, rows))
        finite = np.isfinite(z)
        assert finite.sum() >= 0.3 * n and (~finite).sum() >= 0.1 * n, (label, int(finite.sum()), n)
        assert clean.sum() >= 0.3 * n and finite[clean].all(), label
        assert np.array_equal(z[clean].view(np.uint64), z0[clean].view(np.uint64)), label       # the block structure, bit for bit
