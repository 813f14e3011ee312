"""The restatement of additive Schwarz with ILU(0) subdomain solves (tests/asm_ilu_ref.py) against the oracle and the reference's own
test, without a GPU; the interface the device tests go through exists."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import asm_ref as A
import asm_ilu_ref as R
import nonfinite_cases as C

MODES = ("ilup0", "ilu0")
# every test of this file is about the preconditioner that `with_sub_ilu` selects
SUB_ILU = K.AdditiveSchwarz(0, None, 4).with_sub_ilu


def _random_sparse(n, seed, zeros=True):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.08)
    np.fill_diagonal(m, 4.0 + rng.random(n))
    a = O.Csr.from_dense(m, keep_zeros=False)
    if zeros:                                          # explicit stored zeros: part of the pattern, never part of a sweep
        v = a.vals.copy()
        rows = np.repeat(np.arange(n), np.diff(a.row_ptr))
        v[(rng.random(len(v)) < 0.1) & (rows != a.col_idx)] = 0.0
        a = O.Csr(n, n, a.row_ptr, a.col_idx, v)
    return a


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,n,parts", [("poisson", 216, 4), ("convdiff", 343, 5), ("random", 150, 7), ("random", 150, 151)])
def test_disjoint_parts_equal_the_global_factorisation_of_the_block_diagonal(mode, kind, n, parts):
    """contiguous disjoint parts: the restatement is the oracle's global ilup0 / ilu0_true of A without its off-block entries, bit for bit"""
    assert SUB_ILU(mode).sub_mode == {"ilup0": 1, "ilu0": 2}[mode]
    a = _random_sparse(n, parts) if kind == "random" else O.stencil7(round(n ** (1 / 3)), kind)
    s = R.Setup(a, None, capacity=parts, mode=mode)
    assert len(s.gs) == parts and sum(len(g) for g in s.gs) == a.nrows
    bd = R.block_diagonal(a, s.gs)
    pc = R.MODES[mode](bd)
    rng = np.random.default_rng(n)
    for _ in range(3):
        r = rng.standard_normal(a.nrows)
        r[::7] = -0.0
        want = pc.apply(r)
        assert np.array_equal(s(r), want) and np.array_equal(s.apply_loop(r), want)
        nz = want != 0.0                               # the combine's 0.0 + x turns a -0.0 of the sweeps into +0.0: the one difference
        assert np.array_equal(np.signbit(s(r))[nz], np.signbit(want)[nz]) and not np.signbit(s(r))[~nz].any()
    # the factor values on the blocks' patterns are those of the global factorisation
    w = np.concatenate([R.factor_values(p) for p in s.pcs if p is not None])
    assert np.array_equal(w, R.factor_values(pc))


@pytest.mark.parametrize("mode", MODES)
def test_reference_identity(mode):
    """asm.rs:125-136: the 4 x 4 identity, subdomains [0, 1] and [2, 3], r = [1, 2, 3, 4] gives z == r"""
    assert SUB_ILU(mode).variant == K.AdditiveSchwarz.AS_WRITTEN
    a = O.Csr.from_dense(np.eye(4), keep_zeros=True)
    r = np.array([1.0, 2.0, 3.0, 4.0])
    s = R.Setup(a, [[0, 1], [2, 3]], mode=mode)
    assert np.array_equal(s(r), r) and np.array_equal(s.apply_loop(r), r)


@pytest.mark.parametrize("variant", ["as_written", "grown", "restricted"])
@pytest.mark.parametrize("mode", MODES)
def test_vectorised_combine_equals_the_loop(mode, variant):
    assert SUB_ILU(mode).sub_mode in (1, 2)
    a = O.stencil7(6, "convdiff")
    rng = np.random.default_rng(3)
    sets = [rng.permutation(g) for g in A.uniform_parts(a.nrows, 9)[:-1]] + [rng.choice(a.nrows, 30, replace=False)]
    s = R.Setup(a, sets, overlap=1, variant=variant, mode=mode)
    cover = np.zeros(a.nrows, dtype=np.int64)
    for g in s.gs:
        cover[g] += 1
    assert (cover == 0).any() or variant != "as_written"
    assert cover.max() >= 2
    r = rng.standard_normal(a.nrows)
    z = s(r)
    assert np.array_equal(z, s.apply_loop(r))
    if variant == "as_written":
        assert np.all(z[cover == 0] == 0.0) and not np.signbit(z[cover == 0]).any()


@pytest.mark.parametrize("mode", MODES)
def test_levels_of_a_tridiagonal_and_of_a_diagonal_submatrix(mode):
    assert SUB_ILU(mode).sub_mode in (1, 2)
    t = O.Csr.from_dense(O.tridiag(30, -1.0, 2.5, -0.5), keep_zeros=False)
    pc = R.MODES[mode](t)
    ll, lu = R.levels(t, R.factor_values(pc))
    assert np.array_equal(ll, np.arange(1, 31)) and np.array_equal(lu, np.arange(30, 0, -1))
    d = O.Csr.from_dense(np.diag(np.arange(1.0, 9.0)), keep_zeros=True)    # stored zeros everywhere off the diagonal: one level
    pc = R.MODES[mode](d)
    ll, lu = R.levels(d, R.factor_values(pc))
    assert ll.max() == 1 and lu.max() == 1


# the pinned results of an apply on non-finite and signed-zero input: S = [[2, 0s, .], [-1, 4, -1], [., -1, 2]] in one subdomain, rows 3 and 4
# a subdomain of their own whose coupling to it is stored as 0.0 (dropped with the columns outside the set)
def _pinned_operator():
    d = np.array([[2.0, 0.0, 0.0, 0.0, 0.0],
                  [-1.0, 4.0, -1.0, 0.0, 0.0],
                  [0.0, -1.0, 2.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 8.0, -2.0],
                  [0.0, 0.0, 0.0, -2.0, 4.0]])
    return O.Csr.from_dense(d, keep_zeros=True)


def _pinned_clean():
    """r = [2, 3, 1 | 8, 4] by hand.  Textbook ILU(0) of the first block: l10 = -1/2, l20 = 0/2 = 0 (stored, takes no part), l21 = -1/4,
    u22 = 2 - (-0.25 * -1) = 1.75; of the second: l = -2/8, u11 = 4 - (-0.25 * -2) = 3.5."""
    y1 = 3.0 - (-0.5 * 2.0)
    y2 = 1.0 - (-0.25 * y1)
    z2 = y2 / 1.75
    z1 = (y1 - (-1.0 * z2)) / 4.0
    z0 = 2.0 / 2.0
    y4 = 4.0 - (-0.25 * 8.0)
    z4 = y4 / 3.5
    z3 = (8.0 - (-2.0 * z4)) / 8.0
    return np.array([z0, z1, z2, z3, z4])


@pytest.mark.parametrize("name", ["clean", "neg_zero", "denormal"])
def test_pinned_applies(name):
    assert SUB_ILU("ilu0").sub_mode == 2
    a = _pinned_operator()
    s = R.Setup(a, [[2, 1, 0], [4, 3]], mode="ilu0")
    if name == "clean":
        z = s(np.array([2.0, 3.0, 1.0, 8.0, 4.0]))
        assert np.array_equal(z, _pinned_clean()) and z[0] == 1.0
    elif name == "neg_zero":                            # -0.0 - l * -0.0 and -0.0 / u stay -0.0 in the sweeps; the combine is 0.0 + x
        xs = s.products(np.full(5, -0.0))
        assert all(np.all(x == 0.0) and np.signbit(x).all() for x in xs)
        z = s(np.full(5, -0.0))
        assert np.all(z == 0.0) and not np.signbit(z).any()
    else:                                               # 5e-324 / 2 rounds to even: 0.0; -5e-324 / 3.5 is -0.0 before the combine
        with np.errstate(all="ignore"):
            z = s(np.array([5e-324, 0.0, 0.0, 0.0, -5e-324]))
        assert np.all(z == 0.0) and not np.signbit(z).any()
        z = s(np.array([1e-323, 0.0, 0.0, 0.0, 0.0]))   # 1e-323 / 2 = 5e-324 exactly; forward: y1 = 0 - (-0.5 * 1e-323) = 5e-324
        assert z[0] == 5e-324 and not np.isnan(z).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_input_stays_in_its_subdomain(mode, bad):
    """a poisoned row reaches the rows of its own subdomain only; the stored 0.0 couplings take no part in a sweep"""
    assert SUB_ILU(mode).sub_mode in (1, 2)
    a = _pinned_operator()
    s = R.Setup(a, [[0, 1, 2], [3, 4]], mode=mode)
    r = np.array([1.0, bad, 1.0, 8.0, 4.0])
    clean = s(np.array([1.0, 1.0, 1.0, 8.0, 4.0]))
    with np.errstate(all="ignore"):
        z = s(r)
    assert np.array_equal(z[3:], clean[3:]) and not np.isfinite(z[1])
    assert C.same_ieee(z, s.apply_loop(r))
    if mode == "ilu0" and np.isinf(bad):                # forward: y = (1, bad + .5, ...): the infinity keeps its sign down to z[1]
        assert z[1] == bad
