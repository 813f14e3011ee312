"""SOR / SSOR without a GPU: the reference's own tests (tests/preconditioner_sor.rs) on the restatement tests/sor_ref.py, the level-by-level
form against the literal loops bit for bit, the coloured order against its definition, the host colouring (kryst_host_color_graph)
against coloring.rs as written, and the public surface."""
import itertools
import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import sor_ref as S

FLAGS = {"lower": S.APPLY_LOWER, "upper": S.APPLY_UPPER, "symmetric": S.SYMMETRIC_SWEEP}


def random_sparse(n, seed, density=0.06):
    """unsymmetric, some rows without off-diagonal entries, negative and tiny values, a stored diagonal everywhere but sign-mixed"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) * (rng.random((n, n)) < density)
    m[rng.random((n, n)) < 0.01] = 1e-300
    m[rng.random((n, n)) < 0.01] = -3e-17
    lone = rng.choice(n, max(n // 10, 1), replace=False)
    m[lone, :] = 0.0
    np.fill_diagonal(m, rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 4.0, n))
    return O.Csr.from_dense(m, keep_zeros=False)


# ------------------------------------------------------------------------------------------------ tests/preconditioner_sor.rs
def test_reference_identity():
    d = np.eye(5)
    x = np.ones(5)
    y = S.apply_loop(d, S.setup(d), x, 1.0, 1, S.APPLY_LOWER)
    assert np.array_equal(y, x)
    a = O.Csr.from_dense(d, keep_zeros=False)
    assert np.array_equal(S.apply_levels(a, x, 1.0, 1, S.APPLY_LOWER), x)


def test_reference_tridiag_forward():
    """preconditioner_sor.rs:61-81.  Their bound is 1e-12; the restatement meets it, and is exact wherever (x + l + r) / 4 and
    (x - (-l - r)) * 0.25 round alike -- they do here: a sum and its negation round to the same magnitude, and / 4 and * 0.25 are both exact
    scalings."""
    d = O.tridiag(5, -1.0, 4.0, -1.0)
    a = O.Csr.from_dense(d, keep_zeros=False)
    x = np.ones(5)
    y = S.apply_loop(d, S.setup(d), x, 1.0, 1, S.APPLY_LOWER)
    expected = np.zeros(5)
    for i in range(5):
        left = expected[i - 1] if i > 0 else 0.0
        right = x[i + 1] if i + 1 < 5 else 0.0
        expected[i] = (x[i] + left + right) / 4.0
    assert np.all(np.abs(y - expected) < 1e-12)
    assert np.array_equal(y, expected)
    assert np.array_equal(S.apply_levels(a, x, 1.0, 1, S.APPLY_LOWER), y)


def test_reference_ssor_finite_and_display():
    d = O.tridiag(5, -1.0, 4.0, -1.0)
    y = S.apply_loop(d, S.setup(d), np.ones(5), 1.0, 1, S.SYMMETRIC_SWEEP)
    assert np.all(np.isfinite(y))
    s = str(K.Sor(1.5, 2, 1, K.MatSorType.APPLY_LOWER, 0.1))
    assert s.startswith("SOR(omega=1.5, its=2, lits=1, ") and "SOR(omega=1.5" in s
    assert s == "SOR(omega=1.5, its=2, lits=1, sym=MatSorType(APPLY_LOWER), fshift=0.1)"
    assert str(K.Sor(1.0, 1, 1, K.MatSorType.SYMMETRIC_SWEEP | K.MatSorType.EISENSTAT, 0.0)) == \
        "SOR(omega=1, its=1, lits=1, sym=MatSorType(APPLY_LOWER | APPLY_UPPER | EISENSTAT), fshift=0)"


def test_zero_pivot_with_and_without_shift():
    d = np.diag([2.0, 0.0, 3.0, 0.0])
    d[1, 0] = 1.0
    with pytest.raises(S.ZeroPivot) as e:
        S.setup(d)
    assert e.value.row == 1
    assert np.array_equal(S.setup(d, 0.5), [1.0 / 2.5, 2.0, 1.0 / 3.5, 2.0])
    with pytest.raises(S.ZeroPivot) as e:
        S.setup(d, -3.0)
    assert e.value.row == 2
    a = O.Csr.from_dense(d, keep_zeros=False)                  # rows 1 and 3 have no stored diagonal
    with pytest.raises(S.ZeroPivot) as e:
        S.Plan(a)
    assert e.value.row == 1
    assert np.array_equal(S.Plan(a, 0.5).inv, S.setup(d, 0.5))


# ------------------------------------------------------------------------------------------------ (b) == (a)
CASES = list(itertools.product(FLAGS, (False, True), (0, 1, 3), (1.0, 1.5, 0.3)))


def _all_cases(a, seed, colors=None):
    d = S.dense(a)
    x = np.random.default_rng(seed).standard_normal(a.nrows)
    x[::7] = -0.0
    plans = {e: S.Plan(a, 0.0, colors, e) for e in (False, True)}
    for flag, eis, its, omega in CASES:
        sym = FLAGS[flag] | (S.EISENSTAT if eis else 0) | S.LOCAL_SYMMETRIC_SWEEP      # the LOCAL_* bits change nothing
        got = plans[eis].apply(x, omega, its, sym)
        want = S.apply_loop(d, S.setup(d), x, omega, its, sym) if colors is None else S.apply_permuted(d, x, colors, omega, its, sym)
        assert np.array_equal(got, want), (flag, eis, its, omega)
        if its == 0:
            assert np.all(got == 0.0) and not np.signbit(got).any()


@pytest.mark.parametrize("n,seed", [(1, 0), (37, 1), (120, 2), (200, 3)])
def test_levels_equal_loops_random(n, seed):
    _all_cases(random_sparse(n, seed), seed)


@pytest.mark.parametrize("kind", ["poisson", "varcoef"])
def test_levels_equal_loops_stencil(kind):
    a = O.stencil7(6, kind)
    _all_cases(a, 6)
    p = S.Plan(a)
    assert p.passes(True) == p.passes(False) == 3 * 6 - 2


def test_no_sweep_bits_give_zero():
    a = random_sparse(30, 9)
    x = np.random.default_rng(9).standard_normal(30)
    for sym in (0, S.EISENSTAT, S.LOCAL_SYMMETRIC_SWEEP | S.ZERO_INITIAL_GUESS):
        y = S.apply_levels(a, x, 1.3, 2, sym)
        assert np.array_equal(y, S.apply_loop(S.dense(a), S.setup(S.dense(a)), x, 1.3, 2, sym)) and np.all(y == 0.0)


# ------------------------------------------------------------------------------------------------ the coloured order
def test_one_colour_is_the_order_as_written():
    a = random_sparse(90, 11)
    d = S.dense(a)
    x = np.random.default_rng(11).standard_normal(90)
    for flag, eis, its, omega in CASES:
        sym = FLAGS[flag] | (S.EISENSTAT if eis else 0)
        want = S.apply_loop(d, S.setup(d), x, omega, its, sym)
        assert np.array_equal(S.apply_levels(a, x, omega, its, sym, colors=np.zeros(90, dtype=int)), want)
        assert np.array_equal(S.apply_permuted(d, x, np.full(90, 4), omega, its, sym), want)


@pytest.mark.parametrize("n,seed", [(60, 21), (150, 22)])
def test_random_colours_equal_the_permuted_loops(n, seed):
    a = random_sparse(n, seed)
    _all_cases(a, seed, colors=np.random.default_rng(seed).integers(0, 5, n))


def test_red_black_needs_one_pass_per_colour():
    N = 6
    a = O.stencil7(N, "poisson")
    r = np.arange(N ** 3)
    rb = (r % N + (r // N) % N + r // (N * N)) % 2
    _all_cases(a, 5, colors=rb)
    p = S.Plan(a, colors=rb)
    assert p.passes(True) == p.passes(False) == 2
    c2 = S.color_graph_csr(a)                                   # the distance-2 colouring: more colours, still one pass per colour at most
    p2 = S.Plan(a, colors=c2)
    assert 7 <= int(c2.max()) + 1 and p2.passes(True) <= int(c2.max()) + 1 and p2.passes(False) <= int(c2.max()) + 1


# ------------------------------------------------------------------------------------------------ colouring
def _distance2_ok(a, colors):
    n = a.nrows
    st = S.dense(a) != 0.0
    adj = (st | st.T) & ~np.eye(n, dtype=bool)
    two = adj | ((adj.astype(int) @ adj.astype(int)) > 0)
    np.fill_diagonal(two, False)
    i, j = np.nonzero(two)
    return bool(np.all(colors[i] != colors[j]))


@pytest.mark.parametrize("n,seed", [(1, 0), (40, 31), (200, 32)])
def test_color_graph_random(n, seed):
    a = random_sparse(n, seed, density=0.03)
    want = S.color_graph_csr(a)
    got = K.color_graph(a)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(K.color_graph((a.row_ptr, a.col_idx)), want)
    assert _distance2_ok(a, got)
    blocks = K.build_blocks_from_colors(got)
    assert blocks == S.build_blocks_from_colors([int(c) for c in want])
    assert sorted(i for b in blocks for i in b) == list(range(n)) and all(b == sorted(b) and len(b) > 0 for b in blocks)


def test_color_graph_stencil():
    a = O.stencil7(5, "poisson")
    got = K.color_graph(a)
    assert np.array_equal(got, S.color_graph_csr(a)) and _distance2_ok(a, got)
    assert int(got.max()) + 1 >= 7                              # a row and its six neighbours are pairwise within distance 2
    assert K.build_blocks_from_colors([]) == []
    with pytest.raises(K.KError) as e:
        K.color_graph((np.array([0, 1]), np.array([3])))
    assert e.value.code == 102


# ------------------------------------------------------------------------------------------------ the public surface
def test_public_surface():
    for name in ("Sor", "MatSorType", "color_graph", "build_blocks_from_colors"):
        assert name in K.__all__ and hasattr(K, name)
    for sym in ("kryst_pc_sor", "kryst_pc_sor_info", "kryst_host_color_graph"):
        assert sym in _ffi.SIGNATURES and hasattr(K.lib(), sym)
    T = K.MatSorType
    assert (int(T.ZERO_INITIAL_GUESS), int(T.APPLY_LOWER), int(T.APPLY_UPPER), int(T.SYMMETRIC_SWEEP), int(T.LOCAL_FORWARD_SWEEP),
            int(T.LOCAL_BACKWARD_SWEEP), int(T.LOCAL_SYMMETRIC_SWEEP), int(T.EISENSTAT)) == (1, 2, 4, 6, 8, 16, 24, 32)
    s = K.Sor(1.5, 2, 1, T.APPLY_LOWER, 0.1)
    assert (s.omega(), s.its(), s.lits(), s.sym(), s.fshift()) == (1.5, 2, 1, T.APPLY_LOWER, 0.1)
    s.set_omega(0.7); s.set_its(3); s.set_lits(4); s.set_sym(T.SYMMETRIC_SWEEP | T.EISENSTAT); s.set_fshift(0.0)
    assert (s.omega(), s.its(), s.lits(), s.sym(), s.fshift()) == (0.7, 3, 4, T.SYMMETRIC_SWEEP | T.EISENSTAT, 0.0)
    assert s.with_colors([0, 1, 0]) is s and list(s.colors) == [0, 1, 0]
    with pytest.raises(K.KError) as e:
        s.apply(np.ones(3))
    assert e.value.code == 2                                    # used before setup
    p = K.PC.Ssor()
    assert p.kind == "Ssor" and p.params == {"omega": 1.0, "its": 1}
    m = K.PC.Multicolor([0, 1])
    assert m.kind == "Multicolor" and list(m.params["colors"]) == [0, 1]
    for bare in (K.PC("Ssor"), K.PC("Multicolor"), K.PC("Multicolor", colors=[0, 1])):
        with pytest.raises(K.KError) as e:
            bare.build(None)                                    # raises before it touches the operator
        assert e.value.code == 6


def test_cpp_mirror_and_rust_binding_name_the_type():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hpp = open(os.path.join(root, "include", "kryst_hip.hpp")).read()
    rs = open(os.path.join(root, "bindings", "rust", "src", "lib.rs")).read() + open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    for text in (hpp, rs):
        assert "kryst_pc_sor" in text and "Sor" in text and "EISENSTAT" in text and "SYMMETRIC_SWEEP" in text


# ------------------------------------------------------------------------------------------------ the solver restatements of the GPU tier
@pytest.mark.parametrize("kind", ["varcoef", "convdiff"])
def test_krylov_pc_ref_equals_the_c_oracle_with_jacobi(kind):
    """tests/krylov_pc_ref.py (GMRES left / right and right-preconditioned BiCGStab with the preconditioner as a callable) against the C
    oracle with Jacobi, in the device's reduction order, bit for bit: converging runs and runs cut off after restarts"""
    import krylov_pc_ref as KR
    a = O.stencil7(7, kind)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    t, v, f = K.reduce_spec()
    rs = O.Reduce.tiled(t, v, f)
    pc = O.Pc.jacobi(a)
    for side, oside in (("left", O.SIDE_LEFT), ("right", O.SIDE_RIGHT)):
        for restart, tol, mx in ((30, 1e-10, 200), (5, 1e-14, 13)):
            ref = O.solve("gmres", a, b, pc=pc, tol=tol, max_iters=mx, restart=restart, side=oside, rs=rs, raise_on_error=False)
            x, it, fr, conv, hist = KR.gmres(a, pc.apply, side, b, restart, tol, mx, rs)
            assert (it, fr, conv) == (ref.iterations, ref.final_residual, ref.converged) and it > 3, (side, restart)
            assert np.array_equal(hist, ref.history) and np.array_equal(x, ref.x)
    for tol, mx in ((1e-9, 200), (1e-30, 7)):
        ref = O.solve("bicgstab_rpc", a, b, pc=pc, tol=tol, max_iters=mx, rs=rs, raise_on_error=False)
        x, it, fr, conv, hist = KR.bicgstab_rpc(a, pc.apply, b, tol, mx, rs)
        assert (it, fr, conv) == (ref.iterations, ref.final_residual, ref.converged) and it > 3
        assert np.array_equal(hist, ref.history) and np.array_equal(x, ref.x)
