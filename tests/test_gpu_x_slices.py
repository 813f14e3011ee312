"""CG / PCG with the x updates of a batch paid in SLICES (cg_pcg.hip: DirectionVec, cg_logic.h: XSlices; KRYST_CG_X_SLICE = 1): with a batch length m
iteration `it` applies the updates its slice it % m of the rows still owes, the flush what every slice owes.  Per row that is x = x + alpha_i p_i for
i ascending, each applied once, so error code, iteration count, residual history and x must be the oracle's bits and those of the whole pass every
m-th iteration (KRYST_CG_X_SLICE = 0) -- with the marching fused form and the recompute residual pass forced, on 32^3 (T = 2) and 64^3 (T = 4), as
tests/test_gpu_x_batch_long.py does it.

m = 2, 3, 7, 8, 17, 32; caps 1, 2, m - 1, m, m + 1, 2 m + 1 and 70 (the ring of alphas has wrapped); a tolerance that ends the solve inside a round
of slices; the IndefiniteMatrix exit on the shifted Poisson operator; sessions stepped by 1, by 5 and by m that end inside a round (m = 2 and 3,
where a slice has the least slack before its ring slot is overwritten: 70 iterations one by one); a session with ctx.synchronize() between its
steps (the binding has no read of the history before end(): the history is what is compared first, then x); the knob changed between solves on one
operator; Jacobi-PCG with 7 and 16; the unfused ring form with 16; 16^3 (8 tiles) with m = 32, where most slices are empty; poisoned vector padding."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, "2"), (64, "4")]
MS = [2, 3, 7, 8, 17, 32]
MODES = ("0", "1")                                          # KRYST_CG_X_SLICE: the whole pass every m-th iteration; slices
WRAP = 70                                                   # iterations: beyond the 64 entries of the alpha ring
BASE = {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_MARCH": "1", "KRYST_CG_RECOMPUTE_AP": "1", "KRYST_SPMV_FUSE_SEG": "5"}
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


_ops, _refs = {}, {}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def operator(ctx, N, kind, staged=True):
    """(oracle operator, device operator, b, x0), made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx) if N % 4 == 0 else K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
        if staged:
            assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d, O.splitmix64_uniform(0x51E9 + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows))
    return _ops[(N, kind)]


def reference(rs, N, kind, what, cap, tol=1e-30):
    """the oracle's solve, computed once and shared by every batch length and mode"""
    key = (N, kind, what, cap, tol)
    if key not in _refs:
        a, _, b, x0 = _ops[(N, kind)]
        if what == "pcg":
            _refs[key] = O.solve("pcg", a, b, pc=O.Pc.jacobi(a), x0=x0, tol=tol, max_iters=cap, rs=rs, raise_on_error=False)
        elif what == "session":
            _refs[key] = O.solve("cg", a, b, tol=tol, max_iters=cap, rs=rs, raise_on_error=False)
        else:
            _refs[key] = O.solve("cg", a, b, x0=x0, tol=tol, max_iters=cap, rs=rs, raise_on_error=False)
    return _refs[key]


def solve_dev(cls, tol, cap, d, pc, b, x0):
    s = cls(tol, cap); x = x0.copy()
    try:
        st, code = s.solve(d, pc, b, x), 0
    except K.KError as e:
        st, code = e.stats, e.code
    return code, st.iterations, np.array(s.residual_history, dtype=float), x


def check(ref, got, label):
    code, its, h, x = got
    assert code == ref.code, (label, code, ref.code)
    assert its == ref.iterations, (label, its, ref.iterations)
    assert len(h) == len(ref.history), label
    if code == 0:
        assert np.array_equal(bits(h), bits(ref.history)), (label, "history")
        assert np.array_equal(bits(x), bits(ref.x)), (label, "x", int(np.sum(bits(x) != bits(ref.x))))


def same(a, b, label):
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3])), label


def settings(monkeypatch, T, **more):
    for k, v in {**BASE, "KRYST_SPMV_FUSE_T": T, **more}.items():
        monkeypatch.setenv(k, v)


def form(monkeypatch, m, mode):
    monkeypatch.setenv("KRYST_CG_X_BATCH", str(m)); monkeypatch.setenv("KRYST_CG_X_SLICE", mode)


def every_mode(rs, monkeypatch, N, kind, what, cls, pc, m, cap, tol=1e-30):
    """slices == the oracle == the whole pass -> the oracle's result"""
    _, d, b, x0 = _ops[(N, kind)]
    ref = reference(rs, N, kind, what, cap, tol)
    got = {}
    for mode in MODES:
        form(monkeypatch, m, mode)
        got[mode] = solve_dev(cls, tol, cap, d, pc, b, x0)
        check(ref, got[mode], (N, kind, what, m, mode, cap, tol))
    for mode in MODES[1:]:
        same(got[mode], got["0"], (N, kind, what, m, mode, cap, tol))
    return ref


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_caps_around_a_round(ctx, rs, N, T, m, monkeypatch):
    settings(monkeypatch, T)
    d = operator(ctx, N, "poisson")[1]
    info = d.fuse_march_info()
    assert info["eligible"] and info["on"] and info["recompute_ap"], info
    for cap in sorted({1, 2, m - 1, m, m + 1, 2 * m + 1, WRAP}):
        ref = every_mode(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, m, cap)
        assert ref.code == 0 and ref.iterations == cap


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_tolerance_ends_inside_a_round(ctx, rs, N, T, m, monkeypatch):
    """the tolerance is the relative residual of iteration k, from the oracle's own history: k is the first iteration past the first round, not
    the last of a round, whose residual is below every earlier one (the history rises first: x0 is random), so the solve ends at k exactly and the
    slices paid after it must not apply the updates of iterations that never happened"""
    settings(monkeypatch, T)
    operator(ctx, N, "poisson")
    cap = max(2 * m + 1, 40)
    h = np.asarray(reference(rs, N, "poisson", "cg", cap).history, dtype=float)
    k = next(k for k in range(m + 2, len(h)) if k % m != 0 and h[k] < h[:k].min())
    tol = float(h[k] / h[0]) * (1.0 + 1e-12)
    ref = every_mode(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, m, cap, tol)
    assert ref.code == 0 and ref.converged and ref.iterations == k, (ref.iterations, k, m)


SHIFT = {32: 0.04, 64: 0.02}        # Poisson - shift * I: (p, Ap) <= 0 in iteration 12 (32^3) / 11 (64^3) of the oracle's CG from these b, x0


def shifted(ctx, N):
    """Poisson on N^3 with SHIFT[N] taken off every diagonal entry, through CsrMatrix.from_csr: indefinite; made once"""
    if (N, "shifted") not in _ops:
        p = O.stencil7(N, "poisson")
        rows = np.repeat(np.arange(p.nrows, dtype=np.int64), np.diff(p.row_ptr))
        vals = p.vals.copy()
        vals[p.col_idx.astype(np.int64) == rows] -= SHIFT[N]
        a = O.Csr(p.nrows, p.ncols, p.row_ptr, p.col_idx, vals)
        d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"] and d.fuse_march_info()["eligible"]
        _ops[(N, "shifted")] = (a, d, O.splitmix64_uniform(0x51E9 + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows))
    return _ops[(N, "shifted")]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_indefinite_exit(ctx, rs, N, T, m, monkeypatch):
    """IndefiniteMatrix after ten or more iterations: the updates that happened are applied, by the slices paid before the exit and by the flush,
    no later one; code, count and history against the oracle, x against the whole pass"""
    settings(monkeypatch, T)
    shifted(ctx, N)
    ref = every_mode(rs, monkeypatch, N, "shifted", "cg", K.CgSolver, None, m, 40)
    assert ref.code != 0 and 8 < ref.iterations < 40, (ref.code, ref.iterations)


def session_dev(ctx, d, b, n, steps, cap=1000, sync=False):
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=cap) as sess:
        for q in steps:
            sess.step(q)
            if sync:
                ctx.synchronize()
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


def session_every_mode(ctx, rs, monkeypatch, N, m, steps, cap=1000, sync=False):
    a, d, b, _ = _ops[(N, "poisson")]
    total = min(sum(steps), cap)
    assert total % m != 0, (m, steps, cap)                      # the session ends inside a round
    ref = reference(rs, N, "poisson", "session", total)
    first = None
    for mode in MODES:
        form(monkeypatch, m, mode)
        its, h, x = session_dev(ctx, d, b, a.nrows, steps, cap, sync)
        assert its == total == ref.iterations, (m, mode, its)
        assert np.array_equal(bits(h), bits(ref.history)), (N, m, mode, steps[:3], "history")
        assert np.array_equal(bits(x), bits(ref.x)), (N, m, mode, steps[:3], "x")
        first = x if first is None else first
        assert np.array_equal(bits(x), bits(first))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_sessions_end_inside_a_round(ctx, rs, N, T, m, monkeypatch):
    """steps of 1 (m = 2 and 3: 71 of them, past the wrap of the alpha ring; otherwise m + 3), of 5, and of m cut by the iteration cap 2 m + 1"""
    settings(monkeypatch, T)
    operator(ctx, N, "poisson")
    ones = WRAP + 1 if m <= 3 else m + 3
    session_every_mode(ctx, rs, monkeypatch, N, m, (1,) * ones)
    fives = next(k for k in range(2, 2 * m + 4) if (5 * k) % m != 0 and 5 * k > m)
    session_every_mode(ctx, rs, monkeypatch, N, m, (5,) * fives)
    session_every_mode(ctx, rs, monkeypatch, N, m, (m, m, m), cap=2 * m + 1)


@pytest.mark.parametrize("m", [2, 3, 8, 32])
@pytest.mark.parametrize("N,T", SHAPES)
def test_session_synchronized_between_steps(ctx, rs, N, T, m, monkeypatch):
    """ctx.synchronize() after every step of 3 iterations; nothing reads x before end()"""
    settings(monkeypatch, T)
    operator(ctx, N, "poisson")
    session_every_mode(ctx, rs, monkeypatch, N, m, (3,) * 11 + (2,), sync=True)


@pytest.mark.parametrize("N,T", SHAPES)
def test_knob_changed_between_solves(ctx, rs, N, T, monkeypatch):
    """one operator, one context: the mode and the batch length change from solve to solve, each the oracle's bits"""
    settings(monkeypatch, T)
    _, d, b, x0 = operator(ctx, N, "poisson")
    cap = 35
    ref = reference(rs, N, "poisson", "cg", cap)
    for m, mode in ((32, "1"), (32, "0"), (3, "1"), (8, "0"), (17, "1"), (2, "1"), (32, "1")):
        form(monkeypatch, m, mode)
        check(ref, solve_dev(K.CgSolver, 1e-30, cap, d, None, b, x0), (N, "knob", m, mode))


@pytest.mark.parametrize("m", [7, 16])
@pytest.mark.parametrize("N,T", SHAPES)
def test_jacobi_pcg(ctx, rs, N, T, m, monkeypatch):
    settings(monkeypatch, T)
    d = operator(ctx, N, "aniso")[1]
    pc = K.Jacobi().setup(d)
    for cap in (m - 1, m + 1, 2 * m + 1, WRAP):
        ref = every_mode(rs, monkeypatch, N, "aniso", "pcg", K.PcgSolver, pc, m, cap)
        assert ref.code == 0 and ref.iterations == cap


@pytest.mark.parametrize("N,T", SHAPES)
def test_unfused_ring(ctx, rs, N, T, monkeypatch):
    """KRYST_CG_FUSE_P=0: the direction pass writes into the ring (CgDirectionRingOp) and x is paid in slices of a batch of 16"""
    settings(monkeypatch, T, KRYST_CG_FUSE_P="0")
    operator(ctx, N, "poisson")
    for cap in (15, 16, 17, 33, WRAP):
        ref = every_mode(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, 16, cap)
        assert ref.code == 0 and ref.iterations == cap


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_most_slices_empty(ctx, rs, fuse, monkeypatch):
    """16^3 has 8 tiles: with m = 32 twenty-four of the slices are empty and launch nothing, the other eight hold one tile each"""
    monkeypatch.setenv("KRYST_CG_FUSE_P", fuse); monkeypatch.setenv("KRYST_SPMV_FUSE_T", "2")
    operator(ctx, 16, "poisson")
    assert _ops[(16, "poisson")][0].nrows == 8 * 512
    for cap in (1, 5, 31, 32, 33, WRAP):
        ref = every_mode(rs, monkeypatch, 16, "poisson", "cg", K.CgSolver, None, 32, cap)
        assert ref.code == 0 and ref.iterations == cap


def pvec(ctx, data, poison):
    """`data` in a vector whose padding holds `poison` (None: a clean vector)"""
    v = ctx.vec(np.asarray(data, dtype=np.float64))
    if poison is not None:
        v.poison_padding(poison)
        assert v.padding_dirty() == -(-len(v) // 512) * 512 + 512 - len(v)
    return v


@pytest.mark.parametrize("poison", [QNAN, 1e300], ids=["qnan", "1e300"])
@pytest.mark.parametrize("m", [3, 8])
@pytest.mark.parametrize("N,kind", [(16, "poisson"), (10, "aniso")])
def test_poisoned_padding(ctx, rs, N, kind, m, poison, monkeypatch):
    """b and x0 in vectors whose padding is dirty (the work vectors and the ring inherit it through the padded copies); 10^3 ends inside a tile"""
    monkeypatch.setenv("KRYST_CG_FUSE_P", "1"); monkeypatch.setenv("KRYST_SPMV_FUSE_T", "2")
    a, d, b, x0 = operator(ctx, N, kind)
    for name, cls, opc, kpc in (("cg", K.CgSolver, None, None), ("pcg", K.PcgSolver, O.Pc.jacobi(a), K.Jacobi().setup(d))):
        for cap in (m + 2, 400):
            key = (N, kind, "pad-" + name, cap)
            if key not in _refs:
                _refs[key] = O.solve(name, a, b, pc=opc, x0=x0, tol=1e-9, max_iters=cap, rs=rs)
            ref = _refs[key]
            for mode in MODES:
                form(monkeypatch, m, mode)
                for p in (None, poison):
                    bv, xv = pvec(ctx, b, p), pvec(ctx, x0, p)
                    s = cls(1e-9, cap)
                    st = s.solve(d, kpc, bv, xv)
                    label = (name, N, m, mode, cap, "clean" if p is None else "poisoned")
                    assert st.iterations == ref.iterations and bool(st.converged) == bool(ref.converged), label
                    assert np.array_equal(bits(s.residual_history), bits(ref.history)), (label, "history")
                    assert np.array_equal(bits(xv.to_host()), bits(ref.x)), (label, "x")
                    assert np.array_equal(bits(bv.to_host()), bits(b)), (label, "the solve changed b")
