"""CG / PCG with x updated in batches of more than 8 iterations (cg_pcg.hip: XBatchOp, KRYST_CG_X_BATCH up to 32; DevState::alpha_hist holds 64 entries).

A batch of m iterations applies x = x + alpha_i p_i for i ascending in one pass, each the reference's un-fused multiply and add, so error codes,
iteration counts, residual histories and x must be the oracle's bits and those of the batch length 8 -- on 32^3 (T = 2) and 64^3 (T = 4) with the
marching fused form and the recompute residual pass forced, for m = 9, 16, 17 and 32: caps m - 1, m, m + 1 and 2 m + 1 (a full batch and the partial
one the flush owes each take the instance of their length, a single update the any-length instance); 70 iterations, where the ring of alphas has
wrapped; a tolerance that ends the solve inside a batch (updates beyond `xpend` must not be applied); sessions whose steps (5, m, 3) cut batches and
end inside one; convdiff (on which the oracle's CG takes no error exit) and the IndefiniteMatrix exit inside a batch on a shifted Poisson
operator; the knob changed between solves on one operator; Jacobi-PCG with 9 and 16; the unfused ring form with 16."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, "2"), (64, "4")]
MS = [9, 16, 17, 32]
OLD = 8                                                     # the longest batch before this change
WRAP = 70                                                   # iterations: beyond the 64 entries of the alpha ring
BASE = {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_MARCH": "1", "KRYST_CG_RECOMPUTE_AP": "1", "KRYST_SPMV_FUSE_SEG": "5"}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


_ops, _refs = {}, {}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def operator(ctx, N, kind):
    """(oracle operator, device operator, b, x0), made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d, O.splitmix64_uniform(0x51E9 + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows))
    return _ops[(N, kind)]


def reference(rs, N, kind, what, cap, tol=1e-30):
    """the oracle's solve, computed once and shared by every batch length"""
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


def batch(monkeypatch, m):
    monkeypatch.setenv("KRYST_CG_X_BATCH", str(m))


def both(rs, monkeypatch, N, kind, what, cls, pc, m, cap, tol=1e-30):
    """batch length m == the oracle == batch length 8 -> the oracle's result"""
    _, d, b, x0 = _ops[(N, kind)]
    ref = reference(rs, N, kind, what, cap, tol)
    got = {}
    for q in (OLD, m):
        batch(monkeypatch, q)
        got[q] = solve_dev(cls, tol, cap, d, pc, b, x0)
        check(ref, got[q], (N, kind, what, q, cap, tol))
    same(got[m], got[OLD], (N, kind, what, m, cap, tol))
    return ref


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_caps_around_a_batch(ctx, rs, N, T, m, monkeypatch):
    settings(monkeypatch, T)
    d = operator(ctx, N, "poisson")[1]
    info = d.fuse_march_info()
    assert info["eligible"] and info["on"] and info["recompute_ap"], info
    for cap in (m - 1, m, m + 1, 2 * m + 1):
        ref = both(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, m, cap)
        assert ref.code == 0 and ref.iterations == cap


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_alpha_ring_wraps(ctx, rs, N, T, m, monkeypatch):
    """70 iterations at a tolerance no iterate meets: iterations 65 .. 70 write the ring's entries of iterations 1 .. 6 again"""
    settings(monkeypatch, T)
    operator(ctx, N, "poisson")
    ref = both(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, m, WRAP)
    assert ref.code == 0 and ref.iterations == WRAP > 64


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_tolerance_ends_inside_a_batch(ctx, rs, N, T, m, monkeypatch):
    """the tolerance is the relative residual of iteration k, from the oracle's own history: k is the first iteration past the first batch, not
    the last of a batch, whose residual is below every earlier one (the history rises first: x0 is random), so the solve ends at k exactly"""
    settings(monkeypatch, T)
    operator(ctx, N, "poisson")
    cap = max(2 * m + 1, 40)
    h = np.asarray(reference(rs, N, "poisson", "cg", cap).history, dtype=float)
    k = next(k for k in range(m + 2, len(h)) if k % m != 0 and h[k] < h[:k].min())
    tol = float(h[k] / h[0]) * (1.0 + 1e-12)
    ref = both(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, m, cap, tol)
    assert ref.code == 0 and ref.converged and ref.iterations == k, (ref.iterations, k, m)


def session_dev(ctx, d, b, n, steps):
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for q in steps:
            sess.step(q)
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_session_steps_cut_batches(ctx, rs, N, T, m, monkeypatch):
    """steps of 5, m and 3 iterations: the second step crosses a batch's end, the session ends m + 8 iterations in, inside the second batch"""
    settings(monkeypatch, T)
    a, d, b, _ = operator(ctx, N, "poisson")
    steps = (5, m, 3)
    assert sum(steps) % m != 0
    ref = reference(rs, N, "poisson", "session", sum(steps))
    old = None
    for q in (OLD, m):
        batch(monkeypatch, q)
        its, h, x = session_dev(ctx, d, b, a.nrows, steps)
        assert its == sum(steps) == ref.iterations, (q, its)
        assert np.array_equal(bits(h), bits(ref.history)) and np.array_equal(bits(x), bits(ref.x)), (N, m, q)
        old = old or (its, h, x)
        assert np.array_equal(bits(x), bits(old[2]))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_convdiff(ctx, rs, N, T, m, monkeypatch):
    """the unsymmetric operator: the same code after the same number of iterations, whatever the batch length.  (Its symmetric part is positive
    definite, so the oracle's CG leaves through no error exit on it within 70 iterations; test_indefinite_exit has one that does.)"""
    settings(monkeypatch, T)
    operator(ctx, N, "convdiff")
    for cap in (m + 1, WRAP):
        both(rs, monkeypatch, N, "convdiff", "cg", K.CgSolver, None, m, cap)


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
    """IndefiniteMatrix after ten or more iterations, inside a batch: the updates that happened are applied by the flush, no later one; code,
    count and history against the oracle, x against the batch length 8"""
    settings(monkeypatch, T)
    shifted(ctx, N)
    ref = both(rs, monkeypatch, N, "shifted", "cg", K.CgSolver, None, m, 2 * m + 1)
    assert ref.code != 0 and ref.iterations > 8 and (ref.iterations - 1) % m != 0, (ref.code, ref.iterations)


@pytest.mark.parametrize("N,T", SHAPES)
def test_knob_changed_between_solves(ctx, rs, N, T, monkeypatch):
    """one operator, one context: 32, 9, 8, 17, 16 and 32 again, each solve the oracle's bits (the ring is sized per solve)"""
    settings(monkeypatch, T)
    _, d, b, x0 = operator(ctx, N, "poisson")
    cap = 35
    ref = reference(rs, N, "poisson", "cg", cap)
    for m in (32, 9, OLD, 17, 16, 32):
        batch(monkeypatch, m)
        check(ref, solve_dev(K.CgSolver, 1e-30, cap, d, None, b, x0), (N, "knob", m))


@pytest.mark.parametrize("m", [9, 16])
@pytest.mark.parametrize("N,T", SHAPES)
def test_jacobi_pcg(ctx, rs, N, T, m, monkeypatch):
    settings(monkeypatch, T)
    d = operator(ctx, N, "aniso")[1]
    pc = K.Jacobi().setup(d)
    for cap in (m - 1, m + 1, 2 * m + 1, WRAP):
        ref = both(rs, monkeypatch, N, "aniso", "pcg", K.PcgSolver, pc, m, cap)
        assert ref.code == 0 and ref.iterations == cap


@pytest.mark.parametrize("N,T", SHAPES)
def test_unfused_ring(ctx, rs, N, T, monkeypatch):
    """KRYST_CG_FUSE_P=0: the direction pass writes into the ring (CgDirectionRingOp) and x is paid in batches of 16"""
    settings(monkeypatch, T, KRYST_CG_FUSE_P="0")
    operator(ctx, N, "poisson")
    for cap in (15, 16, 17, 33, WRAP):
        ref = both(rs, monkeypatch, N, "poisson", "cg", K.CgSolver, None, 16, cap)
        assert ref.code == 0 and ref.iterations == cap
