"""The marching mode of the fused direction + SpMV kernel of CG / PCG (spmv_fuse.hip: spmv_pattern_fuse_kernel<.., MARCH>).

A workgroup keeps a strip of 512 T rows of a grid plane and walks a segment of S planes; the operands one plane away come out of its own
LDS windows (below: the lane's own pair of the previous step, in registers; above: the next plane's window) and only the first and the last
plane of a segment form them from z and p_old in memory.  Which workgroup computes a tile changes and nothing else, so iteration counts,
residual histories and x must be the oracle's bits -- and the un-marched kernel's -- for every segment length: S = 1 (every far operand from
memory), 2, 3, 5 (a shorter last segment), N (one segment per strip) and 2 N (beyond the box); on 32^3 with T = 2 (one strip per plane:
every halo crosses a plane boundary) and 64^3 with T = 2 (4 strips) and T = 4 (2 strips); for `convdiff`, whose -k and +k coefficients
differ (a swapped lower / upper operand shows there and not on Poisson's operator); on every way out of a solve (caps 1, 2, 3, 9, a
stepping session), with x updated by the kernel (KRYST_CG_X_BATCH=1) and in batches (4).  Shapes the mode cannot take (40^3: a plane is no
whole number of strips; 16^3: a tile spans two planes) fall back to the un-marched kernel silently."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, "2"), (64, "2"), (64, "4")]
KINDS = ["poisson", "aniso", "convdiff"]
CAPS = (1, 2, 3, 9)
STEPS = (2, 1, 5)


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


_ops, _refs = {}, {}


def operator(ctx, N, kind):
    """(oracle operator, device operator, b, x0) of a grid and kind, made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d, O.splitmix64_uniform(0xD0E + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows))
    return _ops[(N, kind)]


def reference(ctx, rs, N, kind, what, cap):
    """the oracle's solve, computed once per (grid, kind, solve) and shared by every segment length and run length"""
    key = (N, kind, what, cap)
    if key not in _refs:
        a, _, b, x0 = operator(ctx, N, kind)
        if what == "cg":
            r = O.solve("cg", a, b, x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
        elif what == "pcg":
            r = O.solve("pcg", a, b, pc=O.Pc.jacobi(a), x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
        else:
            r = O.solve("cg", a, b, tol=1e-30, max_iters=cap, rs=rs, raise_on_error=False)
        _refs[key] = r
    return _refs[key]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def solve_dev(cls, cap, d, pc, b, x0):
    s = cls(1e-9, cap); x = x0.copy()
    try:
        st, code = s.solve(d, pc, b, x), 0
    except K.KError as e:                                   # (the unsymmetric operator: IndefiniteMatrix must match too)
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


def session_dev(ctx, d, b, n):
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for q in STEPS:
            sess.step(q)
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


def all_solves(ctx, rs, N, kind, monkeypatch, label):
    """every solve of the issue's list under the current KRYST_SPMV_FUSE_* settings, each against the oracle -> the results"""
    a, d, b, x0 = operator(ctx, N, kind)
    out = []
    for xbatch in ("1", "4"):
        monkeypatch.setenv("KRYST_CG_X_BATCH", xbatch)
        for cap in CAPS:
            got = solve_dev(K.CgSolver, cap, d, None, b, x0)
            check(reference(ctx, rs, N, kind, "cg", cap), got, label + ("cg", xbatch, cap))
            out.append(got)
        got = solve_dev(K.PcgSolver, 9, d, K.Jacobi().setup(d), b, x0)
        check(reference(ctx, rs, N, kind, "pcg", 9), got, label + ("pcg", xbatch, 9))
        out.append(got)
        ref = reference(ctx, rs, N, kind, "session", sum(STEPS))
        if ref.code == 0:                                   # (a stepping session has no error path to compare: the kinds CG accepts)
            its, h, x = session_dev(ctx, d, b, a.nrows)
            assert its == sum(STEPS) and np.array_equal(bits(h), bits(ref.history)) and np.array_equal(bits(x), bits(ref.x)), label + ("session", xbatch)
            out.append((0, its, h, x))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seg", ["1", "2", "3", "5", "N", "2N"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_marching_matches_the_oracle_and_the_unmarched_kernel(ctx, rs, N, T, seg, kind, monkeypatch):
    S = {"N": N, "2N": 2 * N}.get(seg) or int(seg)
    monkeypatch.setenv("KRYST_CG_FUSE_P", "1"); monkeypatch.setenv("KRYST_SPMV_FUSE_T", T); monkeypatch.setenv("KRYST_SPMV_FUSE_SEG", str(S))
    a, d, b, x0 = operator(ctx, N, kind)
    monkeypatch.setenv("KRYST_SPMV_FUSE_MARCH", "1")
    info = d.fuse_march_info()
    assert info["eligible"] and info["on"], info
    assert info["T"] == int(T) and info["strips"] == N * N // (512 * int(T)) and info["S"] == min(S, N) and info["segments"] == -(-N // min(S, N)), info
    marched = all_solves(ctx, rs, N, kind, monkeypatch, (N, T, seg, kind, "march"))
    monkeypatch.setenv("KRYST_SPMV_FUSE_MARCH", "0")
    assert d.fuse_march_info()["eligible"] and not d.fuse_march_info()["on"]
    plain = all_solves(ctx, rs, N, kind, monkeypatch, (N, T, seg, kind, "plain"))
    assert len(marched) == len(plain)
    for i, (m, p) in enumerate(zip(marched, plain)):
        same(m, p, (N, T, seg, kind, i))


@pytest.mark.parametrize("N,T", [(40, "4"), (40, "2"), (16, "2"), (16, "4")])
def test_ineligible_shapes_take_the_unmarched_kernel(ctx, rs, N, T, monkeypatch):
    monkeypatch.setenv("KRYST_CG_FUSE_P", "1"); monkeypatch.setenv("KRYST_SPMV_FUSE_T", T); monkeypatch.setenv("KRYST_SPMV_FUSE_MARCH", "1")
    a, d, b, x0 = operator(ctx, N, "poisson")
    info = d.fuse_march_info()
    assert not info["eligible"] and not info["on"], info
    for xbatch in ("1", "4"):
        monkeypatch.setenv("KRYST_CG_X_BATCH", xbatch)
        for cap in (3, 9):
            check(reference(ctx, rs, N, "poisson", "cg", cap), solve_dev(K.CgSolver, cap, d, None, b, x0), (N, T, xbatch, cap))


QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def pvec(ctx, data, poison):
    """`data` in a vector whose padding (the rest of the last tile and the extra tile) holds `poison`"""
    v = ctx.vec(np.asarray(data, dtype=np.float64))
    assert v.padding_dirty() == 0
    if poison is not None:
        v.poison_padding(poison)
        assert v.padding_dirty() == -(-len(v) // 512) * 512 + 512 - len(v)
    return v


@pytest.mark.parametrize("xbatch", ["1", "4"])
def test_poisoned_padding(ctx, rs, xbatch, monkeypatch):
    """64^3, T = 4: the first and the last strip's windows and the far operands of the box's first and last plane are clamped into the
    vectors' padding -- NaNs there must reach nothing"""
    N, T, kind = 64, "4", "aniso"
    for k, v in (("KRYST_CG_FUSE_P", "1"), ("KRYST_SPMV_FUSE_T", T), ("KRYST_SPMV_FUSE_SEG", "5"), ("KRYST_SPMV_FUSE_MARCH", "1"), ("KRYST_CG_X_BATCH", xbatch)):
        monkeypatch.setenv(k, v)
    a, d, b, x0 = operator(ctx, N, kind)
    assert d.fuse_march_info()["on"]
    ref = reference(ctx, rs, N, kind, "cg", 9)
    for poison in (None, QNAN, 1e300):
        bv, xv = pvec(ctx, b, poison), pvec(ctx, x0, poison)
        s = K.CgSolver(1e-9, 9)
        try:
            st, code = s.solve(d, None, bv, xv), 0
        except K.KError as e:
            st, code = e.stats, e.code
        x = xv.to_host()
        assert not np.isnan(x).any() and not np.isnan(np.array(s.residual_history, dtype=float)).any(), poison
        check(ref, (code, st.iterations, np.array(s.residual_history, dtype=float), x), ("padding", xbatch, poison))
