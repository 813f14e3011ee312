"""CG without a stored Ap (KRYST_CG_RECOMPUTE_AP; spmv_fuse.hip: cg_recompute_residual_kernel, spmv_pattern_fuse_kernel<.., MARCH, YS = false>).

In a fused iteration with x in batches the marching kernel stores p_new only, and the residual pass forms A p again from p_new -- the doubles
the fused kernel had in its windows, the same arithmetic -- before r -= alpha Ap and the (r, r) partials.  Nothing but the traffic changes, so
iteration counts, error codes, residual histories and x must be the oracle's bits, and those of the stored-Ap path (KRYST_CG_RECOMPUTE_AP=0):
on 32^3 with T = 2 (one strip per plane: every halo crosses a plane boundary) and 64^3 with T = 2 (4 strips) and T = 4 (2 strips); for segment
lengths 1 (every far operand from memory), 3 (a shorter last segment), N (one segment) and 2 N; for `convdiff`, whose -k and +k coefficients
differ (a swapped lower / upper operand shows there); on every way out of a solve (caps 1 and 2: the hand-over from the stored-Ap first
iteration to the first recompute iteration; 3, 9; a stepping session, whose step boundary lies between the two launches' iterations).  What
the form cannot take (x-batch length 1, 40^3, 16^3, marching off) keeps the stored-Ap path silently."""
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
    """the oracle's solve, computed once per (grid, kind, solve) and shared by every segment length, run length and knob setting"""
    key = (N, kind, what, cap)
    if key not in _refs:
        a, _, b, x0 = operator(ctx, N, kind)
        if what == "cg":
            r = O.solve("cg", a, b, x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
        else:
            r = O.solve("cg", a, b, tol=1e-30, max_iters=cap, rs=rs, raise_on_error=False)
        _refs[key] = r
    return _refs[key]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def solve_dev(cap, d, b, x0):
    s = K.CgSolver(1e-9, cap); x = x0.copy()
    try:
        st, code = s.solve(d, None, b, x), 0
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


def session_dev(ctx, d, b, n, monkeypatch=None, knobs=None):
    """a stepping session of STEPS; knobs: KRYST_CG_RECOMPUTE_AP's value for each step"""
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for i, q in enumerate(STEPS):
            if knobs:
                monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", knobs[i])
            sess.step(q)
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


def all_solves(ctx, rs, N, kind, label):
    """every solve of the list under the current settings, each against the oracle -> the results"""
    a, d, b, x0 = operator(ctx, N, kind)
    out = []
    for cap in CAPS:
        got = solve_dev(cap, d, b, x0)
        check(reference(ctx, rs, N, kind, "cg", cap), got, label + ("cg", cap))
        out.append(got)
    ref = reference(ctx, rs, N, kind, "session", sum(STEPS))
    if ref.code == 0:                                       # (a stepping session has no error path to compare: the kinds CG accepts)
        its, h, x = session_dev(ctx, d, b, a.nrows)
        assert its == sum(STEPS) and np.array_equal(bits(h), bits(ref.history)) and np.array_equal(bits(x), bits(ref.x)), label + ("session",)
        out.append((0, its, h, x))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seg", ["1", "3", "N", "2N"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_recompute_matches_the_oracle_and_the_stored_ap_path(ctx, rs, N, T, seg, kind, monkeypatch):
    S = {"N": N, "2N": 2 * N}.get(seg) or int(seg)
    for k, v in (("KRYST_CG_FUSE_P", "1"), ("KRYST_SPMV_FUSE_MARCH", "1"), ("KRYST_CG_X_BATCH", "4"), ("KRYST_SPMV_FUSE_T", T), ("KRYST_SPMV_FUSE_SEG", str(S))):
        monkeypatch.setenv(k, v)
    a, d, b, x0 = operator(ctx, N, kind)
    monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", "1")
    info = d.fuse_march_info()
    assert info["eligible"] and info["on"] and info["recompute_ap"], info
    assert info["T"] == int(T) and info["S"] == min(S, N), info
    on = all_solves(ctx, rs, N, kind, (N, T, seg, kind, "recompute"))
    monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", "0")
    info = d.fuse_march_info()
    assert info["eligible"] and info["on"] and not info["recompute_ap"], info
    off = all_solves(ctx, rs, N, kind, (N, T, seg, kind, "stored"))
    assert len(on) == len(off)
    for i, (m, p) in enumerate(zip(on, off)):
        same(m, p, (N, T, seg, kind, i))


@pytest.mark.parametrize("N,env", [(64, {"KRYST_CG_X_BATCH": "1"}), (40, {}), (16, {}), (64, {"KRYST_SPMV_FUSE_MARCH": "0"})],
                         ids=["xbatch1", "40", "16", "march0"])
def test_fallbacks_are_silent_and_exact(ctx, rs, N, env, monkeypatch):
    for k, v in {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_MARCH": "1", "KRYST_CG_X_BATCH": "4", "KRYST_SPMV_FUSE_T": "4", "KRYST_CG_RECOMPUTE_AP": "1", **env}.items():
        monkeypatch.setenv(k, v)
    a, d, b, x0 = operator(ctx, N, "poisson")
    assert not d.fuse_march_info()["recompute_ap"], d.fuse_march_info()
    for cap in (3, 9):
        check(reference(ctx, rs, N, "poisson", "cg", cap), solve_dev(cap, d, b, x0), (N, tuple(env.items()), cap))


QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def pvec(ctx, data, poison):
    """`data` in a vector whose padding (the rest of the last tile and the extra tile) holds `poison`"""
    v = ctx.vec(np.asarray(data, dtype=np.float64))
    assert v.padding_dirty() == 0
    if poison is not None:
        v.poison_padding(poison)
        assert v.padding_dirty() == -(-len(v) // 512) * 512 + 512 - len(v)
    return v


def test_poisoned_padding(ctx, rs, monkeypatch):
    """64^3, T = 4, S = 5: the first and the last strip's windows and the far pairs of the box's first and last plane are clamped into the
    vectors' padding -- only absent entries may point there, so NaNs and 1e300 there must reach nothing"""
    N, kind = 64, "aniso"
    for k, v in (("KRYST_CG_FUSE_P", "1"), ("KRYST_SPMV_FUSE_T", "4"), ("KRYST_SPMV_FUSE_SEG", "5"), ("KRYST_SPMV_FUSE_MARCH", "1"), ("KRYST_CG_X_BATCH", "4"),
                 ("KRYST_CG_RECOMPUTE_AP", "1")):
        monkeypatch.setenv(k, v)
    a, d, b, x0 = operator(ctx, N, kind)
    assert d.fuse_march_info()["recompute_ap"]
    ref = reference(ctx, rs, N, kind, "cg", 9)
    for poison in (QNAN, 1e300):
        bv, xv = pvec(ctx, b, poison), pvec(ctx, x0, poison)
        s = K.CgSolver(1e-9, 9)
        try:
            st, code = s.solve(d, None, bv, xv), 0
        except K.KError as e:
            st, code = e.stats, e.code
        x = xv.to_host()
        assert not np.isnan(x).any() and not np.isnan(np.array(s.residual_history, dtype=float)).any(), poison
        check(ref, (code, st.iterations, np.array(s.residual_history, dtype=float), x), ("padding", poison))


def test_knob_flipped_between_session_steps(ctx, rs, monkeypatch):
    """one session on 64^3, KRYST_CG_RECOMPUTE_AP 1 -> 0 -> 1 between its steps: the fused launch and the residual launch of an iteration always
    agree, so history and x are the oracle's"""
    N, kind = 64, "poisson"
    for k, v in (("KRYST_CG_FUSE_P", "1"), ("KRYST_SPMV_FUSE_T", "4"), ("KRYST_SPMV_FUSE_SEG", "3"), ("KRYST_SPMV_FUSE_MARCH", "1"), ("KRYST_CG_X_BATCH", "4")):
        monkeypatch.setenv(k, v)
    a, d, b, x0 = operator(ctx, N, kind)
    ref = reference(ctx, rs, N, kind, "session", sum(STEPS))
    assert ref.code == 0
    its, h, x = session_dev(ctx, d, b, a.nrows, monkeypatch, ("1", "0", "1"))
    assert its == sum(STEPS)
    assert np.array_equal(bits(h), bits(ref.history)), "history"
    assert np.array_equal(bits(x), bits(ref.x)), ("x", int(np.sum(bits(x) != bits(ref.x))))
