"""The windows of the marching CG kernels (spmv_fuse.hip: fuse_march, cg_recompute_residual_kernel; march_window.h): R + 2 n doubles from row r0 - n, a
lane's requests starting with the pairs of its own rows.

Which lane loads which window pair changes; per-element arithmetic, entry order, absent-entry selects and the per-tile partials do not: error codes,
iteration counts, residual histories and x must be the oracle's bits, and those of T = 2 and T = 4 the same --
  64^3 at T = 2 and T = 4: lines of 64 points (halo requests with n < 512: a fifth request that most lanes drop); at T = 4 two strips per plane;
  128^3 at T = 4: eight strips per plane, which share real halo lines; lines of 128 points;
  32^3 at T = 2: a strip is a whole plane, every halo line lies in a neighbouring plane;
for segments of 1, 2, 3, 5 (a shorter last segment) and N planes; the kinds poisson, aniso and convdiff (whose error exit stays); with and without a
stored Ap; KRYST_SPMV_PID_REUSE and KRYST_SPMV_LEG_VALUES 0 and 1; iteration caps 1, 2, 3 and 9; a stepping session with KRYST_SPMV_FUSE_T flipped
between its steps; Jacobi-PCG (both inner products, y stored); and b, x0 in vectors whose padding holds NaNs or 1e300 (the windows of a box's first
and last plane clamp at other addresses than before).

Strips of 8 tiles in workgroups of 512 threads (KRYST_SPMV_FUSE_T=8) were built, passed these cases at 64^3 and 128^3 and were measured slower than
T = 4 at every size (profiles/march_t8/), so they are not in the tree: the knob's value 8 means 4, as every value above 2 always has, and
test_t_above_4_means_4 holds that."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
KINDS = ["poisson", "aniso", "convdiff"]
SEGS = ["1", "2", "3", "5", "N"]
CAPS = (1, 2, 3, 9)
STEPS = (2, 1, 5)
BASE = {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_MARCH": "1", "KRYST_CG_X_BATCH": "4"}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


_ops, _refs, _other = {}, {}, {}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def operator(ctx, N, kind):
    """(oracle operator, device operator from the stencil generator, b, x0), made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d, O.splitmix64_uniform(0x51E9 + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows))
    return _ops[(N, kind)]


def reference(rs, N, kind, what, cap, ctx):
    """the oracle's solve, computed once per (operator, solve) and shared by every T, segment length and knob setting"""
    key = (N, kind, what, cap)
    if key not in _refs:
        a, _, b, x0 = operator(ctx, N, kind)
        if what == "cg":
            _refs[key] = O.solve("cg", a, b, x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
        elif what == "pcg":
            _refs[key] = O.solve("pcg", a, b, pc=O.Pc.jacobi(a), x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
        else:
            _refs[key] = O.solve("cg", a, b, tol=1e-30, max_iters=cap, rs=rs, raise_on_error=False)
    return _refs[key]


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


def settings(monkeypatch, N, T, seg, **more):
    S = N if seg == "N" else int(seg)
    for k, v in {**BASE, "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_SEG": str(S), **more}.items():
        monkeypatch.setenv(k, v)
    return S


def with_other_t(ctx, monkeypatch, N, kind, what, cap, T):
    """the device's result at the other KRYST_SPMV_FUSE_T (4 for 2, 2 for 4) with every other knob at its default, made once per solve"""
    other = "2" if T == "4" else "4"
    key = (N, kind, what, cap, other)
    if key not in _other:
        _, d, b, x0 = operator(ctx, N, kind)
        with monkeypatch.context() as m:
            for k in ("KRYST_CG_RECOMPUTE_AP", "KRYST_SPMV_PID_REUSE", "KRYST_SPMV_LEG_VALUES", "KRYST_SPMV_FUSE_SEG"):
                m.delenv(k, raising=False)
            m.setenv("KRYST_SPMV_FUSE_T", other)
            info = d.fuse_march_info()
            assert info["eligible"] and info["on"] and info["T"] == int(other), info
            if what == "cg":
                _other[key] = solve_dev(K.CgSolver, cap, d, None, b, x0)
            else:
                _other[key] = solve_dev(K.PcgSolver, cap, d, K.Jacobi().setup(d), b, x0)
    return _other[key]


def every_knob(ctx, rs, monkeypatch, N, T, kind, label):
    """with and without a stored Ap, KRYST_SPMV_PID_REUSE and KRYST_SPMV_LEG_VALUES 0 and 1, every cap: the oracle's bits and those of the other T"""
    _, d, b, x0 = operator(ctx, N, kind)
    for recompute in ("1", "0"):
        monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", recompute)
        for reuse in ("1", "0"):
            monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
            for leg in ("1", "0"):
                monkeypatch.setenv("KRYST_SPMV_LEG_VALUES", leg)
                info = d.fuse_march_info()
                assert info["eligible"] and info["on"] and info["T"] == int(T), info
                assert info["recompute_ap"] == (recompute == "1") and info["pid_reuse"] == (reuse == "1"), info
                for cap in CAPS:
                    got = solve_dev(K.CgSolver, cap, d, None, b, x0)
                    check(reference(rs, N, kind, "cg", cap, ctx), got, label + (recompute, reuse, leg, cap))
                    same(got, with_other_t(ctx, monkeypatch, N, kind, "cg", cap, T), label + (recompute, reuse, leg, cap, "other T"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("T", ["2", "4"])
def test_64(ctx, rs, T, seg, kind, monkeypatch):
    """64^3: lines of 64 points; four strips per plane at T = 2, two at T = 4"""
    N = 64
    S = settings(monkeypatch, N, T, seg)
    info = operator(ctx, N, kind)[1].fuse_march_info()
    assert info["strips"] == 8 // int(T) and info["S"] == S and info["segments"] == -(-N // S), info
    every_knob(ctx, rs, monkeypatch, N, T, kind, (N, T, seg, kind))


@pytest.mark.parametrize("seg,kind", [("1", "poisson"), ("2", "aniso"), ("3", "convdiff"), ("5", "poisson"), ("N", "aniso")])
def test_128_strips_share_halo_lines(ctx, rs, seg, kind, monkeypatch):
    """128^3 at T = 4: eight strips per plane, one per XCD; the lines between them are halo of one strip and own rows of the next"""
    N, T = 128, "4"
    S = settings(monkeypatch, N, T, seg)
    info = operator(ctx, N, kind)[1].fuse_march_info()
    assert info["strips"] == 8 and info["S"] == S and info["segments"] == -(-N // S), info
    every_knob(ctx, rs, monkeypatch, N, T, kind, (N, T, seg, kind))


@pytest.mark.parametrize("kind", ["poisson", "convdiff"])
def test_32_one_strip_per_plane(ctx, rs, kind, monkeypatch):
    """32^3 at T = 2: a plane is one strip, so both halo lines of every window lie in the neighbouring planes (or outside the box)"""
    N = 32
    settings(monkeypatch, N, "2", "3")
    _, d, b, x0 = operator(ctx, N, kind)
    info = d.fuse_march_info()
    assert info["T"] == 2 and info["eligible"] and info["on"] and info["strips"] == 1, info
    for recompute in ("1", "0"):
        monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", recompute)
        for cap in CAPS:
            check(reference(rs, N, kind, "cg", cap, ctx), solve_dev(K.CgSolver, cap, d, None, b, x0), (N, kind, recompute, cap))


def test_t_above_4_means_4(ctx, rs, monkeypatch):
    """KRYST_SPMV_FUSE_T=8: strips of 4 tiles, the same plan and the same bits as =4"""
    N, kind = 64, "aniso"
    settings(monkeypatch, N, "4", "5")
    _, d, b, x0 = operator(ctx, N, kind)
    four = d.fuse_march_info()
    monkeypatch.setenv("KRYST_SPMV_FUSE_T", "8")
    assert d.fuse_march_info() == four and four["T"] == 4, (four, d.fuse_march_info())
    check(reference(rs, N, kind, "cg", 9, ctx), solve_dev(K.CgSolver, 9, d, None, b, x0), (N, kind, "T=8"))


@pytest.mark.parametrize("flips", [("4", "2", "4"), ("2", "4", "2")])
@pytest.mark.parametrize("N,seg", [(64, "5"), (128, "3")])
def test_session_with_t_flipped(ctx, rs, N, seg, flips, monkeypatch):
    """a stepping session of 2 + 1 + 5 iterations, KRYST_SPMV_FUSE_T changed between its steps (the direction vector in memory is all they share)"""
    kind = "aniso"
    settings(monkeypatch, N, flips[0], seg)
    a, d, b, _ = operator(ctx, N, kind)
    ref = reference(rs, N, kind, "session", sum(STEPS), ctx)
    xs, bs = K.DeviceVec(ctx, np.zeros(a.nrows)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for T, q in zip(flips, STEPS):
            monkeypatch.setenv("KRYST_SPMV_FUSE_T", T)
            assert d.fuse_march_info()["T"] == int(T)
            sess.step(q)
        st = sess.end()
    assert st.iterations == sum(STEPS) and np.array_equal(bits(sess.residual_history), bits(ref.history)) and np.array_equal(bits(xs.to_host()), bits(ref.x))


@pytest.mark.parametrize("N,T,seg", [(64, "4", "5"), (64, "4", "N"), (128, "4", "3"), (64, "2", "3")])
def test_jacobi_pcg(ctx, rs, N, T, seg, monkeypatch):
    """PCG's fused launch (both inner products, y stored; no recompute residual pass), with the x update on the kernel (KRYST_CG_X_BATCH=1) and in batches"""
    kind = "aniso"
    settings(monkeypatch, N, T, seg)
    _, d, b, x0 = operator(ctx, N, kind)
    ref = reference(rs, N, kind, "pcg", 9, ctx)
    pc = K.Jacobi().setup(d)
    for batch in ("4", "1"):
        monkeypatch.setenv("KRYST_CG_X_BATCH", batch)
        for reuse in ("1", "0"):
            monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
            info = d.fuse_march_info()
            assert info["on"] and info["T"] == int(T), info
            got = solve_dev(K.PcgSolver, 9, d, pc, b, x0)
            check(ref, got, ("pcg", N, T, seg, batch, reuse))
            same(got, with_other_t(ctx, monkeypatch, N, kind, "pcg", 9, T), ("pcg", N, T, seg, batch, reuse, "other T"))


def pvec(ctx, data, poison):
    """`data` in a vector whose padding holds `poison`"""
    v = ctx.vec(np.asarray(data, dtype=np.float64))
    v.poison_padding(poison)
    assert v.padding_dirty() == -(-len(v) // 512) * 512 + 512 - len(v)
    return v


@pytest.mark.parametrize("poison", [QNAN, 1e300], ids=["qnan", "1e300"])
@pytest.mark.parametrize("N,T,seg", [(64, "4", "5"), (128, "4", "N"), (64, "2", "N"), (32, "2", "3")])
def test_poisoned_padding(ctx, rs, N, T, seg, poison, monkeypatch):
    """b and x0 in vectors whose padding is dirty (the work vectors inherit it through the padded copies): the window of a box's last plane reaches
    n elements into the padding, the one of its first plane is clamped at element 0"""
    kind = "poisson"
    settings(monkeypatch, N, T, seg)
    a, d, b, x0 = operator(ctx, N, kind)
    for name, cls, pc in (("cg", K.CgSolver, None), ("pcg", K.PcgSolver, K.Jacobi().setup(d))):
        for recompute in ("1", "0"):
            monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", recompute)
            ref = reference(rs, N, kind, name, 9, ctx)
            bv, xv = pvec(ctx, b, poison), pvec(ctx, x0, poison)
            s = cls(1e-9, 9)
            st = s.solve(d, pc, bv, xv)
            label = (name, N, T, seg, recompute)
            assert st.iterations == ref.iterations and bool(st.converged) == bool(ref.converged), label
            assert np.array_equal(bits(s.residual_history), bits(ref.history)), (label, "history")
            assert np.array_equal(bits(xv.to_host()), bits(ref.x)), (label, "x")
            assert np.array_equal(bits(bv.to_host()), bits(b)), (label, "the solve changed b")
