"""The step of CG's recompute residual pass (spmv_fuse.hip: cg_recompute_residual_kernel): leg values from the kernel arguments
(KRYST_SPMV_LEG_VALUES).

On an operator whose every leg carries one value wherever a row pattern has it, the kernel multiplies by seven uniform kernel arguments and
keeps a row pair's presence masks in registers instead of looking a value up per entry.  A present entry multiplies by the same double, an
absent one is dropped by the same select, entry order, partials and mapping do not change: error codes, iteration counts, residual histories and
x must be the oracle's bits and those of the knob at its old value (0) -- on 32^3 with T = 2 and 64^3 with T = 2 and T = 4; for segments of 1, 2,
3, 4, 5 (a shorter last segment) and N planes; for the kinds poisson, aniso and convdiff (whose error exit stays) and for a Poisson operator with
one raised diagonal entry through from_csr (two bases: not eligible, the table look-ups stay); with and without a stored Ap (without: the plain
residual pass, which the knob must leave alone), KRYST_SPMV_PID_REUSE 0 and 1 (0: the mask word is formed at every plane), on every way out of a
solve (caps 1, 2, 3, 9, a stepping session with the knob flipped between its steps), and in Jacobi-PCG (both inner products, y stored).  The
eligibility flag and the seven values are checked against the oracle's host arrays: per leg, the set of value bit patterns over all rows that
have it.  (The fused kernel was measured with the same step and on three windows with one barrier per step; neither paid at 512^3 and neither is
in the tree -- profiles/march_step/ -- so there is one knob.)"""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, "2"), (64, "2"), (64, "4")]
KINDS = ["poisson", "aniso", "convdiff"]
SEGS = ["1", "2", "3", "4", "5", "N"]
CAPS = (1, 2, 3, 9)
STEPS = (2, 1, 5)
OLD = "0"                                                   # KRYST_SPMV_LEG_VALUES: the table look-ups, as before this step existed
KNOBS = [OLD, "1"]
BASE = {"KRYST_CG_FUSE_P": "1", "KRYST_SPMV_FUSE_MARCH": "1", "KRYST_CG_X_BATCH": "4"}


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


_ops, _refs = {}, {}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def leg_values_of(a, N):
    """(one value per leg?, the seven values) from the oracle's host arrays: per leg -- the entries at column - row = -N^2, -N, -1, 0, 1, N, N^2 --
    the set of value bit patterns over all rows that have it; +0.0 for a leg no row has"""
    rows = np.repeat(np.arange(a.nrows, dtype=np.int64), np.diff(a.row_ptr))
    off = a.col_idx.astype(np.int64) - rows
    legs = [-N * N, -N, -1, 0, 1, N, N * N]
    assert np.isin(off, legs).all()
    sets = [np.unique(bits(a.vals)[off == o]) for o in legs]
    ok = all(len(s) <= 1 for s in sets)
    vals = np.array([s[0] if len(s) == 1 else 0 for s in sets], dtype=np.uint64)
    return ok, (vals if ok else np.zeros(7, dtype=np.uint64))


def vectors(a, N):
    return O.splitmix64_uniform(0x51E9 + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows)


def generated(ctx, N, kind):
    """(oracle operator, device operator from the stencil generator, b, x0), made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d) + vectors(a, N)
    return _ops[(N, kind)]


def bumped(ctx, N):
    """Poisson on N^3 with 1.0 added to the diagonal of one row interior in i, j and k, through CsrMatrix.from_csr; made once"""
    if (N, "bumped") not in _ops:
        p = O.stencil7(N, "poisson")
        row = 5 * N * N + 512 + 1
        i, j = row % N, (row // N) % N
        assert 1 <= i <= N - 2 and 1 <= j <= N - 2
        vals = p.vals.copy()
        assert p.col_idx[p.row_ptr[row] + 3] == row
        vals[p.row_ptr[row] + 3] += 1.0
        a = O.Csr(p.nrows, p.ncols, p.row_ptr, p.col_idx, vals)
        d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
        _ops[(N, "bumped")] = (a, d) + vectors(a, N)
    return _ops[(N, "bumped")]


def reference(rs, key, a, b, x0, what, cap):
    """the oracle's solve, computed once per (operator, solve) and shared by every segment length and knob setting"""
    key = key + (what, cap)
    if key not in _refs:
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


def set_knobs(monkeypatch, knob):
    monkeypatch.setenv("KRYST_SPMV_LEG_VALUES", knob)


def session_dev(ctx, d, b, n, monkeypatch, knobs):
    """a stepping session of STEPS; knobs: the knob's value for each step"""
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for i, q in enumerate(STEPS):
            set_knobs(monkeypatch, knobs[i])
            sess.step(q)
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


def cg_solves(ctx, rs, key, op, monkeypatch, knob, label):
    """CG to every cap and a stepping session (the knob flipped between its steps when it is on), each against the oracle -> the results"""
    a, d, b, x0 = op
    set_knobs(monkeypatch, knob)
    out = []
    for cap in CAPS:
        got = solve_dev(K.CgSolver, cap, d, None, b, x0)
        check(reference(rs, key, a, b, x0, "cg", cap), got, label + ("cg", cap))
        out.append(got)
    ref = reference(rs, key, a, b, x0, "session", sum(STEPS))
    if ref.code == 0:                                       # (a stepping session has no error path to compare: the kinds CG accepts)
        flips = ("1", "0", "1") if knob != OLD else (OLD,) * len(STEPS)
        its, h, x = session_dev(ctx, d, b, a.nrows, monkeypatch, flips)
        assert its == sum(STEPS) and np.array_equal(bits(h), bits(ref.history)) and np.array_equal(bits(x), bits(ref.x)), label + ("session",)
        out.append((0, its, h, x))
    set_knobs(monkeypatch, knob)
    return out


def every_knob(ctx, rs, key, op, monkeypatch, label, eligible=True):
    """with and without a stored Ap, KRYST_SPMV_PID_REUSE 1 and 0: the knob on == the oracle == the knob off"""
    d = op[1]
    for recompute in ("1", "0"):
        monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", recompute)
        for reuse in ("1", "0"):
            monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
            old = None
            for knob in KNOBS:
                set_knobs(monkeypatch, knob)
                march, info = d.fuse_march_info(), d.leg_values_info()
                assert march["eligible"] and march["on"] and march["recompute_ap"] == (recompute == "1") and march["pid_reuse"] == (reuse == "1"), march
                assert info["eligible"] == eligible and info["on"] == (eligible and knob == "1" and recompute == "1"), (knob, info)
                got = cg_solves(ctx, rs, key, op, monkeypatch, knob, label + (recompute, reuse, knob))
                if old is None:
                    old = got
                assert len(got) == len(old)
                for i, (m, p) in enumerate(zip(got, old)):
                    same(m, p, label + (recompute, reuse, knob, i))


def settings(monkeypatch, N, T, seg):
    S = N if seg == "N" else int(seg)
    for k, v in {**BASE, "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_SEG": str(S)}.items():
        monkeypatch.setenv(k, v)
    return S


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("N,T", SHAPES)
def test_generated_boxes(ctx, rs, N, T, seg, kind, monkeypatch):
    S = settings(monkeypatch, N, T, seg)
    op = generated(ctx, N, kind)
    info = op[1].fuse_march_info()
    assert info["T"] == int(T) and info["S"] == S and info["segments"] == -(-N // S), info
    every_knob(ctx, rs, (N, kind), op, monkeypatch, (N, T, seg, kind))


@pytest.mark.parametrize("seg", ["3", "N"])
@pytest.mark.parametrize("T", ["2", "4"])
def test_one_row_different(ctx, rs, T, seg, monkeypatch):
    """64^3 Poisson through from_csr with one diagonal entry raised: leg 3 has two values, the operator is not eligible, the hook says so whatever
    the knob, and every setting solves through the table look-ups to the oracle's bits"""
    N = 64
    settings(monkeypatch, N, T, seg)
    op = bumped(ctx, N)
    d = op[1]
    assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"] and d.fuse_march_info()["eligible"], (d.encoding(), d.pattern_info(), d.fuse_march_info())
    every_knob(ctx, rs, (N, "bumped"), op, monkeypatch, (N, T, seg, "bumped"), eligible=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [32, 64])
def test_eligibility_and_values(ctx, N, kind, monkeypatch):
    """the flag and the seven values against the oracle's host arrays, for the stencil generator and for the same operator through from_csr"""
    settings(monkeypatch, N, "2", "N")
    set_knobs(monkeypatch, "1")
    monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", "1")
    a, d = generated(ctx, N, kind)[:2]
    ok, vals = leg_values_of(a, N)
    assert ok and len(np.unique(vals)) >= 2
    h = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
    for op in (d, h):
        info = op.leg_values_info()
        assert info["eligible"] and info["on"], info
        assert np.array_equal(bits(info["values"]), vals), (info, vals)
    monkeypatch.setenv("KRYST_SPMV_FUSE_MARCH", "0")
    info = d.leg_values_info()
    assert info["eligible"] and not info["on"], info


def test_one_changed_row_clears_the_flag(ctx, monkeypatch):
    N = 64
    settings(monkeypatch, N, "4", "N")
    set_knobs(monkeypatch, "1")
    monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", "1")
    a, d = bumped(ctx, N)[:2]
    ok, vals = leg_values_of(a, N)
    assert not ok
    info = d.leg_values_info()
    assert not info["eligible"] and not info["on"], info
    assert np.array_equal(bits(info["values"]), vals) and not vals.any(), info


def test_jacobi_pcg(ctx, rs, monkeypatch):
    """64^3, T = 4: PCG's fused launch (both inner products, y stored; no recompute residual pass), the knob on == the oracle == the knob off"""
    N, kind = 64, "aniso"
    settings(monkeypatch, N, "4", "5")
    a, d, b, x0 = generated(ctx, N, kind)
    ref = reference(rs, (N, kind), a, b, x0, "pcg", 9)
    pc = K.Jacobi().setup(d)
    for reuse in ("1", "0"):
        monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
        got = {}
        for knob in KNOBS:
            set_knobs(monkeypatch, knob)
            assert d.leg_values_info()["eligible"]
            got[knob] = solve_dev(K.PcgSolver, 9, d, pc, b, x0)
            check(ref, got[knob], ("pcg", reuse, knob))
            same(got[knob], got[OLD], ("pcg", reuse, knob))
