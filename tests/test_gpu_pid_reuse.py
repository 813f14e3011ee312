"""The marching kernels keep row-pattern ids in registers where they repeat from plane to plane (KRYST_SPMV_PID_REUSE; csr_create.hip:
build_pid_same, spmv_fuse.hip: fuse_march, cg_recompute_residual_kernel).

An operator that can take the marching form holds one flag per tile: "all 512 ids are those of the tile one plane below".  Where it is set a
workgroup does not load the tile's ids again.  Nothing but a load changes, so error codes, iteration counts, residual histories and x must be
the oracle's bits and those of KRYST_SPMV_PID_REUSE=0 (no table: every plane loads): on 32^3 with T = 2 (one strip per plane) and 64^3 with
T = 2 and T = 4; for segments of 1 plane (the table is never consulted), 3 (a shorter last segment) and N; with and without a stored Ap; on
every way out of a solve (caps 1, 2, 3, 9, a stepping session with the knob flipped between its steps).  The flags themselves are counted
against the oracle's host arrays compared row by row, plane against plane: a box with constant coefficients repeats in planes 2 .. N - 2, one
changed row clears the flags of its tile and of the tile above (a compare of part of a tile, or with the wrong neighbour, shows there), and
coefficients that change with every plane clear them all."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, "2"), (64, "2"), (64, "4")]
KINDS = ["poisson", "aniso", "convdiff"]
CAPS = (1, 2, 3, 9)
STEPS = (2, 1, 5)
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


def same_tiles_of(a, N):
    """tiles of 512 rows, not in the first plane, whose rows all equal the row one plane below as sequences of (column - row, value bits): from
    the oracle's host arrays"""
    n, plane = a.nrows, N * N
    cnt = np.diff(a.row_ptr)
    assert n % 512 == 0 and plane % 512 == 0 and cnt.max() <= 7
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    pos = np.arange(len(a.col_idx), dtype=np.int64) - np.repeat(a.row_ptr[:-1], cnt)
    off = np.full((n, 7), np.iinfo(np.int64).min, dtype=np.int64)
    val = np.zeros((n, 7), dtype=np.uint64)
    off[rows, pos] = a.col_idx - rows
    val[rows, pos] = bits(a.vals)
    eq = np.zeros(n, dtype=bool)
    eq[plane:] = (cnt[plane:] == cnt[:-plane]) & (off[plane:] == off[:-plane]).all(axis=1) & (val[plane:] == val[:-plane]).all(axis=1)
    return int(eq.reshape(-1, 512).all(axis=1).sum())


def vectors(a, N):
    return O.splitmix64_uniform(0xD0E + N, a.nrows), O.splitmix64_uniform(0xABC, a.nrows)


def generated(ctx, N, kind):
    """(oracle operator, device operator from the stencil generator, b, x0), made once"""
    if (N, kind) not in _ops:
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        _ops[(N, kind)] = (a, d) + vectors(a, N)
    return _ops[(N, kind)]


def changed(ctx, N, name, bump):
    """Poisson on N^3 with bump (rows, amounts) added to those rows' diagonals, through CsrMatrix.from_csr; made once per name"""
    if (N, name) not in _ops:
        p = O.stencil7(N, "poisson")
        vals = p.vals.copy()
        rows, amounts = bump
        diag = p.row_ptr[rows] + 3                            # (rows interior in all three directions: six neighbours, the diagonal fourth)
        assert np.array_equal(p.col_idx[diag], rows)
        vals[diag] += amounts
        a = O.Csr(p.nrows, p.ncols, p.row_ptr, p.col_idx, vals)
        d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
        _ops[(N, name)] = (a, d) + vectors(a, N)
    return _ops[(N, name)]


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


def session_dev(ctx, d, b, n, monkeypatch, knobs):
    """a stepping session of STEPS; knobs: KRYST_SPMV_PID_REUSE's value for each step"""
    xs, bs = K.DeviceVec(ctx, np.zeros(n)), K.DeviceVec(ctx, b)
    with K.Session("cg", d, None, bs, xs, tol=1e-30, max_iters=1000) as sess:
        for i, q in enumerate(STEPS):
            monkeypatch.setenv("KRYST_SPMV_PID_REUSE", knobs[i])
            sess.step(q)
        st = sess.end()
    return st.iterations, np.array(sess.residual_history, dtype=float), xs.to_host()


def cg_solves(ctx, rs, key, op, monkeypatch, reuse, label):
    """CG to every cap and a stepping session (the knob flipped between its steps when reuse is on), each against the oracle -> the results"""
    a, d, b, x0 = op
    monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
    out = []
    for cap in CAPS:
        got = solve_dev(K.CgSolver, cap, d, None, b, x0)
        check(reference(rs, key, a, b, x0, "cg", cap), got, label + ("cg", cap))
        out.append(got)
    ref = reference(rs, key, a, b, x0, "session", sum(STEPS))
    if ref.code == 0:                                       # (a stepping session has no error path to compare: the kinds CG accepts)
        its, h, x = session_dev(ctx, d, b, a.nrows, monkeypatch, ("1", "0", "1") if reuse == "1" else ("0", "0", "0"))
        assert its == sum(STEPS) and np.array_equal(bits(h), bits(ref.history)) and np.array_equal(bits(x), bits(ref.x)), label + ("session",)
        out.append((0, its, h, x))
    monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
    return out


def on_against_off(ctx, rs, key, op, monkeypatch, label):
    """with and without a stored Ap: reuse on == the oracle == reuse off"""
    d = op[1]
    for recompute in ("1", "0"):
        monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", recompute)
        monkeypatch.setenv("KRYST_SPMV_PID_REUSE", "1")
        info = d.fuse_march_info()
        assert info["eligible"] and info["on"] and info["pid_reuse"] and info["recompute_ap"] == (recompute == "1"), info
        on = cg_solves(ctx, rs, key, op, monkeypatch, "1", label + (recompute, "reuse"))
        monkeypatch.setenv("KRYST_SPMV_PID_REUSE", "0")
        info = d.fuse_march_info()
        assert info["eligible"] and info["on"] and not info["pid_reuse"], info
        off = cg_solves(ctx, rs, key, op, monkeypatch, "0", label + (recompute, "reload"))
        assert len(on) == len(off)
        for i, (m, p) in enumerate(zip(on, off)):
            same(m, p, label + (recompute, i))


def settings(monkeypatch, N, T, seg):
    S = N if seg == "N" else int(seg)
    for k, v in {**BASE, "KRYST_SPMV_FUSE_T": T, "KRYST_SPMV_FUSE_SEG": str(S)}.items():
        monkeypatch.setenv(k, v)
    return S


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seg", ["1", "3", "N"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_generated_boxes(ctx, rs, N, T, seg, kind, monkeypatch):
    S = settings(monkeypatch, N, T, seg)
    op = generated(ctx, N, kind)
    info = op[1].fuse_march_info()
    assert info["T"] == int(T) and info["S"] == S, info
    P = N * N // 512
    # planes 2 .. N - 2 repeat the plane below; plane 1 lies above the box's first plane, plane N - 1 is its last
    assert info["tiles"] == N * P and info["pid_same_tiles"] == same_tiles_of(op[0], N) == (N - 3) * P, info
    on_against_off(ctx, rs, (N, kind), op, monkeypatch, (N, T, seg, kind))


@pytest.mark.parametrize("where", ["first-lane", "last-lane"])
@pytest.mark.parametrize("T", ["2", "4"])
def test_one_row_different(ctx, rs, T, where, monkeypatch):
    """64^3, the diagonal of one row interior in i, j and k raised by 1.0: in the first lane of a tile (its second row: the first one has i = 0),
    or in the last lane of a strip's last tile (i = 62, the last but one row of the strip)"""
    N, k0 = 64, 5
    settings(monkeypatch, N, T, "N")
    strip = int(T) * 512
    within = 512 + 1 if where == "first-lane" else strip - 2
    row = k0 * N * N + within                               # (the plane's first strip, past its first tile: j is interior at both places)
    i, j = row % N, (row // N) % N
    assert 1 <= i <= N - 2 and 1 <= j <= N - 2 and 2 <= k0 <= N - 3
    assert (within % 512) // 2 == (0 if where == "first-lane" else 255) and (where == "first-lane" or within // 512 == int(T) - 1)
    op = changed(ctx, N, ("row", row), (np.array([row]), np.array([1.0])))
    a, d = op[0], op[1]
    assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"] and d.fuse_march_info()["eligible"], (d.encoding(), d.pattern_info(), d.fuse_march_info())
    P = N * N // 512
    info = d.fuse_march_info()
    # the row's tile differs from the one below, and the tile above differs from the row's
    assert info["tiles"] == N * P and info["pid_same_tiles"] == same_tiles_of(a, N) == (N - 3) * P - 2, info
    on_against_off(ctx, rs, (N, "row", row), op, monkeypatch, (N, T, where))


@pytest.mark.parametrize("N,T", [(32, "2"), (64, "4")])
def test_ids_that_change_in_every_plane(ctx, rs, N, T, monkeypatch):
    """the diagonal of every row interior in i, j and k raised by float(k % 5): no two neighbouring planes are alike"""
    settings(monkeypatch, N, T, "N")
    r = np.arange(N ** 3, dtype=np.int64)
    i, j, k = r % N, (r // N) % N, r // (N * N)
    inner = (i >= 1) & (i <= N - 2) & (j >= 1) & (j <= N - 2) & (k >= 1) & (k <= N - 2)
    op = changed(ctx, N, "planes", (r[inner], (k[inner] % 5).astype(np.float64)))
    a, d = op[0], op[1]
    enc = d.encoding()
    assert enc[0] == "csr-p16" and 27 < enc[1] < 512 and d.pattern_info()["staged"] and d.fuse_march_info()["eligible"], (enc, d.pattern_info(), d.fuse_march_info())
    info = d.fuse_march_info()
    assert info["tiles"] == N ** 3 // 512 and info["pid_same_tiles"] == same_tiles_of(a, N) == 0, info
    on_against_off(ctx, rs, (N, "planes"), op, monkeypatch, (N, T, "planes"))


def test_segment_seams(ctx, rs, monkeypatch):
    """32^3: S = 1 (every plane is a segment's first plane and loads its ids: the table is never consulted) and S = 3 (ten segments and a shorter
    last one) against S = N"""
    N, T, kind = 32, "2", "convdiff"
    op = generated(ctx, N, kind)
    got = {}
    for seg in ("N", "1", "3"):
        settings(monkeypatch, N, T, seg)
        monkeypatch.setenv("KRYST_CG_RECOMPUTE_AP", "1")
        got[seg] = cg_solves(ctx, rs, (N, kind), op, monkeypatch, "1", (N, T, seg, kind, "seams"))
    for seg in ("1", "3"):
        assert len(got[seg]) == len(got["N"])
        for i, (m, p) in enumerate(zip(got[seg], got["N"])):
            same(m, p, (seg, i))


def test_jacobi_pcg(ctx, rs, monkeypatch):
    """64^3, T = 4: PCG's fused launch (both inner products, y stored) with the knob on == the oracle == the knob off"""
    N, kind = 64, "aniso"
    settings(monkeypatch, N, "4", "5")
    a, d, b, x0 = generated(ctx, N, kind)
    ref = reference(rs, (N, kind), a, b, x0, "pcg", 9)
    got = {}
    for reuse in ("1", "0"):
        monkeypatch.setenv("KRYST_SPMV_PID_REUSE", reuse)
        assert d.fuse_march_info()["pid_reuse"] == (reuse == "1")
        got[reuse] = solve_dev(K.PcgSolver, 9, d, K.Jacobi().setup(d), b, x0)
        check(ref, got[reuse], ("pcg", reuse))
    same(got["1"], got["0"], "pcg")


@pytest.mark.parametrize("N,env", [(40, {}), (16, {}), (64, {"KRYST_SPMV_FUSE_MARCH": "0"})], ids=["40", "16", "march0"])
def test_fallbacks(ctx, rs, N, env, monkeypatch):
    """what the marching form does not take reports no reuse and solves as before"""
    for k, v in {**BASE, "KRYST_SPMV_FUSE_T": "4", "KRYST_CG_RECOMPUTE_AP": "1", "KRYST_SPMV_PID_REUSE": "1", **env}.items():
        monkeypatch.setenv(k, v)
    a, d, b, x0 = generated(ctx, N, "poisson")
    info = d.fuse_march_info()
    assert not info["pid_reuse"], info
    if N != 64:
        assert info["tiles"] == 0 and info["pid_same_tiles"] == 0, info         # (a plane is no whole number of tiles: no table)
    for cap in (3, 9):
        check(reference(rs, (N, "poisson"), a, b, x0, "cg", cap), solve_dev(K.CgSolver, cap, d, None, b, x0), (N, tuple(env.items()), cap))
