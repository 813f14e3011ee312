"""The fp32-stored SpMV, CG, PCG and refinement on the row-pattern (CSR-P16) lowering, against the numpy restatement of the contract
(tests/mixed_ref.py, which is blind to the encoding) and against the same call on the plain-lowered operator.  The rule of
tests/test_gpu_mixed.py holds: integer views, bit for bit, no tolerance; where a NaN can arise (non-finite operands or stored values)
the comparison with the RESTATEMENT is `nonfinite_cases.same_ieee` -- sign and payload of a NaN made by inf - inf differ between host and
device -- while the comparison with the plain-lowered operator stays bit for bit.  Every product goes into a NaN-filled y.

Every case runs under the settings of mixed_pattern_cases.SETTINGS -- the default, KRYST_SPMV32_STAGE=0, KRYST_SPMV32_FORM=plain -- and,
where the staged kernel applies, with runs of one tile instead of two (KRYST_SPMV32_STAGE_T=1); `encoding()` is asserted first, so that no case passes
because another kernel ran.  Fixtures: tests/mixed_pattern_cases.py (their properties: tests/test_mixed_pattern_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import mixed_cases as MC
import mixed_pattern_cases as P
import mixed_ref as R
from nonfinite_cases import same_ieee

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
b32, b64 = MC.bits32, MC.bits64
UNPRE, PRE = K.CgNormType.Unpreconditioned, K.CgNormType.Preconditioned
UNSUPPORTED, ERR_ARG = 6, 102
POISONS32 = [None, np.float32(3e38)]               # the quiet NaN 0x7FC00000, and a finite value
KNOBS = ("KRYST_SPMV32_FORM", "KRYST_SPMV32_STAGE", "KRYST_SPMV32_STAGE_T")
SETTINGS = dict(P.SETTINGS, **{"stage-t1": {"KRYST_SPMV32_STAGE_T": "1"}})


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec32() == R.SPEC32
    return K.Context(0)


class Case:
    """an operator on the host, its restatement, the device operator and both lowerings -- made once per module"""
    def __init__(self, ctx, a, default):
        self.a, self.default, self.ref = a, default, R.Lowered(a)
        self.d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
        self.plain, self.pattern = self.d.lower(), self.d.lower("pattern")
        self.memo = {}

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]


_cases = {}


def case(ctx, name):
    if name not in _cases:
        make, default = P.OPERATORS[name]
        _cases[name] = Case(ctx, make(), default)
    return _cases[name]


def settings_of(c):
    return [s for s in SETTINGS if s != "stage-t1" or c.default == "pattern-stage"]


def enter(monkeypatch, c, setting):
    """switch to `setting` and make sure the kernel under test is the one that runs"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    want = c.default if setting == "stage-t1" else P.expected_kernel(c.default, setting)
    assert c.pattern.encoding() == want, (setting, c.pattern.encoding(), want)
    assert c.plain.encoding() == "plain"


def same32(a, b):
    return a.shape == b.shape and np.array_equal(b32(a), b32(b))


def same64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(b64(a), b64(b))


def nan_filled(ctx, n):
    return K.DeviceVec32(ctx, np.full(n, np.nan, np.float32))


def poisoned32(v, value):
    n = len(v)
    assert v.padding_dirty() == 0
    v.poison_padding(value)
    assert v.padding_dirty() == -(-n // 1024) * 1024 + 1024 - n, (n, v.padding_dirty())
    return v


def product(ctx, d32, x, nrows):
    y = nan_filled(ctx, nrows)
    d32.spmv(K.DeviceVec32(ctx, x), y)
    assert y.padding_dirty() == 0                                               # nothing behind the last row
    return y.to_host()


def run32(solver, d32, pc, b, x0, same_vector=False):
    """-> (code, stats, history, x after the call)"""
    ctx = d32.ctx
    bv = K.DeviceVec32(ctx, b)
    xv = bv if same_vector else K.DeviceVec32(ctx, x0)
    solver.clear_history()
    try:
        stats, code = solver.solve(d32, pc, bv, xv), 0
    except K.KError as e:
        if e.stats is None:
            raise
        stats, code = e.stats, e.code
    return code, stats, list(solver.residual_history), xv.to_host()


def assert_solve(got, ref, what, nan_can_arise=False):
    code, stats, hist, x = got
    assert code == ref.code, (what, code, ref.code)
    assert (stats.iterations, stats.converged) == (ref.iterations, ref.converged), (what, stats, ref.iterations, ref.converged)
    eq64, eq32 = (same_ieee, same_ieee) if nan_can_arise else (same64, same32)
    assert eq64([stats.final_residual], [ref.final_residual]), (what, stats.final_residual, ref.final_residual)
    assert eq64(hist, ref.history), (what, len(hist), len(ref.history))
    assert eq32(x, ref.x), (what, int(np.sum(b32(x) != b32(ref.x))))


def assert_same_run(got, other, what):
    assert got[0] == other[0] and (got[1].iterations, got[1].converged) == (other[1].iterations, other[1].converged), what
    assert same64([got[1].final_residual], [other[1].final_residual]) and same64(got[2], other[2]) and same32(got[3], other[3]), what


# ------------------------------------------------------------------------------------------------------------- the choice
def test_the_choice(ctx, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    c16, c18 = case(ctx, "poisson16"), case(ctx, "poisson18")
    assert c16.d.encoding()[0] == "csr-p16" and c18.d.encoding()[0] == "csr-p16"
    assert c16.pattern.encoding() == "pattern-stage" and c18.pattern.encoding() == "pattern" and c16.plain.encoding() == "plain"
    assert c16.d.lower("auto").encoding() == "pattern-stage" and c16.d.lower("plain").encoding() == "plain"
    monkeypatch.setenv("KRYST_SPMV32_STAGE", "0")
    assert c16.pattern.encoding() == "pattern" and c18.pattern.encoding() == "pattern" and c16.plain.encoding() == "plain"
    monkeypatch.setenv("KRYST_SPMV32_FORM", "plain")
    assert c16.pattern.encoding() == "plain" and c18.pattern.encoding() == "plain" and c16.plain.encoding() == "plain"
    monkeypatch.delenv("KRYST_SPMV32_STAGE")
    monkeypatch.setenv("KRYST_SPMV32_FORM", "pattern")
    assert c16.pattern.encoding() == "pattern-stage" and c18.pattern.encoding() == "pattern" and c16.plain.encoding() == "plain"
    assert c16.pattern.info == c16.plain.info == c16.ref.info                   # the plain arrays are lowered as ever


# ------------------------------------------------------------------------------------------------------------- spmv32
@pytest.mark.parametrize("name", list(P.OPERATORS))
def test_spmv32_on_every_operator(ctx, monkeypatch, name):
    c = case(ctx, name)
    a = c.a
    assert c.pattern.info == c.ref.info == c.plain.info
    operands = [("vec32", MC.vec32(a.ncols))] + ([("special32", MC.special32(a.ncols))] if a.ncols > 8 else [])
    wants = [c.ref.spmv(x) for _, x in operands]
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        for (label, x), want in zip(operands, wants):
            got = product(ctx, c.pattern, x, a.nrows)
            base = product(ctx, c.plain, x, a.nrows)
            assert same32(got, base), (name, setting, label, np.flatnonzero(b32(got) != b32(base))[:8])
            nan_can_arise = label == "special32" or name == "special_values"
            assert (same_ieee if nan_can_arise else same32)(got, want), (name, setting, label, np.flatnonzero(b32(got) != b32(want))[:8])
    if name == "empty_rows":
        assert not b32(wants[0][4::5]).any()                                    # an empty row is +0.0, the sign included


@pytest.mark.parametrize("name", ["tridiag_holes", "poisson16_holes"])
def test_absent_entries_never_see_their_operand(ctx, monkeypatch, name):
    """NaN, +inf and -inf exactly at elements of x that no stored entry reads -- a quad's gather covers them all the same"""
    c = case(ctx, name)
    holes = P.TRIDIAG_HOLES if name == "tridiag_holes" else P.POISSON_HOLES
    xs = P.poison_at(c.a.ncols, holes)
    wants = [c.ref.spmv(x) for x in xs]
    readers = [] if name == "tridiag_holes" else holes                          # (the staged kernel needs every diagonal: row c reads x[c])
    assert all(np.flatnonzero(~np.isfinite(w)).tolist() == sorted(readers) for w in wants)
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        for x, want in zip(xs, wants):
            got = product(ctx, c.pattern, x, c.a.nrows)
            assert (same_ieee if readers else same32)(got, want), (name, setting, np.flatnonzero(b32(got) != b32(want))[:8])
            assert same32(got, product(ctx, c.plain, x, c.a.nrows)), (name, setting)


@pytest.mark.parametrize("name", ["poisson16", "poisson12", "poisson18", "tridiag1", "tridiag1023", "tridiag1025", "long_row", "wide", "tall", "period3"])
def test_spmv32_with_dirty_padding(ctx, monkeypatch, name):
    """the elements behind x's last -- the three past the last column among them -- and behind y's last hold a NaN or 3e38"""
    c = case(ctx, name)
    a = c.a
    x = MC.vec32(a.ncols)
    want = c.ref.spmv(x)
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        clean = product(ctx, c.pattern, x, a.nrows)
        assert same32(clean, want), (name, setting)
        for value in POISONS32:
            xv, yv = poisoned32(K.DeviceVec32(ctx, x), value), poisoned32(nan_filled(ctx, a.nrows), value)
            c.pattern.spmv(xv, yv)
            assert same32(yv.to_host(), clean) and same32(xv.to_host(), x), (name, setting, value)


# ------------------------------------------------------------------------------------------------------------- the fused partial, the solvers
def solve_plans(c):
    """the solves of one operator and their restated results, made once"""
    def make():
        a, n = c.a, c.a.nrows
        inv = O.Pc.jacobi(a).inv_diag
        b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
        plans = []
        for start, x0 in (("zero", zero), ("guess", MC.vec32(n, seed=5))):
            for cap in (1, 2, 7):                                               # tolerance 1e-30: a fixed number of iterations
                ref = R.cg32(c.ref, b, x0, 1e-30, cap)
                assert ref.code == R.OK and ref.iterations == cap
                plans.append((("cg32", start, cap), lambda cap=cap: K.Cg32Solver(1e-30, cap), False, b, x0, ref))
                for nt in (UNPRE, PRE):
                    ref = R.pcg32(c.ref, inv, b, x0, 1e-30, cap, int(nt))
                    assert ref.code == R.OK and ref.iterations == cap
                    plans.append((("pcg32", start, cap, int(nt)), lambda cap=cap, nt=nt: K.Pcg32Solver(1e-30, cap).with_norm(nt), True, b, x0, ref))
        ref = R.cg32(c.ref, b, zero, 1e-5, 400)
        assert ref.code == R.OK and 5 < ref.iterations < 400
        plans.append((("cg32 to 1e-5",), lambda: K.Cg32Solver(1e-5, 400), False, b, zero, ref))
        for nt in (UNPRE, PRE):
            ref = R.pcg32(c.ref, inv, b, zero, 1e-5, 400, int(nt))
            assert ref.code == R.OK and 2 < ref.iterations < 400
            plans.append((("pcg32 to 1e-5", int(nt)), lambda nt=nt: K.Pcg32Solver(1e-5, 400).with_norm(nt), True, b, zero, ref))
        return plans
    return c.once("solve plans", make)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", P.SOLVE_OPERATORS)
def test_cg32_and_pcg32(ctx, monkeypatch, name, setting):
    c = case(ctx, name)
    if setting not in settings_of(c):
        return                                                                  # (runs of one tile: the staged kernel only)
    plans = solve_plans(c)
    pc = c.once("jacobi", lambda: K.Jacobi().setup(c.d))
    enter(monkeypatch, c, setting)
    for what, make, jacobi, b, x0, ref in plans:
        got = run32(make(), c.pattern, pc if jacobi else None, b, x0)
        assert_solve(got, ref, (name, setting) + what)
    what, make, jacobi, b, x0, ref = plans[-1]
    assert_same_run(run32(make(), c.pattern, pc, b, x0), run32(make(), c.plain, pc, b, x0), (name, setting, "against the plain lowering"))


def test_b_and_x_the_same_vector(ctx, monkeypatch):
    c = case(ctx, "poisson16")
    n = c.a.nrows
    b = R.store(MC.rhs(n))
    inv, pc = O.Pc.jacobi(c.a).inv_diag, c.once("jacobi", lambda: K.Jacobi().setup(c.d))
    refs = (R.cg32(c.ref, b, b, 1e-5, 400), R.pcg32(c.ref, inv, b, b, 1e-5, 400, 1))
    assert all(r.code == R.OK and r.iterations > 3 for r in refs)
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        assert_solve(run32(K.Cg32Solver(1e-5, 400), c.pattern, None, b, None, same_vector=True), refs[0], (setting, "cg32"))
        assert_solve(run32(K.Pcg32Solver(1e-5, 400), c.pattern, pc, b, None, same_vector=True), refs[1], (setting, "pcg32"))


def test_an_indefinite_matrix_and_a_zero_jacobi_entry(ctx, monkeypatch):
    for what, a in (("indefinite", MC.indefinite()), ("zero diagonal", MC.zero_diagonal())):
        c = Case(ctx, a, "pattern")
        n = a.nrows
        b = np.zeros(n, np.float32); b[1] = 1.0
        if what == "zero diagonal":
            b = R.store(MC.rhs(n))
        zero = np.zeros(n, np.float32)
        inv, pc = O.Pc.jacobi(a).inv_diag, K.Jacobi().setup(c.d)
        ref, refp = R.cg32(c.ref, b, zero, 1e-6, 50), R.pcg32(c.ref, inv, b, zero, 1e-6, 50, 1)
        if what == "indefinite":
            assert ref.code == R.INDEFINITE_MATRIX
        else:
            assert inv[5] == 0.0
        for setting in settings_of(c):
            enter(monkeypatch, c, setting)
            assert_solve(run32(K.Cg32Solver(1e-6, 50), c.pattern, None, b, zero), ref, (what, setting, "cg32"), nan_can_arise=True)
            assert_solve(run32(K.Pcg32Solver(1e-6, 50), c.pattern, pc, b, zero), refp, (what, setting, "pcg32"), nan_can_arise=True)


def test_two_fold_chunks(ctx, monkeypatch):
    """104^3: 1099 tile partials, more than one chunk of 1024 in the fold"""
    c = Case(ctx, P.poisson(104), "pattern-stage")
    n = c.a.nrows
    assert -(-n // 1024) == 1099
    b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
    ref = R.cg32(c.ref, b, zero, 1e-30, 3)
    assert ref.iterations == 3
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        assert_solve(run32(K.Cg32Solver(1e-30, 3), c.pattern, None, b, zero), ref, setting)


def test_the_tile_stride_and_run_loops(ctx, monkeypatch):
    """16 x 16 x 1100: 275 tiles -- more workgroups than compute units, runs of several tiles, an odd count of tiles for runs of two"""
    c = Case(ctx, P.poisson(16, 16, 1100), "pattern-stage")
    n = c.a.nrows
    assert n == 281600 and n // 1024 == 275
    x = MC.vec32(n)
    want = c.ref.spmv(x)
    b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
    ref = R.cg32(c.ref, b, zero, 1e-30, 3)
    assert ref.iterations == 3
    for setting in settings_of(c):
        enter(monkeypatch, c, setting)
        got = product(ctx, c.pattern, x, n)
        assert same32(got, want), (setting, int(np.sum(b32(got) != b32(want))))
        assert_solve(run32(K.Cg32Solver(1e-30, 3), c.pattern, None, b, zero), ref, setting)


@pytest.mark.parametrize("tpw", ["1", "3", "8"])
def test_tiles_per_workgroup_of_the_pattern_kernel(ctx, monkeypatch, tpw):
    """KRYST_SPMV32_PATTERN_TPW (4 by default) on the unstaged pattern kernel, six tiles: one tile per workgroup, two workgroups of three, and
    one workgroup whose run of eight ends at the last tile"""
    c = case(ctx, "poisson18")
    n = c.a.nrows
    assert -(-n // 1024) == 6
    enter(monkeypatch, c, "stage0")
    monkeypatch.setenv("KRYST_SPMV32_PATTERN_TPW", tpw)
    assert c.pattern.encoding() == "pattern"
    x = MC.vec32(n)
    got, want = product(ctx, c.pattern, x, n), c.ref.spmv(x)
    assert same32(got, want), (tpw, int(np.sum(b32(got) != b32(want))))
    b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
    ref = R.cg32(c.ref, b, zero, 1e-30, 3)
    assert ref.iterations == 3
    assert_solve(run32(K.Cg32Solver(1e-30, 3), c.pattern, None, b, zero), ref, tpw)


# ------------------------------------------------------------------------------------------------------------- refinement
def refine(ctx, d, pc, b, x0, form):
    s = K.RefinementSolver(MC.OUTER_TOL, MC.OUTER_CAP).with_inner(MC.INNER_TOL, MC.INNER_CAP).with_form(form)
    xv = ctx.vec(x0)
    stats = s.solve(d, pc, ctx.vec(b), xv)
    return s, stats, xv.to_host()


def assert_refined(got, ref, what):
    s, stats, x = got
    assert (stats.iterations, stats.converged, stats.inner_iterations) == (ref.iterations, ref.converged, ref.inner_iterations), what
    assert same64([stats.final_residual], [ref.final_residual]) and same64(s.residual_history, ref.history) and same64(x, ref.x), what


def test_refinement_on_the_pattern_lowering(ctx, monkeypatch):
    a = MC.poisson12()
    d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
    b, x0 = MC.rhs(a.nrows), MC.rhs(a.nrows, seed=9)
    ref = R.refine(a, R.Lowered(a), None, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.code == R.OK and ref.converged and ref.iterations >= 2
    for setting, kernel in (("default", "pattern-stage"), ("stage0", "pattern"), ("plain", "plain"), ("stage-t1", "pattern-stage")):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in SETTINGS[setting].items():
            monkeypatch.setenv(k, v)
        got = refine(ctx, d, None, b, x0, "pattern")
        assert got[0].lowered(d).encoding() == kernel, setting
        assert_refined(got, ref, setting)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert refine(ctx, d, None, b, x0, "plain")[0].lowered(d).encoding() == "plain"      # the default lowering is what it was


def test_refinement_where_there_is_no_pattern_form(ctx, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    a = MC.varcoef12()
    d = K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
    assert d.encoding()[0] != "csr-p16"
    pc, inv = K.Jacobi().setup(d), O.Pc.jacobi(a).inv_diag
    b, x0 = MC.rhs(a.nrows), np.zeros(a.nrows)
    ref = R.refine(a, R.Lowered(a), inv, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.code == R.OK and ref.converged
    with pytest.raises(K.KError) as e:
        refine(ctx, d, pc, b, x0, "pattern")
    assert e.value.code == UNSUPPORTED
    for form in ("auto", "plain"):
        got = refine(ctx, d, pc, b, x0, form)
        assert got[0].lowered(d).encoding() == "plain"
        assert_refined(got, ref, form)                                          # the same bits as ever


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    rng = np.random.default_rng(31)
    n = 2000
    cols = np.clip(np.arange(n)[:, None] + np.array([-9, -4, 0, 3, 8])[None, :], 0, n - 1)
    keep = np.ones((n, 5), dtype=bool); keep[:9, :2] = False; keep[-8:, 3:] = False
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    band = O.Csr(n, n, rp, cols[keep], rng.standard_normal(int(rp[-1])))           # 2000 distinct rows: no CSR-P16 form
    d = K.CsrMatrix.from_csr(n, n, band.row_ptr, band.col_idx, band.vals, ctx=ctx)
    assert d.encoding()[0] != "csr-p16"
    with pytest.raises(K.KError) as e:
        d.lower("pattern")
    assert e.value.code == UNSUPPORTED
    h = _ffi.Handle()
    assert K.lib().kryst_csr32_lower_form(d.h, 2, C.byref(h)) == UNSUPPORTED and not h          # the handle is untouched
    assert K.lib().kryst_csr32_lower_form(d.h, 7, C.byref(h)) == ERR_ARG and not h              # a bad form
    assert K.lib().kryst_csr32_lower_form(d.h, -1, C.byref(h)) == ERR_ARG and not h
    with pytest.raises(K.KError) as e:
        d.lower("p16")
    assert e.value.code == ERR_ARG
    auto = d.lower("auto")                                                      # falls back to the plain arrays
    assert auto.encoding() == "plain"
    x = MC.vec32(n)
    assert same32(product(ctx, auto, x, n), R.Lowered(band).spmv(x))
    # a row-partitioned operator, made on this one rank
    a = P.tridiag(1025)
    dd = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)
    for form in ("plain", "auto", "pattern"):
        with pytest.raises(K.KError) as e:
            dd.lower(form)
        assert e.value.code == UNSUPPORTED, form


# ------------------------------------------------------------------------------------------------------------- the C++ mirror
def test_cpp_mixed_pattern_mirror():
    """tests/cpp/test_mixed_pattern_mirror.cpp: HipCsrMatrix32(a, Pattern) of include/kryst_hip.hpp on a 64-row tridiagonal operator"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_mixed_pattern_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for k in KNOBS:
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_MIXED_PATTERN_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
