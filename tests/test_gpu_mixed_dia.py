"""The fp32-stored SpMV, CG, PCG and refinement on the diagonal (CSR-DIA) lowering, against the numpy restatement of the contract
(tests/mixed_ref.py, which is blind to the encoding) and against the same call on the plain-lowered operator.  The rule of
tests/test_gpu_mixed.py holds: integer views, bit for bit, no tolerance; where a NaN can arise (non-finite operands or stored values) the
comparison with the RESTATEMENT is `nonfinite_cases.same_ieee` -- sign and payload of a NaN made by inf - inf differ between host and device --
while the comparison with the plain-lowered operator stays bit for bit.  Every product goes into a NaN-filled y.

The operators are created under KRYST_SPMV_DIA=2 (set around the creation only), so that small operators with few distinct values keep diagonal
streams too.  Every case runs under the settings of mixed_dia_cases.SETTINGS -- the default and the word `dia`, which must report "dia", and
KRYST_SPMV32_FORM=plain, which must report "plain"; `encoding()` is asserted first, so that no case passes because another kernel ran.
Fixtures: tests/mixed_dia_cases.py (their properties: tests/test_mixed_dia_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import mixed_cases as MC
import mixed_dia_cases as D
import mixed_ref as R
from nonfinite_cases import same_ieee

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
b32, b64 = MC.bits32, MC.bits64
UNPRE, PRE = K.CgNormType.Unpreconditioned, K.CgNormType.Preconditioned
UNSUPPORTED, ERR_ARG = 6, 102
POISONS32 = [None, np.float32(3e38)]               # the quiet NaN 0x7FC00000, and a finite value
KNOBS = ("KRYST_SPMV32_FORM", "KRYST_SPMV32_STAGE", "KRYST_SPMV32_BLOCKS_PER_CU", "KRYST_SPMV32_DIA_NT", "KRYST_SPMV_COMPRESS", "KRYST_SPMV_DIA")


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    assert K.reduce_spec32() == R.SPEC32
    return K.Context(0)


def create(ctx, monkeypatch, a, dia="2"):
    """the device operator, created under KRYST_SPMV_DIA=`dia` (None: the defaults)"""
    with monkeypatch.context() as m:
        m.delenv("KRYST_SPMV_DIA", raising=False)
        if dia is not None:
            m.setenv("KRYST_SPMV_DIA", dia)
        return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def holds_dia(monkeypatch, d):
    """(does the operator stream CSR-DIA when the more compact forms are switched off, the number of diagonals)"""
    with monkeypatch.context() as m:
        m.delenv("KRYST_SPMV_DIA", raising=False)
        m.setenv("KRYST_SPMV_COMPRESS", "1")
        e = d.encoding()
    return e[0] == "csr-dia", e[1]


class Case:
    """an operator on the host, its restatement, the device operator and both lowerings -- made once per module"""
    def __init__(self, ctx, monkeypatch, a, dia="2"):
        self.a, self.ref = a, R.Lowered(a)
        self.d = create(ctx, monkeypatch, a, dia)
        assert holds_dia(monkeypatch, self.d) == (True, len(D.offsets(a)))                       # the form is held
        self.plain, self.dia = self.d.lower(), self.d.lower("dia")
        self.memo = {}

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]


_cases = {}


def case(ctx, monkeypatch, name):
    if name not in _cases:
        make = D.OPERATORS.get(name) or D.SOLVE_OPERATORS[name]
        _cases[name] = Case(ctx, monkeypatch, make())
    return _cases[name]


def enter(monkeypatch, c, setting):
    """switch to `setting` and make sure the kernel under test is the one that runs"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    env, want = D.SETTINGS[setting]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert c.dia.encoding() == want, (setting, c.dia.encoding(), want)
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
    a = MC.varcoef12()
    c = Case(ctx, monkeypatch, a, dia=None)                                     # created under the defaults: no CSR-D16 / P16 form, so it has streams
    assert c.d.encoding()[0] == "csr-dia"
    assert c.dia.encoding() == "dia" and c.plain.encoding() == "plain"
    assert c.d.lower("auto").encoding() == "plain"                              # auto never chooses the diagonal form
    assert c.dia.info == c.plain.info == c.ref.info                             # the plain arrays are lowered as ever
    x = MC.vec32(a.ncols)
    want = c.ref.spmv(x)
    for word, kernel in (("plain", "plain"), ("dia", "dia"), ("pattern", "dia"), ("csr", "dia")):
        monkeypatch.setenv("KRYST_SPMV32_FORM", word)
        assert c.dia.encoding() == kernel and c.plain.encoding() == "plain", word
        assert same32(product(ctx, c.dia, x, a.nrows), want), word
    monkeypatch.delenv("KRYST_SPMV32_FORM")
    # a constant-coefficient operator created under the defaults keeps its row patterns and no streams
    p = D.P.poisson(12)
    d = create(ctx, monkeypatch, p, dia=None)
    assert d.encoding()[0] == "csr-p16" and holds_dia(monkeypatch, d)[0] is False
    with pytest.raises(K.KError) as e:
        d.lower("dia")
    assert e.value.code == UNSUPPORTED
    assert d.lower("pattern").encoding() == "pattern-stage"                     # ... and the other forms decide as they did
    with monkeypatch.context() as m:
        m.setenv("KRYST_SPMV32_FORM", "dia")
        assert d.lower("pattern").encoding() == "pattern-stage" and d.lower().encoding() == "plain"


# ------------------------------------------------------------------------------------------------------------- spmv32
@pytest.mark.parametrize("name", list(D.OPERATORS))
def test_spmv32_on_every_operator(ctx, monkeypatch, name):
    c = case(ctx, monkeypatch, name)
    a = c.a
    assert c.dia.info == c.ref.info == c.plain.info
    operands = [("vec32", MC.vec32(a.ncols))] + ([("special32", MC.special32(a.ncols))] if a.ncols > 8 else [])
    wants = [c.ref.spmv(x) for _, x in operands]
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        for (label, x), want in zip(operands, wants):
            got = product(ctx, c.dia, x, a.nrows)
            base = product(ctx, c.plain, x, a.nrows)
            assert same32(got, base), (name, setting, label, np.flatnonzero(b32(got) != b32(base))[:8])
            nan_can_arise = label == "special32" or name == "special_values"
            assert (same_ieee if nan_can_arise else same32)(got, want), (name, setting, label, np.flatnonzero(b32(got) != b32(want))[:8])


def test_varcoef12_created_under_the_defaults(ctx, monkeypatch):
    a = MC.varcoef12()
    c = Case(ctx, monkeypatch, a, dia=None)
    x = MC.vec32(a.ncols)
    want = c.ref.spmv(x)
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        got = product(ctx, c.dia, x, a.nrows)
        assert same32(got, want) and same32(got, product(ctx, c.plain, x, a.nrows)), setting


@pytest.mark.parametrize("name", ["tridiag_holes", "varcoef12_holes"])
def test_absent_entries_never_see_their_operand(ctx, monkeypatch, name):
    """NaN, +inf and -inf exactly at elements of x that only absent entries address -- a lane's 16-byte load covers them all the same"""
    c = case(ctx, monkeypatch, name)
    holes = D.unread_elements(c.a).tolist()
    assert holes == (D.TRIDIAG_HOLES if name == "tridiag_holes" else D.VARCOEF_HOLES)
    xs = D.poison_at(c.a.ncols, holes)
    wants = [c.ref.spmv(x) for x in xs]
    assert all(np.isfinite(w).all() for w in wants)
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        for x, want in zip(xs, wants):
            got = product(ctx, c.dia, x, c.a.nrows)
            assert same32(got, want), (name, setting, np.flatnonzero(b32(got) != b32(want))[:8])
            assert same32(got, product(ctx, c.plain, x, c.a.nrows)), (name, setting)


@pytest.mark.parametrize("name", ["tridiag1", "tridiag1023", "tridiag1024", "tridiag1025", "varcoef12", "varbox16x16x20", "band11", "box27", "far", "nonsquare"])
def test_spmv32_with_dirty_padding(ctx, monkeypatch, name):
    """the elements behind x's last -- absent entries of the last rows address them -- and behind y's last hold a NaN or 3e38"""
    c = case(ctx, monkeypatch, name)
    a = c.a
    x = MC.vec32(a.ncols)
    want = c.ref.spmv(x)
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        clean = product(ctx, c.dia, x, a.nrows)
        assert same32(clean, want), (name, setting)
        for value in POISONS32:
            xv, yv = poisoned32(K.DeviceVec32(ctx, x), value), poisoned32(nan_filled(ctx, a.nrows), value)
            c.dia.spmv(xv, yv)
            assert same32(yv.to_host(), clean) and same32(xv.to_host(), x), (name, setting, value)


def test_stored_special_values(ctx, monkeypatch):
    """a stored -0.0, +inf, ordinary NaN, subnormal-making values are PRESENT and multiplied; a value that lowers to zero beside an inf in x is NaN"""
    c = case(ctx, monkeypatch, "special_values")
    a = c.a
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    k = 2500                                                                    # -1e-50: lowers to -0.0
    assert c.ref.vals32[k] == 0.0 and np.signbit(c.ref.vals32[k])
    x = MC.vec32(a.ncols)
    x[a.col_idx[k]] = np.inf
    want = c.ref.spmv(x)
    assert np.isnan(want[rows[k]])                                              # 0 * inf
    assert np.isnan(want[rows[1501]]) and np.isinf(want[rows[100]])             # the stored NaN and the stored inf
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        got = product(ctx, c.dia, x, a.nrows)
        assert same_ieee(got, want), (setting, np.flatnonzero(b32(got) != b32(want))[:8])
        assert np.isnan(got[rows[k]]) and np.isnan(got[rows[1501]])
        assert same32(got, product(ctx, c.plain, x, a.nrows)), setting
    # row 2: its entry 7 is a stored -0.0; with a zero operand everywhere the row folds 0.0 + (-0.0 * 0.0) ... to +0.0, the reference's sign
    zero = product(ctx, c.dia, np.zeros(a.ncols, np.float32), a.nrows)
    assert same_ieee(zero, c.ref.spmv(np.zeros(a.ncols, np.float32)))


@pytest.mark.parametrize("which", [0, 1])
def test_a_stored_nan_that_rounds_onto_the_marker(ctx, monkeypatch, which):
    a = D.marker_twin(which)
    d = create(ctx, monkeypatch, a)
    assert holds_dia(monkeypatch, d) == (True, 3)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(K.KError) as e:
        d.lower("dia")
    assert e.value.code == UNSUPPORTED
    h = _ffi.Handle()
    assert K.lib().kryst_csr32_lower_form(d.h, 3, C.byref(h)) == UNSUPPORTED and not h          # the handle is untouched
    plain = d.lower()                                                           # the plain lowering still works
    x = MC.vec32(a.ncols)
    assert same_ieee(product(ctx, plain, x, a.nrows), R.Lowered(a).spmv(x))


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


@pytest.mark.parametrize("setting", list(D.SETTINGS))
@pytest.mark.parametrize("name", list(D.SOLVE_OPERATORS))
def test_cg32_and_pcg32(ctx, monkeypatch, name, setting):
    c = case(ctx, monkeypatch, name)
    plans = solve_plans(c)
    pc = c.once("jacobi", lambda: K.Jacobi().setup(c.d))
    enter(monkeypatch, c, setting)
    for what, make, jacobi, b, x0, ref in plans:
        got = run32(make(), c.dia, pc if jacobi else None, b, x0)
        assert_solve(got, ref, (name, setting) + what)
    what, make, jacobi, b, x0, ref = plans[-1]
    assert_same_run(run32(make(), c.dia, pc, b, x0), run32(make(), c.plain, pc, b, x0), (name, setting, "against the plain lowering"))


def test_b_and_x_the_same_vector(ctx, monkeypatch):
    c = case(ctx, monkeypatch, "varcoef12")
    n = c.a.nrows
    b = R.store(MC.rhs(n))
    inv, pc = O.Pc.jacobi(c.a).inv_diag, c.once("jacobi", lambda: K.Jacobi().setup(c.d))
    refs = (R.cg32(c.ref, b, b, 1e-5, 400), R.pcg32(c.ref, inv, b, b, 1e-5, 400, 1))
    assert all(r.code == R.OK and r.iterations > 3 for r in refs)
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        assert_solve(run32(K.Cg32Solver(1e-5, 400), c.dia, None, b, None, same_vector=True), refs[0], (setting, "cg32"))
        assert_solve(run32(K.Pcg32Solver(1e-5, 400), c.dia, pc, b, None, same_vector=True), refs[1], (setting, "pcg32"))


def test_an_indefinite_matrix_and_a_zero_jacobi_entry(ctx, monkeypatch):
    for what, a in (("indefinite", MC.indefinite()), ("zero diagonal", MC.zero_diagonal())):
        c = Case(ctx, monkeypatch, a)
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
        for setting in D.SETTINGS:
            enter(monkeypatch, c, setting)
            assert_solve(run32(K.Cg32Solver(1e-6, 50), c.dia, None, b, zero), ref, (what, setting, "cg32"), nan_can_arise=True)
            assert_solve(run32(K.Pcg32Solver(1e-6, 50), c.dia, pc, b, zero), refp, (what, setting, "pcg32"), nan_can_arise=True)


def test_two_fold_chunks_and_the_capped_grid(ctx, monkeypatch):
    """a 104^3 variable-coefficient box: 1099 tile partials -- more than one chunk of 1024 in the fold, and more tiles than the capped grid has
    workgroups at one, two or four per compute unit on any device of up to 274 compute units -- so every workgroup strides"""
    c = Case(ctx, monkeypatch, D.varbox(104, 104, 104))
    n = c.a.nrows
    assert -(-n // 1024) == 1099
    x = MC.vec32(n)
    want = c.ref.spmv(x)
    b, zero = R.store(MC.rhs(n)), np.zeros(n, np.float32)
    ref = R.cg32(c.ref, b, zero, 1e-30, 3)
    assert ref.iterations == 3
    for setting in D.SETTINGS:
        enter(monkeypatch, c, setting)
        got = product(ctx, c.dia, x, n)
        assert same32(got, want), (setting, int(np.sum(b32(got) != b32(want))))
        assert_solve(run32(K.Cg32Solver(1e-30, 3), c.dia, None, b, zero), ref, setting)
    # the grid cap and the value loads of the A/B change no bit
    enter(monkeypatch, c, "default")
    for knob, values in (("KRYST_SPMV32_BLOCKS_PER_CU", ("1", "2", "4")), ("KRYST_SPMV32_DIA_NT", ("0",))):
        for v in values:
            with monkeypatch.context() as m:
                m.setenv(knob, v)
                assert c.dia.encoding() == "dia"
                assert same32(product(ctx, c.dia, x, n), want), (knob, v)


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


def test_refinement_on_the_diagonal_lowering(ctx, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    a = MC.varcoef12()
    d = create(ctx, monkeypatch, a, dia=None)
    pc, inv = K.Jacobi().setup(d), O.Pc.jacobi(a).inv_diag
    b, x0 = MC.rhs(a.nrows), np.zeros(a.nrows)
    ref = R.refine(a, R.Lowered(a), inv, b, x0, MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
    assert ref.code == R.OK and ref.converged and ref.iterations >= 2
    for setting, (env, kernel) in D.SETTINGS.items():
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            got = refine(ctx, d, pc, b, x0, "dia")
            assert got[0].lowered(d).encoding() == kernel, setting
            assert_refined(got, ref, setting)
    assert refine(ctx, d, pc, b, x0, "plain")[0].lowered(d).encoding() == "plain"               # the default lowering is what it was


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    # an operator whose diagonals are too sparsely filled, created under the defaults and under KRYST_SPMV_DIA=2: no streams either way
    s = D.sparse_diagonals()
    for dia in (None, "2"):
        d = create(ctx, monkeypatch, s, dia)
        assert holds_dia(monkeypatch, d)[0] is False
        with pytest.raises(K.KError) as e:
            d.lower("dia")
        assert e.value.code == UNSUPPORTED
        h = _ffi.Handle()
        assert K.lib().kryst_csr32_lower_form(d.h, 3, C.byref(h)) == UNSUPPORTED and not h      # the handle is untouched
        assert K.lib().kryst_csr32_lower_form(d.h, 4, C.byref(h)) == ERR_ARG and not h          # a bad form
        assert K.lib().kryst_csr32_lower_form(d.h, -1, C.byref(h)) == ERR_ARG and not h
        with pytest.raises(K.KError) as e:
            d.lower("diagonal")
        assert e.value.code == ERR_ARG
        auto = d.lower("auto")
        assert auto.encoding() == "plain"
        x = MC.vec32(s.ncols)
        assert same32(product(ctx, auto, x, s.nrows), R.Lowered(s).spmv(x))
    # the 2000-row band of the row-pattern refusal test: created with KRYST_SPMV_DIA=0 it has no streams and is refused; created under the
    # defaults it satisfies the fill rule (tests/test_mixed_dia_cpu.py) and has no CSR-D16 / P16 form, so it HAS streams and lowers
    band = D.refusal_band()
    d0 = create(ctx, monkeypatch, band, "0")
    with pytest.raises(K.KError) as e:
        d0.lower("dia")
    assert e.value.code == UNSUPPORTED
    dd = create(ctx, monkeypatch, band, None)
    assert dd.encoding()[0] == "csr-dia"
    lowered = dd.lower("dia")
    assert lowered.encoding() == "dia"
    x = MC.vec32(band.ncols)
    assert same32(product(ctx, lowered, x, band.nrows), R.Lowered(band).spmv(x))
    # a row-partitioned operator, made on this one rank
    a = D.tridiag(1025)
    with monkeypatch.context() as m:
        m.setenv("KRYST_SPMV_DIA", "2")
        dist = K.CsrMatrix.from_csr_dist(ctx, a.nrows, [0, a.nrows], a.row_ptr, a.col_idx, a.vals)
    with pytest.raises(K.KError) as e:
        dist.lower("dia")
    assert e.value.code == UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------- the C++ mirror
def test_cpp_mixed_dia_mirror():
    """tests/cpp/test_mixed_dia_mirror.cpp: HipCsrMatrix32(a, Dia) of include/kryst_hip.hpp on a 1500-row tridiagonal operator"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_mixed_dia_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for k in KNOBS:
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CPP_MIXED_DIA_MIRROR_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
