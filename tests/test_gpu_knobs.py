"""Every kernel form and launch geometry that an environment setting selects and that no older test ran (the rows of tests/knob_cases.py),
bit for bit against the CPU oracle or the numpy restatements -- never against another run of the device code.

Where the library offers a witness (encoding(), pattern_info(), ilu_info()["form"], ChebyshevPoly.info()["fused"]) it is asserted BEFORE any
number is compared, so that no case passes on the wrong kernel.  Settings that the sources read once per process run in a fresh child
(tests/knob_worker.py), one at a time; the parent computes the references itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import cheb_poly_ref as CP
import knob_cases as KC
import multi_rhs_cases as MR
import pca_gmres_ref as PR
from nonfinite_cases import box_operator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCN = K.Preconditioning


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


@pytest.fixture(scope="module")
def num_cu():
    """the device's real CU count"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def same_solve(ref, st, s, x, label):
    assert (st.iterations, bool(st.converged)) == (ref.iterations, bool(ref.converged)), (label, st, ref.iterations, ref.converged)
    assert np.array_equal(np.array(s.residual_history, dtype=float), np.array(ref.history, dtype=float)), (label, "residual history")
    assert np.array_equal(x, ref.x), (label, int(np.sum(x != ref.x)))


# ================================================================================================================ SpMV tile mappings
# the storage forms the older tests force (test_spmv_kernel_forms_bit_exact, test_spmv_diagonal_streams_form_bit_exact), per launch
FORMS = {
    "wave": {"KRYST_SPMV_KERNEL": "2", "KRYST_SPMV_COMPRESS": "0", "KRYST_SPMV_DIA": "0"},
    "rows": {"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "0", "KRYST_SPMV_DIA": "0"},
    "d8": {"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "1", "KRYST_SPMV_DIA": "0"},
    "dia": {"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "1", "KRYST_SPMV_DIA": "2"},
    "d16": {"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "2", "KRYST_SPMV_DIA": "0"},
    "p16": {"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "3", "KRYST_SPMV_DIA": "2"},
}
# the encoding each form must report: constant-coefficient stencils have every form, the variable-coefficient one no dictionary of values
# (CSR-D16, CSR-P16 fall back), the random operators nothing but the plain arrays
ENCODING = {
    "const": {"wave": "csr", "rows": "csr", "d8": "csr-d8", "dia": "csr-dia", "d16": "csr-d16", "p16": "csr-p16"},
    "varcoef": {"wave": "csr", "rows": "csr", "d8": "csr-d8", "dia": "csr-dia", "d16": "csr-d8", "p16": "csr-dia"},
    "random": {f: "csr" for f in FORMS},
}


class Op:
    """a host operator, its device twin (made with every storage form it qualifies for: KRYST_SPMV_DIA=2 at creation), x and the oracle's A x"""
    def __init__(self, ctx, a, family, generator=None):
        self.a, self.family = a, family
        self.d = K.CsrMatrix.stencil7(*generator, ctx=ctx) if generator else to_dev(ctx, a)
        self.x = O.splitmix64_uniform(0xC0FFEE + a.nrows, a.ncols) - 0.5
        self.y = a.spmv(self.x)


@pytest.fixture(scope="module")
def ops(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            saved = os.environ.get("KRYST_SPMV_DIA")
            os.environ["KRYST_SPMV_DIA"] = "2"
            try:
                if name in ("ragged", "random"):
                    cache[name] = Op(ctx, MR.ragged() if name == "ragged" else KC.random_csr(), "random")
                else:
                    kind, N, how = name.split("-")
                    cache[name] = Op(ctx, O.stencil7(int(N), kind), "varcoef" if kind == "varcoef" else "const",
                                     generator=(int(N), kind) if how == "gen" else None)
            finally:
                if saved is None:
                    del os.environ["KRYST_SPMV_DIA"]
                else:
                    os.environ["KRYST_SPMV_DIA"] = saved
        return cache[name]
    return get


def stencil_names(sizes):
    return [f"{kind}-{N}-{how}" for N in sizes for kind in ("poisson", "convdiff", "varcoef") for how in ("host", "gen")]


def test_the_operators_have_the_tile_counts_of_the_table(ops):
    assert [KC.ntiles_of(N ** 3) for N in (17, 33)] == list(KC.STENCIL_TILES) and [KC.ntiles_of(N ** 3) for N in (18, 34)] == list(KC.STAGED_TILES)
    assert (KC.ntiles_of(ops("ragged").a.nrows), KC.ntiles_of(ops("random").a.nrows)) == KC.SMALL_TILES[2:]
    assert KC.ntiles_of(65 ** 3) == KC.STRIDED_TILES and KC.ntiles_of(64 ** 3) == 512


MAPPING_SETTINGS = [(k, v) for k, vs in (("KRYST_SPMV_SWIZZLE", "01"), ("KRYST_SPMV_GROUP", "138"), ("KRYST_SPMV_PATTERN_TPW", "138"),
                                         ("KRYST_SPMV_STAGE_GROUP", "13"), ("KRYST_SPMV_STAGE_T", "24")) for v in vs]


# which launches read a mapping setting: (forms, stencil sizes, the random operators too).  SWIZZLE and GROUP are read by every stream kernel
# and by the unstaged pattern kernel (odd N); TPW by the unstaged pattern kernel alone; the staged settings by the staged-window kernel alone,
# which needs an even line length -- N = 18 and 34, not the 17 and 33 of the other settings.  On the random operators every form is the plain
# arrays: the wave and the rows kernel.
READ_BY = {
    "KRYST_SPMV_SWIZZLE": (tuple(FORMS), (17, 33), True), "KRYST_SPMV_GROUP": (tuple(FORMS), (17, 33), True),
    "KRYST_SPMV_PATTERN_TPW": (("p16",), (17, 33), False),
    "KRYST_SPMV_STAGE_GROUP": (("p16",), (18, 34), False), "KRYST_SPMV_STAGE_T": (("p16",), (18, 34), False),
}


def spmv_under_forms(monkeypatch, op, forms, label, staged=None):
    for form in forms:
        with monkeypatch.context() as mp:
            setenv(mp, FORMS[form])
            assert op.d.encoding()[0] == ENCODING[op.family][form], (label, form, op.d.encoding())
            if staged is not None and form == "p16":
                assert op.d.pattern_info()["staged"] == staged, (label, op.d.pattern_info())
            got = op.d.spmv(op.x)
        assert np.array_equal(got, op.y), (label, form, int(np.sum(got != op.y)))


@pytest.mark.parametrize("name,value", MAPPING_SETTINGS, ids=lambda v: v.replace("KRYST_SPMV_", ""))
def test_spmv_tile_mapping_bit_exact(ctx, rs, ops, monkeypatch, name, value):
    """Each value of a mapping setting under the storage forms whose launch reads it (READ_BY), on operators whose tile counts are no
    multiple of 8 x group: a mapping that skips or repeats a tile leaves a row of y wrong.  Then once under a fused inner product (five
    BiCGStab iterations on convdiff, five CG iterations on poisson), so that the per-tile partials are checked, not only y."""
    monkeypatch.setenv(name, value)
    forms, sizes, random_too = READ_BY[name]
    staged = sizes[0] % 2 == 0
    for nm in stencil_names(sizes):
        op = ops(nm)
        if forms == ("p16",) and op.family != "const":
            continue                                    # (the variable-coefficient operator has no row-pattern form)
        spmv_under_forms(monkeypatch, op, forms, (name, value, nm), staged=staged if op.family == "const" else None)
    if random_too:
        for nm in ("ragged", "random"):
            spmv_under_forms(monkeypatch, ops(nm), ("wave", "rows"), (name, value, nm))
    N = sizes[0]
    for kind, method, cls in (("convdiff", "bicgstab", K.BiCgStabSolver), ("poisson", "cg", K.CgSolver)):
        op = ops(f"{kind}-{N}-host")
        b = op.a.spmv(np.ones(op.a.nrows))
        ref = O.solve(method, op.a, b, tol=0.0, max_iters=5, rs=rs)
        assert ref.iterations == 5
        for form in forms:
            with monkeypatch.context() as mp:
                setenv(mp, FORMS[form])
                assert op.d.encoding()[0] == ENCODING["const"][form]
                if form == "p16":
                    assert op.d.pattern_info()["staged"] == staged
                s = cls(0.0, 5); x = np.zeros(op.a.nrows)
                st = s.solve(op.d, None, b, x)
            same_solve(ref, st, s, x, (name, value, kind, N, form))


STREAM_FORMS = ("wave", "rows", "d8", "dia", "d16")


@pytest.fixture(scope="module")
def convdiff65(ctx):
    saved = os.environ.get("KRYST_SPMV_DIA")
    os.environ["KRYST_SPMV_DIA"] = "2"
    try:
        return Op(ctx, O.stencil7(65, "convdiff"), "const", generator=(65, "convdiff"))      # (made on the device: seconds less than an upload)
    finally:
        if saved is None:
            del os.environ["KRYST_SPMV_DIA"]
        else:
            os.environ["KRYST_SPMV_DIA"] = saved


@pytest.mark.parametrize("case", [c for c in KC.GEOMETRY_CASES if c["ntiles"] == KC.STRIDED_TILES], ids=KC.geometry_label)
def test_stream_kernels_stride_under_every_mapping(convdiff65, num_cu, monkeypatch, case):
    """537 tiles on one workgroup per CU: every stream kernel's tile loop takes a second and a third trip under the grouped and the swizzled
    mapping (its default grid hands each workgroup one slot, so nothing smaller reaches the second trip)"""
    visits = KC.mapping(case, num_cu)
    assert KC.visited_once(visits, case["ntiles"]) and KC.max_trips(visits) >= 2, (num_cu, KC.max_trips(visits))
    setenv(monkeypatch, case["env"])
    op = convdiff65
    for form in STREAM_FORMS:
        with monkeypatch.context() as mp:
            setenv(mp, FORMS[form])
            assert op.d.encoding()[0] == ENCODING["const"][form]
            got = op.d.spmv(op.x)
        assert np.array_equal(got, op.y), (form, int(np.sum(got != op.y)))


@pytest.mark.parametrize("bpc", ["1", "2"])
def test_spmv_workgroups_per_cu_at_64_cubed(ctx, rs, num_cu, monkeypatch, bpc):
    """512 tiles: at one workgroup per CU every workgroup of a stream kernel takes two trips (the second re-uses what the first left in LDS
    and writes the second per-tile partial).  One SpMV per storage form, then ten CG iterations."""
    visits = KC.stream_map(512, bpc=int(bpc), num_cu=num_cu)
    assert KC.visited_once(visits, 512)
    if bpc == "1":
        assert KC.max_trips(visits) >= 2, num_cu
    monkeypatch.setenv("KRYST_SPMV_DIA", "2")
    a = O.stencil7(64, "poisson")
    d = K.CsrMatrix.stencil7(64, "poisson", ctx=ctx)
    monkeypatch.setenv("KRYST_SPMV_BLOCKS_PER_CU", bpc)
    x = O.splitmix64_uniform(64, a.ncols) - 0.5
    want = a.spmv(x)
    b = a.spmv(np.ones(a.nrows))
    ref = O.solve("cg", a, b, tol=0.0, max_iters=10, rs=rs)
    for form, env in FORMS.items():
        with monkeypatch.context() as mp:
            setenv(mp, env)
            assert d.encoding()[0] == ENCODING["const"][form]
            got = d.spmv(x)
            assert np.array_equal(got, want), (form, int(np.sum(got != want)))
            s = K.CgSolver(0.0, 10); xs = np.zeros(a.nrows)
            st = s.solve(d, None, b, xs)
        same_solve(ref, st, s, xs, (bpc, form))


# ================================================================================================================ CG's fused direction pass
def _cg_like(ctx, rs, a, d, method, cap, label, jacobi=False):
    b = O.splitmix64_uniform(0xD0E + a.nrows, a.nrows)
    x0 = O.splitmix64_uniform(0xABC, a.nrows)
    opc, kpc = (O.Pc.jacobi(a), K.Jacobi().setup(d)) if jacobi else (None, None)
    res = O.solve(method, a, b, pc=opc, x0=x0, tol=1e-9, max_iters=cap, rs=rs, raise_on_error=False)
    s = (K.PcgSolver if method == "pcg" else K.CgSolver)(1e-9, cap); x = x0.copy()
    try:
        st, code = s.solve(d, kpc, b, x), 0
    except K.KError as e:                               # (the unsymmetric operator: IndefiniteMatrix must match too)
        st, code = e.stats, e.code
    assert code == res.code, (label, code, res.code)
    assert (st.iterations, bool(st.converged)) == (res.iterations, bool(res.converged)), (label, st, res.iterations, res.converged)
    assert len(s.residual_history) == len(res.history), label
    if code == 0:
        assert np.array_equal(np.array(s.residual_history), res.history), label
        assert st.final_residual == res.final_residual and np.array_equal(x, res.x), label
    return res


# the shapes of test_direction_pass_inside_the_spmv_on_every_exit_path, one way out each: convergence, caps inside and at the end of a run of
# iterations, the unsymmetric operator's error exit, Jacobi-PCG
FUSE_SHAPES = [(10, "aniso", "2", "cg", 400, False), (16, "poisson", "2", "pcg", 3, True), (16, "poisson", "4", "cg", 1, False),
               (32, "convdiff", "2", "cg", 8, False), (40, "poisson", "4", "pcg", 9, True)]


@pytest.mark.parametrize("wgcu", ["1", "2", "3"])
def test_fused_direction_pass_workgroups_per_cu(ctx, rs, monkeypatch, wgcu):
    """KRYST_SPMV_FUSE_WG_PER_CU pads the fused kernel's LDS request so that only that many workgroups fit a CU.  The run-of-tiles kernel caps
    the request at 64 KiB: 1 and 2 are the same launch at the five small shapes and only 3 differs.  The marching kernel's cap is 80 KiB
    (80, 79.5 and 52.8 KiB for 1, 2, 3): the 64^3 case, with the marching plan switched on, is where all three values are three launches."""
    monkeypatch.setenv("KRYST_CG_FUSE_P", "1"); monkeypatch.setenv("KRYST_SPMV_FUSE_WG_PER_CU", wgcu)
    for N, kind, T, method, cap, jac in FUSE_SHAPES:
        monkeypatch.setenv("KRYST_SPMV_FUSE_T", T)
        a = O.stencil7(N, kind)
        d = K.CsrMatrix.stencil7(N, kind, ctx=ctx) if N % 4 == 0 else to_dev(ctx, a)
        assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
        res = _cg_like(ctx, rs, a, d, method, cap, (wgcu, N, kind, T, method, cap), jacobi=jac)
        if cap == 400 and kind != "convdiff":
            assert res.converged and res.iterations < cap
    monkeypatch.setenv("KRYST_SPMV_FUSE_T", "4"); monkeypatch.setenv("KRYST_SPMV_FUSE_MARCH", "1")
    a = O.stencil7(64, "poisson")
    d = K.CsrMatrix.stencil7(64, "poisson", ctx=ctx)
    info = d.fuse_march_info()
    assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"] and info["eligible"] and info["on"], info
    _cg_like(ctx, rs, a, d, "cg", 9, (wgcu, 64, "marching"))


@pytest.mark.parametrize("reuse", ["0", "1"])
@pytest.mark.parametrize("N", [16, 40])
def test_pattern_kernel_takes_the_diagonal_operand_from_its_gather(ctx, rs, monkeypatch, N, reuse):
    """KRYST_SPMV_REUSE_DIAG: on a generator-made operator the unstaged pattern kernel fetches x[row - 1 .. row + 2] with two gathers and, in
    CG's p.Ap (the fused dot's vector is x itself), takes p[row] from them.  The staged form is switched off: it never reads the setting."""
    monkeypatch.setenv("KRYST_SPMV_STAGE", "0"); monkeypatch.setenv("KRYST_CG_FUSE_P", "0"); monkeypatch.setenv("KRYST_SPMV_REUSE_DIAG", reuse)
    a = O.stencil7(N, "poisson")
    d = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)
    assert d.encoding()[0] == "csr-p16" and not d.pattern_info()["staged"]
    x = O.splitmix64_uniform(7 + N, a.ncols) - 0.5
    assert np.array_equal(d.spmv(x), a.spmv(x))
    res = _cg_like(ctx, rs, a, d, "cg", 400, (N, reuse))
    assert res.converged and res.iterations < 400


# ================================================================================================================ ILU apply routes
ROUTES = {"direct": {"KRYST_ILU_GRAPH": "0", "KRYST_ILU_DIRECT_ARGS": "1"}, "eager": {"KRYST_ILU_GRAPH": "0", "KRYST_ILU_DIRECT_ARGS": "0"},
          "graph": {"KRYST_ILU_GRAPH": "1", "KRYST_ILU_DIRECT_ARGS": "0"}, "graph+direct": {"KRYST_ILU_GRAPH": "1", "KRYST_ILU_DIRECT_ARGS": "1"}}
QUAD = "grid 16x16 (tri_quad_kernel)"
KINDS = [("true", K.TrueIlu0, O.Pc.ilu0_true), ("compat", K.Ilu0, O.Pc.ilu0_compat), ("ilup1", lambda: K.Ilup(1), lambda a: O.Pc.ilup(a, 1))]


def box7(Ni, Nj, Nk):
    """the 7-point box operator of test_structured_grid_triangular_solve_bit_exact (unsymmetric, another weight per direction)"""
    import scipy.sparse as sp

    def lap(n, w):
        return sp.diags([-w * np.ones(n - 1), 2 * w * np.ones(n), -0.5 * w * np.ones(n - 1)], [-1, 0, 1])
    m = (sp.kron(sp.eye(Nk), sp.kron(sp.eye(Nj), lap(Ni, 1.0))) + sp.kron(sp.eye(Nk), sp.kron(lap(Nj, 0.7), sp.eye(Ni)))
         + sp.kron(lap(Nk, 0.3), sp.kron(sp.eye(Nj), sp.eye(Ni)))).tocsr()
    m.sort_indices(); m.eliminate_zeros()
    return O.Csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)


def level_cases():
    """the level-ordered factors of test_triangular_solve_forms_bit_exact"""
    rng = np.random.default_rng(77)
    dense = rng.random((300, 300)) * (rng.random((300, 300)) < 0.05) + np.diag(5.0 + rng.random(300))
    return [(K.TrueIlu0(), O.Pc.ilu0_true, O.stencil7(24, "aniso")), (K.Ilu0(), O.Pc.ilu0_compat, O.Csr.from_dense(dense, keep_zeros=False)),
            (K.Ilup(2), lambda a: O.Pc.ilup(a, 2), O.stencil7(9, "convdiff")),
            (K.Ilup(0), O.Pc.ilup0, O.Csr.from_dense(O.tridiag(700, -1.0, 2.5, -0.5), keep_zeros=False))]


def apply_on_every_route(monkeypatch, pc, ref, n, label, form=None, routes=ROUTES):
    for route, env in routes.items():
        with monkeypatch.context() as mp:
            setenv(mp, env)
            if form is not None:
                assert pc.ilu_info()["form"] == form, (label, route, pc.ilu_info())
            else:
                assert pc.ilu_info()["form"].startswith("level"), (label, route, pc.ilu_info())
            for seed in (1, 2, 3):
                r = O.splitmix64_uniform(seed, n) - 0.5
                got, want = pc.apply(r), ref.apply(r)
                assert np.array_equal(got, want), (label, route, seed, int(np.sum(got != want)))
            assert pc.ilu_info()["form"] == (form or pc.ilu_info()["form"]), (label, route, "the wavefront solve gave up")


@pytest.mark.parametrize("box", [(17, 9, 20), (24, 24, 24)], ids=lambda b: "x".join(map(str, b)))
def test_ilu_routes_on_the_16x16_grid_form(ctx, monkeypatch, box):
    """direct launch (the arguments in the kernel call), the argument block launched eagerly, and a captured graph over the argument block"""
    monkeypatch.setenv("KRYST_ILU_WAVE", "2")
    a = box7(*box)
    d = to_dev(ctx, a)
    for name, kcls, ofn in KINDS[:2]:
        apply_on_every_route(monkeypatch, kcls().setup(d), ofn(a), a.nrows, (box, name), form=QUAD)
    # Ilup(1)'s fill leaves the 7-point pattern: a box / level-ordered factor, which has no direct launch -- the same four settings
    pc = K.Ilup(1).setup(d)
    ref = O.Pc.ilup(a, 1)
    for route, env in ROUTES.items():
        with monkeypatch.context() as mp:
            setenv(mp, env)
            for seed in (1, 2, 3):
                r = O.splitmix64_uniform(seed, a.nrows) - 0.5
                assert np.array_equal(pc.apply(r), ref.apply(r)), (box, "ilup1", route, seed, pc.ilu_info()["form"])


@pytest.mark.parametrize("syncfree", ["0", "1"])
def test_ilu_routes_on_level_ordered_factors(ctx, monkeypatch, syncfree):
    """one launch per level / narrow run (many launches: a graph by default) and the sync-free single launch (eager by default), each both ways"""
    setenv(monkeypatch, {"KRYST_ILU_SYNCFREE": syncfree, "KRYST_ILU_GRID": "0", "KRYST_ILU_BOX": "0"})     # (no structured form for the stencils)
    for i, (kpc, ofn, a) in enumerate(level_cases()):
        apply_on_every_route(monkeypatch, kpc.setup(to_dev(ctx, a)), ofn(a), a.nrows, (syncfree, i))
    a = level_cases()[1][2]
    d = to_dev(ctx, a)
    for name, kcls, ofn in KINDS:
        apply_on_every_route(monkeypatch, kcls().setup(d), ofn(a), a.nrows, (syncfree, name))


def test_ilu_routes_on_a_27_point_box(ctx, monkeypatch):
    rng = np.random.default_rng(27)
    a = box_operator(rng, 9, 8, 8, lambda dk, dj, di: True)
    d = to_dev(ctx, a)
    monkeypatch.setenv("KRYST_ILU_BOX", "2")
    for name, kcls, ofn in KINDS:
        pc = kcls().setup(d)
        form = pc.ilu_info()["form"]
        assert form.startswith("box wavefront") == (name != "ilup1"), (name, form)        # (fill entries leave the 3 x 3 x 3 cube)
        apply_on_every_route(monkeypatch, pc, ofn(a), a.nrows, name, form=form)


def test_one_preconditioner_gives_the_same_bits_when_the_route_changes(ctx, monkeypatch):
    """six applies on ONE preconditioner: direct, argument block eager, graph, eager, graph, direct -- the wavefront kernels' flags carry the
    apply's number from either source, the graph is captured in the middle of the sequence and replayed after an eager apply"""
    sequence = ("direct", "eager", "graph", "eager", "graph", "direct")
    monkeypatch.setenv("KRYST_ILU_WAVE", "2")
    a = box7(24, 24, 24)
    rng = np.random.default_rng(6)
    boxa = box_operator(rng, 9, 8, 8, lambda dk, dj, di: True)
    lvl = level_cases()[1][2]
    for label, a_, kpc, ofn, form in (("grid", a, K.TrueIlu0(), O.Pc.ilu0_true, QUAD), ("grid-compat", a, K.Ilu0(), O.Pc.ilu0_compat, QUAD),
                                      ("box", boxa, K.TrueIlu0(), O.Pc.ilu0_true, "box"), ("level", lvl, K.Ilu0(), O.Pc.ilu0_compat, "level")):
        pc, ref = kpc.setup(to_dev(ctx, a_)), ofn(a_)
        assert pc.ilu_info()["form"].startswith(form), (label, pc.ilu_info())
        for k, route in enumerate(sequence):
            with monkeypatch.context() as mp:
                setenv(mp, ROUTES[route])
                r = O.splitmix64_uniform(100 + k, a_.nrows) - 0.5
                got, want = pc.apply(r), ref.apply(r)
            assert np.array_equal(got, want), (label, k, route, int(np.sum(got != want)))
        assert pc.ilu_info()["form"].startswith(form), (label, "the wavefront solve gave up")


# ================================================================================================================ the other ILU settings
@pytest.mark.parametrize("held", ["8", "16"])
def test_syncfree_csr_kernel_with_8_and_16_held_entries(ctx, monkeypatch, held):
    """tri_syncfree_csr_kernel<8> / <16> on factors with rows above 8 and above 16 entries: rows longer than what is held take the rest from memory"""
    monkeypatch.setenv("KRYST_ILU_SYNCFREE", "1"); monkeypatch.setenv("KRYST_ILU_GRID", "0"); monkeypatch.setenv("KRYST_ILU_BOX", "0")
    monkeypatch.setenv("KRYST_ILU_CSR_HELD", held)
    cases = level_cases()
    a9, dense = cases[2][2], cases[1][2]
    refs = [(K.Ilup(2), O.Pc.ilup(a9, 2), a9), (K.Ilu0(), O.Pc.ilu0_compat(dense), dense), (K.TrueIlu0(), O.Pc.ilu0_true(dense), dense)]
    # (ILU(0) keeps A's pattern: the longest row of the 300-row factor's strict lower part)
    rp, ci = np.asarray(dense.row_ptr), np.asarray(dense.col_idx)
    assert max(int(np.sum(ci[rp[i]:rp[i + 1]] < i)) for i in range(dense.nrows)) > 16
    for kpc, ref, a in refs:
        pc = kpc.setup(to_dev(ctx, a))
        assert pc.ilu_info()["form"].startswith("level"), pc.ilu_info()
        for seed in (1, 2, 3):
            r = O.splitmix64_uniform(seed, a.nrows) - 0.5
            assert np.array_equal(pc.apply(r), ref.apply(r)), (held, a.nrows, seed)


@pytest.fixture(scope="module")
def deep(ctx):
    a = KC.deep_factor()
    return a, to_dev(ctx, a), {"true": O.Pc.ilu0_true(a), "compat": O.Pc.ilu0_compat(a)}


def _deep_applies(deep, label):
    a, d, refs = deep
    for name, kcls, _ in KINDS[:2]:
        pc = kcls().setup(d)
        info = pc.ilu_info()
        assert info["form"].startswith("level") and min(info["levels"]) > 200, info
        for seed in (1, 2):
            r = O.splitmix64_uniform(seed, a.nrows) - 0.5
            assert np.array_equal(pc.apply(r), refs[name].apply(r)), (label, name, seed)


@pytest.mark.parametrize("threads", ["64", "256", "1024"])
def test_narrow_level_run_kernel_workgroup_sizes(deep, monkeypatch, threads):
    """tri_run_pipe_kernel with 64, 256 and 1 024 threads on the 40 000-row deep factor (levels narrower and wider than the workgroup)"""
    setenv(monkeypatch, {"KRYST_ILU_SYNCFREE": "0", "KRYST_ILU_RUN_FREE": "0", "KRYST_ILU_RUN_PIPE": "1", "KRYST_ILU_RUN_THREADS": threads})
    _deep_applies(deep, threads)


@pytest.mark.parametrize("pct", ["0", "2", "100"])
def test_share_of_long_rows_that_sends_a_factor_to_the_barrier_kernel(deep, monkeypatch, pct):
    """KRYST_ILU_FREE_LONG_PCT (read at set-up): the deep factor has 50 rows in 40 000 longer than eight entries -- 0.125 % --, so 2 and 100
    keep the barrier-free run kernel and 0 sends the factor to the barrier kernel"""
    setenv(monkeypatch, {"KRYST_ILU_SYNCFREE": "0", "KRYST_ILU_RUN_FREE": "1", "KRYST_ILU_FREE_LONG_PCT": pct})
    _deep_applies(deep, pct)


def box27_cases():
    """the box operators of test_box_stencil_triangular_solve_bit_exact, in its order and from its generator"""
    rng = np.random.default_rng(27)
    all27 = lambda dk, dj, di: True                                         # noqa: E731
    p19 = lambda dk, dj, di: abs(dk) + abs(dj) + abs(di) <= 2               # noqa: E731
    p9_2d = lambda dk, dj, di: dk == 0                                      # noqa: E731
    return [box_operator(rng, 5, 4, 3, all27), box_operator(rng, 9, 8, 8, all27), box_operator(rng, 17, 9, 10, all27),
            box_operator(rng, 12, 11, 7, p19), box_operator(rng, 40, 25, 1, p9_2d), box_operator(rng, 3, 3, 3, all27),
            box_operator(rng, 10, 9, 9, all27, drop=0.3), box_operator(rng, 33, 5, 6, all27, drop=0.05),
            box_operator(rng, 41, 30, 19, all27), box_operator(rng, 7, 26, 17, p19, drop=0.1),
            box_operator(rng, 13, 12, 11, all27, drop=0.1, zeros=0.1)]


@pytest.mark.parametrize("regular", ["0", "1"])
def test_box_kernels_with_run_time_stream_tests(ctx, monkeypatch, regular):
    """KRYST_ILU_BOX_REGULAR=0: the box wavefront kernel tests at run time which coefficient streams a row has, also on the factors whose
    sets are known at compile time (27-point, 19-point, Ilup(1) of a 7-point operator)"""
    monkeypatch.setenv("KRYST_ILU_BOX", "2"); monkeypatch.setenv("KRYST_ILU_BOX_REGULAR", regular)
    rng = np.random.default_rng(28)
    regular_seen = set()
    for case, a in enumerate(box27_cases()):
        d = to_dev(ctx, a)
        for name, kcls, ofn in (("true", K.TrueIlu0, O.Pc.ilu0_true), ("compat", K.Ilu0, O.Pc.ilu0_compat)):
            pc, ref = kcls().setup(d), ofn(a)
            info = pc.ilu_info()
            assert info["form"].startswith("box wavefront"), (case, name, info)
            regular_seen.add(info["regular"])
            for rep in range(2):
                r = rng.standard_normal(a.nrows)
                if rep == 0:
                    ctx.poison_lds()
                assert np.array_equal(pc.apply(r), ref.apply(r)), (regular, case, name)
            assert pc.ilu_info()["form"] == info["form"], (case, name, "the wavefront solve gave up and fell back")
    assert regular_seen == {True, False}
    # Ilup(1) of a 7-point operator: the third compile-time set (fill entries inside the 3 x 3 x 3 cube)
    a = box7(12, 9, 10)
    pc = K.Ilup(1).setup(to_dev(ctx, a))
    assert pc.ilu_info()["form"].startswith("box wavefront"), pc.ilu_info()
    r = rng.standard_normal(a.nrows)
    assert np.array_equal(pc.apply(r), O.Pc.ilup(a, 1).apply(r))


@pytest.mark.parametrize("group", ["1", "3", "16"])
def test_ilup_row_pipeline_with_groups_of_host_threads(ctx, monkeypatch, group):
    """KRYST_ILUP_CPU_GROUP with four host threads and blocks of 8 rows, in the manner of test_ilup_row_pipeline_over_host_threads_bit_exact"""
    setenv(monkeypatch, {"KRYST_ILUP_THREADS": "4", "KRYST_ILUP_BLOCK": "8", "KRYST_ILUP_CPU_GROUP": group})
    rng = np.random.default_rng(77)
    dm = rng.random((90, 90)) * (rng.random((90, 90)) < 0.1) + np.diag(4.0 + rng.random(90))
    for a in (O.stencil7(9, "convdiff"), O.stencil7(8, "poisson"), O.Csr.from_dense(dm, keep_zeros=False)):
        for fill in (1, 2, 3):
            r = rng.standard_normal(a.nrows)
            assert np.array_equal(K.Ilup(fill).setup(to_dev(ctx, a)).apply(r), O.Pc.ilup(a, fill).apply(r)), (group, fill, a.nrows)


# ================================================================================================================ Chebyshev polynomial
LO, HI = 0.07, 2.3


@pytest.mark.parametrize("knob", ["0", "1"])
@pytest.mark.parametrize("name", ["ragged-2003", "stencil7-17"])
def test_chebyshev_polynomial_fused_and_unfused_on_the_same_operator(ctx, monkeypatch, name, knob):
    """KRYST_CHEB_POLY_FUSE (read at set-up): 0 the unfused step on an operator whose default is the fused one (plain CSR), 1 the fused step --
    it walks the plain CSR arrays -- on an operator whose own SpMV streams a compressed form"""
    a = MR.ragged() if name == "ragged-2003" else O.stencil7(17, "convdiff")
    d = to_dev(ctx, a)
    assert (d.encoding()[0] == "csr") == (name == "ragged-2003"), d.encoding()
    r = np.random.default_rng(len(name)).standard_normal(a.nrows)
    r[::7] = -0.0
    w = CP.jacobi_w(a)
    monkeypatch.setenv("KRYST_CHEB_POLY_FUSE", knob)
    for jac in (False, True):
        for m in (0, 1, 4):
            pc = K.ChebyshevPoly(m, LO, HI, jacobi=jac).setup(d)
            assert pc.info()["fused"] == (knob == "1"), (name, knob, pc.info())
            want = CP.apply(a, r, m, LO, HI, w if jac else None)
            got = pc.apply(r)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, knob, jac, m, int(np.sum(got.view(np.uint64) != want.view(np.uint64))))
            assert np.array_equal(pc.apply(r).view(np.uint64), got.view(np.uint64))


# ================================================================================================================ settings read once per process
WORKER = os.path.join(ROOT, "tests", "knob_worker.py")
_child_died = []                        # a child that ended on a signal or at its time limit: nothing more is started


def worker_reference(solver, a, b, mx, rs):
    jac = O.Pc.jacobi(a)
    tol = KC.WORKER_TOL
    if solver == "gmres5_right_jacobi":
        return O.solve("gmres", a, b, pc=jac, tol=tol, max_iters=mx, restart=5, side=int(PCN.Right), rs=rs)
    if solver == "fgmres5_classical":
        return O.solve("fgmres", a, b, pc=jac, tol=tol, max_iters=mx, restart=5, orthog=int(K.Orthog.Classical), rs=rs)
    if solver == "fgmres5_modified":
        return O.solve("fgmres", a, b, pc=jac, tol=tol, max_iters=mx, restart=5, orthog=int(K.Orthog.Modified), rs=rs)
    if solver == "pca5_right_jacobi":
        return PR.as_written(a, b, pc=jac, side=int(PCN.Right), restart=5, tol=tol, max_iters=mx, rs=rs)
    assert solver == "sstep3_5_right_jacobi"
    return PR.sstep(a, b, pc=jac, side=2, restart=5, block_size=3, tol=tol, max_iters=mx, rs=rs)


@pytest.fixture(scope="module")
def worker_references(rs):
    """(solver, N, max_iters) -> the oracle's or the restatement's result, computed once for both profiles"""
    out = {}
    for solver, N, mx in KC.WORKER_CASES:
        a = O.stencil7(N, "convdiff")
        out[(solver, N, mx)] = worker_reference(solver, a, a.spmv(np.ones(a.nrows)), mx, rs)
    return out


@pytest.mark.parametrize("profile", list(KC.PROFILES))
def test_solver_pass_grids_read_once_per_process(tmp_path, worker_references, num_cu, profile):
    """GMRES(5), FGMRES(5) classical and modified, PCA-GMRES as written and s-step GMRES (s = 3) in a fresh process whose four
    *_BLOCKS_PER_CU settings are 1 (and the vector arena off) or 8.  What each profile is there to reach is asserted from the device's CU
    count first (knob_cases.profile_conditions): at 64^3 the GMRES, PCA-GMRES and inner-product passes of the low profile stride; FGMRES's
    passes take max(value, their own BPC), so 1 selects nothing for them and they stride at 102^3 on their default grids; at 102^3 every
    pass of the high profile runs a grid that is not its default one and strides."""
    if _child_died:
        pytest.skip("an earlier child ended on a signal or at its time limit: " + _child_died[0])
    wrong = [what for what, holds in KC.profile_conditions(profile, num_cu) if not holds]
    assert wrong == [], (profile, num_cu, wrong)
    env = dict(os.environ, **KC.PROFILES[profile])
    for k in KC.PER_PROCESS_BPC + ("KRYST_NO_ARENA",):
        if k not in KC.PROFILES[profile]:
            env.pop(k, None)
    out = os.path.join(str(tmp_path), "out.npz")
    limit = 60 + 12 * len(KC.WORKER_CASES)              # start-up and two operators, then a few seconds per case at the most
    try:
        p = subprocess.run([sys.executable, WORKER, out], env=env, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _child_died.append(f"profile {profile}: no end after {limit} s")
        pytest.fail(f"the worker did not end within {limit} s\n{(e.stdout or b'')[-3000:]}")
    if p.returncode < 0:
        _child_died.append(f"profile {profile}: signal {-p.returncode}")
    assert p.returncode == 0, f"exit code {p.returncode}\n{p.stdout[-3000:]}"
    got = np.load(out)
    assert [str(s) for s in got["profile_env"]] == [f"{k}={v}" for k, v in sorted(KC.PROFILES[profile].items())]
    for solver, N, mx in KC.WORKER_CASES:
        ref = worker_references[(solver, N, mx)]
        key = f"{solver}_{N}"
        st = got[key + "__stats"]
        nan_ok = solver.startswith("pca5")
        assert (int(st[0]), bool(st[1])) == (ref.iterations, bool(ref.converged)), (profile, key, st, ref.iterations, ref.converged)
        assert np.array_equal(got[key + "__hist"], np.array(ref.history, dtype=float), equal_nan=nan_ok), (profile, key, "residual history")
        assert np.array_equal(st[2:3], [ref.final_residual], equal_nan=nan_ok), (profile, key, st[2], ref.final_residual)
        assert np.array_equal(got[key + "__x"], ref.x, equal_nan=nan_ok), (profile, key, int(np.sum(got[key + "__x"] != ref.x)))
        assert ref.iterations > 0
