"""Results depend on the first n elements of a vector only: every kernel with something behind every operand's end.

A device vector of n elements is allocated as ceil(n / 512) * 512 + 512 doubles, zero at creation, and kernels read past n on purpose: the
16-byte pair loads of the pointwise kernels, the clamped windows of the staged CSR-P16 kernels, the shifted loads of the CSR-DIA kernel,
the gathers of the generator-made operators, the four-lanes-per-line loaders of the grid triangular solves, block Jacobi's shuffles in a
short last block.  The pointwise kernels also WRITE the whole last tile, so a NaN coefficient leaves NaNs there.  Whether each read is
masked, or merely lucky because the padding is zero, is what this file pins: kryst_bench_vec_padding (DeviceVec.poison_padding) fills the
rest of the last tile AND the extra tile -- where every over-read lands when n is a multiple of 512 -- of every operand, inputs and outputs.

Every case: clean data uploaded, the padding of every vector operand poisoned (asserted: padding_dirty() == ceil(n/512)*512 + 512 - n),
the operation run, the first n results compared IN ALL 64 BITS with the reference of that operation (the oracle or the numpy reference
the kind's own tests use) and with the same call on clean vectors.  Two poisons: the quiet NaN 0x7FF8000000000000 (never the bits of
KR_TRI_SENTINEL or of the CSR-DIA marker: those are "not written yet" / "absent" by contract) and the finite 1e300 (a kernel that
multiplies the padding by zero survives the second and not the first; one that adds it survives neither).  What the padding holds after
an operation is unspecified and not asserted.  There is no GMRES stepping session in the ABI (kryst_session_begin: methods 0..9): the
stepping cases are CG and BiCGStab."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import nonfinite_cases as C
import krylov_ext_ref as KR
import pca_gmres_ref as PR
import sor_ref as S
import bjacobi_ref as BR

pytestmark = pytest.mark.gpu

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
POISONS = {"qnan": QNAN, "1e300": 1e300}
assert all(np.float64(v).view(np.uint64) not in (np.uint64(C.TRI_SENTINEL_BITS), np.uint64(0x7FF8D1A0D1A0D1A0)) for v in POISONS.values())
PCN = K.Preconditioning


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


@pytest.fixture(params=list(POISONS), ids=list(POISONS))
def poison(request):
    return POISONS[request.param]


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return bool(np.array_equal(bits(got), bits(want)))


def pad_count(n):
    return -(-n // 512) * 512 + 512 - n


def pvec(ctx, data, poison):
    """`data` in a vector whose padding holds `poison` (None: a clean vector); asserts the padding is dirty, all of it."""
    v = ctx.vec(np.asarray(data, dtype=np.float64))
    assert v.padding_dirty() == 0
    if poison is not None:
        v.poison_padding(poison)
        assert v.padding_dirty() == pad_count(len(v)), (len(v), v.padding_dirty())
    return v


def test_the_hook_counts_and_fills_the_padding_and_nothing_else(ctx):
    for n in (1, 511, 512, 513, 1024):
        x = np.arange(n) + 1.0
        v = ctx.vec(x)
        assert v.padding_dirty() == 0
        for p in POISONS.values():
            v.poison_padding(p)
            assert v.padding_dirty() == pad_count(n) and same_bits(v.to_host(), x)
        v.poison_padding(0.0)
        assert v.padding_dirty() == 0
        v.poison_padding(-0.0)                                  # anything but +0.0 counts
        assert v.padding_dirty() == pad_count(n)


# ------------------------------------------------------------------------------------------------ BLAS-1
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1024])
def test_blas1(ctx, rs, n, poison):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    for p in (None, poison):
        label = ("clean" if p is None else "poisoned", n)
        assert bits([K.dot(pvec(ctx, x, p), pvec(ctx, y, p))])[0] == bits([O.dot(x, y, rs)])[0], ("dot",) + label
        assert bits([K.norm(pvec(ctx, x, p))])[0] == bits([O.norm(x, rs)])[0], ("norm",) + label
        dx, dy = pvec(ctx, x, p), pvec(ctx, y, p)
        K.axpy(0.37, dx, dy)
        assert same_bits(dy.to_host(), y + 0.37 * x), ("axpy",) + label
        dy = pvec(ctx, y, p)
        K.aypx(-1.25, dx, dy)
        assert same_bits(dy.to_host(), x + -1.25 * y), ("aypx",) + label
        out = pvec(ctx, np.full(n, np.nan), p)
        assert same_bits(K.sub(dx, pvec(ctx, y, p), out).to_host(), x - y), ("sub",) + label
        # the result of a pointwise kernel (its padding is whatever the kernel left) feeds an inner product
        assert bits([K.dot(out, dx)])[0] == bits([O.dot(x - y, x, rs)])[0], ("dot of sub's output",) + label
        dst = pvec(ctx, np.zeros(n), p).copy_from(dx)
        assert same_bits(dst.to_host(), x) and bits([K.dot(dst, pvec(ctx, y, p))])[0] == bits([O.dot(x, y, rs)])[0], ("copy, dot",) + label


# ------------------------------------------------------------------------------------------------ SpMV, every storage form
def random_csr(rng, nrows, ncols, row_len):
    rp = [0]; ci = []; va = []
    for _ in range(nrows):
        k = min(int(row_len()), ncols)
        cols = np.sort(rng.choice(ncols, size=k, replace=False)) if k else np.array([], dtype=np.int64)
        ci.extend(cols.tolist()); va.extend(rng.standard_normal(k).tolist()); rp.append(len(ci))
    return O.Csr(nrows, ncols, rp, ci, va)


def banded(rng, n, offs):
    import scipy.sparse as sp
    rows, cols, vs = [], [], []
    for o in offs:
        i = np.arange(max(0, -o), min(n, n - o))
        rows.append(i); cols.append(i + o); vs.append(rng.standard_normal(len(i)))
    m = sp.csr_matrix((np.concatenate(vs), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)); m.sort_indices()
    return O.Csr(n, n, m.indptr, m.indices, m.data)


def box7(ni, nj, nk, vals=(6.0, -1.0, -1.5, -0.25)):
    """the 7-point box of test_spmv_pattern_kernel_with_staged_window_bit_exact (four distinct values: a CSR-P16 operator)"""
    import scipy.sparse as sp
    e = lambda n: sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1])           # noqa: E731
    I = sp.identity
    m = (vals[0] * I(ni * nj * nk) + vals[1] * sp.kron(I(nk), sp.kron(I(nj), e(ni))) + vals[2] * sp.kron(I(nk), sp.kron(e(nj), I(ni))) +
         vals[3] * sp.kron(e(nk), I(nj * ni))).tocsr()
    m.sort_indices()
    return O.Csr(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)


def box7_random(rng, ni, nj, nk):
    """the 7-point box of test_spmv_slab_order_of_the_tiles_bit_exact, values from a set of three"""
    import scipy.sparse as sp
    e = lambda n: sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])   # noqa: E731
    pat = (sp.kron(sp.identity(nk), sp.kron(sp.identity(nj), e(ni))) + sp.kron(sp.identity(nk), sp.kron(e(nj), sp.identity(ni))) +
           sp.kron(e(nk), sp.identity(nj * ni))).tocsr()
    pat.sort_indices()
    return O.Csr(pat.shape[0], pat.shape[1], pat.indptr, pat.indices, rng.choice([-1.0, 6.0, 0.5], pat.nnz))


def tridiag(n):
    return O.Csr.from_dense(O.tridiag(n, -1.0, 2.0, 0.5), keep_zeros=False)


PLAIN = {"KRYST_SPMV_COMPRESS": "0", "KRYST_SPMV_DIA": "0"}
DIA = {"KRYST_SPMV_DIA": "2", "KRYST_SPMV_COMPRESS": "1"}
# id: (settings, operator(rng) -> oracle Csr, the form encoding() must name, staged (None: not CSR-P16))
SPMV_CASES = {}
for _k, _s in (("kernel2", {"KRYST_SPMV_KERNEL": "2"}), ("kernel3", {"KRYST_SPMV_KERNEL": "3"}),
               ("kernel2-slots4", {"KRYST_SPMV_KERNEL": "2", "KRYST_SPMV_SLOTS": "4"}), ("kernel2-slots7", {"KRYST_SPMV_KERNEL": "2", "KRYST_SPMV_SLOTS": "7"})):
    SPMV_CASES[f"csr-{_k}-1000x777"] = (dict(PLAIN, **_s), lambda rng: random_csr(rng, 1000, 777, lambda: rng.integers(0, 12)), "csr", None)
    SPMV_CASES[f"csr-{_k}-513"] = (dict(PLAIN, **_s), lambda rng: random_csr(rng, 513, 513, lambda: rng.integers(0, 3)), "csr", None)
    SPMV_CASES[f"csr-{_k}-1024"] = (dict(PLAIN, **_s), lambda rng: random_csr(rng, 1024, 1024, lambda: rng.integers(0, 9)), "csr", None)
for _n in (1501, 1536):
    SPMV_CASES[f"d8-banded{_n}"] = ({"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "1", "KRYST_SPMV_DIA": "0"}, lambda rng, n=_n: tridiag(n), "csr-d8", None)
    SPMV_CASES[f"d16-banded{_n}"] = ({"KRYST_SPMV_KERNEL": "3", "KRYST_SPMV_COMPRESS": "2", "KRYST_SPMV_DIA": "0"}, lambda rng, n=_n: tridiag(n), "csr-d16", None)
SPMV_CASES["p16-unstaged-9x16x16"] = ({"KRYST_SPMV_STAGE": "1"}, lambda rng: box7(9, 16, 16), "csr-p16", False)
for _b in ((8, 9, 40), (64, 64, 9), (8, 8, 8)):
    SPMV_CASES["p16-staged-%dx%dx%d" % _b] = ({"KRYST_SPMV_STAGE": "1"}, lambda rng, b=_b: box7(*b), "csr-p16", True)
SPMV_CASES["dia-9-diagonals-4099"] = (DIA, lambda rng: banded(rng, 4099, [-1200, -35, -34, -1, 0, 1, 34, 35, 1200]), "csr-dia", None)
SPMV_CASES["dia-tridiagonal-1024"] = (DIA, lambda rng: banded(rng, 1024, [-1, 0, 1]), "csr-dia", None)
SPMV_CASES["dia-varcoef-21"] = (DIA, lambda rng: O.stencil7(21, "varcoef"), "csr-dia", None)


def spmv_both(ctx, d, a, x, poison, transpose=False):
    """y of the clean and of the poisoned run: every element of both must be the reference's"""
    want = KR.transpose(a).spmv(x) if transpose else a.spmv(x)
    out = []
    for p in (None, poison):
        xv, yv = pvec(ctx, x, p), pvec(ctx, np.full(len(want), np.nan), p)
        (d.spmv_transpose if transpose else d.spmv)(xv, yv)
        out.append(yv.to_host())
    assert same_bits(out[0], want), "the clean run differs from the reference"
    assert same_bits(out[1], want), ("the padding reached y", int(np.sum(bits(out[1]) != bits(want))), np.flatnonzero(bits(out[1]) != bits(want))[:8])


@pytest.mark.parametrize("name", list(SPMV_CASES))
def test_spmv_forms(ctx, name, poison, monkeypatch):
    env, make, form, staged = SPMV_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(44)
    a = make(rng)
    d = to_dev(ctx, a)
    assert d.encoding()[0] == form, (name, d.encoding())
    if staged is not None:
        assert d.pattern_info()["staged"] == staged, (name, d.pattern_info())
    spmv_both(ctx, d, a, rng.standard_normal(a.ncols), poison)


@pytest.mark.parametrize("N", [1, 7, 8, 17])
def test_spmv_on_generator_made_operators(ctx, N, poison):
    a = O.stencil7(N)
    spmv_both(ctx, K.CsrMatrix.stencil7(N, "poisson", ctx=ctx), a, O.splitmix64_uniform(0xC0FFEE + N, a.ncols) - 0.5, poison)


def test_spmv_in_the_slab_order_of_the_tiles(ctx, poison, monkeypatch):
    """box 128 x 128 x 7 of test_spmv_slab_order_of_the_tiles_bit_exact with its lowered thresholds, plain CSR"""
    for k, v in dict(PLAIN, KRYST_SPMV_ORDER="2", KRYST_SPMV_ORDER_MIN_PLANE="8192").items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(77)
    a = box7_random(rng, 128, 128, 7)
    d = to_dev(ctx, a)
    assert d.encoding()[0] == "csr" and d.tile_order()["in_use"] and d.tile_order()["plane_rows"] > 0, d.tile_order()
    spmv_both(ctx, d, a, rng.standard_normal(a.ncols), poison)


def test_spmv_transpose(ctx, poison):
    rng = np.random.default_rng(7)
    a = random_csr(rng, 1000, 777, lambda: rng.integers(0, 12))
    spmv_both(ctx, to_dev(ctx, a), a, rng.standard_normal(a.nrows), poison, transpose=True)


# ------------------------------------------------------------------------------------------------ whole solves
def run_dev(ctx, solver, d, pc, b, x0, poison, call="solve"):
    """-> (code, stats, solver, x) of a device-resident solve with b and x0 in vectors whose padding holds `poison`"""
    bv, xv = pvec(ctx, b, poison), pvec(ctx, x0, poison)
    code = 0
    try:
        st = getattr(solver, call)(d, pc, bv, xv)
    except K.KError as e:
        code, st = e.code, e.stats
    assert same_bits(bv.to_host(), b), "the solve changed b"
    return code, st, solver, xv.to_host()


def check_solve(ref, ref_code, got, label, nan_ok=False):
    code, st, s, x = got
    assert code == ref_code, (label, code, ref_code)
    assert st is not None and (st.iterations, bool(st.converged)) == (ref.iterations, bool(ref.converged)), (label, st, ref.iterations, ref.converged)
    h, rh = np.array(s.residual_history, dtype=float), np.array(ref.history, dtype=float)
    if nan_ok:
        assert C.same_ieee(h, rh) and C.same_ieee(x, ref.x) and C.same_ieee([st.final_residual], [ref.final_residual]), label
    else:
        assert same_bits(h, rh), (label, "history")
        assert same_bits([st.final_residual], [ref.final_residual]), (label, "final residual")
        assert same_bits(x, ref.x), (label, "x", int(np.sum(bits(x) != bits(ref.x))))


def _oracle(method, **kw):
    def f(a, b, x0, opc, tol, mx, rs):
        res = O.solve(method, a, b, x0=x0, pc=opc, tol=tol, max_iters=mx, rs=rs, raise_on_error=False, **kw)
        return res, res.code
    return f


def _ext(method):
    return lambda a, b, x0, opc, tol, mx, rs: (KR.SOLVERS[method](a, b, x0, tol, mx, rs), 0)


# name: (reference(a, b, x0, oracle pc, tol, max_iters, rs) -> (result, code), device solver(tol, max_iters), operator kind, takes a
# preconditioner, NaN-tolerant compare (the references of these run into 0 / 0 at exact convergence, as their own tests allow))
SOLVERS = {
    "cg": (_oracle("cg"), lambda t, m: K.CgSolver(t, m), "poisson", False, False),
    "pcg": (_oracle("pcg"), lambda t, m: K.PcgSolver(t, m), "poisson", True, False),
    "bicgstab": (_oracle("bicgstab"), lambda t, m: K.BiCgStabSolver(t, m), "convdiff", False, False),
    "bicgstab_rpc": (_oracle("bicgstab_rpc"), lambda t, m: K.BiCgStabRightPcSolver(t, m), "convdiff", True, False),
    "gmres_nopc": (_oracle("gmres", restart=12, side=0), lambda t, m: K.GmresSolver(12, t, m).with_preconditioning(PCN.NoPc), "convdiff", False, False),
    "gmres_left": (_oracle("gmres", restart=12, side=1), lambda t, m: K.GmresSolver(12, t, m).with_preconditioning(PCN.Left), "convdiff", True, False),
    "gmres_right": (_oracle("gmres", restart=12, side=2), lambda t, m: K.GmresSolver(12, t, m).with_preconditioning(PCN.Right), "convdiff", True, False),
    "gmres_lefttextbook": (_oracle("gmres", restart=12, side=3), lambda t, m: K.GmresSolver(12, t, m).with_preconditioning(PCN.LeftTextbook), "convdiff", True, False),
    "fgmres": (_oracle("fgmres", restart=16, orthog=1), lambda t, m: K.FgmresSolver(t, m, 16).with_orthog(K.Orthog.Modified), "convdiff", True, False),
    "pca_gmres": (lambda a, b, x0, opc, tol, mx, rs: (PR.as_written(a, b, x=x0, pc=opc, side=2, restart=5, tol=tol, max_iters=mx, rs=rs), 0),
                  lambda t, m: K.PcaGmresSolver(5, 2, 1, t, m).with_preconditioning(PCN.Right), "convdiff", True, True),
    "pca_gmres_textbook": (lambda a, b, x0, opc, tol, mx, rs: (PR.sstep(a, b, x=x0, pc=opc, side=2, restart=16, block_size=4, tol=tol, max_iters=mx, rs=rs), 0),
                           lambda t, m: K.PcaGmresSolver(16, 1, 4, t, m).with_preconditioning(PCN.Right).with_textbook(), "convdiff", True, False),
    "cgs": (_oracle("cgs"), lambda t, m: K.CgsSolver(t, m), "convdiff", False, False),
    "tfqmr": (_oracle("tfqmr"), lambda t, m: K.TfqmrSolver(t, m), "convdiff", False, False),
    "minres": (_ext("minres"), lambda t, m: K.MinresSolver(t, m), "poisson", False, False),
    "qmr": (_ext("qmr"), lambda t, m: K.QmrSolver(t, m), "convdiff", False, False),
    "cgnr": (_ext("cgnr"), lambda t, m: K.CgnrSolver(t, m), "convdiff", False, True),
    "minres_textbook": (_ext("minres_textbook"), lambda t, m: K.MinresSolver(t, m).with_textbook(), "poisson", False, False),
    "cgnr_textbook": (_ext("cgnr_textbook"), lambda t, m: K.CgnrSolver(t, m).with_textbook(), "convdiff", False, False),
}
PCS = {"none": (None, None), "jacobi": (K.Jacobi, O.Pc.jacobi), "ilu": (K.TrueIlu0, O.Pc.ilu0_true)}
SOLVER_CASES = [(s, p) for s, spec in SOLVERS.items() for p in (("jacobi", "ilu") if spec[3] else ("none",))]


@pytest.mark.parametrize("N", [9, 8])
@pytest.mark.parametrize("solver,pcname", SOLVER_CASES, ids=[f"{s}-{p}" for s, p in SOLVER_CASES])
def test_every_solver(ctx, rs, solver, pcname, N):
    """b and a non-zero x0 in poisoned vectors (the work vectors inherit the dirt through the padded copies of b and x), 729 and 512 rows"""
    ref_fn, make, kind, _, nan_ok = SOLVERS[solver]
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x0 = O.splitmix64_uniform(0xABC, a.nrows) - 0.5
    kcls, ofn = PCS[pcname]
    with np.errstate(all="ignore"):
        ref, ref_code = ref_fn(a, b, x0, ofn(a) if ofn else None, 1e-9, 40, rs)
    assert ref.iterations > 0
    pc = kcls().setup(d) if kcls else None
    call = "solve_flex" if solver == "fgmres" else "solve"
    for label, p in [("clean", None)] + list(POISONS.items()):
        check_solve(ref, ref_code, run_dev(ctx, make(1e-9, 40), d, pc, b, x0, p, call), (solver, pcname, N, label), nan_ok)


FORMS = {   # one small operator per storage form: (settings, operator, generator-made, the form, staged)
    "csr": (dict(PLAIN, KRYST_SPMV_KERNEL="3"), 9, "poisson", False, "csr", None),
    "csr-kernel2": (dict(PLAIN, KRYST_SPMV_KERNEL="2"), 8, "poisson", False, "csr", None),
    "csr-d8": ({"KRYST_SPMV_COMPRESS": "1", "KRYST_SPMV_DIA": "0"}, 9, "poisson", False, "csr-d8", None),
    "csr-d16": ({"KRYST_SPMV_COMPRESS": "2", "KRYST_SPMV_DIA": "0"}, 9, "poisson", False, "csr-d16", None),
    "csr-p16": ({"KRYST_SPMV_COMPRESS": "3"}, 9, "poisson", False, "csr-p16", False),
    "csr-p16-staged": ({"KRYST_SPMV_COMPRESS": "3", "KRYST_SPMV_STAGE": "1"}, 8, "poisson", False, "csr-p16", True),
    "csr-dia": (DIA, 9, "varcoef", False, "csr-dia", None),
    "csr-dia-512": (DIA, 8, "varcoef", False, "csr-dia", None),
    "generator": ({}, 8, "poisson", True, "csr-p16", True),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_fused_inner_products_on_every_form(ctx, rs, form, poison, monkeypatch):
    """CG ((p, Ap) inside the SpMV) and BiCGStab (two fused inner products) with b and x0 in poisoned vectors"""
    env, N, kind, generated, enc, staged = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = O.stencil7(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx) if generated else to_dev(ctx, a)
    assert d.encoding()[0] == enc, (form, d.encoding())
    if staged is not None:
        assert d.pattern_info()["staged"] == staged, (form, d.pattern_info())
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x0 = O.splitmix64_uniform(0xABC, a.nrows) - 0.5
    for name, cls, tol in (("cg", K.CgSolver, 1e-9), ("bicgstab", K.BiCgStabSolver, 1e-7 * np.linalg.norm(b))):
        ref = O.solve(name, a, b, x0=x0, tol=tol, max_iters=60, rs=rs)
        for p in (None, poison):
            check_solve(ref, 0, run_dev(ctx, cls(tol, 60), d, None, b, x0, p), (form, name, "clean" if p is None else "poisoned"))


@pytest.mark.parametrize("xbatch", ["1", "3", "8"])
@pytest.mark.parametrize("N,kind", [(16, "poisson"), (10, "aniso")])
def test_direction_pass_inside_the_spmv(ctx, rs, N, kind, xbatch, poison, monkeypatch):
    """the shapes of test_direction_pass_inside_the_spmv_on_every_exit_path: CG / PCG with p = z + beta p_old formed inside the staged
    SpMV and x updated in batches, run to convergence and to a cap inside a batch"""
    monkeypatch.setenv("KRYST_CG_FUSE_P", "1"); monkeypatch.setenv("KRYST_SPMV_FUSE_T", "2"); monkeypatch.setenv("KRYST_CG_X_BATCH", xbatch)
    a = O.stencil7(N, kind)
    d = K.CsrMatrix.stencil7(N, kind, ctx=ctx) if N % 4 == 0 else to_dev(ctx, a)
    assert d.encoding()[0] == "csr-p16" and d.pattern_info()["staged"]
    b = O.splitmix64_uniform(0xD0E + N, a.nrows)
    x0 = O.splitmix64_uniform(0xABC, a.nrows)
    for name, cls, opc, kpc in (("cg", K.CgSolver, None, None), ("pcg", K.PcgSolver, O.Pc.jacobi(a), K.Jacobi().setup(d))):
        for cap in (5, 400):
            ref = O.solve(name, a, b, pc=opc, x0=x0, tol=1e-9, max_iters=cap, rs=rs)
            for p in (None, poison):
                check_solve(ref, 0, run_dev(ctx, cls(1e-9, cap), d, kpc, b, x0, p), (name, N, xbatch, cap, "clean" if p is None else "poisoned"))


@pytest.mark.parametrize("method,kind", [("cg", "poisson"), ("bicgstab", "convdiff")])
@pytest.mark.parametrize("N", [9, 8])
def test_stepping_sessions(ctx, rs, method, kind, N, poison):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    b = a.spmv(np.linspace(0.5, 1.5, a.nrows))
    x0 = O.splitmix64_uniform(0xABC, a.nrows) - 0.5
    steps = (3, 4, 1)
    ref = O.solve(method, a, b, x0=x0, tol=1e-30, max_iters=sum(steps), rs=rs)
    for p in (None, poison):
        bv, xv = pvec(ctx, b, p), pvec(ctx, x0, p)
        with K.Session(method, d, None, bv, xv, tol=1e-30, max_iters=1000) as sess:
            for q in steps:
                sess.step(q)
            st = sess.end()
        assert st.iterations == ref.iterations and same_bits(sess.residual_history, ref.history) and same_bits(xv.to_host(), ref.x), (method, N, p)


# ------------------------------------------------------------------------------------------------ every preconditioner apply
def _pow2_cases():
    """one 512-row operator for the kinds whose cases of nonfinite_cases.py have no n that is a multiple of 512"""
    op = lambda: O.stencil7(8, "convdiff")                                 # noqa: E731

    def bj_ref(a, bsize):
        gs, inv, zp = BR.tiles_uniform(a.row_ptr, a.col_idx, a.vals, a.nrows, bsize)
        return C._approx_inverse(*BR.m_ref_uniform(a.nrows, bsize, inv), a.nrows)

    def sor_ref(a):
        plan = S.Plan(a, 0.0, None, False)
        return lambda r: plan.apply(r, 1.5, 2, S.SYMMETRIC_SWEEP)
    return [C.Case("jacobi-512", op, lambda a: O.Pc.jacobi(a).apply, lambda K, d: K.Jacobi().setup(d)),
            C.Case("ilu-grid-512", op, lambda a: O.Pc.ilu0_true(a).apply, lambda K, d: K.TrueIlu0().setup(d),
                   env={"KRYST_ILU_GRID": "1", "KRYST_ILU_WAVE": "2"}, form="grid"),
            C.Case("block-jacobi-uniform8-512", op, lambda a: bj_ref(a, 8), lambda K, d: K.BlockJacobi.uniform(8).setup(d)),
            C.Case("block-jacobi-uniform24-512", op, lambda a: bj_ref(a, 24), lambda K, d: K.BlockJacobi.uniform(24).setup(d)),   # a last block of 8 rows
            C.Case("sor-symmetric-512", op, sor_ref,
                   lambda K, d: K.Sor(1.5, 2, 1, K.MatSorType.SYMMETRIC_SWEEP | K.MatSorType.LOCAL_FORWARD_SWEEP, 0.0).setup(d))]


APPLY_CASES = C.apply_cases() + C.spai_cases() + _pow2_cases()


@pytest.mark.parametrize("case", APPLY_CASES, ids=lambda c: c.id)
def test_every_preconditioner_apply(ctx, case, monkeypatch):
    """r: clean data in a poisoned vector; z: NaN in its n elements (no kind here may read them) and poison behind them.  Both poisons on
    one object, then a clean apply on it that must equal a fresh object's: a captured graph or a re-armed buffer keeps nothing."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    a = case.op()
    n = a.nrows
    d = to_dev(ctx, a)
    fresh, used = case.dev(K, d), case.dev(K, d)
    ref = case.dev_ref(used) if case.dev_ref else case.ref(a)
    form = None
    if case.form:
        form = used.ilu_info()["form"]
        assert form.startswith(case.form), (case.id, form)
        assert case.min_levels == 0 or min(used.ilu_info()["levels"]) > case.min_levels, (case.id, used.ilu_info())
    r0 = C.clean_r(n)
    want = ref(r0)

    def apply(pc, p):
        z = pvec(ctx, np.full(n, np.nan), p)
        pc.apply(pvec(ctx, r0, p), z)
        return z.to_host()
    assert same_bits(apply(fresh, None), want), (case.id, "the clean apply differs from the reference")
    for label, p in POISONS.items():
        got = apply(used, p)
        assert same_bits(got, want), (case.id, label, int(np.sum(bits(got) != bits(want))), np.flatnonzero(bits(got) != bits(want))[:8])
        assert same_bits(apply(used, None), want), (case.id, label, "the apply with poisoned padding left something behind")
        if form is not None:
            assert used.ilu_info()["form"] == form, (case.id, label, "the solve gave up and fell back")


def test_amg_as_written_reads_z(ctx, poison):
    """apply_recursive (amg.rs:200-250) starts the finest level from the incoming z: r and z are clean data in poisoned vectors"""
    import amg_ref as R

    def _exported_levels(pc):
        info = pc.info()
        out = []
        for l in range(info["levels"]):
            L = {"dinv": pc.export(l, "Dinv")}
            for key in ("A", "P", "R"):
                nr, nc, rp, ci, va = pc.export(l, key)
                L[key] = None if (key != "A" and l == info["levels"] - 1) else O.Csr(nr, nc, rp, ci.astype(np.int64), va)
            out.append(L)
        return out
    a = O.stencil7(8, "convdiff")
    n = a.nrows
    d = to_dev(ctx, a)
    pc = K.Amg(10, 0.1).setup(d)
    levels = _exported_levels(pc)
    assert len(levels) >= 2
    r0, z0 = C.clean_r(n, 1), C.clean_r(n, 2)
    want = R.vcycle(levels, r0, z0)
    for p in (None, poison, None):
        z = pvec(ctx, z0, p)
        pc.apply(pvec(ctx, r0, p), z)
        assert same_bits(z.to_host(), want), p
