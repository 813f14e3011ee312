"""Non-finite and signed-zero input on the device: every preconditioner apply and the BLAS-1 pointwise kernels on right-hand sides that hold
+-inf, NaN, -0.0, the denormals and the largest double (tests/nonfinite_cases.py), against the references pinned by test_nonfinite_cpu.py.

Every apply case checks, on one device object:
  * the apply of the poisoned `r` equals the reference by `same_ieee` (NaNs at the same rows, every other row bit for bit);
  * the rows of the un-poisoned half are bit for bit those of the clean apply (the operators are two uncoupled halves: this needs no reference);
  * a following apply of the CLEAN `r` on the same object equals a fresh object's bit for bit: no ready flag, LDS ring, edge buffer or
    captured graph keeps anything of the poisoned run;
  * no apply reports an error (a NaN taken for "not written yet" ends in the give-up path, which `kryst_pc_apply` reports) and the form
    `ilu_info` names is the one the settings select, before and after (a fall-back changes it);
  * z holds NaN on entry for every kind that must not read it; AMG as written reads z (`reads_z`) and has tests of its own below, with
    finite and with poisoned data in z.
`health()` and `fell_back()` are not part of the C ABI.  What they decide is: `kryst_pc_apply` synchronises and asks `health()` for the kinds
whose kernels can give up -- a SOR sweep that abandoned its grid barrier raises the sticky give-up word, which surfaces there as SolveError
(and NaNs in z); an ILU wavefront solve that gave up switches to the plane kernels (`fell_back()`), which `ilu_info` then names.  So "no
apply raises" and "the form is the same before and after" are those two checks.
The kernels under test spin on NaN-patterned ready flags; each has a poll budget that ends in an error, never a hang."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import nonfinite_cases as C
from nonfinite_cases import same_ieee, poisoned, clean_r

pytestmark = pytest.mark.gpu

CASES = C.apply_cases() + C.spai_cases()


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    T, V, F = K.reduce_spec()
    return O.Reduce.tiled(T, V, F)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def apply_into_nans(ctx, pc, r):
    z = ctx.vec(len(r)).fill(float("nan"))
    pc.apply(ctx.vec(r), z)
    return z.to_host()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_apply_on_poisoned_r(ctx, case, monkeypatch):
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
    r0 = clean_r(n)
    z0 = apply_into_nans(ctx, fresh, r0)
    assert np.array_equal(bits(z0), bits(ref(r0))), case.id
    for label, rows, clean in case.poisonings(a):
        rp = poisoned(r0, rows)
        z = apply_into_nans(ctx, used, rp)
        want = ref(rp)
        assert same_ieee(z, want), (case.id, label, int(np.sum(np.isnan(z) != np.isnan(want))))
        assert np.array_equal(bits(z[clean]), bits(z0[clean])), (case.id, label, "the un-poisoned half changed")
        again = apply_into_nans(ctx, used, r0)
        assert np.array_equal(bits(again), bits(z0)), (case.id, label, "the poisoned apply left something behind")
        if form is not None:
            assert used.ilu_info()["form"] == form, (case.id, label, "the solve gave up and fell back")


# ------------------------------------------------------------------------------------------------ BLAS-1
ALPHAS = (np.inf, np.nan, -0.0)


@pytest.mark.parametrize("n", [1, 511, 512, 513])
def test_pointwise_kernels_and_dot_on_special_values(ctx, rs, n):
    """axpy (cg.rs:208 `*xj + alpha * pj`), aypx (cg.rs:275 `rj + beta * *pj`), sub and dot / norm with poison in the first and the last
    element and a coefficient of inf, NaN and -0.0, at one element, one short of a tile, a tile, and one more."""
    rng = np.random.default_rng(n)
    x0, y0 = rng.standard_normal(n), rng.standard_normal(n)
    for first, last in ((np.inf, np.nan), (-0.0, -np.inf), (5e-324, 1.7976931348623157e308), (np.nan, -5e-324)):
        x = x0.copy(); x[0] = first; x[-1] = last
        y = y0.copy(); y[-1] = -0.0
        with np.errstate(all="ignore"):
            for al in ALPHAS + (0.37,):
                dx, dy = ctx.vec(x), ctx.vec(y)
                K.axpy(al, dx, dy)
                assert same_ieee(dy.to_host(), y + al * x), ("axpy", n, al, first)
                dy.upload(y)
                K.aypx(al, dx, dy)
                assert same_ieee(dy.to_host(), x + al * y), ("aypx", n, al, first)
            dx, dy, out = ctx.vec(x), ctx.vec(y), ctx.vec(n).fill(float("nan"))
            assert same_ieee(K.sub(dx, dy, out).to_host(), x - y), ("sub", n, first)
            assert same_ieee(K.sub(dx, dy, dx).to_host(), x - y), ("sub in place", n, first)
            dx = ctx.vec(x)
            assert same_ieee([K.dot(dx, dy)], [O.dot(x, y, rs)]), ("dot", n, first)
            assert same_ieee([K.norm(dx)], [O.norm(x, rs)]), ("norm", n, first)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 729])
def test_a_nan_coefficient_leaves_nothing_in_a_vector_that_is_uploaded_again(ctx, rs, n):
    """A non-finite coefficient turns every element the kernel touches into NaN -- padding past n included, if the kernel writes there.  After
    fresh data are uploaded into the same vectors, dot, norm and (n = 729: stencil7(9)) a CG solve that uses them must give the bits of
    new vectors: nothing may rely on the padding being zero."""
    rng = np.random.default_rng(100 + n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    dx, dy = ctx.vec(x), ctx.vec(y)
    for al in (np.nan, np.inf):
        K.axpy(al, dx, dy); K.aypx(al, dy, dx)
    assert np.isnan(dx.to_host()).all() and np.isnan(dy.to_host()).all()
    dx.upload(x); dy.upload(y)
    nx, ny = ctx.vec(x), ctx.vec(y)
    assert bits([K.dot(dx, dy)])[0] == bits([K.dot(nx, ny)])[0] == bits([O.dot(x, y, rs)])[0]
    assert bits([K.norm(dx)])[0] == bits([K.norm(nx)])[0] == bits([O.norm(x, rs)])[0]
    if n == 729:
        ao = O.stencil7(9)
        a = to_dev(ctx, ao)
        b = ao.spmv(np.ones(n))
        res = O.solve("cg", ao, b, tol=1e-9, max_iters=200, rs=rs)
        dx.upload(b); dy.upload(np.zeros(n))
        s = K.CgSolver(1e-9, 200)
        st = s.solve(a, None, dx, dy)
        assert st.iterations == res.iterations and np.array_equal(np.array(s.residual_history), res.history)
        assert np.array_equal(bits(dy.to_host()), bits(res.x))


# ------------------------------------------------------------------------------------------------ AMG as written: the apply reads z
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


def test_amg_as_written_with_r_and_the_incoming_z_poisoned(ctx):
    """apply_recursive (amg.rs:200-250) starts the finest level from the incoming z, so z is data: finite (the clean apply), with -0.0 and
    denormals (bit for bit against amg_ref.vcycle on the exported hierarchy), and with +-inf / NaN in r, in z, and in both.  The coarsest
    level's CG folds every row into its inner products: the expected output of the non-finite applies is NaN in EVERY row
    (test_nonfinite_cpu.py pins that), so this case checks NaN placement, that no apply reports an error, and that a clean apply afterwards
    equals a fresh object's -- the 30 % condition is carried by the smoothed-aggregation case above."""
    import amg_ref as R
    a = O.stencil7(8, "convdiff")
    n = a.nrows
    d = to_dev(ctx, a)
    fresh, used = K.Amg(10, 0.1).setup(d), K.Amg(10, 0.1).setup(d)
    levels = _exported_levels(used)
    assert len(levels) >= 2
    r0, z0 = clean_r(n, 1), clean_r(n, 2)
    rows = C.row_set(0, n)

    def dev(pc, r, z):
        zv = ctx.vec(z)
        pc.apply(ctx.vec(r), zv)
        return zv.to_host()
    clean = dev(fresh, r0, z0)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(clean), bits(R.vcycle(levels, r0, z0)))
        tame = (-0.0, 5e-324, -5e-324)
        for r, z in ((poisoned(r0, rows, tame), z0), (r0, poisoned(z0, rows, tame)), (poisoned(r0, rows, tame), poisoned(z0, rows[::-1], tame)),
                     (poisoned(r0, rows), z0), (r0, poisoned(z0, rows)), (poisoned(r0, rows), poisoned(z0, rows))):
            got, want = dev(used, r, z), R.vcycle(levels, r, z)
            assert same_ieee(got, want), int(np.sum(np.isnan(got) != np.isnan(want)))
            assert np.array_equal(bits(dev(used, r0, z0)), bits(clean)), "the poisoned apply left something behind"


# ------------------------------------------------------------------------------------------------ whole solves that go non-finite
SOLVES = {
    "bicgstab": (lambda: K.BiCgStabSolver(1e-8, 12), {}, False),
    "cgs": (lambda: K.CgsSolver(1e-8, 12), {}, False),
    "tfqmr": (lambda: K.TfqmrSolver(1e-8, 12), {}, False),
    "gmres": (lambda: K.GmresSolver(5, 1e-8, 12).with_preconditioning(K.Preconditioning.Right), dict(restart=5, side=O.SIDE_RIGHT), True),
    "fgmres": (lambda: K.FgmresSolver(1e-8, 12, 5), dict(restart=5), True),
}


@pytest.mark.parametrize("scale_a,scale_b", [(1e100, 1e100), (1e60, 1e130), (1.0, 1e153)])
@pytest.mark.parametrize("method", list(SOLVES))
def test_whole_solves_that_overflow_break_down_where_the_oracle_does(ctx, rs, method, scale_a, scale_b):
    """BiCGStab, CGS and TFQMR as written, right-preconditioned GMRES(5) and FGMRES (Jacobi) on the 729-row convection-diffusion system
    with the operator scaled by scale_a and the right-hand side by scale_b: squares and products of 1e200 and beyond overflow in the first
    iterations (with 1e100 / 1e100 some inner products stay finite and the iteration goes on with inf and 0 coefficients; with the other
    two the first norm or inner product is already inf).  The solvers are mirrored as written, silent breakdowns included: iteration
    count, converged flag and error code equal the oracle's, history and x agree by same_ieee."""
    a0 = O.stencil7(9, "convdiff")
    a = O.Csr(a0.nrows, a0.ncols, a0.row_ptr, a0.col_idx, a0.vals * scale_a)
    b = a0.spmv(np.linspace(0.5, 1.5, a0.nrows)) * scale_b
    make, kw, with_pc = SOLVES[method]
    res = O.solve(method, a, b, tol=1e-8, max_iters=12, rs=rs, raise_on_error=False, pc=O.Pc.jacobi(a) if with_pc else None, **kw)
    d = to_dev(ctx, a)
    s = make()
    x = np.zeros(a.nrows)
    pc = K.Jacobi().setup(d) if with_pc else None
    code, st = 0, None
    try:
        st = s.solve_flex(d, pc, b, x) if method == "fgmres" else s.solve(d, pc, b, x)
    except K.KError as e:
        code, st = e.code, e.stats
    print(method, scale_a, scale_b, "oracle:", res, "device:", code, st)
    assert code == res.code
    assert st is not None and st.iterations == res.iterations and st.converged == res.converged
    assert same_ieee([st.final_residual], [res.final_residual])
    assert same_ieee(np.array(s.residual_history), res.history)
    assert same_ieee(x, res.x)
