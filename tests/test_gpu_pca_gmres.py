"""PcaGmresSolver on the device (kryst_amd/csrc/pca_gmres.hip), as written and as the labelled s-step extension, bit for bit against
tests/pca_gmres_ref.py in the library's reduction order: x, iterations, converged, final_residual and history."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import pca_gmres_ref as R

pytestmark = pytest.mark.gpu

PCN = K.Preconditioning


@pytest.fixture(scope="module")
def ctx():
    c = K.Context(0)
    c.poison_lds()
    return c


@pytest.fixture(scope="module")
def rs():
    T, V, F = K.reduce_spec()
    return O.Reduce.tiled(T, V, F)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def check(ref, st, s, x, nan_ok=False):
    assert (st.iterations, st.converged) == (ref.iterations, ref.converged), (st, ref)
    assert st.final_residual == ref.final_residual or (nan_ok and np.isnan(st.final_residual) and np.isnan(ref.final_residual))
    assert np.array_equal(np.array(s.residual_history), ref.history, equal_nan=nan_ok)
    assert np.array_equal(x, ref.x, equal_nan=nan_ok)


def nonsym(N):
    return O.stencil7(N, "convdiff")


PCS = {"none": (None, None), "jacobi": (K.Jacobi, O.Pc.jacobi), "ilu0": (K.TrueIlu0, O.Pc.ilu0_true)}


def _pcs(ctx, a, name):
    kc, oc = PCS[name]
    if kc is None:
        return None, None
    return kc().setup(to_dev(ctx, a)), oc(a)


# ----------------------------------------------------------------------------- as written
@pytest.mark.parametrize("restart", [1, 5, 30])
@pytest.mark.parametrize("pcname,side", [("none", PCN.Left), ("jacobi", PCN.Right), ("jacobi", PCN.Left), ("ilu0", PCN.Right),
                                         ("ilu0", PCN.NoPc)])
def test_as_written_bits(ctx, rs, restart, pcname, side):
    a = nonsym(10)
    g = np.random.default_rng(restart)
    b = g.standard_normal(a.nrows)
    x0 = g.standard_normal(a.nrows)                         # ignored (pca_gmres.rs:107)
    d = to_dev(ctx, a)
    kpc, opc = _pcs(ctx, a, pcname)
    for tol, mx in ((1e-6, 40), (0.0, 23)):                 # a stop mid-cycle / the iteration cap
        ref = R.as_written(a, b, pc=opc, side=int(side), restart=restart, tol=tol, max_iters=mx, rs=rs)
        s = K.PcaGmresSolver(restart, 2, 1, tol, mx).with_preconditioning(side)
        x = x0.copy()
        st = s.solve(d, kpc, b, x)
        check(ref, st, s, x, nan_ok=True)


def test_as_written_edges(ctx, rs):
    a = nonsym(8)
    d = to_dev(ctx, a)
    b = np.random.default_rng(3).standard_normal(a.nrows)
    # max_iters = 0: {0, ||b||, false}, x = 0
    s = K.PcaGmresSolver(5, 1, 1, 1e-8, 0)
    x = np.ones(a.nrows)
    st = s.solve(d, None, b, x)
    ref = R.as_written(a, b, restart=5, tol=1e-8, max_iters=0, rs=rs)
    check(ref, st, s, x)
    assert not np.any(x) and st.iterations == 0 and not st.converged
    # b = 0: NaNs, as written
    s = K.PcaGmresSolver(5, 1, 1, 1e-8, 7)
    x = np.ones(a.nrows)
    st = s.solve(d, None, np.zeros(a.nrows), x)
    ref = R.as_written(a, np.zeros(a.nrows), restart=5, tol=1e-8, max_iters=7, rs=rs)
    check(ref, st, s, x, nan_ok=True)
    assert np.isnan(st.final_residual) and np.all(np.isnan(x))
    # KRYST_ERR_ARG with x untouched
    for restart, bs, mx in ((5, 2, 10), (2, 3, 1), (5, 0, 10), (0, 1, 10)):
        s = K.PcaGmresSolver(restart, 1, bs, 1e-8, mx)
        x = np.full(a.nrows, 7.0)
        with pytest.raises(K.KError) as e:
            s.solve(d, None, b, x)
        assert e.value.code == 102 and np.all(x == 7.0)
    # restart 1 with any block size runs (t = min(s, 1) = 1)
    ref = R.as_written(a, b, restart=1, block_size=4, tol=1e-8, max_iters=6, rs=rs)
    s = K.PcaGmresSolver(1, 1, 4, 1e-8, 6)
    x = np.zeros(a.nrows)
    check(ref, s.solve(d, None, b, x), s, x, nan_ok=True)


def test_reference_small_system(ctx):
    """pca_gmres.rs:336-356: restart 6, block size 2 -- KRYST_ERR_ARG as written, solved through the s-step extension"""
    a = O.Csr.from_dense(np.array([[4.0, 1.0, 2.0], [1.0, 3.0, 1.0], [2.0, 1.0, 3.0]]))
    d = to_dev(ctx, a)
    b = a.spmv(np.array([1.0, 2.0, 3.0]))
    x = np.zeros(3)
    with pytest.raises(K.KError) as e:
        K.PcaGmresSolver(6, 2, 2, 1e-10, 30).solve(d, None, b, x)
    assert e.value.code == 102
    s = K.PcaGmresSolver(6, 2, 2, 1e-10, 30).with_textbook()
    st = s.solve(d, None, b, x)
    assert st.converged and np.max(np.abs(x - np.array([1.0, 2.0, 3.0]))) < 1e-8


# ----------------------------------------------------------------------------- s-step
@pytest.mark.parametrize("sb", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("pcname", ["none", "jacobi", "ilu0"])
def test_sstep_bits(ctx, rs, sb, pcname):
    a = nonsym(12)
    g = np.random.default_rng(10 + sb)
    b = g.standard_normal(a.nrows)
    x0 = g.standard_normal(a.nrows) * 0.1
    d = to_dev(ctx, a)
    kpc, opc = _pcs(ctx, a, pcname)
    for restart, tol, mx, xin in ((30, 1e-9, 200, x0), (7, 1e-7, 200, None), (10, 0.0, 17, x0)):   # s not dividing m, the cap
        ref = R.sstep(a, b, x=xin, pc=opc, side=2, restart=restart, block_size=sb, tol=tol, max_iters=mx, rs=rs)
        s = K.PcaGmresSolver(restart, 1, sb, tol, mx).with_preconditioning(PCN.Right).with_textbook()
        x = np.zeros(a.nrows) if xin is None else xin.copy()
        st = s.solve(d, kpc, b, x)
        check(ref, st, s, x)


def test_sstep_truncation_and_breakdown(ctx, rs):
    n = 40
    g = np.random.default_rng(5)
    P = np.eye(n) + 0.1 * g.standard_normal((n, n))
    A = P @ np.diag(np.resize([1.0, 2.0, 3.0], n)) @ np.linalg.inv(P)
    a = O.Csr.from_dense(A)
    b = g.standard_normal(n)
    ref = R.sstep(a, b, restart=10, block_size=5, tol=0.0, max_iters=10, rs=rs)
    kinds = {e[0] for e in ref.events}
    assert {"truncate", "happy"} <= kinds, ref.events
    s = K.PcaGmresSolver(10, 1, 5, 0.0, 10).with_preconditioning(PCN.NoPc).with_textbook()
    x = np.zeros(n)
    st = s.solve(to_dev(ctx, a), None, b, x)
    check(ref, st, s, x)


def test_sstep_left_with_pc_unsupported(ctx):
    a = nonsym(6)
    d = to_dev(ctx, a)
    pc = K.Jacobi().setup(d)
    x = np.zeros(a.nrows)
    with pytest.raises(K.KError) as e:
        K.PcaGmresSolver(10, 1, 4, 1e-8, 50).with_textbook().solve(d, pc, np.ones(a.nrows), x)
    assert e.value.code == 6 and not np.any(x)


def test_sstep_128(ctx, rs):
    a = O.stencil7(128, "poisson")
    d = K.CsrMatrix.stencil7(128, "poisson", ctx=ctx)
    b = a.spmv(np.ones(a.nrows))
    ref = R.sstep(a, b, pc=O.Pc.jacobi(a), side=2, restart=30, block_size=5, tol=0.0, max_iters=12, rs=rs)
    s = K.PcaGmresSolver(30, 1, 5, 0.0, 12).with_preconditioning(PCN.Right).with_textbook()
    x = np.zeros(a.nrows)
    st = s.solve(d, K.Jacobi().setup(d), b, x)
    check(ref, st, s, x)


def test_sstep_iteration_counts_convdiff64(ctx):
    d = K.CsrMatrix.stencil7(64, "convdiff", ctx=ctx)
    a = O.stencil7(64, "convdiff")
    b = a.spmv(np.ones(a.nrows))
    its = {}
    for sb in (1, 5):
        s = K.PcaGmresSolver(30, 1, sb, 1e-8, 3000).with_preconditioning(PCN.Right).with_textbook()
        x = np.zeros(a.nrows)
        st = s.solve(d, K.Jacobi().setup(d), b, x)
        assert st.converged
        assert np.linalg.norm(b - a.spmv(x)) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-9)
        its[sb] = st.iterations
    assert abs(its[5] - its[1]) <= 2, its
