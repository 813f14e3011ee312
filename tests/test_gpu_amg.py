"""AMG as written on the device (kryst_pc_amg; kryst_amd/csrc/amg.hip) against the numpy restatement (tests/amg_ref.py): the uploaded
hierarchy is the host set-up's exactly, the V-cycle on the exported hierarchy gives the restatement's bits (incoming z included), and PCG
preconditioned by it follows the restatement's iterations."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import amg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    T, V, F = K.reduce_spec()
    return O.Reduce.tiled(T, V, F)


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def exported_levels(pc):
    info = pc.info()
    out = []
    for l in range(info["levels"]):
        L = {"dinv": pc.export(l, "Dinv")}
        for key in ("A", "P", "R"):
            nr, nc, rp, ci, va = pc.export(l, key)
            L[key] = None if (key != "A" and l == info["levels"] - 1) else O.Csr(nr, nc, rp, ci.astype(np.int64), va)
        out.append(L)
    return out


def same_bits(x, y):
    x = np.asarray(x); y = np.asarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("kind,N,max_levels,thr", [("poisson", 8, 10, 0.1), ("aniso", 6, 10, 0.1), ("varcoef", 8, 2, 0.05),
                                                   ("poisson", 4, 0, 0.1)])
def test_hierarchy_is_the_host_setup(ctx, kind, N, max_levels, thr):
    a = O.stencil7(N, kind)
    pc = K.Amg(max_levels, thr).setup(to_dev(ctx, a))
    host = K.host_amg(a.row_ptr, a.col_idx.astype(np.int32), a.vals, max_levels, thr)
    info = pc.info()
    assert info["levels"] == len(host)
    assert info["rows"] == [h["A"][0] for h in host]
    for l, h in enumerate(host):
        assert same_bits(pc.export(l, "Dinv"), h["dinv"])
        for key in ("A", "P", "R"):
            if h[key] is None:
                assert pc.export(l, key)[0] == 0
                continue
            g = pc.export(l, key)
            assert g[:2] == h[key][:2]
            assert np.array_equal(g[2], h[key][2]) and np.array_equal(g[3], h[key][3]) and same_bits(g[4], h[key][4])


@pytest.mark.parametrize("kind,N,max_levels", [("poisson", 8, 10), ("convdiff", 8, 10), ("varcoef", 10, 3), ("poisson", 4, 0)])
def test_vcycle_bit_for_bit_with_incoming_z(ctx, kind, N, max_levels):
    a = O.stencil7(N, kind)
    d = to_dev(ctx, a)
    pc = K.Amg(max_levels, 0.1).setup(d)
    levels = exported_levels(pc)
    rng = np.random.default_rng(N)
    r = rng.standard_normal(a.nrows)
    rv = K.DeviceVec(ctx, r)
    outs = []
    for z0 in (np.zeros(a.nrows), rng.standard_normal(a.nrows)):
        zv = K.DeviceVec(ctx, z0)
        pc.apply(rv, zv)
        got = zv.to_host()
        want = R.vcycle(levels, r, z0)
        assert same_bits(got, want)
        outs.append(got)
    if len(levels) > 1:                   # the finest level starts from the incoming z: the two applies differ
        assert not np.array_equal(outs[0], outs[1])
    else:                                 # one level: solve_direct ignores z
        assert same_bits(outs[0], outs[1])


@pytest.mark.parametrize("m,r", [
    ([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]], [5.0, 5.0, 3.0]),                                   # amg.rs:827-849
    ([[4.0, 1.0, 0.0, 0.0], [1.0, 3.0, 1.0, 0.0], [0.0, 1.0, 2.0, 1.0], [0.0, 0.0, 1.0, 4.0]], [5.0, 5.0, 3.0, 1.0]),   # :852-875
])
def test_reference_unit_tests_on_the_device(ctx, m, r):
    m = np.array(m); r = np.array(r)
    a = O.Csr.from_dense(m, keep_zeros=False)
    pc = K.PC.AMG(2, 0.1).build(to_dev(ctx, a))
    z = pc.apply(r)
    assert np.linalg.norm(r - m @ z) < 1.0
    assert same_bits(z, R.vcycle(exported_levels(pc), r, np.zeros(len(r))))


def shifted(N, shift):
    """Poisson N^3 + shift I: diagonally dominant enough for the as-written PCG to run several iterations"""
    a = O.stencil7(N)
    v = a.vals.copy()
    rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
    v[a.col_idx == rows] += shift
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


@pytest.mark.parametrize("N,shift,max_levels", [(8, 0.0, 10), (16, 0.0, 10), (6, 2.0, 10), (6, 20.0, 10), (6, 2.0, 1)])
def test_pcg_follows_the_restatement(ctx, rs, N, shift, max_levels):
    a = shifted(N, shift)
    d = to_dev(ctx, a)
    pc = K.Amg(max_levels, 0.1).setup(d)
    levels = exported_levels(pc)
    b = np.ones(a.nrows)
    xr, it, code, hist = R.pcg(a, levels, b, 1e-8, 200, rs)
    s = K.PcgSolver(1e-8, 200)
    x = np.zeros(a.nrows)
    if code:
        with pytest.raises(K.KError) as e:
            s.solve(d, pc, b, x)
        assert e.value.code == code
        assert e.value.stats is not None and e.value.stats.iterations == it
    else:
        st = s.solve(d, pc, b, x)
        assert st.iterations == it
        assert np.allclose(x, xr, rtol=1e-9, atol=1e-12)
    h = np.asarray(s.residual_history)
    assert len(h) == len(hist)
    fin = np.isfinite(hist)
    assert np.array_equal(np.isfinite(h), fin)
    assert np.allclose(h[fin], np.asarray(hist)[fin], rtol=1e-9, atol=0)


def test_six_iterations_or_more_are_compared(rs):
    """the parameters above include a case where the as-written PCG runs many iterations before its exit"""
    a = shifted(6, 2.0)
    h = K.host_amg(a.row_ptr, a.col_idx.astype(np.int32), a.vals, 10, 0.1)
    mk = lambda t: None if t is None else O.Csr(t[0], t[1], t[2], t[3].astype(np.int64), t[4])
    lv = [dict(A=mk(L["A"]), P=mk(L["P"]), R=mk(L["R"]), dinv=L["dinv"]) for L in h]
    assert R.pcg(a, lv, np.ones(a.nrows), 1e-8, 200, rs)[1] >= 6


@pytest.mark.parametrize("solver", ["gmres_left", "fgmres"])
def test_gmres_and_fgmres_hand_the_apply_the_reference_z(ctx, solver):
    """gmres.rs hands every apply a fresh zero z and fgmres.rs z_basis[j] = v_j (fgmres.rs:208-210).  With the as-written AMG the apply
    is then one fixed linear map M (GMRES: r -> vcycle(r, 0); FGMRES: v -> vcycle(v, v)); the same solve with M given explicitly as
    inverse rows (ApproxInv) must agree.  Leftover work-buffer contents as z would make the two drift apart.  (The right-preconditioned
    form starts from M r0, where the explicit M of this badly scaled operator cancels to only ~1e-3; it shares the same zeroing.)"""
    a = shifted(6, 20.0)
    d = to_dev(ctx, a)
    pc = K.Amg(10, 0.1).setup(d)
    levels = exported_levels(pc)
    n = a.nrows
    eye = np.eye(n)
    cols = [R.vcycle(levels, eye[j], eye[j] if solver == "fgmres" else np.zeros(n)) for j in range(n)]
    M = np.array(cols).T
    m_pc = K.ApproxInv([[(j, M[i, j]) for j in range(n) if M[i, j] != 0.0] for i in range(n)], ctx=ctx)
    b = np.ones(n)
    mk = {"gmres_left": lambda: K.GmresSolver(8, 0.0, 16).with_preconditioning(K.Preconditioning.Left),
          "gmres_right": lambda: K.GmresSolver(8, 0.0, 16).with_preconditioning(K.Preconditioning.Right),
          "fgmres": lambda: K.FgmresSolver(0.0, 16, 8)}[solver]
    s1, s2 = mk(), mk()
    x1 = np.zeros(n); s1.solve(d, pc, b, x1)
    x2 = np.zeros(n); s2.solve(d, m_pc, b, x2)
    h1, h2 = np.asarray(s1.residual_history), np.asarray(s2.residual_history)
    assert np.all(np.isfinite(x1)) and len(h1) == len(h2) >= 1
    # the as-written M is badly scaled (||M r|| ~ 1e8 ||r|| here), so the two forms of M agree only to ~1e-3 after amplification;
    # a stale z changes the first applies outright
    assert np.allclose(h1, h2, rtol=2e-2, atol=1e-12 * h2[0])
    assert np.allclose(x1, x2, rtol=2e-2, atol=1e-9 + 2e-2 * np.abs(x2).max())


def test_errors(ctx):
    a = O.stencil7(4)
    d = to_dev(ctx, a)
    for args, code in (((-1, 0.1), 102),):
        with pytest.raises(K.KError) as e:
            K.Amg(*args).setup(d)
        assert e.value.code == code
    rect = K.CsrMatrix.from_csr(2, 3, np.array([0, 1, 2]), np.array([0, 1]), np.array([1.0, 1.0]), ctx=ctx)
    with pytest.raises(K.KError) as e:
        K.Amg().setup(rect)
    assert e.value.code == 102
    amg = K.Amg(); amg.variant = 7                  # no such variant
    with pytest.raises(K.KError) as e:
        amg.setup(d)
    assert e.value.code == 102
    with pytest.raises(K.KError) as e:              # the coarsest level's CG runs in one workgroup: at most 4096 rows
        K.Amg(0, 0.1).setup(to_dev(ctx, O.stencil7(17)))
    assert e.value.code == 6


def test_pcg_session_queues_the_vcycle(ctx):
    """A stepping session queues the V-cycle with its iterations (no host round trip) and ends the way the one-shot solve does."""
    a = O.stencil7(8)
    d = to_dev(ctx, a)
    pc = K.PC.AMG().build(d)
    b = np.ones(a.nrows)
    with pytest.raises(K.KError) as e1:             # as written, PCG stops with IndefinitePreconditioner (pcg.rs beta < 0)
        K.PcgSolver(1e-8, 200).solve(d, pc, b, np.zeros(a.nrows))
    bv = K.DeviceVec(ctx, b); xv = K.DeviceVec(ctx, np.zeros(a.nrows))
    ses = K.Session("pcg", d, pc, bv, xv, 1e-8, 200)
    with pytest.raises(K.KError) as e2:
        ses.step(10)
        ses.end()
    ses.close()
    assert e1.value.code == e2.value.code == 4
