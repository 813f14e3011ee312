"""Compressed-basis GMRES on the device (kryst_cbgmres_solve_dev, kryst_amd/csrc/gmres_cb.hip) against its numpy
restatement (tests/cb_gmres_ref.py), bit for bit: x, iterations, final residual, converged and the whole residual history.

Sizes are the smallest that reach each edge of the kernels: one row; three rows (an odd tail, one lane with a single element); 511 / 512 / 513
rows (one tile and the tile edge); convdiff 8^3 = 512 rows (one full tile) and 12^3 = 1728 rows (a partial last tile).  Restart 1, 5, 9 and 30
puts the cycle length below, at and above the x update's group of eight; the iteration caps are no multiples of the restart and end in
mid-cycle.  Every solve runs with the cached (<true>) and, under KRYST_KEEP_BYTES=0, the streamed (<false>) link instances."""
import os

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import cb_gmres_ref as CB

pytestmark = pytest.mark.gpu

PCN = K.Preconditioning
MODES = {"cached": None, "streamed": "0"}                    # KRYST_KEEP_BYTES
# restart -> (tol, max_iters): 7 cycles of one; 4 cycles of five and three more; a cap that is no multiple of nine; one cycle of thirty and ten more
RESTARTS = {1: (1e-10, 7), 5: (1e-10, 23), 9: (1e-10, 40), 30: (1e-8, 40)}


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    return K.Context(0)


def tridiag(n):
    """1-D convection-diffusion with a varying diagonal: nonsymmetric, diagonally dominant, Jacobi is not a multiple of the identity"""
    rp, ci, va = [0], [], []
    for i in range(n):
        if i > 0:
            ci.append(i - 1); va.append(-1.5)
        ci.append(i); va.append(3.0 + 0.5 * (i % 3))
        if i + 1 < n:
            ci.append(i + 1); va.append(-0.5)
        rp.append(len(ci))
    return O.Csr(n, n, rp, ci, va)


SIZES = {"n1": lambda: tridiag(1), "n3": lambda: tridiag(3), "n511": lambda: tridiag(511), "n512": lambda: tridiag(512),
         "n513": lambda: tridiag(513), "convdiff8": lambda: O.stencil7(8, "convdiff"), "convdiff12": lambda: O.stencil7(12, "convdiff")}
_ops, _refs = {}, {}


def to_dev(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


def op(ctx, name, make=None, dev=None):
    """name -> (oracle Csr, device CsrMatrix, b = A (1 + i mod 7 / 8), oracle Jacobi, device Jacobi), built once"""
    if name not in _ops:
        a = (make or SIZES[name])()
        d = dev(ctx) if dev else to_dev(ctx, a)
        b = a.spmv(1.0 + (np.arange(a.nrows) % 7) / 8.0)
        _ops[name] = (a, d, b, O.Pc.jacobi(a), K.Jacobi().setup(d))
    return _ops[name]


def ref(key, a, b, x0, opc, side, restart, tol, mx, basis):
    if key not in _refs:
        _refs[key] = CB.cbgmres(a, b, x0, pc=opc, side=int(side), restart=restart, tol=tol, max_iters=mx, basis=basis)
    return _refs[key]


def dev_solve(d, dpc, b, x0, side, restart, tol, mx, basis):
    s = K.CbGmresSolver(restart, tol, mx).with_basis(basis).with_preconditioning(side)
    x = np.array(x0, dtype=np.float64)
    st = s.solve(d, dpc, b, x)
    return st, s, x


def same(r, st, s, x, label):
    h, rh = np.array(s.residual_history, dtype=float), np.array(r.history, dtype=float)
    assert (st.iterations, bool(st.converged)) == (r.iterations, bool(r.converged)), (label, st, r.iterations, r.converged)
    assert len(h) == len(rh) and np.array_equal(h, rh, equal_nan=True), (label, "history", len(h), len(rh), np.flatnonzero(h[:len(rh)] != rh[:len(h)])[:4])
    assert st.final_residual == r.final_residual, (label, st.final_residual, r.final_residual)
    assert np.array_equal(x, r.x), (label, "x", int(np.sum(x != r.x)))


def set_mode(monkeypatch, mode):
    if MODES[mode] is None:
        monkeypatch.delenv("KRYST_KEEP_BYTES", raising=False)
    else:
        monkeypatch.setenv("KRYST_KEEP_BYTES", MODES[mode])


@pytest.mark.parametrize("side", [PCN.NoPc, PCN.Right], ids=["nopc", "right-jacobi"])
@pytest.mark.parametrize("basis", ["f64", "f32"])
@pytest.mark.parametrize("size", list(SIZES))
def test_device_is_the_restatement(ctx, monkeypatch, size, basis, side):
    a, d, b, ojac, djac = op(ctx, size)
    x0 = np.zeros(a.nrows)
    for restart, (tol, mx) in RESTARTS.items():
        r = ref((size, basis, int(side), restart), a, b, x0, ojac if side else None, side, restart, tol, mx, basis)
        for mode in MODES:
            set_mode(monkeypatch, mode)
            st, s, x = dev_solve(d, djac if side else None, b, x0, side, restart, tol, mx, basis)
            same(r, st, s, x, (size, basis, int(side), restart, mode))
    if size == "convdiff12":                                  # the caps really end in mid-cycle, and the long cycle is a whole one
        assert _refs[(size, basis, int(side), 5)].iterations == 23 and _refs[(size, basis, int(side), 30)].iterations == 40


@pytest.mark.parametrize("basis", ["f64", "f32"])
def test_a_preconditioner_that_is_not_pointwise(ctx, monkeypatch, basis):
    """Right with true ILU(0) on aniso 10^3: the apply is a pair of triangular solves, M^-1 u at the cycle end included"""
    a = O.stencil7(10, "aniso")
    d = K.CsrMatrix.stencil7(10, "aniso", ctx=ctx)
    b = a.spmv(1.0 + (np.arange(a.nrows) % 7) / 8.0)
    opc, dpc = O.Pc.ilu0_true(a), K.TrueIlu0().setup(d)
    r = CB.cbgmres(a, b, np.zeros(a.nrows), pc=opc, side=CB.SIDE_RIGHT, restart=30, tol=1e-10, max_iters=100, basis=basis)
    assert r.converged and 2 <= r.iterations < 60
    for mode in MODES:
        set_mode(monkeypatch, mode)
        st, s, x = dev_solve(d, dpc, b, np.zeros(a.nrows), PCN.Right, 30, 1e-10, 100, basis)
        same(r, st, s, x, ("ilu0", basis, mode))


def test_past_one_fold_chunk(ctx):
    """convdiff 81^3 = 531 441 rows: 1038 tiles, two chunks of the fold's first stage"""
    a, d = O.stencil7(81, "convdiff"), K.CsrMatrix.stencil7(81, "convdiff", ctx=ctx)
    b = a.spmv(1.0 + (np.arange(a.nrows) % 7) / 8.0)
    r = CB.cbgmres(a, b, np.zeros(a.nrows), restart=5, tol=1e-12, max_iters=12, basis="f32")
    st, s, x = dev_solve(d, None, b, np.zeros(a.nrows), PCN.NoPc, 5, 1e-12, 12, "f32")
    assert r.iterations == 12
    same(r, st, s, x, "81^3")


@pytest.mark.parametrize("case", ["convdiff12-r30", "convdiff12-r5-cap", "n513-r9", "b0", "max_iters0"])
def test_f64_basis_without_pc_is_gmres_solver(ctx, case):
    size, restart, tol, mx = {"convdiff12-r30": ("convdiff12", 30, 1e-10, 200), "convdiff12-r5-cap": ("convdiff12", 5, 1e-10, 23),
                              "n513-r9": ("n513", 9, 1e-12, 60), "b0": ("convdiff8", 5, 1e-8, 12), "max_iters0": ("convdiff8", 5, 1e-8, 0)}[case]
    a, d, b, _, _ = op(ctx, size)
    if case == "b0":
        b = np.zeros(a.nrows)
    x0 = np.linspace(-1.0, 1.0, a.nrows) if case != "b0" else np.zeros(a.nrows)
    g = K.GmresSolver(restart, tol, mx).with_preconditioning(PCN.NoPc)
    xg = x0.copy()
    sg = g.solve(d, None, b, xg)
    st, s, x = dev_solve(d, None, b, x0, PCN.NoPc, restart, tol, mx, "f64")
    assert (st.iterations, st.converged) == (sg.iterations, sg.converged)
    assert st.final_residual == sg.final_residual or (np.isnan(st.final_residual) and np.isnan(sg.final_residual))
    assert np.array_equal(np.array(s.residual_history), np.array(g.residual_history), equal_nan=True)
    assert np.array_equal(x, xg, equal_nan=True)
    if case == "max_iters0":
        assert st.iterations == 0 and len(s.residual_history) == 0 and np.array_equal(x, x0)


@pytest.mark.parametrize("basis", ["f64", "f32"])
def test_happy_breakdown(ctx, basis):
    """2 I: the Krylov space has dimension one; the first step breaks down happily and (fp64) returns the exact answer"""
    n = 40
    a = O.Csr(n, n, np.arange(n + 1), np.arange(n), np.full(n, 2.0))
    d, b = to_dev(ctx, a), np.linspace(1.0, 3.0, n)
    r = CB.cbgmres(a, b, np.zeros(n), restart=5, tol=1e-10, max_iters=50, basis=basis)
    st, s, x = dev_solve(d, None, b, np.zeros(n), PCN.NoPc, 5, 1e-10, 50, basis)
    same(r, st, s, x, ("happy", basis))
    assert st.converged and np.allclose(x, b / 2.0, rtol=1e-9, atol=0.0)
    if basis == "f64":
        assert st.iterations == 1


def test_in_out_behaviour(ctx, monkeypatch):
    a, d, b, ojac, djac = op(ctx, "convdiff12")
    x0 = np.cos(np.arange(a.nrows))
    r = CB.cbgmres(a, b, x0, pc=ojac, side=CB.SIDE_RIGHT, restart=9, tol=1e-9, max_iters=200, basis="f32")
    r0 = CB.cbgmres(a, b, np.zeros(a.nrows), pc=ojac, side=CB.SIDE_RIGHT, restart=9, tol=1e-9, max_iters=200, basis="f32")
    assert r.converged and not np.array_equal(r.x, r0.x)      # the initial guess matters to the bits
    st, s, x = dev_solve(d, djac, b, x0, PCN.Right, 9, 1e-9, 200, "f32")
    same(r, st, s, x, "x0 host")
    # device vectors with poisoned padding; nothing goes through the host during the solve
    for poison in (None, float("nan"), 1e300):
        bv, xv = K.DeviceVec(ctx, b), K.DeviceVec(ctx, x0)
        if poison is not None:
            bv.poison_padding(poison); xv.poison_padding(poison)
            assert bv.padding_dirty() > 0 and xv.padding_dirty() > 0
        s = K.CbGmresSolver(9, 1e-9, 200).with_basis("f32").with_preconditioning(PCN.Right)
        with monkeypatch.context() as mp:
            def forbidden(*_a, **_k):
                raise AssertionError("a device-resident solve copied a vector to or from the host")
            mp.setattr(K.DeviceVec, "to_host", forbidden)
            mp.setattr(K.DeviceVec, "upload", forbidden)
            st = s.solve(d, djac, bv, xv)
        same(r, st, s, xv.to_host(), ("x0 device", poison))
        assert np.array_equal(bv.to_host(), b)


@pytest.mark.parametrize("what", ["left", "left-textbook", "basis2", "basis-1", "restart0", "restart4097"])
def test_errors_leave_x_untouched(ctx, what):
    a, d, b, _, djac = op(ctx, "convdiff8")
    side, basis, restart, code = {"left": (PCN.Left, "f32", 5, 6), "left-textbook": (PCN.LeftTextbook, "f32", 5, 6),
                                  "basis2": (PCN.Right, 2, 5, 102), "basis-1": (PCN.Right, -1, 5, 102),
                                  "restart0": (PCN.Right, "f32", 0, 102), "restart4097": (PCN.Right, "f32", 4097, 102)}[what]
    x0 = np.sin(np.arange(a.nrows))
    bv, xv = K.DeviceVec(ctx, b), K.DeviceVec(ctx, x0)
    s = K.CbGmresSolver(restart, 1e-8, 20).with_basis(basis).with_preconditioning(side)
    with pytest.raises(K.KError) as e:
        s.solve(d, djac, bv, xv)
    assert e.value.code == code
    assert np.array_equal(xv.to_host(), x0)
    # the context is free again: the next solve runs
    st, _, _ = dev_solve(d, djac, b, x0, PCN.Right, 5, 1e-8, 20, "f32")
    assert st.iterations >= 1
