"""Compressed-basis GMRES, CPU tier: the numpy restatement alone (tests/cb_gmres_ref.py).

1. with nothing rounded and no preconditioner it IS the oracle's GMRES side None, bit for bit;
2. the fp32 basis does not cap the attainable accuracy (tol = 1e-12 is reached, judged by an independent residual);
3. ... and is not paid back in iterations (at most those of the fp64 control + 1 + 5 %);
4. the rounding sits where the contract says: every stored basis vector is float32, and `store` = identity gives case 1 again."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
import cb_gmres_ref as CB
from mixed_ref import F32, F64, RS64

EPS64 = float(np.finfo(np.float64).eps) / 2.0                # unit roundoff


def _diag_system(n=40):
    """2 I: the Krylov space of any b has dimension 1 -- happy breakdown in the first step, the exact answer b / 2"""
    return O.Csr(n, n, np.arange(n + 1), np.arange(n), np.full(n, 2.0)), np.linspace(1.0, 3.0, n)


def _pin_cases():
    a = O.stencil7(8, "convdiff")
    b = a.spmv(np.ones(a.nrows))
    d, db = _diag_system()
    return {"convdiff8-r5": (a, b, 5, 1e-10, 200), "convdiff8-r30": (a, b, 30, 1e-10, 200), "convdiff8-r5-cap23": (a, b, 5, 1e-10, 23),
            "diag-happy": (d, db, 5, 1e-10, 50)}


PIN = _pin_cases()


@pytest.mark.parametrize("name", sorted(PIN))
def test_f64_basis_without_pc_is_the_oracle_gmres(name):
    a, b, restart, tol, mx = PIN[name]
    ref = O.solve("gmres", a, b, tol=tol, max_iters=mx, restart=restart, side=0, rs=RS64)
    out = CB.cbgmres(a, b, np.zeros(a.nrows), restart=restart, tol=tol, max_iters=mx, basis="f64")
    assert (out.iterations, out.converged, out.final_residual) == (ref.iterations, ref.converged, ref.final_residual)
    assert np.array_equal(np.array(out.history), ref.history)
    assert np.array_equal(out.x, ref.x)
    if name == "diag-happy":
        # x = (beta / h00) (b / beta), h00 = 2 (v0, v0): a division, an n-term inner product and two more operations
        assert out.iterations == 1 and out.converged and np.allclose(out.x, b / 2.0, rtol=(a.nrows + 4) * EPS64, atol=0.0)


# ---- accuracy and iterations: restart 30, tol 1e-12, b = A ones, x0 = 0
ACC = [("convdiff", 12), ("convdiff", 16), ("aniso", 12)]
TOL = 1e-12
_runs = {}


def _run(kind, N, jac, basis):
    key = (kind, N, jac, basis)
    if key not in _runs:
        a = O.stencil7(N, kind)
        b = a.spmv(np.ones(a.nrows))
        pc = O.Pc.jacobi(a) if jac else None
        _runs[key] = (a, b, CB.cbgmres(a, b, np.zeros(a.nrows), pc=pc, side=CB.SIDE_RIGHT, restart=30, tol=TOL, max_iters=3000, basis=basis))
    return _runs[key]


@pytest.mark.parametrize("jac", [False, True], ids=["nopc", "jacobi-right"])
@pytest.mark.parametrize("kind,N", ACC)
def test_fp32_basis_does_not_cap_the_accuracy(kind, N, jac):
    """The solve ends on its own fp64 residual: ||fl(b - A x)|| < tol ||b||.  An independent evaluation (scipy's CSR product, numpy's norm)
    differs from it by the rounding of the two evaluations: per component each is within (k + 2) u (|b| + |A| |x|)_i of the exact residual
    (k = 7 terms per row, one subtraction, u = 2^-53), and each norm within n u relatively.  Hence
        ||b - A x|| / ||b||  <=  tol * factor,   factor = 1 + 2 (k + 2) u || |b| + |A| |x| || / (tol ||b||) + 2 n u,
    about 1.03 for these operators (|A| |x| is some ten times |b|)."""
    a, b, out = _run(kind, N, jac, "f32")
    assert out.converged
    m = sp.csr_matrix((a.vals, a.col_idx, a.row_ptr), shape=(a.nrows, a.ncols))
    rel = np.linalg.norm(b - m @ out.x) / np.linalg.norm(b)
    k, n = 7, a.nrows
    factor = 1.0 + 2.0 * (k + 2) * EPS64 * np.linalg.norm(np.abs(b) + abs(m) @ np.abs(out.x)) / (TOL * np.linalg.norm(b)) + 2.0 * n * EPS64
    print(f"{kind} {N} jacobi={jac}: independent relative residual {rel:.3e}, factor {factor:.4f}, iterations {out.iterations}")
    assert factor < 1.1
    assert rel <= TOL * factor


@pytest.mark.parametrize("jac", [False, True], ids=["nopc", "jacobi-right"])
@pytest.mark.parametrize("kind,N", ACC)
def test_fp32_basis_is_not_paid_back_in_iterations(kind, N, jac):
    _, _, f32 = _run(kind, N, jac, "f32")
    _, _, f64 = _run(kind, N, jac, "f64")
    print(f"{kind} {N} jacobi={jac}: iterations f32 {f32.iterations} / f64 {f64.iterations}")
    assert f64.converged and f32.converged
    assert f32.iterations <= f64.iterations + 1 + 0.05 * f64.iterations


# ---- where the rounding sits
def test_every_stored_basis_vector_is_float32_and_widens_exactly():
    a, b, out = _run("convdiff", 12, True, "f32")
    assert len(out.basis) >= 2
    for v in out.basis:
        assert v.dtype == F32
        assert np.array_equal(v.astype(F64).astype(F32), v)
    _, _, ctl = _run("convdiff", 12, True, "f64")
    assert all(v.dtype == F64 for v in ctl.basis)
    assert not np.array_equal(out.x, ctl.x)                  # the rounding is there


@pytest.mark.parametrize("name", sorted(PIN))
def test_identity_store_reproduces_the_oracle(name):
    a, b, restart, tol, mx = PIN[name]
    ref = O.solve("gmres", a, b, tol=tol, max_iters=mx, restart=restart, side=0, rs=RS64)
    out = CB.cbgmres(a, b, np.zeros(a.nrows), restart=restart, tol=tol, max_iters=mx, basis="f32", store=lambda v: np.array(v, dtype=F64))
    assert (out.iterations, out.converged, out.final_residual) == (ref.iterations, ref.converged, ref.final_residual)
    assert np.array_equal(np.array(out.history), ref.history) and np.array_equal(out.x, ref.x)
