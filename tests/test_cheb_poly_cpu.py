"""The host half of the Chebyshev polynomial preconditioner, without a GPU: kryst_host_tridiag_extreme_eigs against the restatement
(tests/cheb_poly_ref.py) bit for bit and against numpy.linalg.eigvalsh, and -- on the restatement alone -- what the preconditioner is for:
with the default bounds a degree-4 polynomial at least halves Jacobi-PCG's iteration count, and the upper bound covers the spectrum."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import amg_ref as AR
import cheb_poly_ref as CP


def _cases():
    g = np.random.default_rng(64)
    return {
        "k1": ([3.25], []),
        "k1-negative": ([-2.0], []),
        "k2": ([2.0, -1.0], [0.5]),
        "k10": (g.uniform(1.0, 3.0, 10), g.uniform(0.1, 1.0, 9)),
        "zero-beta-in-the-middle": ([2.0, 2.5, 1.0, 4.0, 3.0, 0.5], [1.0, 0.25, 0.0, 0.75, 0.5]),
        "equal-alphas": (np.full(8, 2.0), np.full(7, 1.0)),
        "k64-mixed-sign": (g.standard_normal(64) * 10.0, g.standard_normal(63) * 3.0),
        "lanczos-like": (np.linspace(0.2, 1.9, 12), np.geomspace(0.5, 1e-9, 11)),
    }


CASES = _cases()


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(CASES))
def test_extreme_eigs_equal_the_restatement_and_eigvalsh(name):
    al, be = CASES[name]
    got = K.host_tridiag_extreme_eigs(al, be)
    want = CP.tridiag_extreme_eigs(al, be)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    t = CP.tridiag_dense(al, be)
    ev = np.linalg.eigvalsh(t)
    tol = 64 * np.finfo(float).eps * np.abs(t).sum(axis=1).max()      # k eps |T|_inf: the backward error both methods carry at k <= 64
    assert abs(got[0] - ev[0]) <= tol and abs(got[1] - ev[-1]) <= tol, (got, ev[0], ev[-1], tol)
    assert got[0] <= got[1]


def test_extreme_eigs_special_input():
    lo, hi = K.host_tridiag_extreme_eigs([1.0, np.nan, 2.0], [0.5, 0.5])
    assert np.isnan(lo) and np.isnan(hi) and all(np.isnan(v) for v in CP.tridiag_extreme_eigs([1.0, np.nan, 2.0], [0.5, 0.5]))
    lo, hi = K.host_tridiag_extreme_eigs([1.0, 2.0], [np.inf])
    assert np.isnan(lo) and np.isnan(hi)
    big = K.host_tridiag_extreme_eigs([1e300, -1e300], [1e140])       # far from 1.0 in scale
    assert np.array_equal(bits(big), bits(CP.tridiag_extreme_eigs([1e300, -1e300], [1e140]))) and np.allclose(big, [-1e300, 1e300], rtol=1e-14, atol=0)
    zero = K.host_tridiag_extreme_eigs(np.zeros(4), np.zeros(3))      # |T| = 0: the bracket is a few multiples of the smallest normal number
    assert np.array_equal(bits(zero), bits(CP.tridiag_extreme_eigs(np.zeros(4), np.zeros(3)))) and max(abs(v) for v in zero) <= 1e-300
    assert K.host_tridiag_extreme_eigs([2.0, 3.0, 4.0], [9.0, 9.0, 9.0]) == K.host_tridiag_extreme_eigs([2.0, 3.0, 4.0], [9.0, 9.0])
    for al, be in (([], []), (np.zeros(65), np.zeros(64)), ([1.0, 2.0], [])):
        with pytest.raises(K.KError) as e:
            K.host_tridiag_extreme_eigs(al, be)
        assert e.value.code == 102


def test_scalars_follow_the_three_term_recurrence():
    """rho_k = T_{k-1}(sigma) / T_k(sigma): the closed form of the recurrence the contract states"""
    theta, c1, c2 = CP.scalars(6, 0.1, 3.0)
    sigma = theta / ((3.0 - 0.1) / 2.0)
    tk = [1.0, sigma]
    for _ in range(6):
        tk.append(2.0 * sigma * tk[-1] - tk[-2])
    rho = [tk[k] / tk[k + 1] for k in range(7)]
    assert np.allclose(c1, [rho[k + 1] * rho[k] for k in range(6)], rtol=1e-13)
    assert np.allclose(c2, [2.0 * rho[k + 1] / ((3.0 - 0.1) / 2.0) for k in range(6)], rtol=1e-13)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


@pytest.mark.parametrize("kind", ["poisson", "aniso"])
def test_degree_4_at_least_halves_jacobi_pcg(rs, kind):
    """Poisson and the anisotropic operator at 16^3, b = A 1, tol 1e-8, default bounds (a numpy prototype gave 13 against 42 and 20 against 79)"""
    a = O.stencil7(16, kind)
    b = a.spmv(np.ones(a.nrows))
    w = CP.jacobi_w(a)
    lo, hi = CP.default_bounds(CP.estimate(a, rs))
    _, it_j, code_j, hist_j = AR.pcg(a, None, b, 1e-8, 500, rs, apply=lambda r, z: w * r)
    _, it_c, code_c, hist_c = AR.pcg(a, None, b, 1e-8, 500, rs, apply=CP.make_apply(a, 4, lo, hi, w, two_args=True))
    print(kind, "Jacobi-PCG", it_j, "ChebyshevPoly(4)-PCG", it_c)
    assert code_j == 0 and code_c == 0 and hist_j[-1] / hist_j[0] <= 1e-8 and hist_c[-1] / hist_c[0] <= 1e-8
    assert 2 * it_c <= it_j, (it_c, it_j)


@pytest.mark.parametrize("kind", ["poisson", "aniso"])
def test_default_upper_bound_covers_the_spectrum(rs, kind):
    a = O.stencil7(8, kind)
    w = CP.jacobi_w(a)
    s = np.sqrt(w)
    lam_max = np.linalg.eigvalsh(s[:, None] * a.to_dense() * s[None, :])[-1]
    est = CP.estimate(a, rs)
    lo, hi = CP.default_bounds(est)
    print(kind, "lambda_max", lam_max, "theta_max", est["theta_max"], "gershgorin", est["gershgorin"], "hi", hi)
    assert hi >= lam_max and est["gershgorin"] >= lam_max and est["theta_max"] <= lam_max * (1.0 + 1e-12)
    assert lo == hi / 30.0 and est["steps_done"] == 10
