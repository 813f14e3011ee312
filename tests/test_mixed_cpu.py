"""Mixed precision without a GPU: the host twin of the lowering's rounding against numpy, and the numpy restatement of the contract
(tests/mixed_ref.py) on its own -- that it reaches an fp64 tolerance at a bounded price in inner iterations, and that each of its exits
is taken by the case the GPU tier then compares bit for bit (tests/test_gpu_mixed.py)."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import mixed_cases as MC
import mixed_ref as R


# ------------------------------------------------------------------------------------------------------------- the rounding twin
def rounding_input():
    exact = [1.0, -2.5, 0.0, 1024.0, 2.0 ** -126, 2.0 ** -149, 3.0 * 2.0 ** 100]          # exact in fp32 (two of them at its lower end)
    inexact = [1.0 / 3.0, -0.1, 1.0 + 2.0 ** -30, np.pi * 1e20]
    to_subnormal = [1e-40, -3e-42]                                                       # round to fp32 subnormals
    to_zero = [1e-50, -1e-60, 2.0 ** -151]                                               # round to +-0
    special = [-0.0, np.inf, -np.inf, np.nan]
    return np.array(exact + inexact + to_subnormal + to_zero + special)


def test_host_round_f32_is_astype_float32_with_its_counts():
    v = rounding_input()
    out, changed, tiny = K.host_round_f32(v)
    with np.errstate(all="ignore"):
        want = v.astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(MC.bits32(out)[:-1], MC.bits32(want)[:-1]) and np.isnan(out[-1])
    ref, ref_changed, ref_tiny, overflow = R.round_f32(v)
    assert overflow == 0 and (changed, tiny) == (ref_changed, ref_tiny)
    # by hand: the four inexact values, the two that become subnormal, the three that become zero; tiny: the exact subnormal 2^-149 too
    assert changed == 4 + 2 + 3 and tiny == 1 + 2 + 3
    assert np.signbit(out[-4]) and out[-4] == 0.0                                        # -0.0 keeps its sign


def test_host_round_f32_refuses_a_finite_value_that_overflows():
    for bad in (1e39, -1e39, 3.5e38):
        with pytest.raises(K.KError) as e:
            K.host_round_f32(np.array([1.0, bad, 2.0]))
        assert e.value.code == 6
        assert R.round_f32([1.0, bad, 2.0])[3] == 1
    K.host_round_f32(np.array([3.4028234e38, np.inf]))                                   # FLT_MAX and inf itself are fine
    with pytest.raises(O.KrylovError):
        R.Lowered(O.Csr.from_dense(np.array([[1e39]])))


def test_reduce_spec32_is_the_published_tree():
    assert K.reduce_spec32() == R.SPEC32 and K.reduce_spec32()[2] == K.reduce_spec()[2]


# ------------------------------------------------------------------------------------------------------------- the restatement converges
@pytest.fixture(scope="module")
def refined():
    out = {}
    for name, (make, jacobi) in MC.REFINE_CASES.items():
        a = make()
        a32 = R.Lowered(a)
        inv = O.Pc.jacobi(a).inv_diag if jacobi else None
        b = MC.rhs(a.nrows)
        got = R.refine(a, a32, inv, b, np.zeros(a.nrows), MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
        full = O.solve("pcg" if jacobi else "cg", a, b, pc=O.Pc.jacobi(a) if jacobi else None, tol=MC.OUTER_TOL, max_iters=MC.INNER_CAP)
        out[name] = (a, a32, b, got, full)
    return out


@pytest.mark.parametrize("name", list(MC.REFINE_CASES))
def test_the_restatement_reaches_the_fp64_tolerance(refined, name):
    a, a32, b, got, full = refined[name]
    assert got.code == 0 and got.converged and not got.rejected and got.iterations < MC.OUTER_CAP
    rho0 = O.norm(b)
    true = O.norm(b - a.spmv(got.x))
    print(name, "outer", got.iterations, "inner", got.inner_iterations, "fp64 iterations", full.iterations, "true residual / rho0", true / rho0)
    assert true <= MC.OUTER_TOL * rho0
    assert len(got.inner_iterations) == got.iterations and len(got.history) == got.iterations + 1
    # a cap that keeps a broken loop from passing, not a measurement
    assert full.converged and sum(got.inner_iterations) <= 2 * full.iterations
    if name.startswith("varcoef"):
        assert a32.info["changed"] > 0                                                   # values that are inexact in fp32
    if name.startswith("poisson"):
        assert a32.info["changed"] == 0                                                  # -1 and 6 are exact


# ------------------------------------------------------------------------------------------------------------- the exits
def test_exit_rejected_step():
    """Hilbert matrix of order 8, b = ones: the refinement stalls at the conditioning of the fp32 operator and a step fails to reduce the
    fp64 residual.  The order is searched from 8 to 10 in case the tiled fold moves the step (the serial-dot model rejected at order 8)."""
    taken = None
    for n in (8, 9, 10):
        a = MC.hilbert(n)
        got = R.refine(a, R.Lowered(a), None, np.ones(n), np.zeros(n), MC.OUTER_TOL, MC.OUTER_CAP, MC.INNER_TOL, MC.INNER_CAP)
        if got.rejected:
            taken = (n, got)
            break
    assert taken is not None
    n, got = taken
    print("rejected at order", n, "outer step", got.iterations)
    assert got.code == 0 and not got.converged and got.iterations == len(got.inner_iterations) == len(got.history) - 1
    assert not (got.history[-1] < got.history[-2]) and got.final_residual == min(got.history)


def test_exit_inner_error():
    a = MC.singular_when_lowered()
    a32 = R.Lowered(a)
    assert a32.info["changed"] == 2 and np.all(a32.vals32 == 1.0)
    x0 = np.array([0.5, -0.5])                                                            # (the residual stays a multiple of (1, -1))
    got = R.refine(a, a32, None, np.array([1.0, -1.0]), x0, 1e-10, 10, MC.INNER_TOL, 50)
    assert got.code == R.INDEFINITE_MATRIX and got.iterations == 0 and not got.converged
    assert np.array_equal(got.x, x0) and got.inner_iterations == [1] and len(got.history) == 1


def test_exit_max_iters_zero_and_zero_residual():
    a = MC.poisson12()
    a32 = R.Lowered(a)
    b = MC.rhs(a.nrows)
    got = R.refine(a, a32, None, b, np.zeros(a.nrows), 1e-10, 0, MC.INNER_TOL, 50)
    assert got.code == 0 and got.converged and got.iterations == 0 and got.history == [got.final_residual] and got.inner_iterations == []
    got = R.refine(a, a32, None, np.zeros(a.nrows), np.zeros(a.nrows), 1e-10, 5, MC.INNER_TOL, 50)
    assert got.code == 0 and got.converged and got.iterations == 0 and got.final_residual == 0.0 and got.inner_iterations == []


def test_exit_outer_cap():
    a = MC.poisson12()
    got = R.refine(a, R.Lowered(a), None, MC.rhs(a.nrows), np.zeros(a.nrows), 1e-30, 2, MC.INNER_TOL, MC.INNER_CAP)
    # the reference's quirk: reaching the cap reports converged (convergence.rs:18-34)
    assert got.code == 0 and got.iterations == 2 and got.converged and len(got.history) == 3 and got.final_residual > 1e-30 * got.history[0]
