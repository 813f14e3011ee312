"""AMG as written without a GPU: the dense transliteration of amg.rs (tests/amg_ref.py) against the reference's own unit tests, and
the host set-up kryst_host_amg (kryst_amd/csrc/amg_setup.cpp) against the transliteration."""
import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import amg_ref as R


def dense_of(t):
    nr, nc, rp, ci, va = t
    m = np.zeros((nr, nc))
    for i in range(nr):
        m[i, ci[rp[i]:rp[i + 1]]] = va[rp[i]:rp[i + 1]]
    return m


def host_levels(a, max_levels, thr, budget=0):
    return K.host_amg(a.row_ptr, a.col_idx.astype(np.int32), a.vals, max_levels, thr, budget)


@pytest.mark.parametrize("m,r", [
    ([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]], [5.0, 5.0, 3.0]),                                   # amg.rs:827-849
    ([[4.0, 1.0, 0.0, 0.0], [1.0, 3.0, 1.0, 0.0], [0.0, 1.0, 2.0, 1.0], [0.0, 0.0, 1.0, 4.0]], [5.0, 5.0, 3.0, 1.0]),   # :852-875
])
def test_reference_unit_tests_residual_below_one(m, r):
    m = np.array(m); r = np.array(r)
    levels = R.amg_new_dense(m, 2, 0.1)
    z = R.vcycle(R.csr_levels(levels), r, np.zeros(len(r)))
    assert np.linalg.norm(r - m @ z) < 1.0


def test_reference_smooth_interpolation_matrices():          # amg.rs:877-933
    p = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])
    R.smooth_interpolation(p, np.array([[0.5] * 3, [1.0] * 3, [1.5] * 3]), 0.5)
    assert np.array_equal(p, [[0.75, 1.75, 2.75], [3.5, 4.5, 5.5], [6.25, 7.25, 8.25]])
    p = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.0, 10.0, 11.0, 12.0]])
    R.smooth_interpolation(p, np.array([[0.5, 0.5], [1.0, 1.0], [1.5, 1.5]]), 1.0)
    assert np.array_equal(p, [[0.5, 1.5, 3.0, 4.0], [4.0, 5.0, 7.0, 8.0], [7.5, 8.5, 11.0, 12.0]])


@pytest.mark.parametrize("kind,N,thr", [("poisson", 4, 0.1), ("poisson", 5, 0.25), ("aniso", 4, 0.1), ("varcoef", 4, 0.05),
                                        ("convdiff", 4, 0.1)])
def test_host_setup_matches_the_transliteration(kind, N, thr):
    a = O.stencil7(N, kind)
    ref = R.amg_new_dense(a.to_dense(), 10, thr)
    got = host_levels(a, 10, thr)
    assert len(got) == len(ref) >= 2
    for g, r in zip(got, ref):
        assert np.array_equal(g["dinv"], r["dinv"])
        if r["agg"] is not None:
            assert np.array_equal(g["agg"], r["agg"])
        for key in ("A", "P", "R"):
            if r[key] is None:
                assert g[key] is None
                continue
            gd = dense_of(g[key])
            assert gd.shape == r[key].shape
            scale = max(np.abs(r[key]).max(), 1e-300)
            assert np.abs(gd - r[key]).max() <= 1e-12 * scale, key
            rp = g[key][2]
            for i in range(len(rp) - 1):                        # rows strictly ascending
                assert np.all(np.diff(g[key][3][rp[i]:rp[i + 1]]) > 0)


def test_host_setup_levels_stop_at_ten_rows_and_at_max_levels():
    a = O.stencil7(4)
    lv = host_levels(a, 10, 0.1)
    assert lv[-1]["A"][0] <= 10 and all(L["A"][0] > 10 for L in lv[:-1])
    assert len(host_levels(a, 1, 0.1)) == 2
    only = host_levels(a, 0, 0.1)
    assert len(only) == 1 and only[0]["P"] is None and only[0]["A"][0] == a.nrows


def test_vcycle_restatement_matches_dense_transliteration():
    a = O.stencil7(4)
    levels = R.amg_new_dense(a.to_dense(), 10, 0.1)
    rng = np.random.default_rng(3)
    r = rng.standard_normal(a.nrows); z0 = rng.standard_normal(a.nrows)
    z = R.vcycle(R.csr_levels(levels), r, z0)
    # the same cycle on dense matrices
    def vc(l, r, z):
        L = levels[l]
        if l + 1 == len(levels):
            A = L["A"]; x = np.zeros(len(r)); res = r.copy(); p = res.copy(); rr = res @ res
            for _ in range(len(r)):                          # solve_direct (:254-312): CG, not an exact solve (A_c is not symmetric)
                ap = A @ p; al = rr / (p @ ap); x = x + al * p; res = res - al * ap; rr_old, rr = rr, res @ res
                if np.sqrt(rr) < 1e-10:
                    break
                p = res + rr / rr_old * p
            return x
        A = L["A"]
        z = z + L["dinv"] * (r - A @ z)
        zc = vc(l + 1, L["R"] @ (r - A @ z), np.zeros(L["R"].shape[0]))
        z = z + L["P"] @ zc
        return z + L["dinv"] * (r - A @ z)
    assert np.allclose(z, vc(0, r, z0), rtol=1e-8, atol=1e-10)


def test_fill_budget_error():
    a = O.stencil7(6)
    assert len(host_levels(a, 10, 0.1)) >= 2
    with pytest.raises(K.KError) as e:
        host_levels(a, 10, 0.1, budget=a.nnz // 2)
    assert e.value.code == 1 and "fill budget" in str(e.value)


def test_host_setup_argument_errors():
    a = O.stencil7(3)
    with pytest.raises(K.KError) as e:
        host_levels(a, -1, 0.1)
    assert e.value.code == 102
    ci = a.col_idx.astype(np.int32).copy()
    ci[[0, 1]] = ci[[1, 0]]                                          # row 0 no longer ascending
    with pytest.raises(K.KError) as e:
        K.host_amg(a.row_ptr, ci, a.vals, 10, 0.1)
    assert e.value.code == 102


def test_pc_amg_factory():
    p = K.PC.AMG()
    assert p.kind == "AMG" and p.params == {"max_levels": 10, "threshold": 0.1}
    amg = K.Amg(4, 0.2)
    assert (amg.max_levels, amg.threshold, amg.nu_pre, amg.nu_post) == (4, 0.2, 1, 1)


def test_sa_restatement_aggregates_are_a_distance_two_mis_partition():
    a = O.stencil7(8)
    agg = R.sa_aggregates(a)
    assert agg.min() == 0 and set(np.unique(agg)) == set(range(agg.max() + 1))
    assert 8 ** 3 / 27 * 0.5 <= agg.max() + 1 <= 8 ** 3 / 4                 # aggregates of a few to 27 rows
    k = R.sa_key(np.arange(a.nrows))
    assert len(np.unique(k)) == a.nrows
    agg2, P, Rm, Ac, wd = R.sa_level(a)
    assert np.array_equal(agg, agg2) and np.allclose(Ac, Ac.T, rtol=0, atol=1e-12) and np.array_equal(Rm, P.T)
