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


# ----------------------------------------------------------------------------- smoothed aggregation: the ordered restatement
import fractions

import scipy.sparse as sp

import sa_cases as S

U = 2.0 ** -53

# small forms of the GPU tier's matrix set (tests/test_gpu_amg_sa.py): (name, matrix, theta)
SA_CPU_CASES = {
    "poisson8": lambda: (O.stencil7(8), 0.0), "aniso8": lambda: (O.stencil7(8, "aniso"), 0.0),
    "varcoef8": lambda: (O.stencil7(8, "varcoef"), 0.0), "convdiff8": lambda: (O.stencil7(8, "convdiff"), 0.0),
    "poisson12": lambda: (O.stencil7(12), 0.0), "op27_6": lambda: (S.op27(6, 1), 0.0),
    "graph600": lambda: (S.graph_laplacian(600, 2, hub=300), 0.0), "dirichlet8": lambda: (S.dirichlet_poisson(8), 0.0),
    "aniso8_theta005": lambda: (O.stencil7(8, "aniso"), 0.05), "poisson6_theta02": lambda: (O.stencil7(6), 0.2),
    "diagonal500": lambda: (S.diagonal(500), 0.0),
}


def sa_levels_cpu(name):
    a, theta = SA_CPU_CASES[name]()
    return R.sa_hierarchy(a, theta=theta), theta


def coarsened(H):
    """(A_l, the ordered level) of every level that was coarsened, and of a stalled last level"""
    return [(L["A"], L["lvl"]) for L in H if L["lvl"] is not None]


def absmat(c):
    return sp.csr_matrix((np.abs(c.vals), c.col_idx, c.row_ptr), shape=(c.nrows, c.ncols))


def spm(c):
    return sp.csr_matrix((c.vals, c.col_idx, c.row_ptr), shape=(c.nrows, c.ncols))


def p_scale(a, o):
    """|P0| + omega |D^-1| |A| |P0| on P's pattern (dense: the levels here are small)"""
    n = a.nrows
    P0 = sp.csr_matrix((o["p0"], o["agg"], np.arange(n + 1)), shape=(n, o["nc"]))
    s = abs(P0) + sp.diags(o["omega"] * np.abs(o["dinv"])) @ absmat(a) @ abs(P0)
    return s.toarray()


def ac_scale(a, P):
    return (absmat(P).T @ absmat(a) @ absmat(P)).toarray()


def kmax(c):
    return int(np.diff(c.row_ptr).max()) if c.nrows else 0


@pytest.mark.parametrize("name", list(SA_CPU_CASES))
def test_sa_ordered_level_matches_the_dense_restatement(name):
    """every level of the ordered hierarchy against the independent dense route (amg_ref.sa_level: numpy's A @ P0, omega / d).  Both
    round a k-term row sum, the ratio rho, omega, 1/d (or omega / d) and three more operations: c = 2 k + 8 for P, k the longest row
    of A; A_c is compared with the dense P^T (A P) of the same P: c = k_A + k_R + 4."""
    H, theta = sa_levels_cpu(name)
    for a, o in coarsened(H):
        agg, P, Rm, Ac, wd = R.sa_level(a, theta)
        assert np.array_equal(o["agg"], agg)
        Pd = o["P"].to_dense()
        c = 2 * kmax(a) + 8
        assert np.all(np.abs(Pd - P) <= c * U * p_scale(a, o))
        assert np.all(np.abs(o["wdinv"] - wd) <= (2 * kmax(a) + 4) * U * np.abs(wd))     # rho: two k-term row sums
        Ad = a.to_dense()
        c = kmax(a) + kmax(o["R"]) + 4
        assert np.all(np.abs(o["Ac"].to_dense() - Pd.T @ (Ad @ Pd)) <= c * U * ac_scale(a, o["P"]))
        assert np.array_equal(o["R"].to_dense(), Pd.T)                          # R = P^T exactly
        # the dense route's own A_c from its own P: the same bound, with the P bound carried through |R| |A| and |A| |P|
        e = (2 * kmax(a) + 8) * U * p_scale(a, o)
        carry = (np.abs(Pd).T @ np.abs(Ad) @ e + e.T @ np.abs(Ad) @ np.abs(Pd) + e.T @ np.abs(Ad) @ e)
        assert np.all(np.abs(o["Ac"].to_dense() - Ac) <= c * U * ac_scale(a, o["P"]) + carry)


def two_prod(x, y):
    """x * y = p + e exactly (Dekker / Veltkamp, no fused multiply-add)"""
    sp_ = 134217729.0
    def split(v):
        t = sp_ * v
        hi = t - (t - v)
        return hi, v - hi
    p = x * y
    xh, xl = split(x); yh, yl = split(y)
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def ld_spgemm(ap, ac, av, bp, bc, bv, nb):
    """C = A B in np.longdouble with every product formed exactly (two_prod) -> dense (n, nb) longdouble"""
    n = len(ap) - 1
    rows = np.repeat(np.arange(n), np.diff(ap))
    out = np.zeros((n, nb), dtype=np.longdouble)
    blen = np.diff(bp)[ac]
    rep = np.repeat(np.arange(len(ac)), blen)
    h = np.repeat(bp[ac], blen) + (np.arange(len(rep)) - np.repeat(np.cumsum(blen) - blen, blen))
    if np.asarray(av).dtype == np.longdouble or np.asarray(bv).dtype == np.longdouble:
        prod = np.asarray(av, dtype=np.longdouble)[rep] * np.asarray(bv, dtype=np.longdouble)[h]
        np.add.at(out, (rows[rep], bc[h]), prod)
    else:
        p, e = two_prod(np.asarray(av)[rep], np.asarray(bv)[h])
        np.add.at(out, (rows[rep], bc[h]), p.astype(np.longdouble))
        np.add.at(out, (rows[rep], bc[h]), e.astype(np.longdouble))
    return out


def exact_p_ac_fraction(a, o):
    """P = P0 - omega D^-1 A P0 and A_c = P^T A P in exact rational arithmetic, from the doubles omega, p0 and the ordered P"""
    F = fractions.Fraction
    n, nc = a.nrows, o["nc"]
    A = [{int(a.col_idx[k]): F(float(a.vals[k])) for k in range(a.row_ptr[i], a.row_ptr[i + 1])} for i in range(n)]
    p0 = [F(float(v)) for v in o["p0"]]
    om = F(float(o["omega"]))
    P = np.zeros((n, nc), dtype=object); P[:] = F(0)
    for i in range(n):
        acc = {}
        for k, v in A[i].items():
            acc[o["agg"][k]] = acc.get(o["agg"][k], F(0)) + v * p0[k]
        for J, s in acc.items():
            P[i, J] = (p0[i] if J == o["agg"][i] else F(0)) - om / A[i][i] * s
    Pd = o["P"].to_dense()
    Pq = [{J: F(float(Pd[i, J])) for J in np.flatnonzero(Pd[i])} for i in range(n)]
    AP = []
    for i in range(n):
        acc = {}
        for k, v in A[i].items():
            for J, pv in Pq[k].items():
                acc[J] = acc.get(J, F(0)) + v * pv
        AP.append(acc)
    Ac = np.zeros((nc, nc), dtype=object); Ac[:] = F(0)
    for i in range(n):
        for I, pv in Pq[i].items():
            for J, v in AP[i].items():
                Ac[I, J] += pv * v
    return P, Ac


def exact_p_ac_longdouble(a, o):
    """the same in np.longdouble, every double product formed exactly: error ~ k 2^-64 relative to the absolute-value products"""
    n, nc = a.nrows, o["nc"]
    rp, ci, va = a.row_ptr, a.col_idx, a.vals
    AP0 = ld_spgemm(rp, ci, va, np.arange(n + 1), o["agg"], o["p0"], nc)
    w = np.longdouble(o["omega"]) / np.asarray(o["d"], dtype=np.longdouble)
    P = -w[:, None] * AP0
    P[np.arange(n), o["agg"]] += np.asarray(o["p0"], dtype=np.longdouble)
    Pc = o["P"]
    AP = ld_spgemm(rp, ci, va, Pc.row_ptr, Pc.col_idx, Pc.vals, nc)
    Ac = spm(Pc).T.toarray().astype(np.longdouble) @ AP
    return P, Ac


@pytest.mark.parametrize("name,exact", [("poisson4", "fraction"), ("aniso5", "fraction"), ("convdiff6", "fraction"),
                                        ("varcoef6", "fraction"), ("poisson12", "longdouble"), ("op27_6", "longdouble"),
                                        ("graph600", "longdouble"), ("dirichlet8", "longdouble"), ("aniso8_theta005", "longdouble")])
def test_sa_ordered_level_against_exact_arithmetic(name, exact):
    """the ordered P and A_c of every level against exact arithmetic on the same doubles (omega, p0, and for A_c the ordered P): P
    within (k + 5) u (|P0| + omega |D^-1| |A| |P0|) (a k-term sum from 0.0, 1/d, omega * (1/d), the product and the subtraction);
    A_c within (k_A + k_R + 2) u |P|^T |A| |P|"""
    small = {"poisson4": lambda: (O.stencil7(4), 0.0), "aniso5": lambda: (O.stencil7(5, "aniso"), 0.0),
             "convdiff6": lambda: (O.stencil7(6, "convdiff"), 0.0), "varcoef6": lambda: (O.stencil7(6, "varcoef"), 0.0)}
    a, theta = (small.get(name) or SA_CPU_CASES[name])()
    H = R.sa_hierarchy(a, theta=theta)
    lv = coarsened(H) or [(a, R.sa_level_ordered(a, theta))]          # 4^3: no coarse level; check the one level it would form
    for a_l, o in lv:
        P, Ac = (exact_p_ac_fraction if exact == "fraction" else exact_p_ac_longdouble)(a_l, o)
        Pd = o["P"].to_dense()
        tolp = (kmax(a_l) + 5) * U * p_scale(a_l, o)
        tola = (kmax(a_l) + kmax(o["R"]) + 2) * U * ac_scale(a_l, o["P"])
        if exact == "fraction":
            assert all(abs(fractions.Fraction(float(Pd[i, j])) - P[i, j]) <= fractions.Fraction(float(tolp[i, j]))
                       for i in range(P.shape[0]) for j in range(P.shape[1]))
            Acd = o["Ac"].to_dense()
            assert all(abs(fractions.Fraction(float(Acd[i, j])) - Ac[i, j]) <= fractions.Fraction(float(tola[i, j]))
                       for i in range(Ac.shape[0]) for j in range(Ac.shape[1]))
        else:
            assert np.all(np.abs(Pd.astype(np.longdouble) - P) <= tolp)
            assert np.all(np.abs(o["Ac"].to_dense().astype(np.longdouble) - Ac) <= tola)
        # the pattern: P on the pattern of A P0, A_c on the pattern of R (A P)
        assert np.array_equal(Pd != 0, (Pd != 0) & (spm(a_l).astype(bool) @ sp.csr_matrix(
            (np.ones(a_l.nrows), o["agg"], np.arange(a_l.nrows + 1)), shape=(a_l.nrows, o["nc"])).astype(bool)).toarray())


@pytest.mark.parametrize("name", list(SA_CPU_CASES))
def test_sa_aggregation_is_a_distance_two_mis_partition_on_every_level(name):
    """on every level: a partition of the rows; roots numbered in row order, each in its own aggregate; every other member has a strong
    edge to its root (pass 1) or to a pass-1 member (pass 2), or is a leftover singleton numbered after the roots; with symmetric
    strength the roots are at strong-graph distance >= 3 and every row is within distance 2 of a root"""
    H, theta = sa_levels_cpu(name)
    for a, o in coarsened(H):
        n = a.nrows
        agg, roots, nc = o["agg"], np.asarray(o["roots"]), o["nc"]
        rows = np.repeat(np.arange(n), np.diff(a.row_ptr))
        d = np.zeros(n); dm = a.col_idx == rows; d[rows[dm]] = a.vals[dm]
        strong = (a.col_idx != rows) & (np.abs(a.vals) > theta * np.sqrt(np.abs(d[rows] * d[a.col_idx])))
        Sg = sp.csr_matrix((np.ones(strong.sum()), (rows[strong], a.col_idx[strong])), shape=(n, n)).astype(bool).tocsr()
        assert agg.shape == (n,) and agg.min() >= 0 and np.array_equal(np.unique(agg), np.arange(nc))      # a partition, numbered densely
        nr = len(roots)
        assert np.all(np.diff(roots) > 0) and np.array_equal(agg[roots], np.arange(nr))                 # roots in row order, own aggregate
        root_of = np.where(agg < nr, roots[np.minimum(agg, nr - 1)] if nr else 0, -1)
        pass1 = np.zeros(n, dtype=bool)
        member = (agg < nr) & ~np.isin(np.arange(n), roots)
        i1 = np.flatnonzero(member)
        pass1[i1] = np.asarray(Sg[i1, root_of[i1]]).ravel()
        pass1[roots] = True                                       # a pass-2 member may hang off the root itself
        for i in np.flatnonzero(member & ~pass1):
            nb = Sg.indices[Sg.indptr[i]:Sg.indptr[i + 1]]
            assert np.any(pass1[nb] & (agg[nb] == agg[i])), (name, i)
        left = np.flatnonzero(agg >= nr)
        assert np.array_equal(agg[left], nr + np.arange(len(left)))                                      # singletons after the roots
        if len(left):
            near = (Sg @ sp.csr_matrix(pass1.reshape(-1, 1).astype(float))).toarray().ravel() > 0
            assert not np.any(near[left])                          # a leftover has no strong edge to a root or pass-1 member
        if (Sg != Sg.T).nnz == 0:
            S2 = (Sg @ Sg + Sg).astype(bool).tocsr()
            sub = S2[roots][:, roots]
            assert sub.nnz == 0 or np.all(sub.tocoo().row == sub.tocoo().col)                     # roots at distance >= 3
            reach = (S2[:, roots].sum(axis=1).A.ravel() > 0) | np.isin(np.arange(n), roots)
            assert np.all(reach)                                                                    # maximal: nothing further than 2
