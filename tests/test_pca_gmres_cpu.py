"""PcaGmresSolver restated in numpy (tests/pca_gmres_ref.py), checked without a GPU: the as-written form against a line-by-line
transliteration of pca_gmres.rs:99-312 and its quirks pinned; the s-step extension's basis, Arnoldi relation, iteration counts and
column rules.  The entry points are bound (kryst_amd.PcaGmresSolver)."""
import math

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import pca_gmres_ref as R


def _dense_nonsym(n, seed, spread=1.0):
    g = np.random.default_rng(seed)
    return np.eye(n) * 4.0 + spread * g.standard_normal((n, n)) / math.sqrt(n)


def _literal(A, b, restart, tol, max_iters):
    """pca_gmres.rs:99-312 read line by line with Python floats and serial sums (block size 1, pc None)"""
    n = len(b)
    dot = lambda u, v: sum((u[i] * v[i] for i in range(n)), 0.0)
    mv = lambda v: [sum((A[i][k] * v[k] for k in range(n)), 0.0) for i in range(n)]
    xk = [0.0] * n
    tmp = mv(xk)
    r0 = [bi - ax for ax, bi in zip(tmp, b)]
    beta = math.sqrt(dot(r0, r0)); res0 = beta
    stats = [0, beta, False]
    iteration = 0
    for _ in range((max_iters + restart - 1) // restart):
        V = [[ri / beta for ri in r0]]
        m = restart
        h = [[0.0] * m for _ in range(m + 1)]; g = [0.0] * (m + 1); g[0] = beta; cs = [0.0] * m; sn = [0.0] * m
        j = 0
        while j < m:
            w = mv(V[j])
            for i in range(j + 1):
                h[i][j] = dot(V[i], w)
            nv = math.sqrt(dot(w, w)); h[j + 1][j] = nv; inv = 1.0 / nv
            V.append([wi * inv for wi in w])
            col = j
            for i in range(col):
                temp = cs[i] * h[i][col] + sn[i] * h[i + 1][col]
                h[i + 1][col] = -sn[i] * h[i][col] + cs[i] * h[i + 1][col]
                h[i][col] = temp
            hk, hk1 = h[col][col], h[col + 1][col]
            r = math.sqrt(hk * hk + hk1 * hk1)
            if abs(r) < 2.220446049250313e-16:
                cs[col], sn[col] = 1.0, 0.0
            else:
                cs[col], sn[col] = hk / r, hk1 / r
            h[col][col] = cs[col] * hk + sn[col] * hk1; h[col + 1][col] = 0.0
            temp = cs[col] * g[col] + sn[col] * g[col + 1]
            g[col + 1] = -sn[col] * g[col] + cs[col] * g[col + 1]; g[col] = temp
            gn = abs(g[j + 1]); iteration += 1
            stop = gn / res0 <= tol or iteration >= max_iters
            stats = [iteration, gn, stop]
            if stop:
                break
            j += 1
        y = [0.0] * j
        for i in range(j - 1, -1, -1):
            s = g[i]
            for k in range(i + 1, j):
                s = s - h[i][k] * y[k]
            if abs(h[i][i]) > 2.220446049250313e-16:
                y[i] = s / h[i][i]
        for i in range(j):
            xk = [xi + y[i] * qi for xi, qi in zip(xk, V[i])]
        tmp = mv(xk)
        r0 = [bi - ax for ax, bi in zip(tmp, b)]
        beta = math.sqrt(dot(r0, r0)); stats[1] = beta; stats[2] = beta <= tol * res0
        if stats[2] or iteration >= max_iters:
            break
    return np.array(xk), stats


@pytest.mark.parametrize("restart,tol,mx", [(1, 1e-8, 9), (5, 1e-6, 40), (30, 1e-3, 30), (4, 0.0, 13)])
def test_as_written_matches_literal_transliteration(restart, tol, mx):
    A = _dense_nonsym(12, restart)
    a = O.Csr.from_dense(A)
    b = np.random.default_rng(1).standard_normal(12)
    x, st = _literal(A.tolist(), b.tolist(), restart, tol, mx)
    ref = R.as_written(a, b, restart=restart, tol=tol, max_iters=mx, rs=O.Reduce.serial())
    assert [ref.iterations, ref.final_residual, ref.converged] == [st[0], st[1], st[2]]
    assert np.array_equal(ref.x, x)


def test_as_written_quirks():
    A = _dense_nonsym(10, 3); a = O.Csr.from_dense(A)
    b = np.random.default_rng(2).standard_normal(10)
    base = R.as_written(a, b, restart=5, tol=1e-6, max_iters=40)
    # x0 is ignored (:107)
    assert np.array_equal(R.as_written(a, b, x=np.ones(10), restart=5, tol=1e-6, max_iters=40).x, base.x)
    # no orthogonalisation: the first cycle's basis is the normalised power sequence A^k r0 (not orthogonal)
    v = b / np.linalg.norm(b); vs = [v]
    for _ in range(3):
        w = A @ vs[-1]; vs.append(w / np.linalg.norm(w))
    Vm = np.array(vs).T
    assert np.abs(Vm.T @ Vm - np.eye(4)).max() > 1e-2
    # m_eff = j: with restart 1 and one iteration the check stops the first block and its column is left out: x = 0
    r = R.as_written(a, b, restart=1, tol=1e-8, max_iters=1)
    assert r.iterations == 1 and not np.any(r.x) and r.final_residual == math.sqrt(O.dot(b, b)) and not r.converged
    # converged comes from the true residual (:304), not from the check's cap rule
    r = R.as_written(a, b, restart=5, tol=1e-12, max_iters=3)
    assert r.iterations == 3 and not r.converged
    # Right = M^-1 A with the update in V; Left never calls pc
    pc = O.Pc.jacobi(a)
    assert np.array_equal(R.as_written(a, b, pc=pc, side=1, restart=5, tol=1e-6, max_iters=40).x, base.x)
    rr = R.as_written(a, b, pc=pc, side=2, restart=5, tol=1e-6, max_iters=40)
    assert not np.array_equal(rr.x, base.x)
    # max_iters = 0, b = 0
    r = R.as_written(a, b, restart=5, tol=1e-8, max_iters=0)
    assert (r.iterations, r.converged) == (0, False) and not np.any(r.x)
    r = R.as_written(a, np.zeros(10), restart=5, tol=1e-8, max_iters=4)
    assert np.isnan(r.final_residual) and np.all(np.isnan(r.x)) and not r.converged
    # where the reference panics or never returns
    for restart, bs, mx in ((6, 2, 30), (2, 5, 1), (5, 0, 10), (0, 1, 10)):
        with pytest.raises(R.ArgError):
            R.as_written(a, b, restart=restart, block_size=bs, max_iters=mx)
    R.as_written(a, b, restart=1, block_size=3, max_iters=5)          # t = min(s, 1) = 1 runs
    R.as_written(a, b, restart=6, block_size=2, max_iters=0)          # no cycle, no panic


def _gmres_mgs(A, b, m, tol, max_iters):
    """independent GMRES(m): modified Gram-Schmidt, the least-squares problem by numpy.linalg.lstsq at every step"""
    n = len(b); x = np.zeros(n); r0n = np.linalg.norm(b); it = 0
    while it < max_iters:
        r = b - A @ x; beta = np.linalg.norm(r)
        if beta <= tol * r0n:
            return it
        Q = np.zeros((n, m + 1)); H = np.zeros((m + 1, m)); Q[:, 0] = r / beta
        for j in range(m):
            w = A @ Q[:, j]
            for i in range(j + 1):
                H[i, j] = Q[:, i] @ w; w = w - H[i, j] * Q[:, i]
            H[j + 1, j] = np.linalg.norm(w)
            if H[j + 1, j] > 0:
                Q[:, j + 1] = w / H[j + 1, j]
            e = np.zeros(j + 2); e[0] = beta
            y = np.linalg.lstsq(H[:j + 2, :j + 1], e, rcond=None)[0]
            it += 1
            if np.linalg.norm(e - H[:j + 2, :j + 1] @ y) <= tol * r0n or it >= max_iters:
                x = x + Q[:, :j + 1] @ y
                if np.linalg.norm(e - H[:j + 2, :j + 1] @ y) <= tol * r0n:
                    return it
                break
        else:
            x = x + Q[:, :m] @ y
    return it


def _systems():
    A = _dense_nonsym(60, 7)
    s = O.stencil7(8, "convdiff")
    return [(A, O.Csr.from_dense(A)), (s.to_dense(), s)]


@pytest.mark.parametrize("sb", [1, 3, 5])
def test_sstep_basis_and_arnoldi_relation(sb):
    """||Q^T Q - I|| <= 1e-12 and ||A M^-1 Q_k - Q_{k+1} H|| <= 1e-12 ||A||.  The dense operator at s = 5 is the exception for the first
    and the second: its scaled monomial blocks are nearly dependent (A is close to 4 I), and CholQR2 leaves 1.06e-12 in Q^T Q - I and
    1.33e-12 ||A|| in the relation there (measured), so that one case is held to 2e-12."""
    for idx, (A, a) in enumerate(_systems()):
        otol = 2e-12 if (idx == 0 and sb == 5) else 1e-12
        b = np.random.default_rng(4).standard_normal(a.nrows)
        for pc in (None, O.Pc.jacobi(a)):
            r = R.sstep(a, b, pc=pc, side=2, restart=12, block_size=sb, tol=1e-10, max_iters=24)
            Minv = np.diag(1.0 / np.diag(A)) if pc is not None else np.eye(a.nrows)
            anorm = np.linalg.norm(A, 2)
            for cyc in r.cycles:
                m, Q, Hu = cyc["m"], cyc["Q"], cyc["Hu"]
                k = min(Q.shape[1], m + 1)
                assert np.abs(Q[:, :k].T @ Q[:, :k] - np.eye(k)).max() <= otol
                lhs = A @ Minv @ Q[:, :m]
                assert np.linalg.norm(lhs - Q[:, :k] @ Hu[:k, :m]) <= otol * anorm


@pytest.mark.parametrize("sb", [1, 5])
def test_sstep_iterations_match_independent_gmres(sb):
    for A, a in _systems():
        b = np.random.default_rng(6).standard_normal(a.nrows)
        want = _gmres_mgs(A, b, 20, 1e-9, 400)
        r = R.sstep(a, b, side=0, restart=20, block_size=sb, tol=1e-9, max_iters=400)
        assert r.converged and abs(r.iterations - want) <= 1, (r.iterations, want)
        assert np.linalg.norm(b - A @ r.x) <= 1e-9 * np.linalg.norm(b) * (1 + 1e-9)


def test_sstep_truncation_and_happy_breakdown():
    n = 40
    g = np.random.default_rng(5)
    P = np.eye(n) + 0.1 * g.standard_normal((n, n))
    A = P @ np.diag(np.resize([1.0, 2.0, 3.0], n)) @ np.linalg.inv(P)     # three distinct eigenvalues: Krylov dimension 3
    a = O.Csr.from_dense(A)
    b = g.standard_normal(n)
    r = R.sstep(a, b, side=0, restart=10, block_size=5, tol=0.0, max_iters=10)
    assert r.events[0] == ("truncate", 0, 2, 5)          # the first block keeps w_1, w_2: A^3 r0 lies in the span
    assert r.events[1] == ("happy", 2)                   # A q_2 lies in span(q_0, q_1, q_2): kept with a zero subdiagonal
    assert r.cycles[0]["m"] == 3 and r.history[2] <= 1e-12 * np.linalg.norm(b)
    assert np.linalg.norm(b - A @ r.x) <= 1e-10 * np.linalg.norm(b)


def test_sstep_rules():
    A = _dense_nonsym(8, 1); a = O.Csr.from_dense(A); b = np.ones(8)
    with pytest.raises(R.Unsupported):
        R.sstep(a, b, pc=O.Pc.jacobi(a), side=1)
    for sb in (0, 17):
        with pytest.raises(R.ArgError):
            R.sstep(a, b, block_size=sb)
    r = R.sstep(a, np.zeros(8), restart=5, block_size=2, max_iters=10)      # r0 = 0: x0 already solves the system
    assert (r.iterations, r.final_residual, r.converged) == (0, 0.0, True)
    r = R.sstep(a, b, x=np.ones(8), restart=4, block_size=3, tol=0.0, max_iters=7)       # x0 honoured, the last block shortened
    assert r.iterations == 7 and len(r.history) == 7


def test_entry_points_are_bound():
    for nm in ("kryst_pca_gmres_solve", "kryst_pca_gmres_solve_dev", "kryst_pca_gmres_textbook_solve_dev"):
        assert nm in _ffi.SIGNATURES and hasattr(K.lib(), nm)
    s = K.PcaGmresSolver(30, 2, 5, 1e-8, 100)
    assert s.preconditioning == K.Preconditioning.Left and s._extra() == (5, 2, 0.0)
    assert s.with_tau(0.5).with_textbook()._DEV == "kryst_pca_gmres_textbook_solve_dev"
