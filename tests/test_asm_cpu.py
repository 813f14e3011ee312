"""Additive Schwarz without a GPU: the numpy restatement (tests/asm_ref.py) pinned independently of the device -- the reference's own test,
the uniform partition with its capacity quirk, growth against brute force, the pay-off over block Jacobi -- and the public surface."""
import os
import re

import numpy as np
import pytest

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O
import asm_ref as A
import amg_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_asm_dense_lu_blocks():
    """asm.rs:125-137: the 4x4 identity, subdomains [0, 1] and [2, 3]: z == r"""
    a = O.Csr.from_dense(np.eye(4), keep_zeros=True)
    gs, own, inv, zp = A.setup(a, [[0, 1], [2, 3]])
    assert zp == [-1, -1] and all(np.array_equal(t, np.eye(2)) for t in inv)
    r = np.array([1.0, 2.0, 3.0, 4.0])
    assert np.array_equal(A.Apply(4, gs, inv)(r), r)
    assert np.array_equal(A.apply_loop(4, gs, inv, r), r)


@pytest.mark.parametrize("n", [1, 10, 17])
def test_uniform_partition_capacity(n):
    for p in (0, 1, 3, n, n + 2):
        parts = A.uniform_parts(n, p)
        assert len(parts) == max(p, 1)
        chunk = -(-n // max(p, 1))
        assert np.array_equal(np.concatenate(parts), np.arange(n))
        assert all(len(g) <= chunk for g in parts)
    assert [len(g) for g in A.uniform_parts(n, 0)] == [n]              # Vec::new(): capacity 0 -> one subdomain of all n rows
    assert [len(g) for g in A.uniform_parts(n, n + 2)][-2:] == [0, 0]   # trailing parts are empty
    assert [len(g) for g in A.uniform_parts(10, 3)] == [4, 4, 2]
    assert [len(g) for g in A.uniform_parts(10, 4)] == [3, 3, 3, 1]


def _random_pattern(n, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 3)
    cols = np.concatenate([[i, (i + rng.integers(1, n)) % n, rng.integers(0, n)] for i in range(n)])
    m = np.zeros((n, n))
    m[rows, cols] = 1.0
    return O.Csr.from_dense(m, keep_zeros=False)


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_growth_equals_brute_force(overlap):
    a = O.stencil7(6, "poisson")
    ptr, idx = K.AdditiveSchwarz.grid_boxes(6, (2, 3, 2))
    sets = [idx[ptr[k]:ptr[k + 1]][::-1] for k in range(len(ptr) - 1)]
    want = A.grow_dense(a.nrows, a.row_ptr, a.col_idx, sets, overlap)
    got = A.grow(a.nrows, a.row_ptr, a.col_idx, sets, overlap)
    assert all(np.array_equal(u, v) for u, v in zip(got, want))
    if overlap == 1:                                   # a 2x3x2 box plus its face neighbours
        assert len(want[0]) == 12 + 4 + 6 + 6 - 0 - 0 and set(want[0]) >= set(sets[0])
    b = _random_pattern(120, overlap)                  # non-symmetric: A^T's columns count too
    rng = np.random.default_rng(overlap)
    sets = [rng.choice(120, 3, replace=False) for _ in range(15)]
    want = A.grow_dense(120, b.row_ptr, b.col_idx, sets, overlap)
    got = A.grow(120, b.row_ptr, b.col_idx, sets, overlap)
    assert all(np.array_equal(u, v) for u, v in zip(got, want))
    if overlap == 1:
        D = np.zeros((120, 120), bool)
        D[np.repeat(np.arange(120), np.diff(b.row_ptr)), b.col_idx] = True
        assert not np.array_equal(D, D.T)
        g0 = np.sort(sets[0])
        assert set(want[0]) == set(g0) | set(np.nonzero(D[g0].any(axis=0) | D[:, g0].any(axis=1))[0])


def test_owner_is_the_last_ungrown_set():
    own = A.owners(6, [[0, 1, 2], [2, 3], [3, 4]])
    assert list(own) == [0, 0, 1, 2, 2, -1]


def test_apply_vectorised_equals_the_loop():
    a = O.stencil7(5, "varcoef")
    rng = np.random.default_rng(3)
    sets = [rng.choice(a.nrows, int(s), replace=False) for s in rng.integers(0, 30, 12)]
    gs, own, inv, zp = A.setup(a, sets, overlap=1, variant="grown")
    r = rng.standard_normal(a.nrows)
    r[::7] = -0.0
    assert np.array_equal(A.Apply(a.nrows, gs, inv)(r), A.apply_loop(a.nrows, gs, inv, r))
    assert np.array_equal(A.Apply(a.nrows, gs, inv, own, restricted=True)(r), A.apply_loop(a.nrows, gs, inv, r, own, restricted=True))
    z = A.Apply(a.nrows, gs, inv)(np.full(a.nrows, -0.0))
    assert not np.signbit(z).any()                     # z = 0 first: -0.0 becomes +0.0


def test_overlap_pays_on_the_restatement():
    """16^3 Poisson, 4x4x2 boxes, PCG to 1e-8: ASM with one layer of overlap takes fewer iterations than block Jacobi on the boxes"""
    N = 16
    a = O.stencil7(N, "poisson")
    ptr, idx = K.AdditiveSchwarz.grid_boxes(N, (4, 4, 2))
    sets = [idx[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]
    T, V, F = K.reduce_spec()
    rs = O.Reduce.tiled(T, V, F)
    b = np.ones(a.nrows)
    its = {}
    for name, variant, overlap in (("bjacobi", "as_written", 0), ("asm1", "grown", 1)):
        gs, own, inv, zp = A.setup(a, sets, overlap=overlap, variant=variant)
        assert max(len(g) for g in gs) <= A.MAX_ROWS and all(z == -1 for z in zp)
        M = A.Apply(a.nrows, gs, inv)
        x, it, code, hist = AR.pcg(a, None, b, 1e-8, 500, rs, apply=lambda r, z: M(r))
        assert code == 0 and hist[-1] / hist[0] < 1e-6
        its[name] = it
    assert its["asm1"] < its["bjacobi"], its


def test_public_surface():
    assert issubclass(K.AdditiveSchwarz, K._Pc) and "AdditiveSchwarz" in K.__all__
    pc = K.AdditiveSchwarz(1, [[3, 1], [], [0]])
    assert list(pc.ptr) == [0, 2, 2, 3] and list(pc.idx) == [3, 1, 0] and pc.variant == 0
    assert pc.with_overlap().variant == 1 and pc.restricted().variant == 2
    assert K.AdditiveSchwarz().ptr is None and K.AdditiveSchwarz(subdomains=[]).ptr is None and K.AdditiveSchwarz(nparts=4).nparts == 4
    with pytest.raises(K.KError):
        K.AdditiveSchwarz(0, (np.array([0, 4]), np.array([1, 2])))
    p = K.PC.AdditiveSchwarz(1, [[0, 1]])
    assert p.kind == "AdditiveSchwarz" and p.params["overlap"] == 1
    with pytest.raises(K.KError) as e:                 # the bare kind keeps raising Unsupported, before it touches the operator
        K.PC("AdditiveSchwarz").build(None)
    assert e.value.code == 6
    for name in ("kryst_pc_asm", "kryst_pc_asm_uniform", "kryst_pc_asm_info", "kryst_pc_asm_export"):
        assert name in _ffi.SIGNATURES
    h = open(os.path.join(ROOT, "include", "kryst_hip.h")).read()
    assert re.search(r"KRYST_ASM_AS_WRITTEN = 0, KRYST_ASM_GROWN = 1, KRYST_ASM_RESTRICTED = 2, KRYST_ASM_MAX_ROWS = 128", h)
    assert "struct AdditiveSchwarz : DevicePc" in open(os.path.join(ROOT, "include", "kryst_hip.hpp")).read()


def test_grid_boxes():
    ptr, idx = K.AdditiveSchwarz.grid_boxes(6, (4, 4, 2))
    assert len(ptr) - 1 == 2 * 2 * 3 and np.array_equal(np.sort(idx), np.arange(216))
    assert list(np.diff(ptr)[:2]) == [32, 16]
    assert list(idx[:5]) == [0, 1, 2, 3, 6]
