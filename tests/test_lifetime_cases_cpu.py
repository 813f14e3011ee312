"""The tables of tests/lifetime_cases.py held against include/kryst_hip.h, and what of the handle lifetimes can be shown without a GPU: a
new entry point fails here until it is tabled (or exempted with a reason)."""
import gc
import os
import weakref

import numpy as np
import pytest

import kryst_amd as K
import lifetime_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def funcs():
    with open(os.path.join(ROOT, "include", "kryst_hip.h"), encoding="utf-8") as f:
        return L.header_functions(f.read())


def test_the_parser_reads_the_whole_header(funcs):
    names = [n for n, _ in funcs]
    assert len(names) == len(set(names))
    assert set(names) == set(K._ffi.SIGNATURES), set(names) ^ set(K._ffi.SIGNATURES)       # the binding declares every symbol of the header
    d = dict(funcs)
    assert d["kryst_cg_solve"][:5] == ["const double*", "double*", "int64_t", "kryst_csr_t", "kryst_pc_t"]      # (KRYST_SOLVE_ARGS expanded)
    assert d["kryst_vec_create"] == ["kryst_ctx_t", "int64_t", "kryst_vec_t*"]
    assert d["kryst_csr32_info"] == ["kryst_csr32_t", "int64_t*"]
    for n, ts in funcs:                                                                      # as many parameters as the binding passes
        assert len(ts) == len(K._ffi.SIGNATURES[n][1]), (n, ts)


def test_every_handle_creating_entry_point_is_tabled(funcs):
    creators = L.creators(funcs)
    assert "kryst_vec_create" in creators and "kryst_pc_amg" in creators and "kryst_session_begin" in creators and len(creators) >= 36
    tabled = {e for c in L.HANDLE_CASES.values() for e in c.entries}
    assert not tabled & set(L.CREATE_EXEMPT)
    assert sorted(tabled | set(L.CREATE_EXEMPT)) == creators, sorted((tabled | set(L.CREATE_EXEMPT)) ^ set(creators))
    assert all(isinstance(r, str) and len(r) > 10 for r in L.CREATE_EXEMPT.values())


def test_every_entry_point_with_two_handles_is_tabled(funcs):
    multi = L.multi_handle(funcs)
    assert "kryst_apply_chebyshev" in multi and "kryst_session_begin" in multi and "kryst_cbgmres_solve_dev" in multi
    assert "kryst_dense_from_csr" not in multi                                               # (one handle: nothing to mix)
    assert not set(L.TWO_CONTEXT) & set(L.TWO_CONTEXT_EXEMPT)
    assert sorted(set(L.TWO_CONTEXT) | set(L.TWO_CONTEXT_EXEMPT)) == multi, sorted((set(L.TWO_CONTEXT) | set(L.TWO_CONTEXT_EXEMPT)) ^ set(multi))
    assert all(isinstance(r, str) and len(r) > 10 for r in L.TWO_CONTEXT_EXEMPT.values())
    d = dict(funcs)
    for name, (kinds, _) in L.TWO_CONTEXT.items():                                           # the kinds of a call are the handles of its declaration
        want = sorted(t[len("kryst_"):-2] for t in d[name] if t in L.HANDLE_TYPES)
        assert sorted(k.rstrip("*") for k in kinds) == want, (name, kinds, want)


def test_repetitions_reach_what_the_table_says():
    assert L.G == 2 * 1024 * 1024 and L.reach(L.R_MAX) == 32 * 1024
    for name, c in L.HANDLE_CASES.items():
        assert 1 <= c.R <= L.R_MAX, name
    for name in ("vec", "mvec2", "mvec4", "mvec8", "vec32", "dense_create"):                # the one block of these is exactly at the reach
        assert not L.HANDLE_CASES[name].below
    assert 8 * (3584 + 512) * 64 == L.G and 8 * 2 * (1536 + 512) * 64 == L.G and 4 * (7168 + 1024) * 64 == L.G and 8 * 64 * 64 * 64 == L.G
    assert 8 * 4 * (1536 + 512) * L.HANDLE_CASES["mvec4"].R == L.G and 8 * 8 * (1536 + 512) * L.HANDLE_CASES["mvec8"].R == L.G
    # the A^T case reaches the transposition's counters (an int32 per column): what the mutation of csr_transpose loses
    assert 4 * L.ROWS * L.HANDLE_CASES["csr_transpose"].R >= L.G


def test_solver_tables():
    assert set(L.OWN_EXITS) <= set(L.SOLVERS)
    for name in ("cg", "pcg", "bicgstab", "bicgstab_rpc", "cgs", "tfqmr", "minres", "minres_textbook", "cgnr", "cgnr_textbook", "qmr", "fgmres",
                 "pca_gmres", "pca_gmres_sstep", "cb_gmres", "gmres_none", "gmres_left", "gmres_right", "gmres_left_textbook"):
        assert name in L.SOLVERS
    assert len(set(L.SOLVE_CASES)) == len(L.SOLVE_CASES)
    assert sorted(K.Session.METHODS.values()) == list(range(10))


# ------------------------------------------------------------------------------------------------ the binding's bookkeeping, no device
class FakeLib:
    """answers every library call with KRYST_OK and records its name and first argument"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, sym):
        def f(*args):
            first = args[0] if args else None
            self.calls.append((sym, getattr(first, "value", first)))
            return 0
        return f


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(K, "lib", lambda: lib)
    return lib


def _context(handle=1, nranks=1):
    """a Context object without a device: the real class, its fields filled in by hand"""
    c = K.Context.__new__(K.Context)
    c._children = {}
    c.h = K._ffi.Handle(handle) if handle else None
    c.rank, c.nranks, c.device = 0, nranks, 0
    return c


def _child(cls, ctx, handle=None):
    c = cls.__new__(cls)
    c.ctx, c.h = ctx, (K._ffi.Handle(handle) if handle else None)
    ctx._adopt(c)
    return c


def test_close_destroys_children_in_order_and_forgets_dead_ones(fake):
    ctx = _context(1)
    kinds = [K.DeviceVec, K.CsrMatrix, K.CsrMatrix32, K.Jacobi, K.Session, K.MultiVec, K.DenseMatrix, K.LuSolver, K.DeviceVec32, K.TrueIlu0]
    kids = [_child(c, ctx, 10 + i) for i, c in enumerate(kinds)]
    gone = _child(K.DeviceVec, ctx, 99)
    assert len(ctx._children) == len(kids) + 1
    del gone                                              # dropped: destroyed at once, and out of the registry
    gc.collect()
    assert fake.calls == [("kryst_vec_destroy", 99)] and len(ctx._children) == len(kids)
    del fake.calls[:]
    ctx.close()                                           # the real close(): sessions, preconditioners, lowered operators, operators, vectors; then the context
    assert fake.calls == [("kryst_session_end", 14), ("kryst_pc_destroy", 13), ("kryst_pc_destroy", 19), ("kryst_csr32_destroy", 12),
                          ("kryst_csr_destroy", 11), ("kryst_dense_destroy", 16), ("kryst_lu_destroy", 17), ("kryst_vec_destroy", 10),
                          ("kryst_mvec_destroy", 15), ("kryst_vec32_destroy", 18), ("kryst_ctx_destroy", 1)]
    assert all(k.h is None for k in kids) and ctx.h is None and not ctx._children
    del fake.calls[:]
    ctx.close()                                           # twice, and dropping the children afterwards: nothing is destroyed again
    del kids
    gc.collect()
    assert fake.calls == []


def test_children_of_a_closed_context_skip_their_destroy(fake):
    ctx = _context(1)
    v = _child(K.DeviceVec, ctx, 5)
    ctx._children.clear()                                 # (a child the context does not know: what a collector's cycle can leave)
    ctx.close()
    del v
    gc.collect()
    assert fake.calls == [("kryst_ctx_destroy", 1)]


def test_released_children_raise_kerror():
    """h = None is what close() leaves behind: every method then reaches the library's null check (or the binding's own)"""
    K.lib()
    ctx = _context(None)
    v, a, pc, m = _child(K.DeviceVec, ctx), _child(K.CsrMatrix, ctx), _child(K.Jacobi, ctx), _child(K.MultiVec, ctx)
    v.n, a._nrows, a._ncols, a.nnz, m.n, m.k = 4, 4, 4, 4, 4, 2
    for call in (lambda: v.upload(np.zeros(4)), v.to_host, lambda: v.fill(1.0), v.padding_dirty, lambda: a.spmv(v, v), a.encoding, a.download,
                 lambda: pc.apply(v, v), m.to_numpy, lambda: K.dot(v, v), lambda: K.CgSolver(1e-8, 5).solve(a, None, v, v)):
        with pytest.raises(K.KError):
            call()


def test_only_a_context_of_one_rank_is_closed_by_the_collector(fake):
    one, two = _context(1, nranks=1), _context(2, nranks=2)
    del one
    gc.collect()
    assert fake.calls == [("kryst_ctx_destroy", 1)]
    del fake.calls[:]
    ref = weakref.ref(two)
    del two
    gc.collect()
    assert ref() is None and fake.calls == []             # dropped, and left alone: a distributed context keeps its explicit close()


def test_context_docstring_says_who_closes_what():
    doc = K.Context.__doc__
    assert "close()" in doc and "DISTRIBUTED" in doc and "sessions, preconditioners, lowered operators, operators, vectors" in doc


@pytest.mark.parametrize("name", sorted(L.KEEPS_OPERATOR))
def test_preconditioners_keep_their_operator_alive(name, fake):
    """setup() stores the operator (`_a`, the pattern of Jacobi): the library borrows it, so it must outlive the preconditioner.  No device: the
    library call of the set-up is answered by FakeLib (the bounds of ChebyshevPoly are given, so nothing is estimated)."""
    ctx = _context(1)

    class Op:                                             # what setup() reads of an operator
        h = K._ffi.Handle(2)
        def nrows(self): return 8
    a = Op()
    a.ctx = ctx
    pc = L.KEEPS_OPERATOR[name]().setup(a)
    assert not any(sym == "kryst_spectrum_estimate" for sym, _ in fake.calls)
    ref = weakref.ref(a)
    del a
    gc.collect()
    assert ref() is not None and pc._a is ref(), name
    ctx.close()
    assert pc.h is None


def test_the_keeps_operator_table_names_every_preconditioner_class():
    classes = {n for n in K.__all__ if isinstance(getattr(K, n), type) and issubclass(getattr(K, n), K._Pc)}
    assert classes == set(L.KEEPS_OPERATOR) | set(L.TAKES_NO_OPERATOR), classes ^ (set(L.KEEPS_OPERATOR) | set(L.TAKES_NO_OPERATOR))
