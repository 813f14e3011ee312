"""The tables of the handle-lifetime tests, shared by the two tiers: tests/test_gpu_lifetimes.py runs them on the device,
tests/test_lifetime_cases_cpu.py holds them against include/kryst_hip.h without one.

  HANDLE_CASES   part 1: every handle kind -- a create, one use, a destroy, and the creates that must fail
  SOLVE_CASES    part 2: every solver class with the exits it can take
  TWO_CONTEXT    part 4: every entry point that takes two or more handles, for the refusal of handles of two contexts
  *_EXEMPT       entry points left out of a table, each with its reason

The figure the memory checks read (device_memory.free_bytes) moves in steps of G bytes: the driver hands small hipMalloc blocks out of 2 MiB
chunks (measured: one-element vectors of 8 KiB moved it at the 252nd, 508th, 764th held vector, by 2 097 152 bytes each time; 32 KiB vectors every
64, 1 MiB vectors every 2).  A case therefore repeats its create / use / destroy R times per round; a block the case would lose once per
repetition shows as soon as R x its size >= G.  `reach(R)` is the smallest such block.  With R <= 64 nothing under 32 KiB can be reached: the
vector cases are sized so that their one allocation is 32 KiB; the blocks of the other kinds that stay below their case's reach are named in the
case's `below` and are NOT covered by these tests."""
import ctypes as C
import functools

import numpy as np

import kryst_amd as K
from kryst_amd import _ffi
from oracle import oracle as O

G = 2 * 1024 * 1024                    # bytes: the step of the free-memory figure (measured, see above)
R_MAX = 64
N = 24                                 # the grid of the memory cases: 24^3 = 13 824 rows
ROWS = N ** 3


def reach(R):
    """the smallest block whose loss once per repetition moves the figure within one round of R repetitions"""
    return -(-G // R)


def repeats(block_bytes):
    """R for a case whose smallest block to cover has block_bytes"""
    return min(R_MAX, -(-G // int(block_bytes)))


def err(fn, code=None):
    """fn must raise KError (with `code`, where one is given); returns it"""
    try:
        fn()
    except K.KError as e:
        assert code is None or e.code == code, (e.code, code, str(e))
        return e
    raise AssertionError("the call was not refused")


def singular_leading_block(a):
    """rows 0 and 1 made [[1, -1], [-1, 1]] on {0, 1}: u_11 = 0 exactly for ILU(0), and every block that holds just these two rows is singular
    (tests/test_gpu_pc_lifetime.py)"""
    v = a.vals.copy()
    for i, j, x in ((0, 0, 1.0), (0, 1, -1.0), (1, 0, -1.0), (1, 1, 1.0)):
        k = a.row_ptr[i] + int(np.nonzero(a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]] == j)[0][0])
        v[k] = x
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


def zero_diagonal_entry(a, row=5):
    """the operator with a stored 0.0 on the diagonal of `row`"""
    v = a.vals.copy()
    v[a.row_ptr[row] + int(np.nonzero(a.col_idx[a.row_ptr[row]:a.row_ptr[row + 1]] == row)[0][0])] = 0.0
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


@functools.lru_cache(maxsize=None)
def box27(n=N):
    """a 27-point operator on an n^3 box (what __graft_entry__.smoke builds): the box forms of the ILU apply"""
    import scipy.sparse as sp
    t = lambda m: sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], [-1, 0, 1])
    m = (sp.identity(n ** 3) * 28.0 - sp.kron(t(n), sp.kron(t(n), t(n)))).tocsr()
    m.sort_indices()
    return O.Csr(m.shape[0], m.shape[0], m.indptr, m.indices, m.data)


def upload(ctx, a):
    return K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)


class Env:
    """What the cases of one context share: the 24^3 operators, their damaged twins and a pair of vectors.  Built once, before anything is
    measured; the cases create and destroy only what they are about."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.ao = O.stencil7(N, "poisson")
        self.n = self.ao.nrows
        self.d = upload(ctx, self.ao)
        self.dgen = K.CsrMatrix.stencil7(N, "poisson", ctx=ctx)            # the generator's operator: CSR-P16
        self.avar = O.stencil7(N, "varcoef")
        self.dvar = upload(ctx, self.avar)                                    # no D16 / P16 form: CSR-DIA
        self.dbad = upload(ctx, singular_leading_block(self.ao))
        self.dzero = upload(ctx, zero_diagonal_entry(self.ao))
        self.dbox = upload(ctx, box27())
        self.small = upload(ctx, O.stencil7(8, "poisson"))                    # 512 rows: what the dense kinds take
        self.r = K.DeviceVec(ctx, np.random.default_rng(3).standard_normal(self.n))
        self.z = K.DeviceVec(ctx, self.n)
        self.b = K.DeviceVec(ctx, self.ao.spmv(np.linspace(0.5, 1.5, self.n)))
        self.r32 = K.DeviceVec32(ctx, np.random.default_rng(4).standard_normal(self.n).astype(np.float32))
        self.z32 = K.DeviceVec32(ctx, self.n)
        self.pair = [[0, 1]] + [list(range(s, min(s + 8, self.n))) for s in range(2, self.n, 8)]
        self.colors = K.color_graph((self.ao.row_ptr, self.ao.col_idx))
        self.inv_rows = [[(i, 1.0 / 6.0)] for i in range(self.n)]
        self.bad_pattern = K.SparsityPattern.Manual([[3, 5, 3]] + [[j] for j in range(1, self.n)])      # an index repeated within a column
        rng = np.random.default_rng(64)
        self.dense64 = rng.standard_normal((64, 64)) + 16.0 * np.eye(64)
        self.b64 = rng.standard_normal(64)


class Case:
    def __init__(self, entries, use, R, fails=(), env=None, below=""):
        self.entries = (entries,) if isinstance(entries, str) else tuple(entries)    # the C entry points that create the handle(s)
        self.use, self.R, self.fails, self.env, self.below = use, int(R), tuple(fails), dict(env or {}), below

    def round(self, E):
        """R times: every failing create, then the create / use / destroy -- the early returns of a failing create are reached as often as
        the destroy of a working one, so reach(R) holds for both"""
        for _ in range(self.R):
            for f in self.fails:
                f(E)
            self.use(E)


# ------------------------------------------------------------------------------------------------ part 1: vectors, operators, dense
def _vec(E):
    v = K.DeviceVec(E.ctx, 3584)                         # (3584 + 512) doubles = 32 KiB
    v.fill(1.0)
    del v


def _mvec(k):
    def use(E):
        m = K.MultiVec(E.ctx, 1536, k)                   # (1536 + 512) * k doubles = 16 KiB * k
        m.to_numpy()
        del m
    return use


def _vec32(E):
    v = K.DeviceVec32(E.ctx, 7168)                       # (7168 + 1024) floats = 32 KiB
    v.to_host()
    del v


def _csr(make):
    def use(E):
        a = make(E)
        a.spmv(E.r, E.z)
        del a
    return use


def _csr_i32(E):
    o = E.ao
    return K.CsrMatrix.from_csr_i32(o.nrows, o.ncols, o.row_ptr, o.col_idx, o.vals, ctx=E.ctx)


def _unsorted(E, how):
    """new_checked's strictly ascending columns, violated in row 7"""
    o = E.ao
    ci = np.array(o.col_idx).copy()
    s = int(o.row_ptr[7])
    ci[s], ci[s + 1] = ci[s + 1], ci[s]
    if how == "u64":
        return K.CsrMatrix.from_csr(o.nrows, o.ncols, o.row_ptr, ci, o.vals, ctx=E.ctx)
    return K.CsrMatrix.from_csr_i32(o.nrows, o.ncols, o.row_ptr, ci, o.vals, ctx=E.ctx)


def _bad_stencil(E):
    h = _ffi.Handle()
    _ffi.check(K.lib().kryst_csr_create_stencil7(E.ctx.h, N, 99, C.byref(h)))


def _transpose(E):
    a = upload(E.ctx, E.ao)
    a.spmv_transpose(E.r, E.z)                           # builds and caches A^T; kryst_csr_destroy frees it
    del a


def _lower(src, form):
    def use(E):
        m = getattr(E, src).lower(form)
        m.spmv(E.r32, E.z32)
        del m
    return use


def _lower_plain_entry(E):
    h = _ffi.Handle()
    _ffi.check(K.lib().kryst_csr32_lower(E.d.h, C.byref(h)))
    _ffi.check(K.lib().kryst_spmv32(h, E.r32.h, E.z32.h))
    _ffi.check(K.lib().kryst_csr32_destroy(h))


def _dense(E):
    a = K.DenseMatrix.from_numpy(E.dense64, ctx=E.ctx)   # 64 x 64 doubles = 32 KiB
    a.matvec(E.b64)
    del a


def _dense_null(E):
    h = _ffi.Handle()
    _ffi.check(K.lib().kryst_dense_create(E.ctx.h, 4, 4, None, 1, C.byref(h)))


def _dense_from_csr(E):
    a = K.DenseMatrix.from_csr(E.small)                  # 512 x 512 doubles = 2 MiB
    a.matvec(np.ones(512))
    del a


def _lu(E):
    a = K.DenseMatrix.from_numpy(E.dense64, ctx=E.ctx)
    lu = K.LuSolver(E.ctx)
    x = np.zeros(64)
    lu.solve(a, None, E.b64, x)
    lu.solve_cached(E.b64)
    lu.factors()
    del lu, a


def _lu_repeated_row(E):
    import dense_cases as DC
    a = K.DenseMatrix.from_numpy(DC.repeated_row(), ctx=E.ctx)
    lu = K.LuSolver(E.ctx)
    err(lambda: lu.solve(a, None, np.ones(a.nrows()), np.zeros(a.nrows())), 5)
    err(lambda: lu.solve_cached(np.ones(a.nrows())), 2)                   # nothing is cached after a failed factorization


def _qr(E):
    a = K.DenseMatrix.from_numpy(E.dense64, ctx=E.ctx)
    K.QrSolver().solve(a, None, E.b64, np.zeros(64))
    del a


def _qr_zero_column(E):
    import dense_cases as DC
    a = K.DenseMatrix.from_numpy(DC.zero_column(), ctx=E.ctx)
    err(lambda: K.QrSolver().solve(a, None, np.ones(a.nrows()), np.zeros(a.nrows())), 5)


# ------------------------------------------------------------------------------------------------ part 1: preconditioners
def _pc(make, src="d", stub=False):
    def use(E):
        pc = make(E).setup(getattr(E, src))
        if stub:
            err(lambda: pc.apply(E.r, E.z), 2)           # the Chebyshev stub's apply is the reference's Err (chebyshev.rs:68-70)
        else:
            pc.apply(E.r, E.z)
        del pc
    return use


def _refused(make, code, src="d"):
    return lambda E: err(lambda: make(E).setup(getattr(E, src)), code)


def _accepted(make, src):
    """a damaged operator that this kind takes all the same (as written it divides where it divides): set up, applied and destroyed like any other"""
    def f(E):
        pc = make(E).setup(getattr(E, src))
        pc.apply(E.r, E.z)
        del pc
    return f


T = K.MatSorType
_ROWS4 = 4 * ROWS                      # an int32 per row: the smallest per-row array of most kinds, 55 296 bytes
R_ROWS = repeats(_ROWS4)               # 38: reach 55 189 bytes, every per-row array (int32: 55 296, double: 110 592 and more) is covered
R_SLOW = 16                            # kinds whose set-up is made on the host or from Python lists: reach 131 072 bytes
_WORDS = "error / counter / ticket words (4 .. 64 bytes)"
_SLOW = _WORDS + "; at R = 16 also every per-row int32 array (55 KiB) and per-row double array (108 KiB)"
# The stored zero diagonal of row 5 (dzero) is a zero pivot for Ilup(0) alone (KRYST_SOLVE_ERROR, ilup.rs:108-110; tests/cpp/test_host_san.cpp);
# Ilu0, Ilup(1), Ilup(2) and Ilut as written take that operator.  The singular leading block (dbad) is the zero pivot of textbook ILU(0).
PC_KINDS = {
    # name: (entry points, constructor, operator, failing set-ups, R, environment, blocks below the reach)
    "identity": ("kryst_pc_identity", lambda E: K.IdentityPc(), "d", (), 1, {}, "(no device memory)"),
    "chebyshev_stub": ("kryst_pc_chebyshev_stub", lambda E: K.Chebyshev(3), "d", (), 1, {}, "(no device memory)"),
    "jacobi": ("kryst_pc_jacobi", lambda E: K.Jacobi(), "d", (), repeats(8 * ROWS), {}, ""),
    "chebyshev_filter": ("kryst_pc_chebyshev", lambda E: K.ChebyshevPc(3, 0.5, 12.0), "d", (), repeats(8 * ROWS), {}, ""),
    "ilu0_as_written": ("kryst_pc_ilu0", lambda E: K.Ilu0(), "d", (_accepted(lambda E: K.Ilu0(), "dzero"),), R_ROWS, {}, _WORDS),
    "ilup0": ("kryst_pc_ilup", lambda E: K.Ilup(0), "d", (_refused(lambda E: K.Ilup(0), 2, "dzero"),), R_ROWS, {}, _WORDS),
    "ilup1": ("kryst_pc_ilup", lambda E: K.Ilup(1), "d", (_accepted(lambda E: K.Ilup(1), "dzero"),), R_ROWS, {}, _WORDS),
    "ilup2": ("kryst_pc_ilup", lambda E: K.Ilup(2), "d", (_accepted(lambda E: K.Ilup(2), "dzero"),), R_ROWS, {}, _WORDS),
    "ilut": ("kryst_pc_ilut", lambda E: K.Ilut(10, 1e-3), "d", (_accepted(lambda E: K.Ilut(10, 1e-3), "dzero"),), R_ROWS, {}, _WORDS),
    "ilu_grid_device_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "d", (_refused(lambda E: K.TrueIlu0(), 5, "dbad"),), R_ROWS, {}, _WORDS),
    "ilu_grid_host_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "d", (_refused(lambda E: K.TrueIlu0(), 5, "dbad"),), R_ROWS,
                            {"KRYST_ILU_DEVICE_SETUP": "0"}, _WORDS),
    "ilu_levels_device_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "d", (_refused(lambda E: K.TrueIlu0(), 5, "dbad"),), R_ROWS,
                                {"KRYST_ILU_GRID": "0"}, _WORDS + "; per-level tables"),
    "ilu_levels_host_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "d", (_refused(lambda E: K.TrueIlu0(), 5, "dbad"),), R_ROWS,
                              {"KRYST_ILU_GRID": "0", "KRYST_ILU_DEVICE_SETUP": "0"}, _WORDS + "; per-level tables"),
    "ilu_box_device_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "dbox", (), R_ROWS, {}, _WORDS),
    "ilu_box_host_setup": ("kryst_pc_ilu0", lambda E: K.TrueIlu0(), "dbox", (), R_ROWS, {"KRYST_ILU_DEVICE_SETUP": "0"}, _WORDS),
    "chebyshev_poly_estimated": ("kryst_pc_chebyshev_poly", lambda E: K.ChebyshevPoly(3), "d",
                                 (_refused(lambda E: K.ChebyshevPoly(3, 2.0, 1.0), 102), _refused(lambda E: K.ChebyshevPoly(65, 0.1, 2.0), 102)),
                                 repeats(8 * ROWS), {}, ""),
    "approx_inverse_given_rows": ("kryst_pc_approx_inverse", None, "d", (), R_SLOW, {}, "M's dictionaries (1 .. 2 KiB), its row pointers and pattern ids; "
                                  "M is built from Python lists: R = 16"),
    "block_jacobi_sets": ("kryst_pc_block_jacobi", lambda E: K.BlockJacobi(E.pair), "d", (_refused(lambda E: K.BlockJacobi(E.pair), 5, "dbad"),), R_SLOW, {},
                          _SLOW + " (the index streams are packed from Python lists)"),
    "block_jacobi_uniform": ("kryst_pc_block_jacobi_uniform", lambda E: K.BlockJacobi.uniform(8), "d",
                             (_refused(lambda E: K.BlockJacobi.uniform(2), 5, "dbad"), _refused(lambda E: K.BlockJacobi.uniform(65), 6)),      # (block 0 = rows {0, 1})
                             R_ROWS, {}, _WORDS),
    "asm_sets": ("kryst_pc_asm", lambda E: K.AdditiveSchwarz(0, E.pair), "d", (_refused(lambda E: K.AdditiveSchwarz(0, E.pair), 5, "dbad"),), R_SLOW, {},
                 _SLOW + " (the index streams are packed from Python lists)"),
    "asm_overlap": ("kryst_pc_asm", lambda E: K.AdditiveSchwarz(1, K.AdditiveSchwarz.grid_boxes(N)).with_overlap(), "d",
                    (_refused(lambda E: K.AdditiveSchwarz(-1, K.AdditiveSchwarz.grid_boxes(N)).with_overlap(), 102),), R_SLOW, {}, _SLOW + " (the growth runs on the host)"),
    "asm_uniform": ("kryst_pc_asm_uniform", lambda E: K.AdditiveSchwarz(0, None, ROWS // 64), "d",
                    (_refused(lambda E: K.AdditiveSchwarz(0, None, 2), 6),), R_ROWS, {}, _WORDS),
    "asm_ilu_sets": ("kryst_pc_asm_ilu", lambda E: K.AdditiveSchwarz(0, K.AdditiveSchwarz.grid_boxes(N, (8, 8, 8))).with_sub_ilu("ilu0"), "d",
                     (_refused(lambda E: K.AdditiveSchwarz(0, K.AdditiveSchwarz.grid_boxes(N, (8, 8, 8))).with_sub_ilu(0), 6),), R_SLOW, {}, _SLOW),
    "asm_ilu_uniform": ("kryst_pc_asm_ilu_uniform", lambda E: K.AdditiveSchwarz(0, None, 8).with_sub_ilu("ilup0"), "d",
                        (_refused(lambda E: K.AdditiveSchwarz(0, None, 8).with_sub_ilu("ilu0"), 5, "dbad"),), R_SLOW, {}, _SLOW),
    "sor": ("kryst_pc_sor", lambda E: K.Sor(1.5, 2, 1, T.SYMMETRIC_SWEEP, 0.0), "d",
            (_refused(lambda E: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, -6.0), 5),), R_ROWS, {}, _WORDS + " (d_sync, 16 bytes)"),
    "sor_coloured": ("kryst_pc_sor", lambda E: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0).with_colors(E.colors), "d",
                     (_refused(lambda E: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, -6.0).with_colors(E.colors), 5),), R_ROWS, {}, _WORDS),
    "spai": ("kryst_pc_spai", lambda E: K.Spai(K.SparsityPattern.Operator, 1e-9), "d",
             (_refused(lambda E: K.Spai(E.bad_pattern, 1e-9), 102), _refused(lambda E: K.Spai(K.SparsityPattern.Auto, 1e-9), 6)),
             R_SLOW, {}, _SLOW + " (a QR per column)"),
    "amg_as_written": ("kryst_pc_amg", lambda E: K.Amg(10, 0.1), "d", (_refused(lambda E: K.Amg(-1, 0.1), 102),), R_SLOW, {},
                       _SLOW + "; every array of the coarse levels (the hierarchy is made on the host)"),
    "amg_smoothed": ("kryst_pc_amg", lambda E: K.Amg(10).with_textbook(0.0), "d", (_refused(lambda E: K.Amg(10).with_textbook(0.0), 5, "dzero"),), R_SLOW, {},
                     _SLOW + "; every array of the coarse levels"),
}


def _approx_inverse(E):
    pc = K.ApproxInv(E.inv_rows, ctx=E.ctx).setup(E.d)
    pc.apply(E.r, E.z)
    del pc


_D = {"KRYST_SPMV_DIA": "1"}
_CSR_BELOW = "the dictionaries (1 .. 2 KiB), the row-pattern ids (28 KiB) and tables, the tile flags, scratch words"
HANDLE_CASES = {
    "vec": Case("kryst_vec_create", _vec, 64, fails=(lambda E: err(lambda: K.DeviceVec(E.ctx, -1), 102),)),
    "mvec2": Case("kryst_mvec_create", _mvec(2), 64, fails=(lambda E: err(lambda: K.MultiVec(E.ctx, 8, 3), 102),)),
    "mvec4": Case("kryst_mvec_create", _mvec(4), 32),
    "mvec8": Case("kryst_mvec_create", _mvec(8), 16),
    "vec32": Case("kryst_vec32_create", _vec32, 64, fails=(lambda E: err(lambda: K.DeviceVec32(E.ctx, -1), 102),)),
    "csr_from_csr": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.ao)), repeats(_ROWS4), fails=(lambda E: err(lambda: _unsorted(E, "u64"), 103),),
                         below=_CSR_BELOW),
    "csr_create_i32": Case("kryst_csr_create_i32", _csr(_csr_i32), repeats(_ROWS4), fails=(lambda E: err(lambda: _unsorted(E, "i32"), 103),), below=_CSR_BELOW),
    "csr_stencil7": Case("kryst_csr_create_stencil7", _csr(lambda E: K.CsrMatrix.stencil7(N, "poisson", ctx=E.ctx)), repeats(_ROWS4),
                         fails=(lambda E: err(lambda: _bad_stencil(E)),), below=_CSR_BELOW),
    "csr_compress0": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.ao)), repeats(_ROWS4), env={"KRYST_SPMV_COMPRESS": "0"}, below=_CSR_BELOW),
    "csr_compress1": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.ao)), repeats(_ROWS4), env={"KRYST_SPMV_COMPRESS": "1"}, below=_CSR_BELOW),
    "csr_compress2": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.ao)), repeats(_ROWS4), env={"KRYST_SPMV_COMPRESS": "2"}, below=_CSR_BELOW),
    "csr_compress3": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.ao)), repeats(_ROWS4), env={"KRYST_SPMV_COMPRESS": "3"}, below=_CSR_BELOW),
    "csr_dia": Case("kryst_csr_create", _csr(lambda E: upload(E.ctx, E.avar)), repeats(_ROWS4), env=_D, below=_CSR_BELOW),
    "csr_transpose": Case("kryst_csr_create", _transpose, repeats(_ROWS4), below=_CSR_BELOW + "; the transposition's block sums"),
    "csr32_plain": Case("kryst_csr32_lower_form", _lower("d", "plain"), repeats(_ROWS4), below="the counters (16 bytes)"),
    "csr32_plain_entry": Case("kryst_csr32_lower", _lower_plain_entry, repeats(_ROWS4), below="the counters (16 bytes)"),
    "csr32_pattern": Case("kryst_csr32_lower_form", _lower("dgen", "pattern"), repeats(_ROWS4),
                          fails=(lambda E: err(lambda: E.dvar.lower("pattern"), 6),), below="the pattern ids (28 KiB) and tables, the counters"),
    "csr32_auto": Case("kryst_csr32_lower_form", _lower("dgen", "auto"), repeats(_ROWS4), below="the pattern ids (28 KiB) and tables, the counters"),
    "csr32_dia": Case("kryst_csr32_lower_form", _lower("dvar", "dia"), repeats(_ROWS4), fails=(lambda E: err(lambda: E.dgen.lower("dia"), 6),),
                      below="the counters (16 bytes)"),
    "dense_create": Case("kryst_dense_create", _dense, 64, fails=(lambda E: err(lambda: _dense_null(E), 102),)),
    "dense_from_csr": Case("kryst_dense_from_csr", _dense_from_csr, 1),          # (no refusing arguments on one rank)
    "lu": Case("kryst_lu_create", _lu, 64, fails=(_lu_repeated_row,), below="the permutations (256 bytes each) and the pivot search's scratch"),
    "qr": Case((), _qr, 64, fails=(_qr_zero_column,), below="the reflectors' scalars"),
}
for _name, (_entries, _make, _src, _fails, _R, _env, _below) in PC_KINDS.items():
    _use = _approx_inverse if _make is None else _pc(_make, _src, stub=(_name == "chebyshev_stub"))
    HANDLE_CASES["pc_" + _name] = Case(_entries, _use, _R, fails=_fails, env=_env, below=_below)

# functions of include/kryst_hip.h with a kryst_*_t* output parameter that HANDLE_CASES does not create, and why
CREATE_EXEMPT = {
    "kryst_ctx_create": "the context itself: tests/test_gpu_lifetimes.py, part 3 (dropped and closed contexts)",
    "kryst_ctx_create_dist": "distributed only: a context of several ranks keeps its explicit close() (tests/test_gpu_z_multirank_shim.py)",
    "kryst_csr_create_dist": "distributed only (tests/test_gpu_z_multirank_shim.py, tests/test_gpu_y_dist_single.py)",
    "kryst_session_begin": "part 2: SOLVE_CASES['session']",
    "kryst_host_ilup": "host only: no device memory (tests/test_host_factor_cpu.py)",
    "kryst_host_ilut": "host only: no device memory (tests/test_host_factor_cpu.py)",
    "kryst_host_amg": "host only: no device memory (tests/test_amg_cpu.py)",
}

# which preconditioner classes keep their operator alive (the `_a` attribute), and the two that take nothing but the context
KEEPS_OPERATOR = {
    "Jacobi": lambda: K.Jacobi(), "Ilu0": lambda: K.Ilu0(), "Ilup": lambda: K.Ilup(1), "Ilut": lambda: K.Ilut(10, 1e-3), "TrueIlu0": lambda: K.TrueIlu0(),
    "ChebyshevPc": lambda: K.ChebyshevPc(3, 0.5, 12.0), "ChebyshevPoly": lambda: K.ChebyshevPoly(3, 0.1, 2.0), "BlockJacobi": lambda: K.BlockJacobi.uniform(8),
    "AdditiveSchwarz": lambda: K.AdditiveSchwarz(0, None, 8), "Sor": lambda: K.Sor(1.0, 1, 1, T.SYMMETRIC_SWEEP, 0.0),
    "Spai": lambda: K.Spai(K.SparsityPattern.Operator, 1e-9), "Amg": lambda: K.Amg(4, 0.1),
}
TAKES_NO_OPERATOR = {"IdentityPc": "kryst_pc_identity takes the context alone", "Chebyshev": "the stub takes the context alone",
                     "ApproxInv": "owns its matrix M (self.m); the operator is only compared in size"}


# ------------------------------------------------------------------------------------------------ part 2: solvers and their exits
P = K.Preconditioning
SOLVERS = {
    # name: (a fresh solver for (tol, max_iters), the preconditioner it is given: None | "jacobi")
    "cg": (lambda t, m: K.CgSolver(t, m), None),
    "pcg": (lambda t, m: K.PcgSolver(t, m), "jacobi"),
    "gmres_none": (lambda t, m: K.GmresSolver(5, t, m).with_preconditioning(P.NoPc), None),
    "gmres_left": (lambda t, m: K.GmresSolver(5, t, m).with_preconditioning(P.Left), "jacobi"),
    "gmres_right": (lambda t, m: K.GmresSolver(5, t, m).with_preconditioning(P.Right), "jacobi"),
    "gmres_left_textbook": (lambda t, m: K.GmresSolver(5, t, m).with_preconditioning(P.LeftTextbook), "jacobi"),
    "bicgstab": (lambda t, m: K.BiCgStabSolver(t, m), None),
    "bicgstab_rpc": (lambda t, m: K.BiCgStabRightPcSolver(t, m), "jacobi"),
    "cgs": (lambda t, m: K.CgsSolver(t, m), None),
    "tfqmr": (lambda t, m: K.TfqmrSolver(t, m), None),
    "minres": (lambda t, m: K.MinresSolver(t, m), None),
    "minres_textbook": (lambda t, m: K.MinresSolver(t, m).with_textbook(), None),
    "cgnr": (lambda t, m: K.CgnrSolver(t, m), None),
    "cgnr_textbook": (lambda t, m: K.CgnrSolver(t, m).with_textbook(), None),
    "qmr": (lambda t, m: K.QmrSolver(t, m), None),
    "fgmres": (lambda t, m: K.FgmresSolver(t, m, 5), "jacobi"),
    "pca_gmres": (lambda t, m: K.PcaGmresSolver(5, 1, 1, t, m).with_preconditioning(P.Right), "jacobi"),
    "pca_gmres_sstep": (lambda t, m: K.PcaGmresSolver(6, 1, 3, t, m).with_preconditioning(P.Right).with_textbook(), "jacobi"),
    "cb_gmres": (lambda t, m: K.CbGmresSolver(5, t, m).with_preconditioning(P.Right), "jacobi"),
}
# the solvers that meet 1e-8 on the 24^3 Poisson operator within 400 iterations (the others run to the cap: restart 5, the as-written forms)
CONVERGE = ("cg", "pcg", "cgs", "minres", "minres_textbook", "pca_gmres_sstep")
COMMON_EXITS = ("converged", "cap", "max_iters_zero", "zero_rhs", "wrong_length")
# the exits a solver can take beside COMMON_EXITS (built from fixtures the suite has: multirank_ext_cases.C_INDEFINITE, the rotation of
# tests/test_oracle_independent.py and tests/test_gpu_cgs_tfqmr.py)
OWN_EXITS = {"cg": ("indefinite",), "pcg": ("indefinite", "ilu_give_up"), "bicgstab": ("rotation",), "tfqmr": ("rotation",),
             "gmres_right": ("ilu_give_up",)}
SOLVE_R = repeats(8 * (ROWS + 512))    # 19 repetitions of every exit per round: reach 110 377 bytes, one work vector of a solve at 24^3 (114 688
                                       # bytes) whether it comes from the arena or on its own; the per-solve blocks below it (the restarted
                                       # solvers' small arena of H, g, rotations and pointer tables; the state words) are not covered
OTHER_SOLVE_CASES = ("multi_cg", "multi_pcg", "block_cg", "cg32", "pcg32", "refinement", "session", "session_busy", "session_dropped")
SOLVE_CASES = tuple(SOLVERS) + OTHER_SOLVE_CASES


# ------------------------------------------------------------------------------------------------ part 4: handles of two contexts
# kinds of arguments: csr, pc, vec, mvec, vec32, csr32, dense, lu; a trailing "*" marks an operand the call writes
def _solve_dev(make):
    return lambda b, x, a, pc: make().solve(a, pc, b, x)


def _solve_host(make):
    def call(a, pc):
        x = np.full(a.nrows(), -99.0)
        try:
            return make().solve(a, pc, np.ones(a.nrows()), x)
        except K.KError:
            assert np.all(x == -99.0), "a refused host solve wrote x"
            raise
    return call


def _session(b, x, a, pc):
    K.Session("pcg", a, pc, b, x, 1e-8, 5).close()


def _multi(sym):
    def call(b, x, a, pc):
        prm = _ffi.Params(1e-8, 5, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
        _ffi.check(getattr(K.lib(), sym)(b.h, x.h, a.h, pc.h, C.byref(prm), None, None, None, 0, None))
    return call


def _multi_host(sym):
    def call(a, pc):
        n = a.nrows()
        prm = _ffi.Params(1e-8, 5, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
        b, x = np.asfortranarray(np.ones((n, 2))), np.asfortranarray(np.full((n, 2), -99.0))
        try:
            _ffi.check(getattr(K.lib(), sym)(b.ctypes.data_as(_ffi.c_dp), x.ctypes.data_as(_ffi.c_dp), n, 2, n, a.h, pc.h, C.byref(prm), None, None, None, 0, None))
        except K.KError:
            assert np.all(x == -99.0), "a refused host solve wrote X"
            raise
    return call


def _solve32(sym):
    def call(b, x, a, pc):
        prm = _ffi.Params(1e-6, 5, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0)
        st, hist, hlen = _ffi.Stats(), np.zeros(16), C.c_int64(0)
        _ffi.check(getattr(K.lib(), sym)(b.h, x.h, a.h, pc.h, C.byref(prm), C.byref(st), hist.ctypes.data_as(_ffi.c_dp), 16, C.byref(hlen)))
    return call


def _refine(b, x, a, a32, pc):
    po = _ffi.Params(1e-10, 2, 0, 0, 1, 0, 0, 0.0, 0, 0.0, 0)
    pi = _ffi.Params(1e-6, 5, 0, 0, 1, 0, 0, 0.0, 0, 0.0, 0)
    _ffi.check(K.lib().kryst_refine_solve_dev(b.h, x.h, a.h, a32.h, pc.h, C.byref(po), C.byref(pi), None, None, 0, None, None, 0))


def _direct_host(fn_name, with_lu):
    def call(*hs):
        a = hs[1] if with_lu else hs[0]
        n = a.nrows()
        x = np.full(n, -99.0)
        st = _ffi.Stats()
        b = np.ones(n)
        try:
            _ffi.check(getattr(K.lib(), fn_name)(*[h.h for h in hs], b.ctypes.data_as(_ffi.c_dp), x.ctypes.data_as(_ffi.c_dp), n, C.byref(st)))
        except K.KError:
            assert np.all(x == -99.0), "a refused host solve wrote x"
            raise
    return call


def _direct_dev(fn_name):
    def call(*hs):
        st = _ffi.Stats()
        _ffi.check(getattr(K.lib(), fn_name)(*[h.h for h in hs], C.byref(st)))
    return call


_S = {name: (lambda mk=mk: mk(1e-8, 5)) for name, (mk, _) in SOLVERS.items()}
_DEV = ("vec", "vec*", "csr", "pc")
TWO_CONTEXT = {
    # C entry point: (argument kinds in the order of the call below, the call)
    "kryst_vec_copy": (("vec*", "vec"), lambda y, x: y.copy_from(x)),
    "kryst_spmv": (("csr", "vec", "vec*"), lambda a, x, y: a.spmv(x, y)),
    "kryst_spmv_transpose": (("csr", "vec", "vec*"), lambda a, x, y: a.spmv_transpose(x, y)),
    "kryst_dot": (("vec", "vec"), lambda x, y: K.dot(x, y)),
    "kryst_axpy": (("vec", "vec*"), lambda x, y: K.axpy(0.5, x, y)),
    "kryst_aypx": (("vec", "vec*"), lambda x, y: K.aypx(0.5, x, y)),
    "kryst_sub": (("vec", "vec", "vec*"), lambda a, b, out: K.sub(a, b, out)),
    "kryst_pc_apply": (("pc", "vec", "vec*"), lambda pc, r, z: pc.apply(r, z)),
    "kryst_apply_chebyshev": (("csr", "vec", "vec*"), lambda a, r, z: K.apply_chebyshev(a, r, z, 0.5, 12.0, 3)),
    "kryst_cg_solve_dev": (_DEV, _solve_dev(_S["cg"])),
    "kryst_pcg_solve_dev": (_DEV, _solve_dev(_S["pcg"])),
    "kryst_gmres_solve_dev": (_DEV, _solve_dev(_S["gmres_right"])),
    "kryst_bicgstab_solve_dev": (_DEV, _solve_dev(_S["bicgstab"])),
    "kryst_bicgstab_rpc_solve_dev": (_DEV, _solve_dev(_S["bicgstab_rpc"])),
    "kryst_cgs_solve_dev": (_DEV, _solve_dev(_S["cgs"])),
    "kryst_tfqmr_solve_dev": (_DEV, _solve_dev(_S["tfqmr"])),
    "kryst_minres_solve_dev": (_DEV, _solve_dev(_S["minres"])),
    "kryst_qmr_solve_dev": (_DEV, _solve_dev(_S["qmr"])),
    "kryst_cgnr_solve_dev": (_DEV, _solve_dev(_S["cgnr"])),
    "kryst_minres_textbook_solve_dev": (_DEV, _solve_dev(_S["minres_textbook"])),
    "kryst_cgnr_textbook_solve_dev": (_DEV, _solve_dev(_S["cgnr_textbook"])),
    "kryst_fgmres_solve_dev": (_DEV, _solve_dev(_S["fgmres"])),
    "kryst_pca_gmres_solve_dev": (_DEV, _solve_dev(_S["pca_gmres"])),
    "kryst_pca_gmres_textbook_solve_dev": (_DEV, _solve_dev(_S["pca_gmres_sstep"])),
    "kryst_cbgmres_solve_dev": (_DEV, _solve_dev(_S["cb_gmres"])),
    "kryst_cg_solve": (("csr", "pc"), _solve_host(_S["cg"])),
    "kryst_pcg_solve": (("csr", "pc"), _solve_host(_S["pcg"])),
    "kryst_gmres_solve": (("csr", "pc"), _solve_host(_S["gmres_none"])),            # a preconditioner GMRES would not even apply
    "kryst_bicgstab_solve": (("csr", "pc"), _solve_host(_S["bicgstab"])),
    "kryst_cgs_solve": (("csr", "pc"), _solve_host(_S["cgs"])),
    "kryst_tfqmr_solve": (("csr", "pc"), _solve_host(_S["tfqmr"])),
    "kryst_minres_solve": (("csr", "pc"), _solve_host(_S["minres"])),
    "kryst_qmr_solve": (("csr", "pc"), _solve_host(_S["qmr"])),
    "kryst_cgnr_solve": (("csr", "pc"), _solve_host(_S["cgnr"])),
    "kryst_fgmres_solve": (("csr", "pc"), _solve_host(_S["fgmres"])),
    "kryst_pca_gmres_solve": (("csr", "pc"), _solve_host(lambda: K.PcaGmresSolver(5, 1, 1, 1e-8, 5))),      # Left: the preconditioner is never called
    "kryst_session_begin": (_DEV, _session),
    "kryst_dense_matvec": (("dense", "vec", "vec*"), lambda a, x, y: a.matvec(x, y)),
    "kryst_lu_solve_dev": (("lu", "dense", "pc", "vec", "vec*"), _direct_dev("kryst_lu_solve_dev")),
    "kryst_lu_solve": (("lu", "dense", "pc"), _direct_host("kryst_lu_solve", True)),
    "kryst_lu_solve_cached": (("lu", "vec", "vec*"), lambda lu, b, x: lu.solve_cached(b, x)),
    "kryst_qr_solve_dev": (("dense", "pc", "vec", "vec*"), _direct_dev("kryst_qr_solve_dev")),
    "kryst_qr_solve": (("dense", "pc"), _direct_host("kryst_qr_solve", False)),
    "kryst_mvec_set_column": (("mvec*", "vec"), lambda m, v: m.set_column(1, v)),
    "kryst_mvec_get_column": (("mvec", "vec*"), lambda m, v: _ffi.check(K.lib().kryst_mvec_get_column(m.h, 1, v.h))),
    "kryst_spmm": (("csr", "mvec", "mvec*"), lambda a, x, y: a.spmm(x, y)),
    "kryst_cg_solve_multi_dev": (("mvec", "mvec*", "csr", "pc"), _multi("kryst_cg_solve_multi_dev")),
    "kryst_pcg_solve_multi_dev": (("mvec", "mvec*", "csr", "pc"), _multi("kryst_pcg_solve_multi_dev")),
    "kryst_bcg_solve_multi_dev": (("mvec", "mvec*", "csr", "pc"), _multi("kryst_bcg_solve_multi_dev")),
    "kryst_cg_solve_multi": (("csr", "pc"), _multi_host("kryst_cg_solve_multi")),
    "kryst_pcg_solve_multi": (("csr", "pc"), _multi_host("kryst_pcg_solve_multi")),
    "kryst_bcg_solve_multi": (("csr", "pc"), _multi_host("kryst_bcg_solve_multi")),
    "kryst_vec32_from_f64": (("vec32*", "vec"), lambda d, s: K.DeviceVec32.from_f64(s, d)),
    "kryst_vec32_to_f64": (("vec*", "vec32"), lambda d, s: s.to_f64(d)),
    "kryst_dot32": (("vec32", "vec32"), lambda x, y: K.dot32(x, y)),
    "kryst_spmv32": (("csr32", "vec32", "vec32*"), lambda a, x, y: a.spmv(x, y)),
    "kryst_cg32_solve_dev": (("vec32", "vec32*", "csr32", "pc"), _solve32("kryst_cg32_solve_dev")),
    "kryst_pcg32_solve_dev": (("vec32", "vec32*", "csr32", "pc"), _solve32("kryst_pcg32_solve_dev")),
    "kryst_refine_solve_dev": (("vec", "vec*", "csr", "csr32", "pc"), _refine),
}
TWO_CONTEXT_EXEMPT = {
    "kryst_bench_spmv": "measurement hook (bench.py); it makes the check of kryst_spmv",
    "kryst_bench_csr_skeleton": "measurement hook (bench.py); it makes the check of kryst_spmv",
    "kryst_bench_spmv_fused": "measurement hook (bench.py)",
    "kryst_bench_pc_apply": "measurement hook (bench.py); it makes the check of kryst_pc_apply",
    "kryst_bench_mvec_gram": "test hook of block CG (tests/test_gpu_block_cg.py)",
}

HANDLE_TYPES = ("kryst_ctx_t", "kryst_csr_t", "kryst_vec_t", "kryst_pc_t", "kryst_session_t", "kryst_dense_t", "kryst_lu_t", "kryst_mvec_t",
                "kryst_vec32_t", "kryst_csr32_t", "kryst_host_factors_t", "kryst_host_amg_t")


def header_functions(text):
    """[(name, [parameter type, ...])] of every function include/kryst_hip.h declares, KRYST_SOLVE_ARGS expanded; a parameter type is the
    declaration without its name ("kryst_vec_t", "kryst_pc_t*", "const double*", ...)"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"#define KRYST_SOLVE_ARGS(.*?)\n\n", text.replace("\\\n", " "), flags=re.S)
    text = text.replace("\\\n", " ")
    solve_args = m.group(1).strip()
    text = text.replace(m.group(0), "\n\n").replace("KRYST_SOLVE_ARGS", solve_args)
    out = []
    for ret, name, params in re.findall(r"\b(int32_t|int64_t|void|const char\*)\s+(kryst_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if not p or p == "void":
                continue
            p = re.sub(r"\[\w*\]$", "*", p)                                       # int64_t info[3] -> pointer
            mm = re.match(r"(.*?[\s\*])(\w+)\s*(\*?)$", p)
            types.append(((mm.group(1).strip() + mm.group(3)) if mm else p).replace(" *", "*"))
        out.append((name, types))
    return out


def creators(funcs):
    """the functions with a kryst_*_t* output parameter"""
    import re
    return sorted(n for n, ts in funcs if any(re.fullmatch(r"kryst_\w+_t\*", t) and t[:-1] in HANDLE_TYPES for t in ts))


def multi_handle(funcs):
    """the functions with two or more handle-typed parameters"""
    return sorted(n for n, ts in funcs if sum(t in HANDLE_TYPES for t in ts) >= 2)
