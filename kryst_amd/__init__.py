"""kryst_amd -- host-side mirror of kryst's operator / preconditioner / solver interface for the MI355X path.

The classes keep the reference's names, constructor arguments, builder methods, public fields and error
behaviour (paths relative to the kryst crate):

    CsrMatrix.from_csr(nrows, ncols, row_ptr, col_idx, values)      src/matrix/sparse.rs:28-46
    CsrMatrix.spmv(x, y) / matvec(x, y)                             src/matrix/sparse.rs:56-67, core/traits.rs:4-7
    dot(x, y), norm(x)                                              src/core/wrappers.rs:90-127
    Jacobi / Ilu0 / Ilup / Chebyshev  .setup(a) .apply(r, z)        src/preconditioner/*.rs
    ChebyshevPoly(degree, ...), estimate_spectrum(a)                Chebyshev polynomial preconditioner with estimated bounds (extension)
    apply_chebyshev(a, r, z, alpha, beta, m)                        src/preconditioner/chebyshev.rs:83-140
    CgSolver / PcgSolver / GmresSolver / BiCgStabSolver .solve(a, pc, b, x) -> SolveStats   src/solver/*.rs
    MultiVec, CsrMatrix.spmm(X, Y), CgSolver / PcgSolver .solve_many(a, pc, B, X)           several right-hand sides at once (extension)
    DeviceVec32, CsrMatrix.lower() -> CsrMatrix32, Cg32Solver / Pcg32Solver, RefinementSolver   fp32 storage + fp64 refinement (extension)
    DenseMatrix.from_raw(nrows, ncols, data) .matvec(x, y)          src/matrix/dense.rs:16-25, core/wrappers.rs:27-38
    LuSolver / QrSolver .solve(a, pc, b, x), LuSolver.solve_cached  src/solver/direct_lu.rs
    Convergence, SolveStats, KError, CgNormType, Preconditioning    src/utils/convergence.rs, src/error.rs

Everything executes in libkryst_hip.so (hand-written HIP for gfx950) through the C ABI of include/kryst_hip.h.
There is no CPU fallback and no torch dependency.
"""
import ctypes as C
import enum
import weakref
import numpy as np

from . import _ffi
from ._ffi import KError, lib, check

__all__ = ["Context", "DeviceVec", "CsrMatrix", "dot", "norm", "Jacobi", "Ilu0", "Ilup", "Ilut", "TrueIlu0", "Chebyshev",
           "ChebyshevPc", "ChebyshevPoly", "estimate_spectrum", "host_tridiag_extreme_eigs", "IdentityPc", "ApproxInv", "BlockJacobi", "AdditiveSchwarz", "Sor", "MatSorType", "SparsityPattern", "Spai", "Amg", "apply_chebyshev", "Convergence", "SolveStats", "CgNormType",
           "Preconditioning", "CgSolver", "PcgSolver", "GmresSolver", "FgmresSolver", "PcaGmresSolver", "CbGmresSolver", "Orthog", "CgsSolver", "TfqmrSolver", "MinresSolver", "QmrSolver", "CgnrSolver", "CgneSolver", "BiCgStabSolver", "BiCgStabRightPcSolver", "Session", "KspContext", "SolverKind", "PC", "KError", "reduce_spec",
           "host_stencil7", "partition_rows", "halo_recv_plan", "read_matrix_market", "read_petsc_binary", "host_ilup", "host_ilut", "host_amg", "host_levels", "color_graph", "build_blocks_from_colors",
           "DenseMatrix", "LuSolver", "QrSolver", "host_dense_lu", "host_dense_lu_solve", "host_dense_qr_solve",
           "MultiVec", "split_widths", "BlockCgSolver", "mvec_gram", "host_bcg_step",
           "DeviceVec32", "CsrMatrix32", "dot32", "Cg32Solver", "Pcg32Solver", "RefinementSolver", "reduce_spec32", "host_round_f32"]


def _dp(a):
    return a.ctypes.data_as(_ffi.c_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def reduce_spec():
    """(T, V, F) of the library's fixed inner-product tree (kryst_reduce_spec)."""
    t, v, f = C.c_int32(), C.c_int32(), C.c_int32()
    lib().kryst_reduce_spec(C.byref(t), C.byref(v), C.byref(f))
    return t.value, v.value, f.value


class Context:
    """One GPU (one rank).  Replaces the Comm objects of src/parallel (RayonComm / MpiComm).

    Lifetime: a context of ONE rank is destroyed when it is dropped (`__del__` calls `close()`); every handle made on it keeps it alive, so
    that happens after its last vector, operator and preconditioner has gone.  `close()` may also be called while such objects are alive: it
    destroys them first -- sessions, preconditioners, lowered operators, operators, vectors, in this order -- and leaves each with `h = None`
    (its methods then raise KError).  A DISTRIBUTED context (nranks > 1) is never destroyed by the garbage collector: tearing it down tears
    down its communicator, which every rank has to do at a point of its own choosing, so it keeps the explicit `close()`."""

    _default = None

    def __init__(self, device=0, rank=0, nranks=1, unique_id=None):
        self._children = {}                          # id -> weak reference of every live object that holds a handle of this context
        self.h = _ffi.Handle()
        if nranks == 1 and unique_id is None:
            check(lib().kryst_ctx_create(device, C.byref(self.h)))
        else:
            buf = C.create_string_buffer(bytes(unique_id), 128)
            check(lib().kryst_ctx_create_dist(device, rank, nranks, buf, C.byref(self.h)))
        self.rank, self.nranks, self.device = rank, nranks, device

    @staticmethod
    def default():
        if Context._default is None:
            Context._default = Context(0)
        return Context._default

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().kryst_comm_unique_id(buf))
        return buf.raw

    def size(self):
        return self.nranks

    def barrier(self):
        check(lib().kryst_comm_barrier(self.h))

    def all_reduce(self, x):
        out = C.c_double()
        check(lib().kryst_comm_all_reduce(self.h, float(x), C.byref(out)))
        return out.value

    def scalar_reduce(self, mode):
        """'rccl' | 'ipc' | 'query': how the solvers' inner products cross the ranks (kryst_ctx_scalar_reduce; collective except 'query').
        Returns the mode in use afterwards ('ipc' falls back to 'rccl' on every rank when a mailbox cannot be mapped or the test reduction
        does not arrive intact).  A context of several ranks starts on 'ipc' when that works everywhere (KRYST_SCALAR_REDUCE=rccl: never)."""
        active = C.c_int32(0)
        rc = lib().kryst_ctx_scalar_reduce(self.h, {"rccl": 0, "ipc": 1, "query": -1}[mode], C.byref(active))
        if rc not in (0, 6):
            check(rc)
        return "ipc" if active.value else "rccl"

    def synchronize(self):
        check(lib().kryst_ctx_synchronize(self.h))

    def trim(self):
        """Give the device blocks kept for reuse (destroyed ILU preconditioners' storage, the solvers' work arena) back to the driver
        (kryst_ctx_trim) -> bytes released."""
        n = C.c_int64(0)
        check(lib().kryst_ctx_trim(self.h, C.byref(n)))
        return n.value

    def poison_lds(self):
        """Test hook: NaNs into every compute unit's LDS (a kernel must not depend on what LDS held before it started)."""
        check(lib().kryst_bench_poison_lds(self.h))

    def timer_start(self):
        check(lib().kryst_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_double()
        check(lib().kryst_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def phase_timing_begin(self):
        """Start charging device time to phases (spmv / halo_wait / spmv_boundary / reduce / blas1 / pc): measurement only."""
        check(lib().kryst_phase_timing_begin(self.h))

    def phase_timing_end(self):
        """-> {phase name: ms} of the work enqueued since phase_timing_begin (synchronises the context)."""
        n = lib().kryst_phase_count()
        ms = (C.c_double * n)()
        check(lib().kryst_phase_timing_end(self.h, ms, n))
        return {lib().kryst_phase_name(i).decode(): ms[i] for i in range(n)}

    def vec(self, n_or_array):
        return DeviceVec(self, n_or_array)

    def _adopt(self, child):
        """remember `child` (weakly): close() destroys it before the context"""
        key = id(child)
        self._children[key] = weakref.ref(child, lambda _r, k=key, c=self._children: c.pop(k, None))

    def close(self):
        """Destroy the context and, first, whatever still lives on it (see the class docstring).  Safe to call twice."""
        if not getattr(self, "h", None):
            return
        alive = [c for c in (r() for r in list(self._children.values())) if c is not None]
        for c in sorted(alive, key=lambda c: c._CLOSE_ORDER):       # (stable: creation order within a kind)
            c._release()
        self._children.clear()
        lib().kryst_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            if self.nranks == 1:
                self.close()
        except Exception:
            pass


class _Owned:
    """What every object with a handle of a context shares: the context knows it (weakly), `_release()` destroys the handle once and leaves
    `h = None`; dropping the object releases it."""
    _CLOSE_ORDER = 4                                 # Context.close(): 0 sessions, 1 preconditioners, 2 lowered operators, 3 operators, 4 vectors
    _DESTROY = None                                  # the kryst_*_destroy symbol
    h = None
    ctx = None

    def _release(self):
        h, self.h = self.h, None
        if h and self.ctx is not None and self.ctx.h:
            getattr(lib(), self._DESTROY)(h)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


class DeviceVec(_Owned):
    """A Vec<f64> resident in HBM."""
    _DESTROY = "kryst_vec_destroy"

    def __init__(self, ctx, n_or_array):
        self.ctx = ctx
        self.h = _ffi.Handle()
        if np.isscalar(n_or_array):
            self.n = int(n_or_array)
            check(lib().kryst_vec_create(ctx.h, self.n, C.byref(self.h)))
            ctx._adopt(self)
        else:
            a = _f64(n_or_array)
            self.n = len(a)
            check(lib().kryst_vec_create(ctx.h, self.n, C.byref(self.h)))
            ctx._adopt(self)
            self.upload(a)

    def __len__(self):
        return self.n

    def upload(self, a):
        a = _f64(a)
        check(lib().kryst_vec_upload(self.h, _dp(a), len(a)))
        return self

    def to_host(self):
        out = np.empty(self.n)
        check(lib().kryst_vec_download(self.h, _dp(out), self.n))
        return out

    def fill(self, v):
        check(lib().kryst_vec_fill(self.h, float(v)))
        return self

    def fill_splitmix(self, seed, global_offset=0):
        check(lib().kryst_vec_fill_splitmix(self.h, seed, global_offset))
        return self

    def copy_from(self, other):
        check(lib().kryst_vec_copy(self.h, other.h))
        return self

    QUIET_NAN_BITS = 0x7FF8000000000000

    def poison_padding(self, value=None):
        """Test hook (kryst_bench_vec_padding): every allocated element behind the n-th -- the rest of the last 512-element tile and the
        whole extra tile -- becomes `value` (default: the quiet NaN 0x7FF8000000000000).  Results must not depend on it."""
        fill = np.array([self.QUIET_NAN_BITS], dtype=np.uint64).view(np.float64) if value is None else np.array([value], dtype=np.float64)
        check(lib().kryst_bench_vec_padding(self.h, _dp(fill), None))
        return self

    def padding_dirty(self):
        """How many allocated elements behind the n-th are not +0.0 (kryst_bench_vec_padding)."""
        dirty = C.c_int64(-1)
        check(lib().kryst_bench_vec_padding(self.h, None, C.byref(dirty)))
        return dirty.value


MVEC_WIDTHS = (8, 4, 2)


def split_widths(m):
    """How m right-hand sides are cut into multivectors: greedily into groups of 8, 4 and 2 columns; a leftover single column goes through
    the single-vector call (width 1).  15 -> [8, 4, 2, 1].  No padding columns are invented."""
    m = int(m)
    if m < 0:
        raise ValueError("split_widths: m < 0")
    out = []
    for w in MVEC_WIDTHS:
        while m >= w:
            out.append(w)
            m -= w
    if m:
        out.append(1)
    return out


class MultiVec(_Owned):
    """n x k device multivector, k in {2, 4, 8} (kryst_mvec_t): the k values of a row are contiguous in HBM."""
    _DESTROY = "kryst_mvec_destroy"

    def __init__(self, ctx, n, k):
        self.ctx, self.n, self.k = ctx, int(n), int(k)
        self.h = _ffi.Handle()
        check(lib().kryst_mvec_create(ctx.h, self.n, self.k, C.byref(self.h)))
        ctx._adopt(self)

    @staticmethod
    def from_numpy(a, ctx=None):
        """a: array of shape (n, k) in either memory order."""
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2:
            raise KError(102, "MultiVec.from_numpy: a two-dimensional array is required")
        mv = MultiVec(ctx or Context.default(), a.shape[0], a.shape[1])
        return mv.upload(a)

    @property
    def shape(self):
        return (self.n, self.k)

    def upload(self, a):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (self.n, self.k):
            raise KError(102, "MultiVec.upload: shape mismatch")
        cm = np.asfortranarray(a)                       # column j at cm.ravel('K')[j * n:], ld = n
        check(lib().kryst_mvec_upload(self.h, _dp(cm), max(self.n, 1)))
        return self

    def to_numpy(self):
        out = np.empty((self.n, self.k), order="F")
        check(lib().kryst_mvec_download(self.h, _dp(out), max(self.n, 1)))
        return out

    def column(self, j):
        v = DeviceVec(self.ctx, self.n)
        check(lib().kryst_mvec_get_column(self.h, int(j), v.h))
        return v

    def set_column(self, j, v):
        if not isinstance(v, DeviceVec):
            v = DeviceVec(self.ctx, v)
        check(lib().kryst_mvec_set_column(self.h, int(j), v.h))
        return self

    def poison_padding(self, value=None):
        """Test hook (kryst_bench_mvec_padding): every allocated element of row index >= n becomes `value` (default: a quiet NaN)."""
        fill = np.array([DeviceVec.QUIET_NAN_BITS], dtype=np.uint64).view(np.float64) if value is None else np.array([value], dtype=np.float64)
        check(lib().kryst_bench_mvec_padding(self.h, _dp(fill), None))
        return self

    def padding_dirty(self):
        dirty = C.c_int64(-1)
        check(lib().kryst_bench_mvec_padding(self.h, None, C.byref(dirty)))
        return dirty.value


def _fp(a):
    return a.ctypes.data_as(_ffi.c_fp)


def reduce_spec32():
    """(T, V, F) of the inner-product tree of fp32-stored vectors (kryst_reduce_spec32): 256 threads x 4 elements per tile."""
    t, v, f = C.c_int32(), C.c_int32(), C.c_int32()
    lib().kryst_reduce_spec32(C.byref(t), C.byref(v), C.byref(f))
    return t.value, v.value, f.value


def host_round_f32(values):
    """The rounding of CsrMatrix.lower() on the host, no GPU (kryst_host_round_f32) -> (float32 array, changed, tiny): the values the
    rounding changed and the nonzero values that became zero or fp32-subnormal.  A finite value that would round to +-inf raises
    KError Unsupported, as lower() does."""
    v = _f64(values).ravel()
    out = np.empty(len(v), dtype=np.float32)
    info = (C.c_int64 * 2)()
    check(lib().kryst_host_round_f32(_dp(v), len(v), _fp(out), info))
    return out, info[0], info[1]


class DeviceVec32(_Owned):
    """A Vec<f32> resident in HBM (kryst_vec32_t): fp32 is how the elements are stored, every kernel computes in fp64."""
    _DESTROY = "kryst_vec32_destroy"

    def __init__(self, ctx, n_or_array):
        self.ctx = ctx
        self.h = _ffi.Handle()
        if np.isscalar(n_or_array):
            self.n = int(n_or_array)
            check(lib().kryst_vec32_create(ctx.h, self.n, C.byref(self.h)))
            ctx._adopt(self)
        else:
            a = np.ascontiguousarray(n_or_array, dtype=np.float32)
            self.n = len(a)
            check(lib().kryst_vec32_create(ctx.h, self.n, C.byref(self.h)))
            ctx._adopt(self)
            self.upload(a)

    def __len__(self):
        return self.n

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        check(lib().kryst_vec32_upload(self.h, _fp(a), len(a)))
        return self

    def to_host(self):
        out = np.empty(self.n, dtype=np.float32)
        check(lib().kryst_vec32_download(self.h, _fp(out), self.n))
        return out

    @staticmethod
    def from_f64(v, out=None):
        """(float)v[i] of a DeviceVec, rounded on the device."""
        out = DeviceVec32(v.ctx, v.n) if out is None else out
        check(lib().kryst_vec32_from_f64(out.h, v.h))
        return out

    def to_f64(self, out=None):
        """(double)self[i] as a DeviceVec, widened on the device."""
        out = DeviceVec(self.ctx, self.n) if out is None else out
        check(lib().kryst_vec32_to_f64(out.h, self.h))
        return out

    QUIET_NAN_BITS = 0x7FC00000

    def poison_padding(self, value=None):
        """Test hook (kryst_bench_vec32_padding): every allocated float behind the n-th -- the rest of the last 1024-element tile and the
        whole extra tile -- becomes `value` (default: the quiet NaN 0x7FC00000).  Results must not depend on it."""
        fill = np.array([self.QUIET_NAN_BITS], dtype=np.uint32).view(np.float32) if value is None else np.array([value], dtype=np.float32)
        check(lib().kryst_bench_vec32_padding(self.h, _fp(fill), None))
        return self

    def padding_dirty(self):
        """How many allocated floats behind the n-th are not +0.0 (kryst_bench_vec32_padding)."""
        dirty = C.c_int64(-1)
        check(lib().kryst_bench_vec32_padding(self.h, None, C.byref(dirty)))
        return dirty.value


def dot32(x, y):
    """InnerProduct::dot on fp32-stored device vectors: exact fp64 terms folded in the tree of reduce_spec32()."""
    out = C.c_double()
    check(lib().kryst_dot32(x.h, y.h, C.byref(out)))
    return out.value


class CsrMatrix32(_Owned):
    """CsrMatrix<f32> lowered from a CsrMatrix (kryst_csr32_lower_form): its own copies of the index arrays, the values rounded to fp32.
    form "plain" keeps the CSR arrays alone; "pattern" also keeps the operator's CSR-P16 row-pattern form with fp32 tables (KError Unsupported
    when it has none); "auto" keeps it where there is one; "dia" (opt-in, never chosen by "auto") also keeps the operator's CSR-DIA diagonal
    streams in fp32 (Unsupported when it has none: an operator gets them at creation, by default only where it has no CSR-D16 / CSR-P16
    form, under KRYST_SPMV_DIA=2 wherever its diagonals are well filled)."""
    FORMS = {"plain": 0, "auto": 1, "pattern": 2}
    KERNELS = ("plain", "pattern", "pattern-stage")
    FORMS_EXT = {"dia": 3}              # the forms and kernels added since, kept beside the first three
    KERNELS_EXT = ("dia",)
    DIA_ABSENT_BITS = 0x7FD1A0D1        # KRYST_CSR32_DIA_ABSENT_BITS: "no entry here" in an fp32 diagonal stream
    _DESTROY, _CLOSE_ORDER = "kryst_csr32_destroy", 2

    @classmethod
    def form_code(cls, form):
        """the KRYST_CSR32_* code of a form's name; KError ERR_ARG for an unknown name"""
        code = cls.FORMS.get(form, cls.FORMS_EXT.get(form))
        if code is None:
            raise KError(102, f"form must be one of {sorted({**cls.FORMS, **cls.FORMS_EXT})}, not {form!r}")
        return code

    def __init__(self, a, form="plain"):
        self.ctx = a.ctx
        self.h = _ffi.Handle()
        check(lib().kryst_csr32_lower_form(a.h, self.form_code(form), C.byref(self.h)))
        self.ctx._adopt(self)
        self._nrows, self._ncols, self.nnz = a.nrows(), a.ncols(), a.nnz

    def nrows(self):
        return self._nrows

    def ncols(self):
        return self._ncols

    @property
    def info(self):
        """{"changed", "tiny", "rows"}: values the rounding changed, nonzero values that became zero or fp32-subnormal, rows."""
        i = (C.c_int64 * 3)()
        check(lib().kryst_csr32_info(self.h, i))
        return {"changed": i[0], "tiny": i[1], "rows": i[2]}

    def encoding(self):
        """The kernel the next spmv (and every SpMV of a solve) takes under the current settings (kryst_csr32_encoding): "plain",
        "pattern", "pattern-stage" or "dia".  KRYST_SPMV32_FORM=plain|pattern|dia and KRYST_SPMV32_STAGE=0|1 steer it."""
        k = C.c_int32(-1)
        check(lib().kryst_csr32_encoding(self.h, C.byref(k)))
        return (self.KERNELS + self.KERNELS_EXT)[k.value]

    def spmv(self, x, y=None):
        """y <- (float)(A x): the row fold in fp64 over the stored order, rounded once.  DeviceVec32 stays on the device; a host array is
        converted to float32 and round-trips."""
        if isinstance(x, DeviceVec32):
            if y is None:
                y = DeviceVec32(self.ctx, self._nrows)
            check(lib().kryst_spmv32(self.h, x.h, y.h))
            return y
        xv, yv = DeviceVec32(self.ctx, x), DeviceVec32(self.ctx, self._nrows)
        check(lib().kryst_spmv32(self.h, xv.h, yv.h))
        return yv.to_host()


def dot(x, y):
    """InnerProduct::dot (wrappers.rs:90-108) on device vectors."""
    out = C.c_double()
    check(lib().kryst_dot(x.h, y.h, C.byref(out)))
    return out.value


def norm(x):
    """InnerProduct::norm (wrappers.rs:110-127)."""
    out = C.c_double()
    check(lib().kryst_norm(x.h, C.byref(out)))
    return out.value


def axpy(alpha, x, y):
    check(lib().kryst_axpy(float(alpha), x.h, y.h))


def aypx(beta, x, y):
    check(lib().kryst_aypx(float(beta), x.h, y.h))


def sub(a, b, out):
    """out[i] = a[i] - b[i] (cg.rs:123 `bi - ax`); `out` may be `a` or `b`."""
    check(lib().kryst_sub(a.h, b.h, out.h))
    return out


STENCIL_KINDS = {"poisson": 0, "aniso": 1, "convdiff": 2, "varcoef": 3}   # kryst_csr_create_stencil7 / kryst_host_stencil7


class CsrMatrix(_Owned):
    """CsrMatrix<f64> (src/matrix/sparse.rs:22-46) living on the GPU; implements SparseMatrix::spmv and MatVec."""
    _DESTROY, _CLOSE_ORDER = "kryst_csr_destroy", 3

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        ctx._adopt(self)
        nr, nc, nz = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().kryst_csr_shape(self.h, C.byref(nr), C.byref(nc), C.byref(nz)))
        self._nrows, self._ncols, self.nnz = nr.value, nc.value, nz.value

    @staticmethod
    def from_csr(nrows, ncols, row_ptr, col_idx, values, ctx=None):
        """from_csr(nrows, ncols, row_ptr: Vec<usize>, col_idx: Vec<usize>, values)  sparse.rs:28-46.
        Violating new_checked's preconditions raises KError (the reference panics)."""
        ctx = ctx or Context.default()
        rp = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        ci = np.ascontiguousarray(col_idx, dtype=np.uint64)
        va = _f64(values)
        if len(rp) != nrows + 1 or len(ci) != len(va) or (len(rp) and int(rp[-1]) != len(va)):
            raise KError(102, "from_csr: inconsistent array lengths")
        h = _ffi.Handle()
        check(lib().kryst_csr_create(ctx.h, nrows, ncols, rp.ctypes.data_as(_ffi.c_u64p), ci.ctypes.data_as(_ffi.c_u64p),
                                     _dp(va), C.byref(h)))
        return CsrMatrix(ctx, h)

    @staticmethod
    def from_csr_i32(nrows, ncols, row_ptr, col_idx, values, ctx=None):
        ctx = ctx or Context.default()
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        va = _f64(values)
        h = _ffi.Handle()
        check(lib().kryst_csr_create_i32(ctx.h, nrows, ncols, rp.ctypes.data_as(_ffi.c_i64p),
                                         ci.ctypes.data_as(_ffi.c_i32p), _dp(va), C.byref(h)))
        return CsrMatrix(ctx, h)

    @staticmethod
    def from_csr_dist(ctx, n_global, row_offsets, row_ptr, col_idx_global, values):
        """Row block [row_offsets[rank], row_offsets[rank+1]) of a row-partitioned operator (global columns)."""
        ro = np.ascontiguousarray(row_offsets, dtype=np.int64)
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx_global, dtype=np.int64)
        va = _f64(values)
        h = _ffi.Handle()
        check(lib().kryst_csr_create_dist(ctx.h, n_global, ro.ctypes.data_as(_ffi.c_i64p), rp.ctypes.data_as(_ffi.c_i64p),
                                          ci.ctypes.data_as(_ffi.c_i64p), _dp(va), C.byref(h)))
        return CsrMatrix(ctx, h)

    @staticmethod
    def from_matrix_market(path, ctx=None):
        nr, nc, rp, ci, va = read_matrix_market(path)
        return CsrMatrix.from_csr(nr, nc, rp, ci, va, ctx=ctx)

    @staticmethod
    def from_petsc_binary(path, ctx=None):
        nr, nc, rp, ci, va = read_petsc_binary(path)
        return CsrMatrix.from_csr(nr, nc, rp, ci, va, ctx=ctx)

    @staticmethod
    def stencil7(N, kind="poisson", ctx=None):
        """Synthetic 7-point operator on an N^3 grid; each rank of a distributed ctx gets its k-slab."""
        ctx = ctx or Context.default()
        h = _ffi.Handle()
        check(lib().kryst_csr_create_stencil7(ctx.h, N, STENCIL_KINDS[kind], C.byref(h)))
        return CsrMatrix(ctx, h)

    def nrows(self):
        return self._nrows

    def ncols(self):
        return self._ncols

    def spmv(self, x, y=None):
        """SparseMatrix::spmv(&self, x, y): y <- A x.  Device vectors stay on the device; host arrays round-trip
        over PCIe (operator-level drop-in, plumbing only)."""
        if isinstance(x, DeviceVec):
            if y is None:
                y = DeviceVec(self.ctx, self._nrows)
            check(lib().kryst_spmv(self.h, x.h, y.h))
            return y
        xa = _f64(x)
        out = np.empty(self._nrows) if y is None else y
        if len(out) != self._nrows:
            raise KError(102, "spmv: y.len() != nrows")
        tmp = out if (out.dtype == np.float64 and out.flags.c_contiguous) else np.empty(self._nrows)
        check(lib().kryst_spmv_host(self.h, _dp(xa), len(xa), _dp(tmp), len(tmp)))
        if tmp is not out:
            out[:] = tmp
        return out

    def spmv_transpose(self, x, y=None):
        """MatTransVec::mattransvec: y <- A^T x (x of length nrows, y of length ncols).  A^T is built on the device by the first
        call and cached on the operator (it costs about as much memory as A).  Host arrays round-trip over PCIe."""
        if isinstance(x, DeviceVec):
            if y is None:
                y = DeviceVec(self.ctx, self._ncols)
            check(lib().kryst_spmv_transpose(self.h, x.h, y.h))
            return y
        xv = DeviceVec(self.ctx, _f64(x))
        yv = DeviceVec(self.ctx, self._ncols)
        check(lib().kryst_spmv_transpose(self.h, xv.h, yv.h))
        if y is None:
            return yv.to_host()
        if len(y) != self._ncols:
            raise KError(102, "spmv_transpose: y.len() != ncols")
        y[:] = yv.to_host()
        return y

    def spmm(self, X, Y=None):
        """Y <- A X for several columns at once: column j is spmv on column j, bit for bit.  X: MultiVec, or an array of shape (ncols, m)
        with any m (cut by split_widths; a leftover single column takes spmv); returns a MultiVec or an (nrows, m) array."""
        if isinstance(X, MultiVec):
            if Y is None:
                Y = MultiVec(self.ctx, self._nrows, X.k)
            check(lib().kryst_spmm(self.h, X.h, Y.h))
            return Y
        xa = np.asarray(X, dtype=np.float64)
        if xa.ndim != 2 or xa.shape[0] != self._ncols:
            raise KError(102, "spmm: X must have shape (ncols, m)")
        out = np.empty((self._nrows, xa.shape[1]), order="F") if Y is None else Y
        if out.shape != (self._nrows, xa.shape[1]):
            raise KError(102, "spmm: Y must have shape (nrows, m)")
        at = 0
        for w in split_widths(xa.shape[1]):
            if w == 1:
                out[:, at] = self.spmv(np.ascontiguousarray(xa[:, at]))
            else:
                out[:, at:at + w] = self.spmm(MultiVec.from_numpy(xa[:, at:at + w], ctx=self.ctx)).to_numpy()
            at += w
        return out

    SPMM_KERNELS = ("plain", "dia")

    def spmm_kernel(self, k):
        """The kernel spmm and solve_many take for k columns (2, 4 or 8) under the current KRYST_SPMM_FORM (auto | plain | dia): "plain"
        (the CSR arrays) or "dia" (the CSR-DIA value streams)."""
        kernel = C.c_int32()
        check(lib().kryst_spmm_kernel(self.h, int(k), C.byref(kernel)))
        return self.SPMM_KERNELS[kernel.value]

    def lower(self, form="plain"):
        """This operator with fp32-stored values (CsrMatrix32; an extension): a copy, with no tie to this one's lifetime.  form: "plain"
        (the CSR arrays), "pattern" (also the CSR-P16 row-pattern form; refused where the operator has none), "auto", or "dia" (also
        the CSR-DIA diagonal streams in fp32; refused where the operator has none)."""
        return CsrMatrix32(self, form)

    ENCODINGS = ("csr", "csr-d8", "csr-d16", "csr-p16", "csr-dia")

    def encoding(self):
        """(name, patterns, table_entries) of the storage form kryst_spmv streams (see kryst_csr_encoding)."""
        e, p, t = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(lib().kryst_csr_encoding(self.h, C.byref(e), C.byref(p), C.byref(t)))
        return self.ENCODINGS[e.value], p.value, t.value

    def tile_order(self):
        """Measurement hook (kryst_csr_tile_order): {"plane_rows", "slots", "slots8", "in_use"} of the slab order of the tiles."""
        info = (C.c_int64 * 4)()
        check(lib().kryst_csr_tile_order(self.h, info))
        return {"plane_rows": info[0], "slots": info[1], "slots8": info[2], "in_use": bool(info[3])}

    def pattern_info(self):
        """Measurement hook (kryst_csr_pattern_info): {"line", "uniform_far", "interior_first", "staged"} of the CSR-P16 form."""
        info = (C.c_int64 * 4)()
        check(lib().kryst_csr_pattern_info(self.h, info))
        return {"line": info[0], "uniform_far": bool(info[1]), "interior_first": info[2], "staged": bool(info[3])}

    def fuse_march_info(self):
        """Measurement hook (kryst_csr_fuse_march_info): the marching mode of the fused direction + SpMV kernel under the current
        KRYST_SPMV_FUSE_* settings -- {"eligible", "on", "T", "strips", "S", "segments"} -- and "recompute_ap": whether a fused CG iteration would
        now store no Ap and form it again in its residual pass (KRYST_CG_RECOMPUTE_AP, x in batches).  From kryst_csr_pid_reuse_info: "pid_reuse":
        whether a marching launch would now keep repeated row-pattern ids in registers (KRYST_SPMV_PID_REUSE and the operator's per-tile table),
        "pid_same_tiles": tiles whose ids repeat the tile one plane below, "tiles": tiles the table covers (both 0 without a table)."""
        info = (C.c_int64 * 7)()
        check(lib().kryst_csr_fuse_march_info(self.h, info))
        reuse = (C.c_int64 * 3)()
        check(lib().kryst_csr_pid_reuse_info(self.h, reuse))
        return {"eligible": bool(info[0]), "on": bool(info[1]), "T": info[2], "strips": info[3], "S": info[4], "segments": info[5],
                "recompute_ap": bool(info[6]), "pid_reuse": bool(reuse[0]), "pid_same_tiles": reuse[1], "tiles": reuse[2]}

    def leg_values_info(self):
        """Measurement hook (kryst_csr_leg_values_info): the step of CG's recompute residual pass -- {"eligible": every leg of the seven-leg base
        carries one value wherever a row pattern has it, "on": a recompute residual pass would now take the seven values as kernel arguments
        (KRYST_SPMV_LEG_VALUES; the marching mode and KRYST_CG_RECOMPUTE_AP on), "values": the seven leg values (0.0 throughout when not
        eligible)}."""
        info = (C.c_int64 * 2)()
        vals = (C.c_double * 7)()
        check(lib().kryst_csr_leg_values_info(self.h, info, vals))
        return {"eligible": bool(info[0]), "on": bool(info[1]), "values": [vals[u] for u in range(7)]}

    def placement_info(self):
        """Where the CSR arrays live (kryst_csr_placement_info): {"tries", "chosen", "skeleton_ms": [...]} of the homes tried at creation."""
        t, c = C.c_int32(0), C.c_int32(0)
        ms = (C.c_double * 8)()
        check(lib().kryst_csr_placement_info(self.h, C.byref(t), C.byref(c), ms))
        return {"tries": t.value, "chosen": c.value, "skeleton_ms": [ms[k] for k in range(t.value)]}

    def bench_spmv(self, x, y, fused_dots=1, reps=50):
        """Average milliseconds per launch of the SpMV kernel (HIP events on the compute stream)."""
        ms = C.c_double()
        check(lib().kryst_bench_spmv(self.h, x.h, y.h, fused_dots, reps, C.byref(ms)))
        return ms.value

    def bench_spmv_fused(self, x, y, reps=20):
        """Average milliseconds per launch of the fused direction + SpMV kernel of CG / PCG (kryst_bench_spmv_fused); None when the operator
        cannot take that form."""
        ms = C.c_double()
        rc = lib().kryst_bench_spmv_fused(self.h, x.h, y.h, reps, C.byref(ms))
        if rc == 6:
            return None
        check(rc)
        return ms.value

    def halo_mode(self, mode):
        """'rccl' | 'peer' | 'query': how this row-partitioned operator's halo exchange travels (kryst_csr_halo_mode; collective except
        'query').  Returns the mode in use: 'peer' falls back to 'rccl' on every rank when a landing buffer cannot be exported / mapped or
        the test exchange does not arrive intact (KRYST_UNSUPPORTED).  A new operator starts on 'peer' when that works everywhere
        (KRYST_HALO_MODE=rccl: never)."""
        active = C.c_int32(0)
        rc = lib().kryst_csr_halo_mode(self.h, {"rccl": 0, "peer": 1, "query": -1}[mode], C.byref(active))
        if rc not in (0, 6):                     # (6 = KRYST_UNSUPPORTED: the documented fallback)
            check(rc)
        return "peer" if active.value == 1 else "rccl"

    def bench_csr_skeleton(self, x, y, reps=10):
        """Average milliseconds per launch of the plain-CSR kernel's traffic skeleton (the CSR arrays streamed, x read, y written -- no
        arithmetic; y receives garbage)."""
        ms = C.c_double()
        check(lib().kryst_bench_csr_skeleton(self.h, x.h, y.h, reps, C.byref(ms)))
        return ms.value

    matvec = spmv                                # MatVec::matvec (core/traits.rs:4-7)
    spmv_parallel = spmv                         # sparse.rs:103-114 (same arithmetic)

    def download(self):
        rp = np.empty(self._nrows + 1, dtype=np.int64)
        ci = np.empty(self.nnz, dtype=np.int32)
        va = np.empty(self.nnz)
        check(lib().kryst_csr_download(self.h, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va)))
        return rp, ci, va


# ----------------------------------------------------------------------------- preconditioners
class _Pc(_Owned):
    """Preconditioner<M, V> (src/preconditioner/mod.rs:8-13): setup(&mut self, a), apply(&self, r, z)."""
    _DESTROY, _CLOSE_ORDER = "kryst_pc_destroy", 1

    def __init__(self):
        self.h, self.ctx = None, None

    def _set(self, ctx, handle):
        self._free()
        self.ctx, self.h = ctx, handle
        ctx._adopt(self)

    def apply(self, r, z=None):
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        if isinstance(r, DeviceVec):
            z = z if z is not None else DeviceVec(self.ctx, len(r))
            check(lib().kryst_pc_apply(self.h, r.h, z.h))
            return z
        rv = DeviceVec(self.ctx, r)
        zv = DeviceVec(self.ctx, len(rv))
        check(lib().kryst_pc_apply(self.h, rv.h, zv.h))
        out = zv.to_host()
        if z is not None:
            z[:] = out
            return z
        return out

    def bench_apply(self, r, z, reps=20):
        """Average milliseconds of one apply (HIP events on the compute stream, `reps` back-to-back applies)."""
        ms = C.c_double()
        check(lib().kryst_bench_pc_apply(self.h, r.h, z.h, reps, C.byref(ms)))
        return ms.value

    def ilu_info(self):
        """What an ILU-family apply runs and streams (kryst_pc_ilu_info) -> dict."""
        v = np.zeros(13, dtype=np.int64)
        check(lib().kryst_pc_ilu_info(self.h, v.ctypes.data_as(_ffi.c_i64p), 13))
        form = ("level-ordered", "grid 8x8 (tri_wave_kernel)", "grid 16x16 (tri_quad_kernel)", "grid planes (tri_plane_kernel)",
                "box planes (tri_box_plane_kernel)", "box wavefront (tri_box_kernel)")[int(v[0])]
        if form.startswith("box"):          # info[6..8]: coefficient streams L / U have (of 13 each), both factors "regular" (tri_box.h)
            return {"form": form, "box": [int(v[1]), int(v[2]), int(v[3])], "levels": [int(v[4]), int(v[5])], "streams": [int(v[6]), int(v[7])],
                    "regular": bool(v[8]), "chunks": [0, 0], "chunks_not_requested": [0, 0], "bytes_per_chunk": [0, 0]}
        return {"form": form, "box": [int(v[1]), int(v[2]), int(v[3])], "levels": [int(v[4]), int(v[5])], "chunks": [int(v[6]), int(v[7])],
                "chunks_not_requested": [int(v[8]), int(v[9])], "bytes_per_chunk": [int(v[10]), int(v[11])]}

    def _free(self):
        try:
            self._release()
        except Exception:
            pass
        self.h = None


class Jacobi(_Pc):
    """Jacobi::new(); setup extracts 1/diag (src/preconditioner/jacobi.rs:26-95)."""

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_jacobi(a.h, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self


class _IluBase(_Pc):
    MODE = 0

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_ilu0(a.h, self.MODE, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self


class Ilu0(_IluBase):
    """Ilu0 exactly as written in src/preconditioner/ilu.rs:59-122 (L = I + tril(A,-1)D^-1, U = I + triu(A,1))."""
    MODE = 0


class Ilup(_IluBase):
    """Ilup::new(fill) exactly as written in src/preconditioner/ilup.rs:54-167 (level-of-fill p; p = 0 performs no
    elimination at all)."""
    MODE = 1

    def __init__(self, fill=0):
        super().__init__()
        self.fill = fill

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_ilup(a.h, self.fill, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self


class Ilut(_IluBase):
    """Ilut::new(fill, droptol) exactly as written in src/preconditioner/ilut.rs:55-150 (no elimination: drop by
    magnitude, keep the `fill` largest entries of each row, split at the diagonal)."""

    def __init__(self, fill, droptol):
        super().__init__()
        self.fill, self.droptol = fill, droptol

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_ilut(a.h, self.fill, self.droptol, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self


class TrueIlu0(_IluBase):
    """Extension: textbook ILU(0) on A's pattern (not in the reference)."""
    MODE = 2


class Chebyshev(_Pc):
    """Chebyshev::new(degree, lambda_min, lambda_max); the trait apply is a stub that returns Err
    (src/preconditioner/chebyshev.rs:35-70) -- use apply_chebyshev."""

    def __init__(self, degree, lambda_min=None, lambda_max=None):
        super().__init__()
        self.degree, self.lambda_min, self.lambda_max = degree, lambda_min, lambda_max

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_chebyshev_stub(a.ctx.h, self.degree, C.byref(h)))
        self._set(a.ctx, h)
        return self


class ChebyshevPc(_Pc):
    """Extension: a Preconditioner whose apply is apply_chebyshev(a, r, z, alpha, beta, degree)."""

    def __init__(self, degree, alpha, beta):
        super().__init__()
        self.degree, self.alpha, self.beta = degree, alpha, beta

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_chebyshev(a.h, self.alpha, self.beta, self.degree, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self


def host_tridiag_extreme_eigs(alpha, beta):
    """(lo, hi): the extreme eigenvalues of the symmetric tridiagonal matrix with diagonal `alpha` (k entries, k in 1..64) and off-diagonal
    `beta` (its first k - 1 entries are used) by bisection with Sturm counts (kryst_host_tridiag_extreme_eigs; host only, no GPU)."""
    al, be = _f64(alpha), _f64(beta)
    if len(be) < len(al) - 1:
        raise KError(102, "host_tridiag_extreme_eigs: beta needs len(alpha) - 1 entries")
    be = _f64(np.concatenate([be, [0.0]]))              # (never NULL)
    lo, hi = C.c_double(), C.c_double()
    check(lib().kryst_host_tridiag_extreme_eigs(_dp(al), _dp(be), len(al), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def _check_diag(rc):
    """check(), with the row of a diagonal entry Jacobi scaling cannot use (KRYST_INDEFINITE_PRECONDITIONER) in KError.row"""
    if rc == 4:
        msg = lib().kryst_hip_last_error()
        raise KError(rc, msg.decode() if msg else "", None, lib().kryst_hip_last_error_row())
    check(rc)


def estimate_spectrum(a, jacobi=True, steps=10, seed=0x5EED):
    """Extension (kryst_spectrum_estimate): up to `steps` Lanczos steps on W^1/2 A W^1/2 (W = Jacobi's inverse diagonal, or nothing with
    jacobi=False) and the Gershgorin bound of W A -> {"alpha", "beta", "steps_done", "theta_min", "theta_max", "gershgorin"}.  Single-rank
    operators; a distributed one raises KError(Unsupported)."""
    steps = int(steps)
    al, be = np.zeros(max(steps, 1)), np.zeros(max(steps, 1))
    k, tmin, tmax, g = C.c_int32(0), C.c_double(), C.c_double(), C.c_double()
    _check_diag(lib().kryst_spectrum_estimate(a.h, 1 if jacobi else 0, steps, seed, _dp(al), _dp(be), C.byref(k), C.byref(tmin), C.byref(tmax), C.byref(g)))
    return {"alpha": al[:k.value].copy(), "beta": be[:k.value].copy(), "steps_done": k.value, "theta_min": tmin.value, "theta_max": tmax.value,
            "gershgorin": g.value}


class ChebyshevPoly(_Pc):
    """Extension (kryst_pc_chebyshev_poly; nothing in the reference corresponds -- Chebyshev above is its stub, ChebyshevPc its filter): the
    Chebyshev polynomial preconditioner z = p_degree(W A) W r, `degree` SpMVs per apply, with W = Jacobi's inverse diagonal (jacobi=True)
    or nothing.  Bounds of the spectrum of W A that are None are estimated in setup (estimate_spectrum with `steps` and `seed`):
    lambda_max = min(safety * theta_max, gershgorin), lambda_min = lambda_max / ratio.  Takes row-partitioned operators when both bounds
    are given."""

    def __init__(self, degree, lambda_min=None, lambda_max=None, jacobi=True, steps=10, ratio=30.0, safety=1.1, seed=0x5EED):
        super().__init__()
        self.degree, self.lambda_min, self.lambda_max, self.jacobi = degree, lambda_min, lambda_max, jacobi
        self.steps, self.ratio, self.safety, self.seed = steps, ratio, safety, seed
        self.estimate = None

    def setup(self, a):
        lo, hi = self.lambda_min, self.lambda_max
        if lo is None or hi is None:
            self.estimate = estimate_spectrum(a, self.jacobi, self.steps, self.seed)
            if hi is None:
                hi = min(float(self.safety) * self.estimate["theta_max"], self.estimate["gershgorin"])
            if lo is None:
                lo = hi / float(self.ratio)
        h = _ffi.Handle()
        check(lib().kryst_pc_chebyshev_poly(a.h, self.degree, 1 if self.jacobi else 0, lo, hi, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def info(self):
        """{"degree", "jacobi", "lambda_min", "lambda_max", "fused"} of the set-up object (kryst_pc_chebyshev_poly_info); "fused": its step is
        the one-kernel form on the plain CSR arrays."""
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        d, sc, f = C.c_int32(), C.c_int32(), C.c_int32()
        lo, hi = C.c_double(), C.c_double()
        check(lib().kryst_pc_chebyshev_poly_info(self.h, C.byref(d), C.byref(sc), C.byref(lo), C.byref(hi), C.byref(f)))
        return {"degree": d.value, "jacobi": bool(sc.value), "lambda_min": lo.value, "lambda_max": hi.value, "fused": bool(f.value)}


class IdentityPc(_Pc):
    """The reference tests' IdentityPC (src/solver/pcg.rs:245-251)."""

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_identity(a.ctx.h, C.byref(h)))
        self._set(a.ctx, h)
        return self


class ApproxInv(_Pc):
    """ApproxInv (SPAI) with given inverse rows: `inv_rows[i]` = [(col, value), ...] in ascending column order, the layout of
    ApproxInv::inv_rows (src/preconditioner/approxinv.rs:66).  apply (approxinv.rs:268-298) is z = M r on the device.
    setup() here only checks the size against the operator.  To compute the rows from an operator (ApproxInv::setup,
    approxinv.rs:123-264) on the device, use `Spai(pattern, tol).setup(a)` or `PC.ApproxInv(pattern, tol, max_iter).build(a)`."""

    def __init__(self, inv_rows, ctx=None):
        super().__init__()
        n = len(inv_rows)
        rp = np.zeros(n + 1, dtype=np.int64)
        for i, row in enumerate(inv_rows):
            rp[i + 1] = rp[i] + len(row)
        ci = np.array([c for row in inv_rows for c, _ in row], dtype=np.int64)
        va = np.array([v for row in inv_rows for _, v in row], dtype=np.float64)
        self.m = CsrMatrix.from_csr(n, n, rp, ci, va, ctx=ctx)
        h = _ffi.Handle()
        check(lib().kryst_pc_approx_inverse(self.m.h, C.byref(h)))
        self._set(self.m.ctx, h)

    def setup(self, a):
        if a.nrows() != self.m.nrows():
            raise KError(102, "ApproxInv: inverse rows and operator differ in size")
        return self


class BlockJacobi(_Pc):
    """BlockJacobi (src/preconditioner/block_jacobi.rs:39-106) as a device preconditioner on the CSR operator.  `blocks`: a list of
    index lists, or a (ptr, idx) tuple of numpy arrays packed like CSR rows; the last block that contains a row decides it, rows in no block
    give z = +0.0.  `BlockJacobi.uniform(bsize)`: contiguous blocks of bsize rows, the last one shorter (an extension).  Labelled
    deviations: explicit inverses by Gauss-Jordan with full pivoting, index sets sorted ascending, errors (ZeroPivot with `.row`,
    FactorError, ArgumentError, Unsupported for blocks of more than 64 rows) where the reference gives non-finite z or panics."""

    def __init__(self, blocks=None, bsize=None):
        super().__init__()
        self.bsize = bsize
        if bsize is None:
            if isinstance(blocks, tuple) and len(blocks) == 2 and all(isinstance(v, np.ndarray) for v in blocks):   # (ptr, idx)
                self.ptr = np.ascontiguousarray(blocks[0], dtype=np.int64)
                self.idx = np.ascontiguousarray(blocks[1], dtype=np.int64)
            else:
                blocks = [np.asarray(b, dtype=np.int64).ravel() for b in blocks]
                self.ptr = np.zeros(len(blocks) + 1, dtype=np.int64)
                np.cumsum([len(b) for b in blocks], out=self.ptr[1:])
                self.idx = np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.int64)
            if len(self.ptr) < 1 or int(self.ptr[-1]) != len(self.idx):
                raise KError(102, "BlockJacobi: inconsistent (ptr, idx)")

    @staticmethod
    def uniform(bsize):
        return BlockJacobi(bsize=int(bsize))

    def setup(self, a):
        h = _ffi.Handle()
        if self.bsize is not None:
            check(lib().kryst_pc_block_jacobi_uniform(a.h, self.bsize, C.byref(h)))
        else:
            check(lib().kryst_pc_block_jacobi(a.h, self.ptr.ctypes.data_as(_ffi.c_i64p), self.idx.ctypes.data_as(_ffi.c_i64p),
                                              len(self.ptr) - 1, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def inverse_csr(self):
        """The preconditioner as the CSR matrix M with z = M r -> (row_ptr int64, col int32, val float64): row g[i] of the block that
        owns it holds (g[j], Binv[i][j]) for every j of that block, ascending; other rows are empty."""
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        nnz = C.c_int64()
        check(lib().kryst_pc_block_jacobi_export(self.h, C.byref(nnz), None, None, None))
        rp = np.zeros(self._a.nrows() + 1, dtype=np.int64)
        ci = np.zeros(nnz.value, dtype=np.int32)
        va = np.zeros(nnz.value, dtype=np.float64)
        check(lib().kryst_pc_block_jacobi_export(self.h, C.byref(nnz), rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p),
                                                 _dp(va)))
        return rp, ci, va


class AdditiveSchwarz(_Pc):
    """AdditiveSchwarz::new(overlap, subdomains) + setup + apply (src/preconditioner/asm.rs:34-119) with the direct solve as the inner
    solver, as a device preconditioner on the CSR operator: z = 0, then every subdomain in ascending order adds
    (B^-1 r|_g) into z[g]; rows in no subdomain give +0.0.  `subdomains`: a list of index lists, or a (ptr, idx) tuple of numpy arrays packed
    like CSR rows; None or empty: `nparts` uniform parts (asm.rs:46-56 with the reference's `capacity()`; None or 0 gives ONE part of all n
    rows).  As written `overlap` is stored and not used.  Labelled extensions: `.with_overlap()` grows every subdomain by `overlap` layers
    of the symmetrised graph of A; `.restricted()` grows them and keeps, per row, only the product of the last un-grown subdomain that
    contains it (RAS: not symmetric, for GMRES, FGMRES and BiCGStab, not PCG).  Labelled deviations, those of BlockJacobi: explicit
    Gauss-Jordan inverses, sorted index sets, errors (ZeroPivot with `.row`, FactorError, ArgumentError, Unsupported for a subdomain of
    more than 128 rows before or after growth) where the reference gives non-finite z or panics.  `.with_sub_ilu(mode)` (labelled
    extension) replaces the dense inverses by ILU(0) subdomain solves, each solved by one workgroup with its vector
    in LDS: subdomains of up to SUB_ILU_MAX_ROWS rows; with overlap, RAS keeps global ILU(0)'s iteration counts while the plain sum of
    inexact overlapping solves needs more iterations than no overlap at all."""
    AS_WRITTEN, GROWN, RESTRICTED = 0, 1, 2
    MAX_ROWS = 128
    SUB_ILU_MAX_ROWS = 16384
    _SUB_MODES = {"ilup0": 1, "ilu0": 2}

    def __init__(self, overlap=0, subdomains=None, nparts=None):
        super().__init__()
        self.overlap = int(overlap)
        self.nparts = 0 if nparts is None else int(nparts)
        self.variant = self.AS_WRITTEN
        self.sub_mode = None
        self.ptr = self.idx = None
        if subdomains is not None and len(subdomains) > 0:
            if isinstance(subdomains, tuple) and len(subdomains) == 2 and all(isinstance(v, np.ndarray) for v in subdomains):
                self.ptr = np.ascontiguousarray(subdomains[0], dtype=np.int64)
                self.idx = np.ascontiguousarray(subdomains[1], dtype=np.int64)
            else:
                sets = [np.asarray(g, dtype=np.int64).ravel() for g in subdomains]
                self.ptr = np.zeros(len(sets) + 1, dtype=np.int64)
                np.cumsum([len(g) for g in sets], out=self.ptr[1:])
                self.idx = np.concatenate(sets) if sets else np.zeros(0, dtype=np.int64)
            if len(self.ptr) < 1 or int(self.ptr[-1]) != len(self.idx):
                raise KError(102, "AdditiveSchwarz: inconsistent (ptr, idx)")

    def with_sub_ilu(self, mode="ilu0"):
        """Labelled extension: every subdomain is solved with an incomplete factorisation of its submatrix instead of its dense inverse.
        mode "ilu0": textbook ILU(0) on the submatrix's pattern (TrueIlu0); "ilup0": Ilup::new(0) as written (Ilu0).  An integer is passed
        through as the library's sub_mode."""
        self.sub_mode = self._SUB_MODES[mode] if isinstance(mode, str) and mode in self._SUB_MODES else mode
        if isinstance(self.sub_mode, str) or self.sub_mode is None:
            raise KError(102, f"AdditiveSchwarz.with_sub_ilu: unknown mode {mode!r} (\"ilu0\" or \"ilup0\")")
        self.sub_mode = int(self.sub_mode)
        return self

    def with_overlap(self):
        """Labelled extension: grow every subdomain by `overlap` layers before it is inverted."""
        self.variant = self.GROWN
        return self

    def restricted(self):
        """Labelled extension: restricted additive Schwarz (grown subdomains, each row from its last un-grown subdomain only)."""
        self.variant = self.RESTRICTED
        return self

    @staticmethod
    def grid_boxes(N, box=(4, 4, 2)):
        """(ptr, idx) of the boxes of bx x by x bz grid points of the N^3 stencil operators (row = i + N (j + N k)), i fastest, the boxes
        in the same order; boxes at the far faces are shorter when N is not a multiple of the box."""
        bx, by, bz = (int(v) for v in box)
        r = np.arange(N ** 3, dtype=np.int64)
        i, j, k = r % N, (r // N) % N, r // (N * N)
        nx, ny = -(-N // bx), -(-N // by)
        box_of = i // bx + nx * (j // by + ny * (k // bz))
        idx = np.argsort(box_of, kind="stable")             # natural row order inside a box: i fastest, then j, then k
        ptr = np.zeros(nx * ny * -(-N // bz) + 1, dtype=np.int64)
        np.cumsum(np.bincount(box_of, minlength=len(ptr) - 1), out=ptr[1:])
        return ptr, idx.astype(np.int64)

    def setup(self, a):
        h = _ffi.Handle()
        if self.sub_mode is not None and self.ptr is None:
            check(lib().kryst_pc_asm_ilu_uniform(a.h, self.nparts, self.overlap, self.variant, self.sub_mode, C.byref(h)))
        elif self.sub_mode is not None:
            check(lib().kryst_pc_asm_ilu(a.h, self.ptr.ctypes.data_as(_ffi.c_i64p), self.idx.ctypes.data_as(_ffi.c_i64p), len(self.ptr) - 1,
                                         self.overlap, self.variant, self.sub_mode, C.byref(h)))
        elif self.ptr is None:
            check(lib().kryst_pc_asm_uniform(a.h, self.nparts, self.overlap, self.variant, C.byref(h)))
        else:
            check(lib().kryst_pc_asm(a.h, self.ptr.ctypes.data_as(_ffi.c_i64p), self.idx.ctypes.data_as(_ffi.c_i64p), len(self.ptr) - 1,
                                     self.overlap, self.variant, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def info(self):
        """-> dict(nsub, ext_rows = the sum of the (grown) subdomain rows, max_rows); with ILU sub-solves also nnz_l, nnz_u (the kept
        entries strictly below / above the diagonal), max_levels, lds_bytes (per workgroup of the apply), cap, nnz_s (the stored entries of
        the submatrices), layout_entries (the padded level layouts)"""
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        if self.sub_mode is not None:
            v = np.zeros(10, dtype=np.int64)
            check(lib().kryst_pc_asm_ilu_info(self.h, v.ctypes.data_as(_ffi.c_i64p), len(v)))
            keys = ("nsub", "ext_rows", "max_rows", "nnz_l", "nnz_u", "max_levels", "lds_bytes", "cap", "nnz_s", "layout_entries")
            return {k: int(x) for k, x in zip(keys, v)}
        ns, ext, mx = C.c_int64(), C.c_int64(), C.c_int32()
        check(lib().kryst_pc_asm_info(self.h, C.byref(ns), C.byref(ext), C.byref(mx)))
        return {"nsub": ns.value, "ext_rows": ext.value, "max_rows": mx.value}

    def export(self):
        """-> (ptr int64, idx int32, owner int32, tiles float64): the (grown) subdomains sorted ascending, the last un-grown subdomain of
        every row (-1: none), the inverses subdomain after subdomain, column-major inside a tile (tiles[off_k + j b + i] = Binv_k[i][j]).
        With ILU sub-solves -> (ptr, idx, owner, factors): factors[k] = dict(row_ptr int32 (b_k + 1), col int32 (local columns, ascending
        within a row), val float64 (l_ij below the diagonal, u_ij on and above it), lev_l, lev_u int32 (b_k: every row's level, from 1, in
        the forward and in the backward sweep))."""
        inf = self.info()
        if self.sub_mode is not None:
            ns, ext = inf["nsub"], inf["ext_rows"]
            ptr, ent = np.zeros(ns + 1, dtype=np.int64), np.zeros(ns + 1, dtype=np.int64)
            idx, owner = np.zeros(ext, dtype=np.int32), np.zeros(self._a.nrows(), dtype=np.int32)
            rp, col, val = np.zeros(ext + ns, dtype=np.int32), np.zeros(inf["nnz_s"], dtype=np.int32), np.zeros(inf["nnz_s"], dtype=np.float64)
            ll, lu = np.zeros(ext, dtype=np.int32), np.zeros(ext, dtype=np.int32)
            i32 = lambda v: v.ctypes.data_as(_ffi.c_i32p)
            check(lib().kryst_pc_asm_ilu_export(self.h, ptr.ctypes.data_as(_ffi.c_i64p), i32(idx), i32(owner), ent.ctypes.data_as(_ffi.c_i64p),
                                                i32(rp), i32(col), _dp(val), i32(ll), i32(lu)))
            factors = []
            for k in range(ns):
                lo, hi = int(ptr[k]), int(ptr[k + 1])
                factors.append({"row_ptr": rp[lo + k:hi + k + 1].copy() if hi > lo else np.zeros(1, dtype=np.int32),
                                "col": col[ent[k]:ent[k + 1]], "val": val[ent[k]:ent[k + 1]], "lev_l": ll[lo:hi], "lev_u": lu[lo:hi]})
            return ptr, idx, owner, factors
        ptr = np.zeros(inf["nsub"] + 1, dtype=np.int64)
        check(lib().kryst_pc_asm_export(self.h, ptr.ctypes.data_as(_ffi.c_i64p), None, None, None))
        b = np.diff(ptr)
        idx = np.zeros(inf["ext_rows"], dtype=np.int32)
        owner = np.zeros(self._a.nrows(), dtype=np.int32)
        tiles = np.zeros(int((b * b).sum()), dtype=np.float64)
        check(lib().kryst_pc_asm_export(self.h, None, idx.ctypes.data_as(_ffi.c_i32p), owner.ctypes.data_as(_ffi.c_i32p), _dp(tiles)))
        return ptr, idx, owner, tiles


class MatSorType(enum.IntFlag):
    """MatSorType (src/preconditioner/sor.rs:32-44), the reference's bit values."""
    ZERO_INITIAL_GUESS = 0b000_00001
    APPLY_LOWER = 0b000_00010                     # forward Gauss-Seidel
    APPLY_UPPER = 0b000_00100                     # backward
    SYMMETRIC_SWEEP = APPLY_LOWER | APPLY_UPPER
    LOCAL_FORWARD_SWEEP = 0b000_01000
    LOCAL_BACKWARD_SWEEP = 0b000_10000
    LOCAL_SYMMETRIC_SWEEP = LOCAL_FORWARD_SWEEP | LOCAL_BACKWARD_SWEEP
    EISENSTAT = 0b0010_0000


def _rust_float(v):
    """`{}` of an f64 in Rust: the shortest digits that round-trip, no exponent, no trailing ".0" """
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return "NaN" if v != v else ("inf" if v > 0 else "-inf")
    t = repr(v)
    if "e" in t or "E" in t:
        t = np.format_float_positional(v, unique=True, trim="-")
    return t[:-2] if t.endswith(".0") else t


class Sor(_Pc):
    """Sor::new(omega, its, lits, sym, fshift) + setup + apply (src/preconditioner/sor.rs:71-170) as a device preconditioner on the CSR
    operator: inv_diag = 1 / (a_ii + fshift) (ZeroPivot with `.row` where that sum is zero); apply: y = +0.0, then
    `its` times the forward sweep (APPLY_LOWER; no omega in it) and / or the backward sweep (APPLY_UPPER) exactly as written.  `lits` and the
    LOCAL_* / ZERO_INITIAL_GUESS bits are stored and not used, as in the reference.  The parameters are read by setup(): a setter called
    later takes effect at the next setup.  Labelled extension: `.with_colors(colors)` runs the same sweeps in the order (colors[i], i)
    (multicolour Gauss-Seidel; PC::Multicolor has no implementation in the reference)."""

    def __init__(self, omega, its, lits, sym, fshift):
        super().__init__()
        self._omega, self._its, self._lits, self._sym, self._fshift = float(omega), int(its), int(lits), MatSorType(int(sym)), float(fshift)
        self.colors = None

    def set_omega(self, omega): self._omega = float(omega)
    def omega(self): return self._omega
    def set_its(self, its): self._its = int(its)
    def its(self): return self._its
    def set_lits(self, lits): self._lits = int(lits)
    def lits(self): return self._lits
    def set_sym(self, sym): self._sym = MatSorType(int(sym))
    def sym(self): return self._sym
    def set_fshift(self, fshift): self._fshift = float(fshift)
    def fshift(self): return self._fshift

    def __str__(self):                            # sor.rs:91-94; {:?} of a bitflags value: MatSorType(A | B)
        names = [m.name for m in (MatSorType.ZERO_INITIAL_GUESS, MatSorType.APPLY_LOWER, MatSorType.APPLY_UPPER, MatSorType.LOCAL_FORWARD_SWEEP,
                                  MatSorType.LOCAL_BACKWARD_SWEEP, MatSorType.EISENSTAT) if self._sym & m]
        return (f"SOR(omega={_rust_float(self._omega)}, its={self._its}, lits={self._lits}, sym=MatSorType({' | '.join(names) or '0x0'}), "
                f"fshift={_rust_float(self._fshift)})")

    def with_colors(self, colors):
        """Labelled extension: sweep in the order (colors[i], i) ascending (forward) and its exact reverse (backward)."""
        self.colors = None if colors is None else np.ascontiguousarray(np.asarray(colors).ravel(), dtype=np.int64)
        return self

    def setup(self, a):
        c = None
        if self.colors is not None:
            if len(self.colors) != a.nrows():
                raise KError(102, f"Sor: {len(self.colors)} colours for {a.nrows()} rows")
            if len(self.colors) and (self.colors.min() < 0 or self.colors.max() >= 2 ** 31):
                raise KError(102, "Sor: a colour is negative or does not fit 31 bits")
            c = np.ascontiguousarray(self.colors, dtype=np.int32)
        if self._its < 0 or self._lits < 0:
            raise KError(102, "Sor: its and lits are counts")
        h = _ffi.Handle()
        check(lib().kryst_pc_sor(a.h, self._omega, self._its, self._lits, int(self._sym), self._fshift,
                                 c.ctypes.data_as(_ffi.c_i32p) if c is not None else None, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def info(self):
        """-> dict(passes_forward, passes_backward: the dependency levels a sweep walks, one grid barrier between two; rows;
        workgroups_forward, workgroups_backward: the 1024-thread workgroups a sweep launches)"""
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        gf, gb, n, wf, wb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().kryst_pc_sor_info(self.h, C.byref(gf), C.byref(gb), C.byref(n), C.byref(wf), C.byref(wb)))
        return {"passes_forward": gf.value, "passes_backward": gb.value, "rows": n.value, "workgroups_forward": wf.value,
                "workgroups_backward": wb.value}


def color_graph(a):
    """color_graph (src/utils/coloring.rs:57-64) on the stored pattern, on the host (kryst_host_color_graph; no device call): `a` is a
    CsrMatrix (its pattern is downloaded), a (row_ptr, col_idx) pair, or anything with .row_ptr and .col_idx.  -> colors, int64[n]."""
    if isinstance(a, CsrMatrix):
        rp, ci, _ = a.download()
    elif isinstance(a, tuple):
        rp, ci = a
    else:
        rp, ci = a.row_ptr, a.col_idx
    rp = np.ascontiguousarray(rp, dtype=np.int64)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    n = len(rp) - 1
    colors = np.zeros(max(n, 1), dtype=np.int32)
    check(lib().kryst_host_color_graph(n, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), colors.ctypes.data_as(_ffi.c_i32p), None))
    return colors[:n].astype(np.int64)


def build_blocks_from_colors(colors):
    """build_blocks_from_colors (src/utils/coloring.rs:67-74): blocks[c] = the rows of colour c, ascending."""
    colors = np.asarray(colors, dtype=np.int64)
    blocks = [[] for _ in range(int(colors.max()) + 1 if len(colors) else 0)]
    for i, c in enumerate(colors):
        blocks[int(c)].append(i)
    return blocks


class SparsityPattern:
    """SparsityPattern (src/preconditioner/mod.rs) for the SPAI set-up.  `SparsityPattern.Manual(pat)`: pat[j] lists the rows of column j
    of M (n = len(pat)); a list of index lists, or a (ptr, idx) tuple of numpy arrays packed like CSR rows.  `SparsityPattern.Auto`: as
    written, the set-up raises KError(Unsupported) (approxinv.rs:127-133: the downcasts of :301-323 never succeed).
    `SparsityPattern.Operator` (extension): column j of M takes the stored columns of row j of A -- what Auto's code was meant to do."""
    MANUAL, AUTO, OPERATOR = 0, 1, 2

    def __init__(self, kind, ptr=None, idx=None):
        self.kind, self.ptr, self.idx = kind, ptr, idx

    def __repr__(self):
        return {0: "SparsityPattern::Manual", 1: "SparsityPattern::Auto", 2: "SparsityPattern::Operator"}[self.kind]

    @staticmethod
    def Manual(pat):
        if isinstance(pat, tuple) and len(pat) == 2 and all(isinstance(v, np.ndarray) for v in pat):     # (ptr, idx)
            ptr = np.ascontiguousarray(pat[0], dtype=np.int64)
            idx = np.ascontiguousarray(pat[1], dtype=np.int64)
        else:
            cols = [np.asarray(c, dtype=np.int64).ravel() for c in pat]
            ptr = np.zeros(len(cols) + 1, dtype=np.int64)
            np.cumsum([len(c) for c in cols], out=ptr[1:])
            idx = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
        if len(ptr) < 1 or int(ptr[0]) != 0 or int(ptr[-1]) != len(idx):
            raise KError(102, "SparsityPattern.Manual: inconsistent (ptr, idx)")
        return SparsityPattern(SparsityPattern.MANUAL, ptr, idx)


SparsityPattern.Auto = SparsityPattern(SparsityPattern.AUTO)
SparsityPattern.Operator = SparsityPattern(SparsityPattern.OPERATOR)


class Spai(_Pc):
    """ApproxInv::new(pattern, tol, max_iter, nbsteps, max_size, max_new, block_size, cache_size, verbose, sp) + setup(a)
    (src/preconditioner/approxinv.rs:76-264) on the device: column j of M minimises ||A m_j - e_j||_2 over the support J_j of the
    pattern, and inv_rows[i] keeps the (j, M_ij) with |M_ij| > tol, ascending j.  The apply is ApproxInv's (z = M r).  Only `pattern`
    and `tol` are used; the other fields are accepted and ignored, as in the reference.  Labelled deviations: each J_j is sorted; the
    least squares is solved on the reduced problem A[I_j, J_j] (the same minimiser) by Householder QR, so values agree with faer's to
    rounding; errors (ArgumentError for a bad pattern or a non-square operator, FactorError for a rank-deficient or non-finite column,
    Unsupported for a distributed operator or a column over the caps |J_j| <= 64, |I_j| <= 128, 2048 stored entries in A[:, J_j])
    where the reference panics or gives non-finite output.  `export()` returns M as CSR."""

    def __init__(self, pattern, tol, max_iter=0, nbsteps=0, max_size=0, max_new=0, block_size=0, cache_size=0, verbose=False, sp=False):
        super().__init__()
        if not isinstance(pattern, SparsityPattern):
            pattern = SparsityPattern.Manual(pattern)
        self.pattern, self.tol, self.max_iter = pattern, float(tol), max_iter
        self.nbsteps, self.max_size, self.max_new, self.block_size = nbsteps, max_size, max_new, block_size
        self.cache_size, self.verbose, self.sp = cache_size, verbose, sp

    def setup(self, a):
        h = _ffi.Handle()
        p = self.pattern
        if p.kind == SparsityPattern.MANUAL:
            check(lib().kryst_pc_spai(a.h, p.kind, p.ptr.ctypes.data_as(_ffi.c_i64p), p.idx.ctypes.data_as(_ffi.c_i64p), len(p.ptr) - 1,
                                      self.tol, C.byref(h)))
        else:
            check(lib().kryst_pc_spai(a.h, p.kind, None, None, 0, self.tol, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def export(self):
        """M (inv_rows, approxinv.rs:66) as CSR -> (row_ptr int64, col int32, val float64)."""
        if self.h is None:
            raise KError(2, "preconditioner used before setup")
        nnz = C.c_int64()
        check(lib().kryst_pc_spai_export(self.h, C.byref(nnz), None, None, None))
        rp = np.zeros(self._a.nrows() + 1, dtype=np.int64)
        ci = np.zeros(nnz.value, dtype=np.int32)
        va = np.zeros(nnz.value, dtype=np.float64)
        check(lib().kryst_pc_spai_export(self.h, C.byref(nnz), rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va)))
        return rp, ci, va


class Amg(_Pc):
    """AMG::new(a, max_levels, threshold) (src/preconditioner/amg.rs:73-118) as written, with its V-cycle on the device (kryst_pc_amg).
    The set-up runs on the host, quirks included: the adaptive threshold, double-pairwise aggregation, P = rows of (P0 - 0.5 A[:, :nc])
    scaled to unit norm, R = P0^T, A_c = (R A) P.  The apply is apply_recursive (:200-250): one undamped Jacobi sweep before and after
    the coarse correction, the finest level starting from the incoming z (zeros when `apply` makes z), and CG from zero on the coarsest
    level (at most 4096 rows).  The coarse levels fill in: a level over the fill budget raises KError(FactorError).  `info()` and
    `export()` show the hierarchy."""

    def __init__(self, max_levels=10, threshold=0.1):
        super().__init__()
        self.max_levels, self.threshold = int(max_levels), float(threshold)
        self.variant, self.nu_pre, self.nu_post = 0, 1, 1

    def with_textbook(self, theta=0.0):
        """LABELLED EXTENSION (not in the reference): textbook smoothed aggregation, set up on the device (kryst_pc_amg variant 1).
        Strength |a_ij| > theta sqrt(|a_ii a_jj|); aggregates by distance-2 MIS with hashed priorities; P = (I - 4/(3 rho) D^-1 A) P0 with
        rho the Gershgorin bound of D^-1 A; R = P^T; A_c = R (A P); coarsening stops at <= 64 rows, max_levels levels or n_c > 0.8 n; block
        Jacobi of 64 rows on the coarsest level; damped Jacobi (omega = 4/(3 rho)), nu_pre = nu_post = 2, z from zero: M is symmetric."""
        self.variant, self.threshold, self.nu_pre, self.nu_post = 1, float(theta), 2, 2
        return self

    def with_sweeps(self, nu_pre, nu_post):
        self.nu_pre, self.nu_post = int(nu_pre), int(nu_post)
        return self

    def apply(self, r, z=None):
        """As written the finest level starts from the incoming z (amg.rs:211): a host z is uploaded (zeros when z is None)."""
        if z is not None and not isinstance(r, DeviceVec) and self.h is not None:
            rv, zv = DeviceVec(self.ctx, r), DeviceVec(self.ctx, _f64(z))
            check(lib().kryst_pc_apply(self.h, rv.h, zv.h))
            z[:] = zv.to_host()
            return z
        return super().apply(r, z)

    def setup(self, a):
        h = _ffi.Handle()
        check(lib().kryst_pc_amg(a.h, self.max_levels, self.threshold, self.variant, self.nu_pre, self.nu_post, C.byref(h)))
        self._set(a.ctx, h)
        self._a = a
        return self

    def info(self):
        """-> {"levels", "rows", "nnz", "operator_complexity"}: rows and stored entries of A_l per level, sum(nnz) / nnz(A_0)."""
        nl = C.c_int32()
        check(lib().kryst_pc_amg_info(self.h, C.byref(nl), None, None, 0))
        rows = np.zeros(nl.value, dtype=np.int64); nnz = np.zeros(nl.value, dtype=np.int64)
        check(lib().kryst_pc_amg_info(self.h, C.byref(nl), rows.ctypes.data_as(_ffi.c_i64p), nnz.ctypes.data_as(_ffi.c_i64p), nl.value))
        return {"levels": nl.value, "rows": rows.tolist(), "nnz": nnz.tolist(),
                "operator_complexity": float(nnz.sum()) / float(max(nnz[0], 1))}

    def export(self, level, which):
        """which "A", "P", "R" -> (nrows, ncols, row_ptr int64, col int32, val float64) of the device hierarchy; "Dinv" -> D_l^-1 (smoothed
        aggregation: omega D_l^-1, what the sweep multiplies by); "agg" -> the aggregate of every row (smoothed aggregation, not the last level)."""
        w = {"A": 0, "P": 1, "R": 2, "Dinv": 3, "agg": 4}[which]
        nr, nc, nz = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().kryst_pc_amg_export(self.h, level, w, C.byref(nr), C.byref(nc), C.byref(nz), None, None, None))
        if w == 4:
            g = np.zeros(max(nr.value, 1), dtype=np.int32)
            check(lib().kryst_pc_amg_export(self.h, level, w, None, None, None, None, g.ctypes.data_as(_ffi.c_i32p), None))
            return g[:nr.value]
        if w == 3:
            v = np.zeros(max(nr.value, 1))
            check(lib().kryst_pc_amg_export(self.h, level, w, None, None, None, None, None, _dp(v)))
            return v[:nr.value]
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        ci = np.zeros(max(nz.value, 1), dtype=np.int32); va = np.zeros(max(nz.value, 1))
        check(lib().kryst_pc_amg_export(self.h, level, w, None, None, None, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va)))
        return nr.value, nc.value, rp, ci[:nz.value], va[:nz.value]


def apply_chebyshev(a, r, z, alpha, beta, m):
    """apply_chebyshev(a, r, z, alpha, beta, m)  src/preconditioner/chebyshev.rs:83-140."""
    if isinstance(r, DeviceVec):
        check(lib().kryst_apply_chebyshev(a.h, r.h, z.h, alpha, beta, m))
        return z
    rv = DeviceVec(a.ctx, r)
    zv = DeviceVec(a.ctx, len(rv))
    check(lib().kryst_apply_chebyshev(a.h, rv.h, zv.h, alpha, beta, m))
    z[:] = zv.to_host()
    return z


# ----------------------------------------------------------------------------- solvers
class Convergence:
    """Convergence { tol, max_iters }  src/utils/convergence.rs:4-7."""

    def __init__(self, tol, max_iters):
        self.tol, self.max_iters = tol, max_iters


class SolveStats:
    """SolveStats { iterations, final_residual, converged }  src/utils/convergence.rs:10-14."""

    def __init__(self, iterations, final_residual, converged):
        self.iterations, self.final_residual, self.converged = iterations, final_residual, converged

    def __repr__(self):
        return (f"SolveStats {{ iterations: {self.iterations}, final_residual: {self.final_residual:e}, "
                f"converged: {self.converged} }}")


class CgNormType(enum.IntEnum):                  # src/solver/cg.rs:35
    Preconditioned = 0
    Unpreconditioned = 1
    Natural = 2
    NoNorm = 3


class Preconditioning(enum.IntEnum):             # src/solver/gmres.rs:28-32
    NoPc = 0
    Left = 1
    Right = 2
    LeftTextbook = 3                             # LABELLED EXTENSION (not in the reference): Arnoldi on M^-1 A from M^-1 r0, Gram-Schmidt against V --
                                                 # the reference's Left orthogonalises against an un-normalised Z[0] (gmres.rs:240-247, 279-307)


class _Solver:
    _HOST = _DEV = None
    _HIST_PER_ITER = 1

    def __init__(self, tol, max_iters):
        self.conv = Convergence(tol, max_iters)
        self.norm_type = CgNormType.Unpreconditioned
        self.single_reduction = False
        self.radius = None
        self.obj_target = None
        self.monitor = None
        self.residual_history = []
        self.residual_histories = []                 # solve_many: one history per column
        self.restart = 0
        self.preconditioning = Preconditioning.Left
        self.check_every = 0

    def _params(self):
        return _ffi.Params(self.conv.tol, self.conv.max_iters, self.restart, int(self.preconditioning),
                           int(self.norm_type), int(self.single_reduction),
                           int(self.radius is not None), self.radius or 0.0,
                           int(self.obj_target is not None), self.obj_target or 0.0, self.check_every)

    def solve(self, a, pc, b, x):
        """LinearSolver::solve(&mut self, a, pc: Option<&dyn Preconditioner>, b, x) -> Result<SolveStats, KError>
        (src/solver/mod.rs:43-49).  x is in/out.  Host arrays are uploaded / downloaded around the device solve;
        DeviceVec arguments stay in HBM."""
        prm = self._params()
        st = _ffi.Stats()
        cap = min(self._HIST_PER_ITER * self.conv.max_iters + max(self.restart, 1) + 8, (1 << 22) + 8)   # the library records at most 2^22 entries
        hist = np.zeros(cap)
        hlen = C.c_int64(0)
        cb = _ffi.MONITOR(lambda it, res, _u: self.monitor(it, res)) if self.monitor else _ffi.MONITOR()
        pch = pc.h if pc is not None else None
        if pc is not None and pch is None:
            raise KError(2, "preconditioner used before setup")
        tail = self._extra() + (a.h, pch, C.byref(prm), C.byref(st), _dp(hist), cap, C.byref(hlen), cb, None)
        if isinstance(b, DeviceVec):
            rc = getattr(lib(), self._DEV)(b.h, x.h, *tail)
        elif self._HOST is None:                     # extension solvers only exist in device-vector form
            bv, xv = DeviceVec(a.ctx, b), DeviceVec(a.ctx, x)
            rc = getattr(lib(), self._DEV)(bv.h, xv.h, *tail)
            if rc == 0:
                x[:] = xv.to_host()
        else:
            bb = _f64(b)
            if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
                raise KError(102, "x must be a contiguous float64 numpy array (it is written in place)")
            if len(bb) != len(x):
                raise KError(102, "b and x differ in length")
            rc = getattr(lib(), self._HOST)(_dp(bb), _dp(x), len(bb), *tail)
        self.residual_history.extend(hist[:min(hlen.value, cap)].tolist())
        stats = SolveStats(st.iterations, st.final_residual, bool(st.converged))
        check(rc, stats)
        return stats

    _MULTI_DEV = None

    def _solve_group(self, a, pch, bm, xm):
        """one multivector of 2, 4 or 8 columns through the batched entry point -> per column (code, SolveStats, history)"""
        k = bm.k
        prm = self._params()
        st = (_ffi.Stats * k)()
        code = (C.c_int32 * k)()
        cap = min(self.conv.max_iters + 8, (1 << 19) + 8)          # the library records at most 2^19 entries per column
        hist = np.zeros((k, cap))
        hlen = (C.c_int64 * k)()
        check(getattr(lib(), self._MULTI_DEV)(bm.h, xm.h, a.h, pch, C.byref(prm), st, code, _dp(hist), cap, hlen))
        return [(code[j], SolveStats(st[j].iterations, st[j].final_residual, bool(st[j].converged)), hist[j, :min(hlen[j], cap)].tolist())
                for j in range(k)]

    def solve_many(self, a, pc, B, X):
        """solve(a, pc, B[:, j], X[:, j]) for every column j, the matrix read once per group of columns: bit for bit the results of the
        single calls.  B, X: MultiVec (2, 4 or 8 columns, X in/out on the device) or arrays of shape (n, m) with any m -- the columns are
        cut by split_widths into groups of 8, 4 and 2, a leftover single column goes through solve(); X must then be a float64 array and
        is written in place, column by column, where the column's solve succeeded.  Returns a list with a SolveStats or, for a column
        that ended in an error, the KError (carrying .stats) in its place; self.residual_histories holds one history per column."""
        if self._MULTI_DEV is None:
            raise KError(6, "solve_many: CG and PCG only")
        return self._solve_columns(a, pc, B, X, "solve_many", lambda _pc: self)

    def _solve_columns(self, a, pc, B, X, what, single):
        """the body of solve_many and BlockCgSolver.solve_block: groups of 8, 4 and 2 columns through _solve_group, a leftover column through
        single(pc).solve; a column of X is written where its code is 0 (block CG reports one code for a whole group)"""
        pch = pc.h if pc is not None else None
        if pc is not None and pch is None:
            raise KError(2, "preconditioner used before setup")
        if isinstance(B, MultiVec) or isinstance(X, MultiVec):
            if not (isinstance(B, MultiVec) and isinstance(X, MultiVec)):
                raise KError(102, f"{what}: B and X must both be MultiVec or both be arrays")
            res = self._solve_group(a, pch, B, X)
        else:
            ba = np.asarray(B, dtype=np.float64)
            if ba.ndim != 2 or not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.shape != ba.shape:
                raise KError(102, f"{what}: B and X must be float64 arrays of the same shape (n, m)")
            res, at = [], 0
            for w in split_widths(ba.shape[1]):
                if w == 1:
                    one = single(pc)
                    saved, one.residual_history = one.residual_history, []
                    xj = np.ascontiguousarray(X[:, at])
                    try:
                        stats = one.solve(a, pc, np.ascontiguousarray(ba[:, at]), xj)
                        res.append((0, stats, one.residual_history))
                        X[:, at] = xj
                    except KError as e:
                        if e.stats is None:
                            raise
                        res.append((e.code, e.stats, one.residual_history))
                    finally:
                        one.residual_history = saved
                else:
                    bm = MultiVec.from_numpy(ba[:, at:at + w], ctx=a.ctx)
                    xm = MultiVec.from_numpy(X[:, at:at + w], ctx=a.ctx)
                    group = self._solve_group(a, pch, bm, xm)
                    xs = xm.to_numpy()
                    for j, (code, _, _) in enumerate(group):
                        if code == 0:
                            X[:, at + j] = xs[:, j]
                    res.extend(group)
                at += w
        self.residual_histories = [h for _, _, h in res]
        return [stats if code == 0 else KError(code, "", stats) for code, stats, _ in res]

    def _extra(self):
        return ()

    def clear_history(self):
        self.residual_history.clear()

    # builder methods (cg.rs:64-88)
    def with_norm(self, norm_type):
        self.norm_type = norm_type
        return self

    def with_single_reduction(self, flag):
        self.single_reduction = flag
        return self

    def with_radius(self, radius):
        self.radius = radius
        return self

    def with_obj_target(self, obj):
        self.obj_target = obj
        return self

    def with_monitor(self, f):
        self.monitor = f
        return self


class CgSolver(_Solver):
    """CgSolver::new(tol, max_iters)  src/solver/cg.rs:40-93,114-288 (pc is ignored, cg.rs:115)."""
    _HOST, _DEV = "kryst_cg_solve", "kryst_cg_solve_dev"
    _MULTI_DEV = "kryst_cg_solve_multi_dev"


class PcgSolver(_Solver):
    """PcgSolver::new(tol, max_iters)  src/solver/pcg.rs:31-91,114-222."""
    _HOST, _DEV = "kryst_pcg_solve", "kryst_pcg_solve_dev"
    _MULTI_DEV = "kryst_pcg_solve_multi_dev"


class BlockCgSolver(_Solver):
    """Block CG (kryst_bcg_solve_multi_dev; an extension beside solve_many): ONE Krylov space for the columns of a block, so that K right-hand
    sides can take fewer iterations than K solves.  Dubrulle's retooled block CG with a Cholesky-QR of a K x K Gram matrix; pc may be None,
    IdentityPc or Jacobi.  The columns of a block are not independent: a breakdown (dependent or zero right-hand sides, an indefinite matrix or
    preconditioner) ends the whole block with one code and leaves its X untouched -- for right-hand sides that may be dependent use solve_many."""
    _MULTI_DEV = "kryst_bcg_solve_multi_dev"

    def solve(self, a, pc, b, x):
        raise KError(6, "BlockCgSolver: solve_block only (a single right-hand side goes through CgSolver / PcgSolver)")

    def solve_many(self, a, pc, B, X):
        raise KError(6, "BlockCgSolver: solve_block only")

    def solve_block(self, a, pc, B, X):
        """B, X: MultiVec (2, 4 or 8 columns: one block, X in/out on the device) or float64 arrays of shape (n, m) with any m -- the columns are cut
        by split_widths, each group of 8, 4 or 2 is one block, a leftover single column goes through CgSolver (pc None) or PcgSolver; X is
        written in place where the block's solve succeeded.  Returns what solve_many returns: per column a SolveStats or, after an error, the
        KError (carrying .stats) in its place; self.residual_histories holds one history per column."""
        def single(pc_):
            one = (CgSolver if pc_ is None else PcgSolver)(self.conv.tol, self.conv.max_iters)
            one.check_every = self.check_every
            return one
        return self._solve_columns(a, pc, B, X, "solve_block", single)


def mvec_gram(u, v, inv_diag=None):
    """Test hook (kryst_bench_mvec_gram): the K x K Gram matrix of the multivectors u against v as block CG reduces it -- entry (a, b), a <= b, is
    the library's inner product over u(i, a) * v(i, b), or u(i, a) * (d_i * v(i, b)) with weights inv_diag (a DeviceVec); the lower triangle
    mirrors the upper."""
    out = np.zeros((u.k, u.k))
    check(lib().kryst_bench_mvec_gram(u.h, v.h, inv_diag.h if inv_diag is not None else None, _dp(out)))
    return out


def host_bcg_step(step, g, c=None):
    """kryst_host_bcg_step: one K x K scalar step of block CG on the host (no GPU).  step 0 (start), 1 (after the Gram matrix of S against T) or
    2 (after the Gram matrix of the new Q); g the Gram matrix, c the residual factor C (steps 1 and 2).  Returns (code, c, out1, out2, res) as the
    header describes them; after a breakdown code != 0 and the matrices hold whatever the step had written."""
    g = np.ascontiguousarray(g, dtype=np.float64)
    k = g.shape[0]
    cc = np.zeros((k, k)) if c is None else np.array(c, dtype=np.float64, order="C")
    o1, o2, res = np.zeros((k, k)), np.zeros((k, k)), np.zeros(k)
    code = lib().kryst_host_bcg_step(int(step), k, _dp(g), _dp(cc), _dp(o1), _dp(o2), _dp(res))
    if code == 102:
        check(code)
    return code, cc, o1, o2, res


class _Solver32(_Solver):
    """CG / PCG on fp32-stored vectors and a lowered operator (an extension; fp64 arithmetic, scalars and exits).  solve(a32, pc, b, x):
    a32 a CsrMatrix32; b, x DeviceVec32 (x in/out on the device) or arrays (x a float32 array written in place on success)."""
    _DEV32 = None

    def solve(self, a, pc, b, x):
        prm = self._params()
        st = _ffi.Stats()
        cap = min(self.conv.max_iters + 8, (1 << 22) + 8)
        hist = np.zeros(cap)
        hlen = C.c_int64(0)
        pch = pc.h if pc is not None else None
        if pc is not None and pch is None:
            raise KError(2, "preconditioner used before setup")
        host = not isinstance(b, DeviceVec32)
        if host:
            if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous):
                raise KError(102, "x must be a contiguous float32 numpy array (it is written in place)")
        bv = DeviceVec32(a.ctx, b) if host else b
        xv = DeviceVec32(a.ctx, x) if host else x
        rc = getattr(lib(), self._DEV32)(bv.h, xv.h, a.h, pch, C.byref(prm), C.byref(st), _dp(hist), cap, C.byref(hlen))
        if host and rc == 0:
            x[:] = xv.to_host()
        self.residual_history.extend(hist[:min(hlen.value, cap)].tolist())
        stats = SolveStats(st.iterations, st.final_residual, bool(st.converged))
        check(rc, stats)
        return stats


class Cg32Solver(_Solver32):
    """CgSolver::new(tol, max_iters) on fp32 storage (kryst_cg32_solve_dev; pc is ignored, cg.rs:115)."""
    _DEV32 = "kryst_cg32_solve_dev"


class Pcg32Solver(_Solver32):
    """PcgSolver::new(tol, max_iters) on fp32 storage (kryst_pcg32_solve_dev; pc: None, IdentityPc or Jacobi)."""
    _DEV32 = "kryst_pcg32_solve_dev"


class RefinementSolver:
    """fp64 iterative refinement around CG (pc None / Identity) or Jacobi-PCG on the fp32-stored operator (kryst_refine_solve_dev; an
    extension).  RefinementSolver(tol, max_outer).with_inner(tol, max_iters); solve(a, pc, b, x) lowers `a` on first use and keeps the
    lowered operator per operator object; the SolveStats it returns carries .inner_iterations (one count per outer step taken)."""

    def __init__(self, tol, max_outer):
        self.conv = Convergence(tol, max_outer)
        self.inner = Convergence(1e-6, 1000)
        self.residual_history = []
        self._lowered = {}
        self.form = "plain"

    def with_inner(self, tol, max_iters):
        self.inner = Convergence(tol, max_iters)
        return self

    def with_form(self, form):
        """How lowered(a) lowers: "plain" (the default), "auto", "pattern" or "dia" (CsrMatrix.lower)."""
        CsrMatrix32.form_code(form)
        if form != self.form:
            self._lowered = {}
        self.form = form
        return self

    def clear_history(self):
        self.residual_history.clear()

    def lowered(self, a):
        key = id(a)
        hit = self._lowered.get(key)
        if hit is None or hit[0] is not a:
            hit = (a, a.lower(self.form))
            self._lowered[key] = hit
        return hit[1]

    def solve(self, a, pc, b, x):
        pch = pc.h if pc is not None else None
        if pc is not None and pch is None:
            raise KError(2, "preconditioner used before setup")
        a32 = self.lowered(a)
        un = int(CgNormType.Unpreconditioned)
        po = _ffi.Params(self.conv.tol, self.conv.max_iters, 0, 0, un, 0, 0, 0.0, 0, 0.0, 0)
        pi = _ffi.Params(self.inner.tol, self.inner.max_iters, 0, 0, un, 0, 0, 0.0, 0, 0.0, 0)
        st = _ffi.Stats()
        steps = min(max(int(self.conv.max_iters), 0), 1 << 20)      # outer steps recorded (the count of residuals still runs on)
        cap = steps + 2
        hist = np.zeros(cap)
        hlen = C.c_int64(0)
        inner = np.full(max(steps, 1), -1, dtype=np.int64)
        host = not isinstance(b, DeviceVec)
        if host and not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise KError(102, "x must be a contiguous float64 numpy array (it is written in place)")
        bv = DeviceVec(a.ctx, b) if host else b
        xv = DeviceVec(a.ctx, x) if host else x
        rc = lib().kryst_refine_solve_dev(bv.h, xv.h, a.h, a32.h, pch, C.byref(po), C.byref(pi), C.byref(st), _dp(hist), cap,
                                          C.byref(hlen), inner.ctypes.data_as(_ffi.c_i64p), steps)
        if host and rc == 0:
            x[:] = xv.to_host()
        pushed = min(hlen.value, cap)
        self.residual_history.extend(hist[:pushed].tolist())
        stats = SolveStats(st.iterations, st.final_residual, bool(st.converged))
        stats.inner_iterations = inner[inner >= 0].tolist()        # one count per inner solve that ran (its last one may have ended in an error)
        check(rc, stats)
        return stats


class GmresSolver(_Solver):
    """GmresSolver::new(restart, tol, max_iters)  src/solver/gmres.rs:38-60,216-402."""
    _HOST, _DEV = "kryst_gmres_solve", "kryst_gmres_solve_dev"

    def __init__(self, restart, tol, max_iters):
        super().__init__(tol, max_iters)
        self.restart = restart

    def with_preconditioning(self, mode):
        self.preconditioning = mode
        return self


class Orthog(enum.IntEnum):                      # src/solver/fgmres.rs:26-31
    Classical = 0
    Modified = 1


class FgmresSolver(_Solver):
    """FgmresSolver::new(tol, max_iters, restart)  src/solver/fgmres.rs:33-101; solve_flex :114-340.  The flexible
    preconditioner is any device preconditioner object (its action is fixed per apply, which FGMRES permits);
    `solve` forwards to solve_flex so the solver also fits the LinearSolver call shape used elsewhere."""
    _HOST, _DEV = "kryst_fgmres_solve", "kryst_fgmres_solve_dev"

    def __init__(self, tol, max_iters, restart):
        super().__init__(tol, max_iters)
        self.restart = restart
        self.orthog = Orthog.Classical
        self.haptol = 1e-12
        self.preallocate = False
        self.delta_allocate = 10                     # accepted, no effect (allocation granularity, fgmres.rs:77-80)

    def _extra(self):
        return (int(self.orthog), float(self.haptol), int(self.preallocate))

    def with_orthog(self, orthog):
        self.orthog = orthog
        return self

    def with_preallocate(self, flag):
        self.preallocate = flag
        return self

    def with_delta_allocate(self, delta):
        self.delta_allocate = delta
        return self

    def with_haptol(self, haptol):
        self.haptol = haptol
        return self

    def solve_flex(self, a, pc, b, x):
        return self.solve(a, pc, b, x)


class PcaGmresSolver(_Solver):
    """PcaGmresSolver::new(restart, pipeline_depth, block_size, tol, max_iters)  src/solver/pca_gmres.rs:54-76,99-312 as written:
    x starts from zero, no orthogonalisation (the power basis of the default features), Right = M^-1 A with the update in V, the
    stopping block's column left out of the update, converged from the true residual.  Only blocks of one vector run: block_size >= 2
    with restart >= 2 (where the reference panics), block_size = 0 or restart = 0 raise KError(ERR_ARG).  pipeline_depth and tau are
    accepted and never read.  with_textbook() selects the labelled extension: s-step GMRES(restart) from x0, right preconditioned,
    block_size = s in 1..16 (BCGS2 + CholQR2; device form only)."""
    _HOST, _DEV = "kryst_pca_gmres_solve", "kryst_pca_gmres_solve_dev"

    def __init__(self, restart, pipeline_depth, block_size, tol, max_iters):
        super().__init__(tol, max_iters)
        self.restart = restart
        self.pipeline_depth = pipeline_depth
        self.block_size = block_size
        self.tau = None
        self.preconditioning = Preconditioning.Left          # pca_gmres.rs:61

    def _extra(self):
        return (int(self.block_size), int(self.pipeline_depth), float(self.tau) if self.tau is not None else 0.0)

    def with_preconditioning(self, mode):
        self.preconditioning = mode
        return self

    def with_tau(self, tau):
        self.tau = tau
        return self

    def with_textbook(self):
        self._HOST, self._DEV = None, "kryst_pca_gmres_textbook_solve_dev"
        return self


class CbGmresSolver(_Solver):
    """LABELLED EXTENSION (not in the reference): GMRES(restart) whose Krylov basis is stored in fp32 -- rounded once
    when a basis vector is stored, widened exactly at every use -- while the operator, the preconditioner, x, the Hessenberg matrix and all
    arithmetic stay fp64 and the true residual is recomputed in fp64 at every restart.  with_basis("f64") is the control: the same loop with
    nothing rounded (NoPc: the bits of GmresSolver).  NoPc, or Right in its textbook form (Arnoldi on A M^-1 from the true residual, only V
    kept, x += M^-1 (sum y_j V_j) once per cycle); Left and LeftTextbook raise KError(UNSUPPORTED).  One GPU; device form only."""
    _HOST, _DEV = None, "kryst_cbgmres_solve_dev"
    BASES = {"f64": 0, "f32": 1}

    def __init__(self, restart, tol, max_iters):
        super().__init__(tol, max_iters)
        self.restart = restart
        self.basis = "f32"
        self.preconditioning = Preconditioning.Right

    def _extra(self):
        return (int(self.BASES.get(self.basis, self.basis)),)

    def with_basis(self, basis):
        self.basis = basis
        return self

    def with_preconditioning(self, mode):
        self.preconditioning = mode
        return self


class BiCgStabSolver(_Solver):
    """BiCgStabSolver::new(tol, max_iters)  src/solver/bicgstab.rs:36-48,69-293 (pc ignored, absolute tolerance)."""
    _HOST, _DEV = "kryst_bicgstab_solve", "kryst_bicgstab_solve_dev"


class CgsSolver(_Solver):
    """CgsSolver::new(tol, max_iters)  src/solver/cgs.rs:21-35,58-135 (pc ignored, :59)."""
    _HOST, _DEV = "kryst_cgs_solve", "kryst_cgs_solve_dev"


class TfqmrSolver(_Solver):
    """TfqmrSolver::new(tol, max_iters)  src/solver/tfqmr.rs:30-40,64-221 as written (pc ignored, x starts from zero whatever
    the caller passes, :72).  residual_history receives the residual estimate of both substeps."""
    _HOST, _DEV = "kryst_tfqmr_solve", "kryst_tfqmr_solve_dev"
    _HIST_PER_ITER = 2


class MinresSolver(_Solver):
    """MinresSolver::new(tol, max_iters)  src/solver/minres.rs:60-219 as written (pc ignored, :61): x0 enters r0 only, x_out starts
    from zero, x = x_best (the iterate of the smallest estimate), final_residual = phi_min.  Its estimate is not the true residual.
    with_textbook() selects the labelled extension: Paige-Saunders MINRES from x0, last iterate (device form only)."""
    _HOST, _DEV = "kryst_minres_solve", "kryst_minres_solve_dev"

    def with_textbook(self):
        self._HOST, self._DEV = None, "kryst_minres_textbook_solve_dev"
        return self


class QmrSolver(_Solver):
    """QmrSolver::new(tol, max_iters)  src/solver/qmr.rs:61-166 as written (pc ignored): a BiCGStab-type loop stopping on ||b - A x_j||."""
    _HOST, _DEV = "kryst_qmr_solve", "kryst_qmr_solve_dev"


class CgnrSolver(_Solver):
    """CgnrSolver::new(tol, max_iters)  src/solver/cgnr.rs:77-132 as written (pc ignored, A where A^T is meant, ||A(Ap)||^2 as the
    denominator).  with_textbook() selects the labelled extension: CGNR (Saad section 8.3) with the operator's cached A^T (device form only)."""
    _HOST, _DEV = "kryst_cgnr_solve", "kryst_cgnr_solve_dev"

    def with_textbook(self):
        self._HOST, self._DEV = None, "kryst_cgnr_textbook_solve_dev"
        return self


class CgneSolver(CgnrSolver):
    """CgneSolver::new(tol, max_iters)  src/solver/cgnr.rs:153-208: the same floating-point operations as CgnrSolver, the same path."""

    def with_textbook(self):
        raise KError(6, "CgneSolver has no textbook form")


class BiCgStabRightPcSolver(_Solver):
    """Extension: right-preconditioned BiCGStab (device vectors only)."""
    _HOST, _DEV = None, "kryst_bicgstab_rpc_solve_dev"


class DenseMatrix(_Owned):
    """DenseMatrix<f64> (src/matrix/dense.rs) living on the GPU, column-major; implements MatVec (core/wrappers.rs:27-38)."""
    _DESTROY, _CLOSE_ORDER = "kryst_dense_destroy", 3

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        ctx._adopt(self)
        nr, nc = C.c_int64(), C.c_int64()
        check(lib().kryst_dense_shape(self.h, C.byref(nr), C.byref(nc)))
        self._nrows, self._ncols = nr.value, nc.value

    @staticmethod
    def from_raw(nrows, ncols, data, ctx=None):
        """DenseMatrix::from_raw(nrows, ncols, data) (dense.rs:16-25): data column-major, data[i + j * nrows]."""
        ctx = ctx or Context.default()
        d = _f64(data).ravel()
        if len(d) != nrows * ncols:
            raise KError(102, "from_raw: data length differs from nrows * ncols")
        h = _ffi.Handle()
        check(lib().kryst_dense_create(ctx.h, nrows, ncols, _dp(d), 1, C.byref(h)))
        return DenseMatrix(ctx, h)

    @staticmethod
    def from_numpy(a, ctx=None):
        """A 2-D array a[i, j] (extension)."""
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2:
            raise KError(102, "from_numpy: a 2-D array is required")
        return DenseMatrix.from_raw(a.shape[0], a.shape[1], np.asfortranarray(a).ravel(order="F"), ctx=ctx)

    @staticmethod
    def from_csr(a):
        """The CsrMatrix densified on the device, absent entries +0.0 (extension)."""
        h = _ffi.Handle()
        check(lib().kryst_dense_from_csr(a.h, C.byref(h)))
        return DenseMatrix(a.ctx, h)

    def nrows(self):
        return self._nrows

    def ncols(self):
        return self._ncols

    @property
    def shape(self):
        return (self._nrows, self._ncols)

    def to_numpy(self):
        out = np.empty(self._nrows * self._ncols)
        check(lib().kryst_dense_download(self.h, _dp(out)))
        return out.reshape((self._nrows, self._ncols), order="F")

    def matvec(self, x, y=None):
        """MatVec::matvec(&self, x, y) (core/wrappers.rs:27-38): y = A x.  Host arrays in -> host array out; DeviceVec in -> DeviceVec."""
        if isinstance(x, DeviceVec):
            y = y if y is not None else DeviceVec(self.ctx, self._nrows)
            check(lib().kryst_dense_matvec(self.h, x.h, y.h))
            return y
        xv, yv = DeviceVec(self.ctx, _f64(x)), DeviceVec(self.ctx, self._nrows)
        check(lib().kryst_dense_matvec(self.h, xv.h, yv.h))
        out = yv.to_host()
        if y is not None:
            y[:] = out
            return y
        return out


def _direct_solve(host_fn, dev_fn, head, a, pc, b, x):
    """The call shape shared by LuSolver::solve and QrSolver::solve: pc is accepted and ignored (direct_lu.rs:70, :123)."""
    st = _ffi.Stats()
    pch = pc.h if pc is not None else None
    if isinstance(b, DeviceVec):
        rc = dev_fn(*head, a.h, pch, b.h, x.h, C.byref(st))
    else:
        bb = _f64(b)
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise KError(102, "x must be a contiguous float64 numpy array (it is written in place)")
        if len(bb) != len(x):
            raise KError(102, "b and x differ in length")
        rc = host_fn(*head, a.h, pch, _dp(bb), _dp(x), len(bb), C.byref(st))
    stats = SolveStats(st.iterations, st.final_residual, bool(st.converged))
    check(rc, stats)
    return stats


class LuSolver(_Owned):
    """LuSolver (src/solver/direct_lu.rs:14-90) on a DenseMatrix: LU with full pivoting in the operation order of DESIGN.md section 4.12
    (a labelled deviation from faer's FullPivLu)."""
    _DESTROY, _CLOSE_ORDER = "kryst_lu_destroy", 3

    def __init__(self, ctx=None):
        self.ctx = ctx or Context.default()
        self.h = _ffi.Handle()
        check(lib().kryst_lu_create(self.ctx.h, C.byref(self.h)))
        self.ctx._adopt(self)

    def solve(self, a, pc, b, x):
        """LinearSolver::solve (direct_lu.rs:64-90): factor, cache, solve.  b is x is allowed for DeviceVec arguments."""
        return _direct_solve(lib().kryst_lu_solve, lib().kryst_lu_solve_dev, (self.h,), a, pc, b, x)

    def solve_cached(self, b, x=None):
        """solve_cached (direct_lu.rs:34-43) with the cached factors; KError(SolveError) when there are none (the reference panics)."""
        if isinstance(b, DeviceVec):
            x = x if x is not None else DeviceVec(self.ctx, len(b))
            check(lib().kryst_lu_solve_cached(self.h, b.h, x.h))
            return x
        bv = DeviceVec(self.ctx, _f64(b))
        check(lib().kryst_lu_solve_cached(self.h, bv.h, bv.h))
        out = bv.to_host()
        if x is not None:
            x[:] = out
            return x
        return out

    def info(self):
        v = (C.c_int64 * 4)()
        check(lib().kryst_lu_info(self.h, v, 4))
        return {"cap": v[0], "tail": v[1], "tile": v[2], "n": v[3]}

    def factors(self):
        """-> (row_perm, col_perm, factors): P A Q = L U with (P A Q)[i, j] = A[row_perm[i], col_perm[j]], L strictly below the diagonal of
        `factors` (unit diagonal implied), U on and above it."""
        n = self.info()["n"]
        if n < 0:
            raise KError(2, "factors: no factorization is cached")
        rp = np.zeros(max(n, 1), dtype=np.int64); cp = np.zeros(max(n, 1), dtype=np.int64); f = np.zeros(max(n * n, 1))
        check(lib().kryst_lu_export(self.h, n, rp.ctypes.data_as(_ffi.c_i64p), cp.ctypes.data_as(_ffi.c_i64p), _dp(f)))
        return rp[:n], cp[:n], f[:n * n].reshape((n, n), order="F")


class QrSolver:
    """QrSolver (src/solver/direct_lu.rs:96-146) on a square DenseMatrix: Householder QR in the operation order of DESIGN.md section 4.12."""

    def solve(self, a, pc, b, x):
        return _direct_solve(lib().kryst_qr_solve, lib().kryst_qr_solve_dev, (), a, pc, b, x)


def _colmajor(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise KError(102, "a 2-D array is required")
    return a.shape[0], a.shape[1], np.asfortranarray(a).ravel(order="F")


def host_dense_lu(a):
    """LU with full pivoting on the host, no GPU (kryst_host_dense_lu): the bits of LuSolver.  -> (row_perm, col_perm, factors)."""
    nr, nc, d = _colmajor(a)
    rp = np.zeros(max(nr, 1), dtype=np.int64); cp = np.zeros(max(nr, 1), dtype=np.int64); f = np.zeros(max(nr * nr, 1))
    check(lib().kryst_host_dense_lu(nr, nc, _dp(d), rp.ctypes.data_as(_ffi.c_i64p), cp.ctypes.data_as(_ffi.c_i64p), _dp(f)))
    return rp[:nr], cp[:nr], f[:nr * nr].reshape((nr, nr), order="F")


def host_dense_lu_solve(row_perm, col_perm, factors, b, x=None):
    """The two column sweeps of LuSolver on the host (kryst_host_dense_lu_solve) -> x."""
    rp = np.ascontiguousarray(row_perm, dtype=np.int64); cp = np.ascontiguousarray(col_perm, dtype=np.int64)
    n, _, f = _colmajor(factors)
    bb = _f64(b)
    if len(bb) != n or len(rp) != n or len(cp) != n:
        raise KError(102, "host_dense_lu_solve: lengths differ")
    x = np.empty(n) if x is None else x
    check(lib().kryst_host_dense_lu_solve(n, rp.ctypes.data_as(_ffi.c_i64p), cp.ctypes.data_as(_ffi.c_i64p), _dp(f), _dp(bb), _dp(x)))
    return x


def host_dense_qr_solve(a, b, x=None):
    """Householder QR solve on the host (kryst_host_dense_qr_solve): the bits of QrSolver.  x (if given) is untouched on an error."""
    nr, nc, d = _colmajor(a)
    bb = _f64(b)
    if len(bb) != nr:
        raise KError(102, "host_dense_qr_solve: b has the wrong length")
    x = np.empty(nr) if x is None else x
    check(lib().kryst_host_dense_qr_solve(nr, nc, _dp(d), _dp(bb), _dp(x)))
    return x


class PC:
    """PC<T> (src/context/pc_context.rs:36-76): the reference's configuration enum for preconditioners, plus the constructor it
    lacks -- `PC.Ilut(fill=10, droptol=1e-3).build(a)` returns the set-up device preconditioner.  PC::AMG carries no parameters in
    the reference; `PC.AMG()` builds Amg(max_levels=10, threshold=0.1), the as-written hierarchy (a bare `PC("AMG")` without them
    still raises KError(Unsupported), as it did before AMG existed).  `PC.AdditiveSchwarz(overlap=0, subdomains=None, nparts=None)`
    builds AdditiveSchwarz as written; a bare `PC("AdditiveSchwarz")` without its parameters keeps raising KError(Unsupported), following
    AMG.  `PC.Ssor(omega=1.0, its=1)` builds Sor(omega, its, 1, SYMMETRIC_SWEEP, 0.0) and `PC.Multicolor(colors)` the same sweeps in the
    coloured order (labelled extension); the bare `PC("Ssor")` / `PC("Multicolor")` keep raising KError(Unsupported), following AMG.
    `PC.ChebyshevPoly(degree, ...)` builds ChebyshevPoly, the polynomial preconditioner (labelled extension); `PC.Chebyshev` stays the
    reference's stub."""

    def __init__(self, kind, **params):
        self.kind, self.params = kind, params

    def __repr__(self):
        return f"PC::{self.kind}{self.params or ''}"

    @staticmethod
    def Jacobi():
        return PC("Jacobi")

    @staticmethod
    def Ilu0():
        return PC("Ilu0")

    @staticmethod
    def Ilup(fill):
        return PC("Ilup", fill=fill)

    @staticmethod
    def Ilut(fill, droptol):
        return PC("Ilut", fill=fill, droptol=droptol)

    @staticmethod
    def Chebyshev(degree, emin=None, emax=None):
        return PC("Chebyshev", degree=degree, emin=emin, emax=emax)

    @staticmethod
    def ChebyshevPoly(degree, lambda_min=None, lambda_max=None, jacobi=True, steps=10, ratio=30.0, safety=1.1, seed=0x5EED):   # labelled extension
        return PC("ChebyshevPoly", degree=degree, lambda_min=lambda_min, lambda_max=lambda_max, jacobi=jacobi, steps=steps, ratio=ratio,
                  safety=safety, seed=seed)

    @staticmethod
    def BlockJacobi(blocks):                      # pc_context.rs:67 BlockJacobi { blocks }
        return PC("BlockJacobi", blocks=blocks)

    @staticmethod
    def ApproxInv(pattern, tol, max_iter=0):        # pc_context.rs:63 ApproxInv { pattern, tol, max_iter }
        return PC("ApproxInv", pattern=pattern, tol=tol, max_iter=max_iter)

    @staticmethod
    def AMG(max_levels=10, threshold=0.1):            # pc_context.rs:72 AMG (no parameters there: these are the defaults)
        return PC("AMG", max_levels=max_levels, threshold=threshold)

    @staticmethod
    def AdditiveSchwarz(overlap=0, subdomains=None, nparts=None, sub=None):   # pc_context.rs:75 AdditiveSchwarz (no parameters there); asm.rs:34 new(overlap, subdomains)
        return PC("AdditiveSchwarz", overlap=overlap, subdomains=subdomains, nparts=nparts, sub=sub)   # sub: None (direct), "ilu0" or "ilup0" (labelled extension)

    @staticmethod
    def Ssor(omega=1.0, its=1):                      # pc_context.rs:45 Ssor (no parameters there)
        return PC("Ssor", omega=omega, its=its)

    @staticmethod
    def Multicolor(colors, omega=1.0, its=1):        # pc_context.rs:70 Multicolor { colors }
        return PC("Multicolor", colors=colors, omega=omega, its=its)

    def build(self, a):
        k, q = self.kind, self.params
        if k == "Jacobi":
            return Jacobi().setup(a)
        if k == "Ilu0":
            return Ilu0().setup(a)
        if k == "Ilup":
            return Ilup(q["fill"]).setup(a)
        if k == "Ilut":
            return Ilut(q["fill"], q["droptol"]).setup(a)
        if k == "Chebyshev":                         # the trait object of the reference (apply is the stub of chebyshev.rs:68-70)
            return Chebyshev(q["degree"], q["emin"], q["emax"]).setup(a)
        if k == "ChebyshevPoly":                     # labelled extension: the polynomial preconditioner, bounds estimated where not given
            return ChebyshevPoly(**q).setup(a)
        if k == "BlockJacobi":
            return BlockJacobi(q["blocks"]).setup(a)
        if k == "ApproxInv":
            return Spai(q["pattern"], q["tol"], q["max_iter"]).setup(a)
        if k == "AMG" and "max_levels" in q:          # PC.AMG(...); the bare PC("AMG") keeps raising Unsupported, as before
            return Amg(q["max_levels"], q["threshold"]).setup(a)
        if k == "AdditiveSchwarz" and "overlap" in q:  # PC.AdditiveSchwarz(...); the bare PC("AdditiveSchwarz") keeps raising Unsupported
            pc = AdditiveSchwarz(q["overlap"], q["subdomains"], q["nparts"])
            return (pc if q.get("sub") is None else pc.with_sub_ilu(q["sub"])).setup(a)
        if k == "Ssor" and "omega" in q:              # PC.Ssor(...); the bare PC("Ssor") keeps raising Unsupported
            return Sor(q["omega"], q["its"], 1, MatSorType.SYMMETRIC_SWEEP, 0.0).setup(a)
        if k == "Multicolor" and "omega" in q:        # PC.Multicolor(colors); the bare PC("Multicolor") keeps raising Unsupported
            return Sor(q["omega"], q["its"], 1, MatSorType.SYMMETRIC_SWEEP, 0.0).with_colors(q["colors"]).setup(a)
        raise KError(6, f"preconditioner kind {k} is outside the accelerated path")


class SolverKind(enum.Enum):                      # src/context/ksp_context.rs:25-48 (the kinds on the hot path)
    Cg = "cg"
    Pcg = "pcg"
    GmresLeft = "gmres_left"
    GmresRight = "gmres_right"
    Bicgstab = "bicgstab"
    Fgmres = "fgmres"
    Cgs = "cgs"
    Tfqmr = "tfqmr"
    Qmr = "qmr"
    Minres = "minres"
    Cgnr = "cgnr"


class KspContext:
    """KspContext { kind, a, pc, tol, max_it, restart } + solve_context (src/context/ksp_context.rs:54-148): builds a
    fresh solver per call and forwards (a, pc, b, x).  Kinds outside the hot path raise KError(Unsupported)."""

    def __init__(self, kind, a, pc=None, tol=1e-8, max_it=1000, restart=30, flex_pc=None):
        self.kind, self.a, self.pc, self.tol, self.max_it, self.restart = kind, a, pc, tol, max_it, restart
        self.flex_pc = flex_pc                      # ksp_context.rs:62: FGMRES uses flex_pc, never pc (:101-107)

    def solve_context(self, b, x, comm=None):
        k = self.kind
        if k == SolverKind.GmresLeft:
            s = GmresSolver(self.restart, self.tol, self.max_it).with_preconditioning(Preconditioning.Left)
        elif k == SolverKind.GmresRight:
            s = GmresSolver(self.restart, self.tol, self.max_it).with_preconditioning(Preconditioning.Right)
        elif k == SolverKind.Cg:
            s = CgSolver(self.tol, self.max_it)
        elif k == SolverKind.Pcg:
            s = PcgSolver(self.tol, self.max_it)
        elif k == SolverKind.Bicgstab:
            s = BiCgStabSolver(self.tol, self.max_it)
        elif k == SolverKind.Cgs:
            s = CgsSolver(self.tol, self.max_it)
        elif k == SolverKind.Tfqmr:
            s = TfqmrSolver(self.tol, self.max_it)
        elif k == SolverKind.Qmr:                    # ksp_context.rs:128-146: the as-written solvers
            s = QmrSolver(self.tol, self.max_it)
        elif k == SolverKind.Minres:
            s = MinresSolver(self.tol, self.max_it)
        elif k == SolverKind.Cgnr:
            s = CgnrSolver(self.tol, self.max_it)
        elif k == SolverKind.Fgmres:
            return FgmresSolver(self.tol, self.max_it, self.restart).solve_flex(self.a, self.flex_pc, b, x)
        else:
            raise KError(6, f"solver kind {k} is outside the accelerated path")
        return s.solve(self.a, self.pc, b, x)


class Session:
    """Stepping form of CgSolver / PcgSolver / BiCgStabSolver on device vectors: begin, step(k) (enqueue k
    iterations without synchronising), end() -> SolveStats.  bench.py uses it to time exactly K iterations."""
    METHODS = {"cg": 0, "pcg": 1, "bicgstab": 2, "cgs": 3, "tfqmr": 4, "minres": 5, "qmr": 6, "cgnr": 7,
               "minres_textbook": 8, "cgnr_textbook": 9}

    def __init__(self, method, a, pc, b, x, tol, max_iters, norm_type=CgNormType.Unpreconditioned):
        self.a, self.pc, self.b, self.x = a, pc, b, x
        self.max_iters = max_iters
        prm = _ffi.Params(tol, max_iters, 0, 1, int(norm_type), 0, 0, 0.0, 0, 0.0, 0)
        self.ctx = a.ctx
        self.h = _ffi.Handle()
        check(lib().kryst_session_begin(self.METHODS[method], b.h, x.h, a.h, pc.h if pc is not None else None,
                                        C.byref(prm), C.byref(self.h)))
        self.ctx._adopt(self)

    def step(self, k):
        check(lib().kryst_session_step(self.h, k))

    # A session that is never ended keeps its context busy (KRYST_ERR_BUSY for every later solve): `with Session(...) as s:`
    # and the finaliser end it on every path (an exception between begin and end, a failing step)
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    _CLOSE_ORDER = 0                             # Context.close() ends open sessions before it destroys anything they use

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h and self.ctx.h:
            st = _ffi.Stats()
            hlen = C.c_int64(0)
            lib().kryst_session_end(h, C.byref(st), None, 0, C.byref(hlen))

    _release = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def end(self):
        st = _ffi.Stats()
        cap = self.max_iters + 8
        hist = np.zeros(cap)
        hlen = C.c_int64(0)
        rc = lib().kryst_session_end(self.h, C.byref(st), _dp(hist), cap, C.byref(hlen))
        self.h = None
        self.residual_history = hist[:min(hlen.value, cap)].tolist()
        stats = SolveStats(st.iterations, st.final_residual, bool(st.converged))
        check(rc, stats)
        return stats


# ----------------------------------------------------------------------------- host-only helpers
def _read_matrix_file(fn, path):
    nr, nc = C.c_int64(0), C.c_int64(0)
    nnz = fn(str(path).encode(), C.byref(nr), C.byref(nc), None, None, None)
    if nnz < 0:
        raise KError(102, lib().kryst_hip_last_error().decode())
    rp = np.zeros(nr.value + 1, dtype=np.int64); ci = np.zeros(max(nnz, 1), dtype=np.int64); va = np.zeros(max(nnz, 1))
    got = fn(str(path).encode(), C.byref(nr), C.byref(nc), rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i64p), _dp(va))
    if got != nnz:
        raise KError(102, lib().kryst_hip_last_error().decode() if got < 0 else "matrix file changed while reading")
    return nr.value, nc.value, rp, ci[:nnz], va[:nnz]


def read_matrix_market(path):
    """Matrix Market coordinate file -> (nrows, ncols, row_ptr, col_idx, vals) (host only; kryst_host_read_matrix_market)."""
    return _read_matrix_file(lib().kryst_host_read_matrix_market, path)


def read_petsc_binary(path):
    """PETSc binary AIJ matrix -> (nrows, ncols, row_ptr, col_idx, vals) (host only; kryst_host_read_petsc_binary)."""
    return _read_matrix_file(lib().kryst_host_read_petsc_binary, path)


def _host_factors(h):
    try:
        n, nl, nu = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().kryst_host_factors_sizes(h, C.byref(n), C.byref(nl), C.byref(nu)))
        lp = np.zeros(n.value + 1, dtype=np.int64); up = np.zeros(n.value + 1, dtype=np.int64)
        lc = np.zeros(max(nl.value, 1), dtype=np.int32); uc = np.zeros(max(nu.value, 1), dtype=np.int32)
        lv = np.zeros(max(nl.value, 1)); uv = np.zeros(max(nu.value, 1)); dg = np.zeros(max(n.value, 1))
        check(lib().kryst_host_factors_get(h, lp.ctypes.data_as(_ffi.c_i64p), lc.ctypes.data_as(_ffi.c_i32p), _dp(lv),
                                           up.ctypes.data_as(_ffi.c_i64p), uc.ctypes.data_as(_ffi.c_i32p), _dp(uv), _dp(dg)))
        return lp, lc[:nl.value], lv[:nl.value], up, uc[:nu.value], uv[:nu.value], dg[:n.value]
    finally:
        lib().kryst_host_factors_destroy(h)


def _host_rows(row_ptr, col_idx, values):
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    va = _f64(values)
    if len(rp) < 1 or len(ci) != len(va) or int(rp[-1]) != len(va):
        raise KError(102, "host factorisation: inconsistent array lengths")
    return rp, ci, va


def host_ilup(row_ptr, col_idx, values, fill, threads=0, block=0):
    """Ilup::new(fill).setup (ilup.rs:77-134) on host arrays, no GPU (kryst_host_ilup): the row pipeline kryst_pc_ilup runs between download
    and upload.  -> (l_ptr, l_col, l_val, u_ptr, u_col, u_val, diag): L's strictly-lower multipliers, U's strictly-upper kept entries, the kept
    diagonal (1.0 where none is kept).  KError(SolveError) on a zero u_jj, `.row` = that j."""
    rp, ci, va = _host_rows(row_ptr, col_idx, values)
    h = _ffi.Handle()
    check(lib().kryst_host_ilup(len(rp) - 1, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va), fill, threads, block, C.byref(h)))
    return _host_factors(h)


def host_ilut(row_ptr, col_idx, values, fill, droptol, threads=0):
    """Ilut::new(fill, droptol).setup (ilut.rs:80-117) on host arrays, no GPU (kryst_host_ilut); result as host_ilup."""
    rp, ci, va = _host_rows(row_ptr, col_idx, values)
    h = _ffi.Handle()
    check(lib().kryst_host_ilut(len(rp) - 1, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va), fill, float(droptol), threads, C.byref(h)))
    return _host_factors(h)


def host_amg(row_ptr, col_idx, values, max_levels, threshold, level_budget=0):
    """AMG::new(a, max_levels, threshold) (amg.rs:73-118) as written on host arrays, no GPU (kryst_host_amg): the set-up kryst_pc_amg
    uploads.  -> list of levels, each a dict with "A", "P", "R" as (nrows, ncols, row_ptr, col, val) ("P" / "R" None on the last level),
    "dinv" and "agg" (None on the last level).  KError(FactorError) when a level exceeds level_budget entries (<= 0: the default)."""
    rp, ci, va = _host_rows(row_ptr, col_idx, values)
    h = _ffi.Handle()
    check(lib().kryst_host_amg(len(rp) - 1, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i32p), _dp(va), int(max_levels),
                               float(threshold), int(level_budget), C.byref(h)))
    try:
        nl = C.c_int32()
        check(lib().kryst_host_amg_levels(h, C.byref(nl)))
        out = []
        for lv in range(nl.value):
            d = {}
            for w, key in ((0, "A"), (1, "P"), (2, "R")):
                nr, nc, nz = C.c_int64(), C.c_int64(), C.c_int64()
                check(lib().kryst_host_amg_get(h, lv, w, C.byref(nr), C.byref(nc), C.byref(nz), None, None, None))
                if w and lv == nl.value - 1:
                    d[key] = None
                    continue
                p = np.zeros(nr.value + 1, dtype=np.int64); c = np.zeros(max(nz.value, 1), dtype=np.int32); v = np.zeros(max(nz.value, 1))
                check(lib().kryst_host_amg_get(h, lv, w, None, None, None, p.ctypes.data_as(_ffi.c_i64p), c.ctypes.data_as(_ffi.c_i32p), _dp(v)))
                d[key] = (nr.value, nc.value, p, c[:nz.value], v[:nz.value])
            nz = C.c_int64()
            check(lib().kryst_host_amg_get(h, lv, 3, None, None, C.byref(nz), None, None, None))
            dv = np.zeros(max(nz.value, 1))
            check(lib().kryst_host_amg_get(h, lv, 3, None, None, None, None, None, _dp(dv)))
            d["dinv"] = dv[:nz.value]
            check(lib().kryst_host_amg_get(h, lv, 4, None, None, C.byref(nz), None, None, None))
            ag = np.zeros(max(nz.value, 1), dtype=np.int32)
            check(lib().kryst_host_amg_get(h, lv, 4, None, None, None, None, ag.ctypes.data_as(_ffi.c_i32p), None))
            d["agg"] = ag[:nz.value] if nz.value else None
            out.append(d)
        return out
    finally:
        lib().kryst_host_amg_destroy(h)


def host_levels(ptr, col, forward=True):
    """Dependency levels of a strictly-lower (forward) / strictly-upper triangular factor's rows (kryst_host_levels) -> (level[n], nlevels)."""
    p = np.ascontiguousarray(ptr, dtype=np.int64)
    c = np.ascontiguousarray(col, dtype=np.int32)
    lvl = np.zeros(max(len(p) - 1, 1), dtype=np.int32)
    nl = C.c_int32(0)
    check(lib().kryst_host_levels(len(p) - 1, p.ctypes.data_as(_ffi.c_i64p), c.ctypes.data_as(_ffi.c_i32p), 1 if forward else 0,
                                  lvl.ctypes.data_as(_ffi.c_i32p), C.byref(nl)))
    return lvl[:len(p) - 1], nl.value


def host_stencil7(N, kind="poisson", k_lo=0, k_hi=None):
    k_hi = N if k_hi is None else k_hi
    kk = STENCIL_KINDS[kind]
    nnz = lib().kryst_host_stencil7(N, kk, k_lo, k_hi, None, None, None)
    if nnz < 0:
        raise KError(102, "host_stencil7")
    nloc = (k_hi - k_lo) * N * N
    rp = np.empty(nloc + 1, dtype=np.int64); ci = np.empty(nnz, dtype=np.int64); va = np.empty(nnz)
    lib().kryst_host_stencil7(N, kk, k_lo, k_hi, rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i64p), _dp(va))
    return rp, ci, va


def partition_rows(n, nranks, align=1):
    out = np.empty(nranks + 1, dtype=np.int64)
    check(lib().kryst_host_partition_rows(n, nranks, align, out.ctypes.data_as(_ffi.c_i64p)))
    return out


def halo_recv_plan(rank, nranks, row_offsets, row_ptr, col_idx_global):
    ro = np.ascontiguousarray(row_offsets, dtype=np.int64)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col_idx_global, dtype=np.int64)
    args = (rank, nranks, ro.ctypes.data_as(_ffi.c_i64p), rp.ctypes.data_as(_ffi.c_i64p), ci.ctypes.data_as(_ffi.c_i64p))
    total = lib().kryst_host_halo_recv_plan(*args, None, None)
    counts = np.zeros(nranks, dtype=np.int64); cols = np.zeros(max(total, 1), dtype=np.int64)
    lib().kryst_host_halo_recv_plan(*args, counts.ctypes.data_as(_ffi.c_i64p), cols.ctypes.data_as(_ffi.c_i64p))
    return counts, cols[:total]
