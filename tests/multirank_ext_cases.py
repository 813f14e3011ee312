"""Case tables, operators and reference calls of the several-ranks tests of the newer solvers (tests/multirank_ext_worker.py runs one
rank of a case; tests/test_gpu_z_multirank_shim.py starts the ranks and compares; tests/test_multirank_ext_cpu.py checks the tables
with the references alone).

  section A   MINRES (as written and textbook), QMR and CGNR as written on partitioned operators, every transport, stepping sessions
  section B   ChebyshevPoly on a partitioned operator: apply, PCG / GMRES-right / FGMRES with it, the refused estimate
  section C   the run-ahead loop's termination rule at check_every boundaries, error and degenerate exits, the context afterwards
  section D   every entry that refuses a distributed operator or a context of several ranks: REFUSALS, SUPPORT

Every reference folds its inner products in the partition-aware order Reduce.tiled(*K.reduce_spec(), part_off=offs); everything is
compared bit for bit (IEEE-equal for CGNR as written only, as in tests/test_gpu_padding.py)."""
import functools
import math
import os
import re

import numpy as np

import kryst_amd as K
from oracle import oracle as O
import krylov_ext_ref as R
import cheb_poly_ref as CP
import amg_ref as AR
import krylov_pc_ref as KR
from multirank_worker import random_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 512                                    # rows of a tile (common.h: KR_TILE = KR_T * KR_V)
UNSUPPORTED, ERR_ARG, INDEFINITE_MATRIX = 6, 102, 3
TRANSPORTS = (("rccl", "rccl"), ("ipc", "rccl"), ("rccl", "peer"), ("ipc", "peer"))     # (scalars, halo); the first is the reference run


# ------------------------------------------------------------------------------------------------ operators and partitions
@functools.lru_cache(maxsize=None)
def operator(spec):
    """spec: ("stencil", N, kind) | ("general", n, "sym" | "nonsym") | ("indefinite", N, shift) -> oracle.Csr (the global operator)"""
    what = spec[0]
    if what == "stencil":
        return O.stencil7(spec[1], spec[2])
    if what == "general":
        import scipy.sparse as sp
        m = random_system(spec[1])
        if spec[2] == "nonsym":                   # half the strict upper triangle: row sums of |off-diagonal| only shrink, the diagonal stays
            m = (sp.tril(m, 0) + 0.5 * sp.triu(m, 1)).tocsr()
            m.sort_indices()
        return O.Csr(m.shape[0], m.shape[0], m.indptr, m.indices, m.data)
    if what == "indefinite":                      # the Poisson stencil with its diagonal lowered by `shift`
        a = O.stencil7(spec[1], "poisson")
        v = a.vals.copy()
        rows = np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))
        v[a.col_idx == rows] -= spec[2]
        return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)
    raise KeyError(spec)


def offsets(spec, P):
    """row offsets of the P ranks: whole grid planes for the stencils (what the device generator takes), alignment 1 for a general operator"""
    if spec[0] == "general":
        return K.partition_rows(spec[1], P, 1)
    N = spec[1]
    return K.partition_rows(N ** 3, P, N * N)


def reduce_for(offs):
    return O.Reduce.tiled(*K.reduce_spec(), part_off=np.asarray(offs, dtype=np.int64))


def local_rows(a, offs, rank):
    """(row_ptr, global col_idx, vals) of one rank's rows, for CsrMatrix.from_csr_dist"""
    lo, hi = int(offs[rank]), int(offs[rank + 1])
    rp = np.asarray(a.row_ptr, dtype=np.int64)
    s, e = int(rp[lo]), int(rp[hi])
    return rp[lo:hi + 1] - s, np.asarray(a.col_idx, dtype=np.int64)[s:e], np.asarray(a.vals, dtype=np.float64)[s:e]


def tile_kinds(a, offs, rank):
    """per tile of the rank's rows: True where a row of the tile reads a column another rank owns (a boundary tile)"""
    lo, hi = int(offs[rank]), int(offs[rank + 1])
    rp, ci = np.asarray(a.row_ptr), np.asarray(a.col_idx)
    out = []
    for t0 in range(lo, hi, TILE):
        t1 = min(t0 + TILE, hi)
        c = ci[rp[t0]:rp[t1]]
        out.append(bool(((c < lo) | (c >= hi)).any()))
    return out


def halo_sides(a, offs, rank):
    """(reads columns below its rows, reads columns above its rows)"""
    lo, hi = int(offs[rank]), int(offs[rank + 1])
    rp, ci = np.asarray(a.row_ptr), np.asarray(a.col_idx)
    c = ci[rp[lo]:rp[hi]]
    return bool((c < lo).any()), bool((c >= hi).any())


def rhs(a):
    return a.spmv(np.linspace(0.5, 1.5, a.nrows))


def guess(a):
    return np.linspace(-1.0, 1.0, a.nrows)


# ------------------------------------------------------------------------------------------------ section A
EXT = ("minres", "minres_textbook", "qmr", "cgnr")
NAN_OK = {"cgnr"}                               # tests/test_gpu_padding.py: cgnr as written is the one compared IEEE-equal
A_PARAMS = ((1e-8, 80), (1e-30, 7))             # (tol, max_iters): to convergence (or the cap), and a run cut off at 7
# name -> P, operator, the solvers run, stepping sessions or not, light (RCCL + RCCL and both hipIpc forms together only)
A_CASES = {
    "poisson12-p2": dict(P=2, op=("stencil", 12, "poisson"), solvers=("minres", "minres_textbook"), sessions=False, light=False),
    "convdiff12-p3": dict(P=3, op=("stencil", 12, "convdiff"), solvers=("qmr", "cgnr"), sessions=True, light=False),
    "varcoef10-p3": dict(P=3, op=("stencil", 10, "varcoef"), solvers=EXT, sessions=False, light=False),
    "general1031-p4": dict(P=4, op=("general", 1031, "nonsym"), solvers=("qmr", "cgnr"), sessions=False, light=False),
    "general1031sym-p4": dict(P=4, op=("general", 1031, "sym"), solvers=("minres", "minres_textbook"), sessions=False, light=False),
    "poisson48-p4-light": dict(P=4, op=("stencil", 48, "poisson"), solvers=("minres",), sessions=False, light=True),
    # the named 12^3 and 10^3 grids on three ranks leave a rank one or two tiles, all of them boundary tiles: these two give EVERY rank interior
    # and boundary tiles and a halo from both sides on the middle rank (tests/test_multirank_ext_cpu.py asserts which case has what)
    "convdiff16-p3": dict(P=3, op=("stencil", 16, "convdiff"), solvers=("qmr", "cgnr"), sessions=False, light=True),
    "varcoef16-p3": dict(P=3, op=("stencil", 16, "varcoef"), solvers=("minres", "qmr"), sessions=False, light=True),
}
INTERIOR_AND_BOUNDARY_ON_EVERY_RANK = ("poisson12-p2", "poisson48-p4-light", "convdiff16-p3", "varcoef16-p3")
SESSION_METHODS = {"bicgstab": 2, "minres": 5, "qmr": 6, "cgnr": 7, "minres_textbook": 8}     # solve_api.hip: kryst_session_begin
SESSION_STEPS = (3, 0, 6)                       # then the rest of max_iters
SESSION_MAX_ITERS, SESSION_STOP = 20, 6         # the stop falls inside the third step (iterations 4..9)


def a_transports(case):
    return (TRANSPORTS[0], TRANSPORTS[3]) if A_CASES[case]["light"] else TRANSPORTS


def make_solver(method, tol, max_iters):
    return {"minres": lambda: K.MinresSolver(tol, max_iters), "minres_textbook": lambda: K.MinresSolver(tol, max_iters).with_textbook(),
            "qmr": lambda: K.QmrSolver(tol, max_iters), "cgnr": lambda: K.CgnrSolver(tol, max_iters),
            "cg": lambda: K.CgSolver(tol, max_iters), "pcg": lambda: K.PcgSolver(tol, max_iters),
            "bicgstab": lambda: K.BiCgStabSolver(tol, max_iters),
            "gmres5": lambda: K.GmresSolver(5, tol, max_iters).with_preconditioning(K.Preconditioning.NoPc)}[method]()


def a_reference(case, method, tol, max_iters):
    c = A_CASES[case]
    a = operator(c["op"])
    return R.SOLVERS[method](a, rhs(a), guess(a), tol, max_iters, reduce_for(offsets(c["op"], c["P"])))


# ------------------------------------------------------------------------------------------------ one series per solver for the stop rule
def series(method, a, b, rs, max_iters, x0=None):
    """-> (s, res0): s[i] is the residual the solver's convergence rule reads after iteration i (s[0]: before the first), from a reference
    run that never meets its tolerance; res0 is what the rule divides by, None where the tolerance is absolute"""
    x0 = np.zeros(a.nrows) if x0 is None else x0
    r0 = b - a.spmv(x0)
    if method == "cg":
        res = O.solve(method, a, b, x0=x0, tol=0.0, max_iters=max_iters, rs=rs)
        return np.asarray(res.history), float(res.history[0])
    if method == "pcg":                           # res0 = sqrt(|r0 . z0|) whatever the norm type (pcg.rs:134)
        pc = O.Pc.jacobi(a)
        res = O.solve(method, a, b, x0=x0, pc=pc, tol=0.0, max_iters=max_iters, rs=rs)
        return np.asarray(res.history), math.sqrt(abs(float(O.dot(r0, pc.apply(r0), rs))))
    if method == "bicgstab":                      # ABSOLUTE tolerance (bicgstab.rs:98-102, :281-284)
        res = O.solve(method, a, b, x0=x0, tol=0.0, max_iters=max_iters, rs=rs)
        return np.asarray(res.history), None
    n0 = float(O.norm(r0, rs))
    if method == "gmres5":
        res = O.solve("gmres", a, b, x0=x0, tol=0.0, max_iters=max_iters, restart=5, side=O.SIDE_NONE, rs=rs)
        return np.concatenate([[n0], res.history]), n0
    res = R.SOLVERS[method](a, b, x0, 0.0, max_iters, rs)
    return np.concatenate([[n0], np.asarray(res.history, dtype=float)]), n0


def tol_for_stop(s, res0, k):
    """the geometric mean of entries k - 1 and k, relative to res0 under a relative rule"""
    t = math.sqrt(float(s[k - 1]) * float(s[k]))
    return t if res0 is None else t / res0


def reference_solve(method, a, b, rs, tol, max_iters, x0=None):
    """-> (code, iterations, converged, final_residual, history, x)"""
    x0 = np.zeros(a.nrows) if x0 is None else x0
    if method in ("cg", "pcg", "bicgstab", "gmres5"):
        kw = dict(restart=5, side=O.SIDE_NONE) if method == "gmres5" else {}
        res = O.solve("gmres" if method == "gmres5" else method, a, b, x0=x0, pc=O.Pc.jacobi(a) if method == "pcg" else None, tol=tol,
                      max_iters=max_iters, rs=rs, raise_on_error=False, **kw)
        return res.code, res.iterations, res.converged, res.final_residual, np.asarray(res.history), res.x
    res = R.SOLVERS[method](a, b, x0, tol, max_iters, rs)
    return 0, res.iterations, bool(res.converged), float(res.final_residual), np.asarray(res.history, dtype=float), res.x


@functools.lru_cache(maxsize=None)
def session_tol(case, method):
    c = A_CASES[case]
    a = operator(c["op"])
    s, rel = series(method, a, rhs(a), reduce_for(offsets(c["op"], c["P"])), SESSION_MAX_ITERS, guess(a))
    return tol_for_stop(s, rel, SESSION_STOP)


# ------------------------------------------------------------------------------------------------ section B
B_CASES = {"poisson12-p2": dict(P=2, op=("stencil", 12, "poisson")), "varcoef10-p3": dict(P=3, op=("stencil", 10, "varcoef"))}
B_DEGREES, B_SCALINGS = (0, 1, 4), (False, True)
B_SEED = 7
B_PCG, B_GMRES, B_FGMRES = (1e-8, 60), (10, 1e-8, 30), (1e-8, 60, 10)     # (tol, max_iters) | (restart, tol, max_iters) | (tol, max_iters, restart)


def b_bounds(a, jacobi):
    """explicit bounds from the restatement alone: the Gershgorin bound of (W) A and a thirtieth of it (cheb_poly_ref.default_bounds' ratio)"""
    hi = CP.gershgorin(a, CP.jacobi_w(a) if jacobi else None)
    return hi / 30.0, hi


def b_apply_input(a):
    return O.splitmix64_uniform(B_SEED, a.nrows)


def b_reference(case, jacobi, degree):
    """-> dict(z, pcg=(x, iterations, code, history), gmres=(x, iterations, final_residual, converged, history))"""
    c = B_CASES[case]
    a = operator(c["op"])
    rs = reduce_for(offsets(c["op"], c["P"]))
    lo, hi = b_bounds(a, jacobi)
    w = CP.jacobi_w(a) if jacobi else None
    b = rhs(a)
    return {"z": CP.apply(a, b_apply_input(a), degree, lo, hi, w),
            "pcg": AR.pcg(a, None, b, B_PCG[0], B_PCG[1], rs, apply=CP.make_apply(a, degree, lo, hi, w, two_args=True)),
            "gmres": KR.gmres(a, CP.make_apply(a, degree, lo, hi, w), "right", b, B_GMRES[0], B_GMRES[1], B_GMRES[2], rs)}


# ------------------------------------------------------------------------------------------------ section C
C_P, C_N = 3, 8
C_OP = ("stencil", C_N, "poisson")
C_MAX_ITERS = 60
C_CHECK_EVERY = (1, 3, 8)
C_STOPS = (1, 7, 8, 9, 16, 17)
C_SWEEP = ("cg", "pcg", "bicgstab", "minres")
C_GMRES_STOPS = (4, 5, 6, 10, 11)
C_SHIFT = 0.5                                   # poisson(8) - 0.5 I: indefinite; CG and PCG meet p.Ap <= 0 in their 7th iteration
C_INDEFINITE = ("indefinite", C_N, C_SHIFT)
C_ERROR_METHODS = ("cg", "pcg")
C_DEGENERATE = ("zero_rhs", "exact_guess", "max_iters_zero")
C_DEGENERATE_METHODS = {"zero_rhs": ("cg", "pcg", "bicgstab"), "exact_guess": ("cg", "pcg", "bicgstab"),
                        "max_iters_zero": ("cg", "pcg", "bicgstab", "gmres5")}
C_USE = (1e-9, 100)                             # the plain CG solve that shows the context still pairs its collectives


def c_offsets():
    return offsets(C_OP, C_P)


@functools.lru_cache(maxsize=None)
def c_series(method):
    a = operator(C_OP)
    return series(method, a, rhs(a), reduce_for(c_offsets()), 40)


def c_stop_cases():
    """[(method, k, tol)]: the sweep's solver x wanted stop, and GMRES(5)'s"""
    out = []
    for method, stops in [(m, C_STOPS) for m in C_SWEEP] + [("gmres5", C_GMRES_STOPS)]:
        s, rel = c_series(method)
        out += [(method, k, tol_for_stop(s, rel, k)) for k in stops]
    return out


def c_degenerate_problem(which):
    """-> (b, x0, tol, max_iters) on operator(C_OP)"""
    a = operator(C_OP)
    n = a.nrows
    if which == "zero_rhs":
        return np.zeros(n), np.zeros(n), 1e-8, 20
    if which == "exact_guess":
        return a.spmv(np.ones(n)), np.ones(n), 1e-8, 20
    return a.spmv(np.ones(n)), np.zeros(n), 1e-8, 0


def use_reference(spec=C_OP, P=C_P):
    a = operator(spec)
    return reference_solve("cg", a, rhs(a), reduce_for(offsets(spec, P)), C_USE[0], C_USE[1])


# ------------------------------------------------------------------------------------------------ section D
D_P, D_OP = 2, ("stencil", 8, "poisson")
SENTINEL = -99.0

# Every `"... not supported"` message of kryst_amd/csrc: (file, a fragment of the message) -> what it is.
#   entry     the name of the call in D_ENTRIES that reaches it (None: no call of the tests does, `why` says why)
#   status    what include/kryst_hip.h documents for it (silent: KRYST_UNSUPPORTED, like the siblings)
#   needs     "dist": a distributed operator is enough (also runs on a one-rank distributed operator); "ranks": a context of several ranks;
#             None: the refusal is not about distribution
REFUSALS = [
    dict(file="csr_create.hip", frag="transposed SpMV: distributed", count=2, entry="spmv_transpose", needs="dist"),
    dict(file="mixed_refine.hip", frag="refine: distributed", count=1, entry=None, needs="dist",
         why="behind csr32_lower: no lowered operator exists on the context of a distributed one (RefinementSolver is refused there)"),
    dict(file="asm_ilu.hip", frag="additive Schwarz with ILU sub-solves: a context", count=1, entry=None, needs="ranks",
         why="behind additive Schwarz's own check: every operator of a context of several ranks is a distributed one (csr_create refuses)"),
    dict(file="block_jacobi.hip", frag="block Jacobi: distributed", count=1, entry="block_jacobi", needs="dist"),
    dict(file="cheb_poly.hip", frag="spectrum_estimate: distributed", count=1, entry="estimate_spectrum", needs="dist"),
    dict(file="dense.hip", frag="%s: distributed contexts", count=1, entry=None, needs="ranks",
         why="the direct solvers' check of their matrix: no DenseMatrix exists on a context of several ranks (dense_create refuses)"),
    dict(file="dense.hip", frag="dense_create: distributed", count=1, entry="dense_create", needs="ranks"),
    dict(file="dense.hip", frag="dense_from_csr: distributed", count=1, entry="dense_from_csr", needs="dist"),
    dict(file="dense.hip", frag="lu_create: distributed", count=1, entry="lu_create", needs="ranks"),
    dict(file="sor.hip", frag="SOR: distributed", count=1, entry="sor", needs="dist"),
    dict(file="spai.hip", frag="SPAI: distributed", count=1, entry="spai", needs="dist"),
    dict(file="asm.hip", frag="additive Schwarz: distributed", count=1, entry="asm", needs="dist"),
    dict(file="mixed_lower.hip", frag="csr32_lower: distributed", count=1, entry="lower", needs="dist"),
    dict(file="mixed_vec.hip", frag="dot32: distributed", count=1, entry="dot32", needs="ranks"),
    dict(file="multi.hip", frag="solve_multi: %s are not supported", count=1, entry="solve_many_cg", needs="dist"),
    dict(file="multi.hip", frag="spmm: distributed", count=1, entry="spmm", needs="dist"),
    dict(file="gmres_cb.hip", frag="cbgmres: distributed", count=1, entry="cb_gmres", needs="dist"),
    dict(file="amg.hip", frag="pc_amg: distributed", count=1, entry="amg", needs="dist"),
    dict(file="pca_gmres.hip", frag="pca_gmres: distributed", count=1, entry="pca_gmres", needs="dist"),
    # refusals that have nothing to do with distribution (their own files test them)
    dict(file="mmio.cpp", frag="matrix market:", count=2, entry=None, needs=None, why="file format"),
    dict(file="mixed_cg.hip", frag="solve32: %s are not supported", count=1, entry=None, needs=None, why="fp32 storage: norm types, exits, preconditioners"),
    dict(file="mixed_refine.hip", frag="refine: preconditioners", count=1, entry=None, needs=None, why="preconditioner kind"),
    dict(file="asm_ilu.hip", frag="KRYST_ILU_KRYST_COMPAT is not supported", count=1, entry=None, needs=None, why="sub-solve mode"),
    dict(file="gmres_cb.hip", frag="cbgmres: left preconditioning", count=1, entry=None, needs=None, why="side"),
]

# name -> (expected status, what kryst_hip_last_error() must contain, needs); the calls themselves are d_calls() below.  Several entries
# share one source line (the AMG variants, batched CG / PCG and block CG, the two Schwarz forms with ILU); "asm_ilu" with a distributed
# operator on ONE rank is caught by additive Schwarz's own check first.
D_ENTRIES = {
    "asm": (UNSUPPORTED, "additive Schwarz", "dist"),
    "asm_ilu": (UNSUPPORTED, "additive Schwarz", "dist"),
    "sor": (UNSUPPORTED, "SOR", "dist"),
    "block_jacobi": (UNSUPPORTED, "block Jacobi", "dist"),
    "spai": (UNSUPPORTED, "SPAI", "dist"),
    "amg": (UNSUPPORTED, "pc_amg", "dist"),
    "amg_smoothed": (UNSUPPORTED, "pc_amg", "dist"),
    "pca_gmres": (UNSUPPORTED, "pca_gmres", "dist"),
    "pca_gmres_textbook": (UNSUPPORTED, "pca_gmres", "dist"),
    "cb_gmres": (UNSUPPORTED, "cbgmres", "dist"),
    "refinement": (UNSUPPORTED, "csr32_lower", "dist"),
    "cgnr_textbook": (UNSUPPORTED, "transposed SpMV", "dist"),
    "lower": (UNSUPPORTED, "csr32_lower", "dist"),
    "spmv_transpose": (UNSUPPORTED, "transposed SpMV", "dist"),
    "spmm": (UNSUPPORTED, "spmm", "dist"),
    "solve_many_cg": (UNSUPPORTED, "solve_multi", "dist"),
    "solve_many_pcg": (UNSUPPORTED, "solve_multi", "dist"),
    "block_cg": (UNSUPPORTED, "solve_multi", "dist"),
    "estimate_spectrum": (UNSUPPORTED, "spectrum_estimate", "dist"),
    "dense_from_csr": (UNSUPPORTED, "dense_from_csr", "dist"),
    "dot32": (UNSUPPORTED, "dot32", "ranks"),
    "dense_create": (UNSUPPORTED, "dense_create", "ranks"),
    "lu_create": (UNSUPPORTED, "lu_create", "ranks"),
}

# DESIGN.md section 6 carries this table (tests/test_multirank_ext_cpu.py compares the two)
SUPPORT = [
    ("CG, PCG, BiCGStab (both forms), GMRES (every side), FGMRES, CGS, TFQMR", "runs"),
    ("MINRES (as written, textbook), QMR, CGNR as written", "runs"),
    ("stepping sessions of CG, BiCGStab, MINRES (both forms), QMR, CGNR as written", "runs"),
    ("Jacobi, the ILU family (each rank's diagonal block), Chebyshev, ChebyshevPoly with explicit bounds (unfused form)", "runs"),
    ("textbook CGNR, transposed SpMV", "KRYST_UNSUPPORTED"),
    ("PCA-GMRES (both forms), CB-GMRES, RefinementSolver, fp32 lowering, dot32", "KRYST_UNSUPPORTED"),
    ("SpMM, batched CG / PCG, block CG", "KRYST_UNSUPPORTED"),
    ("additive Schwarz (LU and ILU sub-solves), SOR, block Jacobi, SPAI, AMG (both variants)", "KRYST_UNSUPPORTED"),
    ("spectrum estimate, DenseMatrix (creation, from_csr), LuSolver, QrSolver", "KRYST_UNSUPPORTED"),
]


def support_table_markdown():
    lines = ["| entry | on several ranks |", "|---|---|"]
    lines += [f"| {what} | {how} |" for what, how in SUPPORT]
    return "\n".join(lines)


def not_supported_sites():
    """[(file, line text)] of every line of kryst_amd/csrc that holds a "not supported" message"""
    d = os.path.join(ROOT, "kryst_amd", "csrc")
    out = []
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(d, fn), encoding="utf-8") as f:
                out += [(fn, line) for line in f if re.search(r"not supported", line)]
    return out


def d_calls(ctx, dd, ops):
    """name -> a call that must be refused, for a distributed operator `dd` on `ctx`.  `ops` collects the output operands a call was given,
    name -> [(what, read-back function, bits before)], so that the caller can show that a refusal wrote nothing."""
    n = dd.nrows()
    b = ctx.vec(np.linspace(0.5, 1.5, n))

    def sentinel_vec(name, length=n):
        v = ctx.vec(length).fill(SENTINEL)
        ops.setdefault(name, []).append(("vector", v.to_host, v.to_host()))
        return v

    def sentinel_mvec(name, k):
        m = K.MultiVec.from_numpy(np.full((n, k), SENTINEL), ctx=ctx)
        ops.setdefault(name, []).append(("multivector", m.to_numpy, m.to_numpy()))
        return m

    def pc_setup(name, pc):
        def run():
            try:
                pc.setup(dd)
            finally:
                ops.setdefault(name, []).append(("handle", lambda: np.array([0.0 if pc.h is None else 1.0]), np.array([0.0])))
        return run

    def solve(name, s, pc=None):
        return lambda: s.solve(dd, pc, b, sentinel_vec(name))

    def many(name, s, block=False):
        def run():
            B = K.MultiVec.from_numpy(np.ones((n, 4)), ctx=ctx)
            X = sentinel_mvec(name, 4)
            st, code, hlen = (K._ffi.Stats * 4)(), (K._ffi.C.c_int32 * 4)(*([-99] * 4)), (K._ffi.C.c_int64 * 4)(*([-99] * 4))
            hist = np.full((4, 18), SENTINEL)
            prm = s._params()
            fn = K.lib().kryst_bcg_solve_multi_dev if block else getattr(K.lib(), s._MULTI_DEV)
            rc = fn(B.h, X.h, dd.h, None, K._ffi.C.byref(prm), st, code, hist.ctypes.data_as(K._ffi.c_dp), 18, hlen)
            ops[name].append(("codes", lambda: np.array(list(code) + list(hlen), dtype=np.float64), np.full(8, -99.0)))
            ops[name].append(("histories", lambda: hist.copy(), np.full((4, 18), SENTINEL)))
            K._ffi.check(rc)
        return run

    def dot32():
        x = K.DeviceVec32(ctx, np.ones(8, dtype=np.float32))
        return K.dot32(x, x)

    def estimate():
        try:
            K.estimate_spectrum(dd)
        finally:
            ops.setdefault("estimate_spectrum", [])

    calls = {
        "asm": pc_setup("asm", K.AdditiveSchwarz(0, None, 8)),
        "asm_ilu": pc_setup("asm_ilu", K.AdditiveSchwarz(0, None, 8).with_sub_ilu("ilu0")),
        "sor": pc_setup("sor", K.Sor(1.0, 1, 1, K.MatSorType.APPLY_LOWER | K.MatSorType.APPLY_UPPER, 0.0)),
        "block_jacobi": pc_setup("block_jacobi", K.BlockJacobi.uniform(4)),
        "spai": pc_setup("spai", K.Spai(K.SparsityPattern.Operator, 0.0)),
        "amg": pc_setup("amg", K.Amg(4, 0.1)),
        "amg_smoothed": pc_setup("amg_smoothed", K.Amg(4).with_textbook(0.0)),
        "pca_gmres": solve("pca_gmres", K.PcaGmresSolver(5, 2, 1, 1e-8, 10).with_preconditioning(K.Preconditioning.NoPc)),
        "pca_gmres_textbook": solve("pca_gmres_textbook", K.PcaGmresSolver(8, 1, 4, 1e-8, 10).with_preconditioning(K.Preconditioning.NoPc).with_textbook()),
        "cb_gmres": solve("cb_gmres", K.CbGmresSolver(5, 1e-8, 10).with_preconditioning(K.Preconditioning.NoPc)),
        "refinement": solve("refinement", K.RefinementSolver(1e-10, 3)),
        "cgnr_textbook": solve("cgnr_textbook", K.CgnrSolver(1e-8, 10).with_textbook()),
        "lower": lambda: dd.lower(),
        "spmv_transpose": lambda: dd.spmv_transpose(b, sentinel_vec("spmv_transpose")),
        "spmm": lambda: dd.spmm(K.MultiVec.from_numpy(np.ones((n, 4)), ctx=ctx), sentinel_mvec("spmm", 4)),
        "solve_many_cg": many("solve_many_cg", K.CgSolver(1e-8, 10)),
        "solve_many_pcg": many("solve_many_pcg", K.PcgSolver(1e-8, 10)),
        "block_cg": many("block_cg", K.BlockCgSolver(1e-8, 10), block=True),
        "estimate_spectrum": estimate,
        "dense_from_csr": lambda: K.DenseMatrix.from_csr(dd),
        "dot32": dot32,
        "dense_create": lambda: K.DenseMatrix.from_numpy(np.eye(3), ctx=ctx),
        "lu_create": lambda: K.LuSolver(ctx),
    }
    assert set(calls) == set(D_ENTRIES)
    return calls


def run_refusals(ctx, dd, names):
    """-> name -> (status or 0, message, every output operand unchanged).  Calls the entries in table order."""
    ops, out = {}, {}
    calls = d_calls(ctx, dd, ops)
    for name in names:
        try:
            calls[name]()
            code, msg = 0, ""
        except K.KError as e:
            code, msg = e.code, str(e)
        same = all(np.array_equal(np.asarray(read(), dtype=np.float64).view(np.uint64), np.asarray(before, dtype=np.float64).view(np.uint64))
                   for _, read, before in ops.get(name, []))
        out[name] = (code, msg, same)
    return out
