"""What a call leaves behind: every handle kind gives its device memory back (a failing create included), every solve exit does and leaves
the context usable, a dropped or closed context takes everything on it along, and a call that is handed handles of two contexts is refused
before it launches anything.  The tables are tests/lifetime_cases.py; tests/test_lifetime_cases_cpu.py keeps them complete.

The figure and its grain: device_memory.free_bytes -- the driver's free memory after the context has drained.  MEASURED on an MI355X: holding
one-element DeviceVecs (8 KiB each) one by one, the figure first moved when the 252nd was held, by 2 097 152 bytes, and then every 256 vectors;
32 KiB vectors moved it every 64, 1 MiB vectors every 2.  So G = 2 MiB: the driver cuts small blocks out of 2 MiB chunks, and a loss shows
once it adds up to a chunk.  Every case repeats its create / use / destroy R <= 64 times per round (lifetime_cases: R and what stays below
the reach G / R of each case); three measured rounds follow one unmeasured one and all three readings must equal the first
(device_memory.readings)."""
import gc

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import device_memory as DM
import lifetime_cases as L
import block_cg_cases as BC
import mixed_cases as MC
import multirank_ext_cases as MX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return K.Context(0)


@pytest.fixture(scope="module")
def E(ctx):
    e = L.Env(ctx)
    e.jac = K.Jacobi().setup(e.d)
    e.aindef = MX.operator(MX.C_INDEFINITE)                     # poisson(8) - 0.5 I: CG and PCG meet p.Ap <= 0
    e.dindef = L.upload(ctx, e.aindef)
    e.jindef = K.Jacobi().setup(e.dindef)
    e.drot = L.upload(ctx, O.Csr.from_dense([[0.0, 1.0], [-1.0, 0.0]]))      # A r orthogonal to r: BiCGStab's and TFQMR's first-step exits
    e.daniso = L.upload(ctx, O.stencil7(L.N, "aniso"))
    e.d32 = e.d.lower()
    e.b32 = K.DeviceVec32.from_f64(e.b)
    a8 = O.stencil7(8, "poisson")
    e.b8 = a8.spmv(np.ones(a8.nrows))
    e.ref8 = O.solve("cg", a8, e.b8, tol=1e-9, max_iters=100, rs=O.Reduce.tiled(*K.reduce_spec()))
    return e


def context_still_right(E):
    """CG on stencil7(8) on the same context: the oracle's bits"""
    s = K.CgSolver(1e-9, 100)
    x = np.zeros(512)
    st = s.solve(E.small, None, E.b8, x)
    assert st.iterations == E.ref8.iterations and st.converged == E.ref8.converged
    assert np.array_equal(np.array(s.residual_history), E.ref8.history) and np.array_equal(x, E.ref8.x)


# ------------------------------------------------------------------------------------------------ 0. the checker is not blind
def test_the_protocol_reports_a_vector_kept_per_round(E):
    kept = []

    def round_():
        kept.append(K.DeviceVec(E.ctx, 262144))               # (262144 + 512) doubles: a little over G
        L.HANDLE_CASES["vec"].round(E)

    lost = DM.readings(E.ctx, round_)
    assert lost[0] >= L.G and lost[1] >= lost[0] + L.G and lost[2] >= lost[1] + L.G, lost       # a steady loss
    kept.clear()
    with pytest.raises(AssertionError, match="free device memory fell by"):
        DM.assert_gives_back(E.ctx, lambda: kept.append(K.DeviceVec(E.ctx, 262144)), "self-check")
    kept.clear()
    DM.assert_gives_back(E.ctx, lambda: L.HANDLE_CASES["vec"].round(E), "self-check, nothing kept")


# ------------------------------------------------------------------------------------------------ 1. every handle kind
@pytest.mark.parametrize("name", list(L.HANDLE_CASES))
def test_handle_kind_gives_its_memory_back(E, name, monkeypatch):
    case = L.HANDLE_CASES[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    DM.assert_gives_back(E.ctx, lambda: case.round(E), f"{name} (R = {case.R}, reach {L.reach(case.R)} bytes)")


# ------------------------------------------------------------------------------------------------ 2. every solve exit
def _solve(s, a, pc, b, x):
    try:
        return 0, s.solve(a, pc, b, x)
    except K.KError as e:
        return e.code, e.stats


def _exit(E, name, which, monkeypatch):
    make, pck = L.SOLVERS[name]
    ctx, n = E.ctx, E.n
    pc = E.jac if pck else None
    x = K.DeviceVec(ctx, n)
    if which == "converged":                                   # to the tolerance, or as far as 400 iterations take the as-written forms
        code, st = _solve(make(1e-8, 400), E.d, pc, E.b, x)
        assert code == 0 and 7 < st.iterations <= 400, (name, code, st)
        if name in L.CONVERGE:
            assert st.converged and st.iterations < 400 and st.final_residual < 1e-5, (name, st)
    elif which == "cap":
        code, st = _solve(make(1e-30, 7), E.d, pc, E.b, x)
        assert code == 0 and st.iterations == 7, (name, code, st)
    elif which == "max_iters_zero":
        code, st = _solve(make(1e-8, 0), E.d, pc, E.b, x)
        assert code == 0 and st.iterations == 0 and not st.converged, (name, code, st)
    elif which == "zero_rhs":                                  # p.Ap = 0 is IndefiniteMatrix for CG and PCG (cg.rs:168-174); the others end or run on NaNs
        code, st = _solve(make(1e-8, 20), E.d, pc, K.DeviceVec(ctx, n), x)
        assert code == (3 if name in ("cg", "pcg") else 0) and st.iterations <= 20, (name, code, st)
    elif which == "wrong_length":
        x.fill(-99.0)
        code, _ = _solve(make(1e-8, 20), E.d, pc, K.DeviceVec(ctx, n - 1), x)
        assert code == 102 and np.all(x.to_host() == -99.0), (name, code)
    elif which == "indefinite":
        code, st = _solve(make(1e-8, 100), E.dindef, E.jindef if pck else None, K.DeviceVec(ctx, MX.rhs(E.aindef)), K.DeviceVec(ctx, 512))
        assert code == 3, (name, code, st)
    elif which == "rotation":
        code, st = _solve(make(1e-12, 10), E.drot, None, K.DeviceVec(ctx, np.array([1.0, 1.0 if name == "tfqmr" else 0.0])), K.DeviceVec(ctx, 2))
        assert code == 0 and st.iterations <= 1, (name, code, st)      # (tests/test_gpu_cgs_tfqmr.py and tests/test_gpu_0_parity.py pin the bits)
    elif which == "ilu_give_up":                               # the wavefront solve gives up inside the solve; the one-shot entry repeats it
        monkeypatch.setenv("KRYST_ILU_POLL_BUDGET", "1")
        ilu = K.TrueIlu0().setup(E.daniso)
        assert ilu.ilu_info()["form"].startswith("grid 8x8") or ilu.ilu_info()["form"].startswith("grid 16x16")
        code, st = _solve(make(1e-9, 30), E.daniso, ilu, E.b, K.DeviceVec(ctx, n))
        monkeypatch.delenv("KRYST_ILU_POLL_BUDGET")
        assert ilu.ilu_info()["form"].startswith("grid planes"), ilu.ilu_info()     # it gave up and fell back to the plane kernels
        assert code == 0 and st.iterations == 30 and np.isfinite(st.final_residual), (name, code, st)
        del ilu
    else:
        raise KeyError(which)


def _repeat(E, exits, one):
    """every exit SOLVE_R times, the context checked after each exit"""
    def round_():
        for which in exits:
            for _ in range(L.SOLVE_R):
                one(which)
            context_still_right(E)
    return round_


@pytest.mark.parametrize("name", list(L.SOLVERS))
def test_solver_exits_give_their_memory_back(E, name, monkeypatch):
    exits = L.COMMON_EXITS + L.OWN_EXITS.get(name, ())
    DM.assert_gives_back(E.ctx, _repeat(E, exits, lambda which: _exit(E, name, which, monkeypatch)), f"solver {name}, exits {exits}")


def _many(E, cls, pc, which):
    n, k = E.n, 4
    B = np.random.default_rng(24).standard_normal((n, k))     # independent columns (block CG has no deflation)
    tol, cap = {"converged": (1e-8, 400), "cap": (1e-30, 7), "max_iters_zero": (1e-8, 0), "zero_rhs": (1e-8, 20), "wrong_length": (1e-8, 20)}[which]
    s = cls(tol, cap)
    run = s.solve_block if cls is K.BlockCgSolver else s.solve_many
    Bm = K.MultiVec.from_numpy(np.zeros((n, k)) if which == "zero_rhs" else B, ctx=E.ctx)
    if which == "wrong_length":
        Xm = K.MultiVec.from_numpy(np.full((n - 1, k), -99.0), ctx=E.ctx)
        assert L.err(lambda: run(E.d, pc, Bm, Xm), 102) and np.all(Xm.to_numpy() == -99.0)
        return
    res = run(E.d, pc, Bm, K.MultiVec(E.ctx, n, k))
    if which == "converged":
        assert all(isinstance(r, K.SolveStats) and r.converged for r in res), res


def _block_breakdowns(E):
    for name, (a, b, jac, status, it) in BC.breakdown_cases().items():
        d = L.upload(E.ctx, a)
        g, _ = BC.breakdown_reference(name)
        res = K.BlockCgSolver(BC.TOL, BC.CAP).solve_block(d, K.Jacobi().setup(d) if jac else None, K.MultiVec.from_numpy(b, ctx=E.ctx),
                                                          K.MultiVec.from_numpy(g, ctx=E.ctx))
        assert all((r.code if isinstance(r, K.KError) else 0) == status for r in res), (name, status, res)


def _solve32(E, cls, pc, which):
    n = E.n
    tol, cap = {"converged": (1e-5, 400), "cap": (1e-30, 7), "max_iters_zero": (1e-6, 0), "zero_rhs": (1e-6, 20), "wrong_length": (1e-6, 20)}.get(which, (1e-6, 40))
    x = K.DeviceVec32(E.ctx, n)
    if which == "zero_jacobi_entry":                          # mixed_cases.zero_diagonal: Jacobi's inverse is 0.0 in row 5
        z = MC.zero_diagonal()
        dz = L.upload(E.ctx, z)
        _solve(cls(tol, cap), dz.lower(), K.Jacobi().setup(dz), K.DeviceVec32(E.ctx, MC.rhs(z.nrows, seed=4).astype(np.float32)), K.DeviceVec32(E.ctx, z.nrows))
    elif which == "wrong_length":
        assert _solve(cls(tol, cap), E.d32, pc, K.DeviceVec32(E.ctx, n - 1), x)[0] == 102
    else:
        code, st = _solve(cls(tol, cap), E.d32, pc, K.DeviceVec32(E.ctx, n) if which == "zero_rhs" else E.b32, x)
        assert code == (3 if which == "zero_rhs" else 0), (which, code, st)      # b = 0: p.Ap = 0 is IndefiniteMatrix, as cg.rs:168-174 has it


def _refinement(E, which):
    tol, outer = {"converged": (1e-10, 8), "cap": (1e-30, 2), "max_iters_zero": (1e-10, 0), "zero_rhs": (1e-10, 4), "wrong_length": (1e-10, 4)}[which]
    s = K.RefinementSolver(tol, outer).with_inner(1e-4, 200)
    x = K.DeviceVec(E.ctx, E.n)
    if which == "wrong_length":
        assert _solve(s, E.d, None, K.DeviceVec(E.ctx, E.n - 1), x)[0] == 102
    else:
        assert _solve(s, E.d, None, K.DeviceVec(E.ctx, E.n) if which == "zero_rhs" else E.b, x)[0] == 0


def _session(E, method):
    pc = E.jac if method == "pcg" else None
    s = K.Session(method, E.d, pc, E.b, K.DeviceVec(E.ctx, E.n), 1e-8, 12)
    s.step(5)
    s.step(0)
    st = s.end()
    assert st.iterations == 5, (method, st)


def _session_busy(E, _):
    s = K.Session("cg", E.d, None, E.b, K.DeviceVec(E.ctx, E.n), 1e-8, 12)
    s.step(3)
    x = K.DeviceVec(E.ctx, E.n).fill(-99.0)
    assert _solve(K.CgSolver(1e-8, 20), E.d, None, E.b, x)[0] == 104
    assert _solve(K.GmresSolver(5, 1e-8, 20), E.d, E.jac, E.b, x)[0] == 104
    assert L.err(lambda: K.Session("cg", E.d, None, E.b, x, 1e-8, 12), 104)
    assert np.all(x.to_host() == -99.0)
    E.jac.apply(E.r, E.z)                                      # stays legal while the session is open
    assert s.end().iterations == 3


def _session_dropped(E, method):
    s = K.Session(method, E.d, E.jac if method == "pcg" else None, E.b, K.DeviceVec(E.ctx, E.n), 1e-8, 12)
    s.step(3)
    del s                                                      # never ended: the finaliser ends it, the context is free again


OTHER = {
    "multi_cg": (L.COMMON_EXITS, lambda E, w: _many(E, K.CgSolver, None, w)),
    "multi_pcg": (L.COMMON_EXITS, lambda E, w: _many(E, K.PcgSolver, E.jac, w)),
    "block_cg": (L.COMMON_EXITS + ("breakdowns",), lambda E, w: _block_breakdowns(E) if w == "breakdowns" else _many(E, K.BlockCgSolver, E.jac, w)),
    "cg32": (L.COMMON_EXITS, lambda E, w: _solve32(E, K.Cg32Solver, None, w)),
    "pcg32": (L.COMMON_EXITS + ("zero_jacobi_entry",), lambda E, w: _solve32(E, K.Pcg32Solver, E.jac, w)),
    "refinement": (L.COMMON_EXITS, _refinement),
    "session": (tuple(K.Session.METHODS), _session),
    "session_busy": (("busy",), _session_busy),
    "session_dropped": (("cg", "pcg", "bicgstab", "minres_textbook"), _session_dropped),
}


@pytest.mark.parametrize("name", L.OTHER_SOLVE_CASES)
def test_other_solve_exits_give_their_memory_back(E, name):
    assert set(OTHER) == set(L.OTHER_SOLVE_CASES)
    exits, one = OTHER[name]
    DM.assert_gives_back(E.ctx, _repeat(E, exits, lambda which: one(E, which)), f"{name}, exits {exits}")


# ------------------------------------------------------------------------------------------------ 3. contexts
def _solve_on(c, N=64):
    """an operator, two vectors and a CG solve on context c (64^3: a work arena of several MiB) -> the objects made"""
    a = K.CsrMatrix.stencil7(N, "poisson", ctx=c)
    b, x = K.DeviceVec(c, N ** 3).fill(1.0), K.DeviceVec(c, N ** 3)
    pc = K.Jacobi().setup(a)
    st = K.PcgSolver(1e-8, 10).solve(a, pc, b, x)
    assert st.iterations == 10
    return a, b, x, pc


def test_dropped_contexts_give_their_memory_back(E):
    def round_():
        c = K.Context(0)
        objs = _solve_on(c)
        del objs
        del c                                                  # no close(): the last reference goes, __del__ destroys the context
        gc.collect()
    DM.assert_gives_back(E.ctx, round_, "a context that is dropped")
    context_still_right(E)


@pytest.mark.parametrize("order", ["close_then_del", "del_then_close"])
def test_close_with_live_children(E, order):
    def round_():
        c = K.Context(0)
        a, b, x, pc = _solve_on(c)
        low = a.lower()
        mv, v32 = K.MultiVec(c, 4096, 4), K.DeviceVec32(c, 4096)
        dense, lu = K.DenseMatrix.from_numpy(E.dense64, ctx=c), K.LuSolver(c)
        sess = K.Session("cg", a, None, b, K.DeviceVec(c, len(b)), 1e-8, 5)      # open when the context is closed
        kids = [sess, pc, low, a, dense, lu, b, x, mv, v32]
        if order == "close_then_del":
            c.close()
            assert c.h is None and all(k.h is None for k in kids)
            for call in (x.to_host, lambda: a.spmv(b, x), lambda: pc.apply(b, x), mv.to_numpy, v32.to_host, dense.to_numpy, lu.info,
                         lambda: low.spmv(v32, v32), lambda: sess.step(1), lambda: K.DeviceVec(c, 8)):
                with pytest.raises(K.KError):
                    call()
            c.close()                                          # twice: nothing left to do
            del sess, pc, low, a, dense, lu, b, x, mv, v32, kids
        else:
            del sess, pc, low, a, dense, lu, b, x, mv, v32, kids
            gc.collect()
            assert not c._children
            c.close()
            assert c.h is None
        del c
        gc.collect()
    DM.assert_gives_back(E.ctx, round_, f"close() with live children, {order}")
    context_still_right(E)


# ------------------------------------------------------------------------------------------------ 4. handles of two contexts
SENTINEL = -99.0


class Small:
    """the long-lived handles of one context for the two-context calls: 512 rows"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.csr = L.upload(ctx, O.stencil7(8, "poisson"))
        self.pc = K.Jacobi().setup(self.csr)
        self.csr32 = self.csr.lower()
        self.dense = K.DenseMatrix.from_csr(self.csr)
        self.lu = K.LuSolver(ctx)
        self.lu.solve(self.dense, None, np.ones(512), np.zeros(512))          # (solve_cached needs a factorization)

    def make(self, kind):
        """-> (the handle object, a function that reads it back or None)"""
        if kind == "vec":
            v = K.DeviceVec(self.ctx, 512).fill(SENTINEL)
            return v, v.to_host
        if kind == "vec32":
            v = K.DeviceVec32(self.ctx, np.full(512, SENTINEL, dtype=np.float32))
            return v, v.to_host
        if kind == "mvec":
            m = K.MultiVec.from_numpy(np.full((512, 2), SENTINEL), ctx=self.ctx)
            return m, m.to_numpy
        return getattr(self, kind), None


@pytest.fixture(scope="module")
def two(ctx):
    return Small(ctx), Small(K.Context(0))


@pytest.mark.parametrize("name", list(L.TWO_CONTEXT))
def test_handles_of_two_contexts_are_refused(two, name):
    kinds, call = L.TWO_CONTEXT[name]
    kinds = [k.rstrip("*") for k in kinds]
    one, other = two
    call(*[one.make(k)[0] for k in kinds])                     # handles of ONE context: the call is taken -- sizes and kinds are right
    for i in range(len(kinds)):
        made = [(other if j == i else one).make(k) for j, k in enumerate(kinds)]
        before = [read() if read else None for _, read in made]
        e = L.err(lambda: call(*[h for h, _ in made]), 102)
        for (_, read), was in zip(made, before):               # nothing was launched: every vector still holds its sentinel, bit for bit
            if read:
                now = read()
                assert now.tobytes() == was.tobytes() and np.all(now == SENTINEL), (name, i, str(e))
