"""The C++ header (include/kryst_hip.hpp) against the Python binding, bit for bit, for everything tests/cpp/test_mirror.cpp and its siblings do
not construct.  tests/cpp/test_ext_mirror.cpp runs every case once in one child process and writes what the header returned as 64-bit patterns;
here the same case runs through the Python binding on the same device, and code, iterations, converged, final residual, residual history, the
monitor's sequence and the result vector must be the same bits.  Where a restatement gives the result in one call (O.solve,
krylov_ext_ref.SOLVERS, cb_gmres_ref.cbgmres, pca_gmres_ref.as_written / sstep) the C++ record is compared with it as well, so the comparison
does not rest on the binding alone.

Inputs are closed formulas with exactly representable values (no libm, no generator): the device stencil generator, the tridiagonal with
diagonal 3 + (i % 3) / 2, b = 1 + (i % 7) / 8, x0 = r = ((37 i) % 64 - 32) / 16.  Sizes: poisson / aniso 8^3 = 512 rows (one reduction tile),
convdiff 9^3 = 729 rows (a partial second tile, odd), the tridiagonal at 10 and 513 rows, one 3 x 5 matrix.

The comment after each group of cases names the GPU test that pins that Python path to its oracle or restatement."""
import os
import subprocess
import time

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import krylov_ext_ref as KR
import cb_gmres_ref as CB
import pca_gmres_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCN = K.Preconditioning
NORM = K.CgNormType
MS = K.MatSorType


# ----------------------------------------------------------------------------- inputs (the formulas of tests/cpp/test_ext_mirror.cpp)
def fb(n):
    return 1.0 + (np.arange(n) % 7) / 8.0


def fx(n):
    return ((np.arange(n) * 37) % 64 - 32.0) / 16.0


def tridiag(n):
    rp, ci, va = [0], [], []
    for i in range(n):
        if i > 0:
            ci.append(i - 1); va.append(-1.5)
        ci.append(i); va.append(3.0 + 0.5 * (i % 3))
        if i + 1 < n:
            ci.append(i + 1); va.append(-0.5)
        rp.append(len(ci))
    return O.Csr(n, n, rp, ci, va)


def shifted_poisson(N, diag):
    a = O.stencil7(N, "poisson")
    v = a.vals.copy()
    v[a.col_idx == np.repeat(np.arange(a.nrows), np.diff(a.row_ptr))] = diag
    return O.Csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, v)


def chunks(n, length, reverse):
    return [list(range(lo, min(n, lo + length)))[::-1 if reverse else 1] for lo in range(0, n, length)]


BJ10 = [[2, 0, 1], [4, 2, 3], [8, 7, 9, 5]]
BJ512 = chunks(512, 8, True)
SUB729 = chunks(729, 27, True)
TRI_PAT = [([j + 1] if j + 1 < 512 else []) + [j] + ([j - 1] if j > 0 else []) for j in range(512)]
REDBLACK = [(i + j + k) % 2 for k in range(9) for j in range(9) for i in range(9)]


# ----------------------------------------------------------------------------- the child process and its records
def parse(path):
    recs, cur, done = {}, None, None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "CASE":
                assert cur is None and t[1] not in recs, line
                cur = (t[1], {})
            elif t[0] == "END":
                recs[cur[0]] = cur[1]
                cur = None
            elif t[0] == "EXT_MIRROR_DONE":
                done = int(t[1])
            else:
                assert cur is not None and len(t) == 3 + int(t[2]), line[:200]
                if t[0] == "i":
                    cur[1][t[1]] = np.array([int(v) for v in t[3:]], dtype=np.int64)
                else:
                    assert t[0] == "d" and all(len(v) == 16 for v in t[3:]), line[:200]
                    cur[1][t[1]] = np.array([int(v, 16) for v in t[3:]], dtype=np.uint64).view(np.float64)
    return recs, done, cur


class World:
    pass


@pytest.fixture(scope="module")
def W(tmp_path_factory):
    """One child process for the whole module (with this process, two have the GPU open); its exit status is checked before its file is read."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_ext_mirror")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    out = str(tmp_path_factory.mktemp("ext_mirror") / "records.txt")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "kryst_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300, env=env)
    w = World()
    w.child_seconds = time.perf_counter() - t0
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    w.recs, w.done, open_case = parse(out)
    assert open_case is None and w.done is not None, "the child's file ends before its marker line"
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    w.ctx = ctx = K.Context(0)
    T, V, F = K.reduce_spec()
    w.rs = O.Reduce.tiled(T, V, F)
    dev = lambda a: K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
    # name -> (oracle Csr, device operator): the stencils from the device generator, as in the C++ program
    w.o = {"P8": O.stencil7(8, "poisson"), "A8": O.stencil7(8, "aniso"), "C9": O.stencil7(9, "convdiff"), "T10": tridiag(10), "T513": tridiag(513),
           "S6": shifted_poisson(6, 8.0), "R35": O.Csr(3, 5, [0, 2, 3, 5], [0, 4, 1, 2, 3], [1.0, 2.0, 3.0, 4.0, -0.5])}
    w.d = {k: (K.CsrMatrix.stencil7(int(k[1]), {"P": "poisson", "A": "aniso", "C": "convdiff"}[k[0]], ctx=ctx) if k in ("P8", "A8", "C9") else dev(a))
           for k, a in w.o.items()}
    w.jac = {k: K.Jacobi().setup(w.d[k]) for k in ("P8", "C9", "T513")}
    w.ojac = {k: O.Pc.jacobi(w.o[k]) for k in ("P8", "C9", "T513")}
    w.cache = {}
    return w


def I(*v):
    return np.array([int(x) for x in v], dtype=np.int64)


def D(*v):
    return np.array(v, dtype=np.float64)


def py_solve(s, a, pc, b, x0, hist=True, extra=None):
    out = dict(extra or {})
    x = np.array(x0, dtype=np.float64)
    try:
        st = s.solve(a, pc, b, x)
        out.update(code=I(0), iterations=I(st.iterations), converged=I(st.converged), final=D(st.final_residual))
    except K.KError as e:
        out["code"] = I(e.code)
    if hist:
        out["hist"] = np.array(s.residual_history, dtype=np.float64)
    out["x"] = x
    return out


def py_apply(pc, r, zfill=0.0, extra=None):
    out = dict(extra or {}, code=I(0))
    z = np.full(len(r), zfill)
    try:
        if zfill == 0.0:
            z = pc.apply(r)                       # the binding makes z, zeros on the device
        else:
            pc.apply(r, z)
    except K.KError as e:
        out["code"] = I(e.code)
    out["z"] = np.asarray(z, dtype=np.float64)
    return out


def py_setup_error(make):
    try:
        make()
        return {"code": I(0)}
    except K.KError as e:
        return {"code": I(e.code)}


def py_ksp(w, kind):
    x = fx(729)
    st = K.KspContext(kind, w.d["C9"], K.PC.Jacobi().build(w.d["C9"]), 1e-8, 40).solve_context(fb(729), x)
    return {"code": I(0), "iterations": I(st.iterations), "converged": I(st.converged), "final": D(st.final_residual), "x": x}


def py_monitored(s, a, pc, b, x0, every):
    mi, mr = [], []
    s.with_monitor(lambda i, r: (mi.append(i), mr.append(r)))
    s.check_every = every
    out = py_solve(s, a, pc, b, x0)
    out["mon_i"], out["mon_r"] = I(*mi), D(*mr)
    return out


def py_spai(pc, r):
    rp, ci, va = pc.export()
    return py_apply(pc, r, extra={"row_ptr": I(*rp), "col": I(*ci), "val": np.asarray(va, dtype=np.float64)})


def py_spectrum(a, jacobi, steps):
    e = K.estimate_spectrum(a, jacobi, steps)
    assert e["steps_done"] == len(e["alpha"]) == len(e["beta"])
    return {"code": I(0), "alpha": e["alpha"], "beta": e["beta"], "theta_gersh": D(e["theta_min"], e["theta_max"], e["gershgorin"])}


def py_cheb(a, pc, r):
    pc.setup(a)
    inf = pc.info()
    return py_apply(pc, r, extra={"bounds": D(inf["lambda_min"], inf["lambda_max"]), "fused": I(inf["fused"])})


def py_state(w):
    s = K.MinresSolver(1e-8, 100)
    x1, x2 = fx(512), np.zeros(512)
    s.solve(w.d["P8"], None, fb(512), x1)
    first = len(s.residual_history)
    s.solve(w.d["P8"], None, fb(512), x2)
    out = {"code": I(0), "conv_tol": D(s.conv.tol), "conv_max_iters": I(s.conv.max_iters), "lengths": I(first, len(s.residual_history)), "hist": np.array(s.residual_history), "x": x2}
    s.clear_history()
    out["after_clear"] = I(len(s.residual_history))
    return out


def py_mtv(a, x, ny):
    y = np.full(ny, 0.5)
    out = {"code": I(0)}
    try:
        a.spmv_transpose(x, y)
    except K.KError as e:
        out["code"] = I(e.code)
    out["y"] = y
    return out


def asm(overlap, subdomains=None, nparts=None, variant="written", sub=None):
    p = K.AdditiveSchwarz(overlap, subdomains, nparts)
    if variant == "grown":
        p.with_overlap()
    elif variant == "restricted":
        p.restricted()
    return p.with_sub_ilu(sub) if sub is not None else p


def sor(sym, colors=None):
    p = K.Sor(1.3, 2, 1, sym, 0.25)
    return p.with_colors(colors) if colors is not None else p


def sor_by_setters():
    p = K.Sor(1.0, 1, 0, MS.APPLY_LOWER, 0.0)
    p.set_omega(1.3); p.set_its(2); p.set_lits(1); p.set_sym(MS.SYMMETRIC_SWEEP); p.set_fshift(0.25)
    return p


def gm_right():
    return K.GmresSolver(10, 1e-8, 60).with_preconditioning(PCN.Right)


def cases(w):
    """name -> thunk giving the Python binding's fields for that case"""
    d, jac = w.d, w.jac
    P8, A8, C9, T10, T513, S6, R35 = (d[k] for k in ("P8", "A8", "C9", "T10", "T513", "S6", "R35"))
    b512, x512, b729, x729 = fb(512), fx(512), fb(729), fx(729)
    c = {}
    # BlockJacobi: tests/test_gpu_block_jacobi.py
    c["bj_explicit_apply"] = lambda: py_apply(K.BlockJacobi(BJ10).setup(T10), fx(10))
    c["bj_uniform8_apply"] = lambda: py_apply(K.BlockJacobi.uniform(8).setup(C9), x729)
    c["bj_uniform1_apply"] = lambda: py_apply(K.BlockJacobi.uniform(1).setup(C9), x729)
    c["bj_apply"] = lambda: py_apply(K.BlockJacobi(BJ512).setup(P8), x512)
    c["bj_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), P8, K.BlockJacobi(BJ512).setup(P8), b512, x512)
    c["bj_build_apply"] = lambda: py_apply(K.PC.BlockJacobi(BJ512).build(P8), x512)
    c["bj_build_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), P8, K.PC.BlockJacobi(BJ512).build(P8), b512, x512)
    # AdditiveSchwarz: tests/test_gpu_asm.py; with ILU(0) subdomain solves: tests/test_gpu_asm_ilu.py
    for name, a, mk in (("written", C9, lambda: asm(2, SUB729)), ("nparts0", T10, lambda: asm(1, None, 0)), ("nparts3", T10, lambda: asm(1, None, 3)),
                        ("grown", C9, lambda: asm(1, SUB729, 0, "grown")), ("restricted", C9, lambda: asm(1, SUB729, 0, "restricted")),
                        ("ilu_true", C9, lambda: asm(1, None, 3, "restricted", 2)), ("ilu_ilup0", C9, lambda: asm(0, None, 0, "written", 1)),
                        ("ilu_default", C9, lambda: asm(0, SUB729, None, "written", "ilu0"))):
        n = a.nrows()
        c[f"asm_{name}_apply"] = lambda a=a, mk=mk, n=n: py_apply(mk().setup(a), fx(n))
        if name != "nparts0":                         # (one part of all rows is the exact inverse: nothing for GMRES to do)
            c[f"asm_{name}_gmres"] = lambda a=a, mk=mk, n=n: py_solve(gm_right(), a, mk().setup(a), fb(n), fx(n))
    # Sor: tests/test_gpu_sor.py
    c["sor_sym_apply"] = lambda: py_apply(sor(MS.SYMMETRIC_SWEEP).setup(C9), x729)
    c["sor_lower_apply"] = lambda: py_apply(sor(MS.APPLY_LOWER).setup(C9), x729)
    c["sor_upper_zero_apply"] = lambda: py_apply(sor(MS.APPLY_UPPER | MS.ZERO_INITIAL_GUESS).setup(C9), x729)
    c["sor_colors_apply"] = lambda: py_apply(sor(MS.SYMMETRIC_SWEEP, REDBLACK).setup(C9), x729)
    c["sor_setters_apply"] = lambda: py_apply(sor_by_setters().setup(C9), x729, extra={
        "omega_fshift": D(sor_by_setters().omega(), sor_by_setters().fshift()),
        "its_lits_sym": I(sor_by_setters().its(), sor_by_setters().lits(), sor_by_setters().sym())})
    c["sor_colors_wrong_length"] = lambda: py_setup_error(lambda: sor(MS.SYMMETRIC_SWEEP, [0] * 5).setup(C9))
    c["sor_moved_apply"] = lambda: py_apply(sor(MS.SYMMETRIC_SWEEP).setup(C9), x729, extra={"empty_after_move": I(1, 1, 1)})
    c["sor_gmres"] = lambda: py_solve(gm_right(), C9, sor(MS.SYMMETRIC_SWEEP).setup(C9), b729, x729)
    # Amg as written: tests/test_gpu_amg.py
    c["amg_default_apply"] = lambda: py_apply(K.Amg().setup(P8), x512)
    c["amg_l2_apply"] = lambda: py_apply(K.Amg(2, 0.25).setup(P8), x512)
    # (from x = 0: two levels on poisson 8^3 converge; the default hierarchy on poisson 6^3 + 2 I runs on and ends in IndefinitePreconditioner)
    c["amg_default_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), S6, K.Amg().setup(S6), fb(216), np.zeros(216))
    c["amg_l2_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), P8, K.Amg(2, 0.25).setup(P8), b512, np.zeros(512))
    # Spai: tests/test_gpu_spai.py
    c["spai_manual"] = lambda: py_spai(K.Spai(K.SparsityPattern.Manual(TRI_PAT), 0.01).setup(P8), x512)
    c["spai_operator"] = lambda: py_spai(K.Spai(K.SparsityPattern.Operator, 0.01).setup(P8), x512)
    c["spai_operator_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), P8, K.Spai(K.SparsityPattern.Operator, 0.01).setup(P8), b512, x512)
    c["spai_auto"] = lambda: py_setup_error(lambda: K.Spai(K.SparsityPattern.Auto, 0.01).setup(P8))
    c["spai_build_apply"] = lambda: py_apply(K.PC.ApproxInv(K.SparsityPattern.Operator, 0.01, 5).build(P8), x512)
    # estimate_spectrum and ChebyshevPoly: tests/test_gpu_cheb_poly.py
    for j in (1, 0):
        for steps in (1, 10, 64):
            c[f"spec_j{j}_s{steps}"] = lambda j=j, steps=steps: py_spectrum(A8, bool(j), steps)
    c["spec_t10_s64"] = lambda: py_spectrum(T10, True, 64)
    c["cheb_both"] = lambda: py_cheb(P8, K.ChebyshevPoly(4, 0.125, 2.0), x512)
    c["cheb_neither"] = lambda: py_cheb(P8, K.ChebyshevPoly(4), x512)
    c["cheb_max_only"] = lambda: py_cheb(P8, K.ChebyshevPoly(4, None, 1.875), x512)
    c["cheb_no_jacobi"] = lambda: py_cheb(P8, K.ChebyshevPoly(3, None, None, False), x512)
    c["cheb_knobs"] = lambda: py_cheb(P8, K.ChebyshevPoly(5, None, None, True, 6, 20.0, 1.25, 0x1234), x512)
    c["cheb_pcg"] = lambda: py_solve(K.PcgSolver(1e-8, 100), P8, K.ChebyshevPoly(4).setup(P8), b512, x512)
    c["cheb_build_stub"] = lambda: py_apply(K.PC.Chebyshev(3, 0.125, 12.0).build(P8), x512, zfill=0.5)      # the stub: tests/test_gpu_0_parity.py
    # MINRES / QMR / CGNR / CGNE: tests/test_gpu_krylov_ext.py
    c["minres"] = lambda: py_solve(K.MinresSolver(1e-8, 100), P8, None, b512, x512)
    c["minres_textbook"] = lambda: py_solve(K.MinresSolver(1e-8, 100).with_textbook(), P8, None, b512, x512)
    c["qmr"] = lambda: py_solve(K.QmrSolver(1e-8, 100), C9, None, b729, x729)
    c["cgnr"] = lambda: py_solve(K.CgnrSolver(1e-8, 60), C9, None, b729, x729)
    c["cgnr_textbook"] = lambda: py_solve(K.CgnrSolver(1e-8, 60).with_textbook(), C9, None, b729, x729)
    c["cgne"] = lambda: py_solve(K.CgneSolver(1e-8, 60), C9, None, b729, x729)
    # PcaGmresSolver: tests/test_gpu_pca_gmres.py
    pca = lambda restart=5, bs=1, tol=1e-6, mx=23: K.PcaGmresSolver(restart, 2, bs, tol, mx)
    c["pca_default_side"] = lambda: py_solve(pca(), C9, jac["C9"], b729, x729, extra={"side": I(pca().preconditioning)})
    c["pca_right"] = lambda: py_solve(pca().with_preconditioning(PCN.Right), C9, jac["C9"], b729, x729)
    c["pca_tau"] = lambda: py_solve(pca().with_preconditioning(PCN.Right).with_tau(0.5), C9, jac["C9"], b729, x729)
    c["pca_textbook"] = lambda: py_solve(pca(16, 4, 1e-8, 40).with_preconditioning(PCN.Right).with_textbook(), C9, jac["C9"], b729, x729)
    c["pca_block0"] = lambda: py_solve(pca(5, 0), C9, jac["C9"], b729, x729)
    c["pca_textbook_block0"] = lambda: py_solve(pca(16, 0, 1e-8, 40).with_preconditioning(PCN.Right).with_textbook(), C9, jac["C9"], b729, x729)
    # CbGmresSolver: tests/test_gpu_cb_gmres.py
    cb = lambda restart=5, tol=1e-10, mx=23: K.CbGmresSolver(restart, tol, mx)
    c["cb_f32_none_r5"] = lambda: py_solve(cb().with_preconditioning(PCN.NoPc), C9, None, b729, x729)
    c["cb_f64_none_r5"] = lambda: py_solve(cb().with_basis("f64").with_preconditioning(PCN.NoPc), C9, None, b729, x729)
    c["cb_f32_right_r30"] = lambda: py_solve(cb(30, 1e-8, 40).with_basis("f32").with_preconditioning(PCN.Right), C9, jac["C9"], b729, x729)
    c["cb_f64_right_r30"] = lambda: py_solve(cb(30, 1e-8, 40).with_basis("f64").with_preconditioning(PCN.Right), C9, jac["C9"], b729, x729)
    c["cb_f32_right_r5_t513"] = lambda: py_solve(cb().with_preconditioning(PCN.Right), T513, jac["T513"], fb(513), fx(513))
    c["cb_left"] = lambda: py_solve(cb().with_preconditioning(PCN.Left), C9, jac["C9"], b729, x729)
    c["cb_defaults"] = lambda: py_solve(cb(), C9, jac["C9"], b729, x729,
                                        extra={"side_basis": I(cb().preconditioning, K.CbGmresSolver.BASES[cb().basis])})
    # GMRES LeftTextbook, the CG builders, KspContext: tests/test_gpu_0_parity.py; FGMRES: tests/test_gpu_fgmres.py; CGS / TFQMR: tests/test_gpu_cgs_tfqmr.py
    c["gmres_left_textbook"] = lambda: py_solve(K.GmresSolver(10, 1e-8, 60).with_preconditioning(PCN.LeftTextbook), C9, jac["C9"], b729, x729)
    for name, nt in (("preconditioned", NORM.Preconditioned), ("unpreconditioned", NORM.Unpreconditioned), ("natural", NORM.Natural), ("none", NORM.NoNorm)):
        c[f"cg_norm_{name}"] = lambda nt=nt: py_solve(K.CgSolver(1e-8, 40).with_norm(nt), P8, None, b512, x512)
    c["cg_radius"] = lambda: py_solve(K.CgSolver(1e-8, 40).with_radius(64.0), P8, None, b512, np.zeros(512))
    c["cg_obj_target"] = lambda: py_solve(K.CgSolver(1e-8, 40).with_obj_target(-1000.0), P8, None, b512, np.zeros(512))
    c["pcg_norm_preconditioned"] = lambda: py_solve(K.PcgSolver(1e-8, 40).with_norm(NORM.Preconditioned), P8, jac["P8"], b512, x512)
    c["pcg_norm_natural"] = lambda: py_solve(K.PcgSolver(1e-8, 40).with_norm(NORM.Natural), P8, jac["P8"], b512, x512)
    c["fgmres_preallocate"] = lambda: py_solve(K.FgmresSolver(1e-8, 40, 10).with_preallocate(True), C9, jac["C9"], b729, x729)
    c["ksp_cgs"] = lambda: py_ksp(w, K.SolverKind.Cgs)
    c["ksp_tfqmr"] = lambda: py_ksp(w, K.SolverKind.Tfqmr)
    # history capacity (tol 1e-30, 23 iterations, restart 5): the same tests as the solvers above
    for name, (mk, a, pc) in cap_solvers().items():
        n = d[a].nrows()
        c["cap_" + name] = lambda mk=mk, a=a, pc=pc, n=n: py_solve(mk(), d[a], jac[a] if pc else None, fb(n), fx(n))
    # solver object state and the monitor: tests/test_gpu_0_parity.py (monitor, check_every), tests/test_gpu_krylov_ext.py, tests/test_gpu_cb_gmres.py
    c["state_two_solves"] = lambda: py_state(w)
    c["mon_minres"] = lambda: py_monitored(K.MinresSolver(1e-8, 100), P8, None, b512, x512, 0)
    c["mon_minres_every3"] = lambda: py_monitored(K.MinresSolver(1e-8, 100), P8, None, b512, x512, 3)
    c["mon_cb"] = lambda: py_monitored(cb(), C9, jac["C9"], b729, x729, 0)
    c["mon_cb_every3"] = lambda: py_monitored(cb(), C9, jac["C9"], b729, x729, 3)
    # mattransvec: tests/test_gpu_krylov_ext.py (spmv_transpose)
    c["mtv_rect"] = lambda: py_mtv(R35, fx(3), 5)
    c["mtv_convdiff"] = lambda: py_mtv(C9, x729, 729)
    c["mtv_swapped"] = lambda: py_mtv(R35, fx(5), 3)
    # the transport switches on one rank: tests/test_gpu_y_dist_single.py, tests/test_gpu_z_multirank_shim.py
    c["single_rank_modes"] = lambda: {"code": I(0), "peer_ipc": I(C9.halo_mode("peer") == "peer", w.ctx.scalar_reduce("ipc") == "ipc")}
    return c


def cap_solvers():
    """name -> (constructor, operator, with Jacobi): every solver class of the header, tol 1e-30, a cap of 23 that is no multiple of the restart 5
    (TFQMR on the tridiagonal of 513 rows: on convdiff 9^3 it breaks down after 13 iterations and would not reach the cap)"""
    t, m = 1e-30, 23
    return {"cg": (lambda: K.CgSolver(t, m), "P8", False), "pcg": (lambda: K.PcgSolver(t, m), "P8", True),
            "gmres": (lambda: K.GmresSolver(5, t, m), "C9", True), "fgmres": (lambda: K.FgmresSolver(t, m, 5), "C9", True),
            "bicgstab": (lambda: K.BiCgStabSolver(t, m), "C9", False), "cgs": (lambda: K.CgsSolver(t, m), "C9", False),
            "tfqmr": (lambda: K.TfqmrSolver(t, m), "T513", False), "minres": (lambda: K.MinresSolver(t, m), "P8", False),
            "minres_textbook": (lambda: K.MinresSolver(t, m).with_textbook(), "P8", False), "qmr": (lambda: K.QmrSolver(t, m), "C9", False),
            "cgnr": (lambda: K.CgnrSolver(t, m), "C9", False), "cgnr_textbook": (lambda: K.CgnrSolver(t, m).with_textbook(), "C9", False),
            "cgne": (lambda: K.CgneSolver(t, m), "C9", False),
            "pca": (lambda: K.PcaGmresSolver(5, 2, 1, t, m).with_preconditioning(PCN.Right), "C9", True),
            "pca_textbook": (lambda: K.PcaGmresSolver(5, 2, 2, t, m).with_preconditioning(PCN.Right).with_textbook(), "C9", True),
            "cb": (lambda: K.CbGmresSolver(5, t, m), "C9", True)}


# the error cases: name -> KError code; a solve or apply among them leaves its vector as it was given
ERRORS = {"amg_default_pcg": 4, "sor_colors_wrong_length": 102, "spai_auto": 6, "cheb_build_stub": 2, "pca_block0": 102, "pca_textbook_block0": 102,
          "cb_left": 6, "mtv_swapped": 102}
# CG as written stops after its first step under these two norms whatever the system (cg.rs:224-229: Natural takes sqrt|r_new . p_old|, which
# conjugacy makes a rounding error; NoNorm takes 0), so "at least two iterations" cannot be asked of them: one step, two history entries and
# an x that moved in nearly every entry are asked instead
ONE_STEP = ("cg_norm_natural", "cg_norm_none")
# pairs that must be the same bits although they are built differently
SAME = [("bj_build_apply", "bj_apply"), ("bj_build_pcg", "bj_pcg"), ("sor_setters_apply", "sor_sym_apply"), ("sor_moved_apply", "sor_sym_apply"),
        ("spai_build_apply", "spai_operator"), ("pca_tau", "pca_right"), ("cgne", "cgnr"), ("cb_defaults", "mon_cb"), ("mon_cb_every3", "mon_cb"), ("mon_minres", "minres"),
        ("mon_minres_every3", "minres")]
CASE_NAMES = sorted([
    "bj_explicit_apply", "bj_uniform8_apply", "bj_uniform1_apply", "bj_apply", "bj_pcg", "bj_build_apply", "bj_build_pcg",
    *[f"asm_{n}_{k}" for n in ("written", "nparts0", "nparts3", "grown", "restricted", "ilu_true", "ilu_ilup0", "ilu_default") for k in ("apply", "gmres")
      if (n, k) != ("nparts0", "gmres")],
    "sor_sym_apply", "sor_lower_apply", "sor_upper_zero_apply", "sor_colors_apply", "sor_setters_apply", "sor_colors_wrong_length", "sor_moved_apply",
    "sor_gmres",
    "amg_default_apply", "amg_l2_apply", "amg_default_pcg", "amg_l2_pcg",
    "spai_manual", "spai_operator", "spai_operator_pcg", "spai_auto", "spai_build_apply",
    *[f"spec_j{j}_s{s}" for j in (1, 0) for s in (1, 10, 64)], "spec_t10_s64",
    "cheb_both", "cheb_neither", "cheb_max_only", "cheb_no_jacobi", "cheb_knobs", "cheb_pcg", "cheb_build_stub",
    "minres", "minres_textbook", "qmr", "cgnr", "cgnr_textbook", "cgne",
    "pca_default_side", "pca_right", "pca_tau", "pca_textbook", "pca_block0", "pca_textbook_block0",
    "cb_f32_none_r5", "cb_f64_none_r5", "cb_f32_right_r30", "cb_f64_right_r30", "cb_f32_right_r5_t513", "cb_left", "cb_defaults",
    "gmres_left_textbook", "cg_norm_preconditioned", "cg_norm_unpreconditioned", "cg_norm_natural", "cg_norm_none", "cg_radius", "cg_obj_target",
    "pcg_norm_preconditioned", "pcg_norm_natural", "fgmres_preallocate", "ksp_cgs", "ksp_tfqmr",
    *["cap_" + n for n in cap_solvers()],
    "state_two_solves", "mon_minres", "mon_minres_every3", "mon_cb", "mon_cb_every3", "mtv_rect", "mtv_convdiff", "mtv_swapped", "single_rank_modes"])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


def differences(got, want):
    out = []
    if sorted(got) != sorted(want):
        return [("fields", sorted(got), sorted(want))]
    for k in want:
        if not same_bits(got[k], want[k]):
            g, x = np.asarray(got[k]), np.asarray(want[k])
            at = np.flatnonzero(g[:min(len(g), len(x))] != x[:min(len(g), len(x))])[:3]
            out.append((k, "lengths", len(g), len(x), "first at", at.tolist(), g[at].tolist() if len(at) else g[:3].tolist(),
                        x[at].tolist() if len(at) else x[:3].tolist()))
    return out


def expected(w, name):
    if name not in w.cache:
        if "cases" not in w.__dict__:
            w.cases = cases(w)
        w.cache[name] = w.cases[name]()
    return w.cache[name]


def start_vector(name, e):
    """what the case's x / z / y held before the call"""
    if "y" in e:
        return np.full(len(e["y"]), 0.5)
    if "z" in e:
        return np.full(len(e["z"]), 0.5 if name == "cheb_build_stub" else 0.0)
    return np.zeros(len(e["x"])) if name in ("cg_radius", "cg_obj_target", "amg_default_pcg", "amg_l2_pcg") else fx(len(e["x"]))


# ----------------------------------------------------------------------------- the tests
def test_every_case_was_written(W):
    assert len(set(CASE_NAMES)) == len(CASE_NAMES) and sorted(cases(W)) == CASE_NAMES
    assert W.done == len(CASE_NAMES), (W.done, len(CASE_NAMES))
    assert sorted(W.recs) == CASE_NAMES, (sorted(set(CASE_NAMES) - set(W.recs)), sorted(set(W.recs) - set(CASE_NAMES)))
    print(f"child process: {W.child_seconds:.2f} s for {W.done} cases")


def family(name):
    head = name.split("_")[0]
    return {"minres": "krylov", "qmr": "krylov", "cgnr": "krylov", "cgne": "krylov", "cg": "builders", "pcg": "builders", "gmres": "builders",
            "fgmres": "builders", "ksp": "builders", "state": "state", "mon": "state", "single": "state"}.get(head, head)


FAMILIES = sorted({family(n) for n in CASE_NAMES})


def check_case(W, name):
    """-> the list of what is wrong with one case (empty: the header gave the binding's bits, and the expectation is not vacuous)"""
    if name not in W.recs:
        return [(name, "the child wrote no record for this case")]
    got, e = W.recs[name], expected(W, name)
    code, bad = int(e["code"][0]), []
    if not (code == ERRORS.get(name, 0) or name.startswith("cap_")):         # (a cap case may end in the solver's own breakdown error)
        bad.append((name, "the binding's code", code))
    if code != 0 and any(k in e for k in ("x", "z", "y")) and not same_bits(e.get("x", e.get("z", e.get("y"))), start_vector(name, e)):
        bad.append((name, "the binding's error case changed its vector"))
    if code != 0 and "hist" in e and name == "amg_default_pcg" and len(e["hist"]) < 3:
        bad.append((name, "the run that ends in the error is shorter than two iterations", len(e["hist"])))
    if code == 0 and name in ONE_STEP:
        if not (int(e["iterations"][0]) == 1 and len(e["hist"]) == 2 and np.sum(e["x"] != fx(512)) >= 500):
            bad.append((name, "not the one step expected", e["iterations"], len(e["hist"])))
    elif code == 0 and "iterations" in e and not (int(e["iterations"][0]) >= 2 and ("hist" not in e or len(e["hist"]) >= 2)):
        bad.append((name, "vacuous: fewer than two iterations", e["iterations"], len(e.get("hist", []))))
    if code == 0 and "z" in e and not (np.any(e["z"] != fx(len(e["z"]))) and np.any(e["z"] != 0.0)):
        bad.append((name, "vacuous: z is r or zero"))
    if code == 0 and "y" in e and not (np.any(e["y"] != 0.5) and np.any(e["y"] != 0.0)):
        bad.append((name, "vacuous: y was not written"))
    if name.startswith("mon_") and code == 0 and not (len(e["mon_i"]) >= 2 and len(e["mon_i"]) == len(e["mon_r"])):
        bad.append((name, "vacuous: the monitor did not fire"))
    return bad + [(name,) + d for d in differences(got, e)]


@pytest.mark.parametrize("fam", FAMILIES)
def test_header_gives_the_bindings_bits(W, fam):
    bad = [b for name in CASE_NAMES if family(name) == fam for b in check_case(W, name)]
    assert not bad, "\n".join(str(b) for b in bad)


def test_two_routes_one_result(W):
    """PC::build against the class, setters against the constructor, defaults against explicit arguments, a monitor against none"""
    for name, other in SAME:
        a, b = W.recs[name], W.recs[other]
        for k in ("code", "iterations", "converged", "final", "hist", "x", "z"):
            if k in a or k in b:
                assert k in a and k in b and same_bits(a[k], b[k]), (name, other, k)


def test_history_lengths_are_not_truncated(W):
    """tol 1e-30 and 23 iterations: every class records what Python records; TFQMR (two entries per iteration) is the tightest"""
    for n in cap_solvers():
        got, e = W.recs["cap_" + n], expected(W, "cap_" + n)
        assert len(got["hist"]) == len(e["hist"]), (n, len(got["hist"]), len(e["hist"]))
    e = expected(W, "cap_tfqmr")                        # on the tridiagonal it runs to the cap: more than a one-entry-per-iteration buffer holds
    assert int(e["code"][0]) == 0 and int(e["iterations"][0]) == 23 and len(e["hist"]) > 23 + 5 + 8


def test_state_and_modes(W):
    s = W.recs["state_two_solves"]
    assert s["lengths"][1] > s["lengths"][0] >= 2 and len(s["hist"]) == s["lengths"][1] and s["after_clear"][0] == 0
    assert same_bits(s["hist"][:s["lengths"][0]], W.recs["minres"]["hist"])
    m = W.recs["mon_minres_every3"]                       # check_every batches the callbacks; the sequence is every iteration, in order
    assert list(m["mon_i"]) == list(range(len(m["hist"]))) and same_bits(m["mon_r"], m["hist"])
    assert same_bits(W.recs["cb_defaults"]["side_basis"], I(PCN.Right, 1))
    assert same_bits(W.recs["pca_default_side"]["side"], I(PCN.Left))
    z = W.recs["bj_explicit_apply"]["z"]
    assert same_bits(z[6:7], D(0.0)) and np.all(z[[0, 1, 2, 3, 4, 5, 7, 8, 9]] != 0.0)       # the row in no block
    b = W.recs["cheb_neither"]["bounds"]
    assert b[0] == b[1] / 30.0 and not same_bits(b, W.recs["cheb_knobs"]["bounds"])


# ----------------------------------------------------------------------------- the restatements, against the C++ records directly
def restatements(w):
    o, oj, rs = w.o, w.ojac, w.rs
    b512, x512, b729, x729 = fb(512), fx(512), fb(729), fx(729)
    kr = lambda n, a, b, x, tol, mx: KR.SOLVERS[n](o[a], b, x.copy(), tol, mx, rs)
    osolve = lambda m, a, b, x, **kw: O.solve(m, o[a], b, x0=x, rs=rs, raise_on_error=False, **kw)
    cbg = lambda a, b, x, pc, side, restart, tol, mx, basis: CB.cbgmres(o[a], b, x, pc=pc, side=side, restart=restart, tol=tol, max_iters=mx, basis=basis)
    r = {}
    r["minres"] = lambda: kr("minres", "P8", b512, x512, 1e-8, 100)
    r["minres_textbook"] = lambda: kr("minres_textbook", "P8", b512, x512, 1e-8, 100)
    r["qmr"] = lambda: kr("qmr", "C9", b729, x729, 1e-8, 100)
    r["cgnr"] = lambda: kr("cgnr", "C9", b729, x729, 1e-8, 60)
    r["cgne"] = lambda: kr("cgnr", "C9", b729, x729, 1e-8, 60)
    r["cgnr_textbook"] = lambda: kr("cgnr_textbook", "C9", b729, x729, 1e-8, 60)
    r["pca_default_side"] = lambda: PR.as_written(o["C9"], b729, x729, pc=oj["C9"], side=1, restart=5, tol=1e-6, max_iters=23, rs=rs)
    r["pca_right"] = lambda: PR.as_written(o["C9"], b729, x729, pc=oj["C9"], side=2, restart=5, tol=1e-6, max_iters=23, rs=rs)
    r["pca_tau"] = r["pca_right"]
    r["pca_textbook"] = lambda: PR.sstep(o["C9"], b729, x729, pc=oj["C9"], side=2, restart=16, block_size=4, tol=1e-8, max_iters=40, rs=rs)
    r["cap_pca"] = lambda: PR.as_written(o["C9"], b729, x729, pc=oj["C9"], side=2, restart=5, tol=1e-30, max_iters=23, rs=rs)
    r["cap_pca_textbook"] = lambda: PR.sstep(o["C9"], b729, x729, pc=oj["C9"], side=2, restart=5, block_size=2, tol=1e-30, max_iters=23, rs=rs)
    r["cb_f32_none_r5"] = lambda: cbg("C9", b729, x729, None, 0, 5, 1e-10, 23, "f32")
    r["cb_f64_none_r5"] = lambda: cbg("C9", b729, x729, None, 0, 5, 1e-10, 23, "f64")
    r["cb_f32_right_r30"] = lambda: cbg("C9", b729, x729, oj["C9"], 2, 30, 1e-8, 40, "f32")
    r["cb_f64_right_r30"] = lambda: cbg("C9", b729, x729, oj["C9"], 2, 30, 1e-8, 40, "f64")
    r["cb_f32_right_r5_t513"] = lambda: cbg("T513", fb(513), fx(513), oj["T513"], 2, 5, 1e-10, 23, "f32")
    r["cb_defaults"] = lambda: cbg("C9", b729, x729, oj["C9"], 2, 5, 1e-10, 23, "f32")
    r["mon_cb"] = r["mon_cb_every3"] = r["cb_defaults"]
    r["cap_cb"] = lambda: cbg("C9", b729, x729, oj["C9"], 2, 5, 1e-30, 23, "f32")
    r["gmres_left_textbook"] = lambda: osolve("gmres", "C9", b729, x729, pc=oj["C9"], tol=1e-8, max_iters=60, restart=10, side=O.SIDE_LEFT_TEXTBOOK)
    for k, name in enumerate(("preconditioned", "unpreconditioned", "natural", "none")):
        r[f"cg_norm_{name}"] = lambda k=k: osolve("cg", "P8", b512, x512, tol=1e-8, max_iters=40, norm_type=k)
    r["cg_radius"] = lambda: osolve("cg", "P8", b512, np.zeros(512), tol=1e-8, max_iters=40, radius=64.0)
    r["cg_obj_target"] = lambda: osolve("cg", "P8", b512, np.zeros(512), tol=1e-8, max_iters=40, obj_target=-1000.0)
    r["pcg_norm_preconditioned"] = lambda: osolve("pcg", "P8", b512, x512, pc=oj["P8"], tol=1e-8, max_iters=40, norm_type=0)
    r["pcg_norm_natural"] = lambda: osolve("pcg", "P8", b512, x512, pc=oj["P8"], tol=1e-8, max_iters=40, norm_type=2)
    r["fgmres_preallocate"] = lambda: osolve("fgmres", "C9", b729, x729, pc=oj["C9"], tol=1e-8, max_iters=40, restart=10, preallocate=True)
    r["ksp_cgs"] = lambda: osolve("cgs", "C9", b729, x729, pc=oj["C9"], tol=1e-8, max_iters=40)
    r["ksp_tfqmr"] = lambda: osolve("tfqmr", "C9", b729, x729, pc=oj["C9"], tol=1e-8, max_iters=40)
    r["cap_cg"] = lambda: osolve("cg", "P8", b512, x512, tol=1e-30, max_iters=23)
    r["cap_pcg"] = lambda: osolve("pcg", "P8", b512, x512, pc=oj["P8"], tol=1e-30, max_iters=23)
    r["cap_gmres"] = lambda: osolve("gmres", "C9", b729, x729, pc=oj["C9"], tol=1e-30, max_iters=23, restart=5, side=O.SIDE_LEFT)
    r["cap_fgmres"] = lambda: osolve("fgmres", "C9", b729, x729, pc=oj["C9"], tol=1e-30, max_iters=23, restart=5)
    r["cap_bicgstab"] = lambda: osolve("bicgstab", "C9", b729, x729, tol=1e-30, max_iters=23)
    r["cap_cgs"] = lambda: osolve("cgs", "C9", b729, x729, tol=1e-30, max_iters=23)
    r["cap_tfqmr"] = lambda: osolve("tfqmr", "T513", fb(513), fx(513), tol=1e-30, max_iters=23)
    r["cap_minres"] = lambda: kr("minres", "P8", b512, x512, 1e-30, 23)
    r["cap_minres_textbook"] = lambda: kr("minres_textbook", "P8", b512, x512, 1e-30, 23)
    r["cap_qmr"] = lambda: kr("qmr", "C9", b729, x729, 1e-30, 23)
    r["cap_cgnr"] = lambda: kr("cgnr", "C9", b729, x729, 1e-30, 23)
    r["cap_cgne"] = r["cap_cgnr"]
    r["cap_cgnr_textbook"] = lambda: kr("cgnr_textbook", "C9", b729, x729, 1e-30, 23)
    return r


RESTATED = sorted([
    "minres", "minres_textbook", "qmr", "cgnr", "cgne", "cgnr_textbook", "pca_default_side", "pca_right", "pca_tau", "pca_textbook", "cap_pca",
    "cap_pca_textbook", "cb_f32_none_r5", "cb_f64_none_r5", "cb_f32_right_r30", "cb_f64_right_r30", "cb_f32_right_r5_t513", "cb_defaults", "mon_cb",
    "mon_cb_every3", "cap_cb", "gmres_left_textbook", "cg_norm_preconditioned", "cg_norm_unpreconditioned", "cg_norm_natural", "cg_norm_none",
    "cg_radius", "cg_obj_target", "pcg_norm_preconditioned", "pcg_norm_natural", "fgmres_preallocate", "ksp_cgs", "ksp_tfqmr", "cap_cg", "cap_pcg",
    "cap_gmres", "cap_fgmres", "cap_bicgstab", "cap_cgs", "cap_tfqmr", "cap_minres", "cap_minres_textbook", "cap_qmr", "cap_cgnr", "cap_cgne",
    "cap_cgnr_textbook"])


def restated_fields(res, with_hist):
    out = {"code": I(getattr(res, "code", 0))}
    if int(out["code"][0]) == 0:
        out.update(iterations=I(res.iterations), converged=I(bool(res.converged)), final=D(res.final_residual))
    if with_hist:
        out["hist"] = np.array(res.history, dtype=np.float64)
    out["x"] = np.asarray(res.x, dtype=np.float64)
    return out


@pytest.mark.parametrize("fam", sorted({family(n) for n in RESTATED}))
def test_header_gives_the_restatements_bits(W, fam):
    if "restatements" not in W.__dict__:
        W.restatements = restatements(W)
        assert sorted(W.restatements) == RESTATED
    bad = []
    for name in (n for n in RESTATED if family(n) == fam):
        got = W.recs[name]
        want = restated_fields(W.restatements[name](), "hist" in got)
        bad += [(name,) + d for d in differences({k: got[k] for k in want if k in got}, want)]
    assert not bad, "\n".join(str(b) for b in bad)
