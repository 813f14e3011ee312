"""One rank of a case of tests/multirank_ext_cases.py (sections A to D), started by tests/test_gpu_z_multirank_shim.py:

    multirank_ext_worker.py <rank> <P> <outdir> <section> <case>

The rendezvous, the stage markers and the result file per rank are tests/multirank_worker.py's.  A rank never stops at a mismatch it finds
itself (its peers would wait for it inside the next collective): it notes the mismatch, goes on to the barrier and fails after it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kryst_amd as K                                              # noqa: E402
from multirank_worker import make_context, save_rank, stage        # noqa: E402
import multirank_ext_cases as M                                    # noqa: E402
from nonfinite_cases import same_ieee                              # noqa: E402


def bits_equal(u, v):
    u, v = np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    return u.shape == v.shape and bool(np.array_equal(u.view(np.uint64), v.view(np.uint64)))


def run_solve(ctx, s, a, pc, b, x0):
    """-> (stats = [code, iterations, converged, final_residual], history, x after the call)"""
    s.clear_history()
    x = ctx.vec(np.ascontiguousarray(x0, dtype=np.float64))
    try:
        st, code = s.solve(a, pc, b, x), 0
    except K.KError as e:
        if e.stats is None:
            raise
        st, code = e.stats, e.code
    return np.array([code, st.iterations, float(st.converged), st.final_residual]), np.array(s.residual_history, dtype=np.float64), x.to_host()


class Rank:
    def __init__(self, rank, P, outdir):
        self.rank, self.P, self.outdir = rank, P, outdir
        stage(rank, "start")
        self.ctx = make_context(rank, P, outdir)
        self.out = {}
        self.mismatches = []
        self.active = {"ipc": 1, "peer": 1}

    def device_operator(self, spec):
        """the rank's rows of the operator: the device generator for the stencils, the index-list exchange for everything else"""
        if spec[0] == "stencil":
            return K.CsrMatrix.stencil7(spec[1], spec[2], ctx=self.ctx)
        a = M.operator(spec)
        offs = M.offsets(spec, self.P)
        rp, ci, va = M.local_rows(a, offs, self.rank)
        return K.CsrMatrix.from_csr_dist(self.ctx, a.nrows, offs, rp, ci, va)

    def local(self, spec, v):
        offs = M.offsets(spec, self.P)
        return np.ascontiguousarray(v[int(offs[self.rank]):int(offs[self.rank + 1])])

    def transport(self, scal, halo, operators):
        """switch the scalar all-reduce and every operator's halo exchange; False (and noted) where a hipIpc form cannot be had"""
        stage(self.rank, f"transport scalars {scal}, halo {halo}")
        ok = True
        if self.ctx.scalar_reduce(scal) != scal:
            self.active["ipc"], ok = 0, False
        for a in operators:
            if a.halo_mode(halo) != halo:
                self.active["peer"], ok = 0, False
        return ok

    def keep(self, key, stats, hist, x, first, nan_ok=False):
        """store the first run's results; note where a later transport gives other bits"""
        eq = same_ieee if nan_ok else bits_equal
        if first:
            self.out[key + "__stats"], self.out[key + "__hist"], self.out[key + "__x"] = stats, hist, x
        elif not (eq(stats, self.out[key + "__stats"]) and eq(hist, self.out[key + "__hist"]) and eq(x, self.out[key + "__x"])):
            self.mismatches.append(key)
            print(f"[rank {self.rank}] TRANSPORT MISMATCH {key}: stats {stats} / {self.out[key + '__stats']}, history lengths {len(hist)} / "
                  f"{len(self.out[key + '__hist'])}, {int(np.sum(x != self.out[key + '__x']))} x entries differ", flush=True)

    def finish(self):
        stage(self.rank, "barrier")
        self.ctx.barrier()
        self.out["ipc_active"] = np.array([self.active["ipc"]])
        self.out["peer_active"] = np.array([self.active["peer"]])
        self.out["mismatches"] = np.array([len(self.mismatches)])
        save_rank(self.outdir, self.rank, self.out)
        assert not self.mismatches, self.mismatches


# ------------------------------------------------------------------------------------------------ A
def section_a(w, case):
    c = M.A_CASES[case]
    spec = c["op"]
    stage(w.rank, "operator")
    a = w.device_operator(spec)
    g = M.operator(spec)
    w.out["nloc"] = np.array([a.nrows()])
    b = w.ctx.vec(w.local(spec, M.rhs(g)))
    x0 = w.local(spec, M.guess(g))
    for ti, (scal, halo) in enumerate(M.a_transports(case)):
        if not w.transport(scal, halo, [a]):
            continue
        for method in c["solvers"]:
            for j, (tol, mx) in enumerate(M.A_PARAMS):
                stage(w.rank, f"{scal}+{halo} solve {method} tol {tol} max_iters {mx}")
                w.keep(f"{method}_{j}", *run_solve(w.ctx, M.make_solver(method, tol, mx), a, None, b, x0), first=ti == 0, nan_ok=method in M.NAN_OK)
        if not c["sessions"]:
            continue
        for method in M.SESSION_METHODS:
            tol = M.session_tol(case, method)
            stage(w.rank, f"{scal}+{halo} whole solve and session {method} tol {tol}")
            w.keep(f"whole_{method}", *run_solve(w.ctx, M.make_solver(method, tol, M.SESSION_MAX_ITERS), a, None, b, x0), first=ti == 0,
                   nan_ok=method in M.NAN_OK)
            x = w.ctx.vec(x0)
            code = 0
            with K.Session(method, a, None, b, x, tol, M.SESSION_MAX_ITERS) as sess:
                for k in M.SESSION_STEPS + (M.SESSION_MAX_ITERS - sum(M.SESSION_STEPS),):
                    sess.step(k)
                try:
                    st = sess.end()
                except K.KError as e:
                    if e.stats is None:
                        raise
                    st, code = e.stats, e.code
            w.keep(f"sess_{method}", np.array([code, st.iterations, float(st.converged), st.final_residual]),
                   np.array(sess.residual_history, dtype=np.float64), x.to_host(), first=ti == 0, nan_ok=method in M.NAN_OK)


# ------------------------------------------------------------------------------------------------ B
def section_b(w, case):
    spec = M.B_CASES[case]["op"]
    stage(w.rank, "operator")
    a = w.device_operator(spec)
    g = M.operator(spec)
    b = w.ctx.vec(w.local(spec, M.rhs(g)))
    r = w.local(spec, M.b_apply_input(g))
    zero = np.zeros(a.nrows())
    stage(w.rank, "estimate_spectrum")
    try:
        K.estimate_spectrum(a)
        w.out["estimate_code"] = np.array([0])
    except K.KError as e:
        w.out["estimate_code"] = np.array([e.code])
    for ti, (scal, halo) in enumerate((M.TRANSPORTS[0], M.TRANSPORTS[3])):
        if not w.transport(scal, halo, [a]):
            continue
        for jac in M.B_SCALINGS:
            lo, hi = M.b_bounds(g, jac)
            for deg in M.B_DEGREES:
                key = f"{'jacobi' if jac else 'none'}_{deg}"
                stage(w.rank, f"{scal}+{halo} ChebyshevPoly {key}")
                pc = K.ChebyshevPoly(deg, lo, hi, jacobi=jac).setup(a)
                if ti == 0:
                    w.out[key + "__fused"] = np.array([int(bool(pc.info()["fused"]))])
                z = np.asarray(pc.apply(r))
                w.keep(key + "_apply", np.zeros(4), np.zeros(0), z, first=ti == 0)
                stage(w.rank, f"{scal}+{halo} pcg {key}")
                w.keep(key + "_pcg", *run_solve(w.ctx, K.PcgSolver(*M.B_PCG), a, pc, b, zero), first=ti == 0)
                stage(w.rank, f"{scal}+{halo} gmres {key}")
                s = K.GmresSolver(*M.B_GMRES).with_preconditioning(K.Preconditioning.Right)
                w.keep(key + "_gmres", *run_solve(w.ctx, s, a, pc, b, zero), first=ti == 0)
                stage(w.rank, f"{scal}+{halo} fgmres {key}")
                w.keep(key + "_fgmres", *run_solve(w.ctx, K.FgmresSolver(*M.B_FGMRES), a, pc, b, zero), first=ti == 0)
                del pc


# ------------------------------------------------------------------------------------------------ C
class Usable:
    """ctx.all_reduce(rank + 1) and a plain CG solve on the context: right bits only if no rank is a collective ahead of the others"""

    def __init__(self, w, a, b):
        self.w, self.a, self.b, self.first = w, a, b, None
        self.names, self.ok = [], []

    def check(self, after):
        w = self.w
        ar = w.ctx.all_reduce(float(w.rank + 1))
        got = run_solve(w.ctx, K.CgSolver(*M.C_USE), self.a, None, self.b, np.zeros(self.a.nrows()))
        if self.first is None:
            self.first = got
            w.out["use__stats"], w.out["use__hist"], w.out["use__x"] = got
        ok = ar == w.P * (w.P + 1) / 2 and all(bits_equal(u, v) for u, v in zip(got, self.first))
        if not ok:
            print(f"[rank {w.rank}] CONTEXT NOT USABLE after {after}: all_reduce {ar}, CG stats {got[0]} / {self.first[0]}", flush=True)
        self.names.append(after)
        self.ok.append(int(ok))

    def store(self):
        self.w.out["use_ok"] = np.array(self.ok)
        self.w.out["use_after"] = np.array(self.names)


def section_c(w, case):
    scal, halo = case.split("+")
    stage(w.rank, "operators")
    a = w.device_operator(M.C_OP)
    ai = w.device_operator(M.C_INDEFINITE)
    g, gi = M.operator(M.C_OP), M.operator(M.C_INDEFINITE)
    pcs = {id(a): K.Jacobi().setup(a), id(ai): K.Jacobi().setup(ai)}
    w.transport(scal, halo, [a, ai])
    b = w.ctx.vec(w.local(M.C_OP, M.rhs(g)))
    zero = np.zeros(a.nrows())
    use = Usable(w, a, b)
    use.check("start")

    def one(key, method, op, rhs_, x0, tol, mx, chk):
        s = M.make_solver(method, tol, mx)
        s.check_every = chk
        stats, hist, x = run_solve(w.ctx, s, op, pcs[id(op)] if method == "pcg" else None, rhs_, x0)
        w.out[key + "__stats"], w.out[key + "__hist"], w.out[key + "__x"] = stats, hist, x
        use.check(key)

    for method, k, tol in M.c_stop_cases():
        for chk in (M.C_CHECK_EVERY if method != "gmres5" else (0,)):
            stage(w.rank, f"stop {method} k={k} check_every={chk}")
            one(f"stop_{method}_{k}_{chk}", method, a, b, zero, tol, M.C_MAX_ITERS, chk)
    bi = w.ctx.vec(w.local(M.C_OP, M.rhs(gi)))
    x0 = w.local(M.C_OP, M.guess(gi))
    for method in M.C_ERROR_METHODS:
        for chk in M.C_CHECK_EVERY:
            stage(w.rank, f"indefinite {method} check_every={chk}")
            one(f"indef_{method}_{chk}", method, ai, bi, x0, 1e-8, 50, chk)
    for which in M.C_DEGENERATE:
        bb, xx, tol, mx = M.c_degenerate_problem(which)
        for method in M.C_DEGENERATE_METHODS[which]:
            stage(w.rank, f"{which} {method}")
            one(f"{which}_{method}", method, a, w.ctx.vec(w.local(M.C_OP, bb)), w.local(M.C_OP, xx), tol, mx, 0)
    use.store()


# ------------------------------------------------------------------------------------------------ D
def section_d(w, case):
    stage(w.rank, "operator")
    dd = w.device_operator(M.D_OP)
    g = M.operator(M.D_OP)
    b = w.ctx.vec(w.local(M.D_OP, M.rhs(g)))
    use = Usable(w, dd, b)
    use.check("start")
    stage(w.rank, "refusals")
    res = M.run_refusals(w.ctx, dd, list(M.D_ENTRIES))
    for name, (code, msg, same) in res.items():
        stage(w.rank, f"refused {name}: {code} {msg!r} untouched={same}")
    w.out["d_names"] = np.array(list(res))
    w.out["d_codes"] = np.array([res[n][0] for n in res])
    w.out["d_msgs"] = np.array([res[n][1] for n in res])
    w.out["d_same"] = np.array([int(res[n][2]) for n in res])
    use.check("refusals")
    use.store()


def main():
    rank, P, outdir, section, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    w = Rank(rank, P, outdir)
    {"A": section_a, "B": section_b, "C": section_c, "D": section_d}[section](w, case)
    w.finish()


if __name__ == "__main__":
    main()
