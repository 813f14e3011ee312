// Device-resident BiCGStab: LinearSolver::solve (src/solver/mod.rs:30-52) for a HIP CSR operator.  The solver restates its
// reference file operation by operation (line numbers cited inline); the vector work is fused into as few HBM passes as the
// data dependences allow without changing any rounding.
#include "solvers.h"

namespace kr {

// =================================================================== BiCGStab (src/solver/bicgstab.rs:69-293)
template <bool KEEP = false>
struct BicgPOp {                     // p = r + beta*(p - omega_prev*v)   (bicgstab.rs:134/140)
    static constexpr int NQ = 0; static constexpr const char* TAG = "BicgP";
    const DevState* st; const double* r; const double* v; double* p;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double be = st->beta, om = st->omega_prev;
        const d2 rr = ld2_sel<KEEP>(r, i), vv = ld2(v, i), pp = ld2(p, i);      // r was written by the launch before this one
        st2(p, i, rr.a + be * (pp.a - om * vv.a), rr.b + be * (pp.b - om * vv.b));
    }
};
struct BicgSOp {                     // s = r - alpha*v ; partial s.s     (bicgstab.rs:166-188)
    static constexpr int NQ = 1; static constexpr const char* TAG = "BicgS"; static constexpr int BPC = 4;      // tools/solver_ab.py: 2 -> 4 workgroups per CU, BiCGStab +4.5 % (256^3), +2.0 % (512^3)
    const DevState* st; const double* r; const double* v; double* s;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double al = st->alpha;
        const d2 rr = ld2(r, i), vv = ld2(v, i);
        const double s0 = rr.a - al * vv.a, s1 = rr.b - al * vv.b;
        st2(s, i, s0, s1);
        if (in0) acc[0] = acc[0] + s0 * s0;
        if (in1) acc[0] = acc[0] + s1 * s1;
    }
};
// x = x + alpha*p + omega*s ; r = s - omega*t ; partials r.r and rhat.r (the next rho)   (bicgstab.rs:240-279,105-116)
// when the s-norm exit is pending (st->early): only x = x + alpha*p   (bicgstab.rs:191-202)
template <bool KEEP = false>
struct BicgXROp {
    static constexpr int NQ = 2; static constexpr const char* TAG = "BicgXR"; static constexpr int BPC = 3;     // 2 -> 3: +5.2 % (256^3), +3.0 % (512^3)
    // p / sx: the directions x is updated with (M^-1 p, M^-1 s in the right-preconditioned extension); s: the true s
    const DevState* st; const double* p; const double* sx; const double* s; const double* t; const double* rhat; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const double al = st->alpha;
        const d2 pp = ld2(p, i), xx = ld2(x, i);
        if (st->early) { st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b); return; }
        const double om = st->omega;
        const d2 ss = ld2(s, i), tt = ld2(t, i), hh = ld2(rhat, i);
        d2 sd = ss;
        if (sx != s) sd = ld2(sx, i);
        st2(x, i, xx.a + al * pp.a + om * sd.a, xx.b + al * pp.b + om * sd.b);
        const double r0 = ss.a - om * tt.a, r1 = ss.b - om * tt.b;
        st2_sel<KEEP>(r, i, r0, r1);
        if (in0) { acc[0] = acc[0] + r0 * r0; acc[1] = acc[1] + hh.a * r0; }
        if (in1) { acc[0] = acc[0] + r1 * r1; acc[1] = acc[1] + hh.b * r1; }
    }
};
struct BicgInitLogic {               // bicgstab.rs:79-102 ; red0 = (r,r) = (rhat,r)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        st->res0 = dsqrt(red[0]);
        st->iterations = 0; st->final_residual = st->res0; st->converged = 0; st->iter = 0;
        st->rho_prev = 1.0; st->alpha = 1.0; st->omega_prev = 1.0;
        c.push(st->res0);
        if (st->res0 <= c.tol) { st->converged = 1; c.finish(KRYST_OK); return; }   // :98-102 absolute tolerance
        if (c.max_iters <= 0) { c.finish(KRYST_OK); return; }
        st->rho = red[0];                                              // i = 1: rho = (rhat, r), rhat == r
        if (fabs(st->rho) < DBL_EPSILON) { c.finish(KRYST_OK); return; }   // :117-119 break
        st->beta = 0.0;                                                // :120-121
    }
};
struct BicgAlphaLogic {              // bicgstab.rs:149-164 ; red0 = (rhat, v)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double alpha_den = red[0];
        if (fabs(alpha_den) < DBL_EPSILON) { c.finish(KRYST_OK); return; }   // :161-163 break (stats unchanged)
        st->alpha = st->rho / alpha_den;
    }
};
struct BicgSLogic {                  // bicgstab.rs:177-206 ; red0 = (s,s)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double s_norm = dsqrt(red[0]);
        if (s_norm <= c.tol) {
            st->iterations = st->iter + 1; st->final_residual = s_norm; st->converged = 1;
            c.push(s_norm);
            st->early = 1;
            c.finish(KRYST_OK);
        }
    }
};
struct BicgOmegaLogic {              // bicgstab.rs:211-238 ; red0 = (t,s), red1 = (t,t)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        if (fabs(red[1]) < DBL_EPSILON) { c.finish(KRYST_OK); return; }   // :235-237 break
        st->omega = red[0] / red[1];
    }
};
struct BicgEndLogic {                // bicgstab.rs:268-289 then the head of the next iteration :105-124
    static constexpr bool RUN_WHEN_DONE = true;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        if (st->early) { st->early = 0; return; }
        if (st->done) return;
        const long long i = st->iter + 1;
        const double r_norm = dsqrt(red[0]);
        st->iterations = i; st->final_residual = r_norm; st->converged = (r_norm <= c.tol) ? 1 : 0;   // :280
        c.push(r_norm);
        st->iter = i;
        if (r_norm <= c.tol) { c.finish(KRYST_OK); return; }           // :281-284
        if (fabs(st->omega) < DBL_EPSILON) { c.finish(KRYST_OK); return; }   // :285-287 break
        st->rho_prev = st->rho; st->omega_prev = st->omega;           // :288-289
        if (i >= c.max_iters) { c.finish(KRYST_OK); return; }          // loop `1..=max_iters` exhausted
        st->rho = red[1];                                              // :105-116
        if (fabs(st->rho) < DBL_EPSILON) { c.finish(KRYST_OK); return; }   // :117-119
        st->beta = (st->rho / st->rho_prev) * (st->alpha / st->omega_prev);   // :123
    }
};

struct BicgRun : SolverRun {
    bool right_pc;
    double *r = nullptr, *rhat = nullptr, *v = nullptr, *pp = nullptr, *s = nullptr, *t = nullptr, *ph = nullptr, *sh = nullptr;
    BicgRun(kryst_vec_t b, kryst_vec_t x, const SolveIO& io_, bool rp) : SolverRun(b, x, io_), right_pc(rp) {}
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        KR_TRY(common_begin(prm.max_iters + 2, 8));                                               // :73
        if (!right_pc) pc = nullptr;                     // bicgstab.rs:70: the reference ignores pc; the _rpc extension uses it
        if (pc && pc->kind == KR_PC_IDENTITY) pc = nullptr;
        KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&rhat)); KR_TRY(ws.vec(&v)); KR_TRY(ws.vec(&pp)); KR_TRY(ws.vec(&s)); KR_TRY(ws.vec(&t));
        if (pc) { KR_TRY(ws.vec(&ph)); KR_TRY(ws.vec(&sh)); }
        KR_TRY(residual_dot(a, bv->d, xw, r, t, nullptr));                                        // :75-77, :85-96
        KR_HIP(hipMemcpyAsync(rhat, r, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));    // :78
        KR_HIP(hipMemcpyAsync(pp, r, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));      // :83
        return reduce_then<1>(ctx, nt, ws.red, BicgInitLogic{lc});
    }
    int32_t iterate(int64_t) override {
        const DevState* st = ws.st;
        KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_ew(ctx, BicgPOp<K()>{st, r, v, pp}, n, done); }));   // :126-142
        if (pc) { KR_TRY(pc_apply_dev_fresh(pc, n, pp, ph, done, nullptr)); KR_TRY(launch_spmv(a, ph, v, 1, rhat, done)); }
        else KR_TRY(launch_spmv(a, pp, v, 1, rhat, done));                                        // :144-146 + (rhat,v)
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, BicgAlphaLogic{lc})));
        KR_TRY(launch_ew(ctx, BicgSOp{st, r, v, s}, n, done));                                    // :166-188
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, BicgSLogic{lc})));
        if (pc) { KR_TRY(pc_apply_dev_fresh(pc, n, s, sh, done, nullptr)); KR_TRY(launch_spmv(a, sh, t, 2, s, done)); }
        else KR_TRY(launch_spmv(a, s, t, 2, s, done));                                            // :208-209 + (t,s),(t,t)
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, BicgOmegaLogic{lc})));
        KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_ew_gated(ctx, BicgXROp<K()>{st, pc ? ph : pp, pc ? sh : s, s, t, rhat, xw, r}, n, GateEarly{st}); }));
        return reduce_then<2>(ctx, nt, ws.red, BicgEndLogic{lc});
    }
};

SolverRun* make_bicgstab_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io) { return new BicgRun(b, x, io, false); }

int32_t bicgstab_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool right_pc) {
    KR_ARG(io.a && io.params, "solve: null argument");
    BicgRun run(bv, xv, io, right_pc);
    return run.solve();
}

}  // namespace kr
