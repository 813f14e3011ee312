// The scalar steps of CG (src/solver/cg.rs:127-284) and PCG (src/solver/pcg.rs:133-218): run by thread 0 of the kernel that ends a fold,
// on the reduced values.  Shared by the single-vector solvers (cg_pcg.hip) and the batched ones (multi.hip), which bind one instance per
// column to that column's DevState -- the same code, so the same scalars.
#pragma once
#include "solver_common.h"

namespace kr {

struct CgInitLogic {                 // cg.rs:127-140
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        st->rsq = red[0];
        st->res0 = dsqrt(st->rsq);
        st->iterations = 0; st->final_residual = st->res0; st->converged = 0; st->iter = 0;
        // dp: Preconditioned/Unpreconditioned = (r,r); Natural = (r,p) with p == r; None = 0
        const double dp = (c.norm_type == 3) ? 0.0 : st->rsq;
        c.push(dsqrt(dp));
        if (c.max_iters <= 0) c.finish(KRYST_OK);
    }
};
struct CgAlphaLogic {                // cg.rs:164-175
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double p_dot_ap = red[0];
        if (p_dot_ap <= 0.0) {                                         // :168-174
            st->iterations = st->iter + 1; st->final_residual = dsqrt(st->rsq); st->converged = 0;
            c.finish(KRYST_INDEFINITE_MATRIX);
            return;
        }
        st->alpha = st->rsq / p_dot_ap;                                // :175
        st->alpha_hist[(st->iter + 1) & 63] = st->alpha;               // (x updated in batches: XBatchOp reads it; a batch has <= 32 iterations)
    }
};
struct CgBetaLogic {                 // cg.rs:223-284
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const long long i = st->iter + 1;
        st->xpend = i;                                                 // (x += alpha p of this iteration, :207-209, is behind us in the reference)
        const double rsq_new = red[0];
        double res_norm;
        switch (c.norm_type) {                                         // :224-229
            case 0: case 1: res_norm = dsqrt(rsq_new); break;
            case 2: res_norm = dsqrt(fabs(red[1])); break;
            default: res_norm = 0.0;
        }
        if (rsq_new / st->rsq < 0.0) {                                 // :254-259
            st->iterations = i; st->final_residual = res_norm; st->converged = 0;
            st->xlast = i;                                             // (x += alpha p happened at :207)
            c.finish(KRYST_INDEFINITE_PRECONDITIONER);
            return;
        }
        c.push(res_norm);                                              // :260-263
        st->iter = i;
        if (c.check(res_norm, st->res0, i)) { st->xlast = i; c.finish(KRYST_OK); return; }   // :264-269
        st->beta = rsq_new / st->rsq;                                  // :270
        st->rsq = rsq_new;                                             // :284
    }
};

struct PcgInitLogic {                // pcg.rs:133-146 ; red0 = (r,z), red1 = (z,z) | (r,r)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        st->rz = red[0];
        st->res0 = dsqrt(fabs(st->rz));                                // :134
        st->iterations = 0; st->final_residual = st->res0; st->converged = 0; st->iter = 0;
        double dp;
        switch (c.norm_type) { case 0: case 1: dp = red[1]; break; case 2: dp = red[0]; break; default: dp = 0.0; }
        st->normq = dp;
        c.push(dsqrt(dp));                                             // :143-146 (no abs at iteration 0)
        if (c.max_iters <= 0) c.finish(KRYST_OK);
    }
};
struct PcgAlphaLogic {               // pcg.rs:151-173
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double p_dot_ap = red[0];
        if (p_dot_ap <= 0.0) {                                         // :162-172 (the dots of the unchanged r, z)
            st->iterations = st->iter + 1;
            st->final_residual = (c.norm_type == 3) ? 0.0 : dsqrt(c.norm_type == 2 ? fabs(st->normq) : st->normq);
            st->converged = 0;
            c.finish(KRYST_INDEFINITE_MATRIX);
            return;
        }
        st->alpha = st->rz / p_dot_ap;                                 // :173
        st->alpha_hist[(st->iter + 1) & 63] = st->alpha;
    }
};
struct PcgBetaLogic {                // pcg.rs:188-218
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const long long i1 = st->iter + 1;                             // the reference's i + 1
        st->xpend = i1;                                                // (x += alpha p of this iteration, :175-177, is behind us in the reference)
        const double rz_new = red[0];
        double res_norm;
        switch (c.norm_type) {                                         // :190-195
            case 0: case 1: res_norm = dsqrt(red[1]); st->normq = red[1]; break;
            case 2: res_norm = dsqrt(fabs(rz_new)); st->normq = rz_new; break;
            default: res_norm = 0.0;
        }
        c.push(res_norm);                                              // :196-199
        st->iter = i1;
        if (c.check(res_norm, st->res0, i1)) { st->xlast = i1; c.finish(KRYST_OK); return; }   // :200-205 (x += alpha p happened at :175)
        const double beta = rz_new / st->rz;                           // :206
        if (beta < 0.0) {                                              // :208-213
            st->iterations = i1; st->final_residual = res_norm; st->converged = 0;
            st->xlast = i1;
            c.finish(KRYST_INDEFINITE_PRECONDITIONER);
            return;
        }
        st->beta = beta;
        st->rz = rz_new;                                               // :218
    }
};

}  // namespace kr
