// What GmresSolver (gmres.hip) and the compressed-basis extension (gmres_cb.hip) share: the device state of a restart cycle, the launch rule of the
// Gram-Schmidt links and the one-thread logic steps of gmres.rs:216-402.
#pragma once
#include "restart_common.h"

namespace kr {

struct GmState {                     // device
    int cyc_stop;                    // leave the Arnoldi loop of this cycle
    int happy;
    int m;
    int side;                        // 0 none, 1 left, 2 right, 3 textbook left (labelled extension)
    long long iteration;
    double r0_norm, beta, hcur, hj1;
    double res0_in;                  // the norm the in-cycle convergence test divides by: res0, or (side 3) ||M^-1 r0|| of the first cycle
};

struct GmPtrs { GmState* gs; double* h; double* g; double* cs; double* sn; double* y; int restart; };

// work inside the Arnoldi loop is gated on done || cyc_stop (CycleGate).
// The Gram-Schmidt links (3 reads + 1 write + a reduction per tile) want 6 workgroups per CU WHILE z lives in the memory-side cache: GMRES(30)
// 256^3 244 -> 309 it/s with 4 (round 1), 347.7 -> 356.5 with 6 (round 3, tools/solver_ab.py: 2 / 3 / 4 / 5 / 6 / 8 per CU = 250 / 319 / 348 / 356 /
// 357 / 339 it/s).  Beyond the cache every word comes from HBM and the streams' rule holds (ew.h: a narrow moving window keeps DRAM pages open) --
// round 5, tools/fgmres_only.py: 512^3 38.0 / 40.1 / 41.0 / 33.2 it/s with 6 / 4 / 3 / 2 per CU, 384^3 94.9 / 97.6 / 97.8 with 6 / 4 / 3,
// 320^3 165.3 / 169.6 / 166.3: 6 in the cache regime, 3 for vectors beyond 768 MiB, 4 in between.
// `word`: bytes of a stored basis element (8 everywhere but in gmres_cb.hip's fp32 basis).  Both thresholds are byte counts and are judged on the
// bytes the instance has: what the cache must hold between two links is z and B_next, 8 + word bytes per row against 16, and a basis vector is
// n * word bytes.  With word = 8 both reduce to the expressions above.  Measured for word = 4 (tools/cb_gmres_bench.py, profiles/cb_gmres/knobs.jsonl):
// 512^3 35.6 / 46.8 / 53.4 / 52.4 it/s with 2 / 3 / 4 / 6 per CU (its 512 MiB vectors want 4, where the fp64 basis wants 3), and 288^3 289 -> 333 it/s
// when z (182 MiB) and B_next (91 MiB) are kept, 320^3 215 -> 213 when they are (250 + 125 MiB): the limit sits between them on either count.
inline bool keep_links_in_cache(int64_t n, int word = 8) { return keep_in_cache(n * (8 + word) / 16); }
template <class Op>
static int32_t launch_iter(kryst_ctx_t ctx, const Op& op, int64_t n, const CycleGate& cyc, int word = 8) {
    static const int forced = [] { const char* e = getenv("KRYST_GMRES_BLOCKS_PER_CU"); return e ? atoi(e) : 0; }();
    const int bpc = forced > 0 ? forced : keep_links_in_cache(n, word) ? 6 : n * word > (768ll << 20) ? 3 : 4;
    return launch_ew_gated(ctx, op, n, cyc, bpc);
}

// ---- logic
#define HH(i, k) P.h[(i) * P.restart + (k)]
struct GmInitLogic {                 // gmres.rs:227-233 ; red0 = (r0,r0)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P; int side;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double beta = dsqrt(red[0]);
        P.gs->beta = beta; st->res0 = beta; P.gs->res0_in = beta;
        st->iterations = 0; st->final_residual = beta; st->converged = 0;
        P.gs->iteration = 0; P.gs->side = side;
        if (c.max_iters <= 0 || P.restart <= 0) c.finish(KRYST_OK);     // n_outer == 0 (:231,:234)
    }
};
struct GmCycleLogic {                // gmres.rs:238, :268-275 ; for Right: red0 = (z0,z0) (:252,:259)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P; int right;
    __device__ void run(const double* red) const {
        GmState* gs = P.gs;
        double r0_norm = gs->beta;                                      // :238
        if (right) { r0_norm = dsqrt(red[0]); gs->beta = r0_norm; }     // :252, :259
        if (right == 2 && gs->iteration == 0) gs->res0_in = r0_norm;    // side 3: the first cycle's ||M^-1 r0||
        gs->r0_norm = r0_norm;
        for (int k = 0; k < (P.restart + 1) * P.restart; ++k) P.h[k] = 0.0;
        for (int k = 0; k <= P.restart; ++k) P.g[k] = 0.0;
        P.g[0] = r0_norm;                                               // :270
        for (int k = 0; k < P.restart; ++k) { P.cs[k] = 0.0; P.sn[k] = 0.0; P.y[k] = 0.0; }
        gs->m = 0; gs->happy = 0; gs->cyc_stop = 0;
    }
};
struct GmStepBeginLogic {            // gmres.rs:277 iteration += 1
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P;
    __device__ void run(const double*) const { if (!P.gs->cyc_stop) P.gs->iteration = P.gs->iteration + 1; }
};
struct GmHLogic {                    // first sweep: h[i][j] = dot (:84) ; second: h[i][j] += tmp (:91-92)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P; int i, j, second;
    __device__ void run(const double* red) const {
        if (P.gs->cyc_stop) return;
        const double d = red[0];
        if (second) HH(i, j) = HH(i, j) + d; else HH(i, j) = d;
        P.gs->hcur = d;
    }
};
struct GmNormLogic {                 // gmres.rs:97-101 / :299-303 / :331-335 then :347-354
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P; int j;
    __device__ void run(const double* red) const {
        GmState* gs = P.gs;
        if (gs->cyc_stop) return;
        const double eps = 1e-14;                                       // :233
        const double hj1 = dsqrt(red[0]);
        HH(j + 1, j) = hj1; gs->hj1 = hj1;
        if (fabs(hj1) < eps) {
            gs->happy = 1;
            if (gs->side == 1 || gs->side == 2) { gs->cyc_stop = 1; return; }   // :300-303 / :332-335: break BEFORE givens, m unchanged (side 3: as arnoldi)
        }
        givens_column(P.h, P.restart, P.cs, P.sn, P.g, j, EpsGuard{eps});   // apply_givens_and_update_g (:154-176)
        const double res_norm = fabs(P.g[j + 1]);                       // :348
        const bool conv = c.check(res_norm, gs->res0_in, gs->iteration);   // :349-350 (res0_in == res0 unless side 3)
        c.push(res_norm);                                               // addition: the reference keeps no GMRES history
        gs->m = j + 1;                                                  // :351
        if (conv || gs->happy) gs->cyc_stop = 1;                        // :352-354
    }
};
struct GmBackLogic {                 // back_substitution (:180-192) on the leading m x m block
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P;
    __device__ void run(const double*) const { back_substitute(P.h, P.restart, P.g, P.y, P.gs->m, EpsGuard{1e-14}); }
};
struct GmCycleEndLogic {             // gmres.rs:392-398 ; red0 = (r0,r0) of the true residual
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; GmPtrs P;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double beta = dsqrt(red[0]);
        P.gs->beta = beta;
        st->final_residual = beta;                                      // :394
        st->converged = (beta < c.tol * st->res0) ? 1 : 0;              // :395
        st->iter = P.gs->iteration;
        if (st->converged || P.gs->iteration >= c.max_iters) c.finish(KRYST_OK);   // :396-398
    }
};
#undef HH

}  // namespace kr
