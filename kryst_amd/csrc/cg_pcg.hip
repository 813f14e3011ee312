// Device-resident CG and PCG: LinearSolver::solve (src/solver/mod.rs:30-52) for a HIP CSR operator.  Each solver restates its
// reference file operation by operation (line numbers cited inline); the vector work is fused into as few HBM passes as the
// data dependences allow without changing any rounding.  One unit for both: they share the direction vector's bookkeeping
// (DirectionVec) and most of their ew_kernel instances.
#include "solvers.h"
#include "cg_logic.h"

namespace kr {

// =================================================================== shared vector ops
struct DotPairOp {
    static constexpr int NQ = 2; static constexpr const char* TAG = "DotPair";
    const double *a, *b, *c, *d;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const d2 u = ld2(a, i), v = ld2(b, i), w = ld2(c, i), z = ld2(d, i);
        if (in0) { acc[0] = acc[0] + u.a * v.a; acc[1] = acc[1] + w.a * z.a; }
        if (in1) { acc[0] = acc[0] + u.b * v.b; acc[1] = acc[1] + w.b * z.b; }
    }
};
template <bool KEEP = false>
struct AypxDevOp {                   // y = x + beta*y  (cg.rs:274-276, pcg.rs:215-217), beta on the device
    static constexpr int NQ = 0; static constexpr const char* TAG = "AypxDev"; static constexpr int PHASE = KR_PH_BLAS1_DIRECTION;
    const double* beta; const double* x; double* y;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double be = *beta;
        const d2 a = ld2_sel<KEEP>(x, i), b = ld2(y, i);                 // x (the residual) was written by the launch before this one
        st2(y, i, a.a + be * b.a, a.b + be * b.b);
    }
};

// =================================================================== CG (src/solver/cg.rs:114-288)
// x += alpha p ; r -= alpha Ap (cg.rs:207-212) ; partial r.r (cg.rs:223) [; partial r.p for the Natural norm, :227]
template <bool KEEP = false>
struct CgUpdate1 {
    static constexpr int NQ = 1; static constexpr const char* TAG = "CgUpdate1"; static constexpr int PHASE = KR_PH_BLAS1_RESIDUAL;
    const double* alpha; const double* p; const double* ap; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double al = *alpha;
        const d2 pp = ld2(p, i), aa = ld2(ap, i), xx = ld2(x, i), rr = ld2(r, i);
        const double x0 = xx.a + al * pp.a, x1 = xx.b + al * pp.b;
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;
        st2(x, i, x0, x1); st2_sel<KEEP>(r, i, r0, r1);                   // r is read again by the next launch (p = r + beta p)
        if (in0) acc[0] = acc[0] + r0 * r0;
        if (in1) acc[0] = acc[0] + r1 * r1;
    }
};
struct CgUpdate2 {                   // + r.p (old p) for CgNormType::Natural
    static constexpr int NQ = 2; static constexpr const char* TAG = "CgUpdate2";
    const double* alpha; const double* p; const double* ap; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const double al = *alpha;
        const d2 pp = ld2(p, i), aa = ld2(ap, i), xx = ld2(x, i), rr = ld2(r, i);
        const double x0 = xx.a + al * pp.a, x1 = xx.b + al * pp.b;
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;
        st2(x, i, x0, x1); st2(r, i, r0, r1);
        if (in0) { acc[0] = acc[0] + r0 * r0; acc[1] = acc[1] + r0 * pp.a; }
        if (in1) { acc[0] = acc[0] + r1 * r1; acc[1] = acc[1] + r1 * pp.b; }
    }
};
struct CgUpdate0 {                   // no fused dot (PCG with a non-pointwise preconditioner)
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgUpdate0";
    const double* alpha; const double* p; const double* ap; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = *alpha;
        const d2 pp = ld2(p, i), aa = ld2(ap, i), xx = ld2(x, i), rr = ld2(r, i);
        st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b);
        st2(r, i, rr.a - al * aa.a, rr.b - al * aa.b);
    }
};

// ---- the x update deferred to the direction pass.  The reference does x += alpha p (cg.rs:207-209, pcg.rs:175-177) right after alpha;
// nothing reads x again before the solve returns, so here the update rides on the pass that reads p anyway (p = r + beta p, cg.rs:274-276):
// p is read once per iteration instead of twice -- 8 instead of 9 vector passes for CG, 10 instead of 11 for Jacobi-PCG -- and every
// element sees the reference's operations on the reference's operands: x_{k+1} = x_k + alpha_k p_k with p_k not yet overwritten.
// An exit taken after the reference's x update (convergence, iteration cap, indefinite preconditioner) stamps its iteration into
// st->xlast, and that iteration's direction pass still runs its x half (GateXPending); an exit before it (p.Ap <= 0) does not.
// KRYST_CG_DEFER_X=0 keeps the eager form (also used for the Natural norm, the trust region and the objective target, which read p or x
// inside the iteration).
template <bool KEEP = false>
struct CgResidualOp {                // r -= alpha Ap (cg.rs:210-212) ; partial r.r (:223)
    static constexpr int NQ = 1; static constexpr const char* TAG = "CgResidual"; static constexpr int PHASE = KR_PH_BLAS1_RESIDUAL; static constexpr int BPC = 3;       // 2 reads + 1 write + a fold per tile: 3 workgroups per CU (tools/stream_ab.py: 512^3 0.609 -> 0.533 ms, 256^3 0.077 -> 0.065)
    const double* alpha; const double* ap; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double al = *alpha;
        const d2 aa = ld2(ap, i), rr = ld2(r, i);
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;
        st2_sel<KEEP>(r, i, r0, r1);                                      // r is read again by the direction pass
        if (in0) acc[0] = acc[0] + r0 * r0;
        if (in1) acc[0] = acc[0] + r1 * r1;
    }
};
struct CgResidual0Op {               // r -= alpha Ap, no fused dot (PCG with a non-pointwise preconditioner)
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgResidual0";
    const double* alpha; const double* ap; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = *alpha;
        const d2 aa = ld2(ap, i), rr = ld2(r, i);
        st2(r, i, rr.a - al * aa.a, rr.b - al * aa.b);
    }
};
template <bool KEEP = false>
struct CgDirectionOp {               // x += alpha p (cg.rs:207-209, deferred) ; p = z + beta p (cg.rs:274-276, pcg.rs:215-217; z = r for CG)
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgDirection"; static constexpr int PHASE = KR_PH_BLAS1_DIRECTION; static constexpr int BPC = 3;   // inside CG: 2 -> 3 +4.4 % (256^3), +1.1 % (512^3); PCG +3.0 % / -0.7 %
    const DevState* st; const double* z; double* p; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = st->alpha, be = st->beta;
        const bool ended = st->done != 0;                                 // (uniform) the solve ended in this iteration: only x is still owed
        const d2 pp = ld2(p, i), xx = ld2(x, i);
        st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b);
        if (!ended) {
            const d2 zz = ld2_sel<KEEP>(z, i);
            st2(p, i, zz.a + be * pp.a, zz.b + be * pp.b);
        }
    }
};
// the same pass with the direction vectors in a RING and x updated in batches (XBatchOp below): p_new = z + beta p_old, out of place; x is not touched
template <bool KEEP = false>
struct CgDirectionRingOp {
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgDirectionRing"; static constexpr int PHASE = KR_PH_BLAS1_DIRECTION; static constexpr int BPC = 3;
    const DevState* st; const double* z; const double* p_old; double* p_new;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        if (st->done != 0) return;                                        // (uniform) the solve ended in this iteration: no further direction
        const double be = st->beta;
        const d2 pp = ld2(p_old, i), zz = ld2_sel<KEEP>(z, i);
        st2(p_new, i, zz.a + be * pp.a, zz.b + be * pp.b);
    }
};
struct GateXPending {                // runs while the solve is under way, and once more in the iteration that ended it after the x update
    const DevState* st; long long it;
    __device__ __forceinline__ bool skip() const { return st->done && st->xlast != it; }
};
// The direction pass on a distributed operator whose neighbours get contiguous runs of rows (k-slab partitions): the tiles that hold
// those rows first, then the halo exchange of the new p is STARTED (halo.hip: halo_begin), then the rest of the vector -- the planes
// travel while the pass is still writing the interior, not only during the next SpMV's interior tiles (which the staged-window
// kernel has made shorter than the exchange).  Same launches' worth of work, same bits.  KRYST_HALO_EARLY=0: one launch, exchange
// started by the SpMV as before.
template <class Op>
inline int32_t launch_direction(kryst_ctx_t ctx, kryst_csr_t a, const Op& op, int64_t n, const DevState* st, long long it, const double* p_vec) {
    const GateXPending gate{st, it};
    // The early start adds one exchange per iteration, so WHETHER it happens must not depend on anything a rank sees alone: it is
    // a->halo_early_ok (agreed across ranks when the operator was created) and the environment (the same on every rank, like every
    // other setting).  Whether this rank SPLITS its pass around the exchange is a local matter: a rank whose send ranges are most of
    // its block runs the whole pass first and starts the exchange behind it -- the same number of exchanges either way.
    if (a->dist && use_collectives(ctx) && a->halo_early_ok && env_int("KRYST_HALO_EARLY", 1) != 0) {
        std::vector<std::pair<int64_t, int64_t>> early;
        halo_send_tiles(a, early);
        int64_t covered = 0;
        for (const auto& r : early) covered += r.second - r.first;
        const int64_t all = ntiles_of(n);
        if (!early.empty() && early.size() <= 4 && 2 * covered < all) {
            for (const auto& r : early) KR_TRY(launch_ew_gated(ctx, op, n, gate, 0, r.first, std::min(r.second, all)));
            KR_TRY(halo_begin(a, p_vec));
            int64_t at = 0;
            for (const auto& r : early) { KR_TRY(launch_ew_gated(ctx, op, n, gate, 0, at, std::min(r.first, all))); at = std::min(r.second, all); }
            return launch_ew_gated(ctx, op, n, gate, 0, at, all);
        }
        KR_TRY(launch_ew_gated(ctx, op, n, gate));
        return halo_begin(a, p_vec);
    }
    return launch_ew_gated(ctx, op, n, gate);
}
inline bool cg_defer_x() { return env_int("KRYST_CG_DEFER_X", 1) != 0; }      // (read per iteration enqueue: a getenv, not on any critical path)

// ---- CG side exits (off by default in the reference): trust region cg.rs:177-202, objective target cg.rs:231-252
struct CgRadiusLogic {               // red0 = (p,p), red1 = (x,x)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; double radius;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double p_norm = dsqrt(red[0]), x_norm = dsqrt(red[1]);                       // :178-179
        if (x_norm + fabs(st->alpha) * p_norm > radius) {                                  // :180
            st->alpha = (radius - x_norm) / p_norm;                                        // :181 max_step, applied by AxpyIfOp
            st->iterations = st->iter + 1; st->final_residual = dsqrt(st->rsq); st->converged = 0;   // :196-199
            st->early = 1;
            c.finish(KRYST_OK);
        }
    }
};
struct CgRsqLogic {                  // first half of cg.rs:223-229 when the objective exit sits in between
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        st->rz = red[0];                                                                    // rsq_new
        switch (c.norm_type) { case 0: case 1: st->normq = dsqrt(red[0]); break; case 2: st->normq = dsqrt(fabs(red[1])); break; default: st->normq = 0.0; }
    }
};
struct StoreLogic {                  // keeps one reduced value for a later logic step
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; double* slot;
    __device__ void run(const double* red) const { *slot = red[0]; }
};
struct CgObjLogic {                  // cg.rs:231-252 ; red0 = (x,b), *xax = (x,Ax)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; const double* xax; double target;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double obj = 0.5 * (*xax) - red[0];                                           // :237
        if (obj <= target) {                                                                // :245-251
            st->iterations = st->iter + 1; st->final_residual = st->normq; st->converged = 1;
            c.finish(KRYST_OK);
        }
    }
};
struct CgBetaStoredLogic {           // second half: cg.rs:254-284 on the stored rsq_new / res_norm
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double*) const {
        DevState* st = c.st;
        const long long i = st->iter + 1;
        const double rsq_new = st->rz, res_norm = st->normq;
        if (rsq_new / st->rsq < 0.0) {
            st->iterations = i; st->final_residual = res_norm; st->converged = 0;
            c.finish(KRYST_INDEFINITE_PRECONDITIONER);
            return;
        }
        c.push(res_norm);
        st->iter = i;
        if (c.check(res_norm, st->res0, i)) { c.finish(KRYST_OK); return; }
        st->beta = rsq_new / st->rsq;
        st->rsq = rsq_new;
    }
};
struct AxpyIfOp {                    // x += alpha*p, only while st->early is raised (cg.rs:185-187 max_step update)
    static constexpr int NQ = 0; static constexpr const char* TAG = "AxpyIf";
    const DevState* st; const double* p; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = st->alpha;
        const d2 pp = ld2(p, i), xx = ld2(x, i);
        st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b);
    }
};
// the x update the fused form still owes when no further fused SpMV follows (the end of a solve or session)
struct GateXOwed {
    const DevState* st; long long it;
    __device__ __forceinline__ bool skip() const { return st->xpend != it; }
};
struct CgFlushOp {                   // x += alpha p (cg.rs:207-209 / pcg.rs:175-177) of the last enqueued iteration
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgFlush"; static constexpr int PHASE = KR_PH_BLAS1_DIRECTION;
    const DevState* st; const double* p; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = st->alpha;
        const d2 pp = ld2(p, i), xx = ld2(x, i);
        st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b);
    }
};
// ---- x updated in BATCHES (round 5).  A written byte costs this HBM what 2-2.5 read bytes cost (profiles/r05/fuse_kernel_ablations.txt: the fused
// kernel's three written vectors are 0.54 of its 1.34 ms), and x += alpha_i p_i (cg.rs:207-209) writes x every iteration although nothing reads x
// before the solve returns.  With the direction vectors kept in a ring of m + 1 buffers (p_new is written every iteration anyway) the m updates of
// iterations k - m + 1 .. k are applied in ONE pass -- x = x + alpha_i p_i for i ascending, each the reference's un-fused multiply and add on the
// reference's operands, so the same bits -- which reads x once and writes it once per m iterations.  Updates beyond `xpend` (the solve ended before
// them) are not applied; the flush at the end of a solve / session applies what the last partial batch owes.
constexpr int KR_XB_MAX = 32;      // the longest batch (DevState::alpha_hist holds 64 entries; the ring has KR_XB_MAX + 1 slots at most)
template <int M>                   // M: the batch's length when every one of its updates happened (the common case), 0: any length, tested per update
struct XBatchOp {
    static constexpr int NQ = 0; static constexpr const char* TAG = "XBatch"; static constexpr int PHASE = KR_PH_BLAS1_XBATCH; static constexpr int BPC = 2;
    static constexpr int ANY = M > 8 ? M : M > 0 ? 8 : KR_XB_MAX;              // the updates the tested form walks
    const DevState* st; const double* p[KR_XB_MAX]; long long lo; int cnt; double* x;   // p[u]: the direction vector of iteration lo + u
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const long long last = st->xpend;                                     // (uniform) updates of later iterations never happened in the reference
        d2 xx = ld2(x, i);
        // all M loads in flight together, then the M updates in iteration order.  (M = 24 and 32 measured at 512^3 with the loads in chunks of 8 and
        // 16 under the x pair as well, profiles/handoff/xb_chunk_ab.jsonl: 719.0 / 719.4 / 720.0 it/s at M = 32 -- no difference, so the one form)
        if (M > 0 && lo + M - 1 <= last) {
            d2 pp[M > 0 ? M : 1]; double al[M > 0 ? M : 1];
#pragma unroll
            for (int u = 0; u < M; ++u) { pp[u] = ld2(p[u], i); al[u] = st->alpha_hist[(lo + u) & 63]; }
#pragma unroll
            for (int u = 0; u < M; ++u) { xx.a = xx.a + al[u] * pp[u].a; xx.b = xx.b + al[u] * pp[u].b; }
        } else {
#pragma unroll
            for (int u = 0; u < ANY; ++u) {
                if (u < cnt && lo + u <= last) {
                    const double al = st->alpha_hist[(lo + u) & 63];
                    const d2 pp = ld2(p[u], i);
                    xx.a = xx.a + al * pp.a; xx.b = xx.b + al * pp.b;
                }
            }
        }
        st2(x, i, xx.a, xx.b);
    }
};
struct GateXBatch {                  // nothing to apply: the solve ended before this batch's first iteration
    const DevState* st; long long lo;
    __device__ __forceinline__ bool skip() const { return st->xpend < lo; }
};
template <int M>
inline int32_t launch_x_batch_m(kryst_ctx_t ctx, DevState* st, const std::vector<double*>& ring, int xb, long long lo, long long hi, double* x, int64_t n, int64_t tile_lo, int64_t tile_hi) {
    XBatchOp<M> op; op.st = st; op.lo = lo; op.cnt = (int)(hi - lo + 1); op.x = x;
    for (int u = 0; u < KR_XB_MAX; ++u) op.p[u] = ring[(size_t)((lo + std::min<long long>(u, hi - lo)) % (xb + 1))];
    return launch_ew_gated(ctx, op, n, GateXBatch{st, lo}, 0, tile_lo, tile_hi);
}
// x += alpha_i p_i for iterations lo .. hi (those that happened) on tiles [tile_lo, tile_hi) (-1: to the end), p_i in ring[i % (xb + 1)].  Every length from 2 to KR_XB_MAX has an instance of its
// own -- a full batch, and the partial one the flush at the end of a solve or session owes (up to xb - 1 updates: one pass with all its loads in
// flight, not one dependent load after the other); a single update takes the any-length instance
inline int32_t launch_x_batch(kryst_ctx_t ctx, DevState* st, const std::vector<double*>& ring, int xb, long long lo, long long hi, double* x, int64_t n,
                              int64_t tile_lo = 0, int64_t tile_hi = -1) {
    int32_t rc = KRYST_OK;
    const int cnt = (int)(hi - lo + 1);
    KR_ARG(cnt >= 1 && cnt <= KR_XB_MAX, "launch_x_batch: a batch of more than 32 iterations");
    auto exact = [&](auto M) { rc = launch_x_batch_m<M()>(ctx, st, ring, xb, lo, hi, x, n, tile_lo, tile_hi); };
    if (by_int<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(cnt, exact) || by_int<17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32>(cnt, exact)) return rc;
    return launch_x_batch_m<0>(ctx, st, ring, xb, lo, hi, x, n, tile_lo, tile_hi);
}
// x-batch length: 1 = every iteration (x rides on the fused pass that reads p_old); KRYST_CG_X_BATCH forces (<= 32).  Measured at 512^3
// (profiles/r05/cg_xbatch_ab.jsonl): CG 545 / 560 / 575 / 579 / 584 / 582 / 588 it/s at m = 1 / 2 / 4 / 5 / 6 / 7 / 8 (unfused 530); PCG 447 / 459 / 487 /
// 489 / 490 / 490.5 / 472 (unfused 443) -- PCG's thirteen 1 GB work vectors lose at m = 8 what the ninth ring slot costs, so 7 there.
// Batches beyond 8 (<= KR_XB_MAX; the pass moves (m + 2) * 8 / m bytes per row and iteration: 10 at 8, 8.5 at 32), one operator, one process, 192+
// timed iterations x 3 rounds (profiles/handoff/xb_chunk_ab.jsonl, pcg_xbatch_ab.jsonl): CG 709.5 / 713.1 / 714.8 / 720.1 / 720.0 it/s at m = 8 / 12 /
// 16 / 24 / 32, every run of 32 above every run of 8; bench.py alternating with the parent commit 699.8 -> 708.0 it/s (+1.2 %) -- so 32 for CG (a ring of 33 vectors: 33 GiB at 512^3; ring_if_it_fits halves the batch
// until the device can hold its ring).  PCG 523.0 / 521.4 / 540.3 / 544.2 at m = 7 / 8 / 12 / 16, but its runs at 7 spread over
// 30 it/s (541 in the first round, 511 and 517 after the longer rings had been allocated): short of the margin, so PCG stays at 7.
inline int cg_x_batch(bool pcg) {
    return std::max(1, std::min(KR_XB_MAX, env_int("KRYST_CG_X_BATCH", pcg ? 7 : 32)));
}
// how a batch is paid (read in plan(): once per solve or session).  0: all rows in one pass every m-th iteration.  1: the rows cut into m slices,
// iteration it pays slice it % m -- the same bytes, spread evenly: no iteration carries the whole pass (6.6 ms at 512^3 and m = 32 beside 1.2 ms
// for every other iteration, so a short solve or a timing window of 20 iterations used to see one pass more or less).
// Measured at 512^3 (profiles/x_slices/): the slice launch of m = 32 takes 193 us (34 streams over 32 MiB each at 5.90 TB/s) where the whole pass took
// 6610 us = 206.6 per iteration (5.55 TB/s), and the fused SpMV behind it 596 instead of 612 us.  In one process, whole rounds timed, three rounds:
// CG m = 32 718.7 -> 730.6 it/s, PCG m = 7 539.5 -> 540.9, every run in slices above every run of the whole pass, the means apart by more than
// twice the larger spread -- so slices for both.  bench.py alternating with the parent commit: 710.1 -> 730.8 it/s (+2.9 %, every
// run above every run), 675.4 -> 749.5 at --steps 20 --warmup 5, where the parent's windows held the whole pass or not.
// The slices on a low-priority stream of their own beside the dependent chain (ordered by events) were built, measured and taken out again:
// beside a slice the fused SpMV takes 786 us and the slice 462, together what they take one after the other (596 + 193), and CG ran 695.1 it/s.
inline int cg_x_slice() {
    return env_int("KRYST_CG_X_SLICE", 1) != 0 ? 1 : 0;
}
// the ring costs xb - 1 work vectors more than the two alternating direction vectors: only where the device has the room (what the context's
// arena already holds counts as room).  base: the solver's other work vectors.  A ring that does not fit is halved until one does (32 -> 16 -> 8 ..)
inline int ring_if_it_fits(kryst_ctx_t ctx, int64_t n, int xb, int base) {
    if (xb <= 1) return 1;
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 1; }
    for (; xb > 1; xb /= 2) {
        const size_t need = padded_bytes(n) * (size_t)(base + xb + 1 + 2);
        if (need <= ctx->arena_bytes || need <= free_b + ctx->arena_bytes) return xb;
    }
    return 1;
}
// ... and in the UNFUSED deferred form (every operator form, every rank of a partition) the same ring is available: the direction pass writes
// p_new = z + beta p_old out of place (CgDirectionRingOp: 2 reads + 1 write instead of 3 + 2) and XBatchOp pays x -- 34 instead of 40 bytes per row
// and iteration.  MEASURED AND OFF BY DEFAULT (profiles/r05/cg_ring_unfused_ab.jsonl): 192^3 .. 384^3 run 2-7 % SLOWER (the in-place direction vector
// is what the 256 MiB Infinity Cache hands from the direction pass to the SpMV; nine ring slots defeat that), 512^3 on plain CSR +-1 %, 64^3 / 128^3
// +3 %.  KRYST_CG_X_BATCH = m > 1 turns it on (tests do).
inline int cg_x_batch_unfused() {
    return std::max(1, std::min(KR_XB_MAX, env_int("KRYST_CG_X_BATCH", 1)));
}
// ---- the direction vector of CG and PCG: where p lives (in place; two alternating vectors; a ring), the form its update p = z + beta p takes
// (inside the next iteration's SpMV; a ring pass; the in-place pass) and the x updates that ride on it.  One owner for both solvers: what differs
// between them -- whether x is deferred, the batch length, the count of other work vectors, z, whether Ap is stored, the KEEP of the pass -- are
// arguments.  fuse, xb and ringdir are fixed by plan(); the Run reads every other knob where it always did.
struct __attribute__((visibility("hidden"))) DirectionVec {
    SolverRun& s;
    double* pp = nullptr;            // the direction vector of the iteration being enqueued
    double* p2 = nullptr;            // the fused form's second direction vector (p_old / p_new alternate)
    bool fuse = false; long long fused_upto = 0;     // fused_upto: the last iteration enqueued in the fused form (its x update rides on the next one)
    int xb = 1; std::vector<double*> ring;           // xb > 1: x in batches of xb iterations, direction vector of iteration k in ring[k % (xb + 1)]
    bool ringdir = false;                            // the unfused deferred form with the ring (CgDirectionRingOp)
    XSlices xs;                                      // xb > 1: which rows owe which x updates (cg_logic.h)
    int32_t x_batch(const XSliceLaunch& l) {         // apply the x updates of iterations l.lo .. l.hi (those that happened) to the rows of l's tiles
        return launch_x_batch(s.ctx, s.ws.st, ring, xb, l.lo, l.hi, s.xw, s.n, l.tile_lo, l.tile_hi);
    }
    // begin(), first: the form of this solve.  deferred: x += alpha p may ride on the direction pass; base: the solver's work vectors besides x and the
    // ring (CG 3, PCG 4).  -> the work vectors to reserve
    int plan(bool deferred, bool pcg, int base) {
        // the direction pass inside the SpMV (spmv_fuse.hip: spmv_pattern_fuse_kernel) where the operator's form allows it
        fuse = deferred && spmv_can_fuse_direction(s.a);
        xb = fuse ? cg_x_batch(pcg) : deferred ? cg_x_batch_unfused() : 1;
        xb = ring_if_it_fits(s.ctx, s.n, xb, base);
        ringdir = !fuse && xb > 1;
        xs.init(xb, ntiles_of(s.n), cg_x_slice() != 0);
        return xb > 1 ? base + xb + 1 : fuse ? 5 : 4;
    }
    // begin(), once pp has been taken from the workspace: the other vectors p needs
    int32_t alloc() {
        if (xb > 1) {                                  // the ring: slot 1 is p_1 (= pp), the others follow
            ring.assign((size_t)xb + 1, nullptr);
            ring[1 % (xb + 1)] = pp;
            for (int k = 0; k <= xb; ++k) if (!ring[(size_t)k]) KR_TRY(s.ws.vec(&ring[(size_t)k]));
        } else if (fuse) KR_TRY(s.ws.vec(&p2));
        return KRYST_OK;
    }
    // iteration it follows one enqueued in the fused form: its SpMV forms p on the way
    bool fused_now(int64_t it) const { return fuse && fused_upto == it - 1 && it > 1; }
    // the SpMV of iteration it: ap = A p with the partials of (p, Ap).  fused_now: [x += alpha p_old owed by iteration it - 1 (xb == 1); p = z + beta p_old;
    // Ap; (p, Ap)] in ONE pass, and ap may be null (the residual pass forms A p again); otherwise p is there already (the first iteration: p = z)
    int32_t spmv(int64_t it, const double* z, double* ap) {
        DevState* st = s.ws.st;
        if (!fused_now(it)) return launch_spmv(s.a, pp, ap, 1, pp, s.done);
        if (xb > 1) {
            double* p_old = ring[(size_t)((it - 1) % (xb + 1))]; double* p_new = ring[(size_t)(it % (xb + 1))];
            KR_TRY(launch_spmv_fused(s.a, z, p_old, p_new, nullptr, ap, 1, &st->alpha, &st->beta, &st->xpend, (long long)it, s.done));
            pp = p_new;
        } else {
            KR_TRY(launch_spmv_fused(s.a, z, pp, p2, s.xw, ap, 1, &st->alpha, &st->beta, &st->xpend, (long long)it, s.done));
            std::swap(pp, p2);
        }
        return KRYST_OK;
    }
    // the end of a deferred iteration it, after beta.  The fused form launches nothing (the direction pass is the next iteration's SpMV); the ring form
    // writes p_{it+1} = z + beta p_it into the next slot; both then pay x in one pass when a batch is due.  The in-place form: x += alpha p and
    // p = z + beta p in one pass.  keep: z was stored to stay in cache for this pass
    int32_t advance(int64_t it, const double* z, bool keep) {
        DevState* st = s.ws.st;
        if (!fuse && !ringdir)
            return by_bool(keep, [&](auto K) { return launch_direction(s.ctx, s.a, CgDirectionOp<K()>{st, z, pp, s.xw}, s.n, st, (long long)it, pp); });   // cg.rs:207-209, :274-276 / pcg.rs:175-177, :215-217
        if (ringdir) {
            double* p_new = ring[(size_t)((it + 1) % (xb + 1))];
            KR_TRY(by_bool(keep, [&](auto K) { return launch_direction(s.ctx, s.a, CgDirectionRingOp<K()>{st, z, pp, p_new}, s.n, st, (long long)it, p_new); }));
            pp = p_new;
        }
        fused_upto = it;
        XSliceLaunch l;
        if (xb > 1 && xs.advance(it, &l)) KR_TRY(x_batch(l));                                     // the x updates this iteration pays: the last xb on one slice of the rows, or on all rows every xb-th iteration
        return KRYST_OK;
    }
    int32_t flush() {
        if ((!fuse && !ringdir) || fused_upto == 0) return KRYST_OK;
        if (xb > 1) {                                                                             // what every slice still owes (one slice: the last partial batch)
            std::vector<XSliceLaunch> owed;
            xs.flush(fused_upto, owed);
            for (const XSliceLaunch& l : owed) KR_TRY(x_batch(l));
            return KRYST_OK;
        }
        return launch_ew_gated(s.ctx, CgFlushOp{s.ws.st, pp, s.xw}, s.n, GateXOwed{s.ws.st, fused_upto});
    }
};

struct CgRun : SolverRun {
    using SolverRun::SolverRun;
    double *r = nullptr, *ap = nullptr, *ax = nullptr;
    DirectionVec dir{*this};
    // x += alpha p rides on the direction pass (the side exits and the Natural norm read p or x inside the iteration)
    bool deferred() const { return cg_defer_x() && !prm.has_radius && !prm.has_obj_target && prm.norm_type != 2; }
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        KR_TRY(common_begin(prm.max_iters + 2, dir.plan(deferred(), false, 3)));                  // cg.rs:117
        KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&dir.pp)); KR_TRY(ws.vec(&ap));
        KR_TRY(dir.alloc());
        if (prm.has_obj_target) KR_TRY(ws.vec(&ax));
        KR_TRY(residual_dot(a, bv->d, xw, r, ap, nullptr));                                       // :120-125, :127
        KR_HIP(hipMemcpyAsync(dir.pp, r, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));  // :126
        return reduce_then<1>(ctx, nt, ws.red, CgInitLogic{lc});
    }
    int32_t flush() override { return dir.flush(); }
    int32_t iterate(int64_t it) override {
        // recompute: the fused launch stores no Ap and the residual pass forms it again from p_new (spmv_fuse.hip: cg_recompute_residual_kernel) -- decided
        // ONCE per iteration, here, for both launches (KRYST_CG_RECOMPUTE_AP may change between session steps); every other iteration keeps ap
        const bool recompute = dir.fused_now(it) && dir.xb > 1 && spmv_can_recompute_ap(a);
        KR_TRY(dir.spmv(it, r, recompute ? nullptr : ap));                                        // :143-144 + (p,Ap) :164
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgAlphaLogic{lc})));
        double* const pp = dir.pp;
        if (dir.fuse || deferred()) {                                                             // (the fused form was fixed in begin(); the unfused one reads the knob per iteration)
            if (recompute) KR_TRY(launch_cg_residual_recompute(a, pp, r, &ws.st->alpha, keep_in_cache(n), done));
            else KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_ew(ctx, CgResidualOp<K()>{&ws.st->alpha, ap, r}, n, done); }));   // :210-212 + (r,r) :223
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgBetaLogic{lc})));
            return dir.advance(it, r, keep_in_cache(n));
        }
        if (prm.has_radius) {                                                                     // :177-202 (Steihaug-Toint)
            KR_TRY(launch_ew(ctx, DotPairOp{pp, pp, xw, xw}, n, done));
            KR_TRY((reduce_then<2>(ctx, nt, ws.red, CgRadiusLogic{lc, prm.radius})));
            KR_TRY(launch_ew_gated(ctx, AxpyIfOp{ws.st, pp, xw}, n, GateIfEarly{ws.st}));
            KR_TRY(logic_only(ctx, ws.red, ClearEarlyLogic{lc}));
        }
        const bool nat = prm.norm_type == 2;
        if (nat) KR_TRY(launch_ew(ctx, CgUpdate2{&ws.st->alpha, pp, ap, xw, r}, n, done));
        else KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_ew(ctx, CgUpdate1<K()>{&ws.st->alpha, pp, ap, xw, r}, n, done); }));   // :207-212 + (r,r) :223
        if (!prm.has_obj_target) {
            if (nat) KR_TRY((reduce_then<2>(ctx, nt, ws.red, CgBetaLogic{lc})));
            else KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgBetaLogic{lc})));
        } else {                                                                                  // :231-252
            if (nat) KR_TRY((reduce_then<2>(ctx, nt, ws.red, CgRsqLogic{lc})));
            else KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgRsqLogic{lc})));
            KR_TRY(launch_spmv(a, xw, ax, 1, xw, done));                                          // ax = A x, (x, Ax)
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, StoreLogic{lc, &ws.st->omega})));
            KR_TRY(launch_ew(ctx, DotOneOp{xw, bv->d}, n, done));                                 // (x, b)
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgObjLogic{lc, &ws.st->omega, prm.obj_target})));
            KR_TRY(logic_only(ctx, ws.red, CgBetaStoredLogic{lc}));
        }
        return by_bool(keep_in_cache(n), [&](auto K) { return launch_ew(ctx, AypxDevOp<K()>{&ws.st->beta, r, pp}, n, done); });   // :274-276
    }
};

SolverRun* make_cg_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io) { return new CgRun(b, x, io); }

int32_t cg_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io) {
    KR_ARG(io.a && io.params, "solve: null argument");
    CgRun run(bv, xv, io);
    return run.solve();
}

// =================================================================== PCG (src/solver/pcg.rs:114-222)
// fused update for z == r (pc None / identity) and z = D^-1 r (Jacobi):
//   x += alpha p ; r -= alpha Ap ; z = M^-1 r ; partial 0 = r.z ; partial 1 = norm quantity (z.z | r.r)
template <bool JACOBI, bool KEEP = false>
struct PcgUpdateOp {
    static constexpr int NQ = 2; static constexpr const char* TAG = "PcgUpdate"; static constexpr int PHASE = KR_PH_BLAS1_RESIDUAL; static constexpr int BPC = 3;       // 5 reads + 3 writes: 3 workgroups per CU measured best (+3 %)
    const double* alpha; const double* p; const double* ap; double* x; double* r; double* z; const double* inv;
    int norm_type;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const double al = *alpha;
        const d2 pp = ld2(p, i), aa = ld2(ap, i), xx = ld2(x, i), rr = ld2(r, i);
        const double x0 = xx.a + al * pp.a, x1 = xx.b + al * pp.b;                   // pcg.rs:175-177
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;                   // pcg.rs:179-181
        st2(x, i, x0, x1); st2(r, i, r0, r1);
        double z0 = r0, z1 = r1;
        if constexpr (JACOBI) {
            const d2 dv = ld2(inv, i);
            z0 = dv.a * r0; z1 = dv.b * r1;                                          // jacobi.rs:84-86
            st2_sel<KEEP>(z, i, z0, z1);                                             // z is read again by the next launch (p = z + beta p)
        }
        const bool zz = norm_type == 0;                                              // Preconditioned: (z,z); else (r,r)
        if (in0) { acc[0] = acc[0] + r0 * z0; acc[1] = acc[1] + (zz ? z0 * z0 : r0 * r0); }
        if (in1) { acc[0] = acc[0] + r1 * z1; acc[1] = acc[1] + (zz ? z1 * z1 : r1 * r1); }
    }
};

template <bool JACOBI, bool KEEP = false>
struct PcgResidualOp {               // PcgUpdateOp without its x half (deferred to CgDirectionOp): 2-3 reads + 1-2 writes
    static constexpr int NQ = 2; static constexpr const char* TAG = "PcgResidual"; static constexpr int PHASE = KR_PH_BLAS1_RESIDUAL; static constexpr int BPC = 3;
    const double* alpha; const double* ap; double* r; double* z; const double* inv;
    int norm_type;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const double al = *alpha;
        const d2 aa = ld2(ap, i), rr = ld2(r, i);
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;                   // pcg.rs:179-181
        double z0 = r0, z1 = r1;
        if constexpr (JACOBI) {
            st2(r, i, r0, r1);
            const d2 dv = ld2(inv, i);
            z0 = dv.a * r0; z1 = dv.b * r1;                                          // jacobi.rs:84-86
            st2_sel<KEEP>(z, i, z0, z1);                                             // z is read again by the direction pass
        } else {
            st2_sel<KEEP>(r, i, r0, r1);                                             // z == r
        }
        const bool zz = norm_type == 0;                                              // Preconditioned: (z,z); else (r,r)
        if (in0) { acc[0] = acc[0] + r0 * z0; acc[1] = acc[1] + (zz ? z0 * z0 : r0 * r0); }
        if (in1) { acc[0] = acc[0] + r1 * z1; acc[1] = acc[1] + (zz ? z1 * z1 : r1 * r1); }
    }
};

struct PcgRun : SolverRun {
    using SolverRun::SolverRun;
    double *r = nullptr, *z = nullptr, *ap = nullptr;
    DirectionVec dir{*this};
    bool alias = false, jac = false;
    const double* inv_diag = nullptr;  // jac: the Jacobi preconditioner's inverse diagonal, fused into the residual update
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        // radius / obj_target are fields of PcgSolver (pcg.rs:39-41) but PcgSolver::solve never reads them: accepted, ignored
        KR_TRY(common_begin(prm.max_iters + 2, dir.plan(cg_defer_x(), true, 4)));                 // pcg.rs:117
        alias = !pc || pc->kind == KR_PC_IDENTITY;      // z == r  (pcg.rs:130,186 clone_from / IdentityPC)
        jac = pc && pc->kind == KR_PC_JACOBI;
        inv_diag = pc_jacobi_inv_diag(pc);
        KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&dir.pp)); KR_TRY(ws.vec(&ap));
        KR_TRY(dir.alloc());
        if (alias) z = r; else KR_TRY(ws.vec(&z));
        KR_TRY(launch_spmv(a, xw, ap, 0, nullptr, nullptr));                                      // :119-124
        KR_TRY(launch_ew(ctx, SubDotOp{bv->d, ap, r}, n, nullptr));
        if (!alias) KR_TRY(pc_apply_dev(pc, n, r, z, nullptr));                                      // :127-131 (`?`)
        KR_HIP(hipMemcpyAsync(dir.pp, z, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));  // :132
        const double* nq_a = (prm.norm_type == 0) ? z : r;      // Preconditioned: (z,z); Unpreconditioned: (r,r)
        KR_TRY(launch_ew(ctx, DotPairOp{r, z, nq_a, nq_a}, n, nullptr));
        return reduce_then<2>(ctx, nt, ws.red, PcgInitLogic{lc});
    }
    int32_t flush() override { return dir.flush(); }
    int32_t iterate(int64_t it) override {
        const int nt_ = prm.norm_type;
        KR_TRY(dir.spmv(it, z, ap));                                                              // :149-160
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, PcgAlphaLogic{lc})));
        double* const pp = dir.pp;
        if (cg_defer_x()) {                                                                       // x += alpha p (:175-177) rides on the direction pass
            const bool keep = keep_in_cache(n);
            if (alias) {
                KR_TRY(by_bool(keep, [&](auto K) { return launch_ew(ctx, PcgResidualOp<false, K()>{&ws.st->alpha, ap, r, z, nullptr, nt_}, n, done); }));
            } else if (jac) {
                KR_TRY(by_bool(keep, [&](auto K) { return launch_ew(ctx, PcgResidualOp<true, K()>{&ws.st->alpha, ap, r, z, inv_diag, nt_}, n, done); }));
            } else {
                KR_TRY(launch_ew(ctx, CgResidual0Op{&ws.st->alpha, ap, r}, n, done));             // :179-181
                KR_TRY(pc_apply_dev(pc, n, r, z, done));                                             // :183-187
                const double* nq_a = (nt_ == 0) ? z : r;
                KR_TRY(launch_ew(ctx, DotPairOp{r, z, nq_a, nq_a}, n, done));                     // :188-195
            }
            KR_TRY((reduce_then<2>(ctx, nt, ws.red, PcgBetaLogic{lc})));
            return dir.advance(it, z, (alias || jac) && keep);                                    // (KEEP only where the residual pass above stored z itself)
        }
        if (alias) {
            KR_TRY(launch_ew(ctx, PcgUpdateOp<false>{&ws.st->alpha, pp, ap, xw, r, z, nullptr, nt_}, n, done));
        } else if (jac) {
            KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_ew(ctx, PcgUpdateOp<true, K()>{&ws.st->alpha, pp, ap, xw, r, z, inv_diag, nt_}, n, done); }));
        } else {
            KR_TRY(launch_ew(ctx, CgUpdate0{&ws.st->alpha, pp, ap, xw, r}, n, done));             // :175-181
            KR_TRY(pc_apply_dev(pc, n, r, z, done));                                                 // :183-187
            const double* nq_a = (nt_ == 0) ? z : r;
            KR_TRY(launch_ew(ctx, DotPairOp{r, z, nq_a, nq_a}, n, done));                         // :188-195
        }
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, PcgBetaLogic{lc})));
        return by_bool(jac && !alias && keep_in_cache(n), [&](auto K) { return launch_ew(ctx, AypxDevOp<K()>{&ws.st->beta, z, pp}, n, done); });   // :215-217
    }
};

SolverRun* make_pcg_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io) { return new PcgRun(b, x, io); }

int32_t pcg_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io) {
    KR_ARG(io.a && io.params, "solve: null argument");
    PcgRun run(bv, xv, io);
    return run.solve();
}

}  // namespace kr
