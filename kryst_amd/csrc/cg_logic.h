// The scalar steps of CG (src/solver/cg.rs:127-284) and PCG (src/solver/pcg.rs:133-218): run by thread 0 of the kernel that ends a fold,
// on the reduced values.  Shared by the single-vector solvers (cg_pcg.hip) and the batched ones (multi.hip), which bind one instance per
// column to that column's DevState -- the same code, so the same scalars.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kr {

// ---- x paid in SLICES (cg_pcg.hip: DirectionVec, XBatchOp): which rows owe which x updates.  Host only -- no device type, no HIP call -- so that
// tests/cpp/test_x_slices.cpp drives it on the CPU (it defines KRYST_X_SLICES_HOST_ONLY, which ends this header after the struct).
// With a batch length m the NT tiles of the vector are cut into `slices` ranges on tile boundaries, slice j = tiles [j NT / slices, (j + 1) NT / slices)
// (empty where NT < slices).  slices == 1: the whole vector in one pass every m iterations.  slices == m: iteration `it` pays slice it % m, the
// updates applied[j] + 1 .. it, which are m of them once the first m iterations are behind (1 .. m before that).  Per row the updates stay
// x = x + alpha_i p_i for i ascending, each applied once: the bits do not depend on the cut.
// Ring safety: p_i lives in slot i % (m + 1) and the fused SpMV (or the ring direction pass) that forms p_{it+1} overwrites the slot of p_{it-m}.
// After advance(it) every slice has applied[j] >= it - m + 1 (slices == m: slice j was paid at one of the last m iterations; slices == 1: at the
// last multiple of m), so no launch -- neither a later advance nor the flush -- ever reads a slot that has been overwritten.
struct XSliceLaunch { int64_t tile_lo, tile_hi; long long lo, hi; };          // x += alpha_i p_i for i = lo .. hi on tiles [tile_lo, tile_hi)
struct XSlices {
    int m = 1, slices = 1; int64_t nt = 0;
    std::vector<long long> applied;                                           // per slice: the last iteration whose update its rows have
    void init(int m_, int64_t nt_, bool sliced) {
        m = std::max(1, m_); nt = std::max<int64_t>(0, nt_); slices = sliced ? m : 1;
        applied.assign((size_t)slices, 0);
    }
    int64_t tile_at(int j) const { return (int64_t)j * nt / slices; }           // (j <= 32 and nt < 2^53: no overflow)
    bool launch_of(int j, long long upto, XSliceLaunch* out) {
        const XSliceLaunch l{tile_at(j), tile_at(j + 1), applied[(size_t)j] + 1, upto};
        applied[(size_t)j] = std::max(applied[(size_t)j], upto);
        if (l.hi < l.lo || l.tile_hi <= l.tile_lo) return false;              // nothing owed, or an empty slice
        *out = l;
        return true;
    }
    // iteration `it` has been enqueued: the launch it pays, if any
    bool advance(long long it, XSliceLaunch* out) {
        const int j = (int)(it % m);
        return j < slices && launch_of(j, it, out);
    }
    // no further iteration follows `upto` for now: what every slice still owes.  The bookkeeping stays valid for a session that goes on.
    void flush(long long upto, std::vector<XSliceLaunch>& out) {
        out.clear();
        XSliceLaunch l;
        for (int j = 0; j < slices; ++j)
            if (launch_of(j, upto, &l)) out.push_back(l);
    }
};

}  // namespace kr

#ifndef KRYST_X_SLICES_HOST_ONLY
#include "solver_common.h"

namespace kr {

struct CgInitLogic {             // cg.rs:127-140
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
#endif  // KRYST_X_SLICES_HOST_ONLY
