// Device-resident restarted GMRES(m): GmresSolver::solve (src/solver/gmres.rs:216-402) with its helpers
// arnoldi (:65-105), apply_givens_and_update_g (:154-176) and back_substitution (:180-192), restated literally
// -- including the non-standard Left variant (orthogonalisation against Z[0..=j] with Z[0] = M^-1 v0, x updated
// with V), the branch asymmetries on happy breakdown and the epsilon = 1e-14 guards.
//
// Hessenberg matrix, Givens rotations and g live in device memory and are updated by one-thread logic kernels,
// so the 2(j+1) dependent dot -> axpy links of the double modified Gram-Schmidt sweep never touch the host.
// Each link is ONE pass over HBM:  z <- z - h_i B_i  fused with the next link's dot (z, B_{i+1})  (4n words
// instead of the reference's 5n); the last link fuses ||z||^2.
#include "gmres_common.h"
#include "solvers.h"

namespace kr {

// ---- vector ops
template <bool KEEP>
struct MgsLinkOp {                   // z = z - h*Bi (gmres.rs:85-87) ; partial z.Bnext (the next link's dot, :84/:91)
    static constexpr int NQ = 1; static constexpr const char* TAG = "MgsLink";         // bnext == nullptr: partial z.z of the UPDATED z (h[j+1][j] = ||z||, :97)
    const double* h; const double* bi; const double* bnext; double* z;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double hv = *h;
        // z is read again by the very next link and Bnext is its Bi: cacheable accesses for those two, streaming for Bi
        // when they can survive in the memory-side cache (GMRES(30): 256^3 310 -> 336 it/s, 128^3 1377 -> 1495)
        const d2 zz = ld2_sel<KEEP>(z, i), b = ld2(bi, i);
        const double z0 = zz.a - hv * b.a, z1 = zz.b - hv * b.b;
        st2_sel<KEEP>(z, i, z0, z1);
        d2 nx{z0, z1};
        if (bnext) nx = ld2_sel<KEEP>(bnext, i);
        if (in0) acc[0] = acc[0] + z0 * nx.a;
        if (in1) acc[0] = acc[0] + z1 * nx.b;
    }
};

int32_t gmres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io) {
    const EnvFreeze knobs;                    // the tuning knobs are read once per solve, not per launch
    KR_ARG(io.a && io.params, "solve: null argument");
    const kryst_params_t* p = io.params;
    const int side = io.pc ? p->precond_side : 0;     // `match (self.preconditioning, pc)`: anything else takes the `_` arm
    const kryst_pc_t pc = side ? io.pc : nullptr;
    RestartRun run(bv, xv, io);
    KR_TRY(run.check(pc, "gmres: restart out of range"));
    // side 3 -- a LABELLED EXTENSION, not in the reference: textbook left preconditioning (Arnoldi on M^-1 A from M^-1 r0 / ||M^-1 r0||,
    // Gram-Schmidt against V, in-cycle test on the preconditioned residual, cycle-end test on the true one; oracle: kro_gmres side 3).
    // The reference's own Left arm (side 1) orthogonalises against an un-normalised Z[0] and stagnates on BASELINE config 3.
    KR_ARG(side >= 0 && side <= 3, "gmres: precond_side");
    const int R = p->restart;
    const int64_t n_outer = (p->max_iters + R - 1) / R;                                            // :231
    KR_TRY(run.begin(n_outer * R + 2, 5 + (R + 1) + (side == 1 ? 1 : side == 2 ? R + 1 : 0)));
    kryst_csr_t a = run.a; kryst_ctx_t ctx = run.ctx; const int64_t n = run.n, nt = run.nt;
    Workspace& ws = run.ws; const LogicCtx& lc = run.lc; LiveMonitor& mon = run.mon; const int* done = run.done;
    GmPtrs P; P.restart = R;
    int* d_gate = nullptr; double** d_uptr = nullptr;
    SmallArena small;
    auto carve = [&] {
        P.h = small.take<double>((size_t)(R + 1) * R); P.g = small.take<double>(R + 1);
        P.cs = small.take<double>(R); P.sn = small.take<double>(R); P.y = small.take<double>(R);
        P.gs = small.take<GmState>(1); d_gate = small.take<int>(1); d_uptr = small.take<double*>(R + 1);
    };
    carve(); KR_TRY(small.alloc(ws)); carve();
    double *xk, *r0, *w, *z, *tmp;
    KR_TRY(ws.vec(&xk)); KR_TRY(ws.vec(&r0)); KR_TRY(ws.vec(&w)); KR_TRY(ws.vec(&z)); KR_TRY(ws.vec(&tmp));
    std::vector<double*> V((size_t)R + 1), Z((size_t)R + 1, nullptr);
    for (auto& v : V) KR_TRY(ws.vec(&v));
    if (side == 1) { KR_TRY(ws.vec(&Z[0])); for (int k = 1; k <= R; ++k) Z[k] = V[k]; }            // :305-306 Z[j+1] is V[j+1]
    if (side == 2) for (auto& v : Z) KR_TRY(ws.vec(&v));
    {
        const std::vector<double*>& U = (side == 2) ? Z : V;                                      // :362-386
        KR_HIP(hipMemcpyAsync(d_uptr, U.data(), sizeof(double*) * (size_t)(R + 1), hipMemcpyHostToDevice, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
    }
    const CycleGate cyc{done, &P.gs->cyc_stop};
    int32_t rc = KRYST_OK;

    KR_HIP(hipMemcpyAsync(xk, xv->d, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));      // :219
    KR_TRY(residual_dot(a, bv->d, xk, r0, tmp, nullptr));                                         // :221-227
    KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmInitLogic{lc, P, side})));

    for (int64_t outer = 0; outer < n_outer; ++outer) {                                           // :234
        // ---- cycle start
        if (side == 3) {                                                                          // extension: v0 = M^-1 r0 / ||M^-1 r0||
            rc = pc_apply_dev_fresh(pc, n, r0, z, done, nullptr); if (rc) return rc;
            KR_TRY(launch_ew(ctx, DotOneOp{z, z}, n, done));
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmCycleLogic{lc, P, 2})));
            KR_TRY(launch_ew(ctx, DivOp{&P.gs->r0_norm, z, V[0]}, n, done));
        } else if (side == 2) {                                                                   // :248-260
            rc = pc_apply_dev_fresh(pc, n, r0, z, done, nullptr); if (rc) return rc;
            KR_TRY(launch_ew(ctx, DotOneOp{z, z}, n, done));
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmCycleLogic{lc, P, 1})));
            KR_TRY(launch_ew(ctx, DivOp{&P.gs->r0_norm, z, V[0]}, n, done));
            rc = pc_apply_dev_fresh(pc, n, V[0], Z[0], done, nullptr); if (rc) return rc;
        } else {
            KR_TRY(logic_only(ctx, ws.red, GmCycleLogic{lc, P, 0}));
            KR_TRY(launch_ew(ctx, DivOp{&P.gs->r0_norm, r0, V[0]}, n, done));                     // :242 / :263
            if (side == 1) { rc = pc_apply_dev_fresh(pc, n, V[0], Z[0], done, nullptr); if (rc) return rc; }       // :244-246
        }
        // ---- Arnoldi loop (:276-355); everything is gated on done || cyc_stop
        for (int j = 0; j < R; ++j) {
            KR_TRY(logic_only(ctx, ws.red, GmStepBeginLogic{lc, P}));
            KR_TRY(write_cycle_gate(ctx, cyc, d_gate));
            double* zz; const std::vector<double*>& B = (side == 1) ? Z : V;
            if (side == 1) {                                                                      // :281-284
                KR_TRY(launch_spmv(a, V[j], w, 0, nullptr, d_gate));
                rc = pc_apply_dev_fresh(pc, n, w, z, d_gate, nullptr); if (rc) return rc;
                zz = z;
                KR_TRY(launch_iter(ctx, DotOneOp{zz, B[0]}, n, cyc));
            } else if (side == 3) {                                                               // extension: z = M^-1 A v_j against V
                KR_TRY(launch_spmv(a, V[j], w, 0, nullptr, d_gate));
                rc = pc_apply_dev_fresh(pc, n, w, z, d_gate, nullptr); if (rc) return rc;
                zz = z;
                KR_TRY(launch_iter(ctx, DotOneOp{zz, B[0]}, n, cyc));
            } else if (side == 2) {                                                               // :311-317
                rc = pc_apply_dev_fresh(pc, n, V[j], w, d_gate, nullptr); if (rc) return rc;
                KR_TRY(launch_spmv(a, w, z, 1, V[0], d_gate));                                    // + (w2, V[0])
                zz = z;
            } else {                                                                              // arnoldi :79-81
                KR_TRY(launch_spmv(a, V[j], w, 1, V[0], d_gate));                                 // + (w, V[0])
                zz = w;
            }
            // double modified Gram-Schmidt (:83-96 / :286-298 / :318-330): 2(j+1) fused links
            for (int sweep = 0; sweep < 2; ++sweep)
                for (int i = 0; i <= j; ++i) {
                    KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmHLogic{lc, P, i, j, sweep})));
                    const bool last = (sweep == 1 && i == j);
                    const double* nxt = last ? nullptr : (i < j ? B[i + 1] : B[0]);                    // last link: ||z||^2 (:97)
                    KR_TRY(by_bool(keep_in_cache(n), [&](auto K) { return launch_iter(ctx, MgsLinkOp<K()>{&P.gs->hcur, B[i], nxt, zz}, n, cyc); }));
                }
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmNormLogic{lc, P, j})));
            // v_{j+1} = z / h[j+1][j] (:102-103 / :304-306 / :336-341); skipped once the cycle is left
            KR_TRY(launch_iter(ctx, DivOp{&P.gs->hj1, zz, V[j + 1]}, n, cyc));
            if (side == 2) {
                KR_TRY(write_cycle_gate(ctx, cyc, d_gate));
                rc = pc_apply_dev_fresh(pc, n, V[j + 1], Z[j + 1], d_gate, nullptr); if (rc) return rc;
            }
        }
        // ---- cycle end (:357-398)
        KR_TRY(logic_only(ctx, ws.red, GmBackLogic{lc, P}));
        KR_TRY(launch_ew(ctx, BasisUpdateOp<false>{&P.gs->m, P.y, d_uptr, xk}, n, done));
        KR_TRY(residual_dot(a, bv->d, xk, r0, tmp, done));
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmCycleEndLogic{lc, P})));
        // one host sync per restart cycle (a cycle is tens of ms of device work)
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        if (ctx->nranks > 1) KR_HIP(hipStreamSynchronize(ctx->s_comm));
        mon.poll();                                                                               // live monitor: once per restart cycle
        if (ctx->h_prog->done) break;
    }
    return run.end(xk);
}

}  // namespace kr
