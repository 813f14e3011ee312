// Compressed-basis GMRES(m) -- a LABELLED EXTENSION, not in the reference: restarted GMRES whose Krylov basis V is
// STORED in fp32 while every operation stays fp64.  A basis vector is rounded once, (float) round-to-nearest-even, in the pass that stores it
// (v_0 = r / beta, v_{j+1} = z / h[j+1][j]); every later use -- the operand of the next SpMV or preconditioner apply, B_i and B_next of the
// Gram-Schmidt links, the x update -- widens exactly what was stored, so the Arnoldi relation holds for V as stored.  The operator, the
// preconditioner, z, x, the Hessenberg matrix and all scalars are fp64, and the true residual is recomputed in fp64 at every restart.
// basis = KRYST_BASIS_F64 is the control: the same loop, the same kernels' text, nothing rounded.
//
// precond_side 0 (or pc == NULL): the loop of gmres_solve side 0 statement for statement (gmres.rs:216-402 through arnoldi :65-105), with its
// logic steps (gmres_common.h).  precond_side 2: TEXTBOOK right preconditioning -- Arnoldi on A M^-1 from the true residual, v_0 = r_0 / ||r_0||,
// w = M^-1 v_j, z = A w; only V is kept (the as-written Right arm keeps Z = M^-1 V, R + 1 more fp64 vectors); at the cycle end
// u = sum_j y_j V_j (ascending j, from zero), x <- x + M^-1 u, one apply per cycle.  Happy breakdown as in arnoldi (Givens still applied).
//
// The SpMV and the preconditioner read fp64, so the store pass also writes the widened value into ONE fp64 scratch vector (8 B per row once per
// iteration, against 2(j+1) links).  Side 0 keeps the fused first dot of launch_spmv(a, v, w, 1, v_0): the cycle's first store pass writes its
// widened copy into a vector of its own, which stays for the cycle.  Side 2 takes that dot in a pass of its own (CbDotOp) and keeps no such copy.
#include "gmres_common.h"
#include "solvers.h"

namespace kr {

// ---- the basis as stored: fp64 (control) or fp32.  A lane's two floats are ONE 8-byte access at i = q*512 + 2t.
typedef float kr_v2f __attribute__((ext_vector_type(2)));
template <bool KEEP> __device__ __forceinline__ d2 ldb(const double* p, int64_t i) { return ld2_sel<KEEP>(p, i); }
template <bool KEEP> __device__ __forceinline__ d2 ldb(const float* p, int64_t i) {
    kr_v2f v;
#if KR_NT & 1
    if constexpr (KEEP) v = *reinterpret_cast<const kr_v2f*>(p + i); else v = __builtin_nontemporal_load(reinterpret_cast<const kr_v2f*>(p + i));
#else
    v = *reinterpret_cast<const kr_v2f*>(p + i);
#endif
    return {(double)v.x, (double)v.y};                                  // widening is exact
}
// store (a, b); returns what now stands in memory, widened
__device__ __forceinline__ d2 stb(double* p, int64_t i, double a, double b) { st2(p, i, a, b); return {a, b}; }
__device__ __forceinline__ d2 stb(float* p, int64_t i, double a, double b) {
    kr_v2f v; v.x = (float)a; v.y = (float)b;                           // the one rounding of a store
#if KR_NT & 2
    __builtin_nontemporal_store(v, reinterpret_cast<kr_v2f*>(p + i));
#else
    *reinterpret_cast<kr_v2f*>(p + i) = v;
#endif
    return {(double)v.x, (double)v.y};
}

// ---- vector ops
template <class T>
struct CbStoreOp {                   // V_k = store(in / s) ; vcur = widen(V_k)   (v_0 = r / beta, v_{j+1} = z / h[j+1][j])
    static constexpr int NQ = 0; static constexpr const char* TAG = "CbStore";
    const double* s; const double* in; T* vk; double* vcur;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double d = *s;
        const d2 a = ld2(in, i);
        const d2 w = stb(vk, i, a.a / d, a.b / d);
        st2(vcur, i, w.a, w.b);
    }
};
template <bool KEEP, class T>
struct CbLinkOp {                    // MgsLinkOp over a stored basis: z = z - h*widen(Bi) ; partial z.widen(Bnext), or z.z of the UPDATED z (bnext == nullptr)
    static constexpr int NQ = 1; static constexpr const char* TAG = "CbLink";
    const double* h; const T* bi; const T* bnext; double* z;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double hv = *h;
        const d2 zz = ld2_sel<KEEP>(z, i), b = ldb<false>(bi, i);        // as MgsLinkOp: z and Bnext cacheable under KEEP, Bi streaming
        const double z0 = zz.a - hv * b.a, z1 = zz.b - hv * b.b;
        st2_sel<KEEP>(z, i, z0, z1);
        d2 nx{z0, z1};
        if (bnext) nx = ldb<KEEP>(bnext, i);
        if (in0) acc[0] = acc[0] + z0 * nx.a;
        if (in1) acc[0] = acc[0] + z1 * nx.b;
    }
};
template <class T>
struct CbDotOp {                     // partial z.widen(B_0): the first dot of the sweep where the SpMV does not carry it
    static constexpr int NQ = 1; static constexpr const char* TAG = "CbDot"; static constexpr int BPC = 4;
    const double* z; const T* b0;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const d2 u = ld2(z, i), v = ldb<false>(b0, i);
        if (in0) acc[0] = acc[0] + u.a * v.a;
        if (in1) acc[0] = acc[0] + u.b * v.b;
    }
};
template <bool FROM_ZERO, class T>
struct CbBasisUpdateOp {             // BasisUpdateOp over a table of stored basis vectors: x += sum_j y[j] widen(U[j]), j ascending, j < *m
    static constexpr int NQ = 0; static constexpr const char* TAG = "CbBasisUpdate";
    const int* m; const double* y; T* const* u; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const int mm = *m;
        d2 xx{0.0, 0.0};
        if constexpr (!FROM_ZERO) xx = ld2(x, i);
        for (int j0 = 0; j0 < mm; j0 += 8) {                 // 8 basis vectors in flight; the sum keeps its ascending order
            d2 uu[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) uu[k] = ldb<false>(u[min(j0 + k, mm - 1)], i);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (j0 + k < mm) { const double yj = y[j0 + k]; xx.a = xx.a + yj * uu[k].a; xx.b = xx.b + yj * uu[k].b; }
        }
        st2(x, i, xx.a, xx.b);
    }
};
struct CbAddOp {                     // x = x + t   (x <- x + M^-1 u at the end of a right-preconditioned cycle)
    static constexpr int NQ = 0; static constexpr const char* TAG = "CbAdd";
    const double* t; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 a = ld2(x, i), b = ld2(t, i);
        st2(x, i, a.a + b.a, a.b + b.b);
    }
};

static inline int32_t basis_vec(Workspace& ws, double** out) { return ws.vec(out); }
static inline int32_t basis_vec(Workspace& ws, float** out) { return ws.vec32(out); }
static inline int64_t basis_reserve(const Workspace& ws, int64_t count, const double*) { return count; }
static inline int64_t basis_reserve(const Workspace& ws, int64_t count, const float*) { return ws.vecs_for32(count); }

template <class T>
static int32_t cb_run(RestartRun& run, int side, kryst_pc_t pc) {
    const kryst_params_t* p = run.p;
    const int R = p->restart;
    const int64_t n_outer = (p->max_iters + R - 1) / R;                                            // gmres.rs:231
    // fp64: xk, r0, w, z, tmp, vcur and (side 0) the widened v_0 ; the basis: R + 1 vectors of T
    KR_TRY(run.begin(n_outer * R + 2, (side == 0 ? 7 : 6) + basis_reserve(run.ws, R + 1, (const T*)nullptr)));
    kryst_csr_t a = run.a; kryst_ctx_t ctx = run.ctx; const int64_t n = run.n, nt = run.nt;
    Workspace& ws = run.ws; const LogicCtx& lc = run.lc; LiveMonitor& mon = run.mon; const int* done = run.done;
    GmPtrs P; P.restart = R;
    int* d_gate = nullptr; T** d_uptr = nullptr;
    SmallArena small;
    auto carve = [&] {
        P.h = small.take<double>((size_t)(R + 1) * R); P.g = small.take<double>(R + 1);
        P.cs = small.take<double>(R); P.sn = small.take<double>(R); P.y = small.take<double>(R);
        P.gs = small.take<GmState>(1); d_gate = small.take<int>(1); d_uptr = small.take<T*>(R + 1);
    };
    carve(); KR_TRY(small.alloc(ws)); carve();
    double *xk, *r0, *w, *z, *tmp, *vcur, *v0w = nullptr;
    KR_TRY(ws.vec(&xk)); KR_TRY(ws.vec(&r0)); KR_TRY(ws.vec(&w)); KR_TRY(ws.vec(&z)); KR_TRY(ws.vec(&tmp)); KR_TRY(ws.vec(&vcur));
    if (side == 0) KR_TRY(ws.vec(&v0w));
    std::vector<T*> V((size_t)R + 1);
    for (auto& v : V) KR_TRY(basis_vec(ws, &v));
    KR_HIP(hipMemcpyAsync(d_uptr, V.data(), sizeof(T*) * (size_t)(R + 1), hipMemcpyHostToDevice, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    const CycleGate cyc{done, &P.gs->cyc_stop};
    constexpr int word = (int)sizeof(T);       // launch_iter and the choice of the link instance judge their byte thresholds on the stored basis
    const bool keep = keep_links_in_cache(n, word);
    int32_t rc = KRYST_OK;

    KR_HIP(hipMemcpyAsync(xk, run.xv->d, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));   // :219
    KR_TRY(residual_dot(a, run.bv->d, xk, r0, tmp, nullptr));                                     // :221-227
    KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmInitLogic{lc, P, 0})));

    for (int64_t outer = 0; outer < n_outer; ++outer) {                                           // :234
        // ---- cycle start: v_0 = r_0 / ||r_0|| of the TRUE residual on either side (:238, :242 / :263)
        KR_TRY(logic_only(ctx, ws.red, GmCycleLogic{lc, P, 0}));
        KR_TRY(launch_ew(ctx, CbStoreOp<T>{&P.gs->r0_norm, r0, V[0], side == 0 ? v0w : vcur}, n, done));
        // ---- Arnoldi loop (:276-355); everything is gated on done || cyc_stop
        for (int j = 0; j < R; ++j) {
            KR_TRY(logic_only(ctx, ws.red, GmStepBeginLogic{lc, P}));
            KR_TRY(write_cycle_gate(ctx, cyc, d_gate));
            double* zz;
            if (side == 2) {                                                                      // w = M^-1 v_j, z = A w
                rc = pc_apply_dev_fresh(pc, n, vcur, w, d_gate, nullptr); if (rc) return rc;
                KR_TRY(launch_spmv(a, w, z, 0, nullptr, d_gate));
                zz = z;
                KR_TRY(launch_iter(ctx, CbDotOp<T>{zz, V[0]}, n, cyc, word));
            } else {                                                                              // arnoldi :79-81
                KR_TRY(launch_spmv(a, j == 0 ? v0w : vcur, w, 1, v0w, d_gate));                   // + (w, widen(V[0]))
                zz = w;
            }
            // double modified Gram-Schmidt (:83-96): 2(j+1) fused links
            for (int sweep = 0; sweep < 2; ++sweep)
                for (int i = 0; i <= j; ++i) {
                    KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmHLogic{lc, P, i, j, sweep})));
                    const bool last = (sweep == 1 && i == j);
                    const T* nxt = last ? nullptr : (i < j ? V[i + 1] : V[0]);                        // last link: ||z||^2 (:97)
                    KR_TRY(by_bool(keep, [&](auto K) { return launch_iter(ctx, CbLinkOp<K(), T>{&P.gs->hcur, V[i], nxt, zz}, n, cyc, word); }));
                }
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmNormLogic{lc, P, j})));
            // v_{j+1} = store(z / h[j+1][j]) (:102-103) and its widened copy for the next SpMV / apply; skipped once the cycle is left
            KR_TRY(launch_iter(ctx, CbStoreOp<T>{&P.gs->hj1, zz, V[j + 1], vcur}, n, cyc, word));
        }
        // ---- cycle end (:357-398)
        KR_TRY(logic_only(ctx, ws.red, GmBackLogic{lc, P}));
        if (side == 2) {                                                                          // u = sum y_j V_j ; x += M^-1 u
            KR_TRY(launch_ew(ctx, CbBasisUpdateOp<true, T>{&P.gs->m, P.y, d_uptr, w}, n, done));
            rc = pc_apply_dev_fresh(pc, n, w, z, done, nullptr); if (rc) return rc;
            KR_TRY(launch_ew(ctx, CbAddOp{z, xk}, n, done));
        } else {
            KR_TRY(launch_ew(ctx, CbBasisUpdateOp<false, T>{&P.gs->m, P.y, d_uptr, xk}, n, done));
        }
        KR_TRY(residual_dot(a, run.bv->d, xk, r0, tmp, done));
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, GmCycleEndLogic{lc, P})));
        KR_HIP(hipStreamSynchronize(ctx->s_main));                                                // one host sync per restart cycle
        mon.poll();
        if (ctx->h_prog->done) break;
    }
    return run.end(xk);
}

int32_t cbgmres_solve(kryst_vec_t bv, kryst_vec_t xv, int32_t basis, const SolveIO& io) {
    const EnvFreeze knobs;                    // the tuning knobs are read once per solve, not per launch
    KR_ARG(io.a && io.params, "solve: null argument");
    const kryst_params_t* p = io.params;
    KR_ARG(p->precond_side >= 0 && p->precond_side <= 3, "cbgmres: precond_side");
    KR_ARG(basis == KRYST_BASIS_F64 || basis == KRYST_BASIS_F32, "cbgmres: basis must be KRYST_BASIS_F64 or KRYST_BASIS_F32");
    const int side = io.pc ? p->precond_side : 0;     // as GmresSolver: without a preconditioner every side is the unpreconditioned loop
    const kryst_pc_t pc = side ? io.pc : nullptr;
    RestartRun run(bv, xv, io);
    KR_TRY(run.check(pc, "cbgmres: restart out of range"));
    if (side == 1 || side == 3) { set_error("cbgmres: left preconditioning is not supported (None or Right)"); return KRYST_UNSUPPORTED; }
    if (io.a->dist || io.a->ctx->nranks > 1) { set_error("cbgmres: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    return basis == KRYST_BASIS_F32 ? cb_run<float>(run, side, pc) : cb_run<double>(run, side, pc);
}

}  // namespace kr
