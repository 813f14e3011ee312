// Mixed precision: CG and Jacobi-PCG on fp32-stored vectors and a lowered operator -- the pointwise passes and the driver.
#include "mixed.h"
#include "cg_logic.h"

namespace kr {

struct f4 { float v[4]; };
__device__ __forceinline__ f4 ld4(const float* p, int64_t i) {
    const p_v4f q = *reinterpret_cast<const p_v4f*>(p + i);
    return {{q.x, q.y, q.z, q.w}};
}
// one 16-byte store; elements at or behind n are stored as +0.0 (the padding of a work vector stays zero)
__device__ __forceinline__ void st4(float* p, int64_t i, int64_t n, const f4& o) {
    p_v4f q;
    q.x = i < n ? o.v[0] : 0.0f; q.y = i + 1 < n ? o.v[1] : 0.0f; q.z = i + 2 < n ? o.v[2] : 0.0f; q.w = i + 3 < n ? o.v[3] : 0.0f;
    *reinterpret_cast<p_v4f*>(p + i) = q;
}

// Op: static constexpr int NQ; quad(i, n, acc): thread t of tile q owns elements q * 1024 + 4 t .. + 3; a fused reduction folds the thread's terms
// in index order, the butterfly, the 4 waves, and stores one partial per tile into partials[k * pstride + q].
template <class Op>
__global__ __launch_bounds__(KR32_T) void ew32_kernel(Op op, const int* done, int64_t n, int64_t ntiles, double* partials, int64_t pstride) {
    if (done && *done) return;
    constexpr int NQ = Op::NQ;
    constexpr int NA = NQ > 0 ? NQ : 1;
    __shared__ double lds[NA * (KR32_T / 64)];
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t i = q * KR32_TILE + (int64_t)threadIdx.x * KR32_V;
        double acc[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = 0.0;
        op.quad(i, n, acc);
        if constexpr (NQ > 0) {
            block_reduce_any<NA, KR32_T / 64>(acc, lds);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) partials[k * pstride + q] = acc[k];
            }
        }
    }
}

template <class Op>
inline int32_t launch_ew32(kryst_ctx_t ctx, const Op& op, int64_t n, const int* done, int phase = KR_PH_BLAS1) {
    const int64_t ntiles = ntiles32_of(n);
    if (ntiles <= 0) return KRYST_OK;
    if (Op::NQ > 0) KR_TRY(ensure_partials(ctx, ntiles));
    const int64_t grid = std::min<int64_t>(ntiles, (int64_t)ctx->num_cu * std::max(1, env_int("KRYST_EW32_BLOCKS_PER_CU", 3)));
    hipLaunchKernelGGL((ew32_kernel<Op>), dim3((unsigned)grid), dim3(KR32_T), 0, ctx->s_main, op, done, n, ntiles, ctx->d_partials, ctx->partials_cap);
    KR_HIP(hipGetLastError());
    phase_mark(ctx, phase);
    return KRYST_OK;
}

struct Dot32Op {
    static constexpr int NQ = 1;
    const float *a, *b;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&acc)[1]) const {
        const f4 u = ld4(a, i), v = ld4(b, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) { if (i + e < n) acc[0] = acc[0] + (double)u.v[e] * (double)v.v[e]; }
    }
};
// r = (float)(b - A x) (`bi - ax`, cg.rs:123), p = r (:126), partial (r, r) of the stored r (:127)
struct CgInit32Op {
    static constexpr int NQ = 1;
    const float *b, *ax; float *r, *p;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&acc)[1]) const {
        const f4 bb = ld4(b, i), aa = ld4(ax, i);
        f4 rr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            rr.v[e] = (float)((double)bb.v[e] - (double)aa.v[e]);
            if (i + e < n) acc[0] = acc[0] + (double)rr.v[e] * (double)rr.v[e];
        }
        st4(r, i, n, rr); st4(p, i, n, rr);
    }
};
// pcg.rs:119-133: r = (float)(b - A x), z = (float)(dinv * r) (Jacobi, jacobi.rs:84-86; else z == r), p = z, partials (r, z) and (z, z) | (r, r)
template <bool JACOBI>
struct PcgInit32Op {
    static constexpr int NQ = 2;
    const float *b, *ax; float *r, *z, *p; const float* inv; int norm_type;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&acc)[2]) const {
        const f4 bb = ld4(b, i), aa = ld4(ax, i);
        f4 dv = {{0.0f, 0.0f, 0.0f, 0.0f}};
        if constexpr (JACOBI) dv = ld4(inv, i);
        f4 rr, zz;
        const bool nz = norm_type == 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            rr.v[e] = (float)((double)bb.v[e] - (double)aa.v[e]);
            zz.v[e] = JACOBI ? (float)((double)dv.v[e] * (double)rr.v[e]) : rr.v[e];
            if (i + e < n) {
                const double rd = (double)rr.v[e], zd = (double)zz.v[e];
                acc[0] = acc[0] + rd * zd;
                acc[1] = acc[1] + (nz ? zd * zd : rd * rd);
            }
        }
        st4(r, i, n, rr);
        if constexpr (JACOBI) st4(z, i, n, zz);
        st4(p, i, n, zz);
    }
};
// cg.rs:207-223: x = (float)(x + alpha p), r = (float)(r - alpha Ap), partial (r, r) of the stored r
struct CgUpdate32Op {
    static constexpr int NQ = 1;
    const DevState* st; const float *p, *ap; float *x, *r;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&acc)[1]) const {
        const double al = st->alpha;
        const f4 pp = ld4(p, i), aa = ld4(ap, i);
        f4 xx = ld4(x, i), rr = ld4(r, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xx.v[e] = (float)((double)xx.v[e] + al * (double)pp.v[e]);
            rr.v[e] = (float)((double)rr.v[e] - al * (double)aa.v[e]);
            if (i + e < n) acc[0] = acc[0] + (double)rr.v[e] * (double)rr.v[e];
        }
        st4(x, i, n, xx); st4(r, i, n, rr);
    }
};
// pcg.rs:175-195: x, r as above, z = (float)(dinv * r) in the same pass, partials (r, z) and (z, z) | (r, r)
template <bool JACOBI>
struct PcgUpdate32Op {
    static constexpr int NQ = 2;
    const DevState* st; const float *p, *ap; float *x, *r, *z; const float* inv; int norm_type;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&acc)[2]) const {
        const double al = st->alpha;
        const f4 pp = ld4(p, i), aa = ld4(ap, i);
        f4 xx = ld4(x, i), rr = ld4(r, i), zz;
        f4 dv = {{0.0f, 0.0f, 0.0f, 0.0f}};
        if constexpr (JACOBI) dv = ld4(inv, i);
        const bool nz = norm_type == 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xx.v[e] = (float)((double)xx.v[e] + al * (double)pp.v[e]);
            rr.v[e] = (float)((double)rr.v[e] - al * (double)aa.v[e]);
            zz.v[e] = JACOBI ? (float)((double)dv.v[e] * (double)rr.v[e]) : rr.v[e];
            if (i + e < n) {
                const double rd = (double)rr.v[e], zd = (double)zz.v[e];
                acc[0] = acc[0] + rd * zd;
                acc[1] = acc[1] + (nz ? zd * zd : rd * rd);
            }
        }
        st4(x, i, n, xx); st4(r, i, n, rr);
        if constexpr (JACOBI) st4(z, i, n, zz);
    }
};
// p = (float)(z + beta p) (cg.rs:274-276 with z = r, pcg.rs:215-217)
struct Direction32Op {
    static constexpr int NQ = 0;
    const DevState* st; const float* z; float* p;
    __device__ __forceinline__ void quad(int64_t i, int64_t n, double (&)[1]) const {
        const double be = st->beta;
        const f4 zz = ld4(z, i);
        f4 pp = ld4(p, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp.v[e] = (float)((double)zz.v[e] + be * (double)pp.v[e]);
        st4(p, i, n, pp);
    }
};
int32_t launch_dot32(kryst_ctx_t ctx, const float* a, const float* b, int64_t n) { return launch_ew32(ctx, Dot32Op{a, b}, n, nullptr); }

int32_t solve32_check(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg) {
    KR_ARG(b && x && a && io.params, "solve32: null argument");
    KR_TRY(vec32_check(b)); KR_TRY(vec32_check(x)); KR_TRY(csr32_check(a));
    KR_ARG(b->ctx == a->ctx && x->ctx == a->ctx, "solve32: context mismatch");
    KR_ARG(io.params->max_iters >= 0, "solve32: max_iters < 0");
    KR_ARG(io.hist_cap >= 0, "solve32: hist_cap < 0");
    KR_ARG(!io.pc || io.pc->ctx == a->ctx, "solve32: preconditioner belongs to another context");
    const char* why = nullptr;
    if (a->nrows != a->ncols) why = "non-square operators";
    else if (io.params->norm_type != 0 && io.params->norm_type != 1) why = "norm types other than Preconditioned and Unpreconditioned";
    else if (io.params->has_radius) why = "the trust-region exit (with_radius)";
    else if (io.params->has_obj_target) why = "the objective exit (with_obj_target)";
    else if (pcg && io.pc && io.pc->kind != KR_PC_IDENTITY && io.pc->kind != KR_PC_JACOBI) why = "preconditioners other than Identity and Jacobi";
    if (why) { set_error("solve32: %s are not supported on fp32 storage", why); return KRYST_UNSUPPORTED; }
    KR_ARG(b->n == a->nrows && x->n == a->nrows, "solve32: vector length != operator size");
    KR_ARG(!io.pc || io.pc->n < 0 || io.pc->n == a->nrows, "solve32: preconditioner size mismatch");
    return KRYST_OK;
}

int32_t solve32(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg) {
    KR_TRY(solve32_check(b, x, a, io, pcg));
    const EnvFreeze knobs;
    kryst_ctx_t ctx = a->ctx;
    const kryst_params_t prm = *io.params;
    const int64_t n = a->nrows, nt = ntiles32_of(n);
    KR_HIP(hipSetDevice(ctx->device));
    Workspace ws(ctx, ws_len32(n));
    KR_TRY(ws.init(prm.max_iters + 2));
    if (ws.vec_bytes() < sizeof(float) * (size_t)vec32_len(n)) { set_error("solve32: a work vector is smaller than an fp32 vector"); return KRYST_ERR_HIP; }
    const bool jac = pcg && io.pc && io.pc->kind == KR_PC_JACOBI;
    KR_TRY(ws.reserve(jac ? 6 : 4));                                        // xw, r, p, ap [, z, dinv]
    const LogicCtx lc = ws.lctx(&prm);
    const int* done = &ws.st->done;
    const DevState* st = ws.st;
    float* v[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < (jac ? 6 : 4); ++k) { double* raw = nullptr; KR_TRY(ws.vec(&raw)); v[k] = reinterpret_cast<float*>(raw); }
    float *xw = v[0], *r = v[1], *p = v[2], *ap = v[3], *z = jac ? v[4] : r, *dinv = v[5];     // without Jacobi z == r (pcg.rs:130,186 / IdentityPC)
    if (n > 0) KR_HIP(hipMemcpyAsync(xw, x->d, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, ctx->s_main));
    if (jac && n > 0) KR_HIP(enqueue_round32(ctx, dinv, pc_jacobi_inv_diag(io.pc), n, 0, 1.0));       // the Jacobi values, rounded once per solve
    KR_TRY(launch_spmv32(a, xw, ap, 0, nullptr, nullptr));                  // cg.rs:120-122, pcg.rs:119-121
    if (!pcg) {
        KR_TRY(launch_ew32(ctx, CgInit32Op{b->d, ap, r, p}, n, nullptr));
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgInitLogic{lc})));
    } else {
        KR_TRY(by_bool(jac, [&](auto J) { return launch_ew32(ctx, PcgInit32Op<J()>{b->d, ap, r, z, p, dinv, prm.norm_type}, n, nullptr); }));
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, PcgInitLogic{lc})));
    }
    // three launches per iteration, each followed by its fold: no deferred x, no x batches, nothing fused into the SpMV
    auto iterate = [&](int64_t) -> int32_t {
        KR_TRY(launch_spmv32(a, p, ap, 1, p, done));                        // cg.rs:143-144 + (p, Ap) :164 ; pcg.rs:149-160
        if (!pcg) {
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgAlphaLogic{lc})));
            KR_TRY(launch_ew32(ctx, CgUpdate32Op{st, p, ap, xw, r}, n, done, KR_PH_BLAS1_RESIDUAL));
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgBetaLogic{lc})));
        } else {
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, PcgAlphaLogic{lc})));
            KR_TRY(by_bool(jac, [&](auto J) { return launch_ew32(ctx, PcgUpdate32Op<J()>{st, p, ap, xw, r, z, dinv, prm.norm_type}, n, done, KR_PH_BLAS1_RESIDUAL); }));
            KR_TRY((reduce_then<2>(ctx, nt, ws.red, PcgBetaLogic{lc})));
        }
        return launch_ew32(ctx, Direction32Op{st, z, p}, n, done, KR_PH_BLAS1_DIRECTION);
    };
    KR_TRY(run_ahead(ctx, &prm, iterate));
    DevState h;
    KR_TRY(finish_state(ws, pcg ? io.pc : nullptr, io.stats, io.hist, io.hist_cap, io.hist_len, &h));
    if (h.status == KRYST_ERR_HIP && fold_gave_up(ctx)) return h.status;
    if (h.status == KRYST_OK && n > 0)                                      // on Err the reference never reaches `*x = ...`
        KR_HIP(hipMemcpyAsync(x->d, xw, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return h.status;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_cg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats,
                             double* hist, int64_t hist_cap, int64_t* hist_len) {
    KR_ARG(!pc || !a || pc->ctx == a->ctx, "solve32: preconditioner belongs to another context");    // ignored (cg.rs:115 `let _ = pc;`), but of this context as for kryst_cg_solve_dev
    return solve32(b, x, a, Solve32IO{nullptr, params, stats, hist, hist_cap, hist_len}, false);
}

int32_t kryst_pcg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats,
                              double* hist, int64_t hist_cap, int64_t* hist_len) {
    return solve32(b, x, a, Solve32IO{pc, params, stats, hist, hist_cap, hist_len}, true);
}

}  // extern "C"
