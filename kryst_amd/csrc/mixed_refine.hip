// Mixed precision: fp64 iterative refinement around the fp32-stored CG / PCG of mixed_cg.hip.
#include "mixed.h"
#include "solver_common.h"

namespace kr {

// xn = x + rho * (double)c
__global__ void correct_kernel(double* xn, const double* x, const float* c, double rho, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) xn[i] = x[i] + rho * (double)c[i];
}

struct RefineWork {                                   // the vectors of one refinement, freed on every way out
    kryst_vec_t v64[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    kryst_vec32_t v32[2] = {nullptr, nullptr};
    ~RefineWork() {
        for (kryst_vec_t v : v64) (void)kryst_vec_destroy(v);
        for (kryst_vec32_t v : v32) vec32_free(v);
    }
};

// rho = sqrt((r, r)) with r = b - A x: the fp64 SpMV of whatever encoding `a` streams, SubDotOp's partials and the fp64 fold; one scalar to the host
static int32_t refine_residual(kryst_csr_t a, const double* b, const double* x, double* r, double* tmp, double* rho) {
    KR_TRY(residual_dot(a, b, x, r, tmp, nullptr));
    double rr = 0.0;
    KR_TRY(fold_to_host(a->ctx, ntiles_of(a->nrows), &rr));
    *rho = __builtin_sqrt(rr);
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_refine_solve_dev(kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_csr32_t a32, kryst_pc_t pc, const kryst_params_t* outer,
                               const kryst_params_t* inner, kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len,
                               int64_t* inner_iters, int64_t inner_cap) {
    KR_ARG(b && x && a && a32 && outer && inner, "refine: null argument");
    KR_TRY(csr32_check(a32));
    KR_ARG(b->ctx == a->ctx && x->ctx == a->ctx && a32->ctx == a->ctx, "refine: context mismatch");
    KR_ARG(a32->nrows == a->nrows && a32->ncols == a->ncols && a32->nnz == a->nnz, "refine: a32 is not the lowering of an operator with a's shape");
    KR_ARG(hist_cap >= 0 && inner_cap >= 0, "refine: negative capacity");
    KR_ARG(!pc || pc->ctx == a->ctx, "refine: preconditioner belongs to another context");
    if (a->dist || a->ctx->nranks > 1) { set_error("refine: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    const bool pcg = pc && pc->kind == KR_PC_JACOBI;
    if (pc && pc->kind != KR_PC_IDENTITY && pc->kind != KR_PC_JACOBI) { set_error("refine: preconditioners other than Identity and Jacobi are not supported"); return KRYST_UNSUPPORTED; }
    kryst_ctx_t ctx = a->ctx;
    const int64_t n = a->nrows;
    KR_HIP(hipSetDevice(ctx->device));
    RefineWork wk;
    for (int k = 0; k < 2; ++k) KR_TRY(vec32_alloc(ctx, n, &wk.v32[k]));
    kryst_vec32_t r32 = wk.v32[0], c32 = wk.v32[1];
    const Solve32IO inner_io{pcg ? pc : nullptr, inner, nullptr, nullptr, 0, nullptr};
    KR_TRY(solve32_check(r32, c32, a32, inner_io, pcg));                    // (also: square operator, the inner parameters)
    KR_ARG(b->n == n && x->n == n, "refine: vector length != operator size");
    if (ctx->active_ws != nullptr) { set_error("context busy: a solve or stepping session is already open on this context (one at a time)"); return KRYST_ERR_BUSY; }
    for (int k = 0; k < 5; ++k) KR_TRY(kryst_vec_create(ctx, n, &wk.v64[k]));
    double *xw = wk.v64[0]->d, *r = wk.v64[1]->d, *xn = wk.v64[2]->d, *rn = wk.v64[3]->d, *tmp = wk.v64[4]->d;
    KR_TRY(kryst_vec_copy(wk.v64[0], x));
    int64_t pushed = 0;
    auto push = [&](double v) { if (hist && pushed < hist_cap) hist[pushed] = v; ++pushed; if (hist_len) *hist_len = pushed; };
    auto report = [&](int64_t it, double res, int conv) { if (stats) { stats->iterations = it; stats->final_residual = res; stats->converged = conv; } };
    if (hist_len) *hist_len = 0;
    double rho = 0.0;
    KR_TRY(refine_residual(a, b->d, xw, r, tmp, &rho));
    const double rho0 = rho;
    push(rho0);
    report(0, rho0, 0);
    if (outer->max_iters <= 0 || rho0 == 0.0) { report(0, rho0, 1); return KRYST_OK; }     // (x is what it was)
    for (int64_t k = 1; k <= outer->max_iters; ++k) {
        if (n > 0) {
            KR_HIP(enqueue_round32(ctx, r32->d, r, n, 1, rho));
            KR_HIP(hipMemsetAsync(c32->d, 0, sizeof(float) * (size_t)n, ctx->s_main));
        }
        kryst_stats_t ist{0, 0.0, 0};
        Solve32IO io = inner_io; io.stats = &ist;
        const int32_t rc = solve32(r32, c32, a32, io, pcg);
        if (inner_iters && k - 1 < inner_cap) inner_iters[k - 1] = ist.iterations;
        if (rc != KRYST_OK) { report(k - 1, rho, 0); return rc; }            // x untouched
        if (n > 0) {
            hipLaunchKernelGGL(correct_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->s_main, xn, xw, c32->d, rho, n);
            KR_HIP(hipGetLastError());
        }
        double rho_new = 0.0;
        KR_TRY(refine_residual(a, b->d, xn, rn, tmp, &rho_new));
        push(rho_new);
        if (!(rho_new < rho)) { report(k, rho, 0); break; }                  // rejected: x stays as it was
        std::swap(xw, xn); std::swap(r, rn); rho = rho_new;
        const double rel = rho / rho0;                                       // Convergence::check (convergence.rs:18-34)
        const bool conv = (rel <= outer->tol) || (k >= outer->max_iters);
        report(k, rho, conv ? 1 : 0);
        if (conv) break;
    }
    if (n > 0) KR_HIP(hipMemcpyAsync(x->d, xw, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return KRYST_OK;
}

}  // extern "C"
