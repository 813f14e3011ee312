// What the restarted solvers share (gmres.hip, fgmres.hip, pca_gmres.hip): the vector ops and the gate of a restart cycle, the Givens step and the
// back-substitution of the small least-squares problem, the carving of the small device arrays, and the host prologue / epilogue of a solve.
#pragma once
#include "solver_run.h"

namespace kr {

// ---- vector ops
struct DivOp {                       // out = in / s, s a device scalar   (v_0 = r / beta, v_{j+1} = z / h[j+1][j], the s-step inputs w_k / ||w_k||)
    static constexpr int NQ = 0; static constexpr const char* TAG = "Div";
    const double* s; const double* in; double* out;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double d = *s;
        const d2 a = ld2(in, i);
        st2(out, i, a.a / d, a.b / d);
    }
};
template <bool FROM_ZERO>
struct BasisUpdateOp {               // x += sum_j y[j] U[j], j ascending per element, j < *m; FROM_ZERO: the sum alone, x is only written
    static constexpr int NQ = 0; static constexpr const char* TAG = "BasisUpdate";
    const int* m; const double* y; double* const* u; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const int mm = *m;
        d2 xx{0.0, 0.0};
        if constexpr (!FROM_ZERO) xx = ld2(x, i);
        for (int j0 = 0; j0 < mm; j0 += 8) {                 // 8 basis vectors in flight; the sum keeps its ascending order
            d2 uu[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) uu[k] = ld2(u[min(j0 + k, mm - 1)], i);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (j0 + k < mm) { const double yj = y[j0 + k]; xx.a = xx.a + yj * uu[k].a; xx.b = xx.b + yj * uu[k].b; }
        }
        st2(x, i, xx.a, xx.b);
    }
};

// ---- the gate of a restart cycle: a launch is a no-op once the solve has ended or the cycle has been left (cyc_stop == nullptr: done only)
struct CycleGate {
    const int* done; const int* cyc_stop;
    __device__ __forceinline__ bool skip() const { return (done && *done) || (cyc_stop && *cyc_stop); }
};
// launch_spmv / pc_apply_dev_fresh take ONE flag through their `done` hook: this kernel writes done || cyc_stop into that word
static __global__ void cycle_gate_kernel(CycleGate g, int* word) { *word = g.skip() ? 1 : 0; }
static inline int32_t write_cycle_gate(kryst_ctx_t ctx, const CycleGate& g, int* word) {
    hipLaunchKernelGGL(cycle_gate_kernel, dim3(1), dim3(1), 0, ctx->s_main, g, word);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// ---- the least-squares problem of a cycle.  h: Hessenberg matrix, row-major with ld columns; rhs: g (GMRES, PCA-GMRES) / s (FGMRES)
// Each solver states the reference's own test: a Givens step asks tiny(r), a guarded back-substitution asks pivot_ok(h_ii).
struct EpsGuard {                    // |r| < eps -> (1, 0)  /  y_i = 0 unless |h_ii| > eps
    double eps;
    __device__ __forceinline__ bool tiny(double r) const { return fabs(r) < eps; }
    __device__ __forceinline__ bool pivot_ok(double d) const { return fabs(d) > eps; }
};
struct ZeroGuard {                   // r == 0.0 -> (1, 0)   (fgmres.rs:271-275)
    __device__ __forceinline__ bool tiny(double r) const { return r == 0.0; }
};
struct NoGuard {                     // every pivot divides  (fgmres.rs:307-314, the s-step form)
    __device__ __forceinline__ bool pivot_ok(double) const { return true; }
};

// Givens step of column col: the previous rotations, the new one, the right-hand side
template <class Guard>
__device__ inline void givens_column(double* h, int ld, double* cs, double* sn, double* rhs, int col, const Guard& guard) {
    double* hc = h + col;                                                // hc[i * ld] = h[i][col]
    for (int i = 0; i < col; ++i) {
        const double temp = cs[i] * hc[(size_t)i * ld] + sn[i] * hc[(size_t)(i + 1) * ld];
        hc[(size_t)(i + 1) * ld] = -sn[i] * hc[(size_t)i * ld] + cs[i] * hc[(size_t)(i + 1) * ld];
        hc[(size_t)i * ld] = temp;
    }
    const double h_kk = hc[(size_t)col * ld], h_k1k = hc[(size_t)(col + 1) * ld];
    const double r = dsqrt(h_kk * h_kk + h_k1k * h_k1k);
    double c = 1.0, s = 0.0;
    if (!guard.tiny(r)) { c = h_kk / r; s = h_k1k / r; }
    cs[col] = c; sn[col] = s;
    hc[(size_t)col * ld] = c * h_kk + s * h_k1k;
    hc[(size_t)(col + 1) * ld] = 0.0;
    const double temp = c * rhs[col] + s * rhs[col + 1];
    rhs[col + 1] = -s * rhs[col] + c * rhs[col + 1];
    rhs[col] = temp;
}
// y = (leading m x m block of h)^-1 rhs, from the last row up; a pivot the guard refuses leaves y_i = 0.0
template <class Guard>
__device__ inline void back_substitute(const double* h, int ld, const double* rhs, double* y, int m, const Guard& guard) {
    for (int i = m - 1; i >= 0; --i) {
        double sum = rhs[i];
        for (int k = i + 1; k < m; ++k) sum = sum - h[(size_t)i * ld + k] * y[k];
        const double d = h[(size_t)i * ld + i];
        y[i] = guard.pivot_ok(d) ? sum / d : 0.0;
    }
}

// ---- the small device arrays of a solve (H, g, rotations, y, the state struct, the gate word, pointer tables), carved from ONE allocation.
// The solver runs the same sequence of take<T>(count) calls twice: before alloc() they only add up the bytes, after it they hand out the slices.
struct SmallArena {
    char* base = nullptr; size_t off = 0;
    template <class T> T* take(size_t count) {
        static_assert(alignof(T) <= 8, "slices are aligned to 8 bytes");
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (sizeof(T) * count + 7) & ~(size_t)7;
        return p;
    }
    int32_t alloc(Workspace& ws) {                                       // zero filled; freed with the workspace
        KR_HIP(hipMalloc(&base, off));
        ws.vecs.push_back(reinterpret_cast<double*>(base));
        KR_HIP(hipMemsetAsync(base, 0, off, ws.ctx->s_main));
        off = 0;
        return KRYST_OK;
    }
};

// ---- host prologue and epilogue of a restarted solve.  Between check() and begin() the solver makes its own argument checks and sizes its work area.
struct RestartRun {
    kryst_vec_t bv, xv; const SolveIO& io; const kryst_params_t* p;
    kryst_csr_t a; kryst_ctx_t ctx; int64_t n, nt;
    Workspace ws; LogicCtx lc; LiveMonitor mon; const int* done = nullptr;
    RestartRun(kryst_vec_t b, kryst_vec_t x, const SolveIO& io_)       // (the caller has checked io_.a and io_.params)
        : bv(b), xv(x), io(io_), p(io_.params), a(io_.a), ctx(io_.a->ctx), n(io_.a->nrows), nt(ntiles_of(io_.a->nrows)), ws(io_.a->ctx, io_.a->nrows) {}
    // `applied`: the preconditioner the solver will apply -- one it ignores (precond_side = 0, PCA-GMRES Left) is not held against the operator
    int32_t check(kryst_pc_t applied, const char* restart_msg) const {
        SolveIO seen = io; seen.pc = applied;
        KR_TRY(solve_args_check(seen, bv, xv));
        KR_ARG(!io.pc || io.pc->ctx == io.a->ctx, "solve: preconditioner belongs to another context");     // (held against the context even where it is ignored)
        KR_ARG(p->restart >= 1 && p->restart <= 4096, restart_msg);
        return KRYST_OK;
    }
    int32_t begin(int64_t hist_entries, int64_t work_vectors) {
        a->halo_started_for = nullptr;            // (csr.h: an early halo start belongs to the CG / PCG solve that made it)
        KR_HIP(hipSetDevice(ctx->device));
        KR_TRY(ws.init(hist_entries));
        KR_TRY(ws.reserve(work_vectors));
        lc = ws.lctx(p, io.monitor != nullptr);
        mon.io = &io; mon.ws = &ws; mon.first = 1;
        done = &ws.st->done;
        return KRYST_OK;
    }
    int32_t end(const double* xk) {
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        const int32_t status = finish_solve(ws, io);
        if (status == KRYST_OK)                   // on Err the reference never reaches `*x = ...`
            KR_HIP(hipMemcpyAsync(xv->d, xk, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        finish_monitor(mon, ws);
        return status;
    }
};

}  // namespace kr
