// Block CG on multivectors (a labelled extension beside the batched CG / PCG of multi.hip): ONE Krylov space for the K columns, so that every
// column is minimised over the union of all K spaces and K right-hand sides can cost fewer iterations than K solves.  The method is Dubrulle's
// retooled block CG (BCGrQ) with the thin QR done as a Cholesky-QR of a K x K Gram matrix; Jacobi enters through the symmetrically preconditioned
// form.  The iteration, the operation order of every K x K step and the pivot rule are written down in bcg_logic.h.
//
// Per iteration: one SpMM (launch_spmm: the plain or the CSR-DIA kernel) with the Gram of S against T in its epilogue (nq = 2; or a Gram pass over
// S and T behind it, mgram_kernel, under KRYST_BCG_FUSE_GRAM=0), one pass that updates X and
// Q and reduces the Gram matrix of the new Q (bcg_update_kernel), one pass that forms the next Q and S (bcg_direction_kernel), and two folds that
// end in the K x K scalar step (fold_block_kernel).  Every kernel is a plain stream or a fold: nothing waits for another workgroup beyond
// fold2's own hand-off, and nothing goes through the host -- run_ahead polls the progress record as for every other solver.
//
// Bits: an inner product is the tree of DESIGN.md section 4.2 over the products U(i, a) * V(i, b), or U(i, a) * (d_i * V(i, b)) with weights -- the
// lane's two rows in index order from 0.0, the 64-lane butterfly, the four waves, the tile partials in fold2's tree -- per entry of the upper
// triangle; a row product (U M)(i, j) starts from 0.0 and adds U(i, l) * M[l][j] for l ascending over the structurally nonzero l.
#include "multi.h"
#include "bcg_logic.h"
#include "solver_common.h"

namespace kr {

// ---------------------------------------------------------------------------------------------------- the device block of a solve
// The small matrices the scalar step hands to the next pass (K x K, row major with stride K, in the first K * K doubles of each array) and the
// state of the solve.  `done` gates every later launch and is what ends the host's run-ahead loop (through the progress record).
struct BcgDev {
    double c[64], m1[64], gam[64], phi[64], phinv[64];
    double g[36];            // the folded Gram entries, upper triangle row by row
    double res0[8], res[8];
    long long it;            // completed iterations
    long long iterations;    // SolveStats.iterations, the same for every column
    long long hist_len;      // pushes per column
    int done, status;
    int converged[8];
};
struct BcgCtx { BcgDev* dv; double* hist; long long hist_cap; HostProgress* prog; double tol; long long max_iters; double* gram_out; };

// (BcgShape, ld_row / st_row, gram_add, gram_store: multi.h -- the SpMM kernels' Gram epilogue shares them)

// ---------------------------------------------------------------------------------------------------- the passes
// Tile partials of the upper triangle of Gram(U, V [, d]).  Thread t of a tile owns rows 2t and 2t + 1 (2 K contiguous doubles per array) and
// works one row at a time: NG running sums plus 2 K operands per lane.  Bytes per row and column: 16 (8 when U is V), + 8 / K with weights.
template <int K, bool WEIGHTED>
__global__ __launch_bounds__(KR_T, 2) void mgram_kernel(const double* u, const double* v, const double* d, const int* done, int64_t n, int64_t ntiles,
                                                     double* partials, int64_t pstride) {
    if (done && *done) return;
    constexpr int NG = BcgShape<K>::NG;
    __shared__ double lds[BcgShape<K>::RG * (KR_T / 64)];
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t row = q * KR_TILE + (int64_t)threadIdx.x * KR_V;
        double acc[NG];
#pragma unroll
        for (int e = 0; e < NG; ++e) acc[e] = 0.0;
        d2 dd = {0.0, 0.0};
        if constexpr (WEIGHTED) dd = ld2_keep(d, row);
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {                           // one row at a time: NG running sums and one row's operands stay in registers
            double uu[K], vv[K];
            ld_row<K>(u, row + r, uu); ld_row<K>(v, row + r, vv);
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int b = 0; b < K; ++b) vv[b] = (r ? dd.b : dd.a) * vv[b];
            }
            if (row + r < n) gram_add<K>(uu, vv, acc);
        }
        gram_store<K>(acc, lds, partials, pstride, q);
    }
}

// R = B - A X, per element `b - ax` as PcgRun::begin; 16 B read and 8 B written per row and column
template <int K>
__global__ __launch_bounds__(KR_T) void bcg_residual_kernel(const double* b, const double* ax, double* r, int64_t ntiles) {
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t row = q * KR_TILE + (int64_t)threadIdx.x * KR_V;
        double bb[2 * K], aa[2 * K], rr[2 * K];
        ld_rows<K>(b, row, bb); ld_rows<K>(ax, row, aa);
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) rr[e] = bb[e] - aa[e];
        st_rows<K>(r, row, rr);
    }
}

// X(i, j) = X(i, j) + (S M1)(i, j);  Qn(i, j) = Q(i, j) - (T Gamma)(i, j), in place in Q;  tile partials of Gram(Qn, Qn [, d]).
// M1 and Gamma are uniform for the launch: every lane reads them from LDS at the same address (a broadcast).  Bytes per row and column: 32 read,
// 16 written (+ 8 / K with Jacobi).
template <int K, bool JACOBI>
__global__ __launch_bounds__(KR_T, 2) void bcg_update_kernel(const BcgDev* dv, const double* s, const double* tt, double* qv, double* x, const double* d,
                                                          int64_t n, int64_t ntiles, double* partials, int64_t pstride) {
    if (dv->done) return;
    constexpr int NG = BcgShape<K>::NG;
    __shared__ double lds[BcgShape<K>::RG * (KR_T / 64)];
    __shared__ double m1[K * K], gam[K * K];
    if (threadIdx.x < K * K) { m1[threadIdx.x] = dv->m1[threadIdx.x]; gam[threadIdx.x] = dv->gam[threadIdx.x]; }
    __syncthreads();
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t row = q * KR_TILE + (int64_t)threadIdx.x * KR_V;
        double acc[NG];
#pragma unroll
        for (int e = 0; e < NG; ++e) acc[e] = 0.0;
        d2 dd = {0.0, 0.0};
        if constexpr (JACOBI) dd = ld2_keep(d, row);
#pragma unroll
        for (int r = 0; r < 2; ++r) {                           // (unrolled: rolled, the compiler keeps both matrices in registers and spills)
            double ss[K], ts[K], qq[K], xx[K], w[K];
            ld_row<K>(s, row + r, ss); ld_row<K>(tt, row + r, ts); ld_row<K>(qv, row + r, qq); ld_row<K>(x, row + r, xx);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double sx = 0.0, sq = 0.0;
#pragma unroll
                for (int l = 0; l < K; ++l) { sx = sx + ss[l] * m1[l * K + j]; sq = sq + ts[l] * gam[l * K + j]; }
                xx[j] = xx[j] + sx;
                qq[j] = qq[j] - sq;
            }
            st_row<K>(x, row + r, xx); st_row<K>(qv, row + r, qq);
#pragma unroll
            for (int b = 0; b < K; ++b) w[b] = JACOBI ? (r ? dd.b : dd.a) * qq[b] : qq[b];
            if (row + r < n) gram_add<K>(qq, w, acc);
        }
        gram_store<K>(acc, lds, partials, pstride, q);
    }
}

// Q = Qn Phi^-1 (upper: l <= j), in place in Q;  S(i, j) = (d_i * Q(i, j)) + sum_{l = j .. K-1} S(i, l) * Phi[j][l]  (no multiply without Jacobi).
// FIRST (the start of a solve): the Q array holds R, Phi^-1 is C^-1, and S = d Q (or S = Q).  Bytes per row and column: 16 read, 16 written
// (FIRST: 8 read), + 8 / K with Jacobi.
template <int K, bool JACOBI, bool FIRST>
__global__ __launch_bounds__(KR_T, 2) void bcg_direction_kernel(const BcgDev* dv, double* qv, double* s, const double* d, int64_t ntiles) {
    if (dv->done) return;
    __shared__ double phinv[K * K], phi[K * K];
    if (threadIdx.x < K * K) { phinv[threadIdx.x] = dv->phinv[threadIdx.x]; phi[threadIdx.x] = dv->phi[threadIdx.x]; }
    __syncthreads();
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t row = q * KR_TILE + (int64_t)threadIdx.x * KR_V;
        d2 dd = {0.0, 0.0};
        if constexpr (JACOBI) dd = ld2_keep(d, row);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double qn[K], qq[K], ss[K], sn[K];
            ld_row<K>(qv, row + r, qn);
            if constexpr (!FIRST) ld_row<K>(s, row + r, ss);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double a = 0.0;
#pragma unroll
                for (int l = 0; l <= j; ++l) a = a + qn[l] * phinv[l * K + j];
                qq[j] = a;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double dq = JACOBI ? (r ? dd.b : dd.a) * qq[j] : qq[j];
                if constexpr (FIRST) sn[j] = dq;
                else {
                    double a = 0.0;
#pragma unroll
                    for (int l = j; l < K; ++l) a = a + ss[l] * phi[j * K + l];
                    sn[j] = dq + a;
                }
            }
            st_row<K>(qv, row + r, qq); st_row<K>(s, row + r, sn);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the fold and the scalar step
// One launch folds the NG arrays of tile partials (fold2, the tree of every other fold, with its poll budget and error word); thread 0 of the
// workgroup that holds the result then runs the K x K scalar step (bcg_logic.h) in LDS and writes the small matrices of the next pass, the
// histories, the state and `done`.  STEP = BCG_STEP_GRAM only delivers the Gram matrix (kryst_bench_mvec_gram: gram_out holds K * K doubles of result and, behind them,
// NG doubles for the folded entries).
constexpr int BCG_STEP_GRAM = 3;

__device__ __forceinline__ void bcg_finish(const BcgCtx& m, int status) {
    BcgDev* dv = m.dv;
    dv->status = status; dv->done = 1;
    m.prog->iter = dv->it + 1; m.prog->res = dv->res[0]; m.prog->status = status;
    __threadfence_system();
    m.prog->done = 1;
    __threadfence_system();
}

template <int K, int STEP, int E0, int NE>
__global__ __launch_bounds__(KR_F) void fold_block_kernel(const double* partials, int64_t stride, int64_t ntiles, double* chunks, int64_t cstride,
                                                          unsigned int* ticket, unsigned int* err, BcgCtx m) {
    constexpr int NG = BcgShape<K>::NG;
    constexpr int KK = K * K;
    static_assert(E0 >= 0 && NE >= 1 && E0 + NE <= NG, "a group of entries of the upper triangle");
    if (STEP != BCG_STEP_GRAM && m.dv->done) return;          // uniform over the grid: only the workgroup that holds the result ever sets it
    __shared__ double lds[NE * (KR_F / 64)];
    __shared__ double g[KK], cc[KK], o1[KK], o2[KK], w[2 * KK], rr[K];
    double v[NE];
    const int f = fold2<NE>(partials + E0 * stride, stride, ntiles, chunks + E0 * cstride, cstride, ticket, err, v, lds);
    if (!f) return;
    if (threadIdx.x != 0) return;
    if (f == 2) {                                             // the hand-off gave up: no value to act on
        if constexpr (STEP == BCG_STEP_GRAM) { for (int e = 0; e < KK; ++e) m.gram_out[e] = __longlong_as_double(0x7FF8000000000000ll); }
        else bcg_finish(m, KRYST_ERR_HIP);
        return;
    }
    // the folded entries of this group go to the device block; the launch that folds the last group reads them all back (stream order)
    double* gdev = STEP == BCG_STEP_GRAM ? m.gram_out + KK : m.dv->g;
#pragma unroll
    for (int e = 0; e < NE; ++e) gdev[E0 + e] = v[e];
    if constexpr (E0 + NE < NG) return;
    __threadfence();
    {
        int e = 0;
        for (int a = 0; a < K; ++a)
            for (int b = a; b < K; ++b) { const double x = __hip_atomic_load(&gdev[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); g[a * K + b] = x; g[b * K + a] = x; ++e; }
    }
    if constexpr (STEP == BCG_STEP_GRAM) {
        for (int e = 0; e < KK; ++e) m.gram_out[e] = g[e];
        return;
    } else {
        BcgDev* dv = m.dv;
        if constexpr (STEP != BCG_STEP_INIT) {
            for (int e = 0; e < KK; ++e) cc[e] = dv->c[e];
        }
        int k = K;
        asm volatile("" : "+s"(k));                               // (keeps the K x K loops rolled: unrolled for K = 8 they spill to scratch)
        const int32_t rc = bcg_step(STEP, k, g, cc, o1, o2, rr, w);
        if (rc != KRYST_OK) {                                     // a breakdown: the same code for every column, iterations = it
            dv->iterations = STEP == BCG_STEP_INIT ? 0 : dv->it + 1;
            for (int j = 0; j < K; ++j) dv->converged[j] = 0;
            bcg_finish(m, rc);
            return;
        }
        if constexpr (STEP == BCG_STEP_INIT) {
            for (int e = 0; e < KK; ++e) { dv->c[e] = cc[e]; dv->phinv[e] = o1[e]; }
            for (int j = 0; j < K; ++j) {
                dv->res0[j] = rr[j]; dv->res[j] = rr[j]; dv->converged[j] = 0;
                if (0 < m.hist_cap) m.hist[(long long)j * m.hist_cap] = rr[j];
            }
            dv->hist_len = 1; dv->it = 0; dv->iterations = 0;
            if (m.max_iters <= 0) bcg_finish(m, KRYST_OK);
        } else if constexpr (STEP == BCG_STEP_ALPHA) {
            for (int e = 0; e < KK; ++e) { dv->gam[e] = o1[e]; dv->m1[e] = o2[e]; }
        } else {
            for (int e = 0; e < KK; ++e) { dv->c[e] = cc[e]; dv->phi[e] = o1[e]; dv->phinv[e] = o2[e]; }
            const long long it = dv->it + 1, at = dv->hist_len;
            bool all = true;
            for (int j = 0; j < K; ++j) {
                dv->res[j] = rr[j];
                if (at < m.hist_cap) m.hist[(long long)j * m.hist_cap + at] = rr[j];
                const bool conv = (rr[j] / dv->res0[j] <= m.tol);             // Convergence::check, per column
                all = all && conv;
                dv->converged[j] = (conv || it >= m.max_iters) ? 1 : 0;
            }
            dv->hist_len = at + 1; dv->it = it; dv->iterations = it;
            if (all || it >= m.max_iters) bcg_finish(m, KRYST_OK);
        }
    }
}

// fold2 keeps its NE running values in registers and a workgroup of 1024 threads has 128 VGPRs per lane: the 36 entries of K = 8 are folded in
// groups of at most BCG_FOLD_GROUP, one launch per group (K = 2 and 4: one launch)
constexpr int BCG_FOLD_GROUP = 12;
template <int K, int STEP, int E0 = 0>
static int32_t launch_fold_block(kryst_ctx_t ctx, const double* partials, int64_t pstride, int64_t nt, double* chunks, int64_t cstride, const BcgCtx& bc) {
    constexpr int NG = BcgShape<K>::NG;
    constexpr int NE = NG - E0 < BCG_FOLD_GROUP ? NG - E0 : BCG_FOLD_GROUP;
    hipLaunchKernelGGL((fold_block_kernel<K, STEP, E0, NE>), dim3((unsigned)nchunks_of(nt)), dim3(KR_F), 0, ctx->s_main,
                       partials, pstride, nt, chunks, cstride, fold_ticket(ctx), fold_err(ctx), bc);
    KR_HIP(hipGetLastError());
    if constexpr (E0 + NE < NG) return launch_fold_block<K, STEP, E0 + NE>(ctx, partials, pstride, nt, chunks, cstride, bc);
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- the solve
constexpr int BCG_FUSE_GRAM_DEFAULT = 1;     // the epilogue arm: 1.09 - 1.12x per iteration over SpMM + mgram_kernel at 256^3
constexpr size_t BCG_SCAL_AT = 3200;            // doubles: the slice of the context's scalar arena the batched solvers use too (one solve at a time)
static_assert(BCG_SCAL_AT * sizeof(double) + sizeof(BcgDev) <= 4096 * sizeof(double), "the scalar arena holds 4096 doubles (ctx.cpp)");

// the context's reduction scratch holds KR_MAXQ arrays; NG <= 36 arrays of this solve's strides need it sized for more tiles (as the batched PCG
// sizes it for 16)
static int32_t bcg_scratch(kryst_ctx_t ctx, int ng, int64_t nt, double** partials, int64_t* pstride, double** chunks, int64_t* cstride) {
    KR_TRY(ensure_partials(ctx, 5 * nt + 512));
    *pstride = nt + 64; *cstride = nchunks_of(nt);
    *partials = ctx->d_partials; *chunks = ctx->d_chunks;
    if (ng * *pstride > KR_MAXQ * ctx->partials_cap || ng * *cstride > KR_MAXQ * ctx->chunks_cap) { set_error("block CG: reduction scratch does not fit"); return KRYST_ERR_HIP; }
    return KRYST_OK;
}
static unsigned bcg_grid(kryst_ctx_t ctx, int64_t nt) {
    return (unsigned)std::min<int64_t>(nt, (int64_t)ctx->num_cu * std::max(1, env_int("KRYST_EW_BLOCKS_PER_CU", 3)));
}

template <int K>
struct BlockRun {
    static constexpr int NG = BcgShape<K>::NG;
    static constexpr int64_t HIST_MAX_COL = Workspace::HIST_MAX / 8;
    MultiIO io; kryst_params_t prm;
    kryst_csr_t a; kryst_ctx_t ctx; int64_t n, nt;
    Workspace ws;
    bool jac = false; const double* inv_diag = nullptr;
    double *xw = nullptr, *q = nullptr, *s = nullptr, *t = nullptr;
    double* partials = nullptr; int64_t pstride = 0; double* chunks = nullptr; int64_t cstride = 0;
    BcgDev* dv = nullptr; int64_t hist_col = 0;
    BcgCtx bc{};

    static int64_t ws_len(int64_t n) { return mvec_rows(n) * K - KR_TILE; }       // a Workspace vector of this length is exactly one multivector
    explicit BlockRun(const MultiIO& io_)
        : io(io_), prm(*io_.params), a(io_.a), ctx(io_.a->ctx), n(io_.a->nrows), nt(ntiles_of(io_.a->nrows)), ws(io_.a->ctx, ws_len(io_.a->nrows)) {}

    template <int STEP>
    int32_t fold_then() {
        KR_TRY((launch_fold_block<K, STEP>(ctx, partials, pstride, nt, chunks, cstride, bc)));
        phase_mark(ctx, KR_PH_REDUCE);
        return KRYST_OK;
    }
    template <bool FIRST>
    int32_t direction() {
        if (nt <= 0) return KRYST_OK;
        if (jac) hipLaunchKernelGGL((bcg_direction_kernel<K, true, FIRST>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, dv, q, s, inv_diag, nt);
        else hipLaunchKernelGGL((bcg_direction_kernel<K, false, FIRST>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, dv, q, s, inv_diag, nt);
        KR_HIP(hipGetLastError());
        phase_mark(ctx, KR_PH_BLAS1_DIRECTION);
        return KRYST_OK;
    }

    int32_t begin() {
        KR_HIP(hipSetDevice(ctx->device));
        hist_col = std::max<int64_t>(2, std::min<int64_t>(prm.max_iters + 2, HIST_MAX_COL));
        KR_TRY(ws.init(hist_col * K));
        jac = io.pc && io.pc->kind == KR_PC_JACOBI;
        inv_diag = jac ? pc_jacobi_inv_diag(io.pc) : nullptr;
        KR_TRY(ws.reserve(4));                                             // xw, q, s, t
        if (ws.vec_bytes() < sizeof(double) * (size_t)(mvec_rows(n) * K)) { set_error("block CG: a work vector is smaller than a multivector"); return KRYST_ERR_HIP; }
        dv = reinterpret_cast<BcgDev*>(ctx->d_scal + BCG_SCAL_AT);
        KR_HIP(hipMemsetAsync(dv, 0, sizeof(BcgDev), ctx->s_main));
        KR_TRY(ws.vec(&xw)); KR_TRY(ws.vec(&q)); KR_TRY(ws.vec(&s)); KR_TRY(ws.vec(&t));
        KR_TRY(bcg_scratch(ctx, NG, nt, &partials, &pstride, &chunks, &cstride));
        bc = BcgCtx{dv, ws.d_hist, (long long)hist_col, ctx->d_prog, prm.tol, (long long)prm.max_iters, nullptr};
        KR_HIP(hipMemcpyAsync(xw, io.x->d, sizeof(double) * (size_t)(nt * KR_TILE * K), hipMemcpyDeviceToDevice, ctx->s_main));
        KR_TRY(launch_spmm(a, K, xw, t, 0, nullptr, nullptr, 0, nullptr));
        if (nt > 0) {
            hipLaunchKernelGGL((bcg_residual_kernel<K>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, io.b->d, t, q, nt);
            KR_HIP(hipGetLastError());
            if (jac) hipLaunchKernelGGL((mgram_kernel<K, true>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, q, q, inv_diag, nullptr, n, nt, partials, pstride);
            else hipLaunchKernelGGL((mgram_kernel<K, false>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, q, q, inv_diag, nullptr, n, nt, partials, pstride);
            KR_HIP(hipGetLastError());
            phase_mark(ctx, KR_PH_BLAS1);
        }
        KR_TRY(fold_then<BCG_STEP_INIT>());
        return direction<true>();
    }

    int32_t iterate(int64_t) {
        // Gram(S, T): in the SpMM's epilogue (nq = 2: the owner lane holds its T rows and loads its own S rows), or by mgram_kernel behind a plain SpMM
        // (KRYST_BCG_FUSE_GRAM = 1 | 0).  The bits are the same; the default is what the in-process A/B of DESIGN.md section 4.14.2 chose.
        if (env_int("KRYST_BCG_FUSE_GRAM", BCG_FUSE_GRAM_DEFAULT) != 0) {
            KR_TRY(launch_spmm(a, K, s, t, 2, nullptr, partials, pstride, &dv->done));
        } else {
            KR_TRY(launch_spmm(a, K, s, t, 0, nullptr, nullptr, 0, &dv->done));
            if (nt > 0) {
                hipLaunchKernelGGL((mgram_kernel<K, false>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, s, t, nullptr, &dv->done, n, nt, partials, pstride);
                KR_HIP(hipGetLastError());
                phase_mark(ctx, KR_PH_BLAS1);
            }
        }
        KR_TRY(fold_then<BCG_STEP_ALPHA>());
        if (nt > 0) {
            if (jac) hipLaunchKernelGGL((bcg_update_kernel<K, true>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, dv, s, t, q, xw, inv_diag, n, nt, partials, pstride);
            else hipLaunchKernelGGL((bcg_update_kernel<K, false>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, dv, s, t, q, xw, inv_diag, n, nt, partials, pstride);
            KR_HIP(hipGetLastError());
            phase_mark(ctx, KR_PH_BLAS1_RESIDUAL);
        }
        KR_TRY(fold_then<BCG_STEP_BETA>());
        return direction<false>();
    }

    int32_t end() {
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        BcgDev h;
        KR_HIP(hipMemcpyAsync(&h, dv, sizeof(BcgDev), hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        if (h.status == KRYST_ERR_HIP) (void)fold_gave_up(ctx);          // explains, and switches the context to the ticket hand-off
        const int32_t code = (io.pc && pc_health(io.pc) != KRYST_OK) ? KRYST_SOLVE_ERROR : h.status;
        for (int j = 0; j < K; ++j) {
            if (io.stats) { io.stats[j].iterations = h.iterations; io.stats[j].final_residual = h.res[j]; io.stats[j].converged = h.converged[j]; }
            if (io.status) io.status[j] = code;
            if (io.hist_len) io.hist_len[j] = h.hist_len;
            if (io.hist) {
                const int64_t keep = std::min<int64_t>(std::min<int64_t>(h.hist_len, hist_col), io.hist_cap);
                for (int64_t k = 0; k < keep; ++k) io.hist[(size_t)j * io.hist_cap + k] = ws.h_hist[(size_t)j * hist_col + k];
            }
        }
        // X is iterated in the work copy and written back only when the solve ended with KRYST_OK: rows < n, never X's padding
        if (code == KRYST_OK && n > 0) KR_HIP(hipMemcpyAsync(io.x->d, xw, sizeof(double) * (size_t)(n * K), hipMemcpyDeviceToDevice, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        return KRYST_OK;
    }

    int32_t solve() {
        const EnvFreeze knobs;
        KR_TRY(begin());
        KR_TRY(run_ahead(ctx, &prm, [&](int64_t i) -> int32_t { return iterate(i); }));
        return end();
    }
};

static int32_t block_solve(const MultiIO& io) {
    KR_TRY(multi_args_check(io, true));
    switch (io.b->k) {
        case 2: { BlockRun<2> run(io); return run.solve(); }
        case 4: { BlockRun<4> run(io); return run.solve(); }
        case 8: { BlockRun<8> run(io); return run.solve(); }
        default: set_error("block CG: k = %d (2, 4 or 8)", (int)io.b->k); return KRYST_ERR_ARG;
    }
}

template <int K>
static int32_t bench_gram(kryst_mvec_t u, kryst_mvec_t v, const double* d, double* out) {
    constexpr int NG = BcgShape<K>::NG;
    kryst_ctx_t ctx = u->ctx;
    const int64_t n = u->n, nt = ntiles_of(n);
    double *partials, *chunks; int64_t pstride, cstride;
    KR_TRY(bcg_scratch(ctx, NG, nt, &partials, &pstride, &chunks, &cstride));
    double* slot = ctx->d_scal + BCG_SCAL_AT;
    if (nt > 0) {
        if (d) hipLaunchKernelGGL((mgram_kernel<K, true>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, u->d, v->d, d, nullptr, n, nt, partials, pstride);
        else hipLaunchKernelGGL((mgram_kernel<K, false>), dim3(bcg_grid(ctx, nt)), dim3(KR_T), 0, ctx->s_main, u->d, v->d, d, nullptr, n, nt, partials, pstride);
        KR_HIP(hipGetLastError());
    }
    const BcgCtx bc{nullptr, nullptr, 0, nullptr, 0.0, 0, slot};
    KR_TRY((launch_fold_block<K, BCG_STEP_GRAM>(ctx, partials, pstride, nt, chunks, cstride, bc)));
    KR_HIP(hipMemcpyAsync(ctx->h_pinned, slot, sizeof(double) * K * K, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    for (int e = 0; e < K * K; ++e) out[e] = ctx->h_pinned[e];
    return fold_gave_up(ctx) ? KRYST_ERR_HIP : KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

#define KRYST_MULTI_TAIL kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats, int32_t* status, \
        double* hist, int64_t hist_cap, int64_t* hist_len

int32_t kryst_bcg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, KRYST_MULTI_TAIL) {
    return block_solve(MultiIO{b, x, a, pc, params, stats, status, hist, hist_cap, hist_len});
}

int32_t kryst_bcg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, KRYST_MULTI_TAIL) {
    KR_ARG(a && b && x && params, "block CG: null argument");
    KR_ARG(mvec_width_ok(k), "block CG: k must be 2, 4 or 8");
    KR_ARG(n == a->nrows && ld >= n, "block CG: n != operator size or ld < n");
    kryst_mvec_t bv = nullptr, xv = nullptr;
    int32_t rc = kryst_mvec_create(a->ctx, n, k, &bv);
    if (rc == KRYST_OK) rc = kryst_mvec_create(a->ctx, n, k, &xv);
    if (rc == KRYST_OK) rc = kryst_mvec_upload(bv, b, ld);
    if (rc == KRYST_OK) rc = kryst_mvec_upload(xv, x, ld);
    if (rc == KRYST_OK) rc = block_solve(MultiIO{bv, xv, a, pc, params, stats, status, hist, hist_cap, hist_len});
    if (rc == KRYST_OK) rc = kryst_mvec_download(xv, x, ld);            // (after a breakdown xv still holds the initial guesses)
    (void)kryst_mvec_destroy(bv); (void)kryst_mvec_destroy(xv);
    return rc;
}

int32_t kryst_host_bcg_step(int32_t step, int32_t k, const double* g, double* c, double* out1, double* out2, double* res) {
    KR_ARG(step == BCG_STEP_INIT || step == BCG_STEP_ALPHA || step == BCG_STEP_BETA, "host_bcg_step: step must be 0, 1 or 2");
    KR_ARG(mvec_width_ok(k), "host_bcg_step: k must be 2, 4 or 8");
    KR_ARG(g && c && out1 && out2 && res, "host_bcg_step: null argument");
    double w[2 * 64];
    return bcg_step(step, k, g, c, out1, out2, res, w);
}

int32_t kryst_bench_mvec_gram(kryst_mvec_t u, kryst_mvec_t v, kryst_vec_t inv_diag, double* out_kk) {
    KR_TRY(mvec_check(u)); KR_TRY(mvec_check(v));
    KR_ARG(out_kk, "mvec_gram: null output");
    KR_ARG(u->ctx == v->ctx && u->n == v->n && u->k == v->k, "mvec_gram: U and V differ in context or shape");
    KR_ARG(!inv_diag || (inv_diag->d && inv_diag->ctx == u->ctx && inv_diag->n == u->n), "mvec_gram: weights of another context or length");
    kryst_ctx_t ctx = u->ctx;
    if (ctx->active_ws != nullptr) { set_error("context busy: a solve or stepping session is open on this context"); return KRYST_ERR_BUSY; }
    KR_HIP(hipSetDevice(ctx->device));
    const double* d = inv_diag ? inv_diag->d : nullptr;
    switch (u->k) {
        case 2: return bench_gram<2>(u, v, d, out_kk);
        case 4: return bench_gram<4>(u, v, d, out_kk);
        case 8: return bench_gram<8>(u, v, d, out_kk);
        default: set_error("mvec_gram: k = %d (2, 4 or 8)", (int)u->k); return KRYST_ERR_ARG;
    }
}

}  // extern "C"
