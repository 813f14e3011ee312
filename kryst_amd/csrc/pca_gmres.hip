// PcaGmresSolver (src/solver/pca_gmres.rs:99-312) on the device, in two forms.
//
// 1. As written (default features, no `mpi`): x starts from zero whatever the caller passes (:107), the j+1 coefficients
//    h[i][j] = (v_i, A v_j) are recorded but never subtracted (the subtraction lives under cfg(feature = "mpi"), :181-204),
//    v_{j+1} = w * (1 / ||w||) (:224-228), Right applies pc after A (:152,164) while r0 and the x update stay unpreconditioned,
//    Left and None never call pc, Givens with the f64 epsilon guard (:236-262), one Convergence::check per block (:266-272),
//    m_eff = j so the stopping block's column is left out of the update (:277), back-substitution that leaves y = 0 where
//    |h_ii| <= epsilon (:283), converged = beta <= tol * res0 after the true residual (:304).  Any block_size >= 2 with restart >= 2
//    indexes v_basis past its end at the first block (:145,151,163): only blocks of one vector run.  Deviations (labelled):
//    block_size >= 2 with restart >= 2 and at least one cycle, block_size = 0 or restart = 0 return KRYST_ERR_ARG with x untouched
//    where the reference panics or loops forever.
//
// 2. Labelled extension (not in the reference): s-step GMRES(m), right preconditioned (Hoemmen 2010, ch. 3; Yamazaki et al.,
//    IPDPS 2014).  Per block of s columns from the last basis vector q: w_1 = A M^-1 q, w_{i+1} = A M^-1 (w_i / ||w_i||) (scaled
//    monomial basis), BCGS2 against the basis (C = Q^T W, W -= Q C, twice, coefficients summed), CholQR2 among the block (G = W^T W,
//    R1 = chol(G), W <- W R1^-1, again, R = R2 R1).  Column k survives when its first CholQR pivot is finite and > 1e-12 ||w_k||^2
//    (before BCGS2); a failing column 0 is a happy breakdown (kept with a zero subdiagonal, the cycle ends), a later one truncates the
//    block.  The new Hessenberg columns are ([C; R] - [H_prev; 0] T_top) T_bot^-1, solved column by column, then the Givens rotations
//    of part 1 and a test per column on |g_{c+1}| <= tol ||r0||.  Cycle end: x += M^-1 (Q y), the true residual decides `converged`.
//
// Kernels (both forms): pg_pass_kernel walks the vectors in the library's tiles and does, in ONE pass, an optional update of the
// block columns (W -= Q C with ascending i, or the row-wise triangular solve W R^-1) and optional inner products in the library's
// tile order (Q^T W, or the upper triangle of W^T W), one partial per tile and quantity; pg_fold*_kernel fold them as fold2 does
// (common.h), so every coefficient has the bits of oracle.dot(..., Reduce.tiled(*reduce_spec())).  Fused: the second BCGS dot pass
// into the first update (pass B), the first Gram matrix into the second update (pass C), the second Gram matrix into the first
// triangular solve (pass D); pass E writes the new basis vectors.  The scalar work runs in one-thread logic kernels.
#include "restart_common.h"
#include "solvers.h"

namespace kr {

constexpr int PG_SMAX = 16;          // largest s of the s-step form (and of the block kernels)
constexpr int PG_NW = KR_T / 64;

struct PgState {                     // device
    long long iteration;
    int cyc_stop;                    // leave the cycle
    int m;                           // columns that enter the update of this cycle
    int j;                           // s-step: basis vectors in the cycle minus one (the index of the last one)
    int keep;                        // s-step: columns kept by the first CholQR pass of the current block
    double beta, res0, inv;
};

struct PgPtrs {
    PgState* gs;
    double *h, *hu, *g, *cs, *sn, *y;          // rotated / unrotated Hessenberg (row-major, R columns), g, rotations, y
    double *red;                                // folded block inner products
    double *c1, *c2, *g1, *g2;                  // s-step: BCGS coefficients (i*S + k), Gram matrices (packed upper triangle)
    double *nu2, *nu, *r1, *r2;                 // s-step: ||w_k||^2, ||w_k||, R1, R2 (row-major S x S)
    int R, S;
};

// ---- per-tile sums of up to PG_SMAX quantities [lo, cnt): butterfly per quantity, then the waves in order (block_reduce's tree)
__device__ __forceinline__ void pg_block_sum(double (&v)[PG_SMAX], int lo, int cnt, double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < PG_SMAX; ++q)
        if (q >= lo && q < cnt) {
            v[q] = wave_butterfly(v[q]);
            if (lane == 0) lds[q * PG_NW + wave] = v[q];
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PG_SMAX; ++q)
        if (q >= lo && q < cnt) {
            double s = lds[q * PG_NW];
#pragma unroll
            for (int w = 1; w < PG_NW; ++w) s = s + lds[q * PG_NW + w];
            v[q] = s;
        }
    __syncthreads();
}

struct PgPass {
    const double* const* q; int nb;             // basis vectors Q_0 .. Q_{nb-1}
    const double* qx;                           // dots 1: one more vector after them (quantities nb*s ..), or nullptr
    double* const* w; int s; const int* sdev;   // block columns W_0 .. W_{s-1}; sdev: min(s, *sdev) columns (the kept ones)
    const double* coef; int cs;                 // update 1: W_k -= sum_i coef[i*cs + k] Q_i, i ascending
    const double* rm; int rs;                   // update 2: X = W R^-1 row by row, R upper triangular at rm[r*rs + c]
    double* const* out;                         // update 2: destination of X (may be w)
    int update;                                 // 0 none, 1 W -= Q C, 2 W R^-1
    int dots;                                   // 0 none, 1 Q^T W (quantity i*s + k), 2 W^T W upper triangle (row-major packed)
    int64_t n; double* part; int64_t pstride;
};

__global__ __launch_bounds__(KR_T) void pg_pass_kernel(PgPass p, CycleGate gate) {
    if (gate.skip()) return;
    const int s = p.sdev ? min(*p.sdev, p.s) : p.s;
    if (s <= 0) return;
    __shared__ double lds[PG_SMAX * PG_NW];
    const int64_t ntiles = (p.n + KR_TILE - 1) / KR_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t i = t * KR_TILE + (int64_t)threadIdx.x * KR_V;
        const bool in0 = i < p.n, in1 = i + 1 < p.n;
        double wa[PG_SMAX], wb[PG_SMAX];
#pragma unroll
        for (int k = 0; k < PG_SMAX; ++k) {
            wa[k] = 0.0; wb[k] = 0.0;
            if (k < s) { const d2 v = ld2_keep(p.w[k], i); wa[k] = v.a; wb[k] = v.b; }
        }
        if (p.update == 1) {
            for (int r = 0; r < p.nb; ++r) {
                const d2 qq = ld2_keep(p.q[r], i);
                const double* cr = p.coef + (size_t)r * p.cs;
#pragma unroll
                for (int k = 0; k < PG_SMAX; ++k)
                    if (k < s) { const double c = cr[k]; wa[k] = wa[k] - c * qq.a; wb[k] = wb[k] - c * qq.b; }
            }
#pragma unroll
            for (int k = 0; k < PG_SMAX; ++k)
                if (k < s) st2_keep(p.w[k], i, wa[k], wb[k]);
        } else if (p.update == 2) {
#pragma unroll
            for (int c = 0; c < PG_SMAX; ++c)
                if (c < s) {
                    double xa = wa[c], xb = wb[c];
#pragma unroll
                    for (int r = 0; r < c; ++r) { const double rv = p.rm[r * p.rs + c]; xa = xa - wa[r] * rv; xb = xb - wb[r] * rv; }
                    const double d = p.rm[c * p.rs + c];
                    xa = xa / d; xb = xb / d;
                    wa[c] = xa; wb[c] = xb;
                    st2_keep(p.out[c], i, xa, xb);
                }
        }
        if (p.dots == 1) {
            const int nr = p.nb + (p.qx ? 1 : 0);
            for (int r = 0; r < nr; ++r) {
                const d2 qq = ld2_keep(r < p.nb ? p.q[r] : p.qx, i);
                double acc[PG_SMAX];
#pragma unroll
                for (int k = 0; k < PG_SMAX; ++k) {
                    acc[k] = 0.0;
                    if (in0) acc[k] = acc[k] + qq.a * wa[k];
                    if (in1) acc[k] = acc[k] + qq.b * wb[k];
                }
                pg_block_sum(acc, 0, s, lds);
                if (threadIdx.x == 0)
                    for (int k = 0; k < s; ++k) p.part[(int64_t)(r * s + k) * p.pstride + t] = acc[k];
            }
        } else if (p.dots == 2) {
            int base = 0;
#pragma unroll
            for (int a = 0; a < PG_SMAX; ++a)
                if (a < s) {
                    double acc[PG_SMAX];
#pragma unroll
                    for (int b = 0; b < PG_SMAX; ++b) {
                        acc[b] = 0.0;
                        if (in0) acc[b] = acc[b] + wa[a] * wa[b];
                        if (in1) acc[b] = acc[b] + wb[a] * wb[b];
                    }
                    pg_block_sum(acc, a, s, lds);
                    if (threadIdx.x == 0)
                        for (int b = a; b < s; ++b) p.part[(int64_t)(base + b - a) * p.pstride + t] = acc[b];
                    base += s - a;
                }
        }
    }
}

// fold2's tree for many quantities: stage 1 per chunk of KR_F tile partials (blockIdx.y = quantity), stage 2 over the chunks
__global__ __launch_bounds__(KR_F) void pg_fold1_kernel(const double* part, int64_t pstride, int64_t ntiles, int64_t nchunks,
                                                        double* chunks, double* out, CycleGate gate) {
    if (gate.skip()) return;
    __shared__ double lds[KR_F / 64];
    const int64_t qn = blockIdx.y, c = blockIdx.x;
    const int64_t i = c * KR_F + threadIdx.x;
    double v[1] = {(i < ntiles) ? part[qn * pstride + i] : 0.0};
    block_reduce<1, KR_F / 64>(v, lds);
    if (threadIdx.x == 0) {
        if (nchunks == 1) out[qn] = v[0];
        else chunks[qn * nchunks + c] = v[0];
    }
}
__global__ __launch_bounds__(KR_F) void pg_fold2_kernel(const double* chunks, int64_t nchunks, double* out, CycleGate gate) {
    if (gate.skip()) return;
    __shared__ double lds[KR_F / 64];
    const int64_t qn = blockIdx.x;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < nchunks; j += KR_F) acc = acc + chunks[qn * nchunks + j];
    double v[1] = {acc};
    block_reduce<1, KR_F / 64>(v, lds);
    if (threadIdx.x == 0) out[qn] = v[0];
}

struct PgBuf {                       // tile partials and chunk values of up to nq quantities
    double* part = nullptr; double* chunks = nullptr; int64_t ntiles = 0, nchunks = 0; int nq = 0;
};

// one block pass and, when it has inner products, their fold into out[0..nq)
static int32_t pg_pass(kryst_ctx_t ctx, PgPass p, int nq, double* out, const PgBuf& buf, CycleGate gate) {
    p.part = buf.part; p.pstride = buf.ntiles;
    if (p.dots && nq > buf.nq) { set_error("pca_gmres: %d block inner products exceed the work area", nq); return KRYST_ERR_ARG; }
    static const int bpc = [] { const char* e = getenv("KRYST_PG_BLOCKS_PER_CU"); return e ? std::max(1, atoi(e)) : 4; }();
    const int64_t grid = std::min<int64_t>(buf.ntiles, (int64_t)ctx->num_cu * bpc);
    hipLaunchKernelGGL(pg_pass_kernel, dim3((unsigned)grid), dim3(KR_T), 0, ctx->s_main, p, gate);
    KR_HIP(hipGetLastError());
    if (p.dots && nq > 0) {
        hipLaunchKernelGGL(pg_fold1_kernel, dim3((unsigned)buf.nchunks, (unsigned)nq), dim3(KR_F), 0, ctx->s_main,
                           buf.part, buf.ntiles, buf.ntiles, buf.nchunks, buf.chunks, out, gate);
        KR_HIP(hipGetLastError());
        if (buf.nchunks > 1) {
            hipLaunchKernelGGL(pg_fold2_kernel, dim3((unsigned)nq), dim3(KR_F), 0, ctx->s_main, buf.chunks, buf.nchunks, out, gate);
            KR_HIP(hipGetLastError());
        }
    }
    phase_mark(ctx, KR_PH_BLAS1);
    return KRYST_OK;
}

// ---- vector ops
struct PgMulOp {                     // out = in * s    (:227-228 `*vki *= inv`)
    static constexpr int NQ = 0; static constexpr const char* TAG = "PgMul";
    const double* s; const double* in; double* out;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double d = *s;
        const d2 a = ld2(in, i);
        st2(out, i, a.a * d, a.b * d);
    }
};
struct PgAddOp {                     // x = x + z
    static constexpr int NQ = 0; static constexpr const char* TAG = "PgAdd";
    const double* z; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 a = ld2(x, i), b = ld2(z, i);
        st2(x, i, a.a + b.a, a.b + b.b);
    }
};

// ---- logic
#define HH(i, k) P.h[(size_t)(i) * P.R + (k)]
#define HU(i, k) P.hu[(size_t)(i) * P.R + (k)]

struct PgInitLogic {                 // :113-116 (as written) / r0 = b - A x0 (s-step) ; red0 = (r0, r0)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; long long n_outer; int textbook;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double beta = dsqrt(red[0]);
        P.gs->beta = beta; P.gs->res0 = beta; st->res0 = beta;
        st->iterations = 0; st->final_residual = beta; st->converged = 0; st->iter = 0;
        P.gs->iteration = 0;
        if (textbook && beta == 0.0) { st->converged = 1; c.finish(KRYST_OK); return; }   // x0 solves the system
        if (n_outer <= 0) c.finish(KRYST_OK);                                            // :120-121, :310
    }
};
struct PgCycleLogic {                // :123-133
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P;
    __device__ void run(const double*) const {
        for (size_t k = 0; k < (size_t)(P.R + 1) * P.R; ++k) { P.h[k] = 0.0; P.hu[k] = 0.0; }
        for (int k = 0; k <= P.R; ++k) P.g[k] = 0.0;
        P.g[0] = P.gs->beta;
        for (int k = 0; k < P.R; ++k) { P.cs[k] = 0.0; P.sn[k] = 0.0; P.y[k] = 0.0; }
        P.gs->m = P.R; P.gs->cyc_stop = 0; P.gs->j = 0; P.gs->keep = 0;
    }
};
struct PgStepLogic {                 // as written, block of one vector at column j: red = (v_0, w) .. (v_j, w), (w, w)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; int j;
    __device__ void run(const double*) const {
        PgState* gs = P.gs;
        if (gs->cyc_stop) return;
        const double* red = P.red;
        for (int i = 0; i <= j; ++i) HH(i, j) = red[i];                 // :208-212
        const double norm_vk = dsqrt(red[j + 1]);                      // :225-226
        HH(j + 1, j) = norm_vk;
        gs->inv = 1.0 / norm_vk;                                       // :227
        givens_column(P.h, P.R, P.cs, P.sn, P.g, j, EpsGuard{DBL_EPSILON});   // :238-262
        const double gnorm = fabs(P.g[j + 1]);                         // :266
        gs->iteration = gs->iteration + 1;                             // :267
        c.push(gnorm);                                                 // history (an addition): the value handed to the check
        st_iter_check(gnorm, gs->iteration);
        if (c.st->converged) { gs->cyc_stop = 1; gs->m = j; }          // :270-271, :277 m_eff = j
    }
    __device__ void st_iter_check(double gnorm, long long it) const { c.check(gnorm, P.gs->res0, it); }
};
struct PgBackLogic {                 // as written :278-286 (epsilon guard, y = 0 where it fails); s-step: plain back-substitution
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; int textbook;
    __device__ void run(const double*) const {
        for (int i = 0; i < P.R; ++i) P.y[i] = 0.0;
        if (textbook) back_substitute(P.h, P.R, P.g, P.y, P.gs->m, NoGuard{});
        else back_substitute(P.h, P.R, P.g, P.y, P.gs->m, EpsGuard{DBL_EPSILON});
    }
};
struct PgCycleEndLogic {             // :298-307 ; red0 = (r0, r0) of the true residual
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double beta = dsqrt(red[0]);
        P.gs->beta = beta;
        st->final_residual = beta;                                     // :303
        st->converged = (beta <= c.tol * P.gs->res0) ? 1 : 0;          // :304
        st->iter = P.gs->iteration;
        if (st->converged || P.gs->iteration >= c.max_iters) c.finish(KRYST_OK);   // :305-307
    }
};

// ---- s-step logic
__device__ __forceinline__ int pg_upper(int a, int b, int s) { return a * s - a * (a - 1) / 2 + (b - a); }   // packed (a <= b)

struct PgNuLogic {                   // ||w_k||^2 and ||w_k|| of the block column just generated
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; int k;
    __device__ void run(const double* red) const { P.nu2[k] = red[0]; P.nu[k] = dsqrt(red[0]); }
};
struct PgChol1Logic {                // R1 = chol(G1) column by column; the first column whose pivot fails ends the kept set
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; int s;
    __device__ void run(const double*) const {
        const int S = P.S;
        for (int k = 0; k < S * S; ++k) P.r1[k] = 0.0;
        int keep = s;
        for (int cc = 0; cc < s; ++cc) {
            for (int r = 0; r < cc; ++r) {
                double v = P.g1[pg_upper(r, cc, s)];
                for (int i = 0; i < r; ++i) v = v - P.r1[i * S + r] * P.r1[i * S + cc];
                P.r1[r * S + cc] = v / P.r1[r * S + r];
            }
            double d = P.g1[pg_upper(cc, cc, s)];
            for (int i = 0; i < cc; ++i) d = d - P.r1[i * S + cc] * P.r1[i * S + cc];
            if (!(isfinite(d) && d > 1e-12 * P.nu2[cc])) {
                for (int r = 0; r < cc; ++r) P.r1[r * S + cc] = 0.0;
                keep = cc; break;
            }
            P.r1[cc * S + cc] = dsqrt(d);
        }
        P.gs->keep = keep;
    }
};
struct PgBlockLogic {                // R2, R = R2 R1, C = C1 + C2, the new Hessenberg columns, Givens, the test per column
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; PgPtrs P; int j, s;
    __device__ void run(const double*) const {
        PgState* gs = P.gs;
        const int S = P.S, k = gs->keep;
        // R2 = chol(G2) of the k kept columns (packed with k columns)
        for (int q = 0; q < S * S; ++q) P.r2[q] = 0.0;
        for (int cc = 0; cc < k; ++cc) {
            for (int r = 0; r < cc; ++r) {
                double v = P.g2[pg_upper(r, cc, k)];
                for (int i = 0; i < r; ++i) v = v - P.r2[i * S + r] * P.r2[i * S + cc];
                P.r2[r * S + cc] = v / P.r2[r * S + r];
            }
            double d = P.g2[pg_upper(cc, cc, k)];
            for (int i = 0; i < cc; ++i) d = d - P.r2[i * S + cc] * P.r2[i * S + cc];
            P.r2[cc * S + cc] = dsqrt(d);
        }
        const int ncols = k > 0 ? k : 1;
        for (int cc = 0; cc < ncols; ++cc) {
            const int col = j + cc;
            // Y = coordinates of W_cc on q_0 .. q_{col+1}: C (rows 0..j), R = R2 R1 (rows j+1 .. j+1+cc); zero for a breakdown
            // t = coordinates of the input of column cc: e_j, or Y_{cc-1} / nu_{cc-1}
            for (int l = 0; l <= col + 1; ++l) {
                double yv;
                if (l <= j) yv = P.c1[l * s + cc] + P.c2[l * s + cc];
                else if (k == 0) yv = 0.0;
                else {
                    const int a = l - j - 1;              // R[a][cc] = sum_{i=a..cc} R2[a][i] R1[i][cc]
                    double acc = 0.0;
                    for (int i = a; i <= cc; ++i) acc = acc + P.r2[a * S + i] * P.r1[i * S + cc];
                    yv = acc;
                }
                HU(l, col) = yv;
            }
            double tdiag = 1.0;
            if (cc > 0) {
                // v = (Y_l - sum_{i < col} t_i H_u[l][i]) / t_col with t = Y_{cc-1} / nu_{cc-1}: Y_{cc-1} is column col-1 of HU's
                // right-hand side, kept in P.y as scratch (rows 0..col)
                const double nuv = P.nu[cc - 1];
                tdiag = P.y[col] / nuv;
                for (int l = 0; l <= col + 1; ++l) {
                    double v = HU(l, col);
                    for (int i = 0; i < col; ++i) v = v - (P.y[i] / nuv) * HU(l, i);
                    HU(l, col) = v / tdiag;
                }
            }
            // keep Y of this column (before its solve) for the next one
            if (cc + 1 < ncols) {
                for (int l = 0; l <= col + 1; ++l) {
                    double yv;
                    if (l <= j) yv = P.c1[l * s + cc] + P.c2[l * s + cc];
                    else {
                        const int a = l - j - 1;
                        double acc = 0.0;
                        for (int i = a; i <= cc; ++i) acc = acc + P.r2[a * S + i] * P.r1[i * S + cc];
                        yv = acc;
                    }
                    P.y[l] = yv;
                }
            }
            for (int l = 0; l <= col + 1; ++l) HH(l, col) = HU(l, col);
            givens_column(P.h, P.R, P.cs, P.sn, P.g, col, EpsGuard{DBL_EPSILON});
            gs->iteration = gs->iteration + 1;
            const double res = fabs(P.g[col + 1]);
            c.push(res);
            c.st->iterations = gs->iteration; c.st->final_residual = res;
            const bool conv = res <= c.tol * gs->res0;
            c.st->converged = conv ? 1 : 0;
            if (conv || gs->iteration >= c.max_iters || k == 0) { gs->cyc_stop = 1; gs->m = col + 1; return; }
        }
        gs->j = j + ncols;
        if (gs->j >= P.R) { gs->cyc_stop = 1; gs->m = P.R; }
    }
};
#undef HH
#undef HU

static int32_t read_pg(kryst_ctx_t ctx, const PgState* d, PgState* h) {
    KR_HIP(hipMemcpyAsync(h, d, sizeof(PgState), hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return KRYST_OK;
}

int32_t pca_gmres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, int32_t block_size, int32_t pipeline_depth, double tau,
                        bool textbook) {
    (void)pipeline_depth; (void)tau;          // never read (pca_gmres.rs: pipeline_depth, tau)
    const EnvFreeze knobs;
    KR_ARG(io.a && io.params, "solve: null argument");
    const kryst_params_t* p = io.params;
    const kryst_pc_t pc = io.pc && p->precond_side == 2 ? io.pc : nullptr;     // Left and None never call pc
    RestartRun run(bv, xv, io);
    KR_TRY(run.check(pc, "pca_gmres: restart must be in 1..4096 (restart = 0 divides by zero, pca_gmres.rs:120)"));
    kryst_csr_t a = run.a; kryst_ctx_t ctx = run.ctx; const int64_t n = run.n, nt = run.nt;
    if (a->dist || ctx->nranks > 1) { set_error("pca_gmres: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(block_size >= 1, "pca_gmres: block_size = 0 never advances (pca_gmres.rs:273)");
    const int R = p->restart;
    const int64_t n_outer = (p->max_iters + R - 1) / R;                                           // :120
    if (!textbook)
        KR_ARG(!(block_size >= 2 && R >= 2 && n_outer >= 1),
               "pca_gmres: block_size >= 2 with restart >= 2 indexes the basis past its end (pca_gmres.rs:145,151,163)");
    KR_ARG(!textbook || block_size <= PG_SMAX, "pca_gmres: s-step block_size must be in 1..16");
    KR_ARG(p->precond_side >= 0 && p->precond_side <= 2, "pca_gmres: precond_side");
    if (textbook && io.pc && p->precond_side == 1) {
        set_error("pca_gmres: the s-step form is right preconditioned only (Left with a preconditioner)");
        return KRYST_UNSUPPORTED;
    }
    const int S = textbook ? block_size : 1;
    KR_TRY(run.begin(textbook ? p->max_iters + 2 : n_outer * R + 2, 5 + (R + 1) + (textbook ? S + 1 : 0)));
    Workspace& ws = run.ws; const LogicCtx& lc = run.lc; LiveMonitor& mon = run.mon; const int* done = run.done;
    PgPtrs P; P.R = R; P.S = S;
    int* d_gate = nullptr;                  // as written: done || cyc_stop in one word, for the SpMV / pc hooks
    double** d_qptr = nullptr;              // [V_0 .. V_R, w] (as written: the last slot is the block vector)
    double** d_wptr = nullptr;              // s-step block columns
    SmallArena small;
    auto carve = [&] {
        const size_t hsz = (size_t)(R + 1) * R, rs = (size_t)(R + 1) * S, ss = (size_t)S * S;
        P.h = small.take<double>(hsz); P.hu = small.take<double>(hsz); P.g = small.take<double>(R + 1);
        P.cs = small.take<double>(R); P.sn = small.take<double>(R); P.y = small.take<double>(R + 1);
        P.gs = small.take<PgState>(1); d_gate = small.take<int>(1);
        P.red = small.take<double>((size_t)(R + 2) * S);
        P.c1 = small.take<double>(rs); P.c2 = small.take<double>(rs); P.g1 = small.take<double>(ss); P.g2 = small.take<double>(ss);
        P.nu2 = small.take<double>(S); P.nu = small.take<double>(S); P.r1 = small.take<double>(ss); P.r2 = small.take<double>(ss);
        d_qptr = small.take<double*>((size_t)R + 2 + S); d_wptr = d_qptr + (R + 2);       // one table: uploaded in one copy
    };
    carve(); KR_TRY(small.alloc(ws)); carve();
    // tile partials of the block inner products
    PgBuf buf;
    buf.ntiles = nt; buf.nchunks = nchunks_of(nt);
    buf.nq = textbook ? std::max((R + 1) * S, S * (S + 1) / 2) : R + 1;
    KR_HIP(hipMalloc(&buf.part, sizeof(double) * (size_t)buf.nq * (size_t)nt));
    ws.vecs.push_back(buf.part);
    KR_HIP(hipMalloc(&buf.chunks, sizeof(double) * (size_t)buf.nq * (size_t)buf.nchunks));
    ws.vecs.push_back(buf.chunks);

    double *xk, *r0, *w, *z, *tmp;
    KR_TRY(ws.vec(&xk)); KR_TRY(ws.vec(&r0)); KR_TRY(ws.vec(&w)); KR_TRY(ws.vec(&z)); KR_TRY(ws.vec(&tmp));
    std::vector<double*> V((size_t)R + 1), W((size_t)S, nullptr);
    for (auto& v : V) KR_TRY(ws.vec(&v));
    double* u = nullptr;
    if (textbook) { for (auto& v : W) KR_TRY(ws.vec(&v)); KR_TRY(ws.vec(&u)); }
    {
        std::vector<double*> tab(V); tab.push_back(nullptr);
        for (auto* v : W) tab.push_back(v);
        KR_HIP(hipMemcpyAsync(d_qptr, tab.data(), sizeof(double*) * tab.size(), hipMemcpyHostToDevice, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
    }
    const CycleGate gdone{done, nullptr}, gcyc{done, &P.gs->cyc_stop};
    int32_t rc = KRYST_OK;

    if (textbook) KR_HIP(hipMemcpyAsync(xk, xv->d, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));   // x0 honoured
    // (as written: xk = 0, :107 -- the work vectors come zero filled)
    KR_TRY(residual_dot(a, bv->d, xk, r0, tmp, nullptr));                                                         // :108-114
    KR_TRY((reduce_then<1>(ctx, nt, ws.red, PgInitLogic{lc, P, textbook ? p->max_iters : n_outer, textbook ? 1 : 0})));

    if (!textbook) {
        double* const wsel = pc ? z : w;                   // the block vector: A v_j, or M^-1 A v_j (Right, :152-156)
        KR_HIP(hipMemcpyAsync(d_qptr + R + 1, &wsel, sizeof(double*), hipMemcpyHostToDevice, ctx->s_main));
        for (int64_t outer = 0; outer < n_outer; ++outer) {                                                    // :121
            KR_TRY(logic_only(ctx, ws.red, PgCycleLogic{lc, P}));
            KR_TRY(launch_ew(ctx, DivOp{&P.gs->beta, r0, V[0]}, n, done));                                    // :124
            for (int j = 0; j < R; ++j) {
                KR_TRY(write_cycle_gate(ctx, gcyc, d_gate));
                KR_TRY(launch_spmv(a, V[j], w, 0, nullptr, d_gate));                                             // :151 / :163
                if (pc) { rc = pc_apply_dev_fresh(pc, n, w, z, d_gate, nullptr); if (rc) return rc; }              // :152-156
                // (v_i, w) for i = 0..j (:174-179) and (w, w) (:225) in one pass
                PgPass ps{};
                ps.q = d_qptr; ps.nb = j + 1; ps.qx = wsel; ps.w = d_qptr + R + 1; ps.s = 1; ps.dots = 1; ps.n = n;
                KR_TRY(pg_pass(ctx, ps, j + 2, P.red, buf, gcyc));
                KR_TRY(logic_only(ctx, ws.red, PgStepLogic{lc, P, j}));
                KR_TRY(launch_ew_gated(ctx, PgMulOp{&P.gs->inv, wsel, V[j + 1]}, n, gcyc));                    // :227-233
            }
            KR_TRY(logic_only(ctx, ws.red, PgBackLogic{lc, P, 0}));
            KR_TRY(launch_ew(ctx, BasisUpdateOp<false>{&P.gs->m, P.y, d_qptr, xk}, n, done));                   // :289-295
            KR_TRY(residual_dot(a, bv->d, xk, r0, tmp, done));                                                  // :298-302
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, PgCycleEndLogic{lc, P})));
            KR_HIP(hipStreamSynchronize(ctx->s_main));                                                          // one host sync per cycle
            mon.poll();
            if (ctx->h_prog->done) break;
        }
    } else {
        PgState hs{};
        KR_TRY(read_pg(ctx, P.gs, &hs));
        while (!ctx->h_prog->done) {
            KR_TRY(logic_only(ctx, ws.red, PgCycleLogic{lc, P}));
            KR_TRY(launch_ew(ctx, DivOp{&P.gs->beta, r0, V[0]}, n, done));                                    // q0 = r0 / ||r0||
            int j = 0;
            long long it = hs.iteration;
            while (true) {
                const int s_eff = (int)std::min<long long>({(long long)S, (long long)(R - j), (long long)p->max_iters - it});
                if (s_eff <= 0) break;
                // block generation: W_c = A M^-1 (input_c), input_0 = q_j, input_c = W_{c-1} / ||W_{c-1}||
                for (int cc = 0; cc < s_eff; ++cc) {
                    const double* in = (cc == 0) ? V[j] : u;
                    const double* zin = in;
                    if (pc) { rc = pc_apply_dev_fresh(pc, n, in, z, done, nullptr); if (rc) return rc; zin = z; }
                    KR_TRY(launch_spmv(a, zin, W[cc], 0, nullptr, done));
                    KR_TRY(launch_ew(ctx, DotOneOp{W[cc], W[cc]}, n, done));
                    KR_TRY((reduce_then<1>(ctx, nt, ws.red, PgNuLogic{lc, P, cc})));
                    if (cc + 1 < s_eff) KR_TRY(launch_ew(ctx, DivOp{P.nu + cc, W[cc], u}, n, done));
                }
                const int nb = j + 1, ng = s_eff * (s_eff + 1) / 2;
                PgPass ps{};
                ps.q = d_qptr; ps.nb = nb; ps.w = d_wptr; ps.s = s_eff; ps.n = n;
                ps.update = 0; ps.dots = 1;                                                    // pass A: C1 = Q^T W
                KR_TRY(pg_pass(ctx, ps, nb * s_eff, P.c1, buf, gdone));
                ps.update = 1; ps.coef = P.c1; ps.cs = s_eff; ps.dots = 1;                    // pass B: W -= Q C1, C2 = Q^T W
                KR_TRY(pg_pass(ctx, ps, nb * s_eff, P.c2, buf, gdone));
                ps.coef = P.c2; ps.dots = 2;                                                  // pass C: W -= Q C2, G1 = W^T W
                KR_TRY(pg_pass(ctx, ps, ng, P.g1, buf, gdone));
                KR_TRY(logic_only(ctx, ws.red, PgChol1Logic{lc, P, s_eff}));
                ps.update = 2; ps.rm = P.r1; ps.rs = S; ps.out = d_wptr; ps.sdev = &P.gs->keep; ps.dots = 2;   // pass D: W R1^-1, G2
                KR_TRY(pg_pass(ctx, ps, ng, P.g2, buf, gdone));
                KR_TRY(logic_only(ctx, ws.red, PgBlockLogic{lc, P, j, s_eff}));
                ps.rm = P.r2; ps.out = d_qptr + j + 1; ps.dots = 0;                           // pass E: Q_new = W R2^-1
                KR_TRY(pg_pass(ctx, ps, 0, nullptr, buf, gdone));
                KR_TRY(read_pg(ctx, P.gs, &hs));                                               // one host sync per block
                it = hs.iteration;
                if (hs.cyc_stop || ctx->h_prog->done) break;
                j = hs.j;
            }
            // cycle end: x += M^-1 (Q y), the true residual
            KR_TRY(logic_only(ctx, ws.red, PgBackLogic{lc, P, 1}));
            KR_TRY(launch_ew(ctx, BasisUpdateOp<true>{&P.gs->m, P.y, d_qptr, tmp}, n, done));
            const double* add = tmp;
            if (pc) { rc = pc_apply_dev_fresh(pc, n, tmp, z, done, nullptr); if (rc) return rc; add = z; }
            KR_TRY(launch_ew(ctx, PgAddOp{add, xk}, n, done));
            KR_TRY(residual_dot(a, bv->d, xk, r0, tmp, done));
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, PgCycleEndLogic{lc, P})));
            KR_TRY(read_pg(ctx, P.gs, &hs));
            mon.poll();
        }
    }
    return run.end(xk);
}

}  // namespace kr
