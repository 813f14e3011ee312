// Several right-hand sides at once: kryst_mvec_t, Y <- A X (spmm_rows_kernel on plain CSR here, spmm_dia_kernel on the diagonal streams in
// multi_dia.hip; launch_spmm decides) and batched CG / Jacobi-PCG.
//
// The contract is one sentence: column j of a batched call is, bit for bit, what the single-vector call returns for column j -- y, x,
// the iteration count, every residual-history entry, final_residual, converged and the status.  It holds because nothing here re-associates:
// a row of the SpMM is summed in ascending column order from 0.0 with separate multiply and add, per column; a fused
// inner product folds the lane's two terms in index order, the 64-lane butterfly, the four waves, and the tile partials in fold2's tree, per
// column (section 4.2); and the scalar step of every column is the single solver's own code (cg_logic.h), bound to that column's DevState.
// What changes is where bytes move: the matrix is read once for K columns.
#include "multi.h"
#include "cg_logic.h"
#include "spmv.h"

namespace kr {

typedef int32_t v2i __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------- storage
// interleave: d[i * k + j] = cm[j * n + i]  (cm: k columns of n, one after the other) / the inverse
__global__ void mvec_interleave_kernel(double* d, double* cm, int64_t n, int k, int to_rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        for (int j = 0; j < k; ++j) {
            if (to_rows) d[i * k + j] = cm[(int64_t)j * n + i];
            else cm[(int64_t)j * n + i] = d[i * k + j];
        }
    }
}
// column j of the multivector <- v (set != 0) or v <- column j
__global__ void mvec_column_kernel(double* d, double* v, int64_t n, int k, int j, int set) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (set) d[i * k + j] = v[i];
        else v[i] = d[i * k + j];
    }
}
// rows [n, rows) of every column: count the elements whose bits are not +0.0, then (fill) overwrite them.  One workgroup.
__global__ void mvec_padding_kernel(double* d, int64_t n, int64_t rows, int k, int fill, double value, unsigned long long* count) {
    unsigned long long mine = 0;
    for (int64_t e = n * k + threadIdx.x; e < rows * k; e += blockDim.x) {
        if (__double_as_longlong(d[e]) != 0ll) ++mine;
        if (fill) d[e] = value;
    }
    if (mine) atomicAdd(count, mine);
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048)); }

int32_t mvec_check(kryst_mvec_t mv) {
    KR_ARG(mv && mv->d && mv->ctx, "multivector: null handle");
    return KRYST_OK;
}

// host columns (column j at host + j * ld) <-> the interleaved device array, through a compact device staging buffer and a device kernel
static int32_t mvec_transfer(kryst_mvec_t mv, double* host, int64_t ld, bool up) {
    KR_TRY(mvec_check(mv));
    KR_ARG(host && ld >= mv->n, "multivector transfer: null host pointer or ld < n");
    kryst_ctx_t ctx = mv->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    if (mv->n == 0) return KRYST_OK;
    double* tmp = nullptr;
    const size_t col_bytes = sizeof(double) * (size_t)mv->n;
    KR_HIP(hipMalloc(&tmp, col_bytes * (size_t)mv->k));
    hipError_t e = hipSuccess;
    if (up) {
        for (int j = 0; j < mv->k && e == hipSuccess; ++j)
            e = hipMemcpyAsync(tmp + (size_t)j * mv->n, host + (size_t)j * ld, col_bytes, hipMemcpyHostToDevice, ctx->s_main);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(mvec_interleave_kernel, dim3(grid_for(mv->n)), dim3(256), 0, ctx->s_main, mv->d, tmp, mv->n, mv->k, 1);
            e = hipGetLastError();
        }
    } else {
        hipLaunchKernelGGL(mvec_interleave_kernel, dim3(grid_for(mv->n)), dim3(256), 0, ctx->s_main, mv->d, tmp, mv->n, mv->k, 0);
        e = hipGetLastError();
        for (int j = 0; j < mv->k && e == hipSuccess; ++j)
            e = hipMemcpyAsync(host + (size_t)j * ld, tmp + (size_t)j * mv->n, col_bytes, hipMemcpyDeviceToHost, ctx->s_main);
    }
    const hipError_t s = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(tmp);
    KR_HIP(e);
    KR_HIP(s);
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- SpMM
// The shape of spmv_rows_kernel (spmv_stream.hip) on K interleaved columns.  A workgroup owns 512-row tiles, thread t rows 2t and 2t+1.  Phase 1:
// each wave streams the (col, val) run of its 128 rows into a private LDS window, every load of the window in flight at once, ordered by
// wave barriers only.  Phase 2: the owner lane walks its two rows in ascending column order and loads the K contiguous doubles of X-row c
// with 16-byte loads, U entries of each row in flight; 2 K running sums stay in registers.  Rows longer than a window loop over windows.
// Matrix bytes per row and column fall from 88 to 88 / K on a 7-point operator; an x gather fetches 8 K contiguous bytes instead of 8.
struct SpmmArgs {
    const int32_t* row_ptr; const int32_t* col; const double* val;
    const double* x; double* y; const double* dvec; double* partials; int64_t pstride;
    int nrows; int ntiles; const int* done;
};

template <int K, int NQ>
__global__ __launch_bounds__(KR_T) void spmm_rows_kernel(const SpmmArgs a) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(NQ == 0 || NQ == 1 || NQ == 2, "NQ");
    if (a.done && *a.done) return;
    constexpr int SLOTS = 4;
    constexpr int WCAP = SLOTS * 128;                       // entries per wave window
    constexpr int U = K == 8 ? 2 : 4;                       // entries of each row in flight: 2 * U * K gathered doubles per lane
    constexpr int H = K / 2;
    __shared__ __attribute__((aligned(16))) double val_all[4 * WCAP];
    __shared__ __attribute__((aligned(16))) int32_t col_all[4 * WCAP];
    __shared__ double red[(NQ == 2 ? BcgShape<K>::RG : NQ == 1 ? K : 1) * (KR_T / 64)];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    double* lval = val_all + w * WCAP;
    int32_t* lcol = col_all + w * WCAP;
    for (int q = blockIdx.x; q < a.ntiles; q += gridDim.x) {
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int wr0 = min(r0 + 128 * w, r1), wr1 = min(wr0 + 128, r1);
        const int row = r0 + 2 * t;
        const int p0 = a.row_ptr[min(row, r1)];
        const int p1 = a.row_ptr[min(row + 1, r1)];
        const int p2 = a.row_ptr[min(row + 2, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s0[K], s1[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { s0[j] = 0.0; s1[j] = 0.0; }
        for (int base = k0 & ~1; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            const int npairs = (wend - base + 1) >> 1;
            // ---- phase 1: stream the window into LDS (the arrays carry 8 entries of zero padding: a pair may reach one entry past nnz)
            kr_v2d v[SLOTS]; v2i c[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int pi = min(l + j * 64, npairs - 1);
                const int k = base + 2 * pi;
                v[j] = *reinterpret_cast<const kr_v2d*>(a.val + k);
                c[j] = *reinterpret_cast<const v2i*>(a.col + k);
            }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                *reinterpret_cast<double2*>(&lval[2 * (l + j * 64)]) = make_double2(v[j].x, v[j].y);
                *reinterpret_cast<int2*>(&lcol[2 * (l + j * 64)]) = make_int2(c[j].x, c[j].y);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- phase 2: the two rows of the lane, U entries of each in flight, folded in ascending column order, per column
            int ka = max(p0, base), kb = max(p1, base);
            const int ea = min(p1, wend), eb = min(p2, wend);
            while (ka < ea || kb < eb) {
                double va[U], vb[U]; kr_v2d xa[U][H], xb[U][H];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int ia = min(ka + u, max(ea - 1, base)), ib = min(kb + u, max(eb - 1, base));
                    const int ca = lcol[ia - base], cb = lcol[ib - base];
                    va[u] = lval[ia - base]; vb[u] = lval[ib - base];
                    const kr_v2d* pa = reinterpret_cast<const kr_v2d*>(a.x + (int64_t)ca * K);
                    const kr_v2d* pb = reinterpret_cast<const kr_v2d*>(a.x + (int64_t)cb * K);
                    const bool oa = ka + u < ea, ob = kb + u < eb;
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        kr_v2d z; z.x = 0.0; z.y = 0.0;
                        xa[u][h] = oa ? pa[h] : z;
                        xb[u][h] = ob ? pb[h] : z;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (ka + u < ea) {
#pragma unroll
                        for (int h = 0; h < H; ++h) { s0[2 * h] = s0[2 * h] + va[u] * xa[u][h].x; s0[2 * h + 1] = s0[2 * h + 1] + va[u] * xa[u][h].y; }
                    }
                    if (kb + u < eb) {
#pragma unroll
                        for (int h = 0; h < H; ++h) { s1[2 * h] = s1[2 * h] + vb[u] * xb[u][h].x; s1[2 * h + 1] = s1[2 * h + 1] + vb[u] * xb[u][h].y; }
                    }
                }
                ka += U; kb += U;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // Y: 2 K contiguous doubles per lane
        kr_v2d* yp = reinterpret_cast<kr_v2d*>(a.y + (int64_t)row * K);
        if (row < r1) {
#pragma unroll
            for (int h = 0; h < H; ++h) { kr_v2d o; o.x = s0[2 * h]; o.y = s0[2 * h + 1]; yp[h] = o; }
        }
        if (row + 1 < r1) {
#pragma unroll
            for (int h = 0; h < H; ++h) { kr_v2d o; o.x = s1[2 * h]; o.y = s1[2 * h + 1]; yp[H + h] = o; }
        }
        if constexpr (NQ == 2) spmm_gram_epilogue<K>(a.x, row, row < r1, row + 1 < r1, s0, s1, red, a.partials, a.pstride, q);
        if constexpr (NQ == 1) {
            // (D_j, Y_j) per column: the lane's two products in index order, the 64-lane butterfly, the serial fold over the 4 waves
            const kr_v2d* dp = reinterpret_cast<const kr_v2d*>(a.dvec + (int64_t)row * K);     // (rows behind n lie in the padding: read, never used)
            double acc[K];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const kr_v2d d0 = dp[h], d1 = dp[H + h];
                acc[2 * h] = 0.0; acc[2 * h + 1] = 0.0;
                if (row < r1) { acc[2 * h] = acc[2 * h] + d0.x * s0[2 * h]; acc[2 * h + 1] = acc[2 * h + 1] + d0.y * s0[2 * h + 1]; }
                if (row + 1 < r1) { acc[2 * h] = acc[2 * h] + d1.x * s1[2 * h]; acc[2 * h + 1] = acc[2 * h + 1] + d1.y * s1[2 * h + 1]; }
            }
            block_reduce<NQ * K, KR_T / 64>(acc, red);
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < K; ++j) a.partials[j * a.pstride + q] = acc[j];
            }
        }
    }
}

template <int K>
static int32_t launch_spmm_k(kryst_ctx_t ctx, const SpmmArgs& args, int nq) {
    // LDS: 24 KiB per workgroup; memory-bound streaming with a capped grid like the other kernels (ew.h: launch_ew_gated)
    const int bpc = std::max(1, env_int("KRYST_SPMM_BLOCKS_PER_CU", 4));
    const int64_t grid = std::min<int64_t>(args.ntiles, (int64_t)ctx->num_cu * bpc);
    if (grid <= 0) return KRYST_OK;
    if (nq == 2) hipLaunchKernelGGL((spmm_rows_kernel<K, 2>), dim3((unsigned)grid), dim3(KR_T), 0, ctx->s_main, args);
    else if (nq) hipLaunchKernelGGL((spmm_rows_kernel<K, 1>), dim3((unsigned)grid), dim3(KR_T), 0, ctx->s_main, args);
    else hipLaunchKernelGGL((spmm_rows_kernel<K, 0>), dim3((unsigned)grid), dim3(KR_T), 0, ctx->s_main, args);
    KR_HIP(hipGetLastError());
    phase_mark(ctx, KR_PH_SPMV);
    return KRYST_OK;
}

// KRYST_SPMM_FORM = auto | plain | dia: 0 auto (also unset, or no such word), 1 plain, 2 dia; read as env_int reads a number (once per EnvFreeze)
static int spmm_form_knob() {
    static EnvSlot slot;
    return (int)env_parsed_cached(slot, "KRYST_SPMM_FORM", 0, [](const char* v) -> long long { return !strcmp(v, "plain") ? 1 : !strcmp(v, "dia") ? 2 : 0; });
}
// The choice: which SpMM kernel a launch takes is decided HERE; launch_spmm and kryst_spmm_kernel both ask.  `dia`: spmm_dia_kernel wherever the
// operator holds the streams, else (silently) the plain kernel.  `auto`: spmm_dia_kernel where the operator's own SpMV streams CSR-DIA, for the
// widths at which it measured no slower than spmm_rows_kernel on the same operator at 256^3 and 512^3.
constexpr bool SPMM_DIA_AUTO[3] = {true, true, true};                   // K = 2, 4, 8
bool spmm_takes_dia(kryst_csr_t a, int k) {
    const int form = spmm_form_knob();
    if (form == 1 || !mvec_width_ok(k)) return false;
    if (!a->d_dia || a->dist || a->dia_nd <= 0 || a->dia_nd > KR_DIA_MAX) return false;
    if (form == 2) return true;
    return SPMM_DIA_AUTO[k == 2 ? 0 : k == 4 ? 1 : 2] && tile_kernel(a, false, TileRange::Whole) == TileKernel::Dia;
}

int32_t launch_spmm(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done) {
    KR_ARG(nq != 2 || a->nrows == a->xlen, "spmm: the Gram epilogue needs a square operator");
    if (spmm_takes_dia(a, k)) return launch_spmm_dia(a, k, x, y, nq, dvec, partials, pstride, done);
    KR_ARG(a->d_row_ptr && a->d_col && a->d_val, "spmm: the operator keeps no CSR arrays");
    KR_ARG(a->nrows < (1ll << 31) - KR_TILE, "spmm: too many rows");
    SpmmArgs args{a->d_row_ptr, a->d_col, a->d_val, x, y, dvec, partials, pstride, (int)a->nrows, (int)ntiles_of(a->nrows), done};
    switch (k) {
        case 2: return launch_spmm_k<2>(a->ctx, args, nq);
        case 4: return launch_spmm_k<4>(a->ctx, args, nq);
        case 8: return launch_spmm_k<8>(a->ctx, args, nq);
        default: set_error("spmm: k = %d (2, 4 or 8)", k); return KRYST_ERR_ARG;
    }
}

// ---------------------------------------------------------------------------------------------------- pointwise passes over interleaved rows
// (ld_rows / st_rows, a lane's two rows as 2 K contiguous doubles: multi.h)

struct GateAllDone {
    const int* all_done;
    __device__ __forceinline__ bool skip() const { return all_done && *all_done; }
};

// Op: static constexpr int NQ (reductions per column); rows(row, in0, in1, acc) with acc[q * K + j].  Thread t of tile q owns rows
// q * 512 + 2t, +1; the partial of reduction q, column j and this tile goes to partials[(q * K + j) * pstride + tile].
template <int K, class Op>
__global__ __launch_bounds__(KR_T) void mew_kernel(Op op, GateAllDone gate, int64_t n, int64_t ntiles, double* partials, int64_t pstride) {
    if (gate.skip()) return;
    constexpr int NQ = Op::NQ;
    constexpr int NA = NQ > 0 ? NQ * K : 1;
    __shared__ double lds[NA * (KR_T / 64)];
    for (int64_t q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const int64_t row = q * KR_TILE + (int64_t)threadIdx.x * KR_V;
        double acc[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = 0.0;
        op.rows(row, row < n, row + 1 < n, acc);
        if constexpr (NQ > 0) {
            block_reduce_any<NA, KR_T / 64>(acc, lds);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < NA; ++k) partials[k * pstride + q] = acc[k];
            }
        }
    }
}

template <int K, class Op>
inline int32_t launch_mew(kryst_ctx_t ctx, const Op& op, int64_t n, const int* all_done, double* partials, int64_t pstride, int phase) {
    const int64_t ntiles = ntiles_of(n);
    if (ntiles <= 0) return KRYST_OK;
    const int64_t grid = std::min<int64_t>(ntiles, (int64_t)ctx->num_cu * std::max(1, env_int("KRYST_EW_BLOCKS_PER_CU", 3)));
    hipLaunchKernelGGL((mew_kernel<K, Op>), dim3((unsigned)grid), dim3(KR_T), 0, ctx->s_main, op, GateAllDone{all_done}, n, ntiles, partials, pstride);
    KR_HIP(hipGetLastError());
    phase_mark(ctx, phase);
    return KRYST_OK;
}

// r = b - A x (`bi - ax`, cg.rs:123), p = r (:126), partial (r, r) (:127) -- SubDotOp and the copy of CgRun::begin, per column
template <int K>
struct MCgInitOp {
    static constexpr int NQ = 1;
    const double* b; const double* ax; double* r; double* p;
    __device__ __forceinline__ void rows(int64_t row, bool in0, bool in1, double (&acc)[K]) const {
        double bb[2 * K], aa[2 * K], rr[2 * K];
        ld_rows<K>(b, row, bb); ld_rows<K>(ax, row, aa);
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) {
            rr[e] = bb[e] - aa[e];
            if (e < K ? in0 : in1) acc[e % K] = acc[e % K] + rr[e] * rr[e];
        }
        st_rows<K>(r, row, rr); st_rows<K>(p, row, rr);
    }
};
// PcgRun::begin per column: r = b - A x (pcg.rs:119-124), z = M^-1 r (:127-131; Jacobi: inv_diag * r, jacobi.rs:84-86; else z == r), p = z (:132),
// partials (r, z) and (z, z) | (r, r)
template <int K, bool JACOBI>
struct MPcgInitOp {
    static constexpr int NQ = 2;
    const double* b; const double* ax; double* r; double* z; double* p; const double* inv; int norm_type;
    __device__ __forceinline__ void rows(int64_t row, bool in0, bool in1, double (&acc)[2 * K]) const {
        double bb[2 * K], aa[2 * K], rr[2 * K], zz[2 * K];
        ld_rows<K>(b, row, bb); ld_rows<K>(ax, row, aa);
        d2 dv = {0.0, 0.0};
        if constexpr (JACOBI) dv = ld2(inv, row);
        const bool nz = norm_type == 0;                                              // Preconditioned: (z,z); else (r,r)
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) {
            rr[e] = bb[e] - aa[e];
            zz[e] = JACOBI ? (e < K ? dv.a : dv.b) * rr[e] : rr[e];
            if (e < K ? in0 : in1) {
                acc[e % K] = acc[e % K] + rr[e] * zz[e];
                acc[K + e % K] = acc[K + e % K] + (nz ? zz[e] * zz[e] : rr[e] * rr[e]);
            }
        }
        st_rows<K>(r, row, rr);
        if constexpr (JACOBI) st_rows<K>(z, row, zz);
        st_rows<K>(p, row, zz);
    }
};
// CgUpdate1 per column: x += alpha p ; r -= alpha Ap (cg.rs:207-212) ; partial (r, r) (:223).  A column whose solve has ended keeps its x and r.
template <int K>
struct MCgUpdateOp {
    static constexpr int NQ = 1;
    const DevState* st; const double* p; const double* ap; double* x; double* r;
    __device__ __forceinline__ void rows(int64_t row, bool in0, bool in1, double (&acc)[K]) const {
        double al[K]; bool live[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { al[j] = st[j].alpha; live[j] = st[j].done == 0; }
        double pp[2 * K], aa[2 * K], xx[2 * K], rr[2 * K];
        ld_rows<K>(p, row, pp); ld_rows<K>(ap, row, aa); ld_rows<K>(x, row, xx); ld_rows<K>(r, row, rr);
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) {
            const int j = e % K;
            if (live[j]) { xx[e] = xx[e] + al[j] * pp[e]; rr[e] = rr[e] - al[j] * aa[e]; }
            if (e < K ? in0 : in1) acc[j] = acc[j] + rr[e] * rr[e];
        }
        st_rows<K>(x, row, xx); st_rows<K>(r, row, rr);
    }
};
// PcgUpdateOp per column: x += alpha p (pcg.rs:175-177) ; r -= alpha Ap (:179-181) ; z = M^-1 r (:183-187) ; partials (r, z), (z, z) | (r, r)
template <int K, bool JACOBI>
struct MPcgUpdateOp {
    static constexpr int NQ = 2;
    const DevState* st; const double* p; const double* ap; double* x; double* r; double* z; const double* inv; int norm_type;
    __device__ __forceinline__ void rows(int64_t row, bool in0, bool in1, double (&acc)[2 * K]) const {
        double al[K]; bool live[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { al[j] = st[j].alpha; live[j] = st[j].done == 0; }
        double pp[2 * K], aa[2 * K], xx[2 * K], rr[2 * K], zz[2 * K];
        ld_rows<K>(p, row, pp); ld_rows<K>(ap, row, aa); ld_rows<K>(x, row, xx); ld_rows<K>(r, row, rr);
        d2 dv = {0.0, 0.0};
        if constexpr (JACOBI) { ld_rows<K>(z, row, zz); dv = ld2(inv, row); }
        const bool nz = norm_type == 0;
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) {
            const int j = e % K;
            if (live[j]) {
                xx[e] = xx[e] + al[j] * pp[e]; rr[e] = rr[e] - al[j] * aa[e];
                if constexpr (JACOBI) zz[e] = (e < K ? dv.a : dv.b) * rr[e];
            }
            const double ze = JACOBI ? zz[e] : rr[e];
            if (e < K ? in0 : in1) {
                acc[j] = acc[j] + rr[e] * ze;
                acc[K + j] = acc[K + j] + (nz ? ze * ze : rr[e] * rr[e]);
            }
        }
        st_rows<K>(x, row, xx); st_rows<K>(r, row, rr);
        if constexpr (JACOBI) st_rows<K>(z, row, zz);
    }
};
// AypxDevOp per column: p = z + beta p (cg.rs:274-276, pcg.rs:215-217; z = r for CG).  A column whose solve has ended keeps its p.
template <int K>
struct MDirectionOp {
    static constexpr int NQ = 0;
    const DevState* st; const double* z; double* p;
    __device__ __forceinline__ void rows(int64_t row, bool, bool, double (&)[1]) const {
        double be[K]; bool live[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { be[j] = st[j].beta; live[j] = st[j].done == 0; }
        double zz[2 * K], pp[2 * K];
        ld_rows<K>(z, row, zz); ld_rows<K>(p, row, pp);
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) { if (live[e % K]) pp[e] = zz[e] + be[e % K] * pp[e]; }
        st_rows<K>(p, row, pp);
    }
};
// X(:, j) <- XW(:, j) for the columns of `mask` (the columns that ended without an error: on Err the reference never reaches `*x = ...`)
template <int K>
struct MWriteBackOp {
    static constexpr int NQ = 0;
    const double* xw; double* x; unsigned mask;
    __device__ __forceinline__ void rows(int64_t row, bool, bool, double (&)[1]) const {
        double ww[2 * K], xx[2 * K];
        ld_rows<K>(xw, row, ww); ld_rows<K>(x, row, xx);
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) { if ((mask >> (e % K)) & 1u) xx[e] = ww[e]; }
        st_rows<K>(x, row, xx);
    }
};

// ---------------------------------------------------------------------------------------------------- the scalar step of K columns
// One launch folds the NQ * K arrays of tile partials (fold2, the tree of every other fold) and then runs the single solver's logic struct L
// once per column that is still under way, bound to that column's DevState, history slice and reduced values.  A column's own `done`
// freezes it; `all_done` (every column done) gates whole launches the way `done` gates the single solver's, and is what the host polls.
struct MultiCtx {
    DevState* st; double* hist; long long hist_cap; HostProgress* colprog; HostProgress* prog; int* all_done; double* red;
    double tol; long long max_iters; int norm_type;
};

template <int NQ, int K, class L>
__global__ __launch_bounds__(KR_F) void fold_multi_kernel(const double* partials, int64_t stride, int64_t ntiles, double* chunks, int64_t cstride,
                                                          unsigned int* ticket, unsigned int* err, MultiCtx m) {
    if (*m.all_done) return;                                  // uniform over the grid: only the workgroup that holds the result ever sets it
    __shared__ double lds[NQ * K * (KR_F / 64)];
    double v[NQ * K];
    const int f = fold2<NQ * K>(partials, stride, ntiles, chunks, cstride, ticket, err, v, lds);
    if (!f) return;
    if (threadIdx.x != 0) return;
    int live = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        DevState* st = m.st + j;
        if (st->done) continue;
        const LogicCtx c{st, m.hist + (long long)j * m.hist_cap, m.colprog + j, m.red + j * NQ, m.tol, m.max_iters, m.norm_type, m.hist_cap, 0};
        if (f == 2) { c.finish(KRYST_ERR_HIP); continue; }    // the hand-off gave up: no value to act on
#pragma unroll
        for (int q = 0; q < NQ; ++q) m.red[j * NQ + q] = v[q * K + j];
        const L logic{c};
        logic.run(m.red + j * NQ);
        if (!st->done) ++live;
    }
    if (!live) {
        *m.all_done = 1;
        __threadfence_system();
        m.prog->done = 1;
        __threadfence_system();
    }
}

// ---------------------------------------------------------------------------------------------------- batched CG / PCG
// (MultiIO: multi.h)

// what is refused before anything is launched or written
int32_t multi_args_check(const MultiIO& io, bool pcg) {
    KR_ARG(io.b && io.x && io.a && io.params, "solve_multi: null argument");
    KR_TRY(mvec_check(io.b)); KR_TRY(mvec_check(io.x));
    KR_ARG(io.b->ctx == io.a->ctx && io.x->ctx == io.a->ctx, "solve_multi: context mismatch");
    KR_ARG(io.b->k == io.x->k, "solve_multi: B and X differ in their number of columns");
    KR_ARG(io.a->nrows == io.a->xlen, "solve_multi: square operator required");
    KR_ARG(io.b->n == io.a->nrows && io.x->n == io.a->nrows, "solve_multi: multivector length != operator size");
    KR_ARG(io.params->max_iters >= 0, "solve_multi: max_iters < 0");
    KR_ARG(!io.pc || io.pc->ctx == io.a->ctx, "solve_multi: preconditioner belongs to another context");
    KR_ARG(!io.pc || io.pc->n < 0 || io.pc->n == io.a->nrows, "solve_multi: preconditioner size mismatch");
    KR_ARG(io.hist_cap >= 0, "solve_multi: hist_cap < 0");
    const char* why = nullptr;
    if (io.a->dist || io.a->ctx->nranks > 1) why = "distributed operators";
    else if (io.params->norm_type != 0 && io.params->norm_type != 1) why = "norm types other than Preconditioned and Unpreconditioned";
    else if (io.params->has_radius) why = "the trust-region exit (with_radius)";
    else if (io.params->has_obj_target) why = "the objective exit (with_obj_target)";
    else if (pcg && io.pc && io.pc->kind != KR_PC_IDENTITY && io.pc->kind != KR_PC_JACOBI) why = "preconditioners other than Identity and Jacobi";
    if (why) { set_error("solve_multi: %s are not supported on multivectors", why); return KRYST_UNSUPPORTED; }
    return KRYST_OK;
}

template <int K>
struct MultiRun {
    static constexpr int64_t HIST_MAX_COL = Workspace::HIST_MAX / 8;      // entries kept per column (the count still runs on)
    MultiIO io; bool pcg; kryst_params_t prm;
    kryst_csr_t a; kryst_ctx_t ctx; int64_t n, nt;
    Workspace ws;
    bool jac = false; const double* inv_diag = nullptr;
    double *xw = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *ap = nullptr;
    double* partials = nullptr; int64_t pstride = 0; double* chunks = nullptr; int64_t cstride = 0;
    char* scal = nullptr; DevState* st = nullptr; int* all_done = nullptr; HostProgress* colprog = nullptr; double* red = nullptr;
    int64_t hist_col = 0;
    MultiCtx mc{};

    // a Workspace vector of this length is exactly one multivector: (ceil(n / 512) * 512 + 512) * K doubles
    static int64_t ws_len(int64_t n) { return mvec_rows(n) * K - KR_TILE; }
    MultiRun(const MultiIO& io_, bool pcg_)
        : io(io_), pcg(pcg_), prm(*io_.params), a(io_.a), ctx(io_.a->ctx), n(io_.a->nrows), nt(ntiles_of(io_.a->nrows)), ws(io_.a->ctx, ws_len(io_.a->nrows)) {}

    template <int NQ, class L>
    int32_t fold_then() {
        hipLaunchKernelGGL((fold_multi_kernel<NQ, K, L>), dim3((unsigned)nchunks_of(nt)), dim3(KR_F), 0, ctx->s_main,
                           partials, pstride, nt, chunks, cstride, fold_ticket(ctx), fold_err(ctx), mc);
        KR_HIP(hipGetLastError());
        phase_mark(ctx, KR_PH_REDUCE);
        return KRYST_OK;
    }

    int32_t begin() {
        KR_HIP(hipSetDevice(ctx->device));
        hist_col = std::max<int64_t>(2, std::min<int64_t>(prm.max_iters + 2, HIST_MAX_COL));
        KR_TRY(ws.init(hist_col * K));
        jac = pcg && io.pc && io.pc->kind == KR_PC_JACOBI;
        inv_diag = jac ? pc_jacobi_inv_diag(io.pc) : nullptr;
        KR_TRY(ws.reserve(jac ? 5 : 4));                                   // xw, r, p, ap [, z]
        if (ws.vec_bytes() < sizeof(double) * (size_t)(mvec_rows(n) * K)) { set_error("solve_multi: a work vector is smaller than a multivector"); return KRYST_ERR_HIP; }
        // scalar state of the batch: K DevStates, K progress records nobody polls, the reduced values, the word every launch is gated by -- a slice
        // of the context's scalar arena behind what a single solve ([0, 512) doubles) and kryst_dot / kryst_norm ([1024, 3080)) use there
        constexpr size_t ST_BYTES = (sizeof(DevState) * K + 63) & ~(size_t)63, PROG_BYTES = (sizeof(HostProgress) * K + 63) & ~(size_t)63;
        constexpr size_t SCAL_BYTES = ST_BYTES + PROG_BYTES + sizeof(double) * 2 * K + 64;
        constexpr size_t SCAL_AT = 3200;                                   // doubles
        static_assert(SCAL_AT * sizeof(double) + SCAL_BYTES <= 4096 * sizeof(double), "the scalar arena holds 4096 doubles (ctx.cpp)");
        scal = reinterpret_cast<char*>(ctx->d_scal + SCAL_AT);
        KR_HIP(hipMemsetAsync(scal, 0, SCAL_BYTES, ctx->s_main));
        st = reinterpret_cast<DevState*>(scal);
        colprog = reinterpret_cast<HostProgress*>(scal + ST_BYTES);
        red = reinterpret_cast<double*>(scal + ST_BYTES + PROG_BYTES);
        all_done = reinterpret_cast<int*>(scal + ST_BYTES + PROG_BYTES + sizeof(double) * 2 * K);
        KR_TRY(ws.vec(&xw)); KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&p)); KR_TRY(ws.vec(&ap));
        if (jac) KR_TRY(ws.vec(&z)); else z = r;                         // z == r (pcg.rs:130,186 clone_from / IdentityPC)
        // Tile partials of up to 2 K = 16 reductions and the chunk cells of their two-level fold: the context's own reduction scratch, which holds
        // KR_MAXQ = 8 arrays, sized for twice the tiles and addressed with strides of this solve (its capacity is at least what was asked for: 8 (2 nt + 128) = 16 (nt + 64) partials;
        // 8 (nchunks(2 nt + 128) + 8) >= 16 nchunks(nt) cells).  Every cell is armed when the scratch is made and fold2 arms a cell again behind
        // itself, so the cells are armed whatever stride the last fold addressed them with.
        KR_TRY(ensure_partials(ctx, 2 * nt + 128));
        pstride = nt + 64; cstride = nchunks_of(nt);
        partials = ctx->d_partials; chunks = ctx->d_chunks;
        if (2 * K * pstride > KR_MAXQ * ctx->partials_cap || 2 * K * cstride > KR_MAXQ * ctx->chunks_cap) { set_error("solve_multi: reduction scratch does not fit"); return KRYST_ERR_HIP; }
        mc = MultiCtx{st, ws.d_hist, (long long)hist_col, colprog, ctx->d_prog, all_done, red, prm.tol, (long long)prm.max_iters, prm.norm_type};
        KR_HIP(hipMemcpyAsync(xw, io.x->d, sizeof(double) * (size_t)(nt * KR_TILE * K), hipMemcpyDeviceToDevice, ctx->s_main));
        KR_TRY(launch_spmm(a, K, xw, ap, 0, nullptr, nullptr, 0, nullptr));                                   // cg.rs:120-122, pcg.rs:119-121
        if (!pcg) {
            KR_TRY((launch_mew<K>(ctx, MCgInitOp<K>{io.b->d, ap, r, p}, n, nullptr, partials, pstride, KR_PH_BLAS1)));
            return fold_then<1, CgInitLogic>();
        }
        if (jac) KR_TRY((launch_mew<K>(ctx, MPcgInitOp<K, true>{io.b->d, ap, r, z, p, inv_diag, prm.norm_type}, n, nullptr, partials, pstride, KR_PH_BLAS1)));
        else KR_TRY((launch_mew<K>(ctx, MPcgInitOp<K, false>{io.b->d, ap, r, z, p, nullptr, prm.norm_type}, n, nullptr, partials, pstride, KR_PH_BLAS1)));
        return fold_then<2, PcgInitLogic>();
    }

    int32_t iterate(int64_t) {
        KR_TRY(launch_spmm(a, K, p, ap, 1, p, partials, pstride, all_done));                                  // cg.rs:143-144 + (p,Ap) :164 ; pcg.rs:149-160
        if (!pcg) {
            KR_TRY((fold_then<1, CgAlphaLogic>()));
            KR_TRY((launch_mew<K>(ctx, MCgUpdateOp<K>{st, p, ap, xw, r}, n, all_done, partials, pstride, KR_PH_BLAS1_RESIDUAL)));
            KR_TRY((fold_then<1, CgBetaLogic>()));
        } else {
            KR_TRY((fold_then<1, PcgAlphaLogic>()));
            if (jac) KR_TRY((launch_mew<K>(ctx, MPcgUpdateOp<K, true>{st, p, ap, xw, r, z, inv_diag, prm.norm_type}, n, all_done, partials, pstride, KR_PH_BLAS1_RESIDUAL)));
            else KR_TRY((launch_mew<K>(ctx, MPcgUpdateOp<K, false>{st, p, ap, xw, r, z, nullptr, prm.norm_type}, n, all_done, partials, pstride, KR_PH_BLAS1_RESIDUAL)));
            KR_TRY((fold_then<2, PcgBetaLogic>()));
        }
        return launch_mew<K>(ctx, MDirectionOp<K>{st, z, p}, n, all_done, nullptr, 0, KR_PH_BLAS1_DIRECTION);
    }

    int32_t end() {
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        DevState h[K];
        KR_HIP(hipMemcpyAsync(h, st, sizeof(DevState) * K, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        const bool pc_bad = io.pc && pc_health(io.pc) != KRYST_OK;
        bool gave_up = false;
        for (int j = 0; j < K; ++j) gave_up = gave_up || h[j].status == KRYST_ERR_HIP;
        if (gave_up) (void)fold_gave_up(ctx);                             // explains, and switches the context to the ticket hand-off
        unsigned mask = 0;
        for (int j = 0; j < K; ++j) {
            const int32_t code = pc_bad ? KRYST_SOLVE_ERROR : h[j].status;
            if (io.stats) { io.stats[j].iterations = h[j].iterations; io.stats[j].final_residual = h[j].final_residual; io.stats[j].converged = h[j].converged; }
            if (io.status) io.status[j] = code;
            if (io.hist_len) io.hist_len[j] = h[j].hist_len;
            if (io.hist) {
                const int64_t keep = std::min<int64_t>(std::min<int64_t>(h[j].hist_len, hist_col), io.hist_cap);
                for (int64_t k = 0; k < keep; ++k) io.hist[(size_t)j * io.hist_cap + k] = ws.h_hist[(size_t)j * hist_col + k];
            }
            if (code == KRYST_OK) mask |= 1u << j;
        }
        if (mask) KR_TRY((launch_mew<K>(ctx, MWriteBackOp<K>{xw, io.x->d, mask}, n, nullptr, nullptr, 0, KR_PH_BLAS1)));
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

static int32_t multi_solve(const MultiIO& io, bool pcg) {
    KR_TRY(multi_args_check(io, pcg));
    switch (io.b->k) {
        case 2: { MultiRun<2> run(io, pcg); return run.solve(); }
        case 4: { MultiRun<4> run(io, pcg); return run.solve(); }
        case 8: { MultiRun<8> run(io, pcg); return run.solve(); }
        default: set_error("solve_multi: k = %d (2, 4 or 8)", (int)io.b->k); return KRYST_ERR_ARG;
    }
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_mvec_create(kryst_ctx_t ctx, int64_t n, int32_t k, kryst_mvec_t* out) {
    KR_ARG(ctx && out && n >= 0, "mvec_create");
    KR_ARG(mvec_width_ok(k), "mvec_create: k must be 2, 4 or 8");
    KR_HIP(hipSetDevice(ctx->device));
    kryst_mvec_t mv = new kryst_mvec_s();
    mv->ctx = ctx; mv->n = n; mv->k = k;
    const size_t bytes = sizeof(double) * (size_t)mvec_rows(n) * (size_t)k;
    if (hipMalloc(&mv->d, bytes) != hipSuccess) { (void)hipGetLastError(); delete mv; set_error("hipMalloc(%zu) failed", bytes); return KRYST_ERR_HIP; }
    if (hipMemsetAsync(mv->d, 0, bytes, ctx->s_main) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(mv->d); delete mv; set_error("hipMemsetAsync failed"); return KRYST_ERR_HIP; }
    *out = mv;
    return KRYST_OK;
}

int32_t kryst_mvec_destroy(kryst_mvec_t mv) {
    if (!mv) return KRYST_OK;
    (void)hipSetDevice(mv->ctx->device);
    (void)hipStreamSynchronize(mv->ctx->s_main);
    (void)hipFree(mv->d);
    delete mv;
    return KRYST_OK;
}

int32_t kryst_mvec_shape(kryst_mvec_t mv, int64_t* n, int32_t* k) {
    KR_TRY(mvec_check(mv));
    if (n) *n = mv->n;
    if (k) *k = mv->k;
    return KRYST_OK;
}

int32_t kryst_mvec_upload(kryst_mvec_t mv, const double* host, int64_t ld) { return mvec_transfer(mv, const_cast<double*>(host), ld, true); }
int32_t kryst_mvec_download(kryst_mvec_t mv, double* host, int64_t ld) { return mvec_transfer(mv, host, ld, false); }

static int32_t mvec_column(kryst_mvec_t mv, int32_t j, kryst_vec_t v, int set) {
    KR_TRY(mvec_check(mv));
    KR_ARG(v && v->ctx == mv->ctx, "mvec column: null vector or context mismatch");
    KR_ARG(j >= 0 && j < mv->k, "mvec column: j out of range");
    KR_ARG(v->n == mv->n, "mvec column: length mismatch");
    KR_HIP(hipSetDevice(mv->ctx->device));
    if (mv->n == 0) return KRYST_OK;
    hipLaunchKernelGGL(mvec_column_kernel, dim3(grid_for(mv->n)), dim3(256), 0, mv->ctx->s_main, mv->d, v->d, mv->n, (int)mv->k, (int)j, set);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}
int32_t kryst_mvec_set_column(kryst_mvec_t mv, int32_t j, kryst_vec_t v) { return mvec_column(mv, j, v, 1); }
int32_t kryst_mvec_get_column(kryst_mvec_t mv, int32_t j, kryst_vec_t v) { return mvec_column(mv, j, v, 0); }

int32_t kryst_bench_mvec_padding(kryst_mvec_t mv, const double* fill, int64_t* dirty) {
    KR_TRY(mvec_check(mv));
    kryst_ctx_t ctx = mv->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    unsigned long long* d_count = nullptr;
    KR_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->s_main);
    unsigned long long count = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mvec_padding_kernel, dim3(1), dim3(1024), 0, ctx->s_main, mv->d, mv->n, mvec_rows(mv->n), (int)mv->k, fill ? 1 : 0, fill ? *fill : 0.0, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->s_main);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d_count);
    KR_HIP(e);
    if (dirty) *dirty = (int64_t)count;
    return KRYST_OK;
}

int32_t kryst_spmm(kryst_csr_t a, kryst_mvec_t x, kryst_mvec_t y) {
    KR_ARG(a, "spmm");
    KR_TRY(mvec_check(x)); KR_TRY(mvec_check(y));
    KR_ARG(x->ctx == a->ctx && y->ctx == a->ctx, "spmm: context mismatch");
    KR_ARG(x->k == y->k, "spmm: X and Y differ in their number of columns");
    KR_ARG(x->n == a->xlen, "spmm: X rows != ncols");
    KR_ARG(y->n == a->nrows, "spmm: Y rows != nrows");
    KR_ARG(x->d != y->d, "spmm: X and Y alias");
    if (a->dist || a->ctx->nranks > 1) { set_error("spmm: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(a->ctx->device));
    return launch_spmm(a, x->k, x->d, y->d, 0, nullptr, nullptr, 0, nullptr);
}

int32_t kryst_spmm_kernel(kryst_csr_t a, int32_t k, int32_t* kernel) {
    KR_ARG(a && kernel, "spmm_kernel");
    KR_ARG(mvec_width_ok(k), "spmm_kernel: k must be 2, 4 or 8");
    *kernel = spmm_takes_dia(a, k) ? 1 : 0;
    return KRYST_OK;
}

#define KRYST_MULTI_TAIL kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats, int32_t* status, \
        double* hist, int64_t hist_cap, int64_t* hist_len

int32_t kryst_cg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, KRYST_MULTI_TAIL) {
    return multi_solve(MultiIO{b, x, a, pc, params, stats, status, hist, hist_cap, hist_len}, false);
}
int32_t kryst_pcg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, KRYST_MULTI_TAIL) {
    return multi_solve(MultiIO{b, x, a, pc, params, stats, status, hist, hist_cap, hist_len}, true);
}

static int32_t host_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, bool pcg, KRYST_MULTI_TAIL) {
    KR_ARG(a && b && x && params, "solve_multi: null argument");
    KR_ARG(mvec_width_ok(k), "solve_multi: k must be 2, 4 or 8");
    KR_ARG(n == a->nrows && ld >= n, "solve_multi: n != operator size or ld < n");
    kryst_mvec_t bv = nullptr, xv = nullptr;
    int32_t rc = kryst_mvec_create(a->ctx, n, k, &bv);
    if (rc == KRYST_OK) rc = kryst_mvec_create(a->ctx, n, k, &xv);
    if (rc == KRYST_OK) rc = kryst_mvec_upload(bv, b, ld);
    if (rc == KRYST_OK) rc = kryst_mvec_upload(xv, x, ld);
    if (rc == KRYST_OK) rc = multi_solve(MultiIO{bv, xv, a, pc, params, stats, status, hist, hist_cap, hist_len}, pcg);
    if (rc == KRYST_OK) rc = kryst_mvec_download(xv, x, ld);            // (a column that ended in an error still holds its initial guess)
    (void)kryst_mvec_destroy(bv); (void)kryst_mvec_destroy(xv);
    return rc;
}
int32_t kryst_cg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, KRYST_MULTI_TAIL) {
    return host_multi(b, x, n, k, ld, false, a, pc, params, stats, status, hist, hist_cap, hist_len);
}
int32_t kryst_pcg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, KRYST_MULTI_TAIL) {
    return host_multi(b, x, n, k, ld, true, a, pc, params, stats, status, hist, hist_cap, hist_len);
}

}  // extern "C"
