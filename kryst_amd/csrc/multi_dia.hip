// Several right-hand sides on the diagonal encoding: spmm_dia_kernel, Y <- A X over interleaved n x K arrays from the
// operator's CSR-DIA value streams (csr_create.hip: build_dia), and its launcher.  multi.hip has the choice (launch_spmm / spmm_takes_dia) and the
// batched solvers, which reach this kernel through launch_spmm alone; spmv_stream.hip has the single-vector twin, spmv_dia_kernel.
//
// The contract is spmm_rows_kernel's, so that column j stays kryst_spmv on column j bit for bit: 512-row tiles, thread t owns rows 2t and 2t+1
// for all K columns; each of the 2 K running sums starts from 0.0 and folds the PRESENT entries of its row in stored diagonal order with
// separate multiply and add; an absent entry (its stream bits are KR_DIA_ABSENT) is skipped by a select on the value's bits, never by a branch
// around the loads and never multiplied into the sum, so whatever its X row holds -- NaN, inf, poison -- stays out.  nq = 1: the tile partial of
// sum_i D(i, j) Y(i, j) per column, the lane's two products in index order, block_reduce, partials[j * pstride + tile].
//
// The shape: no row pointers, no column indices, no LDS window and no dependent load.  Per diagonal a lane issues one 16-byte load of its two
// values and K 16-byte loads of the X rows row + off and row + 1 + off, which are one contiguous, 16-byte aligned run of 16 K bytes at
// (row + off) * K.  (8 D + 16 K) / K bytes per row and column: 44 / 30 / 23 for seven diagonals at K = 2 / 4 / 8, against 72 for spmv_dia_kernel.
// Registers decide how many diagonals are in flight: one diagonal holds 4 K + 4 VGPRs of operands and values beside the 4 K of the running
// sums, so the diagonals go in batches of DB (8 or 4 / 4 / 2 at K = 2 / 4 / 8) and the sums are carried from batch to batch -- the order of
// the fold does not change with DB.  __launch_bounds__(256, 4) holds every instantiation to 128 VGPRs: 4 waves per SIMD.
#include "multi.h"
#include "ew.h"

namespace kr {

struct SpmmDiaArgs {
    const double* dia; const double* x; double* y; const double* dvec; double* partials; const int* done;
    int64_t stride, pstride;
    int32_t nrows, ntiles, nd, dia_min;
    int32_t xtop;                   // mvec_rows(xlen) - 2: the last X row at which a run of two rows still ends inside the allocation
    int32_t xlast;                  // xlen - 1: the last X row an entry can address
    int32_t off[KR_DIA_MAX];
};

// NB diagonals starting at d0.  CT: d0 and every index are compile-time constants and all NB diagonals exist (the offsets are plain kernel
// arguments); else a batch's tail re-reads the last diagonal and does not fold it.  FAST: one run of 2 K doubles at row + off (clamped at the
// top of X's allocation: only an absent entry can point there); else each of the two operand rows is clamped into [0, xlen - 1] on its own.
template <int K, int NB, bool CT, bool FAST, bool NT>
__device__ __forceinline__ void spmm_dia_batch(const SpmmDiaArgs& a, int row, int d0, int nd, double (&s0)[K], double (&s1)[K]) {
    constexpr int H = K / 2;
    kr_v2d v[NB], xa[NB][H], xb[NB][H];
    const double* vrow = a.dia + row;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int d = CT ? d0 + u : min(d0 + u, nd - 1);
        const kr_v2d* vp = reinterpret_cast<const kr_v2d*>(vrow + (int64_t)d * a.stride);
        if constexpr (NT) v[u] = __builtin_nontemporal_load(vp); else v[u] = *vp;
        const int64_t c = (int64_t)row + a.off[d];
        if constexpr (FAST) {
            const kr_v2d* p = reinterpret_cast<const kr_v2d*>(a.x + min(c, (int64_t)a.xtop) * K);
#pragma unroll
            for (int h = 0; h < H; ++h) { xa[u][h] = p[h]; xb[u][h] = p[H + h]; }
        } else {
            const int64_t c0 = min(max(c, (int64_t)0), (int64_t)a.xlast), c1 = min(max(c + 1, (int64_t)0), (int64_t)a.xlast);
            const kr_v2d* pa = reinterpret_cast<const kr_v2d*>(a.x + c0 * K);
            const kr_v2d* pb = reinterpret_cast<const kr_v2d*>(a.x + c1 * K);
#pragma unroll
            for (int h = 0; h < H; ++h) { xa[u][h] = pa[h]; xb[u][h] = pb[h]; }
        }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (CT || d0 + u < nd) {
            const bool pa = (unsigned long long)__double_as_longlong(v[u].x) != KR_DIA_ABSENT;
            const bool pb = (unsigned long long)__double_as_longlong(v[u].y) != KR_DIA_ABSENT;
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const double ta0 = s0[2 * h] + v[u].x * xa[u][h].x, ta1 = s0[2 * h + 1] + v[u].x * xa[u][h].y;
                const double tb0 = s1[2 * h] + v[u].y * xb[u][h].x, tb1 = s1[2 * h + 1] + v[u].y * xb[u][h].y;
                s0[2 * h] = pa ? ta0 : s0[2 * h]; s0[2 * h + 1] = pa ? ta1 : s0[2 * h + 1];
                s1[2 * h] = pb ? tb0 : s1[2 * h]; s1[2 * h + 1] = pb ? tb1 : s1[2 * h + 1];
            }
        }
    }
}

// exactly ND diagonals, in batches of DB with a last batch of what is left: every index a compile-time constant
template <int K, int DB, int ND, int D0, bool FAST, bool NT>
__device__ __forceinline__ void spmm_dia_exact(const SpmmDiaArgs& a, int row, double (&s0)[K], double (&s1)[K]) {
    if constexpr (D0 < ND) {
        constexpr int NB = ND - D0 < DB ? ND - D0 : DB;
        spmm_dia_batch<K, NB, true, FAST, NT>(a, row, D0, ND, s0, s1);
        spmm_dia_exact<K, DB, ND, D0 + DB, FAST, NT>(a, row, s0, s1);
    }
}

template <int K, int DB, int EXACT, bool FAST, bool NT>
__device__ __forceinline__ void spmm_dia_rows(const SpmmDiaArgs& a, int row, double (&s0)[K], double (&s1)[K]) {
    if constexpr (EXACT > 0) {
        spmm_dia_exact<K, DB, EXACT, 0, FAST, NT>(a, row, s0, s1);
    } else {
        const int nd = a.nd;
        for (int d0 = 0; d0 < nd; d0 += DB) spmm_dia_batch<K, DB, false, FAST, NT>(a, row, d0, nd, s0, s1);
    }
}

// EXACT: the operator's number of diagonals where the launcher has an instantiation for it (3, 5, 7, 9), else 0: batches of DB at run-time indices.
// A capped grid strides over the tiles in natural order, so consecutive tiles go round-robin over the 8 XCDs as in spmv_dia_kernel.
template <int K, int NQ, int DB, int EXACT, bool NT>
__global__ __launch_bounds__(KR_T, NQ == 2 ? 2 : 4) void spmm_dia_kernel(const SpmmDiaArgs a) {
    static_assert(K == 2 || K == 4 || K == 8, "K");
    static_assert(NQ == 0 || NQ == 1 || NQ == 2, "NQ");
    if (a.done && *a.done) return;
    constexpr int H = K / 2;
    __shared__ double red[(NQ == 2 ? BcgShape<K>::RG : NQ == 1 ? K : 1) * (KR_T / 64)];
    const int t = threadIdx.x;
    for (int q = blockIdx.x; q < a.ntiles; q += gridDim.x) {
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int row = r0 + 2 * t;
        double s0[K], s1[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { s0[j] = 0.0; s1[j] = 0.0; }
        if (r0 + a.dia_min >= 0) spmm_dia_rows<K, DB, EXACT, true, NT>(a, row, s0, s1);         // uniform over the workgroup
        else spmm_dia_rows<K, DB, EXACT, false, NT>(a, row, s0, s1);                            // the lowest diagonal would start before X's row 0
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
        // NQ = 2 (block CG): Gram(X, Y) instead; this arm alone is held to 2 waves per SIMD, its 36 running sums at K = 8 do not fit 128 VGPRs
        if constexpr (NQ == 2) spmm_gram_epilogue<K>(a.x, row, row < r1, row + 1 < r1, s0, s1, red, a.partials, a.pstride, q);
        if constexpr (NQ == 1) {
            // (D_j, Y_j) per column, formed as in spmm_rows_kernel: the lane's two products in index order, the 64-lane butterfly, the 4 waves
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

template <int K, int DB4, int DB8>
static int32_t launch_spmm_dia_k(kryst_csr_t a, const SpmmDiaArgs& g, int nq) {
    kryst_ctx_t ctx = a->ctx;
    // No LDS beyond the reduction scratch, so the grid cap is this kernel's own: 2 workgroups per compute unit (KRYST_SPMM_BLOCKS_PER_CU, the knob
    // of spmm_rows_kernel, with another default) although the registers admit 4, and nontemporal value loads (KRYST_SPMM_DIA_NT).  In-process A/B
    // (tools/multi_rhs_dia.py knobs, profiles/multi_rhs_dia/knobs_*.jsonl; windows >= 0.5 s alternated, medians), variable coefficients, seven
    // diagonals, K = 2 / 4 / 8, milliseconds per SpMM:
    //   256^3   2 / 4 / 8 per CU  0.299 / 0.345 / 0.350 | 0.604 / 0.672 / 0.687 | 1.393 / 1.427 / 1.429     plain loads (at 4) 0.360 | 0.685 | 1.435
    //   512^3   2 / 4 / 8 per CU  2.514 / 3.123 / 3.502 | 4.975 / 5.638 / 6.152 | 11.02 / 11.52 / 12.21     plain loads (at 4) 3.262 | 5.815 | 11.68
    const int bpc = std::max(1, std::min(8, env_int("KRYST_SPMM_BLOCKS_PER_CU", 2)));
    const bool nontemporal = env_int("KRYST_SPMM_DIA_NT", 1) != 0;
    const int64_t ngrid = std::min<int64_t>(g.ntiles, (int64_t)ctx->num_cu * bpc);
    if (ngrid <= 0) return KRYST_OK;
    const dim3 grid((unsigned)ngrid), block(KR_T);
    hipStream_t s = ctx->s_main;
    // exactly 3 / 5 / 7 / 9 diagonals at K = 2 and 4: compile-time indices, batches of this K's DB; else batches of DB4 (fewer than 7 diagonals)
    // or DB8 at run-time indices.  K = 8 has no exact instantiations: with every index known the compiler moves the next batch's loads above
    // this batch's fold, and the 5 / 7 / 9-diagonal kernels with the fused dot spilled 28 - 60 bytes per lane at 128 VGPRs.
    const int nd = g.nd, exact = K < 8 && (nd == 3 || nd == 5 || nd == 7 || nd == 9) ? nd : 0;
    by_int<0, 1, 2>(nq, [&](auto Q) { by_bool(nontemporal, [&](auto NT) {
        constexpr int NQ = Q();
        bool launched = false;
        if constexpr (K < 8)
            launched = by_int<3, 5, 7, 9>(exact, [&](auto ND) { hipLaunchKernelGGL((spmm_dia_kernel<K, NQ, DB8, ND(), NT()>), grid, block, 0, s, g); });
        if (!launched) {
            if (nd < 7) hipLaunchKernelGGL((spmm_dia_kernel<K, NQ, DB4, 0, NT()>), grid, block, 0, s, g);
            else hipLaunchKernelGGL((spmm_dia_kernel<K, NQ, DB8, 0, NT()>), grid, block, 0, s, g);
        }
    }); });
    KR_HIP(hipGetLastError());
    phase_mark(ctx, KR_PH_SPMV);
    return KRYST_OK;
}

// the operator holds the streams and is one rank's whole matrix (launch_spmm has asked spmm_takes_dia)
int32_t launch_spmm_dia(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done) {
    KR_ARG(a->d_dia && a->dia_nd > 0 && a->dia_nd <= KR_DIA_MAX && !a->dist, "spmm: the operator has no CSR-DIA form");
    KR_ARG(a->nrows < (1ll << 31) - KR_TILE && a->xlen < (1ll << 31) - 2 * KR_TILE, "spmm: too many rows");
    SpmmDiaArgs g{a->d_dia, x, y, dvec, partials, done, a->dia_stride, pstride, (int32_t)a->nrows, (int32_t)ntiles_of(a->nrows), a->dia_nd, a->dia_min,
                  (int32_t)(mvec_rows(a->xlen) - 2), (int32_t)(a->xlen - 1), {0}};
    for (int d = 0; d < KR_DIA_MAX; ++d) g.off[d] = a->dia_off[d];
    switch (k) {
        case 2: return launch_spmm_dia_k<2, 4, 8>(a, g, nq);
        case 4: return launch_spmm_dia_k<4, 4, 4>(a, g, nq);
        case 8: return launch_spmm_dia_k<8, 2, 2>(a, g, nq);
        default: set_error("spmm: k = %d (2, 4 or 8)", k); return KRYST_ERR_ARG;
    }
}

}  // namespace kr
