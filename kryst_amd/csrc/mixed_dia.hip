// Mixed precision on the diagonal encoding: spmv32_dia_kernel, the SpMV of a lowered operator that keeps fp32 CSR-DIA
// streams (kryst_csr32_lower_form DIA), its enqueue function, and the lowering of the form (when an operator can take it, the kernel that converts
// the fp64 streams, the fields).  mixed_lower.hip has the skeleton of the lowering, mixed_spmv.hip the choice (spmv32_kernel), mixed_cg.hip the
// solvers; spmv_stream.hip has the fp64 twin, spmv_dia_kernel.
//
// The contract is the other fp32 kernels': the fp32 tile of 1024 rows, thread t owns rows 4t .. 4t+3.  y_i = (float) of the fold from 0.0, in
// diagonal (= stored) order, of (double)v * (double)x[row + off] with separate multiply and add; an absent entry is skipped by a select on its
// bits, never multiplied; a present zero or non-finite value is multiplied; one 16-byte store per lane, rows at or beyond nrows are not stored.
// nq = 1: partials[tile] = the tile partial of sum d_i * y_i (y as stored) in the fp32 tree.  A stream entry is (float) of the fp64 stream entry,
// i.e. bit for bit the lowered CSR value at that position, so the bits are spmv32_wave_kernel's.
//
// The shape is spmv_dia_kernel's at the fp32 tile: per diagonal a lane issues one 16-byte load of its four values and one 16-byte load of
// x[4t + off .. + 3] at 4-byte alignment, all 2 D loads in flight before the fold: 4 D + 8 bytes per row (7-point: 36; fp64 CSR-DIA 72).
#include "mixed.h"

namespace kr {

constexpr unsigned KR32_DIA_ABSENT = KRYST_CSR32_DIA_ABSENT_BITS;

struct Spmv32DiaArgs {
    const float* dia; const float* x; float* y; const float* dvec; double* partials; const int* done;
    int64_t stride;
    int32_t nrows, ntiles, nd, dia_min;
    int32_t xcap;                   // allocated floats of x (vec32_len(ncols)): a 16-byte load must end inside it
    int32_t off[KR_DIA_MAX];
};

// s + p with the operands in THIS order.  IEEE leaves open which NaN an add of two NaNs returns; the hardware keeps its first operand's, and the
// compiler may commute a plain `+` (it did, on the quad-load path only).  The adds of spmv32_wave_kernel and of the row-pattern kernels stand as
// (sum, product), and a row that meets inf - inf and then a NaN operand must give their bits.
__device__ __forceinline__ double add_in_order(double s, double p) {
    double t;
    asm("v_add_f64 %0, %1, %2" : "=v"(t) : "v"(s), "v"(p));
    return t;
}

// one batch of DB diagonals starting at d0 (EXACT: the operator has exactly DB diagonals, so every index is a compile-time constant and the
// offsets are plain kernel arguments); FAST: 16-byte quad loads of x, else per-element clamped loads; NT: nontemporal value loads
template <int DB, bool EXACT, bool FAST, bool NT>
__device__ __forceinline__ void dia32_batch(const Spmv32DiaArgs& a, int row, int d0, int nd, double (&s)[4]) {
    p_v4f v[DB], xx[DB];
    const float* vrow = a.dia + row;
#pragma unroll
    for (int u = 0; u < DB; ++u) {
        const int d = EXACT ? u : min(d0 + u, nd - 1);           // (a batch's tail re-reads the last diagonal; not used below)
        const p_v4f* vp = reinterpret_cast<const p_v4f*>(vrow + (int64_t)d * a.stride);
        if constexpr (NT) v[u] = __builtin_nontemporal_load(vp); else v[u] = *vp;
        const int64_t c = (int64_t)row + a.off[d];
        if constexpr (FAST) {
            // c >= 0 on this path; a quad that would end behind x's allocation belongs to absent entries alone: any valid quad will do
            xx[u] = *reinterpret_cast<const p_v4f_a4*>(a.x + min(c, (int64_t)a.xcap - 4));
        } else {
            float e[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = a.x[min(max(c + r, (int64_t)0), (int64_t)a.xcap - 1)];
            xx[u].x = e[0]; xx[u].y = e[1]; xx[u].z = e[2]; xx[u].w = e[3];
        }
    }
#pragma unroll
    for (int u = 0; u < DB; ++u) {
        if (EXACT || d0 + u < nd) {
            const double t0 = add_in_order(s[0], (double)v[u].x * (double)xx[u].x), t1 = add_in_order(s[1], (double)v[u].y * (double)xx[u].y);
            const double t2 = add_in_order(s[2], (double)v[u].z * (double)xx[u].z), t3 = add_in_order(s[3], (double)v[u].w * (double)xx[u].w);
            s[0] = __float_as_uint(v[u].x) != KR32_DIA_ABSENT ? t0 : s[0];
            s[1] = __float_as_uint(v[u].y) != KR32_DIA_ABSENT ? t1 : s[1];
            s[2] = __float_as_uint(v[u].z) != KR32_DIA_ABSENT ? t2 : s[2];
            s[3] = __float_as_uint(v[u].w) != KR32_DIA_ABSENT ? t3 : s[3];
        }
    }
}

// a capped grid that strides over the tiles in natural order
template <int NQ, int DB, bool EXACT, bool NT>
__global__ __launch_bounds__(KR32_T) void spmv32_dia_kernel(const Spmv32DiaArgs a) {
    static_assert(NQ == 0 || NQ == 1, "NQ");
    if (a.done && *a.done) return;
    __shared__ double red[KR32_T / 64];
    const int t = threadIdx.x;
    const int nd = a.nd;
    for (int q = blockIdx.x; q < a.ntiles; q += gridDim.x) {
        const int r0 = q * KR32_TILE;
        const int row = r0 + 4 * t;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (r0 + a.dia_min >= 0) {                                 // uniform over the workgroup
            for (int d0 = 0; d0 < (EXACT ? 1 : nd); d0 += DB) dia32_batch<DB, EXACT, true, NT>(a, row, d0, nd, s);
        } else {                                                   // the lowest diagonal would start before x[0]
            for (int d0 = 0; d0 < (EXACT ? 1 : nd); d0 += DB) dia32_batch<DB, EXACT, false, NT>(a, row, d0, nd, s);
        }
        quad_finish<NQ>(s, a.y, a.dvec, a.partials, q, row, a.nrows, red);
    }
}

int32_t enqueue_spmv32_dia(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nt = ntiles32_of(a->nrows);
    Spmv32DiaArgs g{a->d_dia, x, y, dvec, ctx->d_partials, done, a->dia_stride, (int32_t)a->nrows, (int32_t)nt, a->dia_nd, a->dia_min,
                    (int32_t)vec32_len(a->ncols), {0}};
    for (int d = 0; d < KR_DIA_MAX; ++d) g.off[d] = a->dia_off[d];
    // No LDS beyond the reduction scratch, so the grid cap is this kernel's own: 4 workgroups per compute unit (launch_spmv32's knob,
    // KRYST_SPMV32_BLOCKS_PER_CU, with another default), nontemporal value loads (KRYST_SPMV32_DIA_NT).  In-process A/B (tools/mixed_bench.py
    // dspmv, profiles/mixed/dia_*.jsonl; windows >= 0.5 s alternated, medians), variable coefficients, 7 diagonals, 256^3 | 512^3:
    //   1 / 2 / 4 workgroups per CU   0.1528 / 0.1050 / 0.0993 ms | 1.256 / 0.957 / 0.966 ms   (4 against 2: +5.8 % | -0.9 %; the Poisson operator +9.3 % | +0.2 %)
    //   plain / nontemporal loads     0.1124 / 0.0993 ms          | 1.000 / 0.966 ms           (nontemporal: +13 % | +3.5 %; Poisson +13 % | +3.1 %)
    // (an earlier run with 2 per CU as the default, dia_*_bpc2.jsonl: 4 against 2 +4.4 % | -0.6 %, nontemporal +9.5 % | -0.9 %)
    const int bpc = std::max(1, std::min(8, env_int("KRYST_SPMV32_BLOCKS_PER_CU", 4)));
    const bool nontemporal = env_int("KRYST_SPMV32_DIA_NT", 1) != 0;
    const dim3 grid((unsigned)std::min<int64_t>(nt, (int64_t)ctx->num_cu * bpc)), block(KR32_T);
    hipStream_t s = ctx->s_main;
    // exactly 3 / 5 / 7 / 9 diagonals: one batch with compile-time indices; else batches of 4 (fewer than 7 diagonals) or 8
    const int nd = a->dia_nd, exact = nd == 3 || nd == 5 || nd == 7 || nd == 9 ? nd : 0;
    by_bool(nq != 0, [&](auto Q) { by_bool(nontemporal, [&](auto NT) {
        constexpr int NQ = Q() ? 1 : 0;
        if (!by_int<3, 5, 7, 9>(exact, [&](auto DB) { hipLaunchKernelGGL((spmv32_dia_kernel<NQ, DB(), true, NT()>), grid, block, 0, s, g); }))
            by_int<4, 8>(nd < 7 ? 4 : 8, [&](auto DB) { hipLaunchKernelGGL((spmv32_dia_kernel<NQ, DB(), false, NT()>), grid, block, 0, s, g); });
    }); });
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- the lowering of the streams
// dst[d * dstride + i] = (float)src[d * sstride + i] for a present entry of a row below nrows -- lower_values_kernel's rounding -- and the fp32
// marker for an absent one and for all padding.  *refused counts present entries (NaNs with one particular payload) that round onto the marker.
__global__ void lower_dia_kernel(float* dst, int64_t dstride, const double* src, int64_t sstride, int nd, int64_t nrows, unsigned long long* refused) {
    unsigned long long mine = 0;
    const int64_t count = dstride * nd;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = k / dstride, i = k - d * dstride;
        float f = __uint_as_float(KR32_DIA_ABSENT);
        if (i < nrows) {
            const double v = src[d * sstride + i];
            if ((unsigned long long)__double_as_longlong(v) != KR_DIA_ABSENT) {
                f = (float)v;
                if (__float_as_uint(f) == KR32_DIA_ABSENT) ++mine;
            }
        }
        dst[k] = f;
    }
    if (mine) atomicAdd(refused, mine);
}

// the operator must hold CSR-DIA streams (csr_create.hip: build_dia, at creation only); the pattern form's rule for the offsets
const char* lower_dia_refusal(kryst_csr_t a) {
    if (!(a->d_dia && a->dia_nd > 0 && a->dia_nd <= KR_DIA_MAX)) return "the operator has no CSR-DIA form";
    return offsets_fit32(a) ? nullptr : "the vectors do not fit 32-bit byte offsets";
}

hipError_t enqueue_lower_dia(kryst_csr_t a, kryst_csr32_t m, unsigned long long* d_refused) {
    m->dia_stride = vec32_len(a->nrows); m->dia_nd = a->dia_nd; m->dia_min = a->dia_min; m->dia_max = a->dia_max;
    for (int d = 0; d < KR_DIA_MAX; ++d) m->dia_off[d] = a->dia_off[d];
    const int64_t count = m->dia_stride * m->dia_nd;
    const hipError_t e = hipMalloc(&m->d_dia, sizeof(float) * (size_t)count);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lower_dia_kernel, dim3(grid_for(count)), dim3(256), 0, a->ctx->s_main, m->d_dia, m->dia_stride, a->d_dia, a->dia_stride, m->dia_nd, a->nrows, d_refused);
    return hipGetLastError();
}

}  // namespace kr
