// Mixed precision: the SpMV of a lowered operator -- the kernel on the plain arrays (spmv32_wave_kernel), the choice
// between it and the kernels of the forms (spmv32_kernel: the ONE place that decides) and the launch.
#include "mixed.h"

namespace kr {

typedef int32_t p_v4i __attribute__((ext_vector_type(4)));

// The plain wave kernel's shape at the fp32 tile: a workgroup owns 1024-row tiles, thread t rows 4t .. 4t+3, so a wave owns 256 consecutive
// rows.  Phase 1: the wave streams the (col, val) run of its rows into a private LDS window of 2048 entries with 16-byte loads (4 entries per
// lane and load, all loads of the window in flight at once), ordered by wave barriers only.  The window starts at the wave's first entry rounded
// DOWN to a multiple of 4, so every load is 16-byte aligned whatever the residue of the row start; the arrays carry 8 entries of zero padding, so
// the last quad may reach past nnz.  Phase 2: the lane walks its four rows in ascending stored order, U entries of each in flight, and folds
// (double)val * (double)x[col] from 0.0 with separate multiply and add (sparse.rs:107-113 on widened operands).  Rows longer than a window
// loop over windows; an empty row stores +0.0.
// build-time knobs of the measurements in DESIGN.md section 4.16 (make EXTRA=-DKR32_SPMV_SLOTS=4): entries of each row in flight, window slots
#ifndef KR32_SPMV_U
#define KR32_SPMV_U 2
#endif
#ifndef KR32_SPMV_SLOTS
#define KR32_SPMV_SLOTS 8
#endif
// the wave's LDS window changes hands between its lanes: ordered by a wave barrier, no workgroup barrier
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
struct Spmv32Args {
    const int32_t* row_ptr; const int32_t* col; const float* val;
    const float* x; float* y; const float* dvec; double* partials;
    int nrows; int ntiles; const int* done;
};

template <int NQ>
__global__ __launch_bounds__(KR32_T) void spmv32_wave_kernel(const Spmv32Args a) {
    static_assert(NQ == 0 || NQ == 1, "NQ");
    if (a.done && *a.done) return;
    constexpr int SLOTS = KR32_SPMV_SLOTS;
    constexpr int WCAP = SLOTS * 256;                       // entries per wave window
    constexpr int U = KR32_SPMV_U;                          // entries of each of the lane's 4 rows in flight
    __shared__ __attribute__((aligned(16))) float val_all[4 * WCAP];
    __shared__ __attribute__((aligned(16))) int32_t col_all[4 * WCAP];
    __shared__ double red[KR32_T / 64];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    float* lval = val_all + w * WCAP;
    int32_t* lcol = col_all + w * WCAP;
    for (int q = blockIdx.x; q < a.ntiles; q += gridDim.x) {
        const int r0 = q * KR32_TILE;
        const int r1 = min(r0 + KR32_TILE, a.nrows);
        const int wr0 = min(r0 + 256 * w, r1), wr1 = min(wr0 + 256, r1);
        const int row = r0 + 4 * t;
        int p[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) p[e] = a.row_ptr[min(row + e, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int base = k0 & ~3; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            const int nquads = (wend - base + 3) >> 2;
            // ---- phase 1
            p_v4f v[SLOTS]; p_v4i c[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int qi = min(l + j * 64, nquads - 1);
                const int k = base + 4 * qi;
                v[j] = *reinterpret_cast<const p_v4f*>(a.val + k);
                c[j] = *reinterpret_cast<const p_v4i*>(a.col + k);
            }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                *reinterpret_cast<p_v4f*>(&lval[4 * (l + j * 64)]) = v[j];
                *reinterpret_cast<p_v4i*>(&lcol[4 * (l + j * 64)]) = c[j];
            }
            wave_sync();
            // ---- phase 2
            int k[4], e[4];
            bool more = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) { k[r] = max(p[r], base); e[r] = min(p[r + 1], wend); more = more || k[r] < e[r]; }
            while (more) {
                float vv[4][U], xx[4][U];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = min(k[r] + u, max(e[r] - 1, base)) - base;      // always inside the window
                        const int cc = lcol[idx];
                        vv[r][u] = lval[idx];
                        xx[r][u] = (k[r] + u < e[r]) ? a.x[cc] : 0.0f;
                    }
                }
                more = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (k[r] + u < e[r]) s[r] = s[r] + (double)vv[r][u] * (double)xx[r][u];
                    }
                    k[r] += U;
                    more = more || k[r] < e[r];
                }
            }
            wave_sync();
        }
        quad_finish<NQ>(s, a.y, a.dvec, a.partials, q, row, a.nrows, red);    // (every row of tile q lies below r0 + 1024: r1 and nrows bound the same rows)
    }
}

static int32_t enqueue_spmv32_plain(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nt = ntiles32_of(a->nrows);
    const Spmv32Args args{a->d_row_ptr, a->d_col, a->d_val, x, y, dvec, ctx->d_partials, (int)a->nrows, (int)nt, done};
    // LDS: 64 KiB per workgroup (two fit a compute unit); a capped grid that strides the tiles, like the other streaming kernels.  Measured at 256^3,
    // 7-point: windows of 512 / 1024 / 2048 entries per wave 0.50 / 0.43 / 0.38 ms -- the fewer trips through the window loop the better
    const int bpc = std::max(1, std::min(8, env_int("KRYST_SPMV32_BLOCKS_PER_CU", 2)));
    const int64_t grid = std::min<int64_t>(nt, (int64_t)ctx->num_cu * bpc);
    by_bool(nq != 0, [&](auto Q) { hipLaunchKernelGGL((spmv32_wave_kernel<Q() ? 1 : 0>), dim3((unsigned)grid), dim3(KR32_T), 0, ctx->s_main, args); });
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// KRYST_SPMV32_FORM = plain | pattern | dia: -1 unset (or no such word), 0 plain, 1 pattern, 2 dia; read as env_int reads a number (once per EnvFreeze)
static int spmv32_form_knob() {
    static EnvSlot slot;
    return (int)env_parsed_cached(slot, "KRYST_SPMV32_FORM", -1, [](const char* v) -> long long { return !strcmp(v, "plain") ? 0 : !strcmp(v, "pattern") ? 1 : !strcmp(v, "dia") ? 2 : -1; });
}

// the choice: the diagonal streams, else pattern-stage, then pattern, then plain, from the form the lowered operator holds and the two settings
// (a lowered operator holds the diagonal form or the row-pattern form, never both; `pattern` and `dia` both mean "the form held")
Spmv32Kernel spmv32_kernel(kryst_csr32_t a) {
    if (spmv32_form_knob() == 0) return Spmv32Kernel::Plain;
    if (a->d_dia) return Spmv32Kernel::Dia;
    if (!a->d_pid) return Spmv32Kernel::Plain;
    const bool stage = a->pat_stage_n > 0 && a->pat_stage_n % 4 == 0 && a->pat_far_uniform && env_int("KRYST_SPMV32_STAGE", 1) != 0;
    return stage ? Spmv32Kernel::PatternStage : Spmv32Kernel::Pattern;
}

int32_t launch_spmv32(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    if (ntiles32_of(a->nrows) <= 0) return KRYST_OK;
    if (nq) KR_TRY(ensure_partials(a->ctx, ntiles32_of(a->nrows)));
    switch (spmv32_kernel(a)) {
        case Spmv32Kernel::Plain: KR_TRY(enqueue_spmv32_plain(a, x, y, nq, dvec, done)); break;
        case Spmv32Kernel::Pattern: KR_TRY(enqueue_spmv32_pattern(a, x, y, nq, dvec, done)); break;
        case Spmv32Kernel::PatternStage: KR_TRY(enqueue_spmv32_pattern_stage(a, x, y, nq, dvec, done)); break;
        case Spmv32Kernel::Dia: KR_TRY(enqueue_spmv32_dia(a, x, y, nq, dvec, done)); break;
    }
    phase_mark(a->ctx, KR_PH_SPMV);
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_csr32_encoding(kryst_csr32_t a, int32_t* kernel) {
    KR_TRY(csr32_check(a));
    KR_ARG(kernel, "csr32_encoding");
    *kernel = (int32_t)spmv32_kernel(a);
    return KRYST_OK;
}

int32_t kryst_spmv32(kryst_csr32_t a, kryst_vec32_t x, kryst_vec32_t y) {
    KR_TRY(csr32_check(a)); KR_TRY(vec32_check(x)); KR_TRY(vec32_check(y));
    KR_ARG(x->ctx == a->ctx && y->ctx == a->ctx, "spmv32: context mismatch");
    KR_ARG(x->n == a->ncols, "spmv32: x.len() != ncols");
    KR_ARG(y->n == a->nrows, "spmv32: y.len() != nrows");
    KR_ARG(x->d != y->d, "spmv32: x and y alias");
    KR_HIP(hipSetDevice(a->ctx->device));
    return launch_spmv32(a, x->d, y->d, 0, nullptr, nullptr);
}

}  // extern "C"
