// Mixed precision: fp32-stored vectors and operator, CG / Jacobi-PCG on them, and fp64 iterative refinement around them.
//
// The arithmetic contract -- a LABELLED DEVIATION from the reference's CgSolver<f32>, which would round every operation: fp32 is how numbers are
// STORED.  A kernel widens what it loads (exact), computes in fp64 in the fixed order of its fp64 twin with separate multiply and add, and rounds
// once, (float) = round to nearest even with fp32 subnormals kept, when it stores.  An inner-product term (double)a * (double)b is exact; the fold
// is the published tree at T = 256, V = 4 (kryst_reduce_spec32): the thread's 4 terms in index order from 0.0, the 64-lane xor butterfly, the 4
// waves serially -> one partial per 1024-element tile, then fold2 and the logic structs of cg_logic.h, unchanged.
#include "mixed.h"
#include "cg_logic.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace kr {

typedef float kr_v4f __attribute__((ext_vector_type(4)));
typedef int32_t kr_v4i __attribute__((ext_vector_type(4)));

struct f4 { float v[4]; };
__device__ __forceinline__ f4 ld4(const float* p, int64_t i) {
    const kr_v4f q = *reinterpret_cast<const kr_v4f*>(p + i);
    return {{q.x, q.y, q.z, q.w}};
}
// one 16-byte store; elements at or behind n are stored as +0.0 (the padding of a work vector stays zero)
__device__ __forceinline__ void st4(float* p, int64_t i, int64_t n, const f4& o) {
    kr_v4f q;
    q.x = i < n ? o.v[0] : 0.0f; q.y = i + 1 < n ? o.v[1] : 0.0f; q.z = i + 2 < n ? o.v[2] : 0.0f; q.w = i + 3 < n ? o.v[3] : 0.0f;
    *reinterpret_cast<kr_v4f*>(p + i) = q;
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }

// ---------------------------------------------------------------------------------------------------- conversions
// dst[i] = (float)src[i], or (float)(src[i] / den) when `divide` is set (refinement: r32 = (float)(r / rho))
__global__ void round_kernel(float* dst, const double* src, int64_t n, int divide, double den) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = divide ? (float)(src[i] / den) : (float)src[i];
}
__global__ void widen_kernel(double* dst, const float* src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}
// refinement: xn = x + rho * (double)c
__global__ void correct_kernel(double* xn, const double* x, const float* c, double rho, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) xn[i] = x[i] + rho * (double)c[i];
}

// the verdict of one rounding, shared by the device pass and its host twin (kryst_host_round_f32)
__host__ __device__ __forceinline__ float round_count(double v, unsigned long long (&cnt)[3]) {
    const float f = (float)v;
    const float af = f < 0.0f ? -f : f;
    if (v == v) {                                                     // (a NaN stays a NaN and counts as nothing)
        if ((double)f != v) ++cnt[0];                                 // changed by the rounding
        if (v != 0.0 && af < FLT_MIN) ++cnt[1];                       // became zero or fp32-subnormal
        const double av = v < 0.0 ? -v : v;
        if (av <= DBL_MAX && af > FLT_MAX) ++cnt[2];                  // a finite value that rounds to +-inf
    }
    return f;
}
__global__ void lower_values_kernel(float* dst, const double* src, int64_t n, unsigned long long* count) {
    unsigned long long cnt[3] = {0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = round_count(src[i], cnt);
    for (int k = 0; k < 3; ++k) { if (cnt[k]) atomicAdd(count + k, cnt[k]); }
}
// elements [n, cap): count those whose bits are not +0.0, then (fill) overwrite them.  One workgroup.
__global__ void vec32_padding_kernel(float* d, int64_t n, int64_t cap, int fill, float value, unsigned long long* count) {
    unsigned long long mine = 0;
    for (int64_t e = n + threadIdx.x; e < cap; e += blockDim.x) {
        if (__float_as_uint(d[e]) != 0u) ++mine;
        if (fill) d[e] = value;
    }
    if (mine) atomicAdd(count, mine);
}

// ---------------------------------------------------------------------------------------------------- pointwise passes
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

// ---------------------------------------------------------------------------------------------------- SpMV
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
            kr_v4f v[SLOTS]; kr_v4i c[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int qi = min(l + j * 64, nquads - 1);
                const int k = base + 4 * qi;
                v[j] = *reinterpret_cast<const kr_v4f*>(a.val + k);
                c[j] = *reinterpret_cast<const kr_v4i*>(a.col + k);
            }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                *reinterpret_cast<kr_v4f*>(&lval[4 * (l + j * 64)]) = v[j];
                *reinterpret_cast<kr_v4i*>(&lcol[4 * (l + j * 64)]) = c[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        f4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.v[r] = (float)s[r];
        if (row + 3 < r1) {
            kr_v4f ov; ov.x = o.v[0]; ov.y = o.v[1]; ov.z = o.v[2]; ov.w = o.v[3];
            *reinterpret_cast<kr_v4f*>(a.y + row) = ov;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) { if (row + r < r1) a.y[row + r] = o.v[r]; }
        }
        if constexpr (NQ > 0) {
            // (d, y) with y as stored: the lane's four products in index order, the butterfly, the 4 waves
            const f4 dd = ld4(a.dvec, row);                         // (rows behind n lie in the padding: read, never used)
            double acc[1] = {0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) { if (row + r < r1) acc[0] = acc[0] + (double)dd.v[r] * (double)o.v[r]; }
            block_reduce<1, KR32_T / 64>(acc, red);
            if (t == 0) a.partials[q] = acc[0];
        }
    }
}

// KRYST_SPMV32_FORM = plain | pattern | dia: -1 unset (or no such word), 0 plain, 1 pattern, 2 dia.  Read as env_int reads a number: at every launch outside a
// solve, once per solve inside one (EnvFreeze)
static int spmv32_form_knob() {
    static EnvSlot slot;
    auto parse = [](const char* v) -> long long { return !v ? -1 : !strcmp(v, "plain") ? 0 : !strcmp(v, "pattern") ? 1 : !strcmp(v, "dia") ? 2 : -1; };
    if (g_env_frozen > 0) {
        const uint32_t e = g_env_epoch.load(std::memory_order_relaxed);
        if (slot.epoch.load(std::memory_order_acquire) == e) return (int)slot.val.load(std::memory_order_relaxed);
        const long long v = parse(getenv("KRYST_SPMV32_FORM"));
        slot.has.store(1, std::memory_order_relaxed); slot.val.store(v, std::memory_order_relaxed);
        slot.epoch.store(e, std::memory_order_release);
        return (int)v;
    }
    return (int)parse(getenv("KRYST_SPMV32_FORM"));
}

// the choice: the diagonal streams, else pattern-stage, then pattern, then plain, from the form the lowered operator holds and the two settings
// (a lowered operator holds the diagonal form or the row-pattern form, never both; `pattern` and `dia` both mean "the form held")
int spmv32_kernel(kryst_csr32_t a) {
    if (spmv32_form_knob() == 0) return 0;
    if (a->d_dia) return 3;
    if (!a->d_pid) return 0;
    const bool stage = a->pat_stage_n > 0 && a->pat_stage_n % 4 == 0 && a->pat_far_uniform && env_int("KRYST_SPMV32_STAGE", 1) != 0;
    return stage ? 2 : 1;
}

int32_t launch_spmv32(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nt = ntiles32_of(a->nrows);
    if (nt <= 0) return KRYST_OK;
    if (nq) KR_TRY(ensure_partials(ctx, nt));
    if (const int kernel = spmv32_kernel(a)) {
        KR_TRY(kernel == 3 ? enqueue_spmv32_dia(a, x, y, nq, dvec, done)
               : kernel == 2 ? enqueue_spmv32_pattern_stage(a, x, y, nq, dvec, done) : enqueue_spmv32_pattern(a, x, y, nq, dvec, done));
        phase_mark(ctx, KR_PH_SPMV);
        return KRYST_OK;
    }
    const Spmv32Args args{a->d_row_ptr, a->d_col, a->d_val, x, y, dvec, ctx->d_partials, (int)a->nrows, (int)nt, done};
    // LDS: 64 KiB per workgroup (two fit a compute unit); a capped grid that strides the tiles, like the other streaming kernels.  Measured at 256^3,
    // 7-point: windows of 512 / 1024 / 2048 entries per wave 0.50 / 0.43 / 0.38 ms -- the fewer trips through the window loop the better
    const int bpc = std::max(1, std::min(8, env_int("KRYST_SPMV32_BLOCKS_PER_CU", 2)));
    const int64_t grid = std::min<int64_t>(nt, (int64_t)ctx->num_cu * bpc);
    if (nq) hipLaunchKernelGGL((spmv32_wave_kernel<1>), dim3((unsigned)grid), dim3(KR32_T), 0, ctx->s_main, args);
    else hipLaunchKernelGGL((spmv32_wave_kernel<0>), dim3((unsigned)grid), dim3(KR32_T), 0, ctx->s_main, args);
    KR_HIP(hipGetLastError());
    phase_mark(ctx, KR_PH_SPMV);
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- handles
static int32_t vec32_check(kryst_vec32_t v) {
    KR_ARG(v && v->d && v->ctx, "vec32: null handle");
    return KRYST_OK;
}
static int32_t csr32_check(kryst_csr32_t a) {
    KR_ARG(a && a->ctx && a->d_row_ptr, "csr32: null handle");
    return KRYST_OK;
}
static int32_t vec32_alloc(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out) {
    kryst_vec32_t v = new kryst_vec32_s();
    v->ctx = ctx; v->n = n;
    const size_t bytes = sizeof(float) * (size_t)vec32_len(n);
    if (hipMalloc(&v->d, bytes) != hipSuccess) { (void)hipGetLastError(); delete v; set_error("hipMalloc(%zu) failed", bytes); return KRYST_ERR_HIP; }
    if (hipMemsetAsync(v->d, 0, bytes, ctx->s_main) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(v->d); delete v; set_error("hipMemsetAsync failed"); return KRYST_ERR_HIP; }
    *out = v;
    return KRYST_OK;
}
static void vec32_free(kryst_vec32_t v) {
    if (!v) return;
    (void)hipStreamSynchronize(v->ctx->s_main);
    (void)hipFree(v->d);
    delete v;
}
static void csr32_free(kryst_csr32_t a) {
    if (!a) return;
    (void)hipStreamSynchronize(a->ctx->s_main);
    (void)hipFree(a->d_row_ptr); (void)hipFree(a->d_col); (void)hipFree(a->d_val);
    (void)hipFree(a->d_pid); (void)hipFree(a->d_pmeta); (void)hipFree(a->d_poff); (void)hipFree(a->d_pval);
    (void)hipFree(a->d_dia);
    delete a;
}

// ---------------------------------------------------------------------------------------------------- CG / PCG on fp32 storage
struct Solve32IO {
    kryst_pc_t pc; const kryst_params_t* params; kryst_stats_t* stats; double* hist; int64_t hist_cap; int64_t* hist_len;
};

// what is refused before anything is launched or written
static int32_t solve32_check(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg) {
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

static int32_t solve32(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg) {
    KR_TRY(solve32_check(b, x, a, io, pcg));
    const EnvFreeze knobs;
    kryst_ctx_t ctx = a->ctx;
    const kryst_params_t prm = *io.params;
    const int64_t n = a->nrows, nt = ntiles32_of(n);
    KR_HIP(hipSetDevice(ctx->device));
    // a Workspace vector of this length is exactly one fp32 vector: 8 * (len / 2) bytes
    Workspace ws(ctx, vec32_len(n) / 2 - KR_TILE);
    KR_TRY(ws.init(prm.max_iters + 2));
    if (ws.vec_bytes() < sizeof(float) * (size_t)vec32_len(n)) { set_error("solve32: a work vector is smaller than an fp32 vector"); return KRYST_ERR_HIP; }
    const bool jac = pcg && io.pc && io.pc->kind == KR_PC_JACOBI;
    KR_TRY(ws.reserve(jac ? 6 : 4));                                        // xw, r, p, ap [, z, dinv]
    const LogicCtx lc = ws.lctx(&prm);
    const int* done = &ws.st->done;
    const DevState* st = ws.st;
    double* raw[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < (jac ? 6 : 4); ++k) KR_TRY(ws.vec(&raw[k]));
    float* xw = reinterpret_cast<float*>(raw[0]); float* r = reinterpret_cast<float*>(raw[1]);
    float* p = reinterpret_cast<float*>(raw[2]); float* ap = reinterpret_cast<float*>(raw[3]);
    float* z = jac ? reinterpret_cast<float*>(raw[4]) : r;                  // z == r (pcg.rs:130,186 / IdentityPC)
    float* dinv = jac ? reinterpret_cast<float*>(raw[5]) : nullptr;
    if (n > 0) KR_HIP(hipMemcpyAsync(xw, x->d, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, ctx->s_main));
    if (jac && n > 0) {                                                     // the Jacobi values, rounded once per solve
        hipLaunchKernelGGL(round_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->s_main, dinv, pc_jacobi_inv_diag(io.pc), n, 0, 1.0);
        KR_HIP(hipGetLastError());
    }
    KR_TRY(launch_spmv32(a, xw, ap, 0, nullptr, nullptr));                  // cg.rs:120-122, pcg.rs:119-121
    if (!pcg) {
        KR_TRY(launch_ew32(ctx, CgInit32Op{b->d, ap, r, p}, n, nullptr));
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgInitLogic{lc})));
    } else {
        if (jac) KR_TRY(launch_ew32(ctx, PcgInit32Op<true>{b->d, ap, r, z, p, dinv, prm.norm_type}, n, nullptr));
        else KR_TRY(launch_ew32(ctx, PcgInit32Op<false>{b->d, ap, r, z, p, nullptr, prm.norm_type}, n, nullptr));
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
            if (jac) KR_TRY(launch_ew32(ctx, PcgUpdate32Op<true>{st, p, ap, xw, r, z, dinv, prm.norm_type}, n, done, KR_PH_BLAS1_RESIDUAL));
            else KR_TRY(launch_ew32(ctx, PcgUpdate32Op<false>{st, p, ap, xw, r, z, nullptr, prm.norm_type}, n, done, KR_PH_BLAS1_RESIDUAL));
            KR_TRY((reduce_then<2>(ctx, nt, ws.red, PcgBetaLogic{lc})));
        }
        return launch_ew32(ctx, Direction32Op{st, z, p}, n, done, KR_PH_BLAS1_DIRECTION);
    };
    KR_TRY(run_ahead(ctx, &prm, iterate));
    DevState h;
    KR_HIP(read_state(ws, &h));
    if (io.stats) { io.stats->iterations = h.iterations; io.stats->final_residual = h.final_residual; io.stats->converged = h.converged; }
    if (io.hist_len) *io.hist_len = h.hist_len;
    for (int64_t k = 0; k < h.hist_len && k < ws.hist_cap; ++k) { if (io.hist && k < io.hist_cap) io.hist[k] = ws.h_hist[k]; }
    if (pcg && io.pc && pc_health(io.pc) != KRYST_OK) return KRYST_SOLVE_ERROR;
    if (h.status == KRYST_ERR_HIP && fold_gave_up(ctx)) return h.status;
    if (h.status == KRYST_OK && n > 0)                                      // on Err the reference never reaches `*x = ...`
        KR_HIP(hipMemcpyAsync(x->d, xw, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return h.status;
}

// ---------------------------------------------------------------------------------------------------- fp64 iterative refinement
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
    kryst_ctx_t ctx = a->ctx;
    KR_TRY(residual_dot(a, b, x, r, tmp, nullptr));
    double* slot = ctx->d_scal + 1024;                                      // kryst_dot's result slot: outside the scalar state of a solve
    KR_TRY(launch_final_fold(ctx, 1, ntiles_of(a->nrows), slot));
    KR_HIP(hipMemcpyAsync(ctx->h_pinned, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    const double rr = ctx->h_pinned[0];
    if (rr != rr && fold_gave_up(ctx)) return KRYST_ERR_HIP;
    *rho = __builtin_sqrt(rr);
    return KRYST_OK;
}

static int32_t refine_solve(kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_csr32_t a32, kryst_pc_t pc, const kryst_params_t* outer,
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
            hipLaunchKernelGGL(round_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->s_main, r32->d, r, n, 1, rho);
            KR_HIP(hipGetLastError());
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

}  // namespace kr

using namespace kr;

extern "C" {

void kryst_reduce_spec32(int32_t* T, int32_t* V, int32_t* F) {
    if (T) *T = KR32_T;
    if (V) *V = KR32_V;
    if (F) *F = KR_F;
}

int32_t kryst_host_round_f32(const double* v, int64_t n, float* out, int64_t info[2]) {
    KR_ARG(n >= 0 && (n == 0 || (v && out)), "host_round_f32");
    unsigned long long cnt[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i) out[i] = round_count(v[i], cnt);
    if (info) { info[0] = (int64_t)cnt[0]; info[1] = (int64_t)cnt[1]; }
    if (cnt[2]) { set_error("round_f32: %llu finite value(s) would round to +-inf in fp32", cnt[2]); return KRYST_UNSUPPORTED; }
    return KRYST_OK;
}

int32_t kryst_vec32_create(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out) {
    KR_ARG(ctx && out && n >= 0, "vec32_create");
    KR_HIP(hipSetDevice(ctx->device));
    return vec32_alloc(ctx, n, out);
}

int32_t kryst_vec32_destroy(kryst_vec32_t v) {
    if (!v) return KRYST_OK;
    (void)hipSetDevice(v->ctx->device);
    vec32_free(v);
    return KRYST_OK;
}

int32_t kryst_vec32_upload(kryst_vec32_t v, const float* host, int64_t n) {
    KR_TRY(vec32_check(v));
    KR_ARG(host || n == 0, "vec32_upload");
    KR_ARG(n == v->n, "vec32_upload: length mismatch");
    KR_HIP(hipSetDevice(v->ctx->device));
    if (n > 0) KR_HIP(hipMemcpyAsync(v->d, host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, v->ctx->s_main));
    KR_HIP(hipStreamSynchronize(v->ctx->s_main));
    return KRYST_OK;
}

int32_t kryst_vec32_download(kryst_vec32_t v, float* host, int64_t n) {
    KR_TRY(vec32_check(v));
    KR_ARG(host || n == 0, "vec32_download");
    KR_ARG(n == v->n, "vec32_download: length mismatch");
    KR_HIP(hipSetDevice(v->ctx->device));
    if (n > 0) KR_HIP(hipMemcpyAsync(host, v->d, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, v->ctx->s_main));
    KR_HIP(hipStreamSynchronize(v->ctx->s_main));
    return KRYST_OK;
}

int32_t kryst_bench_vec32_padding(kryst_vec32_t v, const float* fill, int64_t* dirty) {
    KR_TRY(vec32_check(v));
    kryst_ctx_t ctx = v->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    unsigned long long* d_count = nullptr;
    KR_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->s_main);
    unsigned long long count = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(vec32_padding_kernel, dim3(1), dim3(1024), 0, ctx->s_main, v->d, v->n, vec32_len(v->n), fill ? 1 : 0, fill ? *fill : 0.0f, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->s_main);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d_count);
    KR_HIP(e);
    if (dirty) *dirty = (int64_t)count;
    return KRYST_OK;
}

int32_t kryst_vec32_from_f64(kryst_vec32_t dst, kryst_vec_t src) {
    KR_TRY(vec32_check(dst));
    KR_ARG(src && src->ctx == dst->ctx, "vec32_from_f64: null vector or context mismatch");
    KR_ARG(src->n == dst->n, "vec32_from_f64: length mismatch");
    KR_HIP(hipSetDevice(dst->ctx->device));
    if (dst->n == 0) return KRYST_OK;
    hipLaunchKernelGGL(round_kernel, dim3(grid_for(dst->n)), dim3(256), 0, dst->ctx->s_main, dst->d, src->d, dst->n, 0, 1.0);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

int32_t kryst_vec32_to_f64(kryst_vec_t dst, kryst_vec32_t src) {
    KR_TRY(vec32_check(src));
    KR_ARG(dst && dst->ctx == src->ctx, "vec32_to_f64: null vector or context mismatch");
    KR_ARG(src->n == dst->n, "vec32_to_f64: length mismatch");
    KR_HIP(hipSetDevice(src->ctx->device));
    if (src->n == 0) return KRYST_OK;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(src->n)), dim3(256), 0, src->ctx->s_main, dst->d, src->d, src->n);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

int32_t kryst_dot32(kryst_vec32_t x, kryst_vec32_t y, double* out) {
    KR_TRY(vec32_check(x)); KR_TRY(vec32_check(y));
    KR_ARG(x->ctx == y->ctx, "dot32: vectors belong to different contexts");
    KR_ARG(x->n == y->n, "dot32: vector length mismatch");
    KR_ARG(out, "dot32: out");
    kryst_ctx_t ctx = x->ctx;
    if (ctx->nranks > 1) { set_error("dot32: distributed contexts are not supported"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(ctx->device));
    KR_TRY(launch_ew32(ctx, Dot32Op{x->d, y->d}, x->n, nullptr));
    double* slot = ctx->d_scal + 1024;                                      // kryst_dot's result slot
    KR_TRY(launch_final_fold(ctx, 1, ntiles32_of(x->n), slot));
    KR_HIP(hipMemcpyAsync(ctx->h_pinned, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    *out = ctx->h_pinned[0];
    if (*out != *out && fold_gave_up(ctx)) return KRYST_ERR_HIP;
    return KRYST_OK;
}

int32_t kryst_csr32_lower(kryst_csr_t a, kryst_csr32_t* out) { return kryst_csr32_lower_form(a, KRYST_CSR32_PLAIN, out); }

int32_t kryst_csr32_lower_form(kryst_csr_t a, int32_t form, kryst_csr32_t* out) {
    KR_ARG(a && out, "csr32_lower");
    KR_ARG(form == KRYST_CSR32_PLAIN || form == KRYST_CSR32_AUTO || form == KRYST_CSR32_PATTERN || form == KRYST_CSR32_DIA, "csr32_lower: unknown form");
    kryst_ctx_t ctx = a->ctx;
    if (a->dist || ctx->nranks > 1) { set_error("csr32_lower: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->d_row_ptr && a->d_col && a->d_val, "csr32_lower: the operator keeps no CSR arrays");
    KR_ARG(a->nrows < (1ll << 31) - KR32_TILE && a->nnz < (1ll << 31) - 4096, "csr32_lower: too many rows or entries");
    // the row-pattern form: the operator must have one, and the kernels address x and y with 32-bit byte offsets
    const bool has_p16 = a->d_pid && a->d_pmeta && a->d_poff && a->d_pval && a->npat > 0;
    const bool fits = vec32_len(std::max(a->nrows, a->ncols)) * (int64_t)sizeof(float) < (1ll << 31);
    if (form == KRYST_CSR32_PATTERN && !has_p16) { set_error("csr32_lower: the operator has no CSR-P16 form"); return KRYST_UNSUPPORTED; }
    if (form == KRYST_CSR32_PATTERN && !fits) { set_error("csr32_lower: the vectors do not fit 32-bit byte offsets"); return KRYST_UNSUPPORTED; }
    const bool pattern = (form == KRYST_CSR32_AUTO || form == KRYST_CSR32_PATTERN) && has_p16 && fits;
    // the diagonal form: the operator must hold CSR-DIA streams (csr_create.hip: build_dia, at creation only); the same rule for the offsets
    const bool dia = form == KRYST_CSR32_DIA;
    if (dia && !(a->d_dia && a->dia_nd > 0 && a->dia_nd <= KR_DIA_MAX)) { set_error("csr32_lower: the operator has no CSR-DIA form"); return KRYST_UNSUPPORTED; }
    if (dia && !fits) { set_error("csr32_lower: the vectors do not fit 32-bit byte offsets"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(ctx->device));
    kryst_csr32_t m = new kryst_csr32_s();
    m->ctx = ctx; m->nrows = a->nrows; m->ncols = a->ncols; m->nnz = a->nnz;
    unsigned long long* d_count = nullptr;
    unsigned long long cnt[4] = {0, 0, 0, 0};                                // lower_values_kernel's three, and the streams' refused entries
    const size_t ne = (size_t)a->nnz + 8;
    hipError_t e = hipMalloc(&m->d_row_ptr, sizeof(int32_t) * (size_t)(a->nrows + 1));
    if (e == hipSuccess) e = hipMalloc(&m->d_col, sizeof(int32_t) * ne);
    if (e == hipSuccess) e = hipMalloc(&m->d_val, sizeof(float) * ne);
    if (e == hipSuccess) e = hipMalloc(&d_count, sizeof cnt);
    if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, sizeof cnt, ctx->s_main);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_col, 0, sizeof(int32_t) * ne, ctx->s_main);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_val, 0, sizeof(float) * ne, ctx->s_main);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_row_ptr, a->d_row_ptr, sizeof(int32_t) * (size_t)(a->nrows + 1), hipMemcpyDeviceToDevice, ctx->s_main);
    if (e == hipSuccess && a->nnz > 0) e = hipMemcpyAsync(m->d_col, a->d_col, sizeof(int32_t) * (size_t)a->nnz, hipMemcpyDeviceToDevice, ctx->s_main);
    if (e == hipSuccess && a->nnz > 0) {
        hipLaunchKernelGGL(lower_values_kernel, dim3(grid_for(a->nnz)), dim3(256), 0, ctx->s_main, m->d_val, a->d_val, a->nnz, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess && pattern) {
        // ids re-padded to the fp32 tile (the fp64 array is padded to a 512-row tile only); the tables as they are, the values rounded as the CSR values are
        const size_t nid = (size_t)ntiles32_of(a->nrows) * KR32_TILE + KR32_TILE;
        e = hipMalloc(&m->d_pid, sizeof(uint16_t) * nid);
        if (e == hipSuccess) e = hipMalloc(&m->d_pmeta, sizeof(uint32_t) * 2 * (size_t)a->npat);
        if (e == hipSuccess) e = hipMalloc(&m->d_poff, sizeof(int32_t) * (size_t)std::max(a->ntab, 1));
        if (e == hipSuccess) e = hipMalloc(&m->d_pval, sizeof(float) * (size_t)std::max(a->ntab, 1));
        if (e == hipSuccess) e = hipMemsetAsync(m->d_pid, 0, sizeof(uint16_t) * nid, ctx->s_main);
        if (e == hipSuccess) e = hipMemcpyAsync(m->d_pid, a->d_pid, sizeof(uint16_t) * (size_t)a->nrows, hipMemcpyDeviceToDevice, ctx->s_main);
        if (e == hipSuccess) e = hipMemcpyAsync(m->d_pmeta, a->d_pmeta, sizeof(uint32_t) * 2 * (size_t)a->npat, hipMemcpyDeviceToDevice, ctx->s_main);
        if (e == hipSuccess && a->ntab > 0) e = hipMemcpyAsync(m->d_poff, a->d_poff, sizeof(int32_t) * (size_t)a->ntab, hipMemcpyDeviceToDevice, ctx->s_main);
        if (e == hipSuccess && a->ntab > 0) {
            hipLaunchKernelGGL(round_kernel, dim3(grid_for(a->ntab)), dim3(256), 0, ctx->s_main, m->d_pval, a->d_pval, (int64_t)a->ntab, 0, 1.0);
            e = hipGetLastError();
        }
        m->npat = a->npat; m->ntab = a->ntab; m->pat_unroll = a->pat_unroll; m->pat_single = a->pat_single;
        m->pat_stage_n = a->pat_stage_n; m->pat_far_lo = a->pat_far_lo; m->pat_far_hi = a->pat_far_hi; m->pat_far_uniform = a->pat_far_uniform;
    }
    if (e == hipSuccess && dia) {
        m->dia_stride = vec32_len(a->nrows); m->dia_nd = a->dia_nd; m->dia_min = a->dia_min; m->dia_max = a->dia_max;
        for (int d = 0; d < KR_DIA_MAX; ++d) m->dia_off[d] = a->dia_off[d];
        e = hipMalloc(&m->d_dia, sizeof(float) * (size_t)m->dia_stride * (size_t)m->dia_nd);
        if (e == hipSuccess) e = enqueue_lower_dia(a, m, d_count + 3);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost, ctx->s_main);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d_count);
    if (e != hipSuccess) { (void)hipGetLastError(); csr32_free(m); set_error("csr32_lower: %s", hipGetErrorString(e)); return KRYST_ERR_HIP; }
    if (cnt[2]) {
        csr32_free(m);
        set_error("csr32_lower: %llu finite value(s) would round to +-inf in fp32", cnt[2]);
        return KRYST_UNSUPPORTED;
    }
    if (cnt[3]) {
        csr32_free(m);
        set_error("csr32_lower: %llu stored NaN(s) round to the bits of the fp32 absent marker; the diagonal form is refused", cnt[3]);
        return KRYST_UNSUPPORTED;
    }
    m->changed = (int64_t)cnt[0]; m->tiny = (int64_t)cnt[1];
    *out = m;
    return KRYST_OK;
}

int32_t kryst_csr32_info(kryst_csr32_t a, int64_t info[3]) {
    KR_TRY(csr32_check(a));
    KR_ARG(info, "csr32_info");
    info[0] = a->changed; info[1] = a->tiny; info[2] = a->nrows;
    return KRYST_OK;
}

int32_t kryst_csr32_encoding(kryst_csr32_t a, int32_t* kernel) {
    KR_TRY(csr32_check(a));
    KR_ARG(kernel, "csr32_encoding");
    *kernel = spmv32_kernel(a);
    return KRYST_OK;
}

int32_t kryst_csr32_destroy(kryst_csr32_t a) {
    if (!a) return KRYST_OK;
    (void)hipSetDevice(a->ctx->device);
    csr32_free(a);
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

int32_t kryst_cg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats,
                             double* hist, int64_t hist_cap, int64_t* hist_len) {
    (void)pc;                                                               // cg.rs:115 `let _ = pc;`
    return solve32(b, x, a, Solve32IO{nullptr, params, stats, hist, hist_cap, hist_len}, false);
}

int32_t kryst_pcg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats,
                              double* hist, int64_t hist_cap, int64_t* hist_len) {
    return solve32(b, x, a, Solve32IO{pc, params, stats, hist, hist_cap, hist_len}, true);
}

int32_t kryst_refine_solve_dev(kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_csr32_t a32, kryst_pc_t pc, const kryst_params_t* outer,
                               const kryst_params_t* inner, kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len,
                               int64_t* inner_iters, int64_t inner_cap) {
    return refine_solve(b, x, a, a32, pc, outer, inner, stats, hist, hist_cap, hist_len, inner_iters, inner_cap);
}

}  // extern "C"
