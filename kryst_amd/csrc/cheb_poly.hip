// Chebyshev polynomial preconditioner with spectrum estimates -- a labelled EXTENSION: it stands beside the reference's stub
// (src/preconditioner/chebyshev.rs:35-70, whose apply returns Err) and beside its filter (chebyshev.rs:83-140, precond.hip), neither of
// which approximates A^-1.  The arithmetic is DESIGN.md section 4.15, operation by operation; tests/cheb_poly_ref.py restates it in numpy.
//
//   z = p_m(W A) W r   (Saad, Iterative Methods, Alg. 12.1 from z = 0; W = Jacobi's inv_diag or nothing), m SpMVs and pointwise passes only:
//   no dependency levels, no set-up beyond a diagonal, so a row-partitioned operator can use it.
//
// Two forms of the step, the same bits: cheb_poly_step_kernel walks the plain CSR arrays like spmv_wave_kernel and does the four vector
// updates in the owner lane of each row (y = A d never stored); the unfused form is launch_spmv of whatever encoding the operator has
// (halo exchange included) and ChebPolyStepOp (ew.h).  Which one runs is decided at creation from the operator alone.
#include "pc.h"
#include "ew.h"
#include "spmv_window.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace kr {

void tridiag_extreme_eigs(const double* alpha, const double* beta, int k, double* tmin, double* tmax);   // host_spectrum.cpp

struct ChebStepArgs {
    const int32_t* row_ptr; const int32_t* col; const double* val;
    const double* d_old; double* d_new; const double* rin; double* res; const double* w; double* z;
    double c1, c2;
    const int32_t* tiles; int32_t ntiles, nrows, xcd_chunk, swizzle, group, amask;
    const int* done;
};

// spmv_wave_kernel (spmv_stream.hip) with x = d_old and, in place of the y store, the step of ChebPolyStepOp on the two rows the lane owns:
// the row sums s0, s1 ARE y.  d_new is another buffer than d_old (other rows still gather it); res and z are touched by their owner only.
template <bool FIRST, bool LAST, bool SCALED, int SLOTS, bool NT>
__global__ __launch_bounds__(KR_T) void cheb_poly_step_kernel(const ChebStepArgs a) {
    if (a.done && *a.done) return;
    constexpr int WCAP = SLOTS * 128;                       // entries per wave window
    __shared__ __attribute__((aligned(16))) double prod_all[4 * WCAP];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    double* prod = prod_all + w * WCAP;
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    for (int li = slot0; li < a.xcd_chunk; li += per) {
        int ti;
        if (a.swizzle) ti = xcd * a.xcd_chunk + li;
        else ti = ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) { if (a.swizzle) break; else continue; }
        const int q = a.tiles ? a.tiles[ti] : ti;
        if (q < 0) continue;                                    // an empty slot of the slab order
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int wr0 = min(r0 + 128 * w, r1), wr1 = min(wr0 + 128, r1);
        const int row = r0 + 2 * t;
        const int p0 = a.row_ptr[min(row, r1)];
        const int p1 = a.row_ptr[min(row + 1, r1)];
        const int p2 = a.row_ptr[min(row + 2, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        for (int base = k0 & ~a.amask; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            const int npairs = (wend - base + 1) >> 1;
            v2i c[SLOTS]; v2d v[SLOTS]; double xa[SLOTS], xb[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int pi = min(l + j * 64, npairs - 1);
                const int k = base + 2 * pi;
                c[j] = stream_load<NT>(reinterpret_cast<const v2i*>(a.col + k));
                v[j] = stream_load<NT>(reinterpret_cast<const v2d*>(a.val + k));
            }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) { xa[j] = a.d_old[c[j].x]; xb[j] = a.d_old[c[j].y]; }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j)
                *reinterpret_cast<double2*>(&prod[2 * (l + j * 64)]) = make_double2(v[j].x * xa[j], v[j].y * xb[j]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            s0 = row_sum(prod, base, max(p0, base), min(p1, wend), s0);
            s1 = row_sum(prod, base, max(p1, base), min(p2, wend), s1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (row >= r1) continue;
        // (vectors are padded to whole tiles: the pair at `row` is addressable even when row + 1 == r1; its second half is then not stored)
        const d2 rp = ld2(FIRST ? a.rin : a.res, row), dd = ld2_keep(a.d_old, row);
        d2 zz = dd;
        if constexpr (!FIRST) zz = ld2(a.z, row);
        const double ra = rp.a - s0, rb = rp.b - s1;
        double ta = ra, tb = rb;
        if constexpr (SCALED) { const d2 ww = ld2_keep(a.w, row); ta = ww.a * ra; tb = ww.b * rb; }
        const double da = a.c1 * dd.a + a.c2 * ta, db = a.c1 * dd.b + a.c2 * tb;
        const double za = zz.a + da, zb = zz.b + db;
        if (row + 1 < r1) {
            if constexpr (!LAST) { st2(a.res, row, ra, rb); st2_keep(a.d_new, row, da, db); }
            st2(a.z, row, za, zb);
        } else {
            if constexpr (!LAST) { a.res[row] = ra; a.d_new[row] = da; }
            a.z[row] = za;
        }
    }
}

struct ChebPolyInitOp {              // d_0[i] = (w_i * r[i]) / theta; without scaling r[i] / theta
    static constexpr int NQ = 0; static constexpr const char* TAG = "ChebPolyInit";
    double theta; const double* w; const double* r; double* d;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        d2 v = ld2(r, i);
        if (w) { const d2 ww = ld2(w, i); v.a = ww.a * v.a; v.b = ww.b * v.b; }
        st2_keep(d, i, v.a / theta, v.b / theta);
    }
};

static inline int64_t padded(int64_t n) { return (n + KR_TILE - 1) / KR_TILE * KR_TILE; }
static int32_t alloc_vec(kryst_ctx_t ctx, double** p, int64_t n) {
    const size_t bytes = sizeof(double) * (size_t)(padded(n) + KR_TILE);
    KR_HIP(hipMalloc(p, bytes));
    KR_HIP(hipMemsetAsync(*p, 0, bytes, ctx->s_main));
    return KRYST_OK;
}

struct ChebPolyPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_CHEB_POLY;
    int32_t degree, scaling; double lo, hi; bool fused;
    double theta = 0.0, c1[65] = {0}, c2[65] = {0};
    double* d_res = nullptr; double* d_d[2] = {nullptr, nullptr}; double* d_w = nullptr;
    ChebPolyPc(kryst_csr_t a_, int32_t deg, int32_t sc, double lo_, double hi_, bool fused_)
        : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), degree(deg), scaling(sc), lo(lo_), hi(hi_), fused(fused_) {
        theta = (hi + lo) / 2.0;
        const double delta = (hi - lo) / 2.0;
        const double sigma = theta / delta;
        double rho = 1.0 / sigma;
        for (int k = 1; k <= degree; ++k) {
            const double rho_k = 1.0 / (2.0 * sigma - rho);
            c1[k] = rho_k * rho;
            c2[k] = (2.0 * rho_k) / delta;
            rho = rho_k;
        }
    }
    ~ChebPolyPc() override { (void)hipFree(d_res); (void)hipFree(d_d[0]); (void)hipFree(d_d[1]); (void)hipFree(d_w); }

    template <bool FIRST, bool LAST, bool SCALED>
    int32_t launch_fused(int k, const double* r, double* z, const int* done) {
        const PlainWavePlan p = plain_wave_plan(a);
        ChebStepArgs g;
        g.row_ptr = a->d_row_ptr; g.col = a->d_col; g.val = a->d_val;
        g.d_old = d_d[(k - 1) & 1]; g.d_new = d_d[k & 1]; g.rin = r; g.res = d_res; g.w = d_w; g.z = z;
        g.c1 = c1[k]; g.c2 = c2[k];
        g.tiles = p.tiles; g.ntiles = p.ntiles; g.nrows = (int32_t)a->nrows; g.xcd_chunk = p.xcd_chunk; g.swizzle = p.swizzle; g.group = p.group;
        g.amask = p.amask; g.done = done;
        const dim3 grid(p.grid), block(KR_T);
#define KR_CHEB(SL_) do { if (p.nt) hipLaunchKernelGGL((cheb_poly_step_kernel<FIRST, LAST, SCALED, SL_, true>), grid, block, 0, ctx->s_main, g); \
                          else hipLaunchKernelGGL((cheb_poly_step_kernel<FIRST, LAST, SCALED, SL_, false>), grid, block, 0, ctx->s_main, g); } while (0)
        if (p.slots <= 2) KR_CHEB(2); else if (p.slots <= 4) KR_CHEB(4); else KR_CHEB(7);
#undef KR_CHEB
        KR_HIP(hipGetLastError());
        return KRYST_OK;
    }
    template <bool FIRST, bool LAST, bool SCALED>
    int32_t step(int k, const double* r, double* z, const int* done) {
        if (fused) return launch_fused<FIRST, LAST, SCALED>(k, r, z, done);
        // d stays in d_d[0]; d_d[1] receives y = A d
        KR_TRY(launch_spmv(a, d_d[0], d_d[1], 0, nullptr, done));
        return launch_ew(ctx, ChebPolyStepOp<FIRST, LAST, SCALED>{c1[k], c2[k], d_d[1], d_w, r, d_res, d_d[0], z}, n, done);
    }
    template <bool SCALED>
    int32_t run(const double* r, double* z, const int* done) {
        if (degree == 0) return launch_ew(ctx, ChebPolyInitOp{theta, d_w, r, z}, n, done);
        KR_TRY(launch_ew(ctx, ChebPolyInitOp{theta, d_w, r, d_d[0]}, n, done));
        if (degree == 1) return step<true, true, SCALED>(1, r, z, done);
        KR_TRY((step<true, false, SCALED>(1, r, z, done)));
        for (int k = 2; k < degree; ++k) KR_TRY((step<false, false, SCALED>(k, r, z, done)));
        return step<false, true, SCALED>(degree, r, z, done);
    }
    int32_t apply(int64_t, const double* r, double* z, const int* done) override {
        if (n == 0) return KRYST_OK;
        return d_w ? run<true>(r, z, done) : run<false>(r, z, done);
    }
};

// ---------------------------------------------------------------- diagonal check, Gershgorin bound
// the lowest row whose w_i is not a finite positive number (a diagonal entry that is missing, zero, negative or not finite, or whose reciprocal overflows)
__global__ void cheb_check_w_kernel(const double* w, int32_t nrows, unsigned long long* bad_row) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const double v = w[i];
    if (!(v > 0.0 && v <= 1.7976931348623157e308)) atomicMin(bad_row, (unsigned long long)i);
}

// g = max_i((sum_k |a_ik|) * w_i), the row sum from 0.0 in stored order.  Every g_i is >= +0.0 or NaN, so the order of the bit patterns is
// the order of the values with NaN on top: the max fold is an integer max, exact in any order, and a NaN survives it.
__global__ void cheb_gershgorin_kernel(const int32_t* row_ptr, const double* val, const double* w, int32_t nrows, unsigned long long* out) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bits = 0ull;
    if (i < nrows) {
        double s = 0.0;
        for (int32_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) s = s + fabs(val[k]);
        if (w) s = s * w[i];
        bits = s != s ? 0x7FF8000000000000ull : (unsigned long long)__double_as_longlong(fabs(s));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(out, bits);
}

// Jacobi's inv_diag into a fresh vector, checked: KRYST_INDEFINITE_PRECONDITIONER with the row
static int32_t make_checked_w(kryst_csr_t a, double** out) {
    kryst_ctx_t ctx = a->ctx;
    double* w = nullptr;
    KR_TRY(alloc_vec(ctx, &w, a->nrows));
    int32_t rc = jacobi_inv_diag_dev(a, w);
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(dot_slot(ctx));   // kryst_dot's result slot: nothing is in flight between calls
    unsigned long long bad = ~0ull;
    if (rc == KRYST_OK && a->nrows > 0) {
        hipError_t e = hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, ctx->s_main);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(cheb_check_w_kernel, dim3((unsigned)((a->nrows + 255) / 256)), dim3(256), 0, ctx->s_main, w, (int32_t)a->nrows, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->s_main);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
        if (e != hipSuccess) { set_error("chebyshev_poly: checking the diagonal failed: %s", hipGetErrorString(e)); rc = KRYST_ERR_HIP; }
    }
    if (rc == KRYST_OK && bad != ~0ull) {
        const int64_t row = (int64_t)bad;          // (the only caller has refused a distributed operator: local rows are global rows)
        set_error("chebyshev_poly: Jacobi scaling needs a finite positive diagonal; row %lld has none", (long long)row);
        set_error_row(row);
        rc = KRYST_INDEFINITE_PRECONDITIONER;
    }
    if (rc != KRYST_OK) { (void)hipStreamSynchronize(ctx->s_main); (void)hipFree(w); return rc; }
    *out = w;
    return KRYST_OK;
}

// ---------------------------------------------------------------- Lanczos passes
struct SqrtOp {                      // out[i] = sqrt(x[i]), correctly rounded (solver_common.h: dsqrt)
    static constexpr int NQ = 0; static constexpr const char* TAG = "Sqrt";
    const double* x; double* out;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 a = ld2(x, i);
        st2(out, i, __builtin_sqrt(a.a), __builtin_sqrt(a.b));
    }
};
struct HadamardOp {                  // out[i] = a[i] * b[i]
    static constexpr int NQ = 0; static constexpr const char* TAG = "Hadamard";
    const double* a; const double* b; double* out;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 u = ld2(a, i), v = ld2(b, i);
        st2(out, i, u.a * v.a, u.b * v.b);
    }
};
struct DivScalarOp {                 // out[i] = x[i] / s
    static constexpr int NQ = 0; static constexpr const char* TAG = "DivScalar";
    double s; const double* x; double* out;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&)[1]) const {
        const d2 a = ld2(x, i);
        st2(out, i, in0 ? a.a / s : 0.0, in1 ? a.b / s : 0.0);       // padding stays zero
    }
};

struct LanczosVecs {
    kryst_vec_t v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double* s = nullptr; double* w = nullptr; kryst_ctx_t ctx = nullptr;
    ~LanczosVecs() {
        for (kryst_vec_t x : v) (void)kryst_vec_destroy(x);
        if (ctx) (void)hipStreamSynchronize(ctx->s_main);
        (void)hipFree(s); (void)hipFree(w);
    }
};

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_chebyshev_poly(kryst_csr_t a, int32_t degree, int32_t scaling, double lo, double hi, kryst_pc_t* out) {
    KR_ARG(a && out, "pc_chebyshev_poly");
    KR_ARG(a->nrows == a->xlen, "pc_chebyshev_poly: square operator required");
    KR_ARG(degree >= 0 && degree <= 64, "pc_chebyshev_poly: degree outside 0..64");
    KR_ARG(scaling == KRYST_CHEB_SCALE_NONE || scaling == KRYST_CHEB_SCALE_JACOBI, "pc_chebyshev_poly: scaling");
    KR_ARG(std::isfinite(lo) && std::isfinite(hi), "pc_chebyshev_poly: bounds must be finite");
    KR_ARG(lo > 0.0 && lo < hi, "pc_chebyshev_poly: 0 < lo < hi required");
    KR_HIP(hipSetDevice(a->ctx->device));
    // the fused step walks the plain CSR arrays: it is taken where the operator's own SpMV streams those too (no compressed form, one rank)
    int32_t enc = 0;
    KR_TRY(kryst_csr_encoding(a, &enc, nullptr, nullptr));
    bool fused = !a->dist && enc == 0;
    // measurement knob (tools/cheb_poly_only.py times both forms on one operator): 0 the unfused form, 1 the fused one whatever the encoding
    const int knob = env_int("KRYST_CHEB_POLY_FUSE", -1);
    if (knob == 0) fused = false;
    if (knob == 1 && !a->dist) fused = true;
    ChebPolyPc* pc = new ChebPolyPc(a, degree, scaling, lo, hi, fused);
    int32_t rc = alloc_vec(a->ctx, &pc->d_res, pc->n);
    if (rc == KRYST_OK) rc = alloc_vec(a->ctx, &pc->d_d[0], pc->n);
    if (rc == KRYST_OK) rc = alloc_vec(a->ctx, &pc->d_d[1], pc->n);
    // w is Jacobi's inv_diag as kryst_pc_jacobi forms it (0.0 where the diagonal is missing or zero): the apply takes what it is given, the
    // estimate is what insists on a positive diagonal
    if (rc == KRYST_OK && scaling == KRYST_CHEB_SCALE_JACOBI) rc = alloc_vec(a->ctx, &pc->d_w, pc->n);
    if (rc == KRYST_OK && scaling == KRYST_CHEB_SCALE_JACOBI) rc = jacobi_inv_diag_dev(a, pc->d_w);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

int32_t kryst_pc_chebyshev_poly_info(kryst_pc_t pc, int32_t* degree, int32_t* scaling, double* lo, double* hi, int32_t* fused) {
    ChebPolyPc* c = pc_cast<ChebPolyPc>(pc);
    KR_ARG(c, "pc_chebyshev_poly_info: not a Chebyshev polynomial preconditioner");
    if (degree) *degree = c->degree;
    if (scaling) *scaling = c->scaling;
    if (lo) *lo = c->lo;
    if (hi) *hi = c->hi;
    if (fused) *fused = c->fused ? 1 : 0;
    return KRYST_OK;
}

int32_t kryst_spectrum_estimate(kryst_csr_t a, int32_t scaling, int32_t steps, uint64_t seed, double* alpha_out, double* beta_out,
                                int32_t* steps_done, double* theta_min, double* theta_max, double* gershgorin) {
    KR_ARG(a && alpha_out && beta_out && steps_done && theta_min && theta_max && gershgorin, "spectrum_estimate");
    KR_ARG(a->nrows == a->xlen && a->nrows >= 1, "spectrum_estimate: square operator with at least one row required");
    KR_ARG(scaling == KRYST_CHEB_SCALE_NONE || scaling == KRYST_CHEB_SCALE_JACOBI, "spectrum_estimate: scaling");
    KR_ARG(steps >= 1 && steps <= 64, "spectrum_estimate: steps outside 1..64");
    if (a->dist) { set_error("spectrum_estimate: distributed operators are not supported; pass the bounds"); return KRYST_UNSUPPORTED; }
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    const int64_t n = a->nrows;
    LanczosVecs L;
    L.ctx = ctx;
    const bool scaled = scaling == KRYST_CHEB_SCALE_JACOBI;
    if (scaled) {
        KR_TRY(make_checked_w(a, &L.w));
        KR_TRY(alloc_vec(ctx, &L.s, n));
        KR_TRY(launch_ew(ctx, SqrtOp{L.w, L.s}, n));
    }
    // Gershgorin bound of W A
    {
        unsigned long long* d_g = reinterpret_cast<unsigned long long*>(dot_slot(ctx));
        KR_HIP(hipMemsetAsync(d_g, 0, sizeof(unsigned long long), ctx->s_main));
        hipLaunchKernelGGL(cheb_gershgorin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_val, L.w, (int32_t)n, d_g);
        KR_HIP(hipGetLastError());
        unsigned long long bits = 0;
        KR_HIP(hipMemcpyAsync(&bits, d_g, sizeof bits, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        double g;
        memcpy(&g, &bits, sizeof g);
        *gershgorin = g;
        if (!std::isfinite(g)) { set_error("spectrum_estimate: the Gershgorin bound is not finite"); return KRYST_FACTOR_ERROR; }
    }
    for (kryst_vec_t& x : L.v) KR_TRY(kryst_vec_create(ctx, n, &x));
    kryst_vec_t q = L.v[0], q_prev = L.v[1], t = L.v[2], v = L.v[3], y = L.v[4];
    // q_0 = u / sqrt(dot(u, u))
    KR_TRY(kryst_vec_fill_splitmix(t, seed, 0));
    double uu = 0.0;
    KR_TRY(kryst_dot(t, t, &uu));
    KR_TRY(launch_ew(ctx, DivScalarOp{__builtin_sqrt(uu), t->d, q->d}, n));
    const int kmax = (int)std::min<int64_t>(steps, n);
    int k = 0;
    for (int j = 0; j < kmax; ++j) {
        if (scaled) {
            KR_TRY(launch_ew(ctx, HadamardOp{L.s, q->d, v->d}, n));
            KR_TRY(launch_spmv(a, v->d, y->d, 0, nullptr, nullptr));
            KR_TRY(launch_ew(ctx, HadamardOp{L.s, y->d, t->d}, n));
        } else {
            KR_TRY(launch_spmv(a, q->d, t->d, 0, nullptr, nullptr));
        }
        double al = 0.0, tt = 0.0;
        KR_TRY(kryst_dot(q, t, &al));
        KR_TRY(kryst_axpy(-al, q, t));                               // t - al q: the same bits as t + (-al) q
        if (j > 0) KR_TRY(kryst_axpy(-beta_out[j - 1], q_prev, t));
        KR_TRY(kryst_dot(t, t, &tt));
        const double be = __builtin_sqrt(tt);
        alpha_out[j] = al; beta_out[j] = be;
        k = j + 1;
        if (be == 0.0 || !std::isfinite(be) || k == kmax) break;
        std::swap(q, q_prev);
        KR_TRY(launch_ew(ctx, DivScalarOp{be, t->d, q->d}, n));
    }
    *steps_done = k;
    tridiag_extreme_eigs(alpha_out, beta_out, k, theta_min, theta_max);
    if (!(*theta_max > 0.0) || !std::isfinite(*theta_max)) {
        set_error("spectrum_estimate: the largest Ritz value is not a finite positive number (%g)", *theta_max);
        return KRYST_INDEFINITE_MATRIX;
    }
    return KRYST_OK;
}

}  // extern "C"
