// AMG (src/preconditioner/amg.rs) on gfx950: the device hierarchy and its V-cycle.
//
// The as-written set-up runs on the host (amg_setup.cpp) and every level is uploaded through the operator creation path, so A_l, P_l
// and R_l get the storage forms and launch_spmv of any operator.  One apply is apply_recursive (:200-250), queued on ctx->s_main with
// no host round trip and no-ops behind the `done` flag:
//   sweep      launch_spmv(A_l, z, t) + AmgSweepOp       z = z + D^-1 (r - t)     (smooth_jacobi_parallel, :174-196)
//   restrict   launch_spmv(A_l, z, t) + AmgResidualOp    t = r - t, then launch_spmv(R_l, t, r_{l+1})   (:212-227)
//   prolong    launch_spmv(P_l, z_{l+1}, t) + AmgAddOp   z = z + t                 (:235-247)
//   coarsest   amg_coarse_cg_kernel: solve_direct (:254-312) in one workgroup, the stop test taken on the device
// Every row sum is launch_spmv's (ascending stored columns from 0.0, separate mul and add) and every element-wise step keeps the
// reference's expression, so the V-cycle gives the bits of the reference's loops on the same hierarchy.
#include "pc.h"
#include "ew.h"
#include "amg.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cmath>

namespace kr {

struct AmgDevLevel {
    kryst_csr_t a = nullptr;          // level 0: the borrowed operator; coarse levels: owned
    kryst_csr_t p = nullptr, r = nullptr;   // owned; nullptr on the last level
    double* dinv = nullptr;
    double* t = nullptr;              // work: A z, the residual, P e
    double* rv = nullptr; double* zv = nullptr;   // coarse levels: the restricted residual and the correction
    int64_t n = 0;
};
struct AmgDev final : kryst_pc_s {    // the levels, their operators and work vectors
    static constexpr int KIND = KR_PC_AMG;
    const int variant, nu_pre, nu_post;
    std::vector<AmgDevLevel> lv;
    int32_t* c_ptr = nullptr; int32_t* c_col = nullptr; double* c_val = nullptr;   // the coarsest operator, plain CSR for the CG kernel
    double* c_work = nullptr;         // 3 n: residual, p, Ap
    kryst_pc_t bj = nullptr;          // smoothed aggregation: block Jacobi of 64 rows on the coarsest operator (owned)
    std::vector<int32_t*> agg;        // smoothed aggregation: the aggregate of every row, per coarsened level (owned)
    AmgDev(kryst_csr_t a_, int variant_, int pre, int post) : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), variant(variant_), nu_pre(pre), nu_post(post) {}
    ~AmgDev() override;
    int32_t vcycle(size_t l, const double* r, double* z, const int* done);
    int32_t apply(int64_t nv, const double* r, double* z, const int* done) override;
    bool reads_z() const override { return variant == KRYST_AMG_AS_WRITTEN; }
};

struct AmgSweepOp {                  // z[i] += diag_inv[i] * (r[i] - (A z)[i])   (:183-185)
    static constexpr int NQ = 0; static constexpr const char* TAG = "AmgSweep";
    const double* dinv; const double* r; const double* t; double* z;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 d = ld2(dinv, i), rr = ld2(r, i), tt = ld2(t, i), zz = ld2(z, i);
        st2(z, i, zz.a + d.a * (rr.a - tt.a), zz.b + d.b * (rr.b - tt.b));
    }
};
struct AmgResidualOp {               // az[i] = r[i] - az[i]   (:221-223)
    static constexpr int NQ = 0; static constexpr const char* TAG = "AmgResidual";
    const double* r; double* t;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 rr = ld2(r, i), tt = ld2(t, i);
        st2(t, i, rr.a - tt.a, rr.b - tt.b);
    }
};
struct AmgAddOp {                    // z[i] += fine_correction[i]   (:244-246)
    static constexpr int NQ = 0; static constexpr const char* TAG = "AmgAdd";
    const double* t; double* z;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 tt = ld2(t, i), zz = ld2(z, i);
        st2(z, i, zz.a + tt.a, zz.b + tt.b);
    }
};

constexpr int KR_AMG_CG_THREADS = 256;

// solve_direct (:254-312): x = 0, res = r, p = res; up to n iterations of CG; stop when sqrt(res.res) < 1e-10; z = x.  One workgroup: the
// inner products are the reference's serial sums (thread 0, ascending index, from 0.0), the row sums ascending stored columns.  A zero
// p.Ap divides as written (Inf / NaN).  w: 3 n doubles.
__global__ void __launch_bounds__(KR_AMG_CG_THREADS)
amg_coarse_cg_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val, int32_t n,
                     const double* __restrict__ r, double* __restrict__ z, double* __restrict__ w, const int* done) {
    if (done && *(volatile const int*)done) return;
    __shared__ double s_alpha, s_beta;
    __shared__ int s_stop;
    double* res = w; double* p = w + n; double* ap = w + 2 * (int64_t)n;
    const int tid = threadIdx.x;
    for (int32_t i = tid; i < n; i += KR_AMG_CG_THREADS) { z[i] = 0.0; res[i] = r[i]; p[i] = r[i]; }
    __syncthreads();
    double rr_new = 0.0;                                   // thread 0 only
    if (tid == 0) for (int32_t i = 0; i < n; ++i) rr_new = rr_new + res[i] * res[i];
    for (int32_t it = 0; it < n; ++it) {
        for (int32_t i = tid; i < n; i += KR_AMG_CG_THREADS) {
            double s = 0.0;
            for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) s = s + val[k] * p[col[k]];
            ap[i] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double den = 0.0;
            for (int32_t i = 0; i < n; ++i) den = den + p[i] * ap[i];
            s_alpha = rr_new / den;
        }
        __syncthreads();
        const double alpha = s_alpha;
        for (int32_t i = tid; i < n; i += KR_AMG_CG_THREADS) { z[i] = z[i] + alpha * p[i]; res[i] = res[i] - alpha * ap[i]; }
        __syncthreads();
        if (tid == 0) {
            const double rr_old = rr_new;
            rr_new = 0.0;
            for (int32_t i = 0; i < n; ++i) rr_new = rr_new + res[i] * res[i];
            s_stop = std::sqrt(rr_new) < 1e-10;
            s_beta = rr_new / rr_old;
        }
        __syncthreads();
        if (s_stop) break;
        const double beta = s_beta;
        for (int32_t i = tid; i < n; i += KR_AMG_CG_THREADS) p[i] = res[i] + beta * p[i];
        __syncthreads();
    }
}

static inline int64_t amg_padded(int64_t n) { return (n + KR_TILE - 1) / KR_TILE * KR_TILE; }

static int32_t amg_alloc(kryst_ctx_t ctx, double** p, int64_t n) {
    const size_t bytes = sizeof(double) * (size_t)(amg_padded(n) + KR_TILE);
    KR_HIP(hipMalloc(p, bytes));
    KR_HIP(hipMemsetAsync(*p, 0, bytes, ctx->s_main));
    return KRYST_OK;
}

// apply_recursive(level, r, z) (:200-250)
int32_t AmgDev::vcycle(size_t l, const double* r, double* z, const int* done) {
    AmgDev& H = *this;
    AmgDevLevel& L = H.lv[l];
    if (l + 1 == H.lv.size()) {                                                           // :201-204
        if (L.n == 0) return KRYST_OK;
        if (H.variant == KRYST_AMG_SMOOTHED) return H.bj->apply(L.n, r, z, done);        // exact inverse when A_c has <= 64 rows
        hipLaunchKernelGGL(amg_coarse_cg_kernel, dim3(1), dim3(KR_AMG_CG_THREADS), 0, ctx->s_main, H.c_ptr, H.c_col, H.c_val,
                           (int32_t)L.n, r, z, H.c_work, done);
        KR_HIP(hipGetLastError());
        return KRYST_OK;
    }
    AmgDevLevel& C = H.lv[l + 1];
    for (int s = 0; s < H.nu_pre; ++s) {                                                  // :211
        KR_TRY(launch_spmv(L.a, z, L.t, 0, nullptr, done));
        KR_TRY(launch_ew(ctx, AmgSweepOp{L.dinv, r, L.t, z}, L.n, done));
    }
    KR_TRY(launch_spmv(L.a, z, L.t, 0, nullptr, done));                                   // :213-224
    KR_TRY(launch_ew(ctx, AmgResidualOp{r, L.t}, L.n, done));
    KR_TRY(launch_spmv(L.r, L.t, C.rv, 0, nullptr, done));                                // :226-227
    KR_HIP(hipMemsetAsync(C.zv, 0, sizeof(double) * (size_t)amg_padded(C.n), ctx->s_main));   // :229
    KR_TRY(vcycle(l + 1, C.rv, C.zv, done));                                      // :230-234
    KR_TRY(launch_spmv(L.p, C.zv, L.t, 0, nullptr, done));                                // :236-237
    KR_TRY(launch_ew(ctx, AmgAddOp{L.t, z}, L.n, done));                                  // :238-247
    for (int s = 0; s < H.nu_post; ++s) {                                                 // :249
        KR_TRY(launch_spmv(L.a, z, L.t, 0, nullptr, done));
        KR_TRY(launch_ew(ctx, AmgSweepOp{L.dinv, r, L.t, z}, L.n, done));
    }
    return KRYST_OK;
}

int32_t AmgDev::apply(int64_t, const double* r, double* z, const int* done) {
    if (lv.empty()) { set_error("amg: no hierarchy"); return KRYST_SOLVE_ERROR; }
    if (variant == KRYST_AMG_SMOOTHED)                                                     // z starts from zero: M is linear and symmetric
        KR_TRY(launch_ew(ctx, AmgSetOp{nullptr, z}, n, done));
    return vcycle(0, r, z, done);
}

AmgDev::~AmgDev() {
    AmgDev& H = *this;
    for (size_t l = 0; l < H.lv.size(); ++l) {
        AmgDevLevel& L = H.lv[l];
        if (l > 0 && L.a) kryst_csr_destroy(L.a);
        if (L.p) kryst_csr_destroy(L.p);
        if (L.r) kryst_csr_destroy(L.r);
        (void)hipFree(L.dinv); (void)hipFree(L.t); (void)hipFree(L.rv); (void)hipFree(L.zv);
    }
    (void)hipFree(H.c_ptr); (void)hipFree(H.c_col); (void)hipFree(H.c_val); (void)hipFree(H.c_work);
    if (H.bj) kryst_pc_destroy(H.bj);
    for (int32_t* g : H.agg) (void)hipFree(g);
}

static int32_t upload_csr_level(kryst_ctx_t ctx, const HostCsr& m, kryst_csr_t* out) {
    return kryst_csr_create_i32(ctx, m.nrows, m.ncols, m.ptr.data(), m.col.data(), m.val.data(), out);
}

template <class T>
static int32_t upload(kryst_ctx_t ctx, T** d, const T* h, size_t n, size_t alloc) {
    KR_HIP(hipMalloc(d, sizeof(T) * std::max<size_t>(alloc, 1)));
    KR_HIP(hipMemsetAsync(*d, 0, sizeof(T) * std::max<size_t>(alloc, 1), ctx->s_main));
    if (n) KR_HIP(hipMemcpyAsync(*d, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->s_main));
    return KRYST_OK;
}

// the hierarchy the host set-up built, on the device (level 0's operator is `a` itself)
static int32_t amg_upload(AmgDev* pc, std::vector<AmgHostLevel>& hl) {
    kryst_ctx_t ctx = pc->ctx;
    AmgDev& H = *pc;
    H.lv.resize(hl.size());
    for (size_t l = 0; l < hl.size(); ++l) {
        AmgHostLevel& S = hl[l];
        AmgDevLevel& L = H.lv[l];
        L.n = S.a.nrows;
        if (l == 0) L.a = pc->a;
        else KR_TRY(upload_csr_level(ctx, S.a, &L.a));
        KR_TRY(amg_alloc(ctx, &L.dinv, L.n));
        if (L.n) KR_HIP(hipMemcpyAsync(L.dinv, S.dinv.data(), sizeof(double) * (size_t)L.n, hipMemcpyHostToDevice, ctx->s_main));
        KR_TRY(amg_alloc(ctx, &L.t, L.n));
        if (l > 0) { KR_TRY(amg_alloc(ctx, &L.rv, L.n)); KR_TRY(amg_alloc(ctx, &L.zv, L.n)); }
        if (l + 1 < hl.size()) {
            KR_TRY(upload_csr_level(ctx, S.p, &L.p));
            KR_TRY(upload_csr_level(ctx, S.r, &L.r));
        }
    }
    const HostCsr& c = hl.back().a;
    std::vector<int32_t> cp(c.ptr.begin(), c.ptr.end());
    KR_TRY(upload(ctx, &H.c_ptr, cp.data(), cp.size(), cp.size()));
    KR_TRY(upload(ctx, &H.c_col, c.col.data(), c.col.size(), c.col.size()));
    KR_TRY(upload(ctx, &H.c_val, c.val.data(), c.val.size(), c.val.size()));
    KR_HIP(hipMalloc(&H.c_work, sizeof(double) * (size_t)std::max<int64_t>(3 * c.nrows, 1)));
    KR_HIP(hipMemsetAsync(H.c_work, 0, sizeof(double) * (size_t)std::max<int64_t>(3 * c.nrows, 1), ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return KRYST_OK;
}

// ================================================================ textbook smoothed aggregation (labelled extension), set up on the device
// Vaněk, Mandel & Brezina (1996); aggregation by distance-2 MIS with hashed priorities (Bell, Dalton & Olson, SISC 2012).  Every kernel is
// one thread per row with a fixed order of operations: the set-up gives the same bits on every run.
// strength: j != i and |a_ij| > theta sqrt(|a_ii a_jj|)

__device__ __forceinline__ uint64_t sa_key(int32_t i) {
    uint32_t h = (uint32_t)i * 0x9E3779B1u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return ((uint64_t)h << 32) | (uint32_t)i;
}
__device__ __forceinline__ bool sa_strong(int32_t i, int32_t j, double v, const double* d, double theta) {
    return j != i && fabs(v) > theta * sqrt(fabs(d[i] * d[j]));
}

// diagonal, D^-1, Gershgorin row bound sum_j |a_ij| / |a_ii| (max by atomicMax on the bits of a non-negative double: order-free)
__global__ void sa_diag_kernel(const int32_t* ptr, const int32_t* col, const double* val, int32_t n, double* d, double* dinv,
                               unsigned long long* rho_bits, int32_t* zero_row) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double di = 0.0, s = 0.0;
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) { if (col[k] == i) di = val[k]; s = s + fabs(val[k]); }
    d[i] = di;
    if (di == 0.0) { atomicMin(zero_row, i); dinv[i] = 0.0; return; }
    dinv[i] = 1.0 / di;
    const double g = s / fabs(di);
    atomicMax(rho_bits, (unsigned long long)__double_as_longlong(g));
}

// MIS-2 round: m1 = max key of the undecided in {i} + strong(i); m2 = max m1 over {i} + strong(i); IN where m2 == own key
__global__ void sa_mis_max_kernel(const int32_t* ptr, const int32_t* col, const double* val, int32_t n, const double* d, double theta,
                                  const uint8_t* state, const uint64_t* in, uint64_t* out, int first) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t m = first ? (state[i] == 0 ? sa_key(i) : 0) : in[i];
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) {
        const int32_t j = col[k];
        if (!sa_strong(i, j, val[k], d, theta)) continue;
        const uint64_t c = first ? (state[j] == 0 ? sa_key(j) : 0) : in[j];
        m = c > m ? c : m;
    }
    out[i] = m;
}
__global__ void sa_mis_select_kernel(int32_t n, uint8_t* state, const uint64_t* m2) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && state[i] == 0 && m2[i] == sa_key(i)) state[i] = 1;
}
// f = 1 where {i} + strong(i) holds an IN node (pass 1), or a node with f (pass 2: undecided nodes become OUT); counts the undecided
__global__ void sa_mis_near_kernel(const int32_t* ptr, const int32_t* col, const double* val, int32_t n, const double* d, double theta,
                                   uint8_t* state, const uint8_t* fin, uint8_t* fout, int pass, int32_t* undecided) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool f = pass == 1 ? state[i] == 1 : fin[i] != 0;
    for (int32_t k = ptr[i]; k < ptr[i + 1] && !f; ++k) {
        const int32_t j = col[k];
        if (sa_strong(i, j, val[k], d, theta)) f = pass == 1 ? state[j] == 1 : fin[j] != 0;
    }
    if (pass == 1) { fout[i] = f; return; }
    if (state[i] == 0 && f) state[i] = 2;
    if (state[i] == 0) atomicAdd(undecided, 1);
}
// aggregates: roots keep their own (numbered in row order); pass 1: the first strong neighbour that is a root; pass 2: the first strong
// neighbour that has one after pass 1; what is left becomes a singleton (numbered after the roots in row order)
__global__ void sa_agg_kernel(const int32_t* ptr, const int32_t* col, const double* val, int32_t n, const double* d, double theta,
                              const uint8_t* state, const int32_t* rid, const int32_t* ain, int32_t* aout, int pass) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t g = pass == 1 ? (state[i] == 1 ? rid[i] : -1) : ain[i];
    for (int32_t k = ptr[i]; k < ptr[i + 1] && g < 0; ++k) {
        const int32_t j = col[k];
        if (!sa_strong(i, j, val[k], d, theta)) continue;
        if (pass == 1 && state[j] == 1) g = rid[j];
        if (pass == 2 && ain[j] >= 0) g = ain[j];
    }
    aout[i] = g;
}
__global__ void sa_flag_kernel(int32_t n, const uint8_t* state, const int32_t* agg, int32_t* flag, int mode) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = mode == 0 ? (state[i] == 1) : (agg[i] < 0);
}
__global__ void sa_finish_agg_kernel(int32_t n, int32_t* agg, const int32_t* sid, int32_t nroots, int32_t* size) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (agg[i] < 0) agg[i] = nroots + sid[i];
    atomicAdd(&size[agg[i]], 1);
}
// tentative P0 as CSR (one entry per row): unit-norm columns
__global__ void sa_p0_kernel(int32_t n, const int32_t* agg, const int32_t* size, int32_t* pp, double* pv) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    pp[i] = i;
    if (i < n) pv[i] = 1.0 / sqrt((double)size[agg[i]]);
}
// P = (I - omega D^-1 A) P0 on the pattern of A P0: p = [J == agg_i] p0_i - (omega dinv_i) (A P0)_iJ
__global__ void sa_smooth_kernel(int32_t n, const int32_t* cp, const int32_t* cc, double* cv, const int32_t* agg, const double* p0,
                                 const double* dinv, double omega) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double w = omega * dinv[i];
    for (int32_t k = cp[i]; k < cp[i + 1]; ++k) cv[k] = (cc[k] == agg[i] ? p0[i] : 0.0) - w * cv[k];
}

// deterministic SpGEMM C = A B, one thread per row: a merge of the sorted rows of B that row i of A selects; column by column in
// ascending order, each entry summed over ascending stored positions of A's row from 0.0.  Pass FILL = false counts, FILL = true writes.
// head: nnz(A) ints of scratch.  B's rows must be strictly ascending.
template <bool FILL>
__global__ void sa_spgemm_kernel(const int32_t* ap, const int32_t* ac, const double* av, int32_t n, const int32_t* bp, const int32_t* bc,
                                 const double* bv, int32_t* head, int32_t* cnt, const int32_t* cp, int32_t* cc, double* cv) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t a0 = ap[i], a1 = ap[i + 1];
    for (int32_t k = a0; k < a1; ++k) head[k] = bp[ac[k]];
    int32_t out = FILL ? cp[i] : 0;
    for (;;) {
        int32_t cmin = INT_MAX;
        for (int32_t k = a0; k < a1; ++k) {
            const int32_t h = head[k];
            if (h < bp[ac[k] + 1]) cmin = min(cmin, bc[h]);
        }
        if (cmin == INT_MAX) break;
        double s = 0.0;
        for (int32_t k = a0; k < a1; ++k) {
            const int32_t h = head[k];
            if (h < bp[ac[k] + 1] && bc[h] == cmin) {
                if (FILL) s = s + av[k] * bv[h];
                head[k] = h + 1;
            }
        }
        if (FILL) { cc[out] = cmin; cv[out] = s; }
        ++out;
    }
    if (!FILL) cnt[i] = out;
}

static inline dim3 sa_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>((n + 255) / 256, 1)); }

// exclusive prefix sum of cnt[0 .. n) into out[0 .. n]; returns out[n] on the host
static int32_t sa_scan(kryst_ctx_t ctx, const int32_t* cnt, int32_t* out, int64_t n, int64_t* total) {
    size_t tmp_bytes = 0;
    KR_HIP(hipMemsetAsync(out, 0, sizeof(int32_t), ctx->s_main));
    if (n > 0) {
        KR_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, cnt, out + 1, (int)n, ctx->s_main));
        void* tmp = nullptr;
        KR_HIP(hipMalloc(&tmp, std::max<size_t>(tmp_bytes, 1)));
        const hipError_t e = hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, cnt, out + 1, (int)n, ctx->s_main);
        (void)hipStreamSynchronize(ctx->s_main);
        (void)hipFree(tmp);
        KR_HIP(e);
    }
    int32_t t = 0;
    KR_HIP(hipMemcpyAsync(&t, out + n, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    *total = t;
    return KRYST_OK;
}

static int32_t sa_spgemm(kryst_ctx_t ctx, const int32_t* ap, const int32_t* ac, const double* av, int64_t n, int64_t annz,
                         const int32_t* bp, const int32_t* bc, const double* bv, DevCsr& c) {
    int32_t *head = nullptr, *cnt = nullptr;
    KR_HIP(hipMalloc(&head, sizeof(int32_t) * (size_t)std::max<int64_t>(annz, 1)));
    KR_HIP(hipMalloc(&cnt, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)));
    KR_HIP(hipMalloc(&c.ptr, sizeof(int32_t) * (size_t)(n + 1)));
    hipLaunchKernelGGL(sa_spgemm_kernel<false>, sa_grid(n), dim3(256), 0, ctx->s_main, ap, ac, av, (int32_t)n, bp, bc, bv, head, cnt,
                       nullptr, nullptr, nullptr);
    KR_HIP(hipGetLastError());
    int64_t nnz = 0;
    int32_t rc = sa_scan(ctx, cnt, c.ptr, n, &nnz);
    if (rc == KRYST_OK) {
        c.nnz = nnz;
        KR_HIP(hipMalloc(&c.idx, sizeof(int32_t) * (size_t)(nnz + 8)));
        KR_HIP(hipMalloc(&c.val, sizeof(double) * (size_t)(nnz + 8)));
        KR_HIP(hipMemsetAsync(c.idx, 0, sizeof(int32_t) * (size_t)(nnz + 8), ctx->s_main));
        KR_HIP(hipMemsetAsync(c.val, 0, sizeof(double) * (size_t)(nnz + 8), ctx->s_main));
        hipLaunchKernelGGL(sa_spgemm_kernel<true>, sa_grid(n), dim3(256), 0, ctx->s_main, ap, ac, av, (int32_t)n, bp, bc, bv, head, cnt,
                           c.ptr, c.idx, c.val);
        KR_HIP(hipGetLastError());
        KR_HIP(hipStreamSynchronize(ctx->s_main));
    }
    (void)hipFree(head); (void)hipFree(cnt);
    return rc;
}

static int32_t sa_to_operator(kryst_ctx_t ctx, const DevCsr& m, int64_t nrows, int64_t ncols, kryst_csr_t* out) {
    std::vector<int32_t> p32((size_t)nrows + 1);
    std::vector<int32_t> ci((size_t)std::max<int64_t>(m.nnz, 1));
    std::vector<double> va((size_t)std::max<int64_t>(m.nnz, 1));
    KR_HIP(hipMemcpyAsync(p32.data(), m.ptr, sizeof(int32_t) * p32.size(), hipMemcpyDeviceToHost, ctx->s_main));
    if (m.nnz) {
        KR_HIP(hipMemcpyAsync(ci.data(), m.idx, sizeof(int32_t) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipMemcpyAsync(va.data(), m.val, sizeof(double) * (size_t)m.nnz, hipMemcpyDeviceToHost, ctx->s_main));
    }
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    std::vector<int64_t> rp(p32.begin(), p32.end());
    return kryst_csr_create_i32(ctx, nrows, ncols, rp.data(), ci.data(), va.data(), out);
}

// one SA level on A (device rows ptr / col / val, n x n): D^-1 (scaled by omega in `wdinv`), the aggregates, P, R = P^T, A_c = R (A P)
struct SaLevelOut { DevCsr p, r, ac; int32_t* agg = nullptr; int64_t nc = 0; double* wdinv = nullptr; };

static int32_t sa_level(kryst_ctx_t ctx, const int32_t* ptr, const int32_t* col, const double* val, int64_t n, int64_t nnz, double theta,
                        SaLevelOut& o) {
    double *d = nullptr, *dinv = nullptr, *p0v = nullptr;
    unsigned long long* rho_bits = nullptr; int32_t* zero_row = nullptr; int32_t* undecided = nullptr;
    uint8_t *state = nullptr, *f1 = nullptr; uint64_t *m1 = nullptr, *m2 = nullptr;
    int32_t *flag = nullptr, *rid = nullptr, *a1 = nullptr, *size = nullptr, *p0p = nullptr;
    DevCsr ap0, ap;
    int32_t rc = KRYST_OK;
    const dim3 g = sa_grid(n), b(256);
    auto fail = [&](int32_t e) { rc = e; };
    do {
        if (hipMalloc(&d, 8 * n) || hipMalloc(&dinv, 8 * (n + KR_TILE)) || hipMalloc(&rho_bits, 8) || hipMalloc(&zero_row, 4) ||
            hipMalloc(&undecided, 4) || hipMalloc(&state, n) || hipMalloc(&f1, n) || hipMalloc(&m1, 8 * n) || hipMalloc(&m2, 8 * n) ||
            hipMalloc(&flag, 4 * n) || hipMalloc(&rid, 4 * (n + 1)) || hipMalloc(&a1, 4 * n) || hipMalloc(&o.agg, 4 * n) ||
            hipMalloc(&size, 4 * n) || hipMalloc(&p0p, 4 * (n + 1)) || hipMalloc(&p0v, 8 * n)) { set_error("amg: out of device memory"); fail(KRYST_ERR_HIP); break; }
        const int32_t big = INT_MAX;
        KR_HIP(hipMemsetAsync(rho_bits, 0, 8, ctx->s_main));
        KR_HIP(hipMemcpyAsync(zero_row, &big, 4, hipMemcpyHostToDevice, ctx->s_main));
        KR_HIP(hipMemsetAsync(dinv, 0, 8 * (n + KR_TILE), ctx->s_main));
        hipLaunchKernelGGL(sa_diag_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, dinv, rho_bits, zero_row);
        unsigned long long rb = 0; int32_t zr = 0;
        KR_HIP(hipMemcpyAsync(&rb, rho_bits, 8, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipMemcpyAsync(&zr, zero_row, 4, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        if (zr != big) { set_error("amg: zero diagonal in row %d", zr); set_error_row(zr); fail(KRYST_ZERO_PIVOT); break; }
        double rho; std::memcpy(&rho, &rb, 8);
        const double omega = 4.0 / (3.0 * rho);
        // distance-2 MIS
        KR_HIP(hipMemsetAsync(state, 0, n, ctx->s_main));
        for (int round = 0; ; ++round) {
            if (round > 1000) { set_error("amg: aggregation did not finish"); fail(KRYST_FACTOR_ERROR); break; }
            KR_HIP(hipMemsetAsync(undecided, 0, 4, ctx->s_main));
            hipLaunchKernelGGL(sa_mis_max_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, nullptr, m1, 1);
            hipLaunchKernelGGL(sa_mis_max_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, m1, m2, 0);
            hipLaunchKernelGGL(sa_mis_select_kernel, g, b, 0, ctx->s_main, (int32_t)n, state, m2);
            hipLaunchKernelGGL(sa_mis_near_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, nullptr, f1, 1, undecided);
            hipLaunchKernelGGL(sa_mis_near_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, f1, nullptr, 2, undecided);
            KR_HIP(hipGetLastError());
            int32_t und = 0;
            KR_HIP(hipMemcpyAsync(&und, undecided, 4, hipMemcpyDeviceToHost, ctx->s_main));
            KR_HIP(hipStreamSynchronize(ctx->s_main));
            if (und == 0) break;
        }
        if (rc) break;
        int64_t nroots = 0, nleft = 0;
        hipLaunchKernelGGL(sa_flag_kernel, g, b, 0, ctx->s_main, (int32_t)n, state, nullptr, flag, 0);
        if ((rc = sa_scan(ctx, flag, rid, n, &nroots))) break;
        hipLaunchKernelGGL(sa_agg_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, rid, nullptr, a1, 1);
        hipLaunchKernelGGL(sa_agg_kernel, g, b, 0, ctx->s_main, ptr, col, val, (int32_t)n, d, theta, state, rid, a1, o.agg, 2);
        hipLaunchKernelGGL(sa_flag_kernel, g, b, 0, ctx->s_main, (int32_t)n, state, o.agg, flag, 1);
        if ((rc = sa_scan(ctx, flag, rid, n, &nleft))) break;
        o.nc = nroots + nleft;
        KR_HIP(hipMemsetAsync(size, 0, 4 * n, ctx->s_main));
        hipLaunchKernelGGL(sa_finish_agg_kernel, g, b, 0, ctx->s_main, (int32_t)n, o.agg, rid, (int32_t)nroots, size);
        hipLaunchKernelGGL(sa_p0_kernel, sa_grid(n + 1), b, 0, ctx->s_main, (int32_t)n, o.agg, size, p0p, p0v);
        KR_HIP(hipGetLastError());
        // P = (I - omega D^-1 A) P0, R = P^T, A_c = R (A P)
        if ((rc = sa_spgemm(ctx, ptr, col, val, n, nnz, p0p, o.agg, p0v, ap0))) break;
        hipLaunchKernelGGL(sa_smooth_kernel, g, b, 0, ctx->s_main, (int32_t)n, ap0.ptr, ap0.idx, ap0.val, o.agg, p0v, dinv, omega);
        KR_HIP(hipGetLastError());
        o.p = ap0; ap0 = DevCsr();
        if ((rc = csr_transpose(ctx, "amg", o.p.ptr, o.p.idx, o.p.val, n, o.nc, false, 0.0, o.r))) break;
        if ((rc = sa_spgemm(ctx, ptr, col, val, n, nnz, o.p.ptr, o.p.idx, o.p.val, ap))) break;
        if ((rc = sa_spgemm(ctx, o.r.ptr, o.r.idx, o.r.val, o.nc, o.r.nnz, ap.ptr, ap.idx, ap.val, o.ac))) break;
        // the smoother's omega D^-1
        std::vector<double> h((size_t)n);
        KR_HIP(hipMemcpyAsync(h.data(), dinv, 8 * n, hipMemcpyDeviceToHost, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        for (double& v : h) v = omega * v;
        KR_HIP(hipMemcpyAsync(dinv, h.data(), 8 * n, hipMemcpyHostToDevice, ctx->s_main));
        KR_HIP(hipStreamSynchronize(ctx->s_main));
        o.wdinv = dinv; dinv = nullptr;
    } while (false);
    (void)hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d); (void)hipFree(dinv); (void)hipFree(rho_bits); (void)hipFree(zero_row); (void)hipFree(undecided); (void)hipFree(state);
    (void)hipFree(f1); (void)hipFree(m1); (void)hipFree(m2); (void)hipFree(flag); (void)hipFree(rid); (void)hipFree(a1); (void)hipFree(size);
    (void)hipFree(p0p); (void)hipFree(p0v);
    dev_csr_free(ap0); dev_csr_free(ap);
    return rc;
}

// the SA hierarchy: coarsen while n > 64, for at most max_levels levels, and until n_c > 0.8 n (a stalled level is dropped)
static int32_t sa_build(AmgDev* pc, int32_t max_levels, double theta) {
    kryst_ctx_t ctx = pc->ctx;
    AmgDev& H = *pc;
    kryst_csr_t cur = pc->a;
    for (int32_t lv = 0; ; ++lv) {
        AmgDevLevel L;
        L.a = cur; L.n = cur->nrows;
        const bool last = lv >= max_levels || L.n <= 64;
        SaLevelOut o;
        int32_t rc = KRYST_OK;
        if (!last) rc = sa_level(ctx, cur->d_row_ptr, cur->d_col, cur->d_val, L.n, cur->nnz, theta, o);
        const bool stalled = !last && rc == KRYST_OK && (double)o.nc > 0.8 * (double)L.n;
        if (rc != KRYST_OK || last || stalled) {
            dev_csr_free(o.p); dev_csr_free(o.r); dev_csr_free(o.ac); (void)hipFree(o.agg); (void)hipFree(o.wdinv);
            if (rc != KRYST_OK) { if (lv > 0) kryst_csr_destroy(cur); return rc; }
            H.lv.push_back(L);                                   // the coarsest level: block Jacobi of 64 rows
            KR_TRY(amg_alloc(ctx, &H.lv.back().dinv, L.n));
            KR_TRY(amg_alloc(ctx, &H.lv.back().t, L.n));
            if (lv > 0) { KR_TRY(amg_alloc(ctx, &H.lv.back().rv, L.n)); KR_TRY(amg_alloc(ctx, &H.lv.back().zv, L.n)); }
            return kryst_pc_block_jacobi_uniform(cur, (int32_t)std::min<int64_t>(64, std::max<int64_t>(L.n, 1)), &H.bj);
        }
        L.dinv = o.wdinv;
        int32_t e = sa_to_operator(ctx, o.p, L.n, o.nc, &L.p);
        if (e == KRYST_OK) e = sa_to_operator(ctx, o.r, o.nc, L.n, &L.r);
        kryst_csr_t next = nullptr;
        if (e == KRYST_OK) e = sa_to_operator(ctx, o.ac, o.nc, o.nc, &next);
        dev_csr_free(o.p); dev_csr_free(o.r); dev_csr_free(o.ac);
        H.agg.push_back(o.agg);
        if (e == KRYST_OK) e = amg_alloc(ctx, &L.t, L.n);
        if (e == KRYST_OK && lv > 0) { e = amg_alloc(ctx, &L.rv, L.n); if (e == KRYST_OK) e = amg_alloc(ctx, &L.zv, L.n); }
        H.lv.push_back(L);
        if (e != KRYST_OK) { if (next) kryst_csr_destroy(next); return e; }
        cur = next;
    }
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_amg(kryst_csr_t a, int32_t max_levels, double threshold, int32_t variant, int32_t nu_pre, int32_t nu_post, kryst_pc_t* out) {
    KR_ARG(a && out, "pc_amg");
    *out = nullptr;
    if (a->dist) { set_error("pc_amg: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->xlen && a->nrows == a->ncols, "pc_amg: square operator required");
    KR_ARG(max_levels >= 0 && nu_pre >= 0 && nu_post >= 0, "pc_amg: max_levels, nu_pre and nu_post must be >= 0");
    KR_ARG(variant == KRYST_AMG_AS_WRITTEN || variant == KRYST_AMG_SMOOTHED, "pc_amg: unknown variant");
    KR_HIP(hipSetDevice(a->ctx->device));
    if (variant == KRYST_AMG_SMOOTHED) {                  // labelled extension: threshold is theta of the strength test
        KR_ARG(max_levels >= 1, "pc_amg: smoothed aggregation needs max_levels >= 1");
        KR_ARG(threshold >= 0.0, "pc_amg: theta must be >= 0");
        AmgDev* pc = new AmgDev(a, variant, nu_pre, nu_post);
        const int32_t rc = sa_build(pc, max_levels, threshold);
        if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
        *out = pc;
        return KRYST_OK;
    }
    const int64_t n = a->nrows;
    std::vector<int64_t> rp((size_t)n + 1);
    std::vector<int32_t> ci((size_t)a->nnz);
    std::vector<double> va((size_t)a->nnz);
    KR_TRY(kryst_csr_download(a, rp.data(), ci.data(), va.data()));
    std::vector<AmgHostLevel> hl;
    KR_TRY(amg_setup_as_written(n, rp.data(), ci.data(), va.data(), max_levels, threshold, 0, hl));
    if (hl.back().a.nrows > KRYST_AMG_DIRECT_MAX) {
        set_error("pc_amg: the coarsest level has %lld rows, more than the %d its one-workgroup CG takes (raise max_levels)",
                  (long long)hl.back().a.nrows, (int)KRYST_AMG_DIRECT_MAX);
        return KRYST_UNSUPPORTED;
    }
    AmgDev* pc = new AmgDev(a, variant, nu_pre, nu_post);
    const int32_t rc = amg_upload(pc, hl);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

int32_t kryst_pc_amg_info(kryst_pc_t h, int32_t* nlevels, int64_t* rows, int64_t* nnz, int32_t count) {
    AmgDev* pc = pc_cast<AmgDev>(h);
    KR_ARG(pc, "pc_amg_info: not an AMG preconditioner");
    const int32_t L = (int32_t)pc->lv.size();
    if (nlevels) *nlevels = L;
    KR_ARG((!rows && !nnz) || count >= L, "pc_amg_info: count < levels");
    for (int32_t l = 0; l < L; ++l) {
        if (rows) rows[l] = pc->lv[l].n;
        if (nnz) nnz[l] = pc->lv[l].a->nnz;
    }
    return KRYST_OK;
}

int32_t kryst_pc_amg_export(kryst_pc_t h, int32_t level, int32_t which, int64_t* nrows, int64_t* ncols, int64_t* nnz, int64_t* row_ptr,
                            int32_t* col, double* val) {
    AmgDev* pc = pc_cast<AmgDev>(h);
    KR_ARG(pc, "pc_amg_export: not an AMG preconditioner");
    KR_ARG(level >= 0 && level < (int32_t)pc->lv.size(), "pc_amg_export: level out of range");
    KR_ARG(which >= 0 && which <= 4, "pc_amg_export: which must be 0 (A), 1 (P), 2 (R), 3 (D^-1) or 4 (aggregates)");
    KR_HIP(hipSetDevice(pc->ctx->device));
    AmgDevLevel& L = pc->lv[level];
    if (which == 4) {                                      // smoothed aggregation: the aggregate of every row (none on the last level)
        const bool has = level < (int32_t)pc->agg.size();
        if (nrows) *nrows = has ? L.n : 0;
        if (ncols) *ncols = 1;
        if (nnz) *nnz = has ? L.n : 0;
        if (has && col && L.n) {
            KR_HIP(hipMemcpyAsync(col, pc->agg[level], sizeof(int32_t) * (size_t)L.n, hipMemcpyDeviceToHost, pc->ctx->s_main));
            KR_HIP(hipStreamSynchronize(pc->ctx->s_main));
        }
        return KRYST_OK;
    }
    if (which == 3) {
        if (nrows) *nrows = L.n;
        if (ncols) *ncols = 1;
        if (nnz) *nnz = L.n;
        if (val && L.n) {
            KR_HIP(hipMemcpyAsync(val, L.dinv, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToHost, pc->ctx->s_main));
            KR_HIP(hipStreamSynchronize(pc->ctx->s_main));
        }
        return KRYST_OK;
    }
    kryst_csr_t m = which == 0 ? L.a : which == 1 ? L.p : L.r;
    if (nrows) *nrows = m ? m->nrows : 0;
    if (ncols) *ncols = m ? m->ncols : 0;
    if (nnz) *nnz = m ? m->nnz : 0;
    if (!m) { if (row_ptr) row_ptr[0] = 0; return KRYST_OK; }
    if (!row_ptr) return KRYST_OK;
    return kryst_csr_download(m, row_ptr, col, val);
}

}  // extern "C"
