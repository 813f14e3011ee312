// SOR / SSOR (Sor, MatSorType, src/preconditioner/sor.rs:106-170) on the device, and the same sweeps in a coloured row order (labelled
// extension: PC::Multicolor has no implementation in the reference).  DESIGN.md section 4.11.
//
// As written: inv_diag[i] = 1 / (a_ii + fshift), a sum of exactly zero is ZeroPivot(i).  apply: y = +0.0, then `its` times
//   APPLY_LOWER  i ascending:   sigma = +0.0; + a_ij y_j for stored j < i ascending; unless EISENSTAT + a_ij x_j (x, not y) for stored j > i
//                               ascending; y_i = (x_i - sigma) inv_diag[i]                                     (no omega in this sweep)
//   APPLY_UPPER  i descending:  sigma = +0.0; + a_ij y_j for stored j > i ascending; unless EISENSTAT + a_ij y_j for stored j < i ascending
//                               (values this sweep has not touched yet); y_i = (1 - omega) x_i + omega ((x_i - sigma) inv_diag[i])
// every operation rounded on its own.  The reference walks the whole dense row; the absent terms are +-0 products that leave a finite sum
// started at +0.0 unchanged.  lits and the LOCAL_* bits are stored and not used, as written.
//
// Coloured order: rows are visited by (colors[i], i) ascending in a forward sweep, in the exact reverse in a backward one; "j < i" and
// "j > i" above then compare positions in that order, and the terms of a group are summed in ascending position: exactly the loops above
// on the permuted matrix P A P^T with P x, un-permuted.  (Set-up sorts every row's entries by position once: 4 bytes per entry more to read.)
//
// One kernel, one schedule for both: the rows of a sweep are grouped by dependency level of the strictly-lower (forward) / strictly-upper
// (backward) part of the pattern permuted into the sweep order (host_levels), and ONE persistent launch walks the groups with a grid
// barrier between them, a row per lane.  A row of level l reads y only from rows of lower levels (already final for this sweep) and, in a
// backward sweep without EISENSTAT, from rows earlier in the order, which must still hold the previous sweep's value: those rows are made
// to wait for this one (with a symmetric pattern they do anyway), so their level is higher -- the barrier between levels is all the
// ordering a sweep needs.  The kernel reads A's own CSR arrays.
//
// Hand-off between workgroups: every store of y is write-through at agent scope and every load of y bypasses the L1 (relaxed agent-scope
// atomics), every wave waits for its stores before the workgroup barrier in front of the arrival, one lane adds to the arrival counter
// and polls it, the others wait for that lane at a workgroup barrier.  At most one workgroup per CU, so that all of them are resident;
// the poll has a budget, and a workgroup whose patience runs out raises the give-up word and writes NaN from then on: an abandoned
// sweep is an error (kryst_pc_apply, the end of a solve), never a hung device and never a plausible vector.
#include "pc.h"
#include "host_factor.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace kr {

constexpr int KR_SOR_T = 1024;                   // threads of a sweep workgroup: one per CU, sixteen waves
constexpr int KR_SOR_LOWER = 2, KR_SOR_UPPER = 4, KR_SOR_EISENSTAT = 32;     // MatSorType bits (sor.rs:35-42)

__global__ void sor_setup_kernel(const int32_t* row_ptr, const int32_t* col, const double* val, int32_t n, double fshift, double* inv_diag,
                                 unsigned long long* err) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;                                                      // no stored diagonal: a_ii = 0
    for (int32_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
        if (col[k] == i) { d = val[k]; break; }
    const double aii = d + fshift;                                       // sor.rs:111-115
    if (aii == 0.0) atomicMin(err, (unsigned long long)i);
    inv_diag[i] = 1.0 / aii;
}

__global__ void sor_zero_kernel(double* y, int64_t n, const int* done) {
    if (done && *done) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = 0.0;
}

__device__ __forceinline__ double sor_ld(const double* p) { return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sor_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The `which`-th barrier of the launch: arrivals are counted in *cnt (zeroed in front of the launch), so it is passed when the counter
// has reached which * gridDim.x.  Returns false in every thread of a workgroup whose poll ran out of patience.
__device__ __forceinline__ bool sor_grid_barrier(uint32_t* cnt, uint32_t which, uint32_t* gave_up, int* ok_s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // every wave: its write-through stores of y have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t target = which * gridDim.x;
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        // (the other workgroups may be waiting for a CU behind another process's kernel: patience of seconds, short naps first)
        for (int budget = 1 << 22; __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; --budget) {
            if (budget <= 0) { ok = 0; break; }
            if (budget > (1 << 22) - 4096) __builtin_amdgcn_s_sleep(1); else __builtin_amdgcn_s_sleep(64);
        }
        if (!ok) __hip_atomic_store(gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        *ok_s = ok;
    }
    __syncthreads();
    return *ok_s != 0;
}

// One sweep.  rows[off[g] .. off[g + 1]) are the rows of group g; pos[i] is row i's position in the sweep order (nullptr: i itself);
// ent[k0 .. k1) are the entries of a row in ascending position (nullptr: the stored order is that order).
template <bool FORWARD, bool EIS>
__global__ __launch_bounds__(KR_SOR_T) void sor_sweep_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             const double* __restrict__ val, const double* __restrict__ inv_diag,
                                                             const int32_t* __restrict__ pos, const int32_t* __restrict__ ent,
                                                             const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ off, int32_t ngroups, double omega,
                                                             const double* __restrict__ x, double* y, uint32_t* cnt, uint32_t* gave_up,
                                                             const int* done) {
    if (done && *done) return;                                           // (the same answer in every workgroup: nobody waits for one that left)
    __shared__ int ok_s;
    bool alive = true;
    const double om1 = 1.0 - omega;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int32_t g = 0; g < ngroups; ++g) {
        const int32_t p1 = off[g + 1];
        for (int64_t p = (int64_t)off[g] + (int64_t)blockIdx.x * KR_SOR_T + threadIdx.x; p < p1; p += (int64_t)gridDim.x * KR_SOR_T) {
            const int32_t i = rows[p];
            const int32_t pi = pos ? pos[i] : i;
            const int32_t k0 = row_ptr[i], k1 = row_ptr[i + 1];
            double sigma = 0.0;
            for (int32_t k = k0; k < k1; ++k) {                          // the rows this sweep has already visited
                const int32_t e = ent ? ent[k] : k;
                const int32_t j = col[e], pj = pos ? pos[j] : j;
                if (FORWARD ? pj < pi : pj > pi) sigma = sigma + val[e] * sor_ld(y + j);
            }
            if (!EIS)
                for (int32_t k = k0; k < k1; ++k) {                      // the rows it has not: x in a forward sweep, the old y in a backward one
                    const int32_t e = ent ? ent[k] : k;
                    const int32_t j = col[e], pj = pos ? pos[j] : j;
                    if (FORWARD ? pj > pi : pj < pi) sigma = sigma + val[e] * (FORWARD ? x[j] : sor_ld(y + j));
                }
            const double xi = x[i];
            const double t = (xi - sigma) * inv_diag[i];
            const double out = FORWARD ? t : om1 * xi + omega * t;
            sor_st(y + i, alive ? out : nan);
        }
        if (g + 1 < ngroups && alive) alive = sor_grid_barrier(cnt, (uint32_t)g + 1u, gave_up, &ok_s);
    }
}

// the parameters, 1 / (a_ii + fshift), and per sweep direction (0 forward, 1 backward) the rows ordered by dependency level of the
// (coloured) sweep order with the level offsets
struct SorPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_SOR;
    double omega; int32_t its, sym;
    double* d_inv_diag = nullptr;
    int32_t* d_rows[2] = {nullptr, nullptr}; int32_t* d_off[2] = {nullptr, nullptr};
    int32_t groups[2] = {0, 0}; uint32_t grid[2] = {1, 1};
    int32_t* d_pos = nullptr;         // coloured order: the position of every row, or nullptr (position = row)
    int32_t* d_ent = nullptr;         // coloured order: every row's entries in ascending position, or nullptr (the stored order)
    uint32_t* d_sync = nullptr;       // the arrival counter of the sweep kernel's grid barrier, zeroed in front of every launch
    uint32_t* h_gave_up = nullptr; uint32_t* d_gave_up = nullptr;   // mapped host word: a barrier's patience ran out (sticky until read)
    SorPc(kryst_csr_t a_, double omega_, int32_t its_, int32_t sym_) : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), omega(omega_), its(its_), sym(sym_) {}
    ~SorPc() override {
        for (int d = 0; d < 2; ++d) { (void)pool_free(d_rows[d]); (void)pool_free(d_off[d]); }
        (void)pool_free(d_pos); (void)pool_free(d_ent);
        (void)hipFree(d_inv_diag); (void)hipFree(d_sync);
        if (h_gave_up) (void)hipHostFree(h_gave_up);
    }
    void launch(bool forward, bool eis, const double* x, double* y, const int* done);
    int32_t apply(int64_t nv, const double* x, double* y, const int* done) override;
    int32_t health() override;        // after the stream has been synchronised: did a sweep since the last call give up?
    bool check_after_apply() const override { return true; }
};

void SorPc::launch(bool forward, bool eis, const double* x, double* y, const int* done) {
    const int d = forward ? 0 : 1;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid[d]), dim3(KR_SOR_T), 0, ctx->s_main, (const int32_t*)a->d_row_ptr, (const int32_t*)a->d_col,
                           (const double*)a->d_val, (const double*)d_inv_diag, (const int32_t*)d_pos, (const int32_t*)d_ent, (const int32_t*)d_rows[d],
                           (const int32_t*)d_off[d], groups[d], omega, x, y, d_sync, d_gave_up, done);
    };
    if (forward) { if (eis) go(sor_sweep_kernel<true, true>); else go(sor_sweep_kernel<true, false>); }
    else { if (eis) go(sor_sweep_kernel<false, true>); else go(sor_sweep_kernel<false, false>); }
}

int32_t SorPc::apply(int64_t, const double* x, double* y, const int* done) {
    KR_ARG(x != y, "SOR apply: input and output must be different vectors");
    if (n == 0) return KRYST_OK;
    const bool lower = (sym & KR_SOR_LOWER) != 0, upper = (sym & KR_SOR_UPPER) != 0, eis = (sym & KR_SOR_EISENSTAT) != 0;
    const bool sweeps = its > 0 && (lower || upper);
    // y = +0.0 (sor.rs:127).  A forward sweep reads no y it has not written itself, so with one the zeroes would never be looked at.
    if (!sweeps || !lower) {
        hipLaunchKernelGGL(sor_zero_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->s_main, y, n, done);
        KR_HIP(hipGetLastError());
    }
    if (!sweeps) return KRYST_OK;
    for (int32_t it = 0; it < its; ++it) {
        if (lower) {
            KR_HIP(hipMemsetAsync(d_sync, 0, 16, ctx->s_main));      // (a whole 16-byte block at the start of its allocation)
            launch(true, eis, x, y, done);
            KR_HIP(hipGetLastError());
        }
        if (upper) {
            KR_HIP(hipMemsetAsync(d_sync, 0, 16, ctx->s_main));      // (a whole 16-byte block at the start of its allocation)
            launch(false, eis, x, y, done);
            KR_HIP(hipGetLastError());
        }
    }
    return KRYST_OK;
}

int32_t SorPc::health() {
    if (!h_gave_up || *(volatile uint32_t*)h_gave_up == 0u) return KRYST_OK;
    *(volatile uint32_t*)h_gave_up = 0u;
    set_error("SOR: a sweep's grid barrier was abandoned (the device is shared or time-sliced); the result holds NaNs");
    return KRYST_SOLVE_ERROR;
}

template <class T> static int32_t sor_upload(kryst_ctx_t ctx, T** d, const std::vector<T>& h, const char* what) {
    if (pool_malloc(d, sizeof(T) * std::max<size_t>(h.size(), 1)) != hipSuccess) {
        (void)hipGetLastError();
        *d = nullptr;
        set_error("SOR: out of device memory (%s)", what);
        return KRYST_ERR_HIP;
    }
    if (!h.empty()) KR_HIP(hipMemcpyAsync(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->s_main));
    return KRYST_OK;
}

// The schedule of one sweep direction: the dependencies of every row in sweep-order positions -- the stored entries before it (forward) or
// after it (backward) in the order, whose new values it reads -- their levels, and the rows ordered by (level, position).  `anti` (a
// backward sweep without EISENSTAT): row i also reads the OLD y_j of every stored j before it in the order, so j has to wait for i as
// well; with a symmetric pattern j does anyway.  order[p]: the row at position p; pos: its inverse.
static int32_t sor_schedule(int64_t n, const std::vector<int32_t>& rp, const std::vector<int32_t>& col, const std::vector<int32_t>& order,
                            const std::vector<int32_t>& pos, bool forward, bool anti, std::vector<int32_t>& rows, std::vector<int32_t>& off) {
    std::vector<int64_t> tp((size_t)n + 1, 0);
    auto each = [&](auto&& f) {                                          // f(p, q): position p waits for position q
        for (int64_t i = 0; i < n; ++i) {
            const int32_t p = pos[(size_t)i];
            for (int32_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) {
                const int32_t q = pos[(size_t)col[(size_t)k]];
                if (forward ? q < p : q > p) f(p, q);
                else if (anti && q < p) f(q, p);
            }
        }
    };
    each([&](int32_t p, int32_t) { ++tp[(size_t)p + 1]; });
    for (int64_t p = 0; p < n; ++p) tp[(size_t)p + 1] += tp[(size_t)p];
    std::vector<int32_t> tc((size_t)tp[(size_t)n]);
    {
        std::vector<int64_t> w(tp.begin(), tp.end() - 1);
        each([&](int32_t p, int32_t q) { tc[(size_t)w[(size_t)p]++] = q; });
    }
    std::vector<int32_t> lvl((size_t)std::max<int64_t>(n, 1), 0);
    const int32_t nl = n > 0 ? host_levels(n, tp.data(), tc.data(), forward, lvl.data()) : 0;      // (host_factor.cpp)
    off.assign((size_t)nl + 1, 0);
    for (int64_t p = 0; p < n; ++p) ++off[(size_t)lvl[(size_t)p] + 1];
    for (int32_t l = 0; l < nl; ++l) off[(size_t)l + 1] += off[(size_t)l];
    rows.resize((size_t)n);
    std::vector<int32_t> fill(off.begin(), off.end() - (nl > 0 ? 1 : 0));
    // inside a level the rows in sweep order: ascending position forward, descending backward (any order gives the same bits)
    if (forward) for (int64_t p = 0; p < n; ++p) rows[(size_t)fill[(size_t)lvl[(size_t)p]]++] = order[(size_t)p];
    else for (int64_t p = n - 1; p >= 0; --p) rows[(size_t)fill[(size_t)lvl[(size_t)p]]++] = order[(size_t)p];
    return nl;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_sor(kryst_csr_t a, double omega, int64_t its, int64_t lits, uint32_t sym_bits, double fshift, const int32_t* colors, kryst_pc_t* out) {
    KR_ARG(a && out, "pc_sor");
    if (a->dist) { set_error("SOR: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->ncols && a->nrows == a->xlen, "pc_sor: square operator required");
    KR_ARG(a->nrows < INT32_MAX, "pc_sor: more than 2^31 - 1 rows");
    KR_ARG(its >= 0 && its < INT32_MAX && lits >= 0 && lits < INT32_MAX, "pc_sor: its or lits out of range");
    KR_ARG(sym_bits < 64u, "pc_sor: unknown MatSorType bits");
    const int64_t n = a->nrows;
    if (colors)
        for (int64_t i = 0; i < n; ++i) KR_ARG(colors[i] >= 0, "pc_sor: negative colour");
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    SorPc* pc = new SorPc(a, omega, (int32_t)its, (int32_t)sym_bits);
    unsigned long long* d_err = nullptr;
    unsigned long long e = ~0ull;
    auto fail = [&](int32_t rc) { (void)hipStreamSynchronize(ctx->s_main); (void)hipFree(d_err); kryst_pc_destroy(pc); return rc; };
    // ---- the diagonal (device)
    if (hipMalloc(&pc->d_inv_diag, sizeof(double) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess || hipMalloc(&d_err, sizeof e) != hipSuccess ||
        hipMalloc(&pc->d_sync, 16) != hipSuccess ||
        hipHostMalloc((void**)&pc->h_gave_up, sizeof(uint32_t), hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError(); set_error("SOR: out of device memory (%lld rows)", (long long)n); return fail(KRYST_ERR_HIP);
    }
    *pc->h_gave_up = 0u;
    if (hipHostGetDevicePointer((void**)&pc->d_gave_up, pc->h_gave_up, 0) != hipSuccess ||
        hipMemsetAsync(d_err, 0xFF, sizeof e, ctx->s_main) != hipSuccess) { set_error("SOR: set-up failed on the device"); return fail(KRYST_ERR_HIP); }
    if (n > 0) {
        hipLaunchKernelGGL(sor_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->s_main, (const int32_t*)a->d_row_ptr,
                           (const int32_t*)a->d_col, (const double*)a->d_val, (int32_t)n, fshift, pc->d_inv_diag, d_err);
        if (hipGetLastError() != hipSuccess) { set_error("SOR: set-up launch failed"); return fail(KRYST_ERR_HIP); }
    }
    // ---- the pattern (host): sweep order, dependency levels per direction
    std::vector<int32_t> rp((size_t)n + 1, 0), col((size_t)a->nnz);
    if (hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
        hipMemcpyAsync(rp.data(), a->d_row_ptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
        (a->nnz > 0 && hipMemcpyAsync(col.data(), a->d_col, sizeof(int32_t) * col.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess) ||
        hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("SOR: set-up failed on the device"); return fail(KRYST_ERR_HIP); }
    if (e != ~0ull) {
        set_error("SOR: a_ii + fshift is zero at row %lld", (long long)e);
        set_error_row((int64_t)e);
        return fail(KRYST_ZERO_PIVOT);
    }
    std::vector<int32_t> order((size_t)n), pos((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    if (colors) std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return colors[x] < colors[y]; });
    for (int64_t p = 0; p < n; ++p) pos[(size_t)order[(size_t)p]] = (int32_t)p;
    int32_t rc = KRYST_OK;
    if (colors) {
        std::vector<int32_t> ent(col.size());                            // every row's entries in ascending position
        std::iota(ent.begin(), ent.end(), 0);
        for (int64_t i = 0; i < n; ++i)
            std::sort(ent.begin() + rp[(size_t)i], ent.begin() + rp[(size_t)i + 1],
                      [&](int32_t u, int32_t v) { return pos[(size_t)col[(size_t)u]] < pos[(size_t)col[(size_t)v]]; });
        rc = sor_upload(ctx, &pc->d_pos, pos, "sweep order");
        if (rc == KRYST_OK) rc = sor_upload(ctx, &pc->d_ent, ent, "entry order");
        if (rc == KRYST_OK && hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("SOR: set-up failed on the device"); rc = KRYST_ERR_HIP; }
    }
    const bool need[2] = {(sym_bits & KR_SOR_LOWER) != 0, (sym_bits & KR_SOR_UPPER) != 0};
    for (int d = 0; d < 2 && rc == KRYST_OK; ++d) {
        if (!need[d]) continue;
        std::vector<int32_t> rows, off;
        pc->groups[d] = sor_schedule(n, rp, col, order, pos, d == 0, d == 1 && !(sym_bits & KR_SOR_EISENSTAT), rows, off);
        int32_t maxw = 1;
        for (int32_t g = 0; g < pc->groups[d]; ++g) maxw = std::max(maxw, off[(size_t)g + 1] - off[(size_t)g]);
        // one workgroup per CU at most: all of them resident, whatever else the kernel needs
        pc->grid[d] = (uint32_t)std::max(1, std::min(ctx->num_cu, (maxw + KR_SOR_T - 1) / KR_SOR_T));
        if ((unsigned long long)pc->groups[d] * pc->grid[d] >= (1ull << 32)) {       // the barrier's arrival count is 32 bits
            set_error("SOR: %d dependency levels times %u workgroups do not fit the barrier's counter", pc->groups[d], pc->grid[d]);
            rc = KRYST_UNSUPPORTED; break;
        }
        rc = sor_upload(ctx, &pc->d_rows[d], rows, "rows by level");
        if (rc == KRYST_OK) rc = sor_upload(ctx, &pc->d_off[d], off, "level offsets");
        if (rc == KRYST_OK && hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("SOR: set-up failed on the device"); rc = KRYST_ERR_HIP; }
    }
    if (rc == KRYST_OK && hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("SOR: set-up failed on the device"); rc = KRYST_ERR_HIP; }
    if (rc != KRYST_OK) return fail(rc);
    (void)hipFree(d_err);
    *out = pc;
    return KRYST_OK;
}

int32_t kryst_pc_sor_info(kryst_pc_t h, int32_t* groups_forward, int32_t* groups_backward, int64_t* rows, int32_t* grid_forward,
                          int32_t* grid_backward) {
    SorPc* pc = pc_cast<SorPc>(h);
    KR_ARG(pc, "pc_sor_info");
    if (groups_forward) *groups_forward = pc->groups[0];
    if (groups_backward) *groups_backward = pc->groups[1];
    if (rows) *rows = pc->n;
    if (grid_forward) *grid_forward = pc->groups[0] ? (int32_t)pc->grid[0] : 0;
    if (grid_backward) *grid_backward = pc->groups[1] ? (int32_t)pc->grid[1] : 0;
    return KRYST_OK;
}

int32_t kryst_host_color_graph(int64_t n, const int64_t* ptr, const int32_t* col, int32_t* colors, int32_t* ncolors) {
    KR_ARG(n >= 0 && n < INT32_MAX && ptr && (n == 0 || colors) && (ptr[n] == 0 || col), "host_color_graph");
    for (int64_t i = 0; i < n; ++i) {
        KR_ARG(ptr[i + 1] >= ptr[i], "host_color_graph: ptr is not ascending");
        for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) KR_ARG(col[k] >= 0 && col[k] < n, "host_color_graph: column out of range");
    }
    const int32_t nc = host_color_graph(n, ptr, col, colors);
    if (ncolors) *ncolors = nc;
    return KRYST_OK;
}

}  // extern "C"
