// Device-side set-up of ILU(0) (overview: ilu.hip): grid operators and general operators are factored without their values leaving the
// GPU; the IKJ factorisation alone for operators that then take the host path.  The kernels stay in the global namespace.
#include "ilu.h"

using namespace kr;

// ---------------------------------------------------------------------------------------------------------------------------
// Device-side setup for grid operators.  A matrix whose stored entries couple row (i,j,k) of an Ni x Nj x Nk box only to itself
// and its six axis neighbours, in natural ordering (recognised from the CSR-D8 offset dictionary: at most the offsets 0, +-1,
// +-Ni, +-Ni*Nj, no entry wrapping around a line end), never leaves the GPU: one pass pulls the seven coefficient streams out
// of the CSR arrays, the compat / Ilup(0) factors are pointwise quotients, and the textbook ILU(0) -- on this pattern only the
// DIAGONAL is ever updated, u_dd(i) = a_dd - sum_c l_ic u_ci over the lower neighbours c in ascending column order -- is a
// recurrence over the hyperplanes i + j + k = const: one small launch per plane (766 at 256^3, ~3 ms).  Same operations in the
// same order as the host loops above (which remain for every other matrix): same bits.  256^3: 1.8 s -> a few ms.
struct GridStreams {                 // natural row order, n entries each; absent entry = 0.0 and its presence bit clear
    double *km, *jm, *im, *dd, *ip, *jp, *kp; uint8_t* have;     // presence bits: 0 km, 1 jm, 2 im, 3 dd, 4 ip, 5 jp, 6 kp
};

__global__ __launch_bounds__(256) void grid_extract_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                           int64_t n, int32_t s1, int64_t s2, GridStreams G, int32_t* reject) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    unsigned have = 0;
    const int32_t ii = (int32_t)(i % s1), jx = (int32_t)((i / s1) % (s2 / s1));
    const int32_t nj = (int32_t)(s2 / s1);
    bool bad = false;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int64_t o = (int64_t)col[k] - i;
        int slot = -1;
        if (o == -s2) slot = 0; else if (o == -(int64_t)s1) slot = 1; else if (o == -1) slot = 2; else if (o == 0) slot = 3;
        else if (o == 1) slot = 4; else if (o == (int64_t)s1) slot = 5; else if (o == s2) slot = 6;
        if (slot < 0) { bad = true; continue; }
        // an entry must stay on its grid line / plane (a band that wraps around a line end is not a grid operator)
        if ((slot == 2 && ii == 0) || (slot == 4 && ii == s1 - 1) || (slot == 1 && jx == 0) || (slot == 5 && jx == nj - 1)) bad = true;
        v[slot] = val[k]; have |= 1u << slot;
    }
    if (bad) atomicOr(reject, 1);
    G.km[i] = v[0]; G.jm[i] = v[1]; G.im[i] = v[2]; G.dd[i] = v[3]; G.ip[i] = v[4]; G.jp[i] = v[5]; G.kp[i] = v[6];
    G.have[i] = (uint8_t)have;
}

// which of the 256 offset codes occur at all (the stencil generator's dictionary also lists halo offsets it may not use)
__global__ __launch_bounds__(256) void code_usage_kernel(const uint8_t* __restrict__ code, int64_t nnz, int32_t* used) {
    __shared__ int32_t mine[256];
    mine[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) mine[code[k]] = 1;
    __syncthreads();
    if (mine[threadIdx.x]) used[threadIdx.x] = 1;
}

// Ilu0 as written (mode 0) and Ilup::new(0) (mode 1): l_ij = a_ij / a_jj for stored nonzeros below the diagonal, U = triu(A)
// (ilu.rs:76-80, ilup.rs:104-111); bad_row: lowest row whose pivot is zero (Ilup only, ilup.rs:106-108)
__global__ __launch_bounds__(256) void grid_pointwise_factor_kernel(GridStreams G, int64_t n, int32_t s1, int64_t s2, int mode,
                                                                    double* l1, double* l2, double* l3, double* u1, double* u2, double* u3, double* dg,
                                                                    long long* bad_row) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned have = G.have[i];
    const double a[3] = {G.km[i], G.jm[i], G.im[i]};
    const int64_t nb[3] = {i - s2, i - s1, i - 1};
    double l[3];
    bool zero_pivot = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        l[c] = 0.0;
        if (((have >> c) & 1u) && a[c] != 0.0) {
            const double ujj = (G.have[nb[c]] & 8u) ? G.dd[nb[c]] : 0.0;
            if (mode == KRYST_ILU_ILUP0 && ujj == 0.0) zero_pivot = true;
            l[c] = a[c] / ujj;
        }
    }
    if (zero_pivot) atomicMin((unsigned long long*)bad_row, (unsigned long long)i);
    auto kept = [](double x) { return x == 0.0 ? 0.0 : x; };               // a zero entry (either sign) is not kept: +0.0 = "no entry"
    l3[i] = kept(l[0]); l2[i] = kept(l[1]); l1[i] = kept(l[2]);            // coefficient of the k- / j- / i-neighbour
    u1[i] = kept(G.ip[i]); u2[i] = kept(G.jp[i]); u3[i] = kept(G.kp[i]);
    dg[i] = (mode != KRYST_ILU_KRYST_COMPAT && (have & 8u)) ? G.dd[i] : 1.0;   // ilu.rs:115-119 never divides; ilup.rs:160-164 (missing diagonal: no divide)
}

// Textbook ILU(0), the rows of ONE hyperplane (they only need lower planes): the host loop's operations in its order --
// for c ascending: pivot check, l = a_ic / u_cc, then u_ii -= l * u_ci when row c reaches i and row i has a diagonal.
__global__ __launch_bounds__(256) void grid_true_ilu0_plane_kernel(GridStreams G, int32_t Ni, int32_t Nj, int32_t Nk, int level,
                                                                   double* wdd, double* l1, double* l2, double* l3, long long* bad_key) {
    const int jk = blockIdx.x * 256 + threadIdx.x;
    if (jk >= Nj * Nk) return;
    const int j = jk % Nj, k = jk / Nj, ii = level - j - k;
    if (ii < 0 || ii >= Ni) return;
    const int64_t s1 = Ni, s2 = (int64_t)Ni * Nj, i = ii + s1 * j + s2 * k;
    const unsigned have = G.have[i];
    const double a[3] = {G.km[i], G.jm[i], G.im[i]};
    const int64_t nb[3] = {i - s2, i - s1, i - 1};
    const double* up[3] = {G.kp, G.jp, G.ip};                              // row c's entry that points at row i
    const unsigned upbit[3] = {64u, 32u, 16u};
    double wd = G.dd[i];
    double l[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!((have >> c) & 1u)) continue;
        const unsigned hc = G.have[nb[c]];
        const double piv = wdd[nb[c]];
        if (!(hc & 8u) || piv == 0.0) atomicMin((unsigned long long*)bad_key, (unsigned long long)(i * 4 + c));
        l[c] = a[c] / piv;
        if ((hc & upbit[c]) && (have & 8u)) wd = wd - l[c] * up[c][nb[c]];
    }
    wdd[i] = wd;
    auto kept = [](double x) { return x == 0.0 ? 0.0 : x; };
    l3[i] = kept(l[0]); l2[i] = kept(l[1]); l1[i] = kept(l[2]);
}

// -> KRYST_OK and *out set when the operator was handled on the device; *out left null when it is not a grid operator (the host
// path takes over); an error code for a zero pivot.
int32_t kr::grid_setup_on_device(kryst_csr_t a, int mode, kryst_pc_t* out) {
    *out = nullptr;
    kryst_ctx_t ctx = a->ctx;
    const int64_t n = a->nrows;
    if (a->dist || !a->d_dict || !a->d_code || n < 27 || n >= (1ll << 31) || env_int("KRYST_ILU_GRID", 1) == 0 || env_int("KRYST_ILU_DEVICE_SETUP", 1) == 0)
        return KRYST_OK;
    int32_t dict[256], used[256];
    {
        int32_t* d_used = nullptr;
        KR_HIP(pool_malloc(&d_used, sizeof used));
        (void)hipMemsetAsync(d_used, 0, sizeof used, ctx->s_main);
        hipLaunchKernelGGL(code_usage_kernel, dim3((unsigned)std::min<int64_t>(4096, (a->nnz + 255) / 256 + 1)), dim3(256), 0, ctx->s_main, a->d_code, a->nnz, d_used);
        const hipError_t e1 = hipMemcpyAsync(used, d_used, sizeof used, hipMemcpyDeviceToHost, ctx->s_main);
        const hipError_t e2 = hipMemcpyAsync(dict, a->d_dict, sizeof dict, hipMemcpyDeviceToHost, ctx->s_main);
        const hipError_t e3 = hipStreamSynchronize(ctx->s_main);
        (void)pool_free(d_used);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { set_error("code usage scan failed"); return KRYST_ERR_HIP; }
    }
    int64_t offs[3] = {0, 0, 0}; int no = 0;
    for (int q = 0; q < 256; ++q) {
        if (!used[q]) continue;
        const int64_t ao = dict[q] < 0 ? -(int64_t)dict[q] : dict[q];
        if (ao == 0) continue;
        bool seen = false;
        for (int r = 0; r < no; ++r) seen = seen || offs[r] == ao;
        if (!seen) { if (no == 3) return KRYST_OK; offs[no++] = ao; }
    }
    std::sort(offs, offs + no);
    if (no < 2 || offs[0] != 1) return KRYST_OK;
    const int64_t s1 = offs[1], s2 = no == 3 ? offs[2] : n;
    // Ni >= 3 and Nj >= 3 (in 3-D): with a dimension of 2 a lower neighbour's row reaches a SECOND entry of row i and the
    // elimination is no longer confined to the diagonal
    if (s1 < 3 || s2 % s1 != 0 || n % s2 != 0 || s2 <= s1 || (no == 3 && s2 / s1 < 3)) return KRYST_OK;
    const int32_t Ni = (int32_t)s1, Nj = (int32_t)(s2 / s1), Nk = (int32_t)(n / s2);
    const bool verbose = getenv("KRYST_ILU_VERBOSE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // ---- seven coefficient streams + presence bits
    GridStreams G{};
    double* work[8] = {};
    struct Guard { double** w; uint8_t** h; long long** f; int32_t** r; ~Guard() { for (int i = 0; i < 8; ++i) (void)pool_free(w[i]); (void)pool_free(*h); (void)pool_free(*f); (void)pool_free(*r); } };
    uint8_t* d_have = nullptr; long long* d_flag = nullptr; int32_t* d_reject = nullptr;
    Guard guard{work, &d_have, &d_flag, &d_reject};
    const size_t vb = sizeof(double) * (size_t)(n + 8);
    for (int q = 0; q < 8; ++q) KR_HIP(pool_malloc(&work[q], vb));
    KR_HIP(pool_malloc(&d_have, (size_t)n + 8)); KR_HIP(pool_malloc(&d_flag, 16)); KR_HIP(pool_malloc(&d_reject, 4));
    KR_HIP(hipMemsetAsync(d_reject, 0, 4, ctx->s_main));
    KR_HIP(hipMemsetAsync(d_flag, 0xff, 16, ctx->s_main));
    G.km = work[0]; G.jm = work[1]; G.im = work[2]; G.dd = work[3]; G.ip = work[4]; G.jp = work[5]; G.kp = work[6]; G.have = d_have;
    const unsigned rg = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(grid_extract_kernel, dim3(rg), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, n, Ni, s2, G, d_reject);
    KR_HIP(hipGetLastError());
    int32_t reject = 0;
    KR_HIP(hipMemcpyAsync(&reject, d_reject, 4, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    if (reject) return KRYST_OK;                                           // bands that wrap around line ends: the host path (level-ordered)
    // ---- the preconditioner object with its natural-order factor streams
    IluPc* pc = new IluPc(a);
    int32_t rc = KRYST_OK;
    for (double** pp : {&pc->GL.d_c1, &pc->GL.d_c2, &pc->GL.d_c3, &pc->GU.d_c1, &pc->GU.d_c2, &pc->GU.d_c3, &pc->GU.d_diag})
        if (rc == KRYST_OK && pool_malloc(pp, vb) != hipSuccess) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
    if (rc == KRYST_OK) {
        if (mode == KRYST_ILU_TRUE_ILU0) {
            double* wdd = work[7];
            const unsigned pg = (unsigned)(((int64_t)Nj * Nk + 255) / 256);
            for (int lv = 0; lv < Ni + Nj + Nk - 2; ++lv)
                hipLaunchKernelGGL(grid_true_ilu0_plane_kernel, dim3(pg), dim3(256), 0, ctx->s_main, G, Ni, Nj, Nk, lv, wdd, pc->GL.d_c1, pc->GL.d_c2, pc->GL.d_c3, d_flag);
            // U = the upper entries of A (never touched on this pattern) and, as divisor, the eliminated diagonal where the row
            // has one, else 1 (ilup.rs:160-164): the pointwise kernel with the eliminated diagonal in place of A's (mode -1: its
            // L outputs go to scratch that is no longer needed)
            hipLaunchKernelGGL(grid_pointwise_factor_kernel, dim3(rg), dim3(256), 0, ctx->s_main,
                               GridStreams{G.km, G.jm, G.im, wdd, G.ip, G.jp, G.kp, G.have}, n, Ni, s2, -1,
                               work[0], work[1], work[2], pc->GU.d_c1, pc->GU.d_c2, pc->GU.d_c3, pc->GU.d_diag, d_flag + 1);
        } else {
            hipLaunchKernelGGL(grid_pointwise_factor_kernel, dim3(rg), dim3(256), 0, ctx->s_main, G, n, Ni, s2, mode,
                               pc->GL.d_c1, pc->GL.d_c2, pc->GL.d_c3, pc->GU.d_c1, pc->GU.d_c2, pc->GU.d_c3, pc->GU.d_diag, d_flag);
        }
        if (rc == KRYST_OK && hipGetLastError() != hipSuccess) rc = KRYST_ERR_HIP;
    }
    long long flag[2] = {-1, -1};
    if (rc == KRYST_OK && (hipMemcpyAsync(flag, d_flag, 16, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK && flag[0] != -1) {
        if (mode == KRYST_ILU_TRUE_ILU0) {
            const long long i = flag[0] / 4; const int c = (int)(flag[0] % 4);
            const long long row = c == 0 ? i - s2 : c == 1 ? i - s1 : i - 1;
            set_error("ILU(0): zero pivot at row %lld", row); set_error_row(row); rc = KRYST_ZERO_PIVOT;
        } else { set_error("ILUP: zero diagonal in U (first at row %lld)", flag[0]); rc = KRYST_SOLVE_ERROR; }
    }
    if (rc == KRYST_OK) {
        pc->GL.Ni = pc->GU.Ni = Ni; pc->GL.Nj = pc->GU.Nj = Nj; pc->GL.Nk = pc->GU.Nk = Nk; pc->GL.ok = pc->GU.ok = true;
        rc = finish_ilu_device(pc);
    }
    if (verbose) fprintf(stderr, "[kryst ilu] device-side setup of a %d x %d x %d grid operator: %.1f ms\n", Ni, Nj, Nk,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Device-side IKJ factorisation of a GENERAL sparse operator (true ILU(0) on A's pattern; the pointwise kryst-compat / Ilup(0)
// quotients need no elimination and stay parallel host loops).  ONE WAVE PER ROW: the row's entries sit in LDS, its lower entries
// are taken in stored order, and for each the pivot row's entries are spread over the lanes -- lane t looks its column up in the
// row and subtracts there (a pivot row's columns are distinct, so no two lanes touch one entry; each entry receives its updates in
// pivot order: the host loop's operations in the host loop's order, bit for bit).  Rows run concurrently as far as the dependency
// graph allows: the wave polls the "row c is final" flag of the pivot row it needs next.  Waves take the rows in DEPENDENCY-LEVEL
// order (levels of A's lower pattern, computed on the host from the row pointers and columns it has anyway: in natural order the
// few thousand rows in flight are a thin slice of the graph, 100+ levels deep, and the launch crawls): a pivot row sits at a
// smaller position, workgroups start in index order, so the lowest unfinished workgroup only waits for finished ones; a poll
// budget turns a scheduling surprise into a clean fallback to the host loop.  Rows longer than 64 entries: host loop.
__global__ __launch_bounds__(256) void ilu0_dpos_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, int32_t n, int32_t* dpos, int32_t* rowdone) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t d = -1;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) if (col[k] == i) d = k;
    dpos[i] = d; rowdone[i] = 0;
}
__global__ __launch_bounds__(256) void ilu0_ikj_wave_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, double* w,
                                                            const int32_t* __restrict__ dpos, const int32_t* __restrict__ order, int32_t n, int32_t* rowdone,
                                                            unsigned long long* first_bad, int32_t* stalled, int budget0, int ascending) {
    __shared__ int32_t lcol_all[4 * 64];
    __shared__ double lw_all[4 * 64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int32_t pos = blockIdx.x * 4 + wv;
    if (pos >= n) return;                                                  // (uniform over the wave; no workgroup barrier anywhere)
    const int32_t i = order[pos];                                          // rows in dependency-level order: a pivot row sits at a smaller position
    int32_t* const lcol = lcol_all + 64 * wv;
    double* const lw = lw_all + 64 * wv;
    const int32_t kbeg = rp[i], len = rp[i + 1] - kbeg;                    // len <= 64 (checked on the host)
    lcol[l] = l < len ? col[kbeg + l] : 0x7fffffff;
    lw[l] = l < len ? w[kbeg + l] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int e = 0; e < len; ++e) {
        const int32_t c = lcol[e];                                         // (the same word for every lane)
        if (c >= n) continue;                                              // halo column (another rank's row): not part of this block
        if (c >= i) break;
        int budget = budget0;
        while (__hip_atomic_load(&rowdone[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            if (--budget <= 0) break;
            __builtin_amdgcn_s_sleep(1);
        }
        if (budget <= 0) { if (l == 0) __hip_atomic_store(stalled, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }   // the host loop takes over
        // (no acquire fence: everything another wave has written -- pivot and pivot row -- is read with agent-scope loads below;
        // an agent-scope fence writes back / invalidates the whole L2 on this chip, and thirteen of them per row made the launch
        // 190 ms instead of a few)
        const int32_t kd = dpos[c];
        const double pivot = kd >= 0 ? __hip_atomic_load(&w[kd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        if (kd < 0 || pivot == 0.0) {
            // the sequential loop stops at the first (row, entry) that meets a zero pivot and names the PIVOT row
            if (l == 0) atomicMin(first_bad, ((unsigned long long)(unsigned)i << 32) | (unsigned)c);
            break;
        }
        const double lik = lw[e] / pivot;
        __builtin_amdgcn_wave_barrier();                                   // (every lane has read lw[e] before lane 0 replaces it)
        if (l == 0) lw[e] = lik;
        const int32_t cb = rp[c], clen = rp[c + 1] - cb;
        for (int32_t o = 0; o < clen; o += 64) {
            const bool has = o + l < clen;
            const int32_t j = has ? col[cb + o + l] : -1;
            const double wc = has ? __hip_atomic_load(&w[cb + o + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            if (j > c && j < n) {
                // where column j sits in this row, if it does: the row's columns ascend (kryst_csr_create), the slots behind them hold INT_MAX --
                // six halvings of the 64 slots instead of a walk over the row (a 27-point row: 13 pivot rows x 27 compares per lane)
                // (a row block of a distributed operator stores its lower neighbour's halo columns FIRST and numbers them n + h: not ascending, walked)
                if (ascending) {
                    int p = 0;
#pragma unroll
                    for (int step = 32; step >= 1; step >>= 1) if (lcol[p + step] <= j) p += step;
                    if (lcol[p] == j) lw[p] = lw[p] - lik * wc;
                } else {
                    for (int p = 0; p < len; ++p)
                        if (lcol[p] == j) { lw[p] = lw[p] - lik * wc; break; }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // this row's values before its flag: write-through (agent-scope) stores, waited for, then the flag -- no L2-wide release fence
    if (l < len) __hip_atomic_store(&w[kbeg + l], lw[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // the stores have been acknowledged (a workgroup-scope release fence
    __builtin_amdgcn_wave_barrier();                                       // does not wait for vector stores on this target: the flag overtook them)
    if (l == 0) __hip_atomic_store(&rowdone[i], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (also after a failure: nobody must wait for this row)
}

// w <- the true ILU(0) factor values on A's pattern, computed on the device and copied to the host vector `w` (which holds A's
// values on entry).  *used = false when the device path did not run to completion (the caller then runs the host loop).
int32_t kr::ikj_on_device(kryst_csr_t a, const std::vector<int64_t>& rp, const std::vector<int32_t>& col, std::vector<double>& w, bool* used, int64_t* bad_row) {
    *used = false; *bad_row = -1;
    kryst_ctx_t ctx = a->ctx;
    const int64_t n = a->nrows, nnz = a->nnz;
    if (n == 0 || nnz == 0 || n >= (1ll << 31) - 4 || env_int("KRYST_ILU_DEVICE_SETUP", 1) == 0) return KRYST_OK;
    for (int64_t i = 0; i < n; ++i) if (rp[i + 1] - rp[i] > 64) return KRYST_OK;       // (a row must fit one wave's LDS slice)
    const bool verbose = getenv("KRYST_ILU_VERBOSE") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto t0 = tnow();
    auto lap = [&](const char* what) { if (verbose) { fprintf(stderr, "[kryst ilu]   ikj: %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(tnow() - t0).count()); t0 = tnow(); } };
    // dependency levels of the lower pattern (local columns below the diagonal), rows ordered by (level, row)
    std::vector<int32_t> order((size_t)n);
    {
        std::vector<int32_t> lvl((size_t)n, 0), cnt;
        int32_t nl = 0;
        for (int64_t i = 0; i < n; ++i) {
            int32_t lv = 0;
            for (int64_t k = rp[i]; k < rp[i + 1]; ++k) { const int32_t c = col[k]; if (c < i) lv = std::max(lv, lvl[c] + 1); }   // (halo columns are >= n > i)
            lvl[i] = lv; nl = std::max(nl, lv + 1);
        }
        cnt.assign((size_t)nl + 1, 0);
        for (int64_t i = 0; i < n; ++i) cnt[lvl[i] + 1]++;
        for (int32_t q = 0; q < nl; ++q) cnt[q + 1] += cnt[q];
        for (int64_t i = 0; i < n; ++i) order[cnt[lvl[i]]++] = (int32_t)i;
    }
    lap("levels on the host");
    struct Tmp { double* w = nullptr; int32_t* dpos = nullptr; int32_t* done = nullptr; int32_t* order = nullptr; unsigned long long* bad = nullptr;
                 ~Tmp() { (void)pool_free(w); (void)pool_free(dpos); (void)pool_free(done); (void)pool_free(order); (void)pool_free(bad); } } t;
    if (pool_malloc(&t.w, sizeof(double) * (size_t)nnz) != hipSuccess || pool_malloc(&t.dpos, sizeof(int32_t) * (size_t)n) != hipSuccess ||
        pool_malloc(&t.done, sizeof(int32_t) * (size_t)n) != hipSuccess || pool_malloc(&t.order, sizeof(int32_t) * (size_t)n) != hipSuccess ||
        pool_malloc(&t.bad, 16) != hipSuccess) { (void)hipGetLastError(); return KRYST_OK; }
    KR_HIP(hipMemcpyAsync(t.order, order.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->s_main));
    KR_HIP(hipMemcpyAsync(t.w, a->d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->s_main));
    KR_HIP(hipMemsetAsync(t.bad, 0xff, 8, ctx->s_main));
    KR_HIP(hipMemsetAsync(t.bad + 1, 0, 8, ctx->s_main));
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(ilu0_dpos_kernel, dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, (int32_t)n, t.dpos, t.done);
    hipLaunchKernelGGL(ilu0_ikj_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, t.dpos, t.order, (int32_t)n, t.done,
                       t.bad, reinterpret_cast<int32_t*>(t.bad + 1), std::max(1, env_int("KRYST_ILU_SETUP_POLL_BUDGET", 1 << 22)), a->dist ? 0 : 1);
    KR_HIP(hipGetLastError());
    unsigned long long flags[2] = {0, 0};
    KR_HIP(hipMemcpyAsync(flags, t.bad, 16, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    lap("allocations, uploads, kernels");
    if ((int32_t)flags[1] != 0) return KRYST_OK;                       // stalled: host loop
    if (flags[0] != ~0ull) { *bad_row = (int64_t)(flags[0] & 0xffffffffull); *used = true; return KRYST_OK; }
    KR_HIP(hipMemcpyAsync(w.data(), t.w, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    lap("factor values to the host");
    *used = true;
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// GENERAL operators, everything on the device (round 3).  The host loops of kryst_pc_ilu0 download A, eliminate, split into L / U,
// level-order both factors and upload them again; here the VALUES never leave the GPU: the host gets A's pattern (row pointers and
// columns, 4 bytes per entry, once) and does the symbolic part -- dependency levels of the lower and the upper pattern, the rows by
// level, positions, row pointers -- while the device does everything that touches a value:
//   dpos / longest row -> factor values w (mode 2: ilu0_ikj_wave_kernel in the lower pattern's level order; modes 0 / 1: the pointwise
//   quotients) -> kept entries per row and the divisor (checked against the pattern: an operator whose factor DROPS entries -- stored or
//   computed zeros -- takes the host path) -> the factors written in level order straight from (A's pattern, w) -> finish_ilu_device.
// (Levels computed on the device by a sync-free launch in natural row order were tried first: half a million waiting lanes polling
// uncached flags made a 10 716-level band matrix take 1.07 s for what the host's two O(nnz) sweeps do in 40 ms.)
// Same kept entries, same stored order, same divisors as the host path: the apply is bit-identical (the tests run both).  Taken for
// operators -- a rank's diagonal block included: halo columns (>= n) are skipped everywhere -- that are not candidate grid operators
// (more than 7 distinct offsets, 9 for a distributed block; or no offset dictionary at all) and
// whose rows fit a wave (<= 64 entries); everything else, KRYST_ILU_DEVICE_SETUP=0 and any starved poll budget: the host path.
__global__ __launch_bounds__(256) void gen_rowmax_kernel(const int32_t* __restrict__ rp, int32_t n, int32_t* maxlen) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    int32_t len = i < n ? rp[i + 1] - rp[i] : 0;
    for (int off = 32; off >= 1; off >>= 1) len = max(len, __shfl_xor(len, off, 64));
    if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(maxlen, len);
}
// modes 0 / 1 (ilu.rs:76-80, ilup.rs:104-111): l_ij = a_ij / a_jj for stored nonzeros below the diagonal, everything else as stored
__global__ __launch_bounds__(256) void gen_pointwise_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                            const int32_t* __restrict__ dpos, int32_t n, int mode, double* w, unsigned long long* first_bad) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j < i && val[k] != 0.0) {
            const double ujj = dpos[j] >= 0 ? val[dpos[j]] : 0.0;
            if (mode == KRYST_ILU_ILUP0 && ujj == 0.0) { atomicMin(first_bad, ((unsigned long long)(unsigned)i << 32) | (unsigned)j); return; }   // ilup.rs:106-108
            w[k] = val[k] / ujj;
        }
    }
}
// kept entries (`!= T::zero()` filters, local columns only) below / above the diagonal and the backward solve's divisor
__global__ __launch_bounds__(256) void gen_classify_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ w,
                                                           int32_t n, int divide, int32_t* nl, int32_t* nu, double* dg) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t a = 0, b = 0; double d = 1.0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j >= n || w[k] == 0.0) continue;
        if (j < i) ++a; else if (j > i) ++b; else if (divide) d = w[k];                  // ilup.rs:160-164 (missing diagonal: no divide)
    }
    nl[i] = a; nu[i] = b; dg[i] = d;
}
// one factor in level order: position p holds row rowid[p]; its kept entries in stored order, columns as positions
// Is every off-diagonal entry of a (candidate) box operator the coupling to a neighbour inside the 3 x 3 x 3 cube of an Ni x Nj x Nk box, columns
// ascending?  Then the hyperplanes i + 2 j + 4 k are a valid elimination order (every lower entry lies on an earlier plane), and the set-up
// needs neither the pattern on the host nor its level sweeps: box_plane_hist_kernel / box_plane_order_kernel sort the rows by plane on the device.
__global__ __launch_bounds__(256) void box_check_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, int32_t n, int32_t Ni, int32_t Nj, int32_t* bad) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t ii = i % Ni, jj = (i / Ni) % Nj, kk = i / (Ni * Nj);
    int32_t prev = -1;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j >= n || j <= prev) { *bad = 1; return; }
        prev = j;
        const int di = j % Ni - ii, dj = (j / Ni) % Nj - jj, dk = j / (Ni * Nj) - kk;
        if (di < -1 || di > 1 || dj < -1 || dj > 1 || dk < -1 || dk > 1) { *bad = 1; return; }
    }
}
__global__ __launch_bounds__(256) void box_plane_hist_kernel(int32_t n, int32_t Ni, int32_t Nj, int32_t* hist) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&hist[i % Ni + 2 * ((i / Ni) % Nj) + 4 * (i / (Ni * Nj))], 1);
}
__global__ __launch_bounds__(256) void box_plane_order_kernel(int32_t n, int32_t Ni, int32_t Nj, int32_t* cursor, int32_t* order) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) order[atomicAdd(&cursor[i % Ni + 2 * ((i / Ni) % Nj) + 4 * (i / (Ni * Nj))], 1)] = i;
}

// Box-stencil factors straight from the factor values on A's pattern (round 4): stream a of row i = the entry whose column is the
// (dk, dj, di) neighbour of (i, j, k) in the Ni x Nj x Nk box -- BoxFactor's layout; `bad` is raised by an entry that is no such neighbour
// (it wraps around a line or plane end), a halo column, or a row whose columns do not ascend.  Zero values stay +0.0 = no entry.
__global__ __launch_bounds__(256) void gen_box_fill_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ w, const double* __restrict__ dg,
                                                           int32_t n, int32_t Ni, int32_t Nj, int32_t Nk, double* cl, double* cu, int64_t cs, double* diag, int32_t* bad,
                                                           unsigned long long* counts) {           // counts[0..12]: entries per L stream, [13..25]: per U stream
    __shared__ unsigned int cnt[26];
    if (threadIdx.x < 26) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int32_t ii = i % Ni, jj = (i / Ni) % Nj, kk = i / (Ni * Nj);
        int32_t prev = -1;
        for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
            const int32_t j = col[k];
            if (j >= n || j <= prev) { *bad = 1; break; }
            prev = j;
            if (j == i || w[k] == 0.0) continue;
            const int di = j % Ni - ii, dj = (j / Ni) % Nj - jj, dk = j / (Ni * Nj) - kk;
            if (di < -1 || di > 1 || dj < -1 || dj > 1 || dk < -1 || dk > 1) { *bad = 1; break; }
            const int code = 9 * (dk + 1) + 3 * (dj + 1) + (di + 1);
            if (j < i) { cl[(int64_t)code * cs + i] = w[k]; atomicAdd(&cnt[code], 1u); }
            else { cu[(int64_t)(code - 14) * cs + i] = w[k]; atomicAdd(&cnt[13 + code - 14], 1u); }
        }
        diag[i] = dg[i];
    }
    __syncthreads();
    if (threadIdx.x < 26 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

template <bool LOWER>
__global__ __launch_bounds__(256) void gen_fill_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ w, int32_t n,
                                                       const int32_t* __restrict__ rowid, const int32_t* __restrict__ pos, const int32_t* __restrict__ ptr,
                                                       const double* __restrict__ dg, int32_t* out_col, double* out_val, double* out_diag,
                                                       int32_t* ecol, double* eval, uint8_t* elen) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rowid[p];
    int32_t dst = ptr[p], u = 0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j >= n || w[k] == 0.0) continue;
        if (LOWER ? j < i : j > i) {
            out_col[dst] = pos[j]; out_val[dst] = w[k];
            if (ecol && u < ELLW) { ecol[(int64_t)u * n + p] = pos[j]; eval[(int64_t)u * n + p] = w[k]; }
            ++dst; ++u;
        }
    }
    out_diag[p] = LOWER ? 1.0 : dg[i];
    if (elen) elen[p] = (uint8_t)u;
}
__global__ __launch_bounds__(256) void gen_maplu_kernel(const int32_t* __restrict__ posL, const int32_t* __restrict__ posU, int32_t n, int32_t* mapLU) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) mapLU[posU[i]] = posL[i];
}

// rows ordered by (level, row); -> rowid, pos, number of levels, level offsets
static void rows_by_level(const std::vector<int32_t>& lvl, std::vector<int32_t>& rowid, std::vector<int32_t>& pos, std::vector<int32_t>& lvl_off) {
    const int64_t n = (int64_t)lvl.size();
    int32_t nlv = 0;
    for (int64_t i = 0; i < n; ++i) nlv = std::max(nlv, lvl[i] + 1);
    lvl_off.assign((size_t)nlv + 1, 0);
    for (int64_t i = 0; i < n; ++i) lvl_off[lvl[i] + 1]++;
    for (int32_t q = 0; q < nlv; ++q) lvl_off[q + 1] += lvl_off[q];
    std::vector<int32_t> cursor(lvl_off.begin(), lvl_off.end() - 1);
    rowid.resize((size_t)n); pos.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) rowid[cursor[lvl[i]]++] = (int32_t)i;        // ascending row inside a level
    for (int64_t p = 0; p < n; ++p) pos[rowid[p]] = (int32_t)p;
}

// The state of general_setup_on_device: its device temporaries (freed when it leaves), and everything one phase hands to the next --
// the box dimensions, the pattern and its levels on the host, the kept-entry counts, the rows by level, the lap timer.
namespace {
struct GenScratch {
    double *w = nullptr, *dg = nullptr; int32_t *dpos = nullptr, *done = nullptr, *order = nullptr, *nl = nullptr, *nu = nullptr;
    int32_t *posL = nullptr, *posU = nullptr; unsigned long long* flags = nullptr;     // flags: [0] first zero pivot (min), [1] stalled, [2] longest row, [3], [4] "not a box operator"
    int64_t box_ni = 0, box_nj = 0;                                         // > 0: the operator's offsets are those of a box stencil on lines of box_ni rows, box_nj lines per plane
    bool plane_order = false;                                               // ... and `order` holds its rows sorted by hyperplane: no pattern on the host
    hvec<int32_t> hrp, hcol;                                               // the pattern on the host (copied into: not value-initialised)
    std::vector<int32_t> lvl, lvlU, cntL, cntU;                            // levels of the lower / upper pattern, local entries per row
    std::vector<int32_t> hnl, hnu;                                         // kept entries per row below / above the diagonal
    std::vector<int32_t> rowid, pos;                                       // rows by level and back (reused from factor to factor)
    const bool verbose = getenv("KRYST_ILU_VERBOSE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!verbose) return;
        fprintf(stderr, "[kryst ilu]   device setup: %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        t0 = std::chrono::steady_clock::now();
    }
    ~GenScratch() { for (void* q : {(void*)w, (void*)dg, (void*)dpos, (void*)done, (void*)order, (void*)nl, (void*)nu, (void*)posL, (void*)posU, (void*)flags}) (void)pool_free(q); }
};
}  // namespace
// a phase's "not this kind of operator (or no room, or a starved poll budget): the host path takes it".  No KRYST_* code is negative; the
// phases are called by general_setup_on_device alone, which turns it into KRYST_OK with *out left null.
static const int32_t GEN_HOST_PATH = -1;
static inline unsigned gen_grid(kryst_csr_t a) { return (unsigned)((a->nrows + 255) / 256); }

// a handful of offsets: a candidate grid operator (thin boxes, 2-D operators the device-side grid setup passed on) -- the host path recognises
// those and takes the wavefront kernels; the offsets of a box stencil: S.box_ni, S.box_nj
static int32_t gen_candidate(kryst_csr_t a, GenScratch& S) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t n64 = a->nrows, nnz = a->nnz;
    if (!a->d_code) return KRYST_OK;
    int32_t used[256]; int32_t* d_used = nullptr;
    KR_HIP(pool_malloc(&d_used, sizeof used));
    (void)hipMemsetAsync(d_used, 0, sizeof used, ctx->s_main);
    hipLaunchKernelGGL(code_usage_kernel, dim3((unsigned)std::min<int64_t>(4096, (nnz + 255) / 256 + 1)), dim3(256), 0, ctx->s_main, a->d_code, nnz, d_used);
    const hipError_t e1 = hipMemcpyAsync(used, d_used, sizeof used, hipMemcpyDeviceToHost, ctx->s_main), e2 = hipStreamSynchronize(ctx->s_main);
    (void)pool_free(d_used);
    if (e1 != hipSuccess || e2 != hipSuccess) { (void)hipGetLastError(); return GEN_HOST_PATH; }
    int cnt = 0;
    for (int q = 0; q < 256; ++q) cnt += used[q] ? 1 : 0;
    // (a row block of a distributed grid operator lists up to two halo offsets besides its seven)
    if (cnt <= (a->dist ? 9 : 7) && env_int("KRYST_ILU_GRID", 1) != 0) return GEN_HOST_PATH;      // (with the grid forms switched off nothing would recognise it anyway)
    // a box stencil inside the 3 x 3 x 3 cube (up to 27 offsets that decompose for one Ni, Nj): its factors are laid out as
    // natural-order streams for the box kernels (round 4)
    if (!a->dist && cnt <= 27 && ilu_box_knob() != 0) {
        int32_t dict[256];
        if (hipMemcpyAsync(dict, a->d_dict, sizeof dict, hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess && hipStreamSynchronize(ctx->s_main) == hipSuccess) {
            std::vector<int64_t> offs;
            for (int q = 0; q < 256; ++q) if (used[q]) offs.push_back(dict[q]);
            int64_t bi = 0, bj = 0;
            std::vector<int64_t> lower, upper;
            for (int64_t o : offs) { if (o < 0) lower.push_back(o); else if (o > 0) upper.push_back(o); }
            if (lower.size() <= 13 && upper.size() <= 13 && box_dims_from_offsets(offs, n64, &bi, &bj) && n64 >= 27) { S.box_ni = bi; S.box_nj = bj; }
        } else (void)hipGetLastError();
    }
    return KRYST_OK;
}

// the device temporaries; diagonal positions and the longest row (a row must fit one wave's LDS slice)
static int32_t gen_scratch(kryst_csr_t a, GenScratch& t) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows; const int64_t nnz = a->nnz;
    const size_t nb = sizeof(int32_t) * (size_t)n;
    if (pool_malloc(&t.w, sizeof(double) * (size_t)nnz) != hipSuccess || pool_malloc(&t.dg, sizeof(double) * (size_t)n) != hipSuccess || pool_malloc(&t.dpos, nb) != hipSuccess ||
        pool_malloc(&t.done, nb) != hipSuccess || pool_malloc(&t.order, nb) != hipSuccess ||
        pool_malloc(&t.nl, nb) != hipSuccess || pool_malloc(&t.nu, nb) != hipSuccess || pool_malloc(&t.posL, nb) != hipSuccess || pool_malloc(&t.posU, nb) != hipSuccess ||
        pool_malloc(&t.flags, 64) != hipSuccess) { (void)hipGetLastError(); return GEN_HOST_PATH; }
    KR_HIP(hipMemsetAsync(t.flags, 0xff, 8, ctx->s_main));
    KR_HIP(hipMemsetAsync(t.flags + 1, 0, 56, ctx->s_main));
    KR_HIP(hipMemcpyAsync(t.w, a->d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, ctx->s_main));
    hipLaunchKernelGGL(ilu0_dpos_kernel, dim3(gen_grid(a)), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, n, t.dpos, t.done);
    hipLaunchKernelGGL(gen_rowmax_kernel, dim3(gen_grid(a)), dim3(256), 0, ctx->s_main, a->d_row_ptr, n, reinterpret_cast<int32_t*>(t.flags + 2));
    unsigned long long hf[3];
    KR_HIP(hipMemcpyAsync(hf, t.flags, sizeof hf, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return (int32_t)hf[2] > 64 ? GEN_HOST_PATH : KRYST_OK;
}

// a box operator whose every entry is a neighbour inside the cube: rows sorted by hyperplane on the device, no pattern on the host.
// Not (provably) such an operator: S.box_ni = 0, and the general phases go on.
static int32_t gen_plane_order(kryst_csr_t a, GenScratch& t) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows;
    const unsigned g = gen_grid(a);
    const int32_t Ni = (int32_t)t.box_ni, Nj = (int32_t)t.box_nj, Nk = (int32_t)(a->nrows / (t.box_ni * t.box_nj));
    const int32_t H = Ni + 2 * Nj + 4 * Nk;
    int32_t* d_hist = nullptr; int32_t bad = 1;
    int32_t* d_bad = reinterpret_cast<int32_t*>(t.flags + 4);
    std::vector<int32_t> hist((size_t)H + 1, 0);
    if (pool_malloc(&d_hist, sizeof(int32_t) * ((size_t)H + 1)) == hipSuccess && hipMemsetAsync(d_hist, 0, sizeof(int32_t) * ((size_t)H + 1), ctx->s_main) == hipSuccess) {
        hipLaunchKernelGGL(box_check_kernel, dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, n, Ni, Nj, d_bad);
        hipLaunchKernelGGL(box_plane_hist_kernel, dim3(g), dim3(256), 0, ctx->s_main, n, Ni, Nj, d_hist);
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess &&
            hipMemcpyAsync(hist.data(), d_hist, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess &&
            hipStreamSynchronize(ctx->s_main) == hipSuccess && bad == 0) {
            int32_t run = 0;
            for (int32_t h = 0; h < H; ++h) { const int32_t c = hist[(size_t)h]; hist[(size_t)h] = run; run += c; }      // exclusive scan: the planes' first positions
            if (run == n && hipMemcpyAsync(d_hist, hist.data(), sizeof(int32_t) * (size_t)H, hipMemcpyHostToDevice, ctx->s_main) == hipSuccess) {
                hipLaunchKernelGGL(box_plane_order_kernel, dim3(g), dim3(256), 0, ctx->s_main, n, Ni, Nj, d_hist, t.order);
                t.plane_order = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->s_main) == hipSuccess;
            }
        }
    }
    (void)hipGetLastError();
    (void)pool_free(d_hist);
    if (!t.plane_order) t.box_ni = 0;
    else t.lap("box operator checked, rows sorted by hyperplane");
    return KRYST_OK;
}

// the pattern on the host: levels of the lower / upper pattern, local entries per row
static int32_t gen_pattern_levels(kryst_csr_t a, GenScratch& S) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows; const int64_t nnz = a->nnz;
    hvec<int32_t>& hrp = S.hrp; hvec<int32_t>& hcol = S.hcol;
    std::vector<int32_t>& lvl = S.lvl; std::vector<int32_t>& lvlU = S.lvlU; std::vector<int32_t>& cntL = S.cntL; std::vector<int32_t>& cntU = S.cntU;
    janitor_wait();
    hrp.resize((size_t)n + 1); hcol.resize((size_t)nnz); lvl.resize((size_t)n); lvlU.resize((size_t)n); cntL.resize((size_t)n); cntU.resize((size_t)n);
    KR_HIP(hipMemcpyAsync(hrp.data(), a->d_row_ptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipMemcpyAsync(hcol.data(), a->d_col, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    {   // the two sweeps do not touch each other's arrays: side by side
        std::thread upper([&] {
            for (int32_t i = n - 1; i >= 0; --i) {
                int32_t lv = 0, c = 0;
                for (int32_t k = hrp[i]; k < hrp[i + 1]; ++k) { const int32_t j = hcol[k]; if (j > i && j < n) { lv = std::max(lv, lvlU[j] + 1); ++c; } }
                lvlU[i] = lv; cntU[i] = c;
            }
        });
        for (int32_t i = 0; i < n; ++i) {
            int32_t lv = 0, c = 0;
            for (int32_t k = hrp[i]; k < hrp[i + 1]; ++k) { const int32_t j = hcol[k]; if (j < i) { lv = std::max(lv, lvl[j] + 1); ++c; } }
            lvl[i] = lv; cntL[i] = c;
        }
        upper.join();
    }
    S.lap("pattern to the host, levels");
    return KRYST_OK;
}

// factor values (mode 2: ilu0_ikj_wave_kernel in the lower pattern's level order; modes 0 / 1: the pointwise quotients), kept entries per
// row and the divisors; a zero pivot is the set-up's error
static int32_t gen_values(kryst_csr_t a, int mode, GenScratch& t) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows;
    const unsigned g = gen_grid(a);
    const size_t nb = sizeof(int32_t) * (size_t)n;
    if (mode == KRYST_ILU_TRUE_ILU0) {
        if (!t.plane_order) {
            std::vector<int32_t> lvl_off;
            rows_by_level(t.lvl, t.rowid, t.pos, lvl_off);
            KR_HIP(hipMemcpyAsync(t.order, t.rowid.data(), nb, hipMemcpyHostToDevice, ctx->s_main));
        }
        hipLaunchKernelGGL(ilu0_ikj_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, t.dpos, t.order, n, t.done,
                           t.flags, reinterpret_cast<int32_t*>(t.flags + 1), std::max(1, env_int("KRYST_ILU_SETUP_POLL_BUDGET", 1 << 22)), a->dist ? 0 : 1);
    } else {
        hipLaunchKernelGGL(gen_pointwise_kernel, dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, t.dpos, n, mode, t.w, t.flags);
    }
    KR_HIP(hipGetLastError());
    const int divide = mode != KRYST_ILU_KRYST_COMPAT ? 1 : 0;              // ilu.rs:115-119 never divides
    hipLaunchKernelGGL(gen_classify_kernel, dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, n, divide, t.nl, t.nu, t.dg);
    KR_HIP(hipGetLastError());
    t.hnl.resize((size_t)n); t.hnu.resize((size_t)n);
    unsigned long long hf[3];
    KR_HIP(hipMemcpyAsync(t.hnl.data(), t.nl, nb, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipMemcpyAsync(t.hnu.data(), t.nu, nb, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipMemcpyAsync(hf, t.flags, sizeof hf, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    if ((int32_t)hf[1] != 0) return GEN_HOST_PATH;                          // a starved poll budget
    if (hf[0] != ~0ull) {
        if (mode == KRYST_ILU_TRUE_ILU0) { const long long c = (long long)(hf[0] & 0xffffffffull); set_error("ILU(0): zero pivot at row %lld", c); set_error_row(c); return KRYST_ZERO_PIVOT; }
        set_error("ILUP: zero diagonal in U at row %lld", (long long)(hf[0] & 0xffffffffull));
        return KRYST_SOLVE_ERROR;
    }
    t.lap("factor values, kept entries");
    return KRYST_OK;
}

// box stencil: 13 natural-order coefficient streams per factor, written by one kernel (no level machinery at all).  Not a box operator
// after all: the level-ordered forms -- when the pattern is on the host to level-order from
static int32_t gen_box_streams(kryst_csr_t a, GenScratch& t, IluPc* D) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows;
    const size_t cb = sizeof(double) * (size_t)13 * (size_t)box_stream_stride(n);
    int32_t* d_bad = reinterpret_cast<int32_t*>(t.flags + 3);
    unsigned long long* d_counts = nullptr; unsigned long long counts[26];
    int32_t bad = 1;
    if (pool_malloc(&D->BL.d_c, cb) != hipSuccess || pool_malloc(&D->BU.d_c, cb) != hipSuccess || pool_malloc(&D->BU.d_diag, sizeof(double) * (size_t)n) != hipSuccess) {
        (void)hipGetLastError();
    } else if (pool_malloc(&d_counts, sizeof counts) == hipSuccess && hipMemsetAsync(d_counts, 0, sizeof counts, ctx->s_main) == hipSuccess &&
               hipMemsetAsync(D->BL.d_c, 0, cb, ctx->s_main) == hipSuccess && hipMemsetAsync(D->BU.d_c, 0, cb, ctx->s_main) == hipSuccess) {
        const int32_t Ni = (int32_t)t.box_ni, Nj = (int32_t)t.box_nj, Nk = (int32_t)(a->nrows / (t.box_ni * t.box_nj));
        hipLaunchKernelGGL(gen_box_fill_kernel, dim3(gen_grid(a)), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, t.dg, n, Ni, Nj, Nk, D->BL.d_c, D->BU.d_c, box_stream_stride(n), D->BU.d_diag, d_bad,
                           d_counts);
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess &&
            hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess &&
            hipStreamSynchronize(ctx->s_main) == hipSuccess && bad == 0) {
            for (BoxFactor* F : {&D->BL, &D->BU}) { F->Ni = Ni; F->Nj = Nj; F->Nk = Nk; F->ok = true; }
            box_classify(counts, true, Ni, Nj, Nk, &D->BL); box_classify(counts + 13, false, Ni, Nj, Nk, &D->BU);
        }
    }
    (void)pool_free(d_counts);
    (void)hipGetLastError();
    if (D->box()) { t.lap("box-stencil streams"); return KRYST_OK; }
    D->BL.free_all(); D->BU.free_all(); D->BL = BoxFactor(); D->BU = BoxFactor();
    return t.plane_order ? GEN_HOST_PATH : KRYST_OK;
}

// the two level-ordered factors, written in level order straight from (A's pattern, w); a factor that drops entries does not have the
// pattern's levels: host path
static int32_t gen_level_factors(kryst_csr_t a, GenScratch& t, IluPc* D) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t n = (int32_t)a->nrows;
    const unsigned g = gen_grid(a);
    const size_t nb = sizeof(int32_t) * (size_t)n;
    if (t.hnl != t.cntL || t.hnu != t.cntU) return GEN_HOST_PATH;
    std::vector<int32_t> ptr((size_t)n + 1);
    std::vector<int32_t>& rowid = t.rowid; std::vector<int32_t>& pos = t.pos;
    int32_t rc = KRYST_OK;
    for (int which = 0; which < 2 && rc == KRYST_OK; ++which) {
        TriFactor* F = which == 0 ? &D->L : &D->U;
        const std::vector<int32_t>& lv = which == 0 ? t.lvl : t.lvlU;
        const std::vector<int32_t>& len = which == 0 ? t.hnl : t.hnu;
        rows_by_level(lv, rowid, pos, F->lvl_off);
        int32_t maxlen = 0;
        ptr[0] = 0;
        int64_t nlong = 0;
        for (int32_t p = 0; p < n; ++p) { const int32_t L = len[rowid[p]]; ptr[(size_t)p + 1] = ptr[p] + L; maxlen = std::max(maxlen, L); nlong += L > 8; }
        const size_t fn = (size_t)ptr[n];
        F->npos = n;
        choose_level_form(F, n, (int64_t)F->lvl_off.size() - 1, maxlen, nlong, (int64_t)fn);
        int32_t* d_pos = which == 0 ? t.posL : t.posU;
        rc = up(&F->d_row, rowid);
        if (rc == KRYST_OK) rc = up(&F->d_ptr, ptr);
        if (rc == KRYST_OK) rc = up(&F->d_lvl_off, F->lvl_off);
        if (rc == KRYST_OK && (pool_malloc(&F->d_col, sizeof(int32_t) * (fn + 1)) != hipSuccess || pool_malloc(&F->d_val, sizeof(double) * (fn + 1)) != hipSuccess ||
                               pool_malloc(&F->d_diag, sizeof(double) * ((size_t)n + 1)) != hipSuccess)) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
        if (rc == KRYST_OK && F->ell) {
            const size_t eb = (size_t)ELLW * n;
            if (pool_malloc(&F->d_ecol, sizeof(int32_t) * (eb + 1)) != hipSuccess || pool_malloc(&F->d_eval, sizeof(double) * (eb + 1)) != hipSuccess ||
                pool_malloc(&F->d_elen, (size_t)n + 1) != hipSuccess) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
            else if (hipMemsetAsync(F->d_ecol, 0, sizeof(int32_t) * (eb + 1), ctx->s_main) != hipSuccess ||
                     hipMemsetAsync(F->d_eval, 0, sizeof(double) * (eb + 1), ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;      // padding slots: column 0, value 0
        }
        if (rc == KRYST_OK && hipMemcpyAsync(d_pos, pos.data(), nb, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
        if (rc == KRYST_OK) {
            if (which == 0) hipLaunchKernelGGL((gen_fill_kernel<true>), dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, n, F->d_row, d_pos, F->d_ptr, t.dg,
                                               F->d_col, F->d_val, F->d_diag, F->ell ? F->d_ecol : nullptr, F->d_eval, F->ell ? F->d_elen : nullptr);
            else hipLaunchKernelGGL((gen_fill_kernel<false>), dim3(g), dim3(256), 0, ctx->s_main, a->d_row_ptr, a->d_col, t.w, n, F->d_row, d_pos, F->d_ptr, t.dg,
                                    F->d_col, F->d_val, F->d_diag, F->ell ? F->d_ecol : nullptr, F->d_eval, F->ell ? F->d_elen : nullptr);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("factor fill kernel failed"); rc = KRYST_ERR_HIP; }   // (pos lives in a host vector reused below)
            if (rc == KRYST_OK) rc = build_free_streams(F, ctx->s_main, ptr.data());
        }
    }
    if (rc == KRYST_OK && pool_malloc(&D->d_mapLU, nb + 4) != hipSuccess) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
    if (rc == KRYST_OK) {
        hipLaunchKernelGGL(gen_maplu_kernel, dim3(g), dim3(256), 0, ctx->s_main, t.posL, t.posU, n, D->d_mapLU);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
    }
    t.lap("level-ordered factors");
    return rc;
}

int32_t kr::general_setup_on_device(kryst_csr_t a, int mode, kryst_pc_t* out) {
    *out = nullptr;
    if (a->nrows == 0 || a->nnz == 0 || a->nrows >= (1ll << 31) - 4 || env_int("KRYST_ILU_DEVICE_SETUP", 1) == 0) return KRYST_OK;
    tl_setup_stream = a->ctx->s_main;
    GenScratch S;
    IluPc* pc = nullptr;
    int32_t rc = gen_candidate(a, S);
    if (rc == KRYST_OK) rc = gen_scratch(a, S);
    if (rc == KRYST_OK && S.box_ni > 0) rc = gen_plane_order(a, S);
    if (rc == KRYST_OK && !S.plane_order) rc = gen_pattern_levels(a, S);
    if (rc == KRYST_OK) rc = gen_values(a, mode, S);
    if (rc == KRYST_OK) pc = new IluPc(a);
    if (rc == KRYST_OK && S.box_ni > 0) rc = gen_box_streams(a, S, pc);
    if (rc == KRYST_OK && !pc->box()) rc = gen_level_factors(a, S, pc);
    if (rc == KRYST_OK) rc = finish_ilu_device(pc);
    if (rc != KRYST_OK) {
        if (pc) kryst_pc_destroy(pc);
        return rc == GEN_HOST_PATH ? KRYST_OK : rc;                         // the host path takes over with *out left null
    }
    *out = pc;
    return KRYST_OK;
}
