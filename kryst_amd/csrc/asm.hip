// Additive Schwarz (AdditiveSchwarz, src/preconditioner/asm.rs) on the device, with the direct solve as the inner solver (DESIGN.md
// section 4.10).  As written (asm.rs:76-119): z = 0, then for every subdomain in ascending order z[g[i]] = z[g[i]] + (B^-1 r|_g)[i]; the
// `overlap` field is stored and never used.  Labelled deviations, shared with block Jacobi (block_jacobi.hip): each subdomain matrix is
// inverted explicitly (Gauss-Jordan with full pivoting, the textbook `gaussj` order), each index set is sorted ascending first, and a
// singular or non-finite subdomain, a bad index or a non-square operator is an error.  Labelled extensions: KRYST_ASM_GROWN grows every
// subdomain by `overlap` layers of the symmetrised graph of A; KRYST_ASM_RESTRICTED (RAS) grows them too and keeps, for every row, only the
// product of the last un-grown set that contains it.
//
// Set-up: index sets sorted and checked on the host; growth by one workgroup per subdomain (candidates merged in LDS, bitonic sort,
// duplicates removed); tiles by one workgroup per subdomain, one row per lane (one wave up to 64 rows, two waves up to 128), the tile in LDS.
// Apply: a products kernel X[off_k + i] = sum_j Binv_k[i][j] r[g_k[j]] (one position per lane, r|_g staged in LDS, tiles column-major) and a
// combine kernel z[row] = ((+0.0 + X[p1]) + X[p2]) + ... over a row -> positions map built at set-up.
#include "asm.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace kr {

constexpr int KR_ASM_MAX = KRYST_ASM_MAX_ROWS;   // rows per subdomain: one lane each, two waves
constexpr int KR_ASM_T = 256;                    // products / combine / growth workgroups
constexpr int KR_ASM_SORT = 2048;                // growth: entries merged per round (the current set + candidates)
constexpr int64_t KR_ASM_GRID_CAP = 1 << 20;
constexpr unsigned long long KR_ASM_NOERR = ~0ull;

__host__ __device__ inline int asm_stride(int b) { return b + ((b & 1) ? 0 : 1); }   // odd LDS row stride

static unsigned asm_grid(int64_t items, int per_wg) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_wg - 1) / per_wg, KR_ASM_GRID_CAP));
}

// ---------------------------------------------------------------- growth: one workgroup per subdomain
// U (the current set, sorted, at most 128 rows) is merged with the neighbours of the rows of the layer's starting set S: the stored columns
// of row i of A and of A^T.  Candidates go in rounds of up to KR_ASM_SORT - |U| entries together with U through a bitonic sort in LDS; the
// distinct values become the new U.  More than 128 distinct rows: sizes[k] = -1 and err = min(err, k).
__global__ __launch_bounds__(KR_ASM_T) void asm_grow_kernel(const int32_t* a_ptr, const int32_t* a_col, const int32_t* t_ptr, const int32_t* t_col,
                                                           const int64_t* ptr, const int32_t* idx, int64_t nsub, int overlap, int32_t* out,
                                                           int32_t* sizes, unsigned long long* err) {
    __shared__ int32_t U[KR_ASM_MAX], S[KR_ASM_MAX], cum[KR_ASM_MAX + 1], B[KR_ASM_SORT], part[KR_ASM_T];
    constexpr int PER = KR_ASM_SORT / KR_ASM_T;
    const int t = threadIdx.x;
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {                // uniform over the workgroup
        const int64_t lo = ptr[k];
        int nu = (int)(ptr[k + 1] - lo);
        for (int i = t; i < nu; i += KR_ASM_T) U[i] = idx[lo + i];
        __syncthreads();
        bool fail = false;
        for (int layer = 0; layer < overlap && !fail; ++layer) {
            const int ns = nu;
            for (int i = t; i < ns; i += KR_ASM_T) S[i] = U[i];
            __syncthreads();
            if (t == 0) {                                                   // candidate offsets per row of S
                int c = 0;
                for (int i = 0; i < ns; ++i) {
                    cum[i] = c;
                    const int r = S[i];
                    c += (a_ptr[r + 1] - a_ptr[r]) + (t_ptr[r + 1] - t_ptr[r]);
                }
                cum[ns] = c;
            }
            __syncthreads();
            const int total = cum[ns];
            for (int t0 = 0; t0 < total && !fail;) {
                const int m = min(total - t0, KR_ASM_SORT - nu);
                for (int q = t; q < KR_ASM_SORT; q += KR_ASM_T) {
                    int v = INT_MAX;
                    if (q < nu) v = U[q];
                    else if (q - nu < m) {
                        const int c = t0 + q - nu;
                        int l = 0, h = ns;                                  // the last i with cum[i] <= c
                        while (h - l > 1) { const int mid = (l + h) >> 1; if (cum[mid] <= c) l = mid; else h = mid; }
                        const int r = S[l], e = c - cum[l], da = a_ptr[r + 1] - a_ptr[r];
                        v = e < da ? a_col[a_ptr[r] + e] : t_col[t_ptr[r] + e - da];
                    }
                    B[q] = v;
                }
                __syncthreads();
                for (int kk = 2; kk <= KR_ASM_SORT; kk <<= 1)
                    for (int j = kk >> 1; j > 0; j >>= 1) {
                        for (int q = t; q < KR_ASM_SORT; q += KR_ASM_T) {
                            const int x = q ^ j;
                            if (x > q) {
                                const int va = B[q], vb = B[x];
                                if ((va > vb) == ((q & kk) == 0)) { B[q] = vb; B[x] = va; }
                            }
                        }
                        __syncthreads();
                    }
                // keep the first of every run of equal values; thread t owns slots [PER t, PER t + PER)
                int cnt = 0;
                for (int q = t * PER; q < t * PER + PER; ++q) cnt += (B[q] != INT_MAX && (q == 0 || B[q] != B[q - 1])) ? 1 : 0;
                part[t] = cnt;
                __syncthreads();
                for (int o = 1; o < KR_ASM_T; o <<= 1) {
                    const int x = (t >= o) ? part[t - o] : 0;
                    __syncthreads();
                    part[t] += x;
                    __syncthreads();
                }
                const int nnew = part[KR_ASM_T - 1];
                if (nnew > KR_ASM_MAX) {
                    fail = true;
                } else {
                    int w = part[t] - cnt;
                    for (int q = t * PER; q < t * PER + PER; ++q)
                        if (B[q] != INT_MAX && (q == 0 || B[q] != B[q - 1])) U[w++] = B[q];
                    nu = nnew;
                }
                t0 += m;
                __syncthreads();
            }
        }
        if (fail) {
            if (t == 0) { sizes[k] = -1; atomicMin(err, (unsigned long long)k); }
        } else {
            for (int i = t; i < nu; i += KR_ASM_T) out[k * KR_ASM_MAX + i] = U[i];
            if (t == 0) sizes[k] = nu;
        }
        __syncthreads();                                                    // the next subdomain reuses the LDS
    }
}

// ---------------------------------------------------------------- tiles: one workgroup per subdomain of `list`, one row per lane
// Gauss-Jordan with full pivoting in the order of bjacobi_ref.gauss_jordan / block_jacobi.hip: the pivot is the largest |B[p][q]| over the rows
// and columns not pivoted, the smaller row on a tie (within a row the first column: a later one wins only if strictly larger).  With two
// waves the per-wave winners meet in LDS and wave 0 (the smaller rows) keeps a tie.  err: min over the failing subdomains of
// (k << 9 | code << 7 | position); code 0: non-finite entry, 1: zero pivot (position = the smallest position not yet pivoted).
template <int NT>
__global__ __launch_bounds__(NT) void asm_tiles_kernel(const int32_t* row_ptr, const int32_t* col, const double* val, const int32_t* list,
                                                       int64_t nlist, const int32_t* xoff, const int64_t* toff, const int32_t* idx, double* tiles,
                                                       unsigned long long* err) {
    extern __shared__ double asm_lds[];
    __shared__ double wbest[NT / 64];
    __shared__ int wbi[NT / 64], wbj[NT / 64], step_r[KR_ASM_MAX], step_c[KR_ASM_MAX];
    const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
    double* T = asm_lds;
    for (int64_t w = blockIdx.x; w < nlist; w += gridDim.x) {                // uniform over the workgroup
        const int k = list[w];
        const int lo = xoff[k], bk = xoff[k + 1] - lo, bs = asm_stride(bk);
        const bool act = i < bk;
        if (act) {                                                          // B[i][j] = A(g[i], g[j]) when stored, else +0.0
            for (int l = 0; l < bk; ++l) T[i * bs + l] = 0.0;
            const int gi = idx[lo + i];
            bool bad = false;
            for (int32_t e = row_ptr[gi]; e < row_ptr[gi + 1]; ++e) {
                const int c = col[e];
                int l0 = 0, h = bk;
                while (l0 < h) { const int mid = (l0 + h) >> 1; if (idx[lo + mid] < c) l0 = mid + 1; else h = mid; }
                if (l0 < bk && idx[lo + l0] == c) { const double v = val[e]; T[i * bs + l0] = v; bad |= !isfinite(v); }
            }
            if (bad) atomicMin(err, (unsigned long long)k << 9);
        }
        __syncthreads();
        unsigned long long piv0 = 0ull, piv1 = 0ull;                        // columns pivoted (0..63, 64..127), the same in every lane
        bool dead = false;
        for (int s = 0; s < bk; ++s) {
            double best = -1.0; int bj = 0;
            const bool mine = i < 64 ? ((piv0 >> i) & 1ull) != 0 : ((piv1 >> (i - 64)) & 1ull) != 0;
            if (act && !mine) {
                for (int l = 0; l < bk; ++l) {
                    const bool pl = l < 64 ? ((piv0 >> l) & 1ull) != 0 : ((piv1 >> (l - 64)) & 1ull) != 0;
                    if (pl) continue;
                    const double a = fabs(T[i * bs + l]);
                    if (a > best) { best = a; bj = l; }
                }
            }
            int bi = i;
            for (int off = 1; off < 64; off <<= 1) {
                const double ob = __shfl(best, lane + off, 64);
                const int oi = __shfl(bi, lane + off, 64), oj = __shfl(bj, lane + off, 64);
                if (lane + off < 64 && (ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; bj = oj; }
            }
            if (NT > 64) {
                if (lane == 0) { wbest[wave] = best; wbi[wave] = bi; wbj[wave] = bj; }
                __syncthreads();
                int win = 0;
                for (int v = 1; v < NT / 64; ++v) if (wbest[v] > wbest[win]) win = v;
                best = wbest[win]; bi = wbi[win]; bj = wbj[win];
            } else {
                best = __shfl(best, 0, 64); bi = __shfl(bi, 0, 64); bj = __shfl(bj, 0, 64);
            }
            if (best == 0.0) {                                              // uniform: the chosen pivot is 0
                dead = true;
                if (i == 0) {
                    int pos = 0;
                    while (pos < bk && (pos < 64 ? ((piv0 >> pos) & 1ull) != 0 : ((piv1 >> (pos - 64)) & 1ull) != 0)) ++pos;
                    atomicMin(err, ((unsigned long long)k << 9) | (1ull << 7) | (unsigned long long)pos);
                }
                break;
            }
            const int p = bi, q = bj;
            const double piv = T[p * bs + q];
            __syncthreads();
            if (act && p != q) {                                            // swap rows p and q (lane i: column i)
                const double tt = T[p * bs + i]; T[p * bs + i] = T[q * bs + i]; T[q * bs + i] = tt;
            }
            if (i == 0) { step_r[s] = p; step_c[s] = q; }
            if (q < 64) piv0 |= 1ull << q; else piv1 |= 1ull << (q - 64);
            __syncthreads();
            if (act) {                                                      // pivinv = 1/B[q][q]; B[q][q] = 1; B[q][l] *= pivinv
                const double pivinv = 1.0 / piv;
                const double v = (i == q) ? 1.0 : T[q * bs + i];
                T[q * bs + i] = v * pivinv;
            }
            __syncthreads();
            if (act && i != q) {                                            // row m = i: f = B[m][q]; B[m][q] = 0; B[m][l] -= B[q][l] * f
                double* Tm = T + i * bs;
                const double* Tq = T + q * bs;
                const double f = Tm[q];
                Tm[q] = 0.0;
                for (int l = 0; l < bk; ++l) Tm[l] = Tm[l] - Tq[l] * f;
            }
            __syncthreads();
        }
        if (!dead) {
            for (int s = bk - 1; s >= 0; --s) {                             // undo the column permutation, last step first (lane i: its row)
                const int rs = step_r[s], cs = step_c[s];
                if (act && rs != cs) { double* Tm = T + i * bs; const double tt = Tm[rs]; Tm[rs] = Tm[cs]; Tm[cs] = tt; }
            }
            if (act)
                for (int j = 0; j < bk; ++j) tiles[toff[k] + (int64_t)j * bk + i] = T[i * bs + j];
        }
        __syncthreads();                                                    // the next subdomain reuses the LDS
    }
}

// ---------------------------------------------------------------- apply
// X[p] for p = off_k + i: sum_j Binv_k[i][j] * r[g_k[j]], ascending j from +0.0, no FMA.  A workgroup takes 256 consecutive positions; the
// subdomains they touch span at most 127 + 256 + 127 positions, whose r[g] are staged in LDS first.
__global__ __launch_bounds__(KR_ASM_T) void asm_products_kernel(const double* tiles, const int64_t* toff, const int32_t* xoff, const int32_t* posk,
                                                               const int32_t* idx, int64_t total, const double* r, double* X, const int* done) {
    if (done && *done) return;
    __shared__ double rb[KR_ASM_T + 2 * KR_ASM_MAX];
    for (int64_t p0 = (int64_t)blockIdx.x * KR_ASM_T; p0 < total; p0 += (int64_t)gridDim.x * KR_ASM_T) {   // uniform over the workgroup
        const int64_t plast = p0 + KR_ASM_T - 1 < total ? p0 + KR_ASM_T - 1 : total - 1;
        const int32_t qlo = xoff[posk[p0]], qhi = xoff[posk[plast] + 1];
        for (int32_t q = qlo + (int32_t)threadIdx.x; q < qhi; q += KR_ASM_T) rb[q - qlo] = r[idx[q]];
        __syncthreads();
        const int64_t p = p0 + threadIdx.x;
        if (p < total) {
            const int k = posk[p];
            const int32_t lo = xoff[k];
            const int b = xoff[k + 1] - lo, i = (int)(p - lo);
            const double* t = tiles + toff[k] + i;
            const double* rr = rb + (lo - qlo);
            double s = 0.0;
            for (int j = 0; j < b; ++j) s = s + t[(int64_t)j * b] * rr[j];
            X[p] = s;
        }
        __syncthreads();
    }
}

// z[row] = ((+0.0 + X[p1]) + X[p2]) + ... over mpos[mptr[row] .. mptr[row + 1]) (ascending subdomain order; RAS: the owner's one position)
__global__ __launch_bounds__(KR_ASM_T) void asm_combine_kernel(const int32_t* mptr, const int32_t* mpos, const double* X, int64_t n, double* z,
                                                              const int* done) {
    if (done && *done) return;
    for (int64_t row = (int64_t)blockIdx.x * KR_ASM_T + threadIdx.x; row < n; row += (int64_t)gridDim.x * KR_ASM_T) {
        double s = 0.0;
        for (int32_t e = mptr[row]; e < mptr[row + 1]; ++e) s = s + X[mpos[e]];
        z[row] = s;
    }
}

// the (grown) subdomains sorted ascending, their tiles block after block (column-major inside a tile), the products X of an apply (one
// entry per subdomain row) and the row -> positions-in-X map of the combine
struct AsmPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_ASM;
    int64_t nsub = 0, total = 0;      // subdomains; sum of their rows
    int32_t maxb = 0;
    double* d_tile = nullptr; int64_t* d_toff = nullptr; double* d_x = nullptr;
    int32_t* d_xoff = nullptr;        // subdomain k's rows: positions [xoff[k], xoff[k + 1]) of d_idx / X
    int32_t* d_posk = nullptr;        // the subdomain of every position
    int32_t* d_idx = nullptr;
    int32_t* d_mptr = nullptr; int32_t* d_mpos = nullptr;
    std::vector<int64_t> ptr_h; std::vector<int32_t> idx_h, owner_h;   // owner: the last un-grown set containing a row, or -1
    AsmPc(kryst_csr_t a_, int64_t nsub_, int64_t total_, int32_t maxb_) : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), nsub(nsub_), total(total_), maxb(maxb_) {}
    ~AsmPc() override { for (void* p : {(void*)d_tile, (void*)d_toff, (void*)d_xoff, (void*)d_posk, (void*)d_idx, (void*)d_x, (void*)d_mptr, (void*)d_mpos}) (void)pool_free(p); }
    int32_t apply(int64_t nv, const double* r, double* z, const int* done) override;
};

int32_t AsmPc::apply(int64_t, const double* r, double* z, const int* done) {
    if (total > 0) {
        hipLaunchKernelGGL(asm_products_kernel, dim3(asm_grid(total, KR_ASM_T)), dim3(KR_ASM_T), 0, ctx->s_main, (const double*)d_tile,
                           (const int64_t*)d_toff, (const int32_t*)d_xoff, (const int32_t*)d_posk,
                           (const int32_t*)d_idx, total, r, d_x, done);
        KR_HIP(hipGetLastError());
    }
    return asm_combine_launch(ctx, d_mptr, d_mpos, d_x, n, z, done);
}

int32_t asm_combine_launch(kryst_ctx_t ctx, const int32_t* mptr, const int32_t* mpos, const double* X, int64_t n, double* z, const int* done) {
    if (n > 0) {
        hipLaunchKernelGGL(asm_combine_kernel, dim3(asm_grid(n, KR_ASM_T)), dim3(KR_ASM_T), 0, ctx->s_main, mptr, mpos, X, n, z, done);
        KR_HIP(hipGetLastError());
    }
    return KRYST_OK;
}

// Is `need` bytes of device memory available?  hipMemGetInfo counts the blocks kept by the device pool (pool_free: a destroyed ILU's factors,
// an earlier preconditioner's tiles, the growth's own scratch) as used, so when the figure falls short the pool is given back to the driver
// and the figure taken again.  Test hook: KRYST_ASM_MEM_LIMIT_MB caps the free figure at that many MiB less what the pool holds, as if
// the device had that much free with the pool empty.
int32_t asm_check_memory(int device, unsigned long long need) {
    unsigned long long avail = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        size_t fr = 0, tot = 0;
        KR_HIP(hipMemGetInfo(&fr, &tot));
        avail = fr;
        if (const char* e = getenv("KRYST_ASM_MEM_LIMIT_MB")) {
            const long long mb = atoll(e);
            const unsigned long long cap = mb > 0 ? (unsigned long long)mb << 20 : 0ull, pooled = pool_pooled(device);
            if (mb >= 0) avail = std::min<unsigned long long>(avail, cap > pooled ? cap - pooled : 0ull);
        }
        if (need <= avail) return KRYST_OK;
        if (attempt == 0 && pool_trim(device) == 0) break;          // nothing pooled: the figure stands
    }
    set_error("additive Schwarz: the set-up needs %llu bytes of device memory, %llu are available", need, avail);
    return KRYST_ERR_HIP;
}

// the bytes the preconditioner keeps on the device for subdomain sizes with sum b = sb, sum b^2 = sb2, and m map entries
static unsigned long long asm_bytes(int64_t n, int64_t nsub, unsigned long long sb, unsigned long long sb2, unsigned long long m) {
    return 8ull * sb2 + (4ull + 4ull + 8ull) * sb + 12ull * (unsigned long long)(nsub + 1) + 4ull * (unsigned long long)(n + 1) + 4ull * m;
}

// ---------------------------------------------------------------- growth of sets past 128 rows: a bitmap over the rows per workgroup
// Workgroup w owns bm[w W .. (w + 1) W) (W = ceil(n / 32) words, all zero between subdomains) and cur[w cap .. (w + 1) cap).  Per layer the
// neighbours of the rows of cur are marked; the marked rows of the words [wlo, whi] (the span of everything marked so far), taken in
// ascending order, are the new cur.  More than cap rows: sizes[k] = -1 and err = min(err, k).  out == nullptr: sizes only (the first of
// two passes; the host turns the sizes into the offsets ooff of the second).  The bitmap is read and cleared with device-scope atomics:
// the marks are atomics, which a cached load need not see.
__global__ __launch_bounds__(KR_ASM_T) void asm_grow_wide_kernel(const int32_t* a_ptr, const int32_t* a_col, const int32_t* t_ptr, const int32_t* t_col,
                                                                const int64_t* ptr, const int32_t* idx, int64_t nsub, int overlap, int cap, int64_t W,
                                                                unsigned int* bm_all, int32_t* cur_all, const int64_t* ooff, int32_t* out,
                                                                int32_t* sizes, unsigned long long* err) {
    __shared__ int part[KR_ASM_T];
    __shared__ int s_lo, s_hi;
    const int t = threadIdx.x;
    unsigned int* bm = bm_all + (int64_t)blockIdx.x * W;
    int32_t* cur = cur_all + (int64_t)blockIdx.x * cap;
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {                // uniform over the workgroup
        const int64_t lo = ptr[k];
        int nu = (int)(ptr[k + 1] - lo);
        bool fail = false;
        if (nu > 0) {
            if (t == 0) { s_lo = idx[lo] >> 5; s_hi = idx[lo + nu - 1] >> 5; }
            for (int i = t; i < nu; i += KR_ASM_T) { const int r = idx[lo + i]; cur[i] = r; atomicOr(&bm[r >> 5], 1u << (r & 31)); }
            __syncthreads();
            for (int layer = 0; layer < overlap && !fail; ++layer) {
                int mylo = INT_MAX, myhi = -1;
                for (int i = t; i < nu; i += KR_ASM_T) {
                    const int r = cur[i];
                    for (int32_t e = a_ptr[r]; e < a_ptr[r + 1]; ++e) { const int c = a_col[e]; atomicOr(&bm[c >> 5], 1u << (c & 31)); mylo = min(mylo, c >> 5); myhi = max(myhi, c >> 5); }
                    for (int32_t e = t_ptr[r]; e < t_ptr[r + 1]; ++e) { const int c = t_col[e]; atomicOr(&bm[c >> 5], 1u << (c & 31)); mylo = min(mylo, c >> 5); myhi = max(myhi, c >> 5); }
                }
                if (myhi >= 0) { atomicMin(&s_lo, mylo); atomicMax(&s_hi, myhi); }
                __syncthreads();
                const int wlo = s_lo, whi = s_hi;
                int base = 0;
                for (int w0 = wlo; w0 <= whi; w0 += KR_ASM_T) {             // uniform
                    const int w = w0 + t;
                    const unsigned int bits = w <= whi ? __hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                    const int cnt = __popc(bits);
                    part[t] = cnt;
                    __syncthreads();
                    for (int o = 1; o < KR_ASM_T; o <<= 1) {
                        const int x = (t >= o) ? part[t - o] : 0;
                        __syncthreads();
                        part[t] += x;
                        __syncthreads();
                    }
                    int q = base + part[t] - cnt;
                    unsigned int rest = bits;
                    while (rest) {
                        const int bit = __ffs(rest) - 1;
                        rest &= rest - 1;
                        if (q < cap) cur[q] = (w << 5) | bit;
                        ++q;
                    }
                    base += part[KR_ASM_T - 1];
                    __syncthreads();
                }
                if (base > cap) fail = true; else nu = base;
            }
            const int wlo = s_lo, whi = s_hi;
            __syncthreads();
            for (int w = wlo + t; w <= whi; w += KR_ASM_T) __hip_atomic_store(&bm[w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (fail) {
            if (t == 0) { sizes[k] = -1; atomicMin(err, (unsigned long long)k); }
        } else {
            if (out) for (int i = t; i < nu; i += KR_ASM_T) out[ooff[k] + i] = cur[i];
            if (t == 0) sizes[k] = nu;
        }
        __syncthreads();                                                    // the next subdomain reuses cur, the bitmap and the LDS
    }
}

static int32_t asm_grow_wide(kryst_csr_t a, int overlap, std::vector<int64_t>& ptr, std::vector<int32_t>& idx, int cap) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nsub = (int64_t)ptr.size() - 1, n = a->nrows, W = (n + 31) / 32;
    const unsigned grid = (unsigned)std::min<int64_t>(nsub, 128);
    DevCsr at;
    int64_t* d_ptr = nullptr; int32_t* d_idx = nullptr; int32_t* d_out = nullptr; int32_t* d_sizes = nullptr; unsigned long long* d_err = nullptr;
    unsigned int* d_bm = nullptr; int32_t* d_cur = nullptr; int64_t* d_ooff = nullptr;
    std::vector<int32_t> sizes((size_t)nsub);
    std::vector<int64_t> ooff((size_t)nsub + 1, 0);
    int32_t rc = csr_transpose(ctx, "additive Schwarz", a->d_row_ptr, a->d_col, a->d_val, a->nrows, a->ncols, false, 0.0, at);
    do {
        if (rc != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &d_ptr, ptr, "index sets")) != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &d_idx, idx, "index sets")) != KRYST_OK) break;
        if (pool_malloc(&d_bm, sizeof(unsigned int) * (size_t)grid * (size_t)std::max<int64_t>(W, 1)) != hipSuccess ||
            pool_malloc(&d_cur, sizeof(int32_t) * (size_t)grid * (size_t)cap) != hipSuccess ||
            pool_malloc(&d_sizes, sizeof(int32_t) * (size_t)nsub) != hipSuccess || pool_malloc(&d_err, sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("additive Schwarz: out of device memory (growth of %lld subdomains)", (long long)nsub); rc = KRYST_ERR_HIP; break;
        }
        if (hipMemsetAsync(d_bm, 0, sizeof(unsigned int) * (size_t)grid * (size_t)std::max<int64_t>(W, 1), ctx->s_main) != hipSuccess ||
            hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), ctx->s_main) != hipSuccess) { rc = KRYST_ERR_HIP; break; }
        for (int pass = 0; pass < 2 && rc == KRYST_OK; ++pass) {
            if (pass == 1) {
                for (int64_t k = 0; k < nsub; ++k) ooff[(size_t)k + 1] = ooff[(size_t)k] + sizes[(size_t)k];
                if (ooff.back() >= INT32_MAX) { set_error("bad argument: pc_asm: more than 2^31 - 1 subdomain rows after growth"); rc = KRYST_ERR_ARG; break; }
                if ((rc = asm_upload(ctx, &d_ooff, ooff, "grown index sets")) != KRYST_OK) break;
                if (pool_malloc(&d_out, sizeof(int32_t) * (size_t)std::max<int64_t>(ooff.back(), 1)) != hipSuccess) {
                    (void)hipGetLastError(); d_out = nullptr;
                    set_error("additive Schwarz: out of device memory (%lld grown subdomain rows)", (long long)ooff.back()); rc = KRYST_ERR_HIP; break;
                }
            }
            hipLaunchKernelGGL(asm_grow_wide_kernel, dim3(grid), dim3(KR_ASM_T), 0, ctx->s_main, a->d_row_ptr, a->d_col, (const int32_t*)at.ptr,
                               (const int32_t*)at.idx, (const int64_t*)d_ptr, (const int32_t*)d_idx, nsub, overlap, cap, W, d_bm, d_cur,
                               (const int64_t*)d_ooff, d_out, d_sizes, d_err);
            if (hipGetLastError() != hipSuccess) { set_error("additive Schwarz: growth launch failed"); rc = KRYST_ERR_HIP; break; }
            unsigned long long e = KR_ASM_NOERR;
            if (hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                hipMemcpyAsync(sizes.data(), d_sizes, sizeof(int32_t) * sizes.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("additive Schwarz: growth failed on the device"); rc = KRYST_ERR_HIP; break; }
            if (e != KR_ASM_NOERR) {
                set_error("additive Schwarz: subdomain %lld grows past %d rows with overlap %d", (long long)e, cap, overlap);
                rc = KRYST_UNSUPPORTED; break;
            }
        }
        if (rc != KRYST_OK) break;
        idx.resize((size_t)ooff.back());
        if ((!idx.empty() && hipMemcpyAsync(idx.data(), d_out, sizeof(int32_t) * idx.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess) ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("additive Schwarz: growth failed on the device"); rc = KRYST_ERR_HIP; break; }
        ptr = ooff;
    } while (0);
    dev_csr_free(at);
    for (void* p : {(void*)d_ptr, (void*)d_idx, (void*)d_out, (void*)d_sizes, (void*)d_err, (void*)d_bm, (void*)d_cur, (void*)d_ooff}) (void)pool_free(p);
    return rc;
}

// grows the sorted sets (ptr, idx) by `overlap` layers on the device; on success (ptr, idx) hold the grown sets
int32_t asm_grow(kryst_csr_t a, int overlap, std::vector<int64_t>& ptr, std::vector<int32_t>& idx, int cap) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nsub = (int64_t)ptr.size() - 1;
    if (nsub == 0 || overlap <= 0) return KRYST_OK;
    if (cap > KR_ASM_MAX) return asm_grow_wide(a, overlap, ptr, idx, cap);
    DevCsr at;
    int64_t* d_ptr = nullptr; int32_t* d_idx = nullptr; int32_t* d_out = nullptr; int32_t* d_sizes = nullptr; unsigned long long* d_err = nullptr;
    std::vector<int32_t> sizes((size_t)nsub), out;
    unsigned long long e = KR_ASM_NOERR;
    int32_t rc = csr_transpose(ctx, "additive Schwarz", a->d_row_ptr, a->d_col, a->d_val, a->nrows, a->ncols, false, 0.0, at);
    do {
        if (rc != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &d_ptr, ptr, "index sets")) != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &d_idx, idx, "index sets")) != KRYST_OK) break;
        if (pool_malloc(&d_out, sizeof(int32_t) * (size_t)nsub * KR_ASM_MAX) != hipSuccess || pool_malloc(&d_sizes, sizeof(int32_t) * (size_t)nsub) != hipSuccess ||
            pool_malloc(&d_err, sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("additive Schwarz: out of device memory (growth of %lld subdomains)", (long long)nsub); rc = KRYST_ERR_HIP; break;
        }
        if (hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), ctx->s_main) != hipSuccess) { rc = KRYST_ERR_HIP; break; }
        hipLaunchKernelGGL(asm_grow_kernel, dim3(asm_grid(nsub, 1)), dim3(KR_ASM_T), 0, ctx->s_main, a->d_row_ptr, a->d_col, (const int32_t*)at.ptr,
                           (const int32_t*)at.idx, (const int64_t*)d_ptr, (const int32_t*)d_idx, nsub, overlap, d_out, d_sizes, d_err);
        if (hipGetLastError() != hipSuccess) { set_error("additive Schwarz: growth launch failed"); rc = KRYST_ERR_HIP; break; }
        if (hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipMemcpyAsync(sizes.data(), d_sizes, sizeof(int32_t) * sizes.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("additive Schwarz: growth failed on the device"); rc = KRYST_ERR_HIP; break; }
        if (e != KR_ASM_NOERR) {
            set_error("additive Schwarz: subdomain %lld grows past %d rows with overlap %d", (long long)e, KR_ASM_MAX, overlap);
            rc = KRYST_UNSUPPORTED; break;
        }
        out.resize((size_t)nsub * KR_ASM_MAX);
        if (hipMemcpyAsync(out.data(), d_out, sizeof(int32_t) * out.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("additive Schwarz: growth failed on the device"); rc = KRYST_ERR_HIP; break; }
    } while (0);
    dev_csr_free(at);
    (void)pool_free(d_ptr); (void)pool_free(d_idx); (void)pool_free(d_out); (void)pool_free(d_sizes); (void)pool_free(d_err);
    if (rc != KRYST_OK) return rc;
    ptr.assign((size_t)nsub + 1, 0);
    for (int64_t k = 0; k < nsub; ++k) ptr[(size_t)k + 1] = ptr[(size_t)k] + sizes[(size_t)k];
    KR_ARG(ptr.back() < INT32_MAX, "pc_asm: more than 2^31 - 1 subdomain rows after growth");
    idx.resize((size_t)ptr.back());
    for (int64_t k = 0; k < nsub; ++k)
        std::copy(out.begin() + k * KR_ASM_MAX, out.begin() + k * KR_ASM_MAX + sizes[(size_t)k], idx.begin() + ptr[(size_t)k]);
    return KRYST_OK;
}

// inverts every subdomain: the sets of at most 64 rows with one wave, the others with two
static int32_t asm_tiles_run(AsmPc* pc) {
    kryst_ctx_t ctx = pc->ctx;
    kryst_csr_t a = pc->a;
    std::vector<int32_t> small, large;
    int bsmall = 0, blarge = 0;
    for (int64_t k = 0; k < pc->nsub; ++k) {
        const int b = (int)(pc->ptr_h[(size_t)k + 1] - pc->ptr_h[(size_t)k]);
        if (b == 0) continue;
        if (b <= 64) { small.push_back((int32_t)k); bsmall = std::max(bsmall, b); }
        else { large.push_back((int32_t)k); blarge = std::max(blarge, b); }
    }
    if (small.empty() && large.empty()) return KRYST_OK;
    const size_t lds_large = sizeof(double) * (size_t)blarge * asm_stride(blarge);
    if (!large.empty()) {                                                   // the device's own limit, raised for this kernel on this device
        int lds_max = 0;
        KR_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
        if (lds_large + 2048 > (size_t)lds_max) {
            set_error("additive Schwarz: subdomains of %d rows need %zu bytes of LDS per workgroup; the device has %d", blarge, lds_large, lds_max);
            return KRYST_UNSUPPORTED;
        }
        KR_HIP(hipFuncSetAttribute((const void*)asm_tiles_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_large));
    }
    int32_t* d_small = nullptr; int32_t* d_large = nullptr; unsigned long long* d_err = nullptr;
    int32_t rc = asm_upload(ctx, &d_small, small, "subdomain lists");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &d_large, large, "subdomain lists");
    if (rc == KRYST_OK && pool_malloc(&d_err, sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError(); d_err = nullptr; set_error("additive Schwarz: out of device memory"); rc = KRYST_ERR_HIP;
    }
    if (rc == KRYST_OK && hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK) {
        if (!small.empty())
            hipLaunchKernelGGL(asm_tiles_kernel<64>, dim3(asm_grid((int64_t)small.size(), 1)), dim3(64), sizeof(double) * bsmall * asm_stride(bsmall),
                               ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, (const int32_t*)d_small, (int64_t)small.size(),
                               (const int32_t*)pc->d_xoff, (const int64_t*)pc->d_toff, (const int32_t*)pc->d_idx, pc->d_tile, d_err);
        if (!large.empty())
            hipLaunchKernelGGL(asm_tiles_kernel<128>, dim3(asm_grid((int64_t)large.size(), 1)), dim3(128), lds_large,
                               ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, (const int32_t*)d_large, (int64_t)large.size(),
                               (const int32_t*)pc->d_xoff, (const int64_t*)pc->d_toff, (const int32_t*)pc->d_idx, pc->d_tile, d_err);
        if (hipGetLastError() != hipSuccess) { set_error("additive Schwarz: set-up launch failed"); rc = KRYST_ERR_HIP; }
    }
    unsigned long long e = KR_ASM_NOERR;
    if (rc == KRYST_OK && (hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) {
        set_error("additive Schwarz: set-up failed on the device"); rc = KRYST_ERR_HIP;
    }
    (void)pool_free(d_small); (void)pool_free(d_large); (void)pool_free(d_err);
    if (rc != KRYST_OK || e == KR_ASM_NOERR) return rc;
    const int64_t k = (int64_t)(e >> 9);
    const int code = (int)((e >> 7) & 3ull), pos = (int)(e & 127ull);
    if (code == 0) {
        set_error("additive Schwarz: subdomain %lld holds a NaN or Inf", (long long)k);
        return KRYST_FACTOR_ERROR;
    }
    const int64_t row = (int64_t)pc->idx_h[(size_t)(pc->ptr_h[(size_t)k] + pos)];
    set_error("additive Schwarz: subdomain %lld is singular (zero pivot at row %lld)", (long long)k, (long long)row);
    set_error_row(row);
    return KRYST_ZERO_PIVOT;
}

// ---------------------------------------------------------------- the host bookkeeping shared with the ILU sub-solves (asm.h)
int32_t asm_sort_sets(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int cap, AsmSets& s) {
    const int64_t n = a->nrows;
    KR_ARG(nsub == 0 || sub_ptr[0] == 0, "pc_asm: sub_ptr[0] != 0");
    std::vector<int64_t>& ptr = s.ptr;
    ptr.assign((size_t)nsub + 1, 0);
    for (int64_t k = 0; k < nsub; ++k) {
        const int64_t len = sub_ptr[k + 1] - sub_ptr[k];
        KR_ARG(len >= 0, "pc_asm: sub_ptr is not ascending");
        if (len > cap) {
            set_error("additive Schwarz: subdomain %lld has %lld rows; at most %d are supported", (long long)k, (long long)len, cap);
            return KRYST_UNSUPPORTED;
        }
        ptr[(size_t)k + 1] = ptr[(size_t)k] + len;
    }
    KR_ARG(nsub == 0 || sub_idx || ptr.back() == 0, "pc_asm: sub_idx is NULL");
    KR_ARG(ptr.back() < INT32_MAX, "pc_asm: more than 2^31 - 1 subdomain rows");
    // sort each index set (deviation 2), check it, and find the owner of every row: the last un-grown set that contains it
    s.idx.assign((size_t)ptr.back(), 0);
    s.owner.assign((size_t)n, -1);
    for (int64_t k = 0; k < nsub; ++k) {
        const int64_t lo = ptr[(size_t)k], len = ptr[(size_t)k + 1] - lo;
        std::vector<int64_t> g(sub_idx + sub_ptr[k], sub_idx + sub_ptr[k] + len);
        std::sort(g.begin(), g.end());
        for (int64_t i = 0; i < len; ++i) {
            KR_ARG(g[(size_t)i] >= 0 && g[(size_t)i] < n, "pc_asm: index out of range");
            KR_ARG(i == 0 || g[(size_t)i] != g[(size_t)i - 1], "pc_asm: index repeated within a subdomain");
            s.idx[(size_t)(lo + i)] = (int32_t)g[(size_t)i];
            s.owner[(size_t)g[(size_t)i]] = (int32_t)k;
        }
    }
    return KRYST_OK;
}

void asm_row_map(int64_t n, int32_t variant, const AsmSets& s, std::vector<int32_t>& mptr, std::vector<int32_t>& mpos) {
    const std::vector<int64_t>& ptr = s.ptr;
    const std::vector<int32_t>& idx = s.idx;
    mptr.assign((size_t)n + 1, 0);
    mpos.clear();
    if (variant == KRYST_ASM_RESTRICTED) {
        for (int64_t row = 0; row < n; ++row) {
            const int32_t o = s.owner[(size_t)row];
            if (o >= 0) {
                const auto b = idx.begin() + ptr[(size_t)o], e = idx.begin() + ptr[(size_t)o + 1];
                mpos.push_back((int32_t)(std::lower_bound(b, e, (int32_t)row) - idx.begin()));
            }
            mptr[(size_t)row + 1] = (int32_t)mpos.size();
        }
    } else {
        for (int32_t r : idx) ++mptr[(size_t)r + 1];
        for (int64_t row = 0; row < n; ++row) mptr[(size_t)row + 1] += mptr[(size_t)row];
        mpos.resize(idx.size());
        std::vector<int32_t> fill(mptr.begin(), mptr.end() - 1);
        for (size_t p = 0; p < idx.size(); ++p) mpos[(size_t)fill[(size_t)idx[p]]++] = (int32_t)p;   // ascending p = ascending subdomain
    }
}

void asm_uniform_sets(int64_t n, int64_t nparts, std::vector<int64_t>& ptr, std::vector<int64_t>& idx) {
    const int64_t p = std::max<int64_t>(nparts, 1), chunk = (n + p - 1) / p;
    ptr.assign((size_t)p + 1, 0);
    idx.clear();
    idx.reserve((size_t)n);
    for (int64_t i = 0; i < p; ++i) {
        const int64_t s = i * chunk, e = std::min((i + 1) * chunk, n);
        for (int64_t r = s; r < e; ++r) idx.push_back(r);
        ptr[(size_t)i + 1] = (int64_t)idx.size();
    }
}

// the common set-up over index sets packed like CSR rows (unsorted, possibly overlapping, possibly leaving rows uncovered)
static int32_t asm_setup(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant,
                         kryst_pc_t* out) {
    const int64_t n = a->nrows;
    AsmSets sets;
    KR_TRY(asm_sort_sets(a, sub_ptr, sub_idx, nsub, KR_ASM_MAX, sets));
    std::vector<int64_t>& ptr = sets.ptr;
    std::vector<int32_t>& idx = sets.idx;
    unsigned long long sb = 0, sb2 = 0;
    for (int64_t k = 0; k < nsub; ++k) {
        const unsigned long long b = (unsigned long long)(ptr[(size_t)k + 1] - ptr[(size_t)k]);
        sb += b; sb2 += b * b;
    }
    KR_HIP(hipSetDevice(a->ctx->device));
    // the un-grown sets bound the grown ones from below: a request that cannot fit fails before anything is allocated
    KR_TRY(asm_check_memory(a->ctx->device, asm_bytes(n, nsub, sb, sb2, sb)));
    if (variant != KRYST_ASM_AS_WRITTEN) KR_TRY(asm_grow(a, overlap, ptr, idx, KR_ASM_MAX));
    sb = 0; sb2 = 0;
    int bmax = 0;
    for (int64_t k = 0; k < nsub; ++k) {
        const unsigned long long b = (unsigned long long)(ptr[(size_t)k + 1] - ptr[(size_t)k]);
        sb += b; sb2 += b * b; bmax = std::max(bmax, (int)b);
    }
    std::vector<int32_t> mptr, mpos;
    asm_row_map(n, variant, sets, mptr, mpos);
    KR_TRY(asm_check_memory(a->ctx->device, asm_bytes(n, nsub, sb, sb2, mpos.size())));
    std::vector<int32_t> xoff((size_t)nsub + 1), posk(idx.size());
    std::vector<int64_t> toff((size_t)nsub + 1, 0);
    for (int64_t k = 0; k < nsub; ++k) {
        const int64_t b = ptr[(size_t)k + 1] - ptr[(size_t)k];
        xoff[(size_t)k] = (int32_t)ptr[(size_t)k];
        toff[(size_t)k + 1] = toff[(size_t)k] + b * b;
        std::fill(posk.begin() + ptr[(size_t)k], posk.begin() + ptr[(size_t)k + 1], (int32_t)k);
    }
    xoff[(size_t)nsub] = (int32_t)ptr.back();
    AsmPc* pc = new AsmPc(a, nsub, (int64_t)idx.size(), bmax);
    kryst_ctx_t ctx = a->ctx;
    int32_t rc = asm_upload(ctx, &pc->d_xoff, xoff, "subdomain offsets");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &pc->d_toff, toff, "tile offsets");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &pc->d_idx, idx, "index sets");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &pc->d_posk, posk, "position map");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &pc->d_mptr, mptr, "row map");
    if (rc == KRYST_OK) rc = asm_upload(ctx, &pc->d_mpos, mpos, "row map");
    if (rc == KRYST_OK && pool_malloc(&pc->d_x, sizeof(double) * (size_t)std::max<int64_t>(pc->total, 1)) != hipSuccess) {
        (void)hipGetLastError(); pc->d_x = nullptr;
        set_error("additive Schwarz: out of device memory (%lld subdomain rows)", (long long)pc->total); rc = KRYST_ERR_HIP;
    }
    if (rc == KRYST_OK && pool_malloc(&pc->d_tile, sizeof(double) * (size_t)std::max<int64_t>(toff.back(), 1)) != hipSuccess) {
        (void)hipGetLastError(); pc->d_tile = nullptr;
        set_error("additive Schwarz: out of device memory for %lld tile entries", (long long)toff.back()); rc = KRYST_ERR_HIP;
    }
    pc->ptr_h = std::move(sets.ptr); pc->idx_h = std::move(sets.idx); pc->owner_h = std::move(sets.owner);
    if (rc == KRYST_OK) rc = asm_tiles_run(pc);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

int32_t asm_check(kryst_csr_t a, int32_t overlap, int32_t variant) {
    if (a->dist) { set_error("additive Schwarz: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->ncols && a->nrows == a->xlen, "pc_asm: square operator required");
    KR_ARG(a->nrows < INT32_MAX, "pc_asm: more than 2^31 - 1 rows");
    KR_ARG(overlap >= 0, "pc_asm: overlap < 0");
    KR_ARG(variant == KRYST_ASM_AS_WRITTEN || variant == KRYST_ASM_GROWN || variant == KRYST_ASM_RESTRICTED, "pc_asm: unknown variant");
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_asm(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant, kryst_pc_t* out) {
    KR_ARG(a && out && nsub >= 0 && (sub_ptr || nsub == 0), "pc_asm");
    KR_TRY(asm_check(a, overlap, variant));
    return asm_setup(a, sub_ptr, sub_idx, nsub, overlap, variant, out);
}

// asm.rs:46-56: p = max(nparts, 1) parts of chunk = ceil(n / p) rows, part i = [i chunk, min((i + 1) chunk, n)) (trailing parts may be empty)
int32_t kryst_pc_asm_uniform(kryst_csr_t a, int64_t nparts, int32_t overlap, int32_t variant, kryst_pc_t* out) {
    KR_ARG(a && out && nparts >= 0, "pc_asm_uniform");
    KR_TRY(asm_check(a, overlap, variant));
    std::vector<int64_t> ptr, idx;
    asm_uniform_sets(a->nrows, nparts, ptr, idx);
    return asm_setup(a, ptr.data(), idx.data(), (int64_t)ptr.size() - 1, overlap, variant, out);
}

int32_t kryst_pc_asm_info(kryst_pc_t h, int64_t* nsub, int64_t* ext_rows, int32_t* max_rows) {
    AsmPc* pc = pc_cast<AsmPc>(h);
    KR_ARG(pc, "pc_asm_info");
    if (nsub) *nsub = pc->nsub;
    if (ext_rows) *ext_rows = pc->total;
    if (max_rows) *max_rows = pc->maxb;
    return KRYST_OK;
}

int32_t kryst_pc_asm_export(kryst_pc_t h, int64_t* sub_ptr, int32_t* sub_idx, int32_t* owner, double* tiles) {
    AsmPc* pc = pc_cast<AsmPc>(h);
    KR_ARG(pc, "pc_asm_export");
    if (sub_ptr) std::copy(pc->ptr_h.begin(), pc->ptr_h.end(), sub_ptr);
    if (sub_idx) std::copy(pc->idx_h.begin(), pc->idx_h.end(), sub_idx);
    if (owner) std::copy(pc->owner_h.begin(), pc->owner_h.end(), owner);
    if (tiles) {
        int64_t entries = 0;
        for (int64_t k = 0; k < pc->nsub; ++k) {
            const int64_t b = pc->ptr_h[(size_t)k + 1] - pc->ptr_h[(size_t)k];
            entries += b * b;
        }
        KR_HIP(hipSetDevice(pc->ctx->device));
        if (entries > 0) KR_HIP(hipMemcpyAsync(tiles, pc->d_tile, sizeof(double) * (size_t)entries, hipMemcpyDeviceToHost, pc->ctx->s_main));
        KR_HIP(hipStreamSynchronize(pc->ctx->s_main));
    }
    return KRYST_OK;
}

}  // extern "C"
