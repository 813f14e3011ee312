// Block Jacobi (BlockJacobi, src/preconditioner/block_jacobi.rs) on the device, with three labelled deviations (DESIGN.md
// section 4.5): each block is inverted explicitly (Gauss-Jordan with full pivoting, the textbook `gaussj` order) instead of
// kept as faer's FullPivLu; the indices of a block are sorted ascending before the block matrix is formed; a singular or
// non-finite block, a bad index and a non-square operator are errors instead of non-finite output or a panic.
//
// Set-up: one wavefront inverts floor(64 / b) blocks of b <= 32 rows (one block of 33..64 rows), one row per lane, the tiles in LDS.
// Apply: z[g[i]] = sum_j Binv[i][j] * r[g[j]] (ascending j from +0.0, no FMA), the tiles stored block after block, column-major
// inside a tile, r[g[j]] loaded once per lane and broadcast inside the block with a cross-lane shuffle.
#include "pc.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace kr {

constexpr int KR_BJ_MAX = 64;                 // rows per block: one lane each
constexpr int KR_BJ_APPLY_T = 256;            // apply: 4 waves per workgroup
constexpr int64_t KR_BJ_GRID_CAP = 1 << 20;   // workgroups; both kernels stride over the waves beyond it

// LDS row stride of a tile of b rows: odd, so that the lanes' rows start in different banks
__host__ __device__ inline int bj_stride(int b) { return b + ((b & 1) ? 0 : 1); }

// error word of the set-up: min over the failing blocks of (block << 8 | code << 6 | position); code 0: non-finite entry, 1: zero pivot
// (position = the smallest block position not yet pivoted)
constexpr unsigned long long KR_BJ_NOERR = ~0ull;

// Where wave w's lane sits: the block k it works on (-1: none), its position i in it, the block's size bk, the first lane of the
// block, the block's first index in the sorted stream (index-set form) and its tile's offset.
struct BjLane { int64_t k; int i, bk, seg, bw; int64_t lo, tbase; };

template <bool IDX>
__device__ __forceinline__ BjLane bj_lane(int64_t w, int lane, int64_t nblk, int b, int64_t n, const int64_t* ptr, const int64_t* toff) {
    BjLane L;
    if (!IDX) {                                   // contiguous: floor(64/b) blocks of b rows per wave, the last block of all shorter
        const int P = KR_BJ_MAX / b;
        const int sub = lane / b;
        L.i = lane - sub * b; L.seg = sub * b; L.bw = b;
        L.k = (sub < P) ? w * P + sub : -1;
        if (L.k >= nblk) L.k = -1;
        L.lo = (L.k >= 0) ? L.k * (int64_t)b : 0;
        L.bk = (L.k >= 0) ? (int)min<int64_t>((int64_t)b, n - L.lo) : 0;
        L.tbase = L.lo * (int64_t)b;              // every earlier block is full: k b^2
    } else {                                      // index sets: one block per wave
        L.k = w; L.i = lane; L.seg = 0;
        L.lo = ptr[w]; L.bk = (int)(ptr[w + 1] - L.lo); L.bw = L.bk;
        L.tbase = toff[w];
    }
    return L;
}

// ---------------------------------------------------------------- set-up: gather the tile, invert it in LDS, store it column-major
template <bool IDX>
__global__ __launch_bounds__(64) void bj_setup_kernel(const int32_t* row_ptr, const int32_t* col, const double* val, int64_t n,
                                                      int64_t nblk, int b, const int64_t* ptr, const int64_t* toff, const int32_t* idx,
                                                      double* tiles, unsigned long long* err) {
    extern __shared__ double bj_lds[];
    const int lane = threadIdx.x;
    const int64_t nwaves = IDX ? nblk : (nblk + KR_BJ_MAX / b - 1) / (KR_BJ_MAX / b);
    for (int64_t w = blockIdx.x; w < nwaves; w += gridDim.x) {              // uniform over the workgroup (= one wave)
        const BjLane L = bj_lane<IDX>(w, lane, nblk, b, n, ptr, toff);
        const int bs = bj_stride(L.bw);
        const bool act = L.k >= 0 && L.i < L.bk;                            // this lane owns row i (and column i) of block k
        double* T = bj_lds + (IDX ? 0 : (L.seg / max(L.bw, 1)) * L.bw * bs);
        // gather: B[i][j] = A(g[i], g[j]) when stored, else +0.0
        if (act) {
            for (int l = 0; l < L.bk; ++l) T[L.i * bs + l] = 0.0;
            const int64_t gi = IDX ? (int64_t)idx[L.lo + L.i] : L.lo + L.i;
            bool bad = false;
            for (int32_t e = row_ptr[gi]; e < row_ptr[gi + 1]; ++e) {
                const int64_t c = col[e];
                int j = -1;
                if (!IDX) {
                    if (c >= L.lo && c < L.lo + L.bk) j = (int)(c - L.lo);
                } else {                                                    // binary search in the sorted index set
                    int lo = 0, hi = L.bk;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)idx[L.lo + mid] < c) lo = mid + 1; else hi = mid; }
                    if (lo < L.bk && (int64_t)idx[L.lo + lo] == c) j = lo;
                }
                if (j >= 0) { const double v = val[e]; T[L.i * bs + j] = v; bad |= !isfinite(v); }
            }
            if (bad) atomicMin(err, ((unsigned long long)L.k << 8) | (0ull << 6));
        }
        __syncthreads();
        // Gauss-Jordan with full pivoting, step s of every block of the wave together (the loops are uniform over the wave so that
        // every lane takes part in every shuffle; `dead`: the block met a zero pivot and stops)
        unsigned long long pivoted = 0ull;
        bool dead = false;
        int my_r = 0, my_c = 0;                                             // (row_s, col_s) of step s = i, kept by lane i
        for (int s = 0; s < L.bw; ++s) {
            // this row's best candidate over the columns not pivoted: scan ascending, a later one wins only if strictly greater
            double best = -1.0; int bj = 0;
            if (act && s < L.bk && !((pivoted >> L.i) & 1ull)) {
                for (int l = 0; l < L.bk; ++l) {
                    if ((pivoted >> l) & 1ull) continue;
                    const double a = fabs(T[L.i * bs + l]);
                    if (a > best) { best = a; bj = l; }
                }
            }
            // reduction over the block's lanes: larger |value| wins, the smaller row on a tie (= the row-major scan order)
            int bi = L.i;
            for (int off = 1; off < L.bw; off <<= 1) {
                const double ob = __shfl(best, lane + off, 64);
                const int oi = __shfl(bi, lane + off, 64), oj = __shfl(bj, lane + off, 64);
                if (L.i + off < L.bw && (ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; bj = oj; }
            }
            best = __shfl(best, L.seg, 64); bi = __shfl(bi, L.seg, 64); bj = __shfl(bj, L.seg, 64);
            const bool step = L.k >= 0 && s < L.bk && !dead;
            if (step && best == 0.0) {                                      // the chosen pivot is 0
                dead = true;
                if (L.i == 0) {
                    const int pos = __builtin_ctzll(~pivoted);
                    atomicMin(err, ((unsigned long long)L.k << 8) | (1ull << 6) | (unsigned long long)pos);
                }
            }
            const bool go = step && !dead;
            const int p = bi, q = bj;
            double piv = 0.0;
            if (go) piv = T[p * bs + q];
            __syncthreads();
            if (go && act && p != q) {                                      // swap rows p and q (lane i: column i)
                const double t = T[p * bs + L.i]; T[p * bs + L.i] = T[q * bs + L.i]; T[q * bs + L.i] = t;
            }
            if (go && L.i == s) { my_r = p; my_c = q; }
            if (go) pivoted |= 1ull << q;
            __syncthreads();
            if (go && act) {                                                // pivinv = 1/B[q][q]; B[q][q] = 1; B[q][l] *= pivinv
                const double pivinv = 1.0 / piv;
                const double v = (L.i == q) ? 1.0 : T[q * bs + L.i];
                T[q * bs + L.i] = v * pivinv;
            }
            __syncthreads();
            if (go && act && L.i != q) {                                    // row m = i: f = B[m][q]; B[m][q] = 0; B[m][l] -= B[q][l] * f
                double* Tm = T + L.i * bs;
                const double* Tq = T + q * bs;
                const double f = Tm[q];
                Tm[q] = 0.0;
                for (int l = 0; l < L.bk; ++l) Tm[l] = Tm[l] - Tq[l] * f;
            }
            __syncthreads();
        }
        // undo the column permutation: for s = b-1 down to 0, swap columns row_s and col_s (lane i: its own row)
        for (int s = L.bw - 1; s >= 0; --s) {
            const int rs = __shfl(my_r, L.seg + s, 64), cs = __shfl(my_c, L.seg + s, 64);
            if (act && !dead && s < L.bk && rs != cs) {
                double* Tm = T + L.i * bs;
                const double t = Tm[rs]; Tm[rs] = Tm[cs]; Tm[cs] = t;
            }
        }
        __syncthreads();
        if (act && !dead)
            for (int j = 0; j < L.bk; ++j) tiles[L.tbase + (int64_t)j * L.bk + L.i] = T[L.i * bs + j];
        __syncthreads();                                                    // the next wave's gather reuses the LDS
    }
}

// ---------------------------------------------------------------- apply
template <bool IDX>
__global__ __launch_bounds__(KR_BJ_APPLY_T) void bj_apply_kernel(const double* tiles, int64_t n, int64_t nblk, int b, const int64_t* ptr,
                                                                 const int64_t* toff, const int32_t* idx, const int32_t* owner,
                                                                 const double* r, double* z, const int* done) {
    if (done && *done) return;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = IDX ? nblk : (nblk + KR_BJ_MAX / b - 1) / (KR_BJ_MAX / b);
    const int64_t wstride = (int64_t)gridDim.x * (KR_BJ_APPLY_T / 64);
    for (int64_t w = (int64_t)blockIdx.x * (KR_BJ_APPLY_T / 64) + (threadIdx.x >> 6); w < nwaves; w += wstride) {   // uniform over the wave
        const BjLane L = bj_lane<IDX>(w, lane, nblk, b, n, ptr, toff);
        const bool act = L.k >= 0 && L.i < L.bk;
        const int64_t row = act ? (IDX ? (int64_t)idx[L.lo + L.i] : L.lo + L.i) : 0;
        const double rv = act ? r[row] : 0.0;
        double s = 0.0;
        const double* t = tiles + L.tbase + L.i;
        for (int j = 0; j < L.bw; ++j) {
            const double rj = __shfl(rv, L.seg + j, 64);                    // r[g[j]] from lane j of the block
            if (act && j < L.bk) s = s + t[(int64_t)j * L.bk] * rj;
        }
        if (act && (!owner || owner[row] == (int32_t)L.k)) z[row] = s;    // the last block that contains a row decides it
    }
}

__global__ void bj_zero_uncovered_kernel(const int32_t* owner, int64_t n, double* z, const int* done) {
    if (done && *done) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (owner[i] < 0) z[i] = 0.0;
}

static unsigned bj_grid(int64_t waves, int waves_per_wg) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + waves_per_wg - 1) / waves_per_wg, KR_BJ_GRID_CAP));
}

// the inverted tiles block after block, column-major inside a tile
struct BlockJacobiPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_BLOCK_JACOBI;
    int32_t bsize = 0;                // contiguous form: blocks of bsize consecutive rows, the last one shorter; 0: index-set form
    int64_t nblk = 0;
    int64_t uncovered = 0;            // rows in no block (index-set form): z = +0.0 there
    double* d_tile = nullptr;
    int64_t* d_ptr = nullptr; int64_t* d_toff = nullptr;   // index-set form: block offsets into d_idx, tile offsets
    int32_t* d_idx = nullptr;         // index-set form: each block's indices, sorted ascending
    int32_t* d_owner = nullptr;       // index-set form with overlapping blocks or uncovered rows: the last block containing a row, or -1
    std::vector<int64_t> ptr_h; std::vector<int32_t> idx_h;
    BlockJacobiPc(kryst_csr_t a_, int32_t bsize_, int64_t nblk_, int64_t uncovered_)
        : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), bsize(bsize_), nblk(nblk_), uncovered(uncovered_) {}
    ~BlockJacobiPc() override { (void)hipFree(d_tile); (void)hipFree(d_ptr); (void)hipFree(d_toff); (void)hipFree(d_idx); (void)hipFree(d_owner); }
    int64_t nwaves() const { return bsize > 0 ? (nblk + KR_BJ_MAX / bsize - 1) / (KR_BJ_MAX / bsize) : nblk; }
    int32_t apply(int64_t nv, const double* r, double* z, const int* done) override;
};

int32_t BlockJacobiPc::apply(int64_t, const double* r, double* z, const int* done) {
    if (uncovered > 0) {
        hipLaunchKernelGGL(bj_zero_uncovered_kernel, dim3(bj_grid(n, 256)), dim3(256), 0, ctx->s_main, d_owner, n, z, done);
        KR_HIP(hipGetLastError());
    }
    const int64_t waves = nwaves();
    if (waves == 0) return KRYST_OK;
    if (bsize > 0)
        hipLaunchKernelGGL(bj_apply_kernel<false>, dim3(bj_grid(waves, KR_BJ_APPLY_T / 64)), dim3(KR_BJ_APPLY_T), 0, ctx->s_main,
                           (const double*)d_tile, n, nblk, bsize, (const int64_t*)nullptr, (const int64_t*)nullptr,
                           (const int32_t*)nullptr, (const int32_t*)nullptr, r, z, done);
    else
        hipLaunchKernelGGL(bj_apply_kernel<true>, dim3(bj_grid(waves, KR_BJ_APPLY_T / 64)), dim3(KR_BJ_APPLY_T), 0, ctx->s_main,
                           (const double*)d_tile, n, nblk, 0, (const int64_t*)d_ptr, (const int64_t*)d_toff,
                           (const int32_t*)d_idx, (const int32_t*)d_owner, r, z, done);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// runs the set-up kernel over pc's blocks and turns its error word into a status (bmax: the largest block)
static int32_t bj_setup_run(BlockJacobiPc* pc, int bmax) {
    kryst_ctx_t ctx = pc->ctx;
    kryst_csr_t a = pc->a;
    const int64_t waves = pc->nwaves();
    if (waves == 0 || bmax == 0) return KRYST_OK;
    unsigned long long* d_err = nullptr;
    KR_HIP(hipMalloc(&d_err, sizeof(unsigned long long)));
    int32_t rc = KRYST_OK;
    if (hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
    const int bs = bj_stride(bmax);
    const size_t lds = sizeof(double) * (size_t)(pc->bsize > 0 ? (KR_BJ_MAX / bmax) * bmax * bs : bmax * bs);
    if (rc == KRYST_OK) {
        if (pc->bsize > 0)
            hipLaunchKernelGGL(bj_setup_kernel<false>, dim3(bj_grid(waves, 1)), dim3(64), lds, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val,
                               pc->n, pc->nblk, pc->bsize, (const int64_t*)nullptr, (const int64_t*)nullptr, (const int32_t*)nullptr,
                               pc->d_tile, d_err);
        else
            hipLaunchKernelGGL(bj_setup_kernel<true>, dim3(bj_grid(waves, 1)), dim3(64), lds, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val,
                               pc->n, pc->nblk, 0, (const int64_t*)pc->d_ptr, (const int64_t*)pc->d_toff, (const int32_t*)pc->d_idx,
                               pc->d_tile, d_err);
        if (hipGetLastError() != hipSuccess) { set_error("block Jacobi: set-up launch failed"); rc = KRYST_ERR_HIP; }
    }
    unsigned long long e = KR_BJ_NOERR;
    if (rc == KRYST_OK && (hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) {
        set_error("block Jacobi: set-up failed on the device"); rc = KRYST_ERR_HIP;
    }
    (void)hipFree(d_err);
    if (rc != KRYST_OK || e == KR_BJ_NOERR) return rc;
    const int64_t k = (int64_t)(e >> 8);
    const int code = (int)((e >> 6) & 3ull), pos = (int)(e & 63ull);
    if (code == 0) {
        set_error("block Jacobi: block %lld holds a NaN or Inf", (long long)k);
        return KRYST_FACTOR_ERROR;
    }
    const int64_t row = pc->bsize > 0 ? k * pc->bsize + pos : (int64_t)pc->idx_h[(size_t)pc->ptr_h[(size_t)k] + pos];
    set_error("block Jacobi: block %lld is singular (zero pivot at row %lld)", (long long)k, (long long)row);
    set_error_row(row);
    return KRYST_ZERO_PIVOT;
}

static int32_t bj_check_operator(kryst_csr_t a) {
    if (a->dist) { set_error("block Jacobi: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->ncols && a->nrows == a->xlen, "pc_block_jacobi: square operator required");
    KR_ARG(a->nrows < INT32_MAX, "pc_block_jacobi: more than 2^31 - 1 rows");
    return KRYST_OK;
}

template <class T> static int32_t bj_upload(kryst_ctx_t ctx, T** d, const std::vector<T>& h) {
    KR_HIP(hipMalloc(d, sizeof(T) * std::max<size_t>(h.size(), 1)));
    if (!h.empty()) KR_HIP(hipMemcpyAsync(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->s_main));
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_block_jacobi(kryst_csr_t a, const int64_t* blk_ptr, const int64_t* blk_idx, int64_t nblocks, kryst_pc_t* out) {
    KR_ARG(a && out && nblocks >= 0 && (blk_ptr || nblocks == 0), "pc_block_jacobi");
    KR_TRY(bj_check_operator(a));
    const int64_t n = a->nrows;
    KR_ARG(nblocks == 0 || blk_ptr[0] == 0, "pc_block_jacobi: blk_ptr[0] != 0");
    std::vector<int64_t> ptr((size_t)nblocks + 1, 0), toff((size_t)nblocks + 1, 0);
    int bmax = 0;
    for (int64_t k = 0; k < nblocks; ++k) {
        const int64_t len = blk_ptr[k + 1] - blk_ptr[k];
        KR_ARG(len >= 0, "pc_block_jacobi: blk_ptr is not ascending");
        if (len > KR_BJ_MAX) {
            set_error("block Jacobi: block %lld has %lld rows; at most %d are supported", (long long)k, (long long)len, KR_BJ_MAX);
            return KRYST_UNSUPPORTED;
        }
        ptr[(size_t)k + 1] = ptr[(size_t)k] + len;
        toff[(size_t)k + 1] = toff[(size_t)k] + len * len;
        bmax = std::max(bmax, (int)len);
    }
    KR_ARG(nblocks == 0 || blk_idx || ptr.back() == 0, "pc_block_jacobi: blk_idx is NULL");
    // sort each index set (deviation 2), check it, and find the owner of every row: the last block that contains it
    std::vector<int32_t> idx((size_t)ptr.back());
    std::vector<int32_t> owner((size_t)n, -1);
    bool overlap = false;
    for (int64_t k = 0; k < nblocks; ++k) {
        const int64_t lo = ptr[(size_t)k], len = ptr[(size_t)k + 1] - lo;
        std::vector<int64_t> g(blk_idx + blk_ptr[k], blk_idx + blk_ptr[k] + len);
        std::sort(g.begin(), g.end());
        for (int64_t i = 0; i < len; ++i) {
            KR_ARG(g[(size_t)i] >= 0 && g[(size_t)i] < n, "pc_block_jacobi: index out of range");
            KR_ARG(i == 0 || g[(size_t)i] != g[(size_t)i - 1], "pc_block_jacobi: index repeated within a block");
            idx[(size_t)(lo + i)] = (int32_t)g[(size_t)i];
            int32_t& o = owner[(size_t)g[(size_t)i]];
            overlap |= o >= 0;
            o = (int32_t)k;
        }
    }
    const int64_t uncovered = std::count(owner.begin(), owner.end(), -1);
    KR_HIP(hipSetDevice(a->ctx->device));
    BlockJacobiPc* pc = new BlockJacobiPc(a, 0, nblocks, uncovered);
    int32_t rc = bj_upload(a->ctx, &pc->d_ptr, ptr);
    if (rc == KRYST_OK) rc = bj_upload(a->ctx, &pc->d_toff, toff);
    if (rc == KRYST_OK) rc = bj_upload(a->ctx, &pc->d_idx, idx);
    if (rc == KRYST_OK && (overlap || uncovered > 0)) rc = bj_upload(a->ctx, &pc->d_owner, owner);   // only then is an owner test needed
    if (rc == KRYST_OK && hipMalloc(&pc->d_tile, sizeof(double) * (size_t)std::max<int64_t>(toff.back(), 1)) != hipSuccess) {
        set_error("block Jacobi: out of device memory for %lld tile entries", (long long)toff.back()); rc = KRYST_ERR_HIP;
    }
    pc->ptr_h = std::move(ptr); pc->idx_h = std::move(idx);
    if (rc == KRYST_OK) rc = bj_setup_run(pc, bmax);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

int32_t kryst_pc_block_jacobi_uniform(kryst_csr_t a, int32_t bsize, kryst_pc_t* out) {
    KR_ARG(a && out && bsize >= 1, "pc_block_jacobi_uniform");
    KR_TRY(bj_check_operator(a));
    if (bsize > KR_BJ_MAX) {
        set_error("block Jacobi: blocks of %d rows; at most %d are supported", (int)bsize, KR_BJ_MAX);
        return KRYST_UNSUPPORTED;
    }
    const int64_t n = a->nrows;
    KR_HIP(hipSetDevice(a->ctx->device));
    BlockJacobiPc* pc = new BlockJacobiPc(a, bsize, (n + bsize - 1) / bsize, 0);
    const int64_t last = n - (pc->nblk - 1) * bsize;                    // rows of the last block
    const int64_t entries = pc->nblk > 0 ? (pc->nblk - 1) * (int64_t)bsize * bsize + last * last : 0;
    int32_t rc = KRYST_OK;
    if (hipMalloc(&pc->d_tile, sizeof(double) * (size_t)std::max<int64_t>(entries, 1)) != hipSuccess) {
        set_error("block Jacobi: out of device memory for %lld tile entries", (long long)entries); rc = KRYST_ERR_HIP;
    }
    if (rc == KRYST_OK) rc = bj_setup_run(pc, bsize);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

// M as CSR: row g[i] of the block that owns it holds (g[j], Binv[i][j]) for every j of that block, ascending; other rows are empty
int32_t kryst_pc_block_jacobi_export(kryst_pc_t h, int64_t* nnz, int64_t* row_ptr, int32_t* col, double* val) {
    BlockJacobiPc* pc = pc_cast<BlockJacobiPc>(h);
    KR_ARG(pc && nnz, "pc_block_jacobi_export");
    KR_ARG(!row_ptr || (col && val), "pc_block_jacobi_export: col / val are NULL");
    const int64_t n = pc->n, nblk = pc->nblk;
    const int64_t b = pc->bsize;
    auto block_lo = [&](int64_t k) { return b > 0 ? k * b : pc->ptr_h[(size_t)k]; };
    auto block_len = [&](int64_t k) { return b > 0 ? std::min<int64_t>(b, n - k * b) : pc->ptr_h[(size_t)k + 1] - pc->ptr_h[(size_t)k]; };
    // the owning block of every row and the row's position in it (the index-set form keeps an owner stream only when blocks overlap or
    // leave rows uncovered; otherwise every row is in exactly one block)
    std::vector<int32_t> own, posn;
    if (b == 0) {
        own.assign((size_t)n, -1); posn.assign((size_t)n, -1);
        for (int64_t k = 0; k < nblk; ++k)
            for (int64_t e = pc->ptr_h[(size_t)k]; e < pc->ptr_h[(size_t)k + 1]; ++e) {
                const int32_t r = pc->idx_h[(size_t)e];
                own[(size_t)r] = (int32_t)k; posn[(size_t)r] = (int32_t)(e - pc->ptr_h[(size_t)k]);   // the last block wins
            }
    }
    auto owner = [&](int64_t r) -> int64_t { return b > 0 ? r / b : (int64_t)own[(size_t)r]; };
    int64_t total = 0;
    for (int64_t r = 0; r < n; ++r) { const int64_t k = owner(r); if (k >= 0) total += block_len(k); }
    *nnz = total;
    if (!row_ptr) return KRYST_OK;
    std::vector<int64_t> toff((size_t)nblk + 1, 0);
    for (int64_t k = 0; k < nblk; ++k) toff[(size_t)k + 1] = toff[(size_t)k] + block_len(k) * block_len(k);
    std::vector<double> tiles((size_t)toff.back());
    KR_HIP(hipSetDevice(pc->ctx->device));
    if (!tiles.empty())
        KR_HIP(hipMemcpyAsync(tiles.data(), pc->d_tile, sizeof(double) * tiles.size(), hipMemcpyDeviceToHost, pc->ctx->s_main));
    KR_HIP(hipStreamSynchronize(pc->ctx->s_main));
    int64_t e = 0;
    row_ptr[0] = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t k = owner(r);
        if (k >= 0) {
            const int64_t lo = block_lo(k), bk = block_len(k);
            const int64_t i = b > 0 ? r - lo : posn[(size_t)r];
            for (int64_t j = 0; j < bk; ++j, ++e) {
                col[e] = b > 0 ? (int32_t)(lo + j) : pc->idx_h[(size_t)(lo + j)];
                val[e] = tiles[(size_t)(toff[(size_t)k] + j * bk + i)];
            }
        }
        row_ptr[r + 1] = e;
    }
    return KRYST_OK;
}

}  // extern "C"
