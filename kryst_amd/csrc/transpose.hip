// The deterministic device transpose shared by the SPAI set-up (spai.hip: A's columns, M's rows) and the transposed SpMV
// (csr_create.hip: csr_transpose_operator).  Counts per output segment by atomics, an exclusive scan, atomic slots, then every segment
// sorted by its input row: the atomics decide only the arrival order inside a segment, which the sort erases, so the result does not
// depend on scheduling.  Segment j lists the entries of input column j in ascending input row; the input rows' own column order is
// irrelevant (each row contributes at most one entry to a segment).
#include "csr.h"
#include <algorithm>

namespace kr {

constexpr int KR_TR_SCAN_CH = 2048;     // scan: elements per workgroup (256 threads x 8)
constexpr int64_t KR_TR_GRID_CAP = 1 << 20;

static unsigned tr_grid(int64_t items, int per_wg) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_wg - 1) / per_wg, KR_TR_GRID_CAP));
}

// ---------------------------------------------------------------- transpose: (ptr, idx, val) rows -> segments by idx, rows ascending
template <bool DROP>
__global__ void tr_count_kernel(const int32_t* ptr, const int32_t* idx, const double* val, int64_t nin, double tol, int32_t* cnt) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nin; r += (int64_t)gridDim.x * blockDim.x)
        for (int32_t e = ptr[r]; e < ptr[r + 1]; ++e)
            if (!DROP || fabs(val[e]) > tol) atomicAdd(&cnt[idx[e]], 1);
}

template <bool DROP>
__global__ void tr_fill_kernel(const int32_t* ptr, const int32_t* idx, const double* val, int64_t nin, double tol, const int32_t* off,
                                 int32_t* cur, int32_t* oidx, double* oval) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nin; r += (int64_t)gridDim.x * blockDim.x)
        for (int32_t e = ptr[r]; e < ptr[r + 1]; ++e) {
            const double v = val[e];
            if (DROP && !(fabs(v) > tol)) continue;
            const int32_t c = idx[e];
            const int32_t s = off[c] + atomicAdd(&cur[c], 1);
            oidx[s] = (int32_t)r; oval[s] = v;
        }
}

// the atomic slots leave each segment in arrival order: sort it by row (rows are unique within a segment, so the result is the same
// whatever the arrival order); insertion sort for short segments, heapsort beyond
__global__ void tr_sort_kernel(const int32_t* off, int64_t nout, int32_t* oidx, double* oval) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nout; c += (int64_t)gridDim.x * blockDim.x) {
        int32_t* K = oidx + off[c];
        double* V = oval + off[c];
        const int len = off[c + 1] - off[c];
        if (len <= 32) {
            for (int i = 1; i < len; ++i) {
                const int32_t key = K[i]; const double v = V[i];
                int p = i - 1;
                while (p >= 0 && K[p] > key) { K[p + 1] = K[p]; V[p + 1] = V[p]; --p; }
                K[p + 1] = key; V[p + 1] = v;
            }
            continue;
        }
        auto sift = [&](int root, int end) {
            while (2 * root + 1 < end) {
                int ch = 2 * root + 1;
                if (ch + 1 < end && K[ch + 1] > K[ch]) ++ch;
                if (K[root] >= K[ch]) return;
                const int32_t tk = K[root]; K[root] = K[ch]; K[ch] = tk;
                const double tv = V[root]; V[root] = V[ch]; V[ch] = tv;
                root = ch;
            }
        };
        for (int i = len / 2 - 1; i >= 0; --i) sift(i, len);
        for (int end = len - 1; end > 0; --end) {
            const int32_t tk = K[0]; K[0] = K[end]; K[end] = tk;
            const double tv = V[0]; V[0] = V[end]; V[end] = tv;
            sift(0, end);
        }
    }
}

// exclusive scan of int32 counts into off[0..n] in three passes (workgroup sums, one workgroup over the sums, workgroup scans)
__global__ __launch_bounds__(256) void tr_scan_sums_kernel(const int32_t* cnt, int64_t n, int32_t* bsum) {
    __shared__ int32_t red[256];
    const int64_t b0 = (int64_t)blockIdx.x * KR_TR_SCAN_CH + threadIdx.x * 8;
    int32_t s = 0;
    for (int q = 0; q < 8; ++q) if (b0 + q < n) s += cnt[b0 + q];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(1024) void tr_scan_top_kernel(int32_t* bsum, int64_t nb) {
    __shared__ int32_t part[1024];
    const int64_t per = (nb + 1023) / 1024;
    const int64_t lo0 = (int64_t)threadIdx.x * per, lo = lo0 < nb ? lo0 : nb, hi = lo + per < nb ? lo + per : nb;
    int32_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += bsum[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int i = 0; i < 1024; ++i) { const int32_t v = part[i]; part[i] = run; run += v; }
    }
    __syncthreads();
    int32_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { const int32_t v = bsum[i]; bsum[i] = run; run += v; }
}

__global__ __launch_bounds__(256) void tr_scan_apply_kernel(const int32_t* cnt, int64_t n, const int32_t* bofs, int32_t* off) {
    __shared__ int32_t part[256];
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * KR_TR_SCAN_CH + t * 8;
    int32_t v[8], s = 0;
    for (int q = 0; q < 8; ++q) { v[q] = (b0 + q < n) ? cnt[b0 + q] : 0; s += v[q]; }
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int32_t x = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int32_t run = bofs[blockIdx.x] + part[t] - s;
    for (int q = 0; q < 8; ++q) { run += v[q]; if (b0 + q < n) off[b0 + q + 1] = run; }
    if (blockIdx.x == 0 && t == 0) off[0] = 0;
}

void dev_csr_free(DevCsr& m) {
    (void)hipFree(m.ptr); (void)hipFree(m.idx); (void)hipFree(m.val);
    m = DevCsr{};
}

// rows (ptr, idx, val) of nin rows -> nout segments of (row, value) with rows ascending; DROP keeps only |v| > tol
int32_t csr_transpose(kryst_ctx_t ctx, const char* who, const int32_t* ptr, const int32_t* idx, const double* val, int64_t nin, int64_t nout,
                      bool drop, double tol, DevCsr& out) {
    hipStream_t s = ctx->s_main;
    const int64_t nb = std::max<int64_t>(1, (nout + KR_TR_SCAN_CH - 1) / KR_TR_SCAN_CH);
    int32_t* cnt = nullptr; int32_t* bsum = nullptr;
    int32_t rc = KRYST_OK;
    do {
        if (hipMalloc(&cnt, sizeof(int32_t) * (size_t)std::max<int64_t>(nout, 1)) != hipSuccess ||
            hipMalloc(&bsum, sizeof(int32_t) * (size_t)nb) != hipSuccess ||
            hipMalloc(&out.ptr, sizeof(int32_t) * (size_t)(nout + 1 + 8)) != hipSuccess) {
            set_error("%s: out of device memory (transpose of %lld rows)", who, (long long)nin); rc = KRYST_ERR_HIP; break;
        }
        if (hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(nout, 1), s) != hipSuccess ||
            hipMemsetAsync(out.ptr, 0, sizeof(int32_t) * (size_t)(nout + 1 + 8), s) != hipSuccess) { rc = KRYST_ERR_HIP; break; }
        const dim3 rg(tr_grid(nin, 256)), og(tr_grid(nout, 256)), blk(256);
        if (nin > 0) {
            if (drop) hipLaunchKernelGGL(tr_count_kernel<true>, rg, blk, 0, s, ptr, idx, val, nin, tol, cnt);
            else hipLaunchKernelGGL(tr_count_kernel<false>, rg, blk, 0, s, ptr, idx, val, nin, tol, cnt);
        }
        if (nout > 0) {
            hipLaunchKernelGGL(tr_scan_sums_kernel, dim3((unsigned)nb), blk, 0, s, (const int32_t*)cnt, nout, bsum);
            hipLaunchKernelGGL(tr_scan_top_kernel, dim3(1), dim3(1024), 0, s, bsum, nb);
            hipLaunchKernelGGL(tr_scan_apply_kernel, dim3((unsigned)nb), blk, 0, s, (const int32_t*)cnt, nout, (const int32_t*)bsum, out.ptr);
        }
        if (hipGetLastError() != hipSuccess) { set_error("%s: transpose launch failed", who); rc = KRYST_ERR_HIP; break; }
        int32_t total = 0;
        if (hipMemcpyAsync(&total, out.ptr + nout, sizeof total, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { set_error("%s: transpose failed on the device", who); rc = KRYST_ERR_HIP; break; }
        out.nnz = total;
        if (hipMalloc(&out.idx, sizeof(int32_t) * (size_t)(total + 8)) != hipSuccess ||
            hipMalloc(&out.val, sizeof(double) * (size_t)(total + 8)) != hipSuccess) {
            set_error("%s: out of device memory (%lld transposed entries)", who, (long long)total); rc = KRYST_ERR_HIP; break;
        }
        if (hipMemsetAsync(out.idx + total, 0, sizeof(int32_t) * 8, s) != hipSuccess ||
            hipMemsetAsync(out.val + total, 0, sizeof(double) * 8, s) != hipSuccess ||
            hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(nout, 1), s) != hipSuccess) { rc = KRYST_ERR_HIP; break; }
        if (nin > 0 && total > 0) {
            if (drop) hipLaunchKernelGGL(tr_fill_kernel<true>, rg, blk, 0, s, ptr, idx, val, nin, tol, (const int32_t*)out.ptr, cnt, out.idx, out.val);
            else hipLaunchKernelGGL(tr_fill_kernel<false>, rg, blk, 0, s, ptr, idx, val, nin, tol, (const int32_t*)out.ptr, cnt, out.idx, out.val);
            hipLaunchKernelGGL(tr_sort_kernel, og, blk, 0, s, (const int32_t*)out.ptr, nout, out.idx, out.val);
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { set_error("%s: transpose failed on the device", who); rc = KRYST_ERR_HIP; }
    } while (0);
    (void)hipFree(cnt); (void)hipFree(bsum);
    if (rc != KRYST_OK) dev_csr_free(out);
    return rc;
}

}  // namespace kr
