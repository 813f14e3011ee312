// Dense storage (DenseMatrix::from_raw, src/matrix/dense.rs:16-25; matvec, src/core/wrappers.rs:27-38) and the direct solvers (LuSolver,
// QrSolver, src/solver/direct_lu.rs) on the device.  Labelled deviation: the reference keeps faer's FullPivLu / Qr,
// whose summation order is not available; these are the textbook factorizations in the operation order section 4.12 fixes, which
// host_dense.cpp and tests/dense_ref.py restate bit for bit.
//
// LU: a step boundary is a kernel boundary.  Step s reads the trailing block from one buffer and writes the updated block to the other
// (16 B per element, like an in-place update), so nothing a launch reads is written by it: the row / column swap is an index map on the
// reads, the multiplier column and the pivot row come from the buffer no workgroup writes.  While a workgroup writes its tile it keeps the
// largest |value| (smaller row, then smaller column on a tie) and publishes it; every workgroup of the next launch reduces those
// candidates in its prologue.  L and U are stored by ORIGINAL row / column and put in place by one pass at the end, so finished parts are
// never swapped.  A trailing block of at most KR_DENSE_TAIL rows is finished by one workgroup inside LDS (same order per element).
// QR: W row-major, one thread per trailing column folding down it in ascending row order, one launch per step; the thread of column
// s + 1 also leaves that column and its sum of squares for the next step; the last KR_DENSE_TAIL steps run in one workgroup's LDS too.
#include "dense.h"
#include "csr.h"
#include "pc.h"
#include <algorithm>
#include <climits>
#include <cmath>

namespace kr {

struct Cand { double v; int32_t i, j; };          // |value| (-1: none) and its position

__device__ __forceinline__ void cand_merge(Cand& a, const Cand& b) {
    if (b.v > a.v || (b.v == a.v && (b.i < a.i || (b.i == a.i && b.j < a.j)))) a = b;
}

// the best candidate of the workgroup, valid in every thread; lds: one Cand per wave
__device__ __forceinline__ Cand block_best(Cand c, Cand* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    for (int off = 32; off >= 1; off >>= 1) {
        Cand o;
        o.v = __shfl_xor(c.v, off, 64); o.i = __shfl_xor(c.i, off, 64); o.j = __shfl_xor(c.j, off, 64);
        cand_merge(c, o);
    }
    if (lane == 0) lds[wave] = c;
    __syncthreads();
    Cand r = lds[0];
    for (int w = 1; w < nw; ++w) cand_merge(r, lds[w]);
    __syncthreads();
    return r;
}

// the pivot of a step from the reduced candidate: 0 or the failure code
__device__ __forceinline__ int pivot_code(const Cand& c, bool first_is_nan, double piv) {
    if (c.v < 0.0 || first_is_nan) return KR_DENSE_NONFINITE;      // the scan starts from a NaN, which nothing replaces
    if (piv == 0.0) return KR_DENSE_ZERO;
    return isfinite(piv) ? KR_DENSE_OK : KR_DENSE_NONFINITE;
}

__host__ __device__ inline int lu_tile_cols(int m) { return max(8, (m + 63) / 64); }     // <= 64 for m <= KRYST_DENSE_MAX

// ---------------------------------------------------------------- LU: the scan of A (non-finite entries, step 0's candidates, identity maps)
__global__ __launch_bounds__(KR_DENSE_TR) void lu_scan_kernel(const double* a, int n, int tc, Cand* cand_out, int* nan_out, int* rid, int* cid,
                                                              int* err) {
    __shared__ Cand red[KR_DENSE_TR / 64];
    const int i = blockIdx.x * KR_DENSE_TR + threadIdx.x;
    const int j0 = blockIdx.y * tc, jn = min(tc, n - j0);
    Cand best = {-1.0, INT_MAX, INT_MAX};
    bool bad = false;
    if (i < n) {
        for (int jj = 0; jj < jn; ++jj) {
            const double v = a[i + (int64_t)(j0 + jj) * n];
            bad |= !isfinite(v);
            const double av = fabs(v);
            if (av > best.v) { best.v = av; best.i = i; best.j = j0 + jj; }
        }
        if (blockIdx.y == 0) rid[i] = i;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < jn) cid[j0 + threadIdx.x] = j0 + threadIdx.x;
    if (bad) { err[1] = 0; err[0] = KR_DENSE_NONFINITE; }            // every writer stores the same two words
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nan_out = 0;
    best = block_best(best, red);
    if (threadIdx.x == 0) cand_out[blockIdx.y * gridDim.x + blockIdx.x] = best;
}

// ---------------------------------------------------------------- LU: step s
// positions: row / column s of src's frame receive the pivot row p / column q (index maps on the reads); the trailing block (s, n)^2 of
// dst is written in the swapped frame.  rid / cid: position -> original row / column, carried from buffer to buffer for the positions > s.
__global__ __launch_bounds__(KR_DENSE_TR) void lu_step_kernel(const double* src, double* dst, int n, int s, int tc, const Cand* cand_in,
                                                              int ncand, const int* nan_in, Cand* cand_out, int* nan_out, const int* rid_s,
                                                              const int* cid_s, int* rid_d, int* cid_d, int* rowperm, int* colperm, double* fl,
                                                              double* fu, int* err) {
    __shared__ Cand red[KR_DENSE_TR / 64];
    __shared__ double urow[64];
    __shared__ int failed;
    const int tid = threadIdx.x;
    // an earlier step failed?  err is also written by THIS launch (its first workgroup, when this step fails), so one thread reads it and the
    // whole workgroup takes the same branch: no wave may leave ahead of the barriers below
    if (tid == 0) failed = err[0];
    __syncthreads();
    if (failed) return;
    Cand c = {-1.0, INT_MAX, INT_MAX};
    for (int k = tid; k < ncand; k += KR_DENSE_TR) cand_merge(c, cand_in[k]);
    c = block_best(c, red);
    const double piv = (c.v >= 0.0) ? src[c.i + (int64_t)c.j * n] : 0.0;
    const int code = pivot_code(c, *nan_in != 0, piv);
    const bool first = blockIdx.x == 0 && blockIdx.y == 0;
    if (code) {                                                     // every workgroup sees it; the first one reports it
        if (first && tid == 0) { err[1] = s; err[0] = code; }
        return;
    }
    const int p = c.i, q = c.j;
    const int i = s + 1 + blockIdx.x * KR_DENSE_TR + tid;
    const int j0 = s + 1 + blockIdx.y * tc, jn = min(tc, n - j0);
    if (tid < jn) {                                                 // the pivot row's segment of this tile
        const int j = j0 + tid, jp = (j == q) ? s : j;
        const double u = src[p + (int64_t)jp * n];
        urow[tid] = u;
        if (blockIdx.x == 0) { fu[(int64_t)s * n + cid_s[jp]] = u; cid_d[j] = cid_s[jp]; }
    }
    if (first && tid == 0) { fu[(int64_t)s * n + cid_s[q]] = piv; rowperm[s] = rid_s[p]; colperm[s] = cid_s[q]; }
    __syncthreads();
    Cand best = {-1.0, INT_MAX, INT_MAX};
    if (i < n && jn > 0) {
        const int ip = (i == p) ? s : i;
        const double l = src[ip + (int64_t)q * n] / piv;
        if (blockIdx.y == 0) { const int r = rid_s[ip]; fl[r + (int64_t)s * n] = l; rid_d[i] = r; }
        for (int jj = 0; jj < jn; ++jj) {
            const int j = j0 + jj, jp = (j == q) ? s : j;
            const double v = src[ip + (int64_t)jp * n] - l * urow[jj];
            dst[i + (int64_t)j * n] = v;
            const double av = fabs(v);
            if (av > best.v) { best.v = av; best.i = i; best.j = j; }
            if (first && tid == 0 && jj == 0) *nan_out = isnan(v) ? 1 : 0;     // the next scan's first entry
        }
    }
    best = block_best(best, red);
    if (tid == 0) cand_out[blockIdx.y * gridDim.x + blockIdx.x] = best;
}

// ---------------------------------------------------------------- LU: the last m0 = n - s0 steps by one workgroup inside LDS
__host__ __device__ inline int tail_ld(int m0) { return m0 | 1; }   // odd: a row's entries start in different banks
inline size_t tail_lds_bytes(int m0) { return sizeof(double) * (size_t)tail_ld(m0) * m0 + sizeof(int) * 2 * KR_DENSE_TAIL + sizeof(Cand) * 16; }

__global__ __launch_bounds__(1024) void lu_tail_kernel(const double* src, int n, int s0, const int* rid_s, const int* cid_s, int* rowperm,
                                                       int* colperm, double* fl, double* fu, int* err) {
    extern __shared__ double tail_lds[];
    __shared__ int failed;
    if (threadIdx.x == 0) failed = err[0];                          // one read, one branch for the whole workgroup
    __syncthreads();
    if (failed) return;
    const int m0 = n - s0, ld = tail_ld(m0);
    double* T = tail_lds;
    int* lr = reinterpret_cast<int*>(T + (size_t)ld * m0);
    int* lc = lr + KR_DENSE_TAIL;
    Cand* red = reinterpret_cast<Cand*>(lc + KR_DENSE_TAIL);
    const int tid = threadIdx.x, tx = tid & (KR_DENSE_TAIL - 1), ty = tid >> 7;      // 8 columns at a time, one row per thread
    constexpr int NY = 1024 / KR_DENSE_TAIL;
    if (tx < m0)
        for (int j = ty; j < m0; j += NY) T[tx + j * ld] = src[(s0 + tx) + (int64_t)(s0 + j) * n];
    if (tid < m0) { lr[tid] = rid_s[s0 + tid]; lc[tid] = cid_s[s0 + tid]; }
    __syncthreads();
    for (int k = 0; k < m0; ++k) {
        Cand best = {-1.0, INT_MAX, INT_MAX};
        const int i = k + tx;
        if (i < m0)
            for (int j = k + ty; j < m0; j += NY) {
                const double av = fabs(T[i + j * ld]);
                if (av > best.v) { best.v = av; best.i = i; best.j = j; }
            }
        const Cand c = block_best(best, red);
        const double pv = (c.v >= 0.0) ? T[c.i + c.j * ld] : 0.0;
        const int code = pivot_code(c, isnan(T[k + k * ld]), pv);
        if (code) {                                                  // uniform over the workgroup
            if (tid == 0) { err[1] = s0 + k; err[0] = code; }
            return;
        }
        const int p = c.i, q = c.j;
        __syncthreads();                                             // every thread has read the pivot and T[k][k] before the swaps overwrite them
        if (p != k) {
            if (tid < m0) { const double t = T[k + tid * ld]; T[k + tid * ld] = T[p + tid * ld]; T[p + tid * ld] = t; }
            if (tid == 0) { const int t = lr[k]; lr[k] = lr[p]; lr[p] = t; }
        }
        __syncthreads();
        if (q != k) {
            if (tid < m0) { const double t = T[tid + k * ld]; T[tid + k * ld] = T[tid + q * ld]; T[tid + q * ld] = t; }
            if (tid == 0) { const int t = lc[k]; lc[k] = lc[q]; lc[q] = t; }
        }
        __syncthreads();
        const double piv = T[k + k * ld];
        if (tid > k && tid < m0) T[tid + k * ld] = T[tid + k * ld] / piv;
        __syncthreads();
        const int iu = k + 1 + tx;
        if (iu < m0) {
            const double l = T[iu + k * ld];
            for (int j = k + 1 + ty; j < m0; j += NY) T[iu + j * ld] = T[iu + j * ld] - l * T[k + j * ld];
        }
        __syncthreads();
    }
    if (tx < m0)
        for (int j = ty; j < m0; j += NY) {
            const double v = T[tx + j * ld];
            if (tx > j) fl[lr[tx] + (int64_t)(s0 + j) * n] = v;
            else fu[(int64_t)(s0 + tx) * n + lc[j]] = v;
        }
    if (tid < m0) { rowperm[s0 + tid] = lr[tid]; colperm[s0 + tid] = lc[tid]; }
}

// factors[i][j] = L[i][j] below the diagonal, U[i][j] on and above it, in the final (permuted) frame, column-major
__global__ __launch_bounds__(256) void lu_assemble_kernel(const double* fl, const double* fu, const int* rowperm, const int* colperm, int n,
                                                          double* f, const int* err) {
    if (err[0]) return;
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < n) f[i + (int64_t)j * n] = (i > j) ? fl[rowperm[i] + (int64_t)j * n] : fu[(int64_t)i * n + colperm[j]];
}

// ---------------------------------------------------------------- triangular column sweeps by one workgroup (n <= KRYST_DENSE_MAX)
// y_i = b[rowperm[i]]; FWD: for j ascending, y_i -= L[i][j] y_j (i > j); then for j descending, y_j /= U[j][j], y_i -= U[i][j] y_j (i < j);
// x[colperm[j]] = y_j.  A barrier per column; the column after the current one is loaded ahead of the barrier.  b and x may coincide:
// b is read completely (into LDS) before x is written.
template <bool FWD>
__global__ __launch_bounds__(KR_DENSE_SWEEP_T) void dense_sweep_kernel(const double* f, int n, const int* rowperm, const int* colperm,
                                                                      const double* b, double* x) {
    __shared__ double y[KRYST_DENSE_MAX];
    constexpr int R = KRYST_DENSE_MAX / KR_DENSE_SWEEP_T;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += KR_DENSE_SWEEP_T) y[i] = b[rowperm ? rowperm[i] : i];
    __syncthreads();
    double cur[R], nxt[R];
    if (FWD) {
#pragma unroll
        for (int r = 0; r < R; ++r) { const int i = tid + r * KR_DENSE_SWEEP_T; nxt[r] = (i > 0 && i < n) ? f[i] : 0.0; }
        for (int j = 0; j < n; ++j) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = tid + r * KR_DENSE_SWEEP_T;
                cur[r] = nxt[r];
                nxt[r] = (j + 1 < n && i > j + 1 && i < n) ? f[i + (int64_t)(j + 1) * n] : 0.0;
            }
            const double yj = y[j];
#pragma unroll
            for (int r = 0; r < R; ++r) { const int i = tid + r * KR_DENSE_SWEEP_T; if (i > j && i < n) y[i] = y[i] - cur[r] * yj; }
            __syncthreads();
        }
    }
    double dcur, dnxt = (n > 0) ? f[(int64_t)(n - 1) * n + (n - 1)] : 1.0;
#pragma unroll
    for (int r = 0; r < R; ++r) { const int i = tid + r * KR_DENSE_SWEEP_T; nxt[r] = (n > 0 && i < n - 1) ? f[i + (int64_t)(n - 1) * n] : 0.0; }
    for (int j = n - 1; j >= 0; --j) {
        dcur = dnxt;
        if (j > 0) dnxt = f[(int64_t)(j - 1) * n + (j - 1)];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * KR_DENSE_SWEEP_T;
            cur[r] = nxt[r];
            nxt[r] = (j > 0 && i < j - 1) ? f[i + (int64_t)(j - 1) * n] : 0.0;
        }
        const double yj = y[j] / dcur;                               // the same quotient in every thread
        if (tid == 0) x[colperm ? colperm[j] : j] = yj;
#pragma unroll
        for (int r = 0; r < R; ++r) { const int i = tid + r * KR_DENSE_SWEEP_T; if (i < j) y[i] = y[i] - cur[r] * yj; }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- QR
// W row-major from the column-major A, c = b, column 0 and its sum of squares for step 0; a non-finite entry of A is an error
__global__ __launch_bounds__(256) void qr_init_kernel(const double* a, const double* b, int n, double* w, double* c, double* v0, double* ss0,
                                                      int* err) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < n) {
        const double v = a[i + (int64_t)j * n];
        if (!isfinite(v)) { err[1] = 0; err[0] = KR_DENSE_NONFINITE; }
        w[(int64_t)i * n + j] = v;
        if (j == 0) { v0[i] = v; c[i] = b[i]; }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        double ss = 0.0;
        for (int r = 0; r < n; ++r) ss = ss + a[r] * a[r];
        *ss0 = ss;
    }
}

// step s: thread <-> column j in (s, n] (n: the right-hand side); v_in / ss_in: column s and its sum of squares, left by step s - 1
__global__ __launch_bounds__(256) void qr_step_kernel(double* w, double* c, int n, int s, const double* v_in, const double* ss_in, double* v_out,
                                                      double* ss_out, double* rdiag, int* err) {
    __shared__ double vl[KRYST_DENSE_MAX];
    __shared__ double sc[2];
    __shared__ int scode, failed;
    const int tid = threadIdx.x, len = n - s;
    if (tid == 0) failed = err[0];                                  // written by this launch's first workgroup too: one read, one branch per workgroup
    __syncthreads();
    if (failed) return;
    for (int k = tid; k < len; k += 256) vl[k] = v_in[s + k];
    __syncthreads();
    if (tid == 0) {
        int code = 0;
        double alpha = 0.0, vv = 0.0;
        const double nrm = sqrt(*ss_in);
        if (nrm == 0.0) code = KR_DENSE_ZERO;
        else {
            alpha = (vl[0] >= 0.0) ? -nrm : nrm;
            vl[0] = vl[0] - alpha;
            for (int k = 0; k < len; ++k) vv = vv + vl[k] * vl[k];
            if (vv == 0.0) code = KR_DENSE_ZERO;
        }
        sc[0] = alpha; sc[1] = vv; scode = code;
    }
    __syncthreads();
    if (scode) {
        if (blockIdx.x == 0 && tid == 0) { err[1] = s; err[0] = scode; }
        return;
    }
    const double vv = sc[1];
    if (blockIdx.x == 0 && tid == 0) rdiag[s] = sc[0];
    const int j = s + 1 + blockIdx.x * 256 + tid;
    if (j > n) return;
    double* col = (j < n) ? w + j : c;                               // element i of the column: col[i * stride]
    const int64_t stride = (j < n) ? n : 1;
    double t = 0.0;
    for (int k = 0; k < len; ++k) t = t + vl[k] * col[(int64_t)(s + k) * stride];
    t = (2.0 * t) / vv;
    const bool owner = j == s + 1 && j < n;                         // leaves column s + 1 for the next step
    double ssn = 0.0;
    for (int k = 0; k < len; ++k) {
        const double x = col[(int64_t)(s + k) * stride] - vl[k] * t;
        col[(int64_t)(s + k) * stride] = x;
        if (owner && k >= 1) { v_out[s + k] = x; ssn = ssn + x * x; }
    }
    if (owner) *ss_out = ssn;
}

// the last m0 = n - s0 steps by one workgroup inside LDS: the trailing block and c's tail, row-major with c as column m0; thread <-> column
// as in qr_step_kernel, the folds in the same ascending order, so the bits are the same.  (The rows above s0 of these columns are R already.)
__host__ __device__ inline int qr_tail_ld(int m0) { return m0 + 1; }
inline size_t qr_tail_lds_bytes(int m0) { return sizeof(double) * ((size_t)qr_tail_ld(m0) * m0 + KR_DENSE_TAIL); }

__global__ __launch_bounds__(256) void qr_tail_kernel(double* w, double* c, int n, int s0, double* rdiag, int* err) {
    extern __shared__ double qr_lds[];
    __shared__ double sc[2];
    __shared__ int scode, failed;
    const int tid = threadIdx.x;
    if (tid == 0) failed = err[0];
    __syncthreads();
    if (failed) return;
    const int m0 = n - s0, ld = qr_tail_ld(m0);
    double* T = qr_lds;
    double* vl = T + (size_t)ld * m0;
    for (int e = tid; e < m0 * ld; e += 256) {
        const int i = e / ld, j = e - i * ld;
        T[e] = (j < m0) ? w[(int64_t)(s0 + i) * n + s0 + j] : c[s0 + i];
    }
    __syncthreads();
    for (int k = 0; k < m0; ++k) {
        if (tid >= k && tid < m0) vl[tid] = T[tid * ld + k];
        __syncthreads();
        if (tid == 0) {
            int code = 0;
            double alpha = 0.0, vv = 0.0, ss = 0.0;
            for (int i = k; i < m0; ++i) ss = ss + vl[i] * vl[i];
            const double nrm = sqrt(ss);
            if (nrm == 0.0) code = KR_DENSE_ZERO;
            else {
                alpha = (vl[k] >= 0.0) ? -nrm : nrm;
                vl[k] = vl[k] - alpha;
                for (int i = k; i < m0; ++i) vv = vv + vl[i] * vl[i];
                if (vv == 0.0) code = KR_DENSE_ZERO;
            }
            sc[0] = alpha; sc[1] = vv; scode = code;
        }
        __syncthreads();
        if (scode) {                                                 // uniform: read from LDS behind a barrier
            if (tid == 0) { err[1] = s0 + k; err[0] = scode; }
            return;
        }
        const double vv = sc[1];
        if (tid == 0) rdiag[s0 + k] = sc[0];
        const int j = k + 1 + tid;                                   // j == m0: the right-hand side
        if (j <= m0) {
            double t = 0.0;
            for (int i = k; i < m0; ++i) t = t + vl[i] * T[i * ld + j];
            t = (2.0 * t) / vv;
            for (int i = k; i < m0; ++i) T[i * ld + j] = T[i * ld + j] - vl[i] * t;
        }
        __syncthreads();
    }
    for (int e = tid; e < m0 * ld; e += 256) {
        const int i = e / ld, j = e - i * ld;
        if (j == m0) c[s0 + i] = T[e];
        else if (j > i) w[(int64_t)(s0 + i) * n + s0 + j] = T[e];
    }
}

// R (row-major upper triangle of w, diagonal in rdiag) as a column-major factor for the backward sweep
__global__ __launch_bounds__(256) void qr_r_kernel(const double* w, const double* rdiag, int n, double* f, const int* err) {
    if (err[0]) return;
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i < n) f[i + (int64_t)j * n] = (i < j) ? w[(int64_t)i * n + j] : (i == j ? rdiag[i] : 0.0);
}

// ---------------------------------------------------------------- storage kernels
__global__ __launch_bounds__(256) void dense_matvec_kernel(const double* a, int64_t nrows, int64_t ncols, const double* x, double* y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    double s = 0.0;
    for (int64_t j = 0; j < ncols; ++j) s = s + a[i + j * nrows] * x[j];
    y[i] = s;
}

__global__ __launch_bounds__(256) void dense_from_csr_kernel(const int32_t* row_ptr, const int32_t* col, const double* val, int64_t nrows,
                                                             int64_t ncols, double* d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    for (int32_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
        if (col[e] >= 0 && col[e] < ncols) d[i + (int64_t)col[e] * nrows] = val[e];
}

// ---------------------------------------------------------------- host side
struct DevBuf {                                                     // device scratch of one call
    void* p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 8)); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

static int tail_rows() { return std::min(std::max(env_int("KRYST_DENSE_TAIL", KR_DENSE_TAIL), 0), KR_DENSE_TAIL); }

static int32_t dense_check_square(kryst_dense_t a, const char* who) {
    if (a->ctx->nranks > 1) { set_error("%s: distributed contexts are not supported", who); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->ncols, "dense direct solver: square matrix required");
    if (a->nrows > KRYST_DENSE_MAX) {
        set_error("%s: %lld rows; at most %d are supported", who, (long long)a->nrows, (int)KRYST_DENSE_MAX);
        return KRYST_UNSUPPORTED;
    }
    return KRYST_OK;
}

// reads the error word (synchronises the compute stream) and turns it into a status
static int32_t dense_status(kryst_ctx_t ctx, const int* d_err, const char* who) {
    int e[2] = {0, 0};
    KR_HIP(hipMemcpyAsync(e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    if (e[0] == KR_DENSE_OK) return KRYST_OK;
    if (e[0] == KR_DENSE_ZERO) {
        set_error("%s: zero pivot at step %d", who, e[1]); set_error_row(e[1]);
        return KRYST_ZERO_PIVOT;
    }
    set_error("%s: NaN or Inf in the matrix or in the pivot of step %d", who, e[1]);
    return KRYST_FACTOR_ERROR;
}

static bool overlap(const double* p, int64_t np, const double* q, int64_t nq) { return p < q + nq && q < p + np; }

// b and x the same vector is allowed; any other overlap is refused
static int32_t dense_check_vecs(kryst_dense_t a, kryst_vec_t b, kryst_vec_t x) {
    KR_ARG(b && x && b->ctx == a->ctx && x->ctx == a->ctx, "dense solve: vectors of another context");
    KR_ARG(b->n == a->nrows && x->n == a->nrows, "dense solve: vector length");
    KR_ARG(b->d == x->d || !overlap(b->d, b->n, x->d, x->n), "dense solve: b and x overlap without being the same vector");
    KR_ARG(!overlap(a->d, a->nrows * a->ncols, b->d, b->n) && !overlap(a->d, a->nrows * a->ncols, x->d, x->n),
           "dense solve: a vector overlaps the matrix");
    return KRYST_OK;
}

// the preconditioner is accepted and ignored (direct_lu.rs:70, :123), but a handle of another context is still an argument error
static int32_t dense_check_pc(kryst_dense_t a, kryst_pc_t pc) {
    KR_ARG(!pc || pc->ctx == a->ctx, "dense solve: preconditioner belongs to another context");
    return KRYST_OK;
}

static void direct_stats(kryst_stats_t* stats) {                    // direct_lu.rs:84-88
    if (stats) { stats->iterations = 1; stats->final_residual = 0.0; stats->converged = 1; }
}

}  // namespace kr

using namespace kr;

struct kryst_lu_s {
    kryst_ctx_t ctx = nullptr;
    int64_t n = -1;                  // -1: no factorization is cached
    double* d_f = nullptr;           // L below the diagonal (unit diagonal implied), U on and above, column-major, permuted frame
    int32_t* d_rp = nullptr; int32_t* d_cp = nullptr;
    void drop() { (void)hipFree(d_f); (void)hipFree(d_rp); (void)hipFree(d_cp); d_f = nullptr; d_rp = d_cp = nullptr; n = -1; }
};

static int32_t lu_factor(kryst_lu_t lu, kryst_dense_t a) {
    kryst_ctx_t ctx = lu->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    lu->drop();
    const int n = (int)a->nrows;
    const size_t nn = (size_t)n * n;
    const int tail = tail_rows();
    DevBuf w0, w1, fl, fu, cand, ints;
    const bool stepped = n > tail;                                   // some steps run as launches of their own
    const int maxcand = 2048;
    if (fl.alloc(sizeof(double) * nn) != hipSuccess || fu.alloc(sizeof(double) * nn) != hipSuccess ||
        (stepped && (w0.alloc(sizeof(double) * nn) != hipSuccess || w1.alloc(sizeof(double) * nn) != hipSuccess)) ||
        cand.alloc(sizeof(Cand) * 2 * maxcand) != hipSuccess || ints.alloc(sizeof(int) * (4 * (size_t)n + 8)) != hipSuccess ||
        hipMalloc(&lu->d_f, sizeof(double) * std::max<size_t>(nn, 1)) != hipSuccess ||
        hipMalloc(&lu->d_rp, sizeof(int32_t) * std::max(n, 1)) != hipSuccess || hipMalloc(&lu->d_cp, sizeof(int32_t) * std::max(n, 1)) != hipSuccess) {
        (void)hipGetLastError();
        lu->drop();
        set_error("dense LU: out of device memory for %d rows", n);
        return KRYST_ERR_HIP;
    }
    int* d_err = ints.as<int>();                                     // [0] code, [1] step, [2], [3] first-entry-is-NaN of the two buffers
    int* d_nan[2] = {d_err + 2, d_err + 3};
    int* d_rid[2] = {d_err + 8, d_err + 8 + n};
    int* d_cid[2] = {d_err + 8 + 2 * n, d_err + 8 + 3 * n};
    Cand* d_cand[2] = {cand.as<Cand>(), cand.as<Cand>() + maxcand};
    double* wb[2] = {w0.as<double>(), w1.as<double>()};
    hipStream_t st = ctx->s_main;
    int32_t rc = KRYST_OK;
    auto fail = [&](int32_t code) { lu->drop(); return code; };
    if (hipMemsetAsync(d_err, 0, sizeof(int) * 8, st) != hipSuccess) return fail(KRYST_ERR_HIP);
    if (n > 0) {
        {   // the scan publishes into the buffers step 0 reads: parity 1
            const int tc = lu_tile_cols(n);
            const dim3 grid((n + KR_DENSE_TR - 1) / KR_DENSE_TR, (n + tc - 1) / tc);
            hipLaunchKernelGGL(lu_scan_kernel, grid, dim3(KR_DENSE_TR), 0, st, (const double*)a->d, n, tc, d_cand[1], d_nan[1], d_rid[1], d_cid[1], d_err);
        }
        int ncand = ((n + KR_DENSE_TR - 1) / KR_DENSE_TR) * ((n + lu_tile_cols(n) - 1) / lu_tile_cols(n));
        int s = 0;
        for (; n - s > tail; ++s) {
            const int m = n - s - 1, tc = lu_tile_cols(m);
            const dim3 grid(std::max(1, (m + KR_DENSE_TR - 1) / KR_DENSE_TR), std::max(1, (m + tc - 1) / tc));
            const int in = (s + 1) & 1, out = s & 1;
            hipLaunchKernelGGL(lu_step_kernel, grid, dim3(KR_DENSE_TR), 0, st, s == 0 ? (const double*)a->d : (const double*)wb[in], wb[out], n, s, tc,
                               (const Cand*)d_cand[in], ncand, (const int*)d_nan[in], d_cand[out], d_nan[out], (const int*)d_rid[in],
                               (const int*)d_cid[in], d_rid[out], d_cid[out], lu->d_rp, lu->d_cp, fl.as<double>(), fu.as<double>(), d_err);
            ncand = (int)(grid.x * grid.y);
        }
        if (s < n) {
            const int in = (s + 1) & 1;
            const size_t lds = tail_lds_bytes(n - s);
            if (hipFuncSetAttribute((const void*)lu_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                set_error("dense LU: %zu bytes of LDS for the tail are not available", lds);
                return fail(KRYST_ERR_HIP);
            }
            hipLaunchKernelGGL(lu_tail_kernel, dim3(1), dim3(1024), lds, st, s == 0 ? (const double*)a->d : (const double*)wb[in], n, s,
                               (const int*)d_rid[in], (const int*)d_cid[in], lu->d_rp, lu->d_cp, fl.as<double>(), fu.as<double>(), d_err);
        }
        hipLaunchKernelGGL(lu_assemble_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, (const double*)fl.as<double>(), (const double*)fu.as<double>(),
                           (const int*)lu->d_rp, (const int*)lu->d_cp, n, lu->d_f, (const int*)d_err);
        if (hipGetLastError() != hipSuccess) { set_error("dense LU: a launch failed"); return fail(KRYST_ERR_HIP); }
    }
    rc = dense_status(ctx, d_err, "dense LU");                       // the one synchronisation of the factorization
    if (rc != KRYST_OK) return fail(rc);
    lu->n = n;
    return KRYST_OK;
}

static int32_t lu_sweeps(kryst_lu_t lu, const double* b, double* x) {
    if (lu->n == 0) return KRYST_OK;
    hipLaunchKernelGGL(dense_sweep_kernel<true>, dim3(1), dim3(KR_DENSE_SWEEP_T), 0, lu->ctx->s_main, (const double*)lu->d_f, (int)lu->n,
                       (const int*)lu->d_rp, (const int*)lu->d_cp, b, x);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// QR solve of a x = b into x (device pointers; b and x may coincide: x is written by the last kernel only, and only without an error)
static int32_t qr_run(kryst_dense_t a, const double* b, double* x) {
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    const int n = (int)a->nrows;
    if (n == 0) return KRYST_OK;
    const size_t nn = (size_t)n * n;
    DevBuf w, f, small;
    if (w.alloc(sizeof(double) * nn) != hipSuccess || f.alloc(sizeof(double) * nn) != hipSuccess ||
        small.alloc(sizeof(double) * (4 * (size_t)n + 4) + sizeof(int) * 8) != hipSuccess) {
        (void)hipGetLastError();
        set_error("dense QR: out of device memory for %d rows", n);
        return KRYST_ERR_HIP;
    }
    double* c = small.as<double>();
    double* rdiag = c + n;
    double* v[2] = {rdiag + n, rdiag + 2 * n};
    double* ss = rdiag + 3 * n;                                      // 2 entries
    int* d_err = reinterpret_cast<int*>(ss + 4);
    hipStream_t st = ctx->s_main;
    KR_HIP(hipMemsetAsync(d_err, 0, sizeof(int) * 8, st));
    hipLaunchKernelGGL(qr_init_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, (const double*)a->d, b, n, w.as<double>(), c, v[0], ss, d_err);
    const int tail = tail_rows();
    int s = 0;
    for (; n - s > tail; ++s)
        hipLaunchKernelGGL(qr_step_kernel, dim3((n - s + 255) / 256), dim3(256), 0, st, w.as<double>(), c, n, s, (const double*)v[s & 1],
                           (const double*)(ss + (s & 1)), v[(s + 1) & 1], ss + ((s + 1) & 1), rdiag, d_err);
    if (s < n) {
        const size_t lds = qr_tail_lds_bytes(n - s);
        if (hipFuncSetAttribute((const void*)qr_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            set_error("dense QR: %zu bytes of LDS for the tail are not available", lds);
            return KRYST_ERR_HIP;
        }
        hipLaunchKernelGGL(qr_tail_kernel, dim3(1), dim3(256), lds, st, w.as<double>(), c, n, s, rdiag, d_err);
    }
    hipLaunchKernelGGL(qr_r_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, (const double*)w.as<double>(), (const double*)rdiag, n, f.as<double>(),
                       (const int*)d_err);
    KR_HIP(hipGetLastError());
    KR_TRY(dense_status(ctx, d_err, "dense QR"));
    hipLaunchKernelGGL(dense_sweep_kernel<false>, dim3(1), dim3(KR_DENSE_SWEEP_T), 0, st, (const double*)f.as<double>(), n, (const int*)nullptr,
                       (const int*)nullptr, (const double*)c, x);
    KR_HIP(hipGetLastError());
    KR_HIP(hipStreamSynchronize(st));                                // the scratch goes with this call
    return KRYST_OK;
}

// host b / x around a device solve: x_host is written only on success
template <class Solve> static int32_t with_host_vectors(kryst_ctx_t ctx, const double* b_host, double* x_host, int64_t n, Solve solve) {
    KR_HIP(hipSetDevice(ctx->device));
    DevBuf bx;
    if (bx.alloc(sizeof(double) * (size_t)std::max<int64_t>(n, 1)) != hipSuccess) {
        (void)hipGetLastError(); set_error("dense solve: out of device memory for the right-hand side"); return KRYST_ERR_HIP;
    }
    if (n > 0) KR_HIP(hipMemcpyAsync(bx.p, b_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->s_main));
    KR_TRY(solve(bx.as<double>()));
    if (n > 0) KR_HIP(hipMemcpyAsync(x_host, bx.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    return KRYST_OK;
}

extern "C" {

int32_t kryst_dense_create(kryst_ctx_t ctx, int64_t nrows, int64_t ncols, const double* data, int32_t colmajor, kryst_dense_t* out) {
    KR_ARG(ctx && out && nrows >= 0 && ncols >= 0 && (data || nrows * ncols == 0), "dense_create");
    if (ctx->nranks > 1) { set_error("dense_create: distributed contexts are not supported"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(ctx->device));
    const size_t count = (size_t)nrows * (size_t)ncols;
    kryst_dense_s* a = new kryst_dense_s;
    a->ctx = ctx; a->nrows = nrows; a->ncols = ncols;
    if (hipMalloc(&a->d, sizeof(double) * std::max<size_t>(count, 1)) != hipSuccess) {
        (void)hipGetLastError(); delete a;
        set_error("dense_create: out of device memory for %lld x %lld entries", (long long)nrows, (long long)ncols);
        return KRYST_ERR_HIP;
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        if (colmajor) e = hipMemcpy(a->d, data, sizeof(double) * count, hipMemcpyHostToDevice);
        else {
            std::vector<double> t(count);
            for (int64_t i = 0; i < nrows; ++i)
                for (int64_t j = 0; j < ncols; ++j) t[(size_t)(i + j * nrows)] = data[i * ncols + j];
            e = hipMemcpy(a->d, t.data(), sizeof(double) * count, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) { (void)hipFree(a->d); delete a; set_error("dense_create: upload failed: %s", hipGetErrorString(e)); return KRYST_ERR_HIP; }
    *out = a;
    return KRYST_OK;
}

int32_t kryst_dense_from_csr(kryst_csr_t m, kryst_dense_t* out) {
    KR_ARG(m && out, "dense_from_csr");
    if (m->dist || m->ctx->nranks > 1) { set_error("dense_from_csr: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(m->ctx->device));
    const size_t count = (size_t)m->nrows * (size_t)m->ncols;
    kryst_dense_s* a = new kryst_dense_s;
    a->ctx = m->ctx; a->nrows = m->nrows; a->ncols = m->ncols;
    if (hipMalloc(&a->d, sizeof(double) * std::max<size_t>(count, 1)) != hipSuccess) {
        (void)hipGetLastError(); delete a;
        set_error("dense_from_csr: out of device memory for %lld x %lld entries", (long long)m->nrows, (long long)m->ncols);
        return KRYST_ERR_HIP;
    }
    hipError_t e = hipMemsetAsync(a->d, 0, sizeof(double) * std::max<size_t>(count, 1), m->ctx->s_main);
    if (e == hipSuccess && count > 0) {
        hipLaunchKernelGGL(dense_from_csr_kernel, dim3((unsigned)((m->nrows + 255) / 256)), dim3(256), 0, m->ctx->s_main, (const int32_t*)m->d_row_ptr,
                           (const int32_t*)m->d_col, (const double*)m->d_val, m->nrows, m->ncols, a->d);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { (void)hipFree(a->d); delete a; set_error("dense_from_csr failed: %s", hipGetErrorString(e)); return KRYST_ERR_HIP; }
    *out = a;
    return KRYST_OK;
}

int32_t kryst_dense_shape(kryst_dense_t a, int64_t* nrows, int64_t* ncols) {
    KR_ARG(a, "dense_shape");
    if (nrows) *nrows = a->nrows;
    if (ncols) *ncols = a->ncols;
    return KRYST_OK;
}

int32_t kryst_dense_download(kryst_dense_t a, double* colmajor) {
    KR_ARG(a && (colmajor || a->nrows * a->ncols == 0), "dense_download");
    KR_HIP(hipSetDevice(a->ctx->device));
    if (a->nrows * a->ncols > 0)
        KR_HIP(hipMemcpyAsync(colmajor, a->d, sizeof(double) * (size_t)(a->nrows * a->ncols), hipMemcpyDeviceToHost, a->ctx->s_main));
    KR_HIP(hipStreamSynchronize(a->ctx->s_main));
    return KRYST_OK;
}

int32_t kryst_dense_destroy(kryst_dense_t a) {
    if (!a) return KRYST_OK;
    (void)hipSetDevice(a->ctx->device);
    (void)hipFree(a->d);
    delete a;
    return KRYST_OK;
}

int32_t kryst_dense_matvec(kryst_dense_t a, kryst_vec_t x, kryst_vec_t y) {
    KR_ARG(a && x && y && x->ctx == a->ctx && y->ctx == a->ctx, "dense_matvec");
    KR_ARG(x->n == a->ncols && y->n == a->nrows, "dense_matvec: vector length");
    KR_ARG(x != y && !overlap(x->d, x->n, y->d, y->n), "dense_matvec: x and y share storage");
    KR_HIP(hipSetDevice(a->ctx->device));
    if (a->nrows == 0) return KRYST_OK;
    hipLaunchKernelGGL(dense_matvec_kernel, dim3((unsigned)((a->nrows + 255) / 256)), dim3(256), 0, a->ctx->s_main, (const double*)a->d, a->nrows,
                       a->ncols, (const double*)x->d, y->d);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

int32_t kryst_lu_create(kryst_ctx_t ctx, kryst_lu_t* out) {
    KR_ARG(ctx && out, "lu_create");
    if (ctx->nranks > 1) { set_error("lu_create: distributed contexts are not supported"); return KRYST_UNSUPPORTED; }
    kryst_lu_s* lu = new kryst_lu_s;
    lu->ctx = ctx;
    *out = lu;
    return KRYST_OK;
}

int32_t kryst_lu_destroy(kryst_lu_t lu) {
    if (!lu) return KRYST_OK;
    (void)hipSetDevice(lu->ctx->device);
    lu->drop();
    delete lu;
    return KRYST_OK;
}

int32_t kryst_lu_solve_dev(kryst_lu_t lu, kryst_dense_t a, kryst_pc_t pc, kryst_vec_t b, kryst_vec_t x, kryst_stats_t* stats) {
    KR_ARG(lu && a && a->ctx == lu->ctx, "lu_solve_dev");
    KR_TRY(dense_check_pc(a, pc));
    KR_TRY(dense_check_square(a, "dense LU"));
    KR_TRY(dense_check_vecs(a, b, x));
    KR_TRY(lu_factor(lu, a));
    KR_TRY(lu_sweeps(lu, b->d, x->d));
    direct_stats(stats);
    return KRYST_OK;
}

int32_t kryst_lu_solve(kryst_lu_t lu, kryst_dense_t a, kryst_pc_t pc, const double* b, double* x, int64_t n, kryst_stats_t* stats) {
    KR_ARG(lu && a && a->ctx == lu->ctx && ((b && x) || n == 0), "lu_solve");
    KR_TRY(dense_check_pc(a, pc));
    KR_TRY(dense_check_square(a, "dense LU"));
    KR_ARG(n == a->nrows, "lu_solve: vector length");
    KR_TRY(with_host_vectors(lu->ctx, b, x, n, [&](double* d) -> int32_t {
        KR_TRY(lu_factor(lu, a));
        return lu_sweeps(lu, d, d);
    }));
    direct_stats(stats);
    return KRYST_OK;
}

int32_t kryst_lu_solve_cached(kryst_lu_t lu, kryst_vec_t b, kryst_vec_t x) {
    KR_ARG(lu && b && x && b->ctx == lu->ctx && x->ctx == lu->ctx, "lu_solve_cached");
    if (lu->n < 0) { set_error("lu_solve_cached: no factorization is cached"); return KRYST_SOLVE_ERROR; }
    KR_ARG(b->n == lu->n && x->n == lu->n, "lu_solve_cached: vector length");
    KR_ARG(b->d == x->d || !overlap(b->d, b->n, x->d, x->n), "lu_solve_cached: b and x overlap without being the same vector");
    KR_HIP(hipSetDevice(lu->ctx->device));
    return lu_sweeps(lu, b->d, x->d);
}

int32_t kryst_lu_export(kryst_lu_t lu, int64_t n, int64_t* row_perm, int64_t* col_perm, double* factors) {
    KR_ARG(lu, "lu_export");
    if (lu->n < 0) { set_error("lu_export: no factorization is cached"); return KRYST_SOLVE_ERROR; }
    KR_ARG(n == lu->n, "lu_export: n differs from the cached factorization");
    KR_HIP(hipSetDevice(lu->ctx->device));
    std::vector<int32_t> rp((size_t)n), cp((size_t)n);
    hipStream_t st = lu->ctx->s_main;
    if (n > 0) {
        KR_HIP(hipMemcpyAsync(rp.data(), lu->d_rp, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        KR_HIP(hipMemcpyAsync(cp.data(), lu->d_cp, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        if (factors) KR_HIP(hipMemcpyAsync(factors, lu->d_f, sizeof(double) * (size_t)(n * n), hipMemcpyDeviceToHost, st));
    }
    KR_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
        if (row_perm) row_perm[i] = rp[(size_t)i];
        if (col_perm) col_perm[i] = cp[(size_t)i];
    }
    return KRYST_OK;
}

int32_t kryst_lu_info(kryst_lu_t lu, int64_t* info, int32_t count) {
    KR_ARG(lu && info && count >= 4, "lu_info");
    info[0] = KRYST_DENSE_MAX;
    info[1] = tail_rows();
    info[2] = KR_DENSE_TR;
    info[3] = lu->n;
    return KRYST_OK;
}

int32_t kryst_qr_solve_dev(kryst_dense_t a, kryst_pc_t pc, kryst_vec_t b, kryst_vec_t x, kryst_stats_t* stats) {
    KR_ARG(a, "qr_solve_dev");
    KR_TRY(dense_check_pc(a, pc));
    KR_TRY(dense_check_square(a, "dense QR"));
    KR_TRY(dense_check_vecs(a, b, x));
    KR_TRY(qr_run(a, b->d, x->d));
    direct_stats(stats);
    return KRYST_OK;
}

int32_t kryst_qr_solve(kryst_dense_t a, kryst_pc_t pc, const double* b, double* x, int64_t n, kryst_stats_t* stats) {
    KR_ARG(a && ((b && x) || n == 0), "qr_solve");
    KR_TRY(dense_check_pc(a, pc));
    KR_TRY(dense_check_square(a, "dense QR"));
    KR_ARG(n == a->nrows, "qr_solve: vector length");
    KR_TRY(with_host_vectors(a->ctx, b, x, n, [&](double* d) -> int32_t { return qr_run(a, d, d); }));
    direct_stats(stats);
    return KRYST_OK;
}

}  // extern "C"
