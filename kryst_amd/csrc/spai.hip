// SPAI set-up (ApproxInv::setup, src/preconditioner/approxinv.rs:123-264) on the device, with labelled deviations and one extension
// (DESIGN.md section 4.6):
//  * extension: pattern kind 2, the operator's own pattern (J_j = the stored columns of row j of A), what SparsityPattern::Auto's code
//    was meant to do; Auto itself returns KRYST_UNSUPPORTED as written (its downcasts never succeed, approxinv.rs:127-133, 301-323);
//  * reduced least squares: column j is solved on A[I_j, J_j] with e_j restricted to I_j (I_j = the sorted union of the stored rows of
//    the columns J_j); the rows outside I_j are zero in A[:, J_j], so the minimiser is the reference's.  Householder QR replaces faer's
//    FullPivLu / Qr::solve_lstsq, so set-up values agree to rounding, not bit for bit;
//  * errors instead of non-finite output or panics: a bad pattern and a non-square operator KRYST_ERR_ARG, a zero Householder column,
//    a non-finite A[I_j, J_j] or a non-finite m_j KRYST_FACTOR_ERROR, a distributed operator and a column over the caps below
//    KRYST_UNSUPPORTED.  Each column's pattern is used sorted ascending.
//
// Set-up: (1) A's CSC by the deterministic transpose of transpose.hip (atomic counts, a scan, atomic slots, then every segment sorted); (2) a size pass
// (the m cap, the largest m; for wide patterns also the largest stored-entry count); (3) the column kernel: one group of m_max + 1 lanes per column, floor(64 / (m_max + 1))
// columns per wave -- lane k gathers column J_k of A, the lanes merge their sorted row lists into I_j, build A[I_j, J_j] | e_hat (lane k
// owns column k, lane m the right-hand side; with the lists and tiles in registers for m_max <= 15, lists of at most 8 and |I_j| <= 32,
// else in LDS, where a second pass takes the columns the register form deferred), run m Householder steps and back-substitute; (4) M's columns turned into CSR rows by the same
// transpose, with the strict drop |M_ij| > tol applied while counting.  The apply is the existing KR_PC_SPAI kind.
#include "pc.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace kr {

constexpr int KR_SPAI_MMAX = 64;        // pattern entries of a column (m)
constexpr int KR_SPAI_IMAX = 128;       // rows of the reduced problem (|I_j|)
constexpr int KR_SPAI_TMAX = 2048;      // stored entries of A[:, J_j]
constexpr int KR_SPAI_IFAST = 32;       // rows of the first pass's tiles for narrow patterns (register tiles)
constexpr int KR_SPAI_RMAX = 8;         // ... and stored entries per column of A that a lane keeps in registers
constexpr int64_t KR_SPAI_GRID_CAP = 1 << 20;
constexpr unsigned KR_SPAI_SIZE_GRID = 2048;   // size pass: workgroups (its maxima end in one atomic per wave on one word: 2M waves took 48 ms)

// error word: min over the failing columns of (column << 8 | code)
enum { KR_SPAI_CAP = 0, KR_SPAI_NONFINITE_A = 1, KR_SPAI_ZERO_COLUMN = 2, KR_SPAI_NONFINITE_M = 3 };
constexpr unsigned long long KR_SPAI_NOERR = ~0ull;

__device__ __forceinline__ void spai_fail(unsigned long long* err, int64_t j, int code) {
    atomicMin(err, ((unsigned long long)j << 8) | (unsigned long long)code);
}

static unsigned spai_grid(int64_t items, int per_wg) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_wg - 1) / per_wg, KR_SPAI_GRID_CAP));
}

// ---------------------------------------------------------------- size pass: the caps, the largest m and (WITH_T) the largest stored-entry count
template <bool WITH_T>
__global__ __launch_bounds__(256) void spai_size_kernel(const int32_t* pptr, const int32_t* pidx, const int32_t* cp, int64_t n,
                                                        unsigned long long* err, int32_t* stats) {
    int32_t mmax = 0, tmax = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p0 = pptr[j], m = pptr[j + 1] - p0;
        if (m > KR_SPAI_MMAX) { spai_fail(err, j, KR_SPAI_CAP); continue; }
        int64_t t = 0;
        if (WITH_T) for (int q = 0; q < m; ++q) { const int32_t c = pidx[p0 + q]; t += cp[c + 1] - cp[c]; }
        if (t > KR_SPAI_TMAX) { spai_fail(err, j, KR_SPAI_CAP); continue; }
        mmax = max(mmax, m); tmax = max(tmax, (int32_t)t);
    }
    for (int o = 32; o > 0; o >>= 1) { mmax = max(mmax, __shfl_xor(mmax, o, 64)); tmax = max(tmax, __shfl_xor(tmax, o, 64)); }
    if ((threadIdx.x & 63) == 0) { atomicMax(&stats[0], mmax); atomicMax(&stats[1], tmax); }     // one pair of atomics per wave
}

// ---------------------------------------------------------------- the column kernel
struct SpaiCols {
    const int32_t* pptr; const int32_t* pidx;                 // the pattern: column j of M has rows pidx[pptr[j] .. pptr[j+1]), ascending
    const int32_t* cp; const int32_t* cr; const double* cv;   // A as CSC, rows ascending in each column
    int64_t n;
    int G, P, Icap, Tcap;                                       // lanes per column (m_max + 1), columns per workgroup, LDS capacities
    double* mval;                                               // out: m_j at pptr[j] .. pptr[j+1]
    unsigned long long* err;
    uint8_t* defer;                                             // first pass (register tiles): the columns it leaves to the second
    int32_t* ndefer;                                            // ... their count
    int32_t* tdefer;                                            // ... the largest stored-entry count among them
    int second;                                                 // second pass: only the deferred columns
};

// RT = 0: the tile A[I_j, J_j] | e_hat in LDS (a.Icap rows).  RT > 0: each lane keeps its column of the tile in RT registers (a.Icap <= RT)
// and only the current reflector goes through LDS; the LDS tile then holds R and Q^T e_hat for the back substitution (G rows).  The RT form
// also keeps each lane's list (at most KR_SPAI_RMAX entries) in registers, so that the union walks every other list once for all of the
// lane's rows; a column it cannot take (a list longer than KR_SPAI_RMAX, |I_j| > RT) is deferred to the RT = 0 form.
template <int RT>
__global__ __launch_bounds__(128) void spai_column_kernel(const SpaiCols a) {
    extern __shared__ double spai_lds[];
    const int G = a.G, P = a.P, S = P * G;
    double* T = spai_lds;                                       // [rows][S]: group g's column c at g G + c, the right-hand side at c = m
    double* Rd = T + (size_t)(RT > 0 ? G : a.Icap) * S;         // [S] R_kk
    double* Hn = Rd + S;                                        // [P] v^T v / 2 of the current reflector
    double* Vb = Hn + P;                                        // [P][RT] the current reflector (RT > 0)
    double* Lv = Vb + (size_t)P * RT;                           // [P][Tcap] the values of the group's lists (RT = 0; RT > 0: in registers)
    int32_t* Lr = reinterpret_cast<int32_t*>(Lv + (RT > 0 ? 0 : (size_t)P * a.Tcap));   // [P][Tcap] the rows of the group's lists, list after list
    int32_t* Lf = Lr + (size_t)P * a.Tcap;                      // [P][Tcap] first occurrences before this entry in its list
    int32_t* Lo = Lf + (size_t)P * a.Tcap;                      // [P][G + 1] list offsets
    int32_t* Ft = Lo + P * (G + 1);                             // [P][G] first occurrences per list
    int32_t* Ej = Ft + P * G;                                   // [P] position of j in I_j, -1: j is not in I_j
    int32_t* Cm = Ej + P;                                       // [P] the longest list of the column
    const int t = threadIdx.x, g = t / G, k = t - g * G;
    const bool lane = g < P;
    const int col = g * G + k;
    int32_t* lo = Lo + g * (G + 1);
    int32_t* lr = Lr + (size_t)g * a.Tcap;
    double* lv = Lv + (size_t)g * a.Tcap;
    int32_t* lf = Lf + (size_t)g * a.Tcap;
    int32_t* ft = Ft + g * G;
    const int64_t nw = (a.n + P - 1) / P;
    for (int64_t w = blockIdx.x; w < nw; w += gridDim.x) {     // uniform over the workgroup
        const int64_t j = w * P + g;
        int m = 0, p0 = 0;
        if (lane && j < a.n) { p0 = a.pptr[j]; m = a.pptr[j + 1] - p0; }
        bool live = lane && j < a.n && m <= G - 1 && (!a.second || a.defer[j]);      // (a longer column was refused by the size pass)
        const bool own = live && k < m;                         // lane k owns pattern column J_k
        int32_t c0 = 0, cnt = 0;
        if (own) { const int32_t jk = a.pidx[p0 + k]; c0 = a.cp[jk]; cnt = a.cp[jk + 1] - c0; }
        if (lane) { lo[k + 1] = cnt; if (k == 0) { lo[0] = 0; Ej[g] = -1; } }
        __syncthreads();
        if (lane && k == 0) {
            int32_t cm = 0;
            for (int q = 0; q < G; ++q) { cm = max(cm, lo[q + 1]); lo[q + 1] += lo[q]; }
            Cm[g] = cm;
        }
        __syncthreads();
        const int32_t tot = lane ? lo[G] : 0;                   // stored entries of A[:, J_j]
        // the column is deferred to the second pass (the RT form's limits) or refused (the caps)
        auto defer_or_fail = [&](bool can_defer) {
            if (k == 0) {
                if (can_defer && !a.second && a.defer) { a.defer[j] = 1; atomicAdd(a.ndefer, 1); atomicMax(a.tdefer, tot); }
                else spai_fail(a.err, j, KR_SPAI_CAP);
            }
            live = false;
        };
        if (live && tot > KR_SPAI_TMAX) defer_or_fail(false);
        if (live && (tot > a.Tcap || (RT > 0 && Cm[g] > KR_SPAI_RMAX))) defer_or_fail(true);
        const int32_t my0 = lane ? lo[k] : 0;
        constexpr int RM = RT > 0 ? KR_SPAI_RMAX : 1;
        int32_t rr[RM]; double vv[RM];                          // (RT > 0) this lane's list: rows (-1 past its end) and values
        if constexpr (RT > 0) {
#pragma unroll
            for (int i = 0; i < RM; ++i) { rr[i] = -1; vv[i] = 0.0; }
            if (own && live) {
#pragma unroll
                for (int i = 0; i < RM; ++i) if (i < cnt) { rr[i] = a.cr[c0 + i]; vv[i] = a.cv[c0 + i]; }
#pragma unroll
                for (int i = 0; i < RM; ++i) if (i < cnt) lr[my0 + i] = rr[i];
            }
        }
        if (RT == 0 && own && live)
            for (int i = 0; i < cnt; i += 4) {                  // four rows and values in flight
                int32_t x[4]; double y[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { x[q] = i + q < cnt ? a.cr[c0 + i + q] : 0; y[q] = i + q < cnt ? a.cv[c0 + i + q] : 0.0; }
#pragma unroll
                for (int q = 0; q < 4; ++q) if (i + q < cnt) { lr[my0 + i + q] = x[q]; lv[my0 + i + q] = y[q]; }
            }
        __syncthreads();
        // I_j = the union of the lists: a row belongs to the first list that holds it; lf = the first occurrences before it in its own list
        int32_t nf = 0;
        if (RT > 0 && own && live) {                            // each earlier list read once, against all of this lane's rows
            bool fs[RM];
#pragma unroll
            for (int i = 0; i < RM; ++i) fs[i] = true;
            for (int q = 0; q < k; ++q) {
                const int base = lo[q], len = lo[q + 1] - base;
#pragma unroll 4
                for (int u = 0; u < len; ++u) {
                    const int32_t x = lr[base + u];
#pragma unroll
                    for (int i = 0; i < RM; ++i) fs[i] = fs[i] && x != rr[i];
                }
            }
#pragma unroll
            for (int i = 0; i < RM; ++i) if (i < cnt) { lf[my0 + i] = nf; nf += fs[i] ? 1 : 0; }
        }
        if (RT == 0 && own && live)
            for (int i = 0; i < cnt; ++i) {
                const int32_t r = lr[my0 + i];
                bool first = true;
                for (int q = 0; q < k && first; ++q) {         // (linear scans: the lists are short, the loads independent)
                    const int32_t* L = lr + lo[q];
                    const int len = lo[q + 1] - lo[q];
                    bool hit = false;
#pragma unroll 4
                    for (int u = 0; u < len; ++u) hit |= L[u] == r;
                    first = !hit;
                }
                lf[my0 + i] = nf;
                nf += first ? 1 : 0;
            }
        if (lane) ft[k] = nf;
        __syncthreads();
        int ni = 0;                                             // |I_j|
        if (live) for (int q = 0; q < m; ++q) ni += ft[q];
        if (live && ni > a.Icap) defer_or_fail(ni <= KR_SPAI_IMAX);
        // A[I_j, J_j]: the position of row r in I_j = the first occurrences below r, summed over the lists
        double c[RT > 0 ? RT : 1];                              // (RT > 0) this lane's column of the tile
#pragma unroll
        for (int q = 0; q < (RT > 0 ? RT : 1); ++q) c[q] = 0.0;
        if (RT == 0 && live && k <= m) for (int i = 0; i < ni; ++i) T[(size_t)i * S + col] = 0.0;
        bool bad = false;
        if (RT > 0 && own && live) {                            // every list read once: the lower bounds of all of this lane's rows together
            int pos[RM];
#pragma unroll
            for (int i = 0; i < RM; ++i) pos[i] = 0;
            for (int q = 0; q < m; ++q) {
                const int base = lo[q], len = lo[q + 1] - base;
                int pl[RM];
#pragma unroll
                for (int i = 0; i < RM; ++i) pl[i] = 0;
#pragma unroll 4
                for (int u = 0; u < len; ++u) {
                    const int32_t x = lr[base + u];
#pragma unroll
                    for (int i = 0; i < RM; ++i) pl[i] += x < rr[i] ? 1 : 0;
                }
#pragma unroll
                for (int i = 0; i < RM; ++i) pos[i] += pl[i] < len ? lf[base + pl[i]] : ft[q];
            }
#pragma unroll
            for (int i = 0; i < RM; ++i) {
                if (i >= cnt) continue;
                const double v = vv[i];
#pragma unroll
                for (int q = 0; q < (RT > 0 ? RT : 1); ++q) c[q] = q == pos[i] ? v : c[q];
                bad |= !isfinite(v);
                if (rr[i] == j) Ej[g] = pos[i];
            }
        }
        if (RT == 0 && own && live)
            for (int i = 0; i < cnt; ++i) {
                const int32_t r = lr[my0 + i];
                int pos = 0;
                for (int q = 0; q < m; ++q) {
                    const int32_t* L = lr + lo[q];
                    const int len = lo[q + 1] - lo[q];
                    int p = 0;                                  // lower bound of r in list q
#pragma unroll 4
                    for (int u = 0; u < len; ++u) p += L[u] < r ? 1 : 0;
                    pos += p < len ? lf[lo[q] + p] : ft[q];
                }
                const double v = lv[my0 + i];
                if constexpr (RT > 0) {
#pragma unroll
                    for (int q = 0; q < RT; ++q) c[q] = q == pos ? v : c[q];
                } else {
                    T[(size_t)pos * S + col] = v;
                }
                bad |= !isfinite(v);
                if (r == j) Ej[g] = pos;                        // (every list that holds row j finds the same position)
            }
        if (bad) spai_fail(a.err, j, KR_SPAI_NONFINITE_A);
        __syncthreads();
        if constexpr (RT > 0) {
            const int ej = (live && k == m) ? Ej[g] : -1;     // e_j restricted to I_j
#pragma unroll
            for (int q = 0; q < RT; ++q) c[q] = q == ej ? 1.0 : c[q];
            // Householder QR in registers, step s of every column of the workgroup together (the right-hand side's lane too)
            for (int s = 0; s < G - 1; ++s) {
                if (live && k == s && s < m) {
                    double amax = 0.0;
#pragma unroll
                    for (int q = 0; q < RT; ++q) if (q >= s && q < ni) amax = fmax(amax, fabs(c[q]));
                    double alpha = 0.0, hn = 0.0;
                    if (amax == 0.0) {
                        spai_fail(a.err, j, KR_SPAI_ZERO_COLUMN);
                    } else {
                        double ss = 0.0;
#pragma unroll
                        for (int q = 0; q < RT; ++q) if (q >= s && q < ni) { const double y = c[q] / amax; ss = ss + y * y; }
                        const double nrm = amax * sqrt(ss);
                        double x0 = 0.0;
#pragma unroll
                        for (int q = 0; q < RT; ++q) x0 = q == s ? c[q] : x0;
                        alpha = x0 < 0.0 ? nrm : -nrm;
#pragma unroll
                        for (int q = 0; q < RT; ++q) c[q] = q == s ? x0 - alpha : c[q];
                        hn = nrm * (nrm + fabs(x0));
                    }
#pragma unroll
                    for (int q = 0; q < RT; ++q) if (q >= s && q < ni) Vb[g * RT + q] = c[q];
                    Rd[col] = alpha; Hn[g] = hn;
                }
                __syncthreads();
                if (live && k > s && k <= m && s < m && Hn[g] != 0.0) {
                    const double hn = Hn[g];
                    double d = 0.0;
#pragma unroll
                    for (int q = 0; q < RT; ++q) if (q >= s && q < ni) d = d + Vb[g * RT + q] * c[q];
                    const double f = d / hn;
#pragma unroll
                    for (int q = 0; q < RT; ++q) if (q >= s && q < ni) c[q] = c[q] - f * Vb[g * RT + q];
                }
                __syncthreads();
            }
            // R (rows 0..m-1 of the columns) and Q^T e_hat to the LDS tile for the back substitution
            if (live && k <= m && m <= ni) {
#pragma unroll
                for (int q = 0; q < RT; ++q) if (q < m) T[(size_t)q * S + col] = c[q];
            }
            __syncthreads();
        }
        if (RT == 0 && live && k == m && Ej[g] >= 0) T[(size_t)Ej[g] * S + col] = 1.0;    // e_j restricted to I_j
        // Householder QR, step s of every column of the workgroup together; the reflector is applied to the right-hand side too
        for (int s = 0; s < (RT > 0 ? 0 : G - 1); ++s) {
            if (live && k == s && s < m) {
                double amax = 0.0;
                for (int i = s; i < ni; i += 4) {               // (rows four at a time: the LDS loads in flight together)
                    double x[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) x[q] = i + q < ni ? T[(size_t)(i + q) * S + col] : 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) amax = fmax(amax, fabs(x[q]));
                }
                double alpha = 0.0, hn = 0.0;
                if (amax == 0.0) {
                    spai_fail(a.err, j, KR_SPAI_ZERO_COLUMN);
                } else {
                    double ss = 0.0;
                    for (int i = s; i < ni; i += 4) {
                        double x[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) x[q] = i + q < ni ? T[(size_t)(i + q) * S + col] : 0.0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) if (i + q < ni) { const double y = x[q] / amax; ss = ss + y * y; }
                    }
                    const double nrm = amax * sqrt(ss);
                    const double x0 = T[(size_t)s * S + col];
                    alpha = x0 < 0.0 ? nrm : -nrm;              // v = x - alpha e_1 without cancellation
                    T[(size_t)s * S + col] = x0 - alpha;
                    hn = nrm * (nrm + fabs(x0));                // v^T v / 2
                }
                Rd[col] = alpha; Hn[g] = hn;
            }
            __syncthreads();
            if (live && k > s && k <= m && s < m && Hn[g] != 0.0) {
                const double* v = T + g * G + s;
                double d = 0.0;
                for (int i = s; i < ni; i += 4) {
                    double x[4], y[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { x[q] = i + q < ni ? v[(size_t)(i + q) * S] : 0.0; y[q] = i + q < ni ? T[(size_t)(i + q) * S + col] : 0.0; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (i + q < ni) d = d + x[q] * y[q];
                }
                const double f = d / Hn[g];
                for (int i = s; i < ni; i += 4) {
                    double x[4], y[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { x[q] = i + q < ni ? v[(size_t)(i + q) * S] : 0.0; y[q] = i + q < ni ? T[(size_t)(i + q) * S + col] : 0.0; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (i + q < ni) T[(size_t)(i + q) * S + col] = y[q] - f * x[q];
                }
            }
            __syncthreads();
        }
        // back substitution R x = (Q^T e)[0..m) by the right-hand side's lane (rows below m exist only when m <= |I_j|)
        if (live && k == m && m <= ni) {
            bool nonfinite = false;
            for (int s = m - 1; s >= 0; --s) {
                double sum = T[(size_t)s * S + col];
                for (int c = s + 1; c < m; ++c) sum = sum - T[(size_t)s * S + g * G + c] * T[(size_t)c * S + col];
                const double x = sum / Rd[g * G + s];
                T[(size_t)s * S + col] = x;
                nonfinite |= !isfinite(x);
            }
            if (nonfinite) spai_fail(a.err, j, KR_SPAI_NONFINITE_M);
        }
        __syncthreads();
        if (own && live && m <= ni) a.mval[p0 + k] = T[(size_t)k * S + g * G + m];
        __syncthreads();                                        // the next columns reuse the LDS
    }
}

static size_t spai_lds_bytes(int G, int P, int Icap, int Tcap, int RT) {
    const size_t S = (size_t)P * G;
    return sizeof(double) * ((size_t)(RT > 0 ? G : Icap) * S + S + (size_t)P + (size_t)P * RT + (RT > 0 ? 0 : (size_t)P * Tcap)) +
           sizeof(int32_t) * (2 * (size_t)P * Tcap + (size_t)P * (G + 1) + (size_t)P * G + 2 * (size_t)P);
}

// device temporaries of one set-up
struct SpaiTmp {
    int32_t* pptr = nullptr; int32_t* pidx = nullptr;           // a Manual pattern, sorted (the operator's pattern is A's own arrays)
    DevCsr csc;                                                // A by columns
    double* mval = nullptr;                                     // M's columns
    unsigned long long* err = nullptr;
    int32_t* stats = nullptr;
    uint8_t* defer = nullptr;                                   // the first pass's deferred columns, then their count
    ~SpaiTmp() {
        (void)hipFree(pptr); (void)hipFree(pidx); dev_csr_free(csc); (void)hipFree(mval); (void)hipFree(err); (void)hipFree(stats);
        (void)hipFree(defer);
    }
};

static int32_t spai_error(unsigned long long e) {
    const long long j = (long long)(e >> 8);
    switch ((int)(e & 255ull)) {
        case KR_SPAI_CAP:
            set_error("SPAI: column %lld is over the size caps (at most %d pattern entries, %d stored entries in A[:, J], %d rows in I)", j,
                      KR_SPAI_MMAX, KR_SPAI_TMAX, KR_SPAI_IMAX);
            return KRYST_UNSUPPORTED;
        case KR_SPAI_NONFINITE_A: set_error("SPAI: column %lld: A[I, J] holds a NaN or Inf", j); return KRYST_FACTOR_ERROR;
        case KR_SPAI_ZERO_COLUMN: set_error("SPAI: column %lld: A[I, J] is rank deficient (zero Householder column)", j); return KRYST_FACTOR_ERROR;
        default: set_error("SPAI: column %lld: the least-squares solution is not finite", j); return KRYST_FACTOR_ERROR;
    }
}

// the set-up's device part: A's CSC, the size pass, the column kernel, M's rows; M is returned as a plain device CSR operator
static int32_t spai_run(kryst_csr_t a, SpaiTmp& tp, const int32_t* pptr, const int32_t* pidx, int64_t npat, double tol, kryst_csr_t* mout) {
    kryst_ctx_t ctx = a->ctx;
    hipStream_t s = ctx->s_main;
    const int64_t n = a->nrows;
    KR_TRY(csr_transpose(ctx, "SPAI", a->d_row_ptr, a->d_col, a->d_val, n, n, false, 0.0, tp.csc));
    KR_HIP(hipMalloc(&tp.err, sizeof(unsigned long long)));
    KR_HIP(hipMalloc(&tp.stats, sizeof(int32_t) * 4));
    KR_HIP(hipMalloc(&tp.mval, sizeof(double) * (size_t)std::max<int64_t>(npat, 1)));
    KR_HIP(hipMemsetAsync(tp.err, 0xFF, sizeof(unsigned long long), s));
    KR_HIP(hipMemsetAsync(tp.stats, 0, sizeof(int32_t) * 4, s));
    unsigned long long e = KR_SPAI_NOERR;
    int32_t st[4] = {0, 0, 0, 0};                               // largest m, largest stored-entry count, deferred columns, their largest count
    auto fetch = [&]() -> int32_t {
        KR_HIP(hipGetLastError());
        KR_HIP(hipMemcpyAsync(&e, tp.err, sizeof e, hipMemcpyDeviceToHost, s));
        KR_HIP(hipMemcpyAsync(st, tp.stats, sizeof st, hipMemcpyDeviceToHost, s));
        KR_HIP(hipStreamSynchronize(s));
        return e != KR_SPAI_NOERR ? spai_error(e) : KRYST_OK;
    };
    if (n > 0) hipLaunchKernelGGL(spai_size_kernel<false>, dim3(std::min(spai_grid(n, 256), KR_SPAI_SIZE_GRID)), dim3(256), 0, s, pptr, pidx, (const int32_t*)tp.csc.ptr, n, tp.err, tp.stats);
    KR_TRY(fetch());
    // lanes per column: the longest pattern + the right-hand side; one wave of columns, or two waves for one column of 64
    const int G = st[0] + 1;
    const int wg = G <= 64 ? 64 : 128;
    const int P = wg / G;
    // narrow patterns (m_max <= 15; 7-point: |I_j| <= 25 of up to 49 stored entries) first run with the tile and each lane's list in registers
    // (the LDS holds the lists and R only, so more waves fit a CU, and neither the union nor the Householder steps go through LDS for the
    // lane's own data); the columns that form cannot take are left to a second pass with the tile in LDS, sized by those columns alone.
    // Wider patterns take the LDS form at once, sized by the whole pattern's largest stored-entry count (a size pass with the counts).
    const bool fast = G <= 16;
    int lds_max = 0;
    KR_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    if (fast) {
        KR_HIP(hipMalloc(&tp.defer, (size_t)std::max<int64_t>(n, 1)));
        KR_HIP(hipMemsetAsync(tp.defer, 0, (size_t)std::max<int64_t>(n, 1), s));
    } else {
        if (n > 0) hipLaunchKernelGGL(spai_size_kernel<true>, dim3(std::min(spai_grid(n, 256), KR_SPAI_SIZE_GRID)), dim3(256), 0, s, pptr, pidx, (const int32_t*)tp.csc.ptr, n, tp.err, tp.stats);
        KR_TRY(fetch());
    }
    const int64_t nw = (n + P - 1) / P;
    for (int pass = fast ? 0 : 1; pass < 2; ++pass) {
        const bool regs = pass == 0;
        const int tc = regs ? G * KR_SPAI_RMAX : std::max(1, fast ? st[3] : st[1]);
        const int ic = regs ? KR_SPAI_IFAST : std::max(1, std::min(KR_SPAI_IMAX, tc));
        const size_t lds = spai_lds_bytes(G, P, ic, tc, regs ? KR_SPAI_IFAST : 0);
        if (lds > (size_t)lds_max) {                            // (the effective limit of the LDS form: DESIGN.md section 4.6)
            set_error("SPAI: the widest columns (%d pattern entries, %d stored entries in A[:, J]) need %zu bytes of LDS per workgroup; the "
                      "device has %d", G - 1, tc, lds, lds_max);
            return KRYST_UNSUPPORTED;
        }
        const SpaiCols args{pptr, pidx, tp.csc.ptr, tp.csc.idx, tp.csc.val, n, G, P, ic, tc, tp.mval, tp.err,
                            tp.defer, tp.stats + 2, tp.stats + 3, fast && !regs};
        if (n > 0 && regs) {
            hipLaunchKernelGGL(spai_column_kernel<KR_SPAI_IFAST>, dim3(spai_grid(nw, 1)), dim3(wg), lds, s, args);
        } else if (n > 0) {
            if (lds > ((size_t)48 << 10))
                KR_HIP(hipFuncSetAttribute((const void*)spai_column_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(spai_column_kernel<0>, dim3(spai_grid(nw, 1)), dim3(wg), lds, s, args);
        }
        KR_TRY(fetch());
        if (regs && st[2] == 0) break;                          // (no column was deferred)
    }
    dev_csr_free(tp.csc);                                          // (A's columns are not needed any more)
    // M's columns -> M's rows, |M_ij| > tol kept
    DevCsr mr;
    KR_TRY(csr_transpose(ctx, "SPAI", pptr, pidx, tp.mval, n, n, true, tol, mr));
    kryst_csr_t m = new kryst_csr_s();
    m->ctx = ctx; m->nrows = n; m->ncols = n; m->xlen = n; m->nnz = mr.nnz;
    m->d_row_ptr = mr.ptr; m->d_col = mr.idx; m->d_val = mr.val;
    m->ntiles = ntiles_of(n);
    const double per_slice = n > 0 ? (double)mr.nnz / (double)((n + 127) / 128) : 0.0;     // the SpMV's window size (csr_create.hip: upload_csr)
    m->slots = per_slice <= 256.0 ? 2 : (per_slice <= 512.0 ? 4 : 7);
    *mout = m;
    return KRYST_OK;
}

// ApproxInv::apply (approxinv.rs:268-298): z_i = sum_j M_ij r_j, ascending j from 0 -- an SpMV with M, the operator `a` of this object
struct SpaiPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_SPAI;
    const bool owns_m;                // M of a set-up on the device; rows handed in by the caller stay the caller's
    SpaiPc(kryst_csr_t m, bool owns) : kryst_pc_s(m->ctx, KIND, m, m->nrows), owns_m(owns) {}
    ~SpaiPc() override { if (owns_m) kryst_csr_destroy(a); }
    int32_t apply(int64_t, const double* r, double* z, const int* done) override { return launch_spmv(a, r, z, 0, nullptr, done); }
};

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_spai(kryst_csr_t a, int32_t pattern_kind, const int64_t* pat_ptr, const int64_t* pat_idx, int64_t pat_n, double tol,
                      kryst_pc_t* out) {
    KR_ARG(a && out, "pc_spai");
    KR_ARG(pattern_kind >= KRYST_SPAI_MANUAL && pattern_kind <= KRYST_SPAI_OPERATOR, "pc_spai: unknown pattern kind");
    if (pattern_kind == KRYST_SPAI_AUTO) {                      // approxinv.rs:127-133 (the downcasts of :301-323 never succeed)
        set_error("SparsityPattern::Auto requires nrows() or row_indices() support");
        return KRYST_UNSUPPORTED;
    }
    if (a->dist) { set_error("SPAI: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->nrows == a->ncols && a->nrows == a->xlen, "pc_spai: square operator required");
    KR_ARG(a->nnz < (1ll << 31) - 16, "pc_spai: nnz exceeds int32 device indexing");
    const int64_t n = a->nrows;
    std::vector<int32_t> hptr, hidx;
    if (pattern_kind == KRYST_SPAI_MANUAL) {                    // n = pat.len() (approxinv.rs:125); column j = pat[j]
        KR_ARG(pat_n == n, "pc_spai: the pattern's length differs from the operator's size");
        KR_ARG(n == 0 || (pat_ptr && pat_ptr[0] == 0), "pc_spai: pat_ptr is NULL or pat_ptr[0] != 0");
        hptr.assign((size_t)n + 1, 0);
        for (int64_t j = 0; j < n; ++j) {
            const int64_t len = pat_ptr[j + 1] - pat_ptr[j];
            KR_ARG(len >= 0, "pc_spai: pat_ptr is not ascending");
            KR_ARG(pat_ptr[j + 1] < (1ll << 31) - 16, "pc_spai: pattern entries exceed int32 device indexing");
            if (len > KR_SPAI_MMAX) {
                set_error("SPAI: column %lld has %lld pattern entries; at most %d are supported", (long long)j, (long long)len, KR_SPAI_MMAX);
                return KRYST_UNSUPPORTED;
            }
            hptr[(size_t)j + 1] = (int32_t)pat_ptr[j + 1];
        }
        KR_ARG(n == 0 || pat_idx || hptr.back() == 0, "pc_spai: pat_idx is NULL");
        hidx.resize((size_t)hptr.back());
        for (int64_t j = 0; j < n; ++j) {                      // each column sorted ascending (deviation 3), checked
            std::vector<int64_t> g(pat_idx + pat_ptr[j], pat_idx + pat_ptr[j + 1]);
            std::sort(g.begin(), g.end());
            for (size_t i = 0; i < g.size(); ++i) {
                KR_ARG(g[i] >= 0 && g[i] < n, "pc_spai: pattern index out of range");
                KR_ARG(i == 0 || g[i] != g[i - 1], "pc_spai: pattern index repeated within a column");
                hidx[(size_t)hptr[(size_t)j] + i] = (int32_t)g[i];
            }
        }
    }
    KR_HIP(hipSetDevice(a->ctx->device));
    kryst_csr_t m = nullptr;
    int32_t rc = KRYST_OK;
    {
        SpaiTmp tp;
        const int32_t* pptr = a->d_row_ptr;                     // the operator's pattern: column j of M = the columns of row j of A
        const int32_t* pidx = a->d_col;
        int64_t npat = a->nnz;
        if (pattern_kind == KRYST_SPAI_MANUAL) {
            npat = (int64_t)hidx.size();
            if (hipMalloc(&tp.pptr, sizeof(int32_t) * hptr.size()) != hipSuccess ||
                hipMalloc(&tp.pidx, sizeof(int32_t) * std::max<size_t>(hidx.size(), 1)) != hipSuccess ||
                hipMemcpyAsync(tp.pptr, hptr.data(), sizeof(int32_t) * hptr.size(), hipMemcpyHostToDevice, a->ctx->s_main) != hipSuccess ||
                (!hidx.empty() && hipMemcpyAsync(tp.pidx, hidx.data(), sizeof(int32_t) * hidx.size(), hipMemcpyHostToDevice, a->ctx->s_main) != hipSuccess)) {
                set_error("SPAI: pattern upload failed"); rc = KRYST_ERR_HIP;
            }
            pptr = tp.pptr; pidx = tp.pidx;
        }
        if (rc == KRYST_OK) rc = spai_run(a, tp, pptr, pidx, npat, tol, &m);
        (void)hipStreamSynchronize(a->ctx->s_main);             // the temporaries go with tp, after the last kernel that reads them
    }
    if (rc != KRYST_OK) return rc;
    *out = new SpaiPc(m, true);
    return KRYST_OK;
}

int32_t kryst_pc_approx_inverse(kryst_csr_t m, kryst_pc_t* out) {
    KR_ARG(m && out, "pc_approx_inverse");
    KR_ARG(m->nrows == m->xlen, "pc_approx_inverse: the inverse rows must form a square operator");
    *out = new SpaiPc(m, false);
    return KRYST_OK;
}

int32_t kryst_pc_spai_export(kryst_pc_t h, int64_t* nnz, int64_t* row_ptr, int32_t* col, double* val) {
    SpaiPc* pc = pc_cast<SpaiPc>(h);
    KR_ARG(pc && nnz, "pc_spai_export");
    KR_ARG(!row_ptr || (col && val), "pc_spai_export: col / val are NULL");
    *nnz = pc->a->nnz;
    if (!row_ptr) return KRYST_OK;
    return kryst_csr_download(pc->a, row_ptr, col, val);
}

}  // extern "C"
