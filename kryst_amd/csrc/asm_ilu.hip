// Additive Schwarz with ILU(0) subdomain solves: a labelled extension of AdditiveSchwarz::setup's `solver_factory`
// (src/preconditioner/asm.rs:38-40, "e.g. GMRES+ILU").  Index sets, growth, owners, variants and the combine are those of asm.hip (asm.h);
// the inner solver of subdomain k is an incomplete factorisation of S_k = A[g_k, g_k] (every stored entry kept, columns outside g_k dropped):
// KRYST_ILU_ILUP0 is Ilup::new(0) as written (l_ij = a_ij / a_jj, U = triu(S_k)), KRYST_ILU_TRUE_ILU0 the textbook IKJ ILU(0) on S_k's pattern,
// both applied as ilup.rs:138-167 does (sums in ascending column order, every operation rounded on its own, a factor entry equal to 0.0 skipped,
// the division only by a stored non-zero diagonal).
//
// Set-up, one workgroup per subdomain: count and extract S_k in local indices; the factor values (ILUP0 pointwise; textbook ILU(0) round by
// round, a row once every row it eliminates with is done, one lane per row); the levels of the forward and of the backward sweep over the kept
// (non-zero) entries; the rows ordered by level and the entries of a level laid out entry-major (entry e of the q-th row of a level of m rows
// at e m + q), so that the lanes of a level read consecutive addresses.  Apply: one kernel, workgroups stride over subdomains, the
// subdomain's vector in dynamic LDS, a workgroup barrier between levels, the next level's rows and entries loaded ahead of the barrier;
// then the combine kernel of asm.hip.
#include "asm.h"
#include <climits>
#include <cstdlib>
#include <vector>

namespace kr {

constexpr int KR_AI_MAX = KRYST_ASM_ILU_MAX_ROWS;
constexpr int KR_AI_T = 256;
constexpr unsigned long long KR_AI_NOERR = ~0ull;
constexpr unsigned short KR_AI_PAD = 0xFFFFu;       // no entry here (a level's rows are padded to its longest)

// a[i] <- sum of a[j], j < i, for i < n (a workgroup's array in global memory); returns the total.  Called by every thread.
__device__ inline int ai_scan(int32_t* a, int n, int* part) {
    const int t = threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += KR_AI_T) {
        const int i = i0 + t, v = i < n ? a[i] : 0;
        part[t] = v;
        __syncthreads();
        for (int o = 1; o < KR_AI_T; o <<= 1) {
            const int x = (t >= o) ? part[t - o] : 0;
            __syncthreads();
            part[t] += x;
            __syncthreads();
        }
        if (i < n) a[i] = base + part[t] - v;
        base += part[KR_AI_T - 1];
        __syncthreads();
    }
    return base;
}

// the position of local column j in sc[b .. e] (ascending, both ends included), or -1
__device__ inline int ai_find(const int32_t* sc, int b, int e, int j) {
    while (b < e) { const int mid = (b + e) >> 1; if (sc[mid] < j) b = mid + 1; else e = mid; }
    return (sc[b] == j) ? b : -1;
}

// ---------------------------------------------------------------- S_k: count, then extract
// pass 0: sp[i] = the stored entries of row g[i] whose column is in g, then the exclusive scan (sp has b + 1 slots per subdomain) and
// nnz_s[k]; pass 1 (soff known): the entries in local columns, the values, the position of every diagonal
__global__ __launch_bounds__(KR_AI_T) void ai_extract_kernel(const int32_t* row_ptr, const int32_t* col, const double* val, const int32_t* xoff,
                                                            const int32_t* idx, int64_t nsub, int pass, int32_t* sp_all, int64_t* nnz_s,
                                                            const int64_t* soff, int32_t* sc_all, double* w_all, int32_t* dpos_all) {
    __shared__ int part[KR_AI_T];
    const int t = threadIdx.x;
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {
        const int lo = xoff[k], b = xoff[k + 1] - lo;
        const int32_t* g = idx + lo;
        int32_t* sp = sp_all + lo + k;
        if (pass == 0) {
            for (int i = t; i <= b; i += KR_AI_T) {
                int cnt = 0;
                if (i < b) {
                    const int gi = g[i];
                    for (int32_t e = row_ptr[gi]; e < row_ptr[gi + 1]; ++e) {
                        const int c = col[e];
                        int l0 = 0, h = b;
                        while (l0 < h) { const int mid = (l0 + h) >> 1; if (g[mid] < c) l0 = mid + 1; else h = mid; }
                        cnt += (l0 < b && g[l0] == c) ? 1 : 0;
                    }
                }
                sp[i] = cnt;
            }
            __syncthreads();
            const int total = ai_scan(sp, b + 1, part);
            if (t == 0) nnz_s[k] = total;
        } else {
            int32_t* sc = sc_all + soff[k];
            double* w = w_all + soff[k];
            for (int i = t; i < b; i += KR_AI_T) {
                const int gi = g[i];
                int o = sp[i], d = -1;
                for (int32_t e = row_ptr[gi]; e < row_ptr[gi + 1]; ++e) {
                    const int c = col[e];
                    int l0 = 0, h = b;
                    while (l0 < h) { const int mid = (l0 + h) >> 1; if (g[mid] < c) l0 = mid + 1; else h = mid; }
                    if (l0 < b && g[l0] == c) {
                        if (l0 == i) d = o;
                        sc[o] = l0; w[o] = val[e]; ++o;
                    }
                }
                dpos_all[lo + i] = d;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- factor values, sweep levels, the level order and the layout's sizes
// Levels of one sweep round by round: a row takes the number of the round in which every row it reads (a kept entry: w != 0.0, column below
// the diagonal for the forward sweep, above it for the backward one) has a level from an earlier round.  lev must be all zero on entry.
template <bool LOWER>
__device__ inline int ai_levels(int b, const int32_t* sp, const int32_t* sc, const double* w, int32_t* lev) {
    const int t = threadIdx.x;
    int round = 0;
    for (;;) {
        ++round;
        int pending = 0;
        for (int i = t; i < b; i += KR_AI_T) {
            if (lev[i] != 0) continue;
            bool ready = true;
            for (int e = sp[i]; e < sp[i + 1] && ready; ++e) {
                const int j = sc[e];
                if ((LOWER ? j < i : j > i) && w[e] != 0.0) { const int lj = lev[j]; ready = lj != 0 && lj < round; }
            }
            if (ready) lev[i] = round; else pending = 1;
        }
        if (__syncthreads_or(pending) == 0) break;
    }
    return round;                                                           // the number of levels (b > 0)
}

// rows ordered by (level, row) into ord; lvl[l] = the first position of level l + 1's rows (nlev + 1 entries); ent[l] = the first entry of
// level l + 1 in the padded entry-major layout (nlev + 1 entries); returns the layout's entry count, or -1 past 2^31 - 1.  cur: b + 1 scratch.
template <bool LOWER>
__device__ inline long long ai_order(int b, int nlev, const int32_t* sp, const int32_t* sc, const double* w, const int32_t* lev, int32_t* ord,
                                     int32_t* lvl, int32_t* ent, int32_t* cur, int* part, int* levs, long long* kept) {
    const int t = threadIdx.x;
    __shared__ long long s_total, s_kept;
    for (int l = t; l <= nlev; l += KR_AI_T) { lvl[l] = 0; ent[l] = 0; }
    if (t == 0) s_kept = 0;
    __syncthreads();
    long long mykept = 0;
    for (int i = t; i < b; i += KR_AI_T) {
        int len = 0;
        for (int e = sp[i]; e < sp[i + 1]; ++e) { const int j = sc[e]; len += ((LOWER ? j < i : j > i) && w[e] != 0.0) ? 1 : 0; }
        mykept += len;
        atomicAdd(&lvl[lev[i] - 1], 1);
        atomicMax(&ent[lev[i] - 1], len);
    }
    if (mykept) atomicAdd((unsigned long long*)&s_kept, (unsigned long long)mykept);
    __syncthreads();
    (void)ai_scan(lvl, nlev + 1, part);
    for (int l = t; l <= nlev; l += KR_AI_T) cur[l] = lvl[l];
    __syncthreads();
    for (int i0 = 0; i0 < b; i0 += KR_AI_T) {                               // stable: chunk after chunk, inside a chunk by lane
        const int i = i0 + t, my = i < b ? lev[i] - 1 : -1;
        levs[t] = my;
        __syncthreads();
        int rank = 0; bool last = true;
        for (int u = 0; u < KR_AI_T; ++u) { const bool same = levs[u] == my; rank += (same && u < t) ? 1 : 0; last = last && !(same && u > t); }
        const int pos = my >= 0 ? cur[my] + rank : 0;
        __syncthreads();
        if (my >= 0) { ord[pos] = i; if (last) cur[my] = pos + 1; }
        __syncthreads();
    }
    if (t == 0) {                                                           // ent[l]: longest row of level l + 1 -> entry offsets
        long long off = 0;
        for (int l = 0; l < nlev; ++l) {
            const long long sz = (long long)ent[l] * (long long)(lvl[l + 1] - lvl[l]);
            ent[l] = (int32_t)(off > INT_MAX ? INT_MAX : off);
            off += sz;
        }
        ent[nlev] = (int32_t)(off > INT_MAX ? INT_MAX : off);
        s_total = off > INT_MAX ? -1 : off;
    }
    __syncthreads();
    *kept = s_kept;
    const long long total = s_total;
    __syncthreads();
    return total;
}

// err: min over the failures of (k << 28 | row << 14 | pivot row), local rows
__global__ __launch_bounds__(KR_AI_T) void ai_factor_kernel(const int32_t* xoff, int64_t nsub, int mode, const int32_t* sp_all, const int64_t* soff,
                                                           const int32_t* sc_all, double* w_all, const int32_t* dpos_all, int32_t* levl_all,
                                                           int32_t* levu_all, int32_t* ordl_all, int32_t* ordu_all, int32_t* lvll_all,
                                                           int32_t* lvlu_all, int32_t* entl_all, int32_t* entu_all, int32_t* cur_all,
                                                           int32_t* nlev, long long* sizes, double* udiag_all, unsigned long long* err) {
    __shared__ int part[KR_AI_T], levs[KR_AI_T];
    const int t = threadIdx.x;
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {
        const int lo = xoff[k], b = xoff[k + 1] - lo;
        if (b == 0) {
            if (t == 0) { nlev[2 * k] = 0; nlev[2 * k + 1] = 0; for (int q = 0; q < 4; ++q) sizes[4 * k + q] = 0; }
            continue;
        }
        const int32_t* sp = sp_all + lo + k;
        const int32_t* sc = sc_all + soff[k];
        double* w = w_all + soff[k];
        const int32_t* dpos = dpos_all + lo;
        int32_t* levl = levl_all + lo;
        int32_t* levu = levu_all + lo;
        for (int i = t; i < b; i += KR_AI_T) { levl[i] = 0; levu[i] = 0; }
        __syncthreads();
        if (mode == KRYST_ILU_ILUP0) {                                      // ilup.rs:104-111: l_ij = a_ij / a_jj for stored non-zeros
            for (int i = t; i < b; i += KR_AI_T)
                for (int e = sp[i]; e < sp[i + 1]; ++e) {
                    const int j = sc[e];
                    if (j >= i) break;
                    const double v = w[e];
                    if (v != 0.0) {
                        const int kd = dpos[j];
                        const double ujj = kd >= 0 ? w[kd] : 0.0;           // a diagonal is never written here
                        if (ujj == 0.0) { atomicMin(err, ((unsigned long long)k << 28) | ((unsigned long long)i << 14) | (unsigned long long)j); break; }
                        w[e] = v / ujj;
                    }
                }
        } else {                                                            // IKJ on the pattern; levu serves as the rounds' marks
            int round = 0;
            for (;;) {
                ++round;
                int pending = 0;
                for (int i = t; i < b; i += KR_AI_T) {
                    if (levu[i] != 0) continue;
                    bool ready = true;
                    for (int e = sp[i]; e < sp[i + 1] && ready; ++e) {
                        const int c = sc[e];
                        if (c >= i) break;
                        const int lc = levu[c];
                        ready = lc != 0 && lc < round;
                    }
                    if (!ready) { pending = 1; continue; }
                    const int rb = sp[i], re = sp[i + 1];
                    for (int e = rb; e < re; ++e) {
                        const int c = sc[e];
                        if (c >= i) break;
                        const int kd = dpos[c];
                        if (kd < 0 || w[kd] == 0.0) { atomicMin(err, ((unsigned long long)k << 28) | ((unsigned long long)i << 14) | (unsigned long long)c); break; }
                        const double wk = w[e] / w[kd];
                        w[e] = wk;
                        for (int kk = sp[c]; kk < sp[c + 1]; ++kk) {
                            const int j = sc[kk];
                            if (j > c) { const int p = ai_find(sc, rb, re - 1, j); if (p >= 0) w[p] = w[p] - wk * w[kk]; }
                        }
                    }
                    levu[i] = round;
                }
                if (__syncthreads_or(pending) == 0) break;
            }
            for (int i = t; i < b; i += KR_AI_T) levu[i] = 0;
        }
        __syncthreads();
        for (int i = t; i < b; i += KR_AI_T) { const int kd = dpos[i]; udiag_all[lo + i] = (kd >= 0 && w[kd] != 0.0) ? w[kd] : 1.0; }
        const int nl = ai_levels<true>(b, sp, sc, w, levl);
        const int nu = ai_levels<false>(b, sp, sc, w, levu);
        long long kl = 0, ku = 0;
        const long long szl = ai_order<true>(b, nl, sp, sc, w, levl, ordl_all + lo, lvll_all + lo + k, entl_all + lo + k, cur_all + lo + k, part, levs, &kl);
        const long long szu = ai_order<false>(b, nu, sp, sc, w, levu, ordu_all + lo, lvlu_all + lo + k, entu_all + lo + k, cur_all + lo + k, part, levs, &ku);
        if (t == 0) {
            nlev[2 * k] = nl; nlev[2 * k + 1] = nu;
            sizes[4 * k] = szl; sizes[4 * k + 1] = szu; sizes[4 * k + 2] = kl; sizes[4 * k + 3] = ku;
        }
        __syncthreads();
    }
}

// the kept entries of every row into the padded entry-major layout of its level
template <bool LOWER>
__device__ inline void ai_fill(int b, const int32_t* sp, const int32_t* sc, const double* w, const int32_t* lev, const int32_t* ord, const int32_t* lvl,
                               const int32_t* ent, unsigned short* fcol, double* fval) {
    for (int q = threadIdx.x; q < b; q += KR_AI_T) {
        const int i = ord[q], l = lev[i] - 1, q0 = lvl[l], m = lvl[l + 1] - q0, ml = (ent[l + 1] - ent[l]) / m;
        int64_t o = (int64_t)ent[l] + (q - q0);
        int len = 0;
        for (int e = sp[i]; e < sp[i + 1]; ++e) {
            const int j = sc[e];
            if ((LOWER ? j < i : j > i) && w[e] != 0.0) { fcol[o] = (unsigned short)j; fval[o] = w[e]; o += m; ++len; }
        }
        for (; len < ml; ++len) { fcol[o] = KR_AI_PAD; fval[o] = 0.0; o += m; }
    }
}

__global__ __launch_bounds__(KR_AI_T) void ai_fill_kernel(const int32_t* xoff, int64_t nsub, const int32_t* sp_all, const int64_t* soff, const int32_t* sc_all,
                                                         const double* w_all, const int32_t* levl_all, const int32_t* levu_all, const int32_t* ordl_all,
                                                         const int32_t* ordu_all, const int32_t* lvll_all, const int32_t* lvlu_all,
                                                         const int32_t* entl_all, const int32_t* entu_all, const int64_t* loff, const int64_t* uoff,
                                                         unsigned short* lcol, double* lval, unsigned short* ucol, double* uval) {
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {
        const int lo = xoff[k], b = xoff[k + 1] - lo;
        const int32_t* sp = sp_all + lo + k;
        const int32_t* sc = sc_all + soff[k];
        const double* w = w_all + soff[k];
        ai_fill<true>(b, sp, sc, w, levl_all + lo, ordl_all + lo, lvll_all + lo + k, entl_all + lo + k, lcol + loff[k], lval + loff[k]);
        ai_fill<false>(b, sp, sc, w, levu_all + lo, ordu_all + lo, lvlu_all + lo + k, entu_all + lo + k, ucol + uoff[k], uval + uoff[k]);
    }
}

// ---------------------------------------------------------------- apply
constexpr int KR_AI_PRE = 4;        // entries per row that a lane holds in registers one level ahead

// the row of lane t in the level of rows [q0, q1) and entries [e0, e1), loaded ahead of its turn: nothing here depends on y.  false: the
// level is wider than the workgroup or its rows are longer than KR_AI_PRE, and is read when its turn comes.
template <bool UPPER>
__device__ __forceinline__ bool ai_fetch(int q0, int q1, int e0, int e1, const int32_t* ord, const unsigned short* fc, const double* fv, const double* ud,
                                         int& i, unsigned short (&c)[KR_AI_PRE], double (&v)[KR_AI_PRE], double& d) {
    const int t = threadIdx.x, m = q1 - q0, ml = m > 0 ? (e1 - e0) / m : 0;
    if (m > KR_AI_T || ml > KR_AI_PRE) return false;
    if (t < m) {
        i = ord[q0 + t];
#pragma unroll
        for (int e = 0; e < KR_AI_PRE; ++e) {
            c[e] = KR_AI_PAD;
            if (e < ml) { c[e] = fc[e0 + e * m + t]; v[e] = fv[e0 + e * m + t]; }
        }
        if (UPPER) d = ud[i];
    }
    return true;
}

// one sweep over the levels [first, nl): y[i] = y[i] - f_ij y[j] over the kept entries in ascending j (UPPER: then / u_ii), a workgroup
// barrier after every level.  The level tables are read two levels ahead and the next level's rows and entries one level ahead, so that a
// level's own work is LDS arithmetic between two barriers.
template <bool UPPER>
__device__ __forceinline__ void ai_sweep(double* y, int first, int nl, const int32_t* ord, const int32_t* lvl, const int32_t* ent,
                                         const unsigned short* fc, const double* fv, const double* ud) {
    if (first >= nl) return;
    const int t = threadIdx.x;
    int q0 = lvl[first], q1 = lvl[first + 1], e0 = ent[first], e1 = ent[first + 1];
    int q2 = q1, e2 = e1;
    if (first + 1 < nl) { q2 = lvl[first + 2]; e2 = ent[first + 2]; }
    int ci = 0, ni = 0;
    unsigned short cc[KR_AI_PRE], nc[KR_AI_PRE];
    double cv[KR_AI_PRE], nv[KR_AI_PRE], cd = 1.0, nd = 1.0;
#pragma unroll
    for (int e = 0; e < KR_AI_PRE; ++e) { cc[e] = nc[e] = KR_AI_PAD; cv[e] = nv[e] = 0.0; }
    bool cfast = ai_fetch<UPPER>(q0, q1, e0, e1, ord, fc, fv, ud, ci, cc, cv, cd);
    for (int l = first; l < nl; ++l) {                                      // uniform over the workgroup
        int q3 = q2, e3 = e2;
        if (l + 2 < nl) { q3 = lvl[l + 3]; e3 = ent[l + 3]; }
        bool nfast = false;
        if (l + 1 < nl) nfast = ai_fetch<UPPER>(q1, q2, e1, e2, ord, fc, fv, ud, ni, nc, nv, nd);
        const int m = q1 - q0;
        if (cfast) {
            if (t < m) {
                double s = y[ci];
#pragma unroll
                for (int e = 0; e < KR_AI_PRE; ++e)
                    if (cc[e] != KR_AI_PAD) s = s - cv[e] * y[cc[e]];
                y[ci] = UPPER ? s / cd : s;
            }
        } else {
            const int ml = (e1 - e0) / m;
            for (int q = t; q < m; q += KR_AI_T) {
                const int i = ord[q0 + q];
                double s = y[i];
                for (int e = 0; e < ml; ++e) {
                    const unsigned short c = fc[e0 + (int64_t)e * m + q];
                    if (c != KR_AI_PAD) s = s - fv[e0 + (int64_t)e * m + q] * y[c];
                }
                y[i] = UPPER ? s / ud[i] : s;
            }
        }
        __syncthreads();
        q0 = q1; q1 = q2; q2 = q3; e0 = e1; e1 = e2; e2 = e3;
        ci = ni; cd = nd; cfast = nfast;
#pragma unroll
        for (int e = 0; e < KR_AI_PRE; ++e) { cc[e] = nc[e]; cv[e] = nv[e]; }
    }
}

// y = r[g] in LDS; forward: y[i] = y[i] - l_ij y[j] over the kept entries in ascending j, level after level (the first level reads nothing);
// backward: the same with u_ij, then y[i] = s / u_ii (udiag holds 1.0 where no non-zero diagonal is stored: s / 1.0 is s); X[off_k + i] =
// y[i].  Every slot of y that is read was written by the gather.
__global__ __launch_bounds__(KR_AI_T) void ai_apply_kernel(const int32_t* xoff, const int32_t* idx, int64_t nsub, const int32_t* nlev,
                                                          const int32_t* ordl_all, const int32_t* ordu_all, const int32_t* lvll_all,
                                                          const int32_t* lvlu_all, const int32_t* entl_all, const int32_t* entu_all,
                                                          const int64_t* loff, const int64_t* uoff, const unsigned short* lcol, const double* lval,
                                                          const unsigned short* ucol, const double* uval, const double* udiag, const double* r,
                                                          double* X, const int* done) {
    if (done && *done) return;
    extern __shared__ double ai_y[];
    const int t = threadIdx.x;
    for (int64_t k = blockIdx.x; k < nsub; k += gridDim.x) {                 // uniform over the workgroup
        const int lo = xoff[k], b = xoff[k + 1] - lo;
        const int nl = nlev[2 * k], nu = nlev[2 * k + 1];
        for (int i = t; i < b; i += KR_AI_T) ai_y[i] = r[idx[lo + i]];
        __syncthreads();
        ai_sweep<false>(ai_y, 1, nl, ordl_all + lo, lvll_all + lo + k, entl_all + lo + k, lcol + loff[k], lval + loff[k], udiag + lo);
        ai_sweep<true>(ai_y, 0, nu, ordu_all + lo, lvlu_all + lo + k, entu_all + lo + k, ucol + uoff[k], uval + uoff[k], udiag + lo);
        for (int i = t; i < b; i += KR_AI_T) X[lo + i] = ai_y[i];
        __syncthreads();                                                    // the next subdomain reuses the LDS
    }
}

// the (grown) subdomains sorted ascending, S_k with the factor values in its place, the level-ordered factors, X and the combine's map
struct AsmIluPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_ASM_ILU;
    int64_t nsub = 0, total = 0, nnz_s = 0, nnz_l = 0, nnz_u = 0, pad_l = 0, pad_u = 0;
    int32_t maxb = 0, maxlev = 0;
    unsigned grid = 1;
    size_t lds = 0;
    int32_t* d_xoff = nullptr; int32_t* d_idx = nullptr; int32_t* d_mptr = nullptr; int32_t* d_mpos = nullptr; double* d_x = nullptr;
    int32_t* d_sp = nullptr; int64_t* d_soff = nullptr; int32_t* d_sc = nullptr; double* d_w = nullptr; int32_t* d_dpos = nullptr;
    int32_t* d_levl = nullptr; int32_t* d_levu = nullptr; int32_t* d_ordl = nullptr; int32_t* d_ordu = nullptr;
    int32_t* d_lvll = nullptr; int32_t* d_lvlu = nullptr; int32_t* d_entl = nullptr; int32_t* d_entu = nullptr; int32_t* d_nlev = nullptr;
    int64_t* d_loff = nullptr; int64_t* d_uoff = nullptr;
    unsigned short* d_lcol = nullptr; unsigned short* d_ucol = nullptr; double* d_lval = nullptr; double* d_uval = nullptr; double* d_udiag = nullptr;
    std::vector<int64_t> ptr_h, soff_h; std::vector<int32_t> idx_h, owner_h;
    AsmIluPc(kryst_csr_t a_, int64_t nsub_, int64_t total_, int32_t maxb_) : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows), nsub(nsub_), total(total_), maxb(maxb_) {}
    ~AsmIluPc() override {
        for (void* p : {(void*)d_xoff, (void*)d_idx, (void*)d_mptr, (void*)d_mpos, (void*)d_x, (void*)d_sp, (void*)d_soff, (void*)d_sc, (void*)d_w, (void*)d_dpos,
                        (void*)d_levl, (void*)d_levu, (void*)d_ordl, (void*)d_ordu, (void*)d_lvll, (void*)d_lvlu, (void*)d_entl, (void*)d_entu, (void*)d_nlev,
                        (void*)d_loff, (void*)d_uoff, (void*)d_lcol, (void*)d_ucol, (void*)d_lval, (void*)d_uval, (void*)d_udiag}) (void)pool_free(p);
    }
    int32_t apply(int64_t nv, const double* r, double* z, const int* done) override;
};

int32_t AsmIluPc::apply(int64_t, const double* r, double* z, const int* done) {
    if (total > 0) {
        hipLaunchKernelGGL(ai_apply_kernel, dim3(grid), dim3(KR_AI_T), lds, ctx->s_main, (const int32_t*)d_xoff, (const int32_t*)d_idx, nsub,
                           (const int32_t*)d_nlev, (const int32_t*)d_ordl, (const int32_t*)d_ordu, (const int32_t*)d_lvll, (const int32_t*)d_lvlu,
                           (const int32_t*)d_entl, (const int32_t*)d_entu, (const int64_t*)d_loff, (const int64_t*)d_uoff,
                           (const unsigned short*)d_lcol, (const double*)d_lval, (const unsigned short*)d_ucol, (const double*)d_uval,
                           (const double*)d_udiag, r, d_x, done);
        KR_HIP(hipGetLastError());
    }
    return asm_combine_launch(ctx, d_mptr, d_mpos, d_x, n, z, done);
}

template <class T> static int32_t ai_alloc(T** d, size_t count, const char* what) {
    if (pool_malloc(d, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) {
        (void)hipGetLastError();
        *d = nullptr;
        set_error("additive Schwarz: out of device memory (%s)", what);
        return KRYST_ERR_HIP;
    }
    return KRYST_OK;
}

// the bytes kept on the device: per subdomain row (idx, X, dpos, two levels, two orders, four level tables, the diagonal), per subdomain, per
// row of A and map entry (the combine's map), per stored entry of the submatrices (column, value), per entry of the padded layouts
static unsigned long long ai_bytes(int64_t n, int64_t nsub, unsigned long long rows, unsigned long long m, unsigned long long nnz_s, unsigned long long pad) {
    return (4ull + 8ull + 4ull + 8ull + 8ull + 16ull + 4ull + 8ull) * rows + (4ull + 8ull + 8ull + 16ull + 20ull) * (unsigned long long)(nsub + 1) +
           4ull * (unsigned long long)(n + 1) + 4ull * m + 12ull * nnz_s + 10ull * pad;
}

static int32_t ai_build(AsmIluPc* pc, int32_t mode, const std::vector<int32_t>& mptr, const std::vector<int32_t>& mpos) {
    kryst_ctx_t ctx = pc->ctx;
    kryst_csr_t a = pc->a;
    const int64_t nsub = pc->nsub, total = pc->total, n = pc->n;
    std::vector<int32_t> xoff((size_t)nsub + 1);
    for (int64_t k = 0; k <= nsub; ++k) xoff[(size_t)k] = (int32_t)pc->ptr_h[(size_t)k];
    KR_TRY(asm_upload(ctx, &pc->d_xoff, xoff, "subdomain offsets"));
    KR_TRY(asm_upload(ctx, &pc->d_idx, pc->idx_h, "index sets"));
    KR_TRY(asm_upload(ctx, &pc->d_mptr, mptr, "row map"));
    KR_TRY(asm_upload(ctx, &pc->d_mpos, mpos, "row map"));
    const size_t rows = (size_t)total, slots = (size_t)(total + nsub);
    KR_TRY(ai_alloc(&pc->d_x, rows, "subdomain rows"));
    KR_TRY(ai_alloc(&pc->d_sp, slots, "submatrix rows"));
    KR_TRY(ai_alloc(&pc->d_dpos, rows, "submatrix rows"));
    KR_TRY(ai_alloc(&pc->d_levl, rows, "levels"));
    KR_TRY(ai_alloc(&pc->d_levu, rows, "levels"));
    KR_TRY(ai_alloc(&pc->d_ordl, rows, "levels"));
    KR_TRY(ai_alloc(&pc->d_ordu, rows, "levels"));
    KR_TRY(ai_alloc(&pc->d_lvll, slots, "levels"));
    KR_TRY(ai_alloc(&pc->d_lvlu, slots, "levels"));
    KR_TRY(ai_alloc(&pc->d_entl, slots, "levels"));
    KR_TRY(ai_alloc(&pc->d_entu, slots, "levels"));
    KR_TRY(ai_alloc(&pc->d_nlev, 2 * (size_t)nsub, "levels"));
    KR_TRY(ai_alloc(&pc->d_udiag, rows, "diagonal"));
    if (nsub == 0 || total == 0) {
        pc->soff_h.assign((size_t)nsub + 1, 0);
        return KRYST_OK;
    }
    int32_t* d_cur = nullptr; int64_t* d_cnt = nullptr; long long* d_sizes = nullptr; unsigned long long* d_err = nullptr;
    int32_t rc = KRYST_OK;
    auto fail_hip = [&](const char* what) { set_error("additive Schwarz: %s", what); rc = KRYST_ERR_HIP; };
    do {
        if ((rc = ai_alloc(&d_cur, slots, "set-up scratch")) != KRYST_OK) break;
        if ((rc = ai_alloc(&d_cnt, (size_t)nsub, "set-up scratch")) != KRYST_OK) break;
        if ((rc = ai_alloc(&d_sizes, 4 * (size_t)nsub, "set-up scratch")) != KRYST_OK) break;
        if ((rc = ai_alloc(&d_err, 1, "set-up scratch")) != KRYST_OK) break;
        if (hipMemsetAsync(d_err, 0xFF, sizeof(unsigned long long), ctx->s_main) != hipSuccess) { fail_hip("set-up failed on the device"); break; }
        const dim3 grid(pc->grid), block(KR_AI_T);
        hipLaunchKernelGGL(ai_extract_kernel, grid, block, 0, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, (const int32_t*)pc->d_xoff,
                           (const int32_t*)pc->d_idx, nsub, 0, pc->d_sp, d_cnt, (const int64_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, (int32_t*)nullptr);
        std::vector<int64_t> cnt((size_t)nsub);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { fail_hip("set-up failed on the device (counting the submatrices)"); break; }
        pc->soff_h.assign((size_t)nsub + 1, 0);
        for (int64_t k = 0; k < nsub; ++k) pc->soff_h[(size_t)k + 1] = pc->soff_h[(size_t)k] + cnt[(size_t)k];
        pc->nnz_s = pc->soff_h.back();
        if ((rc = asm_check_memory(ctx->device, ai_bytes(n, nsub, (unsigned long long)total, mpos.size(), (unsigned long long)pc->nnz_s, 0))) != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &pc->d_soff, pc->soff_h, "submatrix offsets")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_sc, (size_t)pc->nnz_s, "submatrix entries")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_w, (size_t)pc->nnz_s, "submatrix entries")) != KRYST_OK) break;
        hipLaunchKernelGGL(ai_extract_kernel, grid, block, 0, ctx->s_main, a->d_row_ptr, a->d_col, a->d_val, (const int32_t*)pc->d_xoff,
                           (const int32_t*)pc->d_idx, nsub, 1, pc->d_sp, d_cnt, (const int64_t*)pc->d_soff, pc->d_sc, pc->d_w, pc->d_dpos);
        hipLaunchKernelGGL(ai_factor_kernel, grid, block, 0, ctx->s_main, (const int32_t*)pc->d_xoff, nsub, (int)mode, (const int32_t*)pc->d_sp,
                           (const int64_t*)pc->d_soff, (const int32_t*)pc->d_sc, pc->d_w, (const int32_t*)pc->d_dpos, pc->d_levl, pc->d_levu, pc->d_ordl,
                           pc->d_ordu, pc->d_lvll, pc->d_lvlu, pc->d_entl, pc->d_entu, d_cur, pc->d_nlev, d_sizes, pc->d_udiag, d_err);
        std::vector<long long> sizes(4 * (size_t)nsub);
        std::vector<int32_t> nlev(2 * (size_t)nsub);
        unsigned long long e = KR_AI_NOERR;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&e, d_err, sizeof e, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipMemcpyAsync(sizes.data(), d_sizes, sizeof(long long) * sizes.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipMemcpyAsync(nlev.data(), pc->d_nlev, sizeof(int32_t) * nlev.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { fail_hip("set-up failed on the device (factorising the submatrices)"); break; }
        if (e != KR_AI_NOERR) {                                             // the lowest subdomain, its lowest row, that row's first pivot
            const int64_t k = (int64_t)(e >> 28);
            const int64_t row = (int64_t)pc->idx_h[(size_t)(pc->ptr_h[(size_t)k] + (int64_t)(e & 0x3FFFull))];
            set_error_row(row);
            if (mode == KRYST_ILU_TRUE_ILU0) { set_error("ILU(0): zero pivot at row %lld (additive Schwarz: subdomain %lld)", (long long)row, (long long)k); rc = KRYST_ZERO_PIVOT; }
            else { set_error("ILUP: zero diagonal in U at row %lld (additive Schwarz: subdomain %lld)", (long long)row, (long long)k); rc = KRYST_SOLVE_ERROR; }
            break;
        }
        std::vector<int64_t> loff((size_t)nsub + 1, 0), uoff((size_t)nsub + 1, 0);
        for (int64_t k = 0; k < nsub && rc == KRYST_OK; ++k) {
            const long long sl = sizes[4 * (size_t)k], su = sizes[4 * (size_t)k + 1];
            if (sl < 0 || su < 0) {
                set_error("additive Schwarz: the level layout of subdomain %lld has more than 2^31 - 1 entries", (long long)k);
                rc = KRYST_UNSUPPORTED; break;
            }
            loff[(size_t)k + 1] = loff[(size_t)k] + sl; uoff[(size_t)k + 1] = uoff[(size_t)k] + su;
            pc->nnz_l += sizes[4 * (size_t)k + 2]; pc->nnz_u += sizes[4 * (size_t)k + 3];
            pc->maxlev = std::max(pc->maxlev, std::max(nlev[2 * (size_t)k], nlev[2 * (size_t)k + 1]));
        }
        if (rc != KRYST_OK) break;
        pc->pad_l = loff.back(); pc->pad_u = uoff.back();
        if ((rc = asm_check_memory(ctx->device, ai_bytes(n, nsub, (unsigned long long)total, mpos.size(), (unsigned long long)pc->nnz_s,
                                                       (unsigned long long)(pc->pad_l + pc->pad_u)))) != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &pc->d_loff, loff, "factor offsets")) != KRYST_OK) break;
        if ((rc = asm_upload(ctx, &pc->d_uoff, uoff, "factor offsets")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_lcol, (size_t)pc->pad_l, "factor entries")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_lval, (size_t)pc->pad_l, "factor entries")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_ucol, (size_t)pc->pad_u, "factor entries")) != KRYST_OK) break;
        if ((rc = ai_alloc(&pc->d_uval, (size_t)pc->pad_u, "factor entries")) != KRYST_OK) break;
        hipLaunchKernelGGL(ai_fill_kernel, grid, block, 0, ctx->s_main, (const int32_t*)pc->d_xoff, nsub, (const int32_t*)pc->d_sp, (const int64_t*)pc->d_soff,
                           (const int32_t*)pc->d_sc, (const double*)pc->d_w, (const int32_t*)pc->d_levl, (const int32_t*)pc->d_levu, (const int32_t*)pc->d_ordl,
                           (const int32_t*)pc->d_ordu, (const int32_t*)pc->d_lvll, (const int32_t*)pc->d_lvlu, (const int32_t*)pc->d_entl,
                           (const int32_t*)pc->d_entu, (const int64_t*)pc->d_loff, (const int64_t*)pc->d_uoff, pc->d_lcol, pc->d_lval, pc->d_ucol, pc->d_uval);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) { fail_hip("set-up failed on the device (laying out the factors)"); break; }
    } while (0);
    (void)pool_free(d_cur); (void)pool_free(d_cnt); (void)pool_free(d_sizes); (void)pool_free(d_err);
    return rc;
}

static int32_t ai_setup(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant, int32_t mode,
                        kryst_pc_t* out) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t n = a->nrows;
    AsmSets sets;
    KR_TRY(asm_sort_sets(a, sub_ptr, sub_idx, nsub, KR_AI_MAX, sets));
    KR_HIP(hipSetDevice(ctx->device));
    // the un-grown sets bound the grown ones from below: a request that cannot fit fails before anything is allocated
    KR_TRY(asm_check_memory(ctx->device, ai_bytes(n, nsub, (unsigned long long)sets.ptr.back(), (unsigned long long)sets.ptr.back(), 0, 0)));
    if (variant != KRYST_ASM_AS_WRITTEN) KR_TRY(asm_grow(a, overlap, sets.ptr, sets.idx, KR_AI_MAX));
    int bmax = 0;
    for (int64_t k = 0; k < nsub; ++k) bmax = std::max(bmax, (int)(sets.ptr[(size_t)k + 1] - sets.ptr[(size_t)k]));
    std::vector<int32_t> mptr, mpos;
    asm_row_map(n, variant, sets, mptr, mpos);
    KR_TRY(asm_check_memory(ctx->device, ai_bytes(n, nsub, (unsigned long long)sets.ptr.back(), mpos.size(), 0, 0)));
    const size_t lds = sizeof(double) * (size_t)std::max(bmax, 1);
    if (lds > 64 * 1024) {                                                  // the device's own limit, raised for this kernel on this device
        int lds_max = 0;
        KR_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
        if (lds > (size_t)lds_max) {
            set_error("additive Schwarz: subdomains of %d rows need %zu bytes of LDS per workgroup; the device has %d", bmax, lds, lds_max);
            return KRYST_UNSUPPORTED;
        }
        KR_HIP(hipFuncSetAttribute((const void*)ai_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    AsmIluPc* pc = new AsmIluPc(a, nsub, sets.ptr.back(), bmax);
    pc->lds = lds;
    pc->grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nsub, 8 * (int64_t)std::max(ctx->num_cu, 1)));
    pc->ptr_h = std::move(sets.ptr); pc->idx_h = std::move(sets.idx); pc->owner_h = std::move(sets.owner);
    const int32_t rc = ai_build(pc, mode, mptr, mpos);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

static int32_t ai_check(kryst_csr_t a, int32_t overlap, int32_t variant, int32_t mode) {
    KR_TRY(asm_check(a, overlap, variant));
    if (a->ctx->nranks > 1) { set_error("additive Schwarz with ILU sub-solves: a context of several ranks is not supported"); return KRYST_UNSUPPORTED; }
    if (mode == KRYST_ILU_KRYST_COMPAT) { set_error("additive Schwarz with ILU sub-solves: KRYST_ILU_KRYST_COMPAT is not supported (ILUP0 or TRUE_ILU0)"); return KRYST_UNSUPPORTED; }
    KR_ARG(mode == KRYST_ILU_ILUP0 || mode == KRYST_ILU_TRUE_ILU0, "pc_asm_ilu: unknown sub_mode");
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_pc_asm_ilu(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant, int32_t sub_mode,
                         kryst_pc_t* out) {
    KR_ARG(a && out && nsub >= 0 && (sub_ptr || nsub == 0), "pc_asm_ilu");
    KR_TRY(ai_check(a, overlap, variant, sub_mode));
    return ai_setup(a, sub_ptr, sub_idx, nsub, overlap, variant, sub_mode, out);
}

int32_t kryst_pc_asm_ilu_uniform(kryst_csr_t a, int64_t nparts, int32_t overlap, int32_t variant, int32_t sub_mode, kryst_pc_t* out) {
    KR_ARG(a && out && nparts >= 0, "pc_asm_ilu_uniform");
    KR_TRY(ai_check(a, overlap, variant, sub_mode));
    std::vector<int64_t> ptr, idx;
    asm_uniform_sets(a->nrows, nparts, ptr, idx);
    return ai_setup(a, ptr.data(), idx.data(), (int64_t)ptr.size() - 1, overlap, variant, sub_mode, out);
}

int32_t kryst_pc_asm_ilu_info(kryst_pc_t h, int64_t* info, int32_t count) {
    AsmIluPc* pc = pc_cast<AsmIluPc>(h);
    KR_ARG(pc && info && count >= 0, "pc_asm_ilu_info");
    const int64_t v[KRYST_ASM_ILU_INFO_COUNT] = {pc->nsub, pc->total, pc->maxb, pc->nnz_l, pc->nnz_u, pc->maxlev, (int64_t)pc->lds, KR_AI_MAX,
                                                 pc->nnz_s, pc->pad_l + pc->pad_u};
    for (int32_t i = 0; i < count && i < KRYST_ASM_ILU_INFO_COUNT; ++i) info[i] = v[i];
    return KRYST_OK;
}

int32_t kryst_pc_asm_ilu_export(kryst_pc_t h, int64_t* sub_ptr, int32_t* sub_idx, int32_t* owner, int64_t* ent_ptr, int32_t* row_ptr, int32_t* col,
                                double* val, int32_t* lev_l, int32_t* lev_u) {
    AsmIluPc* pc = pc_cast<AsmIluPc>(h);
    KR_ARG(pc, "pc_asm_ilu_export");
    if (sub_ptr) std::copy(pc->ptr_h.begin(), pc->ptr_h.end(), sub_ptr);
    if (sub_idx) std::copy(pc->idx_h.begin(), pc->idx_h.end(), sub_idx);
    if (owner) std::copy(pc->owner_h.begin(), pc->owner_h.end(), owner);
    if (ent_ptr) std::copy(pc->soff_h.begin(), pc->soff_h.end(), ent_ptr);
    KR_HIP(hipSetDevice(pc->ctx->device));
    hipStream_t s = pc->ctx->s_main;
    const size_t rows = (size_t)pc->total, slots = (size_t)(pc->total + pc->nsub), nz = (size_t)pc->nnz_s;
    if (row_ptr && slots > 0 && rows > 0) KR_HIP(hipMemcpyAsync(row_ptr, pc->d_sp, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, s));
    else if (row_ptr) std::fill(row_ptr, row_ptr + slots, 0);
    if (col && nz > 0) KR_HIP(hipMemcpyAsync(col, pc->d_sc, sizeof(int32_t) * nz, hipMemcpyDeviceToHost, s));
    if (val && nz > 0) KR_HIP(hipMemcpyAsync(val, pc->d_w, sizeof(double) * nz, hipMemcpyDeviceToHost, s));
    if (lev_l && rows > 0) KR_HIP(hipMemcpyAsync(lev_l, pc->d_levl, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, s));
    if (lev_u && rows > 0) KR_HIP(hipMemcpyAsync(lev_u, pc->d_levu, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, s));
    KR_HIP(hipStreamSynchronize(s));
    return KRYST_OK;
}

}  // extern "C"
