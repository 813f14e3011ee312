// Mixed precision on the row-pattern encoding: the two SpMV kernels of a lowered operator that keeps a CSR-P16 form --
// spmv32_pattern_kernel (any CSR-P16 operator) and spmv32_pattern_stage_kernel (boxes of lines: the near operands staged in LDS) -- and their
// enqueue functions, and the lowering of the form (when an operator can take it, its arrays and fields).  mixed_lower.hip has the skeleton of the
// lowering, mixed_spmv.hip the choice (spmv32_kernel), mixed_cg.hip the solvers; spmv_pattern.hip has the fp64 twins.
//
// The contract of both: the fp32 tile of 1024 rows, thread t owns rows 4t .. 4t+3 (ids: one 8-byte load; y: one 16-byte store).  y_i = (float) of
// the fold from 0.0, in stored order, of (double)tableval * (double)x[col] with separate multiply and add; an absent entry is skipped by a select,
// never multiplied; rows at or beyond nrows are not stored.  nq = 1: partials[tile] = the tile partial of sum d_i * y_i (y as stored) in the fp32
// tree -- the lane's four terms in index order from 0.0, the 64-lane butterfly, the 4 waves in turn.  A table value is (float) of the fp64 table
// value, i.e. bit for bit the lowered CSR value of every row that uses it, so the bits are spmv32_wave_kernel's.
#include "mixed.h"

namespace kr {

typedef unsigned p_v2u __attribute__((ext_vector_type(2)));

struct Spmv32PatArgs {
    const uint16_t* pid; const uint32_t* pmeta; const int32_t* poff; const float* pval;
    const float* x; float* y; const float* dvec; double* partials; const int* done;
    int32_t nrows, ntiles, npat, ntab, tpw;
    int32_t xcap;                   // allocated floats of x (vec32_len(ncols)): a 16-byte gather must end inside it
    int32_t red_off;                // byte offset of the reduction scratch in dynamic LDS
};

// ---------------------------------------------------------------------------------------------------- any CSR-P16 operator
// The tables go to LDS once per workgroup; the workgroup walks a run of tpw consecutive tiles with the next tile's ids prefetched.  When the lane's
// four rows share a base (interior rows and the boundary rows next to them do), entry e of all four reads x[4t + off_e .. 4t + off_e + 3] -- one
// 16-byte gather at 4-byte alignment and one table lookup for four rows, each row's presence bit selecting.  Rows with different bases walk their
// own, one entry at a time (kept small, as in spmv_pattern_kernel).  A quad that would start before x[0] or end behind x's allocation takes a
// per-element path (wave-uniform branch).  Bases longer than U entries loop.
template <int NQ, int U>
__global__ __launch_bounds__(KR32_T) void spmv32_pattern_kernel(const Spmv32PatArgs a) {
    static_assert(NQ == 0 || NQ == 1, "NQ");
    if (a.done && *a.done) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    p_v2u* meta = reinterpret_cast<p_v2u*>(smem);                                      // npat
    int32_t* poff = reinterpret_cast<int32_t*>(meta + a.npat);                         // ntab + U
    float* pval = reinterpret_cast<float*>(poff + a.ntab + U);                         // ntab + U
    double* red = reinterpret_cast<double*>(smem + a.red_off);
    const int t = threadIdx.x;
    const int li0 = blockIdx.x * a.tpw, li_end = min(li0 + a.tpw, a.ntiles);
    p_v2u ids = *reinterpret_cast<const p_v2u*>(a.pid + (size_t)li0 * KR32_TILE + 4 * t);    // (on their way while the tables are copied)
    for (int i = t; i < a.npat; i += KR32_T) meta[i] = reinterpret_cast<const p_v2u*>(a.pmeta)[i];
    for (int i = t; i < a.ntab + U; i += KR32_T) { poff[i] = i < a.ntab ? a.poff[i] : 0; pval[i] = i < a.ntab ? a.pval[i] : 0.0f; }
    __syncthreads();
    for (int q = li0; q < li_end; ++q) {
        p_v2u ids_n; ids_n.x = 0u; ids_n.y = 0u;
        if (q + 1 < li_end) ids_n = *reinterpret_cast<const p_v2u*>(a.pid + (size_t)(q + 1) * KR32_TILE + 4 * t);
        const int32_t row = q * KR32_TILE + 4 * t;
        const unsigned id[4] = {ids.x & 0xffffu, ids.x >> 16, ids.y & 0xffffu, ids.y >> 16};
        bool valid[4]; p_v2u m[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            valid[r] = row + r < a.nrows;
            m[r].x = 0u; m[r].y = 0u;
            if (valid[r]) m[r] = meta[id[r]];
        }
        // rows behind the last one take the base of the lane's first row with nothing present, so that the last quad stays on the shared path
#pragma unroll
        for (int r = 1; r < 4; ++r) { if (!valid[r]) m[r].x = m[0].x; }
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (m[0].x == m[1].x && m[0].x == m[2].x && m[0].x == m[3].x) {
            const int len = m[0].x >> 16;
            const float* tv = pval + (m[0].x & 0xffffu); const int32_t* to = poff + (m[0].x & 0xffffu);
            for (int e0 = 0; e0 < len; e0 += U) {
                // masks of the entries e0 .. e0+U-1 (a mask has no bits at or beyond the base length; a base longer than 16 entries has no
                // sub-patterns: every valid row has all of it)
                const unsigned lim = (len - e0 >= 32) ? 0xffffffffu : ((1u << (len - e0)) - 1u);
                unsigned k[4], kk = 0u;
#pragma unroll
                for (int r = 0; r < 4; ++r) { k[r] = (e0 < 16 ? (m[r].y >> e0) : (valid[r] ? 0xffffffffu : 0u)) & lim; kk |= k[r]; }
                int32_t c[U];
                bool odd = false;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    c[u] = ((kk >> u) & 1u) ? row + to[e0 + u] : 0;                  // nobody needs it: x[0 .. 3], always allocated
                    odd = odd || c[u] < 0 || c[u] + 4 > a.xcap;
                }
                p_v4f xx[U];
                if (__builtin_amdgcn_ballot_w64(odd) != 0) {
                    // rare: some lane's quad starts before x[0] (its first rows lack the entry) or would end behind the allocation
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int r = 0; r < 4; ++r) { if ((k[r] >> u) & 1u) e[r] = a.x[c[u] + r]; }
                        xx[u].x = e[0]; xx[u].y = e[1]; xx[u].z = e[2]; xx[u].w = e[3];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) xx[u] = *reinterpret_cast<const p_v4f_a4*>(a.x + c[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double v = (double)tv[e0 + u];
                    const double t0 = s[0] + v * (double)xx[u].x, t1 = s[1] + v * (double)xx[u].y;
                    const double t2 = s[2] + v * (double)xx[u].z, t3 = s[3] + v * (double)xx[u].w;
                    s[0] = ((k[0] >> u) & 1u) ? t0 : s[0];
                    s[1] = ((k[1] >> u) & 1u) ? t1 : s[1];
                    s[2] = ((k[2] >> u) & 1u) ? t2 : s[2];
                    s[3] = ((k[3] >> u) & 1u) ? t3 : s[3];
                }
            }
        } else {
            // ---- different bases (adjacent rows built from unrelated stencils): each row walks its own, one entry at a time
            int len[4], maxlen = 0;
            const float* tv[4]; const int32_t* to[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                len[r] = valid[r] ? (int)(m[r].x >> 16) : 0;
                maxlen = max(maxlen, len[r]);
                tv[r] = pval + (m[r].x & 0xffffu); to[r] = poff + (m[r].x & 0xffffu);
            }
#pragma unroll 1
            for (int e = 0; e < maxlen; ++e) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (e < len[r] && (e >= 16 || ((m[r].y >> e) & 1u))) s[r] = s[r] + (double)tv[r][e] * (double)a.x[row + r + to[r][e]];
                }
            }
        }
        quad_finish<NQ>(s, a.y, a.dvec, a.partials, q, row, a.nrows, red);
        ids = ids_n;
    }
}

int32_t enqueue_spmv32_pattern(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nt = ntiles32_of(a->nrows);
    const int U = a->pat_unroll == 7 ? 7 : 8;
    Spmv32PatArgs g{a->d_pid, a->d_pmeta, a->d_poff, a->d_pval, x, y, dvec, ctx->d_partials, done,
                    (int32_t)a->nrows, (int32_t)nt, a->npat, a->ntab, 0, (int32_t)vec32_len(a->ncols), 0};
    // a run of 4 tiles per workgroup amortises the table copy (the fp64 kernel's 8 tiles of 512 rows): taken over, not measured on its own
    g.tpw = std::max(1, std::min(64, env_int("KRYST_SPMV32_PATTERN_TPW", 4)));
    const size_t tab = (size_t)a->npat * 8 + (size_t)(a->ntab + U) * 8;
    g.red_off = (int32_t)((tab + 15) & ~(size_t)15);
    const size_t lds = (size_t)g.red_off + sizeof(double) * (KR32_T / 64);
    const dim3 grid((unsigned)((nt + g.tpw - 1) / g.tpw)), block(KR32_T);
    by_bool(nq != 0, [&](auto Q) { by_int<7, 8>(U, [&](auto U_) { hipLaunchKernelGGL((spmv32_pattern_kernel<Q() ? 1 : 0, U_()>), grid, block, lds, ctx->s_main, g); }); });
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- boxes of lines: near operands from LDS
// spmv_pattern_stage_kernel with UFAR at the fp32 tile.  Every base is (far_lo, -n, -1, 0, +1, +n, far_hi) with n % 4 == 0 and the same far offsets
// everywhere.  A workgroup takes a run of T tiles and requests, together: the run's ids, the far operands of all T tiles (per element, bounds
// checked, where the run is not wholly inside x), the fused dot's vector, and the window x[r0 - n - 4 .. r0 + 1024 T + n + 4) -- straight into LDS
// with global_load_lds_dwordx4 (16 bytes per lane behind a wave-uniform base, which is the window's layout; every source address is 16-byte
// aligned because r0, n and 4 are multiples of 4).  The compiler does not count LDS-DMA requests: an explicit s_waitcnt vmcnt(0) stands before
// the barrier.  Then tile after tile out of LDS: five aligned 16-byte reads give x[row - n .. +3], x[row - 4 .. row + 7], x[row + n .. +3].  The
// cross-wave step of the fused partial of all T tiles meets at one barrier.  LDS: 4 (1024 T + 2 n + 8) bytes of window (at most 8 T + 8 KiB) plus
// the tables.
template <int NQ, int T>
__global__ __launch_bounds__(KR32_T) void spmv32_pattern_stage_kernel(const Spmv32PatArgs a, const int32_t n, const int32_t far_lo, const int32_t far_hi) {
    static_assert(NQ == 0 || NQ == 1, "NQ");
    if (a.done && *a.done) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int XS = T * KR32_TILE + 2 * n + 8;                                  // staged elements (a multiple of 4)
    float* xs = reinterpret_cast<float*>(smem);
    p_v2u* meta = reinterpret_cast<p_v2u*>(xs + XS);
    float* pval = reinterpret_cast<float*>(meta + a.npat);                     // ntab
    double* red = reinterpret_cast<double*>(smem + a.red_off);
    const int t = threadIdx.x;
    const int qr = blockIdx.x * T;                                             // the run's first tile
    if (qr >= a.ntiles) return;                                                // (uniform over the workgroup)
    const int nt = min(T, a.ntiles - qr);
    const int32_t r0 = qr * KR32_TILE;
    // ---- one round trip: ids, window, far operands, the dot's vector, the tables
    p_v2u ids[T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        ids[k].x = 0u; ids[k].y = 0u;
        if (k < nt) ids[k] = *reinterpret_cast<const p_v2u*>(a.pid + (size_t)(qr + k) * KR32_TILE + 4 * t);
    }
    constexpr int NP = (T * KR32_TILE + 2 * 1024 + 8 + 4 * KR32_T - 1) / (4 * KR32_T);       // quads per lane at most (n <= 1024)
    const int nquads = XS / 4;
    const int32_t e0 = r0 - n - 4;                                             // element of x staged at xs[0] (a multiple of 4)
    const int32_t xcap = a.xcap, xlast = a.xcap - 4;
    const bool inside = e0 >= 0 && (int64_t)e0 + XS <= xcap && (int64_t)r0 + far_lo >= 0 && (int64_t)r0 + T * KR32_TILE + far_hi <= (int64_t)xcap;
    const int wbase = __builtin_amdgcn_readfirstlane(t & ~63);
    p_v4f lo[T], hi[T], dv[T];
    if (inside) {
        const float* xw = a.x + e0 + 4 * t;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (t + i * KR32_T < nquads)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xw + 4 * i * KR32_T),
                                                 (__attribute__((address_space(3))) void*)(xs + 4 * (i * KR32_T + wbase)), 16, 0, 0);
        }
        const float* xl = a.x + (r0 + 4 * t) + far_lo; const float* xh = a.x + (r0 + 4 * t) + far_hi;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            lo[k] = *reinterpret_cast<const p_v4f_a4*>(xl + k * KR32_TILE);
            hi[k] = *reinterpret_cast<const p_v4f_a4*>(xh + k * KR32_TILE);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int qi = t + i * KR32_T;
            if (qi < nquads) {
                const int32_t e = min(max(e0 + 4 * qi, 0), xlast);             // outside x: any valid quad (only absent entries address it)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.x + e),
                                                 (__attribute__((address_space(3))) void*)(xs + 4 * (i * KR32_T + wbase)), 16, 0, 0);
            }
        }
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int64_t row = (int64_t)r0 + k * KR32_TILE + 4 * t;
            float l[4], h[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {                                      // an element outside the allocation belongs to an absent entry
                const int64_t cl = row + r + far_lo, ch = row + r + far_hi;
                l[r] = a.x[min(max(cl, (int64_t)0), (int64_t)xcap - 1)];
                h[r] = a.x[min(max(ch, (int64_t)0), (int64_t)xcap - 1)];
            }
            lo[k].x = l[0]; lo[k].y = l[1]; lo[k].z = l[2]; lo[k].w = l[3];
            hi[k].x = h[0]; hi[k].y = h[1]; hi[k].z = h[2]; hi[k].w = h[3];
        }
    }
    if constexpr (NQ > 0) {
#pragma unroll
        for (int k = 0; k < T; ++k) {
            dv[k].x = 0.0f; dv[k].y = 0.0f; dv[k].z = 0.0f; dv[k].w = 0.0f;
            if (k < nt) dv[k] = *reinterpret_cast<const p_v4f*>(a.dvec + r0 + k * KR32_TILE + 4 * t);
        }
    }
    for (int i = t; i < a.npat; i += KR32_T) meta[i] = reinterpret_cast<const p_v2u*>(a.pmeta)[i];
    for (int i = t; i < a.ntab; i += KR32_T) pval[i] = a.pval[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // the window has landed (LDS-DMA requests are not counted by the compiler)
    __syncthreads();
    // ---- tile after tile out of LDS
#pragma unroll
    for (int k = 0; k < T; ++k) {
        if (k >= nt) break;                                                    // (uniform)
        const int32_t row = r0 + k * KR32_TILE + 4 * t;
        const unsigned id[4] = {ids[k].x & 0xffffu, ids[k].x >> 16, ids[k].y & 0xffffu, ids[k].y >> 16};
        const int j = k * KR32_TILE + 4 * t + n + 4;                           // xs[j] = x[row]
        const p_v4f A = *reinterpret_cast<const p_v4f*>(xs + j - 4), B = *reinterpret_cast<const p_v4f*>(xs + j), C = *reinterpret_cast<const p_v4f*>(xs + j + 4);
        const p_v4f M = *reinterpret_cast<const p_v4f*>(xs + j - n), P = *reinterpret_cast<const p_v4f*>(xs + j + n);
        const float near[4][7] = {{lo[k].x, M.x, A.w, B.x, B.y, P.x, hi[k].x}, {lo[k].y, M.y, B.x, B.y, B.z, P.y, hi[k].y},
                                  {lo[k].z, M.z, B.y, B.z, B.w, P.z, hi[k].z}, {lo[k].w, M.w, B.z, B.w, C.x, P.w, hi[k].w}};
        bool valid[4]; float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            valid[r] = row + r < a.nrows;
            p_v2u m; m.x = 0u; m.y = 0u;
            if (valid[r]) m = meta[id[r]];
            const float* tv = pval + (m.x & 0xffffu);
            double s = 0.0;
#pragma unroll
            for (int u = 0; u < 7; ++u) {
                const double tt = s + (double)tv[u] * (double)near[r][u];
                s = ((m.y >> u) & 1u) ? tt : s;
            }
            o[r] = (float)s;
        }
        quad_store(a.y, row, a.nrows, o);
        if constexpr (NQ > 0) {
            const double wsum = wave_butterfly(quad_dot(dv[k], o, valid));
            if ((t & 63) == 0) red[k * (KR32_T / 64) + (t >> 6)] = wsum;
        }
    }
    if constexpr (NQ > 0) {
        __syncthreads();
        if (t < nt) {                                                          // thread k: tile qr + k, the 4 waves in turn
            double sum = red[t * (KR32_T / 64)];
#pragma unroll
            for (int w2 = 1; w2 < KR32_T / 64; ++w2) sum = sum + red[t * (KR32_T / 64) + w2];
            a.partials[qr + t] = sum;
        }
    }
}

int32_t enqueue_spmv32_pattern_stage(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const int64_t nt = ntiles32_of(a->nrows);
    Spmv32PatArgs g{a->d_pid, a->d_pmeta, a->d_poff, a->d_pval, x, y, dvec, ctx->d_partials, done,
                    (int32_t)a->nrows, (int32_t)nt, a->npat, a->ntab, 0, (int32_t)vec32_len(a->ncols), 0};
    // T: runs of 2 tiles.  In-process A/B (tools/mixed_bench.py pspmv, profiles/mixed/pattern_*.jsonl; windows >= 0.5 s alternated, medians), 7-point:
    // 256^3 0.0420 ms with runs of 1 against 0.0387 ms with runs of 2; 512^3 0.349 against 0.317 ms.  Nothing smaller than 256^3 was measured.
    const int T = env_int("KRYST_SPMV32_STAGE_T", 2) >= 2 ? 2 : 1;
    const int32_t n = a->pat_stage_n;
    const size_t head = sizeof(float) * (size_t)(T * KR32_TILE + 2 * n + 8) + (size_t)a->npat * 8 + sizeof(float) * (size_t)a->ntab;
    g.red_off = (int32_t)((head + 15) & ~(size_t)15);
    const size_t lds = (size_t)g.red_off + sizeof(double) * T * (KR32_T / 64);
    const dim3 grid((unsigned)((nt + T - 1) / T)), block(KR32_T);
    auto launch = [&](auto Q, auto T_) { hipLaunchKernelGGL((spmv32_pattern_stage_kernel<Q() ? 1 : 0, T_()>), grid, block, lds, ctx->s_main, g, n, a->pat_far_lo, a->pat_far_hi); };
    by_bool(nq != 0, [&](auto Q) { by_int<1, 2>(T, [&](auto T_) { launch(Q, T_); }); });
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

// ---------------------------------------------------------------------------------------------------- the lowering of the form
// the operator must have a CSR-P16 form, and the kernels address x and y with 32-bit byte offsets
const char* lower_pattern_refusal(kryst_csr_t a) {
    if (!(a->d_pid && a->d_pmeta && a->d_poff && a->d_pval && a->npat > 0)) return "the operator has no CSR-P16 form";
    return offsets_fit32(a) ? nullptr : "the vectors do not fit 32-bit byte offsets";
}

// ids re-padded to the fp32 tile (the fp64 array is padded to a 512-row tile only); the tables as they are, the values rounded as the CSR values are
hipError_t enqueue_lower_pattern(kryst_csr_t a, kryst_csr32_t m) {
    hipStream_t s = a->ctx->s_main;
    const size_t nid = (size_t)ntiles32_of(a->nrows) * KR32_TILE + KR32_TILE;
    hipError_t e = hipMalloc(&m->d_pid, sizeof(uint16_t) * nid);
    if (e == hipSuccess) e = hipMalloc(&m->d_pmeta, sizeof(uint32_t) * 2 * (size_t)a->npat);
    if (e == hipSuccess) e = hipMalloc(&m->d_poff, sizeof(int32_t) * (size_t)std::max(a->ntab, 1));
    if (e == hipSuccess) e = hipMalloc(&m->d_pval, sizeof(float) * (size_t)std::max(a->ntab, 1));
    if (e == hipSuccess) e = hipMemsetAsync(m->d_pid, 0, sizeof(uint16_t) * nid, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_pid, a->d_pid, sizeof(uint16_t) * (size_t)a->nrows, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_pmeta, a->d_pmeta, sizeof(uint32_t) * 2 * (size_t)a->npat, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && a->ntab > 0) e = hipMemcpyAsync(m->d_poff, a->d_poff, sizeof(int32_t) * (size_t)a->ntab, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && a->ntab > 0) e = enqueue_round32(a->ctx, m->d_pval, a->d_pval, (int64_t)a->ntab, 0, 1.0);
    m->npat = a->npat; m->ntab = a->ntab; m->pat_unroll = a->pat_unroll; m->pat_single = a->pat_single;
    m->pat_stage_n = a->pat_stage_n; m->pat_far_lo = a->pat_far_lo; m->pat_far_hi = a->pat_far_hi; m->pat_far_uniform = a->pat_far_uniform;
    return e;
}

}  // namespace kr
