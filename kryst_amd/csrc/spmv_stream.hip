// The SpMV kernels that STREAM the matrix entry by entry or diagonal by diagonal -- spmv_wave_kernel (plain CSR), spmv_rows_kernel (plain CSR or
// CSR-D8), spmv_dict_kernel (CSR-D16), spmv_dia_kernel (CSR-DIA) -- and their enqueue functions.  spmv.hip has the shared contract and the choice.
#include "spmv.h"

namespace kr {
// Products-in-LDS form (plain int32 columns): each of the 4 waves streams the nnz range of ITS 128 rows (lane l: rows
// 2l, 2l+1 of the wave's slice) through a private LDS window, gathering x and storing the PRODUCTS.  Same-wave LDS traffic is
// ordered by the hardware, so the main path has NO workgroup barrier: waves run their load / gather / LDS / sum
// phases out of step and hide each other's latency.  Only the optional fused inner product meets at one barrier.
template <int NQ, bool HALO, int SLOTS, bool NT, int MINW = 1>
__global__ __launch_bounds__(KR_T, MINW) void spmv_wave_kernel(const SpmvArgs a) {
    if (a.done && *a.done) return;
    constexpr int WCAP = SLOTS * 128;                       // entries per wave window
    __shared__ __attribute__((aligned(16))) double prod_all[4 * WCAP];
    __shared__ double red[(NQ > 0 ? NQ : 1) * (KR_T / 64)];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    double* prod = prod_all + w * WCAP;
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    for (int li = slot0; li < a.xcd_chunk; li += per) {
        int ti;
        if (a.swizzle) ti = xcd * a.xcd_chunk + li;
        else ti = ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) { if (a.swizzle) break; else continue; }
        const int q = a.tiles ? a.tiles[ti] : ti;
        if (q < 0) continue;                                    // an empty slot of the slab order
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int wr0 = min(r0 + 128 * w, r1), wr1 = min(wr0 + 128, r1);
        const int row = r0 + 2 * t;
        const int p0 = a.row_ptr[min(row, r1)];
        const int p1 = a.row_ptr[min(row + 1, r1)];
        const int p2 = a.row_ptr[min(row + 2, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s0 = 0.0, s1 = 0.0;
#ifdef KR_TUNING
        if (a.abl & 128) { if (row + 1 < r1) st2(a.y, row, (double)p0, (double)p1); }     // the y traffic at the START of the tile (timing only)
#endif
        // a window starts on a memory line of both streams when amask = 31 (32 entries = 128 B of columns, 256 B of values):
        // every load instruction then covers whole lines, which matters for nontemporal loads (no L1 copy of a shared line)
        for (int base = k0 & ~a.amask; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            const int npairs = (wend - base + 1) >> 1;
            v2i c[SLOTS]; v2d v[SLOTS]; double xa[SLOTS], xb[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int pi = min(l + j * 64, npairs - 1);
                const int k = base + 2 * pi;
                c[j] = stream_load<NT>(reinterpret_cast<const v2i*>(a.col + k));
                v[j] = stream_load<NT>(reinterpret_cast<const v2d*>(a.val + k));
            }
#ifdef KR_TUNING
            // timing-only ablations (round-2 study, profiles/r02/plain_csr_study/; wrong results): 1 no x gathers, 2 no LDS products / row sums, 4 no y / dot
            if (a.abl & 1) {
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) { xa[j] = (double)c[j].x; xb[j] = (double)c[j].y; }
            } else
#endif
            {
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) { xa[j] = gather<HALO>(a, c[j].x); xb[j] = gather<HALO>(a, c[j].y); }
            }
#ifdef KR_TUNING
            if (a.abl & 2) {
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) { s0 = s0 + v[j].x * xa[j]; s1 = s1 + v[j].y * xb[j]; }
                continue;
            }
#endif
#pragma unroll
            for (int j = 0; j < SLOTS; ++j)
                *reinterpret_cast<double2*>(&prod[2 * (l + j * 64)]) = make_double2(v[j].x * xa[j], v[j].y * xb[j]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            s0 = row_sum(prod, base, max(p0, base), min(p1, wend), s0);
            s1 = row_sum(prod, base, max(p1, base), min(p2, wend), s1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#ifdef KR_TUNING
        if (a.abl & 4) { if (s0 + s1 == 0.123456789) a.y[row] = s0; continue; }
        if (a.abl & 64) { if (row + 1 < r1) st2_keep(a.y, row, s0, s1); else if (row < r1) a.y[row] = s0; } else
#endif
        { if (row + 1 < r1) st2(a.y, row, s0, s1);
        else if (row < r1) a.y[row] = s0; }
        if constexpr (NQ > 0) {
            double acc[NQ];
#ifdef KR_TUNING
            d2 d;
            if (a.abl & 16) { d.a = s1; d.b = s0; }
            else if (a.abl & 8) d = ld2_keep(a.dvec, row);
            else d = ld2(a.dvec, row);
#else
            const d2 d = ld2(a.dvec, row);
#endif
            acc[0] = 0.0;
            if (row < r1) acc[0] = acc[0] + d.a * s0;
            if (row + 1 < r1) acc[0] = acc[0] + d.b * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                if (row < r1) acc[1] = acc[1] + s0 * s0;
                if (row + 1 < r1) acc[1] = acc[1] + s1 * s1;
            }
#ifdef KR_TUNING
            if (a.abl & 32) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) acc[k] = wave_butterfly(acc[k]);
                if (l == 0) {
#pragma unroll
                    for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
                }
                continue;
            }
#endif
            block_reduce<NQ, KR_T / 64>(acc, red);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// "rows" form: phase 1 only STREAMS the matrix (values + column indices, or values + 1-byte column codes) into the
// wave's LDS window -- no dependent gather, every load of the window in flight at once; phase 2 walks each row in
// ascending column order, and the row's owner lane gathers x itself: neighbouring lanes own neighbouring rows, so
// for banded / stencil matrices one gather instruction touches a contiguous run of x (8 cache lines, all used by
// the lane's second row) instead of the 14 scattered lines of an entry-order gather.
//
// CSR-D8 index compression (COMP): when the operator has at most 256 distinct (col - row) offsets -- every
// structured-grid discretisation, whatever its coefficients -- kryst_csr_create stores one byte per entry, a code
// into a 256-entry offset dictionary, beside the plain int32 columns.  The kernel then moves 9 instead of 12 bytes
// per nonzero; the arithmetic (values, ascending column order, un-fused mul/add) is unchanged, so results are
// bit-identical to the plain path.  Matrices with more distinct offsets use the plain int32 columns.
template <int NQ, bool HALO, int SLOTS, bool COMP>
__global__ __launch_bounds__(KR_T) void spmv_rows_kernel(const SpmvArgs a) {
    if (a.done && *a.done) return;
    constexpr int WCAP = SLOTS * 128;                       // entries per wave window
    constexpr int CCAP = WCAP + 32;                         // code bytes per wave window (16-byte aligned start + slack)
    __shared__ __attribute__((aligned(16))) double val_all[4 * WCAP];
    __shared__ __attribute__((aligned(16))) int32_t col_all[COMP ? 4 : 4 * WCAP];
    __shared__ __attribute__((aligned(16))) uint8_t code_all[COMP ? 4 * CCAP : 16];
    __shared__ int32_t dict[COMP ? 256 : 1];
    __shared__ double red[(NQ > 0 ? NQ : 1) * (KR_T / 64)];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    double* lval = val_all + w * WCAP;
    int32_t* lcol = col_all + (COMP ? 0 : w * WCAP);
    uint8_t* lcode = code_all + (COMP ? w * CCAP : 0);
    if constexpr (COMP) { dict[t] = a.dict[t]; __syncthreads(); }
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    for (int li = slot0; li < a.xcd_chunk; li += per) {
        int ti;
        if (a.swizzle) ti = xcd * a.xcd_chunk + li;
        else ti = ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) { if (a.swizzle) break; else continue; }
        const int q = a.tiles ? a.tiles[ti] : ti;
        if (q < 0) continue;                                    // an empty slot of the slab order
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int wr0 = min(r0 + 128 * w, r1), wr1 = min(wr0 + 128, r1);
        const int row = r0 + 2 * t;
        const int p0 = a.row_ptr[min(row, r1)];
        const int p1 = a.row_ptr[min(row + 1, r1)];
        const int p2 = a.row_ptr[min(row + 2, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        for (int base = k0 & ~1; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            const int npairs = (wend - base + 1) >> 1;
            // ---- phase 1: stream the window into LDS
            v2d v[SLOTS];
            [[maybe_unused]] v2i c[SLOTS];
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int pi = min(l + j * 64, npairs - 1);
                const int k = base + 2 * pi;
                v[j] = *reinterpret_cast<const v2d*>(a.val + k);
                if constexpr (!COMP) c[j] = *reinterpret_cast<const v2i*>(a.col + k);
            }
            int cbase = 0;
            if constexpr (COMP) {
                cbase = base & ~15;                                   // 16-byte aligned start of the code window
                const int nbytes = wend - cbase;
                const int off = min(16 * l, ((nbytes + 15) & ~15) - 16);
                const uint4 cw = *reinterpret_cast<const uint4*>(a.code + cbase + off);
                if (16 * l < nbytes + 16) *reinterpret_cast<uint4*>(lcode + off) = cw;
            }
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                *reinterpret_cast<double2*>(&lval[2 * (l + j * 64)]) = make_double2(v[j].x, v[j].y);
                if constexpr (!COMP) *reinterpret_cast<int2*>(&lcol[2 * (l + j * 64)]) = make_int2(c[j].x, c[j].y);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- phase 2: the two rows of the lane, four entries of each in flight, folded in ascending column order
            int ka = max(p0, base), kb = max(p1, base);
            const int ea = min(p1, wend), eb = min(p2, wend);
            while (ka < ea || kb < eb) {
                double va[4], vb[4], xa[4], xb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ia = min(ka + u, max(ea - 1, base)), ib = min(kb + u, max(eb - 1, base));
                    int ca, cb;
                    if constexpr (COMP) { ca = row + dict[lcode[ia - cbase]]; cb = row + 1 + dict[lcode[ib - cbase]]; }
                    else { ca = lcol[ia - base]; cb = lcol[ib - base]; }
                    va[u] = lval[ia - base]; vb[u] = lval[ib - base];
                    xa[u] = (ka + u < ea) ? gather<HALO>(a, ca) : 0.0;
                    xb[u] = (kb + u < eb) ? gather<HALO>(a, cb) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ka + u < ea) s0 = s0 + va[u] * xa[u];
                    if (kb + u < eb) s1 = s1 + vb[u] * xb[u];
                }
                ka += 4; kb += 4;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (row + 1 < r1) st2(a.y, row, s0, s1);
        else if (row < r1) a.y[row] = s0;
        if constexpr (NQ > 0) {
            double acc[NQ];
            const d2 d = ld2(a.dvec, row);
            acc[0] = 0.0;
            if (row < r1) acc[0] = acc[0] + d.a * s0;
            if (row + 1 < r1) acc[0] = acc[0] + d.b * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                if (row < r1) acc[1] = acc[1] + s0 * s0;
                if (row + 1 < r1) acc[1] = acc[1] + s1 * s1;
            }
            block_reduce<NQ, KR_T / 64>(acc, red);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
            }
        }
    }
}

// CSR-D16, the fully dictionary-coded form (spmv_dict_kernel): when, besides the <= 256 distinct (col - row) offsets of
// CSR-D8, the operator also has at most 256 distinct VALUES (bit patterns) -- constant-coefficient discretisations on
// uniform grids: every BASELINE config -- kryst_csr_create keeps one 16-bit word per entry, (value code << 8) | offset
// code, and two 256-entry dictionaries.  The kernel then streams 2 instead of 12 bytes per nonzero (34 instead of 95
// bytes per row of a 7-point stencil, vectors included).  The decoded value is the stored double bit for bit and the
// arithmetic (ascending column order from 0.0, separate mul and add) is unchanged, so y is bit-identical to the plain
// path; operators with more distinct values or offsets use CSR-D8 or plain CSR.  A wave's window is its slice's run
// of code words (<= 1016 per pass), loaded 16 B per lane from an 8-entry-aligned start; no workgroup barrier after
// the dictionaries are in LDS.
template <int NQ, bool HALO>
__global__ __launch_bounds__(KR_T) __attribute__((amdgpu_waves_per_eu(8, 8))) void spmv_dict_kernel(const SpmvArgs a) {
    if (a.done && *a.done) return;
    constexpr int WCAP = 1016;                              // entries per wave pass (2 x 64 lanes x 8 entries, minus alignment slack)
    constexpr int CCAP = 1024 + 8;
    __shared__ __attribute__((aligned(16))) uint16_t code_all[4 * CCAP];
    __shared__ int32_t dict[256];
    __shared__ double vdict[256];
    __shared__ double red[(NQ > 0 ? NQ : 1) * (KR_T / 64)];
    const int t = threadIdx.x, l = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    uint16_t* lcode = code_all + w * CCAP;
    dict[t] = a.dict[t]; vdict[t] = a.vdict[t];
    __syncthreads();
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    for (int li = slot0; li < a.xcd_chunk; li += per) {
        int ti;
        if (a.swizzle) ti = xcd * a.xcd_chunk + li;
        else ti = ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) { if (a.swizzle) break; else continue; }
        const int q = a.tiles ? a.tiles[ti] : ti;
        if (q < 0) continue;                                    // an empty slot of the slab order
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int wr0 = min(r0 + 128 * w, r1), wr1 = min(wr0 + 128, r1);
        const int row = r0 + 2 * t;
        const int p0 = a.row_ptr[min(row, r1)];
        const int p1 = a.row_ptr[min(row + 1, r1)];
        const int p2 = a.row_ptr[min(row + 2, r1)];
        const int k0 = a.row_ptr[wr0], k1 = a.row_ptr[wr1];         // wave-uniform
        double s0 = 0.0, s1 = 0.0;
        for (int base = k0; base < k1; base += WCAP) {
            const int wend = min(base + WCAP, k1);
            // ---- phase 1: the window's code words -> LDS (two 16-byte loads per lane, both in flight)
            const int cbase = base & ~7;
            const int nent = wend - cbase;                            // <= WCAP + 7
            const int lastoff = ((nent + 7) & ~7) - 8;
            const int o0 = min(8 * l, lastoff), o1 = min(8 * (l + 64), lastoff);
            const uint4 c0 = *reinterpret_cast<const uint4*>(a.code16 + cbase + o0);
            const uint4 c1 = *reinterpret_cast<const uint4*>(a.code16 + cbase + o1);
            if (8 * l < nent) *reinterpret_cast<uint4*>(lcode + o0) = c0;
            if (8 * (l + 64) < nent) *reinterpret_cast<uint4*>(lcode + o1) = c1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- phase 2: the two rows of the lane, four entries of each in flight, folded in ascending column order
            int ka = max(p0, base), kb = max(p1, base);
            const int ea = min(p1, wend), eb = min(p2, wend);
            while (ka < ea || kb < eb) {
                // all gathers of the batch are issued before the first value is decoded (U = 7: a 7-point row in one trip)
                constexpr int U = 7;
                double xa[U], xb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int ia = min(ka + u, max(ea - 1, base)), ib = min(kb + u, max(eb - 1, base));
                    const int ca = row + dict[lcode[ia - cbase] & 255u], cb = row + 1 + dict[lcode[ib - cbase] & 255u];
                    xa[u] = (ka + u < ea) ? gather<HALO>(a, ca) : 0.0;
                    xb[u] = (kb + u < eb) ? gather<HALO>(a, cb) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {                       // the code words are re-read from LDS: cheaper than holding them
                    const int ia = min(ka + u, max(ea - 1, base)), ib = min(kb + u, max(eb - 1, base));
                    if (ka + u < ea) s0 = s0 + vdict[lcode[ia - cbase] >> 8] * xa[u];
                    if (kb + u < eb) s1 = s1 + vdict[lcode[ib - cbase] >> 8] * xb[u];
                }
                ka += U; kb += U;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (row + 1 < r1) st2(a.y, row, s0, s1);
        else if (row < r1) a.y[row] = s0;
        if constexpr (NQ > 0) {
            double acc[NQ];
            const d2 d = ld2(a.dvec, row);
            acc[0] = 0.0;
            if (row < r1) acc[0] = acc[0] + d.a * s0;
            if (row + 1 < r1) acc[0] = acc[0] + d.b * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                if (row < r1) acc[1] = acc[1] + s0 * s0;
                if (row + 1 < r1) acc[1] = acc[1] + s1 * s1;
            }
            block_reduce<NQ, KR_T / 64>(acc, red);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
            }
        }
    }
}

// CSR-DIA (spmv_dia_kernel): operators with a handful of well-filled diagonals -- every stencil on a structured grid, variable
// coefficients included.  The values are stored as one stream per diagonal in natural row order (csr_create.hip: build_dia), an
// absent entry carries a NaN payload no stored value may have, so there are NO row pointers, NO per-entry codes and no
// dependent load: lane t (rows 2t, 2t+1) issues, per diagonal, one 16-byte nontemporal load of its two values and one 16-byte
// load of x[2t + off], x[2t + 1 + off] -- all 2 D loads of a tile in flight at once -- and then folds the present entries in
// diagonal (= stored, ascending column) order from 0.0 with separate mul and add: the reference's loop (sparse.rs:107-113), bit
// for bit.  8 D + 16 bytes per row (7-point: 72; CSR-D8 83, plain CSR 104).  Pair loads of x are clamped at the top of x's
// (padded) allocation -- only an absent entry can point there -- and tiles whose lowest diagonal would start before x[0], as well
// as tiles with halo columns, take the per-element clamped path.
// one batch of DB diagonals starting at d0 (EXACT: the operator has exactly DB diagonals, so every index is a compile-time constant
// and the offsets are plain kernel arguments); FAST: 16-byte pair loads of x, else per-element clamped gathers
template <bool HALO, int DB, bool EXACT, bool FAST>
__device__ __forceinline__ void dia_batch(const SpmvArgs& a, int row, int d0, int nd, double& s0, double& s1) {
    v2d v[DB], xx[DB];
    const double* vrow = a.dia + row;
#pragma unroll
    for (int u = 0; u < DB; ++u) {
        const int d = EXACT ? u : min(d0 + u, nd - 1);           // (a batch's tail re-reads the last diagonal; not used below)
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(vrow + (int64_t)d * a.dia_stride));
        const int64_t c = (int64_t)row + a.dia_off[d];
        if constexpr (FAST) {
            xx[u] = *reinterpret_cast<const v2d*>(a.x + min(c, a.xsafe));
        } else {
            const int32_t c0 = (int32_t)min(max(c, (int64_t)0), (int64_t)a.cmax), c1 = (int32_t)min(max(c + 1, (int64_t)0), (int64_t)a.cmax);
            xx[u].x = gather<HALO>(a, c0); xx[u].y = gather<HALO>(a, c1);
        }
    }
#pragma unroll
    for (int u = 0; u < DB; ++u) {
        if (EXACT || d0 + u < nd) {
            const double ta = s0 + v[u].x * xx[u].x, tb = s1 + v[u].y * xx[u].y;
            s0 = ((unsigned long long)__double_as_longlong(v[u].x) != KR_DIA_ABSENT) ? ta : s0;
            s1 = ((unsigned long long)__double_as_longlong(v[u].y) != KR_DIA_ABSENT) ? tb : s1;
        }
    }
}

template <int NQ, bool HALO, int DB, bool EXACT>
__global__ __launch_bounds__(KR_T) void spmv_dia_kernel(const SpmvArgs a) {
    if (a.done && *a.done) return;
    __shared__ double red[(NQ > 0 ? NQ : 1) * (KR_T / 64)];
    const int t = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    const int nd = a.dia_nd;
    for (int li = slot0; li < a.xcd_chunk; li += per) {
        int ti;
        if (a.swizzle) ti = xcd * a.xcd_chunk + li;
        else ti = ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) { if (a.swizzle) break; else continue; }
        const int q = a.tiles ? a.tiles[ti] : ti;
        if (q < 0) continue;                                    // an empty slot of the slab order
        const int r0 = q * KR_TILE;
        const int r1 = min(r0 + KR_TILE, a.nrows);
        const int row = r0 + 2 * t;
        double s0 = 0.0, s1 = 0.0;
        if (!HALO && r0 + a.dia_min >= 0) {                            // uniform over the workgroup
            for (int d0 = 0; d0 < (EXACT ? 1 : nd); d0 += DB) dia_batch<HALO, DB, EXACT, true>(a, row, d0, nd, s0, s1);
        } else {
            for (int d0 = 0; d0 < (EXACT ? 1 : nd); d0 += DB) dia_batch<HALO, DB, EXACT, false>(a, row, d0, nd, s0, s1);
        }
        if (row + 1 < r1) st2(a.y, row, s0, s1);
        else if (row < r1) a.y[row] = s0;
        if constexpr (NQ > 0) {
            double acc[NQ];
            const d2 d = ld2(a.dvec, row);
            acc[0] = 0.0;
            if (row < r1) acc[0] = acc[0] + d.a * s0;
            if (row + 1 < r1) acc[0] = acc[0] + d.b * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                if (row < r1) acc[1] = acc[1] + s0 * s0;
                if (row + 1 < r1) acc[1] = acc[1] + s1 * s1;
            }
            block_reduce<NQ, KR_T / 64>(acc, red);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
            }
        }
    }
}

// spmv.hip's launch_tiles has chosen the kernel and filled the tiles and their slotting (p); comp: the rows kernel streams CSR-D8's byte codes
int32_t enqueue_stream(TileKernel kernel, kryst_csr_t a, SpmvArgs g, bool halo, int nq, const PlainWavePlan& p, bool comp) {
    const dim3 grid(p.grid), block(KR_T);
    hipStream_t s = a->ctx->s_main;
    if (kernel == TileKernel::Dict)
        return by_nq(nq, [&](auto NQ) { by_bool(halo, [&](auto H) { hipLaunchKernelGGL((spmv_dict_kernel<NQ(), H()>), grid, block, 0, s, g); }); });
    if (kernel == TileKernel::Dia) {
        g.dia = a->d_dia; g.dia_stride = a->dia_stride; g.dia_nd = a->dia_nd; g.dia_min = a->dia_min;
        for (int d = 0; d < KR_DIA_MAX; ++d) g.dia_off[d] = a->dia_off[d];
        g.xsafe = xsafe_of(a);
        g.cmax = (int32_t)(halo ? a->nrows + a->plan.total_recv - 1 : a->xlen - 1);
        // exactly 3 / 5 / 7 / 9 diagonals: one batch with compile-time indices; else batches of 4 (fewer than 7 diagonals) or 8
        const int nd = a->dia_nd, exact = nd == 3 || nd == 5 || nd == 7 || nd == 9 ? nd : 0;
        return by_nq(nq, [&](auto NQ) { by_bool(halo, [&](auto H) {
            if (!by_int<3, 5, 7, 9>(exact, [&](auto DB) { hipLaunchKernelGGL((spmv_dia_kernel<NQ(), H(), DB(), true>), grid, block, 0, s, g); }))
                by_int<4, 8>(nd < 7 ? 4 : 8, [&](auto DB) { hipLaunchKernelGGL((spmv_dia_kernel<NQ(), H(), DB(), false>), grid, block, 0, s, g); });
        }); });
    }
    const int slots_env = env_int("KRYST_SPMV_SLOTS", 0);
    if (kernel == TileKernel::Rows) {
        // measured (tools/tune_spmv.py): with vectors beyond the 256 MiB Infinity Cache the smaller window (more resident waves) wins, below it the
        // one-window-per-slice form does -- p.slots; on plain columns (KRYST_SPMV_KERNEL=3) the rows kernel keeps the operator's window
        const int slots = comp ? p.slots : slots_env > 0 ? slots_env : a->slots;
        return by_nq(nq, [&](auto NQ) { by_bool(halo, [&](auto H) { by_int<4, 7>(slots <= 4 ? 4 : 7, [&](auto SL) { by_bool(comp, [&](auto C) {
            hipLaunchKernelGGL((spmv_rows_kernel<NQ(), H(), SL(), C()>), grid, block, 0, s, g); }); }); }); });
    }
    // the wave kernel: pair slots per lane sized to the matrix's average slice length (a wave streams the nnz of 128 rows: <= 256 nnz -> 2 slots,
    // <= 512 -> 4, else 7 = a 7-point stencil's 896)
    return by_nq(nq, [&](auto NQ) { by_bool(halo, [&](auto H) { by_int<2, 4, 7>(p.slots <= 2 ? 2 : p.slots <= 4 ? 4 : 7, [&](auto SL) { by_bool(p.nt, [&](auto NT) {
        hipLaunchKernelGGL((spmv_wave_kernel<NQ(), H(), SL(), NT()>), grid, block, 0, s, g); }); }); }); });
}

}  // namespace kr
