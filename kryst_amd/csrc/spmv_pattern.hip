// The CSR-P16 kernels of a plain SpMV -- spmv_pattern_kernel and spmv_pattern_stage_kernel (near operands staged in LDS) -- and their enqueue
// functions.  spmv.hip has the shared contract and the choice; the staged-window kernels fused with CG's vector passes are in spmv_fuse.hip.
#include "spmv.h"

namespace kr {
// CSR-P16, row-pattern coding (spmv_pattern_kernel): operators assembled from a few stencils -- constant-coefficient
// discretisations on structured grids, i.e. every BASELINE config -- repeat the same ROW, as a sequence of
// (col - row, value) pairs, millions of times (a 7-point operator on a box has 27 distinct rows, all of them
// sub-sequences of the interior row).  kryst_csr_create numbers the distinct rows ("patterns", at most KR_PMAX) and
// expresses each as a BASE sequence (at most KR_TMAX table entries in total) plus a 16-bit presence mask; it keeps one
// 16-bit pattern id per row beside the CSR arrays, and the SpMV streams 2 bytes per ROW (18 bytes per row with x and y,
// against 95 for plain CSR): no row pointers, no per-entry codes, no dependent row_ptr -> entries load chain.  Each lane
// walks its rows' entries in the stored (ascending column) order with the reference's un-fused mul/add, skipping the
// masked-out ones, so y is bit-identical to the plain path.  Everything else falls back to CSR-D16 / CSR-D8 / plain CSR.
//
// At 18 bytes per row the kernel is bound by instruction issue, not by HBM (rocprofv3 --pmc: TA busy 59 %, the texture path
// spends ~16 cycles per 64-lane load whatever its width), so it is built around 16-BYTE gathers: thread t owns the adjacent
// rows 2t, 2t+1; when both rows share a base (interior rows and the boundary rows next to them do) entry e of both rows
// reads x[2t + off_e] and x[2t + 1 + off_e] -- one dwordx4 load -- and one table lookup serves both rows.  Row pairs with
// different bases take the two-loads-per-entry path.  x is addressed with 32-bit byte offsets from a scalar base (the
// launch checks xlen < 2^28).
// x[c8 / 8] for a byte offset c8 >= 0 (local entries below nloc8, halo entries above)
template <bool HALO>
__device__ __forceinline__ const char* gather_base8(const SpmvArgs& a, int32_t c8) {
    if constexpr (HALO) return (c8 < a.nloc8) ? reinterpret_cast<const char*>(a.x) : reinterpret_cast<const char*>(a.halo) - a.nloc8;
    else return reinterpret_cast<const char*>(a.x);
}
template <bool HALO>
__device__ __forceinline__ double gather8(const SpmvArgs& a, int32_t c8) {
    return *reinterpret_cast<const double*>(gather_base8<HALO>(a, c8) + (uint32_t)c8);
}

// SINGLE: no base is longer than U entries (true for every stencil operator), so the entry loop has one trip
// CENTER >= 0: the fused dot's vector is x itself and every row has its diagonal entry at table position CENTER.
// MERGE3: table positions 2, 3, 4 of every base are the columns row-1, row, row+1 (stencil generator): x[row-1 .. row+2] is
// fetched with two 16-byte gathers instead of three (the kernel's cost is per vector-memory instruction).
template <int NQ, bool HALO, int U, bool SINGLE, int CENTER = -1, bool MERGE3 = false>
__global__ __launch_bounds__(KR_T) void spmv_pattern_kernel(const SpmvArgs a) {
    if (a.done && *a.done) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* pval = reinterpret_cast<double*>(smem);                                   // ntab + U entries
    int32_t* poff = reinterpret_cast<int32_t*>(pval + a.ntab + U);                    // BYTE offsets: 8 * (col - row)
    uint2* meta = reinterpret_cast<uint2*>(poff + a.ntab + U + ((a.ntab + U) & 1));   // 8-byte aligned
    double* red = reinterpret_cast<double*>(smem + a.pat_red_off);
    const int t = threadIdx.x;
    // workgroup b of XCD x owns the tpw CONSECUTIVE tile slots [b*tpw, (b+1)*tpw) of that XCD's share; workgroups are
    // handed out in order by the dispatcher, so the tiles in flight on an XCD stay a compact window of the grid and the
    // x planes they share stay in its L2 (a strided persistent loop lets fast workgroups run ahead: 2.5x the x traffic)
    const int xcd = blockIdx.x & 7, slot0 = blockIdx.x >> 3, tpw = a.tpw;
    const int li_end = min((slot0 + 1) * tpw, a.xcd_chunk);
    auto tile_of = [&](int li) -> int {
        if (li >= li_end) return -1;
        const int ti = a.swizzle ? xcd * a.xcd_chunk + li : ((li / a.group) * 8 + xcd) * a.group + (li % a.group);
        if (ti >= a.ntiles) return -1;
        return a.tiles ? a.tiles[ti] : ti;
    };
    int q = tile_of(slot0 * tpw);
    unsigned ids = 0;
    if (q >= 0) ids = *reinterpret_cast<const unsigned*>(a.pid + (size_t)q * KR_TILE + 2 * t);   // rows 2t, 2t+1 (padded array)
    // (the first tile's ids are on their way while the tables are copied)
    for (int i = t; i < a.npat; i += KR_T) meta[i] = reinterpret_cast<const uint2*>(a.pmeta)[i];
    for (int i = t; i < a.ntab + U; i += KR_T) { poff[i] = i < a.ntab ? 8 * a.poff[i] : 0; pval[i] = i < a.ntab ? a.pval[i] : 0.0; }
    __syncthreads();
    for (int li = slot0 * tpw; li < li_end; ++li) {
        const int qn = tile_of(li + 1);                             // prefetch the next tile's ids
        unsigned ids_n = 0;
        if (qn >= 0) ids_n = *reinterpret_cast<const unsigned*>(a.pid + (size_t)qn * KR_TILE + 2 * t);
        if (q >= 0) {
            const int r0 = q * KR_TILE;
            const int r1 = min(r0 + KR_TILE, a.nrows);
            const int row = r0 + 2 * t;
            const int32_t row8 = row << 3;                          // xlen < 2^28: byte offsets fit 31 bits
            const bool va = row < r1, vb = row + 1 < r1;
            uint2 ma = va ? meta[ids & 0xffffu] : make_uint2(0u, 0u), mb = vb ? meta[ids >> 16] : make_uint2(0u, 0u);
            double s0 = 0.0, s1 = 0.0;
            v2d xc; xc.x = 0.0; xc.y = 0.0;                         // x[row], x[row + 1] as the diagonal entry's gather saw them
            if (ma.x == mb.x) {
                // ---- same base: one table lookup and one 16-byte gather per entry serve both rows.  An entry is needed if
                // either row has it; a needed entry addresses x[c], x[c + 1] with c >= -1 (c = -1: only row 2t+1 has it and
                // its column is 0) and c + 1 <= xlen (c + 1 = xlen: only row 2t has it; x is padded at the end).
                const int len = ma.x >> 16;
                const double* tv = pval + (ma.x & 0xffffu); const int32_t* to = poff + (ma.x & 0xffffu);
                for (int e0 = 0; e0 < (SINGLE ? 1 : len); e0 += U) {
                    // masks of the entries e0 .. e0+U-1 (a mask never has bits at or beyond the base length; bases longer than 16
                    // entries have no sub-patterns: all ones up to the length)
                    unsigned ka, kb;
                    if constexpr (SINGLE) { ka = ma.y; kb = mb.y; }
                    else {
                        const unsigned lim = (len - e0 >= 32) ? 0xffffffffu : ((1u << (len - e0)) - 1u);
                        ka = (e0 < 16 ? (ma.y >> e0) : 0xffffffffu) & lim; kb = (e0 < 16 ? (mb.y >> e0) : 0xffffffffu) & lim;
                    }
                    const unsigned kk = ka | kb;
                    int32_t c8[U];
                    int32_t any = 0;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        c8[u] = ((kk >> u) & 1u) ? row8 + to[e0 + u] : row8;
                        if (MERGE3 && u == 2) c8[u] = row8 - 8;          // always: its second element is x[row]
                        if (MERGE3 && u == 4) c8[u] = row8 + 8;          // always: its first element is x[row + 1] (x is padded at the end)
                        any |= c8[u];
                    }
                    v2d xx[U];
                    if (HALO || __builtin_amdgcn_ballot_w64(any < 0) != 0) {
                        // rare: some lane's pair starts one element before x (or the tile touches halo planes)
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            xx[u].x = 0.0; xx[u].y = 0.0;
                            if ((ka >> u) & 1u) xx[u].x = gather8<HALO>(a, c8[u]);
                            if ((kb >> u) & 1u) xx[u].y = gather8<HALO>(a, c8[u] + 8);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (!(MERGE3 && u == 3)) xx[u] = *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(a.x) + (uint32_t)c8[u]);
                        if constexpr (MERGE3) { xx[3].x = xx[2].y; xx[3].y = xx[4].x; }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double v = tv[e0 + u];
                        const double ta = s0 + v * xx[u].x, tb = s1 + v * xx[u].y;
                        s0 = ((ka >> u) & 1u) ? ta : s0;
                        s1 = ((kb >> u) & 1u) ? tb : s1;
                    }
                    if constexpr (CENTER >= 0) xc = xx[CENTER];
                }
            } else {
                // ---- different bases (rare: adjacent rows built from unrelated stencils): each row walks its own, one entry
                // at a time -- kept deliberately small so that it does not cost the common path registers
                const int la = ma.x >> 16, lb = mb.x >> 16;
                const double* tva = pval + (ma.x & 0xffffu); const int32_t* toa = poff + (ma.x & 0xffffu);
                const double* tvb = pval + (mb.x & 0xffffu); const int32_t* tob = poff + (mb.x & 0xffffu);
#pragma unroll 1
                for (int e = 0; e < max(la, lb); ++e) {
                    const bool ia = e < la && (e >= 16 || ((ma.y >> e) & 1u)), ib = e < lb && (e >= 16 || ((mb.y >> e) & 1u));
                    if (ia) s0 = s0 + tva[e] * gather8<HALO>(a, row8 + toa[e]);
                    if (ib) s1 = s1 + tvb[e] * gather8<HALO>(a, row8 + 8 + tob[e]);
                }
            }
            if (vb) st2(a.y, row, s0, s1);
            else if (va) a.y[row] = s0;
            if constexpr (NQ > 0) {
                double acc[NQ];
                d2 d;
                if (CENTER >= 0 && ma.x == mb.x) { d.a = xc.x; d.b = xc.y; }   // (p, Ap): no second load of p, no second wait
                else d = ld2(a.dvec, row);
                acc[0] = 0.0;
                if (va) acc[0] = acc[0] + d.a * s0;
                if (vb) acc[0] = acc[0] + d.b * s1;
                if constexpr (NQ > 1) {
                    acc[1] = 0.0;
                    if (va) acc[1] = acc[1] + s0 * s0;
                    if (vb) acc[1] = acc[1] + s1 * s1;
                }
                block_reduce<NQ, KR_T / 64>(acc, red);
                if (t == 0) {
#pragma unroll
                    for (int k = 0; k < NQ; ++k) a.partials[k * a.pstride + q] = acc[k];
                }
            }
        }
        q = qn; ids = ids_n;
    }
}

// CSR-P16 with the NEAR operands staged in LDS (spmv_pattern_stage_kernel).  spmv_pattern_kernel pays per vector-memory
// instruction (six 16-byte gathers per tile and wave) and per tile a chain of dependent latencies (ids -> tables -> gathers -> store ->
// fold).  For operators whose every base is (far, -n, -1, 0, +1, +n, far) with one even n <= 1024 (csr.h: pat_stage_n -- a box of lines
// of n points; the generator-made operators and host-built ones alike) a workgroup takes a RUN of T consecutive tiles and
//   * requests, together, the ids of all T tiles and the run's window of x -- x[r0 - n - 2 .. r0 + 512 T + n + 2), T + (2 n + 4) / 512
//     coalesced 16-byte loads per lane instead of 4 T gathers -- and copies the tables; one barrier;
//   * requests the far operands (table positions 0 and 6) of all T tiles together;
//   * then computes tile after tile out of LDS: five aligned 16-byte LDS reads give x[row - n], x[row - 2 .. row + 3], x[row + n].
// Two global round trips per RUN instead of a dependent chain per tile, 2 T + T + (2 n + 4) / 512 global loads instead of 6 T.
// The arithmetic is spmv_pattern_kernel's: every row's entries in stored order, un-fused multiply and add, absent entries skipped by
// a select -- the same bits.
// UFAR: the far offsets (table positions 0 and 6) are the same in every base: the far operands are requested with everything else
// (ONE round trip per run), with clamped addresses where a row has no such entry.
template <int NQ, int T, bool CENTER, bool UFAR>
__global__ __launch_bounds__(KR_T) void spmv_pattern_stage_kernel(const SpmvArgs a, const int32_t n, const int32_t far_lo, const int32_t far_hi, const int32_t tile0) {
    if (a.done && *a.done) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int XS = T * KR_TILE + 2 * n + 4;                                  // staged elements (even)
    double* xs = reinterpret_cast<double*>(smem);
    uint2* meta = reinterpret_cast<uint2*>(xs + XS);
    double* pval = reinterpret_cast<double*>(meta + a.npat);
    int32_t* poff = reinterpret_cast<int32_t*>(pval + a.ntab);
    double* red = reinterpret_cast<double*>(smem + a.pat_red_off);
    const int t = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int G = a.group;                                                   // G consecutive runs per XCD (neighbouring runs share window edges)
    // runs of T consecutive tiles of the range [tile0, tile0 + ntiles) (the whole operator, or a rank's interior tiles), groups of G
    // runs round-robin over the XCDs
    const int qr = (((slot / G) * 8 + xcd) * G + slot % G) * T;
    if (qr >= a.ntiles) return;                                              // (uniform over the workgroup)
    const int nt = min(T, a.ntiles - qr);
    const int q0 = tile0 + qr;
    const int32_t r0 = q0 * KR_TILE;                                         // (the launch checks xlen + 2 tiles < 2^31: 32-bit element indices)
    // ---- round trip 1: ids of the run, the window of x, the tables
    // The kernel is bound by VALU issue (a 64-lane instruction takes four cycles whatever it does; 770 of them per wave and run
    // before this paragraph, 45 % selects and compares): indices are 32-bit, and a run that lies INSIDE x with its whole window and
    // its far operands -- all but the first and last few of a box -- takes a path without a single clamp (uniform over the workgroup).
    unsigned ids[T];
#pragma unroll
    for (int k = 0; k < T; ++k) ids[k] = k < nt ? *reinterpret_cast<const unsigned*>(a.pid + (size_t)(q0 + k) * KR_TILE + 2 * t) : 0u;
    constexpr int NP = (T * KR_TILE + 2 * 1024 + 4 + 2 * KR_T - 1) / (2 * KR_T);   // pairs per lane at most (n <= 1024)
    const int npairs = XS / 2;
    const int32_t e0 = r0 - n - 2;                                           // element of x staged at xs[0] (even)
    const int32_t xsafe = (int32_t)a.xsafe;
    const bool inside = e0 >= 0 && e0 + XS <= xsafe && (!UFAR || ((int64_t)r0 + far_lo >= 0 && (int64_t)r0 + T * KR_TILE + far_hi <= (int64_t)xsafe));
    // the window goes STRAIGHT into LDS (global_load_lds_dwordx4, gfx950's LDS-DMA: destination = a wave-uniform base + 16 bytes per
    // lane, which is exactly the window's layout): no staging registers, no LDS store instructions
    const int wbase = __builtin_amdgcn_readfirstlane(t & ~63);
    uint2 ma[T], mb[T]; v2d lo[T], hi[T]; d2 dv[T];
    if (inside) {
        const double* xw = a.x + e0 + 2 * t;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (t + i * KR_T < npairs)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xw + 2 * i * KR_T),
                                                 (__attribute__((address_space(3))) void*)(xs + 2 * (i * KR_T + wbase)), 16, 0, 0);
        }
        if constexpr (UFAR) {
            const double* xl = a.x + (r0 + 2 * t) + far_lo; const double* xh = a.x + (r0 + 2 * t) + far_hi;
#pragma unroll
            for (int k = 0; k < T; ++k) {
#if defined(KR_STAGE_ABL) && (KR_STAGE_ABL & 2)
                lo[k].x = 1.0; lo[k].y = 2.0; hi[k].x = 3.0; hi[k].y = 4.0;  // timing only: no far operands
#else
                lo[k] = *reinterpret_cast<const v2d*>(xl + k * KR_TILE);
                hi[k] = *reinterpret_cast<const v2d*>(xh + k * KR_TILE);
#endif
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pi = t + i * KR_T;
            if (pi < npairs) {
                const int32_t e = min(max(e0 + 2 * pi, 0), xsafe);             // outside x: any valid pair (those operands are absent entries)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.x + e),
                                                 (__attribute__((address_space(3))) void*)(xs + 2 * (i * KR_T + wbase)), 16, 0, 0);
            }
        }
        if constexpr (UFAR) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const int64_t row = (int64_t)r0 + k * KR_TILE + 2 * t;
                lo[k] = *reinterpret_cast<const v2d*>(a.x + min(max(row + far_lo, (int64_t)0), (int64_t)xsafe));
                hi[k] = *reinterpret_cast<const v2d*>(a.x + min(max(row + far_hi, (int64_t)0), (int64_t)xsafe));
            }
        }
    }
    if constexpr (UFAR && NQ > 0 && !CENTER) {
#pragma unroll
        for (int k = 0; k < T; ++k) { dv[k].a = 0.0; dv[k].b = 0.0; if (k < nt) dv[k] = ld2(a.dvec, r0 + k * KR_TILE + 2 * t); }
    }
    for (int i = t; i < a.npat; i += KR_T) meta[i] = reinterpret_cast<const uint2*>(a.pmeta)[i];
    for (int i = t; i < a.ntab; i += KR_T) { poff[i] = a.poff[i]; pval[i] = a.pval[i]; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the window has landed (the compiler does not count LDS-DMA requests)
    __syncthreads();
    // ---- round trip 2 (!UFAR): the far operands of every tile of the run (and the fused dot's vector when it is not x itself)
#pragma unroll
    for (int k = 0; k < T; ++k) {
        const int32_t row = r0 + k * KR_TILE + 2 * t;
        const bool va = k < nt && row < a.nrows, vb = k < nt && row + 1 < a.nrows;
        ma[k] = va ? meta[ids[k] & 0xffffu] : make_uint2(0u, 0u);
        mb[k] = vb ? meta[ids[k] >> 16] : make_uint2(0u, 0u);
        if constexpr (UFAR) continue;
        const int ba = ma[k].x & 0xffffu, bb = mb[k].x & 0xffffu;
        lo[k].x = 0.0; lo[k].y = 0.0; hi[k].x = 0.0; hi[k].y = 0.0;
        const bool a0 = ma[k].y & 1u, b0 = mb[k].y & 1u, a6 = (ma[k].y >> 6) & 1u, b6 = (mb[k].y >> 6) & 1u;
#if defined(KR_STAGE_ABL) && (KR_STAGE_ABL & 2)
        if (t == 12345) lo[k] = *reinterpret_cast<const v2d*>(a.x + row + poff[ba]);        // timing only: no far operands
        if (t == 12345) hi[k] = *reinterpret_cast<const v2d*>(a.x + row + poff[ba + 6]);
        continue;
#endif
        if (a0 && b0 && ba == bb) lo[k] = *reinterpret_cast<const v2d*>(a.x + row + poff[ba]);
        else { if (a0) lo[k].x = a.x[row + poff[ba]]; if (b0) lo[k].y = a.x[row + 1 + poff[bb]]; }
        if (a6 && b6 && ba == bb) hi[k] = *reinterpret_cast<const v2d*>(a.x + row + poff[ba + 6]);
        else { if (a6) hi[k].x = a.x[row + poff[ba + 6]]; if (b6) hi[k].y = a.x[row + 1 + poff[bb + 6]]; }
        if constexpr (NQ > 0 && !CENTER) { dv[k].a = 0.0; dv[k].b = 0.0; if (k < nt) dv[k] = ld2(a.dvec, row); }
    }
    // ---- tile after tile out of LDS
#pragma unroll
    for (int k = 0; k < T; ++k) {
        if (k >= nt) break;                                                  // (uniform)
        const int32_t row = r0 + k * KR_TILE + 2 * t;
        const bool va = row < a.nrows, vb = row + 1 < a.nrows;
        const int j = k * KR_TILE + 2 * t + n + 2;                           // xs[j] = x[row]
        const v2d A = *reinterpret_cast<const v2d*>(xs + j - 2), B = *reinterpret_cast<const v2d*>(xs + j), C = *reinterpret_cast<const v2d*>(xs + j + 2);
        const v2d M = *reinterpret_cast<const v2d*>(xs + j - n), P = *reinterpret_cast<const v2d*>(xs + j + n);
        v2d e[7];
        e[0] = lo[k]; e[1] = M; e[2].x = A.y; e[2].y = B.x; e[3] = B; e[4].x = B.y; e[4].y = C.x; e[5] = P; e[6] = hi[k];
        const double* tva = pval + (ma[k].x & 0xffffu); const double* tvb = pval + (mb[k].x & 0xffffu);
        const unsigned ka = ma[k].y, kb = mb[k].y;
        double s0 = 0.0, s1 = 0.0;
        // (a scalar branch per entry for the entries every row of the wave has -- no select then -- was tried: 114 branches per run cost
        // more than the selects they save, 0.59 -> 0.64 ms at 512^3; so was hoisting the masks' compares and the table values out of
        // the tile loop when a lane's ids repeat over the run, with the values as scalars when the wave has one base: 486 instead of 770
        // VALU instructions per wave and run, and no faster -- 0.576-0.580 ms, the extra paths cost the kernel a wave per SIMD.
        // rocprofv3 --pmc: VALU busy 47 %, LDS 15 %, 21 % of the wave cycles waiting for memory)
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            const double ta = s0 + tva[u] * e[u].x, tb = s1 + tvb[u] * e[u].y;
            s0 = ((ka >> u) & 1u) ? ta : s0;
            s1 = ((kb >> u) & 1u) ? tb : s1;
        }
#if defined(KR_STAGE_ABL) && (KR_STAGE_ABL & 1)
        if (s0 == 1.23456789e-300) a.y[row] = s0;                           // timing only: no y traffic
#else
        if (vb) st2(a.y, row, s0, s1);
        else if (va) a.y[row] = s0;
#endif
        if constexpr (NQ > 0) {
            // the tile's partials in the library's order (thread: its two rows; wave: butterfly; workgroup: the four waves in
            // turn) -- the cross-wave step of all T tiles of the run meets at ONE barrier below
            double acc[NQ];
            d2 d;
            if constexpr (CENTER) { d.a = B.x; d.b = B.y; } else d = dv[k];
            acc[0] = 0.0;
            if (va) acc[0] = acc[0] + d.a * s0;
            if (vb) acc[0] = acc[0] + d.b * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                if (va) acc[1] = acc[1] + s0 * s0;
                if (vb) acc[1] = acc[1] + s1 * s1;
            }
#pragma unroll
            for (int kk = 0; kk < NQ; ++kk) {
                const double wsum = wave_butterfly(acc[kk]);
                if ((t & 63) == 0) red[(k * NQ + kk) * (KR_T / 64) + (t >> 6)] = wsum;
            }
        }
    }
    if constexpr (NQ > 0) {
        __syncthreads();
        if (t < nt * NQ) {                                                   // thread k * NQ + kk: tile q0 + k, quantity kk
            const int k = t / NQ, kk = t % NQ;
            double sum = red[t * (KR_T / 64)];
#pragma unroll
            for (int w2 = 1; w2 < KR_T / 64; ++w2) sum = sum + red[t * (KR_T / 64) + w2];
            a.partials[kk * a.pstride + q0 + k] = sum;
        }
    }
}

// Runs per XCD group of the staged-window kernels (spmv_pattern_stage_kernel / _fuse_kernel: groups of G consecutive runs round-robin over the 8
// XCDs): groups of 4 once the launch is well beyond one wave of workgroups (in-process A/B inside CG: 512^3 +1.2 %, 256^3 +-0, 192^3 +4 %, but
// 128^3 -19 %; 8: +1.3 / -4.5 % at 512^3 / 256^3; 32: -2 / -21 %).  The FUSED kernel reads its far operands (rows +- one plane) from TWO vectors:
// when a grid plane (far_hi rows) is a whole number of groups per XCD -- G = plane / (8 T tiles) -- the same (i, j) strip of every plane lands on
// the same XCD, whose L2 then streams those rows itself: 512^3 fused CG, G = 16 against 4: 613 against 596 it/s (three interleaved rounds,
// tools/cg_fuse_knobs.py).  (Walking SUB-strips of R runs plane by plane -- resident runs then neighbours in k -- was measured and loses: R = 1 / 2 / 4 /
// 8 / 16: 563 / 578 / 590 / 603 / 616 it/s; a run that jumps a plane every few runs costs DRAM page locality more than the far operands' L2 hits give.
// The marching mode, fuse_march_plan below, is the form of that idea that pays: the workgroup ITSELF walks the planes and keeps the far operands in its
// LDS windows and registers, with whole planes' worth of neighbouring strips resident at every step -- 512^3: 631-636 against 611-620 it/s.)  The plain staged kernel does not care at 512^3 (0.500-0.508 ms for G = 1 .. 16, tools/stage_group_ab.py) and loses
// with large groups at 384^3 (0.26 against 0.21 ms), so it keeps 4.
int stage_group_default(kryst_csr_t a, int64_t nruns, int T, bool fused) {
    if (nruns < 2048) return 1;
    const int64_t plane = a->pat_far_uniform ? (int64_t)a->pat_far_hi : 0, per = (int64_t)KR_TILE * 8 * T;
    if (fused && plane > 0 && plane % per == 0 && plane / per >= 2 && plane / per <= 64) return (int)(plane / per);
    return 4;
}
// the near operands staged in LDS, runs of T tiles per workgroup (natural tile order, no halo columns); interior: a rank's contiguous interior tiles
int32_t enqueue_pattern_stage(kryst_csr_t a, SpmvArgs g, int nq, bool interior) {
    kryst_ctx_t ctx = a->ctx;
    const int32_t tile0 = interior ? (int32_t)a->interior_first : 0;
    const int64_t ntiles = g.ntiles;
    g.tiles = nullptr;
    // runs of 4 tiles for large vectors, of 2 below half a gigabyte (63 registers, 8 waves per SIMD: 512^3 2 % slower, 256^3 3.5 % faster)
    const int T = env_int("KRYST_SPMV_STAGE_T", a->nrows * 8 > (512ll << 20) ? 4 : 2) <= 2 ? 2 : 4;     // (in CG: 128^3 +1.2 %, 192^3 +2 %, 256^3 +0.6 %, 320^3 +1.3 % with 2)
    const int32_t n_ = a->pat_stage_n;
    const StagedLds l = staged_lds(a, 1, 12, 1, T, nq > 0 ? nq : 1);
    g.pat_red_off = (int32_t)l.red_off;
    g.xsafe = xsafe_of(a);
    const int64_t nruns = (ntiles + T - 1) / T;
    g.group = std::max(1, env_int("KRYST_SPMV_STAGE_GROUP", stage_group_default(a, nruns, T, false)));
    const int64_t per_xcd = ((nruns + 7) / 8 + g.group - 1) / g.group * g.group;      // slots per XCD: whole groups
    const dim3 sgrid((unsigned)(per_xcd * 8)), block(KR_T);
    const bool center = nq > 0 && g.dvec == g.x;
    const bool ufar = (a->pat_far_uniform || (interior && a->pat_far_interior)) && env_int("KRYST_SPMV_STAGE_UFAR", 1) != 0;
    const int32_t far_lo = ufar ? a->pat_far_lo : 0, far_hi = ufar ? a->pat_far_hi : 0;
    return by_nq(nq, [&](auto NQ) { by_int<2, 4>(T, [&](auto T_) { by_bool(ufar, [&](auto UF) {
        auto launch = [&](auto C) { hipLaunchKernelGGL((spmv_pattern_stage_kernel<NQ(), T_(), C(), UF()>), sgrid, block, l.bytes, ctx->s_main, g, n_, far_lo, far_hi, tile0); };
        if constexpr (NQ() > 0) by_bool(center, launch); else launch(std::false_type{});
    }); }); });
}

int32_t enqueue_pattern(kryst_csr_t a, SpmvArgs g, bool halo, int nq, bool ordered) {
    kryst_ctx_t ctx = a->ctx;
    // a workgroup loads the tables once and walks one run of 8 consecutive tiles (next tile's ids prefetched); runs go
    // round-robin over the XCDs.  Measured at 512^3 (round-2 sweeps and --pmc passes, profiles/r02/): 0.70 ms and 1.6 GB of reads
    // per launch, against 0.79 ms and 4.1 GB for a strided persistent grid whose fast workgroups run ahead.
    g.group = ordered ? 8 : std::max(1, env_int("KRYST_SPMV_GROUP", 8));
    const int64_t pchunk = (((int64_t)g.ntiles + 7) / 8 + g.group - 1) / g.group * g.group;      // an XCD's share is a whole number of runs
    g.xcd_chunk = (int32_t)pchunk;
    g.tpw = std::max(1, env_int("KRYST_SPMV_PATTERN_TPW", 8));
    const int64_t pper = (pchunk + g.tpw - 1) / g.tpw;
    const dim3 pgrid((unsigned)(pper * 8)), block(KR_T);
    const int U = a->pat_unroll;
    const size_t tab = (size_t)(a->ntab + U + 1) * 12 + (size_t)a->npat * 8;
    g.pat_red_off = (int32_t)((tab + 15) & ~(size_t)15);
    g.nloc8 = (int32_t)(a->nrows * 8);
    const size_t lds = (size_t)g.pat_red_off + sizeof(double) * (size_t)(nq > 0 ? nq : 1) * (KR_T / 64);
    const bool gen3 = !halo && a->pat_diag3 && env_int("KRYST_SPMV_REUSE_DIAG", 1);      // generator-made operator, interior tiles
    const bool reuse_diag = gen3 && nq > 0 && g.dvec == g.x;
    // the instance: 0 (U, SINGLE) = (8, false); 1 (8, true); 2 (7, true); 3 (7, true) with MERGE3; 4 ... and CENTER = 3
    const int inst = U != 7 ? (a->pat_single ? 1 : 0) : reuse_diag ? 4 : gen3 ? 3 : 2;
    return by_nq(nq, [&](auto NQ) { by_bool(halo, [&](auto H) { by_int<0, 1, 2, 3, 4>(inst, [&](auto I) {
        hipLaunchKernelGGL((spmv_pattern_kernel<NQ(), H(), (I() < 2 ? 8 : 7), (I() > 0), (I() == 4 ? 3 : -1), (I() >= 3)>), pgrid, block, lds, ctx->s_main, g); }); }); });
}

}  // namespace kr
