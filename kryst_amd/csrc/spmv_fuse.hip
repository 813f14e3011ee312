// The staged-window CSR-P16 kernels fused with CG's vector passes -- spmv_pattern_fuse_kernel (the direction pass inside the SpMV; fuse_march: its marching
// mode), cg_recompute_residual_kernel (the residual pass forms A p again) -- their plans, launches and hooks.  spmv.hip: the contract, the staged form's predicates.
#include "spmv.h"
#include "march_window.h"

namespace kr {
// KRYST_SPMV_PID_REUSE (the marching kernels; csr_create.hip: build_pid_same): the pid_same flags of a strip's T tiles in the plane whose strip starts
// at row r0, as one word -- byte k: tile r0 / 512 + k, a multiple of T, so the word is aligned; 0 ("never the same") without a table.  The address
// depends on the workgroup's strip and the plane alone: the value is uniform, and so is every branch on it.
template <int T>
__device__ __forceinline__ unsigned pid_same_word(const SpmvArgs& a, const int32_t r0) {
    if (!a.pid_same) return 0u;
    const uint8_t* f = a.pid_same + r0 / KR_TILE;
    unsigned w;
    if constexpr (T == 4) w = *reinterpret_cast<const unsigned*>(f);
    else w = *reinterpret_cast<const unsigned short*>(f);
    return w;
}

// CG / PCG with the direction pass INSIDE the SpMV (spmv_pattern_fuse_kernel; round 5).  An iteration used to end with the
// direction pass  x += alpha p, p = z + beta p  (5 vector words per row) and the next one began with the SpMV reading that p again.  Here the
// staged-window kernel forms p itself: its window fill reads z and p_old instead of p and stores  z + beta p_old  -- cg.rs:274-276 /
// pcg.rs:215-217, the same un-fused multiply and add per element, so the same bits -- into LDS; the rows the run OWNS also go to p_new in
// memory, and the deferred  x += alpha p_old  (cg.rs:207-209) rides on the p_old values the fill holds anyway.  The far operands (rows +-
// far_lo / far_hi away) are formed the same way from z and p_old there: a row's p_new is computed by up to three workgroups, from the same
// operands in the same order.  p_old and p_new are DIFFERENT arrays (the solver ping-pongs): nobody reads what another workgroup writes.
// Per row: z, p_old, x read, p_new, x, y written + the pattern id -- 50 bytes instead of 40 (direction) + 18 (SpMV), and one launch fewer.
// (With x in batches, XU = false: z, p_old read, p_new, y written + the id -- 34; and the marching instance with YS = false, which CG takes when its
// residual pass forms A p again (cg_recompute_residual_kernel below), writes p_new alone -- 26.)
//   xpend == it - 1: the x update of the previous iteration is owed (always, unless the solve ended earlier and it has been paid);
//   done: the solve has ended -- only the owed x update happens, nothing else is touched.
struct FuseArgs { const double* z; const double* p_old; double* p_new; double* xvec; const double* alpha; const double* beta; const long long* xpend; long long it; };
// NMAX: the line length the instance is built for (the window's pairs per lane are a compile-time count): 512 or 1024
// XU: the deferred x update rides on this kernel (false: the solver updates x in batches, cg_pcg.hip: XBatchOp -- no registers held for x)
// (measured and not kept, round 5: runs of 8 tiles -- 166 registers, 3 waves per SIMD: 582-590 against 596 it/s; amdgpu_waves_per_eu(5): four
// spilled registers, 565 against 596)
//
// MARCH (the marching mode; launch_spmv_fused_impl: fuse_march_plan decides).  The far operands of a row are the SAME (i, j) row one plane below and
// above, so a workgroup that keeps its strip of R = 512 T consecutive rows of a plane and walks a segment of S planes along k holds them itself:
// e[6] is read from the window of plane s + 1 at the LDS index of B, and e[0] is the lane's own B pair of plane s - 1, carried in registers (the
// lane-to-row mapping is the same in every step).  Only the first and the last plane of a segment form a far operand from z and p_old in memory
// (clamped at the ends of the box), as the un-marched kernel does for every tile: per own line 1 + 2 n / R + 2 / S lines of z and p_old are
// requested instead of 3 + (2 n + 4) / R, and the halo lines are a neighbouring strip's own lines on the same XCD.
//   LDS: TWO windows of R + 2 n doubles (march_window.h: from row r0 - n; a lane requests its own pairs first, then its share of the halo), W(s) and W(s + 1).  A step is
//     a. request W(s + 2): z, p_old (and the owed x) of the whole window into REGISTERS, and the ids of plane s + 1 -- of those tiles whose pid_same
//        flag is clear: the others repeat the plane below and stay in ids[k], KRYST_SPMV_PID_REUSE -- in flight under b.  (Not by
//        LDS-DMA as the un-marched fill: beside a pending DMA the compiler drains vmcnt(0) before the first LDS read of b. and before every use of
//        an ordinary load, which serialises the step; plain loads are counted exactly.  Both forms read at the same rate.)
//     b. the tiles of plane s out of W(s) and W(s + 1), y stored (YS; not when the residual pass recomputes it), partials per wave into red;
//     barrier 1: every wave has read W(s) for the last time;
//     c. the cross-wave step of the partials (threads 0 .. T NQ - 1 out of red); p_new = z + beta p_old into the buffer that held W(s), own
//        rows to p_new in memory, with the owed x update;
//     barrier 2: W(s + 2) is complete; the buffers change roles.
//   Every barrier against the loop: c. of step s overwrites W(s), whose last reads (A, B, C, M, P of b.) are before barrier 1 of step s, W(s + 1)
//   is only read; b. of step s + 1 reads W(s + 2) after barrier 2 of step s; red is written in b. of step s + 1, after barrier 2 of step s, which
//   its readers of c. reach only afterwards.  Both barriers are executed in every step by every wave: the branches around them depend on s and the
//   segment's length alone (uniform over the workgroup).
//   Grid: strips / 8 (rounded up) neighbouring strips per XCD, segment after segment: the workgroups resident on an XCD are neighbouring strips of
//   the same planes (contiguous in memory at every step, halo lines shared in that XCD's L2), and a strip is on the same XCD in every segment.
//   Which workgroup computes a tile changes and nothing else: per-element arithmetic, entry order, absent-entry selects and the per-tile partials
//   (thread, wave butterfly, the four waves in turn, partials[tile]) are the un-marched kernel's -- the same bits.
//   Registers: 156 at T = 4 without the x update (164 with windows of R + 2 n + 4 doubles in plain lane order; the un-marched instance: 98) -- a whole window of z and p_old is held across b. -- i.e. three waves per
//   SIMD, one more than the two workgroups per CU the launch keeps resident need.  Measured at 512^3 (profiles/march/): HBM traffic 39.9 -> 35.4 bytes
//   per row (model 34), the kernel 879 -> 843 us, CG 601 -> 628 it/s.
//   a.group: strips per XCD; a.xcd_chunk: S; a.tpw: strips per plane; far_hi == -far_lo == the plane; every strip and every plane is whole.
template <int NQ, int T, int NMAX, bool XU, bool YS>
__device__ __forceinline__ void fuse_march(const SpmvArgs& a, const FuseArgs& f, const int32_t n, const int32_t plane, unsigned char* smem, const bool ended, const bool owed) {
    const int XS = march_window_elems(n, T);                                 // elements of one window (even)
    double* win = reinterpret_cast<double*>(smem);
    uint2* meta = reinterpret_cast<uint2*>(win + 2 * XS);
    double* pval = reinterpret_cast<double*>(meta + a.npat);
    double* red = reinterpret_cast<double*>(smem + a.pat_red_off);
    const int t = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int spx = a.group, S = a.xcd_chunk;
    const int strip = xcd * spx + slot % spx, k0 = (slot / spx) * S;
    const int nplanes = a.nrows / plane;
    if (strip >= a.tpw || k0 >= nplanes) return;                             // (uniform over the workgroup)
    const int ns = min(S, nplanes - k0);                                     // planes of this segment (the last one may be shorter)
    const int32_t rbeg = k0 * plane + strip * (T * KR_TILE);                 // first row of the strip in the segment's first plane
    const double al = *f.alpha, be = *f.beta;
    if (ended) {                                                             // (uniform) only x += alpha p_old is still owed, on the segment's own rows
        for (int s = 0; s < ns; ++s) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const int32_t row = rbeg + s * plane + k * KR_TILE + 2 * t;
                const d2 pp = ld2(f.p_old, row), xx = ld2(f.xvec, row);
                st2(f.xvec, row, xx.a + al * pp.a, xx.b + al * pp.b);
            }
        }
        return;
    }
    constexpr int NP = march_window_requests(NMAX, T, KR_T);                 // requests per lane at most (n <= NMAX)
    const int32_t xsafe = (int32_t)a.xsafe;
    v2d zz[NP], po[NP], xo[XU ? T : 1];
    // a window's requests (r0: the strip's first row in that plane; march_window.h: requests 0 .. T - 1 are the lane's own pairs, the others its
    // share of the halo).  Every lane loads NP pairs: a request without a pair repeats the lane's first own pair (and is dropped by write_window) -- no
    // branch around a load
    auto request = [&](const int32_t r0) {
        const int32_t e0 = r0 - n;                                           // element at the window's [0] (even)
        const bool inside = e0 >= 0 && e0 + XS <= xsafe;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = march_window_request(t, i, n, T, KR_T).lds, o = q < 0 ? march_window_request(t, 0, n, T, KR_T).lds : q;
            const int32_t e = inside ? e0 + o : min(max(e0 + o, 0), xsafe);  // outside x: any valid pair (those operands are absent entries)
            po[i] = *reinterpret_cast<const v2d*>(f.p_old + e);
            zz[i] = *reinterpret_cast<const v2d*>(f.z + e);
            if constexpr (XU) { if (i < T) { xo[i].x = 0.0; xo[i].y = 0.0; if (owed) xo[i] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(f.xvec + e)); } }     // (own rows are never clamped; read once)
        }
    };
    // p_new = z + beta p_old (cg.rs:274-276 / pcg.rs:215-217, un-fused multiply and add) into the window; own rows also to memory, with their x update
    auto write_window = [&](const int32_t r0, double* xs) {
        const int32_t e0 = r0 - n;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = march_window_request(t, i, n, T, KR_T).lds;
            if (q >= 0) {
                v2d pn; pn.x = zz[i].x + be * po[i].x; pn.y = zz[i].y + be * po[i].y;
                *reinterpret_cast<v2d*>(xs + q) = pn;
                if (i < T) {                                                // (an own pair)
                    st2(f.p_new, e0 + q, pn.x, pn.y);
                    if constexpr (XU) { if (owed) st2(f.xvec, e0 + q, xo[i].x + al * po[i].x, xo[i].y + al * po[i].y); }
                }
            }
        }
    };
    // a far operand the segment does not hold (below its first plane, above its last): formed the same way from z and p_old there
    auto far_pair = [&](const int64_t row) {
        const int64_t c = min(max(row, (int64_t)0), (int64_t)xsafe);
        const v2d zf = *reinterpret_cast<const v2d*>(f.z + c), pf = *reinterpret_cast<const v2d*>(f.p_old + c);
        v2d r; r.x = zf.x + be * pf.x; r.y = zf.y + be * pf.y;
        return r;
    };
    unsigned ids[T], idn[T];
    v2d prev[T], hi[T];
    // the flags of plane s + 1, read one step ahead like the ids they stand for (the segment's first plane always loads its ids)
    unsigned same = ns > 1 ? pid_same_word<T>(a, rbeg + plane) : 0u, samen = 0u;
    // ---- the segment's first two windows
#pragma unroll
    for (int k = 0; k < T; ++k) { ids[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a.pid + (size_t)rbeg + k * KR_TILE + 2 * t)); idn[k] = 0u; }
    double* w0 = win; double* w1 = win + XS;                                 // W(s), W(s + 1)
    request(rbeg);
#pragma unroll
    for (int k = 0; k < T; ++k) { prev[k] = far_pair((int64_t)rbeg + k * KR_TILE + 2 * t - plane); hi[k].x = 0.0; hi[k].y = 0.0; }
    for (int i = t; i < a.npat; i += KR_T) meta[i] = reinterpret_cast<const uint2*>(a.pmeta)[i];
    for (int i = t; i < a.ntab; i += KR_T) pval[i] = a.pval[i];
    write_window(rbeg, w0);
    if (ns > 1) {
        request(rbeg + plane);
        write_window(rbeg + plane, w1);
    }
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const int32_t r0 = rbeg + s * plane;
        const bool last = s + 1 == ns, fill = s + 2 < ns;                   // (uniform)
        // a.
        if (fill) request(r0 + 2 * plane);
        samen = fill ? pid_same_word<T>(a, r0 + 2 * plane) : 0u;
        // byte k set: the ids of tile k repeat the plane below and stay in ids[k] -- no load now, no hand-over at the step's end (uniform; the
        // segment's last plane requests nothing)
        const unsigned sw = last ? ~0u : __builtin_amdgcn_readfirstlane(same);
        if (!last) {
#pragma unroll
            for (int k = 0; k < T; ++k)
                if (!((sw >> (8 * k)) & 1u)) idn[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a.pid + (size_t)(r0 + plane) + k * KR_TILE + 2 * t));
        } else {
#pragma unroll
            for (int k = 0; k < T; ++k) hi[k] = far_pair((int64_t)r0 + k * KR_TILE + 2 * t + plane);
        }
        // b. tile after tile out of LDS (spmv_pattern_stage_kernel's arithmetic)
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int32_t row = r0 + k * KR_TILE + 2 * t;
            const uint2 ma = meta[ids[k] & 0xffffu], mb = meta[ids[k] >> 16];
            const int j = march_window_tile_offset(n, k) + 2 * t;            // w0[j] = p_new[row], w1[j] = p_new[row + plane]
            const v2d A = *reinterpret_cast<const v2d*>(w0 + j - 2), B = *reinterpret_cast<const v2d*>(w0 + j), C = *reinterpret_cast<const v2d*>(w0 + j + 2);
            const v2d M = *reinterpret_cast<const v2d*>(w0 + j - n), P = *reinterpret_cast<const v2d*>(w0 + j + n);
            const v2d U = *reinterpret_cast<const v2d*>(w1 + j);             // (the segment's last plane: not used)
            v2d e[7];
            e[0] = prev[k]; e[1] = M; e[2].x = A.y; e[2].y = B.x; e[3] = B; e[4].x = B.y; e[4].y = C.x; e[5] = P;
            e[6].x = last ? hi[k].x : U.x; e[6].y = last ? hi[k].y : U.y;
            prev[k] = B;
            const double* tva = pval + (ma.x & 0xffffu); const double* tvb = pval + (mb.x & 0xffffu);
            const unsigned ka = ma.y, kb = mb.y;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int u = 0; u < 7; ++u) {
                const double ta = s0 + tva[u] * e[u].x, tb = s1 + tvb[u] * e[u].y;
                s0 = ((ka >> u) & 1u) ? ta : s0;
                s1 = ((kb >> u) & 1u) ? tb : s1;
            }
            if constexpr (YS) st2(a.y, row, s0, s1);                         // (!YS: the residual pass forms A p again, cg_recompute_residual_kernel)
            double acc[NQ];
            acc[0] = 0.0;
            acc[0] = acc[0] + B.x * s0;
            acc[0] = acc[0] + B.y * s1;
            if constexpr (NQ > 1) {
                acc[1] = 0.0;
                acc[1] = acc[1] + s0 * s0;
                acc[1] = acc[1] + s1 * s1;
            }
#pragma unroll
            for (int kk = 0; kk < NQ; ++kk) {
                const double wsum = wave_butterfly(acc[kk]);
                if ((t & 63) == 0) red[(k * NQ + kk) * (KR_T / 64) + (t >> 6)] = wsum;
            }
        }
        __syncthreads();                                                     // barrier 1
        // c.
        if (t < T * NQ) {                                                    // thread k * NQ + kk: tile r0 / 512 + k, quantity kk
            const int k = t / NQ, kk = t % NQ;
            double sum = red[t * (KR_T / 64)];
#pragma unroll
            for (int w = 1; w < KR_T / 64; ++w) sum = sum + red[t * (KR_T / 64) + w];
            a.partials[kk * a.pstride + r0 / KR_TILE + k] = sum;
        }
        if (fill) write_window(r0 + 2 * plane, w0);
        __syncthreads();                                                     // barrier 2
#pragma unroll
        for (int k = 0; k < T; ++k) if (!((sw >> (8 * k)) & 1u)) ids[k] = idn[k];       // (a hand-over, not a copy back and forth: the compiler gathers the plain copies into one register tuple)
        same = samen;
        double* w = w0; w0 = w1; w1 = w;
    }
}

// YS (marching instances only): y is stored; false when the residual pass recomputes A p from p_new (launch_spmv_fused with y == nullptr)
template <int NQ, int T, int NMAX, bool XU, bool MARCH = false, bool YS = true>
__global__ __launch_bounds__(KR_T) void spmv_pattern_fuse_kernel(const SpmvArgs a, const FuseArgs f, const int32_t n, const int32_t far_lo, const int32_t far_hi) {
    const bool ended = a.done && *a.done;
    const bool owed = XU && *f.xpend == f.it - 1;
    if (ended && !owed) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (MARCH) { fuse_march<NQ, T, NMAX, XU, YS>(a, f, n, far_hi, smem, ended, owed); return; }
    const int XS = T * KR_TILE + 2 * n + 4;                                  // staged elements (even)
    double* xs = reinterpret_cast<double*>(smem);                            // p_old's window, overwritten in place by p_new's
    uint2* meta = reinterpret_cast<uint2*>(xs + XS);
    double* pval = reinterpret_cast<double*>(meta + a.npat);
    double* red = reinterpret_cast<double*>(smem + a.pat_red_off);
    const int t = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int G = a.group;
    const int qr = (((slot / G) * 8 + xcd) * G + slot % G) * T;
    if (qr >= a.ntiles) return;
    const int nt = min(T, a.ntiles - qr);
    const int q0 = qr;
    const int32_t r0 = q0 * KR_TILE;
    const double al = *f.alpha, be = *f.beta;
    if (ended) {                                                             // (uniform) only x += alpha p_old is still owed, on the run's own rows
#pragma unroll
        for (int k = 0; k < T; ++k) {
            if (k >= nt) break;
            const int32_t row = r0 + k * KR_TILE + 2 * t;
            const d2 pp = ld2(f.p_old, row), xx = ld2(f.xvec, row);
            st2(f.xvec, row, xx.a + al * pp.a, xx.b + al * pp.b);
        }
        return;
    }
    unsigned ids[T];
#pragma unroll
    // (ids and x are read once: nontemporal, not in the way of z / p_old in L2 -- alternating processes of two builds, 4 rounds: 553 against 552 it/s, no
    // measurable difference beside the 2 % a process's allocation makes; kept because it is the right hint)
    for (int k = 0; k < T; ++k) ids[k] = k < nt ? __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a.pid + (size_t)(q0 + k) * KR_TILE + 2 * t)) : 0u;
    constexpr int NP = (T * KR_TILE + 2 * NMAX + 4 + 2 * KR_T - 1) / (2 * KR_T);   // pairs per lane at most (n <= NMAX)
    const int npairs = XS / 2;
    const int32_t e0 = r0 - n - 2;                                           // element staged at xs[0] (even)
    const int32_t xsafe = (int32_t)a.xsafe;
    const bool inside = e0 >= 0 && e0 + XS <= xsafe && (int64_t)r0 + far_lo >= 0 && (int64_t)r0 + T * KR_TILE + far_hi <= (int64_t)xsafe;
    const int own_lo = (n + 2) / 2, own_hi = own_lo + nt * (KR_TILE / 2);   // window pairs that are rows of this run
    // ---- the window: p_old straight into LDS (LDS-DMA, lane t's pairs t + 256 i land where lane t reads them back), z into registers
    const int wbase = __builtin_amdgcn_readfirstlane(t & ~63);
    v2d zz[NP], xo[XU ? NP : 1];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pi = t + i * KR_T;
        zz[i].x = 0.0; zz[i].y = 0.0; if constexpr (XU) xo[i] = zz[i];
#ifdef KR_TUNING
        if (pi < npairs && (!(a.abl & 2) || (pi >= own_lo && pi < own_hi))) {   // abl 2 (timing only): the window's halo is not loaded
#else
        if (pi < npairs) {
#endif
            const int32_t e = inside ? e0 + 2 * pi : min(max(e0 + 2 * pi, 0), xsafe);     // outside x: any valid pair (those operands are absent entries)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(f.p_old + e),
                                             (__attribute__((address_space(3))) void*)(xs + 2 * (i * KR_T + wbase)), 16, 0, 0);
            zz[i] = *reinterpret_cast<const v2d*>(f.z + e);
            if constexpr (XU) { if (owed && pi >= own_lo && pi < own_hi) xo[i] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(f.xvec + e)); }     // (own rows are never clamped; read once)
        }
    }
    for (int i = t; i < a.npat; i += KR_T) meta[i] = reinterpret_cast<const uint2*>(a.pmeta)[i];
    for (int i = t; i < a.ntab; i += KR_T) pval[i] = a.pval[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // this wave's share of the window has landed (the compiler does not count LDS-DMA requests)
    // p_new = z + beta p_old (cg.rs:274-276 / pcg.rs:215-217, un-fused multiply and add), in place; own rows also to memory, with their x update
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int pi = t + i * KR_T;
        if (pi < npairs) {
            const v2d po = *reinterpret_cast<const v2d*>(xs + 2 * pi);
            v2d pn; pn.x = zz[i].x + be * po.x; pn.y = zz[i].y + be * po.y;
            *reinterpret_cast<v2d*>(xs + 2 * pi) = pn;
            if (pi >= own_lo && pi < own_hi) {
                const int32_t row = e0 + 2 * pi;
#ifdef KR_TUNING
                if (a.abl & 8) { if (pn.x == 1.23456789e-300) st2(f.p_new, row, pn.x, pn.y); } else      // abl 8 (timing only): no p_new / x stores
#endif
                { st2(f.p_new, row, pn.x, pn.y);
                if constexpr (XU) { if (owed) st2(f.xvec, row, xo[i].x + al * po.x, xo[i].y + al * po.y); } }
            }
        }
    }
    // the far operands of every tile of the run, formed the same way from z and p_old there (requested now: in flight across the barrier)
    v2d lo[T], hi[T];
    {
        v2d zl[T], pl[T], zh[T], ph[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int64_t row = (int64_t)r0 + k * KR_TILE + 2 * t;
            const int64_t cl = inside ? row + far_lo : min(max(row + far_lo, (int64_t)0), (int64_t)xsafe);
            const int64_t ch = inside ? row + far_hi : min(max(row + far_hi, (int64_t)0), (int64_t)xsafe);
#ifdef KR_TUNING
            if (a.abl & 1) { zl[k].x = (double)cl; zl[k].y = 1.0; pl[k] = zl[k]; zh[k].x = (double)ch; zh[k].y = 2.0; ph[k] = zh[k]; continue; }   // abl 1 (timing only): no far operands
#endif
            zl[k] = *reinterpret_cast<const v2d*>(f.z + cl); pl[k] = *reinterpret_cast<const v2d*>(f.p_old + cl);
            zh[k] = *reinterpret_cast<const v2d*>(f.z + ch); ph[k] = *reinterpret_cast<const v2d*>(f.p_old + ch);
        }
        __syncthreads();                                                     // every wave's p_new pairs are in LDS
#pragma unroll
        for (int k = 0; k < T; ++k) {
            lo[k].x = zl[k].x + be * pl[k].x; lo[k].y = zl[k].y + be * pl[k].y;
            hi[k].x = zh[k].x + be * ph[k].x; hi[k].y = zh[k].y + be * ph[k].y;
        }
    }
    // ---- tile after tile out of LDS (spmv_pattern_stage_kernel's arithmetic)
#pragma unroll
    for (int k = 0; k < T; ++k) {
        if (k >= nt) break;                                                  // (uniform)
        const int32_t row = r0 + k * KR_TILE + 2 * t;
        const bool va = row < a.nrows, vb = row + 1 < a.nrows;
        const uint2 ma = va ? meta[ids[k] & 0xffffu] : make_uint2(0u, 0u), mb = vb ? meta[ids[k] >> 16] : make_uint2(0u, 0u);
        const int j = k * KR_TILE + 2 * t + n + 2;                           // xs[j] = p_new[row]
        const v2d A = *reinterpret_cast<const v2d*>(xs + j - 2), B = *reinterpret_cast<const v2d*>(xs + j), C = *reinterpret_cast<const v2d*>(xs + j + 2);
        const v2d M = *reinterpret_cast<const v2d*>(xs + j - n), P = *reinterpret_cast<const v2d*>(xs + j + n);
        v2d e[7];
        e[0] = lo[k]; e[1] = M; e[2].x = A.y; e[2].y = B.x; e[3] = B; e[4].x = B.y; e[4].y = C.x; e[5] = P; e[6] = hi[k];
        const double* tva = pval + (ma.x & 0xffffu); const double* tvb = pval + (mb.x & 0xffffu);
        const unsigned ka = ma.y, kb = mb.y;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            const double ta = s0 + tva[u] * e[u].x, tb = s1 + tvb[u] * e[u].y;
            s0 = ((ka >> u) & 1u) ? ta : s0;
            s1 = ((kb >> u) & 1u) ? tb : s1;
        }
#ifdef KR_TUNING
        if (a.abl & 4) { if (s0 == 1.23456789e-300) a.y[row] = s0; } else      // abl 4 (timing only): no y traffic
#endif
        { if (vb) st2(a.y, row, s0, s1);
        else if (va) a.y[row] = s0; }
        if constexpr (NQ > 0) {
            double acc[NQ];
            acc[0] = 0.0;
            if (va) acc[0] = acc[0] + B.x * s0;
            if (vb) acc[0] = acc[0] + B.y * s1;
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
        if (t < nt * NQ) {
            const int k = t / NQ, kk = t % NQ;
            double sum = red[t * (KR_T / 64)];
#pragma unroll
            for (int w2 = 1; w2 < KR_T / 64; ++w2) sum = sum + red[t * (KR_T / 64) + w2];
            a.partials[kk * a.pstride + q0 + k] = sum;
        }
    }
}

// CG's residual pass WITHOUT a stored A p (KRYST_CG_RECOMPUTE_AP; cg_pcg.hip: CgRun::iterate).  The marching fused kernel above writes A p only to
// carry it across the point where alpha is folded: 8 bytes per row written and 8 read back by CgResidualOp.  This kernel forms A p AGAIN from the
// direction vector that kernel has just stored -- the very doubles it had in its windows, the same e[0 .. 6], table values, absent-entry selects and
// un-fused multiply and add from 0.0, so the same bits -- and goes on as CgResidualOp does: r -= alpha Ap (cg.rs:210-212), the tile partial of (r, r)
// (:223) in ew_kernel's order (thread: 0 + r0 r0 + r1 r1; wave butterfly; the four waves in turn; partials[tile]).  Per row: p (own rows once, the
// window's halo 2 n / R and 2 / S far lines besides), r and the pattern id read, r written: 26 + halo instead of 24, and the fused kernel
// writes 8 bytes per row less (p_new and nothing else).
//   Mapping: fuse_march's -- the same T, S, strips per XCD and grid (fuse_march_plan), so a strip is on the same XCD in both kernels of an iteration and
//   the halo lines are a neighbouring strip's own lines in that L2.  The window holds plain p: no z / p_old staging, e[0] is the lane's own B pair of
//   the plane below carried in registers, e[6] comes out of the next plane's window, and only a segment's first and last plane load a far pair of p
//   from memory (clamped at the ends of the box: only absent entries point there).
//   LDS: THREE windows of R + 2 n doubles (march_window.h), W(s), W(s + 1) and the one being filled, and two copies of red.  A step is
//     a. request W(s + 2) of p into registers, and r's own rows and the ids of plane s + 1 (nontemporal: read once) -- in flight under b.  (Plain loads,
//        not LDS-DMA, for fuse_march's reason: r and the ids are in flight beside the window, and beside a pending DMA the compiler drains vmcnt(0)
//        before every use of an ordinary load.)
//     b. the tiles of plane s out of W(s) and W(s + 1): A p, r of plane s (requested one step ago) updated and stored, partials per wave into red[s & 1];
//     c. W(s + 2) from the registers into the third buffer;
//     barrier: W(s + 2) and red[s & 1] are complete;
//     d. the cross-wave step of the partials (threads 0 .. T - 1 out of red[s & 1]); the buffers change roles.
//   ONE barrier per step is enough: c. of step s overwrites the buffer that held W(s - 1), whose last reads (b. of step s - 1) are before the barrier of
//   step s - 1; W(s) and W(s + 1) are only read in step s; b. of step s + 1 reads W(s + 2) after the barrier of step s; red[s & 1] is read in d. of step s
//   and written again in b. of step s + 2, which its writers reach only through the barrier of step s + 1, behind d. of step s in every wave.  The
//   barrier is executed in every step by every wave (the branches around the fills depend on s and the segment's length alone).
//   Resources (gfx950, T = 4, n = 512): 165 VGPRs, no scratch (the compiler keeps a tile's LDS reads and the window in flight side by side: three waves
//   per SIMD would fit, two are resident); LDS 3 x 24 576 B of windows + 8 B per pattern and table entry + 256 B of red, padded to 81 408 B (half a CU's LDS less 512).  Measured at
//   512^3 (profiles/recompute/): the fused kernel 810 -> 632 us (35.3 -> 27.2 bytes per row), the residual pass 507 -> 620 us (24.1 -> 26.5), CG 628 ->
//   674 it/s.  With the ids kept where they repeat (KRYST_SPMV_PID_REUSE, fuse_march's step a.; profiles/pid_reuse/): 168 VGPRs, the residual pass
//   621 -> 576 us (26.5 -> 24.5 bytes per row).
//   a.group: strips per XCD; a.xcd_chunk: S; a.tpw: strips per plane; every strip and every plane is whole, so every row of a strip is a row of the box.
// KEEP: r is stored temporal (keep_in_cache: the next launch reads it again out of the Infinity Cache), as CgResidualOp<KEEP> does.
// LEG (KRYST_SPMV_LEG_VALUES; csr.h: pat_leg_ok, csr_create.hip: set_leg_values).  On an operator with one value per leg the value of entry u is the same
// double in every pattern that has leg u, so step b. needs no table: the seven values arrive BY VALUE in the kernel arguments (uniform: the compiler keeps
// them in scalar registers) and a lane keeps, per tile, the two rows' presence masks as one word, ka | kb << 8 (seven legs: a mask fits a byte), IN PLACE
// of the tile's ids.  The word is formed out of meta when a tile's ids arrive -- a segment's first plane, and the hand-over at a step's end where the
// pid_same flag is clear (with KRYST_SPMV_PID_REUSE = 0: every plane) -- and carried where the ids repeat.  Per tile step b. then issues its 6 window
// reads and nothing else: no meta[id] reads with the table reads behind them (2 + 14 LDS reads, 128 of 224 bytes per lane, two dependent LDS latencies
// in front of the arithmetic).  A present entry multiplies by the same double, an absent one is dropped by the same select, the order is the same: the
// same bits.  Measured at 512^3 (profiles/march_step/): 152 VGPRs instead of 168 at T = 4, the residual pass 576 -> 554 us at the same 24.5 bytes per row
// (5.71 -> 5.94 TB/s, the rate of the plain streams), CG 676 -> 690 it/s.  The fused kernel above keeps its table and its two barriers: with the same
// step it ran at 601 against 599 us and CG lost 10 it/s, and on three windows and one barrier per step (this kernel's schedule) at 626 against 609 us
// -- neither was kept.  (Its table reads hide behind the window reads only because meta[id] is read FIRST: read behind them, the step costs 100 us.)
struct LegVals { double v[7]; };
__device__ __forceinline__ unsigned leg_mask_word(const uint2* meta, const unsigned ids) { return (meta[ids & 0xffffu].y & 0xffu) | ((meta[ids >> 16].y & 0xffu) << 8); }
template <int T, bool KEEP, bool LEG>
__global__ __launch_bounds__(KR_T) void cg_recompute_residual_kernel(const SpmvArgs a, const double* p, double* r, const double* alpha, const int32_t n, const int32_t plane, const LegVals lv) {
    if (a.done && *a.done) return;                                           // (GateDone: alpha's logic may have ended the solve)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int XS = march_window_elems(n, T);                                 // elements of one window (even)
    double* win = reinterpret_cast<double*>(smem);
    uint2* meta = reinterpret_cast<uint2*>(win + 3 * XS);
    double* pval = reinterpret_cast<double*>(meta + a.npat);
    double* red = reinterpret_cast<double*>(smem + a.pat_red_off);           // 2 x T x (KR_T / 64)
    const int t = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int spx = a.group, S = a.xcd_chunk;
    const int strip = xcd * spx + slot % spx, k0 = (slot / spx) * S;
    const int nplanes = a.nrows / plane;
    if (strip >= a.tpw || k0 >= nplanes) return;                             // (uniform over the workgroup)
    const int ns = min(S, nplanes - k0);                                     // planes of this segment (the last one may be shorter)
    const int32_t rbeg = k0 * plane + strip * (T * KR_TILE);                 // first row of the strip in the segment's first plane
    const double al = *alpha;
    constexpr int NP = march_window_requests(512, T, KR_T);                  // requests per lane at most (n <= 512)
    const int32_t xsafe = (int32_t)a.xsafe;
    v2d wp[NP];
    // a window's requests (r0: the strip's first row in that plane; march_window.h: the lane's own pairs first, then its share of the halo).  Every lane
    // loads NP pairs: a request without a pair repeats the lane's first own pair (and is dropped by write_window) -- no branch around a load
    auto request = [&](const int32_t r0) {
        const int32_t e0 = r0 - n;                                           // element at the window's [0] (even)
        const bool inside = e0 >= 0 && e0 + XS <= xsafe;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = march_window_request(t, i, n, T, KR_T).lds, o = q < 0 ? march_window_request(t, 0, n, T, KR_T).lds : q;
            const int32_t e = inside ? e0 + o : min(max(e0 + o, 0), xsafe);  // outside p: any valid pair (those operands are absent entries)
            wp[i] = *reinterpret_cast<const v2d*>(p + e);
        }
    };
    auto write_window = [&](double* xs) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = march_window_request(t, i, n, T, KR_T).lds;
            if (q >= 0) *reinterpret_cast<v2d*>(xs + q) = wp[i];
        }
    };
    // a far operand the segment does not hold (below its first plane, above its last)
    auto far_pair = [&](const int64_t row) {
        return *reinterpret_cast<const v2d*>(p + min(max(row, (int64_t)0), (int64_t)xsafe));
    };
    unsigned ids[T], idn[T];
    d2 rr[T], rn[T];
    v2d prev[T], hi[T];
    unsigned same = ns > 1 ? pid_same_word<T>(a, rbeg + plane) : 0u, samen = 0u;     // fuse_march's: the flags of plane s + 1, one step ahead
    // ---- the segment's first two windows, r and the ids of its first plane
#pragma unroll
    for (int k = 0; k < T; ++k) {
        ids[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a.pid + (size_t)rbeg + k * KR_TILE + 2 * t)); idn[k] = 0u;
        rr[k] = ld2(r, (int64_t)rbeg + k * KR_TILE + 2 * t); rn[k] = rr[k];
    }
    double* w0 = win; double* w1 = win + XS; double* w2 = win + 2 * XS;    // W(s), W(s + 1), the one being filled
    request(rbeg);
#pragma unroll
    for (int k = 0; k < T; ++k) { prev[k] = far_pair((int64_t)rbeg + k * KR_TILE + 2 * t - plane); hi[k].x = 0.0; hi[k].y = 0.0; }
    for (int i = t; i < a.npat; i += KR_T) meta[i] = reinterpret_cast<const uint2*>(a.pmeta)[i];
    if constexpr (!LEG) for (int i = t; i < a.ntab; i += KR_T) pval[i] = a.pval[i];     // (LEG: no table value is read)
    write_window(w0);
    if (ns > 1) {
        request(rbeg + plane);
        write_window(w1);
    }
    __syncthreads();
    if constexpr (LEG) {                                                     // the ids of the segment's first plane have arrived: ids[k] is the mask word from here on
#pragma unroll
        for (int k = 0; k < T; ++k) ids[k] = leg_mask_word(meta, ids[k]);
    }
    for (int s = 0; s < ns; ++s) {
        const int32_t r0 = rbeg + s * plane;
        const bool last = s + 1 == ns, fill = s + 2 < ns;                   // (uniform)
        double* redb = red + (s & 1) * (T * (KR_T / 64));
        // a.
        if (fill) request(r0 + 2 * plane);
        samen = fill ? pid_same_word<T>(a, r0 + 2 * plane) : 0u;
        const unsigned sw = last ? ~0u : __builtin_amdgcn_readfirstlane(same);     // fuse_march's: byte k set, the ids of tile k stay in ids[k] (uniform)
        if (!last) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                if (!((sw >> (8 * k)) & 1u)) idn[k] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(a.pid + (size_t)(r0 + plane) + k * KR_TILE + 2 * t));
                rn[k] = ld2(r, (int64_t)(r0 + plane) + k * KR_TILE + 2 * t);
            }
        } else {
#pragma unroll
            for (int k = 0; k < T; ++k) hi[k] = far_pair((int64_t)r0 + k * KR_TILE + 2 * t + plane);
        }
        // b. tile after tile out of LDS (fuse_march's arithmetic, operand for operand), then CgResidualOp's
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int32_t row = r0 + k * KR_TILE + 2 * t;
            uint2 ma = make_uint2(0u, ids[k] & 0xffu), mb = make_uint2(0u, ids[k] >> 8);     // (LEG: the masks out of the tile's word, no table)
            if constexpr (!LEG) { ma = meta[ids[k] & 0xffffu]; mb = meta[ids[k] >> 16]; }
            const int j = march_window_tile_offset(n, k) + 2 * t;            // w0[j] = p[row], w1[j] = p[row + plane]
            const v2d A = *reinterpret_cast<const v2d*>(w0 + j - 2), B = *reinterpret_cast<const v2d*>(w0 + j), C = *reinterpret_cast<const v2d*>(w0 + j + 2);
            const v2d M = *reinterpret_cast<const v2d*>(w0 + j - n), P = *reinterpret_cast<const v2d*>(w0 + j + n);
            const v2d U = *reinterpret_cast<const v2d*>(w1 + j);             // (the segment's last plane: not used)
            v2d e[7];
            e[0] = prev[k]; e[1] = M; e[2].x = A.y; e[2].y = B.x; e[3] = B; e[4].x = B.y; e[4].y = C.x; e[5] = P;
            e[6].x = last ? hi[k].x : U.x; e[6].y = last ? hi[k].y : U.y;
            prev[k] = B;
            const double* tva = pval + (ma.x & 0xffffu); const double* tvb = pval + (mb.x & 0xffffu);
            const unsigned ka = ma.y, kb = mb.y;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int u = 0; u < 7; ++u) {
                const double va = LEG ? lv.v[u] : tva[u], vb = LEG ? lv.v[u] : tvb[u];
                const double ta = s0 + va * e[u].x, tb = s1 + vb * e[u].y;
                s0 = ((ka >> u) & 1u) ? ta : s0;
                s1 = ((kb >> u) & 1u) ? tb : s1;
            }
            const double q0 = rr[k].a - al * s0, q1 = rr[k].b - al * s1;    // cg.rs:210-212
            st2_sel<KEEP>(r, row, q0, q1);
            double acc = 0.0;
            acc = acc + q0 * q0;
            acc = acc + q1 * q1;
            const double wsum = wave_butterfly(acc);
            if ((t & 63) == 0) redb[k * (KR_T / 64) + (t >> 6)] = wsum;
        }
        // c.
        if (fill) write_window(w2);
        __syncthreads();
        // d.
        if (t < T) {                                                         // thread k: tile r0 / 512 + k
            double sum = redb[t * (KR_T / 64)];
#pragma unroll
            for (int w = 1; w < KR_T / 64; ++w) sum = sum + redb[t * (KR_T / 64) + w];
            a.partials[r0 / KR_TILE + t] = sum;
        }
#pragma unroll
        for (int k = 0; k < T; ++k) { if (!((sw >> (8 * k)) & 1u)) ids[k] = LEG ? leg_mask_word(meta, idn[k]) : idn[k]; rr[k] = rn[k]; }     // (LEG: the new ids become the mask word)
        same = samen;
        double* w = w0; w0 = w1; w1 = w2; w2 = w;
    }
}

// the fused form: a single-rank stencil operator that streams its CSR-P16 form, all bases (far, -n, -1, 0, +1, +n, far) with the same far offsets
static bool fuse_form(kryst_csr_t a) { return staged_form_uniform_far(a) && streams_p16(a, false); }
// the size rule behind the defaults of KRYST_CG_FUSE_P, KRYST_SPMV_FUSE_MARCH and KRYST_CG_RECOMPUTE_AP: vectors beyond KRYST_CG_FUSE_MIN_BYTES (512^3)
static bool beyond_fuse_min_bytes(kryst_csr_t a) { return a->nrows * 8 > env_ll("KRYST_CG_FUSE_MIN_BYTES", 768ll << 20); }
// Can the operator take the fused form (spmv_pattern_fuse_kernel)?
bool spmv_can_fuse_direction(kryst_csr_t a) {
    return fuse_form(a) && staged_settings_ok(a) && env_int("KRYST_SPMV_STAGE_UFAR", 1) != 0 &&
           // measured (profiles/r05/cg_fuse_ab.jsonl, cg_fuse_sweep.jsonl, cg_xbatch_ab.jsonl): fewer bytes only pay where the vectors are far beyond
           // the 256 MiB Infinity Cache -- with x in batches 512^3 CG +11 % (PCG +10 %), 480^3 +6 %, 448^3 +-1 %, 416^3 -1 %, 384^3 -6 %, 256^3 0 .. -5 %.
           // KRYST_CG_FUSE_P = 1 / 0 forces the fused / unfused form.
           env_int("KRYST_CG_FUSE_P", beyond_fuse_min_bytes(a) ? 1 : 0) != 0;
}
// The marching mode of the fused kernel (spmv_pattern_fuse_kernel<.., MARCH>): a workgroup keeps a strip of 512 T rows of a plane and walks a
// segment of S planes.  Eligible: uniform far offsets of exactly +- one plane, a plane that is a whole number of strips, a box that is a whole
// number of planes, lines of at most 512 points, and two windows + tables that leave room for two workgroups per CU; everything else (40^3:
// a plane of 1 600 rows; 16^3: a tile spans two planes) takes the un-marched path untouched.  KRYST_SPMV_FUSE_MARCH (0 / 1), KRYST_SPMV_FUSE_SEG
// (S) and KRYST_SPMV_FUSE_T are read per launch.
struct FuseMarchPlan { bool eligible, on; int T, strips, S, segs; StagedLds lds; };
// (strips of 8 tiles walked by workgroups of 512 threads, one per CU -- 1.25 instead of 1.5 window requests per own row -- were built and measured:
// CG 714 against 768 it/s at 512^3, 0.70 at 384^3, 0.93 at 256^3 of the rate at T = 4; not in the tree, profiles/march_t8/)
static FuseMarchPlan fuse_march_plan(kryst_csr_t a, int nq) {
    FuseMarchPlan m;
    memset(&m, 0, sizeof m);
    m.T = env_int("KRYST_SPMV_FUSE_T", 4) <= 2 ? 2 : 4;
    const int64_t plane = a->pat_far_uniform ? (int64_t)a->pat_far_hi : 0, R = (int64_t)m.T * KR_TILE;
    const int32_t n_ = a->pat_stage_n;
    if (!(a->d_pid && n_ > 0 && n_ <= 512 && plane > 0 && (int64_t)a->pat_far_lo == -plane && plane % R == 0 && a->nrows % plane == 0 && a->nrows == a->xlen)) return m;
    m.lds = staged_lds(a, 2, 8, 1, m.T, nq, 0);
    if (m.lds.bytes > ((size_t)80 << 10)) return m;
    const int64_t nplanes = a->nrows / plane;
    m.eligible = true;
    m.strips = (int)(plane / R);
    // S: KRYST_SPMV_FUSE_SEG, or (0, the default) the longest segments that still give two full rounds of the resident workgroups (two per CU, below):
    // strips x segments <= 4 per CU -- 512^3: 128 strips x 8 segments of 64 planes = 1 024 workgroups; 384^3: 72 x 14 of 28; 256^3: 32 x 32 of 8.
    // Fewer, longer segments leave CUs idle (256^3 with S = 64: 128 workgroups, 0.69 of the un-marched rate), shorter ones read more far operands.
    int S = env_int("KRYST_SPMV_FUSE_SEG", 0);
    if (S <= 0) {
        const int64_t want = std::max<int64_t>(1, (int64_t)a->ctx->num_cu * 4 / m.strips);
        S = (int)std::max<int64_t>((nplanes + want - 1) / want, std::min<int64_t>(4, nplanes));
    }
    m.S = (int)std::min<int64_t>(S, nplanes);
    m.segs = (int)((nplanes + m.S - 1) / m.S);
    // On by default where it was measured to pay and the fused form is the default itself (vectors beyond KRYST_CG_FUSE_MIN_BYTES: 512^3).  In-process
    // A/B inside CG with the fused form forced (tools/cg_march_ab.py, profiles/march/): 512^3 +3.3 .. +3.5 %, 256^3 +4.6 %, 448^3 -0.2 %, 384^3 -2.6 .. -3.4 %.
    m.on = env_int("KRYST_SPMV_FUSE_MARCH", beyond_fuse_min_bytes(a) ? 1 : 0) != 0;
    return m;
}
// CG without a stored A p (cg_recompute_residual_kernel): the marching fused kernel stores p_new only and the residual pass forms A p again.  Taken
// where the marching plan is eligible and on, three windows + tables + two copies of red leave room for two workgroups per CU, CG updates x in
// batches (KRYST_CG_X_BATCH > 1: the fused kernel's instance without the x update) and KRYST_CG_RECOMPUTE_AP (0 / 1, read per iteration) allows it.
// The knob's default follows KRYST_SPMV_FUSE_MARCH's size rule (vectors beyond KRYST_CG_FUSE_MIN_BYTES: 512^3).  Measured (profiles/recompute/): the
// benchmark's command alternating with the parent commit 637 / 624 / 624 -> 677 / 672 / 672 it/s (+7.2 %); in-process A/B with the fused form forced
// (tools/cg_recompute_ab.py): 512^3 +6.2 %, 384^3 +4.0 %, 256^3 +2.0 %, 448^3 -6.0 %.
struct RecomputePlan { bool on; FuseMarchPlan m; StagedLds lds; };
static RecomputePlan recompute_plan(kryst_csr_t a) {
    RecomputePlan q;
    memset(&q, 0, sizeof q);
    q.m = fuse_march_plan(a, 2);
    if (!(q.m.eligible && q.m.on)) return q;
    q.lds = staged_lds(a, 3, 8, 2, q.m.T, 1, 0);
    if (q.lds.bytes > ((size_t)(160 << 10) / 2 - 512)) return q;
    // (32: CG's default batch length in the fused form, cg_pcg.hip: cg_x_batch; the solver also checks the length it really took)
    q.on = env_int("KRYST_CG_X_BATCH", 32) > 1 && env_int("KRYST_CG_RECOMPUTE_AP", beyond_fuse_min_bytes(a) ? 1 : 0) != 0;
    return q;
}
bool spmv_can_recompute_ap(kryst_csr_t a) { return spmv_can_fuse_direction(a) && recompute_plan(a).on; }
// The marching kernels keep a tile's pattern ids in registers from plane to plane where the operator's pid_same table says they repeat (csr.h:
// d_pid_same; on a box with constant coefficients every plane but the first two and the last).  KRYST_SPMV_PID_REUSE (0 / 1, read per launch): 0
// hands the kernels no table, and every plane loads its ids again.
static const uint8_t* pid_same_table(kryst_csr_t a) { return env_int("KRYST_SPMV_PID_REUSE", 1) != 0 ? a->d_pid_same : nullptr; }
// The recompute residual pass takes the seven leg values as kernel arguments where the operator has one value per leg (csr.h: pat_leg_ok) and
// KRYST_SPMV_LEG_VALUES (0 / 1, read per launch) allows it; every other operator keeps the table look-ups.  In-process A/B inside CG with the fused form
// forced (tools/cg_step_ab.py, profiles/march_step/): it costs nothing at 384^3 and 256^3 either, so the knob has no size rule.
static bool leg_values_on(kryst_csr_t a) { return a->pat_leg_ok && env_int("KRYST_SPMV_LEG_VALUES", 1) != 0; }
// r -= alpha A p with the tile partials of (r, r), A p formed from p on the way (the launch after launch_spmv_fused(.., y = nullptr, ..) and alpha's fold)
int32_t launch_cg_residual_recompute(kryst_csr_t a, const double* p, double* r, const double* alpha, bool keep, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    const RecomputePlan q = recompute_plan(a);
    KR_ARG(q.on, "launch_cg_residual_recompute: the operator's marching plan cannot take it");
    KR_TRY(ensure_partials(ctx, a->ntiles));
    SpmvArgs args;
    spmv_args_fill(args, a, p, nullptr, nullptr, done);
    args.xsafe = xsafe_of(a);
    const int spx = (q.m.strips + 7) / 8;
    args.group = spx; args.xcd_chunk = q.m.S; args.tpw = q.m.strips; args.pat_red_off = (int32_t)q.lds.red_off;
    args.pid_same = pid_same_table(a);
    // two resident workgroups per CU, like the fused kernel: the dynamic LDS request is padded so that no third one fits (T = 2)
    const size_t lds = std::max(q.lds.bytes, (size_t)(160 << 10) / 2 - 512);
    static bool raised = false;
    if (!raised) {
#define KR_RESID_FNS(T_, K_) (const void*)cg_recompute_residual_kernel<T_, K_, false>, (const void*)cg_recompute_residual_kernel<T_, K_, true>
        for (const void* fn : {KR_RESID_FNS(2, false), KR_RESID_FNS(2, true), KR_RESID_FNS(4, false), KR_RESID_FNS(4, true)})
            (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 80 << 10);
#undef KR_RESID_FNS
        raised = true;
    }
    const dim3 grid((unsigned)(8 * spx * q.m.segs)), block(KR_T);
    const int32_t n_ = a->pat_stage_n, plane = a->pat_far_hi;
    LegVals lv;
    for (int u = 0; u < 7; ++u) lv.v[u] = a->pat_leg[u];
    by_int<2, 4>(q.m.T, [&](auto T_) { by_bool(keep, [&](auto KEEP) { by_bool(leg_values_on(a), [&](auto LEG) {
        hipLaunchKernelGGL((cg_recompute_residual_kernel<T_(), KEEP(), LEG()>), grid, block, lds, ctx->s_main, args, p, r, alpha, n_, plane, lv); }); }); });
    KR_HIP(hipGetLastError());
    phase_mark(ctx, KR_PH_BLAS1_RESIDUAL);
    return KRYST_OK;
}
// y = A p_new with p_new = z + beta p_old formed on the way (stored to p_new), the owed x += alpha p_old on the same pass, partial (p_new, y)
// [and (y, y)] -- see spmv_pattern_fuse_kernel.  `done`, alpha, beta, xpend: device scalars of the solve; it: the iteration being enqueued.
// force: the measurement hook's launch, whatever the settings say about the fused form
static int32_t launch_spmv_fused_impl(kryst_csr_t a, const double* z, const double* p_old, double* p_new, double* xvec, double* y, int nq,
                                      const double* alpha, const double* beta, const long long* xpend, long long it, const int* done, bool force) {
    kryst_ctx_t ctx = a->ctx;
    KR_ARG((force || spmv_can_fuse_direction(a)) && nq >= 1 && nq <= 2, "launch_spmv_fused: operator cannot take the fused form");
    KR_TRY(ensure_partials(ctx, a->ntiles));
    SpmvArgs args;
    spmv_args_fill(args, a, p_new, y, p_new, done);
    const int T = env_int("KRYST_SPMV_FUSE_T", 4) <= 2 ? 2 : 4;     // runs of 4 tiles: the window's halo (2 n + 4 elements) is read for 2 048 rows instead of 1 024
    const int32_t n_ = a->pat_stage_n;
    const StagedLds l = staged_lds(a, 1, 8, 1, T, nq);
    args.pat_red_off = (int32_t)l.red_off;
    size_t lds_s = l.bytes;
    // resident workgroups per CU: like the BLAS-1 streams (ew.h: 2-3 workgroups per CU keep DRAM pages open, 8 lose a sixth of the bandwidth) this
    // kernel is a mix of read and write streams; the dynamic LDS request is padded so that only `wgcu` workgroups fit a CU's 160 KiB
    const int wgcu = env_int("KRYST_SPMV_FUSE_WG_PER_CU", 0);
    if (wgcu > 0) lds_s = std::max(lds_s, std::min<size_t>((size_t)(160 << 10) / (size_t)wgcu - 512, (size_t)64 << 10));
    args.xsafe = xsafe_of(a);
    const int64_t nruns = (a->ntiles + T - 1) / T;
    args.group = std::max(1, env_int("KRYST_SPMV_STAGE_GROUP", stage_group_default(a, nruns, T, true)));
    const int64_t per_xcd = ((nruns + 7) / 8 + args.group - 1) / args.group * args.group;
    const dim3 sgrid((unsigned)(per_xcd * 8)), block(KR_T);
    const FuseArgs f{z, p_old, p_new, xvec, alpha, beta, xpend, it};
#ifdef KR_TUNING
    args.abl = env_int("KRYST_FUSE_ABL", 0);          // timing-only ablations (tuning builds; wrong results)
#endif
    const FuseMarchPlan m = fuse_march_plan(a, 2);    // (sized for two quantities, like the query: one answer per operator)
#ifdef KR_TUNING
    if (m.eligible && m.on && !args.abl) {
#else
    if (m.eligible && m.on) {
#endif
        const int spx = (m.strips + 7) / 8;
        args.group = spx; args.xcd_chunk = m.S; args.tpw = m.strips; args.pat_red_off = (int32_t)m.lds.red_off;
        args.pid_same = pid_same_table(a);
        size_t lds_m = m.lds.bytes;
        // resident workgroups per CU: two unless KRYST_SPMV_FUSE_WG_PER_CU says otherwise (the three that fit at T = 4 are slower: 512^3 CG 620-624 against
        // 636 it/s, profiles/march/sweep512.jsonl)
        const int wgm = wgcu > 0 ? wgcu : 2;
        lds_m = std::max(lds_m, std::min<size_t>((size_t)(160 << 10) / (size_t)wgm - 512, (size_t)80 << 10));
        static bool raised_m = false;
        if (!raised_m) {
#define KR_MARCH_FNS(NQ_, T_) (const void*)spmv_pattern_fuse_kernel<NQ_, T_, 512, true, true>, (const void*)spmv_pattern_fuse_kernel<NQ_, T_, 512, false, true>
            for (const void* fn : {KR_MARCH_FNS(1, 2), KR_MARCH_FNS(1, 4), KR_MARCH_FNS(2, 2), KR_MARCH_FNS(2, 4),
                                   (const void*)spmv_pattern_fuse_kernel<1, 2, 512, false, true, false>, (const void*)spmv_pattern_fuse_kernel<1, 4, 512, false, true, false>})
                (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 80 << 10);
#undef KR_MARCH_FNS
            raised_m = true;
        }
        const dim3 mgrid((unsigned)(8 * spx * m.segs));
        auto march = [&](auto NQ, auto T_, auto XU, auto YS) {
            hipLaunchKernelGGL((spmv_pattern_fuse_kernel<NQ(), T_(), 512, XU(), true, YS()>), mgrid, block, lds_m, ctx->s_main, args, f, n_, a->pat_far_lo, a->pat_far_hi); };
        if (!y) {                                      // no y store: the residual pass forms A p again (launch_cg_residual_recompute)
            KR_ARG(nq == 1 && !xvec, "launch_spmv_fused: the form without y is CG's with x in batches");
            by_int<2, 4>(m.T, [&](auto T_) { march(std::integral_constant<int, 1>{}, T_, std::false_type{}, std::false_type{}); });
        } else {
            by_int<1, 2>(nq, [&](auto NQ) { by_int<2, 4>(m.T, [&](auto T_) { by_bool(xvec != nullptr, [&](auto XU) { march(NQ, T_, XU, std::true_type{}); }); }); });
        }
        KR_HIP(hipGetLastError());
        phase_mark(ctx, KR_PH_SPMV);
        return KRYST_OK;
    }
    KR_ARG(y, "launch_spmv_fused: only the marching kernel has a form without y");
    if (lds_s > ((size_t)48 << 10)) {       // (more than the default dynamic LDS limit: once per instance)
        static bool raised = false;
        if (!raised) {
#define KR_FUSE_FNS(NQ_, T_, X_) (const void*)spmv_pattern_fuse_kernel<NQ_, T_, 512, X_>, (const void*)spmv_pattern_fuse_kernel<NQ_, T_, 1024, X_>
            for (const void* fn : {KR_FUSE_FNS(1, 2, true), KR_FUSE_FNS(1, 4, true), KR_FUSE_FNS(2, 2, true), KR_FUSE_FNS(2, 4, true),
                                   KR_FUSE_FNS(1, 2, false), KR_FUSE_FNS(1, 4, false), KR_FUSE_FNS(2, 2, false), KR_FUSE_FNS(2, 4, false)})
                (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10);
#undef KR_FUSE_FNS
            raised = true;
        }
    }
    by_int<1, 2>(nq, [&](auto NQ) { by_int<2, 4>(T, [&](auto T_) { by_bool(xvec != nullptr, [&](auto XU) {
        if (n_ <= 512) hipLaunchKernelGGL((spmv_pattern_fuse_kernel<NQ(), T_(), 512, XU()>), sgrid, block, lds_s, ctx->s_main, args, f, n_, a->pat_far_lo, a->pat_far_hi);
        else hipLaunchKernelGGL((spmv_pattern_fuse_kernel<NQ(), T_(), 1024, XU()>), sgrid, block, lds_s, ctx->s_main, args, f, n_, a->pat_far_lo, a->pat_far_hi);
    }); }); });
    KR_HIP(hipGetLastError());
    phase_mark(ctx, KR_PH_SPMV);
    return KRYST_OK;
}
int32_t launch_spmv_fused(kryst_csr_t a, const double* z, const double* p_old, double* p_new, double* xvec, double* y, int nq,
                          const double* alpha, const double* beta, const long long* xpend, long long it, const int* done) {
    return launch_spmv_fused_impl(a, z, p_old, p_new, xvec, y, nq, alpha, beta, xpend, it, done, false);
}

}  // namespace kr

using namespace kr;
extern "C" {
// info[0 .. 5]: fuse_march_plan's eligible, eligible and on, T, strips per plane, S, segments; info[6]: recompute_plan's on
int32_t kryst_csr_fuse_march_info(kryst_csr_t a, int64_t* info) {
    KR_ARG(a && info, "csr_fuse_march_info");
    const bool form = fuse_form(a);
    FuseMarchPlan m;
    memset(&m, 0, sizeof m);
    if (form) m = fuse_march_plan(a, 2);
    info[0] = m.eligible ? 1 : 0; info[1] = m.eligible && m.on ? 1 : 0; info[2] = m.T; info[3] = m.strips; info[4] = m.S; info[5] = m.segs;
    info[6] = form && recompute_plan(a).on ? 1 : 0;
    return KRYST_OK;
}
// info[0]: a marching launch would now be handed the operator's pid_same table (the marching mode on, KRYST_SPMV_PID_REUSE, a table); info[1]: tiles
// flagged "the ids of the tile one plane below"; info[2]: tiles the table covers (info[1 .. 2] 0 without a table)
int32_t kryst_csr_pid_reuse_info(kryst_csr_t a, int64_t* info) {
    KR_ARG(a && info, "csr_pid_reuse_info");
    FuseMarchPlan m;
    memset(&m, 0, sizeof m);
    if (fuse_form(a)) m = fuse_march_plan(a, 2);
    info[0] = m.eligible && m.on && pid_same_table(a) ? 1 : 0;
    info[1] = a->d_pid_same ? a->pid_same_count : 0;
    info[2] = a->d_pid_same ? a->nrows / KR_TILE : 0;
    return KRYST_OK;
}
// info[0]: the operator has one value per leg (csr.h: pat_leg_ok); info[1]: a recompute residual pass would now take the values as kernel arguments (the
// marching mode and the recompute-Ap form on, KRYST_SPMV_LEG_VALUES); values[0 .. 6]: the leg values (+0.0 throughout when info[0] is 0)
int32_t kryst_csr_leg_values_info(kryst_csr_t a, int64_t* info, double* values) {
    KR_ARG(a && info && values, "csr_leg_values_info");
    info[0] = a->pat_leg_ok ? 1 : 0;
    info[1] = fuse_form(a) && recompute_plan(a).on && leg_values_on(a) ? 1 : 0;
    for (int u = 0; u < 7; ++u) values[u] = a->pat_leg[u];
    return KRYST_OK;
}
// Measurement hook: average milliseconds per launch of the fused direction + SpMV kernel of CG / PCG (spmv_pattern_fuse_kernel) on work vectors of its
// own: z = x, p_old = a copy of x, alpha = 1e-3, beta = 0.5, the x update owed at every launch; p_old / p_new alternate like in the solver.
// KRYST_UNSUPPORTED when the operator cannot take the fused form.
int32_t kryst_bench_spmv_fused(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y, int32_t reps, double* avg_ms) {
    KR_ARG(a && x && y && avg_ms && reps >= 1, "bench_spmv_fused");
    KR_ARG(x->n == a->xlen && y->n == a->nrows && x->ctx == a->ctx && y->ctx == a->ctx, "bench_spmv_fused: size / context mismatch");
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    if (!fuse_form(a)) {
        set_error("bench_spmv_fused: the operator has no staged CSR-P16 form with uniform far offsets");
        return KRYST_UNSUPPORTED;
    }
    const size_t bytes = sizeof(double) * (size_t)((x->n + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE);
    double *p[2] = {nullptr, nullptr}, *xv = nullptr, *sc = nullptr;
    int32_t rc = KRYST_OK;
    if (hipMalloc(&p[0], bytes) != hipSuccess || hipMalloc(&p[1], bytes) != hipSuccess || hipMalloc(&xv, bytes) != hipSuccess || hipMalloc(&sc, 64) != hipSuccess) rc = KRYST_ERR_HIP;
    const double host_sc[4] = {1e-3, 0.5, 0.0, 0.0};                 // alpha, beta, xpend (as a long long 0), pad
    if (rc == KRYST_OK && (hipMemcpyAsync(p[0], x->d, bytes, hipMemcpyDeviceToDevice, ctx->s_main) != hipSuccess || hipMemsetAsync(p[1], 0, bytes, ctx->s_main) != hipSuccess ||
                           hipMemsetAsync(xv, 0, bytes, ctx->s_main) != hipSuccess || hipMemcpyAsync(sc, host_sc, sizeof host_sc, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    const long long* xpend = reinterpret_cast<const long long*>(sc + 2);
    auto once = [&](int r) { return launch_spmv_fused_impl(a, x->d, p[r & 1], p[(r + 1) & 1], xv, y->d, 1, sc, sc + 1, xpend, 1ll, nullptr, true); };
    if (rc == KRYST_OK) rc = once(0);
    if (rc == KRYST_OK) {
        (void)hipEventRecord(ctx->tm0, ctx->s_main);
        for (int r = 1; r <= reps && rc == KRYST_OK; ++r) rc = once(r);
        (void)hipEventRecord(ctx->tm1, ctx->s_main);
        (void)hipEventSynchronize(ctx->tm1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->tm0, ctx->tm1);
        *avg_ms = (double)ms / reps;
    }
    (void)hipStreamSynchronize(ctx->s_main);
    (void)hipFree(p[0]); (void)hipFree(p[1]); (void)hipFree(xv); (void)hipFree(sc);
    if (rc == KRYST_ERR_HIP) set_error("bench_spmv_fused: allocation or copy failed");
    return rc;
}

}  // extern "C"
