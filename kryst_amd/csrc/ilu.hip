// ILU(0)-family preconditioners with a level-scheduled triangular solve on the device.
//
//   mode KRYST_ILU_KRYST_COMPAT  Ilu0 exactly as written (src/preconditioner/ilu.rs:59-122): the net effect of its setup is
//                                L = I + tril(A,-1) D^-1 (l_ij = a_ij / a_jj), U = triu(A); apply never divides by u_ii.
//   mode KRYST_ILU_ILUP0         Ilup::new(0) exactly as written (src/preconditioner/ilup.rs:77-167): no elimination happens
//                                at fill 0 (new_level = 1 > fill), same L, U = triu(A), apply divides by the stored diagonal.
//   mode KRYST_ILU_TRUE_ILU0     extension: textbook IKJ ILU(0) on A's pattern (Saad Alg. 10.4).
//
// Setup (host, once): factor values, dependency levels of L (ascending rows) and U (descending rows), and a LEVEL-ORDERED
// copy of each factor (rows of one level contiguous, columns renumbered to level-order positions).
// Apply (device): the vectors are permuted into level order, the two triangular systems are solved -- a lane owns a row and
// subtracts its entries in stored order, exactly the reference's loop -- and the result is permuted back; the launch sequence
// is captured once into a hipGraph.  A 7-point 256^3 grid has 3N-2 = 766 dependency levels per factor, so the solve is
// LATENCY-bound.  Two forms with identical results: one kernel per level (3.4 us per level: kernel boundary + ~3 dependent
// memory round trips; KRYST_ILU_SYNCFREE=0) and, by default, ONE sync-free launch per factor in which every lane polls the
// solution entries it needs (2.05 us per dependency hop, 3.1 instead of 5.2 ms per apply; see tri_syncfree_ell_kernel).
// A band schedule (B levels per launch, each workgroup recomputing the in-band dependency closure of its rows so that
// workgroup barriers replace kernel boundaries) was built and measured: bit-identical but no faster, removed again.
// In a distributed context the factors are block-local (block-Jacobi ILU): halo columns are dropped.
#include "ilu.h"

namespace kr {

// forward:  y[i] = r[i] - sum l_ij y[j]            (ilu.rs:107-113, ilup.rs:143-149)
// backward: z[i] = (y[i] - sum u_ij z[j]) / d_i     (ilu.rs:115-119 with d = 1, ilup.rs:151-165)
// All level kernels work on LEVEL-PERMUTED vectors (`in`, `out` indexed by the level-order position p; the factor's column
// indices are positions too): the rows of a level and, for banded operators, their dependencies in the previous level are
// contiguous in memory, so a level touches a few pages instead of one page per row (the scattered form spent ~5 us per
// level on address translation and uncoalesced 8-byte accesses).  perm_gather / perm_scatter convert at the ends.

// rows of ONE level: positions [p0, p1)
template <bool FORWARD>
__global__ __launch_bounds__(256) void tri_level_kernel(const TriArgs* args, const double* __restrict__ in, double* out,
                                                        const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ val, const double* __restrict__ diag,
                                                        int32_t p0, int32_t p1) {
    if (args->skip) return;
    const int32_t p = p0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= p1) return;
    double s = in[p];
    for (int32_t k = ptr[p]; k < ptr[p + 1]; ++k) s = s - val[k] * out[col[k]];    // stored order
    out[p] = FORWARD ? s : s / diag[p];                                             // diag == 1.0: exact no-op
}

__device__ __forceinline__ double ell_row(const EllView& E, int32_t p, double s, const double* z) {
    int32_t c[ELLW]; double v[ELLW], zz[ELLW];
    const int len = E.len[p];
#pragma unroll
    for (int u = 0; u < ELLW; ++u) { c[u] = E.col[u * E.npos + p]; v[u] = E.val[u * E.npos + p]; }
#pragma unroll
    for (int u = 0; u < ELLW; ++u) zz[u] = z[c[u]];                 // padding slots point at column 0 (valid, unused)
#pragma unroll
    for (int u = 0; u < ELLW; ++u) if (u < len) s = s - v[u] * zz[u];   // stored order
    return s;
}

template <bool FORWARD>
__global__ __launch_bounds__(256) void tri_level_ell_kernel(const TriArgs* args, const double* __restrict__ in, double* out, EllView E,
                                                            const double* __restrict__ diag, int32_t p0, int32_t p1) {
    if (args->skip) return;
    const int32_t p = p0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= p1) return;
    const double s = ell_row(E, p, in[p], out);
    out[p] = FORWARD ? s : s / diag[p];
}

// SYNC-FREE form (ELL factors): ONE launch per factor instead of one per level.  Lane = level-order position; a lane polls
// the solution entries its row depends on until they have been written (the solution vector is pre-filled with a NaN
// sentinel, so the value is its own ready flag: one 8-byte agent-scope load per dependency and poll), then subtracts them in
// the stored order -- the same arithmetic as the level kernels -- and publishes its own entry with an agent-scope store.
// Forward progress: dependencies live at SMALLER positions (earlier levels), workgroups are dispatched in index order per
// XCD, so the lowest unfinished workgroup is always resident and depends only on finished ones.  Lanes of one wave may
// depend on each other (a wave can span several small levels), so nobody blocks: every round each unfinished lane polls
// once, ready lanes finish, and the wave leaves when all its lanes have.  A poll budget turns a logic error into NaNs
// instead of a hung GPU.
template <bool FORWARD>
__global__ __launch_bounds__(256) void tri_syncfree_ell_kernel(const TriArgs* args, const double* __restrict__ in, double* out, EllView E,
                                                               const double* __restrict__ diag, int32_t npos) {
    if (args->skip) return;
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < npos;
    int len = 0; int32_t c[ELLW]; double v[ELLW], zz[ELLW]; double s = 0.0, dg = 1.0;
#pragma unroll
    for (int u = 0; u < ELLW; ++u) { c[u] = 0; v[u] = 0.0; zz[u] = 0.0; }
    if (active) {
        len = E.len[p];
#pragma unroll
        for (int u = 0; u < ELLW; ++u) { c[u] = E.col[u * E.npos + p]; v[u] = E.val[u * E.npos + p]; }
        s = in[p];
        if (!FORWARD) dg = diag[p];
    }
    const unsigned want = (1u << len) - 1u;
    unsigned have = 0;
    bool done = !active;
    // (all (<= 4) dependencies are polled every round: gating them on the deepest one, which pays for rows of 13 entries in
    // tri_syncfree_csr_kernel, adds a dependent round trip here -- 256^3: 3.1 -> 4.2 ms)
    for (int budget = 1 << 22; budget > 0; --budget) {
        if (!done) {
#pragma unroll
            for (int u = 0; u < ELLW; ++u)
                if (u < len && !((have >> u) & 1u)) {
                    const double x = __hip_atomic_load(&out[c[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned long long)__double_as_longlong(x) != KR_TRI_SENTINEL) { zz[u] = x; have |= 1u << u; }
                }
            if (have == want) {
#pragma unroll
                for (int u = 0; u < ELLW; ++u) if (u < len) s = s - v[u] * zz[u];       // stored order
                __hip_atomic_store(&out[p], FORWARD ? s : s / dg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                done = true;
            }
        }
        if (__all(done)) return;
        __builtin_amdgcn_s_sleep(1);                        // the poll period does not matter (0..4 measured alike): the hop is two fabric trips
    }
    if (!done) __hip_atomic_store(&out[p], __longlong_as_double(0x7FF8000000000000ll), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // budget exhausted
}

// the same for factors with longer rows (CSR in level order): a lane advances through its entries as far as they are ready.
// The row's first P entries (columns AND values) are in registers before the lane starts waiting: once its gate opens, what stands
// between the row and its result is ONE uncached round trip for all of them -- with the entries fetched after the gate (round 2:
// batches of eight, columns from L2, values a cold miss each) a 27-point factor's 13 entries per row cost 7.4 us per dependency level.
template <bool FORWARD, int P>
__global__ __launch_bounds__(256) void tri_syncfree_csr_kernel(const TriArgs* args, const double* __restrict__ in, double* out,
                                                               const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ val, const double* __restrict__ diag, int32_t npos) {
    if (args->skip) return;
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < npos;
    int32_t k = 0, kend = 0; double s = 0.0, dg = 1.0;
    if (active) { k = ptr[p]; kend = ptr[p + 1]; s = in[p]; if (!FORWARD) dg = diag[p]; }
    bool done = !active;
    int32_t cc[P]; double vv[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
        const int32_t kk = min(k + u, kend - 1);
        cc[u] = k < kend ? col[kk] : 0;
        vv[u] = k < kend ? val[kk] : 0.0;
    }
    // While a row waits it polls ONE entry: the dependency at the largest level-order position, i.e. of the deepest level -- the
    // last one to be solved in all but rare cases (eight uncached loads per waiting lane and round slowed everybody down: 20 -> 40 ms
    // on a 27-point factor).  Once that one is there, the batch below usually finds everything ready.
    int32_t gate_col = -1;
#pragma unroll
    for (int u = 0; u < P; ++u) if (k + u < kend) gate_col = max(gate_col, cc[u]);
    for (int32_t kk = k + P; kk < kend; ++kk) gate_col = max(gate_col, col[kk]);
    bool open = gate_col < 0;
    bool first = true;
    for (int budget = 1 << 22; budget > 0; --budget) {
        if (!done && !open) {
            const double g = __hip_atomic_load(&out[gate_col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            open = (unsigned long long)__double_as_longlong(g) != KR_TRI_SENTINEL;
        }
        if (!done && open) {
            if (first) {
                // the register-held entries: asked for TOGETHER, the ready prefix consumed in stored order
                first = false;
                double xv[P];
#pragma unroll
                for (int u = 0; u < P; ++u) xv[u] = k + u < kend ? __hip_atomic_load(&out[cc[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
                bool prefix = true;
                int adv = 0;
#pragma unroll
                for (int u = 0; u < P; ++u) {
                    const bool ready = (unsigned long long)__double_as_longlong(xv[u]) != KR_TRI_SENTINEL;
                    prefix = prefix && k + u < kend && ready;
                    if (prefix) { s = s - vv[u] * xv[u]; ++adv; }                          // stored order
                }
                k += adv;
            } else {
                // what is left (a gate that opened before an earlier dependency, rows longer than P): batches of eight from memory
                constexpr int B = 8;
                double xv[B], wv[B];
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const int32_t kk = min(k + u, kend - 1);
                    wv[u] = k < kend ? val[kk] : 0.0;
                    xv[u] = k < kend ? __hip_atomic_load(&out[col[kk]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
                }
                bool prefix = true;
                int adv = 0;
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const bool ready = (unsigned long long)__double_as_longlong(xv[u]) != KR_TRI_SENTINEL;
                    prefix = prefix && k + u < kend && ready;
                    if (prefix) { s = s - wv[u] * xv[u]; ++adv; }                          // stored order
                }
                k += adv;
            }
            if (k == kend) {
                __hip_atomic_store(&out[p], FORWARD ? s : s / dg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                done = true;
            }
        }
        if (__all(done)) return;
        __builtin_amdgcn_s_sleep(1);
    }
    if (!done) __hip_atomic_store(&out[p], __longlong_as_double(0x7FF8000000000000ll), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // budget exhausted
}

// PIPELINED WAVEFRONT solve of a structured-grid factor (GridFactor).  One wave per workgroup owns an 8 x 8 block of grid
// lines (j,k); lane (jl,kl) walks its line i = 0..Ni-1 (backward: everything mirrored), one row per step, skewed by jl + kl
// steps, so that when it reaches row i its j- and k-neighbours' row i was finished one step earlier by the lanes next to it:
// those two values travel by wave shuffles, the i-neighbour stays in a register.  Only block-boundary lanes read neighbours'
// results from memory (another workgroup's output, agent-scope loads, NaN sentinel = not yet written) and they request them
// P steps ahead, so in steady state nobody waits: a dependency hop costs a step of register/shuffle work (~0.1 us) instead of
// a memory round trip (~2 us in the level-order sync-free kernel).  Blocks are dispatched in (K, J) order, so a block only
// waits for lower-numbered ones.  The subtraction order is the stored (ascending column) order of the row: bit-identical.
// Rows are fetched in CHUNKS of 8 steps with 16-byte loads, one chunk ahead (a lane's rows are consecutive in memory), so a
// step issues no load of its own; an entry is present iff its coefficient is nonzero (zero entries are never stored).
template <bool FORWARD>
__global__ __launch_bounds__(64) void tri_grid_kernel(const TriArgs* args, const double* in_ptr, double* out_ptr, GridView G, int64_t n) {
    if (args->skip) return;
    constexpr int C = 8;
    const double* __restrict__ in = in_ptr ? in_ptr : args->r;
    double* out = out_ptr ? out_ptr : args->z;
    const int l = threadIdx.x, jl = l & 7, kl = l >> 3, skew = jl + kl;
    const int nbj = (G.Nj + 7) >> 3;
    const int J = blockIdx.x % nbj, K = blockIdx.x / nbj;
    const int jj = J * 8 + jl, kk = K * 8 + kl;                           // schedule coordinates (mirrored for the backward solve)
    const bool line_ok = jj < G.Nj && kk < G.Nk;
    const int j = FORWARD ? jj : G.Nj - 1 - jj, k = FORWARD ? kk : G.Nk - 1 - kk;
    const int32_t s1 = G.Ni, s2 = G.Ni * G.Nj;
    const int64_t line0 = line_ok ? (int64_t)(k * G.Nj + j) * G.Ni : 0;   // row of i = 0 on this line
    const int32_t dj = FORWARD ? -s1 : s1, dk = FORWARD ? -s2 : s2;       // where the j / k neighbour's row lives
    const bool west_glob = line_ok && jl == 0 && J > 0, south_glob = line_ok && kl == 0 && K > 0;
    auto is_sentinel = [](double x) { return (unsigned long long)__double_as_longlong(x) == KR_TRI_SENTINEL; };
    auto row_of = [&](int ii) -> int64_t { return line0 + (FORWARD ? ii : G.Ni - 1 - ii); };   // may lie outside the line (unused then)
    struct Chunk { double rv[C], a1[C], a2[C], a3[C], dg[C], wv[C], sv[C]; };
    // the C rows of steps t .. t+C-1 are contiguous: ascending for the forward solve, descending for the backward one
    auto fetch = [&](Chunk& q, int t) {
        const int ii0 = t - skew;
        const int64_t lo = FORWARD ? row_of(ii0) : row_of(ii0 + C - 1);  // lowest row of the chunk
        if (lo >= 0 && lo + C <= n) {
            typedef double v2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int h = 0; h < C / 2; ++h) {
                const int e0 = FORWARD ? 2 * h : C - 1 - 2 * h, e1 = FORWARD ? 2 * h + 1 : C - 2 - 2 * h;   // step index of the pair's elements
                const v2 r2 = *reinterpret_cast<const v2*>(in + lo + 2 * h);
                const v2 x1 = *reinterpret_cast<const v2*>(G.c1 + lo + 2 * h), x2 = *reinterpret_cast<const v2*>(G.c2 + lo + 2 * h);
                const v2 x3 = *reinterpret_cast<const v2*>(G.c3 + lo + 2 * h);
                q.rv[e0] = r2.x; q.rv[e1] = r2.y; q.a1[e0] = x1.x; q.a1[e1] = x1.y; q.a2[e0] = x2.x; q.a2[e1] = x2.y; q.a3[e0] = x3.x; q.a3[e1] = x3.y;
                if (!FORWARD) { const v2 d2v = *reinterpret_cast<const v2*>(G.diag + lo + 2 * h); q.dg[e0] = d2v.x; q.dg[e1] = d2v.y; }
            }
        } else {                                                           // first / last rows of the whole vector: element-wise, clamped
#pragma unroll
            for (int u = 0; u < C; ++u) {
                const int64_t row = min(max(row_of(ii0 + u), (int64_t)0), n - 1);
                q.rv[u] = in[row]; q.a1[u] = G.c1[row]; q.a2[u] = G.c2[row]; q.a3[u] = G.c3[row];
                if (!FORWARD) q.dg[u] = G.diag[row];
            }
        }
#pragma unroll
        for (int u = 0; u < C; ++u) {                                       // neighbour blocks' results (boundary lanes only)
            const int ii = ii0 + u;
            const bool in_line = ii >= 0 && ii < G.Ni;
            q.wv[u] = (west_glob && in_line) ? __hip_atomic_load(&out[row_of(ii) + dj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            q.sv[u] = (south_glob && in_line) ? __hip_atomic_load(&out[row_of(ii) + dk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
    };
    double y_own = 0.0, y_last = 0.0;
    auto run = [&](Chunk& q, int t0) {
#pragma unroll
        for (int u = 0; u < C; ++u) {
            const int ii = t0 + u - skew;
            const bool act = line_ok && ii >= 0 && ii < G.Ni;
            const int64_t row = row_of(ii);
            double yj = __shfl_up(y_last, 1, 64), yk = __shfl_up(y_last, 8, 64);
            // block-boundary lanes: a value requested a chunk ago that had not been written yet is requested again, now
            bool need_w = act && west_glob && q.a2[u] != 0.0 && is_sentinel(q.wv[u]);
            bool need_s = act && south_glob && q.a3[u] != 0.0 && is_sentinel(q.sv[u]);
            for (int budget = 1 << 22; __any(need_w || need_s) && budget > 0; --budget) {
                if (need_w) { q.wv[u] = __hip_atomic_load(&out[row + dj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); need_w = is_sentinel(q.wv[u]); }
                if (need_s) { q.sv[u] = __hip_atomic_load(&out[row + dk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); need_s = is_sentinel(q.sv[u]); }
                __builtin_amdgcn_s_sleep(1);
            }
            if (west_glob) yj = q.wv[u];
            if (south_glob) yk = q.sv[u];
            double s = q.rv[u];
            if (FORWARD) {                                                // stored order: k-, j-, i-neighbour (ascending column)
                if (q.a3[u] != 0.0) s = s - q.a3[u] * yk;
                if (q.a2[u] != 0.0) s = s - q.a2[u] * yj;
                if (q.a1[u] != 0.0) s = s - q.a1[u] * y_own;
            } else {                                                      // i-, j-, k-neighbour, then the divisor
                if (q.a1[u] != 0.0) s = s - q.a1[u] * y_own;
                if (q.a2[u] != 0.0) s = s - q.a2[u] * yj;
                if (q.a3[u] != 0.0) s = s - q.a3[u] * yk;
                s = s / q.dg[u];
            }
            if (act) {
                y_own = s; y_last = s;
                __hip_atomic_store(&out[row], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    Chunk qa, qb;
    const int nsteps = G.Ni + 14;
    fetch(qa, 0);
    for (int t0 = 0; t0 < nsteps; t0 += 2 * C) {                          // two chunks per trip: the buffers swap roles without copies
        fetch(qb, t0 + C);
        run(qa, t0);
        fetch(qa, t0 + 2 * C);
        run(qb, t0 + C);
    }
}

}  // namespace kr
#include "tri_wave.h"
#include "tri_quad.h"
#include "tri_box.h"
namespace kr {

__global__ __launch_bounds__(256) void tri_fill_kernel(const TriArgs* args, double* dst_ptr, int64_t n, int32_t* flags = nullptr, int32_t nflags = 0) {
    if (args->skip) return;
    if (flags && (int64_t)blockIdx.x * blockDim.x + threadIdx.x < nflags) flags[(int64_t)blockIdx.x * blockDim.x + threadIdx.x] = 0;
    double* dst = dst_ptr ? dst_ptr : args->z;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dst[p] = __longlong_as_double((long long)KR_TRI_SENTINEL);
}

// Structured-grid factor, one launch per hyperplane i + j + k = level (schedule coordinates; mirrored for the backward solve):
// no workgroup waits for another, so it needs no assumption about dispatch order.  ~4 us per level: the fallback of the
// wavefront kernel (tri_wave.h), never the default.  Same subtraction order, same bits.
template <bool FORWARD>
__global__ __launch_bounds__(256) void tri_plane_kernel(const TriArgs* args, const double* in_ptr, double* out_ptr, GridView G, int level) {
    if (args->skip) return;
    const double* in = in_ptr ? in_ptr : args->r;
    double* out = out_ptr ? out_ptr : args->z;
    const int jk = blockIdx.x * blockDim.x + threadIdx.x;
    if (jk >= G.Nj * G.Nk) return;
    const int jj = jk % G.Nj, kk = jk / G.Nj, ii = level - jj - kk;
    if (ii < 0 || ii >= G.Ni) return;
    const int i = FORWARD ? ii : G.Ni - 1 - ii, j = FORWARD ? jj : G.Nj - 1 - jj, k = FORWARD ? kk : G.Nk - 1 - kk;
    const int64_t s1 = G.Ni, s2 = (int64_t)G.Ni * G.Nj;
    const int64_t row = i + s1 * j + s2 * k;
    const double a1 = G.c1[row], a2 = G.c2[row], a3 = G.c3[row];      // 0.0 = no such entry
    double s = in[row];
    if (FORWARD) {                                                     // stored order: k-, j-, i-neighbour (ascending column)
        if (a3 != 0.0) s = s - a3 * out[row - s2];
        if (a2 != 0.0) s = s - a2 * out[row - s1];
        if (a1 != 0.0) s = s - a1 * out[row - 1];
    } else {
        if (a1 != 0.0) s = s - a1 * out[row + 1];
        if (a2 != 0.0) s = s - a2 * out[row + s1];
        if (a3 != 0.0) s = s - a3 * out[row + s2];
        s = s / G.diag[row];
    }
    out[row] = s;
}

// Box-stencil factor, one launch per hyperplane i + 2 j + 4 k = h (schedule coordinates; mirrored for the backward solve): every lower
// offset (dk, dj, di) of the 3 x 3 x 3 cube has di + 2 dj + 4 dk <= -1 -- the closest are (0, -1, +1) and (-1, +1, +1) -- so the rows of a
// plane only need rows of earlier planes.  Ni + 2 Nj + 4 Nk - 6 launches per factor (replayed as a hipGraph): the barrier-free form of the
// box solve, and the one a preconditioner falls back to.  Stored (ascending column) order, absent entries skipped: the reference's bits.
template <bool FORWARD>
__global__ __launch_bounds__(256) void tri_box_plane_kernel(const TriArgs* args, const double* in_ptr, double* out_ptr, BoxView B, int h) {
    if (args->skip) return;
    const double* in = in_ptr ? in_ptr : args->r;
    double* out = out_ptr ? out_ptr : args->z;
    const int jk = blockIdx.x * blockDim.x + threadIdx.x;
    if (jk >= B.Nj * B.Nk) return;
    const int jj = jk % B.Nj, kk = jk / B.Nj, ii = h - 2 * jj - 4 * kk;
    if (ii < 0 || ii >= B.Ni) return;
    const int i = FORWARD ? ii : B.Ni - 1 - ii, j = FORWARD ? jj : B.Nj - 1 - jj, k = FORWARD ? kk : B.Nk - 1 - kk;
    const int64_t s1 = B.Ni, s2 = (int64_t)B.Ni * B.Nj;
    const int64_t row = i + s1 * j + s2 * k;
    double s = in[row];
#pragma unroll
    for (int a = 0; a < 13; ++a) {
        const int code = FORWARD ? a : a + 14;                             // 9 (dk + 1) + 3 (dj + 1) + (di + 1)
        const int dk = code / 9 - 1, dj = (code / 3) % 3 - 1, di = code % 3 - 1;
        const double c = B.c[(int64_t)a * B.cs + row];
        if (c != 0.0) s = s - c * out[row + di + s1 * dj + s2 * dk];
    }
    out[row] = FORWARD ? s : s / B.diag[row];
}

// a run of consecutive NARROW levels [l0, l1) in one workgroup (CSR fallback for factors that do not fit the ELL form)
template <bool FORWARD>
__global__ __launch_bounds__(1024) void tri_run_kernel(const TriArgs* args, const double* __restrict__ in, double* out,
                                                       const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                       const double* __restrict__ val, const double* __restrict__ diag,
                                                       const int32_t* __restrict__ lvl_off, int32_t l0, int32_t l1) {
    if (args->skip) return;
    for (int32_t lv = l0; lv < l1; ++lv) {
        const int32_t p0 = lvl_off[lv], p1 = lvl_off[lv + 1];
        for (int32_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
            double s = in[p];
            for (int32_t k = ptr[p]; k < ptr[p + 1]; ++k) s = s - val[k] * out[col[k]];
            out[p] = FORWARD ? s : s / diag[p];
        }
        __syncthreads();
    }
}

// The same run, software-pipelined: a level of a narrow factor is three DEPENDENT round trips (row pointers -> entries -> solution
// values) and a workgroup barrier, 3.4 us; only the last of the three depends on the level before.  Here the row pointers and the
// right-hand side of level lv + 2 and the first H entries (columns and values) of the rows of level lv + 1 are requested BEFORE level lv
// is computed, so that between two barriers there is one gather of solution values (this workgroup wrote them: L2 at worst), the
// subtractions in stored order and the store.  Each thread owns up to two rows of a level (levels of at most 2 048 rows, 1 024
// threads: the pipelined row is the thread's first one, a second one is done as in tri_run_kernel); rows longer than H continue from
// memory.  The same operations in the same order as tri_run_kernel: same bits.
template <bool FORWARD, int H>
__global__ __launch_bounds__(1024) void tri_run_pipe_kernel(const TriArgs* args, const double* __restrict__ in, double* out,
                                                            const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ diag,
                                                            const int32_t* __restrict__ lvl_off, int32_t l0, int32_t l1) {
    if (args->skip) return;

    struct Head { int32_t p, k0, k1; double s, dg; };                      // a row's position (-1: none), entry range, right-hand side, divisor
    struct Body { int32_t c[H]; double v[H]; };
    auto head_of = [&](int32_t lv) -> Head {
        Head h{-1, 0, 0, 0.0, 1.0};
        if (lv < l1) {
            const int32_t p = lvl_off[lv] + (int32_t)threadIdx.x;
            if (p < lvl_off[lv + 1]) { h.p = p; h.k0 = ptr[p]; h.k1 = ptr[p + 1]; h.s = in[p]; if (!FORWARD) h.dg = diag[p]; }
        }
        return h;
    };
    auto body_of = [&](const Head& h) -> Body {
        Body b;
#pragma unroll
        for (int u = 0; u < H; ++u) {
            const bool on = h.p >= 0 && h.k0 + u < h.k1;
            b.c[u] = on ? col[h.k0 + u] : 0;
            b.v[u] = on ? val[h.k0 + u] : 0.0;
        }
        return b;
    };
    Head hc = head_of(l0), hn = head_of(l0 + 1);
    Body bc = body_of(hc);
    for (int32_t lv = l0; lv < l1; ++lv) {
        // vector loads return in order: the gather of THIS level is requested first, the look-ahead loads behind it, so that the
        // subtractions wait for the gather alone (look-ahead first would put its cold misses back on the level's critical path)
        double x[H];
#pragma unroll
        for (int u = 0; u < H; ++u) x[u] = out[bc.c[u]];                              // (slots past the row's end read position 0: valid, unused)
        asm volatile("" ::: "memory");
        const Body bn = body_of(hn);                                       // in flight while this level is computed
        const Head hnn = head_of(lv + 2);
        asm volatile("" ::: "memory");
        if (hc.p >= 0) {
            double s = hc.s;
#pragma unroll
            for (int u = 0; u < H; ++u) if (hc.k0 + u < hc.k1) s = s - bc.v[u] * x[u];    // stored order
            for (int32_t k = hc.k0 + H; k < hc.k1; ++k) s = s - val[k] * out[col[k]];
            out[hc.p] = FORWARD ? s : s / hc.dg;
        }
        // levels wider than the workgroup (up to 2 048 rows): the rest as in tri_run_kernel
        for (int32_t p = lvl_off[lv] + (int32_t)threadIdx.x + (int32_t)blockDim.x; p < lvl_off[lv + 1]; p += blockDim.x) {
            double s = in[p];
            for (int32_t k = ptr[p]; k < ptr[p + 1]; ++k) s = s - val[k] * out[col[k]];
            out[p] = FORWARD ? s : s / diag[p];
        }
        __syncthreads();
        hc = hn; bc = bn; hn = hnn;
    }
}

// The same run WITHOUT barriers (round 4, late): one workgroup, its waves take the run's positions in chunks of 64, round-robin, and a lane
// waits for the rows ITS row needs instead of for the whole level.  A solved value is published twice: to the solution vector (agent-scope
// store; the vector starts as sentinels, perm_kernel) and to an LDS ring of the last TRF_RING positions as two self-validating 8-byte words
// (32 bits of the value | the position's tag).  EVERY operand of a row is an LDS word pair with an expected tag: a ring slot for a row of this
// run that no wave can have overtaken yet, a constant pair for an absent entry (value +0.0, coefficient set to 0.0: s - 0.0 * 0.0 == s bit for
// bit), a pair private to the lane for an operand from before the run or further back -- gathered from the vector at the chunk's start, ahead
// of the look-ahead loads (vector loads return in order).  So a turn of the loop has no branch per operand: read the eight pairs, compare the
// sixteen tags, and if all agree subtract in stored order and publish.  Three forms of that loop, tried in this order per chunk: LEAN (every
// unsolved lane looks every turn; ~120 instructions, and a lone wave issues one per ~4.5 cycles, so that is the latency of a dependent hop),
// GATED (a lane first polls the pair of its operand at the largest position; passes batched over the wave's lanes) and GENERAL (vector loads
// allowed: rows longer than H, operands not yet in the vector, ring slots reused under a reader -- a LATER tag).  tri_run_kernel's operations
// in tri_run_kernel's order.  Progress: the lowest unsolved position's row needs only solved rows, and the wave that owns its chunk has finished
// all its earlier chunks (all positions below), so it is on that chunk now; every wave of the one workgroup is resident.  Positions that share
// a ring slot belong to one wave (TRF_RING / 64 is a multiple of the wave count) and are solved in order.  The look-ahead: a chunk's operand
// streams (descriptor and coefficient per operand and lane, laid out at set-up: trf_stream_kernel) are requested two chunks ahead with 16 coalesced
// loads, the gathers from the vector one chunk ahead.  Rows of more than eight entries are chains of virtual rows (below).  The waves are held
// within TRF_AHEAD chunks of each other, so that no ring slot is reused under a reader.  A poll budget turns a logic error into NaNs instead of
// a hung GPU.
#define TRF_RING 4096
#define TRF_THREADS 512
#define TRF_AHEAD 8
#define TRF_LDS_BYTES (TRF_RING * 16 + TRF_THREADS * 8 * 16 + 16 + 64)
template <bool FORWARD, int H>
__global__ __launch_bounds__(TRF_THREADS) void tri_run_free_kernel(const TriArgs* args, const double* __restrict__ in, double* out,
                                                                   const double* __restrict__ diag, const int32_t* __restrict__ vreal,
                                                                   const int32_t* __restrict__ fdesc, const double* __restrict__ fval,
                                                                   const int32_t* __restrict__ fpos, int32_t cbase, int32_t NV, int tune) {
    // Positions are VIRTUAL rows of this run, 0 .. NV: a row of at most eight entries is one virtual row; a longer one is a chain of them -- the
    // first with eight operands, each further one with the partial sum of the one before as operand 0 (taken over, not subtracted) and seven
    // more -- and only the last of a chain divides and stores to the vector.  Same subtractions in the same order (trf_stream_kernel).
    static_assert(H == 8, "eight private pairs per lane");
    if (args->skip) return;
    extern __shared__ unsigned long long trf_lds[];                      // [TRF_RING][2] ring, [TRF_THREADS][8][2] private pairs, [2] the constant pair
    constexpr uint32_t PRIV = TRF_RING * 2, CONSTP = PRIV + TRF_THREADS * 16;      // (in words)
    constexpr uint32_t TAG_PRIV = 0xFFFFFFFEu, TAG_CONST = 0xFFFFFFFFu;
    for (int x = threadIdx.x; x < (int)CONSTP; x += blockDim.x) trf_lds[x] = 0ull;         // tag 0: never written (LDS is not cleared between kernels)
    if (threadIdx.x == 0) { trf_lds[CONSTP] = (unsigned long long)TAG_CONST << 32; trf_lds[CONSTP + 1] = (unsigned long long)TAG_CONST << 32; }
    const int W = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t nchunk = (NV + 63) >> 6;
    // Which chunk every wave is on (all its earlier ones are finished): a wave starts chunk c only when no wave is more than TRF_AHEAD chunks
    // behind it.  An operand is taken from the ring up to `reach` = 55 chunks back (trf_stream_kernel), a slot is reused 64 chunks on: with
    // 55 + TRF_AHEAD < 64 no pair is overwritten while a row that reads it is unsolved.  (Without it a wave whose rows need nothing of a slow
    // wave's chunk ran 64 chunks ahead on a 27-point box and overwrote the partial sum a chain was waiting for.)
    int* const wave_at = reinterpret_cast<int*>(&trf_lds[CONSTP + 2]);
    if (lane == 0) __hip_atomic_store(&wave_at[w], w < nchunk ? w : INT32_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const int batch = tune & 255;

    struct Head { int32_t p, vp; bool first, last; double s, dg; };       // p: the row's position in the vector (-1: no row), vp: virtual position
    struct Stage { int32_t d[H]; double v[H]; };                           // a chunk's operand streams: descriptor and coefficient of operand u of this lane's row
    // every load of the look-ahead is issued by every lane (clamped indices): the waits can then be COUNTED (s_waitcnt vmcnt(n))
    auto head_of = [&](int32_t ch) -> Head {
        Head h;
        const int32_t cc = ch < nchunk ? ch : nchunk - 1;
        const int32_t vr = *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(vreal) + ((uint32_t)(cbase + cc) * 64u + (uint32_t)lane) * 4u);
        const bool valid = ch < nchunk && vr != 0;
        const uint32_t pc = valid ? (uint32_t)(vr & 0x1FFFFFFF) - 1u : 0u;
        h.s = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(in) + pc * 8u);
        h.dg = FORWARD ? 1.0 : *reinterpret_cast<const double*>(reinterpret_cast<const char*>(diag) + pc * 8u);
        h.p = valid ? (int32_t)pc : -1;
        h.vp = (ch << 6) + lane;
        h.first = (vr >> 30) & 1; h.last = (vr >> 29) & 1;
        return h;
    };
    // 16 fully coalesced loads (32-bit byte offsets from the uniform base: one address instruction per load).  (With each lane loading ITS row's
    // entries from the CSR arrays -- the pipe kernel's way -- every cache line is asked for by eight different instructions: 650 L1 accesses per
    // chunk, the L1 busy or stalled on pending lines for 60 % of the run; PMC, round 4.)
    auto stage_of = [&](int32_t ch, Stage& st) {
        const uint32_t base = (uint32_t)(cbase + (ch < nchunk ? ch : nchunk - 1)) * (uint32_t)(H * 64) + (uint32_t)lane;
#pragma unroll
        for (int u = 0; u < H; ++u) {
            st.d[u] = *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(fdesc) + (base + 64u * u) * 4u);
            st.v[u] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(fval) + (base + 64u * u) * 8u);
        }
    };
    auto pair_at = [&](uint32_t word, unsigned long long& a, unsigned long long& b) {
        a = __hip_atomic_load(&trf_lds[word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        b = __hip_atomic_load(&trf_lds[word + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto put_pair = [&](uint32_t word, double x, uint32_t tag) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x), t = (unsigned long long)tag << 32;
        __hip_atomic_store(&trf_lds[word], (bits & 0xffffffffull) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&trf_lds[word + 1], (bits >> 32) | t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto publish = [&](const Head& h, double res) {                        // (a partial sum only to the ring: its one reader is the next virtual row)
        if (h.last) __hip_atomic_store(&out[h.p], res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        put_pair(((uint32_t)h.vp & (TRF_RING - 1)) * 2, res, (uint32_t)h.vp + 1u);
    };
    auto solved = [](double x) { return (unsigned long long)__double_as_longlong(x) != KR_TRI_SENTINEL; };
    // one chunk: its head hc and its operand streams bc are here; the next chunk's streams (into st) and the head after that are requested on the way
    auto chunk = [&](const Head& hc, const Stage& bc, const Stage& nx, Stage& st, Head& hnn, int32_t ch, double (&xg)[H]) {
        const int len = H, nh = H;                                         // (rows longer than H are chains of virtual rows: nothing is left over)
        if (lane == 0) __hip_atomic_store(&wave_at[w], ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (int spins = 0; spins < (1 << 24); ++spins) {
            const int at = __hip_atomic_load(&wave_at[lane < W ? lane : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (__all(ch - at <= TRF_AHEAD)) break;
            __builtin_amdgcn_s_sleep(2);
        }
        // every operand as (word offset of its pair, expected tag); bit u of `vecm`: operand u comes from the vector, of `vpend`: ... and is not there yet
        uint32_t word[H], etag[H];
        unsigned vecm = 0, vpend = 0;
        int32_t gpos = -1;                                                 // (the largest ring tag among the operands)
        // the operand's position in the vector: in its descriptor, or -- for a ring operand, asked for only when its slot has been reused -- in the
        // third stream
        auto pos_of = [&](int u) -> int32_t {
            if (bc.d[u] < 0) return (int32_t)((uint32_t)bc.d[u] & 0x7fffffffu);
            return fpos[((size_t)(cbase + ch) * H + u) * 64 + lane];
        };
#pragma unroll
        for (int u = 0; u < H; ++u) {
            const int32_t d = hc.p >= 0 ? bc.d[u] : 0;
            const bool near = d > 0, vec = d < 0;
            word[u] = near ? ((uint32_t)(d - 1) & (TRF_RING - 1)) * 2 : vec ? PRIV + (threadIdx.x * 8 + u) * 2 : CONSTP;
            etag[u] = near ? (uint32_t)d : vec ? TAG_PRIV : TAG_CONST;
            if (vec) vecm |= 1u << u;
            if (near) gpos = d > gpos ? d : gpos;
        }
        // Gathers from the vector.  They are requested ONE CHUNK AHEAD (the next chunk's descriptors are here by now; an operand that far back has
        // long been solved -- if not, the pair stays invalid and the general loop polls the vector), by every lane for every operand (lanes without
        // such an operand at one common address) and in front of the look-ahead, so that every wait is a COUNTED one.  (Waited for in per-operand
        // branches at the chunk's start they were two or three L2 round trips one after the other: 30 -> 23 ms; a chunk ahead: no wait at all.)
        if (__any(vecm != 0)) {
#pragma unroll
            for (int u = 0; u < H; ++u)
                if ((vecm >> u) & 1u) { const bool ok = solved(xg[u]); put_pair(word[u], xg[u], ok ? TAG_PRIV : 0u); if (!ok) vpend |= 1u << u; }
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < H; ++u)
            xg[u] = __hip_atomic_load(&out[nx.d[u] < 0 ? (int32_t)((uint32_t)nx.d[u] & 0x7fffffffu) : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::: "memory");
        stage_of(ch + 2 * W, st);                                          // the look-ahead: in flight while this chunk and the next wait and compute
        hnn = head_of(ch + 2 * W);
        asm volatile("" ::: "memory");
        bool done = hc.p < 0, wait = !done && gpos > 0, headdone = false;
        double s = hc.s;
        int cons = 0, fails = 0;
        const uint32_t gword = ((uint32_t)(gpos - 1) & (TRF_RING - 1)) * 2, ge = (uint32_t)gpos;
        int budget = 1 << 22, since = 0, idle = 0;
        // FAST: no vector-memory load inside the loop -- the common case.  (With one anywhere in the loop body the compiler has to wait for ALL
        // outstanding loads, the look-ahead included, at the top of every iteration: the loaded registers may be the ones a poll writes.)
        // A lane that needs the vector or has a row longer than H raises `rare`, and the chunk is finished by the general form of the loop.
        auto run = [&](auto fast_tag) -> bool {
            constexpr bool FAST = decltype(fast_tag)::value;
            for (;;) {
                bool moved = false, rare = false;
                if (wait) {                                                // the gate: one word pair (a LATER tag opens it too: the pass sorts that out)
                    unsigned long long a, b; pair_at(gword, a, b);
                    const uint32_t ta = (uint32_t)(a >> 32), tb = (uint32_t)(b >> 32);
                    if ((ta < tb ? ta : tb) >= ge) wait = false;
                }
                const bool open = !wait && !done;
                ++since;
                if (__any(open) && (!__any(wait) || since >= batch)) {
                    since = 0;
                    if (open && !headdone) {
                        unsigned long long ra[H], rb[H];
#pragma unroll
                        for (int u = 0; u < H; ++u) pair_at(word[u], ra[u], rb[u]);
                        uint32_t bad = 0;                                  // (no branch per operand)
#pragma unroll
                        for (int u = 0; u < H; ++u) bad |= ((uint32_t)(ra[u] >> 32) ^ etag[u]) | ((uint32_t)(rb[u] >> 32) ^ etag[u]);
                        if (bad == 0) {
#pragma unroll
                            for (int u = 0; u < H; ++u) {                  // stored order (absent: s - 0.0 * 0.0); operand 0 of a chain's later rows IS s
                                const double x = __longlong_as_double((long long)((ra[u] & 0xffffffffull) | (rb[u] << 32)));
                                const double t = bc.v[u] * x;
                                s = (u == 0 && !hc.first) ? x : s - t;
                            }
                            headdone = true; cons = nh;
                        } else if (++fails >= 3) {
                            // rare: a ring slot that belongs to a later position now, or an operand that was not in the vector when gathered
                            if constexpr (FAST) rare = true;
                            else {
#pragma unroll
                                for (int u = 0; u < H; ++u) {
                                    const bool over = etag[u] < TAG_PRIV && ((uint32_t)(ra[u] >> 32) > etag[u] || (uint32_t)(rb[u] >> 32) > etag[u]);
                                    if (over) { word[u] = PRIV + (threadIdx.x * 8 + u) * 2; etag[u] = TAG_PRIV; put_pair(word[u], 0.0, 0u); vecm |= 1u << u; vpend |= 1u << u; }
                                    if ((vpend >> u) & 1u) {
                                        const double x = __hip_atomic_load(&out[pos_of(u)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        if (solved(x)) { put_pair(word[u], x, TAG_PRIV); vpend &= ~(1u << u); }
                                    }
                                }
                            }
                        }
                        moved = true;
                    }
                    if (open && headdone && cons >= len) {
                        publish(hc, (FORWARD || !hc.last) ? s : s / hc.dg);
                        done = true; moved = true;
                    }
                }
                if (__all(done)) return true;
                if (FAST && __any(rare)) return false;
                if (--budget <= 0) {                                       // a logic error: NaNs, not a hung GPU
                    if (!done) publish(hc, __longlong_as_double(0x7FF8000000000000ll));
                    return true;
                }
                // a wave that makes progress is at the front: it gets the SIMD ahead of the waves that only look; those back off
                if (__any(moved)) { if (idle && (tune & 256)) __builtin_amdgcn_s_setprio(3); idle = 0; }
                else {
                    if (!idle && (tune & 256)) __builtin_amdgcn_s_setprio(0);
                    if (idle < ((tune >> 9) & 15)) ++idle;
                    for (int q = 0; q < idle; ++q) __builtin_amdgcn_s_sleep(1);
                }
            }
        };
        // LEAN: the loop a chunk normally lives in -- every unsolved lane whose gate is open looks at all its operands every turn (no batching, no
        // bookkeeping per lane: a lone wave issues an instruction every ~4.5 cycles, so the turn's LENGTH is the hop's latency).  It leaves to the
        // loops above when a lane has a row longer than H or an operand that was not in the vector, or when a ring slot has been
        // reused under a reader (looked for every 16th turn without progress).
        auto lean = [&]() -> bool {
            if (tune & 8192) return false;
            if (__any(!done && vpend != 0)) return false;
            bool stuck = false;
            for (int quiet = 0;;) {
                bool got = false;
                if (wait && (tune & 16384)) wait = false;
                if (wait) {                                                // the gate: one word pair (waves that are early keep the LDS free)
                    unsigned long long a, b; pair_at(gword, a, b);
                    const uint32_t ta = (uint32_t)(a >> 32), tb = (uint32_t)(b >> 32);
                    if ((ta < tb ? ta : tb) >= ge) wait = false;
                }
                if (!done && !wait) {
                    unsigned long long ra[H], rb[H];
#pragma unroll
                    for (int u = 0; u < H; ++u) pair_at(word[u], ra[u], rb[u]);
                    uint32_t bad = 0;
#pragma unroll
                    for (int u = 0; u < H; ++u) bad |= ((uint32_t)(ra[u] >> 32) ^ etag[u]) | ((uint32_t)(rb[u] >> 32) ^ etag[u]);
                    if (bad == 0) {
#pragma unroll
                        for (int u = 0; u < H; ++u) {                      // stored order (absent: s - 0.0 * 0.0); operand 0 of a chain's later rows IS s
                            const double x = __longlong_as_double((long long)((ra[u] & 0xffffffffull) | (rb[u] << 32)));
                            const double t = bc.v[u] * x;
                            s = (u == 0 && !hc.first) ? x : s - t;
                        }
                        publish(hc, (FORWARD || !hc.last) ? s : s / hc.dg);
                        done = true; got = true;
                    } else if ((quiet & 15) == 15) {                       // now and then: has one of my ring slots been reused under me?
#pragma unroll
                        for (int u = 0; u < H; ++u)
                            stuck = stuck || (etag[u] < TAG_PRIV && ((uint32_t)(ra[u] >> 32) > etag[u] || (uint32_t)(rb[u] >> 32) > etag[u]));
                    }
                }
                if (__all(done)) return true;
                if (__any(got)) quiet = 0;
                else { if (++quiet > 4096 || __any(stuck)) return false; __builtin_amdgcn_s_sleep(1); }
            }
        };
        if (!lean()) if (!run(std::true_type{})) run(std::false_type{});
    };
    Head hc = head_of(w), hn = head_of(w + W), hnn;
    Stage sa, sb, sc;
    double xg[H];
    stage_of(w, sa);
#pragma unroll
    for (int u = 0; u < H; ++u)
        xg[u] = __hip_atomic_load(&out[sa.d[u] < 0 ? (int32_t)((uint32_t)sa.d[u] & 0x7fffffffu) : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stage_of(w + W, sb);
    for (int32_t ch = w; ch < nchunk; ch += 3 * W) {
        chunk(hc, sa, sb, sc, hnn, ch, xg);
        if (ch + W >= nchunk) break;
        hc = hn; hn = hnn;
        chunk(hc, sb, sc, sa, hnn, ch + W, xg);
        if (ch + 2 * W >= nchunk) break;
        hc = hn; hn = hnn;
        chunk(hc, sc, sa, sb, hnn, ch + 2 * W, xg);
        hc = hn; hn = hnn;
    }
    if (lane == 0) __hip_atomic_store(&wave_at[w], INT32_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the operand streams of one narrow run (see TriFactor, tri_run_free_kernel): one thread per row of the run; `vstart` = first virtual row of
// every row of the run (and the run's total behind the last).  The streams were zeroed before: 0 = no row / no such entry.
__global__ __launch_bounds__(256) void trf_stream_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                         int32_t P0, int32_t P1, int32_t reach, int32_t cbase, const int32_t* __restrict__ vstart,
                                                         int32_t* vreal, int32_t* fdesc, double* fval, int32_t* fpos) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P1 - P0) return;
    const int32_t p = P0 + i, k0 = ptr[p], L = ptr[p + 1] - k0, v0 = vstart[i], nv = vstart[i + 1] - v0;
    for (int32_t j = 0; j < nv; ++j) {
        const int32_t vp = v0 + j;
        const size_t cl = (size_t)(cbase + (vp >> 6)) * 64 + (size_t)(vp & 63), base = (size_t)(cbase + (vp >> 6)) * 512 + (size_t)(vp & 63);
        vreal[cl] = ((p + 1) & 0x1FFFFFFF) | (j == 0 ? 1 << 30 : 0) | (j == nv - 1 ? 1 << 29 : 0);
        for (int u = 0; u < 8; ++u) {
            int32_t d = 0, c = 0; double v = 0.0;
            if (j > 0 && u == 0) { d = vp; v = 1.0; c = p; }             // the partial sum of the virtual row before (its tag: (vp - 1) + 1)
            else {
                const int32_t e = j == 0 ? u : 8 + (j - 1) * 7 + (u - 1);                // the row's entry in this slot
                if (e < L) {
                    c = col[k0 + e]; v = val[k0 + e];
                    const int32_t vl = c >= P0 ? vstart[c - P0 + 1] - 1 : -1;             // the LAST virtual row of the operand's row holds its value
                    d = (c >= P0 && vp - vl < reach) ? vl + 1 : (int32_t)(0x80000000u | (uint32_t)c);
                }
            }
            fdesc[base + 64 * (size_t)u] = d; fval[base + 64 * (size_t)u] = v; fpos[base + 64 * (size_t)u] = c;
        }
    }
}

// runs in stream order before the level kernels, so it sees the solver's `done` flag as of this apply
__global__ void tri_set_args(TriArgs* a, const double* r, double* z, const int* done) {
    a->r = r; a->z = z; a->skip = (done && *done) ? 1 : 0;
    a->epoch = (a->epoch & 0x3fffffff) + 1;         // 1, 2, ... (d_args is zeroed at setup); never 0, the flags' initial value
}

// dst[p] = src[map[p]]   (MODE 0: src = the caller's r;  MODE 1: plain gather;  MODE 2: scatter into the caller's z: z[map[p]] = src[p])
template <int MODE>
__global__ __launch_bounds__(256) void perm_kernel(const TriArgs* args, double* dst, const double* src, const int32_t* __restrict__ map, int64_t n,
                                                   double* fill) {
    if (args->skip) return;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (MODE == 0) dst[p] = args->r[map[p]];
    else if (MODE == 1) dst[p] = src[map[p]];
    else args->z[map[p]] = src[p];
    if (fill) fill[p] = __longlong_as_double((long long)KR_TRI_SENTINEL);     // "not yet solved" marks for the sync-free kernel
}

// KRYST_ILU_RUN_FREE (default 1): runs of narrow levels without barriers; needs 128 KiB of LDS, twice what a kernel gets without asking
// `long_rows`: the share of the factor's rows with more than eight entries.  Such a row is a chain of virtual rows in the kernel's streams (before
// that it sent its whole chunk to a loop that took its entries from memory one at a time, and factors with more than 2 % of them were better off
// with the barrier kernel: 12 entries per row of A 32.4 ms against 22.9; as chains 12.2).  KRYST_ILU_FREE_LONG_PCT (default 100) brings the limit back.
static bool grant_free_runs(double long_rows) {
    if (env_int("KRYST_ILU_RUN_FREE", 1) == 0) return false;
    if (long_rows > 0.01 * (double)env_int("KRYST_ILU_FREE_LONG_PCT", 100) && env_int("KRYST_ILU_RUN_FREE", 1) < 2) return false;
    const bool ok = hipFuncSetAttribute((const void*)tri_run_free_kernel<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, TRF_LDS_BYTES) == hipSuccess &&
                    hipFuncSetAttribute((const void*)tri_run_free_kernel<false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, TRF_LDS_BYTES) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}


// The operand streams of every narrow run of a factor that takes tri_run_free_kernel (F->free_runs), in the order enqueue_factor meets the runs.
// `hptr`: the factor's row pointers on the host.  8 KiB per chunk of 64 virtual rows.  Not enough memory, or offsets past 32 bits: the factor keeps
// the barrier kernel (free_runs = false).
int32_t build_free_streams(TriFactor* F, hipStream_t st, const int32_t* hptr) {
    // tri_run_free_kernel packs a row's absolute position into 29 bits of `vreal` (flags at bits 29, 30) and forms byte offsets in 32 bits:
    // a factor of 2^29 rows or more -- it would fit a 288 GB card -- takes the pipe / sync-free kernels instead
    if (F->free_runs && F->npos >= (1ll << 29)) F->free_runs = false;
    if (!F->free_runs) return KRYST_OK;
    const int nl = (int)F->lvl_off.size() - 1;
    std::vector<std::pair<int32_t, int32_t>> runs;
    std::vector<size_t> voff;                              // where a run's vstart begins in `vs`
    hvec<int32_t> vs;
    size_t chunks = 0;
    for (int lv = 0; lv < nl;) {
        if (F->lvl_off[lv + 1] - F->lvl_off[lv] <= NARROW) {
            int l1 = lv + 1;
            while (l1 < nl && F->lvl_off[l1 + 1] - F->lvl_off[l1] <= NARROW) ++l1;
            const int32_t P0 = F->lvl_off[lv], P1 = F->lvl_off[l1];
            runs.emplace_back(P0, P1);
            voff.push_back(vs.size());
            int64_t v = 0;
            vs.push_back(0);
            for (int32_t p = P0; p < P1; ++p) { const int32_t L = hptr[p + 1] - hptr[p]; v += L <= 8 ? 1 : 1 + (L - 8 + 6) / 7; vs.push_back((int32_t)std::min<int64_t>(v, INT32_MAX)); }
            if (v >= (1ll << 29)) { chunks = 0; runs.clear(); break; }
            F->run_cbase.push_back((int32_t)chunks);
            F->run_nvirt.push_back((int32_t)v);
            chunks += (size_t)(v + 63) / 64;
            lv = l1;
        } else ++lv;
    }
    int32_t* d_vs = nullptr;
    const bool ok = chunks > 0 && chunks * 512 * 8 < ((size_t)1 << 32) &&
                    pool_malloc(&F->d_fdesc, chunks * 512 * sizeof(int32_t)) == hipSuccess && pool_malloc(&F->d_fval, chunks * 512 * sizeof(double)) == hipSuccess &&
                    pool_malloc(&F->d_fpos, chunks * 512 * sizeof(int32_t)) == hipSuccess && pool_malloc(&F->d_vreal, chunks * 64 * sizeof(int32_t)) == hipSuccess &&
                    pool_malloc(&d_vs, vs.size() * sizeof(int32_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        (void)pool_free(F->d_fdesc); (void)pool_free(F->d_fval); (void)pool_free(F->d_fpos); (void)pool_free(F->d_vreal); (void)pool_free(d_vs);
        F->d_fdesc = nullptr; F->d_fval = nullptr; F->d_fpos = nullptr; F->d_vreal = nullptr; F->run_cbase.clear(); F->run_nvirt.clear();
        F->free_runs = false;
        if (F->ell) F->syncfree = true;                    // (an ELL factor's other form)
        return KRYST_OK;
    }
    // an operand counts as "in the ring" when no wave can have reused its slot yet in the ordinary course of things: the most advanced wave is
    // held within TRF_AHEAD chunks of the least advanced one (tri_run_free_kernel: wave_at); 16 instead of 8 with a shorter reach: 20.2 ms against 20.0
    const int32_t reach = TRF_RING - 64 * (TRF_AHEAD + 1);
    hipError_t e = hipMemcpyAsync(d_vs, vs.data(), vs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(F->d_fdesc, 0, chunks * 512 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(F->d_fval, 0, chunks * 512 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(F->d_fpos, 0, chunks * 512 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(F->d_vreal, 0, chunks * 64 * sizeof(int32_t), st);
    for (size_t r = 0; e == hipSuccess && r < runs.size(); ++r) {
        const int32_t rows = runs[r].second - runs[r].first;
        hipLaunchKernelGGL(trf_stream_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, F->d_ptr, F->d_col, F->d_val, runs[r].first, runs[r].second,
                           reach, F->run_cbase[r], d_vs + voff[r], F->d_vreal, F->d_fdesc, F->d_fval, F->d_fpos);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)pool_free(d_vs);
    if (e != hipSuccess) { set_error("operand streams of the run kernel: %s", hipGetErrorString(e)); return KRYST_ERR_HIP; }
    return KRYST_OK;
}

template <bool FORWARD>
static int32_t enqueue_factor(hipStream_t s, const TriFactor& F, const TriArgs* d_args, const double* in, double* out) {
    if (F.syncfree && F.npos > 0) {
        const dim3 grid((unsigned)((F.npos + 255) / 256));
        if (F.ell) hipLaunchKernelGGL((tri_syncfree_ell_kernel<FORWARD>), grid, dim3(256), 0, s, d_args, in, out, F.view(), F.d_diag, (int32_t)F.npos);
        // (Ilup(1) on a 7-point operator, 6 entries per row: 7.3 -> 5.9 ms per apply with 8 held, 6.3 with 16; a 27-point factor, 13 per
        // row: 9.8 -> 9.4 with 8, 6.9 with 16)
        else if (env_int("KRYST_ILU_CSR_HELD", F.held) <= 8) hipLaunchKernelGGL((tri_syncfree_csr_kernel<FORWARD, 8>), grid, dim3(256), 0, s, d_args, in, out, F.d_ptr, F.d_col, F.d_val, F.d_diag,
                                (int32_t)F.npos);
        else hipLaunchKernelGGL((tri_syncfree_csr_kernel<FORWARD, 16>), grid, dim3(256), 0, s, d_args, in, out, F.d_ptr, F.d_col, F.d_val, F.d_diag,
                                (int32_t)F.npos);
        KR_HIP(hipGetLastError());
        return KRYST_OK;
    }
    const int nl = (int)F.lvl_off.size() - 1;
    int lv = 0;
    size_t run_index = 0;
    while (lv < nl) {
        const int rows = F.lvl_off[lv + 1] - F.lvl_off[lv];
        if (rows <= NARROW && (!F.ell || F.free_runs)) {
            int l1 = lv + 1;
            while (l1 < nl && F.lvl_off[l1 + 1] - F.lvl_off[l1] <= NARROW) ++l1;
            // Threads: what a level costs is the instructions every wave of the workgroup issues for it, needed or not -- the random band
            // matrix of tools/band_apply.py (187 rows per level): 46.1 ms per apply with 1 024 threads, 39.2 with 512, 34.4 with 256, 35.8 with 320,
            // 79.5 with 128 (only a thread's first row of a level is pipelined).  Hence 5/4 of the run's mean level width, 256 at least.
            // (Not the branches around its predicated look-ahead loads: with every load unconditional -- clamped indices, straight-line code,
            // half the instructions -- the same apply took 38.7 ms, and 38.2 with the last 8 192 solution values in an LDS ring:
            // profiles/r04/narrow_level_kernel_experiments.txt.)
            const int mean_rows = (int)((F.lvl_off[l1] - F.lvl_off[lv]) / std::max(1, l1 - lv));
            const unsigned run_threads = (unsigned)std::min(1024, std::max(64, env_int("KRYST_ILU_RUN_THREADS", std::max(256, (mean_rows * 5 / 4 + 63) / 64 * 64)) / 64 * 64));
            if (F.free_runs) {
                // (waves: a power of two, so that the positions that share a ring slot belong to ONE wave and are solved in order)
                // (8 waves where a level fills a wave; 4 on narrower levels, where the waves that only wait cost the one that works:
                // 22 rows per level 0.50 us per level against 0.53, 3 rows 0.42 against 0.44; 187 rows: 30.4 ms with 8, 42.6 with 4)
                const int fw = env_int("KRYST_ILU_FREE_WAVES", mean_rows >= 64 ? 8 : 4);
                const unsigned waves = fw >= 8 ? 8u : fw >= 4 ? 4u : fw >= 2 ? 2u : 1u;
                hipLaunchKernelGGL((tri_run_free_kernel<FORWARD, 8>), dim3(1), dim3(64 * waves), (size_t)TRF_LDS_BYTES, s, d_args, in, out, F.d_diag, F.d_vreal,
                                   F.d_fdesc, F.d_fval, F.d_fpos, F.run_cbase[run_index], F.run_nvirt[run_index], env_int("KRYST_ILU_FREE_TUNE", 1 | (1 << 9) | 16384));
                ++run_index;
            } else if (env_int("KRYST_ILU_RUN_PIPE", 1) != 0)
                hipLaunchKernelGGL((tri_run_pipe_kernel<FORWARD, 8>), dim3(1), dim3(run_threads), 0, s, d_args, in, out, F.d_ptr, F.d_col, F.d_val,
                                   F.d_diag, F.d_lvl_off, lv, l1);
            else
                hipLaunchKernelGGL((tri_run_kernel<FORWARD>), dim3(1), dim3(1024), 0, s, d_args, in, out, F.d_ptr, F.d_col, F.d_val,
                                   F.d_diag, F.d_lvl_off, lv, l1);
            lv = l1;
        } else {
            if (F.ell)
                hipLaunchKernelGGL((tri_level_ell_kernel<FORWARD>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_args, in, out,
                                   F.view(), F.d_diag, F.lvl_off[lv], F.lvl_off[lv + 1]);
            else
                hipLaunchKernelGGL((tri_level_kernel<FORWARD>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_args, in, out, F.d_ptr,
                                   F.d_col, F.d_val, F.d_diag, F.lvl_off[lv], F.lvl_off[lv + 1]);
            lv += 1;
        }
        KR_HIP(hipGetLastError());
    }
    return KRYST_OK;
}

// The launch sequences an apply can take.  laid_out_form: what the factors and the state permit; apply_form: that, plus the per-apply
// KRYST_ILU_PLANES override.  Everything that has to know the form -- enqueue_apply, the direct launch and the graph default of IluPc::apply,
// check_after_apply, kryst_pc_ilu_info, the set-up's verbose line -- asks these two.
enum class IluForm {
    Level,          // level-ordered factors: permute, enqueue_factor twice, permute back
    GridOneWave,    // tri_grid_kernel: one wave per 8 x 8 lines (KRYST_ILU_WAVE=0, and any grid with Ni == 1)
    GridWave,       // tri_wave_kernel: 8 x 8 lines per workgroup (tri_wave.h)
    GridQuad,       // tri_quad_kernel: 16 x 16 lines per workgroup on the blocked copy (tri_quad.h)
    GridPlanes,     // tri_plane_kernel: one launch per hyperplane i + j + k (after a give-up, or KRYST_ILU_PLANES)
    BoxWave,        // tri_box_kernel: pipelined wavefront over parallelograms of 8 x 8 lines (tri_box.h)
    BoxPlanes       // tri_box_plane_kernel: one launch per hyperplane i + 2 j + 4 k (KRYST_ILU_BOX=1, KRYST_ILU_PLANES, no blocked copy, or after a give-up)
};
static bool grid_wavefront(IluForm f) { return f == IluForm::GridOneWave || f == IluForm::GridWave || f == IluForm::GridQuad; }

static bool quad_laid_out(const IluPc* pc) { return ilu_wave_knob(pc->GL) >= 2 && pc->GL.d_blocked && pc->GU.d_blocked; }   // the blocked copy exists and is wanted
static IluForm laid_out_form(const IluPc* pc) {
    if (pc->box()) return pc->box_wave_ready && !pc->safe && ilu_box_knob() >= 2 ? IluForm::BoxWave : IluForm::BoxPlanes;
    if (!pc->grid()) return IluForm::Level;
    if (pc->safe) return IluForm::GridPlanes;
    if (quad_laid_out(pc)) return IluForm::GridQuad;
    return ilu_wave_knob(pc->GL) > 0 && pc->GL.Ni >= 2 ? IluForm::GridWave : IluForm::GridOneWave;
}
static IluForm apply_form(const IluPc* pc) {
    const IluForm f = laid_out_form(pc);
    if ((grid_wavefront(f) || f == IluForm::BoxWave) && ilu_planes_knob()) return f == IluForm::BoxWave ? IluForm::BoxPlanes : IluForm::GridPlanes;
    return f;
}

// info[0] of kryst_pc_ilu_info: 0 level-ordered, 1 grid 8 x 8, 2 grid 16 x 16, 3 grid after a give-up, 4 box planes, 5 box wavefront.
// What is reported is not symmetric between the two structured forms, and callers rely on it as it is (tests/nonfinite_cases.py):
//   * a grid reports what is LAID OUT: 1 for the one-wave kernel too (KRYST_ILU_WAVE=0, Ni == 1), and "grid 8x8" / "16x16" under KRYST_ILU_PLANES=1,
//     although the plane kernels then run; 3 only after a give-up;
//   * a box reports what an apply TAKES: 4 under KRYST_ILU_PLANES=1;
//   * likewise check_after_apply is true for any grid that has not given up, whatever KRYST_ILU_PLANES says, but for a box only when the
//     wavefront kernels run; and a hipGraph is the default (few_launches false) for every form under KRYST_ILU_PLANES=1, the level-ordered
//     sync-free one included, although that knob changes nothing else about it.
static int form_info(const IluPc* pc) {
    if (pc->box()) return apply_form(pc) == IluForm::BoxWave ? 5 : 4;
    switch (laid_out_form(pc)) {
        case IluForm::Level: return 0;
        case IluForm::GridPlanes: return 3;
        case IluForm::GridQuad: return 2;
        default: return 1;
    }
}
// a hipGraph pays where an apply is MANY launches (one per dependency level / hyperplane); the wavefront and the sync-free forms are
// three to five launches, and launching them directly is 0.6 % (256^3) to 1.9 % (128^3) of a BiCGStab + ILU(0) iteration faster
static bool few_launches(const IluPc* pc, IluForm f) {
    return grid_wavefront(f) || f == IluForm::BoxWave || (f == IluForm::Level && pc->L.syncfree && pc->U.syncfree && !ilu_planes_knob());
}

// r -> rL (L level order) -> forward -> yL -> yU (U level order) -> backward -> zU -> z
// the structured forms work in natural order, r -> forward -> y -> backward -> z, no permutations: the factors as kernel arguments
static GridView grid_view(const GridFactor& G, bool forward) { return GridView{G.Ni, G.Nj, G.Nk, G.d_c1, G.d_c2, G.d_c3, forward ? nullptr : G.d_diag}; }
static BoxView box_view(const BoxFactor& B, int64_t n, bool forward) { return BoxView{B.Ni, B.Nj, B.Nk, n, B.d_c, forward ? nullptr : B.d_diag, box_stream_stride(n), B.d_cb}; }
static int poll_budget() { return std::max(1, env_int("KRYST_ILU_POLL_BUDGET", 1 << 22)); }   // (tests force the give-up path with a tiny budget)

static int32_t enqueue_apply(hipStream_t s, IluPc* pc, IluForm form, const TriDirect* direct = nullptr) {
    const int64_t n = pc->n;
    const unsigned g = (unsigned)((n + 255) / 256);
    const GridFactor& GA = pc->GL; const GridFactor& GB = pc->GU;
    const BoxFactor& BA = pc->BL; const BoxFactor& BB = pc->BU;
    switch (form) {
    case IluForm::Level:
        hipLaunchKernelGGL((perm_kernel<0>), dim3(g), dim3(256), 0, s, pc->d_args, pc->d_rL, (const double*)nullptr, pc->L.d_row, n,
                           (pc->L.syncfree || pc->L.free_runs) ? pc->d_y : (double*)nullptr);
        KR_HIP(hipGetLastError());
        KR_TRY(enqueue_factor<true>(s, pc->L, pc->d_args, pc->d_rL, pc->d_y));
        hipLaunchKernelGGL((perm_kernel<1>), dim3(g), dim3(256), 0, s, pc->d_args, pc->d_yU, (const double*)pc->d_y, pc->d_mapLU, n,
                           (pc->U.syncfree || pc->U.free_runs) ? pc->d_zU : (double*)nullptr);
        KR_HIP(hipGetLastError());
        KR_TRY(enqueue_factor<false>(s, pc->U, pc->d_args, pc->d_yU, pc->d_zU));
        hipLaunchKernelGGL((perm_kernel<2>), dim3(g), dim3(256), 0, s, pc->d_args, (double*)nullptr, (const double*)pc->d_zU, pc->U.d_row, n,
                           (double*)nullptr);
        break;
    case IluForm::GridOneWave: {
        const GridView VA = grid_view(GA, true), VB = grid_view(GB, false);
        const unsigned nb = (unsigned)wave_blocks(GA.Nj, GA.Nk);
        hipLaunchKernelGGL(tri_fill_kernel, dim3(g), dim3(256), 0, s, pc->d_args, pc->d_y, n);
        hipLaunchKernelGGL((tri_grid_kernel<true>), dim3(nb), dim3(64), 0, s, pc->d_args, (const double*)nullptr, pc->d_y, VA, n);
        hipLaunchKernelGGL(tri_fill_kernel, dim3(g), dim3(256), 0, s, pc->d_args, (double*)nullptr, n);
        hipLaunchKernelGGL((tri_grid_kernel<false>), dim3(nb), dim3(64), 0, s, pc->d_args, (const double*)pc->d_y, (double*)nullptr, VB, n);
        break;
    }
    case IluForm::GridWave: {
        const GridView VA = grid_view(GA, true), VB = grid_view(GB, false);
        const unsigned nb = (unsigned)wave_blocks(GA.Nj, GA.Nk);
        const int budget = poll_budget();
        // (the abort word behind the 2 nb flags stays set once raised: later applies of a solve that has given up leave at their
        // first poll instead of burning the poll budget again; the host switches to the plane kernels at its next sync)
        hipLaunchKernelGGL((tri_wave_fill_kernel<true>), dim3(nb), dim3(256), 0, s, pc->d_args, pc->d_y, VA, pc->d_flags, (int32_t)(2 * nb));
        hipLaunchKernelGGL((tri_wave_kernel<true>), dim3(nb), dim3(192), 0, s, pc->d_args, (const double*)nullptr, pc->d_y, VA, n, pc->d_flags, pc->d_flags + 2 * nb, pc->d_gave_up, budget);
        hipLaunchKernelGGL((tri_wave_fill_kernel<false>), dim3(nb), dim3(256), 0, s, pc->d_args, (double*)nullptr, VB, (int32_t*)nullptr, 0);
        hipLaunchKernelGGL((tri_wave_kernel<false>), dim3(nb), dim3(192), 0, s, pc->d_args, (const double*)pc->d_y, (double*)nullptr, VB, n, pc->d_flags + nb, pc->d_flags + 2 * nb, pc->d_gave_up, budget);
        break;
    }
    case IluForm::GridQuad: {
        const unsigned nb = (unsigned)wave_blocks(GA.Nj, GA.Nk);
        const int budget = poll_budget();
        // 16 x 16 lines per workgroup (tri_quad.h): blocked coefficients, edge buffers between workgroups
        const unsigned nq = (unsigned)(GA.nbj * GA.nbk);
        const QuadView QA{GA.Ni, GA.Nj, GA.Nk, GA.nbj, GA.nbk, GA.nch, (const tw_v2*)GA.d_blocked, GA.d_edge_e, GA.d_edge_n, GA.d_skip};
        const QuadView QB{GB.Ni, GB.Nj, GB.Nk, GB.nbj, GB.nbk, GB.nch, (const tw_v2*)GB.d_blocked, GB.d_edge_e, GB.d_edge_n, GB.d_skip};
        // (no per-apply launch re-arms the edge buffers or the flags: tri_quad.h, poller / epoch)
        const TriDirect dir = direct ? *direct : TriDirect{nullptr, nullptr, nullptr, 0};
        hipLaunchKernelGGL((tri_quad_kernel<true>), dim3(nq), dim3(512), 0, s, pc->d_args, (const double*)nullptr, pc->d_y, QA, n, pc->d_flags, pc->d_flags + 2 * nb, pc->d_gave_up, budget, dir);
        hipLaunchKernelGGL((tri_quad_kernel<false>), dim3(nq), dim3(512), 0, s, pc->d_args, (const double*)pc->d_y, (double*)nullptr, QB, n, pc->d_flags + nb, pc->d_flags + 2 * nb, pc->d_gave_up, budget, dir);
        break;
    }
    case IluForm::GridPlanes: {
        const GridView VA = grid_view(GA, true), VB = grid_view(GB, false);
        // the wavefront kernel gave up once on this preconditioner (or the caller asks for it): one launch per hyperplane
        const int nlev = GA.Ni + GA.Nj + GA.Nk - 2;
        const unsigned pg = (unsigned)(((int64_t)GA.Nj * GA.Nk + 255) / 256);
        for (int lv = 0; lv < nlev; ++lv)
            hipLaunchKernelGGL((tri_plane_kernel<true>), dim3(pg), dim3(256), 0, s, pc->d_args, (const double*)nullptr, pc->d_y, VA, lv);
        for (int lv = 0; lv < nlev; ++lv)
            hipLaunchKernelGGL((tri_plane_kernel<false>), dim3(pg), dim3(256), 0, s, pc->d_args, (const double*)pc->d_y, (double*)nullptr, VB, lv);
        break;
    }
    case IluForm::BoxWave: {
        const BoxView WA = box_view(BA, n, true), WB = box_view(BB, n, false);
        const unsigned nb = (unsigned)(tb_nbj(BA.Nj) * tb_nbk(BA.Nk));
        const int budget = poll_budget();
        // pipelined wavefront over parallelograms of 8 x 8 lines (tri_box.h); the abort word behind the 2 nb flags stays set once raised
        hipLaunchKernelGGL((tri_box_fill_kernel<true>), dim3(nb), dim3(256), 0, s, pc->d_args, pc->d_y, WA, pc->d_flags, (int32_t)(2 * nb));
        const bool reg = BA.regular && BB.regular && env_int("KRYST_ILU_BOX_REGULAR", 1) != 0;
        // streams known at compile time: all 13 (27-point), a 19-point stencil's (lower 0x1eba / upper 0x0baf), Ilup(1)'s on a 7-point operator
        // (0x1cb0 / 0x01a7); any other set: run-time tests
        auto launch = [&](auto fwd, const BoxView& V, const double* in, double* out, int32_t* fl, uint32_t present) {
            constexpr bool F = decltype(fwd)::value;
            constexpr uint32_t FILL1 = F ? 0x1cb0u : 0x01a7u, P19 = F ? 0x1ebau : 0x0bafu;
            const size_t lds = tb_lds_bytes<F>();
#define KR_BOX_LAUNCH(R, M) hipLaunchKernelGGL((tri_box_kernel<F, R, M>), dim3(nb), dim3(256), lds, s, pc->d_args, in, out, V, fl, pc->d_flags + 2 * nb, pc->d_gave_up, budget, present)
            if (present == 0x1fffu) { if (reg) KR_BOX_LAUNCH(true, 0x1fffu); else KR_BOX_LAUNCH(false, 0x1fffu); }
            else if (present == FILL1) { if (reg) KR_BOX_LAUNCH(true, FILL1); else KR_BOX_LAUNCH(false, FILL1); }
            else if (present == P19) { if (reg) KR_BOX_LAUNCH(true, P19); else KR_BOX_LAUNCH(false, P19); }
            else { if (reg) KR_BOX_LAUNCH(true, 0u); else KR_BOX_LAUNCH(false, 0u); }
#undef KR_BOX_LAUNCH
        };
        launch(std::true_type(), WA, (const double*)nullptr, pc->d_y, pc->d_flags, BA.present);
        hipLaunchKernelGGL((tri_box_fill_kernel<false>), dim3(nb), dim3(256), 0, s, pc->d_args, (double*)nullptr, WB, (int32_t*)nullptr, 0);
        launch(std::false_type(), WB, (const double*)pc->d_y, (double*)nullptr, pc->d_flags + nb, BB.present);
        break;
    }
    case IluForm::BoxPlanes: {
        const BoxView WA = box_view(BA, n, true), WB = box_view(BB, n, false);
        const int nlev = (BA.Ni - 1) + 2 * (BA.Nj - 1) + 4 * (BA.Nk - 1) + 1;
        const unsigned pg = (unsigned)(((int64_t)BA.Nj * BA.Nk + 255) / 256);
        for (int lv = 0; lv < nlev; ++lv)
            hipLaunchKernelGGL((tri_box_plane_kernel<true>), dim3(pg), dim3(256), 0, s, pc->d_args, (const double*)nullptr, pc->d_y, WA, lv);
        for (int lv = 0; lv < nlev; ++lv)
            hipLaunchKernelGGL((tri_box_plane_kernel<false>), dim3(pg), dim3(256), 0, s, pc->d_args, (const double*)pc->d_y, (double*)nullptr, WB, lv);
        break;
    }
    }
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

int32_t IluPc::apply(int64_t, const double* r, double* z, const int* done) {
    if (n == 0) return KRYST_OK;
    const IluForm form = apply_form(this);
    if (form == IluForm::GridQuad && env_int("KRYST_ILU_GRAPH", 0) == 0 && env_int("KRYST_ILU_DIRECT_ARGS", 1) != 0) {
        // launched directly: the caller's vectors, the `done` flag and the apply's number travel as kernel arguments (tri_quad.h: TriDirect)
        direct_epoch = (direct_epoch & 0x3fffffff) + 1;
        const TriDirect dir{r, z, done, (int32_t)(0x40000000u | (uint32_t)direct_epoch)};
        return enqueue_apply(ctx->s_main, this, form, &dir);
    }
    hipLaunchKernelGGL(tri_set_args, dim3(1), dim3(1), 0, ctx->s_main, d_args, r, z, done);
    KR_HIP(hipGetLastError());
    const int use_graph = env_int("KRYST_ILU_GRAPH", few_launches(this, form) ? 0 : 1);        // (read per apply: tools/solver_ab.py)
    if (!exec && use_graph) {
        // capture the launch sequence once; the graph only refers to the device argument block
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(ctx->s_main, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int32_t rc = enqueue_apply(ctx->s_main, this, form);
            hipError_t e = hipStreamEndCapture(ctx->s_main, &g);
            if (rc == KRYST_OK && e == hipSuccess && g && hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess) {
                graph = g;
            } else {
                if (g) (void)hipGraphDestroy(g);
                exec = nullptr;
                (void)hipGetLastError();
            }
        }
    }
    if (exec && use_graph) { KR_HIP(hipGraphLaunch(exec, ctx->s_main)); return KRYST_OK; }
    return enqueue_apply(ctx->s_main, this, form);                    // eager fallback (same kernels)
}

// After a stream synchronisation: has the wavefront solve given up during an apply since the last check?  If so the
// preconditioner switches to the plane kernels for good (the captured graph is dropped) and the caller must repeat the work.
int32_t IluPc::health() {
    if (!h_gave_up || *(volatile int32_t*)h_gave_up == 0) return KRYST_OK;
    *(volatile int32_t*)h_gave_up = 0;
    safe = true; switched = true;
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    set_error("ILU apply: the wavefront triangular solve gave up waiting for a neighbour block (workgroups not dispatched in index "
              "order?); its result was discarded and this preconditioner now uses the level-per-launch plane kernels");
    return KRYST_SOLVE_ERROR;
}
bool IluPc::fell_back() {
    if (!switched) return false;
    switched = false;
    return true;
}
bool IluPc::check_after_apply() const { return grid() ? !safe : apply_form(this) == IluForm::BoxWave; }

IluPc::~IluPc() {
    if (h_gave_up) (void)hipHostFree(h_gave_up);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    L.free_all(); U.free_all(); GL.free_all(); GU.free_all(); BL.free_all(); BU.free_all();
    for (void* q : {(void*)d_args, (void*)d_flags, (void*)d_y, (void*)d_rL, (void*)d_yU, (void*)d_zU, (void*)d_mapLU}) (void)pool_free(q);
}

// How a level-ordered factor of n rows is solved, for both set-ups (host rows: build_factor; device: general_setup_on_device).
void choose_level_form(TriFactor* F, int64_t n, int64_t levels, int64_t longest_row, int64_t rows_longer_than_8, int64_t entries) {
    F->ell = longest_row <= ELLW && n > 0;
    F->held = longest_row <= 8 ? 8 : 16;
    // one sync-free launch per factor, except for CSR factors whose levels are narrow (a deep graph of a few hundred rows per level:
    // the one-workgroup run kernel's workgroup barrier, 3.4 us per level, beats two uncached round trips, 5.9 us -- measured on a
    // random band matrix with 10 716 levels of 187 rows: 127 -> 72 ms; a 27-point factor with 1 328 rows per level: 9.9 ms sync-free,
    // 13.0 ms otherwise).  KRYST_ILU_SYNCFREE = 0 / 1 forces either form.
    const double rows_per_level = levels > 0 ? (double)n / (double)levels : 0.0;
    // (round 4: an ELL factor with FEWER than 256 rows per level takes the one-workgroup barrier-free run kernel as well -- 0.45-1.4 us per level
    // there against the sync-free kernel's two fabric trips, 2 us, whatever the width)
    F->syncfree = env_int("KRYST_ILU_SYNCFREE", ((F->ell && (rows_per_level >= 256.0 || env_int("KRYST_ILU_RUN_FREE", 1) == 0)) || rows_per_level >= 512.0) ? 1 : 0) != 0;
    F->last_entry = (int32_t)entries - 1;
    F->free_runs = !F->syncfree && entries > 0 && grant_free_runs(n > 0 ? (double)rows_longer_than_8 / (double)n : 0.0);
}

// the wavefront solves' shared state: 2 nb + 1 zeroed flags ("this block is under way" per block and direction, the abort word behind them)
// and the mapped give-up word
static int32_t alloc_wave_state(IluPc* pc, size_t nb) {
    if (pool_malloc(&pc->d_flags, sizeof(int32_t) * (2 * nb + 1)) != hipSuccess || zero_dev(pc->d_flags, sizeof(int32_t) * (2 * nb + 1), pc->ctx->s_main) != KRYST_OK) { set_error("hipMalloc failed"); return KRYST_ERR_HIP; }
    if (hipHostMalloc((void**)&pc->h_gave_up, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&pc->d_gave_up, pc->h_gave_up, 0) != hipSuccess) { set_error("hipHostMalloc failed"); return KRYST_ERR_HIP; }
    *pc->h_gave_up = 0;
    return KRYST_OK;
}

// device buffers every ILU-family preconditioner needs once its factors are on the device (grid form, box form or level-ordered form)
int32_t finish_ilu_device(IluPc* D) {
    kryst_ctx_t ctx = D->ctx;
    const int64_t n = D->n;
    int32_t rc = KRYST_OK;
    if (pool_malloc(&D->d_args, sizeof(TriArgs)) != hipSuccess || zero_dev(D->d_args, sizeof(TriArgs), ctx->s_main) != KRYST_OK) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
    if (rc == KRYST_OK) {
        const size_t bytes = sizeof(double) * (size_t)((n + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE);
        const bool in_place = D->grid() || D->box();   // the wavefront / box solves work in place: one intermediate vector
        for (double** pp : {&D->d_y, &D->d_rL, &D->d_yU, &D->d_zU}) {
            if (rc != KRYST_OK) break;
            if (in_place && pp != &D->d_y) continue;
            if (pool_malloc(pp, bytes) != hipSuccess) { set_error("hipMalloc failed"); rc = KRYST_ERR_HIP; }
            else if (hipMemsetAsync(*pp, 0, bytes, ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
        }
        if (rc == KRYST_OK && hipStreamSynchronize(ctx->s_main) != hipSuccess) rc = KRYST_ERR_HIP;
    }
    if (rc == KRYST_OK && D->box() && D->BL.Ni >= 2) {
        const size_t nb = (size_t)tb_nbj(D->BL.Nj) * (size_t)tb_nbk(D->BL.Nk);
        rc = alloc_wave_state(D, nb);
        if (rc == KRYST_OK && ilu_box_knob() >= 2) {
            // blocked copies of both factors for the wavefront kernels' loaders, one device pass each
            const size_t nch = (size_t)(D->BL.Ni + 29 + TB_C - 1) / TB_C;
            const size_t el = (size_t)(TB_C / 2) * 64 * 16;
            const BoxView VA{D->BL.Ni, D->BL.Nj, D->BL.Nk, n, D->BL.d_c, nullptr, box_stream_stride(n), nullptr};
            const BoxView VB{D->BU.Ni, D->BU.Nj, D->BU.Nk, n, D->BU.d_c, D->BU.d_diag, box_stream_stride(n), nullptr};
            if (pool_malloc(&D->BL.d_cb, nb * nch * 13 * el) != hipSuccess || pool_malloc(&D->BU.d_cb, nb * nch * 14 * el) != hipSuccess) {
                (void)hipGetLastError(); (void)pool_free(D->BL.d_cb); (void)pool_free(D->BU.d_cb); D->BL.d_cb = D->BU.d_cb = nullptr;     // (no room: the hyperplane kernels)
            } else {
                hipLaunchKernelGGL((tri_box_layout_kernel<true>), dim3((unsigned)(nb * nch)), dim3(256), 0, ctx->s_main, VA, (tw_v2*)D->BL.d_cb);
                hipLaunchKernelGGL((tri_box_layout_kernel<false>), dim3((unsigned)(nb * nch)), dim3(256), 0, ctx->s_main, VB, (tw_v2*)D->BU.d_cb);
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("box layout kernel failed"); rc = KRYST_ERR_HIP; }
            }
        }
        if (rc == KRYST_OK) {
            // 70 / 73 KiB of LDS per workgroup (two per CU): more than the 64 KiB a kernel gets without asking
            bool ok = true;
#define KR_BOX_ATTR(F, R, M) ok = ok && hipFuncSetAttribute((const void*)tri_box_kernel<F, R, M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tb_lds_bytes<F>()) == hipSuccess
            KR_BOX_ATTR(true, true, 0x1ebau); KR_BOX_ATTR(true, false, 0x1ebau); KR_BOX_ATTR(false, true, 0x0bafu); KR_BOX_ATTR(false, false, 0x0bafu);
            KR_BOX_ATTR(true, true, 0x1fffu); KR_BOX_ATTR(true, true, 0x1cb0u); KR_BOX_ATTR(true, true, 0u); KR_BOX_ATTR(true, false, 0x1fffu); KR_BOX_ATTR(true, false, 0x1cb0u); KR_BOX_ATTR(true, false, 0u);
            KR_BOX_ATTR(false, true, 0x1fffu); KR_BOX_ATTR(false, true, 0x01a7u); KR_BOX_ATTR(false, true, 0u); KR_BOX_ATTR(false, false, 0x1fffu); KR_BOX_ATTR(false, false, 0x01a7u); KR_BOX_ATTR(false, false, 0u);
#undef KR_BOX_ATTR
            D->box_wave_ready = ok && D->BL.d_cb && D->BU.d_cb;
            (void)hipGetLastError();
        }
    }
    if (rc == KRYST_OK && D->grid()) {
        rc = alloc_wave_state(D, (size_t)wave_blocks(D->GL.Nj, D->GL.Nk));
        if (rc == KRYST_OK && D->GL.Ni >= 2 && ilu_wave_knob(D->GL) >= 2) {
            // blocked coefficient layout + edge buffers of the 16 x 16 kernel (tri_quad.h), one device pass per factor
            for (GridFactor* G : {&D->GL, &D->GU}) {
                if (rc != KRYST_OK) break;
                const bool fwd = G == &D->GL;
                G->nbj = (G->Nj + 15) / 16; G->nbk = (G->Nk + 15) / 16; G->nch = (G->Ni + 14 + TQ_C - 1) / TQ_C;
                const size_t nq = (size_t)G->nbj * G->nbk;
                const int NA = fwd ? 3 : 4;
                const size_t cbytes = nq * G->nch * NA * 4 * TQ_LINES * sizeof(tw_v2);
                const size_t ebytes = nq * (size_t)(G->nch * TQ_C + 8) * 16 * sizeof(double);
                if (pool_malloc(&G->d_blocked, cbytes) != hipSuccess || pool_malloc(&G->d_edge_e, ebytes) != hipSuccess ||
                    pool_malloc(&G->d_edge_n, ebytes) != hipSuccess) {
                    // no room for the blocked copy (it doubles the factor's footprint): the 8 x 8 kernel works on the natural-order streams
                    (void)hipGetLastError();
                    for (GridFactor* H : {&D->GL, &D->GU}) {
                        (void)pool_free(H->d_blocked); (void)pool_free(H->d_edge_e); (void)pool_free(H->d_edge_n); (void)pool_free(H->d_skip);
                        H->d_blocked = nullptr; H->d_edge_e = H->d_edge_n = nullptr; H->d_skip = nullptr;
                    }
                    break;
                }
                const GridView V{G->Ni, G->Nj, G->Nk, G->d_c1, G->d_c2, G->d_c3, G->d_diag};
                const unsigned lg = (unsigned)(nq * G->nch);
                if (fwd) hipLaunchKernelGGL((tri_quad_layout_kernel<true, 3>), dim3(lg), dim3(256), 0, ctx->s_main, V, G->nbj, G->nbk, G->nch, (tw_v2*)G->d_blocked);
                else hipLaunchKernelGGL((tri_quad_layout_kernel<false, 4>), dim3(lg), dim3(256), 0, ctx->s_main, V, G->nbj, G->nbk, G->nch, (tw_v2*)G->d_blocked);
                // edge buffers armed once (sentinels; zeros past the last step): between applies the pollers re-arm what they consume
                hipLaunchKernelGGL(tri_quad_fill_kernel, dim3(std::min<unsigned>(1024u, (unsigned)nq * 4u)), dim3(256), 0, ctx->s_main, G->d_edge_e, G->d_edge_n, (int)nq, G->nch, (int32_t*)nullptr, 0);
                // which chunks repeat chunk - 3 bit for bit (their coefficients are in the solving wave's registers already)
                if (env_int("KRYST_ILU_DEDUP", 1) && G->nch + 3 <= TQ_SKIPMAX) {
                    if (pool_malloc(&G->d_skip, nq * 4 * (size_t)G->nch) != hipSuccess) { (void)hipGetLastError(); G->d_skip = nullptr; }      // (flags are optional)
                    else if (fwd) hipLaunchKernelGGL((tri_quad_dedup_kernel<3>), dim3(lg), dim3(256), 0, ctx->s_main, (const tw_v2*)G->d_blocked, G->nch, G->d_skip);
                    else hipLaunchKernelGGL((tri_quad_dedup_kernel<4>), dim3(lg), dim3(256), 0, ctx->s_main, (const tw_v2*)G->d_blocked, G->nch, G->d_skip);
                }
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) { set_error("blocked layout kernel failed"); rc = KRYST_ERR_HIP; }
                if (rc == KRYST_OK && G->d_skip && getenv("KRYST_ILU_VERBOSE")) {
                    std::vector<uint8_t> h(nq * 4 * (size_t)G->nch);
                    if (hipMemcpyAsync(h.data(), G->d_skip, h.size(), hipMemcpyDeviceToHost, ctx->s_main) == hipSuccess && hipStreamSynchronize(ctx->s_main) == hipSuccess) { G->nskip = 0; for (uint8_t v : h) G->nskip += v; }
                    fprintf(stderr, "[kryst ilu] %s factor: %lld of %zu coefficient chunks repeat (no request)\n", fwd ? "forward" : "backward", (long long)G->nskip, h.size());
                }
            }
        }
    }
    if (getenv("KRYST_ILU_VERBOSE")) {
        if (D->BL.ok) { fprintf(stderr, "[kryst ilu] box streams: L present %#x regular %d, U present %#x regular %d\n", D->BL.present, (int)D->BL.regular, D->BU.present, (int)D->BU.regular); }
        const IluForm f = laid_out_form(D);
        fprintf(stderr, "[kryst ilu] n=%lld %s; levels L/U=%zu/%zu\n", (long long)n, f == IluForm::Level ? "level-ordered" : (f == IluForm::BoxWave || f == IluForm::BoxPlanes) ? "box stencil (13 streams per factor)" : "structured grid (wavefront kernel)",
                D->L.lvl_off.empty() ? (size_t)0 : D->L.lvl_off.size() - 1, D->U.lvl_off.empty() ? (size_t)0 : D->U.lvl_off.size() - 1);
    }
    return rc;
}

}  // namespace kr

using namespace kr;

// What an ILU-family preconditioner's apply runs and streams (bench.py prices the triangular solve with it):
//   info[0] form: 0 level-ordered factors (sync-free / level kernels), 1 structured grid, 8 x 8 lines per workgroup, 2 structured
//           grid, 16 x 16 lines per workgroup (tri_quad.h), 3 structured grid after a give-up (plane kernels), 4 box stencil inside the
//           3 x 3 x 3 cube, one launch per hyperplane i + 2 j + 4 k (info[4], info[5]: hyperplanes per factor), 5 box stencil, pipelined
//           wavefront over parallelograms of 8 x 8 lines (tri_box.h); form_info says which state each of them reflects
//   info[1..3] Ni, Nj, Nk (grid forms)          info[4], info[5] dependency levels of L, U (level-ordered forms)
//   box forms (4, 5): info[6], info[7] coefficient streams L / U have (of 13), info[8] 1 when both factors are "regular" (tri_box.h)
//   info[6], info[7] coefficient chunks (per block quadrant) of the forward / backward factor; info[8], info[9] how many of them
//           repeat chunk - 3 bit for bit and are not requested; info[10], info[11] bytes per chunk request (forward, backward)
//   info[12] stored entries of L + U (level-ordered forms)
extern "C" int32_t kryst_pc_ilu_info(kryst_pc_t pc, int64_t* info, int32_t count) {
    KR_ARG(pc && info && count >= 13, "pc_ilu_info: need room for 13 values");
    IluPc* D = pc_cast<IluPc>(pc);
    KR_ARG(D, "pc_ilu_info: not an ILU-family preconditioner");
    kryst_ctx_t ctx = pc->ctx;
    for (int i = 0; i < count; ++i) info[i] = 0;
    info[0] = form_info(D);
    if (D->box()) {
        info[1] = D->BL.Ni; info[2] = D->BL.Nj; info[3] = D->BL.Nk;
        info[4] = info[5] = (D->BL.Ni - 1) + 2 * (D->BL.Nj - 1) + 4 * (D->BL.Nk - 1) + 1;
        info[6] = __builtin_popcount(D->BL.present); info[7] = __builtin_popcount(D->BU.present);   // coefficient streams the factors have (of 13 each)
        info[8] = (D->BL.regular && D->BU.regular) ? 1 : 0;                                          // tri_box.h: REGULAR
        return KRYST_OK;
    }
    if (!D->grid()) {
        info[4] = D->L.lvl_off.empty() ? 0 : (int64_t)D->L.lvl_off.size() - 1;
        info[5] = D->U.lvl_off.empty() ? 0 : (int64_t)D->U.lvl_off.size() - 1;
        return KRYST_OK;
    }
    info[1] = D->GL.Ni; info[2] = D->GL.Nj; info[3] = D->GL.Nk;
    if (quad_laid_out(D)) {                                                // (the blocked copy's figures, after a give-up too)
        KR_HIP(hipSetDevice(ctx->device));
        int q = 0;
        for (GridFactor* G : {&D->GL, &D->GU}) {
            const size_t cnt = (size_t)G->nbj * G->nbk * 4 * (size_t)G->nch;
            info[6 + q] = (int64_t)cnt;
            info[10 + q] = (int64_t)((q == 0 ? 3 : 4) * 4 * 64 * sizeof(tw_v2));
            if (G->d_skip && cnt) {
                std::vector<uint8_t> h(cnt);
                KR_HIP(hipMemcpyAsync(h.data(), G->d_skip, cnt, hipMemcpyDeviceToHost, ctx->s_main));
                KR_HIP(hipStreamSynchronize(ctx->s_main));
                int64_t ns = 0;
                for (uint8_t v : h) ns += v;
                info[8 + q] = ns;
            }
            ++q;
        }
    }
    return KRYST_OK;
}

#ifdef KR_TW_TRACE
extern "C" int32_t kryst_debug_tq_trace(long long* host, int32_t count) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(kr::tq_trace), sizeof(long long) * count) == hipSuccess ? 0 : 1;
}
extern "C" int32_t kryst_debug_tq_select(int32_t a, int32_t b) {
    const int v[2] = {a, b};
    return hipMemcpyToSymbol(HIP_SYMBOL(kr::tq_sel), v, sizeof(v)) == hipSuccess ? 0 : 1;
}
extern "C" int32_t kryst_debug_tq_steps(long long* host) {          // 3 x 1024: solver steps, poller deliveries, exporter stores
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(kr::tq_steps), sizeof(long long) * 1024) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(host + 1024, HIP_SYMBOL(kr::tq_deliv), sizeof(long long) * 1024) != hipSuccess) return 1;
    return hipMemcpyFromSymbol(host + 2048, HIP_SYMBOL(kr::tq_export), sizeof(long long) * 1024) == hipSuccess ? 0 : 1;
}
extern "C" int32_t kryst_debug_tw_trace(long long* host, int32_t count) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(kr::tw_trace), sizeof(long long) * count) == hipSuccess ? 0 : 1;
}
extern "C" int32_t kryst_debug_tw_steps(long long* host, int32_t count) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(kr::tw_steps), sizeof(long long) * count) == hipSuccess ? 0 : 1;
}
extern "C" int32_t kryst_debug_tw_rounds(long long* host, int32_t count) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(kr::tw_rounds), sizeof(long long) * count) == hipSuccess ? 0 : 1;
}
#endif
