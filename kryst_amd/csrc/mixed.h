// Mixed precision (with the map of the family's units): the two handles and what crosses the units.
// The arithmetic contract -- a LABELLED DEVIATION from the reference's CgSolver<f32>, which would round every operation: fp32 is how numbers are
// STORED.  A kernel widens what it loads (exact), computes in fp64 in the fixed order of its fp64 twin with separate multiply and add, and rounds
// once, (float) = round to nearest even with fp32 subnormals kept, when it stores.  An inner-product term (double)a * (double)b is exact; the fold
// is the published tree at T = 256, V = 4 (kryst_reduce_spec32): the thread's 4 terms in index order from 0.0, the 64-lane xor butterfly, the 4
// waves serially -> one partial per 1024-element tile, then fold2, DevState and the logic structs of cg_logic.h, the fp64 solvers' own code.
#pragma once
#include "csr.h"
#include <cfloat>

// ---- the fp32 inner-product tree (kryst_reduce_spec32): a tile is 256 threads x 4 consecutive elements, one 16-byte access per array and lane ----
#define KR32_T 256
#define KR32_V 4
#define KR32_TILE (KR32_T * KR32_V)

struct kryst_vec32_s {
    kryst_ctx_t ctx = nullptr;
    int64_t n = 0;
    float* d = nullptr;             // ceil(n / 1024) * 1024 + 1024 floats, zero at creation (kryst_vec_t's rule at the fp32 tile size)
};

// the lowered operator: copies of the fp64 operator's index arrays and its values rounded to fp32 -- no lifetime tie to the operator it came from
struct kryst_csr32_s {
    kryst_ctx_t ctx = nullptr;
    int64_t nrows = 0, ncols = 0, nnz = 0;
    int32_t* d_row_ptr = nullptr;   // nrows + 1
    int32_t* d_col = nullptr;       // nnz + 8, zeroed tail
    float* d_val = nullptr;         // nnz + 8, zeroed tail
    int64_t changed = 0, tiny = 0;  // values the rounding changed / nonzero values that became zero or fp32-subnormal
    // the row-pattern form (CSR-P16 with fp32 tables; kryst_csr32_lower_form PATTERN, or AUTO where the operator has one): the operator's own copies
    uint16_t* d_pid = nullptr;      // ntiles32 * 1024 + 1024 ids, zeroed tail (a lane reads its four ids with one 8-byte load), or nullptr
    uint32_t* d_pmeta = nullptr;    // 2 words per pattern, as kryst_csr_s::d_pmeta
    int32_t* d_poff = nullptr;      // table: col - row
    float* d_pval = nullptr;        // table: (float)value -- bit for bit the rounded CSR value of every row that uses the entry
    int32_t npat = 0, ntab = 0, pat_unroll = 8; bool pat_single = false;
    int32_t pat_stage_n = 0, pat_far_lo = 0, pat_far_hi = 0; bool pat_far_uniform = false;
    // the diagonal form (CSR-DIA with fp32 streams; kryst_csr32_lower_form DIA only): the operator's own copy
    float* d_dia = nullptr;         // dia_nd streams of dia_stride floats, d_dia[d * dia_stride + row]: (float) of the fp64 stream entry, or the marker
    int64_t dia_stride = 0;         // ntiles32 * 1024 + 1024: a lane's 16-byte value load is aligned and in bounds in every tile; padding = marker
    int32_t dia_nd = 0, dia_min = 0, dia_max = 0;
    int32_t dia_off[kr::KR_DIA_MAX] = {0};      // col - row of diagonal d, in the rows' stored order (kryst_csr_s::dia_off)
};

namespace kr {

inline int64_t ntiles32_of(int64_t n) { return (n + KR32_TILE - 1) / KR32_TILE; }
inline int64_t vec32_len(int64_t n) { return ntiles32_of(n) * KR32_TILE + KR32_TILE; }      // allocated floats
inline int64_t ws_len32(int64_t n) { return vec32_len(n) / 2 - KR_TILE; }                   // the Workspace length whose vectors are one fp32 vector each
static inline unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }   // 256-thread grid-stride passes (static: multi.hip has its own, with another cap)

// ---- mixed_vec.hip: the vector handle and the conversions
int32_t vec32_check(kryst_vec32_t v);
int32_t vec32_alloc(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out);
void vec32_free(kryst_vec32_t v);
// dst[i] = (float)src[i], or (float)(src[i] / den) when `divide` is set (refinement: r32 = (float)(r / rho)); n > 0
hipError_t enqueue_round32(kryst_ctx_t ctx, float* dst, const double* src, int64_t n, int divide, double den);

// ---- mixed_lower.hip: the lowered operator.  Each form lowers itself beside its kernels: *_refusal says why the operator cannot take the form (nullptr: it
// can; asked before anything is allocated), enqueue_lower_* allocates the form's arrays on m (csr32_free releases them), copies, rounds and sets the fields
int32_t csr32_check(kryst_csr32_t a);
inline bool offsets_fit32(kryst_csr_t a) { return vec32_len(std::max(a->nrows, a->ncols)) * (int64_t)sizeof(float) < (1ll << 31); }   // the form kernels address x and y with 32-bit byte offsets
const char* lower_pattern_refusal(kryst_csr_t a);
hipError_t enqueue_lower_pattern(kryst_csr_t a, kryst_csr32_t m);
const char* lower_dia_refusal(kryst_csr_t a);
hipError_t enqueue_lower_dia(kryst_csr_t a, kryst_csr32_t m, unsigned long long* d_refused);   // *d_refused: stored NaNs whose rounding has the marker's bits

// ---- mixed_spmv.hip: y <- (float)(A x) on ctx->s_main; nq = 1: also the tile partials of sum_i d[i] * y[i] (y as stored) in the fp32 tree into
// partial array 0.  `done` (device flag) makes the launch a no-op when set.
int32_t launch_spmv32(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
// the kernel that launch takes under the current settings (KRYST_SPMV32_FORM, KRYST_SPMV32_STAGE): the ONE place that decides; kryst_csr32_encoding reports the value
enum class Spmv32Kernel : int32_t { Plain = 0, Pattern = 1, PatternStage = 2, Dia = 3 };     // spmv32_wave_ / _pattern_ / _pattern_stage_ / _dia_kernel
Spmv32Kernel spmv32_kernel(kryst_csr32_t a);
int32_t enqueue_spmv32_pattern(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);          // mixed_pattern.hip
int32_t enqueue_spmv32_pattern_stage(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
int32_t enqueue_spmv32_dia(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);              // mixed_dia.hip

// ---- mixed_cg.hip: CG (pcg = false) / PCG with Identity or Jacobi on fp32 storage; refinement is the second caller
struct Solve32IO { kryst_pc_t pc; const kryst_params_t* params; kryst_stats_t* stats; double* hist; int64_t hist_cap; int64_t* hist_len; };
int32_t solve32_check(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg);     // what is refused before anything is launched or written
int32_t solve32(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, const Solve32IO& io, bool pcg);
int32_t launch_dot32(kryst_ctx_t ctx, const float* a, const float* b, int64_t n);               // the tile partials of (a, b) into partial array 0

// the verdict of one rounding, shared by the device pass (lower_values_kernel) and its host twin (kryst_host_round_f32)
__host__ __device__ __forceinline__ float round_count(double v, unsigned long long (&cnt)[3]) {
    const float f = (float)v;
    const float af = f < 0.0f ? -f : f;
    if (v == v) {                                                     // (a NaN stays a NaN and counts as nothing)
        if ((double)f != v) ++cnt[0];                                 // changed by the rounding
        if (v != 0.0 && af < FLT_MIN) ++cnt[1];                       // became zero or fp32-subnormal
        const double av = v < 0.0 ? -v : v;
        if (av <= DBL_MAX && af > FLT_MAX) ++cnt[2];                  // a finite value that rounds to +-inf
    }
    return f;
}

#ifdef __HIPCC__
// ---- what the SpMV kernels share: thread t of a tile owns rows 4t .. 4t+3 ----
typedef float p_v4f __attribute__((ext_vector_type(4)));
typedef float p_v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte access at 4-byte alignment (gathers at any column)

// the lane's four terms in index order from 0.0 (rows at or beyond nrows contribute nothing)
__device__ __forceinline__ double quad_dot(const p_v4f d, const float (&o)[4], const bool (&valid)[4]) {
    double acc = 0.0;
    if (valid[0]) acc = acc + (double)d.x * (double)o[0];
    if (valid[1]) acc = acc + (double)d.y * (double)o[1];
    if (valid[2]) acc = acc + (double)d.z * (double)o[2];
    if (valid[3]) acc = acc + (double)d.w * (double)o[3];
    return acc;
}
__device__ __forceinline__ void quad_store(float* y, int32_t row, int32_t nrows, const float (&o)[4]) {
    if (row + 3 < nrows) {
        p_v4f ov; ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
        *reinterpret_cast<p_v4f*>(y + row) = ov;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) { if (row + r < nrows) y[row + r] = o[r]; }
    }
}
// the end of tile q in the kernels that finish one tile at a time: y = (float)s, one 16-byte store; under NQ the tile partial of (d, y) with y as
// stored -- the lane's four products, the butterfly, the 4 waves (red: KR32_T / 64 doubles of LDS).  Called by all threads of the workgroup.
template <int NQ>
__device__ __forceinline__ void quad_finish(const double (&s)[4], float* y, const float* dvec, double* partials, int32_t q, int32_t row, int32_t nrows, double* red) {
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (float)s[r];
    quad_store(y, row, nrows, o);
    if constexpr (NQ > 0) {
        const p_v4f dd = *reinterpret_cast<const p_v4f*>(dvec + row);       // (rows behind n lie in the padding: read, never used)
        const bool valid[4] = {row < nrows, row + 1 < nrows, row + 2 < nrows, row + 3 < nrows};
        double acc[1] = {quad_dot(dd, o, valid)};
        block_reduce<1, KR32_T / 64>(acc, red);
        if (threadIdx.x == 0) partials[q] = acc[0];
    }
}
#endif

}  // namespace kr
