// Mixed precision: fp32 as a STORAGE format.  Vectors and matrix values are kept as floats; every kernel widens what
// it loads, computes in fp64 in the fixed order of its fp64 twin and rounds once -- (float), round to nearest even -- when it stores.  Scalars,
// inner products, DevState and the logic structs of cg_logic.h stay fp64 and are the fp64 solvers' own code.
#pragma once
#include "csr.h"

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

// y <- (float)(A x) on ctx->s_main; nq = 1: also the tile partials of sum_i d[i] * y[i] (y as stored) in the fp32 tree into partial array 0.
// `done` (device flag) makes the launch a no-op when set.
int32_t launch_spmv32(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
// the kernel that launch takes under the current settings (KRYST_SPMV32_FORM, KRYST_SPMV32_STAGE): 0 spmv32_wave_kernel on the plain arrays,
// 1 spmv32_pattern_kernel, 2 spmv32_pattern_stage_kernel, 3 spmv32_dia_kernel.  The ONE place that decides; kryst_csr32_encoding reports it.
int spmv32_kernel(kryst_csr32_t a);
// mixed_pattern.hip: the two kernels of the row-pattern form
int32_t enqueue_spmv32_pattern(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
int32_t enqueue_spmv32_pattern_stage(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
// mixed_dia.hip: the kernel of the diagonal form, and the conversion of the fp64 streams (*refused: stored NaNs whose rounding has the marker's bits)
int32_t enqueue_spmv32_dia(kryst_csr32_t a, const float* x, float* y, int nq, const float* dvec, const int* done);
hipError_t enqueue_lower_dia(kryst_csr_t a, kryst_csr32_t m, unsigned long long* d_refused);

#ifdef __HIPCC__
// ---- what the kernels of mixed_pattern.hip and mixed_dia.hip share: thread t of a tile owns rows 4t .. 4t+3 ----
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
#endif

}  // namespace kr
