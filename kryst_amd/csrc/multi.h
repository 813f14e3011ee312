// Multivectors (n x K, K in {2, 4, 8}) for several right-hand sides at once: storage and the SpMM launcher.
//
// Element (i, j) lives at i*K + j: the K values of a row are contiguous, so a gather of x-row c is one aligned run of 8 K bytes and the
// two rows a lane owns (ew.h: thread t of a tile owns rows 2t, 2t+1) are 2 K contiguous doubles.  The allocation holds
// ceil(n / 512) * 512 + 512 rows, zero at creation -- kryst_vec_t's padding rule, per column.
#pragma once
#include "csr.h"
#include "ew.h"

struct kryst_mvec_s {
    kryst_ctx_t ctx = nullptr;
    int64_t n = 0;
    int32_t k = 0;
    double* d = nullptr;
};

namespace kr {

inline int64_t mvec_rows(int64_t n) { return (n + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE; }      // allocated rows
inline bool mvec_width_ok(int k) { return k == 2 || k == 4 || k == 8; }

// Y <- A X on ctx->s_main over interleaved n x k arrays, from the operator's CSR-DIA streams or its plain CSR arrays (spmm_takes_dia decides).
// nq = 1: also the tile partials of sum_i D(i, j) * Y(i, j) for every column j into partials[j * pstride + tile].  nq = 2: also the tile partials
// of the upper triangle of Gram(X, Y), K (K + 1) / 2 arrays, entry e into partials[e * pstride + tile] (spmm_gram_epilogue; square operators).  `done` (device flag) makes the
// launch a no-op when set.
int32_t launch_spmm(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done);
// The choice (multi.hip), from the forms the operator has and KRYST_SPMM_FORM = auto | plain | dia, read at every launch: does launch_spmm take
// spmm_dia_kernel for k columns?
bool spmm_takes_dia(kryst_csr_t a, int k);
// multi_dia.hip: the same launch through spmm_dia_kernel, for an operator that holds the streams
int32_t launch_spmm_dia(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done);


int32_t mvec_check(kryst_mvec_t mv);                   // a live handle, else KRYST_ERR_ARG
// the arguments of a solve on multivectors (kryst_cg / pcg / bcg_solve_multi_dev)
struct MultiIO {
    kryst_mvec_t b, x; kryst_csr_t a; kryst_pc_t pc; const kryst_params_t* params;
    kryst_stats_t* stats; int32_t* status; double* hist; int64_t hist_cap; int64_t* hist_len;
};
// what such a solve refuses before anything is launched or written; `pcg`: the solve reads pc (Identity or Jacobi only)
int32_t multi_args_check(const MultiIO& io, bool pcg);

#ifdef __HIPCC__
// A lane's two rows are 2 K contiguous doubles; element e of them belongs to column e % K and to the lane's row e / K.
template <int K> __device__ __forceinline__ void ld_rows(const double* p, int64_t row, double (&v)[2 * K]) {
    const kr_v2d* q = reinterpret_cast<const kr_v2d*>(p + row * K);
#pragma unroll
    for (int h = 0; h < K; ++h) { const kr_v2d t = q[h]; v[2 * h] = t.x; v[2 * h + 1] = t.y; }
}
template <int K> __device__ __forceinline__ void st_rows(double* p, int64_t row, const double (&v)[2 * K]) {
    kr_v2d* q = reinterpret_cast<kr_v2d*>(p + row * K);
#pragma unroll
    for (int h = 0; h < K; ++h) { kr_v2d t; t.x = v[2 * h]; t.y = v[2 * h + 1]; q[h] = t; }
}

template <int K> struct BcgShape { static constexpr int NG = K * (K + 1) / 2; static constexpr int RG = K == 8 ? 6 : NG; };      // entries of the upper triangle, row by row

// one row of K contiguous doubles
template <int K> __device__ __forceinline__ void ld_row(const double* p, int64_t row, double (&v)[K]) {
    const kr_v2d* q = reinterpret_cast<const kr_v2d*>(p + row * K);
#pragma unroll
    for (int h = 0; h < K / 2; ++h) { const kr_v2d t = q[h]; v[2 * h] = t.x; v[2 * h + 1] = t.y; }
}
template <int K> __device__ __forceinline__ void st_row(double* p, int64_t row, const double (&v)[K]) {
    kr_v2d* q = reinterpret_cast<kr_v2d*>(p + row * K);
#pragma unroll
    for (int h = 0; h < K / 2; ++h) { kr_v2d t; t.x = v[2 * h]; t.y = v[2 * h + 1]; q[h] = t; }
}
// acc[(a, b)] += u[a] * w[b] over the upper triangle, row by row
template <int K> __device__ __forceinline__ void gram_add(const double (&u)[K], const double (&w)[K], double (&acc)[BcgShape<K>::NG]) {
    int e = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
#pragma unroll
        for (int b = a; b < K; ++b) { acc[e] = acc[e] + u[a] * w[b]; ++e; }
    }
}
// The tile partial of every entry: block_reduce per entry, in groups of BcgShape<K>::RG entries so that a group's butterflies, not all NG of them,
// are in flight at once (the values per entry are those of one block_reduce<NG> over all of them; lds holds RG * 4 doubles)
template <int K, int E0 = 0>
__device__ __forceinline__ void gram_store(double (&acc)[BcgShape<K>::NG], double* lds, double* partials, int64_t pstride, int64_t tile) {
    constexpr int NG = BcgShape<K>::NG, RG = BcgShape<K>::RG;
    double v[RG];
#pragma unroll
    for (int e = 0; e < RG; ++e) v[e] = acc[E0 + e];
    block_reduce<RG, KR_T / 64>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < RG; ++e) partials[(E0 + e) * pstride + tile] = v[e];
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (E0 + RG < NG) gram_store<K, E0 + RG>(acc, lds, partials, pstride, tile);
}

// Gram(X, Y) in an SpMM's epilogue (nq = 2; block CG, block_cg.hip): the tile partials of the upper triangle, entry (a, b) the inner product over
// X(i, a) * Y(i, b).  The owner lane holds its two Y rows (s0, s1) and loads its own two X rows; the lane's two rows in index order from 0.0, then
// gram_store -- the values of mgram_kernel on the stored Y, entry by entry.  X must have the operator's row count (a square operator).
template <int K>
__device__ __forceinline__ void spmm_gram_epilogue(const double* x, int64_t row, bool in0, bool in1, const double (&s0)[K], const double (&s1)[K],
                                                   double* lds, double* partials, int64_t pstride, int64_t tile) {
    double acc[BcgShape<K>::NG];
#pragma unroll
    for (int e = 0; e < BcgShape<K>::NG; ++e) acc[e] = 0.0;
    double xr[K];
    ld_row<K>(x, row, xr);
    if (in0) gram_add<K>(xr, s0, acc);
    ld_row<K>(x, row + 1, xr);
    if (in1) gram_add<K>(xr, s1, acc);
    gram_store<K>(acc, lds, partials, pstride, tile);
}
#endif

}  // namespace kr
