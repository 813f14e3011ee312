// Multivectors (n x K, K in {2, 4, 8}) for several right-hand sides at once: storage and the SpMM launcher.
//
// Element (i, j) lives at i*K + j: the K values of a row are contiguous, so a gather of x-row c is one aligned run of 8 K bytes and the
// two rows a lane owns (ew.h: thread t of a tile owns rows 2t, 2t+1) are 2 K contiguous doubles.  The allocation holds
// ceil(n / 512) * 512 + 512 rows, zero at creation -- kryst_vec_t's padding rule, per column.
#pragma once
#include "csr.h"

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
// nq = 1: also the tile partials of sum_i D(i, j) * Y(i, j) for every column j into partials[j * pstride + tile].  `done` (device flag) makes the
// launch a no-op when set.
int32_t launch_spmm(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done);
// The choice (multi.hip), from the forms the operator has and KRYST_SPMM_FORM = auto | plain | dia, read at every launch: does launch_spmm take
// spmm_dia_kernel for k columns?
bool spmm_takes_dia(kryst_csr_t a, int k);
// multi_dia.hip: the same launch through spmm_dia_kernel, for an operator that holds the streams
int32_t launch_spmm_dia(kryst_csr_t a, int k, const double* x, double* y, int nq, const double* dvec, double* partials, int64_t pstride, const int* done);

}  // namespace kr
