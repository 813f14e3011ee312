// What the window kernels of the plain CSR arrays share (spmv_stream.hip: spmv_wave_kernel; cheb_poly.hip: cheb_poly_step_kernel): the
// streamed loads and the ascending row sum over a wave's LDS window of products.
#pragma once
#include "common.h"

namespace kr {

typedef int    v2i __attribute__((ext_vector_type(2)));
typedef double v2d __attribute__((ext_vector_type(2)));

template <bool NT, class T>
__device__ __forceinline__ T stream_load(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// ascending serial sum of prod[beg-base .. end-base) continued into s: LDS reads are issued four at a time
// (clamped, branch-free) and folded in index order
__device__ __forceinline__ double row_sum(const double* prod, int base, int beg, int end, double s) {
    for (int k = beg; k < end; k += 4) {
        const int last = end - 1 - base;
        const double v0 = prod[k - base];
        const double v1 = prod[min(k + 1 - base, last)];
        const double v2 = prod[min(k + 2 - base, last)];
        const double v3 = prod[min(k + 3 - base, last)];
        s = s + v0;
        if (k + 1 < end) s = s + v1;
        if (k + 2 < end) s = s + v2;
        if (k + 3 < end) s = s + v3;
    }
    return s;
}

}  // namespace kr
