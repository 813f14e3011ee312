// What the two additive Schwarz kinds share (asm.hip defines it; asm_ilu.hip uses it): the host bookkeeping of the index sets (sorting,
// owners, the row -> positions map of the combine), the growth on the device, the memory check and the combine launch.
#pragma once
#include "pc.h"
#include <algorithm>
#include <vector>

namespace kr {

// the sets of a set-up: sorted ascending and packed like CSR rows, the last un-grown set of every row (-1: none)
struct AsmSets {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx, owner;
};

int32_t asm_check(kryst_csr_t a, int32_t overlap, int32_t variant);
// asm.rs:46-56: p = max(nparts, 1) parts of chunk = ceil(n / p) rows (trailing parts may be empty), packed like CSR rows
void asm_uniform_sets(int64_t n, int64_t nparts, std::vector<int64_t>& ptr, std::vector<int64_t>& idx);
// sorts and checks the given sets and finds the owners; a set of more than `cap` rows is KRYST_UNSUPPORTED
int32_t asm_sort_sets(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int cap, AsmSets& s);
// grows the sorted sets by `overlap` layers on the device; a set that passes `cap` rows is KRYST_UNSUPPORTED.  cap <= KRYST_ASM_MAX_ROWS:
// merged and sorted in LDS; larger caps: a bitmap over the rows per workgroup
int32_t asm_grow(kryst_csr_t a, int overlap, std::vector<int64_t>& ptr, std::vector<int32_t>& idx, int cap);
// row -> positions in X: every set that contains the row, ascending (restricted: the owner's position only)
void asm_row_map(int64_t n, int32_t variant, const AsmSets& s, std::vector<int32_t>& mptr, std::vector<int32_t>& mpos);
int32_t asm_check_memory(int device, unsigned long long need);
// z[row] = ((+0.0 + X[p1]) + X[p2]) + ... over the map, on ctx->s_main
int32_t asm_combine_launch(kryst_ctx_t ctx, const int32_t* mptr, const int32_t* mpos, const double* X, int64_t n, double* z, const int* done);

template <class T> inline int32_t asm_upload(kryst_ctx_t ctx, T** d, const std::vector<T>& h, const char* what) {
    if (pool_malloc(d, sizeof(T) * std::max<size_t>(h.size(), 1)) != hipSuccess) {
        (void)hipGetLastError();
        *d = nullptr;
        set_error("additive Schwarz: out of device memory (%s)", what);
        return KRYST_ERR_HIP;
    }
    if (!h.empty()) KR_HIP(hipMemcpyAsync(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->s_main));
    return KRYST_OK;
}

}  // namespace kr
