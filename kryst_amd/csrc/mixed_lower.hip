// Mixed precision: the lowered operator.  kryst_csr32_lower_form is the skeleton -- the plain arrays, the counters, one
// synchronisation, the refusals -- and each storage form lowers itself beside its kernels (mixed_pattern.hip, mixed_dia.hip).
#include "mixed.h"

namespace kr {

__global__ void lower_values_kernel(float* dst, const double* src, int64_t n, unsigned long long* count) {
    unsigned long long cnt[3] = {0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = round_count(src[i], cnt);
    for (int k = 0; k < 3; ++k) { if (cnt[k]) atomicAdd(count + k, cnt[k]); }
}

int32_t csr32_check(kryst_csr32_t a) { KR_ARG(a && a->ctx && a->d_row_ptr, "csr32: null handle"); return KRYST_OK; }
static void csr32_free(kryst_csr32_t a) {
    if (!a) return;
    (void)hipStreamSynchronize(a->ctx->s_main);
    (void)hipFree(a->d_row_ptr); (void)hipFree(a->d_col); (void)hipFree(a->d_val);
    (void)hipFree(a->d_pid); (void)hipFree(a->d_pmeta); (void)hipFree(a->d_poff); (void)hipFree(a->d_pval);
    (void)hipFree(a->d_dia);
    delete a;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_csr32_lower(kryst_csr_t a, kryst_csr32_t* out) { return kryst_csr32_lower_form(a, KRYST_CSR32_PLAIN, out); }

int32_t kryst_csr32_lower_form(kryst_csr_t a, int32_t form, kryst_csr32_t* out) {
    KR_ARG(a && out, "csr32_lower");
    KR_ARG(form == KRYST_CSR32_PLAIN || form == KRYST_CSR32_AUTO || form == KRYST_CSR32_PATTERN || form == KRYST_CSR32_DIA, "csr32_lower: unknown form");
    kryst_ctx_t ctx = a->ctx;
    if (a->dist || ctx->nranks > 1) { set_error("csr32_lower: distributed operators are not supported"); return KRYST_UNSUPPORTED; }
    KR_ARG(a->d_row_ptr && a->d_col && a->d_val, "csr32_lower: the operator keeps no CSR arrays");
    KR_ARG(a->nrows < (1ll << 31) - KR32_TILE && a->nnz < (1ll << 31) - 4096, "csr32_lower: too many rows or entries");
    // a form asked for by name is refused where the operator cannot take it; AUTO is the row-pattern form where it can, else plain, never the diagonal form
    const char* no_pattern = lower_pattern_refusal(a);
    const char* why = form == KRYST_CSR32_PATTERN ? no_pattern : form == KRYST_CSR32_DIA ? lower_dia_refusal(a) : nullptr;
    if (why) { set_error("csr32_lower: %s", why); return KRYST_UNSUPPORTED; }
    const bool pattern = (form == KRYST_CSR32_AUTO || form == KRYST_CSR32_PATTERN) && !no_pattern;
    KR_HIP(hipSetDevice(ctx->device));
    kryst_csr32_t m = new kryst_csr32_s();
    m->ctx = ctx; m->nrows = a->nrows; m->ncols = a->ncols; m->nnz = a->nnz;
    unsigned long long* d_count = nullptr;
    unsigned long long cnt[4] = {0, 0, 0, 0};                                // lower_values_kernel's three, and the streams' refused entries
    const size_t ne = (size_t)a->nnz + 8;
    hipError_t e = hipMalloc(&m->d_row_ptr, sizeof(int32_t) * (size_t)(a->nrows + 1));
    if (e == hipSuccess) e = hipMalloc(&m->d_col, sizeof(int32_t) * ne);
    if (e == hipSuccess) e = hipMalloc(&m->d_val, sizeof(float) * ne);
    if (e == hipSuccess) e = hipMalloc(&d_count, sizeof cnt);
    if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, sizeof cnt, ctx->s_main);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_col, 0, sizeof(int32_t) * ne, ctx->s_main);
    if (e == hipSuccess) e = hipMemsetAsync(m->d_val, 0, sizeof(float) * ne, ctx->s_main);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_row_ptr, a->d_row_ptr, sizeof(int32_t) * (size_t)(a->nrows + 1), hipMemcpyDeviceToDevice, ctx->s_main);
    if (e == hipSuccess && a->nnz > 0) e = hipMemcpyAsync(m->d_col, a->d_col, sizeof(int32_t) * (size_t)a->nnz, hipMemcpyDeviceToDevice, ctx->s_main);
    if (e == hipSuccess && a->nnz > 0) {
        hipLaunchKernelGGL(lower_values_kernel, dim3(grid_for(a->nnz)), dim3(256), 0, ctx->s_main, m->d_val, a->d_val, a->nnz, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess && pattern) e = enqueue_lower_pattern(a, m);
    if (e == hipSuccess && form == KRYST_CSR32_DIA) e = enqueue_lower_dia(a, m, d_count + 3);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost, ctx->s_main);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d_count);
    if (e != hipSuccess) { (void)hipGetLastError(); csr32_free(m); set_error("csr32_lower: %s", hipGetErrorString(e)); return KRYST_ERR_HIP; }
    if (cnt[2] || cnt[3]) {
        csr32_free(m);
        if (cnt[2]) set_error("csr32_lower: %llu finite value(s) would round to +-inf in fp32", cnt[2]);
        else set_error("csr32_lower: %llu stored NaN(s) round to the bits of the fp32 absent marker; the diagonal form is refused", cnt[3]);
        return KRYST_UNSUPPORTED;
    }
    m->changed = (int64_t)cnt[0]; m->tiny = (int64_t)cnt[1];
    *out = m;
    return KRYST_OK;
}

int32_t kryst_csr32_info(kryst_csr32_t a, int64_t info[3]) {
    KR_TRY(csr32_check(a));
    KR_ARG(info, "csr32_info");
    info[0] = a->changed; info[1] = a->tiny; info[2] = a->nrows;
    return KRYST_OK;
}

int32_t kryst_csr32_destroy(kryst_csr32_t a) {
    if (!a) return KRYST_OK;
    (void)hipSetDevice(a->ctx->device);
    csr32_free(a);
    return KRYST_OK;
}

}  // extern "C"
