// Mixed precision: the fp32 vector handle, the conversions between fp32 and fp64 vectors, the inner product of two fp32
// vectors and the published shape of its tree.
#include "mixed.h"

namespace kr {

__global__ void round_kernel(float* dst, const double* src, int64_t n, int divide, double den) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = divide ? (float)(src[i] / den) : (float)src[i];
}
__global__ void widen_kernel(double* dst, const float* src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}
// elements [n, cap): count those whose bits are not +0.0, then (fill) overwrite them.  One workgroup.
__global__ void vec32_padding_kernel(float* d, int64_t n, int64_t cap, int fill, float value, unsigned long long* count) {
    unsigned long long mine = 0;
    for (int64_t e = n + threadIdx.x; e < cap; e += blockDim.x) {
        if (__float_as_uint(d[e]) != 0u) ++mine;
        if (fill) d[e] = value;
    }
    if (mine) atomicAdd(count, mine);
}

hipError_t enqueue_round32(kryst_ctx_t ctx, float* dst, const double* src, int64_t n, int divide, double den) {
    hipLaunchKernelGGL(round_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->s_main, dst, src, n, divide, den);
    return hipGetLastError();
}

int32_t vec32_check(kryst_vec32_t v) { KR_ARG(v && v->d && v->ctx, "vec32: null handle"); return KRYST_OK; }
int32_t vec32_alloc(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out) {
    kryst_vec32_t v = new kryst_vec32_s();
    v->ctx = ctx; v->n = n;
    const size_t bytes = sizeof(float) * (size_t)vec32_len(n);
    if (hipMalloc(&v->d, bytes) != hipSuccess) { (void)hipGetLastError(); delete v; set_error("hipMalloc(%zu) failed", bytes); return KRYST_ERR_HIP; }
    if (hipMemsetAsync(v->d, 0, bytes, ctx->s_main) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(v->d); delete v; set_error("hipMemsetAsync failed"); return KRYST_ERR_HIP; }
    *out = v;
    return KRYST_OK;
}
void vec32_free(kryst_vec32_t v) {
    if (!v) return;
    (void)hipStreamSynchronize(v->ctx->s_main);
    (void)hipFree(v->d);
    delete v;
}

}  // namespace kr

using namespace kr;

extern "C" {

void kryst_reduce_spec32(int32_t* T, int32_t* V, int32_t* F) {
    if (T) *T = KR32_T;
    if (V) *V = KR32_V;
    if (F) *F = KR_F;
}

int32_t kryst_host_round_f32(const double* v, int64_t n, float* out, int64_t info[2]) {
    KR_ARG(n >= 0 && (n == 0 || (v && out)), "host_round_f32");
    unsigned long long cnt[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i) out[i] = round_count(v[i], cnt);
    if (info) { info[0] = (int64_t)cnt[0]; info[1] = (int64_t)cnt[1]; }
    if (cnt[2]) { set_error("round_f32: %llu finite value(s) would round to +-inf in fp32", cnt[2]); return KRYST_UNSUPPORTED; }
    return KRYST_OK;
}

int32_t kryst_vec32_create(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out) {
    KR_ARG(ctx && out && n >= 0, "vec32_create");
    KR_HIP(hipSetDevice(ctx->device));
    return vec32_alloc(ctx, n, out);
}

int32_t kryst_vec32_destroy(kryst_vec32_t v) {
    if (!v) return KRYST_OK;
    (void)hipSetDevice(v->ctx->device);
    vec32_free(v);
    return KRYST_OK;
}

int32_t kryst_vec32_upload(kryst_vec32_t v, const float* host, int64_t n) {
    KR_TRY(vec32_check(v));
    KR_ARG(host || n == 0, "vec32_upload");
    KR_ARG(n == v->n, "vec32_upload: length mismatch");
    KR_HIP(hipSetDevice(v->ctx->device));
    if (n > 0) KR_HIP(hipMemcpyAsync(v->d, host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, v->ctx->s_main));
    KR_HIP(hipStreamSynchronize(v->ctx->s_main));
    return KRYST_OK;
}

int32_t kryst_vec32_download(kryst_vec32_t v, float* host, int64_t n) {
    KR_TRY(vec32_check(v));
    KR_ARG(host || n == 0, "vec32_download");
    KR_ARG(n == v->n, "vec32_download: length mismatch");
    KR_HIP(hipSetDevice(v->ctx->device));
    if (n > 0) KR_HIP(hipMemcpyAsync(host, v->d, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, v->ctx->s_main));
    KR_HIP(hipStreamSynchronize(v->ctx->s_main));
    return KRYST_OK;
}

int32_t kryst_bench_vec32_padding(kryst_vec32_t v, const float* fill, int64_t* dirty) {
    KR_TRY(vec32_check(v));
    kryst_ctx_t ctx = v->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    unsigned long long* d_count = nullptr;
    KR_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->s_main);
    unsigned long long count = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(vec32_padding_kernel, dim3(1), dim3(1024), 0, ctx->s_main, v->d, v->n, vec32_len(v->n), fill ? 1 : 0, fill ? *fill : 0.0f, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->s_main);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->s_main);
    (void)hipFree(d_count);
    KR_HIP(e);
    if (dirty) *dirty = (int64_t)count;
    return KRYST_OK;
}

int32_t kryst_vec32_from_f64(kryst_vec32_t dst, kryst_vec_t src) {
    KR_TRY(vec32_check(dst));
    KR_ARG(src && src->ctx == dst->ctx, "vec32_from_f64: null vector or context mismatch");
    KR_ARG(src->n == dst->n, "vec32_from_f64: length mismatch");
    KR_HIP(hipSetDevice(dst->ctx->device));
    if (dst->n > 0) KR_HIP(enqueue_round32(dst->ctx, dst->d, src->d, dst->n, 0, 1.0));
    return KRYST_OK;
}

int32_t kryst_vec32_to_f64(kryst_vec_t dst, kryst_vec32_t src) {
    KR_TRY(vec32_check(src));
    KR_ARG(dst && dst->ctx == src->ctx, "vec32_to_f64: null vector or context mismatch");
    KR_ARG(src->n == dst->n, "vec32_to_f64: length mismatch");
    KR_HIP(hipSetDevice(src->ctx->device));
    if (src->n == 0) return KRYST_OK;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(src->n)), dim3(256), 0, src->ctx->s_main, dst->d, src->d, src->n);
    KR_HIP(hipGetLastError());
    return KRYST_OK;
}

int32_t kryst_dot32(kryst_vec32_t x, kryst_vec32_t y, double* out) {
    KR_TRY(vec32_check(x)); KR_TRY(vec32_check(y));
    KR_ARG(x->ctx == y->ctx, "dot32: vectors belong to different contexts");
    KR_ARG(x->n == y->n, "dot32: vector length mismatch");
    KR_ARG(out, "dot32: out");
    kryst_ctx_t ctx = x->ctx;
    if (ctx->nranks > 1) { set_error("dot32: distributed contexts are not supported"); return KRYST_UNSUPPORTED; }
    KR_HIP(hipSetDevice(ctx->device));
    KR_TRY(launch_dot32(ctx, x->d, y->d, x->n));
    return fold_to_host(ctx, ntiles32_of(x->n), out);
}

}  // extern "C"
