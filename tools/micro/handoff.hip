// Micro-benchmark: what does a kernel on this MI355X get back from the 256 MiB Infinity Cache of what the kernel BEFORE it in the stream touched
// last?  (CG's two marching kernels hand 1 GiB vectors to each other; both walk upward, so each starts where the other began, not where it ended.)
//   producer  512 resident workgroups of 256 threads, 16 B per lane, tiles b, b + 512, ... ascending: reads A and B, writes C   -- the fused SpMV's shape
//   consumer  the same grid: reads C and A, writes A
//             dir 0  ascending from the start (what the residual pass does today)
//             dir 1  descending from the end: tile ntiles - 1 - q, exactly mirrored, so the rows the producer touched last come first
//   policies  producer stores plain | nontemporal; consumer loads plain | nontemporal (its stores are nontemporal, as the residual pass's are)
// Prints the consumer's time: min / median / max of 5 timed launches after a warm-up, every (policy, direction, extent) pair interleaved in one
// process; the producer runs in full before every consumer launch.  extent: the consumer's first 64 / 128 / 256 / 512 MiB of each buffer in ITS
// order (a shortened pass), or all of it.  The front of a strided grid is the ideal case: a marching kernel's workgroups end on 512 strips of
// several segments, not on one contiguous top.
// build: hipcc --offload-arch=gfx950 -O3 tools/micro/handoff.hip -o tools/micro/handoff
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double v2d __attribute__((ext_vector_type(2)));

template <bool NT> __device__ __forceinline__ v2d ld(const v2d* p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT> __device__ __forceinline__ void st(v2d* p, v2d v) { if (NT) __builtin_nontemporal_store(v, p); else *p = v; }

// ntiles tiles of 256 lanes x 16 B in each buffer
template <bool ST_NT>
__global__ __launch_bounds__(256) void producer(const v2d* a, const v2d* b, v2d* c, long long ntiles) {
    for (long long q = blockIdx.x; q < ntiles; q += gridDim.x) {
        const long long i = q * 256 + threadIdx.x;
        const v2d x = ld<true>(a + i), y = ld<true>(b + i);
        st<ST_NT>(c + i, x + 0.5 * y);
    }
}
// the first `take` tiles of the consumer's order
template <bool LD_NT, bool DOWN>
__global__ __launch_bounds__(256) void consumer(const v2d* c, v2d* a, long long ntiles, long long take) {
    for (long long q = blockIdx.x; q < take; q += gridDim.x) {
        const long long t = DOWN ? ntiles - 1 - q : q;
        const long long i = t * 256 + threadIdx.x;
        const v2d x = ld<LD_NT>(a + i), y = ld<LD_NT>(c + i);
        st<true>(a + i, x - 0.25 * y);
    }
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

struct Form { int st_nt, ld_nt, down; long long mib; std::vector<float> ms; };

int main() {
    const size_t bytes = 1ull << 30;
    const long long ntiles = (long long)(bytes / 4096);
    v2d *a, *b, *c;
    CK(hipMalloc(&a, bytes)); CK(hipMalloc(&b, bytes)); CK(hipMalloc(&c, bytes));
    {
        std::vector<double> h(bytes / 8);
        for (size_t i = 0; i < h.size(); ++i) h[i] = 1.0 + (double)(i & 1023) * 1e-3;
        CK(hipMemcpy(a, h.data(), bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(b, h.data(), bytes, hipMemcpyHostToDevice));
        CK(hipMemset(c, 0, bytes));
    }
    std::vector<Form> forms;
    for (long long mib : {1024ll, 64ll, 128ll, 256ll, 512ll})
        for (int st_nt : {0, 1}) for (int ld_nt : {0, 1}) for (int down : {0, 1}) forms.push_back({st_nt, ld_nt, down, mib, {}});
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const dim3 grid(512), block(256);
    for (int r = 0; r < 6; ++r) {
        for (Form& f : forms) {
            if (f.st_nt) hipLaunchKernelGGL((producer<true>), grid, block, 0, 0, a, b, c, ntiles);
            else hipLaunchKernelGGL((producer<false>), grid, block, 0, 0, a, b, c, ntiles);
            const long long take = f.mib * 256;                      // tiles of 4 KiB
            CK(hipEventRecord(e0, 0));
            if (f.ld_nt && f.down) hipLaunchKernelGGL((consumer<true, true>), grid, block, 0, 0, c, a, ntiles, take);
            else if (f.ld_nt) hipLaunchKernelGGL((consumer<true, false>), grid, block, 0, 0, c, a, ntiles, take);
            else if (f.down) hipLaunchKernelGGL((consumer<false, true>), grid, block, 0, 0, c, a, ntiles, take);
            else hipLaunchKernelGGL((consumer<false, false>), grid, block, 0, 0, c, a, ntiles, take);
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float m; CK(hipEventElapsedTime(&m, e0, e1));
            if (r) f.ms.push_back(m);
        }
    }
    printf("consumer after a full producer pass; 3 buffers of 1 GiB; us = min / median / max of 5; GB/s at the median (3 x extent bytes)\n");
    printf("extent_MiB producer_store consumer_load direction   us_min  us_med  us_max   GB/s\n");
    for (Form& f : forms) {
        std::sort(f.ms.begin(), f.ms.end());
        printf("%10lld %14s %13s %9s  %7.1f %7.1f %7.1f  %6.0f\n", f.mib, f.st_nt ? "nt" : "plain", f.ld_nt ? "nt" : "plain", f.down ? "down" : "up",
               f.ms[0] * 1e3, f.ms[2] * 1e3, f.ms[4] * 1e3, 3.0 * (double)f.mib * 1048576.0 / (f.ms[2] * 1e-3) / 1e9);
    }
    hipFree(a); hipFree(b); hipFree(c);
    return 0;
}
