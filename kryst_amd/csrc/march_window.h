// The window of the marching kernels (spmv_fuse.hip: fuse_march, cg_recompute_residual_kernel) and which lane requests which of its pairs.  Host and
// device: no other header is needed (tests/cpp/test_march_window.cpp drives it on the CPU).
//   A strip is R = 512 T consecutive rows of a plane, first row r0; its window is the R + 2 n doubles from row r0 - n (n: the line length, even), i.e.
//   R / 2 + n pairs of 16 bytes: n / 2 pairs of the line below, the strip's own R / 2, n / 2 of the line above.  Nothing else is read by a tile: its
//   operands are rows -n, -1, 0, +1, +n (the far ones are not in the window).  Window pair q holds rows r0 - n + 2 q, + 1 and lies at doubles 2 q, 2 q + 1
//   of the window's LDS buffer.
//   Requests.  Lane t of `threads` computes TL = 256 T / threads tiles per plane: tile (t / 256) TL + k, rows 2 (t % 256), + 1 of it, k = 0 .. TL - 1.  Its
//   request k < TL is that pair -- what the lane loads first is what it computes on and what it stores, and whether a request is an own pair is a
//   compile-time fact of its index -- and requests TL, TL + 1, .. are its share of the n halo pairs: halo pair h = (k - TL) threads + t, the line below
//   first (h < n / 2), then the line above; h >= n: no pair (the lane repeats some valid pair and drops it, so that no load stands behind a branch).
//   Every lane issues march_window_requests() = ceil((R + 2 n) / (2 threads)) requests: 6 at n = 512, T = 4 and 256 threads.  The kernels run 256
//   threads (TL = T); the map also holds for the 512 that strips of 8 tiles were measured with (profiles/march_t8/).
#pragma once
#if defined(__HIPCC__)
#define KR_MW_FN __host__ __device__ __forceinline__
#else
#define KR_MW_FN inline
#endif

namespace kr {

constexpr int KR_MW_TILE = 512, KR_MW_TILE_LANES = 256;     // rows of a tile; lanes that compute a tile, a pair of rows each (common.h: KR_TILE, KR_T)

KR_MW_FN constexpr int march_window_elems(int n, int T) { return T * KR_MW_TILE + 2 * n; }                   // doubles of one window
KR_MW_FN constexpr int march_window_own_requests(int T, int threads) { return T * KR_MW_TILE_LANES / threads; }     // TL
KR_MW_FN constexpr int march_window_requests(int n, int T, int threads) { return (march_window_elems(n, T) / 2 + threads - 1) / threads; }
// doubles from the window's [0] to the first row of tile k of the strip
KR_MW_FN constexpr int march_window_tile_offset(int n, int k) { return n + k * KR_MW_TILE; }

struct MarchWindowRequest { int pair; int lds; };           // window pair (-1: none) and the doubles from the window's [0] to it
KR_MW_FN MarchWindowRequest march_window_request(int t, int k, int n, int T, int threads) {
    const int tl = march_window_own_requests(T, threads);
    int q;
    if (k < tl) {
        q = n / 2 + ((t / KR_MW_TILE_LANES) * tl + k) * KR_MW_TILE_LANES + t % KR_MW_TILE_LANES;
    } else {
        const int h = (k - tl) * threads + t;
        q = h < n / 2 ? h : h < n ? T * KR_MW_TILE_LANES + h : -1;
    }
    return MarchWindowRequest{q, q < 0 ? -1 : 2 * q};
}

}  // namespace kr
