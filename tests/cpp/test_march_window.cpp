// The window map of the marching kernels (kryst_amd/csrc/march_window.h) on the CPU: for every even line length n from 4 to 512, strips of T = 2, 4 and
// 8 tiles and workgroups of 256 and 512 threads, every pair of the window is requested by exactly one (lane, request), request k of a lane is the pair
// of its own tile k, no LDS offset leaves the window, and every lane issues ceil((R + 2 n) / (2 threads)) requests.  Stand-alone: built with
// -fsanitize=address,undefined and run by tests/test_march_window_cpu.py; needs no GPU and no HIP header.
#include "../../kryst_amd/csrc/march_window.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                                                                                     \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                    \
    } while (0)

int main() {
    long cases = 0, requests = 0;
    for (int n = 4; n <= 512; n += 2)
        for (int T : {2, 4, 8})
            for (int threads : {256, 512}) {
                ++cases;
                const int R = 512 * T, elems = R + 2 * n, pairs = elems / 2;
                CHECK(kr::march_window_elems(n, T) == elems, "n %d T %d", n, T);
                const int nreq = kr::march_window_requests(n, T, threads);
                CHECK(nreq == (elems + 2 * threads - 1) / (2 * threads), "n %d T %d threads %d: %d requests", n, T, threads, nreq);
                const int tl = kr::march_window_own_requests(T, threads);
                CHECK(tl * threads * 2 == R, "n %d T %d threads %d: %d own requests", n, T, threads, tl);
                // the window's LDS buffer, exactly as long as the window: the sanitizer sees an offset that leaves it
                std::vector<int> hits((size_t)elems, 0);
                for (int t = 0; t < threads; ++t)
                    for (int k = 0; k < nreq; ++k) {
                        ++requests;
                        const kr::MarchWindowRequest q = kr::march_window_request(t, k, n, T, threads);
                        if (k < tl) {
                            // the lane's own tile k: tile (t / 256) tl + k of the strip, rows 2 (t % 256), + 1 of it, at the offset step b. reads B from
                            const int tile = (t / 256) * tl + k, row = tile * 512 + 2 * (t % 256);
                            CHECK(tile < T, "n %d T %d threads %d lane %d request %d: tile %d", n, T, threads, t, k, tile);
                            CHECK(q.pair == (n + row) / 2, "n %d T %d threads %d lane %d request %d: pair %d, own row %d", n, T, threads, t, k, q.pair, row);
                            CHECK(q.lds == kr::march_window_tile_offset(n, tile) + 2 * (t % 256), "n %d T %d threads %d lane %d request %d: lds %d", n, T, threads, t, k, q.lds);
                        } else if (q.pair >= 0) {
                            CHECK(q.pair < n / 2 || q.pair >= n / 2 + R / 2, "n %d T %d threads %d lane %d request %d: halo request on own pair %d", n, T, threads, t, k, q.pair);
                        }
                        if (q.pair < 0) { CHECK(q.lds < 0, "lds %d without a pair", q.lds); continue; }
                        CHECK(q.pair < pairs && q.lds == 2 * q.pair, "n %d T %d threads %d lane %d request %d: pair %d of %d, lds %d", n, T, threads, t, k, q.pair, pairs, q.lds);
                        if (q.pair < pairs && q.lds >= 0) { ++hits.at((size_t)q.lds); ++hits.at((size_t)q.lds + 1); }
                    }
                for (int e = 0; e < elems; ++e) CHECK(hits[(size_t)e] == 1, "n %d T %d threads %d: element %d requested %d times", n, T, threads, e, hits[(size_t)e]);
                // what step b. reads of the window for the strip's first and last pair of rows: -n, -2 .. +3, +n
                CHECK(kr::march_window_tile_offset(n, 0) - n == 0 && kr::march_window_tile_offset(n, T - 1) + 510 + n + 1 == elems - 1, "n %d T %d: operands leave the window", n, T);
            }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("march window ok: %ld cases, %ld requests\n", cases, requests);
    return 0;
}
