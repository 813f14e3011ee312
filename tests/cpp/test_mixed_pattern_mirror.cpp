// The row-pattern lowering through the C++ mirror (include/kryst_hip.hpp): HipCsrMatrix32(a, Pattern) on a 64-row tridiagonal operator must
// report the pattern kernel and give, bit for bit, the product of the plain-lowered operator and of a host fold of the contract (DESIGN.md
// section 4.16); a plain lowering reports "plain"; Auto keeps the pattern form where there is one.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
    const size_t n = 64;
    std::vector<size_t> rp{0}, ci; Vec va;
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { ci.push_back(i - 1); va.push_back(-1.1); }                    // (not fp32 numbers: the lowering rounds them)
        ci.push_back(i); va.push_back(2.7);
        if (i + 1 < n) { ci.push_back(i + 1); va.push_back(-0.9); }
        rp.push_back(ci.size());
    }
    const HipCsrMatrix a = HipCsrMatrix::from_csr(n, n, rp, ci, va);
    const HipCsrMatrix32 plain(a), pattern(a, HipCsrMatrix32::Pattern), any(a, HipCsrMatrix32::Auto);
    REQUIRE(plain.encoding() == "plain");
    REQUIRE(pattern.encoding() == "pattern");
    REQUIRE(any.encoding() == "pattern");
    REQUIRE(pattern.info() == plain.info());
    std::vector<float> x(n), yp(n, NAN), yq(n, NAN), ya(n, NAN), want(n);
    for (size_t i = 0; i < n; ++i) x[i] = (float)(0.37 * (double)i - 1.3) / 3.0f;
    for (size_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (size_t k = rp[i]; k < rp[i + 1]; ++k) s = s + (double)(float)va[k] * (double)x[ci[k]];
        want[i] = (float)s;
    }
    plain.spmv(x, yp); pattern.spmv(x, yq); any.spmv(x, ya);
    REQUIRE(std::memcmp(yq.data(), yp.data(), n * sizeof(float)) == 0);
    REQUIRE(std::memcmp(ya.data(), yp.data(), n * sizeof(float)) == 0);
    REQUIRE(std::memcmp(yq.data(), want.data(), n * sizeof(float)) == 0);
    std::printf("CPP_MIXED_PATTERN_MIRROR_OK\n");
    return 0;
}
