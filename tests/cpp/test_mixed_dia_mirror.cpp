// The diagonal lowering through the C++ mirror (include/kryst_hip.hpp): HipCsrMatrix32(a, Dia) on a 1500-row tridiagonal operator with distinct
// values, created under KRYST_SPMV_DIA=2 so that it keeps CSR-DIA streams, must report the dia kernel and give, bit for bit, the product of the
// plain-lowered operator and of a host fold of the contract; Auto never chooses the diagonal form; an operator created
// without streams refuses it.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
    const size_t n = 1500;                                                         // two fp32 tiles, the second partial
    std::vector<size_t> rp{0}, ci; Vec va;
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { ci.push_back(i - 1); va.push_back(-1.1 - 1e-3 * (double)i); }  // (not fp32 numbers: the lowering rounds them)
        ci.push_back(i); va.push_back(2.7 + 1e-3 * (double)i);
        if (i + 1 < n) { ci.push_back(i + 1); va.push_back(-0.9 + 1e-4 * (double)i); }
        rp.push_back(ci.size());
    }
    unsetenv("KRYST_SPMV32_FORM");
    setenv("KRYST_SPMV_DIA", "0", 1);
    const HipCsrMatrix bare = HipCsrMatrix::from_csr(n, n, rp, ci, va);             // no streams: the form is refused
    bool refused = false;
    try { const HipCsrMatrix32 no(bare, HipCsrMatrix32::Dia); } catch (const std::exception&) { refused = true; }
    REQUIRE(refused);
    setenv("KRYST_SPMV_DIA", "2", 1);
    const HipCsrMatrix a = HipCsrMatrix::from_csr(n, n, rp, ci, va);
    unsetenv("KRYST_SPMV_DIA");
    const HipCsrMatrix32 plain(a), dia(a, HipCsrMatrix32::Dia), any(a, HipCsrMatrix32::Auto);
    REQUIRE(plain.encoding() == "plain");
    REQUIRE(dia.encoding() == "dia");
    REQUIRE(any.encoding() != "dia");
    REQUIRE(dia.info() == plain.info());
    std::vector<float> x(n), yp(n, NAN), yd(n, NAN), want(n);
    for (size_t i = 0; i < n; ++i) x[i] = (float)(0.37 * (double)(i % 97) - 1.3) / 3.0f;
    for (size_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (size_t k = rp[i]; k < rp[i + 1]; ++k) s = s + (double)(float)va[k] * (double)x[ci[k]];
        want[i] = (float)s;
    }
    plain.spmv(x, yp); dia.spmv(x, yd);
    REQUIRE(std::memcmp(yd.data(), yp.data(), n * sizeof(float)) == 0);
    REQUIRE(std::memcmp(yd.data(), want.data(), n * sizeof(float)) == 0);
    setenv("KRYST_SPMV32_FORM", "plain", 1);
    REQUIRE(dia.encoding() == "plain");
    unsetenv("KRYST_SPMV32_FORM");
    std::printf("CPP_MIXED_DIA_MIRROR_OK\n");
    return 0;
}
