// HipCsrMatrix::spmm_kernel(k) through the C++ mirror (include/kryst_hip.hpp): on a 1500-row tridiagonal operator with 4498 distinct values --
// one that keeps CSR-DIA streams under the defaults -- the hook reports the diagonal kernel under KRYST_SPMM_FORM=dia and the plain one under
// KRYST_SPMM_FORM=plain, and spmm gives the bits of spmv on every column under both.  Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static bool same_bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

int main() {
    const size_t n = 1500;
    std::vector<size_t> row_ptr{0}, col_idx;
    Vec values;
    for (size_t i = 0; i < n; ++i) {
        for (int off = -1; off <= 1; ++off) {
            if ((off < 0 && i == 0) || (off > 0 && i + 1 == n)) continue;
            col_idx.push_back(i + off);
            values.push_back((off == 0 ? 4.0 : -1.0) + 1e-4 * (double)(3 * i + (size_t)(off + 1)));      // no two alike
        }
        row_ptr.push_back(col_idx.size());
    }
    auto a = HipCsrMatrix::from_csr(n, n, row_ptr, col_idx, values);
    std::vector<Vec> cols(8, Vec(n));
    for (size_t j = 0; j < 8; ++j)
        for (size_t i = 0; i < n; ++i) cols[j][i] = 1.0 / (double)(1 + (7 * i + 13 * j) % 101) - 0.25 * (double)j;
    std::vector<Vec> want;
    for (size_t j = 0; j < 8; ++j) { Vec y(n, 0.0); a.spmv(cols[j], y); want.push_back(y); }
    for (const char* form : {"dia", "plain"}) {
        setenv("KRYST_SPMM_FORM", form, 1);
        for (int k : {2, 4, 8}) {
            REQUIRE(a.spmm_kernel(k) == form);
            MultiVec x = MultiVec::from_columns(std::vector<Vec>(cols.begin(), cols.begin() + k)), y(n, k);
            a.spmm(x, y);
            for (int j = 0; j < k; ++j) REQUIRE(same_bits(y.column((size_t)j), want[(size_t)j]));
        }
        bool threw = false;
        try { (void)a.spmm_kernel(3); } catch (const KError& e) { threw = e.code == KRYST_ERR_ARG; }
        REQUIRE(threw);
    }
    unsetenv("KRYST_SPMM_FORM");
    std::printf("CPP_SPMM_DIA_MIRROR_OK\n");
    return 0;
}
