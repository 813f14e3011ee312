// Two columns of the reference's 2 x 2 CG case (src/solver/cg.rs:310-323) at once through the C++ mirror (include/kryst_hip.hpp): MultiVec,
// spmm and solve_many against the single-vector calls, bit for bit.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static bool same_bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

int main() {
    // [[4,1],[1,3]] x = [1,2] -> [1/11, 7/11]; the second column is the same system with another right-hand side
    auto a = HipCsrMatrix::from_csr(2, 2, {0, 2, 4}, {0, 1, 0, 1}, {4.0, 1.0, 1.0, 3.0});
    const std::vector<Vec> bs = {{1.0, 2.0}, {-3.0, 0.5}};
    const Vec expected{0.09090909090909091, 0.6363636363636364};
    {   // spmm: column j is spmv on column j
        MultiVec x = MultiVec::from_columns(bs), y(2, 2);
        a.spmm(x, y);
        for (size_t j = 0; j < 2; ++j) { Vec yj(2, 0.0); a.spmv(bs[j], yj); REQUIRE(same_bits(y.column(j), yj)); }
        bool threw = false;
        try { a.spmm(x, x); } catch (const KError& e) { threw = e.code == KRYST_ERR_ARG; }
        REQUIRE(threw);
    }
    for (int pcg = 0; pcg < 2; ++pcg) {
        std::vector<Vec> xs; std::vector<SolveStats<double>> single; std::vector<std::vector<double>> hists;
        IdentityPC id; id.setup(a);
        for (size_t j = 0; j < 2; ++j) {
            Vec x{0.0, 0.0};
            if (pcg) { PcgSolver s(1e-10, 20); single.push_back(s.solve(a, &id, bs[j], x)); hists.push_back(s.residual_history); }
            else { CgSolver s(1e-10, 20); single.push_back(s.solve(a, nullptr, bs[j], x)); hists.push_back(s.residual_history); }
            xs.push_back(x);
        }
        for (size_t i = 0; i < 2; ++i) REQUIRE(std::fabs(xs[0][i] - expected[i]) < 1e-8);
        MultiVec b = MultiVec::from_columns(bs), x(2, 2);
        std::vector<SolveStats<double>> stats;
        std::vector<int32_t> codes;
        std::vector<std::vector<double>> many;
        if (pcg) { PcgSolver s(1e-10, 20); codes = s.solve_many(a, &id, b, x, stats); many = s.residual_histories; }
        else { CgSolver s(1e-10, 20); codes = s.solve_many(a, nullptr, b, x, stats); many = s.residual_histories; }
        REQUIRE(codes.size() == 2 && stats.size() == 2 && many.size() == 2);
        for (size_t j = 0; j < 2; ++j) {
            REQUIRE(codes[j] == KRYST_OK && stats[j].converged && stats[j].iterations == single[j].iterations);
            REQUIRE(std::memcmp(&stats[j].final_residual, &single[j].final_residual, sizeof(double)) == 0);
            REQUIRE(same_bits(many[j], hists[j]));
            REQUIRE(same_bits(x.column(j), xs[j]));
        }
    }
    {   // three columns: refused
        bool threw = false;
        try { MultiVec bad(2, 3); } catch (const KError& e) { threw = e.code == KRYST_ERR_ARG; }
        REQUIRE(threw);
    }
    std::printf("CPP_MULTI_MIRROR_OK\n");
    return 0;
}
