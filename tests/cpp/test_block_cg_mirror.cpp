// Block CG through the C++ mirror (include/kryst_hip.hpp: BlockCgSolver::solve_block) on tridiag(-1, 4, -1) of 600 rows with four right-hand
// sides, with and without Jacobi: against the host twin of the C interface (kryst_bcg_solve_multi) bit for bit, against the true residuals, and
// the two refusals of the class.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static bool same_bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

int main() {
    const size_t n = 600, k = 4;
    std::vector<size_t> rp{0}, ci; Vec va;
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { ci.push_back(i - 1); va.push_back(-1.0); }
        ci.push_back(i); va.push_back(4.0 + 0.001 * (double)(i % 7));
        if (i + 1 < n) { ci.push_back(i + 1); va.push_back(-1.0); }
        rp.push_back(ci.size());
    }
    auto a = HipCsrMatrix::from_csr(n, n, rp, ci, va);
    std::vector<Vec> bs(k, Vec(n));
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (size_t j = 0; j < k; ++j)
        for (size_t i = 0; i < n; ++i) { z = z * 6364136223846793005ull + 1442695040888963407ull; bs[j][i] = (double)(z >> 11) / 9007199254740992.0; }
    for (int jac = 0; jac < 2; ++jac) {
        Jacobi pc; pc.setup(a);
        const Preconditioner<HipCsrMatrix, Vec>* use = jac ? &pc : nullptr;
        MultiVec b = MultiVec::from_columns(bs), x(n, k);
        BlockCgSolver s(1e-10, 100);
        std::vector<SolveStats<double>> stats;
        const std::vector<int32_t> codes = s.solve_block(a, use, b, x, stats);
        REQUIRE(codes.size() == k && stats.size() == k && s.residual_histories.size() == k);
        // the host twin of the C interface, column-major with ld > n
        const size_t ld = n + 5, cap = 108;
        Vec bh(k * ld, 0.0), xh(k * ld, 0.0), hist(k * cap, 0.0);
        for (size_t j = 0; j < k; ++j) std::copy(bs[j].begin(), bs[j].end(), bh.begin() + (long)(j * ld));
        kryst_params_t p{};
        p.tol = 1e-10; p.max_iters = 100; p.norm_type = 1;
        std::vector<kryst_stats_t> st(k); std::vector<int32_t> code(k, -1); std::vector<int64_t> len(k, -1);
        check(kryst_bcg_solve_multi(bh.data(), xh.data(), (int64_t)n, (int32_t)k, (int64_t)ld, a.handle(), jac ? pc.device_handle() : nullptr, &p, st.data(),
                                    code.data(), hist.data(), (int64_t)cap, len.data()));
        for (size_t j = 0; j < k; ++j) {
            REQUIRE(codes[j] == KRYST_OK && code[j] == KRYST_OK && stats[j].converged);
            REQUIRE(stats[j].iterations == (size_t)st[j].iterations && stats[j].iterations == stats[0].iterations && stats[j].iterations < 100);
            REQUIRE(std::memcmp(&stats[j].final_residual, &st[j].final_residual, sizeof(double)) == 0);
            REQUIRE((size_t)len[j] == stats[j].iterations + 1 && s.residual_histories[j].size() == (size_t)len[j]);
            REQUIRE(same_bits(s.residual_histories[j], Vec(hist.begin() + (long)(j * cap), hist.begin() + (long)(j * cap + (size_t)len[j]))));
            const Vec xj = x.column(j);
            REQUIRE(same_bits(xj, Vec(xh.begin() + (long)(j * ld), xh.begin() + (long)(j * ld + n))));
            Vec ax(n, 0.0);
            a.spmv(xj, ax);
            double rr = 0.0, bb = 0.0;
            for (size_t i = 0; i < n; ++i) { rr += (bs[j][i] - ax[i]) * (bs[j][i] - ax[i]); bb += bs[j][i] * bs[j][i]; }
            REQUIRE(std::sqrt(rr) <= 2e-10 * std::sqrt(bb));            // (the diagonal varies by 0.2 %: the M^-1 norm and the 2-norm nearly agree)
        }
    }
    {   // dependent right-hand sides: one code for the block, X untouched
        std::vector<Vec> dup = bs;
        dup[3] = dup[1];
        MultiVec b = MultiVec::from_columns(dup), x(n, k);
        BlockCgSolver s(1e-10, 100);
        std::vector<SolveStats<double>> stats;
        const std::vector<int32_t> codes = s.solve_block(a, nullptr, b, x, stats);
        for (size_t j = 0; j < k; ++j) {
            REQUIRE(codes[j] == KRYST_SOLVE_ERROR && stats[j].iterations == 0 && !stats[j].converged);
            REQUIRE(same_bits(x.column(j), Vec(n, 0.0)));
        }
    }
    {   // a single right-hand side has no block form
        BlockCgSolver s(1e-10, 100);
        Vec x(n, 0.0);
        bool threw = false;
        try { s.solve(a, nullptr, bs[0], x); } catch (const KError& e) { threw = e.code == KRYST_UNSUPPORTED; }
        REQUIRE(threw);
    }
    std::printf("CPP_BLOCK_CG_MIRROR_OK\n");
    return 0;
}
