// The scalar step of block CG (kryst_amd/csrc/bcg_logic.h) as a stand-alone host program, meant to be built with -fsanitize=address,undefined:
// every K x K step on heap buffers of exactly the documented sizes (so that one index past a matrix is a finding), for K = 2, 4, 8, on healthy
// Gram matrices and on each breakdown of the pivot rule, with the algebra checked to rounding: U^T U = G, V = U^-1, Gamma = V V^T, M1 = Gamma C,
// C' = Phi C, res_j = ||C'(:, j)||.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../kryst_amd/csrc/bcg_logic.h"

using namespace kr;

static int fails = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

struct Mat {
    int k; std::unique_ptr<double[]> d;
    explicit Mat(int k_) : k(k_), d(new double[(size_t)k_ * k_]) { for (int e = 0; e < k * k; ++e) d[e] = std::nan(""); }
    double& operator()(int a, int b) { return d[a * k + b]; }
    double operator()(int a, int b) const { return d[a * k + b]; }
};

static Mat spd(int k, std::mt19937_64& gen) {
    std::normal_distribution<double> nd;
    std::vector<double> a((size_t)(k + 3) * k);
    for (double& x : a) x = nd(gen);
    Mat g(k);
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            double s = 0.0;
            for (int r = 0; r < k + 3; ++r) s += a[(size_t)r * k + i] * a[(size_t)r * k + j];
            g(i, j) = s;
        }
    return g;
}

static double max_abs_diff_product(const Mat& a, bool a_t, const Mat& b, bool b_t, const Mat& want) {
    const int k = a.k;
    double worst = 0.0;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            double s = 0.0;
            for (int l = 0; l < k; ++l) s += (a_t ? a(l, i) : a(i, l)) * (b_t ? b(j, l) : b(l, j));
            worst = std::fmax(worst, std::fabs(s - want(i, j)));
        }
    return worst;
}

static void healthy(int k, std::mt19937_64& gen) {
    const Mat g0 = spd(k, gen), g1 = spd(k, gen), g2 = spd(k, gen);
    Mat c(k), o1(k), o2(k);
    std::unique_ptr<double[]> res(new double[k]), w(new double[2 * k * k]);
    double scale = 0.0;
    for (int e = 0; e < k * k; ++e) scale = std::fmax(scale, std::fabs(g0.d[e]));
    const double eps = 1e-9 * scale;

    CHECK(bcg_step(BCG_STEP_INIT, k, g0.d.get(), c.d.get(), o1.d.get(), o2.d.get(), res.get(), w.get()) == KRYST_OK);
    CHECK(max_abs_diff_product(c, true, c, false, g0) < eps);                    // C^T C = G
    Mat eye(k);
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) eye(i, j) = i == j ? 1.0 : 0.0;
    CHECK(max_abs_diff_product(c, false, o1, false, eye) < 1e-9);                // C C^-1 = I
    for (int i = 0; i < k; ++i) for (int j = 0; j < i; ++j) CHECK(c(i, j) == 0.0 && o1(i, j) == 0.0);
    for (int j = 0; j < k; ++j) CHECK(std::fabs(res[j] * res[j] - g0(j, j)) < eps);      // ||C(:, j)||^2 = G[j][j]

    CHECK(bcg_step(BCG_STEP_ALPHA, k, g1.d.get(), c.d.get(), o1.d.get(), o2.d.get(), res.get(), w.get()) == KRYST_OK);
    CHECK(max_abs_diff_product(o1, false, g1, false, eye) < 1e-7);               // Gamma = G^-1
    CHECK(max_abs_diff_product(o1, false, c, false, o2) < 1e-9 * (1.0 + scale)); // M1 = Gamma C
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) CHECK(o1(i, j) == o1(j, i));

    Mat c_old(k);
    for (int e = 0; e < k * k; ++e) c_old.d[e] = c.d[e];
    CHECK(bcg_step(BCG_STEP_BETA, k, g2.d.get(), c.d.get(), o1.d.get(), o2.d.get(), res.get(), w.get()) == KRYST_OK);
    CHECK(max_abs_diff_product(o1, true, o1, false, g2) < 1e-9 * (1.0 + scale)); // Phi^T Phi = G
    CHECK(max_abs_diff_product(o1, false, o2, false, eye) < 1e-9);               // Phi Phi^-1 = I
    CHECK(max_abs_diff_product(o1, false, c_old, false, c) < 1e-9 * (1.0 + scale) * (1.0 + scale));   // C' = Phi C
    for (int j = 0; j < k; ++j) {
        double s = 0.0;
        for (int l = 0; l < k; ++l) s += c(l, j) * c(l, j);
        CHECK(std::fabs(res[j] - std::sqrt(s)) <= 1e-12 * (1.0 + std::sqrt(s)));
    }
}

static int32_t run(int step, const Mat& g, Mat& c) {
    const int k = g.k;
    Mat o1(k), o2(k);
    std::unique_ptr<double[]> res(new double[k]), w(new double[2 * k * k]);
    return bcg_step(step, k, g.d.get(), c.d.get(), o1.d.get(), o2.d.get(), res.get(), w.get());
}

static void breakdowns(int k, std::mt19937_64& gen) {
    Mat c(k);
    {
        Mat g = spd(k, gen);
        CHECK(run(BCG_STEP_INIT, g, c) == KRYST_OK);
    }
    {   // an exactly dependent pair: column k-1 = column 0
        Mat g = spd(k, gen);
        for (int i = 0; i < k; ++i) { g(i, k - 1) = g(i, 0); g(k - 1, i) = g(0, i); }
        g(k - 1, k - 1) = g(0, 0);
        Mat cc(k);
        CHECK(run(BCG_STEP_INIT, g, cc) == KRYST_SOLVE_ERROR);
        CHECK(run(BCG_STEP_BETA, g, c) == KRYST_SOLVE_ERROR);
    }
    {   // a zero column
        Mat g = spd(k, gen);
        for (int i = 0; i < k; ++i) { g(i, 1) = 0.0; g(1, i) = 0.0; }
        Mat cc(k);
        CHECK(run(BCG_STEP_INIT, g, cc) == KRYST_SOLVE_ERROR);
        CHECK(run(BCG_STEP_ALPHA, g, c) == KRYST_INDEFINITE_MATRIX);
    }
    {   // an indefinite Gram matrix of S against T
        Mat g = spd(k, gen);
        for (int e = 0; e < k * k; ++e) g.d[e] = -g.d[e];
        CHECK(run(BCG_STEP_ALPHA, g, c) == KRYST_INDEFINITE_MATRIX);
        Mat h = spd(k, gen);
        h(k - 1, k - 1) = -h(k - 1, k - 1);
        CHECK(run(BCG_STEP_ALPHA, h, c) == KRYST_INDEFINITE_MATRIX);
        Mat nn = spd(k, gen);
        nn(0, k - 1) = std::nan("");
        CHECK(run(BCG_STEP_ALPHA, nn, c) == KRYST_INDEFINITE_MATRIX);
    }
    {   // a negative diagonal entry of a weighted residual Gram matrix
        Mat g = spd(k, gen);
        g(k - 1, k - 1) = -1.0;
        Mat cc(k);
        CHECK(run(BCG_STEP_INIT, g, cc) == KRYST_INDEFINITE_PRECONDITIONER);
        CHECK(run(BCG_STEP_BETA, g, c) == KRYST_INDEFINITE_PRECONDITIONER);
        Mat nn = spd(k, gen);
        nn(0, 0) = std::nan("");
        CHECK(run(BCG_STEP_BETA, nn, c) == KRYST_SOLVE_ERROR);
    }
}

int main() {
    std::mt19937_64 gen(20250101);
    const int widths[3] = {2, 4, 8};
    for (int k : widths) {
        for (int rep = 0; rep < 50; ++rep) healthy(k, gen);
        for (int rep = 0; rep < 10; ++rep) breakdowns(k, gen);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("bcg logic ok\n");
    return 0;
}
