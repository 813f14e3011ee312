// The mixed-precision part of the C++ mirror (include/kryst_hip.hpp): HipCsrMatrix32 and RefinementSolver on the reference's 2 x 2 CG case
// (src/solver/cg.rs:310-323) and on a 64-row tridiagonal operator.  The product against a host fold of the contract (DESIGN.md section
// 4.16: widen, fold in fp64 in stored order, round once), bit for bit; the refinement to 1e-12 with and without Jacobi, its fp64 residual
// checked on the host; the refusal of an ILU preconditioner.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

struct HostCsr {
    size_t n; std::vector<size_t> rp, ci; Vec va;
    HipCsrMatrix upload() const { return HipCsrMatrix::from_csr(n, n, rp, ci, va); }
    // y = A x in fp64, the row fold from 0.0 in stored order
    Vec spmv(const Vec& x) const {
        Vec y(n, 0.0);
        for (size_t i = 0; i < n; ++i) { double s = 0.0; for (size_t k = rp[i]; k < rp[i + 1]; ++k) s = s + va[k] * x[ci[k]]; y[i] = s; }
        return y;
    }
    // the fp32 product of the contract: values and operands rounded to fp32 when stored, widened, folded in fp64, rounded once
    std::vector<float> spmv32(const std::vector<float>& x) const {
        std::vector<float> y(n, 0.0f);
        for (size_t i = 0; i < n; ++i) {
            double s = 0.0;
            for (size_t k = rp[i]; k < rp[i + 1]; ++k) s = s + (double)(float)va[k] * (double)x[ci[k]];
            y[i] = (float)s;
        }
        return y;
    }
};

static HostCsr two_by_two() { return {2, {0, 2, 4}, {0, 1, 0, 1}, {4.0, 1.0, 1.0, 3.0}}; }

static HostCsr tridiagonal(size_t n) {
    HostCsr a{n, {0}, {}, {}};
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { a.ci.push_back(i - 1); a.va.push_back(-1.0); }
        a.ci.push_back(i); a.va.push_back(2.5 + 0.1 * (double)(i % 7));          // (0.1 * k is not an fp32 number: the lowering rounds it)
        if (i + 1 < n) { a.ci.push_back(i + 1); a.va.push_back(-1.0); }
        a.rp.push_back(a.ci.size());
    }
    return a;
}

static double norm2(const Vec& v) { double s = 0.0; for (double e : v) s = s + e * e; return std::sqrt(s); }

static int run(const HostCsr& h, const Vec& b) {
    const HipCsrMatrix a = h.upload();
    {   // the lowering and its product
        const HipCsrMatrix32 a32(a);
        int64_t changed = 0;
        for (double v : h.va) changed += (double)(float)v != v;
        const auto info = a32.info();
        REQUIRE(info[0] == changed && info[1] == 0 && info[2] == (int64_t)h.n);
        std::vector<float> x(h.n), y(h.n, NAN);
        for (size_t i = 0; i < h.n; ++i) x[i] = (float)(0.37 * (double)i - 1.3) / 3.0f;
        a32.spmv(x, y);
        const std::vector<float> want = h.spmv32(x);
        REQUIRE(std::memcmp(y.data(), want.data(), h.n * sizeof(float)) == 0);
    }
    for (int jacobi = 0; jacobi < 2; ++jacobi) {
        Jacobi pc;
        if (jacobi) pc.setup(a);
        RefinementSolver s(1e-12, 30);
        s.with_inner(1e-6, 500);
        Vec x(h.n, 0.0);
        const SolveStats<double> st = s.solve(a, jacobi ? &pc : nullptr, b, x);
        REQUIRE(st.converged && st.iterations >= 1 && st.iterations < 30);
        REQUIRE(s.residual_history.size() == st.iterations + 1 && s.inner_iterations.size() == st.iterations);
        REQUIRE(std::fabs(s.residual_history.front() - norm2(b)) <= 1e-14 * norm2(b) && s.residual_history.back() == st.final_residual);
        for (int64_t it : s.inner_iterations) REQUIRE(it >= 1);
        Vec r = h.spmv(x);
        for (size_t i = 0; i < h.n; ++i) r[i] = b[i] - r[i];
        REQUIRE(norm2(r) <= 1e-12 * norm2(b));
    }
    {   // an ILU preconditioner is refused, x untouched
        Ilu0 ilu; ilu.setup(a);
        RefinementSolver s(1e-12, 30);
        Vec x(h.n, 0.25);
        bool threw = false;
        try { s.solve(a, &ilu, b, x); } catch (const KError& e) { threw = e.code == KRYST_UNSUPPORTED; }
        REQUIRE(threw);
        for (double e : x) REQUIRE(e == 0.25);
    }
    return 0;
}

int main() {
    {   // [[4,1],[1,3]] x = [1,2] -> [1/11, 7/11]
        const HostCsr h = two_by_two();
        if (run(h, {1.0, 2.0})) return 1;
        RefinementSolver s(1e-12, 30);
        Vec x{0.0, 0.0};
        s.solve(h.upload(), nullptr, {1.0, 2.0}, x);
        REQUIRE(std::fabs(x[0] - 0.09090909090909091) < 1e-11 && std::fabs(x[1] - 0.6363636363636364) < 1e-11);
    }
    {
        const HostCsr h = tridiagonal(64);
        Vec b(64);
        for (size_t i = 0; i < 64; ++i) b[i] = std::sin(0.7 * (double)i) + 0.2;
        if (run(h, b)) return 1;
    }
    std::printf("CPP_MIXED_MIRROR_OK\n");
    return 0;
}
