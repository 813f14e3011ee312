// The reference's two direct-solver tests (src/solver/direct_lu.rs:150-192) re-encoded against the C++ mirror (include/kryst_hip.hpp),
// plus solve_cached and the dense matvec on the same system.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "kryst_hip.hpp"

using namespace kryst;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
    // [[2,1,1],[1,3,2],[1,0,0]] x = [4,5,6], true solution [6,15,-23]; column-major like DenseMatrix::from_raw
    const Vec data = {2.0, 1.0, 1.0, 1.0, 3.0, 0.0, 1.0, 2.0, 0.0};
    const Vec b = {4.0, 5.0, 6.0}, expected = {6.0, 15.0, -23.0};
    const double tol = 1e-10;
    HipDenseMatrix a = HipDenseMatrix::from_raw(3, 3, data);
    REQUIRE(a.nrows() == 3 && a.ncols() == 3 && a.to_raw() == data);
    {   // lu_solver_solves_dense_system
        Vec x(3, 0.0);
        LuSolver solver;
        const SolveStats<double> stats = solver.solve(a, nullptr, b, x);
        for (size_t i = 0; i < 3; ++i) REQUIRE(std::fabs(x[i] - expected[i]) < tol);
        REQUIRE(stats.converged && stats.iterations == 1 && stats.final_residual == 0.0);
        Vec y(3, 0.0);
        solver.solve_cached(b, y);
        REQUIRE(y == x);
    }
    {   // qr_solver_solves_dense_system
        Vec x(3, 0.0);
        QrSolver solver;
        const SolveStats<double> stats = solver.solve(a, nullptr, b, x);
        for (size_t i = 0; i < 3; ++i) REQUIRE(std::fabs(x[i] - expected[i]) < tol);
        REQUIRE(stats.converged);
    }
    {   // MatVec: A [6,15,-23] = [4,5,6] exactly (small integers)
        Vec y(3, 0.0);
        a.matvec(expected, y);
        REQUIRE(y == b);
    }
    {   // solve_cached before any factorization: SolveError where the reference panics
        LuSolver fresh;
        Vec y(3, 0.0);
        bool threw = false;
        try { fresh.solve_cached(b, y); } catch (const KError& e) { threw = e.code == KRYST_SOLVE_ERROR; }
        REQUIRE(threw);
    }
    std::printf("CPP_DENSE_MIRROR_OK\n");
    return 0;
}
