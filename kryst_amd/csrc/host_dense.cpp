// Host twins of the dense direct solvers (LuSolver / QrSolver, src/solver/direct_lu.rs): the loops of DESIGN.md section 4.12 exactly as
// stated, on plain host arrays -- no device, no context.  Column-major, every operation rounded on its own (the library is built with
// -ffp-contract=off).  dense.hip computes the same bits on the device.
#include "dense.h"
#include <cmath>

using namespace kr;

namespace {

bool all_finite(const double* a, int64_t count) {
    for (int64_t e = 0; e < count; ++e)
        if (!std::isfinite(a[e])) return false;
    return true;
}

// backward column sweep on the upper triangle of f (column-major, n x n), j descending: y_j = y_j / U[j][j], then y_i -= U[i][j] y_j for i < j
void back_sweep(int64_t n, const double* f, double* y) {
    for (int64_t j = n - 1; j >= 0; --j) {
        y[j] = y[j] / f[j + j * n];
        const double yj = y[j];
        for (int64_t i = 0; i < j; ++i) y[i] = y[i] - f[i + j * n] * yj;
    }
}

}  // namespace

extern "C" {

int32_t kryst_host_dense_lu(int64_t nrows, int64_t ncols, const double* a, int64_t* row_perm, int64_t* col_perm, double* factors) {
    KR_ARG(nrows >= 0 && ncols >= 0 && (a || nrows * ncols == 0) && row_perm && col_perm && factors, "host_dense_lu");
    KR_ARG(nrows == ncols, "host_dense_lu: square matrix required");
    const int64_t n = nrows;
    if (!all_finite(a, n * n)) { set_error("dense LU: the matrix holds a NaN or Inf"); return KRYST_FACTOR_ERROR; }
    std::vector<double> w(a, a + n * n);
    std::vector<int64_t> rp((size_t)n), cp((size_t)n);
    for (int64_t i = 0; i < n; ++i) rp[(size_t)i] = cp[(size_t)i] = i;
    for (int64_t s = 0; s < n; ++s) {
        // row by row, a later entry replaces the current one only if strictly greater
        int64_t p = s, q = s;
        double best = std::fabs(w[s + s * n]);
        for (int64_t i = s; i < n; ++i)
            for (int64_t j = s; j < n; ++j) {
                const double v = std::fabs(w[i + j * n]);
                if (v > best) { best = v; p = i; q = j; }
            }
        const double piv = w[p + q * n];
        if (piv == 0.0) {
            set_error("dense LU: zero pivot at step %lld", (long long)s); set_error_row(s);
            return KRYST_ZERO_PIVOT;
        }
        if (!std::isfinite(piv)) { set_error("dense LU: non-finite pivot at step %lld", (long long)s); return KRYST_FACTOR_ERROR; }
        if (p != s) {
            for (int64_t j = 0; j < n; ++j) std::swap(w[s + j * n], w[p + j * n]);
            std::swap(rp[(size_t)s], rp[(size_t)p]);
        }
        if (q != s) {
            for (int64_t i = 0; i < n; ++i) std::swap(w[i + s * n], w[i + q * n]);
            std::swap(cp[(size_t)s], cp[(size_t)q]);
        }
        const double d = w[s + s * n];
        for (int64_t i = s + 1; i < n; ++i) w[i + s * n] = w[i + s * n] / d;
        for (int64_t j = s + 1; j < n; ++j) {
            const double u = w[s + j * n];
            for (int64_t i = s + 1; i < n; ++i) w[i + j * n] = w[i + j * n] - w[i + s * n] * u;
        }
    }
    for (int64_t e = 0; e < n * n; ++e) factors[e] = w[(size_t)e];
    for (int64_t i = 0; i < n; ++i) { row_perm[i] = rp[(size_t)i]; col_perm[i] = cp[(size_t)i]; }
    return KRYST_OK;
}

// b and x may be the same array
int32_t kryst_host_dense_lu_solve(int64_t n, const int64_t* row_perm, const int64_t* col_perm, const double* factors, const double* b, double* x) {
    KR_ARG(n >= 0 && ((row_perm && col_perm && factors && b && x) || n == 0), "host_dense_lu_solve");
    for (int64_t i = 0; i < n; ++i)
        KR_ARG(row_perm[i] >= 0 && row_perm[i] < n && col_perm[i] >= 0 && col_perm[i] < n, "host_dense_lu_solve: permutation entry out of range");
    std::vector<double> y((size_t)n);
    for (int64_t i = 0; i < n; ++i) y[(size_t)i] = b[row_perm[i]];
    for (int64_t j = 0; j < n; ++j) {
        const double yj = y[(size_t)j];
        for (int64_t i = j + 1; i < n; ++i) y[(size_t)i] = y[(size_t)i] - factors[i + j * n] * yj;
    }
    back_sweep(n, factors, y.data());
    for (int64_t j = 0; j < n; ++j) x[col_perm[j]] = y[(size_t)j];
    return KRYST_OK;
}

// b and x may be the same array; x is written only when the factorization went through
int32_t kryst_host_dense_qr_solve(int64_t nrows, int64_t ncols, const double* a, const double* b, double* x) {
    KR_ARG(nrows >= 0 && ncols >= 0 && ((a && b && x) || nrows * ncols == 0), "host_dense_qr_solve");
    KR_ARG(nrows == ncols, "host_dense_qr_solve: square matrix required");
    const int64_t n = nrows;
    if (!all_finite(a, n * n)) { set_error("dense QR: the matrix holds a NaN or Inf"); return KRYST_FACTOR_ERROR; }
    std::vector<double> w(a, a + n * n), c(b, b + n), v((size_t)n);
    for (int64_t s = 0; s < n; ++s) {
        double ss = 0.0;
        for (int64_t i = s; i < n; ++i) ss = ss + w[i + s * n] * w[i + s * n];
        const double nrm = std::sqrt(ss);
        if (nrm == 0.0) { set_error("dense QR: zero column at step %lld", (long long)s); set_error_row(s); return KRYST_ZERO_PIVOT; }
        const double alpha = (w[s + s * n] >= 0.0) ? -nrm : nrm;
        for (int64_t i = s; i < n; ++i) v[(size_t)i] = w[i + s * n];
        v[(size_t)s] = w[s + s * n] - alpha;
        double vv = 0.0;
        for (int64_t i = s; i < n; ++i) vv = vv + v[(size_t)i] * v[(size_t)i];
        if (vv == 0.0) { set_error("dense QR: zero reflector at step %lld", (long long)s); set_error_row(s); return KRYST_ZERO_PIVOT; }
        for (int64_t j = s + 1; j <= n; ++j) {                      // j == n: the right-hand side as one more column
            double* col = (j < n) ? &w[j * n] : c.data();
            double t = 0.0;
            for (int64_t i = s; i < n; ++i) t = t + v[(size_t)i] * col[i];
            t = (2.0 * t) / vv;
            for (int64_t i = s; i < n; ++i) col[i] = col[i] - v[(size_t)i] * t;
        }
        w[s + s * n] = alpha;
    }
    back_sweep(n, w.data(), c.data());
    for (int64_t i = 0; i < n; ++i) x[i] = c[(size_t)i];
    return KRYST_OK;
}

}  // extern "C"
