// Extreme eigenvalues of a symmetric tridiagonal matrix by bisection with Sturm counts: host only -- no device,
// no context -- every operation rounded on its own (the library is built with -ffp-contract=off).  kryst_spectrum_estimate (cheb_poly.hip)
// feeds it the Lanczos coefficients; tests/cheb_poly_ref.py restates it operation by operation.
#include "common.h"
#include <cfloat>
#include <cmath>

namespace kr {

namespace {

// the number of eigenvalues below x: the negative pivots of the LDL^T factorisation of T - x I; a pivot smaller than pivmin counts as -pivmin
int sturm_count(const double* a, const double* b, int k, double pivmin, double x) {
    int c = 0;
    double q = a[0] - x;
    if (std::fabs(q) < pivmin) q = -pivmin;
    if (q < 0.0) ++c;
    for (int i = 1; i < k; ++i) {
        q = (a[i] - x) - (b[i - 1] * b[i - 1]) / q;
        if (std::fabs(q) < pivmin) q = -pivmin;
        if (q < 0.0) ++c;
    }
    return c;
}

// halve [lo, hi] until the midpoint is one of its ends: count(lo) < want <= count(hi) throughout
void bisect(const double* a, const double* b, int k, double pivmin, int want, double& lo, double& hi) {
    for (;;) {
        const double mid = lo * 0.5 + hi * 0.5;
        if (!(mid > lo && mid < hi)) return;
        if (sturm_count(a, b, k, pivmin, mid) >= want) hi = mid; else lo = mid;
    }
}

}  // namespace

// k x k, diagonal alpha[0..k), off-diagonal beta[0..k-1): *tmin = the LOWER end of the final bracket of the smallest eigenvalue, *tmax = the UPPER
// end of that of the largest (k == 1: alpha[0] itself; an entry that is not finite: NaN for both)
void tridiag_extreme_eigs(const double* alpha, const double* beta, int k, double* tmin, double* tmax) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(alpha[i]) || (i + 1 < k && !std::isfinite(beta[i]))) { *tmin = *tmax = std::nan(""); return; }
    if (k == 1) { *tmin = *tmax = alpha[0]; return; }
    // Gershgorin interval of T, widened so that the counts at its ends are 0 and k whatever the rounding (as LAPACK's dstebz does)
    double gl = 0.0, gu = 0.0, bmax = 0.0;
    for (int i = 0; i < k; ++i) {
        const double off = (i > 0 ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(beta[i]) : 0.0);
        const double l = alpha[i] - off, u = alpha[i] + off;
        if (i == 0 || l < gl) gl = l;
        if (i == 0 || u > gu) gu = u;
        if (i + 1 < k) { const double bb = beta[i] * beta[i]; if (bb > bmax) bmax = bb; }
    }
    const double pivmin = DBL_MIN * (bmax > 1.0 ? bmax : 1.0);
    const double tnorm = std::fabs(gl) > std::fabs(gu) ? std::fabs(gl) : std::fabs(gu);
    const double widen = (2.0 * tnorm) * DBL_EPSILON * (double)k + 2.0 * pivmin;
    gl = gl - widen;
    gu = gu + widen;
    double lo = gl, hi = gu;
    bisect(alpha, beta, k, pivmin, 1, lo, hi);
    *tmin = lo;
    lo = gl; hi = gu;
    bisect(alpha, beta, k, pivmin, k, lo, hi);
    *tmax = hi;
}

}  // namespace kr

extern "C" int32_t kryst_host_tridiag_extreme_eigs(const double* alpha, const double* beta, int32_t k, double* lo, double* hi) {
    KR_ARG(alpha && lo && hi && k >= 1 && k <= 64 && (beta || k == 1), "host_tridiag_extreme_eigs");
    kr::tridiag_extreme_eigs(alpha, beta, k, lo, hi);
    return KRYST_OK;
}
