// The scalar steps of block CG (Dubrulle's retooled block CG, BCGrQ, with the thin QR done as a Cholesky-QR of a K x K Gram matrix): everything
// that happens on K x K matrices between two passes over the multivectors.  Plain C++ with no device type and no HIP call: thread 0 of
// fold_block_kernel (block_cg.hip) runs it on the folded Gram matrix, and kryst_host_bcg_step runs the same code on the host, which is how the
// CPU tier compares it bit for bit with the numpy restatement (tests/block_cg_ref.py).
//
// The iteration (multivectors n x K, d = the Jacobi inv_diag or nothing):
//   init  R = B - A X;  C = chol(Gram(R, R, d));  Q = R C^-1;  S = d Q  (or S = Q);  res0_j = sqrt(sum_{l <= j} C[l][j]^2)
//   it    T = A S;  U = chol(Gram(S, T));  Gamma = U^-1 U^-T;  M1 = Gamma C
//         X = X + S M1;  Qn = Q - T Gamma;  Phi = chol(Gram(Qn, Qn, d));  C <- Phi C;  res_j as above
//         Q = Qn Phi^-1;  S = d Q + S Phi^T
// The residual block is R = Q C throughout, so C^T (Q^T D Q) C = C^T C is its Gram matrix and res_j, the 2-norm of column j of C, is in exact
// arithmetic ||r_j||_2 without a preconditioner and ||r_j|| in the M^-1 norm (sqrt(r^T D r)) with Jacobi.
//
// THE OPERATION ORDER (pinned bit for bit by the tests; every product and every sum is a separate rounding, -ffp-contract=off).  All matrices
// are K x K, row major with stride K: M[a][b] = m[a * K + b].  "from 0.0, l ascending" means  s = 0.0; s = s + term_l  for l in that order.
//   chol(G) -> upper U with U^T U = G.  Only the upper triangle of G is read.  For j ascending:
//       s = G[j][j];  s = s - U[l][j] * U[l][j]  for l = 0 .. j-1 ascending;  the pivot rule (below);  U[j][j] = sqrt(s);
//       for i = j+1 .. K-1 ascending:  t = G[j][i];  t = t - U[l][j] * U[l][i]  for l = 0 .. j-1 ascending;  U[j][i] = t / U[j][j].
//       The strictly lower triangle of U is written as 0.0.
//   inverse of an upper triangular U -> upper V, by back substitution, column by column, j ascending:
//       V[j][j] = 1.0 / U[j][j];  for i = j-1 down to 0:  s from 0.0, s = s + U[i][l] * V[l][j] for l = i+1 .. j ascending;  V[i][j] = (0.0 - s) / U[i][i].
//       The strictly lower triangle of V is written as 0.0.
//   Gamma = V V^T for a <= b:  from 0.0, Gamma[a][b] = sum_{l = b .. K-1} V[a][l] * V[b][l], l ascending;  Gamma[b][a] = Gamma[a][b].
//   M1 = Gamma C (C upper):  from 0.0, M1[a][j] = sum_{l = 0 .. j} Gamma[a][l] * C[l][j], l ascending.
//   Phi C (both upper):  from 0.0, (Phi C)[a][j] = sum_{l = a .. j} Phi[a][l] * C[l][j], l ascending, for a <= j;  0.0 below the diagonal.
//   res_j:  from 0.0, s = sum_{l = 0 .. j} C[l][j] * C[l][j], l ascending;  res_j = sqrt(s).
//
// THE PIVOT RULE, on pivot j of a chol with g = G[j][j] and s as above (KRYST_BCG_RANK_TOL = 2^-26):
//   Gram of S against T (BCG_GRAM_ST):  !(g > 0) or !(s > 0) -- that is g <= 0, s <= 0 or a NaN anywhere, since a NaN of G reaches a later s --
//       is KRYST_INDEFINITE_MATRIX; else !(s > RANK_TOL * g) is KRYST_SOLVE_ERROR.
//   a residual Gram, weighted or not (BCG_GRAM_RES):  g < 0 is KRYST_INDEFINITE_PRECONDITIONER; else !(s > RANK_TOL * g) is KRYST_SOLVE_ERROR:
//       dependent or zero columns, n < K, a column that converged exactly, a NaN.
// A healthy run keeps s / g far above the constant (the CPU tier asserts >= 0.05 on its fixtures): it only separates such runs from rank loss.
// The factorisation stops at the first pivot that fails; what it wrote up to there is not used.
#pragma once
#include <cstdint>
#include "../../include/kryst_hip.h"

#if defined(__HIPCC__)
#define KR_HD __host__ __device__
#else
#define KR_HD
#endif

// KRYST_BCG_RANK_TOL = 2^-26 is a documented constant of the interface: include/kryst_hip.h defines it

namespace kr {

enum { BCG_GRAM_RES = 0, BCG_GRAM_ST = 1 };
enum { BCG_STEP_INIT = 0, BCG_STEP_ALPHA = 1, BCG_STEP_BETA = 2 };

KR_HD inline int32_t bcg_chol(int k, const double* g, double* u, int gram_kind) {
    for (int j = 0; j < k; ++j) {
        const double gjj = g[j * k + j];
        double s = gjj;
        for (int l = 0; l < j; ++l) s = s - u[l * k + j] * u[l * k + j];
        if (gram_kind == BCG_GRAM_ST) {
            if (!(gjj > 0.0) || !(s > 0.0)) return KRYST_INDEFINITE_MATRIX;
        } else if (gjj < 0.0) {
            return KRYST_INDEFINITE_PRECONDITIONER;
        }
        if (!(s > KRYST_BCG_RANK_TOL * gjj)) return KRYST_SOLVE_ERROR;
        const double ujj = __builtin_sqrt(s);
        u[j * k + j] = ujj;
        for (int i = j + 1; i < k; ++i) {
            double t = g[j * k + i];
            for (int l = 0; l < j; ++l) t = t - u[l * k + j] * u[l * k + i];
            u[j * k + i] = t / ujj;
        }
        for (int i = 0; i < j; ++i) u[j * k + i] = 0.0;
    }
    return KRYST_OK;
}

KR_HD inline void bcg_upper_inverse(int k, const double* u, double* v) {
    for (int j = 0; j < k; ++j) {
        v[j * k + j] = 1.0 / u[j * k + j];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int l = i + 1; l <= j; ++l) s = s + u[i * k + l] * v[l * k + j];
            v[i * k + j] = (0.0 - s) / u[i * k + i];
        }
        for (int i = j + 1; i < k; ++i) v[i * k + j] = 0.0;
    }
}

KR_HD inline void bcg_gamma(int k, const double* v, double* gam) {
    for (int a = 0; a < k; ++a)
        for (int b = a; b < k; ++b) {
            double s = 0.0;
            for (int l = b; l < k; ++l) s = s + v[a * k + l] * v[b * k + l];
            gam[a * k + b] = s;
            gam[b * k + a] = s;
        }
}

// out = Gamma C, C upper; out may not alias either
KR_HD inline void bcg_full_times_upper(int k, const double* gam, const double* c, double* out) {
    for (int a = 0; a < k; ++a)
        for (int j = 0; j < k; ++j) {
            double s = 0.0;
            for (int l = 0; l <= j; ++l) s = s + gam[a * k + l] * c[l * k + j];
            out[a * k + j] = s;
        }
}

// out = Phi C, both upper; out may not alias either
KR_HD inline void bcg_upper_times_upper(int k, const double* phi, const double* c, double* out) {
    for (int a = 0; a < k; ++a)
        for (int j = 0; j < k; ++j) {
            double s = 0.0;
            for (int l = a; l <= j; ++l) s = s + phi[a * k + l] * c[l * k + j];
            out[a * k + j] = s;
        }
}

KR_HD inline void bcg_column_norms(int k, const double* c, double* res) {
    for (int j = 0; j < k; ++j) {
        double s = 0.0;
        for (int l = 0; l <= j; ++l) s = s + c[l * k + j] * c[l * k + j];
        res[j] = __builtin_sqrt(s);
    }
}

// One scalar step.  g: the folded Gram matrix (upper triangle read).  c: C, written by INIT, read by ALPHA, replaced by BETA.  out1 / out2:
//   INIT   C = chol(g, RES);  out1 = C^-1;                        res = res0
//   ALPHA  U = chol(g, ST);   out1 = Gamma;  out2 = M1 = Gamma C
//   BETA   Phi = chol(g, RES) -> out1;  out2 = Phi^-1;  C <- Phi C;  res
// w: 2 K^2 doubles of working storage.  Returns KRYST_OK or the pivot rule's code; on a code nothing but w and (INIT: c, BETA: out1) has been
// written.
KR_HD inline int32_t bcg_step(int step, int k, const double* g, double* c, double* out1, double* out2, double* res, double* w) {
    const int kk = k * k;
    if (step == BCG_STEP_INIT) {
        const int32_t rc = bcg_chol(k, g, c, BCG_GRAM_RES);
        if (rc != KRYST_OK) return rc;
        bcg_upper_inverse(k, c, out1);
        bcg_column_norms(k, c, res);
        return KRYST_OK;
    }
    if (step == BCG_STEP_ALPHA) {
        double* u = w; double* v = w + kk;
        const int32_t rc = bcg_chol(k, g, u, BCG_GRAM_ST);
        if (rc != KRYST_OK) return rc;
        bcg_upper_inverse(k, u, v);
        bcg_gamma(k, v, out1);
        bcg_full_times_upper(k, out1, c, out2);
        return KRYST_OK;
    }
    const int32_t rc = bcg_chol(k, g, out1, BCG_GRAM_RES);
    if (rc != KRYST_OK) return rc;
    bcg_upper_inverse(k, out1, out2);
    bcg_upper_times_upper(k, out1, c, w);
    for (int e = 0; e < kk; ++e) c[e] = w[e];
    bcg_column_norms(k, c, res);
    return KRYST_OK;
}

}  // namespace kr
