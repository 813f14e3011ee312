// Dense storage and the direct solvers (DenseMatrix::from_raw src/matrix/dense.rs:16-25, LuSolver / QrSolver src/solver/direct_lu.rs):
// what dense.hip (device) and host_dense.cpp (host twins) share.  The arithmetic contract is DESIGN.md section 4.12.
#pragma once
#include "common.h"

namespace kr {

constexpr int KR_DENSE_TAIL = 128;      // LU: a trailing block of at most this many rows is finished by one workgroup inside LDS
constexpr int KR_DENSE_TR = 256;        // LU: rows of an update tile (one thread each)
constexpr int KR_DENSE_SWEEP_T = 1024;  // threads of the one-workgroup triangular sweeps: KRYST_DENSE_MAX / 4 columns entries each

// error word of a factorization: code (0: none) and the step that raised it
enum { KR_DENSE_OK = 0, KR_DENSE_ZERO = 1, KR_DENSE_NONFINITE = 2 };

}  // namespace kr

// column-major, d[i + j * nrows]
struct kryst_dense_s {
    kryst_ctx_t ctx = nullptr;
    int64_t nrows = 0, ncols = 0;
    double* d = nullptr;
};
