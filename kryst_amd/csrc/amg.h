// AMG (src/preconditioner/amg.rs): the host set-up of the hierarchy as written (amg_setup.cpp) and the device hierarchy the
// V-cycle runs on (amg.hip).
#pragma once
#include <cstdint>
#include <vector>

namespace kr {

// one host CSR: rows in ascending column order, int64 row pointers
struct HostCsr {
    int64_t nrows = 0, ncols = 0;
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> col;
    std::vector<double> val;
    int64_t nnz() const { return (int64_t)col.size(); }
};

// AMGLevel (amg.rs:55-64): A_l (the field the reference calls coarse_matrix holds the level's OWN operator, :99), D_l^-1, and for every
// level but the last P_l (n_l x n_{l+1}, smoothed and row-normalised) and R_l = P0_l^T (n_{l+1} x n_l, the UNsmoothed P0, :135).
// The last level carries identity P / R in the reference (:107-112), which the V-cycle never reads: here they are left empty.
struct AmgHostLevel {
    HostCsr a, p, r;
    std::vector<double> dinv;
    std::vector<int32_t> agg;     // aggregate of every row (empty on the last level)
    double threshold = 0;         // the adaptive threshold the level was coarsened with (:83)
};

// the default fill budget of one level: every matrix the set-up forms for a coarse level (R*A, A_c = R*A*P, P) may hold at most
// max(KR_AMG_FILL_FACTOR * nnz(A_0), KR_AMG_FILL_MIN) entries
constexpr int64_t KR_AMG_FILL_FACTOR = 8;
constexpr int64_t KR_AMG_FILL_MIN = 1 << 16;

// AMG::new(a, max_levels, base_threshold) (amg.rs:73-118) on host CSR rows (strictly ascending columns per row, n x n).
// level_budget <= 0: the default budget above.  KRYST_FACTOR_ERROR (with the level in the message) when a level would exceed it.
int32_t amg_setup_as_written(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t max_levels,
                             double base_threshold, int64_t level_budget, std::vector<AmgHostLevel>& levels);

}  // namespace kr
