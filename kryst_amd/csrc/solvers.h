// What the solver units show each other and the entry points (solve_api.hip): one `*_solve` per method for the one-shot LinearSolver::solve, and
// one `make_*_run` per method a stepping session can drive.
#pragma once
#include "solver_run.h"

namespace kr {

int32_t cg_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);       // cg_pcg.hip
int32_t pcg_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);
int32_t bicgstab_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool right_pc);   // bicgstab.hip
#pragma GCC visibility push(hidden)      // (new with the split of the CG / PCG / BiCGStab unit: the library's dynamic symbol table stays what it was)
SolverRun* make_cg_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
SolverRun* make_pcg_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
SolverRun* make_bicgstab_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
#pragma GCC visibility pop
int32_t gmres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);    // gmres.hip
int32_t cgs_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);      // cgs_tfqmr.hip
int32_t tfqmr_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);
SolverRun* make_cgs_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
SolverRun* make_tfqmr_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
int32_t minres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool textbook);    // minres_qmr_cgnr.hip
int32_t qmr_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io);
int32_t cgnr_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool textbook);
SolverRun* make_minres_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io, bool textbook);
SolverRun* make_qmr_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io);
SolverRun* make_cgnr_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io, bool textbook);
int32_t fgmres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, int32_t orthog, double haptol, int32_t preallocate);   // fgmres.hip
int32_t pca_gmres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, int32_t block_size, int32_t pipeline_depth, double tau,
                        bool textbook);   // pca_gmres.hip
int32_t cbgmres_solve(kryst_vec_t bv, kryst_vec_t xv, int32_t basis, const SolveIO& io);   // gmres_cb.hip

}  // namespace kr
