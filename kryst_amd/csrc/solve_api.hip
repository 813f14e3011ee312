// The solve entry points of the C API: LinearSolver::solve (src/solver/mod.rs:30-52) on host slices and on device vectors for every
// method, and the stepping session.  The solvers themselves are in cg_pcg.hip, bicgstab.hip, cgs_tfqmr.hip, minres_qmr_cgnr.hip and the
// restarted units (solvers.h).
#include "solvers.h"

using namespace kr;

// host-slice entry points: upload b and the initial guess, solve on the device, download x
template <class F>
static int32_t host_solve(const double* b, double* x, int64_t n, const SolveIO& io, F f) {
    KR_ARG(io.a && b && x, "solve: null argument");
    KR_ARG(n == io.a->nrows, "solve: b.len() != nrows");
    kryst_vec_t bv = nullptr, xv = nullptr;
    KR_TRY(kryst_vec_create(io.a->ctx, n, &bv));
    int32_t rc = kryst_vec_create(io.a->ctx, n, &xv);
    if (rc == KRYST_OK) rc = kryst_vec_upload(bv, b, n);
    if (rc == KRYST_OK) rc = kryst_vec_upload(xv, x, n);
    if (rc == KRYST_OK) {
        rc = f(bv, xv, io);
        if (rc == KRYST_OK) { int32_t rd = kryst_vec_download(xv, x, n); if (rd != KRYST_OK) rc = rd; }
    }
    kryst_vec_destroy(bv); kryst_vec_destroy(xv);
    return rc;
}

#define IO_FROM_ARGS SolveIO io{a, pc, params, stats, hist, hist_cap, hist_len, monitor, user}

// A solve whose preconditioner had to switch kernels mid-way (pc.h: pc_health) is repeated once from the caller's x: on an
// error the solvers never touch x, like the reference (monitor callbacks then start over).
template <class F>
static int32_t retry_on_pc_fallback(kryst_pc_t pc, F f) {
    int32_t rc = f();
    if (rc == KRYST_SOLVE_ERROR && pc_fell_back(pc)) rc = f();
    return rc;
}

struct kryst_session_s { SolverRun* run; };

extern "C" {

int32_t kryst_session_begin(int32_t method, kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_pc_t pc,
                            const kryst_params_t* params, kryst_session_t* out) {
    KR_ARG(a && params && b && x && out, "session_begin: null argument");
    SolveIO io{a, pc, params, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
    SolverRun* run = nullptr;
    switch (method) {
        case 0: run = make_cg_run(b, x, io); break;
        case 1: run = make_pcg_run(b, x, io); break;
        case 2: run = make_bicgstab_run(b, x, io); break;
        case 3: run = make_cgs_run(b, x, io); break;
        case 4: run = make_tfqmr_run(b, x, io); break;
        case 5: run = make_minres_run(b, x, io, false); break;
        case 6: run = make_qmr_run(b, x, io); break;
        case 7: run = make_cgnr_run(b, x, io, false); break;
        case 8: run = make_minres_run(b, x, io, true); break;
        case 9: run = make_cgnr_run(b, x, io, true); break;
        default: set_error("session_begin: unknown method %d", method); return KRYST_ERR_ARG;
    }
    const int32_t rc = run->begin();
    if (rc != KRYST_OK) { delete run; return rc; }
    *out = new kryst_session_s{run};
    return KRYST_OK;
}

int32_t kryst_session_step(kryst_session_t s, int64_t k) {
    KR_ARG(s && s->run && k >= 0, "session_step");
    return s->run->step(k);
}

int32_t kryst_session_end(kryst_session_t s, kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len) {
    KR_ARG(s && s->run, "session_end");
    s->run->io.stats = stats; s->run->io.hist = hist; s->run->io.hist_cap = hist_cap; s->run->io.hist_len = hist_len;
    const int32_t rc = s->run->end();
    delete s->run;
    delete s;
    return rc;
}

int32_t kryst_cg_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return cg_solve(b, x, io); }
int32_t kryst_pcg_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return pcg_solve(b, x, io); }); }
int32_t kryst_gmres_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return gmres_solve(b, x, io); }); }
int32_t kryst_cgs_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return cgs_solve(b, x, io); }
int32_t kryst_tfqmr_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return tfqmr_solve(b, x, io); }
int32_t kryst_cgs_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return cgs_solve(bv, xv, i); });
}
int32_t kryst_tfqmr_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return tfqmr_solve(bv, xv, i); });
}
int32_t kryst_minres_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return minres_solve(b, x, io, false); }
int32_t kryst_qmr_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return qmr_solve(b, x, io); }
int32_t kryst_cgnr_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return cgnr_solve(b, x, io, false); }
int32_t kryst_minres_textbook_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return minres_solve(b, x, io, true); }
int32_t kryst_cgnr_textbook_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return cgnr_solve(b, x, io, true); }
int32_t kryst_minres_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return minres_solve(bv, xv, i, false); });
}
int32_t kryst_qmr_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return qmr_solve(bv, xv, i); });
}
int32_t kryst_cgnr_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return cgnr_solve(bv, xv, i, false); });
}
int32_t kryst_fgmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t orthog, double haptol, int32_t preallocate, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return fgmres_solve(b, x, io, orthog, haptol, preallocate); });
}
int32_t kryst_fgmres_solve(const double* b, double* x, int64_t n, int32_t orthog, double haptol, int32_t preallocate, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS;
    return host_solve(b, x, n, io, [=](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return retry_on_pc_fallback(i.pc, [&] { return fgmres_solve(bv, xv, i, orthog, haptol, preallocate); }); });
}
int32_t kryst_bicgstab_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return bicgstab_solve(b, x, io, false); }
int32_t kryst_bicgstab_rpc_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS) { IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return bicgstab_solve(b, x, io, true); }); }

int32_t kryst_cg_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return cg_solve(bv, xv, i); });
}
int32_t kryst_pcg_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return retry_on_pc_fallback(i.pc, [&] { return pcg_solve(bv, xv, i); }); });
}
int32_t kryst_pca_gmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return pca_gmres_solve(b, x, io, block_size, pipeline_depth, tau, false); });
}
int32_t kryst_pca_gmres_solve(const double* b, double* x, int64_t n, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS;
    return host_solve(b, x, n, io, [=](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) {
        return retry_on_pc_fallback(i.pc, [&] { return pca_gmres_solve(bv, xv, i, block_size, pipeline_depth, tau, false); }); });
}
int32_t kryst_pca_gmres_textbook_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return pca_gmres_solve(b, x, io, block_size, pipeline_depth, tau, true); });
}
int32_t kryst_cbgmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t basis, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return retry_on_pc_fallback(pc, [&] { return cbgmres_solve(b, x, basis, io); });
}
int32_t kryst_gmres_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return retry_on_pc_fallback(i.pc, [&] { return gmres_solve(bv, xv, i); }); });
}
int32_t kryst_bicgstab_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
    IO_FROM_ARGS; return host_solve(b, x, n, io, [](kryst_vec_t bv, kryst_vec_t xv, const SolveIO& i) { return bicgstab_solve(bv, xv, i, false); });
}

}  // extern "C"
