// The host-side factorisations on plain host arrays (kryst_hip.h: no device, no context): what kryst_pc_ilup / kryst_pc_ilut run between the
// download of the operator's rows and the upload of the factors, for CPU-only callers, for tests against the oracle and for the sanitizer tier
#include "common.h"
#include "host_factor.h"
#include <memory>

using namespace kr;

struct kryst_host_factors_s { kr::FlatRows le, ue; kr::hvec<double> dg; int64_t n = 0; };
static int32_t host_rows_check(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, const char* who) {
    if (n < 0 || !row_ptr || (row_ptr[n] > 0 && (!col || !val)) || row_ptr[0] != 0) { set_error("bad argument: %s", who); return KRYST_ERR_ARG; }
    for (int64_t i = 0; i < n; ++i) if (row_ptr[i + 1] < row_ptr[i]) { set_error("bad argument: %s: row_ptr must not decrease", who); return KRYST_ERR_ARG; }
    for (int64_t k = 0; k < row_ptr[n]; ++k) if (col[k] < 0) { set_error("bad argument: %s: negative column", who); return KRYST_ERR_ARG; }
    return KRYST_OK;
}
extern "C" int32_t kryst_host_ilup(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t fill, int32_t threads, int64_t block,
                                   kryst_host_factors_t* out) {
    KR_ARG(out && fill >= 0, "host_ilup");
    KR_TRY(host_rows_check(n, row_ptr, col, val, "host_ilup"));
    std::unique_ptr<kryst_host_factors_s> F(new kryst_host_factors_s());
    F->n = n;
    IlupOptions opt; opt.threads = threads; opt.block = block > 0 ? block : 2048; opt.cpu_group = 0;
    long long zero_col = -1;
    int hrc = 2;
    try { hrc = host_ilup_rows(n, row_ptr, col, val, fill, opt, F->le, F->ue, F->dg, &zero_col, nullptr); } catch (const std::bad_alloc&) { hrc = 2; }
    if (hrc == 1) { set_error("ILUP: zero diagonal in U at row %lld", zero_col); set_error_row(zero_col); return KRYST_SOLVE_ERROR; }
    if (hrc != 0) { set_error("host_ilup: out of host memory"); return KRYST_ERR_ARG; }
    *out = F.release();
    return KRYST_OK;
}
extern "C" int32_t kryst_host_ilut(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t fill, double droptol, int32_t threads,
                                   kryst_host_factors_t* out) {
    KR_ARG(out && fill >= 0, "host_ilut");
    KR_TRY(host_rows_check(n, row_ptr, col, val, "host_ilut"));
    std::unique_ptr<kryst_host_factors_s> F(new kryst_host_factors_s());
    F->n = n;
    try { host_ilut_rows(n, row_ptr, col, val, fill, droptol, F->le, F->ue, F->dg, threads); } catch (const std::bad_alloc&) { set_error("host_ilut: out of host memory"); return KRYST_ERR_ARG; }
    *out = F.release();
    return KRYST_OK;
}
extern "C" int32_t kryst_host_factors_sizes(kryst_host_factors_t f, int64_t* n, int64_t* nnz_l, int64_t* nnz_u) {
    KR_ARG(f, "host_factors_sizes");
    if (n) *n = f->n;
    if (nnz_l) *nnz_l = f->le.ptr.empty() ? 0 : f->le.ptr[(size_t)f->n];
    if (nnz_u) *nnz_u = f->ue.ptr.empty() ? 0 : f->ue.ptr[(size_t)f->n];
    return KRYST_OK;
}
extern "C" int32_t kryst_host_factors_get(kryst_host_factors_t f, int64_t* l_ptr, int32_t* l_col, double* l_val, int64_t* u_ptr, int32_t* u_col, double* u_val, double* diag) {
    KR_ARG(f, "host_factors_get");
    const size_t n = (size_t)f->n;
    if (l_ptr) std::copy(f->le.ptr.begin(), f->le.ptr.begin() + (std::ptrdiff_t)n + 1, l_ptr);
    if (u_ptr) std::copy(f->ue.ptr.begin(), f->ue.ptr.begin() + (std::ptrdiff_t)n + 1, u_ptr);
    if (l_col) std::copy(f->le.col.begin(), f->le.col.end(), l_col);
    if (l_val) std::copy(f->le.val.begin(), f->le.val.end(), l_val);
    if (u_col) std::copy(f->ue.col.begin(), f->ue.col.end(), u_col);
    if (u_val) std::copy(f->ue.val.begin(), f->ue.val.end(), u_val);
    if (diag) std::copy(f->dg.begin(), f->dg.begin() + (std::ptrdiff_t)n, diag);
    return KRYST_OK;
}
extern "C" int32_t kryst_host_factors_destroy(kryst_host_factors_t f) { delete f; return KRYST_OK; }
extern "C" int32_t kryst_host_levels(int64_t n, const int64_t* ptr, const int32_t* col, int32_t forward, int32_t* level, int32_t* nlevels) {
    KR_ARG(n >= 0 && ptr && level && (ptr[n] == 0 || col), "host_levels");
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k)
            if (col[k] < 0 || col[k] >= n || (forward ? col[k] >= i : col[k] <= i)) { set_error("bad argument: host_levels: row %lld is not strictly %s", (long long)i, forward ? "lower" : "upper"); return KRYST_ERR_ARG; }
    const int32_t nl = host_levels(n, ptr, col, forward != 0, level);
    if (nlevels) *nlevels = nl;
    return KRYST_OK;
}
