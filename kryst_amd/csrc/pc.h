// Preconditioner objects (Preconditioner<M,V>, src/preconditioner/mod.rs:8-13).  A kind is one state struct derived from kryst_pc_s,
// defined in the file that implements it; nothing here knows the kinds apart beyond their number.
#pragma once
#include "csr.h"

enum { KR_PC_IDENTITY = 1, KR_PC_JACOBI = 2, KR_PC_ILU = 3, KR_PC_CHEB_STUB = 6, KR_PC_CHEB = 7, KR_PC_SPAI = 9, KR_PC_BLOCK_JACOBI = 10, KR_PC_AMG = 11, KR_PC_ASM = 12, KR_PC_SOR = 13, KR_PC_ASM_ILU = 14, KR_PC_CHEB_POLY = 15 };

struct kryst_pc_s {
    const kryst_ctx_t ctx;
    const int kind;
    const kryst_csr_t a;              // borrowed: the operator the state refers to (nullptr: none)
    const int64_t n;                  // its size; < 0: sizeless (Identity, the Chebyshev stub), any vector length is taken
    kryst_pc_s(kryst_ctx_t ctx_, int kind_, kryst_csr_t a_, int64_t n_) : ctx(ctx_), kind(kind_), a(a_), n(n_) {}
    kryst_pc_s(const kryst_pc_s&) = delete;
    kryst_pc_s& operator=(const kryst_pc_s&) = delete;
    virtual ~kryst_pc_s() {}          // releases exactly what the kind owns; null members are harmless (a half-built object is destroyed too)
    // z <- M^-1 r for vectors of length nv on ctx->s_main (device pointers, padded vectors).  `done`: device flag that turns kernels into no-ops.
    virtual int32_t apply(int64_t nv, const double* r, double* z, const int* done) = 0;
    // Call after the stream has been synchronised: KRYST_OK, or KRYST_SOLVE_ERROR when an apply since the last check was abandoned
    // by the device (the ILU wavefront solve's give-up path, tri_wave.h; a SOR sweep's grid barrier); an ILU has then switched itself
    // to kernels that cannot stall, fell_back() reports that switch once, and the caller repeats the work.
    virtual int32_t health() { return KRYST_OK; }
    virtual bool fell_back() { return false; }
    virtual bool reads_z() const { return false; }          // the apply reads z on entry (AMG as written starts its finest level from the incoming z, amg.rs:211)
    virtual bool check_after_apply() const { return false; }   // a single kryst_pc_apply waits and asks health(): its kernels may give up
};

namespace kr {
inline int32_t pc_apply_dev(kryst_pc_t pc, int64_t n, const double* r, double* z, const int* done) {
    const int32_t rc = pc->apply(n, r, z, done);
    phase_mark(pc->ctx, KR_PH_PC);
    return rc;
}
// pc_apply_dev for solvers whose reference apply gets a FRESH z: z = 0 (init == nullptr; gmres.rs:244, 250, 256, 283, 311, 339) or
// z = init (fgmres.rs:208-210: z_basis[j] = v_basis[j].clone()) first, when the preconditioner reads z; both gated by `done`
int32_t pc_apply_dev_fresh(kryst_pc_t pc, int64_t n, const double* r, double* z, const int* done, const double* init);   // precond.hip
inline int32_t pc_health(kryst_pc_t pc) { return pc ? pc->health() : KRYST_OK; }
inline bool pc_fell_back(kryst_pc_t pc) { return pc && pc->fell_back(); }
inline bool pc_reads_z(kryst_pc_t pc) { return pc && pc->reads_z(); }
// the kind's state behind a handle, or nullptr when the handle is null or of another kind (the *_info / *_export entry points)
template <class T> inline T* pc_cast(kryst_pc_t pc) { return pc && pc->kind == T::KIND ? static_cast<T*>(pc) : nullptr; }
const double* pc_jacobi_inv_diag(kryst_pc_t pc);            // KR_PC_JACOBI only: PCG fuses the Jacobi apply into its residual update
int32_t jacobi_inv_diag_dev(kryst_csr_t a, double* inv_diag);   // Jacobi's inv_diag (jacobi.rs:69-71) into a vector of the operator's rows, on ctx->s_main (precond.hip)
int32_t chebyshev_dev(kryst_csr_t a, const double* r, double* z, double alpha, double beta, int64_t m,
                      double* v0, double* v1, double* v2, const int* done);
}
