// Preconditioner objects (Preconditioner<M,V>, src/preconditioner/mod.rs:8-13).
#pragma once
#include "csr.h"

enum { KR_PC_IDENTITY = 1, KR_PC_JACOBI = 2, KR_PC_ILU = 3, KR_PC_CHEB_STUB = 6, KR_PC_CHEB = 7, KR_PC_SPAI = 9, KR_PC_BLOCK_JACOBI = 10, KR_PC_AMG = 11, KR_PC_ASM = 12, KR_PC_SOR = 13 };

namespace kr { struct AmgDev; }

struct kryst_pc_s {
    kryst_ctx_t ctx = nullptr;
    int kind = 0;
    kryst_csr_t a = nullptr;          // borrowed: the operator the factors refer to
    kryst_csr_t spai_m = nullptr;     // owned: M of a SPAI set-up on the device (spai.hip); pc->a is then M too
    int64_t n = 0;
    double* d_inv_diag = nullptr;     // JACOBI
    // ILU kinds: factor values on A's pattern + level schedule (precond.hip)
    int ilu_mode = 0;
    double* d_lfac = nullptr; double* d_ufac = nullptr;
    int divide_diag = 0;
    int32_t* d_lvl_rows_l = nullptr; int32_t* d_lvl_rows_u = nullptr;   // rows ordered by level
    std::vector<int32_t> lvl_off_l, lvl_off_u;                          // level offsets (host)
    int32_t* d_lvl_off_l = nullptr; int32_t* d_lvl_off_u = nullptr;
    double* d_work = nullptr;
    int32_t* d_sync = nullptr;        // grid-barrier words of the persistent triangular solve
    // Chebyshev
    double cheb_alpha = 0, cheb_beta = 0; int64_t cheb_degree = 0;
    double* d_v0 = nullptr; double* d_v1 = nullptr; double* d_v2 = nullptr;
    // block Jacobi (block_jacobi.hip): the inverted tiles block after block, column-major inside a tile
    int32_t bj_bsize = 0;             // contiguous form: blocks of bj_bsize consecutive rows, the last one shorter; 0: index-set form
    int64_t bj_nblk = 0;
    int64_t bj_uncovered = 0;         // rows in no block (index-set form): z = +0.0 there
    double* d_bj_tile = nullptr;
    int64_t* d_bj_ptr = nullptr; int64_t* d_bj_toff = nullptr;   // index-set form: block offsets into d_bj_idx, tile offsets
    int32_t* d_bj_idx = nullptr;      // index-set form: each block's indices, sorted ascending
    int32_t* d_bj_owner = nullptr;    // index-set form with overlapping blocks or uncovered rows: the last block containing a row, or -1
    std::vector<int64_t> bj_ptr_h; std::vector<int32_t> bj_idx_h;
    kr::AmgDev* amg = nullptr;        // AMG (amg.hip): the levels, their operators and work vectors
    // additive Schwarz (asm.hip): the (grown) subdomains sorted ascending, their tiles block after block (column-major inside a tile), the
    // products X of an apply (one entry per subdomain row) and the row -> positions-in-X map of the combine
    int64_t asm_nsub = 0, asm_total = 0;   // subdomains; sum of their rows
    int32_t asm_maxb = 0;
    double* d_asm_tile = nullptr; int64_t* d_asm_toff = nullptr; double* d_asm_x = nullptr;
    int32_t* d_asm_xoff = nullptr;    // subdomain k's rows: positions [xoff[k], xoff[k + 1]) of d_asm_idx / X
    int32_t* d_asm_posk = nullptr;    // the subdomain of every position
    int32_t* d_asm_idx = nullptr;
    int32_t* d_asm_mptr = nullptr; int32_t* d_asm_mpos = nullptr;
    std::vector<int64_t> asm_ptr_h; std::vector<int32_t> asm_idx_h, asm_owner_h;   // owner: the last un-grown set containing a row, or -1
    // SOR / SSOR (sor.hip): the parameters, 1 / (a_ii + fshift) in d_inv_diag, and per sweep direction (0 forward, 1 backward) the rows
    // ordered by dependency level of the (coloured) sweep order with the level offsets
    double sor_omega = 1.0, sor_fshift = 0.0;
    int32_t sor_its = 1, sor_lits = 1, sor_sym = 0;
    int32_t* d_sor_rows[2] = {nullptr, nullptr}; int32_t* d_sor_off[2] = {nullptr, nullptr};
    int32_t sor_groups[2] = {0, 0}; uint32_t sor_grid[2] = {1, 1};
    int32_t* d_sor_pos = nullptr;     // coloured order: the position of every row, or nullptr (position = row)
    int32_t* d_sor_ent = nullptr;     // coloured order: every row's entries in ascending position, or nullptr (the stored order)
    uint32_t* d_sor_sync = nullptr;   // the arrival counter of the sweep kernel's grid barrier, zeroed in front of every launch
    uint32_t* h_sor_gave_up = nullptr; uint32_t* d_sor_gave_up = nullptr;   // mapped host word: a barrier's patience ran out (sticky until read)
};

namespace kr {
// z <- M^-1 r on ctx->s_main (device pointers, padded vectors).  `done`: device flag that turns kernels into no-ops.
int32_t pc_apply_dev(kryst_pc_t pc, const double* r, double* z, const int* done);
// Call after the stream has been synchronised: KRYST_OK, or KRYST_SOLVE_ERROR when an apply since the last check was abandoned
// by the device (the ILU wavefront solve's give-up path, tri_wave.h); the preconditioner has then switched itself to kernels
// that cannot stall, pc_fell_back() reports that switch once, and the caller repeats the work.
int32_t pc_health(kryst_pc_t pc);
bool pc_fell_back(kryst_pc_t pc);
int32_t bj_apply_dev(kryst_pc_t pc, const double* r, double* z, const int* done);   // block_jacobi.hip
void bj_free(kryst_pc_t pc);
int32_t amg_apply_dev(kryst_pc_t pc, const double* r, double* z, const int* done);   // amg.hip
int32_t asm_apply_dev(kryst_pc_t pc, const double* r, double* z, const int* done);   // asm.hip
void asm_free(kryst_pc_t pc);
int32_t sor_apply_dev(kryst_pc_t pc, const double* r, double* z, const int* done);   // sor.hip
void sor_free(kryst_pc_t pc);
int32_t sor_health(kryst_pc_t pc);
// whether the apply reads z on entry (AMG as written starts its finest level from the incoming z, amg.rs:211)
bool pc_reads_z(kryst_pc_t pc);
// pc_apply_dev for solvers whose reference apply gets a FRESH z: z = 0 (init == nullptr; gmres.rs:244, 250, 256, 283, 311, 339) or
// z = init (fgmres.rs:208-210: z_basis[j] = v_basis[j].clone()) first, when the preconditioner reads z; both gated by `done`
int32_t pc_apply_dev_fresh(kryst_pc_t pc, const double* r, double* z, const int* done, const double* init);
void amg_free(kryst_pc_t pc);
int32_t chebyshev_dev(kryst_csr_t a, const double* r, double* z, double alpha, double beta, int64_t m,
                      double* v0, double* v1, double* v2, const int* done);
}
