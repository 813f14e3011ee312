//! Raw `extern "C"` declarations of include/kryst_hip.h (ABI version 5), one to one.  Everything returns an `i32` status:
//! 0 OK, 1..6 = `KError` (src/error.rs:6-19), >= 100 runtime / argument errors (`kryst_hip_last_error()` has the text).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_void};

pub type Ctx = *mut c_void;
pub type Csr = *mut c_void;
pub type Vecd = *mut c_void;
pub type Pc = *mut c_void;
pub type Session = *mut c_void;
pub type HostFactors = *mut c_void;
pub type HostAmg = *mut c_void;
pub type Dense = *mut c_void;
pub type Lu = *mut c_void;
pub type MVec = *mut c_void;

pub const KRYST_OK: i32 = 0;
pub const KRYST_FACTOR_ERROR: i32 = 1;
pub const KRYST_SOLVE_ERROR: i32 = 2;
pub const KRYST_INDEFINITE_MATRIX: i32 = 3;
pub const KRYST_INDEFINITE_PRECONDITIONER: i32 = 4;
pub const KRYST_ZERO_PIVOT: i32 = 5;
pub const KRYST_UNSUPPORTED: i32 = 6;
pub const KRYST_ERR_HIP: i32 = 100;
pub const KRYST_ERR_RCCL: i32 = 101;
pub const KRYST_ERR_ARG: i32 = 102;
pub const KRYST_ERR_CSR: i32 = 103;
pub const KRYST_ERR_BUSY: i32 = 104;

pub const KRYST_ILU_KRYST_COMPAT: i32 = 0;
pub const KRYST_ILU_ILUP0: i32 = 1;
pub const KRYST_ILU_TRUE_ILU0: i32 = 2;
pub const KRYST_CHEB_SCALE_NONE: i32 = 0;
pub const KRYST_CHEB_SCALE_JACOBI: i32 = 1;
pub const KRYST_AMG_AS_WRITTEN: i32 = 0;
pub const KRYST_AMG_SMOOTHED: i32 = 1;
pub const KRYST_AMG_DIRECT_MAX: i32 = 4096;
pub const KRYST_ASM_AS_WRITTEN: i32 = 0;
pub const KRYST_ASM_GROWN: i32 = 1;
pub const KRYST_ASM_RESTRICTED: i32 = 2;
pub const KRYST_ASM_MAX_ROWS: i32 = 128;

/// kryst_params_t
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct Params {
    pub tol: f64,
    pub max_iters: i64,
    pub restart: i32,
    pub precond_side: i32,
    pub norm_type: i32,
    pub single_reduction: i32,
    pub has_radius: i32,
    pub radius: f64,
    pub has_obj_target: i32,
    pub obj_target: f64,
    pub check_every: i32,
}

/// kryst_stats_t
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct Stats {
    pub iterations: i64,
    pub final_residual: f64,
    pub converged: i32,
}

pub type MonitorFn = Option<unsafe extern "C" fn(iteration: i64, residual: f64, user: *mut c_void)>;

extern "C" {
    pub fn kryst_hip_last_error() -> *const c_char;
    pub fn kryst_hip_last_error_row() -> i64;
    pub fn kryst_hip_abi_version() -> i32;
    pub fn kryst_device_count(count: *mut i32) -> i32;
    pub fn kryst_reduce_spec(t: *mut i32, v: *mut i32, f: *mut i32);

    pub fn kryst_ctx_create(device_id: i32, out: *mut Ctx) -> i32;
    pub fn kryst_comm_unique_id(out128: *mut c_void) -> i32;
    pub fn kryst_ctx_create_dist(device_id: i32, rank: i32, nranks: i32, unique_id128: *const c_void, out: *mut Ctx) -> i32;
    pub fn kryst_ctx_destroy(ctx: Ctx) -> i32;
    pub fn kryst_ctx_synchronize(ctx: Ctx) -> i32;
    pub fn kryst_ctx_rank(ctx: Ctx, rank: *mut i32, nranks: *mut i32) -> i32;
    pub fn kryst_comm_barrier(ctx: Ctx) -> i32;
    pub fn kryst_comm_all_reduce(ctx: Ctx, x: f64, out: *mut f64) -> i32;
    pub fn kryst_ctx_scalar_reduce(ctx: Ctx, mode: i32, active: *mut i32) -> i32;
    pub fn kryst_csr_halo_mode(a: Csr, mode: i32, active: *mut i32) -> i32;
    pub fn kryst_ctx_trim(ctx: Ctx, bytes_released: *mut i64) -> i32;
    pub fn kryst_phase_timing_begin(ctx: Ctx) -> i32;
    pub fn kryst_phase_timing_end(ctx: Ctx, ms: *mut f64, count: i32) -> i32;
    pub fn kryst_phase_count() -> i32;
    pub fn kryst_phase_name(phase: i32) -> *const c_char;
    pub fn kryst_ctx_timer_start(ctx: Ctx) -> i32;
    pub fn kryst_ctx_timer_stop(ctx: Ctx, ms: *mut f64) -> i32;

    pub fn kryst_vec_create(ctx: Ctx, n: i64, out: *mut Vecd) -> i32;
    pub fn kryst_vec_destroy(v: Vecd) -> i32;
    pub fn kryst_vec_len(v: Vecd, n: *mut i64) -> i32;
    pub fn kryst_vec_upload(v: Vecd, host: *const f64, n: i64) -> i32;
    pub fn kryst_vec_download(v: Vecd, host: *mut f64, n: i64) -> i32;
    pub fn kryst_vec_fill(v: Vecd, value: f64) -> i32;
    pub fn kryst_vec_copy(dst: Vecd, src: Vecd) -> i32;
    pub fn kryst_vec_fill_splitmix(v: Vecd, seed: u64, global_offset: i64) -> i32;

    pub fn kryst_csr_create(ctx: Ctx, nrows: i64, ncols: i64, row_ptr: *const u64, col_idx: *const u64, vals: *const f64, out: *mut Csr) -> i32;
    pub fn kryst_csr_create_i32(ctx: Ctx, nrows: i64, ncols: i64, row_ptr: *const i64, col_idx: *const i32, vals: *const f64, out: *mut Csr) -> i32;
    pub fn kryst_csr_create_dist(ctx: Ctx, n_global: i64, row_offsets: *const i64, row_ptr: *const i64, col_idx_global: *const i64,
                                 vals: *const f64, out: *mut Csr) -> i32;
    pub fn kryst_csr_create_stencil7(ctx: Ctx, n: i32, kind: i32, out: *mut Csr) -> i32;
    pub fn kryst_csr_destroy(a: Csr) -> i32;
    pub fn kryst_csr_shape(a: Csr, nrows_local: *mut i64, ncols_global: *mut i64, nnz_local: *mut i64) -> i32;
    pub fn kryst_csr_encoding(a: Csr, encoding: *mut i32, patterns: *mut i32, table_entries: *mut i32) -> i32;
    pub fn kryst_csr_tile_order(a: Csr, info: *mut i64) -> i32;
    pub fn kryst_csr_pattern_info(a: Csr, info: *mut i64) -> i32;
    pub fn kryst_csr_fuse_march_info(a: Csr, info: *mut i64) -> i32;
    pub fn kryst_csr_pid_reuse_info(a: Csr, info: *mut i64) -> i32;
    pub fn kryst_csr_leg_values_info(a: Csr, info: *mut i64, values: *mut f64) -> i32;
    pub fn kryst_csr_download(a: Csr, row_ptr: *mut i64, col_idx_local: *mut i32, vals: *mut f64) -> i32;
    pub fn kryst_csr_placement_info(a: Csr, tries: *mut i32, chosen: *mut i32, skeleton_ms8: *mut f64) -> i32;

    pub fn kryst_spmv(a: Csr, x: Vecd, y: Vecd) -> i32;
    pub fn kryst_spmv_transpose(a: Csr, x: Vecd, y: Vecd) -> i32;
    pub fn kryst_spmv_host(a: Csr, x: *const f64, nx: i64, y: *mut f64, ny: i64) -> i32;
    pub fn kryst_bench_spmv(a: Csr, x: Vecd, y: Vecd, fused_dots: i32, reps: i32, avg_ms: *mut f64) -> i32;
    pub fn kryst_bench_streams(ctx: Ctx, n: i64, stride_bytes: i64, kind: i32, reps: i32, avg_ms: *mut f64) -> i32;
    pub fn kryst_bench_csr_skeleton(a: Csr, x: Vecd, y: Vecd, reps: i32, avg_ms: *mut f64) -> i32;
    pub fn kryst_bench_spmv_fused(a: Csr, x: Vecd, y: Vecd, reps: i32, avg_ms: *mut f64) -> i32;
    pub fn kryst_bench_poison_lds(ctx: Ctx) -> i32;
    pub fn kryst_bench_vec_padding(v: Vecd, fill: *const f64, dirty: *mut i64) -> i32;

    pub fn kryst_dot(x: Vecd, y: Vecd, out: *mut f64) -> i32;
    pub fn kryst_norm(x: Vecd, out: *mut f64) -> i32;
    pub fn kryst_axpy(alpha: f64, x: Vecd, y: Vecd) -> i32;
    pub fn kryst_aypx(beta: f64, x: Vecd, y: Vecd) -> i32;
    pub fn kryst_sub(a: Vecd, b: Vecd, out: Vecd) -> i32;

    pub fn kryst_pc_identity(ctx: Ctx, out: *mut Pc) -> i32;
    pub fn kryst_pc_jacobi(a: Csr, out: *mut Pc) -> i32;
    pub fn kryst_pc_ilu0(a: Csr, mode: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_ilup(a: Csr, fill: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_ilut(a: Csr, fill: i32, droptol: f64, out: *mut Pc) -> i32;
    pub fn kryst_pc_chebyshev_stub(ctx: Ctx, degree: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_chebyshev(a: Csr, alpha: f64, beta: f64, degree: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_chebyshev_poly(a: Csr, degree: i32, scaling: i32, lo: f64, hi: f64, out: *mut Pc) -> i32;
    pub fn kryst_pc_chebyshev_poly_info(pc: Pc, degree: *mut i32, scaling: *mut i32, lo: *mut f64, hi: *mut f64, fused: *mut i32) -> i32;
    pub fn kryst_spectrum_estimate(a: Csr, scaling: i32, steps: i32, seed: u64, alpha_out: *mut f64, beta_out: *mut f64, steps_done: *mut i32,
                                   theta_min: *mut f64, theta_max: *mut f64, gershgorin: *mut f64) -> i32;
    pub fn kryst_host_tridiag_extreme_eigs(alpha: *const f64, beta: *const f64, k: i32, lo: *mut f64, hi: *mut f64) -> i32;
    pub fn kryst_pc_approx_inverse(m: Csr, out: *mut Pc) -> i32;
    pub fn kryst_pc_block_jacobi(a: Csr, blk_ptr: *const i64, blk_idx: *const i64, nblocks: i64, out: *mut Pc) -> i32;
    pub fn kryst_pc_block_jacobi_uniform(a: Csr, bsize: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_block_jacobi_export(pc: Pc, nnz: *mut i64, row_ptr: *mut i64, col: *mut i32, val: *mut f64) -> i32;
    pub fn kryst_pc_asm(a: Csr, sub_ptr: *const i64, sub_idx: *const i64, nsub: i64, overlap: i32, variant: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_asm_uniform(a: Csr, nparts: i64, overlap: i32, variant: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_asm_info(pc: Pc, nsub: *mut i64, ext_rows: *mut i64, max_rows: *mut i32) -> i32;
    pub fn kryst_pc_asm_export(pc: Pc, sub_ptr: *mut i64, sub_idx: *mut i32, owner: *mut i32, tiles: *mut f64) -> i32;
    pub fn kryst_pc_asm_ilu(a: Csr, sub_ptr: *const i64, sub_idx: *const i64, nsub: i64, overlap: i32, variant: i32, sub_mode: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_asm_ilu_uniform(a: Csr, nparts: i64, overlap: i32, variant: i32, sub_mode: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_asm_ilu_info(pc: Pc, info: *mut i64, count: i32) -> i32;
    pub fn kryst_pc_asm_ilu_export(pc: Pc, sub_ptr: *mut i64, sub_idx: *mut i32, owner: *mut i32, ent_ptr: *mut i64, row_ptr: *mut i32, col: *mut i32,
                                   val: *mut f64, lev_l: *mut i32, lev_u: *mut i32) -> i32;
    pub fn kryst_pc_sor(a: Csr, omega: f64, its: i64, lits: i64, sym_bits: u32, fshift: f64, colors: *const i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_sor_info(pc: Pc, groups_forward: *mut i32, groups_backward: *mut i32, rows: *mut i64, grid_forward: *mut i32, grid_backward: *mut i32) -> i32;
    // dense storage and the direct solvers (DenseMatrix src/matrix/dense.rs, LuSolver / QrSolver src/solver/direct_lu.rs)
    pub fn kryst_dense_create(ctx: Ctx, nrows: i64, ncols: i64, data: *const f64, colmajor: i32, out: *mut Dense) -> i32;
    pub fn kryst_dense_from_csr(a: Csr, out: *mut Dense) -> i32;
    pub fn kryst_dense_shape(a: Dense, nrows: *mut i64, ncols: *mut i64) -> i32;
    pub fn kryst_dense_download(a: Dense, colmajor: *mut f64) -> i32;
    pub fn kryst_dense_destroy(a: Dense) -> i32;
    pub fn kryst_dense_matvec(a: Dense, x: Vecd, y: Vecd) -> i32;
    pub fn kryst_lu_create(ctx: Ctx, out: *mut Lu) -> i32;
    pub fn kryst_lu_destroy(lu: Lu) -> i32;
    pub fn kryst_lu_solve(lu: Lu, a: Dense, pc: Pc, b: *const f64, x: *mut f64, n: i64, stats: *mut Stats) -> i32;
    pub fn kryst_lu_solve_dev(lu: Lu, a: Dense, pc: Pc, b: Vecd, x: Vecd, stats: *mut Stats) -> i32;
    pub fn kryst_lu_solve_cached(lu: Lu, b: Vecd, x: Vecd) -> i32;
    pub fn kryst_lu_export(lu: Lu, n: i64, row_perm: *mut i64, col_perm: *mut i64, factors_colmajor: *mut f64) -> i32;
    pub fn kryst_lu_info(lu: Lu, info: *mut i64, count: i32) -> i32;
    pub fn kryst_qr_solve(a: Dense, pc: Pc, b: *const f64, x: *mut f64, n: i64, stats: *mut Stats) -> i32;
    pub fn kryst_qr_solve_dev(a: Dense, pc: Pc, b: Vecd, x: Vecd, stats: *mut Stats) -> i32;
    pub fn kryst_host_dense_lu(nrows: i64, ncols: i64, a: *const f64, row_perm: *mut i64, col_perm: *mut i64, factors: *mut f64) -> i32;
    pub fn kryst_host_dense_lu_solve(n: i64, row_perm: *const i64, col_perm: *const i64, factors: *const f64, b: *const f64, x: *mut f64) -> i32;
    pub fn kryst_host_dense_qr_solve(nrows: i64, ncols: i64, a: *const f64, b: *const f64, x: *mut f64) -> i32;
    pub fn kryst_host_color_graph(n: i64, ptr: *const i64, col: *const i32, colors: *mut i32, ncolors: *mut i32) -> i32;
    pub fn kryst_pc_spai(a: Csr, pattern_kind: i32, pat_ptr: *const i64, pat_idx: *const i64, pat_n: i64, tol: f64, out: *mut Pc) -> i32;
    pub fn kryst_pc_spai_export(pc: Pc, nnz: *mut i64, row_ptr: *mut i64, col: *mut i32, val: *mut f64) -> i32;
    pub fn kryst_pc_amg(a: Csr, max_levels: i32, threshold: f64, variant: i32, nu_pre: i32, nu_post: i32, out: *mut Pc) -> i32;
    pub fn kryst_pc_amg_info(pc: Pc, nlevels: *mut i32, rows: *mut i64, nnz: *mut i64, count: i32) -> i32;
    pub fn kryst_pc_amg_export(pc: Pc, level: i32, which: i32, nrows: *mut i64, ncols: *mut i64, nnz: *mut i64, row_ptr: *mut i64,
                               col: *mut i32, val: *mut f64) -> i32;
    pub fn kryst_pc_apply(pc: Pc, r: Vecd, z: Vecd) -> i32;
    pub fn kryst_pc_destroy(pc: Pc) -> i32;
    pub fn kryst_bench_pc_apply(pc: Pc, r: Vecd, z: Vecd, reps: i32, avg_ms: *mut f64) -> i32;
    pub fn kryst_pc_ilu_info(pc: Pc, info: *mut i64, count: i32) -> i32;
    pub fn kryst_apply_chebyshev(a: Csr, r: Vecd, z: Vecd, alpha: f64, beta: f64, m: i64) -> i32;
}

/// The tail every solve entry point shares (KRYST_SOLVE_ARGS).
macro_rules! solve_fn {
    ($($name:ident),* ; host) => { extern "C" { $( pub fn $name(b: *const f64, x: *mut f64, n: i64, a: Csr, pc: Pc, params: *const Params,
        stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64, monitor: MonitorFn, user: *mut c_void) -> i32; )* } };
    ($($name:ident),* ; dev) => { extern "C" { $( pub fn $name(b: Vecd, x: Vecd, a: Csr, pc: Pc, params: *const Params,
        stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64, monitor: MonitorFn, user: *mut c_void) -> i32; )* } };
}
solve_fn!(kryst_cg_solve, kryst_pcg_solve, kryst_gmres_solve, kryst_bicgstab_solve, kryst_cgs_solve, kryst_tfqmr_solve,
          kryst_minres_solve, kryst_qmr_solve, kryst_cgnr_solve; host);
solve_fn!(kryst_cg_solve_dev, kryst_pcg_solve_dev, kryst_gmres_solve_dev, kryst_bicgstab_solve_dev, kryst_bicgstab_rpc_solve_dev,
          kryst_cgs_solve_dev, kryst_tfqmr_solve_dev, kryst_minres_solve_dev, kryst_qmr_solve_dev, kryst_cgnr_solve_dev,
          kryst_minres_textbook_solve_dev, kryst_cgnr_textbook_solve_dev; dev);

extern "C" {
    pub fn kryst_fgmres_solve(b: *const f64, x: *mut f64, n: i64, orthog: i32, haptol: f64, preallocate: i32, a: Csr, pc: Pc,
                              params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                              monitor: MonitorFn, user: *mut c_void) -> i32;
    pub fn kryst_fgmres_solve_dev(b: Vecd, x: Vecd, orthog: i32, haptol: f64, preallocate: i32, a: Csr, pc: Pc,
                                  params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                                  monitor: MonitorFn, user: *mut c_void) -> i32;

    // PcaGmresSolver::solve (src/solver/pca_gmres.rs:99-312) as written; the s-step extension (device vectors only)
    pub fn kryst_pca_gmres_solve(b: *const f64, x: *mut f64, n: i64, block_size: i32, pipeline_depth: i32, tau: f64, a: Csr, pc: Pc,
                                 params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                                 monitor: MonitorFn, user: *mut c_void) -> i32;
    pub fn kryst_pca_gmres_solve_dev(b: Vecd, x: Vecd, block_size: i32, pipeline_depth: i32, tau: f64, a: Csr, pc: Pc,
                                     params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                                     monitor: MonitorFn, user: *mut c_void) -> i32;
    pub fn kryst_pca_gmres_textbook_solve_dev(b: Vecd, x: Vecd, block_size: i32, pipeline_depth: i32, tau: f64, a: Csr, pc: Pc,
                                              params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                                              monitor: MonitorFn, user: *mut c_void) -> i32;

    // compressed-basis GMRES (extension): basis 0 = fp64 (control), 1 = fp32-stored Krylov basis; sides None and Right; device vectors only
    pub fn kryst_cbgmres_solve_dev(b: Vecd, x: Vecd, basis: i32, a: Csr, pc: Pc,
                                   params: *const Params, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64,
                                   monitor: MonitorFn, user: *mut c_void) -> i32;

    pub fn kryst_session_begin(method: i32, b: Vecd, x: Vecd, a: Csr, pc: Pc, params: *const Params, out: *mut Session) -> i32;
    pub fn kryst_session_step(s: Session, k: i64) -> i32;
    pub fn kryst_session_end(s: Session, stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;

    pub fn kryst_host_stencil7(n: i32, kind: i32, k_lo: i32, k_hi: i32, row_ptr: *mut i64, col_idx: *mut i64, vals: *mut f64) -> i64;
    pub fn kryst_host_partition_rows(n: i64, nranks: i32, align: i64, row_offsets: *mut i64) -> i32;
    pub fn kryst_host_halo_recv_plan(rank: i32, nranks: i32, row_offsets: *const i64, row_ptr: *const i64, col_idx_global: *const i64,
                                     recv_counts: *mut i64, recv_cols: *mut i64) -> i64;
    pub fn kryst_host_ilup(n: i64, row_ptr: *const i64, col: *const i32, val: *const f64, fill: i32, threads: i32, block: i64, out: *mut HostFactors) -> i32;
    pub fn kryst_host_ilut(n: i64, row_ptr: *const i64, col: *const i32, val: *const f64, fill: i32, droptol: f64, threads: i32, out: *mut HostFactors) -> i32;
    pub fn kryst_host_factors_sizes(f: HostFactors, n: *mut i64, nnz_l: *mut i64, nnz_u: *mut i64) -> i32;
    pub fn kryst_host_factors_get(f: HostFactors, l_ptr: *mut i64, l_col: *mut i32, l_val: *mut f64, u_ptr: *mut i64, u_col: *mut i32, u_val: *mut f64, diag: *mut f64) -> i32;
    pub fn kryst_host_factors_destroy(f: HostFactors) -> i32;
    pub fn kryst_host_amg(n: i64, row_ptr: *const i64, col: *const i32, val: *const f64, max_levels: i32, threshold: f64, level_budget: i64,
                          out: *mut HostAmg) -> i32;
    pub fn kryst_host_amg_levels(h: HostAmg, nlevels: *mut i32) -> i32;
    pub fn kryst_host_amg_get(h: HostAmg, level: i32, which: i32, nrows: *mut i64, ncols: *mut i64, nnz: *mut i64, row_ptr: *mut i64,
                              col: *mut i32, val: *mut f64) -> i32;
    pub fn kryst_host_amg_destroy(h: HostAmg) -> i32;
    pub fn kryst_host_levels(n: i64, ptr: *const i64, col: *const i32, forward: i32, level: *mut i32, nlevels: *mut i32) -> i32;
    pub fn kryst_host_read_matrix_market(path: *const c_char, nrows: *mut i64, ncols: *mut i64, row_ptr: *mut i64, col_idx: *mut i64,
                                         vals: *mut f64) -> i64;
    pub fn kryst_host_read_petsc_binary(path: *const c_char, nrows: *mut i64, ncols: *mut i64, row_ptr: *mut i64, col_idx: *mut i64,
                                        vals: *mut f64) -> i64;
}

// several right-hand sides at once (kryst_mvec_t: n x k, k in {2, 4, 8}; column j of a batched call = the single-vector call on column j)
extern "C" {
    pub fn kryst_mvec_create(ctx: Ctx, n: i64, k: i32, out: *mut MVec) -> i32;
    pub fn kryst_mvec_destroy(mv: MVec) -> i32;
    pub fn kryst_mvec_shape(mv: MVec, n: *mut i64, k: *mut i32) -> i32;
    pub fn kryst_mvec_upload(mv: MVec, host: *const f64, ld: i64) -> i32;
    pub fn kryst_mvec_download(mv: MVec, host: *mut f64, ld: i64) -> i32;
    pub fn kryst_mvec_set_column(mv: MVec, j: i32, v: Vecd) -> i32;
    pub fn kryst_mvec_get_column(mv: MVec, j: i32, v: Vecd) -> i32;
    pub fn kryst_bench_mvec_padding(mv: MVec, fill: *const f64, dirty: *mut i64) -> i32;
    pub fn kryst_spmm(a: Csr, x: MVec, y: MVec) -> i32;
    pub fn kryst_spmm_kernel(a: Csr, k: i32, kernel: *mut i32) -> i32;
    pub fn kryst_cg_solve_multi_dev(b: MVec, x: MVec, a: Csr, pc: Pc, params: *const Params, stats: *mut Stats, status: *mut i32,
                                    hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_pcg_solve_multi_dev(b: MVec, x: MVec, a: Csr, pc: Pc, params: *const Params, stats: *mut Stats, status: *mut i32,
                                     hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_cg_solve_multi(b: *const f64, x: *mut f64, n: i64, k: i32, ld: i64, a: Csr, pc: Pc, params: *const Params,
                                stats: *mut Stats, status: *mut i32, hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_pcg_solve_multi(b: *const f64, x: *mut f64, n: i64, k: i32, ld: i64, a: Csr, pc: Pc, params: *const Params,
                                 stats: *mut Stats, status: *mut i32, hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
}

// block CG: one Krylov space for the k columns of a multivector (declared, not wrapped: an extension like the batched solvers above)
extern "C" {
    pub fn kryst_bcg_solve_multi_dev(b: MVec, x: MVec, a: Csr, pc: Pc, params: *const Params, stats: *mut Stats, status: *mut i32,
                                     hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_bcg_solve_multi(b: *const f64, x: *mut f64, n: i64, k: i32, ld: i64, a: Csr, pc: Pc, params: *const Params,
                                 stats: *mut Stats, status: *mut i32, hist: *mut f64, hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_host_bcg_step(step: i32, k: i32, g: *const f64, c: *mut f64, out1: *mut f64, out2: *mut f64, res: *mut f64) -> i32;
    pub fn kryst_bench_mvec_gram(u: MVec, v: MVec, inv_diag: Vecd, out_kk: *mut f64) -> i32;
}

// mixed precision: fp32 as a storage format (fp64 arithmetic and scalars), CG / Jacobi-PCG on it and fp64 iterative refinement around them
pub type Vec32 = *mut c_void;
pub type Csr32 = *mut c_void;
// what the lowered operator keeps beside the plain arrays (kryst_csr32_lower_form); kryst_csr32_encoding reports 0 plain, 1 pattern,
// 2 pattern-stage, 3 dia
pub const KRYST_CSR32_PLAIN: i32 = 0;
pub const KRYST_CSR32_AUTO: i32 = 1;
pub const KRYST_CSR32_PATTERN: i32 = 2;
pub const KRYST_CSR32_DIA: i32 = 3;
pub const KRYST_CSR32_DIA_ABSENT_BITS: u32 = 0x7FD1_A0D1;        // "no entry here" in an fp32 diagonal stream
#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Csr32Form { Plain = KRYST_CSR32_PLAIN, Auto = KRYST_CSR32_AUTO, Pattern = KRYST_CSR32_PATTERN, Dia = KRYST_CSR32_DIA }
extern "C" {
    pub fn kryst_reduce_spec32(t: *mut i32, v: *mut i32, f: *mut i32);
    pub fn kryst_vec32_create(ctx: Ctx, n: i64, out: *mut Vec32) -> i32;
    pub fn kryst_vec32_destroy(v: Vec32) -> i32;
    pub fn kryst_vec32_upload(v: Vec32, host: *const f32, n: i64) -> i32;
    pub fn kryst_vec32_download(v: Vec32, host: *mut f32, n: i64) -> i32;
    pub fn kryst_bench_vec32_padding(v: Vec32, fill: *const f32, dirty: *mut i64) -> i32;
    pub fn kryst_vec32_from_f64(dst: Vec32, src: Vecd) -> i32;
    pub fn kryst_vec32_to_f64(dst: Vecd, src: Vec32) -> i32;
    pub fn kryst_dot32(x: Vec32, y: Vec32, out: *mut f64) -> i32;
    pub fn kryst_csr32_lower(a: Csr, out: *mut Csr32) -> i32;
    pub fn kryst_csr32_lower_form(a: Csr, form: i32, out: *mut Csr32) -> i32;        // form: Csr32Form as i32
    pub fn kryst_csr32_encoding(a: Csr32, kernel: *mut i32) -> i32;
    pub fn kryst_csr32_info(a: Csr32, info: *mut i64) -> i32;
    pub fn kryst_csr32_destroy(a: Csr32) -> i32;
    pub fn kryst_host_round_f32(v: *const f64, n: i64, out: *mut f32, info: *mut i64) -> i32;
    pub fn kryst_spmv32(a: Csr32, x: Vec32, y: Vec32) -> i32;
    pub fn kryst_cg32_solve_dev(b: Vec32, x: Vec32, a: Csr32, pc: Pc, params: *const Params, stats: *mut Stats, hist: *mut f64,
                                hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_pcg32_solve_dev(b: Vec32, x: Vec32, a: Csr32, pc: Pc, params: *const Params, stats: *mut Stats, hist: *mut f64,
                                 hist_cap: i64, hist_len: *mut i64) -> i32;
    pub fn kryst_refine_solve_dev(b: Vecd, x: Vecd, a: Csr, a32: Csr32, pc: Pc, outer: *const Params, inner: *const Params,
                                  stats: *mut Stats, hist: *mut f64, hist_cap: i64, hist_len: *mut i64, inner_iters: *mut i64,
                                  inner_cap: i64) -> i32;
}
