/*
 * kryst_hip.h -- C ABI of libkryst_hip.so: the MI355X (gfx950) Krylov inner loop behind kryst's
 * MatVec / Preconditioner / LinearSolver traits.
 *
 * Every entry point names the reference interface it replaces (paths relative to the kryst crate,
 * tmathis720/kryst v0.5.3).  A Rust maintainer binds these with `extern "C"` (INTEGRATION.md shows the
 * stub); tests and bench.py bind them with ctypes (kryst_amd/_ffi.py).
 *
 * Conventions
 *   - every function returns an int32 status: 0 OK, 1..6 mirror `KError` (src/error.rs:6-19),
 *     >= 100 are HIP / RCCL / argument errors; kryst_hip_last_error() gives the text.  Nothing unwinds
 *     across the ABI.
 *   - handles are opaque, created and destroyed by the library; host arrays are borrowed only for the
 *     duration of a call; one host thread per context; contexts are independent.
 *   - all handles of one call belong to ONE context: a call that is handed handles of two contexts returns KRYST_ERR_ARG before any
 *     launch and writes nothing -- a preconditioner the solver ignores included.
 *   - all arithmetic is IEEE fp64 with no FMA contraction; row sums run over ascending stored columns.
 *   - inner products use ONE fixed association tree (kryst_reduce_spec): results are run-to-run and
 *     launch-configuration independent; with nranks > 1 rank results are folded in rank order.
 *   - there is no CPU fallback: without a GPU every compute call fails with KRYST_ERR_HIP.
 *   - Contexts: the scalar state of a solve (alpha, beta, the convergence record, the progress record the host polls)
 *     lives in per-context device scratch, so ONE solve or stepping session can be open per context at a time.  While
 *     a session is open, kryst_*_solve[_dev] and kryst_session_begin on the same context return KRYST_ERR_BUSY;
 *     kryst_spmv, kryst_dot / kryst_norm, the vector updates and kryst_pc_apply stay legal (they are stream-ordered
 *     behind the session's enqueued iterations and use scratch of their own).  Use a second context for a second
 *     concurrent solve.
 */
#ifndef KRYST_HIP_H
#define KRYST_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: src/error.rs:6-19 ---- */
enum {
    KRYST_OK = 0,
    KRYST_FACTOR_ERROR = 1,             /* KError::FactorError */
    KRYST_SOLVE_ERROR = 2,              /* KError::SolveError */
    KRYST_INDEFINITE_MATRIX = 3,        /* KError::IndefiniteMatrix            cg.rs:168-174, pcg.rs:162-172 */
    KRYST_INDEFINITE_PRECONDITIONER = 4,/* KError::IndefinitePreconditioner    cg.rs:254-259, pcg.rs:208-213 */
    KRYST_ZERO_PIVOT = 5,               /* KError::ZeroPivot(row) */
    KRYST_UNSUPPORTED = 6,              /* KError::Unsupported */
    KRYST_ERR_HIP = 100,                /* HIP runtime error / no device */
    KRYST_ERR_RCCL = 101,               /* RCCL error / library not found */
    KRYST_ERR_ARG = 102,                /* bad argument (length mismatch = the reference's assert_eq! panics) */
    KRYST_ERR_CSR = 103,                /* CSR violates new_checked preconditions (sparse.rs:36-42) */
    KRYST_ERR_BUSY = 104                /* a solve / stepping session is already open on this context (see "Contexts") */
};

typedef struct kryst_ctx_s* kryst_ctx_t;
typedef struct kryst_csr_s* kryst_csr_t;
typedef struct kryst_vec_s* kryst_vec_t;
typedef struct kryst_pc_s*  kryst_pc_t;

const char* kryst_hip_last_error(void);
/* the row of the last KRYST_ZERO_PIVOT on this thread (KError::ZeroPivot(row), src/error.rs:15-16), -1 if none yet */
int64_t     kryst_hip_last_error_row(void);
int32_t     kryst_hip_abi_version(void);
/* The fixed inner-product tree: tile = T*V elements; thread t folds its V elements, 64-lane xor butterfly,
 * serial across the T/64 waves; the tile partials are folded in chunks of F (one per thread, butterfly, serial
 * across the F/64 waves) and, when there is more than one chunk, the chunk values by F threads (stride F) likewise. */
void        kryst_reduce_spec(int32_t* T, int32_t* V, int32_t* F);

/* ---- context: one per GPU / per rank.  Replaces src/parallel (Comm trait, parallel/mod.rs:4-35) ---- */
/* HIP devices this process sees (0 without a GPU): a launcher checks it before it hands LOCAL_RANK to kryst_ctx_create_dist -- one rank
 * per GPU, as MpiComm::new gets one rank per process from mpirun (src/parallel/mpi_comm.rs:49-55) */
int32_t kryst_device_count(int32_t* count);
int32_t kryst_ctx_create(int32_t device_id, kryst_ctx_t* out);
/* rank/nranks + 128-byte RCCL unique id (rank 0 makes it with kryst_comm_unique_id and ships it to the other
 * ranks by any side channel).  Replaces MpiComm::new (src/parallel/mpi_comm.rs:49-55). */
int32_t kryst_comm_unique_id(void* out128);
int32_t kryst_ctx_create_dist(int32_t device_id, int32_t rank, int32_t nranks, const void* unique_id128,
                              kryst_ctx_t* out);
int32_t kryst_ctx_destroy(kryst_ctx_t ctx);
int32_t kryst_ctx_synchronize(kryst_ctx_t ctx);                    /* hipStreamSynchronize on the ctx streams */
int32_t kryst_ctx_rank(kryst_ctx_t ctx, int32_t* rank, int32_t* nranks);   /* Comm::rank / Comm::size */
int32_t kryst_comm_barrier(kryst_ctx_t ctx);                       /* Comm::barrier, mpi_comm.rs:67 */
int32_t kryst_comm_all_reduce(kryst_ctx_t ctx, double x, double* out);     /* Comm::all_reduce, mpi_comm.rs:116-121 */
/* How the solvers' inner products cross the ranks (DistributedInnerProduct, core/wrappers.rs:134-156): mode 0 = RCCL all-gather +
 * rank-ordered fold, 1 = hipIpc-mapped mailboxes written and polled by the kernel that finishes the local fold (one launch, no
 * collective; the same bits), -1 = query (*active only; not collective).  Modes 0 / 1: COLLECTIVE over the context's ranks, no solve
 * open.  Mode 1 returns KRYST_UNSUPPORTED -- on every rank, which all stay on RCCL -- when a mailbox cannot be exported or mapped or ONE
 * CHECKED TEST REDUCTION over the fresh mailboxes does not arrive intact on some rank.  *active (may be NULL): mode in use.
 * DEFAULT (ABI 5): kryst_ctx_create_dist with more than one rank tries mode 1 and keeps it when it works on every rank;
 * KRYST_SCALAR_REDUCE=rccl keeps mode 0. */
int32_t kryst_ctx_scalar_reduce(kryst_ctx_t ctx, int32_t mode, int32_t* active);
/* How a row-partitioned operator's halo exchange travels (the neighbour exchange src/parallel/mpi_comm.rs:133-143 leaves as a TODO): mode 0 =
 * grouped ncclSend / ncclRecv on the second stream, 1 = direct peer stores -- a push kernel writes the rows each neighbour needs
 * straight into that neighbour's hipIpc-mapped landing buffer and stamps the exchange's epoch behind them, the receiver's compute stream
 * polls its stamps in front of the boundary tiles: no collective launch, no pack kernel, no event between receive and compute stream --
 * -1 = query (*active only; not collective).  Modes 0 / 1: COLLECTIVE over the context's ranks, no solve open.  Mode 1 returns
 * KRYST_UNSUPPORTED -- on every rank, which all stay on RCCL -- when a landing buffer cannot be exported or mapped, a neighbour relation is
 * one-way, or ONE CHECKED TEST EXCHANGE (every rank sends its global row numbers and compares what lands with its column list) does not
 * arrive intact on some rank.  The same bits either way.  *active (may be NULL): mode in use.
 * DEFAULT (ABI 5): kryst_csr_create_dist / kryst_csr_create_stencil7 on a context of several ranks try mode 1 and keep it when it works on
 * every rank; KRYST_HALO_MODE=rccl keeps mode 0.  kryst_spmv on an operator in mode 1 returns KRYST_ERR_RCCL when a neighbour's stamp
 * never arrived (the halo was NaNs). */
int32_t kryst_csr_halo_mode(kryst_csr_t a, int32_t mode, int32_t* active);
/* Returns to the driver what the context keeps between calls: the device blocks of destroyed ILU-family preconditioners -- kept, keyed by
 * size, so that the next Preconditioner::setup of the same matrix (ilup.rs:77-134 is called per matrix, repeatedly) costs the factorisation
 * and not 22 GB of allocation at 512^3; bounded by KRYST_DEV_POOL_MB (default 65536, 0 = no pool) -- and, when no solve is open, the solvers'
 * work-vector arena.  *bytes_released may be NULL. */
int32_t kryst_ctx_trim(kryst_ctx_t ctx, int64_t* bytes_released);
/* measurement only: per-phase device time of the work enqueued between begin and end (hipEvents recorded on the compute stream
 * after each phase: time between two marks is charged to the later one).  ms[p] for p < kryst_phase_count(): "spmv" (tiles
 * without halo columns; single rank: the whole SpMV), "halo_wait" (compute stream waiting for the neighbour planes),
 * "spmv_boundary", "reduce" (tile-partial fold + RCCL all-gather + rank-ordered fold + scalar step), "blas1" (vector updates other than
 * the next two), "pc", "blas1_residual" (CG / PCG: r -= alpha Ap with its fused inner products), "blas1_direction" (CG / PCG: x += alpha p,
 * p = z + beta p), "blas1_xbatch" (CG / PCG with the direction pass inside the SpMV: x += alpha_i p_i for a batch of iterations in one pass). */
int32_t kryst_phase_timing_begin(kryst_ctx_t ctx);
int32_t kryst_phase_timing_end(kryst_ctx_t ctx, double* ms, int32_t count);
int32_t kryst_phase_count(void);
const char* kryst_phase_name(int32_t phase);
/* wall-clock of the device work enqueued between the two marks, in ms (hipEvent on the ctx compute stream) */
int32_t kryst_ctx_timer_start(kryst_ctx_t ctx);
int32_t kryst_ctx_timer_stop(kryst_ctx_t ctx, double* ms);

/* ---- device vectors (the reference's V = Vec<f64>); in a distributed ctx n is the LOCAL length ---- */
int32_t kryst_vec_create(kryst_ctx_t ctx, int64_t n, kryst_vec_t* out);
int32_t kryst_vec_destroy(kryst_vec_t v);
int32_t kryst_vec_len(kryst_vec_t v, int64_t* n);
int32_t kryst_vec_upload(kryst_vec_t v, const double* host, int64_t n);
int32_t kryst_vec_download(kryst_vec_t v, double* host, int64_t n);
int32_t kryst_vec_fill(kryst_vec_t v, double value);
int32_t kryst_vec_copy(kryst_vec_t dst, kryst_vec_t src);             /* dst == src: allowed, nothing is done */
/* deterministic synthetic fill on device: v[i] = uniform[0,1) from splitmix64(seed, global index) */
int32_t kryst_vec_fill_splitmix(kryst_vec_t v, uint64_t seed, int64_t global_offset);

/* ---- CSR operator: CsrMatrix::from_csr (src/matrix/sparse.rs:28-46), usize = uint64 layout ---- */
int32_t kryst_csr_create(kryst_ctx_t ctx, int64_t nrows, int64_t ncols, const uint64_t* row_ptr,
                         const uint64_t* col_idx, const double* vals, kryst_csr_t* out);
/* same with int32 column indices / int64 row pointers (what the device keeps; avoids 2x host memory) */
int32_t kryst_csr_create_i32(kryst_ctx_t ctx, int64_t nrows, int64_t ncols, const int64_t* row_ptr,
                             const int32_t* col_idx, const double* vals, kryst_csr_t* out);
/* Row-partitioned operator: this rank owns global rows [row_lo,row_hi) (= row_offsets[rank..rank+1]);
 * row_ptr is local (row_ptr[0] == 0), col_idx are GLOBAL columns.  Builds the halo exchange plan (one
 * RCCL exchange of index lists).  The reference has no counterpart (mpi_comm.rs:133-143 is a TODO). */
int32_t kryst_csr_create_dist(kryst_ctx_t ctx, int64_t n_global, const int64_t* row_offsets /*nranks+1*/,
                              const int64_t* row_ptr, const int64_t* col_idx_global, const double* vals,
                              kryst_csr_t* out);
/* Synthetic 7-point stencil operator generated on the device: kind 0 Poisson, 1 anisotropic,
 * 2 upwind convection-diffusion, 3 symmetric variable-coefficient diffusion (per-edge weights from splitmix64: no two rows
 * alike, so no value dictionary / row patterns apply -- what a structured grid with real coefficients looks like);
 * grid N^3; in a distributed ctx each rank builds its k-slab. */
int32_t kryst_csr_create_stencil7(kryst_ctx_t ctx, int32_t N, int32_t kind, kryst_csr_t* out);
int32_t kryst_csr_destroy(kryst_csr_t a);
int32_t kryst_csr_shape(kryst_csr_t a, int64_t* nrows_local, int64_t* ncols_global, int64_t* nnz_local);
/* storage form kryst_spmv streams for this operator (all forms are lossless re-encodings made at creation beside the CSR arrays;
 * results are bit-identical): 0 plain CSR, 1 CSR-D8 (1-byte column-offset codes), 2 CSR-D16 (offset + value codes, 2 B per
 * entry), 3 CSR-P16 (one 16-bit row-pattern id per row), 4 CSR-DIA (one value stream per diagonal: operators with at most 32
 * well-filled diagonals that have no D16 / P16 form, e.g. variable-coefficient stencils).  patterns / table_entries (may be NULL):
 * size of the P16 tables. */
int32_t kryst_csr_encoding(kryst_csr_t a, int32_t* encoding, int32_t* patterns, int32_t* table_entries);
/* measurement hook: the order in which an operator's 512-row tiles are handed to the XCDs (plane-structured operators walk the
 * plane segment by segment so that an XCD's L2 keeps its window of x; which rows a tile holds and every result bit are unchanged).
 * info[0] rows per plane (0: natural order only), info[1], info[2] slots of the two orders, info[3] 1 if kryst_spmv uses it now */
int32_t kryst_csr_tile_order(kryst_csr_t a, int64_t* info);
/* measurement hook: the staged-window form of the CSR-P16 kernel (operators whose row patterns are (far, -n, -1, 0, +1, +n, far) with one
 * even n <= 1024: the near operands of a run of tiles come out of an LDS window).  info[0] n (0: not this form), info[1] 1 if the far
 * offsets are the same in every pattern, info[2] first tile of a rank's contiguous interior range (-1: none), info[3] 1 if kryst_spmv
 * takes that kernel now */
int32_t kryst_csr_pattern_info(kryst_csr_t a, int64_t* info);
/* measurement hook: the marching mode of the fused direction + SpMV kernel of CG / PCG (a workgroup keeps a strip of 512 T rows of a grid
 * plane and walks a segment of S planes, the operands one plane away come out of its own LDS windows; results are the same bits).  With the
 * KRYST_SPMV_FUSE_* settings as they are now: info[0] 1 if the operator's shape allows it (far offsets of +- one plane, a plane that is a
 * whole number of strips, a box that is a whole number of planes, lines of at most 512 points), info[1] 1 if a fused launch takes it now,
 * info[2] T, info[3] strips per plane, info[4] S, info[5] segments (info[3 .. 5] 0 when not eligible), info[6] 1 if a fused CG iteration would
 * now store no A p and form it again in its residual pass (KRYST_CG_RECOMPUTE_AP; the marching mode on, x updated in batches).  info: 7 values */
int32_t kryst_csr_fuse_march_info(kryst_csr_t a, int64_t* info);
/* measurement hook: the marching kernels keep a tile's row-pattern ids in registers where they repeat those of the tile one grid plane below
 * (a per-tile table made once at creation; KRYST_SPMV_PID_REUSE = 0 hands the kernels no table: every plane loads its ids; the same bits either
 * way).  info[0] 1 if a marching launch would be handed the table now, info[1] tiles flagged as repeating, info[2] tiles the table covers
 * (info[1], info[2] 0 for an operator without a table).  info: 3 values */
int32_t kryst_csr_pid_reuse_info(kryst_csr_t a, int64_t* info);
/* measurement hook: the step of CG's recompute residual pass.  On an operator whose every leg (table position of the seven-leg base) carries one
 * value in every row pattern that has it -- a constant-coefficient stencil -- the kernel takes the seven values as kernel arguments and keeps a row
 * pair's presence masks in registers instead of looking values up per entry (KRYST_SPMV_LEG_VALUES = 0: the table look-ups; the same bits either
 * way).  info[0] 1 if the operator has one value per leg, info[1] 1 if a recompute residual pass would now take them as arguments (the marching mode
 * and KRYST_CG_RECOMPUTE_AP on); values[0 .. 6] the leg values (+0.0 throughout when info[0] is 0).  info: 2 values, values: 7 */
int32_t kryst_csr_leg_values_info(kryst_csr_t a, int64_t* info, double* values);
int32_t kryst_csr_download(kryst_csr_t a, int64_t* row_ptr, int32_t* col_idx_local, double* vals);
/* Measurement hook (ABI 5): where the CSR arrays live.  The same plain-CSR stream mix runs at 0.70 .. 0.76 of the HBM peak depending on where
 * the driver put the three arrays (round 4, 512^3), so a single-rank creation may try several homes for (row_ptr, col, val) -- K =
 * KRYST_CSR_PLACEMENT_TRIES, default 3 once the arrays exceed 4 GB, else 1 -- time the kernel's traffic skeleton on each and keep the fastest.
 * *tries homes tried, *chosen the one kept, skeleton_ms8[8] the skeleton's milliseconds per launch on each home tried. */
int32_t kryst_csr_placement_info(kryst_csr_t a, int32_t* tries, int32_t* chosen, double* skeleton_ms8);

/* MatVec::matvec (src/core/traits.rs:4-7) == SparseMatrix::spmv (sparse.rs:56-67): y <- A x, y overwritten.  REFUSED: x and y the same
 * vector (KRYST_ERR_ARG before any launch, y unchanged); the same holds for kryst_spmv_transpose. */
int32_t kryst_spmv(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y);
/* MatTransVec::mattransvec (src/core/traits.rs; the reference's CsrMatrix has none): y <- A^T x, x of length nrows, y of length
 * ncols (rectangular operators allowed).  A^T is built on the device by the first call -- row j lists column j of A in ascending row
 * order -- and cached on the operator as an operator of its own, with the same storage-form choice and SpMV kernels as any other;
 * it is freed by kryst_csr_destroy.  Memory: A^T costs about as much as A again (plain CSR at 512^3: about 11 GB).  Distributed
 * operators: KRYST_UNSUPPORTED; length mismatches KRYST_ERR_ARG; device out of memory KRYST_ERR_HIP. */
int32_t kryst_spmv_transpose(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y);
/* operator-level drop-in on host slices (PCIe both ways; plumbing / Jacobi::setup-style callers only) */
int32_t kryst_spmv_host(kryst_csr_t a, const double* x, int64_t nx, double* y, int64_t ny);

/* measurement hook: `reps` back-to-back launches of the SpMV kernel (fused_dots = 0 plain, 1 = the CG kernel
 * with the (x,Ax) partials, 2 = BiCGStab's) between two HIP events on the compute stream; average ms per launch */
int32_t kryst_bench_spmv(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y, int32_t fused_dots, int32_t reps, double* avg_ms);
/* measurement only: average time of one pass of a BLAS-1 stream shape (kind 0: Gram-Schmidt link, 3 vectors; 1: eight batched
 * dots, 9 vectors; 2: CG x/r update, 4 vectors; 3-5: the same with forced nontemporal loads/stores; 6: CG direction update,
 * 2 vectors; 7: CG residual pass r -= a q with (r,r), 2 vectors; 8: CG direction pass with the deferred x update, 3 vectors)
 * over vectors of n doubles placed stride_bytes apart in one allocation */
int32_t kryst_bench_streams(kryst_ctx_t ctx, int64_t n, int64_t stride_bytes, int32_t kind, int32_t reps, double* avg_ms);
/* measurement only: the plain-CSR SpMV's TRAFFIC without its arithmetic on the operator's own CSR arrays -- row pointers, values and
 * column indices streamed, x read once, y written once (SURVEY 8(d)'s bytes; y receives garbage): what this mix of five read streams and
 * one written reaches on this HBM, for `roofline_csr`'s "fraction of what the mix can reach" (bench.py: stream_skeleton) */
int32_t kryst_bench_csr_skeleton(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y, int32_t reps, double* avg_ms);
/* measurement only (ABI 5): average ms per launch of the kernel CG / PCG launch when the direction pass rides inside the SpMV (cg.rs:207-209,274-276 +
 * sparse.rs:107-113 in one pass: z = x, p_old, x-update vectors of its own); KRYST_UNSUPPORTED when the operator has no staged CSR-P16 form */
int32_t kryst_bench_spmv_fused(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y, int32_t reps, double* avg_ms);
/* test hook: fills the LDS of every compute unit with NaNs.  LDS is not cleared between kernels, so whatever a kernel reads from LDS
 * before writing it is what an earlier kernel -- of any process -- left there; a round-4 kernel did, and was wrong on one GPU box in five */
int32_t kryst_bench_poison_lds(kryst_ctx_t ctx);
/* test hook (ABI 6): what lies behind a vector's end.  A vector of n elements is allocated as ceil(n / 512) * 512 + 512 doubles, zero at
 * creation; kernels read past n (16-byte pair loads, shifted and clamped windows) and the pointwise kernels write the whole last tile.
 * Results depend on the first n elements only and the padding after any operation is unspecified; this hook lets a
 * test put something there.  *dirty (may be NULL) receives the number of allocated elements at index >= n whose 64 bits are not +0.0,
 * counted BEFORE any fill; if fill is not NULL every allocated element at index >= n -- the rest of the last tile and the whole extra tile,
 * ceil(n / 512) * 512 + 512 - n elements -- is then set to *fill.  Ordinary stores on the compute stream; elements < n are untouched. */
int32_t kryst_bench_vec_padding(kryst_vec_t v, const double* fill, int64_t* dirty);

/* ---- BLAS-1: InnerProduct for () (src/core/wrappers.rs:90-127) and the solvers' pointwise loops ----
 * Operands that share storage are ALLOWED here and defined element by element: kryst_dot(v, v), kryst_axpy(al, v, v) = v + al * v,
 * kryst_aypx(be, v, v) = v + be * v, kryst_sub with out, a and b the same or different in any combination (every element is read
 * before it is written, by the thread that writes it). */
int32_t kryst_dot(kryst_vec_t x, kryst_vec_t y, double* out);       /* wrappers.rs:90-108 */
int32_t kryst_norm(kryst_vec_t x, double* out);                     /* wrappers.rs:110-127 */
int32_t kryst_axpy(double alpha, kryst_vec_t x, kryst_vec_t y);     /* y[i] = y[i] + alpha*x[i]   cg.rs:207-209 */
int32_t kryst_aypx(double beta, kryst_vec_t x, kryst_vec_t y);      /* y[i] = x[i] + beta*y[i]    cg.rs:274-276 */
int32_t kryst_sub(kryst_vec_t a, kryst_vec_t b, kryst_vec_t out);   /* out[i] = a[i] - b[i]       cg.rs:123 */

/* ---- preconditioners: Preconditioner<M,V>::{setup,apply} (src/preconditioner/mod.rs:8-13) ---- */
enum { KRYST_ILU_KRYST_COMPAT = 0,   /* Ilu0 exactly as written, src/preconditioner/ilu.rs:59-122 */
       KRYST_ILU_ILUP0 = 1,          /* Ilup::new(0) exactly as written, src/preconditioner/ilup.rs:77-167 */
       KRYST_ILU_TRUE_ILU0 = 2 };    /* extension: textbook ILU(0) on A's pattern */
int32_t kryst_pc_identity(kryst_ctx_t ctx, kryst_pc_t* out);                        /* test IdentityPC, pcg.rs:245-251 */
int32_t kryst_pc_jacobi(kryst_csr_t a, kryst_pc_t* out);                            /* Jacobi::setup jacobi.rs:53-73 */
int32_t kryst_pc_ilu0(kryst_csr_t a, int32_t mode, kryst_pc_t* out);                /* Ilu0::setup / Ilup::setup */
/* Ilup::new(fill).setup(a), src/preconditioner/ilup.rs:77-134 exactly as written (level-of-fill p), on sparse rows */
int32_t kryst_pc_ilup(kryst_csr_t a, int32_t fill, kryst_pc_t* out);
/* Ilut::new(fill, droptol).setup(a), src/preconditioner/ilut.rs:80-117 exactly as written */
int32_t kryst_pc_ilut(kryst_csr_t a, int32_t fill, double droptol, kryst_pc_t* out);
int32_t kryst_pc_chebyshev_stub(kryst_ctx_t ctx, int32_t degree, kryst_pc_t* out);  /* Chebyshev trait object: apply -> SolveError, chebyshev.rs:68-70 */
int32_t kryst_pc_chebyshev(kryst_csr_t a, double alpha, double beta, int32_t degree, kryst_pc_t* out); /* extension: apply == apply_chebyshev */
/* EXTENSION (nothing in the reference corresponds; it stands beside the stub Chebyshev::apply, chebyshev.rs:35-70, which returns Err, and
 * beside the filter above): the Chebyshev POLYNOMIAL preconditioner z = p_m(W A) W r of Saad's Alg. 12.1 started from z = 0, DESIGN.md
 * section 4.15.  degree m in 0..64 is the number of SpMVs (m = 0: a scaled Jacobi); 0 < lo < hi, both finite, bound the spectrum of W A;
 * scaling KRYST_CHEB_SCALE_JACOBI takes W = kryst_pc_jacobi's inv_diag exactly as that forms it (jacobi.rs:69-71: 0.0 where the diagonal is
 * missing or zero), KRYST_CHEB_SCALE_NONE multiplies by nothing.  Host scalars, in double, un-fused: theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
 * rho_k = 1 / (2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = (2 rho_k) / delta.  Vectors: d_0 = (w r) / theta, z_0 = d_0, res_0 = r;
 * step k: y = A d_{k-1} (the row sum of kryst_spmv), res_k = res_{k-1} - y, t = w res_k, d_k = c1_k d_{k-1} + c2_k t, z_k = z_{k-1} + d_k.
 * SpMVs and pointwise passes only: row-partitioned operators are taken.  The step runs fused in one kernel on the plain CSR arrays where the
 * operator is on one rank and has no compressed form (kryst_csr_encoding == 0 at creation), else as kryst_spmv + one pointwise pass: the same
 * bits.  a is borrowed.  KRYST_ERR_ARG: non-square operator, degree outside 0..64, lo <= 0, lo >= hi, non-finite bounds, unknown scaling. */
enum { KRYST_CHEB_SCALE_NONE = 0, KRYST_CHEB_SCALE_JACOBI = 1 };
int32_t kryst_pc_chebyshev_poly(kryst_csr_t a, int32_t degree, int32_t scaling, double lo, double hi, kryst_pc_t* out);
/* extension (beside chebyshev.rs:35-70): what a kryst_pc_chebyshev_poly object holds; *fused = 1 when its step is the fused kernel.  Any
 * pointer may be NULL.  Another kind of preconditioner: KRYST_ERR_ARG. */
int32_t kryst_pc_chebyshev_poly_info(kryst_pc_t pc, int32_t* degree, int32_t* scaling, double* lo, double* hi, int32_t* fused);
/* extension (beside chebyshev.rs:35-70, whose bounds the caller must know): bounds for kryst_pc_chebyshev_poly.  min(steps, n) Lanczos steps
 * without reorthogonalisation on S = W^1/2 A W^1/2 (scaling as above; none: S = A) from q_0 = u / sqrt(dot(u, u)), u =
 * kryst_vec_fill_splitmix(seed, 0): v = s q_j, y = A v, t = s y, alpha_j = dot(q_j, t), t = t - alpha_j q_j, t = t - beta_{j-1} q_{j-1}
 * (j > 0), beta_j = sqrt(dot(t, t)), stop when beta_j is zero or not finite, q_{j+1} = t / beta_j; every dot in the order of
 * kryst_reduce_spec.  alpha_out / beta_out (room for `steps` entries each) receive *steps_done coefficients; *theta_min / *theta_max are
 * kryst_host_tridiag_extreme_eigs of them; *gershgorin = max_i((sum_k |a_ik|) w_i), a true upper bound.  steps in 1..64.  Errors:
 * KRYST_ERR_ARG (non-square or empty operator, steps, scaling), KRYST_UNSUPPORTED (a distributed operator: pass bounds),
 * KRYST_INDEFINITE_PRECONDITIONER (Jacobi scaling and a diagonal entry that is missing, not finite or <= 0, or whose reciprocal overflows;
 * the row in kryst_hip_last_error_row()), KRYST_FACTOR_ERROR (a non-finite Gershgorin bound), KRYST_INDEFINITE_MATRIX
 * (theta_max <= 0 or not finite; the outputs are filled). */
int32_t kryst_spectrum_estimate(kryst_csr_t a, int32_t scaling, int32_t steps, uint64_t seed, double* alpha_out, double* beta_out,
                                int32_t* steps_done, double* theta_min, double* theta_max, double* gershgorin);
/* ApproxInv with GIVEN inverse rows (ApproxInv::inv_rows, approxinv.rs:66): apply (approxinv.rs:268-298) is the sparse-row
 * product z = M r, i.e. kryst_spmv with M.  m is borrowed (must outlive the preconditioner).  ApproxInv::setup -- a
 * least-squares fit per column through faer's QR (approxinv.rs:129-264) -- stays on the host with the reference. */
int32_t kryst_pc_approx_inverse(kryst_csr_t m, kryst_pc_t* out);
/* BlockJacobi::setup (src/preconditioner/block_jacobi.rs:39-62) + apply (:69-106) as a device Preconditioner on the CSR operator.
 * blk_ptr / blk_idx: the index sets packed like CSR rows (blk_ptr[0] = 0, nblocks + 1 entries), in the given order, each unsorted.
 * z = 0, then every block in order writes z[g[i]] = (B^-1 r|_g)[i]: the last block that contains a row decides it, a row in no block
 * stays +0.0; empty blocks do nothing.  Labelled deviations: each block is inverted explicitly by Gauss-Jordan with full pivoting
 * (the reference keeps faer's FullPivLu); each index set is sorted ascending first; KRYST_ZERO_PIVOT (kryst_hip_last_error_row() =
 * the global row of the smallest block position not yet pivoted), KRYST_FACTOR_ERROR (NaN / Inf in a block), KRYST_ERR_ARG (index out
 * of range or repeated in a block, non-square operator), KRYST_UNSUPPORTED (a block of more than 64 rows, a distributed operator) where
 * the reference gives non-finite z or panics.  a is borrowed (must outlive the preconditioner). */
int32_t kryst_pc_block_jacobi(kryst_csr_t a, const int64_t* blk_ptr, const int64_t* blk_idx, int64_t nblocks, kryst_pc_t* out); /* BlockJacobi::setup block_jacobi.rs:39-62 */
int32_t kryst_pc_block_jacobi_uniform(kryst_csr_t a, int32_t bsize, kryst_pc_t* out);   /* extension: contiguous blocks of bsize rows, the last one shorter */
/* the preconditioner as the CSR matrix M with z = M r: row g[i] of the block that owns it stores (g[j], Binv[i][j]) for every j of the
 * block, ascending; other rows are empty.  row_ptr == NULL: *nnz only; else row_ptr (n + 1), col and val (*nnz each) are filled. */
int32_t kryst_pc_block_jacobi_export(kryst_pc_t pc, int64_t* nnz, int64_t* row_ptr, int32_t* col, double* val);
/* AdditiveSchwarz::new(overlap, subdomains) + setup + apply (src/preconditioner/asm.rs:34-119) with the direct solve as the inner
 * solver, as a device Preconditioner on the CSR operator.  sub_ptr / sub_idx: the subdomains packed like CSR rows
 * (sub_ptr[0] = 0, nsub + 1 entries), unsorted, possibly overlapping, possibly leaving rows uncovered.  The apply is asm.rs:76-119:
 * z = 0, then for every subdomain in ascending order z[g[i]] = z[g[i]] + (B^-1 r|_g)[i] (a row in no subdomain stays +0.0).
 * variant KRYST_ASM_AS_WRITTEN ignores `overlap`, as the reference does; KRYST_ASM_GROWN (labelled extension) first grows every subdomain
 * by `overlap` layers of the symmetrised graph of A (row i's neighbours: the stored columns of rows i of A and of A^T, i excluded);
 * KRYST_ASM_RESTRICTED (RAS, labelled extension) grows them too and keeps, for every row, only the product of the last un-grown
 * subdomain that contains it.  Labelled deviations, those of kryst_pc_block_jacobi: explicit Gauss-Jordan inverses, index sets sorted
 * ascending, KRYST_ZERO_PIVOT (kryst_hip_last_error_row() = the global row), KRYST_FACTOR_ERROR (NaN / Inf), KRYST_ERR_ARG (index out of
 * range or repeated in a subdomain, non-square operator, overlap < 0), KRYST_UNSUPPORTED (a subdomain of more than KRYST_ASM_MAX_ROWS
 * rows, before or after growth -- the message names it --, a distributed operator).  The set-up checks the device memory it needs
 * (8 sum b_k^2 bytes of tiles and the index streams) against hipMemGetInfo -- for the un-grown sets before it allocates anything, for
 * the grown ones again before the tiles --, giving the library's device pool back to the driver first when the figure falls short:
 * KRYST_ERR_HIP with the byte count in kryst_hip_last_error() when it does not fit.  a is borrowed (must outlive the preconditioner). */
enum { KRYST_ASM_AS_WRITTEN = 0, KRYST_ASM_GROWN = 1, KRYST_ASM_RESTRICTED = 2, KRYST_ASM_MAX_ROWS = 128 };
int32_t kryst_pc_asm(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant, kryst_pc_t* out);
/* asm.rs:46-56, the subdomains left empty: p = max(nparts, 1) parts of chunk = ceil(n / p) rows, part i = [i chunk, min((i + 1) chunk, n));
 * trailing parts may be empty.  nparts stands for the reference's subdomains.capacity() (0 for Vec::new(): ONE subdomain of all n rows). */
int32_t kryst_pc_asm_uniform(kryst_csr_t a, int64_t nparts, int32_t overlap, int32_t variant, kryst_pc_t* out);
/* the subdomain count, the sum of their (grown) rows and the largest; any pointer may be NULL */
int32_t kryst_pc_asm_info(kryst_pc_t pc, int64_t* nsub, int64_t* ext_rows, int32_t* max_rows);
/* the set-up, downloaded; any pointer may be NULL (size them with kryst_pc_asm_info and a first call for sub_ptr): sub_ptr (nsub + 1) and
 * sub_idx (ext_rows) the grown subdomains sorted ascending, owner (n) the last un-grown subdomain that contains each row or -1, tiles
 * (sum b_k^2) the inverses subdomain after subdomain, column-major inside a tile (tiles[off_k + j b_k + i] = Binv_k[i][j]). */
int32_t kryst_pc_asm_export(kryst_pc_t pc, int64_t* sub_ptr, int32_t* sub_idx, int32_t* owner, double* tiles);

/* Additive Schwarz with ILU(0) subdomain solves (labelled extension of AdditiveSchwarz::setup's `solver_factory`, asm.rs:38-40; DESIGN.md
 * section 4.13).  Index sets, growth, owners, variants, the uniform partition and the combine are those of kryst_pc_asm; the inner solver of
 * subdomain k is an incomplete factorisation of S_k = A[g_k, g_k] (sorted g_k; every stored entry kept, explicit zeros included; columns outside
 * g_k dropped): sub_mode KRYST_ILU_ILUP0 is Ilup::new(0) as written (ilup.rs:77-167), KRYST_ILU_TRUE_ILU0 the textbook IKJ ILU(0) on S_k's
 * pattern, both applied as ilup.rs:138-167 does (a factor entry equal to 0.0 takes no part; the division only by a stored non-zero diagonal);
 * KRYST_ILU_KRYST_COMPAT is KRYST_UNSUPPORTED.  The apply solves every subdomain in one workgroup with its vector in LDS.  Errors: those of
 * kryst_pc_asm for the sets; those of kryst_pc_ilu0 for the factors (KRYST_ZERO_PIVOT / KRYST_SOLVE_ERROR, the row a row of A in the message
 * and in kryst_hip_last_error_row(), the lowest-numbered failing subdomain); KRYST_UNSUPPORTED for a subdomain of more than
 * KRYST_ASM_ILU_MAX_ROWS rows before or after growth (the message names the cap), a context of several ranks, a distributed operator;
 * KRYST_ERR_HIP with byte counts when the device memory does not suffice.  a is borrowed (must outlive the preconditioner). */
enum { KRYST_ASM_ILU_MAX_ROWS = 16384, KRYST_ASM_ILU_INFO_COUNT = 10 };
int32_t kryst_pc_asm_ilu(kryst_csr_t a, const int64_t* sub_ptr, const int64_t* sub_idx, int64_t nsub, int32_t overlap, int32_t variant,
                         int32_t sub_mode, kryst_pc_t* out);
int32_t kryst_pc_asm_ilu_uniform(kryst_csr_t a, int64_t nparts, int32_t overlap, int32_t variant, int32_t sub_mode, kryst_pc_t* out);
/* the first min(count, KRYST_ASM_ILU_INFO_COUNT) of: nsub, ext_rows (the sum of the grown subdomain rows), max_rows, nnz_L and nnz_U (the kept,
 * i.e. non-zero, entries strictly below / strictly above the diagonal), the largest level count of a sweep, the LDS bytes per workgroup of
 * the apply, the cap KRYST_ASM_ILU_MAX_ROWS, nnz_S (the stored entries of all submatrices), the entries of the padded level layouts */
int32_t kryst_pc_asm_ilu_info(kryst_pc_t pc, int64_t* info, int32_t count);
/* the set-up, downloaded; any pointer may be NULL: sub_ptr (nsub + 1), sub_idx (ext_rows) and owner (n) as kryst_pc_asm_export gives them;
 * the factors on the submatrices' patterns, subdomain after subdomain: ent_ptr (nsub + 1) the first entry of every subdomain, row_ptr
 * (ext_rows + nsub: b_k + 1 row pointers per subdomain, relative to ent_ptr[k]), col (nnz_S, local columns = positions in g_k, ascending
 * within a row), val (nnz_S: l_ij below the diagonal, u_ij on and above it); lev_l and lev_u (ext_rows): every row's level (from 1) in the
 * forward and in the backward sweep */
int32_t kryst_pc_asm_ilu_export(kryst_pc_t pc, int64_t* sub_ptr, int32_t* sub_idx, int32_t* owner, int64_t* ent_ptr, int32_t* row_ptr, int32_t* col,
                                double* val, int32_t* lev_l, int32_t* lev_u);

/* Sor::new(omega, its, lits, sym, fshift) + setup + apply (src/preconditioner/sor.rs:71-170) as a device preconditioner on the CSR operator
 * (DESIGN.md section 4.11).  sym_bits: the MatSorType bits below.  Set-up: inv_diag[i] = 1 / (a_ii + fshift), a row without a stored
 * diagonal counts as a_ii = 0; a sum of exactly zero is KRYST_ZERO_PIVOT with the lowest such row in kryst_hip_last_error_row().  apply:
 * y = +0.0, then `its` times the forward sweep (APPLY_LOWER) and / or the backward sweep (APPLY_UPPER) exactly as written, every operation
 * rounded on its own; `lits` and the ZERO_INITIAL_GUESS / LOCAL_* bits are stored and not used, as written.  The input and the output of an
 * apply must be different vectors.  `colors` (labelled extension, the reference's PC::Multicolor has no implementation): NULL, or one
 * non-negative colour per row; the sweeps then visit the rows by (colour, row) ascending (forward) and in the exact reverse (backward), "before"
 * and "after" mean positions in that order and the terms of a group are summed in ascending position: the loops as written on P A P^T
 * with P x, un-permuted.  Either way one persistent launch per sweep walks the dependency levels of the (permuted) pattern with a grid barrier between
 * them.  Errors: KRYST_ERR_ARG (non-square operator, negative its / lits / colour, unknown bits), KRYST_UNSUPPORTED (distributed operator),
 * KRYST_ZERO_PIVOT; also KRYST_UNSUPPORTED when levels x workgroups of a sweep reach 2^32.  kryst_pc_apply, kryst_bench_pc_apply, kryst_pc_destroy and every solver take the result. */
enum { KRYST_SOR_ZERO_INITIAL_GUESS = 1, KRYST_SOR_APPLY_LOWER = 2, KRYST_SOR_APPLY_UPPER = 4, KRYST_SOR_SYMMETRIC_SWEEP = 6,
       KRYST_SOR_LOCAL_FORWARD_SWEEP = 8, KRYST_SOR_LOCAL_BACKWARD_SWEEP = 16, KRYST_SOR_LOCAL_SYMMETRIC_SWEEP = 24, KRYST_SOR_EISENSTAT = 32 };
int32_t kryst_pc_sor(kryst_csr_t a, double omega, int64_t its, int64_t lits, uint32_t sym_bits, double fshift, const int32_t* colors, kryst_pc_t* out);
/* dependency levels (= grid-barrier separated passes) of the forward / backward sweep (0 for a sweep sym_bits does not ask for), rows, and the
 * workgroups (of 1024 threads) a forward / backward sweep launches: min(CUs, ceil(widest level / 1024)); any pointer may be NULL */
int32_t kryst_pc_sor_info(kryst_pc_t pc, int32_t* groups_forward, int32_t* groups_backward, int64_t* rows, int32_t* grid_forward,
                          int32_t* grid_backward);
/* ApproxInv::setup (src/preconditioner/approxinv.rs:123-264) on the device: column j of M minimises || A m_j - e_j ||_2 over the
 * vectors with support J_j; inv_rows[i] = the (j, M_ij) with |M_ij| > tol (strict: 0 and NaN are dropped), ascending j.  The apply is
 * kryst_pc_approx_inverse's (approxinv.rs:268-298); M is owned by the preconditioner.  pattern_kind: KRYST_SPAI_MANUAL
 * (SparsityPattern::Manual(pat), approxinv.rs:125, 146: n = pat.len() = pat_n, J_j = pat_idx[pat_ptr[j] .. pat_ptr[j+1])),
 * KRYST_SPAI_AUTO (as written: KRYST_UNSUPPORTED, approxinv.rs:127-133 -- its downcasts at :301-323 never succeed), KRYST_SPAI_OPERATOR
 * (extension: J_j = the stored columns of row j of A, what Auto's code was meant to do; pat_* are ignored).  max_iter, nbsteps and the
 * other tuning fields of ApproxInv::new are unused, as in the reference.  Labelled deviations: each J_j is sorted ascending; the least
 * squares is solved on the reduced problem A[I_j, J_j] (I_j = the stored rows of the columns J_j: the same minimiser) by Householder QR
 * instead of faer's FullPivLu / Qr::solve_lstsq (values agree to rounding); KRYST_ERR_ARG (pattern of the wrong length, index out of
 * range or repeated within a column, non-square operator), KRYST_FACTOR_ERROR (a zero Householder column, a non-finite A[I_j, J_j] or
 * m_j; the message names the column), KRYST_UNSUPPORTED (a distributed operator; a column over the caps: |J_j| <= 64, at most 2048
 * stored entries in A[:, J_j], |I_j| <= 128; or, inside the caps, tiles sized by the widest columns that exceed the device's LDS per
 * workgroup -- DESIGN.md section 4.6) where the reference panics or gives non-finite output.  a is not kept. */
enum { KRYST_SPAI_MANUAL = 0, KRYST_SPAI_AUTO = 1, KRYST_SPAI_OPERATOR = 2 };
int32_t kryst_pc_spai(kryst_csr_t a, int32_t pattern_kind, const int64_t* pat_ptr, const int64_t* pat_idx, int64_t pat_n, double tol,
                      kryst_pc_t* out);                                                 /* ApproxInv::setup approxinv.rs:123-264 */
/* inv_rows (approxinv.rs:66) of a SPAI preconditioner as CSR: row_ptr == NULL: *nnz only; else row_ptr (n + 1), col and val (*nnz each) */
int32_t kryst_pc_spai_export(kryst_pc_t pc, int64_t* nnz, int64_t* row_ptr, int32_t* col, double* val);
/* AMG (src/preconditioner/amg.rs) with its V-cycle on the device (kryst_amd/csrc/amg.hip).  variant
 * KRYST_AMG_AS_WRITTEN: AMG::new(a, max_levels, threshold) (amg.rs:73-118) with every quirk, set up on the host (kryst_host_amg) and
 * uploaded; the apply is apply_recursive (:200-250): nu_pre / nu_post undamped Jacobi sweeps (the reference fixes both at 1, :115-116)
 * around the coarse correction, the finest level starting from the INCOMING z, coarse levels from zero, and on the coarsest level
 * solve_direct (:254-312): CG from zero for up to n iterations, stopped on the device when sqrt(r.r) < 1e-10.  The coarsest level
 * may hold at most KRYST_AMG_DIRECT_MAX rows (else KRYST_UNSUPPORTED: its CG runs in one workgroup).  KRYST_AMG_SMOOTHED: the labelled
 * extension, textbook smoothed aggregation set up on the device (threshold = theta of |a_ij| > theta sqrt(|a_ii a_jj|); distance-2 MIS
 * aggregates; P = (I - 4/(3 rho) D^-1 A) P0; R = P^T; A_c = R (A P); stop at <= 64 rows, max_levels >= 1 levels or n_c > 0.8 n; block
 * Jacobi of 64 rows on the coarsest level); its apply starts from z = 0 with nu_pre / nu_post damped Jacobi sweeps, and a zero diagonal
 * is KRYST_ZERO_PIVOT.  Export which 3 then gives omega D^-1, which 4 the aggregates (col).  Errors: KRYST_ERR_ARG (non-square operator,
 * rows not strictly ascending, max_levels / nu_pre / nu_post < 0), KRYST_UNSUPPORTED (a distributed operator), KRYST_FACTOR_ERROR (a level over the fill budget of kryst_host_amg).
 * a is borrowed (must outlive the preconditioner); the coarse levels are owned. */
enum { KRYST_AMG_AS_WRITTEN = 0, KRYST_AMG_SMOOTHED = 1, KRYST_AMG_DIRECT_MAX = 4096 };
int32_t kryst_pc_amg(kryst_csr_t a, int32_t max_levels, double threshold, int32_t variant, int32_t nu_pre, int32_t nu_post, kryst_pc_t* out);
/* *nlevels, and per level (count >= nlevels entries; either array may be NULL) the rows and the stored entries of A_l */
int32_t kryst_pc_amg_info(kryst_pc_t pc, int32_t* nlevels, int64_t* rows, int64_t* nnz, int32_t count);
/* A_l (which 0), P_l (1, n_l x n_{l+1}), R_l (2, n_{l+1} x n_l), D_l^-1 (3: nrows entries in val) or the aggregates (4, smoothed aggregation:
 * nrows entries in col) of the device hierarchy, downloaded.
 * P / R of the last level are empty (0 x 0).  row_ptr == NULL: the sizes only; else row_ptr (nrows + 1), col and val (*nnz each). */
int32_t kryst_pc_amg_export(kryst_pc_t pc, int32_t level, int32_t which, int64_t* nrows, int64_t* ncols, int64_t* nnz, int64_t* row_ptr,
                            int32_t* col, double* val);
/* Preconditioner::apply(&self, r: &V, z: &mut V).  REFUSED for every kind: r and z the same handle or the same device storage
 * (KRYST_ERR_ARG before any launch, both vectors unchanged) -- the Rust signature cannot alias either, and most applies would race or
 * overwrite their own input.  The same rule holds for kryst_bench_pc_apply and kryst_apply_chebyshev. */
int32_t kryst_pc_apply(kryst_pc_t pc, kryst_vec_t r, kryst_vec_t z);
int32_t kryst_pc_destroy(kryst_pc_t pc);
/* measurement hooks (bench.py): average ms of `reps` back-to-back applies between two HIP events on the compute stream; and what
 * an ILU-family preconditioner's apply runs and streams -- info[0] form (0 level-ordered, 1 grid 8 x 8 lines per workgroup,
 * 2 grid 16 x 16, 3 plane kernels after a give-up), [1..3] Ni Nj Nk, [4..5] dependency levels of L / U, [6..7] coefficient chunks
 * forward / backward, [8..9] of which repeat and are not requested, [10..11] bytes per chunk request, [12] reserved; count >= 13 */
int32_t kryst_bench_pc_apply(kryst_pc_t pc, kryst_vec_t r, kryst_vec_t z, int32_t reps, double* avg_ms);
int32_t kryst_pc_ilu_info(kryst_pc_t pc, int64_t* info, int32_t count);
/* apply_chebyshev(a, r, z, alpha, beta, m), src/preconditioner/chebyshev.rs:83-140 */
int32_t kryst_apply_chebyshev(kryst_csr_t a, kryst_vec_t r, kryst_vec_t z, double alpha, double beta, int64_t m);

/* ---- solvers: LinearSolver<M,V>::solve (src/solver/mod.rs:30-52) ---- */
typedef struct {
    double  tol;                 /* Convergence::tol      src/utils/convergence.rs:4-7 */
    int64_t max_iters;           /* Convergence::max_iters */
    int32_t restart;             /* GmresSolver::restart  gmres.rs:40 */
    int32_t precond_side;        /* gmres.rs:28-32 Preconditioning: 0 None, 1 Left (default), 2 Right; 3 = textbook Left, a labelled extension (kryst_gmres_solve) */
    int32_t norm_type;           /* CgNormType cg.rs:35: 0 Preconditioned, 1 Unpreconditioned (default), 2 Natural, 3 None */
    int32_t single_reduction;    /* with_single_reduction cg.rs:69 (same fold on the device; accepted, no effect) */
    int32_t has_radius;  double radius;        /* with_radius     cg.rs:74  (CG: trust-region exit cg.rs:177-202; PCG ignores it like the reference) */
    int32_t has_obj_target; double obj_target; /* with_obj_target cg.rs:79  (CG: objective exit cg.rs:231-252) */
    int32_t check_every;         /* host polls the device convergence flag every this many iterations (0 = default);
                                    the device stops at the exact reference iteration regardless */
} kryst_params_t;

typedef struct {                 /* SolveStats src/utils/convergence.rs:10-14 */
    int64_t iterations;
    double  final_residual;
    int32_t converged;
} kryst_stats_t;

typedef void (*kryst_monitor_fn)(int64_t iteration, double residual, void* user);   /* with_monitor cg.rs:84 */

/* Residual history: hist[0..min(*hist_len,hist_cap)) receives what CgSolver/PcgSolver push to
 * residual_history (cg.rs:140,263; pcg.rs:146,199); GMRES / BiCGStab record |g[j+1]| / ||r|| per iteration
 * (an addition: the reference keeps none).  At most 2^22 entries are recorded per solve; *hist_len counts every push.
 * monitor (if non-NULL) is LIVE like the reference's (cg.rs:137-140,260-263; pcg.rs:143-146,196-199): the device
 * publishes each history entry to mapped host memory and the host fires monitor(iteration, residual, user) on the
 * calling thread, in order, every time its poll loop has waited for a batch of params->check_every iterations
 * (default 8; 1 = after every iteration; GMRES / FGMRES: once per restart cycle) and for the remaining entries when
 * the solve ends -- always before the call returns.  The callback must not call into the same context. */
#define KRYST_SOLVE_ARGS kryst_csr_t a, kryst_pc_t pc /* NULL = None */, \
        const kryst_params_t* params, kryst_stats_t* stats, \
        double* hist, int64_t hist_cap, int64_t* hist_len, kryst_monitor_fn monitor, void* user

/* b, x on the host (x in/out = initial guess / solution), exactly the reference call shape */
int32_t kryst_cg_solve      (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);  /* CgSolver::solve       cg.rs:114-288 */
int32_t kryst_pcg_solve     (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);  /* PcgSolver::solve      pcg.rs:114-222 */
int32_t kryst_gmres_solve   (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);  /* GmresSolver::solve    gmres.rs:216-402 */
int32_t kryst_bicgstab_solve(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);  /* BiCgStabSolver::solve bicgstab.rs:69-293 */
/* same with b, x resident in HBM (the performant drop-in; bench.py times these).  ALLOWED for every *_solve_dev and for a stepping
 * session: b and x the same vector (x0 = b; every solver iterates on a copy and writes x once at the end: the vector holds x afterwards) */
int32_t kryst_cg_solve_dev      (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_pcg_solve_dev     (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_gmres_solve_dev   (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_bicgstab_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
/* extension: right-preconditioned BiCGStab (the reference ignores pc, bicgstab.rs:70) */
int32_t kryst_bicgstab_rpc_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);

/* CgsSolver::solve (src/solver/cgs.rs:58-135) and TfqmrSolver::solve (src/solver/tfqmr.rs:64-221).  Both ignore pc like the
 * reference (cgs.rs:59, tfqmr.rs:66); TFQMR also overwrites the initial guess with zeros (tfqmr.rs:72).  History (an
 * addition): ||r|| per iteration (CGS), the residual estimate dpest per substep, two per iteration (TFQMR). */
int32_t kryst_cgs_solve      (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);
int32_t kryst_tfqmr_solve    (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);
int32_t kryst_cgs_solve_dev  (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_tfqmr_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
/* MinresSolver::solve (src/solver/minres.rs:60-219), QmrSolver::solve (src/solver/qmr.rs:61-166) and CgnrSolver::solve
 * (src/solver/cgnr.rs:77-132), as written; CgneSolver::solve (cgnr.rs:153-208) does the same floating-point operations and binds
 * to kryst_cgnr_solve[_dev].  All three ignore pc (minres.rs:61, qmr.rs:64, cgnr.rs:78); history (an addition) = the value each
 * passes to Convergence::check.  MINRES: x0 enters r0 only, x_out starts from zero (minres.rs:72-77, :94); x = x_best, the iterate
 * of the smallest |phi_bar| estimate, final_residual = phi_min (:207-218); the estimate is not the true residual.  QMR: a
 * BiCGStab-type loop whose A^T p_tld is never read (qmr.rs:121-122, dropped here), stopping on ||b - A x_j|| (:146-152).  CGNR:
 * A where A^T is meant and ||A(Ap)||^2 as the denominator (cgnr.rs:84, :94-97, :105), without a guard. */
int32_t kryst_minres_solve    (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);
int32_t kryst_qmr_solve       (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);
int32_t kryst_cgnr_solve      (const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS);
int32_t kryst_minres_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_qmr_solve_dev   (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_cgnr_solve_dev  (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
/* extensions (not in the reference; pc ignored): textbook MINRES (Paige & Saunders 1975, unpreconditioned) from x0, last
 * iterate returned, stop on |phi_bar_k| / beta_1 <= tol or the cap (reported like Convergence::check), beta_{k+1} = 0 an exact exit
 * with converged = true; textbook CGNR (Saad, Iterative Methods for Sparse Linear Systems, section 8.3) with z = A^T r through
 * kryst_spmv_transpose's cached A^T, stop on ||r|| / ||r0||.  History: |phi_bar_k| / ||r|| per iteration. */
int32_t kryst_minres_textbook_solve_dev(kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
int32_t kryst_cgnr_textbook_solve_dev  (kryst_vec_t b, kryst_vec_t x, KRYST_SOLVE_ARGS);
/* FgmresSolver::solve_flex (src/solver/fgmres.rs:114-340); pc plays the FlexiblePreconditioner (preconditioner/mod.rs:16-19),
 * NULL = None.  params: tol, max_iters, restart (fgmres.rs:52-54).  orthog: OrthogMethod 0 Classical (default, :59) /
 * 1 Modified; haptol: happy-breakdown tolerance (default 1e-12, :60); preallocate: set_preallocate_vectors (:77; only
 * the cycle length `m` depends on it, :203).  History = what residual_history receives (:292). */
int32_t kryst_fgmres_solve    (const double* b, double* x, int64_t n, int32_t orthog, double haptol, int32_t preallocate, KRYST_SOLVE_ARGS);
int32_t kryst_fgmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t orthog, double haptol, int32_t preallocate, KRYST_SOLVE_ARGS);

/* PcaGmresSolver::solve (src/solver/pca_gmres.rs:99-312) as written with the default features: x starts from zero whatever the caller
 * passes (:107) and receives the result (:310); no orthogonalisation (the subtraction is under cfg(feature = "mpi"), :181-204);
 * Right (params->precond_side 2) applies pc after A (:152,164), Left (1, the default, :61) and None (0) never call it; the stopping
 * block's column stays out of the update (:277); converged = ||b - A x|| <= tol ||r0|| (:304).  restart and side come from params;
 * pipeline_depth and tau are accepted and never read (:40-45).  Deviations where the reference panics or never returns:
 * block_size >= 2 with restart >= 2 and max_iters >= 1 (:145,151,163), block_size = 0 (:273) or restart = 0 (:120) return
 * KRYST_ERR_ARG with x untouched.  History = |g[j+t]| handed to Convergence::check (:266-268), one per block.  Distributed
 * operators: KRYST_UNSUPPORTED. */
int32_t kryst_pca_gmres_solve    (const double* b, double* x, int64_t n, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS);
int32_t kryst_pca_gmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS);
/* extension (not in the reference; pca_gmres.rs:10 names it): s-step GMRES(restart) from x0, right preconditioned, block_size = s in
 * 1..16 -- scaled monomial blocks, BCGS2 against the basis, CholQR2 within the block, columns whose first pivot keeps less than 1e-6 of
 * their length dropped (column 0: happy breakdown).  Left with a pc: KRYST_UNSUPPORTED.  History: |g_{c+1}| per column; the stop is
 * exact to the column; converged = ||b - A x|| <= tol ||r0|| at a cycle end. */
int32_t kryst_pca_gmres_textbook_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t block_size, int32_t pipeline_depth, double tau, KRYST_SOLVE_ARGS);

/* extension (not in the reference): compressed-basis GMRES(restart) -- the Krylov basis V is STORED in fp32 (basis = KRYST_BASIS_F32), everything
 * else is fp64: the operator (every SpMV encoding as it is), the preconditioner (every kind), z, x, the Hessenberg matrix, all scalars and all
 * arithmetic.  A basis vector is rounded once, (float) round-to-nearest-even, when it is stored; every later use widens exactly what was stored;
 * the true residual is recomputed in fp64 at every restart, so the fp32 basis does not cap the attainable accuracy.  KRYST_BASIS_F64 is the control:
 * the same loop with nothing rounded.  params: tol, max_iters, restart (1..4096), precond_side.  Side 0 or pc == NULL: the loop of
 * kryst_gmres_solve_dev side 0, statement for statement (with KRYST_BASIS_F64: its bits).  Side 2: TEXTBOOK right preconditioning -- a deviation
 * from the as-written Right arm of gmres.rs: Arnoldi on A M^-1 from the true residual, v0 = r0 / ||r0||, only V kept, x += M^-1 (sum_j y_j V_j)
 * with one apply per cycle.  Sides 1 and 3 and contexts of several ranks: KRYST_UNSUPPORTED; basis outside {0, 1}, restart outside 1..4096:
 * KRYST_ERR_ARG; x untouched on every error.  History: |g[j+1]| per iteration, as kryst_gmres_solve_dev. */
enum { KRYST_BASIS_F64 = 0, KRYST_BASIS_F32 = 1 };
int32_t kryst_cbgmres_solve_dev(kryst_vec_t b, kryst_vec_t x, int32_t basis, KRYST_SOLVE_ARGS);

/* ---- stepping session: the same solver split into begin / step / end, so that a caller (bench.py) can
 * enqueue and time exactly K iterations.  method: 0 CgSolver, 1 PcgSolver, 2 BiCgStabSolver, 3 CgsSolver, 4 TfqmrSolver,
 * 5 MinresSolver, 6 QmrSolver, 7 CgnrSolver (all three as written), 8 textbook MINRES, 9 textbook CGNR (extensions).
 * step() enqueues up to k further iterations (never past max_iters) without synchronising the host. ---- */
typedef struct kryst_session_s* kryst_session_t;
int32_t kryst_session_begin(int32_t method, kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_pc_t pc,
                            const kryst_params_t* params, kryst_session_t* out);
int32_t kryst_session_step(kryst_session_t s, int64_t k);
/* A session that is begun must be ended (the context stays busy until then: KRYST_ERR_BUSY for every other solve).  If an ILU
 * preconditioner's wavefront solve gave up during the session (see kryst_pc_ilu0), kryst_session_end returns KRYST_SOLVE_ERROR
 * once -- the preconditioner has switched to its plane kernels and the caller repeats the session; the one-shot kryst_*_solve
 * entry points repeat the solve themselves. */
int32_t kryst_session_end(kryst_session_t s, kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len);

/* ---- dense storage and the direct solvers: DenseMatrix (src/matrix/dense.rs), LuSolver / QrSolver (src/solver/direct_lu.rs) ----
 * Labelled deviation: the reference keeps faer's FullPivLu / Qr; these are the textbook factorizations -- LU with
 * full pivoting (largest |w_ij| of the trailing block, the smaller row and then the smaller column on a tie), Householder QR -- in the
 * operation order section 4.12 fixes: fp64, every operation rounded on its own, true divisions, column sweeps.  The host twins below and the
 * device compute the same bits.  Square systems of at most KRYST_DENSE_MAX rows: more is KRYST_UNSUPPORTED, a non-square matrix
 * KRYST_ERR_ARG, a context of several ranks KRYST_UNSUPPORTED.  KRYST_ZERO_PIVOT (kryst_hip_last_error_row() = the step) on a zero pivot /
 * zero Householder column, KRYST_FACTOR_ERROR on a NaN or Inf in the matrix or in a pivot; x is untouched on every error.  Stats are
 * direct_lu.rs:84-88 (iterations 1, final_residual 0.0, converged); pc is accepted and ignored (direct_lu.rs:70, :123).
 * ALIASING: b and x may be the same vector (the reference copies b into x and solves in place); every other overlap of b, x and the
 * matrix is refused with KRYST_ERR_ARG. */
enum { KRYST_DENSE_MAX = 4096 };
typedef struct kryst_dense_s* kryst_dense_t;
typedef struct kryst_lu_s*    kryst_lu_t;
/* DenseMatrix::from_raw(nrows, ncols, data) (dense.rs:16-25): data column-major, data[i + j * nrows]; colmajor == 0 (extension): row-major input */
int32_t kryst_dense_create(kryst_ctx_t ctx, int64_t nrows, int64_t ncols, const double* data, int32_t colmajor, kryst_dense_t* out);
/* extension: the operator densified on the device, absent entries +0.0 (a CSR operator holds no column twice in a row: kryst_csr_create checks
 * new_checked's strictly ascending columns, so every entry has a place of its own) */
int32_t kryst_dense_from_csr(kryst_csr_t a, kryst_dense_t* out);
int32_t kryst_dense_shape(kryst_dense_t a, int64_t* nrows, int64_t* ncols);         /* nrows() / ncols() dense.rs:32-37 */
int32_t kryst_dense_download(kryst_dense_t a, double* colmajor);
int32_t kryst_dense_destroy(kryst_dense_t a);
/* MatVec for DenseMatrix (core/wrappers.rs:27-38): y[i] = +0.0, then y[i] = y[i] + a[i][j] * x[j] for ascending j; rectangular allowed;
 * x and y sharing storage: KRYST_ERR_ARG */
int32_t kryst_dense_matvec(kryst_dense_t a, kryst_vec_t x, kryst_vec_t y);
int32_t kryst_lu_create(kryst_ctx_t ctx, kryst_lu_t* out);                          /* LuSolver::new direct_lu.rs:24 */
int32_t kryst_lu_destroy(kryst_lu_t lu);
/* LuSolver::solve (direct_lu.rs:64-90): factor, cache the factors, solve */
int32_t kryst_lu_solve(kryst_lu_t lu, kryst_dense_t a, kryst_pc_t pc, const double* b, double* x, int64_t n, kryst_stats_t* stats);
int32_t kryst_lu_solve_dev(kryst_lu_t lu, kryst_dense_t a, kryst_pc_t pc, kryst_vec_t b, kryst_vec_t x, kryst_stats_t* stats);
/* LuSolver::solve_cached (direct_lu.rs:34-43); KRYST_SOLVE_ERROR before any factorization or after a failed one (the reference panics) */
int32_t kryst_lu_solve_cached(kryst_lu_t lu, kryst_vec_t b, kryst_vec_t x);
/* the cached factorization: row_perm[i] / col_perm[j] = the row / column of A at position i / j, factors column-major in that frame
 * (L below the diagonal, its unit diagonal implied, U on and above); any pointer may be NULL */
int32_t kryst_lu_export(kryst_lu_t lu, int64_t n, int64_t* row_perm, int64_t* col_perm, double* factors_colmajor);
/* info[0] KRYST_DENSE_MAX, info[1] rows of the trailing block that one workgroup finishes inside LDS (KRYST_DENSE_TAIL = 0 .. 128 sets it,
 * 0: every step is a launch of its own; a test hook), info[2] rows of an update tile, info[3] rows of the cached factorization (-1: none);
 * count >= 4 */
int32_t kryst_lu_info(kryst_lu_t lu, int64_t* info, int32_t count);
/* QrSolver::solve (direct_lu.rs:117-146), square systems */
int32_t kryst_qr_solve(kryst_dense_t a, kryst_pc_t pc, const double* b, double* x, int64_t n, kryst_stats_t* stats);
int32_t kryst_qr_solve_dev(kryst_dense_t a, kryst_pc_t pc, kryst_vec_t b, kryst_vec_t x, kryst_stats_t* stats);

/* ---- host-only helpers (no GPU needed) ---- */
/* 7-point stencil rows of planes [k_lo,k_hi) with global columns; returns nnz; pass NULL arrays to size */
int64_t kryst_host_stencil7(int32_t N, int32_t kind, int32_t k_lo, int32_t k_hi,
                            int64_t* row_ptr, int64_t* col_idx, double* vals);
/* contiguous row blocks, boundaries aligned to `align` rows (k-slabs: align = N*N) */
int32_t kryst_host_partition_rows(int64_t n, int32_t nranks, int64_t align, int64_t* row_offsets /*nranks+1*/);
/* halo plan of one rank: which global columns it must receive from each owner.
 * recv_counts[nranks]; recv_cols[sum] ascending per owner.  Returns total count (call with NULL to size). */
int64_t kryst_host_halo_recv_plan(int32_t rank, int32_t nranks, const int64_t* row_offsets,
                                  const int64_t* row_ptr, const int64_t* col_idx_global,
                                  int64_t* recv_counts, int64_t* recv_cols);

/* ---- host-side factorisations on plain host arrays: no device, no context (ABI 5).  Exactly the code kryst_pc_ilup / kryst_pc_ilut run between
 * the download of the operator's rows and the upload of the factors (kryst_amd/csrc/host_factor.cpp), for CPU-only callers, for parity tests
 * against the oracle without a GPU and for the sanitizer tier (make -C kryst_amd/csrc san SAN=thread | address,undefined).
 * Rows (row_ptr[n+1], col[nnz] as int32, val[nnz]) of an n x n block; columns >= n (halo slots of a row-partitioned operator) are dropped.
 * Results: L's strictly-lower kept entries with their multipliers, U's strictly-upper kept entries, the kept diagonal (1.0 where none is
 * kept), each row in stored = ascending-column order (Ilut: in the order ilut.rs leaves them). */
typedef struct kryst_host_factors_s* kryst_host_factors_t;
/* extension (beside chebyshev.rs:35-70), host only, no GPU: the extreme eigenvalues of the symmetric tridiagonal k x k matrix with diagonal
 * alpha[0..k) and off-diagonal beta[0..k-1) (k in 1..64) by bisection with Sturm counts, each run until the midpoint of the bracket is one
 * of its ends: *lo = the lower end of the smallest eigenvalue's bracket, *hi = the upper end of the largest one's (k = 1: alpha[0]; an
 * entry that is not finite: NaN for both). */
int32_t kryst_host_tridiag_extreme_eigs(const double* alpha, const double* beta, int32_t k, double* lo, double* hi);
/* Ilup::new(fill).setup (src/preconditioner/ilup.rs:77-134) as a row pipeline over `threads` host threads (<= 0: up to 16) in round-robin blocks
 * of `block` rows (<= 0: 2048); any thread count and block size gives the bits of the one-thread loop.  KRYST_SOLVE_ERROR on a zero u_jj
 * (ilup.rs:108-110), the column j of the LOWEST row that met one through kryst_hip_last_error_row(). */
int32_t kryst_host_ilup(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t fill, int32_t threads, int64_t block,
                        kryst_host_factors_t* out);
/* Ilut::new(fill, droptol).setup (src/preconditioner/ilut.rs:80-117): drop by magnitude, keep the `fill` largest of a row, split at the diagonal */
int32_t kryst_host_ilut(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t fill, double droptol, int32_t threads,
                        kryst_host_factors_t* out);
int32_t kryst_host_factors_sizes(kryst_host_factors_t f, int64_t* n, int64_t* nnz_l, int64_t* nnz_u);
/* any pointer may be NULL; l_ptr / u_ptr hold n + 1 entries, diag n */
int32_t kryst_host_factors_get(kryst_host_factors_t f, int64_t* l_ptr, int32_t* l_col, double* l_val, int64_t* u_ptr, int32_t* u_col, double* u_val,
                               double* diag);
int32_t kryst_host_factors_destroy(kryst_host_factors_t f);
/* The level scheduler of the general triangular solve (ilup.rs:138-167 walks rows one after the other; rows of one level are independent):
 * level[i] = 1 + the highest level among the rows that row i of a strictly-lower (forward != 0: rows ascending) or strictly-upper (rows
 * descending) factor depends on, 0 when it depends on none.  *nlevels (may be NULL): the number of levels. */
int32_t kryst_host_levels(int64_t n, const int64_t* ptr, const int32_t* col, int32_t forward, int32_t* level, int32_t* nlevels);
/* color_graph (src/utils/coloring.rs:7-64) on the stored pattern (ptr, col) of an n x n matrix, host only: adjacency symmetrised without the
 * diagonal, distance-2 neighbourhoods, rows in ascending order take the lowest colour their neighbourhood does not hold yet.
 * colors: n entries; *ncolors (may be NULL): the number of colours. */
int32_t kryst_host_color_graph(int64_t n, const int64_t* ptr, const int32_t* col, int32_t* colors, int32_t* ncolors);

/* AMG::new(a, max_levels, threshold) (src/preconditioner/amg.rs:73-118) as written, on host rows (strictly ascending columns, n x n): the
 * code kryst_pc_amg runs before the upload (kryst_amd/csrc/amg_setup.cpp).  level_budget: the most entries P_l, R*A and A_{l+1} of one level
 * may hold (<= 0: max(8 nnz(A), 65536)); KRYST_FACTOR_ERROR when a level would exceed it (the reference's coarse levels fill in).  Level l
 * holds A_l, D_l^-1 and, except on the last level, P_l, R_l = P0_l^T and the aggregate of every row (which 4: in col, nrows entries). */
typedef struct kryst_host_amg_s* kryst_host_amg_t;
int32_t kryst_host_amg(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t max_levels, double threshold,
                       int64_t level_budget, kryst_host_amg_t* out);
int32_t kryst_host_amg_levels(kryst_host_amg_t h, int32_t* nlevels);
/* which: 0 A_l, 1 P_l, 2 R_l, 3 D_l^-1 (val), 4 aggregates (col); any pointer may be NULL */
int32_t kryst_host_amg_get(kryst_host_amg_t h, int32_t level, int32_t which, int64_t* nrows, int64_t* ncols, int64_t* nnz, int64_t* row_ptr,
                           int32_t* col, double* val);
int32_t kryst_host_amg_destroy(kryst_host_amg_t h);

/* The dense direct solvers of kryst_lu_solve / kryst_qr_solve (direct_lu.rs:64-90, :117-146) on host arrays, in the same operation order
 * (kryst_amd/csrc/host_dense.cpp): the same bits as the device.  a column-major; no size cap; the same statuses;
 * factors / row_perm / col_perm as kryst_lu_export gives them; b and x may be the same array, x is untouched on an error. */
int32_t kryst_host_dense_lu(int64_t nrows, int64_t ncols, const double* a, int64_t* row_perm, int64_t* col_perm, double* factors);
int32_t kryst_host_dense_lu_solve(int64_t n, const int64_t* row_perm, const int64_t* col_perm, const double* factors, const double* b, double* x);
int32_t kryst_host_dense_qr_solve(int64_t nrows, int64_t ncols, const double* a, const double* b, double* x);

/* Matrix Market coordinate file -> CSR (0-based, rows sorted, symmetric / skew-symmetric storage expanded, duplicates summed;
 * real, integer and pattern fields).  Returns nnz, or -1 (kryst_hip_last_error() says why).  Call with NULL arrays to size,
 * then with row_ptr[nrows+1], col_idx[nnz], vals[nnz].  The reference has no file I/O. */
int64_t kryst_host_read_matrix_market(const char* path, int64_t* nrows, int64_t* ncols, int64_t* row_ptr,
                                      int64_t* col_idx, double* vals);
/* PETSc binary AIJ matrix (MatView with a binary viewer: big-endian header 1211216, rows, cols, nnz, row lengths, columns,
 * values) -> CSR, same calling convention. */
int64_t kryst_host_read_petsc_binary(const char* path, int64_t* nrows, int64_t* ncols, int64_t* row_ptr,
                                     int64_t* col_idx, double* vals);

/* ---- several right-hand sides at once (an extension: the reference solves one b per call, src/solver/mod.rs:43-49) ----
 * THE RULE: column j of a batched call is, bit for bit, what the single-vector call returns for column j -- y, x, iterations, every
 * residual-history entry, final_residual, converged and the status.  The matrix is read once for all columns.
 * fp64, one rank; k is 2, 4 or 8 (anything else: KRYST_ERR_ARG).
 *
 * kryst_mvec_t widens V = Vec<f64> (the `b` / `x` of src/solver/mod.rs:43-49) to n x k: element (i, j) lives at i * k + j on the device (a
 * row's k values are contiguous), allocated as (ceil(n / 512) * 512 + 512) * k doubles, zero at creation -- kryst_vec_t's padding, per column. */
typedef struct kryst_mvec_s* kryst_mvec_t;
int32_t kryst_mvec_create(kryst_ctx_t ctx, int64_t n, int32_t k, kryst_mvec_t* out);
int32_t kryst_mvec_destroy(kryst_mvec_t mv);
int32_t kryst_mvec_shape(kryst_mvec_t mv, int64_t* n, int32_t* k);                    /* either pointer may be NULL */
/* the host side is column-major: column j starts at host + j * ld, ld >= n (kryst_vec_upload / _download, wrappers.rs' Vec<f64>, per column);
 * the (de)interleave runs on the device */
int32_t kryst_mvec_upload(kryst_mvec_t mv, const double* host, int64_t ld);
int32_t kryst_mvec_download(kryst_mvec_t mv, double* host, int64_t ld);
/* column j <- v / v <- column j (kryst_vec_copy per column); lengths must agree, 0 <= j < k */
int32_t kryst_mvec_set_column(kryst_mvec_t mv, int32_t j, kryst_vec_t v);
int32_t kryst_mvec_get_column(kryst_mvec_t mv, int32_t j, kryst_vec_t v);
/* test hook, kryst_bench_vec_padding for a multivector: *dirty (may be NULL) counts the allocated elements of ROW index >= n whose 64 bits
 * are not +0.0, before any fill; fill != NULL then sets every one of them -- (ceil(n / 512) * 512 + 512 - n) * k elements -- to *fill */
int32_t kryst_bench_mvec_padding(kryst_mvec_t mv, const double* fill, int64_t* dirty);
/* SparseMatrix::spmv (sparse.rs:56-67) on k columns: Y <- A X, Y overwritten; column j is kryst_spmv on column j, whatever storage form
 * kryst_spmv streams for the operator.  The kernel reads the operator's CSR-DIA value streams where kryst_spmm_kernel says so, else the plain
 * CSR arrays; the bits are the same.  REFUSED like kryst_spmv: X and Y the same multivector
 * (KRYST_ERR_ARG before any launch, Y unchanged); a row count or k that does not match: KRYST_ERR_ARG; distributed operators: KRYST_UNSUPPORTED. */
int32_t kryst_spmm(kryst_csr_t a, kryst_mvec_t x, kryst_mvec_t y);
/* which kernel kryst_spmm and the batched solvers take for this operator and k columns under the current KRYST_SPMM_FORM setting (auto | plain |
 * dia, read at every launch): *kernel = 0 the plain-CSR rows kernel, 1 the diagonal (CSR-DIA) kernel.  `dia` takes the diagonal kernel wherever
 * the operator holds the streams and falls back to the plain one silently elsewhere; `auto` (the default) takes it where kryst_spmv itself
 * streams CSR-DIA, for the widths at which it measured no slower.  k outside {2, 4, 8}: KRYST_ERR_ARG. */
int32_t kryst_spmm_kernel(kryst_csr_t a, int32_t k, int32_t* kernel);
/* CgSolver::solve (cg.rs:114-288) / PcgSolver::solve (pcg.rs:114-222) on every column of B with the initial guesses in X: one SpMM per
 * iteration, every column's scalars on the device in a state of its own; a column that has ended -- converged, the cap (converged = true
 * at max_iters like the reference), IndefiniteMatrix, IndefinitePreconditioner, max_iters <= 0 -- is frozen while the others go on.
 * stats[k], status[k] (the column's KError code, KRYST_OK = 0), hist_len[k] and hist (k slices of hist_cap entries, slice j at
 * hist + j * hist_cap) may each be NULL.  The call returns KRYST_OK whenever it ran, whatever the columns' codes; X(:, j) is written only
 * when status[j] == KRYST_OK.  B and X may be the same multivector (x0 = b).  kryst_cg_solve_multi* ignores pc (cg.rs:115); for
 * kryst_pcg_solve_multi* pc may be NULL, Identity or Jacobi, any other kind is KRYST_UNSUPPORTED, as are norm_type outside {0, 1},
 * has_radius, has_obj_target and distributed operators; nothing is written then.  There is no monitor and no stepping session. */
int32_t kryst_cg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params,
                                 kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap, int64_t* hist_len);
int32_t kryst_pcg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params,
                                  kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap, int64_t* hist_len);
/* the same with B and X on the host, column-major with leading dimension ld (column j at b + j * ld; x in/out) */
int32_t kryst_cg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, kryst_csr_t a, kryst_pc_t pc,
                             const kryst_params_t* params, kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap,
                             int64_t* hist_len);
int32_t kryst_pcg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, kryst_csr_t a, kryst_pc_t pc,
                              const kryst_params_t* params, kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap,
                              int64_t* hist_len);

/* ---- block CG: ONE Krylov space for the k columns (a labelled extension beside the batched solvers above, whose behaviour it does not change) ----
 * Dubrulle's retooled block CG (BCGrQ) with the thin QR done as a Cholesky-QR of a k x k Gram matrix; Jacobi enters through the symmetrically
 * preconditioned form.  Every column is minimised over the union of all k Krylov spaces, so k right-hand sides can take fewer iterations than
 * k solves; the columns are NOT independent any more (there is no per-column rule here: the reference is the restatement of the operation
 * order in kryst_amd/csrc/bcg_logic.h, which the tests pin bit for bit).  fp64, one rank, k in {2, 4, 8}.
 * Argument lists, NULL rules and the history layout are those of kryst_pcg_solve_multi*: pc may be NULL, Identity or Jacobi; other kinds,
 * norm_type outside {0, 1}, has_radius, has_obj_target and distributed operators are KRYST_UNSUPPORTED, k outside {2, 4, 8} or mismatched shapes
 * KRYST_ERR_ARG, and nothing is written then.  B and X may be the same multivector.
 * The history entry of column j is res_j = the 2-norm of column j of the k x k residual factor: in exact arithmetic ||r_j||_2 with no
 * preconditioner and ||r_j|| in the M^-1 norm, sqrt(r_j^T D^-1 r_j), with Jacobi (whatever norm_type says).  Per column converged =
 * res_j / res0_j <= tol || it >= max_iters; the solve stops when every column has res_j <= tol * res0_j or at max_iters; all columns report the
 * same `iterations`; final_residual is res_j; max_iters <= 0 ends after the initial residual as the batched solvers do.
 * Breakdowns end the whole block with ONE code for every column, iterations = the iteration it happened in (0: at the start), the history kept
 * up to there and X untouched (X is written only when the solve ends with KRYST_OK): KRYST_INDEFINITE_MATRIX (the Gram matrix of the directions
 * against their images is not positive definite, or holds a NaN), KRYST_INDEFINITE_PRECONDITIONER (a weighted residual Gram matrix with a negative
 * diagonal entry), KRYST_SOLVE_ERROR (rank loss: a pivot s of a k x k Cholesky factor with !(s > KRYST_BCG_RANK_TOL * G[j][j]),
 * KRYST_BCG_RANK_TOL = 2^-26 -- dependent or zero right-hand sides, n < k, a column that converged exactly).  There is no deflation: for
 * right-hand sides that may be dependent use kryst_cg_solve_multi* / kryst_pcg_solve_multi* (solve_many). */
#define KRYST_BCG_RANK_TOL 0x1p-26   /* 2^-26: the smallest s / G[j][j] a pivot of block CG's k x k Cholesky factors may have (kryst_amd/csrc/bcg_logic.h) */
int32_t kryst_bcg_solve_multi_dev(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params,
                                  kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap, int64_t* hist_len);
int32_t kryst_bcg_solve_multi(const double* b, double* x, int64_t n, int32_t k, int64_t ld, kryst_csr_t a, kryst_pc_t pc,
                              const kryst_params_t* params, kryst_stats_t* stats, int32_t* status, double* hist, int64_t hist_cap,
                              int64_t* hist_len);
/* One k x k scalar step of block CG on the HOST, no GPU involved: the code the device runs between two passes (bcg_logic.h), for tests.
 * Matrices are k x k, row major.  g: the Gram matrix (its upper triangle is read).  step 0 (start): c <- chol(g), out1 <- c^-1, res <- res0.
 * step 1: out1 <- Gamma = U^-1 U^-T with U = chol(g), out2 <- Gamma c.  step 2: out1 <- Phi = chol(g), out2 <- Phi^-1, c <- Phi c, res.
 * Returns KRYST_OK or the breakdown code of the pivot rule above; KRYST_ERR_ARG for a null pointer, another step or k outside {2, 4, 8}. */
int32_t kryst_host_bcg_step(int32_t step, int32_t k, const double* g, double* c, double* out1, double* out2, double* res);
/* test hook: out_kk (host, k x k row major, the lower triangle the mirror of the upper) <- the Gram matrix of U against V as block CG reduces
 * it: entry (a, b), a <= b, is the inner product of DESIGN.md section 4.2 over U(i, a) * V(i, b), or U(i, a) * (d_i * V(i, b)) with weights
 * inv_diag (may be NULL).  U and V may be the same multivector. */
int32_t kryst_bench_mvec_gram(kryst_mvec_t u, kryst_mvec_t v, kryst_vec_t inv_diag, double* out_kk);

/* ---- mixed precision: fp32 as a STORAGE format, and fp64 iterative refinement on top of it ----
 * A LABELLED DEVIATION from the reference at T = f32 (CsrMatrix<f32>, CgSolver<f32>, `T: Float`), which would round every operation: here
 * fp32 is how vector elements and matrix values are STORED.  Every kernel widens what it loads, computes in fp64 in the fixed order of its
 * fp64 twin (separate multiply and add) and rounds once -- (float), round to nearest even, fp32 subnormals kept -- when it stores; every
 * scalar (alpha, beta, the inner products, the residual norms, the exits) is fp64 and is the fp64 solver's own code.  One rank; the plain CSR
 * arrays, or (kryst_csr32_lower_form) the CSR-P16 row-pattern form or the CSR-DIA diagonal form; nothing here runs unless it is called. */
typedef struct kryst_vec32_s* kryst_vec32_t;
typedef struct kryst_csr32_s* kryst_csr32_t;
/* kryst_reduce_spec for fp32-stored vectors: T = 256 threads own V = 4 consecutive elements each (a 1024-element tile, one 16-byte access
 * per lane); a term is (double)a * (double)b, exact; the thread folds its 4 terms in index order from 0.0, then the tree of
 * kryst_reduce_spec with the library's F. */
void    kryst_reduce_spec32(int32_t* T, int32_t* V, int32_t* F);
/* V = Vec<f32> of core/wrappers.rs on the device: ceil(n / 1024) * 1024 + 1024 floats, zero at creation (kryst_vec_create's rule at the fp32
 * tile size); upload / download move n floats (kryst_vec_upload / _download) */
int32_t kryst_vec32_create(kryst_ctx_t ctx, int64_t n, kryst_vec32_t* out);
int32_t kryst_vec32_destroy(kryst_vec32_t v);
int32_t kryst_vec32_upload(kryst_vec32_t v, const float* host, int64_t n);
int32_t kryst_vec32_download(kryst_vec32_t v, float* host, int64_t n);
/* test hook, kryst_bench_vec_padding for an fp32 vector: *dirty (may be NULL) counts the allocated floats of index >= n whose 32 bits are
 * not +0.0, then *fill (may be NULL) sets them all; elements below n are never touched */
int32_t kryst_bench_vec32_padding(kryst_vec32_t v, const float* fill, int64_t* dirty);
/* dst[i] = (float)src[i] (rounds) / dst[i] = (double)src[i] (widens, exact), on the device; lengths must agree */
int32_t kryst_vec32_from_f64(kryst_vec32_t dst, kryst_vec_t src);
int32_t kryst_vec32_to_f64(kryst_vec_t dst, kryst_vec32_t src);
/* InnerProduct::dot (wrappers.rs:90-108) on fp32-stored vectors: fp64 terms and sums in the tree of kryst_reduce_spec32 */
int32_t kryst_dot32(kryst_vec32_t x, kryst_vec32_t y, double* out);
/* CsrMatrix<f32> from a CsrMatrix<f64> (sparse.rs:22-46): device-to-device COPIES of the operator's row pointers and columns and its values
 * rounded to fp32 on the device (nnz + 8 entries, zeroed tail) -- no lifetime tie to `a`.  REFUSED with KRYST_UNSUPPORTED, nothing
 * created: a finite value that would round to +-inf; a distributed operator.  A non-square operator is accepted (kryst_spmv32 handles it,
 * the solvers refuse it). */
int32_t kryst_csr32_lower(kryst_csr_t a, kryst_csr32_t* out);
/* The lowering with a choice of what the lowered operator keeps.  Every form keeps the plain arrays exactly as kryst_csr32_lower (= PLAIN) makes
 * them -- the counts of kryst_csr32_info, the overflow refusal and the fallback kernel are the same.  PATTERN, and AUTO when `a` has a CSR-P16
 * (row-pattern) form, ALSO keeps its own copies of that form: one 16-bit pattern id per row (re-padded to the 1024-row fp32 tile), the pattern
 * table's offsets, and its values rounded with the same (float) as the CSR values, so a table value is bit for bit the lowered value of every row
 * that uses it and kryst_spmv32 gives the same bits on either form.  KRYST_UNSUPPORTED, *out untouched: PATTERN on an operator without a CSR-P16
 * form, or whose vectors do not fit 32-bit byte offsets (AUTO keeps the plain arrays alone in both cases); a distributed operator.  An unknown
 * form: KRYST_ERR_ARG.
 * DIA (opt-in: AUTO never chooses it) ALSO keeps its own fp32 copy of the operator's CSR-DIA value streams: one stream of
 * ceil(nrows / 1024) * 1024 + 1024 floats per diagonal, in the diagonals' stored order, the offsets copied.  A stream entry is (float) of the
 * fp64 stream entry -- bit for bit the lowered CSR value at that position, so kryst_spmv32 gives the same bits as on the plain arrays -- and an
 * absent entry (and all padding) carries the bits KRYST_CSR32_DIA_ABSENT_BITS: a quiet NaN whose payload (float) of the canonical NaN never
 * has.  KRYST_UNSUPPORTED, *out untouched: `a` keeps no CSR-DIA streams; a stored NaN whose rounding has the marker's bits (the fp64 form
 * refuses a stored value with its own marker's bits the same way); vectors that do not fit 32-bit byte offsets; a distributed operator.
 * An operator is given CSR-DIA streams at creation only: at most 32 distinct (col - row) offsets, every row in one common diagonal order,
 * D * nrows <= 1.125 * nnz + 64, and -- by default (KRYST_SPMV_DIA=1) -- no CSR-D16 / CSR-P16 form, which stream fewer bytes in fp64;
 * KRYST_SPMV_DIA=2 at creation builds the streams whenever the other rules hold, KRYST_SPMV_DIA=0 never. */
#define KRYST_CSR32_PLAIN 0
#define KRYST_CSR32_AUTO 1
#define KRYST_CSR32_PATTERN 2
#define KRYST_CSR32_DIA 3
#define KRYST_CSR32_DIA_ABSENT_BITS 0x7FD1A0D1u
int32_t kryst_csr32_lower_form(kryst_csr_t a, int32_t form, kryst_csr32_t* out);
/* *kernel: the kernel the next kryst_spmv32 (and every SpMV of the fp32 solvers) takes under the current settings -- 0 the plain wave kernel,
 * 1 the row-pattern kernel, 2 the row-pattern kernel with the near operands staged in LDS (boxes of lines of n points, n % 4 == 0, uniform far
 * offsets), 3 the diagonal-stream kernel of an operator lowered with DIA.  Settings, read at every launch (once per solve inside one):
 * KRYST_SPMV32_FORM = plain | pattern | dia (default: the most compact form held; `plain` sends every operator to the plain wave kernel, the
 * other two words mean the default for an operator that holds the form), KRYST_SPMV32_STAGE = 0 | 1 (default 1). */
int32_t kryst_csr32_encoding(kryst_csr32_t a, int32_t* kernel);
/* info[0]: values the rounding changed; info[1]: nonzero values that became zero or fp32-subnormal; info[2]: rows */
int32_t kryst_csr32_info(kryst_csr32_t a, int64_t info[3]);
int32_t kryst_csr32_destroy(kryst_csr32_t a);
/* host twin of the lowering's rounding, no GPU: out[i] = (float)v[i], info[0] / info[1] as kryst_csr32_info (info may be NULL);
 * KRYST_UNSUPPORTED when a finite value rounds to +-inf (the verdict of kryst_csr32_lower) */
int32_t kryst_host_round_f32(const double* v, int64_t n, float* out, int64_t info[2]);
/* SparseMatrix::spmv (sparse.rs:56-67, the row loop of :107-113 on widened operands): y[i] = (float) of the fold from 0.0, in stored
 * (ascending column) order, of (double)val * (double)x[col].  x and y the same vector: KRYST_ERR_ARG before any launch. */
int32_t kryst_spmv32(kryst_csr32_t a, kryst_vec32_t x, kryst_vec32_t y);
/* CgSolver::solve (cg.rs:114-288) / PcgSolver::solve (pcg.rs:114-222) on fp32-stored vectors and operator, with the scalar steps and exits
 * of kryst_cg_solve_dev / kryst_pcg_solve_dev: x = (float)(x + alpha p), r = (float)(r - alpha Ap), p = (float)(z + beta p),
 * z = (float)(dinv r); three launches per iteration.  x is written once, at the end, and only on KRYST_OK; b and x may be the same vector.
 * kryst_cg32_solve_dev ignores pc (cg.rs:115); kryst_pcg32_solve_dev takes NULL, Identity or Jacobi (jacobi.rs:84-86, its inverse
 * diagonal rounded to fp32 once per solve).  KRYST_UNSUPPORTED, nothing written: any other preconditioner kind, norm_type outside {0, 1},
 * has_radius, has_obj_target, a non-square operator.  No monitor, no stepping session; one solve per context at a time (KRYST_ERR_BUSY). */
int32_t kryst_cg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params,
                             kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len);
int32_t kryst_pcg32_solve_dev(kryst_vec32_t b, kryst_vec32_t x, kryst_csr32_t a, kryst_pc_t pc, const kryst_params_t* params,
                              kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len);
/* fp64 iterative refinement around the fp32 solvers (an extension: the reference has no counterpart; it stands beside LinearSolver::solve,
 * src/solver/mod.rs:43-49).  Outer work in fp64 with kryst_spmv's own kernel for `a`: r = b - A x, rho0 = ||r|| (pushed to hist); for
 * k = 1 .. outer->max_iters: solve a32 c = (float)(r / rho) from c = 0 with kryst_cg32 (pc NULL / Identity) or kryst_pcg32 (Jacobi) under
 * `inner` (its iteration count goes to inner_iters[k - 1] while k - 1 < inner_cap); an inner error status is returned as it is, x untouched,
 * iterations = k - 1; x' = x + rho * (double)c, rho' = ||b - A x'|| (pushed); !(rho' < rho): the step is REJECTED -- x stays the last
 * accepted iterate, iterations = k, converged = 0, final_residual = rho, KRYST_OK; else accepted and Convergence::check(rho, rho0, k)
 * (convergence.rs:18-34: reaching the cap reports converged).  outer->max_iters <= 0 or rho0 == 0: KRYST_OK, converged = 1, x untouched.
 * a32 must be the lowering of an operator of a's shape (KRYST_ERR_ARG); refusals as the fp32 solvers'.  stats, hist, hist_len, inner_iters
 * may be NULL.  The host reads one scalar per outer step. */
int32_t kryst_refine_solve_dev(kryst_vec_t b, kryst_vec_t x, kryst_csr_t a, kryst_csr32_t a32, kryst_pc_t pc, const kryst_params_t* outer,
                               const kryst_params_t* inner, kryst_stats_t* stats, double* hist, int64_t hist_cap, int64_t* hist_len,
                               int64_t* inner_iters, int64_t inner_cap);

#ifdef __cplusplus
}
#endif
#endif
