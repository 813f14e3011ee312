// CSR SpMV for gfx950 -- replaces CsrMatrix::spmv / spmv_parallel (src/matrix/sparse.rs:56-67,103-114).
//
// HBM-bound (0.134 flop/B; MFMA is useless here), so the kernels differ in how many bytes describe the matrix -- the operator is stored in up to
// five lossless forms built at creation (csr_create.hip) and the most compact one is streamed.  The units, by job (no relocatable device code: a
// kernel template is in the unit of every launch and hipFuncSetAttribute that names it):
//   spmv.h            SpmvArgs and its fills, device helpers, the choice's types, what crosses the unit boundaries
//   spmv.hip          the choice (tile_kernel, the staged form's predicates), launch_tiles, launch_spmv, plain_wave_plan, the entry points and query hooks
//   spmv_pattern.hip  spmv_pattern_kernel        CSR-P16  one 16-bit row-pattern id per ROW        (constant-coefficient grid operators)
//                     spmv_pattern_stage_kernel  CSR-P16  ... the near operands of a run of tiles staged in LDS (boxes of lines of n points)
//   spmv_stream.hip   spmv_dict_kernel           CSR-D16  one 16-bit (value, offset) code per entry
//                     spmv_dia_kernel            CSR-DIA  one value stream per diagonal            (stencils, variable coefficients included)
//                     spmv_rows_kernel           CSR-D8   raw values + 1-byte column-offset codes  (any structured grid)
//                     spmv_wave_kernel           plain    8 B value + 4 B column per entry         (everything else)
//   spmv_fuse.hip     spmv_pattern_fuse_kernel (CG's direction pass inside the staged SpMV; fuse_march: a workgroup walks the planes),
//                     cg_recompute_residual_kernel (the residual pass forms A p again), their plans, launches and hooks
//   halo.hip          the halo exchange: pack / push / pull kernels, halo_begin, halo_finish, halo_peer_*, halo_send_tiles, kryst_csr_halo_mode
// Shared contract:
//  * a workgroup owns ROW TILES of KR_TILE = 512 consecutive rows (thread t: rows 2t, 2t+1); every lane sums its rows in
//    ASCENDING column order starting from 0.0 with separate mul and add -- bit-identical to the reference's per-row loop
//    (sparse.rs:107-113) in every form.
//  * the window kernels (wave / rows / dict): each of the 4 waves streams the contiguous nnz range of ITS 128 rows through a
//    private LDS window with coalesced loads, every load of the window in flight before the first use; rows longer than a
//    window continue their running sum in the next one.  Same-wave LDS traffic is ordered by the hardware: NO workgroup barrier.
//  * y is written 16 B per lane; optional fused inner products (d.y, y.y) reuse the tile's rows and produce one partial per
//    tile in the library-wide association order (see ew.h), so CG's (p,Ap) costs no extra pass.
//  * tile -> workgroup map: consecutive tiles (pattern kernel: runs of 8 tiles) round-robin over the 8 XCDs.
//  * distributed: interior tiles run while the halo planes travel over xGMI on a second stream; boundary tiles follow.
//    Column indices >= nloc address the halo buffer.
#include "spmv.h"

namespace kr {

// ---- the choice.  Which kernel a launch takes is decided HERE, from the forms the operator has and the KRYST_SPMV_* settings (read per launch);
// launch_tiles, uses_tile_order and the query hooks below all ask tile_kernel, the fused launches (spmv_fuse.hip) the predicates.
bool streams_p16(kryst_csr_t a, bool halo) {
    return a->d_pid && env_int("KRYST_SPMV_COMPRESS", 3) >= 3 && a->xlen + (halo ? a->plan.total_recv : 0) < (1ll << 28) && a->nrows < (1ll << 28);
}
// every base is (far, -n, -1, 0, +1, +n, far) with one even n <= 1024 (csr.h: pat_stage_n) and the tables fit beside the window
bool staged_form(kryst_csr_t a) { return a->d_pid && a->pat_stage_n > 0 && a->npat <= 512 && a->ntab <= 512; }
bool staged_form_uniform_far(kryst_csr_t a) { return staged_form(a) && !a->dist && a->pat_far_uniform && a->nrows == a->xlen; }
bool staged_settings_ok(kryst_csr_t a) { return env_int("KRYST_SPMV_STAGE", 1) != 0 && a->xlen + 2 * KR_TILE < (1ll << 31); }
// The form cascade: CSR-P16, then CSR-D16, CSR-DIA, CSR-D8, plain.  KRYST_SPMV_COMPRESS: 0 plain CSR, 1 CSR-D8 (offset codes) and CSR-DIA, 2 CSR-D16
// (offset + value codes), 3 CSR-P16 (row patterns); each level falls back to the next lower one the operator qualifies for.  KRYST_SPMV_KERNEL: 2 the
// products-in-LDS wave kernel for plain CSR, 3 the rows kernel.  The staged-window kernel walks runs of consecutive tiles in natural order without
// halo columns, so a list never takes it.
TileKernel tile_kernel(kryst_csr_t a, bool halo, TileRange range) {
    const int level = env_int("KRYST_SPMV_COMPRESS", 3);
    if (streams_p16(a, halo)) return !halo && range != TileRange::List && staged_form(a) && staged_settings_ok(a) ? TileKernel::PatternStage : TileKernel::Pattern;
    if (a->d_code16 && level >= 2) return TileKernel::Dict;
    if (a->d_dia && level >= 1 && env_int("KRYST_SPMV_DIA", 1) != 0) return TileKernel::Dia;
    return d8_codes(a, level, false) || env_int("KRYST_SPMV_KERNEL", 2) == 3 ? TileKernel::Rows : TileKernel::Wave;
}
// slab order (csr_create.hip: build_tile_order) for a whole local operator.  KRYST_SPMV_ORDER: 1 (default) where it was measured
// to pay -- the CSR-DIA kernel, and the plain kernel once two planes of x outgrow an XCD's L2 (in-process A/B, tools/spmv_ab.py,
// profiles/r03/slab_order/: plain 512^3 +1.3-2.2 %, 448^3 -1.4 %, 384^3 -1.1 %, 256^3 -2.2 %; CSR-DIA 512^3 / 256^3 +0.4 / +1.9 %;
// CSR-D8 -2.4 / -3.6 %, CSR-D16 -0.7 / -2.9 %, CSR-P16 -4.8 / -4.6 % -- although the x re-reads go away in every form: 17.3 -> 14.3 GB
// per launch through the fabric for plain CSR at 512^3, 11.8 -> 9.7 GB for CSR-DIA); 2 every kernel; 0 never
static bool uses_tile_order(kryst_csr_t a) {
    if (!a->d_tile_order || a->dist) return false;
    const int order_mode = env_int("KRYST_SPMV_ORDER", 1);
    if (order_mode <= 0) return false;
    if (order_mode >= 2) return true;
    const TileKernel k = tile_kernel(a, false, TileRange::List);           // the kernel that would walk the order's list
    return k == TileKernel::Dia || (k == TileKernel::Wave && a->order_plane >= 262144);
}
// tiles, XCD slotting, grid, window alignment, pair slots and load kind of a launch of the stream kernels (the wave kernel reads all of them, the
// others the slotting and the grid); ordered: `tiles` is the slab order
static PlainWavePlan stream_plan(kryst_csr_t a, const int32_t* tiles, int64_t ntiles, bool ordered) {
    PlainWavePlan p;
    p.tiles = tiles; p.ntiles = (int32_t)ntiles;
    // the plain kernel beyond the Infinity Cache: nontemporal matrix streams in windows that start on whole memory lines (in-process
    // A/B, tools/spmv_ab.py, profiles/r03/slab_order/: 384^3 +0.8 %, 448^3 +1.6-2.0 %, 512^3 +1.1-2.1 %; nontemporal loads alone lose 1 %)
    const bool beyond_cache = a->nrows * 8 > (256ll << 20);
    p.amask = env_int("KRYST_SPMV_ALIGN", beyond_cache ? 1 : 0) ? 31 : 1;
    p.nt = env_int("KRYST_SPMV_NT", beyond_cache ? 1 : 0) != 0;
    p.swizzle = ordered ? 0 : env_int("KRYST_SPMV_SWIZZLE", 0);
    p.group = ordered ? 1 : std::max(1, env_int("KRYST_SPMV_GROUP", 1));
    int64_t chunk = (ntiles + 7) / 8;                       // tiles per XCD
    if (!p.swizzle) chunk = (chunk + p.group - 1) / p.group * p.group;   // a whole number of runs of `group` tiles
    p.xcd_chunk = (int32_t)chunk;
    int64_t per = chunk;                                    // one tile per workgroup by default
    const int bpc = env_int("KRYST_SPMV_BLOCKS_PER_CU", 0);
    if (bpc > 0) per = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)a->ctx->num_cu * bpc / 8));
    p.grid = (unsigned)(per * 8);
    // window size of the plain kernel: one window per 128-row slice (7 pair slots for a 7-point stencil's 896 entries) while the
    // vectors fit the 256 MiB Infinity Cache, 4 slots (74 registers, 6 waves per SIMD instead of 4) beyond it -- measured
    // (profiles/r02/plain_csr_study/README.md): 256^3 0.298 / 0.309 ms with 7 / 4 slots, 512^3 2.84 / 2.62 ms
    p.slots = a->slots;
    if (p.slots > 4 && beyond_cache) p.slots = 4;
    const int slots_env = env_int("KRYST_SPMV_SLOTS", 0);
    if (slots_env > 0) p.slots = slots_env;
    return p;
}
// what launch_tiles hands spmv_wave_kernel for the whole single-rank operator under the current settings, for a kernel of another file that walks
// the plain arrays the same way (cheb_poly.hip)
PlainWavePlan plain_wave_plan(kryst_csr_t a) {
    const bool ordered = uses_tile_order(a);
    return stream_plan(a, ordered ? a->d_tile_order : nullptr, ordered ? a->order_slots1 : a->ntiles, ordered);
}
// one launch over the tiles `tiles` (nullptr: all of them in natural order); halo: they have halo columns (>= nloc: the halo buffer)
static int32_t launch_tiles(kryst_csr_t a, bool halo, const double* x, double* y, int nq, const double* dvec, const int* done,
                            const int32_t* tiles, int64_t ntiles) {
    if (ntiles == 0) return KRYST_OK;
    const bool ordered = !tiles && !halo && ntiles == a->ntiles && uses_tile_order(a);
    const bool interior = tiles && tiles == a->d_tiles_interior && a->interior_first >= 0 && ntiles == a->n_interior;
    const TileKernel kernel = tile_kernel(a, halo, ordered ? TileRange::List : !tiles ? TileRange::Whole : interior ? TileRange::Interior : TileRange::List);
    if (ordered) {                                          // (the pattern kernel walks runs of 8 slots per XCD, the others runs of 1)
        tiles = kernel == TileKernel::Pattern ? a->d_tile_order + a->order_slots1 : a->d_tile_order;
        ntiles = kernel == TileKernel::Pattern ? a->order_slots8 : a->order_slots1;
    }
    const PlainWavePlan p = stream_plan(a, tiles, ntiles, ordered);
    SpmvArgs args;
    spmv_args_fill(args, a, x, y, dvec, done);
    args.row_ptr = a->d_row_ptr; args.col = a->d_col; args.val = a->d_val; args.halo = a->plan.d_halo;
    args.tiles = p.tiles; args.ntiles = p.ntiles; args.swizzle = p.swizzle; args.group = p.group; args.xcd_chunk = p.xcd_chunk; args.amask = p.amask;
#ifdef KR_TUNING
    args.abl = env_int("KRYST_SPMV_ABL", 0);
#endif
    const bool comp = d8_codes(a, env_int("KRYST_SPMV_COMPRESS", 3), false);
    args.code = comp ? a->d_code : nullptr; args.dict = comp ? a->d_dict : nullptr;
    args.code16 = a->d_code16; args.vdict = a->d_vdict;
    switch (kernel) {
        case TileKernel::PatternStage: return enqueue_pattern_stage(a, args, nq, interior);
        case TileKernel::Pattern: return enqueue_pattern(a, args, halo, nq, ordered);
        default: return enqueue_stream(kernel, a, args, halo, nq, p, comp);
    }
}

int32_t launch_spmv(kryst_csr_t a, const double* x, double* y, int nq, const double* dvec, const int* done) {
    kryst_ctx_t ctx = a->ctx;
    if (nq > 0) KR_TRY(ensure_partials(ctx, a->ntiles));
    if (!a->dist || !use_collectives(ctx)) {
        const int32_t rc = launch_tiles(a, false, x, y, nq, dvec, done, nullptr, a->ntiles);
        phase_mark(ctx, KR_PH_SPMV);
        return rc;
    }
    // halo exchange on s_comm (unless the solver has started it already), overlapped with the interior tiles
    if (a->halo_started_for != x) KR_TRY(halo_begin(a, x));
    a->halo_started_for = nullptr;
    KR_TRY(launch_tiles(a, false, x, y, nq, dvec, done, a->d_tiles_interior, a->n_interior));   // interior tiles have no halo columns
    phase_mark(ctx, KR_PH_SPMV);
    KR_TRY(halo_finish(a, 0));
    phase_mark(ctx, KR_PH_HALO_WAIT);
    KR_TRY(launch_tiles(a, true, x, y, nq, dvec, done, a->d_tiles_boundary, a->n_boundary));
    phase_mark(ctx, KR_PH_SPMV_BOUNDARY);
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_spmv(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y) {
    KR_ARG(a && x && y, "spmv");
    KR_ARG(x->ctx == a->ctx && y->ctx == a->ctx, "spmv: context mismatch");
    KR_ARG(x->n == a->xlen, "spmv: x.len() != ncols");      // sparse.rs:57 assert_eq!
    KR_ARG(y->n == a->nrows, "spmv: y.len() != nrows");     // sparse.rs:58 assert_eq!
    KR_ARG(x->d != y->d, "spmv: x and y alias");
    KR_HIP(hipSetDevice(a->ctx->device));
    KR_TRY(launch_spmv(a, x->d, y->d, 0, nullptr, nullptr));
    // outside a solver nobody else reads the pull's error word: a neighbour's stamp that never came (the halo is NaNs then) is this call's error
    if (a->dist && a->plan.peer.on && use_collectives(a->ctx) && fold_gave_up(a->ctx)) return KRYST_ERR_RCCL;
    return KRYST_OK;
}

// which encoding kryst_spmv streams for this operator under the current KRYST_SPMV_COMPRESS setting:
// 0 plain CSR (12 B/nnz), 1 CSR-D8 (9 B/nnz), 2 CSR-D16 (2 B/nnz), 3 CSR-P16 (2 B/row), 4 CSR-DIA (8 B per diagonal and row)
int32_t kryst_csr_encoding(kryst_csr_t a, int32_t* encoding, int32_t* patterns, int32_t* table_entries) {
    KR_ARG(a && encoding, "csr_encoding");
    const int lvl = env_int("KRYST_SPMV_COMPRESS", 3);
    // (asked with the halo included, whatever tiles a launch covers: the form is reported for the operator as a whole)
    const TileKernel k = tile_kernel(a, true, TileRange::List);
    const int e = k == TileKernel::Pattern || k == TileKernel::PatternStage ? 3 : k == TileKernel::Dict ? 2 : k == TileKernel::Dia ? 4 : d8_codes(a, lvl, true) ? 1 : 0;
    *encoding = e;
    if (patterns) *patterns = e == 4 ? a->dia_nd : (a->d_pid ? a->npat : 0);      // CSR-DIA: the number of diagonals
    if (table_entries) *table_entries = a->d_pid ? a->ntab : 0;
    return KRYST_OK;
}

// info[0]: rows per plane of the slab order (0: the operator has none), info[1] / info[2]: tile slots in the orders for runs of 1 / 8
// slots per XCD, info[3]: 1 when kryst_spmv would use the order under the current settings
int32_t kryst_csr_tile_order(kryst_csr_t a, int64_t* info) {
    KR_ARG(a && info, "csr_tile_order");
    info[0] = a->d_tile_order ? a->order_plane : 0; info[1] = a->order_slots1; info[2] = a->order_slots8;
    info[3] = uses_tile_order(a) ? 1 : 0;
    return KRYST_OK;
}
// info[0]: line length n of the staged-window form of the CSR-P16 kernel (0: the operator's bases are not (far, -n, -1, 0, +1, +n, far)),
// info[1]: 1 when every base has the same far offsets (one round trip per run), info[2]: first tile of a rank's contiguous interior
// range (-1: none), info[3]: 1 when kryst_spmv would take the staged-window kernel under the current settings
// (the whole operator in natural order, or a rank's interior tiles)
int32_t kryst_csr_pattern_info(kryst_csr_t a, int64_t* info) {
    KR_ARG(a && info, "csr_pattern_info");
    info[0] = a->d_pid ? a->pat_stage_n : 0; info[1] = a->pat_far_uniform ? 1 : 0; info[2] = a->interior_first;
    const TileRange range = !a->dist || !use_collectives(a->ctx) ? TileRange::Whole : a->interior_first >= 0 ? TileRange::Interior : TileRange::List;
    info[3] = tile_kernel(a, false, range) == TileKernel::PatternStage ? 1 : 0;
    return KRYST_OK;
}

int32_t kryst_bench_spmv(kryst_csr_t a, kryst_vec_t x, kryst_vec_t y, int32_t fused_dots, int32_t reps, double* avg_ms) {
    KR_ARG(a && x && y && avg_ms && reps >= 1 && fused_dots >= 0 && fused_dots <= 2, "bench_spmv");
    KR_ARG(x->n == a->xlen && y->n == a->nrows, "bench_spmv: size mismatch");
    KR_ARG(x->ctx == a->ctx && y->ctx == a->ctx, "bench_spmv: context mismatch");
    KR_ARG(fused_dots == 0 || a->nrows == a->xlen, "bench_spmv: fused dots need a square operator");
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    // rotate over three copies of x: inside a solver the input vector has just been rewritten and does not sit in the
    // 256 MiB Infinity Cache, which a loop over ONE 128 MiB vector would (256^3: 63 us cache-warm against 86 us in CG)
    const size_t bytes = sizeof(double) * (size_t)((x->n + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE);
    double* xs[3] = {x->d, nullptr, nullptr};
    for (int k = 1; k < 3; ++k) {
        if (hipMalloc(&xs[k], bytes) != hipSuccess) { (void)hipGetLastError(); xs[k] = x->d; continue; }
        KR_HIP(hipMemcpyAsync(xs[k], x->d, bytes, hipMemcpyDeviceToDevice, ctx->s_main));
    }
    int32_t rc = launch_spmv(a, xs[0], y->d, fused_dots, xs[0], nullptr);        // warm-up launch
    (void)hipEventRecord(ctx->tm0, ctx->s_main);
    for (int r = 0; r < reps && rc == KRYST_OK; ++r) rc = launch_spmv(a, xs[(r + 1) % 3], y->d, fused_dots, xs[(r + 1) % 3], nullptr);
    (void)hipEventRecord(ctx->tm1, ctx->s_main);
    (void)hipEventSynchronize(ctx->tm1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->tm0, ctx->tm1);
    *avg_ms = (double)ms / reps;
    (void)hipStreamSynchronize(ctx->s_main);
    if (use_collectives(ctx)) (void)hipStreamSynchronize(ctx->s_comm);
    for (int k = 1; k < 3; ++k) if (xs[k] != x->d) (void)hipFree(xs[k]);
    return rc;
}

int32_t kryst_spmv_host(kryst_csr_t a, const double* x, int64_t nx, double* y, int64_t ny) {
    KR_ARG(a && x && y, "spmv_host");
    kryst_vec_t vx = nullptr, vy = nullptr;
    KR_TRY(kryst_vec_create(a->ctx, nx, &vx));
    int32_t rc = kryst_vec_create(a->ctx, ny, &vy);
    if (rc == KRYST_OK) rc = kryst_vec_upload(vx, x, nx);
    if (rc == KRYST_OK) rc = kryst_spmv(a, vx, vy);
    if (rc == KRYST_OK) rc = kryst_vec_download(vy, y, ny);
    kryst_vec_destroy(vx); kryst_vec_destroy(vy);
    return rc;
}

}  // extern "C"
