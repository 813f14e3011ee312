// State of the ILU-family preconditioners and what its three units share (overview: ilu.hip): ilu.hip applies, ilu_setup_host.hip and
// ilu_setup_device.hip set up.
#pragma once
#include "pc.h"
#include "host_factor.h"
#include <chrono>
#include <thread>
#include <sched.h>
#include <sys/mman.h>
#include <cstdlib>
#include <new>
#include <pthread.h>
#include <memory>
#include <string>
#include <mutex>
#include <atomic>
#include "ew.h"
#include <algorithm>
#include <cmath>
#include <map>

namespace kr {

// (par_rows, the host block pool / hvec, the janitor thread, FlatRows and the host-side factorisations themselves: host_factor.h -- no device call
// in there, so that the same code builds for the CPU alone under the sanitizers)

// wavefront kernel by number of 8 x 8 line blocks in the (j, k) plane: the 16 x 16 kernel from 32^3 up (table at its use)
static int default_wave_form(unsigned nb8) { return nb8 >= 16 ? 2 : 1; }

#define KR_ILU_BOX_DEFAULT 2         // KRYST_ILU_BOX: 0 box-stencil factors take the level-ordered forms, 1 hyperplane launches, 2 pipelined wavefront (tri_box.h)

struct TriArgs {                    // device-resident argument block, rewritten before every apply (graph-friendly):
    const double* r; double* z; long long skip;   // one scalar load gives a level kernel everything it needs
    long long epoch;                              // number of this apply (tri_quad.h: the value of its "under way" flags)
};

#define ELLW 4
struct EllView { const int32_t* col; const double* val; const uint8_t* len; int64_t npos; };

struct TriFactor {                  // one triangular factor in level order
    int32_t* d_ptr = nullptr;       // npos+1: entry range of the row at level-position p
    int32_t* d_col = nullptr;       // column (original numbering)
    double*  d_val = nullptr;
    int32_t* d_row = nullptr;       // npos: original row id
    double*  d_diag = nullptr;      // npos: divisor (1.0 when the apply does not divide)
    // ELL copy (rows of <= ELLW kept entries, e.g. any 7-point factor): slot-major, so a lane's loads do not depend
    // on a row pointer -- one round trip less on a latency-bound kernel
    int32_t* d_ecol = nullptr; double* d_eval = nullptr; uint8_t* d_elen = nullptr; int64_t npos = 0; bool ell = false;
    bool syncfree = false;          // ELL factor solved by ONE sync-free launch (KRYST_ILU_SYNCFREE=0: one launch per level)
    // operand streams of tri_run_free_kernel, built at set-up: per chunk of 64 level-order positions of a narrow run, [operand 0..7][lane] -- a
    // descriptor (> 0: the ring tag of an operand of this run that lies within reach, < 0: 0x80000000 | position of an operand to be gathered
    // from the vector, 0: no such entry) and the coefficient; what a lane needs lies where a coalesced load puts it, and nothing is classified per apply
    int32_t* d_fdesc = nullptr; double* d_fval = nullptr; int32_t* d_fpos = nullptr; int32_t* d_vreal = nullptr;   // (+ the operand's position in the vector; per virtual row its row and first / last flags)
    std::vector<int32_t> run_cbase; // first chunk of every narrow run in the streams, in the order enqueue_factor meets them
    std::vector<int32_t> run_nvirt; // virtual rows of every narrow run (a row of more than eight entries is a chain of them)
    int32_t last_entry = -1;        // index of the factor's last stored entry (tri_run_free_kernel clamps its look-ahead to it)
    bool free_runs = false;         // runs of narrow levels take tri_run_free_kernel (its 128 KiB of LDS were granted at set-up): the vector starts as sentinels
    int held = 16;                  // entries of a row the CSR sync-free kernel holds in registers (8: no row is longer than that)
    std::vector<int32_t> lvl_off;   // host: position offsets per level
    int32_t* d_lvl_off = nullptr;
    void free_all() { (void)pool_free(d_ptr); (void)pool_free(d_col); (void)pool_free(d_val); (void)pool_free(d_row); (void)pool_free(d_diag); (void)pool_free(d_lvl_off);
                      (void)pool_free(d_fdesc); (void)pool_free(d_fval); (void)pool_free(d_fpos); (void)pool_free(d_vreal);
                      (void)pool_free(d_ecol); (void)pool_free(d_eval); (void)pool_free(d_elen); }
    EllView view() const { return EllView{d_ecol, d_eval, d_elen, npos}; }
};

// Structured-grid form of one factor (natural row order): every kept entry of row (i,j,k) of an Ni x Nj x Nk box couples it to
// its -1 / -Ni / -Ni*Nj neighbour (L) or +1 / +Ni / +Ni*Nj neighbour (U) -- any ILU-family factor of a 7-point (or 5-point)
// operator in natural ordering.  Such a factor is solved by the pipelined wavefront kernel tri_grid_kernel instead of the
// level machinery.
struct GridFactor {
    bool ok = false;
    int32_t Ni = 0, Nj = 0, Nk = 0;
    double* d_c1 = nullptr; double* d_c2 = nullptr; double* d_c3 = nullptr;   // coefficient of the i / j / k neighbour
                                                                            // (0.0 = no such entry: zero entries are never stored)
    double* d_diag = nullptr;                                               // divisor (backward factor only)
    // blocked copy for tri_quad_kernel (16 x 16 lines per workgroup): [block][chunk][array][step pair][line], built on the device
    void* d_blocked = nullptr; int32_t nbj = 0, nbk = 0, nch = 0;
    double* d_edge_e = nullptr; double* d_edge_n = nullptr;                // edge rows handed to the next workgroup: [block][steps + 8][16]
    uint8_t* d_skip = nullptr;                                              // [block][quadrant][chunk]: coefficients repeat chunk - 3's (tri_quad_dedup_kernel)
    int64_t nskip = 0;                                                      // how many of them do (KRYST_ILU_VERBOSE)
    void free_all() { (void)pool_free(d_c1); (void)pool_free(d_c2); (void)pool_free(d_c3); (void)pool_free(d_diag);
                      (void)pool_free(d_blocked); (void)pool_free(d_edge_e); (void)pool_free(d_edge_n); (void)pool_free(d_skip); }
};
struct GridView { int32_t Ni, Nj, Nk; const double* c1; const double* c2; const double* c3; const double* diag; };

// Box-stencil form of one factor (round 4): every kept entry of row (i, j, k) of an Ni x Nj x Nk box couples it to (i + di, j + dj, k + dk)
// with |di|, |dj|, |dk| <= 1 -- strictly lower (L) or strictly upper (U) in natural ordering: any ILU-family factor of a stencil inside the
// 3 x 3 x 3 cube (27-point, 19-point, 9-point 2-D, ...) that is not a 7-point factor (those take GridFactor).  Thirteen coefficient streams
// in natural row order, stream a = the a-th offset in ASCENDING COLUMN order (the order the reference subtracts in): L: (dk, dj, di) =
// (-1,-1,-1), (-1,-1,0), ... (0,0,-1), i.e. a = 9 (dk + 1) + 3 (dj + 1) + (di + 1); U: (0,0,1), (0,1,-1), ... (1,1,1), a = that code - 14.
// 0.0 = no such entry (zero entries are never stored).
struct BoxFactor {
    bool ok = false;
    int32_t Ni = 0, Nj = 0, Nk = 0;
    double* d_c = nullptr;          // 13 streams, box_stream_stride(n) doubles apart: d_c[a stride + row]
    double* d_diag = nullptr;       // divisor (backward factor only)
    void* d_cb = nullptr;           // blocked copy for tri_box_kernel: [block][chunk][stream (, divisor)][step pair][lane] (tri_box_layout_kernel)
    uint32_t present = 0x1fff;      // streams with at least one entry
    bool regular = false;           // every present stream has an entry wherever the neighbour row exists in the box (tri_box.h: REGULAR)
    void free_all() { (void)pool_free(d_c); (void)pool_free(d_diag); (void)pool_free(d_cb); d_c = nullptr; d_diag = nullptr; d_cb = nullptr; }
};
struct BoxView { int32_t Ni, Nj, Nk; int64_t n; const double* c; const double* diag; int64_t cs; const void* cb; };   // cs: doubles from one stream to the next; cb: blocked copy (tri_box.h)
// Streams are NOT n doubles apart: with n = 128^3 that is 16 MiB, and the 13 coefficients of a row would sit in the same HBM channel and bank
// (measured: 27-point 128^3 apply 1.75 ms where the hop / step model says 1.0).  n rounded up to 64 rows plus 72 rows: consecutive streams are
// 576 bytes apart modulo any power of two from 1 KiB up.
static inline int64_t box_stream_stride(int64_t n) { return (n + 63) / 64 * 64 + 72; }

// 8 x 8 blocks of grid lines in the (j, k) plane: the workgroups of tri_wave_kernel / tri_grid_kernel, and the flags per direction
static inline int wave_blocks(int32_t Nj, int32_t Nk) { return ((Nj + 7) / 8) * ((Nk + 7) / 8); }

// The three knobs that choose between the forms of an apply, each read here and nowhere else (laid_out_form / apply_form; the
// set-ups ask the first two whether a form is to be laid out at all).
//   KRYST_ILU_WAVE: 2 = 16 x 16 lines per workgroup (tri_quad.h), 1 = 8 x 8 lines (tri_wave.h), 0 = its one-wave predecessor.
//   Default by size (measured, MI355X, true ILU(0) apply, 16 x 16 vs 8 x 8): 24^3 0.088 / 0.083 ms, 32^3 0.091 / 0.098,
//   64^3 0.154 / 0.184, 96^3 0.217 / 0.286, 128^3 0.283 / 0.356, 256^3 0.65 / 1.00, 384^3 1.13 / 2.65, 512^3 1.91 / 5.7
static inline int ilu_wave_knob(const GridFactor& G) { return env_int("KRYST_ILU_WAVE", default_wave_form((unsigned)wave_blocks(G.Nj, G.Nk))); }
static inline int ilu_box_knob() { return env_int("KRYST_ILU_BOX", KR_ILU_BOX_DEFAULT); }
static inline bool ilu_planes_knob() { return env_int("KRYST_ILU_PLANES", 0) != 0; }    // per apply: one launch per hyperplane, whatever is laid out

struct IluPc final : kryst_pc_s {
    static constexpr int KIND = KR_PC_ILU;
    TriFactor L, U;
    GridFactor GL, GU;
    BoxFactor BL, BU;
    TriArgs* d_args = nullptr;
    double* d_rL = nullptr; double* d_y = nullptr; double* d_yU = nullptr; double* d_zU = nullptr;   // level-permuted work vectors
    int32_t* d_mapLU = nullptr;     // L-position of the row at U-position q
    int32_t* d_flags = nullptr;     // wavefront solve: "this block is under way", one per block and direction
    int32_t direct_epoch = 0;       // number of the last directly launched apply (1 .. 2^30 - 1; its flag value has bit 30 set)
    int32_t* h_gave_up = nullptr;   // mapped host word the wavefront kernel raises when a poller runs out of patience (never cleared on the device)
    int32_t* d_gave_up = nullptr;   // its device address
    bool box_wave_ready = false;    // box factor: flags, give-up word and the kernels' LDS size are set up for tri_box_kernel
    bool safe = false;              // the wavefront kernel gave up once: this preconditioner now uses the plane kernels (no inter-workgroup waits)
    bool switched = false;          // ... and the switch happened since the last pc_fell_back() query
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    explicit IluPc(kryst_csr_t a_) : kryst_pc_s(a_->ctx, KIND, a_, a_->nrows) {}
    ~IluPc() override;
    int32_t apply(int64_t nv, const double* r, double* z, const int* done) override;
    int32_t health() override;
    bool fell_back() override;
    bool check_after_apply() const override;               // the wavefront forms wait for neighbour workgroups (tri_wave.h) and may give up
    bool grid() const { return GL.ok && GU.ok; }
    bool box() const { return BL.ok && BU.ok; }
};

static const int NARROW = 2048;     // levels with at most this many rows are folded into one-workgroup runs (CSR fallback)
#define KR_TRI_SENTINEL 0xFFF8DEADBEEFCAFEull

// Every device initialisation of a preconditioner is issued on the context's compute stream and waited for.  That stream is
// non-blocking, so the null stream does not order with it, and hipMemset on the null stream returns before the fill has run:
// round 2 zeroed the argument block with it, and under a time-sliced GPU the fill could land AFTER the first apply's
// tri_set_args had written r and z there -- the level kernels then read through a null pointer.
// One per set-up unit (a static: an extern thread_local's weak init-function reference resolves to a non-null address in a shared object),
// each set by that unit's entry points -- finish_ilu_pc, general_setup_on_device -- before its calls of up().
static thread_local hipStream_t tl_setup_stream = nullptr;
static int32_t zero_dev(void* dst, size_t bytes, hipStream_t s) {
    KR_HIP(hipMemsetAsync(dst, 0, bytes, s));
    KR_HIP(hipStreamSynchronize(s));
    return KRYST_OK;
}
template <class T, class A>
static int32_t up(T** dst, const std::vector<T, A>& v) {
    KR_HIP(pool_malloc(dst, sizeof(T) * (v.size() + 1)));
    KR_HIP(hipMemsetAsync(*dst, 0, sizeof(T) * (v.size() + 1), tl_setup_stream));
    if (!v.empty()) KR_HIP(hipMemcpyAsync(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, tl_setup_stream));
    KR_HIP(hipStreamSynchronize(tl_setup_stream));
    return KRYST_OK;
}


// ---- what crosses the file boundaries (the library exports none of it)
#pragma GCC visibility push(hidden)
// ilu.hip, with the launches: a kernel's raised dynamic-LDS limit belongs to the translation unit that launches it
void choose_level_form(TriFactor* F, int64_t n, int64_t levels, int64_t longest_row, int64_t rows_longer_than_8, int64_t entries);
int32_t build_free_streams(TriFactor* F, hipStream_t st, const int32_t* hptr);
int32_t finish_ilu_device(IluPc* pc);
// ilu_setup_host.hip
bool box_dims_from_offsets(const std::vector<int64_t>& offs, int64_t n, int64_t* Ni_out, int64_t* Nj_out);
void box_classify(const unsigned long long cnt[13], bool forward, int64_t Ni, int64_t Nj, int64_t Nk, BoxFactor* B);
// ilu_setup_device.hip: -> KRYST_OK and *out set when the operator was handled on the device, *out left null when the host path is to take over
int32_t grid_setup_on_device(kryst_csr_t a, int mode, kryst_pc_t* out);
int32_t general_setup_on_device(kryst_csr_t a, int mode, kryst_pc_t* out);
int32_t ikj_on_device(kryst_csr_t a, const std::vector<int64_t>& rp, const std::vector<int32_t>& col, std::vector<double>& w, bool* used, int64_t* bad_row);
#pragma GCC visibility pop

}  // namespace kr
