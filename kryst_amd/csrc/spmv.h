// What the units of the CSR SpMV share (spmv.hip holds the map of the units): the kernels' argument block and its fills, the choice of the
// kernel a tile launch takes, and the enqueue functions of the units that hold the kernels.  Internal: csr.h has what other subsystems call.
#pragma once
#include "csr.h"
#include "ew.h"
#include "spmv_window.h"
#include <algorithm>

namespace kr {

struct SpmvArgs {
    const int32_t* row_ptr; const int32_t* col; const double* val;
    const double* x; const double* halo; int32_t nloc;
    double* y; const int32_t* tiles; int32_t ntiles; int32_t nrows;
    const double* dvec; double* partials; int64_t pstride;
    const int* done; int32_t xcd_chunk; int32_t swizzle; int32_t group;
    const uint8_t* code; const int32_t* dict;      // CSR-D8: col = row + dict[code] (nullptr when not compressed)
    const uint16_t* code16; const double* vdict;   // CSR-D16: col = row + dict[c & 255], val = vdict[c >> 8]
    const uint16_t* pid; const uint32_t* pmeta; const int32_t* poff; const double* pval; int32_t npat, ntab;   // CSR-P16
    const uint8_t* pid_same;                       // marching kernels: per tile, 1 = its ids are those of the tile one plane below (nullptr: never the same)
    int32_t pat_red_off;                           // byte offset of the reduction scratch in the kernel's dynamic LDS
    int32_t nloc8;                                 // 8 * nloc
    int32_t tpw;                                   // pattern kernel: consecutive tile slots per workgroup
    int32_t amask;                                 // window start = k0 & ~amask (1: value pairs; 31: whole memory lines)
    const double* dia; int64_t dia_stride; int32_t dia_nd; int32_t dia_min;    // CSR-DIA: value streams, diagonals, lowest offset
    int64_t xsafe; int32_t cmax;                   // last safe start of a 16-byte pair in x's allocation; last valid local column
    int32_t dia_off[KR_DIA_MAX];
#ifdef KR_TUNING
    int32_t abl;                                   // timing-only ablation mask (tuning builds)
#endif
};

template <bool HALO>
__device__ __forceinline__ double gather(const SpmvArgs& a, int32_t c) {
    if constexpr (HALO) {
        const double* base = (c < a.nloc) ? a.x : (a.halo - a.nloc);
        return base[c];
    } else {
        return a.x[c];
    }
}

// ---- what crosses the unit boundaries (the library exports none of it)
#pragma GCC visibility push(hidden)
// The choice (spmv.hip): which kernel a tile launch takes, from the forms the operator has and the KRYST_SPMV_* settings, read at every launch.
enum class TileKernel { Wave, Rows, Dict, Dia, Pattern, PatternStage };
// the tiles a launch covers: the whole operator in natural order, a rank's contiguous interior tiles, or a list (boundary tiles, the slab order)
enum class TileRange { Whole, Interior, List };
TileKernel tile_kernel(kryst_csr_t a, bool halo, TileRange range);      // halo: the CSR-P16 size limit counts the halo buffer
// CSR-D8's byte codes are streamed: a launch takes them at every KRYST_SPMV_COMPRESS level but 0, kryst_csr_encoding reports them from level 1
inline bool d8_codes(kryst_csr_t a, int level, bool as_reported) { return a->d_code && (as_reported ? level >= 1 : level != 0); }
bool streams_p16(kryst_csr_t a, bool halo);        // the CSR-P16 form is the one streamed (KRYST_SPMV_COMPRESS >= 3, 32-bit byte offsets)
bool staged_form(kryst_csr_t a);                   // structure: a CSR-P16 form whose near operands can be staged in LDS
bool staged_form_uniform_far(kryst_csr_t a);       // ... on one rank, square, the same far offsets in every base: what the fused kernels need
bool staged_settings_ok(kryst_csr_t a);            // KRYST_SPMV_STAGE and the 32-bit element indices of the staged kernels
int stage_group_default(kryst_csr_t a, int64_t nruns, int T, bool fused);      // spmv_pattern.hip
// last safe start of a 16-byte pair in a vector of the operator's xlen: vectors are allocated padded to a tile multiple + one tile (blas1.hip)
inline int64_t xsafe_of(kryst_csr_t a) { return (a->xlen + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE - 2; }
// the fields every launch sets and the CSR-P16 tables; everything else zero
inline void spmv_args_fill(SpmvArgs& g, kryst_csr_t a, const double* x, double* y, const double* dvec, const int* done) {
    memset(&g, 0, sizeof g);
    g.x = x; g.y = y; g.dvec = dvec; g.done = done; g.partials = a->ctx->d_partials; g.pstride = a->ctx->partials_cap;
    g.ntiles = (int32_t)a->ntiles; g.nrows = (int32_t)a->nrows; g.nloc = (int32_t)a->nrows;
    g.pid = a->d_pid; g.pmeta = a->d_pmeta; g.poff = a->d_poff; g.pval = a->d_pval; g.npat = a->npat; g.ntab = a->ntab;
}
// dynamic LDS of the staged-window kernels: `windows` windows of 512 T + 2 n + pad doubles (pad 4: a pair beyond the lines below and above, the
// un-marched kernels; 0: the marching kernels, march_window.h), 8 bytes per pattern, entry_bytes per table entry (12: values and offsets, 8: values),
// then -- 16-byte aligned, at red_off -- red_copies x T x nq partials per wave
struct StagedLds { size_t red_off, bytes; };
inline StagedLds staged_lds(kryst_csr_t a, int windows, int entry_bytes, int red_copies, int T, int nq, int pad = 4) {
    const size_t tab = (size_t)windows * sizeof(double) * (size_t)((int64_t)T * KR_TILE + 2 * a->pat_stage_n + pad) + (size_t)a->npat * 8 + (size_t)a->ntab * (size_t)entry_bytes;
    const size_t red_off = (tab + 15) & ~(size_t)15;
    return StagedLds{red_off, red_off + sizeof(double) * (size_t)red_copies * (size_t)T * (size_t)nq * (KR_T / 64)};
}
// compile-time dispatch of a launch (common.h: by_int / by_bool)
template <class F> inline int32_t by_nq(int nq, F&& f) {          // the fused inner products of a tile launch: nq = 0, 1, 2
    if (!by_int<0, 1, 2>(nq, f)) { set_error("spmv: nq=%d", nq); return KRYST_ERR_ARG; }
    KR_HIP(hipGetLastError()); return KRYST_OK;
}
// enqueue functions, on ctx->s_main: `g` arrives with the common fields, the tiles and their slotting filled (spmv.hip: launch_tiles) and an enqueue
// function adds what its kernels alone read
int32_t enqueue_stream(TileKernel kernel, kryst_csr_t a, SpmvArgs g, bool halo, int nq, const PlainWavePlan& p, bool comp);      // spmv_stream.hip (comp: CSR-D8's codes)
int32_t enqueue_pattern(kryst_csr_t a, SpmvArgs g, bool halo, int nq, bool ordered);                                  // spmv_pattern.hip
int32_t enqueue_pattern_stage(kryst_csr_t a, SpmvArgs g, int nq, bool interior);
int32_t halo_finish(kryst_csr_t a, int budget);    // halo.hip: the receiving half of an exchange halo_begin started
#pragma GCC visibility pop

}  // namespace kr
