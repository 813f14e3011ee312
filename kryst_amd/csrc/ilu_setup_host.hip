// Host-side set-up of the ILU family (overview: ilu.hip): factors that arrive as host rows -- ILU(0) when the device set-ups pass,
// Ilup(p >= 1), Ilut -- are recognised as structured-grid or box-stencil factors or level-ordered, and uploaded.
#include "ilu.h"

namespace kr {

// level order of one factor
static int32_t build_factor(int64_t n, const FlatRows& ent, const hvec<double>& diag, bool forward, TriFactor* F,
                            std::vector<int32_t>* pos_out) {
    std::vector<int32_t> lvl((size_t)n, 0);
    const int32_t nl = host_levels(n, ent.ptr.data(), ent.col.data(), forward, lvl.data());      // (host_factor.cpp)
    F->lvl_off.assign((size_t)nl + 1, 0);
    for (int64_t i = 0; i < n; ++i) F->lvl_off[lvl[i] + 1]++;
    for (int l = 0; l < nl; ++l) F->lvl_off[l + 1] += F->lvl_off[l];
    std::vector<int32_t> cursor(F->lvl_off.begin(), F->lvl_off.end() - 1), rowid((size_t)n), ptr((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) rowid[cursor[lvl[i]]++] = (int32_t)i;        // ascending row inside a level
    std::vector<int32_t> pos((size_t)n);
    for (int64_t p = 0; p < n; ++p) pos[rowid[p]] = (int32_t)p;
    if (pos_out) *pos_out = pos;
    const size_t nnz = ent.col.size();
    hvec<int32_t> col(nnz); hvec<double> val(nnz), dg((size_t)n);          // (every element is written below: not value-initialised)
    int64_t maxlen = 0, nlong = 0;
    for (int64_t p = 0; p < n; ++p) { const int64_t len = ent.len(rowid[p]); ptr[p + 1] = ptr[p] + (int32_t)len; maxlen = std::max(maxlen, len); nlong += len > 8; }
    par_rows(n, [&](int64_t lo, int64_t hi) {
        for (int64_t p = lo; p < hi; ++p) {
            const int32_t i = rowid[p];
            size_t w = (size_t)ptr[p];
            for (int64_t k = ent.ptr[i]; k < ent.ptr[i + 1]; ++k) { col[w] = pos[ent.col[k]]; val[w] = ent.val[k]; ++w; }   // columns as level-order positions
            dg[p] = diag[i];
        }
    });
    F->npos = n;
    choose_level_form(F, n, nl, maxlen, nlong, ptr[n]);
    if (F->ell) {
        hvec<int32_t> ecol((size_t)ELLW * n); hvec<double> eval((size_t)ELLW * n); hvec<uint8_t> elen((size_t)n);
        par_rows(n, [&](int64_t lo, int64_t hi) {
            for (int64_t p = lo; p < hi; ++p) {
                const int64_t len = ptr[p + 1] - ptr[p];
                elen[p] = (uint8_t)len;
                for (int64_t u = 0; u < ELLW; ++u) {                     // (padding slots: column 0, value 0)
                    ecol[(size_t)u * n + p] = u < len ? col[ptr[p] + u] : 0; eval[(size_t)u * n + p] = u < len ? val[ptr[p] + u] : 0.0;
                }
            }
        });
        KR_TRY(up(&F->d_ecol, ecol)); KR_TRY(up(&F->d_eval, eval)); KR_TRY(up(&F->d_elen, elen));
    }
    KR_TRY(up(&F->d_ptr, ptr)); KR_TRY(up(&F->d_col, col)); KR_TRY(up(&F->d_val, val)); KR_TRY(up(&F->d_row, rowid));
    KR_TRY(up(&F->d_diag, dg)); KR_TRY(up(&F->d_lvl_off, F->lvl_off));
    KR_TRY(build_free_streams(F, tl_setup_stream, ptr.data()));
    return KRYST_OK;
}

// Recognise a structured-grid factor and lay it out for tri_grid_kernel.  Not an error when it does not apply.
static int32_t build_grid(int64_t n, const FlatRows& ent, const hvec<double>& diag, bool forward, GridFactor* G) {
    if (n < 2 || n >= (1ll << 31) || env_int("KRYST_ILU_GRID", 1) == 0) return KRYST_OK;
    int64_t offs[3] = {0, 0, 0}; int no = 0;                              // distinct |col - row|, at most three
    {
        std::atomic<bool> reject{false};
        std::mutex mu;
        par_rows(n, [&](int64_t lo, int64_t hi) {
            int64_t mine[3] = {0, 0, 0}; int nm = 0;
            for (int64_t i = lo; i < hi && !reject.load(std::memory_order_relaxed); ++i)
                for (int64_t k = ent.ptr[i]; k < ent.ptr[i + 1]; ++k) {
                    const int64_t o = (int64_t)ent.col[k] - i;
                    if ((forward && o >= 0) || (!forward && o <= 0)) { reject = true; return; }
                    if (k > ent.ptr[i] && ent.col[k] <= ent.col[k - 1]) { reject = true; return; }   // the kernel subtracts in ascending column order (Ilut stores by magnitude)
                    const int64_t ao = o < 0 ? -o : o;
                    bool seen = false;
                    for (int q = 0; q < nm; ++q) seen = seen || mine[q] == ao;
                    if (!seen) { if (nm == 3) { reject = true; return; } mine[nm++] = ao; }
                }
            std::lock_guard<std::mutex> g(mu);
            for (int q = 0; q < nm; ++q) {
                bool seen = false;
                for (int r = 0; r < no; ++r) seen = seen || offs[r] == mine[q];
                if (!seen) { if (no == 3) { reject = true; return; } offs[no++] = mine[q]; }
            }
        });
        if (reject) return KRYST_OK;
    }
    std::sort(offs, offs + no);
    if (no < 2 || offs[0] != 1) return KRYST_OK;
    const int64_t s1 = offs[1], s2 = no == 3 ? offs[2] : n;
    if (s1 < 2 || s2 % s1 != 0 || n % s2 != 0 || s2 <= s1) return KRYST_OK;
    const int64_t Ni = s1, Nj = s2 / s1, Nk = n / s2;
    std::vector<double> c1((size_t)n, 0.0), c2((size_t)n, 0.0), c3((size_t)n, 0.0);
    {
        std::atomic<bool> reject{false};
        par_rows(n, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t ii = i % Ni, jx = (i / Ni) % Nj;
                for (int64_t k = ent.ptr[i]; k < ent.ptr[i + 1]; ++k) {
                    const int64_t ao = std::llabs((long long)ent.col[k] - (long long)i);
                    if (ao == 1) { if (forward ? ii == 0 : ii == Ni - 1) { reject = true; return; } c1[i] = ent.val[k]; }   // must stay on the line
                    else if (ao == s1) { if (forward ? jx == 0 : jx == Nj - 1) { reject = true; return; } c2[i] = ent.val[k]; }
                    else c3[i] = ent.val[k];
                }
            }
        });
        if (reject) return KRYST_OK;
    }
    KR_TRY(up(&G->d_c1, c1)); KR_TRY(up(&G->d_c2, c2)); KR_TRY(up(&G->d_c3, c3));
    if (!forward) KR_TRY(up(&G->d_diag, diag));
    G->Ni = (int32_t)Ni; G->Nj = (int32_t)Nj; G->Nk = (int32_t)Nk; G->ok = true;
    return KRYST_OK;
}

// Which box makes every offset of `offs` (col - row values, any sign) a step inside the 3 x 3 x 3 cube?  offset = di + Ni dj + Ni Nj dk with
// |d| <= 1.  Candidates for Ni (and for Ni Nj) are the offsets' magnitudes and their neighbours; the smallest consistent pair wins (any
// consistent pair gives a correct solve: the per-entry range checks of build_box make the decomposition unique for every row).
static bool box_decompose(int64_t o, int64_t s1, int64_t s2, int& dk, int& dj, int& di) {
    // o = di + s1 dj + s2 dk: take dk, dj as the nearest multiples
    const int64_t ao = o < 0 ? -o : o;
    for (int k = -1; k <= 1; ++k)
        for (int j = -1; j <= 1; ++j) {
            const int64_t rest = o - s2 * k - s1 * j;
            if (rest >= -1 && rest <= 1) { dk = k; dj = j; di = (int)rest; (void)ao; return true; }
        }
    return false;
}
bool box_dims_from_offsets(const std::vector<int64_t>& offs, int64_t n, int64_t* Ni_out, int64_t* Nj_out) {
    std::vector<int64_t> mags;
    for (int64_t o : offs) { const int64_t m = o < 0 ? -o : o; if (m > 0) mags.push_back(m); }
    std::sort(mags.begin(), mags.end()); mags.erase(std::unique(mags.begin(), mags.end()), mags.end());
    if (mags.empty() || mags.size() > 13) return false;
    std::vector<int64_t> cand;
    for (int64_t m : mags) for (int64_t c : {m - 1, m, m + 1}) if (c >= 3 && c <= n) cand.push_back(c);      // lines of at least 3 rows: +1 and -1 steps are distinct from +-Ni -+ 1
    cand.push_back(n);
    std::sort(cand.begin(), cand.end()); cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    for (int64_t s1 : cand) {
        if (n % s1 != 0) continue;
        for (int64_t s2 : cand) {
            if (s2 <= s1 || s2 % s1 != 0 || n % s2 != 0 || s2 / s1 < 3) continue;      // (at least 3 lines per plane, or one plane: s2 == n)
            bool all = true;
            for (int64_t o : offs) { int dk, dj, di; if (o != 0 && !box_decompose(o, s1, s2, dk, dj, di)) { all = false; break; } if (o != 0 && s2 == n && dk != 0) { all = false; break; } }
            if (all) { *Ni_out = s1; *Nj_out = s2 / s1; return true; }
        }
    }
    return false;
}

// entries per stream -> which streams a factor has, and whether each of those has an entry wherever the neighbour row exists in the box
void box_classify(const unsigned long long cnt[13], bool forward, int64_t Ni, int64_t Nj, int64_t Nk, BoxFactor* B) {
    B->present = 0; B->regular = true;
    for (int a = 0; a < 13; ++a) {
        const int code = forward ? a : a + 14, dk = code / 9 - 1, dj = (code / 3) % 3 - 1, di = code % 3 - 1;
        const int64_t expect = std::max<int64_t>(0, Ni - std::abs(di)) * std::max<int64_t>(0, Nj - std::abs(dj)) * std::max<int64_t>(0, Nk - std::abs(dk));
        if (cnt[a] != 0) B->present |= 1u << a;
        if (cnt[a] != 0 && (int64_t)cnt[a] != expect) B->regular = false;
    }
}

// one factor's kept entries (host FlatRows, uploaded) -> its 13 coefficient streams; `bad` is raised by an entry that is not a neighbour
// inside the box (it wraps around a line or plane end) or lies on the wrong side of the diagonal
__global__ __launch_bounds__(256) void box_rows_fill_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val, int32_t n,
                                                            int32_t Ni, int32_t Nj, int32_t Nk, int forward, double* c, int64_t cs, int32_t* bad, unsigned long long* counts) {
    __shared__ unsigned int cnt[13];
    if (threadIdx.x < 13) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int32_t ii = i % Ni, jj = (i / Ni) % Nj, kk = i / (Ni * Nj);
        for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) {
            const int32_t j = col[k];
            if (j < 0 || j >= n) { *bad = 1; break; }
            const int di = j % Ni - ii, dj = (j / Ni) % Nj - jj, dk = j / (Ni * Nj) - kk;
            if (di < -1 || di > 1 || dj < -1 || dj > 1 || dk < -1 || dk > 1 || kk + dk >= Nk) { *bad = 1; break; }
            const int code = 9 * (dk + 1) + 3 * (dj + 1) + (di + 1);
            if (forward ? code >= 13 : code <= 13) { *bad = 1; break; }
            c[(int64_t)(forward ? code : code - 14) * cs + i] = val[k];
            atomicAdd(&cnt[forward ? code : code - 14], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 13 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// Recognise a box-stencil factor and lay it out as 13 natural-order coefficient streams.  Not an error when it does not apply.
static int32_t build_box(int64_t n, const FlatRows& ent, const hvec<double>& diag, bool forward, BoxFactor* B) {
    if (n < 27 || n >= (1ll << 31) || ilu_box_knob() == 0) return KRYST_OK;
    // distinct offsets (at most 13), rows in ascending column order, strictly lower / upper
    std::vector<int64_t> offs;
    {
        std::atomic<bool> reject{false};
        std::mutex mu;
        par_rows(n, [&](int64_t lo, int64_t hi) {
            std::vector<int64_t> mine;
            for (int64_t i = lo; i < hi && !reject.load(std::memory_order_relaxed); ++i)
                for (int64_t k = ent.ptr[i]; k < ent.ptr[i + 1]; ++k) {
                    const int64_t o = (int64_t)ent.col[k] - i;
                    if ((forward && o >= 0) || (!forward && o <= 0)) { reject = true; return; }
                    if (k > ent.ptr[i] && ent.col[k] <= ent.col[k - 1]) { reject = true; return; }   // the kernels subtract in ascending column order
                    if (std::find(mine.begin(), mine.end(), o) == mine.end()) { if (mine.size() == 13) { reject = true; return; } mine.push_back(o); }
                }
            std::lock_guard<std::mutex> g(mu);
            for (int64_t o : mine) if (std::find(offs.begin(), offs.end(), o) == offs.end()) offs.push_back(o);
        });
        if (reject || offs.empty() || offs.size() > 13) return KRYST_OK;
    }
    int64_t Ni = 0, Nj = 0;
    if (!box_dims_from_offsets(offs, n, &Ni, &Nj)) return KRYST_OK;
    const int64_t Nk = n / (Ni * Nj);
    // the streams are written on the device from the uploaded rows (round 4: the host used to fill 13 n doubles per factor and send those)
    hipStream_t st = tl_setup_stream;
    int64_t* d_ptr = nullptr; int32_t* d_col = nullptr; double* d_val = nullptr; int32_t* d_bad = nullptr;
    const size_t cb = sizeof(double) * (size_t)13 * (size_t)box_stream_stride(n), ne = (size_t)ent.ptr[(size_t)n];
    int32_t bad = 1;
    bool ok = pool_malloc(&d_ptr, sizeof(int64_t) * ((size_t)n + 1)) == hipSuccess && pool_malloc(&d_col, sizeof(int32_t) * (ne + 1)) == hipSuccess &&
              pool_malloc(&d_val, sizeof(double) * (ne + 1)) == hipSuccess && pool_malloc(&d_bad, 128) == hipSuccess && pool_malloc(&B->d_c, cb) == hipSuccess;
    unsigned long long hostw[16];                                           // [0]: "not a box factor", [1..13]: entries per stream
    ok = ok && hipMemsetAsync(B->d_c, 0, cb, st) == hipSuccess && hipMemsetAsync(d_bad, 0, 128, st) == hipSuccess &&
         hipMemcpyAsync(d_ptr, ent.ptr.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d_col, ent.col.data(), sizeof(int32_t) * ne, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d_val, ent.val.data(), sizeof(double) * ne, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(box_rows_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_ptr, d_col, d_val, (int32_t)n, (int32_t)Ni, (int32_t)Nj, (int32_t)Nk,
                           forward ? 1 : 0, B->d_c, box_stream_stride(n), d_bad, reinterpret_cast<unsigned long long*>(d_bad) + 1);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(hostw, d_bad, 128, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        if (ok) bad = (int32_t)(hostw[0] & 0xffffffffull);
    }
    (void)pool_free(d_ptr); (void)pool_free(d_col); (void)pool_free(d_val); (void)pool_free(d_bad);
    if (!ok) { (void)hipGetLastError(); B->free_all(); set_error("box-stencil factor: device allocation or copy failed"); return KRYST_ERR_HIP; }
    if (bad != 0) { B->free_all(); return KRYST_OK; }
    if (!forward) KR_TRY(up(&B->d_diag, diag));
    box_classify(hostw + 1, forward, Ni, Nj, Nk, B);
    B->Ni = (int32_t)Ni; B->Nj = (int32_t)Nj; B->Nk = (int32_t)Nk; B->ok = true;
    return KRYST_OK;
}

// shared tail of every host-side ILU-family setup: recognise a structured grid or level-order both factors, then hand out the
// preconditioner object
static int32_t finish_ilu_pc(kryst_csr_t a, const FlatRows& le, const FlatRows& ue,
                             const hvec<double>& dg, kryst_pc_t* out) {
    kryst_ctx_t ctx = a->ctx;
    tl_setup_stream = ctx->s_main;
    const int64_t n = a->nrows;
    hvec<double> ones((size_t)n, 1.0);
    IluPc* pc = new IluPc(a);
    // structured-grid factors take the wavefront kernel; everything else is level-ordered
    int32_t rc = build_grid(n, le, ones, true, &pc->GL);
    if (rc == KRYST_OK) rc = build_grid(n, ue, dg, false, &pc->GU);
    if (pc->GL.ok && pc->GU.ok && (pc->GL.Ni != pc->GU.Ni || pc->GL.Nj != pc->GU.Nj)) pc->GL.ok = false;
    if (rc == KRYST_OK && !(pc->GL.ok && pc->GU.ok)) {
        pc->GL.free_all(); pc->GU.free_all(); pc->GL = GridFactor(); pc->GU = GridFactor();
        // box stencils wider than 7 points (round 4): natural-order streams, hyperplane / wavefront kernels, no level machinery
        rc = build_box(n, le, ones, true, &pc->BL);
        if (rc == KRYST_OK && pc->BL.ok) rc = build_box(n, ue, dg, false, &pc->BU);
        if (!(pc->BL.ok && pc->BU.ok && pc->BL.Ni == pc->BU.Ni && pc->BL.Nj == pc->BU.Nj)) { pc->BL.free_all(); pc->BU.free_all(); pc->BL = BoxFactor(); pc->BU = BoxFactor(); }
    }
    if (rc == KRYST_OK && !(pc->GL.ok && pc->GU.ok) && !(pc->BL.ok && pc->BU.ok)) {
        std::vector<int32_t> posL, posU;
        // the two factors' level orders are independent: side by side (each has its own host arrays; the uploads share the context's stream)
        // (the error text is thread-local and an exception must not leave a thread function: the worker hands both back -- ADVICE r04)
        int32_t rc_u = KRYST_OK;
        std::string err_u;
        std::thread upper([&] {
            try {
                (void)hipSetDevice(ctx->device);
                tl_setup_stream = ctx->s_main;
                rc_u = build_factor(n, ue, dg, false, &pc->U, &posU);
                if (rc_u != KRYST_OK) err_u = kryst_hip_last_error();
            } catch (const std::bad_alloc&) { rc_u = KRYST_ERR_ARG; err_u = "ILU set-up: out of host memory while level-ordering U";
            } catch (...) { rc_u = KRYST_ERR_ARG; err_u = "ILU set-up: unexpected exception while level-ordering U"; }
        });
        try { rc = build_factor(n, le, ones, true, &pc->L, &posL); }
        catch (const std::bad_alloc&) { rc = KRYST_ERR_ARG; set_error("ILU set-up: out of host memory while level-ordering L"); }
        upper.join();
        if (rc == KRYST_OK && rc_u != KRYST_OK) { rc = rc_u; set_error("%s", err_u.c_str()); }
        if (rc == KRYST_OK) {
            std::vector<int32_t> mapLU((size_t)n);
            for (int64_t i = 0; i < n; ++i) mapLU[posU[i]] = posL[i];
            rc = up(&pc->d_mapLU, mapLU);
        }
    }
    if (rc == KRYST_OK) rc = finish_ilu_device(pc);
    if (rc != KRYST_OK) { kryst_pc_destroy(pc); return rc; }
    *out = pc;
    return KRYST_OK;
}

static int32_t download_rows(kryst_csr_t a, hvec<int64_t>& rp, hvec<int32_t>& col, hvec<double>& val) {
    janitor_wait();
    rp.resize((size_t)a->nrows + 1); col.resize((size_t)a->nnz); val.resize((size_t)a->nnz);
    return kryst_csr_download(a, rp.data(), col.data(), val.data());
}

}  // namespace kr

using namespace kr;

extern "C" int32_t kryst_pc_ilu0(kryst_csr_t a, int32_t mode, kryst_pc_t* out) {
    KR_ARG(a && out && mode >= 0 && mode <= 2, "pc_ilu0");
    KR_ARG(a->nrows == a->xlen, "pc_ilu0: square operator required");
    kryst_ctx_t ctx = a->ctx;
    KR_HIP(hipSetDevice(ctx->device));
    {   // grid operators are factored on the device (no download, no host loops)
        kryst_pc_t pc = nullptr;
        KR_TRY(grid_setup_on_device(a, mode, &pc));
        if (pc) { *out = pc; return KRYST_OK; }
        KR_TRY(general_setup_on_device(a, mode, &pc));      // general operators: factor values, levels and the level-ordered factors on the device
        if (pc) { *out = pc; return KRYST_OK; }
    }
    const int64_t n = a->nrows, nnz = a->nnz;
    const bool verbose = getenv("KRYST_ILU_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_phase = now();
    auto lap = [&](const char* what) { if (verbose) { fprintf(stderr, "[kryst ilu] %s %.0f ms\n", what, std::chrono::duration<double, std::milli>(now() - t_phase).count()); t_phase = now(); } };
    std::vector<int64_t> rp((size_t)n + 1); std::vector<int32_t> col((size_t)nnz); std::vector<double> val((size_t)nnz);
    KR_TRY(kryst_csr_download(a, rp.data(), col.data(), val.data()));
    lap("download");
    // factor values on A's pattern (host_factor.cpp).  Textbook ILU(0): IKJ restricted to the pattern on the device first (one wave per row, rows
    // concurrent along the dependency graph), the same operations in the same order as the host loop, which takes over when
    // KRYST_ILU_DEVICE_SETUP=0 or the device path gave up
    std::vector<double> w(val);
    bool on_device = false;
    int64_t bad = -1;
    if (mode == KRYST_ILU_TRUE_ILU0) {
        KR_TRY(ikj_on_device(a, rp, col, w, &on_device, &bad));
        if (on_device && bad < 0) lap("device-side IKJ factorisation");
    }
    if (!on_device) bad = host_ilu0_values(n, rp.data(), col.data(), val.data(), mode, w.data());
    if (bad >= 0 && mode == KRYST_ILU_TRUE_ILU0) { set_error("ILU(0): zero pivot at row %lld", (long long)bad); set_error_row(bad); return KRYST_ZERO_PIVOT; }
    if (bad >= 0) { set_error("ILUP: zero diagonal in U at row %lld", (long long)bad); return KRYST_SOLVE_ERROR; }
    lap("factorisation");
    FlatRows le, ue;
    hvec<double> dg;
    host_ilu0_split(n, rp.data(), col.data(), w.data(), mode != KRYST_ILU_KRYST_COMPAT, le, ue, dg);      // ilu.rs:115-119 never divides
    lap("split into L / U rows");
    const int32_t rc = finish_ilu_pc(a, le, ue, dg, out);
    lap("device structures");
    return rc;
}
// Ilup::new(fill).setup(a) exactly as written (src/preconditioner/ilup.rs:77-134), on sparse rows instead of the reference's
// dense n x n `level` / `a_work` arrays: an entry that the dense code never touches is (0.0, usize::MAX) here too.
// Ilup(p >= 1), ilup.rs:77-167: IKJ elimination with level-of-fill bookkeeping; whether an entry takes part depends on its VALUE too
// (`!= 0.0` tests at :106, :117, :129), so pattern and values are computed together, row by row.  Row i only needs the finished rows j < i
// that appear in its working row (original entries and fill): rows are dealt out to the host's cores in small blocks, round-robin,
// every thread walks its blocks in ascending order and waits on the block's "finished" flag before it uses another thread's pivot row (round 4;
// one thread did all of it before: 300 ms of the 620 ms Ilup(1) setup at 128^3).  The lowest unfinished row never waits for an
// unfinished one, so somebody always makes progress.  The same operations on the same operands in the same order as the one-thread
// loop: same bits.
static int32_t ilup_setup(kryst_csr_t a, int32_t fill, kryst_pc_t* out);
extern "C" int32_t kryst_pc_ilup(kryst_csr_t a, int32_t fill, kryst_pc_t* out) {
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = ilup_setup(a, fill, out);
    if (getenv("KRYST_ILU_VERBOSE")) fprintf(stderr, "[kryst ilup] all of it, host arrays freed: %.0f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}
static int32_t ilup_setup(kryst_csr_t a, int32_t fill, kryst_pc_t* out) {
    KR_ARG(a && out && fill >= 0, "pc_ilup");
    KR_ARG(a->nrows == a->xlen, "pc_ilup: square operator required");
    if (fill == 0) return kryst_pc_ilu0(a, KRYST_ILU_ILUP0, out);
    KR_HIP(hipSetDevice(a->ctx->device));
    const int64_t n = a->nrows;
    const bool verbose = getenv("KRYST_ILU_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_phase = now();
    auto lap = [&](const char* what) { if (verbose) { fprintf(stderr, "[kryst ilup] %s %.0f ms\n", what, std::chrono::duration<double, std::milli>(now() - t_phase).count()); t_phase = now(); } };
    hvec<int64_t> rp; hvec<int32_t> col; hvec<double> val;
    KR_TRY(download_rows(a, rp, col, val));
    lap("download");
    // the elimination itself: the row pipeline over the host's cores (host_factor.cpp: host_ilup_rows -- ilup.rs:77-134 on sparse rows)
    IlupOptions opt;
    opt.threads = env_int("KRYST_ILUP_THREADS", 0); opt.block = std::max(1, env_int("KRYST_ILUP_BLOCK", 2048));
    opt.cpu_group = env_int("KRYST_ILUP_CPU_GROUP", 16); opt.verbose = verbose; opt.trace = verbose && getenv("KRYST_ILUP_TRACE") != nullptr;
    FlatRows le, ue; hvec<double> dg;
    long long zero_col = -1;
    std::shared_ptr<void> scratch;
    int hrc = 2;
    try { hrc = host_ilup_rows(n, rp.data(), col.data(), val.data(), fill, opt, le, ue, dg, &zero_col, &scratch); }
    catch (const std::bad_alloc&) { hrc = 2; }
    if (hrc == 1) { set_error("ILUP: zero diagonal in U at row %lld", zero_col); return KRYST_SOLVE_ERROR; }
    if (hrc != 0) { set_error("ILUP: out of host memory during the elimination"); return KRYST_ERR_ARG; }
    const int32_t rc = finish_ilu_pc(a, le, ue, dg, out);
    lap("device structures");
    // ~1 GB of host arrays at 128^3: unmapping them takes 60-70 ms, which the caller need not wait for
    struct Bundle { std::shared_ptr<void> scratch; FlatRows le, ue; hvec<int64_t> rp; hvec<int32_t> col; hvec<double> val; hvec<double> dg; };
    auto bundle = std::make_shared<Bundle>();
    bundle->scratch.swap(scratch);
    bundle->le.ptr.swap(le.ptr); bundle->le.col.swap(le.col); bundle->le.val.swap(le.val); bundle->ue.ptr.swap(ue.ptr); bundle->ue.col.swap(ue.col); bundle->ue.val.swap(ue.val);
    bundle->rp.swap(rp); bundle->col.swap(col); bundle->val.swap(val); bundle->dg.swap(dg);
    janitor_run(bundle);
    lap("host arrays handed to the janitor thread");
    return rc;
}

extern "C" int32_t kryst_pc_ilut(kryst_csr_t a, int32_t fill, double droptol, kryst_pc_t* out) {
    KR_ARG(a && out && fill >= 0, "pc_ilut");
    KR_ARG(a->nrows == a->xlen, "pc_ilut: square operator required");
    KR_HIP(hipSetDevice(a->ctx->device));
    const int64_t n = a->nrows;
    hvec<int64_t> rp; hvec<int32_t> col; hvec<double> val;
    KR_TRY(download_rows(a, rp, col, val));
    FlatRows le, ue; hvec<double> dg;
    try { host_ilut_rows(n, rp.data(), col.data(), val.data(), fill, droptol, le, ue, dg); }     // (host_factor.cpp; ilut.rs:80-150)
    catch (const std::bad_alloc&) { set_error("ILUT: out of host memory"); return KRYST_ERR_ARG; }
    return finish_ilu_pc(a, le, ue, dg, out);
}
