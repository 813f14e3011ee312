// The halo exchange of a row-partitioned operator's SpMV: grouped ncclSend / ncclRecv on the second stream, or direct peer stores into hipIpc-mapped landing
// buffers (dist.h: HaloPeer).  halo_begin starts one, halo_finish makes the compute stream wait for it; spmv.hip's launch_spmv runs the interior tiles in between.
#include "spmv.h"

namespace kr {
__global__ void pack_kernel(const double* x, const int32_t* idx, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[idx[i]];
}
void halo_send_tiles(kryst_csr_t a, std::vector<std::pair<int64_t, int64_t>>& ranges) {
    ranges.clear();
    if (!a->dist || !a->send_contiguous) return;
    const HaloPlan& pl = a->plan;
    for (size_t p = 0; p < pl.send_counts.size(); ++p)
        if (pl.send_counts[p] > 0) ranges.emplace_back(pl.send_off[p] / KR_TILE, (pl.send_off[p] + pl.send_counts[p] + KR_TILE - 1) / KR_TILE);
    std::sort(ranges.begin(), ranges.end());
    std::vector<std::pair<int64_t, int64_t>> merged;
    for (const auto& r : ranges) {
        if (!merged.empty() && r.first <= merged.back().second) merged.back().second = std::max(merged.back().second, r.second);
        else merged.push_back(r);
    }
    ranges.swap(merged);
}

// ---- halo exchange by direct peer stores (dist.h: HaloPeer)
// push: workgroup (bx, seg) stores its share of segment `seg` into the neighbour's landing buffer; the workgroup that finishes LAST (all
// data stores of the launch acknowledged: write-through system-scope stores + s_waitcnt vmcnt(0) in front of the ticket) stamps the epoch
// into every neighbour's cell -- the protocol of fold_ipc_logic_kernel (solver_common.h).
__global__ __launch_bounds__(256) void halo_push_kernel(const double* __restrict__ x, const int32_t* __restrict__ send_idx, const HaloPushSeg* __restrict__ segs,
                                                        int nsegs, int parity, unsigned long long epoch, unsigned int* ticket) {
    const HaloPushSeg sg = segs[blockIdx.y];
    double* dst = sg.dst + (size_t)parity * sg.dst_stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.count; i += (int64_t)gridDim.x * 256) {
        const double v = send_idx ? x[send_idx[sg.src + i]] : x[sg.src + i];
        __hip_atomic_store(dst + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __shared__ int last;
    __syncthreads();                                                  // every wave of the workgroup has had its stores acknowledged
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x * gridDim.y - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x < nsegs) __hip_atomic_store(segs[threadIdx.x].stamp, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next (stream-ordered) push
}
// pull: wait for the sender's stamp, then landing[parity] -> d_halo (uncached reads: the landing buffer is written by another agent).
// A stamp that never comes (budget) poisons the halo with NaNs and raises the context's error word instead of hanging the GPU.
__global__ __launch_bounds__(256) void halo_pull_kernel(const double* __restrict__ landing, double* __restrict__ halo, const HaloPullSeg* __restrict__ segs,
                                                        unsigned long long epoch, int budget, unsigned int* err) {
    const HaloPullSeg sg = segs[blockIdx.y];
    __shared__ int ok;
    if (threadIdx.x == 0) {
        // (a pull that has given up once on this context stays given up until the host has read the error word: the exchanges a solver has
        // already enqueued behind it must not burn the budget again, one after the other)
        int b = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1 : budget;
        unsigned long long seen = __hip_atomic_load(sg.stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        while (seen < epoch && --b > 0) { __builtin_amdgcn_s_sleep(2); seen = __hip_atomic_load(sg.stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
        ok = seen >= epoch ? 1 : 0;
        if (!ok) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const bool good = ok != 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.count; i += (int64_t)gridDim.x * 256)
        halo[sg.off + i] = good ? __hip_atomic_load(landing + sg.off + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : __longlong_as_double(0x7FF8000000000000ll);
}

// the landing buffer's first state (data and stamps zero), written with the stores its later writers use
__global__ void halo_landing_init_kernel(double* landing, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) __hip_atomic_store(landing + i, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

void halo_peer_destroy(kryst_csr_t a) {
    HaloPeer& hp = a->plan.peer;
    for (void* q : hp.opened) ipc_close_shared(q);
    hp.opened.clear();
    // A landing buffer that a rank THREAD of this process stores into by raw pointer (no hipIpc mapping keeps the memory alive for it) outlives
    // the operator: a slower neighbour's last early push (cg_pcg.hip: launch_direction) may still be queued when this rank destroys its
    // operator.  It is freed with the context (ctx.cpp), after the streams of every rank of a rehearsal have drained.
    if (hp.landing && hp.sibling) { a->ctx->deferred_free.push_back(hp.landing); hp.landing = nullptr; }
    (void)hipFree(hp.landing); (void)hipFree(hp.d_push); (void)hipFree(hp.d_pull); (void)hipFree(hp.d_ticket);
    hp.landing = nullptr; hp.d_push = nullptr; hp.d_pull = nullptr; hp.d_ticket = nullptr; hp.on = false;
    (void)hipGetLastError();
}

int32_t halo_peer_setup(kryst_csr_t a) {
    kryst_ctx_t ctx = a->ctx;
    HaloPlan& pl = a->plan;
    HaloPeer& hp = pl.peer;
    if (hp.on) return KRYST_OK;
    if (hp.landing && hp.failed) { set_error("halo by peer stores: the test exchange failed on this operator before; the RCCL exchange stays in use"); return KRYST_UNSUPPORTED; }
    if (hp.landing) { hp.on = true; return KRYST_OK; }               // set up before and switched off: still mapped everywhere, epochs counted alike
    KR_ARG(a->dist && ctx->comm, "halo_peer_setup: not a distributed operator");
    const int P = ctx->nranks, me = ctx->rank;
    KR_ARG(P <= 257, "halo by peer stores: at most 256 neighbours (one stamping lane each)");      // (the same answer on every rank: P is)
    KR_HIP(hipStreamSynchronize(ctx->s_comm));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    // local: landing buffer (zeroed: stamps start at epoch 0); a rank that fails here, or whose neighbour relations are not mutual, still
    // takes part in the collectives below with a null buffer, which then fail on every rank alike
    bool mutual = true;
    for (int p = 0; p < P; ++p) mutual = mutual && ((pl.send_counts[p] > 0) == (pl.recv_counts[p] > 0));
    hp.stride = std::max<int64_t>(2, (pl.total_recv + 1) & ~(int64_t)1);
    const size_t bytes = sizeof(double) * (size_t)(2 * hp.stride + 2 * P);
    // (everything this rank allocates is allocated BEFORE the collectives: a rank that fails alone afterwards would leave the others switched on)
    if (!mutual || hipMalloc(&hp.d_push, sizeof(HaloPushSeg) * ((size_t)P + 1)) != hipSuccess || hipMalloc(&hp.d_pull, sizeof(HaloPullSeg) * ((size_t)P + 1)) != hipSuccess ||
        hipMalloc(&hp.d_ticket, 64) != hipSuccess || hipMemsetAsync(hp.d_ticket, 0, 64, ctx->s_main) != hipSuccess ||
        hipExtMallocWithFlags((void**)&hp.landing, std::max<size_t>(bytes, (size_t)2 << 20), hipDeviceMallocFinegrained) != hipSuccess) {   // (an allocation of its own: dist.cpp, ipc_reduce_setup)
        (void)hipGetLastError();
        (void)hipFree(hp.landing); hp.landing = nullptr;
    }
    if (hp.landing) {
        const int64_t cnt = (int64_t)(bytes / sizeof(double));
        hipLaunchKernelGGL(halo_landing_init_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->s_main, hp.landing, cnt);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(hp.landing); hp.landing = nullptr; }
    }
    std::vector<void*> peers;
    // (a pull kernel waits for a push its neighbour's host thread enqueues LATER -- at its next exchange: rank threads that share one device are refused)
    int32_t rc = ipc_map_peers(ctx, hp.landing, peers, hp.opened, false, &hp.sibling);
    if (rc != KRYST_OK) { halo_peer_destroy(a); return rc; }
    // where my rows land in each neighbour's buffer: every rank's {stride, recv_off[0..P)} in one all-gather
    std::vector<int64_t> mine((size_t)P + 1), all((size_t)(P + 1) * P, 0);
    mine[0] = hp.stride;
    for (int p = 0; p < P; ++p) mine[(size_t)p + 1] = pl.recv_off[p];
    int64_t *d_s = nullptr, *d_r = nullptr;
    if (hipMalloc(&d_s, sizeof(int64_t) * (P + 1)) != hipSuccess || hipMalloc(&d_r, sizeof(int64_t) * (size_t)(P + 1) * P) != hipSuccess) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK && (hipMemcpyAsync(d_s, mine.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK) rc = comm_all_gather_i64(ctx, d_s, d_r, P + 1, ctx->s_main);
    if (rc == KRYST_OK && (hipMemcpyAsync(all.data(), d_r, sizeof(int64_t) * all.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    (void)hipFree(d_s); (void)hipFree(d_r);
    if (rc != KRYST_OK) { halo_peer_destroy(a); return rc; }         // (a failing collective fails on every rank)
    std::vector<HaloPushSeg> push; std::vector<HaloPullSeg> pull;
    hp.push_max = hp.pull_max = 0;
    // (send_off: for contiguous lists the first local row of the run, otherwise the list's first entry in d_send_idx -- csr_create.hip)
    for (int p = 0; p < P; ++p) {
        if (p != me && pl.send_counts[p] > 0) {
            const int64_t pstride = all[(size_t)(P + 1) * p], poff = all[(size_t)(P + 1) * p + 1 + me];
            double* base = static_cast<double*>(peers[p]);
            push.push_back(HaloPushSeg{base + poff, reinterpret_cast<unsigned long long*>(base + 2 * pstride + 2 * me), pstride, pl.send_off[p], pl.send_counts[p]});
            hp.push_max = std::max(hp.push_max, pl.send_counts[p]);
        }
        if (p != me && pl.recv_counts[p] > 0) {
            pull.push_back(HaloPullSeg{reinterpret_cast<const unsigned long long*>(hp.landing + 2 * hp.stride + 2 * p), pl.recv_off[p], pl.recv_counts[p]});
            hp.pull_max = std::max(hp.pull_max, pl.recv_counts[p]);
        }
    }
    hp.npush = (int)push.size(); hp.npull = (int)pull.size();
    if (env_int("KRYST_HALO_DEBUG", 0)) {
        fprintf(stderr, "[kryst halo rank %d] landing %p stride %lld total_recv %lld\n", me, (void*)hp.landing, (long long)hp.stride, (long long)pl.total_recv);
        for (int p = 0; p < P; ++p) fprintf(stderr, "[kryst halo rank %d]   peer %d -> %p\n", me, p, peers[p]);
        for (auto& q : push) fprintf(stderr, "[kryst halo rank %d]   push dst %p stamp %p dst_stride %lld src %lld count %lld\n", me, (void*)q.dst, (void*)q.stamp, (long long)q.dst_stride, (long long)q.src, (long long)q.count);
        for (auto& q : pull) fprintf(stderr, "[kryst halo rank %d]   pull stamp %p off %lld count %lld\n", me, (const void*)q.stamp, (long long)q.off, (long long)q.count);
    }
    if (!push.empty()) KR_HIP(hipMemcpyAsync(hp.d_push, push.data(), sizeof(HaloPushSeg) * push.size(), hipMemcpyHostToDevice, ctx->s_main));
    if (!pull.empty()) KR_HIP(hipMemcpyAsync(hp.d_pull, pull.data(), sizeof(HaloPullSeg) * pull.size(), hipMemcpyHostToDevice, ctx->s_main));
    KR_HIP(hipStreamSynchronize(ctx->s_main));
    hp.on = true;
    return halo_peer_selftest(a);
}

// One real exchange over the freshly mapped buffers before anybody relies on them: x[i] = this rank's global row number, pushed, pulled
// and compared with the plan's column list on every rank; the verdict is agreed through an all-gather, so the peer stores are on everywhere
// or nowhere (KRYST_UNSUPPORTED: the RCCL exchange stays).  A mapping that "succeeds" but does not carry the stores -- the one failure the
// set-up itself cannot see -- ends here with a short poll budget instead of in a user's solve.  KRYST_HALO_SELFTEST=0 skips it.
__global__ void halo_iota_kernel(double* x, int64_t n, int64_t base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = (double)(base + i);
}
int32_t halo_peer_selftest(kryst_csr_t a) {
    kryst_ctx_t ctx = a->ctx;
    HaloPlan& pl = a->plan;
    if (env_int("KRYST_HALO_SELFTEST", 1) == 0) return KRYST_OK;
    const int P = ctx->nranks;
    int64_t ok = 1;
    double* x = nullptr;
    std::vector<double> got((size_t)pl.total_recv);
    const bool have_cols = (int64_t)pl.recv_cols.size() == pl.total_recv;
    const size_t xbytes = sizeof(double) * (size_t)((a->xlen + KR_TILE - 1) / KR_TILE * KR_TILE + KR_TILE);
    if (hipMalloc(&x, xbytes) != hipSuccess) { (void)hipGetLastError(); ok = 0; x = nullptr; }
    // (a rank that could not allocate still takes part: its neighbours' pulls need its push -- of anything -- and everybody its vote)
    double* src = x ? x : pl.d_halo;                                    // never dereferenced beyond the plan's rows when ok; garbage otherwise
    if (x) {
        hipLaunchKernelGGL(halo_iota_kernel, dim3((unsigned)((a->xlen + 255) / 256)), dim3(256), 0, ctx->s_main, x, a->xlen, pl.row_lo);
        if (hipGetLastError() != hipSuccess) { (void)hipGetLastError(); ok = 0; }
    }
    int32_t rc = KRYST_OK;
    if (x) {
        rc = halo_begin(a, src);
        if (rc == KRYST_OK) rc = halo_finish(a, 1 << 24);     // (a short budget by the solvers' standards -- 2^26 -- yet long enough for peers that time-slice one GPU in the tests)
    } else {
        ++pl.peer.epoch;                                                // keep the exchange count in step with the other ranks
    }
    a->halo_started_for = nullptr;
    if (rc == KRYST_OK && (hipStreamSynchronize(ctx->s_comm) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) { (void)hipGetLastError(); ok = 0; }
    if (rc != KRYST_OK) ok = 0;
    if (fold_gave_up(ctx)) ok = 0;                                      // (reads and clears the error word of the pull)
    if (ok && pl.total_recv > 0) {
        if (hipMemcpyAsync(got.data(), pl.d_halo, sizeof(double) * got.size(), hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
            hipStreamSynchronize(ctx->s_main) != hipSuccess) { (void)hipGetLastError(); ok = 0; }
        for (int p = 0; p < P && ok; ++p) {
            const int64_t lo = a->row_offsets.size() > (size_t)p + 1 ? a->row_offsets[(size_t)p] : 0, hi = a->row_offsets.size() > (size_t)p + 1 ? a->row_offsets[(size_t)p + 1] : (1ll << 62);
            for (int64_t k = 0; k < pl.recv_counts[p] && ok; ++k) {
                const double v = got[(size_t)(pl.recv_off[p] + k)];
                if (have_cols) ok = v == (double)pl.recv_cols[(size_t)(pl.recv_off[p] + k)];
                else ok = v >= (double)lo && v < (double)hi && (k == 0 || v > got[(size_t)(pl.recv_off[p] + k - 1)]);      // rows of rank p, ascending
            }
        }
    }
    (void)hipFree(x);
    (void)hipMemsetAsync(pl.d_halo, 0, sizeof(double) * (size_t)(pl.total_recv + 2), ctx->s_main);
    // the agreed verdict
    int64_t *d_s = nullptr, *d_r = nullptr;
    std::vector<int64_t> all((size_t)P, 0);
    rc = KRYST_OK;
    if (hipMalloc(&d_s, 8) != hipSuccess || hipMalloc(&d_r, sizeof(int64_t) * P) != hipSuccess) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK && (hipMemcpyAsync(d_s, &ok, 8, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK) rc = comm_all_gather_i64(ctx, d_s, d_r, 1, ctx->s_main);
    if (rc == KRYST_OK && (hipMemcpyAsync(all.data(), d_r, sizeof(int64_t) * P, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    (void)hipFree(d_s); (void)hipFree(d_r);
    if (rc != KRYST_OK) { (void)hipGetLastError(); a->plan.peer.on = false; return rc; }
    for (int p = 0; p < P; ++p)
        if (all[(size_t)p] != 1) {
            a->plan.peer.on = false;                                    // (the buffers stay mapped; a later kryst_csr_halo_mode(a, 1) tests again)
            a->plan.peer.failed = true;
            set_error("halo by peer stores: the test exchange did not arrive intact on rank %d; the RCCL exchange stays in use", p);
            return KRYST_UNSUPPORTED;
        }
    return KRYST_OK;
}

// messages up to this many bytes in total are pushed from the compute stream itself (no second stream, no event): below it the two
// cross-stream dependencies cost more than the stores' time on the wire
static int64_t halo_inline_bytes() { return env_ll("KRYST_HALO_INLINE_BYTES", 256 << 10); }

int32_t halo_begin(kryst_csr_t a, const double* x) {
    kryst_ctx_t ctx = a->ctx;
    HaloPlan& pl = a->plan;
    if (pl.peer.on) {
        HaloPeer& hp = pl.peer;
        ++hp.epoch;
        const bool inl = pl.total_send * 8 <= halo_inline_bytes();
        hipStream_t s = inl ? ctx->s_main : ctx->s_comm;
        if (!inl) {
            KR_HIP(hipEventRecord(ctx->ev_x_ready, ctx->s_main));
            KR_HIP(hipStreamWaitEvent(ctx->s_comm, ctx->ev_x_ready, 0));
        }
        if (hp.npush > 0) {
            const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>(1, (hp.push_max + 1023) / 1024), 64);   // <= 64 workgroups per neighbour: the wire, not the CUs, bounds it
            hipLaunchKernelGGL(halo_push_kernel, dim3(gx, (unsigned)hp.npush), dim3(256), 0, s, x, a->send_contiguous ? nullptr : pl.d_send_idx, hp.d_push, hp.npush,
                               (int)(hp.epoch & 1ull), hp.epoch, hp.d_ticket);
            KR_HIP(hipGetLastError());
        }
        if (!inl) KR_HIP(hipEventRecord(ctx->ev_halo_done, ctx->s_comm));
        a->halo_pushed_inline = inl;
        a->halo_started_for = x;
        return KRYST_OK;
    }
    KR_HIP(hipEventRecord(ctx->ev_x_ready, ctx->s_main));
    KR_HIP(hipStreamWaitEvent(ctx->s_comm, ctx->ev_x_ready, 0));
    const void* sendbase = pl.d_sendbuf;
    if (a->send_contiguous) {
        // k-slab stencils: every send list is a contiguous run of x; ship it in place
        // (send_off then holds the first local row of each run, see kryst_csr_create_dist)
        sendbase = x;
    } else if (pl.total_send > 0) {
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((pl.total_send + 255) / 256)), dim3(256), 0, ctx->s_comm,
                           x, pl.d_send_idx, pl.d_sendbuf, pl.total_send);
        KR_HIP(hipGetLastError());
    }
    KR_TRY(comm_exchange(ctx, sendbase, pl.send_counts.data(), pl.send_off.data(), pl.d_halo, pl.recv_counts.data(),
                         pl.recv_off.data(), true, ctx->s_comm));
    KR_HIP(hipEventRecord(ctx->ev_halo_done, ctx->s_comm));
    a->halo_started_for = x;
    return KRYST_OK;
}

// the receiving half of an exchange halo_begin started: afterwards the compute stream may read the plan's d_halo (budget <= 0: the default poll budget)
int32_t halo_finish(kryst_csr_t a, int budget) {
    kryst_ctx_t ctx = a->ctx;
    if (a->plan.peer.on) {
        HaloPeer& hp = a->plan.peer;
        // (my own push has read x: only needed before x is overwritten, and long since true -- the one local dependency that is left)
        if (!a->halo_pushed_inline) KR_HIP(hipStreamWaitEvent(ctx->s_main, ctx->ev_halo_done, 0));
        if (hp.npull > 0) {
            static const int dflt = [] { const char* e = getenv("KRYST_IPC_POLL_BUDGET"); return e ? std::max(1, atoi(e)) : (1 << 26); }();
            const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>(1, (hp.pull_max + 1023) / 1024), 256);
            hipLaunchKernelGGL(halo_pull_kernel, dim3(gx, (unsigned)hp.npull), dim3(256), 0, ctx->s_main, hp.landing + (size_t)(hp.epoch & 1ull) * hp.stride,
                               a->plan.d_halo, hp.d_pull, hp.epoch, budget > 0 ? std::min(budget, dflt) : dflt, fold_err(ctx) + 1);
            KR_HIP(hipGetLastError());
        }
    } else {
        KR_HIP(hipStreamWaitEvent(ctx->s_main, ctx->ev_halo_done, 0));
    }
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;
extern "C" {
// How the operator's halo exchange travels: mode 0 = grouped ncclSend / ncclRecv on the second stream (default), 1 = direct peer stores
// into hipIpc-mapped landing buffers (dist.h: HaloPeer).  COLLECTIVE: every rank calls it with the same mode.  KRYST_UNSUPPORTED (mode 1)
// when some rank cannot export / map a landing buffer or a neighbour relation is one-way: every rank then stays on RCCL.  *active: the
// mode in use.  The results are bit-identical either way (the same values land in the same halo slots).
int32_t kryst_csr_halo_mode(kryst_csr_t a, int32_t mode, int32_t* active) {
    KR_ARG(a && (mode == 0 || mode == 1 || mode == -1), "csr_halo_mode");
    if (mode == -1) { if (active) *active = a->plan.peer.on ? 1 : 0; return KRYST_OK; }       // query only
    KR_ARG(a->ctx->active_ws == nullptr, "csr_halo_mode: a solve or stepping session is open on this context");
    int32_t rc = KRYST_OK;
    if (a->dist && a->ctx->comm) {
        KR_HIP(hipSetDevice(a->ctx->device));
        KR_HIP(hipStreamSynchronize(a->ctx->s_comm));
        KR_HIP(hipStreamSynchronize(a->ctx->s_main));
        a->halo_started_for = nullptr;
        // a pull that gave up earlier must not hand its exhausted patience to the mode chosen now (the word is sticky until the host reads it)
        KR_HIP(hipMemsetAsync(fold_err(a->ctx) + 1, 0, sizeof(unsigned int), a->ctx->s_main));
        KR_HIP(hipStreamSynchronize(a->ctx->s_main));
        if (mode == 1) rc = halo_peer_setup(a);
        else a->plan.peer.on = false;            // (the landing buffers stay mapped: switching back costs nothing)
    }
    if (active) *active = a->plan.peer.on ? 1 : 0;
    return rc;
}

}  // extern "C"

namespace kr {
// A freshly created row-partitioned operator takes the peer-store exchange when every rank can map its neighbours' landing buffers and the
// test exchange arrives intact everywhere (agreed outcome); otherwise -- not an error -- the grouped ncclSend / ncclRecv exchange stays.
// KRYST_HALO_MODE=rccl: do not try.  COLLECTIVE like the creation itself.
int32_t halo_default_mode(kryst_csr_t a) {
    if (!a->dist || !a->ctx->comm || a->ctx->nranks < 2) return KRYST_OK;
    const char* e = getenv("KRYST_HALO_MODE");
    if (e && strcmp(e, "rccl") == 0) return KRYST_OK;
    const int32_t rc = kryst_csr_halo_mode(a, 1, nullptr);
    return rc == KRYST_UNSUPPORTED ? KRYST_OK : rc;
}
}
