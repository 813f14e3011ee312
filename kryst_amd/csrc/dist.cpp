// RCCL binding + halo planning.  Compiled with hipcc (host code only).
#include "dist.h"
#include "ipc_table.h"
#include <map>
#include <array>
#include <mutex>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <mutex>
#include <unistd.h>
#include <ctime>
#include <cstdio>

namespace kr {

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
};
static Rccl g_rccl;

struct Comm { ncclComm_t comm = nullptr; };

static std::mutex g_rccl_mutex;             // several ranks of one process (one host thread each) may create their contexts at once
static int32_t rccl_load() {
    const std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return KRYST_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    // KRYST_RCCL_LIB: an alternative library exporting the same nine symbols (the tests' shared-GPU stand-in)
    if (const char* alt = getenv("KRYST_RCCL_LIB")) {
        h = dlopen(alt, RTLD_NOW | RTLD_LOCAL);
        if (!h) { set_error("cannot load KRYST_RCCL_LIB=%s: %s", alt, dlerror()); return KRYST_ERR_RCCL; }
    }
    for (const char* nm : names) { if (h) break; h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); }
    if (!h) { set_error("cannot load librccl.so.1: %s", dlerror()); return KRYST_ERR_RCCL; }
#define SYM(field, name)                                                       \
    *(void**)(&g_rccl.field) = dlsym(h, name);                                 \
    if (!g_rccl.field) { set_error("RCCL symbol %s missing", name); return KRYST_ERR_RCCL; }
    SYM(GetUniqueId, "ncclGetUniqueId") SYM(CommInitRank, "ncclCommInitRank") SYM(CommDestroy, "ncclCommDestroy")
    SYM(GetErrorString, "ncclGetErrorString") SYM(AllGather, "ncclAllGather") SYM(Send, "ncclSend")
    SYM(Recv, "ncclRecv") SYM(GroupStart, "ncclGroupStart") SYM(GroupEnd, "ncclGroupEnd")
#undef SYM
    g_rccl.lib = h;
    return KRYST_OK;
}

#define KR_NCCL(call)                                                                                  \
    do {                                                                                               \
        ncclResult_t r__ = (call);                                                                     \
        if (r__ != ncclSuccess) {                                                                      \
            set_error("%s failed: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r__) : "?"); \
            return KRYST_ERR_RCCL;                                                                     \
        }                                                                                              \
    } while (0)

int32_t comm_unique_id(void* out128) {
    KR_TRY(rccl_load());
    ncclUniqueId id;
    KR_NCCL(g_rccl.GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(out128, &id, 128);
    return KRYST_OK;
}

int32_t comm_init(kryst_ctx_t ctx, const void* uid128) {
    KR_TRY(rccl_load());
    ncclUniqueId id;
    memcpy(&id, uid128, 128);
    ctx->comm = new Comm();
    KR_NCCL(g_rccl.CommInitRank(&ctx->comm->comm, ctx->nranks, id, ctx->rank));
    return KRYST_OK;
}

void comm_destroy(kryst_ctx_t ctx) {
    ipc_reduce_destroy(ctx);
    if (ctx->comm) {
        if (ctx->comm->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm->comm);
        delete ctx->comm;
        ctx->comm = nullptr;
    }
}

int32_t comm_all_gather(kryst_ctx_t ctx, const double* send, double* recv, int count) {
    KR_ARG(ctx->comm, "context has no communicator");
    KR_NCCL(g_rccl.AllGather(send, recv, (size_t)count, ncclFloat64, ctx->comm->comm, ctx->s_main));
    return KRYST_OK;
}

int32_t comm_all_gather_i64(kryst_ctx_t ctx, const int64_t* send, int64_t* recv, int count, hipStream_t s) {
    KR_ARG(ctx->comm, "context has no communicator");
    KR_NCCL(g_rccl.AllGather(send, recv, (size_t)count, ncclInt64, ctx->comm->comm, s));
    return KRYST_OK;
}

int32_t comm_exchange(kryst_ctx_t ctx, const void* send, const int64_t* send_counts, const int64_t* send_off,
                      void* recv, const int64_t* recv_counts, const int64_t* recv_off, bool is_double, hipStream_t s) {
    KR_ARG(ctx->comm, "context has no communicator");
    const ncclDataType_t dt = is_double ? ncclFloat64 : ncclInt64;
    KR_NCCL(g_rccl.GroupStart());
    for (int p = 0; p < ctx->nranks; ++p) {
        if (p == ctx->rank) continue;
        if (send_counts[p] > 0)
            KR_NCCL(g_rccl.Send((const char*)send + 8 * send_off[p], (size_t)send_counts[p], dt, p, ctx->comm->comm, s));
        if (recv_counts[p] > 0)
            KR_NCCL(g_rccl.Recv((char*)recv + 8 * recv_off[p], (size_t)recv_counts[p], dt, p, ctx->comm->comm, s));
    }
    KR_NCCL(g_rccl.GroupEnd());
    return KRYST_OK;
}

// ---- scalar all-reduce through IPC-mapped mailboxes (replaces the two tiny RCCL all-gathers of a CG iteration: Comm::all_reduce,
// src/parallel/mpi_comm.rs:116-121 / DistributedInnerProduct, src/core/wrappers.rs:134-156)
void ipc_reduce_destroy(kryst_ctx_t ctx) {
    for (void* p : ctx->ipc_opened) ipc_close_shared(p);
    ctx->ipc_opened.clear();
    (void)hipFree(ctx->ipc_mine); (void)hipFree(ctx->d_ipc_peers); (void)hipFree(ctx->d_ipc_epoch);
    ctx->ipc_mine = nullptr; ctx->d_ipc_peers = nullptr; ctx->d_ipc_epoch = nullptr; ctx->ipc_on = false;
    (void)hipGetLastError();
}

// hipIpcOpenMemHandle / hipIpcCloseMemHandle, once per handle and PROCESS: two ranks of one process (rank threads) both want their common
// peers' buffers, and a second open of a handle the process already holds -- or two opens of it at the same moment -- is not something the
// runtime promises to survive (seen on one box in four: the mailbox set-up of the 4 x 2 rehearsal fell back to RCCL now and then).  The
// mappings are shared and counted; the last close unmaps (ipc_table.h: the counting itself, free of HIP so that the sanitizer tier runs it).
namespace {
struct HipIpcOps {
    static int open(void** ptr, const SharedMappingKey& key) {
        hipIpcMemHandle_t h; memcpy(&h, key.data(), 64);
        return (int)hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess);
    }
    static void close(void* ptr) { (void)hipIpcCloseMemHandle(ptr); }
};
SharedMappings<HipIpcOps> g_ipc_open;
}  // namespace
hipError_t ipc_open_shared(void** ptr, const hipIpcMemHandle_t& h) {
    SharedMappingKey key; memcpy(key.data(), &h, 64);
    int dev = -1; (void)hipGetDevice(&dev); memcpy(key.data() + 64, &dev, 4);      // key: the handle and the device it is opened on
    return (hipError_t)g_ipc_open.open(ptr, key);
}
void ipc_close_shared(void* ptr) { g_ipc_open.close(ptr); }

// Map one allocation of every rank into this process: `mine` (device memory of this rank, fine-grained when peers write it with
// system-scope stores) is exported, the handles travel in one all-gather, and peers[p] receives rank p's allocation as THIS process
// addresses it (own entry: mine).  A peer that lives in this very process (several ranks of one process, one host thread each) is
// addressed directly -- hipIpcOpenMemHandle refuses a handle of its own process -- after peer access to its device has been enabled.
// Collective; the outcome is agreed: KRYST_OK on every rank, or KRYST_UNSUPPORTED (nothing left mapped) on every rank.
// same_device_siblings = false refuses ranks of this process that share this rank's DEVICE (a rehearsal set-up: several rank threads on
// one GPU): for them a kernel of one rank that waits for a kernel the sibling's host thread has yet to enqueue can wait for ever, because
// host calls of that thread which synchronise the device or stage through the runtime (hipFree, a copy to pageable memory) wait for the
// waiting kernel first -- measured: tools/peer_debug.py, DESIGN.md section 6.
// Who a rank's process is, beyond its pid: pids repeat across nodes, PID namespaces and containers (pods start with small pids), and a
// foreign rank that merely shares this process's pid must never be addressed by its raw device pointer.  A random 64-bit nonce drawn once
// per process plus a hash of the host's boot id and name: only a rank that carries BOTH of this process's values lives in this address space.
static uint64_t process_nonce() {
    static const uint64_t nonce = [] {
        uint64_t v = 0;
        if (FILE* f = fopen("/dev/urandom", "rb")) { if (fread(&v, sizeof v, 1, f) != 1) v = 0; fclose(f); }
        if (v == 0) v = ((uint64_t)getpid() * 0x9E3779B97F4A7C15ull) ^ (uint64_t)(uintptr_t)&v ^ (uint64_t)time(nullptr);
        return v | 1ull;
    }();
    return nonce;
}
static uint64_t host_hash() {
    static const uint64_t h = [] {
        uint64_t x = 0xcbf29ce484222325ull;                              // FNV-1a over boot id + host name
        auto eat = [&x](const char* s, size_t n) { for (size_t i = 0; i < n; ++i) { x ^= (unsigned char)s[i]; x *= 0x100000001b3ull; } };
        char buf[256];
        if (FILE* f = fopen("/proc/sys/kernel/random/boot_id", "rb")) { const size_t n = fread(buf, 1, sizeof buf, f); fclose(f); eat(buf, n); }
        if (gethostname(buf, sizeof buf) == 0) { buf[sizeof buf - 1] = 0; eat(buf, strlen(buf)); }
        return x;
    }();
    return h;
}

int32_t ipc_map_peers(kryst_ctx_t ctx, void* mine, std::vector<void*>& peers, std::vector<void*>& opened, bool same_device_siblings, bool* sibling) {
    if (sibling) *sibling = false;
    KR_ARG(ctx->comm, "ipc_map_peers: context has no communicator");
    const int P = ctx->nranks, me = ctx->rank;
    constexpr int W = 14;                      // words per rank: ok, pid, device, address, process nonce, host hash, handle[8]
    int64_t send[W] = {0};
    hipIpcMemHandle_t hmine;
    memset(&hmine, 0, sizeof hmine);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    int64_t ok_mine = mine != nullptr ? 1 : 0;
    const char* why = "";
    if (!ok_mine) why = "no buffer to export";
    if (ok_mine) { const hipError_t e = hipIpcGetMemHandle(&hmine, mine); if (e != hipSuccess) { (void)hipGetLastError(); ok_mine = 0; why = hipGetErrorString(e); set_error("hipIpcGetMemHandle: %s", why); } }
    send[0] = ok_mine; send[1] = (int64_t)getpid(); send[2] = ctx->device; send[3] = (int64_t)(uintptr_t)mine;
    send[4] = (int64_t)process_nonce(); send[5] = (int64_t)host_hash(); memcpy(send + 6, &hmine, 64);
    std::vector<int64_t> all((size_t)W * P, 0);
    int64_t *d_s = nullptr, *d_r = nullptr;
    int32_t rc = KRYST_OK;
    if (hipMalloc(&d_s, sizeof send) != hipSuccess || hipMalloc(&d_r, sizeof(int64_t) * W * P) != hipSuccess) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK && (hipMemcpyAsync(d_s, send, sizeof send, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK) rc = comm_all_gather_i64(ctx, d_s, d_r, W, ctx->s_main);
    if (rc == KRYST_OK && (hipMemcpyAsync(all.data(), d_r, sizeof(int64_t) * W * P, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    (void)hipFree(d_s); (void)hipFree(d_r);
    if (rc != KRYST_OK) return rc;                                   // (a failing collective fails on every rank)
    int64_t ok_all = 1;
    for (int p = 0; p < P; ++p) { if (all[(size_t)W * p] != 1 && getenv("KRYST_IPC_DEBUG")) fprintf(stderr, "[kryst] rank %d: rank %d could not export its buffer\n", me, p); ok_all = ok_all && all[(size_t)W * p] == 1; }
    peers.assign((size_t)P, nullptr);
    const size_t opened_before = opened.size();
    for (int p = 0; p < P && ok_all; ++p) {
        const int64_t* w = &all[(size_t)W * p];
        if (p == me) { peers[p] = mine; continue; }
        if (w[1] == (int64_t)getpid() && w[4] == (int64_t)process_nonce() && w[5] == (int64_t)host_hash()) {      // a rank of THIS process: same address space
            const int pdev = (int)w[2];
            if (pdev == ctx->device && !same_device_siblings) { ok_all = 0; break; }      // (the caller's kernels must not wait on a sibling that shares the device)
            if (pdev != ctx->device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, ctx->device, pdev) != hipSuccess || !can) { (void)hipGetLastError(); ok_all = 0; break; }
                const hipError_t e = hipDeviceEnablePeerAccess(pdev, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { ok_all = 0; }
                (void)hipGetLastError();
            }
            peers[p] = reinterpret_cast<void*>((uintptr_t)w[3]);
            if (sibling) *sibling = true;
            continue;
        }
        hipIpcMemHandle_t h; memcpy(&h, w + 6, 64);
        void* ptr = nullptr;
        { const hipError_t e = ipc_open_shared(&ptr, h); if (e != hipSuccess) { (void)hipGetLastError(); ok_all = 0; fprintf(stderr, "[kryst] rank %d: hipIpcOpenMemHandle of rank %d's buffer: %s\n", me, p, hipGetErrorString(e)); break; } }
        opened.push_back(ptr);
        peers[p] = ptr;
    }
    // everybody mapped everybody?
    int64_t *d_s2 = nullptr, *d_r2 = nullptr;
    std::vector<int64_t> all2((size_t)P, 0);
    if (hipMalloc(&d_s2, 8) != hipSuccess || hipMalloc(&d_r2, sizeof(int64_t) * P) != hipSuccess) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK && (hipMemcpyAsync(d_s2, &ok_all, 8, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    if (rc == KRYST_OK) rc = comm_all_gather_i64(ctx, d_s2, d_r2, 1, ctx->s_main);
    if (rc == KRYST_OK && (hipMemcpyAsync(all2.data(), d_r2, sizeof(int64_t) * P, hipMemcpyDeviceToHost, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;
    (void)hipFree(d_s2); (void)hipFree(d_r2);
    bool everybody = rc == KRYST_OK;
    for (int p = 0; p < P && everybody; ++p) everybody = all2[p] == 1;
    if (!everybody) {
        while (opened.size() > opened_before) { ipc_close_shared(opened.back()); opened.pop_back(); }
        (void)hipGetLastError();
        peers.assign((size_t)P, nullptr);
        if (rc != KRYST_OK) return rc;
        set_error("hipIpc: a rank could not allocate, export or map a peer's buffer; the RCCL path stays in use");
        return KRYST_UNSUPPORTED;
    }
    return KRYST_OK;
}

int32_t ipc_reduce_setup(kryst_ctx_t ctx) {
    if (ctx->ipc_on) return KRYST_OK;
    if (ctx->ipc_mine && ctx->ipc_failed) { set_error("scalar all-reduce through mailboxes: the test reduction failed on this context before; the RCCL path stays in use"); return KRYST_UNSUPPORTED; }
    if (ctx->ipc_mine) { ctx->ipc_on = true; return KRYST_OK; }      // set up before and switched off: the mailboxes are still mapped on every rank,
                                                                     // and every rank has counted the same epochs
    KR_ARG(ctx->comm, "ipc_reduce_setup: context has no communicator");
    const int P = ctx->nranks;
    KR_ARG(P <= 64, "ipc_reduce_setup: at most 64 ranks (one lane per peer)");
    const size_t cells = (size_t)2 * P * 16;
    // local: mailbox in fine-grained device memory (coherent for the peers' system-scope stores), zeroed; a rank that fails here still
    // takes part in the collective mapping below, which then fails on every rank alike
    // (2 MiB although 2 KB would do: small allocations of one process are carved out of one underlying buffer, and a peer that opens the handles of
    // two such pieces -- the mailboxes of two rank threads of one process -- gets "invalid device pointer" for the second, now and then)
    if (hipExtMallocWithFlags((void**)&ctx->ipc_mine, std::max<size_t>(sizeof(double) * cells, (size_t)2 << 20), hipDeviceMallocFinegrained) != hipSuccess ||
        hipMemsetAsync(ctx->ipc_mine, 0, sizeof(double) * cells, ctx->s_main) != hipSuccess ||
        hipMalloc(&ctx->d_ipc_peers, sizeof(double*) * P) != hipSuccess || hipMalloc(&ctx->d_ipc_epoch, 8) != hipSuccess ||
        hipMemsetAsync(ctx->d_ipc_epoch, 0, 8, ctx->s_main) != hipSuccess || hipStreamSynchronize(ctx->s_main) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(ctx->ipc_mine); ctx->ipc_mine = nullptr;
    }
    std::vector<void*> peers;
    // (the mailbox kernels of a solve are enqueued by every rank before any of them blocks: siblings on one device are fine here)
    int32_t rc = ipc_map_peers(ctx, ctx->ipc_mine, peers, ctx->ipc_opened, true);
    if (rc == KRYST_OK && (hipMemcpyAsync(ctx->d_ipc_peers, peers.data(), sizeof(double*) * P, hipMemcpyHostToDevice, ctx->s_main) != hipSuccess ||
                           hipStreamSynchronize(ctx->s_main) != hipSuccess)) rc = KRYST_ERR_HIP;      // (cannot fail on one rank alone in practice: an 8 P byte copy)
    if (rc != KRYST_OK) { ipc_reduce_destroy(ctx); return rc; }
    ctx->ipc_on = true;
    return ipc_reduce_selftest(ctx);                                 // (ipc_selftest.hip: one checked reduction; agreed verdict)
}

static int owner_of(const int64_t* row_offsets, int nranks, int64_t c) {
    // row_offsets ascending, nranks+1 entries; owner p has row_offsets[p] <= c < row_offsets[p+1]
    int lo = 0, hi = nranks;
    while (hi - lo > 1) { int mid = (lo + hi) / 2; if (row_offsets[mid] <= c) lo = mid; else hi = mid; }
    return lo;
}

void halo_recv_plan(int rank, int nranks, const int64_t* row_offsets, int64_t nloc, const int64_t* row_ptr,
                    const int64_t* col_global, HaloPlan* plan) {
    plan->nranks = nranks; plan->rank = rank;
    plan->row_lo = row_offsets[rank]; plan->row_hi = row_offsets[rank + 1];
    std::vector<std::vector<int64_t>> need(nranks);
    const int64_t nnz = row_ptr[nloc];
    for (int64_t k = 0; k < nnz; ++k) {
        const int64_t c = col_global[k];
        if (c >= plan->row_lo && c < plan->row_hi) continue;
        need[owner_of(row_offsets, nranks, c)].push_back(c);
    }
    plan->recv_counts.assign(nranks, 0); plan->recv_off.assign(nranks, 0);
    plan->recv_cols.clear();
    for (int p = 0; p < nranks; ++p) {
        auto& v = need[p];
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        plan->recv_off[p] = (int64_t)plan->recv_cols.size();
        plan->recv_counts[p] = (int64_t)v.size();
        plan->recv_cols.insert(plan->recv_cols.end(), v.begin(), v.end());
    }
    plan->total_recv = (int64_t)plan->recv_cols.size();
}

int64_t halo_slot(const HaloPlan& plan, const int64_t* row_offsets, int64_t c) {
    const int p = owner_of(row_offsets, plan.nranks, c);
    const int64_t* b = plan.recv_cols.data() + plan.recv_off[p];
    const int64_t* e = b + plan.recv_counts[p];
    const int64_t* it = std::lower_bound(b, e, c);
    return (it != e && *it == c) ? (int64_t)(it - plan.recv_cols.data()) : -1;
}

}  // namespace kr

using namespace kr;

extern "C" {

int32_t kryst_host_partition_rows(int64_t n, int32_t nranks, int64_t align, int64_t* row_offsets) {
    KR_ARG(n >= 0 && nranks >= 1 && align >= 1 && row_offsets, "partition_rows");
    const int64_t units = (n + align - 1) / align;       // e.g. grid planes
    for (int p = 0; p <= nranks; ++p) {
        int64_t u = units * p / nranks;                  // balanced contiguous blocks of whole units
        int64_t r = u * align;
        row_offsets[p] = r > n ? n : r;
    }
    row_offsets[nranks] = n;
    return KRYST_OK;
}

int64_t kryst_host_halo_recv_plan(int32_t rank, int32_t nranks, const int64_t* row_offsets, const int64_t* row_ptr,
                                  const int64_t* col_idx_global, int64_t* recv_counts, int64_t* recv_cols) {
    HaloPlan plan;
    const int64_t nloc = row_offsets[rank + 1] - row_offsets[rank];
    halo_recv_plan(rank, nranks, row_offsets, nloc, row_ptr, col_idx_global, &plan);
    if (recv_counts) for (int p = 0; p < nranks; ++p) recv_counts[p] = plan.recv_counts[p];
    if (recv_cols) memcpy(recv_cols, plan.recv_cols.data(), sizeof(int64_t) * (size_t)plan.total_recv);
    return plan.total_recv;
}

}  // extern "C"
