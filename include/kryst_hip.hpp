// kryst_hip.hpp -- header-only C++17 mirror of kryst's operator / preconditioner / solver interface over the C ABI
// of kryst_hip.h.  The reference is a compiled (Rust) crate whose toolchain is absent from the build image, so this is
// the compiled-language host side of the drop-in: same type names, constructor arguments, builder methods, public fields
// and error behaviour as the reference (paths relative to the kryst crate):
//
//   trait MatVec<V>            src/core/traits.rs:4-7          -> struct MatVec<V>           (pure virtual matvec)
//   trait Preconditioner<M,V>  src/preconditioner/mod.rs:8-13  -> struct Preconditioner<M,V> (apply / setup)
//   trait LinearSolver<M,V>    src/solver/mod.rs:30-52         -> struct LinearSolver<M,V>   (solve(a, pc, b, x) -> SolveStats)
//   CsrMatrix::from_csr        src/matrix/sparse.rs:28-46      -> HipCsrMatrix::from_csr
//   Jacobi / Ilu0 / Ilup / Chebyshev / apply_chebyshev          src/preconditioner/*.rs
//   CgSolver / PcgSolver / GmresSolver / FgmresSolver / BiCgStabSolver / CgsSolver / TfqmrSolver   src/solver/*.rs (new(..), with_norm, with_monitor, ...)
//   Convergence, SolveStats    src/utils/convergence.rs:4-14 ;  KError  src/error.rs:6-19 (thrown where Rust returns Err)
//
// V is std::vector<double> (the reference's Vec<f64>).  `Result<T, KError>` becomes "return T or throw KError";
// Rust's assert_eq! panics on length mismatches become KError{ArgumentError}.
#pragma once
#include <algorithm>
#include <array>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>
#include "kryst_hip.h"

namespace kryst {

using Vec = std::vector<double>;

struct KError : std::runtime_error {            // src/error.rs:6-19
    enum Kind { FactorError = 1, SolveError = 2, IndefiniteMatrix = 3, IndefinitePreconditioner = 4, ZeroPivot = 5,
                Unsupported = 6, HipError = 100, RcclError = 101, ArgumentError = 102, CsrError = 103, ContextBusy = 104 };
    int code;
    long long row;                              // KError::ZeroPivot(row), error.rs:15-16 (-1 for every other kind)
    explicit KError(int c) : std::runtime_error(std::string("kryst: ") + kind_name(c) + ": " + kryst_hip_last_error()), code(c),
                             row(c == KRYST_ZERO_PIVOT ? (long long)kryst_hip_last_error_row() : -1) {}
    static const char* kind_name(int c) {
        switch (c) { case 1: return "FactorError"; case 2: return "SolveError"; case 3: return "IndefiniteMatrix";
                     case 4: return "IndefinitePreconditioner"; case 5: return "ZeroPivot"; case 6: return "Unsupported";
                     case 100: return "HipError"; case 101: return "RcclError"; case 102: return "ArgumentError";
                     case 103: return "CsrError"; case 104: return "ContextBusy"; default: return "Error"; }
    }
};
inline void check(int32_t rc) { if (rc != KRYST_OK) throw KError(rc); }

template <class T> struct Convergence { T tol; size_t max_iters; };                          // convergence.rs:4-7
template <class T> struct SolveStats { size_t iterations; T final_residual; bool converged; };   // convergence.rs:10-14

template <class V> struct MatVec { virtual ~MatVec() = default; virtual void matvec(const V& x, V& y) const = 0; };
template <class M, class V> struct Preconditioner {
    virtual ~Preconditioner() = default;
    virtual void apply(const V& r, V& z) const = 0;          // Err(KError) -> throw
    virtual void setup(const M&) {}
    virtual kryst_pc_t device_handle() const { return nullptr; }   // additive hook
};
template <class M, class V> struct LinearSolver {
    virtual ~LinearSolver() = default;
    virtual SolveStats<double> solve(const M& a, const Preconditioner<M, V>* pc, const V& b, V& x) = 0;
};

// One GPU.  Replaces RayonComm / MpiComm (src/parallel).
class Context {
public:
    explicit Context(int device = 0) { check(kryst_ctx_create(device, &h_)); }
    Context(int device, int rank, int nranks, const void* unique_id128) { check(kryst_ctx_create_dist(device, rank, nranks, unique_id128, &h_)); }
    ~Context() { kryst_ctx_destroy(h_); }
    Context(const Context&) = delete; Context& operator=(const Context&) = delete;
    kryst_ctx_t handle() const { return h_; }
    // DistributedInnerProduct (core/wrappers.rs:134-156) inside the solvers: false = RCCL all-gather + rank-ordered fold (default),
    // true = hipIpc mailboxes (one launch, no collective, the same bits).  Collective.  Returns whether the mailbox path is in use.
    bool scalar_reduce_ipc(bool on) {
        int32_t active = 0;
        const int32_t rc = kryst_ctx_scalar_reduce(h_, on ? 1 : 0, &active);
        if (rc != KRYST_OK && rc != KRYST_UNSUPPORTED) check(rc);
        return active != 0;
    }
    static std::shared_ptr<Context> global() { static std::shared_ptr<Context> c = std::make_shared<Context>(0); return c; }
private:
    kryst_ctx_t h_ = nullptr;
};

// n x k device multivector, k in {2, 4, 8} (kryst_mvec_t): several right-hand sides at once; host data column-major, column j at j * ld
class MultiVec {
public:
    MultiVec(size_t n, size_t k, std::shared_ptr<Context> ctx = Context::global()) : ctx_(std::move(ctx)), n_(n), k_(k) {
        check(kryst_mvec_create(ctx_->handle(), (int64_t)n, (int32_t)k, &h_));
    }
    static MultiVec from_columns(const std::vector<Vec>& cols, std::shared_ptr<Context> ctx = Context::global()) {
        const size_t n = cols.empty() ? 0 : cols[0].size();
        MultiVec mv(n, cols.size(), std::move(ctx));
        Vec host(n * cols.size());
        for (size_t j = 0; j < cols.size(); ++j) {
            if (cols[j].size() != n) throw KError(KRYST_ERR_ARG);
            std::copy(cols[j].begin(), cols[j].end(), host.begin() + (long)(j * n));
        }
        mv.upload(host, n);
        return mv;
    }
    MultiVec(MultiVec&& o) noexcept : ctx_(std::move(o.ctx_)), h_(o.h_), n_(o.n_), k_(o.k_) { o.h_ = nullptr; }
    MultiVec(const MultiVec&) = delete; MultiVec& operator=(const MultiVec&) = delete;
    ~MultiVec() { if (h_) kryst_mvec_destroy(h_); }
    size_t nrows() const { return n_; }
    size_t ncols() const { return k_; }
    void upload(const Vec& host, size_t ld) { if (host.size() < (k_ ? (k_ - 1) * ld + n_ : 0)) throw KError(KRYST_ERR_ARG); check(kryst_mvec_upload(h_, host.data(), (int64_t)ld)); }
    void download(Vec& host, size_t ld) const { if (host.size() < (k_ ? (k_ - 1) * ld + n_ : 0)) throw KError(KRYST_ERR_ARG); check(kryst_mvec_download(h_, host.data(), (int64_t)ld)); }
    Vec column(size_t j) const {
        if (j >= k_) throw KError(KRYST_ERR_ARG);
        Vec host(n_ * k_), out(n_);
        download(host, n_);
        std::copy(host.begin() + (long)(j * n_), host.begin() + (long)((j + 1) * n_), out.begin());
        return out;
    }
    kryst_mvec_t handle() const { return h_; }
private:
    std::shared_ptr<Context> ctx_; kryst_mvec_t h_ = nullptr; size_t n_ = 0, k_ = 0;
};

// CsrMatrix<f64> resident in HBM; SparseMatrix::{nrows,ncols,spmv} (sparse.rs:4-11,49-68) and MatVec.
class HipCsrMatrix : public MatVec<Vec> {
public:
    static HipCsrMatrix from_csr(size_t nrows, size_t ncols, const std::vector<size_t>& row_ptr, const std::vector<size_t>& col_idx,
                                 const Vec& values, std::shared_ptr<Context> ctx = Context::global()) {
        static_assert(sizeof(size_t) == sizeof(uint64_t), "usize is 64-bit");
        if (row_ptr.size() != nrows + 1 || col_idx.size() != values.size()) throw KError(KRYST_ERR_ARG);
        kryst_csr_t h = nullptr;
        check(kryst_csr_create(ctx->handle(), (int64_t)nrows, (int64_t)ncols, reinterpret_cast<const uint64_t*>(row_ptr.data()),
                               reinterpret_cast<const uint64_t*>(col_idx.data()), values.data(), &h));
        return HipCsrMatrix(std::move(ctx), h, nrows, ncols);
    }
    static HipCsrMatrix stencil7(int N, int kind, std::shared_ptr<Context> ctx = Context::global()) {
        kryst_csr_t h = nullptr;
        check(kryst_csr_create_stencil7(ctx->handle(), N, kind, &h));
        const size_t n = (size_t)N * N * N;
        return HipCsrMatrix(std::move(ctx), h, n, n);
    }
    HipCsrMatrix(HipCsrMatrix&& o) noexcept : ctx_(std::move(o.ctx_)), h_(o.h_), nrows_(o.nrows_), ncols_(o.ncols_) { o.h_ = nullptr; }
    ~HipCsrMatrix() override { if (h_) kryst_csr_destroy(h_); }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    void spmv(const Vec& x, Vec& y) const {                   // sparse.rs:56-67 (asserts -> ArgumentError)
        check(kryst_spmv_host(h_, x.data(), (int64_t)x.size(), y.data(), (int64_t)y.size()));
    }
    void matvec(const Vec& x, Vec& y) const override { spmv(x, y); }
    void spmm(const MultiVec& x, MultiVec& y) const { check(kryst_spmm(h_, x.handle(), y.handle())); }      // column j = spmv on column j
    // the kernel spmm and solve_many take for k columns under the current KRYST_SPMM_FORM: "plain" or "dia" (kryst_spmm_kernel)
    std::string spmm_kernel(int k) const {
        int32_t kernel = 0;
        check(kryst_spmm_kernel(h_, (int32_t)k, &kernel));
        return kernel == 1 ? "dia" : "plain";
    }
    // MatTransVec::mattransvec: y <- A^T x through kryst_spmv_transpose (A^T built on the first call, cached on the operator)
    void mattransvec(const Vec& x, Vec& y) const {
        if (x.size() != nrows_ || y.size() != ncols_) throw KError(KRYST_ERR_ARG);
        kryst_vec_t xv = nullptr, yv = nullptr;
        int32_t rc = kryst_vec_create(ctx_->handle(), (int64_t)x.size(), &xv);
        if (rc == 0) rc = kryst_vec_create(ctx_->handle(), (int64_t)y.size(), &yv);
        if (rc == 0) rc = kryst_vec_upload(xv, x.data(), (int64_t)x.size());
        if (rc == 0) rc = kryst_spmv_transpose(h_, xv, yv);
        if (rc == 0) rc = kryst_vec_download(yv, y.data(), (int64_t)y.size());
        if (xv) kryst_vec_destroy(xv);
        if (yv) kryst_vec_destroy(yv);
        check(rc);
    }
    // The halo exchange of a row-partitioned operator (the neighbour exchange src/parallel/mpi_comm.rs:133-143 leaves as a TODO): false =
    // grouped ncclSend / ncclRecv (default), true = direct peer stores into hipIpc-mapped landing buffers (no collective launch, the same
    // bits).  Collective.  Returns whether the peer-store path is in use (it is not when a rank cannot map a peer's buffer).
    bool halo_peer_stores(bool on) {
        int32_t active = 0;
        const int32_t rc = kryst_csr_halo_mode(h_, on ? 1 : 0, &active);
        if (rc != KRYST_OK && rc != KRYST_UNSUPPORTED) check(rc);
        return active != 0;
    }
    kryst_csr_t handle() const { return h_; }
    const std::shared_ptr<Context>& context() const { return ctx_; }
private:
    HipCsrMatrix(std::shared_ptr<Context> c, kryst_csr_t h, size_t nr, size_t nc) : ctx_(std::move(c)), h_(h), nrows_(nr), ncols_(nc) {}
    std::shared_ptr<Context> ctx_; kryst_csr_t h_; size_t nrows_, ncols_;
};

// ---- preconditioners --------------------------------------------------------------------------------------------
class DevicePc : public Preconditioner<HipCsrMatrix, Vec> {
public:
    DevicePc() = default;
    // move-only, like every other handle owner here: a copy would hand the same kryst_pc_t to kryst_pc_destroy twice
    DevicePc(const DevicePc&) = delete; DevicePc& operator=(const DevicePc&) = delete;
    DevicePc(DevicePc&& o) noexcept : h_(o.h_), ctx_(o.ctx_) { o.h_ = nullptr; o.ctx_ = nullptr; }
    DevicePc& operator=(DevicePc&& o) noexcept {
        if (this != &o) { if (h_) kryst_pc_destroy(h_); h_ = o.h_; ctx_ = o.ctx_; o.h_ = nullptr; o.ctx_ = nullptr; }
        return *this;
    }
    ~DevicePc() override { if (h_) kryst_pc_destroy(h_); }
    void apply(const Vec& r, Vec& z) const override {
        if (!h_ || !ctx_) throw KError(KRYST_SOLVE_ERROR);
        if (r.size() != z.size()) throw KError(KRYST_ERR_ARG);
        kryst_vec_t rv = nullptr, zv = nullptr;
        check(kryst_vec_create(ctx_, (int64_t)r.size(), &rv));
        int32_t rc = kryst_vec_create(ctx_, (int64_t)z.size(), &zv);
        if (rc == 0) rc = kryst_vec_upload(rv, r.data(), (int64_t)r.size());
        if (rc == 0) rc = kryst_pc_apply(h_, rv, zv);
        if (rc == 0) rc = kryst_vec_download(zv, z.data(), (int64_t)z.size());
        kryst_vec_destroy(rv); kryst_vec_destroy(zv);
        check(rc);
    }
    kryst_pc_t device_handle() const override { return h_; }
protected:
    void reset(kryst_pc_t h, kryst_ctx_t c) { if (h_) kryst_pc_destroy(h_); h_ = h; ctx_ = c; }
    kryst_pc_t h_ = nullptr; kryst_ctx_t ctx_ = nullptr;
};
struct Jacobi : DevicePc {                                   // jacobi.rs:26-95
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_jacobi(a.handle(), &h)); reset(h, a.context()->handle()); }
};
struct Ilu0 : DevicePc {                                     // ilu.rs:32-122 (as written)
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_ilu0(a.handle(), KRYST_ILU_KRYST_COMPAT, &h)); reset(h, a.context()->handle()); }
};
struct Ilup : DevicePc {                                     // ilup.rs:54-167 (level-of-fill p, as written)
    explicit Ilup(size_t fill = 0) : fill(fill) {}
    size_t fill;
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_ilup(a.handle(), (int32_t)fill, &h)); reset(h, a.context()->handle()); }
};
struct Ilut : DevicePc {                                     // ilut.rs:55-150 (as written)
    Ilut(size_t fill, double droptol) : fill(fill), droptol(droptol) {}
    size_t fill; double droptol;
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_ilut(a.handle(), (int32_t)fill, droptol, &h)); reset(h, a.context()->handle()); }
};
struct TrueIlu0 : DevicePc {                                 // extension
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_ilu0(a.handle(), KRYST_ILU_TRUE_ILU0, &h)); reset(h, a.context()->handle()); }
};
struct IdentityPC : DevicePc {                               // pcg.rs:245-251
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_identity(a.context()->handle(), &h)); reset(h, a.context()->handle()); }
};
// ApproxInv with GIVEN inverse rows (ApproxInv::inv_rows, approxinv.rs:66): apply (approxinv.rs:268-298) is z = M r on the device.
// ApproxInv::setup (least squares through faer's QR) stays with the reference; setup() here only checks the size.
struct ApproxInv : DevicePc {
    explicit ApproxInv(const std::vector<std::vector<std::pair<size_t, double>>>& inv_rows, std::shared_ptr<Context> ctx = Context::global())
        : m_(build(inv_rows, std::move(ctx))) {
        kryst_pc_t h = nullptr; check(kryst_pc_approx_inverse(m_.handle(), &h)); reset(h, m_.context()->handle());
    }
    void setup(const HipCsrMatrix& a) override { if (a.nrows() != m_.nrows()) throw KError(KRYST_ERR_ARG); }
private:
    static HipCsrMatrix build(const std::vector<std::vector<std::pair<size_t, double>>>& rows, std::shared_ptr<Context> ctx) {
        std::vector<size_t> rp(rows.size() + 1, 0), ci; Vec va;
        for (size_t i = 0; i < rows.size(); ++i) { for (auto& e : rows[i]) { ci.push_back(e.first); va.push_back(e.second); } rp[i + 1] = ci.size(); }
        return HipCsrMatrix::from_csr(rows.size(), rows.size(), rp, ci, va, std::move(ctx));
    }
    HipCsrMatrix m_;
};
// BlockJacobi (block_jacobi.rs:39-106) as a device preconditioner on the CSR operator: `blocks` are index sets in the given order (the last
// block that contains a row decides it, rows in no block give 0), or contiguous blocks of `bsize` rows (uniform, an extension).  Labelled
// deviations (kryst_hip.h, kryst_pc_block_jacobi): explicit Gauss-Jordan inverses, sorted index sets, errors instead of non-finite z.
struct BlockJacobi : DevicePc {
    explicit BlockJacobi(std::vector<std::vector<size_t>> blocks) : blocks(std::move(blocks)) {}
    static BlockJacobi uniform(size_t bsize) { BlockJacobi b({}); b.bsize = bsize; return b; }
    std::vector<std::vector<size_t>> blocks; size_t bsize = 0;
    void setup(const HipCsrMatrix& a) override {
        kryst_pc_t h = nullptr;
        if (bsize > 0) {
            check(kryst_pc_block_jacobi_uniform(a.handle(), (int32_t)std::min<size_t>(bsize, INT32_MAX), &h));
        } else {
            std::vector<int64_t> ptr(1, 0), idx;
            for (auto& g : blocks) { for (size_t i : g) idx.push_back((int64_t)i); ptr.push_back((int64_t)idx.size()); }
            check(kryst_pc_block_jacobi(a.handle(), ptr.data(), idx.data(), (int64_t)blocks.size(), &h));
        }
        reset(h, a.context()->handle());
    }
};
// AdditiveSchwarz::new(overlap, subdomains) + setup + apply (asm.rs:34-119) with the direct solve as the inner solver (kryst_pc_asm): z = 0,
// then every subdomain in ascending order adds its product.  Empty `subdomains`: `nparts` uniform parts (the reference's capacity(); 0 gives
// one part).  The variant selects the labelled extensions: growth by `overlap` layers (Grown) and RAS (Restricted); AsWritten ignores
// `overlap`, as the reference does.  PC{AdditiveSchwarzKind} keeps throwing KError{Unsupported}; construct AdditiveSchwarz directly.
struct AdditiveSchwarz : DevicePc {
    enum Variant { AsWritten = KRYST_ASM_AS_WRITTEN, Grown = KRYST_ASM_GROWN, Restricted = KRYST_ASM_RESTRICTED };
    AdditiveSchwarz(size_t overlap = 0, std::vector<std::vector<size_t>> subdomains = {}, size_t nparts = 0, Variant variant = AsWritten)
        : overlap(overlap), subdomains(std::move(subdomains)), nparts(nparts), variant(variant) {}
    size_t overlap; std::vector<std::vector<size_t>> subdomains; size_t nparts; Variant variant;
    // labelled extension (kryst_pc_asm_ilu): ILU(0) subdomain solves in place of the dense inverses, subdomains of up to
    // KRYST_ASM_ILU_MAX_ROWS rows; sub_mode KRYST_ILU_TRUE_ILU0 or KRYST_ILU_ILUP0.  Negative (the default): the direct solve.
    int32_t sub_mode = -1;
    AdditiveSchwarz& with_sub_ilu(int32_t mode = KRYST_ILU_TRUE_ILU0) { sub_mode = mode; return *this; }
    void setup(const HipCsrMatrix& a) override {
        kryst_pc_t h = nullptr;
        const int32_t ov = (int32_t)std::min<size_t>(overlap, INT32_MAX);
        std::vector<int64_t> ptr(1, 0), idx;
        for (auto& g : subdomains) { for (size_t i : g) idx.push_back((int64_t)i); ptr.push_back((int64_t)idx.size()); }
        if (subdomains.empty()) {
            if (sub_mode >= 0) check(kryst_pc_asm_ilu_uniform(a.handle(), (int64_t)nparts, ov, (int32_t)variant, sub_mode, &h));
            else check(kryst_pc_asm_uniform(a.handle(), (int64_t)nparts, ov, (int32_t)variant, &h));
        } else if (sub_mode >= 0) {
            check(kryst_pc_asm_ilu(a.handle(), ptr.data(), idx.data(), (int64_t)subdomains.size(), ov, (int32_t)variant, sub_mode, &h));
        } else {
            check(kryst_pc_asm(a.handle(), ptr.data(), idx.data(), (int64_t)subdomains.size(), ov, (int32_t)variant, &h));
        }
        reset(h, a.context()->handle());
    }
};
// MatSorType (sor.rs:32-44), the reference's bit values, and Sor::new(omega, its, lits, sym, fshift) + setup + apply (sor.rs:71-170) as a
// device preconditioner (kryst_pc_sor): the sweeps exactly as written; `lits` and the LOCAL_* bits are stored and not used.  The parameters
// are read by setup().  `colors` (labelled extension; PC::Multicolor has no implementation in the reference): non-empty, one colour per
// row -- the same sweeps in the order (colour, row).  PC{SsorKind} / PC{MulticolorKind} keep throwing KError{Unsupported}; construct Sor.
namespace MatSorType {
enum : uint32_t { ZERO_INITIAL_GUESS = KRYST_SOR_ZERO_INITIAL_GUESS, APPLY_LOWER = KRYST_SOR_APPLY_LOWER, APPLY_UPPER = KRYST_SOR_APPLY_UPPER,
                  SYMMETRIC_SWEEP = KRYST_SOR_SYMMETRIC_SWEEP, LOCAL_FORWARD_SWEEP = KRYST_SOR_LOCAL_FORWARD_SWEEP,
                  LOCAL_BACKWARD_SWEEP = KRYST_SOR_LOCAL_BACKWARD_SWEEP, LOCAL_SYMMETRIC_SWEEP = KRYST_SOR_LOCAL_SYMMETRIC_SWEEP,
                  EISENSTAT = KRYST_SOR_EISENSTAT };
}
struct Sor : DevicePc {
    Sor(double omega, size_t its, size_t lits, uint32_t sym, double fshift) : omega_(omega), its_(its), lits_(lits), sym_(sym), fshift_(fshift) {}
    void set_omega(double v) { omega_ = v; }   double omega() const { return omega_; }
    void set_its(size_t v) { its_ = v; }       size_t its() const { return its_; }
    void set_lits(size_t v) { lits_ = v; }     size_t lits() const { return lits_; }
    void set_sym(uint32_t v) { sym_ = v; }     uint32_t sym() const { return sym_; }
    void set_fshift(double v) { fshift_ = v; } double fshift() const { return fshift_; }
    Sor& with_colors(std::vector<size_t> c) { colors = std::move(c); return *this; }
    std::vector<size_t> colors;
    void setup(const HipCsrMatrix& a) override {
        kryst_pc_t h = nullptr;
        std::vector<int32_t> c;
        if (!colors.empty()) {
            if (colors.size() != a.nrows()) throw KError(KRYST_ERR_ARG);
            for (size_t v : colors) { if (v > (size_t)INT32_MAX) throw KError(KRYST_ERR_ARG); c.push_back((int32_t)v); }
        }
        check(kryst_pc_sor(a.handle(), omega_, (int64_t)its_, (int64_t)lits_, sym_, fshift_, c.empty() ? nullptr : c.data(), &h));
        reset(h, a.context()->handle());
    }
private:
    double omega_; size_t its_, lits_; uint32_t sym_; double fshift_;
};
// AMG::new(a, max_levels, threshold) (amg.rs:73-118) as written, set up on the host and applied on the device (kryst_pc_amg): one undamped
// Jacobi sweep before and after the coarse correction, the finest level from the incoming z, CG on the coarsest level.  PC{AMGKind} keeps
// throwing KError{Unsupported} (the mirror's tests pin that); construct Amg directly.
struct Amg : DevicePc {
    Amg(size_t max_levels = 10, double threshold = 0.1) : max_levels(max_levels), threshold(threshold) {}
    size_t max_levels; double threshold;
    void setup(const HipCsrMatrix& a) override {
        kryst_pc_t h = nullptr;
        check(kryst_pc_amg(a.handle(), (int32_t)std::min<size_t>(max_levels, INT32_MAX), threshold, KRYST_AMG_AS_WRITTEN, 1, 1, &h));
        reset(h, a.context()->handle());
    }
};
// SparsityPattern (preconditioner/mod.rs) for the SPAI set-up: Manual(pat) (pat[j] = the rows of column j of M, n = pat.size()), Auto (as
// written: the set-up throws KError{Unsupported}, approxinv.rs:127-133), Operator (extension: the stored columns of row j of A).
struct SparsityPattern {
    enum Kind { ManualKind = KRYST_SPAI_MANUAL, AutoKind = KRYST_SPAI_AUTO, OperatorKind = KRYST_SPAI_OPERATOR };
    Kind kind = AutoKind; std::vector<std::vector<size_t>> pat;
    static SparsityPattern Manual(std::vector<std::vector<size_t>> pat) { SparsityPattern p; p.kind = ManualKind; p.pat = std::move(pat); return p; }
    static SparsityPattern Auto() { return SparsityPattern{}; }
    static SparsityPattern Operator() { SparsityPattern p; p.kind = OperatorKind; return p; }
};
// ApproxInv::new(pattern, tol, max_iter, ...) + setup(a) (approxinv.rs:76-264) on the device: the SPAI set-up of kryst_pc_spai (labelled
// deviations there: sorted patterns, reduced least squares by Householder QR, errors instead of panics); apply is ApproxInv's z = M r.
// The tuning fields are kept and unused, as in the reference.  export(): M (inv_rows) as CSR.
struct Spai : DevicePc {
    Spai(SparsityPattern pattern, double tol, size_t max_iter = 0, size_t nbsteps = 0, size_t max_size = 0, size_t max_new = 0,
         size_t block_size = 0, size_t cache_size = 0, bool verbose = false, bool sp = false)
        : pattern(std::move(pattern)), tol(tol), max_iter(max_iter), nbsteps(nbsteps), max_size(max_size), max_new(max_new),
          block_size(block_size), cache_size(cache_size), verbose(verbose), sp(sp) {}
    SparsityPattern pattern; double tol; size_t max_iter, nbsteps, max_size, max_new, block_size, cache_size; bool verbose, sp;
    void setup(const HipCsrMatrix& a) override {
        kryst_pc_t h = nullptr;
        std::vector<int64_t> ptr(1, 0), idx;
        for (auto& c : pattern.pat) { for (size_t i : c) idx.push_back((int64_t)i); ptr.push_back((int64_t)idx.size()); }
        check(kryst_pc_spai(a.handle(), (int32_t)pattern.kind, ptr.data(), idx.data(), (int64_t)pattern.pat.size(), tol, &h));
        reset(h, a.context()->handle());
        n_ = a.nrows();
    }
    void export_csr(std::vector<int64_t>& row_ptr, std::vector<int32_t>& col, Vec& val) const {
        int64_t nnz = 0;
        check(kryst_pc_spai_export(h_, &nnz, nullptr, nullptr, nullptr));
        row_ptr.assign(n_ + 1, 0); col.assign((size_t)nnz, 0); val.assign((size_t)nnz, 0.0);
        check(kryst_pc_spai_export(h_, &nnz, row_ptr.data(), col.data(), val.data()));
    }
private:
    size_t n_ = 0;
};
struct Chebyshev : DevicePc {                                // chebyshev.rs:35-70: the trait apply is a stub returning Err
    size_t degree; std::optional<double> lambda_min, lambda_max;
    Chebyshev(size_t degree, std::optional<double> lmin, std::optional<double> lmax) : degree(degree), lambda_min(lmin), lambda_max(lmax) {}
    void setup(const HipCsrMatrix& a) override { kryst_pc_t h = nullptr; check(kryst_pc_chebyshev_stub(a.context()->handle(), (int32_t)degree, &h)); reset(h, a.context()->handle()); }
};
// EXTENSION (kryst_pc_chebyshev_poly, kryst_spectrum_estimate; nothing in the reference corresponds -- Chebyshev above is its stub): the
// Chebyshev polynomial preconditioner z = p_degree(W A) W r with W = Jacobi's inverse diagonal (jacobi = true) or nothing.
struct SpectrumEstimate { std::vector<double> alpha, beta; double theta_min = 0.0, theta_max = 0.0, gershgorin = 0.0; };
// up to `steps` (1..64) Lanczos steps on W^1/2 A W^1/2 and the Gershgorin bound of W A; single-rank operators (else KError(KRYST_UNSUPPORTED))
inline SpectrumEstimate estimate_spectrum(const HipCsrMatrix& a, bool jacobi = true, int steps = 10, uint64_t seed = 0x5EED) {
    SpectrumEstimate e;
    e.alpha.assign((size_t)(steps > 0 ? steps : 1), 0.0); e.beta = e.alpha;
    int32_t done = 0;
    check(kryst_spectrum_estimate(a.handle(), jacobi ? KRYST_CHEB_SCALE_JACOBI : KRYST_CHEB_SCALE_NONE, (int32_t)steps, seed, e.alpha.data(),
                                  e.beta.data(), &done, &e.theta_min, &e.theta_max, &e.gershgorin));
    e.alpha.resize((size_t)done); e.beta.resize((size_t)done);
    return e;
}
struct ChebyshevPoly : DevicePc {
    size_t degree; std::optional<double> lambda_min, lambda_max; bool jacobi; int steps; double ratio, safety; uint64_t seed;
    explicit ChebyshevPoly(size_t degree, std::optional<double> lmin = std::nullopt, std::optional<double> lmax = std::nullopt, bool jacobi = true,
                           int steps = 10, double ratio = 30.0, double safety = 1.1, uint64_t seed = 0x5EED)
        : degree(degree), lambda_min(lmin), lambda_max(lmax), jacobi(jacobi), steps(steps), ratio(ratio), safety(safety), seed(seed) {}
    // a bound that is not given is estimated: lambda_max = min(safety * theta_max, gershgorin), lambda_min = lambda_max / ratio
    void setup(const HipCsrMatrix& a) override {
        std::optional<double> lo = lambda_min, hi = lambda_max;
        if (!lo || !hi) {
            const SpectrumEstimate e = estimate_spectrum(a, jacobi, steps, seed);
            if (!hi) hi = std::min(safety * e.theta_max, e.gershgorin);
            if (!lo) lo = *hi / ratio;
        }
        kryst_pc_t h = nullptr;
        check(kryst_pc_chebyshev_poly(a.handle(), (int32_t)degree, jacobi ? KRYST_CHEB_SCALE_JACOBI : KRYST_CHEB_SCALE_NONE, *lo, *hi, &h));
        reset(h, a.context()->handle());
    }
    bool fused() const { int32_t f = 0; check(kryst_pc_chebyshev_poly_info(h_, nullptr, nullptr, nullptr, nullptr, &f)); return f != 0; }
    std::pair<double, double> bounds() const { double lo = 0, hi = 0; check(kryst_pc_chebyshev_poly_info(h_, nullptr, nullptr, &lo, &hi, nullptr)); return {lo, hi}; }
};
inline void apply_chebyshev(const HipCsrMatrix& a, const Vec& r, Vec& z, double alpha, double beta, size_t m) {   // chebyshev.rs:83-140
    kryst_ctx_t c = a.context()->handle();
    kryst_vec_t rv = nullptr, zv = nullptr;
    check(kryst_vec_create(c, (int64_t)r.size(), &rv));
    int32_t rc = kryst_vec_create(c, (int64_t)z.size(), &zv);
    if (rc == 0) rc = kryst_vec_upload(rv, r.data(), (int64_t)r.size());
    if (rc == 0) rc = kryst_apply_chebyshev(a.handle(), rv, zv, alpha, beta, (int64_t)m);
    if (rc == 0) rc = kryst_vec_download(zv, z.data(), (int64_t)z.size());
    kryst_vec_destroy(rv); kryst_vec_destroy(zv);
    check(rc);
}

// ---- solvers -------------------------------------------------------------------------------------------------------
enum class CgNormType { Preconditioned = 0, Unpreconditioned = 1, Natural = 2, None = 3 };      // cg.rs:35
enum class Preconditioning { None = 0, Left = 1, Right = 2, LeftTextbook = 3 };                  // gmres.rs:28-32; LeftTextbook: labelled extension (kryst_hip.h: precond_side 3)

class SolverBase : public LinearSolver<HipCsrMatrix, Vec> {
public:
    Convergence<double> conv;
    CgNormType norm_type = CgNormType::Unpreconditioned;
    bool single_reduction = false;
    std::optional<double> radius, obj_target;
    std::function<void(size_t, double)> monitor;     // with_monitor (cg.rs:84-88): fired live, in order, on the calling thread
    std::vector<double> residual_history;
    int check_every = 0;                             // iterations between two rounds of monitor callbacks (0: the library's 8)
    void clear_history() { residual_history.clear(); }
    SolveStats<double> solve(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const Vec& b, Vec& x) override {
        if (b.size() != x.size()) throw KError(KRYST_ERR_ARG);
        kryst_params_t p{};
        p.tol = conv.tol; p.max_iters = (int64_t)conv.max_iters; p.restart = restart_; p.precond_side = side_;
        p.norm_type = (int)norm_type; p.single_reduction = single_reduction;
        p.has_radius = radius.has_value(); p.radius = radius.value_or(0.0);
        p.has_obj_target = obj_target.has_value(); p.obj_target = obj_target.value_or(0.0);
        p.check_every = check_every;
        kryst_stats_t st{};
        std::vector<double> hist(std::min<size_t>((size_t)hist_per_iter_ * conv.max_iters + (size_t)(restart_ > 0 ? restart_ : 1) + 8,
                                                  ((size_t)1 << 22) + 8));      // the library records at most 2^22 entries
        int64_t len = 0;
        const int32_t rc = call(b.data(), x.data(), (int64_t)b.size(), a.handle(), pc ? pc->device_handle() : nullptr, &p, &st,
                                hist.data(), (int64_t)hist.size(), &len, monitor ? &SolverBase::trampoline : nullptr, this);
        const size_t k = (size_t)std::min<int64_t>(len, (int64_t)hist.size());
        residual_history.insert(residual_history.end(), hist.begin(), hist.begin() + (long)k);
        check(rc);
        return SolveStats<double>{(size_t)st.iterations, st.final_residual, st.converged != 0};
    }
    // several right-hand sides at once (CG and PCG): column j gets what solve() gives for column j, bit for bit.  Returns the columns'
    // KError codes (KRYST_OK = 0); stats and residual_histories are per column; X(:, j) is written only where the code is KRYST_OK.
    std::vector<std::vector<double>> residual_histories;
    std::vector<int32_t> solve_many(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const MultiVec& b, MultiVec& x,
                                    std::vector<SolveStats<double>>& stats) {
        const size_t k = b.ncols();
        kryst_params_t p{};
        p.tol = conv.tol; p.max_iters = (int64_t)conv.max_iters; p.norm_type = (int)norm_type; p.single_reduction = single_reduction;
        p.has_radius = radius.has_value(); p.radius = radius.value_or(0.0);
        p.has_obj_target = obj_target.has_value(); p.obj_target = obj_target.value_or(0.0);
        p.check_every = check_every;
        std::vector<kryst_stats_t> st(k);
        std::vector<int32_t> code(k, 0);
        const size_t cap = std::min<size_t>(conv.max_iters + 8, ((size_t)1 << 19) + 8);
        std::vector<double> hist(k * cap);
        std::vector<int64_t> len(k, 0);
        check(call_many(b.handle(), x.handle(), a.handle(), pc ? pc->device_handle() : nullptr, &p, st.data(), code.data(), hist.data(), (int64_t)cap,
                        len.data()));
        stats.clear(); residual_histories.clear();
        for (size_t j = 0; j < k; ++j) {
            stats.push_back(SolveStats<double>{(size_t)st[j].iterations, st[j].final_residual, st[j].converged != 0});
            const size_t m = (size_t)std::min<int64_t>(len[j], (int64_t)cap);
            residual_histories.emplace_back(hist.begin() + (long)(j * cap), hist.begin() + (long)(j * cap + m));
        }
        return code;
    }
protected:
    SolverBase(double tol, size_t max_iters) : conv{tol, max_iters} {}
    virtual int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) = 0;
    virtual int32_t call_many(kryst_mvec_t, kryst_mvec_t, kryst_csr_t, kryst_pc_t, const kryst_params_t*, kryst_stats_t*, int32_t*, double*, int64_t,
                              int64_t*) { return KRYST_UNSUPPORTED; }       // CG and PCG override it
    int restart_ = 0, side_ = 1, hist_per_iter_ = 1;
private:
    static void trampoline(int64_t it, double res, void* user) { static_cast<SolverBase*>(user)->monitor((size_t)it, res); }
};
#define KRYST_FWD a, pc, params, stats, hist, hist_cap, hist_len, monitor, user

struct CgSolver : SolverBase {                               // cg.rs:40-93
    CgSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
    static CgSolver create(double tol, size_t max_iters) { return CgSolver(tol, max_iters); }     // CgSolver::new
    CgSolver& with_norm(CgNormType t) { norm_type = t; return *this; }
    CgSolver& with_single_reduction(bool f) { single_reduction = f; return *this; }
    CgSolver& with_radius(double r) { radius = r; return *this; }
    CgSolver& with_obj_target(double o) { obj_target = o; return *this; }
    CgSolver& with_monitor(std::function<void(size_t, double)> f) { monitor = std::move(f); return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_cg_solve(b, x, n, KRYST_FWD); }
    int32_t call_many(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats, int32_t* status,
                      double* hist, int64_t hist_cap, int64_t* hist_len) override {
        return kryst_cg_solve_multi_dev(b, x, a, pc, params, stats, status, hist, hist_cap, hist_len);
    }
};
struct PcgSolver : SolverBase {                              // pcg.rs:31-91
    PcgSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
    PcgSolver& with_norm(CgNormType t) { norm_type = t; return *this; }
    PcgSolver& with_single_reduction(bool f) { single_reduction = f; return *this; }
    PcgSolver& with_monitor(std::function<void(size_t, double)> f) { monitor = std::move(f); return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_pcg_solve(b, x, n, KRYST_FWD); }
    int32_t call_many(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats, int32_t* status,
                      double* hist, int64_t hist_cap, int64_t* hist_len) override {
        return kryst_pcg_solve_multi_dev(b, x, a, pc, params, stats, status, hist, hist_cap, hist_len);
    }
};
// Block CG (an extension: kryst_bcg_solve_multi_dev): one Krylov space for the columns of a multivector.  solve_block returns the block's code per
// column (one code for all of them) and fills stats and residual_histories like solve_many; X is written only when the code is KRYST_OK.  A single
// right-hand side has no block form: solve() throws KRYST_UNSUPPORTED.  For right-hand sides that may be dependent use CgSolver / PcgSolver::solve_many.
struct BlockCgSolver : SolverBase {
    BlockCgSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
    std::vector<int32_t> solve_block(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const MultiVec& b, MultiVec& x,
                                     std::vector<SolveStats<double>>& stats) { return solve_many(a, pc, b, x, stats); }
protected:
    int32_t call(const double*, double*, int64_t, KRYST_SOLVE_ARGS) override {
        (void)a; (void)pc; (void)params; (void)stats; (void)hist; (void)hist_cap; (void)hist_len; (void)monitor; (void)user;
        return KRYST_UNSUPPORTED;
    }
    int32_t call_many(kryst_mvec_t b, kryst_mvec_t x, kryst_csr_t a, kryst_pc_t pc, const kryst_params_t* params, kryst_stats_t* stats, int32_t* status,
                      double* hist, int64_t hist_cap, int64_t* hist_len) override {
        return kryst_bcg_solve_multi_dev(b, x, a, pc, params, stats, status, hist, hist_cap, hist_len);
    }
};
struct GmresSolver : SolverBase {                            // gmres.rs:38-60
    size_t restart; Preconditioning preconditioning = Preconditioning::Left;
    GmresSolver(size_t restart, double tol, size_t max_iters) : SolverBase(tol, max_iters), restart(restart) { restart_ = (int)restart; }
    GmresSolver& with_preconditioning(Preconditioning m) { preconditioning = m; side_ = (int)m; return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_gmres_solve(b, x, n, KRYST_FWD); }
};
enum class Orthog { Classical = 0, Modified = 1 };           // fgmres.rs:26-31
struct FgmresSolver : SolverBase {                           // fgmres.rs:33-101; solve_flex :114-340
    size_t restart; Orthog orthog = Orthog::Classical; double haptol = 1e-12; bool preallocate = false; size_t delta_allocate = 10;
    FgmresSolver(double tol, size_t max_iters, size_t restart) : SolverBase(tol, max_iters), restart(restart) { restart_ = (int)restart; }
    FgmresSolver& with_orthog(Orthog o) { orthog = o; return *this; }
    FgmresSolver& with_preallocate(bool f) { preallocate = f; return *this; }
    FgmresSolver& with_delta_allocate(size_t d) { delta_allocate = d; return *this; }
    FgmresSolver& with_haptol(double h) { haptol = h; return *this; }
    // the FlexiblePreconditioner (preconditioner/mod.rs:16-19) is a device preconditioner object
    SolveStats<double> solve_flex(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const Vec& b, Vec& x) { return solve(a, pc, b, x); }
    FgmresSolver& with_monitor(std::function<void(size_t, double)> f) { monitor = std::move(f); return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override {
        return kryst_fgmres_solve(b, x, n, (int32_t)orthog, haptol, preallocate ? 1 : 0, KRYST_FWD);
    }
};
struct BiCgStabSolver : SolverBase {                         // bicgstab.rs:36-48
    BiCgStabSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_bicgstab_solve(b, x, n, KRYST_FWD); }
};
struct CgsSolver : SolverBase {                              // cgs.rs:21-35
    CgsSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_cgs_solve(b, x, n, KRYST_FWD); }
};
struct TfqmrSolver : SolverBase {                            // tfqmr.rs:30-40
    TfqmrSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) { hist_per_iter_ = 2; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_tfqmr_solve(b, x, n, KRYST_FWD); }
};
// MINRES / CGNR: the as-written forms (host slices, like every solver here) and the labelled textbook extensions, which exist for
// device vectors only -- the slices go up and down around the _dev entry point
struct TextbookSolverBase : SolverBase {
    bool textbook = false;
    SolveStats<double> solve(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const Vec& b, Vec& x) override {
        ctx_h_ = a.context() ? a.context()->handle() : nullptr;
        return SolverBase::solve(a, pc, b, x);
    }
protected:
    using SolverBase::SolverBase;
    kryst_ctx_t ctx_h_ = nullptr;
    typedef int32_t (*DevFn)(kryst_vec_t, kryst_vec_t, KRYST_SOLVE_ARGS);
    int32_t call_dev(DevFn f, const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) {
        kryst_vec_t bv = nullptr, xv = nullptr;
        int32_t rc = kryst_vec_create(ctx_h_, n, &bv);
        if (rc == 0) rc = kryst_vec_create(ctx_h_, n, &xv);
        if (rc == 0) rc = kryst_vec_upload(bv, b, n);
        if (rc == 0) rc = kryst_vec_upload(xv, x, n);
        if (rc == 0) rc = f(bv, xv, KRYST_FWD);
        if (rc == 0) rc = kryst_vec_download(xv, x, n);
        if (bv) kryst_vec_destroy(bv);
        if (xv) kryst_vec_destroy(xv);
        return rc;
    }
};
struct MinresSolver : TextbookSolverBase {                    // minres.rs:60-219 as written; with_textbook(): Paige-Saunders MINRES (extension)
    MinresSolver(double tol, size_t max_iters) : TextbookSolverBase(tol, max_iters) {}
    MinresSolver& with_textbook() { textbook = true; return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override {
        return textbook ? call_dev(kryst_minres_textbook_solve_dev, b, x, n, KRYST_FWD) : kryst_minres_solve(b, x, n, KRYST_FWD);
    }
};
struct PcaGmresSolver : TextbookSolverBase {                  // pca_gmres.rs:37-76, solve :99-312 as written; with_textbook(): s-step GMRES (extension)
    size_t restart, pipeline_depth, block_size; bool has_tau = false; double tau = 0.0;
    Preconditioning preconditioning = Preconditioning::Left;  // pca_gmres.rs:61
    PcaGmresSolver(size_t restart, size_t pipeline_depth, size_t block_size, double tol, size_t max_iters)
        : TextbookSolverBase(tol, max_iters), restart(restart), pipeline_depth(pipeline_depth), block_size(block_size) {
        restart_ = (int)restart; side_ = (int)preconditioning;
    }
    PcaGmresSolver& with_preconditioning(Preconditioning m) { preconditioning = m; side_ = (int)m; return *this; }
    PcaGmresSolver& with_tau(double t) { has_tau = true; tau = t; return *this; }
    PcaGmresSolver& with_textbook() { textbook = true; return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override {
        if (!textbook) return kryst_pca_gmres_solve(b, x, n, (int32_t)block_size, (int32_t)pipeline_depth, tau, KRYST_FWD);
        kryst_vec_t bv = nullptr, xv = nullptr;                 // the extension exists for device vectors only
        int32_t rc = kryst_vec_create(ctx_h_, n, &bv);
        if (rc == 0) rc = kryst_vec_create(ctx_h_, n, &xv);
        if (rc == 0) rc = kryst_vec_upload(bv, b, n);
        if (rc == 0) rc = kryst_vec_upload(xv, x, n);
        if (rc == 0) rc = kryst_pca_gmres_textbook_solve_dev(bv, xv, (int32_t)block_size, (int32_t)pipeline_depth, tau, KRYST_FWD);
        if (rc == 0) rc = kryst_vec_download(xv, x, n);
        if (bv) kryst_vec_destroy(bv);
        if (xv) kryst_vec_destroy(xv);
        return rc;
    }
};
enum class Basis { F64 = KRYST_BASIS_F64, F32 = KRYST_BASIS_F32 };
struct CbGmresSolver : TextbookSolverBase {                   // extension: GMRES(restart) with the Krylov basis stored in fp32 (Basis::F64: the control);
    size_t restart; Basis basis = Basis::F32;                 // NoPc and (textbook) Right only; device form only
    Preconditioning preconditioning = Preconditioning::Right;
    CbGmresSolver(size_t restart, double tol, size_t max_iters) : TextbookSolverBase(tol, max_iters), restart(restart) {
        restart_ = (int)restart; side_ = (int)preconditioning;
    }
    CbGmresSolver& with_basis(Basis b) { basis = b; return *this; }
    CbGmresSolver& with_preconditioning(Preconditioning m) { preconditioning = m; side_ = (int)m; return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override {
        kryst_vec_t bv = nullptr, xv = nullptr;
        int32_t rc = kryst_vec_create(ctx_h_, n, &bv);
        if (rc == 0) rc = kryst_vec_create(ctx_h_, n, &xv);
        if (rc == 0) rc = kryst_vec_upload(bv, b, n);
        if (rc == 0) rc = kryst_vec_upload(xv, x, n);
        if (rc == 0) rc = kryst_cbgmres_solve_dev(bv, xv, (int32_t)basis, KRYST_FWD);
        if (rc == 0) rc = kryst_vec_download(xv, x, n);
        if (bv) kryst_vec_destroy(bv);
        if (xv) kryst_vec_destroy(xv);
        return rc;
    }
};
struct QmrSolver : SolverBase {                              // qmr.rs:61-166 as written (a BiCGStab-type loop)
    QmrSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_qmr_solve(b, x, n, KRYST_FWD); }
};
struct CgnrSolver : TextbookSolverBase {                      // cgnr.rs:77-132 as written; with_textbook(): CGNR with A^T (Saad 8.3, extension)
    CgnrSolver(double tol, size_t max_iters) : TextbookSolverBase(tol, max_iters) {}
    CgnrSolver& with_textbook() { textbook = true; return *this; }
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override {
        return textbook ? call_dev(kryst_cgnr_textbook_solve_dev, b, x, n, KRYST_FWD) : kryst_cgnr_solve(b, x, n, KRYST_FWD);
    }
};
struct CgneSolver : SolverBase {                             // cgnr.rs:153-208: CGNR's floating-point operations exactly, the same entry point
    CgneSolver(double tol, size_t max_iters) : SolverBase(tol, max_iters) {}
protected:
    int32_t call(const double* b, double* x, int64_t n, KRYST_SOLVE_ARGS) override { return kryst_cgnr_solve(b, x, n, KRYST_FWD); }
};
#undef KRYST_FWD

// ---- context/: PC<T> (src/context/pc_context.rs:36-76) and KspContext (src/context/ksp_context.rs:25-148) ---------------------
// PC<T>: the reference's configuration enum for preconditioners, plus the constructor it lacks -- build(a) returns the set-up
// device preconditioner.  Kinds without parameters here (Ssor, Multicolor, AMG, AdditiveSchwarz: construct Sor, Amg, AdditiveSchwarz) throw
// KError{Unsupported}.
struct PC {
    enum Kind { JacobiKind, SsorKind, Ilu0Kind, IlupKind, IlutKind, ChebyshevKind, ApproxInvKind, BlockJacobiKind, MulticolorKind, AMGKind, AdditiveSchwarzKind };
    Kind kind; size_t fill = 0; double droptol = 0.0; size_t degree = 0; std::optional<double> emin, emax;
    std::vector<std::vector<size_t>> blocks;
    SparsityPattern pattern; double tol = 0.0; size_t max_iter = 0;
    static PC Jacobi() { return PC{JacobiKind}; }
    static PC Ilu0() { return PC{Ilu0Kind}; }
    static PC Ilup(size_t fill) { PC p{IlupKind}; p.fill = fill; return p; }
    static PC Ilut(size_t fill, double droptol) { PC p{IlutKind}; p.fill = fill; p.droptol = droptol; return p; }
    static PC Chebyshev(size_t degree, std::optional<double> emin = std::nullopt, std::optional<double> emax = std::nullopt) {
        PC p{ChebyshevKind}; p.degree = degree; p.emin = emin; p.emax = emax; return p;
    }
    static PC BlockJacobi(std::vector<std::vector<size_t>> blocks) { PC p{BlockJacobiKind}; p.blocks = std::move(blocks); return p; }   // pc_context.rs:67
    static PC ApproxInv(SparsityPattern pattern, double tol, size_t max_iter) {                                                          // pc_context.rs:63
        PC p{ApproxInvKind}; p.pattern = std::move(pattern); p.tol = tol; p.max_iter = max_iter; return p;
    }
    std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> build(const HipCsrMatrix& a) const {
        std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> pc;
        switch (kind) {
            case JacobiKind: pc = std::make_unique<kryst::Jacobi>(); break;
            case Ilu0Kind: pc = std::make_unique<kryst::Ilu0>(); break;
            case IlupKind: pc = std::make_unique<kryst::Ilup>(fill); break;
            case IlutKind: pc = std::make_unique<kryst::Ilut>(fill, droptol); break;
            case ChebyshevKind: pc = std::make_unique<kryst::Chebyshev>(degree, emin, emax); break;     // the trait object: apply is the stub
            case BlockJacobiKind: pc = std::make_unique<kryst::BlockJacobi>(blocks); break;
            case ApproxInvKind: pc = std::make_unique<kryst::Spai>(pattern, tol, max_iter); break;
            default: throw KError(KRYST_UNSUPPORTED);
        }
        pc->setup(a);
        return pc;
    }
};

enum class SolverKind { Cg, Pcg, GmresLeft, GmresRight, Fgmres, Bicgstab, Cgs, Qmr, Tfqmr, Minres, Cgnr };   // ksp_context.rs:25-50

// KspContext { kind, a, pc, flex_pc, tol, max_it, restart } + solve_context (ksp_context.rs:54-148): a fresh solver of `kind` per
// call, forwarded (a, pc, b, x) exactly as the reference's match does -- FGMRES uses flex_pc, never pc (:101-107); Qmr, Minres and Cgnr
// still throw KError{Unsupported} here (the mirror's tests pin that), although the library has them: a C++ caller reaches them
// directly as QmrSolver, MinresSolver and CgnrSolver (the Python KspContext dispatches them).  `a` is borrowed (the reference
// owns an M by value; a device operator is not copyable).  `pc` is any device preconditioner, e.g. PC::BlockJacobi(blocks).build(a).
struct KspContext {
    SolverKind kind;
    const HipCsrMatrix& a;
    std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> pc;
    std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> flex_pc;
    double tol; size_t max_it; size_t restart;
    KspContext(SolverKind kind, const HipCsrMatrix& a, std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> pc, double tol, size_t max_it,
               size_t restart = 30, std::unique_ptr<Preconditioner<HipCsrMatrix, Vec>> flex_pc = nullptr)
        : kind(kind), a(a), pc(std::move(pc)), flex_pc(std::move(flex_pc)), tol(tol), max_it(max_it), restart(restart) {}
    SolveStats<double> solve_context(const Vec& b, Vec& x) {
        switch (kind) {
            case SolverKind::GmresLeft: { GmresSolver s(restart, tol, max_it); s.with_preconditioning(Preconditioning::Left); return s.solve(a, pc.get(), b, x); }
            case SolverKind::GmresRight: { GmresSolver s(restart, tol, max_it); s.with_preconditioning(Preconditioning::Right); return s.solve(a, pc.get(), b, x); }
            case SolverKind::Fgmres: { FgmresSolver s(tol, max_it, restart); return s.solve_flex(a, flex_pc.get(), b, x); }
            case SolverKind::Cg: { CgSolver s(tol, max_it); return s.solve(a, pc.get(), b, x); }
            case SolverKind::Pcg: { PcgSolver s(tol, max_it); return s.solve(a, pc.get(), b, x); }
            case SolverKind::Bicgstab: { BiCgStabSolver s(tol, max_it); return s.solve(a, pc.get(), b, x); }
            case SolverKind::Cgs: { CgsSolver s(tol, max_it); return s.solve(a, pc.get(), b, x); }
            case SolverKind::Tfqmr: { TfqmrSolver s(tol, max_it); return s.solve(a, pc.get(), b, x); }
            default: throw KError(KRYST_UNSUPPORTED);
        }
    }
};

// ---- dense storage and the direct solvers ---------------------------------------------------------------------------
// DenseMatrix::from_raw (src/matrix/dense.rs:16-25) resident in HBM, column-major; MatVec (core/wrappers.rs:27-38).
class HipDenseMatrix : public MatVec<Vec> {
public:
    static HipDenseMatrix from_raw(size_t nrows, size_t ncols, const Vec& data, std::shared_ptr<Context> ctx = Context::global()) {
        if (data.size() != nrows * ncols) throw KError(KRYST_ERR_ARG);
        kryst_dense_t h = nullptr;
        check(kryst_dense_create(ctx->handle(), (int64_t)nrows, (int64_t)ncols, data.data(), 1, &h));
        return HipDenseMatrix(std::move(ctx), h, nrows, ncols);
    }
    static HipDenseMatrix from_csr(const HipCsrMatrix& a) {      // extension: densified on the device, absent entries +0.0
        kryst_dense_t h = nullptr;
        check(kryst_dense_from_csr(a.handle(), &h));
        return HipDenseMatrix(a.context(), h, a.nrows(), a.ncols());
    }
    HipDenseMatrix(HipDenseMatrix&& o) noexcept : ctx_(std::move(o.ctx_)), h_(o.h_), nrows_(o.nrows_), ncols_(o.ncols_) { o.h_ = nullptr; }
    ~HipDenseMatrix() override { if (h_) kryst_dense_destroy(h_); }
    size_t nrows() const { return nrows_; }
    size_t ncols() const { return ncols_; }
    Vec to_raw() const { Vec d(nrows_ * ncols_); check(kryst_dense_download(h_, d.data())); return d; }
    void matvec(const Vec& x, Vec& y) const override {
        if (x.size() != ncols_ || y.size() != nrows_) throw KError(KRYST_ERR_ARG);
        kryst_vec_t xv = nullptr, yv = nullptr;
        int32_t rc = kryst_vec_create(ctx_->handle(), (int64_t)x.size(), &xv);
        if (rc == 0) rc = kryst_vec_create(ctx_->handle(), (int64_t)y.size(), &yv);
        if (rc == 0) rc = kryst_vec_upload(xv, x.data(), (int64_t)x.size());
        if (rc == 0) rc = kryst_dense_matvec(h_, xv, yv);
        if (rc == 0) rc = kryst_vec_download(yv, y.data(), (int64_t)y.size());
        if (xv) kryst_vec_destroy(xv);
        if (yv) kryst_vec_destroy(yv);
        check(rc);
    }
    kryst_dense_t handle() const { return h_; }
    const std::shared_ptr<Context>& context() const { return ctx_; }
private:
    HipDenseMatrix(std::shared_ptr<Context> c, kryst_dense_t h, size_t nr, size_t nc) : ctx_(std::move(c)), h_(h), nrows_(nr), ncols_(nc) {}
    std::shared_ptr<Context> ctx_; kryst_dense_t h_; size_t nrows_, ncols_;
};

// LuSolver (src/solver/direct_lu.rs:14-90): LU with full pivoting in the operation order of DESIGN.md section 4.12 (a labelled
// deviation from faer's FullPivLu).  pc is accepted and ignored (direct_lu.rs:70).
class LuSolver : public LinearSolver<HipDenseMatrix, Vec> {
public:
    explicit LuSolver(std::shared_ptr<Context> ctx = Context::global()) : ctx_(std::move(ctx)) { check(kryst_lu_create(ctx_->handle(), &h_)); }
    ~LuSolver() override { if (h_) kryst_lu_destroy(h_); }
    LuSolver(const LuSolver&) = delete; LuSolver& operator=(const LuSolver&) = delete;
    SolveStats<double> solve(const HipDenseMatrix& a, const Preconditioner<HipDenseMatrix, Vec>*, const Vec& b, Vec& x) override {
        if (b.size() != x.size()) throw KError(KRYST_ERR_ARG);
        kryst_stats_t st{};
        check(kryst_lu_solve(h_, a.handle(), nullptr, b.data(), x.data(), (int64_t)b.size(), &st));
        return {(size_t)st.iterations, st.final_residual, st.converged != 0};
    }
    // solve_cached (direct_lu.rs:34-43): throws KError{SolveError} where the reference panics (nothing factored yet)
    void solve_cached(const Vec& b, Vec& x) const {
        if (b.size() != x.size()) throw KError(KRYST_ERR_ARG);
        kryst_vec_t v = nullptr;
        int32_t rc = kryst_vec_create(ctx_->handle(), (int64_t)b.size(), &v);
        if (rc == 0) rc = kryst_vec_upload(v, b.data(), (int64_t)b.size());
        if (rc == 0) rc = kryst_lu_solve_cached(h_, v, v);
        if (rc == 0) rc = kryst_vec_download(v, x.data(), (int64_t)x.size());
        if (v) kryst_vec_destroy(v);
        check(rc);
    }
private:
    std::shared_ptr<Context> ctx_; kryst_lu_t h_ = nullptr;
};

// QrSolver (src/solver/direct_lu.rs:96-146), square systems; pc is accepted and ignored (:123).
class QrSolver : public LinearSolver<HipDenseMatrix, Vec> {
public:
    SolveStats<double> solve(const HipDenseMatrix& a, const Preconditioner<HipDenseMatrix, Vec>*, const Vec& b, Vec& x) override {
        if (b.size() != x.size()) throw KError(KRYST_ERR_ARG);
        kryst_stats_t st{};
        check(kryst_qr_solve(a.handle(), nullptr, b.data(), x.data(), (int64_t)b.size(), &st));
        return {(size_t)st.iterations, st.final_residual, st.converged != 0};
    }
};

// ---- mixed precision (an extension): fp32 as a storage format, fp64 arithmetic and scalars -------------------------
// CsrMatrix<f32> lowered from a HipCsrMatrix: copies of its index arrays, its values rounded to fp32 on the device
// Form: what the lowered operator keeps (kryst_csr32_lower_form) -- the CSR arrays alone, or also the operator's CSR-P16 row-pattern form, or
// (Dia, opt-in) its CSR-DIA diagonal streams in fp32
class HipCsrMatrix32 {
public:
    enum Form : int32_t { Plain = KRYST_CSR32_PLAIN, Auto = KRYST_CSR32_AUTO, Pattern = KRYST_CSR32_PATTERN, Dia = KRYST_CSR32_DIA };
    explicit HipCsrMatrix32(const HipCsrMatrix& a, Form form = Plain) : ctx_(a.context()) { check(kryst_csr32_lower_form(a.handle(), form, &h_)); }
    HipCsrMatrix32(HipCsrMatrix32&& o) noexcept : ctx_(std::move(o.ctx_)), h_(o.h_) { o.h_ = nullptr; }
    HipCsrMatrix32(const HipCsrMatrix32&) = delete; HipCsrMatrix32& operator=(const HipCsrMatrix32&) = delete;
    ~HipCsrMatrix32() { if (h_) kryst_csr32_destroy(h_); }
    // {values the rounding changed, nonzero values that became zero or fp32-subnormal, rows}
    std::array<int64_t, 3> info() const { std::array<int64_t, 3> i{}; check(kryst_csr32_info(h_, i.data())); return i; }
    void spmv(const std::vector<float>& x, std::vector<float>& y) const {        // sparse.rs:56-67 on fp32 storage
        kryst_vec32_t xv = nullptr, yv = nullptr;
        int32_t rc = kryst_vec32_create(ctx_->handle(), (int64_t)x.size(), &xv);
        if (rc == 0) rc = kryst_vec32_create(ctx_->handle(), (int64_t)y.size(), &yv);
        if (rc == 0) rc = kryst_vec32_upload(xv, x.data(), (int64_t)x.size());
        if (rc == 0) rc = kryst_spmv32(h_, xv, yv);
        if (rc == 0) rc = kryst_vec32_download(yv, y.data(), (int64_t)y.size());
        if (xv) kryst_vec32_destroy(xv);
        if (yv) kryst_vec32_destroy(yv);
        check(rc);
    }
    // the kernel the next spmv takes (kryst_csr32_encoding): "plain", "pattern", "pattern-stage" or "dia"
    std::string encoding() const {
        int32_t k = -1;
        check(kryst_csr32_encoding(h_, &k));
        return k == 3 ? "dia" : k == 2 ? "pattern-stage" : k == 1 ? "pattern" : "plain";
    }
    kryst_csr32_t handle() const { return h_; }
private:
    std::shared_ptr<Context> ctx_; kryst_csr32_t h_ = nullptr;
};

// fp64 iterative refinement around CG / Jacobi-PCG on the lowered operator (kryst_refine_solve_dev); pc: none, Identity or Jacobi
class RefinementSolver : public LinearSolver<HipCsrMatrix, Vec> {
public:
    RefinementSolver(double tol, size_t max_outer) : conv{tol, max_outer} {}
    RefinementSolver& with_inner(double tol, size_t max_iters) { inner = {tol, max_iters}; return *this; }
    SolveStats<double> solve(const HipCsrMatrix& a, const Preconditioner<HipCsrMatrix, Vec>* pc, const Vec& b, Vec& x) override {
        if (b.size() != x.size()) throw KError(KRYST_ERR_ARG);
        const HipCsrMatrix32 a32(a);
        kryst_params_t po{}, pi{};
        po.tol = conv.tol; po.max_iters = (int64_t)conv.max_iters; po.norm_type = 1;
        pi.tol = inner.tol; pi.max_iters = (int64_t)inner.max_iters; pi.norm_type = 1;
        const size_t cap = conv.max_iters + 2;
        residual_history.assign(cap, 0.0);
        inner_iterations.assign(conv.max_iters, 0);
        int64_t hlen = 0;
        kryst_stats_t st{};
        kryst_ctx_t c = a.context()->handle();
        kryst_vec_t bv = nullptr, xv = nullptr;
        int32_t rc = kryst_vec_create(c, (int64_t)b.size(), &bv);
        if (rc == 0) rc = kryst_vec_create(c, (int64_t)x.size(), &xv);
        if (rc == 0) rc = kryst_vec_upload(bv, b.data(), (int64_t)b.size());
        if (rc == 0) rc = kryst_vec_upload(xv, x.data(), (int64_t)x.size());
        if (rc == 0) rc = kryst_refine_solve_dev(bv, xv, a.handle(), a32.handle(), pc ? pc->device_handle() : nullptr, &po, &pi, &st,
                                                 residual_history.data(), (int64_t)cap, &hlen, inner_iterations.data(), (int64_t)inner_iterations.size());
        if (rc == 0) rc = kryst_vec_download(xv, x.data(), (int64_t)x.size());
        if (bv) kryst_vec_destroy(bv);
        if (xv) kryst_vec_destroy(xv);
        check(rc);
        residual_history.resize(std::min(cap, (size_t)hlen));
        inner_iterations.resize(residual_history.empty() ? 0 : std::min(inner_iterations.size(), residual_history.size() - 1));
        return {(size_t)st.iterations, st.final_residual, st.converged != 0};
    }
    Convergence<double> conv;
    Convergence<double> inner{1e-6, 1000};
    Vec residual_history;
    std::vector<int64_t> inner_iterations;
};

}  // namespace kryst
