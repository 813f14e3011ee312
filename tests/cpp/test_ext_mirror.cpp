// The part of include/kryst_hip.hpp that tests/cpp/test_mirror.cpp and its siblings do not reach, case by case: every class, builder and default
// of the header is driven once on closed-formula inputs, and what it returns is written out bit for bit.  tests/test_gpu_cpp_ext_mirror.py runs
// the same cases through the Python binding (and, where one exists, a restatement) and compares the bits.
//
//   test_ext_mirror OUT      one record per case to OUT:   CASE <name> / i <field> <n> <ints...> / d <field> <n> <16 hex digits...> / END
//                            (doubles as their 64-bit patterns), then the line EXT_MIRROR_DONE <number of cases>
//
// An exception in a case becomes that case's `code` (KError::code; -1 for anything else) and the program goes on.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "kryst_hip.hpp"

using namespace kryst;
typedef Preconditioner<HipCsrMatrix, Vec> Pc;
typedef std::vector<std::vector<size_t>> Sets;

struct Rec {
    long long code = 0;
    std::vector<std::pair<std::string, std::vector<long long>>> ints;
    std::vector<std::pair<std::string, Vec>> dbls;
    void I(const char* f, std::vector<long long> v) { ints.emplace_back(f, std::move(v)); }
    void D(const char* f, Vec v) { dbls.emplace_back(f, std::move(v)); }
};
static FILE* g_out = nullptr;
static int g_cases = 0;

template <class F> static void run(const char* name, F body) {
    Rec r;
    try { body(r); }
    catch (const KError& e) { r.code = e.code; }
    catch (const std::exception&) { r.code = -1; }
    std::fprintf(g_out, "CASE %s\ni code 1 %lld\n", name, r.code);
    for (auto& f : r.ints) {
        std::fprintf(g_out, "i %s %zu", f.first.c_str(), f.second.size());
        for (long long v : f.second) std::fprintf(g_out, " %lld", v);
        std::fprintf(g_out, "\n");
    }
    for (auto& f : r.dbls) {
        std::fprintf(g_out, "d %s %zu", f.first.c_str(), f.second.size());
        for (double v : f.second) { uint64_t u; std::memcpy(&u, &v, 8); std::fprintf(g_out, " %016" PRIx64, u); }
        std::fprintf(g_out, "\n");
    }
    std::fprintf(g_out, "END\n");
    std::fflush(g_out);
    ++g_cases;
}

// ---- inputs: closed formulas with exactly representable values, the same in tests/test_gpu_cpp_ext_mirror.py
static Vec fb(size_t n) { Vec v(n); for (size_t i = 0; i < n; ++i) v[i] = 1.0 + (double)(i % 7) / 8.0; return v; }
static Vec fx(size_t n) { Vec v(n); for (size_t i = 0; i < n; ++i) v[i] = ((double)((i * 37) % 64) - 32.0) / 16.0; return v; }
static HipCsrMatrix tridiag(size_t n) {                            // lower -1.5, diagonal 3 + (i % 3) / 2, upper -0.5
    std::vector<size_t> rp(n + 1, 0), ci; Vec va;
    for (size_t i = 0; i < n; ++i) {
        if (i > 0) { ci.push_back(i - 1); va.push_back(-1.5); }
        ci.push_back(i); va.push_back(3.0 + 0.5 * (double)(i % 3));
        if (i + 1 < n) { ci.push_back(i + 1); va.push_back(-0.5); }
        rp[i + 1] = ci.size();
    }
    return HipCsrMatrix::from_csr(n, n, rp, ci, va);
}
static HipCsrMatrix shifted_poisson(size_t N, double diag) {       // 7 points, -1 off the diagonal, `diag` on it, row = i + N (j + N k)
    std::vector<size_t> rp(N * N * N + 1, 0), ci; Vec va;
    for (size_t k = 0; k < N; ++k) for (size_t j = 0; j < N; ++j) for (size_t i = 0; i < N; ++i) {
        const size_t row = i + N * (j + N * k);
        if (k > 0) { ci.push_back(row - N * N); va.push_back(-1.0); }
        if (j > 0) { ci.push_back(row - N); va.push_back(-1.0); }
        if (i > 0) { ci.push_back(row - 1); va.push_back(-1.0); }
        ci.push_back(row); va.push_back(diag);
        if (i + 1 < N) { ci.push_back(row + 1); va.push_back(-1.0); }
        if (j + 1 < N) { ci.push_back(row + N); va.push_back(-1.0); }
        if (k + 1 < N) { ci.push_back(row + N * N); va.push_back(-1.0); }
        rp[row + 1] = ci.size();
    }
    return HipCsrMatrix::from_csr(N * N * N, N * N * N, rp, ci, va);
}
static Sets chunks(size_t n, size_t len, bool reversed) {           // contiguous index sets of `len` rows, each listed backwards if asked
    Sets s;
    for (size_t lo = 0; lo < n; lo += len) {
        std::vector<size_t> g;
        for (size_t i = lo; i < std::min(n, lo + len); ++i) g.push_back(i);
        if (reversed) std::reverse(g.begin(), g.end());
        s.push_back(g);
    }
    return s;
}

// ---- the two shapes of a case
static void solve(Rec& r, SolverBase& s, const HipCsrMatrix& a, const Pc* pc, const Vec& b, Vec x, bool with_history = true) {
    LinearSolver<HipCsrMatrix, Vec>& trait = s;                     // through the trait, as a caller of the reference would
    try {
        const SolveStats<double> st = trait.solve(a, pc, b, x);
        r.I("iterations", {(long long)st.iterations}); r.I("converged", {st.converged ? 1 : 0}); r.D("final", {st.final_residual});
    } catch (const KError& e) { r.code = e.code; }
    if (with_history) r.D("hist", s.residual_history);
    r.D("x", x);
}
static void apply(Rec& r, const Pc& pc, const Vec& rr, double zfill = 0.0) {
    Vec z(rr.size(), zfill);
    try { pc.apply(rr, z); } catch (const KError& e) { r.code = e.code; }
    r.D("z", z);
}
static void watch(SolverBase& s, std::vector<long long>& mi, Vec& mr) { s.monitor = [&mi, &mr](size_t i, double v) { mi.push_back((long long)i); mr.push_back(v); }; }

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_ext_mirror OUT\n"); return 2; }
    g_out = std::fopen(argv[1], "w");
    if (!g_out) { std::fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }

    const std::shared_ptr<Context> ctx = Context::global();
    HipCsrMatrix P8 = HipCsrMatrix::stencil7(8, 0, ctx), A8 = HipCsrMatrix::stencil7(8, 1, ctx), C9 = HipCsrMatrix::stencil7(9, 2, ctx);
    HipCsrMatrix T10 = tridiag(10), T513 = tridiag(513), S6 = shifted_poisson(6, 8.0);
    HipCsrMatrix R35 = HipCsrMatrix::from_csr(3, 5, {0, 2, 3, 5}, {0, 4, 1, 2, 3}, {1.0, 2.0, 3.0, 4.0, -0.5});
    const Vec b512 = fb(512), x512 = fx(512), b729 = fb(729), x729 = fx(729), b513 = fb(513), x513 = fx(513);
    Jacobi jacP; jacP.setup(P8);
    Jacobi jacC; jacC.setup(C9);
    Jacobi jacT; jacT.setup(T513);

    // ---- BlockJacobi
    const Sets bj10 = {{2, 0, 1}, {4, 2, 3}, {8, 7, 9, 5}};         // unsorted, row 2 twice (the last block decides), row 6 in none
    run("bj_explicit_apply", [&](Rec& r) { BlockJacobi p(bj10); p.setup(T10); apply(r, p, fx(10)); });
    run("bj_uniform8_apply", [&](Rec& r) { BlockJacobi p = BlockJacobi::uniform(8); p.setup(C9); apply(r, p, x729); });
    run("bj_uniform1_apply", [&](Rec& r) { BlockJacobi p = BlockJacobi::uniform(1); p.setup(C9); apply(r, p, x729); });
    const Sets bj512 = chunks(512, 8, true);
    run("bj_apply", [&](Rec& r) { BlockJacobi p(bj512); p.setup(P8); apply(r, p, x512); });
    run("bj_pcg", [&](Rec& r) { BlockJacobi p(bj512); p.setup(P8); PcgSolver s(1e-8, 100); solve(r, s, P8, &p, b512, x512); });
    run("bj_build_apply", [&](Rec& r) { auto p = PC::BlockJacobi(bj512).build(P8); apply(r, *p, x512); });
    run("bj_build_pcg", [&](Rec& r) { auto p = PC::BlockJacobi(bj512).build(P8); PcgSolver s(1e-8, 100); solve(r, s, P8, p.get(), b512, x512); });

    // ---- AdditiveSchwarz: 27 subdomains of 27 rows (three grid lines) on convdiff 9^3; right-preconditioned GMRES(10)
    const Sets sub729 = chunks(729, 27, true);
    auto asm_pair = [&](const char* n_apply, const char* n_solve, const HipCsrMatrix& a, AdditiveSchwarz& p) {
        bool ok = false;
        run(n_apply, [&](Rec& r) { p.setup(a); ok = true; apply(r, p, fx(a.nrows())); });
        if (n_solve) run(n_solve, [&](Rec& r) {
            if (!ok) throw KError(KRYST_SOLVE_ERROR);
            GmresSolver s(10, 1e-8, 60); s.with_preconditioning(Preconditioning::Right); solve(r, s, a, &p, fb(a.nrows()), fx(a.nrows()));
        });
    };
    { AdditiveSchwarz p(2, sub729); asm_pair("asm_written_apply", "asm_written_gmres", C9, p); }               // overlap 2 is ignored as written
    { AdditiveSchwarz p(1, {}, 0); asm_pair("asm_nparts0_apply", nullptr, T10, p); }        // one part of all rows: the exact inverse
    { AdditiveSchwarz p(1, {}, 3); asm_pair("asm_nparts3_apply", "asm_nparts3_gmres", T10, p); }
    { AdditiveSchwarz p(1, sub729, 0, AdditiveSchwarz::Grown); asm_pair("asm_grown_apply", "asm_grown_gmres", C9, p); }
    { AdditiveSchwarz p(1, sub729, 0, AdditiveSchwarz::Restricted); asm_pair("asm_restricted_apply", "asm_restricted_gmres", C9, p); }
    { AdditiveSchwarz p(1, {}, 3, AdditiveSchwarz::Restricted); p.with_sub_ilu(KRYST_ILU_TRUE_ILU0); asm_pair("asm_ilu_true_apply", "asm_ilu_true_gmres", C9, p); }
    { AdditiveSchwarz p(0, {}, 0); p.with_sub_ilu(KRYST_ILU_ILUP0); asm_pair("asm_ilu_ilup0_apply", "asm_ilu_ilup0_gmres", C9, p); }
    { AdditiveSchwarz p(0, sub729); p.with_sub_ilu(); asm_pair("asm_ilu_default_apply", "asm_ilu_default_gmres", C9, p); }

    // ---- Sor on convdiff 9^3: omega 1.3, its 2, lits 1, fshift 0.25
    run("sor_sym_apply", [&](Rec& r) { Sor p(1.3, 2, 1, MatSorType::SYMMETRIC_SWEEP, 0.25); p.setup(C9); apply(r, p, x729); });
    run("sor_lower_apply", [&](Rec& r) { Sor p(1.3, 2, 1, MatSorType::APPLY_LOWER, 0.25); p.setup(C9); apply(r, p, x729); });
    run("sor_upper_zero_apply", [&](Rec& r) { Sor p(1.3, 2, 1, MatSorType::APPLY_UPPER | MatSorType::ZERO_INITIAL_GUESS, 0.25); p.setup(C9); apply(r, p, x729); });
    std::vector<size_t> redblack(729);
    for (size_t k = 0; k < 9; ++k) for (size_t j = 0; j < 9; ++j) for (size_t i = 0; i < 9; ++i) redblack[i + 9 * (j + 9 * k)] = (i + j + k) % 2;
    run("sor_colors_apply", [&](Rec& r) { Sor p(1.3, 2, 1, MatSorType::SYMMETRIC_SWEEP, 0.25); p.with_colors(redblack); p.setup(C9); apply(r, p, x729); });
    run("sor_setters_apply", [&](Rec& r) {
        Sor p(1.0, 1, 0, MatSorType::APPLY_LOWER, 0.0);
        p.set_omega(1.3); p.set_its(2); p.set_lits(1); p.set_sym(MatSorType::SYMMETRIC_SWEEP); p.set_fshift(0.25);
        r.D("omega_fshift", {p.omega(), p.fshift()}); r.I("its_lits_sym", {(long long)p.its(), (long long)p.lits(), (long long)p.sym()});
        p.setup(C9); apply(r, p, x729);
    });
    run("sor_colors_wrong_length", [&](Rec&) { Sor p(1.3, 2, 1, MatSorType::SYMMETRIC_SWEEP, 0.25); p.with_colors(std::vector<size_t>(5, 0)); p.setup(C9); });
    run("sor_moved_apply", [&](Rec& r) {                           // DevicePc is move-only: the handle travels, the source is left empty
        Sor p(1.3, 2, 1, MatSorType::SYMMETRIC_SWEEP, 0.25); p.setup(C9);
        Sor q(std::move(p));
        Sor t(1.0, 1, 0, MatSorType::APPLY_LOWER, 0.0); t.setup(C9);
        const bool held = t.device_handle() != nullptr;
        t = std::move(q);                                          // destroys the handle t held, takes q's
        r.I("empty_after_move", {p.device_handle() == nullptr ? 1 : 0, q.device_handle() == nullptr ? 1 : 0, held ? 1 : 0});
        const DevicePc& base = t;
        apply(r, base, x729);
    });
    run("sor_gmres", [&](Rec& r) {
        Sor p(1.3, 2, 1, MatSorType::SYMMETRIC_SWEEP, 0.25); p.setup(C9);
        GmresSolver s(10, 1e-8, 60); s.with_preconditioning(Preconditioning::Right); solve(r, s, C9, &p, b729, x729);
    });

    // ---- Amg as written, applies and PCG from x = 0: two levels on poisson 8^3 converge; the default hierarchy on poisson 6^3 + 2 I runs
    // for some iterations and ends in IndefinitePreconditioner, as written
    run("amg_default_apply", [&](Rec& r) { Amg p; p.setup(P8); apply(r, p, x512); });
    run("amg_l2_apply", [&](Rec& r) { Amg p(2, 0.25); p.setup(P8); apply(r, p, x512); });
    run("amg_default_pcg", [&](Rec& r) { Amg p; p.setup(S6); PcgSolver s(1e-8, 100); solve(r, s, S6, &p, fb(216), Vec(216, 0.0)); });
    run("amg_l2_pcg", [&](Rec& r) { Amg p(2, 0.25); p.setup(P8); PcgSolver s(1e-8, 100); solve(r, s, P8, &p, b512, Vec(512, 0.0)); });

    // ---- Spai on poisson 8^3
    auto spai_export = [](Rec& r, const Spai& p) {
        std::vector<int64_t> rp; std::vector<int32_t> col; Vec val;
        p.export_csr(rp, col, val);
        r.I("row_ptr", std::vector<long long>(rp.begin(), rp.end())); r.I("col", std::vector<long long>(col.begin(), col.end())); r.D("val", val);
    };
    Sets tri_pat(512);
    for (size_t j = 0; j < 512; ++j) { if (j + 1 < 512) tri_pat[j].push_back(j + 1); tri_pat[j].push_back(j); if (j > 0) tri_pat[j].push_back(j - 1); }
    run("spai_manual", [&](Rec& r) { Spai p(SparsityPattern::Manual(tri_pat), 0.01); p.setup(P8); spai_export(r, p); apply(r, p, x512); });
    run("spai_operator", [&](Rec& r) { Spai p(SparsityPattern::Operator(), 0.01); p.setup(P8); spai_export(r, p); apply(r, p, x512); });
    run("spai_operator_pcg", [&](Rec& r) { Spai p(SparsityPattern::Operator(), 0.01); p.setup(P8); PcgSolver s(1e-8, 100); solve(r, s, P8, &p, b512, x512); });
    run("spai_auto", [&](Rec&) { Spai p(SparsityPattern::Auto(), 0.01); p.setup(P8); });
    run("spai_build_apply", [&](Rec& r) { auto p = PC::ApproxInv(SparsityPattern::Operator(), 0.01, 5).build(P8); apply(r, *p, x512); });

    // ---- estimate_spectrum on aniso 8^3, and on 10 rows where the Lanczos run ends before `steps`
    auto spectrum = [](Rec& r, const HipCsrMatrix& a, bool jac, int steps) {
        const SpectrumEstimate e = estimate_spectrum(a, jac, steps);
        r.D("alpha", e.alpha); r.D("beta", e.beta); r.D("theta_gersh", {e.theta_min, e.theta_max, e.gershgorin});
    };
    run("spec_j1_s1", [&](Rec& r) { spectrum(r, A8, true, 1); });
    run("spec_j1_s10", [&](Rec& r) { spectrum(r, A8, true, 10); });
    run("spec_j1_s64", [&](Rec& r) { spectrum(r, A8, true, 64); });
    run("spec_j0_s1", [&](Rec& r) { spectrum(r, A8, false, 1); });
    run("spec_j0_s10", [&](Rec& r) { spectrum(r, A8, false, 10); });
    run("spec_j0_s64", [&](Rec& r) { spectrum(r, A8, false, 64); });
    run("spec_t10_s64", [&](Rec& r) { spectrum(r, T10, true, 64); });

    // ---- ChebyshevPoly on poisson 8^3
    auto cheb = [&](Rec& r, ChebyshevPoly& p) {
        p.setup(P8);
        const std::pair<double, double> bd = p.bounds();
        r.D("bounds", {bd.first, bd.second}); r.I("fused", {p.fused() ? 1 : 0});
        apply(r, p, x512);
    };
    run("cheb_both", [&](Rec& r) { ChebyshevPoly p(4, 0.125, 2.0); cheb(r, p); });
    run("cheb_neither", [&](Rec& r) { ChebyshevPoly p(4); cheb(r, p); });
    run("cheb_max_only", [&](Rec& r) { ChebyshevPoly p(4, std::nullopt, 1.875); cheb(r, p); });
    run("cheb_no_jacobi", [&](Rec& r) { ChebyshevPoly p(3, std::nullopt, std::nullopt, false); cheb(r, p); });
    run("cheb_knobs", [&](Rec& r) { ChebyshevPoly p(5, std::nullopt, std::nullopt, true, 6, 20.0, 1.25, 0x1234); cheb(r, p); });
    run("cheb_pcg", [&](Rec& r) { ChebyshevPoly p(4); p.setup(P8); PcgSolver s(1e-8, 100); solve(r, s, P8, &p, b512, x512); });
    run("cheb_build_stub", [&](Rec& r) { auto p = PC::Chebyshev(3, 0.125, 12.0).build(P8); apply(r, *p, x512, 0.5); });

    // ---- MINRES / QMR / CGNR / CGNE
    run("minres", [&](Rec& r) { MinresSolver s(1e-8, 100); solve(r, s, P8, nullptr, b512, x512); });
    run("minres_textbook", [&](Rec& r) { MinresSolver s(1e-8, 100); s.with_textbook(); solve(r, s, P8, nullptr, b512, x512); });
    run("qmr", [&](Rec& r) { QmrSolver s(1e-8, 100); solve(r, s, C9, nullptr, b729, x729); });
    run("cgnr", [&](Rec& r) { CgnrSolver s(1e-8, 60); solve(r, s, C9, nullptr, b729, x729); });
    run("cgnr_textbook", [&](Rec& r) { CgnrSolver s(1e-8, 60); s.with_textbook(); solve(r, s, C9, nullptr, b729, x729); });
    run("cgne", [&](Rec& r) { CgneSolver s(1e-8, 60); solve(r, s, C9, nullptr, b729, x729); });

    // ---- PcaGmresSolver
    run("pca_default_side", [&](Rec& r) { PcaGmresSolver s(5, 2, 1, 1e-6, 23); r.I("side", {(long long)s.preconditioning}); solve(r, s, C9, &jacC, b729, x729); });
    run("pca_right", [&](Rec& r) { PcaGmresSolver s(5, 2, 1, 1e-6, 23); s.with_preconditioning(Preconditioning::Right); solve(r, s, C9, &jacC, b729, x729); });
    run("pca_tau", [&](Rec& r) { PcaGmresSolver s(5, 2, 1, 1e-6, 23); s.with_preconditioning(Preconditioning::Right).with_tau(0.5); solve(r, s, C9, &jacC, b729, x729); });
    run("pca_textbook", [&](Rec& r) { PcaGmresSolver s(16, 2, 4, 1e-8, 40); s.with_preconditioning(Preconditioning::Right).with_textbook(); solve(r, s, C9, &jacC, b729, x729); });
    run("pca_block0", [&](Rec& r) { PcaGmresSolver s(5, 2, 0, 1e-6, 23); solve(r, s, C9, &jacC, b729, x729); });
    run("pca_textbook_block0", [&](Rec& r) { PcaGmresSolver s(16, 2, 0, 1e-8, 40); s.with_preconditioning(Preconditioning::Right).with_textbook(); solve(r, s, C9, &jacC, b729, x729); });

    // ---- CbGmresSolver: non-zero x0 throughout
    run("cb_f32_none_r5", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); s.with_preconditioning(Preconditioning::None); solve(r, s, C9, nullptr, b729, x729); });
    run("cb_f64_none_r5", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); s.with_basis(Basis::F64).with_preconditioning(Preconditioning::None); solve(r, s, C9, nullptr, b729, x729); });
    run("cb_f32_right_r30", [&](Rec& r) { CbGmresSolver s(30, 1e-8, 40); s.with_basis(Basis::F32).with_preconditioning(Preconditioning::Right); solve(r, s, C9, &jacC, b729, x729); });
    run("cb_f64_right_r30", [&](Rec& r) { CbGmresSolver s(30, 1e-8, 40); s.with_basis(Basis::F64).with_preconditioning(Preconditioning::Right); solve(r, s, C9, &jacC, b729, x729); });
    run("cb_f32_right_r5_t513", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); s.with_preconditioning(Preconditioning::Right); solve(r, s, T513, &jacT, b513, x513); });
    run("cb_left", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); s.with_preconditioning(Preconditioning::Left); solve(r, s, C9, &jacC, b729, x729); });
    run("cb_defaults", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); r.I("side_basis", {(long long)s.preconditioning, (long long)s.basis}); solve(r, s, C9, &jacC, b729, x729); });

    // ---- GMRES LeftTextbook, the CG builders, FGMRES preallocate, KspContext Cgs / Tfqmr
    run("gmres_left_textbook", [&](Rec& r) { GmresSolver s(10, 1e-8, 60); s.with_preconditioning(Preconditioning::LeftTextbook); solve(r, s, C9, &jacC, b729, x729); });
    run("cg_norm_preconditioned", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_norm(CgNormType::Preconditioned); solve(r, s, P8, nullptr, b512, x512); });
    run("cg_norm_unpreconditioned", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_norm(CgNormType::Unpreconditioned); solve(r, s, P8, nullptr, b512, x512); });
    run("cg_norm_natural", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_norm(CgNormType::Natural); solve(r, s, P8, nullptr, b512, x512); });
    run("cg_norm_none", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_norm(CgNormType::None); solve(r, s, P8, nullptr, b512, x512); });
    run("cg_radius", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_radius(64.0); solve(r, s, P8, nullptr, b512, Vec(512, 0.0)); });
    run("cg_obj_target", [&](Rec& r) { CgSolver s(1e-8, 40); s.with_obj_target(-1000.0); solve(r, s, P8, nullptr, b512, Vec(512, 0.0)); });
    run("pcg_norm_preconditioned", [&](Rec& r) { PcgSolver s(1e-8, 40); s.with_norm(CgNormType::Preconditioned); solve(r, s, P8, &jacP, b512, x512); });
    run("pcg_norm_natural", [&](Rec& r) { PcgSolver s(1e-8, 40); s.with_norm(CgNormType::Natural); solve(r, s, P8, &jacP, b512, x512); });
    run("fgmres_preallocate", [&](Rec& r) { FgmresSolver s(1e-8, 40, 10); s.with_preallocate(true); solve(r, s, C9, &jacC, b729, x729); });
    auto ksp = [&](Rec& r, SolverKind k) {
        KspContext c(k, C9, PC::Jacobi().build(C9), 1e-8, 40);
        Vec x = x729;
        const SolveStats<double> st = c.solve_context(b729, x);
        r.I("iterations", {(long long)st.iterations}); r.I("converged", {st.converged ? 1 : 0}); r.D("final", {st.final_residual}); r.D("x", x);
    };
    run("ksp_cgs", [&](Rec& r) { ksp(r, SolverKind::Cgs); });
    run("ksp_tfqmr", [&](Rec& r) { ksp(r, SolverKind::Tfqmr); });

    // ---- history capacity: tol 1e-30, 23 iterations (no multiple of the restart 5), every solver class
    run("cap_cg", [&](Rec& r) { CgSolver s(1e-30, 23); solve(r, s, P8, nullptr, b512, x512); });
    run("cap_pcg", [&](Rec& r) { PcgSolver s(1e-30, 23); solve(r, s, P8, &jacP, b512, x512); });
    run("cap_gmres", [&](Rec& r) { GmresSolver s(5, 1e-30, 23); solve(r, s, C9, &jacC, b729, x729); });
    run("cap_fgmres", [&](Rec& r) { FgmresSolver s(1e-30, 23, 5); solve(r, s, C9, &jacC, b729, x729); });
    run("cap_bicgstab", [&](Rec& r) { BiCgStabSolver s(1e-30, 23); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_cgs", [&](Rec& r) { CgsSolver s(1e-30, 23); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_tfqmr", [&](Rec& r) { TfqmrSolver s(1e-30, 23); solve(r, s, T513, nullptr, b513, x513); });      // (on convdiff 9^3 it breaks down at 13)
    run("cap_minres", [&](Rec& r) { MinresSolver s(1e-30, 23); solve(r, s, P8, nullptr, b512, x512); });
    run("cap_minres_textbook", [&](Rec& r) { MinresSolver s(1e-30, 23); s.with_textbook(); solve(r, s, P8, nullptr, b512, x512); });
    run("cap_qmr", [&](Rec& r) { QmrSolver s(1e-30, 23); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_cgnr", [&](Rec& r) { CgnrSolver s(1e-30, 23); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_cgnr_textbook", [&](Rec& r) { CgnrSolver s(1e-30, 23); s.with_textbook(); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_cgne", [&](Rec& r) { CgneSolver s(1e-30, 23); solve(r, s, C9, nullptr, b729, x729); });
    run("cap_pca", [&](Rec& r) { PcaGmresSolver s(5, 2, 1, 1e-30, 23); s.with_preconditioning(Preconditioning::Right); solve(r, s, C9, &jacC, b729, x729); });
    run("cap_pca_textbook", [&](Rec& r) { PcaGmresSolver s(5, 2, 2, 1e-30, 23); s.with_preconditioning(Preconditioning::Right).with_textbook(); solve(r, s, C9, &jacC, b729, x729); });
    run("cap_cb", [&](Rec& r) { CbGmresSolver s(5, 1e-30, 23); solve(r, s, C9, &jacC, b729, x729); });

    // ---- solver object state: histories accumulate, clear_history empties, the monitor's sequence
    run("state_two_solves", [&](Rec& r) {
        MinresSolver s(1e-8, 100);
        Vec x1 = x512, x2(512, 0.0);
        s.solve(P8, nullptr, b512, x1);
        const size_t first = s.residual_history.size();
        s.solve(P8, nullptr, b512, x2);
        const Convergence<double> c = s.conv;
        r.D("conv_tol", {c.tol}); r.I("conv_max_iters", {(long long)c.max_iters});
        r.I("lengths", {(long long)first, (long long)s.residual_history.size()}); r.D("hist", s.residual_history); r.D("x", x2);
        s.clear_history();
        r.I("after_clear", {(long long)s.residual_history.size()});
    });
    auto monitored = [&](Rec& r, TextbookSolverBase& s, const HipCsrMatrix& a, const Pc* pc, const Vec& b, const Vec& x, int every) {
        std::vector<long long> mi; Vec mr;
        watch(s, mi, mr); s.check_every = every;
        solve(r, s, a, pc, b, x);
        r.I("mon_i", mi); r.D("mon_r", mr);
    };
    run("mon_minres", [&](Rec& r) { MinresSolver s(1e-8, 100); monitored(r, s, P8, nullptr, b512, x512, 0); });
    run("mon_minres_every3", [&](Rec& r) { MinresSolver s(1e-8, 100); monitored(r, s, P8, nullptr, b512, x512, 3); });
    run("mon_cb", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); monitored(r, s, C9, &jacC, b729, x729, 0); });
    run("mon_cb_every3", [&](Rec& r) { CbGmresSolver s(5, 1e-10, 23); monitored(r, s, C9, &jacC, b729, x729, 3); });

    // ---- mattransvec
    run("mtv_rect", [&](Rec& r) { Vec y(5, 0.5); try { R35.mattransvec(fx(3), y); } catch (const KError& e) { r.code = e.code; } r.D("y", y); });
    run("mtv_convdiff", [&](Rec& r) { Vec y(729, 0.5); try { C9.mattransvec(x729, y); } catch (const KError& e) { r.code = e.code; } r.D("y", y); });
    run("mtv_swapped", [&](Rec& r) { Vec y(3, 0.5); try { R35.mattransvec(fx(5), y); } catch (const KError& e) { r.code = e.code; } r.D("y", y); });

    // ---- the two transport switches on a single-rank context
    run("single_rank_modes", [&](Rec& r) {
        const bool peer = C9.halo_peer_stores(true);
        const bool ipc = ctx->scalar_reduce_ipc(true);
        r.I("peer_ipc", {peer ? 1 : 0, ipc ? 1 : 0});
    });

    std::fprintf(g_out, "EXT_MIRROR_DONE %d\n", g_cases);
    std::fclose(g_out);
    return 0;
}
