// Device-resident MINRES, QMR and CGNR: MinresSolver::solve (src/solver/minres.rs:60-219), QmrSolver::solve (src/solver/qmr.rs:61-166)
// and CgnrSolver::solve (src/solver/cgnr.rs:77-132) as written, operation by operation, plus two labelled extensions: textbook MINRES
// (Paige & Saunders 1975, unpreconditioned) and textbook CGNR (Saad, Iterative Methods for Sparse Linear Systems, section 8.3) with a
// real A^T.  All five ignore the preconditioner like the reference (minres.rs:61, qmr.rs:64, cgnr.rs:78).  CgneSolver::solve
// (cgnr.rs:153-208) does CGNR's floating-point operations exactly and binds to the CGNR path.
//
// Reference work with no observable effect is dropped (like TFQMR's `w`): MINRES's true-residual SpMV and its prints (minres.rs:173-180,
// 183-186), QMR's A^T p_tld (qmr.rs:121-122, v_tld is never read).
//
// HBM passes per iteration (n-word vectors, SpMVs aside):
//   MINRES as written  1 SpMV, 2 vector kernels, 2 folds, 12 words (+1 for x_best on an improving step)
//   QMR as written     3 SpMVs (A p, A s, A x), 4 vector kernels, 3 folds, 19 words
//   CGNR as written    3 SpMVs (A p, A(Ap), A r), 2 vector kernels, 3 folds, 9 words
//   textbook MINRES    1 SpMV, 2 vector kernels, 2 folds, 12 words
//   textbook CGNR      2 SpMVs (A p, A^T r), 2 vector kernels, 3 folds, 9 words
#include "solvers.h"

namespace kr {

// the update owed by the iteration that ended the solve (st->early raised, st->iter = k) still runs; every later one is skipped
struct GateStopAt {
    const DevState* st; long long k;
    __device__ __forceinline__ bool skip() const { return st->done && !(st->early && st->iter == k); }
};

// =================================================================== MINRES (both forms)
struct MinState {                    // device, next to DevState
    double beta, phi, rho_bar, c_prev, s_prev, phi_min, beta1;       // as written: the recurrences of minres.rs:97-124
    double c, s, eta;                                                // textbook: the last rotation and phi_bar
    double beta_next, delta, epsilon, rho, coef;                     // what the update kernel of this iteration reads
    int best;                                                        // as written: |phi_bar| < phi_min, x_best = x_out (:203-206)
};
struct MinScaleOp {                  // v = r / beta1 (minres.rs:95)
    static constexpr int NQ = 0; static constexpr const char* TAG = "MinScale";
    const MinState* ms; const double* r; double* v;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double b1 = ms->beta1;
        const d2 rr = ld2(r, i);
        st2(v, i, rr.a / b1, rr.b / b1);
    }
};
struct MinLanczosOp {                // v_next = v_next - alpha v - beta v_prev (minres.rs:129-133); partial (v_next, v_next) (:134)
    static constexpr int NQ = 1; static constexpr const char* TAG = "MinLanczos";
    const DevState* st; const MinState* ms; const double* v; const double* vp; double* vn;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double al = st->alpha, be = ms->beta;
        const d2 nn = ld2(vn, i), vv = ld2(v, i), pp = ld2(vp, i);
        const double n0 = nn.a - al * vv.a - be * pp.a, n1 = nn.b - al * vv.b - be * pp.b;
        st2(vn, i, n0, n1);
        if (in0) acc[0] = acc[0] + n0 * n0;
        if (in1) acc[0] = acc[0] + n1 * n1;
    }
};
struct MinAlphaLogic {               // alpha = (v, A v) (minres.rs:128)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const { c.st->alpha = red[0]; }
};
struct MinInitLogic {                // minres.rs:72-124 ; red0 = (r, r).  textbook: the same start from x0
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; MinState* ms;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double beta1 = dsqrt(red[0]);                             // :80
        ms->beta1 = beta1; st->res0 = beta1;
        st->iter = 0; st->iterations = 0; st->final_residual = beta1; st->converged = 0;   // :118-122
        if (beta1 == 0.0) { st->converged = 1; c.finish(KRYST_OK); return; }   // :81-85 (x = 0; textbook: x0 is exact)
        ms->beta = beta1; ms->c_prev = 1.0; ms->s_prev = 0.0; ms->rho_bar = beta1; ms->phi = beta1;   // :98-110
        ms->phi_min = fabs(beta1);                                      // :94
        ms->c = 1.0; ms->s = 0.0; ms->eta = beta1;
        if (c.max_iters <= 0) c.finish(KRYST_OK);                       // :216-218 with an empty loop
    }
};
struct MinStepLogic {                // minres.rs:134-211 scalars ; red0 = (v_next, v_next)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; MinState* ms; long long j;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double alpha = st->alpha, beta = ms->beta;
        const double beta_next = dsqrt(red[0]);                         // :134
        if (beta_next == 0.0) { c.finish(KRYST_OK); return; }           // :136-139, before stats is touched
        double delta, epsilon;
        if (j == 1) { delta = 0.0; epsilon = 0.0; }                     // :147-153
        else { delta = ms->s_prev * beta; epsilon = -ms->c_prev * beta; }
        const double rho = dsqrt(ms->rho_bar * ms->rho_bar + alpha * alpha);   // :156
        const double cc = rho != 0.0 ? ms->rho_bar / rho : 1.0;         // :157
        const double ss = rho != 0.0 ? alpha / rho : 0.0;               // :158
        const double phi_next = cc * ms->phi;                           // :159
        const double phi_bar = -ss * ms->phi;                           // :160
        ms->beta_next = beta_next; ms->delta = delta; ms->epsilon = epsilon; ms->rho = rho; ms->coef = phi_next;
        if (rho == 0.0) { c.finish(KRYST_OK); return; }                 // :182-186: x_out is updated, x_best is not -- x_out is never returned
        ms->beta = beta_next; ms->phi = phi_next; ms->rho_bar = -ss * beta_next;   // :189-198
        ms->c_prev = cc; ms->s_prev = ss;
        const double res = fabs(phi_bar);
        ms->best = res < ms->phi_min ? 1 : 0;                           // :202-206
        if (ms->best) ms->phi_min = res;
        c.push(res);                                                    // addition: the reference keeps no history
        const bool stop = c.check(res, ms->beta1, j);                   // :207-208 (stop implies converged)
        st->final_residual = ms->phi_min;                               // :211 / :217
        st->iter = j;
        if (stop) { st->early = 1; c.finish(KRYST_OK); }                // :209-213 after this iteration's x_best update
    }
};
struct MinUpdateOp {                 // v_next /= beta_next (:141-144) ; w_new (:163-174) ; x_out += phi_next w_new (:177-179) ; x_best (:205)
    static constexpr int NQ = 0; static constexpr const char* TAG = "MinUpdate";
    const MinState* ms; int first; const double* v; const double* w; const double* wp; double* vn; double* wn; double* xo; double* xb;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double bn = ms->beta_next, rho = ms->rho, pn = ms->coef;
        const d2 nn = ld2(vn, i), vv = ld2(v, i), xx = ld2(xo, i);
        st2(vn, i, nn.a / bn, nn.b / bn);
        double w0, w1;
        if (first) { w0 = vv.a / rho; w1 = vv.b / rho; }
        else {
            const double de = ms->delta, ep = ms->epsilon;
            const d2 ww = ld2(w, i), pp = ld2(wp, i);
            w0 = (vv.a - de * ww.a - ep * pp.a) / rho; w1 = (vv.b - de * ww.b - ep * pp.b) / rho;
        }
        st2(wn, i, w0, w1);
        const double x0 = xx.a + pn * w0, x1 = xx.b + pn * w1;
        st2(xo, i, x0, x1);
        if (ms->best) st2(xb, i, x0, x1);
    }
};

// textbook: after the Lanczos step, the rotations k-2 and k-1 act on the new column (epsilon, delta, gamma_bar), a fresh rotation
// annihilates beta_{k+1}; phi_bar follows the right-hand side
struct TbStepLogic {                 // red0 = (v_next, v_next)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; MinState* ms; long long k;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double alpha = st->alpha, beta = ms->beta;
        const double bn = dsqrt(red[0]);
        const double gbar = ms->c * alpha - ms->c_prev * ms->s * beta;
        const double delta = ms->s * alpha + ms->c_prev * ms->c * beta;
        const double epsilon = ms->s_prev * beta;
        const double gamma = dsqrt(gbar * gbar + bn * bn);              // not hypot: the host restatement must round the same way
        const double cn = gbar / gamma, sn = bn / gamma;
        ms->beta_next = bn; ms->delta = delta; ms->epsilon = epsilon; ms->rho = gamma; ms->coef = cn * ms->eta;
        ms->eta = -sn * ms->eta;
        ms->c_prev = ms->c; ms->c = cn; ms->s_prev = ms->s; ms->s = sn; ms->beta = bn;
        const double res = fabs(ms->eta);
        c.push(res);
        bool stop = c.check(res, ms->beta1, k);
        if (bn == 0.0) { st->converged = 1; stop = true; }              // the Krylov space is exhausted: x_k is exact
        st->iter = k;
        if (stop) { st->early = 1; c.finish(KRYST_OK); }                // this iteration's x update still runs
    }
};
struct TbUpdateOp {                  // v_next /= beta_{k+1} ; w_k = (v_k - epsilon w_{k-2} - delta w_{k-1}) / gamma ; x += c_k phi_bar_{k-1} w_k
    static constexpr int NQ = 0; static constexpr const char* TAG = "TbUpdate";
    const MinState* ms; const double* v; const double* w; const double* wp; double* vn; double* wn; double* x;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double bn = ms->beta_next, ga = ms->rho, cf = ms->coef, de = ms->delta, ep = ms->epsilon;
        const d2 nn = ld2(vn, i), vv = ld2(v, i), ww = ld2(w, i), pp = ld2(wp, i), xx = ld2(x, i);
        st2(vn, i, nn.a / bn, nn.b / bn);
        const double w0 = (vv.a - ep * pp.a - de * ww.a) / ga, w1 = (vv.b - ep * pp.b - de * ww.b) / ga;
        st2(wn, i, w0, w1);
        st2(x, i, xx.a + cf * w0, xx.b + cf * w1);
    }
};

struct MinresRun : SolverRun {
    bool textbook;
    MinresRun(kryst_vec_t b, kryst_vec_t x, const SolveIO& io_, bool tb) : SolverRun(b, x, io_), textbook(tb) {}
    double *V[3] = {nullptr, nullptr, nullptr}, *W[3] = {nullptr, nullptr, nullptr}, *r = nullptr, *xo = nullptr;
    MinState* ms = nullptr;
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        KR_TRY(common_begin(prm.max_iters + 2, textbook ? 7 : 8));
        pc = nullptr;                                                                             // minres.rs:61
        ms = reinterpret_cast<MinState*>(ctx->d_scal + 128);        // d_scal: DevState at 0, MinState at +128, red at +256 doubles
        for (int q = 0; q < 3; ++q) { KR_TRY(ws.vec(&V[q])); KR_TRY(ws.vec(&W[q])); }
        KR_TRY(ws.vec(&r));
        if (!textbook) KR_TRY(ws.vec(&xo));
        KR_TRY(residual_dot(a, bv->d, xw, r, V[2], nullptr));                                     // :66-70 (x0 enters r0 only)
        if (!textbook) KR_HIP(hipMemsetAsync(xw, 0, padded_bytes(n), ctx->s_main));               // x_best = x_out = 0 (:94-95, :84)
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, MinInitLogic{lc, ms})));
        return launch_ew(ctx, MinScaleOp{ms, r, V[1]}, n, done);                                  // :90
    }
    int32_t iterate(int64_t j) override {
        const DevState* st = ws.st;
        double *vp = V[(j - 1) % 3], *v = V[j % 3], *vn = V[(j + 1) % 3];
        double *wp = W[(j - 1) % 3], *w = W[j % 3], *wn = W[(j + 1) % 3];
        KR_TRY(launch_spmv(a, v, vn, 1, v, done));                                                // :127-128
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, MinAlphaLogic{lc})));
        KR_TRY(launch_ew(ctx, MinLanczosOp{st, ms, v, vp, vn}, n, done));                         // :129-134
        if (textbook) {
            KR_TRY((reduce_then<1>(ctx, nt, ws.red, TbStepLogic{lc, ms, j})));
            return launch_ew_gated(ctx, TbUpdateOp{ms, v, w, wp, vn, wn, xw}, n, GateStopAt{st, j});
        }
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, MinStepLogic{lc, ms, j})));
        return launch_ew_gated(ctx, MinUpdateOp{ms, j == 1 ? 1 : 0, v, w, wp, vn, wn, xo, xw}, n, GateStopAt{st, j});
    }
};

// =================================================================== QMR as written (a BiCGStab-type loop)
struct QmrDirOp {                    // j == 0: p = r, p_tld = r_tld (qmr.rs:107-109) ; else p = r + beta p, p_tld = r_tld + beta p_tld (:117-120)
    static constexpr int NQ = 0; static constexpr const char* TAG = "QmrDir";
    const DevState* st; int first; const double* r; const double* rt; double* p; double* pt;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const d2 rr = ld2(r, i), tt = ld2(rt, i);
        if (first) { st2(p, i, rr.a, rr.b); st2(pt, i, tt.a, tt.b); return; }
        const double be = st->beta;
        const d2 pp = ld2(p, i), qq = ld2(pt, i);
        st2(p, i, rr.a + be * pp.a, rr.b + be * pp.b);
        st2(pt, i, tt.a + be * qq.a, tt.b + be * qq.b);
    }
};
struct QmrSOp {                      // s = r - alpha v (qmr.rs:129-131)
    static constexpr int NQ = 0; static constexpr const char* TAG = "QmrS";
    const DevState* st; const double* r; const double* v; double* s;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = st->alpha;
        const d2 rr = ld2(r, i), vv = ld2(v, i);
        st2(s, i, rr.a - al * vv.a, rr.b - al * vv.b);
    }
};
struct QmrXrOp {                     // x = x + alpha p + omega s (qmr.rs:138-140) ; r = s - omega t (:142-144)
    static constexpr int NQ = 0; static constexpr const char* TAG = "QmrXr";
    const DevState* st; const double* p; const double* s; const double* t; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double al = st->alpha, om = st->omega;
        const d2 pp = ld2(p, i), ss = ld2(s, i), tt = ld2(t, i), xx = ld2(x, i);
        st2(x, i, xx.a + al * pp.a + om * ss.a, xx.b + al * pp.b + om * ss.b);
        st2(r, i, ss.a - om * tt.a, ss.b - om * tt.b);
    }
};
struct QmrResOp {                    // partials ||b - A x_j||^2 (qmr.rs:146-150; the vector itself is dead) and (r_tld, r) (:112)
    static constexpr int NQ = 2; static constexpr const char* TAG = "QmrRes"; static constexpr int BPC = 4;
    const double* b; const double* ax; const double* rt; const double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[2]) const {
        const d2 bb = ld2(b, i), aa = ld2(ax, i), tt = ld2(rt, i), rr = ld2(r, i);
        const double e0 = bb.a - aa.a, e1 = bb.b - aa.b;
        if (in0) { acc[0] = acc[0] + e0 * e0; acc[1] = acc[1] + tt.a * rr.a; }
        if (in1) { acc[0] = acc[0] + e1 * e1; acc[1] = acc[1] + tt.b * rr.b; }
    }
};
struct QmrInitLogic {                // qmr.rs:81-104 ; red0 = (r, r) = (r_tld, r)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double norm_r0 = dsqrt(red[0]);                           // :88
        st->res0 = norm_r0; st->rho = red[0];                           // :90
        st->iter = 0; st->iterations = 0; st->final_residual = norm_r0; st->converged = 0;   // :89
        if (st->rho == 0.0) { st->converged = 1; c.finish(KRYST_OK); return; }   // :91-96 (final_residual = ||r||)
        if (c.max_iters <= 0) c.finish(KRYST_OK);                       // :163-165 with an empty loop
    }
};
struct QmrSigmaLogic {               // qmr.rs:123-127 ; red0 = (p_tld, v)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double sigma = red[0];
        if (sigma == 0.0) { c.finish(KRYST_OK); return; }               // :124-126 break: the last check's stats, the previous res_norm
        st->alpha = st->rho / sigma;
    }
};
struct QmrOmegaLogic {               // qmr.rs:133-137 ; red0 = (s, t) = (t, s), red1 = (t, t)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const { c.st->omega = red[1] != 0.0 ? red[0] / red[1] : 0.0; }
};
struct QmrEndLogic {                 // qmr.rs:150-158, then the head of the next iteration :110-116 ; red0 = ||b - A x||^2, red1 = (r_tld, r)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; long long i;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double res_norm = dsqrt(red[0]);
        c.push(res_norm);                                               // addition: the reference keeps no history
        st->iter = i;
        if (c.check(res_norm, st->res0, i)) { st->converged = 1; c.finish(KRYST_OK); return; }   // :151-157
        st->rho_prev = st->rho; st->rho = red[1];                       // :111-112
        if (st->rho == 0.0) { c.finish(KRYST_OK); return; }             // :113-115
        st->beta = st->rho / st->rho_prev;                              // :116
    }
};

struct QmrRun : SolverRun {
    using SolverRun::SolverRun;
    double *r = nullptr, *rt = nullptr, *p = nullptr, *pt = nullptr, *v = nullptr, *s = nullptr, *t = nullptr;
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        KR_TRY(common_begin(prm.max_iters + 2, 7));
        pc = nullptr;                                                                             // qmr.rs:64
        KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&rt)); KR_TRY(ws.vec(&p)); KR_TRY(ws.vec(&pt)); KR_TRY(ws.vec(&v)); KR_TRY(ws.vec(&s));
        KR_TRY(ws.vec(&t));
        KR_TRY(residual_dot(a, bv->d, xw, r, v, nullptr));                                        // :81-85, :88
        KR_HIP(hipMemcpyAsync(rt, r, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));      // :87
        return reduce_then<1>(ctx, nt, ws.red, QmrInitLogic{lc});
    }
    int32_t iterate(int64_t i) override {
        const DevState* st = ws.st;
        KR_TRY(launch_ew(ctx, QmrDirOp{st, i == 1 ? 1 : 0, r, rt, p, pt}, n, done));               // :106-121
        KR_TRY(launch_spmv(a, p, v, 1, pt, done));                                                // :120 + (p_tld, v) :123
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, QmrSigmaLogic{lc})));
        KR_TRY(launch_ew(ctx, QmrSOp{st, r, v, s}, n, done));                                     // :129-131
        KR_TRY(launch_spmv(a, s, t, 2, s, done));                                                 // :133 + (t, s), (t, t) :134-135
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, QmrOmegaLogic{lc})));
        KR_TRY(launch_ew(ctx, QmrXrOp{st, p, s, t, xw, r}, n, done));                             // :138-144
        KR_TRY(launch_spmv(a, xw, t, 0, nullptr, done));                                          // :146 (t's storage: t is dead)
        KR_TRY(launch_ew(ctx, QmrResOp{bv->d, t, rt, r}, n, done));                               // :147-150 + the next rho :112
        return reduce_then<2>(ctx, nt, ws.red, QmrEndLogic{lc, i});
    }
};

// =================================================================== CGNR as written / textbook CGNR
// as written: ap = A p, at_ap = A ap, alpha = rz / (at_ap, at_ap), z = A r (cgnr.rs:90-105)
// textbook:   w  = A p,  alpha = rz / (w, w), z = A^T r (Saad, section 8.3)
struct CgnrXrOp {                    // x = x + alpha p (cgnr.rs:99-101) ; r = r - alpha ap (:102-104) ; partial (r, r) (:107)
    static constexpr int NQ = 1; static constexpr const char* TAG = "CgnrXr";
    const DevState* st; const double* p; const double* ap; double* x; double* r;
    __device__ __forceinline__ void pair(int64_t i, bool in0, bool in1, double (&acc)[1]) const {
        const double al = st->alpha;
        const d2 pp = ld2(p, i), aa = ld2(ap, i), xx = ld2(x, i), rr = ld2(r, i);
        st2(x, i, xx.a + al * pp.a, xx.b + al * pp.b);
        const double r0 = rr.a - al * aa.a, r1 = rr.b - al * aa.b;
        st2(r, i, r0, r1);
        if (in0) acc[0] = acc[0] + r0 * r0;
        if (in1) acc[0] = acc[0] + r1 * r1;
    }
};
struct CgnrPOp {                     // p = z + beta p (cgnr.rs:115-119)
    static constexpr int NQ = 0; static constexpr const char* TAG = "CgnrP";
    const DevState* st; const double* z; double* p;
    __device__ __forceinline__ void pair(int64_t i, bool, bool, double (&)[1]) const {
        const double be = st->beta;
        const d2 zz = ld2(z, i), pp = ld2(p, i);
        st2(p, i, zz.a + be * pp.a, zz.b + be * pp.b);
    }
};
struct CgnrRes0Logic {               // res0 = ||r|| (cgnr.rs:88-89) ; red0 = (r, r)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        st->res0 = dsqrt(red[0]);
        st->iter = 0; st->iterations = 0; st->final_residual = st->res0; st->converged = 0;
    }
};
struct CgnrInitLogic {               // rz = (z, z) (cgnr.rs:87) ; red1 = (z, z)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const {
        c.st->rz = red[1];
        if (c.max_iters <= 0) c.finish(KRYST_OK);                       // :129-131 with an empty loop
    }
};
struct CgnrAlphaLogic {              // alpha = rz / (at_ap, at_ap) (cgnr.rs:97) -- textbook: rz / (w, w) ; red1.  No guard, like the reference
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const { c.st->alpha = c.st->rz / red[1]; }
};
struct CgnrRsqLogic {                // keeps (r, r) for the end of the iteration
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c;
    __device__ void run(const double* red) const { c.st->rsq = red[0]; }
};
struct CgnrEndLogic {                // cgnr.rs:106-120 ; red1 = (z, z)
    static constexpr bool RUN_WHEN_DONE = false;
    LogicCtx c; long long i;
    __device__ void run(const double* red) const {
        DevState* st = c.st;
        const double rz_new = red[1];                                   // :106
        const double res_norm = dsqrt(st->rsq);                         // :107
        c.push(res_norm);                                               // addition: the reference keeps no history
        st->iter = i;
        if (c.check(res_norm, st->res0, i)) { c.finish(KRYST_OK); return; }   // :108-113
        st->beta = rz_new / st->rz;                                     // :115
        st->rz = rz_new;                                                // :120
    }
};

struct CgnrRun : SolverRun {
    bool textbook; kryst_csr_t az = nullptr;      // the operator of z = A^T r: A itself as written (cgnr.rs:84, :105), A^T in the textbook form
    CgnrRun(kryst_vec_t b, kryst_vec_t x, const SolveIO& io_, bool tb) : SolverRun(b, x, io_), textbook(tb) {}
    double *r = nullptr, *z = nullptr, *p = nullptr, *ap = nullptr, *atap = nullptr;
    int32_t begin() override {
        KR_TRY(solve_args_check(io, bv, xv));
        az = a;
        if (textbook) KR_TRY(csr_transpose_operator(a, &az));
        KR_TRY(common_begin(prm.max_iters + 2, textbook ? 4 : 5));
        pc = nullptr;                                                                             // cgnr.rs:78
        KR_TRY(ws.vec(&r)); KR_TRY(ws.vec(&z)); KR_TRY(ws.vec(&p)); KR_TRY(ws.vec(&ap));
        if (!textbook) KR_TRY(ws.vec(&atap));
        KR_TRY(residual_dot(a, bv->d, xw, r, z, nullptr));                                        // :81-86, :88
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgnrRes0Logic{lc})));
        KR_TRY(launch_spmv(az, r, z, 2, r, done));                                                // :84, :87
        KR_HIP(hipMemcpyAsync(p, z, padded_bytes(n), hipMemcpyDeviceToDevice, ctx->s_main));       // :86
        return reduce_then<2>(ctx, nt, ws.red, CgnrInitLogic{lc});
    }
    int32_t iterate(int64_t i) override {
        const DevState* st = ws.st;
        if (textbook) KR_TRY(launch_spmv(a, p, ap, 2, p, done));                                  // w = A p, (w, w)
        else {
            KR_TRY(launch_spmv(a, p, ap, 0, nullptr, done));                                       // :92-93
            KR_TRY(launch_spmv(a, ap, atap, 2, ap, done));                                         // :95-96 + (at_ap, at_ap) :97
        }
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, CgnrAlphaLogic{lc})));
        KR_TRY(launch_ew(ctx, CgnrXrOp{st, p, ap, xw, r}, n, done));                              // :99-104, (r, r) :107
        KR_TRY((reduce_then<1>(ctx, nt, ws.red, CgnrRsqLogic{lc})));
        KR_TRY(launch_spmv(az, r, z, 2, r, done));                                                // :105-106
        KR_TRY((reduce_then<2>(ctx, nt, ws.red, CgnrEndLogic{lc, i})));
        return launch_ew(ctx, CgnrPOp{st, z, p}, n, done);                                        // :115-120
    }
};

SolverRun* make_minres_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io, bool textbook) { return new MinresRun(b, x, io, textbook); }
SolverRun* make_qmr_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io) { return new QmrRun(b, x, io); }
SolverRun* make_cgnr_run(kryst_vec_t b, kryst_vec_t x, const SolveIO& io, bool textbook) { return new CgnrRun(b, x, io, textbook); }

int32_t minres_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool textbook) {
    KR_ARG(io.a && io.params, "solve: null argument");
    MinresRun run(bv, xv, io, textbook);
    return run.solve();
}
int32_t qmr_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io) {
    KR_ARG(io.a && io.params, "solve: null argument");
    QmrRun run(bv, xv, io);
    return run.solve();
}
int32_t cgnr_solve(kryst_vec_t bv, kryst_vec_t xv, const SolveIO& io, bool textbook) {
    KR_ARG(io.a && io.params, "solve: null argument");
    CgnrRun run(bv, xv, io, textbook);
    return run.solve();
}

}  // namespace kr
