// AMG::new as written (src/preconditioner/amg.rs:73-118), on the host.  The reference builds every level on dense faer matrices; this
// restatement keeps the rows sparse and gives the dense loops' values: a dense row loop adds only exact zeros (x + 0 = x) where a row
// stores nothing, so summing the stored entries in the dense loop's order (ascending column; fine row-major for the coarse graph)
// gives the same bits.  The set-up is a sequential greedy pass whose coarse levels fill in, so it runs here and the hierarchy is
// uploaded (amg.hip); kryst_host_amg exposes it without a device.
#include "common.h"
#include "amg.h"
#include <algorithm>
#include <cmath>
#include <numeric>

namespace kr {

namespace {

double diag_of(const HostCsr& a, int64_t i) {
    for (int64_t k = a.ptr[i]; k < a.ptr[i + 1]; ++k)
        if (a.col[k] == i) return a.val[k];
    return 0.0;
}

// compute_anisotropy + compute_adaptive_threshold (:447-498)
double adaptive_threshold(const HostCsr& a, double base) {
    const int64_t n = a.nrows;
    if (n == 0) return base * (1.0 + std::max(1.0, 0.5));
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double mx = 0.0, d = 0.0;
        for (int64_t k = a.ptr[i]; k < a.ptr[i + 1]; ++k) {
            if (a.col[k] == i) { d = a.val[k]; continue; }
            mx = std::fmax(mx, std::fabs(a.val[k]));              // fold(0.0, f64::max)
        }
        sum += (std::fabs(d) > 1e-14) ? mx / std::fabs(d) : 0.0;
    }
    const double avg = sum / (double)n;
    return base * (1.0 + std::fmax(avg, 0.5));
}

// compute_strength_matrix (:605-658): S_ij = |a_ij| / sqrt(|a_ii| |a_jj|) where both diagonals exceed 1e-14 and S_ij > threshold.
// Entries the reference stores as 0.0 (the diagonal, weak pairs) are left out: pairwise aggregation needs a strength > 0.0 (:719-727)
// and the coarse graph skips zeros (:764), so they change nothing.
HostCsr strength(const HostCsr& a, double threshold) {
    const int64_t n = a.nrows;
    std::vector<double> ad(n);
    for (int64_t i = 0; i < n; ++i) ad[i] = std::fabs(diag_of(a, i));
    HostCsr s; s.nrows = s.ncols = n; s.ptr.assign(n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t k = a.ptr[i]; k < a.ptr[i + 1]; ++k) {
            const int64_t j = a.col[k];
            if (j == i) continue;
            if (ad[i] > 1e-14 && ad[j] > 1e-14) {
                const double st = std::fabs(a.val[k]) / std::sqrt(ad[i] * ad[j]);
                if (st > threshold && st != 0.0) { s.col.push_back((int32_t)j); s.val.push_back(st); }
            }
        }
        s.ptr[i + 1] = s.nnz();
    }
    return s;
}

// pairwise_aggregation (:707-747): the first strictly strongest unvisited neighbour in column order, else a singleton
std::vector<int64_t> pairwise(const HostCsr& s) {
    const int64_t n = s.nrows;
    std::vector<int64_t> agg(n, -1);
    std::vector<char> visited(n, 0);
    int64_t id = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (visited[i]) continue;
        double best = 0.0; int64_t nb = -1;
        for (int64_t k = s.ptr[i]; k < s.ptr[i + 1]; ++k) {
            const int64_t j = s.col[k];
            if (j != i && !visited[j] && s.val[k] > best) { best = s.val[k]; nb = j; }
        }
        agg[i] = id; visited[i] = 1;
        if (nb >= 0) { agg[nb] = id; visited[nb] = 1; }
        ++id;
    }
    return agg;
}

// build_coarse_graph (:752-771): coarse[agg_i][agg_j] += s_ij over the fine entries in row-major order
HostCsr coarse_graph(const HostCsr& s, const std::vector<int64_t>& agg) {
    int64_t nc = 0;
    for (int64_t v : agg) nc = std::max(nc, v + 1);
    struct T { int64_t r, c, seq; double v; };
    std::vector<T> t;
    t.reserve((size_t)s.nnz());
    for (int64_t i = 0; i < s.nrows; ++i)
        for (int64_t k = s.ptr[i]; k < s.ptr[i + 1]; ++k)
            t.push_back({agg[i], agg[s.col[k]], (int64_t)t.size(), s.val[k]});
    std::stable_sort(t.begin(), t.end(), [](const T& x, const T& y) { return x.r != y.r ? x.r < y.r : x.c < y.c; });
    HostCsr g; g.nrows = g.ncols = nc; g.ptr.assign(nc + 1, 0);
    for (size_t q = 0; q < t.size();) {
        size_t e = q;
        double sum = 0.0;
        while (e < t.size() && t[e].r == t[q].r && t[e].c == t[q].c) { sum += t[e].v; ++e; }   // the row-major (seq) order survives the stable sort
        g.col.push_back((int32_t)t[q].c); g.val.push_back(sum); g.ptr[t[q].r + 1]++;
        q = e;
    }
    for (int64_t i = 0; i < nc; ++i) g.ptr[i + 1] += g.ptr[i];
    return g;
}

// one sparse accumulator row: acc[c] over the touched columns, handed out in ascending column order
struct Spa {
    std::vector<double> acc; std::vector<char> on; std::vector<int32_t> cols;
    explicit Spa(int64_t n) : acc(n, 0.0), on(n, 0) {}
    void add(int32_t c, double v) {
        if (!on[c]) { on[c] = 1; acc[c] = 0.0; cols.push_back(c); }
        acc[c] += v;
    }
    void flush(HostCsr& out) {
        std::sort(cols.begin(), cols.end());
        for (int32_t c : cols) { out.col.push_back(c); out.val.push_back(acc[c]); on[c] = 0; }
        cols.clear();
        out.ptr.push_back(out.nnz());
    }
};

std::vector<double> diag_inverse(const HostCsr& a) {       // extract_diagonal_inverse (:139-170)
    std::vector<double> d(a.nrows);
    for (int64_t i = 0; i < a.nrows; ++i) {
        const double v = diag_of(a, i);
        d[i] = std::fabs(v) < 1e-14 ? 0.0 : 1.0 / v;
    }
    return d;
}

}  // namespace

int32_t amg_setup_as_written(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t max_levels,
                             double base_threshold, int64_t level_budget, std::vector<AmgHostLevel>& levels) {
    KR_ARG(n >= 0 && (n == 0 || (row_ptr && col && val)), "amg: null rows");
    KR_ARG(max_levels >= 0, "amg: max_levels < 0");
    KR_ARG(row_ptr[0] == 0, "amg: row_ptr[0] != 0");
    HostCsr cur; cur.nrows = cur.ncols = n; cur.ptr.assign(row_ptr, row_ptr + n + 1);
    for (int64_t i = 0; i < n; ++i) {
        KR_ARG(row_ptr[i + 1] >= row_ptr[i], "amg: row_ptr not monotone");
        for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            KR_ARG(col[k] >= 0 && col[k] < n, "amg: column out of range (the operator must be square)");
            KR_ARG(k == row_ptr[i] || col[k] > col[k - 1], "amg: columns of a row must be strictly ascending");
        }
    }
    cur.col.assign(col, col + row_ptr[n]); cur.val.assign(val, val + row_ptr[n]);
    const int64_t budget = level_budget > 0 ? level_budget : std::max<int64_t>(KR_AMG_FILL_FACTOR * cur.nnz(), KR_AMG_FILL_MIN);
    levels.clear();
    std::vector<double> cur_dinv = diag_inverse(cur);
    for (int32_t lv = 0; lv < max_levels; ++lv) {
        const int64_t nl = cur.nrows;
        if (nl <= 10) break;                                                                   // :79-81
        AmgHostLevel L;
        L.threshold = adaptive_threshold(cur, base_threshold);                                 // :83
        // generate_operators (:123-137) with double_pairwise = true (:664-674)
        const HostCsr s = strength(cur, L.threshold);
        const std::vector<int64_t> first = pairwise(s);
        const std::vector<int64_t> second = pairwise(coarse_graph(s, first));
        L.agg.resize(nl);
        int64_t nc = 0;
        for (int64_t i = 0; i < nl; ++i) { L.agg[i] = (int32_t)second[first[i]]; nc = std::max<int64_t>(nc, L.agg[i] + 1); }   // remap_aggregates
        // construct_prolongation (:794-818) P0[i][agg_i] = 1, smooth_interpolation(P, A, 0.5) (:502-525): P[i][j] -= 0.5 a_ij for
        // j < min(nc, n) -- the first nc COLUMNS of A, whatever they are -- then minimize_energy (:529-565): every row scaled to unit norm
        HostCsr p; p.nrows = nl; p.ncols = nc; p.ptr.assign(1, 0);
        for (int64_t i = 0; i < nl; ++i) {
            const int64_t g = L.agg[i];
            const int64_t beg = p.nnz();
            bool put = false;
            for (int64_t k = cur.ptr[i]; k < cur.ptr[i + 1] && cur.col[k] < nc; ++k) {
                const int64_t j = cur.col[k];
                if (!put && g < j) { p.col.push_back((int32_t)g); p.val.push_back(1.0); put = true; }
                const double p0 = (j == g) ? 1.0 : 0.0;
                if (j == g) put = true;
                p.col.push_back((int32_t)j); p.val.push_back(p0 - 0.5 * cur.val[k]);
            }
            if (!put) { p.col.push_back((int32_t)g); p.val.push_back(1.0); }
            double ss = 0.0;
            for (int64_t k = beg; k < p.nnz(); ++k) ss += p.val[k] * p.val[k];
            const double nf = std::fabs(ss) > 1e-14 ? std::sqrt(ss) : 1.0;
            for (int64_t k = beg; k < p.nnz(); ++k) p.val[k] /= nf;
            p.ptr.push_back(p.nnz());
            if (p.nnz() > budget) { set_error("amg: level %d: P exceeds the fill budget of %lld entries", (int)lv + 1, (long long)budget); return KRYST_FACTOR_ERROR; }
        }
        // R = P0^T (:135, transposed before the smoothing): row g lists the rows of aggregate g, ascending
        HostCsr r; r.nrows = nc; r.ncols = nl; r.ptr.assign(nc + 1, 0);
        for (int64_t i = 0; i < nl; ++i) r.ptr[L.agg[i] + 1]++;
        for (int64_t g = 0; g < nc; ++g) r.ptr[g + 1] += r.ptr[g];
        r.col.resize(nl); r.val.assign(nl, 1.0);
        {
            std::vector<int64_t> fill(r.ptr.begin(), r.ptr.end() - 1);
            for (int64_t i = 0; i < nl; ++i) r.col[fill[L.agg[i]]++] = (int32_t)i;
        }
        // coarse_matrix = (R * A) * P (:94): entry sums in ascending inner index, from 0.0
        HostCsr ra; ra.nrows = nc; ra.ncols = nl; ra.ptr.assign(1, 0);
        Spa spa(std::max(nl, nc));
        for (int64_t g = 0; g < nc; ++g) {
            for (int64_t q = r.ptr[g]; q < r.ptr[g + 1]; ++q) {
                const int64_t i = r.col[q];
                for (int64_t k = cur.ptr[i]; k < cur.ptr[i + 1]; ++k) spa.add(cur.col[k], r.val[q] * cur.val[k]);
            }
            spa.flush(ra);
            if (ra.nnz() > budget) { set_error("amg: level %d: R*A exceeds the fill budget of %lld entries", (int)lv + 1, (long long)budget); return KRYST_FACTOR_ERROR; }
        }
        HostCsr ac; ac.nrows = ac.ncols = nc; ac.ptr.assign(1, 0);
        for (int64_t g = 0; g < nc; ++g) {
            for (int64_t q = ra.ptr[g]; q < ra.ptr[g + 1]; ++q) {
                const int64_t j = ra.col[q];
                for (int64_t k = p.ptr[j]; k < p.ptr[j + 1]; ++k) spa.add(p.col[k], ra.val[q] * p.val[k]);
            }
            spa.flush(ac);
            if (ac.nnz() > budget) { set_error("amg: level %d: A_c exceeds the fill budget of %lld entries", (int)lv + 1, (long long)budget); return KRYST_FACTOR_ERROR; }
        }
        L.a = std::move(cur); L.p = std::move(p); L.r = std::move(r); L.dinv = std::move(cur_dinv);   // :96-101
        levels.push_back(std::move(L));
        cur = std::move(ac);
        cur_dinv = diag_inverse(cur);
    }
    AmgHostLevel last;                                                                         // :106-112
    last.a = std::move(cur); last.dinv = std::move(cur_dinv);
    levels.push_back(std::move(last));
    return KRYST_OK;
}

}  // namespace kr

using namespace kr;

struct kryst_host_amg_s { std::vector<AmgHostLevel> levels; };

extern "C" {

int32_t kryst_host_amg(int64_t n, const int64_t* row_ptr, const int32_t* col, const double* val, int32_t max_levels, double threshold,
                       int64_t level_budget, kryst_host_amg_t* out) {
    KR_ARG(out && row_ptr, "host_amg");
    *out = nullptr;
    kryst_host_amg_s* h = new kryst_host_amg_s();
    const int32_t rc = amg_setup_as_written(n, row_ptr, col, val, max_levels, threshold, level_budget, h->levels);
    if (rc != KRYST_OK) { delete h; return rc; }
    *out = h;
    return KRYST_OK;
}

int32_t kryst_host_amg_levels(kryst_host_amg_t h, int32_t* nlevels) {
    KR_ARG(h && nlevels, "host_amg_levels");
    *nlevels = (int32_t)h->levels.size();
    return KRYST_OK;
}

int32_t kryst_host_amg_get(kryst_host_amg_t h, int32_t level, int32_t which, int64_t* nrows, int64_t* ncols, int64_t* nnz, int64_t* row_ptr,
                           int32_t* col, double* val) {
    KR_ARG(h && level >= 0 && level < (int32_t)h->levels.size(), "host_amg_get: level out of range");
    KR_ARG(which >= 0 && which <= 4, "host_amg_get: which must be 0 (A), 1 (P), 2 (R), 3 (D^-1) or 4 (aggregates)");
    const AmgHostLevel& L = h->levels[level];
    if (which == 3 || which == 4) {
        const int64_t m = which == 3 ? (int64_t)L.dinv.size() : (int64_t)L.agg.size();
        if (nrows) *nrows = m;
        if (ncols) *ncols = 1;
        if (nnz) *nnz = m;
        if (which == 3 && val) std::copy(L.dinv.begin(), L.dinv.end(), val);
        if (which == 4 && col) std::copy(L.agg.begin(), L.agg.end(), col);
        return KRYST_OK;
    }
    const HostCsr& m = which == 0 ? L.a : which == 1 ? L.p : L.r;
    if (nrows) *nrows = m.nrows;
    if (ncols) *ncols = m.ncols;
    if (nnz) *nnz = m.nnz();
    if (row_ptr) std::copy(m.ptr.begin(), m.ptr.end(), row_ptr);
    if (col) std::copy(m.col.begin(), m.col.end(), col);
    if (val) std::copy(m.val.begin(), m.val.end(), val);
    return KRYST_OK;
}

int32_t kryst_host_amg_destroy(kryst_host_amg_t h) {
    delete h;
    return KRYST_OK;
}

}  // extern "C"
