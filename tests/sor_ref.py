"""Restatements of Sor (src/preconditioner/sor.rs:106-170) and of the colouring utility (src/utils/coloring.rs), for the tests of
kryst_amd/csrc/sor.hip:

  (a) setup / apply_loop      the two dense loops literally as written, on Python floats (IEEE double, every operation rounded on its own)
  (b) Plan                    the same sweeps one dependency level at a time in numpy, the terms of a row in the order of (a): the stored
                              entries before the row in the sweep order by ascending position, then those after it; for operators too
                              large for (a).  Takes the coloured order too.
  (c) color_graph, ...        extract_adjacency / distance2_neighbors / greedy_distance2_coloring / build_blocks_from_colors as written
  (d) apply_permuted          the coloured order by definition: (a) on the explicitly permuted dense matrix, un-permuted
"""
import numpy as np

ZERO_INITIAL_GUESS, APPLY_LOWER, APPLY_UPPER, SYMMETRIC_SWEEP = 1, 2, 4, 6
LOCAL_FORWARD_SWEEP, LOCAL_BACKWARD_SWEEP, LOCAL_SYMMETRIC_SWEEP, EISENSTAT = 8, 16, 24, 32


class ZeroPivot(Exception):
    def __init__(self, row):
        super().__init__(f"ZeroPivot({row})")
        self.row = row


def dense(a):
    """the dense matrix a[(i, j)] of an oracle Csr (or anything with nrows, row_ptr, col_idx, vals): +0.0 where nothing is stored"""
    d = np.zeros((a.nrows, a.nrows))
    for i in range(a.nrows):
        d[i, a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]]] = a.vals[a.row_ptr[i]:a.row_ptr[i + 1]]
    return d


def setup(d, fshift=0.0):
    """sor.rs:106-118 on a dense matrix -> inv_diag; raises ZeroPivot(i) at the first row whose a_ii + fshift is zero"""
    n = len(d)
    inv = np.zeros(n)
    for i in range(n):
        aii = float(d[i, i]) + float(fshift)
        if aii == 0.0:
            raise ZeroPivot(i)
        inv[i] = 1.0 / aii
    return inv


def apply_loop(d, inv_diag, x, omega=1.0, its=1, sym=APPLY_LOWER):
    """sor.rs:124-170, line for line"""
    a = [[float(v) for v in row] for row in np.asarray(d)]
    inv = [float(v) for v in inv_diag]
    x = [float(v) for v in x]
    omega = float(omega)
    n = len(x)
    y = [0.0] * n
    for _ in range(its):
        if sym & APPLY_LOWER:
            for i in range(n):
                sigma = 0.0
                for j in range(i):
                    sigma = sigma + a[i][j] * y[j]
                if not sym & EISENSTAT:
                    for j in range(i + 1, n):
                        sigma = sigma + a[i][j] * x[j]
                xi = x[i]
                yi = (xi - sigma) * inv[i]
                y[i] = yi
        if sym & APPLY_UPPER:
            for ii in range(n - 1, -1, -1):
                sigma = 0.0
                for j in range(ii + 1, n):
                    sigma = sigma + a[ii][j] * y[j]
                if not sym & EISENSTAT:
                    for j in range(ii):
                        sigma = sigma + a[ii][j] * y[j]
                xi = x[ii]
                yi = (xi - sigma) * inv[ii]
                y[ii] = (1.0 - omega) * xi + omega * yi
    return np.array(y)


# ------------------------------------------------------------------------------------------------ (d) the coloured order
def order_of(colors):
    """rows by (colors[i], i) ascending"""
    return np.argsort(np.asarray(colors, dtype=np.int64), kind="stable")


def apply_permuted(d, x, colors, omega=1.0, its=1, sym=APPLY_LOWER, fshift=0.0):
    """the sweeps in the coloured order, by definition: (a) on P A P^T with P x, un-permuted"""
    o = order_of(colors)
    dp = np.asarray(d)[np.ix_(o, o)]
    yp = apply_loop(dp, setup(dp, fshift), np.asarray(x, dtype=float)[o], omega, its, sym)
    y = np.zeros(len(x))
    y[o] = yp
    return y


# ------------------------------------------------------------------------------------------------ (b) level by level
def _levels(n, ptr, col, forward):
    """lvl[p] = 1 + the highest level among the positions p depends on (strictly lower forward, strictly upper backward)"""
    lvl = [0] * n
    ptr = [int(v) for v in ptr]
    col = [int(v) for v in col]
    for p in (range(n) if forward else range(n - 1, -1, -1)):
        l = 0
        for k in range(ptr[p], ptr[p + 1]):
            v = lvl[col[k]] + 1
            if v > l:
                l = v
        lvl[p] = l
    return np.array(lvl, dtype=np.int64)


class Plan:
    """The sweeps of Sor on a CSR operator (row_ptr, col_idx ascending inside a row, vals), one dependency level at a time.  Per direction:
    the terms of every row in summation order as padded arrays (column, value, whether the operand is x), and the rows grouped by level of
    the sweep-order dependency graph (a backward sweep that reads old values makes their rows wait).  A row's operands from y are final
    (lower level) or untouched (higher level) when its level runs, so a level is one vectorised pass: sigma = +0.0, then term after term sigma = sigma + value * operand, each rounded on its own."""

    def __init__(self, a, fshift=0.0, colors=None, eisenstat=False):
        n = a.nrows
        rp = np.asarray(a.row_ptr, dtype=np.int64)
        ci = np.asarray(a.col_idx, dtype=np.int64)
        va = np.asarray(a.vals, dtype=float)
        self.n = n
        rows = np.repeat(np.arange(n), np.diff(rp))
        diag = np.zeros(n)
        on = ci == rows
        diag[rows[on]] = va[on]
        s = diag + float(fshift)
        if np.any(s == 0.0):
            raise ZeroPivot(int(np.flatnonzero(s == 0.0)[0]))
        self.inv = 1.0 / s
        order = order_of(colors) if colors is not None else np.arange(n)
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        before = pos[ci] < pos[rows]
        after = pos[ci] > pos[rows]
        self.dirs = {}
        for forward in (True, False):
            first, second = (before, after) if forward else (after, before)
            # summation order: the `first` entries in ascending position (= stored order when uncoloured), then the `second` ones
            sel = [np.flatnonzero(first)] + ([] if eisenstat else [np.flatnonzero(second)])
            grp = np.concatenate([np.full(len(e), g) for g, e in enumerate(sel)])
            ent = np.concatenate(sel)
            key = np.lexsort((pos[ci[ent]], grp, rows[ent]))      # by row, then group, then position in the sweep order
            ent, grp = ent[key], grp[key]
            r = rows[ent]
            cnt = np.bincount(r, minlength=n)
            start = np.concatenate([[0], np.cumsum(cnt)])
            slot = np.arange(len(ent)) - start[r]
            w = int(cnt.max()) if n else 0
            tc = np.zeros((n, w), dtype=np.int64); tv = np.zeros((n, w)); tm = np.zeros((n, w), dtype=bool); tx = np.zeros((n, w), dtype=bool)
            tc[r, slot] = ci[ent]; tv[r, slot] = va[ent]; tm[r, slot] = True
            tx[r, slot] = (grp == 1) if forward else False       # forward: the rows not yet visited contribute x, not y
            # dependency levels in sweep-order positions: a row waits for the `first` rows it reads; in a backward sweep that also reads
            # the OLD y of the rows before it, those rows wait for this one too (with a symmetric pattern they do anyway)
            wp, wq = pos[rows[first]], pos[ci[first]]
            if not forward and not eisenstat:
                wp, wq = np.concatenate([wp, pos[ci[second]]]), np.concatenate([wq, pos[rows[second]]])
            dk = np.argsort(wp, kind="stable")
            dptr = np.concatenate([[0], np.cumsum(np.bincount(wp, minlength=n))])
            lvl_pos = _levels(n, dptr, wq[dk], forward)
            lvl = lvl_pos[pos]                                     # per row
            by = np.lexsort((pos, lvl))
            off = np.concatenate([[0], np.cumsum(np.bincount(lvl, minlength=(int(lvl.max()) + 1 if n else 0)))])
            self.dirs[forward] = (tc, tv, tm, tx, by, off)

    def passes(self, forward):
        return len(self.dirs[forward][5]) - 1

    def sweep(self, forward, x, y, omega):
        tc, tv, tm, tx, by, off = self.dirs[forward]
        for g in range(len(off) - 1):
            R = by[off[g]:off[g + 1]]
            sigma = np.zeros(len(R))
            for t in range(tc.shape[1]):
                m = tm[R, t]
                if not m.any():
                    continue
                c = tc[R, t]
                op = np.where(tx[R, t], x[c], y[c])
                sigma = np.where(m, sigma + tv[R, t] * op, sigma)
            yi = (x[R] - sigma) * self.inv[R]
            y[R] = yi if forward else (1.0 - omega) * x[R] + omega * yi

    def apply(self, x, omega=1.0, its=1, sym=APPLY_LOWER):
        """y = M^-1 x.  The plan was built with or without EISENSTAT; `sym` picks the sweeps."""
        x = np.asarray(x, dtype=float)
        y = np.zeros(self.n)
        omega = float(omega)
        with np.errstate(all="ignore"):
            for _ in range(its):
                if sym & APPLY_LOWER:
                    self.sweep(True, x, y, omega)
                if sym & APPLY_UPPER:
                    self.sweep(False, x, y, omega)
        return y


def apply_levels(a, x, omega=1.0, its=1, sym=APPLY_LOWER, fshift=0.0, colors=None):
    return Plan(a, fshift, colors, bool(sym & EISENSTAT)).apply(x, omega, its, sym)


# ------------------------------------------------------------------------------------------------ (c) coloring.rs as written
def extract_adjacency(n, is_nz):
    adj = [[] for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i != j and (is_nz(i, j) or is_nz(j, i)):
                adj[i].append(j)
    return adj


def distance2_neighbors(adj):
    dist2 = [set() for _ in adj]
    for i in range(len(adj)):
        for j in adj[i]:
            dist2[i].add(j)
            for k in adj[j]:
                dist2[i].add(k)
        dist2[i].add(i)
    return dist2


def greedy_distance2_coloring(dist2):
    n = len(dist2)
    color_of = [None] * n
    for i in range(n):
        banned = {color_of[k] for k in dist2[i] if color_of[k] is not None}
        c = 0
        while c in banned:
            c += 1
        color_of[i] = c
    return color_of


def color_graph(n, is_nz):
    return greedy_distance2_coloring(distance2_neighbors(extract_adjacency(n, is_nz)))


def color_graph_csr(a):
    """color_graph with is_nz = "the entry is stored" """
    stored = np.zeros((a.nrows, a.nrows), dtype=bool)
    for i in range(a.nrows):
        stored[i, a.col_idx[a.row_ptr[i]:a.row_ptr[i + 1]]] = True
    return np.array(color_graph(a.nrows, lambda i, j: bool(stored[i, j])), dtype=np.int64)


def build_blocks_from_colors(colors):
    num_colors = (max(colors) + 1) if len(colors) else 0
    blocks = [[] for _ in range(num_colors)]
    for i, c in enumerate(colors):
        blocks[c].append(i)
    return blocks
