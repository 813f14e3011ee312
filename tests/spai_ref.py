"""numpy restatement of the SPAI set-up (ApproxInv::setup, src/preconditioner/approxinv.rs:123-264; kryst_amd/csrc/spai.hip; DESIGN.md
section 4.6).

Column j of M: the pattern J_j sorted ascending, I_j = the sorted union of the stored rows of the columns J_j of A, and m_j =
argmin || A[I_j, J_j] m - e_j|I_j ||_2 by np.linalg.lstsq (the reduced problem: the rows of A[:, J_j] outside I_j are zero, so the
minimiser is that of the reference's full n-row problem).  inv_rows[i] = the (j, M_ij) with |M_ij| > tol (strict), ascending j, returned
as CSR arrays.  The device solves the same problem by Householder QR, so its values agree with these to rounding, not bit for bit."""
import numpy as np


def csc(rp, ci, va, n):
    """A's columns: (col_ptr, rows, vals), rows ascending within each column."""
    rp = np.asarray(rp, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    order = np.argsort(ci, kind="stable")                       # CSR rows come ascending, a stable sort keeps them so
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=cp[1:])
    return cp, rows[order], np.asarray(va, dtype=np.float64)[order]


def column_lists(cp, cr, cv):
    """col(k) -> (rows, vals) of column k of A."""
    return lambda k: (cr[cp[k]:cp[k + 1]], cv[cp[k]:cp[k + 1]])


def reduced_problem(j, J, col):
    """(J sorted, I_j, A[I_j, J_j] dense, e_j restricted to I_j)."""
    J = np.sort(np.asarray(J, dtype=np.int64))
    lists = [col(int(k)) for k in J]
    I = np.unique(np.concatenate([r for r, _ in lists])) if lists else np.zeros(0, dtype=np.int64)
    Ah = np.zeros((len(I), len(J)))
    for q, (r, v) in enumerate(lists):
        Ah[np.searchsorted(I, r), q] = v
    e = (I == j).astype(np.float64)
    return J, I, Ah, e


def solve_column(Ah, e):
    if Ah.shape[1] == 0:
        return np.zeros(0)
    return np.linalg.lstsq(Ah, e, rcond=None)[0]


def columns(n, col, pptr, pidx, cols=None):
    """{j: (J_j sorted, m_j)} for the columns `cols` (all when None); pattern column j = pidx[pptr[j]:pptr[j+1]]."""
    out = {}
    for j in (range(n) if cols is None else cols):
        J, I, Ah, e = reduced_problem(int(j), pidx[pptr[j]:pptr[j + 1]], col)
        out[int(j)] = (J, solve_column(Ah, e))
    return out


def to_csr(n, cols, tol):
    """inv_rows as CSR (row_ptr, col, val): the entries |M_ij| > tol of the columns, ascending j inside each row."""
    ii, jj, vv = [], [], []
    for j, (J, m) in cols.items():
        keep = np.abs(m) > tol
        ii.append(J[keep]); jj.append(np.full(int(keep.sum()), j, dtype=np.int64)); vv.append(m[keep])
    ii = np.concatenate(ii) if ii else np.zeros(0, dtype=np.int64)
    jj = np.concatenate(jj) if jj else np.zeros(0, dtype=np.int64)
    vv = np.concatenate(vv) if vv else np.zeros(0)
    order = np.lexsort((jj, ii))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ii, minlength=n), out=rp[1:])
    return rp, jj[order], vv[order]


def setup(a, pptr, pidx, tol):
    """The whole set-up on an oracle.Csr `a` -> (row_ptr, col, val) of M and the per-column solutions."""
    col = column_lists(*csc(a.row_ptr, a.col_idx, a.vals, a.nrows))
    cols = columns(a.nrows, col, np.asarray(pptr, dtype=np.int64), np.asarray(pidx, dtype=np.int64))
    return to_csr(a.nrows, cols, tol), cols


def manual_ptr_idx(pat):
    ptr = np.zeros(len(pat) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in pat], out=ptr[1:])
    idx = np.concatenate([np.asarray(c, dtype=np.int64) for c in pat]) if pat else np.zeros(0, dtype=np.int64)
    return ptr, idx
