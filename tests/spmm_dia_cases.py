"""Operators, columns and the host restatement for the multiple-right-hand-side tests on the diagonal (CSR-DIA) encoding, shared by the CPU tier
(test_spmm_dia_cpu.py: the fixtures and the restatement, on the oracle alone) and the GPU tier (test_gpu_spmm_dia.py: spmm_dia_kernel against
kryst_spmv and the oracle, bit for bit).  The builders are those of mixed_dia_cases.py, mixed_pattern_cases.py and multi_rhs_cases.py.

The multivector tile is 512 rows, lane t owns rows 2t and 2t+1, and a multivector of n rows has mvec_rows(n) = ceil(n / 512) * 512 + 512
allocated rows.  Everything here is numpy and the oracle; nothing touches the device."""
import functools

import numpy as np

from oracle import oracle as O
import mixed_dia_cases as D
import multi_rhs_cases as MC

TILE = 512
WIDTHS = MC.WIDTHS

OPERATORS = {**D.OPERATORS, **{f"tridiag{n}": functools.partial(D.tridiag, n) for n in (511, 512, 513)}}
DIAGONALS = {**D.DIAGONALS, "tridiag511": 3, "tridiag512": 3, "tridiag513": 3}
# created under KRYST_SPMV_DIA=2: with few distinct values they take a more compact form by default and keep no streams
CONSTANT_COEFFICIENTS = ("five_point", "nine_point", "box27")
# operators whose rows leave out entries in the interior, and the elements of x that nothing reads any more
HOLES = {"tridiag_holes": D.TRIDIAG_HOLES, "varcoef12_holes": D.VARCOEF_HOLES}
SOLVE_OPERATORS = D.SOLVE_OPERATORS


@functools.lru_cache(maxsize=None)
def operator(name):
    return (OPERATORS.get(name) or SOLVE_OPERATORS[name])()


def mvec_rows(n):
    return -(-n // TILE) * TILE + TILE


def clamped_tiles(a):
    """the 512-row tiles whose lowest diagonal would start before X's row 0: they clamp each operand row on its own"""
    lo = D.dia_min_max(a)[0]
    return [q for q in range(-(-a.nrows // TILE)) if q * TILE + lo < 0]


def rows_pointing_beyond(a):
    """rows with an (absent) entry whose column lies at or beyond the allocated rows of X"""
    idx = np.arange(a.nrows)
    return idx[idx + D.dia_min_max(a)[1] >= mvec_rows(a.ncols)]


def interior_absent(a):
    """number of absent stream entries whose column lies inside [0, ncols)"""
    s = D.streams64(a)
    offs = D.offsets(a)
    cols = np.arange(a.nrows)[None, :] + offs[:, None]
    return int(np.count_nonzero((s == D.ABSENT64) & (cols >= 0) & (cols < a.ncols)))


def fold_columns(a, x):
    """the contract, column-wise: every row folds its PRESENT entries in ascending offset (= stored) order from 0.0 with separate multiply
    and add; an absent entry leaves the sum as it is, whatever x holds where it points"""
    x = np.asarray(x, dtype=np.float64)
    s64 = D.streams64(a)
    offs = D.offsets(a)
    rows = np.arange(a.nrows)
    y = np.zeros((a.nrows, x.shape[1]))
    with np.errstate(all="ignore"):
        for d, off in enumerate(offs):
            present = s64[d] != D.ABSENT64
            v = np.where(present, s64[d].view(np.float64), 0.0)
            c = np.clip(rows + off, 0, a.ncols - 1)
            prod = v[:, None] * x[c]
            y = np.where(present[:, None], y + prod, y)
    return y


@functools.lru_cache(maxsize=None)
def xcols8(name):
    """eight ordinary columns for the operator"""
    return MC.xcols(operator(name).ncols, 8)


@functools.lru_cache(maxsize=None)
def want8(name):
    """oracle_spmm on xcols8: made once"""
    return MC.oracle_spmm(operator(name), xcols8(name))


def with_special_columns(x, where):
    """a copy of x with column j replaced by special_column(kind) for (j, kind) in where"""
    out = np.array(x, copy=True)
    for j, kind in where.items():
        out[:, j] = MC.special_column(kind, x.shape[0])
    return out


SPECIAL_AT = {1: "nan", 3: "inf", 4: "negzero", 6: "denormal"}


def poisoned_columns(n, k, where, seed=21):
    """three (n, k) arrays with NaN / +inf / -inf in every column exactly at the rows `where`"""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        x = np.random.default_rng(seed).standard_normal((n, k))
        x[where, :] = bad
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------------ solver fixtures
@functools.lru_cache(maxsize=None)
def solve_columns(name, m=8):
    """multi_rhs_cases.stencil_columns for any operator: A 1 plus m - 1 splitmix columns, column j scaled by 10^(j - 3)"""
    a = operator(name)
    return np.stack([a.spmv(np.ones(a.nrows))] + [O.splitmix64_uniform(0x5EED + j, a.nrows) * 10.0 ** (j - 3) for j in range(1, m)], axis=1)


@functools.lru_cache(maxsize=None)
def solve_reference(name, method, pc):
    return MC.oracle_columns(method, operator(name), solve_columns(name), pc=pc)
