"""What tests/multirank_ext_cases.py promises to the several-ranks tests, checked with the references alone (no GPU): the tabled stop
iterations and the indefinite exit, the operators' properties, the partitions' tiles, and the table of refusals against the sources."""
import os
import re

import numpy as np
import pytest

import kryst_amd as K
import multirank_ext_cases as M

ROOT = M.ROOT


# ------------------------------------------------------------------------------------------------ section C: the stop tables
@pytest.mark.parametrize("method,k,tol", M.c_stop_cases(), ids=[f"{m}-{k}" for m, k, _ in M.c_stop_cases()])
def test_the_reference_stops_at_exactly_the_tabled_iteration(method, k, tol):
    a = M.operator(M.C_OP)
    s, res0 = M.c_series(method)
    assert s[k - 1] / s[k] >= 1.001, "the two entries around the stop are too close for a tolerance between them"
    code, it, conv, fin, hist, _ = M.reference_solve(method, a, M.rhs(a), M.reduce_for(M.c_offsets()), tol, M.C_MAX_ITERS)
    assert (code, it, conv) == (0, k, True)
    assert it < M.C_MAX_ITERS
    assert fin <= tol if res0 is None else hist[-1] == s[k]   # (BiCGStab may leave iteration k at its half step: s_norm, not r_norm)


def test_the_sweep_covers_the_batch_boundaries():
    """a stop on the last iteration of a batch, on the first of the next, and inside one, for every check_every"""
    for chk in M.C_CHECK_EVERY:
        rem = {k % chk for k in M.C_STOPS}
        assert 0 in rem and (chk == 1 or 1 in rem), (chk, rem)
    assert set(M.C_GMRES_STOPS) >= {4, 5, 6, 10, 11}        # around the restarts of GMRES(5)


@pytest.mark.parametrize("method", M.C_ERROR_METHODS)
def test_the_indefinite_operator_ends_in_an_error_after_the_first_iteration(method):
    a = M.operator(M.C_INDEFINITE)
    code, it, conv, fin, hist, x = M.reference_solve(method, a, M.rhs(a), M.reduce_for(M.c_offsets()), 1e-8, 50, M.guess(a))
    assert code == M.INDEFINITE_MATRIX and it >= 2 and not conv
    assert np.array_equal(x, M.guess(a))                      # the reference writes nothing back on Err


def test_degenerate_exits_of_the_reference_are_finite_statuses():
    a = M.operator(M.C_OP)
    rs = M.reduce_for(M.c_offsets())
    for which in M.C_DEGENERATE:
        b, x0, tol, mx = M.c_degenerate_problem(which)
        for method in M.C_DEGENERATE_METHODS[which]:
            code, it, conv, fin, hist, x = M.reference_solve(method, a, b, rs, tol, mx, x0)
            assert code in (0, M.INDEFINITE_MATRIX) and it <= max(mx, 1), (which, method, code, it)


# ------------------------------------------------------------------------------------------------ section A: operators, partitions, sessions
def test_the_general_operators_are_strictly_diagonally_dominant():
    import scipy.sparse as sp
    for kind in ("nonsym", "sym"):
        a = M.operator(("general", 1031, kind))
        m = sp.csr_matrix((a.vals, a.col_idx, a.row_ptr), shape=(a.nrows, a.ncols))
        d = m.diagonal()
        off = np.asarray(abs(m).sum(axis=1)).ravel() - np.abs(d)
        assert (d > off).all() and (d > 0).all()
        assert (abs(m - m.T).max() > 0) == (kind == "nonsym")


def test_every_rank_of_a_stencil_case_has_the_tiles_the_case_is_for():
    for name, c in M.A_CASES.items():
        a = M.operator(c["op"])
        offs = M.offsets(c["op"], c["P"])
        assert len(offs) == c["P"] + 1 and offs[0] == 0 and offs[-1] == a.nrows and (np.diff(offs) > 0).all()
        for r in range(c["P"]):
            below, above = M.halo_sides(a, offs, r)
            assert below == (r > 0) and above == (r < c["P"] - 1), (name, r)         # middle ranks: a halo from both sides
            kinds = M.tile_kinds(a, offs, r)
            assert True in kinds, (name, r)
            if name in M.INTERIOR_AND_BOUNDARY_ON_EVERY_RANK:
                assert False in kinds, (name, r)
    # the grids named for three ranks are too small for that: a middle rank of 12^3 / 3 holds 576 rows, two tiles, each next to a neighbour's plane
    assert all(M.tile_kinds(M.operator(("stencil", 12, "convdiff")), M.offsets(("stencil", 12, "convdiff"), 3), 1))
    assert M.A_CASES["poisson48-p4-light"]["P"] == 4 and min(len(M.tile_kinds(M.operator(("stencil", 48, "poisson")), M.offsets(("stencil", 48, "poisson"), 4), r))
                                                              for r in range(4)) >= 50


def test_every_extension_solver_meets_every_kind_of_partition():
    seen = {m: set() for m in M.EXT}
    for c in M.A_CASES.values():
        for m in c["solvers"]:
            seen[m].add(c["op"][:1] + c["op"][2:])
    for m in M.EXT:
        assert ("general", "sym" if m.startswith("minres") else "nonsym") in seen[m] and ("stencil", "varcoef") in seen[m], (m, seen[m])
    assert max(c["P"] for c in M.A_CASES.values()) <= 5


def test_session_tolerances_converge_inside_the_third_step():
    lo, hi = sum(M.SESSION_STEPS[:2]), sum(M.SESSION_STEPS)
    assert lo < M.SESSION_STOP <= hi < M.SESSION_MAX_ITERS
    for case, c in M.A_CASES.items():
        if not c["sessions"]:
            continue
        a = M.operator(c["op"])
        rs = M.reduce_for(M.offsets(c["op"], c["P"]))
        for method in M.SESSION_METHODS:
            code, it, conv, fin, hist, x = M.reference_solve(method, a, M.rhs(a), rs, M.session_tol(case, method), M.SESSION_MAX_ITERS, M.guess(a))
            assert (code, it, conv) == (0, M.SESSION_STOP, True), (case, method, it)
    assert set(M.SESSION_METHODS.values()) == {2, 5, 6, 7, 8}
    assert all(K.Session.METHODS[m] == v for m, v in M.SESSION_METHODS.items())


def test_section_b_bounds_are_usable():
    for c in M.B_CASES.values():
        a = M.operator(c["op"])
        for jac in M.B_SCALINGS:
            lo, hi = M.b_bounds(a, jac)
            assert 0.0 < lo < hi and np.isfinite(hi)


# ------------------------------------------------------------------------------------------------ section D: the table against the sources
def test_the_refusal_table_covers_every_not_supported_message_of_the_sources():
    sites = M.not_supported_sites()
    assert len(sites) == sum(e["count"] for e in M.REFUSALS)
    for e in M.REFUSALS:
        hits = [line for fn, line in sites if fn == e["file"] and e["frag"] in line]
        assert len(hits) == e["count"], (e["file"], e["frag"], len(hits))
        if e["needs"] is not None:                                 # a refusal of a distributed operator or context: its status in the source
            assert all("KRYST_UNSUPPORTED" in line and "KR_ARG" not in line for line in hits), (e["file"], e["frag"])
            assert (e["entry"] in M.D_ENTRIES) != (e["entry"] is None and bool(e.get("why"))), e
    matched = sum(1 for fn, line in sites if any(fn == e["file"] and e["frag"] in line for e in M.REFUSALS))
    assert matched == len(sites)
    # every entry the GPU tests call leads to a tabled source line
    frags = " ".join(e["frag"] for e in M.REFUSALS)
    for name, (status, word, needs) in M.D_ENTRIES.items():
        assert status == M.UNSUPPORTED and needs in ("dist", "ranks") and word in frags, name


def test_the_header_documents_the_statuses():
    with open(os.path.join(ROOT, "include", "kryst_hip.h"), encoding="utf-8") as f:
        h = f.read()
    amg = h[h.index("/* AMG (src/preconditioner/amg.rs)"):h.index("int32_t kryst_pc_amg(")]
    assert re.search(r"KRYST_UNSUPPORTED \(a distributed operator\)", amg)
    assert not re.search(r"KRYST_ERR_ARG \([^)]*distributed", amg)


def test_design_carries_the_support_table():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        assert M.support_table_markdown() in f.read()
