"""Whole solves past one chunk of the inner-product fold, bit for bit against the references, in both hand-offs of its second stage.

Every inner product ends in fold2 (kryst_amd/csrc/common.h): stage 1 folds the tile partials in chunks of 1024 tiles (512 rows each),
stage 2 -- only with more than one chunk, n > 524 288 -- folds the chunk values, handed over either by polling (the default) or by a
ticket (KRYST_FOLD_POLL=0; the form a context keeps after a polling fold ran out of patience).  PCA-GMRES and s-step GMRES have a
two-stage fold of their own (pg_fold1_kernel / pg_fold2_kernel).  Beyond the cache regime (keep_in_cache, solver_common.h) the solvers
run the streamed (<false>) instances of their fused operations; KRYST_KEEP_BYTES=0 forces them at any size.

Each case computes its reference once and runs the device solve three times: with the defaults, with the ticket hand-off, and with the
streamed instances on a grid of one workgroup per CU (every workgroup strides over several tiles).  Iterations, converged,
final_residual, the whole residual history and x must equal the reference bit for bit in all three.  Operators: tests/chunked_cases.py."""
import os

import numpy as np
import pytest

import kryst_amd as K
from oracle import oracle as O
import chunked_cases as CC
import krylov_ext_ref as KR
import pca_gmres_ref as PR

pytestmark = pytest.mark.gpu

PCN = K.Preconditioning

KNOBS = {
    "poll": {},
    "ticket": {"KRYST_FOLD_POLL": "0"},
    "streamed": {"KRYST_KEEP_BYTES": "0", "KRYST_EW_BLOCKS_PER_CU": "1"},
}
_KNOB_NAMES = sorted({k for v in KNOBS.values() for k in v})


def _set_knobs(monkeypatch, name):
    for k in _KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in KNOBS[name].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def ctx():
    O.set_threads(min(len(os.sched_getaffinity(0)), 16))
    return K.Context(0)


@pytest.fixture(scope="module")
def rs():
    return O.Reduce.tiled(*K.reduce_spec())


@pytest.fixture(scope="module")
def ops(ctx):
    """(size, variant) -> (host oracle.Csr, device CsrMatrix, b), built once per module."""
    cache = {}

    def get(size, var):
        key = (size, var)
        if key not in cache:
            n = CC.SIZES[size][0]
            if size == "S":
                a, d = O.stencil7(96, var), K.CsrMatrix.stencil7(96, var, ctx=ctx)
            else:
                a = CC.variant(n, var)
                d = K.CsrMatrix.from_csr(n, n, a.row_ptr, a.col_idx, a.vals, ctx=ctx)
            cache[key] = (a, d, CC.rhs(n))
        return cache[key]
    return get


def test_sizes_have_the_tile_and_chunk_counts():
    T, V, F = K.reduce_spec()
    assert (T * V, F) == (512, 1024)
    for name, (n, tiles, chunks) in CC.SIZES.items():
        assert CC.tiles_and_chunks(n, T, V, F) == (tiles, chunks), name
    assert CC.SIZES["S"][0] == 96 ** 3


def check(ref, st, s, x, label, nan_ok=False):
    h, rh = np.array(s.residual_history, dtype=float), np.array(ref.history, dtype=float)
    assert (st.iterations, bool(st.converged)) == (ref.iterations, bool(ref.converged)), (label, st, ref.iterations, ref.converged)
    if len(h) != len(rh) or not np.array_equal(h, rh, equal_nan=nan_ok):
        m = min(len(h), len(rh))
        diff = np.flatnonzero(~((h[:m] == rh[:m]) | (nan_ok & np.isnan(h[:m]) & np.isnan(rh[:m]))))
        pytest.fail(f"{label}: residual history differs (lengths {len(h)} / {len(rh)}, first differing entry "
                    f"{diff[0] if len(diff) else m}: {h[diff[0]] if len(diff) else None!r} vs {rh[diff[0]] if len(diff) else None!r})")
    assert st.final_residual == ref.final_residual or (nan_ok and np.isnan(st.final_residual) and np.isnan(ref.final_residual)), label
    assert np.array_equal(x, ref.x, equal_nan=nan_ok), (label, int(np.sum(x != ref.x)))


# ---------------------------------------------------------------------------------------------------------------- the cases
# pc: None | "jacobi" | "ilu0" (true ILU(0): K.TrueIlu0 with O.Pc.ilu0_true, as ILU_MODES in test_gpu_0_parity.py pairs them)
PCS = {None: (None, None), "jacobi": (K.Jacobi, O.Pc.jacobi), "ilu0": (K.TrueIlu0, O.Pc.ilu0_true)}


def _o(method, **kw):
    return lambda a, b, opc, tol, mx, rs: O.solve(method, a, b, pc=opc, tol=tol, max_iters=mx, rs=rs, **kw)


def _ext(method):
    return lambda a, b, opc, tol, mx, rs: KR.SOLVERS[method](a, b, np.zeros(a.nrows), tol, mx, rs)


def _cg(norm):
    return dict(ref=_o("cg", norm_type=int(norm)), dev=lambda tol, mx: K.CgSolver(tol, mx).with_norm(norm))


def _gmres(side, restart):
    return dict(ref=_o("gmres", restart=restart, side=int(side)),
                dev=lambda tol, mx: K.GmresSolver(restart, tol, mx).with_preconditioning(side))


def _fgmres(orthog, restart):
    return dict(ref=_o("fgmres", restart=restart, orthog=int(orthog)),
                dev=lambda tol, mx: K.FgmresSolver(tol, mx, restart).with_orthog(orthog), call="solve_flex")


def _pca(side, restart):
    return dict(ref=lambda a, b, opc, tol, mx, rs: PR.as_written(a, b, pc=opc, side=int(side), restart=restart, tol=tol, max_iters=mx, rs=rs),
                dev=lambda tol, mx: K.PcaGmresSolver(restart, 2, 1, tol, mx).with_preconditioning(side), nan_ok=True)


def _sstep(sb, restart):
    return dict(ref=lambda a, b, opc, tol, mx, rs: PR.sstep(a, b, pc=opc, side=2, restart=restart, block_size=sb, tol=tol, max_iters=mx, rs=rs),
                dev=lambda tol, mx: K.PcaGmresSolver(restart, 1, sb, tol, mx).with_preconditioning(PCN.Right).with_textbook())


SOLVER = {
    "cg": dict(ref=_o("cg"), dev=lambda tol, mx: K.CgSolver(tol, mx)),
    "cg_unprec": _cg(K.CgNormType.Unpreconditioned),
    "cg_natural": _cg(K.CgNormType.Natural),
    "cg_nonorm": _cg(K.CgNormType.NoNorm),
    "pcg_prec": dict(ref=_o("pcg", norm_type=int(K.CgNormType.Preconditioned)),
                     dev=lambda tol, mx: K.PcgSolver(tol, mx).with_norm(K.CgNormType.Preconditioned)),
    "pcg": dict(ref=_o("pcg"), dev=lambda tol, mx: K.PcgSolver(tol, mx)),
    "bicgstab": dict(ref=_o("bicgstab"), dev=lambda tol, mx: K.BiCgStabSolver(tol, mx)),
    "bicgstab_rpc": dict(ref=_o("bicgstab_rpc"), dev=lambda tol, mx: K.BiCgStabRightPcSolver(tol, mx)),
    "cgs": dict(ref=_o("cgs"), dev=lambda tol, mx: K.CgsSolver(tol, mx)),
    "tfqmr": dict(ref=_o("tfqmr"), dev=lambda tol, mx: K.TfqmrSolver(tol, mx)),
    "minres": dict(ref=_ext("minres"), dev=lambda tol, mx: K.MinresSolver(tol, mx)),
    "qmr": dict(ref=_ext("qmr"), dev=lambda tol, mx: K.QmrSolver(tol, mx)),
    "cgnr": dict(ref=_ext("cgnr"), dev=lambda tol, mx: K.CgnrSolver(tol, mx), nan_ok=True),
    "gmres_nopc_12": _gmres(PCN.NoPc, 12),
    "gmres_left_12": _gmres(PCN.Left, 12),
    "gmres_right_12": _gmres(PCN.Right, 12),
    "gmres_lefttextbook_12": _gmres(PCN.LeftTextbook, 12),
    "fgmres_classical_16": _fgmres(K.Orthog.Classical, 16),
    "fgmres_modified_16": _fgmres(K.Orthog.Modified, 16),
    "pca_left_5": _pca(PCN.Left, 5),
    "pca_right_5": _pca(PCN.Right, 5),
    "sstep1_16": _sstep(1, 16),
    "sstep8_16": _sstep(8, 16),
}

# (size, operator variant, solver, pc, tol, max_iters)
CASES = [
    ("B", "sym", "cg_unprec", None, 0.0, 40),
    ("B", "sym", "cg_natural", None, 0.0, 40),
    ("B", "sym", "cg_nonorm", None, 0.0, 40),
    ("B", "sym", "pcg_prec", "jacobi", 0.0, 40),
    ("B", "nonsym", "bicgstab", None, 0.0, 30),
    ("B", "nonsym", "bicgstab_rpc", "jacobi", 0.0, 30),
    ("B", "nonsym", "bicgstab_rpc", "ilu0", 0.0, 30),
    ("B", "nonsym", "cgs", None, 0.0, 30),
    ("B", "nonsym", "tfqmr", None, 0.0, 30),
    ("B", "sym", "minres", None, 0.0, 40),
    ("B", "nonsym", "qmr", None, 0.0, 30),
    ("B", "nonsym", "cgnr", None, 0.0, 30),
    ("B", "nonsym", "gmres_nopc_12", None, 0.0, 30),
    ("B", "nonsym", "gmres_left_12", "jacobi", 0.0, 30),
    ("B", "nonsym", "gmres_right_12", "jacobi", 0.0, 30),
    ("B", "nonsym", "gmres_lefttextbook_12", "jacobi", 0.0, 30),
    ("B", "nonsym", "fgmres_classical_16", None, 0.0, 40),
    ("B", "nonsym", "fgmres_modified_16", None, 0.0, 40),
    ("B", "nonsym", "pca_left_5", "jacobi", 0.0, 30),
    ("B", "nonsym", "pca_right_5", "jacobi", 0.0, 30),
    ("B", "nonsym", "sstep1_16", "jacobi", 0.0, 32),
    ("B", "nonsym", "sstep8_16", "jacobi", 0.0, 32),
    # converged exits past one chunk: these stop by convergence, well inside the cap (checked below).  TFQMR as written cannot: it starts
    # each step from r = u (tfqmr.rs:203), its estimate sqrt(2k + m + 2) tau grows on this operator, and it takes its converged return at the cap
    ("B", "dom_sym", "cg", None, 1e-8, 300),
    ("B", "dom_nonsym", "bicgstab", None, 1e-8, 300),
    ("B", "dom_nonsym", "gmres_right_12", None, 1e-8, 300),
    ("B", "dom_nonsym", "fgmres_modified_16", None, 1e-8, 300),
    ("B", "dom_nonsym", "cgs", None, 1e-8, 300),
    ("B", "dom_nonsym", "tfqmr", None, 1e-8, 300),
    ("B", "dom_nonsym", "qmr", None, 1e-8, 300),
    ("B", "dom_sym", "minres", None, 1e-8, 300),
    ("C", "sym", "cg", None, 0.0, 25),
    ("C", "sym", "pcg", "jacobi", 0.0, 25),
    ("C", "nonsym", "bicgstab", None, 0.0, 25),
    ("C", "nonsym", "cgs", None, 0.0, 25),
    ("C", "nonsym", "tfqmr", None, 0.0, 25),
    ("C", "sym", "minres", None, 0.0, 25),
    ("C", "nonsym", "cgnr", None, 0.0, 25),
    ("A", "sym", "cg", None, 0.0, 30),
    ("A", "nonsym", "bicgstab", None, 0.0, 30),
    ("A", "nonsym", "fgmres_modified_16", None, 0.0, 30),
    ("S", "convdiff", "bicgstab", None, 0.0, 30),
    ("S", "aniso", "tfqmr", None, 0.0, 30),
    ("S", "convdiff", "gmres_right_12", "jacobi", 0.0, 30),
]


def _case_id(c):
    size, var, solver, pc, tol, mx = c
    return f"{size}-{var}-{solver}" + (f"-{pc}" if pc else "") + ("-tol" if tol else "")


def reference(a, b, solver, pc, tol, mx, rs):
    _, ofn = PCS[pc]
    return SOLVER[solver]["ref"](a, b, ofn(a) if ofn else None, tol, mx, rs)


def device_solve(d, b, solver, pc, tol, mx):
    kcls, _ = PCS[pc]
    spec = SOLVER[solver]
    s = spec["dev"](tol, mx)
    x = np.zeros(len(b))
    st = getattr(s, spec.get("call", "solve"))(d, kcls().setup(d) if kcls else None, b, x)
    return st, s, x


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_solve_past_one_chunk_bit_for_bit(ctx, rs, ops, monkeypatch, case):
    size, var, solver, pc, tol, mx = case
    a, d, b = ops(size, var)
    ref = reference(a, b, solver, pc, tol, mx, rs)
    if tol > 0.0 and solver == "tfqmr":
        assert ref.converged and ref.iterations == mx, (case, ref.iterations)
    elif tol > 0.0:
        assert ref.converged and ref.iterations < mx // 4, (case, ref.iterations)        # a few dozen iterations at most
    else:
        assert ref.iterations > 0, case
    nan_ok = SOLVER[solver].get("nan_ok", False)
    for knob in KNOBS:
        _set_knobs(monkeypatch, knob)
        st, s, x = device_solve(d, b, solver, pc, tol, mx)
        check(ref, st, s, x, f"{_case_id(case)} [{knob}]", nan_ok=nan_ok)
    print(f"[chunked folds] {_case_id(case)}: n = {a.nrows}, {ref.iterations} iterations, converged = {bool(ref.converged)}: "
          f"bit-identical under {', '.join(KNOBS)}")


# ---------------------------------------------------------------------------------------------------------------- hand-offs alternating
def test_hand_offs_alternate_in_one_context(rs, ops, monkeypatch):
    """A fresh context whose first fold runs in the ticket form (the partials and the chunk cells are allocated and armed in the middle of
    that first solve), then dot / norm and solves alternating polling, ticket, polling: every result equals the reference bit for bit
    ("both forms leave the cells armed, so they can alternate", common.h).  Then a second fresh context whose partials grow (re-allocated
    and re-armed) between multi-chunk solves of either form."""
    a24 = O.stencil7(24, "convdiff")
    hosts = {"C": ops("C", "sym")[0::2], "B": ops("B", "sym")[0::2], "Bn": ops("B", "nonsym")[0::2], "24": (a24, CC.rhs(a24.nrows))}
    runs = {"C": ("cg", 25), "B": ("cg", 30), "Bn": ("bicgstab", 30), "24": ("bicgstab", 30)}
    refs = {k: reference(a, b, runs[k][0], None, 0.0, runs[k][1], rs) for k, (a, b) in hosts.items()}

    def solver_in(c):
        devs = {k: K.CsrMatrix.from_csr(a.nrows, a.ncols, a.row_ptr, a.col_idx, a.vals, ctx=c) for k, (a, _) in hosts.items()}

        def solve(k, form, label):
            _set_knobs(monkeypatch, form)
            st, s, x = device_solve(devs[k], hosts[k][1], runs[k][0], None, 0.0, runs[k][1])
            check(refs[k], st, s, x, f"{label} [{form}]")
        return solve

    c = K.Context(0)
    solve = solver_in(c)                   # (uploads only: no fold runs before the first solve)
    solve("C", "ticket", "first fold of the context: CG at size C")
    g = np.random.default_rng(2024)
    for n in (524288, 524289, 1572900, (1 << 20) + 1):
        x, y = g.standard_normal(n), g.standard_normal(n)
        dx, dy = c.vec(x), c.vec(y)
        want = (O.dot(x, y, rs), O.norm(x, rs))
        for form in ("poll", "ticket", "poll"):
            _set_knobs(monkeypatch, form)
            assert (K.dot(dx, dy), K.norm(dx)) == want, (n, form)
    for form in ("poll", "ticket", "poll"):
        solve("B", form, "CG at size B")
        solve("Bn", form, "BiCGStab at size B")
    solve("24", "poll", "BiCGStab at 24^3 (one chunk)")
    solve("C", "poll", "CG at size C again")
    solve("C", "ticket", "CG at size C again")
    del solve
    c.synchronize()

    solve = solver_in(K.Context(0))
    solve("B", "ticket", "fresh context: CG at size B")
    solve("C", "poll", "fresh context: CG at size C (the partials grow)")
    solve("B", "ticket", "fresh context: CG at size B after the growth")
    solve("C", "ticket", "fresh context: CG at size C in the ticket form")
