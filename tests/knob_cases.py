"""The inventory of the KRYST_* environment settings the library reads, and a restatement of the SpMV tile mappings some of them steer.

One row per setting (numpy and the oracle only: nothing here touches the device).  tests/test_knob_inventory_cpu.py holds the table
against the sources -- a setting read in kryst_amd/csrc without a row, or a row whose setting is gone, fails there -- and
tests/test_gpu_knobs.py runs the rows that no older test ran.

A row's class:
  form       the setting chooses a kernel or a code path
  geometry   the same kernel on another grid, group, tile run or workgroup size
  transport  how ranks exchange data
  not-run    never set in a test, for the reason the row gives

per_process: the source reads the setting once, through a function-local `static const ... = [] { getenv ... }()`; monkeypatch.setenv
cannot reach it after the first solve of a process, so its cases run in a fresh child (tests/knob_worker.py).

witness: the query hook a test asserts BEFORE it compares numbers, so that no case passes on the wrong kernel (None: the library offers
none for this setting).

The second half restates, in plain Python, which tile every (workgroup, trip) pair of an SpMV launch visits: the stream kernels
(spmv_stream.hip), the row-pattern kernel (spmv_pattern.hip: spmv_pattern_kernel) and its staged-window form (spmv_pattern_stage_kernel),
with the launch arithmetic of spmv.hip: stream_plan, enqueue_pattern and enqueue_pattern_stage."""
import collections
import functools

import numpy as np

from oracle import oracle as O

Row = collections.namedtuple("Row", "name cls per_process values op shape witness reason")

ASSUMED_CUS = 256           # the CU count the CPU tier assumes; the GPU tier asks the device


def _r(name, cls, values, op, shape, witness=None, per_process=False, reason=None):
    assert cls in ("form", "geometry", "transport", "not-run") and (cls == "not-run") == (reason is not None), name
    return Row(name, cls, per_process, tuple(values), op, shape, witness, reason)


PRINTS = "it only prints"
ROWS = [
    # ---- fp64 SpMV: the storage form
    _r("KRYST_SPMV_COMPRESS", "form", "0123", "spmv", "stencil7 N=17", "encoding()"),
    _r("KRYST_SPMV_KERNEL", "form", "23", "spmv on plain CSR", "any", "encoding()"),
    _r("KRYST_SPMV_DIA", "form", "012", "spmv, operator creation", "stencil7 N=17", "encoding()"),
    _r("KRYST_SPMV_STAGE", "form", "01", "spmv on CSR-P16", "stencil7 even N", "pattern_info()['staged']"),
    _r("KRYST_SPMV_STAGE_UFAR", "form", "01", "staged CSR-P16 spmv", "stencil7 even N", "pattern_info()"),
    _r("KRYST_SPMV_ORDER", "form", "012", "spmv in the slab order of the tiles", "128 x 128 x 7 box", "tile_order()['in_use']"),
    _r("KRYST_SPMV_ORDER_MIN_PLANE", "form", ("8192",), "operator creation", "128 x 128 x 7 box", "tile_order()"),
    _r("KRYST_SPMV_ORDER_SEG_ROWS", "geometry", ("4096",), "operator creation", "128 x 128 x 7 box", "tile_order()"),
    _r("KRYST_SPMV_ALIGN", "form", "01", "plain-CSR spmv", "any"),
    _r("KRYST_SPMV_NT", "form", "01", "plain-CSR spmv", "any"),
    _r("KRYST_SPMV_SLOTS", "geometry", "247", "plain-CSR spmv", "rows longer than a window"),
    _r("KRYST_SPMV_REUSE_DIAG", "form", "01", "CG's p.Ap on a generator-made CSR-P16 operator (dvec == x)", "stencil7 N=16 (unstaged), 40"),
    _r("KRYST_STENCIL_HOST", "form", "01", "stencil7 creation", "any"),
    _r("KRYST_CSR_PLACEMENT_TRIES", "form", "13", "operator creation", "any"),
    # ---- fp64 SpMV: the tile mapping
    _r("KRYST_SPMV_SWIZZLE", "geometry", "01", "spmv, every stream kernel and the pattern kernel", "10 tiles", "encoding()"),
    _r("KRYST_SPMV_GROUP", "geometry", "138", "spmv, every stream kernel and the pattern kernel", "10 tiles", "encoding()"),
    _r("KRYST_SPMV_BLOCKS_PER_CU", "geometry", "12", "spmv, stream kernels", "more than 256 tiles: 64^3", "encoding()"),
    _r("KRYST_SPMV_PATTERN_TPW", "geometry", "138", "spmv, pattern kernel", "10 tiles", "encoding()"),
    _r("KRYST_SPMV_STAGE_GROUP", "geometry", "13", "staged CSR-P16 spmv and CG's fused direction pass", "12 tiles (N=18)", "pattern_info()['staged']"),
    _r("KRYST_SPMV_STAGE_T", "geometry", "24", "staged CSR-P16 spmv", "12 tiles (N=18)", "pattern_info()['staged']"),
    # ---- CG's fused direction pass
    _r("KRYST_CG_FUSE_P", "form", "01", "cg / pcg", "stencil7 N=16", "fuse_march_info()"),
    _r("KRYST_CG_FUSE_MIN_BYTES", "form", ("1",), "cg", "stencil7 N=64", "fuse_march_info()"),
    _r("KRYST_CG_RECOMPUTE_AP", "form", "01", "cg", "stencil7 N=64", "fuse_march_info()['recompute_ap']"),
    _r("KRYST_CG_X_BATCH", "form", "1238", "cg / pcg", "stencil7 N=16", None),
    _r("KRYST_CG_X_SLICE", "form", "01", "cg with x in batches", "stencil7 N=64"),
    _r("KRYST_CG_DEFER_X", "form", "01", "cg / pcg", "stencil7 N=4"),
    _r("KRYST_SPMV_FUSE_MARCH", "form", "01", "cg", "stencil7 N=64", "fuse_march_info()['on']"),
    _r("KRYST_SPMV_FUSE_T", "geometry", "24", "cg", "stencil7 N=16", "fuse_march_info()['T']"),
    _r("KRYST_SPMV_FUSE_SEG", "geometry", ("2", "4"), "cg, marching kernel", "stencil7 N=64", "fuse_march_info()['S']"),
    # (the run-of-tiles kernel pads its LDS request to min(160 KiB / value - 512, 64 KiB): 1 and 2 are the same launch there and only 3
    # differs; the marching kernel's cap is 80 KiB, where 1, 2 and 3 are three launches)
    _r("KRYST_SPMV_FUSE_WG_PER_CU", "geometry", "123", "cg / pcg through the fused SpMV", "stencil7 N=16 (3 differs); marching kernel, N=64 (1, 2, 3 differ)",
       "pattern_info()['staged'], fuse_march_info()['on']"),
    _r("KRYST_SPMV_PID_REUSE", "form", "01", "cg, marching kernel", "stencil7 N=64", "fuse_march_info()['pid_reuse']"),
    _r("KRYST_SPMV_LEG_VALUES", "form", "01", "cg, marching kernel", "stencil7 N=64"),
    # ---- element-wise passes, folds, solver grids
    _r("KRYST_EW_BLOCKS_PER_CU", "geometry", ("1",), "every solver's vector passes", "more tiles than CUs"),
    _r("KRYST_KEEP_BYTES", "form", ("0",), "the streamed instances of the fused vector operations", "any"),
    _r("KRYST_FOLD_POLL", "form", "01", "every inner product past one fold chunk", "n > 524 288"),
    # fg_launch takes max(value, the operation's own BPC): 2 by default, 3 MultiAxpy, 6 the modified Gram-Schmidt link.  A value below an
    # operation's BPC selects nothing for it -- 1 runs the default launches (which stride past 2 / 3 / 6 x CUs tiles), 8 is the value
    # that changes every grid, and only past 8 x CUs tiles does it stride
    _r("KRYST_FG_BLOCKS_PER_CU", "geometry", "8", "fgmres vector passes", "more than 8 x CUs tiles: 102^3 (2 073); 1 is floored to the operations' own BPC",
       per_process=True),
    # defaults 4 (DOT, PG) and 6 / 4 / 3 (GMRES): 1 strides past CUs tiles (64^3), 8 differs from the default past 4 (6) x CUs tiles and
    # strides past 8 x CUs tiles (102^3)
    _r("KRYST_DOT_BLOCKS_PER_CU", "geometry", "18", "fgmres / gmres inner products", "1: more tiles than CUs, 64^3; 8: more than 8 x CUs tiles, 102^3", per_process=True),
    _r("KRYST_GMRES_BLOCKS_PER_CU", "geometry", "18", "gmres", "1: more tiles than CUs, 64^3; 8: more than 8 x CUs tiles, 102^3", per_process=True),
    _r("KRYST_PG_BLOCKS_PER_CU", "geometry", "18", "pca-gmres, s-step gmres", "1: more tiles than CUs, 64^3; 8: more than 8 x CUs tiles, 102^3", per_process=True),
    _r("KRYST_NO_ARENA", "form", ("1",), "every solver's vectors", "any", per_process=True),
    _r("KRYST_BPC_<TAG>", "not-run", (), "-", "-", reason="it overrides the grid of the same ew_kernel whose strided loop the 'streamed' profile "
       "(KRYST_EW_BLOCKS_PER_CU=1) already runs"),
    # ---- the ILU family
    _r("KRYST_ILU_GRID", "form", "01", "ilu apply", "7-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_WAVE", "form", "012", "ilu apply", "7-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_BOX", "form", "012", "ilu apply", "27-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_BOX_REGULAR", "form", "01", "ilu apply, box wavefront kernel", "27-point box 9 x 8 x 8", "ilu_info()['form'], ['regular']"),
    _r("KRYST_ILU_PLANES", "form", "01", "ilu apply", "7-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_SYNCFREE", "form", "01", "ilu apply, level-ordered", "any", "ilu_info()['form']"),
    _r("KRYST_ILU_RUN_FREE", "form", "012", "ilu apply, deep narrow factor", "40 000 rows", "ilu_info()['form']"),
    _r("KRYST_ILU_RUN_PIPE", "form", "01", "ilu apply, deep narrow factor", "40 000 rows", "ilu_info()['form']"),
    _r("KRYST_ILU_FREE_WAVES", "geometry", "148", "ilu apply, deep narrow factor", "40 000 rows", "ilu_info()['form']"),
    _r("KRYST_ILU_FREE_TUNE", "form", ("16897", "513", "8705"), "ilu apply, chains of virtual rows", "27-point 41 x 30 x 19", "ilu_info()['form']"),
    _r("KRYST_ILU_FREE_LONG_PCT", "form", ("0", "2", "100"), "ilu set-up of a deep narrow factor (0: rows longer than 8 send it to the barrier kernel)",
       "40 000 rows", "ilu_info()['form']"),
    _r("KRYST_ILU_RUN_THREADS", "geometry", ("64", "256", "1024"), "ilu apply, tri_run_pipe_kernel", "40 000 rows", "ilu_info()['form']"),
    _r("KRYST_ILU_CSR_HELD", "geometry", ("8", "16"), "ilu apply, tri_syncfree_csr_kernel", "rows above 8 and 16 entries", "ilu_info()['form']"),
    _r("KRYST_ILU_GRAPH", "form", "01", "ilu apply", "any", "ilu_info()['form']"),
    _r("KRYST_ILU_DIRECT_ARGS", "form", "01", "ilu apply, 16 x 16 grid form", "7-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_DEDUP", "form", "01", "ilu set-up, 16 x 16 grid form", "7-point box", "ilu_info()['chunks_not_requested']"),
    _r("KRYST_ILU_DEVICE_SETUP", "form", "01", "ilu set-up", "any"),
    _r("KRYST_ILU_POLL_BUDGET", "form", ("1",), "ilu apply, the wavefront kernels' give-up path", "7-point box", "ilu_info()['form']"),
    _r("KRYST_ILU_SETUP_POLL_BUDGET", "form", ("1",), "ilu set-up on the device, give-up path", "any"),
    _r("KRYST_ILUP_THREADS", "geometry", ("1", "3", "4", "16"), "Ilup(p >= 1) set-up on host threads", "any"),
    _r("KRYST_ILUP_BLOCK", "geometry", ("1", "8", "32", "2048"), "Ilup(p >= 1) set-up on host threads", "any"),
    _r("KRYST_ILUP_CPU_GROUP", "geometry", ("1", "3", "16"), "Ilup(p >= 1) set-up on host threads", "any"),
    _r("KRYST_ILU_VERBOSE", "not-run", (), "-", "-", reason=PRINTS),
    _r("KRYST_ILUP_TRACE", "not-run", (), "-", "-", reason=PRINTS),
    # ---- other preconditioners and solvers
    _r("KRYST_CHEB_POLY_FUSE", "form", "01", "ChebyshevPoly apply", "any", "ChebyshevPoly.info()['fused']"),
    _r("KRYST_ASM_MEM_LIMIT_MB", "form", ("1",), "additive Schwarz set-up, refusal", "any"),
    _r("KRYST_BCG_FUSE_GRAM", "form", "01", "block CG", "any"),
    _r("KRYST_DENSE_TAIL", "geometry", ("0", "8"), "dense LU / QR", "any"),
    # ---- several right-hand sides, fp32 storage
    _r("KRYST_SPMM_FORM", "form", ("plain", "dia"), "spmm", "any", "spmm_kernel()"),
    _r("KRYST_SPMM_BLOCKS_PER_CU", "geometry", "18", "spmm", "more tiles than CUs", "spmm_kernel()"),
    _r("KRYST_SPMM_DIA_NT", "form", "01", "spmm on CSR-DIA", "any", "spmm_kernel()"),
    _r("KRYST_SPMV32_FORM", "form", ("plain", "pattern", "dia"), "fp32-stored spmv", "any", "CsrMatrix32.encoding()"),
    _r("KRYST_SPMV32_STAGE", "form", "01", "fp32-stored spmv on CSR-P16", "stencil7 even N", "CsrMatrix32.encoding()"),
    _r("KRYST_SPMV32_STAGE_T", "geometry", "12", "fp32-stored spmv, staged", "stencil7 even N", "CsrMatrix32.encoding()"),
    _r("KRYST_SPMV32_PATTERN_TPW", "geometry", "138", "fp32-stored spmv, pattern kernel", "10 tiles", "CsrMatrix32.encoding()"),
    _r("KRYST_SPMV32_BLOCKS_PER_CU", "geometry", "18", "fp32-stored spmv", "more tiles than CUs", "CsrMatrix32.encoding()"),
    _r("KRYST_SPMV32_DIA_NT", "form", "01", "fp32-stored spmv on CSR-DIA", "any", "CsrMatrix32.encoding()"),
    _r("KRYST_EW32_BLOCKS_PER_CU", "geometry", "18", "fp32-stored cg", "more tiles than CUs"),
    # ---- several ranks
    _r("KRYST_HALO_EARLY", "transport", "01", "cg / pcg on several ranks", "2 ranks"),
    _r("KRYST_HALO_MODE", "transport", ("rccl",), "a new row-partitioned operator's halo exchange", "2 ranks", "halo_mode('query')"),
    _r("KRYST_HALO_INLINE_BYTES", "transport", ("0",), "peer-store halo exchange", "2 ranks", "halo_mode()"),
    _r("KRYST_SCALAR_REDUCE", "transport", ("rccl",), "a new context's scalar all-reduce", "2 ranks", "scalar_reduce('query')"),
    _r("KRYST_FORCE_COMM", "transport", ("1",), "the collective path on one rank", "1 rank"),
    _r("KRYST_RCCL_LIB", "not-run", (), "-", "-", reason="a path"),
    _r("KRYST_HALO_SELFTEST", "not-run", (), "-", "-", reason="it only skips a safety check"),
    _r("KRYST_IPC_SELFTEST", "not-run", (), "-", "-", reason="it only skips a safety check"),
    _r("KRYST_IPC_POLL_BUDGET", "not-run", (), "-", "-", per_process=True,
       reason="its give-up path spans ranks, and one rank abandoning a wait is not something to stage on a shared machine"),
    _r("KRYST_HALO_DEBUG", "not-run", (), "-", "-", reason=PRINTS),
    _r("KRYST_IPC_DEBUG", "not-run", (), "-", "-", reason=PRINTS),
    # ---- pools, ablations
    _r("KRYST_DEV_POOL_POISON", "form", ("1",), "every device allocation (the whole GPU tier runs under it)", "any", per_process=True),
    _r("KRYST_DEV_POOL_MB", "not-run", (), "-", "-", per_process=True, reason="a pool size"),
    _r("KRYST_HOST_POOL_MB", "not-run", (), "-", "-", reason="a pool size"),
    _r("KRYST_SPMV_ABL", "not-run", (), "-", "-", reason="compiled only into KR_TUNING builds, and wrong by design"),
    _r("KRYST_FUSE_ABL", "not-run", (), "-", "-", reason="compiled only into KR_TUNING builds, and wrong by design"),
]
BY_NAME = {r.name: r for r in ROWS}
FAMILY = "KRYST_BPC_<TAG>"


# where each setting that runs is set: the settings covered before this table was written point at their older tests
TESTED_IN = {
    "KRYST_SPMV_COMPRESS": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_KERNEL": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_DIA": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_STAGE": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_STAGE_UFAR": "tests/test_gpu_spmv_choice.py",
    "KRYST_SPMV_ORDER": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_ORDER_MIN_PLANE": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_ORDER_SEG_ROWS": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_ALIGN": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_NT": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_SLOTS": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_REUSE_DIAG": "tests/test_gpu_knobs.py",
    "KRYST_STENCIL_HOST": "tests/test_gpu_z_multirank_shim.py",
    "KRYST_CSR_PLACEMENT_TRIES": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_SWIZZLE": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_GROUP": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_BLOCKS_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_PATTERN_TPW": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_STAGE_GROUP": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_STAGE_T": "tests/test_gpu_knobs.py",
    "KRYST_CG_FUSE_P": "tests/test_gpu_0_parity.py",
    "KRYST_CG_FUSE_MIN_BYTES": "tests/test_gpu_spmv_choice.py",
    "KRYST_CG_RECOMPUTE_AP": "tests/test_gpu_cg_recompute_ap.py",
    "KRYST_CG_X_BATCH": "tests/test_gpu_0_parity.py",
    "KRYST_CG_X_SLICE": "tests/test_gpu_x_slices.py",
    "KRYST_CG_DEFER_X": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_FUSE_MARCH": "tests/test_gpu_cg_recompute_ap.py",
    "KRYST_SPMV_FUSE_T": "tests/test_gpu_0_parity.py",
    "KRYST_SPMV_FUSE_SEG": "tests/test_gpu_cg_recompute_ap.py",
    "KRYST_SPMV_FUSE_WG_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_SPMV_PID_REUSE": "tests/test_gpu_march_step.py",
    "KRYST_SPMV_LEG_VALUES": "tests/test_gpu_march_step.py",
    "KRYST_EW_BLOCKS_PER_CU": "tests/test_gpu_chunked_folds.py",
    "KRYST_KEEP_BYTES": "tests/test_gpu_0_parity.py",
    "KRYST_FOLD_POLL": "tests/test_gpu_block_cg.py",
    "KRYST_FG_BLOCKS_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_DOT_BLOCKS_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_GMRES_BLOCKS_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_PG_BLOCKS_PER_CU": "tests/test_gpu_knobs.py",
    "KRYST_NO_ARENA": "tests/test_gpu_knobs.py",
    "KRYST_ILU_GRID": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_WAVE": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_BOX": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_BOX_REGULAR": "tests/test_gpu_knobs.py",
    "KRYST_ILU_PLANES": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_SYNCFREE": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_RUN_FREE": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_RUN_PIPE": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_FREE_WAVES": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_FREE_TUNE": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_FREE_LONG_PCT": "tests/test_gpu_knobs.py",
    "KRYST_ILU_RUN_THREADS": "tests/test_gpu_knobs.py",
    "KRYST_ILU_CSR_HELD": "tests/test_gpu_knobs.py",
    "KRYST_ILU_GRAPH": "tests/test_gpu_knobs.py",
    "KRYST_ILU_DIRECT_ARGS": "tests/test_gpu_knobs.py",
    "KRYST_ILU_DEDUP": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_DEVICE_SETUP": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_POLL_BUDGET": "tests/test_gpu_0_parity.py",
    "KRYST_ILU_SETUP_POLL_BUDGET": "tests/test_gpu_0_parity.py",
    "KRYST_ILUP_THREADS": "tests/test_gpu_0_parity.py",
    "KRYST_ILUP_BLOCK": "tests/test_gpu_0_parity.py",
    "KRYST_ILUP_CPU_GROUP": "tests/test_gpu_knobs.py",
    "KRYST_CHEB_POLY_FUSE": "tests/test_gpu_knobs.py",
    "KRYST_ASM_MEM_LIMIT_MB": "tests/test_gpu_asm.py",
    "KRYST_BCG_FUSE_GRAM": "tests/test_gpu_block_cg.py",
    "KRYST_DENSE_TAIL": "tests/test_gpu_dense.py",
    "KRYST_SPMM_FORM": "tests/test_gpu_block_cg.py",
    "KRYST_SPMM_BLOCKS_PER_CU": "tests/test_gpu_spmm_dia.py",
    "KRYST_SPMM_DIA_NT": "tests/test_gpu_spmm_dia.py",
    "KRYST_SPMV32_FORM": "tests/test_gpu_mixed_dia.py",
    "KRYST_SPMV32_STAGE": "tests/test_gpu_mixed_dia.py",
    "KRYST_SPMV32_STAGE_T": "tests/test_gpu_mixed_pattern.py",
    "KRYST_SPMV32_PATTERN_TPW": "tests/test_gpu_mixed_pattern.py",
    "KRYST_SPMV32_BLOCKS_PER_CU": "tests/test_gpu_mixed_dia.py",
    "KRYST_SPMV32_DIA_NT": "tests/test_gpu_mixed_dia.py",
    "KRYST_EW32_BLOCKS_PER_CU": "tests/test_gpu_mixed_edges.py",
    "KRYST_HALO_EARLY": "tests/test_gpu_z_multirank_shim.py",
    "KRYST_HALO_MODE": "tests/test_gpu_z_multirank_shim.py",
    "KRYST_HALO_INLINE_BYTES": "tests/multirank_worker.py",
    "KRYST_SCALAR_REDUCE": "tests/test_gpu_z_multirank_shim.py",
    "KRYST_FORCE_COMM": "tests/test_gpu_y_dist_single.py",
    "KRYST_DEV_POOL_POISON": "tests/test_gpu_0_parity.py",
}


# ---------------------------------------------------------------------------------------------------------------- the tile mappings
TILE = 512


def ntiles_of(nrows):
    return (nrows + TILE - 1) // TILE


def _ceil(a, b):
    return (a + b - 1) // b


def stream_map(ntiles, group=1, swizzle=0, bpc=0, num_cu=ASSUMED_CUS):
    """spmv_stream.hip (every kernel's tile loop) under spmv.hip: stream_plan.  -> {(workgroup, trip): tile or None}; None: a slot past
    ntiles that the loop steps over (grouped) -- the swizzled loop ends there instead."""
    group = max(1, group)
    chunk = _ceil(ntiles, 8)
    if not swizzle:
        chunk = _ceil(chunk, group) * group
    per = chunk if bpc <= 0 else min(chunk, max(1, num_cu * bpc // 8))
    visits = {}
    for wg in range(per * 8):
        xcd, slot0 = wg & 7, wg >> 3
        for trip, li in enumerate(range(slot0, chunk, per)):
            ti = xcd * chunk + li if swizzle else ((li // group) * 8 + xcd) * group + li % group
            if ti >= ntiles:
                if swizzle:
                    break
                visits[(wg, trip)] = None
                continue
            visits[(wg, trip)] = ti
    return visits


def pattern_map(ntiles, group=8, swizzle=0, tpw=8):
    """spmv_pattern_kernel under enqueue_pattern: workgroup b of XCD x owns the tpw consecutive slots [b tpw, (b + 1) tpw) of the XCD's
    share, a whole number of runs of `group` slots"""
    group, tpw = max(1, group), max(1, tpw)
    chunk = _ceil(_ceil(ntiles, 8), group) * group
    per = _ceil(chunk, tpw)
    visits = {}
    for wg in range(per * 8):
        xcd, slot0 = wg & 7, wg >> 3
        for trip, li in enumerate(range(slot0 * tpw, min((slot0 + 1) * tpw, chunk))):
            ti = xcd * chunk + li if swizzle else ((li // group) * 8 + xcd) * group + li % group
            visits[(wg, trip)] = ti if ti < ntiles else None
    return visits


def stage_map(ntiles, group=1, T=2):
    """spmv_pattern_stage_kernel under enqueue_pattern_stage: a workgroup takes ONE run of T consecutive tiles; groups of `group` runs go
    round-robin over the XCDs.  A trip is a tile of the run."""
    group = max(1, group)
    nruns = _ceil(ntiles, T)
    per = _ceil(_ceil(nruns, 8), group) * group
    visits = {}
    for wg in range(per * 8):
        xcd, slot = wg & 7, wg >> 3
        qr = (((slot // group) * 8 + xcd) * group + slot % group) * T
        if qr >= ntiles:
            visits[(wg, 0)] = None
            continue
        for trip in range(min(T, ntiles - qr)):
            visits[(wg, trip)] = qr + trip
    return visits


def mapping(case, num_cu=ASSUMED_CUS):
    k = case["kernel"]
    if k == "stream":
        return stream_map(case["ntiles"], case.get("group", 1), case.get("swizzle", 0), case.get("bpc", 0), num_cu)
    if k == "pattern":
        return pattern_map(case["ntiles"], case.get("group", 8), case.get("swizzle", 0), case.get("tpw", 8))
    return stage_map(case["ntiles"], case.get("group", 1), case.get("T", 2))


def visited_once(visits, ntiles):
    seen = sorted(t for t in visits.values() if t is not None)
    return seen == list(range(ntiles))


def max_trips(visits):
    per = collections.Counter(wg for (wg, _), t in visits.items() if t is not None)
    return max(per.values()) if per else 0


def slots_past_the_end(visits):
    return sum(1 for t in visits.values() if t is None)


# The SpMV geometry cases of tests/test_gpu_knobs.py, as the mapping sees them.  Tile counts: stencil7 N = 17 / 33 -> 10 / 71 (odd N: the
# pattern kernel, no staged form), N = 18 / 34 -> 12 / 77 (the staged form), the ragged operator 4, the random one 9, N = 65 -> 537, N = 64 -> 512.
# "trips": "many" -- some workgroup must take two or more trips (asserted); "one" -- the launch hands every workgroup ONE slot by
# construction (a stream kernel's default grid is 8 x the XCD share; a pattern workgroup with one tile per workgroup), so these values get
# their second trip from the rows below them that add KRYST_SPMV_BLOCKS_PER_CU=1 at 537 tiles.
SMALL_TILES = (10, 71, 4, 9)
STENCIL_TILES = (10, 71)    # the operators with a row-pattern form; the two random ones stream plain CSR
STAGED_TILES = (12, 77)
STRIDED_TILES = 537         # 65^3 rows: 3 trips per workgroup at one workgroup per CU, and no multiple of 8, 24 or 64


def _geometry_cases():
    out = []
    for nt in SMALL_TILES:
        for sw in (0, 1):
            out.append(dict(kernel="stream", ntiles=nt, swizzle=sw, group=1, trips="one", env={"KRYST_SPMV_SWIZZLE": str(sw)}))
            if nt in STENCIL_TILES:
                out.append(dict(kernel="pattern", ntiles=nt, swizzle=sw, group=8, tpw=8, trips="many", env={"KRYST_SPMV_SWIZZLE": str(sw)}))
        for g in (1, 3, 8):
            out.append(dict(kernel="stream", ntiles=nt, group=g, trips="one", grouped=True, env={"KRYST_SPMV_GROUP": str(g)}))
            if nt in STENCIL_TILES:
                out.append(dict(kernel="pattern", ntiles=nt, group=g, tpw=8, trips="many", grouped=True, env={"KRYST_SPMV_GROUP": str(g)}))
        for tpw in (1, 3, 8) if nt in STENCIL_TILES else ():
            out.append(dict(kernel="pattern", ntiles=nt, group=8, tpw=tpw, trips="one" if tpw == 1 else "many", grouped=True,
                            env={"KRYST_SPMV_PATTERN_TPW": str(tpw)}))
    for nt in STAGED_TILES:
        for g in (1, 3):
            out.append(dict(kernel="stage", ntiles=nt, group=g, T=2, trips="many", grouped=True, env={"KRYST_SPMV_STAGE_GROUP": str(g)}))
        for T in (2, 4):
            out.append(dict(kernel="stage", ntiles=nt, group=1, T=T, trips="many", grouped=True, env={"KRYST_SPMV_STAGE_T": str(T)}))
    for sw in (0, 1):
        out.append(dict(kernel="stream", ntiles=STRIDED_TILES, swizzle=sw, bpc=1, trips="many",
                        env={"KRYST_SPMV_SWIZZLE": str(sw), "KRYST_SPMV_BLOCKS_PER_CU": "1"}))
    for g in (1, 3, 8):
        out.append(dict(kernel="stream", ntiles=STRIDED_TILES, group=g, bpc=1, trips="many", grouped=True,
                        env={"KRYST_SPMV_GROUP": str(g), "KRYST_SPMV_BLOCKS_PER_CU": "1"}))
    out.append(dict(kernel="stream", ntiles=512, bpc=1, trips="many", env={"KRYST_SPMV_BLOCKS_PER_CU": "1"}))
    out.append(dict(kernel="stream", ntiles=512, bpc=2, trips="one", env={"KRYST_SPMV_BLOCKS_PER_CU": "2"}))
    return out


GEOMETRY_CASES = _geometry_cases()


def geometry_label(c):
    return "%s-%dtiles-%s" % (c["kernel"], c["ntiles"], ",".join("%s=%s" % (k[len("KRYST_SPMV_"):], v) for k, v in sorted(c["env"].items())))


# ---------------------------------------------------------------------------------------------------------------- shared operators
@functools.lru_cache(maxsize=None)
def random_csr(n=512 * 9 - 5, seed=31):
    """n rows of 0 .. 12 entries at random columns (far more than 256 distinct offsets: plain CSR only); 9 tiles, the last one 5 rows short"""
    g = np.random.default_rng(seed)
    lens = g.integers(0, 13, size=n)
    cols = [np.unique(g.integers(0, n, size=int(k))) for k in lens]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    ci = np.concatenate(cols)
    return O.Csr(n, n, rp, ci, g.standard_normal(len(ci)))


def deep_factor(wide_first=False, wide_middle=False, seed=2024):
    """The deep, narrow operator of test_narrow_level_runs_of_a_deep_factor_bit_exact: 40 000 rows and a thousand dependency levels --
    dependencies in the previous level and tens of thousands of positions back, 50 rows of ~30 entries (longer than the eight held in
    registers), a first level of 1 500 (wide_first: 3 000) independent rows; wide_middle: 2 500 more rows that all hang on ONE row half way
    down the chain (a level of > 2 048 rows between two runs of narrow levels)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n, free = 40000, (3000 if wide_first else 1500)
    rows = np.repeat(np.arange(free, n), 9)
    near = rows + rng.integers(-300, 301, len(rows))
    far = rng.integers(0, n, len(rows))                                   # one entry in ten couples to ANY row: dependencies far below the window
    cols = np.clip(np.where(rng.random(len(rows)) < 0.1, far, near), 0, n - 1)
    vals = rng.uniform(-1.0, 1.0, len(rows))
    chain = n
    if wide_middle:
        rows = np.concatenate([rows, np.arange(n, n + 2500)]); cols = np.concatenate([cols, np.full(2500, 20000)]); vals = np.concatenate([vals, rng.uniform(-1.0, 1.0, 2500)])
        n += 2500
    m = sp.csr_matrix((vals, (rows, cols)), shape=(n, n)); m.sum_duplicates()
    dense_rows = rng.choice(np.arange(free, chain), 50, replace=False)    # rows with ~30 entries: longer than the held eight
    extra = sp.csr_matrix((rng.uniform(-1.0, 1.0, 50 * 24), (np.repeat(dense_rows, 24), np.clip(np.repeat(dense_rows, 24) + rng.integers(-2000, 2001, 50 * 24), 0, chain - 1))), shape=(n, n))
    m = (m + extra).tocsr(); m.sum_duplicates()
    m = m - sp.diags(m.diagonal()) + sp.diags(np.asarray(abs(m).sum(axis=1)).ravel() + 1.0)
    m = m.tocsr(); m.sort_indices(); m.eliminate_zeros()
    return O.Csr(n, n, m.indptr, m.indices, m.data)


# ---------------------------------------------------------------------------------------------------------------- per-process profiles
PER_PROCESS_BPC = ("KRYST_FG_BLOCKS_PER_CU", "KRYST_DOT_BLOCKS_PER_CU", "KRYST_GMRES_BLOCKS_PER_CU", "KRYST_PG_BLOCKS_PER_CU")
PROFILES = {
    "low": dict({k: "1" for k in PER_PROCESS_BPC}, KRYST_NO_ARENA="1"),
    "high": {k: "8" for k in PER_PROCESS_BPC},
}
# (solver, N, max_iters): convdiff at 12^3 to convergence or the cap; at 64^3 -- 512 tiles: the GMRES, PCA-GMRES and inner-product passes
# stride at one workgroup per CU -- with at most 10 iterations; and at 102^3 -- 2 073 tiles, more than 8 x 256 -- with at most 6, where
# FGMRES's passes stride at their own BPC (the low profile's 1 is floored to it) and every pass of the high profile runs a grid that is
# not the default one and strides
WORKER_SOLVERS = ("gmres5_right_jacobi", "fgmres5_classical", "fgmres5_modified", "pca5_right_jacobi", "sstep3_5_right_jacobi")
WORKER_BIG = 102
WORKER_CASES = [(s, 12, 40) for s in WORKER_SOLVERS] + [(s, 64, 10) for s in WORKER_SOLVERS] + [(s, WORKER_BIG, 6) for s in WORKER_SOLVERS]
WORKER_TOL = 1e-8

# the launch arithmetic of the passes (ew.h: launch_ew_gated; fgmres.hip: fg_launch; gmres_common.h; pca_gmres.hip)
FG_OP_BPC = {"default": 2, "MultiAxpy": 3, "modified link": 6}
DEFAULT_BPC = {"KRYST_DOT_BLOCKS_PER_CU": (4,), "KRYST_PG_BLOCKS_PER_CU": (4,), "KRYST_GMRES_BLOCKS_PER_CU": (6, 4, 3)}


def ew_grid(ntiles, num_cu, bpc):
    return min(ntiles, num_cu * bpc)


def profile_conditions(profile, num_cu=ASSUMED_CUS):
    """-> list of (what, holds): what each profile is there to reach, from the CU count"""
    t64, tbig = ntiles_of(64 ** 3), ntiles_of(WORKER_BIG ** 3)
    out = []
    if profile == "low":
        out.append(("GMRES / PCA-GMRES / dot passes stride at 64^3 on one workgroup per CU", ew_grid(t64, num_cu, 1) < t64))
        # the value 1 is floored: FGMRES's passes run their default grids, and those stride at 102^3
        out += [(f"FGMRES {op} pass strides at {WORKER_BIG}^3 on its own BPC", ew_grid(tbig, num_cu, max(1, b)) < tbig) for op, b in FG_OP_BPC.items()]
    else:
        out.append((f"every pass strides at {WORKER_BIG}^3 on 8 workgroups per CU", ew_grid(tbig, num_cu, 8) < tbig))
        out += [(f"FGMRES {op} pass: 8 is not the default grid", ew_grid(tbig, num_cu, max(8, b)) != ew_grid(tbig, num_cu, b)) for op, b in FG_OP_BPC.items()]
        out += [(f"{k}: 8 is not the default grid", ew_grid(tbig, num_cu, 8) != ew_grid(tbig, num_cu, b)) for k, bs in DEFAULT_BPC.items() for b in bs]
    return out
