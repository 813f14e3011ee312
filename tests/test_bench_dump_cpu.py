"""bench.py --dump-outputs without a GPU: dump_outputs on synthetic iterates (x[i] = i, so a sampled value names its own row).  The whole-x
branch, the sampled branch that the default 512^3 run takes (one seeded row per stride, the row numbers beside the values), the same files on
every call, and the 64 MiB budget over all ranks at 1, 2 and 8 ranks."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 64 << 20


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _dump(B, d, n, rank, world, hist_len=931):
    B.dump_outputs(str(d), {"x": np.arange(n, dtype=np.float64), "residual_history": np.linspace(1.0, 0.5, hist_len)}, rank, world)
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_x_is_dumped_whole(tmp_path):
    B = _bench()
    n = 32 ** 3
    fs = _dump(B, tmp_path, n, 0, 1)
    assert sorted(fs) == ["residual_history.npy", "x.npy"]
    assert all(v.dtype == np.float64 for v in fs.values())
    assert np.array_equal(fs["x.npy"], np.arange(n, dtype=np.float64))
    assert np.array_equal(fs["residual_history.npy"], np.linspace(1.0, 0.5, 931))


@pytest.mark.parametrize("n,world", [((1 << 22) + 12345, 1), (5_000_000, 1), (512 ** 3 // 8, 8), (3_000_000, 2)])
def test_large_x_is_a_fixed_seeded_sample_within_the_budget(tmp_path, n, world):
    B = _bench()
    total = 0
    for rank in ([0, world - 1] if world > 2 else range(world)):
        d1, d2 = tmp_path / f"a{rank}", tmp_path / f"b{rank}"
        fs = _dump(B, d1, n, rank, world)
        sfx = f"_rank{rank}" if world > 1 else ""
        assert sorted(fs) == sorted(f"{k}{sfx}.npy" for k in ("residual_history", "x", "x_index"))
        assert all(v.dtype == np.float64 for v in fs.values())
        idx, x = fs[f"x_index{sfx}.npy"], fs[f"x{sfx}.npy"]
        k = B.DUMP_X_SAMPLE // world
        stride = n // k
        assert len(idx) == len(x) == k
        assert idx[0] >= 0 and idx[-1] < n and np.all(np.diff(idx) > 0)                  # in bounds, distinct, ascending
        assert np.all((idx // stride) == np.arange(k))                                   # one row in each stride
        assert np.array_equal(x, idx)                                                    # x[i] = i: the values of exactly those rows
        fs2 = _dump(B, d2, n, rank, world)                                               # the same files on every call
        assert all(np.array_equal(fs[f], fs2[f]) for f in fs)
        total += sum(os.path.getsize(d1 / f) for f in fs)
    # every rank writes the same amount: the whole dump over `world` ranks
    per_rank = total / (2 if world > 2 else world)
    assert per_rank * world <= BUDGET
