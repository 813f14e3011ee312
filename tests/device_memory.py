"""The device-memory figure of the lifetime tests and the protocol that reads it (tests/test_gpu_lifetimes.py, tests/test_gpu_pc_lifetime.py).

The library has no query for the bytes it holds, so the figure is the driver's: the free memory of device 0 (hipMemGetInfo through
torch.cuda.mem_get_info) after the context's streams have drained.  It moves in steps of G bytes (lifetime_cases.G, measured), so a create / use /
destroy whose allocations are smaller than G is repeated until a leak of it would cross a step (lifetime_cases.repeats)."""
ROUNDS = 3


def free_bytes(ctx):
    import torch
    ctx.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def settled_free_bytes(ctx):
    """free_bytes after one small block has been taken and given back.  The driver cuts small blocks out of 2 MiB chunks and does not hand an
    emptied chunk back at once: which emptied chunks it still holds depends on the frees before the reading (MEASURED: after identical rounds
    of 57 blocks of 112 KiB, all freed, the figure read 2 MiB or 4 MiB low in some rounds and not in others, without ever growing; after one
    8 KiB block was taken and freed it read the same in 36 rounds running).  Taking and freeing one small block puts every reading behind the
    same last step."""
    import torch
    import kryst_amd as K
    torch.cuda.synchronize()                          # every stream of the device, not the context's two alone
    v = K.DeviceVec(ctx, 8)
    ctx.synchronize()
    del v
    torch.cuda.synchronize()
    return free_bytes(ctx)


def readings(ctx, round_, rounds=ROUNDS):
    """One unmeasured warm round (kernels load, the partials grow, whatever the runtime allocates once), a trim, the reading f0; then `rounds`
    measured rounds, each followed by a trim and a reading -> [f0 - f_1, ..., f0 - f_rounds]: the bytes lost since f0 after each round."""
    free_bytes(ctx)                                   # (the first query brings its own runtime state)
    round_()
    ctx.trim()
    f0 = settled_free_bytes(ctx)
    lost = []
    for _ in range(rounds):
        round_()
        ctx.trim()
        lost.append(f0 - settled_free_bytes(ctx))
    return lost


def assert_gives_back(ctx, round_, what, rounds=ROUNDS):
    """Every reading equals f0.  The message carries every difference: a steady loss (k, 2k, 3k) reads differently from one jump (k, k, k)
    or from a chunk that came back (k, k, 0).  The figure is the whole device's: nothing is measured twice and nothing is excused."""
    lost = readings(ctx, round_, rounds)
    assert all(v == 0 for v in lost), f"{what}: free device memory fell by {lost} bytes after rounds 1..{rounds} (a leak grows, a one-off stays)"
