"""DensityProfile timing on one GPU: 32 768 atoms x PROFILE_FRAMES frames (default 10 000, the benchmark's C2 shape),
3 axes x 201 bins.  HBM-resident frames: one group, two groups, ``recenter=0``, ``average=False`` and a slab-like
input (> 90 % of the particles in three z bins: the LDS-collision case); then pageable host memory.  Every case is
warmed up and run REPS times; the median wall time of ``DensityProfile(...).run()`` is reported as ms, frames/s and
as a fraction of the streaming floor (12 B x atoms x frames at 6.3 TB/s achievable HBM rate), next to the device
time of the engine's kernels alone (HIP events), also with the LDS replica count capped at 1 and with global atomics
(``ProfileEngine(replicas=...)``).  PROFILE_FRAMES=... PROFILE_REPS=... shorten a run, e.g. under a profiler."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DensityProfile

N = 32768
F = int(os.environ.get("PROFILE_FRAMES", 10000))
F_HOST = min(F, int(os.environ.get("PROFILE_HOST_FRAMES", 1000)))
REPS = int(os.environ.get("PROFILE_REPS", 7))
HBM_RATE = 6.3e12
L = np.array([64.0, 64.0, 96.0])
dims = [*L, 90.0, 90.0, 90.0]


def measure(name, make, n_frames, floor_rate=HBM_RATE):
    make().run(stop=min(n_frames, 64))                   # warm-up: pools, streams, code objects
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        make().run()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    floor = 12.0 * N * n_frames / floor_rate
    print(f"{name}: {n_frames} frames of {N} atoms: median {t * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, "
          f"max {max(times) * 1e3:.2f}, {REPS} runs), {n_frames / t:.0f} frames/s, "
          f"{12.0 * N * n_frames / t / 1e12:.3f} TB/s, floor {floor * 1e3:.2f} ms -> {floor / t:.2f} of the floor",
          flush=True)


def kernel_time(name, d, n_frames, sizes, recenter=False, per_frame=False, replicas=None):
    eng = _core.ProfileEngine(sizes, [0, 1, 2], 201, L, per_frame=per_frame, timing=True, replicas=replicas)
    try:
        if recenter:
            eng.set_recenter(0)
        eng.accumulate_device(d.ptr, N, min(n_frames, 64))
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, n_frames)
            ms.append(eng.stats()["kernel_ms"])
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        floor = 12.0 * N * n_frames / HBM_RATE
        print(f"{name} [kernels only, {eng.stats()['replicas']} LDS replicas]: median {t * 1e3:.2f} ms, "
              f"{n_frames / t:.0f} frames/s, {12.0 * N * n_frames / t / 1e12:.3f} TB/s -> {floor / t:.2f} of the floor", flush=True)
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk, uniform density
u = mdhelper_amd.ArrayUniverse.from_device(d, dims)
one = [u.atoms]
two = [u.select(np.arange(N // 3)), u.select(np.arange(N // 3, N))]
measure("HBM, 1 group", lambda: DensityProfile(one, verbose=False), F)
kernel_time("HBM, 1 group", d, F, [N])
kernel_time("HBM, 1 group", d, F, [N], replicas=1)
kernel_time("HBM, 1 group", d, F, [N], replicas=0)
measure("HBM, 2 groups", lambda: DensityProfile(two, verbose=False), F)
kernel_time("HBM, 2 groups", d, F, [N // 3, N - N // 3])
measure("HBM, 1 group, average=False", lambda: DensityProfile(one, average=False, verbose=False), F)
kernel_time("HBM, 1 group, average=False", d, F, [N], per_frame=True)
measure("HBM, 2 groups, recenter=0", lambda: DensityProfile(two, recenter=0, verbose=False), F)
kernel_time("HBM, 2 groups, recenter=0", d, F, [N // 3, N - N // 3], recenter=True)
d.free()

# slab: 93 % of the particles inside three z bins
rng = np.random.default_rng(0)
slab = (rng.random((F_HOST, N, 3), dtype=np.float32) * L.astype(np.float32))
w = np.float32(L[2] / 201)
dense = rng.random(N) < 0.93
slab[:, dense, 2] = 100 * w + rng.random((F_HOST, int(dense.sum())), dtype=np.float32) * 3 * w
ds = _core.DeviceArray.upload(slab)
us = mdhelper_amd.ArrayUniverse.from_device(ds, dims)
measure("HBM, slab, 1 group", lambda: DensityProfile(us.atoms, verbose=False), F_HOST)
kernel_time("HBM, slab, 1 group", ds, F_HOST, [N])
kernel_time("HBM, slab, 1 group", ds, F_HOST, [N], replicas=1)
kernel_time("HBM, slab, 1 group", ds, F_HOST, [N], replicas=0)
ds.free()

# pageable host memory: compare with the link rate `bench.py --workload ingest` prints on the same machine
uh = mdhelper_amd.ArrayUniverse(slab, dims)
measure("pageable host memory, 1 group", lambda: DensityProfile(uh.atoms, verbose=False), F_HOST)
