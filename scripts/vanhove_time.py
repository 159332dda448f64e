"""VanHove timing on one GPU: 32 768 points x VANHOVE_FRAMES frames (default 1 024) of float32 positions resident in
HBM, two groups, 64 lags, VANHOVE_BINS bins (default 201; a few wide bins put every displacement of a wave into one
or two of them at every lag), with ``unwrap``.  Two cases: short lags (0 ... 63 frames: nearly every
displacement of a tile falls into one or two bins, lag 0 all of them into one — the LDS-contention case) and long lags
(0, 8, ... 504 frames: the displacements spread over the bins and the history reaches far back).  Prints the device
time of the engine's kernels (``stats()["kernel_ms"]`` of ``mdx_vh_stats``, HIP events, median of VANHOVE_REPS runs
after a warm-up) and the evaluations (frame pairs x points) per second, then the wall time of ``VanHove(...).run()``
end to end from host memory.  The counts of the first frames are compared with ``numpy.histogram`` before anything is
printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import VanHove

N = 32768
SIZES = [N // 2, N - N // 2]
F = int(os.environ.get("VANHOVE_FRAMES", 1024))
F_HOST = min(F, int(os.environ.get("VANHOVE_HOST_FRAMES", 512)))
REPS = int(os.environ.get("VANHOVE_REPS", 5))
L = np.array([64.0, 64.0, 96.0])
EDGES = np.linspace(0.0, 15.0, int(os.environ.get("VANHOVE_BINS", 201)) + 1)
CASES = (("short lags", np.arange(64)), ("long lags", 8 * np.arange(64)))


def kernel_time(name, d, lags):
    eng = _core.VanHoveEngine(SIZES, EDGES, lags, timing=True)
    try:
        eng.set_unwrap(L)
        eng.accumulate_device(d.ptr, N, min(F, 8))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            counts, moments = eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        print(f"{name} [kernels only]: {F} frames of {N} points in {len(SIZES)} groups, {len(lags)} lags up to "
              f"{int(lags[-1])}, {len(EDGES) - 1} bins: median {t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, "
              f"{REPS} runs), {stats['evaluations']} evaluations, {stats['evaluations'] / t / 1e9:.2f} G evaluations/s",
              flush=True)
        return counts, moments
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk: every particle crosses faces
head = d.to_host(0, min(F, 4)).astype(np.float64)

# the first frames against numpy.histogram (steps far below L / 2: the minimum image is the unwrapped displacement)
check = _core.VanHoveEngine(SIZES, EDGES, [0, 1, 3])
check.set_unwrap(L)
check.accumulate_device(d.ptr, N, len(head))
got, _ = check.result()
check.close()
for k, lag in enumerate((0, 1, 3)):
    if lag >= len(head):
        continue
    dx = head[lag:] - head[:len(head) - lag]
    dx -= np.round(dx / L) * L
    r = np.sqrt((dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2])
    for g, lo in enumerate((0, SIZES[0])):
        want = np.histogram(r[:, lo:lo + SIZES[g]], len(EDGES) - 1, (EDGES[0], EDGES[-1]))[0]
        assert np.abs(got[k, g] - want).sum() <= 2, (lag, g)     # the image shift rounds: a count may move a bin

results = {name: kernel_time(name, d, lags) for name, lags in CASES}

host = d.to_host(0, F_HOST)
d.free()
u = mdhelper_amd.ArrayUniverse(host, [*L, 90.0, 90.0, 90.0])
groups = [u.select(np.arange(SIZES[0])), u.select(np.arange(SIZES[0], N))]
for name, lags in CASES:
    make = lambda: VanHove(groups, len(EDGES) - 1, (EDGES[0], EDGES[-1]), lags=lags, unwrap=True,      # noqa: E731
                           verbose=False)
    make().run(stop=min(F_HOST, 16))
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        v = make().run()
        times.append(time.perf_counter() - t0)
    if F_HOST == F:
        np.testing.assert_array_equal(v.results.counts, results[name][0])
    t = float(np.median(times))
    print(f"VanHove({name}, unwrap=True).run() from host memory: {F_HOST} frames: median {t * 1e3:.2f} ms "
          f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {REPS} runs), {F_HOST / t:.0f} frames/s",
          flush=True)
