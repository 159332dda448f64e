"""FourPointSusceptibility timing on one GPU, at the shape of scripts/vanhove_time.py: 32 768 points x FOURPOINT_FRAMES
frames (default 1 024) of float32 positions resident in HBM, two groups, 64 lags, with ``unwrap``, every frame an
origin.  Two lag cases (short lags 0 ... 63 frames, long lags 0, 8, ... 504 frames), each with one cutoff and with
three.  Prints the device time of the engine's kernels (``stats()["kernel_ms"]`` of ``mdx_chi4_stats``, HIP events,
median of FOURPOINT_REPS runs after a warm-up) and the evaluations (frame pairs x points) per second, then the wall
time of ``FourPointSusceptibility(...).run()`` end to end from host memory.  The sums of the first frames are compared
with a NumPy restatement before anything is printed.  FOURPOINT_SEGMENT sets the point segment (0: the default).

The yardstick is scripts/vanhove_time.py in the same job: per evaluation the van Hove kernel does strictly more."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import FourPointSusceptibility

N = 32768
SIZES = [N // 2, N - N // 2]
F = int(os.environ.get("FOURPOINT_FRAMES", 1024))
F_HOST = min(F, int(os.environ.get("FOURPOINT_HOST_FRAMES", 512)))
REPS = int(os.environ.get("FOURPOINT_REPS", 5))
SEGMENT = int(os.environ.get("FOURPOINT_SEGMENT", 0))
L = np.array([64.0, 64.0, 96.0])
CUTOFF_SETS = ((1.0,), (0.5, 1.0, 2.0))             # a step is 0.3 per component: Q_s falls through 1/e inside the lags
CASES = (("short lags", np.arange(64)), ("long lags", 8 * np.arange(64)))


def kernel_time(name, d, lags, cutoffs):
    eng = _core.FourPointEngine(SIZES, cutoffs, lags, timing=True)
    try:
        eng.set_unwrap(L)
        eng.set_segment_points(SEGMENT)
        eng.accumulate_device(d.ptr, N, min(F, 8))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            result = eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        print(f"{name}, {len(cutoffs)} cutoff(s) [kernels only]: {F} frames of {N} points in {len(SIZES)} groups, "
              f"{len(lags)} lags up to {int(lags[-1])}: median {t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, "
              f"{REPS} runs), {stats['evaluations']} evaluations, {stats['evaluations'] / t / 1e9:.2f} G evaluations/s",
              flush=True)
        return result
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk: every particle crosses faces
head = d.to_host(0, min(F, 4)).astype(np.float64)

# the first frames against NumPy (steps far below L / 2: the minimum image is the unwrapped displacement; the image
# shift rounds, so a point within an ulp of a cutoff may fall on the other side)
check = _core.FourPointEngine(SIZES, CUTOFF_SETS[1], [0, 1, 3])
check.set_unwrap(L)
check.accumulate_device(d.ptr, N, len(head))
got, got2, origins = check.result()
check.close()
for k, lag in enumerate((0, 1, 3)):
    if lag >= len(head):
        continue
    dx = head[lag:] - head[:len(head) - lag]
    dx -= np.round(dx / L) * L
    r2 = (dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2]
    assert origins[k] == len(head) - lag
    for g, lo in enumerate((0, SIZES[0])):
        for c, a in enumerate(CUTOFF_SETS[1]):
            q = (r2[:, lo:lo + SIZES[g]] <= a * a).sum(axis=1)
            assert abs(int(got[k, g, c]) - int(q.sum())) <= 2, (lag, g, c)
            assert abs(int(got2[k, g, c]) - int((q * q).sum())) <= 4 * SIZES[g] * len(q), (lag, g, c)

results = {(name, len(cutoffs)): kernel_time(name, d, lags, cutoffs) for name, lags in CASES for cutoffs in CUTOFF_SETS}
for name, _ in CASES:           # the cutoff 1.0 is in both sets: the same sums
    np.testing.assert_array_equal(results[name, 1][0][..., 0], results[name, 3][0][..., 1])
    np.testing.assert_array_equal(results[name, 1][1][..., 0], results[name, 3][1][..., 1])

host = d.to_host(0, F_HOST)
d.free()
u = mdhelper_amd.ArrayUniverse(host, [*L, 90.0, 90.0, 90.0])
groups = [u.select(np.arange(SIZES[0])), u.select(np.arange(SIZES[0], N))]
for name, lags in CASES:
    make = lambda: FourPointSusceptibility(groups, CUTOFF_SETS[1], lags=lags, unwrap=True, verbose=False)  # noqa: E731
    make().run(stop=min(F_HOST, 16))
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        v = make().run()
        times.append(time.perf_counter() - t0)
    if F_HOST == F:
        np.testing.assert_array_equal(v.results.sums, results[name, 3][0])
    t = float(np.median(times))
    print(f"FourPointSusceptibility({name}, 3 cutoffs, unwrap=True).run() from host memory: {F_HOST} frames: median "
          f"{t * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {REPS} runs), "
          f"{F_HOST / t:.0f} frames/s", flush=True)
v.calculate_relaxation_times()
print("tau_alpha [group, cutoff] (ps):", np.round(v.results.relaxation_time, 3).tolist(), " chi4 peak:",
      np.round(v.results.peak_height, 3).tolist(), "at", np.round(v.results.peak_time, 3).tolist(), flush=True)
