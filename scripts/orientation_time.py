"""OrientationalRelaxation timing on one GPU, at the shape of scripts/vanhove_time.py: 32 768 vectors (point v to point
v + 1 of 32 768 wrapped random walkers, minimum image) x ORIENTATION_FRAMES frames (default 1 024) of float32 positions
resident in HBM, two groups, 64 lags.  Two cases: short lags (0 ... 63 frames) and long lags (0, 8, ... 504 frames:
the history reaches far back).  Prints the device time of the engine's kernels (``stats()["kernel_ms"]`` of
``mdx_ori_stats``, HIP events, median of ORIENTATION_REPS runs after a warm-up) and the evaluations (frame pairs x
vectors) per second, then the wall time of ``OrientationalRelaxation(...).run()`` end to end from host memory.  The
sums of the first frames are compared with NumPy before anything is printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import OrientationalRelaxation

N = 32768
SIZES = [N // 2, N - N // 2]
PAIRS = np.stack((np.arange(N), (np.arange(N) + 1) % N), axis=1).astype(np.int32)
F = int(os.environ.get("ORIENTATION_FRAMES", 1024))
F_HOST = min(F, int(os.environ.get("ORIENTATION_HOST_FRAMES", 512)))
REPS = int(os.environ.get("ORIENTATION_REPS", 5))
L = np.array([64.0, 64.0, 96.0])
CASES = (("short lags", np.arange(64)), ("long lags", 8 * np.arange(64)))


def kernel_time(name, d, lags):
    eng = _core.OrientationEngine(SIZES, PAIRS, N, lags, timing=True)
    try:
        eng.set_box(L)
        eng.accumulate_device(d.ptr, N, min(F, 8))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            sums = eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        print(f"{name} [kernels only]: {F} frames of {N} vectors in {len(SIZES)} groups, {len(lags)} lags up to "
              f"{int(lags[-1])}: median {t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs), "
              f"{stats['evaluations']} evaluations, {stats['evaluations'] / t / 1e9:.2f} G evaluations/s", flush=True)
        return sums
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk: every particle crosses faces
head = d.to_host(0, min(F, 4)).astype(np.float64)

# the first frames against NumPy (the order of the sums differs: a relative 1e-12)
check = _core.OrientationEngine(SIZES, PAIRS, N, [0, 1, 3])
check.set_box(L)
check.accumulate_device(d.ptr, N, len(head))
got, products = check.result(), check.frame_sums()
check.close()
w = head[:, PAIRS[:, 1]] - head[:, PAIRS[:, 0]]
w -= L * np.rint(w * (1.0 / L))
u = w / np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])[..., None]
for g, lo in enumerate((0, SIZES[0])):
    sl = slice(lo, lo + SIZES[g])
    for k, lag in enumerate((0, 1, 3)):
        if lag >= len(head):
            continue
        c = (u[lag:, sl] * u[:len(head) - lag, sl]).sum(axis=-1)
        assert np.allclose(got[k, g], [c.sum(), (1.5 * c * c - 0.5).sum()], rtol=1e-12, atol=1e-9), (lag, g)
    assert np.allclose(products[:, g, 5], (u[:, sl, 2] * u[:, sl, 2]).sum(axis=1), rtol=1e-12), g

results = {name: kernel_time(name, d, lags) for name, lags in CASES}

host = d.to_host(0, F_HOST)
d.free()
u = mdhelper_amd.ArrayUniverse(host, [*L, 90.0, 90.0, 90.0])
tails = [u.select(PAIRS[:SIZES[0], 0]), u.select(PAIRS[SIZES[0]:, 0])]
heads = [u.select(PAIRS[:SIZES[0], 1]), u.select(PAIRS[SIZES[0]:, 1])]
for name, lags in CASES:
    make = lambda: OrientationalRelaxation(tails, heads, lags=lags, verbose=False)      # noqa: E731
    make().run(stop=min(F_HOST, 16))
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        o = make().run()
        times.append(time.perf_counter() - t0)
    if F_HOST == F:
        terms = np.maximum(F - lags, 0)[:, None] * np.array(SIZES)[None, :]
        np.testing.assert_array_equal(o.results.c1, results[name][..., 0] / terms)
    t = float(np.median(times))
    print(f"OrientationalRelaxation({name}).run() from host memory: {F_HOST} frames: median {t * 1e3:.2f} ms "
          f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {REPS} runs), {F_HOST / t:.0f} frames/s",
          flush=True)
