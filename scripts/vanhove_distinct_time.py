"""DistinctVanHove timing on one GPU: VHD_POINTS points (default 8 192) x VHD_FRAMES frames (default 64) of float32
positions resident in HBM, one set against itself, VHD_LAGS lags 0 ... (default 8), VHD_BINS bins up to 15 A (default
201), every frame an origin.  Two timings over the same frame pairs:

(a) the engine: the device time of its kernels (``stats()["kernel_ms"]`` of ``mdx_vhd_stats``, HIP events, median of
    VHD_REPS runs after a warm-up) and the pair distances of the contract (``stats()["evaluations"]``) per second;
(b) the loop a user writes without the engine: ``radial_histogram(pos[f0], pos[f0 + lag], ..., exclusion=(1, 1))`` of
    the public API once per frame pair, wall time of the whole loop ending in its last (synchronous) call, median of
    VHD_REPS runs after a warm-up.

The two have different contracts (the histogram of (b) forms float32 differences, takes ``(r0, r1]`` bins and culls by
cells; (a) is the float64 ``numpy.histogram`` contract and evaluates every pair), so the counts may differ by a few
pairs next to a bin edge and no ratio is asserted.  The engine's counts of the first frames are compared with
``numpy.histogram`` before anything is printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core
from mdhelper_amd.analysis.structure import radial_histogram

N = int(os.environ.get("VHD_POINTS", 8192))
F = int(os.environ.get("VHD_FRAMES", 64))
LAGS = np.arange(int(os.environ.get("VHD_LAGS", 8)))
N_BINS = int(os.environ.get("VHD_BINS", 201))
REPS = int(os.environ.get("VHD_REPS", 5))
L = np.array([48.0, 48.0, 48.0])
R_MAX = 15.0
EDGES = np.linspace(0.0, R_MAX, N_BINS + 1)
PAIRS = [(f0, f0 + int(lag)) for lag in LAGS for f0 in range(F - int(lag))]

d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk
host = d.to_host(0, F)

# the first frames against numpy.histogram, with the contract's arithmetic
n_check = min(N, 1024)
head = host[:min(F, 3), :n_check]
check = _core.DistinctVanHoveEngine(n_check, n_check, EDGES, [0, 2], L, same=True)
check.accumulate(head)
got = check.result()
check.close()
x = head.astype(np.float64)
for k, lag in enumerate((0, 2)):
    rs = []
    for f0 in range(len(x) - lag):
        dx = x[f0 + lag][None, :, :] - x[f0][:, None, :]
        s = dx * (1.0 / L)
        w = dx - L * np.rint(s)
        r = np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])
        rs.append(r[~np.eye(n_check, dtype=bool)])
    if rs:
        np.testing.assert_array_equal(got[k], np.histogram(np.concatenate(rs), N_BINS, (0.0, R_MAX))[0])

# (a) the engine
eng = _core.DistinctVanHoveEngine(N, N, EDGES, LAGS, L, same=True, timing=True)
try:
    eng.accumulate_device(d.ptr, N, min(F, int(LAGS[-1]) + 2))      # warm-up: pools, streams, code objects
    eng.reset()
    ms = []
    for _ in range(REPS):
        eng.accumulate_device(d.ptr, N, F)
        stats = eng.stats()
        ms.append(stats["kernel_ms"])
        counts = eng.result()
        eng.reset()
finally:
    eng.close()
d.free()
assert stats["evaluations"] == len(PAIRS) * N * (N - 1)
t = float(np.median(ms)) * 1e-3
print(f"(a) DistinctVanHoveEngine [kernels only]: {F} frames of {N} points, {len(LAGS)} lags up to {int(LAGS[-1])}, "
      f"{len(PAIRS)} frame pairs, {N_BINS} bins: median {t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, "
      f"{REPS} runs), {stats['evaluations']} pair distances, {stats['evaluations'] / t / 1e12:.3f} T pair distances/s",
      flush=True)

# (b) one radial_histogram call per frame pair
box = [*L, 90.0, 90.0, 90.0]
for f0, f1 in PAIRS[:4]:
    radial_histogram(host[f0], host[f1], N_BINS, (0.0, R_MAX), box, exclusion=(1, 1))
times = []
for _ in range(REPS):
    loop = np.zeros((len(LAGS), N_BINS), dtype=np.int64)
    t0 = time.perf_counter()
    for f0, f1 in PAIRS:
        loop[f1 - f0] += radial_histogram(host[f0], host[f1], N_BINS, (0.0, R_MAX), box, exclusion=(1, 1))
    times.append(time.perf_counter() - t0)
t = float(np.median(times))
moved = int(np.abs(loop - counts).sum())
print(f"(b) radial_histogram loop [wall]: {len(PAIRS)} calls: median {t * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, "
      f"max {max(times) * 1e3:.2f}, {REPS} runs), {t / len(PAIRS) * 1e3:.3f} ms per call; its counts differ from the "
      f"engine's by {moved} of {int(counts.sum())} (float32 differences and (r0, r1] bins against the float64 "
      f"numpy.histogram contract)", flush=True)
