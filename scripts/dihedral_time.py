"""Dihedrals timing on one GPU: DIHEDRAL_CHAINS chains (default 1 000) of 100 monomers, their 97 backbone dihedrals
each (97 000 in all), DIHEDRAL_FRAMES frames (default 1 000) of float32 positions resident in HBM (wrapped random
walkers, minimum image: the geometry has no meaning, the work is the same), 180 bins, three states, lags 0 ... 99.
Prints the device time of the engine's kernels (``stats()["kernel_ms"]`` of ``mdx_dih_stats``, HIP events, median of
DIHEDRAL_REPS runs after a warm-up) and the evaluations (frame pairs x dihedrals) per second; then, in the same
process and with the same pattern, the orientation engine on the 99 000 bonds of the same chains with the same lags
as the yardstick (its correlate kernel has the same shape), and the ratio per (row, lag, frame); then the wall time of
``Dihedrals.from_chains(...).run()`` end to end from host memory.  The results of the first frames are compared with
NumPy before anything is printed.  The share of each kernel comes from a kernel trace of this script
(``rocprofv3 --kernel-trace --stats``)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import Dihedrals
from mdhelper_amd.analysis.dihedral import cosine_thresholds, states_of_bins

CHAINS = int(os.environ.get("DIHEDRAL_CHAINS", 1000))
MONOMERS = 100
N = CHAINS * MONOMERS
F = int(os.environ.get("DIHEDRAL_FRAMES", 1000))
F_HOST = min(F, int(os.environ.get("DIHEDRAL_HOST_FRAMES", 250)))
REPS = int(os.environ.get("DIHEDRAL_REPS", 5))
L = np.array([64.0, 64.0, 96.0])
LAGS = np.arange(100)
PLACE = np.arange(N).reshape(CHAINS, MONOMERS)
QUADS = np.stack([PLACE[:, i:MONOMERS - 3 + i].ravel() for i in range(4)], axis=1).astype(np.int32)
BONDS = np.stack((PLACE[:, :-1].ravel(), PLACE[:, 1:].ravel()), axis=1).astype(np.int32)
THRESHOLDS, STATES = cosine_thresholds(180), states_of_bins(180, (-120.0, 0.0, 120.0))


def dihedral_engine(lags, timing=False):
    eng = _core.DihedralEngine([len(QUADS)], QUADS, N, THRESHOLDS, STATES, lags, n_states=3, timing=timing)
    eng.set_box(L)
    return eng


def orientation_engine(lags, timing=False):
    eng = _core.OrientationEngine([len(BONDS)], BONDS, N, lags, timing=timing)
    eng.set_box(L)
    return eng


def kernel_time(name, make, rows, d):
    eng = make(LAGS, timing=True)
    try:
        eng.accumulate_device(d.ptr, N, min(F, 8))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        print(f"{name} [kernels only]: {F} frames of {rows} rows, {len(LAGS)} lags up to {int(LAGS[-1])}, slab "
              f"{eng.plan()['slab_frames']}: median {t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} "
              f"runs), "
              f"{stats['evaluations']} evaluations, {stats['evaluations'] / t / 1e9:.2f} G evaluations/s", flush=True)
        return t / stats["evaluations"]
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk: every particle crosses faces
head = d.to_host(0, min(F, 4)).astype(np.float64)

# the first frames against NumPy (the order of the sums differs: a relative 1e-12)
check = dihedral_engine([0, 1, 3])
check.accumulate_device(d.ptr, N, len(head))
got, counts, moves = check.result(), check.counts(), check.transitions()
check.close()


def cross(a, b):
    return np.stack(((a[..., 1] * b[..., 2]) - (a[..., 2] * b[..., 1]),
                     (a[..., 2] * b[..., 0]) - (a[..., 0] * b[..., 2]),
                     (a[..., 0] * b[..., 1]) - (a[..., 1] * b[..., 0])), axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


b1, b2, b3 = (head[:, QUADS[:, i + 1]] - head[:, QUADS[:, i]] for i in range(3))
b1, b2, b3 = (b - L * np.rint(b * (1.0 / L)) for b in (b1, b2, b3))
m, n = cross(b1, b2), cross(b2, b3)
den = np.sqrt(dot(m, m) * dot(n, n))
c, s, q = dot(m, n) / den, (np.sqrt(dot(b2, b2)) * dot(b1, n)) / den, dot(b1, n)
above = np.searchsorted(-THRESHOLDS[1:90], -c, side="right")
bins = np.where(q < 0, 89 - above, 90 + above)
state = STATES[bins]
assert np.array_equal(counts[0], np.bincount(bins.ravel(), minlength=180))
want = np.zeros((3, 3), dtype=np.int64)
np.add.at(want, (state[:-1].ravel(), state[1:].ravel()), 1)
assert np.array_equal(moves[0], want)
for k, lag in enumerate((0, 1, 3)):
    if lag < len(head):
        terms = c[lag:] * c[:len(head) - lag] + s[lag:] * s[:len(head) - lag]
        assert np.allclose(got["sums"][k, 0], terms.sum(), rtol=1e-12, atol=1e-9), lag
        assert got["same"][k, 0] == (state[lag:] == state[:len(head) - lag]).sum(), lag

per_dihedral = kernel_time("dihedrals", dihedral_engine, len(QUADS), d)
per_bond = kernel_time("orientation (yardstick)", orientation_engine, len(BONDS), d)
print(f"kernel time per (row, lag, frame): dihedrals {per_dihedral * 1e12:.3f} ps, "
      f"orientation {per_bond * 1e12:.3f} ps, ratio {per_dihedral / per_bond:.3f}", flush=True)

host = d.to_host(0, F_HOST)
d.free()
u = mdhelper_amd.ArrayUniverse(host, [*L, 90.0, 90.0, 90.0])
ag = u.select(np.arange(N))
new = lambda: Dihedrals.from_chains(ag, CHAINS, MONOMERS, lags=LAGS, verbose=False)      # noqa: E731
new().run(stop=min(F_HOST, 16))
times = []
for _ in range(REPS):
    t0 = time.perf_counter()
    new().run()
    times.append(time.perf_counter() - t0)
t = float(np.median(times))
print(f"Dihedrals.from_chains(...).run() from host memory: {F_HOST} frames: median {t * 1e3:.2f} ms "
      f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {REPS} runs), {F_HOST / t:.0f} frames/s", flush=True)
