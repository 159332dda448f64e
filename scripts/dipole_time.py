"""DipoleMoment timing on one GPU: 32 768 atoms x DIPOLE_FRAMES frames (default 10 000) of float32 positions resident
in HBM, two groups, with and without ``unwrap``.  Prints the device time of the dipole engine's kernels
(``stats()["kernel_ms"]``, HIP events, median of DIPOLE_REPS runs after a warm-up), the rate they reach at 12 B per
atom-frame in GB/s, that rate as a fraction of the device's copy bandwidth (DIPOLE_COPY_TBS in TB/s: what
``scripts/hbm_bench.hip`` printed for "copy" on the same device; default 6.3, the figure DESIGN.md carries), and the
wall time of ``DipoleMoment(...).run()`` end to end from host memory.  The engine's rows are compared with the NumPy
sum of the first frames before anything is printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DipoleMoment

N = 32768
SIZES = [N // 2, N - N // 2]
F = int(os.environ.get("DIPOLE_FRAMES", 10000))
F_HOST = min(F, int(os.environ.get("DIPOLE_HOST_FRAMES", 2000)))
REPS = int(os.environ.get("DIPOLE_REPS", 7))
COPY_RATE = float(os.environ.get("DIPOLE_COPY_TBS", 6.3)) * 1e12
L = np.array([64.0, 64.0, 96.0])
dims = [*L, 90.0, 90.0, 90.0]


def kernel_time(name, d, charges, unwrap_start=None):
    eng = _core.DipoleEngine(SIZES, charges, timing=True)
    try:
        if unwrap_start is not None:
            eng.set_unwrap(L, unwrap_start)
        eng.accumulate_device(d.ptr, N, min(F, 64))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            ms.append(eng.stats()["kernel_ms"])
            rows = eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        rate = 12.0 * N * F / t
        print(f"{name} [kernels only]: {F} frames of {N} atoms in {len(SIZES)} groups, tiles of {eng.TILE}: median "
              f"{t * 1e3:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs), {F / t:.0f} frames/s, "
              f"{rate / 1e9:.0f} GB/s = {rate / COPY_RATE:.2f} of the copy bandwidth ({COPY_RATE / 1e12:.2f} TB/s)",
              flush=True)
        return rows
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk: every particle crosses faces
charges = np.random.default_rng(0).normal(size=N)
head = d.to_host(0, min(F, 8))

rows = kernel_time("HBM", d, charges)
lo = 0
for g, n in enumerate(SIZES):
    terms = charges[lo:lo + n, None] * head[:, lo:lo + n].astype(np.float64)
    bound = n * 2.0 ** -52 * np.abs(terms).sum(axis=1)
    assert np.all(np.abs(rows[g, :len(head)] - terms.sum(axis=1)) <= 2 * bound)
    lo += n
unwrapped = kernel_time("HBM, unwrap", d, charges, unwrap_start=head[0].astype(np.float64))
assert np.abs(unwrapped[:, -1] - rows[:, -1]).max() > 1.0     # the walk left the box: another answer

host = d.to_host(0, F_HOST)
d.free()
u = mdhelper_amd.ArrayUniverse(host, dims, charges=charges)
groups = [u.select(np.arange(SIZES[0])), u.select(np.arange(SIZES[0], N))]
for unwrap in (False, True):
    DipoleMoment(groups, unwrap=unwrap, verbose=False).run(stop=min(F_HOST, 64))
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        m = DipoleMoment(groups, unwrap=unwrap, verbose=False).run()
        times.append(time.perf_counter() - t0)
    np.testing.assert_array_equal(m.results.dipoles.transpose(1, 0, 2), (unwrapped if unwrap else rows)[:, :F_HOST])
    t = float(np.median(times))
    print(f"DipoleMoment(unwrap={unwrap}).run() from host memory: {F_HOST} frames: median {t * 1e3:.2f} ms "
          f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}, {REPS} runs), {F_HOST / t:.0f} frames/s, "
          f"{12.0 * N * F_HOST / t / 1e9:.1f} GB/s", flush=True)
