"""Gyradius timing on one GPU: 500 chains x 64 monomers x GYRADIUS_FRAMES frames (default 4 000), HBM-resident
float32 frames.  Prints three numbers: the device time of the gyration engine's kernels (``stats()["kernel_ms"]``, HIP
events, median of GYRADIUS_REPS runs after a warm-up), the time the same 12 B x atoms x frames need at the 6.3 TB/s
the HBM reads at when streamed, and the wall time of the NumPy restatement of the reference's per-frame work on the
host (over GYRADIUS_HOST_FRAMES frames, scaled to all frames).  Also the wall time of ``Gyradius(...).run()`` and the
same kernels with ``unwrap``.  The two sets of radii are compared before anything is printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.algorithm.molecule import radius_of_gyration
from mdhelper_amd.analysis import Gyradius

M, N_P = 500, 64
N = M * N_P
F = int(os.environ.get("GYRADIUS_FRAMES", 4000))
F_HOST = min(F, int(os.environ.get("GYRADIUS_HOST_FRAMES", 200)))
REPS = int(os.environ.get("GYRADIUS_REPS", 7))
HBM_RATE = 6.3e12
L = np.array([80.0, 80.0, 80.0])
dims = [*L, 90.0, 90.0, 90.0]


def host_restatement(frames, masses):
    """The reference's Gyradius._single_frame per frame: float64 [F] mean radius over the chains."""
    m = masses.reshape(M, N_P)
    return np.array([radius_of_gyration(grouping="segments", positions=x.reshape(M, N_P, 3), masses=m).mean()
                     for x in frames])


def kernel_time(name, d, masses, unwrap_start=None):
    eng = _core.GyrationEngine([M], [N_P], masses, timing=True)
    try:
        if unwrap_start is not None:
            eng.set_unwrap(L, unwrap_start)
        eng.accumulate_device(d.ptr, N, min(F, 64))          # warm-up: pools, streams, code objects
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            ms.append(eng.stats()["kernel_ms"])
            radii = eng.result()
            eng.reset()
        t = float(np.median(ms)) * 1e-3
        floor = 12.0 * N * F / HBM_RATE
        print(f"{name} [kernels only]: {F} frames of {M} x {N_P} monomers: median {t * 1e3:.3f} ms "
              f"(min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs), {F / t:.0f} frames/s, "
              f"{12.0 * N * F / t / 1e12:.3f} TB/s; the same bytes at {HBM_RATE / 1e12:.1f} TB/s: {floor * 1e3:.3f} ms "
              f"-> {floor / t:.2f} of the floor", flush=True)
        return radii
    finally:
        eng.close()


d = _core.synth_random_walk(F, N, L, 0.3, 7, wrap=False)   # every particle diffuses: chains of 64 consecutive ones
masses = np.random.default_rng(0).uniform(1.0, 20.0, N)
head = d.to_host(0, F_HOST)

t0 = time.perf_counter()
want = host_restatement(head, masses)
t_host = time.perf_counter() - t0

radii = kernel_time("HBM", d, masses)
err = np.abs(radii[0, :F_HOST, 0] / want - 1).max()
assert err < 1e-11, err
kernel_time("HBM, unwrap", d, masses, unwrap_start=head[0].astype(np.float64))

u = mdhelper_amd.ArrayUniverse.from_device(d, dims, masses=masses)
Gyradius(u.atoms, n_chains=M, n_monomers=N_P, verbose=False).run(stop=min(F, 64))
times = []
for _ in range(REPS):
    t0 = time.perf_counter()
    g = Gyradius(u.atoms, n_chains=M, n_monomers=N_P, verbose=False).run()
    times.append(time.perf_counter() - t0)
np.testing.assert_array_equal(g.results.gyradii, radii[..., 0])
print(f"Gyradius(...).run(): median {np.median(times) * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, "
      f"max {max(times) * 1e3:.2f}, {REPS} runs), {F / np.median(times):.0f} frames/s", flush=True)
print(f"NumPy restatement on the host: {t_host * 1e3:.1f} ms for {F_HOST} frames = {t_host / F_HOST * 1e3:.3f} ms "
      f"per frame -> {t_host / F_HOST * F * 1e3:.0f} ms for {F} frames; largest relative difference to the device "
      f"over these frames {err:.1e}", flush=True)
d.free()
