"""SingleChainStructureFactor timing on one GPU: a bead-spring-like melt of 500 chains x 64 beads (32 000 beads) on
the default 32^3 wavevector grid, frames resident in HBM; StructureFactor (mode=None) on the same frames and grid in
the same process.  Prints frames/s and terms/s (wavevectors x beads per frame) of both, their ratio, and the
per-frame time of the float64 NumPy restatement on one core for one frame."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import SingleChainStructureFactor, StructureFactor

M, NP, F, L, NPTS = 500, 64, int(os.environ.get("SCSF_FRAMES", 512)), 34.2, 32
rng = np.random.default_rng(0)
start = rng.random((F, M, 1, 3)) * L
steps = rng.normal(0, 0.97 / np.sqrt(3), (F, M, NP, 3))
pos = np.mod(start + np.cumsum(steps, axis=2), L).reshape(F, M * NP, 3).astype(np.float32)
dims = [L, L, L, 90, 90, 90]
n_q, N = NPTS ** 3, M * NP
d = _core.DeviceArray.from_host(pos)
u = mdhelper_amd.ArrayUniverse.from_device(d, dims)


def timed(make, reps=3):
    make().run(stop=8)                                   # warm-up: plans, LDS attributes, pools
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        make().run()
        best = min(best, time.perf_counter() - t0)
    return best


t_sc = timed(lambda: SingleChainStructureFactor(u.atoms, n_points=NPTS, n_chains=M, n_monomers=NP))
t_sf = timed(lambda: StructureFactor(u.atoms, n_points=NPTS))
d.free()
for name, t in (("SingleChainStructureFactor", t_sc), ("StructureFactor(mode=None)", t_sf)):
    print(f"{name}: {F} frames of {N} beads, {n_q} wavevectors: {t * 1e3:.1f} ms, {F / t:.0f} frames/s, "
          f"{F * n_q * N / t:.3e} terms/s")
print(f"ratio (single-chain / StructureFactor terms/s): {t_sf / t_sc:.3f}")

# the float64 NumPy restatement, one frame, one core
q = np.stack(np.meshgrid(*[2 * np.pi * np.arange(NPTS) / L] * 3), -1).reshape(-1, 3)
t0 = time.perf_counter()
acc = np.zeros(n_q)
for c in range(M):
    qr = pos[0, c * NP:(c + 1) * NP].astype(float) @ q.T
    acc += np.cos(qr).sum(axis=0) ** 2 + np.sin(qr).sum(axis=0) ** 2
t_np = time.perf_counter() - t0
print(f"NumPy restatement (one core, float64): {t_np:.2f} s per frame; GPU speed-up {t_np / (t_sc / F):.3g} x")
