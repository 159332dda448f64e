"""Chain-projection timing on one GPU: 1 000 chains x 100 monomers, 10 Rouse modes, ROUSE_FRAMES frames (default
2 000) of HBM-resident float32.  Prints ``stats()["kernel_ms"]`` of the projection engine (HIP events, one run after a
warm-up) with the GB/s the 12 B x atoms x frames it reads amount to, and beside it the same figure of the gyration
engine, which makes the same one pass over the same bytes.  The amplitudes of the first frames are compared with
the sequential NumPy sum before anything is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

M, N_P, P = 1000, 100, 10
N = M * N_P
F = int(os.environ.get("ROUSE_FRAMES", 2000))
L = np.array([80.0, 80.0, 80.0])

d = _core.synth_random_walk(F, N, L, 0.3, 7, wrap=False)
w = np.stack([np.cos(np.pi * p * (np.arange(N_P) + 0.5) / N_P) / N_P for p in range(1, P + 1)])
masses = np.random.default_rng(0).uniform(1.0, 20.0, N)
bytes_read = 12.0 * N * F


def report(name, eng):
    try:
        eng.accumulate_device(d.ptr, N, min(F, 64))          # warm-up: pools, streams, code objects
        eng.reset()
        eng.accumulate_device(d.ptr, N, F)
        ms = eng.stats()["kernel_ms"]
        out = eng.result()
        print(f"{name}: {F} frames of {M} x {N_P} monomers: kernel_ms = {ms:.3f} (one run), "
              f"{bytes_read / ms / 1e6:.0f} GB/s of positions read", flush=True)
        return out
    finally:
        eng.close()


amps = report(f"projection, {P} modes", _core.ChainProjectionEngine([M], [N_P], [w], timing=True))
head = d.to_host(0, 4).astype(np.float64).reshape(4, M, N_P, 3)
acc = np.zeros((4, P, M, 3))
for n in range(N_P):
    acc = acc + w[None, :, n, None, None] * head[:, None, :, n, :]
np.testing.assert_array_equal(amps[:4], acc.reshape(4, P * M, 3))
report("gyration", _core.GyrationEngine([M], [N_P], masses, timing=True))
d.free()
