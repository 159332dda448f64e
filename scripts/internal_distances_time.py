"""Internal-distance timing on one GPU: 1 000 chains x 100 monomers, MSID_FRAMES frames (default 2 000) of
HBM-resident float32.  Prints ``stats()["kernel_ms"]`` of the internal-distance engine (HIP events, one run after a
warm-up) with the pair terms per second it amounts to (M * N (N - 1) / 2 distance terms per frame; as many cosine terms
ride along), and beside it the same figure of the gyration engine on the same frames, which makes one
O(N) pass over the same bytes.  The rows of the first frames are compared with the NumPy restatement of the
definitions before anything is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

M, N_P = 1000, 100
N = M * N_P
F = int(os.environ.get("MSID_FRAMES", 2000))
L = np.array([80.0, 80.0, 80.0])
HEAD = 2

d = _core.synth_random_walk(F, N, L, 0.3, 7, wrap=False)
masses = np.random.default_rng(0).uniform(1.0, 20.0, N)
pair_terms = M * N_P * (N_P - 1) / 2 * F


def restated(points):
    """float64 [F, M, N_P, 3] -> [F, 2, N_P - 1]: the terms of every separation added one after the other over (c, i)."""
    def norm2(v):
        return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]

    b = points[:, :, 1:] - points[:, :, :-1]
    bb = norm2(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((bb == 0.0)[..., None], 0.0, b / np.sqrt(bb)[..., None])
    r2, cos = np.zeros((len(points), N_P - 1)), np.zeros((len(points), N_P - 1))
    for c in range(M):
        for i in range(N_P - 1):
            r2[:, :N_P - 1 - i] += norm2(points[:, c, i + 1:] - points[:, c, i:i + 1])
            ui, uj = u[:, c, i:i + 1], u[:, c, i:]
            cos[:, :N_P - 1 - i] += (ui[..., 0] * uj[..., 0] + ui[..., 1] * uj[..., 1]) + ui[..., 2] * uj[..., 2]
    s = np.arange(1, N_P)
    return np.stack((r2 / (M * (N_P - s)), cos / (M * (N_P - s))), axis=1)


def run(eng):
    try:
        eng.accumulate_device(d.ptr, N, min(F, 64))          # warm-up: pools, streams, code objects
        eng.reset()
        eng.accumulate_device(d.ptr, N, F)
        return eng.stats()["kernel_ms"], eng.result()
    finally:
        eng.close()


ms, (rows,) = run(_core.InternalDistanceEngine([M], [N_P], timing=True))
want = restated(d.to_host(0, HEAD).astype(np.float64).reshape(HEAD, M, N_P, 3))
# both sides add at most M N terms per separation in float64: the bounds of tests/test_gpu_internal_distances.py
np.testing.assert_allclose(rows[:HEAD, 0], want[:, 0], rtol=16 * (N + 8) * 2.0 ** -53, atol=0)
np.testing.assert_allclose(rows[:HEAD, 1], want[:, 1], rtol=0, atol=16 * (N + 16) * 2.0 ** -53)
print(f"internal distances: {F} frames of {M} x {N_P} monomers: kernel_ms = {ms:.3f} (one run), "
      f"{pair_terms / ms / 1e6:.1f} G pair terms/s, {12.0 * N * F / ms / 1e6:.0f} GB/s of positions read", flush=True)
ms_gyr, _ = run(_core.GyrationEngine([M], [N_P], masses, timing=True))
print(f"gyration: the same frames: kernel_ms = {ms_gyr:.3f} (one run), "
      f"{12.0 * N * F / ms_gyr / 1e6:.0f} GB/s of positions read", flush=True)
d.free()
