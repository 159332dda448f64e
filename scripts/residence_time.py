"""PairResidence timing on one GPU: PRS_POINTS points (default 8 192) x PRS_FRAMES frames (default 64) of float32
positions resident in HBM, one set against itself, cutoff PRS_CUTOFF (default 2 A in a 48 A box: two to three contacts a
row), every frame an origin.  Device time of the kernels (``stats()["kernel_ms"]``, HIP events), medians of PRS_REPS
runs after a warm-up, all in one process on the same frames:

(a) the pair residence engine with lag 0 only: prepare + contact kernel (+ a walk over lag distance 0, which tests
    no membership); the contract's pair evaluations (``stats()["evaluations"]``) per second;
(b) the yardstick: the distinct van Hove engine (``vhd_pair_kernel``) with lag 0 only on the same frames, with its
    default histogram (201 bins up to 15 A) and with one bin up to the cutoff; the contact kernel issues a strict
    subset of that kernel's float64 instructions (no square root, no bin rule);
(c) the pair residence engine with lags 0 ... PRS_LAGS - 1 (default 64): the walk kernel's time is (c) - (a);
    and the same without ``continuous``.

The engine's results for the first frames are compared with a NumPy restatement before anything is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

N = int(os.environ.get("PRS_POINTS", 8192))
F = int(os.environ.get("PRS_FRAMES", 64))
N_LAGS = int(os.environ.get("PRS_LAGS", 64))
CUTOFF = float(os.environ.get("PRS_CUTOFF", 2.0))
REPS = int(os.environ.get("PRS_REPS", 5))
L = np.array([48.0, 48.0, 48.0])
LAGS = np.arange(min(N_LAGS, F))

d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk
host = d.to_host(0, F)

# the first frames against the restatement, with the contract's arithmetic
n_check = min(N, 1024)
head = host[:min(F, 4), :n_check]
check = _core.PairResidenceEngine(n_check, n_check, CUTOFF, [0, 1, 3], L, same=True)
check.accumulate(head)
got, contacts = check.result(), check.contacts()
check.close()
x = head.astype(np.float64)
dx = x[:, None, :, :] - x[:, :, None, :]
w = dx - L * np.rint(dx * (1.0 / L))
h = ((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2] <= CUTOFF * CUTOFF) \
    & ~np.eye(n_check, dtype=bool)
np.testing.assert_array_equal(contacts, h.sum(axis=(1, 2)))
for k, lag in enumerate((0, 1, 3)):
    o = range(len(x) - lag)
    np.testing.assert_array_equal(
        [got["origin_counts"][k], got["intermittent"][k], got["continuous"][k]],
        [sum(h[f].sum() for f in o), sum((h[f] & h[f + lag]).sum() for f in o),
         sum(np.logical_and.reduce(h[f:f + lag + 1]).sum() for f in o)])


def timed(eng, label):
    """Median device time of REPS passes over the resident frames after a warm-up; prints one line."""
    try:
        eng.accumulate_device(d.ptr, N, min(F, 4))          # warm-up: pools, streams, code objects
        eng.synchronize()
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            eng.result()
            eng.reset()
    finally:
        eng.close()
    t = float(np.median(ms))
    print(f"{label}: median {t:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs)", end="", flush=True)
    return t, stats


print(f"{F} frames of {N} points, one set, box {L[0]:g} A, cutoff {CUTOFF:g} A")
t_a, stats = timed(_core.PairResidenceEngine(N, N, CUTOFF, [0], L, same=True, timing=True),
                   "(a) PairResidenceEngine, lag 0 only [prepare + contact (+ walk at distance 0)]")
assert stats["evaluations"] == F * N * (N - 1)
print(f", {stats['evaluations']} pair evaluations, {stats['evaluations'] / t_a / 1e9:.3f} T pair evaluations/s, "
      f"largest row {stats['max_row']}")
for label, edges in (("201 bins up to 15 A", np.linspace(0.0, 15.0, 202)),
                     (f"1 bin up to {CUTOFF:g} A", np.array([0.0, CUTOFF]))):
    t_b, vstats = timed(_core.DistinctVanHoveEngine(N, N, edges, [0], L, same=True, timing=True),
                        f"(b) DistinctVanHoveEngine, lag 0 only, {label} [prepare + vhd_pair_kernel]")
    assert vstats["evaluations"] == stats["evaluations"]
    print(f", {vstats['evaluations'] / t_b / 1e9:.3f} T pair distances/s; (b) / (a) = {t_b / t_a:.2f}")
t_c, _ = timed(_core.PairResidenceEngine(N, N, CUTOFF, LAGS, L, same=True, timing=True),
               f"(c) PairResidenceEngine, lags 0 ... {int(LAGS[-1])}")
print(f"; walk kernel (c) - (a) = {t_c - t_a:.3f} ms")
t_i, _ = timed(_core.PairResidenceEngine(N, N, CUTOFF, LAGS, L, same=True, continuous=False, timing=True),
               f"(c') the same without continuous")
print(f"; walk kernel (c') - (a) = {t_i - t_a:.3f} ms")
d.free()
