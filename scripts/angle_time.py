"""AngularDistribution timing on one GPU: ANG_CENTERS centres (default 2 000) and ANG_LIGANDS ligands (default 8 000:
two species of 4 000) x ANG_FRAMES frames (default 2 000) of float32 positions resident in HBM, cutoff ANG_CUTOFF
(default 3.5 A) in a 60 A box, 180 bins of equal width in the angle.  Device time of the kernels
(``stats()["kernel_ms"]``, HIP events), medians of ANG_REPS runs after a warm-up, all in one process on the same
frames:

(a) the angle engine with two ligand species of one cutoff: prepare + ``ang_contact_kernel`` + ``ang_triplet_kernel``;
    frames, the contract's pair evaluations and triplets (``stats()``) per second;
(a') the angle engine with two cutoffs (c, 0.9 c): the bound of a ligand comes from its species;
(b) the yardstick for phase 1: the pair residence engine, the same centres and ligands, ``lags=[0]``, ``continuous``
    off, on the same frames and cutoff: prepare + ``prs_contact_kernel`` (+ a walk over lag distance 0, which tests
    no membership).  That is the same phase 1 without phase 2: (a) - (b) is what the angle phase costs, and the split
    of (a) between the two phases is printed from it.

The engine's results for the first ANG_CHECK frames (default 2) are compared with a NumPy restatement of the contract
before anything is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np
from scipy.spatial import cKDTree

from mdhelper_amd import _core

N0 = int(os.environ.get("ANG_CENTERS", 2000))
NL = int(os.environ.get("ANG_LIGANDS", 8000))
F = int(os.environ.get("ANG_FRAMES", 2000))
CUTOFF = float(os.environ.get("ANG_CUTOFF", 3.5))
REPS = int(os.environ.get("ANG_REPS", 5))
CHECK = min(F, int(os.environ.get("ANG_CHECK", 2)))
L = np.array([60.0, 60.0, 60.0])
SIZES = [NL // 2, NL - NL // 2]
THRESHOLDS = np.cos(np.deg2rad(np.linspace(0.0, 180.0, 181)))

d = _core.synth_random_walk(F, N0 + NL, L, 0.3, 7)      # wrapped random walk


def restate(x, cutoff):
    """counts [3, 180] of one frame.  A periodic k-d tree names the (centre, ligand) pairs within 1.01 of the largest
    cutoff (no pair outside can be a neighbour); the contract's float64 arithmetic decides among them."""
    species = np.repeat([0, 1], SIZES)
    ligands = cKDTree(np.mod(x[N0:], L), boxsize=L)
    counts = np.zeros((3, 180), dtype=np.int64)
    for i, near in enumerate(ligands.query_ball_point(np.mod(x[:N0], L), 1.01 * max(cutoff))):
        j = np.array(sorted(near), dtype=np.int64)
        dx = x[N0 + j] - x[i]
        w = dx - L * np.rint(dx * (1.0 / L))
        r2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        keep = r2 <= (np.asarray(cutoff) ** 2)[species[j]]
        w, r2, g = w[keep], r2[keep], species[j[keep]]
        a, b = np.triu_indices(len(w), 1)
        dot = (w[a, 0] * w[b, 0] + w[a, 1] * w[b, 1]) + w[a, 2] * w[b, 2]
        c = dot / np.sqrt(r2[a] * r2[b])
        # the pairs (0, 0), (0, 1), (1, 1) of two species are p = 0, 1, 2
        np.add.at(counts, (g[a] + g[b], np.searchsorted(-THRESHOLDS[1:-1], -c, side="right")), 1)
    return counts


head = d.to_host(0, CHECK).astype(np.float64)
for cutoff in ([CUTOFF, CUTOFF], [CUTOFF, 0.9 * CUTOFF]):
    check = _core.AngleEngine(N0, SIZES, cutoff, THRESHOLDS, L)
    check.accumulate_device(d.ptr, N0 + NL, CHECK)
    got = check.result()
    check.close()
    assert not got["degenerate"].any()
    np.testing.assert_array_equal(got["counts"], sum(restate(head[f], cutoff) for f in range(CHECK)))


def timed(eng, label):
    """Median device time of REPS passes over the resident frames after a warm-up; prints one line."""
    try:
        eng.accumulate_device(d.ptr, N0 + NL, min(F, 4))        # warm-up: pools, streams, code objects
        eng.synchronize()
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N0 + NL, F)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            eng.result()
            eng.reset()
    finally:
        eng.close()
    t = float(np.median(ms))
    print(f"{label}: median {t:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs)", end="", flush=True)
    return t, stats


print(f"{F} frames of {N0} centres and {NL} ligands ({SIZES[0]} + {SIZES[1]}), box {L[0]:g} A, cutoff {CUTOFF:g} A, "
      f"180 bins; frames 0 ... {CHECK - 1} equal the restatement")
t_a, stats = timed(_core.AngleEngine(N0, SIZES, CUTOFF, THRESHOLDS, L, timing=True),
                   "(a) AngleEngine, two species, one cutoff [prepare + contact + triplet]")
assert stats["evaluations"] == F * N0 * NL
print(f", {F / t_a * 1e3:.0f} frames/s, {stats['evaluations'] / t_a / 1e9:.3f} T pair evaluations/s, "
      f"{stats['triplets']} triplets, {stats['triplets'] / t_a / 1e6:.3f} G triplets/s, largest row "
      f"{stats['max_row']}")
t_u, ustats = timed(_core.AngleEngine(N0, SIZES, [CUTOFF, 0.9 * CUTOFF], THRESHOLDS, L, timing=True),
                    "(a') AngleEngine, two species, two cutoffs")
print(f", {ustats['triplets']} triplets, largest row {ustats['max_row']}")
t_b, pstats = timed(_core.PairResidenceEngine(N0, NL, CUTOFF, [0], L, continuous=False, timing=True),
                    "(b) PairResidenceEngine, lag 0 only, continuous off [prepare + prs_contact_kernel (+ walk at lag 0)]")
assert pstats["evaluations"] == stats["evaluations"]
print(f", {pstats['evaluations'] / t_b / 1e9:.3f} T pair evaluations/s, largest row {pstats['max_row']}")
print(f"(a) / (b) = {t_a / t_b:.3f}, (a') / (b) = {t_u / t_b:.3f}; of (a), phase 1 (lists) takes about "
      f"{min(t_b / t_a, 1.0) * 100:.0f} %, phase 2 (angles) about {max(1.0 - t_b / t_a, 0.0) * 100:.0f} % "
      f"({max(t_a - t_b, 0.0):.3f} ms, {stats['triplets'] / max(t_a - t_b, 1e-9) / 1e6:.3f} G triplets/s)")
d.free()
