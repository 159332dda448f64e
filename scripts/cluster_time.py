"""Clusters timing on one GPU: CLU_POINTS points (default 10 000: two species of 5 000) x CLU_FRAMES frames (default
2 000) of float32 positions resident in HBM, unlike-only cutoff CLU_CUTOFF (default 3.5 A) in a 60 A box.  Device time
of the kernels (``stats()["kernel_ms"]``, HIP events), medians of CLU_REPS runs after a warm-up, all in one process on
the same frames:

(a) the cluster engine with the unlike-only table [[0, c], [c, 0]]: prepare + contact kernel + labelling sweeps +
    tallies; its ``sweeps`` and the contract's pair evaluations (``stats()["evaluations"]``, unordered pairs) per
    second;
(a') the cluster engine with one species and the one cutoff c: the bonds of (b)'s contacts, no table lookup;
(b) the yardstick for phase 1: the pair residence engine, one set, ``lags=[0]`` on the same frames and cutoff: prepare
    + ``prs_contact_kernel`` (+ a walk over lag distance 0, which tests no membership).  Both contact kernels evaluate
    the ordered pairs, n (n - 1) per frame;
(c) the host: the wall time of ``scipy.sparse.csgraph.connected_components`` over the restatement's bond matrices of
    CLU_CHECK of the frames (default 20), scaled to all frames; building the matrices is not timed.

How the device time divides among the three phases is read from a kernel trace of this script (the per-kernel totals),
not from the script itself.  The engine's results for the CLU_CHECK frames are compared with the restatement before
anything is printed."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from mdhelper_amd import _core

N = int(os.environ.get("CLU_POINTS", 10000))
F = int(os.environ.get("CLU_FRAMES", 2000))
CUTOFF = float(os.environ.get("CLU_CUTOFF", 3.5))
REPS = int(os.environ.get("CLU_REPS", 5))
CHECK = min(F, int(os.environ.get("CLU_CHECK", 20)))
L = np.array([60.0, 60.0, 60.0])
SPECIES = (np.arange(N) >= N // 2).astype(np.int32)
UNLIKE = np.array([[0.0, CUTOFF], [CUTOFF, 0.0]])

d = _core.synth_random_walk(F, N, L, 0.3, 7)             # wrapped random walk


def bond_matrix(x, table):
    """The contract's bonds of one frame as a sparse matrix.  A periodic k-d tree names the pairs within 1.01 of the
    largest cutoff (no pair outside can be a bond); the contract's float64 arithmetic decides among them."""
    i, j = cKDTree(np.mod(x, L), boxsize=L).query_pairs(1.01 * table.max(), output_type="ndarray").T
    dx = x[j] - x[i]
    w = dx - L * np.rint(dx * (1.0 / L))
    r2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    lim = table[SPECIES[i], SPECIES[j]]
    keep = r2 <= np.where(lim > 0.0, lim * lim, -1.0)
    i, j = np.concatenate((i[keep], j[keep])), np.concatenate((j[keep], i[keep]))
    return csr_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(N, N))


# the first frames against the restatement, and the host's time for the labelling alone
head = d.to_host(0, CHECK).astype(np.float64)
check = _core.ClusterEngine(SPECIES, UNLIKE, L, keep_labels=True)
check.accumulate_device(d.ptr, N, CHECK)
got, labels = check.frames(), check.labels()
check.close()
t_host = 0.0
for f in range(CHECK):
    m = bond_matrix(head[f], UNLIKE)
    t0 = time.perf_counter()
    count, comp = connected_components(m, directed=False)
    t_host += time.perf_counter() - t0
    first = np.full(count, N)
    np.minimum.at(first, comp, np.arange(N))
    np.testing.assert_array_equal(labels[f], first[comp])
    assert got["bonds"][f] == m.nnz // 2 and got["n_clusters"][f] == count
    assert got["largest"][f] == np.bincount(comp).max()


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


print(f"{F} frames of {N} points ({N // 2} + {N - N // 2}), box {L[0]:g} A, cutoff {CUTOFF:g} A; frames 0 ... "
      f"{CHECK - 1} equal the restatement: {int(got['n_clusters'].mean())} clusters a frame, the largest of "
      f"{int(got['largest'].max())}, {int(got['bonds'].mean())} bonds a frame")
t_a, stats = timed(_core.ClusterEngine(SPECIES, UNLIKE, L, timing=True),
                   "(a) ClusterEngine, unlike-only table [prepare + contact + sweeps + tallies]")
assert stats["evaluations"] == F * (N * (N - 1) // 2)
print(f", {stats['sweeps']} sweeps, {stats['evaluations']} pair evaluations, "
      f"{stats['evaluations'] / t_a / 1e9:.3f} T pair evaluations/s ({2 * stats['evaluations'] / t_a / 1e9:.3f} T "
      f"ordered), largest row {stats['max_row']}")
t_u, ustats = timed(_core.ClusterEngine(np.zeros(N, dtype=np.int32), CUTOFF, L, timing=True),
                    "(a') ClusterEngine, one species, one cutoff")
print(f", {ustats['sweeps']} sweeps, largest row {ustats['max_row']}")
t_b, pstats = timed(_core.PairResidenceEngine(N, N, CUTOFF, [0], L, same=True, timing=True),
                    "(b) PairResidenceEngine, one set, lag 0 only [prepare + prs_contact_kernel (+ walk at lag 0)]")
assert pstats["evaluations"] == 2 * stats["evaluations"]
print(f", {pstats['evaluations'] / t_b / 1e9:.3f} T ordered pair evaluations/s, largest row {pstats['max_row']}; "
      f"(a) / (b) = {t_a / t_b:.3f}, (a') / (b) = {t_u / t_b:.3f}")
print(f"(c) scipy connected_components over the bond matrices of {CHECK} frames: {t_host * 1e3:.1f} ms wall, "
      f"{t_host / CHECK * F * 1e3:.0f} ms scaled to {F} frames (building the matrices not counted); "
      f"(c) / (a) = {t_host / CHECK * F * 1e3 / t_a:.1f}")
d.free()
