"""BondOrientationalOrder timing on one GPU: BOO_PARTICLES particles (default 10 000), the centres and their own
neighbours, x BOO_FRAMES frames (default 2 000) of float32 positions resident in HBM, cutoff BOO_CUTOFF (default
4.0 A: about 12 neighbours) in a 60 A box, 100 bins on (0, 1), max_neighbors 64.  Device time of the kernels
(``stats()["kernel_ms"]``, HIP events), medians of BOO_REPS runs after a warm-up, all in one process on the same
frames:

(a) the bond-order engine, degrees (4, 6), averaged: gather + ``boo_contact_kernel`` + ``boo_rows_kernel`` + per degree
    ``boo_qlm_kernel`` and ``boo_average_kernel`` + ``boo_bin_kernel`` + ``boo_sum_kernel``; frames, the contract's pair
    evaluations and bonds (``stats()``) per second;
(a') the engine with degree (6,), not averaged: one ``boo_qlm_kernel`` per slab and no ``boo_average_kernel``;
(b) the yardstick for phase 1: the pair residence engine on the same particles (``same``), ``lags=[0]``, ``continuous``
    off, on the same frames and cutoff: gather + ``prs_contact_kernel`` (+ a walk over lag distance 0, which tests no
    membership).  That is the same phase 1 without the phases behind it: (a) - (b) is what sorting, harmonics,
    averaging, binning and sums cost, and the split of (a) is printed from it.

The engine's values, sums and counts for the first BOO_CHECK frames (default 2) are compared bit for bit with the
restatement of the contract (``tests/bond_order_cases.py``; a periodic k-d tree names the candidate pairs, the
contract's float64 arithmetic decides among them) before anything is printed."""
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
from scipy.spatial import cKDTree

import bond_order_cases as cases
from mdhelper_amd import _core

N = int(os.environ.get("BOO_PARTICLES", 10000))
F = int(os.environ.get("BOO_FRAMES", 2000))
CUTOFF = float(os.environ.get("BOO_CUTOFF", 4.0))
REPS = int(os.environ.get("BOO_REPS", 5))
CHECK = min(F, int(os.environ.get("BOO_CHECK", 2)))
L = np.array([60.0, 60.0, 60.0])
EDGES = np.linspace(0.0, 1.0, 101)
DEGREES = (4, 6)
CAP = 64

d = _core.synth_random_walk(F, N, L, 0.3, 7)            # wrapped random walk


def restate(x):
    """values [D, 2, N] of one float64 frame: q_l and qbar_l of every particle among all the others."""
    tree = cKDTree(np.mod(x, L), boxsize=L)
    rows = []
    for i, near in enumerate(tree.query_ball_point(np.mod(x, L), 1.01 * CUTOFF)):
        j = np.array(sorted(k for k in near if k != i), dtype=np.int64)
        dx = x[j] - x[i]
        w = dx - L * np.rint(dx * (1.0 / L))
        r2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        keep = r2 <= CUTOFF * CUTOFF
        rows.append((j[keep], w[keep], r2[keep]))
    m = np.array([len(j) for j, _, _ in rows])
    out = np.full((len(DEGREES), 2, N), np.nan)
    for k, l in enumerate(DEGREES):
        q_re, q_im = np.full((l + 1, N), np.nan), np.full((l + 1, N), np.nan)
        for s in range(int(m.max())):                   # slot by slot: ascending j
            i = np.flatnonzero(m > s)
            w = np.array([rows[c][1][s] for c in i])
            r = np.sqrt(np.array([rows[c][2][s] for c in i]))
            re, im = cases.bond_terms(w[:, 0] / r, w[:, 1] / r, w[:, 2] / r, l)
            if s == 0:
                q_re[:, i], q_im[:, i] = 0.0, 0.0
            q_re[:, i] = q_re[:, i] + re
            q_im[:, i] = q_im[:, i] + im
        have = m > 0
        q_re[:, have] = q_re[:, have] / m[have].astype(np.float64)
        q_im[:, have] = q_im[:, have] / m[have].astype(np.float64)
        out[k, 0] = cases.invariant(q_re, q_im, l)
        a_re, a_im = q_re.copy(), q_im.copy()
        for s in range(int(m.max())):
            i = np.flatnonzero(m > s)
            j = np.array([rows[c][0][s] for c in i])
            a_re[:, i] = a_re[:, i] + q_re[:, j]
            a_im[:, i] = a_im[:, i] + q_im[:, j]
        out[k, 1] = cases.invariant(a_re / (m + 1), a_im / (m + 1), l)
    return out


head = d.to_host(0, CHECK).astype(np.float64)
check = _core.BondOrderEngine(N, None, CUTOFF, DEGREES, EDGES, L, same=True, averaged=True, max_neighbors=CAP,
                              keep_values=True)
check.accumulate_device(d.ptr, N, CHECK)
got, rows, values = check.result(), check.frames(), check.values()
check.close()
want = np.stack([restate(head[f]) for f in range(CHECK)])
np.testing.assert_array_equal(values, want)
for f in range(CHECK):
    for k in range(len(DEGREES)):
        for a in range(2):
            assert rows["sums"][f, k, a] == cases.tile_sum(want[f, k, a])
kept = want[~np.isnan(want)].reshape(-1)
assert got["counts"].sum() + got["outside"].sum() == len(kept)
q4 = want[:, 0, 0][~np.isnan(want[:, 0, 0])]
np.testing.assert_array_equal(got["counts"][0, 0], np.histogram(q4, bins=EDGES)[0])


def timed(eng, label):
    """Median device time of REPS passes over the resident frames after a warm-up; prints one line."""
    try:
        eng.accumulate_device(d.ptr, N, min(F, 4))      # warm-up: pools, streams, code objects
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


print(f"{F} frames of {N} particles, their own neighbours, box {L[0]:g} A, cutoff {CUTOFF:g} A, 100 bins, "
      f"max_neighbors {CAP}; frames 0 ... {CHECK - 1} equal the restatement bit for bit")
t_a, stats = timed(_core.BondOrderEngine(N, None, CUTOFF, DEGREES, EDGES, L, same=True, averaged=True,
                                         max_neighbors=CAP, timing=True),
                   "(a) BondOrderEngine, degrees (4, 6), averaged "
                   "[gather + contact + rows + 2 x (qlm + average) + bin + sum]")
assert stats["evaluations"] == F * N * (N - 1)
print(f", {F / t_a * 1e3:.0f} frames/s, {stats['evaluations'] / t_a / 1e9:.3f} T pair evaluations/s, "
      f"{stats['bonds']} bonds ({stats['bonds'] / (F * N):.2f} per particle), largest row {stats['max_row']}")
t_s, sstats = timed(_core.BondOrderEngine(N, None, CUTOFF, (6,), EDGES, L, same=True, averaged=False,
                                          max_neighbors=CAP, timing=True),
                    "(a') BondOrderEngine, degree (6,), not averaged [gather + contact + rows + qlm + bin + sum]")
print(f", {F / t_s * 1e3:.0f} frames/s, {sstats['bonds']} bonds")
t_b, pstats = timed(_core.PairResidenceEngine(N, N, CUTOFF, [0], L, same=True, continuous=False, max_neighbors=CAP,
                                              timing=True),
                    "(b) PairResidenceEngine, same, lag 0 only, continuous off "
                    "[gather + prs_contact_kernel (+ walk at lag 0)]")
assert pstats["evaluations"] == stats["evaluations"]
print(f", {pstats['evaluations'] / t_b / 1e9:.3f} T pair evaluations/s, largest row {pstats['max_row']}")
rest = max(t_a - t_b, 0.0)
print(f"(a) / (b) = {t_a / t_b:.3f}, (a') / (b) = {t_s / t_b:.3f}; of (a), phase 1 (lists) takes about "
      f"{min(t_b / t_a, 1.0) * 100:.0f} %, the phases behind it (rows, harmonics, averages, bins, sums) about "
      f"{max(1.0 - t_b / t_a, 0.0) * 100:.0f} % ({rest:.3f} ms, "
      f"{stats['bonds'] / max(rest, 1e-9) / 1e6:.3f} G bonds/s)")
d.free()
