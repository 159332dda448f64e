"""TetrahedralOrder timing on one GPU: TET_PARTICLES centres (default 16 384), their own candidates, x TET_FRAMES frames
(default 16) of float32 positions resident in HBM in an 80 A box.  Device time of the kernels (``stats()["kernel_ms"]``,
HIP events).  A sample is TET_PASSES passes (default 8) over the frames; every line is the median of TET_REPS samples
(default 9) after a warm-up, with the smallest and the largest, and the engines take their samples in turn so that
what else the machine does meets all of them alike.

(a) the tetrahedral engine, n_nearest 4, the default cutoff (half the box: every candidate is in range, so the bound
    of a lane is its fourth r2 from its fifth step on), the plan's chunk;
(b) the same with ``set_chunk(1024)``;
(c) n_nearest 8, the plan's chunk;
(d) n_nearest 4 with the yardstick's cutoff, the plan's chunk: about four candidates in range, hardly an insert;
(y) the bond-order engine on the same frames with a cutoff that gives about 4 neighbours (TET_CUTOFF, default
    3.1 A), degree 1 alone, not averaged: gather + ``boo_contact_kernel``, the same walk and the same evaluations, +
    rows, ``boo_qlm_kernel<1>``, bin and sum over about 4 bonds a centre.  The engine has no switch that stops behind
    its contact kernel, so (y) bounds the contact phase from above and every ratio to (y) is a LOWER bound of the ratio
    to the contact phase; the ratio itself comes from a kernel trace (below);
(z) the pair residence engine at lag 0 with ``continuous`` off and the same cutoff: gather + ``prs_contact_kernel``,
    the yardstick the other pair engines' scripts use.

The yardstick proper, ``boo_contact_kernel`` alone against ``tet_select_kernel<K>`` alone, is read from a kernel
trace in a run of its own: with TET_TRACE=a the script only runs a warm-up and TET_PASSES passes of (a), (c) and (y),
with TET_TRACE=b of (b) and (y), checks and prints nothing else, and is meant to run under
``rocprofv3 --kernel-trace --stats``, whose per-kernel averages are then per launch of F frames.

Before anything is timed the neighbours, q and S_k of frame 0 are compared with a periodic k-d tree and the contract's
arithmetic (``tests/tetrahedral_cases.py``).

Then, on the r2 of frame 0 itself, the share of a wave's steps in which at least one of its 64 lanes inserts — what
the model in csrc/mdx_tetrahedral_device.hpp estimates as min(1, 64 K / t) — counted on the CPU for TET_WAVES waves
(default 4) of 64 consecutive centres, for one chunk and for chunks of 1 024, K = 4 and 8."""
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
from scipy.spatial import cKDTree

import tetrahedral_cases as cases
from mdhelper_amd import _core
from mdhelper_amd.analysis.order import distance_table

N = int(os.environ.get("TET_PARTICLES", 16384))
F = int(os.environ.get("TET_FRAMES", 16))
CUTOFF = float(os.environ.get("TET_CUTOFF", 3.1))
REPS = int(os.environ.get("TET_REPS", 9))
PASSES = int(os.environ.get("TET_PASSES", 8))
WAVES = int(os.environ.get("TET_WAVES", 4))
L = np.array([80.0, 80.0, 80.0])
HALF = float(L.min() / 2)
Q_EDGES, S_EDGES = np.linspace(-0.5, 1.0, 151), np.linspace(0.0, 1.0, 101)

d = _core.synth_random_walk(F, N, L, 0.3, 7)            # wrapped random walk


def tet(k, cutoff, chunk=0, **kw):
    eng = _core.TetrahedralEngine(N, None, cutoff, Q_EDGES, S_EDGES, distance_table(np.linspace(0.0, cutoff, 201)), L,
                                  n_nearest=k, same=True, **kw)
    eng.set_chunk(chunk)
    return eng


TRACE = os.environ.get("TET_TRACE", "")
if TRACE:
    boo = _core.BondOrderEngine(N, None, CUTOFF, (1,), np.linspace(0.0, 1.0, 101), L, same=True, averaged=False,
                                max_neighbors=64)
    traced = {"a": [tet(4, HALF), tet(8, HALF), boo], "b": [tet(4, HALF, 1024), boo]}[TRACE]
    for eng in traced:
        for _ in range(1 + PASSES):
            eng.accumulate_device(d.ptr, N, F)
        eng.synchronize()
        eng.close()
    d.free()
    print(f"traced {1 + PASSES} launches of {F} frames per engine, set {TRACE}")
    sys.exit(0)

# ---- frame 0 against a k-d tree and the contract's arithmetic
x = d.to_host(0, 1)[0].astype(np.float64)
check = tet(4, HALF, keep_values=True)
check.accumulate_device(d.ptr, N, 1)
kept = check.values()
check.close()
_, near = cKDTree(np.mod(x, L), boxsize=L).query(np.mod(x, L), k=6)
w = x[near[:, 1:]] - x[:, None, :]
w = w - L * np.rint(w * (1.0 / L))
r2 = cases.r2_of(w)
order = np.argsort(r2, axis=1, kind="stable")[:, :4]
assert (np.diff(np.sort(r2, axis=1), axis=1) > 0).all(), "a tie among the nearest five: compare by hand"
np.testing.assert_array_equal(kept["neighbors"][0].T, np.take_along_axis(near[:, 1:], order, 1))
q, sk = cases.q_sk(np.take_along_axis(w, order[..., None], 1), np.take_along_axis(r2, order, 1))
np.testing.assert_array_equal(kept["values"][0], np.stack((q, sk)))

# ---- timing
engines = {
    "(a) TetrahedralEngine, k = 4, cutoff L / 2, the plan's chunk": tet(4, HALF, timing=True),
    "(b) TetrahedralEngine, k = 4, cutoff L / 2, set_chunk(1024)": tet(4, HALF, 1024, timing=True),
    "(c) TetrahedralEngine, k = 8, cutoff L / 2, the plan's chunk": tet(8, HALF, timing=True),
    f"(d) TetrahedralEngine, k = 4, cutoff {CUTOFF:g}, the plan's chunk": tet(4, CUTOFF, timing=True),
    f"(y) BondOrderEngine, degree 1, not averaged, cutoff {CUTOFF:g} [gather + contact + rows + qlm<1> + bin + sum]":
        _core.BondOrderEngine(N, None, CUTOFF, (1,), np.linspace(0.0, 1.0, 101), L, same=True, averaged=False,
                              max_neighbors=64, timing=True),
    f"(z) PairResidenceEngine, lag 0, continuous off, cutoff {CUTOFF:g} [gather + prs_contact_kernel + walk at lag 0]":
        _core.PairResidenceEngine(N, N, CUTOFF, [0], L, same=True, continuous=False, max_neighbors=64, timing=True),
}
samples = {label: [] for label in engines}
last = {}
try:
    for eng in engines.values():                        # warm-up: pools, streams, code objects
        eng.accumulate_device(d.ptr, N, F)
        eng.synchronize()
        eng.reset()
    for _ in range(REPS):
        for label, eng in engines.items():
            for _ in range(PASSES):
                eng.accumulate_device(d.ptr, N, F)
            last[label] = eng.stats()
            samples[label].append(last[label]["kernel_ms"] / PASSES)
            eng.reset()
finally:
    for eng in engines.values():
        eng.close()

evaluations = F * N * (N - 1)
print(f"{F} frames of {N} particles, their own candidates, box {L[0]:g} A; a sample is {PASSES} passes, {REPS} samples "
      f"per line, taken in turn; frame 0 equals the k-d tree and the contract bit for bit")
medians = {}
for label, ms in samples.items():
    assert last[label]["evaluations"] == PASSES * evaluations
    medians[label[:3]] = t = float(np.median(ms))
    extra = f", {last[label]['chunks']} chunk(s)" if "chunks" in last[label] else ""
    print(f"{label}: median {t:.3f} ms a pass (min {min(ms):.3f}, max {max(ms):.3f}), "
          f"{evaluations / t / 1e9:.3f} T pair evaluations/s{extra}")
for key in ("(a)", "(b)", "(c)", "(d)"):
    print(f"{key} / (y) = {medians[key] / medians['(y)']:.3f} (a lower bound of the ratio to the contact phase: (y) "
          f"holds more than that phase), {key} / (z) = {medians[key] / medians['(z)']:.3f}")
print(f"(b) / (a) = {medians['(b)'] / medians['(a)']:.3f}, (c) / (a) = {medians['(c)'] / medians['(a)']:.3f}, "
      f"(a) / (d) = {medians['(a)'] / medians['(d)']:.3f}")
d.free()

# ---- the share of a wave's steps with an insert, counted on frame 0
xf = x.astype(np.float32).astype(np.float64)


def insert_share(first, k, chunk):
    """Of the steps of the wave of centres first ... first + 63 over all candidates in chunks of `chunk`: the share in
    which a lane's r2 is below its bound (the list of a chunk starts empty)."""
    i = np.arange(first, first + 64)
    dx = xf[None, :, :] - xf[i, None, :]
    wv = dx - L * np.rint(dx * (1.0 / L))
    r2v = cases.r2_of(wv)
    r2v[np.arange(64), i] = np.inf                      # j == i never counts
    r2v[r2v > HALF * HALF] = np.inf
    steps = hits = 0
    for j0 in range(0, N, chunk):
        best = np.full((64, k), np.inf)
        for j in range(j0, min(j0 + chunk, N)):
            ins = r2v[:, j] < best[:, -1]
            steps += 1
            if ins.any():
                hits += 1
                best[ins, -1] = r2v[ins, j]
                best.sort(axis=1)
    return hits / steps


firsts = [w0 * 64 * max(1, N // 64 // WAVES) for w0 in range(WAVES)]
for k in (4, 8):
    for chunk in (N, 1024):
        share = float(np.mean([insert_share(first, k, chunk) for first in firsts]))
        t = np.arange(1, chunk + 1)
        model = float(np.minimum(1.0, 64.0 * k / t).mean())
        print(f"steps of a wave with an insert, K = {k}, chunks of {chunk}: {share:.3f} counted on {WAVES} waves of "
              f"frame 0, {model:.3f} by min(1, 64 K / t)")
