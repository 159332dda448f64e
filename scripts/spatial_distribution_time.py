"""SpatialDistributionFunction timing on one GPU: SDF_MOLECULES three-site waters (default 16 384: the oxygens as
reference molecules, O H H, against all 49 152 atoms as partners, oxygens and hydrogens as two groups, every atom owned
by its molecule) x SDF_FRAMES frames (default 16) of float32 positions resident in HBM, at the number density of water
(box 78.9 A for the default), SDF_BINS bins per axis (default 60).  Device time of the kernels
(``stats()["kernel_ms"]``, HIP events), medians of SDF_REPS runs after a warm-up, all in one process on the same
frames.  One line per range R (the local box is [-R, R]^3, the cutoff its circumscribed sphere), R = 6 A and R = 10 A:

(a) the engine in the axis frame and (b) in the bisector frame: gather + sdf_pair_kernel; the contract's pair
    evaluations (``stats()["evaluations"]``) per second, the counted pairs (hits) per second and the hit fraction;
(c) the yardstick: the pair residence engine (``prs_contact_kernel``) with lag 0 only and ``continuous`` off on the same
    two sets (the oxygens against all atoms), box and cutoff (the SDF's sphere): the same 14-operation pair step
    without the frames, the rotation and the histogram.  Its rows overflow at these cutoffs, which it counts without
    storing; only its time is read.

The engine's results for the first frames of the first molecules are compared with a NumPy restatement before anything
is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

N_MOL = int(os.environ.get("SDF_MOLECULES", 16384))
F = int(os.environ.get("SDF_FRAMES", 16))
BINS = int(os.environ.get("SDF_BINS", 60))
REPS = int(os.environ.get("SDF_REPS", 5))
RANGES = [float(r) for r in os.environ.get("SDF_RANGES", "6,10").split(",")]
L = np.full(3, round((N_MOL / 0.0334) ** (1 / 3), 1))


def water(seed, n_frames, n_mol, dims, step=0.15, turn=0.15):
    """float32 [n_frames, 3 * n_mol, 3], rows O, H, H per molecule: walking oxygens, O-H unit vectors that turn, every
    atom wrapped into the box by itself."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.0, 1.0, (1, n_mol, 3)) * dims + np.cumsum(rng.normal(0.0, step, (n_frames, n_mol, 3)), axis=0)
    u = np.cumsum(np.concatenate((rng.normal(0.0, 1.0, (1, n_mol, 2, 3)),
                                  rng.normal(0.0, turn, (n_frames - 1, n_mol, 2, 3)))), axis=0)
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    true = np.concatenate((o[:, :, None], o[:, :, None] + u), axis=2).reshape(n_frames, 3 * n_mol, 3)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0
    return wrapped


def tables(n_mol):
    """o_row, a_row, b_row, group_start, p_row, owner: every oxygen, then every hydrogen, owned by their molecules."""
    o = 3 * np.arange(n_mol, dtype=np.int32)
    p_row = np.concatenate((o, np.stack((o + 1, o + 2), axis=1).ravel()))
    return o, o + 1, o + 2, [0, n_mol, 3 * n_mol], p_row, p_row // 3


def min_image(d):
    return d - L * np.rint(d * (1.0 / L))


def r2_of(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def unit(v):
    return v / np.sqrt(r2_of(v))[..., None]


def cross(p, q):
    return np.stack((p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]), axis=-1)


def dot(w, e):
    return (w[..., 0] * e[..., 0] + w[..., 1] * e[..., 1]) + w[..., 2] * e[..., 2]


def sphere(R):
    """The cutoff SpatialDistributionFunction takes for range=R."""
    return float(np.sqrt(3.0 * R * R) * (1.0 + 2.0 ** -40))


host = water(7, F, N_MOL, L)
d = _core.DeviceArray.from_host(host)
N = 3 * N_MOL
TABLES = tables(N_MOL)

# the first frames of the first molecules against the restatement, with the contract's arithmetic, in both frames
m_check = min(N_MOL, 256)
head = host[:min(F, 2), :3 * m_check]
o_row, a_row, b_row, start, p_row, owner = tables(m_check)
edges = np.linspace(-RANGES[0], RANGES[0], 13)
x = head.astype(np.float64)
for mode in (0, 1):
    check = _core.SpatialDistributionEngine(3 * m_check, o_row, a_row, b_row, start, p_row, owner, mode,
                                            sphere(RANGES[0]), L)
    check.set_bins(edges, edges, edges)
    check.accumulate(head)
    got, inside = check.result(), check.inside()
    check.close()
    O = x[:, o_row]
    va, vb = min_image(x[:, a_row] - O), min_image(x[:, b_row] - O)
    p = va if mode == 0 else unit(va) + unit(vb)
    e1, e3 = unit(p), unit(cross(p, vb))
    e2 = cross(e3, e1)
    w = min_image(x[:, None, p_row] - O[:, :, None])
    near = (r2_of(w) <= sphere(RANGES[0]) ** 2) & (owner[None, :] != np.arange(m_check)[:, None])
    local = np.stack([dot(w, e[:, :, None]) for e in (e1, e2, e3)], axis=-1)
    kept = near & np.all((local >= edges[0]) & (local <= edges[-1]), axis=-1)
    want = np.zeros((2, 12, 12, 12), dtype=np.int64)
    f, i, j = np.nonzero(kept)
    cell = (local[f, i, j][:, :, None] >= edges[None, None, 1:-1]).sum(axis=2)
    np.add.at(want, ((j >= m_check).astype(int), cell[:, 0], cell[:, 1], cell[:, 2]), 1)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(inside, kept.sum(axis=(1, 2)))
    assert want.sum() > 0


def timed(eng, index=None, collect=None):
    """Median device time of REPS passes over the resident frames after a warm-up."""
    try:
        eng.accumulate_device(d.ptr, N, min(F, 2), index)      # warm-up: pools, streams, code objects
        eng.synchronize() if collect else eng.stats()
        eng.reset()
        ms, extra = [], None
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F, index)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            if collect:
                extra = collect(eng)
            eng.reset()
    finally:
        eng.close()
    return float(np.median(ms)), min(ms), max(ms), stats, extra


print(f"{F} frames of {N_MOL} waters ({N_MOL} molecules x {N} partners in two groups), box {L[0]:g} A, "
      f"{BINS}^3 bins, medians of {REPS} runs")
for R in RANGES:
    cutoff, e = sphere(R), np.linspace(-R, R, BINS + 1)
    line = [f"R = {R:g} A (cutoff {cutoff:.3f} A):"]
    times = []
    for label, mode in (("(a) axis", 0), ("(b) bisector", 1)):
        eng = _core.SpatialDistributionEngine(N, *TABLES, mode, cutoff, L, timing=True)
        eng.set_bins(e, e, e)
        t, lo, hi, stats, hits = timed(eng, collect=lambda g: int(g.inside().sum()))
        assert stats["evaluations"] == F * (N_MOL * N - N) and stats["degenerate"] == 0
        times.append(t)
        line.append(f"{label} {t:.3f} ms (min {lo:.3f}, max {hi:.3f}), {stats['evaluations'] / t / 1e9:.3f} T "
                    f"evaluations/s, {hits / t / 1e6:.3f} G hits/s, hit fraction {hits / stats['evaluations']:.5f};")
    prs = _core.PairResidenceEngine(N_MOL, N, cutoff, [0], L, max_neighbors=64, continuous=False, timing=True)
    t_c, lo, hi, pstats, _ = timed(prs, np.concatenate((TABLES[0], TABLES[4])))
    assert pstats["evaluations"] == F * N_MOL * N
    line.append(f"(c) PairResidenceEngine, lag 0 only, continuous off {t_c:.3f} ms (min {lo:.3f}, max {hi:.3f}), "
                f"{pstats['evaluations'] / t_c / 1e9:.3f} T evaluations/s; (a) / (c) = {times[0] / t_c:.3f}, "
                f"(b) / (c) = {times[1] / t_c:.3f}")
    print(" ".join(line), flush=True)
d.free()
