"""HydrogenBonds timing on one GPU: HB_MOLECULES three-site waters (default 4 096: 8 192 hydrogens against 4 096
acceptor oxygens) x HB_FRAMES frames (default 64) of float32 positions resident in HBM, at the number density of water
(box 49.7 A for the default), distance HB_DISTANCE (default 3.5 A), angle HB_ANGLE (default 150 degrees), every frame
an origin.  Device time of the kernels (``stats()["kernel_ms"]``, HIP events), medians of HB_REPS runs after a warm-up,
all in one process on the same frames:

(a) the hydrogen-bond engine with lag 0 only and 60 + 60 bins: prepare + contact kernel + geometry kernel (+ a walk
    over lag distance 0, which tests no membership); the contract's pair evaluations (``stats()["evaluations"]``) per
    second;
(b) the yardstick: the pair residence engine (``prs_contact_kernel``) with lag 0 only and ``continuous`` off on the same
    n_h x n_a (the hydrogens against the oxygens), box and cutoff: the same 14-operation pair step without the angle,
    without the indexed staging and without the registers for H;
(c) the hydrogen-bond engine with lags 0 ... HB_LAGS - 1 (default 64): the walk kernel's time is (c) - (a).

The engine's results for the first frames of the first molecules are compared with a NumPy restatement before anything
is printed."""
import os
import sys

sys.path.insert(0, ".")
import numpy as np

from mdhelper_amd import _core

N_MOL = int(os.environ.get("HB_MOLECULES", 4096))
F = int(os.environ.get("HB_FRAMES", 64))
N_LAGS = int(os.environ.get("HB_LAGS", 64))
DISTANCE = float(os.environ.get("HB_DISTANCE", 3.5))
ANGLE = float(os.environ.get("HB_ANGLE", 150.0))
REPS = int(os.environ.get("HB_REPS", 5))
L = np.full(3, round((N_MOL / 0.0334) ** (1 / 3), 1))
LAGS = np.arange(min(N_LAGS, F))
COS_MAX = float(np.cos(np.deg2rad(ANGLE)))


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
    o = 3 * np.arange(n_mol, dtype=np.int32)
    return np.stack((o + 1, o + 2), axis=1).ravel(), np.repeat(o, 2), o


def min_image(d):
    return d - L * np.rint(d * (1.0 / L))


def r2_of(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


host = water(7, F, N_MOL, L)
d = _core.DeviceArray.from_host(host)
N = 3 * N_MOL
H_ROW, D_ROW, A_ROW = tables(N_MOL)
EDGES = np.linspace(0.0, DISTANCE, 61)
COS_T = np.cos(np.deg2rad(np.linspace(ANGLE, 180.0, 61)))

# the first frames of the first molecules against the restatement, with the contract's arithmetic
m_check = min(N_MOL, 256)
head = host[:min(F, 4), :3 * m_check]
h_row, d_row, a_row = tables(m_check)
check = _core.HydrogenBondEngine(3 * m_check, h_row, d_row, a_row, DISTANCE, COS_MAX, [0, 1, 3], L)
check.accumulate(head)
got, bonds = check.result(), check.bonds()
check.close()
x = head.astype(np.float64)
pos_h, pos_d, pos_a = x[:, h_row], x[:, d_row], x[:, a_row]
r2 = r2_of(min_image(pos_a[:, None, :, :] - pos_d[:, :, None, :]))
hd = min_image(pos_d - pos_h)[:, :, None, :]
ha = min_image(pos_a[:, None, :, :] - pos_h[:, :, None, :])
with np.errstate(invalid="ignore", divide="ignore"):
    c = ((hd[..., 0] * ha[..., 0] + hd[..., 1] * ha[..., 1]) + hd[..., 2] * ha[..., 2]) / np.sqrt(r2_of(hd) * r2_of(ha))
    b = (r2 <= DISTANCE * DISTANCE) & (a_row[None, :] != d_row[:, None]) & (c <= COS_MAX)
np.testing.assert_array_equal(bonds, b.sum(axis=(1, 2)))
for k, lag in enumerate((0, 1, 3)):
    o = range(len(x) - lag)
    np.testing.assert_array_equal(
        [got["origin_counts"][k], got["intermittent"][k], got["continuous"][k]],
        [sum(b[f].sum() for f in o), sum((b[f] & b[f + lag]).sum() for f in o),
         sum(np.logical_and.reduce(b[f:f + lag + 1]).sum() for f in o)])


def timed(eng, label, index=None):
    """Median device time of REPS passes over the resident frames after a warm-up; prints one line."""
    try:
        eng.accumulate_device(d.ptr, N, min(F, 4), index)      # warm-up: pools, streams, code objects
        eng.synchronize()
        eng.reset()
        ms = []
        for _ in range(REPS):
            eng.accumulate_device(d.ptr, N, F, index)
            stats = eng.stats()
            ms.append(stats["kernel_ms"])
            eng.result()
            eng.reset()
    finally:
        eng.close()
    t = float(np.median(ms))
    print(f"{label}: median {t:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs)", end="", flush=True)
    return t, stats


def hb_engine(lags):
    eng = _core.HydrogenBondEngine(N, H_ROW, D_ROW, A_ROW, DISTANCE, COS_MAX, lags, L, timing=True)
    eng.set_bins(EDGES * EDGES, COS_T)
    return eng


print(f"{F} frames of {N_MOL} waters ({len(H_ROW)} hydrogens x {len(A_ROW)} acceptors), box {L[0]:g} A, "
      f"distance {DISTANCE:g} A, angle {ANGLE:g} degrees")
t_a, stats = timed(hb_engine([0]),
                   "(a) HydrogenBondEngine, lag 0 only [prepare + contact + geometry (+ walk at distance 0)]")
assert stats["evaluations"] == F * (len(H_ROW) * len(A_ROW) - len(H_ROW))
print(f", {stats['evaluations']} pair evaluations, {stats['evaluations'] / t_a / 1e9:.3f} T pair evaluations/s, "
      f"largest row {stats['max_row']}")
t_b, pstats = timed(_core.PairResidenceEngine(len(H_ROW), len(A_ROW), DISTANCE, [0], L, max_neighbors=64,
                                              continuous=False, timing=True),
                    "(b) PairResidenceEngine, hydrogens x oxygens, lag 0 only, continuous off "
                    "[prepare + prs_contact_kernel (+ walk at distance 0)]", np.concatenate((H_ROW, A_ROW)))
assert pstats["evaluations"] == F * len(H_ROW) * len(A_ROW)
print(f", {pstats['evaluations'] / t_b / 1e9:.3f} T pair evaluations/s, largest row {pstats['max_row']}; "
      f"(a) / (b) = {t_a / t_b:.3f}")
t_c, _ = timed(hb_engine(LAGS), f"(c) HydrogenBondEngine, lags 0 ... {int(LAGS[-1])}")
print(f"; walk kernel (c) - (a) = {t_c - t_a:.3f} ms")
d.free()
