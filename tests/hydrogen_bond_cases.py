"""
The float64 NumPy restatement of the hydrogen-bond contract (csrc/mdx_hbond_device.hpp) and the water generator of its
tests: shared by ``test_hydrogen_bonds_host.py`` and ``test_gpu_hydrogen_bonds.py``.

Per frame, hydrogen i and acceptor j, with H, D, A the float32 positions of h_row[i], d_row[i], a_row[j] widened:

    w(x) = x - L * rint(x * (1.0 / L))   (+0.0 for a dropped component)
    w_DA = w(A - D);  r2_DA = (w_DAx^2 + w_DAy^2) + w_DAz^2;  w_HD = w(D - H);  w_HA = w(A - H)
    c = ((w_HDx*w_HAx + w_HDy*w_HAy) + w_HDz*w_HAz) / sqrt(r2_HD * r2_HA)
    inside = r2_DA <= distance * distance and a_row[j] != d_row[i];  bond = inside and c <= cos_max

one float64 operation at a time, as the device does (its unit is built with contraction off; rint rounds ties to even
on both sides; sqrt and / are correctly rounded on both sides), so every comparison against it is
``assert_array_equal``.
"""

import numpy as np

BOX = np.array([18.0, 20.0, 22.5])
LAGS = [0, 1, 2, 5, 8, 11, 13]          # lag 13 never has an origin in 12 frames
F = 12
DISTANCE = 3.5
KEYS = ("intermittent", "continuous", "origin_counts")
COUNTS = KEYS + ("bonds", "donated", "distance_counts", "cosine_counts")


def cos_of(angle):
    """``cos_max`` of an angle in degrees, as the class forms it."""
    return float(np.cos(np.deg2rad(angle)))


def water(seed, F, n_mol, dims, step=0.15, turn=0.15):
    """float32 ``[F, 3 * n_mol, 3]``: rows O, H, H per molecule.  The oxygens start uniform in the box and walk; the two
    O-H unit vectors of a molecule start at random and turn by a walk of their own.  Every atom is wrapped into [0, L)
    by itself, so a molecule may straddle a face."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    O = rng.uniform(0.0, 1.0, (1, n_mol, 3)) * dims + np.cumsum(rng.normal(0.0, step, (F, n_mol, 3)), axis=0)
    u = np.cumsum(np.concatenate((rng.normal(0.0, 1.0, (1, n_mol, 2, 3)),
                                  rng.normal(0.0, turn, (F - 1, n_mol, 2, 3)))), axis=0)
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    H = O[:, :, None] + u
    true = np.concatenate((O[:, :, None], H), axis=2).reshape(F, 3 * n_mol, 3)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


def water_tables(n_mol):
    """``(h_row, d_row, a_row)`` of the water above: every H with its O, every O an acceptor."""
    o = 3 * np.arange(n_mol, dtype=np.int32)
    h_row = np.stack((o + 1, o + 2), axis=1).ravel()
    d_row = np.repeat(o, 2)
    return h_row, d_row, o


def _min_image(d, dims, inv, zero_dims):
    s = d * inv
    w = d - dims * np.rint(s)
    for c in range(3):
        if zero_dims >> c & 1:
            w[..., c] = 0.0
    return w


def _r2(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def frame_geometry(frame, h_row, d_row, a_row, dims, zero_dims=0):
    """``(r2_DA, c)``, float64 ``[n_h, n_a]`` each, of one float32 frame ``[n_rows, 3]``."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    x = np.asarray(frame).astype(np.float64)
    H, D, A = x[h_row], x[d_row], x[a_row]
    r2 = _r2(_min_image(A[None, :, :] - D[:, None, :], dims, inv, zero_dims))
    hd = _min_image(D - H, dims, inv, zero_dims)[:, None, :]
    ha = _min_image(A[None, :, :] - H[:, None, :], dims, inv, zero_dims)
    dot = (hd[..., 0] * ha[..., 0] + hd[..., 1] * ha[..., 1]) + hd[..., 2] * ha[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = dot / np.sqrt(_r2(hd) * _r2(ha))
    return r2, c


def bin_up(values, thresholds):
    """``#{m in 1 ... n - 1 : value >= t[m]}`` per value: the rule of ``distance_counts``."""
    inner = np.asarray(thresholds, dtype=np.float64)[1:-1]
    return (np.asarray(values)[:, None] >= inner[None, :]).sum(axis=1)


def bin_down(values, thresholds):
    """``#{m in 1 ... n - 1 : value <= t[m]}`` per value: the rule of ``cosine_counts``."""
    inner = np.asarray(thresholds, dtype=np.float64)[1:-1]
    return (np.asarray(values)[:, None] <= inner[None, :]).sum(axis=1)


def restate(pos, h_row, d_row, a_row, distance, cos_max, lags, dims, *, origin_step=1, zero_dims=0, max_neighbors=8,
            r2_thresholds=None, cos_thresholds=None):
    """Every result of the contract for float32 ``pos [F, n_rows, 3]``, and with them ``r2`` and ``c`` of the bonds
    (in frame, hydrogen, acceptor order), ``bond`` (bool ``[F, n_h, n_a]``), ``rows`` (the bonds of every (frame,
    hydrogen)), ``evaluations``, ``frames``, ``max_row`` and ``degenerate``.  ``donated`` needs
    ``max_row <= max_neighbors``: the caller asserts it."""
    h_row, d_row, a_row = (np.asarray(t, dtype=np.int64) for t in (h_row, d_row, a_row))
    n_frames = len(pos)
    rc2 = np.float64(distance) * np.float64(distance)
    own = a_row[None, :] == d_row[:, None]
    bond = np.zeros((n_frames, len(h_row), len(a_row)), dtype=bool)
    r2_b, c_b, degenerate = [], [], 0
    for f in range(n_frames):
        r2, c = frame_geometry(pos[f], h_row, d_row, a_row, dims, zero_dims)
        inside = (r2 <= rc2) & ~own
        degenerate += int((inside & np.isnan(c)).sum())
        with np.errstate(invalid="ignore"):
            bond[f] = inside & (c <= np.float64(cos_max))
        r2_b.append(r2[bond[f]])
        c_b.append(c[bond[f]])
    out = {key: np.zeros(len(lags), dtype=np.int64) for key in KEYS}
    for k, lag in enumerate(lags):
        for f0 in range(0, n_frames - lag, origin_step):
            out["origin_counts"][k] += bond[f0].sum()
            out["intermittent"][k] += (bond[f0] & bond[f0 + lag]).sum()
            out["continuous"][k] += np.logical_and.reduce(bond[f0:f0 + lag + 1], axis=0).sum()
    rows = bond.sum(axis=2)
    out["bonds"] = bond.sum(axis=(1, 2)).astype(np.int64)
    out["bond"] = bond
    out["rows"] = rows
    out["max_row"] = int(rows.max()) if rows.size else 0
    out["donated"] = np.bincount(np.minimum(rows.ravel(), max_neighbors), minlength=max_neighbors + 1).astype(np.int64)
    out["r2"] = np.concatenate(r2_b) if r2_b else np.zeros(0)
    out["c"] = np.concatenate(c_b) if c_b else np.zeros(0)
    r2_thresholds = [0.0, 1.0] if r2_thresholds is None else r2_thresholds
    cos_thresholds = [1.0, -1.0] if cos_thresholds is None else cos_thresholds
    out["distance_counts"] = np.bincount(bin_up(out["r2"], r2_thresholds),
                                         minlength=len(r2_thresholds) - 1).astype(np.int64)
    out["cosine_counts"] = np.bincount(bin_down(out["c"], cos_thresholds),
                                       minlength=len(cos_thresholds) - 1).astype(np.int64)
    out["evaluations"] = n_frames * (len(h_row) * len(a_row) - int(own.sum()))
    out["frames"] = n_frames
    out["degenerate"] = degenerate
    return out


def collect(eng):
    """What ``restate`` returns, of an engine."""
    got = eng.result()
    got["bonds"] = eng.bonds()
    got.update(eng.geometry())
    stats = eng.stats()
    for key in ("evaluations", "frames", "max_row", "degenerate"):
        got[key] = stats[key]
    return got


def assert_same(got, want, continuous=True):
    for key in COUNTS:
        expect = want[key] if continuous or key != "continuous" else np.zeros_like(want[key])
        np.testing.assert_array_equal(got[key], expect, err_msg=key)
        assert got[key].dtype == np.int64
    for key in ("evaluations", "frames", "max_row", "degenerate"):
        assert got[key] == want[key], key
    assert got["distance_counts"].sum() == got["cosine_counts"].sum() == got["bonds"].sum()
    assert got["donated"].sum() == want["frames"] * want["rows"].shape[1]
