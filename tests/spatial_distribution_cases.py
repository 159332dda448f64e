"""
The float64 NumPy restatement of the spatial-distribution contract (csrc/mdx_sdf_device.hpp) and the generators of its
tests: shared by ``test_spatial_distribution_host.py`` and ``test_gpu_spatial_distribution.py``.

Per frame, reference molecule i (origin O, axis atom A, plane atom B) and partner j at P, float32 positions widened:

    w(x) = x - L * rint(x * (1.0 / L))
    a = w(A - O);  b = w(B - O);  p = a  (axis)  or  a / sqrt(r2(a)) + b / sqrt(r2(b))  (bisector)
    e1 = p / sqrt(r2(p));  c = p x b;  e3 = c / sqrt(r2(c));  e2 = e3 x e1
    w_ij = w(P - O);  near = r2(w_ij) <= rc2 and owner[j] != i and the frame of i is finite
    (u, v, t) = ((w_x*e_x + w_y*e_y) + w_z*e_z for e in e1, e2, e3)

one float64 operation at a time, as the device does (its unit is built with contraction off; rint rounds ties to even
on both sides; sqrt and / are correctly rounded on both sides), so every comparison against it is
``assert_array_equal``.
"""

import numpy as np

from hydrogen_bond_cases import BOX, water       # noqa: F401  (re-exported for the tests)

AXIS, BISECTOR = 0, 1
F = 12
N_MOL = 257


def water_system(n_ref=N_MOL, owners=True):
    """``(o_row, a_row, b_row, group_start, p_row, owner)`` of ``water``: the first ``n_ref`` molecules as references
    (O, H, H), every oxygen and then every hydrogen as partners, each owned by its molecule (or by none).  Beyond 257
    references the waters are taken a second time, seen from their first hydrogen (H, O, H): those frames own
    nothing."""
    mol = np.arange(N_MOL, dtype=np.int32)
    o = 3 * mol[:n_ref]
    if n_ref > N_MOL:
        again = 3 * mol[:n_ref - N_MOL]
        a_row, b_row = np.concatenate((o + 1, again)), np.concatenate((o + 2, again + 2))
        o = np.concatenate((o, again + 1))
        start, p_row, owner = water_system(owners=owners)[3:]
        return o, a_row, b_row, start, p_row, owner
    p_row = np.concatenate((3 * mol, np.stack((3 * mol + 1, 3 * mol + 2), axis=1).ravel())).astype(np.int32)
    owner = (p_row // 3).astype(np.int32)
    owner[owner >= n_ref] = -1
    if not owners:
        owner[:] = -1
    return o, o + 1, o + 2, np.array([0, N_MOL, 3 * N_MOL], dtype=np.int32), p_row, owner


_shared = {}


def shared_water():
    """The 12 frames of 257 waters every test shares: computed once, never written to."""
    if "pos" not in _shared:
        pos = water(357, F, N_MOL, BOX)
        pos.setflags(write=False)
        _shared["pos"] = pos
    return _shared["pos"]


def _min_image(d, dims, inv):
    return d - dims * np.rint(d * inv)


def _r2(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def _cross(p, q):
    return np.stack((p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1],
                     p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]), axis=-1)


def _dot(w, e):
    return (w[..., 0] * e[..., 0] + w[..., 1] * e[..., 1]) + w[..., 2] * e[..., 2]


def frames_of(frame, o_row, a_row, b_row, mode, dims):
    """``(e1, e2, e3, degenerate)`` of one float32 frame: float64 ``[n_ref, 3]`` each and bool ``[n_ref]``."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    x = np.asarray(frame).astype(np.float64)
    O = x[o_row]
    a = _min_image(x[a_row] - O, dims, inv)
    b = _min_image(x[b_row] - O, dims, inv)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = a if mode == AXIS else a / np.sqrt(_r2(a))[:, None] + b / np.sqrt(_r2(b))[:, None]
        e1 = p / np.sqrt(_r2(p))[:, None]
        c = _cross(p, b)
        e3 = c / np.sqrt(_r2(c))[:, None]
        e2 = _cross(e3, e1)
    degenerate = ~(np.isfinite(e1).all(axis=1) & np.isfinite(e2).all(axis=1) & np.isfinite(e3).all(axis=1))
    return e1, e2, e3, degenerate


def local_coordinates(frame, o_row, a_row, b_row, p_row, owner, mode, rc2, dims):
    """``(uvt, near)`` of one frame: float64 ``[n_ref, n_p, 3]`` (NaN where not near) and bool ``[n_ref, n_p]``."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    x = np.asarray(frame).astype(np.float64)
    e1, e2, e3, degenerate = frames_of(frame, o_row, a_row, b_row, mode, dims)
    w = _min_image(x[p_row][None, :, :] - x[o_row][:, None, :], dims, inv)
    own = np.asarray(owner)[None, :] == np.arange(len(o_row))[:, None]
    with np.errstate(invalid="ignore"):
        near = (_r2(w) <= np.float64(rc2)) & ~own & ~degenerate[:, None]
    uvt = np.full(w.shape, np.nan)
    i, j = np.nonzero(near)
    wn = w[i, j]
    uvt[i, j] = np.stack((_dot(wn, e1[i]), _dot(wn, e2[i]), _dot(wn, e3[i])), axis=-1)
    return uvt, near


def bin_of(values, edges):
    """``#{m in 1 ... n - 1 : value >= edges[m]}`` per value: only the inner edges are compared."""
    inner = np.asarray(edges, dtype=np.float64)[1:-1]
    return (np.asarray(values)[:, None] >= inner[None, :]).sum(axis=1)


def restate(pos, o_row, a_row, b_row, group_start, p_row, owner, mode, rc2, edges, dims, keep_local=False):
    """Every result of the contract for float32 ``pos [F, n_rows, 3]``: ``counts`` int64 ``[G, nx, ny, nz]``,
    ``inside`` int64 ``[F]``, ``degenerate``, ``evaluations``, ``frames``; with ``keep_local`` also ``local``: per
    group the ``[m, 3]`` local coordinates of its near pairs, in frame order."""
    o_row, a_row, b_row, p_row, owner = (np.asarray(t, dtype=np.int64) for t in (o_row, a_row, b_row, p_row, owner))
    ex, ey, ez = (np.asarray(e, dtype=np.float64) for e in edges)
    G = len(group_start) - 1
    counts = np.zeros((G, len(ex) - 1, len(ey) - 1, len(ez) - 1), dtype=np.int64)
    inside = np.zeros(len(pos), dtype=np.int64)
    group_of = np.searchsorted(np.asarray(group_start)[1:], np.arange(len(p_row)), side="right")
    degenerate = 0
    local = [[] for _ in range(G)]
    for f in range(len(pos)):
        degenerate += int(frames_of(pos[f], o_row, a_row, b_row, mode, dims)[3].sum())
        uvt, near = local_coordinates(pos[f], o_row, a_row, b_row, p_row, owner, mode, rc2, dims)
        i, j = np.nonzero(near)
        q = uvt[i, j]
        with np.errstate(invalid="ignore"):
            ok = ((q[:, 0] >= ex[0]) & (q[:, 0] <= ex[-1]) & (q[:, 1] >= ey[0]) & (q[:, 1] <= ey[-1])
                  & (q[:, 2] >= ez[0]) & (q[:, 2] <= ez[-1]))
        g = group_of[j]
        if keep_local:
            for m in range(G):
                local[m].append(q[g == m])
        q, g = q[ok], g[ok]
        np.add.at(counts, (g, bin_of(q[:, 0], ex), bin_of(q[:, 1], ey), bin_of(q[:, 2], ez)), 1)
        inside[f] = ok.sum()
    own = int((owner >= 0).sum())       # owner[j] names one molecule: one excluded pair per owned partner
    out = {"counts": counts, "inside": inside, "degenerate": degenerate, "frames": len(pos),
           "evaluations": len(pos) * (len(o_row) * len(p_row) - own)}
    if keep_local:
        out["local"] = [np.concatenate(rows) if rows else np.zeros((0, 3)) for rows in local]
    return out


def cube_edges(R, n):
    """``n`` bins (an int or three) of ``[-R, R]`` on every axis."""
    n = (n, n, n) if np.isscalar(n) else n
    return [np.linspace(-R, R, m + 1) for m in n]


def collect(eng):
    """What ``restate`` returns, of an engine."""
    got = {"counts": eng.result(), "inside": eng.inside()}
    stats = eng.stats()
    for key in ("evaluations", "frames", "degenerate"):
        got[key] = stats[key]
    return got


def assert_same(got, want):
    for key in ("counts", "inside"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert got[key].dtype == np.int64
    for key in ("evaluations", "frames", "degenerate"):
        assert got[key] == want[key], key
    assert got["counts"].sum() == got["inside"].sum()
