"""
What the tetrahedral order tests share (``test_tetrahedral_host.py``, ``test_gpu_tetrahedral.py``):

``restate`` — the float64 NumPy restatement of the device contract (csrc/mdx_tetrahedral_device.hpp), one operation at
a time: per frame, centre i and candidate j

    d = x_j - x_i;  s = d * (1.0 / L);  w = d - L * rint(s);  r2 = (wx*wx + wy*wy) + wz*wz;  in range = r2 <= rc2

the candidates in range of a centre ordered with ``np.lexsort((j, r2))`` (ascending r2, ties by ascending j), the first
``k`` of them its neighbours, ``q`` and ``S_k`` of the first four by ``q_sk`` and the counts by ``numpy.histogram``
(the distances as ``sqrt(r2)`` against distance edges); the frame sums through the two tile loops.  Every array
operation below is elementwise, so each element sees the scalar sequence of the contract.

``textbook_q`` — the independent definition through ``arccos`` and ``cos``.

``sc``, ``diamond`` — lattices with coordinates on an integer grid (exact in float32).
"""
import numpy as np

SUM_TILE = 64
THIRD = 1.0 / 3.0
PAIRS = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))       # the contract's order


def pairs(x, n0, same, cutoff, dims):
    """(near bool [n0, n1], w float64 [n0, n1, 3], r2 [n0, n1]) of one float64 frame."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    xc = x[:n0]
    xl = xc if same else x[n0:]
    d = xl[None, :, :] - xc[:, None, :]
    s = d * inv
    w = d - dims * np.rint(s)
    r2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    near = r2 <= cutoff * cutoff
    if same:
        near &= ~np.eye(n0, dtype=bool)
    return near, w, r2


def ordered(near_row, r2_row):
    """The candidates in range of one centre in the contract's total order."""
    j = np.flatnonzero(near_row)
    return j[np.lexsort((j, r2_row[j]))]


def q_sk(w, r2):
    """(q, S_k) of centres whose four nearest have w [..., 4, 3] and r2 [..., 4], in the contract's operations."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(r2)
        acc = np.zeros(r2.shape[:-1])
        for a, b in PAIRS:
            dot = (w[..., a, 0] * w[..., b, 0] + w[..., a, 1] * w[..., b, 1]) + w[..., a, 2] * w[..., b, 2]
            c = dot / np.sqrt(r2[..., a] * r2[..., b])
            t = c + THIRD
            acc = acc + t * t
        q = 1.0 - 0.375 * acc
        total = np.zeros(r2.shape[:-1])
        for a in range(4):
            total = total + r[..., a]
        rbar = total * 0.25
        v = np.zeros(r2.shape[:-1])
        for a in range(4):
            e = r[..., a] - rbar
            v = v + e * e
        sk = 1.0 - v / (12.0 * (rbar * rbar))
    return q, sk


def r2_of(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def textbook_q(w):
    """q of w [..., 4, 3] through the angles themselves: 1 - 3/8 sum (cos(psi) + 1/3)^2, psi from arccos."""
    u = w / np.linalg.norm(w, axis=-1, keepdims=True)
    total = 0.0
    for a in range(4):
        for b in range(a + 1, 4):
            psi = np.arccos(np.clip((u[..., a, :] * u[..., b, :]).sum(axis=-1), -1.0, 1.0))
            total = total + (np.cos(psi) + 1.0 / 3.0) ** 2
    return 1.0 - 3.0 / 8.0 * total


def tile_sum(values):
    """The values of one frame's centres added per tile of 64 in row order from +0.0 (a NaN left out), then the tiles
    in tile order from +0.0."""
    total = 0.0
    for t0 in range(0, len(values), SUM_TILE):
        part = 0.0
        for v in values[t0:t0 + SUM_TILE]:
            if v == v:
                part = part + float(v)
        total = total + part
    return total


def histogram(x, edges):
    """(counts, outside) as numpy.histogram counts: NaN never appears here."""
    counts = np.histogram(x, bins=edges)[0].astype(np.int64)
    return counts, int(len(x) - counts.sum())


def restate(pos, n0, n1, cutoff, k, q_edges, s_edges, d_edges, dims, *, same=False):
    """Every result of the engine for float32 pos[F, rows, 3]: the n0 centres, then the n1 candidates (with `same` the
    centres alone).  d_edges are edges of the distance, not of r2.  Also `in_range` [F, n0], the m_i."""
    x_all = np.asarray(pos).astype(np.float64)
    F = len(x_all)
    n1 = n0 if same else n1
    q_edges, s_edges, d_edges = (np.asarray(e, dtype=np.float64) for e in (q_edges, s_edges, d_edges))
    values = np.full((F, 2, n0), np.nan)
    neighbors = np.full((F, k, n0), -1, dtype=np.int32)
    in_range = np.zeros((F, n0), dtype=np.int64)
    sums, counted = np.zeros((F, 2)), np.zeros(F, dtype=np.int64)
    q_counts, s_counts = np.zeros(len(q_edges) - 1, dtype=np.int64), np.zeros(len(s_edges) - 1, dtype=np.int64)
    outside = np.zeros(2, dtype=np.int64)
    distance_counts = np.zeros((k, len(d_edges) - 1), dtype=np.int64)
    distance_outside = np.zeros(k, dtype=np.int64)
    found = np.zeros(k + 1, dtype=np.int64)
    degenerate = 0
    for f in range(F):
        near, w, r2 = pairs(x_all[f], n0, same, float(cutoff), dims)
        in_range[f] = near.sum(axis=1)
        for i in range(n0):
            nb = ordered(near[i], r2[i])[:k]
            neighbors[f, :len(nb), i] = nb
        have = neighbors[f] >= 0                                    # [k, n0]
        found += np.bincount(have.sum(axis=0), minlength=k + 1)
        for a in range(k):
            i = np.flatnonzero(have[a])
            counts, out = histogram(np.sqrt(r2[i, neighbors[f, a, i]]), d_edges)
            distance_counts[a] += counts
            distance_outside[a] += out
        full = np.flatnonzero(have[3])
        four = neighbors[f, :4, full].reshape(len(full), 4)          # [centres, 4]
        w4, r4 = w[full[:, None], four], r2[full[:, None], four]
        values[f, 0, full], values[f, 1, full] = q_sk(w4, r4)
        degenerate += int((r4 == 0.0).sum())
        counted[f] = len(full)
        for which, (edges, counts) in enumerate(((q_edges, q_counts), (s_edges, s_counts))):
            v = values[f, which]
            sums[f, which] = tile_sum(v)
            got, out = histogram(v[~np.isnan(v)], edges)
            counts += got
            outside[which] += out
    return {"values": values, "neighbors": neighbors, "sums": sums, "counted": counted, "q_counts": q_counts,
            "s_counts": s_counts, "outside": outside, "distance_counts": distance_counts,
            "distance_outside": distance_outside, "found": found, "in_range": in_range,
            "evaluations": F * (n0 * n1 - (n0 if same else 0)), "frames": F, "degenerate": degenerate}


# ---------------------------------------------------------------- systems

def _exact(points):
    frame = points.astype(np.float32)
    assert np.array_equal(frame.astype(np.float64), points)          # on an integer grid: exact in float32
    return frame[None]


def sc(cells=11):
    """(pos float32 [1, cells^3, 3], dims): a simple-cubic lattice on integer coordinates in a box of `cells`; site
    (x, y, z) is row (x * cells + y) * cells + z, and its six neighbours have r2 == 1.0 bit for bit."""
    grid = np.array([(i, j, k) for i in range(cells) for j in range(cells) for k in range(cells)], dtype=np.float64)
    return _exact(grid), np.full(3, float(cells))


def diamond(cells=3):
    """(pos float32 [1, 8 cells^3, 3], dims): diamond with cell edge 4.0; four neighbours with r2 == 3.0, the next
    twelve at r2 == 8.0."""
    basis = np.array([(0, 0, 0), (0, 2, 2), (2, 0, 2), (2, 2, 0), (1, 1, 1), (1, 3, 3), (3, 1, 3), (3, 3, 1)],
                     dtype=np.float64)
    grid = np.array([(i, j, k) for i in range(cells) for j in range(cells) for k in range(cells)],
                    dtype=np.float64) * 4.0
    return _exact((grid[:, None, :] + basis[None]).reshape(-1, 3)), np.full(3, 4.0 * cells)


def cloud(seed, F, n, dims):
    """Uniform random points in the box: float32 [F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    pos = (rng.uniform(0.0, 1.0, (F, n, 3)) * dims).astype(np.float32)
    pos[pos >= dims.astype(np.float32)] = 0.0              # float32 rounding at the upper face
    return pos


def box_for(n, neighbours, cutoff):
    """The cubic box in which n uniform points have about `neighbours` others within the cutoff, at least twice the
    cutoff and a little more long."""
    shell = 4.0 / 3.0 * np.pi * cutoff ** 3
    return np.full(3, max(2.0 * cutoff + 0.5, float(np.ceil(4.0 * (n * shell / neighbours) ** (1.0 / 3.0)) / 4.0)))
