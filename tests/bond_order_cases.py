"""
What the bond-orientational order tests share (``test_bond_order_host.py``, ``test_gpu_bond_order.py``):

``restate`` — the float64 NumPy restatement of the device contract (csrc/mdx_bond_order_device.hpp), one operation at
a time: per frame, centre i and candidate j

    d = x_j - x_i;  s = d * (1.0 / L);  w = d - L * rint(s);  r2 = (wx*wx + wy*wy) + wz*wz;  neighbour = r2 <= rc2

per bond  r = sqrt(r2); u = w / r;  (c_0, s_0) = (1, 0), c_m = c_{m-1}*ux - s_{m-1}*uy, s_m = c_{m-1}*uy + s_{m-1}*ux;
T_m^m = (2m-1)!!, T_{m+1}^m = ((2m+1)*uz)*T_m^m, T_n^m = (a[n][m]*uz)*T_{n-1}^m - b[n][m]*T_{n-2}^m;  y = N[l][m]*T_l^m;
term = (y*c_m, y*s_m), with the host tables formed as the engine forms them; per centre the terms of its neighbours
added in ascending j by a Python loop over the slots of the sorted rows, q_lm = Q_lm / m_i, S and sqrt(k_l * S); the
averaged form alike; the frame sums through the two tile loops.  Every array operation below is elementwise, so each
element sees the scalar sequence of the contract.

``define`` — the independent definition with ``scipy.special.sph_harm_y`` over all m = -l ... l.

``fcc``, ``bcc``, ``sc`` — lattices with coordinates on an integer grid (exact in float32).
"""
import math

import numpy as np

MAX_DEGREE = 12
SUM_TILE = 64
FOUR_PI = 4.0 * 3.141592653589793

# The restatement and scipy differ only by the roundings of a few hundred operations.  Largest differences seen on the
# CPU (the inputs of test_bond_order_host.py, l = 1 ... 12): 4.5e-15 against the definition (1.2e-15 on the clusters,
# plain and rotated, 4.5e-15 across the faces of a box), 1.0e-15 between a cluster and its rotated copy, 5.6e-16
# against the closed forms, 2.3e-16 between qbar_l and q_l on a lattice.  Each bound is 16 times what was seen, so
# that another libm has room.
TOL_DEFINITION = 16 * 4.5e-15
TOL_ROTATION = 16 * 1.0e-15
TOL_CLOSED = 16 * 5.6e-16
TOL_AVERAGED = 16 * 2.3e-16


def tables():
    """a[n][m], b[n][m], N[l][m], k[l] as float64: exact integers first, then one division (and one sqrt)."""
    size = MAX_DEGREE + 1
    a, b, norm, k = np.zeros((size, size)), np.zeros((size, size)), np.zeros((size, size)), np.zeros(size)
    for n in range(size):
        for m in range(n - 1):
            a[n, m] = float(2 * n - 1) / float(n - m)
            b[n, m] = float(n + m - 1) / float(n - m)
    for l in range(size):
        for m in range(l + 1):
            product = math.factorial(l + m) // math.factorial(l - m)       # an exact integer; float() rounds it once
            root = math.sqrt(float(2 * l + 1) / (FOUR_PI * float(product)))
            norm[l, m] = -root if m % 2 else root
        k[l] = FOUR_PI / float(2 * l + 1)
    return a, b, norm, k


A, B, NORM, K_L = tables()
DOUBLE_FACTORIAL = [float(np.prod(np.arange(1, 2 * m, 2, dtype=np.int64))) for m in range(MAX_DEGREE + 1)]


def bond_terms(ux, uy, uz, l):
    """(re, im), float64 [l + 1, bonds]: Y_lm of every bond, m = 0 ... l, by the contract's recurrences."""
    re, im = np.zeros((l + 1,) + ux.shape), np.zeros((l + 1,) + ux.shape)
    c, s = np.ones_like(ux), np.zeros_like(ux)
    for m in range(l + 1):
        if m > 0:
            c_next = c * ux - s * uy
            s = c * uy + s * ux
            c = c_next
        below = np.full_like(ux, DOUBLE_FACTORIAL[m])
        T = below
        if m < l:
            T = (float(2 * m + 1) * uz) * below
            for n in range(m + 2, l + 1):
                T, below = (A[n, m] * uz) * T - B[n, m] * below, T
        y = NORM[l, m] * T
        re[m] = y * c
        im[m] = y * s
    return re, im


def invariant(re, im, l):
    """sqrt(k_l * S), S = re_0^2, then + 2 (re_m^2 + im_m^2) for m = 1 ... l; re, im [l + 1, centres]."""
    S = re[0] * re[0]
    for m in range(1, l + 1):
        S = S + 2.0 * (re[m] * re[m] + im[m] * im[m])
    return np.sqrt(K_L[l] * S)


def neighbours(x, n0, same, cutoff, dims):
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


def rows_of(near):
    """(m int [n0], row int [n0, max m]): every centre's neighbours in ascending j, -1 behind them."""
    m = near.sum(axis=1)
    row = np.full((len(near), max(int(m.max()), 1)), -1, dtype=np.int64)
    for i in range(len(near)):
        row[i, :m[i]] = np.flatnonzero(near[i])
    return m, row


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


def restate(pos, n0, n1, cutoff, degrees, edges, dims, *, same=False, averaged=False, max_neighbors=32):
    """Every result of the engine for float32 pos[F, rows, 3]: the n0 centres, then the n1 candidates (with `same` the
    centres alone).  coordination is [max_neighbors + 1] where no row goes beyond the cap, which the caller asserts
    through max_row."""
    x_all = np.asarray(pos).astype(np.float64)
    F = len(x_all)
    n1 = n0 if same else n1
    degrees = [int(l) for l in np.atleast_1d(degrees)]
    D, K = len(degrees), 2 if averaged else 1
    edges = np.asarray(edges, dtype=np.float64)
    n_bins = len(edges) - 1
    width = max(max_neighbors, n1) + 1
    values = np.full((F, D, K, n0), np.nan)
    sums, counted = np.zeros((F, D, K)), np.zeros(F, dtype=np.int64)
    counts, outside = np.zeros((D, K, n_bins), dtype=np.int64), np.zeros((D, K), dtype=np.int64)
    coordination = np.zeros(width, dtype=np.int64)
    bonds = degenerate = max_row = 0
    for f in range(F):
        near, w, r2 = neighbours(x_all[f], n0, same, float(cutoff), dims)
        m, row = rows_of(near)
        coordination += np.bincount(m, minlength=width)
        bonds += int(m.sum())
        degenerate += int((r2[near] == 0.0).sum())
        max_row = max(max_row, int(m.max()))
        counted[f] = int((m > 0).sum())
        have = m > 0
        for d, l in enumerate(degrees):
            Q_re, Q_im = np.zeros((l + 1, n0)), np.zeros((l + 1, n0))
            for s in range(int(m.max())):                   # slot by slot: ascending j
                i = np.flatnonzero(m > s)
                j = row[i, s]
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.sqrt(r2[i, j])
                    ux, uy, uz = w[i, j, 0] / r, w[i, j, 1] / r, w[i, j, 2] / r
                    re, im = bond_terms(ux, uy, uz, l)
                Q_re[:, i] = Q_re[:, i] + re
                Q_im[:, i] = Q_im[:, i] + im
            q_re, q_im = np.full((l + 1, n0), np.nan), np.full((l + 1, n0), np.nan)
            q_re[:, have] = Q_re[:, have] / m[have].astype(np.float64)
            q_im[:, have] = Q_im[:, have] / m[have].astype(np.float64)
            values[f, d, 0] = invariant(q_re, q_im, l)
            if averaged:
                A_re, A_im = q_re.copy(), q_im.copy()
                for s in range(int(m.max())):
                    i = np.flatnonzero(m > s)
                    j = row[i, s]
                    A_re[:, i] = A_re[:, i] + q_re[:, j]
                    A_im[:, i] = A_im[:, i] + q_im[:, j]
                count = (m + 1).astype(np.float64)
                values[f, d, 1] = invariant(A_re / count, A_im / count, l)
                values[f, d, 1, ~have] = np.nan
            for k in range(K):
                v = values[f, d, k]
                sums[f, d, k] = tile_sum(v)
                v = v[~np.isnan(v)]
                inside = (v >= edges[0]) & (v <= edges[-1])
                outside[d, k] += int((~inside).sum())
                counts[d, k] += np.bincount(np.searchsorted(edges[1:-1], v[inside], side="right"), minlength=n_bins)
    if max_row <= max_neighbors:
        assert not coordination[max_neighbors + 1:].any()
        coordination = coordination[:max_neighbors + 1].copy()
    return {"values": values, "sums": sums, "counted": counted, "counts": counts, "outside": outside,
            "coordination": coordination, "evaluations": F * (n0 * n1 - (n0 if same else 0)), "frames": F,
            "bonds": bonds, "degenerate": degenerate, "max_row": max_row}


def define(pos, n0, cutoff, degrees, dims, *, same=True, averaged=False):
    """values [F, D, K, n0] from the definition: scipy's Y_lm over all m = -l ... l, numpy's own sums."""
    from scipy.special import sph_harm_y
    x_all = np.asarray(pos).astype(np.float64)
    degrees = [int(l) for l in np.atleast_1d(degrees)]
    out = np.full((len(x_all), len(degrees), 2 if averaged else 1, n0), np.nan)
    for f, x in enumerate(x_all):
        near, w, r2 = neighbours(x, n0, same, float(cutoff), dims)
        theta = np.arccos(np.clip(w[..., 2] / np.sqrt(np.where(near, r2, 1.0)), -1.0, 1.0))
        phi = np.arctan2(w[..., 1], w[..., 0])
        m_i = near.sum(axis=1)
        for d, l in enumerate(degrees):
            orders = np.arange(-l, l + 1)
            Y = sph_harm_y(l, orders[:, None, None], theta[None], phi[None])       # [2l + 1, n0, n1]
            with np.errstate(invalid="ignore", divide="ignore"):
                q_lm = np.where(near[None], Y, 0.0).sum(axis=2) / m_i
                out[f, d, 0] = np.sqrt(4.0 * np.pi / (2 * l + 1) * (np.abs(q_lm) ** 2).sum(axis=0))
                if averaged:
                    q_safe = np.where(m_i[None] > 0, q_lm, 0.0)
                    bar = (q_lm + q_safe @ near.T.astype(np.float64)) / (m_i + 1)
                    out[f, d, 1] = np.sqrt(4.0 * np.pi / (2 * l + 1) * (np.abs(bar) ** 2).sum(axis=0))
    return out


# ---------------------------------------------------------------- lattices

def _lattice(basis, cells, a):
    grid = np.array([(i, j, k) for i in range(cells) for j in range(cells) for k in range(cells)], dtype=np.float64) * a
    points = (grid[:, None, :] + np.asarray(basis, dtype=np.float64)[None] * (a / 2)).reshape(-1, 3)
    frame = points.astype(np.float32)
    assert np.array_equal(frame.astype(np.float64), points)             # on an integer grid: exact in float32
    return frame[None], np.full(3, float(cells * a))


def fcc(cells=4, a=2):
    """(pos float32 [1, 4 cells^3, 3], dims): 12 neighbours at a / sqrt(2) within cutoff 1.7 (a = 2)."""
    return _lattice([(0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)], cells, a)


def bcc(cells=4, a=2):
    """... 2 cells^3 points: 8 neighbours at a sqrt(3) / 2 within cutoff 1.9 (a = 2)."""
    return _lattice([(0, 0, 0), (1, 1, 1)], cells, a)


def sc(cells=4, a=2):
    """... cells^3 points: 6 neighbours at a within cutoff 2.5 (a = 2)."""
    return _lattice([(0, 0, 0)], cells, a)


LATTICES = {"fcc": (fcc, 1.7, 12, {4: math.sqrt(7 / 192), 6: math.sqrt(169 / 512)}),
            "bcc": (bcc, 1.9, 8, {4: math.sqrt(7 / 27), 6: math.sqrt(32 / 81)}),
            "sc": (sc, 2.5, 6, {4: math.sqrt(7 / 12), 6: math.sqrt(1 / 8)})}


def cloud(seed, F, n, dims):
    """Uniform random points in the box: float32 [F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    pos = (rng.uniform(0.0, 1.0, (F, n, 3)) * dims).astype(np.float32)
    pos[pos >= dims.astype(np.float32)] = 0.0              # float32 rounding at the upper face
    return pos
