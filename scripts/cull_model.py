"""Evaluations per binned pair for (G_i x G_j) particle-group culling on a C2-like frame sorted the way
rdf_cell_sort_kernel sorts (columns a x a, thin layers, serpentine)."""
import numpy as np
rng = np.random.default_rng(0)
N, L, R = 32768, 68.94, 15.0
pos = rng.random((N, 3)) * L
a = (64 * L**3 / N) ** (1 / 3)
nc0 = nc1 = max(int(round(L / a)), 1)
nc2 = max(int(round(16 * L / a)), 1)
c = np.minimum((pos / L * [nc0, nc1, nc2]).astype(int), [nc0 - 1, nc1 - 1, nc2 - 1])
cx, cy, cz = c[:, 0], c[:, 1].copy(), c[:, 2].copy()
cy = np.where(cx & 1, nc1 - 1 - cy, cy)
col = cx * nc1 + cy
cz = np.where(col & 1, nc2 - 1 - cz, cz)
key = col * nc2 + cz
order = np.argsort(key, kind="stable")
P = pos[order]

def boxes(G):
    g = P.reshape(N // G, G, 3)
    return g.min(1), g.max(1)

def gap2(lo_i, hi_i, lo_j, hi_j):
    # minimum-image gap between boxes (centre difference folded)
    ci, hi_ = 0.5 * (lo_i + hi_i), 0.5 * (hi_i - lo_i)
    cj, hj_ = 0.5 * (lo_j + hi_j), 0.5 * (hi_j - lo_j)
    d = cj[None] - ci[:, None]
    d -= L * np.rint(d / L)
    g = np.maximum(0.0, np.abs(d) - hi_[:, None] - hj_[None])
    return (g * g).sum(-1)

# binned (ordered) pairs per particle: 4/3 pi R^3 rho
binned_per_i = 4 / 3 * np.pi * R**3 * N / L**3
for Gi, Gj in [(64, 1), (64, 8), (32, 1), (8, 8), (16, 4), (8, 4), (4, 4), (16, 8)]:
    li, hi = boxes(Gi)
    lj, hj = boxes(Gj)
    sel = rng.choice(len(li), 64, replace=False)
    g2 = gap2(li[sel], hi[sel], lj, hj)
    surv = (g2 <= R * R).sum(1).mean()          # j groups per i group
    evals_per_i = surv * Gj                       # each i particle evaluated against surv*Gj j particles
    print(f"G_i={Gi:3d} G_j={Gj:3d}: evaluations per binned pair {evals_per_i / binned_per_i:.2f}   "
          f"(trips of 64 lanes per frame, unordered: {N * evals_per_i / 64 / 2:.3e})")

print("--- Morton order on fine cells")
def morton_order(cells_per_axis):
    c = np.minimum((pos / L * cells_per_axis).astype(np.int64), cells_per_axis - 1)
    def spread(v):
        out = np.zeros_like(v)
        for b in range(10):
            out |= ((v >> b) & 1) << (3 * b)
        return out
    return np.argsort(spread(c[:, 0]) | (spread(c[:, 1]) << 1) | (spread(c[:, 2]) << 2), kind="stable")
for cpa in (16, 32, 64):
    P = pos[morton_order(cpa)]
    for Gi, Gj in [(64, 1), (8, 8), (8, 4), (16, 4), (4, 4), (32, 2)]:
        li, hi = boxes(Gi); lj, hj = boxes(Gj)
        sel = rng.choice(len(li), 64, replace=False)
        surv = (gap2(li[sel], hi[sel], lj, hj) <= R * R).sum(1).mean()
        print(f"cells/axis {cpa:3d} G_i={Gi:3d} G_j={Gj:3d}: evaluations per binned pair {surv * Gj / binned_per_i:.2f}")


# ---------------------------------------------------------------------------------------------
# Second model: the two 32-lane halves of a wave take different j rows where a row is needed by one
# 32-particle quarter only (rows paired up within a tile visit).
def quarter_model():
    rng = np.random.default_rng(1)
    N, L, R = 32768, 68.94, 15.0
    pos = rng.random((N, 3)) * L
    a = (64 * L**3 / N) ** (1 / 3)
    nc0 = nc1 = max(int(round(L / a)), 1); nc2 = max(int(round(16 * L / a)), 1)
    c = np.minimum((pos / L * [nc0, nc1, nc2]).astype(int), [nc0 - 1, nc1 - 1, nc2 - 1])
    cx, cy, cz = c[:, 0], c[:, 1].copy(), c[:, 2].copy()
    cy = np.where(cx & 1, nc1 - 1 - cy, cy); col = cx * nc1 + cy
    cz = np.where(col & 1, nc2 - 1 - cz, cz)
    P = pos[np.argsort(col * nc2 + cz, kind="stable")]

    def box(g):
        return g.min(0), g.max(0)
    def reach(lo, hi, pts):
        """rows (points) within R of the box, minimum image per component"""
        cen, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        d = pts - cen; d -= L * np.rint(d / L)
        g = np.maximum(0.0, np.abs(d) - half)
        return (g * g).sum(-1) <= R * R

    old = new = new_union = vis = 0
    tiles = rng.choice(N // 64, 48, replace=False)
    for t in tiles:
        I = P[t * 64:(t + 1) * 64]
        lo, hi = box(I)
        (loA, hiA), (loB, hiB) = box(I[:32]), box(I[32:])
        H = reach(lo, hi, P).reshape(-1, 64)
        A = reach(loA, hiA, P).reshape(-1, 64)
        B = reach(loB, hiB, P).reshape(-1, 64)
        for j in range(N // 64):
            h = H[j].sum()
            if not h:
                continue
            vis += 1
            old += h
            both = (A[j] & B[j]).sum(); xa = (A[j] & ~B[j]).sum(); xb = (B[j] & ~A[j]).sum()
            new += both + max(xa, xb)
            new_union += (A[j] | B[j]).sum()
    print(f"visits per (64-half): {vis / len(tiles):.1f}; rows per visit old {old / vis:.1f}")
    print(f"trips: old {old / len(tiles):.0f} per half-tile; union of quarters {new_union / len(tiles):.0f} "
          f"({new_union / old:.3f}); paired {new / len(tiles):.0f} ({new / old:.3f})")


quarter_model()


# ---------------------------------------------------------------------------------------------
# Third model: candidates per wave step.  A step is one j row against the 64 particles of an i unit; the row
# loops run the rows within R of the unit's BOX.  How many of the 64 lanes (and of each 32-lane half) then hold a
# pair within R — and how many steps hold none, which cell_step<..., SKIP> leaves behind its candidate test?
def step_model(units=40):
    rng = np.random.default_rng(2)
    N, L, R = 32768, 68.94, 15.0
    pos = rng.random((N, 3)) * L
    a = (64 * L**3 / N) ** (1 / 3)
    nc0 = nc1 = max(int(round(L / a)), 1); nc2 = max(int(round(16 * L / a)), 1)
    c = np.minimum((pos / L * [nc0, nc1, nc2]).astype(int), [nc0 - 1, nc1 - 1, nc2 - 1])
    cx, cy, cz = c[:, 0], c[:, 1].copy(), c[:, 2].copy()
    cy = np.where(cx & 1, nc1 - 1 - cy, cy); col = cx * nc1 + cy
    cz = np.where(col & 1, nc2 - 1 - cz, cz)
    P = pos[np.argsort(col * nc2 + cz, kind="stable")]

    def reach(I, pts):
        """points within R of the box of the particles I, minimum image per component"""
        lo, hi = I.min(0), I.max(0)
        d = pts - 0.5 * (lo + hi); d -= L * np.rint(d / L)
        g = np.maximum(0.0, np.abs(d) - 0.5 * (hi - lo))
        return (g * g).sum(-1) <= R * R

    hist = np.zeros(65, dtype=np.int64)
    half_empty = halves = 0
    kept = {2: 0, 8: 0}          # empty steps a finer box test (2 x 32, 8 x 8 particles) would still run
    for t in rng.choice(N // 64, units, replace=False):
        I = P[t * 64:(t + 1) * 64]
        rows = P[reach(I, P)]
        d = rows[:, None, :] - I[None]
        d -= L * np.rint(d / L)
        cand = (d * d).sum(-1) < R * R                       # [rows, 64 lanes]
        hist += np.bincount(cand.sum(1), minlength=65)
        h = cand.reshape(len(rows), 2, 32).sum(2)
        half_empty += (h == 0).sum(); halves += h.size
        empty = rows[cand.sum(1) == 0]
        for parts in kept:
            g = 64 // parts
            kept[parts] += np.logical_or.reduce([reach(I[k * g:(k + 1) * g], empty) for k in range(parts)]).sum()
    steps = hist.sum()
    print("--- candidates per wave step (64-particle unit x rows within R of its box)")
    print(f"units {units}, steps {steps}, candidate lanes {(hist * np.arange(65)).sum() / (64 * steps):.3f} of all lanes")
    print(f"steps with no candidate: {hist[0] / steps:.3f} per 64 lanes, {half_empty / halves:.3f} per 32-lane half")
    for k in (1, 2, 4, 8, 16, 32):
        print(f"steps with at most {k:2d} candidates: {hist[:k + 1].sum() / steps:.3f}")
    for parts, n in kept.items():
        print(f"empty steps kept by a test against {parts} boxes of {64 // parts} particles: {n / max(hist[0], 1):.3f}")


step_model()
