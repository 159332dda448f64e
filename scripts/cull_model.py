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


# ---------------------------------------------------------------------------------------------
# Fourth model: how evenly the four waves of a block end an item.  One uniform C2 frame in the sort kernel's
# column / layer order; items are 128-particle i tiles I with the self schedule J >= 2 I over the 64-particle
# j tiles; a tile is visited when its box comes within R of the item's 128-particle box, and a visit runs one
# trip per (row, 64-particle half) whose row comes within R of the half's box.  Four waves take the visits
# greedily in queue (J) order; `visit_cost` trip-equivalents are charged per visit for the pop and the staging.
# Idle share at the closing barrier = 1 - work / (4 x length of the longest wave).
def item_model():
    rng = np.random.default_rng(3)
    N, L, R = 32768, 68.94, 15.0
    pos = rng.random((N, 3)) * L
    a = (64 * L**3 / N) ** (1 / 3)
    nc0 = nc1 = max(int(round(L / a)), 1); nc2 = max(int(round(16 * L / a)), 1)
    c = np.minimum((pos / L * [nc0, nc1, nc2]).astype(int), [nc0 - 1, nc1 - 1, nc2 - 1])
    cx, cy, cz = c[:, 0], c[:, 1].copy(), c[:, 2].copy()
    cy = np.where(cx & 1, nc1 - 1 - cy, cy); col = cx * nc1 + cy
    cz = np.where(col & 1, nc2 - 1 - cz, cz)
    P = pos[np.argsort(col * nc2 + cz, kind="stable")]
    T = P.reshape(N // 64, 64, 3)
    tlo, thi = T.min(1), T.max(1)

    def box_gap2(lo, hi, cen, half):
        """squared minimum-image gap between the box (lo, hi) and boxes / points (cen, half)"""
        d = cen - 0.5 * (lo + hi); d -= L * np.rint(d / L)
        g = np.maximum(0.0, np.abs(d) - 0.5 * (hi - lo) - half)
        return (g * g).sum(-1)

    visits_per_item, trips_of_visits, trips_old = [], [], 0
    for I in range(N // 128):
        i0, i1 = T[2 * I], T[2 * I + 1]
        lo, hi = np.minimum(tlo[2 * I], tlo[2 * I + 1]), np.maximum(thi[2 * I], thi[2 * I + 1])
        J = np.arange(2 * I, N // 64)
        J = J[box_gap2(lo, hi, 0.5 * (tlo[J] + thi[J]), 0.5 * (thi[J] - tlo[J])) <= R * R]
        rows = T[J]                                                        # [visits, 64, 3]
        t0 = (box_gap2(i0.min(0), i0.max(0), rows, 0.0) <= R * R).sum(1)
        t1 = (box_gap2(i1.min(0), i1.max(0), rows, 0.0) <= R * R).sum(1)
        t = t0 + t1
        trips_old += t.sum()
        # the diagonal, every pair once (round 18; the tile's half extents are far below L / 6 here): visit 2 I is 33
        # rotated steps of half a and the rows of a within R of b's box, visit 2 I + 1 the 33 rotated steps of half b
        assert J[0] == 2 * I and J[1] == 2 * I + 1 and np.all(3.0 * 0.5 * (hi - lo) < 0.4999 * L)
        t[0], t[1] = 33 + t1[0], 33
        visits_per_item.append(len(J))
        trips_of_visits.append(t)
    allt = np.concatenate(trips_of_visits)
    print("--- the four waves of a block around an item (one frame, 256 items)")
    print(f"trips per frame with both diagonal visits in full {trips_old:.7g}, every diagonal pair once {allt.sum():.7g} "
          f"({trips_old - allt.sum():.0f} fewer, {1.0 - allt.sum() / trips_old:.4f})")
    print(f"trips per frame {allt.sum():.4g}; visits per item {np.mean(visits_per_item):.1f} "
          f"(max {max(visits_per_item)}); trips per visit {allt.mean():.1f}")
    print(f"visits with no trip: {(allt == 0).mean():.3f}; with at most 8 trips: {(allt <= 8).mean():.3f}, "
          f"holding {allt[allt <= 8].sum() / allt.sum():.3f} of the trips")
    for visit_cost in (0, 6):
        length, work = [], 0
        for t in trips_of_visits:
            waves = np.zeros(4)
            for v in t + visit_cost:                                       # greedy: the wave that is free first
                waves[waves.argmin()] += v
            length.append(waves.max())
            work += waves.sum()
        length = np.array(length)
        print(f"{visit_cost} trip-equivalents per visit: item length {length.mean():.0f} trip units (max {length.max():.0f}), "
              f"idle share at the closing barrier {1.0 - work / (4.0 * length.sum()):.3f}")
    own = np.array([t.sum() for t in trips_of_visits])
    print(f"an item owned by one wave: {own.mean():.0f} trip units (max {own.max()}); the last 32 items dealt of a "
          f"frame {own[-32:].mean():.0f}")


item_model()
