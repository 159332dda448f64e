"""
The diagonal of the cell-sorted pair kernel's self schedule, every pair once (``mdx_rdf_cell.hpp``; DESIGN.md §4,
row a-1), restated in NumPy.

An i tile holds two 64-particle halves, a (j tile 2 I) and b (2 I + 1).  The schedule of its two diagonal visits:
  visit 2 I      half a against itself by rotation — in step k = 0 .. 32 lane l meets row (l + k) & 63; weight 1 at
                 k = 0 and k = 32, weight 2 at k = 1 .. 31 — then rows of a against the lanes of b at weight 2;
  visit 2 I + 1  half b against itself by rotation, nothing else.
Every ORDERED pair of the 128 particles, (i, i) included, must come to weight 1, as under the old schedule (both
visits run all 64 rows of their tile against both halves at weight 1); a weight 2 stands for both orders of a pair.

The scheme applies to an i tile whose box half extents hI satisfy 3 hI < 0.4999 L in every component
(``cell_diag_once``), in float32 as the kernel evaluates it.  Both visits read the same hI and L, and the rule bounds
the reach of either visit's cull below 0.4999 L: image shift 0, no per-pair image search.
"""
import numpy as np

ROT_STEPS = 33       # CELL_DIAG_ROT_STEPS
f32 = np.float32


def rot_weight(k):
    return 2 if 1 <= k <= 31 else 1


def once_schedule():
    """Total weight of every ordered pair of the 128 particles of an i tile under the once-only schedule, and the
    wave steps it takes."""
    w = np.zeros((128, 128), dtype=np.int64)
    steps = 0
    lane = np.arange(64)
    for half in (0, 1):                        # visit 2 I: half a; visit 2 I + 1: half b
        for k in range(ROT_STEPS):
            i, j = 64 * half + lane, 64 * half + ((lane + k) & 63)
            if rot_weight(k) == 2:             # one evaluation stands for both orders
                np.add.at(w, (i, j), 1)
                np.add.at(w, (j, i), 1)
            else:
                np.add.at(w, (i, j), 1)
            steps += 1
    for row in range(64):                      # visit 2 I: row of a against the lanes of b, weight 2
        np.add.at(w, (64 + lane, row), 1)
        np.add.at(w, (row, 64 + lane), 1)
        steps += 1
    return w, steps


def old_schedule():
    w = np.zeros((128, 128), dtype=np.int64)
    steps = 0
    lane = np.arange(64)
    for tile in (0, 1):
        for row in range(64):
            for half in (0, 1):
                np.add.at(w, (64 * half + lane, 64 * tile + row), 1)
                steps += 1
    return w, steps


def test_every_ordered_pair_of_the_tile_gets_weight_one():
    w, steps = once_schedule()
    assert np.array_equal(w, np.ones((128, 128), dtype=np.int64))
    assert steps == 130


def test_the_old_schedule_gives_the_same_totals_in_256_steps():
    w, steps = old_schedule()
    assert np.array_equal(w, once_schedule()[0])
    assert steps == 256


def test_rotation_steps_1_to_31_reach_every_unordered_pair_once_and_32_from_both_sides():
    lane = np.arange(64)
    seen = np.zeros((64, 64), dtype=np.int64)
    for k in range(1, 32):
        np.add.at(seen, (np.minimum(lane, (lane + k) & 63), np.maximum(lane, (lane + k) & 63)), 1)
    d = (lane[None, :] - lane[:, None]) & 63
    upper = lane[:, None] < lane[None, :]
    assert np.array_equal(seen[upper & (d != 32)], np.ones(np.count_nonzero(upper & (d != 32)), dtype=np.int64))
    assert not seen[upper & (d == 32)].any() and not seen[~upper].any()
    both = np.zeros((64, 64), dtype=np.int64)
    np.add.at(both, (lane, (lane + 32) & 63), 1)
    assert np.array_equal(both, (d == 32).astype(np.int64))          # (l, l + 32) and (l + 32, l): each order once


# ------------------------------------------------------------------------------------------------- the rule

def diag_once(hI, L):
    """``cell_diag_once``: float32 products, compared per component."""
    hI, L = np.asarray(hI, dtype=f32), np.asarray(L, dtype=f32)
    return bool(np.all(f32(3.0) * hI < f32(0.4999) * L))


def tile_geometry(lo0, hi0, lo1, hi1):
    """Centre and half extent of the i tile's box and of its two halves, as lane 0 of the pair kernel forms them."""
    lo, hi = np.minimum(lo0, lo1), np.maximum(hi0, hi1)
    h = f32(0.5)
    return (h * (lo + hi), h * (hi - lo)), [(h * (a + b), h * (b - a)) for a, b in ((lo0, hi0), (lo1, hi1))]


def cull(cI, hI, cJ, hJ, L, cut):
    """First-level cull of one j tile against the i tile (orthorhombic): image shift and `general` bits, float32."""
    invL = (1.0 / L.astype(np.float64)).astype(f32)
    d = cJ - cI
    sft = np.rint(d * invL).astype(f32)
    d = (d.astype(np.float64) - sft.astype(np.float64) * L.astype(np.float64)).astype(f32)     # one rounding: the fma
    reach = np.abs(d) + (hI + hJ)
    halfL = f32(0.4999) * L
    general = ~(reach < halfL) & ~((cut < halfL) & (reach < L - cut - f32(1e-4) * L))
    return sft, general, reach


def _random_tiles(rng, n, near_sixth):
    L = rng.uniform(8.0, 120.0, (n, 3)).astype(f32)
    if near_sixth:      # tile half extents within a few ulp .. a few per cent of L / 6 (0.4999 / 3 = 0.16663)
        hI = (L.astype(np.float64) * 0.4999 / 3.0 * (1.0 + rng.choice([-1, 1], (n, 3)) * 10.0 ** rng.uniform(-7.5, -1.5, (n, 3))))
    else:
        hI = L.astype(np.float64) * rng.uniform(0.0, 0.25, (n, 3))
    centre = rng.uniform(0.0, 1.0, (n, 3)) * L
    lo, hi = (centre - hI).astype(f32), (centre + hI).astype(f32)
    # two halves inside [lo, hi] whose union touches it in every component
    cutp = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3)).astype(f32)
    swap = rng.random((n, 3)) < 0.5
    lo0 = np.where(swap, lo, np.minimum(cutp, lo + (hi - lo) * f32(0.3))).astype(f32)
    hi0 = np.where(swap, np.maximum(cutp, lo), hi).astype(f32)
    lo1 = np.where(swap, np.minimum(cutp, hi), lo).astype(f32)
    hi1 = np.where(swap, hi, np.maximum(cutp, lo)).astype(f32)
    return L, lo0, hi0, lo1, hi1


def test_the_rule_implies_shift_zero_and_no_image_search_in_both_diagonal_visits():
    rng = np.random.default_rng(18)
    held = failed = 0
    for near in (False, True):
        L, lo0, hi0, lo1, hi1 = _random_tiles(rng, 4000, near)
        for t in range(L.shape[0]):
            (cI, hI), halves = tile_geometry(lo0[t], hi0[t], lo1[t], hi1[t])
            # (the rule reads the i tile's box alone — the same words in either visit's item — not the visited half)
            if not diag_once(hI, L[t]):
                failed += 1
                continue
            held += 1
            for cJ, hJ in halves:
                for cut in (f32(3.0), f32(15.0), f32(0.49) * L[t].min()):
                    sft, general, reach = cull(cI, hI, cJ, hJ, L[t], cut)
                    assert not sft.any() and not general.any()
                    assert np.all(reach <= f32(3.0) * hI + f32(1e-5) * L[t])
    assert held > 1000 and failed > 1000


def test_the_rule_at_its_threshold():
    L = np.array([60.0, 60.0, 60.0], dtype=f32)
    assert diag_once([9.9, 9.9, 9.9], L)
    assert not diag_once([9.9, 10.0, 9.9], L)               # 30.0 against 29.994
    assert not diag_once([np.nan, 1.0, 1.0], L)             # no box: the old schedule
    assert diag_once([0.0, 0.0, 0.0], L)
