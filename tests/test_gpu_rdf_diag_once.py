"""
The two diagonal visits of an i tile of the cell-sorted pair kernel evaluate every pair of the tile once (rotation steps
of a half against itself, a x b at weight 2 in the first visit alone: ``mdx_rdf_cell.hpp``; the schedule
itself is restated in ``test_rdf_diag_once_host.py``).  Every case here is a call whose counts must EQUAL those of
``oracle.cbind.c_radial_histogram``.

Shapes: particle counts around one and two 64-particle halves and one to three i tiles, so that a call is nothing but
the diagonal (N <= 128), has padding rows inside a diagonal tile, or mixes diagonal and off-diagonal tile pairs; with
and without exclusion (the k = 0 step drops out by its tags or has to run); ranges from 0 and from r0 > 0, ending at 3
(the a x b rows are culled against the other half's box) and beyond the tile's diameter.  Where the range covers the
whole cluster every cull passes and the number of wave steps is known exactly: ``expected_units``.  Particles of one
tile on bin edges and on top of each other send pairs of the rotated steps and of the a x b rows to the exact
arithmetic under the index the step lists them with; a brick dense in such pairs overflows the wave's list inside a
diagonal visit, which is then redone in the old order.  A tile too large against its box, a two-set call and a
triclinic call keep the old schedule.
"""
import functools

import numpy as np
import pytest

from mdhelper_amd import _core
from oracle.cbind import c_radial_histogram
from rdf_cases import set_env

BOX60 = (60.0, 61.0, 62.0, 90.0, 90.0, 90.0)        # 0.3 x 60 = 18: a range end of 15 keeps the skipping step
BOX40 = (40.0, 41.0, 42.0, 90.0, 90.0, 90.0)        # 0.3 x 40 = 12: a range end of 15 takes the unconditional tail
TRI = (31.0, 28.5, 35.25, 75.0, 80.0, 110.0)
# the cluster: 5 x 5 x 12, diameter 13.9 — half extents (2.5, 2.5, 6) are below a sixth of either box
CLUSTER = np.array([5.0, 5.0, 12.0])
COUNTS = (64, 65, 127, 128, 129, 192, 256, 320)
# (box, range, bins): skip kernel to 3 and beyond the cluster; LOWER; the kernel without the skip
RANGES = ((BOX60, (0.0, 3.0), 30), (BOX60, (0.0, 15.0), 75), (BOX60, (1.5, 15.0), 54), (BOX60, (1.0, 3.0), 20),
          (BOX40, (0.0, 15.0), 75))


def _cluster(rng, n, size=CLUSTER, origin=(10.0, 11.0, 12.0)):
    return (np.asarray(origin) + rng.random((n, 3)) * size).astype(np.float32)


def _lattice_subset(rng, n, dims, origin=(10.0, 10.0, 10.0), twins=0):
    """n distinct sites of a dims[0] x dims[1] x dims[2] lattice of constant 0.5 = five bin widths of (0, 6) / 60:
    coordinates and differences are exact and every pair along an axis sits exactly on a bin edge; the last `twins`
    particles lie exactly on the first `twins` (distinct particles at distance 0)."""
    total = dims[0] * dims[1] * dims[2]
    pick = rng.choice(total, n - twins, replace=False)
    xyz = np.stack(np.unravel_index(pick, dims), axis=-1).astype(np.float32) * np.float32(0.5)
    xyz += np.asarray(origin, dtype=np.float32)
    return np.concatenate((xyz, xyz[:twins]))


def _run(pos1, pos2, boxes, rng, bins, excl, algo="cell"):
    edges = np.linspace(rng[0], rng[1], bins + 1)
    eng = _core.RdfEngine(edges, excl, algo=algo)
    eng.accumulate(pos1, pos2, boxes)
    got, st = eng.counts(), eng.stats()
    eng.close()
    return got, st


def _oracle(pos1, pos2, boxes, rng, bins, excl):
    want = np.zeros(bins, dtype=np.int64)
    for f in range(pos1.shape[0]):
        c_radial_histogram(pos1[f], pos1[f] if pos2 is None else pos2[f], bins, rng, boxes[f], exclusion=excl,
                           counts=want)
    want.setflags(write=False)
    return want


def _boxes(box, frames):
    return np.tile(np.asarray(box, dtype=np.float32), (frames, 1))


def expected_units(n):
    """Wave steps of ONE frame of n particles when every cull passes (the range covers the cluster): per i tile the
    33 rotated steps of half a, one a x b step per real row of a, the 33 rotated steps of half b if it holds a
    particle, and two steps (one per i half) for every real row of every j tile behind the diagonal.  The last j tile
    of an odd number of halves holds padding rows alone: its box is no box, the cull cannot drop it and cannot shift
    it, and it takes the 128 steps of the straddling loops (``general_units``), as it always did."""
    t64 = -(-n // 128) * 2
    real = [min(64, max(0, n - 64 * t)) for t in range(t64)]
    units = 0
    for i in range(t64 // 2):
        units += 33 + real[2 * i] + (33 if real[2 * i + 1] else 0) + 2 * sum(real[2 * i + 2:])
    return units + general_units(n)


def general_units(n):
    """Steps of one frame on the per-pair image path when the cluster is small against its box: 128 for every visit
    of a j tile of padding rows alone, which every i tile pays."""
    t64 = -(-n // 128) * 2
    return 128 * (t64 // 2) if n <= 64 * (t64 - 1) else 0


def test_expected_units_of_full_and_padded_tiles():
    assert (expected_units(128), general_units(128)) == (130, 0)
    assert (expected_units(256), general_units(256)) == (2 * 130 + 2 * 128, 0)
    assert (expected_units(64), general_units(64)) == (33 + 64 + 128, 128)
    assert (expected_units(129), general_units(129)) == (130 + 2 + 128 + 33 + 1 + 128, 256)


# ------------------------------------------------------------------------------------------------- the plans

@pytest.mark.parametrize("box, rng, bins", RANGES)
def test_small_cases_plan_to_the_cell_kernel(box, rng, bins):
    for excl in (None, (1, 1)):
        p = _core.RdfEngine.plan(np.linspace(rng[0], rng[1], bins + 1), excl, "cell", 128, None, box, 2)
        assert (p["family"], p["self"], p["gh"], p["lower"]) == (2, 1, 0, int(rng[0] > 0)), p
        assert p["skip"] == int(box == BOX60), p
    p = _core.RdfEngine.plan(np.linspace(0.0, 6.0, 5201), None, "cell", 128, None, BOX60, 1)
    assert (p["family"], p["gh"]) == (2, 1), p


# ------------------------------------------------------------------------------------------------- counts and ranges

@functools.lru_cache(maxsize=None)
def _cluster_frames(n):
    rng = np.random.default_rng(1800 + n)
    # three i tiles at 320: the cluster keeps its cross-section, so every i tile stays a slab of it
    pos = np.stack([_cluster(rng, n) for _ in range(2)])
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def _cluster_want(n, excl, case):
    box, rng, bins = RANGES[case]
    return _oracle(_cluster_frames(n), None, _boxes(box, 2), rng, bins, excl)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(RANGES)), ids=lambda k: f"L={RANGES[k][0][0]:g} range={RANGES[k][1]}")
@pytest.mark.parametrize("excl", (None, (1, 1)), ids=("no exclusion", "exclusion (1, 1)"))
@pytest.mark.parametrize("n", COUNTS)
def test_counts_equal_the_oracle(n, excl, case):
    box, rng, bins = RANGES[case]
    pos = _cluster_frames(n)
    want = _cluster_want(n, excl, case)
    assert want.sum() >= 500
    got, st = _run(pos, None, _boxes(box, 2), rng, bins, excl)
    np.testing.assert_array_equal(got, want)
    if rng[1] == 15.0:      # beyond the cluster's diameter: every cull passes, the steps are known
        assert st["pairs_computed"] == 2 * 64 * expected_units(n), (st, expected_units(n))
        assert st["cell_units_general"] == 2 * general_units(n), st
    else:                   # a x b rows culled against the other half's box
        assert 2 * 64 * (33 + general_units(n)) <= st["pairs_computed"] <= 2 * 64 * expected_units(n), st
        if n >= 127:
            assert st["pairs_computed"] < 2 * 64 * expected_units(n), st


@pytest.mark.gpu
def test_block_exclusion_compares_tags_in_the_rotated_steps():
    pos = _cluster_frames(192)
    for excl in ((3, 3), (64, 64)):
        want = _oracle(pos, None, _boxes(BOX60, 2), (0.0, 15.0), 75, excl)
        got, st = _run(pos, None, _boxes(BOX60, 2), (0.0, 15.0), 75, excl)
        np.testing.assert_array_equal(got, want)
        assert st["pairs_computed"] == 2 * 64 * expected_units(192), st


# ------------------------------------------------------------------------------------------------- the step statistic

@pytest.mark.gpu
@pytest.mark.parametrize("bins", (75, 201, 5200), ids=("75 bins", "201 bins", "5200 bins, global histogram"))
def test_one_full_tile_takes_130_steps(bins):
    """One frame of 128 particles, range beyond the tile, no exclusion: 33 + 64 + 33 steps — in the LDS forms and in
    the global form (more than 5 119 bins), whose rotated steps bin through the float position."""
    pos = _cluster_frames(128)[:1]
    want = _oracle(pos, None, _boxes(BOX60, 1), (0.0, 15.0), bins, None)
    got, st = _run(pos, None, _boxes(BOX60, 1), (0.0, 15.0), bins, None)
    np.testing.assert_array_equal(got, want)
    assert want.sum() == 128 * 128
    assert st["pairs_computed"] == 64 * 130, st


@pytest.mark.gpu
def test_the_global_form_lists_the_pairs_of_its_rotated_steps():
    """5 200 bins to 0.52: a bin is 10^-4 wide, so a tenth of the candidates is undecided in float32, but only some
    twenty pairs of the cluster are candidates at all — the 64 pairs (i, i) of a half's k = 0 step and the few others
    fit a wave's list, no visit is redone, and every (i, i) reaches bin 0 through the entry the rotated step of the
    global form lists it under."""
    pos = _cluster_frames(128)
    rng, bins = (0.0, 0.52), 5200
    p = _core.RdfEngine.plan(np.linspace(rng[0], rng[1], bins + 1), None, "cell", 128, None, BOX60, 2)
    assert (p["family"], p["gh"]) == (2, 1), p
    want = _oracle(pos, None, _boxes(BOX60, 2), rng, bins, None)
    assert want[0] == 2 * 128 and want.sum() < 2 * 128 + 120
    got, st = _run(pos, None, _boxes(BOX60, 2), rng, bins, None)
    np.testing.assert_array_equal(got, want)
    assert 2 * 128 <= st["pairs_exact"] <= 2 * 128 + 120, st


@functools.lru_cache(maxsize=None)
def _two_items():
    """66 j tiles (more than the 64 a chunk holds at least) in a cluster 4 across: with 64 tiles to a chunk the tiles
    of an i tile are dealt to two items by residue — its two diagonal visits run in different items — with 128 to
    one."""
    rng = np.random.default_rng(4224)
    pos = _cluster(rng, 4224, size=np.array([4.0, 4.0, 4.0]))[None]
    boxes = _boxes((100.0, 100.0, 100.0, 90.0, 90.0, 90.0), 1)
    return pos, boxes, _oracle(pos, None, boxes, (0.0, 8.0), 40, None)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_tiles, chunks", (("64", 2), ("128", 1)))
def test_diagonal_visits_in_one_item_and_in_two(monkeypatch, chunk_tiles, chunks):
    pos, boxes, want = _two_items()
    set_env(monkeypatch, {"MDX_RDF_CHUNK_TILES": chunk_tiles})
    p = _core.RdfEngine.plan(np.linspace(0.0, 8.0, 41), None, "cell", 4224, None, boxes[0], 1)
    assert p["family"] == 2 and -(-66 // p["chunk"]) == chunks, p
    got, st = _run(pos, None, boxes, (0.0, 8.0), 40, None)
    np.testing.assert_array_equal(got, want)
    assert want.sum() == 4224 * 4224
    # 33 i tiles: 130 steps on the diagonal and 128 for each of the 64 - 2 I tiles behind it
    assert expected_units(4224) == 33 * 130 + 128 * sum(64 - 2 * i for i in range(33))
    assert st["pairs_computed"] == 64 * expected_units(4224), st


# ------------------------------------------------------------------------------------------------- undecided pairs

EDGE_CASES = {
    # name: (n, lattice dims, twins, exclusion, range, bins, frames, particles on the lattice)
    # (a sixteenth of the lattice's pairs are on edges, not only those along an axis: wherever the squared distance in
    # lattice constants is a perfect square.  Without exclusion the k = 0 step alone lists 64 pairs, so only 40 of the
    # particles sit on the lattice there, the others anywhere in its volume: some 100 entries in visit 2 I, fewer than
    # the 128 a wave's list holds — the visit is not redone and every entry is the step's own)
    "sparse lattice and coincident, no exclusion": (128, (16, 16, 32), 6, None, (0.0, 6.0), 60, 32, 40),
    "lattice, exclusion (1, 1)": (128, (12, 12, 24), 0, (1, 1), (0.0, 6.0), 60, 32, 128),
    "lattice, range (2, 6)": (128, (8, 8, 24), 4, None, (2.0, 6.0), 40, 16, 128),
    "three halves, no exclusion": (192, (16, 16, 32), 6, None, (0.0, 6.0), 60, 16, 60),
    "two i tiles, exclusion (1, 1)": (256, (8, 8, 24), 0, (1, 1), (0.0, 6.0), 60, 8, 256),
}


@functools.lru_cache(maxsize=None)
def _edge_inputs(name):
    n, dims, twins, excl, rng, bins, frames, n_lat = EDGE_CASES[name]
    gen = np.random.default_rng(sum(map(ord, name)))
    size = 0.5 * (np.asarray(dims) - 1)
    pos = np.stack([gen.permutation(np.concatenate((_lattice_subset(gen, n_lat, dims, twins=twins),
                                                    _cluster(gen, n - n_lat, size=size, origin=(10.0, 10.0, 10.0)))))
                    for _ in range(frames)])
    boxes = _boxes(BOX60, frames)
    pos.setflags(write=False)
    return pos, boxes, _oracle(pos, None, boxes, rng, bins, excl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_CASES)
def test_pairs_on_bin_edges_and_at_distance_zero(name):
    """A random subset of a lattice whose constant is five bin widths: the pairs whose squared distance in lattice
    constants is a perfect square, those along an axis among them, sit exactly on bin edges — spread over the rotation
    steps and the a x b rows as the sort happens to order the tile — and are, like the pairs at distance 0 (every
    (i, i) without exclusion: the whole k = 0 step), undecided in float32 and listed for the exact arithmetic."""
    n, dims, twins, excl, rng, bins, frames, n_lat = EDGE_CASES[name]
    pos, boxes, want = _edge_inputs(name)
    got, st = _run(pos, None, boxes, rng, bins, excl)
    np.testing.assert_array_equal(got, want)
    assert st["pairs_exact"] >= frames * (n if excl is None and rng[0] == 0.0 else 8), st
    assert st["cell_units_general"] == frames * general_units(n), st


@functools.lru_cache(maxsize=None)
def _brick_inputs(excl):
    """8 x 8 x 8 particles on a lattice of constant 0.5, all on bin edges of (0, 6) / 60: every diagonal visit of its
    four i tiles lists more undecided pairs than a wave's list holds and is redone"""
    g = np.arange(8, dtype=np.float32) * np.float32(0.5)
    pos = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(4.0))[None]
    boxes = _boxes((30.0, 29.5, 31.0, 90.0, 90.0, 90.0), 1)
    return pos, boxes, _oracle(pos, None, boxes, (0.0, 6.0), 60, excl)


@pytest.mark.gpu
@pytest.mark.parametrize("excl", (None, (1, 1)), ids=("no exclusion", "exclusion (1, 1)"))
def test_a_brick_on_bin_edges_overflows_the_list_inside_a_diagonal_visit(excl):
    pos, boxes, want = _brick_inputs(excl)
    got, st = _run(pos, None, boxes, (0.0, 6.0), 60, excl)
    np.testing.assert_array_equal(got, want)
    # along the axes alone a particle has 21 neighbours on bin edges, and every such pair is listed at least once
    assert st["pairs_exact"] >= 512 * 21 // 2, st


# ------------------------------------------------------------------------------------------------- the old schedule

@pytest.mark.gpu
@pytest.mark.parametrize("box, cloud, general", (((24.0, 24.5, 25.0, 90.0, 90.0, 90.0), (0.36, 0.04, 0.04), False),
                                                 ((12.0, 12.5, 12.25, 90.0, 90.0, 90.0), (1.0, 1.0, 1.0), True)),
                         ids=("half extent 0.18 L", "tile across the box"))
def test_a_tile_too_large_for_its_box_keeps_the_old_schedule(box, cloud, general):
    """128 particles in a cloud 0.36 box lengths long and 0.04 thick (half extent 0.18 L: 3 hI is above 0.4999 L and
    the rule fails; reach 0.36 L below L / 2: the old row loops; range 0.45 L beyond the cloud's diameter, so every
    cull passes), and across the whole of a small box (the straddling loops): the old schedule's 256 steps."""
    rng = np.random.default_rng(int(box[0]))
    L = np.asarray(box[:3])
    pos = ((0.3 * L + rng.random((1, 128, 3)) * (np.asarray(cloud) * L)) if not general else rng.random((1, 128, 3)) * L)
    pos = pos.astype(np.float32)
    rng_r = (0.0, 0.45 * float(L.min()))
    want = _oracle(pos, None, _boxes(box, 1), rng_r, 50, None)
    got, st = _run(pos, None, _boxes(box, 1), rng_r, 50, None)
    np.testing.assert_array_equal(got, want)
    assert st["pairs_computed"] == 64 * 256, st
    assert st["cell_units_general"] == (256 if general else 0), st
    if not general:
        assert want.sum() == 128 * 128


@pytest.mark.gpu
def test_a_two_set_call_is_unchanged():
    rng = np.random.default_rng(7)
    pos1, pos2 = _cluster(rng, 128)[None], _cluster(rng, 192)[None]
    want = _oracle(pos1, pos2, _boxes(BOX60, 1), (0.0, 15.0), 75, None)
    got, st = _run(pos1, pos2, _boxes(BOX60, 1), (0.0, 15.0), 75, None)
    np.testing.assert_array_equal(got, want)
    assert want.sum() == 128 * 192
    # one i tile: two steps for every row of the second set, 128 for its fourth tile (padding rows alone)
    assert st["pairs_computed"] == 64 * (2 * 192 + 128) and st["cell_units_general"] == 128, st


@pytest.mark.gpu
def test_a_triclinic_self_call_is_unchanged():
    rng = np.random.default_rng(11)
    pos = (rng.random((1, 1024, 3)) * np.array([8.0, 8.0, 8.0]) + 6.0).astype(np.float32)
    p = _core.RdfEngine.plan(np.linspace(0.0, 6.0, 61), (1, 1), "auto", 1024, None, TRI, 1)
    assert p["family"] == 4, p
    want = _oracle(pos, None, _boxes(TRI, 1), (0.0, 6.0), 60, (1, 1))
    got, st = _run(pos, None, _boxes(TRI, 1), (0.0, 6.0), 60, (1, 1), algo="auto")
    np.testing.assert_array_equal(got, want)
    assert want.sum() >= 1000
