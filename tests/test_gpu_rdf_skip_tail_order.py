"""
The tail of the pair kernel's skipping step (``mdx_rdf_cell.hpp``, ``MDX_CELL_SKIP_TAIL``) forms the histogram address
of EVERY candidate lane and narrows EXEC to the sure lanes behind it: the undecided test must read the fixed-point
position before the address overwrites it, an undecided lane's address must never be added to, and such a pair must
still reach the exact arithmetic once.  Every case is a call whose counts must EQUAL those of
``oracle.cbind.c_radial_histogram``.

Shapes: clusters of one half (64), one half and one particle (65), one full tile, three halves and two and a half
tiles, a few Å across in a box wide enough for the every-pair-once rule of the diagonal — the a x b rows of a tile and
the tile pairs behind the diagonal run the skipping step, the rotated steps beside them the unconditional tail;
without exclusion, with exclusion (1, 1) and (4, 4); a range from 0 and one from r0 > 0 (the second candidate test),
both beyond the cluster's diameter, so that every cull passes and the number of wave steps is known exactly; 201 bins
(per-wave LDS histograms, the form the tail belongs to) and 5 200 (the global form, which must not change).  Subsets
of a lattice on bin edges put undecided pairs into the skipping steps of the a x b rows and of the tile pairs behind
the diagonal, and into the rotated steps; a brick of such pairs overflows the wave's list, which is rolled back and
redone; a tile too wide for its box, a two-set call and a triclinic frame take the other loops.
"""
import functools

import numpy as np
import pytest

from mdhelper_amd import _core
from oracle.cbind import c_radial_histogram

BOX60 = (60.0, 61.0, 62.0, 90.0, 90.0, 90.0)
TRI = (31.0, 28.5, 35.25, 75.0, 80.0, 110.0)
CLUSTER = np.array([5.0, 5.0, 12.0])          # diameter 13.9; half extents below a sixth of the box
COUNTS = (64, 65, 128, 192, 320)
EXCLUSIONS = (None, (1, 1), (4, 4))
RANGES = ((0.0, 15.0), (1.5, 15.0))
BINS = (201, 5200)


def _cluster(rng, n, size=CLUSTER, origin=(10.0, 11.0, 12.0)):
    return (np.asarray(origin) + rng.random((n, 3)) * size).astype(np.float32)


def _boxes(box, frames):
    return np.tile(np.asarray(box, dtype=np.float32), (frames, 1))


def _run(pos1, pos2, boxes, rng, bins, excl, algo="cell"):
    eng = _core.RdfEngine(np.linspace(rng[0], rng[1], bins + 1), excl, algo=algo)
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


def general_units(n):
    """Steps of one frame on the per-pair image path: 128 for every visit of a j tile of padding rows alone (its box
    is no box, the cull can neither drop nor shift it), which every i tile pays."""
    t64 = -(-n // 128) * 2
    return 128 * (t64 // 2) if n <= 64 * (t64 - 1) else 0


def expected_units(n):
    """Wave steps of one frame of n particles when every cull passes: per i tile the 33 rotated steps of half a, one
    a x b step per real row of a, the 33 rotated steps of half b if it holds a particle, and two steps for every real
    row of every j tile behind the diagonal; then the padding tile's steps."""
    t64 = -(-n // 128) * 2
    real = [min(64, max(0, n - 64 * t)) for t in range(t64)]
    units = 0
    for i in range(t64 // 2):
        units += 33 + real[2 * i] + (33 if real[2 * i + 1] else 0) + 2 * sum(real[2 * i + 2:])
    return units + general_units(n)


def test_expected_units():
    assert expected_units(128) == 130
    assert expected_units(64) == 33 + 64 + 128
    assert expected_units(65) == 33 + 64 + 33
    assert expected_units(192) == 130 + 2 * 64 + 33 + 64 + 2 * 128


# ------------------------------------------------------------------------------------------------- counts and steps

@functools.lru_cache(maxsize=None)
def _cluster_frames(n):
    rng = np.random.default_rng(1900 + n)
    pos = np.stack([_cluster(rng, n) for _ in range(2)])
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def _cluster_want(n, excl, rng, bins):
    return _oracle(_cluster_frames(n), None, _boxes(BOX60, 2), rng, bins, excl)


@pytest.mark.gpu
@pytest.mark.parametrize("bins", BINS, ids=("201 bins", "5200 bins, global histogram"))
@pytest.mark.parametrize("rng", RANGES, ids=("range (0, 15)", "range (1.5, 15)"))
@pytest.mark.parametrize("excl", EXCLUSIONS, ids=("no exclusion", "exclusion (1, 1)", "exclusion (4, 4)"))
@pytest.mark.parametrize("n", COUNTS)
def test_counts_and_steps_of_a_cluster(n, excl, rng, bins):
    p = _core.RdfEngine.plan(np.linspace(rng[0], rng[1], bins + 1), excl, "cell", n, None, BOX60, 2)
    assert (p["family"], p["self"], p["gh"], p["lower"]) == (2, 1, int(bins > 5119), int(rng[0] > 0)), p
    assert p["skip"] == 1, p        # the range ends below 0.3 L (the global form ignores the flag)
    want = _cluster_want(n, excl, rng, bins)
    assert want.sum() >= 2 * n * (n - 8) * 0.9
    got, st = _run(_cluster_frames(n), None, _boxes(BOX60, 2), rng, bins, excl)
    np.testing.assert_array_equal(got, want)
    # the range covers the cluster: every cull passes
    assert st["pairs_computed"] == 2 * 64 * expected_units(n), (st, expected_units(n))
    assert st["cell_units_general"] == 2 * general_units(n), st


# ------------------------------------------------------------------------------------------------- undecided pairs

def _lattice_subset(rng, n, dims, origin=(10.0, 10.0, 10.0), twins=0):
    """n distinct sites of a lattice of constant 0.5 = five bin widths of (0, 6) / 60: coordinates and differences are
    exact, and a pair whose squared distance in lattice constants is a perfect square sits exactly on a bin edge; the
    last `twins` particles lie exactly on the first `twins`."""
    pick = rng.choice(dims[0] * dims[1] * dims[2], n - twins, replace=False)
    xyz = np.stack(np.unravel_index(pick, dims), axis=-1).astype(np.float32) * np.float32(0.5)
    xyz += np.asarray(origin, dtype=np.float32)
    return np.concatenate((xyz, xyz[:twins]))


EDGE_CASES = {
    # name: (n, lattice dims, twins, exclusion, range, bins, frames, particles on the lattice)
    # Part of the particles on the lattice, the others anywhere in its volume: without exclusion the k = 0 step of a
    # half alone lists 64 pairs, and a visit that lists more than the 128 a wave's list holds is redone through
    # another path.  From 128 particles on, the a x b rows are skipping steps; from 192 on, so are tile pairs behind
    # the diagonal.
    "one half, no exclusion": (64, (12, 12, 24), 4, None, (0.0, 6.0), 60, 32, 40),
    "one half, exclusion (1, 1)": (64, (8, 8, 16), 0, (1, 1), (0.0, 6.0), 60, 32, 40),
    "one half, exclusion (4, 4)": (64, (8, 8, 16), 2, (4, 4), (0.0, 6.0), 60, 32, 40),
    "one half, range (2, 6)": (64, (8, 8, 16), 4, None, (2.0, 6.0), 40, 16, 40),
    "one half, global histogram": (64, (12, 12, 24), 0, (1, 1), (0.0, 6.0), 6000, 16, 40),
    "a full tile, exclusion (1, 1)": (128, (12, 12, 24), 0, (1, 1), (0.0, 6.0), 60, 16, 80),
    "a full tile, range (2, 6)": (128, (12, 12, 24), 4, None, (2.0, 6.0), 40, 16, 80),
    "three halves, no exclusion": (192, (16, 16, 32), 6, None, (0.0, 6.0), 60, 16, 60),
    "three halves, exclusion (1, 1)": (192, (12, 12, 24), 0, (1, 1), (0.0, 6.0), 60, 16, 120),
    "two i tiles, exclusion (4, 4)": (256, (12, 12, 24), 0, (4, 4), (0.0, 6.0), 60, 8, 160),
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
def test_pairs_on_bin_edges_are_binned_once_by_the_exact_arithmetic(name):
    n, dims, twins, excl, rng, bins, frames, n_lat = EDGE_CASES[name]
    pos, boxes, want = _edge_inputs(name)
    got, st = _run(pos, None, boxes, rng, bins, excl)
    p = _core.RdfEngine.plan(np.linspace(rng[0], rng[1], bins + 1), excl, "cell", n, None, BOX60, frames)
    assert (p["family"], p["skip"], p["gh"]) == (2, 1, int(bins > 5119)), p    # (the global form ignores the skip)
    np.testing.assert_array_equal(got, want)
    assert st["pairs_exact"] >= frames * (n if excl is None and rng[0] == 0.0 else 4), st
    assert st["cell_units_general"] == frames * general_units(n), st


@pytest.mark.gpu
@pytest.mark.parametrize("excl", (None, (1, 1)), ids=("no exclusion", "exclusion (1, 1)"))
def test_a_brick_on_bin_edges_is_rolled_back_and_redone(excl):
    """8 x 8 x 8 particles on a lattice of constant 0.5, all on bin edges of (0, 6) / 60: the visits of its four i
    tiles list more undecided pairs than a wave's list holds."""
    g = np.arange(8, dtype=np.float32) * np.float32(0.5)
    pos = (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(4.0))[None]
    boxes = _boxes((30.0, 29.5, 31.0, 90.0, 90.0, 90.0), 1)
    want = _oracle(pos, None, boxes, (0.0, 6.0), 60, excl)
    got, st = _run(pos, None, boxes, (0.0, 6.0), 60, excl)
    np.testing.assert_array_equal(got, want)
    assert st["pairs_exact"] >= 512 * 21 // 2, st


# ------------------------------------------------------------------------------------------------- the old schedule

@pytest.mark.gpu
def test_a_tile_too_wide_for_its_box_keeps_the_old_diagonal():
    """128 particles in a cloud 0.36 box lengths long (half extent 0.18 L: the rule fails) and 0.04 thick, range
    0.45 L beyond its diameter: the old diagonal's 256 steps on the row loops."""
    box = (24.0, 24.5, 25.0, 90.0, 90.0, 90.0)
    L = np.asarray(box[:3])
    pos = (0.3 * L + np.random.default_rng(24).random((1, 128, 3)) * (np.array([0.36, 0.04, 0.04]) * L)).astype(np.float32)
    rng = (0.0, 0.45 * float(L.min()))
    want = _oracle(pos, None, _boxes(box, 1), rng, 50, None)
    got, st = _run(pos, None, _boxes(box, 1), rng, 50, None)
    np.testing.assert_array_equal(got, want)
    assert want.sum() == 128 * 128
    assert st["pairs_computed"] == 64 * 256 and st["cell_units_general"] == 0, st


@pytest.mark.gpu
def test_a_two_set_call():
    rng = np.random.default_rng(19)
    pos1, pos2 = _cluster(rng, 128)[None], _cluster(rng, 192)[None]
    want = _oracle(pos1, pos2, _boxes(BOX60, 1), (0.0, 15.0), 201, None)
    got, st = _run(pos1, pos2, _boxes(BOX60, 1), (0.0, 15.0), 201, None)
    np.testing.assert_array_equal(got, want)
    assert want.sum() == 128 * 192
    assert st["pairs_computed"] == 64 * (2 * 192 + 128) and st["cell_units_general"] == 128, st


@pytest.mark.gpu
def test_a_triclinic_frame():
    rng = np.random.default_rng(23)
    pos = (rng.random((1, 1024, 3)) * np.array([8.0, 8.0, 8.0]) + 6.0).astype(np.float32)
    p = _core.RdfEngine.plan(np.linspace(0.0, 6.0, 61), (1, 1), "auto", 1024, None, TRI, 1)
    assert p["family"] == 4, p
    want = _oracle(pos, None, _boxes(TRI, 1), (0.0, 6.0), 60, (1, 1))
    got, _ = _run(pos, None, _boxes(TRI, 1), (0.0, 6.0), 60, (1, 1), algo="auto")
    np.testing.assert_array_equal(got, want)
    assert want.sum() >= 1000
