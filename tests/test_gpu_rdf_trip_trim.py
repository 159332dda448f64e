"""
What the pair kernel issues AROUND its step (mdx_rdf_cell.hpp): the six row loops of a tile visit and the append of an
undecided pair to the wave's list.  The row loops hand cell_step the pieces of a pair's indices (the item's i base and
the half; the tile's j base, the row of the turn and the row's offset in the turn) and the append puts them together
under EXEC = the mask of undecided lanes.  A wrong piece lists a pair under another pair's indices: the exact
arithmetic then bins a distance that is not on a bin edge, or drops the weight flag, and the counts differ from the
oracle's.  Every case is compared with the C oracle count for count; 2 048 - 4 096 particles, one to three frames.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mdhelper_amd import _core  # noqa: E402
from oracle import rdf as orf  # noqa: E402
from oracle.cbind import c_radial_histogram  # noqa: E402

WIDTH = np.float32(0.75)      # bin width of the lattice cases = lattice spacing (multiples are exact in float32)


def _cube(L):
    return np.array([L, L, L, 90, 90, 90], dtype=np.float32)


def _run(p1, p2, n_bins, rng_range, dims, exclusion):
    eng = _core.RdfEngine(np.linspace(rng_range[0], rng_range[1], n_bins + 1), exclusion, algo="cell", timing=True)
    eng.accumulate(p1, p2, dims)
    got, st = eng.counts(), eng.stats()
    eng.close()
    return got, st


def _want(p1, p2, n_bins, rng_range, dims, exclusion):
    p1, p2 = np.asarray(p1), np.asarray(p1 if p2 is None else p2)
    if p1.ndim == 2:
        p1, p2 = p1[None], p2[None]
    dims = np.broadcast_to(np.asarray(dims), (len(p1), 6))
    return sum(c_radial_histogram(a, b, n_bins, rng_range, d, exclusion=exclusion) for a, b, d in zip(p1, p2, dims))


def _assert_trips(st):
    """Trips were run, and not all of them by the image-search loop: the shifted row loops ran."""
    assert st["cell_units"] > 0 and st["cell_units_general"] < st["cell_units"], st
    assert 0 < st["pairs_computed"] < st["pairs_evaluated"], st


def _lattice_in_gas(n_shapes, shape, n_gas, sites, seed):
    """`n_shapes` bricks of shape[0] x shape[1] x shape[2] simple-cubic lattice points (spacing = bin width: their
    separations along the axes sit exactly on bin edges) at distinct random sites of a coarse grid, in a cubic box of
    `sites` lattice spacings that also holds `n_gas` uniform particles; shuffled, so that after the sort a brick's
    points land in any row of a j tile, even or odd, and in either half of an i tile."""
    rng = np.random.default_rng(seed)
    L = np.float32(sites) * WIDTH
    pitch = max(shape) + 1
    coarse = sites // pitch
    cells = rng.choice(coarse ** 3, n_shapes, replace=False)
    origin = np.stack(np.unravel_index(cells, (coarse,) * 3), -1) * pitch
    block = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    lattice = ((origin[:, None, :] + block[None]).reshape(-1, 3) * WIDTH).astype(np.float32)
    pos = np.concatenate([lattice, (rng.random((n_gas, 3)) * L).astype(np.float32)])
    pos = pos[rng.permutation(len(pos))]
    pos.setflags(write=False)
    return pos, _cube(L)


@pytest.fixture(scope="module")
def cubes():
    """64 bricks of 2 x 2 x 2 points (12 pairs one bin width apart each) in 1 536 gas particles: 2 048, L = 27.75."""
    return _lattice_in_gas(64, (2, 2, 2), 1536, 37, seed=11)


@pytest.fixture(scope="module")
def rods():
    """100 rods of 6 points along x (per rod two pairs 3.0 apart, one 3.75 apart: edges of range (3, 6) in bins of
    0.75) in 1 448 gas particles: 2 048, L = 27.75."""
    return _lattice_in_gas(100, (6, 1, 1), 1448, 37, seed=12)


@pytest.mark.parametrize("groups", ["self", "two"])
@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_append_indices(cubes, groups, exclusion):
    """Undecided pairs listed from every place of a turn.  Self: a brick inside one 64-particle tile is listed from a
    diagonal tile pair with weight 1 (and, with exclusion (1, 1), beside the tag comparison), a brick cut by a tile
    boundary from an off-diagonal pair with weight 2 — the flag in bit 31 of the j index.  Two groups: weight 1
    everywhere, two sorted copies.  The shuffled order puts a brick's points in even and odd rows (row r and r + 1
    of a paired turn) and in both i halves; a pair listed under a neighbouring row or the other half has another
    distance, which the exact arithmetic bins elsewhere or not at all."""
    pos, dims = cubes
    p1, p2 = (pos, None) if groups == "self" else (pos[:1024], pos[1024:])
    got, st = _run(p1, p2, 7, (0.0, 5.25), dims, exclusion)
    np.testing.assert_array_equal(got, _want(p1, p2, 7, (0.0, 5.25), dims, exclusion))
    _assert_trips(st)
    if groups == "self":
        assert st["pairs_exact"] >= 64 * 12      # every on-edge pair went through the list


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_append_indices_lower_bound(rods, exclusion):
    """range = (3, 6), the LOWER form of the step: the rods' pairs 3.0 apart sit on the lower end of the range (in or
    out by the exact arithmetic alone), those 3.75 apart on the first inner edge."""
    pos, dims = rods
    got, st = _run(pos, None, 4, (3.0, 6.0), dims, exclusion)
    np.testing.assert_array_equal(got, _want(pos, None, 4, (3.0, 6.0), dims, exclusion))
    _assert_trips(st)
    assert st["pairs_exact"] >= 100 * 3


@pytest.mark.parametrize("side", ["slab_is_j", "slab_is_i"])
def test_every_row_loop(side):
    """Rows that survive against both i halves, against one only, in adjacent pairs and alone.  Group one: 16 compact
    clusters of 128 particles (an i item; sorted, its two halves are the two ends of the cluster, 5 A apart).  Group
    two: a slab 1.2 A thick and 2 048 particles wide that passes the clusters at 4 - 9 A.  Of a slab tile's 64 rows
    those under a cluster reach both halves, those to either side one half, those farther out none; neighbours in
    the sorted order are neighbours in space, so the survivors come in runs (paired turns) with odd ends (single
    rows).  Either group on the i side."""
    rng = np.random.default_rng(13)
    L = np.float32(36.0)
    centres = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 2) * 9.0 + 4.5
    centres = np.concatenate([centres, np.full((16, 1), 12.0)], axis=1)
    clusters = centres[:, None] + rng.uniform(-1.0, 1.0, (16, 128, 3)) * np.array([3.5, 1.2, 1.2])
    slab = rng.random((2048, 3)) * np.array([L, L, 1.2]) + np.array([0.0, 0.0, 17.5])
    p1, p2 = clusters.reshape(-1, 3).astype(np.float32), slab.astype(np.float32)
    if side == "slab_is_i":
        p1, p2 = p2, p1
    dims = _cube(L)
    want = _want(p1, p2, 64, (0.0, 7.2), dims, None)
    assert want.sum() > 0
    got, st = _run(p1, p2, 64, (0.0, 7.2), dims, None)
    np.testing.assert_array_equal(got, want)
    _assert_trips(st)


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_list_overflow(exclusion):
    """32 bricks of 4 x 4 x 4 points in 2 048 gas particles (4 096, L = 34.5, range end 6.75).  One brick has 144
    nearest-neighbour pairs one bin width apart — more than the wave's list of 128 — and its points are adjacent in
    the sorted order: the visit overflows the list, rolls it back to its mark and is redone by cell_slow_unit, which
    must find the list as the append left it."""
    pos, dims = _lattice_in_gas(32, (4, 4, 4), 2048, 46, seed=14)
    got, st = _run(pos, None, 9, (0.0, 6.75), dims, exclusion)
    np.testing.assert_array_equal(got, _want(pos, None, 9, (0.0, 6.75), dims, exclusion))
    _assert_trips(st)
    assert st["pairs_exact"] >= 32 * 144


def test_visits_without_and_with_one_row():
    """Two groups out of range of each other, inside each other's tile reach: group one on eight spherical shells of
    radius 7.6, group two within 0.45 of the shells' centres (range end 6.9): visits whose rows all fall to the
    second cull or run only skipped steps.  Then eight particles of group two moved to 6.0 from a shell point each:
    visits with a single surviving row that holds a pair."""
    rng = np.random.default_rng(15)
    L = np.float32(34.5)
    centres = (np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * (L / 2)
    u = rng.normal(size=(8, 256, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    shells = centres[:, None] + 7.6 * u
    v = rng.normal(size=(8, 256, 3))
    cores = centres[:, None] + 0.45 * rng.random((8, 256, 1)) * v / np.linalg.norm(v, axis=-1, keepdims=True)
    p1 = shells.reshape(-1, 3).astype(np.float32)
    dims = _cube(L)
    p2 = cores.reshape(-1, 3).astype(np.float32)
    want = _want(p1, p2, 100, (0.0, 6.9), dims, None)
    assert want.sum() == 0
    got, st = _run(p1, p2, 100, (0.0, 6.9), dims, None)
    np.testing.assert_array_equal(got, want)
    assert st["cell_units"] > 0, st

    cores[:, 0] = centres + 1.6 * u[:, 0]      # 6.0 from shell point 0 of its own shell, along the radius
    p2 = cores.reshape(-1, 3).astype(np.float32)
    want = _want(p1, p2, 100, (0.0, 6.9), dims, None)
    assert want.sum() >= 8
    got, st = _run(p1, p2, 100, (0.0, 6.9), dims, None)
    np.testing.assert_array_equal(got, want)
    assert st["cell_units"] > 0, st


def test_unconditional_tail_beyond_skip_range(cubes):
    """Range end 9.0 = 0.324 L, beyond the launch's threshold for the skipping step (0.3 of the shortest box length):
    the instantiation with the unconditional tail, which shares the row loops and the append."""
    pos, dims = cubes
    got, st = _run(pos, None, 12, (0.0, 9.0), dims, (1, 1))
    np.testing.assert_array_equal(got, _want(pos, None, 12, (0.0, 9.0), dims, (1, 1)))
    _assert_trips(st)
    assert st["pairs_exact"] >= 64 * 12


def test_triclinic_frame(monkeypatch):
    """One triclinic frame (27 tile images, the four-wave instantiation): rods along the first cell vector, which is
    the x axis, in a gas; the rods' separations are multiples of the bin width up to the rounding of their origins."""
    monkeypatch.delenv("MDX_RDF_TRI_BRUTE", raising=False)
    rng = np.random.default_rng(16)
    dims = np.array((30.0, 33.0, 36.0, 101.5, 90.0, 67.25), dtype=np.float32)
    B = orf.triclinic_vectors(dims).astype(np.float64)
    origin = rng.random((100, 1, 3)) @ B
    rods = origin + np.arange(6)[None, :, None] * np.array([float(WIDTH), 0.0, 0.0])
    pos = np.concatenate([rods.reshape(-1, 3), rng.random((1448, 3)) @ B]).astype(np.float32)
    pos = pos[rng.permutation(len(pos))]
    for rng_range, nb, exclusion in [((0.0, 6.0), 8, (1, 1)), ((3.0, 6.0), 4, None)]:
        got, st = _run(pos, None, nb, rng_range, dims, exclusion)
        np.testing.assert_array_equal(got, _want(pos, None, nb, rng_range, dims, exclusion))
        assert st["cell_units"] > 0 and st["pairs_exact"] > 0, st


def test_several_slabs(cubes, rods, monkeypatch):
    """Three frames of 4 096 (the bricks and the rods together) in slabs of 400 000 bytes, two frames to a slab: the
    second slab is sorted by the small sort kernel in the block slots the pair kernel of the first leaves free."""
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", "400000")
    both = np.concatenate([cubes[0], rods[0]])
    frames = np.stack([both, both[::-1], np.roll(both, 1000, axis=0)])
    dims = np.tile(cubes[1], (3, 1))
    got, st = _run(frames, None, 7, (0.0, 5.25), dims, (1, 1))
    np.testing.assert_array_equal(got, _want(frames, None, 7, (0.0, 5.25), dims, (1, 1)))
    _assert_trips(st)
    assert st["slabs_sorted_beside"] >= 1, st
