"""
The pair kernel's skipped steps (mdx_rdf_cell.hpp, cell_step<..., SKIP>): a wave step none of whose 64 pairs is a
candidate leaves behind the candidate test, and the mask of undecided lanes must then read zero.  Small systems at a
number density near 0.1 / A^3 with the range end near 0.2 L, so that the shifted row loops run with empty and
non-empty steps mixed; every case against the C oracle, count for count.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mdhelper_amd import _core  # noqa: E402
from oracle import rdf as orf  # noqa: E402
from oracle.cbind import c_radial_histogram  # noqa: E402

WIDTH = np.float32(0.75)      # bin width of the lattice cases = lattice spacing


def _cube(L):
    return np.array([L, L, L, 90, 90, 90], dtype=np.float32)


def _run(p1, p2, n_bins, rng_range, dims, exclusion):
    """Counts and statistics of the cell-sorted kernel on (a stack of) frames."""
    eng = _core.RdfEngine(np.linspace(rng_range[0], rng_range[1], n_bins + 1), exclusion, algo="cell", timing=True)
    eng.accumulate(p1, p2, dims)
    got, st = eng.counts(), eng.stats()
    eng.close()
    return got, st


def _want(p1, p2, n_bins, rng_range, dims, exclusion):
    p1, p2 = np.asarray(p1), np.asarray(p1 if p2 is None else p2)
    if p1.ndim == 2:
        p1, p2 = p1[None], p2[None]
    return sum(c_radial_histogram(a, b, n_bins, rng_range, dims, exclusion=exclusion) for a, b in zip(p1, p2))


def _assert_culled(st):
    # the culled path ran (rows were dropped: fewer distance evaluations than pairs; at a range end of 0.2 L and
    # 64-particle units 8.6 A across that is about half of them) ...
    assert 0 < st["pairs_computed"] < st["pairs_evaluated"], st
    # ... and the image-search share is below 1: some units went through the shifted row loops
    assert st["cell_units"] > 0 and st["cell_units_general"] < st["cell_units"], st


@pytest.fixture(scope="module")
def gas():
    """Three frames of 4 096 uniform particles at 0.1 / A^3 (L = 34.47), some of them unwrapped images."""
    rng = np.random.default_rng(2024)
    L = np.float32(34.47)
    frames = (rng.random((3, 4096, 3)) * L).astype(np.float32)
    frames[:, :200] += L * np.array([2, -1, 1], dtype=np.float32)
    frames.setflags(write=False)
    return frames, _cube(L)


@pytest.mark.parametrize("groups,exclusion", [("self", None), ("self", (1, 1)), ("two", None)])
def test_rdf_empty_steps_weights_tags_diagonal(gas, groups, exclusion):
    """Self without exclusion (weight 2 off the diagonal, weight 1 on it, no tags), self with exclusion (1, 1) (tags
    compared in the diagonal tiles), two groups (weight 1 everywhere)."""
    frames, dims = gas
    p1, p2 = (frames, None) if groups == "self" else (frames[:, :2560], frames[:, 2560:])
    got, st = _run(p1, p2, 201, (0.0, 6.9), dims, exclusion)
    np.testing.assert_array_equal(got, _want(p1, p2, 201, (0.0, 6.9), dims, exclusion))
    _assert_culled(st)


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_rdf_empty_steps_lower_bound(gas, exclusion):
    """range = (3, 6): the variants of the step that test the lower end of the range as well."""
    frames, dims = gas
    got, st = _run(frames[:2], None, 64, (3.0, 6.0), dims, exclusion)
    np.testing.assert_array_equal(got, _want(frames[:2], None, 64, (3.0, 6.0), dims, exclusion))
    _assert_culled(st)


@pytest.mark.parametrize("end", [10.3, 10.4])
def test_rdf_step_chosen_per_launch(gas, end):
    """The launch takes the skipping step up to a range end of 0.3 of the shortest box length (10.341 here) and the
    unconditional tail beyond (mdx_rdf.hip, CELL_SKIP_MAX_RANGE): one frame on either side of the threshold."""
    frames, dims = gas
    got, st = _run(frames[0], None, 103, (0.0, end), dims, (1, 1))
    np.testing.assert_array_equal(got, _want(frames[0], None, 103, (0.0, end), dims, (1, 1)))
    _assert_culled(st)


def _blocks_in_gas(n_blocks, side, n_gas, sites, seed):
    """`n_blocks` cubes of side^3 simple-cubic lattice points (spacing = bin width, so their separations sit exactly
    on bin edges: multiples of 0.75 are exact in float32) at distinct random sites of a coarse grid, in a box of
    `sites` lattice spacings that also holds `n_gas` uniform particles.  The gas and the other blocks give the rows
    that lie within reach of a tile's box and of none of its particles."""
    rng = np.random.default_rng(seed)
    L = np.float32(sites) * WIDTH
    coarse = sites // (side + 1)
    cells = rng.choice(coarse ** 3, n_blocks, replace=False)
    origin = np.stack(np.unravel_index(cells, (coarse,) * 3), -1) * (side + 1)
    idx = np.arange(side)
    block = np.stack(np.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3)
    lattice = ((origin[:, None, :] + block[None]).reshape(-1, 3) * WIDTH).astype(np.float32)
    pos = np.concatenate([lattice, (rng.random((n_gas, 3)) * L).astype(np.float32)])
    return pos[rng.permutation(len(pos))], _cube(L)


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_rdf_empty_steps_next_to_undecided_pairs(exclusion):
    """64 blocks of 2 x 2 x 2 lattice points in 1 536 gas particles (2 048 in all, L = 27.75, range end 5.25 =
    0.19 L).  A block has 12 pairs exactly one bin width apart; a 64-particle tile holds about two blocks, so a
    tile's undecided pairs fit the wave's list (128 entries, flushed at 64) and are appended by the step itself —
    between steps that were skipped.  A mask left over from an earlier step would append a pair twice."""
    pos, dims = _blocks_in_gas(64, 2, 1536, 37, seed=7)
    got, st = _run(pos, None, 7, (0.0, 5.25), dims, exclusion)
    np.testing.assert_array_equal(got, _want(pos, None, 7, (0.0, 5.25), dims, exclusion))
    _assert_culled(st)
    assert st["pairs_exact"] >= 64 * 12      # every on-edge pair went to the exact arithmetic


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_rdf_empty_steps_before_list_overflow(exclusion):
    """32 blocks of 4 x 4 x 4 lattice points in 2 048 gas particles (4 096 in all, L = 34.5, range end 6.75 =
    0.196 L).  One block alone has 144 nearest-neighbour pairs exactly one bin width apart, more than the wave's
    list of 128 holds, and its 64 points are adjacent in the sorted order: the tiles that hold it overflow the list,
    roll back and are redone by cell_slow_unit after steps that were skipped."""
    pos, dims = _blocks_in_gas(32, 4, 2048, 46, seed=8)
    got, st = _run(pos, None, 9, (0.0, 6.75), dims, exclusion)
    np.testing.assert_array_equal(got, _want(pos, None, 9, (0.0, 6.75), dims, exclusion))
    _assert_culled(st)
    assert st["pairs_exact"] >= 32 * 144


def test_rdf_every_step_empty():
    """Two groups farther apart than the range end, inside each other's tile reach: group one on eight spherical
    shells of radius 7.6, group two within 0.45 of the shells' centres (2 048 each, L = 34.5, range end 6.9).  No
    pair is closer than 7.15, yet the bounding boxes of the shell tiles reach the centres, so steps run and every
    one of them is skipped."""
    rng = np.random.default_rng(9)
    L = np.float32(34.5)
    centres = (np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * (L / 2)
    u = rng.normal(size=(8, 256, 3))
    shells = centres[:, None] + 7.6 * u / np.linalg.norm(u, axis=-1, keepdims=True)
    v = rng.normal(size=(8, 256, 3))
    cores = centres[:, None] + 0.45 * rng.random((8, 256, 1)) * v / np.linalg.norm(v, axis=-1, keepdims=True)
    p1, p2 = shells.reshape(-1, 3).astype(np.float32), cores.reshape(-1, 3).astype(np.float32)
    dims = _cube(L)
    want = _want(p1, p2, 100, (0.0, 6.9), dims, None)
    assert want.sum() == 0
    got, st = _run(p1, p2, 100, (0.0, 6.9), dims, None)
    np.testing.assert_array_equal(got, want)
    _assert_culled(st)
    assert st["pairs_exact"] == 0


def test_rdf_empty_steps_triclinic(monkeypatch):
    """One triclinic frame through the culled kernel (27 tile images; the same step)."""
    monkeypatch.delenv("MDX_RDF_TRI_BRUTE", raising=False)
    rng = np.random.default_rng(46)
    dims = np.array((33.0, 36.0, 39.0, 101.5, 90.0, 67.25), dtype=np.float32)
    B = orf.triclinic_vectors(dims).astype(np.float64)
    pos = (rng.random((4096, 3)) @ B + rng.normal(0, 30.0, (4096, 3))).astype(np.float32)
    for rng_range, nb, exclusion in [((0.0, 6.6), 120, (1, 1)), ((3.0, 6.0), 33, None)]:
        got, st = _run(pos, None, nb, rng_range, dims, exclusion)
        np.testing.assert_array_equal(got, _want(pos, None, nb, rng_range, dims, exclusion))
        _assert_culled(st)
