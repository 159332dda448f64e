"""
The pair kernel's item machinery (mdx_rdf_cell.hpp): every WAVE of a block pulls its own (frame, i tile) items from
the XCD's counter, loads the frame's constants from the table rdf_cell_frame_geo_kernel wrote in front of the launch,
culls the candidate j tiles into its own quarter of the queue, 256 candidates to a round, and walks that queue alone;
the block's 32-bit LDS bins are moved out by whichever wave's announcement crosses the flush threshold, with
exchanges, while the other waves go on adding.  A wave that decodes an item wrongly, reads another frame's constants,
loses or repeats a queue entry at a round's seam or drops an add around an exchange changes a count: every case is
compared with the C oracle count for count.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mdhelper_amd import _core  # noqa: E402
from oracle import rdf as orf  # noqa: E402
from oracle.cbind import c_radial_histogram  # noqa: E402

WIDTH = np.float32(0.75)      # bin width of the lattice case = lattice spacing (multiples are exact in float32)
N_BINS, RANGE = 64, (0.0, 8.0)


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


@pytest.fixture(scope="module")
def gas():
    """Nine frames of 3 072 uniform particles in boxes of 31 - 35 A, a box per frame: a wave that reads another
    frame's constants wraps with the wrong box length."""
    rng = np.random.default_rng(21)
    L = np.linspace(31.0, 35.0, 9).astype(np.float32)
    pos = (rng.random((9, 3072, 3)) * L[:, None, None]).astype(np.float32)
    dims = np.stack([_cube(x) for x in L])
    pos.setflags(write=False)
    return pos, dims


@pytest.fixture(scope="module")
def gas_self(gas):
    """The oracle's counts of every frame of `gas` on its own, without exclusion."""
    pos, dims = gas
    want = np.stack([_want(pos[f], None, N_BINS, RANGE, dims[f], None) for f in range(len(pos))])
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("exclusion", [None, (1, 1)])
def test_self(gas, gas_self, exclusion):
    """Three frames, 24 items each, dealt to the waves one by one (fewer than eight frames: the `spread` mapping)."""
    pos, dims = gas
    want = _want(pos[:3], None, N_BINS, RANGE, dims[:3], exclusion) if exclusion else gas_self[:3].sum(axis=0)
    got, st = _run(pos[:3], None, N_BINS, RANGE, dims[:3], exclusion)
    np.testing.assert_array_equal(got, want)
    assert st["cell_units"] > 0 and st["pairs_computed"] < st["pairs_evaluated"], st


def test_two_groups(gas):
    """Two sorted copies, 1 024 against 2 048 particles, weight 1 everywhere, every item starts at j tile 0."""
    pos, dims = gas
    p1, p2 = pos[:2, :1024], pos[:2, 1024:]
    got, _ = _run(p1, p2, N_BINS, RANGE, dims[:2], None)
    np.testing.assert_array_equal(got, _want(p1, p2, N_BINS, RANGE, dims[:2], None))


@pytest.mark.parametrize("n_i", [128, 200])
def test_few_items(gas, n_i):
    """One or two items per frame (the second half empty but for 72 particles): most waves of every block find the
    counter exhausted at their first look and go straight to the closing barrier."""
    pos, dims = gas
    p1, p2 = pos[:2, :n_i], pos[:2, 512:2560]
    got, _ = _run(p1, p2, N_BINS, RANGE, dims[:2], None)
    np.testing.assert_array_equal(got, _want(p1, p2, N_BINS, RANGE, dims[:2], None))


@pytest.mark.parametrize("n_frames", [1, 7, 8, 9])
def test_frames_to_xcds(gas, gas_self, n_frames):
    """One and seven frames: items dealt to the XCDs one by one; eight: a frame per XCD; nine: XCD 0 has two frames
    and the others one (uneven residues).  The frames' boxes differ."""
    pos, dims = gas
    got, _ = _run(pos[:n_frames], None, N_BINS, RANGE, dims[:n_frames], None)
    np.testing.assert_array_equal(got, gas_self[:n_frames].sum(axis=0))


@pytest.fixture(scope="module")
def many_tiles():
    """256 particles against 20 480 in a box of 60 A: 320 candidate j tiles per item, two rounds of a wave's queue
    (256 and 64 candidates)."""
    rng = np.random.default_rng(22)
    L = np.float32(60.0)
    p1 = (rng.random((256, 3)) * L).astype(np.float32)
    p2 = (rng.random((20480, 3)) * L).astype(np.float32)
    return p1, p2, _cube(L)


@pytest.fixture(scope="module")
def many_tiles_want(many_tiles):
    p1, p2, dims = many_tiles
    return {r: _want(p1, p2, 60, (0.0, r), dims, None) for r in (6.0, 30.0)}


@pytest.mark.parametrize("chunk_tiles", ["100000", "64", None])
@pytest.mark.parametrize("r_max", [6.0, 30.0])
def test_rounds_of_the_queue(many_tiles, many_tiles_want, r_max, chunk_tiles, monkeypatch):
    """MDX_RDF_CHUNK_TILES beyond the tile count: an item is a whole i tile, two rounds of its wave's queue.  Range
    end 6 A: a few tiles of either round survive the cull; L / 2: all 320 do, the first round fills the queue to
    its last entry.  64: five items to an i tile (every fifth tile each), one cull pass each.  Unset: the host's
    choice (chunks of 128 and of 64 tiles: three and five items)."""
    if chunk_tiles is None:
        monkeypatch.delenv("MDX_RDF_CHUNK_TILES", raising=False)
    else:
        monkeypatch.setenv("MDX_RDF_CHUNK_TILES", chunk_tiles)
    p1, p2, dims = many_tiles
    got, st = _run(p1, p2, 60, (0.0, r_max), dims, None)
    np.testing.assert_array_equal(got, many_tiles_want[r_max])
    if r_max == 30.0:
        assert st["cell_units"] >= 2 * 2 * 320 * 64, st      # every (half, row) of every tile pair


@pytest.mark.parametrize("chunk_tiles", ["64", "128", None])
def test_chunks_of_a_self_histogram(chunk_tiles, monkeypatch):
    """8 192 particles, 128 j tiles, exclusion (1, 1): with chunks of 64 an i tile I is two items, the tiles 2 I,
    2 I + 2, ... and 2 I + 1, 2 I + 3, ... — a diagonal tile in each; with chunks of 128 it is one item; the host's
    choice is two as well (a quarter of the 128 tiles rounds up to 64)."""
    if chunk_tiles is None:
        monkeypatch.delenv("MDX_RDF_CHUNK_TILES", raising=False)
    else:
        monkeypatch.setenv("MDX_RDF_CHUNK_TILES", chunk_tiles)
    rng = np.random.default_rng(25)
    L = np.float32(44.0)
    pos = (rng.random((2, 8192, 3)) * L).astype(np.float32)
    got, _ = _run(pos, None, N_BINS, RANGE, _cube(L), (1, 1))
    np.testing.assert_array_equal(got, _want(pos, None, N_BINS, RANGE, _cube(L), (1, 1)))


def test_exchange_flush_beside_adds(gas, gas_self, monkeypatch):
    """MDX_RDF_LDS_FLUSH_UNITS = 1 and 3: a wave moves the bins out at every round (every few rounds) while the other
    waves of its block add.  1 024 copies of one frame are 24 576 items, several to every wave of the grid; the
    result is the unflushed one and 1 024 times the oracle's."""
    pos, dims = gas
    frames = np.ascontiguousarray(np.broadcast_to(pos[0], (1024,) + pos[0].shape))
    boxes = np.ascontiguousarray(np.broadcast_to(dims[0], (1024, 6)))
    monkeypatch.delenv("MDX_RDF_LDS_FLUSH_UNITS", raising=False)
    plain, _ = _run(frames, None, N_BINS, RANGE, boxes, None)
    np.testing.assert_array_equal(plain, 1024 * gas_self[0])
    for units in ("1", "3"):
        monkeypatch.setenv("MDX_RDF_LDS_FLUSH_UNITS", units)
        got, _ = _run(frames, None, N_BINS, RANGE, boxes, None)
        np.testing.assert_array_equal(got, plain)


def _lattice_in_gas(n_shapes, shape, n_gas, sites, seed):
    """`n_shapes` bricks of simple-cubic lattice points (spacing = bin width: their separations along the axes sit
    exactly on bin edges) at distinct random sites of a coarse grid, in a cubic box of `sites` lattice spacings that
    also holds `n_gas` uniform particles; shuffled (the construction of test_gpu_rdf_trip_trim.py)."""
    rng = np.random.default_rng(seed)
    L = np.float32(sites) * WIDTH
    pitch = max(shape) + 1
    coarse = sites // pitch
    cells = rng.choice(coarse ** 3, n_shapes, replace=False)
    origin = np.stack(np.unravel_index(cells, (coarse,) * 3), -1) * pitch
    block = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    lattice = ((origin[:, None, :] + block[None]).reshape(-1, 3) * WIDTH).astype(np.float32)
    pos = np.concatenate([lattice, (rng.random((n_gas, 3)) * L).astype(np.float32)])
    return pos[rng.permutation(len(pos))], _cube(L)


@pytest.fixture(scope="module")
def bricks():
    """32 bricks of 4 x 4 x 4 points (144 pairs one bin width apart each: more than a wave's list of 128) in 2 048
    gas particles: 4 096, L = 34.5."""
    return _lattice_in_gas(32, (4, 4, 4), 2048, 46, seed=23)


def test_list_overflow_in_a_wave_owned_item(bricks):
    """The visit that overflows the list rolls it back to its mark and is redone by cell_slow_unit, inside an item
    the wave runs alone: the redo reads the wave's own s_geo and slab."""
    pos, dims = bricks
    got, st = _run(pos, None, 9, (0.0, 6.75), dims, (1, 1))
    np.testing.assert_array_equal(got, _want(pos, None, 9, (0.0, 6.75), dims, (1, 1)))
    assert st["pairs_exact"] >= 32 * 144, st


def test_triclinic_frame(monkeypatch):
    """One triclinic frame: the table carries the cell matrix, the wave's queue the image masks."""
    monkeypatch.delenv("MDX_RDF_TRI_BRUTE", raising=False)
    rng = np.random.default_rng(24)
    dims = np.array((30.0, 33.0, 36.0, 101.5, 90.0, 67.25), dtype=np.float32)
    B = orf.triclinic_vectors(dims).astype(np.float64)
    pos = (rng.random((2048, 3)) @ B).astype(np.float32)
    got, st = _run(pos, None, 8, (0.0, 6.0), dims, (1, 1))
    np.testing.assert_array_equal(got, _want(pos, None, 8, (0.0, 6.0), dims, (1, 1)))
    assert st["cell_units"] > 0, st


def test_two_slabs(gas, gas_self, monkeypatch):
    """Three frames of 3 072 in slabs of two frames (the host keeps 33 bytes per padded particle and frame: the hook
    is sized from that), so the call is a slab of two frames and one of one: the table is written anew in front of
    the second slab's launch, for that slab's frame and box — the three boxes differ (32.5, 33.0 and 33.5 A), so a
    table row left from the first slab wraps the third frame with the wrong box length.  That the call did split
    shows in the statistics: the second slab was sorted beside the first one's pair launch, and each slab's pair
    launches are one bracket of the timer."""
    pos, dims = gas
    n_pad = -(-pos.shape[1] // 128) * 128
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", str(2 * 33 * n_pad))
    assert len({float(d[0]) for d in dims[3:6]}) == 3
    got, st = _run(pos[3:6], None, N_BINS, RANGE, dims[3:6], None)
    np.testing.assert_array_equal(got, gas_self[3:6].sum(axis=0))
    assert st["slabs_sorted_beside"] == 1 and st["launches"] == 2, st


def test_calls_and_reset(gas, gas_self):
    """Two calls on one engine add up (the table and the counters are the handle's and are rewritten per launch);
    after reset() a call stands alone, and so does the call after the next reset()."""
    pos, dims = gas
    eng = _core.RdfEngine(np.linspace(RANGE[0], RANGE[1], N_BINS + 1), None, algo="cell")
    eng.accumulate(pos[:2], None, dims[:2])
    eng.accumulate(pos[6:9], None, dims[6:9])
    np.testing.assert_array_equal(eng.counts(), gas_self[:2].sum(axis=0) + gas_self[6:9].sum(axis=0))
    eng.reset()
    eng.accumulate(pos[4], None, dims[4])
    np.testing.assert_array_equal(eng.counts(), gas_self[4])
    eng.reset()
    eng.accumulate(pos[5:7], None, dims[5:7])
    np.testing.assert_array_equal(eng.counts(), gas_self[5:7].sum(axis=0))
    eng.close()
