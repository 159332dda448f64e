"""
VanHove / VanHoveEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_vanhove_device.hpp): per point, lag and frame f >= lag

    x = (double)r + image * L;  d = x(f) - x(f - lag) (+0.0 for a dropped component);
    r2 = (dx*dx + dy*dy) + dz*dz;  r = sqrt(r2);  counts += numpy.histogram(r);  m2 += r2;  m4 += r2*r2

with the image counts of the reference's global unwrap restated frame by frame (the first frame is its own start).

No tolerance anywhere.  The restatement does one float64 operation at a time, as the device does (the unit is built
with contraction off; sqrt is correctly rounded on both sides); the accumulator of every point receives its terms in
frame order from a Python loop over the frames, and a group's moments add the accumulators of its points in row
order from a Python loop over the points.  The same operations in the same order give the same bits, so counts AND
moments are compared with ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import VanHove, calculate_non_gaussian_parameter

pytestmark = pytest.mark.gpu

T = _core.VanHoveEngine.TILE
LAGS = [0, 1, 2, 5, 36, 40]           # lag 40 never has an origin in 37 frames
EDGES = np.linspace(0.0, 15.0, 202)


# ---------------------------------------------------------------- restatement

def images_ref(pos, dims):
    """The reference's rule frame by frame: d = x - x_prev; |d| >= dims / 2 moves the image count by -sign(d);
    the first frame is its own start.  float32[F, n, 3] -> int[F, n, 3]."""
    x = np.asarray(pos).astype(np.float64)
    dims = np.asarray(dims, dtype=np.float64)
    images = np.zeros(x.shape[1:], dtype=int)
    out = np.zeros(x.shape, dtype=int)
    for f in range(1, len(x)):
        d = x[f] - x[f - 1]
        crossed = np.abs(d) >= dims / 2
        images[crossed] -= np.sign(d[crossed]).astype(int)
        out[f] = images
    return out


def restate(pos, sizes, edges, lags, *, dims=None, zero_dims=0):
    """(counts int64 [K, G, n_bins], moments [K, G, 2], point accumulators [K, n, 2], evaluations)."""
    x = np.asarray(pos).astype(np.float64)
    if dims is not None:
        x = x + images_ref(pos, dims).astype(np.float64) * np.asarray(dims, dtype=np.float64)
    F, n = x.shape[:2]
    n_bins = len(edges) - 1
    acc = np.zeros((len(lags), n, 2))
    counts = np.zeros((len(lags), len(sizes), n_bins), dtype=np.int64)
    evaluations = 0
    for k, lag in enumerate(lags):
        rs = []
        for f in range(lag, F):                                 # the accumulators take their terms in frame order
            d = x[f] - x[f - lag]
            for c in range(3):
                if zero_dims >> c & 1:
                    d[:, c] = 0.0
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            rs.append(np.sqrt(r2))
            acc[k, :, 0] = acc[k, :, 0] + r2
            acc[k, :, 1] = acc[k, :, 1] + r2 * r2
            evaluations += n
        lo = 0
        for g, size in enumerate(sizes):
            if rs:
                counts[k, g] = np.histogram(np.array(rs)[:, lo:lo + size], n_bins, (edges[0], edges[-1]))[0]
            lo += size
    moments = np.zeros((len(lags), len(sizes), 2))
    lo = 0
    for g, size in enumerate(sizes):
        s = np.zeros((len(lags), 2))
        for p in range(lo, lo + size):                          # a group's points in row order
            s = s + acc[:, p, :]
        moments[:, g] = s
        lo += size
    return counts, moments, acc, evaluations


def engine_run(pos, sizes, edges, lags, *, splits=None, setup=None, zero_dims=0):
    eng = _core.VanHoveEngine(sizes, edges, lags, zero_dims=zero_dims)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        counts, moments = eng.result()
        return counts, moments, eng.point_moments(), eng.stats()
    finally:
        eng.close()


def assert_same(got, want):
    """got: engine_run's tuple; want: restate's."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[3]["evaluations"] == want[3]
    assert got[0].dtype == np.int64


def diffusing(seed, F, n, step=1.2):
    """A free random walk, float32[F, n, 3]: displacements from 0 to beyond 15 at the long lags."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 40.0, (1, n, 3)) + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)).astype(np.float32)


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3}))
def test_engine_group_sizes_and_frame_counts(n):
    for F in (1, 2, 37):
        pos = diffusing(100 + n, F, n)
        want = restate(pos, [n], EDGES, LAGS)
        got = engine_run(pos, [n], EDGES, LAGS)
        assert_same(got, want)
        assert got[3]["frames"] == F
        assert want[3] == n * sum(max(F - lag, 0) for lag in LAGS)
        assert not got[0][5].any() and not got[1][5].any()          # lag 40: no origin
        if F == 37:
            inside = got[0].sum(axis=-1)[:, 0]
            assert inside[0] == n * 37 and inside[4] <= n           # lag 0: all in the bin of 0
            assert 0 < inside[3] <= n * 32
            assert np.all(got[1][1:5] > 0)


def test_engine_three_unequal_groups():
    sizes = [1, 65, T + 1]
    n, F = sum(sizes), 37
    pos = diffusing(7, F, n)
    got = engine_run(pos, sizes, EDGES, LAGS)
    assert_same(got, restate(pos, sizes, EDGES, LAGS))
    # the rows of a group do not depend on what the other groups are: the tiles never span two groups
    for g, (lo, hi) in enumerate(((0, 1), (1, 66), (66, n))):
        solo = engine_run(pos[:, lo:hi], [hi - lo], EDGES, LAGS)
        np.testing.assert_array_equal(solo[0][:, 0], got[0][:, g])
        np.testing.assert_array_equal(solo[1][:, 0], got[1][:, g])
        np.testing.assert_array_equal(solo[2], got[2][:, lo:hi])
    # an empty group between them: zero rows, the others unchanged
    wide = engine_run(pos, [1, 0, 65, T + 1], EDGES, LAGS)
    np.testing.assert_array_equal(wide[0][:, [0, 2, 3]], got[0])
    np.testing.assert_array_equal(wide[1][:, [0, 2, 3]], got[1])
    assert not wide[0][:, 1].any() and not wide[1][:, 1].any()
    with pytest.raises(ValueError):
        engine_run(pos[:, :50], sizes, EDGES, LAGS)                 # wrong number of rows


@pytest.mark.parametrize("n_bins", [1, 2, 201, 5000])      # 5000: more than the LDS holds, counted in HBM directly
def test_engine_bin_counts_and_a_positive_r_min(n_bins):
    sizes = [1, 65, T + 1]
    pos = diffusing(8, 37, sum(sizes))
    edges = np.linspace(0.5, 9.0, n_bins + 1)
    want = restate(pos, sizes, edges, LAGS)
    got = engine_run(pos, sizes, edges, LAGS)
    assert_same(got, want)
    assert not got[0][0].any()                                      # lag 0: r = 0 lies below r_min
    assert got[1][0].sum() == 0 and 0 < got[0][1].sum() < sum(sizes) * 36
    np.testing.assert_array_equal(got[2], engine_run(pos, sizes, EDGES, LAGS)[2])      # moments: all the same


def test_engine_displacements_on_the_edges():
    """float32 coordinates on a grid of 0.25 and edges = linspace(0, 8, 33): every r below is exact."""
    edges = np.linspace(0.0, 8.0, 33)
    moves = np.array([[0.75, 0.0, 0.0],        # r = 0.75, an inner edge: counted in the bin that starts there
                      [0.75, 1.0, 0.0],        # r = 1.25 exactly
                      [0.0, -3.0, 4.0],        # r = 5
                      [8.0, 0.0, 0.0],         # r == r_max: the last bin
                      [0.0, 4.75, -6.5],       # r just above r_max (8.0505...): not counted, in the moments
                      [8.25, 0.0, 0.0],        # the same, exact
                      [0.0, 0.0, 0.0],
                      [0.25, 0.0, 0.0]])
    n = len(moves)
    rng = np.random.default_rng(3)
    first = rng.integers(0, 400, (n, 3)) * 0.25
    pos = np.stack((first, first + moves)).astype(np.float32)
    np.testing.assert_array_equal(pos.astype(np.float64), np.stack((first, first + moves)))
    got = engine_run(pos, [n], edges, [0, 1])
    assert_same(got, restate(pos, [n], edges, [0, 1]))
    r = np.sqrt((moves ** 2).sum(axis=1))
    np.testing.assert_array_equal(r[:4], [0.75, 1.25, 5.0, 8.0])
    want = np.zeros(32, dtype=np.int64)
    for b in (3, 5, 20, 31, 0, 1):
        want[b] += 1
    np.testing.assert_array_equal(got[0][1, 0], want)
    assert got[0][1, 0].sum() == n - 2 and got[0][0, 0, 0] == 2 * n
    assert got[1][1, 0, 0] == (moves ** 2).sum()                    # the uncounted ones are in the moments
    np.testing.assert_array_equal(got[2][1, :, 0], (moves ** 2).sum(axis=1))


@pytest.mark.parametrize("n", [65, 2 * T + 3])
def test_engine_all_points_at_rest(n):
    """Every count of every lag in the bin of 0: the contended path."""
    F = 37
    pos = np.broadcast_to(diffusing(9, 1, n), (F, n, 3)).copy()
    got = engine_run(pos, [n], EDGES, LAGS)
    np.testing.assert_array_equal(got[0].sum(axis=-1)[:, 0], [n * max(F - lag, 0) for lag in LAGS])
    np.testing.assert_array_equal(got[0][:, 0, 0], got[0].sum(axis=-1)[:, 0])
    assert not got[1].any() and not got[2].any()
    assert_same(got, restate(pos, [n], EDGES, LAGS))


def _walk(seed, F, n, dims):
    """A random walk with steps of about L / 5 per frame, wrapped into the box: float32[F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, 1.0, (F, n, 3)) * dims / 5, axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


UNWRAP_DIMS = np.array([31.0, 44.5, 57.25])
UNWRAP_SIZES = [1, 65, T + 1]
UNWRAP_EDGES = np.linspace(0.0, 60.0, 202)


@pytest.fixture(scope="module")
def walk():
    """Frames and the restatement with and without unwrap, shared and left unchanged."""
    pos = _walk(11, 37, sum(UNWRAP_SIZES), UNWRAP_DIMS)
    want = restate(pos, UNWRAP_SIZES, UNWRAP_EDGES, LAGS, dims=UNWRAP_DIMS)
    wrapped = restate(pos, UNWRAP_SIZES, UNWRAP_EDGES, LAGS)
    images = images_ref(pos, UNWRAP_DIMS)
    for a in (pos, images, *want[:3], *wrapped[:3]):
        a.setflags(write=False)
    return {"pos": pos, "images": images, "want": want, "wrapped": wrapped}


def test_unwrap_input_cannot_pass_with_the_unwrap_off(walk):
    """What the test asserts of its own input, so that the unwrap cases mean something."""
    steps = np.diff(walk["images"], axis=0)
    for d in range(3):
        assert (steps[..., d] == 1).any() and (steps[..., d] == -1).any()      # crossings of both signs
    assert np.abs(steps).max() == 1 and np.abs(walk["images"]).max() >= 2
    differs = (walk["want"][0] != walk["wrapped"][0]).any(axis=-1)              # [lag, group]
    assert differs[1:5].any(axis=0).all()                                       # every group, at some lag
    assert not differs[0].any() and not differs[5].any()                        # lag 0 and the lag without origin


def test_unwrap_against_the_rule(walk):
    setup = lambda e: e.set_unwrap(UNWRAP_DIMS)      # noqa: E731
    assert_same(engine_run(walk["pos"], UNWRAP_SIZES, UNWRAP_EDGES, LAGS, setup=setup), walk["want"])
    assert_same(engine_run(walk["pos"], UNWRAP_SIZES, UNWRAP_EDGES, LAGS), walk["wrapped"])
    eng = _core.VanHoveEngine(UNWRAP_SIZES, UNWRAP_EDGES, LAGS)
    try:
        eng.set_unwrap(UNWRAP_DIMS)
        eng.accumulate(walk["pos"][:4])
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_unwrap(UNWRAP_DIMS)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_unwrap(None)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(8)
        eng.reset()
        eng.set_unwrap(None)
        eng.set_slab_frames(8)
        eng.accumulate(walk["pos"])
        counts, moments = eng.result()
        np.testing.assert_array_equal(counts, walk["wrapped"][0])
        np.testing.assert_array_equal(moments, walk["wrapped"][1])
    finally:
        eng.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(walk, axis):
    pos = walk["pos"]
    want = restate(pos, UNWRAP_SIZES, UNWRAP_EDGES, LAGS, dims=UNWRAP_DIMS, zero_dims=1 << axis)
    got = engine_run(pos, UNWRAP_SIZES, UNWRAP_EDGES, LAGS, setup=lambda e: e.set_unwrap(UNWRAP_DIMS),
                     zero_dims=1 << axis)
    assert_same(got, want)
    assert (want[1][1:5] < walk["want"][1][1:5]).all()
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    np.testing.assert_array_equal(engine_run(flat, UNWRAP_SIZES, UNWRAP_EDGES, LAGS,
                                             setup=lambda e: e.set_unwrap(UNWRAP_DIMS))[1], got[1])


@pytest.mark.parametrize("unwrap", [False, True])
def test_one_set_of_bits_whatever_the_split_slab_route_or_index(walk, unwrap, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, sizes = walk["pos"], UNWRAP_SIZES
    F, n = pos.shape[:2]
    want = walk["want" if unwrap else "wrapped"]

    def setup(e, slab=None):
        if unwrap:
            e.set_unwrap(UNWRAP_DIMS)
        if slab is not None:
            e.set_slab_frames(slab)

    def same(eng):
        counts, moments = eng.result()
        np.testing.assert_array_equal(counts, want[0])
        np.testing.assert_array_equal(moments, want[1])
        np.testing.assert_array_equal(eng.point_moments(), want[2])
        assert eng.stats()["evaluations"] == want[3] and eng.stats()["frames"] == F

    run = lambda **kw: engine_run(pos, sizes, UNWRAP_EDGES, LAGS, **kw)      # noqa: E731
    assert_same(run(setup=setup), want)
    assert_same(run(splits=[0, 1, 5, 37], setup=setup), want)       # lag 36 spans every call
    assert_same(run(setup=lambda e: setup(e, 8)), want)
    assert_same(run(splits=[0, 1, 5, 37], setup=lambda e: setup(e, 8)), want)
    assert_same(run(setup=lambda e: setup(e, 1)), want)

    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    rng = np.random.default_rng(13)
    n_total = 2 * n + 5
    index = rng.permutation(n_total)[:n]
    assert np.any(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    big = rng.uniform(0.0, 30.0, (F, n_total, 3)).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.tile(UNWRAP_DIMS, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.VanHoveEngine(sizes, UNWRAP_EDGES, LAGS)
    try:
        setup(eng)
        eng.accumulate_device(d.ptr, n, F)
        same(eng)                                                   # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.stats()["evaluations"] == 0
        counts, moments = eng.result()
        assert not counts.any() and not moments.any() and not eng.point_moments().any()
        eng.accumulate_traj(tf, np.arange(F))
        same(eng)                                                   # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        same(eng)                                                   # HBM through the index
        with pytest.raises(ValueError):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))      # out of range
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        same(eng)                                                   # file through the index
        eng.reset()
        eng.set_slab_frames(8)
        eng.accumulate_device(d.rows(0, 5).ptr, n, 5)               # routes mixed within one pass
        eng.accumulate(pos[5:20])
        eng.accumulate_traj(tf, np.arange(20, F))
        same(eng)
        eng.reset()
        eng.set_slab_frames(0)                                      # the default again
        eng.accumulate(pos)
        same(eng)
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


WRAP_LAGS = [0, 1, 3]


@pytest.fixture(scope="module")
def short_walk():
    """9 frames of 65 points (a tile and one point) and the restatement for lags 0, 1, 3 without and with unwrap,
    shared and left unchanged."""
    pos = _walk(17, 9, 65, UNWRAP_DIMS)
    want = {unwrap: restate(pos, [65], UNWRAP_EDGES, WRAP_LAGS, dims=UNWRAP_DIMS if unwrap else None)
            for unwrap in (False, True)}
    assert (want[False][0] != want[True][0]).any()                  # points cross the box within 9 frames
    assert all(w[0].sum(axis=(1, 2)).all() for w in want.values())  # every lag counts something
    for a in (pos, *want[False][:3], *want[True][:3]):
        a.setflags(write=False)
    return pos, want


@pytest.mark.parametrize("unwrap", [False, True])
@pytest.mark.parametrize("slab", [1, 2])
def test_the_ring_wraps(short_walk, slab, unwrap):
    """With lags up to 3 the ring holds 3 + slab frames, fewer than the 9 fed in two calls: every slot is written
    twice or more, the second call starts in the middle of the ring, and lag 3 reaches back across the wrap and
    across the calls.  (The other tests of this file feed 37 frames to a ring of at least 41.)"""
    pos, want = short_walk
    assert WRAP_LAGS[-1] + slab < len(pos)

    def setup(e):
        if unwrap:
            e.set_unwrap(UNWRAP_DIMS)
        e.set_slab_frames(slab)

    assert_same(engine_run(pos, [65], UNWRAP_EDGES, WRAP_LAGS, splits=[0, 4, 9], setup=setup), want[unwrap])
    assert_same(engine_run(pos, [65], UNWRAP_EDGES, WRAP_LAGS, setup=setup), want[unwrap])


# ---------------------------------------------------------------- the class

def _mixture(seed=20, F=12):
    """Cations, three particles of no group, anions: (pos float32[F, n, 3], boxes float32[F, 6], ia, ib)."""
    n_c, extra, n_a = 70, 3, T + 5
    n = n_c + extra + n_a
    pos = diffusing(seed, F, n, step=0.8)
    boxes = np.tile(np.array([60.0, 60.0, 60.0, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    return pos, boxes, np.arange(n_c), np.arange(n_c + extra, n)


def test_class_groups_routes_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    pos, boxes, ia, ib = _mixture()
    F = len(pos)
    order = np.concatenate((ib, ia))                       # anions first: not the order of the frame
    sizes = [len(ib), len(ia)]
    lags = np.array([0, 1, 3, 11, 15])
    edges = np.linspace(0.0, 6.0, 25)
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)

    def check(v, frames, step):
        """v.results against the restatement on the selected frames."""
        counts, moments, _, _ = restate(pos[frames][:, order], sizes, edges, lags)
        res = v.results
        np.testing.assert_array_equal(res.counts, counts)
        assert res.counts.dtype == np.int64 and res.counts.shape == (5, 2, 24)
        np.testing.assert_array_equal(res.edges, edges)
        np.testing.assert_array_equal(res.bins, (edges[:-1] + edges[1:]) / 2)
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        origins = np.maximum(len(frames) - lags, 0).astype(float)
        origins[origins == 0] = np.nan
        pairs = origins[:, None] * np.array(sizes)[None, :]
        np.testing.assert_array_equal(res.msd, moments[..., 0] / pairs)
        assert np.all(res.msd[0] == 0.0)                                        # lag 0: exactly 0
        np.testing.assert_array_equal(res.alpha2,
                                      calculate_non_gaussian_parameter(moments[..., 0] / pairs,
                                                                       moments[..., 1] / pairs))
        assert np.isnan(res.alpha2[0]).all()
        # a row of the probability integrates to the share of displacements inside the range
        live = ~np.isnan(origins)
        np.testing.assert_allclose((res.probability * np.diff(edges)).sum(axis=-1)[live],
                                   (counts.sum(axis=-1) / pairs)[live], rtol=1e-14)
        shell = 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
        np.testing.assert_array_equal(res.vanhove[live], (counts / (pairs[:, :, None] * shell))[live])
        for a in (res.probability, res.vanhove, res.msd, res.alpha2):           # lags without an origin: NaN
            assert np.isnan(a[~live]).all()
        assert not res.counts[~live].any()
        assert set(res.units) == {"results.bins", "results.edges", "results.times", "results.probability",
                                  "results.vanhove", "results.msd"}

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            groups = [u.select(ib), u.select(ia)]
            make = lambda: VanHove(groups, 24, (0.0, 6.0), lags=lags, verbose=False)      # noqa: E731
            full = make().run()
            check(full, np.arange(F), 1)
            assert 0 < full.results.counts[3].sum() < sum(sizes) * (F - 11)     # part of lag 11 beyond the range
            check(make().run(start=1, stop=12, step=2), np.arange(1, 12, 2), 2)
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in ("counts", "msd", "alpha2", "probability", "vanhove"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # every particle in order (no index), and neither lags nor n_lags: every analysed frame is a lag
        one = VanHove(u.atoms, 24, (0.0, 6.0), verbose=False).run()
        counts, moments, _, _ = restate(pos, [pos.shape[1]], edges, np.arange(F))
        np.testing.assert_array_equal(one.results.counts, counts)
        np.testing.assert_array_equal(one.results.msd, moments[..., 0] / ((F - np.arange(F))[:, None] * pos.shape[1]))
        np.testing.assert_array_equal(VanHove(u.atoms, 24, (0.0, 6.0), n_lags=4, verbose=False).run().results.counts,
                                      counts[:4])
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(VanHove([u.select(ib), u.select(ia)], 24, (0.0, 6.0), lags=lags, verbose=False)).run()
        np.testing.assert_array_equal(slow.results.counts, results["host"].counts)
        np.testing.assert_array_equal(slow.results.msd, results["host"].msd)
        with pytest.raises(ValueError, match="evenly spaced"):
            VanHove(u.atoms, verbose=False).run(frames=[0, 1, 3])
    finally:
        d.free()


def test_class_unwrap_and_drop_axis(walk):
    pos = walk["pos"]
    n = pos.shape[1]
    u = mdhelper_amd.ArrayUniverse(pos, [*UNWRAP_DIMS, 90.0, 90.0, 90.0])
    lags = np.array(LAGS)
    live = lags < len(pos)
    off = VanHove(u.atoms, 201, (0.0, 60.0), lags=LAGS, verbose=False).run()
    np.testing.assert_array_equal(off.results.counts, walk["wrapped"][0].sum(axis=1, keepdims=True))
    for dimensions in (None, UNWRAP_DIMS):                 # the universe's box lengths are the default
        on = VanHove(u.atoms, 201, (0.0, 60.0), lags=LAGS, dimensions=dimensions, unwrap=True, verbose=False).run()
        np.testing.assert_array_equal(on.results.counts, walk["want"][0].sum(axis=1, keepdims=True))
    counts, moments, _, _ = restate(pos, [n], UNWRAP_EDGES, LAGS, dims=UNWRAP_DIMS, zero_dims=4)
    flat = VanHove(u.atoms, 201, (0.0, 60.0), lags=LAGS, drop_axis="z", unwrap=True, verbose=False).run()
    np.testing.assert_array_equal(flat.results.counts, counts)
    pairs = (np.maximum(len(pos) - lags, 0) * n).astype(float)[:, None]
    pairs[pairs == 0] = np.nan
    ring = np.pi * (UNWRAP_EDGES[1:] ** 2 - UNWRAP_EDGES[:-1] ** 2)
    np.testing.assert_array_equal(flat.results.vanhove[live], (counts / (pairs[:, :, None] * ring))[live])
    np.testing.assert_array_equal(flat.results.alpha2[live],
                                  calculate_non_gaussian_parameter(moments[..., 0] / pairs, moments[..., 1] / pairs,
                                                                   2)[live])
    assert np.isnan(flat.results.vanhove[~live]).all() and flat.results.units["results.vanhove"] == "angstrom^-2"
