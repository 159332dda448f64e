"""
FourPointSusceptibility / FourPointEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_chi4_device.hpp): per lag k, cutoff c and origin f0 (a multiple of origin_step with f0 + lag analysed)

    x = (double)r + image * L;  d = x(f0 + lag) - x(f0) (+0.0 for a dropped component);
    r2 = (dx*dx + dy*dy) + dz*dz;  Q = #{points of the group: r2 <= a_c * a_c};  S1 += Q;  S2 += Q*Q

with the image counts of the reference's global unwrap restated frame by frame (the first frame is its own start).

No tolerance anywhere.  The restatement does one float64 operation at a time, as the device does (the unit is built
with contraction off), so every r2 has the same bits on both sides and every comparison the same outcome; Q, S1 and S2
are integers, and integer sums do not depend on the order.  Everything is compared with ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import FourPointSusceptibility, calculate_four_point_susceptibility

pytestmark = pytest.mark.gpu

T = _core.FourPointEngine.TILE
LAGS = [0, 1, 2, 5, 36, 40]           # lag 40 never has an origin in 37 frames
CUTOFFS = (0.0, 1.5, 4.0)


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


def squared_displacements(x, f, f0, zero_dims=0):
    d = x[f] - x[f0]
    for c in range(3):
        if zero_dims >> c & 1:
            d[:, c] = 0.0
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def restate(pos, sizes, cutoffs, lags, *, origin_step=1, dims=None, zero_dims=0):
    """(sums int64 [K, G, C], square_sums int64 [K, G, C], n_origins int64 [K], evaluations)."""
    x = np.asarray(pos).astype(np.float64)
    if dims is not None:
        x = x + images_ref(pos, dims).astype(np.float64) * np.asarray(dims, dtype=np.float64)
    F, n = x.shape[:2]
    a = np.atleast_1d(np.asarray(cutoffs, dtype=np.float64))
    a2 = a * a
    shape = (len(lags), len(sizes), len(a2))
    s1, s2 = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    origins = np.zeros(len(lags), dtype=np.int64)
    evaluations = 0
    for k, lag in enumerate(lags):
        for f0 in range(0, F - lag, origin_step):
            r2 = squared_displacements(x, f0 + lag, f0, zero_dims)
            lo = 0
            for g, size in enumerate(sizes):
                for c in range(len(a2)):
                    q = int(np.count_nonzero(r2[lo:lo + size] <= a2[c]))
                    s1[k, g, c] += q
                    s2[k, g, c] += q * q
                lo += size
            origins[k] += 1
            evaluations += n
    return s1, s2, origins, evaluations


def engine_run(pos, sizes, cutoffs, lags, *, splits=None, setup=None, origin_step=1, zero_dims=0):
    eng = _core.FourPointEngine(sizes, cutoffs, lags, origin_step=origin_step, zero_dims=zero_dims)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return (*eng.result(), eng.stats())
    finally:
        eng.close()


def assert_same(got, want):
    """got: engine_run's tuple; want: restate's."""
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(a, b)
        assert a.dtype == np.int64 and a.shape == b.shape
    assert got[3]["evaluations"] == want[3]


def segment(points):
    return lambda e: e.set_segment_points(points)


def diffusing(seed, F, n, step=1.2):
    """A free random walk, float32[F, n, 3]: displacements from 0 to far beyond the cutoffs at the long lags."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 40.0, (1, n, 3)) + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)).astype(np.float32)


# ---------------------------------------------------------------- engine

# 200: two whole loads at a time, then one more, then a tail
@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, 2 * T - 1, 2 * T, 2 * T + 1, 200, 4 * T + 3}))
def test_engine_group_sizes_and_frame_counts(n):
    for F in (1, 2, 37):
        pos = diffusing(100 + n, F, n)
        want = restate(pos, [n], CUTOFFS, LAGS)
        for setup in (None, segment(64), segment(128)):     # one segment; several, a tail, a boundary inside
            got = engine_run(pos, [n], CUTOFFS, LAGS, setup=setup)
            assert_same(got, want)
            assert got[3]["frames"] == F
        assert want[3] == n * sum(max(F - lag, 0) for lag in LAGS)
        np.testing.assert_array_equal(want[2], [max(F - lag, 0) for lag in LAGS])
        assert not got[0][5].any() and not got[1][5].any() and got[2][5] == 0      # lag 40: no origin
        np.testing.assert_array_equal(got[0][0, 0], [n * F] * 3)                    # lag 0: r2 = 0 <= 0
        np.testing.assert_array_equal(got[1][0, 0], [n * n * F] * 3)
        if F == 37 and n >= 63:
            assert got[0][4, 0, 2] < n                                              # lag 36: most have left
            assert np.all(np.diff(got[0][1:4, 0], axis=-1) > 0)                     # the cutoffs tell apart
            assert 0 < got[0][1, 0, 1] < n * 36


def test_engine_three_unequal_groups():
    sizes = [1, 65, 130]
    n, F = sum(sizes), 37
    pos = diffusing(7, F, n)
    want = restate(pos, sizes, CUTOFFS, LAGS)
    for setup in (None, segment(64), segment(128)):
        got = engine_run(pos, sizes, CUTOFFS, LAGS, setup=setup)
        assert_same(got, want)
        # the rows of a group do not depend on what the other groups are: a load never spans two groups
        for g, (lo, hi) in enumerate(((0, 1), (1, 66), (66, n))):
            solo = engine_run(pos[:, lo:hi], [hi - lo], CUTOFFS, LAGS, setup=setup)
            np.testing.assert_array_equal(solo[0][:, 0], got[0][:, g])
            np.testing.assert_array_equal(solo[1][:, 0], got[1][:, g])
        # an empty group between them: zero rows, the others unchanged
        wide = engine_run(pos, [1, 0, 65, 130, 0], CUTOFFS, LAGS, setup=setup)
        np.testing.assert_array_equal(wide[0][:, [0, 2, 3]], got[0])
        np.testing.assert_array_equal(wide[1][:, [0, 2, 3]], got[1])
        assert not wide[0][:, [1, 4]].any() and not wide[1][:, [1, 4]].any()
    with pytest.raises(ValueError):
        engine_run(pos[:, :50], sizes, CUTOFFS, LAGS)               # wrong number of rows


@pytest.mark.parametrize("sizes", [[65], [4 * T + 3], [1, 65, 130]])
def test_engine_all_points_at_rest(sizes):
    """Q = n_g for every cutoff, 0.0 included, and S2 = n_origins n_g^2: a tail lane that was counted, or a lane
    counted twice, shows here."""
    F, n = 37, sum(sizes)
    pos = np.broadcast_to(diffusing(9, 1, n), (F, n, 3)).copy()
    for setup in (None, segment(64), segment(128)):
        s1, s2, origins, _ = engine_run(pos, sizes, CUTOFFS, LAGS, setup=setup)
        np.testing.assert_array_equal(origins, [max(F - lag, 0) for lag in LAGS])
        for g, size in enumerate(sizes):
            np.testing.assert_array_equal(s1[:, g], np.repeat(origins * size, 3).reshape(-1, 3))
            np.testing.assert_array_equal(s2[:, g], np.repeat(origins * size * size, 3).reshape(-1, 3))
    assert_same(engine_run(pos, sizes, CUTOFFS, LAGS), restate(pos, sizes, CUTOFFS, LAGS))


def test_engine_displacements_on_the_cutoff():
    """float32-exact moves against the cutoff 5.0: r2 == 25 counts, the next float32 above 5 does not."""
    above = np.nextafter(np.float32(5.0), np.float32(6.0))          # 5.0000005
    assert 5.0 < float(above) < 5.000001
    moves = np.array([[3.0, 4.0, 0.0],           # r2 = 25 exactly: counted
                      [0.0, -3.0, 4.0],          # the same
                      [5.0, 0.0, 0.0],           # the same
                      [float(above), 0.0, 0.0],  # just beyond: not counted
                      [3.0, 4.0, 7.0],           # counted only where z is dropped
                      [0.0, 0.0, 0.0],
                      [3.0, 4.0, 0.25]])         # r2 = 25.0625: not counted; counted where z is dropped
    n = len(moves)
    first = np.zeros((n, 3))
    first[[0, 1, 2, 4, 5, 6]] = np.random.default_rng(3).integers(0, 16, (6, 3)) * 0.25     # exact in float32
    pos = np.stack((first, first + moves)).astype(np.float32)
    np.testing.assert_array_equal(pos.astype(np.float64), np.stack((first, first + moves)))
    for zero, q in ((0, 4), (4, 6)):
        got = engine_run(pos, [n], [5.0], [0, 1], zero_dims=zero)
        assert_same(got, restate(pos, [n], [5.0], [0, 1], zero_dims=zero))
        np.testing.assert_array_equal(got[0][:, 0, 0], [2 * n, q])
        np.testing.assert_array_equal(got[1][:, 0, 0], [2 * n * n, q * q])
    # the two cutoffs on either side of the float32 step tell the point apart
    got = engine_run(pos, [n], [5.0, float(above)], [1])
    np.testing.assert_array_equal(got[0][0, 0], [4, 5])
    # dropping x or y instead: the restatement again
    for zero in (1, 2, 3, 5, 6):
        assert_same(engine_run(pos, [n], [5.0], [0, 1], zero_dims=zero),
                    restate(pos, [n], [5.0], [0, 1], zero_dims=zero))


@pytest.mark.parametrize("origin_step", [1, 3, 7])
def test_engine_origin_step_counts_global_frames(origin_step):
    """The origins are the multiples of the step in global frame numbers, across calls and slabs."""
    sizes = [65, 130]
    pos = diffusing(21, 37, sum(sizes))
    want = restate(pos, sizes, CUTOFFS, LAGS, origin_step=origin_step)
    np.testing.assert_array_equal(want[2], [-(-max(37 - lag, 0) // origin_step) for lag in LAGS])
    slab = lambda e: e.set_slab_frames(8)      # noqa: E731
    assert_same(engine_run(pos, sizes, CUTOFFS, LAGS, origin_step=origin_step), want)
    assert_same(engine_run(pos, sizes, CUTOFFS, LAGS, origin_step=origin_step, setup=slab), want)
    assert_same(engine_run(pos, sizes, CUTOFFS, LAGS, origin_step=origin_step, splits=[0, 1, 9, 10, 37]), want)
    assert_same(engine_run(pos, sizes, CUTOFFS, LAGS, origin_step=origin_step, splits=[0, 1, 9, 10, 37], setup=slab),
                want)
    if origin_step > 1:
        assert (want[0][1:5] < restate(pos, sizes, CUTOFFS, LAGS)[0][1:5]).any()


def _walk(seed, F, n, dims):
    """A random walk with steps of about L / 5 per frame, wrapped into the box: float32[F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, 1.0, (F, n, 3)) * dims / 5, axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


UNWRAP_DIMS = np.array([31.0, 44.5, 57.25])
UNWRAP_SIZES = [1, 65, 130]
UNWRAP_CUTOFFS = (8.0, 16.0, 30.0)


@pytest.fixture(scope="module")
def walk():
    """Frames and the restatement with and without unwrap, shared and left unchanged."""
    pos = _walk(11, 37, sum(UNWRAP_SIZES), UNWRAP_DIMS)
    want = restate(pos, UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS, dims=UNWRAP_DIMS)
    wrapped = restate(pos, UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS)
    images = images_ref(pos, UNWRAP_DIMS)
    for a in (pos, images, *want[:3], *wrapped[:3]):
        a.setflags(write=False)
    return {"pos": pos, "images": images, "want": want, "wrapped": wrapped}


def test_unwrap_against_the_rule(walk):
    # what the test asserts of its own input, so that the unwrap cases mean something
    steps = np.diff(walk["images"], axis=0)
    for d in range(3):
        assert (steps[..., d] == 1).any() and (steps[..., d] == -1).any()      # crossings of both signs
    differs = (walk["want"][0] != walk["wrapped"][0]).any(axis=-1)              # [lag, group]
    assert differs[1:5, 1:].any(axis=0).all()                                   # both larger groups, at some lag
    assert not differs[0].any() and not differs[5].any()                        # lag 0 and the lag without origin

    setup = lambda e: e.set_unwrap(UNWRAP_DIMS)      # noqa: E731
    assert_same(engine_run(walk["pos"], UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS, setup=setup), walk["want"])
    got = engine_run(walk["pos"], UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS)
    assert_same(got, walk["wrapped"])                                           # the same input, unwrap off
    assert (got[0] != walk["want"][0]).any() and (got[1] != walk["want"][1]).any()
    eng = _core.FourPointEngine(UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS)
    try:
        eng.set_unwrap(UNWRAP_DIMS)
        eng.accumulate(walk["pos"][:4])
        for late in (lambda: eng.set_unwrap(UNWRAP_DIMS), lambda: eng.set_unwrap(None),
                     lambda: eng.set_slab_frames(8), lambda: eng.set_segment_points(64)):
            with pytest.raises(ValueError, match="before the first frame"):
                late()
        eng.reset()
        eng.set_unwrap(None)
        eng.set_slab_frames(8)
        eng.set_segment_points(64)
        eng.accumulate(walk["pos"])
        for a, b in zip(eng.result(), walk["wrapped"][:3]):
            np.testing.assert_array_equal(a, b)
    finally:
        eng.close()


@pytest.mark.parametrize("unwrap", [False, True])
def test_one_set_of_bits_whatever_the_split_slab_segment_route_or_index(walk, unwrap, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, sizes = walk["pos"], UNWRAP_SIZES
    F, n = pos.shape[:2]
    want = walk["want" if unwrap else "wrapped"]

    def setup(e, slab=None, points=None):
        if unwrap:
            e.set_unwrap(UNWRAP_DIMS)
        if slab is not None:
            e.set_slab_frames(slab)
        if points is not None:
            e.set_segment_points(points)

    def same(eng):
        for a, b in zip(eng.result(), want[:3]):
            np.testing.assert_array_equal(a, b)
        assert eng.stats()["evaluations"] == want[3] and eng.stats()["frames"] == F

    run = lambda **kw: engine_run(pos, sizes, UNWRAP_CUTOFFS, LAGS, **kw)      # noqa: E731
    assert_same(run(setup=setup), want)
    assert_same(run(splits=[0, 1, 5, 37], setup=setup), want)       # lag 36 spans every call
    assert_same(run(setup=lambda e: setup(e, 8)), want)
    assert_same(run(setup=lambda e: setup(e, None, 64)), want)
    assert_same(run(splits=[0, 1, 5, 37], setup=lambda e: setup(e, 8, 64)), want)
    assert_same(run(setup=lambda e: setup(e, 1, 128)), want)

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
    eng = _core.FourPointEngine(sizes, UNWRAP_CUTOFFS, LAGS)
    try:
        setup(eng)
        eng.accumulate_device(d.ptr, n, F)
        same(eng)                                                   # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.stats()["evaluations"] == 0
        s1, s2, origins = eng.result()
        assert not s1.any() and not s2.any() and not origins.any()
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
        eng.set_segment_points(64)
        eng.accumulate_device(d.rows(0, 5).ptr, n, 5)               # routes mixed within one pass
        eng.accumulate(pos[5:20])
        eng.accumulate_traj(tf, np.arange(20, F))
        same(eng)
        eng.reset()
        eng.set_slab_frames(0)                                      # the defaults again
        eng.set_segment_points(0)
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
    """9 frames of 65 points (a wave and one point) and the restatement for lags 0, 1, 3 without and with unwrap,
    shared and left unchanged."""
    pos = _walk(17, 9, 65, UNWRAP_DIMS)
    want = {unwrap: restate(pos, [65], UNWRAP_CUTOFFS, WRAP_LAGS, dims=UNWRAP_DIMS if unwrap else None)
            for unwrap in (False, True)}
    assert (want[False][0] != want[True][0]).any()                  # points cross the box within 9 frames
    assert all(w[0].all() for w in want.values())                   # every lag and cutoff counts something
    np.testing.assert_array_equal(want[True][2], [9, 8, 6])
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

    assert_same(engine_run(pos, [65], UNWRAP_CUTOFFS, WRAP_LAGS, splits=[0, 4, 9], setup=setup), want[unwrap])
    assert_same(engine_run(pos, [65], UNWRAP_CUTOFFS, WRAP_LAGS, setup=setup), want[unwrap])


def test_sums_equal_the_van_hove_counts_up_to_the_cutoff():
    """One cutoff a against the van Hove engine with the single bin [0, a] (closed on the right): the same points,
    found by r2 <= a*a here and by sqrt(r2) <= a there.  The two can disagree only for an r2 within an ulp or so of
    a*a; the data keep every r2 a relative 1e-9 away from it, which is asserted first."""
    sizes, a = [65, 130], 3.0
    pos = diffusing(31, 37, sum(sizes))
    x = pos.astype(np.float64)
    gaps = [np.abs(squared_displacements(x, f0 + lag, f0) / (a * a) - 1.0).min()
            for lag in LAGS for f0 in range(37 - lag)]
    assert min(gaps) > 1e-9
    s1, _, origins, stats = engine_run(pos, sizes, [a], LAGS)
    vh = _core.VanHoveEngine(sizes, [0.0, a], LAGS)
    try:
        vh.accumulate(pos)
        counts, _ = vh.result()
        assert vh.stats()["evaluations"] == stats["evaluations"]
    finally:
        vh.close()
    np.testing.assert_array_equal(s1[..., 0], counts[..., 0])
    assert 0 < s1[3].sum() < origins[3] * sum(sizes)


# ---------------------------------------------------------------- the class

def _mixture(seed=20, F=12):
    """Cations, three particles of no group, anions: (pos float32[F, n, 3], boxes float32[F, 6], ia, ib)."""
    n_c, extra, n_a = 70, 3, 2 * T + 5
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
    cutoffs = [1.0, 2.5]
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)

    def check(v, frames, step, origin_step=1):
        """v.results against the engine fed directly with the selected frames, and against the restatement."""
        rows = np.ascontiguousarray(pos[frames][:, order])
        live = lags < len(frames)
        s1, s2, origins, _ = engine_run(rows, sizes, cutoffs, lags[live], origin_step=origin_step)
        want = restate(rows, sizes, cutoffs, lags, origin_step=origin_step)
        res = v.results
        np.testing.assert_array_equal(res.sums[live], s1)
        np.testing.assert_array_equal(res.square_sums[live], s2)
        np.testing.assert_array_equal(res.n_origins[live], origins)
        np.testing.assert_array_equal(res.sums, want[0])
        np.testing.assert_array_equal(res.square_sums, want[1])
        np.testing.assert_array_equal(res.n_origins, want[2])
        assert res.sums.dtype == np.int64 and res.sums.shape == (5, 2, 2)
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        np.testing.assert_array_equal(res.cutoffs, cutoffs)
        terms = (want[2][:, None] * np.array(sizes)[None, :]).astype(float)
        terms[terms == 0] = np.nan
        np.testing.assert_array_equal(res.overlap, want[0] / terms[:, :, None])
        assert np.all(res.overlap[0] == 1.0)                                    # lag 0: every point, exactly
        np.testing.assert_array_equal(res.chi4,
                                      calculate_four_point_susceptibility(want[0], want[1], want[2], sizes))
        assert np.all(res.chi4[0] == 0.0) and np.all(res.chi4[live] >= 0.0)
        for a in (res.overlap, res.chi4):                                       # lags without an origin: NaN rows
            assert np.isnan(a[~live]).all() and not np.isnan(a[live]).any()
        assert not res.sums[~live].any() and not res.n_origins[~live].any()
        assert (~live).any()                                                    # lag 15 >= n_frames in every case
        assert set(res.units) == {"results.times", "results.cutoffs", "results.relaxation_time",
                                  "results.peak_time"}

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            groups = [u.select(ib), u.select(ia)]
            make = lambda **kw: FourPointSusceptibility(groups, cutoffs, lags=lags, verbose=False, **kw)   # noqa: E731
            full = make().run()
            check(full, np.arange(F), 1)
            assert 0 < full.results.sums[2].sum() < sum(sizes) * (F - 3) * 2    # some have left after 3 frames
            check(make().run(start=1, stop=12, step=2), np.arange(1, 12, 2), 2)
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3)
            check(make(origin_step=3).run(), np.arange(F), 1, origin_step=3)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in ("sums", "square_sums", "n_origins", "overlap", "chi4"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # every particle in order (no index), a scalar cutoff, and neither lags nor n_lags: every frame is a lag
        one = FourPointSusceptibility(u.atoms, 2.5, verbose=False).run()
        want = restate(pos, [pos.shape[1]], [2.5], np.arange(F))
        np.testing.assert_array_equal(one.results.sums, want[0])
        np.testing.assert_array_equal(one.results.square_sums, want[1])
        np.testing.assert_array_equal(FourPointSusceptibility(u.atoms, 2.5, n_lags=4, verbose=False).run().results.sums,
                                      want[0][:4])
        one.calculate_relaxation_times()
        assert one.results.relaxation_time.shape == one.results.peak_time.shape == (1, 1)
        assert 0.0 < one.results.relaxation_time[0, 0] < one.results.times[-1]
        assert one.results.peak_height[0, 0] == np.nanmax(one.results.chi4)
        # an empty group: NaN without a warning, the other group unchanged
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            holed = FourPointSusceptibility([u.select(ib), u.select(np.arange(0)), u.select(ia)], cutoffs, lags=lags,
                                            verbose=False).run()
        np.testing.assert_array_equal(holed.results.sums[:, [0, 2]], results["host"].sums)
        np.testing.assert_array_equal(holed.results.chi4[:, [0, 2]], results["host"].chi4)
        assert np.isnan(holed.results.overlap[:, 1]).all() and np.isnan(holed.results.chi4[:, 1]).all()
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(FourPointSusceptibility([u.select(ib), u.select(ia)], cutoffs, lags=lags,
                                                 verbose=False)).run()
        np.testing.assert_array_equal(slow.results.sums, results["host"].sums)
        np.testing.assert_array_equal(slow.results.square_sums, results["host"].square_sums)
    finally:
        d.free()


def test_class_unwrap_and_drop_axis(walk):
    pos = walk["pos"]
    n = pos.shape[1]
    u = mdhelper_amd.ArrayUniverse(pos, [*UNWRAP_DIMS, 90.0, 90.0, 90.0])
    groups = [u.select(np.arange(lo, lo + size)) for lo, size in zip(np.cumsum([0, *UNWRAP_SIZES]), UNWRAP_SIZES)]
    make = lambda **kw: FourPointSusceptibility(groups, UNWRAP_CUTOFFS, lags=LAGS, verbose=False, **kw)   # noqa: E731
    off = make().run()
    np.testing.assert_array_equal(off.results.sums, walk["wrapped"][0])
    np.testing.assert_array_equal(off.results.square_sums, walk["wrapped"][1])
    for dimensions in (None, UNWRAP_DIMS):                 # the universe's box lengths are the default
        on = make(dimensions=dimensions, unwrap=True).run()
        np.testing.assert_array_equal(on.results.sums, walk["want"][0])
        np.testing.assert_array_equal(on.results.square_sums, walk["want"][1])
    assert (on.results.sums != off.results.sums).any()
    want = restate(pos, UNWRAP_SIZES, UNWRAP_CUTOFFS, LAGS, dims=UNWRAP_DIMS, zero_dims=4)
    flat = make(drop_axis="z", unwrap=True).run()
    np.testing.assert_array_equal(flat.results.sums, want[0])
    np.testing.assert_array_equal(flat.results.square_sums, want[1])
    assert (flat.results.sums >= on.results.sums).all() and (flat.results.sums > on.results.sums).any()
    assert np.isnan(flat.results.chi4[5]).all() and np.isnan(flat.results.overlap[5]).all()       # lag 40
    assert n == sum(UNWRAP_SIZES)
