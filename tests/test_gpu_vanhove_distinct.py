"""
DistinctVanHove / DistinctVanHoveEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_vanhove_distinct_device.hpp): per frame pair (f0, f0 + lag), f0 a multiple of origin_step, and per pair
(i of set 1 at f0, j of set 2 at f0 + lag, j != i when both are one set)

    d = x2_j - x1_i;  s = d * (1.0 / L);  w = d - L * rint(s) (+0.0 for a dropped component);
    r2 = (wx*wx + wy*wy) + wz*wz;  r = sqrt(r2);  counts[lag] += numpy.histogram(r)

No tolerance anywhere: the counts are integers, the restatement does one float64 operation at a time, as the device
does (the unit is built with contraction off; rint rounds ties to even and sqrt is correctly rounded on both sides),
so every comparison is ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DistinctVanHove

pytestmark = pytest.mark.gpu

T = _core.DistinctVanHoveEngine.TILE
J = _core.DistinctVanHoveEngine.JCHUNK
LAGS = [0, 1, 2, 5, 8, 10]             # lag 10 never has an origin in 9 frames
BOX = np.array([31.0, 44.5, 57.25])
EDGES = np.linspace(0.0, 15.0, 202)    # 15 <= 15.5, half the shortest length


# ---------------------------------------------------------------- restatement

def distances(a, b, dims, zero_dims=0):
    """float64 [n1, n2]: the contract's r for every pair of a float64[n1, 3] and b float64[n2, 3]."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    d = b[None, :, :] - a[:, None, :]
    s = d * inv
    w = d - dims * np.rint(s)
    for c in range(3):
        if zero_dims >> c & 1:
            w[..., c] = 0.0
    r2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    return np.sqrt(r2)


def restate(x1, x2, edges, lags, dims, *, origin_step=1, zero_dims=0):
    """(counts int64 [K, n_bins], n_origins [K], evaluations); x2 None: one set, the pair i == j left out."""
    same = x2 is None
    a = np.asarray(x1).astype(np.float64)
    b = a if same else np.asarray(x2).astype(np.float64)
    F, n1, n2 = len(a), a.shape[1], b.shape[1]
    n_bins = len(edges) - 1
    counts = np.zeros((len(lags), n_bins), dtype=np.int64)
    n_origins = np.zeros(len(lags), dtype=np.int64)
    off_diagonal = ~np.eye(n1, dtype=bool) if same else None
    for k, lag in enumerate(lags):
        rs = []
        for f0 in range(0, F - lag, origin_step):
            r = distances(a[f0], b[f0 + lag], dims, zero_dims)
            rs.append(r[off_diagonal] if same else r.ravel())
            n_origins[k] += 1
        if rs:
            counts[k] = np.histogram(np.concatenate(rs), n_bins, (edges[0], edges[-1]))[0]
    evaluations = int(n_origins.sum()) * (n1 * n2 - (n1 if same else 0))
    return counts, n_origins, evaluations


def engine_run(x1, x2, edges, lags, dims, *, splits=None, setup=None, origin_step=1, zero_dims=0):
    """(counts, stats) of one pass over the frames, host route."""
    same = x2 is None
    pos = x1 if same else np.concatenate((x1, x2), axis=1)
    eng = _core.DistinctVanHoveEngine(x1.shape[1], x1.shape[1] if same else x2.shape[1], edges, lags, dims,
                                      same=same, origin_step=origin_step, zero_dims=zero_dims)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return eng.result(), eng.stats()
    finally:
        eng.close()


def assert_same(got, want, F=None):
    np.testing.assert_array_equal(got[0], want[0])
    assert got[0].dtype == np.int64
    assert got[1]["evaluations"] == want[2]
    if F is not None:
        assert got[1]["frames"] == F


def walk(seed, F, n, dims=BOX, step=0.7):
    """Uniform in the box, then a random walk wrapped into the box: float32[F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


def origins(F, lag, step=1):
    return len(range(0, max(F - lag, 0), step))


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n", sorted({1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3}))
def test_one_set_sizes_and_frame_counts(n):
    for F in (1, 2, 9):
        pos = walk(100 + n, F, n)
        want = restate(pos, None, EDGES, LAGS, BOX)
        got = engine_run(pos, None, EDGES, LAGS, BOX)
        assert_same(got, want, F)
        assert want[2] == sum(origins(F, lag) for lag in LAGS) * (n * n - n)
        assert not got[0][5].any()                                  # lag 10: no origin
        if n == 1:
            assert not got[0].any() and want[2] == 0                # no pair at all
        elif n >= 63 and F == 9:
            assert (got[0][:5].sum(axis=-1) > 0).all()
            assert got[0][0].sum() < 9 * (n * n - n)                # most pairs lie beyond r_max


@pytest.mark.parametrize("n1, n2", [(1, 1), (1, 2 * T + 3), (2 * T + 3, 1), (65, T + 1), (T + 1, 65)])
def test_two_sets_sizes_and_frame_counts(n1, n2):
    for F in (1, 2, 9):
        pos = walk(200 + n1, F, n1 + n2)
        x1, x2 = pos[:, :n1], pos[:, n1:]
        want = restate(x1, x2, EDGES, LAGS, BOX)
        got = engine_run(x1, x2, EDGES, LAGS, BOX)
        assert_same(got, want, F)
        assert want[2] == sum(origins(F, lag) for lag in LAGS) * n1 * n2
        assert not got[0][5].any()
    with pytest.raises(ValueError, match="rows given"):
        engine_run(x1, x2, EDGES, LAGS, BOX, setup=lambda e: e.accumulate(pos[:, :-1]))       # wrong row count


@pytest.mark.parametrize("n2", [J - 1, J, J + 1])
def test_partners_around_one_chunk_and_a_ring_that_wraps_inside_one_call(n2):
    """JCHUNK - 1, JCHUNK and JCHUNK + 1 partners (the last: a second chunk of one partner counts into the same bins)
    against T + 1 points (a second tile of one live lane).  Lags 0 and 1 with slabs of one frame: the ring holds two
    frames, so the third frame of the one call goes into the slot of the first."""
    n1 = T + 1
    pos = walk(300 + n2, 3, n1 + n2)
    x1, x2 = pos[:, :n1], pos[:, n1:]
    want = restate(x1, x2, EDGES, [0, 1], BOX)
    assert want[0].sum(axis=-1).all()
    assert_same(engine_run(x1, x2, EDGES, [0, 1], BOX, setup=lambda e: e.set_slab_frames(1)), want, 3)
    if n2 == J + 1:
        # one set: the second chunk's only partner is the own point of the one live lane of the last tile
        one = pos[:, :n2]
        assert_same(engine_run(one, None, EDGES, [0, 1], BOX, setup=lambda e: e.set_slab_frames(1)),
                    restate(one, None, EDGES, [0, 1], BOX), 3)


@pytest.fixture(scope="module")
def short_walk():
    """9 frames of one set of 65 points and the restatement for lags 0, 1, 3, shared and left unchanged."""
    pos = walk(400, 9, 65)
    want = restate(pos, None, EDGES, [0, 1, 3], BOX)
    assert want[0].sum(axis=-1).all()
    np.testing.assert_array_equal(want[1], [9, 8, 6])
    pos.setflags(write=False)
    want[0].setflags(write=False)
    return pos, want


@pytest.mark.parametrize("slab", [1, 2])
def test_the_ring_wraps_across_two_calls(short_walk, slab):
    """With lags up to 3 the ring holds 3 + slab frames, fewer than the 9 fed as 4 + 5: every slot is written twice
    or more, the second call starts in the middle of the ring, and lag 3 reaches back across the wrap and across the
    calls.  (The split tests below feed 9 frames to a ring of at least 11.)"""
    pos, want = short_walk
    setup = lambda e: e.set_slab_frames(slab)      # noqa: E731
    assert_same(engine_run(pos, None, EDGES, [0, 1, 3], BOX, splits=[0, 4, 9], setup=setup), want, 9)
    assert_same(engine_run(pos, None, EDGES, [0, 1, 3], BOX, setup=setup), want, 9)


@pytest.mark.parametrize("n", [65, T + 1])
def test_self_exclusion_is_the_self_part(n):
    """Two sets of the same rows count the pair i == j as well: at lag 0 that is n * n_origins in the bin that
    holds 0, at the other lags the self van Hove counts of those rows (the box is large, no displacement folds)."""
    F, dims = 9, np.array([200.0, 210.0, 220.0])
    rng = np.random.default_rng(n)
    pos = (rng.uniform(20.0, 60.0, (1, n, 3)) + np.cumsum(rng.normal(0.0, 1.2, (F, n, 3)), axis=0)).astype(np.float32)
    one = engine_run(pos, None, EDGES, LAGS, dims)
    two = engine_run(pos, pos, EDGES, LAGS, dims)
    assert_same(one, restate(pos, None, EDGES, LAGS, dims))
    assert_same(two, restate(pos, pos, EDGES, LAGS, dims))
    diff = two[0] - one[0]
    want0 = np.zeros(len(EDGES) - 1, dtype=np.int64)
    want0[0] = n * F
    np.testing.assert_array_equal(diff[0], want0)
    vh = _core.VanHoveEngine([n], EDGES, LAGS[:5])
    try:
        vh.accumulate(pos)
        self_counts = vh.result()[0][:, 0]
    finally:
        vh.close()
    np.testing.assert_array_equal(diff[:5], self_counts)
    assert (diff[1:5].sum(axis=-1) > 0).all() and diff[1:5, 1:].any() and not diff[5].any()
    assert two[1]["evaluations"] - one[1]["evaluations"] == n * sum(origins(F, lag) for lag in LAGS)


@pytest.mark.parametrize("r_min", [0.0, 0.5])
@pytest.mark.parametrize("n_bins", [1, 2, 201, _core.DistinctVanHoveEngine.LDS_BINS,
                                    _core.DistinctVanHoveEngine.LDS_BINS + 1])
def test_bin_counts_and_a_positive_r_min(n_bins, r_min):
    """LDS_BINS bins are the most the LDS holds; LDS_BINS + 1 are counted in HBM directly."""
    pos = walk(8, 3, 65 + T + 1)
    x1, x2 = pos[:, :65], pos[:, 65:]
    edges = np.linspace(r_min, 15.0, n_bins + 1)
    want = restate(x1, x2, edges, [0, 1, 2], BOX)
    assert_same(engine_run(x1, x2, edges, [0, 1, 2], BOX), want, 3)
    assert (want[0].sum(axis=-1) > 0).all()
    assert_same(engine_run(x2, None, edges, [0, 2], BOX), restate(x2, None, edges, [0, 2], BOX), 3)


def test_exact_arithmetic_on_the_edges():
    """float32 coordinates on a grid of 0.25, box (16, 16, 32), edges = linspace(0, 8, 33): every r below is exact."""
    dims = np.array([16.0, 16.0, 32.0])
    edges = np.linspace(0.0, 8.0, 33)
    moves = np.array([[8.0, 0.0, 0.0],         # s = +0.5 -> rint 0 (ties to even): w = 8 = r_max, the last bin
                      [-8.0, 0.0, 0.0],        # s = -0.5 -> rint -0: w = -8, the last bin
                      [12.0, 0.0, 0.0],        # s = 0.75 -> w = -4: r = 4, bin 16
                      [0.75, 0.0, 0.0],        # r on an inner edge: the bin that starts there
                      [3.0, -4.0, 0.0],        # r = 5, on an edge
                      [0.0, 0.0, 8.25],        # r just above r_max (half of 32 is 16: not folded): not counted
                      [0.0, 4.75, -6.5],       # r = 8.0505...: not counted
                      [0.0, 0.0, 0.0],         # a distinct pair at one place: r = 0, bin 0
                      [0.0, 24.0, 0.25],       # s = 1.5 -> rint 2: w = -8 in y, r = 8.0039...: not counted
                      [0.0, 0.0, -24.0]])      # s = -0.75 -> rint -1: w = 8 in z, the last bin
    origin = np.array([[3.25, 9.5, 20.75]])
    x1 = origin[None].astype(np.float32)
    x2 = (origin + moves)[None].astype(np.float32)
    np.testing.assert_array_equal(x2.astype(np.float64)[0], origin + moves)
    r = distances(x1[0].astype(np.float64), x2[0].astype(np.float64), dims)[0]
    np.testing.assert_array_equal(r[[0, 1, 2, 3, 4, 5, 7, 9]], [8.0, 8.0, 4.0, 0.75, 5.0, 8.25, 0.0, 8.0])
    table = np.zeros(32, dtype=np.int64)
    for b in (31, 31, 16, 3, 20, 0, 31):
        table[b] += 1
    got = engine_run(x1, x2, edges, [0], dims)
    assert_same(got, restate(x1, x2, edges, [0], dims), 1)
    np.testing.assert_array_equal(got[0][0], table)
    # the other way round every d changes sign: the ties still go to even, the table is the same
    back = engine_run(x2, x1, edges, [0], dims)
    assert_same(back, restate(x2, x1, edges, [0], dims), 1)
    np.testing.assert_array_equal(back[0][0], table)
    # all eleven points as one set: against the restatement
    both = np.concatenate((x1, x2), axis=1)
    assert_same(engine_run(both, None, edges, [0], dims), restate(both, None, edges, [0], dims), 1)


@pytest.fixture(scope="module")
def system():
    """Frames, two unequal sets and their restatement, shared and left unchanged."""
    n1, n2, F = 65, T + 1, 9
    pos = walk(11, F, n1 + n2)
    want = restate(pos[:, :n1], pos[:, n1:], EDGES, LAGS, BOX)
    want_one = restate(pos, None, EDGES, LAGS, BOX)
    for a in (pos, want[0], want_one[0]):
        a.setflags(write=False)
    return {"pos": pos, "n1": n1, "n2": n2, "want": want, "want_one": want_one}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(system, axis):
    pos, n1 = system["pos"], system["n1"]
    x1, x2 = pos[:, :n1], pos[:, n1:]
    want = restate(x1, x2, EDGES, LAGS, BOX, zero_dims=1 << axis)
    got = engine_run(x1, x2, EDGES, LAGS, BOX, zero_dims=1 << axis)
    assert_same(got, want, 9)
    assert (want[0][:5].sum(axis=-1) > system["want"][0][:5].sum(axis=-1)).all()     # more pairs inside the range
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    np.testing.assert_array_equal(engine_run(flat[:, :n1], flat[:, n1:], EDGES, LAGS, BOX)[0], got[0])
    one = engine_run(pos, None, EDGES, LAGS, BOX, zero_dims=1 << axis)
    assert_same(one, restate(pos, None, EDGES, LAGS, BOX, zero_dims=1 << axis), 9)


@pytest.mark.parametrize("origin_step", [1, 2, 3, 20])
def test_origin_step(system, origin_step):
    pos, n1, n2 = system["pos"], system["n1"], system["n2"]
    x1, x2 = pos[:, :n1], pos[:, n1:]
    want = restate(x1, x2, EDGES, LAGS, BOX, origin_step=origin_step)
    np.testing.assert_array_equal(want[1], [origins(9, lag, origin_step) for lag in LAGS])
    assert want[2] == want[1].sum() * n1 * n2
    if origin_step == 1:
        np.testing.assert_array_equal(want[0], system["want"][0])
    assert_same(engine_run(x1, x2, EDGES, LAGS, BOX, origin_step=origin_step), want, 9)
    # ... and the same whatever the split into calls and slabs
    assert_same(engine_run(x1, x2, EDGES, LAGS, BOX, origin_step=origin_step, splits=[0, 1, 5, 9],
                           setup=lambda e: e.set_slab_frames(4)), want, 9)
    assert_same(engine_run(pos, None, EDGES, LAGS, BOX, origin_step=origin_step),
                restate(pos, None, EDGES, LAGS, BOX, origin_step=origin_step), 9)


@pytest.mark.parametrize("same", [False, True])
def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, same, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, n1, n2 = system["pos"], system["n1"], system["n2"]
    F, n = pos.shape[:2]
    want = system["want_one" if same else "want"]
    x1, x2 = (pos, None) if same else (pos[:, :n1], pos[:, n1:])

    def check(eng):
        np.testing.assert_array_equal(eng.result(), want[0])
        assert eng.stats()["evaluations"] == want[2] and eng.stats()["frames"] == F

    run = lambda **kw: engine_run(x1, x2, EDGES, LAGS, BOX, **kw)      # noqa: E731
    assert_same(run(), want, F)
    assert_same(run(splits=[0, 1, 5, 9]), want, F)                  # lag 8 spans every call
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want, F)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want, F)
    assert_same(run(splits=[0, 1, 5, 9], setup=lambda e: e.set_slab_frames(4)), want, F)

    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    rng = np.random.default_rng(13)
    n_total = 2 * n + 5
    index = rng.permutation(n_total)[:n]
    assert np.any(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    big = (rng.uniform(0.0, 1.0, (F, n_total, 3)) * BOX).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.tile(BOX, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.DistinctVanHoveEngine(n if same else n1, n if same else n2, EDGES, LAGS, BOX, same=same)
    try:
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.stats()["evaluations"] == 0
        assert not eng.result().any()
        eng.accumulate_traj(tf, np.arange(F))
        check(eng)                                                  # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        check(eng)                                                  # HBM through the index
        with pytest.raises(ValueError, match="out of range"):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        check(eng)                                                  # file through the index
        eng.reset()
        eng.set_slab_frames(4)
        eng.accumulate_device(d.rows(0, 2).ptr, n, 2)               # routes mixed within one pass
        eng.accumulate(pos[2:6])
        eng.accumulate_traj(tf, np.arange(6, F))
        check(eng)
        eng.reset()
        eng.set_slab_frames(0)                                      # the default again
        eng.accumulate(pos)
        check(eng)
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


# ---------------------------------------------------------------- the class

def _shell(edges):
    return 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)


def test_class_routes_groups_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_c, extra, n_a, F = 70, 3, T + 5, 9
    n = n_c + extra + n_a
    pos = walk(20, F, n)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    ia, ib = np.arange(n_c), np.arange(n_c + extra, n)
    lags = np.array([0, 1, 3, 8, 12])
    edges = np.linspace(0.0, 12.0, 25)
    volume = np.prod(BOX)
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)

    def check(v, frames, step, i1, i2, origin_step=1):
        """v.results against the restatement and the formulas on the selected frames."""
        x = pos[frames]
        counts, n_origins, _ = restate(x[:, i1], None if i2 is None else x[:, i2], edges, lags, BOX,
                                       origin_step=origin_step)
        res = v.results
        np.testing.assert_array_equal(res.counts, counts)
        assert res.counts.dtype == np.int64 and res.counts.shape == (5, 24)
        np.testing.assert_array_equal(res.n_origins, n_origins)
        np.testing.assert_array_equal(res.edges, edges)
        np.testing.assert_array_equal(res.bins, (edges[:-1] + edges[1:]) / 2)
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        live = n_origins > 0
        assert live[0] and not live[-1]
        o = n_origins.astype(float)
        o[~live] = np.nan
        vanhove = counts / (o[:, None] * len(i1) * _shell(edges))
        partners = len(i1) - 1 if i2 is None else len(i2)
        np.testing.assert_array_equal(res.vanhove[live], vanhove[live])
        np.testing.assert_array_equal(res.normalized[live], (vanhove * volume / partners)[live])
        assert np.isnan(res.vanhove[~live]).all() and np.isnan(res.normalized[~live]).all()      # no origin: NaN
        assert not res.counts[~live].any()
        # lag 0 is g(r): the pair histogram of the analysed frames themselves
        a = x.astype(np.float64)
        rs = []
        for f in range(0, len(x), origin_step):
            r = distances(a[f][i1], a[f][i1 if i2 is None else i2], BOX)
            rs.append(r[~np.eye(len(i1), dtype=bool)] if i2 is None else r.ravel())
        hist = np.histogram(np.concatenate(rs), 24, (0.0, 12.0))[0]
        g = hist / (float(len(rs)) * len(i1) * _shell(edges)) * volume / partners
        np.testing.assert_array_equal(res.normalized[0], g)
        assert 0.5 < g[-1] < 1.5                                                   # an ideal gas: about 1
        assert set(res.units) == {"results.bins", "results.edges", "results.times", "results.vanhove"}
        assert res.units["results.vanhove"] == "angstrom^-3"

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            # anions at the origin, cations after the lag: not the order of the frame
            def make(u=u, **kw):
                return DistinctVanHove(u.select(ib), u.select(ia), 24, (0.0, 12.0), lags=lags, verbose=False, **kw)

            full = make().run()
            check(full, np.arange(F), 1, ib, ia)
            check(make().run(start=1, stop=9, step=2), np.arange(1, 9, 2), 2, ib, ia)
            check(make().run(frames=[2, 5, 8]), np.array([2, 5, 8]), 3, ib, ia)
            check(make(origin_step=2).run(), np.arange(F), 1, ib, ia, origin_step=2)
            one = DistinctVanHove(u.select(ib), None, 24, (0.0, 12.0), lags=lags, verbose=False).run()
            check(one, np.arange(F), 1, ib, None)
            again = DistinctVanHove(u.select(ib), u.select(ib), 24, (0.0, 12.0), lags=lags, verbose=False).run()
            for key in ("counts", "vanhove", "normalized"):                         # ag2 equal to ag1 is ag2=None
                np.testing.assert_array_equal(again.results[key], one.results[key])
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in ("counts", "vanhove", "normalized"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # every particle in order (no index), and neither lags nor n_lags: every analysed frame is a lag
        whole = DistinctVanHove(u.atoms, None, 24, (0.0, 12.0), verbose=False).run()
        counts, n_origins, _ = restate(pos, None, edges, np.arange(F), BOX)
        np.testing.assert_array_equal(whole.results.counts, counts)
        np.testing.assert_array_equal(whole.results.n_origins, n_origins)
        np.testing.assert_array_equal(
            DistinctVanHove(u.atoms, n_bins=24, range=(0.0, 12.0), n_lags=4, verbose=False).run().results.counts,
            counts[:4])
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(DistinctVanHove(u.select(ib), u.select(ia), 24, (0.0, 12.0), lags=lags,
                                         verbose=False)).run()
        np.testing.assert_array_equal(slow.results.counts, results["host"].counts)
        np.testing.assert_array_equal(slow.results.normalized, results["host"].normalized)
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = DistinctVanHove(u.select(ib), u.select(ia), 24, (0.0, 12.0), lags=lags, dimensions=wide,
                                verbose=False).run()
        np.testing.assert_array_equal(other.results.counts, restate(pos[:, ib], pos[:, ia], edges, lags, wide)[0])
        assert (other.results.counts != results["host"].counts).any()
    finally:
        d.free()


def test_class_drop_axis(system):
    pos = system["pos"]
    n, F = pos.shape[1], len(pos)
    u = mdhelper_amd.ArrayUniverse(pos, [*BOX, 90.0, 90.0, 90.0])
    lags = np.array(LAGS)
    counts, n_origins, _ = restate(pos, None, EDGES, LAGS, BOX, zero_dims=4)
    flat = DistinctVanHove(u.atoms, None, 201, (0.0, 15.0), lags=LAGS, drop_axis="z", verbose=False).run()
    np.testing.assert_array_equal(flat.results.counts, counts)
    live = lags < F
    o = n_origins.astype(float)
    o[~live] = np.nan
    ring = np.pi * (EDGES[1:] ** 2 - EDGES[:-1] ** 2)
    vanhove = counts / (o[:, None] * n * ring)
    np.testing.assert_array_equal(flat.results.vanhove[live], vanhove[live])
    np.testing.assert_array_equal(flat.results.normalized[live], (vanhove * (BOX[0] * BOX[1]) / (n - 1))[live])
    assert np.isnan(flat.results.vanhove[~live]).all() and np.isnan(flat.results.normalized[~live]).all()
    assert flat.results.units["results.vanhove"] == "angstrom^-2"
    # with x dropped the shortest length that takes part is 44.5: a range up to 22 is allowed
    far = DistinctVanHove(u.atoms, None, 44, (0.0, 22.0), lags=[0, 3], drop_axis="x", verbose=False).run()
    np.testing.assert_array_equal(far.results.counts,
                                  restate(pos, None, np.linspace(0.0, 22.0, 45), [0, 3], BOX, zero_dims=1)[0])
