"""
Host-side checks of the hydrogen-bond analysis that need no GPU: the argument handling of
``analysis.hbond.HydrogenBonds``, what ``_prepare`` derives (the feed index and the three tables, times, origins), the
thresholds of both histograms, and the argument errors of the engine, which are raised before any device is touched (a
handle touches its device with the first frame).

Not reachable without a device, and therefore checked in ``test_gpu_hydrogen_bonds.py``: ``set_bins`` and
``set_slab_frames`` after the first frame and a row beyond ``max_neighbors`` (there is no first frame without a
device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from hydrogen_bond_cases import BOX, DISTANCE, F, LAGS, cos_of, restate, water, water_tables
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import HydrogenBonds, hbond


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


def _groups(u):
    """Four waters O H H: donors, hydrogens, acceptors."""
    o = 3 * np.arange(4)
    return u.select(np.repeat(o, 2)), u.select(np.stack((o + 1, o + 2), axis=1).ravel()), u.select(o)


def test_constructor_errors():
    u = _universe()
    d, h, a = _groups(u)
    assert mdhelper_amd.analysis.HydrogenBonds is hbond.HydrogenBonds
    with pytest.raises(ValueError, match="'donors' holds 7 atoms and 'hydrogens' 8"):
        HydrogenBonds(u.select(np.repeat(3 * np.arange(4), 2)[:7]), h, a)
    with pytest.raises(ValueError, match="its own donor"):
        HydrogenBonds(u.select([0, 2]), u.select([1, 2]), a)
    with pytest.raises(ValueError, match="a hydrogen is no acceptor"):
        HydrogenBonds(d, h, u.select([0, 3, 4]))
    with pytest.raises(ValueError, match="'hydrogens' holds an atom twice"):
        HydrogenBonds(u.select([0, 3]), u.select([1, 1]), a)
    with pytest.raises(ValueError, match="'acceptors' holds an atom twice"):
        HydrogenBonds(d, h, u.select([0, 3, 0]))
    with pytest.raises(ValueError, match="at least one atom"):
        HydrogenBonds(d, h, u.select(np.zeros(0, dtype=int)))
    for angle in (-0.5, 180.5, np.nan):
        with pytest.raises(ValueError, match="'angle' must lie in \\[0, 180\\]"):
            HydrogenBonds(d, h, a, angle=angle)
    for distance in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="'distance' must be positive and finite"):
            HydrogenBonds(d, h, a, distance=distance)
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        HydrogenBonds(d, h, a, distance=20.5)                                   # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        HydrogenBonds(d, h, a, distance=3.0, dimensions=[5.9, 60.0, 60.0])
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        HydrogenBonds(d, h, a, distance=21.5, drop_axis="z")                    # x is still 40
    HydrogenBonds(d, h, a, distance=20.0)                                       # exactly half is allowed
    HydrogenBonds(d, h, a, distance=21.0, drop_axis="x")                        # x dropped: 42 / 2 = 21
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        HydrogenBonds(d, h, a, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        HydrogenBonds(d, h, a, lags=[-1, 0])
    with pytest.raises(ValueError, match="array of integers"):
        HydrogenBonds(d, h, a, lags=[0.5, 1.0])
    with pytest.raises(ValueError, match="cannot both be given"):
        HydrogenBonds(d, h, a, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="'n_lags' must be at least 1"):
        HydrogenBonds(d, h, a, n_lags=0)
    with pytest.raises(ValueError, match="'origin_step' must be at least 1"):
        HydrogenBonds(d, h, a, origin_step=0)
    for slots in (0, 65, -3):
        with pytest.raises(ValueError, match="'max_neighbors' must lie in \\[1, 64\\]"):
            HydrogenBonds(d, h, a, max_neighbors=slots)
    HydrogenBonds(d, h, a, max_neighbors=1)
    HydrogenBonds(d, h, a, max_neighbors=64)
    for kw in (dict(n_distance_bins=0), dict(n_angle_bins=0)):
        with pytest.raises(ValueError, match="must be at least 1"):
            HydrogenBonds(d, h, a, **kw)
    with pytest.raises(ValueError, match="not strictly decreasing"):
        HydrogenBonds(d, h, a, angle=180.0)                                     # no room for a bin
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        HydrogenBonds(d, h, a, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        HydrogenBonds(d, h, a, drop_axis=3)
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        HydrogenBonds(*_groups(_universe(dims=None)))
    with pytest.raises(ValueError, match="orthorhombic"):
        HydrogenBonds(*_groups(_universe(angles=(90.0, 90.0, 60.0))))
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            HydrogenBonds(d, h, a, comm=TwoRanks(rank))
    v = HydrogenBonds(d, h, a)
    assert (v._distance, v._angle, v._max_neighbors, v._continuous, v._origin_step) == (3.0, 150.0, 8, True, 1)
    assert v._cos_max == cos_of(150.0) and v._shard_frames is False
    assert len(v._distance_edges) == len(v._angle_edges) == 61
    with pytest.raises(RuntimeError, match="run\\(\\)"):
        v.calculate_lifetimes()
    with pytest.raises(ValueError, match="molecules of equal size"):
        HydrogenBonds.from_molecules(u.atoms, 5)
    with pytest.raises(ValueError, match="places must lie in \\[0, 3\\)"):
        HydrogenBonds.from_molecules(u.atoms, 4, donors=[(0, 3)])
    with pytest.raises(ValueError, match="places must lie in \\[0, 3\\)"):
        HydrogenBonds.from_molecules(u.atoms, 4, acceptors=[-1])


def _run_until_the_device(v, **kwargs):
    """``run()`` up to the point where the device is asked for: everything ``_prepare`` derives from the arguments
    is in place by then."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            v.run(**kwargs)
    else:
        v.run(**kwargs)
    return v


def test_the_feed_index_and_the_three_tables():
    u = _universe(n_atoms=14)
    # a three-site water by from_molecules: the feed is the twelve atoms in order
    v = HydrogenBonds.from_molecules(u.select(np.arange(12)), 4)
    np.testing.assert_array_equal(v._index, np.arange(12))
    np.testing.assert_array_equal(v._h_row, [1, 2, 4, 5, 7, 8, 10, 11])
    np.testing.assert_array_equal(v._d_row, [0, 0, 3, 3, 6, 6, 9, 9])
    np.testing.assert_array_equal(v._a_row, [0, 3, 6, 9])
    assert v._h_row.dtype == v._d_row.dtype == v._a_row.dtype == np.int32 and (v._n_h, v._n_a) == (8, 4)
    # the same from the groups given by hand
    w = HydrogenBonds(*_groups(u))
    for key in ("_index", "_h_row", "_d_row", "_a_row"):
        np.testing.assert_array_equal(getattr(w, key), getattr(v, key))
    # other places inside a molecule of four: one donor with one hydrogen, two acceptors that are no donors
    m = HydrogenBonds.from_molecules(u.select(np.arange(2, 14)), 3, donors=[(3, 0)], acceptors=[1, 2])
    np.testing.assert_array_equal(m._index, np.arange(2, 14))
    np.testing.assert_array_equal(m._h_row, [0, 4, 8])
    np.testing.assert_array_equal(m._d_row, [3, 7, 11])
    np.testing.assert_array_equal(m._a_row, [1, 2, 5, 6, 9, 10])
    # hand-given groups in no order, a repeated donor, atoms that take no part: the distinct atoms are fed once,
    # ascending, and the tables name them by their place in the feed
    g = HydrogenBonds(u.select([9, 9, 2]), u.select([13, 4, 7]), u.select([11, 9, 0]))
    np.testing.assert_array_equal(g._index, [0, 2, 4, 7, 9, 11, 13])
    np.testing.assert_array_equal(g._h_row, [6, 2, 3])
    np.testing.assert_array_equal(g._d_row, [4, 4, 1])
    np.testing.assert_array_equal(g._a_row, [5, 4, 0])
    np.testing.assert_array_equal(g._index[g._h_row], [13, 4, 7])
    np.testing.assert_array_equal(g._index[g._d_row], [9, 9, 2])
    np.testing.assert_array_equal(g._index[g._a_row], [11, 9, 0])


def test_prepare_errors_times_and_origins():
    u = _universe()
    make = lambda **kw: HydrogenBonds(*_groups(u), verbose=False, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        make().run(frames=[0, 1, 3])
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        make().run(frames=[4, 2, 0])
    v = _run_until_the_device(make(lags=[0, 1, 2, 5]), step=3)
    assert v.n_frames == 3
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [3, 2, 1, 0])
    assert v.results.units["results.times"] == v.results.units["results.lifetime"] == "picosecond"
    assert v.results.units["results.angle_bins"] == "degree" and v.results.units["results.distance_bins"] == "angstrom"
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument; every second frame an origin
    v = _run_until_the_device(make(dt=2.0, drop_axis="x", origin_step=2))
    np.testing.assert_array_equal(v.results.times, np.arange(7) * 2.0)
    np.testing.assert_array_equal(v.results.n_origins, [4, 3, 3, 2, 2, 1, 1])     # origins 0, 2, 4, 6 below 7 - lag
    v = _run_until_the_device(make(lags=[0, 1, 4, 9], origin_step=3), frames=[0, 2, 4, 6])
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 4, 9]) * 2 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [2, 1, 0, 0])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            HydrogenBonds(*_groups(_universe()), verbose=False).run()
        eng = _core.HydrogenBondEngine(12, *water_tables(4), 3.0, -0.5, [0, 1], [10.0, 10.0, 10.0])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        with pytest.raises(RuntimeError):
            eng.geometry()
        eng.close()


# ---------------------------------------------------------------- thresholds

@pytest.mark.parametrize("distance, n_bins", [(3.5, 60), (3.0, 1), (3.0, 7), (2.75, 513), (0.1, 60), (19.3, 1000)])
def test_r2_thresholds_reproduce_numpy_histogram_of_the_distance(distance, n_bins):
    edges = np.linspace(0.0, distance, n_bins + 1)
    t = hbond.distance_thresholds(edges)
    assert t[0] == 0.0 and np.all(np.diff(t) > 0)
    with np.errstate(invalid="ignore"):
        assert np.all(np.sqrt(t) >= edges) and not np.any(np.sqrt(np.nextafter(t, -np.inf)) >= edges)
    # values one ulp either side of every edges[b] ** 2, and the square itself
    sq = edges * edges
    x = np.concatenate((sq, np.nextafter(sq, np.inf), np.nextafter(sq[1:], -np.inf), t, np.nextafter(t[1:], -np.inf)))
    x = x[np.sqrt(x) <= distance]                       # what a bond can have: r2 <= distance * distance
    assert len(x) >= 3 * n_bins
    from hydrogen_bond_cases import bin_up
    got = np.bincount(bin_up(x, t), minlength=n_bins)
    np.testing.assert_array_equal(got, np.histogram(np.sqrt(x), edges)[0])
    # the largest r2 of a bond, distance * distance itself, lies in the last bin
    assert bin_up([np.float64(distance) * np.float64(distance)], t)[0] == n_bins - 1


@pytest.mark.parametrize("n_bins", [1, 60, 180])
@pytest.mark.parametrize("angle", [90.0, 120.0, 150.0])
def test_cosine_thresholds_are_strictly_decreasing(angle, n_bins):
    u = _universe()
    v = HydrogenBonds(*_groups(u), angle=angle, n_angle_bins=n_bins, n_distance_bins=3)
    t = v._cos_thresholds
    assert len(t) == n_bins + 1 and np.all(np.diff(t) < 0)
    assert t[0] == v._cos_max == cos_of(angle) and t[-1] == -1.0
    np.testing.assert_array_equal(v._angle_edges, np.linspace(angle, 180.0, n_bins + 1))
    np.testing.assert_array_equal(t, np.cos(np.deg2rad(v._angle_edges)))
    np.testing.assert_array_equal(v._r2_thresholds, hbond.distance_thresholds(np.linspace(0.0, 3.0, 4)))


# ---------------------------------------------------------------- the restatement

def test_the_restatement_gives_the_figures_it_was_checked_with():
    """The cases of the GPU tests are not vacuous: bonds in every frame, the two lifetime functions apart from lag 2
    on, rows within the cap."""
    h, d, a = water_tables(257)
    pos = water(357, F, 257, BOX)
    want = restate(pos, h, d, a, DISTANCE, cos_of(150.0), LAGS, BOX)
    assert (want["bonds"].min(), want["bonds"].max(), want["max_row"]) == (66, 85, 3)
    np.testing.assert_array_equal(want["intermittent"], [921, 495, 352, 146, 54, 15, 0])
    np.testing.assert_array_equal(want["continuous"], [921, 495, 290, 61, 8, 0, 0])
    assert want["evaluations"] == F * (514 * 257 - 514) and want["degenerate"] == 0
    wide = restate(pos, h, d, a, DISTANCE, cos_of(120.0), LAGS, BOX)
    assert (wide["bonds"].min(), wide["bonds"].max(), wide["max_row"], wide["continuous"][5]) == (314, 364, 5, 49)
    small = restate(water(228, F, 128, BOX), *water_tables(128), DISTANCE, cos_of(150.0), LAGS, BOX)
    assert (small["bonds"].min(), small["bonds"].max(), small["max_row"]) == (13, 24, 2)


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]
H_ROW, D_ROW, A_ROW = [1, 2, 4], [0, 0, 3], [0, 3, 5]


def _engine(**kwargs):
    args = dict(n_rows=6, h_row=H_ROW, d_row=D_ROW, a_row=A_ROW, distance=3.0, cos_max=-0.5, lags=[0, 1, 4], dims=DIMS,
                origin_step=1, zero_dims=0, max_neighbors=8, continuous=True)
    args.update(kwargs)
    return _core.HydrogenBondEngine(
        args["n_rows"], args["h_row"], args["d_row"], args["a_row"], args["distance"], args["cos_max"], args["lags"],
        args["dims"], origin_step=args["origin_step"], zero_dims=args["zero_dims"],
        max_neighbors=args["max_neighbors"], continuous=args["continuous"])


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(distance=0.0), "distance must be positive and finite"),
                         (dict(distance=-2.0), "distance must be positive and finite"),
                         (dict(distance=np.nan), "distance must be positive and finite"),
                         (dict(distance=np.inf), "distance must be positive and finite"),
                         (dict(distance=5.5), "distance 5.5 reaches beyond half the shortest box length 10"),
                         (dict(dims=[5.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 11.0, 5.9], zero_dims=3), "beyond half the shortest box length"),
                         (dict(distance=5.5, zero_dims=2), "beyond half the shortest box length"),
                         (dict(cos_max=1.5), "cos_max must lie in \\[-1, 1\\]"),
                         (dict(cos_max=-1.0000001), "cos_max must lie in \\[-1, 1\\]"),
                         (dict(cos_max=np.nan), "cos_max must lie in \\[-1, 1\\]"),
                         (dict(max_neighbors=0), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(max_neighbors=65), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(lags=[]), "at least one lag"),
                         (dict(lags=[-1, 0]), "not be negative"),
                         (dict(lags=[0, 2, 2]), "strictly increasing"),
                         (dict(lags=[3, 1]), "strictly increasing"),
                         (dict(origin_step=0), "origin_step must be at least 1"),
                         (dict(zero_dims=7), "at least one component"),
                         (dict(zero_dims=-1), "at least one component"),
                         (dict(h_row=[], d_row=[]), "at least one hydrogen and one acceptor"),
                         (dict(a_row=[]), "at least one hydrogen and one acceptor"),
                         (dict(h_row=[1, 2]), "of one length"),
                         (dict(h_row=[1, 2, 6]), "h_row\\[2\\] = 6 out of range \\[0, 6\\)"),
                         (dict(h_row=[-1, 2, 4]), "h_row\\[0\\] = -1 out of range"),
                         (dict(d_row=[0, 7, 3]), "d_row\\[1\\] = 7 out of range"),
                         (dict(a_row=[0, 3, 6]), "a_row\\[2\\] = 6 out of range"),
                         (dict(h_row=[1, 1, 4]), "row 1 is a hydrogen twice"),
                         (dict(a_row=[0, 3, 3]), "row 3 is an acceptor twice"),
                         (dict(a_row=[0, 2, 5]), "row 2 is both a hydrogen and an acceptor"),
                         (dict(d_row=[0, 2, 3]), "hydrogen 1 \\(row 2\\) is its own donor"),
                         (dict(n_rows=0), "2\\^31 / 3"),
                         (dict(n_rows=2 ** 31 // 3), "2\\^31 / 3"),
                         (dict(dims=[10.0, 0.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, np.nan, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0]), "three box lengths")):
        with pytest.raises(ValueError, match=word):
            _engine(**kwargs)
    # half the shortest kept length itself is allowed, and a dropped component does not count; the ends of cos_max
    _engine(distance=5.0).close()
    _engine(distance=5.5, zero_dims=1).close()
    _engine(cos_max=1.0, max_neighbors=1).close()
    _engine(cos_max=-1.0, max_neighbors=64, continuous=False).close()
    _engine(d_row=[3, 5, 5]).close()                    # a donor may repeat and may be an acceptor
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    hr, dr, ar = (np.array(t, dtype=np.int32) for t in (H_ROW, D_ROW, A_ROW))
    lag0, dims = np.array([0], dtype=np.int64), np.array(DIMS)
    create = lambda *a: lib.mdx_hb_create(ctypes.byref(h), 0, *a)      # noqa: E731
    good = (6, 3, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 1, p(lag0), 1, p(dims), 0, 8, 1)
    assert create(*good) == 0
    assert lib.mdx_hb_destroy(h) == 0
    for at in (2, 3, 5, 9, 11):
        args = list(good)
        args[at] = None
        assert create(*args) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_create(None, 0, *good) == -1 and b"NULL" in lib.mdx_last_error()
    assert create(6, 0, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 1, p(lag0), 1, p(dims), 0, 8, 1) == -1
    assert b"at least one hydrogen" in lib.mdx_last_error()
    assert create(6, 3, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 0, p(lag0), 1, p(dims), 0, 8, 1) == -1
    assert b"at least one lag" in lib.mdx_last_error()
    assert create(6, 3, p(hr), p(dr), 3, p(ar), 5.25, -0.5, 1, p(lag0), 1, p(dims), 0, 8, 1) == -1
    assert b"distance 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(6, 3, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 1, p(lag0), 1, p(dims), 0, 65, 1) == -1
    assert b"max_neighbors" in lib.mdx_last_error()
    assert create(2 ** 31 // 3, 3, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 1, p(lag0), 1, p(dims), 0, 8, 1) == -1
    assert b"2^31 / 3" in lib.mdx_last_error()
    assert create(6, 2 ** 31 // 3, p(hr), p(dr), 3, p(ar), 3.0, -0.5, 1, p(lag0), 1, p(dims), 0, 8, 1) == -1
    assert b"2^31 / 3" in lib.mdx_last_error()
    for call in (lib.mdx_hb_reset, lib.mdx_hb_synchronize):
        assert call(None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_set_bins(None, 1, None, 1, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_result(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_geometry(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_bonds(None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_hb_destroy(None) == 0
    assert (_core.HydrogenBondEngine.TILE, _core.HydrogenBondEngine.JCHUNK,
            _core.HydrogenBondEngine.MAX_NEIGHBORS) == (256, 1024, 64)


def test_set_bins_errors_need_no_device():
    eng = _engine()
    lib = _lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    up, down = np.array([0.0, 1.0, 4.0, 9.0]), np.array([-0.5, -0.7, -0.9, -1.0])
    try:
        for r, c, word in (([0.0, 1.0, 1.0, 9.0], down,
                            "r2_thresholds must be strictly increasing: \\[1\\] = 1, \\[2\\] = 1"),
                           ([0.0, 4.0, 1.0, 9.0], down, "r2_thresholds must be strictly increasing"),
                           (up[::-1], down, "r2_thresholds must be strictly increasing"),
                           ([0.0, np.nan, 9.0], down, "r2_thresholds must be strictly increasing"),
                           (up, [-0.5, -0.7, -0.7, -1.0], "cos_thresholds must be strictly decreasing: \\[1\\] = -0.7"),
                           (up, down[::-1], "cos_thresholds must be strictly decreasing"),
                           (up, [-0.5, np.nan], "cos_thresholds must be strictly decreasing"),
                           ([1.0], down, "at least two"),
                           (up, [[-0.5, -1.0]], "at least two")):
            with pytest.raises(ValueError, match=word):
                eng.set_bins(r, c)
        assert (eng.n_distance_bins, eng.n_cosine_bins) == (1, 1)          # a refused table changes nothing
        assert lib.mdx_hb_set_bins(eng.handle, 3, None, 3, p(down)) == -1 and b"NULL" in lib.mdx_last_error()
        assert lib.mdx_hb_set_bins(eng.handle, 3, p(up), 3, None) == -1 and b"NULL" in lib.mdx_last_error()
        assert lib.mdx_hb_set_bins(eng.handle, 0, p(up), 3, p(down)) == -1 and b"n_r and n_c" in lib.mdx_last_error()
        assert lib.mdx_hb_set_bins(eng.handle, 3, p(up), 2 ** 20 + 1, p(down)) == -1
        assert b"n_r and n_c" in lib.mdx_last_error()
        eng.set_bins(up, down)
        assert (eng.n_distance_bins, eng.n_cosine_bins) == (3, 3)
        eng.set_bins(up[:2], down[:3])                                      # more than once, before the first frame
        assert (eng.n_distance_bins, eng.n_cosine_bins) == (1, 2)
    finally:
        eng.close()


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _engine(origin_step=2, zero_dims=2)
    one = _engine(max_neighbors=4, continuous=False)
    try:
        assert (two.n_rows, two.n_h, two.n_a, two.n_lags, two.max_neighbors, two.continuous) == (6, 3, 3, 3, 8, True)
        assert (one.n_rows, one.n_h, one.n_a, one.n_lags, one.max_neighbors, one.continuous) == (6, 3, 3, 3, 4, False)
        for eng in (two, one):
            with pytest.raises(ValueError, match="5 rows given, the tables hold 6"):
                eng.accumulate(np.zeros((2, 5, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="12 rows given, the tables hold 6"):
                eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="7 rows given, the tables hold 6"):
                eng.accumulate_device(rows, 7, 2)
            with pytest.raises(ValueError, match="4 rows given, the tables hold 6"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
            with pytest.raises(ValueError, match="index 7 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 4, 7])
            with pytest.raises(ValueError, match="index -1 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, -1, 3, 4, 5])
            for frames in (-1, 32769):
                with pytest.raises(ValueError, match="frames must lie in"):
                    eng.set_slab_frames(frames)
            out = np.zeros(3, dtype=np.int64)
            assert _lib.lib().mdx_hb_bonds(eng.handle, out.ctypes.data_as(ctypes.c_void_p), 3) == -1
            assert b"3 frames asked for, 0 seen" in _lib.lib().mdx_last_error()
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            eng.reset()
            eng.synchronize()
            eng.set_slab_frames(0)
            eng.synchronize()
            eng.reset()
            assert len(eng.bonds()) == 0
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "max_row": 0,
                                   "degenerate": 0}
    finally:
        two.close()
        one.close()
