"""
HydrogenBonds / HydrogenBondEngine on the GPU against the float64 NumPy restatement of the device contract
(``hydrogen_bond_cases.py``, csrc/mdx_hbond_device.hpp).

No tolerance anywhere: the results are integers, the restatement does one float64 operation at a time, as the device
does, so every comparison is ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from hydrogen_bond_cases import (BOX, DISTANCE, F, KEYS, LAGS, assert_same, bin_down, collect, cos_of, frame_geometry,
                                 restate, water, water_tables)
from mdhelper_amd import _core
from mdhelper_amd.analysis import HydrogenBonds, calculate_residence_time
from mdhelper_amd.analysis.hbond import distance_thresholds

pytestmark = pytest.mark.gpu

T = _core.HydrogenBondEngine.TILE
J = _core.HydrogenBondEngine.JCHUNK
COS150, COS120 = cos_of(150.0), cos_of(120.0)


def bins_of(distance, angle, n_r, n_c):
    """``(edges, r2_thresholds, cos_thresholds)`` as the class forms them."""
    edges = np.linspace(0.0, distance, n_r + 1)
    cos_t = np.cos(np.deg2rad(np.linspace(angle, 180.0, n_c + 1)))
    assert np.all(np.diff(cos_t) < 0)
    return edges, distance_thresholds(edges), cos_t


def engine_run(pos, tables, distance, cos_max, lags, dims, *, splits=None, setup=None, bins=None, **kwargs):
    """One pass over the frames, host route: what ``restate`` returns."""
    eng = _core.HydrogenBondEngine(pos.shape[1], *tables, distance, cos_max, lags, dims, **kwargs)
    try:
        if bins is not None:
            eng.set_bins(*bins)
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def freeze(want):
    for value in want.values():
        if isinstance(value, np.ndarray):
            value.setflags(write=False)
    return want


@pytest.fixture(scope="module")
def system():
    """257 waters over 12 frames, the thresholds of 60 + 60 bins and the restatement, shared and left unchanged."""
    n_mol = 257
    pos = water(100 + n_mol, F, n_mol, BOX)
    tables = water_tables(n_mol)
    edges, r2_t, cos_t = bins_of(DISTANCE, 150.0, 60, 60)
    want = restate(pos, *tables, DISTANCE, COS150, LAGS, BOX, r2_thresholds=r2_t, cos_thresholds=cos_t)
    # not vacuous: bonds in every frame, the two functions apart from lag 2 on, rows within the default cap
    assert want["bonds"].min() == 66 and want["bonds"].max() == 85 and want["max_row"] == 3
    np.testing.assert_array_equal(want["intermittent"], [921, 495, 352, 146, 54, 15, 0])
    np.testing.assert_array_equal(want["continuous"], [921, 495, 290, 61, 8, 0, 0])
    pos.setflags(write=False)
    return {"pos": pos, "tables": tables, "edges": edges, "bins": (r2_t, cos_t), "want": freeze(want)}


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n_h", sorted({1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 2}))
def test_sizes_and_frame_counts(system, n_h):
    """The first n_h hydrogens of the water (an odd number splits a molecule) against all 257 oxygens."""
    pos = system["pos"]
    h_row, d_row, a_row = system["tables"]
    tables = (h_row[:n_h], d_row[:n_h], a_row)
    for frames in (1, 2, 12):
        want = restate(pos[:frames], *tables, DISTANCE, COS150, LAGS, BOX)
        assert want["evaluations"] == frames * (n_h * 257 - n_h)
        if n_h >= 63:
            assert want["bonds"].sum() > 0
        got = engine_run(pos[:frames], tables, DISTANCE, COS150, LAGS, BOX)
        assert_same(got, want)
        for key in KEYS:
            assert got[key][-1] == 0                                # lag 13 never has an origin
            assert not got[key][np.array(LAGS) >= frames].any()
    if n_h == 2 * T + 2:
        for key in KEYS + ("bonds",):
            np.testing.assert_array_equal(got[key], system["want"][key])


@pytest.mark.parametrize("n_a", [J - 1, J, J + 1])
def test_acceptors_around_one_chunk_and_rings_that_wrap_inside_one_call(n_a):
    """T + 1 hydrogens, each with a donor of its own, against n_a points that are no donors; the last acceptor is put
    on the axis of the first hydrogen, so that the last entry of a chunk (or the only one of a second chunk) bonds.
    Lags 0 and 1 with slabs of one frame: the rings hold two frames and wrap inside the one call."""
    frames, n_mol = 4, T + 1
    w = water(7, frames, n_mol, BOX).reshape(frames, n_mol, 3, 3)
    rng = np.random.default_rng(n_a)
    pts = rng.uniform(0.0, 1.0, (1, n_a, 3)) * BOX + np.cumsum(rng.normal(0.0, 0.1, (frames, n_a, 3)), axis=0)
    o, h = w[:, 0, 0].astype(np.float64), w[:, 0, 1].astype(np.float64)
    axis = h - o
    axis -= BOX * np.rint(axis / BOX)
    pts[:, -1] = o + 2.75 * axis
    pts = (pts - np.floor(pts / BOX) * BOX).astype(np.float32)
    pts[pts >= BOX.astype(np.float32)] = 0.0
    pos = np.concatenate((w[:, :, 0], w[:, :, 1], pts), axis=1)          # donors, hydrogens, acceptors
    tables = (np.arange(n_mol, 2 * n_mol), np.arange(n_mol), np.arange(2 * n_mol, 2 * n_mol + n_a))
    want = restate(pos, *tables, DISTANCE, COS150, [0, 1], BOX, max_neighbors=16)
    assert want["bond"][:, 0, -1].all() and want["bonds"].min() > 100 and want["max_row"] <= 16
    assert want["evaluations"] == frames * n_mol * n_a                  # no donor among the acceptors
    assert 0 < want["continuous"][1] < want["origin_counts"][1]
    got = engine_run(pos, tables, DISTANCE, COS150, [0, 1], BOX, max_neighbors=16,
                     setup=lambda e: e.set_slab_frames(1))
    assert_same(got, want)


@pytest.fixture(scope="module")
def short_walk():
    """9 frames of 65 waters in a box of half the lengths (about twenty bonds a frame), the first 65 hydrogens, and the
    restatement for lags 0, 1, 3, shared and left unchanged."""
    box = BOX / 2
    pos = water(400, 9, 65, box)
    h_row, d_row, a_row = water_tables(65)
    tables = (h_row[:65], d_row[:65], a_row)
    want = restate(pos, *tables, DISTANCE, COS150, [0, 1, 3], box)
    assert want["continuous"].all() and want["continuous"][2] < want["intermittent"][2] < want["origin_counts"][2]
    assert want["bonds"].min() >= 10
    pos.setflags(write=False)
    return pos, tables, box, freeze(want)


@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("slab", [1, 2])
def test_the_rings_wrap_across_two_calls(short_walk, slab, continuous):
    """With lags up to 3 the rings hold 3 + slab frames, fewer than the 9 fed as 4 + 5: every slot of the lists and
    of the alive masks is emptied and written twice or more, the second call starts in the middle of the rings, and
    lag 3 reaches back across the wrap and across the calls.  (The split tests below feed 12 frames to rings of at
    least 14.)"""
    pos, tables, box, want = short_walk

    def run(**kw):
        return engine_run(pos, tables, DISTANCE, COS150, [0, 1, 3], box, continuous=continuous,
                          setup=lambda e: e.set_slab_frames(slab), **kw)

    assert_same(run(splits=[0, 4, 9]), want, continuous=continuous)
    assert_same(run(), want, continuous=continuous)


def _three_rows(cases, dims):
    """float32 ``[len(cases), 3, 3]``: rows D, H, A of one frame per case ``(D, H - D, A - D)``, wrapped into the box
    (exact on the grid)."""
    pos = np.array([[d, np.add(d, h), np.add(d, a)] for d, h, a in cases], dtype=np.float64)
    pos -= np.floor(pos / dims) * dims
    out = pos.astype(np.float32)
    np.testing.assert_array_equal(out.astype(np.float64), pos)
    return out


def test_exact_arithmetic_on_the_cutoff_and_on_the_angle():
    """float32 coordinates on a grid of 0.25 (the hydrogens of the distance table on one of 0.0625), box (16, 16, 32):
    every r2, dot and c below is exact.  One D-H and one acceptor per frame, so bonds[f] is the rule for that triple;
    the tables are written out by hand."""
    dims = np.array([16.0, 16.0, 32.0])
    tables = ([1], [0], [2])
    o = (3.25, 9.5, 20.75)
    # distance 5, a wide angle (the hydrogen a quarter of the way along w_DA: c = -1 or next to it)
    cases = [(o, (0.75, -1.0, 0.0), (3.0, -4.0, 0.0)),          # r2_DA = 25 == rc2: a bond
             (o, (0.75, -1.0, 0.0), (3.0, -4.0, 0.25)),         # one grid step outside: r2_DA = 25.0625
             (o, (1.0, 0.0, 0.0), (5.25, 0.0, 0.0)),            # one grid step outside along x
             (o, (1.0, 0.0, 0.0), (8.0, 0.0, 0.0)),             # s = +0.5 -> rint 0 (ties to even): w = 8, r2 = 64
             (o, (-1.0, 0.0, 0.0), (-8.0, 0.0, 0.0)),           # s = -0.5 -> rint -0: w = -8
             (o, (-0.75, 1.0, 0.0), (13.0, 4.0, 0.0)),          # s = 0.8125 -> w = -3 in x: folded onto the cutoff
             (o, (0.0, 0.0, 1.0), (0.0, 0.0, -27.0)),           # s = -0.84375 -> w = 5 in z: folded onto the cutoff
             (o, (0.0, 0.0, -1.0), (0.0, 0.0, 26.75)),          # w = -5.25 in z: one grid step outside after the fold
             # D at x = 0.25, H at 15.25 beyond the face: D - H = -15 -> w_HD = +1; without the minimum image of
             # D - H the cosine would be +1 and the bond lost
             ((0.25, 9.5, 20.75), (-1.0, 0.0, 0.0), (-3.0, 0.0, 0.0)),
             (o, (-1.0, 0.0, 0.0), (3.0, 0.0, 0.0))]            # the hydrogen points away: c = +1
    table = np.array([1, 0, 0, 0, 0, 1, 1, 0, 1, 0], dtype=np.int64)
    pos = _three_rows(cases, dims)
    want = restate(pos, *tables, 5.0, -0.5, [0], dims)
    np.testing.assert_array_equal(want["bonds"], table)
    got = engine_run(pos, tables, 5.0, -0.5, [0], dims)
    assert_same(got, want)
    np.testing.assert_array_equal(got["bonds"], table)
    assert got["intermittent"][0] == got["continuous"][0] == got["origin_counts"][0] == 4 and got["degenerate"] == 0
    # distance 8, half the box: after the tie the pairs at +-8 along x lie exactly on it
    table8 = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0], dtype=np.int64)
    got = engine_run(pos, tables, 8.0, -0.5, [0], dims)
    assert_same(got, restate(pos, *tables, 8.0, -0.5, [0], dims))
    np.testing.assert_array_equal(got["bonds"], table8)

    # the angle: H = D + (1, 0, 0), so w_HD = (-1, 0, 0) and dot = -w_HAx
    h = (1.0, 0.0, 0.0)
    cases = [(o, h, (1.0, 2.0, 0.0)),           # w_HA = (0, 2, 0): a right angle, c = 0 == cos_max
             (o, h, (1.25, 2.0, 0.0)),          # one grid step wider: c < 0
             (o, h, (0.75, 2.0, 0.0)),          # one grid step narrower: c > 0
             (o, h, (3.0, 0.0, 0.0)),           # D, H, A collinear: c = -2 / sqrt(1 * 4) = -1 exactly
             (o, h, (3.0, 0.25, 0.0)),          # next to collinear: c > -1
             (o, h, (1.0, 0.0, 0.0)),           # the acceptor on the hydrogen: c = 0 / 0, no bond, degenerate
             (o, (0.0, 0.0, 0.0), (3.0, 0.0, 0.0))]     # the hydrogen on its donor: the same
    pos = _three_rows(cases, dims)
    r2, c = zip(*(frame_geometry(frame, *tables, dims) for frame in pos))
    np.testing.assert_array_equal(np.ravel(c)[[0, 3]], [0.0, -1.0])
    assert np.ravel(c)[1] < 0 < np.ravel(c)[2] and np.ravel(c)[4] > -1 and np.isnan(np.ravel(c)[5:]).all()
    for cos_max, table, last_bin in ((0.0, [1, 1, 0, 1, 1, 0, 0], None), (-1.0, [0, 0, 0, 1, 0, 0, 0], 1),
                                     (1.0, [1, 1, 1, 1, 1, 0, 0], None)):
        want = restate(pos, *tables, 5.0, cos_max, [0], dims)
        np.testing.assert_array_equal(want["bonds"], table)
        got = engine_run(pos, tables, 5.0, cos_max, [0], dims)
        assert_same(got, want)
        np.testing.assert_array_equal(got["bonds"], table)
        assert got["degenerate"] == 2
    # c on a threshold belongs to the bin below it (c <= t[m]), r2 on a threshold to the bin above it (r2 >= t[m])
    bins = ([0.0, 4.0, 9.0, 25.0], [0.0, -0.5, -1.0])
    want = restate(pos, *tables, 5.0, 0.0, [0], dims, r2_thresholds=bins[0], cos_thresholds=bins[1])
    np.testing.assert_array_equal(want["distance_counts"], [0, 2, 2])       # r2_DA = 5, 5.5625 | 9, 9.0625
    np.testing.assert_array_equal(want["cosine_counts"], [2, 2])            # c = 0, -0.12 | -1, -0.997
    assert_same(engine_run(pos, tables, 5.0, 0.0, [0], dims, bins=bins), want)


def test_a_donor_is_never_the_acceptor_of_its_own_hydrogens():
    """Two waters, both oxygens acceptors, every angle allowed (cos_max = 1): without the exclusion every hydrogen
    would be bonded to its own oxygen (r2_DA = 0, c = +1)."""
    dims = np.array([20.0, 20.0, 20.0])
    tables = ([1, 2, 4, 5], [0, 0, 3, 3], [0, 3])
    one = np.array([[5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [5.0, 6.0, 5.0]])
    far = np.stack((np.concatenate((one, one + [9.0, 0.0, 0.0])),
                    np.concatenate((one, one + [2.75, 0.0, 0.0])))).astype(np.float32)
    want = restate(far, *tables, 3.5, 1.0, [0, 1], dims)
    np.testing.assert_array_equal(want["bonds"], [0, 4])        # apart: nothing; 2.75 apart: every H to the other O
    assert want["evaluations"] == 2 * (4 * 2 - 4) and want["degenerate"] == 0
    got = engine_run(far, tables, 3.5, 1.0, [0, 1], dims)
    assert_same(got, want)
    np.testing.assert_array_equal(got["bonds"], [0, 4])
    np.testing.assert_array_equal(got["donated"], [4, 4, 0, 0, 0, 0, 0, 0, 0])
    # an acceptor that is nobody's donor is counted in: one more oxygen-like row
    lone = np.concatenate((far, np.full((2, 1, 3), 15.0, dtype=np.float32)), axis=1)
    got = engine_run(lone, (tables[0], tables[1], [0, 3, 6]), 3.5, 1.0, [0, 1], dims)
    assert got["evaluations"] == 2 * (4 * 3 - 4)
    np.testing.assert_array_equal(got["bonds"], [0, 4])


def test_hand_made_intermittent_and_continuous():
    """One D-H...A at rest but for the hydrogen, which turns away at frame 3 and back at frame 5: the acceptor stays
    inside the distance, the bond breaks by the angle alone."""
    dims = np.array([40.0, 40.0, 40.0])
    tables = ([1], [0], [2])
    bonded = np.array([1, 1, 1, 0, 0, 1, 1, 1], dtype=bool)     # breaks at frame 3, returns at frame 5
    lags = np.arange(8)
    pos = np.tile(np.array([[20.0, 20.0, 20.0], [21.0, 20.0, 20.0], [22.75, 20.0, 20.0]]), (8, 1, 1))
    pos[~bonded, 1] = [20.0, 21.0, 20.0]
    pos = pos.astype(np.float32)
    r2 = np.array([frame_geometry(frame, *tables, dims)[0][0, 0] for frame in pos])
    assert (r2 == 2.75 ** 2).all() and (r2 <= 3.0 ** 2).all()   # inside in every frame
    got = engine_run(pos, tables, 3.0, COS150, lags, dims)
    assert_same(got, restate(pos, *tables, 3.0, COS150, lags, dims))
    np.testing.assert_array_equal(got["bonds"], bonded.astype(np.int64))
    np.testing.assert_array_equal(got["intermittent"], [6, 4, 2, 1, 2, 3, 2, 1])
    np.testing.assert_array_equal(got["continuous"], [6, 4, 2, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got["origin_counts"], [6, 5, 4, 3, 3, 3, 2, 1])
    np.testing.assert_array_equal(got["donated"][:2], [2, 6])
    # every second frame an origin
    got = engine_run(pos, tables, 3.0, COS150, lags, dims, origin_step=2)
    np.testing.assert_array_equal(got["intermittent"], [3, 2, 1, 1, 1, 2, 1, 1])     # origins 0, 2, (4), 6
    np.testing.assert_array_equal(got["continuous"], [3, 2, 1, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got["origin_counts"], [3, 3, 2, 2, 2, 2, 1, 1])
    assert_same(got, restate(pos, *tables, 3.0, COS150, lags, dims, origin_step=2))


@pytest.mark.parametrize("n_r, n_c", [(60, 60), (512, 512), (513, 60), (60, 513), (513, 513), (1, 1)])
def test_geometry_histograms_and_donated(system, n_r, n_c):
    """Up to 512 bins each the histograms are counted in LDS, beyond in HBM."""
    pos, tables, base = system["pos"], system["tables"], system["want"]
    edges, r2_t, cos_t = bins_of(DISTANCE, 150.0, n_r, n_c)
    got = engine_run(pos, tables, DISTANCE, COS150, LAGS, BOX, bins=(r2_t, cos_t))
    np.testing.assert_array_equal(got["distance_counts"], np.histogram(np.sqrt(base["r2"]), edges)[0])
    np.testing.assert_array_equal(got["cosine_counts"], np.bincount(bin_down(base["c"], cos_t), minlength=n_c))
    np.testing.assert_array_equal(got["donated"], np.bincount(base["rows"].ravel(), minlength=9))
    assert got["distance_counts"].sum() == got["cosine_counts"].sum() == got["bonds"].sum() == base["bonds"].sum()
    assert got["donated"].sum() == F * 514 and got["donated"] @ np.arange(9) == base["bonds"].sum()
    assert (got["distance_counts"] > 0).sum() > min(n_r, 10) - 1 and (got["cosine_counts"] > 0).sum() > min(n_c, 10) - 1
    assert_same(got, restate(pos, *tables, DISTANCE, COS150, LAGS, BOX, r2_thresholds=r2_t, cos_thresholds=cos_t))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(system, axis):
    pos, tables, bins = system["pos"], system["tables"], system["bins"]
    kw = dict(r2_thresholds=bins[0], cos_thresholds=bins[1], max_neighbors=64)
    want = restate(pos, *tables, DISTANCE, COS150, LAGS, BOX, zero_dims=1 << axis, **kw)
    assert want["max_row"] <= 64 and (want["bonds"] > system["want"]["bonds"]).all()
    got = engine_run(pos, tables, DISTANCE, COS150, LAGS, BOX, zero_dims=1 << axis, bins=bins, max_neighbors=64)
    assert_same(got, want)
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    again = engine_run(flat, tables, DISTANCE, COS150, LAGS, BOX, bins=bins, max_neighbors=64)
    for key in KEYS + ("bonds", "distance_counts", "cosine_counts", "donated"):
        np.testing.assert_array_equal(again[key], got[key])


def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, tables, bins, want = system["pos"], system["tables"], system["bins"], system["want"]
    n = pos.shape[1]

    def check(eng):
        assert_same(collect(eng), want)

    run = lambda **kw: engine_run(pos, tables, DISTANCE, COS150, LAGS, BOX, bins=bins, **kw)      # noqa: E731
    assert_same(run(), want)
    assert_same(run(splits=[0, 1, 5, 12]), want)                    # lag 11 spans every call
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want)    # an alive mask crosses three slabs
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want)
    wide = run(max_neighbors=64)                                    # another stride of the lists
    np.testing.assert_array_equal(wide.pop("donated"), np.pad(want["donated"], (0, 56)))
    assert_same({**wide, "donated": want["donated"]}, want)
    assert want["continuous"].any()
    assert_same(run(continuous=False), want, continuous=False)
    assert_same(run(continuous=False, splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want,
                continuous=False)

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
    eng = _core.HydrogenBondEngine(n, *tables, DISTANCE, COS150, LAGS, BOX)
    try:
        eng.set_bins(*bins)
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_bins(*bins)
        eng.reset()
        stats = eng.stats()
        assert stats["frames"] == 0 and stats["evaluations"] == 0 and stats["max_row"] == 0
        assert stats["degenerate"] == 0
        assert not any(v.any() for v in eng.result().values()) and len(eng.bonds()) == 0
        assert not any(v.any() for v in eng.geometry().values())
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
        eng.set_bins(*bins_of(DISTANCE, 150.0, 513, 7)[1:])         # other bins after a reset: the counters resize
        eng.accumulate(pos)
        other = collect(eng)
        assert other["distance_counts"].shape == (513,) and other["cosine_counts"].shape == (7,)
        assert other["distance_counts"].sum() == other["cosine_counts"].sum() == want["bonds"].sum()
        np.testing.assert_array_equal(other["continuous"], want["continuous"])
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


def test_a_row_beyond_max_neighbors_is_an_error_never_a_truncation(system):
    """257 waters at 120 degrees: the fullest hydrogen holds 5 bonds."""
    pos, tables = system["pos"], system["tables"]
    want = restate(pos, *tables, DISTANCE, COS120, LAGS, BOX)
    assert want["max_row"] == 5 and want["bonds"].min() == 314 and want["bonds"].max() == 364
    assert want["continuous"][5] == 49
    calm = np.flatnonzero(want["rows"].max(axis=1) <= 4)            # frames that fit four slots
    assert len(calm) >= 2 and len(calm) < F
    sparse = pos[calm[:2]]
    sparse_want = restate(sparse, *tables, DISTANCE, COS120, [0, 1], BOX, max_neighbors=4)
    assert 0 < sparse_want["max_row"] <= 4
    eng = _core.HydrogenBondEngine(pos.shape[1], *tables, DISTANCE, COS120, [0, 1], BOX, max_neighbors=4)
    try:
        eng.accumulate(pos)
        for call in (eng.result, eng.result, eng.synchronize, eng.bonds, eng.geometry):    # ... and again
            with pytest.raises(ValueError, match="max_neighbors") as err:
                call()
            assert "5" in str(err.value) and "= 4" in str(err.value)
        assert eng.stats()["max_row"] == 5                          # the kernel kept counting
        eng.reset()
        eng.accumulate(sparse)
        assert_same(collect(eng), sparse_want)                      # works again after reset
    finally:
        eng.close()
    assert_same(engine_run(pos, tables, DISTANCE, COS120, LAGS, BOX), want)
    exact = engine_run(pos, tables, DISTANCE, COS120, LAGS, BOX, max_neighbors=5)   # exactly full is no error
    np.testing.assert_array_equal(exact["donated"], want["donated"][:6])
    for key in KEYS + ("bonds",):
        np.testing.assert_array_equal(exact[key], want[key])
    with pytest.raises(ValueError, match="max_neighbors"):
        engine_run(pos, tables, DISTANCE, COS120, LAGS, BOX, max_neighbors=4)


# ---------------------------------------------------------------- the class

def test_class_routes_groups_and_frame_selections(system, tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_mol, extra = 257, 3
    water_pos = system["pos"]
    rng = np.random.default_rng(3)
    # three atoms that take no part in front of the water: the feed is an index
    pos = np.concatenate(((rng.uniform(0.0, 1.0, (F, extra, 3)) * BOX).astype(np.float32), water_pos), axis=1)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    h_row, d_row, a_row = (t + extra for t in system["tables"])
    lags = np.array([0, 1, 3, 8, 12])
    path = tmp_path / "w.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    counts = ("bonds", "intermittent_counts", "continuous_counts", "origin_counts", "donated_counts",
              "distance_counts", "angle_counts")

    def check(v, frames, step, origin_step=1, dims=BOX, angle=150.0):
        """v.results against the restatement and the formulas on the selected frames."""
        want = restate(water_pos[frames], *system["tables"], DISTANCE, cos_of(angle), lags, dims,
                       origin_step=origin_step, r2_thresholds=v._r2_thresholds, cos_thresholds=v._cos_thresholds)
        res = v.results
        for key in KEYS[:2]:
            np.testing.assert_array_equal(res[key + "_counts"], want[key])
            assert res[key + "_counts"].dtype == np.int64
        np.testing.assert_array_equal(res.origin_counts, want["origin_counts"])
        np.testing.assert_array_equal(res.bonds, want["bonds"])
        np.testing.assert_array_equal(res.bonds_per_hydrogen, want["bonds"] / (2 * n_mol))
        np.testing.assert_array_equal(res.n_origins, [len(range(0, max(len(frames) - lag, 0), origin_step))
                                                      for lag in lags])
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        live = want["origin_counts"] > 0
        assert live[0] and not live[-1]
        o = want["origin_counts"].astype(float)
        np.testing.assert_array_equal(res.intermittent[live], want["intermittent"][live] / o[live])
        np.testing.assert_array_equal(res.continuous[live], want["continuous"][live] / o[live])
        assert np.isnan(res.intermittent[~live]).all() and np.isnan(res.continuous[~live]).all()    # no origin: NaN
        assert res.intermittent[0] == 1.0 and res.continuous[0] == 1.0
        assert (res.continuous[live] <= res.intermittent[live]).all()
        np.testing.assert_array_equal(res.donated_counts, want["donated"])
        np.testing.assert_array_equal(res.donated, want["donated"] / (len(frames) * 2 * n_mol))
        assert res.donated.sum() == pytest.approx(1.0, abs=1e-14)
        np.testing.assert_array_equal(res.distance_counts, np.histogram(np.sqrt(want["r2"]), res.distance_edges)[0])
        np.testing.assert_array_equal(res.angle_counts, want["cosine_counts"])
        np.testing.assert_array_equal(res.distance_edges, np.linspace(0.0, DISTANCE, 61))
        np.testing.assert_array_equal(res.angle_edges, np.linspace(angle, 180.0, 61))
        np.testing.assert_array_equal(res.distance_bins, (res.distance_edges[1:] + res.distance_edges[:-1]) / 2)
        np.testing.assert_array_equal(res.angle_bins, (res.angle_edges[1:] + res.angle_edges[:-1]) / 2)
        total = want["bonds"].sum()
        assert total > 0 and res.distance_counts.sum() == res.angle_counts.sum() == total
        assert (res.distance_distribution * np.diff(res.distance_edges)).sum() == pytest.approx(1.0, abs=1e-13)
        assert (res.angle_distribution * np.diff(res.angle_edges)).sum() == pytest.approx(1.0, abs=1e-13)
        np.testing.assert_array_equal(res.distance_distribution,
                                      res.distance_counts / (float(total) * np.diff(res.distance_edges)))
        assert res.degenerate == 0 and res.units["results.times"] == "picosecond"

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            def make(u=u, **kw):
                return HydrogenBonds(u.select(d_row), u.select(h_row), u.select(a_row), distance=DISTANCE, lags=lags,
                                     verbose=False, **kw)

            full = make().run()
            check(full, np.arange(F), 1)
            check(make().run(start=1, stop=11, step=2), np.arange(1, 11, 2), 2)
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3)
            check(make(origin_step=2).run(), np.arange(F), 1, origin_step=2)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in counts + ("intermittent", "degenerate"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        make = lambda **kw: HydrogenBonds(u.select(d_row), u.select(h_row), u.select(a_row), distance=DISTANCE,  # noqa
                                          lags=lags, verbose=False, **kw)
        # the molecules by their places: the same tables, the same integers
        mol = HydrogenBonds.from_molecules(u.select(np.arange(extra, extra + 3 * n_mol)), n_mol, distance=DISTANCE,
                                           lags=lags, verbose=False).run()
        for key in counts:
            np.testing.assert_array_equal(mol.results[key], results["host"][key])
        # neither lags nor n_lags: every analysed frame is a lag
        every = HydrogenBonds(u.select(d_row), u.select(h_row), u.select(a_row), distance=DISTANCE,
                              verbose=False).run()
        want = restate(water_pos, *system["tables"], DISTANCE, cos_of(150.0), np.arange(F), BOX)
        np.testing.assert_array_equal(every.results.continuous_counts, want["continuous"])
        np.testing.assert_array_equal(every.results.intermittent_counts, want["intermittent"])
        # the lifetimes are the explicit trapezoid sums
        every.calculate_lifetimes()
        t, s_c, s_i = every.results.times, every.results.continuous, every.results.intermittent
        assert np.isfinite(s_c).all() and s_c[0] == 1.0
        assert every.results.lifetime == float(((s_c[1:] + s_c[:-1]) * np.diff(t)).sum() / 2)
        assert every.results.relaxation_time == float(((s_i[1:] + s_i[:-1]) * np.diff(t)).sum() / 2)
        assert every.results.lifetime == calculate_residence_time(t, s_c) < every.results.relaxation_time
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(make()).run()
        for key in counts:
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = make(dimensions=wide).run()
        check(other, np.arange(F), 1, dims=wide)
        assert (other.results.bonds != results["host"].bonds).any()
        # another angle, fewer bins, and without the frames between the lags
        check(make(angle=120.0).run(), np.arange(F), 1, angle=120.0)
        few = make(n_distance_bins=1, n_angle_bins=3, continuous=False).run()
        np.testing.assert_array_equal(few.results.intermittent_counts, results["host"].intermittent_counts)
        assert not few.results.continuous_counts.any()
        np.testing.assert_array_equal(few.results.distance_counts, [results["host"].bonds.sum()])
        assert few.results.angle_counts.shape == (3,) and few.results.angle_counts.sum() == results["host"].bonds.sum()
        # no lag with an origin: the bonds and their geometry all the same
        late = HydrogenBonds(u.select(d_row), u.select(h_row), u.select(a_row), distance=DISTANCE, lags=[20],
                             verbose=False).run()
        np.testing.assert_array_equal(late.results.bonds, results["host"].bonds)
        np.testing.assert_array_equal(late.results.distance_counts, results["host"].distance_counts)
        assert not late.results.origin_counts.any() and np.isnan(late.results.intermittent).all()
        # too few slots: the error of the engine reaches the caller of run()
        with pytest.raises(ValueError, match="max_neighbors"):
            make(angle=120.0, max_neighbors=4).run()
    finally:
        d.free()
