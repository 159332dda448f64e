"""
PairResidence / PairResidenceEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_residence_device.hpp): per frame f and pair (i of set 1, j of set 2, j != i when both are one set), both at
frame f,

    d = x2_j - x1_i;  s = d * (1.0 / L);  w = d - L * rint(s) (+0.0 for a dropped component);
    r2 = (wx*wx + wy*wy) + wz*wz;  h_ij(f) = r2 <= cutoff * cutoff

and per lag, over the origins f0 that are multiples of origin_step with f0 + lag < F: origin_counts += sum(h(f0)),
intermittent += sum(h(f0) & h(f0 + lag)), continuous += sum(h(f0) & h(f0 + 1) & ... & h(f0 + lag)).

No tolerance anywhere: the results are integers, the restatement does one float64 operation at a time, as the device
does (the unit is built with contraction off; rint rounds ties to even on both sides), so every comparison is
``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import PairResidence, calculate_residence_time

pytestmark = pytest.mark.gpu

T = _core.PairResidenceEngine.TILE
J = _core.PairResidenceEngine.JCHUNK
LAGS = [0, 1, 2, 5, 8, 11, 13]          # lag 13 never has an origin in 12 frames
BOX = np.array([31.0, 44.5, 57.25])
CUTOFF = 6.0
KEYS = ("intermittent", "continuous", "origin_counts")


# ---------------------------------------------------------------- restatement

def contact_matrix(a, b, dims, cutoff, zero_dims=0):
    """bool [n1, n2]: the contract's h for every pair of a float64[n1, 3] and b float64[n2, 3]."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    d = b[None, :, :] - a[:, None, :]
    s = d * inv
    w = d - dims * np.rint(s)
    for c in range(3):
        if zero_dims >> c & 1:
            w[..., c] = 0.0
    r2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    return r2 <= np.float64(cutoff) * np.float64(cutoff)


def restate(x1, x2, cutoff, lags, dims, *, origin_step=1, zero_dims=0):
    """The four result arrays, evaluations, frames and max_row; x2 None: one set, the pair i == j left out."""
    same = x2 is None
    a = np.asarray(x1).astype(np.float64)
    b = a if same else np.asarray(x2).astype(np.float64)
    F, n1, n2 = len(a), a.shape[1], b.shape[1]
    h = np.stack([contact_matrix(a[f], b[f], dims, cutoff, zero_dims) for f in range(F)])
    if same:
        h &= ~np.eye(n1, dtype=bool)
    out = {key: np.zeros(len(lags), dtype=np.int64) for key in KEYS}
    for k, lag in enumerate(lags):
        for f0 in range(0, F - lag, origin_step):
            out["origin_counts"][k] += h[f0].sum()
            out["intermittent"][k] += (h[f0] & h[f0 + lag]).sum()
            out["continuous"][k] += np.logical_and.reduce(h[f0:f0 + lag + 1], axis=0).sum()
    out["contacts"] = h.sum(axis=(1, 2)).astype(np.int64)
    out["evaluations"] = F * (n1 * n2 - (n1 if same else 0))
    out["frames"] = F
    out["max_row"] = int(h.sum(axis=2).max())
    return out


def collect(eng):
    got = eng.result()
    got["contacts"] = eng.contacts()
    stats = eng.stats()
    got.update(evaluations=stats["evaluations"], frames=stats["frames"], max_row=stats["max_row"])
    return got


def engine_run(x1, x2, cutoff, lags, dims, *, splits=None, setup=None, **kwargs):
    """One pass over the frames, host route: what ``restate`` returns."""
    same = x2 is None
    pos = x1 if same else np.concatenate((x1, x2), axis=1)
    eng = _core.PairResidenceEngine(x1.shape[1], x1.shape[1] if same else x2.shape[1], cutoff, lags, dims, same=same,
                                    **kwargs)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def assert_same(got, want, continuous=True):
    for key in KEYS + ("contacts",):
        expect = want[key] if continuous or key != "continuous" else np.zeros_like(want[key])
        np.testing.assert_array_equal(got[key], expect, err_msg=key)
        assert got[key].dtype == np.int64
    for key in ("evaluations", "frames", "max_row"):
        assert got[key] == want[key], key


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
    for F in (1, 2, 12):
        pos = walk(100 + n, F, n, step=0.25)
        want = restate(pos, None, CUTOFF, LAGS, BOX)
        got = engine_run(pos, None, CUTOFF, LAGS, BOX)
        assert_same(got, want)
        assert want["evaluations"] == F * (n * n - n)
        for key in KEYS:
            assert got[key][6] == 0                                 # lag 13: no origin
            assert not got[key][[origins(F, lag) == 0 for lag in LAGS]].any()
        if n == 1:
            assert not got["contacts"].any() and want["evaluations"] == 0       # no pair at all
        elif n >= 63 and F == 12:
            assert (got["intermittent"][:6] > 0).all() and (got["continuous"][:6] > 0).all()
            assert want["max_row"] <= 32
            if n >= T - 1:
                assert (got["continuous"][2:6] < got["intermittent"][2:6]).all()    # pairs part and come back


@pytest.mark.parametrize("n1, n2", [(1, 1), (1, 2 * T + 3), (2 * T + 3, 1), (65, T + 1), (T + 1, 65)])
def test_two_sets_sizes_and_frame_counts(n1, n2):
    for F in (1, 2, 12):
        pos = walk(200 + n1, F, n1 + n2, step=0.25)
        x1, x2 = pos[:, :n1], pos[:, n1:]
        want = restate(x1, x2, CUTOFF, LAGS, BOX)
        got = engine_run(x1, x2, CUTOFF, LAGS, BOX)
        assert_same(got, want)
        assert want["evaluations"] == F * n1 * n2
        for key in KEYS:
            assert got[key][6] == 0
    with pytest.raises(ValueError, match="rows given"):
        engine_run(x1, x2, CUTOFF, LAGS, BOX, setup=lambda e: e.accumulate(pos[:, :-1]))      # wrong row count


@pytest.mark.parametrize("n2", [J - 1, J, J + 1])
def test_partners_around_one_chunk_and_rings_that_wrap_inside_one_call(n2):
    """JCHUNK - 1, JCHUNK and JCHUNK + 1 partners (the last: a second chunk of one partner appends to the same rows)
    against T + 1 points (a second tile of one live lane).  Lags 0 and 1 with slabs of one frame: the rings hold two
    frames, so the third frame of the one call goes into the slot of the first."""
    n1 = T + 1
    pos = walk(300 + n2, 3, n1 + n2, step=0.25)
    x1, x2 = pos[:, :n1], pos[:, n1:]
    want = restate(x1, x2, 4.0, [0, 1], BOX)
    assert 1 <= want["max_row"] <= 32 and want["intermittent"].all()
    assert_same(engine_run(x1, x2, 4.0, [0, 1], BOX, setup=lambda e: e.set_slab_frames(1)), want)
    if n2 == J + 1:
        # one set: the second chunk's only partner is the own point of the one live lane of the last tile
        one = pos[:, :n2]
        assert_same(engine_run(one, None, 4.0, [0, 1], BOX, setup=lambda e: e.set_slab_frames(1)),
                    restate(one, None, 4.0, [0, 1], BOX))


@pytest.fixture(scope="module")
def short_walk():
    """9 frames of one set of 65 points and the restatement for lags 0, 1, 3, shared and left unchanged."""
    pos = walk(400, 9, 65, step=0.25)
    want = restate(pos, None, CUTOFF, [0, 1, 3], BOX)
    assert want["continuous"].all() and want["continuous"][2] < want["intermittent"][2] < want["origin_counts"][2]
    pos.setflags(write=False)
    for key in KEYS + ("contacts",):
        want[key].setflags(write=False)
    return pos, want


@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("slab", [1, 2])
def test_the_rings_wrap_across_two_calls(short_walk, slab, continuous):
    """With lags up to 3 the rings hold 3 + slab frames, fewer than the 9 fed as 4 + 5: every slot of the lists and
    of the alive masks is emptied and written twice or more, the second call starts in the middle of the rings, and
    lag 3 reaches back across the wrap and across the calls.  (The split tests below feed 12 frames to rings of at
    least 14.)"""
    pos, want = short_walk

    def run(**kw):
        return engine_run(pos, None, CUTOFF, [0, 1, 3], BOX, continuous=continuous,
                          setup=lambda e: e.set_slab_frames(slab), **kw)

    assert_same(run(splits=[0, 4, 9]), want, continuous=continuous)
    assert_same(run(), want, continuous=continuous)


def test_the_issue_figures_for_321_points():
    """The figures the restatement gives for walk(seed, 12, 321, step=0.25): rows well inside the default cap, the
    two functions apart from lag 2 on, lag 11 alive and lag 13 without an origin."""
    pos = walk(100 + 321, 12, 321, step=0.25)
    want = restate(pos, None, CUTOFF, LAGS, BOX)
    assert 1 <= want["max_row"] <= 16
    assert want["intermittent"][0] == want["continuous"][0] == want["origin_counts"][0] == want["contacts"].sum()
    assert want["intermittent"][1] >= want["continuous"][1]
    assert (want["intermittent"][2:6] > want["continuous"][2:6]).all() and want["continuous"][5] > 0
    assert want["origin_counts"][6] == 0
    assert_same(engine_run(pos, None, CUTOFF, LAGS, BOX), want)


def test_exact_arithmetic_on_the_cutoff():
    """float32 coordinates on a grid of 0.25, box (16, 16, 32), cutoff 5: every r2 below is exact.  One pair per
    frame, so contacts[f] is h of that pair; the table is written out by hand."""
    dims = np.array([16.0, 16.0, 32.0])
    moves = np.array([[3.0, -4.0, 0.0],        # r2 = 25 == rc2: a contact
                      [3.0, -4.0, 0.25],       # one grid step outside: r2 = 25.0625
                      [5.25, 0.0, 0.0],        # one grid step outside along x
                      [8.0, 0.0, 0.0],         # s = +0.5 -> rint 0 (ties to even): w = 8, r2 = 64
                      [-8.0, 0.0, 0.0],        # s = -0.5 -> rint -0: w = -8
                      [13.0, 4.0, 0.0],        # s = 0.8125 -> w = -3 in x: folded onto the cutoff, r2 = 25
                      [0.0, 0.0, -27.0],       # s = -0.84375 -> w = 5 in z: folded onto the cutoff
                      [0.0, 0.0, 26.75],       # w = -5.25 in z: one grid step outside after the fold
                      [0.0, 24.0, 0.25],       # s = 1.5 -> rint 2: w = -8 in y
                      [0.0, 0.0, 0.0],         # a distinct pair at one place: r2 = 0
                      [-4.0, 0.0, 3.0]])       # r2 = 25
    table = np.array([1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1], dtype=np.int64)
    origin = np.array([3.25, 9.5, 20.75])
    x1 = np.tile(origin, (len(moves), 1, 1)).astype(np.float32)
    x2 = (origin + moves)[:, None, :].astype(np.float32)
    np.testing.assert_array_equal(x2.astype(np.float64)[:, 0], origin + moves)
    for a, b in ((x1, x2), (x2, x1)):          # the other way round every d changes sign: the same table
        want = restate(a, b, 5.0, [0], dims)
        np.testing.assert_array_equal(want["contacts"], table)
        got = engine_run(a, b, 5.0, [0], dims)
        assert_same(got, want)
        np.testing.assert_array_equal(got["contacts"], table)
        assert got["intermittent"][0] == got["continuous"][0] == got["origin_counts"][0] == 5
    # cutoff 8, half the box: after the tie the pairs at +-8 along x or y lie exactly on it
    table8 = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=np.int64)      # (0, -8, 0.25): r2 = 64.0625
    got = engine_run(x1, x2, 8.0, [0], dims)
    assert_same(got, restate(x1, x2, 8.0, [0], dims))
    np.testing.assert_array_equal(got["contacts"], table8)
    # all the points of one frame as one set: against the restatement
    both = np.concatenate((x1[:1], x2.reshape(1, -1, 3)), axis=1)
    assert_same(engine_run(both, None, 5.0, [0], dims), restate(both, None, 5.0, [0], dims))


def test_hand_made_intermittent_and_continuous():
    """One point of set 1 at rest; a partner is at distance 1 (a contact) or 10 (none) by a pattern."""
    dims = np.array([40.0, 40.0, 40.0])
    leaves = np.array([1, 1, 1, 0, 0, 1, 1, 1], dtype=bool)     # leaves at frame 3, returns at frame 5
    stays = np.ones(8, dtype=bool)
    lags = np.arange(8)
    centre = np.array([20.0, 20.0, 20.0])

    def frames(patterns):
        x2 = np.tile(centre, (8, len(patterns), 1))
        for j, p in enumerate(patterns):
            x2[:, j, j % 3] += np.where(p, 1.0, 10.0)
        return np.tile(centre, (8, 1, 1)).astype(np.float32), x2.astype(np.float32)

    x1, x2 = frames([leaves])
    got = engine_run(x1, x2, 2.0, lags, dims)
    assert_same(got, restate(x1, x2, 2.0, lags, dims))
    np.testing.assert_array_equal(got["contacts"], leaves.astype(np.int64))
    np.testing.assert_array_equal(got["intermittent"], [6, 4, 2, 1, 2, 3, 2, 1])
    np.testing.assert_array_equal(got["continuous"], [6, 4, 2, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got["origin_counts"], [6, 5, 4, 3, 3, 3, 2, 1])
    x1, x2 = frames([stays])
    got = engine_run(x1, x2, 2.0, lags, dims)
    for key in KEYS:
        np.testing.assert_array_equal(got[key], 8 - lags)       # present in every frame: all three agree
    x1, x2 = frames([leaves, stays, ~leaves])
    got = engine_run(x1, x2, 2.0, lags, dims)
    assert_same(got, restate(x1, x2, 2.0, lags, dims))
    np.testing.assert_array_equal(got["contacts"], [2, 2, 2, 2, 2, 2, 2, 2])
    np.testing.assert_array_equal(got["continuous"], np.array([6, 4, 2, 0, 0, 0, 0, 0]) + (8 - lags)
                                  + np.array([2, 1, 0, 0, 0, 0, 0, 0]))
    # every second frame an origin
    got = engine_run(x1, x2[:, :1], 2.0, lags, dims, origin_step=2)
    np.testing.assert_array_equal(got["intermittent"], [3, 2, 1, 1, 1, 2, 1, 1])     # origins 0, 2, (4), 6
    np.testing.assert_array_equal(got["continuous"], [3, 2, 1, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got["origin_counts"], [3, 3, 2, 2, 2, 2, 1, 1])


@pytest.fixture(scope="module")
def system():
    """Frames, two unequal sets and their restatement, shared and left unchanged."""
    n1, n2, F = 65, T + 1, 12
    pos = walk(11, F, n1 + n2, step=0.25)
    want = restate(pos[:, :n1], pos[:, n1:], CUTOFF, LAGS, BOX)
    want_one = restate(pos, None, CUTOFF, LAGS, BOX)
    pos.setflags(write=False)
    for w in (want, want_one):
        for key in KEYS + ("contacts",):
            w[key].setflags(write=False)
    return {"pos": pos, "n1": n1, "n2": n2, "want": want, "want_one": want_one}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(system, axis):
    pos, n1 = system["pos"], system["n1"]
    x1, x2 = pos[:, :n1], pos[:, n1:]
    # with a component dropped a cutoff of 6 would fill rows beyond 32: a shorter one keeps the default cap
    want = restate(x1, x2, 3.0, LAGS, BOX, zero_dims=1 << axis)
    assert want["max_row"] <= 32 and (want["contacts"] > restate(x1, x2, 3.0, LAGS, BOX)["contacts"]).all()
    got = engine_run(x1, x2, 3.0, LAGS, BOX, zero_dims=1 << axis)
    assert_same(got, want)
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    again = engine_run(flat[:, :n1], flat[:, n1:], 3.0, LAGS, BOX)
    for key in KEYS + ("contacts",):
        np.testing.assert_array_equal(again[key], got[key])
    assert_same(engine_run(pos, None, 3.0, LAGS, BOX, zero_dims=1 << axis, max_neighbors=64),
                restate(pos, None, 3.0, LAGS, BOX, zero_dims=1 << axis))


@pytest.mark.parametrize("origin_step", [1, 2, 3, 20])
def test_origin_step(system, origin_step):
    pos, n1 = system["pos"], system["n1"]
    x1, x2 = pos[:, :n1], pos[:, n1:]
    want = restate(x1, x2, CUTOFF, LAGS, BOX, origin_step=origin_step)
    if origin_step == 1:
        for key in KEYS:
            np.testing.assert_array_equal(want[key], system["want"][key])
    np.testing.assert_array_equal(want["contacts"], system["want"]["contacts"])     # every frame, origin or not
    assert_same(engine_run(x1, x2, CUTOFF, LAGS, BOX, origin_step=origin_step), want)
    # ... and the same whatever the split into calls and slabs
    assert_same(engine_run(x1, x2, CUTOFF, LAGS, BOX, origin_step=origin_step, splits=[0, 1, 5, 12],
                           setup=lambda e: e.set_slab_frames(4)), want)
    assert_same(engine_run(pos, None, CUTOFF, LAGS, BOX, origin_step=origin_step),
                restate(pos, None, CUTOFF, LAGS, BOX, origin_step=origin_step))


@pytest.mark.parametrize("same", [False, True])
def test_without_continuous_the_walk_visits_lag_frames_only(system, same):
    pos, n1 = system["pos"], system["n1"]
    x1, x2 = (pos, None) if same else (pos[:, :n1], pos[:, n1:])
    want = system["want_one" if same else "want"]
    assert want["continuous"].any()
    assert_same(engine_run(x1, x2, CUTOFF, LAGS, BOX, continuous=False), want, continuous=False)
    assert_same(engine_run(x1, x2, CUTOFF, LAGS, BOX, continuous=False, splits=[0, 1, 5, 12],
                           setup=lambda e: e.set_slab_frames(4)), want, continuous=False)


@pytest.mark.parametrize("same", [False, True])
def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, same, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, n1, n2 = system["pos"], system["n1"], system["n2"]
    F, n = pos.shape[:2]
    want = system["want_one" if same else "want"]
    x1, x2 = (pos, None) if same else (pos[:, :n1], pos[:, n1:])

    def check(eng):
        assert_same(collect(eng), want)

    run = lambda **kw: engine_run(x1, x2, CUTOFF, LAGS, BOX, **kw)      # noqa: E731
    assert_same(run(), want)
    assert_same(run(splits=[0, 1, 5, 12]), want)                    # lag 11 spans every call
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want)    # an alive mask crosses three slabs
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want)
    assert_same(run(max_neighbors=64), want)                        # another stride of the lists

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
    eng = _core.PairResidenceEngine(n if same else n1, n if same else n2, CUTOFF, LAGS, BOX, same=same)
    try:
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        stats = eng.stats()
        assert stats["frames"] == 0 and stats["evaluations"] == 0 and stats["max_row"] == 0
        assert not any(v.any() for v in eng.result().values()) and len(eng.contacts()) == 0
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


def test_a_row_beyond_max_neighbors_is_an_error_never_a_truncation():
    """Frame 0 of walk(12, 12, 322, step=0.25), sets 65 | 257, cutoff 15: the largest row holds 63 contacts."""
    pos = walk(12, 12, 322, step=0.25)[:1]
    x1, x2 = pos[:, :65], pos[:, 65:]
    want = restate(x1, x2, 15.0, [0], BOX)
    assert want["max_row"] == 63 and want["contacts"][0] > 65 * 32
    # sparse input for the same engine: set 1 in one corner, 20 partners next to it, the others half a box away
    rng = np.random.default_rng(5)
    sparse = np.empty((2, 322, 3), dtype=np.float32)
    sparse[:, :65] = rng.uniform(0.0, 1.0, (2, 65, 3))
    sparse[:, 65:85] = rng.uniform(1.0, 3.0, (2, 20, 3))
    sparse[:, 85:] = np.array([15.5, 22.0, 28.0]) + rng.uniform(-1.0, 1.0, (2, 237, 3))
    sparse_want = restate(sparse[:, :65], sparse[:, 65:], 15.0, [0, 1], BOX)
    assert sparse_want["max_row"] == 20
    np.testing.assert_array_equal(sparse_want["contacts"], [65 * 20, 65 * 20])
    eng = _core.PairResidenceEngine(65, 257, 15.0, [0, 1], BOX, max_neighbors=32)
    try:
        eng.accumulate(pos)
        for call in (eng.result, eng.result, eng.synchronize, eng.contacts):        # ... and again on the next call
            with pytest.raises(ValueError, match="max_neighbors") as err:
                call()
            assert "63" in str(err.value) and "32" in str(err.value)
        assert eng.stats()["max_row"] == 63                         # the kernel kept counting
        eng.reset()
        eng.accumulate(sparse)
        assert_same(collect(eng), sparse_want)                      # works again after reset
    finally:
        eng.close()
    assert_same(engine_run(x1, x2, 15.0, [0], BOX, max_neighbors=64), want)
    assert_same(engine_run(x1, x2, 15.0, [0], BOX, max_neighbors=63), want)         # exactly full is no error
    with pytest.raises(ValueError, match="max_neighbors"):
        engine_run(x1, x2, 15.0, [0], BOX, max_neighbors=62)


# ---------------------------------------------------------------- the class

def test_class_routes_groups_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_c, extra, n_a, F = 70, 3, T + 5, 12
    n = n_c + extra + n_a
    pos = walk(20, F, n, step=0.25)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    ia, ib = np.arange(n_c), np.arange(n_c + extra, n)
    lags = np.array([0, 1, 3, 8, 12])
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)

    def check(v, frames, step, i1, i2, origin_step=1, dims=BOX, zero_dims=0):
        """v.results against the restatement and the formulas on the selected frames."""
        x = pos[frames]
        want = restate(x[:, i1], None if i2 is None else x[:, i2], CUTOFF, lags, dims, origin_step=origin_step,
                       zero_dims=zero_dims)
        res = v.results
        for key in KEYS[:2]:
            np.testing.assert_array_equal(res[key + "_counts"], want[key])
            assert res[key + "_counts"].dtype == np.int64
        np.testing.assert_array_equal(res.origin_counts, want["origin_counts"])
        np.testing.assert_array_equal(res.contacts, want["contacts"])
        np.testing.assert_array_equal(res.coordination, want["contacts"] / len(i1))
        np.testing.assert_array_equal(res.n_origins, [origins(len(frames), lag, origin_step) for lag in lags])
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        live = want["origin_counts"] > 0
        assert live[0] and not live[-1]
        o = want["origin_counts"].astype(float)
        np.testing.assert_array_equal(res.intermittent[live], want["intermittent"][live] / o[live])
        np.testing.assert_array_equal(res.continuous[live], want["continuous"][live] / o[live])
        assert np.isnan(res.intermittent[~live]).all() and np.isnan(res.continuous[~live]).all()    # no origin: NaN
        assert res.intermittent[0] == 1.0 and res.continuous[0] == 1.0
        assert (res.continuous[live] <= res.intermittent[live]).all()
        assert res.units["results.times"] == "picosecond"

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            # anions at the origin, cations as partners: not the order of the frame
            def make(u=u, **kw):
                return PairResidence(u.select(ib), u.select(ia), CUTOFF, lags=lags, verbose=False, **kw)

            full = make().run()
            check(full, np.arange(F), 1, ib, ia)
            check(make().run(start=1, stop=11, step=2), np.arange(1, 11, 2), 2, ib, ia)
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3, ib, ia)
            check(make(origin_step=2).run(), np.arange(F), 1, ib, ia, origin_step=2)
            one = PairResidence(u.select(ib), None, CUTOFF, lags=lags, verbose=False).run()
            check(one, np.arange(F), 1, ib, None)
            again = PairResidence(u.select(ib), u.select(ib), CUTOFF, lags=lags, verbose=False).run()
            for key in ("contacts", "intermittent_counts", "continuous_counts", "origin_counts", "continuous"):
                np.testing.assert_array_equal(again.results[key], one.results[key])     # ag2 equal to ag1 is ag2=None
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in ("contacts", "intermittent_counts", "continuous_counts", "origin_counts", "intermittent"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        make = lambda **kw: PairResidence(u.select(ib), u.select(ia), CUTOFF, lags=lags, verbose=False, **kw)  # noqa
        # every particle in order (no index), and neither lags nor n_lags: every analysed frame is a lag
        whole = PairResidence(u.atoms, cutoff=CUTOFF, verbose=False).run()
        want = restate(pos, None, CUTOFF, np.arange(F), BOX)
        np.testing.assert_array_equal(whole.results.continuous_counts, want["continuous"])
        np.testing.assert_array_equal(whole.results.intermittent_counts, want["intermittent"])
        np.testing.assert_array_equal(
            PairResidence(u.atoms, None, CUTOFF, n_lags=4, verbose=False).run().results.continuous_counts,
            want["continuous"][:4])
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(make()).run()
        for key in ("contacts", "intermittent_counts", "continuous_counts", "origin_counts"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = make(dimensions=wide).run()
        check(other, np.arange(F), 1, ib, ia, dims=wide)
        assert (other.results.intermittent_counts != results["host"].intermittent_counts).any()
        # a dropped component (more contacts: more slots), and without the frames between the lags
        check(make(drop_axis="z", max_neighbors=64).run(), np.arange(F), 1, ib, ia, zero_dims=4)
        quick = make(continuous=False).run()
        np.testing.assert_array_equal(quick.results.intermittent_counts, results["host"].intermittent_counts)
        assert not quick.results.continuous_counts.any()
        # too few slots: the error of the engine reaches the caller of run()
        with pytest.raises(ValueError, match="max_neighbors"):
            make(max_neighbors=1).run()
        # the residence times are the explicit trapezoid sums
        full = make().run()
        full.calculate_residence_times()
        res = full.results
        t = res.times[:4]                                   # lag 12 has no origin: the finite leading part is 4 long
        for key, name in (("continuous", "residence_time"), ("intermittent", "relaxation_time")):
            s = res[key][:4]
            assert np.isfinite(s).all() and np.isnan(res[key][4])
            assert res[name] == float(((s[1:] + s[:-1]) * np.diff(t)).sum() / 2)
            assert res[name] == calculate_residence_time(res.times, res[key])
        assert 0 < res.residence_time <= res.relaxation_time <= t[-1]
    finally:
        d.free()
