"""
OrientationalRelaxation / OrientationEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_orient_device.hpp): per vector (tail, head) and frame

    d = x_head - x_tail;  w = d - L * rint(d * (1.0 / L)) with a box, else w = d (+0.0 for a dropped component);
    n2 = (wx*wx + wy*wy) + wz*wz;  u = w / sqrt(n2)

per vector, lag and frame f >= lag

    c = (ux(f)*ux(f-lag) + uy(f)*uy(f-lag)) + uz(f)*uz(f-lag);  acc[0] += c;  acc[1] += (1.5 * (c*c)) - 0.5

and per frame, group and product ab = xx, xy, xz, yy, yz, zz the sum of ua*ub over the tiles of 64 vectors in row
order and then over the group's tiles in tile order.

No tolerance in any comparison with the restatement (the physics test and a few sanity checks of sums against
their closed forms have bounds, derived where they stand).  The restatement does one float64 operation at a time, as the device
does (the unit is built with contraction off; sqrt and the divide are correctly rounded on both sides); the accumulator
of every vector receives its terms in frame order from a Python loop over the frames, a group's sums add the
accumulators of its vectors in row order from a Python loop over the vectors, and the products go through a loop over
the vectors of a tile and a loop over the tiles.  The same operations in the same order give the same bits, so every
result is compared with ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import OrientationalRelaxation, calculate_residence_time

pytestmark = pytest.mark.gpu

T = _core.OrientationEngine.TILE
LAGS = [0, 1, 2, 5, 36, 40]           # lag 40 never has an origin in 37 frames
PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---------------------------------------------------------------- restatement

def unit_vectors(pos, pairs, *, dims=None, zero_dims=0):
    """float64 [F, V, 3]: one operation at a time."""
    x = np.asarray(pos).astype(np.float64)
    pairs = np.asarray(pairs)
    w = x[:, pairs[:, 1]] - x[:, pairs[:, 0]]
    if dims is not None:
        L = np.asarray(dims, dtype=np.float64)
        inv = 1.0 / L
        w = w - L * np.rint(w * inv)
    for c in range(3):
        if zero_dims >> c & 1:
            w[..., c] = 0.0
    n2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    assert np.all(n2 > 0) and np.all(np.isfinite(n2))
    return w / np.sqrt(n2)[..., None]


def restate(pos, sizes, pairs, lags, *, dims=None, zero_dims=0):
    """(sums [K, G, 2], vector accumulators [K, V, 2], frame sums [F, G, 6], evaluations)."""
    u = unit_vectors(pos, pairs, dims=dims, zero_dims=zero_dims)
    F, V = u.shape[:2]
    acc = np.zeros((len(lags), V, 2))
    evaluations = 0
    for k, lag in enumerate(lags):
        for f in range(lag, F):                                 # the accumulators take their terms in frame order
            a, b = u[f], u[f - lag]
            c = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
            acc[k, :, 0] = acc[k, :, 0] + c
            acc[k, :, 1] = acc[k, :, 1] + ((1.5 * (c * c)) - 0.5)
            evaluations += V
    sums = np.zeros((len(lags), len(sizes), 2))
    frame_sums = np.zeros((F, len(sizes), 6))
    lo = 0
    for g, size in enumerate(sizes):
        s = np.zeros((len(lags), 2))
        for v in range(lo, lo + size):                          # a group's vectors in row order
            s = s + acc[:, v, :]
        sums[:, g] = s
        total = np.zeros((F, 6))
        for t0 in range(lo, lo + size, T):                      # its tiles in tile order
            partial = np.zeros((F, 6))
            for v in range(t0, min(t0 + T, lo + size)):         # a tile's vectors in row order
                partial = partial + np.stack([u[:, v, a] * u[:, v, b] for a, b in PRODUCTS], axis=1)
            total = total + partial
        frame_sums[:, g] = total
        lo += size
    return sums, acc, frame_sums, evaluations


def engine_run(pos, sizes, pairs, lags, *, splits=None, setup=None, zero_dims=0):
    eng = _core.OrientationEngine(sizes, pairs, pos.shape[1], lags, zero_dims=zero_dims)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return eng.result(), eng.vector_sums(), eng.frame_sums(), eng.stats()
    finally:
        eng.close()


def assert_same(got, want):
    """got: engine_run's tuple; want: restate's."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[3]["evaluations"] == want[3] and got[3]["degenerate"] == 0


def diffusing(seed, F, n, step=1.2):
    """A free random walk, float32[F, n, 3]."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 40.0, (1, n, 3)) + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)).astype(np.float32)


def random_pairs(seed, V, n_rows):
    """int32 [V, 2]: tail != head, rows shared between vectors, in no order."""
    rng = np.random.default_rng(seed)
    tail = rng.integers(0, n_rows, V)
    head = (tail + rng.integers(1, n_rows, V)) % n_rows
    return np.stack((tail, head), axis=1).astype(np.int32)


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("V", [1, 63, 64, 65, 2 * T + 3])
def test_engine_group_sizes_and_frame_counts(V):
    n_rows = V + 3
    pairs = random_pairs(V, V, n_rows)
    for F in (1, 2, 37):
        pos = diffusing(100 + V, F, n_rows)
        want = restate(pos, [V], pairs, LAGS)
        got = engine_run(pos, [V], pairs, LAGS)
        assert_same(got, want)
        assert got[3]["frames"] == F and got[2].shape == (F, 1, 6)
        assert want[3] == V * sum(max(F - lag, 0) for lag in LAGS)
        assert not got[0][5].any() and not got[1][5].any()          # lag 40: no origin
        # lag 0: c is 1 to rounding and the traces of the products add up to the number of vectors, within the
        # n * 2^-53 of n float64 additions (n <= 131 * 37 < 2^13: 2^-40 < 1e-12)
        np.testing.assert_allclose(got[0][0, 0], [V * F, V * F], rtol=1e-12)
        np.testing.assert_allclose(got[2][:, 0, [0, 3, 5]].sum(axis=-1), V, rtol=1e-12)


def test_engine_three_unequal_groups():
    sizes = [1, 65, 65]
    V, F = sum(sizes), 37
    n_rows = V + 3
    pairs = random_pairs(7, V, n_rows)
    pos = diffusing(7, F, n_rows)
    got = engine_run(pos, sizes, pairs, LAGS)
    assert_same(got, restate(pos, sizes, pairs, LAGS))
    # the rows of a group do not depend on what the other groups are: the tiles never span two groups
    for g, (lo, hi) in enumerate(((0, 1), (1, 66), (66, V))):
        solo = engine_run(pos, [hi - lo], pairs[lo:hi], LAGS)
        np.testing.assert_array_equal(solo[0][:, 0], got[0][:, g])
        np.testing.assert_array_equal(solo[1], got[1][:, lo:hi])
        np.testing.assert_array_equal(solo[2][:, 0], got[2][:, g])
    # an empty group between them: zero rows, the others unchanged
    wide = engine_run(pos, [1, 0, 65, 65], pairs, LAGS)
    np.testing.assert_array_equal(wide[0][:, [0, 2, 3]], got[0])
    np.testing.assert_array_equal(wide[2][:, [0, 2, 3]], got[2])
    np.testing.assert_array_equal(wide[1], got[1])
    assert not wide[0][:, 1].any() and not wide[2][:, 1].any()
    eng = _core.OrientationEngine(sizes, pairs, n_rows, LAGS)
    try:
        with pytest.raises(ValueError, match="50 rows given"):
            eng.accumulate(pos[:, :50])                             # wrong number of rows
    finally:
        eng.close()


BOX = np.array([31.0, 44.5, 57.25])
BOX_SIZES = [1, 65, 65]


def _bonds_across_the_faces(seed, F, V, dims):
    """Bonds of length 1 ... 2 that turn from frame to frame, their tails within 0.2 of a face: vector v sits at the
    upper (v // 3 even) or lower face of component v % 3.  Rows 2v (tail) and 2v + 1 (head), wrapped into the box:
    float32[F, 2V, 3]."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 0.9, (V, 3)) * dims
    v = np.arange(V)
    base[v, v % 3] = np.where(v // 3 % 2 == 0, dims[v % 3] - 0.2, 0.2)
    tails = base + rng.normal(0.0, 0.02, (F, V, 3))
    turn = rng.normal(0.0, 1.0, (1, V, 3)) + np.cumsum(rng.normal(0.0, 0.3, (F, V, 3)), axis=0)
    turn[:, v, v % 3] += np.where(v // 3 % 2 == 0, 1.0, -1.0)          # more often than not towards the face
    turn /= np.sqrt((turn * turn).sum(axis=-1, keepdims=True))
    heads = tails + turn * rng.uniform(1.0, 2.0, (1, V, 1))
    true = np.stack((tails, heads), axis=2).reshape(F, 2 * V, 3)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


@pytest.fixture(scope="module")
def bonds():
    """Frames, pairs and the restatement with and without the box, shared and left unchanged."""
    V = sum(BOX_SIZES)
    pos = _bonds_across_the_faces(11, 37, V, BOX)
    pairs = np.stack((2 * np.arange(V), 2 * np.arange(V) + 1), axis=1).astype(np.int32)
    want = restate(pos, BOX_SIZES, pairs, LAGS, dims=BOX)
    raw = restate(pos, BOX_SIZES, pairs, LAGS)
    for a in (pos, pairs, *want[:3], *raw[:3]):
        a.setflags(write=False)
    return {"pos": pos, "pairs": pairs, "want": want, "raw": raw}


def test_box_input_cannot_pass_with_the_box_off(bonds):
    """What the test asserts of its own input, so that the minimum-image cases mean something."""
    x = bonds["pos"].astype(np.float64)
    d = x[:, bonds["pairs"][:, 1]] - x[:, bonds["pairs"][:, 0]]
    for c in range(3):
        assert (d[..., c] > BOX[c] / 2).any() and (d[..., c] < -BOX[c] / 2).any()      # both signs straddle
    w = d - BOX * np.rint(d * (1.0 / BOX))
    length = np.sqrt((w * w).sum(axis=-1))
    assert 0.99 < length.min() and length.max() < 2.01
    lo = 0
    for g, size in enumerate(BOX_SIZES):                                    # every group has bonds across a face
        assert (np.abs(d[:, lo:lo + size]) > BOX / 2).any()
        assert (bonds["want"][0][1:5, g] != bonds["raw"][0][1:5, g]).any()
        assert (bonds["want"][2][:, g] != bonds["raw"][2][:, g]).any()
        lo += size


def test_box_against_the_rule(bonds):
    pos, pairs = bonds["pos"], bonds["pairs"]
    assert_same(engine_run(pos, BOX_SIZES, pairs, LAGS, setup=lambda e: e.set_box(BOX)), bonds["want"])
    assert_same(engine_run(pos, BOX_SIZES, pairs, LAGS), bonds["raw"])
    eng = _core.OrientationEngine(BOX_SIZES, pairs, pos.shape[1], LAGS)
    try:
        eng.accumulate(pos[:4])
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_box(BOX)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_box(None)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(8)
        eng.reset()
        eng.set_box(BOX)
        eng.set_slab_frames(8)
        eng.accumulate(pos)
        np.testing.assert_array_equal(eng.result(), bonds["want"][0])
        np.testing.assert_array_equal(eng.frame_sums(), bonds["want"][2])
    finally:
        eng.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(bonds, axis):
    pos, pairs = bonds["pos"], bonds["pairs"]
    want = restate(pos, BOX_SIZES, pairs, LAGS, dims=BOX, zero_dims=1 << axis)
    got = engine_run(pos, BOX_SIZES, pairs, LAGS, setup=lambda e: e.set_box(BOX), zero_dims=1 << axis)
    assert_same(got, want)
    assert (want[0] != bonds["want"][0])[1:5].any()
    dropped = [q for q, ab in enumerate(PRODUCTS) if axis in ab]
    assert not got[2][:, :, dropped].any()
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    level = engine_run(flat, BOX_SIZES, pairs, LAGS, setup=lambda e: e.set_box(BOX))
    for a, b in zip(level[:3], got[:3]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("boxed", [False, True])
def test_one_set_of_bits_whatever_the_split_slab_route_or_index(bonds, boxed, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, pairs, sizes = bonds["pos"], bonds["pairs"], BOX_SIZES
    F, n = pos.shape[:2]
    want = bonds["want" if boxed else "raw"]

    def setup(e, slab=None):
        if boxed:
            e.set_box(BOX)
        if slab is not None:
            e.set_slab_frames(slab)

    def same(eng):
        np.testing.assert_array_equal(eng.result(), want[0])
        np.testing.assert_array_equal(eng.vector_sums(), want[1])
        np.testing.assert_array_equal(eng.frame_sums(), want[2])
        assert eng.stats()["evaluations"] == want[3] and eng.stats()["frames"] == F

    run = lambda **kw: engine_run(pos, sizes, pairs, LAGS, **kw)      # noqa: E731
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
    lengths, angles = np.tile(BOX, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.OrientationEngine(sizes, pairs, n, LAGS)
    try:
        setup(eng)
        eng.accumulate_device(d.ptr, n, F)
        same(eng)                                                   # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.stats()["evaluations"] == 0
        assert not eng.result().any() and not eng.vector_sums().any() and eng.frame_sums().shape == (0, 3, 6)
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


@pytest.mark.parametrize("slab", [1, 8])
def test_the_ring_wraps(bonds, slab):
    """With lags up to 5 the ring holds 5 + slab frames, fewer than the 37 fed: every slot is written several times,
    and a lag reaches back across the wrap."""
    pos, pairs, lags = bonds["pos"], bonds["pairs"], [0, 1, 2, 5]
    assert lags[-1] + slab < len(pos) // 2
    want = restate(pos, BOX_SIZES, pairs, lags, dims=BOX)
    for k, lag in enumerate(lags):                                  # the lags the fixture shares: the same rows
        np.testing.assert_array_equal(want[1][k], bonds["want"][1][LAGS.index(lag)])

    def setup(e):
        e.set_box(BOX)
        e.set_slab_frames(slab)

    assert_same(engine_run(pos, BOX_SIZES, pairs, lags, setup=setup), want)
    assert_same(engine_run(pos, BOX_SIZES, pairs, lags, splits=[0, 1, 5, 37], setup=setup), want)


def test_a_vector_without_a_direction_refuses_the_results(bonds):
    """Data, not a fault: in one frame the head of one vector lies on its tail."""
    pos, pairs = bonds["pos"], bonds["pairs"]
    bad = pos.copy()
    bad[3, pairs[70, 1]] = bad[3, pairs[70, 0]]
    eng = _core.OrientationEngine(BOX_SIZES, pairs, pos.shape[1], LAGS)
    try:
        eng.set_box(BOX)
        eng.accumulate(bad)
        for read in (eng.result, eng.vector_sums, eng.frame_sums, eng.synchronize):
            with pytest.raises(ValueError, match="1 vectors had no direction"):
                read()
        stats = eng.stats()
        assert stats["degenerate"] == 1 and stats["frames"] == len(pos)
        eng.accumulate(pos[:2])                                     # still refused: only a reset starts over
        with pytest.raises(ValueError, match="had no direction"):
            eng.result()
        eng.reset()
        assert eng.stats()["degenerate"] == 0
        eng.accumulate(pos)
        np.testing.assert_array_equal(eng.result(), bonds["want"][0])
        np.testing.assert_array_equal(eng.vector_sums(), bonds["want"][1])
        np.testing.assert_array_equal(eng.frame_sums(), bonds["want"][2])
        assert eng.stats()["degenerate"] == 0
    finally:
        eng.close()


# ---------------------------------------------------------------- physics

def test_rigid_rotation_about_z():
    """Bonds of length b = 1 in the xy plane that all turn about z by phi = 0.1 rad per frame: C_1(k) = cos(k phi),
    C_2(k) = (3 cos^2(k phi) - 1) / 2."""
    phi, b, F, V = 0.1, 1.0, 37, 200
    lags = np.array([0, 1, 2, 5, 36])
    rng = np.random.default_rng(5)
    tails = rng.integers(-255, 256, (V, 3)) * 0.25                  # on a grid of 0.25, |x| < 64: exact in float32
    assert np.abs(tails).max() < 64
    angle = rng.uniform(0.0, 2 * np.pi, V)[None, :] + phi * np.arange(F)[:, None]
    heads = tails + b * np.stack((np.cos(angle), np.sin(angle), np.zeros_like(angle)), axis=-1)
    pos = np.empty((F, 2 * V, 3), dtype=np.float32)
    pos[:, 0::2], pos[:, 1::2] = tails, heads
    np.testing.assert_array_equal(pos[:, 0::2].astype(np.float64), np.broadcast_to(tails, (F, V, 3)))
    pairs = np.stack((2 * np.arange(V), 2 * np.arange(V) + 1), axis=1).astype(np.int32)
    sums, _, _, _ = engine_run(pos, [V], pairs, lags)
    terms = ((F - lags) * V).astype(float)
    c1, c2 = sums[:, 0, 0] / terms, sums[:, 0, 1] / terms

    # the float64 definition on the float32-rounded positions, vectorised: only the order of the sums differs
    u = unit_vectors(pos, pairs)
    for k, lag in enumerate(lags):
        c = (u[lag:] * u[:F - lag]).sum(axis=-1)
        np.testing.assert_allclose(c1[k], c.mean(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(c2[k], (1.5 * c * c - 0.5).mean(), rtol=1e-12, atol=0)

    # The closed forms, within what rounding the heads to float32 allows.  The tails are exact.  A head coordinate
    # lies below 64 + b < 128, where float32 numbers are 2^-17 apart: it moves by at most delta = 2^-18 =
    # 2^-24 * max|x| with max|x| = 64, so the bond w moves by at most sqrt(3) delta and the unit vector by at most
    # e = 2 sqrt(3) delta / b  (|w'/|w'| - w/|w|| <= 2 |w' - w| / |w|).  Then, with |u| = 1,
    #   |dc| <= 2 e + e^2                          for c = u(f) . u(f - lag)
    #   |d(1.5 c^2 - 0.5)| <= 1.5 (2 |dc| + dc^2)  since |c| <= 1
    # and the same bounds hold for the averages; the float64 rounding of the engine's own operations (a few
    # 2^-53 per term) is covered by the 1e-12 above, added here.
    delta = 2.0 ** -24 * 64
    e = 2 * np.sqrt(3.0) * delta / b
    dc = 2 * e + e * e
    cos = np.cos(lags * phi)
    assert np.abs(c1 - cos).max() <= dc + 1e-12
    assert np.abs(c2 - (3 * cos * cos - 1) / 2).max() <= 1.5 * (2 * dc + dc * dc) + 1e-12


def test_vectors_along_z_are_perfectly_ordered():
    F, V = 5, 70
    rng = np.random.default_rng(6)
    tails = rng.integers(-255, 256, (V, 3)) * 0.25
    heads = tails + np.where(np.arange(V) % 2 == 0, 1.0, -1.0)[:, None] * np.array([0.0, 0.0, 1.0])
    pos = np.broadcast_to(np.concatenate((tails, heads))[None], (F, 2 * V, 3)).astype(np.float32)
    u = mdhelper_amd.ArrayUniverse(pos, None, dt=1.0)
    o = OrientationalRelaxation(u.select(np.arange(V)), u.select(np.arange(V, 2 * V)), minimum_image=False,
                                verbose=False).run()
    assert np.all(o.results.order_parameter == 1.0) and o.results.order_parameter.shape == (F, 1)
    np.testing.assert_array_equal(np.abs(o.results.director), np.broadcast_to([0.0, 0.0, 1.0], (F, 1, 3)))
    np.testing.assert_array_equal(o.results.order_tensor, np.broadcast_to(np.diag([-0.5, -0.5, 1.0]), (F, 1, 3, 3)))
    assert np.all(o.results.c1 == 1.0) and np.all(o.results.c2 == 1.0)


# ---------------------------------------------------------------- the class

def test_class_groups_routes_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    F, n = 12, 170
    pos = diffusing(20, F, n, step=0.8)
    dims = np.array([60.0, 50.0, 40.0])
    boxes = np.tile(np.array([*dims, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    # two groups given in an order that is not the frame's; the first is a run of bonds that share their atoms
    t0, h0 = np.arange(90, 90 + T + 5), np.arange(91, 91 + T + 5)
    t1, h1 = np.arange(70, 0, -1), np.arange(5, 75)
    sizes = [len(t0), len(t1)]
    index, inverse = np.unique(np.concatenate((t0, t1, h0, h1)), return_inverse=True)
    pairs = np.stack((inverse[:sum(sizes)], inverse[sum(sizes):]), axis=1)
    lags = np.array([0, 1, 3, 11, 15])
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)

    def check(o, frames, step):
        """o.results against the restatement on the selected frames."""
        sums, _, frame_sums, _ = restate(pos[frames][:, index], sizes, pairs, lags, dims=dims)
        res = o.results
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        terms = np.maximum(len(frames) - lags, 0).astype(float)[:, None] * np.array(sizes)[None, :]
        terms[terms == 0] = np.nan
        np.testing.assert_array_equal(res.c1, sums[..., 0] / terms)
        np.testing.assert_array_equal(res.c2, sums[..., 1] / terms)
        live = lags < len(frames)
        assert np.isnan(res.c1[~live]).all() and np.isnan(res.c2[~live]).all() and not np.isnan(res.c1[live]).any()
        np.testing.assert_allclose(res.c1[0], 1.0, rtol=1e-14)
        mean = np.zeros((len(frames), 2, 3, 3))
        for q, (a, b) in enumerate(PRODUCTS):
            mean[..., a, b] = mean[..., b, a] = frame_sums[..., q] / np.array(sizes)
        tensor = 1.5 * mean - 0.5 * np.eye(3)
        np.testing.assert_array_equal(res.order_tensor, tensor)
        np.testing.assert_array_equal(res.order_parameter, np.linalg.eigvalsh(tensor)[..., -1])
        assert res.director.shape == (len(frames), 2, 3)
        np.testing.assert_allclose((res.director ** 2).sum(axis=-1), 1.0, rtol=1e-14)
        np.testing.assert_allclose(np.einsum("fgab,fgb->fga", tensor, res.director),
                                   res.order_parameter[..., None] * res.director, atol=1e-14)
        assert set(res.units) == {"results.times", "results.relaxation_times"}

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            tails, heads = [u.select(t0), u.select(t1)], [u.select(h0), u.select(h1)]
            make = lambda: OrientationalRelaxation(tails, heads, lags=lags, verbose=False)      # noqa: E731
            full = make().run()
            check(full, np.arange(F), 1)
            check(make().run(start=1, stop=12, step=2), np.arange(1, 12, 2), 2)
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in ("c1", "c2", "order_tensor", "order_parameter", "director"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        tails, heads = [u.select(t0), u.select(t1)], [u.select(h0), u.select(h1)]
        # neither lags nor n_lags: every analysed frame is a lag
        every = OrientationalRelaxation(tails, heads, verbose=False).run()
        sums, _, _, _ = restate(pos[:, index], sizes, pairs, np.arange(F), dims=dims)
        np.testing.assert_array_equal(every.results.c2,
                                      sums[..., 1] / ((F - np.arange(F))[:, None] * np.array(sizes)[None, :]))
        few = OrientationalRelaxation(tails, heads, n_lags=4, verbose=False).run()
        np.testing.assert_array_equal(few.results.c1, every.results.c1[:4])
        # the relaxation times are the existing trapezoid helper, column by column
        every.calculate_relaxation_times()
        want = [[calculate_residence_time(every.results.times, c[:, g]) for g in range(2)]
                for c in (every.results.c1, every.results.c2)]
        np.testing.assert_array_equal(every.results.relaxation_times, want)
        assert every.results.relaxation_times.shape == (2, 2)
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(OrientationalRelaxation(tails, heads, lags=lags, verbose=False)).run()
        for key in ("c1", "c2", "order_tensor", "order_parameter"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # without the box the vectors are the raw differences
        raw = OrientationalRelaxation(tails, heads, lags=lags, minimum_image=False, verbose=False).run()
        sums, _, _, _ = restate(pos[:, index], sizes, pairs, lags)
        terms = np.maximum(F - lags, 0).astype(float)[:, None] * np.array(sizes)[None, :]
        terms[terms == 0] = np.nan
        np.testing.assert_array_equal(raw.results.c1, sums[..., 0] / terms)
        with pytest.raises(ValueError, match="evenly spaced"):
            OrientationalRelaxation(tails, heads, verbose=False).run(frames=[0, 1, 3])
    finally:
        d.free()


def test_class_from_chains_and_drop_axis():
    n_chains, n_monomers, F = 3, 7, 9
    n = n_chains * n_monomers
    pos = diffusing(21, F, n + 4, step=0.5)
    dims = np.array([60.0, 50.0, 40.0])
    u = mdhelper_amd.ArrayUniverse(pos, [*dims, 90.0, 90.0, 90.0], dt=2.0)
    ag = u.select(np.arange(2, 2 + n))
    for stride in (1, 3):
        chains = OrientationalRelaxation.from_chains(ag, n_chains, n_monomers, stride=stride, n_lags=5,
                                                     verbose=False).run()
        place = np.arange(n).reshape(n_chains, n_monomers)
        tails, heads = ag[place[:, :-stride].ravel()], ag[place[:, stride:].ravel()]
        explicit = OrientationalRelaxation(tails, heads, n_lags=5, verbose=False).run()
        for key in ("c1", "c2", "order_tensor", "order_parameter", "director", "times"):
            np.testing.assert_array_equal(chains.results[key], explicit.results[key])
        V = n_chains * (n_monomers - stride)
        index, inverse = np.unique(np.concatenate((tails.indices, heads.indices)), return_inverse=True)
        pairs = np.stack((inverse[:V], inverse[V:]), axis=1)
        sums, _, _, _ = restate(pos[:, index], [V], pairs, np.arange(5), dims=dims)
        np.testing.assert_array_equal(chains.results.c1, sums[..., 0] / ((F - np.arange(5))[:, None] * V))
        np.testing.assert_array_equal(chains.results.times, np.arange(5) * 2.0)
    # drop_axis: the two-dimensional tensor 2 <u u^T> - I on the kept components
    flat = OrientationalRelaxation.from_chains(ag, n_chains, n_monomers, n_lags=5, drop_axis="y", verbose=False).run()
    V = n_chains * (n_monomers - 1)
    tails, heads = ag[place[:, :-1].ravel()], ag[place[:, 1:].ravel()]
    index, inverse = np.unique(np.concatenate((tails.indices, heads.indices)), return_inverse=True)
    pairs = np.stack((inverse[:V], inverse[V:]), axis=1)
    sums, _, frame_sums, _ = restate(pos[:, index], [V], pairs, np.arange(5), dims=dims, zero_dims=2)
    np.testing.assert_array_equal(flat.results.c2, sums[..., 1] / ((F - np.arange(5))[:, None] * V))
    tensor = np.zeros((F, 1, 3, 3))
    tensor[..., 0, 0] = 2.0 * (frame_sums[..., 0] / V) - 1.0
    tensor[..., 2, 2] = 2.0 * (frame_sums[..., 5] / V) - 1.0
    tensor[..., 0, 2] = tensor[..., 2, 0] = 2.0 * (frame_sums[..., 2] / V) - 0.0
    np.testing.assert_array_equal(flat.results.order_tensor, tensor)
    small = tensor[..., [0, 2], :][..., [0, 2]]
    np.testing.assert_array_equal(flat.results.order_parameter, np.linalg.eigvalsh(small)[..., -1])
    assert np.all(flat.results.order_parameter >= 0) and not flat.results.director[..., 1].any()
    np.testing.assert_allclose((flat.results.director ** 2).sum(axis=-1), 1.0, rtol=1e-14)
