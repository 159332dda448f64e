"""
Dihedrals / DihedralEngine on the GPU against the float64 NumPy restatement of the device contract in
``dihedral_cases.py`` (csrc/mdx_dihedral_device.hpp): the same operations in the same order, the accumulator of every
(lag, dihedral) taking its terms from a Python loop over the frames and a group's sum adding its dihedrals from a
Python loop over the rows.  Every comparison with the restatement uses ``assert_array_equal``: there is no tolerance
(the rigid-torsion test has a bound, derived where it stands).

What the inputs are asserted to be before they are used stands in ``test_the_input_exercises_the_contract``.  One
property asked of them cannot hold and is replaced by the identity that holds instead: ``run(f) >= 1`` exactly where
``state(f) == state(f - 1)``, so ``stay == same`` at lags 0 and 1 whatever the data; ``0 < stay < same < cases`` is
asserted at lags 2 and 5, and ``0 < stay == same < cases`` at lag 1.
"""
import numpy as np
import pytest

import dihedral_cases as dc
import mdhelper_amd
from dihedral_cases import BOX, KEYS, LAGS
from mdhelper_amd import _core
from mdhelper_amd.analysis import Dihedrals, calculate_residence_time
from mdhelper_amd.analysis.dihedral import cosine_thresholds, states_of_bins

pytestmark = pytest.mark.gpu

T = _core.DihedralEngine.TILE
SIZES = [1, 65, 65]
EDGES = (-120.0, 0.0, 120.0)
PAST_LDS = _core.DihedralEngine.LDS_BINS + 2       # the first even bin count the LDS histogram does not take


def read(eng):
    got = eng.result()
    got.update(acc=eng.dihedral_sums(), counts=eng.counts(), state_counts=eng.state_counts(),
               transitions=eng.transitions(), stats=eng.stats())
    return got


def make(sizes, quads, n_rows, lags, *, n_bins=180, state_edges=EDGES):
    return _core.DihedralEngine(sizes, quads, n_rows, cosine_thresholds(n_bins), states_of_bins(n_bins, state_edges),
                                lags, n_states=len(state_edges))


def engine_run(pos, sizes, quads, lags, *, splits=None, setup=None, **kwargs):
    eng = make(sizes, quads, pos.shape[1], lags, **kwargs)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return read(eng)
    finally:
        eng.close()


def assert_same(got, want):
    """got: read's dict; want: restate's."""
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["stats"]["evaluations"] == want["evaluations"] and got["stats"]["degenerate"] == 0


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("D", [1, 63, 64, 65, 2 * T + 3])
def test_engine_group_sizes_and_frame_counts(D):
    for F in (1, 2, 37):
        pos, quads = dc.chains(100 + D, F, [D])
        want = dc.restate(pos, [D], quads, LAGS, dims=BOX)
        got = engine_run(pos, [D], quads, LAGS, setup=lambda e: e.set_box(BOX))
        assert_same(got, want)
        assert got["stats"]["frames"] == F and got["state_counts"].shape == (F, 1, 3)
        assert want["evaluations"] == D * sum(max(F - lag, 0) for lag in LAGS)
        assert not got["sums"][5].any() and not got["same"][5].any() and not got["stay"][5].any()   # lag 40: no origin
        # lag 0: cos^2 + sin^2 is 1 to rounding, every case is in its own state and has run at least 0 frames
        np.testing.assert_allclose(got["sums"][0, 0], D * F, rtol=1e-12)
        assert got["same"][0, 0] == got["stay"][0, 0] == D * F == got["counts"].sum() == got["state_counts"].sum()
        assert got["transitions"].sum() == D * (F - 1)


@pytest.fixture(scope="module")
def chains():
    """Frames, quads and the restatement with and without the box, shared and left unchanged."""
    pos, quads = dc.chains(7, 37, SIZES)
    want = dc.restate(pos, SIZES, quads, LAGS, dims=BOX)
    raw = dc.restate(pos, SIZES, quads, LAGS)
    for a in (pos, quads, *(want[k] for k in KEYS), *(raw[k] for k in KEYS)):
        a.setflags(write=False)
    return {"pos": pos, "quads": quads, "want": want, "raw": raw}


def test_the_input_exercises_the_contract(chains):
    """What the tests assert of their own input, so that the cases mean something."""
    pos, quads, want, raw = chains["pos"], chains["quads"], chains["want"], chains["raw"]
    F = len(pos)
    c, s, q, mn = dc.geometry(pos, quads, BOX)
    assert np.all(mn > 0) and np.all(np.isfinite(mn))               # no degenerate dihedral
    b = dc.bond_vectors(pos, quads, BOX)
    length = np.sqrt((b * b).sum(axis=-1))
    assert 1.49 < length.min() and length.max() < 1.51              # the minimum image restores the bonds
    angle = np.degrees(np.arccos(-(b[0] * b[1]).sum(axis=-1) / (length[0] * length[1])))
    assert 109.9 < angle.min() and angle.max() < 110.1
    d = dc.bond_vectors(pos, quads)
    for k in range(3):                                              # bonds straddle both faces of every component
        assert (d[..., k] > BOX[k] / 2).any() and (d[..., k] < -BOX[k] / 2).any()
    lo = 0
    for g, size in enumerate(SIZES):
        rows = slice(lo, lo + size)
        lo += size
        assert set(np.unique(want["state"][:, rows])) == {0, 1, 2}  # all three default states
        assert (q[:, rows] < 0).any() and (q[:, rows] > 0).any()    # both signs of q
        moves = want["transitions"][g]
        assert moves.sum() - np.trace(moves) > 0                    # some off-diagonal transitions
        for k in (2, 3):                                            # lags 2 and 5: the run logic decides
            assert 0 < want["stay"][k, g] < want["same"][k, g] < size * (F - LAGS[k])
        assert 0 < want["stay"][1, g] == want["same"][1, g] < size * (F - 1)    # lag 1: an identity (docstring)
        assert (np.abs(d[:, :, rows]) > BOX / 2).any()              # every group has bonds across a face
        assert (want["sums"][1:4, g] != raw["sums"][1:4, g]).any()  # ... and cannot pass with the box off
        assert (want["counts"][g] != raw["counts"][g]).any()
    dc.check_threshold_rule_against_atan2()


def test_three_unequal_groups(chains):
    pos, quads = chains["pos"], chains["quads"]
    boxed = lambda e: e.set_box(BOX)        # noqa: E731
    got = engine_run(pos, SIZES, quads, LAGS, setup=boxed)
    assert_same(got, chains["want"])
    assert_same(engine_run(pos, SIZES, quads, LAGS), chains["raw"])
    # the rows of a group do not depend on what the other groups are: the tiles never span two groups
    for g, (lo, hi) in enumerate(((0, 1), (1, 66), (66, 131))):
        solo = engine_run(pos, [hi - lo], quads[lo:hi], LAGS, setup=boxed)
        for key in ("sums", "same", "stay"):
            np.testing.assert_array_equal(solo[key][:, 0], got[key][:, g])
        np.testing.assert_array_equal(solo["acc"], got["acc"][:, lo:hi])
        np.testing.assert_array_equal(solo["counts"][0], got["counts"][g])
        np.testing.assert_array_equal(solo["state_counts"][:, 0], got["state_counts"][:, g])
        np.testing.assert_array_equal(solo["transitions"][0], got["transitions"][g])
    # an empty group between them: zero rows, the others unchanged
    wide = engine_run(pos, [1, 0, 65, 65], quads, LAGS, setup=boxed)
    for key in ("sums", "same", "stay"):
        np.testing.assert_array_equal(wide[key][:, [0, 2, 3]], got[key])
        assert not wide[key][:, 1].any()
    np.testing.assert_array_equal(wide["acc"], got["acc"])
    np.testing.assert_array_equal(wide["counts"][[0, 2, 3]], got["counts"])
    np.testing.assert_array_equal(wide["state_counts"][:, [0, 2, 3]], got["state_counts"])
    np.testing.assert_array_equal(wide["transitions"][[0, 2, 3]], got["transitions"])
    assert not wide["counts"][1].any() and not wide["state_counts"][:, 1].any() and not wide["transitions"][1].any()
    eng = make(SIZES, quads, pos.shape[1], LAGS)
    try:
        with pytest.raises(ValueError, match="50 rows given"):
            eng.accumulate(pos[:, :50])                             # wrong number of rows
    finally:
        eng.close()


@pytest.mark.parametrize("n_bins,state_edges", [(2, (-180.0, 0.0)), (180, EDGES),
                                                (_core.DihedralEngine.LDS_BINS, (-90.0, 0.0, 90.0)),
                                                (PAST_LDS, (-180.0, 0.0))])
def test_both_histogram_routes(chains, n_bins, state_edges):
    """The per-wave LDS histogram up to LDS_BINS bins and the direct one beyond, with G = 3."""
    pos, quads = chains["pos"], chains["quads"]
    want = dc.restate(pos, SIZES, quads, LAGS, n_bins=n_bins, state_edges=state_edges, dims=BOX)
    got = engine_run(pos, SIZES, quads, LAGS, n_bins=n_bins, state_edges=state_edges, setup=lambda e: e.set_box(BOX))
    assert_same(got, want)
    assert got["counts"].shape == (3, n_bins) and got["counts"].sum() == 131 * 37
    np.testing.assert_array_equal(got["acc"], chains["want"]["acc"])        # c and s do not depend on the bins
    if n_bins > 2:
        assert (np.count_nonzero(got["counts"], axis=1) > min(n_bins, 37) // 2).all()


def test_set_box_and_slab_only_before_the_first_frame(chains):
    pos, quads, want = chains["pos"], chains["quads"], chains["want"]
    eng = make(SIZES, quads, pos.shape[1], LAGS)
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
        assert eng.plan() == {"slab_frames": 8, "ring_frames": 48}
        eng.accumulate(pos)
        assert_same(read(eng), want)
    finally:
        eng.close()


@pytest.mark.parametrize("boxed", [False, True])
def test_one_set_of_bits_whatever_the_split_slab_route_or_index(chains, boxed, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, quads = chains["pos"], chains["quads"]
    F, n = pos.shape[:2]
    want = chains["want" if boxed else "raw"]

    def setup(e, slab=None):
        if boxed:
            e.set_box(BOX)
        if slab is not None:
            e.set_slab_frames(slab)

    def same(eng):
        assert_same(read(eng), want)
        assert eng.stats()["frames"] == F

    run = lambda **kw: engine_run(pos, SIZES, quads, LAGS, **kw)      # noqa: E731
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
    eng = make(SIZES, quads, n, LAGS)
    try:
        setup(eng)
        eng.accumulate_device(d.ptr, n, F)
        same(eng)                                                   # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.stats()["evaluations"] == 0
        empty = read(eng)
        assert not any(empty[key].any() for key in KEYS) and empty["state_counts"].shape == (0, 3, 3)
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
        eng.accumulate(big[:, index])
        same(eng)                                                   # host, the rows picked by the caller
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
def test_the_ring_wraps(chains, slab):
    """With lags up to 5 the rings hold 5 + slab frames, fewer than the 37 fed: every slot is written several times,
    a lag reaches back across the wrap, and so does the run length from one slab to the next."""
    pos, quads, lags = chains["pos"], chains["quads"], [0, 1, 2, 5]
    assert lags[-1] + slab < len(pos) // 2
    want = dc.restate(pos, SIZES, quads, lags, dims=BOX)
    for k, lag in enumerate(lags):                                  # the lags the fixture shares: the same rows
        np.testing.assert_array_equal(want["acc"][k], chains["want"]["acc"][LAGS.index(lag)])

    def setup(e):
        e.set_box(BOX)
        e.set_slab_frames(slab)
        assert e.plan() == {"slab_frames": slab, "ring_frames": 5 + slab}

    assert_same(engine_run(pos, SIZES, quads, lags, setup=setup), want)
    assert_same(engine_run(pos, SIZES, quads, lags, splits=[0, 1, 5, 37], setup=setup), want)

    def lone(e):            # lag 0 alone: the ring still holds the frame before the slab, for the run length
        e.set_box(BOX)
        e.set_slab_frames(slab)
        assert e.plan() == {"slab_frames": slab, "ring_frames": 1 + slab}

    got = engine_run(pos, SIZES, quads, [0], setup=lone)
    np.testing.assert_array_equal(got["transitions"], want["transitions"])
    np.testing.assert_array_equal(got["stay"], want["stay"][:1])


def test_a_dihedral_without_an_angle_refuses_the_results(chains):
    """Data, not a fault: in one frame three atoms of the lone dihedral of group 0 lie on a line, on a grid of 0.25
    that float32 holds exactly."""
    pos, quads, want = chains["pos"], chains["quads"], chains["want"]
    bad = pos.copy()
    a, b, c, _ = quads[0]
    bad[3, a], bad[3, b], bad[3, c] = (1.0, 1.25, 1.5), (1.25, 1.75, 2.25), (1.75, 2.75, 3.75)
    np.testing.assert_array_equal(np.cross(bad[3, b] - bad[3, a], bad[3, c] - bad[3, b]), 0.0)
    assert dc.geometry(bad, quads, BOX)[3][3, 0] == 0.0 and np.count_nonzero(dc.geometry(bad, quads, BOX)[3] > 0) == \
        bad.shape[0] * len(quads) - 1
    eng = make(SIZES, quads, pos.shape[1], LAGS)
    try:
        eng.set_box(BOX)
        eng.accumulate(bad)
        for call in (eng.result, eng.dihedral_sums, eng.counts, eng.state_counts, eng.transitions, eng.synchronize):
            with pytest.raises(ValueError, match="1 dihedrals had no angle"):
                call()
        stats = eng.stats()
        assert stats["degenerate"] == 1 and stats["frames"] == len(pos)
        eng.accumulate(pos[:2])                                     # still refused: only a reset starts over
        with pytest.raises(ValueError, match="had no angle"):
            eng.result()
        with pytest.raises(ValueError, match="had no angle"):
            eng.counts()
        eng.reset()
        assert eng.stats()["degenerate"] == 0
        eng.accumulate(pos)
        assert_same(read(eng), want)
    finally:
        eng.close()


# ---------------------------------------------------------------- closed forms

def test_a_planar_zigzag_is_all_trans():
    """Atoms at (1.25 i, 0.75 (i % 2), 0), exact in float32: m and n are antiparallel along z, m2 = n2 = 3.515625 and
    their product is a square float64 holds exactly, so c == -1.0, q == +-0 and every dihedral lands in the last
    bin."""
    n, F = 70, 3
    i = np.arange(n)
    pos = np.broadcast_to(np.stack((1.25 * i, 0.75 * (i % 2), np.zeros(n)), axis=1), (F, n, 3)).astype(np.float32)
    quads = (np.arange(n - 3)[:, None] + np.arange(4)[None, :]).astype(np.int32)
    c, s, q, _ = dc.geometry(pos, quads)
    assert np.all(c == -1.0) and np.all(q == 0.0) and np.all(s == 0.0)
    for n_bins in (2, 180):
        got = engine_run(pos, [n - 3], quads, [0, 1], n_bins=n_bins, state_edges=(-180.0, 0.0))
        want = np.zeros((1, n_bins), dtype=np.int64)
        want[0, -1] = (n - 3) * F
        np.testing.assert_array_equal(got["counts"], want)
        np.testing.assert_array_equal(got["sums"], [[(n - 3) * 3.0], [(n - 3) * 2.0]])      # c * c = 1 exactly
        np.testing.assert_array_equal(got["state_counts"][:, 0], [[0, n - 3]] * F)


def _torsion_rows(phi, tails):
    """Rows (a, b, c, d) = t + (1, 0, 0), t, t + (0, 0, 1), t + (cos phi, sin phi, 1) for phi [F, D] (radians) and
    tails t [D, 3]: float32 [F, 4 D, 3], dihedral v on rows 4 v ... 4 v + 3.  Its angle is phi (IUPAC sign)."""
    F, D = phi.shape
    pos = np.empty((F, D, 4, 3))
    pos[:, :, 0] = tails + (1.0, 0.0, 0.0)
    pos[:, :, 1] = tails
    pos[:, :, 2] = tails + (0.0, 0.0, 1.0)
    pos[:, :, 3] = tails + np.stack((np.cos(phi), np.sin(phi), np.ones_like(phi)), axis=-1)
    return pos.reshape(F, 4 * D, 3).astype(np.float32)


def _torsion_quads(D):
    return np.arange(4 * D, dtype=np.int32).reshape(D, 4)


@pytest.mark.parametrize("n_bins,degrees", [(180, [61.0, -61.0, 179.0, -179.0, 1.0, -1.0, 119.0, -121.0, 91.0, -89.0]),
                                            (2, [60.0, -60.0, 179.0, -179.0, 1.0, -1.0]),
                                            (8, [60.0, -60.0, 100.0, -100.0, 170.0, -170.0, 20.0, -20.0])])
def test_the_construction_lands_in_the_bin_of_its_angle_and_pins_the_sign(n_bins, degrees):
    """Angles at least half a degree from a bin edge (float32 rounding of the fourth atom moves the angle by about
    1e-7 rad)."""
    degrees = np.array(degrees)
    width = 360.0 / n_bins
    assert np.all(np.abs((degrees + 180.0) / width - np.rint((degrees + 180.0) / width)) * width > 0.5)
    D = len(degrees)
    pos = _torsion_rows(np.deg2rad(degrees)[None, :], np.zeros((D, 3)))
    got = engine_run(pos, np.ones(D, dtype=int), _torsion_quads(D), [0], n_bins=n_bins, state_edges=(-180.0, 0.0))
    want = np.zeros((D, n_bins), dtype=np.int64)
    want[np.arange(D), np.floor((degrees + 180.0) / width).astype(int)] = 1
    np.testing.assert_array_equal(got["counts"], want)
    np.testing.assert_array_equal(got["state_counts"][0, :, 1], degrees > 0)       # state 1 is [0, 180): sin phi > 0


def test_a_rigid_torsion_gives_the_cosine_of_its_advance():
    """Every dihedral advances by delta = 0.1 rad per frame: cos(phi(f) - phi(f - k)) = cos(k delta)."""
    delta, F, D = 0.1, 37, 200
    lags = np.array([0, 1, 2, 5, 36])
    rng = np.random.default_rng(5)
    tails = rng.integers(-255, 256, (D, 3)) * 0.25                  # on a grid of 0.25, |x| < 64: exact in float32
    assert np.abs(tails).max() < 64
    phi = rng.uniform(-np.pi, np.pi, D)[None, :] + delta * np.arange(F)[:, None]
    pos = _torsion_rows(phi, tails)
    quads = _torsion_quads(D)
    fixed = pos.reshape(F, D, 4, 3)[:, :, :3].astype(np.float64)
    np.testing.assert_array_equal(fixed[:, :, 1], np.broadcast_to(tails, (F, D, 3)))       # a, b and c are exact
    np.testing.assert_array_equal(fixed[:, :, 0] - fixed[:, :, 1], np.broadcast_to((1.0, 0.0, 0.0), (F, D, 3)))
    np.testing.assert_array_equal(fixed[:, :, 2] - fixed[:, :, 1], np.broadcast_to((0.0, 0.0, 1.0), (F, D, 3)))
    got = engine_run(pos, [D], quads, lags)
    tacf = got["sums"][:, 0] / ((F - lags) * D)
    # The fourth atom d = t + (cos phi, sin phi, 1) has coordinates below 64 + 1 < 128, where float32 numbers are
    # 2^-17 apart: each moves by at most e = 2^-18.  With b2 = (0, 0, 1) exactly, n = b2 x b3 = (-b3y, b3x, 0) and
    # m = (0, 1, 0): the angle the engine sees is that of the in-plane vector (b3x, b3y), a unit vector moved by at
    # most sqrt(2) e, which turns it by at most asin(sqrt(2) e) <= (pi / 2) sqrt(2) e = a.  The difference of two
    # such angles is off by at most 2 a, and |cos x - cos y| <= |x - y|; the average obeys the same bound.  The
    # float64 rounding of the engine's own operations (a few 2^-53 per term) is the 1e-12.
    a = (np.pi / 2) * np.sqrt(2.0) * 2.0 ** -18
    assert np.abs(tacf - np.cos(lags * delta)).max() <= 2 * a + 1e-12
    assert np.abs(tacf[1:] - np.cos(lags[1:] * delta)).max() > 0        # the bound is not vacuous: float32 shows


def test_a_dihedral_that_switches_every_three_frames():
    """phi = +60 (gauche+, state 1) for three frames, 180 (trans, state 2) for three, and so on for 12 frames:
    states 1 1 1 2 2 2 1 1 1 2 2 2, runs 0 1 2 0 1 2 0 1 2 0 1 2.  The counts are written out by hand."""
    F, p = 12, 3
    degrees = np.where(np.arange(F) // p % 2 == 0, 60.0, 178.0)
    pos = _torsion_rows(np.deg2rad(degrees)[:, None], np.zeros((1, 3)))
    got = engine_run(pos, [1], _torsion_quads(1), [0, 1, 2, 3, 6, 7])
    np.testing.assert_array_equal(got["state_counts"][:, 0], [[0, 1, 0]] * 3 + [[0, 0, 1]] * 3 + [[0, 1, 0]] * 3 +
                                  [[0, 0, 1]] * 3)
    # f >= 1: 1->1 at f = 1, 2, 7, 8; 2->2 at f = 4, 5, 10, 11; 1->2 at f = 3, 9; 2->1 at f = 6
    np.testing.assert_array_equal(got["transitions"][0], [[0, 0, 0], [0, 4, 2], [0, 1, 4]])
    # same: lag 1 the eight diagonal cases; lag 2 only f = 2, 5, 8, 11; lag 3 never (always the other state); lag 6
    # the period, all of f = 6 ... 11; lag 7 = lag 1 pattern shifted: f = 7, 8, 10, 11 match f - 7 = 0, 1, 3, 4
    np.testing.assert_array_equal(got["same"][:, 0], [12, 8, 4, 0, 6, 4])
    # stay: run(f) >= lag; no run is longer than 2
    np.testing.assert_array_equal(got["stay"][:, 0], [12, 8, 4, 0, 0, 0])


# ---------------------------------------------------------------- the class

def test_class_groups_routes_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    F, sizes = 12, [T + 5, 40]
    rows, quads = dc.chains(20, F, sizes)
    n = rows.shape[1] + 9
    rng = np.random.default_rng(20)
    place = np.sort(rng.permutation(n)[:rows.shape[1]])             # the chains' atoms among others, in frame order
    pos = rng.uniform(0.0, 30.0, (F, n, 3)).astype(np.float32)
    pos[:, place] = rows
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    lags = np.array([0, 1, 3, 11, 15])
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    atoms = place[quads]                                            # [D, 4] atom numbers
    cut = sizes[0]

    def check(o, frames, step, dims=BOX):
        """o.results against the restatement on the selected frames."""
        want = dc.restate(rows[frames], sizes, quads, lags, dims=dims)
        res = o.results
        np.testing.assert_array_equal(res.times, lags * step * 0.5)
        np.testing.assert_array_equal(res.edges, np.linspace(-180.0, 180.0, 181))
        np.testing.assert_array_equal(res.angles, np.arange(-179.0, 180.0, 2.0))
        for key in ("counts", "state_counts", "transitions"):
            np.testing.assert_array_equal(res[key], want[key])
        terms = np.maximum(len(frames) - lags, 0).astype(float)[:, None] * np.array(sizes)[None, :]
        terms[terms == 0] = np.nan
        np.testing.assert_array_equal(res.tacf, want["sums"] / terms)
        np.testing.assert_array_equal(res.intermittent, want["same"] / terms)
        np.testing.assert_array_equal(res.continuous, want["stay"] / terms)
        live = lags < len(frames)
        assert np.isnan(res.tacf[~live]).all() and not np.isnan(res.tacf[live]).any()
        np.testing.assert_allclose(res.tacf[0], 1.0, rtol=1e-14)
        assert np.all(res.intermittent[0] == 1.0) and np.all(res.continuous[0] == 1.0)
        assert np.all(res.continuous[live] <= res.intermittent[live])
        # populations sum to 1, the distribution integrates to 1, and the transitions that leave or keep a state add
        # up to the dihedrals that were in it in the frames 0 ... F - 2
        np.testing.assert_allclose(res.populations.sum(axis=1), 1.0, rtol=1e-15)
        np.testing.assert_array_equal(res.populations, want["state_counts"].sum(axis=0) /
                                      (np.array(sizes)[:, None] * float(len(frames))))
        np.testing.assert_allclose((res.distribution * 2.0).sum(axis=1), 1.0, rtol=1e-14)
        np.testing.assert_array_equal(res.transitions.sum(axis=2), res.state_counts[:-1].sum(axis=0))

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            legs = [[u.select(atoms[:cut, i]), u.select(atoms[cut:, i])] for i in range(4)]
            new = lambda **kw: Dihedrals(*legs, lags=lags, verbose=False, **kw)      # noqa: E731
            full = new().run()
            check(full, np.arange(F), 1)
            check(new().run(start=1, stop=12, step=2), np.arange(1, 12, 2), 2)
            check(new().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]), 3)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in ("tacf", "intermittent", "continuous", "counts", "state_counts", "transitions"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        legs = [[u.select(atoms[:cut, i]), u.select(atoms[cut:, i])] for i in range(4)]
        # neither lags nor n_lags: every analysed frame is a lag
        every = Dihedrals(*legs, verbose=False).run()
        want = dc.restate(rows, sizes, quads, np.arange(F), dims=BOX)
        terms = (F - np.arange(F))[:, None] * np.array(sizes)[None, :]
        np.testing.assert_array_equal(every.results.tacf, want["sums"] / terms)
        np.testing.assert_array_equal(every.results.continuous, want["stay"] / terms)
        few = Dihedrals(*legs, n_lags=4, verbose=False).run()
        np.testing.assert_array_equal(few.results.tacf, every.results.tacf[:4])
        # the host helpers
        every.calculate_relaxation_times()
        times = [[calculate_residence_time(every.results.times, c[:, g]) for g in range(2)]
                 for c in (every.results.tacf, every.results.continuous)]
        np.testing.assert_array_equal(every.results.relaxation_times, times)
        every.calculate_transition_rates()
        spent = want["state_counts"][:-1].sum(axis=0) * 0.5
        rates = want["transitions"] / spent[:, :, None]
        rates[:, np.arange(3), np.arange(3)] = 0.0
        np.testing.assert_array_equal(every.results.transition_rates, rates)
        assert (rates > 0).any()
        every.calculate_pmf(300.0)
        p = every.results.distribution
        with np.errstate(divide="ignore"):
            np.testing.assert_array_equal(every.results.pmf,
                                          -8.31446261815324e-3 * 300.0 * np.log(p / p.max(axis=1, keepdims=True)))
        assert every.results.pmf.min() == 0.0
        with pytest.raises(ValueError, match="'temperature' must be positive"):
            every.calculate_pmf(0.0)
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(Dihedrals(*legs, lags=lags, verbose=False)).run()
        for key in ("tacf", "intermittent", "continuous", "counts", "state_counts", "transitions"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # without the box the bond vectors are the raw differences; other bins and states
        raw = Dihedrals(*legs, lags=lags, minimum_image=False, n_bins=36, state_edges=(-90.0, 90.0),
                        verbose=False).run()
        want = dc.restate(rows, sizes, quads, lags, n_bins=36, state_edges=(-90.0, 90.0))
        terms = np.maximum(F - lags, 0).astype(float)[:, None] * np.array(sizes)[None, :]
        terms[terms == 0] = np.nan
        np.testing.assert_array_equal(raw.results.tacf, want["sums"] / terms)
        np.testing.assert_array_equal(raw.results.counts, want["counts"])
        np.testing.assert_array_equal(raw.results.transitions, want["transitions"])
        assert raw.results.populations.shape == (2, 2) and raw.results.angles.shape == (36,)
        # no lag with an origin: the histogram and the states are still there
        late = Dihedrals(*legs, lags=[20, 30], verbose=False).run()
        assert np.isnan(late.results.tacf).all() and np.isnan(late.results.continuous).all()
        np.testing.assert_array_equal(late.results.counts, results["host"]["counts"])
        np.testing.assert_array_equal(late.results.transitions, results["host"]["transitions"])
    finally:
        d.free()


def test_class_from_chains_and_a_degenerate_frame():
    n_chains, n_monomers, F = 3, 7, 9
    rng = np.random.default_rng(21)
    torsions = rng.uniform(-180.0, 180.0, (1, n_chains, n_monomers - 3)) + \
        np.cumsum(rng.normal(0.0, 25.0, (F, n_chains, n_monomers - 3)), axis=0)
    true = np.concatenate([dc.place_chain(torsions[:, c]) + rng.uniform(0.0, 30.0, 3) for c in range(n_chains)], axis=1)
    n = n_chains * n_monomers
    pos = np.zeros((F, n + 4, 3), dtype=np.float32)
    pos[:, 2:2 + n] = dc.wrap(true)
    u = mdhelper_amd.ArrayUniverse(pos, [*BOX, 90.0, 90.0, 90.0], dt=2.0)
    ag = u.select(np.arange(2, 2 + n))
    o = Dihedrals.from_chains(ag, n_chains, n_monomers, n_lags=5, verbose=False).run()
    quads = np.concatenate([c * n_monomers + np.arange(n_monomers - 3)[:, None] + np.arange(4)[None, :]
                            for c in range(n_chains)])
    D = len(quads)
    want = dc.restate(pos[:, 2:2 + n], [D], quads, np.arange(5), dims=BOX)
    terms = (F - np.arange(5))[:, None] * D
    np.testing.assert_array_equal(o.results.tacf, want["sums"] / terms)
    np.testing.assert_array_equal(o.results.intermittent, want["same"] / terms)
    np.testing.assert_array_equal(o.results.counts, want["counts"])
    np.testing.assert_array_equal(o.results.times, np.arange(5) * 2.0)
    # the angles the chains were built with, recovered to what float32 leaves of them
    c, s, _, _ = dc.geometry(pos[:, 2:2 + n], quads, BOX)
    turned = np.degrees(np.arctan2(s, c)) - torsions.reshape(F, D)
    assert np.abs((turned + 180.0) % 360.0 - 180.0).max() < 1e-3
    # three atoms on a line in one frame: run() raises, nothing is averaged silently
    bad = pos.copy()
    bad[4, 2:5] = [(1.0, 1.0, 1.0), (1.5, 1.5, 1.5), (2.5, 2.5, 2.5)]
    ub = mdhelper_amd.ArrayUniverse(bad, [*BOX, 90.0, 90.0, 90.0], dt=2.0)
    with pytest.raises(ValueError, match="had no angle"):
        Dihedrals.from_chains(ub.select(np.arange(2, 2 + n)), n_chains, n_monomers, n_lags=5, verbose=False).run()
