"""
BondOrientationalOrder / BondOrderEngine on the GPU against the float64 NumPy restatement of the device contract
(``bond_order_cases.restate``; csrc/mdx_bond_order_device.hpp): the neighbour test of mdx_pairs_device.hpp, per bond
the recurrences for Y_lm one operation at a time with the host tables formed as the engine forms them, per centre the
sums over its neighbours in ascending j, and the frame sums through the two tile loops.

No tolerance between engine and restatement: both do one float64 operation at a time in one order (the unit is built
with contraction off; rint rounds ties to even, sqrt and / are correctly rounded on both sides), so every comparison
of values, sums, counts, outside, coordination and stats is ``assert_array_equal`` (which takes NaN for NaN: an
isolated centre).  The closed forms of the lattices hold within the tolerance measured on the CPU
(``bond_order_cases.TOL_CLOSED``).
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import BondOrientationalOrder

import bond_order_cases as cases

pytestmark = pytest.mark.gpu

T = _core.BondOrderEngine.TILE
JCHUNK = _core.BondOrderEngine.JCHUNK
EDGES = np.linspace(0.0, 1.0, 101)
CUTOFF = 3.0
ARRAYS = ("values", "sums", "counted", "counts", "outside", "coordination")
SCALARS = ("evaluations", "frames", "bonds", "degenerate", "max_row")


def box_for(n, neighbours=12.0, cutoff=CUTOFF):
    """The cubic box in which n uniform points have about `neighbours` others within the cutoff, at least 6.5 long
    (the cutoff may reach half of it)."""
    shell = 4.0 / 3.0 * np.pi * cutoff ** 3
    return np.full(3, max(6.5, float(np.ceil(4.0 * (n * shell / neighbours) ** (1.0 / 3.0)) / 4.0)))


def collect(eng):
    got = eng.result()
    got.update(eng.frames())
    got["values"] = eng.values()
    stats = eng.stats()
    got.update({key: stats[key] for key in SCALARS})
    return got


def engine_run(pos, n0, n1, cutoff, degrees, edges, dims, *, splits=None, setup=None, keep_values=True, **kwargs):
    """One pass over the frames, host route: what ``cases.restate`` returns."""
    eng = _core.BondOrderEngine(n0, n1, cutoff, degrees, edges, dims, keep_values=keep_values, **kwargs)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def assert_same(got, want, n0):
    for key in ARRAYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert got[key].dtype == want[key].dtype, key
    for key in SCALARS:
        assert got[key] == want[key], key
    # what follows from the definitions, whatever the input
    assert got["coordination"].sum() == got["frames"] * n0
    assert got["bonds"] == (got["coordination"] * np.arange(len(got["coordination"]))).sum()
    np.testing.assert_array_equal((~np.isnan(got["values"])).sum(axis=-1),
                                  np.broadcast_to(got["counted"][:, None, None], got["values"].shape[:3]))
    np.testing.assert_array_equal(got["counts"].sum(axis=-1) + got["outside"],
                                  np.full(got["outside"].shape, got["counted"].sum()))


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T, T + 1, 2 * T + 3])
def test_one_set_sizes(n, F):
    """The centres as their own neighbours, uniform points in a box sized for about 12 neighbours at cutoff 3.0.
    From 63 points on the restatement's mean row lies in 6 ... 20 and the rows differ in length; one point has no
    neighbour at all and two have one another or nobody (a row of 6 needs 7 points), which is asserted instead."""
    dims = box_for(n)
    pos = cases.cloud(700 + n, F, n, dims)
    want = cases.restate(pos, n, None, CUTOFF, [4, 6], EDGES, dims, same=True, averaged=True)
    rows = np.repeat(np.arange(len(want["coordination"])), want["coordination"])
    if n >= 63:
        assert 6 <= rows.mean() <= 20 and len(set(rows.tolist())) > 1 and want["max_row"] <= 32
    elif n == 2:
        assert want["max_row"] <= 1 and set(want["counted"].tolist()) <= {0, 2}     # the bonded pair: the next test
    else:
        assert want["max_row"] == 0 and not want["counted"].any() and np.isnan(want["values"]).all()
        assert not want["counts"].any() and not want["outside"].any() and not want["sums"].any()
    assert want["evaluations"] == F * n * (n - 1) and want["degenerate"] == 0
    got = engine_run(pos, n, None, CUTOFF, [4, 6], EDGES, dims, same=True, averaged=True)
    assert_same(got, want, n)


def test_two_points_that_see_each_other():
    """n0 = 2 with a bond: q_l = 1 for every l (one bond is perfectly ordered); the two ends see opposite directions,
    Y_lm(-u) = (-1)^l Y_lm(u), so qbar_l is 1 for an even l and 0 for an odd one."""
    dims = np.full(3, 6.5)
    pos = np.array([[[1.0, 1.0, 1.0], [2.5, 0.25, 6.0]]], dtype=np.float32)      # the bond crosses a face
    want = cases.restate(pos, 2, None, CUTOFF, [1, 2, 3, 12], EDGES, dims, same=True, averaged=True)
    assert want["counted"].tolist() == [2] and want["bonds"] == 2
    np.testing.assert_allclose(want["values"][0, :, 0], 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(want["values"][0, :, 1], np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.0], [1.0, 1.0]]),
                               rtol=0, atol=1e-14)
    assert_same(engine_run(pos, 2, None, CUTOFF, [1, 2, 3, 12], EDGES, dims, same=True, averaged=True), want, 2)


def test_more_candidates_than_one_chunk():
    """65 centres and JCHUNK + 1 candidates: two blocks append to one centre's row, and the last stage of the walk
    holds one candidate.  Centre 0 has neighbours on both sides of j = JCHUNK, so its row is filled by two blocks in
    whatever order their atomics arrive: an unsorted sum would differ from run to run and from the restatement."""
    n0, n1 = 65, JCHUNK + 1
    dims = box_for(n1)
    pos = cases.cloud(71, 3, n0 + n1, dims)
    pos[:, 0] = (10.0, 10.0, 10.0)
    pos[:, n0 + JCHUNK] = (11.0, 10.5, 10.25)
    want = cases.restate(pos, n0, n1, CUTOFF, [4, 6], EDGES, dims)
    near = cases.neighbours(pos[0].astype(np.float64), n0, False, CUTOFF, dims)[0]
    assert near[0, JCHUNK] and near[0, :JCHUNK].sum() >= 3
    assert 6 <= want["bonds"] / (3 * n0) <= 20 and want["max_row"] <= 32
    assert_same(engine_run(pos, n0, n1, CUTOFF, [4, 6], EDGES, dims), want, n0)


@pytest.fixture(scope="module")
def system():
    """Twelve frames of 130 points in a box for about 12 neighbours, shared and left unchanged."""
    n, F = 130, 12
    dims = box_for(n)
    pos = cases.cloud(11, F, n, dims)
    pos.setflags(write=False)
    want = cases.restate(pos, n, None, CUTOFF, [4, 6], EDGES, dims, same=True, averaged=True)
    assert 6 <= want["bonds"] / (F * n) <= 20 and want["max_row"] <= 32 and want["counted"].min() >= n - 2
    for key in ARRAYS:
        want[key].setflags(write=False)
    return {"pos": pos, "n": n, "dims": dims, "want": want}


@pytest.mark.parametrize("degrees", [(4, 6), (6,), (1, 2, 3, 12), (12, 5, 7, 9), (8, 10, 11)])
def test_degrees(system, degrees):
    """Every degree 1 ... 12 once across the cases, in orders that are not ascending."""
    pos, n, dims = system["pos"][:3], system["n"], system["dims"]
    want = cases.restate(pos, n, None, CUTOFF, degrees, EDGES, dims, same=True, averaged=True)
    got = engine_run(pos, n, None, CUTOFF, degrees, EDGES, dims, same=True, averaged=True)
    assert_same(got, want, n)
    assert got["values"].shape == (3, len(degrees), 2, n)
    if degrees == (4, 6):
        for key in ("values", "sums", "counts"):
            np.testing.assert_array_equal(got[key], system["want"][key][:3] if key != "counts" else want[key])


def test_averaged_on_and_off_give_the_same_q(system):
    pos, n, dims = system["pos"], system["n"], system["dims"]
    plain = engine_run(pos, n, None, CUTOFF, [4, 6], EDGES, dims, same=True, averaged=False)
    assert_same(plain, cases.restate(pos, n, None, CUTOFF, [4, 6], EDGES, dims, same=True), n)
    both = system["want"]
    assert plain["values"].shape == (12, 2, 1, n)
    np.testing.assert_array_equal(plain["values"][:, :, 0], both["values"][:, :, 0])
    np.testing.assert_array_equal(plain["sums"][:, :, 0], both["sums"][:, :, 0])
    np.testing.assert_array_equal(plain["counts"][:, 0], both["counts"][:, 0])
    assert (both["values"][:, :, 1] != both["values"][:, :, 0]).any()


@pytest.mark.parametrize("name", ["fcc", "bcc", "sc"])
def test_lattices(name):
    build, cutoff, shell, closed = cases.LATTICES[name]
    pos, dims = build()
    n = pos.shape[1]
    want = cases.restate(pos, n, None, cutoff, [4, 6], EDGES, dims, same=True, averaged=True)
    got = engine_run(pos, n, None, cutoff, [4, 6], EDGES, dims, same=True, averaged=True)
    assert_same(got, want, n)
    assert got["coordination"][shell] == n and got["max_row"] == shell and got["bonds"] == n * shell
    for d, l in enumerate((4, 6)):
        worst = float(np.abs(got["values"][0, d] - closed[l]).max())
        print(f"{name} q{l}: engine - closed form {worst:.3g}")
        assert worst <= cases.TOL_CLOSED
        assert np.abs(got["values"][0, d, 1] - got["values"][0, d, 0]).max() <= cases.TOL_AVERAGED


def test_one_set_of_bits_whatever_the_split_slab_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, n, dims, want = (system[k] for k in ("pos", "n", "dims", "want"))
    F = len(pos)
    args = (n, None, CUTOFF, [4, 6], EDGES, dims)
    kw = dict(same=True, averaged=True)

    def check(eng):
        assert_same(collect(eng), want, n)

    run = lambda **more: engine_run(pos, *args, **kw, **more)       # noqa: E731
    assert_same(run(), want, n)
    assert_same(run(splits=[0, 1, 5, 12]), want, n)
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want, n)
    assert_same(run(setup=lambda e: e.set_slab_frames(8)), want, n)
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(8)), want, n)
    wide = run(max_neighbors=64)                                    # another stride of the lists
    np.testing.assert_array_equal(wide["coordination"][:33], want["coordination"])
    assert not wide["coordination"][33:].any()
    for key in ("values", "sums", "counts"):
        np.testing.assert_array_equal(wide[key], want[key])

    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    rng = np.random.default_rng(13)
    n_total = 2 * n + 5
    index = np.sort(rng.permutation(n_total)[:n])[::-1].copy()
    assert np.all(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    big = (rng.uniform(0.0, 1.0, (F, n_total, 3)) * dims).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.tile(dims, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.BondOrderEngine(*args, keep_values=True, **kw)
    try:
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        stats = eng.stats()
        assert all(stats[key] == 0 for key in SCALARS)
        assert not any(v.any() for v in eng.result().values())
        assert eng.values().shape == (0, 2, 2, n) and eng.frames()["counted"].shape == (0,)
        eng.accumulate_traj(tf, np.arange(F))
        check(eng)                                                  # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        check(eng)                                                  # HBM through the descending index
        with pytest.raises(ValueError, match="out of range"):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        check(eng)                                                  # file through the index
        eng.reset()
        eng.set_slab_frames(8)
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


def _shell(count, far=0):
    """One frame: a centre and `count` candidates on a sphere of radius 2 around it (the last `far` of them 8 away
    instead), box 20."""
    rng = np.random.default_rng(64)
    v = rng.normal(size=(count, 3))
    v = 2.0 * v / np.linalg.norm(v, axis=1)[:, None]
    if far:
        v[-far:] *= 4.0
    origin = np.array([3.25, 9.5, 17.75])
    frame = np.concatenate(([origin], origin + v))
    return np.mod(frame, 20.0)[None].astype(np.float32)


def test_a_full_row_is_no_error_and_one_more_is_never_a_truncation():
    dims = np.full(3, 20.0)
    full, over, away = _shell(64), _shell(65), _shell(65, far=1)
    want = cases.restate(full, 1, 64, CUTOFF, [6], EDGES, dims, max_neighbors=64)
    assert (want["max_row"], want["bonds"]) == (64, 64)
    assert_same(engine_run(full, 1, 64, CUTOFF, [6], EDGES, dims, max_neighbors=64), want, 1)
    want_away = cases.restate(away, 1, 65, CUTOFF, [6], EDGES, dims, max_neighbors=64)
    assert (want_away["max_row"], want_away["bonds"]) == (64, 64)
    eng = _core.BondOrderEngine(1, 65, CUTOFF, [6], EDGES, dims, max_neighbors=64, keep_values=True)
    try:
        eng.accumulate(over)
        for call in (eng.result, eng.frames, eng.values, eng.synchronize, eng.result):      # ... and again
            with pytest.raises(ValueError, match="max_neighbors") as err:
                call()
            assert "65" in str(err.value) and "64" in str(err.value)
        assert eng.stats()["max_row"] == 65                         # the kernel kept counting
        eng.reset()
        eng.accumulate(away)
        assert_same(collect(eng), want_away, 1)                     # works again after reset
        eng.accumulate(over)                                        # an overflow in a later call of the pass
        with pytest.raises(ValueError, match="max_neighbors"):
            eng.result()
        assert eng.stats()["max_row"] == 65
    finally:
        eng.close()
    with pytest.raises(ValueError, match="max_neighbors"):
        engine_run(full, 1, 64, CUTOFF, [6], EDGES, dims, max_neighbors=63)


def test_a_neighbour_on_its_centre_refuses_the_results():
    n0, n1 = 40, 90
    dims = box_for(n1)
    pos = cases.cloud(5, 2, n0 + n1, dims)
    want = cases.restate(pos, n0, n1, CUTOFF, [4, 6], EDGES, dims)
    assert want["degenerate"] == 0 and want["bonds"] > 6 * 2 * n0
    bad = pos.copy()
    bad[1, n0 + 17] = bad[1, 3]                                     # candidate 17 sits on centre 3 in frame 1
    eng = _core.BondOrderEngine(n0, n1, CUTOFF, [4, 6], EDGES, dims, keep_values=True)
    try:
        eng.accumulate(bad)
        for call in (eng.result, eng.frames, eng.values, eng.synchronize):
            with pytest.raises(ValueError, match="1 bonds had no direction"):
                call()
        stats = eng.stats()
        assert stats["degenerate"] == 1 == cases.restate(bad, n0, n1, CUTOFF, [4, 6], EDGES, dims)["degenerate"]
        eng.reset()
        assert eng.stats()["degenerate"] == 0
        eng.accumulate(pos)
        assert_same(collect(eng), want, n0)                         # a clean pass after reset
    finally:
        eng.close()


def test_values_outside_the_range_and_on_the_edges(system):
    """Edges taken from the restatement's own values: a value on edges[0] or on edges[n_bins] is counted, one on an
    inner edge opens the bin above, and what lies beyond goes into `outside`."""
    pos, n, dims = system["pos"][:2], system["n"], system["dims"]
    base = system["want"]["values"][:2]
    v = np.unique(base[:, 0, 0][~np.isnan(base[:, 0, 0])])                  # q_4, ascending
    assert len(v) > 200
    edges = np.array([v[20], v[60], v[61], v[150], v[-30]])
    want = cases.restate(pos, n, None, CUTOFF, [4, 6], edges, dims, same=True, averaged=True)
    q4 = base[:, 0, 0][~np.isnan(base[:, 0, 0])]
    np.testing.assert_array_equal(want["counts"][0, 0], np.histogram(q4, bins=edges)[0])
    assert len(q4) == len(v)                                                # no value twice
    # [v20, v60): 40 values; [v60, v61): v60 alone; [v61, v150): 89; [v150, v[-30]], closed above: the rest
    assert want["counts"][0, 0].tolist() == [40, 1, 89, len(v) - 179]
    assert want["outside"][0, 0] == 20 + 29 and want["outside"].all()
    assert_same(engine_run(pos, n, None, CUTOFF, [4, 6], edges, dims, same=True, averaged=True), want, n)


@pytest.mark.parametrize("n_bins", [1, _core.BondOrderEngine.LDS_BINS, _core.BondOrderEngine.LDS_BINS + 1])
def test_histograms_in_lds_and_in_hbm(system, n_bins):
    """1024 bins still count in LDS, 1025 count in HBM directly; one bin has no inner edge at all."""
    pos, n, dims = system["pos"][:3], system["n"], system["dims"]
    edges = np.linspace(0.05, 0.7, n_bins + 1)
    want = cases.restate(pos, n, None, CUTOFF, [6, 4], edges, dims, same=True, averaged=True)
    assert (want["counts"].sum(axis=-1) > 100).all() and want["outside"].any()
    assert_same(engine_run(pos, n, None, CUTOFF, [6, 4], edges, dims, same=True, averaged=True), want, n)


# ---------------------------------------------------------------- the class

def test_class_routes_groups_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_a, extra, n_b, F = 140, 3, 200, 10
    n = n_a + extra + n_b
    dims = box_for(n)
    pos = cases.cloud(20, F, n, dims)
    boxes = np.tile(np.array([*dims, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    ia, ib = np.arange(n_a), np.arange(n_a + extra, n)
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    INTS = ("counts", "outside", "coordination_counts")

    def check(v, frames, *, idx, n0, n1=None, same=True, averaged=True, degrees=(4, 6), cutoff=3.5, box=dims):
        """v.results against the restatement and the formulas on the selected frames."""
        want = cases.restate(pos[frames][:, idx], n0, n1, cutoff, degrees, EDGES, box, same=same, averaged=averaged)
        res = v.results
        m_max = int(np.flatnonzero(want["coordination"])[-1])
        np.testing.assert_array_equal(res.counts, want["counts"])
        np.testing.assert_array_equal(res.outside, want["outside"])
        np.testing.assert_array_equal(res.coordination_counts, want["coordination"][:m_max + 1])
        np.testing.assert_array_equal(res["values"], want["values"])
        for key in INTS:
            assert res[key].dtype == np.int64, key
        np.testing.assert_array_equal(res.degrees, degrees)
        np.testing.assert_array_equal(res.edges, EDGES)
        np.testing.assert_array_equal(res.bins, (EDGES[:-1] + EDGES[1:]) / 2)
        width = np.diff(EDGES)
        assert (res.counts.sum(axis=-1) > 0).all()
        np.testing.assert_array_equal(res.distribution, res.counts / (res.counts.sum(axis=-1)[..., None] * width))
        np.testing.assert_allclose((res.distribution * width).sum(axis=-1), 1.0, rtol=0, atol=1e-12)
        assert want["counted"].all()
        np.testing.assert_array_equal(res.mean, want["sums"] / want["counted"][:, None, None])
        np.testing.assert_array_equal(res.mean_overall, want["sums"].sum(axis=0) / want["counted"].sum())
        np.testing.assert_allclose(res.mean, np.nanmean(want["values"], axis=-1), rtol=1e-13, atol=0)
        f = len(frames)
        np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (f * n0))
        np.testing.assert_allclose(res.coordination_number, want["bonds"] / (f * n0), rtol=1e-12, atol=0)
        return want

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            def make(u=u, **kw):
                return BondOrientationalOrder(u.select(ib), None, 3.5, keep_values=True, verbose=False, **kw)

            full = make().run()
            want = check(full, np.arange(F), idx=ib, n0=n_b)
            assert want["max_row"] <= 32 and 6 <= want["bonds"] / (F * n_b) <= 20
            check(make().run(start=1, stop=9, step=2), np.arange(1, 9, 2), idx=ib, n0=n_b)
            check(make().run(frames=[2, 5, 8, 9]), np.array([2, 5, 8, 9]), idx=ib, n0=n_b)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in INTS + ("values", "mean", "mean_overall"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(BondOrientationalOrder(u.select(ib), None, 3.5, keep_values=True, verbose=False)).run()
        for key in INTS + ("values", "mean"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # disjoint groups: the centres behind their candidates in the frame; K = 1
        apart = BondOrientationalOrder(u.select(ib), u.select(ia), 3.5, degrees=(6,), keep_values=True,
                                       verbose=False).run()
        check(apart, np.arange(F), idx=np.concatenate((ib, ia)), n0=n_b, n1=n_a, same=False, averaged=False,
              degrees=(6,))
        assert apart.results.counts.shape == (1, 1, 100)
        # every particle in order (no index), not averaged; dimensions given replace the universe's box
        wide = dims + 1.0
        whole = BondOrientationalOrder(u.atoms, cutoff=3.5, averaged=False, dimensions=wide, keep_values=True,
                                       verbose=False).run()
        check(whole, np.arange(F), idx=np.arange(n), n0=n, averaged=False, box=wide)
        # without keep_values nothing is kept
        assert "values" not in BondOrientationalOrder(u.select(ib), None, 3.5, verbose=False).run().results
        # too few slots: the error of the engine reaches the caller of run()
        with pytest.raises(ValueError, match="max_neighbors"):
            BondOrientationalOrder(u.select(ib), None, 3.5, max_neighbors=2, verbose=False).run()
    finally:
        d.free()
