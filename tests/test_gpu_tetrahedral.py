"""
TetrahedralOrder / TetrahedralEngine on the GPU against the float64 NumPy restatement of the device contract
(``tetrahedral_cases.restate``; csrc/mdx_tetrahedral_device.hpp): the range test of mdx_pairs_device.hpp, the
candidates of a centre ordered by ``lexsort((j, r2))``, q and S_k of the first four one operation at a time, the counts
by ``numpy.histogram`` (the distances as ``sqrt(r2)`` against distance edges) and the frame sums through the two tile
loops.

No tolerance between engine and restatement: both do one float64 operation at a time in one order (the unit is built
with contraction off; rint rounds ties to even, sqrt and / are correctly rounded on both sides), so every comparison,
``values`` and ``neighbors`` included, is ``assert_array_equal`` (which takes NaN for NaN: a short centre).  The known
answer of the diamond lattice holds within the 1e-12 of about 30 float64 operations on values of order 1.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import TetrahedralOrder
from mdhelper_amd.analysis.order import distance_table

import tetrahedral_cases as cases

pytestmark = pytest.mark.gpu

T = _core.TetrahedralEngine.TILE
STAGE = _core.TetrahedralEngine.STAGE
LDS_BINS = _core.TetrahedralEngine.LDS_BINS
CUTOFF = 3.0
Q_EDGES, S_EDGES, D_EDGES = np.linspace(-0.5, 1.0, 151), np.linspace(0.0, 1.0, 101), np.linspace(0.0, CUTOFF, 201)
ARRAYS = ("values", "neighbors", "sums", "counted", "q_counts", "s_counts", "outside", "distance_counts",
          "distance_outside", "found")
SCALARS = ("evaluations", "frames", "degenerate")


def collect(eng):
    got = eng.result()
    got.update(eng.frames())
    got.update(eng.values())
    stats = eng.stats()
    got.update({key: stats[key] for key in SCALARS})
    got["chunks"] = stats["chunks"]
    return got


def engine_run(pos, n0, n1, cutoff, k, dims, *, q_edges=Q_EDGES, s_edges=S_EDGES, d_edges=D_EDGES, same=False,
               splits=None, setup=None):
    """One pass over the frames, host route: what ``cases.restate`` returns."""
    eng = _core.TetrahedralEngine(n0, n1, cutoff, q_edges, s_edges, distance_table(d_edges), dims, n_nearest=k,
                                  same=same, keep_values=True)
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
    k = got["neighbors"].shape[1]
    assert got["found"].sum() == got["frames"] * n0
    np.testing.assert_array_equal((~np.isnan(got["values"])).sum(axis=-1),
                                  np.broadcast_to(got["counted"][:, None], got["values"].shape[:2]))
    np.testing.assert_array_equal(got["q_counts"].sum() + got["outside"][0], got["counted"].sum())
    np.testing.assert_array_equal(got["s_counts"].sum() + got["outside"][1], got["counted"].sum())
    np.testing.assert_array_equal(got["distance_counts"].sum(axis=1) + got["distance_outside"],
                                  [got["found"][a + 1:].sum() for a in range(k)])


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 6, 63, 64, 65, T, T + 1, 2 * T + 3])
def test_one_set_sizes(n, F):
    """The centres as their own candidates, uniform points in a box sized for about 8 within cutoff 3.0.  Up to four
    points every centre is short; five points in reach of one another give every centre exactly four candidates."""
    dims = cases.box_for(n, 8.0, CUTOFF)
    pos = cases.cloud(900 + n, F, n, dims)
    if n in (5, 6):
        pos = (pos * np.float32(0.2)).astype(np.float32)            # all within 0.2 * sqrt(3) * 6.5 < 3 of one another
    want = cases.restate(pos, n, None, CUTOFF, 4, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    if n <= 4:
        assert not want["counted"].any() and np.isnan(want["values"]).all() and want["found"][4] == 0
        assert not want["q_counts"].any() and not want["s_counts"].any() and not want["sums"].any()
    elif n in (5, 6):
        assert (want["in_range"] == n - 1).all() and want["found"].tolist() == [0, 0, 0, 0, F * n]
    else:
        assert 4 <= want["in_range"].mean() <= 14 and want["counted"].min() >= n // 2
        assert len(set(want["in_range"].ravel().tolist())) > 3
    assert want["evaluations"] == F * n * (n - 1) and want["degenerate"] == 0
    got = engine_run(pos, n, None, CUTOFF, 4, dims, same=True)
    assert_same(got, want, n)


def test_two_sets():
    n0, n1 = 300, 700
    dims = cases.box_for(n1, 8.0, CUTOFF)
    pos = cases.cloud(31, 2, n0 + n1, dims)
    want = cases.restate(pos, n0, n1, CUTOFF, 4, Q_EDGES, S_EDGES, D_EDGES, dims)
    assert 4 <= want["in_range"].mean() <= 14 and want["evaluations"] == 2 * n0 * n1
    assert_same(engine_run(pos, n0, n1, CUTOFF, 4, dims), want, n0)


@pytest.fixture(scope="module")
def system():
    """Six frames of 600 points (more than two stages of candidates) in a box for about 8 within the cutoff, shared
    and left unchanged; the restatement for n_nearest = 5."""
    n, F = 600, 6
    dims = cases.box_for(n, 8.0, CUTOFF)
    pos = cases.cloud(12, F, n, dims)
    pos.setflags(write=False)
    want = cases.restate(pos, n, None, CUTOFF, 5, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    assert 4 <= want["in_range"].mean() <= 14 and want["counted"].min() >= n // 2 and want["found"][:5].all()
    for key in ARRAYS:
        want[key].setflags(write=False)
    return {"pos": pos, "n": n, "dims": dims, "want": want}


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_every_n_nearest(system, k):
    """Each K instantiation; the first four, and with them q and S_k, do not depend on k."""
    pos, n, dims = system["pos"][:2], system["n"], system["dims"]
    want = cases.restate(pos, n, None, CUTOFF, k, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    got = engine_run(pos, n, None, CUTOFF, k, dims, same=True)
    assert_same(got, want, n)
    assert got["neighbors"].shape == (2, k, n) and got["found"].shape == (k + 1,) and want["found"][k] > 0
    np.testing.assert_array_equal(got["values"], system["want"]["values"][:2])
    np.testing.assert_array_equal(got["neighbors"][:, :4], system["want"]["neighbors"][:2, :4])


def test_candidate_chunks():
    """n1 = 3 * 256 + 1 with a chunk of 256: four chunks, the last holding one candidate, which is made the nearest
    of centre 0; against the plan's own choice and against the restatement."""
    n0, n1 = 65, 3 * STAGE + 1
    dims = cases.box_for(n1, 8.0, CUTOFF)
    pos = cases.cloud(77, 2, n0 + n1, dims)
    pos[:, 0] = (10.0, 10.0, 10.0)
    pos[:, n0 + 3 * STAGE] = (10.25, 10.0, 10.5)
    want = cases.restate(pos, n0, n1, CUTOFF, 6, Q_EDGES, S_EDGES, D_EDGES, dims)
    assert (want["neighbors"][:, 0, 0] == 3 * STAGE).all()
    spread = want["neighbors"][:, :, :] // STAGE                    # the chunk every neighbour comes from
    chunks_of = [set(spread[0, :, i][want["neighbors"][0, :, i] >= 0].tolist()) for i in range(n0)]
    assert max(len(c) for c in chunks_of) > 1
    pinned = engine_run(pos, n0, n1, CUTOFF, 6, dims, setup=lambda e: e.set_chunk(STAGE))
    planned = engine_run(pos, n0, n1, CUTOFF, 6, dims)
    assert pinned["chunks"] == 4 and planned["chunks"] >= 1
    assert_same(pinned, want, n0)
    assert_same(planned, want, n0)


@pytest.mark.parametrize("chunk", [STAGE, 0], ids=["chunk_256", "plan"])
def test_ties_go_to_the_lowest_candidates(chunk):
    """A simple-cubic lattice of 11^3 sites on integer coordinates in a box of 11: six neighbours with bit-equal r2,
    of which the four of lowest j are kept, across chunks and across the periodic seam.  An insert or a merge that is
    not stable keeps another four."""
    pos, dims = cases.sc(11)
    n = pos.shape[1]
    assert n == 1331
    d_edges = np.array([0.0, 0.5, 1.0, 1.25])
    want = cases.restate(pos, n, None, 1.25, 4, Q_EDGES, S_EDGES, d_edges, dims, same=True)
    x = np.arange(n)
    six = np.stack([((x // 121 + dx) % 11) * 121 + ((x // 11 % 11 + dy) % 11) * 11 + (x % 11 + dz) % 11
                    for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))])
    lowest = np.sort(six, axis=0)[:4]
    np.testing.assert_array_equal(want["neighbors"][0], lowest)
    assert (want["in_range"] == 6).all()
    assert ((lowest // STAGE).max(axis=0) > (lowest // STAGE).min(axis=0)).any()        # ties that span chunks
    got = engine_run(pos, n, None, 1.25, 4, dims, d_edges=d_edges, same=True, setup=lambda e: e.set_chunk(chunk))
    np.testing.assert_array_equal(got["neighbors"][0], lowest)
    assert_same(got, want, n)
    assert got["chunks"] == (6 if chunk else got["chunks"]) and got["distance_counts"][:, 2].tolist() == [n] * 4


def test_diamond_has_a_known_answer():
    pos, dims = cases.diamond(3)
    pos = np.repeat(pos, 2, axis=0)
    n = pos.shape[1]
    assert n == 216
    want = cases.restate(pos, n, None, 2.0, 4, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    got = engine_run(pos, n, None, 2.0, 4, dims, same=True)
    assert_same(got, want, n)
    worst = float(np.abs(got["values"][:, 0] - 1.0).max())
    print(f"diamond: |q - 1| at most {worst:.3g}")
    assert worst <= 1e-12 and (got["values"][:, 1] == 1.0).all()
    assert got["found"][4] == 2 * n and got["counted"].tolist() == [n, n]
    wide = engine_run(pos, n, None, 3.0, 8, dims, same=True)        # the second shell fills the other slots
    np.testing.assert_array_equal(wide["values"], got["values"])
    assert wide["found"][8] == 2 * n


def test_short_centres():
    """A sparse system in which centres have 0, 1, 2, 3 and at least 4 candidates in range."""
    n, F, k = 200, 2, 5
    dims = cases.box_for(n, 2.5, CUTOFF)
    pos = cases.cloud(44, F, n, dims)
    want = cases.restate(pos, n, None, CUTOFF, k, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    m = want["in_range"]
    for count in (0, 1, 2, 3):
        assert (m == count).any()
    assert (m == 4).any() and (m >= k).any()
    np.testing.assert_array_equal(want["found"], np.bincount(np.minimum(m, k).ravel(), minlength=k + 1))
    assert want["found"].all()
    got = engine_run(pos, n, None, CUTOFF, k, dims, same=True)
    assert_same(got, want, n)
    short = m < 4
    assert np.isnan(got["values"][:, 0][short]).all() and np.isnan(got["values"][:, 1][short]).all()
    assert not np.isnan(got["values"][:, 0][~short]).any()
    np.testing.assert_array_equal((got["neighbors"] >= 0).sum(axis=1), np.minimum(m, k))
    np.testing.assert_array_equal(got["counted"], (~short).sum(axis=1))
    assert got["q_counts"].sum() + got["outside"][0] == (~short).sum()
    # ... but present in the distance histograms of the ranks they have
    np.testing.assert_array_equal(got["distance_counts"].sum(axis=1) + got["distance_outside"],
                                  [(m > a).sum() for a in range(k)])
    assert got["distance_counts"][0].sum() > (~short).sum()


def test_a_neighbour_on_its_centre_refuses_the_results(system):
    pos, n, dims, want = (system[key] for key in ("pos", "n", "dims", "want"))
    pos = pos[:2]
    clean = cases.restate(pos, n, None, CUTOFF, 5, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    bad = pos.copy()
    centre = int(np.flatnonzero(want["in_range"][1] >= 4)[0])
    other = centre + 17
    bad[1, other] = bad[1, centre]                                  # they sit on each other in frame 1
    assert cases.restate(bad, n, None, CUTOFF, 5, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)["degenerate"] == 2
    eng = _core.TetrahedralEngine(n, None, CUTOFF, Q_EDGES, S_EDGES, distance_table(D_EDGES), dims, n_nearest=5,
                                  same=True, keep_values=True)
    try:
        eng.accumulate(bad)
        for call in (eng.synchronize, eng.result, eng.frames, eng.values, eng.result):
            with pytest.raises(ValueError, match="2 of the four nearest neighbors had no direction"):
                call()
        assert eng.stats()["degenerate"] == 2
        eng.reset()
        assert eng.stats()["degenerate"] == 0 and eng.stats()["frames"] == 0
        eng.accumulate(pos)
        assert_same(collect(eng), clean, n)                         # a clean pass after reset
    finally:
        eng.close()


def test_a_candidate_on_a_short_centre_is_no_error():
    """Three points, two of them on one another: every centre is short and has no q, so the pair at r2 == 0 is counted
    in `found` and in the first distance bin and refuses nothing (include/mdx.h)."""
    dims = np.full(3, 20.0)
    pos = np.array([[[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [2.0, 2.0, 3.0]]], dtype=np.float32)
    got = engine_run(pos, 3, None, CUTOFF, 4, dims, same=True)
    assert got["degenerate"] == 0 and got["found"].tolist() == [0, 0, 3, 0, 0] and np.isnan(got["values"]).all()
    assert got["neighbors"][0, :2].tolist() == [[1, 0, 0], [2, 2, 1]]
    assert got["distance_counts"][0, 0] == 2 and got["distance_counts"].sum(axis=1).tolist() == [3, 3, 0, 0]
    assert_same(got, cases.restate(pos, 3, None, CUTOFF, 4, Q_EDGES, S_EDGES, D_EDGES, dims, same=True), 3)


def test_values_on_the_edges_and_outside_the_range(system):
    """Edges taken from the restatement's own values: a value on the first or the last edge is counted, one on an
    inner edge opens the bin above, and what lies beyond goes into `outside`; for q, S_k and the distances."""
    pos, n, dims = system["pos"][:2], system["n"], system["dims"]
    base = system["want"]
    tables = []
    for v in (base["values"][:2, 0], base["values"][:2, 1]):
        v = np.unique(v[~np.isnan(v)])
        assert len(v) > 400
        tables.append(np.array([v[20], v[60], v[61], v[150], v[-30]]))
    near, _, r2 = cases.pairs(pos[0].astype(np.float64), n, True, CUTOFF, dims)
    r = np.unique(np.sqrt(r2[near]))
    tables.append(np.array([r[40], r[300], r[301], r[-500]]))
    want = cases.restate(pos, n, None, CUTOFF, 5, *tables, dims, same=True)
    q = base["values"][:2, 0]
    q = q[~np.isnan(q)]
    np.testing.assert_array_equal(want["q_counts"], np.histogram(q, bins=tables[0])[0])
    assert want["q_counts"][1] >= 1 and want["outside"].all() and want["distance_outside"].all()
    assert want["q_counts"].sum() + want["outside"][0] == len(q)
    got = engine_run(pos, n, None, CUTOFF, 5, dims, q_edges=tables[0], s_edges=tables[1], d_edges=tables[2], same=True)
    assert_same(got, want, n)


@pytest.mark.parametrize("n_bins", [1, LDS_BINS, LDS_BINS + 1])
def test_histograms_in_lds_and_in_hbm(system, n_bins):
    """1024 bins still count in LDS, 1025 count in HBM directly; one bin has no inner edge at all.  The same switch
    for the value histograms and for the distance histograms."""
    pos, n, dims = system["pos"][:3], system["n"], system["dims"]
    tables = (np.linspace(-0.2, 0.8, n_bins + 1), np.linspace(0.7, 0.999, n_bins + 1),
              np.linspace(1.0, 2.9, n_bins + 1))
    want = cases.restate(pos, n, None, CUTOFF, 5, *tables, dims, same=True)
    assert want["q_counts"].sum() > 100 and want["s_counts"].sum() > 100 and want["outside"].all()
    assert (want["distance_counts"].sum(axis=1) > 100).all() and want["distance_outside"].all()
    got = engine_run(pos, n, None, CUTOFF, 5, dims, q_edges=tables[0], s_edges=tables[1], d_edges=tables[2], same=True)
    assert_same(got, want, n)


def test_one_set_of_bits_whatever_the_split_slab_chunk_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, n, dims, want = (system[k] for k in ("pos", "n", "dims", "want"))
    F = len(pos)

    def run(**more):
        return engine_run(pos, n, None, CUTOFF, 5, dims, same=True, **more)

    def both(*setters):
        return lambda e: [setter(e) for setter in setters]

    assert_same(run(), want, n)
    assert_same(run(splits=[0, 1, 4, 6]), want, n)
    for slab in (1, 2):
        assert_same(run(setup=lambda e: e.set_slab_frames(slab)), want, n)
    for chunk, chunks in ((256, 3), (512, 2)):
        got = run(setup=lambda e: e.set_chunk(chunk))
        assert got["chunks"] == chunks
        assert_same(got, want, n)
    assert_same(run(splits=[0, 1, 4, 6], setup=both(lambda e: e.set_slab_frames(2), lambda e: e.set_chunk(256))),
                want, n)

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
    eng = _core.TetrahedralEngine(n, None, CUTOFF, Q_EDGES, S_EDGES, distance_table(D_EDGES), dims, n_nearest=5,
                                  same=True, keep_values=True)

    def check():
        assert_same(collect(eng), want, n)

    try:
        plan = eng.plan()
        assert plan["ring_frames"] == 0 and plan["slab_frames"] >= F and plan["chunk"] % STAGE == 0
        eng.accumulate_device(d.ptr, n, F)
        check()                                                     # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_chunk(256)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        stats = eng.stats()
        assert all(stats[key] == 0 for key in SCALARS)
        assert not any(v.any() for v in eng.result().values())
        assert eng.values()["neighbors"].shape == (0, 5, n) and eng.frames()["counted"].shape == (0,)
        eng.accumulate_traj(tf, np.arange(F))
        check()                                                     # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        check()                                                     # HBM through the descending index
        with pytest.raises(ValueError, match="out of range"):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))
        eng.reset()
        eng.set_chunk(512)
        eng.accumulate_traj(tf_big, np.arange(F), index)
        check()                                                     # file through the index, two chunks
        eng.reset()
        eng.set_chunk(0)
        eng.set_slab_frames(2)
        eng.accumulate_device(d.rows(0, 2).ptr, n, 2)               # routes mixed within one pass
        eng.accumulate(pos[2:5])
        eng.accumulate_traj(tf, np.arange(5, F))
        check()
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


# ---------------------------------------------------------------- the class

def test_class_routes_groups_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_mol, n_b, F = 150, 260, 8
    n = 3 * n_mol + n_b
    cutoff = 3.5
    dims = cases.box_for(n_mol, 8.0, cutoff)
    pos = cases.cloud(21, F, n, dims)
    boxes = np.tile(np.array([*dims, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    oxygens, ib = np.arange(0, 3 * n_mol, 3), np.arange(3 * n_mol, n)
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    d_edges = np.linspace(0.0, cutoff, 201)
    INTS = ("q_counts", "q_outside", "sk_counts", "sk_outside", "distance_counts", "distance_outside", "found_counts")

    def check(v, frames, *, idx, n0, n1=None, same=True, k=4, box=dims):
        """v.results against the restatement and the formulas on the selected frames."""
        want = cases.restate(pos[frames][:, idx], n0, n1, cutoff, k, Q_EDGES, S_EDGES, d_edges, box, same=same)
        res = v.results
        for key, ref in (("q_counts", want["q_counts"]), ("q_outside", want["outside"][0]),
                         ("sk_counts", want["s_counts"]), ("sk_outside", want["outside"][1]),
                         ("distance_counts", want["distance_counts"]), ("distance_outside", want["distance_outside"]),
                         ("found_counts", want["found"]), ("values", want["values"]), ("neighbors", want["neighbors"])):
            np.testing.assert_array_equal(res[key], ref, err_msg=key)
            assert np.asarray(res[key]).dtype == np.asarray(ref).dtype, key
        for name, edges in (("q", Q_EDGES), ("sk", S_EDGES), ("distance", d_edges)):
            np.testing.assert_array_equal(res[f"{name}_edges"], edges)
            np.testing.assert_array_equal(res[f"{name}_bins"], (edges[:-1] + edges[1:]) / 2)
            counts, width = res[f"{name}_counts"], np.diff(edges)
            assert (counts.sum(axis=-1) > 0).all()
            np.testing.assert_array_equal(res[f"{name}_distribution"],
                                          counts / (counts.sum(axis=-1, keepdims=True) * width))
            np.testing.assert_allclose((res[f"{name}_distribution"] * width).sum(axis=-1), 1.0, rtol=0, atol=1e-12)
        assert want["counted"].all() and res.distance_counts.shape == (k, 200)
        np.testing.assert_array_equal(res.mean, want["sums"] / want["counted"][:, None])
        np.testing.assert_array_equal(res.mean_overall, want["sums"].sum(axis=0) / want["counted"].sum())
        # the means against the kept values: 150 additions of values of order 1 in another order
        np.testing.assert_allclose(res.mean, np.nanmean(res["values"], axis=-1), rtol=0, atol=1e-13)
        assert res.units["results.distance_edges"] == "angstrom"
        return want

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            def make(u=u, **kw):
                return TetrahedralOrder(u.select(oxygens), cutoff=cutoff, keep_values=True, verbose=False, **kw)

            full = make().run()
            want = check(full, np.arange(F), idx=oxygens, n0=n_mol)
            assert 4 <= want["in_range"].mean() <= 14
            check(make().run(start=1, stop=8, step=2), np.arange(1, 8, 2), idx=oxygens, n0=n_mol)
            check(make().run(frames=[2, 5, 7]), np.array([2, 5, 7]), idx=oxygens, n0=n_mol)
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for key in INTS + ("values", "neighbors", "mean", "mean_overall"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(TetrahedralOrder(u.select(oxygens), cutoff=cutoff, keep_values=True, verbose=False)).run()
        for key in INTS + ("values", "neighbors", "mean"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # "O H H" molecules laid end to end: the oxygens are the centres and their own candidates
        water = TetrahedralOrder.from_molecules(u.select(np.arange(3 * n_mol)), n_mol, cutoff=cutoff,
                                                keep_values=True, verbose=False).run()
        for key in INTS + ("values", "neighbors", "mean"):
            np.testing.assert_array_equal(water.results[key], results["host"][key])
        # disjoint groups: the centres behind their candidates in the frame, six nearest
        apart = TetrahedralOrder(u.select(ib), u.select(oxygens), cutoff=cutoff, n_nearest=6, keep_values=True,
                                 verbose=False).run()
        check(apart, np.arange(F), idx=np.concatenate((ib, oxygens)), n0=n_b, n1=n_mol, same=False, k=6)
        # without keep_values nothing is kept
        bare = TetrahedralOrder(u.select(oxygens), cutoff=cutoff, verbose=False).run().results
        assert "values" not in bare and "neighbors" not in bare
        np.testing.assert_array_equal(bare.mean, results["host"].mean)
        # the default cutoff is half the shortest box length
        half = TetrahedralOrder(u.select(oxygens), dimensions=[dims[0], dims[1] + 1.0, dims[2] + 2.0],
                                verbose=False).run().results
        assert half.distance_edges[-1] == dims[0] / 2
    finally:
        d.free()
