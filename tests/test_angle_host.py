"""
Host-side checks of the angular distribution that need no GPU: the argument handling of
``analysis.angle.AngularDistribution``, the argument errors of the engine, which are raised before any device is
touched (a handle touches its device with the first frame), the numbering of the species pairs, and the arithmetic of
``AngularDistribution._conclude`` on the integers of a stub engine.

Not reachable without a device, and therefore checked in ``test_gpu_angle.py``: ``set_slab_frames`` after the first
frame and a row beyond ``max_neighbors`` (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import AngularDistribution, angle


def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


# ---------------------------------------------------------------- the class

def test_constructor_errors():
    u = _universe()
    assert mdhelper_amd.analysis.AngularDistribution is angle.AngularDistribution
    c, a, b = u.select(np.arange(4)), u.select(np.arange(4, 9)), u.select(np.arange(9, 12))
    # the groups
    with pytest.raises(ValueError, match="share some atoms"):
        AngularDistribution(c, u.select(np.arange(3, 9)), 5.0)                  # centre and ligands overlap
    with pytest.raises(ValueError, match="share some atoms"):
        AngularDistribution(c, [a, u.select(np.arange(8, 12))], 5.0)            # two ligand groups overlap
    with pytest.raises(ValueError, match="share some atoms"):
        AngularDistribution(c, u.select([3, 2, 1, 0]), 5.0)                     # the same atoms in another order
    with pytest.raises(ValueError, match="share some atoms"):
        AngularDistribution(c, [c, a], 5.0)                                     # the centres beside another group
    with pytest.raises(ValueError, match="at least one atom"):
        AngularDistribution(c, [a, u.select(np.arange(0))], 5.0)
    with pytest.raises(ValueError, match="at least one atom"):
        AngularDistribution(u.select(np.arange(0)), a, 5.0)
    with pytest.raises(ValueError, match="between 1 and 4 groups"):
        AngularDistribution(c, [u.select([i]) for i in range(4, 9)], 5.0)
    with pytest.raises(ValueError, match="between 1 and 4 groups"):
        AngularDistribution(c, [], 5.0)
    AngularDistribution(c, [u.select([i]) for i in range(4, 8)], 5.0)
    # the cutoffs
    for wrong in ([5.0], [5.0, 5.0, 5.0], [[5.0, 5.0]]):
        with pytest.raises(ValueError, match="a number or 2 values, one per ligand group"):
            AngularDistribution(c, [a, b], wrong)
    with pytest.raises(ValueError, match="a number or 1 values"):
        AngularDistribution(c, a, [5.0, 5.0])
    for wrong in (0.0, -1.0, np.nan, np.inf, [5.0, 0.0], [np.nan, 5.0], [5.0, -np.inf]):
        with pytest.raises(ValueError, match="'cutoff' must be positive and finite"):
            AngularDistribution(c, [a, b], wrong)
    # the box: too small for the largest cutoff, none at all, not orthorhombic
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        AngularDistribution(c, a, 20.5)                                          # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        AngularDistribution(c, [a, b], [2.0, 20.5])                              # the largest value counts
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        AngularDistribution(c, a, 15.0, dimensions=[29.0, 60.0, 60.0])
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        AngularDistribution(c, a, 21.5, drop_axis="z")                           # x is still 40
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        v = _universe(dims=None)
        AngularDistribution(v.select(np.arange(4)), v.select(np.arange(4, 9)), 5.0)
    with pytest.raises(ValueError, match="orthorhombic"):
        v = _universe(angles=(90.0, 90.0, 60.0))
        AngularDistribution(v.select(np.arange(4)), v.select(np.arange(4, 9)), 5.0)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        AngularDistribution(c, a, 5.0, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        AngularDistribution(c, a, 5.0, drop_axis=3)
    # bins and slots
    for n_bins in (0, -4):
        with pytest.raises(ValueError, match="'n_bins' must be at least 1"):
            AngularDistribution(c, a, 5.0, n_bins=n_bins)
    for bins in ("degrees", "cos", None):
        with pytest.raises(ValueError, match="'bins'"):
            AngularDistribution(c, a, 5.0, bins=bins)
    for slots in (0, 65, -3):
        with pytest.raises(ValueError, match="'max_neighbors' must lie in \\[1, 64\\]"):
            AngularDistribution(c, a, 5.0, max_neighbors=slots)
    AngularDistribution(c, a, 20.0)                                              # exactly half is allowed
    AngularDistribution(c, a, 21.0, drop_axis="x")                               # x dropped: 42 / 2 = 21
    AngularDistribution(c, a, 5.0, n_bins=1, max_neighbors=1)
    AngularDistribution(c, a, 5.0, max_neighbors=64)
    # what the arguments become: the centres, then the ligand groups as given, whatever their order in the frame
    two = AngularDistribution(b, [a, c], [3.0, 4.0], n_bins=4, bins="cosine", drop_axis="z", max_neighbors=8)
    np.testing.assert_array_equal(two._index, [9, 10, 11, 4, 5, 6, 7, 8, 0, 1, 2, 3])
    np.testing.assert_array_equal(two._ligand_sizes, [5, 4])
    assert two._ligand_sizes.dtype == np.int64
    np.testing.assert_array_equal(two._cutoff, [3.0, 4.0])
    np.testing.assert_array_equal(two._thresholds, [1.0, 0.5, 0.0, -0.5, -1.0])
    np.testing.assert_array_equal(two._edges, [1.0, 0.5, 0.0, -0.5, -1.0])
    assert (two._same, two._n_centers, two._drop_axis, two._max_neighbors) == (False, 3, 2, 8)
    one = AngularDistribution(c, u.select(np.arange(4)), 5.0)                    # the very atoms of the centres
    np.testing.assert_array_equal(one._index, [0, 1, 2, 3])
    np.testing.assert_array_equal(one._ligand_sizes, [4])
    np.testing.assert_array_equal(one._dimensions, [40.0, 42.0, 44.0])
    assert (one._same, one._n_centers, one._drop_axis, one._max_neighbors, one._n_bins) == (True, 4, None, 32, 180)
    np.testing.assert_array_equal(one._edges, np.linspace(0.0, 180.0, 181))
    np.testing.assert_array_equal(one._thresholds, np.cos(np.deg2rad(np.linspace(0.0, 180.0, 181))))
    assert np.all(np.diff(one._thresholds) < 0)
    np.testing.assert_array_equal(AngularDistribution(c, [a, b], 5.0)._cutoff, [5.0, 5.0])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            AngularDistribution(u.select(np.arange(4)), u.select(np.arange(4, 12)), 5.0, verbose=False).run()
        eng = _core.AngleEngine(4, [8], 2.0, [1.0, 0.0, -1.0], [10.0, 10.0, 10.0])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- the pair numbering

def test_pair_numbering():
    """p = a*G - a*(a-1)/2 + (b-a) numbers the pairs a <= b row by row of the upper triangle, either order given."""
    pair = _core.AngleEngine.pair_index
    for G in (1, 2, 3, 4):
        want = [(a, b) for a in range(G) for b in range(a, G)]
        assert len(want) == G * (G + 1) // 2
        for p, (a, b) in enumerate(want):
            assert pair(a, b, G) == p and pair(b, a, G) == p
    assert [pair(a, b, 4) for a, b in ((0, 0), (0, 3), (1, 1), (1, 3), (2, 2), (2, 3), (3, 3))] == [0, 3, 4, 6, 7, 8, 9]
    assert [pair(a, b, 2) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))] == [0, 1, 1, 2]


# ---------------------------------------------------------------- _conclude on a stub engine

class Stub:
    """Stands in for ``_core.AngleEngine``: records what it is fed and hands out hand-made integers, one frame like
    the next: 3 centres, two ligand species, 4 cosine bins; per frame the pair (0, 0) has 1 + 3 + 0 + 4 triplets and
    one degenerate one, the pair (0, 1) has none at all, the pair (1, 1) has 2 in its last bin; two centres have 3
    neighbours of species 0 and one has 5, all three have 2 neighbours of species 1."""
    MAX_SPECIES, MAX_NEIGHBORS = 4, 64
    made = []

    def __init__(self, n_centers, ligand_sizes, cutoff, thresholds, dims, *, same=False, zero_dims=0,
                 max_neighbors=32, dev=0, timing=False):
        self.n_centers, self.ligand_sizes, self.cutoff = n_centers, np.array(ligand_sizes), np.array(cutoff)
        self.thresholds, self.dims = np.array(thresholds), np.array(dims)
        self.args = dict(same=same, zero_dims=zero_dims, max_neighbors=max_neighbors)
        self.max_neighbors, self.n_frames, self.calls, self.closed = max_neighbors, 0, [], False
        Stub.made.append(self)

    def accumulate(self, pos):
        self.calls.append(np.array(pos))
        self.n_frames += len(pos)

    def result(self):
        counts = np.array([[1, 3, 0, 4], [0, 0, 0, 0], [0, 0, 0, 2]], dtype=np.int64) * self.n_frames
        degenerate = np.array([1, 0, 0], dtype=np.int64) * self.n_frames
        coordination = np.zeros((2, self.max_neighbors + 1), dtype=np.int64)
        coordination[0, [3, 5]] = np.array([2, 1]) * self.n_frames
        coordination[1, 2] = 3 * self.n_frames
        return {"counts": counts, "degenerate": degenerate, "coordination": coordination}

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    Stub.made = []
    monkeypatch.setattr(_core, "AngleEngine", Stub)
    monkeypatch.setattr(_lib, "require_device", lambda dev=0: None)
    return Stub


def test_conclude_normalises_trims_and_marks_empty_pairs(stub):
    u = _universe(n_frames=5)
    c, a, b = u.select(np.arange(9, 12)), u.select(np.arange(4, 9)), u.select(np.arange(4))
    v = AngularDistribution(c, [a, b], [3.5, 2.0], n_bins=4, bins="cosine", drop_axis="y", max_neighbors=16,
                            verbose=False).run(step=2)
    eng = stub.made[0]
    assert eng.closed and eng.n_frames == 3
    assert eng.args == dict(same=False, zero_dims=2, max_neighbors=16)
    assert eng.n_centers == 3
    np.testing.assert_array_equal(eng.ligand_sizes, [5, 4])
    np.testing.assert_array_equal(eng.cutoff, [3.5, 2.0])
    np.testing.assert_array_equal(eng.thresholds, [1.0, 0.5, 0.0, -0.5, -1.0])
    np.testing.assert_array_equal(eng.dims, [40.0, 42.0, 44.0])
    index = np.r_[9:12, 4:9, 0:4]
    np.testing.assert_array_equal(np.concatenate(eng.calls), u.trajectory.frame_block([0, 2, 4])[:, index])
    res = v.results
    F, n0 = 3, 3
    np.testing.assert_array_equal(res.edges, [1.0, 0.5, 0.0, -0.5, -1.0])
    np.testing.assert_array_equal(res.bins, [0.75, 0.25, -0.25, -0.75])
    assert res.pairs == [(0, 0), (0, 1), (1, 1)]
    np.testing.assert_array_equal(res.counts, [[3, 9, 0, 12], [0, 0, 0, 0], [0, 0, 0, 6]])
    np.testing.assert_array_equal(res.degenerate, [3, 0, 0])
    np.testing.assert_array_equal(res.coordination_counts, [[0, 0, 0, 6, 0, 3], [0, 0, 9, 0, 0, 0]])   # trimmed to 5
    for key in ("counts", "degenerate", "coordination_counts"):
        assert res[key].dtype == np.int64, key
    # counts / (counts.sum(-1) * bin width): the width of a cosine bin is 0.5; a pair without a triplet is NaN
    np.testing.assert_array_equal(res.distribution[0], np.array([3, 9, 0, 12]) / (24 * 0.5))
    assert np.isnan(res.distribution[1]).all()
    np.testing.assert_array_equal(res.distribution[2], [0.0, 0.0, 0.0, 2.0])
    np.testing.assert_allclose((res.distribution[[0, 2]] * 0.5).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (F * n0))
    np.testing.assert_array_equal(res.coordination_distribution.sum(axis=1), [1.0, 1.0])
    np.testing.assert_allclose(res.coordination_number, [(2 * 3 + 5) / 3, 2.0], rtol=0, atol=1e-12)
    assert res.units["results.bins"] == "dimensionless"
    # bins in degrees: edges and centres in degrees, the thresholds their cosines, the width 45
    w = AngularDistribution(c, [a, b], 3.5, n_bins=4, verbose=False).run()
    eng = stub.made[1]
    assert eng.n_frames == 5 and eng.args == dict(same=False, zero_dims=0, max_neighbors=32)
    np.testing.assert_array_equal(eng.thresholds, np.cos(np.deg2rad([0.0, 45.0, 90.0, 135.0, 180.0])))
    np.testing.assert_array_equal(eng.cutoff, [3.5, 3.5])
    np.testing.assert_array_equal(w.results.edges, [0.0, 45.0, 90.0, 135.0, 180.0])
    np.testing.assert_array_equal(w.results.bins, [22.5, 67.5, 112.5, 157.5])
    np.testing.assert_array_equal(w.results.distribution[0], np.array([5, 15, 0, 20]) / (40 * 45.0))
    assert w.results.units["results.bins"] == "degree"
    # the centres as their own ligands: one group, the rows once
    s = AngularDistribution(c, u.select(np.arange(9, 12)), 3.5, n_bins=4, verbose=False)
    assert s._same and len(s._index) == 3


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank, self.reduced = rank, []

    def allreduce(self, arr, op="sum"):
        arr = np.asarray(arr)
        assert arr.dtype == np.int64 and op == "sum"
        self.reduced.append(arr.copy())
        return arr * 2                      # "the other rank" held the same numbers


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_shard_frames_and_allreduce(stub, rank):
    u = _universe(n_frames=7)
    c, a, b = u.select(np.arange(3)), u.select(np.arange(3, 8)), u.select(np.arange(8, 12))
    comm = TwoRanks(rank)
    v = AngularDistribution(c, [a, b], 3.5, n_bins=4, bins="cosine", verbose=False, comm=comm).run()
    eng = stub.made[0]
    lo, hi = ((0, 4), (4, 7))[rank]
    assert eng.n_frames == hi - lo
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(lo, hi)))
    # the integers travel at their full shapes, this rank's frames only
    sent = comm.reduced
    assert [s.shape for s in sent] == [(3, 4), (3,), (2, 33)]
    np.testing.assert_array_equal(sent[0][0], np.array([1, 3, 0, 4]) * (hi - lo))
    res = v.results
    np.testing.assert_array_equal(res.counts, 2 * sent[0])
    np.testing.assert_array_equal(res.degenerate, 2 * sent[1])
    np.testing.assert_array_equal(res.coordination_counts, 2 * sent[2][:, :6])
    # the distributions are formed after the sum, over all 7 frames
    np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (7 * 3))
    np.testing.assert_array_equal(res.distribution[0], res.counts[0] / (res.counts[0].sum() * 0.5))


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]
COS4 = [1.0, 0.5, 0.0, -0.5, -1.0]


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(thresholds=[1.0, 0.5, 0.5, -1.0]), "strictly decreasing: \\[1\\] = 0.5, \\[2\\] = 0.5"),
                         (dict(thresholds=[-1.0, 0.0, 1.0]), "strictly decreasing"),
                         (dict(thresholds=[1.0, np.nan, -1.0]), "strictly decreasing"),
                         (dict(thresholds=[1.0, 0.0, -0.5, -0.25]), "strictly decreasing: \\[2\\] = -0.5"),
                         (dict(thresholds=[1.0]), "at least two"),
                         (dict(thresholds=[[1.0, 0.0], [0.0, -1.0]]), "at least two"),
                         (dict(cutoff=[2.0, 0.0]), "cutoff\\[1\\] must be positive and finite"),
                         (dict(cutoff=[-2.0, 2.0]), "cutoff\\[0\\] must be positive and finite"),
                         (dict(cutoff=[2.0, np.nan]), "cutoff\\[1\\] must be positive and finite"),
                         (dict(cutoff=[np.inf, 2.0]), "cutoff\\[0\\] must be positive and finite"),
                         (dict(cutoff=[2.0, 2.0, 2.0]), "a number or 2 values"),
                         (dict(cutoff=[[2.0, 2.0]]), "a number or 2 values"),
                         (dict(ligand_sizes=[3, 0]), "ligand group 1 must hold at least one point"),
                         (dict(ligand_sizes=[]), "between 1 and 4 sizes"),
                         (dict(ligand_sizes=[1, 1, 1, 1, 1], cutoff=2.0), "between 1 and 4 sizes"),
                         (dict(n_centers=0), "at least one point"),
                         (dict(same=True), "with same there is one ligand group"),
                         (dict(same=True, ligand_sizes=[4], cutoff=2.0), "with same there is one ligand group"),
                         (dict(cutoff=5.5), "beyond half the shortest box length"),
                         (dict(cutoff=[1.0, 5.5]), "beyond half the shortest box length"),
                         (dict(dims=[3.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 11.0, 3.9], zero_dims=3), "beyond half the shortest box length"),
                         (dict(cutoff=5.5, zero_dims=2), "beyond half the shortest box length"),
                         (dict(max_neighbors=0), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(max_neighbors=65), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(zero_dims=7), "at least one component"),
                         (dict(zero_dims=-1), "at least one component"),
                         (dict(dims=[10.0, 0.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, np.nan, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0]), "three box lengths")):
        args = dict(n_centers=3, ligand_sizes=[3, 2], cutoff=[2.0, 1.5], thresholds=COS4, dims=DIMS, same=False,
                    zero_dims=0, max_neighbors=32)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.AngleEngine(args["n_centers"], args["ligand_sizes"], args["cutoff"], args["thresholds"],
                              args["dims"], same=args["same"], zero_dims=args["zero_dims"],
                              max_neighbors=args["max_neighbors"])
    # half the shortest kept length itself is allowed, and a dropped component does not count
    _core.AngleEngine(3, [3, 2], [2.0, 1.5], COS4, [4.0, 11.0, 12.0]).close()
    _core.AngleEngine(3, [3, 2], [2.0, 1.5], COS4, [1.0, 11.0, 12.0], zero_dims=1).close()
    _core.AngleEngine(3, [3, 2], 5.5, COS4, DIMS, zero_dims=1).close()
    _core.AngleEngine(3, 5, 2.0, COS4, DIMS, max_neighbors=1).close()
    _core.AngleEngine(3, [3], 2.0, [1.0, -1.0], DIMS, same=True, max_neighbors=64).close()
    _core.AngleEngine(1, [1, 1, 1, 1], 2.0, np.linspace(1.0, -1.0, 2001), DIMS).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    sizes, cut, thr, dims = np.array([3, 2], dtype=np.int64), np.array([2.0, 1.5]), np.array(COS4), np.array(DIMS)
    create = lambda *a: lib.mdx_ang_create(ctypes.byref(h), 0, *a)      # noqa: E731
    assert create(3, 2, p(sizes), 0, p(cut), 4, p(thr), p(dims), 0, 32) == 0
    assert lib.mdx_ang_destroy(h) == 0
    assert create(3, 5, p(sizes), 0, p(cut), 4, p(thr), p(dims), 0, 32) == -1
    assert b"n_species must lie in [1, 4]" in lib.mdx_last_error()
    assert create(3, 2, p(sizes), 0, p(cut), 0, p(thr), p(dims), 0, 32) == -1
    assert b"n_bins" in lib.mdx_last_error()
    assert create(3, 2, p(sizes), 0, p(np.array([2.0, 5.25])), 4, p(thr), p(dims), 0, 32) == -1
    assert b"cutoff 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(2 ** 31 // 3, 2, p(sizes), 0, p(cut), 4, p(thr), p(dims), 0, 32) == -1
    assert b"2^31 / 3" in lib.mdx_last_error()
    for args in ((3, 2, None, 0, p(cut), 4, p(thr), p(dims), 0, 32), (3, 2, p(sizes), 0, None, 4, p(thr), p(dims), 0, 32),
                 (3, 2, p(sizes), 0, p(cut), 4, None, p(dims), 0, 32), (3, 2, p(sizes), 0, p(cut), 4, p(thr), None, 0, 32)):
        assert create(*args) == -1
        assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_ang_create(None, 0, 3, 2, p(sizes), 0, p(cut), 4, p(thr), p(dims), 0, 32) == -1
    assert lib.mdx_ang_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_ang_result(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    eng = _core.AngleEngine
    assert (eng.TILE, eng.STAGE, eng.JCHUNK, eng.MAX_NEIGHBORS, eng.MAX_SPECIES) == (256, 256, 1024, 64, 4)


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _core.AngleEngine(2, [2, 1], [2.0, 1.5], COS4, DIMS, zero_dims=2)
    one = _core.AngleEngine(5, [5], 2.0, COS4, DIMS, same=True, max_neighbors=4)
    try:
        assert (two.n_rows, two.n_species, two.n_pairs, two.n_bins, two.max_neighbors) == (5, 2, 3, 4, 32)
        assert (one.n_rows, one.n_species, one.n_pairs, one.n_bins, one.max_neighbors) == (5, 1, 1, 4, 4)
        for eng in (two, one):
            with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
                eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="7 rows given, the groups hold 5"):
                eng.accumulate_device(rows, 7, 2)
            with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
            with pytest.raises(ValueError, match="index 7 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 7])
            with pytest.raises(ValueError, match="index -1 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, -1, 3, 4])
            for frames in (-1, 32769):
                with pytest.raises(ValueError, match="frames must lie in"):
                    eng.set_slab_frames(frames)
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            eng.set_slab_frames(0)
            eng.reset()
            eng.synchronize()
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "triplets": 0,
                                   "max_row": 0}
    finally:
        two.close()
        one.close()
