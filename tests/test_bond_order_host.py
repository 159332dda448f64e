"""
Host-side checks of the bond-orientational order analysis that need no GPU: the argument handling of
``analysis.order.BondOrientationalOrder``, the argument errors of the engine, which are raised before any device is
touched (a handle touches its device with the first frame), the arithmetic of ``BondOrientationalOrder._conclude`` on
the numbers of a stub engine, and the float64 restatement of the device contract (``bond_order_cases.restate``, which
``test_gpu_bond_order.py`` holds the engine to bit for bit) against the definition with ``scipy.special.sph_harm_y``
and against the closed forms of the perfect lattices.

Not reachable without a device, and therefore checked in ``test_gpu_bond_order.py``: ``set_slab_frames`` after the
first frame, a row beyond ``max_neighbors`` and a neighbour on its centre (there is no first frame without a device).
"""
import ctypes
import math

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import BondOrientationalOrder, order

import bond_order_cases as cases


def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


# ---------------------------------------------------------------- the class

def test_constructor_errors():
    u = _universe()
    assert mdhelper_amd.analysis.BondOrientationalOrder is order.BondOrientationalOrder
    c, a = u.select(np.arange(4)), u.select(np.arange(4, 12))
    # the groups
    with pytest.raises(ValueError, match="share some atoms"):
        BondOrientationalOrder(c, u.select(np.arange(3, 9)), 5.0)               # the groups overlap
    with pytest.raises(ValueError, match="share some atoms"):
        BondOrientationalOrder(c, u.select([3, 2, 1, 0]), 5.0)                  # the same atoms in another order
    with pytest.raises(ValueError, match="at least one atom"):
        BondOrientationalOrder(c, u.select(np.arange(0)), 5.0)
    with pytest.raises(ValueError, match="at least one atom"):
        BondOrientationalOrder(u.select(np.arange(0)), a, 5.0)
    with pytest.raises(TypeError, match="cutoff"):
        BondOrientationalOrder(c)
    # averaged needs same; it defaults to what the groups allow
    with pytest.raises(ValueError, match="'averaged' needs"):
        BondOrientationalOrder(c, a, 5.0, averaged=True)
    assert BondOrientationalOrder(c, a, 5.0)._averaged is False
    assert BondOrientationalOrder(c, a, 5.0, averaged=False)._averaged is False
    assert BondOrientationalOrder(c, cutoff=5.0)._averaged is True
    assert BondOrientationalOrder(c, u.select(np.arange(4)), 5.0)._averaged is True
    assert BondOrientationalOrder(c, None, 5.0, averaged=False)._averaged is False
    # the degrees
    for wrong, word in (([0, 4], "lie in \\[1, 12\\]"), ([13], "lie in \\[1, 12\\]"), ([-2], "lie in \\[1, 12\\]"),
                        ([4, 6, 4], "twice"), ([1, 2, 3, 4, 5], "between 1 and 4"), ([], "between 1 and 4"),
                        ([4.0, 6.0], "between 1 and 4 integers"), ([[4, 6]], "between 1 and 4")):
        with pytest.raises(ValueError, match=word):
            BondOrientationalOrder(c, None, 5.0, degrees=wrong)
    # the cutoff
    for wrong in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="'cutoff' must be positive and finite"):
            BondOrientationalOrder(c, None, wrong)
    # the box: too small for the cutoff, none at all, not orthorhombic
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        BondOrientationalOrder(c, None, 20.5)                                   # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        BondOrientationalOrder(c, a, 15.0, dimensions=[60.0, 60.0, 29.0])
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        v = _universe(dims=None)
        BondOrientationalOrder(v.select(np.arange(4)), None, 5.0)
    with pytest.raises(ValueError, match="orthorhombic"):
        v = _universe(angles=(90.0, 90.0, 60.0))
        BondOrientationalOrder(v.select(np.arange(4)), None, 5.0)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        BondOrientationalOrder(c, None, 5.0, dimensions=[10.0, 10.0])
    with pytest.raises(TypeError):
        BondOrientationalOrder(c, None, 5.0, drop_axis="z")                     # q_l is a 3-D quantity
    # bins, range and slots
    for n_bins in (0, -4):
        with pytest.raises(ValueError, match="'n_bins' must be at least 1"):
            BondOrientationalOrder(c, None, 5.0, n_bins=n_bins)
    for wrong in ((0.0, 0.0), (1.0, 0.0), (0.0, np.inf), (np.nan, 1.0), (0.0, 0.5, 1.0)):
        with pytest.raises(ValueError, match="'range'"):
            BondOrientationalOrder(c, None, 5.0, range=wrong)
    for slots in (0, 65, -3):
        with pytest.raises(ValueError, match="'max_neighbors' must lie in \\[1, 64\\]"):
            BondOrientationalOrder(c, None, 5.0, max_neighbors=slots)
    BondOrientationalOrder(c, None, 20.0)                                       # exactly half is allowed
    BondOrientationalOrder(c, None, 5.0, n_bins=1, max_neighbors=1, degrees=12)
    BondOrientationalOrder(c, None, 5.0, max_neighbors=64, degrees=(1, 2, 3, 12))
    # what the arguments become
    two = BondOrientationalOrder(a, c, 3.0, degrees=(6,), n_bins=4, range=(0.0, 0.8), max_neighbors=8,
                                 keep_values=True)
    np.testing.assert_array_equal(two._index, [4, 5, 6, 7, 8, 9, 10, 11, 0, 1, 2, 3])
    assert (two._same, two._n_centers, two._n_neighbors, two._max_neighbors, two._keep_values) == (False, 8, 4, 8, True)
    np.testing.assert_array_equal(two._edges, np.linspace(0.0, 0.8, 5))
    np.testing.assert_array_equal(two._degrees, [6])
    one = BondOrientationalOrder(c, None, 5.0)
    np.testing.assert_array_equal(one._index, [0, 1, 2, 3])
    np.testing.assert_array_equal(one._dimensions, [40.0, 42.0, 44.0])
    np.testing.assert_array_equal(one._degrees, [4, 6])
    assert one._degrees.dtype == np.int32
    assert (one._same, one._n_centers, one._n_neighbors, one._max_neighbors, one._n_bins, one._keep_values) == \
        (True, 4, 4, 32, 100, False)
    np.testing.assert_array_equal(one._edges, np.linspace(0.0, 1.0, 101))


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            BondOrientationalOrder(u.atoms, None, 5.0, verbose=False).run()
        eng = _core.BondOrderEngine(12, None, 2.0, [4, 6], [0.0, 0.5, 1.0], [10.0, 10.0, 10.0], same=True)
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- _conclude on a stub engine

class Stub:
    """Stands in for ``_core.BondOrderEngine``: records what it is fed and hands out hand-made numbers, one frame like
    the next: 5 centres, of which one is isolated, two have 3 neighbours and two have 6; 4 bins.  Degree d, kind k:
    the four centres with a neighbour have the values (0.1, 0.3, 0.3, 0.9) + d / 8 - k / 16, the last of which falls
    outside a range that ends at 0.8."""
    MAX_NEIGHBORS, MAX_DEGREE, MAX_DEGREES = 64, 12, 4
    made = []

    def __init__(self, n_centers, n_neighbors, cutoff, degrees, edges, dims, *, same=False, averaged=False,
                 max_neighbors=32, keep_values=False, dev=0, timing=False):
        self.n_centers, self.n_neighbors, self.cutoff = n_centers, n_neighbors, cutoff
        self.degrees, self.edges, self.dims = np.array(degrees), np.array(edges), np.array(dims)
        self.args = dict(same=same, averaged=averaged, max_neighbors=max_neighbors, keep_values=keep_values)
        self.max_neighbors, self.n_frames, self.calls, self.closed = max_neighbors, 0, [], False
        self.D, self.K = len(self.degrees), 2 if averaged else 1
        Stub.made.append(self)

    def accumulate(self, pos):
        self.calls.append(np.array(pos))
        self.n_frames += len(pos)

    def _values(self):
        base = np.array([0.1, 0.3, np.nan, 0.3, 0.9])
        shift = np.arange(self.D)[:, None, None] / 8 - np.arange(self.K)[None, :, None] / 16
        return np.tile((base + shift)[None], (self.n_frames, 1, 1, 1))

    def result(self):
        v = self._values()
        counts = np.zeros((self.D, self.K, len(self.edges) - 1), dtype=np.int64)
        outside = np.zeros((self.D, self.K), dtype=np.int64)
        for d in range(self.D):
            for k in range(self.K):
                x = v[:, d, k][~np.isnan(v[:, d, k])]
                counts[d, k] = np.histogram(x, bins=self.edges)[0]
                outside[d, k] = len(x) - counts[d, k].sum()
        coordination = np.zeros(self.max_neighbors + 1, dtype=np.int64)
        coordination[[0, 3, 6]] = np.array([1, 2, 2]) * self.n_frames
        return {"counts": counts, "outside": outside, "coordination": coordination}

    def frames(self):
        return {"sums": np.nansum(self._values(), axis=-1), "counted": np.full(self.n_frames, 4, dtype=np.int64)}

    def values(self):
        assert self.args["keep_values"]
        return self._values()

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    Stub.made = []
    monkeypatch.setattr(_core, "BondOrderEngine", Stub)
    monkeypatch.setattr(_lib, "require_device", lambda dev=0: None)
    return Stub


def test_conclude_normalises_trims_and_averages(stub):
    u = _universe(n_frames=5)
    c = u.select(np.arange(3, 8))
    v = BondOrientationalOrder(c, None, 3.5, n_bins=4, range=(0.0, 0.8), max_neighbors=16, keep_values=True,
                               verbose=False).run(step=2)
    eng = stub.made[0]
    assert eng.closed and eng.n_frames == 3
    assert eng.args == dict(same=True, averaged=True, max_neighbors=16, keep_values=True)
    assert (eng.n_centers, eng.n_neighbors, eng.cutoff) == (5, 5, 3.5)
    np.testing.assert_array_equal(eng.degrees, [4, 6])
    np.testing.assert_array_equal(eng.edges, [0.0, 0.2, 0.4, 0.6000000000000001, 0.8])
    np.testing.assert_array_equal(eng.dims, [40.0, 42.0, 44.0])
    np.testing.assert_array_equal(np.concatenate(eng.calls), u.trajectory.frame_block([0, 2, 4])[:, 3:8])
    res = v.results
    F, n0 = 3, 5
    np.testing.assert_array_equal(res.degrees, [4, 6])
    np.testing.assert_array_equal(res.edges, np.linspace(0.0, 0.8, 5))
    np.testing.assert_array_equal(res.bins, (res.edges[:-1] + res.edges[1:]) / 2)
    assert res.counts.shape == (2, 2, 4) and res.outside.shape == (2, 2)
    np.testing.assert_array_equal(res.counts[0, 0], [3, 6, 0, 0])          # 0.1 | 0.3, 0.3 | - | - and 0.9 outside
    np.testing.assert_array_equal(res.outside, [[3, 3], [3, 3]])
    for key in ("counts", "outside", "coordination_counts", "degrees"):
        assert res[key].dtype == np.int64, key
    width = np.diff(res.edges)
    np.testing.assert_array_equal(res.distribution, res.counts / (res.counts.sum(axis=-1)[..., None] * width))
    np.testing.assert_allclose((res.distribution * width).sum(axis=-1), 1.0, rtol=0, atol=1e-12)
    # the means: sums / counted per frame, and over all frames
    per_frame = np.nansum(eng._values(), axis=-1) / 4
    np.testing.assert_array_equal(res.mean, per_frame)
    assert res.mean.shape == (F, 2, 2)
    np.testing.assert_allclose(res.mean[0, 0, 0], (0.1 + 0.3 + 0.3 + 0.9) / 4, rtol=1e-15)
    np.testing.assert_array_equal(res.mean_overall, np.nansum(eng._values(), axis=-1).sum(axis=0) / 12)
    np.testing.assert_array_equal(res.coordination_counts, [3, 0, 0, 6, 0, 0, 6])      # trimmed to 6
    np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (F * n0))
    np.testing.assert_allclose(res.coordination_number, (2 * 3 + 2 * 6) / 5, rtol=1e-15)
    np.testing.assert_array_equal(res["values"], eng._values())
    assert res["values"].shape == (F, 2, 2, n0)
    assert res.units["results.bins"] == "dimensionless"
    # disjoint groups, not averaged: K = 1, no values kept; nothing counted in a histogram: a row of NaN
    w = BondOrientationalOrder(c, u.select(np.arange(8, 12)), 3.5, degrees=(6,), n_bins=2, range=(2.0, 3.0),
                               verbose=False).run()
    eng = stub.made[1]
    assert eng.n_frames == 5 and eng.args == dict(same=False, averaged=False, max_neighbors=32, keep_values=False)
    assert (eng.n_centers, eng.n_neighbors) == (5, 4)
    np.testing.assert_array_equal(np.concatenate(eng.calls), u.trajectory.frame_block(np.arange(5))[:, 3:12])
    assert w.results.counts.shape == (1, 1, 2) and not w.results.counts.any()
    np.testing.assert_array_equal(w.results.outside, [[20]])
    assert np.isnan(w.results.distribution).all()
    assert w.results.mean.shape == (5, 1, 1) and "values" not in w.results


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank, self.reduced = rank, []

    def allreduce(self, arr, op="sum"):
        arr = np.asarray(arr)
        assert op == "sum"
        self.reduced.append(arr.copy())
        return arr * 2                      # "the other rank" held the same numbers


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_shard_frames_allreduce_and_gather(stub, rank):
    u = _universe(n_frames=7)
    comm = TwoRanks(rank)
    v = BondOrientationalOrder(u.select(np.arange(5)), None, 3.5, n_bins=4, range=(0.0, 0.8), keep_values=True,
                               verbose=False, comm=comm).run()
    eng = stub.made[0]
    lo, hi = ((0, 4), (4, 7))[rank]
    assert eng.n_frames == hi - lo
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(lo, hi))[:, :5])
    # the integers travel at their full shapes, this rank's frames only; the per-frame rows inside all 7 frames
    sent = comm.reduced
    assert [s.shape for s in sent] == [(2, 2, 4), (2, 2), (33,), (7, 2, 2), (7,), (7, 2, 2, 5)]
    assert [s.dtype for s in sent[:3]] == [np.int64] * 3 and sent[4].dtype == np.int64
    np.testing.assert_array_equal(sent[0][0, 0], np.array([1, 2, 0, 0]) * (hi - lo))
    mine = np.zeros(7, dtype=bool)
    mine[lo:hi] = True
    np.testing.assert_array_equal(sent[4], 4 * mine)
    assert not sent[3][~mine].any() and sent[3][mine].all()
    np.testing.assert_array_equal(sent[5][~mine], 0.0)
    np.testing.assert_array_equal(sent[5][mine], eng._values())
    res = v.results
    np.testing.assert_array_equal(res.counts, 2 * sent[0])
    np.testing.assert_array_equal(res.outside, 2 * sent[1])
    np.testing.assert_array_equal(res.coordination_counts, 2 * sent[2][:7])
    # the quotients are formed after the sums, over all 7 frames
    np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (7 * 5))
    np.testing.assert_array_equal(res.mean[mine], (2 * sent[3][mine]) / (2 * 4))
    assert np.isnan(res.mean[~mine]).all()                  # "the other rank" of this stand-in counted nothing there
    np.testing.assert_array_equal(res.mean_overall, (2 * sent[3]).sum(axis=0) / (2 * sent[4]).sum())


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]
EDGES = [0.0, 0.25, 0.5, 0.75, 1.0]


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(degrees=[0]), "degrees\\[0\\] = 0 must lie in \\[1, 12\\]"),
                         (dict(degrees=[4, 13]), "degrees\\[1\\] = 13 must lie in \\[1, 12\\]"),
                         (dict(degrees=[4, 6, 4]), "degrees holds 4 twice"),
                         (dict(degrees=[1, 2, 3, 4, 5]), "between 1 and 4 degrees"),
                         (dict(degrees=[]), "between 1 and 4 degrees"),
                         (dict(averaged=True), "averaged needs same"),
                         (dict(same=True, n_neighbors=4), "with same the neighbors are the 3 centers"),
                         (dict(cutoff=0.0), "cutoff must be positive and finite"),
                         (dict(cutoff=-2.0), "cutoff must be positive and finite"),
                         (dict(cutoff=np.nan), "cutoff must be positive and finite"),
                         (dict(cutoff=np.inf), "cutoff must be positive and finite"),
                         (dict(cutoff=5.5), "beyond half the shortest box length"),
                         (dict(dims=[3.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 0.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, np.nan, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0]), "three box lengths"),
                         (dict(n_centers=0), "centers must hold at least one point"),
                         (dict(n_neighbors=0), "neighbors must hold at least one point"),
                         (dict(n_centers=2 ** 31 // 3), "2\\^31 / 3"),
                         (dict(edges=[0.0, 0.5, 0.5, 1.0]), "strictly increasing: \\[1\\] = 0.5, \\[2\\] = 0.5"),
                         (dict(edges=[1.0, 0.5, 0.0]), "strictly increasing"),
                         (dict(edges=[0.0, np.nan, 1.0]), "strictly increasing"),
                         (dict(edges=[0.0, np.inf]), "edges must be finite"),
                         (dict(edges=[0.0]), "at least two"),
                         (dict(edges=[[0.0, 0.5], [0.5, 1.0]]), "at least two"),
                         (dict(max_neighbors=0), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(max_neighbors=65), "max_neighbors must lie in \\[1, 64\\]")):
        args = dict(n_centers=3, n_neighbors=5, cutoff=2.0, degrees=[4, 6], edges=EDGES, dims=DIMS, same=False,
                    averaged=False, max_neighbors=32)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.BondOrderEngine(args["n_centers"], args["n_neighbors"], args["cutoff"], args["degrees"],
                                  args["edges"], args["dims"], same=args["same"], averaged=args["averaged"],
                                  max_neighbors=args["max_neighbors"])
    # what is allowed: half the shortest length itself, every degree, one bin, many bins, both caps
    _core.BondOrderEngine(3, 5, 5.0, [4, 6], EDGES, DIMS).close()
    _core.BondOrderEngine(3, None, 2.0, [1, 2, 3, 12], EDGES, DIMS, same=True, averaged=True, max_neighbors=64).close()
    _core.BondOrderEngine(3, 3, 2.0, 6, [0.0, 1.0], DIMS, same=True, max_neighbors=1, keep_values=True).close()
    _core.BondOrderEngine(1, 1, 2.0, [12], np.linspace(0.0, 1.0, 2 ** 20 + 1), DIMS).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    deg, edges, dims = np.array([4, 6], dtype=np.int32), np.array(EDGES), np.array(DIMS)
    create = lambda *a: lib.mdx_boo_create(ctypes.byref(h), 0, *a)      # noqa: E731
    assert create(3, 5, 0, 2.0, 2, p(deg), 0, 4, p(edges), p(dims), 32, 0) == 0
    assert lib.mdx_boo_destroy(h) == 0
    assert create(3, 5, 0, 2.0, 5, p(deg), 0, 4, p(edges), p(dims), 32, 0) == -1
    assert b"between 1 and 4 degrees" in lib.mdx_last_error()
    assert create(3, 5, 0, 2.0, 2, p(deg), 0, 0, p(edges), p(dims), 32, 0) == -1
    assert b"n_bins" in lib.mdx_last_error()
    assert create(3, 5, 0, 2.0, 2, p(deg), 0, 2 ** 20 + 1, p(edges), p(dims), 32, 0) == -1
    assert b"n_bins" in lib.mdx_last_error()
    assert create(3, 5, 0, 5.25, 2, p(deg), 0, 4, p(edges), p(dims), 32, 0) == -1
    assert b"cutoff 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(3, 5, 0, 2.0, 2, p(deg), 1, 4, p(edges), p(dims), 32, 0) == -1
    assert b"averaged needs same" in lib.mdx_last_error()
    for args in ((3, 5, 0, 2.0, 2, None, 0, 4, p(edges), p(dims), 32, 0),
                 (3, 5, 0, 2.0, 2, p(deg), 0, 4, None, p(dims), 32, 0),
                 (3, 5, 0, 2.0, 2, p(deg), 0, 4, p(edges), None, 32, 0)):
        assert create(*args) == -1
        assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_boo_create(None, 0, 3, 5, 0, 2.0, 2, p(deg), 0, 4, p(edges), p(dims), 32, 0) == -1
    assert lib.mdx_boo_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_boo_result(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_boo_frames(None, None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_boo_values(None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    eng = _core.BondOrderEngine
    assert (eng.TILE, eng.JCHUNK, eng.MAX_NEIGHBORS, eng.MAX_DEGREE, eng.MAX_DEGREES) == (256, 1024, 64, 12, 4)
    assert (eng.SUM_TILE, cases.SUM_TILE, cases.MAX_DEGREE) == (64, 64, 12)


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _core.BondOrderEngine(2, 3, 2.0, [4, 6], EDGES, DIMS)
    one = _core.BondOrderEngine(5, None, 2.0, [6], EDGES, DIMS, same=True, averaged=True, max_neighbors=4,
                                keep_values=True)
    try:
        assert (two.n_rows, two.n_degrees, two.n_kinds, two.n_bins, two.max_neighbors) == (5, 2, 1, 4, 32)
        assert (one.n_rows, one.n_degrees, one.n_kinds, one.n_bins, one.max_neighbors) == (5, 1, 2, 4, 4)
        for eng in (two, one):
            with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
                eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="7 rows given, the groups hold 5"):
                eng.accumulate_device(rows, 7, 2)
            with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
            with pytest.raises(ValueError, match="index 7 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 7])
            for frames in (-1, 32769):
                with pytest.raises(ValueError, match="frames must lie in"):
                    eng.set_slab_frames(frames)
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            eng.set_slab_frames(0)
            eng.reset()
            eng.synchronize()
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "bonds": 0,
                                   "degenerate": 0, "max_row": 0}
            got = eng.frames()
            assert got["sums"].shape == (0, eng.n_degrees, eng.n_kinds) and got["counted"].shape == (0,)
        assert one.values().shape == (0, 1, 2, 5)
        with pytest.raises(ValueError, match="keep_values"):
            two.values()
    finally:
        two.close()
        one.close()


# ---------------------------------------------------------------- the restatement against the definitions

ALL_DEGREES = [list(range(1, 5)), list(range(5, 9)), list(range(9, 13))]
TOL_DEFINITION, TOL_ROTATION = cases.TOL_DEFINITION, cases.TOL_ROTATION
TOL_CLOSED, TOL_AVERAGED = cases.TOL_CLOSED, cases.TOL_AVERAGED
BINS = np.linspace(0.0, 1.0, 101)


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@pytest.mark.parametrize("seed", [5, 6])
def test_restatement_equals_the_definition_and_is_rotation_invariant(seed):
    """Random clusters of 120 points in a ball of radius 5.5 around the origin of a box of 40 (no image is ever
    taken), cutoff 3.0, and the same cluster turned by a random rotation (float64 coordinates, so that the turned
    copy is the same cluster to 1e-15).  Largest differences seen: restatement - definition 1.2e-15, turned -
    plain 1.0e-15."""
    rng = np.random.default_rng(seed)
    n, dims = 120, np.full(3, 40.0)
    x = rng.normal(size=(3 * n, 3))
    x = (x / np.linalg.norm(x, axis=1)[:, None] * 5.5 * rng.uniform(0.0, 1.0, (3 * n, 1)) ** (1 / 3))[:n]
    turned = x @ _rotation(rng).T
    near = cases.neighbours(x, n, True, 3.0, dims)[0]
    np.testing.assert_array_equal(cases.neighbours(turned, n, True, 3.0, dims)[0], near)     # the same bonds
    rows = near.sum(axis=1)
    assert 4 < rows.mean() < 20 and rows.max() <= 32 and len(set(rows.tolist())) > 3
    seen_definition = seen_rotation = 0.0
    for degrees in ALL_DEGREES:
        plain = cases.restate(x[None], n, None, 3.0, degrees, BINS, dims, same=True, averaged=True)["values"]
        other = cases.restate(turned[None], n, None, 3.0, degrees, BINS, dims, same=True, averaged=True)["values"]
        for values, points in ((plain, x), (other, turned)):
            want = cases.define(points[None], n, 3.0, degrees, dims, averaged=True)
            np.testing.assert_array_equal(np.isnan(values), np.isnan(want))
            seen_definition = max(seen_definition, float(np.nanmax(np.abs(values - want))))
        seen_rotation = max(seen_rotation, float(np.nanmax(np.abs(other - plain))))
        assert np.nanmin(plain) >= 0.0 and np.nanmax(plain) <= 1.0 + 1e-12
    print(f"restatement - definition {seen_definition:.3g}, turned - plain {seen_rotation:.3g}")
    assert seen_definition <= TOL_DEFINITION
    assert seen_rotation <= TOL_ROTATION


def test_restatement_equals_the_definition_across_the_faces_of_a_box():
    """Points all through a periodic box (the minimum image is taken) and disjoint groups.  Largest difference seen:
    4.5e-15."""
    dims = np.array([14.0, 15.0, 16.0])
    pos = cases.cloud(1, 2, 150, dims)
    seen = 0.0
    for degrees in ALL_DEGREES:
        got = cases.restate(pos, 150, None, 3.0, degrees, BINS, dims, same=True, averaged=True)
        want = cases.define(pos, 150, 3.0, degrees, dims, averaged=True)
        np.testing.assert_array_equal(np.isnan(got["values"]), np.isnan(want))
        seen = max(seen, float(np.nanmax(np.abs(got["values"] - want))))
        apart = cases.restate(pos, 50, 100, 3.0, degrees, BINS, dims)
        want = cases.define(pos, 50, 3.0, degrees, dims, same=False)
        seen = max(seen, float(np.nanmax(np.abs(apart["values"] - want))))
        assert np.isnan(apart["values"]).sum() == len(degrees) * int((50 - apart["counted"]).sum())    # the isolated
    print(f"restatement - definition {seen:.3g}")
    assert seen <= TOL_DEFINITION


@pytest.mark.parametrize("name", ["fcc", "bcc", "sc"])
def test_restatement_reproduces_the_closed_forms_of_the_lattices(name):
    """sc: q4 = sqrt(7/12), q6 = sqrt(1/8); bcc with 8 neighbours: sqrt(7/27), sqrt(32/81); fcc: sqrt(7/192),
    sqrt(169/512); and qbar_l == q_l where every centre has the same shell.  Largest differences seen: 5.6e-16 against
    the closed forms, 2.3e-16 between qbar_l and q_l."""
    build, cutoff, shell, closed = cases.LATTICES[name]
    pos, dims = build()
    n = pos.shape[1]
    got = cases.restate(pos, n, None, cutoff, [4, 6], BINS, dims, same=True, averaged=True)
    assert got["coordination"][shell] == n and got["coordination"].sum() == n and got["max_row"] == shell
    assert got["bonds"] == n * shell and got["degenerate"] == 0 and got["counted"].tolist() == [n]
    seen_closed = seen_averaged = 0.0
    for d, l in enumerate((4, 6)):
        seen_closed = max(seen_closed, float(np.abs(got["values"][0, d] - closed[l]).max()))
        seen_averaged = max(seen_averaged, float(np.abs(got["values"][0, d, 1] - got["values"][0, d, 0]).max()))
        want = cases.define(pos, n, cutoff, [l], dims, averaged=True)
        assert np.abs(got["values"][0, d] - want[0, 0]).max() <= TOL_DEFINITION
    print(f"{name}: closed forms {seen_closed:.3g}, qbar - q {seen_averaged:.3g}")
    assert seen_closed <= TOL_CLOSED
    assert seen_averaged <= TOL_AVERAGED
    # the histogram and the sums follow from the values
    for d in range(2):
        for k in range(2):
            np.testing.assert_array_equal(got["counts"][d, k], np.histogram(got["values"][0, d, k], bins=BINS)[0])
            assert got["sums"][0, d, k] == cases.tile_sum(got["values"][0, d, k])
            total = got["values"][0, d, k].sum()                 # any order of the float64 additions
            assert abs(got["sums"][0, d, k] - total) <= n * 2.0 ** -52 * total
    assert not got["outside"].any()


def test_tables_and_tile_sums_of_the_restatement():
    """N[l][m] is the normalisation of Y_lm (against math.factorial in one expression), the double factorials are
    exact, and the tile sums leave a NaN out."""
    for l in range(13):
        for m in range(l + 1):
            want = (-1) ** m * math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            assert abs(cases.NORM[l, m] - want) <= 4 * 2.0 ** -53 * abs(want)
    assert cases.DOUBLE_FACTORIAL[:5] == [1.0, 1.0, 3.0, 15.0, 105.0] and cases.DOUBLE_FACTORIAL[12] == 316234143225.0
    assert cases.FOUR_PI == 4.0 * np.pi and cases.K_L[6] == 4.0 * np.pi / 13.0
    assert cases.tile_sum(np.array([np.nan, 1.0, 2.0] + [np.nan] * 70 + [0.5])) == 3.5
    assert cases.tile_sum(np.full(3, np.nan)) == 0.0
