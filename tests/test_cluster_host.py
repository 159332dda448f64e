"""
Host-side checks of the cluster analysis that need no GPU: the argument handling of ``analysis.cluster.Clusters``,
the argument errors of the engine, which are raised before any device is touched (a handle touches its device with the
first frame), the host helpers ``find_connected_nodes`` / ``depth_first_search``, and the arithmetic of
``Clusters._conclude`` on the integers of a stub engine.

Not reachable without a device, and therefore checked in ``test_gpu_cluster.py``: ``set_slab_frames`` after the first
frame and a row beyond ``max_neighbors`` (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.algorithm.utility import depth_first_search, find_connected_nodes
from mdhelper_amd.analysis import Clusters, cluster


def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


# ---------------------------------------------------------------- the class

def test_constructor_errors():
    u = _universe()
    assert mdhelper_amd.analysis.Clusters is cluster.Clusters
    a, b = u.select(np.arange(5)), u.select(np.arange(5, 12))
    unlike = [[0.0, 3.5], [3.5, 0.0]]
    # the groups
    with pytest.raises(ValueError, match="share some atoms"):
        Clusters([a, u.select(np.arange(4, 12))], 5.0)
    with pytest.raises(ValueError, match="share some atoms"):
        Clusters([a, b, u.select([7])], 5.0)
    with pytest.raises(ValueError, match="at least one atom"):
        Clusters([a, u.select(np.arange(0))], 5.0)
    with pytest.raises(ValueError, match="between 1 and 8 groups"):
        Clusters([u.select([i]) for i in range(9)], 5.0)
    with pytest.raises(ValueError, match="between 1 and 8 groups"):
        Clusters([], 5.0)
    Clusters([u.select([i]) for i in range(8)], 5.0)
    # the cutoff table
    with pytest.raises(ValueError, match="must be symmetric"):
        Clusters([a, b], [[0.0, 3.5], [3.0, 0.0]])
    with pytest.raises(ValueError, match="finite and not negative"):
        Clusters([a, b], [[0.0, -3.5], [-3.5, 0.0]])
    with pytest.raises(ValueError, match="finite and not negative"):
        Clusters([a, b], [[0.0, np.nan], [np.nan, 0.0]])
    with pytest.raises(ValueError, match="finite and not negative"):
        Clusters([a, b], [[np.inf, 1.0], [1.0, 1.0]])
    with pytest.raises(ValueError, match="finite and not negative"):
        Clusters(a, -1.0)
    with pytest.raises(ValueError, match="at least one positive entry"):
        Clusters([a, b], [[0.0, 0.0], [0.0, 0.0]])
    with pytest.raises(ValueError, match="at least one positive entry"):
        Clusters(a, 0.0)
    for wrong in ([3.5, 3.5], [[3.5]], np.full((3, 3), 3.5), np.full((2, 2, 2), 3.5)):
        with pytest.raises(ValueError, match="a number or a 2 x 2 table"):
            Clusters([a, b], wrong)
    with pytest.raises(ValueError, match="a number or a 1 x 1 table"):
        Clusters(a, unlike)
    # the box: too small for the largest cutoff, none at all, not orthorhombic
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        Clusters(u.atoms, 20.5)                                                  # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        Clusters([a, b], [[1.0, 2.0], [2.0, 20.5]])                              # the largest entry counts
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        Clusters(u.atoms, 15.0, dimensions=[29.0, 60.0, 60.0])
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        Clusters(u.atoms, 21.5, drop_axis="z")                                   # x is still 40
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        Clusters(_universe(dims=None).atoms, 5.0)
    with pytest.raises(ValueError, match="orthorhombic"):
        Clusters(_universe(angles=(90.0, 90.0, 60.0)).atoms, 5.0)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        Clusters(u.atoms, 5.0, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="positive and finite"):
        Clusters(u.atoms, 5.0, dimensions=[40.0, np.nan, 40.0])
    with pytest.raises(ValueError, match="drop_axis"):
        Clusters(u.atoms, 5.0, drop_axis=3)
    for slots in (0, 65, -3):
        with pytest.raises(ValueError, match="'max_neighbors' must lie in \\[1, 64\\]"):
            Clusters(u.atoms, 5.0, max_neighbors=slots)
    Clusters(u.atoms, 20.0)                                                      # exactly half is allowed
    Clusters(u.atoms, 21.0, drop_axis="x")                                       # x dropped: 42 / 2 = 21
    Clusters(_universe(dims=None).atoms, 5.0, dimensions=[30.0, 31.0, 32.0])
    Clusters(u.atoms, 5.0, max_neighbors=1)
    Clusters(u.atoms, 5.0, max_neighbors=64)
    # what the arguments become: rows of group 0, then group 1, whatever their order in the frame
    two = Clusters([b, a], unlike, drop_axis="z", max_neighbors=8, store_labels=True)
    np.testing.assert_array_equal(two._index, [5, 6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4])
    np.testing.assert_array_equal(two._species, [0] * 7 + [1] * 5)
    assert two._species.dtype == np.int32
    np.testing.assert_array_equal(two._n_group, [7, 5])
    np.testing.assert_array_equal(two._cutoff, unlike)
    assert (two._N, two._drop_axis, two._max_neighbors, two._store_labels) == (12, 2, 8, True)
    one = Clusters(a, 5.0)
    np.testing.assert_array_equal(one._cutoff, [[5.0]])
    np.testing.assert_array_equal(one._dimensions, [40.0, 42.0, 44.0])
    assert (one._N, one._drop_axis, one._max_neighbors, one._store_labels) == (5, None, 32, False)
    np.testing.assert_array_equal(Clusters([a, b], 5.0)._cutoff, [[5.0, 5.0], [5.0, 5.0]])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            Clusters(_universe().atoms, 5.0, verbose=False).run()
        eng = _core.ClusterEngine(np.zeros(12, dtype=np.int32), 2.0, [10.0, 10.0, 10.0])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- _conclude on a stub engine

class Stub:
    """Stands in for ``_core.ClusterEngine``: records what it is fed and hands out hand-made integers, one frame
    like the next: 12 rows (7 of species 0, 5 of species 1) in clusters of 1, 1, 2, 3 and 5 rows."""
    MAX_SPECIES, MAX_NEIGHBORS = 8, 64
    made = []

    def __init__(self, species, cutoff, dims, *, n_species=None, zero_dims=0, max_neighbors=32, keep_labels=False,
                 dev=0, timing=False):
        self.species, self.cutoff, self.dims = np.array(species), np.array(cutoff), np.array(dims)
        self.args = dict(n_species=n_species, zero_dims=zero_dims, max_neighbors=max_neighbors,
                         keep_labels=keep_labels)
        self.n, self.n_frames, self.calls, self.closed = len(self.species), 0, [], False
        Stub.made.append(self)

    def accumulate(self, pos):
        self.calls.append(np.array(pos))
        self.n_frames += len(pos)

    def result(self):
        size_counts = np.zeros(self.n + 1, dtype=np.int64)
        size_counts[[1, 2, 3, 5]] = np.array([2, 1, 1, 1]) * self.n_frames
        species_counts = np.zeros((2, self.n + 1), dtype=np.int64)
        species_counts[0, [1, 2, 3, 5]] = np.array([2, 1, 1, 3]) * self.n_frames
        species_counts[1, [1, 2, 3, 5]] = np.array([0, 1, 2, 2]) * self.n_frames
        return {"size_counts": size_counts, "species_counts": species_counts}

    def frames(self):
        f = np.arange(self.n_frames, dtype=np.int64)
        return {"bonds": 7 + f, "n_clusters": 5 + 0 * f, "largest": 5 + 0 * f, "sum_squares": 40 + 0 * f}

    def labels(self):
        return np.tile(np.array([0, 1, 2, 2, 4, 4, 4, 0, 2, 4, 4, 4], dtype=np.int32), (self.n_frames, 1))

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    Stub.made = []
    monkeypatch.setattr(_core, "ClusterEngine", Stub)
    monkeypatch.setattr(_lib, "require_device", lambda dev=0: None)
    return Stub


def test_conclude_trims_and_forms_the_distributions(stub):
    u = _universe(n_frames=5)
    a, b = u.select(np.arange(5, 12)), u.select(np.arange(5))
    table = [[0.0, 3.5], [3.5, 2.0]]
    v = Clusters([a, b], table, drop_axis="y", max_neighbors=16, store_labels=True, verbose=False).run(step=2)
    eng = stub.made[0]
    assert eng.closed and eng.n_frames == 3
    assert eng.args == dict(n_species=2, zero_dims=2, max_neighbors=16, keep_labels=True)
    np.testing.assert_array_equal(eng.species, [0] * 7 + [1] * 5)
    np.testing.assert_array_equal(eng.cutoff, table)
    np.testing.assert_array_equal(eng.dims, [40.0, 42.0, 44.0])
    index = np.r_[5:12, 0:5]
    np.testing.assert_array_equal(np.concatenate(eng.calls), u.trajectory.frame_block([0, 2, 4])[:, index])
    res = v.results
    F, n = 3, 12
    np.testing.assert_array_equal(res.sizes, np.arange(6))                       # trimmed to the largest size seen
    np.testing.assert_array_equal(res.size_counts, [0, 6, 3, 3, 0, 3])
    np.testing.assert_array_equal(res.species_counts, [[0, 6, 3, 3, 0, 9], [0, 0, 3, 6, 0, 6]])
    assert res.size_counts.dtype == np.int64 and res.species_counts.dtype == np.int64
    np.testing.assert_array_equal(res.bonds, [7, 8, 9])
    np.testing.assert_array_equal(res.n_clusters, [5, 5, 5])
    np.testing.assert_array_equal(res.largest, [5, 5, 5])
    np.testing.assert_array_equal(res.sum_squares, [40, 40, 40])
    np.testing.assert_array_equal(res.size_distribution, res.size_counts / res.size_counts.sum())
    np.testing.assert_array_equal(res.size_distribution, np.array([0, 6, 3, 3, 0, 3]) / 15)
    np.testing.assert_array_equal(res.weight_distribution, res.sizes * res.size_counts / (F * n))
    np.testing.assert_array_equal(res.weight_distribution, np.array([0, 6, 6, 9, 0, 15]) / 36)
    np.testing.assert_array_equal(res.species_fractions, res.species_counts / (F * np.array([7, 5]))[:, None])
    np.testing.assert_array_equal(res.species_fractions[:, 1], [6 / 21, 0.0])   # the free fraction of each species
    np.testing.assert_array_equal(res.species_counts.sum(axis=0), res.sizes * res.size_counts)
    np.testing.assert_array_equal(res.mean_size, n / np.array([5, 5, 5]))
    np.testing.assert_array_equal(res.weight_mean_size, np.array([40, 40, 40]) / n)
    assert res.labels.shape == (3, 12) and res.labels.dtype == np.int32
    assert "results.sizes" in res.units
    # without store_labels there are none
    assert "labels" not in Clusters([a, b], table, verbose=False).run().results


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank, self.reduced = rank, []

    def allreduce(self, arr, op="sum"):
        arr = np.asarray(arr)
        assert arr.dtype in (np.int64, np.int32) and op == "sum"
        self.reduced.append(arr.copy())
        return arr * 2                      # "the other rank" held the same numbers


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_shard_frames_and_allreduce(stub, rank):
    u = _universe(n_frames=7)
    a, b = u.select(np.arange(7)), u.select(np.arange(7, 12))
    comm = TwoRanks(rank)
    v = Clusters([a, b], 3.5, store_labels=True, verbose=False, comm=comm).run()
    eng = stub.made[0]
    lo, hi = ((0, 4), (4, 7))[rank]
    assert eng.n_frames == hi - lo
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(lo, hi)))
    # the counts travel at their full length n + 1, this rank's rows inside zero-filled arrays over all frames
    sent = comm.reduced
    assert [s.shape for s in sent] == [(13,), (2, 13), (7,), (7,), (7,), (7,), (7, 12)]
    for rows in sent[2:]:
        assert not rows[:lo].any() and not rows[hi:].any()
    assert sent[3][lo:hi].all() and sent[6].dtype == np.int32
    np.testing.assert_array_equal(sent[0][[1, 2, 3, 5]], np.array([2, 1, 1, 1]) * (hi - lo))
    res = v.results
    np.testing.assert_array_equal(res.size_counts, 2 * sent[0][:6])
    np.testing.assert_array_equal(res.species_counts, 2 * sent[1][:, :6])
    np.testing.assert_array_equal(res.bonds, 2 * sent[2])
    np.testing.assert_array_equal(res.labels, 2 * sent[6])
    # the distributions are formed after the sum, over all 7 frames
    np.testing.assert_array_equal(res.weight_distribution, res.sizes * res.size_counts / (7 * 12))
    np.testing.assert_array_equal(res.species_fractions, res.species_counts / (7 * np.array([7, 5]))[:, None])


# ---------------------------------------------------------------- find_connected_nodes

def _components(graph):
    return sorted(sorted(group) for group in find_connected_nodes(graph))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_find_connected_nodes_against_scipy(seed):
    rng = np.random.default_rng(seed)
    n = 200 + 50 * seed
    pairs = rng.integers(0, n, (n * (seed + 1) // 3, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    graph = {i: [] for i in range(n)}
    for i, j in pairs:
        graph[int(i)].append(int(j))
        graph[int(j)].append(int(i))
    groups = find_connected_nodes(graph)
    m = csr_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    count, comp = connected_components(m, directed=False)
    assert len(groups) == count and 1 < count < n
    assert sorted(sum(groups, [])) == list(range(n))                            # every node once
    assert sorted(sorted(g) for g in groups) == sorted(sorted(np.flatnonzero(comp == c).tolist())
                                                        for c in range(count))
    assert [g[0] for g in groups] == sorted(g[0] for g in groups)               # in the order of their first node


def test_find_connected_nodes_needs_no_recursion():
    n = 5000                                            # a path: the recursive search dies at depth 1 000
    graph = {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)}
    assert find_connected_nodes(graph) == [list(range(n))]
    # any hashable node, in place, in depth-first preorder
    graph = {"a": ["c", "b"], "b": ["a"], "c": ["a", "d"], "d": ["c"], "e": []}
    assert find_connected_nodes(graph) == [["a", "c", "d", "b"], ["e"]]
    visited, group = {node: False for node in graph}, ["x"]
    visited["c"] = True                                 # a node marked beforehand is not passed
    depth_first_search(graph, "a", visited, group)
    assert group == ["x", "a", "b"] and visited == {"a": True, "b": True, "c": True, "d": False, "e": False}
    assert _components({1: [2], 2: [1], 3: []}) == [[1, 2], [3]]


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]


def test_engine_create_errors_need_no_device():
    sp = [0, 0, 1, 1, 1]
    unlike = [[0.0, 2.0], [2.0, 0.0]]
    for kwargs, word in ((dict(cutoff=[[0.0, 2.0], [1.5, 0.0]]), "must be symmetric"),
                         (dict(cutoff=[[0.0, -2.0], [-2.0, 0.0]]), "finite and not negative"),
                         (dict(cutoff=[[0.0, np.nan], [np.nan, 0.0]]), "finite and not negative"),
                         (dict(cutoff=[[np.inf, 1.0], [1.0, 1.0]]), "finite and not negative"),
                         (dict(cutoff=[[0.0, 0.0], [0.0, 0.0]]), "at least one positive entry"),
                         (dict(cutoff=0.0), "at least one positive entry"),
                         (dict(cutoff=[2.0, 2.0]), "a number or a 2 x 2 table"),
                         (dict(cutoff=np.full((3, 3), 2.0), n_species=2), "a number or a 2 x 2 table"),
                         (dict(species=[0, 2, 1, 1, 1]), "species\\[1\\] = 2 out of range \\[0, 2\\)"),
                         (dict(species=[0, 0, 1, -1, 1]), "species\\[3\\] = -1 out of range"),
                         (dict(species=[]), "at least one point"),
                         (dict(cutoff=2.0, n_species=9), "n_species must lie in \\[1, 8\\]"),
                         (dict(cutoff=2.0, n_species=0), "n_species must lie in \\[1, 8\\]"),
                         (dict(cutoff=5.5), "beyond half the shortest box length"),
                         (dict(cutoff=[[1.0, 2.0], [2.0, 5.5]]), "beyond half the shortest box length"),
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
        args = dict(species=sp, cutoff=unlike, dims=DIMS, n_species=None, zero_dims=0, max_neighbors=32)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.ClusterEngine(args["species"], args["cutoff"], args["dims"], n_species=args["n_species"],
                                zero_dims=args["zero_dims"], max_neighbors=args["max_neighbors"])
    # half the shortest kept length itself is allowed, and a dropped component does not count
    _core.ClusterEngine(sp, unlike, [4.0, 11.0, 12.0]).close()
    _core.ClusterEngine(sp, unlike, [1.0, 11.0, 12.0], zero_dims=1).close()
    _core.ClusterEngine(sp, 5.5, DIMS, zero_dims=1).close()
    _core.ClusterEngine(sp, unlike, DIMS, max_neighbors=1).close()
    _core.ClusterEngine([0], 2.0, DIMS, max_neighbors=64, keep_labels=True).close()
    _core.ClusterEngine(np.arange(8), np.full((8, 8), 2.0), DIMS).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    species, table, dims = np.array(sp, dtype=np.int32), np.array(unlike), np.array(DIMS)
    create = lambda *a: lib.mdx_clu_create(ctypes.byref(h), 0, *a)      # noqa: E731
    assert create(5, p(species), 2, p(table), p(dims), 0, 32, 0) == 0
    assert lib.mdx_clu_destroy(h) == 0
    assert create(5, p(species), 9, p(table), p(dims), 0, 32, 0) == -1
    assert b"n_species" in lib.mdx_last_error()
    assert create(5, p(species), 2, p(np.array([[0.0, 5.25], [5.25, 0.0]])), p(dims), 0, 32, 0) == -1
    assert b"cutoff 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(2 ** 31 // 3, p(species), 2, p(table), p(dims), 0, 32, 0) == -1
    assert b"2^31 / 3" in lib.mdx_last_error()
    for args in ((5, None, 2, p(table), p(dims), 0, 32, 0), (5, p(species), 2, None, p(dims), 0, 32, 0),
                 (5, p(species), 2, p(table), None, 0, 32, 0)):
        assert create(*args) == -1
        assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_clu_create(None, 0, 5, p(species), 2, p(table), p(dims), 0, 32, 0) == -1
    assert lib.mdx_clu_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_clu_result(None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_clu_labels(None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    eng = _core.ClusterEngine
    assert (eng.TILE, eng.JCHUNK, eng.MAX_NEIGHBORS, eng.MAX_SPECIES) == (256, 1024, 64, 8)


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _core.ClusterEngine([0, 0, 1, 1, 1], [[0.0, 2.0], [2.0, 0.0]], DIMS, zero_dims=2)
    one = _core.ClusterEngine(np.zeros(5), 2.0, DIMS, max_neighbors=4, keep_labels=True)
    try:
        assert (two.n, two.n_species, two.max_neighbors, two.keep_labels) == (5, 2, 32, False)
        assert (one.n, one.n_species, one.max_neighbors, one.keep_labels) == (5, 1, 4, True)
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
            out = np.zeros(3, dtype=np.int64)
            q = out.ctypes.data_as(ctypes.c_void_p)
            assert _lib.lib().mdx_clu_frames(eng.handle, q, q, q, q, 3) == -1
            assert b"3 frames asked for, 0 seen" in _lib.lib().mdx_last_error()
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            eng.set_slab_frames(0)
            eng.reset()
            eng.synchronize()
            assert all(len(v) == 0 and v.dtype == np.int64 for v in eng.frames().values())
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "max_row": 0,
                                   "sweeps": 0}
        assert one.labels().shape == (0, 5)
        with pytest.raises(ValueError, match="keep_labels"):
            two.labels()
    finally:
        two.close()
        one.close()
