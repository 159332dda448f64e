"""
TetrahedralOrder without a GPU: the restatement of the device contract (``tetrahedral_cases``) against the order rule,
the textbook formula and fixed figures; the table of r2 the class hands the engine; every argument error of the class
and of ``mdx_tet_create``; and the plan's chunk choice.  Nothing here touches a device.
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import TetrahedralOrder
from mdhelper_amd.analysis.order import distance_table

import tetrahedral_cases as cases

Q_EDGES, S_EDGES, D_EDGES = np.linspace(-0.5, 1.0, 151), np.linspace(0.0, 1.0, 101), np.linspace(0.0, 3.0, 61)


# ---------------------------------------------------------------- the restatement

def test_the_order_is_a_stable_argsort_of_r2():
    """lexsort((j, r2)) against a stable argsort over all candidates, on the lattice whose ties are bit-equal and on
    a cloud that has none."""
    lattice, dims = cases.sc(5)
    for pos, box, cutoff in ((lattice, dims, 1.5), (cases.cloud(3, 1, 90, [7.0, 7.0, 7.0]), np.full(3, 7.0), 3.0)):
        near, _, r2 = cases.pairs(pos[0].astype(np.float64), pos.shape[1], True, cutoff, box)
        ties = 0
        for i in range(pos.shape[1]):
            stable = np.argsort(r2[i], kind="stable")
            stable = stable[near[i][stable]]
            np.testing.assert_array_equal(cases.ordered(near[i], r2[i]), stable)
            ties += len(stable) - len(np.unique(r2[i][stable]))
        assert (ties > 0) == (pos is lattice)


def test_q_agrees_with_the_textbook_form():
    """About 30 float64 operations on values of order 1: 1e-12 absolute."""
    rng = np.random.default_rng(8)
    w = rng.normal(size=(4000, 4, 3)) * rng.uniform(0.5, 3.0, size=(4000, 4, 1))
    q, sk = cases.q_sk(w, cases.r2_of(w))
    worst = float(np.abs(q - cases.textbook_q(w)).max())
    print(f"q against the textbook form: {worst:.3g}")
    assert worst <= 1e-12
    assert q.min() >= -3.0 and q.max() <= 1.0 and sk.min() >= 0.0 and sk.max() <= 1.0
    r = np.sqrt(cases.r2_of(w))
    plain = 1.0 - ((r - r.mean(axis=-1, keepdims=True)) ** 2).sum(axis=-1) / (12.0 * r.mean(axis=-1) ** 2)
    assert np.abs(sk - plain).max() <= 1e-12


def test_fixed_figures():
    tetrahedron = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    q, sk = cases.q_sk(tetrahedron, cases.r2_of(tetrahedron))
    assert abs(q - 1.0) <= 1e-15 and sk == 1.0
    square = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    q, sk = cases.q_sk(square, cases.r2_of(square))
    assert abs(q - 0.5) <= 1e-15 and abs(q - (1.0 - 3.0 / 8.0 * (4.0 / 9.0 + 8.0 / 9.0))) <= 1e-15 and sk == 1.0
    # three neighbours almost on the centre and one at R: rbar -> R / 4, the spread -> 12 rbar^2, S_k -> 0
    for eps in (1e-3, 1e-6, 1e-9):
        spread = np.array([[eps, 0.0, 0.0], [0.0, eps, 0.0], [0.0, 0.0, eps], [2.0, 0.0, 0.0]])
        sk = cases.q_sk(spread, cases.r2_of(spread))[1]
        assert 3.0 * eps <= sk <= 5.0 * eps                          # 8 eps / (R + 3 eps) with R = 2


def test_the_restatement_on_a_lattice_and_a_short_system():
    pos, dims = cases.diamond(2)
    want = cases.restate(pos, 64, None, 2.0, 4, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    assert np.abs(want["values"][0, 0] - 1.0).max() <= 1e-12 and (want["values"][0, 1] == 1.0).all()
    assert want["found"].tolist() == [0, 0, 0, 0, 64] and want["counted"].tolist() == [64]
    assert want["q_counts"][-1] == 64 and want["distance_counts"].sum(axis=1).tolist() == [64] * 4
    few = cases.restate(cases.cloud(1, 2, 4, dims), 4, None, 4.0, 5, Q_EDGES, S_EDGES, D_EDGES, dims, same=True)
    assert np.isnan(few["values"]).all() and not few["counted"].any() and few["found"][4:].sum() == 0
    assert few["found"].sum() == 8 and not few["q_counts"].any() and not few["sums"].any()


@pytest.mark.parametrize("edges", [np.linspace(0.0, 3.0, 61), np.linspace(0.3, 4.7, 12),
                                   np.array([0.1, 1.0 / 3.0, 2.5]), np.sqrt(np.array([0.5, 2.0, 3.0, 7.0]))])
def test_the_table_of_r2_counts_like_the_edges_of_the_distance(edges):
    """Around every threshold, the r2 within a few ulp on either side fall where numpy.histogram puts their roots."""
    table = distance_table(edges)
    assert table.shape == edges.shape and np.all(np.diff(table) > 0)
    probes = []
    for t in np.concatenate((table, edges * edges)):
        x = y = t
        for _ in range(6):
            x, y = np.nextafter(x, np.inf), np.nextafter(y, -np.inf)
            probes += [x, y]
        probes.append(t)
    r2 = np.array([p for p in probes if p >= 0.0])
    np.testing.assert_array_equal(np.histogram(r2, bins=table)[0], np.histogram(np.sqrt(r2), bins=edges)[0])
    assert ((r2 >= table[0]) & (r2 <= table[-1])).sum() == np.histogram(np.sqrt(r2), bins=edges)[0].sum()


# ---------------------------------------------------------------- the engine's arguments

def engine(n0=10, n1=None, cutoff=2.0, **kw):
    args = dict(q_edges=Q_EDGES, s_edges=S_EDGES, distance_thresholds=distance_table(D_EDGES), dims=[8.0, 9.0, 10.0],
                same=n1 is None)
    args.update(kw)
    return _core.TetrahedralEngine(n0, n1, cutoff, args.pop("q_edges"), args.pop("s_edges"),
                                   args.pop("distance_thresholds"), args.pop("dims"), **args)


@pytest.mark.parametrize("kw,text", [
    (dict(n_nearest=3), "n_nearest"), (dict(n_nearest=9), "n_nearest"),
    (dict(n0=0), "centers must hold"), (dict(n0=5, n1=0, same=False), "neighbors must hold"),
    (dict(n0=5, n1=6, same=True), "centers themselves"),
    (dict(cutoff=0.0), "cutoff must be positive"), (dict(cutoff=np.inf), "cutoff must be positive"),
    (dict(cutoff=np.nan), "cutoff must be positive"), (dict(cutoff=4.01), "half the shortest box length"),
    (dict(dims=[8.0, -1.0, 8.0]), r"dims\[1\]"), (dict(dims=[8.0, 8.0]), "three box lengths"),
    (dict(q_edges=[0.0, 1.0, 0.5]), "q_edges must be strictly increasing"),
    (dict(s_edges=[0.0, np.inf]), "s_edges must be finite"),
    (dict(distance_thresholds=[1.0, 1.0]), "distance_thresholds must be strictly increasing"),
    (dict(q_edges=[0.0]), "q_edges must hold"), (dict(s_edges=np.zeros((2, 2))), "s_edges must hold"),
])
def test_every_argument_error_of_create_needs_no_device(kw, text):
    with pytest.raises(ValueError, match=text):
        engine(**kw)


def test_create_checks_its_pointers():
    h = ctypes.c_void_p()
    table = np.array([0.0, 1.0])
    p = table.ctypes.data_as(ctypes.c_void_p)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        rc = _lib.lib().mdx_tet_create(ctypes.byref(h), 0, 5, 5, 1, 4, 0.4, 1, args[0], 1, args[1], 1, args[2],
                                       args[3], 0)
        assert rc == -1 and _lib.lib().mdx_last_error() == b"NULL argument"


def test_a_handle_lives_without_a_device():
    """create, set_chunk, set_slab_frames, the plan of a pinned chunk, stats, reset, synchronize and close."""
    eng = engine(n0=700, n_nearest=6, cutoff=4.0)
    try:
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "degenerate": 0,
                               "chunks": 0}
        for bad in (-256, 100, 255, 257):
            with pytest.raises(ValueError, match="multiple of 256"):
                eng.set_chunk(bad)
        eng.set_chunk(512)
        eng.set_slab_frames(7)
        assert eng.plan() == {"slab_frames": 7, "ring_frames": 0, "chunk": 512}
        eng.set_chunk(4096)                                         # beyond the candidates: all of them, one chunk
        assert eng.plan()["chunk"] == 768
        with pytest.raises(ValueError, match=r"frames must lie in \[0, 32768\]"):
            eng.set_slab_frames(32769)
        assert eng.frames()["sums"].shape == (0, 2)
        with pytest.raises(ValueError, match="keep_values"):
            eng.values()
        eng.reset()
        eng.synchronize()
        with pytest.raises(ValueError, match="rows given, the groups hold 700"):
            eng.accumulate(np.zeros((1, 699, 3), dtype=np.float32))
    finally:
        eng.close()
    for name, text in (("set_chunk", b"NULL handle"), ("stats", b"NULL handle"), ("plan", b"NULL argument"),
                       ("result", b"NULL argument"), ("frames", b"NULL argument"), ("values", b"NULL argument")):
        fn = getattr(_lib.lib(), f"mdx_tet_{name}")
        assert fn(*(0 if t in (ctypes.c_int, ctypes.c_int64) else None for t in fn.argtypes)) == -1
        assert _lib.lib().mdx_last_error() == text


@pytest.mark.parametrize("n0,n1,frames,cus,chunk", [
    (16384, 16384, 16, 256, 16384),     # 64 tiles x 16 frames fill 256 units: one chunk
    (16384, 16384, 4, 256, 16384),      # 256 blocks: just full
    (16384, 16384, 3, 256, 8192),       # 192 blocks: two parts
    (16384, 16384, 1, 256, 4096),       # 64 blocks: four parts
    (2000, 2000, 1, 256, 256),          # 8 tiles, 32 parts of 63 candidates: a stage each
    (2000, 2000, 40, 256, 2048),        # 320 blocks: one chunk, the candidates rounded up to the stage
    (300, 700, 3, 256, 256),            # 6 blocks, 43 parts: 17 candidates round up to one stage
    (300, 700, 3, 4, 768),
    (1, 100000, 1, 256, 512),           # 391 candidates a part
    (1, 1, 1, 256, 256),
    (257, 1000, 1, 3, 512),             # 2 tiles, 2 parts
])
def test_the_plan_chooses_the_chunk_from_tiles_frames_and_compute_units(n0, n1, frames, cus, chunk):
    got = _core.TetrahedralEngine.chunk_for(n0, n1, frames, cus)
    assert got == chunk and got % _core.TetrahedralEngine.STAGE == 0
    tiles = -(-n0 // _core.TetrahedralEngine.TILE)
    if tiles * frames >= cus:
        assert got >= n1                                            # one chunk wherever the device is full already
    else:
        parts = -(-n1 // got)
        assert parts <= -(-cus // (tiles * frames))                 # never more parts than it takes to fill it
    with pytest.raises(ValueError, match="at least 1"):
        _core.TetrahedralEngine.chunk_for(n0, n1, 0, cus)


def test_the_constants():
    e = _core.TetrahedralEngine
    assert (e.MIN_NEAREST, e.MAX_NEAREST, e.LDS_BINS, e.STAGE, e.TILE, e.SUM_TILE) == (4, 8, 1024, 256, 256, 64)
    assert e.SUM_TILE == cases.SUM_TILE
    for name in ("create", "set_chunk", "chunk_for", "plan", "result", "frames", "values", "stats", "accumulate",
                 "accumulate_device", "accumulate_traj", "synchronize", "reset", "destroy", "enable_timing",
                 "set_slab_frames"):
        assert f"mdx_tet_{name}" in _lib.EXPORTS


# ---------------------------------------------------------------- the class's arguments

@pytest.fixture(scope="module")
def universe():
    pos = cases.cloud(2, 2, 30, [9.0, 10.0, 11.0])
    boxes = np.tile(np.array([9.0, 10.0, 11.0, 90.0, 90.0, 90.0], dtype=np.float32), (2, 1))
    return mdhelper_amd.ArrayUniverse(pos, boxes, dt=1.0)


def test_class_defaults(universe):
    t = TetrahedralOrder(universe.atoms, verbose=False)
    assert t._cutoff == 4.5 and t._n_nearest == 4 and t._same and t._shard_frames
    np.testing.assert_array_equal(t._q_edges, np.linspace(-0.5, 1.0, 151))
    np.testing.assert_array_equal(t._s_edges, np.linspace(0.0, 1.0, 101))
    np.testing.assert_array_equal(t._d_edges, np.linspace(0.0, 4.5, 201))
    t = TetrahedralOrder(universe.select(np.arange(10)), universe.select(np.arange(12, 30)), cutoff=3.0,
                         distance_range=(1.0, 2.0), distance_bins=4, n_nearest=8, verbose=False)
    assert not t._same and (t._n_centers, t._n_neighbors) == (10, 18)
    assert t._d_edges.tolist() == [1.0, 1.25, 1.5, 1.75, 2.0]
    np.testing.assert_array_equal(t._index, np.concatenate((np.arange(10), np.arange(12, 30))))
    w = TetrahedralOrder.from_molecules(universe.atoms, 10, verbose=False)
    np.testing.assert_array_equal(w._index, np.arange(0, 30, 3))
    assert w._same and w._n_centers == 10
    np.testing.assert_array_equal(TetrahedralOrder.from_molecules(universe.atoms, 10, atom=2, verbose=False)._index,
                                  np.arange(2, 30, 3))


@pytest.mark.parametrize("kw,error,text", [
    (dict(drop_axis=2), TypeError, "drop_axis"),
    (dict(n_nearest=3), ValueError, "n_nearest"), (dict(n_nearest=9), ValueError, "n_nearest"),
    (dict(n_nearest=4.5), ValueError, "n_nearest"),
    (dict(cutoff=0.0), ValueError, "cutoff"), (dict(cutoff=np.inf), ValueError, "cutoff"),
    (dict(cutoff=4.6), ValueError, "half the shortest box length"),
    (dict(dimensions=[8.0, 8.0]), ValueError, "length 3"),
    (dict(dimensions=[8.0, 8.0, 8.0], cutoff=4.1), ValueError, "half the shortest box length"),
    (dict(n_bins=0), ValueError, "n_bins"), (dict(range=(1.0, 1.0)), ValueError, "'range'"),
    (dict(range=(0.0, np.inf)), ValueError, "'range'"),
    (dict(sk_bins=0), ValueError, "sk_bins"), (dict(sk_range=(1.0, 0.0)), ValueError, "sk_range"),
    (dict(distance_bins=0), ValueError, "distance_bins"),
    (dict(distance_range=(2.0, 1.0)), ValueError, "distance_range"),
    (dict(distance_range=(-1.0, 1.0)), ValueError, "distance_range"),
    (dict(distance_range=(0.0, 1.0, 2.0)), ValueError, "distance_range"),
])
def test_class_argument_errors(universe, kw, error, text):
    with pytest.raises(error, match=text):
        TetrahedralOrder(universe.atoms, verbose=False, **kw)


def test_class_group_errors(universe):
    with pytest.raises(ValueError, match="share some atoms"):
        TetrahedralOrder(universe.select(np.arange(10)), universe.select(np.arange(5, 20)), verbose=False)
    with pytest.raises(ValueError, match="molecules of equal size"):
        TetrahedralOrder.from_molecules(universe.atoms, 7, verbose=False)
    with pytest.raises(ValueError, match="'atom' must lie in"):
        TetrahedralOrder.from_molecules(universe.atoms, 10, atom=3, verbose=False)

