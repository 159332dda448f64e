"""
Host-side checks of the spatial-distribution analysis that need no GPU: the argument handling of
``analysis.spatial.SpatialDistributionFunction``, what it derives (the feed index, the tables, the owners, the cutoff
and the edges), the argument errors of the engine, which are raised before any device is touched (a handle touches its
device with the first frame), and the NumPy restatement of the device contract against ``numpy.histogramdd`` and the
figures it was checked with.

Not reachable without a device, and therefore checked in ``test_gpu_spatial_distribution.py``: ``set_bins`` and
``set_slab_frames`` after the first frame (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import SpatialDistributionFunction, spatial
from spatial_distribution_cases import (AXIS, BISECTOR, BOX, F, N_MOL, cube_edges, local_coordinates, restate,
                                        shared_water, water_system)

RC2 = 75.0 * (1.0 + 2.0 ** -40)


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


def _groups(u):
    """Four waters O H H: origins, axis atoms, plane atoms, and the neighbours (every O, then every H)."""
    o = 3 * np.arange(4)
    return (u.select(o), u.select(o + 1), u.select(o + 2),
            [u.select(o), u.select(np.stack((o + 1, o + 2), axis=1).ravel())])


def test_constructor_errors():
    u = _universe()
    o, a, b, nb = _groups(u)
    SDF = SpatialDistributionFunction
    assert mdhelper_amd.analysis.SpatialDistributionFunction is spatial.SpatialDistributionFunction
    with pytest.raises(ValueError, match="'origins' holds 3 atoms, 'axis_atoms' 4 and 'plane_atoms' 4"):
        SDF(u.select([0, 3, 6]), a, b, nb)
    with pytest.raises(ValueError, match="at least one reference molecule"):
        SDF(*(u.select(np.zeros(0, dtype=int)),) * 3, nb)
    with pytest.raises(ValueError, match="three different atoms"):
        SDF(o, o, b, nb)
    with pytest.raises(ValueError, match="three different atoms"):
        SDF(o, a, a, nb)
    with pytest.raises(ValueError, match="'origins' holds an atom twice"):
        SDF(u.select([0, 0]), u.select([1, 4]), u.select([2, 5]), nb)
    with pytest.raises(ValueError, match="'neighbors' holds an atom twice"):
        SDF(o, a, b, [u.select([0, 3]), u.select([3, 4])])
    with pytest.raises(ValueError, match="at least one atom"):
        SDF(o, a, b, u.select(np.zeros(0, dtype=int)))
    with pytest.raises(ValueError, match="between 1 and 8 groups"):
        SDF(o, a, b, [u.select([k]) for k in range(9)])
    with pytest.raises(ValueError, match="between 1 and 8 groups"):
        SDF(o, a, b, [])
    SDF(o, a, b, [u.select([k]) for k in range(8)])
    with pytest.raises(ValueError, match="'frame'"):
        SDF(o, a, b, nb, frame="dipole")
    for bad in (0.0, -1.0, np.nan, [(0.0, 1.0), (1.0, 1.0), (0.0, 1.0)], [(0.0, 1.0), (0.0, 1.0)]):
        with pytest.raises(ValueError, match="'range' must be"):
            SDF(o, a, b, nb, range=bad)
    for bad in (0, 513, (4, 4), (4, 0, 4), 2.5):
        with pytest.raises(ValueError, match="'n_bins' must be an integer or three"):
            SDF(o, a, b, nb, n_bins=bad)
    with pytest.raises(ValueError, match="more than 2\\^26 counters"):
        SDF(o, a, b, nb, n_bins=(512, 512, 129))
    SDF(o, a, b, nb, n_bins=(512, 512, 128))
    for bad in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="'cutoff' must be positive and finite"):
            SDF(o, a, b, nb, cutoff=bad)
    with pytest.raises(ValueError, match="'owners' must hold one integer per neighbour atom, 12"):
        SDF(o, a, b, nb, owners=np.zeros(11, dtype=int))
    with pytest.raises(ValueError, match="'owners' must hold one integer"):
        SDF(o, a, b, nb, owners=np.zeros(12))
    for bad in (-2, 4):
        with pytest.raises(ValueError, match="'owners' must lie in \\[-1, 4\\)"):
            SDF(o, a, b, nb, owners=np.full(12, bad))
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        SDF(o, a, b, nb, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        SDF(*_groups(_universe(dims=None)))
    with pytest.raises(ValueError, match="orthorhombic"):
        SDF(*_groups(_universe(angles=(90.0, 90.0, 60.0))))
    v = SDF(o, a, b, nb)
    assert v._shard_frames is True and v._mode == AXIS and SDF(o, a, b, nb, frame="bisector")._mode == BISECTOR
    with pytest.raises(RuntimeError, match="run\\(\\)"):
        v.calculate_radial_average()
    with pytest.raises(ValueError, match="molecules of equal size"):
        SDF.from_molecules(u.atoms, 5)
    with pytest.raises(ValueError, match="places must lie in \\[0, 3\\)"):
        SDF.from_molecules(u.atoms, 4, plane=3)
    with pytest.raises(ValueError, match="places must lie in \\[0, 3\\)"):
        SDF.from_molecules(u.atoms, 4, neighbors=[(0,), (-1,)])
    with pytest.raises(ValueError, match="at least one group"):
        SDF.from_molecules(u.atoms, 4, neighbors=[])


def test_the_cutoff_default_and_the_half_box_error():
    u = _universe()
    o, a, b, nb = _groups(u)
    SDF = SpatialDistributionFunction
    v = SDF(o, a, b, nb)
    assert v._cutoff == float(np.sqrt(108.0) * (1.0 + 2.0 ** -40)) and v._cutoff > np.sqrt(108.0)
    for e in v._edges:
        np.testing.assert_array_equal(e, np.linspace(-6.0, 6.0, 61))
    # three (lo, hi) pairs and three bin counts: the sphere reaches the farthest corner
    w = SDF(o, a, b, nb, range=[(-1.0, 2.0), (-3.0, 0.5), (0.0, 4.0)], n_bins=(3, 7, 8))
    assert w._cutoff == float(np.sqrt(4.0 + 9.0 + 16.0) * (1.0 + 2.0 ** -40))
    np.testing.assert_array_equal(w._edges[0], np.linspace(-1.0, 2.0, 4))
    np.testing.assert_array_equal(w._edges[1], np.linspace(-3.0, 0.5, 8))
    np.testing.assert_array_equal(w._edges[2], np.linspace(0.0, 4.0, 9))
    assert SDF(o, a, b, nb, cutoff=4.5)._cutoff == 4.5
    # R = 11.6: the sphere of the cube is 20.09 > 40 / 2
    with pytest.raises(ValueError, match="beyond half the shortest box length.*smaller cutoff="):
        SDF(o, a, b, nb, range=11.6)
    SDF(o, a, b, nb, range=11.6, cutoff=20.0)                       # exactly half is allowed
    with pytest.raises(ValueError, match="beyond half the shortest box length.*smaller cutoff="):
        SDF(o, a, b, nb, cutoff=20.5)
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        SDF(o, a, b, nb, range=3.0, dimensions=[10.0, 60.0, 60.0])  # 5.196 > 5


def test_the_feed_index_the_tables_and_the_owners():
    u = _universe(n_atoms=14)
    SDF = SpatialDistributionFunction
    # a three-site water by from_molecules: the feed is the twelve atoms in order
    v = SDF.from_molecules(u.select(np.arange(12)), 4)
    np.testing.assert_array_equal(v._index, np.arange(12))
    np.testing.assert_array_equal(v._o_row, [0, 3, 6, 9])
    np.testing.assert_array_equal(v._a_row, [1, 4, 7, 10])
    np.testing.assert_array_equal(v._b_row, [2, 5, 8, 11])
    np.testing.assert_array_equal(v._p_row, [0, 3, 6, 9, 1, 2, 4, 5, 7, 8, 10, 11])
    np.testing.assert_array_equal(v._owner, [0, 1, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3])
    np.testing.assert_array_equal(v._group_start, [0, 4, 12])
    assert all(getattr(v, k).dtype == np.int32 for k in ("_o_row", "_a_row", "_b_row", "_p_row", "_owner"))
    assert v._group_start.dtype == np.int64 and (v._n_ref, v._n_p) == (4, 12)
    # the same from the groups given by hand: the default owners are the molecules the atoms frame
    w = SDF(*_groups(u))
    for key in ("_index", "_o_row", "_a_row", "_b_row", "_p_row", "_owner", "_group_start"):
        np.testing.assert_array_equal(getattr(w, key), getattr(v, key))
    # other places inside a molecule of four, one group: an atom that frames nothing is still its molecule's
    m = SDF.from_molecules(u.select(np.arange(2, 14)), 3, origin=3, axis=0, plane=2, neighbors=[(1, 3)])
    np.testing.assert_array_equal(m._index, np.arange(2, 14))
    np.testing.assert_array_equal(m._o_row, [3, 7, 11])
    np.testing.assert_array_equal(m._a_row, [0, 4, 8])
    np.testing.assert_array_equal(m._b_row, [2, 6, 10])
    np.testing.assert_array_equal(m._p_row, [1, 3, 5, 7, 9, 11])
    np.testing.assert_array_equal(m._owner, [0, 0, 1, 1, 2, 2])
    # hand-given groups in no order, atoms that take no part: the distinct atoms are fed once, ascending; a neighbour
    # that frames no molecule has no owner
    g = SDF(u.select([9, 2]), u.select([13, 4]), u.select([7, 0]), [u.select([11, 9, 0]), u.select([4])])
    np.testing.assert_array_equal(g._index, [0, 2, 4, 7, 9, 11, 13])
    np.testing.assert_array_equal(g._index[g._o_row], [9, 2])
    np.testing.assert_array_equal(g._index[g._a_row], [13, 4])
    np.testing.assert_array_equal(g._index[g._b_row], [7, 0])
    np.testing.assert_array_equal(g._index[g._p_row], [11, 9, 0, 4])
    np.testing.assert_array_equal(g._owner, [-1, 0, 1, 1])
    np.testing.assert_array_equal(g._group_start, [0, 3, 4])
    # an atom that frames two molecules (a shared plane atom) needs owners= where it is a neighbour, and only there
    shared = (u.select([0, 3]), u.select([1, 4]), u.select([2, 2]))
    with pytest.raises(ValueError, match="Atom 2 of 'neighbors' is a frame atom of several reference molecules.*"
                                         "owners="):
        SDF(*shared, u.select([2, 5]))
    np.testing.assert_array_equal(SDF(*shared, u.select([1, 5, 3]))._owner, [0, -1, 1])
    np.testing.assert_array_equal(SDF(*shared, u.select([2, 5]), owners=[1, -1])._owner, [1, -1])
    # an atom that frames one molecule twice over is no conflict (it cannot: the three differ), but the same atom as
    # the axis atom of one and the plane atom of another is
    with pytest.raises(ValueError, match="owners="):
        SDF(u.select([0, 3]), u.select([1, 4]), u.select([2, 1]), u.select([1]))


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            SpatialDistributionFunction(*_groups(_universe()), verbose=False).run()
        eng = _engine()
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 6, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- the restatement

@pytest.fixture(scope="module")
def figures():
    """The restatement on the shared water in both modes, R = 5, 20 bins per axis: computed once."""
    pos, edges = shared_water(), cube_edges(5.0, 20)
    return {mode: restate(pos, *water_system(), mode, RC2, edges, BOX, keep_local=True) for mode in (AXIS, BISECTOR)}


def test_the_restatement_counts_like_numpy_histogramdd(figures):
    edges = cube_edges(5.0, 20)
    for mode in (AXIS, BISECTOR):
        want = figures[mode]
        for g, local in enumerate(want["local"]):
            assert len(local) > want["counts"][g].sum()             # some near pairs lie in the sphere's caps
            np.testing.assert_array_equal(want["counts"][g], np.histogramdd(local, edges)[0].astype(np.int64))
    # the last bin is closed above, the others below: values on the edges themselves
    e = [np.array([-1.0, 0.0, 0.5, 1.0])] * 3
    o, a, b = np.array([0]), np.array([1]), np.array([2])
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0],                                    # O, A on +x, B on +y
                    [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [0.5, 0.0, 1.0], [1.0, 0.5, 0.0],
                    [1.00001, 0, 0], [0, -1.00001, 0]], dtype=np.float32) + 8.0
    p_row = np.arange(3, len(pts))
    owner = np.full(len(p_row), -1)
    got = restate(pts[None], o, a, b, [0, len(p_row)], p_row, owner, AXIS, 4.0, e, [16.0, 16.0, 16.0],
                  keep_local=True)
    np.testing.assert_array_equal(got["local"][0], pts[3:].astype(np.float64) - 8.0)    # e = the lab axes, exactly
    np.testing.assert_array_equal(np.argwhere(got["counts"][0]), [[0, 0, 0], [2, 1, 2], [2, 2, 1], [2, 2, 2]])
    np.testing.assert_array_equal(got["counts"][0], np.histogramdd(got["local"][0], e)[0].astype(np.int64))
    assert got["inside"][0] == 4 and got["evaluations"] == 6 and got["degenerate"] == 0


def test_the_restatement_gives_the_figures_it_was_checked_with(figures):
    pos, edges = shared_water(), cube_edges(5.0, 20)
    axis, bis = figures[AXIS], figures[BISECTOR]
    assert axis["counts"].shape == (2, 20, 20, 20) and axis["counts"].dtype == np.int64
    assert axis["counts"].sum() == axis["inside"].sum() == 298_789
    np.testing.assert_array_equal(axis["counts"].sum(axis=(1, 2, 3)), [99_728, 199_061])
    assert (axis["inside"].min(), axis["inside"].max()) == (24_783, 25_078)
    assert axis["degenerate"] == 0 and bis["degenerate"] == 0
    assert (axis["counts"] > 0).sum() == 16_000                     # every bin of both groups is hit
    assert axis["evaluations"] == F * (N_MOL * 3 * N_MOL - 3 * N_MOL) == bis["evaluations"]
    assert bis["counts"].sum() == bis["inside"].sum() == 298_345
    np.testing.assert_array_equal(bis["counts"].sum(axis=(1, 2, 3)), [99_518, 198_827])
    # without owners a molecule sees its own three atoms: the origin at (0, 0, 0), the hydrogens one unit away
    free = restate(pos, *water_system(owners=False), AXIS, RC2, edges, BOX)
    assert free["counts"].sum() - axis["counts"].sum() == F * N_MOL * 3 == 9_252
    assert free["evaluations"] == F * N_MOL * 3 * N_MOL
    np.testing.assert_array_equal((free["counts"] - axis["counts"]).sum(axis=(1, 2, 3)), [F * N_MOL, 2 * F * N_MOL])
    assert (free["counts"] - axis["counts"])[0, 10, 10, 10] == F * N_MOL


def test_swapping_axis_and_plane_atoms_mirrors_the_bisector_frame(figures):
    """The bisector is symmetric in A and B; the normal p x b changes sign with the swap, and e2 with it."""
    o, a, b, start, p_row, owner = water_system()
    swapped = restate(shared_water(), o, b, a, start, p_row, owner, BISECTOR, RC2, cube_edges(5.0, 20), BOX)
    np.testing.assert_array_equal(swapped["counts"], figures[BISECTOR]["counts"][:, :, ::-1, ::-1])
    np.testing.assert_array_equal(swapped["inside"], figures[BISECTOR]["inside"])
    assert (swapped["counts"] != figures[BISECTOR]["counts"]).any()


def test_the_restatement_counts_a_degenerate_molecule_once_and_none_of_its_pairs():
    dims = [16.0, 16.0, 16.0]
    base = np.array([[4, 4, 4], [5, 4, 4], [4, 5, 4],           # a sound molecule
                     [9, 9, 9], [9, 9, 9], [9, 10, 9],          # A on O
                     [2, 9, 9], [3, 9, 9], [2, 9, 9],           # B on O
                     [9, 2, 2], [10, 2, 2], [7, 2, 2],          # collinear: b = -2 a exactly
                     [4.5, 4.5, 4.5], [9.5, 9.5, 9.5], [2.5, 9.5, 9.5], [9.5, 2.5, 2.5]], dtype=np.float32)
    o, p_row = np.arange(0, 12, 3), np.arange(12, 16)
    e = cube_edges(2.0, 4)
    for mode in (AXIS, BISECTOR):
        got = restate(np.stack((base, base)), o, o + 1, o + 2, [0, 4], p_row, np.full(4, -1), mode, 9.0, e, dims)
        assert got["degenerate"] == 2 * 3 and got["evaluations"] == 2 * 16
        np.testing.assert_array_equal(got["inside"], [1, 1])        # the sound molecule's one partner
        uvt, near = local_coordinates(base, o, o + 1, o + 2, p_row, np.full(4, -1), mode, 9.0, dims)
        np.testing.assert_array_equal(np.argwhere(near), [[0, 0]])
        if mode == AXIS:
            np.testing.assert_array_equal(uvt[0, 0], [0.5, 0.5, 0.5])


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]
O_ROW, A_ROW, B_ROW, P_ROW, OWNER, START = [0, 3], [1, 4], [2, 5], [0, 3, 1, 2, 4, 5], [0, 1, 0, 0, 1, 1], [0, 2, 6]


def _engine(**kwargs):
    args = dict(n_rows=6, o_row=O_ROW, a_row=A_ROW, b_row=B_ROW, group_start=START, p_row=P_ROW, owner=OWNER, mode=0,
                cutoff=3.0, dims=DIMS)
    args.update(kwargs)
    return _core.SpatialDistributionEngine(*(args[k] for k in ("n_rows", "o_row", "a_row", "b_row", "group_start",
                                                                "p_row", "owner", "mode", "cutoff", "dims")))


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(cutoff=0.0), "cutoff must be positive and finite"),
                         (dict(cutoff=-2.0), "cutoff must be positive and finite"),
                         (dict(cutoff=np.nan), "cutoff must be positive and finite"),
                         (dict(cutoff=np.inf), "cutoff must be positive and finite"),
                         (dict(cutoff=5.5), "cutoff 5.5 reaches beyond half the shortest box length 10"),
                         (dict(dims=[5.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 11.0, 5.9]), "beyond half the shortest box length"),
                         (dict(mode=2), "mode must be 0 \\(axis\\) or 1 \\(bisector\\)"),
                         (dict(mode=-1), "mode must be 0"),
                         (dict(o_row=[], a_row=[], b_row=[]), "n_ref: there must be at least one reference molecule"),
                         (dict(o_row=[0]), "of one length"),
                         (dict(owner=[0, 1]), "of one length"),
                         (dict(group_start=[0]), "at least two"),
                         (dict(group_start=[0, 2, 5]), "end at the number of partners"),
                         (dict(group_start=[1, 2, 6]), "group_start\\[0\\] must be 0"),
                         (dict(group_start=[0, 4, 3, 6]), "group_start must not decrease: \\[1\\] = 4, \\[2\\] = 3"),
                         (dict(group_start=[0, 1, 2, 3, 4, 5, 6, 6, 6, 6]), "n_groups must lie in \\[1, 8\\]"),
                         (dict(group_start=[0, 0], p_row=[], owner=[]), "group_start: there must be at least one"),
                         (dict(o_row=[0, 6]), "o_row\\[1\\] = 6 out of range \\[0, 6\\)"),
                         (dict(o_row=[-1, 3]), "o_row\\[0\\] = -1 out of range"),
                         (dict(a_row=[1, 7]), "a_row\\[1\\] = 7 out of range"),
                         (dict(b_row=[-2, 5]), "b_row\\[0\\] = -2 out of range"),
                         (dict(p_row=[0, 3, 1, 2, 4, 6]), "p_row\\[5\\] = 6 out of range"),
                         (dict(o_row=[0, 0]), "o_row holds row 0 twice"),
                         (dict(p_row=[0, 3, 1, 1, 4, 5]), "p_row holds row 1 twice"),
                         (dict(a_row=[0, 4]), "a_row\\[0\\] = 0 is the molecule's origin"),
                         (dict(b_row=[2, 3]), "b_row\\[1\\] = 3 is the molecule's origin"),
                         (dict(b_row=[2, 4]), "b_row\\[1\\] = 4 is the molecule's axis atom"),
                         (dict(owner=[0, 2, 0, 0, 1, 1]), "owner\\[1\\] = 2 out of range \\[-1, 2\\)"),
                         (dict(owner=[0, 1, -2, 0, 1, 1]), "owner\\[2\\] = -2 out of range"),
                         (dict(n_rows=2 ** 31 // 3), "2\\^31 / 3"),
                         (dict(dims=[10.0, 0.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, np.nan, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0]), "three box lengths")):
        with pytest.raises(ValueError, match=word):
            _engine(**kwargs)
    _engine(cutoff=5.0).close()                                     # half the shortest length itself is allowed
    _engine(mode=1, owner=[-1] * 6).close()
    _engine(a_row=[1, 1], b_row=[2, 2]).close()                     # only the origins may not repeat
    _engine(group_start=[0, 0, 6, 6]).close()                       # a group may be empty
    eng = _engine(group_start=[0, 1, 2, 3, 4, 5, 6, 6, 6])
    assert (eng.n_rows, eng.n_ref, eng.n_p, eng.n_groups, eng.n_bins) == (6, 2, 6, 8, (1, 1, 1))
    eng.close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    o, a, b, pr, ow = (np.array(t, dtype=np.int32) for t in (O_ROW, A_ROW, B_ROW, P_ROW, OWNER))
    start, dims = np.array(START, dtype=np.int64), np.array(DIMS)
    create = lambda *args: lib.mdx_sdf_create(ctypes.byref(h), 0, *args)      # noqa: E731
    good = (6, 2, p(o), p(a), p(b), 2, p(start), p(pr), p(ow), 0, 3.0, p(dims))
    assert create(*good) == 0
    assert lib.mdx_sdf_destroy(h) == 0
    for at in (2, 3, 4, 6, 7, 8, 11):
        args = list(good)
        args[at] = None
        assert create(*args) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_create(None, 0, *good) == -1 and b"NULL" in lib.mdx_last_error()
    assert create(6, 0, p(o), p(a), p(b), 2, p(start), p(pr), p(ow), 0, 3.0, p(dims)) == -1
    assert b"n_ref" in lib.mdx_last_error()
    assert create(6, 2, p(o), p(a), p(b), 0, p(start), p(pr), p(ow), 0, 3.0, p(dims)) == -1
    assert b"n_groups" in lib.mdx_last_error()
    assert create(6, 2, p(o), p(a), p(b), 2, p(start), p(pr), p(ow), 0, 5.25, p(dims)) == -1
    assert b"cutoff 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(0, 2, p(o), p(a), p(b), 2, p(start), p(pr), p(ow), 0, 3.0, p(dims)) == -1
    assert b"2^31 / 3" in lib.mdx_last_error()
    for call in (lib.mdx_sdf_reset, lib.mdx_sdf_synchronize):
        assert call(None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_set_bins(None, 1, None, 1, None, 1, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_result(None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_inside(None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_sdf_destroy(None) == 0
    E = _core.SpatialDistributionEngine
    assert (E.TILE, E.JCHUNK, E.MAX_GROUPS, E.MAX_AXIS_BINS, E._prefix) == (256, 1024, 8, 512, "mdx_sdf")


def test_set_bins_errors_need_no_device():
    eng = _engine()
    lib = _lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    up = np.array([-2.0, -1.0, 0.5, 2.0])
    try:
        for at, name in enumerate(("ex", "ey", "ez")):
            for bad, word in (([-2.0, 1.0, 1.0, 2.0], f"{name} must be strictly increasing: \\[1\\] = 1, \\[2\\] = 1"),
                              ([-2.0, 1.0, 0.0, 2.0], f"{name} must be strictly increasing"),
                              (up[::-1], f"{name} must be strictly increasing"),
                              ([-2.0, np.nan, 2.0], f"{name}\\[1\\] must be finite"),
                              ([-np.inf, 0.0, 2.0], f"{name}\\[0\\] must be finite"),
                              ([-2.0, 0.0, np.inf], f"{name}\\[2\\] must be finite"),
                              (np.linspace(-1.0, 1.0, 514), f"n{name[1]} must lie in \\[1, 512\\]"),
                              ([1.0], "at least two"),
                              ([[-1.0, 1.0]], "at least two")):
                edges = [up, up, up]
                edges[at] = bad
                with pytest.raises(ValueError, match=word):
                    eng.set_bins(*edges)
        assert eng.n_bins == (1, 1, 1)                              # a refused table changes nothing
        for at in (2, 4, 6):
            args = [eng.handle, 3, p(up), 3, p(up), 3, p(up)]
            args[at] = None
            assert lib.mdx_sdf_set_bins(*args) == -1 and b"NULL" in lib.mdx_last_error()
        assert lib.mdx_sdf_set_bins(eng.handle, 0, p(up), 3, p(up), 3, p(up)) == -1 and b"nx" in lib.mdx_last_error()
        # the size cap: 2 groups x 512 x 512 x 128 = 2^26 is allowed, one bin more is not
        wide = np.linspace(-2.0, 2.0, 513)
        with pytest.raises(ValueError, match="2 groups of nx \\* ny \\* nz = 512 x 512 x 129 bins are more than"):
            eng.set_bins(wide, wide, np.linspace(-2.0, 2.0, 130))
        eng.set_bins(wide, wide, np.linspace(-2.0, 2.0, 129))
        assert eng.n_bins == (512, 512, 128)
        eng.set_bins(up, up[:2], up[:3])                            # more than once, before the first frame
        assert eng.n_bins == (3, 1, 2)
    finally:
        eng.close()


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    for eng in (_engine(), _engine(mode=1, owner=[-1] * 6)):
        try:
            with pytest.raises(ValueError, match="5 rows given, the tables hold 6"):
                eng.accumulate(np.zeros((2, 5, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="7 rows given, the tables hold 6"):
                eng.accumulate_device(rows, 7, 2)
            with pytest.raises(ValueError, match="4 rows given, the tables hold 6"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
            with pytest.raises(ValueError, match="index 7 out of range"):
                eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 4, 7])
            for frames in (-1, 32769):
                with pytest.raises(ValueError, match="frames must lie in"):
                    eng.set_slab_frames(frames)
            out = np.zeros(3, dtype=np.int64)
            assert _lib.lib().mdx_sdf_inside(eng.handle, out.ctypes.data_as(ctypes.c_void_p), 3) == -1
            assert b"3 frames asked for, 0 seen" in _lib.lib().mdx_last_error()
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            assert eng.plan() == {"slab_frames": 8, "ring_frames": 0}
            eng.reset()
            eng.synchronize()
            eng.set_slab_frames(0)
            assert eng.plan() == {"slab_frames": 32768, "ring_frames": 0}      # 256 MB of frames of 6 rows
            eng.reset()
            assert len(eng.inside()) == 0
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "degenerate": 0}
        finally:
            eng.close()
