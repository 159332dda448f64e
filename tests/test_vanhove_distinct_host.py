"""
Host-side checks of the distinct van Hove analysis that need no GPU: the argument handling of
``analysis.dynamics.DistinctVanHove`` and the argument errors of the engine, which are raised before any device is
touched (a handle touches its device with the first frame).

Not reachable without a device, and therefore checked in ``test_gpu_vanhove_distinct.py``: ``set_slab_frames`` after
the first frame (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import DistinctVanHove, dynamics


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=12, dims=(40.0, 42.0, 44.0), dt=0.5, angles=(90.0, 90.0, 90.0)):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (40.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


def test_constructor_errors():
    u = _universe()
    assert mdhelper_amd.analysis.DistinctVanHove is dynamics.DistinctVanHove
    with pytest.raises(ValueError, match="'range' must be an increasing pair"):
        DistinctVanHove(u.atoms, range=(5.0, 5.0))
    with pytest.raises(ValueError, match="'range' must be an increasing pair"):
        DistinctVanHove(u.atoms, range=(5.0, 1.0))
    with pytest.raises(ValueError, match="'n_bins' must be at least 1"):
        DistinctVanHove(u.atoms, n_bins=0)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        DistinctVanHove(u.atoms, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        DistinctVanHove(u.atoms, lags=[-1, 0])
    with pytest.raises(ValueError, match="array of integers"):
        DistinctVanHove(u.atoms, lags=[0.5, 1.0])
    with pytest.raises(ValueError, match="cannot both be given"):
        DistinctVanHove(u.atoms, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="'origin_step' must be at least 1"):
        DistinctVanHove(u.atoms, origin_step=0)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        DistinctVanHove(u.atoms, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        DistinctVanHove(u.atoms, drop_axis=3)
    # the box: none at all, not orthorhombic, too small for the range
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        DistinctVanHove(_universe(dims=None).atoms)
    with pytest.raises(ValueError, match="orthorhombic"):
        DistinctVanHove(_universe(angles=(90.0, 90.0, 60.0)).atoms)
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        DistinctVanHove(u.atoms, range=(0.0, 20.5))                              # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        DistinctVanHove(u.atoms, dimensions=[29.0, 60.0, 60.0])                  # the default range reaches 15
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        DistinctVanHove(u.atoms, range=(0.0, 21.5), drop_axis="z")               # x is still 40
    with pytest.raises(ValueError, match="positive and finite"):
        DistinctVanHove(u.atoms, dimensions=[40.0, np.nan, 40.0])
    DistinctVanHove(u.atoms, range=(0.0, 20.0))                                  # exactly half is allowed
    DistinctVanHove(u.atoms, range=(0.0, 21.0), drop_axis="x")                   # x dropped: 42 / 2 = 21
    DistinctVanHove(_universe(dims=None).atoms, dimensions=[30.0, 31.0, 32.0])   # the box from the argument
    # the two groups
    a, b = u.select(np.arange(5)), u.select(np.arange(5, 12))
    with pytest.raises(ValueError, match="share some atoms"):
        DistinctVanHove(a, u.select(np.arange(4, 12)))
    with pytest.raises(ValueError, match="share some atoms"):
        DistinctVanHove(a, u.select(np.arange(3)))
    with pytest.raises(ValueError, match="share some atoms"):
        DistinctVanHove(a, u.select(np.arange(5)[::-1]))                         # the same atoms in another order
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            DistinctVanHove(a, b, comm=TwoRanks(rank))
    two = DistinctVanHove(b, a, n_lags=3, origin_step=2, drop_axis="z")
    np.testing.assert_array_equal(two._lags, [0, 1, 2])
    np.testing.assert_array_equal(two._index, [5, 6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4])
    assert (two._N1, two._N2, two._same, two._drop_axis, two._origin_step) == (7, 5, False, 2, 2)
    one = DistinctVanHove(a)
    twin = DistinctVanHove(a, u.select(np.arange(5)))
    for v in (one, twin):
        assert (v._N1, v._N2, v._same) == (5, 5, True)
        np.testing.assert_array_equal(v._index, np.arange(5))
        np.testing.assert_array_equal(v._dimensions, [40.0, 42.0, 44.0])


def _run_until_the_device(v, **kwargs):
    """``run()`` up to the point where the device is asked for: everything ``_prepare`` derives from the arguments
    is in place by then."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            v.run(**kwargs)
    else:
        v.run(**kwargs)
    return v


def test_prepare_errors_times_and_origins():
    u = _universe()
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        DistinctVanHove(u.atoms, verbose=False).run(frames=[0, 1, 3])
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        DistinctVanHove(u.atoms, verbose=False).run(frames=[4, 2, 0])
    v = _run_until_the_device(DistinctVanHove(u.atoms, n_bins=4, range=(1.0, 3.0), lags=[0, 1, 2, 5], verbose=False),
                              step=3)
    assert v.n_frames == 3
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [3, 2, 1, 0])
    np.testing.assert_array_equal(v.results.edges, np.linspace(1.0, 3.0, 5))
    np.testing.assert_array_equal(v.results.bins, [1.25, 1.75, 2.25, 2.75])
    assert v.results.units == {"results.bins": "angstrom", "results.edges": "angstrom",
                               "results.times": "picosecond", "results.vanhove": "angstrom^-3"}
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument; every second frame an origin
    v = _run_until_the_device(DistinctVanHove(u.atoms, dt=2.0, drop_axis="x", origin_step=2, verbose=False))
    np.testing.assert_array_equal(v.results.times, np.arange(7) * 2.0)
    np.testing.assert_array_equal(v.results.n_origins, [4, 3, 3, 2, 2, 1, 1])     # origins 0, 2, 4, 6 below 7 - lag
    assert v.results.units["results.vanhove"] == "angstrom^-2"
    v = _run_until_the_device(DistinctVanHove(u.atoms, lags=[0, 1, 4, 9], origin_step=3, verbose=False),
                              frames=[0, 2, 4, 6])
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 4, 9]) * 2 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [2, 1, 0, 0])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            DistinctVanHove(_universe().atoms, verbose=False).run()
        eng = _core.DistinctVanHoveEngine(12, 12, np.linspace(0.0, 1.0, 3), [0, 1], [10.0, 10.0, 10.0], same=True)
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- the engine's argument errors

EDGES = np.linspace(0.0, 2.0, 5)
DIMS = [10.0, 11.0, 12.0]


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(edges=[0.0, 1.0, 1.0]), "strictly increasing"),
                         (dict(edges=[0.0, 2.0, 1.0]), "strictly increasing"),
                         (dict(edges=[0.0, np.inf]), "finite"),
                         (dict(edges=[np.nan, 1.0]), "finite"),
                         (dict(edges=[1.0]), "n_bins"),
                         (dict(edges=[]), "n_bins"),
                         (dict(lags=[]), "at least one lag"),
                         (dict(lags=[-1, 0]), "not be negative"),
                         (dict(lags=[0, 2, 2]), "strictly increasing"),
                         (dict(lags=[3, 1]), "strictly increasing"),
                         (dict(origin_step=0), "origin_step must be at least 1"),
                         (dict(origin_step=-2), "origin_step must be at least 1"),
                         (dict(zero_dims=7), "at least one component"),
                         (dict(zero_dims=8), "at least one component"),
                         (dict(zero_dims=-1), "at least one component"),
                         (dict(n1=0), "at least one point"),
                         (dict(n2=0), "at least one point"),
                         (dict(n1=-3), "at least one point"),
                         (dict(n1=3, n2=4, same=True), "n1 = 3 and n2 = 4"),
                         (dict(n1=2 ** 31 // 3), "2\\^31 / 3"),
                         (dict(dims=[10.0, 0.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0, -1.0]), "must be positive and finite"),
                         (dict(dims=[np.inf, 10.0, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, np.nan, 10.0]), "must be positive and finite"),
                         (dict(dims=[10.0, 10.0]), "three box lengths"),
                         (dict(dims=[3.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 11.0, 3.9], zero_dims=3), "beyond half the shortest box length"),
                         (dict(edges=np.linspace(0.0, 5.5, 5), zero_dims=2), "beyond half the shortest box length")):
        args = dict(n1=2, n2=3, edges=EDGES, lags=[0, 1, 4], dims=DIMS, same=False, origin_step=1, zero_dims=0)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.DistinctVanHoveEngine(args["n1"], args["n2"], args["edges"], args["lags"], args["dims"],
                                        same=args["same"], origin_step=args["origin_step"],
                                        zero_dims=args["zero_dims"])
    # half the shortest kept length itself is allowed, and a dropped component does not count
    _core.DistinctVanHoveEngine(2, 3, EDGES, [0], [4.0, 11.0, 12.0]).close()
    _core.DistinctVanHoveEngine(2, 3, EDGES, [0], [1.0, 11.0, 12.0], zero_dims=1).close()
    _core.DistinctVanHoveEngine(2, 3, np.linspace(0.0, 5.5, 5), [0], DIMS, zero_dims=1).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    lag0, dims = np.array([0], dtype=np.int64), np.array(DIMS)
    create = lambda *a: lib.mdx_vhd_create(ctypes.byref(h), 0, *a)      # noqa: E731
    assert create(2, 3, 0, 0, p(EDGES), 1, p(lag0), 1, p(dims), 0) == -1
    assert b"n_bins" in lib.mdx_last_error()
    assert create(2, 3, 0, 4, p(EDGES), 0, p(lag0), 1, p(dims), 0) == -1
    assert b"at least one lag" in lib.mdx_last_error()
    for args in ((2, 3, 0, 4, None, 1, p(lag0), 1, p(dims), 0), (2, 3, 0, 4, p(EDGES), 1, None, 1, p(dims), 0),
                 (2, 3, 0, 4, p(EDGES), 1, p(lag0), 1, None, 0)):
        assert create(*args) == -1
        assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_vhd_create(None, 0, 2, 3, 0, 4, p(EDGES), 1, p(lag0), 1, p(dims), 0) == -1
    assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_vhd_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_vhd_result(None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert _core.DistinctVanHoveEngine.TILE == 256


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _core.DistinctVanHoveEngine(2, 3, EDGES, [0, 1, 4], DIMS, origin_step=2, zero_dims=2)
    one = _core.DistinctVanHoveEngine(5, 5, EDGES, [0, 1, 4], DIMS, same=True)
    try:
        assert (two.n_rows, two.n_bins, two.n_lags, two.same) == (5, 4, 3, False)
        assert (one.n_rows, one.n_bins, one.n_lags, one.same) == (5, 4, 3, True)      # the rows arrive once
        for eng in (two, one):
            with pytest.raises(ValueError, match="4 rows given, the sets hold 5"):
                eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="10 rows given, the sets hold 5"):
                eng.accumulate(np.zeros((2, 10, 3), dtype=np.float32))
            with pytest.raises(ValueError, match="7 rows given, the sets hold 5"):
                eng.accumulate_device(rows, 7, 2)
            with pytest.raises(ValueError, match="4 rows given, the sets hold 5"):
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
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0}
        assert not hasattr(two, "set_unwrap") and not hasattr(two, "point_moments")
    finally:
        two.close()
        one.close()
