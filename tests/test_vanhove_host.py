"""
Host-side checks of the van Hove analysis that need no GPU: ``calculate_non_gaussian_parameter`` against closed
forms, the argument handling of ``analysis.dynamics.VanHove`` and the argument errors of the engine, which are raised
before any device is touched (a handle touches its device with the first frame).

Not reachable without a device, and therefore checked in ``test_gpu_vanhove.py``: ``set_unwrap`` /
``set_slab_frames`` after the first frame (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import VanHove, calculate_non_gaussian_parameter, dynamics


# ---------------------------------------------------------------- the function

def test_non_gaussian_parameter_closed_forms():
    for s in (0.3, 1.0, 7.5):
        # a Gaussian of width s per component: <r2> = d s^2, <r4> = d (d + 2) s^4
        assert abs(calculate_non_gaussian_parameter(3 * s ** 2, 15 * s ** 4)) <= 1e-15
        assert abs(calculate_non_gaussian_parameter(2 * s ** 2, 8 * s ** 4, n_dims=2)) <= 1e-15
        # every point the same |dr|: <r4> = <r2>^2
        assert calculate_non_gaussian_parameter(s ** 2, s ** 4) == pytest.approx(-2 / 5, abs=1e-15)
    assert isinstance(calculate_non_gaussian_parameter(3.0, 15.0), float)
    assert mdhelper_amd.analysis.calculate_non_gaussian_parameter is dynamics.calculate_non_gaussian_parameter


def test_non_gaussian_parameter_without_displacement_is_nan_without_a_warning():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isnan(calculate_non_gaussian_parameter(0.0, 0.0))
        out = calculate_non_gaussian_parameter([[0.0, 3.0], [2.0, np.nan]], [[0.0, 15.0], [4.0, np.nan]])
    assert out.shape == (2, 2)
    assert np.isnan(out[0, 0]) and np.isnan(out[1, 1])
    assert abs(out[0, 1]) <= 1e-15 and out[1, 0] == pytest.approx(-2 / 5, abs=1e-15)


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=12, dims=(10.0, 12.0, 14.0), dt=0.5):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, 90.0, 90.0, 90.0]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


def test_constructor_errors():
    u = _universe()
    with pytest.raises(ValueError, match="'range' must be an increasing pair"):
        VanHove(u.atoms, range=(5.0, 5.0))
    with pytest.raises(ValueError, match="'range' must be an increasing pair"):
        VanHove(u.atoms, range=(5.0, 1.0))
    with pytest.raises(ValueError, match="'n_bins' must be at least 1"):
        VanHove(u.atoms, n_bins=0)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        VanHove(u.atoms, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        VanHove(u.atoms, lags=[0, 1, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        VanHove(u.atoms, lags=[-1, 0])
    with pytest.raises(ValueError, match="array of integers"):
        VanHove(u.atoms, lags=[0.5, 1.0])
    with pytest.raises(ValueError, match="cannot both be given"):
        VanHove(u.atoms, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="unwrap=True needs the box lengths"):
        VanHove(_universe(dims=None).atoms, unwrap=True)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        VanHove(u.atoms, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        VanHove(u.atoms, drop_axis=3)
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            VanHove(u.atoms, comm=TwoRanks(rank))
    VanHove(_universe(dims=None).atoms)                                          # no box needed without unwrap
    v = VanHove(_universe(dims=None).atoms, dimensions=[10.0, 11.0, 12.0], unwrap=True, drop_axis="z")
    np.testing.assert_array_equal(v._dimensions, [10.0, 11.0, 12.0])
    assert v._drop_axis == 2
    two = VanHove([u.select(np.arange(4)), u.select(np.arange(4, 12))], n_lags=3)
    np.testing.assert_array_equal(two._lags, [0, 1, 2])
    np.testing.assert_array_equal(two._Ns, [4, 8])


def _run_until_the_device(v, **kwargs):
    """``run()`` up to the point where the device is asked for: everything ``_prepare`` derives from the arguments
    is in place by then."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            v.run(**kwargs)
    else:
        v.run(**kwargs)
    return v


def test_prepare_errors_and_times():
    u = _universe()
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        VanHove(u.atoms, verbose=False).run(frames=[0, 1, 3])
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        VanHove(u.atoms, verbose=False).run(frames=[4, 2, 0])
    v = _run_until_the_device(VanHove(u.atoms, n_bins=4, range=(1.0, 3.0), lags=[0, 1, 2, 5], verbose=False), step=3)
    assert v.n_frames == 3
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    np.testing.assert_array_equal(v.results.edges, np.linspace(1.0, 3.0, 5))
    np.testing.assert_array_equal(v.results.bins, [1.25, 1.75, 2.25, 2.75])
    assert v.results.units["results.times"] == "picosecond" and v.results.units["results.vanhove"] == "angstrom^-3"
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument
    v = _run_until_the_device(VanHove(u.atoms, dt=2.0, drop_axis="x", verbose=False), frames=[1, 3, 5])
    np.testing.assert_array_equal(v.results.times, np.arange(3) * 2 * 2.0)
    assert v.results.units["results.vanhove"] == "angstrom^-2"


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            VanHove(_universe().atoms, verbose=False).run()
        eng = _core.VanHoveEngine([12], np.linspace(0.0, 1.0, 3), [0, 1])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- the engine's argument errors

EDGES = np.linspace(0.0, 2.0, 5)


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
                         (dict(zero_dims=7), "at least one component"),
                         (dict(zero_dims=8), "at least one component"),
                         (dict(zero_dims=-1), "at least one component"),
                         (dict(n_points=[3, -1]), "not negative"),
                         (dict(n_points=[0, 0]), "hold no point"),
                         (dict(n_points=[]), "one entry per group"),
                         (dict(n_points=[2 ** 31 // 3]), "2\\^31 / 3")):
        args = dict(n_points=[2, 3], edges=EDGES, lags=[0, 1, 4])
        zero_dims = kwargs.pop("zero_dims", 0)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.VanHoveEngine(args["n_points"], args["edges"], args["lags"], zero_dims=zero_dims)
    # n_bins < 1 at the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    one, lag0 = np.array([2], dtype=np.int64), np.array([0], dtype=np.int64)
    assert lib.mdx_vh_create(ctypes.byref(h), 0, 1, p(one), 0, p(EDGES), 1, p(lag0), 0) == -1
    assert b"n_bins" in lib.mdx_last_error()
    assert lib.mdx_vh_create(ctypes.byref(h), 0, 1, p(one), 4, p(EDGES), 0, p(lag0), 0) == -1
    assert b"at least one lag" in lib.mdx_last_error()
    assert lib.mdx_vh_create(ctypes.byref(h), 0, 1, None, 4, p(EDGES), 1, p(lag0), 0) == -1
    assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_vh_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert _core.VanHoveEngine.TILE == 64


def test_engine_call_errors_need_no_device():
    eng = _core.VanHoveEngine([2, 0, 3], EDGES, [0, 1, 4], zero_dims=2)          # an empty group is allowed
    try:
        assert (eng.n_groups, eng.n_points, eng.n_bins, eng.n_lags) == (3, 5, 4, 3)
        with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
            eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
        rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
        with pytest.raises(ValueError, match="7 rows given, the groups hold 5"):
            eng.accumulate_device(rows, 7, 2)
        with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
        with pytest.raises(ValueError, match="index 7 out of range"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 7])
        with pytest.raises(ValueError, match="index -1 out of range"):
            eng.accumulate_device(rows, 7, 2, [0, 1, -1, 3, 4])
        for dims in ([10.0, 0.0, 10.0], [10.0, 10.0, -1.0], [np.inf, 10.0, 10.0], [10.0, np.nan, 10.0]):
            with pytest.raises(ValueError, match="must be positive and finite"):
                eng.set_unwrap(dims)
        with pytest.raises(ValueError, match="three box lengths"):
            eng.set_unwrap([10.0, 10.0])
        for frames in (-1, 32769):
            with pytest.raises(ValueError, match="frames must lie in"):
                eng.set_slab_frames(frames)
        # what is allowed before the first frame, in any order and more than once
        eng.set_unwrap([10.0, 11.0, 12.0])
        eng.set_slab_frames(8)
        eng.set_unwrap(None)
        eng.set_slab_frames(0)
        eng.reset()
        eng.synchronize()
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0}
    finally:
        eng.close()
