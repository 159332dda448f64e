"""
Host-side checks of the pair residence analysis that need no GPU: the argument handling of
``analysis.dynamics.PairResidence``, ``calculate_residence_time``, and the argument errors of the engine, which are
raised before any device is touched (a handle touches its device with the first frame).

Not reachable without a device, and therefore checked in ``test_gpu_residence.py``: ``set_slab_frames`` after the
first frame and a row beyond ``max_neighbors`` (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import PairResidence, calculate_residence_time, dynamics


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
    assert mdhelper_amd.analysis.PairResidence is dynamics.PairResidence
    assert mdhelper_amd.analysis.calculate_residence_time is dynamics.calculate_residence_time
    with pytest.raises(ValueError, match="'cutoff' must be given"):
        PairResidence(u.atoms)
    for cutoff in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="'cutoff' must be positive and finite"):
            PairResidence(u.atoms, cutoff=cutoff)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        PairResidence(u.atoms, cutoff=5.0, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        PairResidence(u.atoms, cutoff=5.0, lags=[-1, 0])
    with pytest.raises(ValueError, match="array of integers"):
        PairResidence(u.atoms, cutoff=5.0, lags=[0.5, 1.0])
    with pytest.raises(ValueError, match="cannot both be given"):
        PairResidence(u.atoms, cutoff=5.0, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="'n_lags' must be at least 1"):
        PairResidence(u.atoms, cutoff=5.0, n_lags=0)
    with pytest.raises(ValueError, match="'origin_step' must be at least 1"):
        PairResidence(u.atoms, cutoff=5.0, origin_step=0)
    for slots in (0, 65, -3):
        with pytest.raises(ValueError, match="'max_neighbors' must lie in \\[1, 64\\]"):
            PairResidence(u.atoms, cutoff=5.0, max_neighbors=slots)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        PairResidence(u.atoms, cutoff=5.0, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        PairResidence(u.atoms, cutoff=5.0, drop_axis=3)
    # the box: none at all, not orthorhombic, too small for the cutoff
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        PairResidence(_universe(dims=None).atoms, cutoff=5.0)
    with pytest.raises(ValueError, match="orthorhombic"):
        PairResidence(_universe(angles=(90.0, 90.0, 60.0)).atoms, cutoff=5.0)
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        PairResidence(u.atoms, cutoff=20.5)                                      # 40 / 2 = 20
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        PairResidence(u.atoms, cutoff=15.0, dimensions=[29.0, 60.0, 60.0])
    with pytest.raises(ValueError, match="beyond half the shortest box length"):
        PairResidence(u.atoms, cutoff=21.5, drop_axis="z")                       # x is still 40
    with pytest.raises(ValueError, match="positive and finite"):
        PairResidence(u.atoms, cutoff=5.0, dimensions=[40.0, np.nan, 40.0])
    PairResidence(u.atoms, cutoff=20.0)                                          # exactly half is allowed
    PairResidence(u.atoms, cutoff=21.0, drop_axis="x")                           # x dropped: 42 / 2 = 21
    PairResidence(_universe(dims=None).atoms, cutoff=5.0, dimensions=[30.0, 31.0, 32.0])
    PairResidence(u.atoms, cutoff=5.0, max_neighbors=1)
    PairResidence(u.atoms, cutoff=5.0, max_neighbors=64)
    # the two groups
    a, b = u.select(np.arange(5)), u.select(np.arange(5, 12))
    with pytest.raises(ValueError, match="share some atoms"):
        PairResidence(a, u.select(np.arange(4, 12)), 5.0)
    with pytest.raises(ValueError, match="share some atoms"):
        PairResidence(a, u.select(np.arange(3)), 5.0)
    with pytest.raises(ValueError, match="share some atoms"):
        PairResidence(a, u.select(np.arange(5)[::-1]), 5.0)                      # the same atoms in another order
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            PairResidence(a, b, 5.0, comm=TwoRanks(rank))
    two = PairResidence(b, a, 4.5, n_lags=3, origin_step=2, drop_axis="z", max_neighbors=8, continuous=False)
    np.testing.assert_array_equal(two._lags, [0, 1, 2])
    np.testing.assert_array_equal(two._index, [5, 6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4])
    assert (two._N1, two._N2, two._same, two._drop_axis, two._origin_step) == (7, 5, False, 2, 2)
    assert (two._cutoff, two._max_neighbors, two._continuous) == (4.5, 8, False)
    one = PairResidence(a, cutoff=5.0)
    twin = PairResidence(a, u.select(np.arange(5)), 5.0)
    for v in (one, twin):
        assert (v._N1, v._N2, v._same, v._max_neighbors, v._continuous) == (5, 5, True, 32, True)
        np.testing.assert_array_equal(v._index, np.arange(5))
        np.testing.assert_array_equal(v._dimensions, [40.0, 42.0, 44.0])
    with pytest.raises(RuntimeError, match="run\\(\\)"):
        one.calculate_residence_times()


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
        PairResidence(u.atoms, cutoff=5.0, verbose=False).run(frames=[0, 1, 3])
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        PairResidence(u.atoms, cutoff=5.0, verbose=False).run(frames=[4, 2, 0])
    v = _run_until_the_device(PairResidence(u.atoms, cutoff=5.0, lags=[0, 1, 2, 5], verbose=False), step=3)
    assert v.n_frames == 3
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [3, 2, 1, 0])
    assert v.results.units == {"results.times": "picosecond", "results.residence_time": "picosecond",
                               "results.relaxation_time": "picosecond"}
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument; every second frame an origin
    v = _run_until_the_device(PairResidence(u.atoms, cutoff=5.0, dt=2.0, drop_axis="x", origin_step=2, verbose=False))
    np.testing.assert_array_equal(v.results.times, np.arange(7) * 2.0)
    np.testing.assert_array_equal(v.results.n_origins, [4, 3, 3, 2, 2, 1, 1])     # origins 0, 2, 4, 6 below 7 - lag
    v = _run_until_the_device(PairResidence(u.atoms, cutoff=5.0, lags=[0, 1, 4, 9], origin_step=3, verbose=False),
                              frames=[0, 2, 4, 6])
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 4, 9]) * 2 * 0.5)
    np.testing.assert_array_equal(v.results.n_origins, [2, 1, 0, 0])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            PairResidence(_universe().atoms, cutoff=5.0, verbose=False).run()
        eng = _core.PairResidenceEngine(12, 12, 2.0, [0, 1], [10.0, 10.0, 10.0], same=True)
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- calculate_residence_time

def test_residence_time_is_the_trapezoid_integral_of_the_finite_leading_part():
    tau = 3.0
    t = np.arange(9) * 0.5
    s = np.exp(-t / tau)
    # equal steps: the trapezoid formula in closed form, h * (sum - (first + last) / 2)
    closed = 0.5 * (s.sum() - (s[0] + s[-1]) / 2)
    assert calculate_residence_time(t, s) == pytest.approx(closed, rel=1e-15)
    assert calculate_residence_time(t, s) == float(((s[1:] + s[:-1]) * np.diff(t)).sum() / 2)
    assert calculate_residence_time(t, s) < tau                 # truncated at the last lag
    # uneven lags
    tu = np.array([0.0, 0.5, 1.0, 2.5, 4.0, 8.0])
    su = np.exp(-tu / tau)
    assert calculate_residence_time(tu, su) == float(((su[1:] + su[:-1]) * np.diff(tu)).sum() / 2)
    # a NaN tail (lags without an origin) is left out; so is everything after the first NaN
    tail = s.copy()
    tail[6:] = np.nan
    assert calculate_residence_time(t, tail) == calculate_residence_time(t[:6], s[:6])
    hole = s.copy()
    hole[4] = np.inf
    assert calculate_residence_time(t, hole) == calculate_residence_time(t[:4], s[:4])
    assert calculate_residence_time(t[:1], s[:1]) == 0.0        # one value: nothing to integrate
    assert np.isnan(calculate_residence_time(t, np.full(9, np.nan)))
    assert np.isnan(calculate_residence_time([], []))
    assert isinstance(calculate_residence_time(list(t), list(s)), float)
    with pytest.raises(ValueError, match="one length"):
        calculate_residence_time(t, s[:-1])
    with pytest.raises(ValueError, match="one-dimensional"):
        calculate_residence_time(t.reshape(3, 3), s.reshape(3, 3))
    assert "truncated at the last lag" in " ".join(calculate_residence_time.__doc__.split())


# ---------------------------------------------------------------- the engine's argument errors

DIMS = [10.0, 11.0, 12.0]


def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(cutoff=0.0), "cutoff must be positive and finite"),
                         (dict(cutoff=-2.0), "cutoff must be positive and finite"),
                         (dict(cutoff=np.nan), "cutoff must be positive and finite"),
                         (dict(cutoff=np.inf), "cutoff must be positive and finite"),
                         (dict(cutoff=5.5), "beyond half the shortest box length"),
                         (dict(dims=[3.9, 11.0, 12.0]), "beyond half the shortest box length"),
                         (dict(dims=[10.0, 11.0, 3.9], zero_dims=3), "beyond half the shortest box length"),
                         (dict(cutoff=5.5, zero_dims=2), "beyond half the shortest box length"),
                         (dict(max_neighbors=0), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(max_neighbors=65), "max_neighbors must lie in \\[1, 64\\]"),
                         (dict(max_neighbors=-1), "max_neighbors must lie in \\[1, 64\\]"),
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
                         (dict(dims=[10.0, 10.0]), "three box lengths")):
        args = dict(n1=2, n2=3, cutoff=2.0, lags=[0, 1, 4], dims=DIMS, same=False, origin_step=1, zero_dims=0,
                    max_neighbors=32)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.PairResidenceEngine(args["n1"], args["n2"], args["cutoff"], args["lags"], args["dims"],
                                      same=args["same"], origin_step=args["origin_step"], zero_dims=args["zero_dims"],
                                      max_neighbors=args["max_neighbors"])
    # half the shortest kept length itself is allowed, and a dropped component does not count
    _core.PairResidenceEngine(2, 3, 2.0, [0], [4.0, 11.0, 12.0]).close()
    _core.PairResidenceEngine(2, 3, 2.0, [0], [1.0, 11.0, 12.0], zero_dims=1).close()
    _core.PairResidenceEngine(2, 3, 5.5, [0], DIMS, zero_dims=1).close()
    _core.PairResidenceEngine(2, 3, 2.0, [0], DIMS, max_neighbors=1).close()
    _core.PairResidenceEngine(2, 3, 2.0, [0], DIMS, max_neighbors=64, continuous=False).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    lag0, dims = np.array([0], dtype=np.int64), np.array(DIMS)
    create = lambda *a: lib.mdx_prs_create(ctypes.byref(h), 0, *a)      # noqa: E731
    assert create(2, 3, 0, 2.0, 0, p(lag0), 1, p(dims), 0, 32, 1) == -1
    assert b"at least one lag" in lib.mdx_last_error()
    assert create(2, 3, 0, 5.25, 1, p(lag0), 1, p(dims), 0, 32, 1) == -1
    assert b"cutoff 5.25" in lib.mdx_last_error() and b"half the shortest box length 10" in lib.mdx_last_error()
    assert create(2, 3, 0, 2.0, 1, p(lag0), 1, p(dims), 0, 65, 1) == -1
    assert b"max_neighbors" in lib.mdx_last_error()
    for args in ((2, 3, 0, 2.0, 1, None, 1, p(dims), 0, 32, 1), (2, 3, 0, 2.0, 1, p(lag0), 1, None, 0, 32, 1)):
        assert create(*args) == -1
        assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_prs_create(None, 0, 2, 3, 0, 2.0, 1, p(lag0), 1, p(dims), 0, 32, 1) == -1
    assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_prs_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_prs_result(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_prs_contacts(None, None, 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert (_core.PairResidenceEngine.TILE, _core.PairResidenceEngine.MAX_NEIGHBORS) == (256, 64)


def test_engine_call_errors_need_no_device():
    rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
    two = _core.PairResidenceEngine(2, 3, 2.0, [0, 1, 4], DIMS, origin_step=2, zero_dims=2)
    one = _core.PairResidenceEngine(5, 5, 2.0, [0, 1, 4], DIMS, same=True, max_neighbors=4, continuous=False)
    try:
        assert (two.n_rows, two.n_lags, two.same, two.max_neighbors, two.continuous) == (5, 3, False, 32, True)
        assert (one.n_rows, one.n_lags, one.same, one.max_neighbors, one.continuous) == (5, 3, True, 4, False)
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
            out = np.zeros(3, dtype=np.int64)
            assert _lib.lib().mdx_prs_contacts(eng.handle, out.ctypes.data_as(ctypes.c_void_p), 3) == -1
            assert b"3 frames asked for, 0 seen" in _lib.lib().mdx_last_error()
            # what is allowed before the first frame, in any order and more than once
            eng.set_slab_frames(8)
            eng.set_slab_frames(0)
            eng.reset()
            eng.synchronize()
            assert len(eng.contacts()) == 0
            assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "max_row": 0}
    finally:
        two.close()
        one.close()
