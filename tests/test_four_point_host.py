"""
Host-side checks of the four-point analysis that need no GPU: ``calculate_four_point_susceptibility`` against closed
forms and on sums where only exact integer arithmetic gives the answer, ``calculate_relaxation_times`` on hand-made
arrays, the argument handling of ``analysis.dynamics.FourPointSusceptibility``, the argument errors of the engine —
raised before any device is touched (a handle touches its device with the first frame) — and the overflow refusal of
the accumulate calls.

Not reachable without a device, and therefore checked in ``test_gpu_four_point.py``: ``set_unwrap`` /
``set_slab_frames`` / ``set_segment_points`` after the first frame (there is no first frame without a device).
"""
import ctypes
import warnings

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import FourPointSusceptibility, calculate_four_point_susceptibility, dynamics


# ---------------------------------------------------------------- the function

def test_four_point_susceptibility_closed_forms():
    for n in (1, 7, 1000):
        for origins in (1, 2, 10, 37):
            for q in (0, 1, n):                     # every Q equal: no fluctuation, exactly 0.0
                chi4 = calculate_four_point_susceptibility(origins * q, origins * q * q, origins, n)
                assert isinstance(chi4, float) and chi4 == 0.0
        for origins in (2, 10, 36):                 # Q alternating 0, n: q = 0, 1 with weight 1/2 each, variance 1/4
            assert calculate_four_point_susceptibility(origins // 2 * n, origins // 2 * n * n, origins, n) == n / 4
    # arrays [N_t, N_g, N_a] with n_origins [N_t] and n_points [N_g]
    sums = np.array([[[6, 12]], [[4, 0]]])                     # Q = 3, 3 | 6, 6 at lag 0;  Q = 0, 4 | 0, 0 at lag 1
    squares = np.array([[[18, 72]], [[16, 0]]])
    out = calculate_four_point_susceptibility(sums, squares, [2, 2], [6])
    assert out.shape == (2, 1, 2) and out.dtype == np.float64
    np.testing.assert_array_equal(out, [[[0.0, 0.0]], [[(2 * 16 - 16) / (4 * 6), 0.0]]])
    assert mdhelper_amd.analysis.calculate_four_point_susceptibility is dynamics.calculate_four_point_susceptibility
    with pytest.raises(ValueError, match="must hold integers"):
        calculate_four_point_susceptibility(np.array([1.0]), np.array([1]), 1, 1)


def test_four_point_susceptibility_takes_the_integer_path():
    """Four origins with Q = 10^9, 10^9, 10^9, 10^9 + 1 of N = 10^9 + 1 points: n S2 = 16 * 10^18 + 8 * 10^9 + 4 and
    S1^2 = 16 * 10^18 + 8 * 10^9 + 1 differ by 3, far below the spacing of float64 there (2048)."""
    big = 10 ** 9
    q = [big, big, big, big + 1]
    s1, s2 = sum(q), sum(x * x for x in q)
    assert s2 > 4 * 10 ** 18 and 4 * s2 - s1 * s1 == 3
    want = 3 / (16 * (big + 1))
    assert calculate_four_point_susceptibility(s1, s2, 4, big + 1) == want
    out = calculate_four_point_susceptibility(np.array([[[s1]]], dtype=np.int64), np.array([[[s2]]], dtype=np.int64),
                                              np.array([4]), np.array([big + 1]))
    np.testing.assert_array_equal(out, [[[want]]])
    # what float64 makes of the same difference: not the answer
    assert (4.0 * float(s2) - float(s1) * float(s1)) / (16.0 * (big + 1)) != want


def test_four_point_susceptibility_nan_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isnan(calculate_four_point_susceptibility(0, 0, 0, 5))                  # no origin
        assert np.isnan(calculate_four_point_susceptibility(0, 0, 3, 0))                  # an empty group
        out = calculate_four_point_susceptibility(np.array([[[4], [0]], [[0], [0]]]), np.array([[[16], [0]], [[0], [0]]]),
                                                  [2, 0], [4, 0])
    assert out.shape == (2, 2, 1)
    assert out[0, 0, 0] == (2 * 16 - 16) / (4 * 4)
    assert np.isnan(out[0, 1, 0]) and np.isnan(out[1]).all()


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


def test_relaxation_times_on_hand_made_arrays():
    u = _universe()
    with pytest.raises(RuntimeError, match="run\\(\\) before"):
        FourPointSusceptibility(u.atoms, 1.0).calculate_relaxation_times()
    level = np.exp(-1.0)
    v = FourPointSusceptibility([u.select(np.arange(4)), u.select(np.arange(4, 12))], [1.0, 2.0])
    v.results.times = np.array([0.0, 1.0, 2.0, 4.0])
    overlap = np.empty((4, 2, 2))
    chi4 = np.empty((4, 2, 2))
    overlap[:, 0, 0] = [1.0, 0.5, 0.25, 0.1]                # crosses 1/e between the times 1 and 2
    chi4[:, 0, 0] = [0.0, 0.3, 0.7, 0.2]
    overlap[:, 0, 1] = [1.0, 0.9, 0.8, 0.5]                 # never falls to 1/e: not bracketed
    chi4[:, 0, 1] = [0.0, 0.1, 0.2, 0.4]                    # still rising: the last lag
    overlap[:, 1, 0] = np.nan                               # an all-NaN column (an empty group)
    chi4[:, 1, 0] = np.nan
    overlap[:, 1, 1] = [1.0, np.nan, 0.2, 0.1]              # the lag before the crossing has no value
    chi4[:, 1, 1] = [0.0, np.nan, 0.6, 0.6]                 # two lags share the largest value: the first
    v.results.overlap, v.results.chi4 = overlap, chi4
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v.calculate_relaxation_times()
    tau, peak_time, peak_height = v.results.relaxation_time, v.results.peak_time, v.results.peak_height
    assert tau.shape == peak_time.shape == peak_height.shape == (2, 2)
    assert tau[0, 0] == 1.0 + (0.5 - level) / (0.5 - 0.25) * (2.0 - 1.0) and 1.0 < tau[0, 0] < 2.0
    assert np.isnan(tau[0, 1]) and np.isnan(tau[1, 0]) and np.isnan(tau[1, 1])
    np.testing.assert_array_equal(peak_time, [[2.0, 4.0], [np.nan, 2.0]])
    np.testing.assert_array_equal(peak_height, [[0.7, 0.4], [np.nan, 0.6]])
    # already below 1/e at the first lag (the lags need not start at 0): not bracketed; exactly 1/e: that lag
    v.results.overlap = np.array([0.3, 0.2, 0.1, 0.0]).reshape(4, 1, 1) * np.ones((1, 2, 2))
    v.calculate_relaxation_times()
    assert np.isnan(v.results.relaxation_time).all()
    v.results.overlap = np.array([1.0, 0.6, level, 0.0]).reshape(4, 1, 1) * np.ones((1, 2, 2))
    v.calculate_relaxation_times()
    np.testing.assert_array_equal(v.results.relaxation_time, np.full((2, 2), 2.0))


def test_constructor_errors():
    u = _universe()
    with pytest.raises(TypeError):
        FourPointSusceptibility(u.atoms)                    # cutoffs must be given
    for cutoffs in ([1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], -0.5, [1.0, np.inf], [np.nan]):
        with pytest.raises(ValueError, match="finite, non-negative and strictly increasing"):
            FourPointSusceptibility(u.atoms, cutoffs)
    for cutoffs in ([], np.arange(9.0), [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="1 to 8 cutoffs"):
            FourPointSusceptibility(u.atoms, cutoffs)
    with pytest.raises(ValueError, match="'origin_step' must be at least 1"):
        FourPointSusceptibility(u.atoms, 1.0, origin_step=0)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        FourPointSusceptibility(u.atoms, 1.0, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        FourPointSusceptibility(u.atoms, 1.0, lags=[-1, 0])
    with pytest.raises(ValueError, match="array of integers"):
        FourPointSusceptibility(u.atoms, 1.0, lags=[0.5, 1.0])
    with pytest.raises(ValueError, match="cannot both be given"):
        FourPointSusceptibility(u.atoms, 1.0, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="unwrap=True needs the box lengths"):
        FourPointSusceptibility(_universe(dims=None).atoms, 1.0, unwrap=True)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        FourPointSusceptibility(u.atoms, 1.0, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="drop_axis"):
        FourPointSusceptibility(u.atoms, 1.0, drop_axis=3)
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            FourPointSusceptibility(u.atoms, 1.0, comm=TwoRanks(rank))
    FourPointSusceptibility(_universe(dims=None).atoms, 0.0)                     # no box needed without unwrap
    v = FourPointSusceptibility(_universe(dims=None).atoms, 1.5, dimensions=[10.0, 11.0, 12.0], unwrap=True,
                                drop_axis="z", origin_step=3)
    np.testing.assert_array_equal(v._dimensions, [10.0, 11.0, 12.0])
    np.testing.assert_array_equal(v._cutoffs, [1.5])                             # a scalar is one cutoff
    assert v._drop_axis == 2 and v._origin_step == 3
    two = FourPointSusceptibility([u.select(np.arange(4)), u.select(np.arange(4, 12))], (0.0, 1.0, 2.5), n_lags=3)
    np.testing.assert_array_equal(two._lags, [0, 1, 2])
    np.testing.assert_array_equal(two._Ns, [4, 8])
    np.testing.assert_array_equal(two._cutoffs, [0.0, 1.0, 2.5])


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
        FourPointSusceptibility(u.atoms, 1.0, verbose=False).run(frames=[0, 1, 3])
    v = _run_until_the_device(FourPointSusceptibility(u.atoms, [1.0, 3.0], lags=[0, 1, 2, 5], verbose=False), step=3)
    assert v.n_frames == 3
    np.testing.assert_array_equal(v.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    np.testing.assert_array_equal(v.results.cutoffs, [1.0, 3.0])
    np.testing.assert_array_equal(v.results.n_origins, [3, 2, 1, 0])
    assert v.results.units["results.times"] == "picosecond" and v.results.units["results.cutoffs"] == "angstrom"
    # neither lags nor n_lags: every analysed frame is a lag; origins are the multiples of origin_step
    v = _run_until_the_device(FourPointSusceptibility(u.atoms, 1.0, dt=2.0, origin_step=2, verbose=False))
    np.testing.assert_array_equal(v.results.times, np.arange(7) * 2.0)
    np.testing.assert_array_equal(v.results.n_origins, [4, 3, 3, 2, 2, 1, 1])


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            FourPointSusceptibility(_universe().atoms, 1.0, verbose=False).run()
        eng = _core.FourPointEngine([12], [1.0], [0, 1])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 12, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()


# ---------------------------------------------------------------- the engine's argument errors

def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(cutoffs=[]), "1 to 8 cutoffs"),
                         (dict(cutoffs=np.arange(9.0)), "1 to 8 cutoffs"),
                         (dict(cutoffs=[1.0, 1.0]), "strictly increasing"),
                         (dict(cutoffs=[2.0, 1.0]), "strictly increasing"),
                         (dict(cutoffs=[-1.0, 1.0]), "finite and not negative"),
                         (dict(cutoffs=[1.0, np.inf]), "finite and not negative"),
                         (dict(cutoffs=[np.nan]), "finite and not negative"),
                         (dict(origin_step=0), "origin_step must be at least 1"),
                         (dict(origin_step=-2), "origin_step must be at least 1"),
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
        args = dict(n_points=[2, 3], cutoffs=[0.0, 1.0], lags=[0, 1, 4], origin_step=1, zero_dims=0)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.FourPointEngine(args["n_points"], args["cutoffs"], args["lags"], origin_step=args["origin_step"],
                                  zero_dims=args["zero_dims"])
    # n_cutoffs outside 1 ... 8 at the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    one, lag0, cut = np.array([2], dtype=np.int64), np.array([0], dtype=np.int64), np.arange(1.0, 10.0)
    for n_cutoffs in (0, 9, -1):
        assert lib.mdx_chi4_create(ctypes.byref(h), 0, 1, p(one), n_cutoffs, p(cut), 1, p(lag0), 1, 0) == -1
        assert b"n_cutoffs" in lib.mdx_last_error()
    assert lib.mdx_chi4_create(ctypes.byref(h), 0, 1, p(one), 2, p(cut), 0, p(lag0), 1, 0) == -1
    assert b"at least one lag" in lib.mdx_last_error()
    assert lib.mdx_chi4_create(ctypes.byref(h), 0, 1, p(one), 2, None, 1, p(lag0), 1, 0) == -1
    assert b"NULL" in lib.mdx_last_error()
    assert lib.mdx_chi4_set_segment_points(None, 64) == -1 and b"NULL" in lib.mdx_last_error()
    assert _core.FourPointEngine.TILE == 64 and _core.FourPointEngine._prefix == "mdx_chi4"


def test_engine_call_errors_need_no_device():
    eng = _core.FourPointEngine([2, 0, 3], [0.5, 1.0], [0, 1, 4], origin_step=2, zero_dims=2)     # an empty group
    try:
        assert (eng.n_groups, eng.n_points, eng.n_cutoffs, eng.n_lags) == (3, 5, 2, 3)
        with pytest.raises(ValueError, match="4 rows given, the groups hold 5"):
            eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
        rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
        with pytest.raises(ValueError, match="7 rows given, the groups hold 5"):
            eng.accumulate_device(rows, 7, 2)
        with pytest.raises(ValueError, match="index 7 out of range"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 7])
        for dims in ([10.0, 0.0, 10.0], [np.inf, 10.0, 10.0], [10.0, np.nan, 10.0]):
            with pytest.raises(ValueError, match="must be positive and finite"):
                eng.set_unwrap(dims)
        with pytest.raises(ValueError, match="three box lengths"):
            eng.set_unwrap([10.0, 10.0])
        for frames in (-1, 32769):
            with pytest.raises(ValueError, match="frames must lie in"):
                eng.set_slab_frames(frames)
        for points in (-64, 1, 63, 65, 100, 2 ** 31):
            with pytest.raises(ValueError, match="multiple of 64"):
                eng.set_segment_points(points)
        # what is allowed before the first frame, in any order and more than once
        eng.set_unwrap([10.0, 11.0, 12.0])
        eng.set_segment_points(64)
        eng.set_slab_frames(8)
        eng.set_unwrap(None)
        eng.set_segment_points(0)
        eng.set_slab_frames(0)
        eng.reset()
        eng.synchronize()
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0}
    finally:
        eng.close()


def test_overflow_is_refused_before_the_device():
    """12 points and 2^62 frames: 2^62 * 144 is beyond 2^63, so the sum of Q*Q could leave an int64.  The call returns
    -1 and names the overflow (not the missing device, not the frames it never read), on all three routes' entry
    points that need no file, and the handle stays usable."""
    lib = _lib.lib()
    eng = _core.FourPointEngine([12], [1.0], [0, 1])
    try:
        pos = np.zeros((1, 12, 3), dtype=np.float32)
        ptr = pos.ctypes.data_as(ctypes.c_void_p)
        assert lib.mdx_chi4_accumulate(eng.handle, ptr, 12, 2 ** 62) == -1
        message = lib.mdx_last_error()
        assert b"overflow" in message and b"12 points" in message and b"device" not in message
        assert lib.mdx_chi4_accumulate_device(eng.handle, ctypes.c_void_p(4096), 12, 2 ** 62, None, 0) == -1
        assert b"overflow" in lib.mdx_last_error()
        # the largest count that fits: (2^63 - 1) // 144 frames pass this check and fail later (rows, or the device)
        fits = (2 ** 63 - 1) // 144
        assert lib.mdx_chi4_accumulate(eng.handle, ptr, 12, fits + 1) == -1 and b"overflow" in lib.mdx_last_error()
        assert lib.mdx_chi4_accumulate(eng.handle, ptr, 11, fits) == -1
        assert b"11 rows given" in lib.mdx_last_error()
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0}
    finally:
        eng.close()
