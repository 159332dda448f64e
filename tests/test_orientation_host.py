"""
Host-side checks of the orientational relaxation analysis that need no GPU: the argument errors of ``mdx_ori_create``
and of the engine's calls, which are raised before any device is touched (a handle touches its device with the first
frame), the argument handling of ``analysis.dynamics.OrientationalRelaxation`` and the index arithmetic of its
``from_chains``.

Not reachable without a device, and therefore checked in ``test_gpu_orientation.py``: ``set_box`` /
``set_slab_frames`` after the first frame, and a degenerate vector (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import OrientationalRelaxation, dynamics

PAIRS = np.array([[0, 1], [1, 2], [2, 3], [4, 3], [0, 4]], dtype=np.int32)


# ---------------------------------------------------------------- the engine's argument errors

def test_engine_create_errors_need_no_device():
    for kwargs, word in ((dict(pairs=[[0, 1], [1, 2], [2, 3], [4, 5], [0, 4]]), "out of range"),
                         (dict(pairs=[[0, 1], [1, 2], [-1, 3], [4, 3], [0, 4]]), "out of range"),
                         (dict(pairs=[[0, 1], [1, 2], [3, 3], [4, 3], [0, 4]]), "both tail and head"),
                         (dict(pairs=[[0, 1], [1, 2]]), "one \\(tail, head\\) row per vector"),
                         (dict(lags=[]), "at least one lag"),
                         (dict(lags=[-1, 0]), "not be negative"),
                         (dict(lags=[0, 2, 2]), "strictly increasing"),
                         (dict(lags=[3, 1]), "strictly increasing"),
                         (dict(zero_dims=7), "at least one component"),
                         (dict(zero_dims=8), "at least one component"),
                         (dict(zero_dims=-1), "at least one component"),
                         (dict(n_vectors=[6, -1]), "not negative"),
                         (dict(n_vectors=[]), "one entry per group"),
                         (dict(n_rows=1), "n_rows"),
                         (dict(n_rows=2 ** 31 // 3), "n_rows")):
        args = dict(n_vectors=[2, 3], pairs=PAIRS, n_rows=5, lags=[0, 1, 4])
        zero_dims = kwargs.pop("zero_dims", 0)
        args.update(kwargs)
        with pytest.raises(ValueError, match=word):
            _core.OrientationEngine(args["n_vectors"], args["pairs"], args["n_rows"], args["lags"],
                                    zero_dims=zero_dims)
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    sizes, lags = np.array([2, 3], dtype=np.int64), np.array([0, 1, 4], dtype=np.int64)
    create = lambda *a: lib.mdx_ori_create(ctypes.byref(h), 0, *a)      # noqa: E731
    far = PAIRS.copy()
    far[3, 1] = 5
    assert create(2, p(sizes), 5, p(far), 3, p(lags), 0) == -1 and b"out of range" in lib.mdx_last_error()
    loop = PAIRS.copy()
    loop[2] = (3, 3)
    assert create(2, p(sizes), 5, p(loop), 3, p(lags), 0) == -1 and b"both tail and head" in lib.mdx_last_error()
    unsorted = np.array([0, 4, 1], dtype=np.int64)
    assert create(2, p(sizes), 5, p(PAIRS), 3, p(unsorted), 0) == -1
    assert b"strictly increasing" in lib.mdx_last_error()
    assert create(2, p(sizes), 5, p(PAIRS), 3, p(lags), 7) == -1 and b"at least one component" in lib.mdx_last_error()
    assert create(2, p(sizes), 5, p(PAIRS), 0, p(lags), 0) == -1 and b"at least one lag" in lib.mdx_last_error()
    none = np.zeros(2, dtype=np.int64)
    assert create(2, p(none), 5, p(PAIRS), 3, p(lags), 0) == -1 and b"hold no vector" in lib.mdx_last_error()
    assert create(2, p(sizes), 5, None, 3, p(lags), 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert create(2, None, 5, p(PAIRS), 3, p(lags), 0) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_ori_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_ori_set_box(None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert _core.OrientationEngine.TILE == 64 and _core.OrientationEngine._prefix == "mdx_ori"


def test_engine_call_errors_need_no_device():
    eng = _core.OrientationEngine([2, 0, 3], PAIRS, 5, [0, 1, 4], zero_dims=2)          # an empty group is allowed
    try:
        assert (eng.n_groups, eng.n_vectors, eng.n_rows, eng.n_lags) == (3, 5, 5, 3)
        with pytest.raises(ValueError, match="4 rows given, the pairs hold 5"):
            eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
        rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
        with pytest.raises(ValueError, match="7 rows given, the pairs hold 5"):
            eng.accumulate_device(rows, 7, 2)
        with pytest.raises(ValueError, match="4 rows given, the pairs hold 5"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
        with pytest.raises(ValueError, match="index 7 out of range"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 7])
        for dims in ([10.0, 0.0, 10.0], [10.0, 10.0, -1.0], [np.inf, 10.0, 10.0], [10.0, np.nan, 10.0]):
            with pytest.raises(ValueError, match="must be positive and finite"):
                eng.set_box(dims)
        with pytest.raises(ValueError, match="three box lengths"):
            eng.set_box([10.0, 10.0])
        for frames in (-1, 32769):
            with pytest.raises(ValueError, match="frames must lie in"):
                eng.set_slab_frames(frames)
        # what is allowed before the first frame, in any order and more than once
        eng.set_box([10.0, 11.0, 12.0])
        eng.set_slab_frames(8)
        eng.set_box(None)
        eng.set_slab_frames(0)
        eng.reset()
        eng.synchronize()
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "degenerate": 0}
        assert eng.frame_sums().shape == (0, 3, 6)
    finally:
        eng.close()


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=12, dims=(10.0, 12.0, 14.0), angles=(90.0, 90.0, 90.0), dt=0.5):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


def test_constructor_errors():
    u = _universe()
    tails, heads = u.select(np.arange(0, 6)), u.select(np.arange(6, 12))
    with pytest.raises(ValueError, match="a vector needs one of each"):
        OrientationalRelaxation(tails, u.select(np.arange(6, 11)))
    with pytest.raises(ValueError, match="same number of groups"):
        OrientationalRelaxation([tails, tails], [heads])
    with pytest.raises(ValueError, match="starts and ends on the same atom"):
        OrientationalRelaxation(u.select([0, 1, 2]), u.select([3, 1, 5]))
    with pytest.raises(ValueError, match="cannot both be given"):
        OrientationalRelaxation(tails, heads, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        OrientationalRelaxation(tails, heads, lags=[0, 2, 1])
    with pytest.raises(ValueError, match="drop_axis"):
        OrientationalRelaxation(tails, heads, drop_axis=3)
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        OrientationalRelaxation(tails, heads, dimensions=[10.0, 10.0])
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            OrientationalRelaxation(tails, heads, comm=TwoRanks(rank))
    # the box: orthorhombic with minimum_image=True, none needed with False
    skew = _universe(angles=(90.0, 80.0, 90.0))
    with pytest.raises(ValueError, match="needs an orthorhombic box"):
        OrientationalRelaxation(skew.select(np.arange(0, 6)), skew.select(np.arange(6, 12)))
    OrientationalRelaxation(skew.select(np.arange(0, 6)), skew.select(np.arange(6, 12)), minimum_image=False)
    bare = _universe(dims=None)
    with pytest.raises(ValueError, match="needs the box lengths"):
        OrientationalRelaxation(bare.select(np.arange(0, 6)), bare.select(np.arange(6, 12)))
    o = OrientationalRelaxation(bare.select(np.arange(0, 6)), bare.select(np.arange(6, 12)), minimum_image=False)
    assert o._dimensions is None
    o = OrientationalRelaxation(bare.select(np.arange(0, 6)), bare.select(np.arange(6, 12)),
                                dimensions=[10.0, 11.0, 12.0], drop_axis="z", n_lags=3)
    np.testing.assert_array_equal(o._dimensions, [10.0, 11.0, 12.0])
    np.testing.assert_array_equal(o._lags, [0, 1, 2])
    assert o._drop_axis == 2 and OrientationalRelaxation._shard_frames is False
    assert mdhelper_amd.analysis.OrientationalRelaxation is dynamics.OrientationalRelaxation


def test_index_and_pairs_feed_every_distinct_atom_once():
    u = _universe()
    # two groups given in an order that is not the frame's; atom 7 sits in three vectors
    tails = [u.select([9, 7, 7]), u.select([2, 0])]
    heads = [u.select([7, 3, 11]), u.select([0, 5])]
    o = OrientationalRelaxation(tails, heads, minimum_image=False)
    np.testing.assert_array_equal(o._index, [0, 2, 3, 5, 7, 9, 11])
    np.testing.assert_array_equal(o._Ns, [3, 2])
    assert o._pairs.dtype == np.int32
    np.testing.assert_array_equal(o._index[o._pairs], [[9, 7], [7, 3], [7, 11], [2, 0], [0, 5]])


@pytest.mark.parametrize("stride", [1, 3])
def test_from_chains_index_arithmetic(stride):
    n_chains, n_monomers = 3, 7
    u = _universe(n_atoms=n_chains * n_monomers + 4)
    ag = u.select(np.arange(2, 2 + n_chains * n_monomers)[::-1])       # any order: the chains are runs of `ag`
    o = OrientationalRelaxation.from_chains(ag, n_chains, n_monomers, stride=stride, minimum_image=False)
    want = [(ag.indices[c * n_monomers + n], ag.indices[c * n_monomers + n + stride])
            for c in range(n_chains) for n in range(n_monomers - stride)]
    np.testing.assert_array_equal(o._index[o._pairs], want)
    np.testing.assert_array_equal(o._Ns, [n_chains * (n_monomers - stride)])
    assert len(o._index) == n_chains * n_monomers
    explicit = OrientationalRelaxation(u.select([a for a, _ in want]), u.select([b for _, b in want]),
                                       minimum_image=False)
    np.testing.assert_array_equal(explicit._pairs, o._pairs)
    np.testing.assert_array_equal(explicit._index, o._index)
    with pytest.raises(ValueError, match="n_chains \\* n_monomers"):
        OrientationalRelaxation.from_chains(ag, n_chains, n_monomers + 1, minimum_image=False)
    for bad in (0, n_monomers):
        with pytest.raises(ValueError, match="'stride' must lie in"):
            OrientationalRelaxation.from_chains(ag, n_chains, n_monomers, stride=bad, minimum_image=False)


def _run_until_the_device(o, **kwargs):
    """``run()`` up to the point where the device is asked for: everything ``_prepare`` derives from the arguments
    is in place by then."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            o.run(**kwargs)
    else:
        o.run(**kwargs)
    return o


def test_prepare_errors_and_times():
    u = _universe()
    tails, heads = u.select(np.arange(0, 6)), u.select(np.arange(6, 12))
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        OrientationalRelaxation(tails, heads, verbose=False).run(frames=[0, 1, 3])
    o = _run_until_the_device(OrientationalRelaxation(tails, heads, lags=[0, 1, 2, 5], verbose=False), step=3)
    assert o.n_frames == 3
    np.testing.assert_array_equal(o.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    assert o.results.units["results.times"] == "picosecond"
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument
    o = _run_until_the_device(OrientationalRelaxation(tails, heads, dt=2.0, verbose=False), frames=[1, 3, 5])
    np.testing.assert_array_equal(o.results.times, np.arange(3) * 2 * 2.0)
    with pytest.raises(RuntimeError, match="before calculate_relaxation_times"):
        OrientationalRelaxation(tails, heads, verbose=False).calculate_relaxation_times()


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            OrientationalRelaxation(u.select(np.arange(0, 6)), u.select(np.arange(6, 12)), verbose=False).run()
        eng = _core.OrientationEngine([5], PAIRS, 5, [0, 1])
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 5, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()
