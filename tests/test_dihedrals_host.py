"""
Host-side checks of the dihedral analysis that need no GPU: the argument errors of ``mdx_dih_create`` and of the
engine's calls, which are raised before any device is touched (a handle touches its device with the first frame), the
argument handling of ``analysis.dihedral.Dihedrals``, the index arithmetic of its ``from_chains``, the bins its
``state_edges`` map to, and the threshold rule of the contract against the angle itself on the CPU.

Not reachable without a device, and therefore checked in ``test_gpu_dihedrals.py``: ``set_box`` / ``set_slab_frames``
after the first frame, and a degenerate dihedral (there is no first frame without a device).
"""
import ctypes

import numpy as np
import pytest

import dihedral_cases as dc
import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import Dihedrals, dihedral

QUADS = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 2, 0, 5], [5, 4, 3, 2], [0, 5, 1, 4]], dtype=np.int32)
N_BINS = 6
THRESHOLDS = dihedral.cosine_thresholds(N_BINS)
STATES = dihedral.states_of_bins(N_BINS, (-120.0, 0.0, 120.0))


def _engine(**kwargs):
    args = dict(n_dihedrals=[2, 3], quads=QUADS, n_rows=6, thresholds=THRESHOLDS, state_of_bin=STATES,
                lags=[0, 1, 4], n_states=3)
    args.update(kwargs)
    n_states = args.pop("n_states")
    return _core.DihedralEngine(args["n_dihedrals"], args["quads"], args["n_rows"], args["thresholds"],
                                args["state_of_bin"], args["lags"], n_states=n_states)


# ---------------------------------------------------------------- the engine's argument errors

def test_engine_create_errors_need_no_device():
    far, low, twice = QUADS.copy(), QUADS.copy(), QUADS.copy()
    far[3, 2], low[2, 0], twice[4, 3] = 6, -1, 0
    flat = THRESHOLDS.copy()
    flat[2] = flat[1]
    for kwargs, word in ((dict(quads=far), "out of range"),
                         (dict(quads=low), "out of range"),
                         (dict(quads=twice), "named twice"),
                         (dict(quads=QUADS[:2]), "one \\(a, b, c, d\\) row per dihedral"),
                         (dict(quads=QUADS[:, :3]), "one \\(a, b, c, d\\) row per dihedral"),
                         (dict(state_of_bin=STATES[:5]), "even number"),
                         (dict(state_of_bin=[0, 0, 0, 0, 0]), "even number"),
                         (dict(thresholds=THRESHOLDS[:3]), "n_bins / 2 \\+ 1"),
                         (dict(thresholds=flat), "strictly decreasing"),
                         (dict(thresholds=THRESHOLDS[::-1]), "strictly decreasing"),
                         (dict(thresholds=[1.0, np.nan, -0.5, -1.0]), "strictly decreasing"),
                         (dict(state_of_bin=[0, 1, 2, 3, 0, 1]), "state_of_bin\\[3\\] = 3 out of range"),
                         (dict(state_of_bin=[0, 1, -1, 2, 0, 1]), "state_of_bin\\[2\\] = -1 out of range"),
                         (dict(n_states=0), "n_states must lie in \\[1, 8\\]"),
                         (dict(n_states=9), "n_states must lie in \\[1, 8\\]"),
                         (dict(lags=[]), "at least one lag"),
                         (dict(lags=[-1, 0]), "not be negative"),
                         (dict(lags=[0, 2, 2]), "strictly increasing"),
                         (dict(lags=[3, 1]), "strictly increasing"),
                         (dict(lags=[0, 2 ** 31]), "below 2\\^31"),
                         (dict(n_dihedrals=[6, -1]), "not negative"),
                         (dict(n_dihedrals=[]), "one entry per group"),
                         (dict(n_rows=3), "n_rows"),
                         (dict(n_rows=2 ** 31 // 4), "n_rows")):
        with pytest.raises(ValueError, match=word):
            _engine(**kwargs)
    _engine(lags=[0, 2 ** 31 - 1]).close()                  # the largest lag a run length can reach
    _engine(n_states=8).close()
    # the C entry point itself
    lib, h = _lib.lib(), ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    sizes, lags = np.array([2, 3], dtype=np.int64), np.array([0, 1, 4], dtype=np.int64)

    def create(sizes=p(sizes), n_rows=6, quads=p(QUADS), n_bins=N_BINS, thresholds=p(THRESHOLDS), n_states=3,
               states=p(STATES), n_lags=3, lags=p(lags)):
        return lib.mdx_dih_create(ctypes.byref(h), 0, 2, sizes, n_rows, quads, n_bins, thresholds, n_states, states,
                                  n_lags, lags)

    assert create(quads=p(far)) == -1 and b"out of range" in lib.mdx_last_error()
    assert create(quads=p(twice)) == -1 and b"named twice" in lib.mdx_last_error()
    assert create(n_bins=5) == -1 and b"n_bins must be even" in lib.mdx_last_error()
    assert create(n_bins=0) == -1 and b"n_bins must be even" in lib.mdx_last_error()
    assert create(thresholds=p(flat)) == -1 and b"strictly decreasing" in lib.mdx_last_error()
    assert create(n_states=2) == -1 and b"state_of_bin[0] = 2 out of range" in lib.mdx_last_error()
    assert create(n_states=0) == -1 and b"n_states must lie in" in lib.mdx_last_error()
    assert create(n_states=9) == -1 and b"n_states must lie in" in lib.mdx_last_error()
    unsorted = np.array([0, 4, 1], dtype=np.int64)
    assert create(lags=p(unsorted)) == -1 and b"strictly increasing" in lib.mdx_last_error()
    long = np.array([0, 1, 2 ** 31], dtype=np.int64)
    assert create(lags=p(long)) == -1 and b"below 2^31" in lib.mdx_last_error()
    assert create(n_lags=0) == -1 and b"at least one lag" in lib.mdx_last_error()
    assert create(n_rows=3) == -1 and b"n_rows" in lib.mdx_last_error()
    none = np.zeros(2, dtype=np.int64)
    assert create(sizes=p(none)) == -1 and b"hold no dihedral" in lib.mdx_last_error()
    for name in ("sizes", "quads", "thresholds", "states", "lags"):
        assert create(**{name: None}) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dih_create(None, 0, 2, p(sizes), 6, p(QUADS), N_BINS, p(THRESHOLDS), 3, p(STATES), 3,
                              p(lags)) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dih_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dih_set_box(None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dih_result(None, None, None, None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dih_destroy(None) == 0
    assert _core.DihedralEngine.TILE == 64 and _core.DihedralEngine._prefix == "mdx_dih"
    assert _core.DihedralEngine.MAX_STATES == 8 and _core.DihedralEngine.LDS_BINS % 2 == 0


def test_engine_call_errors_need_no_device():
    eng = _engine(n_dihedrals=[2, 0, 3])                    # an empty group is allowed
    try:
        assert (eng.n_groups, eng.n_dihedrals, eng.n_rows, eng.n_lags, eng.n_bins, eng.n_states) == (3, 5, 6, 3, 6, 3)
        with pytest.raises(ValueError, match="4 rows given, the quads hold 6"):
            eng.accumulate(np.zeros((2, 4, 3), dtype=np.float32))
        rows = ctypes.c_void_p(4096)        # never read: the arguments are refused first
        with pytest.raises(ValueError, match="7 rows given, the quads hold 6"):
            eng.accumulate_device(rows, 7, 2)
        with pytest.raises(ValueError, match="4 rows given, the quads hold 6"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3])
        with pytest.raises(ValueError, match="index 7 out of range"):
            eng.accumulate_device(rows, 7, 2, [0, 1, 2, 3, 4, 7])
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
        assert eng.plan() == {"slab_frames": 8, "ring_frames": 12}          # max lag 4 + slab 8
        eng.set_box(None)
        eng.set_slab_frames(0)
        eng.reset()
        eng.synchronize()
        assert eng.stats() == {"launches": 0, "kernel_ms": 0.0, "frames": 0, "evaluations": 0, "degenerate": 0}
        assert eng.state_counts().shape == (0, 3, 3)
    finally:
        eng.close()
    # run(f) looks at frame f - 1, so the ring holds at least one frame before the slab even without a lag
    eng = _engine(lags=[0])
    try:
        eng.set_slab_frames(8)
        assert eng.plan() == {"slab_frames": 8, "ring_frames": 9}
    finally:
        eng.close()


# ---------------------------------------------------------------- the rule and the states, on the CPU

def test_threshold_rule_agrees_with_the_angle():
    dc.check_threshold_rule_against_atan2()


def test_thresholds_and_states_of_bins():
    t = dihedral.cosine_thresholds(180)
    assert t.shape == (91,) and t[0] == 1.0 and t[90] == -1.0 and np.all(np.diff(t) < 0)
    np.testing.assert_allclose(t, np.cos(np.deg2rad(np.arange(0, 181, 2))), atol=1e-15)
    # the default: gauche- [-120, 0), gauche+ [0, 120), trans through +-180
    states = dihedral.states_of_bins(180, (-120.0, 0.0, 120.0))
    lower = -180.0 + 2.0 * np.arange(180)
    np.testing.assert_array_equal(states,
                                  np.where(lower < -120, 2, np.where(lower < 0, 0, np.where(lower < 120, 1, 2))))
    np.testing.assert_array_equal(dihedral.states_of_bins(6, (-120.0, 0.0, 120.0)), [2, 0, 0, 1, 1, 2])
    np.testing.assert_array_equal(dihedral.states_of_bins(4, (-180.0, 0.0)), [0, 0, 1, 1])
    np.testing.assert_array_equal(dihedral.states_of_bins(4, (90.0,)), [0, 0, 0, 0])
    np.testing.assert_array_equal(dihedral.states_of_bins(8, (-135.0, -90.0, 45.0)), [2, 0, 1, 1, 1, 2, 2, 2])
    for edges, word in (((-120.0, 1.0, 120.0), "fall on a bin edge"),
                        ((-119.0,), "fall on a bin edge"),
                        ((0.0, -120.0), "ascending"),
                        ((0.0, 0.0), "ascending"),
                        ((-182.0, 0.0), "ascending and lie in"),
                        ((0.0, 180.0), "ascending and lie in"),
                        ((), "1 to 8 boundaries"),
                        (tuple(-180.0 + 40.0 * np.arange(9)), "1 to 8 boundaries")):
        with pytest.raises(ValueError, match=word):
            dihedral.states_of_bins(180, edges)


# ---------------------------------------------------------------- the class

def _universe(n_frames=7, n_atoms=16, dims=(10.0, 12.0, 14.0), angles=(90.0, 90.0, 90.0), dt=0.5):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, dt=dt)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


def _legs(u):
    return [u.select(np.arange(4 * i, 4 * i + 4)) for i in range(4)]


def test_constructor_errors():
    u = _universe()
    legs = _legs(u)
    with pytest.raises(ValueError, match="a dihedral needs one of each"):
        Dihedrals(legs[0], legs[1], legs[2], u.select(np.arange(12, 15)))
    with pytest.raises(ValueError, match="same number of groups"):
        Dihedrals([legs[0], legs[0]], [legs[1]], [legs[2]], [legs[3]])
    with pytest.raises(ValueError, match="names an atom twice"):
        Dihedrals(u.select([0, 1]), u.select([2, 3]), u.select([4, 5]), u.select([6, 1]))
    with pytest.raises(ValueError, match="at least one dihedral"):
        Dihedrals(*(u.select([]) for _ in range(4)))
    with pytest.raises(ValueError, match="cannot both be given"):
        Dihedrals(*legs, lags=[0, 1], n_lags=2)
    with pytest.raises(ValueError, match="non-negative and strictly increasing"):
        Dihedrals(*legs, lags=[0, 2, 1])
    for n_bins in (0, 7, 181):
        with pytest.raises(ValueError, match="'n_bins' must be even"):
            Dihedrals(*legs, n_bins=n_bins)
    with pytest.raises(ValueError, match="fall on a bin edge"):
        Dihedrals(*legs, n_bins=36, state_edges=(-120.0, 5.0, 120.0))
    with pytest.raises(ValueError, match="fall on a bin edge"):
        Dihedrals(*legs, n_bins=8)                          # -120 is no multiple of 45 from -180
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        Dihedrals(*legs, dimensions=[10.0, 10.0])
    for rank in (0, 1):
        with pytest.raises(ValueError, match="runs on one rank"):
            Dihedrals(*legs, comm=TwoRanks(rank))
    # the box: orthorhombic with minimum_image=True, none needed with False
    skew = _universe(angles=(90.0, 80.0, 90.0))
    with pytest.raises(ValueError, match="needs an orthorhombic box"):
        Dihedrals(*_legs(skew))
    Dihedrals(*_legs(skew), minimum_image=False)
    bare = _universe(dims=None)
    with pytest.raises(ValueError, match="needs the box lengths"):
        Dihedrals(*_legs(bare))
    o = Dihedrals(*_legs(bare), minimum_image=False)
    assert o._dimensions is None and o._n_bins == 180 and o._n_states == 3
    o = Dihedrals(*_legs(bare), dimensions=[10.0, 11.0, 12.0], n_lags=3, n_bins=4, state_edges=(-90.0, 90.0))
    np.testing.assert_array_equal(o._dimensions, [10.0, 11.0, 12.0])
    np.testing.assert_array_equal(o._lags, [0, 1, 2])
    np.testing.assert_array_equal(o._state_of_bin, [1, 0, 0, 1])
    np.testing.assert_array_equal(o._thresholds, [1.0, np.cos(np.pi / 2), -1.0])
    assert Dihedrals._shard_frames is False
    assert mdhelper_amd.analysis.Dihedrals is dihedral.Dihedrals


def test_index_and_quads_feed_every_distinct_atom_once():
    u = _universe()
    # two groups given in an order that is not the frame's; atom 7 sits in three dihedrals
    first = [u.select([9, 7, 3]), u.select([2, 0])]
    second = [u.select([7, 3, 11]), u.select([0, 5])]
    third = [u.select([3, 11, 7]), u.select([5, 14])]
    fourth = [u.select([11, 9, 9]), u.select([14, 2])]
    o = Dihedrals(first, second, third, fourth, minimum_image=False)
    np.testing.assert_array_equal(o._index, [0, 2, 3, 5, 7, 9, 11, 14])
    np.testing.assert_array_equal(o._Ns, [3, 2])
    assert o._quads.dtype == np.int32 and o._quads.flags.c_contiguous
    np.testing.assert_array_equal(o._index[o._quads],
                                  [[9, 7, 3, 11], [7, 3, 11, 9], [3, 11, 7, 9], [2, 0, 5, 14], [0, 5, 14, 2]])


def test_from_chains_index_arithmetic():
    n_chains, n_monomers = 3, 7
    u = _universe(n_atoms=n_chains * n_monomers + 4)
    ag = u.select(np.arange(2, 2 + n_chains * n_monomers)[::-1])       # any order: the chains are runs of `ag`
    o = Dihedrals.from_chains(ag, n_chains, n_monomers, minimum_image=False)
    want = [tuple(ag.indices[c * n_monomers + n + i] for i in range(4))
            for c in range(n_chains) for n in range(n_monomers - 3)]
    np.testing.assert_array_equal(o._index[o._quads], want)
    np.testing.assert_array_equal(o._Ns, [n_chains * (n_monomers - 3)])
    assert len(o._index) == n_chains * n_monomers
    explicit = Dihedrals(*(u.select([w[i] for w in want]) for i in range(4)), minimum_image=False)
    np.testing.assert_array_equal(explicit._quads, o._quads)
    np.testing.assert_array_equal(explicit._index, o._index)
    assert len(Dihedrals.from_chains(u.select(np.arange(8)), 2, 4, minimum_image=False)._quads) == 2
    with pytest.raises(ValueError, match="n_chains \\* n_monomers"):
        Dihedrals.from_chains(ag, n_chains, n_monomers + 1, minimum_image=False)
    with pytest.raises(ValueError, match="n_monomers >= 4"):
        Dihedrals.from_chains(u.select(np.arange(9)), 3, 3, minimum_image=False)


def _run_until_the_device(o, **kwargs):
    """``run()`` up to the point where the device is asked for: everything ``_prepare`` derives from the arguments
    is in place by then."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            o.run(**kwargs)
    else:
        o.run(**kwargs)
    return o


def test_prepare_errors_times_and_helpers_before_run():
    u = _universe()
    legs = _legs(u)
    with pytest.raises(ValueError, match="evenly spaced and proceed forward in time"):
        Dihedrals(*legs, verbose=False).run(frames=[0, 1, 3])
    o = _run_until_the_device(Dihedrals(*legs, lags=[0, 1, 2, 5], verbose=False), step=3)
    assert o.n_frames == 3
    np.testing.assert_array_equal(o.results.times, np.array([0, 1, 2, 5]) * 3 * 0.5)
    assert o.results.units["results.times"] == "picosecond" and o.results.units["results.angles"] == "degree"
    # neither lags nor n_lags: every analysed frame is a lag; dt from the argument
    o = _run_until_the_device(Dihedrals(*legs, dt=2.0, verbose=False), frames=[1, 3, 5])
    np.testing.assert_array_equal(o.results.times, np.arange(3) * 2 * 2.0)
    fresh = Dihedrals(*legs, verbose=False)
    with pytest.raises(RuntimeError, match="before calculate_relaxation_times"):
        fresh.calculate_relaxation_times()
    with pytest.raises(RuntimeError, match="before calculate_transition_rates"):
        fresh.calculate_transition_rates()
    with pytest.raises(RuntimeError, match="before calculate_pmf"):
        fresh.calculate_pmf(300.0)


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine's first frame raise."""
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            Dihedrals(*_legs(u), verbose=False).run()
        eng = _engine()
        with pytest.raises(RuntimeError):
            eng.accumulate(np.zeros((2, 6, 3), dtype=np.float32))
        with pytest.raises(RuntimeError):
            eng.result()
        eng.close()
