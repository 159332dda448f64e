"""
Host-side checks of ``analysis.polymer.InternalDistances`` that need no GPU: the argument handling, the calls it hands
to its engine (a recorder stands in for ``_core.InternalDistanceEngine``, which is only created in ``_prepare``), the
result layout, the host formulas and the engine's argument errors.  The reference project has no such analysis:
nothing is compared with it.
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.algorithm.topology import unwrap_edge
from mdhelper_amd.analysis import InternalDistances, polymer
from mdhelper_amd.comm import shard_range

L = np.array([10.0, 12.0, 14.0])


def _universe(n_frames=6, n_atoms=60, dims=L, seed=0, angles=(90.0, 90.0, 90.0), **topology):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, *angles]
    return mdhelper_amd.ArrayUniverse(pos, box, **topology)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank, self.reduced = rank, []

    def allreduce(self, arr, op="sum"):
        arr = np.asarray(arr)
        assert arr.dtype == np.float64 and op == "sum"
        self.reduced.append(arr.copy())
        return arr * 2                      # "the other rank" held the same numbers


class Recorder:
    """Stands in for ``_core.InternalDistanceEngine``: records what it is fed; row r of frame f of its result is
    1000 f' + r with f' counted over the frames it was handed."""
    made = []

    def __init__(self, n_chains, n_monomers, *, dev=0, timing=False):
        self.n_chains, self.n_monomers = [int(x) for x in n_chains], [int(x) for x in n_monomers]
        self.frames, self.calls, self.log = 0, [], []
        self.grouping = self.unwrap = self.whole = self.reserved = None
        self.closed = False
        Recorder.made.append(self)

    def set_grouping(self, offsets, masses):
        self.log.append("set_grouping")
        self.grouping = (np.asarray(offsets), np.asarray(masses))

    def set_unwrap(self, dims, start=None):
        self.log.append("set_unwrap")
        self.unwrap = (np.asarray(dims), np.asarray(start))

    def set_whole(self, dims):
        self.log.append("set_whole")
        self.whole = np.asarray(dims)

    def reserve(self, n_frames):
        self.reserved = n_frames

    def accumulate(self, pos):
        self.log.append("accumulate")
        self.calls.append(np.array(pos))
        self.frames += len(pos)

    def result(self):
        assert not self.closed
        out, r0 = [], 0
        for N in self.n_monomers:
            rows = 1000.0 * np.arange(self.frames)[:, None] + r0 + np.arange(2 * (N - 1))[None, :]
            out.append(rows.reshape(self.frames, 2, N - 1))
            r0 += 2 * (N - 1)
        return out

    def close(self):
        self.closed = True


@pytest.fixture
def recorder(monkeypatch):
    Recorder.made = []
    monkeypatch.setattr(_core, "InternalDistanceEngine", Recorder)
    return Recorder


# ---------------------------------------------------------------- arguments

def test_argument_errors():
    u = _universe()
    kw = {"n_chains": 6, "n_monomers": 10, "verbose": False}
    with pytest.raises(ValueError, match="n_monomers >= 2"):
        InternalDistances(u.atoms, n_chains=60, n_monomers=1, verbose=False)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    with pytest.raises(ValueError, match="Group 1 has chains of 1 monomer"):
        InternalDistances([a, b], n_chains=(5, 40), n_monomers=(4, 1), verbose=False)
    with pytest.raises(ValueError, match="'unwrap' and 'whole' cannot be combined"):
        InternalDistances(u.atoms, unwrap=True, whole=True, **kw)
    with pytest.raises(ValueError, match="no system dimensions found or provided"):
        InternalDistances(_universe(dims=None).atoms, whole=True, **kw)
    with pytest.raises(ValueError, match="orthorhombic"):
        InternalDistances(_universe(angles=(90.0, 80.0, 90.0)).atoms, whole=True, **kw)
    with pytest.raises(ValueError, match="must have length 3"):
        InternalDistances(u.atoms, whole=True, dimensions=[10.0, 10.0], **kw)
    with pytest.raises(ValueError, match="positive and finite"):
        InternalDistances(u.atoms, whole=True, dimensions=[10.0, 0.0, 10.0], **kw)
    with pytest.raises(ValueError, match="positive and finite"):
        InternalDistances(u.atoms, whole=True, dimensions=[10.0, np.inf, 10.0], **kw)
    # what it shares with the other chain analyses
    with pytest.raises(ValueError, match="No system dimensions found"):
        InternalDistances(_universe(dims=None).atoms, unwrap=True, **kw)
    with pytest.raises(ValueError, match="unwrap cannot be combined with more than one rank"):
        InternalDistances(u.atoms, unwrap=True, comm=TwoRanks(0), **kw)
    with pytest.raises(ValueError, match="Group 0 holds 60 atoms, which do not form n_chains"):
        InternalDistances(u.atoms, n_chains=7, n_monomers=10, verbose=False)
    with pytest.raises(ValueError, match="Invalid grouping 'segments'"):
        InternalDistances(u.atoms, "segments", 6, 10)
    InternalDistances(_universe(dims=None).atoms, **kw)                      # no box needed without unwrap / whole
    InternalDistances(_universe(dims=None).atoms, whole=True, dimensions=L, **kw)
    InternalDistances(u.atoms, whole=True, comm=TwoRanks(1), **kw)           # whole keeps the frames shardable
    InternalDistances(_universe(angles=(90.0, 80.0, 90.0)).atoms, **kw)      # the box plays no part without whole


def test_evaluation_needs_a_run(recorder):
    r = InternalDistances(_universe().atoms, n_chains=6, n_monomers=10, verbose=False)
    with pytest.raises(RuntimeError, match="Call InternalDistances.run"):
        r.calculate_characteristic_ratio()
    with pytest.raises(RuntimeError, match="Call InternalDistances.run"):
        r.calculate_persistence_length()


# ---------------------------------------------------------------- calls

def test_plain_atoms_reach_the_engine(recorder):
    u = _universe()
    a, b = u.select(np.arange(20, 60)), u.select(np.arange(20))
    InternalDistances([a, b], n_chains=(4, 5), n_monomers=(10, 4), verbose=False).run(step=2)
    (eng,) = recorder.made
    assert (eng.n_chains, eng.n_monomers) == ([4, 5], [10, 4])
    assert eng.log == ["accumulate"] and eng.closed and eng.reserved == 3
    order = np.r_[20:60, 0:20]                              # concatenated-group order
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(0, 6, 2))[:, order])


def test_residues_reach_the_engine(recorder):
    masses = np.tile([12.0, 1.0, 3.0], 20)
    u = _universe(masses=masses)
    InternalDistances(u.atoms, "residues", 4, 5, verbose=False).run()
    (eng,) = recorder.made
    assert eng.log == ["set_grouping", "accumulate"] and eng.closed
    assert (eng.n_chains, eng.n_monomers) == ([4], [5])
    np.testing.assert_array_equal(eng.grouping[0], 3 * np.arange(21))
    np.testing.assert_array_equal(eng.grouping[1], masses)
    assert eng.calls[0].shape == (6, 60, 3)


def test_unwrap_starts_from_whole_chains(recorder):
    rng = np.random.default_rng(3)
    M, N_p, F = 3, 8, 4
    steps = rng.normal(size=(F, M, N_p, 3))
    steps *= 0.7 / np.linalg.norm(steps, axis=-1, keepdims=True)
    pos = np.mod(rng.random((F, M, 1, 3)) * L + np.cumsum(steps, axis=2), L).reshape(F, -1, 3).astype(np.float32)
    u = mdhelper_amd.ArrayUniverse(pos, [*L, 90.0, 90.0, 90.0])
    InternalDistances(u.atoms, n_chains=M, n_monomers=N_p, unwrap=True, verbose=False).run(start=1)
    (eng,) = recorder.made
    assert eng.log == ["set_unwrap", "accumulate"] and eng.whole is None
    dims, start = eng.unwrap
    np.testing.assert_array_equal(dims, L)
    bonds = (np.arange(M)[:, None] * N_p + np.arange(N_p - 1)[None, :]).ravel()
    want = unwrap_edge(positions=pos[1].astype(float), bonds=np.stack((bonds, bonds + 1), axis=1), dimensions=L,
                       masses=np.ones(M * N_p))
    np.testing.assert_array_equal(start, want)
    assert start.dtype == np.float64
    np.testing.assert_array_equal(eng.calls[0], pos[1:])


def test_whole_hands_the_box_lengths_over(recorder):
    u = _universe(masses=np.ones(60))
    InternalDistances(u.atoms, n_chains=6, n_monomers=10, whole=True, verbose=False).run()
    (eng,) = recorder.made
    assert sorted(eng.log) == ["accumulate", "set_whole"] and eng.log[-1] == "accumulate"
    assert eng.unwrap is None
    np.testing.assert_array_equal(eng.whole, L)
    assert eng.whole.dtype == np.float64
    # box lengths given by the caller win; with a grouping the centres are formed first and then made whole
    InternalDistances(u.atoms, "residues", 6, 5, whole=True, dimensions=[20.0, 21.0, 22.0], verbose=False).run()
    eng = recorder.made[1]
    assert sorted(eng.log) == ["accumulate", "set_grouping", "set_whole"] and eng.log[-1] == "accumulate"
    np.testing.assert_array_equal(eng.whole, [20.0, 21.0, 22.0])


# ---------------------------------------------------------------- results

def test_result_shapes_for_two_chain_lengths(recorder):
    u = _universe(n_frames=5)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    r = InternalDistances([a, b], n_chains=(5, 4), n_monomers=(4, 10), verbose=False).run()
    res = r.results
    assert [len(x) for x in (res.separations, res.squared_distances, res.bond_cosines, res.mean_squared_distances,
                             res.mean_bond_cosines)] == [2] * 5
    for g, (N, r0) in enumerate(((4, 0), (10, 6))):
        np.testing.assert_array_equal(res.separations[g], np.arange(1, N))
        assert np.issubdtype(res.separations[g].dtype, np.integer)
        rows = 1000.0 * np.arange(5)[:, None] + r0 + np.arange(2 * (N - 1))[None, :]
        np.testing.assert_array_equal(res.squared_distances[g], rows[:, :N - 1])
        np.testing.assert_array_equal(res.bond_cosines[g], rows[:, N - 1:])
        np.testing.assert_array_equal(res.mean_squared_distances[g], rows[:, :N - 1].mean(axis=0))
        np.testing.assert_array_equal(res.mean_bond_cosines[g], rows[:, N - 1:].mean(axis=0))
    assert res.units["results.squared_distances"] == "angstrom^2"
    r.calculate_characteristic_ratio()
    for g in range(2):
        r2 = res.mean_squared_distances[g]
        np.testing.assert_array_equal(res.characteristic_ratio[g], r2 / (res.separations[g] * r2[0]))


def test_two_ranks_share_the_frames_and_reduce_once(recorder):
    u = _universe(n_frames=7)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    full = []
    for rank in (0, 1):
        comm = TwoRanks(rank)
        r = InternalDistances([a, b], n_chains=(5, 4), n_monomers=(4, 10), whole=True, verbose=False, comm=comm).run()
        eng = recorder.made[rank]
        lo, hi = shard_range(7, rank, 2)
        assert eng.frames == hi - lo == eng.reserved
        np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(lo, hi)))
        (sent,) = comm.reduced                              # one float64 all-reduce of all groups' rows
        assert sent.shape == (7, 6 + 18) and sent.dtype == np.float64
        assert np.all(sent[:lo] == 0) and np.all(sent[hi:] == 0)
        # what the recorder returned for this rank's frames: group 0's 6 rows, then group 1's 18
        np.testing.assert_array_equal(sent[lo:hi], 1000.0 * np.arange(hi - lo)[:, None] + np.arange(24)[None, :])
        assert r.results.squared_distances[1].shape == (7, 9)
        np.testing.assert_array_equal(r.results.bond_cosines[1], 2 * sent[:, 6 + 9:])
        full.append(sent)
    assert np.all((full[0] != 0).any(axis=1) ^ (full[1] != 0).any(axis=1))       # every frame on one rank


# ---------------------------------------------------------------- host formulas

def test_characteristic_ratio_of_a_rod():
    s = np.arange(1, 30)
    np.testing.assert_allclose(polymer.calculate_characteristic_ratio((1.5 * s) ** 2), s, rtol=1e-15)
    both = polymer.calculate_characteristic_ratio(np.stack(((1.5 * s) ** 2, 2.0 * s)))     # a rod, a random walk
    np.testing.assert_allclose(both, np.stack((s, np.ones(29))), rtol=1e-15)


def test_persistence_length_of_an_exponential():
    c = np.exp(-np.arange(30) / 5)
    for n_fit in (None, 1, 4, 12, 29):
        np.testing.assert_allclose(polymer.calculate_persistence_length(c, 1.5, n_fit), 7.5, rtol=1e-12)
    # the default window ends before C first falls to 1 / e: a correlation that turns negative later is no obstacle
    tail = c.copy()
    tail[8:] = -0.01
    np.testing.assert_allclose(polymer.calculate_persistence_length(tail, 1.5), 7.5, rtol=1e-12)
    with pytest.raises(ValueError, match="positive inside the fit window"):
        polymer.calculate_persistence_length(tail, 1.5, n_fit=8)
    with pytest.raises(ValueError, match="positive inside the fit window"):
        polymer.calculate_persistence_length(np.array([1.0, 0.0, 0.5]), 1.5)        # n_fit is at least 1
    with pytest.raises(ValueError, match="n_fit"):
        polymer.calculate_persistence_length(c, 1.5, n_fit=30)
    with pytest.raises(ValueError, match="n_fit"):
        polymer.calculate_persistence_length(c, 1.5, n_fit=0)
    with pytest.raises(ValueError, match="at least two"):
        polymer.calculate_persistence_length(np.array([1.0]), 1.5)
    assert polymer.calculate_persistence_length(np.ones(5), 1.5) == np.inf          # a rod


def test_persistence_length_lands_in_the_results(recorder):
    class Exponential(Recorder):
        def result(self):
            (N,) = self.n_monomers
            r2 = 2.25 * np.arange(1, N)
            c = np.exp(-1.5 * np.arange(N - 1) / 6.0)
            return [np.tile(np.stack((r2, c))[None], (self.frames, 1, 1))]
    import unittest.mock as mock
    with mock.patch.object(_core, "InternalDistanceEngine", Exponential):
        r = InternalDistances(_universe().atoms, n_chains=3, n_monomers=20, verbose=False).run()
    r.calculate_persistence_length()
    assert len(r.results.persistence_length) == 1
    np.testing.assert_allclose(r.results.persistence_length[0], 6.0, rtol=1e-12)
    assert r.results.units["results.persistence_length"] == "angstrom"
    r.calculate_persistence_length(n_fit=2)
    np.testing.assert_allclose(r.results.persistence_length[0], 6.0, rtol=1e-12)


# ---------------------------------------------------------------- the engine without a device

def test_no_cpu_fallback():
    """Without a HIP device the class and the engine raise; nothing walks the chains on the host instead."""
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            InternalDistances(_universe().atoms, n_chains=6, n_monomers=10, verbose=False).run()
        with pytest.raises(RuntimeError):
            _core.InternalDistanceEngine([6], [10])
    assert mdhelper_amd.analysis.InternalDistances is polymer.InternalDistances


def test_engine_argument_errors_need_no_device():
    lib = _lib.lib()
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)         # noqa: E731
    for n_chains, n_monomers, word in ((i64(0), i64(3), b"n_chains"),
                                       (i64(3), i64(1), b"n_monomers must be at least 2"),
                                       (i64(3), i64(0), b"n_monomers must be at least 2"),
                                       (i64(1 << 20), i64(1 << 20), b"2^31 / 3 points"),
                                       (i64(1), i64(1 << 30), b"n_monomers")):
        rc = lib.mdx_msid_create(ctypes.byref(h), 0, 1, p(n_chains), p(n_monomers))
        assert rc == -1 and word in lib.mdx_last_error(), (word, lib.mdx_last_error())
    two = i64(3, 3)
    assert lib.mdx_msid_create(ctypes.byref(h), 0, 2, p(two), p(i64(5, 1))) == -1
    assert b"group 1: n_monomers" in lib.mdx_last_error()
    for args in ((None, 0, 1, p(two), p(two)), (ctypes.byref(h), 0, 1, None, p(two)),
                 (ctypes.byref(h), 0, 1, p(two), None)):
        assert lib.mdx_msid_create(*args) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_msid_create(ctypes.byref(h), 0, 0, p(two), p(two)) == -1 and b"n_groups" in lib.mdx_last_error()
    for fn in (lib.mdx_msid_reset, lib.mdx_msid_synchronize):
        assert fn(None) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_msid_set_whole(None, p(L)) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_msid_set_unwrap(None, p(L), p(L)) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_msid_destroy(None) == 0
    with pytest.raises(ValueError, match="one entry per group"):
        _core.InternalDistanceEngine([2, 1], [3])
    with pytest.raises(ValueError, match="at least 2"):
        _core.InternalDistanceEngine([2], [1])
