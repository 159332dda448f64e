"""
Host-side checks of ``analysis.polymer.RouseModes`` that need no GPU: the argument handling, the weights and the
calls it hands to its two engines.  Recorders stand in for ``_core.ChainProjectionEngine`` and ``_core.MsdEngine``,
which are only created in ``_prepare`` / ``_conclude``.  ``Gyradius`` shares its selection and unwrap set-up with
``RouseModes`` through ``_PolymerAnalysisBase``; the last tests pin the calls it makes to its engine.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.algorithm.topology import unwrap_edge
from mdhelper_amd.analysis import Gyradius, RouseModes, polymer
from mdhelper_amd.comm import shard_range


def _universe(n_frames=6, n_atoms=60, dims=(10.0, 12.0, 14.0), seed=0, **topology):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, 90.0, 90.0, 90.0]
    return mdhelper_amd.ArrayUniverse(pos, box, **topology)


def weights_formula(p, N_p):
    return np.cos(np.pi * p * (np.arange(N_p) + 0.5) / N_p) / N_p


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


class Projection:
    """Stands in for ``_core.ChainProjectionEngine``: records what it is fed."""
    made = []

    def __init__(self, n_chains, n_monomers, weights, *, dev=0, timing=False):
        self.n_chains, self.n_monomers = [int(x) for x in n_chains], [int(x) for x in n_monomers]
        self.weights = [np.array(w) for w in weights]
        self.n_rows = len(self.weights[0])
        self.n_series = self.n_rows * sum(self.n_chains)
        self.frames, self.calls, self.log = 0, [], []
        self.grouping = self.unwrap = self.reserved = None
        self.closed = False
        Projection.made.append(self)

    def set_grouping(self, offsets, masses):
        self.log.append("set_grouping")
        self.grouping = (np.asarray(offsets), np.asarray(masses))

    def set_unwrap(self, dims, start=None):
        self.log.append("set_unwrap")
        self.unwrap = (np.asarray(dims), np.asarray(start))

    def reserve(self, n_frames):
        self.reserved = n_frames

    def accumulate(self, pos):
        self.log.append("accumulate")
        self.calls.append(np.array(pos))
        self.frames += len(pos)

    def result(self):
        assert not self.closed
        return np.random.default_rng(5).normal(size=(self.frames, self.n_series, 3))

    def device_result(self):
        assert not self.closed
        return "amplitudes in HBM", self.frames, self.n_series

    def close(self):
        self.closed = True


class Correlator:
    """Stands in for ``_core.MsdEngine``: records the pushes; its ACF encodes (group, block, lag)."""
    made = []

    def __init__(self, n_frames_block, n_blocks, n_groups, *, dev=0, timing=False):
        self.shape = (n_groups, n_blocks, n_frames_block)
        self.pushes, self.closed = [], False
        Correlator.made.append(self)

    def push_device(self, group, d_pos, n_total, first, count, zero_dims=0):
        assert not Projection.made[-1].closed        # the amplitudes are read where they lie
        self.pushes.append((group, d_pos, n_total, first, count, zero_dims))

    def result_acf(self):
        G, B, T = self.shape
        g, b, m = np.ogrid[:G, :B, :T]
        return (1.0 + g + 0.25 * b) * (T - m) * 0.5 ** m

    def close(self):
        self.closed = True


@pytest.fixture
def recorders(monkeypatch):
    Projection.made, Correlator.made = [], []
    monkeypatch.setattr(_core, "ChainProjectionEngine", Projection)
    monkeypatch.setattr(_core, "MsdEngine", Correlator)
    return Projection, Correlator


# ---------------------------------------------------------------- arguments

def test_argument_errors():
    u = _universe()
    kw = {"n_chains": 6, "n_monomers": 10, "verbose": False}
    with pytest.raises(ValueError, match="1 <= p <= n_monomers - 1 = 9"):
        RouseModes(u.atoms, modes=[0, 1], **kw)                     # p = 0: the centre of geometry
    with pytest.raises(ValueError, match="1 <= p <= n_monomers - 1 = 9"):
        RouseModes(u.atoms, modes=[1, 10], **kw)                    # p = N_p
    with pytest.raises(ValueError, match="1 <= p <= n_monomers - 1 = 9"):
        RouseModes(u.atoms, modes=10, **kw)
    with pytest.raises(ValueError, match="1 <= p"):
        RouseModes(u.atoms, modes=0, **kw)
    with pytest.raises(ValueError, match="distinct"):
        RouseModes(u.atoms, modes=[1, 3, 3], **kw)
    with pytest.raises(ValueError, match="sequence of ints"):
        RouseModes(u.atoms, modes=[1.5], **kw)
    # the shortest chain of all groups bounds p
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    with pytest.raises(ValueError, match="n_monomers - 1 = 3"):
        RouseModes([a, b], n_chains=(5, 4), n_monomers=(4, 10), modes=4, verbose=False)
    RouseModes([a, b], n_chains=(5, 4), n_monomers=(4, 10), modes=3, verbose=False)
    with pytest.raises(ValueError, match="No system dimensions found"):
        RouseModes(_universe(dims=None).atoms, unwrap=True, **kw)
    with pytest.raises(ValueError, match="unwrap cannot be combined with more than one rank"):
        RouseModes(u.atoms, unwrap=True, comm=TwoRanks(0), **kw)
    with pytest.raises(ValueError, match="Group 0 holds 60 atoms, which do not form n_chains"):
        RouseModes(u.atoms, n_chains=7, n_monomers=10, verbose=False)
    with pytest.raises(ValueError, match="Group 1 holds 40 atoms"):
        RouseModes([a, b], "residues", (2, 3), (5, 9), verbose=False)
    with pytest.raises(ValueError, match="Invalid grouping 'segments'"):
        RouseModes(u.atoms, "segments", 6, 10)
    RouseModes(_universe(dims=None).atoms, **kw)                    # no box needed without unwrap
    RouseModes(u.atoms, comm=TwoRanks(1), **kw)


def test_more_series_groups_than_the_correlation_engine_has():
    big = _universe(n_frames=1, n_atoms=4100)
    with pytest.raises(ValueError, match=r"n_groups \* len\(modes\) = 4097 exceeds the 4096 groups"):
        RouseModes(big.atoms, n_chains=1, n_monomers=4100, modes=4097, verbose=False)
    r = RouseModes(big.atoms, n_chains=1, n_monomers=4100, modes=4096, verbose=False)
    np.testing.assert_array_equal(r._modes, np.arange(1, 4097))
    halves = [big.select(np.arange(2050)), big.select(np.arange(2050, 4100))]
    with pytest.raises(ValueError, match=r"= 4098 exceeds the 4096 groups"):
        RouseModes(halves, n_chains=1, n_monomers=2050, modes=2049, verbose=False)
    RouseModes(halves, n_chains=1, n_monomers=2050, modes=2048, verbose=False)


def test_relaxation_times_need_a_run(recorders):
    u = _universe()
    r = RouseModes(u.atoms, n_chains=6, n_monomers=10, verbose=False)
    with pytest.raises(RuntimeError, match="Call RouseModes.run"):
        r.calculate_relaxation_times()


# ---------------------------------------------------------------- weights

def test_weights_reach_the_engine(recorders):
    u = _universe()
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    r = RouseModes([a, b], n_chains=(5, 4), n_monomers=(4, 10), modes=[3, 1], dt=2.0, verbose=False).run(step=2)
    eng = recorders[0].made[0]
    assert (eng.n_chains, eng.n_monomers) == ([5, 4], [4, 10])
    assert [w.shape for w in eng.weights] == [(2, 4), (2, 10)]
    for w, N_p in zip(eng.weights, (4, 10)):
        assert w.dtype == np.float64
        for row, p in zip(w, (3, 1)):
            np.testing.assert_array_equal(row, weights_formula(p, N_p))
    assert eng.reserved == 3 and eng.frames == 3 and eng.closed
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(0, 6, 2)))
    np.testing.assert_array_equal(r.results.modes, [3, 1])
    np.testing.assert_array_equal(r.results.times, [0.0, 4.0, 8.0])
    assert r.results.units == {"results.times": "picosecond", "results.amplitudes": "angstrom^2"}


@pytest.mark.parametrize("N_p", [2, 33, 64])
def test_weights_are_the_orthogonal_dct(recorders, N_p):
    """DCT-II rows: sum_n cos(p pi (n + 1/2) / N) cos(q pi (n + 1/2) / N) = (N / 2) delta_pq for 1 <= p, q < N."""
    u = _universe(n_frames=1, n_atoms=2 * N_p)
    RouseModes(u.atoms, n_chains=2, n_monomers=N_p, modes=N_p - 1, verbose=False).run()
    (W,) = recorders[0].made[0].weights
    assert W.shape == (N_p - 1, N_p)
    np.testing.assert_allclose(W @ W.T * N_p, 0.5 * np.eye(N_p - 1), rtol=0, atol=1e-14)


# ---------------------------------------------------------------- correlation

def test_pushes_address_one_contiguous_range_per_group_and_mode(recorders):
    u = _universe(n_frames=9)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    n_chains, P = (5, 4), 3
    with pytest.warns(UserWarning, match="last 1 frame"):
        r = RouseModes([a, b], n_chains=n_chains, n_monomers=(4, 10), modes=P, n_blocks=2, verbose=False).run()
    proj, corr = recorders[0].made[0], recorders[1].made[0]
    assert corr.shape == (2 * P, 2, 4) and corr.closed and proj.closed and proj.frames == 9
    S = P * sum(n_chains)
    series0 = [0, P * 5]
    want = [(g * P + k, "amplitudes in HBM", S, series0[g] + k * M, M, 0)
            for g, M in enumerate(n_chains) for k in range(P)]
    assert sorted(corr.pushes) == sorted(want)
    # results: lag m normalised by M (T_b - m), the ACF by its lag-0 value
    raw = corr.result_acf().reshape(2, P, 2, 4)
    for g, M in enumerate(n_chains):
        norm = np.swapaxes(raw[g], 0, 1) / (4 - np.arange(4)) / M
        np.testing.assert_allclose(r.results.amplitudes[g], norm[..., 0], rtol=1e-15)
        np.testing.assert_allclose(r.results.acf[g], norm / norm[..., :1], rtol=1e-15)
    assert r.results.amplitudes.shape == (2, 2, P) and r.results.acf.shape == (2, 2, P, 4)
    np.testing.assert_array_equal(r.results.acf[..., 0], 1.0)
    r.calculate_relaxation_times()
    assert r.results.relaxation_times.shape == (2, 2, P)
    assert r.results.units["results.relaxation_times"] == "picosecond"
    # C(m) = 2^-m: tau = 1 / ln 2 frames, beta = 1
    np.testing.assert_allclose(r.results.relaxation_times, 1 / np.log(2), rtol=1e-5)


def test_two_ranks_cover_every_chain_once(recorders):
    u = _universe(n_frames=8)
    a, b = u.select(np.arange(21)), u.select(np.arange(21, 60))
    n_chains, n_monomers, P = (7, 3), (3, 13), 2
    S, series0 = P * 10, [0, P * 7]
    covered = np.zeros(S, dtype=int)
    for rank in (0, 1):
        comm = TwoRanks(rank)
        r = RouseModes([a, b], n_chains=n_chains, n_monomers=n_monomers, modes=P, verbose=False, comm=comm).run()
        proj, corr = recorders[0].made[rank], recorders[1].made[rank]
        assert proj.frames == 8                          # every rank projects all frames
        for g, M in enumerate(n_chains):
            lo, hi = shard_range(M, rank, 2)
            for k in range(P):
                assert (g * P + k, "amplitudes in HBM", S, series0[g] + k * M + lo, hi - lo, 0) in corr.pushes
        assert len(corr.pushes) == 2 * P
        for group, _, n_total, first, count, _ in corr.pushes:
            g, k = divmod(group, P)
            assert series0[g] + k * n_chains[g] <= first and first + count <= series0[g] + (k + 1) * n_chains[g]
            covered[first:first + count] += 1
        (sent,) = comm.reduced                           # one all-reduce of the accumulators
        np.testing.assert_array_equal(sent, corr.result_acf())
        np.testing.assert_allclose(r.results.acf[..., 0], 1.0, rtol=1e-15)
    np.testing.assert_array_equal(covered, 1)


def test_direct_windows_on_the_host_copy(recorders):
    u = _universe(n_frames=8)
    r = RouseModes(u.atoms, n_chains=6, n_monomers=10, modes=[2, 5], n_blocks=2, fft=False, verbose=False).run()
    proj = recorders[0].made[0]
    assert proj.closed and recorders[1].made == []
    X = np.random.default_rng(5).normal(size=(8, 12, 3))            # what the recorder's result() returns
    for k in range(2):
        raw = polymer.correlation_shift(X[:, 6 * k:6 * k + 6].reshape(2, 4, 6, 3), average=True, vector=True)
        np.testing.assert_array_equal(r.results.amplitudes[0, :, k], raw[:, 0])
        np.testing.assert_array_equal(r.results.acf[0, :, k], raw / raw[:, :1])


def test_residues_and_unwrap_reach_the_projection_engine(recorders):
    L = np.array([10.0, 12.0, 14.0])
    rng = np.random.default_rng(3)
    M, N_p, size, F = 3, 4, 2, 3
    steps = rng.normal(size=(F, M, N_p * size, 3))
    steps *= 0.7 / np.linalg.norm(steps, axis=-1, keepdims=True)
    pos = np.mod(rng.random((F, M, 1, 3)) * L + np.cumsum(steps, axis=2), L).reshape(F, -1, 3).astype(np.float32)
    masses = rng.uniform(1, 5, M * N_p * size)
    u = mdhelper_amd.ArrayUniverse(pos, [*L, 90.0, 90.0, 90.0], masses=masses)
    RouseModes(u.atoms, "residues", M, N_p, modes=2, unwrap=True, verbose=False).run(start=1)
    eng = recorders[0].made[0]
    assert eng.log == ["set_grouping", "set_unwrap", "accumulate"]
    np.testing.assert_array_equal(eng.grouping[0], size * np.arange(M * N_p + 1))
    np.testing.assert_array_equal(eng.grouping[1], masses)
    dims, start = eng.unwrap
    np.testing.assert_array_equal(dims, L)
    assert start.shape == (M * N_p, 3) and start.dtype == np.float64


# ---------------------------------------------------------------- Gyradius after the refactor

class GyrationRecorder(Projection):
    def __init__(self, n_chains, n_monomers, masses, *, dev=0, timing=False):
        self.n_chains, self.n_monomers = [int(x) for x in n_chains], [int(x) for x in n_monomers]
        self.masses = np.array(masses)
        self.frames, self.calls, self.log = 0, [], []
        self.grouping = self.unwrap = None
        self.closed = False
        Projection.made.append(self)

    def result(self):
        return np.zeros((len(self.n_chains), self.frames, 4))


def test_gyradius_hands_its_engine_the_same_calls(monkeypatch):
    """The calls ``Gyradius`` made before its selection, unwrap start and frame feed moved into
    ``_PolymerAnalysisBase``, restated here: engine(n_chains, n_monomers, monomer masses), the grouping as CSR
    offsets over all groups with the atom masses, the unwrap start from ``unwrap_edge`` on the monomer centres of
    the first analysed frame, then the frames in concatenated-group order."""
    Projection.made = []
    monkeypatch.setattr(_core, "GyrationEngine", GyrationRecorder)
    L = np.array([10.0, 12.0, 14.0])
    rng = np.random.default_rng(7)
    pos = (rng.random((5, 60, 3)) * L).astype(np.float32)
    masses = np.tile([12.0, 1.0, 3.0], 20)
    u = mdhelper_amd.ArrayUniverse(pos, [*L, 90.0, 90.0, 90.0], masses=masses)
    beads, atomistic = u.select(np.arange(48, 60)), u.select(np.arange(48))
    g = Gyradius([beads, atomistic], ("atoms", "residues"), (3, 2), (4, 8), unwrap=True, components=True,
                 verbose=False).run(start=2)
    eng = Projection.made[0]
    assert eng.log == ["set_grouping", "set_unwrap", "accumulate"] and eng.closed
    assert (eng.n_chains, eng.n_monomers) == ([3, 2], [4, 8])
    np.testing.assert_array_equal(eng.masses, np.concatenate((masses[48:], np.full(16, 16.0))))
    np.testing.assert_array_equal(eng.grouping[0], np.concatenate((np.arange(12), 12 + 3 * np.arange(17))))
    np.testing.assert_array_equal(eng.grouping[1], np.concatenate((masses[48:], masses[:48])))
    order = np.r_[48:60, 0:48]
    np.testing.assert_array_equal(eng.calls[0], pos[2:, order])
    # the start: frame 2, beads as they are, monomers of 3 atoms as centres of mass, chains made whole
    x = pos[2].astype(float)
    centres = np.add.reduceat(x[:48] * masses[:48, None], 3 * np.arange(16), axis=0) / 16.0
    want = []
    for points, pm, M, N_p in ((x[48:], masses[48:], 3, 4), (centres, np.full(16, 16.0), 2, 8)):
        bonds = (np.arange(M)[:, None] * N_p + np.arange(N_p - 1)[None, :]).ravel()
        want.append(unwrap_edge(positions=points, bonds=np.stack((bonds, bonds + 1), axis=1), dimensions=L,
                                masses=pm))
    dims, start = eng.unwrap
    np.testing.assert_array_equal(dims, L)
    np.testing.assert_array_equal(start, np.concatenate(want))
    assert g.results.gyradii.shape == (2, 3, 3)
    np.testing.assert_array_equal(g._Ns, [12, 16])
    assert g._slices == [slice(0, 12), slice(12, 28)] and g._components is True


def test_no_cpu_fallback():
    """Without a HIP device the class and the engine raise; nothing projects the chains on the host instead."""
    from mdhelper_amd import _lib
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            RouseModes(u.atoms, n_chains=6, n_monomers=10, verbose=False).run()
        with pytest.raises(RuntimeError):
            _core.ChainProjectionEngine([6], [10], [np.ones((2, 10))])
    assert _core.RouseEngine is _core.ChainProjectionEngine and polymer.RouseModes is RouseModes


def test_engine_argument_errors_need_no_device():
    import ctypes
    from mdhelper_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)         # noqa: E731
    w = np.ones(6)
    for n_chains, n_monomers, K, weights, word in ((i64(0), i64(3), 2, w, b"n_chains"),
                                                   (i64(1), i64(0), 2, w, b"n_monomers"),
                                                   (i64(1), i64(3), 0, w, b"n_rows"),
                                                   (i64(1), i64(3), 2, np.array([1, 2, np.inf, 4, 5, 6.0]), b"finite"),
                                                   (i64(1), i64(3), 2, np.array([1, 2, 3, 4, np.nan, 6.0]), b"finite"),
                                                   (i64(1 << 20), i64(1 << 20), 1, w, b"2^31 / 3 points"),
                                                   (i64(1 << 20), i64(1), 1 << 10, w, b"series")):
        rc = lib.mdx_rouse_create(ctypes.byref(h), 0, 1, p(n_chains), p(n_monomers), K, p(weights))
        assert rc == -1 and word in lib.mdx_last_error(), (word, lib.mdx_last_error())
    with pytest.raises(ValueError, match="one entry per group"):
        _core.ChainProjectionEngine([2, 1], [3], [np.ones((1, 3))])
    with pytest.raises(ValueError, match=r"one array \[n_rows, n_monomers\] per group"):
        _core.ChainProjectionEngine([2], [3], [np.ones((1, 4))])
    with pytest.raises(ValueError, match=r"one array \[n_rows, n_monomers\] per group"):
        _core.ChainProjectionEngine([2, 2], [3, 3], [np.ones((1, 3)), np.ones((2, 3))])
