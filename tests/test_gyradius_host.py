"""
Host-side checks of the radius of gyration that need no GPU: ``algorithm.molecule.radius_of_gyration`` against
outputs of the reference's function (``tests/golden/gyradius_ref.npz``, written by
``scripts/make_golden_gyradius.py``), the argument handling of ``analysis.polymer.Gyradius`` and what it hands to the
engine (a recorder stands in for ``_core.GyrationEngine``, which is only created in ``_prepare``).

Tolerance against the reference.  Both sides form, per chain, float64 sums of at most N_p terms: the centre (N_p
products, one division) and, after centring, N_p non-negative terms m (x - c)^2 per axis.  A sum of n non-negative
terms carries a relative error of at most ~n 2^-53 whatever its order, the centring, the square, the product with
the mass, the division and the square root add a few roundings each, and the centre's own error enters only in second
order (sum m (x - c) = 0): about (N_p + 8) 2^-53 per side, 2 (N_p + 8) 2^-53 between the two, which is under 3e-14
for the largest golden case (N_p = 130).  rtol = 1e-11 is ~350 times above that bound and ~200 times below the 2e-9
that the one-pass formula sum m x^2 - (sum m x)^2 / sum m loses on the chains 9 000 A from the origin.  A chain of one
point has Rg = 0 up to the rounding of m x / m: there atol = 8 2^-53 max|r| applies.
"""
import pathlib

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.algorithm.molecule import radius_of_gyration
from mdhelper_amd.analysis import Gyradius
from mdhelper_amd.analysis import polymer

RTOL = 1e-11


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(golden_dir / "gyradius_ref.npz")


def test_fixture_covers_the_cases(ref):
    shapes = {tuple(ref[f"pos_{name}"].shape[:2]) for name in ref["cases"]}
    assert shapes == {(5, 2), (7, 63), (4, 64), (4, 65), (3, 130)}
    assert len(ref["cases"]) == 6
    assert ref["pos_far"].dtype == np.float32 and ref["pos_far"].min() > 8000.0
    assert ref["out_far_rg"].max() < 100.0                  # chains of 130 bonds of 1.5 A, far from the origin


@pytest.mark.parametrize("name", ["m5_n2", "m7_n63", "m4_n64", "m4_n65", "m3_n130", "far"])
@pytest.mark.parametrize("components", [False, True])
def test_grouped_arrays_against_the_reference(ref, name, components):
    pos, masses = ref[f"pos_{name}"], ref[f"masses_{name}"]
    want = ref[f"out_{name}_{'xyz' if components else 'rg'}"]
    got = radius_of_gyration(grouping="segments", positions=pos, masses=masses, components=components)
    assert got.shape == want.shape == ((len(pos), 3) if components else (len(pos),))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    # the shape decides, whatever `grouping` says; flat arrays with n_groups are reshaped
    np.testing.assert_array_equal(radius_of_gyration(positions=pos, masses=masses, components=components), got)
    np.testing.assert_array_equal(
        radius_of_gyration(positions=pos.reshape(-1, 3), masses=masses.ravel(), n_groups=len(pos),
                           components=components), got)


def test_ungrouped_and_ragged_forms_against_the_reference(ref):
    pos, masses = ref["pos_m7_n63"][2], ref["masses_m7_n63"][2]
    got = radius_of_gyration(positions=pos, masses=masses)
    assert np.ndim(got) == 0
    np.testing.assert_allclose(got, ref["out_single_rg"], rtol=RTOL, atol=0)
    got = radius_of_gyration(positions=pos, masses=masses, components=True)
    assert got.shape == (3,)
    np.testing.assert_allclose(got, ref["out_single_xyz"], rtol=RTOL, atol=0)
    lengths = ref["ragged_lengths"]
    assert 1 in lengths and len(set(lengths)) == len(lengths)
    rp = [p[:n] for p, n in zip(ref["pos_m4_n65"], lengths)]
    rm = [m[:n] for m, n in zip(ref["masses_m4_n65"], lengths)]
    atol = 8 * 2.0 ** -53 * np.abs(ref["pos_m4_n65"]).max()            # the chain of one point
    got = radius_of_gyration(positions=rp, masses=rm)
    assert got.shape == (4,)
    np.testing.assert_allclose(got, ref["out_ragged_rg"], rtol=RTOL, atol=atol)
    got = radius_of_gyration(positions=rp, masses=rm, components=True)
    assert got.shape == (4, 3)
    np.testing.assert_allclose(got, ref["out_ragged_xyz"], rtol=RTOL, atol=atol)


def test_components_are_the_radii_around_the_axes(ref):
    pos, masses = ref["pos_m4_n65"], ref["masses_m4_n65"]
    rg = radius_of_gyration(positions=pos, masses=masses)
    xyz = radius_of_gyration(positions=pos, masses=masses, components=True)
    # Rg_x^2 + Rg_y^2 + Rg_z^2 = 2 Rg^2
    np.testing.assert_allclose((xyz ** 2).sum(axis=1), 2 * rg ** 2, rtol=1e-13)
    x = pos.astype(float)
    c = (masses[:, :, None] * x).sum(axis=1) / masses.sum(axis=1)[:, None]
    want_x = np.sqrt((masses * ((x - c[:, None]) ** 2)[:, :, 1:].sum(axis=2)).sum(axis=1) / masses.sum(axis=1))
    np.testing.assert_allclose(xyz[:, 0], want_x, rtol=1e-13)


def test_group_forms(ref):
    pos, masses = ref["pos_m4_n65"], ref["masses_m4_n65"]
    flat, m = pos.reshape(1, -1, 3), masses.ravel()
    u = mdhelper_amd.ArrayUniverse(flat, [500.0] * 3 + [90.0] * 3, masses=m, segids=np.repeat(np.arange(4), 65),
                                   resids=np.arange(260) // 5)
    want = radius_of_gyration(positions=pos, masses=masses)
    np.testing.assert_array_equal(radius_of_gyration(u.atoms, "segments"), want)
    np.testing.assert_array_equal(radius_of_gyration(u.atoms, n_groups=4), want)
    np.testing.assert_array_equal(radius_of_gyration(u.atoms, "segments", components=True),
                                  radius_of_gyration(positions=pos, masses=masses, components=True))
    res = radius_of_gyration(u.atoms, "residues")
    assert res.shape == (52,)
    np.testing.assert_array_equal(res, radius_of_gyration(positions=flat.reshape(52, 5, 3), masses=m.reshape(52, 5)))
    whole = radius_of_gyration(u.atoms)
    assert np.ndim(whole) == 0
    np.testing.assert_array_equal(whole, radius_of_gyration(positions=flat[0], masses=m))
    # segments of different sizes come back as one radius each, gathered by their indices
    segids = np.concatenate((np.zeros(100, dtype=int), np.ones(160, dtype=int)))
    order = np.random.default_rng(1).permutation(260)
    u2 = mdhelper_amd.ArrayUniverse(flat[:, order], [500.0] * 3 + [90.0] * 3, masses=m[order], segids=segids[order])
    got = radius_of_gyration(u2.atoms, "segments")
    want = [radius_of_gyration(positions=flat[0, lo:hi], masses=m[lo:hi]) for lo, hi in ((0, 100), (100, 260))]
    np.testing.assert_allclose(got, want, rtol=1e-13)
    # image flags unwrap the positions of the group with the box of the universe
    images = np.zeros((260, 3), dtype=int)
    images[:65] = (1, 0, -2)
    shifted = flat[0].astype(float) + images * 500.0
    np.testing.assert_array_equal(radius_of_gyration(u.atoms, "segments", images=images),
                                  radius_of_gyration(positions=shifted.reshape(4, 65, 3), masses=masses))


def test_function_errors():
    with pytest.raises(ValueError, match="Invalid grouping: 'atoms'"):
        radius_of_gyration(grouping="atoms", positions=np.zeros((4, 3)), masses=np.ones(4))
    with pytest.raises(ValueError, match="Either a group of atoms or atom positions and masses"):
        radius_of_gyration(positions=np.zeros((4, 3)))
    with pytest.raises(ValueError, match="incompatible"):
        radius_of_gyration(positions=np.zeros((4, 3)), masses=np.ones(5))


# ---------------------------------------------------------------- the class

def _universe(n_frames=5, n_atoms=60, dims=(10.0, 12.0, 14.0), **topology):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, 90.0, 90.0, 90.0]
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


def test_constructor_validation():
    u = _universe()
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    with pytest.raises(ValueError, match="Invalid grouping 'segments'"):
        Gyradius(u.atoms, "segments", 6, 10)
    with pytest.raises(ValueError, match="number of grouping values"):
        Gyradius([a, b], ["atoms"], (2, 4), (10, 10))
    with pytest.raises(ValueError, match="Invalid grouping 'x'"):
        Gyradius([a, b], ["atoms", "x"], (2, 4), (10, 10))
    with pytest.raises(ValueError, match="number of polymer counts"):
        Gyradius([a, b], "atoms", (2, 4, 1), (10, 10))
    with pytest.raises(ValueError, match="number of chain lengths"):
        Gyradius([a, b], "atoms", (2, 4), (10, 10, 10))
    with pytest.raises(ValueError, match="Group 0 holds 60 atoms, which do not form n_chains"):
        Gyradius(u.atoms, "atoms", 7, 10)
    with pytest.raises(ValueError, match="Group 1 holds 40 atoms"):
        Gyradius([a, b], "residues", (2, 3), (5, 9))
    with pytest.raises(ValueError, match="No system dimensions found"):
        Gyradius(_universe(dims=None).atoms, n_chains=6, n_monomers=10, unwrap=True)
    with pytest.raises(ValueError, match="unwrap cannot be combined with more than one rank"):
        Gyradius(u.atoms, n_chains=6, n_monomers=10, unwrap=True, comm=TwoRanks(0))
    Gyradius(_universe(dims=None).atoms, n_chains=6, n_monomers=10)     # no box needed without unwrap
    Gyradius(u.atoms, n_chains=6, n_monomers=10, comm=TwoRanks(1))      # frames shard without unwrap


def test_chain_counts_from_arguments_and_topology():
    u = _universe()
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    g = Gyradius([a, b], "atoms", (2, 4), 10, components=True, parallel=True, verbose=False)
    np.testing.assert_array_equal(g._n_chains, [2, 4])
    np.testing.assert_array_equal(g._n_monomers, [10, 10])             # a scalar gives one entry per group
    np.testing.assert_array_equal(g._Ns, [20, 40])
    assert g._slices == [slice(0, 20), slice(20, 60)] and g._components is True
    # read from the topology: chains are segments; monomers are atoms, or residues per segment
    ut = _universe(segids=np.repeat(np.arange(4), 15), resids=np.arange(60) // 3,
                   masses=np.tile([12.0, 1.0, 1.0], 20))
    g = Gyradius(ut.atoms, verbose=False)
    assert (g._n_chains[0], g._n_monomers[0]) == (4, 15)
    g = Gyradius(ut.atoms, "residues", verbose=False)
    assert (g._n_chains[0], g._n_monomers[0]) == (4, 5)
    uneven = _universe(segids=np.concatenate((np.zeros(24, dtype=int), np.ones(36, dtype=int))),
                       resids=np.arange(60) // 3)
    with pytest.raises(ValueError, match="same number of atoms"):
        Gyradius(uneven.atoms, verbose=False)
    with pytest.raises(ValueError, match="same number of residues"):
        Gyradius(uneven.atoms, "residues", verbose=False)


class Recorder:
    """Stands in for ``_core.GyrationEngine``: records what it is fed; its rows encode (group, frame, value)."""
    made = []

    def __init__(self, n_chains, n_monomers, masses, *, dev=0, timing=False):
        self.n_chains, self.n_monomers = list(n_chains), list(n_monomers)
        self.masses = np.array(masses)
        self.frames, self.calls = 0, []
        self.grouping = self.unwrap = None
        self.closed = False
        Recorder.made.append(self)

    def set_grouping(self, offsets, masses):
        self.grouping = (np.asarray(offsets), np.asarray(masses))

    def set_unwrap(self, dims, start=None):
        self.unwrap = (np.asarray(dims), np.asarray(start))

    def accumulate(self, pos):
        self.calls.append(np.array(pos))
        self.frames += len(pos)

    def result(self):
        g = np.arange(len(self.n_chains))[:, None, None]
        f = np.arange(self.frames)[None, :, None]
        k = np.arange(4)[None, None, :]
        return (100.0 * (g + 1) + f + 0.125 * k).astype(np.float64)

    def close(self):
        self.closed = True


@pytest.fixture
def recorder(monkeypatch):
    Recorder.made = []
    monkeypatch.setattr(_core, "GyrationEngine", Recorder)
    return Recorder


def test_results_units_and_layout(recorder):
    u = _universe(n_frames=7)
    a, b = u.select(np.arange(20, 60)), u.select(np.arange(20))
    g = Gyradius([a, b], n_chains=(4, 2), n_monomers=(10, 10), verbose=False).run()
    eng = recorder.made[0]
    assert eng.closed and eng.frames == 7 and eng.grouping is None and eng.unwrap is None
    assert (eng.n_chains, eng.n_monomers) == ([4, 2], [10, 10])
    # rows in concatenated-group order
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(7))[:, np.r_[20:60, 0:20]])
    assert g.results.units == {"results.gyradii": "angstrom"}
    assert g.results.gyradii.shape == (2, 7)
    np.testing.assert_array_equal(g.results.gyradii, eng.result()[..., 0])
    g = Gyradius([a, b], n_chains=(4, 2), n_monomers=(10, 10), components=True, parallel=True,
                 verbose=False).run(step=2)
    assert g.results.gyradii.shape == (2, 4, 3)                        # the serial layout, whatever `parallel`
    np.testing.assert_array_equal(g.results.gyradii, recorder.made[1].result()[..., 1:])
    np.testing.assert_array_equal(recorder.made[1].calls[0],
                                  u.trajectory.frame_block(np.arange(0, 7, 2))[:, np.r_[20:60, 0:20]])
    np.testing.assert_array_equal(g.frames, [0, 2, 4, 6])


def test_monomer_masses_and_grouping_reach_the_engine(recorder):
    masses = np.tile([12.0, 1.0, 3.0], 20)
    u = _universe(masses=masses)
    beads, atomistic = u.select(np.arange(12)), u.select(np.arange(12, 60))
    # 48 atoms = 2 chains x 8 monomers x 3 atoms
    Gyradius([beads, atomistic], ("atoms", "residues"), (3, 2), (4, 8), verbose=False).run()
    eng = recorder.made[0]
    np.testing.assert_array_equal(eng.masses, np.concatenate((masses[:12], np.full(16, 16.0))))
    offsets, m = eng.grouping
    np.testing.assert_array_equal(offsets, np.concatenate((np.arange(12), 12 + 3 * np.arange(17))))
    np.testing.assert_array_equal(m, masses)
    # residues of the topology, in any atom order: rows sorted monomer by monomer
    order = np.random.default_rng(2).permutation(60)
    resids, segids = (np.arange(60) // 3)[order], (np.arange(60) // 15)[order]
    ut = _universe(masses=masses[order], resids=resids, segids=segids)
    Gyradius(ut.atoms, "residues", verbose=False).run()
    eng = recorder.made[1]
    assert (eng.n_chains, eng.n_monomers) == ([4], [5])
    np.testing.assert_array_equal(eng.grouping[0], 3 * np.arange(21))
    fed = eng.calls[0][0]
    want_rows = np.argsort(resids, kind="stable")
    np.testing.assert_array_equal(fed, ut.trajectory.frame_block(np.arange(1))[0][want_rows])
    np.testing.assert_array_equal(eng.masses, np.full(20, 16.0))


def test_unwrap_start_makes_the_chains_of_the_first_analysed_frame_whole(recorder):
    L = np.array([10.0, 12.0, 14.0])
    rng = np.random.default_rng(3)
    M, N_p, F = 3, 8, 4
    steps = rng.normal(size=(F, M, N_p, 3))
    steps *= 1.0 / np.linalg.norm(steps, axis=-1, keepdims=True)
    whole = rng.random((F, M, 1, 3)) * L + np.cumsum(steps, axis=2)        # chains that leave the box
    pos = np.mod(whole, L).reshape(F, M * N_p, 3).astype(np.float32)
    assert np.any(np.abs(np.diff(pos.reshape(F, M, N_p, 3), axis=2)) > L / 2)      # some chains straddle a face
    u = mdhelper_amd.ArrayUniverse(pos, [*L, 90.0, 90.0, 90.0], masses=rng.uniform(1, 5, M * N_p))
    Gyradius(u.atoms, n_chains=M, n_monomers=N_p, unwrap=True, verbose=False).run(start=1)
    dims, start = recorder.made[0].unwrap
    np.testing.assert_array_equal(dims, L)
    assert start.shape == (M * N_p, 3) and start.dtype == np.float64
    # frame 1, every bond at its minimum image, each monomer an image of the stored one
    bonds = np.diff(start.reshape(M, N_p, 3), axis=1)
    np.testing.assert_allclose(np.linalg.norm(bonds, axis=-1), 1.0, atol=2e-5)
    shift = (start - pos[1]) / L
    np.testing.assert_allclose(shift, np.round(shift), atol=1e-12)
    assert np.any(np.round(shift) != 0)


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_shard_frames_and_allreduce(recorder, rank):
    u = _universe(n_frames=7)
    comm = TwoRanks(rank)
    g = Gyradius(u.atoms, n_chains=6, n_monomers=10, components=True, verbose=False, comm=comm).run()
    eng = recorder.made[0]
    lo, hi = ((0, 4), (4, 7))[rank]
    assert eng.frames == hi - lo
    np.testing.assert_array_equal(eng.calls[0], u.trajectory.frame_block(np.arange(lo, hi)))
    # this rank's rows sit inside a zero-filled array over all frames before the sum
    (sent,) = comm.reduced
    assert sent.shape == (1, 7, 3)
    assert np.all(sent[:, :lo] == 0) and np.all(sent[:, hi:] == 0)
    np.testing.assert_array_equal(sent[:, lo:hi], eng.result()[..., 1:])
    np.testing.assert_array_equal(g.results.gyradii, 2 * sent)


def test_no_cpu_fallback():
    """Without a HIP device the class and the engine raise; nothing computes the radii on the host instead."""
    from mdhelper_amd import _lib
    if _lib.device_count() == 0:
        u = _universe()
        with pytest.raises(RuntimeError):
            Gyradius(u.atoms, n_chains=6, n_monomers=10, verbose=False).run()
        with pytest.raises(RuntimeError):
            _core.GyrationEngine([6], [10], np.ones(60))
    text = (pathlib.Path(polymer.__file__)).read_text()
    body = text[text.index("class Gyradius"):text.index("class EndToEndVector")]
    assert "radius_of_gyration" not in body and "_core.GyrationEngine" in body


def test_engine_argument_errors_need_no_device():
    import ctypes
    from mdhelper_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    one = np.array([1], dtype=np.int64)
    masses = np.array([1.0, 0.0])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for n_chains, n_monomers, m, word in ((np.array([0]), one, masses, b"n_chains"),
                                          (one, np.array([0]), masses, b"n_monomers"),
                                          (one, np.array([2]), np.array([1.0, -1.0]), b"masses"),
                                          (one, np.array([2]), np.array([0.0, 0.0]), b"no mass")):
        rc = lib.mdx_gyr_create(ctypes.byref(h), 0, 1, p(n_chains.astype(np.int64)), p(n_monomers.astype(np.int64)),
                                p(m))
        assert rc == -1 and word in lib.mdx_last_error()
    with pytest.raises(ValueError, match="one entry per point"):
        _core.GyrationEngine([2], [3], np.ones(5))
    with pytest.raises(ValueError, match="one entry per group"):
        _core.GyrationEngine([2, 1], [3], np.ones(6))
    assert polymer.Gyradius is Gyradius
