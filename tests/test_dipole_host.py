"""
Host-side checks of the dipole-moment analysis that need no GPU: ``calculate_relative_permittivity`` against outputs
of the reference's function (``tests/golden/permittivity_ref.npz``, written by ``scripts/make_golden_permittivity.py``),
the argument handling of ``analysis.electrostatics.DipoleMoment``, the effective charges of ``neutralize`` and the
errors of its ``calculate_relative_permittivity``.

The reduced branch is the same NumPy expression on both sides, hence rtol = 1e-14.  The non-reduced branch of the
reference multiplies its arguments by pint units; pint is not installed where the golden file is written, so that
branch is NOT pinned by the reference: it is compared with the closed form
``1 + e^2 / (eps0 k_B 1e-10 m) * fluctuation / (V T)`` built from the CODATA-2018 constants instead.
"""
import ctypes

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DipoleMoment, calculate_relative_permittivity, electrostatics


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(golden_dir / "permittivity_ref.npz")


# ---------------------------------------------------------------- the function

def test_fixture_covers_the_cases(ref):
    assert list(ref["cases"]) == ["one_frame", "short", "long", "hot"]
    assert ref["M_one_frame"].shape == (1, 3) and ref["M_long"].shape == (400, 3)
    assert ref["V_long"].std() > 0 and ref["V_hot"].shape == (1,)


@pytest.mark.parametrize("name", ["one_frame", "short", "long", "hot"])
def test_reduced_against_the_reference(ref, name):
    M, T, V = ref[f"M_{name}"], float(ref[f"T_{name}"]), ref[f"V_{name}"]
    M0, V0 = M.copy(), V.copy()
    got = calculate_relative_permittivity(M, T, V, reduced=True)
    assert isinstance(got, float)
    np.testing.assert_allclose(got, ref[f"out_{name}"], rtol=1e-14, atol=0)
    if name == "one_frame":
        assert got == 1.0
    np.testing.assert_array_equal(M, M0)               # the inputs are not modified
    np.testing.assert_array_equal(V, V0)
    # a float volume is its own mean
    np.testing.assert_allclose(calculate_relative_permittivity(M, T, float(V.mean()), reduced=True), got, rtol=1e-14)


@pytest.mark.parametrize("name", ["one_frame", "short", "long", "hot"])
def test_not_reduced_against_the_closed_form(ref, name):
    """Not pinned by the reference (its branch needs pint): the closed form from the CODATA-2018 constants."""
    M, V = ref[f"M_{name}"], ref[f"V_{name}"]
    T = 298.15
    M0, V0 = M.copy(), V.copy()
    e, eps0, kB = 1.602176634e-19, 8.8541878128e-12, 1.380649e-23
    C = e * e / (eps0 * kB * 1e-10)
    assert abs(C / 2.0998524e6 - 1) < 1e-7
    want = 1 + C * (M ** 2 - M.mean(axis=0) ** 2).mean() / (V.mean() * T)
    got = calculate_relative_permittivity(M, T, V)
    assert isinstance(got, float)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(M, M0)
    np.testing.assert_array_equal(V, V0)
    assert electrostatics.PERMITTIVITY_FACTOR == pytest.approx(C, rel=1e-15)


# ---------------------------------------------------------------- the class

def _universe(n_frames=5, n_atoms=12, dims=(10.0, 12.0, 14.0), **topology):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, 90.0, 90.0, 90.0]
    return mdhelper_amd.ArrayUniverse(pos, box, **topology)


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank


Q12 = np.tile([1.0, -1.0], 6)


def test_signature_matches_the_reference():
    import inspect
    params = list(inspect.signature(DipoleMoment.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["groups", "charges", "dimensions", "scales", "average", "reduced",
                                        "neutralize", "unwrap", "parallel", "verbose", "kwargs"]
    assert [p.default for p in params[1:-1]] == [None, None, 1, False, False, False, False, False, True]
    assert electrostatics.DipoleMoment is DipoleMoment
    assert mdhelper_amd.analysis.calculate_relative_permittivity is calculate_relative_permittivity


def test_constructor_errors():
    u = _universe(charges=Q12)
    a, b = u.select(np.arange(4)), u.select(np.arange(4, 12))
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        DipoleMoment(u.atoms, dimensions=[10.0, 10.0])
    with pytest.raises(ValueError, match="No system dimensions found or provided"):
        DipoleMoment(_universe(dims=None, charges=Q12).atoms)
    with pytest.raises(ValueError, match="scaling factor"):
        DipoleMoment(u.atoms, scales=(1, 2))
    with pytest.raises(ValueError, match="scaling factor"):
        DipoleMoment(u.atoms, scales=("a", "b", "c"))
    with pytest.raises(ValueError, match="number of group charge arrays"):
        DipoleMoment([a, b], charges=[1.0])
    with pytest.raises(ValueError, match=r"number of charges in 'charges\[1\]'"):
        DipoleMoment([a, b], charges=[1.0, np.ones(7)])
    with pytest.raises(ValueError, match="The topology has no charge information"):
        DipoleMoment(_universe().atoms)
    with pytest.raises(ValueError, match="unwrap cannot be combined with more than one rank"):
        DipoleMoment(u.atoms, unwrap=True, comm=TwoRanks(0))
    DipoleMoment(u.atoms, comm=TwoRanks(1))                      # frames shard without unwrap
    DipoleMoment(_universe(dims=None, charges=Q12).atoms, dimensions=[10.0, 10.0, 10.0])


def test_dimensions_scales_and_charge_forms():
    u = _universe(charges=Q12)
    a, b = u.select(np.arange(4)), u.select(np.arange(4, 12))
    d = DipoleMoment([a, b], scales=(1, 1, 2), verbose=False)
    np.testing.assert_array_equal(d._dimensions, [10.0, 12.0, 28.0])
    assert d._dimensions.dtype == np.float64
    np.testing.assert_array_equal(DipoleMoment(u.atoms, dimensions=[3, 4, 5], scales=0.5)._dimensions,
                                  [1.5, 2.0, 2.5])
    np.testing.assert_array_equal(d._Ns, [4, 8])
    assert d._slices == [slice(0, 4), slice(4, 12)]
    np.testing.assert_array_equal(d._effective_charges(), Q12)                  # from the universe
    d = DipoleMoment([a, b], charges=[2, np.arange(8.0)], verbose=False)
    np.testing.assert_array_equal(d._effective_charges(), np.r_[2.0, 2.0, 2.0, 2.0, np.arange(8.0)])
    # a topology without charges takes them from the argument
    d = DipoleMoment(_universe().atoms, charges=[Q12])
    np.testing.assert_array_equal(d._effective_charges(), Q12)
    assert d._all_included and not d._all_neutral                                # residues of one atom each
    assert DipoleMoment(_universe(resids=np.arange(12) // 2).atoms, charges=[Q12])._all_neutral


def test_neutral_and_included_flags():
    u = _universe(charges=Q12, resids=np.arange(12) // 2)
    assert DipoleMoment(u.atoms)._all_neutral and DipoleMoment(u.atoms)._all_included
    assert not DipoleMoment(u.select(np.arange(10)))._all_included
    ions = _universe(charges=Q12, resids=np.arange(12))
    assert not DipoleMoment(ions.atoms)._all_neutral
    nearly = _universe(charges=Q12 + np.tile([4e-7, 0.0], 6), resids=np.arange(12) // 2)
    assert DipoleMoment(nearly.atoms)._all_neutral                              # atol = 1e-6


def test_neutralize_effective_charges():
    rng = np.random.default_rng(5)
    n = 40
    resids = np.sort(rng.integers(0, 9, n))
    q = rng.normal(size=n)
    m = rng.uniform(1.0, 20.0, n)
    u = _universe(n_atoms=n, charges=q, masses=m, resids=resids)
    a, b = u.select(np.arange(0, n, 2)), u.select(np.arange(1, n, 2))      # residues split over two groups
    d = DipoleMoment([a, b], neutralize=True, verbose=False)
    eff = d._effective_charges()
    assert eff.dtype == np.float64 and eff.shape == (n,)
    for g, s in zip((a, b), d._slices):
        r = resids[g.indices]
        for k in np.unique(r):
            assert abs(eff[s][r == k].sum()) <= 1e-12 * np.abs(q[g.indices][r == k]).sum()
    # the charges of the universe and of the object are left alone
    np.testing.assert_array_equal(u.atoms.charges, q)
    np.testing.assert_array_equal(np.concatenate(d._charges), np.r_[q[0::2], q[1::2]])
    # a charged three-atom residue with unequal masses, by hand: Q = 0.5, M = 19
    u3 = _universe(n_atoms=3, charges=[1.0, -0.2, -0.3], masses=[16.0, 1.0, 2.0], resids=[0, 0, 0])
    eff = DipoleMoment(u3.atoms, neutralize=True)._effective_charges()
    np.testing.assert_allclose(eff, [1.0 - 0.5 * 16 / 19, -0.2 - 0.5 * 1 / 19, -0.3 - 0.5 * 2 / 19], rtol=1e-15)
    np.testing.assert_array_equal(DipoleMoment(u3.atoms)._effective_charges(), [1.0, -0.2, -0.3])


class Kelvin:
    """A quantity with units, as ``strip_unit`` recognises pint's."""
    units = object()            # not a str: a str is the name strip_unit assumes for plain numbers
    magnitude = 300.0

    def m_as(self, unit):
        return self.magnitude


def test_relative_permittivity_errors_and_value():
    rng = np.random.default_rng(2)
    M = rng.normal(size=(6, 2, 3))
    V = np.full(6, 1680.0)
    neutral = _universe(n_frames=6, charges=Q12, resids=np.arange(12) // 2)
    ions = _universe(n_frames=6, charges=Q12, resids=np.arange(12))

    def state(d, dipoles=M, volumes=V):
        d.results.dipoles, d.results.volumes = dipoles, volumes
        return d

    halves = lambda u: [u.select(np.arange(6)), u.select(np.arange(6, 12))]      # noqa: E731
    with pytest.raises(RuntimeError, match="averaged dipole moment"):
        state(DipoleMoment(halves(neutral), average=True), M.mean(axis=0), V.mean()) \
            .calculate_relative_permittivity(300.0)
    with pytest.raises(RuntimeError, match="non-neutral system or a system with ions"):
        state(DipoleMoment(halves(ions))).calculate_relative_permittivity(300.0)
    with pytest.raises(RuntimeError, match="not all"):
        state(DipoleMoment([neutral.select(np.arange(6)), neutral.select(np.arange(6, 10))])) \
            .calculate_relative_permittivity(300.0)
    with pytest.raises(ValueError, match="'temperature' cannot have units when reduced=True"):
        state(DipoleMoment(halves(neutral), reduced=True)).calculate_relative_permittivity(Kelvin())

    d = state(DipoleMoment(halves(neutral)))
    d.calculate_relative_permittivity(300.0)
    assert isinstance(d.results.dielectric, float)
    assert d.results.dielectric == calculate_relative_permittivity(M.sum(axis=1), 300.0, V)
    d.calculate_relative_permittivity(Kelvin())                                    # units are fine when not reduced
    assert d.results.dielectric == calculate_relative_permittivity(M.sum(axis=1), 300.0, V)
    # ions are fine with neutralize; reduced units; a single group
    d = state(DipoleMoment(halves(ions), neutralize=True, reduced=True))
    d.calculate_relative_permittivity(1.5)
    assert d.results.dielectric == calculate_relative_permittivity(M.sum(axis=1), 1.5, V, reduced=True)
    d = state(DipoleMoment(neutral.atoms, reduced=True), M[:, :1])
    d.calculate_relative_permittivity(1.0)
    assert d.results.dielectric == calculate_relative_permittivity(M[:, 0], 1.0, V, reduced=True)


def test_run_raises_without_a_device():
    """There is no CPU fallback: without a HIP device the class and the engine raise."""
    from mdhelper_amd import _lib
    if _lib.device_count() == 0:
        with pytest.raises(RuntimeError):
            DipoleMoment(_universe(charges=Q12).atoms, verbose=False).run()
        with pytest.raises(RuntimeError):
            _core.DipoleEngine([12], Q12)


def test_engine_argument_errors_need_no_device():
    from mdhelper_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    one, q = np.array([2], dtype=np.int64), np.array([1.0, -1.0])
    for n_groups, n_points, charges, word in ((0, one, q, b"n_groups"),
                                              (4097, one, q, b"n_groups"),
                                              (1, np.array([0], dtype=np.int64), q, b"at least 1 point"),
                                              (1, np.array([2 ** 31 // 3], dtype=np.int64), q, b"2^31 / 3"),
                                              (1, one, np.array([1.0, np.nan]), b"finite"),
                                              (1, one, np.array([np.inf, 1.0]), b"finite")):
        rc = lib.mdx_dip_create(ctypes.byref(h), 0, n_groups, p(n_points), p(charges))
        assert rc == -1 and word in lib.mdx_last_error(), (n_groups, n_points, lib.mdx_last_error())
    assert lib.mdx_dip_create(ctypes.byref(h), 0, 1, None, p(q)) == -1 and b"NULL" in lib.mdx_last_error()
    assert lib.mdx_dip_set_slab_frames(None, 8) == -1 and b"NULL" in lib.mdx_last_error()
    with pytest.raises(ValueError, match="one entry per point"):
        _core.DipoleEngine([2, 3], np.ones(4))
    with pytest.raises(ValueError, match="one entry per group"):
        _core.DipoleEngine([], np.ones(0))
    assert _core.DipoleEngine.TILE == 128
