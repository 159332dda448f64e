"""
Host-side checks of ``mdhelper_amd.analysis.profile`` that need no GPU: ``calculate_potential_profile`` against
outputs of the reference's function (``tests/golden/profile_ref.npz``, written by
``scripts/make_golden_profile.py``), the constructor's validation and argument parsing, the arithmetic of
``_conclude`` on a recorder engine, and the loud failure without a device.
"""
import ctypes
import json
import warnings

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import DensityProfile, calculate_potential_profile, profile


def _universe(n_frames=4, n_atoms=60, dims=(10.0, 12.0, 14.0), **topology):
    rng = np.random.default_rng(0)
    pos = (rng.random((n_frames, n_atoms, 3)) * (10.0 if dims is None else dims)).astype(np.float32)
    box = None if dims is None else [*dims, 90.0, 90.0, 90.0]
    return mdhelper_amd.ArrayUniverse(pos, box, **topology)


# ---------------------------------------------------------------- potential profile

@pytest.fixture(scope="module")
def ref(golden_dir):
    z = np.load(golden_dir / "profile_ref.npz")
    return z, json.loads(str(z["cases"]))


def _potential(z, which, kw):
    kw = dict(kw)
    dielectric = kw.pop("dielectric", 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return calculate_potential_profile(z["bins"], z[which], float(z["L"]), dielectric, reduced=True, **kw)


def test_fixture_covers_the_cases(ref):
    z, cases = ref
    kws = [kw for _, kw in cases.values()]
    assert any("sigma_q" in k and k.get("method", "integral") == "integral" for k in kws)
    assert any("dV" in k and "sigma_q" not in k and k.get("method", "integral") == "integral" for k in kws)
    assert any(k.get("V0") for k in kws)
    assert any(k.get("method") == "matrix" and not k.get("pbc") for k in kws)
    assert any(k.get("method") == "matrix" and k.get("pbc") for k in kws)
    assert any(not k for k in kws)      # integral method without sigma_q or dV: the plateau search


@pytest.mark.parametrize("name", ["integral_sigma", "integral_sigma_dielectric", "integral_dV",
                                  "integral_plateau"])
def test_integral_method_against_the_reference(ref, name):
    z, cases = ref
    want = z["out_" + name]
    got = _potential(z, *cases[name])
    # two trapezoid sums of ~200 terms: <= n eps ~ 5e-14 of max|psi|; 1e-12 leaves a factor of ~20
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", ["matrix_slab", "matrix_slab_dV", "matrix_pbc"])
def test_matrix_method_against_the_reference(ref, name):
    z, cases = ref
    want = z["out_" + name]
    got = _potential(z, *cases[name])
    # condition number of the second-difference matrix at n = 201 <~ (2 n / pi)^2 ~ 1.6e4, times 2^-52
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_nonzero_V0(ref):
    """The reference passes V0 as cumulative_trapezoid(initial=V0): the installed SciPy refuses that (the
    fixture records the error it raised), older SciPy only wrote V0 into the first element.  The port follows
    the documented step instead, "apply the second BC by adding V0 to all points": the V0 = 0 result, which IS
    checked against the reference above, plus V0."""
    z, cases = ref
    which, kw = cases["integral_V0"]
    assert "out_integral_V0" not in z.files and "initial" in str(z["error_integral_V0"])
    zero = {k: v for k, v in kw.items() if k != "V0"}
    assert zero == cases["integral_sigma"][1]
    want = z["out_integral_sigma"] + kw["V0"]
    got = _potential(z, which, kw)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert got[0] == kw["V0"]


def test_plateau_case_warns_and_has_a_plateau(ref):
    z, cases = ref
    with pytest.warns(UserWarning, match="No surface charge density information"):
        psi = calculate_potential_profile(z["bins"], z["layers"], float(z["L"]), reduced=True)
    assert np.all(np.isfinite(psi))


def test_potential_errors_and_factor():
    bins = np.linspace(0.5, 9.5, 10)
    rho = np.sin(bins)
    with pytest.raises(ValueError, match="must have the same length"):
        calculate_potential_profile(bins, rho[:-1], 10.0)
    with pytest.raises(ValueError, match="Either 'sigma_q' or 'dV' must be provided"):
        calculate_potential_profile(bins, rho, 10.0, method="matrix")
    with pytest.raises(ValueError, match="uniformly spaced"):
        calculate_potential_profile(bins ** 2, rho, 10.0, sigma_q=0.0, method="matrix")
    assert calculate_potential_profile(bins, rho, 10.0, sigma_q=0.0, method="other") is None
    # e / (eps0 * angstrom) in volts, from the two CODATA 2018 constants
    assert profile.ELEMENTARY_CHARGE == 1.602176634e-19 and profile.VACUUM_PERMITTIVITY == 8.8541878128e-12
    assert profile.POTENTIAL_FACTOR == 1.602176634e-19 / (8.8541878128e-12 * 1e-10)
    assert abs(profile.POTENTIAL_FACTOR - 180.95126) < 1e-4
    real = calculate_potential_profile(bins, rho, 10.0, 2.0, sigma_q=0.1)
    reduced = calculate_potential_profile(bins, rho, 10.0, 2.0, sigma_q=0.1, reduced=True)
    np.testing.assert_allclose(real, reduced * profile.POTENTIAL_FACTOR / (4 * np.pi), rtol=1e-14)


# ---------------------------------------------------------------- constructor

def test_constructor_validation():
    u = _universe()
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    with pytest.raises(ValueError, match="Invalid grouping 'molecules'"):
        DensityProfile(u.atoms, "molecules")
    with pytest.raises(ValueError, match="number of grouping values"):
        DensityProfile([a, b], ["atoms"])
    with pytest.raises(ValueError, match="Invalid grouping 'x'"):
        DensityProfile([a, b], ["atoms", "x"])
    with pytest.raises(ValueError, match="incompatible with the number of axes"):
        DensityProfile(u.atoms, axes="xy", n_bins=(10, 20, 30))
    with pytest.raises(ValueError, match="must be an integer or an iterable"):
        DensityProfile(u.atoms, n_bins="many")
    with pytest.raises(ValueError, match="same number of bins when parallel=True"):
        DensityProfile(u.atoms, axes="xy", n_bins=(10, 20), parallel=True)
    with pytest.raises(ValueError, match="number of group charges"):
        DensityProfile([a, b], charges=[1.0])
    with pytest.raises(ValueError, match="'dimensions' must have length 3"):
        DensityProfile(u.atoms, dimensions=[1.0, 2.0])
    with pytest.raises(ValueError, match="No system dimensions found or provided"):
        DensityProfile(_universe(dims=None).atoms)
    with pytest.raises(ValueError, match="scaling factor"):
        DensityProfile(u.atoms, scales=(1.0, 2.0))
    with pytest.raises(ValueError, match="Invalid value passed to 'recenter'"):
        DensityProfile([a, b], recenter="first")
    with pytest.raises(ValueError, match="Invalid group index passed to 'recenter'"):
        DensityProfile([a, b], recenter=2)
    with pytest.raises(ValueError, match="not in 'groups'"):
        DensityProfile([a, b], recenter=u.select(np.arange(5)))


@pytest.mark.parametrize("axes,want", [(2, [2]), ("xy", [0, 1]), ((0, 1), [0, 1]), ("zx", [2, 0]),
                                       ("XYZ", [0, 1, 2]), (("y", 0), [1, 0])])
def test_axes_parsing(axes, want):
    dp = DensityProfile(_universe().atoms, axes=axes, n_bins=7)
    np.testing.assert_array_equal(dp._axes, want)
    np.testing.assert_array_equal(dp._n_bins, [7] * len(want))


def test_universe_box_lengths_scale_in_float32():
    """MDAnalysis holds the box in float32 and the reference multiplies it by ``scales`` in place: the scaled
    length is the float32 product, widened; explicit float64 ``dimensions`` scale in float64."""
    u = _universe(dims=(10.1, 12.3, 14.7))
    scales = (1.1, 0.7, 1.3)
    want = (np.array([10.1, 12.3, 14.7], dtype=np.float32) * np.array(scales)).astype(np.float32).astype(float)
    got = DensityProfile(u.atoms, scales=scales)._dimensions
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    assert np.any(want != np.array([10.1, 12.3, 14.7], dtype=np.float32).astype(float) * np.array(scales))
    got = DensityProfile(u.atoms, dimensions=[10.1, 12.3, 14.7], scales=scales)._dimensions
    np.testing.assert_array_equal(got, np.array([10.1, 12.3, 14.7]) * np.array(scales))
    got = DensityProfile(u.atoms, dimensions=[10, 12, 14], scales=1.5)._dimensions
    np.testing.assert_array_equal(got, [15.0, 18.0, 21.0])


def test_scales_charges_and_recenter_forms():
    u = _universe(charges=np.repeat([1.0, -2.0], 30))
    a, b = u.select(np.arange(30)), u.select(np.arange(30, 60))
    dp = DensityProfile([a, b], scales=(1.0, 0.5, 2.0))
    np.testing.assert_array_equal(dp._dimensions, [10.0, 6.0, 28.0])
    np.testing.assert_array_equal(dp._charges, [1.0, -2.0])
    np.testing.assert_array_equal(DensityProfile([a, b], scales=3)._dimensions, [30.0, 36.0, 42.0])
    np.testing.assert_array_equal(DensityProfile([a, b], charges=[3, 4])._charges, [3, 4])
    with pytest.warns(UserWarning, match="share the same charge"):
        assert DensityProfile([u.atoms])._charges is None
    assert DensityProfile([_universe().atoms])._charges is None
    k, target = DensityProfile([a, b], scales=2, recenter=1)._recenter
    assert k == 1
    np.testing.assert_array_equal(target, [10.0, 12.0, 14.0])          # the centre of the SCALED box
    assert DensityProfile([a, b], recenter=b)._recenter[0] == 1
    k, target = DensityProfile([a, b], recenter=(a, [1.0, np.nan, 3.0]))._recenter
    assert k == 0 and target[0] == 1.0 and np.isnan(target[1]) and target[2] == 3.0


# ---------------------------------------------------------------- conclude arithmetic on a recorder engine

class Recorder:
    """Stands in for ``_core.ProfileEngine``: records what it is fed and returns counts that encode
    (axis, group, frame, bin)."""
    made = []

    def __init__(self, sizes, axes, n_bins, dims, *, per_frame=False, dev=0, timing=False):
        self.sizes, self.axes, self.n_bins, self.dims = list(sizes), list(axes), list(n_bins), np.array(dims)
        self.per_frame, self.frames, self.calls = per_frame, 0, []
        self.grouping = self.recenter = None
        self.closed = False
        Recorder.made.append(self)

    def set_grouping(self, offsets, masses):
        self.grouping = (np.asarray(offsets), np.asarray(masses))

    def set_recenter(self, group, masses=None, target=None):
        self.recenter = (group, np.asarray(masses), np.asarray(target))

    def accumulate(self, pos):
        self.calls.append(("host", np.array(pos)))
        self.frames += len(pos)

    def counts(self):
        out = []
        for a, nb in enumerate(self.n_bins):
            g = np.arange(len(self.sizes))[:, None, None]
            f = np.arange(self.frames)[None, :, None]
            b = np.arange(nb)[None, None, :]
            c = (1000 * (a + 1) + 100 * g + 10 * f + b + 1).astype(np.int64)
            out.append(c if self.per_frame else c.sum(axis=1))
        return out

    def close(self):
        self.closed = True


@pytest.fixture
def recorder(monkeypatch):
    Recorder.made = []
    monkeypatch.setattr(_core, "ProfileEngine", Recorder)
    return Recorder


def test_conclude_averaging_charges_and_bins(recorder):
    u = _universe(n_frames=5)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    dp = DensityProfile([a, b], axes="zx", n_bins=(4, 3), charges=[1.0, -2.0], scales=(1.0, 1.0, 2.0),
                        verbose=False).run(step=2)
    eng = recorder.made[0]
    assert eng.closed and eng.frames == 3 and not eng.per_frame and eng.axes == [2, 0] and eng.n_bins == [4, 3]
    np.testing.assert_array_equal(eng.dims, [10.0, 12.0, 28.0])
    np.testing.assert_array_equal(eng.calls[0][1], u.trajectory.frame_block([0, 2, 4]))
    V = 10.0 * 12.0 * 28.0
    raw = Recorder([20, 40], [2, 0], [4, 3], eng.dims)
    raw.frames = 3
    for i, (nb, L) in enumerate(((4, 28.0), (3, 10.0))):
        want = raw.counts()[i] * (nb / V / 3)
        np.testing.assert_array_equal(dp.results.number_densities[i], want)
        np.testing.assert_array_equal(dp.results.charge_densities[i], 1.0 * want[0] - 2.0 * want[1])
        np.testing.assert_array_equal(dp.results.bins[i], np.linspace(L / (2 * nb), L - L / (2 * nb), nb))
    assert "times" not in dp.results
    assert dp.results.units == {"results.bins": "angstrom", "results.number_densities": "angstrom^-3",
                                "results.charge_densities": "elementary_charge/angstrom^3"}


def test_conclude_per_frame_shapes_and_times(recorder):
    u = _universe(n_frames=6)
    a, b = u.select(np.arange(20)), u.select(np.arange(20, 60))
    dp = DensityProfile([b, a], axes=1, n_bins=5, charges=[0.5, 1.5], dt=0.2, average=False,
                        verbose=False).run(start=1)
    eng = recorder.made[0]
    assert eng.per_frame and eng.frames == 5 and eng.sizes == [40, 20]
    # rows arrive in the order of the concatenated groups
    np.testing.assert_array_equal(eng.calls[0][1], u.trajectory.frame_block(np.arange(1, 6))[:, np.r_[20:60, 0:20]])
    V = 10.0 * 12.0 * 14.0
    raw = Recorder([40, 20], [1], [5], eng.dims, per_frame=True)
    raw.frames = 5
    want = raw.counts()[0] * (5 / V)
    assert dp.results.number_densities[0].shape == (2, 5, 5)
    np.testing.assert_array_equal(dp.results.number_densities[0], want)
    assert dp.results.charge_densities[0].shape == (5, 5)
    np.testing.assert_array_equal(dp.results.charge_densities[0], 0.5 * want[0] + 1.5 * want[1])
    np.testing.assert_allclose(dp.results.times, 0.2 * np.arange(1, 6), rtol=1e-15)
    dp.calculate_potential_profile(2.0, "y", sigma_q=0.0)
    np.testing.assert_array_equal(
        dp.results.potentials[0],
        calculate_potential_profile(dp.results.bins[0], dp.results.charge_densities[0].mean(axis=0), 12.0, 2.0,
                                    sigma_q=0.0))
    with pytest.raises(RuntimeError, match="provide charge information"):
        DensityProfile([a], verbose=False).calculate_potential_profile(1.0, 0)


def test_grouping_and_recenter_reach_the_engine(recorder):
    resids = np.repeat(np.arange(20), 3)
    masses = np.tile([16.0, 1.0, 1.0], 20)
    u = _universe(resids=resids, masses=masses)
    ions, water = u.select(np.arange(0, 15)), u.select(np.arange(15, 60))
    DensityProfile([ions, water], ("atoms", "residues"), recenter=(1, [np.nan, 2.0, 3.0]), verbose=False).run()
    eng = recorder.made[0]
    assert eng.sizes == [15, 15]
    offsets, m = eng.grouping
    np.testing.assert_array_equal(offsets, np.concatenate((np.arange(15), 15 + 3 * np.arange(16))))
    np.testing.assert_array_equal(m, np.concatenate((np.ones(15), masses[15:])))
    group, rm, target = eng.recenter
    assert group == 1
    np.testing.assert_array_equal(rm, np.full(15, 18.0))                # masses of the grouping level
    np.testing.assert_array_equal(target, [np.nan, 2.0, 3.0])


class TwoRanks:
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank, self.reduced = rank, []

    def allreduce(self, arr, op="sum"):
        arr = np.asarray(arr)
        assert arr.dtype == np.int64 and op == "sum"
        self.reduced.append(arr.copy())
        return arr * 2                      # "the other rank" held the same numbers


@pytest.mark.parametrize("rank", [0, 1])
def test_two_ranks_shard_frames_and_allreduce(recorder, rank):
    u = _universe(n_frames=7)
    comm = TwoRanks(rank)
    dp = DensityProfile(u.atoms, axes="x", n_bins=3, average=False, verbose=False, comm=comm).run()
    eng = recorder.made[0]
    lo, hi = ((0, 4), (4, 7))[rank]
    assert eng.frames == hi - lo
    np.testing.assert_array_equal(eng.calls[0][1], u.trajectory.frame_block(np.arange(lo, hi)))
    # this rank's rows sit inside a zero-filled array over all frames before the sum
    (sent,) = comm.reduced
    assert sent.shape == (1, 7, 3)
    assert np.all(sent[:, :lo] == 0) and np.all(sent[:, hi:] == 0) and np.all(sent[:, lo:hi] > 0)
    np.testing.assert_array_equal(dp.results.number_densities[0], 2 * sent * (3 / (10.0 * 12.0 * 14.0)))
    comm = TwoRanks(rank)
    dp = DensityProfile(u.atoms, axes="x", n_bins=3, verbose=False, comm=comm).run()
    (sent,) = comm.reduced
    assert sent.shape == (1, 3)
    np.testing.assert_array_equal(dp.results.number_densities[0], 2 * sent * (3 / (10.0 * 12.0 * 14.0) / 7))


def test_recenter_with_two_ranks_raises(recorder):
    u = _universe()
    with pytest.raises(ValueError, match="recenter cannot be combined with more than one rank"):
        DensityProfile(u.atoms, recenter=0, verbose=False, comm=TwoRanks(0)).run()
    assert not recorder.made


# ---------------------------------------------------------------- C-ABI and no-device behaviour

def test_create_argument_errors_need_no_device():
    lib = _lib.lib()

    def create(offsets, axes, n_bins, dims, n_groups=None):
        h = ctypes.c_void_p()
        o = np.asarray(offsets, dtype=np.int64)
        a = np.asarray(axes, dtype=np.int32)
        b = np.asarray(n_bins, dtype=np.int64)
        d = np.asarray(dims, dtype=np.float64)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
        rc = lib.mdx_prof_create(ctypes.byref(h), 0, len(o) - 1 if n_groups is None else n_groups, p(o), len(a),
                                 p(a), p(b), p(d), 0)
        return rc, lib.mdx_last_error().decode()

    for args, word in ((([0, 5], [3], [10], [1, 1, 1]), "axis 3"),
                       (([0, 5], [0, 0], [10, 10], [1, 1, 1]), "given twice"),
                       (([0, 5], [0], [0], [1, 1, 1]), "n_bins"),
                       (([0, 5], [2], [10], [1, 1, 0]), "dims[2]"),
                       (([0, 5], [2], [10], [1, -1, 1]), "dims[1]"),
                       (([1, 5], [2], [10], [1, 1, 1]), "start at 0"),
                       (([0, 5, 3], [2], [10], [1, 1, 1]), "must not decrease"),
                       (([0, 0], [2], [10], [1, 1, 1]), "points")):
        rc, msg = create(*args)
        assert rc == -1 and word in msg, (args, rc, msg)
    with pytest.raises(ValueError, match="axis 7"):
        _core.ProfileEngine([5], [7], 10, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="three box lengths"):
        _core.ProfileEngine([5], [0], 10, [1.0, 1.0])


def test_run_fails_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    u = _universe()
    with pytest.raises(RuntimeError, match="no CPU fallback|not available"):
        DensityProfile(u.atoms).run()
    with pytest.raises(RuntimeError):
        _core.ProfileEngine([60], [0, 1, 2], 201, [10.0, 12.0, 14.0])
