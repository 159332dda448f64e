"""
Gyradius / GyrationEngine on the GPU against a float64 NumPy restatement of the reference's per-frame work
(reference src/mdhelper/analysis/polymer.py:439-465 with algorithm/molecule.py radius_of_gyration and
algorithm/topology.py unwrap): points -> (global unwrap from `start`) -> per chain the centre of mass, then the
mass-weighted second moments of the centred coordinates, both summed sequentially -> square roots -> mean over chains.
The restatement itself is first asserted against outputs of the reference's function
(``tests/golden/gyradius_ref.npz``), so the chain reference -> restatement -> device is closed.

Tolerance: restatement and device form the same float64 sums in different orders (the device folds 64 lanes in a
tree); sums of at most N_p non-negative terms after centring differ by at most ~2 (N_p + 8) 2^-53 relative — 2.3e-13
at N_p = 1000, the longest chain here — and the mean over at most 7 chains adds a few 2^-53.  rtol = 1e-11 is ~45
times above that at N_p = 1000 (~350 times at N_p = 130) and 200 times below the 2e-9 a one-pass second moment loses on
the chains 9 000 A from the origin.  A chain of one point has Rg = 0 up to the rounding of m x / m, so
atol = 8 2^-53 max|r| is added.  Outputs that must not depend on the route or on the split into calls are compared
with ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import Gyradius

pytestmark = pytest.mark.gpu

RTOL = 1e-11


def atol_for(pos):
    return 8 * 2.0 ** -53 * float(np.abs(pos).max())


# ---------------------------------------------------------------- restatement

def chain_radii_ref(points, masses):
    """points float64[..., M, N_p, 3], masses float64[M, N_p] -> [..., M, 4]: Rg, Rg_x, Rg_y, Rg_z per chain;
    sequential two-pass sums over the monomers."""
    points = np.asarray(points, dtype=np.float64)
    masses = np.asarray(masses, dtype=np.float64)
    N_p = masses.shape[-1]
    total = np.zeros(masses.shape[:-1])
    acc = np.zeros(points.shape[:-2] + (3,))
    for j in range(N_p):
        total = total + masses[:, j]
        acc = acc + masses[:, j, None] * points[..., j, :]
    c = acc / total[:, None]
    S = np.zeros_like(acc)
    for j in range(N_p):
        e = points[..., j, :] - c
        S = S + masses[:, j, None] * (e * e)
    sx, sy, sz = S[..., 0], S[..., 1], S[..., 2]
    return np.sqrt(np.stack(((sx + sy) + sz, sy + sz, sx + sz, sx + sy), axis=-1) / total[:, None])


def radii_ref(points, masses, n_chains, n_monomers):
    """points float64[F, N, 3] in concatenated-group order -> [G, F, 4], the mean over each group's chains."""
    out, lo = [], 0
    for M, N_p in zip(n_chains, n_monomers):
        hi = lo + M * N_p
        p = np.asarray(points[:, lo:hi], dtype=np.float64).reshape(len(points), M, N_p, 3)
        out.append(chain_radii_ref(p, np.asarray(masses[lo:hi]).reshape(M, N_p)).mean(axis=1))
        lo = hi
    return np.stack(out)


def unwrap_ref(points, start, dims, margin=None):
    """The reference's rule frame by frame from `start`: d = x - x_prev; |d| >= dims / 2 moves the image count by
    -sign(d); x_prev becomes the raw x; the point used is x + image * L.  margin: filled with the smallest
    | |d| - L/2 | met."""
    points = np.asarray(points, dtype=np.float64)
    dims = np.asarray(dims, dtype=np.float64)
    old = np.array(start, dtype=np.float64)
    images = np.zeros(points.shape[1:], dtype=int)
    out = np.empty_like(points)
    for f in range(len(points)):
        d = points[f] - old
        if margin is not None:
            margin.append(np.abs(np.abs(d) - dims / 2).min())
        crossed = np.abs(d) >= dims / 2
        images[crossed] -= np.sign(d[crossed]).astype(int)
        old = points[f].copy()
        out[f] = points[f] + images * dims
    return out


def centres_ref(pos, size, masses):
    """float64 centres of monomers of `size` consecutive rows: sequential sum in row order, one division."""
    F, N, _ = pos.shape
    p = pos.astype(np.float64).reshape(F, N // size, size, 3)
    m = np.asarray(masses, dtype=np.float64).reshape(N // size, size)
    acc = np.zeros((F, N // size, 3))
    tot = np.zeros(N // size)
    for a in range(size):
        acc = acc + m[None, :, a, None] * p[:, :, a]
        tot = tot + m[:, a]
    return acc / tot[None, :, None]


def walks(rng, F, M, N_p, *, bond=1.5, spread=40.0, offset=0.0):
    """float32[F, M * N_p, 3] random-walk chains, independent per frame."""
    steps = rng.normal(size=(F, M, N_p, 3))
    steps *= bond / np.linalg.norm(steps, axis=-1, keepdims=True)
    pos = rng.uniform(0.0, spread, (F, M, 1, 3)) + np.cumsum(steps, axis=2) + offset
    return pos.reshape(F, M * N_p, 3).astype(np.float32)


def engine_radii(pos, n_chains, n_monomers, masses, *, splits=None, setup=None):
    eng = _core.GyrationEngine(n_chains, n_monomers, masses)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return eng.result(), eng.stats()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "gyradius_ref.npz")


def box(dims):
    return [*dims, 90.0, 90.0, 90.0]


# ---------------------------------------------------------------- reference -> restatement

def test_restatement_against_the_reference(golden):
    for name in golden["cases"]:
        pos, masses = golden[f"pos_{name}"], golden[f"masses_{name}"]
        got = chain_radii_ref(pos.astype(np.float64), masses)
        np.testing.assert_allclose(got[:, 0], golden[f"out_{name}_rg"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got[:, 1:], golden[f"out_{name}_xyz"], rtol=RTOL, atol=0)


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("M", [1, 3, 7])
@pytest.mark.parametrize("N_p", [1, 2, 63, 64, 65, 130, 1000])
def test_engine_shapes(N_p, M):
    rng = np.random.default_rng(1000 * N_p + M)
    F = 3
    pos = walks(rng, F, M, N_p)
    masses = rng.uniform(1.0, 20.0, M * N_p)
    got, st = engine_radii(pos, [M], [N_p], masses)
    assert got.shape == (1, F, 4) and st["frames"] == F
    np.testing.assert_allclose(got, radii_ref(pos, masses, [M], [N_p]), rtol=RTOL, atol=atol_for(pos))
    if N_p == 1:
        assert np.abs(got).max() <= atol_for(pos)


def test_engine_against_the_golden_chains(golden):
    """The device against the reference's own outputs, every golden case as one group of one engine."""
    names = list(golden["cases"])
    pos = np.concatenate([golden[f"pos_{n}"].reshape(-1, 3) for n in names])[None]
    masses = np.concatenate([golden[f"masses_{n}"].ravel() for n in names])
    shapes = [golden[f"pos_{n}"].shape[:2] for n in names]
    got, _ = engine_radii(pos, [s[0] for s in shapes], [s[1] for s in shapes], masses)
    for g, n in enumerate(names):
        np.testing.assert_allclose(got[g, 0, 0], golden[f"out_{n}_rg"].mean(), rtol=RTOL, atol=0)
        np.testing.assert_allclose(got[g, 0, 1:], golden[f"out_{n}_xyz"].mean(axis=0), rtol=RTOL, atol=0)


def test_engine_mixed_groups():
    rng = np.random.default_rng(2)
    n_chains, n_monomers, F = [3, 7, 5], [65, 2, 1], 7
    pos = np.concatenate([walks(rng, F, M, N) for M, N in zip(n_chains, n_monomers)], axis=1)
    masses = rng.uniform(0.5, 30.0, pos.shape[1])
    got, st = engine_radii(pos, n_chains, n_monomers, masses)
    assert got.shape == (3, F, 4) and st["frames"] == F
    want = radii_ref(pos, masses, n_chains, n_monomers)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol_for(pos))
    assert np.all(got[:2, :, 0] > 0.5)
    with pytest.raises(ValueError):
        engine_radii(pos[:, :50], n_chains, n_monomers, masses)        # wrong number of rows


def test_cancellation_far_from_the_origin(golden):
    pos, masses = golden["pos_far"], golden["masses_far"]
    assert pos.min() > 8000.0
    frames = pos.reshape(1, -1, 3)
    got, _ = engine_radii(frames, [3], [130], masses.ravel())
    np.testing.assert_allclose(got[0, 0, 0], golden["out_far_rg"].mean(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[0, 0, 1:], golden["out_far_xyz"].mean(axis=0), rtol=RTOL, atol=0)
    np.testing.assert_allclose(got, radii_ref(frames, masses.ravel(), [3], [130]), rtol=RTOL, atol=0)
    # the one-pass form on the same chains misses this tolerance by orders of magnitude
    x = pos.astype(np.float64)
    one_pass = (masses[:, :, None] * x * x).sum(axis=1) - (masses[:, :, None] * x).sum(axis=1) ** 2 \
        / masses.sum(axis=1)[:, None]
    bad = np.sqrt(one_pass.sum(axis=1) / masses.sum(axis=1))
    assert np.abs(bad / golden["out_far_rg"] - 1).max() > 100 * RTOL


def test_determinism_across_splits_and_routes():
    rng = np.random.default_rng(3)
    n_chains, n_monomers, F = [4, 9], [130, 7], 9
    pos = np.concatenate([walks(rng, F, M, N) for M, N in zip(n_chains, n_monomers)], axis=1)
    masses = rng.uniform(1.0, 20.0, pos.shape[1])
    once, _ = engine_radii(pos, n_chains, n_monomers, masses)
    split, st = engine_radii(pos, n_chains, n_monomers, masses, splits=[0, 1, 4, 9])
    assert st["frames"] == F
    np.testing.assert_array_equal(split, once)
    d = _core.DeviceArray.from_host(pos)
    eng = _core.GyrationEngine(n_chains, n_monomers, masses)
    try:
        eng.accumulate_device(d.ptr, pos.shape[1], F)
        np.testing.assert_array_equal(eng.result(), once)
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.result().shape == (2, 0, 4)
        eng.accumulate_device(d.rows(2, 5).ptr, pos.shape[1], 5)
        eng.accumulate(pos[7:])
        np.testing.assert_array_equal(eng.result(), once[:, 2:])
    finally:
        eng.close()
        d.free()
    np.testing.assert_allclose(once, radii_ref(pos, masses, n_chains, n_monomers), rtol=RTOL, atol=atol_for(pos))


def test_gather_through_an_index():
    rng = np.random.default_rng(4)
    M, N_p, F = 5, 33, 4
    n_total = 3 * M * N_p + 2
    frame = (rng.random((F, n_total, 3)) * 50).astype(np.float32)
    chains = walks(rng, F, M, N_p)
    # the group is every third particle of the larger frame, the chains in reversed order
    index = (3 * np.arange(M * N_p)).reshape(M, N_p)[::-1].ravel()
    frame[:, index] = chains
    masses = rng.uniform(1.0, 20.0, M * N_p)
    want = radii_ref(frame[:, index], masses, [M], [N_p])
    d = _core.DeviceArray.from_host(frame)
    eng = _core.GyrationEngine([M], [N_p], masses)
    try:
        eng.accumulate_device(d.ptr, n_total, F, index)
        got = eng.result()
        with pytest.raises(ValueError):
            eng.accumulate_device(d.ptr, n_total, F, np.append(index[:-1], n_total))      # out of range
    finally:
        eng.close()
        d.free()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol_for(frame))
    host, _ = engine_radii(frame[:, index], [M], [N_p], masses)
    np.testing.assert_array_equal(got, host)


def test_grouping_forms_the_monomer_centres():
    rng = np.random.default_rng(5)
    M, N_p, size, F = 4, 5, 3, 6
    centres = walks(rng, F, M, N_p, bond=4.0).astype(np.float64)
    pos = (centres[:, :, None, :] + rng.uniform(-1, 1, (F, M * N_p, size, 3))).reshape(F, -1, 3).astype(np.float32)
    atom_masses = rng.uniform(1.0, 16.0, M * N_p * size)
    point_masses = atom_masses.reshape(-1, size).sum(axis=1)
    want = radii_ref(centres_ref(pos, size, atom_masses), point_masses, [M], [N_p])
    offsets = size * np.arange(M * N_p + 1)
    got, _ = engine_radii(pos, [M], [N_p], point_masses, setup=lambda e: e.set_grouping(offsets, atom_masses))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol_for(pos))
    split, _ = engine_radii(pos, [M], [N_p], point_masses, splits=[0, 2, 3, 6],
                            setup=lambda e: e.set_grouping(offsets, atom_masses))
    np.testing.assert_array_equal(split, got)
    with pytest.raises(ValueError):
        engine_radii(pos, [M], [N_p], point_masses, setup=lambda e: e.set_grouping(offsets[:-1], atom_masses[:-size]))


# ---------------------------------------------------------------- unwrap

def _drifting_chains(seed, F, M, N_p, L, drift):
    """Chains with 1 A bonds that wriggle a little and drift together; returns (wrapped float32[F, N, 3],
    image counts int[F, N, 3] with wrapped + images * L = the whole chains)."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(M, N_p, 3))
    steps /= np.linalg.norm(steps, axis=-1, keepdims=True)
    first = rng.uniform(0.0, L, (M, 1, 3)) + np.cumsum(steps, axis=1)
    true = (first[None] + np.cumsum(rng.normal(0, 0.05, (F, M, N_p, 3)), axis=0)
            + np.arange(F)[:, None, None, None] * np.asarray(drift)).reshape(F, M * N_p, 3)
    cell = np.floor(true / L)
    wrapped = (true - cell * L).astype(np.float32)
    return wrapped, cell.astype(int)


def test_unwrap_follows_the_chains_across_the_faces():
    L, F, M, N_p = 20.0, 12, 6, 65
    dims = np.array([L, L, L])
    pos, cell = _drifting_chains(6, F, M, N_p, L, (3.0, -2.6, 2.9))
    masses = np.random.default_rng(7).uniform(1.0, 20.0, M * N_p)
    per_chain = cell.reshape(F, M, N_p, 3)
    assert np.any(per_chain[0].max(axis=1) != per_chain[0].min(axis=1))            # a chain straddles a face in frame 0
    assert np.all((per_chain[-1] != per_chain[0]).any(axis=(1, 2)))                # every chain crosses a face
    start = pos[0].astype(np.float64) + cell[0] * L                                # frame 0, every chain whole
    margin = []
    whole = unwrap_ref(pos, start, dims, margin)
    assert min(margin) > 1e-3              # no image decision can flip on a float32-versus-float64 last bit
    np.testing.assert_allclose(whole, pos.astype(np.float64) + cell * L, atol=1e-9)     # the rule recovers the chains
    want = radii_ref(whole, masses, [M], [N_p])
    wrapped_rg = radii_ref(pos, masses, [M], [N_p])
    assert np.abs(wrapped_rg[..., 0] / want[..., 0] - 1).max() > 0.1              # without unwrap: another answer
    setup = lambda e: e.set_unwrap(dims, start)      # noqa: E731
    got, _ = engine_radii(pos, [M], [N_p], masses, setup=setup)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    two, _ = engine_radii(pos, [M], [N_p], masses, splits=[0, 5, 12], setup=setup)
    np.testing.assert_array_equal(two, got)
    many, _ = engine_radii(pos, [M], [N_p], masses, splits=list(range(F + 1)), setup=setup)
    np.testing.assert_array_equal(many, got)
    eng = _core.GyrationEngine([M], [N_p], masses)
    d = _core.DeviceArray.from_host(pos)
    try:
        eng.set_unwrap(dims, start)
        eng.accumulate(pos[:4])
        eng.reset()                                    # the unwrap state starts over from `start`
        eng.accumulate_device(d.ptr, M * N_p, F)
        np.testing.assert_array_equal(eng.result(), got)
        with pytest.raises(ValueError):
            eng.set_unwrap(dims, start)                # only before the first frame
        eng.reset()
        eng.set_unwrap(None)
        eng.accumulate(pos)
        np.testing.assert_allclose(eng.result(), wrapped_rg, rtol=RTOL, atol=0)
    finally:
        eng.close()
        d.free()


# ---------------------------------------------------------------- the class

def test_class_routes_components_and_frame_selections(tmp_path):
    from trajfiles import write_amber_netcdf
    rng = np.random.default_rng(8)
    dims = np.array([60.0, 60.0, 60.0])
    F, n_chains, n_monomers = 9, (3, 11), (65, 4)
    n_a, n_b = 3 * 65, 11 * 4
    extra = 7                                              # particles of no group, between the two groups
    a, b = walks(rng, F, 3, 65), walks(rng, F, 11, 4)
    pos = np.concatenate((b, (rng.random((F, extra, 3)) * 60).astype(np.float32), a), axis=1)
    n = pos.shape[1]
    masses = rng.uniform(1.0, 20.0, n)
    ia, ib = np.arange(n_b + extra, n), np.arange(n_b)
    order = np.concatenate((ia, ib))
    want = radii_ref(pos[:, order], masses[order], n_chains, n_monomers)
    path = tmp_path / "g.nc"
    write_amber_netcdf(path, pos, lengths=np.tile(dims, (F, 1)), angles=np.tile([90.0] * 3, (F, 1)))
    d = _core.DeviceArray.from_host(pos)
    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, box(dims), masses=masses)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, box(dims), masses=masses)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=1.0, masses=masses))):
            groups = [u.select(ia), u.select(ib)]
            g = Gyradius(groups, "atoms", n_chains, n_monomers, verbose=False).run()
            assert g.results.gyradii.shape == (2, F)
            assert g.results.units == {"results.gyradii": "angstrom"}
            np.testing.assert_allclose(g.results.gyradii, want[..., 0], rtol=RTOL, atol=0)
            c = Gyradius(groups, "atoms", n_chains, n_monomers, components=True, verbose=False).run()
            assert c.results.gyradii.shape == (2, F, 3)
            np.testing.assert_allclose(c.results.gyradii, want[..., 1:], rtol=RTOL, atol=0)
            s = Gyradius(groups, "atoms", n_chains, n_monomers, verbose=False).run(step=2)
            np.testing.assert_array_equal(s.results.gyradii, g.results.gyradii[:, ::2])
            picked = Gyradius(groups, "atoms", n_chains, n_monomers, components=True, verbose=False).run(
                frames=[7, 2, 2, 8])
            np.testing.assert_array_equal(picked.results.gyradii, c.results.gyradii[:, [7, 2, 2, 8]])
            np.testing.assert_array_equal(picked.frames, [7, 2, 2, 8])
            results[name] = (g.results.gyradii, c.results.gyradii)
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            np.testing.assert_array_equal(results[name][0], results["host"][0])
            np.testing.assert_array_equal(results[name][1], results["host"][1])
    finally:
        d.free()


def test_class_residues_and_unwrap():
    L, F, M, N_p, size = 20.0, 8, 4, 12, 3
    dims = np.array([L, L, L])
    centres, cell = _drifting_chains(9, F, M, N_p, L, (2.8, 3.1, -2.7))
    rng = np.random.default_rng(10)
    # whole monomers of 3 atoms within 0.4 A of a wrapped centre: not wrapped themselves
    pos = (centres.astype(np.float64)[:, :, None, :] + rng.uniform(-0.4, 0.4, (F, M * N_p, size, 3)))
    pos = pos.reshape(F, -1, 3).astype(np.float32)
    atom_masses = rng.uniform(1.0, 16.0, M * N_p * size)
    point_masses = atom_masses.reshape(-1, size).sum(axis=1)
    points = centres_ref(pos, size, atom_masses)
    margin = []
    whole = unwrap_ref(points, points[0] + cell[0] * L, dims, margin)
    assert min(margin) > 1e-3
    want = radii_ref(whole, point_masses, [M], [N_p])
    assert np.abs(radii_ref(points, point_masses, [M], [N_p])[..., 0] / want[..., 0] - 1).max() > 0.1
    n = pos.shape[1]
    for topo, counts in (({}, {"n_chains": M, "n_monomers": N_p}),
                         ({"resids": np.arange(n) // size, "segids": np.arange(n) // (size * N_p)}, {})):
        u = mdhelper_amd.ArrayUniverse(pos, box(dims), masses=atom_masses, **topo)
        g = Gyradius(u.atoms, "residues", unwrap=True, verbose=False, **counts).run()
        # the class makes the chains of frame 0 whole itself and may place them in another image: the radii move by
        # the rounding of x + k L only
        np.testing.assert_allclose(g.results.gyradii, want[..., 0], rtol=RTOL, atol=0)
        c = Gyradius(u.atoms, "residues", unwrap=True, components=True, verbose=False, **counts).run()
        np.testing.assert_allclose(c.results.gyradii, want[..., 1:], rtol=RTOL, atol=0)
