"""
DensityProfile / ProfileEngine on the GPU against the float64 restatement of the reference's per-frame work
(reference src/mdhelper/analysis/profile.py:775-818): positions -> (global unwrap, shift by the recentre
group's centre of mass) -> ``wrap`` -> ``numpy.histogram(x, n_bins, (0, L))`` per group and axis.  The counts
are integers and must be EQUAL (``assert_array_equal``), not close.

Where a centre of mass enters (grouped levels, ``recenter``) it is a float64 sum whose last bits depend on the
order of summation, so those tests first assert, on their own restatement, that no shifted-and-wrapped
coordinate lies within DELTA = 1e-7 Å of a bin edge (n * eps * max|x| with n <= 1e4 terms and |x| <= 1e3 Å is
2.2e-9 Å: a factor of ~45 of room), and then demand exact equality.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DensityProfile, calculate_potential_profile

pytestmark = pytest.mark.gpu

DELTA = 1e-7


# ---------------------------------------------------------------- restatement

def wrap_ref(x, L):
    x = np.array(x, dtype=np.float64)
    outside = (x < 0) | (x > L)
    with np.errstate(invalid="ignore"):
        x[outside] -= np.floor(x[outside] / L) * L
    return x


def counts_ref(points, sizes, axes, n_bins, dims, average=True):
    """points float64[F, N, 3] (already shifted, not wrapped) -> list per axis of int64 [G, n_bins] or
    [G, F, n_bins]."""
    points = np.asarray(points, dtype=np.float64)
    F = points.shape[0]
    offs = np.concatenate(([0], np.cumsum(sizes)))
    out = []
    for a, nb in zip(axes, np.broadcast_to(n_bins, (len(axes),))):
        c = np.zeros((len(sizes), F, int(nb)), dtype=np.int64)
        for g in range(len(sizes)):
            x = wrap_ref(points[:, offs[g]:offs[g + 1], a], dims[a])
            for f in range(F):
                with np.errstate(invalid="ignore"):
                    c[g, f] = np.histogram(x[f], int(nb), (0, dims[a]))[0]
        out.append(c.sum(axis=1) if average else c)
    return out


def recentre_ref(points, dims, sl, masses, target):
    """The reference's per-frame unwrap + shift (profile.py:782-801, topology.py unwrap) in float64."""
    points = np.asarray(points, dtype=np.float64)
    dims = np.asarray(dims, dtype=np.float64)
    old = points[0].copy()
    images = np.zeros(points.shape[1:], dtype=int)
    out = np.empty_like(points)
    for f in range(len(points)):
        pos = points[f].copy()
        d = pos - old
        crossed = np.abs(d) >= dims / 2
        images[crossed] -= np.sign(d[crossed]).astype(int)
        old = pos.copy()
        pos += images * dims
        scom = (masses[:, None] * pos[sl]).sum(axis=0) / masses.sum()
        pos -= np.array([0.0 if np.isnan(c) else s - c for s, c in zip(scom, target)])
        out[f] = pos
    return out


def centres_ref(pos, size, masses):
    """float64 centres of molecules of `size` consecutive rows: sequential sum in row order, one division."""
    F, N, _ = pos.shape
    p = pos.astype(np.float64).reshape(F, N // size, size, 3)
    m = np.asarray(masses, dtype=np.float64).reshape(N // size, size)
    acc = np.zeros((F, N // size, 3))
    tot = np.zeros(N // size)
    for a in range(size):
        acc = acc + m[None, :, a, None] * p[:, :, a]
        tot = tot + m[:, a]
    return acc / tot[None, :, None]


def edge_distance(points, axes, n_bins, dims):
    """Smallest distance of a wrapped coordinate to a bin edge over the requested axes."""
    best = np.inf
    for a, nb in zip(axes, np.broadcast_to(n_bins, (len(axes),))):
        x = wrap_ref(points[..., a], dims[a]).ravel()
        edges = np.linspace(0, dims[a], int(nb) + 1)
        i = np.clip(np.searchsorted(edges, x), 1, int(nb))
        best = min(best, np.minimum(np.abs(x - edges[i - 1]), np.abs(edges[i] - x)).min())
    return best


def engine_counts(pos, sizes, axes, n_bins, dims, *, per_frame=False, splits=None, **kw):
    eng = _core.ProfileEngine(sizes, axes, n_bins, dims, per_frame=per_frame, **kw)
    try:
        if splits is None:
            eng.accumulate(pos)
        else:
            for lo, hi in zip(splits[:-1], splits[1:]):
                eng.accumulate(pos[lo:hi])
        return eng.counts(), eng.stats()
    finally:
        eng.close()


def assert_counts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def box(dims):
    return [*dims, 90.0, 90.0, 90.0]


# ---------------------------------------------------------------- plain atoms

def test_edges_and_coordinates_far_outside():
    L, nb = 32.0, 64                       # width 0.5: every edge is float32-exact
    rng = np.random.default_rng(1)
    edges = np.linspace(0, L, nb + 1)
    special = np.concatenate((edges, np.nextafter(edges.astype(np.float32), np.float32(-1)),
                              np.nextafter(edges.astype(np.float32), np.float32(100)),
                              [0.0, L, -1e-20, -0.0, 1e-20, -L, 2 * L, -3 * L, 5 * L, 3 * L + 0.5, -2 * L - 0.5]))
    n = 4000
    pos = (rng.random((3, n, 3)) * 8 * L - 4 * L).astype(np.float32)      # several boxes outside on both sides
    pos[0, :len(special), 0] = special
    pos[1, :len(special), 1] = special[::-1]
    pos[2, :len(special), 2] = special
    pos[2, -1] = (np.nan, np.inf, -np.inf)                                  # not finite: not counted
    dims = (L, L, L)
    got, _ = engine_counts(pos, [n], [0, 1, 2], nb, dims)
    want = counts_ref(pos, [n], [0, 1, 2], nb, dims)
    assert_counts(got, want)
    assert sum(int(c.sum()) for c in got) == 3 * 3 * n - 3
    # x == L stays in the last bin, a tiny negative x wraps to exactly L
    one = np.zeros((1, 4, 3), dtype=np.float32)
    one[0, :, 0] = (0.0, L, -1e-20, np.nextafter(np.float32(L), np.float32(0)))
    got, _ = engine_counts(one, [4], [0], nb, dims)
    assert got[0][0, 0] == 1 and got[0][0, -1] == 3


@pytest.mark.parametrize("axes,n_bins", [("xyz", 201), ("zx", (1, 4096)), (1, 37), ((2, 0, 1), (5, 64, 500)),
                                          ("y", 4096), ((0, 1), (1, 1))])
def test_class_axes_bins_groups_scales(axes, n_bins):
    rng = np.random.default_rng(2)
    raw = np.array([20.0, 17.5, 30.0])
    scales = (2.0, 2.0, 2.0)
    dims = raw * scales
    F, n = 5, 3000
    pos = (rng.random((F, n, 3)) * dims * 3 - dims).astype(np.float32)
    u = mdhelper_amd.ArrayUniverse(pos, box(raw))
    groups = [u.select(np.arange(0, 1700)), u.select(np.arange(1700, 1701)), u.select(np.arange(1701, n))]
    dp = DensityProfile(groups, axes=axes, n_bins=n_bins, scales=scales, verbose=False).run()
    ax = dp._axes
    want = counts_ref(pos, [1700, 1, n - 1701], ax, n_bins, dims)
    V = np.prod(dims)
    for i, a in enumerate(ax):
        nb = want[i].shape[-1]
        np.testing.assert_array_equal(dp.results.number_densities[i], want[i] * (nb / V / F))
        np.testing.assert_array_equal(dp.results.bins[i],
                                      np.linspace(dims[a] / (2 * nb), dims[a] - dims[a] / (2 * nb), nb))


def test_frame_selections_and_per_frame_results():
    rng = np.random.default_rng(3)
    dims = np.array([12.0, 15.0, 9.0])
    F, n = 23, 500
    pos = (rng.random((F, n, 3)) * dims * 2 - dims / 2).astype(np.float32)
    u = mdhelper_amd.ArrayUniverse(pos, box(dims), dt=0.25)
    sizes = [200, 300]
    groups = [u.select(np.arange(200)), u.select(np.arange(200, n))]
    V = np.prod(dims)
    for kw, sel in (({"step": 3}, np.arange(0, F, 3)), ({"start": 4, "stop": 19}, np.arange(4, 19)),
                    ({"frames": [7, 2, 2, 20]}, np.array([7, 2, 2, 20]))):
        dp = DensityProfile(groups, axes="xz", n_bins=(40, 11), verbose=False).run(**kw)
        want = counts_ref(pos[sel], sizes, [0, 2], (40, 11), dims)
        for i, nb in enumerate((40, 11)):
            np.testing.assert_array_equal(dp.results.number_densities[i], want[i] * (nb / V / len(sel)))
        dp = DensityProfile(groups, axes="xz", n_bins=(40, 11), average=False, verbose=False).run(**kw)
        want = counts_ref(pos[sel], sizes, [0, 2], (40, 11), dims, average=False)
        for i, nb in enumerate((40, 11)):
            assert dp.results.number_densities[i].shape == (2, len(sel), nb)
            np.testing.assert_array_equal(dp.results.number_densities[i], want[i] * (nb / V))
        np.testing.assert_array_equal(dp.results.times, sel * 0.25)
        assert dp.results.units["results.times"] == "picosecond"


# ---------------------------------------------------------------- routes and engine behaviour

def test_ingest_routes_agree(tmp_path):
    from trajfiles import write_amber_netcdf
    rng = np.random.default_rng(4)
    dims = np.array([15.0, 18.0, 21.0])
    F, n = 9, 1203                                         # 3 n not a multiple of 4: unaligned frames in HBM
    pos = (rng.random((F, n, 3)) * dims * 2 - dims / 2).astype(np.float32)
    path = tmp_path / "p.nc"
    write_amber_netcdf(path, pos, lengths=np.tile(dims, (F, 1)), angles=np.tile([90.0] * 3, (F, 1)))
    d = _core.DeviceArray.from_host(pos)
    try:
        universes = {"host": mdhelper_amd.ArrayUniverse(pos, box(dims)),
                     "hbm": mdhelper_amd.ArrayUniverse.from_device(d, box(dims)),
                     "file": mdhelper_amd.FileUniverse(path, dt=1.0)}
        pick = np.concatenate((np.arange(900, 1100), np.arange(0, 350)))      # a gather, out of order
        for average in (True, False):
            want_all = counts_ref(pos, [n], [0, 1, 2], 50, dims, average=average)
            want_sel = counts_ref(pos[:, pick], [200, 350], [2, 1], (33, 7), dims, average=average)
            for name, u in universes.items():
                dp = DensityProfile(u.atoms, n_bins=50, average=average, verbose=False)
                got = _run_counts(dp)
                assert_counts(got, want_all)
                dp = DensityProfile([u.select(pick[:200]), u.select(pick[200:])], axes="zy", n_bins=(33, 7),
                                    average=average, verbose=False)
                assert_counts(_run_counts(dp), want_sel)
    finally:
        d.free()


def _run_counts(dp, **kw):
    """Integer counts behind the densities of a run: the engine's, captured before the class scales them."""
    seen = {}
    conclude = dp._conclude

    def spy():
        counts = dp._engine.counts
        dp._engine.counts = lambda: seen.setdefault("c", counts())
        conclude()

    dp._conclude = spy
    dp.run(**kw)
    return seen["c"]


def test_split_calls_reset_and_per_frame_rows():
    rng = np.random.default_rng(5)
    dims = (10.0, 11.0, 12.0)
    F, n = 150, 700                                         # 150 frames: the per-frame row buffer grows twice
    pos = (rng.random((F, n, 3)) * 30 - 10).astype(np.float32)
    sizes = [300, 400]
    for per_frame in (False, True):
        want = counts_ref(pos, sizes, [0, 1, 2], (20, 30, 40), dims, average=not per_frame)
        once, _ = engine_counts(pos, sizes, [0, 1, 2], (20, 30, 40), dims, per_frame=per_frame)
        assert_counts(once, want)
        split, st = engine_counts(pos, sizes, [0, 1, 2], (20, 30, 40), dims, per_frame=per_frame,
                                  splits=[0, 1, 2, 40, 41, 149, 150])
        assert_counts(split, want)
        assert st["frames"] == F
    eng = _core.ProfileEngine(sizes, [1], 30, dims)
    try:
        eng.accumulate(pos[:10])
        eng.reset()
        assert eng.stats()["frames"] == 0 and int(eng.counts()[0].sum()) == 0
        eng.accumulate(pos[10:30])
        assert_counts(eng.counts(), counts_ref(pos[10:30], sizes, [1], 30, dims))
        with pytest.raises(ValueError):
            eng.accumulate(pos[:, :50])                     # wrong number of rows
    finally:
        eng.close()


# ---------------------------------------------------------------- sizes

def test_fullsize_exact():
    rng = np.random.default_rng(6)
    dims = (64.0, 60.0, 71.0)
    F, n = 64, 32768
    pos = (rng.random((F, n, 3)) * np.array(dims) * 1.5 - np.array(dims) * 0.25).astype(np.float32)
    for sizes, replicas in (([n], 8), ([10000, 22768], 4)):
        got, st = engine_counts(pos, sizes, [0, 1, 2], 201, dims)
        assert st["replicas"] == replicas
        assert_counts(got, counts_ref(pos, sizes, [0, 1, 2], 201, dims))


@pytest.mark.parametrize("n_bins,replicas", [(500, 4), (1200, 2), (4000, 1), (20000, 0)])
def test_slot_counts_beyond_the_lds_budget(n_bins, replicas):
    """The replica count steps down with the slot count and finally the kernels bin straight into global
    memory: 4 groups x 3 axes x 20 000 bins = 240 000 slots."""
    rng = np.random.default_rng(7)
    dims = (30.0, 40.0, 50.0)
    sizes = [1000, 1, 2500, 499] if n_bins == 20000 else [4000]
    n = sum(sizes)
    pos = (rng.random((6, n, 3)) * 100 - 25).astype(np.float32)
    for per_frame in (False, True):
        got, st = engine_counts(pos, sizes, [0, 1, 2], n_bins, dims, per_frame=per_frame)
        assert st["replicas"] == replicas
        assert_counts(got, counts_ref(pos, sizes, [0, 1, 2], n_bins, dims, average=not per_frame))


@pytest.mark.parametrize("forced", [0, 1, 2, 4])
def test_forced_replica_counts_agree(forced):
    rng = np.random.default_rng(8)
    dims = (20.0, 20.0, 20.0)
    pos = (rng.random((4, 5000, 3)) * 20).astype(np.float32)
    got, st = engine_counts(pos, [2000, 3000], [0, 1, 2], 201, dims, replicas=forced)
    assert st["replicas"] == forced
    assert_counts(got, counts_ref(pos, [2000, 3000], [0, 1, 2], 201, dims))


def test_slab_with_most_particles_in_three_bins():
    rng = np.random.default_rng(9)
    dims = (40.0, 40.0, 80.0)
    F, n = 16, 20000
    pos = (rng.random((F, n, 3)) * np.array(dims)).astype(np.float32)
    w = dims[2] / 201
    dense = rng.random(n) < 0.93
    pos[:, dense, 2] = (100 * w + rng.random((F, int(dense.sum()))) * 3 * w).astype(np.float32)
    want = counts_ref(pos, [n], [0, 1, 2], 201, dims)
    assert want[2][0, 100:103].sum() > 0.9 * F * n
    got, _ = engine_counts(pos, [n], [0, 1, 2], 201, dims)
    assert_counts(got, want)


# ---------------------------------------------------------------- grouped levels and recenter

def _drifting(seed, F, n, dims, drift):
    """Particles that diffuse and drift together, so that they and any group's centre cross the boundary;
    stored wrapped into [0, L), as float32."""
    rng = np.random.default_rng(seed)
    start = rng.random((1, n, 3)) * dims
    walk = np.cumsum(rng.normal(0, 0.4, (F, n, 3)), axis=0) + np.arange(F)[:, None, None] * np.asarray(drift)
    return np.mod(start + walk, dims).astype(np.float32)


@pytest.mark.parametrize("form", ["int", "group", "target_nan"])
def test_recenter_atoms(form):
    dims = np.array([40.0, 35.0, 60.0])
    F, n, n_bins = 20, 6000, (201, 64, 500)
    pos = _drifting(0, F, n, dims, (1.9, -1.3, 2.7))
    masses = np.random.default_rng(10).uniform(1, 20, n)
    u = mdhelper_amd.ArrayUniverse(pos, box(dims), masses=masses)
    groups = [u.select(np.arange(2000)), u.select(np.arange(2000, n))]
    target = dims / 2
    if form == "int":
        recenter = 0
    elif form == "group":
        recenter = groups[0]
    else:
        target = np.array([7.5, np.nan, 41.25])
        recenter = (0, target)
    shifted = recentre_ref(pos, dims, slice(0, 2000), masses[:2000], target)
    held = ~np.isnan(target)
    assert np.abs(np.diff(shifted[:, :2000].mean(axis=1), axis=0))[:, held].max() < 1.0   # held in place
    assert (np.abs(pos[1:].astype(float) - pos[:-1]) >= dims / 2).any()              # particles do cross
    assert edge_distance(shifted, [0, 1, 2], n_bins, dims) > DELTA
    for average in (True, False):
        want = counts_ref(shifted, [2000, n - 2000], [0, 1, 2], n_bins, dims, average=average)
        dp = DensityProfile(groups, n_bins=n_bins, recenter=recenter, average=average, verbose=False)
        got = _run_counts(dp)
        assert_counts(got, want)
        if not average:       # every group's counts sum to its size in every frame
            for c in got:
                np.testing.assert_array_equal(c.sum(axis=-1), np.repeat([[2000], [n - 2000]], F, axis=1))


def test_recenter_does_not_depend_on_the_split_into_calls():
    dims = np.array([25.0, 30.0, 20.0])
    F, n, n_bins = 30, 2500, (100, 201, 77)
    pos = _drifting(11, F, n, dims, (-2.1, 1.7, 0.9))
    masses = np.random.default_rng(12).uniform(1, 5, 1000)
    target = np.array([3.0, 29.0, np.nan])
    shifted = recentre_ref(pos, dims, slice(1500, 2500), masses, target)
    assert edge_distance(shifted, [0, 1, 2], n_bins, dims) > DELTA
    want = counts_ref(shifted, [1500, 1000], [0, 1, 2], n_bins, dims, average=False)
    for splits in (None, [0, 1, 2, 17, 29, 30], list(range(F + 1))):
        eng = _core.ProfileEngine([1500, 1000], [0, 1, 2], n_bins, dims, per_frame=True)
        try:
            eng.set_recenter(1, masses, target)
            cuts = splits or [0, F]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                eng.accumulate(pos[lo:hi])
            assert_counts(eng.counts(), want)
            eng.reset()                                     # the unwrap state starts over
            eng.accumulate(pos)
            assert_counts(eng.counts(), want)
        finally:
            eng.close()


@pytest.mark.parametrize("grouping", ["residues", "segments"])
@pytest.mark.parametrize("recenter", [False, True])
def test_grouped_levels(grouping, recenter, tmp_path):
    from trajfiles import write_amber_netcdf
    dims = np.array([30.0, 26.0, 34.0])
    F, n_mol, size, n_bins = 12, 900, 4, (64, 201, 90)
    rng = np.random.default_rng(13)
    # whole molecules (atoms within 1 Å of a wrapped, drifting centre: not wrapped themselves, as the
    # reference asks for grouped levels)
    centres = _drifting(14, F, n_mol, dims, (1.1, -2.3, 1.6)).astype(np.float64)
    pos = (centres[:, :, None, :] + rng.uniform(-1, 1, (F, n_mol, size, 3))).reshape(F, n_mol * size, 3)
    pos = pos.astype(np.float32)
    n = n_mol * size
    masses = rng.uniform(1, 16, n)
    ids = np.repeat(np.arange(n_mol), size)
    topo = {"resids": ids} if grouping == "residues" else {"segids": ids}
    com = centres_ref(pos, size, masses)
    sizes = [500, n_mol - 500]
    mol_mass = masses.reshape(n_mol, size).sum(axis=1)
    points = recentre_ref(com, dims, slice(500, n_mol), mol_mass[500:], dims / 2) if recenter else com
    assert edge_distance(points, [0, 1, 2], n_bins, dims) > DELTA
    want = counts_ref(points, sizes, [0, 1, 2], n_bins, dims, average=False)
    path = tmp_path / "g.nc"
    write_amber_netcdf(path, pos, lengths=np.tile(dims, (F, 1)), angles=np.tile([90.0] * 3, (F, 1)))
    d = _core.DeviceArray.from_host(pos)
    try:
        for u in (mdhelper_amd.ArrayUniverse(pos, box(dims), masses=masses, **topo),
                  mdhelper_amd.ArrayUniverse.from_device(d, box(dims), masses=masses, **topo),
                  mdhelper_amd.FileUniverse(path, dt=1.0, masses=masses, **topo)):
            groups = [u.select(np.arange(500 * size)), u.select(np.arange(500 * size, n))]
            dp = DensityProfile(groups, grouping, n_bins=n_bins, average=False,
                                recenter=1 if recenter else None, verbose=False)
            got = _run_counts(dp)
            assert_counts(got, want)
            for c in got:
                np.testing.assert_array_equal(c.sum(axis=-1), np.repeat([[500], [n_mol - 500]], F, axis=1))
    finally:
        d.free()


def test_mixed_groupings():
    dims = np.array([18.0, 18.0, 24.0])
    rng = np.random.default_rng(15)
    F, n_mol, size, n_ions = 6, 300, 3, 450
    centres = rng.random((F, n_mol, 1, 3)) * dims
    water = (centres + rng.uniform(-0.8, 0.8, (F, n_mol, size, 3))).reshape(F, n_mol * size, 3)
    ions = rng.random((F, n_ions, 3)) * dims * 1.2 - 0.1 * dims
    pos = np.concatenate((ions, water), axis=1).astype(np.float32)
    n = pos.shape[1]
    masses = np.concatenate((np.full(n_ions, 23.0), np.tile([16.0, 1.008, 1.008], n_mol)))
    resids = np.concatenate((np.arange(n_ions), n_ions + np.repeat(np.arange(n_mol), size)))
    u = mdhelper_amd.ArrayUniverse(pos, box(dims), masses=masses, resids=resids)
    groups = [u.select(np.arange(n_ions)), u.select(np.arange(n_ions, n))]
    points = np.concatenate((pos[:, :n_ions].astype(np.float64),
                             centres_ref(pos[:, n_ions:], size, masses[n_ions:])), axis=1)
    assert edge_distance(points, [2, 0], (150, 40), dims) > DELTA
    dp = DensityProfile(groups, ("atoms", "residues"), axes="zx", n_bins=(150, 40), verbose=False)
    assert_counts(_run_counts(dp), counts_ref(points, [n_ions, n_mol], [2, 0], (150, 40), dims))


# ---------------------------------------------------------------- charges

def test_charge_densities_and_potential_method():
    rng = np.random.default_rng(16)
    dims = np.array([20.0, 20.0, 50.0])
    F, n = 8, 4000
    pos = (rng.random((F, n, 3)) * dims).astype(np.float32)
    pos[:, :2000, 2] = (rng.normal(8, 2, (F, 2000)) % 50).astype(np.float32)
    pos[:, 2000:, 2] = (rng.normal(42, 2, (F, 2000)) % 50).astype(np.float32)
    charges = np.concatenate((np.full(2000, 1.0), np.full(2000, -1.0)))
    u = mdhelper_amd.ArrayUniverse(pos, box(dims), charges=charges)
    groups = [u.select(np.arange(2000)), u.select(np.arange(2000, n))]
    want = counts_ref(pos, [2000, 2000], [2, 0], (201, 50), dims)
    for kw in ({}, {"charges": [2.0, -0.5]}):
        q = np.asarray(kw.get("charges", [1.0, -1.0]))
        for average in (True, False):
            dp = DensityProfile(groups, axes="zx", n_bins=(201, 50), reduced=True, average=average,
                                verbose=False, **kw).run()
            for i in range(2):
                nd = dp.results.number_densities[i]
                # [G, n_bins] -> [n_bins]; per frame [G, F, n_bins] -> [F, n_bins], frame by frame the same sum
                want_q = (np.einsum("g,...gb->...b", q, nd) if average
                          else np.stack([np.einsum("g,...gb->...b", q, nd[:, f]) for f in range(F)]))
                np.testing.assert_array_equal(dp.results.charge_densities[i], want_q)
            if average:
                np.testing.assert_array_equal(dp.results.number_densities[0],
                                              want[0] * (201 / np.prod(dims) / F))
            assert dp.results.units["results.charge_densities"] == "elementary_charge/angstrom^3"
            rho = dp.results.charge_densities[0]
            rho = rho if average else rho.mean(axis=0)
            for pk in ({"sigma_q": 0.01}, {"dV": 0.3, "method": "matrix"}, {"sigma_q": 0.0, "V0": 0.2}):
                dp.calculate_potential_profile(3.0, "z", **pk)
                np.testing.assert_array_equal(
                    dp.results.potentials[0],
                    calculate_potential_profile(dp.results.bins[0], rho, dims[2], 3.0, reduced=True, **pk))
            assert dp.results.units["results.potentials"] == "volt"
