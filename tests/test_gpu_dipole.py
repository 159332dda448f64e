"""
DipoleMoment / DipoleEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_dipole_device.hpp): per frame, group and component

    M = sum over the group's points of  q * (x + image * L),      x the float32 coordinate widened to float64,

image from the reference's global unwrap rule (algorithm/topology.py `unwrap`) restated frame by frame below.

Tolerance.  The restatement forms the terms q * (x + image * L) with the same elementwise float64 operations as the
device (the unit is built with contraction off), so the terms are bit-equal on both sides and only the order of the
sum differs.  The restatement adds them with ``math.fsum`` (correctly rounded); the device adds n terms in its fixed
order.  Any order of n float64 additions is within (n - 1) 2^-53 sum|t_i| of the exact sum, hence, per frame, group
and component,

    |device - ref| <= n * 2^-52 * sum_i |q_i x_id|,      n the group's size.

Nothing in it is measured, and no rtol applies to the result itself: charges of both signs cancel.  Outputs that must
not depend on the route, on the split into calls or slabs, or on a reset are compared with ``assert_array_equal``.
"""
import math

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import DipoleMoment, calculate_relative_permittivity
from mdhelper_amd.universe import box_volumes

pytestmark = pytest.mark.gpu

T = _core.DipoleEngine.TILE


# ---------------------------------------------------------------- restatement

def unwrap_ref(points, start, dims):
    """The reference's rule frame by frame from `start`: d = x - x_prev; |d| >= dims / 2 moves the image count by
    -sign(d); x_prev becomes the raw x.  points float32[F, n, 3] -> image counts int[F, n, 3]."""
    points = np.asarray(points).astype(np.float64)
    dims = np.asarray(dims, dtype=np.float64)
    old = np.array(start, dtype=np.float64)
    images = np.zeros(points.shape[1:], dtype=int)
    out = np.empty(points.shape, dtype=int)
    for f in range(len(points)):
        d = points[f] - old
        crossed = np.abs(d) >= dims / 2
        images[crossed] -= np.sign(d[crossed]).astype(int)
        old = points[f].copy()
        out[f] = images
    return out


def terms_ref(pos, q, images=None, dims=None):
    """float64[F, n, 3]: q * (x + image * L), one operation at a time as the device does them."""
    x = np.asarray(pos).astype(np.float64)
    if images is not None:
        x = x + images.astype(np.float64) * np.asarray(dims, dtype=np.float64)
    return np.asarray(q, dtype=np.float64)[None, :, None] * x


def sums_ref(terms, sizes):
    """(dipoles [G, F, 3] by math.fsum, tolerance [G, F, 3] = n 2^-52 sum|t|)."""
    F = terms.shape[0]
    out, tol, lo = np.empty((len(sizes), F, 3)), np.empty((len(sizes), F, 3)), 0
    for g, n in enumerate(sizes):
        for f in range(F):
            for d in range(3):
                t = terms[f, lo:lo + n, d]
                out[g, f, d] = math.fsum(t)
                tol[g, f, d] = n * 2.0 ** -52 * math.fsum(np.abs(t))
        lo += n
    return out, tol


def assert_within(got, want, tol):
    assert got.shape == want.shape
    worst = np.abs(got - want) - tol
    assert np.all(worst <= 0), f"largest excess over the bound {worst.max():.3e} (bound there " \
                               f"{tol.ravel()[worst.argmax()]:.3e})"


def engine_rows(pos, sizes, q, *, splits=None, setup=None):
    eng = _core.DipoleEngine(sizes, q)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return eng.result()
    finally:
        eng.close()


def box(dims):
    return [*dims, 90.0, 90.0, 90.0]


def charges_for(rng, n):
    """Non-uniform charges of both signs."""
    return rng.normal(size=n) * rng.choice([0.2, 1.0, 3.0], n)


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_engine_group_sizes_and_frame_counts(n):
    rng = np.random.default_rng(100 + n)
    q = charges_for(rng, n)
    for F in (1, 2, 37):
        pos = rng.uniform(-300.0, 300.0, (F, n, 3)).astype(np.float32)
        got = engine_rows(pos, [n], q)
        want, tol = sums_ref(terms_ref(pos, q), [n])
        assert got.shape == (1, F, 3)
        assert_within(got, want, tol)
    if n == 1:
        np.testing.assert_array_equal(got, want)          # one term: nothing to round


def test_engine_three_unequal_groups():
    rng = np.random.default_rng(7)
    sizes = [1, 65, T + 1]
    n, F = sum(sizes), 37
    q = charges_for(rng, n)
    pos = rng.uniform(0.0, 400.0, (F, n, 3)).astype(np.float32)
    got = engine_rows(pos, sizes, q)
    want, tol = sums_ref(terms_ref(pos, q), sizes)
    assert_within(got, want, tol)
    assert np.all(np.abs(got[1:]).max(axis=(1, 2)) > 1.0)
    # the sum of a group does not depend on what the other groups are: the tiles never span two groups
    for g, (lo, hi) in enumerate(((0, 1), (1, 66), (66, n))):
        np.testing.assert_array_equal(engine_rows(pos[:, lo:hi], [hi - lo], q[lo:hi])[0], got[g])
    with pytest.raises(ValueError):
        engine_rows(pos[:, :50], sizes, q)                 # wrong number of rows


def _walk(seed, F, n, dims):
    """A random walk with steps of about L / 5 per frame, wrapped into the box: (float32[F, n, 3] in [0, L),
    start float64[n, 3] = the first frame shifted by whole images for part of the points)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, 1.0, (F, n, 3)) * dims / 5, axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    shift = rng.integers(-2, 3, (n, 3)) * (rng.random((n, 1)) < 0.4)
    return wrapped, wrapped[0].astype(np.float64) + shift * dims


UNWRAP_DIMS = np.array([31.0, 44.5, 57.25])
UNWRAP_SIZES = [1, 65, T + 1]
UNWRAP_SEED = 11


@pytest.fixture(scope="module")
def walk():
    """Frames, charges, start and the restatement with and without unwrap, shared and left unchanged."""
    n, F = sum(UNWRAP_SIZES), 37
    pos, start = _walk(UNWRAP_SEED, F, n, UNWRAP_DIMS)
    q = charges_for(np.random.default_rng(12), n)
    images = unwrap_ref(pos, start, UNWRAP_DIMS)
    want, tol = sums_ref(terms_ref(pos, q, images, UNWRAP_DIMS), UNWRAP_SIZES)
    wrapped, wtol = sums_ref(terms_ref(pos, q), UNWRAP_SIZES)
    for a in (pos, start, q, images, want, tol, wrapped, wtol):
        a.setflags(write=False)
    return {"pos": pos, "start": start, "q": q, "images": images, "want": want, "tol": tol, "wrapped": wrapped,
            "wtol": wtol}


def test_unwrap_input_cannot_pass_with_the_unwrap_off(walk):
    """What the test asserts of its own input, so that the unwrap cases mean something."""
    images = walk["images"]
    steps = np.diff(np.concatenate((np.zeros((1,) + images.shape[1:], dtype=int), images)), axis=0)
    for d in range(3):
        assert (steps[..., d] == 1).any() and (steps[..., d] == -1).any()      # crossings of both signs
    assert np.abs(images).max() >= 2
    assert np.abs(steps).max() == 1
    assert (np.abs(walk["start"] - walk["pos"][0]) > 1.0).any(axis=1).mean() > 0.2   # part of the points start shifted
    excess = np.abs(walk["want"] - walk["wrapped"]) / walk["tol"]
    assert np.all(excess.max(axis=1) > 100)                # every group and component, at some frame


def test_unwrap_against_the_rule(walk):
    setup = lambda e: e.set_unwrap(UNWRAP_DIMS, walk["start"])      # noqa: E731
    got = engine_rows(walk["pos"], UNWRAP_SIZES, walk["q"], setup=setup)
    assert_within(got, walk["want"], walk["tol"])
    off = engine_rows(walk["pos"], UNWRAP_SIZES, walk["q"])
    assert_within(off, walk["wrapped"], walk["wtol"])
    eng = _core.DipoleEngine(UNWRAP_SIZES, walk["q"])
    try:
        eng.set_unwrap(UNWRAP_DIMS, walk["start"])
        eng.accumulate(walk["pos"][:4])
        with pytest.raises(ValueError):
            eng.set_unwrap(UNWRAP_DIMS, walk["start"])     # only before the first frame
        eng.reset()
        eng.set_unwrap(None)
        eng.accumulate(walk["pos"])
        np.testing.assert_array_equal(eng.result(), off)
    finally:
        eng.close()


@pytest.mark.parametrize("unwrap", [False, True])
def test_one_set_of_bits_whatever_the_split_slab_route_or_index(walk, unwrap, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, q, sizes = walk["pos"], walk["q"], UNWRAP_SIZES
    F, n = pos.shape[:2]

    def setup(e, slab=None):
        if unwrap:
            e.set_unwrap(UNWRAP_DIMS, walk["start"])
        if slab is not None:
            e.set_slab_frames(slab)

    once = engine_rows(pos, sizes, q, setup=setup)
    assert_within(once, walk["want" if unwrap else "wrapped"], walk["tol" if unwrap else "wtol"])
    np.testing.assert_array_equal(engine_rows(pos, sizes, q, splits=[0, 1, 5, 37], setup=setup), once)
    np.testing.assert_array_equal(engine_rows(pos, sizes, q, setup=lambda e: setup(e, 8)), once)
    np.testing.assert_array_equal(engine_rows(pos, sizes, q, splits=[0, 1, 5, 37], setup=lambda e: setup(e, 8)),
                                  once)

    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    rng = np.random.default_rng(13)
    n_total = 2 * n + 5
    index = rng.permutation(n_total)[:n]
    assert np.any(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    big = rng.uniform(0.0, 30.0, (F, n_total, 3)).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.tile(UNWRAP_DIMS, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.DipoleEngine(sizes, q)
    try:
        setup(eng)
        eng.accumulate_device(d.ptr, n, F)
        np.testing.assert_array_equal(eng.result(), once)                       # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.result().shape == (3, 0, 3)
        eng.accumulate_traj(tf, np.arange(F))
        np.testing.assert_array_equal(eng.result(), once)                       # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        np.testing.assert_array_equal(eng.result(), once)                       # HBM through the index
        with pytest.raises(ValueError):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))      # out of range
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        np.testing.assert_array_equal(eng.result(), once)                       # file through the index
        eng.reset()
        eng.set_slab_frames(8)
        eng.accumulate_device(d.rows(0, 5).ptr, n, 5)                           # routes mixed within one pass
        eng.accumulate(pos[5:20])
        eng.accumulate_traj(tf, np.arange(20, F))
        np.testing.assert_array_equal(eng.result(), once)
        eng.reset()
        eng.set_slab_frames(0)                                                   # the default again
        eng.accumulate(pos)
        np.testing.assert_array_equal(eng.result(), once)
        with pytest.raises(ValueError):
            eng.set_slab_frames(-1)
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


# ---------------------------------------------------------------- the class

def _electrolyte(seed=20, F=9):
    """Cations, three particles of no group, anions: (pos float32[F, n, 3], boxes float32[F, 6], charges, ia, ib)."""
    rng = np.random.default_rng(seed)
    n_c, extra, n_a = 70, 3, T + 5
    n = n_c + extra + n_a
    lengths = np.array([30.0, 40.0, 50.0]) + 0.25 * np.arange(F)[:, None]          # exact in float32
    pos = (rng.random((F, n, 3)) * lengths[:, None, :]).astype(np.float32)
    boxes = np.hstack((lengths, np.full((F, 3), 90.0))).astype(np.float32)
    q = np.concatenate((rng.uniform(0.5, 1.5, n_c), np.zeros(extra), -rng.uniform(0.5, 1.5, n_a)))
    return pos, boxes, q, np.arange(n_c), np.arange(n_c + extra, n)


def test_class_groups_routes_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    pos, boxes, q, ia, ib = _electrolyte()
    F, n = pos.shape[:2]
    order = np.concatenate((ib, ia))                       # anions first: not the order of the frame
    want, tol = sums_ref(terms_ref(pos[:, order], q[order]), [len(ib), len(ia)])
    all_want, all_tol = sums_ref(terms_ref(pos, q), [n])
    path = tmp_path / "e.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5, charges=q)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5, charges=q)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5, charges=q))):
            groups = [u.select(ib), u.select(ia)]
            two = DipoleMoment(groups, verbose=False).run()
            assert two.results.dipoles.shape == (F, 2, 3)
            assert_within(two.results.dipoles.transpose(1, 0, 2), want, tol)
            np.testing.assert_array_equal(two.results.volumes, box_volumes(boxes))
            np.testing.assert_array_equal(two.results.times, 0.5 * np.arange(F))
            assert two.results.units == {"results.dipoles": "elementary_charge*angstrom",
                                         "results.volumes": "angstrom^3", "results.times": "picosecond"}
            one = DipoleMoment(u.atoms, verbose=False).run()                      # every particle in order: no index
            assert one.results.dipoles.shape == (F, 1, 3)
            assert_within(one.results.dipoles.transpose(1, 0, 2), all_want, all_tol)
            s = DipoleMoment(groups, verbose=False).run(step=2)
            np.testing.assert_array_equal(s.results.dipoles, two.results.dipoles[::2])
            np.testing.assert_array_equal(s.results.volumes, box_volumes(boxes)[::2])
            np.testing.assert_array_equal(s.results.times, 2 * 0.5 * np.arange(5))
            picked = DipoleMoment(groups, parallel=True, verbose=False).run(frames=[7, 2, 2, 8])
            np.testing.assert_array_equal(picked.results.dipoles, two.results.dipoles[[7, 2, 2, 8]])
            np.testing.assert_array_equal(picked.results.volumes, box_volumes(boxes)[[7, 2, 2, 8]])
            np.testing.assert_array_equal(picked.results.times, 0.5 * np.arange(4))
            avg = DipoleMoment(groups, average=True, verbose=False).run()
            assert avg.results.dipoles.shape == (2, 3) and np.ndim(avg.results.volumes) == 0
            np.testing.assert_array_equal(avg.results.dipoles, two.results.dipoles.mean(axis=0))
            assert avg.results.volumes == box_volumes(boxes).mean() and "times" not in avg.results
            results[name] = (two.results.dipoles, one.results.dipoles, two.results.volumes)
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            for got, host in zip(results[name], results["host"]):
                np.testing.assert_array_equal(got, host)
        # a reader without block access goes frame by frame through the batcher
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5, charges=q)
        slow = per_frame(DipoleMoment([u.select(ib), u.select(ia)], verbose=False)).run()
        np.testing.assert_array_equal(slow.results.dipoles, results["host"][0])
        np.testing.assert_array_equal(slow.results.volumes, results["host"][2])
    finally:
        d.free()


class HalfOfTwoRanks:
    """A communicator of two ranks whose all-reduce adds nothing: what comes back is this rank's share."""
    world_size = 2
    device_collectives = False

    def __init__(self, rank):
        self.rank = rank

    def allreduce(self, arr, op="sum"):
        assert op == "sum"
        return np.asarray(arr)


def test_class_charge_forms_and_frame_shards():
    pos, boxes, _, ia, ib = _electrolyte(seed=21)
    n = pos.shape[1]
    q = np.zeros(n)
    q[ia], q[ib] = 2.0, -1.0
    u = mdhelper_amd.ArrayUniverse(pos, boxes, charges=q)
    bare = mdhelper_amd.ArrayUniverse(pos, boxes)
    from_universe = DipoleMoment([u.select(ia), u.select(ib)], verbose=False).run().results.dipoles
    scalars = DipoleMoment([bare.select(ia), bare.select(ib)], charges=[2.0, -1], verbose=False).run()
    arrays = DipoleMoment([bare.select(ia), bare.select(ib)], charges=[q[ia], q[ib]], verbose=False).run()
    np.testing.assert_array_equal(scalars.results.dipoles, from_universe)
    np.testing.assert_array_equal(arrays.results.dipoles, from_universe)
    want, tol = sums_ref(terms_ref(pos[:, np.concatenate((ia, ib))], q[np.concatenate((ia, ib))]), [len(ia), len(ib)])
    assert_within(from_universe.transpose(1, 0, 2), want, tol)
    # frames shard across ranks: each rank's rows inside a zero-filled array, one all-reduce
    shares = [DipoleMoment([u.select(ia), u.select(ib)], verbose=False, comm=HalfOfTwoRanks(r)).run().results.dipoles
              for r in (0, 1)]
    assert np.all(shares[0][5:] == 0) and np.all(shares[1][:5] == 0)
    np.testing.assert_array_equal(shares[0] + shares[1], from_universe)


def test_class_scales_change_the_unwrap_lengths_and_nothing_else(walk):
    pos, q = walk["pos"], walk["q"]
    F, n = pos.shape[:2]
    u = mdhelper_amd.ArrayUniverse(pos, box(UNWRAP_DIMS), charges=q)             # no bonds: start = the first frame
    plain = DipoleMoment(u.atoms, verbose=False).run()
    scaled = DipoleMoment(u.atoms, scales=(1, 1, 2), verbose=False).run()
    np.testing.assert_array_equal(scaled.results.dipoles, plain.results.dipoles)
    np.testing.assert_array_equal(scaled.results.volumes, np.full(F, box_volumes(box(UNWRAP_DIMS))[0]))
    for scales in (1, (1, 1, 2)):
        dims = UNWRAP_DIMS * scales
        images = unwrap_ref(pos, pos[0].astype(np.float64), dims)
        want, tol = sums_ref(terms_ref(pos, q, images, dims), [n])
        got = DipoleMoment(u.atoms, scales=scales, unwrap=True, verbose=False).run()
        assert_within(got.results.dipoles.transpose(1, 0, 2), want, tol)
        np.testing.assert_array_equal(got.results.volumes, plain.results.volumes)
        np.testing.assert_array_equal(
            DipoleMoment(u.atoms, dimensions=UNWRAP_DIMS, scales=scales, unwrap=True, verbose=False).run()
            .results.dipoles, got.results.dipoles)
        if scales == 1:
            first = got.results.dipoles
    assert np.abs(got.results.dipoles[..., 2] - first[..., 2]).max() > 1.0        # z follows the doubled length
    np.testing.assert_array_equal(got.results.dipoles[..., :2], first[..., :2])   # x and y do not


GRID = 1024.0       # coordinates, translations and box lengths on a grid of 1/1024 Å are exact in float32 and float64


def _molecules(seed, n_mol, F=1):
    """Three-atom molecules on the grid: float64[F, 3 n_mol, 3] (whole), resids, bonds."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 16 * 1024, (1, n_mol, 1, 3))
    arms = rng.integers(-1536, 1536, (1, n_mol, 3, 3))             # bond vectors under 1.5 Å per component
    arms[:, :, 0] = 0
    pos = (centre + arms + np.zeros((F, 1, 1, 1), dtype=int)).reshape(F, 3 * n_mol, 3) / GRID
    first = 3 * np.arange(n_mol)
    bonds = np.concatenate((np.stack((first, first + 1), axis=1), np.stack((first, first + 2), axis=1)))
    return pos, np.repeat(np.arange(n_mol), 3), bonds


def test_class_neutralize_makes_charged_molecules_translation_invariant():
    n_mol, F = 60, 3
    rng = np.random.default_rng(31)
    pos, resids, _ = _molecules(30, n_mol, F)
    pos = pos + rng.integers(-2048, 2048, (F, 1, 3)) / GRID * np.arange(F)[:, None, None]
    q = np.tile([0.9, -0.3, 0.2], n_mol) * rng.uniform(0.5, 2.0, 3 * n_mol)         # every molecule charged
    masses = rng.uniform(1.0, 16.0, 3 * n_mol)
    shift = np.repeat(rng.integers(-20 * 1024, 20 * 1024, (n_mol, 3)), 3, axis=0) / GRID   # one vector per molecule
    moved = pos + shift
    for a in (pos, moved):
        np.testing.assert_array_equal(a.astype(np.float32).astype(np.float64), a)   # nothing is rounded away
    dims = [40.0, 40.0, 40.0]

    def run(p, neutralize):
        u = mdhelper_amd.ArrayUniverse(p.astype(np.float32), box(dims), charges=q, masses=masses, resids=resids)
        d = DipoleMoment(u.atoms, neutralize=neutralize, verbose=False)
        return d.run().results.dipoles, d._effective_charges()

    here, eff = run(pos, True)
    there, _ = run(moved, True)
    # each run is within its summation bound of its exact sum; the exact sums differ by sum_mol t_mol * (the net
    # effective charge of the molecule, a few roundings of q - Q m / M), all in exact terms below
    _, tol_here = sums_ref(terms_ref(pos, eff), [3 * n_mol])
    _, tol_there = sums_ref(terms_ref(moved, eff), [3 * n_mol])
    residual = np.array([abs(math.fsum(eff[3 * k:3 * k + 3])) for k in range(n_mol)])
    assert residual.max() < 1e-15
    leak = (np.abs(shift[::3]) * residual[:, None]).sum(axis=0)
    bound = tol_here[0] + tol_there[0] + leak[None, :]
    assert np.all(np.abs(there[:, 0] - here[:, 0]) <= bound)
    plain_here, plain_q = run(pos, False)
    plain_there, _ = run(moved, False)
    np.testing.assert_array_equal(plain_q, q)
    assert np.all(np.abs(plain_there - plain_here)[:, 0].max(axis=0) > 1e6 * bound.max())


def test_class_unwrap_makes_the_molecules_of_the_first_frame_whole():
    n_mol, F = 50, 12
    L = np.array([16.0, 20.0, 24.0])
    rng = np.random.default_rng(41)
    _, resids, bonds = _molecules(40, n_mol)
    first = rng.integers(0, (L * GRID).astype(int), (n_mol, 1, 3)) / GRID            # first atoms inside the box
    arms = rng.integers(-1024, 1024, (n_mol, 3, 3)) / GRID                            # bonds under 1 Å per component
    arms[:, 0] = 0
    whole = first + arms
    whole[0] = [[0.25, 10.0, 23.75], [1.0, 9.5, 24.5], [-0.5, 10.5, 23.0]]            # one that straddles two faces
    # every molecule moves as a body, under L / 2 per frame and component, and drifts along x and against z
    steps = (rng.integers(-3 * 1024, 3 * 1024, (F, n_mol, 1, 3)) + np.array([4096, 0, -4096])) / GRID
    steps[0] = 0
    assert np.abs(steps).max() < L.min() / 2
    true = (whole[None] + np.cumsum(steps, axis=0)).reshape(F, 3 * n_mol, 3)
    cell = np.floor(true / L)
    wrapped = true - cell * L
    for a in (true, wrapped):
        np.testing.assert_array_equal(a.astype(np.float32).astype(np.float64), a)
    per_mol = cell[0].reshape(n_mol, 3, 3)
    assert np.any(per_mol.max(axis=1) != per_mol.min(axis=1))                         # split across a face in frame 0
    assert np.abs(cell[0]).max() == 1 and np.abs(cell).max() >= 2
    q = np.tile([-0.8, 0.4, 0.4], n_mol) * np.repeat(rng.uniform(0.5, 2.0, n_mol), 3)
    stored_whole = mdhelper_amd.ArrayUniverse(true.astype(np.float32), box(L), charges=q, resids=resids, bonds=bonds)
    stored_wrapped = mdhelper_amd.ArrayUniverse(wrapped.astype(np.float32), box(L), charges=q, resids=resids,
                                                bonds=bonds)
    want = DipoleMoment(stored_whole.atoms, verbose=False).run().results.dipoles
    got = DipoleMoment(stored_wrapped.atoms, unwrap=True, verbose=False).run().results.dipoles
    # x + image * L is exact on the grid, so the terms are the same numbers in the same order
    np.testing.assert_array_equal(got, want)
    ref, tol = sums_ref(terms_ref(true, q), [3 * n_mol])
    assert_within(got.transpose(1, 0, 2), ref, tol)
    split = DipoleMoment(stored_wrapped.atoms, verbose=False).run().results.dipoles
    assert np.abs(split - want).max() > 1.0                # without unwrap: another answer
    later = DipoleMoment(stored_wrapped.atoms, unwrap=True, verbose=False).run(start=3).results.dipoles
    np.testing.assert_allclose(later, want[3:], atol=1e-9)  # made whole in frame 3, possibly in another image


def test_class_relative_permittivity_of_a_neutral_system():
    pos, resids, _ = _molecules(50, 40, 6)
    rng = np.random.default_rng(51)
    pos = (pos + rng.normal(0.0, 0.3, pos.shape)).astype(np.float32)
    q = np.tile([-0.8, 0.4, 0.4], 40)
    u = mdhelper_amd.ArrayUniverse(pos, box([16.0, 16.0, 16.0]), charges=q, resids=resids)
    oxygens, hydrogens = u.select(np.arange(0, 120, 3)), u.select(np.setdiff1d(np.arange(120), np.arange(0, 120, 3)))
    d = DipoleMoment([oxygens, hydrogens], verbose=False).run()
    d.calculate_relative_permittivity(300.0)
    assert isinstance(d.results.dielectric, float) and d.results.dielectric > 1.0
    assert d.results.dielectric == calculate_relative_permittivity(d.results.dipoles.sum(axis=1), 300.0,
                                                                   d.results.volumes)
    r = DipoleMoment([oxygens, hydrogens], reduced=True, verbose=False).run()
    r.calculate_relative_permittivity(1.2)
    assert r.results.dielectric == calculate_relative_permittivity(r.results.dipoles.sum(axis=1), 1.2,
                                                                   r.results.volumes, reduced=True)
    with pytest.raises(RuntimeError, match="not all"):
        DipoleMoment(oxygens, charges=[0.0], verbose=False).run().calculate_relative_permittivity(300.0)
