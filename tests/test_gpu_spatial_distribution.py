"""
SpatialDistributionFunction / SpatialDistributionEngine on the GPU against the float64 NumPy restatement of the device
contract (``spatial_distribution_cases.py``, csrc/mdx_sdf_device.hpp).

No tolerance anywhere: the results are integers, the restatement does one float64 operation at a time, as the device
does, so every comparison is ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import SpatialDistributionFunction
from spatial_distribution_cases import (AXIS, BISECTOR, BOX, F, N_MOL, assert_same, bin_of, collect, cube_edges,
                                        frames_of, local_coordinates, restate, shared_water, water, water_system)

pytestmark = pytest.mark.gpu

T = _core.SpatialDistributionEngine.TILE
J = _core.SpatialDistributionEngine.JCHUNK
CUT = float(np.sqrt(75.0) * (1.0 + 2.0 ** -40))     # the class's default for R = 5
RC2 = CUT * CUT                                     # as the engine forms it
EDGES = cube_edges(5.0, 20)
SPOT = np.array([1.25, -0.75, 2.25])                # a bin centre of EDGES: bin (12, 8, 14)
SPOT_BIN = (12, 8, 14)


def engine_run(pos, tables, mode, cutoff, edges, dims, *, splits=None, setup=None):
    """One pass over the frames, host route: what ``restate`` returns."""
    eng = _core.SpatialDistributionEngine(pos.shape[1], *tables, mode, cutoff, dims)
    try:
        if edges is not None:
            eng.set_bins(*edges)
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def wrap32(x, dims):
    """float64 positions wrapped into [0, L) and narrowed."""
    dims = np.asarray(dims, dtype=np.float64)
    out = (x - np.floor(x / dims) * dims).astype(np.float32)
    out[out >= dims.astype(np.float32)] = 0.0
    return out


@pytest.fixture(scope="module")
def system():
    """257 waters over 12 frames, every O and every H a partner, and the restatement in both modes: shared and left
    unchanged."""
    pos, tables = shared_water(), water_system()
    want = {mode: restate(pos, *tables, mode, RC2, EDGES, BOX) for mode in (AXIS, BISECTOR)}
    for w in want.values():
        # not vacuous: a third of a million pairs, every bin of both groups hit
        assert w["counts"].sum() > 298_000 and (w["counts"] > 0).all() and w["degenerate"] == 0
        for value in w.values():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
    assert (want[AXIS]["counts"] != want[BISECTOR]["counts"]).any()
    return {"pos": pos, "tables": tables, "want": want}


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n_ref", sorted({1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 2}))
def test_sizes_and_frame_counts(system, n_ref):
    """The first n_ref molecules (beyond 257 the waters once more, seen from a hydrogen: three tiles) against all 771
    partners, whose group boundary at 257 sits one past a stage."""
    pos = system["pos"]
    tables = water_system(n_ref)
    for frames in (1, 2, 12):
        for mode in (AXIS, BISECTOR):
            want = restate(pos[:frames], *tables, mode, RC2, EDGES, BOX)
            assert want["evaluations"] == frames * (n_ref * 771 - 3 * min(n_ref, N_MOL))
            assert want["inside"].min() > 50 * n_ref
            assert_same(engine_run(pos[:frames], tables, mode, CUT, EDGES, BOX), want)
    if n_ref == N_MOL:
        np.testing.assert_array_equal(want["counts"], system["want"][BISECTOR]["counts"])


@pytest.mark.parametrize("n_p", [J - 1, J, J + 1])
def test_partners_around_one_chunk(n_p):
    """T + 1 waters against n_p points that belong to no molecule; the last one sits at SPOT in the frame of molecule
    0 in every frame, so that the last entry of a chunk (or the only one of a second chunk) counts.  Slabs of one
    frame."""
    frames, n_mol = 4, T + 1
    w = water(11, frames, n_mol, BOX)
    rng = np.random.default_rng(n_p)
    pts = rng.uniform(0.0, 1.0, (1, n_p, 3)) * BOX + np.cumsum(rng.normal(0.0, 0.1, (frames, n_p, 3)), axis=0)
    mol = 3 * np.arange(n_mol, dtype=np.int32)
    for f in range(frames):
        e1, e2, e3, degenerate = frames_of(w[f], mol[:1], mol[:1] + 1, mol[:1] + 2, AXIS, BOX)
        assert not degenerate.any()
        pts[f, -1] = w[f, 0].astype(np.float64) + SPOT[0] * e1[0] + SPOT[1] * e2[0] + SPOT[2] * e3[0]
    pos = np.concatenate((w, wrap32(pts, BOX)), axis=1)
    p_row = np.arange(3 * n_mol, 3 * n_mol + n_p, dtype=np.int32)
    tables = (mol, mol + 1, mol + 2, [0, n_p], p_row, np.full(n_p, -1))
    for f in range(frames):
        uvt, near = local_coordinates(pos[f], *tables[:3], p_row, tables[5], AXIS, RC2, BOX)
        assert near[0, -1] and tuple(bin_of(uvt[0, -1, c:c + 1], EDGES[c])[0] for c in range(3)) == SPOT_BIN
    want = restate(pos, *tables, AXIS, RC2, EDGES, BOX)
    assert want["evaluations"] == frames * n_mol * n_p and want["inside"].min() > 10_000
    assert want["counts"][0][SPOT_BIN] >= frames
    assert_same(engine_run(pos, tables, AXIS, CUT, EDGES, BOX, setup=lambda e: e.set_slab_frames(1)), want)


@pytest.mark.parametrize("bins, spans", [((1, 1, 1), [(-5.0, 5.0)] * 3),
                                         ((2, 3, 5), [(-5.0, 5.0), (-3.0, 4.0), (-2.5, 1.5)]),
                                         ((7, 20, 33), [(-4.0, 1.0), (0.5, 5.0), (-5.0, 2.25)]),
                                         ((512, 4, 4), [(-5.0, 5.0), (-5.0, 0.0), (0.0, 5.0)])])
def test_bin_shapes_and_ranges(system, bins, spans):
    """Three different bin counts over three different ranges: a transposed stride or a swapped axis shows."""
    pos, tables = system["pos"][:3], system["tables"]
    edges = [np.linspace(lo, hi, n + 1) for (lo, hi), n in zip(spans, bins)]
    for mode in (AXIS, BISECTOR):
        want = restate(pos, *tables, mode, RC2, edges, BOX)
        assert want["counts"].shape == (2, *bins) and want["counts"].sum() > 5_000
        if np.prod(bins) <= 30:
            assert (want["counts"] > 0).all()
        got = engine_run(pos, tables, mode, CUT, edges, BOX)
        assert got["counts"].shape == (2, *bins)
        assert_same(got, want)
    # without set_bins: one bin per axis, the cube around the sphere, which holds every near pair
    alone = engine_run(pos, tables, AXIS, CUT, None, BOX)
    assert_same(alone, restate(pos, *tables, AXIS, RC2, cube_edges(CUT, 1), BOX))


def test_edges_of_unequal_width(system):
    """The kernel guesses a bin as if the edges were evenly spaced and lets the edges decide: widths that grow by a
    factor of 4000 across an axis, random widths, and two bins one of which is 1e-9 wide."""
    pos, tables = system["pos"][:3], system["tables"]
    rng = np.random.default_rng(29)
    grow = np.concatenate(([-5.0], -5.0 + 10.0 * np.geomspace(2.5e-4, 1.0, 40)))
    jumble = np.concatenate(([-4.0], np.sort(rng.uniform(-4.0, 3.0, 62)), [3.0]))
    sliver = np.array([-5.0, 1.0, 1.0 + 1e-9, 5.0])
    assert np.all(np.diff(jumble) > 0) and np.diff(grow).max() / np.diff(grow).min() > 100
    for edges in ([grow, jumble, sliver], [sliver, grow, jumble], [jumble[::3], sliver, grow]):
        for mode in (AXIS, BISECTOR):
            want = restate(pos, *tables, mode, RC2, edges, BOX)
            assert want["counts"].sum() > 20_000
            assert_same(engine_run(pos, tables, mode, CUT, edges, BOX), want)


@pytest.mark.parametrize("start", [[0, 771], [0, 257, 771], [0, 1, 256, 256, 300, 512, 513, 770, 771]])
def test_one_two_and_eight_groups(system, start):
    """Group boundaries on, before and behind the boundary of a stage, an empty group and groups of one."""
    pos, (o, a, b, _, p_row, owner) = system["pos"][:4], system["tables"]
    tables = (o, a, b, start, p_row, owner)
    want = restate(pos, *tables, BISECTOR, RC2, EDGES, BOX)
    got = engine_run(pos, tables, BISECTOR, CUT, EDGES, BOX)
    assert got["counts"].shape == (len(start) - 1, 20, 20, 20)
    assert_same(got, want)
    np.testing.assert_array_equal(got["counts"].sum(axis=0), system_sum(system, pos))
    if len(start) == 9:
        assert not got["counts"][2].any() and all(got["counts"][g].any() for g in (0, 1, 3, 4, 5, 6, 7))


def system_sum(system, pos):
    """The counts of all partners as one group, of the frames ``pos``."""
    o, a, b, _, p_row, owner = system["tables"]
    return restate(pos, o, a, b, [0, 771], p_row, owner, BISECTOR, RC2, EDGES, BOX)["counts"][0]


def test_owner_exclusion(system):
    """Without owners every molecule counts its own three atoms: 12 x 257 x 3 more pairs, the oxygens in the bin of
    the origin."""
    pos, want = system["pos"], system["want"][AXIS]
    got = engine_run(pos, system["tables"], AXIS, CUT, EDGES, BOX)
    assert_same(got, want)
    tables = water_system(owners=False)
    free_want = restate(pos, *tables, AXIS, RC2, EDGES, BOX)
    free = engine_run(pos, tables, AXIS, CUT, EDGES, BOX)
    assert_same(free, free_want)
    assert free["counts"].sum() - got["counts"].sum() == 9_252 == F * N_MOL * 3
    assert free["evaluations"] - got["evaluations"] == 9_252
    assert (free["counts"] - got["counts"])[0, 10, 10, 10] == F * N_MOL
    # an owner that is another molecule excludes that pair instead
    o, a, b, start, p_row, owner = water_system()
    shifted = (o, a, b, start, p_row, np.roll(owner, 1))
    assert_same(engine_run(pos[:2], shifted, AXIS, CUT, EDGES, BOX), restate(pos[:2], *shifted, AXIS, RC2, EDGES, BOX))


def test_exact_arithmetic_on_the_edges_the_cutoff_and_the_faces():
    """Box (16, 16, 32), O = (3.25, 9.5, 20.75), A = O + (0, 2, 0), B = O + (0, 1, 1): e1 = (0, 1, 0), e2 = (0, 0, 1),
    e3 = (1, 0, 0) exactly, so the local coordinates are (w_y, w_z, w_x), and every number below is a float32."""
    dims = np.array([16.0, 16.0, 32.0])
    O1 = np.array([3.25, 9.5, 20.75])
    O2 = np.array([15.5, 15.0, 31.5])                   # A and B of this one lie across the y and z faces
    eps = np.float64(np.nextafter(np.float32(4.25), np.float32(5.0))) - 4.25
    offsets = [(1.0, 0.5, -0.25),                       # every coordinate on an inner edge: bin (10, 7, 12)
               (0.0, 0.0, 2.0),                         # v on the top edge: the last bin, (8, 15, 8)
               (0.0, 0.0, 2.25),                        # one grid step beyond: not counted
               (1.0, 2.0, 2.0),                         # r2 = 9 = rc2 exactly, u and v on the top edge: (15, 15, 12)
               (1.0 + eps, 2.0, 2.0),                   # one float32 step outside rc2: not counted
               (-1.0, -2.0, -2.0),                      # r2 = 9, u and v on the bottom edge: (0, 0, 4)
               (17.0, 0.5, -0.25), (-15.0, 0.5, -0.25),         # (1, 0.5, -0.25) through the x faces
               (1.0, 16.5, -0.25), (1.0, -15.5, -0.25),         # ... the y faces
               (1.0, 0.5, 31.75), (1.0, 0.5, -32.25)]           # ... the z faces
    rows = [O1, O1 + (0, 2, 0), O1 + (0, 1, 1)] + [O1 + np.array(d) for d in offsets]
    n1 = len(rows)
    rows += [O2, O2 + (0, 2, 0), O2 + (0, 1, 1), O2 + (1.0, 0.5, -0.25)]
    raw = np.array(rows)
    raw[n1:] -= np.floor(raw[n1:] / dims) * dims        # the second molecule and its partner are wrapped
    pos = raw.astype(np.float32)[None]
    np.testing.assert_array_equal(pos[0].astype(np.float64), raw)           # nothing was rounded
    np.testing.assert_array_equal(pos[0, n1 + 1:n1 + 4], [[15.5, 1.0, 31.5], [15.5, 0.0, 0.5], [0.5, 15.5, 31.25]])
    o = np.array([0, n1], dtype=np.int32)
    p_row = np.concatenate((np.arange(3, n1), [n1 + 3])).astype(np.int32)
    tables = (o, o + 1, o + 2, [0, len(p_row)], p_row, np.full(len(p_row), -1))
    e1, e2, e3, degenerate = frames_of(pos[0], o, o + 1, o + 2, AXIS, dims)
    np.testing.assert_array_equal(e1, [[0, 1, 0]] * 2)
    np.testing.assert_array_equal(e2, [[0, 0, 1]] * 2)
    np.testing.assert_array_equal(e3, [[1, 0, 0]] * 2)
    edges = [np.linspace(-2.0, 2.0, 17)] * 3
    want = restate(pos, *tables, AXIS, 9.0, edges, dims)
    expect = np.zeros((16, 16, 16), dtype=np.int64)
    expect[10, 7, 12] = 8                               # itself, six images, and the second molecule's
    expect[8, 15, 8] = expect[15, 15, 12] = expect[0, 0, 4] = 1
    np.testing.assert_array_equal(want["counts"][0], expect)
    np.testing.assert_array_equal(want["inside"], [11])
    assert_same(engine_run(pos, tables, AXIS, 3.0, edges, dims), want)

    # the +-L/2 tie: rint rounds +-0.5 to 0 and +-1.5 to +-2, so d = +-8 stays and d = 24 becomes -8, d = -24 becomes
    # +8; with edges that end at 8 all are inside, on the outermost edges, and r2 = 64 = rc2
    ties = [(8.0, 0.0, 0.0), (24.0, 0.0, 0.0), (-8.0, 0.0, 0.0), (0.0, 8.0, 0.0), (0.0, -24.0, 0.0)]
    raw = np.array([O1, O1 + (0, 2, 0), O1 + (0, 1, 1)] + [O1 + np.array(d) for d in ties])
    pos = raw.astype(np.float32)[None]
    o = np.array([0], dtype=np.int32)
    p_row = np.arange(3, 8, dtype=np.int32)
    tables = (o, o + 1, o + 2, [0, 5], p_row, np.full(5, -1))
    edges = [np.linspace(-8.0, 8.0, 17)] * 3
    want = restate(pos, *tables, AXIS, 64.0, edges, dims)
    expect = np.zeros((16, 16, 16), dtype=np.int64)
    expect[8, 8, 15] = 1                                # d_x = +8: t on the top edge, the last bin
    expect[8, 8, 0] = 2                                 # d_x = 24 and d_x = -8: t on the bottom edge
    expect[15, 8, 8] = 2                                # d_y = +8 and d_y = -24: u on the top edge
    np.testing.assert_array_equal(want["counts"][0], expect)
    assert_same(engine_run(pos, tables, AXIS, 8.0, edges, dims), want)


@pytest.mark.parametrize("mode", [AXIS, BISECTOR])
def test_degenerate_molecules_count_once_and_nothing_else(mode):
    """A on O, B on O, and A, O, B collinear, among sound molecules, against partners of three j chunks."""
    dims, frames, n_p = [16.0, 16.0, 16.0], 3, 2 * J + 5
    mols = np.array([[4, 4, 4], [5, 4, 4], [4, 5, 4],           # sound
                     [9, 9, 9], [9, 9, 9], [9, 10, 9],          # A on O
                     [2, 9, 9], [3, 9, 9], [2, 9, 9],           # B on O
                     [9, 2, 2], [10, 2, 2], [7, 2, 2],          # collinear: b = -2 a exactly
                     [12, 12, 4], [12, 13, 4], [12.5, 12, 5]], dtype=np.float64)
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.0, 16.0, (frames, n_p, 3))
    pos = np.concatenate((np.tile(mols, (frames, 1, 1)), pts), axis=1).astype(np.float32)
    o = np.arange(0, 15, 3, dtype=np.int32)
    p_row = np.arange(15, 15 + n_p, dtype=np.int32)
    tables = (o, o + 1, o + 2, [0, n_p], p_row, np.full(n_p, -1))
    edges = cube_edges(4.0, 8)
    want = restate(pos, *tables, mode, 36.0, edges, dims)
    assert want["degenerate"] == 3 * frames and want["inside"].min() > 100
    sound = (o[[0, 4]], o[[0, 4]] + 1, o[[0, 4]] + 2, [0, n_p], p_row, np.full(n_p, -1))
    np.testing.assert_array_equal(want["counts"], restate(pos, *sound, mode, 36.0, edges, dims)["counts"])
    assert_same(engine_run(pos, tables, mode, 6.0, edges, dims), want)
    assert_same(engine_run(pos, tables, mode, 6.0, edges, dims, setup=lambda e: e.set_slab_frames(1)), want)


@pytest.mark.parametrize("mode", [AXIS, BISECTOR])
def test_rigid_molecules_carry_a_tagged_partner_into_one_bin(mode):
    """48 rigid molecules on a lattice of spacing 20, in random orientations in every frame, each with a tagged atom
    at SPOT of its own frame (a group of its own, owned by nobody).  The other tagged atoms are at least 20 - 2 x 2.7
    away, beyond the cutoff: exactly F x n_ref counts, all in one bin."""
    frames, dims = 5, np.array([80.0, 80.0, 60.0])
    rng = np.random.default_rng(17 + mode)
    centre = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    n_ref = len(centre)
    O = centre * 20.0 + rng.uniform(2.0, 6.0, (frames, n_ref, 3))
    q, r = np.linalg.qr(rng.normal(size=(frames, n_ref, 3, 3)))
    q = q * np.sign(np.linalg.det(q))[..., None, None]          # proper rotations: columns x, y, z of the body
    A = O + 1.0 * q[..., 0]
    B = O - 0.3 * q[..., 0] + 0.9 * q[..., 1]
    body = np.stack((O, A, B), axis=2).reshape(frames, 3 * n_ref, 3)
    mol = 3 * np.arange(n_ref, dtype=np.int32)
    tagged = np.empty((frames, n_ref, 3))
    for f in range(frames):
        e1, e2, e3, degenerate = frames_of(body[f], mol, mol + 1, mol + 2, mode, dims)
        assert not degenerate.any()
        tagged[f] = O[f] + SPOT[0] * e1 + SPOT[1] * e2 + SPOT[2] * e3
    n_free = 300
    free = rng.uniform(0.0, 1.0, (frames, n_free, 3)) * dims
    pos = wrap32(np.concatenate((body, free, tagged), axis=1), dims)
    p_row = np.arange(3 * n_ref, 3 * n_ref + n_free + n_ref, dtype=np.int32)
    tables = (mol, mol + 1, mol + 2, [0, n_free, n_free + n_ref], p_row, np.full(len(p_row), -1))
    want = restate(pos, *tables, mode, RC2, EDGES, dims)
    expect = np.zeros((20, 20, 20), dtype=np.int64)
    expect[SPOT_BIN] = frames * n_ref
    np.testing.assert_array_equal(want["counts"][1], expect)
    assert want["counts"][0].sum() > 100
    got = engine_run(pos, tables, mode, CUT, EDGES, dims)
    assert_same(got, want)
    np.testing.assert_array_equal(got["counts"][1], expect)


def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, tables, want = system["pos"], system["tables"], system["want"][BISECTOR]
    n = pos.shape[1]

    def check(eng):
        assert_same(collect(eng), want)

    run = lambda **kw: engine_run(pos, tables, BISECTOR, CUT, EDGES, BOX, **kw)      # noqa: E731
    assert_same(run(), want)
    assert_same(run(splits=[0, 1, 5, 12]), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want)
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want)

    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    rng = np.random.default_rng(13)
    n_total = 2 * n + 5
    index = rng.permutation(n_total)[:n]
    assert np.any(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    big = (rng.uniform(0.0, 1.0, (F, n_total, 3)) * BOX).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.tile(BOX, (F, 1)), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.SpatialDistributionEngine(n, *tables, BISECTOR, CUT, BOX)
    try:
        eng.set_bins(*EDGES)
        assert eng.plan()["ring_frames"] == 0
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_bins(*EDGES)
        eng.reset()
        stats = eng.stats()
        assert stats["frames"] == 0 and stats["evaluations"] == 0 and stats["degenerate"] == 0
        assert not eng.result().any() and len(eng.inside()) == 0
        eng.accumulate_traj(tf, np.arange(F))
        check(eng)                                                  # file, and a second pass after reset
        eng.reset()
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        check(eng)                                                  # HBM through the index
        with pytest.raises(ValueError, match="out of range"):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        check(eng)                                                  # file through the index
        eng.reset()
        eng.set_slab_frames(4)
        eng.accumulate_device(d.rows(0, 2).ptr, n, 2)               # routes mixed within one pass
        eng.accumulate(pos[2:6])
        eng.accumulate_traj(tf, np.arange(6, F))
        check(eng)
        eng.reset()
        eng.set_slab_frames(0)                                      # the default again
        other = [np.linspace(-5.0, 5.0, 34), np.linspace(-3.0, 4.0, 8), np.linspace(-2.5, 1.5, 3)]
        eng.set_bins(*other)                                        # other bins after a reset: the counters resize
        eng.accumulate(pos)
        got = collect(eng)
        assert got["counts"].shape == (2, 33, 7, 2)
        assert_same(got, restate(pos, *tables, BISECTOR, RC2, other, BOX))
        eng.reset()
        eng.set_bins(*EDGES)                                        # ... and back, larger again
        eng.accumulate(pos[:5])
        eng.accumulate_device(d.rows(5, 7).ptr, n, 7)
        check(eng)
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


# ---------------------------------------------------------------- the class

def test_class_routes_groups_and_frame_selections(system, tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    extra = 3
    water_pos = system["pos"]
    rng = np.random.default_rng(3)
    # three atoms that take no part in front of the water: the feed is an index
    pos = np.concatenate(((rng.uniform(0.0, 1.0, (F, extra, 3)) * BOX).astype(np.float32), water_pos), axis=1)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    o_row, a_row, b_row, start, p_row, owner = system["tables"]
    path = tmp_path / "w.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    modes = {"axis": AXIS, "bisector": BISECTOR}

    def check(v, frames, frame="axis", dims=BOX, edges=EDGES, rc2=RC2):
        """v.results against the restatement and the formulas on the selected frames."""
        want = restate(water_pos[frames], *system["tables"], modes[frame], rc2, edges, dims)
        res = v.results
        np.testing.assert_array_equal(res.counts, want["counts"])
        np.testing.assert_array_equal(res.inside, want["inside"])
        assert res.counts.dtype == res.inside.dtype == np.int64 and res.counts.sum() == res.inside.sum() > 0
        assert res.degenerate == 0 and v.n_frames == len(frames)
        np.testing.assert_array_equal(res.coordination, want["inside"] / N_MOL)
        for c in range(3):
            np.testing.assert_array_equal(res.edges[c], edges[c])
            np.testing.assert_array_equal(res.bins[c], (edges[c][:-1] + edges[c][1:]) / 2)
        dx, dy, dz = (np.diff(e) for e in edges)
        volume = dx[:, None, None] * dy[None, :, None] * dz[None, None, :]
        density = want["counts"] / (len(frames) * N_MOL * volume)
        np.testing.assert_array_equal(res.density, density)
        # a molecule sees the other 256 oxygens and the other 512 hydrogens
        rho = (np.array([257, 514]) - np.array([257, 514]) / N_MOL) / np.prod(np.asarray(dims, dtype=float))
        np.testing.assert_array_equal(rho * np.prod(np.asarray(dims, dtype=float)), [256.0, 512.0])
        np.testing.assert_array_equal(res.sdf, density / rho[:, None, None, None])
        assert res.units["results.density"] == "angstrom^-3" and res.units["results.edges"] == "angstrom"

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            def make(u=u, **kw):
                kw = {"range": 5.0, "n_bins": 20, **kw}
                return SpatialDistributionFunction(
                    u.select(o_row + extra), u.select(a_row + extra), u.select(b_row + extra),
                    [u.select(p_row[:257] + extra), u.select(p_row[257:] + extra)], verbose=False, **kw)

            full = make().run()
            assert full._cutoff == CUT
            np.testing.assert_array_equal(full._owner, owner)       # the default: the molecule an atom frames
            check(full, np.arange(F))
            check(make(frame="bisector").run(start=1, stop=11, step=2), np.arange(1, 11, 2), "bisector")
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]))
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in ("counts", "inside", "degenerate"):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        # the molecules by their places: the same tables, the same integers
        mol = SpatialDistributionFunction.from_molecules(u.select(np.arange(extra, extra + 3 * N_MOL)), N_MOL,
                                                         range=5.0, n_bins=20, verbose=False)
        for key, table in (("_o_row", o_row), ("_a_row", a_row), ("_b_row", b_row), ("_p_row", p_row),
                           ("_owner", owner)):
            np.testing.assert_array_equal(getattr(mol, key), table)
        np.testing.assert_array_equal(mol.run().results.counts, results["host"].counts)
        # one group, an AtomGroup by itself
        one = SpatialDistributionFunction(u.select(o_row + extra), u.select(a_row + extra), u.select(b_row + extra),
                                          u.select(p_row + extra), range=5.0, n_bins=20, verbose=False).run()
        np.testing.assert_array_equal(one.results.counts[0], results["host"].counts.sum(axis=0))
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(make()).run()
        for key in ("counts", "inside"):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = make(dimensions=wide).run()
        check(other, np.arange(F), dims=wide)
        assert (other.results.counts != results["host"].counts).any()
        # other ranges, bins and a cutoff of the caller's
        spans = [(-5.0, 5.0), (-3.0, 4.0), (-2.5, 1.5)]
        edges = [np.linspace(lo, hi, n + 1) for (lo, hi), n in zip(spans, (7, 20, 33))]
        odd = make(range=spans, n_bins=(7, 20, 33), cutoff=4.5, frame="bisector").run()
        check(odd, np.arange(F), "bisector", edges=edges, rc2=4.5 * 4.5)
        # owners of the caller's: nobody owns anything
        free = make(owners=np.full(771, -1)).run()
        assert free.results.counts.sum() - results["host"].counts.sum() == 9_252
        # the radial average: shells of bin centres, weighted by the bin volumes
        full.calculate_radial_average(10)
        res = full.results
        assert res.radial_density.shape == (2, 10) and np.isfinite(res.radial_density).all()
        np.testing.assert_array_equal(res.radial_edges, np.linspace(0.0, 5.0, 11))
        cx, cy, cz = res.bins
        r = np.sqrt(cx[:, None, None] ** 2 + cy[None, :, None] ** 2 + cz[None, None, :] ** 2)
        shell = (r >= 2.5) & (r < 3.0)
        np.testing.assert_allclose(res.radial_density[:, 5], res.density[:, shell].mean(axis=1), rtol=1e-12)
        assert (res.radial_density > 0.0).all()
    finally:
        d.free()
