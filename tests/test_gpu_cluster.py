"""
Clusters / ClusterEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_cluster_device.hpp): per frame and pair of rows i != j with species a, b,

    d = x_j - x_i;  s = d * (1.0 / L);  w = d - L * rint(s) (+0.0 for a dropped component);
    r2 = (wx*wx + wy*wy) + wz*wz;  bonded = r2 <= cutoff[a][b] * cutoff[a][b], never where cutoff[a][b] == 0

and the connected components of the bonds from ``scipy.sparse.csgraph.connected_components``, relabelled to the
smallest row of each component.

No tolerance anywhere: the results are integers, the restatement does one float64 operation at a time, as the device
does (the unit is built with contraction off; rint rounds ties to even on both sides), so every comparison is
``assert_array_equal``.
"""
import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import Clusters

pytestmark = pytest.mark.gpu

T = _core.ClusterEngine.TILE
J = _core.ClusterEngine.JCHUNK
BOX = np.array([31.0, 44.5, 57.25])
ARRAYS = ("size_counts", "species_counts", "bonds", "n_clusters", "largest", "sum_squares", "labels")
SCALARS = ("evaluations", "frames", "max_row")


# ---------------------------------------------------------------- restatement

def bond_matrix(x, species, table, dims, zero_dims=0):
    """bool [n, n]: the contract's bonds among the rows x float64[n, 3]."""
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    d = x[None, :, :] - x[:, None, :]
    s = d * inv
    w = d - dims * np.rint(s)
    for c in range(3):
        if zero_dims >> c & 1:
            w[..., c] = 0.0
    r2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    rc = np.asarray(table, dtype=np.float64)[species][:, species]
    rc2 = np.where(rc > 0.0, rc * rc, -1.0)
    return (r2 <= rc2) & ~np.eye(len(x), dtype=bool)


def min_labels(h):
    """int32 [n]: the smallest row of the connected component of every row of the bond matrix h."""
    n = len(h)
    count, comp = connected_components(csr_matrix(h), directed=False)
    first = np.full(count, n, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32)


def restate(pos, species, cutoff, dims, zero_dims=0):
    """Every result array, evaluations, frames and max_row for float32 pos[F, n, 3]."""
    x = np.asarray(pos).astype(np.float64)
    F, n = x.shape[:2]
    species = np.asarray(species)
    G = int(species.max()) + 1 if np.ndim(cutoff) == 0 else len(cutoff)
    table = np.full((G, G), float(cutoff)) if np.ndim(cutoff) == 0 else np.asarray(cutoff, dtype=np.float64)
    out = {"size_counts": np.zeros(n + 1, dtype=np.int64), "species_counts": np.zeros((G, n + 1), dtype=np.int64),
           "labels": np.zeros((F, n), dtype=np.int32)}
    for key in ("bonds", "n_clusters", "largest", "sum_squares"):
        out[key] = np.zeros(F, dtype=np.int64)
    max_row = 0
    for f in range(F):
        h = bond_matrix(x[f], species, table, dims, zero_dims)
        assert np.array_equal(h, h.T)
        out["bonds"][f] = h.sum() // 2
        max_row = max(max_row, int(h.sum(axis=1).max()))
        lab = min_labels(h)
        out["labels"][f] = lab
        size_of_root = np.bincount(lab, minlength=n)            # rows per root, 0 for a row that is no root
        sizes = size_of_root[size_of_root > 0]
        out["size_counts"] += np.bincount(sizes, minlength=n + 1)
        for g in range(G):
            out["species_counts"][g] += np.bincount(size_of_root[lab[species == g]], minlength=n + 1)
        out["n_clusters"][f] = len(sizes)
        out["largest"][f] = sizes.max()
        out["sum_squares"][f] = (sizes.astype(np.int64) ** 2).sum()
    out.update(evaluations=F * (n * (n - 1) // 2), frames=F, max_row=max_row)
    return out


def collect(eng):
    got = eng.result()
    got.update(eng.frames())
    got["labels"] = eng.labels()
    stats = eng.stats()
    got.update(evaluations=stats["evaluations"], frames=stats["frames"], max_row=stats["max_row"],
               sweeps=stats["sweeps"])
    return got


def engine_run(pos, species, cutoff, dims, *, splits=None, setup=None, **kwargs):
    """One pass over the frames, host route: what ``restate`` returns (and the sweeps)."""
    eng = _core.ClusterEngine(species, cutoff, dims, keep_labels=True, **kwargs)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def assert_same(got, want):
    for key in ARRAYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert got[key].dtype == (np.int32 if key == "labels" else np.int64), key
    for key in SCALARS:
        assert got[key] == want[key], key
    # what follows from the definitions, whatever the input
    n = got["labels"].shape[1]
    s = np.arange(n + 1)
    np.testing.assert_array_equal(got["species_counts"].sum(axis=0), s * got["size_counts"])
    assert got["size_counts"][0] == 0 and not got["species_counts"][:, 0].any()
    assert got["size_counts"].sum() == got["n_clusters"].sum()
    assert (s * got["size_counts"]).sum() == got["frames"] * n
    assert (s * s * got["size_counts"]).sum() == got["sum_squares"].sum()


def walk(seed, F, n, dims=BOX, step=0.7):
    """Uniform in the box, then a random walk wrapped into the box: float32[F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 4 * T + 5])
def test_one_species_sizes(n):
    """From all singletons over broad distributions to one percolating cluster: the figures asserted of the
    restatement are those of walk(300 + n, 3, n, step=0.25), so that a change of the inputs cannot hollow the test
    out."""
    pos = walk(300 + n, 3, n, step=0.25)
    species = np.zeros(n, dtype=np.int32)
    for cutoff in (4.5, 6.0):
        want = restate(pos, species, cutoff, BOX)
        got = engine_run(pos, species, cutoff, BOX)
        assert_same(got, want)
        assert want["evaluations"] == 3 * (n * (n - 1) // 2)
        assert want["max_row"] <= 26                                # inside the default cap of 32
        assert 1 <= got["sweeps"] <= n + 1                          # the three frames are one slab
        if n <= 2:
            assert (want["n_clusters"] == n).all() and not want["bonds"].any()      # all singletons
        if T - 1 <= n <= T + 1:
            seen = np.flatnonzero(want["size_counts"])
            if cutoff == 4.5:
                assert seen[0] == 1 and 9 <= seen[-1] <= 15 and len(seen) >= 9       # a broad distribution
            else:
                assert 71 <= want["largest"].min() and want["largest"].max() <= 210
        if n == 4 * T + 5 and cutoff == 6.0:
            np.testing.assert_array_equal(want["n_clusters"], [1, 1, 1])            # one percolating cluster
            np.testing.assert_array_equal(want["largest"], [n, n, n])
            assert want["size_counts"][n] == 3


@pytest.mark.parametrize("n", [J - 1, J, J + 1])
def test_partners_around_one_chunk(n):
    """JCHUNK - 1, JCHUNK and JCHUNK + 1 rows: the last is a second chunk of one partner that appends to the same
    rows, and that partner is the own row of the one live lane of the last tile.  One species (the bound is a kernel
    argument), then two whose border lies inside a stage (the bound of that stage is looked up pair by pair)."""
    pos = walk(500 + n, 2, n, step=0.25)
    for species, cutoff in ((np.zeros(n, dtype=np.int32), 4.5),
                            ((np.arange(n) >= 3 * T + 7).astype(np.int32), [[4.5, 5.0], [5.0, 0.0]])):
        want = restate(pos, species, cutoff, BOX)
        assert 1 <= want["max_row"] <= 32 and want["bonds"].all()
        assert_same(engine_run(pos, species, cutoff, BOX), want)


@pytest.fixture(scope="module")
def two_species():
    """Frames of 130 + 191 rows and their species, shared and left unchanged."""
    n, n0 = 321, 130
    pos = walk(421, 3, n, step=0.25)
    species = (np.arange(n) >= n0).astype(np.int32)
    pos.setflags(write=False)
    species.setflags(write=False)
    return pos, species


def test_two_species_unlike_only(two_species):
    pos, species = two_species
    table = [[0.0, 6.0], [6.0, 0.0]]
    want = restate(pos, species, table, BOX)
    assert 79 <= want["n_clusters"].min() and want["n_clusters"].max() <= 88
    assert 81 <= want["largest"].min() and want["largest"].max() <= 88
    assert want["max_row"] == 7
    assert want["species_counts"][0].sum() == 3 * 130 and want["species_counts"][1].sum() == 3 * 191
    assert_same(engine_run(pos, species, table, BOX), want)
    # like rows never bond: no bond inside a species, so every bond joins species 0 and species 1
    h = bond_matrix(pos[0].astype(np.float64), species, np.array(table), BOX)
    assert not h[:130, :130].any() and not h[130:, 130:].any() and h[:130, 130:].any()


def test_two_species_wider_unlike_cutoff(two_species):
    pos, species = two_species
    table = [[0.0, 7.5], [7.5, 0.0]]
    want = restate(pos, species, table, BOX)
    assert 305 <= want["largest"].min() and want["largest"].max() <= 309
    assert want["max_row"] <= 32
    assert_same(engine_run(pos, species, table, BOX), want)


def test_two_species_full_table(two_species):
    pos, species = two_species
    table = [[3.0, 6.0], [6.0, 4.0]]
    want = restate(pos, species, table, BOX)
    unlike = restate(pos, species, [[0.0, 6.0], [6.0, 0.0]], BOX)
    assert want["max_row"] <= 32 and (want["bonds"] > unlike["bonds"]).all()           # like pairs bond as well
    assert_same(engine_run(pos, species, table, BOX), want)
    # the same atoms with a uniform table are the one-species problem, up to the rows of species_counts summing
    uniform = engine_run(pos, species, [[6.0, 6.0], [6.0, 6.0]], BOX)
    one = restate(pos, np.zeros(len(species), dtype=np.int32), 6.0, BOX)
    assert_same(uniform, restate(pos, species, 6.0, BOX))
    np.testing.assert_array_equal(uniform["species_counts"].sum(axis=0), one["species_counts"][0])
    for key in ("size_counts", "bonds", "n_clusters", "largest", "sum_squares", "labels"):
        np.testing.assert_array_equal(uniform[key], one[key])


def test_a_zero_entry_never_bonds_not_even_at_distance_zero():
    """One hand-made frame: rows 0 and 1 (species 0) at one place, row 2 (species 1) at the same place, row 3
    (species 1) on top of row 4 (species 1) far away, row 5 (species 0) within the unlike cutoff of rows 3 and 4."""
    dims = np.array([40.0, 40.0, 40.0])
    pos = np.array([[[5.0, 5.0, 5.0], [5.0, 5.0, 5.0], [5.0, 5.0, 5.0],
                     [25.0, 25.0, 25.0], [25.0, 25.0, 25.0], [25.0, 26.0, 25.0]]], dtype=np.float32)
    species = np.array([0, 0, 1, 1, 1, 0], dtype=np.int32)
    got = engine_run(pos, species, [[0.0, 2.0], [2.0, 0.0]], dims)
    assert_same(got, restate(pos, species, [[0.0, 2.0], [2.0, 0.0]], dims))
    np.testing.assert_array_equal(got["labels"], [[0, 0, 0, 3, 3, 3]])          # 0-2, 1-2 and 3-5, 4-5: four bonds
    np.testing.assert_array_equal(got["bonds"], [4])
    # ... and with no bond between the species at all the like pairs at distance 0 stay apart
    got = engine_run(pos, species, [[0.0, 0.0], [0.0, 2.0]], dims)
    np.testing.assert_array_equal(got["labels"], [[0, 1, 2, 3, 3, 5]])          # only 3-4, both of species 1
    np.testing.assert_array_equal(got["bonds"], [1])
    np.testing.assert_array_equal(got["species_counts"][:, :3], [[0, 3, 0], [0, 1, 2]])
    got = engine_run(pos, species, [[2.0, 0.0], [0.0, 0.0]], dims)
    np.testing.assert_array_equal(got["labels"], [[0, 0, 2, 3, 4, 5]])          # only 0-1
    np.testing.assert_array_equal(got["n_clusters"], [5])


def test_exact_arithmetic_on_the_cutoff():
    """float32 coordinates on a grid of 0.25, box (16, 16, 32), cutoff 5: every r2 below is exact.  Two points per
    frame, so bonds[f] is the table written out by hand and n_clusters[f] is 2 minus it."""
    dims = np.array([16.0, 16.0, 32.0])
    moves = np.array([[3.0, -4.0, 0.0],        # r2 = 25 == rc2: a bond
                      [3.0, -4.0, 0.25],       # one grid step outside: r2 = 25.0625
                      [5.25, 0.0, 0.0],        # one grid step outside along x
                      [8.0, 0.0, 0.0],         # s = +0.5 -> rint 0 (ties to even): w = 8, r2 = 64
                      [-8.0, 0.0, 0.0],        # s = -0.5 -> rint -0: w = -8
                      [13.0, 4.0, 0.0],        # s = 0.8125 -> w = -3 in x: folded onto the cutoff, r2 = 25
                      [0.0, 0.0, -27.0],       # s = -0.84375 -> w = 5 in z: folded onto the cutoff
                      [0.0, 0.0, 26.75],       # w = -5.25 in z: one grid step outside after the fold
                      [0.0, 24.0, 0.25],       # s = 1.5 -> rint 2: w = -8 in y
                      [0.0, 0.0, 0.0],         # a distinct pair at one place: r2 = 0
                      [-4.0, 0.0, 3.0]])       # r2 = 25
    table = np.array([1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1], dtype=np.int64)
    table8 = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=np.int64)      # (0, -8, 0.25): r2 = 64.0625
    origin = np.array([3.25, 9.5, 20.75])
    x1 = np.tile(origin, (len(moves), 1, 1)).astype(np.float32)
    x2 = (origin + moves)[:, None, :].astype(np.float32)
    np.testing.assert_array_equal(x2.astype(np.float64)[:, 0], origin + moves)
    species = np.zeros(2, dtype=np.int32)
    for a, b in ((x1, x2), (x2, x1)):          # the other way round every d changes sign: the same table
        pos = np.concatenate((a, b), axis=1)
        for cutoff, expect in ((5.0, table), (8.0, table8)):        # 8: half the box, the pairs at +-8 lie on it
            got = engine_run(pos, species, cutoff, dims)
            assert_same(got, restate(pos, species, cutoff, dims))
            np.testing.assert_array_equal(got["bonds"], expect)
            np.testing.assert_array_equal(got["n_clusters"], 2 - expect)
            np.testing.assert_array_equal(got["labels"][:, 1], 1 - expect)
            # ... and the same through the table lookup
            two = engine_run(pos, np.array([0, 1], dtype=np.int32), [[1.0, cutoff], [cutoff, 1.0]], dims)
            np.testing.assert_array_equal(two["bonds"], expect)


@pytest.mark.parametrize("case", ["ring", "path", "two"])
def test_long_paths_the_worst_case_of_the_labelling(case):
    """Points at x = 0.5 k on a line in a box of 512: every bond has r2 == rc2 == 0.25 exactly, and the rows are in
    a seeded random order, so that labels travel along a path as long as the graph allows."""
    dims = np.array([512.0, 16.0, 16.0])
    k = {"ring": np.arange(1024),                                   # closed through the periodic face
         "path": np.arange(700),
         "two": np.setdiff1d(np.arange(1024), [300, 800])}[case]
    rng = np.random.default_rng(1024)
    k = rng.permutation(k)
    n = len(k)
    pos = np.empty((1, n, 3), dtype=np.float32)
    pos[0, :, 0] = 0.5 * k
    pos[0, :, 1:] = 8.0
    species = np.zeros(n, dtype=np.int32)
    want = restate(pos, species, 0.5, dims)
    got = engine_run(pos, species, 0.5, dims)
    assert_same(got, want)
    assert want["max_row"] == 2
    if case == "ring":
        assert got["bonds"][0] == 1024 and got["largest"][0] == 1024 and got["n_clusters"][0] == 1
        assert not got["labels"].any()
    elif case == "path":
        assert got["bonds"][0] == 699 and got["largest"][0] == 700 and got["n_clusters"][0] == 1
    else:
        assert got["n_clusters"][0] == 2 and got["bonds"][0] == 1020
        assert sorted(np.flatnonzero(got["size_counts"])) == [499, 523]
    assert 1 <= got["sweeps"] <= n + 1


@pytest.fixture(scope="module")
def system():
    """Twelve frames of two species and their restatements, shared and left unchanged."""
    n0, n1, F = 65, T + 1, 12
    pos = walk(11, F, n0 + n1, step=0.25)
    species = (np.arange(n0 + n1) >= n0).astype(np.int32)
    table = np.array([[3.0, 6.0], [6.0, 4.0]])
    want = restate(pos, species, table, BOX)
    assert want["max_row"] <= 32 and want["largest"].max() > 32
    pos.setflags(write=False)
    for key in ARRAYS:
        want[key].setflags(write=False)
    return {"pos": pos, "species": species, "table": table, "want": want}


def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, species, table, want = system["pos"], system["species"], system["table"], system["want"]
    F, n = pos.shape[:2]

    def check(eng):
        assert_same(collect(eng), want)

    run = lambda **kw: engine_run(pos, species, table, BOX, **kw)       # noqa: E731
    assert_same(run(), want)
    assert_same(run(splits=[0, 1, 5, 12]), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want)
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want)
    assert_same(run(max_neighbors=64), want)                        # another stride of the lists

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
    eng = _core.ClusterEngine(species, table, BOX, keep_labels=True)
    try:
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        stats = eng.stats()
        assert stats["frames"] == 0 and stats["evaluations"] == 0 and stats["max_row"] == 0 and stats["sweeps"] == 0
        assert not any(v.any() for v in eng.result().values()) and len(eng.frames()["bonds"]) == 0
        assert eng.labels().shape == (0, n)
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
        eng.accumulate(pos)
        check(eng)
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()
    # without keep_labels the labels are refused, the rest is the same
    eng = _core.ClusterEngine(species, table, BOX)
    try:
        eng.accumulate(pos)
        np.testing.assert_array_equal(eng.result()["size_counts"], want["size_counts"])
        with pytest.raises(ValueError, match="keep_labels"):
            eng.labels()
    finally:
        eng.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_dims_drops_one_component(system, axis):
    pos, species = system["pos"], system["species"]
    # with a component dropped the cutoffs of the fixture would fill rows beyond 32: shorter ones keep the default cap
    table = [[1.5, 3.0], [3.0, 2.0]]
    want = restate(pos, species, table, BOX, zero_dims=1 << axis)
    assert want["max_row"] <= 32 and (want["bonds"] > restate(pos, species, table, BOX)["bonds"]).all()
    got = engine_run(pos, species, table, BOX, zero_dims=1 << axis)
    assert_same(got, want)
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    again = engine_run(flat, species, table, BOX)
    for key in ARRAYS:
        np.testing.assert_array_equal(again[key], got[key])


def test_a_row_beyond_max_neighbors_is_an_error_never_a_truncation():
    """Frame 0 of walk(12, 12, 322, step=0.25), one species, cutoff 15: the largest row holds 79 bonds, more than any
    max_neighbors allows, so the passes that must succeed use the cutoff lowered to 14, where the largest row of the
    restatement holds 63."""
    pos = walk(12, 12, 322, step=0.25)[:1]
    species = np.zeros(322, dtype=np.int32)
    want = restate(pos, species, 15.0, BOX)
    assert want["max_row"] == 79
    lower = restate(pos, species, 14.0, BOX)
    assert lower["max_row"] == 63
    # sparse input for the same engine: twelve tight blobs of 26 or 27 rows, more than the cutoff apart
    rng = np.random.default_rng(5)
    site = np.arange(322) % 12
    sparse = np.stack((site % 2 * 15.5, site // 2 % 2 * 22.25, site // 4 * 19.0), axis=1) + 1.0
    sparse = (sparse + rng.uniform(-0.1, 0.1, (2, 322, 3))).astype(np.float32)
    sparse_want = restate(sparse, species, 15.0, BOX)
    assert sparse_want["max_row"] == 26
    np.testing.assert_array_equal(sparse_want["n_clusters"], [12, 12])
    eng = _core.ClusterEngine(species, 15.0, BOX, max_neighbors=32, keep_labels=True)
    try:
        eng.accumulate(pos)
        for call in (eng.result, eng.result, eng.synchronize, eng.frames, eng.labels):    # ... and again on the next
            with pytest.raises(ValueError, match="max_neighbors") as err:
                call()
            assert str(want["max_row"]) in str(err.value) and "32" in str(err.value)
        assert eng.stats()["max_row"] == want["max_row"]            # the kernel kept counting
        eng.reset()
        eng.accumulate(sparse)
        assert_same(collect(eng), sparse_want)                      # works again after reset
    finally:
        eng.close()
    assert_same(engine_run(pos, species, 14.0, BOX, max_neighbors=64), lower)
    assert_same(engine_run(pos, species, 14.0, BOX, max_neighbors=63), lower)       # exactly full is no error
    with pytest.raises(ValueError, match="max_neighbors"):
        engine_run(pos, species, 14.0, BOX, max_neighbors=62)
    with pytest.raises(ValueError, match="max_neighbors"):          # an overflow in a later call of the pass
        engine_run(np.concatenate((sparse, pos)), species, 15.0, BOX, splits=[0, 2, 3])


# ---------------------------------------------------------------- the class

class _EchoComm:
    """World size 2, this process plays `rank`; allreduce returns its input."""

    def __init__(self, rank):
        self.rank, self.world_size = rank, 2

    def allreduce(self, arr, op="sum"):
        return arr

    def barrier(self):
        pass


def test_class_routes_groups_and_frame_selections(tmp_path):
    from trajfiles import per_frame, write_amber_netcdf
    n_c, extra, n_a, F = 70, 3, T + 5, 12
    n = n_c + extra + n_a
    pos = walk(20, F, n, step=0.25)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    ia, ib = np.arange(n_c), np.arange(n_c + extra, n)
    table = np.array([[4.0, 6.0], [6.0, 3.0]])          # rows: anions (ib) first, then cations (ia)
    index = np.concatenate((ib, ia))
    species = np.repeat([0, 1], [len(ib), len(ia)]).astype(np.int32)
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    INTS = ("size_counts", "species_counts", "bonds", "n_clusters", "largest", "sum_squares")

    def check(v, frames, cutoff=table, sp=species, idx=index, dims=BOX, zero_dims=0, labels=False):
        """v.results against the restatement and the formulas on the selected frames."""
        want = restate(pos[frames][:, idx], sp, cutoff, dims, zero_dims=zero_dims)
        res = v.results
        s_max = int(want["largest"].max())
        np.testing.assert_array_equal(res.sizes, np.arange(s_max + 1))
        np.testing.assert_array_equal(res.size_counts, want["size_counts"][:s_max + 1])
        np.testing.assert_array_equal(res.species_counts, want["species_counts"][:, :s_max + 1])
        assert not want["size_counts"][s_max + 1:].any() and want["size_counts"][s_max] > 0
        for key in INTS:
            assert res[key].dtype == np.int64, key
        for key in INTS[2:]:
            np.testing.assert_array_equal(res[key], want[key], err_msg=key)
        f, m = len(frames), len(idx)
        n_g = np.bincount(sp)
        np.testing.assert_array_equal(res.size_distribution, res.size_counts / res.size_counts.sum())
        np.testing.assert_array_equal(res.weight_distribution, res.sizes * res.size_counts / (f * m))
        np.testing.assert_array_equal(res.species_fractions, res.species_counts / (f * n_g)[:, None])
        np.testing.assert_array_equal(res.mean_size, m / want["n_clusters"])
        np.testing.assert_array_equal(res.weight_mean_size, want["sum_squares"] / m)
        assert res.weight_distribution.sum() == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(res.species_fractions.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        if labels:
            np.testing.assert_array_equal(res.labels, want["labels"])
            assert res.labels.dtype == np.int32
        else:
            assert "labels" not in res

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            # anions first, cations second: not the order of the frame
            def make(u=u, **kw):
                return Clusters([u.select(ib), u.select(ia)], table, verbose=False, **kw)

            full = make(store_labels=True).run()
            check(full, np.arange(F), labels=True)
            check(make().run(start=1, stop=11, step=2), np.arange(1, 11, 2))
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]))
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in INTS + ("labels",):
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        make = lambda **kw: Clusters([u.select(ib), u.select(ia)], table, verbose=False, **kw)   # noqa: E731
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(make(store_labels=True)).run()
        for key in INTS + ("labels",):
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # every particle in order (no index) as one group with one cutoff
        whole = Clusters(u.atoms, 5.0, verbose=False).run()
        check(whole, np.arange(F), cutoff=5.0, sp=np.zeros(n, dtype=np.int32), idx=np.arange(n))
        # a scalar cutoff with a list of groups: the same atoms as one group, up to the rows of species_counts summing
        split = Clusters([u.select(ib), u.select(ia)], 5.0, verbose=False, store_labels=True).run()
        check(split, np.arange(F), cutoff=5.0, labels=True)
        one = Clusters(u.select(index), 5.0, verbose=False, store_labels=True).run()
        for key in ("sizes", "size_counts", "bonds", "n_clusters", "largest", "sum_squares", "labels"):
            np.testing.assert_array_equal(split.results[key], one.results[key])
        np.testing.assert_array_equal(split.results.species_counts.sum(axis=0), one.results.species_counts[0])
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = make(dimensions=wide).run()
        check(other, np.arange(F), dims=wide)
        assert (other.results.bonds != results["host"].bonds).any()
        # a dropped component (more bonds: shorter cutoffs keep the rows inside the cap)
        short = table / 2
        check(Clusters([u.select(ib), u.select(ia)], short, drop_axis="z", verbose=False).run(), np.arange(F),
              cutoff=short, zero_dims=4)
        # two ranks: the integers add up to the single-rank run's, the per-frame arrays are complementary
        parts = [make(store_labels=True, comm=_EchoComm(r)).run().results for r in (0, 1)]
        host = results["host"]
        total = parts[0].size_counts.shape[0], parts[1].size_counts.shape[0]
        s_all = len(host.size_counts)
        assert max(total) == s_all

        def pad(a):
            return np.concatenate((a, np.zeros(a.shape[:-1] + (s_all - a.shape[-1],), dtype=a.dtype)), axis=-1)

        for key in ("size_counts", "species_counts"):
            np.testing.assert_array_equal(pad(parts[0][key]) + pad(parts[1][key]), host[key])
        for key in INTS[2:] + ("labels",):
            np.testing.assert_array_equal(parts[0][key] + parts[1][key], host[key])
            assert not parts[0][key][F // 2:].any() and not parts[1][key][:F // 2].any()
        assert parts[0].n_clusters[:F // 2].all() and parts[1].n_clusters[F // 2:].all()
        # too few slots: the error of the engine reaches the caller of run()
        with pytest.raises(ValueError, match="max_neighbors"):
            make(max_neighbors=1).run()
    finally:
        d.free()
