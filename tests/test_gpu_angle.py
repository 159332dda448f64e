"""
AngularDistribution / AngleEngine on the GPU against a float64 NumPy restatement of the device contract
(csrc/mdx_angle_device.hpp): per frame, centre i and ligand j of species g,

    d = x_j - x_i;  s = d * (1.0 / L);  w = d - L * rint(s) (+0.0 for a dropped component);
    r2 = (wx*wx + wy*wy) + wz*wz;  neighbour = r2 <= cutoff[g] * cutoff[g]  (j != i with `same`)

and for every unordered pair {j, k} of neighbours of i

    dot = (w_ijx*w_ikx + w_ijy*w_iky) + w_ijz*w_ikz;  c = dot / sqrt(r2_ij * r2_ik)
    bin = #{m in 1 ... n_bins - 1 : c <= t[m]} = searchsorted(-t[1:-1], -c, side="right");  a NaN c is `degenerate`.

No tolerance anywhere: the results are integers, the restatement does one float64 operation at a time, as the device
does (the unit is built with contraction off; rint rounds ties to even, sqrt and / are correctly rounded on both
sides), so every comparison is ``assert_array_equal``.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import AngularDistribution

pytestmark = pytest.mark.gpu

T = _core.AngleEngine.TILE
STAGE = _core.AngleEngine.STAGE
BOX = np.array([31.0, 44.5, 57.25])
ANGLE180 = np.cos(np.deg2rad(np.linspace(0.0, 180.0, 181)))
COS4 = np.linspace(1.0, -1.0, 5)
ARRAYS = ("counts", "degenerate", "coordination")
SCALARS = ("evaluations", "frames", "triplets", "max_row")


# ---------------------------------------------------------------- restatement

def pair_number(a, b, G):
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * G - lo * (lo - 1) // 2 + (hi - lo)


def restate(pos, n0, sizes, cutoff, thresholds, dims, *, same=False, zero_dims=0, max_neighbors=32):
    """Every result array, evaluations, frames, triplets and max_row for float32 pos[F, rows, 3]: the n0 centres,
    then the ligand groups of `sizes` (with `same` the centres alone).  coordination is [G, max_neighbors + 1] where
    no row goes beyond the cap, which the caller asserts through max_row."""
    x = np.asarray(pos).astype(np.float64)
    F = len(x)
    sizes = np.atleast_1d(sizes)
    G, n_lig = len(sizes), int(np.sum(sizes))
    P = G * (G + 1) // 2
    species = np.repeat(np.arange(G), sizes)
    cut = np.full(G, float(cutoff)) if np.ndim(cutoff) == 0 else np.asarray(cutoff, dtype=np.float64)
    rc2 = (cut * cut)[species]
    t = np.asarray(thresholds, dtype=np.float64)
    n_bins = len(t) - 1
    dims = np.asarray(dims, dtype=np.float64)
    inv = 1.0 / dims
    width = max(max_neighbors, n_lig) + 1
    out = {"counts": np.zeros((P, n_bins), dtype=np.int64), "degenerate": np.zeros(P, dtype=np.int64),
           "coordination": np.zeros((G, width), dtype=np.int64)}
    max_row = 0
    for f in range(F):
        xc = x[f, :n0]
        xl = xc if same else x[f, n0:]
        assert len(xl) == n_lig
        d = xl[None, :, :] - xc[:, None, :]
        s = d * inv
        w = d - dims * np.rint(s)
        for c in range(3):
            if zero_dims >> c & 1:
                w[..., c] = 0.0
        r2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
        near = r2 <= rc2[None, :]
        if same:
            near &= ~np.eye(n0, dtype=bool)
        max_row = max(max_row, int(near.sum(axis=1).max()))
        for g in range(G):
            out["coordination"][g] += np.bincount(near[:, species == g].sum(axis=1), minlength=width)
        for i in np.flatnonzero(near.sum(axis=1) >= 2):
            idx = np.flatnonzero(near[i])
            a, b = np.triu_indices(len(idx), 1)
            wa, wb = w[i, idx[a]], w[i, idx[b]]
            dot = (wa[:, 0] * wb[:, 0] + wa[:, 1] * wb[:, 1]) + wa[:, 2] * wb[:, 2]
            prod = r2[i, idx[a]] * r2[i, idx[b]]
            with np.errstate(invalid="ignore", divide="ignore"):
                cosine = dot / np.sqrt(prod)
            p = pair_number(species[idx[a]], species[idx[b]], G)
            nan = np.isnan(cosine)
            out["degenerate"] += np.bincount(p[nan], minlength=P)
            bins = np.searchsorted(-t[1:-1], -cosine[~nan], side="right")
            np.add.at(out["counts"], (p[~nan], bins), 1)
    if max_row <= max_neighbors:
        assert not out["coordination"][:, max_neighbors + 1:].any()
        out["coordination"] = out["coordination"][:, :max_neighbors + 1].copy()
    out.update(evaluations=F * (n0 * n_lig - (n0 if same else 0)), frames=F, max_row=max_row,
               triplets=int(out["counts"].sum() + out["degenerate"].sum()))
    return out


def collect(eng):
    got = eng.result()
    stats = eng.stats()
    got.update({key: stats[key] for key in SCALARS})
    return got


def engine_run(pos, n0, sizes, cutoff, thresholds, dims, *, splits=None, setup=None, **kwargs):
    """One pass over the frames, host route: what ``restate`` returns."""
    eng = _core.AngleEngine(n0, sizes, cutoff, thresholds, dims, **kwargs)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return collect(eng)
    finally:
        eng.close()


def assert_same(got, want, n0):
    for key in ARRAYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert got[key].dtype == np.int64, key
    for key in SCALARS:
        assert got[key] == want[key], key
    # what follows from the definitions, whatever the input
    assert got["triplets"] == got["counts"].sum() + got["degenerate"].sum()
    np.testing.assert_array_equal(got["coordination"].sum(axis=1), got["frames"] * n0)


def walk(seed, F, n, dims=BOX, step=0.7):
    """Uniform in the box, then a random walk wrapped into the box: float32[F, n, 3] in [0, L)."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.float64)
    true = rng.uniform(0.0, 1.0, (1, n, 3)) * dims + np.cumsum(rng.normal(0.0, step, (F, n, 3)), axis=0)
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


# ---------------------------------------------------------------- engine

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_one_set_sizes(n):
    """The centres as their own ligands.  The figures asserted of the restatement are those of
    walk(300 + n, 3, n, step=0.25), so that a change of the inputs cannot hollow the test out."""
    pos = walk(300 + n, 3, n, step=0.25)
    for cutoff in (4.5, 6.0):
        want = restate(pos, n, [n], cutoff, ANGLE180, BOX, same=True)
        got = engine_run(pos, n, [n], cutoff, ANGLE180, BOX, same=True)
        assert_same(got, want, n)
        assert want["evaluations"] == 3 * n * (n - 1)
        assert want["max_row"] <= 14                                # inside the default cap of 32
        if n <= 2:
            assert want["triplets"] == 0 and not got["counts"].any()               # no triplet at all
        if n == 65 and cutoff == 6.0:
            assert (want["triplets"], want["max_row"]) == (102, 4)
        if n == 2 * T + 3 and cutoff == 6.0:
            assert (want["triplets"], want["max_row"]) == (28417, 14)
            assert want["counts"].all() and not want["degenerate"].any()            # all 180 bins occupied


def test_more_ligands_than_one_chunk():
    """70 centres and 4 * STAGE + 1 ligands: two blocks append to one centre's row.  As one group (every stage of
    one species, one bound), and as two groups of 300 and 725 with two cutoffs: the first stage is of one species,
    the second spans both (the bound is read per partner), the rest are of the other."""
    n0, n_lig = 70, 4 * STAGE + 1
    assert n_lig > _core.AngleEngine.JCHUNK
    pos = walk(71, 3, n0 + n_lig, step=0.25)
    want = restate(pos, n0, [n_lig], 5.0, ANGLE180, BOX)
    assert (want["max_row"], want["triplets"]) == (15, 5275)
    assert_same(engine_run(pos, n0, [n_lig], 5.0, ANGLE180, BOX), want, n0)
    two = restate(pos, n0, [300, 725], [6.0, 4.0], ANGLE180, BOX)
    assert two["max_row"] == 14
    assert two["counts"].sum(axis=1).tolist() == [1394, 2032, 798]
    assert_same(engine_run(pos, n0, [300, 725], [6.0, 4.0], ANGLE180, BOX), two, n0)


@pytest.mark.parametrize("n_lig", [_core.AngleEngine.JCHUNK - 1, _core.AngleEngine.JCHUNK])
def test_ligands_just_inside_one_chunk(n_lig):
    """T + 1 centres (a second tile of one live lane) and JCHUNK - 1 and JCHUNK ligands: the last stage of the one
    chunk is one ligand short, and full.  Two groups with two cutoffs whose border lies inside the second stage."""
    n0 = T + 1
    pos = walk(600 + n_lig, 2, n0 + n_lig, step=0.25)
    sizes = [300, n_lig - 300]
    want = restate(pos, n0, sizes, [6.0, 4.0], ANGLE180, BOX)
    assert 2 <= want["max_row"] <= 32 and want["counts"].any(axis=1).all()
    assert_same(engine_run(pos, n0, sizes, [6.0, 4.0], ANGLE180, BOX), want, n0)


@pytest.fixture(scope="module")
def two_species():
    """Frames of 130 centres + 100 + 91 ligands, shared and left unchanged."""
    pos = walk(421, 3, 321, step=0.25)
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("cutoff, max_row, triplets", [((6.0, 6.0), 7, (263, 417, 201)),
                                                       ((7.5, 5.0), 8, (1131, 459, 55)),
                                                       ((12.0, 12.0), 26, (15614, 29405, 13454))])
def test_two_species(two_species, cutoff, max_row, triplets):
    pos = two_species
    want = restate(pos, 130, [100, 91], cutoff, ANGLE180, BOX)
    assert want["max_row"] == max_row
    assert tuple((want["counts"].sum(axis=1) + want["degenerate"]).tolist()) == triplets
    got = engine_run(pos, 130, [100, 91], cutoff, ANGLE180, BOX)
    assert_same(got, want, 130)
    np.testing.assert_array_equal(got["coordination"].sum(axis=1), [3 * 130, 3 * 130])
    if cutoff[0] == cutoff[1]:
        # the same atoms as one ligand group give the sum over p, and the coordination of the two together
        one = engine_run(pos, 130, [191], cutoff[0], ANGLE180, BOX)
        assert_same(one, restate(pos, 130, [191], cutoff[0], ANGLE180, BOX), 130)
        np.testing.assert_array_equal(one["counts"][0], got["counts"].sum(axis=0))
        assert one["max_row"] == got["max_row"] and one["triplets"] == got["triplets"]
        m = np.arange(got["coordination"].shape[1])
        assert (one["coordination"][0] * m).sum() == (got["coordination"] * m).sum()


@pytest.mark.parametrize("sizes, n_bins", [([191], 513), ([60, 50, 41, 40], 200), ([60, 50, 41, 40], 180),
                                           ([100, 50, 41], 1)])
def test_histograms_in_hbm_and_in_lds(two_species, sizes, n_bins):
    """513 bins of one pair and 10 pairs of 200 bins count in HBM directly (more than 512 bins; more than 1920
    words); 10 pairs of 180 bins still count in LDS; one bin has no inner threshold at all."""
    pos = two_species
    G = len(sizes)
    cutoff = [12.0, 11.0, 10.0, 9.0][:G]
    thresholds = np.linspace(1.0, -1.0, n_bins + 1)
    want = restate(pos, 130, sizes, cutoff, thresholds, BOX)
    assert want["max_row"] <= 32 and (want["counts"].sum(axis=1) > 100).all()
    assert_same(engine_run(pos, 130, sizes, cutoff, thresholds, BOX), want, 130)


def test_exact_arithmetic_on_the_thresholds():
    """float32 coordinates on a grid of 0.25, box (16, 16, 32), cutoff 5, thresholds 1, 1/2, 0, -1/2, -1: every w,
    r2, dot and c below is exact.  One centre and two ligands per frame, the bin written out by hand."""
    dims = np.array([16.0, 16.0, 32.0])
    origin = np.array([3.25, 9.5, 20.75])
    cases = [((1, 0, 0), (0, 1, 0), 2),             # c = 0: 0 <= 1/2, 0 <= 0, not 0 <= -1/2
             ((1, 1, 0), (1, 0, 1), 1),             # dot 1, r2 2 and 2: c = 1/2 exactly, on the threshold
             ((1, 1, 0), (-1, 0, -1), 3),           # c = -1/2: on the threshold, the last bin
             ((1, 0, 0), (2, 0, 0), 0),             # c = 1
             ((1, 0, 0), (-2.5, 0, 0), 3),          # dot -2.5, sqrt(6.25) = 2.5: c = -1, the last bin is closed
             ((13, 4, 0), (0, 0, -27), 2),          # both fold through the faces onto the cutoff: w = (-3, 4, 0), (0, 0, 5)
             ((0, 0, 0), (1, 0, 0), None),          # a ligand on its centre: r2 = 0, c = 0 / 0, no bin
             ((3, -4, 0.25), (1, 0, 0), -1),        # r2 = 25.0625, just outside the cutoff: no triplet
             ((3, -4, 0), (-4, 0, 3), 2)]           # both on the cutoff: dot -12, c = -12 / 25 > -1/2
    eng = _core.AngleEngine(1, [2], 5.0, COS4, dims)
    try:
        for first, second, expect in cases:
            for moves in ((first, second), (second, first)):            # the ligands swapped: the same bin
                frame = np.array([[origin, origin + moves[0], origin + moves[1]]], dtype=np.float32)
                np.testing.assert_array_equal(frame.astype(np.float64)[0, 1:], origin + np.array(moves))
                eng.reset()
                eng.accumulate(frame)
                got = collect(eng)
                assert_same(got, restate(frame, 1, [2], 5.0, COS4, dims), 1)
                counts, degenerate = np.zeros((1, 4), dtype=np.int64), np.zeros(1, dtype=np.int64)
                if expect is None:
                    degenerate[0] = 1
                elif expect >= 0:
                    counts[0, expect] = 1
                np.testing.assert_array_equal(got["counts"], counts)
                np.testing.assert_array_equal(got["degenerate"], degenerate)
                assert got["max_row"] == (1 if expect == -1 else 2)
    finally:
        eng.close()


def _shell(count):
    """One frame: a centre and `count` ligands on grid points within sqrt(12) of it, box (16, 16, 32)."""
    k = np.array([(a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3) if (a, b, c) != (0, 0, 0)],
                 dtype=np.float64)
    assert len(k) == 124 and count <= 124
    origin = np.array([3.25, 9.5, 20.75])
    return np.concatenate(([origin], origin + k[:count]))[None].astype(np.float32)


def test_a_full_row_is_no_error_and_one_more_is_never_a_truncation():
    dims = np.array([16.0, 16.0, 32.0])
    full, over = _shell(64), _shell(65)
    want = restate(full, 1, [64], 5.0, ANGLE180, dims, max_neighbors=64)
    assert (want["max_row"], want["triplets"]) == (64, 2016)      # the pair loop crosses 64-lane rounds
    assert_same(engine_run(full, 1, [64], 5.0, ANGLE180, dims, max_neighbors=64), want, 1)
    # the 65th ligand far away in the first frame, in its place in the second
    away = over.copy()
    away[0, 65] = away[0, 0] + np.array([0.0, 0.0, 12.0], dtype=np.float32)
    want_away = restate(away, 1, [65], 5.0, ANGLE180, dims, max_neighbors=64)
    assert (want_away["max_row"], want_away["triplets"]) == (64, 2016)
    eng = _core.AngleEngine(1, [65], 5.0, ANGLE180, dims, max_neighbors=64)
    try:
        eng.accumulate(over)
        for call in (eng.result, eng.result, eng.synchronize):      # ... and again on the next
            with pytest.raises(ValueError, match="max_neighbors") as err:
                call()
            assert "65" in str(err.value) and "64" in str(err.value)
        assert eng.stats()["max_row"] == 65                         # the kernel kept counting
        eng.reset()
        eng.accumulate(away)
        assert_same(collect(eng), want_away, 1)                     # works again after reset
        eng.accumulate(over)                                        # an overflow in a later call of the pass
        with pytest.raises(ValueError, match="max_neighbors"):
            eng.result()
        assert eng.stats()["max_row"] == 65
    finally:
        eng.close()
    with pytest.raises(ValueError, match="max_neighbors"):
        engine_run(full, 1, [64], 5.0, ANGLE180, dims, max_neighbors=63)


@pytest.fixture(scope="module")
def system():
    """Twelve frames of 65 centres and ligand groups of 100 and 160, and their restatement, shared and left
    unchanged."""
    n0, sizes, F = 65, [100, 160], 12
    pos = walk(11, F, n0 + sum(sizes), step=0.25)
    cutoff = np.array([8.0, 7.0])
    want = restate(pos, n0, sizes, cutoff, ANGLE180, BOX)
    assert (want["max_row"], want["triplets"]) == (12, 10781)
    pos.setflags(write=False)
    for key in ARRAYS:
        want[key].setflags(write=False)
    return {"pos": pos, "n0": n0, "sizes": sizes, "cutoff": cutoff, "want": want}


def test_one_set_of_integers_whatever_the_split_slab_route_or_index(system, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    pos, n0, sizes, cutoff, want = (system[k] for k in ("pos", "n0", "sizes", "cutoff", "want"))
    F, n = pos.shape[:2]

    def check(eng):
        assert_same(collect(eng), want, n0)

    run = lambda **kw: engine_run(pos, n0, sizes, cutoff, ANGLE180, BOX, **kw)       # noqa: E731
    assert_same(run(), want, n0)
    assert_same(run(splits=[0, 1, 5, 12]), want, n0)
    assert_same(run(setup=lambda e: e.set_slab_frames(1)), want, n0)
    assert_same(run(setup=lambda e: e.set_slab_frames(4)), want, n0)
    assert_same(run(splits=[0, 1, 5, 12], setup=lambda e: e.set_slab_frames(4)), want, n0)
    wide = run(max_neighbors=64)                                    # another stride of the lists
    np.testing.assert_array_equal(wide["coordination"][:, :33], want["coordination"])
    assert not wide["coordination"][:, 33:].any()
    np.testing.assert_array_equal(wide["counts"], want["counts"])

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
    eng = _core.AngleEngine(n0, sizes, cutoff, ANGLE180, BOX)
    try:
        eng.accumulate_device(d.ptr, n, F)
        check(eng)                                                  # HBM
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_slab_frames(4)
        eng.reset()
        stats = eng.stats()
        assert all(stats[key] == 0 for key in SCALARS)
        assert not any(v.any() for v in eng.result().values())
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


@pytest.mark.parametrize("axis, max_row", [(0, 8), (1, 8), (2, 10)])
def test_zero_dims_drops_one_component(system, axis, max_row):
    pos, n0, sizes = system["pos"], system["n0"], system["sizes"]
    # with a component dropped the cutoffs of the fixture would fill rows beyond 32: shorter ones keep the default cap
    cutoff = [3.0, 2.5]
    want = restate(pos, n0, sizes, cutoff, ANGLE180, BOX, zero_dims=1 << axis)
    assert want["max_row"] == max_row
    assert want["triplets"] > 20 * restate(pos, n0, sizes, cutoff, ANGLE180, BOX)["triplets"]
    got = engine_run(pos, n0, sizes, cutoff, ANGLE180, BOX, zero_dims=1 << axis)
    assert_same(got, want, n0)
    flat = pos.copy()
    flat[:, :, axis] = 0.0                                          # the same as frames without that component
    again = engine_run(flat, n0, sizes, cutoff, ANGLE180, BOX)
    for key in ARRAYS:
        np.testing.assert_array_equal(again[key], got[key])


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
    n_a, n_c, extra, n_b, F = 90, 70, 3, T + 5, 12
    n = n_a + n_c + extra + n_b
    pos = walk(20, F, n, step=0.25)
    boxes = np.tile(np.array([*BOX, 90.0, 90.0, 90.0], dtype=np.float32), (F, 1))
    ia, ic, ib = np.arange(n_a), np.arange(n_a, n_a + n_c), np.arange(n_a + n_c + extra, n)
    cutoff = np.array([7.0, 8.0])                       # ligands: ib first, then ia; the centres lie between them
    index = np.concatenate((ic, ib, ia))
    sizes = [n_b, n_a]
    path = tmp_path / "m.nc"
    write_amber_netcdf(path, pos, lengths=boxes[:, :3], angles=boxes[:, 3:])
    d = _core.DeviceArray.from_host(pos)
    INTS = ("counts", "degenerate", "coordination_counts")

    def check(v, frames, cut=cutoff, sz=sizes, idx=index, n0=n_c, dims=BOX, zero_dims=0, thresholds=ANGLE180,
              edges=np.linspace(0.0, 180.0, 181), same=False):
        """v.results against the restatement and the formulas on the selected frames."""
        want = restate(pos[frames][:, idx], n0, sz, cut, thresholds, dims, zero_dims=zero_dims, same=same)
        res = v.results
        G = len(sz)
        m_max = int(np.flatnonzero(want["coordination"].any(axis=0))[-1])
        np.testing.assert_array_equal(res.counts, want["counts"])
        np.testing.assert_array_equal(res.degenerate, want["degenerate"])
        np.testing.assert_array_equal(res.coordination_counts, want["coordination"][:, :m_max + 1])
        for key in INTS:
            assert res[key].dtype == np.int64, key
        assert res.pairs == [(a, b) for a in range(G) for b in range(a, G)]
        np.testing.assert_array_equal(res.edges, edges)
        np.testing.assert_array_equal(res.bins, (edges[:-1] + edges[1:]) / 2)
        width = np.abs(np.diff(edges))
        assert (res.counts.sum(axis=1) > 0).all()
        np.testing.assert_array_equal(res.distribution, res.counts / (res.counts.sum(axis=1)[:, None] * width))
        np.testing.assert_allclose((res.distribution * width).sum(axis=1), 1.0, rtol=0, atol=1e-12)
        f = len(frames)
        np.testing.assert_array_equal(res.coordination_distribution, res.coordination_counts / (f * n0))
        np.testing.assert_allclose(res.coordination_distribution.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(res.coordination_number,
                                   (want["coordination"] * np.arange(want["coordination"].shape[1])).sum(axis=1)
                                   / (f * n0), rtol=1e-12, atol=0)
        return want

    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, boxes, dt=0.5)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=0.5))):
            # ligand groups in an order that is not the frame's
            def make(u=u, **kw):
                return AngularDistribution(u.select(ic), [u.select(ib), u.select(ia)], cutoff, verbose=False, **kw)

            full = make().run()
            want = check(full, np.arange(F))
            assert want["max_row"] <= 32 and want["triplets"] > 5000
            check(make().run(start=1, stop=11, step=2), np.arange(1, 11, 2))
            check(make().run(frames=[2, 5, 8, 11]), np.array([2, 5, 8, 11]))
            results[name] = full.results
        for name in ("hbm", "file"):                       # one set of integers whatever the route
            for key in INTS:
                np.testing.assert_array_equal(results[name][key], results["host"][key])
        u = mdhelper_amd.ArrayUniverse(pos, boxes, dt=0.5)
        make = lambda **kw: AngularDistribution(u.select(ic), [u.select(ib), u.select(ia)], cutoff,   # noqa: E731
                                                verbose=False, **kw)
        # a reader without block access goes frame by frame through the batcher
        slow = per_frame(make()).run()
        for key in INTS:
            np.testing.assert_array_equal(slow.results[key], results["host"][key])
        # bins of equal width in the cosine
        cosine = make(bins="cosine", n_bins=50).run()
        check(cosine, np.arange(F), thresholds=np.linspace(1.0, -1.0, 51), edges=np.linspace(1.0, -1.0, 51))
        assert cosine.results.counts.sum() == results["host"].counts.sum()
        assert cosine.results.units["results.bins"] == "dimensionless"
        assert results["host"].units["results.bins"] == "degree"
        # every particle in order (no index) as the centres and their own ligands
        whole = AngularDistribution(u.atoms, u.atoms, 5.0, verbose=False).run()
        check(whole, np.arange(F), cut=5.0, sz=[n], idx=np.arange(n), n0=n, same=True)
        # one ligand group with one cutoff: the sum over the pairs of the two groups with that cutoff
        split = AngularDistribution(u.select(ic), [u.select(ib), u.select(ia)], 7.0, verbose=False).run()
        check(split, np.arange(F), cut=7.0)
        one = AngularDistribution(u.select(ic), u.select(np.concatenate((ib, ia))), 7.0, verbose=False).run()
        np.testing.assert_array_equal(one.results.counts[0], split.results.counts.sum(axis=0))
        # dimensions given: they replace the universe's box
        wide = BOX + 2.0
        other = make(dimensions=wide).run()
        check(other, np.arange(F), dims=wide)
        assert (other.results.counts != results["host"].counts).any()
        # a dropped component (more neighbours: shorter cutoffs keep the rows inside the cap)
        short = cutoff / 3
        check(AngularDistribution(u.select(ic), [u.select(ib), u.select(ia)], short, drop_axis="z",
                                  verbose=False).run(), np.arange(F), cut=short, zero_dims=4)
        # two ranks: the integers add up to the single-rank run's
        parts = [make(comm=_EchoComm(r)).run().results for r in (0, 1)]
        host = results["host"]
        m_all = host.coordination_counts.shape[1]
        assert max(p.coordination_counts.shape[1] for p in parts) == m_all

        def pad(a):
            return np.concatenate((a, np.zeros(a.shape[:-1] + (m_all - a.shape[-1],), dtype=a.dtype)), axis=-1)

        np.testing.assert_array_equal(parts[0].counts + parts[1].counts, host.counts)
        np.testing.assert_array_equal(parts[0].degenerate + parts[1].degenerate, host.degenerate)
        np.testing.assert_array_equal(pad(parts[0].coordination_counts) + pad(parts[1].coordination_counts),
                                      host.coordination_counts)
        assert parts[0].counts.any() and parts[1].counts.any()
        # too few slots: the error of the engine reaches the caller of run()
        with pytest.raises(ValueError, match="max_neighbors"):
            make(max_neighbors=1).run()
    finally:
        d.free()
