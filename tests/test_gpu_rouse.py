"""
RouseModes / ChainProjectionEngine on the GPU against the definition

    X[c][k] = sum_n w[k][n] x_n,        x_n = (double) r_n + image_n * L,

restated as a float64 NumPy loop that adds the products one after the other, n = 0, 1, ..., after the same
``unwrap_ref`` / ``centres_ref`` rules that ``test_gpu_gyradius.py`` states (the reference project has no such
analysis: nothing is compared with it).

Tolerance (derived, not tuned).  Restatement and device both sum N_p products in float64.  Whatever the two orders
are, each side is within (N_p + 2) 2^-53 sum_n |w_n x_n| of the exact sum (N_p - 1 additions and one rounding per
product, first order), so the two differ by at most

    2 (N_p + 2) 2^-53 sum_n |w_n x_n|  <=  2 (N_p + 2) 2^-53 max|x|,       since sum_n |w_n| <= 1

for the weights used here (cos(...) / N_p, or random numbers in [-1, 1] / N_p).  The tests use
atol = 16 (N_p + 8) 2^-53 max|x| and rtol = 0: 8 times the bound.  (The engine happens to add in the order of the
restatement, so the two usually agree to the last bit; the tolerance does not rely on it.)  Outputs that must not
depend on the route or on the split into calls are compared with ``assert_array_equal``.  (The correlation engine
reading the amplitudes in HBM against the same engine fed their host copy is not among them: see that test.)

The class is checked against ``algorithm.correlation.correlation_fft`` of the restated amplitudes with rtol = 1e-9,
atol = 1e-11 on the normalised ACF — the tolerances ``test_end_to_end_vector_acf_on_device`` applies to the same
correlation engine — and rtol = 1e-9 on the mean-square amplitudes.
"""
import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.algorithm import correlation
from mdhelper_amd.analysis import RouseModes

pytestmark = pytest.mark.gpu

STAGE = 1024            # points a workgroup stages at a time (ROUSE_STAGE of csrc/mdx_rouse_device.hpp)


def atol_for(N_p, x):
    return 16 * (N_p + 8) * 2.0 ** -53 * float(np.abs(x).max())


# ---------------------------------------------------------------- restatement

def rouse_weights(N_p, modes):
    return np.stack([np.cos(np.pi * p * (np.arange(N_p) + 0.5) / N_p) / N_p for p in modes])


def amplitudes_ref(points, n_chains, n_monomers, weights):
    """points float64[F, N, 3] in concatenated-group order, weights[g] float64[K, N_p] -> [F, S, 3] with series
    series0[g] + k * M + c; the products are added sequentially over n."""
    points = np.asarray(points, dtype=np.float64)
    out, lo = [], 0
    for M, N_p, w in zip(n_chains, n_monomers, weights):
        x = points[:, lo:lo + M * N_p].reshape(len(points), M, N_p, 3)
        acc = np.zeros((len(points), len(w), M, 3))
        for n in range(N_p):
            acc = acc + w[None, :, n, None, None] * x[:, None, :, n, :]
        out.append(acc.reshape(len(points), -1, 3))
        lo += M * N_p
    return np.concatenate(out, axis=1)


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


def engine_amplitudes(pos, n_chains, n_monomers, weights, *, splits=None, setup=None):
    eng = _core.ChainProjectionEngine(n_chains, n_monomers, weights)
    try:
        if setup is not None:
            setup(eng)
        cuts = splits or [0, len(pos)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate(pos[lo:hi])
        return eng.result(), eng.stats()
    finally:
        eng.close()


def box(dims):
    return [*dims, 90.0, 90.0, 90.0]


# ---------------------------------------------------------------- engine against the restatement

# (N_p, rows, chains): chains that share a workgroup (N_p <= STAGE / 2) with and without a remainder, more
# (chain, row) pairs than the 256 threads of a workgroup (32 x 31 ... 130 x 129), several workgroups per group
# (33 x 40: 31 + 9 chains; N_p = 1000: one chain each), and chains longer than the staged chunk with one row tile
# (1030) and with two (1100 x 300)
SHAPES = [(2, [1], 5), (31, range(1, 6), 7), (32, range(1, 32), 7), (33, range(1, 33), 3), (63, range(1, 8), 7),
          (64, range(1, 64), 4), (65, range(1, 65), 4), (130, range(1, 130), 3),
          (1000, [1, 2, 3, 500, 996, 997, 998, 999], 3),
          (33, range(1, 5), 40), (1030, range(1, 6), 2), (1100, range(1, 301), 2)]


@pytest.mark.parametrize("N_p, rows, M", SHAPES, ids=[f"{n}x{len(r)}x{m}" for n, r, m in SHAPES])
def test_engine_shapes(N_p, rows, M):
    rng = np.random.default_rng(1000 * N_p + M)
    F = 6
    pos = walks(rng, F, M, N_p)
    w = rouse_weights(N_p, rows)
    assert np.abs(w).sum(axis=1).max() <= 1.0
    got, st = engine_amplitudes(pos, [M], [N_p], [w])
    assert got.shape == (F, len(w) * M, 3) and st["frames"] == F
    want = amplitudes_ref(pos, [M], [N_p], [w])
    print(f"N_p={N_p} K={len(w)} M={M}: max|got - want| = {np.abs(got - want).max():.3e}, "
          f"atol = {atol_for(N_p, pos):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=atol_for(N_p, pos))
    assert np.abs(got).max() > 1e-3                          # not a comparison of zeros


def test_engine_two_groups():
    rng = np.random.default_rng(2)
    n_chains, n_monomers, F, K = [5, 3], [2, 130], 6, 3
    pos = np.concatenate([walks(rng, F, M, N) for M, N in zip(n_chains, n_monomers)], axis=1)
    weights = [rng.uniform(-1.0, 1.0, (K, N)) / N for N in n_monomers]      # any weights: sum |w| <= 1
    got, st = engine_amplitudes(pos, n_chains, n_monomers, weights)
    assert got.shape == (F, K * 8, 3) and st["frames"] == F
    want = amplitudes_ref(pos, n_chains, n_monomers, weights)
    # series series0[g] + k * M + c: the short chains first, then the long ones
    np.testing.assert_allclose(got[:, :15], want[:, :15], rtol=0, atol=atol_for(2, pos))
    np.testing.assert_allclose(got[:, 15:], want[:, 15:], rtol=0, atol=atol_for(130, pos))
    x = pos.astype(np.float64)
    np.testing.assert_allclose(got[:, 15 + 1 * 3 + 2], (weights[1][1][:, None] * x[:, 10 + 2 * 130:]).sum(axis=1),
                               rtol=0, atol=atol_for(130, pos))
    with pytest.raises(ValueError):
        engine_amplitudes(pos[:, :50], n_chains, n_monomers, weights)        # wrong number of rows
    eng = _core.RouseEngine(n_chains, n_monomers, weights)                   # the alias; ±1 on the chain ends
    eng.close()
    ends = [np.zeros((1, N)) for N in n_monomers]
    for e in ends:
        e[0, 0], e[0, -1] = -1.0, 1.0
    got, _ = engine_amplitudes(pos, n_chains, n_monomers, ends)
    np.testing.assert_array_equal(got[:, :5], x[:, 1:10:2] - x[:, 0:10:2])   # the end-to-end vectors, exactly
    long = x[:, 10:].reshape(F, 3, 130, 3)
    np.testing.assert_array_equal(got[:, 5:], long[:, :, -1] - long[:, :, 0])


def test_far_from_the_origin():
    """Chains 9 000 A from the origin in float32: the coordinates are widened before any arithmetic."""
    rng = np.random.default_rng(3)
    F, M, N_p = 6, 3, 130
    pos = walks(rng, F, M, N_p, offset=9000.0)
    assert pos.dtype == np.float32 and pos.min() > 8900.0
    w = rouse_weights(N_p, range(1, 11))
    got, _ = engine_amplitudes(pos, [M], [N_p], [w])
    np.testing.assert_allclose(got, amplitudes_ref(pos, [M], [N_p], [w]), rtol=0, atol=atol_for(N_p, pos))
    assert np.abs(got).max() < 50.0                          # the offset projects out of every mode p >= 1


def test_definition_cosine_chains_have_one_mode():
    """r_n = A cos(q pi (n + 1/2) / N_p) e_x + const gives X_p = (A / 2) delta_pq e_x for 1 <= p, q <= N_p - 1
    (orthogonality of the DCT-II rows) — checked without the restatement.  Tolerance: the summation bound of the
    module docstring plus the rounding of the float32 input, 2^-24 max|r| (sum |w_n| <= 1)."""
    N_p, A = 65, 7.0
    qs = [1, 7, 64]
    const = np.array([3.0, -2.0, 5.0])
    n = np.arange(N_p)
    pos = np.tile(const, (len(qs) * N_p, 1))
    for c, q in enumerate(qs):
        pos[c * N_p:(c + 1) * N_p, 0] += A * np.cos(q * np.pi * (n + 0.5) / N_p)
    pos32 = pos.astype(np.float32)[None]
    modes = np.arange(1, N_p)
    got, _ = engine_amplitudes(pos32, [len(qs)], [N_p], [rouse_weights(N_p, modes)])
    got = got[0].reshape(len(modes), len(qs), 3)            # [k, c]
    want = np.zeros_like(got)
    for c, q in enumerate(qs):
        want[q - 1, c, 0] = A / 2
    atol = atol_for(N_p, pos32) + 2.0 ** -24 * float(np.abs(pos32).max())
    print(f"max|X - (A/2) delta| = {np.abs(got - want).max():.3e}, atol = {atol:.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=atol)


# ---------------------------------------------------------------- unwrap and grouping

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
    L, F, M, N_p = 30.0, 12, 6, 65
    dims = np.array([L, L, L])
    pos, cell = _drifting_chains(6, F, M, N_p, L, (4.0, -3.6, 3.9))
    per_chain = cell.reshape(F, M, N_p, 3)
    assert np.all((per_chain[-1] != per_chain[0]).any(axis=(1, 2)))                # every chain crosses a face
    start = pos[0].astype(np.float64) + cell[0] * L                                # frame 0, every chain whole
    margin = []
    whole = unwrap_ref(pos, start, dims, margin)
    assert min(margin) > 1e-3              # no image decision can flip on a float32-versus-float64 last bit
    np.testing.assert_allclose(whole, pos.astype(np.float64) + cell * L, atol=1e-9)     # the rule recovers the chains
    w = rouse_weights(N_p, range(1, 9))
    want = amplitudes_ref(whole, [M], [N_p], [w])
    wrapped = amplitudes_ref(pos, [M], [N_p], [w])
    assert np.abs(wrapped - want).max() > 0.1                                      # without unwrap: another answer
    tol = atol_for(N_p, whole)
    setup = lambda e: e.set_unwrap(dims, start)      # noqa: E731
    got, _ = engine_amplitudes(pos, [M], [N_p], [w], setup=setup)
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)
    two, _ = engine_amplitudes(pos, [M], [N_p], [w], splits=[0, 5, 12], setup=setup)
    np.testing.assert_array_equal(two, got)
    many, _ = engine_amplitudes(pos, [M], [N_p], [w], splits=list(range(F + 1)), setup=setup)
    np.testing.assert_array_equal(many, got)
    eng = _core.ChainProjectionEngine([M], [N_p], [w])
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
        np.testing.assert_allclose(eng.result(), wrapped, rtol=0, atol=atol_for(N_p, pos))
    finally:
        eng.close()
        d.free()


def test_grouping_forms_the_monomer_centres():
    rng = np.random.default_rng(5)
    M, N_p, size, F = 4, 5, 3, 6
    centres = walks(rng, F, M, N_p, bond=4.0).astype(np.float64)
    pos = (centres[:, :, None, :] + rng.uniform(-1, 1, (F, M * N_p, size, 3))).reshape(F, -1, 3).astype(np.float32)
    atom_masses = rng.uniform(1.0, 16.0, M * N_p * size)
    w = rouse_weights(N_p, range(1, N_p))
    want = amplitudes_ref(centres_ref(pos, size, atom_masses), [M], [N_p], [w])
    offsets = size * np.arange(M * N_p + 1)
    setup = lambda e: e.set_grouping(offsets, atom_masses)      # noqa: E731
    got, _ = engine_amplitudes(pos, [M], [N_p], [w], setup=setup)
    np.testing.assert_allclose(got, want, rtol=0, atol=atol_for(N_p, pos))
    split, _ = engine_amplitudes(pos, [M], [N_p], [w], splits=[0, 2, 3, 6], setup=setup)
    np.testing.assert_array_equal(split, got)
    with pytest.raises(ValueError):
        engine_amplitudes(pos, [M], [N_p], [w], setup=lambda e: e.set_grouping(offsets[:-1], atom_masses[:-size]))


# ---------------------------------------------------------------- routes

def test_one_set_of_bits_on_every_route(tmp_path):
    from mdhelper_amd.io import TrajectoryFile
    from trajfiles import write_amber_netcdf
    rng = np.random.default_rng(4)
    n_chains, n_monomers, F = [4, 9], [130, 7], 9
    pos = np.concatenate([walks(rng, F, M, N) for M, N in zip(n_chains, n_monomers)], axis=1)
    n = pos.shape[1]
    weights = [rouse_weights(N, range(1, 7)) for N in n_monomers]
    once, st = engine_amplitudes(pos, n_chains, n_monomers, weights)
    assert st["frames"] == F
    np.testing.assert_allclose(once, amplitudes_ref(pos, n_chains, n_monomers, weights), rtol=0,
                               atol=atol_for(130, pos))
    split, _ = engine_amplitudes(pos, n_chains, n_monomers, weights, splits=[0, 1, 4, 9])      # a one-frame call
    np.testing.assert_array_equal(split, once)
    # the same rows inside larger frames, picked by an index that is neither contiguous nor ascending
    n_total = 2 * n + 5
    index = rng.permutation(n_total)[:n]
    big = rng.uniform(0.0, 40.0, (F, n_total, 3)).astype(np.float32)
    big[:, index] = pos
    path, big_path = tmp_path / "rows.nc", tmp_path / "big.nc"
    lengths, angles = np.full((F, 3), 60.0), np.full((F, 3), 90.0)
    write_amber_netcdf(path, pos, lengths=lengths, angles=angles)
    write_amber_netcdf(big_path, big, lengths=lengths, angles=angles)
    d, d_big = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(big)
    tf, tf_big = TrajectoryFile(path), TrajectoryFile(big_path)
    eng = _core.ChainProjectionEngine(n_chains, n_monomers, weights)
    try:
        eng.reserve(F)
        eng.accumulate_device(d.ptr, n, F)
        np.testing.assert_array_equal(eng.result(), once)                       # HBM
        eng.reset()
        assert eng.stats()["frames"] == 0 and eng.result().shape == (0, once.shape[1], 3)
        eng.accumulate_device(d_big.ptr, n_total, F, index)
        np.testing.assert_array_equal(eng.result(), once)                       # HBM through the index
        with pytest.raises(ValueError):
            eng.accumulate_device(d_big.ptr, n_total, F, np.append(index[:-1], n_total))      # out of range
        eng.reset()
        eng.accumulate_traj(tf, np.arange(F))
        np.testing.assert_array_equal(eng.result(), once)                       # file
        eng.reset()
        eng.accumulate_traj(tf_big, np.arange(F), index)
        np.testing.assert_array_equal(eng.result(), once)                       # file through the index
        eng.reset()
        eng.accumulate_device(d.rows(0, 2).ptr, n, 2)                           # routes mixed within one pass
        eng.accumulate(pos[2:5])
        eng.accumulate_traj(tf, np.arange(5, F))
        np.testing.assert_array_equal(eng.result(), once)
        ptr, frames, series = eng.device_result()
        assert (frames, series) == (F, once.shape[1]) and ptr.value
    finally:
        eng.close()
        tf.close()
        tf_big.close()
        d.free()
        d_big.free()


def test_correlation_engine_reads_the_amplitudes_where_they_lie():
    """``device_result`` + ``MsdEngine.push_device`` + ``result_acf`` against ``MsdEngine.push`` of the host copy of
    the same amplitudes.  The same float64 numbers reach the same pipeline, but not bit for bit the same sums: the
    correlation engine packs two real series into one complex transform and enters a range that starts inside a
    128-byte line a few coordinates early (``head`` in ``msd_push_device``, csrc/mdx_msd.hip), so which series
    share a transform depends on where the range lies in its frame — `first = k M` of S here, 0 of M in the staged
    host copy.  Measured: 64 % of the lags differ, by at most 4.4e-14 relative.  The comparison therefore uses the
    tolerances of this correlation engine's own tests (rtol = 1e-9, atol = 1e-11 on the normalised ACF, rtol = 1e-9
    on its lag-0 value)."""
    rng = np.random.default_rng(6)
    M, N_p, K, B, Tb = 12, 16, 4, 2, 40
    pos = walks(rng, B * Tb, M, N_p)
    eng = _core.ChainProjectionEngine([M], [N_p], [rouse_weights(N_p, range(1, K + 1))])
    dev, host = _core.MsdEngine(Tb, B, K), _core.MsdEngine(Tb, B, K)
    try:
        eng.accumulate(pos)
        ptr, frames, S = eng.device_result()
        assert (frames, S) == (B * Tb, K * M)
        X = eng.result()
        for k in range(K):
            dev.push_device(k, ptr, S, k * M, M)
            host.push(k, X, k * M, M)
        got, want = dev.result_acf(), host.result_acf()
    finally:
        dev.close()
        host.close()
        eng.close()
    assert got.shape == (K, B, Tb) and np.all(got[..., 0] > 0)
    print("largest relative difference between the two pushes:", np.abs(got / want - 1).max())
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got / got[..., :1], want / want[..., :1], rtol=1e-9, atol=1e-11)


# ---------------------------------------------------------------- the class

@pytest.fixture(scope="module")
def melt():
    """12 chains of 16 monomers, 256 frames, in larger frames; the restated amplitudes [T, P, M, 3] of all modes."""
    rng = np.random.default_rng(8)
    T, M, N_p = 256, 12, 16
    conf = np.cumsum(rng.normal(scale=0.55, size=(1, M, N_p, 3)), axis=2)
    wiggle = np.cumsum(rng.normal(scale=0.06, size=(T, M, N_p, 3)), axis=0)
    chains = (rng.uniform(0, 20.0, (1, M, 1, 3)) + conf + wiggle).reshape(T, M * N_p, 3).astype(np.float32)
    extra = 5                                               # particles of no group, in front
    pos = np.concatenate(((rng.random((T, extra, 3)) * 20).astype(np.float32), chains), axis=1)
    modes = np.arange(1, N_p)
    X = amplitudes_ref(chains, [M], [N_p], [rouse_weights(N_p, modes)]).reshape(T, len(modes), M, 3)
    X.setflags(write=False)
    return {"pos": pos, "index": np.arange(extra, extra + M * N_p), "M": M, "N_p": N_p, "X": X}


def _acf_ref(X, modes, n_blocks):
    """(amplitudes [B, P], acf [B, P, T_b]) of restated amplitudes X[T, 15, M, 3] (all modes p = 1 ... 15)."""
    T, _, M, _ = X.shape
    Tb = T // n_blocks
    amp, acf = [], []
    for p in modes:
        raw = correlation.correlation_fft(X[:n_blocks * Tb, p - 1].reshape(n_blocks, Tb, M, 3), axis=1,
                                          average=True, vector=True)
        amp.append(raw[:, 0])
        acf.append(raw / raw[:, :1])
    return np.stack(amp, axis=1), np.stack(acf, axis=1)


@pytest.mark.parametrize("n_blocks, modes", [(1, 15), (2, 15), (2, [7, 1, 15])])
def test_class_against_the_restated_amplitudes(melt, n_blocks, modes):
    u = mdhelper_amd.ArrayUniverse(melt["pos"], box([40.0] * 3), dt=2.0)
    group = u.select(melt["index"])
    kw = {"n_chains": melt["M"], "n_monomers": melt["N_p"], "modes": modes, "n_blocks": n_blocks, "verbose": False}
    r = RouseModes(group, **kw).run()
    listed = np.arange(1, modes + 1) if isinstance(modes, int) else np.asarray(modes)
    P, Tb = len(listed), 256 // n_blocks
    np.testing.assert_array_equal(r.results.modes, listed)
    np.testing.assert_array_equal(r.results.times, 2.0 * np.arange(Tb))
    assert r.results.amplitudes.shape == (1, n_blocks, P) and r.results.acf.shape == (1, n_blocks, P, Tb)
    assert r.results.units == {"results.times": "picosecond", "results.amplitudes": "angstrom^2"}
    amp, acf = _acf_ref(melt["X"], listed, n_blocks)
    np.testing.assert_allclose(r.results.amplitudes[0], amp, rtol=1e-9, atol=0)
    np.testing.assert_allclose(r.results.acf[0], acf, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(r.results.acf[..., 0], 1.0, rtol=0, atol=1e-12)
    direct = RouseModes(group, fft=False, **kw).run()
    np.testing.assert_allclose(direct.results.amplitudes, r.results.amplitudes, rtol=1e-9, atol=0)
    np.testing.assert_allclose(direct.results.acf, r.results.acf, rtol=1e-9, atol=1e-11)


def test_class_routes_and_discarded_frames(melt, tmp_path):
    from trajfiles import write_amber_netcdf
    pos = melt["pos"][:101]
    path = tmp_path / "melt.nc"
    write_amber_netcdf(path, pos, lengths=np.full((101, 3), 40.0), angles=np.full((101, 3), 90.0))
    d = _core.DeviceArray.from_host(pos)
    amp, acf = _acf_ref(melt["X"][:100], [1, 2, 3], 2)
    try:
        results = {}
        for name, u in (("host", mdhelper_amd.ArrayUniverse(pos, box([40.0] * 3), dt=2.0)),
                        ("hbm", mdhelper_amd.ArrayUniverse.from_device(d, box([40.0] * 3), dt=2.0)),
                        ("file", mdhelper_amd.FileUniverse(path, dt=2.0))):
            with pytest.warns(UserWarning, match="last 1 frame"):
                r = RouseModes(u.select(melt["index"]), n_chains=melt["M"], n_monomers=melt["N_p"], modes=3,
                               n_blocks=2, verbose=False).run()
            assert r.results.acf.shape == (1, 2, 3, 50)
            np.testing.assert_allclose(r.results.amplitudes[0], amp, rtol=1e-9, atol=0)
            np.testing.assert_allclose(r.results.acf[0], acf, rtol=1e-9, atol=1e-11)
            results[name] = r.results
        for name in ("hbm", "file"):                       # one set of bits whatever the route
            np.testing.assert_array_equal(results[name].amplitudes, results["host"].amplitudes)
            np.testing.assert_array_equal(results[name].acf, results["host"].acf)
    finally:
        d.free()


def test_class_residues_and_unwrap():
    L, F, M, N_p, size = 30.0, 40, 4, 12, 3
    dims = np.array([L, L, L])
    centres, cell = _drifting_chains(9, F, M, N_p, L, (3.8, 4.1, -3.7))
    rng = np.random.default_rng(10)
    # whole monomers of 3 atoms within 0.4 A of a wrapped centre: not wrapped themselves
    pos = (centres.astype(np.float64)[:, :, None, :] + rng.uniform(-0.4, 0.4, (F, M * N_p, size, 3)))
    pos = pos.reshape(F, -1, 3).astype(np.float32)
    atom_masses = rng.uniform(1.0, 16.0, M * N_p * size)
    points = centres_ref(pos, size, atom_masses)
    margin = []
    whole = unwrap_ref(points, points[0] + cell[0] * L, dims, margin)
    assert min(margin) > 1e-3
    modes = [1, 2, 5, 11]
    X = amplitudes_ref(whole, [M], [N_p], [rouse_weights(N_p, modes)]).reshape(F, len(modes), M, 3)
    want = np.stack([correlation.correlation_fft(X[:, k][None], axis=1, average=True, vector=True)[0]
                     for k in range(len(modes))])
    n = pos.shape[1]
    for topo, counts in (({}, {"n_chains": M, "n_monomers": N_p}),
                         ({"resids": np.arange(n) // size, "segids": np.arange(n) // (size * N_p)}, {})):
        u = mdhelper_amd.ArrayUniverse(pos, box(dims), masses=atom_masses, dt=1.0, **topo)
        r = RouseModes(u.atoms, "residues", modes=modes, unwrap=True, verbose=False, **counts).run()
        # the class makes the chains of frame 0 whole itself and may place them in another image: modes p >= 1
        # project a constant shift out, up to the rounding of x + k L
        np.testing.assert_allclose(r.results.amplitudes[0, 0], want[:, 0], rtol=1e-9, atol=0)
        np.testing.assert_allclose(r.results.acf[0, 0], want / want[:, :1], rtol=1e-9, atol=1e-11)


def test_relaxation_times_of_autoregressive_modes():
    """Chains whose mode amplitudes follow independent AR(1) series X(t + 1) = a_p X(t) + noise, built by the
    inverse transform r_n = sum_p 2 X_p cos(p pi (n + 1/2) / N_p): C_p(m) = a_p^m = exp(-m / tau_p), and the fitted
    relaxation time recovers tau_p within 10 % (series length and margin of
    ``test_end_to_end_relaxation_time_of_rotational_diffusion``)."""
    rng = np.random.default_rng(4)
    T, M, N_p = 4000, 600, 4
    taus = np.array([400.0, 100.0, 25.0])
    a = np.exp(-1.0 / taus)[None, :, None]
    modes = np.arange(1, N_p)
    basis = 2.0 * np.cos(np.pi * modes[:, None] * (np.arange(N_p) + 0.5) / N_p)       # [P, N_p]
    X = rng.normal(size=(M, 3, 3))                                                    # [chain, mode, xyz]
    pos = np.empty((T, M * N_p, 3), dtype=np.float32)
    for t in range(T):
        pos[t] = (10.0 + np.einsum("cpd,pn->cnd", X, basis)).reshape(-1, 3)
        X = a * X + np.sqrt(1.0 - a * a) * rng.normal(size=(M, 3, 3))
    uni = mdhelper_amd.ArrayUniverse(pos, box([20.0] * 3), dt=1.0)
    r = RouseModes(uni.atoms, n_chains=M, n_monomers=N_p, modes=3, verbose=False).run()
    r.calculate_relaxation_times()
    assert r.results.relaxation_times.shape == (1, 1, 3)
    print("tau fitted:", r.results.relaxation_times[0, 0], "expected:", taus)
    np.testing.assert_allclose(r.results.relaxation_times[0, 0], taus, rtol=0.1)
    np.testing.assert_allclose(r.results.amplitudes[0, 0], 3.0, rtol=0.1)             # <X_p^2> = 3 (unit variance per axis)
    m = np.arange(1, 100)
    np.testing.assert_allclose(r.results.acf[0, 0, :, 1:100], np.exp(-m[None] / taus[:, None]), rtol=0, atol=0.02)
