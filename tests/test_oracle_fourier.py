"""
Oracle pinning: oracle.fourier against the reference's accelerated.py loop
bodies (tests/golden/fourier_ref.npz) and analytic lattice answers.
"""
import numpy as np
import pytest

from oracle import fourier as of


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "fourier_ref.npz")


def test_fourier_sum_matches_reference(g):
    assert np.allclose(of.fourier_sum_ref(g["qs"], g["rs"]), g["out_fourier_sum"], rtol=1e-12, atol=1e-10)
    assert np.allclose(of.fourier_sum_ref(g["qs"], g["rs2"]), g["out_fourier_sum_parallel"], rtol=1e-12, atol=1e-10)
    assert np.allclose(of.inner_ref(g["qs"], g["rs"]), g["out_inner"], rtol=0, atol=1e-12)


def test_trig_form_matches_reference(g):
    n1, n2 = len(g["rs"]), len(g["rs2"])
    pos = np.vstack((g["rs"], g["rs2"]))
    slices = [slice(0, n1), slice(n1, n1 + n2)]
    pairs = of.ssf_pairs(2, "partial")
    trig = of.ssf_frame_ref(g["qs"], pos, slices, pairs, "partial", "trig")
    expf = of.ssf_frame_ref(g["qs"], pos, slices, pairs, "partial", "exp")
    assert np.allclose(trig[0], g["out_pythag"], rtol=1e-10, atol=1e-8)
    assert np.allclose(trig[1], g["out_pythag_cross"], rtol=1e-10, atol=1e-8)
    assert np.allclose(trig, expf, rtol=1e-9, atol=1e-7)


def test_simple_cubic_bragg_peaks():
    """S(q) of a perfect simple-cubic lattice: N at reciprocal-lattice vectors, 0 elsewhere on the grid."""
    n, a = 4, 1.5
    L = n * a
    idx = np.arange(n)
    pos = a * np.stack(np.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3)
    q = of.grid_wavevectors([L, L, L], 2 * n)
    res = of.ssf_run_ref(pos[None].astype(np.float64), [n ** 3], q, sort=False, unique=False)
    m = np.rint(q * L / (2 * np.pi)).astype(int)
    bragg = np.all(m % n == 0, axis=1)
    assert np.allclose(res["ssf"][0][bragg], n ** 3)
    assert np.allclose(res["ssf"][0][~bragg], 0, atol=1e-9)


def test_meshgrid_row_order():
    q = of.grid_wavevectors([10.0, 10.0, 10.0], 3)
    g1 = 2 * np.pi / 10.0
    # numpy.meshgrid default 'xy' indexing: row index = (j, i, k)
    assert np.allclose(q[1], [0, 0, g1])
    assert np.allclose(q[3], [g1, 0, 0])
    assert np.allclose(q[9], [0, g1, 0])


@pytest.mark.parametrize("mode", [None, "partial", "pair"])
def test_isf_definition_agrees_with_the_restated_driver(mode):
    """``isf_definition_ref`` (no ring, extended precision) against ``isf_run_ref`` (the reference's ring, float64)
    with its normalisation undone; the error scales S, the slots, exact zeros and the span are what they are meant
    to be."""
    rng = np.random.default_rng(5)
    F, sizes, n_lags = 9, (11, 4, 7), 5
    N = sum(sizes)
    pos = (rng.random((F, N + 3, 3)) * 12.0).astype(np.float32)        # three rows beyond the groups' span
    q = rng.normal(0.0, 1.5, (13, 3))
    pairs = of.ssf_pairs(3, mode)
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    got = of.isf_definition_ref(pos, offsets, pairs, q, n_lags)
    want = of.isf_run_ref(pos, sizes, q, n_lags, mode=mode, incoherent=True, sort=False, unique=False)
    norm = N * np.arange(F, F - n_lags, -1)[:, None, None]
    assert np.allclose(got["cisf"], want["cisf"] * norm, rtol=1e-11, atol=1e-10)
    assert np.allclose(got["iisf"], want["iisf"] * norm, rtol=1e-11, atol=1e-10)
    assert np.all(np.abs(got["cisf"]) <= got["S_cisf"] * (1 + 1e-12))
    slot_sizes = {None: [N], "partial": sizes, "pair": [0, 0, 0]}[mode]
    for lag in range(n_lags):
        for slot, n in enumerate(slot_sizes):
            assert np.all(got["S_iisf"][lag, slot] == n * (F - lag))
            assert np.all(got["iisf"][0, slot] == n * F)             # cos(0) = 1, summed exactly
    assert got["phi_max"] == pytest.approx(np.abs(of.inner_ref(q, pos[:, :N].reshape(-1, 3))).max(), rel=1e-12)
    # an arbitrary pair list: one slot per group, zero without a diagonal pair; lags beyond the frames are zero
    custom = of.isf_definition_ref(pos[:3], offsets, ((1, 1), (0, 2)), q, n_lags)
    assert not custom["iisf"][:, 0].any() and not custom["iisf"][:, 2].any() and custom["iisf"][:3, 1].all()
    assert not custom["cisf"][3:].any() and not custom["iisf"][3:].any() and not custom["S_cisf"][3:].any()
    partial = of.isf_definition_ref(pos[:3], offsets, of.ssf_pairs(3, "partial"), q, n_lags)
    assert np.array_equal(custom["cisf"][:, 0], partial["cisf"][:, 3])       # (1, 1)
    assert np.array_equal(custom["cisf"][:, 1], partial["cisf"][:, 2])       # (0, 2)


def test_molecule_centres_follow_the_kernel_statement():
    rng = np.random.default_rng(6)
    sizes = np.resize([1, 2, 5], 11)
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    masses = rng.uniform(1.0, 30.0, offsets[-1])
    pos = (rng.random((4, offsets[-1], 3)) * 50.0).astype(np.float32)
    got = of.molecule_centres_ref(pos, offsets, masses)
    assert got.dtype == np.float32 and got.shape == (4, 11, 3)
    for f in range(4):
        for g in range(11):
            acc, total = np.zeros(3), 0.0
            for a in range(offsets[g], offsets[g + 1]):                  # sequential, separate multiply and add
                acc = acc + masses[a] * pos[f, a].astype(np.float64)
                total = total + masses[a]
            assert np.array_equal(got[f, g], (acc / total).astype(np.float32))
    assert np.array_equal(got[:, 0], pos[:, 0])                          # a molecule of one atom: m x / m
