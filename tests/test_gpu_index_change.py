"""
A particle index that changes between calls on a live handle, and then repeats.

The engines keep the index they were last given in HBM and upload a new one only when it differs, after a wait
for the kernels and staging copies that may still read the old one.  The route suites give every handle one
index; here one handle takes index A, then B, then B again (kept), then A once more through a trajectory file,
for an engine of each family: the dipole engine (device side made on creation) and the cluster engine (device side
made by the first frame).  The results are those of a second handle that is fed the gathered rows ``big[f][index]``
through host memory, exactly: the dipole rows bit for bit, the cluster results count for count.
"""

import numpy as np
import pytest

from mdhelper_amd import _core

pytestmark = pytest.mark.gpu

BOX = np.array([20.0, 22.0, 24.0])
F = 6


def frames_and_indices(seed, n):
    """``F`` frames of ``2n + 5`` rows in the box, and two indices of ``n`` rows each, neither contiguous nor
    ascending, that select different rows."""
    rng = np.random.default_rng(seed)
    n_total = 2 * n + 5
    big = (rng.uniform(0.0, 1.0, (F, n_total, 3)) * BOX).astype(np.float32)
    a = rng.permutation(n_total)[:n].astype(np.int32)
    b = rng.permutation(n_total)[:n].astype(np.int32)
    for index in (a, b):
        assert np.any(np.diff(index) < 0) and np.any(np.abs(np.diff(index)) > 1)
    assert set(a) != set(b) and np.any(a != b)
    gathered = np.concatenate([big[0:2][:, a], big[2:4][:, b], big[4:5][:, b], big[5:6][:, a]])
    return big, a, b, np.ascontiguousarray(gathered)


def feed_changing_index(eng, big, a, b, tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd.io import TrajectoryFile
    n_total = big.shape[1]
    path = tmp_path / "big.nc"
    write_amber_netcdf(path, big, lengths=np.tile(BOX, (F, 1)), angles=np.full((F, 3), 90.0))
    d_big, tf = _core.DeviceArray.from_host(big), TrajectoryFile(path)
    try:
        eng.accumulate_device(d_big.rows(0, 2).ptr, n_total, 2, a)
        eng.accumulate_device(d_big.rows(2, 2).ptr, n_total, 2, b)      # another index while A's kernels may run
        eng.accumulate_device(d_big.rows(4, 1).ptr, n_total, 1, b)      # the same again: kept
        eng.accumulate_traj(tf, np.array([5]), a)                       # back to A, on the file route
        eng.synchronize()
    finally:
        tf.close()
        d_big.free()


def test_dipole_rows_follow_an_index_that_changes_and_repeats(tmp_path):
    n = 130                                     # one full tile of 128 and a ragged one of 2
    assert n == _core.DipoleEngine.TILE + 2
    big, a, b, gathered = frames_and_indices(41, n)
    charges = np.random.default_rng(42).normal(0.0, 1.0, n)
    eng, ref = _core.DipoleEngine([n], charges), _core.DipoleEngine([n], charges)
    try:
        feed_changing_index(eng, big, a, b, tmp_path)
        ref.accumulate(gathered)
        got, want = eng.result(), ref.result()
        assert got.shape == want.shape == (1, F, 3) and np.abs(want).min() > 0.0
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        # the two indices select different rows: frames 2 ... 4 under index A are other numbers
        wrong = _core.DipoleEngine([n], charges)
        try:
            wrong.accumulate(np.ascontiguousarray(big[:, a]))
            other = wrong.result()
        finally:
            wrong.close()
        np.testing.assert_array_equal(got[:, [0, 1, 5]].view(np.uint64), other[:, [0, 1, 5]].view(np.uint64))
        assert np.all(got[:, 2:5] != other[:, 2:5])
    finally:
        eng.close()
        ref.close()


def test_cluster_counts_follow_an_index_that_changes_and_repeats(tmp_path):
    n = 65                                      # a wave and one
    big, a, b, gathered = frames_and_indices(43, n)
    species, cutoff = np.zeros(n, dtype=np.int32), 4.0

    def collect(e):
        out = e.result()
        out.update(e.frames())
        out["labels"] = e.labels()
        return out

    eng = _core.ClusterEngine(species, cutoff, BOX, keep_labels=True)
    ref = _core.ClusterEngine(species, cutoff, BOX, keep_labels=True)
    try:
        feed_changing_index(eng, big, a, b, tmp_path)
        ref.accumulate(gathered)
        got, want = collect(eng), collect(ref)
        assert eng.stats()["frames"] == ref.stats()["frames"] == F
        # the frames hold bonds and clusters of several sizes: equal results are not equal zeros
        assert want["bonds"].min() > 0 and want["largest"].max() > 2 and np.all(want["n_clusters"] < n)
        assert sorted(got) == sorted(want)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        # the two indices select different rows: frames 2 ... 4 under index A bond differently
        wrong = _core.ClusterEngine(species, cutoff, BOX, keep_labels=True)
        try:
            wrong.accumulate(np.ascontiguousarray(big[:, a]))
            other = wrong.labels()
        finally:
            wrong.close()
        np.testing.assert_array_equal(got["labels"][[0, 1, 5]], other[[0, 1, 5]])
        assert all(np.any(got["labels"][f] != other[f]) for f in (2, 3, 4))
    finally:
        eng.close()
        ref.close()
