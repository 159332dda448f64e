"""
SingleChainStructureFactor on the MI355X against a float64 NumPy restatement of its definition
(reference polymer.py:1095-1130): per frame and chain (sum cos q.r)^2 + (sum sin q.r)^2, summed over
chains and frames, divided by n_chains * n_monomers * n_frames, then averaged over the wavevectors
whose wavenumber is numpy.isclose to each of np.unique(|q|.round(11)).
"""
import pathlib
import sys

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core
from mdhelper_amd.analysis import SingleChainStructureFactor

sys.path.insert(0, str(pathlib.Path(__file__).parent))

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9


def _grid(dims, n_points):
    return np.stack(np.meshgrid(*[2 * np.pi * np.arange(n_points) / L for L in dims]), -1).reshape(-1, 3)


def _isclose_mean(values, q):
    wn = np.linalg.norm(q, axis=1)
    unique = np.unique(wn.round(11))
    return unique, np.array([values[np.isclose(v, wn)].mean() for v in unique])


def _restate(points, dims, n_points, n_chains):
    """points float[F, N, 3] (the float32 values the device sees, widened)."""
    q = _grid(dims, n_points)
    p = np.asarray(points, dtype=np.float64)
    F, N = p.shape[:2]
    acc = np.zeros(len(q))
    for f in range(F):
        qr = p[f].reshape(n_chains, N // n_chains, 3) @ q.T
        acc += (np.cos(qr).sum(axis=1) ** 2 + np.sin(qr).sum(axis=1) ** 2).sum(axis=0)
    return _isclose_mean(acc / (N * F), q)


def _melt(M, Np, F, dims, seed=0, bond=1.0):
    """Random-walk chains wrapped into the box, float32."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=float)
    start = rng.random((F, M, 1, 3)) * dims
    steps = rng.normal(0, bond / np.sqrt(3), (F, M, Np, 3))
    steps[:, :, 0] = 0
    pos = (start + np.cumsum(steps, axis=2)).reshape(F, M * Np, 3)
    return np.mod(pos, dims).astype(np.float32)


def _check(u, M, Np, n_points, dims, frames=None, **run):
    s = SingleChainStructureFactor(u.atoms, n_points=n_points, n_chains=M, n_monomers=Np).run(**run)
    pos = u.trajectory.frame_block(np.arange(u.trajectory.n_frames) if frames is None else frames)
    wn, ref = _restate(pos, dims, n_points, M)
    np.testing.assert_array_equal(s.results.wavenumbers, wn)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=RTOL, atol=ATOL)
    assert s.results.units == {"results.wavenumbers": "angstrom^-1"}
    return s


@pytest.mark.parametrize("M, Np, n_points, F", [(40, 10, 5, 6), (7, 37, 8, 3), (9, 37, 6, 2), (2, 3000, 4, 2)])
def test_atoms_against_restatement(M, Np, n_points, F):
    dims = (15.0, 15.0, 15.0)
    u = mdhelper_amd.ArrayUniverse(_melt(M, Np, F, dims), [*dims, 90, 90, 90])
    _check(u, M, Np, n_points, dims)


def test_non_cubic_box():
    dims = (12.0, 17.5, 21.25)
    u = mdhelper_amd.ArrayUniverse(_melt(20, 16, 3, dims, seed=3), [*dims, 90, 90, 90])
    _check(u, 20, 16, 8, dims)


@pytest.mark.parametrize("n_points", [1, 2])
def test_tiny_grids(n_points):
    dims = (10.0, 10.0, 10.0)
    u = mdhelper_amd.ArrayUniverse(_melt(6, 5, 2, dims, seed=4), [*dims, 90, 90, 90])
    _check(u, 6, 5, n_points, dims)


def test_default_grid():
    dims = (20.0, 20.0, 20.0)
    u = mdhelper_amd.ArrayUniverse(_melt(25, 40, 2, dims, seed=5), [*dims, 90, 90, 90])
    s = SingleChainStructureFactor(u.atoms, n_chains=25, n_monomers=40).run()
    wn, ref = _restate(u.trajectory.frame_block(np.arange(2)), dims, 32, 25)
    np.testing.assert_array_equal(s.results.wavenumbers, wn)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=RTOL, atol=ATOL)


def test_frame_selections():
    dims = (15.0, 15.0, 15.0)
    u = mdhelper_amd.ArrayUniverse(_melt(12, 11, 9, dims, seed=6), [*dims, 90, 90, 90])
    _check(u, 12, 11, 6, dims, frames=np.arange(1, 8, 3), start=1, stop=8, step=3)
    s = SingleChainStructureFactor(u.atoms, n_points=6, n_chains=12, n_monomers=11).run(frames=[0, 4, 5, 8])
    wn, ref = _restate(u.trajectory.frame_block(np.array([0, 4, 5, 8])), dims, 6, 12)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(s.frames, [0, 4, 5, 8])


def test_one_monomer_chains_give_one():
    dims = (10.0, 10.0, 10.0)
    u = mdhelper_amd.ArrayUniverse(_melt(50, 1, 3, dims, seed=7), [*dims, 90, 90, 90])
    for n_points in (5, 8):
        s = SingleChainStructureFactor(u.atoms, n_points=n_points, n_chains=50, n_monomers=1).run()
        np.testing.assert_allclose(s.results.scsf, 1.0, rtol=1e-12, atol=0)


def test_dimers_closed_form():
    dims = (10.0, 10.0, 10.0)
    rng = np.random.default_rng(8)
    M, F = 30, 4
    d = rng.normal(0, 1.0, (M, 3))
    first = rng.random((F, M, 3)) * 10
    pos = np.stack([first, first + d], axis=2).reshape(F, 2 * M, 3).astype(np.float32)
    d32 = pos[:, 1::2].astype(float) - pos[:, ::2].astype(float)       # the bond the device sees
    u = mdhelper_amd.ArrayUniverse(pos, [*dims, 90, 90, 90])
    s = SingleChainStructureFactor(u.atoms, n_points=8, n_chains=M, n_monomers=2).run()
    q = _grid(dims, 8)
    closed = 1 + np.mean(np.cos(d32 @ q.T), axis=(0, 1))
    _, ref = _isclose_mean(closed, q)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=RTOL, atol=ATOL)


def test_q_zero_is_chain_length():
    dims = (15.0, 15.0, 15.0)
    for M, Np, n_points in [(7, 37, 8), (40, 10, 5)]:
        u = mdhelper_amd.ArrayUniverse(_melt(M, Np, 2, dims, seed=9), [*dims, 90, 90, 90])
        s = SingleChainStructureFactor(u.atoms, n_points=n_points, n_chains=M, n_monomers=Np).run()
        assert s.results.wavenumbers[0] == 0.0
        assert abs(s.results.scsf[0] - Np) <= 1e-12 * Np


def test_residues_explicit_counts():
    dims = (15.0, 15.0, 15.0)
    M, Np, A, F = 8, 12, 3, 3
    pos = _melt(M, Np * A, F, dims, seed=10, bond=0.5)
    masses = np.tile([12.0, 1.0, 16.0], M * Np)
    u = mdhelper_amd.ArrayUniverse(pos, [*dims, 90, 90, 90], masses=masses)
    s = SingleChainStructureFactor(u.atoms, "residues", n_points=6, n_chains=M, n_monomers=Np).run()
    p = pos.astype(float).reshape(F, M * Np, A, 3)
    com = ((p * masses[:A, None]).sum(axis=2) / masses[:A].sum()).astype(np.float32)
    wn, ref = _restate(com, dims, 6, M)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=1e-5, atol=1e-8)


def test_residues_from_topology():
    dims = (15.0, 15.0, 15.0)
    M, Np, A, F = 6, 10, 2, 3
    pos = _melt(M, Np * A, F, dims, seed=11, bond=0.5)
    masses = np.tile([3.0, 1.0], M * Np)
    resids = np.arange(M * Np * A) // A
    segids = np.arange(M * Np * A) // (Np * A)
    u = mdhelper_amd.ArrayUniverse(pos, [*dims, 90, 90, 90], masses=masses, resids=resids, segids=segids)
    s = SingleChainStructureFactor(u.atoms, "residues", n_points=6).run()
    assert (s._n_chains, s._n_monomers) == (M, Np)
    p = pos.astype(float).reshape(F, M * Np, A, 3)
    com = ((p * masses[:A, None]).sum(axis=2) / masses[:A].sum()).astype(np.float32)
    wn, ref = _restate(com, dims, 6, M)
    np.testing.assert_allclose(s.results.scsf, ref, rtol=1e-5, atol=1e-8)


def test_unwrap_changes_nothing():
    dims = (10.0, 10.0, 10.0)
    u = mdhelper_amd.ArrayUniverse(_melt(10, 30, 3, dims, seed=12), [*dims, 90, 90, 90])
    a = SingleChainStructureFactor(u.atoms, n_points=8, n_chains=10, n_monomers=30, unwrap=False).run()
    b = SingleChainStructureFactor(u.atoms, n_points=8, n_chains=10, n_monomers=30, unwrap=True).run()
    np.testing.assert_allclose(b.results.scsf, a.results.scsf, rtol=1e-12, atol=0)


def test_ingest_routes_agree(tmp_path):
    from trajfiles import write_amber_netcdf
    from mdhelper_amd import _core
    dims = (15.0, 15.0, 15.0)
    pos = _melt(16, 20, 5, dims, seed=13)
    kw = dict(n_points=8, n_chains=16, n_monomers=20)
    host = SingleChainStructureFactor(mdhelper_amd.ArrayUniverse(pos, [*dims, 90, 90, 90]).atoms, **kw).run()
    d = _core.DeviceArray.from_host(pos)
    try:
        dev = SingleChainStructureFactor(mdhelper_amd.ArrayUniverse.from_device(d, [*dims, 90, 90, 90]).atoms,
                                         **kw).run()
    finally:
        d.free()
    path = tmp_path / "chains.nc"
    write_amber_netcdf(path, pos, lengths=np.tile(dims, (5, 1)), angles=np.tile([90.0] * 3, (5, 1)))
    fil = SingleChainStructureFactor(mdhelper_amd.FileUniverse(path, dt=1.0).atoms, **kw).run()
    for other in (dev, fil):
        np.testing.assert_allclose(other.results.scsf, host.results.scsf, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n_points", [6, 8])
def test_quad_and_plain_kernels_agree(monkeypatch, n_points):
    dims = (15.0, 15.0, 15.0)
    u = mdhelper_amd.ArrayUniverse(_melt(9, 37, 3, dims, seed=14), [*dims, 90, 90, 90])
    kw = dict(n_points=n_points, n_chains=9, n_monomers=37)
    plan = lambda: _core.SqEngine.plan(_grid(dims, n_points), (9 * 37,), 3, 37)["route"]      # noqa: E731
    assert plan() == 3                                  # sq_chain_quads_kernel
    quad = SingleChainStructureFactor(u.atoms, **kw).run()
    monkeypatch.setenv("MDX_SQ_NO_QUADS", "1")
    assert plan() == 0                                  # sq_chain_sincos_kernel
    plain = SingleChainStructureFactor(u.atoms, **kw).run()
    np.testing.assert_allclose(quad.results.scsf, plain.results.scsf, rtol=1e-10, atol=0)


def test_runs_are_bit_identical():
    dims = (20.0, 20.0, 20.0)
    u = mdhelper_amd.ArrayUniverse(_melt(25, 40, 3, dims, seed=15), [*dims, 90, 90, 90])
    a = SingleChainStructureFactor(u.atoms, n_points=16, n_chains=25, n_monomers=40).run()
    b = SingleChainStructureFactor(u.atoms, n_points=16, n_chains=25, n_monomers=40).run()
    assert np.array_equal(a.results.scsf, b.results.scsf)


class _EchoComm:
    """World size 2, this process plays `rank`; allreduce returns its input."""

    def __init__(self, rank):
        self.rank, self.world_size = rank, 2

    def allreduce(self, arr, op="sum"):
        return arr

    def barrier(self):
        pass


def test_frame_sharding_adds_up():
    dims = (15.0, 15.0, 15.0)
    u = mdhelper_amd.ArrayUniverse(_melt(10, 12, 7, dims, seed=16), [*dims, 90, 90, 90])
    kw = dict(n_points=6, n_chains=10, n_monomers=12)
    whole = SingleChainStructureFactor(u.atoms, **kw).run()
    parts = [SingleChainStructureFactor(u.atoms, comm=_EchoComm(r), **kw).run() for r in (0, 1)]
    np.testing.assert_allclose(parts[0].results.scsf + parts[1].results.scsf, whole.results.scsf,
                               rtol=1e-12, atol=1e-15)
