"""
Polymer dynamics and structure (operator surface of ``mdhelper.analysis.polymer``):
``EndToEndVector`` — the end-to-end vector autocorrelation function of polymer chains and the
orientational relaxation time fitted to it — and ``SingleChainStructureFactor`` — the
single-chain structure factor on the reciprocal grid.

Mirrors reference ``src/mdhelper/analysis/polymer.py``: ``correlation_fft`` /
``correlation_shift`` aliases (:30-57), ``calculate_relaxation_time`` (:59-108),
``_PolymerAnalysisBase.__init__`` (:175-237), ``Gyradius`` (:239-508) and ``EndToEndVector``
(:510-803) keep their names, arguments, defaults, result attributes and error behaviour.

Where the work goes: the reference stores ``e2e[T, N_chains, 3]`` frame by frame and calls
``correlation_fft(..., average=True, vector=True)`` per group (:765-781), which transforms
every chain and component on one core.  Here the unit vectors of a group are pushed to the
correlation engine of ``Onsager`` (``mdx_msd_push``), whose device pipeline sums the power
spectra over chains and components and inverts once per (group, block); the ACF is
``mdx_msd_result_acf / (M (T_b - m))``.  The end positions of in-memory and native-file
trajectories are gathered for all frames in one vectorised step; unwrapping is the same
image-flag rule as ``unwrap`` (topology.py:366-376), evaluated for all frames at once.
With ``comm=`` the chains shard across ranks (one all-reduce of the accumulators).

``SingleChainStructureFactor`` (reference :805-1130) runs on the structure-factor engine in
single-chain mode (``mdx_sq_set_chains``): per frame and chain the device forms
``rho_c(q) = sum_{j in c} exp(i q.r_j)`` and adds ``|rho_c|^2``; frames shard across ranks.

``Gyradius`` runs on the gyration engine (``mdx_gyr_*``): per frame the device forms the monomer
centres of mass, follows the points across the boundaries (``unwrap``), and computes every
chain's centre of mass and mass-weighted second moments in float64; frames shard across ranks.

``RouseModes`` (an extension; the reference has no such analysis) runs on the chain-projection engine
(``mdx_rouse_*``): per frame and chain the device forms ``X_p = sum_n w_pn r_n`` for every requested mode in
float64 and keeps the amplitudes in HBM, where the correlation engine reads them (``mdx_msd_push_device``);
the chains of each (group, mode) shard across ranks.

``InternalDistances`` (an extension; the reference has no such analysis) runs on the internal-distance engine
(``mdx_msid_*``): per frame and group the device sums ``|r_{i+s} - r_i|^2`` and ``b_i . b_{i+s}`` over every pair of
monomers and of bonds of every chain, in float64 out of LDS; ``whole=True`` makes the chains whole per frame on the
device, so wrapped trajectories still shard by frame across ranks.
"""

from __future__ import annotations

import warnings
from typing import Union

import numpy as np
from scipy import optimize, special

from .. import _core
from ..algorithm import correlation
from ..algorithm.topology import unwrap_edge
from ..algorithm.unit import strip_unit
from ..comm import shard_range
from .base import DynamicAnalysisBase, EngineFedAnalysis, block_frames, grouping_of, has_frame_blocks

_GROUPINGS = {"atoms", "residues"}


def correlation_fft(*args, **kwargs):
    """Alias of :func:`mdhelper_amd.algorithm.correlation.correlation_fft` (reference :30-42)."""
    return correlation.correlation_fft(*args, **kwargs)


def correlation_shift(*args, **kwargs) -> np.ndarray:
    """Alias of :func:`mdhelper_amd.algorithm.correlation.correlation_shift` (reference :44-57)."""
    return correlation.correlation_shift(*args, **kwargs)


def stretched_exp(x, alpha, beta):
    r""":math:`y=\exp[-(x/\alpha)^\beta]` (reference fit/exponential.py:205-231)."""
    return np.exp(-(x / alpha) ** beta)


def calculate_relaxation_time(time: np.ndarray, acf: np.ndarray) -> float:
    r"""
    Orientational relaxation time :math:`\tau_\mathrm{r}=\tau\,\Gamma(1+1/\beta)` from a
    stretched-exponential fit :math:`C_\mathrm{ee}=\exp[-(t/\tau)^\beta]` to the end-to-end
    vector ACF (reference :59-108; the time axis is scaled by ``time[1]`` for the fit).
    """
    tau_r, beta = optimize.curve_fit(stretched_exp, time / time[1], acf, bounds=(0, np.inf))[0]
    return tau_r * time[1] * special.gamma(1 + beta ** -1)


class _PolymerAnalysisBase(DynamicAnalysisBase):
    """
    Argument handling shared by the polymer analyses (reference :110-237).

    groups : AtomGroup or sequence of AtomGroups — all chains of a group have the same length
    groupings : {"atoms", "residues"} or one per group
    n_chains, n_monomers : int or one per group, optional — chains per group and monomers per
        chain when the trajectory carries no segment / residue information
    unwrap : bool, keyword-only
    """

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms", n_chains=None,
                 n_monomers=None, *, unwrap: bool = False, parallel: bool = False,
                 verbose: bool = True, **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "universe") else list(groups)
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, parallel, verbose, **kwargs)

        self._dimensions = self.universe.dimensions
        if self._dimensions is not None:
            self._dimensions = np.array(self._dimensions[:3], dtype=float)

        self._n_groups = len(self._groups)
        if isinstance(groupings, str):
            if groupings not in _GROUPINGS:
                raise ValueError(f"Invalid grouping '{groupings}'. Valid values: "
                                 f"{', '.join(sorted(_GROUPINGS))}.")
            self._groupings = self._n_groups * [groupings]
        else:
            if self._n_groups != len(groupings):
                raise ValueError("The number of grouping values is not equal to the "
                                 "number of groups.")
            for g in groupings:
                if g not in _GROUPINGS:
                    raise ValueError(f"Invalid grouping '{g}'. Valid values: "
                                     f"{', '.join(sorted(_GROUPINGS))}.")
            self._groupings = list(groupings)

        if n_chains is None or n_monomers is None:
            self._internal = True
            self._n_chains = np.empty(self._n_groups, dtype=int)
            self._n_monomers = np.empty_like(self._n_chains)
            for i, g in enumerate(self._groups):
                self._n_chains[i] = g.segments.n_segments
                self._n_monomers[i] = g.n_atoms // self._n_chains[i]
        else:
            self._internal = False
            if isinstance(n_chains, (int, np.integer)):
                self._n_chains = n_chains * np.ones(self._n_groups, dtype=int)
            elif self._n_groups == len(n_chains):
                self._n_chains = np.asarray(n_chains, dtype=int)
            else:
                raise ValueError("The number of polymer counts is not equal to the "
                                 "number of groups.")
            if isinstance(n_monomers, (int, np.integer)):
                # (the reference sizes this array by n_monomers, :226; one entry per group is meant)
                self._n_monomers = n_monomers * np.ones(self._n_groups, dtype=int)
            elif self._n_groups == len(n_monomers):
                self._n_monomers = np.asarray(n_monomers, dtype=int)
            else:
                raise ValueError("The number of chain lengths is not equal to the "
                                 "number of groups.")

        self._unwrap = unwrap
        self._verbose = verbose

    # ---------------------------------------------------------------- points of whole chains
    # (shared by the analyses whose engines take every monomer of every chain: Gyradius, RouseModes, InternalDistances)

    def _setup_points(self) -> None:
        """Chain lengths read from the topology, the group-size and ``unwrap`` checks, and the groups' point
        ranges ``_Ns`` / ``_N`` / ``_slices``."""
        if self._internal:
            for i, (g, gr) in enumerate(zip(self._groups, self._groupings)):
                seg = np.asarray(g.segindices)
                if gr == "residues":
                    _, first = np.unique(np.asarray(g.resindices), return_index=True)
                    _, per_seg = np.unique(seg[first], return_counts=True)      # residues per segment
                    what = "residues"
                else:
                    _, per_seg = np.unique(seg, return_counts=True)
                    what = "atoms"
                if np.any(per_seg != per_seg[0]):
                    raise ValueError(f"All segments of group {i} must hold the same number of {what}.")
                self._n_monomers[i] = per_seg[0]
        for i, (g, gr, M, N_p) in enumerate(zip(self._groups, self._groupings, self._n_chains,
                                                self._n_monomers)):
            N = int(M) * int(N_p)
            if gr == "atoms" or self._internal:
                n_have = g.n_atoms if gr == "atoms" else len(np.unique(np.asarray(g.resindices)))
                bad = N <= 0 or n_have != N
            else:
                n_have = g.n_atoms
                bad = N <= 0 or n_have == 0 or n_have % N != 0
            if bad:
                what = "atoms" if gr == "atoms" or not self._internal else "residues"
                raise ValueError(f"Group {i} holds {n_have} {what}, which do not form n_chains * "
                                 f"n_monomers = {M} * {N_p} = {N} monomers.")
        if self._unwrap:
            if self._comm.world_size > 1:
                raise ValueError("unwrap cannot be combined with more than one rank: the image counts "
                                 "run from frame to frame, so the frames cannot shard.  Run it on one "
                                 "rank.")
            if self._dimensions is None:
                raise ValueError("No system dimensions found: unwrapping is not possible.")

        self._Ns = np.fromiter((M * N_p for M, N_p in zip(self._n_chains, self._n_monomers)),
                               dtype=int, count=self._n_groups)
        self._N = self._Ns.sum()
        self._slices = []
        index = 0
        for N in self._Ns:
            self._slices.append(slice(index, index + N))
            index += N

    def _selection(self, g, gr, N):
        """(particle indices monomer by monomer, monomer offsets or None, particle masses, monomer
        masses) of a group of ``N`` monomers."""
        idx = np.asarray(g.indices)
        masses = np.asarray(g.masses, dtype=np.float64)
        if gr == "atoms":
            return idx, None, masses, masses
        if not self._internal:
            # a monomer is n_atoms / N consecutive atoms
            offsets = np.arange(N + 1, dtype=np.int64) * (g.n_atoms // N)
        else:
            # residues of the topology, monomer by monomer; a chain is a segment
            _, inverse = np.unique(np.asarray(g.resindices), return_inverse=True)
            order = np.argsort(inverse, kind="stable")
            offsets = np.concatenate(([0], np.cumsum(np.bincount(inverse)))).astype(np.int64)
            n_chains = len(np.unique(np.asarray(g.segindices)))
            seg = np.asarray(g.segindices)[order][offsets[:-1]].reshape(n_chains, -1)
            if np.any(seg != seg[:, :1]) or len(np.unique(seg[:, 0])) != n_chains:
                raise ValueError("The residues of every segment must be consecutive.")
            idx, masses = idx[order], masses[order]
        return idx, offsets, masses, np.add.reduceat(masses, offsets[:-1])

    def _start(self, sels):
        """float64[N, 3]: the points of the current frame with every chain made whole."""
        pos = np.asarray(self.universe.trajectory.ts.positions, dtype=float)
        start = np.empty((self._N, 3))
        for (idx, off, m, pm), s, M, N_p in zip(sels, self._slices, self._n_chains, self._n_monomers):
            points = pos[idx]
            if off is not None:
                points = np.add.reduceat(points * m[:, None], off[:-1], axis=0) / pm[:, None]
            bonds = (np.arange(M)[:, None] * N_p + np.arange(N_p - 1)[None, :]).ravel()
            start[s] = unwrap_edge(positions=points, bonds=np.stack((bonds, bonds + 1), axis=1),
                                   dimensions=self._dimensions, masses=pm)
        return start

    def _feed_points(self, engine, sels) -> None:
        """Hands the grouping (monomers of several atoms), the unwrap start and the rows of a frame — those of
        ``sels``, the ``_selection`` of every group, in concatenated-group order — to a chain engine."""
        grouping = grouping_of([sel[:3] for sel in sels])
        if grouping is not None:
            engine.set_grouping(*grouping)
        if self._unwrap:
            st = self._sliced_trajectory
            self.universe.trajectory[st.frames[0] if hasattr(st, "frames") else (self.start or 0)]
            engine.set_unwrap(self._dimensions, self._start(sels))
        self._feed_engine(engine, np.concatenate([sel[0] for sel in sels]))


class Gyradius(EngineFedAnalysis, _PolymerAnalysisBase):
    r"""
    Radius of gyration of polymer chains (reference :239-508),

    .. math:: R_\mathrm g=\sqrt{\frac{\sum_i m_i\|\mathbf r_i-\mathbf R_\mathrm{com}\|^2}{\sum_i m_i}}

    per frame, averaged over the chains of each group; with ``components=True`` the radii around the
    coordinate axes instead (:math:`R_{\mathrm g,x}` from the :math:`y` and :math:`z` components, ...).

    Parameters (reference :337-343)
    ----------
    groups, groupings, n_chains, n_monomers : see ``_PolymerAnalysisBase``; a group holds
        ``n_chains * n_monomers`` monomers, chain after chain
    components : bool, keyword-only — the three radii around the axes instead of :math:`R_\mathrm g`
    unwrap : bool, keyword-only — follow the monomers across the periodic boundaries from frame to
        frame, starting from chains made whole in the first analysed frame
    parallel : bool, keyword-only — accepted; the serial result layout is returned
    comm, device : keyword-only (extension) — frames shard across ranks, one all-reduce at the end

    Results: ``results.gyradii`` ``[N_g, N_t]`` (``[N_g, N_t, 3]`` with ``components=True``, Å),
    ``results.units``.

    Where this differs from the reference:

    * A monomer's mass is the sum of its atoms' masses.  The reference reshapes the *atom* masses to
      ``(n_chains, n_monomers)``, which only runs with one atom per monomer; there both agree.
    * ``"residues"`` read from the topology: one chain per segment and ``n_monomers`` = residues per
      segment, as in ``SingleChainStructureFactor``.  The reference uses atoms per chain.
    * Image shifts are applied in float64 (the reference adds ``images * dimensions`` to the float32
      positions, topology.py:376).
    * ``parallel`` is accepted and returns the serial layout ``[N_g, N_t(, 3)]``.
    * A scalar ``n_monomers`` gives one entry per group (the reference sizes that array by
      ``n_monomers``, :226).
    * ``unwrap=True`` with more than one rank raises ``ValueError``: the image counts run from frame to
      frame, so the frames cannot shard.  ``unwrap=True`` without box dimensions, and groups whose size
      does not match ``n_chains * n_monomers``, raise ``ValueError`` at construction.
    * The chains of the first analysed frame are made whole along bonds between consecutive monomers
      (``unwrap_edge``), for ``"residues"`` on the monomers' centres of mass; the array universes carry
      no fragments for ``make_whole`` (:380-383).
    * There is no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms", n_chains=None,
                 n_monomers=None, *, components: bool = False, unwrap: bool = False,
                 parallel: bool = False, verbose: bool = True, **kwargs) -> None:
        super().__init__(groups, groupings, n_chains, n_monomers, unwrap=unwrap, parallel=parallel,
                         verbose=verbose, **kwargs)
        self._setup_points()
        self._components = components

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # (unwrap, which makes the frames sequential, runs on one rank)

    def _prepare(self) -> None:
        shape = [self._n_groups, self.n_frames]
        if self._components:
            shape.append(3)
        self.results.gyradii = np.empty(shape)
        self.results.units = {"results.gyradii": "angstrom"}

        # rows of every frame in concatenated-group order, sorted monomer by monomer; the monomers'
        # centres of mass are formed on the device (plain-atom groups: monomers of one particle)
        sels = [self._selection(g, gr, int(N)) for g, gr, N in zip(self._groups, self._groupings, self._Ns)]
        self._feed_points(_core.GyrationEngine(self._n_chains, self._n_monomers,
                                               np.concatenate([sel[3] for sel in sels]), dev=self._device), sels)

    def _conclude(self) -> None:
        self._batch.flush()
        radii = self._engine.result()                       # [N_g, frames of this rank, 4]
        self._engine.close()
        self.results.gyradii = self._gather_frame_rows(radii[..., 1:] if self._components else radii[..., 0], 1)


class EndToEndVector(_PolymerAnalysisBase):
    r"""
    End-to-end vector ACF :math:`C_\mathrm{ee}(t)=\langle\hat{\mathbf R}_\mathrm{ee}(t)\cdot
    \hat{\mathbf R}_\mathrm{ee}(0)\rangle` of polymer chains, :math:`\mathbf R_\mathrm{ee}=
    \mathbf r_N-\mathbf r_1`, and the orientational relaxation time (reference :510-803).

    Parameters (reference :651-656)
    ----------
    groups, groupings, n_chains, n_monomers : see ``_PolymerAnalysisBase``
    n_blocks : int, keyword-only — blocks the trajectory is split into
    dt : float, keyword-only, optional — time between frames (ps)
    fft : bool, keyword-only — FFT-based ACF on the GPU (``False``: direct sliding windows, NumPy)
    unwrap : bool, keyword-only — follow the end monomers across the periodic boundaries
    comm : communicator, keyword-only (extension) — chains shard across ranks

    Results: ``results.times`` ``[N_t]``, ``results.acf`` ``[N_g, N_b, N_t]``, ``results.units``;
    ``results.relaxation_times`` ``[N_g, N_b]`` after ``calculate_relaxation_time()``.
    """

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms", n_chains=None,
                 n_monomers=None, *, n_blocks: int = 1, dt=None, fft: bool = True,
                 unwrap: bool = False, verbose: bool = True, **kwargs) -> None:
        kwargs.pop("parallel", None)          # no parallel variant of this class (:659-660)
        super().__init__(groups, groupings, n_chains, n_monomers, unwrap=unwrap,
                         verbose=verbose, **kwargs)
        self._N_chains = int(self._n_chains.sum())
        self._slices = []
        index = 0
        for N in self._n_chains:
            self._slices.append(slice(index, index + N))
            index += N
        self._n_blocks = n_blocks
        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._fft = fft

    # ---------------------------------------------------------------- end monomers

    def _end_selection(self, g, gr, M, N_p):
        """Atoms and weights forming the first and last monomer position of every chain:
        ``(index[K], slot_start[2 M], weight[K])`` with the atoms of slot ``2 c + e`` (chain c,
        end e) contiguous; positions_end[c, e] = sum w x (reference :741-757)."""
        if self._internal and gr == "residues":
            # first and last residue of every segment, centres of mass
            seg, res, masses = g.segindices, g.resindices, g.masses
            idx, start, w = [], [], []
            for s in _ordered_unique(seg):
                in_seg = np.flatnonzero(seg == s)
                residues = _ordered_unique(res[in_seg])
                for r in (residues[0], residues[-1]):
                    atoms = in_seg[res[in_seg] == r]
                    start.append(len(idx))
                    idx.extend(atoms)
                    w.extend(masses[atoms] / masses[atoms].sum())
            return g.indices[np.asarray(idx, dtype=int)], np.asarray(start), np.asarray(w)
        if g.n_atoms % (M * N_p):
            raise ValueError(f"A group of {g.n_atoms} atoms cannot be divided into {M} chains of "
                             f"{N_p} monomers.")
        A = g.n_atoms // (M * N_p)                       # atoms per monomer
        local = np.arange(g.n_atoms).reshape(M, N_p, A)[:, (0, -1)].reshape(2 * M, A)
        if gr == "atoms":
            local = local[:, :1]                         # positions_end[:, :, 0] (:750)
            w = np.ones(2 * M)
        else:
            m = g.masses[local]
            w = (m / m.sum(axis=1, keepdims=True)).ravel()
        start = np.arange(2 * M) * local.shape[1]
        return g.indices[local.ravel()], start, w

    def _ends_of_block(self, block, sel):
        """float64[T, M, 2, 3] end positions from a block float[T, K, 3] of the selected atoms."""
        _, start, w = sel
        x = np.asarray(block, dtype=float)
        if len(w) == len(start):
            ends = x * w[None, :, None] if not np.all(w == 1.0) else x
        else:
            ends = np.add.reduceat(x * w[None, :, None], start, axis=1)
        return ends.reshape(x.shape[0], -1, 2, 3)

    def _initial_ends(self, g, gr, M, N_p):
        """Reference ends for unwrapping: chains made whole in the first frame and placed
        with their centre of mass inside the cell (reference :700-727)."""
        pos = np.array(g.positions, dtype=float)
        if self._internal and gr == "residues":
            # no bond topology in the array universes: consecutive atoms of a segment are bonded
            seg = g.segindices
            bonds = np.concatenate([np.stack([c[:-1], c[1:]], 1) for c in
                                    (np.flatnonzero(seg == s) for s in _ordered_unique(seg))])
        else:
            n = g.n_atoms // M
            bonds = np.array([(i * n + j, i * n + j + 1) for i in range(M) for j in range(n - 1)],
                             dtype=int).reshape(-1, 2)
        whole = unwrap_edge(positions=pos, bonds=bonds, dimensions=self._dimensions,
                            masses=g.masses)
        sel = self._end_selection(g, gr, M, N_p)
        lookup = np.full(self.universe.atoms.n_atoms, -1)
        lookup[g.indices] = np.arange(g.n_atoms)
        return self._ends_of_block(whole[lookup[sel[0]]][None], sel)[0]

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        self._n_frames_block = self.n_frames // self._n_blocks
        self._n_frames = self._n_blocks * self._n_frames_block
        extra = self.n_frames - self._n_frames
        if extra > 0:
            warnings.warn(f"The trajectory is not divisible into {self._n_blocks:,} blocks, so "
                          f"the last {extra:,} frame(s) will be discarded. To maximize "
                          "performance, set appropriate starting and ending frames in run() so "
                          "that the number of frames to be analyzed is divisible by the number "
                          "of blocks.")

        self._e2e = np.empty((self.n_frames, self._N_chains, 3))
        self._selections = [self._end_selection(g, gr, M, N_p) for g, gr, M, N_p in
                            zip(self._groups, self._groupings, self._n_chains, self._n_monomers)]
        if self._unwrap:
            if self._dimensions is None:
                raise ValueError("No system dimensions found: unwrapping is not possible.")
            st = self._sliced_trajectory
            self.universe.trajectory[st.frames[0] if hasattr(st, "frames") else (self.start or 0)]
            self._positions_end_old = np.empty((self._N_chains, 2, 3))
            for g, gr, s, M, N_p in zip(self._groups, self._groupings, self._slices,
                                        self._n_chains, self._n_monomers):
                self._positions_end_old[s] = self._initial_ends(g, gr, M, N_p)
            self._images = np.zeros((self._N_chains, 2, 3), dtype=int)
            self._thresholds = self._dimensions / 2

        step = self.step if self.step is not None else 1
        self.results.times = step * self._dt * np.arange(self._n_frames // self._n_blocks)
        self.results.acf = np.empty((self._n_groups, self._n_blocks, self._n_frames_block))
        self.results.units = {"results.times": "picosecond"}

    def _store(self, first, ends, s):
        """ends float64[n, M, 2, 3] of consecutive analysed frames -> e2e[first : first + n, s];
        with ``unwrap`` the image flags of every frame follow from the running sum of the
        boundary crossings (the frame-by-frame rule of topology.py:366-376)."""
        if self._unwrap:
            prev = np.concatenate((self._positions_end_old[s][None], ends[:-1]))
            dpos = ends - prev
            crossed = np.abs(dpos) >= self._thresholds
            images = self._images[s] - np.cumsum(np.where(crossed, np.sign(dpos), 0.0).astype(int),
                                                 axis=0)
            self._positions_end_old[s] = ends[-1]
            self._images[s] = images[-1]
            ends = ends + images * self._dimensions
        self._e2e[first:first + len(ends), s] = ends[:, :, 1] - ends[:, :, 0]

    def _single_frame(self) -> None:
        positions = self.universe.atoms.positions
        for sel, s in zip(self._selections, self._slices):
            self._store(self._frame_index, self._ends_of_block(positions[sel[0]][None], sel), s)

    def run(self, start=None, stop=None, step=None, frames=None, n_jobs: int = 1, verbose=None,
            **kwargs):
        traj = self._trajectory
        if not has_frame_blocks(traj):
            return super().run(start=start, stop=stop, step=step, frames=frames, n_jobs=n_jobs,
                               verbose=verbose, **kwargs)
        # trajectories with block access: the end monomers of ~256 MiB of frames at a time
        mine = self._batched_frames(start, stop, step, frames, shard=False)
        size = block_frames(self.universe.atoms.n_atoms, 1, 1 << 28)
        for first in range(0, len(mine), size):
            block = traj.frame_block(mine[first:first + size])
            for sel, s in zip(self._selections, self._slices):
                self._store(first, self._ends_of_block(block[:, sel[0]], sel), s)
        self._conclude()
        return self

    def _conclude(self) -> None:
        if self._unwrap:
            del self._positions_end_old, self._images, self._thresholds
        B, Tb = self._n_blocks, self._n_frames_block
        e2e = self._e2e[:self._n_frames]
        unit = e2e / np.linalg.norm(e2e, axis=-1, keepdims=True)            # (:776-777)
        if not self._fft:
            for i, (s, M) in enumerate(zip(self._slices, self._n_chains)):
                self.results.acf[i] = correlation_shift(unit[:, s].reshape(B, -1, M, 3),
                                                        average=True, vector=True)
            return
        rank, world = self._comm.rank, self._comm.world_size
        eng = _core.MsdEngine(Tb, B, self._n_groups, dev=self._device)
        try:
            for i, (s, M) in enumerate(zip(self._slices, self._n_chains)):
                lo, hi = shard_range(int(M), rank, world)
                if hi > lo:
                    eng.push(i, unit, s.start + lo, hi - lo, 0)
            if world > 1 and getattr(self._comm, "device_collectives", False):
                eng.allreduce(self._comm)
                acf = eng.result_acf()
            else:
                acf = eng.result_acf()
                if world > 1:
                    acf = self._comm.allreduce(acf, op="sum")
        finally:
            eng.close()
        # correlation_fft: normalise lag m by T_b - m, average over the chains (:209-224)
        weights = (Tb - np.arange(Tb)).astype(float)
        for i, M in enumerate(self._n_chains):
            self.results.acf[i] = acf[i] / weights / M

    def calculate_relaxation_time(self) -> None:
        """Stretched-exponential relaxation time of every (group, block) (reference :783-803)."""
        if "acf" not in self.results:
            raise RuntimeError("Call EndToEndVector.run() before "
                               "EndToEndVector.calculate_relaxation_time().")
        self.results.relaxation_times = np.empty((self._n_groups, self._n_blocks))
        self.results.units["results.relaxation_times"] = "picosecond"
        for i, g in enumerate(self.results.acf):
            for j, acf in enumerate(g):
                valid = np.where(acf >= 0)[0]
                self.results.relaxation_times[i, j] = calculate_relaxation_time(
                    self.results.times[valid], acf[valid])


class RouseModes(EngineFedAnalysis, _PolymerAnalysisBase):
    r"""
    Rouse mode amplitudes of polymer chains and their relaxation (no counterpart in the reference),

    .. math:: \mathbf X_p(t)=\frac1N\sum_{n=0}^{N-1}\mathbf r_n(t)\cos\frac{p\pi(n+\frac12)}{N},
              \qquad p=1,\dots,N-1,

    their mean squares :math:`\langle X_p^2\rangle`, the normalised autocorrelations
    :math:`C_p(t)=\langle\mathbf X_p(t)\cdot\mathbf X_p(0)\rangle/\langle X_p^2\rangle` averaged over the
    chains of each group, and a relaxation time :math:`\tau_p` per mode.

    Parameters
    ----------
    groups, groupings, n_chains, n_monomers : see ``_PolymerAnalysisBase``; a group holds
        ``n_chains * n_monomers`` monomers, chain after chain (checks as in ``Gyradius``)
    modes : int or sequence of distinct ints, keyword-only — ``P`` means :math:`p=1,\dots,P`; every
        :math:`p` must satisfy :math:`1\le p\le\min_g N_g-1`
    n_blocks : int, keyword-only — blocks the trajectory is split into
    dt : float, keyword-only, optional — time between frames (ps)
    fft : bool, keyword-only — FFT-based ACF on the GPU (``False``: direct sliding windows, NumPy, on
        amplitudes copied from the device)
    unwrap : bool, keyword-only — follow the monomers across the periodic boundaries from frame to
        frame, starting from chains made whole in the first analysed frame
    comm, device : keyword-only (extension) — every rank projects all frames; the chains of each
        (group, mode) shard across ranks in the correlation, one all-reduce of the accumulators

    Results: ``results.modes`` ``[P]``, ``results.times`` ``[T_b]`` (ps), ``results.amplitudes``
    ``[N_g, N_b, P]`` (:math:`\langle X_p^2\rangle` in Å², the lag-0 value of the ACF after the
    :math:`M(T_b-m)` normalisation), ``results.acf`` ``[N_g, N_b, P, T_b]`` (:math:`C_p(t)`, 1 at lag 0),
    ``results.units``; ``results.relaxation_times`` ``[N_g, N_b, P]`` after ``calculate_relaxation_times()``.

    Where the work goes: the projection engine (``mdx_rouse_*``) forms the float64 monomer centres, follows
    them across the boundaries and computes every :math:`\mathbf X_p` of every chain and frame, in HBM; with
    ``fft=True`` the correlation engine of ``Onsager`` reads them there (``mdx_msd_push_device``), one contiguous
    range of series per (group, mode), and the amplitudes never visit the host.

    What it restricts:

    * :math:`p=0` (the centre of geometry, whose observable is an MSD, not an ACF), :math:`p\ge N`, repeated
      modes and ``n_groups * len(modes) > 4096`` (the correlation engine's groups) raise ``ValueError`` at
      construction.
    * The modes are not weighted by mass (the usual definition); with ``"residues"`` the :math:`\mathbf r_n` are
      the monomers' centres of mass.  The weights ``cos(pi p (n + 1/2) / N) / N`` are formed on the host in
      float64; the device multiplies and adds.
    * ``unwrap=True`` with more than one rank, or without box dimensions, and groups whose size does not match
      ``n_chains * n_monomers`` raise ``ValueError`` at construction, as in ``Gyradius``; the chains of the first
      analysed frame are made whole along bonds between consecutive monomers.
    * Frames beyond ``n_blocks * (n_frames // n_blocks)`` are discarded with a warning, as in
      ``EndToEndVector``.  Frames do not shard across ranks.
    * Cross-correlations between different modes and the MSD of :math:`p=0` are not computed.
    * There is no CPU fallback for the projection: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    _MAX_SERIES_GROUPS = 4096          # groups of the correlation engine (mdx_msd_create)

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms", n_chains=None,
                 n_monomers=None, *, modes=5, n_blocks: int = 1, dt=None, fft: bool = True,
                 unwrap: bool = False, verbose: bool = True, **kwargs) -> None:
        kwargs.pop("parallel", None)
        super().__init__(groups, groupings, n_chains, n_monomers, unwrap=unwrap,
                         verbose=verbose, **kwargs)
        self._setup_points()
        if isinstance(modes, (int, np.integer)):
            modes = np.arange(1, int(modes) + 1)
        else:
            given = np.asarray(modes)
            if given.ndim != 1 or (given.size and not np.issubdtype(given.dtype, np.integer)):
                raise ValueError("'modes' must be an int or a sequence of ints.")
            modes = given.astype(int)
        p_max = int(self._n_monomers.min()) - 1
        if len(modes) == 0 or modes.min() < 1 or modes.max() > p_max:
            raise ValueError(f"Every mode p must satisfy 1 <= p <= n_monomers - 1 = {p_max}; p = 0 is the "
                             "centre of geometry, whose observable is a mean squared displacement.")
        if len(np.unique(modes)) != len(modes):
            raise ValueError("The modes must be distinct.")
        if self._n_groups * len(modes) > self._MAX_SERIES_GROUPS:
            raise ValueError(f"n_groups * len(modes) = {self._n_groups * len(modes)} exceeds the "
                             f"{self._MAX_SERIES_GROUPS} groups of the correlation engine.")
        self._modes = modes
        self._n_blocks = n_blocks
        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._fft = fft

    def _weights(self):
        """One float64 array ``[P, N_p]`` per group: ``cos(pi p (n + 1/2) / N_p) / N_p``."""
        return [np.stack([np.cos(np.pi * p * (np.arange(N_p) + 0.5) / N_p) / N_p for p in self._modes])
                for N_p in self._n_monomers]

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        self._n_frames_block = self.n_frames // self._n_blocks
        self._n_frames = self._n_blocks * self._n_frames_block
        extra = self.n_frames - self._n_frames
        if extra > 0:
            warnings.warn(f"The trajectory is not divisible into {self._n_blocks:,} blocks, so "
                          f"the last {extra:,} frame(s) will be discarded. To maximize "
                          "performance, set appropriate starting and ending frames in run() so "
                          "that the number of frames to be analyzed is divisible by the number "
                          "of blocks.")
        P = len(self._modes)
        step = self.step if self.step is not None else 1
        self.results.modes = self._modes.copy()
        self.results.times = step * self._dt * np.arange(self._n_frames_block)
        self.results.amplitudes = np.empty((self._n_groups, self._n_blocks, P))
        self.results.acf = np.empty((self._n_groups, self._n_blocks, P, self._n_frames_block))
        self.results.units = {"results.times": "picosecond", "results.amplitudes": "angstrom^2"}

        # every rank projects all frames: the chains shard in the correlation
        sels = [self._selection(g, gr, int(N)) for g, gr, N in zip(self._groups, self._groupings, self._Ns)]
        self._feed_points(_core.ChainProjectionEngine(self._n_chains, self._n_monomers, self._weights(),
                                                      dev=self._device), sels)
        self._engine.reserve(self.n_frames)

    def _conclude(self) -> None:
        self._batch.flush()
        B, Tb, P = self._n_blocks, self._n_frames_block, len(self._modes)
        series0 = np.concatenate(([0], np.cumsum(P * self._n_chains)))
        try:
            if not self._fft:
                X = self._engine.result()[:self._n_frames]                   # [T, S, 3]
                for g, M in enumerate(self._n_chains):
                    for k in range(P):
                        lo = series0[g] + k * M
                        raw = correlation_shift(X[:, lo:lo + M].reshape(B, Tb, M, 3), average=True,
                                                vector=True)
                        self.results.amplitudes[g, :, k] = raw[:, 0]
                        self.results.acf[g, :, k] = raw / raw[:, :1]
                return
            rank, world = self._comm.rank, self._comm.world_size
            d_amp, n_seen, S = self._engine.device_result()
            if n_seen < self._n_frames:
                raise RuntimeError(f"The projection engine holds {n_seen} frames, {self._n_frames} were "
                                   "expected.")
            eng = _core.MsdEngine(Tb, B, self._n_groups * P, dev=self._device)
            try:
                # the chains of a (group, mode) are a contiguous range of series: read where they lie
                for g, M in enumerate(self._n_chains):
                    lo, hi = shard_range(int(M), rank, world)
                    if hi > lo:
                        for k in range(P):
                            eng.push_device(g * P + k, d_amp, S, int(series0[g] + k * M + lo), hi - lo, 0)
                if world > 1 and getattr(self._comm, "device_collectives", False):
                    eng.allreduce(self._comm)
                    acf = eng.result_acf()
                else:
                    acf = eng.result_acf()
                    if world > 1:
                        acf = self._comm.allreduce(acf, op="sum")
            finally:
                eng.close()
        finally:
            self._engine.close()
        # correlation_fft: normalise lag m by T_b - m, average over the chains
        weights = (Tb - np.arange(Tb)).astype(float)
        acf = np.asarray(acf).reshape(self._n_groups, P, B, Tb)
        for g, M in enumerate(self._n_chains):
            raw = np.swapaxes(acf[g], 0, 1) / weights / M                   # [B, P, T_b]
            self.results.amplitudes[g] = raw[..., 0]
            self.results.acf[g] = raw / raw[..., :1]

    def calculate_relaxation_times(self) -> None:
        """Stretched-exponential relaxation time of every (group, block, mode), fitted to the non-negative
        part of the ACF as in ``EndToEndVector.calculate_relaxation_time``."""
        if "acf" not in self.results:
            raise RuntimeError("Call RouseModes.run() before RouseModes.calculate_relaxation_times().")
        self.results.relaxation_times = np.empty(self.results.acf.shape[:3])
        self.results.units["results.relaxation_times"] = "picosecond"
        for idx in np.ndindex(*self.results.acf.shape[:3]):
            acf = self.results.acf[idx]
            valid = np.where(acf >= 0)[0]
            self.results.relaxation_times[idx] = calculate_relaxation_time(self.results.times[valid],
                                                                           acf[valid])


def calculate_characteristic_ratio(r2: np.ndarray) -> np.ndarray:
    r"""
    :math:`C(s)=\langle R^2(s)\rangle/(s\,\langle R^2(1)\rangle)` from the mean-square internal distances
    ``r2[..., s - 1]``, :math:`s=1,\dots,N-1`; its plateau is the characteristic ratio :math:`C_\infty`.
    """
    r2 = np.asarray(r2, dtype=float)
    return r2 / (np.arange(1, r2.shape[-1] + 1) * r2[..., :1])


def calculate_persistence_length(cosines: np.ndarray, bond_length: float, n_fit: int = None) -> float:
    r"""
    Persistence length :math:`l_\mathrm p=-b/m` from the bond-orientation correlation ``cosines[s]``,
    :math:`s=0,1,\dots`, with :math:`m` the least-squares slope through the origin of :math:`\ln C(s)` against
    :math:`s` over :math:`s=0,\dots,` ``n_fit`` (:math:`C(s)=e^{-sb/l_\mathrm p}`).  ``n_fit`` defaults to the last
    :math:`s` before :math:`C` first falls to :math:`1/e` or below, at least 1.  A correlation that is not positive
    inside the window raises ``ValueError``.
    """
    c = np.asarray(cosines, dtype=float)
    if c.ndim != 1 or len(c) < 2:
        raise ValueError("'cosines' must hold C(s) for s = 0, 1, ...: at least two separations.")
    if n_fit is None:
        below = np.flatnonzero(c <= np.exp(-1.0))
        n_fit = max(1, (below[0] if len(below) else len(c)) - 1)
    n_fit = int(n_fit)
    if not 1 <= n_fit < len(c):
        raise ValueError(f"'n_fit' must satisfy 1 <= n_fit <= {len(c) - 1}.")
    window = c[:n_fit + 1]
    if np.any(window <= 0) or not np.all(np.isfinite(window)):
        raise ValueError("The bond-orientation correlation must be positive inside the fit window.")
    s = np.arange(n_fit + 1, dtype=float)
    slope = (s * np.log(window)).sum() / (s * s).sum()
    return np.inf if slope == 0 else -bond_length / slope


class InternalDistances(EngineFedAnalysis, _PolymerAnalysisBase):
    r"""
    Mean-square internal distances and bond-orientation correlations of polymer chains (no counterpart in the
    reference),

    .. math:: \langle R^2(s)\rangle=\frac{1}{M(N-s)}\sum_c\sum_{i=0}^{N-1-s}|\mathbf r_{c,i+s}-\mathbf r_{c,i}|^2,
              \qquad C(s)=\frac{1}{M(N-1-s)}\sum_c\sum_{i=0}^{N-2-s}\hat{\mathbf b}_{c,i}\cdot\hat{\mathbf b}_{c,i+s},

    with :math:`\hat{\mathbf b}_i` the unit vector of the bond from monomer :math:`i` to :math:`i+1`, per frame and
    group.  :math:`\langle R^2(s)\rangle/s` against :math:`s` shows whether a melt is equilibrated; from the two
    follow the characteristic ratio and the persistence length.

    Parameters
    ----------
    groups, groupings, n_chains, n_monomers : see ``_PolymerAnalysisBase``; a group holds
        ``n_chains * n_monomers`` monomers, chain after chain (checks as in ``Gyradius``), ``n_monomers >= 2``
    unwrap : bool, keyword-only — follow the monomers across the periodic boundaries from frame to frame,
        starting from chains made whole in the first analysed frame (one rank only)
    whole : bool, keyword-only — make every chain whole in every frame by itself, on the device: bond after
        bond from the chain's first monomer, each bond by its minimum image.  **Every bond must be shorter than half
        the shortest box length.**  Needs a constant orthorhombic box; the frames still shard across ranks.
        Excludes ``unwrap``.
    dimensions : array-like (3,), keyword-only, optional — box lengths (Å) for ``whole``; default: the universe's
    parallel : bool, keyword-only — accepted; the serial result layout is returned
    comm, device : keyword-only (extension) — frames shard across ranks, one all-reduce at the end

    Results, one entry per group (the chain lengths differ between groups): ``results.separations[g]`` ``[N-1]``
    (:math:`s=1,\dots,N-1`), ``results.squared_distances[g]`` ``[N_t, N-1]`` (Å², per frame),
    ``results.bond_cosines[g]`` ``[N_t, N-1]`` (:math:`s=0,\dots,N-2`), ``results.mean_squared_distances[g]`` and
    ``results.mean_bond_cosines[g]`` ``[N-1]`` (means over the frames), ``results.units``;
    ``results.characteristic_ratio[g]`` ``[N-1]`` after ``calculate_characteristic_ratio()`` and
    ``results.persistence_length[g]`` (Å) after ``calculate_persistence_length()``.

    Where the work goes: the internal-distance engine (``mdx_msid_*``) forms the float64 monomer centres, makes
    the chains whole (or follows them), and sums every pair term of every chain in float64 out of LDS; the host
    sees ``2 (N - 1)`` numbers per frame and group.  With ``"residues"`` the points are the monomers' centres of
    mass; a bond of no length has the unit vector 0.  There is no CPU fallback: without a HIP device ``run()``
    raises ``RuntimeError``.
    """

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms", n_chains=None,
                 n_monomers=None, *, unwrap: bool = False, whole: bool = False, dimensions=None,
                 parallel: bool = False, verbose: bool = True, **kwargs) -> None:
        super().__init__(groups, groupings, n_chains, n_monomers, unwrap=unwrap, parallel=parallel,
                         verbose=verbose, **kwargs)
        if unwrap and whole:
            raise ValueError("'unwrap' and 'whole' cannot be combined: either follow the monomers from frame to "
                             "frame or make the chains whole in every frame.")
        self._setup_points()
        for i, N_p in enumerate(self._n_monomers):
            if N_p < 2:
                raise ValueError(f"Group {i} has chains of {N_p} monomer(s): internal distances need n_monomers "
                                 ">= 2.")
        self._whole = bool(whole)
        self._drop_axis = None
        self._whole_dimensions = self._box_lengths(dimensions, 0.0, "whole") if whole else None

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # (unwrap, which makes the frames sequential, runs on one rank)

    def _prepare(self) -> None:
        self.results.separations = [np.arange(1, N_p) for N_p in self._n_monomers]
        self.results.units = {"results.squared_distances": "angstrom^2",
                              "results.mean_squared_distances": "angstrom^2"}
        sels = [self._selection(g, gr, int(N)) for g, gr, N in zip(self._groups, self._groupings, self._Ns)]
        engine = _core.InternalDistanceEngine(self._n_chains, self._n_monomers, dev=self._device)
        if self._whole:
            engine.set_whole(self._whole_dimensions)
        self._feed_points(engine, sels)
        lo, hi = self._frames_mine
        self._engine.reserve(hi - lo)

    def _conclude(self) -> None:
        self._batch.flush()
        per_group = self._engine.result()                   # [frames of this rank, 2, N - 1] per group
        self._engine.close()
        rows = self._gather_frame_rows(np.concatenate([r.reshape(len(r), -1) for r in per_group], axis=1))
        row0 = np.concatenate(([0], np.cumsum(2 * (self._n_monomers - 1))))
        both = [rows[:, lo:lo + 2 * (N_p - 1)].reshape(len(rows), 2, N_p - 1)
                for lo, N_p in zip(row0[:-1], self._n_monomers)]
        self.results.squared_distances = [b[:, 0].copy() for b in both]
        self.results.bond_cosines = [b[:, 1].copy() for b in both]
        self.results.mean_squared_distances = [r2.mean(axis=0) for r2 in self.results.squared_distances]
        self.results.mean_bond_cosines = [c.mean(axis=0) for c in self.results.bond_cosines]

    def calculate_characteristic_ratio(self) -> None:
        r""":math:`\langle R^2(s)\rangle/(s\langle R^2(1)\rangle)` of every group, from the means over the frames."""
        if "mean_squared_distances" not in self.results:
            raise RuntimeError("Call InternalDistances.run() before "
                               "InternalDistances.calculate_characteristic_ratio().")
        self.results.characteristic_ratio = [calculate_characteristic_ratio(r2)
                                             for r2 in self.results.mean_squared_distances]

    def calculate_persistence_length(self, n_fit: int = None) -> None:
        r"""Persistence length (Å) of every group from the mean bond-orientation correlation, with the bond length
        :math:`b=\sqrt{\langle R^2(1)\rangle}` (``calculate_persistence_length``)."""
        if "mean_bond_cosines" not in self.results:
            raise RuntimeError("Call InternalDistances.run() before "
                               "InternalDistances.calculate_persistence_length().")
        self.results.persistence_length = [
            calculate_persistence_length(c, np.sqrt(r2[0]), n_fit)
            for c, r2 in zip(self.results.mean_bond_cosines, self.results.mean_squared_distances)]
        self.results.units["results.persistence_length"] = "angstrom"


class SingleChainStructureFactor(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Single-chain structure factor of a homopolymer (reference :805-1130):

    .. math:: S_\mathrm{sc}(\mathbf q)=\frac{1}{MN_\mathrm p}\sum_{m=1}^M\left\langle
              \left|\sum_{j\in m}e^{i\mathbf q\cdot\mathbf r_j}\right|^2\right\rangle

    averaged over the wavevectors of equal wavenumber.  In the Guinier regime
    :math:`S_\mathrm{sc}(q)\approx N_\mathrm p(1-(qR_g)^2/3)` gives the radius of gyration; the
    slope :math:`s` of the log-log plot in the intermediate regime gives the scaling exponent
    :math:`\nu=-1/s`.

    Parameters (reference :934-938)
    ----------
    group : AtomGroup — the chains, all of one length
    grouping : {"atoms", "residues"}
    n_points : int, default 32 — wavevectors ``2 pi n / L``, ``n = 0 ... n_points - 1`` per axis
    n_chains, n_monomers : int, keyword-only, optional — read from the topology (chains =
        segments) when either is missing
    dimensions : array-like (3,), keyword-only, optional — box lengths in Å
    unwrap : bool, keyword-only — accepted; it changes nothing (see below)
    parallel : bool, keyword-only — accepted and ignored
    comm, device : keyword-only (extension) — frames shard across ranks, one all-reduce at the end

    Results: ``results.wavenumbers`` ``[N_q]`` (Å⁻¹), ``results.scsf`` ``[N_q]``, ``results.units``.

    Where this differs from the reference:

    * ``unwrap`` computes on the coordinates as given, for both values.  Image shifts are whole
      multiples of the box lengths the wavevectors are built from, so every phase moves by a
      multiple of :math:`2\pi` and the result is the same; the reference applies the shifts in
      float32 (topology.py:376), so its ``unwrap=True`` result only loses digits.
    * ``"residues"``: the monomer centres of mass are float32, formed on the device (as in
      ``StructureFactor``); the reference keeps them in float64.
    * ``"residues"`` read from the topology: one chain per segment and ``n_monomers`` = residues per
      chain.  The reference sets it to atoms per chain, which only works with one atom per residue;
      wherever the reference runs, both agree.
    * A point count other than ``n_chains * n_monomers`` and segments of unequal length raise
      ``ValueError`` before any work (the reference fails in a reshape).
    """

    def __init__(self, group, grouping: str = "atoms", n_points: int = 32, *, n_chains: int = None,
                 n_monomers: int = None, dimensions=None, unwrap: bool = False,
                 parallel: bool = False, verbose: bool = True, **kwargs) -> None:
        self._group = group
        self.universe = group.universe
        super().__init__(self.universe.trajectory, parallel, verbose, **kwargs)

        if dimensions is not None:
            if len(dimensions) != 3:
                raise ValueError("'dimensions' must have length 3.")
            self._dimensions = np.asarray(strip_unit(dimensions, "angstrom")[0], dtype=float)
        elif self.universe.dimensions is not None:
            self._dimensions = np.array(self.universe.dimensions[:3], dtype=float)
        else:
            raise ValueError("No system dimensions found or provided.")

        if grouping not in _GROUPINGS:
            raise ValueError(f"Invalid grouping '{grouping}'. Valid values: "
                             f"{', '.join(sorted(_GROUPINGS))}.")
        self._grouping = grouping

        if n_chains is None or n_monomers is None:
            self._internal = True
            seg = np.asarray(group.segindices)
            _, seg_sizes = np.unique(seg, return_counts=True)
            self._n_chains = len(seg_sizes)
            if grouping == "residues":
                _, first = np.unique(np.asarray(group.resindices), return_index=True)
                _, per_seg = np.unique(seg[first], return_counts=True)      # residues per segment
                if np.any(per_seg != per_seg[0]):
                    raise ValueError("All segments must hold the same number of residues.")
                self._n_monomers = int(per_seg[0])
            else:
                if np.any(seg_sizes != seg_sizes[0]):
                    raise ValueError("All segments must hold the same number of atoms.")
                self._n_monomers = group.n_atoms // self._n_chains
        else:
            self._internal = False
            if not isinstance(n_chains, (int, np.integer)):
                raise ValueError("The number of chains must be specified when the universe does "
                                 "not contain segment information.")
            if not isinstance(n_monomers, (int, np.integer)):
                raise ValueError("The number of monomers per chain must be specified when the "
                                 "universe does not contain segment information.")
            self._n_chains, self._n_monomers = int(n_chains), int(n_monomers)
        self._N = self._n_chains * self._n_monomers
        n_have = group.n_atoms if grouping == "atoms" or not self._internal else \
            len(np.unique(np.asarray(group.resindices)))
        if self._N <= 0 or (n_have % self._N if grouping == "residues" and not self._internal
                            else n_have != self._N):
            what = "atoms" if grouping == "atoms" or not self._internal else "residues"
            raise ValueError(f"The group holds {n_have} {what}, which do not form n_chains * "
                             f"n_monomers = {self._n_chains} * {self._n_monomers} = {self._N} "
                             f"monomers.")

        # reference :1016-1023; numpy.meshgrid's default 'xy' indexing fixes the row order
        self._n_points = n_points
        self._wavevectors = np.stack(
            np.meshgrid(*[2 * np.pi * np.arange(n_points) / L for L in self._dimensions]),
            -1).reshape(-1, 3)
        self._wavenumbers = np.linalg.norm(self._wavevectors, axis=1)
        self._unwrap = unwrap
        self._verbose = verbose

    # ------------------------------------------------------------------ points

    def _selection(self):
        """(particle indices in chain order, monomer offsets or None, masses or None)."""
        g = self._group
        idx = np.asarray(g.indices)
        if self._grouping == "atoms":
            return idx, None, None
        masses = np.asarray(g.masses, dtype=np.float64)
        if not self._internal:
            # a monomer is n_atoms / (n_chains n_monomers) consecutive atoms
            return idx, np.arange(self._N + 1, dtype=np.int64) * (g.n_atoms // self._N), masses
        # residues of the topology, molecule by molecule; a chain is a segment
        _, inverse = np.unique(np.asarray(g.resindices), return_inverse=True)
        order = np.argsort(inverse, kind="stable")
        offsets = np.concatenate(([0], np.cumsum(np.bincount(inverse)))).astype(np.int64)
        seg = np.asarray(g.segindices)[order][offsets[:-1]].reshape(self._n_chains, self._n_monomers)
        if np.any(seg != seg[:, :1]) or len(np.unique(seg[:, 0])) != self._n_chains:
            raise ValueError("The residues of every segment must be consecutive.")
        return idx[order], offsets, masses[order]

    def _points(self, sel):
        """Positions float[N, 3] of the points in the current frame (per-frame path)."""
        idx, off, m = sel
        pos = np.asarray(self.universe.trajectory.ts.positions, dtype=float)[idx]
        if off is None:
            return pos
        msum = np.add.reduceat(m, off[:-1])
        return np.add.reduceat(pos * m[:, None], off[:-1], axis=0) / msum[:, None]

    # ------------------------------------------------------------------ protocol

    _shard_frames = True
    _device_index = False       # SqEngine.accumulate_device takes every particle in order

    def _prepare(self) -> None:
        self.results.wavenumbers = np.unique(self._wavenumbers.round(11))
        self.results.units = {"results.wavenumbers": "angstrom^-1"}
        self._sel = self._selection()
        engine = _core.SqEngine(self._wavevectors, [self._N], ((None, None),), dev=self._device)
        engine.set_chains(self._n_monomers)
        self._feed_engine(engine, self._sel[0], rows=int(self._N))

    def _frame_rows(self):
        return self._points(self._sel)

    # the batched route forms the monomer centres of mass on the device, which then cannot read the frames in HBM
    def _before_blocks(self) -> None:
        _, offsets, masses = self._sel
        if offsets is not None:
            self._engine.set_grouping(offsets, masses)
            self._hbm = False

    def _conclude(self) -> None:
        from .structure import _mean_over_equal_wavenumbers
        self._batch.flush()
        if self._comm.world_size > 1 and getattr(self._comm, "device_collectives", False):
            self._engine.allreduce(self._comm)
            acc = self._engine.result()[0]
        else:
            acc = self._comm.allreduce(self._engine.result()[0])
        self._engine.close()
        scsf = acc / (self._n_chains * self._n_monomers * self.n_frames)
        self.results.scsf = _mean_over_equal_wavenumbers(scsf, self._wavenumbers,
                                                         self.results.wavenumbers)


def _ordered_unique(ids):
    """Distinct values in order of first appearance."""
    _, first = np.unique(ids, return_index=True)
    return np.asarray(ids)[np.sort(first)]

