"""
Angular distributions: ``AngularDistribution`` — the distribution of the angle j–i–k between two ligands j, k in the
first shell of a centre i (tetrahedral against octahedral cation shells, mono- against bidentate anion binding), per
pair of ligand species, and the distribution of the per-species coordination numbers that goes with it.

Whole blocks of frames go to the angle engine (``mdx_ang_*``), which tests every (centre, ligand) pair of a frame in
float64 (minimum image, ``r2 <= cutoff[g] ** 2`` for a ligand of group ``g``), keeps the neighbours as capped
per-centre lists in HBM, and bins ``c = dot / sqrt(r2_ij * r2_ik)`` of every pair of neighbours of a centre against a
decreasing table of thresholds with integer atomics (csrc/mdx_angle_device.hpp).  A frame needs no other frame, so the
frames shard across ranks.
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, parse_drop_axis, zero_dims


class AngularDistribution(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Distribution of the angle :math:`\theta_{jik}` at a centre :math:`i` between two of its neighbours :math:`j\ne k`:
    a ligand of group :math:`g` is a neighbour where its minimum-image distance from the centre is at most
    ``cutoff[g]``, and with :math:`\mathbf w` the minimum-image vectors from the centre

    .. math:: \cos\theta_{jik}=\frac{\mathbf w_{ij}\cdot\mathbf w_{ik}}{\sqrt{r_{ij}^2\,r_{ik}^2}}

    is counted, for every analysed frame, centre and unordered pair :math:`\{j,k\}`, in the bin ``b`` with
    ``thresholds[b + 1] < cos θ <= thresholds[b]`` of a decreasing table of thresholds of the cosine (the first bin
    also takes what rounds above 1, the last one is closed at θ = 180°), separately for every unordered pair of
    ligand groups.

    Parameters
    ----------
    center : AtomGroup — the centres
    ligands : AtomGroup or sequence of at most 4 AtomGroups — the ligand species.  A single group of the very atoms
        of ``center`` in the same order: the neighbours of a centre are the other centres.  Otherwise ``center`` and
        all ligand groups must be disjoint; none may be empty
    cutoff : float or one value per ligand group — the radius of the first shell (Å), positive and finite; the
        largest may not exceed half the shortest box length that takes part
    n_bins : int, keyword-only — bins of the distribution
    bins : {"angle", "cosine"}, keyword-only — bins of equal width in θ (``thresholds = cos(deg2rad(linspace(0, 180,
        n_bins + 1)))``) or in cos θ (``thresholds = linspace(1, -1, n_bins + 1)``)
    max_neighbors : int, keyword-only — the neighbours of all groups together a centre may have in one frame
        (1 ... 64).  A frame with more raises ``ValueError`` at the end of ``run()``: nothing is truncated silently
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    verbose : bool
    device : keyword-only — the HIP device
    comm : communicator, keyword-only — the frames shard across ranks

    Results
    -------
    With ``G`` ligand groups, ``P = G (G + 1) / 2`` unordered pairs of them, ``F`` analysed frames and ``n0`` centres:
    ``results.edges`` ``[n_bins + 1]`` and ``results.bins`` ``[n_bins]`` (the bin centres), in degrees, or in cos θ
    (decreasing) with ``bins="cosine"``; ``results.pairs`` — the list of ``(a, b)``, ``a <= b``, pair ``p`` at
    ``a * G - a * (a - 1) / 2 + (b - a)``; ``results.counts`` ``[P, n_bins]``, ``results.degenerate`` ``[P]`` (the
    triplets with a ligand on its centre, which have no angle) and ``results.coordination_counts`` ``[G, m_max + 1]``
    (the (frame, centre) cases with exactly ``m`` neighbours of group ``g``, trimmed to the largest ``m`` seen), all
    int64; ``results.distribution`` — ``counts / (counts.sum(-1) * bin width)``, rows that integrate to 1, a row of
    NaN where a pair has no triplet; ``results.coordination_distribution`` — ``coordination_counts / (F * n0)``;
    ``results.coordination_number`` ``[G]`` — its mean; and ``results.units``.

    Limits: a constant orthorhombic box, coordinates as given, no molecule centres, every (centre, ligand) pair
    evaluated (no cell list), no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, center, ligands, cutoff, *, n_bins: int = 180, bins: str = "angle", max_neighbors: int = 32,
                 dimensions=None, drop_axis=None, verbose: bool = True, **kwargs) -> None:
        self._ligands = [ligands] if hasattr(ligands, "indices") else list(ligands)
        if not 1 <= len(self._ligands) <= _core.AngleEngine.MAX_SPECIES:
            raise ValueError(f"'ligands' must hold between 1 and {_core.AngleEngine.MAX_SPECIES} groups.")
        self.universe = center.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        G = len(self._ligands)

        i0 = np.asarray(center.indices)
        indices = [np.asarray(g.indices) for g in self._ligands]
        self._same = G == 1 and np.array_equal(i0, indices[0])
        if len(i0) < 1 or any(len(i) < 1 for i in indices):
            raise ValueError("The groups must hold at least one atom.")
        self._index = i0 if self._same else np.concatenate((i0, *indices))
        if len(np.unique(self._index)) != len(self._index):
            raise ValueError("'center' and 'ligands' share some atoms: they must be disjoint, or the very same atoms "
                             "in the same order.")
        self._n_centers = len(i0)
        self._ligand_sizes = np.array([len(i) for i in indices], dtype=np.int64)

        cut = np.asarray(strip_unit(cutoff, "angstrom")[0], dtype=float)
        if cut.ndim == 0:
            cut = np.full(G, float(cut))
        if cut.shape != (G,):
            raise ValueError(f"'cutoff' must be a number or {G} values, one per ligand group.")
        if not (np.all(np.isfinite(cut)) and np.all(cut > 0)):
            raise ValueError("'cutoff' must be positive and finite.")
        self._cutoff = cut

        self._n_bins = int(n_bins)
        if self._n_bins < 1:
            raise ValueError("'n_bins' must be at least 1.")
        if bins == "angle":
            self._edges = np.linspace(0.0, 180.0, self._n_bins + 1)
            self._thresholds = np.cos(np.deg2rad(self._edges))
        elif bins == "cosine":
            self._edges = self._thresholds = np.linspace(1.0, -1.0, self._n_bins + 1)
        else:
            raise ValueError("Invalid value passed to 'bins'. The valid values are 'angle' and 'cosine'.")
        self._bins = bins
        self._max_neighbors = int(max_neighbors)
        if not 1 <= self._max_neighbors <= _core.AngleEngine.MAX_NEIGHBORS:
            raise ValueError(f"'max_neighbors' must lie in [1, {_core.AngleEngine.MAX_NEIGHBORS}].")

        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, self._cutoff.max(), "cutoff")
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # a frame needs no other frame

    def _prepare(self) -> None:
        unit = "degree" if self._bins == "angle" else "dimensionless"
        self.results.units = {"results.edges": unit, "results.bins": unit}
        _lib.require_device(self._device)
        self._feed_engine(_core.AngleEngine(
            self._n_centers, self._ligand_sizes, self._cutoff, self._thresholds, self._dimensions, same=self._same,
            zero_dims=zero_dims(self._drop_axis), max_neighbors=self._max_neighbors, dev=self._device), self._index)

    def _conclude(self) -> None:
        try:
            self._batch.flush()
            got = self._engine.result()
        finally:
            self._engine.close()
        counts, degenerate, coordination = got["counts"], got["degenerate"], got["coordination"]
        if self._comm.world_size > 1:
            counts = np.asarray(self._comm.allreduce(counts, op="sum"))
            degenerate = np.asarray(self._comm.allreduce(degenerate, op="sum"))
            coordination = np.asarray(self._comm.allreduce(coordination, op="sum"))
        G, F, n0 = len(self._ligands), self.n_frames, self._n_centers
        seen = np.flatnonzero(coordination.any(axis=0))
        m_max = int(seen[-1]) if len(seen) else 0
        res = self.results
        res.edges = self._edges
        res.bins = (self._edges[:-1] + self._edges[1:]) / 2
        res.pairs = [(a, b) for a in range(G) for b in range(a, G)]
        res.counts = counts
        res.degenerate = degenerate
        res.coordination_counts = coordination[:, :m_max + 1]
        total = counts.sum(axis=-1).astype(float)
        total[total == 0] = np.nan
        res.distribution = counts / (total[:, None] * np.abs(np.diff(self._edges)))
        res.coordination_distribution = res.coordination_counts / ((F * n0) if F else np.nan)
        res.coordination_number = res.coordination_distribution @ np.arange(m_max + 1)
