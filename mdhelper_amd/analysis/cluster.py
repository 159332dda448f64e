"""
Ion clusters: ``Clusters`` — per analysed frame the connected components of the contact graph of one or several
groups of atoms, and from them the cluster-size distribution, the per-species membership by cluster size (free ions,
pairs, larger aggregates) and per-frame cluster counts.

The reference package answers this on the host: the user builds a contact graph frame by frame and hands it to the
recursive ``find_connected_nodes`` of ``algorithm/utility.py`` (kept here as an iterative host helper).  Here whole
blocks of frames go to the cluster engine (``mdx_clu_*``), which tests every pair of a frame in float64 (minimum
image, ``r2 <= cutoff[a][b] ** 2`` for the species ``a``, ``b`` of the pair), keeps the bonds as capped per-atom
lists in HBM, labels the connected components on the device from the lists and tallies the labels with integer
atomics (csrc/mdx_cluster_device.hpp).  A frame needs no other frame, so the frames shard across ranks.
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, parse_drop_axis, zero_dims


class Clusters(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Connected components of the contact graph of ``groups``: two atoms are bonded in a frame where their
    minimum-image distance is at most the cutoff of their two groups, and a cluster is a set of atoms connected by
    bonds.  With :math:`N_s(f)` the clusters of :math:`s` atoms in frame :math:`f`,

    .. math:: P(s)=\frac{\sum_f N_s(f)}{\sum_f\sum_{s'}N_{s'}(f)},\qquad
              W(s)=\frac{s\sum_f N_s(f)}{F\,n}

    are the number and the weight distribution of the cluster sizes: ``W(1)`` is the fraction of free ions, ``W(2)``
    that of ions in pairs.

    Parameters
    ----------
    groups : AtomGroup or sequence of at most 8 AtomGroups — the species; the groups must be disjoint and none may
        be empty
    cutoff : float or array-like ``(G, G)`` — the bond distance (Å): one value for every pair of atoms, or a
        symmetric table by species with non-negative entries, at least one of them positive.  A 0 means that pair of
        species makes no bond: ``[[0, 3.5], [3.5, 0]]`` counts cation–anion contacts only.  The largest entry may not
        exceed half the shortest box length that takes part
    max_neighbors : int, keyword-only — the bonds an atom may have in one frame (1 ... 64).  A frame with more raises
        ``ValueError`` at the end of ``run()``: nothing is truncated silently
    store_labels : bool, keyword-only — keep ``results.labels``
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    verbose : bool
    device : keyword-only — the HIP device
    comm : communicator, keyword-only — the frames shard across ranks

    Results
    -------
    With ``s_max`` the largest cluster seen, ``F`` the analysed frames, ``n`` the atoms and ``N_g`` those of group
    ``g``: ``results.sizes`` — ``arange(s_max + 1)`` — ``results.size_counts`` ``[s_max + 1]`` (int64, clusters of
    each size over all frames; entry 0 is 0), ``results.species_counts`` ``[G, s_max + 1]`` (int64, atoms of each
    group in clusters of each size), ``results.bonds``, ``results.n_clusters``, ``results.largest`` and
    ``results.sum_squares`` ``[F]`` (int64, per frame: bonded pairs, clusters, the largest cluster, the sum of
    the squared sizes), ``results.size_distribution`` — ``size_counts / size_counts.sum()`` —
    ``results.weight_distribution`` — ``sizes * size_counts / (F * n)`` — ``results.species_fractions`` —
    ``species_counts / (F * N_g)``, column 1 is the free fraction of each group — ``results.mean_size`` —
    ``n / n_clusters`` — ``results.weight_mean_size`` — ``sum_squares / n`` — ``results.labels`` ``[F, n]`` (int32,
    with ``store_labels``: the smallest row of every atom's cluster, rows in the order of the concatenated groups)
    and ``results.units``.

    Limits: a constant orthorhombic box, coordinates as given, no molecule centres, every pair of atoms evaluated
    (no cell list), no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, groups, cutoff, *, max_neighbors: int = 32, store_labels: bool = False, dimensions=None,
                 drop_axis=None, verbose: bool = True, **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "indices") else list(groups)
        if not 1 <= len(self._groups) <= _core.ClusterEngine.MAX_SPECIES:
            raise ValueError(f"'groups' must hold between 1 and {_core.ClusterEngine.MAX_SPECIES} groups.")
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        G = len(self._groups)

        indices = [np.asarray(g.indices) for g in self._groups]
        if any(len(i) < 1 for i in indices):
            raise ValueError("The groups must hold at least one atom.")
        self._index = np.concatenate(indices)
        if len(np.unique(self._index)) != len(self._index):
            raise ValueError("The groups share some atoms: they must be disjoint.")
        self._n_group = np.array([len(i) for i in indices], dtype=np.int64)
        self._species = np.repeat(np.arange(G, dtype=np.int32), self._n_group)
        self._N = len(self._index)

        table = np.asarray(strip_unit(cutoff, "angstrom")[0], dtype=float)
        if table.ndim == 0:
            table = np.full((G, G), float(table))
        if table.shape != (G, G):
            raise ValueError(f"'cutoff' must be a number or a {G} x {G} table, one row per group.")
        if not (np.all(np.isfinite(table)) and np.all(table >= 0)):
            raise ValueError("'cutoff' must be finite and not negative.")
        if not np.array_equal(table, table.T):
            raise ValueError("The 'cutoff' table must be symmetric.")
        if not np.any(table > 0):
            raise ValueError("The 'cutoff' table must hold at least one positive entry.")
        self._cutoff = table

        self._max_neighbors = int(max_neighbors)
        if not 1 <= self._max_neighbors <= _core.ClusterEngine.MAX_NEIGHBORS:
            raise ValueError(f"'max_neighbors' must lie in [1, {_core.ClusterEngine.MAX_NEIGHBORS}].")
        self._store_labels = bool(store_labels)

        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, self._cutoff.max(), "cutoff")
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # a frame needs no other frame

    def _prepare(self) -> None:
        self.results.units = {"results.sizes": "atoms"}
        _lib.require_device(self._device)
        self._feed_engine(_core.ClusterEngine(
            self._species, self._cutoff, self._dimensions, n_species=len(self._groups),
            zero_dims=zero_dims(self._drop_axis), max_neighbors=self._max_neighbors,
            keep_labels=self._store_labels, dev=self._device), self._index)

    def _conclude(self) -> None:
        try:
            self._batch.flush()
            counts = self._engine.result()
            per_frame = self._engine.frames()
            labels = self._engine.labels() if self._store_labels else None
        finally:
            self._engine.close()
        F, n = self.n_frames, self._N
        size_counts, species_counts = counts["size_counts"], counts["species_counts"]
        if self._comm.world_size > 1:
            # the counts add up at their full length n + 1; the per-frame arrays (and the labels) are gathered
            size_counts = np.asarray(self._comm.allreduce(size_counts, op="sum"))
            species_counts = np.asarray(self._comm.allreduce(species_counts, op="sum"))
            for key, rows in per_frame.items():
                per_frame[key] = self._gather_frame_rows(rows)
            if labels is not None:
                labels = self._gather_frame_rows(labels)
        seen = np.flatnonzero(size_counts)
        s_max = int(seen[-1]) if len(seen) else 0
        res = self.results
        res.sizes = np.arange(s_max + 1)
        res.size_counts = size_counts[:s_max + 1]
        res.species_counts = species_counts[:, :s_max + 1]
        for key, rows in per_frame.items():
            res[key] = rows
        total = res.size_counts.sum()
        res.size_distribution = res.size_counts / (total if total else np.nan)
        res.weight_distribution = res.sizes * res.size_counts / ((F * n) if F else np.nan)
        res.species_fractions = res.species_counts / ((F * self._n_group) if F else
                                                      np.full(len(self._n_group), np.nan))[:, None]
        clusters = res.n_clusters.astype(float)
        clusters[clusters == 0] = np.nan
        res.mean_size = n / clusters
        res.weight_mean_size = res.sum_squares / n
        if labels is not None:
            res.labels = labels
