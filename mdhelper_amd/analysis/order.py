"""
Local order: ``BondOrientationalOrder`` — the Steinhardt bond-orientational order parameters ``q_l`` of every particle
and their neighbour-averaged form ``q̄_l`` (Lechner and Dellago), which tell a liquid-like shell from an fcc-, hcp- or
bcc-like one — and ``TetrahedralOrder`` — the orientational tetrahedral order ``q`` of water and other network
liquids over the four nearest neighbours, its translational counterpart ``S_k`` and the distances to the nearest
neighbours rank by rank.

Whole blocks of frames go to the bond-order engine (``mdx_boo_*``), which tests every (centre, candidate) pair of a
frame in float64 (minimum image, ``r2 <= cutoff ** 2``), keeps the neighbours as capped per-centre lists in HBM, sorts
every list, sums the spherical harmonics of a centre's bonds in ascending neighbour order, and bins the invariants with
integer atomics (csrc/mdx_bond_order_device.hpp).  A frame needs no other frame, so the frames shard across ranks.

``TetrahedralOrder`` feeds the tetrahedral engine (``mdx_tet_*``), which walks the same pairs but keeps, per centre and
in registers, the ``n_nearest`` nearest candidates in range, ordered by ``(r2, candidate number)``: a function of the
frame alone (csrc/mdx_tetrahedral_device.hpp).
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, pair_selection
from .hbond import distance_thresholds


class BondOrientationalOrder(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Steinhardt bond-orientational order.  A candidate :math:`j` is a neighbour of a centre :math:`i` where its
    minimum-image distance is at most ``cutoff``; with :math:`N_b(i)` the number of neighbours and
    :math:`\hat{\mathbf r}_{ij}` the unit vector of the bond,

    .. math:: q_{lm}(i)=\frac{1}{N_b(i)}\sum_{j}Y_{lm}(\hat{\mathbf r}_{ij}),\qquad
              q_l(i)=\sqrt{\frac{4\pi}{2l+1}\sum_{m=-l}^{l}|q_{lm}(i)|^2}

    (:math:`Y_{lm}` with the Condon–Shortley phase, ``scipy.special.sph_harm_y``), and the neighbour-averaged form

    .. math:: \bar q_{lm}(i)=\frac{1}{N_b(i)+1}\Big(q_{lm}(i)+\sum_{j}q_{lm}(j)\Big),\qquad
              \bar q_l(i)=\sqrt{\frac{4\pi}{2l+1}\sum_{m=-l}^{l}|\bar q_{lm}(i)|^2}

    which separates the crystal structures more sharply.  Both are rotationally invariant and lie in ``[0, 1]``.  What
    the perfect lattices give (first shell, :math:`\bar q_l=q_l` there):

    ========  ===========  ==============================  ===============================
    lattice   neighbours   :math:`q_4`                     :math:`q_6`
    ========  ===========  ==============================  ===============================
    sc        6            :math:`\sqrt{7/12}=0.7638`      :math:`\sqrt{1/8}=0.3536`
    bcc       8            :math:`\sqrt{7/27}=0.5092`      :math:`\sqrt{32/81}=0.6285`
    fcc       12           :math:`\sqrt{7/192}=0.1909`     :math:`\sqrt{169/512}=0.5745`
    hcp       12           :math:`0.0972`                  :math:`0.4848`
    liquid    ≈ 12         ≈ 0.19 (broad)                  ≈ 0.3 – 0.4 (broad); :math:`\bar q_6` ≈ 0.15
    ========  ===========  ==============================  ===============================

    Parameters
    ----------
    group : AtomGroup — the centres
    neighbors : AtomGroup, optional — the neighbour candidates.  ``None``, or the very atoms of ``group`` in the same
        order: the neighbours of a centre are the other centres.  Otherwise it must be disjoint from ``group``
    cutoff : float — the radius of the first shell (Å), positive and finite, at most half the shortest box length
    degrees : sequence of int, keyword-only — the degrees ``l``, ``1 ... 12``, at most 4 distinct ones
    averaged : bool, keyword-only — also form :math:`\bar q_l`.  It needs the neighbours of a centre to be centres
        themselves: the default is ``True`` where ``neighbors`` is ``group`` (or ``None``) and ``False`` for a
        disjoint ``neighbors``, with which ``averaged=True`` raises ``ValueError``
    n_bins, range : int and ``(low, high)``, keyword-only — the histogram's bins of equal width,
        ``edges = linspace(low, high, n_bins + 1)``, counted as ``numpy.histogram`` does
    max_neighbors : int, keyword-only — the neighbours a centre may have in one frame (1 ... 64).  A frame with more
        raises ``ValueError`` at the end of ``run()``: nothing is truncated silently
    keep_values : bool, keyword-only — keep every centre's values of every frame (``results["values"]``)
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    verbose : bool
    device : keyword-only — the HIP device
    comm : communicator, keyword-only — the frames shard across ranks

    Results
    -------
    With ``D`` degrees, ``K = 2`` with ``averaged`` (``k = 0``: :math:`q_l`, ``k = 1``: :math:`\bar q_l`) and else 1,
    ``F`` analysed frames and ``n0`` centres: ``results.degrees``; ``results.edges`` ``[n_bins + 1]`` and
    ``results.bins`` ``[n_bins]`` (the bin centres); ``results.counts`` ``[D, K, n_bins]`` and ``results.outside``
    ``[D, K]`` (the values outside ``range``), int64, over every (frame, centre) with at least one neighbour;
    ``results.distribution`` — ``counts / (counts.sum(-1) * bin width)``, rows that integrate to 1, a row of NaN where
    nothing was counted; ``results.mean`` ``[F, D, K]`` — the mean over the centres of a frame that have a neighbour
    (NaN where there is none) and ``results.mean_overall`` ``[D, K]`` over all frames; ``results.coordination_counts``
    ``[m_max + 1]`` (the (frame, centre) cases with exactly ``m`` neighbours, trimmed to the largest ``m`` seen),
    ``results.coordination_distribution`` — ``coordination_counts / (F * n0)`` and ``results.coordination_number`` —
    its mean; with ``keep_values`` ``results["values"]`` ``[F, D, K, n0]``, NaN for a centre without a neighbour
    (read it by item: as an attribute ``values`` is the mapping's own method); and ``results.units``.

    Limits: a constant orthorhombic box, three dimensions, coordinates as given, every (centre, candidate) pair
    evaluated (no cell list).  A neighbour that sits exactly on its centre has no direction: ``run()`` then raises
    ``ValueError`` instead of averaging it.  No CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, group, neighbors=None, cutoff=None, *, degrees=(4, 6), averaged: bool = None,
                 n_bins: int = 100, range=(0.0, 1.0), max_neighbors: int = 32, keep_values: bool = False,
                 dimensions=None, verbose: bool = True, **kwargs) -> None:
        if "drop_axis" in kwargs:
            raise TypeError("BondOrientationalOrder takes no 'drop_axis': q_l is a quantity of three dimensions.")
        self.universe = group.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if cutoff is None:
            raise TypeError("'cutoff' is required.")
        self._same, self._n_centers, self._n_neighbors, self._index = pair_selection(group, neighbors)
        if averaged and not self._same:
            raise ValueError("'averaged' needs the neighbours of a centre to be centres themselves: leave 'neighbors' "
                             "out or pass averaged=False.")
        self._averaged = self._same if averaged is None else bool(averaged)

        cut = float(strip_unit(cutoff, "angstrom")[0])
        if not (np.isfinite(cut) and cut > 0):
            raise ValueError("'cutoff' must be positive and finite.")
        self._cutoff = cut

        engine = _core.BondOrderEngine
        self._degrees = np.atleast_1d(np.asarray(degrees))
        if (self._degrees.ndim != 1 or not 1 <= len(self._degrees) <= engine.MAX_DEGREES
                or not np.issubdtype(self._degrees.dtype, np.integer)):
            raise ValueError(f"'degrees' must hold between 1 and {engine.MAX_DEGREES} integers.")
        if self._degrees.min() < 1 or self._degrees.max() > engine.MAX_DEGREE:
            raise ValueError(f"'degrees' must lie in [1, {engine.MAX_DEGREE}].")
        if len(np.unique(self._degrees)) != len(self._degrees):
            raise ValueError("'degrees' holds a degree twice.")
        self._degrees = self._degrees.astype(np.int32)

        self._n_bins = int(n_bins)
        if self._n_bins < 1:
            raise ValueError("'n_bins' must be at least 1.")
        if len(range) != 2 or not (np.all(np.isfinite(range)) and range[0] < range[1]):
            raise ValueError("'range' must be (low, high) with low < high, both finite.")
        self._edges = np.linspace(float(range[0]), float(range[1]), self._n_bins + 1)
        self._max_neighbors = int(max_neighbors)
        if not 1 <= self._max_neighbors <= engine.MAX_NEIGHBORS:
            raise ValueError(f"'max_neighbors' must lie in [1, {engine.MAX_NEIGHBORS}].")
        self._keep_values = bool(keep_values)

        self._drop_axis = None              # q_l is a quantity of three dimensions
        self._dimensions = self._box_lengths(dimensions, self._cutoff, "cutoff")
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # a frame needs no other frame

    def _prepare(self) -> None:
        self.results.units = {"results.edges": "dimensionless", "results.bins": "dimensionless"}
        _lib.require_device(self._device)
        self._feed_engine(_core.BondOrderEngine(
            self._n_centers, self._n_neighbors, self._cutoff, self._degrees, self._edges, self._dimensions,
            same=self._same, averaged=self._averaged, max_neighbors=self._max_neighbors,
            keep_values=self._keep_values, dev=self._device), self._index)

    def _conclude(self) -> None:
        try:
            self._batch.flush()
            got = self._engine.result()
            rows = self._engine.frames()
            values = self._engine.values() if self._keep_values else None
        finally:
            self._engine.close()
        counts, outside, coordination = got["counts"], got["outside"], got["coordination"]
        if self._comm.world_size > 1:
            counts = np.asarray(self._comm.allreduce(counts, op="sum"))
            outside = np.asarray(self._comm.allreduce(outside, op="sum"))
            coordination = np.asarray(self._comm.allreduce(coordination, op="sum"))
        sums = self._gather_frame_rows(rows["sums"])
        counted = self._gather_frame_rows(rows["counted"])
        F, n0 = self.n_frames, self._n_centers
        seen = np.flatnonzero(coordination)
        m_max = int(seen[-1]) if len(seen) else 0
        res = self.results
        res.degrees = self._degrees.astype(np.int64)
        res.edges = self._edges
        res.bins = (self._edges[:-1] + self._edges[1:]) / 2
        res.counts = counts
        res.outside = outside
        total = counts.sum(axis=-1).astype(float)
        total[total == 0] = np.nan
        res.distribution = counts / (total[..., None] * np.diff(self._edges))
        per_frame = counted.astype(float)
        per_frame[per_frame == 0] = np.nan          # a frame of isolated centres: NaN, without a warning
        res.mean = sums / per_frame[:, None, None]
        res.mean_overall = sums.sum(axis=0) / (counted.sum() if counted.sum() else np.nan)
        res.coordination_counts = coordination[:m_max + 1]
        res.coordination_distribution = res.coordination_counts / ((F * n0) if F else np.nan)
        res.coordination_number = res.coordination_distribution @ np.arange(m_max + 1)
        if values is not None:
            res["values"] = self._gather_frame_rows(values)


def distance_table(edges) -> np.ndarray:
    """The increasing table of ``r2`` against which ``numpy.histogram``'s rule counts like ``edges`` of
    ``r = sqrt(r2)``: ``hbond.distance_thresholds`` for every edge but the last, which a value may equal and still be
    counted: there the table holds ``max{x : sqrt(x) <= edges[-1]}``."""
    edges = np.asarray(edges, dtype=np.float64)
    table = distance_thresholds(edges)
    x, last = table[-1], edges[-1]
    if np.sqrt(x) > last:                   # no r2 has this root: the largest below it
        x = np.nextafter(x, -np.inf)
    else:
        while np.sqrt(np.nextafter(x, np.inf)) <= last:
            x = np.nextafter(x, np.inf)
    table[-1] = x
    return table


class TetrahedralOrder(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Tetrahedral order.  With :math:`\psi_{ab}` the angle at a centre between its :math:`a`-th and :math:`b`-th nearest
    neighbours and :math:`r_a` their distances, over the four nearest neighbours (Chau and Hardwick; Errington and
    Debenedetti),

    .. math:: q=1-\frac{3}{8}\sum_{a<b}\Big(\cos\psi_{ab}+\frac{1}{3}\Big)^2,\qquad
              S_k=1-\frac{1}{3}\sum_{a=1}^{4}\frac{(r_a-\bar r)^2}{4\bar r^2}

    :math:`q` is 1 for a regular tetrahedron and 0 on average for an ideal gas (its lowest value is :math:`-3`);
    :math:`S_k` is 1 where the four distances are equal and falls towards 0 as they spread.  The neighbours of a
    centre are the ``n_nearest`` nearest candidates within ``cutoff`` by minimum-image distance; two candidates at
    bit-equal distances are ordered by their place in ``neighbors``, so the selection is a function of the frame
    alone.

    Parameters
    ----------
    group : AtomGroup — the centres
    neighbors : AtomGroup, optional — the neighbour candidates.  ``None``, or the very atoms of ``group`` in the same
        order: the neighbours of a centre are the other centres.  Otherwise it must be disjoint from ``group``
    n_nearest : int, keyword-only — the neighbours selected per centre, ``4 ... 8``; :math:`q` and :math:`S_k` take
        the first four, the distance distributions all of them
    cutoff : float, keyword-only — the reach of the search (Å); defaults to half the shortest box length, which it
        may not exceed.  A centre with fewer than four candidates within it is *short*: it has no :math:`q`
    n_bins, range : keyword-only — the histogram of :math:`q`, ``edges = linspace(low, high, n_bins + 1)``, counted as
        ``numpy.histogram`` does
    sk_bins, sk_range : keyword-only — the same for :math:`S_k`
    distance_bins, distance_range : keyword-only — the same for the distance to the neighbour of every rank (Å);
        ``distance_range`` defaults to ``(0, cutoff)``
    keep_values : bool, keyword-only — keep every centre's values and neighbours of every frame
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    verbose : bool
    device : keyword-only — the HIP device
    comm : communicator, keyword-only — the frames shard across ranks

    Results
    -------
    With ``k = n_nearest``, ``F`` analysed frames and ``n0`` centres: ``results.q_edges``, ``results.q_bins`` (the bin
    centres), ``results.q_counts`` ``[n_bins]`` and ``results.q_outside`` (int64, over every (frame, centre) that is
    not short), ``results.q_distribution`` — ``counts / (counts.sum() * bin width)``, NaN where nothing was counted
    — and the same five with ``sk_``; ``results.distance_edges``, ``results.distance_bins``,
    ``results.distance_counts`` ``[k, distance_bins]`` and ``results.distance_outside`` ``[k]`` — rank ``a``'s
    distance over every (frame, centre) that has more than ``a`` candidates within the cutoff, short ones included —
    and ``results.distance_distribution``, rows that integrate to 1; ``results.mean`` ``[F, 2]`` — the means of
    :math:`q` and :math:`S_k` over the centres of a frame that are not short (NaN where all are) and ``results.mean_overall`` ``[2]``; ``results.found_counts``
    ``[k + 1]`` — the (frame, centre) cases with ``min(candidates within the cutoff, k) = m``; with ``keep_values``
    ``results["values"]`` ``[F, 2, n0]``, NaN for a short centre (read it by item: as an attribute ``values`` is the
    mapping's own method) and ``results.neighbors`` ``[F, k, n0]``, int32 places in ``neighbors``, nearest first, ``-1``
    beyond those a centre has; and ``results.units``.

    Limits: a constant orthorhombic box, three dimensions, coordinates as given, every (centre, candidate) pair
    evaluated (no cell list).  One of a centre's four nearest exactly on it has no direction: ``run()`` then raises
    ``ValueError``.  No CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, group, neighbors=None, *, n_nearest: int = 4, cutoff=None, n_bins: int = 150,
                 range=(-0.5, 1.0), sk_bins: int = 100, sk_range=(0.0, 1.0), distance_bins: int = 200,
                 distance_range=None, keep_values: bool = False, dimensions=None, verbose: bool = True,
                 **kwargs) -> None:
        if "drop_axis" in kwargs:
            raise TypeError("TetrahedralOrder takes no 'drop_axis': q is a quantity of three dimensions.")
        self.universe = group.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        self._same, self._n_centers, self._n_neighbors, self._index = pair_selection(group, neighbors)

        engine = _core.TetrahedralEngine
        if int(n_nearest) != n_nearest or not engine.MIN_NEAREST <= n_nearest <= engine.MAX_NEAREST:
            raise ValueError(f"'n_nearest' must be an integer in [{engine.MIN_NEAREST}, {engine.MAX_NEAREST}].")
        self._n_nearest = int(n_nearest)

        self._drop_axis = None              # q is a quantity of three dimensions
        if cutoff is None:
            self._dimensions = self._box_lengths(dimensions, 0.0, "cutoff")
            self._cutoff = float(self._dimensions.min() / 2)
        else:
            cut = float(strip_unit(cutoff, "angstrom")[0])
            if not (np.isfinite(cut) and cut > 0):
                raise ValueError("'cutoff' must be positive and finite.")
            self._cutoff = cut
            self._dimensions = self._box_lengths(dimensions, cut, "cutoff")

        def edges_of(bins, span, what, low_limit=-np.inf):
            if int(bins) != bins or bins < 1:
                raise ValueError(f"'{what[0]}' must be at least 1.")
            if (span is None or len(span) != 2 or not np.all(np.isfinite(span)) or not span[0] < span[1]
                    or span[0] < low_limit):
                raise ValueError(f"'{what[1]}' must be (low, high) with low < high, both finite"
                                 + (f" and low >= {low_limit:g}." if np.isfinite(low_limit) else "."))
            return np.linspace(float(span[0]), float(span[1]), int(bins) + 1)

        self._q_edges = edges_of(n_bins, range, ("n_bins", "range"))
        self._s_edges = edges_of(sk_bins, sk_range, ("sk_bins", "sk_range"))
        if distance_range is None:
            distance_range = (0.0, self._cutoff)
        else:
            distance_range = tuple(strip_unit(x, "angstrom")[0] for x in distance_range)
        self._d_edges = edges_of(distance_bins, distance_range, ("distance_bins", "distance_range"), 0.0)
        self._keep_values = bool(keep_values)
        self._verbose = verbose

    @classmethod
    def from_molecules(cls, group, n_molecules: int, atom: int = 0, **kwargs):
        """``group`` holds ``n_molecules`` molecules of equal size laid end to end; the atom at place ``atom`` of every
        molecule (the default: the first, the oxygen of an "O H H" water) is a centre, and the centres are their own
        candidates."""
        n_molecules = int(n_molecules)
        if n_molecules < 1 or group.n_atoms % n_molecules:
            raise ValueError("'group' must hold n_molecules molecules of equal size.")
        size = group.n_atoms // n_molecules
        if int(atom) != atom or not 0 <= atom < size:
            raise ValueError(f"'atom' must lie in [0, {size}), the size of a molecule.")
        return cls(group[np.arange(n_molecules) * size + int(atom)], **kwargs)

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # a frame needs no other frame

    def _prepare(self) -> None:
        self.results.units = {"results.q_edges": "dimensionless", "results.q_bins": "dimensionless",
                              "results.sk_edges": "dimensionless", "results.sk_bins": "dimensionless",
                              "results.distance_edges": "angstrom", "results.distance_bins": "angstrom",
                              "results.distance_distribution": "angstrom^-1"}
        _lib.require_device(self._device)
        self._feed_engine(_core.TetrahedralEngine(
            self._n_centers, self._n_neighbors, self._cutoff, self._q_edges, self._s_edges,
            distance_table(self._d_edges), self._dimensions, n_nearest=self._n_nearest, same=self._same,
            keep_values=self._keep_values, dev=self._device), self._index)

    def _conclude(self) -> None:
        try:
            self._batch.flush()
            got = self._engine.result()
            rows = self._engine.frames()
            kept = self._engine.values() if self._keep_values else None
        finally:
            self._engine.close()
        if self._comm.world_size > 1:
            got = {key: np.asarray(self._comm.allreduce(value, op="sum")) for key, value in got.items()}
        sums = self._gather_frame_rows(rows["sums"])
        counted = self._gather_frame_rows(rows["counted"])

        def distribution(counts, edges):
            total = counts.sum(axis=-1, keepdims=True).astype(float)
            total[total == 0] = np.nan
            return counts / (total * np.diff(edges))

        res = self.results
        for name, edges, counts, outside in (("q", self._q_edges, got["q_counts"], got["outside"][0]),
                                             ("sk", self._s_edges, got["s_counts"], got["outside"][1]),
                                             ("distance", self._d_edges, got["distance_counts"],
                                              got["distance_outside"])):
            res[f"{name}_edges"] = edges
            res[f"{name}_bins"] = (edges[:-1] + edges[1:]) / 2
            res[f"{name}_counts"] = counts
            res[f"{name}_outside"] = outside
            res[f"{name}_distribution"] = distribution(counts, edges)
        per_frame = counted.astype(float)
        per_frame[per_frame == 0] = np.nan          # a frame of short centres: NaN, without a warning
        res.mean = sums / per_frame[:, None]
        res.mean_overall = sums.sum(axis=0) / (counted.sum() if counted.sum() else np.nan)
        res.found_counts = got["found"]
        if kept is not None:
            res["values"] = self._gather_frame_rows(kept["values"])
            res.neighbors = self._gather_frame_rows(kept["neighbors"])
