"""
Spatial distribution functions: ``SpatialDistributionFunction`` — the three-dimensional density of a species around a
reference molecule, in that molecule's own (body-fixed) frame: the tetrahedral lobes around a water molecule, the
anions above and below an imidazolium ring.

Whole blocks of frames go to the spatial-distribution engine (``mdx_sdf_*``), which forms the frame of every reference
molecule from three of its atoms, tests every (molecule, partner) pair of a frame in float64 (minimum image,
``r2 <= cutoff ** 2``), rotates the partners within the cutoff into the molecule's frame and counts them in a 3-D
histogram per partner group with integer atomics (csrc/mdx_sdf_device.hpp).  A frame needs no other frame, so the
frames shard across ranks.
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis

_MODES = {"axis": _core.SpatialDistributionEngine.AXIS, "bisector": _core.SpatialDistributionEngine.BISECTOR}


class SpatialDistributionFunction(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Density of neighbour atoms around reference molecules, in the local frame of each molecule.  A molecule is three
    atoms: the origin :math:`O`, the axis atom :math:`A` and the plane atom :math:`B`.  With :math:`\mathbf a`,
    :math:`\mathbf b` the minimum-image vectors from :math:`O` to :math:`A` and :math:`B`, and :math:`\mathbf p =
    \mathbf a` (``frame="axis"``) or :math:`\mathbf p = \hat{\mathbf a} + \hat{\mathbf b}` (``frame="bisector"``),

    .. math:: \mathbf e_1 = \hat{\mathbf p},\qquad \mathbf e_3 = \widehat{\mathbf p\times\mathbf b},\qquad
              \mathbf e_2 = \mathbf e_3\times\mathbf e_1

    so that :math:`B` lies in the local xy plane at :math:`y > 0`.  A neighbour at the minimum-image vector
    :math:`\mathbf w` from :math:`O`, with :math:`|\mathbf w|` at most ``cutoff``, is counted at :math:`(\mathbf
    w\cdot\mathbf e_1, \mathbf w\cdot\mathbf e_2, \mathbf w\cdot\mathbf e_3)` with ``numpy.histogramdd``'s rule.

    Parameters
    ----------
    origins, axis_atoms, plane_atoms : AtomGroup — of one length: molecule ``i`` is ``origins[i]``, ``axis_atoms[i]``
        and ``plane_atoms[i]``, three different atoms.  An origin may not repeat
    neighbors : AtomGroup or sequence of at most 8 AtomGroups — the species whose density is mapped; no atom twice
    range : float or three ``(lo, hi)`` pairs, keyword-only — ``R`` for ``[-R, R]`` on all three local axes (Å)
    n_bins : int or three ints, keyword-only — bins per axis (at most 512 each); the edges are ``numpy.linspace``
    frame : {"axis", "bisector"}, keyword-only — ``"axis"`` puts :math:`A` on local +x; ``"bisector"`` puts the
        bisector of :math:`A` and :math:`B` there (the choice for water: the dipole axis)
    cutoff : float, keyword-only — the radius of the sphere beyond which nothing counts (Å).  Defaults to the sphere
        around the box of ``range``, inflated by ``1 + 2**-40`` so that rounding in the rotation clips no corner.  It
        may not exceed half the shortest box length
    owners : array-like of int, keyword-only — over the concatenated neighbour atoms: the molecule (its place in
        ``origins``) an atom belongs to, or -1.  An atom is never counted around its own molecule.  By default an
        atom that is the origin, axis or plane atom of exactly one molecule belongs to it, and one that is a frame
        atom of several molecules raises ``ValueError``
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    verbose : bool
    device : keyword-only — the HIP device
    comm : communicator, keyword-only — the frames shard across ranks

    Results
    -------
    With ``G`` neighbour groups, ``F`` analysed frames and ``n_ref`` molecules: ``results.edges`` and
    ``results.bins`` (the bin centres) — lists of three arrays, Å; ``results.counts`` int64 ``[G, nx, ny, nz]``;
    ``results.inside`` int64 ``[F]`` (the counted pairs of every frame) and ``results.coordination`` — ``inside /
    n_ref``; ``results.degenerate`` — the (frame, molecule) cases whose three atoms span no frame (one on another, or
    collinear): they count nothing; ``results.density`` — ``counts / (F * n_ref * bin volume)``, Å⁻³;
    ``results.sdf`` — ``density / rho_g`` with ``rho_g = (N_g - x_g) / V`` and ``x_g`` the mean number of atoms of
    group ``g`` a molecule owns, so that a structureless fluid gives 1; and ``results.units``.
    ``calculate_radial_average()`` adds ``results.radial_edges``, ``results.radial_bins`` and
    ``results.radial_density``.

    Limits: a constant orthorhombic box, coordinates as given, all three components take part, every (molecule,
    neighbour) pair evaluated (no cell list), no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    _shard_frames = True        # a frame needs no other frame
    _drop_axis = None           # all three components take part (_box_lengths)

    def __init__(self, origins, axis_atoms, plane_atoms, neighbors, *, range=6.0, n_bins=60, frame: str = "axis",
                 cutoff: float = None, owners=None, dimensions=None, verbose: bool = True, **kwargs) -> None:
        groups = [neighbors] if hasattr(neighbors, "indices") else list(neighbors)
        max_groups = _core.SpatialDistributionEngine.MAX_GROUPS
        if not 1 <= len(groups) <= max_groups:
            raise ValueError(f"'neighbors' must hold between 1 and {max_groups} groups.")
        self.universe = origins.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)

        o, a, b = (np.asarray(g.indices) for g in (origins, axis_atoms, plane_atoms))
        if not len(o) == len(a) == len(b):
            raise ValueError(f"'origins' holds {len(o)} atoms, 'axis_atoms' {len(a)} and 'plane_atoms' {len(b)}: a "
                             "molecule needs one of each.")
        if len(o) < 1:
            raise ValueError("There must be at least one reference molecule.")
        if np.any(o == a) or np.any(o == b) or np.any(a == b):
            raise ValueError("The origin, the axis atom and the plane atom of a molecule must be three different "
                             "atoms.")
        if len(np.unique(o)) != len(o):
            raise ValueError("'origins' holds an atom twice.")
        parts = [np.asarray(g.indices) for g in groups]
        p = np.concatenate(parts)
        if len(p) < 1:
            raise ValueError("'neighbors' must hold at least one atom.")
        if len(np.unique(p)) != len(p):
            raise ValueError("'neighbors' holds an atom twice.")
        self._n_ref, self._n_p = len(o), len(p)
        self._group_start = np.concatenate(([0], np.cumsum([len(i) for i in parts]))).astype(np.int64)

        if owners is None:
            # the molecules an atom frames: one of them owns it, several need the caller's word
            atoms = np.concatenate((o, a, b))
            molecule = np.tile(np.arange(len(o)), 3)
            pairs = np.unique(np.stack((atoms, molecule), axis=1), axis=0)
            framed, times = np.unique(pairs[:, 0], return_counts=True)
            shared = np.intersect1d(framed[times > 1], p)
            if len(shared):
                raise ValueError(f"Atom {shared[0]} of 'neighbors' is a frame atom of several reference molecules: "
                                 "pass owners= to say which molecule it belongs to.")
            owner = np.full(len(p), -1, dtype=np.int32)
            place = np.searchsorted(pairs[:, 0], p)
            place[place == len(pairs)] = 0
            found = pairs[place, 0] == p
            owner[found] = pairs[place[found], 1]
        else:
            owner = np.asarray(owners)
            if owner.shape != (len(p),) or not np.issubdtype(owner.dtype, np.integer):
                raise ValueError(f"'owners' must hold one integer per neighbour atom, {len(p)} of them.")
            if owner.min() < -1 or owner.max() >= len(o):
                raise ValueError(f"'owners' must lie in [-1, {len(o)}): a molecule's place in 'origins', or -1.")
            owner = owner.astype(np.int32)
        self._owner = owner

        # the distinct atoms are fed once; the tables name them by their place in that feed
        self._index, inverse = np.unique(np.concatenate((o, a, b, p)), return_inverse=True)
        inverse = inverse.astype(np.int32)
        n = len(o)
        self._o_row, self._a_row, self._b_row, self._p_row = (inverse[:n], inverse[n:2 * n], inverse[2 * n:3 * n],
                                                              inverse[3 * n:])

        if frame not in _MODES:
            raise ValueError("Invalid value passed to 'frame'. The valid values are 'axis' and 'bisector'.")
        self._mode = _MODES[frame]

        span = np.asarray(strip_unit(range, "angstrom")[0], dtype=float)
        if span.ndim == 0:
            span = np.tile([-float(span), float(span)], (3, 1))
        if span.shape != (3, 2) or not np.all(np.isfinite(span)) or np.any(span[:, 0] >= span[:, 1]):
            raise ValueError("'range' must be a positive number R, for [-R, R] on every axis, or three (lo, hi) pairs "
                             "with lo < hi.")
        bins = np.asarray(n_bins)
        if bins.ndim == 0:
            bins = np.tile(bins, 3)
        most = _core.SpatialDistributionEngine.MAX_AXIS_BINS
        if bins.shape != (3,) or not np.issubdtype(bins.dtype, np.integer) or bins.min() < 1 or bins.max() > most:
            raise ValueError(f"'n_bins' must be an integer or three, each in [1, {most}].")
        if len(groups) * int(np.prod(bins.astype(np.int64))) > 1 << 26:
            raise ValueError("'n_bins' asks for more than 2^26 counters over all groups.")
        self._edges = [np.linspace(lo, hi, int(m) + 1) for (lo, hi), m in zip(span, bins)]

        if cutoff is None:
            self._cutoff = float(np.sqrt((np.abs(span).max(axis=1) ** 2).sum()) * (1.0 + 2.0 ** -40))
        else:
            self._cutoff = float(strip_unit(cutoff, "angstrom")[0])
            if not (np.isfinite(self._cutoff) and self._cutoff > 0):
                raise ValueError("'cutoff' must be positive and finite.")
        try:
            self._dimensions = self._box_lengths(dimensions, self._cutoff, "cutoff")
        except ValueError as err:
            if "beyond half" not in str(err):
                raise
            raise ValueError(f"{err}  The sphere of radius {self._cutoff:g} Å around 'range' does not fit: pass a "
                             "smaller cutoff= (or a smaller range).") from None
        self._verbose = verbose

    @classmethod
    def from_molecules(cls, ag, n_molecules: int, origin: int = 0, axis: int = 1, plane: int = 2,
                       neighbors=((0,), (1, 2)), **kwargs):
        """``ag`` holds ``n_molecules`` molecules of equal size laid end to end; ``origin``, ``axis`` and ``plane``
        are the places of the three frame atoms inside a molecule and ``neighbors`` lists, per group, the places of
        the atoms to map.  Every atom belongs to its molecule.  The defaults are a three-site water: the oxygen
        first, then its two hydrogens; the oxygens are one group and the hydrogens another."""
        n_molecules = int(n_molecules)
        if n_molecules < 1 or ag.n_atoms % n_molecules:
            raise ValueError("'ag' must hold n_molecules molecules of equal size.")
        size = ag.n_atoms // n_molecules
        groups = [np.atleast_1d(np.asarray(g, dtype=int)) for g in neighbors]
        if not groups or any(len(g) < 1 for g in groups):
            raise ValueError("'neighbors' must hold at least one group of at least one place.")
        places = np.concatenate(([origin, axis, plane], *groups))
        if places.min() < 0 or places.max() >= size:
            raise ValueError(f"The places must lie in [0, {size}), the size of a molecule.")
        place = np.arange(n_molecules * size).reshape(n_molecules, size)
        owners = np.concatenate([np.repeat(np.arange(n_molecules), len(g)) for g in groups])
        return cls(ag[place[:, origin]], ag[place[:, axis]], ag[place[:, plane]],
                   [ag[place[:, g].ravel()] for g in groups], owners=owners, **kwargs)

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        self.results.units = {"results.edges": "angstrom", "results.bins": "angstrom",
                              "results.density": "angstrom^-3", "results.radial_edges": "angstrom",
                              "results.radial_bins": "angstrom", "results.radial_density": "angstrom^-3"}
        _lib.require_device(self._device)
        engine = _core.SpatialDistributionEngine(
            len(self._index), self._o_row, self._a_row, self._b_row, self._group_start, self._p_row, self._owner,
            self._mode, self._cutoff, self._dimensions, dev=self._device)
        engine.set_bins(*self._edges)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        try:
            self._batch.flush()
            counts = self._engine.result()
            inside = self._engine.inside()
            degenerate = np.array([self._engine.stats()["degenerate"]], dtype=np.int64)
        finally:
            self._engine.close()
        if self._comm.world_size > 1:
            counts = np.asarray(self._comm.allreduce(counts, op="sum"))
            degenerate = np.asarray(self._comm.allreduce(degenerate, op="sum"))
        inside = self._gather_frame_rows(inside)
        res = self.results
        res.edges = self._edges
        res.bins = [(e[:-1] + e[1:]) / 2 for e in self._edges]
        res.counts = counts
        res.inside = inside
        res.coordination = inside / self._n_ref
        res.degenerate = int(degenerate[0])
        dx, dy, dz = (np.diff(e) for e in self._edges)
        volume = dx[:, None, None] * dy[None, :, None] * dz[None, None, :]
        res.density = counts / ((self.n_frames * self._n_ref if self.n_frames else np.nan) * volume)
        # what a molecule sees of group g in a structureless fluid: the group without the atoms the molecule owns
        sizes = np.diff(self._group_start)
        owned = np.array([(self._owner[lo:hi] >= 0).sum() for lo, hi in zip(self._group_start[:-1],
                                                                            self._group_start[1:])])
        rho = (sizes - owned / self._n_ref) / np.prod(self._dimensions)
        with np.errstate(divide="ignore", invalid="ignore"):
            res.sdf = res.density / rho[:, None, None, None]

    def calculate_radial_average(self, n_bins: int = 60) -> None:
        """``results.radial_density`` ``[G, n_bins]``: ``results.density`` averaged, weighted by the bin volumes, over
        the bins whose centres lie in a shell of ``results.radial_edges`` (``n_bins`` shells from 0 to the largest
        distance of an axis' end from the origin that all six ends reach: the sphere inside the box of ``range``).
        Approximate: a bin belongs to the shell of its centre, so the result follows g(r) times the density only to
        within a bin's width; a shell without a bin centre is NaN."""
        if "density" not in self.results:
            raise RuntimeError("Call run() before calculate_radial_average().")
        n_bins = int(n_bins)
        if n_bins < 1:
            raise ValueError("'n_bins' must be at least 1.")
        edges = self._edges
        reach = min(min(abs(e[0]), abs(e[-1])) for e in edges)
        radial_edges = np.linspace(0.0, reach, n_bins + 1)
        cx, cy, cz = self.results.bins
        r = np.sqrt(cx[:, None, None] ** 2 + cy[None, :, None] ** 2 + cz[None, None, :] ** 2).ravel()
        dx, dy, dz = (np.diff(e) for e in edges)
        volume = (dx[:, None, None] * dy[None, :, None] * dz[None, None, :]).ravel()
        shell = np.searchsorted(radial_edges, r, side="right") - 1
        ok = (shell >= 0) & (shell < n_bins)
        total = np.bincount(shell[ok], weights=volume[ok], minlength=n_bins)
        density = self.results.density.reshape(len(self.results.density), -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.results.radial_density = np.stack(
                [np.bincount(shell[ok], weights=(row * volume)[ok], minlength=n_bins) / total for row in density])
        self.results.radial_edges = radial_edges
        self.results.radial_bins = (radial_edges[:-1] + radial_edges[1:]) / 2
