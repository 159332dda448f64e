"""
Hydrogen bonds: ``HydrogenBonds`` — how many donor–H···acceptor bonds a frame holds, how many a hydrogen donates, the
distributions of the bonds' donor–acceptor distances and D–H···A angles, and how long a bond lasts (intermittent and
continuous lifetimes).

Whole blocks of frames go to the hydrogen-bond engine (``mdx_hb_*``), which tests every (hydrogen, acceptor) pair of a
frame in float64 (minimum image, ``r2_DA <= distance ** 2``, then the cosine of the angle at the hydrogen against
``cos(angle)``), keeps the bonds as capped per-hydrogen lists in a ring of frames in HBM, bins the geometry of every
bond with integer atomics and walks the lags over the rings as the residence engine does
(csrc/mdx_hbond_device.hpp).  Every lag needs every frame, so the class runs on one rank.
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, parse_drop_axis, parse_lags, zero_dims
from .dynamics import calculate_residence_time


def distance_thresholds(edges) -> np.ndarray:
    """The thresholds of ``r2`` that bin like ``edges`` of ``r = sqrt(r2)``: ``t[b] = min{x : sqrt(x) >= edges[b]}``
    in float64, found from ``edges[b] ** 2`` with ``nextafter``.  ``sqrt`` is correctly rounded and monotonic, so
    ``r2 >= t[b]`` exactly where ``sqrt(r2) >= edges[b]``: counting on ``r2`` against ``t`` gives
    ``numpy.histogram(sqrt(r2), edges)`` count for count, without a square root per value."""
    edges = np.asarray(edges, dtype=np.float64)
    t = edges * edges
    with np.errstate(invalid="ignore"):
        for b, e in enumerate(edges):
            x = t[b]
            while np.sqrt(x) < e:
                x = np.nextafter(x, np.inf)
            while np.sqrt(np.nextafter(x, -np.inf)) >= e:
                x = np.nextafter(x, -np.inf)
            t[b] = x
    return t


class HydrogenBonds(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Hydrogen bonds by the geometric rule: hydrogen :math:`H` (bonded to the donor :math:`D`) and the acceptor
    :math:`A\ne D` are bonded in a frame where the minimum-image distance :math:`r_{DA}` is at most ``distance`` and
    the angle :math:`\theta_{DHA}` at the hydrogen is at least ``angle``.  With :math:`h_{HA}(t)` 1 for a bond and 0
    otherwise the class reports the bonds of every frame, the distribution of the bonds a hydrogen donates, the
    distributions of :math:`r_{DA}` and :math:`\theta_{DHA}` over the bonds, and the lifetime functions

    .. math:: C_\mathrm{int}(t)=\frac{\langle\sum h(t_0)\,h(t_0+t)\rangle_{t_0}}{\langle\sum h(t_0)\rangle_{t_0}},
              \qquad C_\mathrm{cont}(t)=\frac{\langle\sum\prod_{t'=t_0}^{t_0+t}h(t')\rangle_{t_0}}
              {\langle\sum h(t_0)\rangle_{t_0}}

    of ``PairResidence``, over the bonds instead of the contacts.

    Parameters
    ----------
    donors, hydrogens : AtomGroup — of one length: ``donors[v]`` is the atom ``hydrogens[v]`` is bonded to.  A donor
        may repeat (both hydrogens of a water name one oxygen); a hydrogen may not, and it is never its own donor
    acceptors : AtomGroup — the acceptors, each once; no hydrogen is an acceptor, a donor may be one (it is never the
        acceptor of its own hydrogens)
    distance : float, keyword-only — the largest donor–acceptor distance of a bond (Å), positive; it may not exceed
        half the shortest box length that takes part
    angle : float, keyword-only — the smallest angle D–H···A of a bond, in degrees in ``[0, 180)``
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    origin_step : int, keyword-only — every ``origin_step``-th analysed frame is a time origin
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    max_neighbors : int, keyword-only — the bonds a hydrogen may donate in one frame (1 ... 64).  A frame with more
        raises ``ValueError`` at the end of ``run()``: nothing is truncated silently
    continuous : bool, keyword-only — ``False`` skips the frames between the lags: ``results.continuous_counts`` is
        then zero
    n_distance_bins : int, keyword-only — bins of equal width in :math:`r_{DA}` from 0 to ``distance``
    n_angle_bins : int, keyword-only — bins of equal width in :math:`\theta_{DHA}` from ``angle`` to 180°
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.times`` ``[N_t]`` (ps), ``results.n_origins`` ``[N_t]``, ``results.bonds`` ``[N_f]`` (int64, the bonds
    of every analysed frame), ``results.bonds_per_hydrogen`` — ``bonds / N_H`` — ``results.intermittent_counts``,
    ``results.continuous_counts`` and ``results.origin_counts`` ``[N_t]`` (int64), ``results.intermittent`` and
    ``results.continuous`` — the counts over ``origin_counts``, NaN without a warning where that is 0 —
    ``results.donated_counts`` ``[max_neighbors + 1]`` (int64, the (frame, hydrogen) cases with exactly ``m`` bonds)
    and ``results.donated`` — its share, which sums to 1 — ``results.distance_edges``, ``results.distance_bins`` (the
    bin centres, Å), ``results.distance_counts`` (int64: ``numpy.histogram`` of :math:`r_{DA}` over the edges, count
    for count) and ``results.distance_distribution`` (per Å, integrates to 1, NaN where there is no bond),
    ``results.angle_edges``, ``results.angle_bins`` (degrees), ``results.angle_counts`` and
    ``results.angle_distribution`` (per degree), ``results.degenerate`` (the pairs within ``distance`` whose hydrogen
    sits on its donor or on the acceptor: they have no angle and are no bond) and ``results.units``.
    ``calculate_lifetimes()`` adds ``results.lifetime`` and ``results.relaxation_time``.

    Limits: a constant orthorhombic box, coordinates as given, one rank, evenly spaced frames forward in time, every
    (hydrogen, acceptor) pair evaluated (no cell list), no exclusion but a hydrogen's own donor, no CPU fallback:
    without a HIP device ``run()`` raises ``RuntimeError``.
    """

    _shard_frames = False

    def __init__(self, donors, hydrogens, acceptors, *, distance: float = 3.0, angle: float = 150.0, lags=None,
                 n_lags: int = None, origin_step: int = 1, dt=None, dimensions=None, drop_axis=None,
                 max_neighbors: int = 8, continuous: bool = True, n_distance_bins: int = 60, n_angle_bins: int = 60,
                 verbose: bool = True, **kwargs) -> None:
        self.universe = hydrogens.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("HydrogenBonds runs on one rank: every lag needs every frame.")

        d, h, a = (np.asarray(g.indices) for g in (donors, hydrogens, acceptors))
        if len(d) != len(h):
            raise ValueError(f"'donors' holds {len(d)} atoms and 'hydrogens' {len(h)}: a hydrogen needs one donor.")
        if len(h) < 1 or len(a) < 1:
            raise ValueError("The groups must hold at least one atom.")
        if np.any(d == h):
            raise ValueError("A hydrogen is its own donor.")
        if len(np.unique(h)) != len(h):
            raise ValueError("'hydrogens' holds an atom twice.")
        if len(np.unique(a)) != len(a):
            raise ValueError("'acceptors' holds an atom twice.")
        if len(np.intersect1d(h, a)):
            raise ValueError("'hydrogens' and 'acceptors' share some atoms: a hydrogen is no acceptor.")
        self._n_h, self._n_a = len(h), len(a)
        # the distinct atoms are fed once; the tables name them by their place in that feed
        self._index, inverse = np.unique(np.concatenate((d, h, a)), return_inverse=True)
        inverse = inverse.astype(np.int32)
        self._d_row, self._h_row, self._a_row = inverse[:len(d)], inverse[len(d):2 * len(d)], inverse[2 * len(d):]

        self._distance = float(strip_unit(distance, "angstrom")[0])
        if not (np.isfinite(self._distance) and self._distance > 0):
            raise ValueError("'distance' must be positive and finite.")
        self._angle = float(angle)
        if not 0.0 <= self._angle <= 180.0:
            raise ValueError("'angle' must lie in [0, 180] degrees.")
        self._cos_max = float(np.cos(np.deg2rad(self._angle)))

        self._lags = parse_lags(lags, n_lags)
        self._origin_step = int(origin_step)
        if self._origin_step < 1:
            raise ValueError("'origin_step' must be at least 1.")
        self._max_neighbors = int(max_neighbors)
        if not 1 <= self._max_neighbors <= _core.HydrogenBondEngine.MAX_NEIGHBORS:
            raise ValueError(f"'max_neighbors' must lie in [1, {_core.HydrogenBondEngine.MAX_NEIGHBORS}].")
        self._continuous = bool(continuous)

        if int(n_distance_bins) < 1 or int(n_angle_bins) < 1:
            raise ValueError("'n_distance_bins' and 'n_angle_bins' must be at least 1.")
        self._distance_edges = np.linspace(0.0, self._distance, int(n_distance_bins) + 1)
        self._r2_thresholds = distance_thresholds(self._distance_edges)
        if np.any(np.diff(self._r2_thresholds) <= 0):
            raise ValueError("'n_distance_bins' is too large: the thresholds of r^2 are not strictly increasing.")
        self._angle_edges = np.linspace(self._angle, 180.0, int(n_angle_bins) + 1)
        self._cos_thresholds = np.cos(np.deg2rad(self._angle_edges))
        if np.any(np.diff(self._cos_thresholds) >= 0):
            raise ValueError("The thresholds of the cosine are not strictly decreasing: 'angle' leaves no room for "
                             "'n_angle_bins' bins below 180 degrees.")

        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, self._distance, "distance")
        self._verbose = verbose

    @classmethod
    def from_molecules(cls, ag, n_molecules: int, donors=((0, 1), (0, 2)), acceptors=(0,), **kwargs):
        """``ag`` holds ``n_molecules`` molecules of equal size laid end to end; ``donors`` lists the
        ``(donor, hydrogen)`` places and ``acceptors`` the acceptor places inside a molecule.  The defaults are a
        three-site water: the oxygen first, then its two hydrogens."""
        n_molecules = int(n_molecules)
        if n_molecules < 1 or ag.n_atoms % n_molecules:
            raise ValueError("'ag' must hold n_molecules molecules of equal size.")
        size = ag.n_atoms // n_molecules
        pairs = np.asarray(donors, dtype=int).reshape(-1, 2)
        places = np.atleast_1d(np.asarray(acceptors, dtype=int))
        if len(pairs) < 1 or len(places) < 1:
            raise ValueError("'donors' and 'acceptors' must hold at least one place.")
        if pairs.min() < 0 or pairs.max() >= size or places.min() < 0 or places.max() >= size:
            raise ValueError(f"The places must lie in [0, {size}), the size of a molecule.")
        place = np.arange(n_molecules * size).reshape(n_molecules, size)
        return cls(ag[place[:, pairs[:, 0]].ravel()], ag[place[:, pairs[:, 1]].ravel()], ag[place[:, places].ravel()],
                   **kwargs)

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        self.results.times = lags * df * self._dt
        # the origins of a lag: the multiples of origin_step below n_frames - lag
        self.results.n_origins = -(-np.maximum(self.n_frames - lags, 0) // self._origin_step)
        self.results.units = {"results.times": "picosecond", "results.lifetime": "picosecond",
                              "results.relaxation_time": "picosecond", "results.distance_edges": "angstrom",
                              "results.distance_bins": "angstrom", "results.angle_edges": "degree",
                              "results.angle_bins": "degree"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others (the bonds of a frame and their
        # geometry need no lag: lag 0 stands in where no lag has an origin)
        self._live = lags < self.n_frames
        engine = _core.HydrogenBondEngine(
            len(self._index), self._h_row, self._d_row, self._a_row, self._distance, self._cos_max,
            lags[self._live] if self._live.any() else np.zeros(1, dtype=np.int64), self._dimensions,
            origin_step=self._origin_step, zero_dims=zero_dims(self._drop_axis), max_neighbors=self._max_neighbors,
            continuous=self._continuous, dev=self._device)
        engine.set_bins(self._r2_thresholds, self._cos_thresholds)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        n_t = len(self._lags_run)
        counts = {key: np.zeros(n_t, dtype=np.int64) for key in ("intermittent", "continuous", "origin_counts")}
        try:
            self._batch.flush()
            if self._live.any():
                for key, value in self._engine.result().items():
                    counts[key][self._live] = value
            bonds = self._engine.bonds()
            geometry = self._engine.geometry()
            degenerate = self._engine.stats()["degenerate"]
        finally:
            self._engine.close()
        res = self.results
        res.bonds = bonds
        res.bonds_per_hydrogen = bonds / self._n_h
        res.intermittent_counts = counts["intermittent"]
        res.continuous_counts = counts["continuous"]
        res.origin_counts = counts["origin_counts"]
        norm = counts["origin_counts"].astype(float)
        norm[norm == 0] = np.nan            # no origin, or no bond at any: NaN, without a warning
        res.intermittent = counts["intermittent"] / norm
        res.continuous = counts["continuous"] / norm
        res.donated_counts = geometry["donated"]
        cases = float(geometry["donated"].sum())
        res.donated = geometry["donated"] / (cases if cases else np.nan)
        total = float(bonds.sum()) if bonds.sum() else np.nan
        res.distance_edges = self._distance_edges
        res.distance_bins = (self._distance_edges[:-1] + self._distance_edges[1:]) / 2
        res.distance_counts = geometry["distance_counts"]
        res.distance_distribution = geometry["distance_counts"] / (total * np.diff(self._distance_edges))
        res.angle_edges = self._angle_edges
        res.angle_bins = (self._angle_edges[:-1] + self._angle_edges[1:]) / 2
        res.angle_counts = geometry["cosine_counts"]
        res.angle_distribution = geometry["cosine_counts"] / (total * np.diff(self._angle_edges))
        res.degenerate = int(degenerate)

    def calculate_lifetimes(self) -> None:
        """``results.lifetime`` from ``results.continuous`` and ``results.relaxation_time`` from
        ``results.intermittent`` (``calculate_residence_time``: trapezoid integrals truncated at the last lag)."""
        if "continuous" not in self.results:
            raise RuntimeError("Call run() before calculate_lifetimes().")
        self.results.lifetime = calculate_residence_time(self.results.times, self.results.continuous)
        self.results.relaxation_time = calculate_residence_time(self.results.times, self.results.intermittent)
