"""
Real-space dynamics: ``VanHove`` — the self part of the van Hove function ``G_s(r, t)``, the distribution of
displacement magnitudes after a lag and the non-Gaussian parameter — ``calculate_non_gaussian_parameter``, and
``DistinctVanHove`` — the distinct part ``G_d(r, t)``, the time-dependent pair distribution — and ``PairResidence`` —
the intermittent and continuous survival functions of the contacts between two groups (ion-pair lifetimes, residence
times) with ``calculate_residence_time`` — and ``OrientationalRelaxation`` — the reorientation functions ``C_1(t)`` and
``C_2(t)`` of unit vectors (bonds, segments, molecular axes) and their nematic order tensor — and
``FourPointSusceptibility`` — the self-overlap function ``Q_s(t)``, its fluctuation over the time origins, the
four-point susceptibility ``chi_4(t)``, the structural relaxation time and the peak of ``chi_4`` (whether the motion
is cooperative), with ``calculate_four_point_susceptibility``.

The reference package has no counterpart; this sits next to ``IntermediateScatteringFunction(incoherent=True)``
(``F_s(q, t)``, the Fourier transform of ``G_s``) and the mean squared displacements of the correlation
engine (its second moment).

Where the work goes: whole blocks of frames go to the van Hove engine (``mdx_vh_*``), which keeps a history of
widened (and unwrapped) float64 points in HBM, bins ``|x(f) - x(f - lag)|`` for every point, lag and frame into
integer histograms and adds ``r^2`` and ``r^4`` per point in frame order.  Counts equal ``numpy.histogram``
count for count; the moments have a fixed summation order (csrc/mdx_vanhove_device.hpp).  ``DistinctVanHove``
feeds the same blocks to the distinct van Hove engine (``mdx_vhd_*``), which keeps a history of float32 frames in HBM
and bins the minimum-image distance of every pair of points for every (origin, lag) frame pair into integer
histograms (csrc/mdx_vanhove_distinct_device.hpp).  ``PairResidence`` feeds them to the pair residence engine
(``mdx_prs_*``), which keeps a history of capped per-atom contact lists in HBM and counts, per lag, the contacts of an
origin that are there again, or still (csrc/mdx_residence_device.hpp).  ``OrientationalRelaxation`` feeds the distinct
atoms of its vectors to the orientation engine (``mdx_ori_*``), which keeps a history of float64 unit vectors in HBM,
adds the first and second Legendre polynomials of ``u(f) . u(f - lag)`` per vector in frame order and the products
``u_a u_b`` of every frame per group (csrc/mdx_orient_device.hpp).  ``FourPointSusceptibility`` feeds its blocks to
the four-point engine (``mdx_chi4_*``), which keeps the van Hove engine's history of float64 points, counts per frame
pair, group and cutoff the points that moved at most the cutoff (a wave-wide count, not a per-point accumulator) and
adds that count and its square over the time origins: all integers, the same bits on every route
(csrc/mdx_chi4_device.hpp).
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import (DynamicAnalysisBase, EngineFedAnalysis, kept_components, pair_selection, parse_drop_axis,
                   parse_lags, shell_volumes, zero_dims)


def calculate_non_gaussian_parameter(m2, m4, n_dims: int = 3):
    r"""
    Non-Gaussian parameter of a displacement distribution in ``n_dims`` dimensions,

    .. math:: \alpha_2=\frac{d\,\langle\Delta r^4\rangle}{(d+2)\,\langle\Delta r^2\rangle^2}-1

    (``3 <dr^4> / (5 <dr^2>^2) - 1`` in three dimensions), which is zero for a Gaussian distribution.

    m2, m4 : float or array-like — the mean second and fourth powers of the displacement magnitude
    n_dims : int — the number of dimensions the displacements have

    Returns NaN where ``m2 == 0`` (no displacement, or no data), without a warning.
    """
    m2 = np.asarray(m2, dtype=float)
    m4 = np.asarray(m4, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = n_dims * m4 / ((n_dims + 2) * m2 ** 2) - 1
    out = np.where(m2 == 0, np.nan, out)
    return float(out) if out.ndim == 0 else out


class VanHove(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Self part of the van Hove function and the moments of the displacements,

    .. math:: G_s(r,t)=\frac1N\Big\langle\sum_i\delta\big(\mathbf r-[\mathbf r_i(t_0+t)-\mathbf r_i(t_0)]\big)
              \Big\rangle_{t_0},\qquad
              \alpha_2(t)=\frac{3\langle\Delta r^4\rangle}{5\langle\Delta r^2\rangle^2}-1

    per group, averaged over every time origin ``t_0`` of the analysed frames.

    Parameters
    ----------
    groups : AtomGroup or sequence of AtomGroups
    n_bins : int — number of histogram bins of ``|dr|``
    range : (float, float) — ``(r_min, r_max)`` of the histogram (Å), ``r_min < r_max``
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å) for ``unwrap``; defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    unwrap : bool, keyword-only — follow the particles across the periodic boundaries from frame to frame (a step
        of at least half a box length between analysed frames counts as a crossing); for wrapped trajectories
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.edges`` ``[N_b + 1]``, ``results.bins`` ``[N_b]`` (bin centres, Å), ``results.times`` ``[N_t]``
    (ps), ``results.counts`` ``[N_t, N_g, N_b]`` (int64), ``results.probability`` — the density of ``|dr|``
    (Å⁻¹), ``counts / (N_g n_origins width)``: a row integrates to the share of displacements inside the range —
    ``results.vanhove`` — ``G_s(r, t)``, ``counts / (N_g n_origins shell)`` with the volume of the spherical
    shell of the bin (Å⁻³; the area of the ring, Å⁻², with ``drop_axis``) — ``results.msd`` ``[N_t, N_g]``
    (Å²), ``results.alpha2`` ``[N_t, N_g]`` and ``results.units``.  ``n_origins = n_frames - lag``; a lag without
    an origin has zero counts and NaN in the normalised results.

    Limits: more than one rank raises ``ValueError`` (every lag needs every frame, and sharding the points would
    change the summation order); molecule centres are not supported; the frames must be evenly spaced and go
    forward in time; there is no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, groups, n_bins: int = 201, range: tuple = (0.0, 15.0), *, lags=None, n_lags: int = None,
                 dt=None, dimensions=None, drop_axis=None, unwrap: bool = False, verbose: bool = True,
                 **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "universe") else list(groups)
        self._n_groups = len(self._groups)
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("VanHove runs on one rank: every lag needs every frame, and sharding the points "
                             "would change the order of the sums.")

        self._n_bins = int(n_bins)
        if self._n_bins < 1:
            raise ValueError("'n_bins' must be at least 1.")
        r_min, r_max = (float(x) for x in strip_unit(range, "angstrom")[0])
        if not (np.isfinite(r_min) and np.isfinite(r_max) and r_min < r_max):
            raise ValueError("'range' must be an increasing pair of finite numbers.")
        self._range = (r_min, r_max)

        self._lags = parse_lags(lags, n_lags)

        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        if dimensions is not None:
            if len(dimensions) != 3:
                raise ValueError("'dimensions' must have length 3.")
            self._dimensions = np.asarray(strip_unit(dimensions, "angstrom")[0], dtype=float)
        elif self.universe.dimensions is not None:
            self._dimensions = np.asarray(self.universe.dimensions[:3], dtype=float)
        else:
            self._dimensions = None
        if unwrap and self._dimensions is None:
            raise ValueError("unwrap=True needs the box lengths: no system dimensions found or provided.")
        self._unwrap = unwrap

        self._Ns = np.fromiter((g.n_atoms for g in self._groups), dtype=int, count=self._n_groups)
        self._N = int(self._Ns.sum())
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        edges = np.linspace(*self._range, self._n_bins + 1)
        self.results.edges = edges
        self.results.bins = (edges[:-1] + edges[1:]) / 2
        self.results.times = lags * df * self._dt
        self.results.units = {"results.bins": "angstrom", "results.edges": "angstrom",
                              "results.times": "picosecond", "results.probability": "angstrom^-1",
                              "results.vanhove": "angstrom^-2" if self._drop_axis is not None else "angstrom^-3",
                              "results.msd": "angstrom^2"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others
        self._live = lags < self.n_frames
        engine = None
        if self._live.any():
            engine = _core.VanHoveEngine(self._Ns, edges, lags[self._live], zero_dims=zero_dims(self._drop_axis),
                                         dev=self._device)
            if self._unwrap:
                engine.set_unwrap(self._dimensions)
        self._feed_engine(engine, np.concatenate([np.asarray(g.indices) for g in self._groups]))

    def _conclude(self) -> None:
        self._batch.flush()
        n_t = len(self._lags_run)
        counts = np.zeros((n_t, self._n_groups, self._n_bins), dtype=np.int64)
        moments = np.zeros((n_t, self._n_groups, 2))
        if self._engine is not None:
            counts[self._live], moments[self._live] = self._engine.result()
            self._engine.close()
        edges = self.results.edges
        n_dims = 3 if self._drop_axis is None else 2
        shell = shell_volumes(edges, n_dims)
        pairs = (np.maximum(self.n_frames - self._lags_run, 0)[:, None] * self._Ns[None, :]).astype(float)
        pairs[pairs == 0] = np.nan          # no origin (or an empty group): NaN, without a warning
        self.results.counts = counts
        self.results.probability = counts / (pairs[:, :, None] * np.diff(edges))
        self.results.vanhove = counts / (pairs[:, :, None] * shell)
        self.results.msd = moments[:, :, 0] / pairs
        self.results.alpha2 = calculate_non_gaussian_parameter(self.results.msd, moments[:, :, 1] / pairs, n_dims)


class DistinctVanHove(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Distinct part of the van Hove function,

    .. math:: G_d(r,t)=\frac1{N_1}\Big\langle\sum_{i\in1}\sum_{j\in2,\,j\ne i}
              \delta\big(r-|\mathbf r_j(t_0+t)-\mathbf r_i(t_0)|\big)\Big\rangle_{t_0}

    with minimum-image distances, averaged over the time origins ``t_0`` of the analysed frames.  At ``t = 0`` it is
    ``rho g(r)``; ``G_s + G_d`` is the full van Hove function.

    Parameters
    ----------
    ag1 : AtomGroup — the points at the time origin
    ag2 : AtomGroup, optional — the points after the lag; ``None`` (or a group of the very same atoms in the same
        order): the pairs of ``ag1`` with itself, ``j != i``.  A group that shares only some atoms with ``ag1``, or
        the same atoms in another order, raises ``ValueError``
    n_bins : int — number of histogram bins of the distance
    range : (float, float) — ``(r_min, r_max)`` of the histogram (Å), ``r_min < r_max``; ``r_max`` may not exceed
        half the shortest box length that takes part
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    origin_step : int, keyword-only — every ``origin_step``-th analysed frame is a time origin
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.edges`` ``[N_b + 1]``, ``results.bins`` ``[N_b]`` (bin centres, Å), ``results.times`` ``[N_t]`` (ps),
    ``results.counts`` ``[N_t, N_b]`` (int64), ``results.n_origins`` ``[N_t]``, ``results.vanhove`` —
    ``G_d(r, t) = counts / (n_origins N_1 shell)`` with the volume of the spherical shell of the bin (Å⁻³; the area
    of the ring, Å⁻², with ``drop_axis``) — ``results.normalized`` — ``vanhove V / N_2'`` with ``N_2' = N_2 - 1``
    for one set and ``N_2`` for two, ``V`` the box volume (the area with ``drop_axis``): the normalisation of
    ``RadialDistributionFunction``'s ``"rdf"`` with ``exclusion=(1, 1)``, so lag 0 is ``g(r)`` — and
    ``results.units``.  A lag without an origin has zero counts and NaN in the normalised results.

    Limits: the box is orthorhombic and taken as constant (``dimensions``, or else the universe's box): NPT
    trajectories are outside the contract.  The coordinates are used as given; no unwrap is needed, because the
    minimum image of a difference does not depend on the periodic images.  More than one rank raises ``ValueError``;
    molecule centres are not supported; the frames must be evenly spaced and go forward in time; every pair of points
    is evaluated (no cell list); there is no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, ag1, ag2=None, n_bins: int = 201, range: tuple = (0.0, 15.0), *, lags=None,
                 n_lags: int = None, origin_step: int = 1, dt=None, dimensions=None, drop_axis=None,
                 verbose: bool = True, **kwargs) -> None:
        self.universe = ag1.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("DistinctVanHove runs on one rank: every lag needs every frame.")

        self._n_bins = int(n_bins)
        if self._n_bins < 1:
            raise ValueError("'n_bins' must be at least 1.")
        r_min, r_max = (float(x) for x in strip_unit(range, "angstrom")[0])
        if not (np.isfinite(r_min) and np.isfinite(r_max) and r_min < r_max):
            raise ValueError("'range' must be an increasing pair of finite numbers.")
        self._range = (r_min, r_max)

        self._lags = parse_lags(lags, n_lags)
        self._origin_step = int(origin_step)
        if self._origin_step < 1:
            raise ValueError("'origin_step' must be at least 1.")

        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, r_max, "range")

        self._same, self._N1, self._N2, self._index = pair_selection(ag1, ag2)
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        edges = np.linspace(*self._range, self._n_bins + 1)
        self.results.edges = edges
        self.results.bins = (edges[:-1] + edges[1:]) / 2
        self.results.times = lags * df * self._dt
        # the origins of a lag: the multiples of origin_step below n_frames - lag
        self.results.n_origins = -(-np.maximum(self.n_frames - lags, 0) // self._origin_step)
        per = "angstrom^-2" if self._drop_axis is not None else "angstrom^-3"
        self.results.units = {"results.bins": "angstrom", "results.edges": "angstrom",
                              "results.times": "picosecond", "results.vanhove": per}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others
        self._live = lags < self.n_frames
        engine = None
        if self._live.any():
            engine = _core.DistinctVanHoveEngine(
                self._N1, self._N2, edges, lags[self._live], self._dimensions, same=self._same,
                origin_step=self._origin_step, zero_dims=zero_dims(self._drop_axis), dev=self._device)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        self._batch.flush()
        counts = np.zeros((len(self._lags_run), self._n_bins), dtype=np.int64)
        if self._engine is not None:
            counts[self._live] = self._engine.result()
            self._engine.close()
        edges = self.results.edges
        kept = kept_components(self._drop_axis)
        shell = shell_volumes(edges, len(kept))
        origins = self.results.n_origins.astype(float)
        origins[origins == 0] = np.nan          # no origin: NaN, without a warning
        partners = self._N2 - 1 if self._same else self._N2
        self.results.counts = counts
        self.results.vanhove = counts / (origins[:, None] * self._N1 * shell)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.results.normalized = self.results.vanhove * np.prod(self._dimensions[kept]) / partners


def calculate_residence_time(times, survival):
    r"""
    Residence time of a survival function as its time integral,

    .. math:: \tau=\int_0^{t_\mathrm{max}}S(t)\,\mathrm dt

    by the trapezoid rule over the finite leading part of ``survival`` (the values before the first NaN or
    infinity).  The integral is truncated at the last lag: it is the residence time only where ``survival`` has
    decayed to about zero by then, and a lower bound otherwise.

    times : array-like ``[N_t]`` — the lag times, increasing
    survival : array-like ``[N_t]`` — the survival function at those times (``results.continuous`` or
        ``results.intermittent`` of ``PairResidence``)

    Returns NaN where not even the first value is finite.
    """
    t = np.asarray(times, dtype=float)
    s = np.asarray(survival, dtype=float)
    if t.ndim != 1 or t.shape != s.shape:
        raise ValueError("'times' and 'survival' must be one-dimensional and of one length.")
    bad = np.flatnonzero(~np.isfinite(s))
    n = bad[0] if len(bad) else len(s)
    if n == 0:
        return float("nan")
    return float(((s[1:n] + s[:n - 1]) * np.diff(t[:n])).sum() / 2)


class PairResidence(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Survival functions of the contacts between two groups: with :math:`h_{ij}(t)=1` where the minimum-image distance
    of :math:`i\in1` and :math:`j\in2` is at most ``cutoff`` (:math:`j\ne i` for one set) and 0 otherwise,

    .. math:: C_\mathrm{int}(t)=\frac{\langle\sum_{ij}h_{ij}(t_0)\,h_{ij}(t_0+t)\rangle_{t_0}}
              {\langle\sum_{ij}h_{ij}(t_0)\rangle_{t_0}},\qquad
              C_\mathrm{cont}(t)=\frac{\langle\sum_{ij}\prod_{t'=t_0}^{t_0+t}h_{ij}(t')\rangle_{t_0}}
              {\langle\sum_{ij}h_{ij}(t_0)\rangle_{t_0}}

    the intermittent function (the pair is together again, or still, after ``t``) and the continuous one (the pair
    has not parted in any analysed frame up to ``t``), averaged over the time origins ``t_0`` of the analysed frames:
    ion-pair lifetimes, residence times of ions at polymer sites.

    Parameters
    ----------
    ag1 : AtomGroup — the rows of the contact lists (the averages are per atom of ``ag1``)
    ag2 : AtomGroup, optional — the partners; ``None`` (or a group of the very same atoms in the same order): the
        pairs of ``ag1`` with itself, ``j != i``, both ``(i, j)`` and ``(j, i)``.  A group that shares only some atoms
        with ``ag1``, or the same atoms in another order, raises ``ValueError``
    cutoff : float — the contact distance (Å), positive; it may not exceed half the shortest box length that takes
        part
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    origin_step : int, keyword-only — every ``origin_step``-th analysed frame is a time origin
    max_neighbors : int, keyword-only — the contacts an atom of ``ag1`` may have in one frame (1 ... 64).  A frame
        with more raises ``ValueError`` at the end of ``run()``: nothing is truncated silently
    continuous : bool, keyword-only — ``False`` skips the frames between the lags: ``results.continuous_counts`` is
        then zero
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å); defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.times`` ``[N_t]`` (ps), ``results.n_origins`` ``[N_t]``, ``results.contacts`` ``[N_f]`` (int64, the
    contacts of every analysed frame), ``results.coordination`` — ``contacts / N_1`` — ``results.intermittent_counts``,
    ``results.continuous_counts`` and ``results.origin_counts`` ``[N_t]`` (int64), ``results.intermittent`` and
    ``results.continuous`` — the counts over ``origin_counts``, NaN without a warning where that is 0 (a lag without
    an origin, or no contact at any origin) — and ``results.units``.  ``calculate_residence_times()`` adds
    ``results.residence_time`` and ``results.relaxation_time``.

    Limits: as ``DistinctVanHove`` — a constant orthorhombic box, coordinates as given, one rank, no molecule
    centres, evenly spaced frames forward in time, every pair of points evaluated (no cell list), no CPU fallback:
    without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, ag1, ag2=None, cutoff: float = None, *, lags=None, n_lags: int = None, origin_step: int = 1,
                 max_neighbors: int = 32, continuous: bool = True, dt=None, dimensions=None, drop_axis=None,
                 verbose: bool = True, **kwargs) -> None:
        self.universe = ag1.universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("PairResidence runs on one rank: every lag needs every frame.")

        if cutoff is None:
            raise ValueError("'cutoff' must be given.")
        self._cutoff = float(strip_unit(cutoff, "angstrom")[0])
        if not (np.isfinite(self._cutoff) and self._cutoff > 0):
            raise ValueError("'cutoff' must be positive and finite.")

        self._lags = parse_lags(lags, n_lags)
        self._origin_step = int(origin_step)
        if self._origin_step < 1:
            raise ValueError("'origin_step' must be at least 1.")
        self._max_neighbors = int(max_neighbors)
        if not 1 <= self._max_neighbors <= _core.PairResidenceEngine.MAX_NEIGHBORS:
            raise ValueError(f"'max_neighbors' must lie in [1, {_core.PairResidenceEngine.MAX_NEIGHBORS}].")
        self._continuous = bool(continuous)

        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, self._cutoff, "cutoff")

        self._same, self._N1, self._N2, self._index = pair_selection(ag1, ag2)
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        self.results.times = lags * df * self._dt
        # the origins of a lag: the multiples of origin_step below n_frames - lag
        self.results.n_origins = -(-np.maximum(self.n_frames - lags, 0) // self._origin_step)
        self.results.units = {"results.times": "picosecond", "results.residence_time": "picosecond",
                              "results.relaxation_time": "picosecond"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others
        self._live = lags < self.n_frames
        engine = None
        if self._live.any():
            engine = _core.PairResidenceEngine(
                self._N1, self._N2, self._cutoff, lags[self._live], self._dimensions, same=self._same,
                origin_step=self._origin_step, zero_dims=zero_dims(self._drop_axis),
                max_neighbors=self._max_neighbors, continuous=self._continuous, dev=self._device)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        self._batch.flush()
        n_t = len(self._lags_run)
        counts = {key: np.zeros(n_t, dtype=np.int64) for key in ("intermittent", "continuous", "origin_counts")}
        contacts = np.zeros(0, dtype=np.int64)
        if self._engine is not None:
            try:
                for key, value in self._engine.result().items():
                    counts[key][self._live] = value
                contacts = self._engine.contacts()
            finally:
                self._engine.close()
        self.results.contacts = contacts
        self.results.coordination = contacts / self._N1
        self.results.intermittent_counts = counts["intermittent"]
        self.results.continuous_counts = counts["continuous"]
        self.results.origin_counts = counts["origin_counts"]
        norm = counts["origin_counts"].astype(float)
        norm[norm == 0] = np.nan            # no origin, or no contact at any: NaN, without a warning
        self.results.intermittent = counts["intermittent"] / norm
        self.results.continuous = counts["continuous"] / norm

    def calculate_residence_times(self) -> None:
        """``results.residence_time`` from ``results.continuous`` and ``results.relaxation_time`` from
        ``results.intermittent`` (``calculate_residence_time``: trapezoid integrals truncated at the last lag)."""
        if "continuous" not in self.results:
            raise RuntimeError("Call run() before calculate_residence_times().")
        self.results.residence_time = calculate_residence_time(self.results.times, self.results.continuous)
        self.results.relaxation_time = calculate_residence_time(self.results.times, self.results.intermittent)


class OrientationalRelaxation(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Reorientation of unit vectors (bonds, chain segments, molecular axes): with :math:`\mathbf u_v(t)` the unit
    vector from ``tails[v]`` to ``heads[v]``,

    .. math:: C_1(t)=\big\langle\mathbf u_v(t_0+t)\cdot\mathbf u_v(t_0)\big\rangle_{v,t_0},\qquad
              C_2(t)=\big\langle\tfrac32\,[\mathbf u_v(t_0+t)\cdot\mathbf u_v(t_0)]^2-\tfrac12\big\rangle_{v,t_0}

    per group of vectors, averaged over every time origin ``t_0`` of the analysed frames — the first and second
    Legendre polynomials of the angle a vector turns through in ``t``, the quantities behind dielectric (``C_1``) and
    NMR / depolarised light scattering (``C_2``) relaxation times — and per frame the nematic order tensor

    .. math:: \mathbf Q=\tfrac32\,\langle\mathbf u\,\mathbf u^{\mathsf T}\rangle_v-\tfrac12\,\mathbf I

    with its largest eigenvalue (the order parameter ``S``) and the eigenvector that goes with it (the director).

    Parameters
    ----------
    tails, heads : AtomGroup, or two equally long sequences of AtomGroups — vector ``v`` of a group points from
        ``tails[v]`` to ``heads[v]``; the two groups must be of one length, and no vector may start where it ends.  An
        atom may sit in many vectors (the bonds along a chain): every distinct atom is read once per frame
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å) for the minimum image; defaults to the universe's
    minimum_image : bool, keyword-only — take ``head - tail`` as its minimum image in one constant orthorhombic box
        (wrapped trajectories); ``False`` needs no box and suits molecules that are whole already
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part: the vectors are the unit
        vectors of the projections onto the remaining plane
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.times`` ``[N_t]`` (ps), ``results.c1`` and ``results.c2`` ``[N_t, N_g]`` — the engine's sums over
    ``n_origins V_g`` with ``n_origins = n_frames - lag``; NaN without a warning for a lag without an origin or an empty
    group — ``results.order_tensor`` ``[N_f, N_g, 3, 3]``, ``results.order_parameter`` ``[N_f, N_g]`` (the largest
    eigenvalue of ``Q``, ``numpy.linalg.eigvalsh``), ``results.director`` ``[N_f, N_g, 3]`` (a unit vector; its sign
    means nothing) and ``results.units``.  With ``drop_axis`` the tensor is the two-dimensional form
    ``Q = 2 <u u^T> - I`` on the kept components (its eigenvalues are ``+S`` and ``-S``); the row and the column of
    the dropped component are zero, and so is that component of the director.  ``calculate_relaxation_times()`` adds
    ``results.relaxation_times``.

    Limits: the box is orthorhombic and taken as constant (``dimensions``, or else the universe's box): NPT
    trajectories are outside the contract.  A vector whose head lies on its tail in some frame has no direction:
    ``run()`` then raises ``ValueError`` instead of averaging it.  More than one rank raises ``ValueError``; the
    frames must be evenly spaced and go forward in time; there is no CPU fallback: without a HIP device ``run()``
    raises ``RuntimeError``.
    """

    _shard_frames = False

    def __init__(self, tails, heads, *, lags=None, n_lags: int = None, dt=None, dimensions=None,
                 minimum_image: bool = True, drop_axis=None, verbose: bool = True, **kwargs) -> None:
        tails = [tails] if hasattr(tails, "universe") else list(tails)
        heads = [heads] if hasattr(heads, "universe") else list(heads)
        if len(tails) != len(heads) or len(tails) == 0:
            raise ValueError("'tails' and 'heads' must hold the same number of groups, at least one.")
        self._n_groups = len(tails)
        self.universe = tails[0].universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("OrientationalRelaxation runs on one rank: every lag needs every frame, and sharding "
                             "the vectors would change the order of the sums.")

        for g, (t, h) in enumerate(zip(tails, heads)):
            if t.n_atoms != h.n_atoms:
                raise ValueError(f"group {g}: 'tails' holds {t.n_atoms} atoms and 'heads' {h.n_atoms}: a vector "
                                 "needs one of each.")
            if np.any(np.asarray(t.indices) == np.asarray(h.indices)):
                raise ValueError(f"group {g}: a vector starts and ends on the same atom.")
        self._Ns = np.fromiter((t.n_atoms for t in tails), dtype=int, count=self._n_groups)
        self._V = int(self._Ns.sum())
        if self._V < 1:
            raise ValueError("The groups must hold at least one vector.")
        # the distinct atoms are fed once; the pairs name them by their place in that feed
        atoms = np.concatenate([np.asarray(t.indices) for t in tails] + [np.asarray(h.indices) for h in heads])
        self._index, inverse = np.unique(atoms, return_inverse=True)
        self._pairs = np.stack((inverse[:self._V], inverse[self._V:]), axis=1).astype(np.int32)

        self._lags = parse_lags(lags, n_lags)
        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        self._dimensions = self._box_lengths(dimensions, 0.0, "minimum_image") if minimum_image else None
        self._verbose = verbose

    @classmethod
    def from_chains(cls, ag, n_chains: int, n_monomers: int, *, stride: int = 1, **kwargs):
        """The polymer case: ``ag`` holds ``n_chains`` chains of ``n_monomers`` consecutive atoms each, and the
        vectors go from monomer ``n`` to monomer ``n + stride`` of every chain, ``n = 0 ... n_monomers - stride - 1``,
        in one group (``stride=1``: the bonds)."""
        n_chains, n_monomers, stride = int(n_chains), int(n_monomers), int(stride)
        if n_chains < 1 or n_monomers < 2 or ag.n_atoms != n_chains * n_monomers:
            raise ValueError("'ag' must hold n_chains * n_monomers atoms, n_monomers >= 2.")
        if not 1 <= stride < n_monomers:
            raise ValueError("'stride' must lie in [1, n_monomers).")
        place = np.arange(n_chains * n_monomers).reshape(n_chains, n_monomers)
        return cls(ag[place[:, :-stride].ravel()], ag[place[:, stride:].ravel()], **kwargs)

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        self.results.times = lags * df * self._dt
        self.results.units = {"results.times": "picosecond", "results.relaxation_times": "picosecond"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others
        self._live = lags < self.n_frames
        engine = None
        if self._live.any():
            engine = _core.OrientationEngine(self._Ns, self._pairs, len(self._index), lags[self._live],
                                             zero_dims=zero_dims(self._drop_axis), dev=self._device)
            if self._dimensions is not None:
                engine.set_box(self._dimensions)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        self._batch.flush()
        sums = np.zeros((len(self._lags_run), self._n_groups, 2))
        products = np.full((self.n_frames, self._n_groups, 6), np.nan)     # no lag with an origin: no engine ran
        if self._engine is not None:
            try:
                sums[self._live] = self._engine.result()
                products = self._engine.frame_sums()
            finally:
                self._engine.close()
        terms = (np.maximum(self.n_frames - self._lags_run, 0)[:, None] * self._Ns[None, :]).astype(float)
        terms[terms == 0] = np.nan          # no origin (or an empty group): NaN, without a warning
        self.results.c1 = sums[:, :, 0] / terms
        self.results.c2 = sums[:, :, 1] / terms

        kept = kept_components(self._drop_axis)
        filled = self._Ns > 0
        mean = np.full((len(products), self._n_groups, 3, 3), np.nan)
        for q, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            mean[:, filled, a, b] = mean[:, filled, b, a] = products[:, filled, q] / self._Ns[filled]
        tensor = np.zeros_like(mean)
        block = np.ix_(kept, kept)
        if len(kept) == 3:
            tensor = 1.5 * mean - 0.5 * np.eye(3)
        else:
            tensor[(..., *block)] = 2.0 * mean[(..., *block)] - np.eye(2)
            tensor[:, ~filled] = np.nan
        order = np.full(mean.shape[:2], np.nan)
        director = np.full(mean.shape[:2] + (3,), np.nan)
        if filled.any() and len(products) and self._engine is not None:
            q_kept = tensor[:, filled][(..., *block)]
            order[:, filled] = np.linalg.eigvalsh(q_kept)[..., -1]
            axis = np.zeros(q_kept.shape[:2] + (3,))
            axis[..., kept] = np.linalg.eigh(q_kept)[1][..., -1]
            director[:, filled] = axis
        self.results.order_tensor = tensor
        self.results.order_parameter = order
        self.results.director = director

    def calculate_relaxation_times(self) -> None:
        r"""``results.relaxation_times`` ``[2, N_g]``: :math:`\tau_l=\int_0^{t_\mathrm{max}}C_l(t)\,\mathrm dt` of
        ``results.c1`` (row 0) and ``results.c2`` (row 1) for every group (``calculate_residence_time``: the trapezoid
        rule).  The integral is truncated at the last lag: it is the relaxation time only where ``C_l`` has decayed
        to about zero by then, and a lower bound otherwise.  In a nematic sample ``C_2`` does not decay to 0: it
        levels off near ``<S>^2``, the square of ``results.order_parameter``, so read its long-time value against
        that plateau before trusting ``tau_2``."""
        if "c1" not in self.results:
            raise RuntimeError("Call run() before calculate_relaxation_times().")
        self.results.relaxation_times = np.array(
            [[calculate_residence_time(self.results.times, c[:, g]) for g in range(self._n_groups)]
             for c in (self.results.c1, self.results.c2)])


def _exact_integers(a, name: str) -> np.ndarray:
    """``a`` as an object array of Python ints."""
    a = np.asarray(a)
    if a.dtype != object and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"'{name}' must hold integers.")
    return a.astype(object)


def calculate_four_point_susceptibility(sums, square_sums, n_origins, n_points):
    r"""
    Four-point susceptibility from the sums of the overlap ``Q`` and of its square over ``n`` time origins,

    .. math:: \chi_4=N\big(\langle q^2\rangle-\langle q\rangle^2\big)=\frac{n\,S_2-S_1^2}{n^2N},\qquad q=Q/N

    the population variance of ``q`` over the origins times the number of points ``N``.  ``n S_2 - S_1^2`` is formed
    in exact integer arithmetic (Python ints) and divided only after that: both terms are of order ``10^18`` and more
    for a long trajectory of a large group, and a float64 difference of them is noise.

    sums, square_sums : integer array-like — ``S_1`` and ``S_2``; ``[N_t, N_g, N_a]`` as in
        ``FourPointSusceptibility.results``, or anything that broadcasts with the two below
    n_origins : integer array-like — the origins; ``[N_t]`` for three-dimensional sums
    n_points : integer array-like — the points of the groups; ``[N_g]`` for three-dimensional sums

    Returns float64 of the broadcast shape (a float for scalars): NaN without a warning where ``n_origins`` or
    ``n_points`` is 0.
    """
    s1, s2 = _exact_integers(sums, "sums"), _exact_integers(square_sums, "square_sums")
    n, size = _exact_integers(n_origins, "n_origins"), _exact_integers(n_points, "n_points")
    if s1.ndim == 3 and n.ndim == 1 and size.ndim <= 1:
        n = n.reshape(-1, 1, 1)
        size = size.reshape(1, -1, 1)
    numerator = n * s2 - s1 * s1
    denominator = n * n * size
    ratio = np.frompyfunc(lambda a, b: a / b if b else float("nan"), 2, 1)     # int / int: correctly rounded
    out = np.asarray(ratio(numerator, denominator), dtype=float)
    return float(out) if out.ndim == 0 else out


class FourPointSusceptibility(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Self-overlap function and four-point susceptibility: with
    :math:`Q(t_0,t)=\sum_i\Theta\big(a-|\mathbf r_i(t_0+t)-\mathbf r_i(t_0)|\big)` the number of points of a group
    that moved at most ``a`` in ``t``,

    .. math:: Q_s(t)=\frac{\langle Q\rangle_{t_0}}N,\qquad
              \chi_4(t)=\frac{\langle Q^2\rangle_{t_0}-\langle Q\rangle_{t_0}^2}N

    per group and cutoff ``a``, over the time origins ``t_0`` of the analysed frames.  ``Q_s`` falls to ``1/e`` at the
    structural relaxation time :math:`\tau_\alpha`; ``chi_4`` measures how cooperative the motion is: its peak height
    gives the size of the dynamically correlated regions and the peak time their lifetime.

    Parameters
    ----------
    groups : AtomGroup or sequence of AtomGroups
    cutoffs : float or sequence of up to 8 floats — the overlap lengths ``a`` (Å), not negative, strictly increasing;
        a displacement of exactly ``a`` counts
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    origin_step : int, keyword-only — every ``origin_step``-th analysed frame is a time origin
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å) for ``unwrap``; defaults to the universe's
    drop_axis : {0, 1, 2, "x", "y", "z"}, keyword-only — a component that takes no part (slabs, 2-D systems)
    unwrap : bool, keyword-only — follow the particles across the periodic boundaries from frame to frame (a step
        of at least half a box length between analysed frames counts as a crossing); for wrapped trajectories
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.times`` ``[N_t]`` (ps), ``results.cutoffs`` ``[N_a]`` (Å), ``results.n_origins`` ``[N_t]``,
    ``results.sums`` and ``results.square_sums`` ``[N_t, N_g, N_a]`` (int64, the sums of ``Q`` and of ``Q^2`` over the
    origins), ``results.overlap`` — ``sums / (n_origins N_g)`` — ``results.chi4`` —
    ``calculate_four_point_susceptibility``: ``N_g`` times the population variance of ``Q / N_g`` over the origins —
    and ``results.units``.  A lag without an origin and an empty group give NaN without a warning.
    ``calculate_relaxation_times()`` adds ``results.relaxation_time``, ``results.peak_time`` and
    ``results.peak_height``.

    Limits: ``chi_4`` is the variance over the time origins of one trajectory in its own ensemble (the constraints of
    the simulation suppress a part of the fluctuations), and neighbouring origins are correlated: it needs many more
    frames than ``Q_s``.  More than one rank raises ``ValueError``; molecule centres are not supported; the frames
    must be evenly spaced and go forward in time; there is no CPU fallback: without a HIP device ``run()`` raises
    ``RuntimeError``.
    """

    def __init__(self, groups, cutoffs, *, lags=None, n_lags: int = None, origin_step: int = 1, dt=None,
                 dimensions=None, drop_axis=None, unwrap: bool = False, verbose: bool = True, **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "universe") else list(groups)
        self._n_groups = len(self._groups)
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("FourPointSusceptibility runs on one rank: every lag needs every frame, and the overlap "
                             "of a frame pair needs every point.")

        a = np.atleast_1d(np.asarray(strip_unit(cutoffs, "angstrom")[0], dtype=float))
        if a.ndim != 1 or not 1 <= len(a) <= _core.FourPointEngine.MAX_CUTOFFS:
            raise ValueError(f"'cutoffs' must hold 1 to {_core.FourPointEngine.MAX_CUTOFFS} cutoffs.")
        if not np.all(np.isfinite(a)) or a[0] < 0 or np.any(np.diff(a) <= 0):
            raise ValueError("'cutoffs' must be finite, non-negative and strictly increasing.")
        self._cutoffs = a

        self._lags = parse_lags(lags, n_lags)
        self._origin_step = int(origin_step)
        if self._origin_step < 1:
            raise ValueError("'origin_step' must be at least 1.")

        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = parse_drop_axis(drop_axis)
        if dimensions is not None:
            if len(dimensions) != 3:
                raise ValueError("'dimensions' must have length 3.")
            self._dimensions = np.asarray(strip_unit(dimensions, "angstrom")[0], dtype=float)
        elif self.universe.dimensions is not None:
            self._dimensions = np.asarray(self.universe.dimensions[:3], dtype=float)
        else:
            self._dimensions = None
        if unwrap and self._dimensions is None:
            raise ValueError("unwrap=True needs the box lengths: no system dimensions found or provided.")
        self._unwrap = unwrap

        self._Ns = np.fromiter((g.n_atoms for g in self._groups), dtype=int, count=self._n_groups)
        self._N = int(self._Ns.sum())
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        self.results.times = lags * df * self._dt
        self.results.cutoffs = self._cutoffs.copy()
        # the origins of a lag: the multiples of origin_step below n_frames - lag
        self.results.n_origins = -(-np.maximum(self.n_frames - lags, 0) // self._origin_step)
        self.results.units = {"results.times": "picosecond", "results.cutoffs": "angstrom",
                              "results.relaxation_time": "picosecond", "results.peak_time": "picosecond"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others
        self._live = lags < self.n_frames
        engine = None
        if self._live.any():
            engine = _core.FourPointEngine(self._Ns, self._cutoffs, lags[self._live], origin_step=self._origin_step,
                                           zero_dims=zero_dims(self._drop_axis), dev=self._device)
            if self._unwrap:
                engine.set_unwrap(self._dimensions)
        self._feed_engine(engine, np.concatenate([np.asarray(g.indices) for g in self._groups]))

    def _conclude(self) -> None:
        self._batch.flush()
        shape = (len(self._lags_run), self._n_groups, len(self._cutoffs))
        sums, square_sums = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        if self._engine is not None:
            try:
                sums[self._live], square_sums[self._live], _ = self._engine.result()      # n_origins: as _prepare's
            finally:
                self._engine.close()
        terms = (self.results.n_origins[:, None] * self._Ns[None, :]).astype(float)
        terms[terms == 0] = np.nan          # no origin (or an empty group): NaN, without a warning
        self.results.sums = sums
        self.results.square_sums = square_sums
        self.results.overlap = sums / terms[:, :, None]
        self.results.chi4 = calculate_four_point_susceptibility(sums, square_sums, self.results.n_origins, self._Ns)

    def calculate_relaxation_times(self) -> None:
        """``results.relaxation_time`` ``[N_g, N_a]``: the time where ``results.overlap`` first falls to ``1/e``, by
        linear interpolation between the two lags that bracket the crossing; NaN where it is not bracketed (the
        overlap never falls that far, is there already at the first lag, or the lag before the crossing has no
        value).  ``results.peak_time`` and ``results.peak_height`` ``[N_g, N_a]``: the largest finite value of
        ``results.chi4`` and its time (the first one, if several lags share it); NaN where there is none.  A peak
        at the last lag means that ``chi_4`` may still be rising there."""
        if "overlap" not in self.results:
            raise RuntimeError("Call run() before calculate_relaxation_times().")
        times = np.asarray(self.results.times, dtype=float)
        overlap = np.asarray(self.results.overlap, dtype=float)
        chi4 = np.asarray(self.results.chi4, dtype=float)
        level = np.exp(-1.0)
        tau = np.full(overlap.shape[1:], np.nan)
        for g, c in np.ndindex(*tau.shape):
            q = overlap[:, g, c]
            below = np.flatnonzero(q <= level)              # a NaN is not below
            if len(below) == 0 or below[0] == 0:
                continue
            i = below[0]
            if not q[i - 1] > level:                        # NaN before the crossing
                continue
            tau[g, c] = times[i - 1] + (q[i - 1] - level) / (q[i - 1] - q[i]) * (times[i] - times[i - 1])
        finite = np.isfinite(chi4)
        best = np.where(finite, chi4, -np.inf).argmax(axis=0) if len(chi4) else np.zeros(chi4.shape[1:], dtype=int)
        some = finite.any(axis=0)
        height = np.take_along_axis(chi4, best[None], axis=0)[0] if len(chi4) else np.full(chi4.shape[1:], np.nan)
        self.results.relaxation_time = tau
        self.results.peak_time = np.where(some, times[best] if len(times) else np.nan, np.nan)
        self.results.peak_height = np.where(some, height, np.nan)
