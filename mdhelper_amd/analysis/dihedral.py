"""
Dihedrals: ``Dihedrals`` — the distribution of torsion angles, the populations of the conformer states (trans, gauche+,
gauche-), the torsional autocorrelation function, how long a conformer lives and how often it jumps.

Whole blocks of frames go to the dihedral engine (``mdx_dih_*``), which forms the cosine and the sine of every torsion
angle in float64 (minimum image of the three bond vectors), bins the angle by thresholds of the cosine and the sign of
the sine (no ``acos`` or ``atan2``), maps the bin to a state, keeps cosine, sine, state and the run length of the state
in rings of frames in HBM and walks the lags over them (csrc/mdx_dihedral_device.hpp).  Every lag needs every frame,
so the class runs on one rank.
"""

from __future__ import annotations

import numpy as np

from .. import _core, _lib
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, parse_lags
from .dynamics import calculate_residence_time

_GAS_CONSTANT = 8.31446261815324e-3     # kJ / (mol K)


def cosine_thresholds(n_bins: int) -> np.ndarray:
    """The thresholds of ``cos(phi)`` that bin ``|phi|`` into ``n_bins / 2`` bins of equal width over [0, 180]
    degrees: ``t[m] = cos(m pi / n_half)`` with ``t[0] = 1`` and ``t[n_half] = -1`` exactly."""
    n_half = int(n_bins) // 2
    t = np.cos(np.arange(n_half + 1) * np.pi / n_half)
    t[0], t[n_half] = 1.0, -1.0
    return t


def states_of_bins(n_bins: int, state_edges) -> np.ndarray:
    """``int32 [n_bins]``: the state of every bin of width ``360 / n_bins`` degrees from -180 on.  ``state_edges``:
    ascending boundaries in degrees within [-180, 180), each on a bin edge; state ``j`` is ``[e_j, e_{j + 1})`` and
    the last state wraps through +-180."""
    edges = np.atleast_1d(np.asarray(state_edges, dtype=float))
    if edges.ndim != 1 or not 1 <= len(edges) <= _core.DihedralEngine.MAX_STATES:
        raise ValueError(f"'state_edges' must hold 1 to {_core.DihedralEngine.MAX_STATES} boundaries.")
    if not np.all(np.isfinite(edges)) or edges[0] < -180.0 or edges[-1] >= 180.0 or np.any(np.diff(edges) <= 0):
        raise ValueError("'state_edges' must be ascending and lie in [-180, 180) degrees.")
    place = (edges + 180.0) * n_bins / 360.0
    if np.any(np.abs(place - np.rint(place)) > 1e-9 * n_bins):
        raise ValueError(f"Every boundary of 'state_edges' must fall on a bin edge (a multiple of {360.0 / n_bins:g} "
                         "degrees from -180).")
    first = np.rint(place).astype(int)
    return ((np.searchsorted(first, np.arange(n_bins), side="right") - 1) % len(edges)).astype(np.int32)


class Dihedrals(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Torsion angles :math:`\varphi` of four atoms ``first``–``second``–``third``–``fourth`` (IUPAC sign, trans at
    :math:`\pm180^\circ`): their distribution per group, the populations of the conformer states the angle range is
    cut into, the transitions between the states from one analysed frame to the next, the torsional autocorrelation
    function

    .. math:: C_\varphi(t)=\big\langle\cos[\varphi_v(t_0+t)-\varphi_v(t_0)]\big\rangle_{v,t_0}

    and the two lifetime functions of a state: the intermittent one (the dihedral is in the state of ``t_0`` again, or
    still, after ``t``) and the continuous one (it has not left that state in any analysed frame up to ``t``).

    Parameters
    ----------
    first, second, third, fourth : AtomGroup, or four equally long sequences of AtomGroups — dihedral ``v`` of a group
        is ``first[v]``, ``second[v]``, ``third[v]``, ``fourth[v]``; the four groups must be of one length and the four
        atoms of a dihedral distinct.  An atom may sit in many dihedrals: every distinct atom is read once per frame
    n_bins : int, keyword-only — bins of equal width over [-180, 180) degrees, even
    state_edges : array-like, keyword-only — ascending boundaries in degrees within [-180, 180), each on a bin edge;
        state ``j`` is ``[e_j, e_{j+1})`` and the last state wraps through ±180.  The default gives gauche−
        ``[-120, 0)``, gauche+ ``[0, 120)`` and trans
    lags : array-like of int, keyword-only — lag times in frames of the analysed selection, strictly increasing,
        non-negative
    n_lags : int, keyword-only — shorthand for ``lags=arange(n_lags)``; with neither, every analysed frame is a lag
    dt : float, keyword-only — time between trajectory frames (ps); defaults to the trajectory's
    dimensions : array-like ``(3,)``, keyword-only — box lengths (Å) for the minimum image; defaults to the universe's
    minimum_image : bool, keyword-only — take the bond vectors as minimum images in one constant orthorhombic box
        (wrapped trajectories); ``False`` needs no box and suits molecules that are whole already
    verbose : bool
    device : keyword-only — the HIP device

    Results
    -------
    ``results.edges`` ``[n_bins + 1]`` and ``results.angles`` ``[n_bins]`` (degrees), ``results.counts``
    ``[N_g, n_bins]`` (int64), ``results.distribution`` (per degree, integrates to 1; NaN for an empty group),
    ``results.populations`` ``[N_g, S]`` (sum to 1), ``results.state_counts`` ``[N_f, N_g, S]`` and
    ``results.transitions`` ``[N_g, S, S]`` (int64; row ``s0``, column ``s1``, the diagonal included),
    ``results.times`` ``[N_t]`` (ps), ``results.tacf``, ``results.intermittent`` and ``results.continuous``
    ``[N_t, N_g]`` — the engine's sums over ``n_origins D_g`` with ``n_origins = n_frames - lag``; NaN without a
    warning for a lag without an origin or an empty group — and ``results.units``.
    ``calculate_relaxation_times()``, ``calculate_transition_rates()`` and ``calculate_pmf(temperature)`` add
    ``results.relaxation_times``, ``results.transition_rates`` and ``results.pmf``.

    Limits: the box is orthorhombic and taken as constant (``dimensions``, or else the universe's box): NPT
    trajectories are outside the contract.  A dihedral with three atoms on a line or two on one point in some frame
    has no angle: ``run()`` then raises ``ValueError`` instead of averaging it.  Improper dihedrals get no convention
    of their own.  Every analysed frame is a time origin.  More than one rank raises ``ValueError``; the frames must be
    evenly spaced and go forward in time; there is no CPU fallback: without a HIP device ``run()`` raises
    ``RuntimeError``.
    """

    _shard_frames = False

    def __init__(self, first, second, third, fourth, *, n_bins: int = 180, state_edges=(-120.0, 0.0, 120.0),
                 lags=None, n_lags: int = None, dt=None, dimensions=None, minimum_image: bool = True,
                 verbose: bool = True, **kwargs) -> None:
        legs = [[leg] if hasattr(leg, "universe") else list(leg) for leg in (first, second, third, fourth)]
        if len({len(leg) for leg in legs}) != 1 or len(legs[0]) == 0:
            raise ValueError("'first', 'second', 'third' and 'fourth' must hold the same number of groups, at least "
                             "one.")
        self._n_groups = len(legs[0])
        self.universe = legs[0][0].universe
        super().__init__(self.universe.trajectory, False, verbose, **kwargs)
        if self._comm.world_size > 1:
            raise ValueError("Dihedrals runs on one rank: every lag needs every frame, and sharding the dihedrals "
                             "would change the order of the sums.")

        for g in range(self._n_groups):
            sizes = [leg[g].n_atoms for leg in legs]
            if len(set(sizes)) != 1:
                raise ValueError(f"group {g}: the four groups hold {sizes} atoms: a dihedral needs one of each.")
            atoms = np.stack([np.asarray(leg[g].indices) for leg in legs], axis=1)
            if len(atoms) and np.any(np.sort(atoms, axis=1)[:, 1:] == np.sort(atoms, axis=1)[:, :-1]):
                raise ValueError(f"group {g}: a dihedral names an atom twice.")
        self._Ns = np.fromiter((a.n_atoms for a in legs[0]), dtype=int, count=self._n_groups)
        self._D = int(self._Ns.sum())
        if self._D < 1:
            raise ValueError("The groups must hold at least one dihedral.")
        # the distinct atoms are fed once; the quads name them by their place in that feed
        atoms = np.concatenate([np.asarray(a.indices) for leg in legs for a in leg])
        self._index, inverse = np.unique(atoms, return_inverse=True)
        self._quads = np.ascontiguousarray(inverse.reshape(4, self._D).T, dtype=np.int32)

        self._n_bins = int(n_bins)
        if self._n_bins < 2 or self._n_bins % 2:
            raise ValueError("'n_bins' must be even and at least 2.")
        self._state_of_bin = states_of_bins(self._n_bins, state_edges)
        self._n_states = len(np.atleast_1d(state_edges))
        self._thresholds = cosine_thresholds(self._n_bins)
        if np.any(np.diff(self._thresholds) >= 0):
            raise ValueError("'n_bins' is too large: the thresholds of the cosine are not strictly decreasing.")

        self._lags = parse_lags(lags, n_lags)
        self._dt = strip_unit(dt or self._trajectory.dt, "picosecond")[0]
        self._drop_axis = None
        self._dimensions = self._box_lengths(dimensions, 0.0, "minimum_image") if minimum_image else None
        self._verbose = verbose

    @classmethod
    def from_chains(cls, ag, n_chains: int, n_monomers: int, **kwargs):
        """The polymer case: ``ag`` holds ``n_chains`` chains of ``n_monomers`` consecutive atoms each, and the
        dihedrals are the backbone ones, monomers ``(n, n + 1, n + 2, n + 3)`` of every chain,
        ``n = 0 ... n_monomers - 4``, in one group."""
        n_chains, n_monomers = int(n_chains), int(n_monomers)
        if n_chains < 1 or n_monomers < 4 or ag.n_atoms != n_chains * n_monomers:
            raise ValueError("'ag' must hold n_chains * n_monomers atoms, n_monomers >= 4.")
        place = np.arange(n_chains * n_monomers).reshape(n_chains, n_monomers)
        return cls(*(ag[place[:, i:n_monomers - 3 + i].ravel()] for i in range(4)), **kwargs)

    # ------------------------------------------------------------------ protocol

    def _prepare(self) -> None:
        self._df = self._frame_stride()
        lags = np.arange(self.n_frames, dtype=np.int64) if self._lags is None else self._lags
        self._lags_run = lags
        self.results.times = lags * self._df * self._dt
        self.results.units = {"results.times": "picosecond", "results.relaxation_times": "picosecond",
                              "results.transition_rates": "1/picosecond", "results.edges": "degree",
                              "results.angles": "degree", "results.distribution": "1/degree",
                              "results.pmf": "kilojoule/mole"}
        _lib.require_device(self._device)
        # lags without an origin never meet a frame pair: the engine gets the others (the histogram and the states
        # need no lag: lag 0 stands in where no lag has an origin)
        self._live = lags < self.n_frames
        engine = _core.DihedralEngine(
            self._Ns, self._quads, len(self._index), self._thresholds, self._state_of_bin,
            lags[self._live] if self._live.any() else np.zeros(1, dtype=np.int64), n_states=self._n_states,
            dev=self._device)
        if self._dimensions is not None:
            engine.set_box(self._dimensions)
        self._feed_engine(engine, self._index)

    def _conclude(self) -> None:
        n_t = len(self._lags_run)
        got = {"sums": np.zeros((n_t, self._n_groups)), "same": np.zeros((n_t, self._n_groups), dtype=np.int64),
               "stay": np.zeros((n_t, self._n_groups), dtype=np.int64)}
        try:
            self._batch.flush()
            if self._live.any():
                for key, value in self._engine.result().items():
                    got[key][self._live] = value
            counts = self._engine.counts()
            state_counts = self._engine.state_counts()
            transitions = self._engine.transitions()
        finally:
            self._engine.close()
        res = self.results
        res.edges = np.linspace(-180.0, 180.0, self._n_bins + 1)
        res.angles = (res.edges[:-1] + res.edges[1:]) / 2
        res.counts = counts
        total = counts.sum(axis=1, keepdims=True).astype(float)
        total[total == 0] = np.nan          # an empty group (or no frame): NaN, without a warning
        res.distribution = counts / (total * (360.0 / self._n_bins))
        res.state_counts = state_counts
        res.populations = state_counts.sum(axis=0) / total
        res.transitions = transitions
        terms = (np.maximum(self.n_frames - self._lags_run, 0)[:, None] * self._Ns[None, :]).astype(float)
        terms[terms == 0] = np.nan          # no origin (or an empty group): NaN, without a warning
        res.sums, res.same_counts, res.stay_counts = got["sums"], got["same"], got["stay"]
        res.tacf = got["sums"] / terms
        res.intermittent = got["same"] / terms
        res.continuous = got["stay"] / terms

    # ------------------------------------------------------------------ host helpers

    def calculate_relaxation_times(self) -> None:
        r"""``results.relaxation_times`` ``[2, N_g]``: :math:`\tau=\int_0^{t_\mathrm{max}}C(t)\,\mathrm dt` of
        ``results.tacf`` (row 0) and ``results.continuous`` (row 1) for every group (``calculate_residence_time``: the
        trapezoid rule, truncated at the last lag — a lower bound where the function has not decayed by then)."""
        if "tacf" not in self.results:
            raise RuntimeError("Call run() before calculate_relaxation_times().")
        self.results.relaxation_times = np.array(
            [[calculate_residence_time(self.results.times, c[:, g]) for g in range(self._n_groups)]
             for c in (self.results.tacf, self.results.continuous)])

    def calculate_transition_rates(self) -> None:
        """``results.transition_rates`` ``[N_g, S, S]`` (1/ps): the jumps ``s0 -> s1`` of ``results.transitions`` over
        the time the group's dihedrals spent in ``s0`` in the frames ``0 ... N_f - 2`` (those a jump can start from).
        The diagonal is 0; a state nobody was in gives NaN."""
        if "transitions" not in self.results:
            raise RuntimeError("Call run() before calculate_transition_rates().")
        spent = self.results.state_counts[:-1].sum(axis=0).astype(float) * (self._df * self._dt)
        spent[spent == 0] = np.nan
        rates = self.results.transitions / spent[:, :, None]
        rates[:, np.arange(self._n_states), np.arange(self._n_states)] = 0.0
        self.results.transition_rates = rates

    def calculate_pmf(self, temperature: float) -> None:
        r"""``results.pmf`` ``[N_g, n_bins]`` (kJ/mol): :math:`-k_\mathrm BT\ln[p(\varphi)/\max p]` of
        ``results.distribution`` at ``temperature`` (K); ``inf`` for an empty bin."""
        if "distribution" not in self.results:
            raise RuntimeError("Call run() before calculate_pmf().")
        temperature = float(strip_unit(temperature, "kelvin")[0])
        if not (np.isfinite(temperature) and temperature > 0):
            raise ValueError("'temperature' must be positive and finite.")
        p = self.results.distribution
        with np.errstate(divide="ignore", invalid="ignore"):
            self.results.pmf = -_GAS_CONSTANT * temperature * np.log(p / p.max(axis=1, keepdims=True))
