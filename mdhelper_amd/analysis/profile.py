"""
Linear profiles (operator surface of ``mdhelper.analysis.profile``).

``DensityProfile`` (reference ``src/mdhelper/analysis/profile.py:287-996``): number and
charge density of groups of particles along x / y / z, optionally with the centre of
mass of one group held in place, and ``calculate_potential_profile`` (:28-285), the
Poisson solve of a charge density profile.

The per-frame work of the reference — positions → (unwrap, shift) → ``wrap`` →
``numpy.histogram`` per group and axis — runs in the HIP library (``mdx_prof_*``,
``csrc/mdx_profile.hip``): whole blocks of frames are binned in one pass at 12 bytes per
atom-frame, and the integer bin counts equal ``numpy.histogram``'s count for count.  The
potential profile is a 201-point problem and stays on the host (NumPy / SciPy).
"""

from __future__ import annotations

import logging
import warnings
from numbers import Real
from typing import Union

import numpy as np
from scipy import integrate, sparse
from scipy.sparse.linalg import spsolve

from .. import _core
from ..algorithm.molecule import molecule_rows
from ..algorithm.unit import strip_unit
from .base import DynamicAnalysisBase, EngineFedAnalysis, grouping_of

# CODATA 2018: elementary charge (C, exact) and vacuum permittivity (F/m)
ELEMENTARY_CHARGE = 1.602176634e-19
VACUUM_PERMITTIVITY = 8.8541878128e-12
#: e / (eps0 * angstrom) in volts: potentials from charge densities in e/Å^3 and lengths in Å
POTENTIAL_FACTOR = ELEMENTARY_CHARGE / (VACUUM_PERMITTIVITY * 1e-10)

_GROUPINGS = {"atoms", "residues", "segments"}


def calculate_potential_profile(bins, charge_density, L: float, dielectric: float = 1, *,
                                sigma_q: float = None, dV: float = None, threshold: float = 1e-5,
                                V0: float = 0, method: str = "integral", pbc: bool = False,
                                reduced: bool = False) -> np.ndarray:
    r"""
    Potential profile :math:`\Psi(z)` from a charge density profile: Poisson's equation
    :math:`\varepsilon_0\varepsilon_\mathrm r\Psi''(z)=-\rho_q(z)` with
    :math:`\Psi'(0)=-\sigma_q/\varepsilon_0\varepsilon_\mathrm r` and :math:`\Psi(0)=\Psi_0`
    (reference profile.py:28-285).

    ``method="integral"`` integrates the profile twice with the trapezoidal rule, adding
    :math:`\sigma_q` between the two; ``method="matrix"`` solves the second-order finite-difference
    system, periodic (``pbc=True``: :math:`\Psi_0=\Psi_{N-1}`) or for a slab (first row the one-sided
    derivative :math:`(-3\Psi_0+4\Psi_1-\Psi_2)/2h`, last row :math:`\Psi_0=0`).

    Parameters
    ----------
    bins : array-like ``[N_bins]`` — bin centres (Å)
    charge_density : array-like ``[N_bins]`` — charge density (e/Å³)
    L : float — system size along the axis (Å)
    dielectric : float, default 1 — relative permittivity
    sigma_q : float, keyword-only, optional — total surface charge density (e/Å²); when missing it
        follows from ``dV``, or, for ``method="integral"`` only, from the plateau of the integrated
        charge density around the middle bin (a warning is issued)
    dV : float, keyword-only, optional — potential difference across the axis (V); only used to get
        ``sigma_q``
    threshold : float, keyword-only — gradient below which the integrated profile counts as plateau
    V0 : float, keyword-only — potential at the left boundary (V)
    method : {"integral", "matrix"}, keyword-only
    pbc : bool, keyword-only — periodic axis (``method="matrix"`` only)
    reduced : bool, keyword-only — reduced units: the conversion factor is :math:`4\pi` instead of
        :math:`e/(\varepsilon_0\,\text{Å})` (``POTENTIAL_FACTOR``, from the two CODATA 2018 constants
        above; ``pint`` is not a dependency here)

    Returns
    -------
    potential : ``numpy.ndarray`` ``[N_bins]`` (V)

    Where this differs from the reference: with ``method="integral"`` the left-boundary potential is added
    to every point, the reference's documented step 5.  The reference passes ``V0`` as
    ``cumulative_trapezoid(..., initial=V0)`` instead, which SciPy >= 1.12 refuses for any value but 0 and
    older SciPy only wrote into the first element; for ``V0 = 0`` both agree.  ``method="matrix"`` ignores
    ``V0``, as the reference does.
    """
    if len(bins) != len(charge_density):
        raise ValueError("'bins' and 'charge_density' arrays must have the same length.")
    bins = np.asarray(bins, dtype=float)
    charge_density = np.asarray(charge_density, dtype=float)
    factor = 4 * np.pi if reduced else POTENTIAL_FACTOR

    # perfectly conducting boundaries: the surface charge that gives the potential difference dV
    if sigma_q is None and dV is not None:
        sigma_q = (integrate.trapezoid(bins * charge_density, bins) - dielectric * dV / factor) / L

    if method == "integral":
        field = integrate.cumulative_trapezoid(charge_density, bins, initial=0)
        if sigma_q is None:
            warnings.warn("No surface charge density information. The value will be extracted from "
                          "the integrated charge density profile, which may be inaccurate due to "
                          "numerical errors.")
            flat = np.abs(np.gradient(field)) < threshold
            cuts = np.where(np.diff(flat))[0] + 1
            if len(cuts) == 0:
                logging.warning("No bulk plateau region found in the charge density profile. The "
                                "average value over the entire profile will be used.")
                sigma_q = field.mean()
            else:
                middle = len(field) // 2
                sigma_q = field[cuts[cuts <= middle][-1]:cuts[cuts >= middle][0]].mean()
        return -factor * integrate.cumulative_trapezoid(field + sigma_q, bins, initial=0) / dielectric + V0

    elif method == "matrix":
        if sigma_q is None:
            raise ValueError("No surface charge density information. Either 'sigma_q' or 'dV' must be "
                             "provided when method='matrix'.")
        h = bins[1] - bins[0]
        if not np.allclose(np.diff(bins), h):
            raise ValueError("'bins' must be uniformly spaced.")
        N = len(bins)
        A = sparse.diags((1, -2, 1), (-1, 0, 1), shape=(N, N), format="csc")
        b = charge_density.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=sparse.SparseEfficiencyWarning)
            if pbc:
                A[0, -1] = A[-1, 0] = 1
                b *= -factor * h ** 2 / dielectric
                psi = np.empty_like(b)
                psi[1:] = spsolve(A[1:, 1:], b[1:])
                psi[0] = psi[-1]
                return psi
            A[0, :3] = -1.5, 2, -0.5
            A[-1, 0] = 1
            A[-1, -2:] = 0
            b[0] = -factor * h * sigma_q / dielectric
            b[1:-1] *= -factor * h ** 2 / dielectric
            b[-1] = 0
            return spsolve(A, b)


def _parse_axes(axes) -> np.ndarray:
    if isinstance(axes, (int, np.integer)):
        return np.array((axes,), dtype=int)
    return np.fromiter((ord(a.lower()) - 120 if isinstance(a, str) else a for a in axes),
                       count=len(axes), dtype=int)


class DensityProfile(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Number and charge density profiles :math:`\rho_i(z)` and :math:`\rho_q(z)=\sum_i z_ie\rho_i(z)`
    along the given axes (reference profile.py:287-996): particle positions are binned along each axis,

    .. math:: \rho_i(z)=\frac{N_\mathrm{bins}}{V}\left\langle\sum_\alpha\delta(z-z_\alpha)\right\rangle

    Parameters (reference :507-520)
    ----------
    groups : AtomGroup or sequence of AtomGroups
    groupings : {"atoms", "residues", "segments"} or one per group — positions binned: atoms, or the
        centres of mass of residues / segments (which must be whole)
    axes : int, str or sequence, default ``"xyz"`` — e.g. ``2``, ``"xy"``, ``(0, 1)``
    n_bins : int or one per axis, default 201
    charges : array-like ``[N_g]``, keyword-only, optional — charge number of every group's
        entities; read from the topology when it has charges and they are uniform within a group
    dimensions : array-like ``(3,)``, keyword-only, optional — box lengths (Å); multiplied by ``scales``
    dt : float, keyword-only, optional — time between frames (ps)
    scales : float or array-like ``(3,)``, keyword-only — scaling of the dimensions
    average : bool, keyword-only, default True — average over the frames, else one profile per frame
    recenter : int, AtomGroup or ``(group, position)``, keyword-only, optional — hold the centre of
        mass of one of ``groups`` at ``position`` (default: the box centre; a NaN component leaves
        that axis alone) by shifting all particles every frame
    reduced : bool, keyword-only — reduced units
    parallel : bool, keyword-only — accepted and ignored
    comm, device : keyword-only (extension) — see below

    Results
    -------
    ``results.bins`` — list per axis of bin centres ``[N_bins]`` (Å); ``results.number_densities`` —
    list per axis of ``[N_g, N_bins]``, or ``[N_g, N_frames, N_bins]`` with ``average=False`` (Å⁻³);
    ``results.charge_densities`` — list per axis of ``[N_bins]`` / ``[N_frames, N_bins]`` when charges
    are known (e/Å³); ``results.times`` with ``average=False`` (ps); ``results.units``;
    ``results.potentials`` after :meth:`calculate_potential_profile`.

    Where this differs from the reference:

    * The serial result layout above is returned whatever ``parallel`` is (the reference's parallel
      path stacks the axes into one array and needs equal bin counts for it; that restriction on
      ``n_bins`` is still checked).
    * With ``comm=`` of more than one rank, frames shard across the ranks and the integer counts are
      summed once at the end.  ``recenter`` cannot shard: the unwrap that precedes the centre of mass
      carries image counts from frame to frame, so ``recenter`` with more than one rank raises
      ``ValueError``.
    * The centre of mass that ``recenter`` holds in place is summed in a fixed order on the device; the
      reference's ``einsum`` may associate the same terms differently (last-bit differences of the
      shift, which move a count only for a coordinate within ~1e-9 Å of a bin edge).
    * ``average=False`` with charges gives ``charge_densities`` of ``[N_frames, N_bins]``: the sum runs over the
      leading group axis of ``[N_g, N_frames, N_bins]``.  The reference's ``einsum("g,...gb->...b")`` takes the
      group axis second to last, which only fits the averaged layout and raises for this one.
    * :meth:`calculate_potential_profile` averages ``average=False`` charge densities over the frames
      (the reference tests ``ndim == 3``, which its ``[N_frames, N_bins]`` arrays never have, and
      then fails on the 2-D array).
    * There is no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    * Two messages: the warning for groups of mixed charge says the charge density profile "will not be
      calculated" (the reference's text says "will be calculated", while its code skips it as this one
      does), and the invalid-grouping error lists the valid values in sorted order (the reference joins a
      set, whose order varies from run to run).
    * Integer ``dimensions`` are converted to float64 before ``scales`` applies (the reference multiplies the
      integer array in place, which NumPy refuses for a fractional scale).  Box lengths taken from the
      universe are scaled in float32, as the reference does, and widened afterwards.
    """

    def __init__(self, groups, groupings: Union[str, tuple] = "atoms",
                 axes: Union[int, str, tuple] = "xyz", n_bins: Union[int, tuple] = 201, *,
                 charges=None, dimensions=None, dt=None, scales: Union[float, tuple] = 1,
                 average: bool = True, recenter=None, reduced: bool = False, parallel: bool = False,
                 verbose: bool = True, **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "universe") else list(groups)
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, parallel, verbose, **kwargs)

        self._n_groups = len(self._groups)
        if isinstance(groupings, str):
            if groupings not in _GROUPINGS:
                raise ValueError(f"Invalid grouping '{groupings}'. Valid values: "
                                 f"{', '.join(sorted(_GROUPINGS))}.")
            self._groupings = self._n_groups * [groupings]
        else:
            if self._n_groups != len(groupings):
                raise ValueError("The number of grouping values is not equal to the number of groups.")
            for g in groupings:
                if g not in _GROUPINGS:
                    raise ValueError(f"Invalid grouping '{g}'. Valid values: "
                                     f"{', '.join(sorted(_GROUPINGS))}.")
            self._groupings = list(groupings)

        self._axes = _parse_axes(axes)

        if isinstance(n_bins, (int, np.integer)):
            self._n_bins = n_bins * np.ones(self._axes.shape, dtype=int)
        elif not isinstance(n_bins, str):
            if len(n_bins) == len(self._axes):
                n_bins = np.asarray(n_bins, dtype=int)
                if parallel and np.any(n_bins != n_bins[0]):
                    raise ValueError("All axes must use the same number of bins when parallel=True.")
                self._n_bins = n_bins
            else:
                raise ValueError("The dimension of the array of bin counts is incompatible with the "
                                 "number of axes to calculate density profiles along.")
        else:
            raise ValueError("The specified bin counts must be an integer or an iterable object.")

        if charges is not None:
            if len(charges) != self._n_groups:
                raise ValueError("The number of group charges is not equal to the number of groups.")
            charges, unit_ = strip_unit(charges, "elementary_charge")
            if reduced and not isinstance(unit_, str):
                raise TypeError("'charges' cannot have units when reduced=True.")
            self._charges = np.asarray(charges)
        elif hasattr(self.universe.atoms, "charges"):
            self._charges = np.empty(self._n_groups)
            for i, (g, gr) in enumerate(zip(self._groups, self._groupings)):
                qs = getattr(g, gr).charges
                if not np.allclose((q := qs[0]), qs):
                    self._charges = None
                    warnings.warn(f"Not all {gr} in group {i} share the same charge. The charge "
                                  "density profile will not be calculated.")
                    break
                self._charges[i] = q
        else:
            self._charges = None

        if dimensions is not None:
            if len(dimensions) != 3:
                raise ValueError("'dimensions' must have length 3.")
            self._dimensions = np.array(strip_unit(dimensions, "angstrom")[0])
            if not np.issubdtype(self._dimensions.dtype, np.floating):
                self._dimensions = self._dimensions.astype(float)
        elif self.universe.dimensions is not None:
            # MDAnalysis holds box lengths in float32 and the reference scales them in place, in float32
            self._dimensions = np.array(self.universe.dimensions[:3], dtype=np.float32)
        else:
            raise ValueError("No system dimensions found or provided.")

        if isinstance(scales, Real) or (len(scales) == 3 and isinstance(scales[0], Real)):
            self._dimensions *= scales            # in the precision of the array, as the reference does
            self._dimensions = self._dimensions.astype(float)
        else:
            raise ValueError("The scaling factor(s) must be provided as a floating-point number or in "
                             "an array with shape (3,).")

        self._dt, unit_ = strip_unit(dt or self._trajectory.dt, "picosecond")
        if reduced and not isinstance(unit_, str):
            raise TypeError("'dt' cannot have units when reduced=True.")

        if recenter is None:
            self._recenter = None
        else:
            is_group = hasattr(recenter, "universe")
            if isinstance(recenter, (int, np.integer)) or is_group:
                recenter_group = recenter
                recenter_position = self._dimensions / 2
            elif isinstance(recenter, tuple) and len(recenter) == 2:
                recenter_group, recenter_position = recenter
                recenter_position = np.asarray(recenter_position, dtype=float)
            else:
                raise ValueError("Invalid value passed to 'recenter'. The argument must either be a "
                                 "MDAnalysis.AtomGroup, its index in 'groups', multiple groups/indices, "
                                 "or a tuple containing the aforementioned information and a "
                                 "specified center of mass, in that order.")
            if isinstance(recenter_group, (int, np.integer)):
                if not 0 <= recenter_group < self._n_groups:
                    raise ValueError("Invalid group index passed to 'recenter'.")
            elif hasattr(recenter_group, "universe"):
                try:
                    recenter_group = self._groups.index(recenter_group)
                except ValueError:
                    raise ValueError("The specified AtomGroup in 'recenter' is not in 'groups'.")
            self._recenter = (int(recenter_group), recenter_position)
            if self._comm.world_size > 1:
                raise ValueError("recenter cannot be combined with more than one rank: the unwrap before "
                                 "the centre of mass carries image counts from frame to frame, so the "
                                 "frames cannot shard.  Run it on one rank.")

        self._Ns = np.fromiter((getattr(a, f"n_{g}") for a, g in zip(self._groups, self._groupings)),
                               dtype=int, count=self._n_groups)
        self._N = self._Ns.sum()
        self._slices = []
        index = 0
        for N in self._Ns:
            self._slices.append(slice(index, index + N))
            index += N

        self._average = average
        self._reduced = reduced
        self._verbose = verbose

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # (recenter, which makes the frames sequential, runs on one rank)

    def _prepare(self) -> None:
        self.results.bins = [
            np.linspace(self._dimensions[a] / (2 * self._n_bins[i]),
                        self._dimensions[a] - self._dimensions[a] / (2 * self._n_bins[i]), self._n_bins[i])
            for i, a in enumerate(self._axes)]
        if not self._average:
            self.results.times = self._frame_numbers() * self._dt
        self.results.units = {"results.bins": "angstrom", "results.number_densities": "angstrom^-3"}
        if not self._average:
            self.results.units["results.times"] = "picosecond"
        if self._charges is not None:
            self.results.charge_densities = [None for _ in self._axes]
            self.results.units["results.charge_densities"] = "elementary_charge/angstrom^3"

        # rows of every frame in concatenated-group order; residue / segment centres of mass are formed on
        # the device from rows sorted molecule by molecule (plain-atom groups: molecules of one particle)
        rows = [molecule_rows(g, gr) for g, gr in zip(self._groups, self._groupings)]
        engine = _core.ProfileEngine(self._Ns, self._axes, self._n_bins, self._dimensions,
                                     per_frame=not self._average, dev=self._device)
        grouping = grouping_of(rows)
        if grouping is not None:
            engine.set_grouping(*grouping)
        if self._recenter is not None:
            k, target = self._recenter
            engine.set_recenter(k, getattr(self._groups[k], self._groupings[k]).masses, target)
        self._feed_engine(engine, np.concatenate([r[0] for r in rows]))

    def _conclude(self) -> None:
        self._batch.flush()
        counts = self._engine.counts()
        self._engine.close()
        if self._comm.world_size > 1:
            for a, c in enumerate(counts):
                c = np.ascontiguousarray(c, dtype=np.int64)
                counts[a] = np.asarray(self._comm.allreduce(c)) if self._average else self._gather_frame_rows(c, 1)
        V = np.prod(self._dimensions)
        self.results.number_densities = []
        for a, c in enumerate(counts):
            denom = self._n_bins[a] / V
            if self._average:
                denom /= self.n_frames
            density = c.astype(float)
            density *= denom
            self.results.number_densities.append(density)
            if self._charges is not None:
                # "g,...gb->...b" for the averaged [N_g, N_bins]; the group axis leads in both layouts
                self.results.charge_densities[a] = np.einsum("g,g...b->...b", self._charges, density)

    def calculate_potential_profile(self, dielectric: float, axis: Union[int, str], *, sigma_q=None,
                                    dV=None, threshold: float = 1e-5, V0=0, method: str = "integral",
                                    pbc: bool = False) -> None:
        """
        Potential profile along ``axis`` (``2`` or ``"z"``...) from the charge density profile of the run
        (module function :func:`calculate_potential_profile`, reference :879-996); stored in
        ``results.potentials[i]``, ``i`` the position of the axis in ``axes``.
        """
        if "charge_densities" not in self.results:
            raise RuntimeError("Either call run() before calculate_potential_profile() or provide "
                               "charge information when initializing the DensityProfile object.")
        if "potentials" not in self.results:
            self.results.potentials = {}
            self.results.units["results.potentials"] = "volt"
        if isinstance(axis, str):
            axis = ord(axis.lower()) - 120
        index = np.where(self._axes == axis)[0][0]

        if sigma_q is not None:
            sigma_q, unit_ = strip_unit(sigma_q, "elementary_charge/angstrom**2")
            if self._reduced and not isinstance(unit_, str):
                raise ValueError("'sigma_q' cannot have units when reduced=True.")
        if dV is not None:
            dV, unit_ = strip_unit(dV, "volt")
            if self._reduced and not isinstance(unit_, str):
                raise ValueError("'dV' cannot have units when reduced=True.")
        if V0 is not None:
            V0, unit_ = strip_unit(V0, "volt")
            if self._reduced and not isinstance(unit_, str):
                raise ValueError("'V0' cannot have units when reduced=True.")

        charge_density = self.results.charge_densities[index]
        if charge_density.ndim == 2:
            charge_density = charge_density.mean(axis=0)
        self.results.potentials[index] = calculate_potential_profile(
            self.results.bins[index], charge_density, self._dimensions[axis], dielectric, sigma_q=sigma_q,
            dV=dV, threshold=threshold, V0=V0, method=method, pbc=pbc, reduced=self._reduced)
