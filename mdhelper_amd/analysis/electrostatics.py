"""
Electrostatics (operator surface of ``mdhelper.analysis.electrostatics``): ``DipoleMoment`` — the
instantaneous dipole moment vectors of groups of atoms — and ``calculate_relative_permittivity``, the
dipole moment fluctuation formula.

Mirrors reference ``src/mdhelper/analysis/electrostatics.py``: ``calculate_relative_permittivity``
(:25-103) and ``DipoleMoment`` (:105-482) keep their names, arguments, defaults, result attributes and
error behaviour.

Where the work goes: the reference forms ``q @ positions`` per frame and group on one core (:374-391).
Here whole blocks of frames go to the dipole engine (``mdx_dip_*``), which reads the positions once,
follows the atoms across the boundaries in registers (``unwrap``) and sums ``q (r + image L)`` in float64
in a fixed order; frames shard across ranks.
"""

from __future__ import annotations

from numbers import Real

import numpy as np

from .. import _core
from ..algorithm.topology import make_whole_images
from ..algorithm.unit import strip_unit
from ..universe import box_volumes
from .base import DynamicAnalysisBase, EngineFedAnalysis
from .profile import ELEMENTARY_CHARGE, VACUUM_PERMITTIVITY

# CODATA 2018 (exact)
BOLTZMANN = 1.380649e-23
# e^2 / (eps0 k_B 1e-10 m): M^2 / (V T) in e^2 Å^2 / (Å^3 K) to a pure number, ≈ 2.0998524e6 K
PERMITTIVITY_FACTOR = ELEMENTARY_CHARGE ** 2 / (VACUUM_PERMITTIVITY * BOLTZMANN * 1e-10)


def calculate_relative_permittivity(M, temperature: float, volume, *, reduced: bool = False) -> float:
    r"""
    Relative permittivity (static dielectric constant) from the instantaneous dipole moments by the
    dipole moment fluctuation formula (reference :25-103),

    .. math:: \varepsilon_\mathrm r=1+\frac{\overline{\langle\mathbf M^2\rangle
              -\langle\mathbf M\rangle^2}}{3\varepsilon_0Vk_\mathrm BT}

    evaluated as ``1 + C * (M**2 - M.mean(axis=0)**2).mean() / (V * T)``: the mean over frames and
    components carries the 1/3.

    M : array-like ``[N_t, 3]`` (e·Å) — instantaneous dipole moments
    temperature : float (K; the energy scale with ``reduced=True``)
    volume : float or array-like (Å³) — its mean is used
    reduced : bool, keyword-only — reduced units: ``C = 4 pi``; else ``C = e^2 / (eps0 k_B 1e-10 m)``

    The inputs are not modified (the reference's non-reduced branch multiplies them by units in place).
    """
    M = np.asarray(M, dtype=float)
    fluctuation = (M ** 2 - M.mean(axis=0) ** 2).mean()
    V = np.asarray(volume, dtype=float).mean()
    if reduced:
        return float(1 + 4 * np.pi * fluctuation / (V * temperature))
    return float(1 + PERMITTIVITY_FACTOR * fluctuation / (V * temperature))


class DipoleMoment(EngineFedAnalysis, DynamicAnalysisBase):
    r"""
    Instantaneous dipole moment vectors (reference :105-482),

    .. math:: \mathbf M=\sum_i^Nq_i\mathbf z_i

    per frame and group, and from them the relative permittivity
    (:meth:`calculate_relative_permittivity`).

    Parameters (reference :242-249)
    ----------
    groups : AtomGroup or sequence of AtomGroups
    charges : array-like, optional — per group a real number or an array with one entry per atom (e);
        read from the topology when absent
    dimensions : array-like ``(3,)``, optional — box lengths (Å); multiplied by ``scales``
    scales : float or array-like ``(3,)`` — scaling of the dimensions
    average : bool — time-average the dipole moments and volumes
    reduced : bool — reduced units; only affects :meth:`calculate_relative_permittivity`
    neutralize : bool — subtract the net charge of every molecule (residue) at its centre of mass, so that
        the dipole of a charged molecule does not depend on where it is
    unwrap : bool — follow the atoms across the periodic boundaries from frame to frame, starting from
        molecules made whole in the first analysed frame
    parallel : bool — accepted; the same layout is returned
    comm, device : keyword-only (extension) — frames shard across ranks, one all-reduce at the end

    Results: ``results.dipoles`` ``[N_t, N_g, 3]`` (e·Å), ``results.volumes`` ``[N_t]`` (Å³),
    ``results.times`` ``[N_t]`` (ps; absent with ``average=True``, which also makes the dipoles
    ``[N_g, 3]`` and the volume a scalar), ``results.units``, ``results.dielectric`` after
    :meth:`calculate_relative_permittivity`.

    Where this differs from the reference:

    * The serial reference adds ``L_x / 2`` to the x coordinate of the first row before every group's
      product (:379); its parallel path does not.  This class computes the stated definition
      ``M = sum q z``, which is the parallel path.
    * ``neutralize``: the reference rewrites the charge array in place every frame with
      ``q -= q * m / M_res`` (:384-386), which neither removes the net charge nor stays fixed over the
      frames.  Here the effective charges are formed once, on the host in float64:
      ``q'_i = q_i - Q_res m_i / M_res`` with ``Q_res`` and ``M_res`` summed over the atoms of that residue
      inside the group.  This is ``sum q_i (r_i - R_com)``, what the parameter's description says.
    * Image shifts are applied in float64 (the reference adds ``images * dimensions`` to the float32
      positions, topology.py:376).
    * ``parallel`` is accepted and returns the same layout.
    * ``results.dielectric`` is a float, which is what the reference's code returns (its docstring says
      ``(3,)``).
    * ``unwrap=True`` with more than one rank raises ``ValueError``: the image counts run from frame to
      frame, so the frames cannot shard.
    * The molecules of the first analysed frame are made whole along the universe's bonds
      (``make_whole_images``); ``L`` and the thresholds of the unwrap are the constructor's
      ``dimensions * scales``, which the reference keeps fixed over the run as well.
    * A topology without charges, with ``charges`` given: whether every residue is neutral is decided from
      the given charges (the reference asks the topology, which then raises).
    * There is no CPU fallback: without a HIP device ``run()`` raises ``RuntimeError``.
    """

    def __init__(self, groups, charges=None, dimensions=None, scales=1, average: bool = False,
                 reduced: bool = False, neutralize: bool = False, unwrap: bool = False,
                 parallel: bool = False, verbose: bool = True, **kwargs) -> None:
        self._groups = [groups] if hasattr(groups, "universe") else list(groups)
        self._n_groups = len(self._groups)
        self.universe = self._groups[0].universe
        super().__init__(self.universe.trajectory, parallel, verbose, **kwargs)

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
                             "an array with shape (3,). ")

        self._Ns = np.fromiter((g.n_atoms for g in self._groups), dtype=int, count=self._n_groups)
        self._N = self._Ns.sum()
        self._slices = []
        index = 0
        for N in self._Ns:
            self._slices.append(slice(index, index + N))
            index += N

        has_charges = hasattr(self.universe.atoms, "charges")
        if charges is not None:
            charges = list(charges)
            if len(charges) == self._n_groups:
                for i, (g, q) in enumerate(zip(self._groups, charges)):
                    q = strip_unit(q, "elementary_charge")[0]
                    if isinstance(q, Real):
                        q = q * np.ones(g.n_atoms)
                    elif g.n_atoms != len(q):
                        raise ValueError(f"The number of charges in 'charges[{i}]' is not equal to the "
                                         "number of atoms in the corresponding group.")
                    charges[i] = np.array(q, dtype=float)
                self._charges = charges
            else:
                raise ValueError("The number of group charge arrays is not equal to the number of groups.")
        elif has_charges:
            self._charges = [np.array(g.charges, dtype=float) for g in self._groups]
        else:
            raise ValueError("The topology has no charge information.")

        if has_charges:
            residue_charges = self.universe.atoms.residues.charges
        else:
            _, inverse = np.unique(np.concatenate([np.asarray(g.resindices) for g in self._groups]),
                                   return_inverse=True)
            residue_charges = np.bincount(inverse, weights=np.concatenate(self._charges))
        self._all_neutral = np.allclose(residue_charges, 0, atol=1e-6)
        self._all_included = sum(g.n_atoms for g in self._groups) == self.universe.atoms.n_atoms

        if unwrap and self._comm.world_size > 1:
            raise ValueError("unwrap cannot be combined with more than one rank: the image counts run "
                             "from frame to frame, so the frames cannot shard.  Run it on one rank.")

        self._average = average
        self._reduced = reduced
        self._neutralize = neutralize
        self._unwrap = unwrap
        self._verbose = verbose

    def _effective_charges(self) -> np.ndarray:
        """float64[N]: the charges in concatenated-group order; with ``neutralize`` every residue's net
        charge inside its group is taken off in proportion to the masses, ``q - Q_res m / M_res``."""
        out = []
        for g, q in zip(self._groups, self._charges):
            q = np.asarray(q, dtype=np.float64)
            if self._neutralize:
                m = np.asarray(g.masses, dtype=np.float64)
                _, inverse = np.unique(np.asarray(g.resindices), return_inverse=True)
                Q_res = np.bincount(inverse, weights=q)
                M_res = np.bincount(inverse, weights=m)
                q = q - Q_res[inverse] * m / M_res[inverse]
            out.append(q)
        return np.concatenate(out)

    # ------------------------------------------------------------------ protocol

    _shard_frames = True        # (unwrap, which makes the frames sequential, runs on one rank)

    def _prepare(self) -> None:
        index = np.concatenate([np.asarray(g.indices) for g in self._groups])
        engine = _core.DipoleEngine(self._Ns, self._effective_charges(), dev=self._device)
        if self._unwrap:
            st = self._sliced_trajectory
            self.universe.trajectory[st.frames[0] if hasattr(st, "frames") else (self.start or 0)]
            # the first analysed frame with every molecule whole, in float64
            positions = np.asarray(self.universe.trajectory.ts.positions, dtype=np.float64)
            images = make_whole_images(self.universe, self._dimensions)
            engine.set_unwrap(self._dimensions, positions[index] + images[index] * self._dimensions)

        self.results.dipoles = np.zeros((self.n_frames, self._n_groups, 3))
        self.results.volumes = np.zeros(self.n_frames)
        self.results.units = {"results.dipoles": "elementary_charge*angstrom", "results.volumes": "angstrom^3"}
        if not self._average:
            self.results.times = (self.step or 1) * self._trajectory.dt * np.arange(self.n_frames)
            self.results.units["results.times"] = "picosecond"
        self._feed_engine(engine, index)

    def _single_frame(self) -> None:
        self.results.volumes[self._frame_index] = self._ts.volume
        super()._single_frame()

    def _before_blocks(self) -> None:
        boxes = self._trajectory.box_block(self._frame_numbers())
        if boxes is not None:
            self.results.volumes = box_volumes(boxes)

    def _conclude(self) -> None:
        self._batch.flush()
        rows = self._engine.result()                        # [N_g, frames of this rank, 3]
        self._engine.close()
        self.results.dipoles = self._gather_frame_rows(np.ascontiguousarray(rows.transpose(1, 0, 2)))
        if self._average:
            self.results.dipoles = self.results.dipoles.mean(axis=0)
            self.results.volumes = self.results.volumes.mean()

    def calculate_relative_permittivity(self, temperature) -> None:
        """
        Relative permittivity from the dipole moments of the run, summed over the groups (module function
        :func:`calculate_relative_permittivity`, reference :431-482); stored in ``results.dielectric``.

        temperature : float (K), or the energy scale with ``reduced=True``
        """
        if self._average:
            raise RuntimeError("Cannot compute relative permittivity using the"
                               "averaged dipole moment.")
        elif not self._all_neutral and not self._neutralize:
            raise RuntimeError("Cannot compute relative permittivity for a "
                               "non-neutral system or a system with ions unless "
                               "the net charge is subtracted at the center of "
                               "mass of each molecule carrying a net charge.")
        elif not self._all_included:
            raise RuntimeError("Cannot compute relative permittivity when not all"
                               "atoms in the system are accounted for in the "
                               "groups.")
        temperature, unit_ = strip_unit(temperature, "kelvin")
        if self._reduced and not isinstance(unit_, str):
            raise ValueError("'temperature' cannot have units when reduced=True.")

        self.results.dielectric = calculate_relative_permittivity(
            self.results.dipoles.sum(axis=1), temperature, self.results.volumes.mean(), reduced=self._reduced)
