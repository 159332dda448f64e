"""
Frame-preparation helpers ``center_of_mass`` (reference
``src/mdhelper/algorithm/molecule.py:15-310``) — per-residue / per-segment centres
of mass used when ``groupings != "atoms"`` — and ``radius_of_gyration`` (reference
:312-587).  O(N) per frame, host NumPy (frame prep stays on the
host in this round); the per-frame radii of ``analysis.polymer.Gyradius`` are
computed on the device instead (``mdx_gyr_*``).
"""

from __future__ import annotations

import numpy as np


def _level_ids(group, grouping):
    if grouping == "residues":
        ids = getattr(group, "resindices", None)
    elif grouping == "segments":
        ids = getattr(group, "segindices", None)
    else:
        raise ValueError(f"Invalid grouping '{grouping}'.")
    if ids is None:
        raise ValueError(f"The group does not expose per-atom {grouping} indices.")
    return np.asarray(ids)


def molecule_rows(group, grouping):
    """
    ``(particle indices, CSR offsets, masses)`` of ``group`` with the rows sorted molecule by molecule (atom
    order kept inside a molecule): what the engines form residue / segment centres of mass on the device
    from.  ``grouping="atoms"``: ``(indices, None, None)``.
    """
    idx = np.asarray(group.indices)
    if grouping == "atoms":
        return idx, None, None
    _, inverse = np.unique(_level_ids(group, grouping), return_inverse=True)
    order = np.argsort(inverse, kind="stable")
    offsets = np.concatenate(([0], np.cumsum(np.bincount(inverse))))
    return idx[order], offsets, np.asarray(group.masses, dtype=np.float64)[order]


def center_of_mass(group=None, grouping: str = None, *, masses=None, positions=None,
                   images=None, dimensions=None, n_groups: int = None, raw: bool = False):
    r"""
    Centre(s) of mass :math:`\mathbf R=\sum_a m_a\mathbf r_a/\sum_a m_a`.

    Either pass a ``group`` (optionally with ``grouping`` = ``"residues"`` /
    ``"segments"`` for one centre per residue / segment, ``None`` for the whole
    group), or pass ``masses`` and ``positions`` directly (optionally reshaped into
    ``n_groups`` equal molecules).  ``images`` (boundary-crossing counts) unwrap
    the positions with ``dimensions`` first.
    """
    # (reference molecule.py:218-221: the grouping is checked before anything else)
    if grouping not in {None, "residues", "segments"}:
        raise ValueError(f"Invalid grouping: '{grouping}'. Valid options are None, 'residues', "
                         "and 'segments'.")
    if group is not None:
        pos = np.array(group.positions if positions is None else positions, dtype=float)
        m = np.asarray(group.masses if masses is None else masses, dtype=float)
        if images is not None:
            if dimensions is None:
                dims = getattr(group, "dimensions", None)
                if dims is None:
                    dims = getattr(group.universe, "dimensions", None)
                if dims is None:
                    raise ValueError("The number of periodic boundary crossings was provided, "
                                     "but no system dimensions were provided or found in the "
                                     "trajectory.")
                dimensions = dims
            pos = pos + np.asarray(images) * np.asarray(dimensions, dtype=float)[:3]
        if grouping is None and not n_groups:
            com = (m[:, None] * pos).sum(axis=0) / m.sum()
            return (com, m, pos) if raw else com
        if n_groups:
            m2 = m.reshape((n_groups, -1))
            p2 = pos.reshape((n_groups, -1, 3))
            com = np.einsum("...a,...ad->...d", m2, p2) / m2.sum(axis=-1, keepdims=True)
            return (com, m2, p2) if raw else com
        ids = _level_ids(group, grouping)
        _, inverse = np.unique(ids, return_inverse=True)
        n = inverse.max() + 1
        msum = np.bincount(inverse, weights=m, minlength=n)
        com = np.stack([np.bincount(inverse, weights=m * pos[:, k], minlength=n) for k in range(3)],
                       axis=1) / msum[:, None]
        return (com, m, pos) if raw else com

    if masses is None or positions is None:
        raise ValueError("Either a group or both masses and positions must be provided.")
    try:
        p = np.asarray(positions, dtype=float)
        m = np.asarray(masses, dtype=float)
        ragged = False
    except ValueError:
        ragged = True
    if ragged:
        return np.array([np.dot(np.asarray(mm, dtype=float), np.asarray(pp, dtype=float))
                         / np.sum(mm) for mm, pp in zip(masses, positions)])
    if n_groups:
        m = m.reshape((n_groups, -1))
        p = p.reshape((n_groups, -1, 3))
    if m.shape != p.shape[:-1]:
        raise ValueError("The shapes of the arrays containing the particle masses and "
                         "positions are incompatible.")
    return np.einsum("...a,...ad->...d", m, p) / m.sum(axis=-1, keepdims=True)


def _group_arrays(group, grouping, masses, positions, images, dimensions, n_groups):
    """Masses and float64 positions of ``group`` for ``radius_of_gyration``: flat ``[N]`` / ``[N, 3]`` for the
    whole group, ``[G, N/G]`` / ``[G, N/G, 3]`` for equally sized residues / segments (or ``n_groups`` equal
    parts), lists of arrays for residues / segments of different sizes (reference molecule.py:228-279)."""
    if group is None:
        raise ValueError("Either a group of atoms or atom positions and masses must be provided.")
    pos = np.array(group.positions if positions is None else positions, dtype=float)
    m = np.asarray(group.masses if masses is None else masses, dtype=float)
    if images is not None and positions is None:
        if dimensions is None:
            dims = getattr(group, "dimensions", None)
            if dims is None:
                dims = getattr(group.universe, "dimensions", None)
            if dims is None:
                raise ValueError("The number of periodic boundary crossings was provided, but no system "
                                 "dimensions were provided or found in the trajectory.")
            dimensions = dims
        pos = pos + np.asarray(images) * np.asarray(dimensions, dtype=float)[:3]
    if n_groups:
        return m.reshape((n_groups, -1)), pos.reshape((n_groups, -1, 3))
    if grouping is None:
        return m, pos
    _, inverse = np.unique(_level_ids(group, grouping), return_inverse=True)
    order = np.argsort(inverse, kind="stable")
    sizes = np.bincount(inverse)
    m, pos = m.reshape(-1)[order], pos.reshape(-1, 3)[order]
    if np.all(sizes == sizes[0]):
        return m.reshape((len(sizes), -1)), pos.reshape((len(sizes), -1, 3))
    cuts = np.cumsum(sizes)[:-1]
    return np.split(m, cuts), np.split(pos, cuts)


def radius_of_gyration(group=None, grouping: str = None, *, positions=None, masses=None, com=None,
                       images=None, dimensions=None, n_groups: int = None, components: bool = False):
    r"""
    Radii of gyration :math:`R_\mathrm g=\sqrt{\sum_i m_i\|\mathbf r_i-\mathbf R_\mathrm{com}\|^2/\sum_i m_i}`
    (reference molecule.py:312-587).

    Either pass a ``group`` (``grouping`` = ``None`` for one radius of all its atoms, ``"residues"`` /
    ``"segments"`` for one per residue / segment, or ``n_groups`` equal parts), or pass the *unwrapped*
    ``positions`` and ``masses`` directly: ``[N, 3]`` / ``[N]`` for one radius, ``[G, N/G, 3]`` / ``[G, N/G]``
    for one per group, or lists of per-group arrays of different lengths.  ``com`` — the centre(s) of mass —
    is computed when missing.  ``images`` and ``dimensions`` unwrap the positions read from ``group``.

    ``components=True`` returns the radii around the coordinate axes instead, e.g.
    :math:`R_{\mathrm g,x}` from the :math:`y` and :math:`z` components: shape ``(3,)`` / ``(G, 3)``.

    Returns a scalar, or ``[G]`` for grouped input (``[3]`` / ``[G, 3]`` with ``components``), in Å.

    Where this differs from the reference: residues / segments read from a ``group`` are gathered by their
    indices (the reference reshapes the atoms as they lie, which needs them contiguous and in order), grouped
    arrays are recognised by their shape whatever ``grouping`` says, and ``n_groups`` also reshapes arrays
    passed directly (the reference reshapes them for the centre of mass only and then fails).
    """
    if grouping not in {None, "residues", "segments"}:
        raise ValueError(f"Invalid grouping: '{grouping}'. Valid options are None, 'residues', "
                         "and 'segments'.")
    if masses is None or positions is None:
        masses, positions = _group_arrays(group, grouping, masses, positions, images, dimensions, n_groups)
    else:
        try:
            positions = np.asarray(positions, dtype=float)
            masses = np.asarray(masses, dtype=float)
        except ValueError:
            masses = [np.asarray(m, dtype=float) for m in masses]
            positions = [np.asarray(p, dtype=float) for p in positions]
        if n_groups and isinstance(positions, np.ndarray):
            masses = masses.reshape((n_groups, -1))
            positions = positions.reshape((n_groups, -1, 3))
    if com is None:
        com = center_of_mass(masses=masses, positions=positions)
    com = np.asarray(com, dtype=float)

    def around_axes(sq):
        """[..., 3] squared components -> the sums orthogonal to x, y and z."""
        return np.stack((sq[..., 1] + sq[..., 2], sq[..., 0] + sq[..., 2], sq[..., 0] + sq[..., 1]), axis=-1)

    if isinstance(positions, np.ndarray):
        if masses.shape != positions.shape[:-1]:
            raise ValueError("The shapes of the arrays containing the particle masses and "
                             "positions are incompatible.")
        sq = (positions - np.expand_dims(com, axis=positions.ndim - 2)) ** 2
        if positions.ndim == 3:
            if components:
                return np.sqrt(np.einsum("ga,gad->gd", masses, around_axes(sq))
                               / masses.sum(axis=1, keepdims=True))
            return np.sqrt(np.einsum("ga,gad->gd", masses, sq).sum(axis=1) / masses.sum(axis=1))
        if components:
            return np.sqrt(np.dot(masses, around_axes(sq)) / masses.sum())
        return np.sqrt(np.dot(masses, sq).sum() / masses.sum())

    if components:
        return np.sqrt(np.array([np.dot(m, around_axes((p - c) ** 2)) / m.sum()
                                 for m, p, c in zip(masses, positions, com)]))
    return np.sqrt(np.array([np.dot(m, (p - c) ** 2).sum() / m.sum()
                             for m, p, c in zip(masses, positions, com)]))
