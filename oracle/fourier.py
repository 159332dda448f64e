"""
oracle.fourier — CPU restatement of the structure-factor path.

TEST INFRASTRUCTURE (see ``oracle/__init__.py``).

Follows:

* ``fourier_sum_ref``   reference ``src/mdhelper/algorithm/accelerated.py:81-122``
                        (``F[q] = sum_j exp(i q . r_j)``; ``dot_1d_1d :12-43``,
                        ``delta_fourier_transform_1d_1d :45-79``)
* ``inner_ref``         ``accelerated.py:167-206`` (``q . r`` table)
* ``ssf_frame_ref``     ``src/mdhelper/analysis/structure.py:1481-1527``
                        (``_single_frame``: exp and trig forms, modes None/pair/partial)
* ``grid_wavevectors``  ``structure.py:1376-1381, 1404-1410`` (meshgrid, default 'xy' indexing)
* ``ssf_run_ref``       ``_prepare :1456-1479`` + ``_conclude :1529-1550``
"""

from __future__ import annotations

from itertools import combinations_with_replacement

import numpy as np


def fourier_sum_ref(qs: np.ndarray, rs: np.ndarray, q_chunk: int = 64) -> np.ndarray:
    """complex128[N_q] = sum over particles of exp(i q.r), float64 throughout."""
    qs = np.asarray(qs, dtype=np.float64).reshape(-1, 3)
    rs = np.asarray(rs, dtype=np.float64).reshape(-1, 3)
    out = np.empty(qs.shape[0], dtype=np.complex128)
    for lo in np.arange(0, qs.shape[0], q_chunk):
        q = qs[lo:lo + q_chunk]
        # a[0]*b[0] + a[1]*b[1] + a[2]*b[2]  (accelerated.py:43)
        phase = (q[:, None, 0] * rs[None, :, 0] + q[:, None, 1] * rs[None, :, 1]) \
            + q[:, None, 2] * rs[None, :, 2]
        out[lo:lo + q_chunk] = np.exp(1j * phase).sum(axis=1)
    return out


def inner_ref(qs, rs):
    qs = np.asarray(qs, dtype=np.float64).reshape(-1, 3)
    rs = np.asarray(rs, dtype=np.float64).reshape(-1, 3)
    return (qs[:, None, 0] * rs[None, :, 0] + qs[:, None, 1] * rs[None, :, 1]) \
        + qs[:, None, 2] * rs[None, :, 2]


def ssf_pairs(n_groups: int, mode):
    """``_prepare`` (structure.py:1459-1464)."""
    if mode == "partial":
        return tuple(combinations_with_replacement(range(n_groups), 2))
    if mode == "pair":
        return ((0, n_groups - 1),)
    return ((None, None),)


def ssf_frame_ref(wavevectors, positions, slices, pairs, mode, form="exp"):
    """One frame's un-normalised contribution, float64[n_pairs, N_q]."""
    out = np.zeros((len(pairs), len(wavevectors)))
    if form == "exp":
        if mode is None:
            rho = fourier_sum_ref(wavevectors, positions)
            out[0] = (rho * rho.conj()).real
        else:
            for i, (j, k) in enumerate(pairs):
                rho_j = fourier_sum_ref(wavevectors, positions[slices[j]])
                if j == k:
                    out[i] = (rho_j * rho_j.conj()).real
                else:
                    rho_k = fourier_sum_ref(wavevectors, positions[slices[k]])
                    out[i] = 2 * (rho_j * rho_k.conj()).real
    elif form == "trig":
        # accelerated.py:249-321 (Pythagorean identities on the q.r table)
        if mode is None:
            qr = inner_ref(wavevectors, positions)
            out[0] = np.cos(qr).sum(1) ** 2 + np.sin(qr).sum(1) ** 2
        else:
            for i, (j, k) in enumerate(pairs):
                qr_j = inner_ref(wavevectors, positions[slices[j]])
                if j == k:
                    out[i] = np.cos(qr_j).sum(1) ** 2 + np.sin(qr_j).sum(1) ** 2
                else:
                    qr_k = inner_ref(wavevectors, positions[slices[k]])
                    out[i] = 2 * (np.cos(qr_j).sum(1) * np.cos(qr_k).sum(1)
                                  + np.sin(qr_j).sum(1) * np.sin(qr_k).sum(1))
    else:
        raise ValueError("Invalid form.")
    return out


def grid_wavevectors(dimensions, n_points):
    """Cubic / non-cubic reciprocal grid, rows ordered as numpy.meshgrid's default 'xy'."""
    dimensions = np.asarray(dimensions, dtype=np.float64)
    if np.allclose(dimensions, dimensions[0]):
        grid = 2 * np.pi * np.arange(n_points) / dimensions[0]
        return np.stack(np.meshgrid(grid, grid, grid), -1).reshape(-1, 3)
    return np.stack(
        np.meshgrid(*[2 * np.pi * np.arange(n_points) / L for L in dimensions]), axis=-1
    ).reshape(-1, 3)


def ssf_run_ref(frames, group_sizes, wavevectors, *, mode=None, form="exp",
                sort=True, unique=True):
    """
    frames : float[F, N, 3] with the groups laid out consecutively
    (``self._positions[s]`` of structure.py:1484-1486).
    """
    wavevectors = np.asarray(wavevectors, dtype=np.float64)
    wavenumbers = np.linalg.norm(wavevectors, axis=1)
    slices, idx = [], 0
    for n in group_sizes:
        slices.append(slice(idx, idx + n))
        idx += n
    n_total = idx
    pairs = ssf_pairs(len(group_sizes), mode)
    ssf = np.zeros((len(pairs), len(wavenumbers)))
    positions = np.empty((n_total, 3))
    for f in np.arange(len(frames)):
        positions[:] = frames[f][:n_total]
        ssf += ssf_frame_ref(wavevectors, positions, slices, pairs, mode, form)
    ssf /= len(frames) * n_total
    out_q = np.unique(wavenumbers.round(11)) if unique else wavenumbers
    if unique:
        ssf = np.hstack([ssf[:, np.isclose(q, wavenumbers)].mean(axis=1, keepdims=True)
                         for q in out_q])
    if sort:
        order = np.argsort(out_q)
        out_q = out_q[order]
        ssf = ssf[:, order]
    return {"pairs": pairs, "wavenumbers": out_q, "ssf": ssf}


def isf_run_ref(frames, group_sizes, wavevectors, n_lags=None, *, mode=None, incoherent=False,
                sort=True, unique=True):
    """
    Intermediate scattering functions, restating
    ``IntermediateScatteringFunction._prepare/_single_frame/_conclude``
    (reference structure.py:1904-2127, form="exp"; the "trig" form computes the same numbers).

    frames : float[F, N, 3] with the groups laid out consecutively.
    Returns cisf[n_lags, n_pairs or 1, N_q'], iisf[n_lags, n_groups or 1, N_q'] (or None).
    """
    frames = np.asarray(frames, dtype=np.float64)
    n_frames = len(frames)
    n_lags = n_lags or n_frames
    wavevectors = np.asarray(wavevectors, dtype=np.float64)
    wavenumbers = np.linalg.norm(wavevectors, axis=1)
    slices, idx = [], 0
    for n in group_sizes:
        slices.append(slice(idx, idx + n))
        idx += n
    n_total = idx
    n_groups = len(group_sizes)
    pairs = ssf_pairs(n_groups, mode)
    n_q = len(wavevectors)
    cisf = np.zeros((n_lags, 1 if mode is None else len(pairs), n_q))
    iisf = np.zeros((n_lags, 1 if mode is None else n_groups, n_q)) if incoherent else None
    ring_pos = np.zeros((n_lags, n_total, 3))
    ring_rho = np.empty((n_lags, 1 if mode is None else n_groups, n_q), dtype=complex)
    for f in range(n_frames):
        cur = f % n_lags
        ring_pos[cur] = frames[f][:n_total]
        if mode is None:
            ring_rho[cur, 0] = fourier_sum_ref(wavevectors, ring_pos[cur])
        else:
            for g in range(n_groups):
                ring_rho[cur, g] = fourier_sum_ref(wavevectors, ring_pos[cur, slices[g]])
        for lag in range(min(n_lags, f + 1)):
            old = (f - lag) % n_lags
            if mode is None:
                cisf[lag, 0] += (ring_rho[old, 0] * ring_rho[cur, 0].conj()).real
                if incoherent:
                    iisf[lag, 0] += fourier_sum_ref(wavevectors, ring_pos[cur] - ring_pos[old]).real
            else:
                for i, (j, k) in enumerate(pairs):
                    if j == k:
                        cisf[lag, i] += (ring_rho[old, j] * ring_rho[cur, j].conj()).real
                        if incoherent:
                            iisf[lag, j] += fourier_sum_ref(
                                wavevectors, ring_pos[cur, slices[j]] - ring_pos[old, slices[j]]).real
                    else:
                        cisf[lag, i] += ((ring_rho[old, j] * ring_rho[cur, k].conj()).real
                                         + (ring_rho[old, k] * ring_rho[cur, j].conj()).real)
    norm = n_total * np.arange(n_frames, n_frames - n_lags, -1)[:, None, None]
    cisf /= norm
    if incoherent:
        iisf /= norm
    out_q = np.unique(wavenumbers.round(11)) if unique else wavenumbers
    if unique:
        cisf = np.stack([cisf[:, :, np.isclose(q, wavenumbers)].mean(axis=2) for q in out_q], axis=-1)
        if incoherent:
            iisf = np.stack([iisf[:, :, np.isclose(q, wavenumbers)].mean(axis=2) for q in out_q], axis=-1)
    if sort:
        order = np.argsort(out_q)
        out_q = out_q[order]
        cisf = cisf[:, :, order]
        if incoherent:
            iisf = iisf[:, :, order]
    return {"pairs": pairs, "wavenumbers": out_q, "cisf": cisf, "iisf": iisf}


# --------------------------------------------------------------------------------------------------
# The ISF engine's outputs straight from their definition (header comment of csrc/mdx_isf.hip): no ring, frames
# f and f - lag indexed directly, every phase, sine, cosine and sum in extended precision.

_WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


def _wide(a):
    return np.asarray(a, dtype=np.float64).astype(_WIDE or np.float64)


def _sum_rows(terms):
    """Sum over the last axis: in extended precision as it stands, else exactly rounded (math.fsum)."""
    if _WIDE is not None:
        return terms.sum(axis=-1)
    import math
    flat = terms.reshape(-1, terms.shape[-1])
    return np.array([math.fsum(row) for row in flat]).reshape(terms.shape[:-1])


def molecule_centres_ref(frames, mol_offsets, masses):
    """float32[F, n_molecules, 3]: the centres of mass as ``molecule_com_kernel`` (csrc/mdx_molecules.hpp) states
    them — a float64 sum of ``m * x`` over the rows of a molecule in row order with separate multiply and add, one
    division by the sequentially summed mass, cast to float32."""
    x = np.asarray(frames, dtype=np.float32).astype(np.float64)
    o = np.asarray(mol_offsets, dtype=np.int64)
    m = np.asarray(masses, dtype=np.float64)
    lens = np.diff(o)
    acc = np.zeros((x.shape[0], len(lens), 3))
    total = np.zeros(len(lens))
    for k in range(int(lens.max())):
        has = np.flatnonzero(lens > k)
        rows = o[has] + k
        acc[:, has] = acc[:, has] + m[rows][None, :, None] * x[:, rows]
        total[has] = total[has] + m[rows]
    return (acc / total[None, :, None]).astype(np.float32)


def isf_definition_ref(frames, group_offsets, pairs, wavevectors, n_lags):
    """
    Un-normalised ``cisf[lag][p][q]`` and ``iisf[lag][slot][q]`` of ``IsfEngine.result()``:

        rho_g(q, f) = sum_{j in g} exp(i q . r_j(f))
        cisf[lag][p] = sum_{f >= lag} Re rho_j(f - lag) rho_j(f)^*                                      p = (j, j)
                       sum_{f >= lag} Re rho_j(f - lag) rho_k(f)^* + Re rho_k(f - lag) rho_j(f)^*       p = (j, k)
                       sum_{f >= lag} Re rho(f - lag) rho(f)^*,  rho = sum_g rho_g                      p = (None, None)
        iisf[lag][g] = sum_{f >= lag} sum_{j in g} cos(q . (r_j(f) - r_j(f - lag)))

    frames : float32[F, n >= group_offsets[-1], 3] (rows beyond the groups' span are ignored); ``pairs``: ANY list
    of pairs of groups, or ``((None, None),)`` for the total mode.  The ``iisf`` slots are the engine's: one for the
    total mode, else one per group, zero for a group without a ``(g, g)`` pair.  Lags >= F are zero.

    The float32 coordinates are widened exactly; phases, sines, cosines and sums are formed in ``numpy.longdouble``
    where that is wider than float64 (x86), else in float64 with exactly rounded sums.

    Also returned, for error bounds: ``S_cisf`` = sum_f |rho_a(f - lag)| |rho_b(f)| (both orderings for a cross
    pair), ``S_iisf`` = slot size x number of frame pairs at the lag, ``phi_max`` = the largest |q . r| of a particle
    of a group in any frame.  All outputs float64.
    """
    x = _wide(np.asarray(frames, dtype=np.float32))
    q = _wide(np.asarray(wavevectors, dtype=np.float64).reshape(-1, 3))
    o = [int(v) for v in group_offsets]
    n_groups, n_q, n_frames = len(o) - 1, len(q), len(x)
    total_mode = pairs[0][0] is None
    dtype = x.dtype

    def phases(r):          # [..., n, 3] -> [..., n_q, n]
        return (q[:, None, 0] * r[..., None, :, 0] + q[:, None, 1] * r[..., None, :, 1]) + q[:, None, 2] * r[..., None, :, 2]

    # rho[f][g][q], cos and sin parts
    rc = np.zeros((n_frames, n_groups, n_q), dtype=dtype)
    rs = np.zeros((n_frames, n_groups, n_q), dtype=dtype)
    phi_max = 0.0
    for g in range(n_groups):
        if o[g + 1] == o[g]:
            continue
        for f in range(n_frames):
            ph = phases(x[f, o[g]:o[g + 1]])
            phi_max = max(phi_max, float(np.abs(ph).max()))
            rc[f, g] = _sum_rows(np.cos(ph))
            rs[f, g] = _sum_rows(np.sin(ph))
    if total_mode:
        rc = rc.sum(axis=1, keepdims=True)
        rs = rs.sum(axis=1, keepdims=True)
        use = [(0, 0)]
        slots = [(o[0], o[n_groups])]
    else:
        use = [(int(j), int(k)) for j, k in pairs]
        diagonal = {j for j, k in use if j == k}
        slots = [(o[g], o[g + 1]) if g in diagonal else (0, 0) for g in range(n_groups)]
    mod = np.sqrt(rc * rc + rs * rs)

    cisf = np.zeros((n_lags, len(use), n_q), dtype=dtype)
    s_cisf = np.zeros((n_lags, len(use), n_q), dtype=dtype)
    iisf = np.zeros((n_lags, len(slots), n_q), dtype=dtype)
    s_iisf = np.zeros((n_lags, len(slots), n_q))
    for lag in range(min(n_lags, n_frames)):
        old, new = slice(0, n_frames - lag), slice(lag, n_frames)
        for p, (j, k) in enumerate(use):
            re = rc[old, j] * rc[new, k] + rs[old, j] * rs[new, k]
            s = mod[old, j] * mod[new, k]
            if j != k:
                re = re + (rc[old, k] * rc[new, j] + rs[old, k] * rs[new, j])
                s = s + mod[old, k] * mod[new, j]
            cisf[lag, p] = re.sum(axis=0)
            s_cisf[lag, p] = s.sum(axis=0)
        for slot, (lo, hi) in enumerate(slots):
            if hi == lo:
                continue
            d = x[new, lo:hi] - x[old, lo:hi]                  # exact: float32 differences fit the wide type
            acc = np.zeros(n_q, dtype=dtype)
            for f in range(n_frames - lag):
                acc = acc + _sum_rows(np.cos(phases(d[f])))
            iisf[lag, slot] = acc
            s_iisf[lag, slot] = float(hi - lo) * (n_frames - lag)
    return {"cisf": cisf.astype(np.float64), "iisf": iisf.astype(np.float64),
            "S_cisf": s_cisf.astype(np.float64), "S_iisf": s_iisf, "phi_max": phi_max}


def ssf_definition_ref(frames, group_offsets, pairs, wavevectors, chain_length=0):
    """
    Un-normalised ``ssf[p][q]`` of ``SqEngine.result()`` straight from the definition (header comment of
    csrc/mdx_sq.hip):

        rho_g(q, f) = sum_{j in g} exp(i q . r_j(f))
        ssf[p] = sum_f |rho_j(f)|^2                                    p = (j, j)
                 sum_f 2 Re rho_j(f) rho_k(f)^*                        p = (j, k), j != k, in either order
                 sum_f |sum_g rho_g(f)|^2                              p = (None, None)
        ssf[0] = sum_f sum_c |rho_c(f)|^2, chain c = points [c L, (c + 1) L)      chain_length = L > 0

    frames : float32[F, n >= group_offsets[-1], 3] (rows beyond the groups' span are ignored); ``pairs``: ANY list
    of pairs of groups, or ``((None, None),)`` for the total mode (which the chain mode requires, with one group).

    The float32 coordinates are widened exactly; phases, sines, cosines and sums are formed in ``numpy.longdouble``
    where that is wider than float64 (x86), else in float64 with exactly rounded sums.

    Also returned, for error bounds: ``S[p][q]`` = sum_f (n_j |rho_k| + n_k |rho_j|) with n the group sizes (total
    mode: 2 N |rho|; chains: sum_f sum_c 2 L |rho_c|) — the first-order effect on ssf of errors of n eps in every
    rho, whatever the configuration — and ``phi_max``, the largest |q . r| of a particle of a group in any frame.
    All outputs float64.
    """
    x = _wide(np.asarray(frames, dtype=np.float32))
    q = _wide(np.asarray(wavevectors, dtype=np.float64).reshape(-1, 3))
    o = [int(v) for v in group_offsets]
    n_groups, n_q, n_frames = len(o) - 1, len(q), len(x)
    dtype = x.dtype
    phi_max = 0.0

    def rho(r):
        """[F, ..., n, 3] -> cos and sin sums [F, ..., n_q], a slab of frames at a time (bounded memory)."""
        nonlocal phi_max
        rc = np.zeros(r.shape[:-2] + (n_q,), dtype=dtype)
        rs = np.zeros_like(rc)
        per_frame = max(1, int(np.prod(r.shape[1:-1])) * n_q)
        step = max(1, (1 << 21) // per_frame)
        for f0 in range(0, len(r), step):
            s = r[f0:f0 + step]
            ph = (q[:, None, 0] * s[..., None, :, 0] + q[:, None, 1] * s[..., None, :, 1]) + q[:, None, 2] * s[..., None, :, 2]
            if ph.size:
                phi_max = max(phi_max, float(np.abs(ph).max()))
            rc[f0:f0 + step] = _sum_rows(np.cos(ph))
            rs[f0:f0 + step] = _sum_rows(np.sin(ph))
        return rc, rs

    if chain_length > 0:
        n_total = o[n_groups]
        assert n_groups == 1 and pairs[0][0] is None and n_total % chain_length == 0
        rc, rs = rho(x[:, o[0]:n_total].reshape(n_frames, n_total // chain_length, chain_length, 3))
        ssf = (rc * rc + rs * rs).sum(axis=(0, 1))[None]
        scale = (2 * chain_length * np.sqrt(rc * rc + rs * rs)).sum(axis=(0, 1))[None]
        return {"ssf": ssf.astype(np.float64), "S": scale.astype(np.float64), "phi_max": phi_max}

    rc = np.zeros((n_groups, n_frames, n_q), dtype=dtype)
    rs = np.zeros((n_groups, n_frames, n_q), dtype=dtype)
    for g in range(n_groups):
        if o[g + 1] > o[g]:
            rc[g], rs[g] = rho(x[:, o[g]:o[g + 1]])
    sizes = [o[g + 1] - o[g] for g in range(n_groups)]
    if pairs[0][0] is None:
        rc, rs = rc.sum(axis=0, keepdims=True), rs.sum(axis=0, keepdims=True)
        sizes, use = [o[n_groups] - o[0]], [(0, 0)]
    else:
        use = [(int(j), int(k)) for j, k in pairs]
    mod = np.sqrt(rc * rc + rs * rs)
    ssf = np.zeros((len(use), n_q), dtype=dtype)
    scale = np.zeros((len(use), n_q), dtype=dtype)
    for p, (j, k) in enumerate(use):
        re = rc[j] * rc[k] + rs[j] * rs[k]
        ssf[p] = (re if j == k else 2 * re).sum(axis=0)
        scale[p] = (sizes[j] * mod[k] + sizes[k] * mod[j]).sum(axis=0)
    return {"ssf": ssf.astype(np.float64), "S": scale.astype(np.float64), "phi_max": phi_max}
