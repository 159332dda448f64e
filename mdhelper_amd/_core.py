"""
Thin object wrappers over the C-ABI handles of ``libmdx.so``: device arrays,
the RCCL communicator and the three analysis engines.  Host-side glue only —
all arithmetic happens in the HIP library.
"""

from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int, c_int64, c_size_t, c_void_p

import numpy as np

from . import _lib
from ._lib import check, lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


class DeviceArray:
    """A typed HBM allocation (``mdx_malloc``); inputs of the ``*_device`` entry points."""

    def __init__(self, shape, dtype, dev: int = 0):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.dev = dev
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = c_void_p()
        check(lib().mdx_malloc(dev, self.nbytes, byref(p)))
        self.ptr = p

    @classmethod
    def from_host(cls, arr, dev: int = 0):
        arr = np.ascontiguousarray(arr)
        out = cls(arr.shape, arr.dtype, dev)
        check(lib().mdx_memcpy_h2d(dev, out.ptr, _ptr(arr), arr.nbytes))
        return out

    @classmethod
    def upload(cls, arr, dev: int = 0):
        """Large host arrays: through the library's pinned ring and its copy threads, or by one DMA
        when the array is page-locked (``mdx_upload``)."""
        arr = np.ascontiguousarray(arr)
        out = cls(arr.shape, arr.dtype, dev)
        try:
            check(lib().mdx_upload(dev, out.ptr, _ptr(arr), arr.nbytes))
        except Exception:
            out.free()
            raise
        return out

    def upload_columns(self, host, first: int, count: int):
        """Fill this array ``[T, count, ...]`` with columns ``[first, first + count)`` of the host array
        ``[T, N, ...]`` (``mdx_upload_rows``: rows of >= 4 KB in pageable anonymous memory are page-locked, read by 2-D DMA
        and unlocked slice by slice; page-locked memory: one 2-D DMA; short rows, file mappings: copy threads + pinned ring)."""
        host = np.asarray(host)
        if host.dtype != self.dtype or not host.flags.c_contiguous or host.shape[0] != self.shape[0] \
                or host.shape[2:] != self.shape[2:] or self.shape[1] != count \
                or not 0 <= first <= first + count <= host.shape[1]:
            raise ValueError("upload_columns: shapes / dtype do not match")
        item = int(np.prod(host.shape[2:], dtype=np.int64)) * host.dtype.itemsize
        src = c_void_p(host.ctypes.data + first * item)
        check(lib().mdx_upload_rows(self.dev, self.ptr, src, count * item, host.shape[1] * item, host.shape[0]))

    def to_host(self, first: int = 0, count: int | None = None):
        """Copy rows [first, first+count) of the leading axis back to the host."""
        n0 = self.shape[0]
        count = n0 - first if count is None else count
        row = self.nbytes // max(n0, 1)
        out = np.empty((count,) + self.shape[1:], dtype=self.dtype)
        src = c_void_p(self.ptr.value + first * row)
        check(lib().mdx_memcpy_d2h(self.dev, _ptr(out), src, count * row))
        return out

    def offset(self, first: int):
        """Raw pointer to row ``first`` of the leading axis."""
        row = self.nbytes // max(self.shape[0], 1)
        return c_void_p(self.ptr.value + first * row)

    @staticmethod
    def view(base, shape):
        """The leading bytes of ``base`` as an array of another shape (same dtype) that does not own its memory."""
        v = object.__new__(_DeviceView)
        v.shape = tuple(int(x) for x in shape)
        v.dtype, v.dev = base.dtype, base.dev
        v.nbytes = int(np.prod(v.shape)) * base.dtype.itemsize
        if v.nbytes > base.nbytes:
            raise ValueError("view larger than its base")
        v.ptr = c_void_p(base.ptr.value)
        v.base = base
        return v

    def rows(self, first: int, count: int):
        """Rows [first, first+count) of the leading axis as a DeviceArray that does not own its memory
        (valid as long as this one is)."""
        if not 0 <= first <= first + count <= self.shape[0]:
            raise IndexError("rows out of range")
        view = object.__new__(_DeviceView)
        view.shape = (int(count),) + self.shape[1:]
        view.dtype, view.dev = self.dtype, self.dev
        view.nbytes = self.nbytes // max(self.shape[0], 1) * int(count)
        view.ptr = self.offset(first)
        view.base = self
        return view

    def free(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            lib().mdx_free(self.dev, self.ptr)
            self.ptr = c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceView(DeviceArray):
    """Non-owning window into a DeviceArray (``DeviceArray.rows``)."""

    def free(self):
        self.ptr = c_void_p()


def device_info(dev: int = 0):
    name = ctypes.create_string_buffer(256)
    cus = c_int()
    total = c_size_t()
    free = c_size_t()
    check(lib().mdx_device_info(dev, name, 256, byref(cus), byref(total), byref(free)))
    cached = c_size_t()
    check(lib().mdx_cached_bytes(dev, byref(cached)))
    # hbm_free_bytes: what the driver reports; hbm_cached_bytes: blocks of destroyed handles this process keeps
    # (mdx_trim_cache) — the library's own allocations can take them, nobody else can
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": total.value,
            "hbm_free_bytes": free.value, "hbm_cached_bytes": cached.value,
            "hbm_available_bytes": free.value + cached.value}


def synchronize(dev: int = 0):
    check(lib().mdx_device_synchronize(dev))


def synth_random_walk(n_frames, n_atoms, box_lengths, sigma, seed, *, wrap=True, dev=0,
                      dtype=np.float32):
    """Synthetic trajectory generated in HBM (``mdx_synth_random_walk``)."""
    out = DeviceArray((n_frames, n_atoms, 3), dtype, dev)
    L = (ctypes.c_float * 3)(*[float(x) for x in box_lengths])
    if np.dtype(dtype) == np.float32:
        check(lib().mdx_synth_random_walk(dev, out.ptr, n_frames, n_atoms, L, float(sigma),
                                          int(seed), int(bool(wrap))))
    else:
        check(lib().mdx_synth_random_walk_f64(dev, out.ptr, n_frames, n_atoms, L, float(sigma),
                                              int(seed)))
    return out


class RcclComm:
    """One rank of an RCCL communicator (``mdx_comm_*``)."""

    device_collectives = True

    def __init__(self, rank: int, world_size: int, unique_id: bytes, dev: int = 0):
        assert len(unique_id) == 128
        self.rank, self.world_size, self.dev = rank, world_size, dev
        buf = ctypes.create_string_buffer(unique_id, 128)
        h = c_void_p()
        check(lib().mdx_comm_init_rank(byref(h), dev, buf, rank, world_size))
        self.handle = h

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        check(lib().mdx_comm_unique_id(buf))
        return buf.raw

    def barrier(self):
        check(lib().mdx_comm_barrier(self.handle))

    def rccl_info(self):
        """(ranks, this rank, device) as RCCL reports them for the communicator."""
        n, r, d = c_int(), c_int(), c_int()
        check(lib().mdx_comm_count(self.handle, byref(n), byref(r), byref(d)))
        return n.value, r.value, d.value

    def allreduce(self, arr, op="sum"):
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.int64 and op == "sum":
            check(lib().mdx_comm_allreduce_i64(self.handle, _ptr(arr), arr.size))
        else:
            arr = arr.astype(np.float64)
            check(lib().mdx_comm_allreduce_f64(self.handle, _ptr(arr), arr.size, int(op == "max")))
        return arr

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().mdx_comm_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Engine:
    _destroy = None

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            getattr(lib(), self._destroy)(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RdfEngine(_Engine):
    """``mdx_rdf_*``: pair-distance histogram accumulated over batches of frames."""

    _destroy = "mdx_rdf_destroy"

    def __init__(self, edges, exclusion=None, *, algo="auto", dev=0, timing=False):
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        self.n_bins = self.edges.size - 1
        e1, e2 = (0, 0) if exclusion is None else (int(exclusion[0]), int(exclusion[1]))
        h = c_void_p()
        check(lib().mdx_rdf_create(byref(h), dev, self.n_bins, _ptr(self.edges), e1, e2,
                                   _lib.RDF_ALGO[algo]))
        self.handle = h
        self.dev = dev
        if timing:
            check(lib().mdx_rdf_enable_timing(h, 1))

    PLAN_FIELDS = ("family", "ipt", "self", "excl", "pbc", "lower", "skip", "gh", "n_hist", "lds_bytes",
                   "lds_attribute", "n1_pad", "n2_pad", "tiles1", "tiles2", "chunk", "grid_x", "slab_frames",
                   "n_slabs", "lazy_orig")
    FAMILIES = ("tile-exact", "tile-filter", "cell-ortho", "tri-brute", "tri-culled")

    @staticmethod
    def plan(edges, exclusion, algo, n1, n2=None, boxes=None, n_frames=1):
        """``mdx_rdf_plan``: the pair kernel an engine built from ``edges``, ``exclusion`` and ``algo`` launches for ONE
        run of ``n_frames`` frames of one cell kind, as a dict of ``PLAN_FIELDS`` — ``family`` indexes ``FAMILIES``.
        ``n2=None``: one set against itself.  ``boxes``: ``None``, one cell or ``float32[n_frames, 6]``.  Needs no
        device; reads ``MDX_RDF_SLAB_BYTES`` / ``MDX_RDF_TRI_BRUTE`` / ``MDX_RDF_CHUNK_TILES`` as the engine does."""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        e1, e2 = (0, 0) if exclusion is None else (int(exclusion[0]), int(exclusion[1]))
        b = None
        if boxes is not None:
            b = np.ascontiguousarray(np.broadcast_to(np.asarray(boxes, dtype=np.float32), (int(n_frames), 6)))
        out = np.zeros(24, dtype=np.int64)
        check(lib().mdx_rdf_plan(e.size - 1, _ptr(e), e1, e2, _lib.RDF_ALGO[algo], int(n1),
                                 int(n1 if n2 is None else n2), int(n2 is None), _ptr(b), int(n_frames), _ptr(out)))
        return dict(zip(RdfEngine.PLAN_FIELDS, (int(v) for v in out)))

    def last_plan(self):
        """``mdx_rdf_last_plan``: the plan of this engine's most recent run as it was launched, the dict ``plan()``
        returns; an error before any run and after ``reset()``."""
        out = np.zeros(24, dtype=np.int64)
        check(lib().mdx_rdf_last_plan(self.handle, _ptr(out)))
        return dict(zip(RdfEngine.PLAN_FIELDS, (int(v) for v in out)))

    FILTER_FIELDS = ("eta", "sure_w", "tq", "inv_w", "pos0", "iwq", "p0q", "cand_hi", "cand_lo")

    @staticmethod
    def filter_constants(edges, box, max_abs):
        """``mdx_rdf_filter_constants``: the float32 filter constants of the cell-sorted pair kernel for one
        orthorhombic frame with cell lengths ``box`` and a largest |coordinate| of ``max_abs``, as a dict of
        ``FILTER_FIELDS`` (``tq`` an int, the others the float32 values as Python floats).  Needs no device."""
        e = np.ascontiguousarray(edges, dtype=np.float64)
        b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).ravel()[:3])
        out = np.zeros(10, dtype=np.float64)
        check(lib().mdx_rdf_filter_constants(e.size - 1, float(e[0]), float(e[-1]), _ptr(b), float(max_abs),
                                             _ptr(out)))
        d = dict(zip(RdfEngine.FILTER_FIELDS, (float(v) for v in out)))
        d["tq"] = int(d["tq"])
        return d

    def accumulate(self, pos1, pos2=None, boxes=None):
        """pos: float32[F, N, 3] (host); boxes float32[F, 6] or None."""
        p1 = np.ascontiguousarray(pos1, dtype=np.float32)
        if p1.ndim == 2:
            p1 = p1[None]
        F, n1 = p1.shape[0], p1.shape[1]
        if pos2 is None or pos2 is pos1:
            p2, n2 = None, n1
        else:
            p2 = np.ascontiguousarray(pos2, dtype=np.float32)
            if p2.ndim == 2:
                p2 = p2[None]
            n2 = p2.shape[1]
            if p2.shape[0] != F:
                raise ValueError("pos1 and pos2 must hold the same number of frames.")
        b = None
        if boxes is not None:
            b = np.ascontiguousarray(np.broadcast_to(np.asarray(boxes, dtype=np.float32), (F, 6)))
        check(lib().mdx_rdf_accumulate(self.handle, _ptr(p1), n1, _ptr(p2), n2, _ptr(b), F))

    def accumulate_device(self, d_pos1, n1, d_pos2, n2, d_boxes, n_frames):
        check(lib().mdx_rdf_accumulate_device(self.handle, d_pos1, n1, d_pos2, n2, d_boxes, n_frames))

    def set_drop_axis(self, axis):
        """2-D mode: coordinate ``axis`` (0, 1, 2; ``None`` = off) is zeroed on the device and the
        cell length along it set to the largest one (``mdx_rdf_set_drop_axis``)."""
        check(lib().mdx_rdf_set_drop_axis(self.handle, -1 if axis is None else int(axis)))

    def set_grouping(self, which, offsets, masses):
        """Rows of set ``which`` (1 or 2) become particles of molecules ``[offsets[g], offsets[g+1])``
        whose centres of mass are binned; ``offsets=None`` removes the grouping."""
        if offsets is None:
            check(lib().mdx_rdf_set_grouping(self.handle, which, 0, None, None))
            return
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != o[-1]:
            raise ValueError("masses must hold one entry per particle of the grouping.")
        check(lib().mdx_rdf_set_grouping(self.handle, which, len(o) - 1, _ptr(o), _ptr(m)))

    def accumulate_traj(self, traj_file, frames, boxes, index1=None, index2=None, same=True):
        """Frames of a native trajectory file (``io.TrajectoryFile``); ``index``: particle
        selections (None = all particles), ``same``: one group against itself."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        b = None if boxes is None else np.ascontiguousarray(boxes, dtype=np.float32)
        i1 = None if index1 is None else np.ascontiguousarray(index1, dtype=np.int32)
        i2 = None if (same or index2 is None) else np.ascontiguousarray(index2, dtype=np.int32)
        n1 = 0 if i1 is None else len(i1)
        # index2 NULL with n2 == 0 means "the same group twice"; n2 < 0 can never mean that
        n2 = 0 if same else (traj_file.n_atoms if i2 is None else len(i2))
        check(lib().mdx_rdf_accumulate_traj(self.handle, traj_file.handle, _ptr(f), len(f), _ptr(b),
                                            _ptr(i1), n1, _ptr(i2), n2))

    def counts(self):
        out = np.zeros(self.n_bins, dtype=np.int64)
        check(lib().mdx_rdf_counts(self.handle, _ptr(out)))
        return out

    def synchronize(self):
        check(lib().mdx_rdf_synchronize(self.handle))

    def reset(self):
        check(lib().mdx_rdf_reset(self.handle))

    def allreduce(self, comm: RcclComm):
        check(lib().mdx_rdf_allreduce(self.handle, comm.handle))

    def stats(self):
        n, ms, pe, px, pc = c_int64(), c_double(), c_int64(), c_int64(), c_int64()
        check(lib().mdx_rdf_stats(self.handle, byref(n), byref(ms), byref(pe), byref(px), byref(pc)))
        raw = np.zeros(4, dtype=np.int64)
        check(lib().mdx_rdf_debug_counters(self.handle, _ptr(raw)))
        hz = c_double()
        check(lib().mdx_rdf_kernel_clock(self.handle, byref(hz)))
        beside = c_int64()
        check(lib().mdx_rdf_slabs_sorted_beside(self.handle, byref(beside)))
        return {"launches": n.value, "kernel_ms": ms.value, "pairs_evaluated": pe.value,
                "pairs_exact": px.value, "pairs_computed": pc.value,
                "cell_units": int(raw[1]), "cell_units_general": int(raw[2]),
                "slabs_sorted_beside": beside.value, "clock_hz": hz.value}


def radial_histogram_device(pos1, pos2, n_bins, edges, dims, exclusion=None, dev=0):
    """``mdx_radial_histogram``: one frame, host buffers."""
    p1 = np.ascontiguousarray(pos1, dtype=np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(pos2, dtype=np.float32).reshape(-1, 3)
    box = None if dims is None else np.ascontiguousarray(dims, dtype=np.float32).reshape(6)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    e1, e2 = (0, 0) if exclusion is None else (int(exclusion[0]), int(exclusion[1]))
    counts = np.zeros(n_bins, dtype=np.int64)
    same = pos2 is pos1
    check(lib().mdx_radial_histogram(dev, _ptr(p1), p1.shape[0], _ptr(p1 if same else p2),
                                     p2.shape[0], n_bins, _ptr(edges), _ptr(box), e1, e2,
                                     _ptr(counts)))
    return counts


class SqEngine(_Engine):
    """``mdx_sq_*``: fused exp(i q.r) accumulation and pair products."""

    _destroy = "mdx_sq_destroy"

    def __init__(self, wavevectors, group_sizes, pairs, *, dev=0, timing=False):
        self.q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        self.offsets = np.concatenate(([0], np.cumsum(group_sizes))).astype(np.int64)
        self.pairs = np.ascontiguousarray(
            [(-1, -1) if p[0] is None else (int(p[0]), int(p[1])) for p in pairs], dtype=np.int32)
        h = c_void_p()
        check(lib().mdx_sq_create(byref(h), dev, _ptr(self.q), self.q.shape[0], _ptr(self.offsets),
                                  len(group_sizes), _ptr(self.pairs), self.pairs.shape[0]))
        self.handle = h
        self.dev = dev
        if timing:
            check(lib().mdx_sq_enable_timing(h, 1))

    PLAN_FIELDS = ("route", "regular_stride", "tile", "n_sub", "items_per_block", "blocks", "threads", "n_split",
                   "slab_frames", "chains_per_part")
    ROUTES = ("general", "tables", "columns", "quads")

    @staticmethod
    def plan(wavevectors, group_sizes, n_frames, chain_length=0):
        """``mdx_sq_plan``: the kernels an engine built from these arguments launches for ONE accumulate call of
        ``n_frames`` frames, as a dict of ``PLAN_FIELDS`` — ``route`` indexes ``ROUTES`` (in the single-chain mode,
        ``chain_length > 0``: ``general`` is the sincos kernel, ``quads`` the quad kernel).  Needs no device; reads
        ``MDX_SQ_NO_LATTICE`` / ``MDX_SQ_NO_COLUMNS`` / ``MDX_SQ_NO_QUADS`` as the constructor does."""
        q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        sizes = [int(s) for s in group_sizes]
        out = np.zeros(10, dtype=np.int32)
        check(lib().mdx_sq_plan(_ptr(q), q.shape[0], len(sizes), max(sizes), sum(sizes), int(chain_length),
                                int(n_frames), _ptr(out)))
        return dict(zip(SqEngine.PLAN_FIELDS, (int(v) for v in out)))

    _set_grouping = "mdx_sq_set_grouping"

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of molecules ``[offsets[g], offsets[g+1])`` whose float32
        centres of mass enter the Fourier sums; ``offsets=None`` removes the grouping."""
        fn = getattr(lib(), self._set_grouping)
        if offsets is None:
            check(fn(self.handle, 0, None, None))
            return
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != o[-1]:
            raise ValueError("masses must hold one entry per particle of the grouping.")
        check(fn(self.handle, len(o) - 1, _ptr(o), _ptr(m)))

    def set_chains(self, chain_length):
        """Single-chain mode (``mdx_sq_set_chains``): the points form chains of ``chain_length``
        consecutive points and ``result()[0]`` is the sum over frames of ``sum_c |rho_c(q)|^2``;
        ``chain_length <= 0`` restores the normal mode.  Only before the first frame."""
        check(lib().mdx_sq_set_chains(self.handle, int(chain_length)))

    def accumulate(self, pos):
        p = np.ascontiguousarray(pos, dtype=np.float32)
        if p.ndim == 2:
            p = p[None]
        check(lib().mdx_sq_accumulate(self.handle, _ptr(p), p.shape[1], p.shape[0]))

    def accumulate_device(self, d_pos, n, n_frames):
        """Asynchronous on the engine's stream: ``synchronize()`` before the frames are overwritten."""
        check(lib().mdx_sq_accumulate_device(self.handle, d_pos, n, n_frames))

    def synchronize(self):
        check(lib().mdx_sq_synchronize(self.handle))

    def accumulate_traj(self, traj_file, frames, index=None):
        """Frames of a native trajectory file; ``index``: particles in concatenated-group order."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        check(lib().mdx_sq_accumulate_traj(self.handle, traj_file.handle, _ptr(f), len(f), _ptr(i),
                                           0 if i is None else len(i)))

    def result(self):
        out = np.zeros((self.pairs.shape[0], self.q.shape[0]), dtype=np.float64)
        check(lib().mdx_sq_result(self.handle, _ptr(out)))
        return out

    def reset(self):
        check(lib().mdx_sq_reset(self.handle))

    def allreduce(self, comm: RcclComm):
        check(lib().mdx_sq_allreduce(self.handle, comm.handle))

    def stats(self):
        n, ms = c_int64(), c_double()
        check(lib().mdx_sq_stats(self.handle, byref(n), byref(ms)))
        return {"launches": n.value, "kernel_ms": ms.value}


class IsfEngine(_Engine):
    """``mdx_isf_*``: coherent / incoherent intermediate scattering functions."""

    _destroy = "mdx_isf_destroy"

    def __init__(self, wavevectors, group_sizes, pairs, n_lags, incoherent=False, *, dev=0,
                 timing=False):
        self.q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        self.offsets = np.concatenate(([0], np.cumsum(group_sizes))).astype(np.int64)
        self.pairs = np.ascontiguousarray(
            [(-1, -1) if p[0] is None else (int(p[0]), int(p[1])) for p in pairs], dtype=np.int32)
        self.n_lags = int(n_lags)
        self.incoherent = bool(incoherent)
        self.n_slots = 1 if self.pairs[0, 0] < 0 else len(group_sizes)
        h = c_void_p()
        check(lib().mdx_isf_create(byref(h), dev, _ptr(self.q), self.q.shape[0], _ptr(self.offsets),
                                   len(group_sizes), _ptr(self.pairs), self.pairs.shape[0],
                                   self.n_lags, int(self.incoherent)))
        self.handle = h
        self.dev = dev
        if timing:
            check(lib().mdx_isf_enable_timing(h, 1))

    PLAN_FIELDS = ("route", "regular_stride", "tile", "n_sub", "items_per_block", "blocks", "rho_split",
                   "incoherent_split")
    ROUTES = ("general", "tables", "quads")

    @staticmethod
    def plan(wavevectors, group_sizes, pairs, n_lags, n_new=None):
        """``mdx_isf_plan``: the kernels an engine built from these arguments launches for a chunk of ``n_new`` new
        frames (default: ``n_lags``, a full chunk), as a dict of ``PLAN_FIELDS`` — ``route`` indexes ``ROUTES``.
        Needs no device; reads ``MDX_SQ_NO_LATTICE`` / ``MDX_ISF_NO_QUADS`` as the constructor does."""
        q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        sizes = [int(s) for s in group_sizes]
        if pairs[0][0] is None:
            ranges = [sum(sizes)]
        else:
            diagonal = {int(j) for j, k in pairs if int(j) == int(k)}
            ranges = [s if g in diagonal else 0 for g, s in enumerate(sizes)]
        out = np.zeros(8, dtype=np.int32)
        check(lib().mdx_isf_plan(_ptr(q), q.shape[0], len(sizes), len(ranges), int(n_lags), max(sizes),
                                 max(ranges), int(n_lags if n_new is None else n_new), _ptr(out)))
        return dict(zip(IsfEngine.PLAN_FIELDS, (int(v) for v in out)))

    _set_grouping = "mdx_isf_set_grouping"

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of molecules ``[offsets[g], offsets[g+1])`` whose float32
        centres of mass enter the Fourier sums; ``offsets=None`` removes the grouping."""
        fn = getattr(lib(), self._set_grouping)
        if offsets is None:
            check(fn(self.handle, 0, None, None))
            return
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != o[-1]:
            raise ValueError("masses must hold one entry per particle of the grouping.")
        check(fn(self.handle, len(o) - 1, _ptr(o), _ptr(m)))

    def accumulate(self, pos):
        """pos: float32[F, N, 3], frames in analysis order."""
        p = np.ascontiguousarray(pos, dtype=np.float32)
        if p.ndim == 2:
            p = p[None]
        check(lib().mdx_isf_accumulate(self.handle, _ptr(p), p.shape[1], p.shape[0]))

    def accumulate_device(self, d_pos, n, n_frames):
        """float32[n_frames][n][3] already in HBM (raw device pointer).  Asynchronous on the engine's
        stream: ``synchronize()`` before the frames are overwritten."""
        check(lib().mdx_isf_accumulate_device(self.handle, d_pos, n, n_frames))

    def synchronize(self):
        check(lib().mdx_isf_synchronize(self.handle))

    def accumulate_traj(self, traj_file, frames, index=None):
        """Frames (in analysis order) of a native trajectory file; ``index`` as for SqEngine."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        check(lib().mdx_isf_accumulate_traj(self.handle, traj_file.handle, _ptr(f), len(f), _ptr(i),
                                            0 if i is None else len(i)))

    def result(self):
        cisf = np.zeros((self.n_lags, self.pairs.shape[0], self.q.shape[0]))
        iisf = np.zeros((self.n_lags, self.n_slots, self.q.shape[0])) if self.incoherent else None
        check(lib().mdx_isf_result(self.handle, _ptr(cisf), _ptr(iisf)))
        return cisf, iisf

    def reset(self):
        check(lib().mdx_isf_reset(self.handle))

    def stats(self):
        n, ms, fr = c_int64(), c_double(), c_int64()
        check(lib().mdx_isf_stats(self.handle, byref(n), byref(ms), byref(fr)))
        return {"launches": n.value, "kernel_ms": ms.value, "frames": fr.value}


def feed_slab_frames(n_frames, rows):
    """``mdx_feed_slab_frames``: the frames a per-frame engine stages at a time when ``accumulate`` (``rows``: the
    rows of a frame) or ``accumulate_traj`` (``rows``: the file's atoms) is given ``n_frames`` frames.  Needs no
    device."""
    out = c_int64()
    check(lib().mdx_feed_slab_frames(int(n_frames), int(rows), byref(out)))
    return out.value


def _chain_layout(n_chains, n_monomers):
    """``(n_chains, n_monomers)`` as int64 arrays of one entry per group."""
    c = np.ascontiguousarray(np.atleast_1d(n_chains), dtype=np.int64)
    m = np.ascontiguousarray(np.atleast_1d(n_monomers), dtype=np.int64)
    if c.ndim != 1 or c.shape != m.shape or len(c) == 0:
        raise ValueError("n_chains and n_monomers must hold one entry per group.")
    return c, m


class _FrameEngine(_Engine):
    """What the per-frame engines share: the three routes frames take (host memory, HBM, a trajectory file),
    ``synchronize``, ``reset``, ``stats`` and the ``timing=`` switch.  A subclass names the prefix of its symbols and
    what its ``mdx_X_stats`` reports behind launches, kernel time and frames."""

    _prefix = None
    _stats_extra = ()       # (key, ctype) of every further field of mdx_X_stats, in its order

    @property
    def _destroy(self):
        return f"{self._prefix}_destroy"

    def _fn(self, name):
        return getattr(lib(), f"{self._prefix}_{name}")

    def _adopt(self, handle, dev, timing):
        """The tail of every constructor: keeps the created handle and switches the event timers on."""
        self.handle = handle
        self.dev = dev
        if timing:
            check(self._fn("enable_timing")(handle, 1))

    def accumulate(self, pos):
        """pos: float32[F, N, 3], rows in the engine's incoming order (concatenated groups unless its class says
        otherwise)."""
        p = np.ascontiguousarray(pos, dtype=np.float32)
        if p.ndim == 2:
            p = p[None]
        check(self._fn("accumulate")(self.handle, _ptr(p), p.shape[1], p.shape[0]))

    def accumulate_device(self, d_pos, n_atoms, n_frames, index=None):
        """Frames in HBM, read where they lie (``index``: rows of a frame in incoming order).  Asynchronous on
        the engine's stream: ``synchronize()`` before the frames are overwritten."""
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        check(self._fn("accumulate_device")(self.handle, d_pos, n_atoms, n_frames, _ptr(i),
                                            0 if i is None else len(i)))

    def accumulate_traj(self, traj_file, frames, index=None):
        """Frames of a native trajectory file; ``index``: particles in incoming order."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        check(self._fn("accumulate_traj")(self.handle, traj_file.handle, _ptr(f), len(f), _ptr(i),
                                          0 if i is None else len(i)))

    def synchronize(self):
        check(self._fn("synchronize")(self.handle))

    def reset(self):
        check(self._fn("reset")(self.handle))

    def _set_grouping(self, name, offsets, masses):
        """``mdx_X_<name>(handle, n_groups, offsets, masses)``; ``offsets=None`` removes the grouping."""
        if offsets is None:
            check(self._fn(name)(self.handle, 0, None, None))
            return
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != o[-1]:
            raise ValueError("masses must hold one entry per particle of the grouping.")
        check(self._fn(name)(self.handle, len(o) - 1, _ptr(o), _ptr(m)))

    def _set_unwrap(self, name, dims, start):
        """``mdx_X_<name>(handle, dims, start)`` with ``start`` float64 ``[n_points, 3]``; ``dims=None`` switches the
        unwrap off."""
        if dims is None:
            check(self._fn(name)(self.handle, None, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        s = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
        if s is None or s.shape != (self.n_points, 3):
            raise ValueError("start must hold three coordinates per point of the groups.")
        check(self._fn(name)(self.handle, _ptr(d), _ptr(s)))

    def stats(self):
        keys = ("launches", "kernel_ms", "frames") + tuple(key for key, _ in self._stats_extra)
        out = [c_int64(), c_double(), c_int64()] + [ctype() for _, ctype in self._stats_extra]
        check(self._fn("stats")(self.handle, *map(byref, out)))
        return {key: value.value for key, value in zip(keys, out)}


class _SlabbedFrameEngine(_FrameEngine):
    """... of which these export ``mdx_X_set_slab_frames``."""

    def set_slab_frames(self, frames):
        """Frames per kernel launch at most; 0 restores the default.  The results do not depend on it.  Every
        engine but the dipole one takes it only before the first frame."""
        check(self._fn("set_slab_frames")(self.handle, int(frames)))

    def plan(self):
        """``mdx_X_plan``: where the next call is cut.  ``slab_frames``: frames per kernel launch at most;
        ``ring_frames``: frames in the ring of a lag engine (``max(lags) + slab``, decided before the first frame of a
        pass), 0 for an engine without one.  Needs no device and reads no frame."""
        slab, ring = c_int64(), c_int64()
        check(self._fn("plan")(self.handle, byref(slab), byref(ring)))
        return {"slab_frames": slab.value, "ring_frames": ring.value}


class ProfileEngine(_FrameEngine):
    """``mdx_prof_*``: per-axis, per-group position histograms with ``numpy.histogram``'s counts."""

    _prefix = "mdx_prof"
    _stats_extra = (("replicas", c_int),)

    def __init__(self, group_sizes, axes, n_bins, dims, *, per_frame=False, dev=0, timing=False, replicas=None):
        self.offsets = np.concatenate(([0], np.cumsum(group_sizes))).astype(np.int64)
        self.axes = np.ascontiguousarray(np.atleast_1d(axes), dtype=np.int32)
        self.n_bins = np.ascontiguousarray(np.broadcast_to(n_bins, self.axes.shape), dtype=np.int64)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.n_groups = len(self.offsets) - 1
        self.per_frame = bool(per_frame)
        h = c_void_p()
        check(lib().mdx_prof_create(byref(h), dev, self.n_groups, _ptr(self.offsets), len(self.axes),
                                    _ptr(self.axes), _ptr(self.n_bins), _ptr(self.dims), int(self.per_frame)))
        self._adopt(h, dev, timing)
        if replicas is not None:
            self.set_replicas(replicas)

    @staticmethod
    def slab_frames(n_points, *, grouped=False, recenter=False):
        """``mdx_prof_slab_frames``: the frames per kernel launch inside one call of an engine whose groups hold
        ``n_points`` points, with a grouping and / or recentring set.  Needs no device."""
        out = c_int64()
        check(lib().mdx_prof_slab_frames(int(n_points), int(bool(grouped)), int(bool(recenter)), byref(out)))
        return out.value

    def set_replicas(self, replicas):
        """Caps the LDS copies of the counters (8, 4, 2, 1), 0: global atomics, -1: the engine's own choice.
        For measurements and tests: the counts do not depend on it."""
        check(lib().mdx_prof_set_replicas(self.handle, int(replicas)))

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of molecules ``[offsets[m], offsets[m+1])`` — one per point of the
        groups — whose float64 centres of mass are binned; ``offsets=None`` removes the grouping."""
        self._set_grouping("set_grouping", offsets, masses)

    def set_recenter(self, group, masses=None, target=None):
        """Every frame is shifted so that the mass-weighted centre of the globally unwrapped points of
        ``group`` sits at ``target`` (a NaN component leaves that axis alone); ``group=None`` switches it
        off.  Frames must then be fed in analysis order."""
        if group is None:
            check(lib().mdx_prof_set_recenter(self.handle, -1, None, None))
            return
        group = int(group)
        if not 0 <= group < self.n_groups:
            raise ValueError("Invalid group index.")
        n = int(self.offsets[group + 1] - self.offsets[group])
        m = np.ones(n) if masses is None else np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != n:
            raise ValueError("masses must hold one entry per point of the group.")
        t = np.ascontiguousarray(self.dims / 2 if target is None else target, dtype=np.float64)
        if t.shape != (3,):
            raise ValueError("target must hold three coordinates.")
        check(lib().mdx_prof_set_recenter(self.handle, group, _ptr(m), _ptr(t)))

    def counts(self):
        """One int64 array per axis: ``[G, n_bins]``, or ``[G, frames seen, n_bins]`` for per-frame engines."""
        frames = self.stats()["frames"]
        out = []
        for slot, nb in enumerate(self.n_bins):
            shape = (self.n_groups, frames, int(nb)) if self.per_frame else (self.n_groups, int(nb))
            c = np.zeros(shape, dtype=np.int64)
            check(lib().mdx_prof_counts(self.handle, slot, _ptr(c)))
            out.append(c)
        return out


class GyrationEngine(_FrameEngine):
    """``mdx_gyr_*``: per frame and group the mean over the chains of ``Rg, Rg_x, Rg_y, Rg_z``."""

    _prefix = "mdx_gyr"

    def __init__(self, n_chains, n_monomers, masses, *, dev=0, timing=False):
        self.n_chains = np.ascontiguousarray(np.atleast_1d(n_chains), dtype=np.int64)
        self.n_monomers = np.ascontiguousarray(np.atleast_1d(n_monomers), dtype=np.int64)
        if self.n_chains.ndim != 1 or self.n_chains.shape != self.n_monomers.shape or len(self.n_chains) == 0:
            raise ValueError("n_chains and n_monomers must hold one entry per group.")
        self.n_groups = len(self.n_chains)
        self.n_points = int((self.n_chains * self.n_monomers).sum())
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if m.shape != (self.n_points,):
            raise ValueError("masses must hold one entry per point of the groups.")
        h = c_void_p()
        check(lib().mdx_gyr_create(byref(h), dev, self.n_groups, _ptr(self.n_chains), _ptr(self.n_monomers),
                                   _ptr(m)))
        self._adopt(h, dev, timing)

    @staticmethod
    def slab_frames(n_chains, n_monomers, *, grouped=False, unwrap=False):
        """``mdx_gyr_slab_frames``: the frames per kernel launch inside one call of an engine built from these chain
        counts, with a grouping and / or the unwrap set.  Needs no device."""
        c, m = _chain_layout(n_chains, n_monomers)
        out = c_int64()
        check(lib().mdx_gyr_slab_frames(int(c.sum()), int((c * m).sum()), int(bool(grouped)), int(bool(unwrap)),
                                        byref(out)))
        return out.value

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of monomers ``[offsets[m], offsets[m+1])`` — one per point of the
        groups — whose float64 centres of mass are the points; ``offsets=None`` removes the grouping."""
        self._set_grouping("set_grouping", offsets, masses)

    def set_unwrap(self, dims, start=None):
        """The reference's global unwrap from frame to frame, starting from the points ``start``
        (float64 ``[n_points, 3]``, every chain whole); ``dims=None`` switches it off.  Frames must then be
        fed in analysis order."""
        self._set_unwrap("set_unwrap", dims, start)

    def result(self):
        """float64 ``[G, frames seen, 4]``: ``Rg, Rg_x, Rg_y, Rg_z`` averaged over the chains of each group."""
        out = np.zeros((self.n_groups, self.stats()["frames"], 4), dtype=np.float64)
        check(lib().mdx_gyr_result(self.handle, _ptr(out)))
        return out


class ChainProjectionEngine(_FrameEngine):
    """``mdx_rouse_*``: per frame, chain and weight row ``X = sum_n w_n x_n`` in float64, kept in HBM as
    ``[frames, S, 3]`` with series ``series0[g] + k * n_chains[g] + c`` (group g, row k, chain c)."""

    _prefix = "mdx_rouse"

    def __init__(self, n_chains, n_monomers, weights, *, dev=0, timing=False):
        """weights: one float64 array ``[K, n_monomers[g]]`` per group (a single 2-D array for one group)."""
        self.n_chains = np.ascontiguousarray(np.atleast_1d(n_chains), dtype=np.int64)
        self.n_monomers = np.ascontiguousarray(np.atleast_1d(n_monomers), dtype=np.int64)
        if self.n_chains.ndim != 1 or self.n_chains.shape != self.n_monomers.shape or len(self.n_chains) == 0:
            raise ValueError("n_chains and n_monomers must hold one entry per group.")
        self.n_groups = len(self.n_chains)
        self.n_points = int((self.n_chains * self.n_monomers).sum())
        if isinstance(weights, np.ndarray) and weights.ndim == 2:
            weights = [weights]
        w = [np.ascontiguousarray(x, dtype=np.float64) for x in weights]
        if len(w) != self.n_groups or any(x.ndim != 2 for x in w):
            raise ValueError("weights must hold one array [n_rows, n_monomers] per group.")
        self.n_rows = int(w[0].shape[0])
        if self.n_rows < 1 or any(x.shape != (self.n_rows, N) for x, N in zip(w, self.n_monomers)):
            raise ValueError("weights must hold one array [n_rows, n_monomers] per group.")
        self.series0 = np.concatenate(([0], np.cumsum(self.n_rows * self.n_chains)))[:-1]
        self.n_series = int(self.n_rows * self.n_chains.sum())
        flat = np.concatenate([x.ravel() for x in w])
        h = c_void_p()
        check(lib().mdx_rouse_create(byref(h), dev, self.n_groups, _ptr(self.n_chains), _ptr(self.n_monomers),
                                     self.n_rows, _ptr(flat)))
        self._adopt(h, dev, timing)

    @staticmethod
    def slab_frames(n_chains, n_monomers, *, grouped=False, unwrap=False):
        """``mdx_rouse_slab_frames``: the frames per kernel launch inside one call of an engine built from these
        chain counts, with a grouping and / or the unwrap set.  Needs no device."""
        c, m = _chain_layout(n_chains, n_monomers)
        out = c_int64()
        check(lib().mdx_rouse_slab_frames(int((c * m).sum()), int(bool(grouped)), int(bool(unwrap)), byref(out)))
        return out.value

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of monomers ``[offsets[m], offsets[m+1])`` — one per point of the
        groups — whose float64 centres of mass are the points; ``offsets=None`` removes the grouping."""
        self._set_grouping("set_grouping", offsets, masses)

    def set_unwrap(self, dims, start=None):
        """The global unwrap of ``GyrationEngine.set_unwrap``: from frame to frame, starting from the points
        ``start`` (float64 ``[n_points, 3]``, every chain whole); ``dims=None`` switches it off."""
        self._set_unwrap("set_unwrap", dims, start)

    def reserve(self, n_frames):
        """Room for ``n_frames`` frames in all, allocated once."""
        check(lib().mdx_rouse_reserve(self.handle, int(n_frames)))

    def result(self):
        """float64 ``[frames seen, S, 3]`` on the host."""
        out = np.zeros((self.stats()["frames"], self.n_series, 3), dtype=np.float64)
        check(lib().mdx_rouse_result(self.handle, _ptr(out)))
        return out

    def device_result(self):
        """``(pointer, frames seen, S)``: the amplitudes ``double[frames][S][3]`` where they lie in HBM, after a
        wait for the engine's stream; valid until the next accumulate, reset or close."""
        p, f, s = c_void_p(), c_int64(), c_int64()
        check(lib().mdx_rouse_device_result(self.handle, byref(p), byref(f), byref(s)))
        return p, f.value, s.value


RouseEngine = ChainProjectionEngine


class InternalDistanceEngine(_FrameEngine):
    """``mdx_msid_*``: per frame and group the mean-square internal distances ``R2(s)``, ``s = 1 ... N - 1``, and the
    bond-orientation correlations ``C(s)``, ``s = 0 ... N - 2``, of chains of ``N`` points, in float64."""

    _prefix = "mdx_msid"

    def __init__(self, n_chains, n_monomers, *, dev=0, timing=False):
        self.n_chains = np.ascontiguousarray(np.atleast_1d(n_chains), dtype=np.int64)
        self.n_monomers = np.ascontiguousarray(np.atleast_1d(n_monomers), dtype=np.int64)
        if self.n_chains.ndim != 1 or self.n_chains.shape != self.n_monomers.shape or len(self.n_chains) == 0:
            raise ValueError("n_chains and n_monomers must hold one entry per group.")
        self.n_groups = len(self.n_chains)
        self.n_points = int((self.n_chains * self.n_monomers).sum())
        self.row0 = np.concatenate(([0], np.cumsum(2 * (self.n_monomers - 1))))
        h = c_void_p()
        check(lib().mdx_msid_create(byref(h), dev, self.n_groups, _ptr(self.n_chains), _ptr(self.n_monomers)))
        self._adopt(h, dev, timing)

    @staticmethod
    def slab_frames(n_chains, n_monomers, *, grouped=False, whole=False, unwrap=False):
        """``mdx_msid_slab_frames``: the frames per kernel launch inside one call of an engine built from these chain
        counts, with a grouping, ``whole`` or the unwrap set.  Needs no device."""
        c, m = _chain_layout(n_chains, n_monomers)
        out = c_int64()
        check(lib().mdx_msid_slab_frames(len(c), _ptr(c), _ptr(m), int(bool(grouped)), int(bool(whole)),
                                         int(bool(unwrap)), byref(out)))
        return out.value

    def set_grouping(self, offsets, masses):
        """Incoming rows become particles of monomers ``[offsets[m], offsets[m+1])`` — one per point of the
        groups — whose float64 centres of mass are the points; ``offsets=None`` removes the grouping."""
        self._set_grouping("set_grouping", offsets, masses)

    def set_unwrap(self, dims, start=None):
        """The global unwrap of ``GyrationEngine.set_unwrap``: from frame to frame, starting from the points
        ``start`` (float64 ``[n_points, 3]``, every chain whole); ``dims=None`` switches it off.  Excludes
        ``set_whole``."""
        self._set_unwrap("set_unwrap", dims, start)

    def set_whole(self, dims):
        """Every chain is made whole in every frame by itself, bond after bond from its first point, by the
        minimum image of each bond in the box ``dims``; ``dims=None`` switches it off.  Bonds must be shorter than
        half the shortest box length.  Frames may come in any order.  Excludes ``set_unwrap``."""
        if dims is None:
            check(lib().mdx_msid_set_whole(self.handle, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        check(lib().mdx_msid_set_whole(self.handle, _ptr(d)))

    def reserve(self, n_frames):
        """Room for ``n_frames`` frames in all, allocated once."""
        check(lib().mdx_msid_reserve(self.handle, int(n_frames)))

    def result(self):
        """One float64 array ``[frames seen, 2, N_g - 1]`` per group: ``[:, 0]`` is ``R2(1 ... N_g - 1)``,
        ``[:, 1]`` is ``C(0 ... N_g - 2)``."""
        rows = np.zeros((self.stats()["frames"], int(self.row0[-1])), dtype=np.float64)
        check(lib().mdx_msid_result(self.handle, _ptr(rows)))
        return [rows[:, lo:lo + 2 * (N - 1)].reshape(len(rows), 2, N - 1).copy()
                for lo, N in zip(self.row0[:-1], self.n_monomers)]


class DipoleEngine(_SlabbedFrameEngine):
    """``mdx_dip_*``: per frame and group the dipole moment ``sum q (r + image L)`` in float64."""

    _prefix = "mdx_dip"
    TILE = 128          # points per tile of the summation order (DIP_TILE of csrc/mdx_dipole_device.hpp)

    def __init__(self, n_points, charges, *, dev=0, timing=False):
        self.n_per_group = np.ascontiguousarray(np.atleast_1d(n_points), dtype=np.int64)
        if self.n_per_group.ndim != 1 or len(self.n_per_group) == 0:
            raise ValueError("n_points must hold one entry per group.")
        self.n_groups = len(self.n_per_group)
        self.n_points = int(self.n_per_group.sum())
        q = np.ascontiguousarray(charges, dtype=np.float64)
        if q.shape != (self.n_points,):
            raise ValueError("charges must hold one entry per point of the groups.")
        h = c_void_p()
        check(lib().mdx_dip_create(byref(h), dev, self.n_groups, _ptr(self.n_per_group), _ptr(q)))
        self._adopt(h, dev, timing)

    def set_unwrap(self, dims, start=None):
        """The reference's global unwrap from frame to frame, starting from the points ``start``
        (float64 ``[n_points, 3]``, every molecule whole); ``dims=None`` switches it off.  Frames must then be
        fed in analysis order."""
        self._set_unwrap("set_unwrap", dims, start)

    def result(self):
        """float64 ``[G, frames seen, 3]``: the dipole moment of every group in every frame."""
        out = np.zeros((self.n_groups, self.stats()["frames"], 3), dtype=np.float64)
        check(lib().mdx_dip_result(self.handle, _ptr(out)))
        return out


class VanHoveEngine(_SlabbedFrameEngine):
    """``mdx_vh_*``: per lag and group the histogram of the displacement magnitudes ``|x(f) - x(f - lag)|`` and the
    sums of their second and fourth powers, in float64.  The device is first touched by the first frame, so the
    argument errors (``ValueError``) need none."""

    _prefix = "mdx_vh"
    _stats_extra = (("evaluations", c_int64),)
    TILE = 64           # points per tile: a tile never spans two groups (VH_TILE of csrc/mdx_vanhove_device.hpp)

    def __init__(self, n_points, edges, lags, *, zero_dims=0, dev=0, timing=False):
        self.n_per_group = np.ascontiguousarray(np.atleast_1d(n_points), dtype=np.int64)
        if self.n_per_group.ndim != 1 or len(self.n_per_group) == 0:
            raise ValueError("n_points must hold one entry per group.")
        self.n_groups = len(self.n_per_group)
        self.n_points = int(self.n_per_group.sum())
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        if self.edges.ndim != 1 or len(self.edges) < 2:
            raise ValueError("edges must hold n_bins + 1 >= 2 bin edges.")
        self.n_bins = len(self.edges) - 1
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        h = c_void_p()
        check(lib().mdx_vh_create(byref(h), dev, self.n_groups, _ptr(self.n_per_group), self.n_bins,
                                  _ptr(self.edges), self.n_lags, _ptr(self.lags), int(zero_dims)))
        self._adopt(h, dev, timing)

    def set_unwrap(self, dims):
        """The reference's global unwrap from frame to frame with the box lengths ``dims``; the first frame is its
        own start.  ``dims=None`` switches it off.  Only before the first frame."""
        if dims is None:
            check(lib().mdx_vh_set_unwrap(self.handle, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        check(lib().mdx_vh_set_unwrap(self.handle, _ptr(d)))

    def result(self):
        """``(counts int64 [n_lags, G, n_bins], moments float64 [n_lags, G, 2])``: the moments are the sums of
        ``r^2`` and ``r^4`` over the group's points and every frame pair of the lag."""
        counts = np.zeros((self.n_lags, self.n_groups, self.n_bins), dtype=np.int64)
        moments = np.zeros((self.n_lags, self.n_groups, 2), dtype=np.float64)
        check(lib().mdx_vh_result(self.handle, _ptr(counts), _ptr(moments)))
        return counts, moments

    def point_moments(self):
        """float64 ``[n_lags, n_points, 2]``: every point's own sums of ``r^2`` and ``r^4``."""
        out = np.zeros((self.n_lags, self.n_points, 2), dtype=np.float64)
        check(lib().mdx_vh_point_moments(self.handle, _ptr(out)))
        return out


class FourPointEngine(_SlabbedFrameEngine):
    """``mdx_chi4_*``: per lag, group and cutoff the number ``Q`` of points with ``|x(f0 + lag) - x(f0)|^2 <= a^2``
    and, over the origins ``f0`` that are multiples of ``origin_step``, the sums of ``Q`` and of ``Q * Q``.  All
    integers: the same bits whatever the route, split, slab or segment.  The device is first touched by the first
    frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_chi4"
    _stats_extra = (("evaluations", c_int64),)
    TILE = 64           # points per load: a load never spans two groups (CHI4_TILE of csrc/mdx_chi4_device.hpp)
    MAX_CUTOFFS = 8     # cutoffs at most (CHI4_MAX_CUTOFFS)

    def __init__(self, n_points, cutoffs, lags, *, origin_step=1, zero_dims=0, dev=0, timing=False):
        self.n_per_group = np.ascontiguousarray(np.atleast_1d(n_points), dtype=np.int64)
        if self.n_per_group.ndim != 1 or len(self.n_per_group) == 0:
            raise ValueError("n_points must hold one entry per group.")
        self.n_groups = len(self.n_per_group)
        self.n_points = int(self.n_per_group.sum())
        self.cutoffs = np.ascontiguousarray(np.atleast_1d(cutoffs), dtype=np.float64)
        if self.cutoffs.ndim != 1 or not 1 <= len(self.cutoffs) <= self.MAX_CUTOFFS:
            raise ValueError(f"cutoffs must hold 1 to {self.MAX_CUTOFFS} cutoffs.")
        self.n_cutoffs = len(self.cutoffs)
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        h = c_void_p()
        check(lib().mdx_chi4_create(byref(h), dev, self.n_groups, _ptr(self.n_per_group), self.n_cutoffs,
                                    _ptr(self.cutoffs), self.n_lags, _ptr(self.lags), int(origin_step),
                                    int(zero_dims)))
        self._adopt(h, dev, timing)

    def set_unwrap(self, dims):
        """The reference's global unwrap from frame to frame with the box lengths ``dims``; the first frame is its
        own start.  ``dims=None`` switches it off.  Only before the first frame."""
        if dims is None:
            check(lib().mdx_chi4_set_unwrap(self.handle, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        check(lib().mdx_chi4_set_unwrap(self.handle, _ptr(d)))

    def set_segment_points(self, points):
        """Points one block of the counting kernel walks: a multiple of 64, 0 restores the default.  For tests and
        measurement: the results do not depend on it.  Only before the first frame."""
        check(lib().mdx_chi4_set_segment_points(self.handle, int(points)))

    def result(self):
        """``(sums, square_sums, n_origins)``: int64 ``[n_lags, G, n_cutoffs]`` twice — the sums of ``Q`` and of
        ``Q * Q`` over the origins — and int64 ``[n_lags]``, the origins of every lag."""
        sums = np.zeros((self.n_lags, self.n_groups, self.n_cutoffs), dtype=np.int64)
        square_sums = np.zeros_like(sums)
        n_origins = np.zeros(self.n_lags, dtype=np.int64)
        check(lib().mdx_chi4_result(self.handle, _ptr(sums), _ptr(square_sums), _ptr(n_origins)))
        return sums, square_sums, n_origins


class DistinctVanHoveEngine(_SlabbedFrameEngine):
    """``mdx_vhd_*``: per lag the histogram of the minimum-image distances ``|x2_j(f0 + lag) - x1_i(f0)|`` over every
    pair of points (``j != i`` with ``same``) and every frame pair whose origin ``f0`` is a multiple of
    ``origin_step``, in float64.  Incoming rows are set 1 then set 2, or set 1 alone with ``same``.  The device is
    first touched by the first frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_vhd"
    _stats_extra = (("evaluations", c_int64),)
    TILE = 256          # set-1 points per block (VHD_TILE of csrc/mdx_vanhove_distinct_device.hpp)
    JCHUNK = 512        # set-2 points per block (VHD_JCHUNK)
    LDS_BINS = 2048     # n_bins up to which the histograms live in LDS (VHD_LDS_BINS)

    def __init__(self, n1, n2, edges, lags, dims, *, same=False, origin_step=1, zero_dims=0, dev=0, timing=False):
        self.n1, self.n2, self.same = int(n1), int(n2), bool(same)
        self.n_rows = self.n1 if self.same else self.n1 + self.n2
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        if self.edges.ndim != 1 or len(self.edges) < 2:
            raise ValueError("edges must hold n_bins + 1 >= 2 bin edges.")
        self.n_bins = len(self.edges) - 1
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        h = c_void_p()
        check(lib().mdx_vhd_create(byref(h), dev, self.n1, self.n2, int(self.same), self.n_bins, _ptr(self.edges),
                                   self.n_lags, _ptr(self.lags), int(origin_step), _ptr(self.dims), int(zero_dims)))
        self._adopt(h, dev, timing)

    def result(self):
        """``counts int64 [n_lags, n_bins]``."""
        counts = np.zeros((self.n_lags, self.n_bins), dtype=np.int64)
        check(lib().mdx_vhd_result(self.handle, _ptr(counts)))
        return counts


class PairResidenceEngine(_SlabbedFrameEngine):
    """``mdx_prs_*``: per frame the pairs of points (``j != i`` with ``same``) whose minimum-image distance lies
    within ``cutoff`` (``r2 <= cutoff * cutoff`` in float64), and per lag the sizes of the intersections of an origin's
    contact set with the set a lag later (intermittent) and with every set up to there (continuous), summed over the
    origins that are multiples of ``origin_step``.  Incoming rows are set 1 then set 2, or set 1 alone with ``same``.
    A row may hold ``max_neighbors`` contacts in one frame; one that would hold more makes ``synchronize()``,
    ``result()`` and ``contacts()`` raise ``ValueError`` until ``reset()``.  The device is first touched by the first
    frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_prs"
    _stats_extra = (("evaluations", c_int64), ("max_row", c_int64))
    TILE = 256          # set-1 points per block (PRS_TILE of csrc/mdx_residence_device.hpp)
    JCHUNK = 1024       # set-2 points per block (PRS_JCHUNK)
    MAX_NEIGHBORS = 64  # slots of a row at most (PRS_MAX_NEIGHBORS)

    def __init__(self, n1, n2, cutoff, lags, dims, *, same=False, origin_step=1, zero_dims=0, max_neighbors=32,
                 continuous=True, dev=0, timing=False):
        self.n1, self.n2, self.same = int(n1), int(n2), bool(same)
        self.n_rows = self.n1 if self.same else self.n1 + self.n2
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.max_neighbors, self.continuous = int(max_neighbors), bool(continuous)
        h = c_void_p()
        check(lib().mdx_prs_create(byref(h), dev, self.n1, self.n2, int(self.same), float(cutoff), self.n_lags,
                                   _ptr(self.lags), int(origin_step), _ptr(self.dims), int(zero_dims),
                                   self.max_neighbors, int(self.continuous)))
        self._adopt(h, dev, timing)

    def result(self):
        """``{"intermittent", "continuous", "origin_counts"}``, ``int64 [n_lags]`` each."""
        out = {key: np.zeros(self.n_lags, dtype=np.int64) for key in ("intermittent", "continuous", "origin_counts")}
        check(lib().mdx_prs_result(self.handle, _ptr(out["intermittent"]), _ptr(out["continuous"]),
                                   _ptr(out["origin_counts"])))
        return out

    def contacts(self):
        """``int64 [frames]``: the contacts of every frame seen."""
        frames = c_int64()
        check(lib().mdx_prs_stats(self.handle, None, None, byref(frames), None, None))
        out = np.zeros(frames.value, dtype=np.int64)
        check(lib().mdx_prs_contacts(self.handle, _ptr(out), len(out)))
        return out


class HydrogenBondEngine(_SlabbedFrameEngine):
    """``mdx_hb_*``: per frame the hydrogen bonds among ``n_rows`` incoming rows.  ``h_row[i]`` is a hydrogen,
    ``d_row[i]`` the donor it is bonded to (it may repeat), ``a_row[j]`` an acceptor; hydrogen ``i`` and acceptor ``j``
    (not the hydrogen's own donor) are bonded where the minimum-image ``r2_DA <= distance ** 2`` and the cosine ``c``
    of the angle D-H...A at the hydrogen is at most ``cos_max``, all in float64 (csrc/mdx_hbond_device.hpp).  Per lag
    the intermittent and continuous intersections of ``PairResidenceEngine`` over the bond sets; per bond a count in
    the histograms of ``r2_DA`` and ``c`` (``set_bins``); per (frame, hydrogen) a count in ``donated``.  A hydrogen
    may hold ``max_neighbors`` bonds in one frame; one that would hold more makes ``synchronize()``, ``result()``,
    ``bonds()`` and ``geometry()`` raise ``ValueError`` until ``reset()``.  The device is first touched by the first
    frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_hb"
    _stats_extra = (("evaluations", c_int64), ("max_row", c_int64), ("degenerate", c_int64))
    TILE = 256          # hydrogens per block (HB_TILE of csrc/mdx_hbond_device.hpp)
    JCHUNK = 1024       # acceptors per block (HB_JCHUNK)
    MAX_NEIGHBORS = 64  # slots of a row at most (HB_MAX_NEIGHBORS)

    def __init__(self, n_rows, h_row, d_row, a_row, distance, cos_max, lags, dims, *, origin_step=1, zero_dims=0,
                 max_neighbors=8, continuous=True, dev=0, timing=False):
        self.n_rows = int(n_rows)
        self.h_row = np.ascontiguousarray(np.atleast_1d(h_row), dtype=np.int32)
        self.d_row = np.ascontiguousarray(np.atleast_1d(d_row), dtype=np.int32)
        self.a_row = np.ascontiguousarray(np.atleast_1d(a_row), dtype=np.int32)
        if self.h_row.ndim != 1 or self.h_row.shape != self.d_row.shape:
            raise ValueError("h_row and d_row must be one-dimensional and of one length.")
        if self.a_row.ndim != 1:
            raise ValueError("a_row must be one-dimensional.")
        self.n_h, self.n_a = len(self.h_row), len(self.a_row)
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.max_neighbors, self.continuous = int(max_neighbors), bool(continuous)
        self.n_distance_bins = self.n_cosine_bins = 1
        h = c_void_p()
        check(lib().mdx_hb_create(byref(h), dev, self.n_rows, self.n_h, _ptr(self.h_row), _ptr(self.d_row), self.n_a,
                                  _ptr(self.a_row), float(distance), float(cos_max), self.n_lags, _ptr(self.lags),
                                  int(origin_step), _ptr(self.dims), int(zero_dims), self.max_neighbors,
                                  int(self.continuous)))
        self._adopt(h, dev, timing)

    def set_bins(self, r2_thresholds, cos_thresholds):
        """``r2_thresholds``: float64 ``[n_r + 1]``, strictly increasing thresholds of ``r2_DA``; ``cos_thresholds``:
        float64 ``[n_c + 1]``, strictly decreasing thresholds of ``c``.  Only before the first frame."""
        r = np.ascontiguousarray(r2_thresholds, dtype=np.float64)
        c = np.ascontiguousarray(cos_thresholds, dtype=np.float64)
        if r.ndim != 1 or len(r) < 2 or c.ndim != 1 or len(c) < 2:
            raise ValueError("the thresholds must hold n_bins + 1 values, at least two.")
        check(lib().mdx_hb_set_bins(self.handle, len(r) - 1, _ptr(r), len(c) - 1, _ptr(c)))
        self.n_distance_bins, self.n_cosine_bins = len(r) - 1, len(c) - 1

    def result(self):
        """``{"intermittent", "continuous", "origin_counts"}``, ``int64 [n_lags]`` each."""
        out = {key: np.zeros(self.n_lags, dtype=np.int64) for key in ("intermittent", "continuous", "origin_counts")}
        check(lib().mdx_hb_result(self.handle, _ptr(out["intermittent"]), _ptr(out["continuous"]),
                                  _ptr(out["origin_counts"])))
        return out

    def bonds(self):
        """``int64 [frames]``: the bonds of every frame seen."""
        frames = c_int64()
        check(lib().mdx_hb_stats(self.handle, None, None, byref(frames), None, None, None))
        out = np.zeros(frames.value, dtype=np.int64)
        check(lib().mdx_hb_bonds(self.handle, _ptr(out), len(out)))
        return out

    def geometry(self):
        """``{"distance_counts": int64 [n_r], "cosine_counts": int64 [n_c], "donated": int64 [max_neighbors + 1]}``
        over the frames seen."""
        out = {"distance_counts": np.zeros(self.n_distance_bins, dtype=np.int64),
               "cosine_counts": np.zeros(self.n_cosine_bins, dtype=np.int64),
               "donated": np.zeros(self.max_neighbors + 1, dtype=np.int64)}
        check(lib().mdx_hb_geometry(self.handle, _ptr(out["distance_counts"]), _ptr(out["cosine_counts"]),
                                    _ptr(out["donated"])))
        return out


class SpatialDistributionEngine(_SlabbedFrameEngine):
    """``mdx_sdf_*``: per frame the partner atoms around every reference molecule, counted in the molecule's own
    frame.  ``o_row[i]``, ``a_row[i]`` and ``b_row[i]`` are the origin, the axis atom and the plane atom of molecule
    ``i`` among the ``n_rows`` incoming rows; ``p_row`` the partners, group after group (``group_start``, at most
    ``MAX_GROUPS`` groups); ``owner[j]`` the molecule partner ``j`` belongs to, or -1: that pair is never evaluated.
    ``mode`` 0 puts the axis atom on local +x, 1 the bisector of the axis and the plane atom; the plane atom lies in
    the local xy plane at y > 0.  A partner within ``cutoff`` of the origin (minimum image) is rotated into the frame
    and counted per group with ``numpy.histogramdd``'s counts over the edges of ``set_bins``, all in float64
    (csrc/mdx_sdf_device.hpp).  The device is first touched by the first frame, so the argument errors
    (``ValueError``) need none."""

    _prefix = "mdx_sdf"
    _stats_extra = (("evaluations", c_int64), ("degenerate", c_int64))
    TILE = 256          # reference molecules per block (SDF_TILE of csrc/mdx_sdf_device.hpp)
    JCHUNK = 1024       # partners per block (SDF_JCHUNK)
    MAX_GROUPS = 8      # partner groups at most (SDF_MAX_GROUPS)
    MAX_AXIS_BINS = 512
    AXIS, BISECTOR = 0, 1

    def __init__(self, n_rows, o_row, a_row, b_row, group_start, p_row, owner, mode, cutoff, dims, *, dev=0,
                 timing=False):
        self.n_rows = int(n_rows)
        self.o_row, self.a_row, self.b_row, self.p_row, self.owner = (
            np.ascontiguousarray(np.atleast_1d(t), dtype=np.int32) for t in (o_row, a_row, b_row, p_row, owner))
        if self.o_row.ndim != 1 or self.o_row.shape != self.a_row.shape or self.o_row.shape != self.b_row.shape:
            raise ValueError("o_row, a_row and b_row must be one-dimensional and of one length.")
        if self.p_row.ndim != 1 or self.p_row.shape != self.owner.shape:
            raise ValueError("p_row and owner must be one-dimensional and of one length.")
        self.group_start = np.ascontiguousarray(np.atleast_1d(group_start), dtype=np.int64)
        if self.group_start.ndim != 1 or len(self.group_start) < 2:
            raise ValueError("group_start must hold n_groups + 1 values, at least two.")
        if self.group_start[-1] != len(self.p_row):
            raise ValueError("group_start must end at the number of partners.")
        self.n_ref, self.n_p, self.n_groups = len(self.o_row), len(self.p_row), len(self.group_start) - 1
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.n_bins = (1, 1, 1)
        h = c_void_p()
        check(lib().mdx_sdf_create(byref(h), dev, self.n_rows, self.n_ref, _ptr(self.o_row), _ptr(self.a_row),
                                   _ptr(self.b_row), self.n_groups, _ptr(self.group_start), _ptr(self.p_row),
                                   _ptr(self.owner), int(mode), float(cutoff), _ptr(self.dims)))
        self._adopt(h, dev, timing)

    def set_bins(self, ex, ey, ez):
        """Strictly increasing float64 edges per axis, ``n + 1`` of them for ``n <= 512`` bins.  Only before the
        first frame."""
        e = [np.ascontiguousarray(t, dtype=np.float64) for t in (ex, ey, ez)]
        if any(t.ndim != 1 or len(t) < 2 for t in e):
            raise ValueError("the edges must hold n_bins + 1 values, at least two.")
        check(lib().mdx_sdf_set_bins(self.handle, len(e[0]) - 1, _ptr(e[0]), len(e[1]) - 1, _ptr(e[1]),
                                     len(e[2]) - 1, _ptr(e[2])))
        self.n_bins = tuple(len(t) - 1 for t in e)

    def result(self):
        """``int64 [n_groups, nx, ny, nz]``: the counts over the frames seen."""
        out = np.zeros((self.n_groups,) + self.n_bins, dtype=np.int64)
        check(lib().mdx_sdf_result(self.handle, _ptr(out)))
        return out

    def inside(self):
        """``int64 [frames]``: the counted pairs of every frame seen."""
        frames = c_int64()
        check(lib().mdx_sdf_stats(self.handle, None, None, byref(frames), None, None))
        out = np.zeros(frames.value, dtype=np.int64)
        check(lib().mdx_sdf_inside(self.handle, _ptr(out), len(out)))
        return out


class ClusterEngine(_SlabbedFrameEngine):
    """``mdx_clu_*``: per frame the connected components of the bond graph of ``n`` rows.  ``species`` (``int [n]``,
    ``0 ... G - 1``, ``G <= 8``) names the group of a row; ``cutoff`` is a float or a symmetric ``G x G`` table of
    non-negative values (0: that pair of species never bonds); rows ``i != j`` are bonded where the minimum-image
    ``r2 <= cutoff[a][b] ** 2`` in float64.  ``label[f][i]`` is the smallest row of the component of ``i``.  A row
    may hold ``max_neighbors`` bonds in one frame; one that would hold more makes ``synchronize()`` and every result
    call raise ``ValueError`` until ``reset()``.  Incoming rows are those of group 0, then group 1, ...  The device is
    first touched by the first frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_clu"
    _stats_extra = (("evaluations", c_int64), ("max_row", c_int64), ("sweeps", c_int64))
    TILE = 256          # rows per block (CLU_TILE of csrc/mdx_cluster_device.hpp)
    JCHUNK = 1024       # partners per block (CLU_JCHUNK)
    MAX_NEIGHBORS = 64  # slots of a row at most (CLU_MAX_NEIGHBORS)
    MAX_SPECIES = 8     # CLU_MAX_SPECIES

    def __init__(self, species, cutoff, dims, *, n_species=None, zero_dims=0, max_neighbors=32, keep_labels=False,
                 dev=0, timing=False):
        self.species = np.ascontiguousarray(np.atleast_1d(species), dtype=np.int32)
        if self.species.ndim != 1:
            raise ValueError("species must be one-dimensional.")
        self.n = len(self.species)
        table = np.asarray(cutoff, dtype=np.float64)
        if n_species is None:
            n_species = len(table) if table.ndim == 2 else (int(self.species.max()) + 1 if self.n else 1)
        self.n_species = int(n_species)
        if not 1 <= self.n_species <= self.MAX_SPECIES:
            raise ValueError(f"n_species must lie in [1, {self.MAX_SPECIES}].")
        if table.ndim == 0:
            table = np.full((self.n_species, self.n_species), float(table))
        if table.shape != (self.n_species, self.n_species):
            raise ValueError(f"cutoff must be a number or a {self.n_species} x {self.n_species} table.")
        self.cutoff = np.ascontiguousarray(table)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.max_neighbors, self.keep_labels = int(max_neighbors), bool(keep_labels)
        h = c_void_p()
        check(lib().mdx_clu_create(byref(h), dev, self.n, _ptr(self.species), self.n_species, _ptr(self.cutoff),
                                   _ptr(self.dims), int(zero_dims), self.max_neighbors, int(self.keep_labels)))
        self._adopt(h, dev, timing)

    def result(self):
        """``{"size_counts": int64 [n + 1], "species_counts": int64 [G, n + 1]}`` over the frames seen."""
        out = {"size_counts": np.zeros(self.n + 1, dtype=np.int64),
               "species_counts": np.zeros((self.n_species, self.n + 1), dtype=np.int64)}
        check(lib().mdx_clu_result(self.handle, _ptr(out["size_counts"]), _ptr(out["species_counts"])))
        return out

    def _frames_seen(self):
        frames = c_int64()
        check(lib().mdx_clu_stats(self.handle, None, None, byref(frames), None, None, None))
        return frames.value

    def frames(self):
        """``{"bonds", "n_clusters", "largest", "sum_squares"}``, ``int64 [frames]`` each: every frame seen."""
        n = self._frames_seen()
        out = {key: np.zeros(n, dtype=np.int64) for key in ("bonds", "n_clusters", "largest", "sum_squares")}
        check(lib().mdx_clu_frames(self.handle, _ptr(out["bonds"]), _ptr(out["n_clusters"]), _ptr(out["largest"]),
                                   _ptr(out["sum_squares"]), n))
        return out

    def labels(self):
        """``int32 [frames, n]``: the smallest row of every row's cluster (``keep_labels``)."""
        out = np.zeros((self._frames_seen(), self.n), dtype=np.int32)
        check(lib().mdx_clu_labels(self.handle, _ptr(out), len(out)))
        return out


class AngleEngine(_SlabbedFrameEngine):
    """``mdx_ang_*``: per frame the neighbours of each of ``n_centers`` centres among ``G <= 4`` ligand groups of
    ``ligand_sizes`` rows (minimum-image ``r2 <= cutoff[g] ** 2`` in float64 for a ligand of group ``g``), and for
    every unordered pair of neighbours of a centre ``c = dot / sqrt(r2_ij * r2_ik)``, counted in bin
    ``#{m in 1 ... n_bins - 1 : c <= thresholds[m]}`` of the unordered pair ``p = a*G - a*(a-1)/2 + (b-a)`` of the two
    ligands' species; a NaN ``c`` (a ligand on its centre) counts in ``degenerate[p]``.  ``thresholds`` is
    ``float64 [n_bins + 1]``, strictly decreasing.  Incoming rows are the centres, then the ligands group by group;
    with ``same`` the one ligand group is the centres themselves, the rows arrive once and ``j == i`` never counts.
    A centre may hold ``max_neighbors`` neighbours in one frame; one that would hold more makes ``synchronize()`` and
    ``result()`` raise ``ValueError`` until ``reset()``.  The device is first touched by the first frame, so the
    argument errors (``ValueError``) need none."""

    _prefix = "mdx_ang"
    _stats_extra = (("evaluations", c_int64), ("triplets", c_int64), ("max_row", c_int64))
    TILE = 256          # centres per block of the list kernel (ANG_TILE of csrc/mdx_angle_device.hpp)
    STAGE = 256         # ligands per LDS stage (ANG_STAGE)
    JCHUNK = 1024       # ligands per block (ANG_JCHUNK)
    MAX_NEIGHBORS = 64  # slots of a row at most (ANG_MAX_NEIGHBORS)
    MAX_SPECIES = 4     # ANG_MAX_SPECIES

    @staticmethod
    def pair_index(a, b, n_species):
        """The number ``p`` of the unordered pair of ligand species ``(a, b)``."""
        a, b = min(a, b), max(a, b)
        return a * n_species - a * (a - 1) // 2 + (b - a)

    def __init__(self, n_centers, ligand_sizes, cutoff, thresholds, dims, *, same=False, zero_dims=0,
                 max_neighbors=32, dev=0, timing=False):
        self.n_centers, self.same = int(n_centers), bool(same)
        self.ligand_sizes = np.ascontiguousarray(np.atleast_1d(ligand_sizes), dtype=np.int64)
        if self.ligand_sizes.ndim != 1 or not 1 <= len(self.ligand_sizes) <= self.MAX_SPECIES:
            raise ValueError(f"ligand_sizes must hold between 1 and {self.MAX_SPECIES} sizes.")
        self.n_species = len(self.ligand_sizes)
        self.n_pairs = self.n_species * (self.n_species + 1) // 2
        self.n_rows = self.n_centers if self.same else self.n_centers + int(self.ligand_sizes.sum())
        cut = np.asarray(cutoff, dtype=np.float64)
        if cut.ndim == 0:
            cut = np.full(self.n_species, float(cut))
        if cut.shape != (self.n_species,):
            raise ValueError(f"cutoff must be a number or {self.n_species} values, one per ligand group.")
        self.cutoff = np.ascontiguousarray(cut)
        self.thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
        if self.thresholds.ndim != 1 or len(self.thresholds) < 2:
            raise ValueError("thresholds must hold n_bins + 1 values, at least two.")
        self.n_bins = len(self.thresholds) - 1
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.max_neighbors = int(max_neighbors)
        h = c_void_p()
        check(lib().mdx_ang_create(byref(h), dev, self.n_centers, self.n_species, _ptr(self.ligand_sizes),
                                   int(self.same), _ptr(self.cutoff), self.n_bins, _ptr(self.thresholds),
                                   _ptr(self.dims), int(zero_dims), self.max_neighbors))
        self._adopt(h, dev, timing)

    def result(self):
        """``{"counts": int64 [P, n_bins], "degenerate": int64 [P], "coordination": int64 [G, max_neighbors + 1]}``
        over the frames seen."""
        out = {"counts": np.zeros((self.n_pairs, self.n_bins), dtype=np.int64),
               "degenerate": np.zeros(self.n_pairs, dtype=np.int64),
               "coordination": np.zeros((self.n_species, self.max_neighbors + 1), dtype=np.int64)}
        check(lib().mdx_ang_result(self.handle, _ptr(out["counts"]), _ptr(out["degenerate"]),
                                   _ptr(out["coordination"])))
        return out


class OrientationEngine(_SlabbedFrameEngine):
    """``mdx_ori_*``: per frame the unit vectors ``u`` from row ``pairs[v, 0]`` to row ``pairs[v, 1]`` of the ``n_rows``
    incoming rows (with the minimum image where ``set_box`` gave a box), per lag and vector the sums of
    ``c = u(f) . u(f - lag)`` and of ``1.5 c^2 - 0.5`` over the frames, and per frame and group the sums of the six
    products ``u_a u_b``, in float64.  Group ``g`` holds ``n_vectors[g]`` consecutive vectors.  A vector without a
    direction (head on its tail, or a length that is not finite) makes ``synchronize()``, ``result()``,
    ``vector_sums()`` and ``frame_sums()`` raise ``ValueError`` until ``reset()``.  The device is first touched by the
    first frame, so the argument errors (``ValueError``) need none."""

    _prefix = "mdx_ori"
    _stats_extra = (("evaluations", c_int64), ("degenerate", c_int64))
    TILE = 64           # vectors per tile: a tile never spans two groups (ORI_TILE of csrc/mdx_orient_device.hpp)

    def __init__(self, n_vectors, pairs, n_rows, lags, *, zero_dims=0, dev=0, timing=False):
        self.n_per_group = np.ascontiguousarray(np.atleast_1d(n_vectors), dtype=np.int64)
        if self.n_per_group.ndim != 1 or len(self.n_per_group) == 0:
            raise ValueError("n_vectors must hold one entry per group.")
        self.n_groups = len(self.n_per_group)
        self.n_vectors = int(self.n_per_group.sum())
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        if self.pairs.ndim != 2 or self.pairs.shape[1] != 2 or len(self.pairs) != max(self.n_vectors, 0):
            raise ValueError("pairs must hold one (tail, head) row per vector of the groups.")
        self.n_rows = int(n_rows)
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        h = c_void_p()
        check(lib().mdx_ori_create(byref(h), dev, self.n_groups, _ptr(self.n_per_group), self.n_rows,
                                   _ptr(self.pairs), self.n_lags, _ptr(self.lags), int(zero_dims)))
        self._adopt(h, dev, timing)

    def set_box(self, dims):
        """The box lengths ``dims`` of one constant orthorhombic box: ``head - tail`` is then the minimum image.
        ``dims=None``: no box, for molecules that are whole already.  Only before the first frame."""
        if dims is None:
            check(lib().mdx_ori_set_box(self.handle, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        check(lib().mdx_ori_set_box(self.handle, _ptr(d)))

    def result(self):
        """float64 ``[n_lags, G, 2]``: the sums of ``c`` and of ``1.5 c^2 - 0.5`` over the group's vectors and every
        frame pair of the lag."""
        sums = np.zeros((self.n_lags, self.n_groups, 2), dtype=np.float64)
        check(lib().mdx_ori_result(self.handle, _ptr(sums)))
        return sums

    def vector_sums(self):
        """float64 ``[n_lags, V, 2]``: every vector's own sums."""
        out = np.zeros((self.n_lags, self.n_vectors, 2), dtype=np.float64)
        check(lib().mdx_ori_vector_sums(self.handle, _ptr(out)))
        return out

    def frame_sums(self):
        """float64 ``[frames seen, G, 6]``: the sums of ``u_a u_b`` over the group's vectors, ``ab = xx, xy, xz, yy,
        yz, zz``, of every frame seen."""
        frames = c_int64()
        check(lib().mdx_ori_stats(self.handle, None, None, byref(frames), None, None))
        out = np.zeros((frames.value, self.n_groups, 6), dtype=np.float64)
        check(lib().mdx_ori_frame_sums(self.handle, _ptr(out), len(out)))
        return out


class DihedralEngine(_SlabbedFrameEngine):
    """``mdx_dih_*``: per frame ``cos`` and ``sin`` of the torsion angle of the rows ``quads[v] = (a, b, c, d)`` of the
    ``n_rows`` incoming rows (with the minimum image where ``set_box`` gave a box), its bin among ``n_bins`` (even)
    bins by the strictly decreasing ``thresholds`` (float64 ``[n_bins / 2 + 1]``) of the cosine and the sign of the
    sine, and its state ``state_of_bin[bin]`` (``0 ... n_states - 1``, at most ``MAX_STATES`` states); per group the
    histogram, per frame and group the state populations, per group the transitions between consecutive frames, and
    per lag the sums of ``cos(phi(f) - phi(f - lag))``, the cases in the same state again and the cases that never
    left it, in float64 and integers (csrc/mdx_dihedral_device.hpp).  Group ``g`` holds ``n_dihedrals[g]`` consecutive
    dihedrals.  A dihedral without an angle (three atoms on a line, two on one point) makes ``synchronize()`` and
    every read-out raise ``ValueError`` until ``reset()``.  The device is first touched by the first frame, so the
    argument errors (``ValueError``) need none."""

    _prefix = "mdx_dih"
    _stats_extra = (("evaluations", c_int64), ("degenerate", c_int64))
    TILE = 64           # dihedrals per tile: a tile never spans two groups (DIH_TILE of csrc/mdx_dihedral_device.hpp)
    MAX_STATES = 8      # DIH_MAX_STATES
    LDS_BINS = 1024     # bins at most for the LDS form of the histogram (DIH_LDS_BINS)

    def __init__(self, n_dihedrals, quads, n_rows, thresholds, state_of_bin, lags, *, n_states=None, dev=0,
                 timing=False):
        self.n_per_group = np.ascontiguousarray(np.atleast_1d(n_dihedrals), dtype=np.int64)
        if self.n_per_group.ndim != 1 or len(self.n_per_group) == 0:
            raise ValueError("n_dihedrals must hold one entry per group.")
        self.n_groups = len(self.n_per_group)
        self.n_dihedrals = int(self.n_per_group.sum())
        self.quads = np.ascontiguousarray(quads, dtype=np.int32)
        if self.quads.ndim != 2 or self.quads.shape[1] != 4 or len(self.quads) != max(self.n_dihedrals, 0):
            raise ValueError("quads must hold one (a, b, c, d) row per dihedral of the groups.")
        self.n_rows = int(n_rows)
        self.thresholds = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
        self.state_of_bin = np.ascontiguousarray(np.atleast_1d(state_of_bin), dtype=np.int32)
        if self.thresholds.ndim != 1 or self.state_of_bin.ndim != 1 or len(self.state_of_bin) % 2 or \
                len(self.thresholds) != len(self.state_of_bin) // 2 + 1:
            raise ValueError("state_of_bin must hold an even number n_bins of entries and thresholds "
                             "n_bins / 2 + 1.")
        self.n_bins = len(self.state_of_bin)
        self.n_states = int(self.state_of_bin.max(initial=0)) + 1 if n_states is None else int(n_states)
        self.lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.int64)
        if self.lags.ndim != 1 or len(self.lags) == 0:
            raise ValueError("lags must hold at least one lag.")
        self.n_lags = len(self.lags)
        h = c_void_p()
        check(lib().mdx_dih_create(byref(h), dev, self.n_groups, _ptr(self.n_per_group), self.n_rows,
                                   _ptr(self.quads), self.n_bins, _ptr(self.thresholds), self.n_states,
                                   _ptr(self.state_of_bin), self.n_lags, _ptr(self.lags)))
        self._adopt(h, dev, timing)

    def set_box(self, dims):
        """The box lengths ``dims`` of one constant orthorhombic box: the three bond vectors are then minimum images.
        ``dims=None``: no box, for molecules that are whole already.  Only before the first frame."""
        if dims is None:
            check(lib().mdx_dih_set_box(self.handle, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.float64)
        if d.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        check(lib().mdx_dih_set_box(self.handle, _ptr(d)))

    def result(self):
        """``{"sums": float64 [n_lags, G], "same": int64 [n_lags, G], "stay": int64 [n_lags, G]}``."""
        out = {"sums": np.zeros((self.n_lags, self.n_groups), dtype=np.float64),
               "same": np.zeros((self.n_lags, self.n_groups), dtype=np.int64),
               "stay": np.zeros((self.n_lags, self.n_groups), dtype=np.int64)}
        check(lib().mdx_dih_result(self.handle, _ptr(out["sums"]), _ptr(out["same"]), _ptr(out["stay"])))
        return out

    def dihedral_sums(self):
        """float64 ``[n_lags, D]``: every dihedral's own sums."""
        out = np.zeros((self.n_lags, self.n_dihedrals), dtype=np.float64)
        check(lib().mdx_dih_dihedral_sums(self.handle, _ptr(out)))
        return out

    def counts(self):
        """int64 ``[G, n_bins]``: the histogram of every group over the frames seen."""
        out = np.zeros((self.n_groups, self.n_bins), dtype=np.int64)
        check(lib().mdx_dih_counts(self.handle, _ptr(out)))
        return out

    def state_counts(self):
        """int64 ``[frames seen, G, n_states]``: the dihedrals of a group in every state, frame by frame."""
        frames = c_int64()
        check(lib().mdx_dih_stats(self.handle, None, None, byref(frames), None, None))
        out = np.zeros((frames.value, self.n_groups, self.n_states), dtype=np.int64)
        check(lib().mdx_dih_state_counts(self.handle, _ptr(out), len(out)))
        return out

    def transitions(self):
        """int64 ``[G, n_states, n_states]``: the (dihedral, frame ``f >= 1``) cases by state at ``f - 1`` and ``f``."""
        out = np.zeros((self.n_groups, self.n_states, self.n_states), dtype=np.int64)
        check(lib().mdx_dih_transitions(self.handle, _ptr(out)))
        return out


class BondOrderEngine(_SlabbedFrameEngine):
    """``mdx_boo_*``: per frame the neighbours of each of ``n_centers`` centres among ``n_neighbors`` candidates
    (minimum-image ``r2 <= cutoff ** 2`` in float64), and per centre ``i`` with ``m_i >= 1`` neighbours and degree
    ``l`` of ``degrees`` (``1 ... 12``, at most 4 distinct ones) ``q_lm = sum_j Y_lm(w_ij / r_ij) / m_i`` over the
    neighbours in ascending ``j`` and ``q_l = sqrt(4 pi / (2l + 1) * sum_m |q_lm|^2)``; with ``averaged`` also
    ``qbar_l`` from ``qbar_lm = (q_lm(i) + sum_j q_lm(j)) / (m_i + 1)``.  Recurrences, host tables and summation
    orders: csrc/mdx_bond_order_device.hpp.  ``K = 2`` with ``averaged``, else 1.  A value ``q`` is counted in bin
    ``#{m in 1 ... n_bins - 1 : q >= edges[m]}`` iff ``edges[0] <= q <= edges[n_bins]`` (``numpy.histogram``), else in
    ``outside``; a centre without a neighbour has NaN values and is counted nowhere.  Incoming rows are the centres,
    then the candidates; with ``same`` the candidates are the centres themselves, the rows arrive once and ``j == i``
    never counts; ``averaged`` needs ``same``.  A centre may hold ``max_neighbors`` neighbours in one frame; one that
    would hold more, or a neighbour on top of its centre (a bond without a direction), makes ``synchronize()``,
    ``result()``, ``frames()`` and ``values()`` raise ``ValueError`` until ``reset()``.  Every result is the same bits
    whatever the route, the split into calls or the slab.  The device is first touched by the first frame, so the
    argument errors (``ValueError``) need none."""

    _prefix = "mdx_boo"
    _stats_extra = (("evaluations", c_int64), ("bonds", c_int64), ("degenerate", c_int64), ("max_row", c_int64))
    TILE = 256          # centres per block of the list kernel (BOO_TILE of csrc/mdx_bond_order_device.hpp)
    JCHUNK = 1024       # candidates per block (BOO_JCHUNK)
    MAX_NEIGHBORS = 64  # slots of a row at most (BOO_MAX_NEIGHBORS)
    MAX_DEGREE = 12     # the largest l (BOO_MAX_DEGREE)
    MAX_DEGREES = 4     # degrees per engine at most (BOO_MAX_DEGREES)
    SUM_TILE = 64       # centres per tile of the frame sums (BOO_SUM_TILE)
    LDS_BINS = 1024     # n_bins at most for the histogram in LDS (BOO_LDS_BINS)

    def __init__(self, n_centers, n_neighbors, cutoff, degrees, edges, dims, *, same=False, averaged=False,
                 max_neighbors=32, keep_values=False, dev=0, timing=False):
        self.n_centers, self.same, self.averaged = int(n_centers), bool(same), bool(averaged)
        self.n_neighbors = self.n_centers if n_neighbors is None else int(n_neighbors)
        self.n_rows = self.n_centers if self.same else self.n_centers + self.n_neighbors
        self.degrees = np.ascontiguousarray(np.atleast_1d(degrees), dtype=np.int32)
        if self.degrees.ndim != 1 or not 1 <= len(self.degrees) <= self.MAX_DEGREES:
            raise ValueError(f"degrees must hold between 1 and {self.MAX_DEGREES} degrees.")
        self.n_degrees, self.n_kinds = len(self.degrees), 2 if self.averaged else 1
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        if self.edges.ndim != 1 or len(self.edges) < 2:
            raise ValueError("edges must hold n_bins + 1 values, at least two.")
        self.n_bins = len(self.edges) - 1
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.cutoff, self.max_neighbors, self.keep_values = float(cutoff), int(max_neighbors), bool(keep_values)
        h = c_void_p()
        check(lib().mdx_boo_create(byref(h), dev, self.n_centers, self.n_neighbors, int(self.same), self.cutoff,
                                   self.n_degrees, _ptr(self.degrees), int(self.averaged), self.n_bins,
                                   _ptr(self.edges), _ptr(self.dims), self.max_neighbors, int(self.keep_values)))
        self._adopt(h, dev, timing)

    def _frames_seen(self):
        frames = c_int64()
        check(lib().mdx_boo_stats(self.handle, None, None, byref(frames), None, None, None, None))
        return frames.value

    def result(self):
        """``{"counts": int64 [D, K, n_bins], "outside": int64 [D, K], "coordination": int64 [max_neighbors + 1]}``
        over the frames seen."""
        out = {"counts": np.zeros((self.n_degrees, self.n_kinds, self.n_bins), dtype=np.int64),
               "outside": np.zeros((self.n_degrees, self.n_kinds), dtype=np.int64),
               "coordination": np.zeros(self.max_neighbors + 1, dtype=np.int64)}
        check(lib().mdx_boo_result(self.handle, _ptr(out["counts"]), _ptr(out["outside"]), _ptr(out["coordination"])))
        return out

    def frames(self):
        """``{"sums": float64 [frames, D, K], "counted": int64 [frames]}`` of every frame seen: the sum of the values
        of the centres that have a neighbour, and how many those are."""
        n = self._frames_seen()
        out = {"sums": np.zeros((n, self.n_degrees, self.n_kinds), dtype=np.float64),
               "counted": np.zeros(n, dtype=np.int64)}
        check(lib().mdx_boo_frames(self.handle, _ptr(out["sums"]), _ptr(out["counted"]), n))
        return out

    def values(self):
        """float64 ``[frames, D, K, n_centers]``: every centre's values, NaN for an isolated one (``keep_values``)."""
        out = np.zeros((self._frames_seen(), self.n_degrees, self.n_kinds, self.n_centers), dtype=np.float64)
        check(lib().mdx_boo_values(self.handle, _ptr(out), len(out)))
        return out


class TetrahedralEngine(_SlabbedFrameEngine):
    """``mdx_tet_*``: per frame the ``n_nearest`` (4 ... 8) nearest of the ``n_neighbors`` candidates in range
    (minimum-image ``r2 <= cutoff ** 2`` in float64) of each of ``n_centers`` centres, ordered by ascending ``r2`` and,
    where two are bit-equal, ascending candidate number; from the first four the orientational tetrahedral order ``q``
    and its translational counterpart ``S_k`` (every operation: csrc/mdx_tetrahedral_device.hpp), a histogram of each
    against its own ``edges`` (``numpy.histogram``'s rule), and per neighbour rank a histogram of ``r2`` against
    ``distance_thresholds``.  A centre with fewer than four candidates in range is short: NaN values, counted in no
    value histogram and no sum, but in the distance histograms of the ranks it has.  Incoming rows are the centres,
    then the candidates; with ``same`` the candidates are the centres themselves, the rows arrive once and ``j == i``
    never counts.  One of a centre's four nearest on top of it (no direction) makes ``synchronize()``, ``result()``,
    ``frames()`` and ``values()`` raise ``ValueError`` until ``reset()``.  Every result is the same bits whatever the
    route, the split into calls, the slab or the candidate chunk.  The device is first touched by the first frame, so
    the argument errors (``ValueError``) need none."""

    _prefix = "mdx_tet"
    _stats_extra = (("evaluations", c_int64), ("degenerate", c_int64), ("chunks", c_int64))
    TILE = 256          # centres per block of the selection kernel (TET_TILE of csrc/mdx_tetrahedral_device.hpp)
    STAGE = 256         # candidates per LDS stage: a chunk is a multiple of it (TET_STAGE)
    MIN_NEAREST = 4     # what q and S_k need (TET_MIN_NEAREST)
    MAX_NEAREST = 8     # the largest n_nearest (TET_MAX_NEAREST)
    SUM_TILE = 64       # centres per tile of the frame sums (TET_SUM_TILE)
    LDS_BINS = 1024     # bins at most for a histogram in LDS (TET_LDS_BINS)

    def __init__(self, n_centers, n_neighbors, cutoff, q_edges, s_edges, distance_thresholds, dims, *, n_nearest=4,
                 same=False, keep_values=False, dev=0, timing=False):
        self.n_centers, self.same, self.n_nearest = int(n_centers), bool(same), int(n_nearest)
        self.n_neighbors = self.n_centers if n_neighbors is None else int(n_neighbors)
        self.n_rows = self.n_centers if self.same else self.n_centers + self.n_neighbors
        if not self.MIN_NEAREST <= self.n_nearest <= self.MAX_NEAREST:
            raise ValueError(f"n_nearest must lie in [{self.MIN_NEAREST}, {self.MAX_NEAREST}].")
        tables = []
        for name, table in (("q_edges", q_edges), ("s_edges", s_edges), ("distance_thresholds", distance_thresholds)):
            table = np.ascontiguousarray(table, dtype=np.float64)
            if table.ndim != 1 or len(table) < 2:
                raise ValueError(f"{name} must hold n_bins + 1 values, at least two.")
            tables.append(table)
        self.q_edges, self.s_edges, self.distance_thresholds = tables
        self.q_bins, self.s_bins, self.distance_bins = (len(table) - 1 for table in tables)
        self.dims = np.ascontiguousarray(dims, dtype=np.float64)
        if self.dims.shape != (3,):
            raise ValueError("dims must hold the three box lengths.")
        self.cutoff, self.keep_values = float(cutoff), bool(keep_values)
        h = c_void_p()
        check(lib().mdx_tet_create(byref(h), dev, self.n_centers, self.n_neighbors, int(self.same), self.n_nearest,
                                   self.cutoff, self.q_bins, _ptr(self.q_edges), self.s_bins, _ptr(self.s_edges),
                                   self.distance_bins, _ptr(self.distance_thresholds), _ptr(self.dims),
                                   int(self.keep_values)))
        self._adopt(h, dev, timing)

    @staticmethod
    def chunk_for(n_centers, n_neighbors, frames, compute_units):
        """``mdx_tet_chunk_for``: the candidates per block the plan chooses for a launch of ``frames`` frames on a
        device of ``compute_units`` compute units.  Needs no device."""
        chunk = c_int64()
        check(lib().mdx_tet_chunk_for(int(n_centers), int(n_neighbors), int(frames), int(compute_units), byref(chunk)))
        return chunk.value

    def set_chunk(self, candidates):
        """Candidates per block of the selection kernel, a multiple of ``STAGE``; 0 restores the plan's choice.  Only
        before the first frame.  The results do not depend on it."""
        check(lib().mdx_tet_set_chunk(self.handle, int(candidates)))

    def plan(self):
        """``mdx_tet_plan``: ``slab_frames`` and ``ring_frames`` as every engine's, and ``chunk``, the candidates per
        block of a launch of ``slab_frames`` frames.  Where no chunk is set the choice reads the compute units of the
        engine's device (and nothing else of it)."""
        slab, ring, chunk = c_int64(), c_int64(), c_int64()
        check(lib().mdx_tet_plan(self.handle, byref(slab), byref(ring), byref(chunk)))
        return {"slab_frames": slab.value, "ring_frames": ring.value, "chunk": chunk.value}

    def _frames_seen(self):
        frames = c_int64()
        check(lib().mdx_tet_stats(self.handle, None, None, byref(frames), None, None, None))
        return frames.value

    def result(self):
        """``{"q_counts": int64 [q_bins], "s_counts": int64 [s_bins], "outside": int64 [2] (q, S_k),
        "distance_counts": int64 [n_nearest, distance_bins], "distance_outside": int64 [n_nearest],
        "found": int64 [n_nearest + 1]}`` over the frames seen."""
        k = self.n_nearest
        out = {"q_counts": np.zeros(self.q_bins, dtype=np.int64), "s_counts": np.zeros(self.s_bins, dtype=np.int64),
               "outside": np.zeros(2, dtype=np.int64),
               "distance_counts": np.zeros((k, self.distance_bins), dtype=np.int64),
               "distance_outside": np.zeros(k, dtype=np.int64), "found": np.zeros(k + 1, dtype=np.int64)}
        check(lib().mdx_tet_result(self.handle, *(_ptr(out[key]) for key in (
            "q_counts", "s_counts", "outside", "distance_counts", "distance_outside", "found"))))
        return out

    def frames(self):
        """``{"sums": float64 [frames, 2], "counted": int64 [frames]}`` of every frame seen: the sums of ``q`` and
        ``S_k`` over the centres that are not short, and how many those are."""
        n = self._frames_seen()
        out = {"sums": np.zeros((n, 2), dtype=np.float64), "counted": np.zeros(n, dtype=np.int64)}
        check(lib().mdx_tet_frames(self.handle, _ptr(out["sums"]), _ptr(out["counted"]), n))
        return out

    def values(self):
        """``{"values": float64 [frames, 2, n_centers], "neighbors": int32 [frames, n_nearest, n_centers]}``: every
        centre's ``q`` and ``S_k`` (NaN for a short one) and its neighbours in the contract's order, ``-1`` beyond
        those it has (``keep_values``)."""
        n = self._frames_seen()
        out = {"values": np.zeros((n, 2, self.n_centers), dtype=np.float64),
               "neighbors": np.zeros((n, self.n_nearest, self.n_centers), dtype=np.int32)}
        check(lib().mdx_tet_values(self.handle, _ptr(out["values"]), _ptr(out["neighbors"]), n))
        return out


def fourier_sum_device(wavevectors, positions, dev=0):
    """``mdx_fourier_sum``: complex128[N_q] = sum_j exp(i q.r_j), float64 positions."""
    q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(q.shape[0], dtype=np.complex128)
    check(lib().mdx_fourier_sum(dev, _ptr(q), q.shape[0], _ptr(r), r.shape[0], _ptr(out)))
    return out


def inner_device(wavevectors, positions, dev=0):
    """``mdx_inner``: float64[N_q, N] of q_i . r_j."""
    q = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((q.shape[0], r.shape[0]), dtype=np.float64)
    if out.size:
        for lo in range(0, q.shape[0], 65535):           # (one launch covers 65 535 wavevectors)
            hi = min(q.shape[0], lo + 65535)
            check(lib().mdx_inner(dev, _ptr(q[lo:hi]), hi - lo, _ptr(r), r.shape[0], _ptr(out[lo:hi])))
    return out


def trig_rowsums_device(xs, *, cos=True, sin=True, dev=0):
    """``mdx_trig_rowsums``: ``(sum_j cos(xs[i, j]), sum_j sin(xs[i, j]))`` of a float64 matrix (``None`` for a
    sum that was not asked for)."""
    x = np.ascontiguousarray(xs, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("xs must be a two-dimensional array.")
    c = np.zeros(x.shape[0]) if cos else None
    s = np.zeros(x.shape[0]) if sin else None
    if x.shape[0]:
        check(lib().mdx_trig_rowsums(dev, _ptr(x), x.shape[0], x.shape[1], _ptr(c), _ptr(s)))
    return c, s


class MsdEngine(_Engine):
    """``mdx_msd_*``: per-group sums of per-particle MSDs through rocFFT."""

    _destroy = "mdx_msd_destroy"

    def __init__(self, n_frames_block, n_blocks, n_groups, *, dev=0, timing=False):
        h = c_void_p()
        check(lib().mdx_msd_create(byref(h), dev, int(n_frames_block), int(n_blocks), int(n_groups)))
        self.handle = h
        self.dev = dev
        self.t_block, self.n_blocks, self.n_groups = int(n_frames_block), int(n_blocks), int(n_groups)
        self.has_grouping = False
        if timing:
            check(lib().mdx_msd_enable_timing(h, 1))

    @property
    def n_fft(self):
        n = c_int64()
        check(lib().mdx_msd_n_fft(self.handle, byref(n)))
        return n.value

    @property
    def transform(self):
        """``(own, r1, r2)``: the engine's own two-pass transform ``n_fft = r1 * r2`` (``own`` True), or the rocFFT
        pipeline (``(False, 0, 0)``)."""
        own, r1, r2 = c_int(), c_int(), c_int()
        check(lib().mdx_msd_transform(self.handle, byref(own), byref(r1), byref(r2)))
        return bool(own.value), r1.value, r2.value

    PLAN_FIELDS = ("n_fft", "own", "r1", "r2", "single", "fused_sums", "reads_f32", "pass_a", "pass_b", "head", "n_elem",
                   "p_pad", "super_groups", "split", "rows_parts", "pg_major")
    PASS_A = ("rocfft", "single400", "cols400_fused", "cols_small_fused", "cols")
    PASS_B = ("none", "tiny", "short", "mid", "rows512", "rows1024", "general")

    @staticmethod
    def plan(n_frames_block, n_blocks, n_total, first, count, elem_bytes=8, base_aligned=True):
        """``mdx_msd_plan``: the kernels an engine ``MsdEngine(n_frames_block, n_blocks, ...)`` launches for ONE
        ``push_device`` (``elem_bytes=8``) or ``push_device_f32`` (``4``) of particles ``[first, first + count)`` of
        an array of ``n_total`` particles per frame, as a dict of ``PLAN_FIELDS`` — ``pass_a`` indexes ``PASS_A``,
        ``pass_b`` indexes ``PASS_B``; the push is described as one chunk.  ``push`` stages its selection first:
        ``plan(T_b, B, count, 0, count)``.  Needs no device; reads ``MDX_MSD_ROCFFT`` / ``MDX_MSD_TWO_PASS`` as the
        constructor does."""
        out = np.zeros(16, dtype=np.int64)
        check(lib().mdx_msd_plan(int(n_frames_block), int(n_blocks), int(n_total), int(first), int(count),
                                 int(elem_bytes), 1 if base_aligned else 0, _ptr(out)))
        return dict(zip(MsdEngine.PLAN_FIELDS, (int(v) for v in out)))

    def push(self, group, positions, first, count, zero_dims=0):
        """positions: float64[T, N_total, 3] on the host."""
        p = np.ascontiguousarray(positions, dtype=np.float64)
        if p.shape[0] < self.t_block * self.n_blocks:
            raise ValueError("positions hold fewer frames than n_blocks * n_frames_block.")
        check(lib().mdx_msd_push(self.handle, group, _ptr(p), p.shape[1], first, count, zero_dims))

    def push_device(self, group, d_pos, n_total, first, count, zero_dims=0):
        check(lib().mdx_msd_push_device(self.handle, group, d_pos, n_total, first, count, zero_dims))

    @property
    def reads_f32(self):
        """Whether the first pass of this engine reads float32 positions where they lie (``push_device_f32``): the
        transforms with a 400- or 64-point first factor (the single-pass kernel, the 400 x R2 family, 2^13 .. 2^16:
        every block length up to 204 800 frames)."""
        own, r1, _r2 = self.transform
        return bool(own) and r1 in (400, 64)

    def push_device_f32(self, group, d_pos, n_total, first, count, zero_dims=0):
        """``mdx_msd_push_device_f32``: a plain particle range of float32 frames resident in HBM, widened by pass A as
        it stages them (``NotImplementedError`` from engines whose transforms do not: see :attr:`reads_f32`)."""
        check(lib().mdx_msd_push_device_f32(self.handle, group, d_pos, n_total, first, count, zero_dims))

    def set_grouping(self, offsets, masses):
        """Rows of the following ``push_traj`` calls are particles of molecules
        ``[offsets[g], offsets[g+1])``; the engine receives their float64 centres of mass.
        ``offsets=None`` removes the grouping (``mdx_msd_set_grouping``)."""
        self.has_grouping = offsets is not None
        if offsets is None:
            check(lib().mdx_msd_set_grouping(self.handle, 0, None, None))
            return
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if len(m) != o[-1]:
            raise ValueError("masses must hold one entry per particle of the grouping.")
        check(lib().mdx_msd_set_grouping(self.handle, len(o) - 1, _ptr(o), _ptr(m)))

    def set_initial_images(self, images):
        """int[n_sel, 3] image flags the rows of the following unwrapped pushes / system-COM calls
        start from (molecules made whole in the first analysed frame); ``None`` clears."""
        if images is None:
            check(lib().mdx_msd_set_initial_images(self.handle, None, 0))
            return
        im = np.ascontiguousarray(images, dtype=np.int32).reshape(-1, 3)
        check(lib().mdx_msd_set_initial_images(self.handle, _ptr(im), im.shape[0]))

    def push_f32(self, group, positions, *, unwrap_dims=None, zero_dims=0, shift=None):
        """A group's float32 (or float64) positions ``[T, n_sel, 3]`` from host memory through the
        device-side frame preparation (unwrap, molecule centres, shift): ``mdx_msd_push_f32`` /
        ``mdx_msd_push_f64``."""
        f64 = np.asarray(positions).dtype == np.float64
        p = np.ascontiguousarray(positions, dtype=np.float64 if f64 else np.float32)
        d = None if unwrap_dims is None else np.ascontiguousarray(unwrap_dims, dtype=np.float64)[:3]
        sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        fn = lib().mdx_msd_push_f64 if f64 else lib().mdx_msd_push_f32
        check(fn(self.handle, group, _ptr(p), p.shape[0], p.shape[1], 0 if d is None else 1, _ptr(d),
                 zero_dims, _ptr(sh)))

    def system_com_f32(self, positions, masses, *, unwrap_dims=None, wrap_dims=None):
        """float64[T, 3] system centre of mass per frame of float32 / float64 positions
        ``[T, n_sel, 3]``; with a grouping set: of the molecules' (wrapped) centres."""
        f64 = np.asarray(positions).dtype == np.float64
        p = np.ascontiguousarray(positions, dtype=np.float64 if f64 else np.float32)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        dims = unwrap_dims if unwrap_dims is not None else wrap_dims
        d = None if dims is None else np.ascontiguousarray(dims, dtype=np.float64)[:3]
        out = np.empty((p.shape[0], 3), dtype=np.float64)
        fn = lib().mdx_msd_system_com_f64 if f64 else lib().mdx_msd_system_com_f32
        check(fn(self.handle, _ptr(p), p.shape[0], p.shape[1], _ptr(m), 0 if unwrap_dims is None else 1,
                 _ptr(d), 0 if wrap_dims is None else 1, _ptr(out)))
        return out

    def push_frames_device(self, group, d_pos, n_total, index=None, *, unwrap_dims=None, zero_dims=0,
                           shift=None):
        """A group's positions out of frames resident in HBM (``DeviceArray`` float32 / float64
        ``[T, n_total, 3]``): rows ``index`` (None: all) gathered by the frame-preparation kernels
        (``mdx_msd_push_frames_device``)."""
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        d = None if unwrap_dims is None else np.ascontiguousarray(unwrap_dims, dtype=np.float64)[:3]
        sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        check(lib().mdx_msd_push_frames_device(
            self.handle, group, d_pos.ptr, d_pos.dtype.itemsize, d_pos.shape[0], int(n_total), _ptr(i),
            0 if i is None else len(i), 0 if d is None else 1, _ptr(d), zero_dims, _ptr(sh)))

    def system_com_device(self, d_pos, n_total, index, masses, *, unwrap_dims=None, wrap_dims=None):
        """float64[T, 3] system centre of mass per frame of HBM-resident frames."""
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        dims = unwrap_dims if unwrap_dims is not None else wrap_dims
        d = None if dims is None else np.ascontiguousarray(dims, dtype=np.float64)[:3]
        out = np.empty((d_pos.shape[0], 3), dtype=np.float64)
        check(lib().mdx_msd_system_com_device(
            self.handle, d_pos.ptr, d_pos.dtype.itemsize, d_pos.shape[0], int(n_total), _ptr(i), len(m),
            _ptr(m), 0 if unwrap_dims is None else 1, _ptr(d), 0 if wrap_dims is None else 1, _ptr(out)))
        return out

    def system_com_traj(self, traj_file, frames, index, masses, *, unwrap_dims=None, wrap_dims=None):
        """float64[len(frames), 3] system centre of mass per frame (``Onsager(center=True)``)."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        m = np.ascontiguousarray(masses, dtype=np.float64)
        dims = unwrap_dims if unwrap_dims is not None else wrap_dims
        d = None if dims is None else np.ascontiguousarray(dims, dtype=np.float64)[:3]
        out = np.empty((len(f), 3), dtype=np.float64)
        check(lib().mdx_msd_system_com_traj(self.handle, traj_file.handle, _ptr(f), len(f), _ptr(i),
                                            len(m), _ptr(m), 0 if unwrap_dims is None else 1, _ptr(d),
                                            0 if wrap_dims is None else 1, _ptr(out)))
        return out

    def push_traj(self, group, traj_file, frames, index=None, *, unwrap_dims=None, zero_dims=0,
                  shift=None):
        """A group's positions straight from a native trajectory file; ``unwrap_dims``: box
        lengths for the device-side global unwrap (None: positions are used as stored)."""
        f = np.ascontiguousarray(frames, dtype=np.int64)
        i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        d = None if unwrap_dims is None else np.ascontiguousarray(unwrap_dims, dtype=np.float64)[:3]
        sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
        check(lib().mdx_msd_push_traj(self.handle, group, traj_file.handle, _ptr(f), len(f), _ptr(i),
                                      0 if i is None else len(i), 0 if d is None else 1, _ptr(d),
                                      zero_dims, _ptr(sh)))

    def result(self, want_msd=True):
        msd = np.zeros((self.n_groups, self.n_blocks, self.t_block)) if want_msd else None
        traj = np.zeros((self.n_groups, self.n_blocks, self.t_block, 3))
        check(lib().mdx_msd_result(self.handle, _ptr(msd), _ptr(traj)))
        return msd, traj

    def cross(self, pairs):
        """float64[n_pairs, n_blocks, t_block]: ``msd_fft(sum_i r, sum_j r)`` for every pair of groups, from the
        summed trajectories in HBM (``mdx_msd_cross``)."""
        p = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.empty((len(p), self.n_blocks, self.t_block))
        check(lib().mdx_msd_cross(self.handle, _ptr(p), len(p), _ptr(out)))
        return out

    def result_acf(self):
        """float64[n_groups, n_blocks, t_block]: sum over the pushed entities and dimensions of
        ``sum_k x(k) x(k+m)`` (the un-normalised vector ACF; ``mdx_msd_result_acf``)."""
        acf = np.zeros((self.n_groups, self.n_blocks, self.t_block))
        check(lib().mdx_msd_result_acf(self.handle, _ptr(acf)))
        return acf

    def reset(self):
        check(lib().mdx_msd_reset(self.handle))

    def synchronize(self):
        """Wait for everything queued on the engine's stream."""
        check(lib().mdx_msd_stats(self.handle, None, None, None))

    def allreduce(self, comm: RcclComm):
        check(lib().mdx_msd_allreduce(self.handle, comm.handle))

    def stats(self):
        n, ms, nb = c_int64(), c_double(), c_int64()
        check(lib().mdx_msd_stats(self.handle, byref(n), byref(ms), byref(nb)))
        return {"launches": n.value, "kernel_ms": ms.value, "bytes_moved": nb.value}


def correlate_device(a, b=None, *, negative=False, dev=0):
    """
    ``mdx_correlate``: un-normalised linear correlations of real series.

    a, b : float64[n_series, n_t].  Returns ``pos[n_series, n_t]`` with
    ``pos[s, m] = sum_k a[s, k] b[s, k+m]`` and, when ``negative``, also
    ``neg[s, m] = sum_k a[s, k+m] b[s, k]``.
    """
    a = np.ascontiguousarray(a, dtype=np.float64)
    n_series, n_t = a.shape
    bb = None
    if b is not None:
        bb = np.ascontiguousarray(b, dtype=np.float64)
        if bb.shape != a.shape:
            raise ValueError("The arrays must have the same dimensions.")
    out = np.zeros_like(a)
    neg = np.zeros_like(a) if negative else None
    check(lib().mdx_correlate(dev, _ptr(a), _ptr(bb), n_series, n_t, _ptr(out), _ptr(neg)))
    return (out, neg) if negative else out
