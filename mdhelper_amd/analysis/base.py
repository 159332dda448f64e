"""
Analysis base classes (operator surface of ``mdhelper.analysis.base``).

Mirrors reference ``src/mdhelper/analysis/base.py``: ``Hash`` (:72-113),
``SerialAnalysisBase`` (:115-210), ``NumbaAnalysisBase`` (:212-279),
``ParallelAnalysisBase`` (:281-507) and ``DynamicAnalysisBase`` (:509-584) keep
their names, ``run()`` signatures and ``save()``; underneath sits a small
restatement of ``MDAnalysis.analysis.base.AnalysisBase`` (frame selection,
``_prepare`` / ``_single_frame`` / ``_conclude`` protocol, ``results``), because
MDAnalysis is not a dependency here.

What changes is where the frames go: the classes built on these bases hand
*batches* of frames to a HIP engine instead of doing per-frame NumPy work, so
the process-pool / joblib / dask / numba-thread machinery of the reference has
nothing left to parallelise.  The keyword arguments that steered it
(``n_jobs``, ``module``, ``block``, ``method``, ``n_threads``) are accepted and
ignored.  Scaling past one GPU is by frame (or particle) sharding across ranks,
one process per GPU, with one all-reduce at the end (``comm=``).
"""

from __future__ import annotations

import logging
from datetime import datetime
from typing import Any, TextIO, Union

import numpy as np

from ..algorithm.unit import strip_unit
from ..comm import SerialComm, shard_range


class Hash(dict):
    """``dict`` with attribute access (reference base.py:72-113)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for arg in args:
            if not isinstance(arg, dict):
                raise TypeError("Positional arguments must be dictionaries.")
            for k, v in arg.items():
                self[k] = v
        for k, v in kwargs.items():
            self[k] = v

    def __getattr__(self, attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return self.get(attr)

    def __setattr__(self, key, value):
        self[key] = value

    def __delattr__(self, item):
        del self[item]

    def __contains__(self, key):
        return dict.__contains__(self, key)


class AnalysisBase:
    """
    Frame-iteration protocol of ``MDAnalysis.analysis.base.AnalysisBase``:
    ``run()`` = ``_setup_frames`` → ``_prepare`` → per frame (``_frame_index``,
    ``_ts``, ``frames[i]``, ``times[i]``, ``_single_frame``) → ``_conclude``.
    """

    def __init__(self, trajectory, verbose: bool = False, **kwargs):
        self._trajectory = trajectory
        self._verbose = verbose
        self.results = Hash()
        self._comm = kwargs.pop("comm", None) or SerialComm()
        self._device = int(kwargs.pop("device", 0))

    def _setup_frames(self, trajectory, start=None, stop=None, step=None, frames=None):
        if frames is not None:
            if not all(x is None for x in (start, stop, step)):
                raise ValueError("start/stop/step cannot be combined with frames")
            slicer = frames
        else:
            start, stop, step = trajectory.check_slice_indices(start, stop, step)
            slicer = slice(start, stop, step)
        self._sliced_trajectory = trajectory[slicer]
        self.start, self.stop, self.step = start, stop, step
        self.n_frames = len(self._sliced_trajectory)
        self.frames = np.zeros(self.n_frames, dtype=int)
        self.times = np.zeros(self.n_frames)

    def _frame_numbers(self) -> np.ndarray:
        """Trajectory frame numbers selected by ``_setup_frames``."""
        st = self._sliced_trajectory
        if hasattr(st, "frames"):
            return np.asarray(st.frames, dtype=int)
        return np.arange(self.start, self.stop, self.step)

    def _batched_frames(self, start, stop, step, frames, *, shard: bool) -> np.ndarray:
        """
        Prologue of a ``run()`` that hands whole blocks of frames to an engine: ``_setup_frames`` →
        ``_prepare`` → ``frames`` / ``times`` of every selected frame.  Returns the frame numbers this
        rank analyses: its contiguous share when frames shard across ranks (``shard``), else all of them.
        """
        traj = self._trajectory
        self._setup_frames(traj, start=start, stop=stop, step=step, frames=frames)
        self._prepare()
        numbers = self._frame_numbers()
        self.frames[:] = numbers
        self.times[:] = numbers * traj.dt
        if not shard:
            return numbers
        lo, hi = shard_range(len(numbers), self._comm.rank, self._comm.world_size)
        return numbers[lo:hi]

    def _frame_stride(self) -> int:
        """Trajectory frames between two analysed frames, for the analyses whose lags are counted in analysed
        frames: these must be evenly spaced and go forward in time."""
        st = self._sliced_trajectory
        if hasattr(st, "frames"):
            df = np.diff(st.frames)
            if len(df) and (df[0] <= 0 or not np.allclose(df, df[0])):
                raise ValueError("The selected frames must be evenly spaced and proceed forward in time.")
            return df[0] if len(df) else 1
        step = getattr(st, "step", None)
        if step is not None and step <= 0:
            raise ValueError("The analysis must proceed forward in time.")
        return step if step is not None else 1

    def _prepare(self):
        pass

    def _single_frame(self):
        raise NotImplementedError

    def _conclude(self):
        pass

    def run(self, start=None, stop=None, step=None, frames=None, verbose=None, **kwargs):
        verbose = getattr(self, "_verbose", False) if verbose is None else verbose
        self._setup_frames(self._trajectory, start=start, stop=stop, step=step, frames=frames)
        self._prepare()
        t0 = datetime.now()
        for i, ts in enumerate(self._sliced_trajectory):
            self._frame_index = i
            self._ts = ts
            self.frames[i] = ts.frame
            self.times[i] = ts.time
            self._single_frame()
        self._conclude()
        if verbose:
            logging.getLogger("mdhelper_amd").info("Analysis finished in %s.", datetime.now() - t0)
        return self


class SerialAnalysisBase(AnalysisBase):
    """Reference base.py:115-210 (``run`` :137-172, ``save`` :174-210)."""

    def __init__(self, trajectory, verbose: bool = False, **kwargs):
        super().__init__(trajectory, verbose, **kwargs)

    def run(self, start: int = None, stop: int = None, step: int = None,
            frames: Union[slice, np.ndarray] = None, n_jobs: int = 1, verbose: bool = None,
            **kwargs) -> "SerialAnalysisBase":
        return AnalysisBase.run(self, start, stop, step, frames, verbose, **kwargs)

    def save(self, file: Union[str, TextIO], archive: bool = True, compress: bool = True,
             **kwargs) -> None:
        data = {k: v for k, v in self.results.items() if k != "units"}
        if archive and compress:
            np.savez_compressed(file, **data, **kwargs)
        elif archive:
            np.savez(file, **data, **kwargs)
        else:
            for name, value in data.items():
                np.save(f"{file}_{name}", value, **kwargs)


class NumbaAnalysisBase(SerialAnalysisBase):
    """Reference base.py:212-279; ``n_threads`` has no meaning on the GPU and is ignored."""

    def run(self, start: int = None, stop: int = None, step: int = None,
            frames: Union[slice, np.ndarray] = None, n_threads: int = None,
            verbose: bool = None, **kwargs) -> "NumbaAnalysisBase":
        return AnalysisBase.run(self, start=start, stop=stop, step=step, frames=frames,
                                verbose=verbose, **kwargs)


class ParallelAnalysisBase(SerialAnalysisBase):
    """
    Reference base.py:281-507.  The reference fans frames out to worker
    processes (:396-501) and sums their per-frame results; here one process
    drives one GPU and the fan-out is the device's.  ``n_jobs``, ``module``,
    ``block`` and ``method`` are accepted for drop-in compatibility and ignored.
    """

    def _single_frame_parallel(self, frame: int, index: int) -> Any:
        raise NotImplementedError

    def run(self, start: int = None, stop: int = None, step: int = None,
            frames: Union[slice, np.ndarray] = None, verbose: bool = None, n_jobs: int = None,
            module: str = "multiprocessing", block: bool = True, method: str = None,
            **kwargs) -> "ParallelAnalysisBase":
        if method is not None and method not in {"fork", "forkserver", "spawn"}:
            raise ValueError("Invalid multiprocessing start method.")
        return AnalysisBase.run(self, start, stop, step, frames, verbose, **kwargs)


class DynamicAnalysisBase(ParallelAnalysisBase, SerialAnalysisBase):
    """Reference base.py:509-584: serial / parallel switch by the ``parallel`` flag."""

    def __init__(self, trajectory, parallel: bool, verbose: bool = False, **kwargs) -> None:
        self._parallel = parallel
        SerialAnalysisBase.__init__(self, trajectory, verbose=verbose, **kwargs)

    def run(self, start: int = None, stop: int = None, step: int = None,
            frames: Union[slice, np.ndarray] = None, verbose: bool = None,
            **kwargs) -> Union[SerialAnalysisBase, ParallelAnalysisBase]:
        return (ParallelAnalysisBase if self._parallel else SerialAnalysisBase).run(
            self, start=start, stop=stop, step=step, frames=frames, verbose=verbose, **kwargs)


class FrameBatcher:
    """
    Collects per-frame float32 position blocks (one per group) into contiguous
    batches and hands full batches to ``flush([positions[F, N_g, 3], ...], boxes[F, 6] | None)``.
    """

    def __init__(self, n_atoms, flush, with_box: bool = True, max_bytes: int = 256 << 20):
        sizes = [int(n) for n in np.atleast_1d(n_atoms)]
        self.capacity = int(max(1, min(4096, max_bytes // max(12 * sum(sizes), 1))))
        self._pos = [np.empty((self.capacity, n, 3), dtype=np.float32) for n in sizes]
        self._box = np.empty((self.capacity, 6), dtype=np.float32) if with_box else None
        self._n = 0
        self._flush = flush

    def add(self, positions, box=None):
        for buf, p in zip(self._pos, positions):
            buf[self._n] = p
        if self._box is not None:
            self._box[self._n] = box
        self._n += 1
        if self._n == self.capacity:
            self.flush()

    def flush(self):
        if self._n:
            self._flush([b[:self._n] for b in self._pos],
                        None if self._box is None else self._box[:self._n])
            self._n = 0


# The batched frame feed of the classes' run(): trajectories with block access hand whole blocks of frames to an
# engine, read from a trajectory file, from float32 frames already in HBM or from host memory.  ``accumulate_blocks``
# is the one block loop; ``EngineFedAnalysis`` is the ``run()`` around it of every class that feeds one engine the
# same rows of every frame.  RadialDistributionFunction (boxes and two groups per call), EndToEndVector (host gathers)
# and Onsager (whole trajectories per group) use the helpers from runs of their own.

FILE_BLOCK = 4096       # frames per trajectory-file call, at least (the library pipelines inside a call)


def has_frame_blocks(traj) -> bool:
    """Whether ``traj`` hands out blocks of frames (``ArrayTrajectory``, ``DeviceTrajectory``,
    ``io.FileTrajectory``); other readers go through the per-frame ``AnalysisBase.run``."""
    return hasattr(traj, "frame_block") and hasattr(traj, "box_block")


def block_frames(n_atoms: int, least: int, nbytes: int) -> int:
    """Frames per engine call: as many as ``nbytes`` of float32 positions of ``n_atoms`` hold, at least ``least``."""
    return max(least, nbytes // max(12 * n_atoms, 1))


def all_particles(index, n_atoms) -> bool:
    """Whether ``index`` is every particle in order: the engines then read the frames without a gather."""
    return len(index) == n_atoms and np.array_equal(index, np.arange(len(index)))


def block_source(traj, frames, hbm: bool):
    """
    Where the engine reads the block ``frames`` from: ``("file", TrajectoryFile)`` (frames stream file -> pinned
    memory -> HBM inside the library); ``("hbm", rows)`` when ``hbm`` allows it and the frames are consecutive
    float32 frames already in HBM (``ArrayUniverse.from_device``: the kernels read them where they lie); else
    ``("host", positions[len(frames), n_atoms, 3])`` for the caller to gather from.
    """
    native = getattr(traj, "native", None)
    if native is not None:
        return "file", native
    if hbm and getattr(traj, "device_block", None) is not None and traj.device_array.dtype == np.float32:
        rows = traj.device_block(frames)
        if rows is not None:
            return "hbm", rows
    return "host", traj.frame_block(frames)


def source_blocks(traj, frames, size: int, hbm: bool):
    """``frames`` in consecutive blocks of ``size``: ``(frames of the block, *block_source(...))`` of each."""
    for b0 in range(0, len(frames), size):
        sel = frames[b0:b0 + size]
        yield (sel, *block_source(traj, sel, hbm))


def accumulate_blocks(engine, traj, frames, index, capacity: int, *, hbm: bool = True,
                      device_index: bool = True) -> None:
    """
    ``frames`` into ``engine``, particles ``index`` of every frame in that order, block by block: ``FILE_BLOCK``
    frames per ``accumulate_traj`` from a file, else ~1 GiB (at least ``capacity`` frames) per ``accumulate_device``
    or ``accumulate``.  ``hbm``: frames in HBM may be read where they lie (the engine has no grouping set that
    forbids it).  ``device_index``: the engine's ``accumulate_device`` takes the index; one that does not (``SqEngine``,
    ``IsfEngine``) reads HBM only for every particle in order.
    """
    whole = all_particles(index, traj.n_atoms)
    rows = None if whole else index
    hbm = hbm and (device_index or whole)
    size = (FILE_BLOCK if getattr(traj, "native", None) is not None
            else block_frames(traj.n_atoms, capacity, 1 << 30))
    for sel, route, src in source_blocks(traj, frames, size, hbm):
        if route == "file":
            engine.accumulate_traj(src, sel, rows)
        elif route == "hbm":
            engine.accumulate_device(src.ptr, traj.n_atoms, len(sel), *((rows,) if device_index else ()))
        else:
            engine.accumulate(src if whole else src[:, index])


class EngineFedAnalysis:
    """
    ``run()`` of the classes that hand the same rows of every analysed frame to one engine; mixed in ahead of an
    analysis base.  ``_prepare`` ends with ``_feed_engine(engine, index)``; from there on this class owns the frames
    of this rank, the per-frame route (``_single_frame`` into a ``FrameBatcher``) and the batched one
    (``accumulate_blocks``).  ``_conclude`` starts with ``self._batch.flush()`` and closes the engine.
    """

    _shard_frames = False       # whether the frames shard across ranks (else every rank is handed all of them)
    _device_index = True        # whether the engine's accumulate_device takes an index (accumulate_blocks)

    def _feed_engine(self, engine, index=None, *, rows: int = None, max_bytes: int = 256 << 20) -> None:
        """``engine`` (``None``: this run has nothing to accumulate) gets the particles ``index`` of every frame, in
        that order; ``_before_blocks`` may still set ``_index``.  ``rows``: rows of a frame on the per-frame route
        where they are not ``len(index)``."""
        self._engine, self._index, self._hbm = engine, index, True
        self._frames_mine = (shard_range(self.n_frames, self._comm.rank, self._comm.world_size)
                             if self._shard_frames else (0, self.n_frames))
        self._batch = FrameBatcher(len(index) if rows is None else rows,
                                   lambda p, b: self._engine.accumulate(p[0]) if self._engine else None,
                                   with_box=False, max_bytes=max_bytes)

    def _frame_rows(self):
        """The rows of the current frame on the per-frame route."""
        return np.asarray(self._ts.positions, dtype=np.float32)[self._index]

    def _single_frame(self) -> None:
        lo, hi = self._frames_mine
        if lo <= self._frame_index < hi:
            self._batch.add([self._frame_rows()])

    def _before_blocks(self) -> None:
        """Runs on the batched route only, between ``_prepare`` and the first block, where there is an engine."""

    def run(self, start=None, stop=None, step=None, frames=None, verbose=None, **kwargs):
        traj = self._trajectory
        if not has_frame_blocks(traj):
            return super().run(start=start, stop=stop, step=step, frames=frames, verbose=verbose, **kwargs)
        mine = self._batched_frames(start, stop, step, frames, shard=self._shard_frames)
        if self._engine is not None:
            try:
                self._before_blocks()
                accumulate_blocks(self._engine, traj, mine, self._index, self._batch.capacity, hbm=self._hbm,
                                  device_index=self._device_index)
            except BaseException:
                self._engine.close()        # its stream and HBM go now, not when the collector finds the handle
                raise
        self._conclude()
        return self

    def _gather_frame_rows(self, rows: np.ndarray, axis: int = 0) -> np.ndarray:
        """Per-frame results of this rank's frames (along ``axis``) to those of all frames on every rank: this
        rank's rows inside the full, zero-filled array, summed across the ranks."""
        if self._comm.world_size == 1:
            return rows
        lo, hi = self._frames_mine
        full = np.zeros(rows.shape[:axis] + (self.n_frames,) + rows.shape[axis + 1:], dtype=rows.dtype)
        full[(slice(None),) * axis + (slice(lo, hi),)] = rows
        return np.asarray(self._comm.allreduce(full, op="sum"))

    def _box_lengths(self, dimensions, reach: float, what: str) -> np.ndarray:
        """Box lengths (Å) for minimum-image distances up to ``reach``, the value of the argument ``what``: the
        given ``dimensions`` or else the universe's box, which must be orthorhombic.  After ``_drop_axis`` is set."""
        if dimensions is not None:
            if len(dimensions) != 3:
                raise ValueError("'dimensions' must have length 3.")
            lengths = np.asarray(strip_unit(dimensions, "angstrom")[0], dtype=float)
        elif self.universe.dimensions is not None:
            box = np.asarray(self.universe.dimensions, dtype=float)
            if len(box) > 3 and not np.all(box[3:6] == 90.0):
                raise ValueError(f"{type(self).__name__} needs an orthorhombic box.")
            lengths = box[:3].copy()
        else:
            raise ValueError("The minimum image needs the box lengths: no system dimensions found or provided.")
        if not (np.all(np.isfinite(lengths)) and np.all(lengths > 0)):
            raise ValueError("The box lengths must be positive and finite.")
        if reach > lengths[kept_components(self._drop_axis)].min() / 2:
            raise ValueError(f"'{what}' reaches beyond half the shortest box length, where the minimum image is not "
                             "the nearest image.")
        return lengths


# Argument checks that several classes make.

def parse_lags(lags, n_lags):
    """``lags`` / ``n_lags`` of the lag-time analyses: int64 lags in analysed frames, strictly increasing and
    non-negative, or ``None`` (every analysed frame is a lag)."""
    if lags is not None and n_lags is not None:
        raise ValueError("'lags' and 'n_lags' cannot both be given.")
    if n_lags is not None:
        if int(n_lags) < 1:
            raise ValueError("'n_lags' must be at least 1.")
        lags = np.arange(int(n_lags))
    if lags is None:
        return None
    lags = np.atleast_1d(np.asarray(lags))
    if lags.ndim != 1 or len(lags) == 0 or not np.issubdtype(lags.dtype, np.integer):
        raise ValueError("'lags' must be a one-dimensional array of integers.")
    if lags[0] < 0 or np.any(np.diff(lags) <= 0):
        raise ValueError("'lags' must be non-negative and strictly increasing.")
    return lags.astype(np.int64)


def parse_drop_axis(drop_axis, message: str = "Invalid value passed to 'drop_axis'. The valid values are 0 or 'x', "
                                               "1 or 'y', and 2 or 'z'."):
    """``drop_axis`` (0, 1, 2, "x", "y", "z" or ``None``) as 0, 1, 2 or ``None``."""
    axis = ord(drop_axis) - 120 if isinstance(drop_axis, str) else drop_axis
    if axis not in {0, 1, 2, None}:
        raise ValueError(message)
    return axis


def zero_dims(drop_axis) -> int:
    """The engines' bit mask of the components that take no part."""
    return 0 if drop_axis is None else 1 << drop_axis


def kept_components(drop_axis) -> list:
    """The components that take part."""
    return [c for c in (0, 1, 2) if c != drop_axis]


def pair_selection(ag1, ag2):
    """``(same, N_1, N_2, index)`` of the two sets of a pair analysis: ``ag2`` is ``None`` or the very atoms of
    ``ag1`` in the same order (``same``: one set, ``index`` its atoms) or disjoint from it (``index``: set 1, then
    set 2)."""
    i1 = np.asarray(ag1.indices)
    i2 = i1 if ag2 is None else np.asarray(ag2.indices)
    same = ag2 is None or np.array_equal(i1, i2)
    if not same and len(np.intersect1d(i1, i2)):
        raise ValueError("'ag1' and 'ag2' share some atoms: they must be disjoint, or the very same atoms in "
                         "the same order.")
    if len(i1) < 1 or len(i2) < 1:
        raise ValueError("The groups must hold at least one atom.")
    return same, len(i1), len(i2), i1 if same else np.concatenate((i1, i2))


def shell_volumes(edges, n_dims: int) -> np.ndarray:
    """Volume of the spherical shell of every bin (``n_dims == 3``), or area of its ring (2)."""
    if n_dims == 3:
        return 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    return np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)


def grouping_of(rows):
    """``(offsets, masses)`` for an engine's ``set_grouping`` from the ``(indices, offsets or None, masses or
    None)`` of every group (``molecule_rows``), concatenated; plain-atom groups enter as molecules of one particle
    (of unit mass where they carry none).  ``None`` where no group has molecules."""
    if all(off is None for _, off, _ in rows):
        return None
    sizes = [np.ones(len(i), dtype=np.int64) if off is None else np.diff(off) for i, off, _ in rows]
    masses = [np.ones(len(i)) if m is None else m for i, _, m in rows]
    return np.concatenate(([0], np.cumsum(np.concatenate(sizes)))), np.concatenate(masses)
