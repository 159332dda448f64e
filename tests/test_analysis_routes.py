"""
The routing contract of the analysis classes' ``run()``: which engine calls each class makes for each kind of
trajectory (a trajectory file, float32 frames already in HBM, host memory with a gather, the per-frame fallback),
grouping, frame list and world size.  The engines, device arrays and device queries are replaced by recorders, so
this runs without a GPU.  Every call is written down with its arguments (frame lists and block boundaries, index
arrays, grouping offsets and masses, device pointers) and compared with the trace in ``EXPECTED``.

Positions say where they come from: particle ``a`` of frame ``f`` sits at ``(f, a, 0.25)`` and the box of frame ``f``
is ``L + f / 8`` long in x, so a block of positions or boxes handed to an engine prints as the frames and particles
it holds.
"""

import hashlib
import warnings

import numpy as np
import pytest

import mdhelper_amd
from mdhelper_amd import _core, _lib
from mdhelper_amd.analysis import (Clusters, DensityProfile, DipoleMoment, DistinctVanHove, EndToEndVector, Gyradius,
                                   IntermediateScatteringFunction, Onsager, PairResidence,
                                   RadialDistributionFunction, RouseModes, SingleChainStructureFactor, StructureFactor,
                                   VanHove)

F, N, L = 10, 120, 50.0
BIG_N = 1 << 20          # particles of the zero-stride trajectories whose frames split into several blocks

_trace = []
_tokens = [0]
_failing = set()         # names of the recorders whose accumulate raises


# ----------------------------------------------------------------------------------------------- formatting

def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:10]


def _ints(a):
    a = np.asarray(a, dtype=np.int64).ravel()
    if len(a) == 0:
        return "-"
    if len(a) > 1 and np.all(a == a[0]):
        return f"{a[0]}x{len(a)}"
    runs = np.split(a, np.flatnonzero(np.diff(a) != 1) + 1)
    if len(runs) <= 6:
        return ",".join(str(r[0]) if len(r) == 1 else f"{r[0]}..{r[-1]}" for r in runs)
    d = np.diff(a)
    if np.all(d == d[0]):
        return f"{a[0]}..{a[-1]}/{d[0]}"
    return f"<{len(a)} ints #{_digest(a)}>"


def _floats(a):
    a = np.asarray(a, dtype=np.float64)
    if a.size <= 8:
        return "[" + " ".join(f"{x:.6g}" for x in a.ravel()) + "]"
    return f"<{a.shape} #{_digest(np.round(a, 4))}>"


def _positions(a):
    tag = "pos32" if a.dtype == np.float32 else "pos64"
    if a.shape[0] > 1 and a.strides[0] == 0:
        return f"{tag}<zero-stride {a.shape}>"
    if a.shape[0] and a.shape[1]:
        f, atoms = a[:, 0, 0], a[0, :, 1]
        if (np.array_equal(a[..., 0], np.broadcast_to(f[:, None], a.shape[:2]))
                and np.array_equal(a[..., 1], np.broadcast_to(atoms[None], a.shape[:2]))
                and np.all(a[..., 2] == 0.25)):
            return f"{tag}[{_ints(f)} | {_ints(atoms)}]"
    return f"{tag}<{a.shape} #{_digest(np.round(np.asarray(a, dtype=np.float64), 4))}>"


def _fmt(v):
    if v is None or isinstance(v, (bool, str)):
        return repr(v)
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        return f"{float(v):.6g}"
    if isinstance(v, mdhelper_amd.io.TrajectoryFile):
        return "file"
    if isinstance(v, np.dtype):
        return v.name
    if hasattr(v, "ptr") and not isinstance(v, np.ndarray):
        return str(v.ptr)
    if isinstance(v, (tuple, list)) and not all(isinstance(x, (int, float, np.number)) for x in v):
        return "(" + ", ".join(_fmt(x) for x in v) + ")"
    a = np.asarray(v)
    if a.ndim == 3 and a.shape[-1] == 3 and a.dtype.kind == "f":
        return _positions(a)
    if a.ndim == 2 and a.shape[-1] == 6 and a.dtype == np.float32:
        return f"box[{_ints(np.round((a[:, 0] - L) * 8))}]"
    if a.dtype.kind in "iu":
        return _ints(a)
    return _floats(a)


def _record(name, args=(), kwargs=None):
    parts = [_fmt(a) for a in args] + [f"{k}={_fmt(v)}" for k, v in sorted((kwargs or {}).items())]
    _trace.append(f"{name}({', '.join(parts)})")


# ------------------------------------------------------------------------------------------------ recorders

class _Recorder:
    name = None

    def __init__(self, *args, **kwargs):
        _record(self.name, args, kwargs)
        self._args = args

    def __getattr__(self, method):
        if method.startswith("_"):
            raise AttributeError(method)

        def call(*args, **kwargs):
            _record(f"{self.name}.{method}", args, kwargs)
        return call


class RdfRecorder(_Recorder):
    name = "Rdf"

    def counts(self):
        _record("Rdf.counts")
        return np.zeros(len(self._args[0]) - 1, dtype=np.int64)


class SqRecorder(_Recorder):
    name = "Sq"

    def result(self):
        _record("Sq.result")
        return np.zeros((len(self._args[2]), len(self._args[0])))


class IsfRecorder(_Recorder):
    name = "Isf"

    def result(self):
        _record("Isf.result")
        q, sizes, pairs, n_lags, incoherent = self._args[:5]
        slots = 1 if pairs[0][0] is None else len(sizes)
        return (np.zeros((n_lags, len(pairs), len(q))),
                np.zeros((n_lags, slots, len(q))) if incoherent else None)


class MsdRecorder(_Recorder):
    name = "Msd"
    reads_f32 = True

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.has_grouping = False
        self._shape = (int(args[2]), int(args[1]), int(args[0]))     # groups, blocks, block length

    def set_grouping(self, offsets, masses):
        _record("Msd.set_grouping", (offsets, masses))
        self.has_grouping = offsets is not None

    def system_com_device(self, *args, **kwargs):
        _record("Msd.system_com_device", args, kwargs)
        return np.zeros((args[0].shape[0], 3))

    def system_com_traj(self, *args, **kwargs):
        _record("Msd.system_com_traj", args, kwargs)
        return np.zeros((len(args[1]), 3))

    def system_com_f32(self, *args, **kwargs):
        _record("Msd.system_com_f32", args, kwargs)
        return np.zeros((np.shape(args[0])[0], 3))

    def result(self, want_msd=True):
        _record("Msd.result")
        return np.zeros(self._shape), np.zeros(self._shape + (3,))

    def result_acf(self):
        _record("Msd.result_acf")
        return np.zeros(self._shape)

    def cross(self, pairs):
        _record("Msd.cross", (pairs,))
        return np.zeros((len(pairs),) + self._shape[1:])


class _FrameRecorder(_Recorder):
    """The per-frame engines hold one row per frame seen: the three routes count the frames they are handed.  A
    recorder named in ``_failing`` raises in ``accumulate``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._kwargs = kwargs
        self._seen = 0

    def accumulate(self, *args, **kwargs):
        _record(f"{self.name}.accumulate", args, kwargs)
        if self.name in _failing:
            raise RuntimeError(f"{self.name}.accumulate fails")
        self._seen += np.shape(args[0])[0]

    def accumulate_device(self, *args, **kwargs):
        _record(f"{self.name}.accumulate_device", args, kwargs)
        self._seen += int(args[2])

    def accumulate_traj(self, *args, **kwargs):
        _record(f"{self.name}.accumulate_traj", args, kwargs)
        self._seen += len(args[1])


class VanHoveRecorder(_FrameRecorder):
    name = "VanHove"

    def result(self):
        _record("VanHove.result")
        sizes, edges, lags = self._args[:3]
        return (np.zeros((len(lags), len(sizes), len(edges) - 1), dtype=np.int64),
                np.zeros((len(lags), len(sizes), 2)))


class DistinctVanHoveRecorder(_FrameRecorder):
    name = "DistinctVanHove"

    def result(self):
        _record("DistinctVanHove.result")
        return np.zeros((len(self._args[3]), len(self._args[2]) - 1), dtype=np.int64)


class ResidenceRecorder(_FrameRecorder):
    name = "Residence"
    MAX_NEIGHBORS = 64

    def result(self):
        _record("Residence.result")
        return {key: np.zeros(len(self._args[3]), dtype=np.int64)
                for key in ("intermittent", "continuous", "origin_counts")}

    def contacts(self):
        _record("Residence.contacts")
        return np.zeros(self._seen, dtype=np.int64)


class ClusterRecorder(_FrameRecorder):
    name = "Cluster"
    MAX_NEIGHBORS = 64
    MAX_SPECIES = 8

    def result(self):
        _record("Cluster.result")
        n = len(self._args[0])
        return {"size_counts": np.zeros(n + 1, dtype=np.int64),
                "species_counts": np.zeros((self._kwargs["n_species"], n + 1), dtype=np.int64)}

    def frames(self):
        _record("Cluster.frames")
        return {key: np.zeros(self._seen, dtype=np.int64)
                for key in ("bonds", "n_clusters", "largest", "sum_squares")}

    def labels(self):
        _record("Cluster.labels")
        return np.zeros((self._seen, len(self._args[0])), dtype=np.int32)


class DipoleRecorder(_FrameRecorder):
    name = "Dipole"

    def result(self):
        _record("Dipole.result")
        return np.zeros((len(self._args[0]), self._seen, 3))


class ProfileRecorder(_FrameRecorder):
    name = "Profile"

    def counts(self):
        _record("Profile.counts")
        sizes, axes, n_bins = self._args[:3]
        frames = (self._seen,) if self._kwargs.get("per_frame") else ()
        return [np.zeros((len(sizes),) + frames + (int(nb),), dtype=np.int64)
                for nb in np.broadcast_to(n_bins, np.shape(axes))]


class GyrationRecorder(_FrameRecorder):
    name = "Gyration"

    def result(self):
        _record("Gyration.result")
        return np.zeros((len(self._args[0]), self._seen, 4))


class ProjectionRecorder(_FrameRecorder):
    name = "Projection"

    def _series(self):
        return int(len(self._args[2][0]) * np.sum(self._args[0]))

    def result(self):
        _record("Projection.result")
        return np.zeros((self._seen, self._series(), 3))

    def device_result(self):
        _record("Projection.device_result")
        return "amplitudes", self._seen, self._series()


class DeviceArrayRecorder:
    """``_core.DeviceArray``: allocations are named d0, d1, ... in the order they are made."""

    base = None

    def __init__(self, shape, dtype, dev=0, *, _name="DeviceArray", _host=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.ptr = f"d{_tokens[0]}"
        _tokens[0] += 1
        _record(f"{_name}->{self.ptr}", (self.shape, self.dtype) if _host is None else (_host,))

    @classmethod
    def from_host(cls, arr, dev=0):
        return cls(np.shape(arr), np.asarray(arr).dtype, dev, _name="DeviceArray.from_host", _host=arr)

    @classmethod
    def upload(cls, arr, dev=0):
        return cls(np.shape(arr), np.asarray(arr).dtype, dev, _name="DeviceArray.upload", _host=arr)

    @staticmethod
    def view(base, shape):
        v = object.__new__(DeviceArrayRecorder)
        v.shape, v.dtype, v.ptr, v.base = tuple(shape), base.dtype, base.ptr, base
        return v

    def upload_columns(self, host, first, count):
        _record(f"{self.ptr}.upload_columns", (host, first, count))

    def free(self):
        _record(f"{self.ptr}.free")


class _Rows:
    def __init__(self, base, first, count):
        self.base, self.dtype = base, base.dtype
        self.shape = (count,) + base.shape[1:]
        self.ptr = f"rows{first}+{count}"

    def free(self):
        _record(f"{self.ptr}.free")


class DuckDeviceFrames:
    """Frames "in HBM" for ``ArrayUniverse.from_device``: ``shape``, ``dtype``, ``rows()``, ``to_host()``."""

    def __init__(self, host):
        self._host = host
        self.shape, self.dtype = host.shape, host.dtype

    def rows(self, first, count):
        _record("rows", (first, count))
        return _Rows(self, first, count)

    def to_host(self, first=0, count=None):
        count = self.shape[0] - first if count is None else count
        _record("to_host", (first, count))
        return self._host[first:first + count].copy()


class _Comm:
    device_collectives = False

    def __init__(self, rank, world_size):
        self.rank, self.world_size = rank, world_size

    def allreduce(self, arr, op="sum"):
        return arr


def _correlate(a, b=None, *, negative=False, dev=0):
    """``_core.correlate_device`` (the cross terms of ranks that do not share the summed trajectories in HBM)."""
    _record("correlate_device", (np.shape(a), b is None, negative))
    out = np.zeros(np.shape(a))
    return (out, out.copy()) if negative else out


def install_recorders(monkeypatch):
    monkeypatch.setattr(_core, "RdfEngine", RdfRecorder)
    monkeypatch.setattr(_core, "SqEngine", SqRecorder)
    monkeypatch.setattr(_core, "IsfEngine", IsfRecorder)
    monkeypatch.setattr(_core, "MsdEngine", MsdRecorder)
    monkeypatch.setattr(_core, "VanHoveEngine", VanHoveRecorder)
    monkeypatch.setattr(_core, "DistinctVanHoveEngine", DistinctVanHoveRecorder)
    monkeypatch.setattr(_core, "PairResidenceEngine", ResidenceRecorder)
    monkeypatch.setattr(_core, "ClusterEngine", ClusterRecorder)
    monkeypatch.setattr(_core, "DipoleEngine", DipoleRecorder)
    monkeypatch.setattr(_core, "ProfileEngine", ProfileRecorder)
    monkeypatch.setattr(_core, "GyrationEngine", GyrationRecorder)
    monkeypatch.setattr(_core, "ChainProjectionEngine", ProjectionRecorder)
    monkeypatch.setattr(_lib, "require_device", lambda dev=0: None)
    monkeypatch.setattr(_core, "DeviceArray", DeviceArrayRecorder)
    monkeypatch.setattr(_core, "device_info", lambda dev=0: _record("device_info") or {"hbm_available_bytes": 1 << 40})
    monkeypatch.setattr(_core, "synchronize", lambda dev=0: _record("synchronize"))
    monkeypatch.setattr(_core, "correlate_device", _correlate)
    monkeypatch.setattr(mdhelper_amd.io.TrajectoryFile, "load_device",
                        lambda self, frames, d_out, dev=0, **kw: _record("file.load_device", (frames, d_out)))
    _trace.clear()
    _tokens[0] = 0
    _failing.clear()


@pytest.fixture(autouse=True)
def recorders(monkeypatch):
    install_recorders(monkeypatch)
    yield
    _trace.clear()
    _failing.clear()


# ---------------------------------------------------------------------------------------------- trajectories

TOPOLOGY = dict(masses=1.0 + np.arange(N) % 7, resids=np.arange(N) // 3, segids=np.arange(N) // 12)


def _frames(dtype=np.float32):
    pos = np.empty((F, N, 3), dtype=dtype)
    pos[..., 0] = np.arange(F)[:, None]
    pos[..., 1] = np.arange(N)[None]
    pos[..., 2] = 0.25
    return pos


def _boxes():
    box = np.tile(np.array([L, L, L, 90, 90, 90], dtype=np.float32), (F, 1))
    box[:, 0] += np.arange(F) / 8
    return box


def _universe(kind, tmp_path):
    if kind == "memory":
        return mdhelper_amd.ArrayUniverse(_frames(), _boxes(), dt=0.5, **TOPOLOGY)
    if kind == "bonds":          # two bonds longer than half the box: the first frame has fragments to make whole
        return mdhelper_amd.ArrayUniverse(_frames(), _boxes(), dt=0.5, bonds=[(0, 119), (5, 70)], **TOPOLOGY)
    if kind in ("hbm32", "hbm64"):
        frames = DuckDeviceFrames(_frames(np.float32 if kind == "hbm32" else np.float64))
        return mdhelper_amd.ArrayUniverse.from_device(frames, _boxes(), dt=0.5, **TOPOLOGY)
    if kind == "file":
        from trajfiles import write_amber_netcdf
        path = tmp_path / "routes.nc"
        write_amber_netcdf(path, _frames(), _boxes()[:, :3], times=0.5 * np.arange(F))
        return mdhelper_amd.FileUniverse(path, dt=0.5, **TOPOLOGY)
    # "big": zero-stride frames of BIG_N particles, set after construction: several blocks per run, no memory
    u = mdhelper_amd.ArrayUniverse(np.zeros((1, BIG_N, 3), dtype=np.float32), [L, L, L, 90, 90, 90], dt=0.5)
    u.trajectory._positions = np.broadcast_to(u.trajectory._positions, (BIG_FRAMES[kind[4:]], BIG_N, 3))
    return u


BIG_FRAMES = {"rdf": 400, "sq": 100, "isf": 100, "scsf": 100, "e2e": 50,
              # the engine-fed classes: 85 frames of BIG_N particles make a block of 1 GiB
              "vh": 100, "vhd": 100, "prs": 100, "clu": 100, "dip": 100, "prof": 100, "gyr": 100, "rouse": 100}


def _per_frame(analysis):
    from trajfiles import per_frame
    return per_frame(analysis)


def _reads(u):
    """Record the host blocks an analysis reads (EndToEndVector gathers its chunks itself)."""
    read = u.trajectory.frame_block

    def frame_block(frames):
        _record("frame_block", (frames,))
        return read(frames)
    u.trajectory.frame_block = frame_block
    return u


# ------------------------------------------------------------------------------------------------------ cases

def _rdf(*groups, **kw):
    return RadialDistributionFunction(*groups, n_bins=4, range=(0.0, 5.0), verbose=False, **kw)


def _sq(groups, groupings="atoms", **kw):
    return StructureFactor(groups, groupings, verbose=False, **{"n_points": 2, **kw})


def _isf(groups, groupings="atoms", **kw):
    return IntermediateScatteringFunction(groups, groupings, verbose=False, **{"n_points": 2, "n_lags": 3, **kw})


def _scsf(group, grouping="atoms", **kw):
    return SingleChainStructureFactor(group, grouping, verbose=False, **{"n_points": 2, **kw})


def _e2e(groups, groupings="atoms", **kw):
    return EndToEndVector(groups, groupings, verbose=False, **kw)


def _ons(groups, groupings="atoms", *, hbm_share=None, columns=None, **kw):
    o = Onsager(groups, groupings, temperature=300, verbose=False, **kw)
    if hbm_share is not None:
        o._hbm_share = hbm_share
    if columns is not None:
        o._stream_columns = columns
    return o


def _vh(groups, **kw):
    return VanHove(groups, n_bins=4, range=(0.0, 5.0), verbose=False, **{"n_lags": 3, **kw})


def _vhd(*groups, **kw):
    return DistinctVanHove(*groups, n_bins=4, range=(0.0, 5.0), verbose=False, **{"n_lags": 3, **kw})


def _prs(*groups, **kw):
    return PairResidence(*groups, cutoff=4.0, verbose=False, **{"n_lags": 3, **kw})


UNLIKE = [[0, 3.5], [3.5, 0]]          # a cutoff table of two species: bonds between unlike atoms only


def _clu(groups, cutoff=4.0, **kw):
    return Clusters(groups, cutoff, verbose=False, **kw)


def _dip(groups, **kw):
    n_groups = 1 if hasattr(groups, "universe") else len(groups)
    return DipoleMoment(groups, charges=[0.5 * (g + 1) for g in range(n_groups)], verbose=False, **kw)


def _prof(groups, groupings="atoms", **kw):
    return DensityProfile(groups, groupings, axes="z", n_bins=4, verbose=False, **kw)


def _gyr(groups, groupings="atoms", **kw):
    return Gyradius(groups, groupings, verbose=False, **kw)


def _rouse(groups, groupings="atoms", **kw):
    return RouseModes(groups, groupings, verbose=False, **{"modes": 2, **kw})


def _volumes(analysis):
    """Record ``results.volumes`` of a finished DipoleMoment (the batched route reads them from ``box_block``)."""
    _record("results.volumes", (analysis.results.volumes,))


def _fails(name, analysis):
    """Run ``analysis`` with the recorder ``name`` raising in ``accumulate``."""
    _failing.add(name)
    with pytest.raises(RuntimeError, match=f"{name}.accumulate fails"):
        analysis.run()


CASES = {
    # radial distribution function
    "rdf-memory": ("memory", lambda u: _rdf(u.atoms, exclusion=(1, 1)).run()),
    "rdf-memory-pair-residues-frames": ("memory", lambda u: _rdf(
        u.atoms[:60], u.atoms[60:], groupings="residues", drop_axis="z").run(frames=[0, 2, 3, 7])),
    "rdf-memory-rank1": ("memory", lambda u: _rdf(u.atoms, comm=_Comm(1, 2)).run()),
    "rdf-hbm32": ("hbm32", lambda u: _rdf(u.atoms).run(start=1, stop=9)),
    "rdf-hbm32-frames": ("hbm32", lambda u: _rdf(u.atoms).run(frames=[1, 3, 5])),
    "rdf-hbm32-residues": ("hbm32", lambda u: _rdf(u.atoms, groupings="residues").run()),
    "rdf-hbm32-subset": ("hbm32", lambda u: _rdf(u.atoms[:60]).run()),
    "rdf-hbm64": ("hbm64", lambda u: _rdf(u.atoms).run()),
    "rdf-file": ("file", lambda u: _rdf(u.atoms, drop_axis=0).run(step=2)),
    "rdf-file-pair-residues": ("file", lambda u: _rdf(
        u.atoms[:60], u.atoms[60:], groupings=("residues", "atoms")).run()),
    "rdf-file-frames": ("file", lambda u: _rdf(u.atoms[30:90]).run(frames=[7, 1, 4])),
    "rdf-per-frame": ("memory", lambda u: _per_frame(_rdf(u.atoms[:60], u.atoms[60:])).run()),
    "rdf-blocks": ("big-rdf", lambda u: _rdf(u.atoms).run()),
    # static structure factor
    "sq-memory": ("memory", lambda u: _sq(u.atoms).run()),
    "sq-memory-partial-residues-frames": ("memory", lambda u: _sq(
        (u.atoms[60:], u.atoms[:60]), ("residues", "atoms"), mode="partial").run(frames=[0, 4, 5])),
    "sq-memory-rank1": ("memory", lambda u: _sq(u.atoms, comm=_Comm(1, 2)).run()),
    "sq-hbm32": ("hbm32", lambda u: _sq(u.atoms).run()),
    "sq-hbm32-frames": ("hbm32", lambda u: _sq(u.atoms).run(frames=[0, 2])),
    "sq-hbm32-residues": ("hbm32", lambda u: _sq(u.atoms, "residues").run()),
    "sq-hbm64": ("hbm64", lambda u: _sq(u.atoms).run()),
    "sq-file": ("file", lambda u: _sq(u.atoms).run(stop=6)),
    "sq-file-partial-residues": ("file", lambda u: _sq(
        (u.atoms[60:], u.atoms[:60]), "residues", mode="partial").run(step=3)),
    "sq-per-frame": ("memory", lambda u: _per_frame(_sq(u.atoms)).run()),
    "sq-blocks": ("big-sq", lambda u: _sq(u.atoms, n_points=1).run()),
    # intermediate scattering function
    "isf-memory": ("memory", lambda u: _isf(u.atoms).run()),
    "isf-memory-partial-residues-step": ("memory", lambda u: _isf(
        (u.atoms[:60], u.atoms[60:]), "residues", mode="partial", incoherent=True).run(step=2)),
    "isf-memory-rank1": ("memory", lambda u: _isf(u.atoms, comm=_Comm(1, 2)).run()),
    "isf-memory-rank-without-wavevectors": ("memory", lambda u: _isf(
        u.atoms, n_points=1, n_lags=2, comm=_Comm(1, 2)).run()),
    "isf-hbm32": ("hbm32", lambda u: _isf(u.atoms).run()),
    "isf-hbm64": ("hbm64", lambda u: _isf(u.atoms).run()),
    "isf-file": ("file", lambda u: _isf((u.atoms[:30], u.atoms[30:]), mode="pair").run(start=2)),
    "isf-per-frame": ("memory", lambda u: _per_frame(_isf(u.atoms)).run()),
    "isf-blocks": ("big-isf", lambda u: _isf(u.atoms, n_points=1, n_lags=2).run()),
    # single-chain structure factor
    "scsf-memory": ("memory", lambda u: _scsf(u.atoms).run()),
    "scsf-memory-residues-frames": ("memory", lambda u: _scsf(u.atoms, "residues").run(frames=[1, 2, 6])),
    "scsf-memory-explicit-residues": ("memory", lambda u: _scsf(
        u.atoms[:60], "residues", n_chains=5, n_monomers=4).run()),
    "scsf-memory-rank1": ("memory", lambda u: _scsf(u.atoms, comm=_Comm(1, 2)).run()),
    "scsf-hbm32": ("hbm32", lambda u: _scsf(u.atoms).run()),
    "scsf-hbm32-residues": ("hbm32", lambda u: _scsf(u.atoms, "residues").run()),
    "scsf-hbm64": ("hbm64", lambda u: _scsf(u.atoms).run(step=3)),
    "scsf-file": ("file", lambda u: _scsf(u.atoms).run()),
    "scsf-file-subset": ("file", lambda u: _scsf(u.atoms[12:60]).run(frames=[3, 1])),
    "scsf-per-frame": ("memory", lambda u: _per_frame(_scsf(u.atoms)).run()),
    "scsf-blocks": ("big-scsf", lambda u: _scsf(u.atoms, n_points=1).run()),
    # end-to-end vector
    "e2e-memory": ("memory", lambda u: _e2e(_reads(u).atoms, n_blocks=2).run()),
    "e2e-memory-residues-step": ("memory", lambda u: _e2e(_reads(u).atoms, "residues").run(step=2)),
    "e2e-memory-groups-rank1": ("memory", lambda u: _e2e(
        (_reads(u).atoms[:60], u.atoms[60:]), comm=_Comm(1, 2)).run()),
    "e2e-hbm64": ("hbm64", lambda u: _e2e(_reads(u).atoms).run(frames=[0, 1, 2, 5])),
    "e2e-file": ("file", lambda u: _e2e(_reads(u).atoms, "residues", n_blocks=3).run()),
    "e2e-per-frame": ("memory", lambda u: _per_frame(_e2e(u.atoms)).run()),
    "e2e-blocks": ("big-e2e", lambda u: _e2e(_reads(u).atoms, n_chains=2, n_monomers=BIG_N // 2).run()),
    # Onsager: column-streamed, HBM-resident, group by group from host, file
    "ons-memory-columns": ("memory", lambda u: _ons((u.atoms[:60], u.atoms[60:])).run()),
    "ons-memory-columns-unwrap": ("bonds", lambda u: _ons((u.atoms[:60], u.atoms[60:]), unwrap=True).run()),
    "ons-memory-hbm": ("memory", lambda u: _ons((u.atoms[:60], u.atoms[60:]), columns=False).run()),
    "ons-memory-hbm-zero-dimension": ("memory", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), columns=False, dimensions=[L, L, 0.0]).run()),
    "ons-memory-hbm-residues-centre": ("bonds", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), ("residues", "atoms"), columns=False, unwrap=True, center=True,
        center_wrap=True).run()),
    "ons-memory-hbm-centre-groups": ("memory", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), center=True, n_blocks=2).run()),
    "ons-memory-host": ("memory", lambda u: _ons((u.atoms[:60], u.atoms[60:]), hbm_share=0.0).run()),
    "ons-memory-host-centre-atoms": ("bonds", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), "segments", hbm_share=0.0, unwrap=True, center=True,
        center_atom=True).run(frames=[0, 2, 4, 6])),
    "ons-memory-host-rank1": ("memory", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), ("atoms", "residues"), comm=_Comm(1, 2)).run()),
    "ons-memory-no-fft": ("memory", lambda u: _ons((_reads(u).atoms[:60], u.atoms[60:]), fft=False).run()),
    "ons-memory-no-fft-unwrap": ("memory", lambda u: _ons(_reads(u).atoms[:60], fft=False, unwrap=True).run()),
    "ons-hbm64": ("hbm64", lambda u: _ons((u.atoms[:60], u.atoms[60:])).run()),
    "ons-hbm32-frames": ("hbm32", lambda u: _ons((u.atoms[:60], u.atoms[60:])).run(frames=[0, 2, 4, 6, 8])),
    "ons-hbm32-residues-centre-wrap": ("hbm32", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), "residues", center=True, center_wrap=True).run()),
    "ons-file": ("file", lambda u: _ons((u.atoms[:60], u.atoms[60:]), hbm_share=0.0).run()),
    "ons-file-residues-centre-wrap": ("file", lambda u: _ons(
        (u.atoms[:60], u.atoms[60:]), ("residues", "atoms"), hbm_share=0.0, unwrap=True, center=True,
        center_wrap=True).run()),
    "ons-file-hbm": ("file", lambda u: _ons((u.atoms[:60], u.atoms[60:]), unwrap=True).run(step=2)),
    "ons-per-frame": ("memory", lambda u: _per_frame(_ons((u.atoms[:60], u.atoms[60:]))).run()),
    # self van Hove function
    "vh-memory": ("memory", lambda u: _vh(u.atoms).run()),
    "vh-memory-gather": ("memory", lambda u: _vh((u.atoms[60:], u.atoms[:60])).run(step=2)),
    "vh-hbm32": ("hbm32", lambda u: _vh(u.atoms).run()),
    "vh-hbm32-subset": ("hbm32", lambda u: _vh(u.atoms[30:90]).run(start=1, stop=9)),
    "vh-hbm32-frames": ("hbm32", lambda u: _vh(u.atoms[30:90]).run(frames=[0, 2, 4, 6])),
    "vh-hbm64": ("hbm64", lambda u: _vh(u.atoms).run()),
    "vh-file-subset": ("file", lambda u: _vh(u.atoms[30:90]).run(start=2)),
    "vh-file": ("file", lambda u: _vh(u.atoms).run(stop=6)),
    "vh-per-frame": ("memory", lambda u: _per_frame(_vh(u.atoms[30:90])).run()),
    "vh-blocks": ("big-vh", lambda u: _vh(u.atoms, n_lags=2).run()),
    "vh-memory-unwrap-drop": ("memory", lambda u: _vh(u.atoms, unwrap=True, drop_axis="y").run()),
    "vh-memory-lags-beyond": ("memory", lambda u: _vh(u.atoms[30:90], n_lags=None, lags=[20, 25]).run()),
    # distinct van Hove function
    "vhd-memory": ("memory", lambda u: _vhd(u.atoms).run()),
    "vhd-memory-gather": ("memory", lambda u: _vhd(u.atoms[60:], u.atoms[:60]).run(step=2)),
    "vhd-hbm32": ("hbm32", lambda u: _vhd(u.atoms).run()),
    "vhd-hbm32-subset": ("hbm32", lambda u: _vhd(u.atoms[30:60], u.atoms[90:]).run(start=1, stop=9)),
    "vhd-hbm32-frames": ("hbm32", lambda u: _vhd(u.atoms[30:60], u.atoms[90:]).run(frames=[0, 2, 4, 6])),
    "vhd-hbm64": ("hbm64", lambda u: _vhd(u.atoms).run()),
    "vhd-file-subset": ("file", lambda u: _vhd(u.atoms[30:60], u.atoms[90:]).run(start=2)),
    "vhd-file": ("file", lambda u: _vhd(u.atoms).run(stop=6)),
    "vhd-per-frame": ("memory", lambda u: _per_frame(_vhd(u.atoms[30:60], u.atoms[90:])).run()),
    "vhd-blocks": ("big-vhd", lambda u: _vhd(u.atoms, n_lags=2).run()),
    "vhd-memory-lags-beyond": ("memory", lambda u: _vhd(u.atoms[30:90], n_lags=None, lags=[10]).run()),
    # pair residence
    "prs-memory": ("memory", lambda u: _prs(u.atoms).run()),
    "prs-memory-gather": ("memory", lambda u: _prs(u.atoms[60:], u.atoms[:60]).run(step=2)),
    "prs-hbm32": ("hbm32", lambda u: _prs(u.atoms).run()),
    "prs-hbm32-subset": ("hbm32", lambda u: _prs(u.atoms[30:60], u.atoms[90:]).run(start=1, stop=9)),
    "prs-hbm32-frames": ("hbm32", lambda u: _prs(u.atoms[30:60], u.atoms[90:]).run(frames=[0, 2, 4, 6])),
    "prs-hbm64": ("hbm64", lambda u: _prs(u.atoms).run()),
    "prs-file-subset": ("file", lambda u: _prs(u.atoms[30:60], u.atoms[90:]).run(start=2)),
    "prs-file": ("file", lambda u: _prs(u.atoms).run(stop=6)),
    "prs-per-frame": ("memory", lambda u: _per_frame(_prs(u.atoms[30:60], u.atoms[90:])).run()),
    "prs-blocks": ("big-prs", lambda u: _prs(u.atoms, n_lags=2).run()),
    "prs-memory-lags-beyond": ("memory", lambda u: _prs(u.atoms[30:90], n_lags=None, lags=[12]).run()),
    # clusters
    "clu-memory": ("memory", lambda u: _clu(u.atoms).run()),
    "clu-memory-gather": ("memory", lambda u: _clu((u.atoms[60:], u.atoms[:60]), store_labels=True).run(step=2)),
    "clu-hbm32": ("hbm32", lambda u: _clu(u.atoms).run()),
    "clu-hbm32-subset": ("hbm32", lambda u: _clu((u.atoms[30:60], u.atoms[90:]), UNLIKE).run(start=1, stop=9)),
    "clu-hbm32-frames": ("hbm32", lambda u: _clu(
        (u.atoms[30:60], u.atoms[90:]), UNLIKE).run(frames=[0, 2, 3, 7])),
    "clu-hbm64": ("hbm64", lambda u: _clu(u.atoms).run()),
    "clu-file-subset": ("file", lambda u: _clu((u.atoms[30:60], u.atoms[90:]), UNLIKE).run(start=2)),
    "clu-file": ("file", lambda u: _clu(u.atoms).run(stop=6)),
    "clu-per-frame": ("memory", lambda u: _per_frame(_clu((u.atoms[30:60], u.atoms[90:]), UNLIKE)).run()),
    "clu-blocks": ("big-clu", lambda u: _clu(u.atoms).run()),
    "clu-memory-rank1": ("memory", lambda u: _clu(u.atoms, store_labels=True, comm=_Comm(1, 2)).run()),
    "clu-per-frame-rank1": ("memory", lambda u: _per_frame(_clu(u.atoms[30:90], comm=_Comm(1, 2))).run()),
    "clu-memory-accumulate-raises": ("memory", lambda u: _fails("Cluster", _clu(u.atoms[30:90]))),
    # dipole moments
    "dip-memory": ("memory", lambda u: _volumes(_dip(u.atoms).run())),
    "dip-memory-gather": ("memory", lambda u: _dip((u.atoms[60:], u.atoms[:60])).run(step=2)),
    "dip-hbm32": ("hbm32", lambda u: _volumes(_dip(u.atoms).run())),
    "dip-hbm32-subset": ("hbm32", lambda u: _volumes(_dip((u.atoms[30:60], u.atoms[90:])).run(start=1, stop=9))),
    "dip-hbm32-frames": ("hbm32", lambda u: _volumes(
        _dip((u.atoms[30:60], u.atoms[90:])).run(frames=[0, 2, 3, 7]))),
    "dip-hbm64": ("hbm64", lambda u: _volumes(_dip(u.atoms).run())),
    "dip-file-subset": ("file", lambda u: _volumes(_dip((u.atoms[30:60], u.atoms[90:])).run(start=2))),
    "dip-file": ("file", lambda u: _volumes(_dip(u.atoms).run(stop=6))),
    "dip-per-frame": ("memory", lambda u: _volumes(_per_frame(_dip((u.atoms[30:60], u.atoms[90:]))).run())),
    "dip-blocks": ("big-dip", lambda u: _dip(u.atoms).run()),
    "dip-memory-unwrap": ("bonds", lambda u: _dip(u.atoms, unwrap=True).run(start=3)),
    "dip-memory-rank1": ("memory", lambda u: _volumes(_dip(u.atoms, comm=_Comm(1, 2)).run())),
    "dip-per-frame-rank1": ("memory", lambda u: _volumes(_per_frame(_dip(u.atoms[30:90], comm=_Comm(1, 2))).run())),
    # density profiles
    "prof-memory": ("memory", lambda u: _prof(u.atoms).run()),
    "prof-memory-gather": ("memory", lambda u: _prof((u.atoms[60:], u.atoms[:60]), average=False).run(step=2)),
    "prof-hbm32": ("hbm32", lambda u: _prof(u.atoms).run()),
    "prof-hbm32-subset": ("hbm32", lambda u: _prof((u.atoms[30:60], u.atoms[90:])).run(start=1, stop=9)),
    "prof-hbm32-frames": ("hbm32", lambda u: _prof((u.atoms[30:60], u.atoms[90:])).run(frames=[0, 2, 3, 7])),
    "prof-hbm64": ("hbm64", lambda u: _prof(u.atoms).run()),
    "prof-file-subset": ("file", lambda u: _prof((u.atoms[30:60], u.atoms[90:])).run(start=2)),
    "prof-file": ("file", lambda u: _prof(u.atoms).run(stop=6)),
    "prof-per-frame": ("memory", lambda u: _per_frame(_prof((u.atoms[30:60], u.atoms[90:]))).run()),
    "prof-blocks": ("big-prof", lambda u: _prof(u.atoms).run()),
    "prof-memory-residues": ("memory", lambda u: _prof((u.atoms[60:], u.atoms[:60]), ("residues", "atoms")).run()),
    "prof-file-residues-recenter": ("file", lambda u: _prof(u.atoms, "residues", recenter=0).run()),
    "prof-memory-rank1": ("memory", lambda u: _prof(u.atoms, average=False, comm=_Comm(1, 2)).run()),
    "prof-per-frame-rank1": ("memory", lambda u: _per_frame(_prof(u.atoms[30:90], comm=_Comm(1, 2))).run()),
    # radii of gyration
    "gyr-memory": ("memory", lambda u: _gyr(u.atoms).run()),
    "gyr-memory-gather": ("memory", lambda u: _gyr((u.atoms[60:], u.atoms[:60]), components=True).run(step=2)),
    "gyr-hbm32": ("hbm32", lambda u: _gyr(u.atoms).run()),
    "gyr-hbm32-subset": ("hbm32", lambda u: _gyr((u.atoms[24:60], u.atoms[96:])).run(start=1, stop=9)),
    "gyr-hbm32-frames": ("hbm32", lambda u: _gyr((u.atoms[24:60], u.atoms[96:])).run(frames=[0, 2, 3, 7])),
    "gyr-hbm64": ("hbm64", lambda u: _gyr(u.atoms).run()),
    "gyr-file-subset": ("file", lambda u: _gyr((u.atoms[24:60], u.atoms[96:])).run(start=2)),
    "gyr-file": ("file", lambda u: _gyr(u.atoms).run(stop=6)),
    "gyr-per-frame": ("memory", lambda u: _per_frame(_gyr((u.atoms[24:60], u.atoms[96:]))).run()),
    "gyr-blocks": ("big-gyr", lambda u: _gyr(u.atoms, n_chains=2, n_monomers=BIG_N // 2).run()),
    "gyr-memory-residues-unwrap": ("bonds", lambda u: _gyr(u.atoms, "residues", unwrap=True).run(start=2)),
    "gyr-file-explicit-residues": ("file", lambda u: _gyr(u.atoms[:60], "residues", n_chains=5, n_monomers=4).run()),
    "gyr-memory-rank1": ("memory", lambda u: _gyr(u.atoms, comm=_Comm(1, 2)).run()),
    "gyr-per-frame-rank1": ("memory", lambda u: _per_frame(_gyr(u.atoms[24:60], comm=_Comm(1, 2))).run()),
    # Rouse modes
    "rouse-memory": ("memory", lambda u: _rouse(u.atoms).run()),
    "rouse-memory-gather": ("memory", lambda u: _rouse((u.atoms[60:], u.atoms[:60]), n_blocks=2).run(step=2)),
    "rouse-hbm32": ("hbm32", lambda u: _rouse(u.atoms).run()),
    "rouse-hbm32-subset": ("hbm32", lambda u: _rouse((u.atoms[24:60], u.atoms[96:])).run(start=1, stop=9)),
    "rouse-hbm32-frames": ("hbm32", lambda u: _rouse((u.atoms[24:60], u.atoms[96:])).run(frames=[0, 2, 3, 7])),
    "rouse-hbm64": ("hbm64", lambda u: _rouse(u.atoms).run()),
    "rouse-file-subset": ("file", lambda u: _rouse((u.atoms[24:60], u.atoms[96:])).run(start=2)),
    "rouse-file": ("file", lambda u: _rouse(u.atoms).run(stop=6)),
    "rouse-per-frame": ("memory", lambda u: _per_frame(_rouse((u.atoms[24:60], u.atoms[96:]))).run()),
    "rouse-blocks": ("big-rouse", lambda u: _rouse(u.atoms, modes=1, n_chains=2, n_monomers=BIG_N // 2).run()),
    "rouse-memory-residues-unwrap": ("bonds", lambda u: _rouse(u.atoms, "residues", unwrap=True).run(start=2)),
    "rouse-memory-no-fft": ("memory", lambda u: _rouse(u.atoms[:60], fft=False).run()),
    "rouse-memory-rank1": ("memory", lambda u: _rouse(u.atoms, comm=_Comm(1, 2)).run()),
    "rouse-per-frame-rank1": ("memory", lambda u: _per_frame(_rouse(u.atoms[24:60], comm=_Comm(1, 2))).run()),
}


def trace_of(case, tmp_path):
    kind, run = CASES[case]
    u = _universe(kind, tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run(u)
    return list(_trace)


@pytest.mark.parametrize("case", sorted(CASES))
def test_engine_calls(case, tmp_path):
    assert trace_of(case, tmp_path) == EXPECTED[case]


# a block that raises: the shared run() closes the engine (its stream and HBM) before the error leaves
FAILING = {
    "VanHove": (lambda u: _vh(u.atoms[30:90]), "30..89"),
    "DistinctVanHove": (lambda u: _vhd(u.atoms[30:60], u.atoms[90:]), "30..59,90..119"),
    "Residence": (lambda u: _prs(u.atoms[30:60], u.atoms[90:]), "30..59,90..119"),
    "Dipole": (lambda u: _dip(u.atoms[30:90]), "30..89"),
    "Profile": (lambda u: _prof(u.atoms[30:90]), "30..89"),
    "Gyration": (lambda u: _gyr(u.atoms[24:60]), "24..59"),
    "Projection": (lambda u: _rouse(u.atoms[24:60]), "24..59"),
}


@pytest.mark.parametrize("name", sorted(FAILING))
def test_engine_closed_when_a_block_raises(name, tmp_path):
    make, atoms = FAILING[name]
    _fails(name, make(_universe("memory", tmp_path)))
    assert _trace[-2:] == [f"{name}.accumulate(pos32[0..9 | {atoms}])", f"{name}.close()"]


# the engine calls of every case
EXPECTED = {'e2e-blocks': ['frame_block(0..20)',
                'frame_block(21..41)',
                'frame_block(42..49)',
                'Msd(50, 1, 1, dev=0)',
                'Msd.push(0, pos64<(50, 2, 3) #b527751bf4>, 0, 2, 0)',
                'Msd.result_acf()',
                'Msd.close()'],
 'e2e-file': ['frame_block(0..9)',
              'Msd(3, 3, 1, dev=0)',
              'Msd.push(0, pos64<(9, 10, 3) #2f3a5ecd0e>, 0, 10, 0)',
              'Msd.result_acf()',
              'Msd.close()'],
 'e2e-hbm64': ['frame_block(0..2,5)',
               'to_host(0, 1)',
               'to_host(1, 1)',
               'to_host(2, 1)',
               'to_host(5, 1)',
               'Msd(4, 1, 1, dev=0)',
               'Msd.push(0, pos64<(4, 10, 3) #012a9b174e>, 0, 10, 0)',
               'Msd.result_acf()',
               'Msd.close()'],
 'e2e-memory': ['frame_block(0..9)',
                'Msd(5, 2, 1, dev=0)',
                'Msd.push(0, pos64<(10, 10, 3) #a89b1ecfac>, 0, 10, 0)',
                'Msd.result_acf()',
                'Msd.close()'],
 'e2e-memory-groups-rank1': ['frame_block(0..9)',
                             'Msd(10, 1, 2, dev=0)',
                             'Msd.push(0, pos64<(10, 10, 3) #a89b1ecfac>, 3, 2, 0)',
                             'Msd.push(1, pos64<(10, 10, 3) #a89b1ecfac>, 8, 2, 0)',
                             'Msd.result_acf()',
                             'Msd.close()'],
 'e2e-memory-residues-step': ['frame_block(0,2,4,6,8)',
                              'Msd(5, 1, 1, dev=0)',
                              'Msd.push(0, pos64<(5, 10, 3) #6d8a789238>, 0, 10, 0)',
                              'Msd.result_acf()',
                              'Msd.close()'],
 'e2e-per-frame': ['Msd(10, 1, 1, dev=0)',
                   'Msd.push(0, pos64<(10, 10, 3) #a89b1ecfac>, 0, 10, 0)',
                   'Msd.result_acf()',
                   'Msd.close()'],
 'isf-blocks': ['Isf([0 0 0], 1048576, ((None, None)), 2, False, dev=0)',
                'Isf.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'Isf.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'Isf.result()',
                'Isf.close()'],
 'isf-file': ['Isf(<(8, 3) #2e53c0a7cb>, 30,90, (0..1), 3, False, dev=0)',
              'Isf.accumulate_traj(file, 2..9, None)',
              'Isf.result()',
              'Isf.close()'],
 'isf-hbm32': ['Isf(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), 3, False, dev=0)',
               'rows(0, 10)',
               "Isf.accumulate_device('rows0+10', 120, 10)",
               'Isf.result()',
               'Isf.close()'],
 'isf-hbm64': ['Isf(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), 3, False, dev=0)',
               'to_host(0, 10)',
               'Isf.accumulate(pos64[0..9 | 0..119])',
               'Isf.result()',
               'Isf.close()'],
 'isf-memory': ['Isf(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), 3, False, dev=0)',
                'Isf.accumulate(pos32[0..9 | 0..119])',
                'Isf.result()',
                'Isf.close()'],
 'isf-memory-partial-residues-step': ['Isf(<(8, 3) #2e53c0a7cb>, 20x2, (0x2, 0..1, 1x2), 3, True, dev=0)',
                                      'Isf.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                                      'Isf.accumulate(pos32[0,2,4,6,8 | 0..119])',
                                      'Isf.result()',
                                      'Isf.close()'],
 'isf-memory-rank-without-wavevectors': [],
 'isf-memory-rank1': ['Isf(<(4, 3) #0f6f6152c3>, 120, ((None, None)), 3, False, dev=0)',
                      'Isf.accumulate(pos32[0..9 | 0..119])',
                      'Isf.result()',
                      'Isf.close()'],
 'isf-per-frame': ['Isf(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), 3, False, dev=0)',
                   'Isf.accumulate(pos32[0..9 | 0..119])',
                   'Isf.result()',
                   'Isf.close()'],
 'ons-file': ['Msd(10, 1, 2, dev=0)',
              'Msd.set_grouping(None, None)',
              'Msd.push_traj(0, file, 0..9, 0..59, shift=None, unwrap_dims=None, zero_dims=0)',
              'Msd.set_grouping(None, None)',
              'Msd.push_traj(1, file, 0..9, 60..119, shift=None, unwrap_dims=None, zero_dims=0)',
              'Msd.result()',
              'Msd.cross((0x2, 0..1, 1x2))',
              'Msd.close()'],
 'ons-file-hbm': ['Msd(5, 1, 2, dev=0)',
                  'device_info()',
                  'DeviceArray->d0(5,120,3, float32)',
                  "file.load_device(0,2,4,6,8, 'd0')",
                  'Msd.set_grouping(None, None)',
                  'Msd.set_initial_images(None)',
                  'Msd.push_frames_device(0, d0, 120, 0..59, shift=None, unwrap_dims=[50 50 50], zero_dims=0)',
                  'Msd.set_grouping(None, None)',
                  'Msd.set_initial_images(None)',
                  'Msd.push_frames_device(1, d0, 120, 60..119, shift=None, unwrap_dims=[50 50 50], zero_dims=0)',
                  'synchronize()',
                  'd0.free()',
                  'Msd.result()',
                  'Msd.cross((0x2, 0..1, 1x2))',
                  'Msd.close()'],
 'ons-file-residues-centre-wrap': ['Msd(10, 1, 2, dev=0)',
                                   'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                   'Msd.set_initial_images(None)',
                                   'Msd.system_com_traj(file, 0..9, 0..59, <(60,) #b2c88767f2>, unwrap_dims=[50 50 '
                                   '50], wrap_dims=[50 50 50])',
                                   'Msd.set_grouping(None, None)',
                                   'Msd.set_initial_images(None)',
                                   'Msd.system_com_traj(file, 0..9, 60..119, <(60,) #9693887936>, unwrap_dims=[50 '
                                   '50 50], wrap_dims=[50 50 50])',
                                   'Msd.set_grouping(None, None)',
                                   'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                   'Msd.set_initial_images(None)',
                                   'Msd.push_traj(0, file, 0..9, 0..59, shift=<(10, 3) #de0e7c9e49>, '
                                   'unwrap_dims=[50 50 50], zero_dims=0)',
                                   'Msd.set_grouping(None, None)',
                                   'Msd.set_initial_images(None)',
                                   'Msd.push_traj(1, file, 0..9, 60..119, shift=<(10, 3) #de0e7c9e49>, '
                                   'unwrap_dims=[50 50 50], zero_dims=0)',
                                   'Msd.result()',
                                   'Msd.cross((0x2, 0..1, 1x2))',
                                   'Msd.close()'],
 'ons-hbm32-frames': ['Msd(5, 1, 2, dev=0)',
                      'device_info()',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(4, 1)',
                      'to_host(6, 1)',
                      'to_host(8, 1)',
                      'DeviceArray.upload->d0(pos32[0,2,4,6,8 | 0..119])',
                      'Msd.set_grouping(None, None)',
                      "Msd.push_device_f32(0, 'd0', 120, 0, 60, 0)",
                      'Msd.set_grouping(None, None)',
                      "Msd.push_device_f32(1, 'd0', 120, 60, 60, 0)",
                      'synchronize()',
                      'd0.free()',
                      'Msd.result()',
                      'Msd.cross((0x2, 0..1, 1x2))',
                      'Msd.close()'],
 'ons-hbm32-residues-centre-wrap': ['Msd(10, 1, 2, dev=0)',
                                    'rows(0, 10)',
                                    'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                    'Msd.system_com_device(rows0+10, 120, 0..59, <(60,) #b2c88767f2>, '
                                    'unwrap_dims=None, wrap_dims=[50 50 50])',
                                    'Msd.set_grouping(0..60/3, <(60,) #9693887936>)',
                                    'Msd.system_com_device(rows0+10, 120, 60..119, <(60,) #9693887936>, '
                                    'unwrap_dims=None, wrap_dims=[50 50 50])',
                                    'Msd.set_grouping(None, None)',
                                    'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                    'Msd.push_frames_device(0, rows0+10, 120, 0..59, shift=<(10, 3) #de0e7c9e49>, '
                                    'unwrap_dims=None, zero_dims=0)',
                                    'Msd.set_grouping(0..60/3, <(60,) #9693887936>)',
                                    'Msd.push_frames_device(1, rows0+10, 120, 60..119, shift=<(10, 3) '
                                    '#de0e7c9e49>, unwrap_dims=None, zero_dims=0)',
                                    'Msd.result()',
                                    'Msd.cross((0x2, 0..1, 1x2))',
                                    'Msd.close()'],
 'ons-hbm64': ['Msd(10, 1, 2, dev=0)',
               'rows(0, 10)',
               'Msd.set_grouping(None, None)',
               "Msd.push_device(0, 'rows0+10', 120, 0, 60, 0)",
               'Msd.set_grouping(None, None)',
               "Msd.push_device(1, 'rows0+10', 120, 60, 60, 0)",
               'Msd.result()',
               'Msd.cross((0x2, 0..1, 1x2))',
               'Msd.close()'],
 'ons-memory-columns': ['Msd(10, 1, 2, dev=0)',
                        'device_info()',
                        'DeviceArray->d0(10,32,3, float32)',
                        'DeviceArray->d1(10,32,3, float32)',
                        'Msd.set_grouping(None, None)',
                        'd0.upload_columns(pos32[0..9 | 0..119], 0, 32)',
                        'Msd.synchronize()',
                        "Msd.push_device_f32(0, 'd0', 32, 0, 32, 0)",
                        'd1.upload_columns(pos32[0..9 | 0..119], 32, 28)',
                        'Msd.synchronize()',
                        "Msd.push_device_f32(0, 'd1', 28, 0, 28, 0)",
                        'd0.upload_columns(pos32[0..9 | 0..119], 60, 32)',
                        'Msd.synchronize()',
                        "Msd.push_device_f32(1, 'd0', 32, 0, 32, 0)",
                        'd1.upload_columns(pos32[0..9 | 0..119], 92, 28)',
                        'Msd.synchronize()',
                        "Msd.push_device_f32(1, 'd1', 28, 0, 28, 0)",
                        'Msd.synchronize()',
                        'd0.free()',
                        'd1.free()',
                        'Msd.result()',
                        'Msd.cross((0x2, 0..1, 1x2))',
                        'Msd.close()'],
 'ons-memory-columns-unwrap': ['Msd(10, 1, 2, dev=0)',
                               'device_info()',
                               'DeviceArray->d0(10,32,3, float32)',
                               'DeviceArray->d1(10,32,3, float32)',
                               'Msd.set_grouping(None, None)',
                               'd0.upload_columns(pos32[0..9 | 0..119], 0, 32)',
                               'Msd.synchronize()',
                               'Msd.set_initial_images(0x96)',
                               'Msd.push_frames_device(0, d0, 32, None, unwrap_dims=[50 50 50], zero_dims=0)',
                               'd1.upload_columns(pos32[0..9 | 0..119], 32, 28)',
                               'Msd.synchronize()',
                               'Msd.set_initial_images(0x84)',
                               'Msd.push_frames_device(0, d1, 28, None, unwrap_dims=[50 50 50], zero_dims=0)',
                               'd0.upload_columns(pos32[0..9 | 0..119], 60, 32)',
                               'Msd.synchronize()',
                               'Msd.set_initial_images(<96 ints #e2886559b2>)',
                               'Msd.push_frames_device(1, d0, 32, None, unwrap_dims=[50 50 50], zero_dims=0)',
                               'd1.upload_columns(pos32[0..9 | 0..119], 92, 28)',
                               'Msd.synchronize()',
                               'Msd.set_initial_images(<84 ints #183a84c578>)',
                               'Msd.push_frames_device(1, d1, 28, None, unwrap_dims=[50 50 50], zero_dims=0)',
                               'Msd.synchronize()',
                               'd0.free()',
                               'd1.free()',
                               'Msd.result()',
                               'Msd.cross((0x2, 0..1, 1x2))',
                               'Msd.close()'],
 'ons-memory-hbm': ['Msd(10, 1, 2, dev=0)',
                    'device_info()',
                    'DeviceArray.upload->d0(pos32[0..9 | 0..119])',
                    'Msd.set_grouping(None, None)',
                    "Msd.push_device_f32(0, 'd0', 120, 0, 60, 0)",
                    'Msd.set_grouping(None, None)',
                    "Msd.push_device_f32(1, 'd0', 120, 60, 60, 0)",
                    'synchronize()',
                    'd0.free()',
                    'Msd.result()',
                    'Msd.cross((0x2, 0..1, 1x2))',
                    'Msd.close()'],
 'ons-memory-hbm-centre-groups': ['Msd(5, 2, 2, dev=0)',
                                  'device_info()',
                                  'DeviceArray.upload->d0(pos32[0..9 | 0..119])',
                                  'Msd.system_com_device(d0, 120, 0..119, <(120,) #2a35702bbc>, unwrap_dims=None, '
                                  'wrap_dims=None)',
                                  'Msd.set_grouping(None, None)',
                                  'Msd.push_frames_device(0, d0, 120, 0..59, shift=<(10, 3) #de0e7c9e49>, '
                                  'unwrap_dims=None, zero_dims=0)',
                                  'Msd.set_grouping(None, None)',
                                  'Msd.push_frames_device(1, d0, 120, 60..119, shift=<(10, 3) #de0e7c9e49>, '
                                  'unwrap_dims=None, zero_dims=0)',
                                  'synchronize()',
                                  'd0.free()',
                                  'Msd.result()',
                                  'Msd.cross((0x2, 0..1, 1x2))',
                                  'Msd.close()'],
 'ons-memory-hbm-residues-centre': ['Msd(10, 1, 2, dev=0)',
                                    'device_info()',
                                    'DeviceArray.upload->d0(pos32[0..9 | 0..119])',
                                    'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                    'Msd.set_initial_images(0x180)',
                                    'Msd.system_com_device(d0, 120, 0..59, <(60,) #b2c88767f2>, unwrap_dims=[50 50 '
                                    '50], wrap_dims=[50 50 50])',
                                    'Msd.set_grouping(None, None)',
                                    'Msd.set_initial_images(<180 ints #d4fd0e19a7>)',
                                    'Msd.system_com_device(d0, 120, 60..119, <(60,) #9693887936>, unwrap_dims=[50 '
                                    '50 50], wrap_dims=[50 50 50])',
                                    'Msd.set_grouping(None, None)',
                                    'Msd.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                    'Msd.set_initial_images(0x180)',
                                    'Msd.push_frames_device(0, d0, 120, 0..59, shift=<(10, 3) #de0e7c9e49>, '
                                    'unwrap_dims=[50 50 50], zero_dims=0)',
                                    'Msd.set_grouping(None, None)',
                                    'Msd.set_initial_images(<180 ints #d4fd0e19a7>)',
                                    'Msd.push_frames_device(1, d0, 120, 60..119, shift=<(10, 3) #de0e7c9e49>, '
                                    'unwrap_dims=[50 50 50], zero_dims=0)',
                                    'synchronize()',
                                    'd0.free()',
                                    'Msd.result()',
                                    'Msd.cross((0x2, 0..1, 1x2))',
                                    'Msd.close()'],
 'ons-memory-hbm-zero-dimension': ['Msd(10, 1, 2, dev=0)',
                                   'device_info()',
                                   'DeviceArray.upload->d0(pos32[0..9 | 0..119])',
                                   'Msd.set_grouping(None, None)',
                                   "Msd.push_device_f32(0, 'd0', 120, 0, 60, 4)",
                                   'Msd.set_grouping(None, None)',
                                   "Msd.push_device_f32(1, 'd0', 120, 60, 60, 4)",
                                   'synchronize()',
                                   'd0.free()',
                                   'Msd.result()',
                                   'Msd.cross((0x2, 0..1, 1x2))',
                                   'Msd.close()'],
 'ons-memory-host': ['Msd(10, 1, 2, dev=0)',
                     'Msd.set_grouping(None, None)',
                     'Msd.push_f32(0, pos32[0..9 | 0..59], shift=None, unwrap_dims=None, zero_dims=0)',
                     'Msd.set_grouping(None, None)',
                     'Msd.push_f32(1, pos32[0..9 | 60..119], shift=None, unwrap_dims=None, zero_dims=0)',
                     'Msd.result()',
                     'Msd.cross((0x2, 0..1, 1x2))',
                     'Msd.close()'],
 'ons-memory-host-centre-atoms': ['Msd(4, 1, 2, dev=0)',
                                  'Msd.set_initial_images(<360 ints #2d8b052067>)',
                                  'Msd.system_com_f32(pos32[0,2,4,6 | 0..119], <(120,) #2a35702bbc>, '
                                  'unwrap_dims=[50 50 50], wrap_dims=None)',
                                  'Msd.set_grouping(0,12,24,36,48,60, <(60,) #b2c88767f2>)',
                                  'Msd.set_initial_images(0x180)',
                                  'Msd.push_f32(0, pos32[0,2,4,6 | 0..59], shift=<(4, 3) #c49a9785b2>, '
                                  'unwrap_dims=[50 50 50], zero_dims=0)',
                                  'Msd.set_grouping(0,12,24,36,48,60, <(60,) #9693887936>)',
                                  'Msd.set_initial_images(<180 ints #d4fd0e19a7>)',
                                  'Msd.push_f32(1, pos32[0,2,4,6 | 60..119], shift=<(4, 3) #c49a9785b2>, '
                                  'unwrap_dims=[50 50 50], zero_dims=0)',
                                  'Msd.result()',
                                  'Msd.cross((0x2, 0..1, 1x2))',
                                  'Msd.close()'],
 'ons-memory-host-rank1': ['Msd(10, 1, 2, dev=0)',
                           'Msd.set_grouping(None, None)',
                           'Msd.push_f32(0, pos32[0..9 | 30..59], shift=None, unwrap_dims=None, zero_dims=0)',
                           'Msd.set_grouping(0..30/3, <(30,) #dff639c600>)',
                           'Msd.push_f32(1, pos32[0..9 | 90..119], shift=None, unwrap_dims=None, zero_dims=0)',
                           'Msd.result()',
                           'Msd.close()',
                           'correlate_device(3,10, True, False)',
                           'correlate_device(3,10, False, True)',
                           'correlate_device(3,10, True, False)'],
 'ons-memory-no-fft': ['frame_block(0..9)'],
 'ons-memory-no-fft-unwrap': [],
 'ons-per-frame': ['Msd(10, 1, 2, dev=0)',
                   'Msd.push(0, pos64[0..9 | 0..119], 0, 60, 0)',
                   'Msd.push(1, pos64[0..9 | 0..119], 60, 60, 0)',
                   'Msd.result()',
                   'Msd.cross((0x2, 0..1, 1x2))',
                   'Msd.close()'],
 'rdf-blocks': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                'Rdf.set_drop_axis(None)',
                'Rdf.accumulate(pos32<zero-stride (341, 1048576, 3)>, None, box[0x341])',
                'Rdf.accumulate(pos32<zero-stride (59, 1048576, 3)>, None, box[0x59])',
                'Rdf.counts()',
                'Rdf.close()'],
 'rdf-file': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
              'Rdf.set_drop_axis(0)',
              'Rdf.accumulate_traj(file, 0,2,4,6,8, box[0,2,4,6,8], None, None, same=True)',
              'Rdf.counts()',
              'Rdf.close()'],
 'rdf-file-frames': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                     'Rdf.set_drop_axis(None)',
                     'Rdf.accumulate_traj(file, 7,1,4, box[7,1,4], 30..89, None, same=True)',
                     'Rdf.counts()',
                     'Rdf.close()'],
 'rdf-file-pair-residues': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                            'Rdf.set_grouping(1, 0..60/3, <(60,) #b2c88767f2>)',
                            'Rdf.set_drop_axis(None)',
                            'Rdf.accumulate_traj(file, 0..9, box[0..9], 0..59, 60..119, same=False)',
                            'Rdf.counts()',
                            'Rdf.close()'],
 'rdf-hbm32': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
               'Rdf.set_drop_axis(None)',
               'rows(1, 8)',
               'DeviceArray.from_host->d0(box[1..8])',
               "Rdf.accumulate_device('rows1+8', 120, None, 120, 'd0', 8)",
               'Rdf.synchronize()',
               'd0.free()',
               'Rdf.counts()',
               'Rdf.close()'],
 'rdf-hbm32-frames': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                      'Rdf.set_drop_axis(None)',
                      'to_host(1, 1)',
                      'to_host(3, 1)',
                      'to_host(5, 1)',
                      'Rdf.accumulate(pos32[1,3,5 | 0..119], None, box[1,3,5])',
                      'Rdf.counts()',
                      'Rdf.close()'],
 'rdf-hbm32-residues': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                        'Rdf.set_grouping(1, 0..120/3, <(120,) #2a35702bbc>)',
                        'Rdf.set_drop_axis(None)',
                        'to_host(0, 10)',
                        'Rdf.accumulate(pos32[0..9 | 0..119], None, box[0..9])',
                        'Rdf.counts()',
                        'Rdf.close()'],
 'rdf-hbm32-subset': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                      'Rdf.set_drop_axis(None)',
                      'to_host(0, 10)',
                      'Rdf.accumulate(pos32[0..9 | 0..59], None, box[0..9])',
                      'Rdf.counts()',
                      'Rdf.close()'],
 'rdf-hbm64': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
               'Rdf.set_drop_axis(None)',
               'to_host(0, 10)',
               'Rdf.accumulate(pos64[0..9 | 0..119], None, box[0..9])',
               'Rdf.counts()',
               'Rdf.close()'],
 'rdf-memory': ["Rdf([0 1.25 2.5 3.75 5], 1x2, algo='auto', dev=0)",
                'Rdf.set_drop_axis(None)',
                'Rdf.accumulate(pos32[0..9 | 0..119], None, box[0..9])',
                'Rdf.counts()',
                'Rdf.close()'],
 'rdf-memory-pair-residues-frames': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                                     'Rdf.set_grouping(1, 0..60/3, <(60,) #b2c88767f2>)',
                                     'Rdf.set_grouping(2, 0..60/3, <(60,) #9693887936>)',
                                     'Rdf.set_drop_axis(2)',
                                     'Rdf.accumulate(pos32[0,2..3,7 | 0..59], pos32[0,2..3,7 | 60..119], '
                                     'box[0,2..3,7])',
                                     'Rdf.counts()',
                                     'Rdf.close()'],
 'rdf-memory-rank1': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                      'Rdf.set_drop_axis(None)',
                      'Rdf.accumulate(pos32[5..9 | 0..119], None, box[5..9])',
                      'Rdf.counts()',
                      'Rdf.close()'],
 'rdf-per-frame': ["Rdf([0 1.25 2.5 3.75 5], None, algo='auto', dev=0)",
                   'Rdf.accumulate(pos32[0..9 | 0..59], pos32[0..9 | 60..119], box[0..9])',
                   'Rdf.counts()',
                   'Rdf.close()'],
 'scsf-blocks': ['Sq([0 0 0], 1048576, ((None, None)), dev=0)',
                 'Sq.set_chains(1048576)',
                 'Sq.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                 'Sq.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                 'Sq.result()',
                 'Sq.close()'],
 'scsf-file': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
               'Sq.set_chains(12)',
               'Sq.accumulate_traj(file, 0..9, None)',
               'Sq.result()',
               'Sq.close()'],
 'scsf-file-subset': ['Sq(<(8, 3) #2e53c0a7cb>, 48, ((None, None)), dev=0)',
                      'Sq.set_chains(12)',
                      'Sq.accumulate_traj(file, 3,1, 12..59)',
                      'Sq.result()',
                      'Sq.close()'],
 'scsf-hbm32': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                'Sq.set_chains(12)',
                'rows(0, 10)',
                "Sq.accumulate_device('rows0+10', 120, 10)",
                'Sq.result()',
                'Sq.close()'],
 'scsf-hbm32-residues': ['Sq(<(8, 3) #2e53c0a7cb>, 40, ((None, None)), dev=0)',
                         'Sq.set_chains(4)',
                         'Sq.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                         'to_host(0, 10)',
                         'Sq.accumulate(pos32[0..9 | 0..119])',
                         'Sq.result()',
                         'Sq.close()'],
 'scsf-hbm64': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                'Sq.set_chains(12)',
                'to_host(0, 1)',
                'to_host(3, 1)',
                'to_host(6, 1)',
                'to_host(9, 1)',
                'Sq.accumulate(pos64[0,3,6,9 | 0..119])',
                'Sq.result()',
                'Sq.close()'],
 'scsf-memory': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                 'Sq.set_chains(12)',
                 'Sq.accumulate(pos32[0..9 | 0..119])',
                 'Sq.result()',
                 'Sq.close()'],
 'scsf-memory-explicit-residues': ['Sq(<(8, 3) #2e53c0a7cb>, 20, ((None, None)), dev=0)',
                                   'Sq.set_chains(4)',
                                   'Sq.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                   'Sq.accumulate(pos32[0..9 | 0..59])',
                                   'Sq.result()',
                                   'Sq.close()'],
 'scsf-memory-rank1': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                       'Sq.set_chains(12)',
                       'Sq.accumulate(pos32[5..9 | 0..119])',
                       'Sq.result()',
                       'Sq.close()'],
 'scsf-memory-residues-frames': ['Sq(<(8, 3) #2e53c0a7cb>, 40, ((None, None)), dev=0)',
                                 'Sq.set_chains(4)',
                                 'Sq.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                                 'Sq.accumulate(pos32[1..2,6 | 0..119])',
                                 'Sq.result()',
                                 'Sq.close()'],
 'scsf-per-frame': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                    'Sq.set_chains(12)',
                    'Sq.accumulate(pos32[0..9 | 0..119])',
                    'Sq.result()',
                    'Sq.close()'],
 'sq-blocks': ['Sq([0 0 0], 1048576, ((None, None)), dev=0)',
               'Sq.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
               'Sq.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
               'Sq.result()',
               'Sq.close()'],
 'sq-file': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
             'Sq.accumulate_traj(file, 0..5, None)',
             'Sq.result()',
             'Sq.close()'],
 'sq-file-partial-residues': ['Sq(<(8, 3) #2e53c0a7cb>, 20x2, (0x2, 0..1, 1x2), dev=0)',
                              'Sq.set_grouping(0..120/3, <(120,) #f985569a2d>)',
                              'Sq.accumulate_traj(file, 0,3,6,9, 60..119,0..59)',
                              'Sq.result()',
                              'Sq.close()'],
 'sq-hbm32': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
              'rows(0, 10)',
              "Sq.accumulate_device('rows0+10', 120, 10)",
              'Sq.result()',
              'Sq.close()'],
 'sq-hbm32-frames': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                     'to_host(0, 1)',
                     'to_host(2, 1)',
                     'Sq.accumulate(pos32[0,2 | 0..119])',
                     'Sq.result()',
                     'Sq.close()'],
 'sq-hbm32-residues': ['Sq(<(8, 3) #2e53c0a7cb>, 40, ((None, None)), dev=0)',
                       'Sq.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                       'to_host(0, 10)',
                       'Sq.accumulate(pos32[0..9 | 0..119])',
                       'Sq.result()',
                       'Sq.close()'],
 'sq-hbm64': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
              'to_host(0, 10)',
              'Sq.accumulate(pos64[0..9 | 0..119])',
              'Sq.result()',
              'Sq.close()'],
 'sq-memory': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
               'Sq.accumulate(pos32[0..9 | 0..119])',
               'Sq.result()',
               'Sq.close()'],
 'sq-memory-partial-residues-frames': ['Sq(<(8, 3) #2e53c0a7cb>, 20,60, (0x2, 0..1, 1x2), dev=0)',
                                       'Sq.set_grouping(<81 ints #95475c9bc2>, <(120,) #7f4d5a97af>)',
                                       'Sq.accumulate(pos32[0,4..5 | 60..119,0..59])',
                                       'Sq.result()',
                                       'Sq.close()'],
 'sq-memory-rank1': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                     'Sq.accumulate(pos32[5..9 | 0..119])',
                     'Sq.result()',
                     'Sq.close()'],
 'sq-per-frame': ['Sq(<(8, 3) #2e53c0a7cb>, 120, ((None, None)), dev=0)',
                  'Sq.accumulate(pos32[0..9 | 0..119])',
                  'Sq.result()',
                  'Sq.close()']}


# ... and those of the engine-fed classes (VanHove, DistinctVanHove, PairResidence, Clusters, DipoleMoment,
# DensityProfile, Gyradius, RouseModes), recorded while each class still had a run() of its own
EXPECTED.update(
{'clu-blocks': ['Cluster(0x1048576, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, '
                'zero_dims=0)',
                'Cluster.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'Cluster.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'Cluster.result()',
                'Cluster.frames()',
                'Cluster.close()'],
 'clu-file': ['Cluster(0x120, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, zero_dims=0)',
              'Cluster.accumulate_traj(file, 0..5, None)',
              'Cluster.result()',
              'Cluster.frames()',
              'Cluster.close()'],
 'clu-file-subset': ['Cluster(<60 ints #0f7eb7b687>, [0 3.5 3.5 0], [50 50 50], dev=0, keep_labels=False, '
                     'max_neighbors=32, n_species=2, zero_dims=0)',
                     'Cluster.accumulate_traj(file, 2..9, 30..59,90..119)',
                     'Cluster.result()',
                     'Cluster.frames()',
                     'Cluster.close()'],
 'clu-hbm32': ['Cluster(0x120, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, zero_dims=0)',
               'rows(0, 10)',
               "Cluster.accumulate_device('rows0+10', 120, 10, None)",
               'Cluster.result()',
               'Cluster.frames()',
               'Cluster.close()'],
 'clu-hbm32-frames': ['Cluster(<60 ints #0f7eb7b687>, [0 3.5 3.5 0], [50 50 50], dev=0, keep_labels=False, '
                      'max_neighbors=32, n_species=2, zero_dims=0)',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(3, 1)',
                      'to_host(7, 1)',
                      'Cluster.accumulate(pos32[0,2..3,7 | 30..59,90..119])',
                      'Cluster.result()',
                      'Cluster.frames()',
                      'Cluster.close()'],
 'clu-hbm32-subset': ['Cluster(<60 ints #0f7eb7b687>, [0 3.5 3.5 0], [50 50 50], dev=0, keep_labels=False, '
                      'max_neighbors=32, n_species=2, zero_dims=0)',
                      'rows(1, 8)',
                      "Cluster.accumulate_device('rows1+8', 120, 8, 30..59,90..119)",
                      'Cluster.result()',
                      'Cluster.frames()',
                      'Cluster.close()'],
 'clu-hbm64': ['Cluster(0x120, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, zero_dims=0)',
               'to_host(0, 10)',
               'Cluster.accumulate(pos64[0..9 | 0..119])',
               'Cluster.result()',
               'Cluster.frames()',
               'Cluster.close()'],
 'clu-memory': ['Cluster(0x120, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, zero_dims=0)',
                'Cluster.accumulate(pos32[0..9 | 0..119])',
                'Cluster.result()',
                'Cluster.frames()',
                'Cluster.close()'],
 'clu-memory-accumulate-raises': ['Cluster(0x60, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, '
                                  'n_species=1, zero_dims=0)',
                                  'Cluster.accumulate(pos32[0..9 | 30..89])',
                                  'Cluster.close()'],
 'clu-memory-gather': ['Cluster(<120 ints #ffb434c782>, [4 4 4 4], [50 50 50], dev=0, keep_labels=True, '
                       'max_neighbors=32, n_species=2, zero_dims=0)',
                       'Cluster.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                       'Cluster.result()',
                       'Cluster.frames()',
                       'Cluster.labels()',
                       'Cluster.close()'],
 'clu-memory-rank1': ['Cluster(0x120, [4], [50 50 50], dev=0, keep_labels=True, max_neighbors=32, n_species=1, '
                      'zero_dims=0)',
                      'Cluster.accumulate(pos32[5..9 | 0..119])',
                      'Cluster.result()',
                      'Cluster.frames()',
                      'Cluster.labels()',
                      'Cluster.close()'],
 'clu-per-frame': ['Cluster(<60 ints #0f7eb7b687>, [0 3.5 3.5 0], [50 50 50], dev=0, keep_labels=False, '
                   'max_neighbors=32, n_species=2, zero_dims=0)',
                   'Cluster.accumulate(pos32[0..9 | 30..59,90..119])',
                   'Cluster.result()',
                   'Cluster.frames()',
                   'Cluster.close()'],
 'clu-per-frame-rank1': ['Cluster(0x60, [4], [50 50 50], dev=0, keep_labels=False, max_neighbors=32, n_species=1, '
                         'zero_dims=0)',
                         'Cluster.accumulate(pos32[5..9 | 30..89])',
                         'Cluster.result()',
                         'Cluster.frames()',
                         'Cluster.close()'],
 'dip-blocks': ['Dipole(1048576, <(1048576,) #14c194b18a>, dev=0)',
                'Dipole.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'Dipole.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'Dipole.result()',
                'Dipole.close()'],
 'dip-file': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
              'Dipole.accumulate_traj(file, 0..5, None)',
              'Dipole.result()',
              'Dipole.close()',
              'results.volumes([125000 125312 125625 125938 126250 126562])'],
 'dip-file-subset': ['Dipole(30x2, <(60,) #12b5303bb1>, dev=0)',
                     'Dipole.accumulate_traj(file, 2..9, 30..59,90..119)',
                     'Dipole.result()',
                     'Dipole.close()',
                     'results.volumes([125625 125938 126250 126562 126875 127188 127500 127812])'],
 'dip-hbm32': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
               'rows(0, 10)',
               "Dipole.accumulate_device('rows0+10', 120, 10, None)",
               'Dipole.result()',
               'Dipole.close()',
               'results.volumes(<(10,) #e82c6627dc>)'],
 'dip-hbm32-frames': ['Dipole(30x2, <(60,) #12b5303bb1>, dev=0)',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(3, 1)',
                      'to_host(7, 1)',
                      'Dipole.accumulate(pos32[0,2..3,7 | 30..59,90..119])',
                      'Dipole.result()',
                      'Dipole.close()',
                      'results.volumes([125000 125625 125938 127188])'],
 'dip-hbm32-subset': ['Dipole(30x2, <(60,) #12b5303bb1>, dev=0)',
                      'rows(1, 8)',
                      "Dipole.accumulate_device('rows1+8', 120, 8, 30..59,90..119)",
                      'Dipole.result()',
                      'Dipole.close()',
                      'results.volumes([125312 125625 125938 126250 126562 126875 127188 127500])'],
 'dip-hbm64': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
               'to_host(0, 10)',
               'Dipole.accumulate(pos64[0..9 | 0..119])',
               'Dipole.result()',
               'Dipole.close()',
               'results.volumes(<(10,) #e82c6627dc>)'],
 'dip-memory': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
                'Dipole.accumulate(pos32[0..9 | 0..119])',
                'Dipole.result()',
                'Dipole.close()',
                'results.volumes(<(10,) #e82c6627dc>)'],
 'dip-memory-gather': ['Dipole(60x2, <(120,) #5e7d5d6bf0>, dev=0)',
                       'Dipole.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                       'Dipole.result()',
                       'Dipole.close()'],
 'dip-memory-rank1': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
                      'Dipole.accumulate(pos32[5..9 | 0..119])',
                      'Dipole.result()',
                      'Dipole.close()',
                      'results.volumes(<(10,) #e82c6627dc>)'],
 'dip-memory-unwrap': ['Dipole(120, <(120,) #fd59dbb533>, dev=0)',
                       'Dipole.set_unwrap([50 50 50], <(120, 3) #66606d5eaa>)',
                       'Dipole.accumulate(pos32[3..9 | 0..119])',
                       'Dipole.result()',
                       'Dipole.close()'],
 'dip-per-frame': ['Dipole(30x2, <(60,) #12b5303bb1>, dev=0)',
                   'Dipole.accumulate(pos32[0..9 | 30..59,90..119])',
                   'Dipole.result()',
                   'Dipole.close()',
                   'results.volumes(<(10,) #e82c6627dc>)'],
 'dip-per-frame-rank1': ['Dipole(60, <(60,) #e0bdd5f931>, dev=0)',
                         'Dipole.accumulate(pos32[5..9 | 30..89])',
                         'Dipole.result()',
                         'Dipole.close()',
                         'results.volumes(<(10,) #e82c6627dc>)'],
 'gyr-blocks': ['Gyration(2, 524288, <(1048576,) #01dfa447da>, dev=0)',
                'Gyration.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'Gyration.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'Gyration.result()',
                'Gyration.close()'],
 'gyr-file': ['Gyration(10, 12, <(120,) #2a35702bbc>, dev=0)',
              'Gyration.accumulate_traj(file, 0..5, None)',
              'Gyration.result()',
              'Gyration.close()'],
 'gyr-file-explicit-residues': ['Gyration(5, 4, <(20,) #08c8d5ab2e>, dev=0)',
                                'Gyration.set_grouping(0..60/3, <(60,) #b2c88767f2>)',
                                'Gyration.accumulate_traj(file, 0..9, 0..59)',
                                'Gyration.result()',
                                'Gyration.close()'],
 'gyr-file-subset': ['Gyration(3,2, 12x2, <(60,) #9848ddd21b>, dev=0)',
                     'Gyration.accumulate_traj(file, 2..9, 24..59,96..119)',
                     'Gyration.result()',
                     'Gyration.close()'],
 'gyr-hbm32': ['Gyration(10, 12, <(120,) #2a35702bbc>, dev=0)',
               'rows(0, 10)',
               "Gyration.accumulate_device('rows0+10', 120, 10, None)",
               'Gyration.result()',
               'Gyration.close()'],
 'gyr-hbm32-frames': ['Gyration(3,2, 12x2, <(60,) #9848ddd21b>, dev=0)',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(3, 1)',
                      'to_host(7, 1)',
                      'Gyration.accumulate(pos32[0,2..3,7 | 24..59,96..119])',
                      'Gyration.result()',
                      'Gyration.close()'],
 'gyr-hbm32-subset': ['Gyration(3,2, 12x2, <(60,) #9848ddd21b>, dev=0)',
                      'rows(1, 8)',
                      "Gyration.accumulate_device('rows1+8', 120, 8, 24..59,96..119)",
                      'Gyration.result()',
                      'Gyration.close()'],
 'gyr-hbm64': ['Gyration(10, 12, <(120,) #2a35702bbc>, dev=0)',
               'to_host(0, 10)',
               'Gyration.accumulate(pos64[0..9 | 0..119])',
               'Gyration.result()',
               'Gyration.close()'],
 'gyr-memory': ['Gyration(10, 12, <(120,) #2a35702bbc>, dev=0)',
                'Gyration.accumulate(pos32[0..9 | 0..119])',
                'Gyration.result()',
                'Gyration.close()'],
 'gyr-memory-gather': ['Gyration(5x2, 12x2, <(120,) #f985569a2d>, dev=0)',
                       'Gyration.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                       'Gyration.result()',
                       'Gyration.close()'],
 'gyr-memory-rank1': ['Gyration(10, 12, <(120,) #2a35702bbc>, dev=0)',
                      'Gyration.accumulate(pos32[5..9 | 0..119])',
                      'Gyration.result()',
                      'Gyration.close()'],
 'gyr-memory-residues-unwrap': ['Gyration(10, 4, <(40,) #94036cb298>, dev=0)',
                                'Gyration.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                                'Gyration.set_unwrap([50 50 50], <(40, 3) #fb5db8ad72>)',
                                'Gyration.accumulate(pos32[2..9 | 0..119])',
                                'Gyration.result()',
                                'Gyration.close()'],
 'gyr-per-frame': ['Gyration(3,2, 12x2, <(60,) #9848ddd21b>, dev=0)',
                   'Gyration.accumulate(pos32[0..9 | 24..59,96..119])',
                   'Gyration.result()',
                   'Gyration.close()'],
 'gyr-per-frame-rank1': ['Gyration(3, 12, <(36,) #17ac4c3d94>, dev=0)',
                         'Gyration.accumulate(pos32[5..9 | 24..59])',
                         'Gyration.result()',
                         'Gyration.close()'],
 'prof-blocks': ['Profile(1048576, 2, 4, [50 50 50], dev=0, per_frame=False)',
                 'Profile.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                 'Profile.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                 'Profile.counts()',
                 'Profile.close()'],
 'prof-file': ['Profile(120, 2, 4, [50 50 50], dev=0, per_frame=False)',
               'Profile.accumulate_traj(file, 0..5, None)',
               'Profile.counts()',
               'Profile.close()'],
 'prof-file-residues-recenter': ['Profile(40, 2, 4, [50 50 50], dev=0, per_frame=False)',
                                 'Profile.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                                 'Profile.set_recenter(0, <(40,) #94036cb298>, [25 25 25])',
                                 'Profile.accumulate_traj(file, 0..9, None)',
                                 'Profile.counts()',
                                 'Profile.close()'],
 'prof-file-subset': ['Profile(30x2, 2, 4, [50 50 50], dev=0, per_frame=False)',
                      'Profile.accumulate_traj(file, 2..9, 30..59,90..119)',
                      'Profile.counts()',
                      'Profile.close()'],
 'prof-hbm32': ['Profile(120, 2, 4, [50 50 50], dev=0, per_frame=False)',
                'rows(0, 10)',
                "Profile.accumulate_device('rows0+10', 120, 10, None)",
                'Profile.counts()',
                'Profile.close()'],
 'prof-hbm32-frames': ['Profile(30x2, 2, 4, [50 50 50], dev=0, per_frame=False)',
                       'to_host(0, 1)',
                       'to_host(2, 1)',
                       'to_host(3, 1)',
                       'to_host(7, 1)',
                       'Profile.accumulate(pos32[0,2..3,7 | 30..59,90..119])',
                       'Profile.counts()',
                       'Profile.close()'],
 'prof-hbm32-subset': ['Profile(30x2, 2, 4, [50 50 50], dev=0, per_frame=False)',
                       'rows(1, 8)',
                       "Profile.accumulate_device('rows1+8', 120, 8, 30..59,90..119)",
                       'Profile.counts()',
                       'Profile.close()'],
 'prof-hbm64': ['Profile(120, 2, 4, [50 50 50], dev=0, per_frame=False)',
                'to_host(0, 10)',
                'Profile.accumulate(pos64[0..9 | 0..119])',
                'Profile.counts()',
                'Profile.close()'],
 'prof-memory': ['Profile(120, 2, 4, [50 50 50], dev=0, per_frame=False)',
                 'Profile.accumulate(pos32[0..9 | 0..119])',
                 'Profile.counts()',
                 'Profile.close()'],
 'prof-memory-gather': ['Profile(60x2, 2, 4, [50 50 50], dev=0, per_frame=True)',
                        'Profile.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                        'Profile.counts()',
                        'Profile.close()'],
 'prof-memory-rank1': ['Profile(120, 2, 4, [50 50 50], dev=0, per_frame=True)',
                       'Profile.accumulate(pos32[5..9 | 0..119])',
                       'Profile.counts()',
                       'Profile.close()'],
 'prof-memory-residues': ['Profile(20,60, 2, 4, [50 50 50], dev=0, per_frame=False)',
                          'Profile.set_grouping(<81 ints #95475c9bc2>, <(120,) #7f4d5a97af>)',
                          'Profile.accumulate(pos32[0..9 | 60..119,0..59])',
                          'Profile.counts()',
                          'Profile.close()'],
 'prof-per-frame': ['Profile(30x2, 2, 4, [50 50 50], dev=0, per_frame=False)',
                    'Profile.accumulate(pos32[0..9 | 30..59,90..119])',
                    'Profile.counts()',
                    'Profile.close()'],
 'prof-per-frame-rank1': ['Profile(60, 2, 4, [50 50 50], dev=0, per_frame=False)',
                          'Profile.accumulate(pos32[5..9 | 30..89])',
                          'Profile.counts()',
                          'Profile.close()'],
 'prs-blocks': ['Residence(1048576, 1048576, 4, 0..1, [50 50 50], continuous=True, dev=0, max_neighbors=32, '
                'origin_step=1, same=True, zero_dims=0)',
                'Residence.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'Residence.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'Residence.result()',
                'Residence.contacts()',
                'Residence.close()'],
 'prs-file': ['Residence(120, 120, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
              'same=True, zero_dims=0)',
              'Residence.accumulate_traj(file, 0..5, None)',
              'Residence.result()',
              'Residence.contacts()',
              'Residence.close()'],
 'prs-file-subset': ['Residence(30, 30, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
                     'same=False, zero_dims=0)',
                     'Residence.accumulate_traj(file, 2..9, 30..59,90..119)',
                     'Residence.result()',
                     'Residence.contacts()',
                     'Residence.close()'],
 'prs-hbm32': ['Residence(120, 120, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
               'same=True, zero_dims=0)',
               'rows(0, 10)',
               "Residence.accumulate_device('rows0+10', 120, 10, None)",
               'Residence.result()',
               'Residence.contacts()',
               'Residence.close()'],
 'prs-hbm32-frames': ['Residence(30, 30, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
                      'same=False, zero_dims=0)',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(4, 1)',
                      'to_host(6, 1)',
                      'Residence.accumulate(pos32[0,2,4,6 | 30..59,90..119])',
                      'Residence.result()',
                      'Residence.contacts()',
                      'Residence.close()'],
 'prs-hbm32-subset': ['Residence(30, 30, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
                      'same=False, zero_dims=0)',
                      'rows(1, 8)',
                      "Residence.accumulate_device('rows1+8', 120, 8, 30..59,90..119)",
                      'Residence.result()',
                      'Residence.contacts()',
                      'Residence.close()'],
 'prs-hbm64': ['Residence(120, 120, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
               'same=True, zero_dims=0)',
               'to_host(0, 10)',
               'Residence.accumulate(pos64[0..9 | 0..119])',
               'Residence.result()',
               'Residence.contacts()',
               'Residence.close()'],
 'prs-memory': ['Residence(120, 120, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
                'same=True, zero_dims=0)',
                'Residence.accumulate(pos32[0..9 | 0..119])',
                'Residence.result()',
                'Residence.contacts()',
                'Residence.close()'],
 'prs-memory-gather': ['Residence(60, 60, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, '
                       'origin_step=1, same=False, zero_dims=0)',
                       'Residence.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                       'Residence.result()',
                       'Residence.contacts()',
                       'Residence.close()'],
 'prs-memory-lags-beyond': [],
 'prs-per-frame': ['Residence(30, 30, 4, 0..2, [50 50 50], continuous=True, dev=0, max_neighbors=32, origin_step=1, '
                   'same=False, zero_dims=0)',
                   'Residence.accumulate(pos32[0..9 | 30..59,90..119])',
                   'Residence.result()',
                   'Residence.contacts()',
                   'Residence.close()'],
 'rouse-blocks': ['Projection(2, 524288, (<(1, 524288) #e75350f232>), dev=0)',
                  'Projection.reserve(100)',
                  'Projection.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                  'Projection.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                  'Projection.device_result()',
                  'Msd(100, 1, 1, dev=0)',
                  "Msd.push_device(0, 'amplitudes', 2, 0, 2, 0)",
                  'Msd.result_acf()',
                  'Msd.close()',
                  'Projection.close()'],
 'rouse-file': ['Projection(10, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                'Projection.reserve(6)',
                'Projection.accumulate_traj(file, 0..5, None)',
                'Projection.device_result()',
                'Msd(6, 1, 2, dev=0)',
                "Msd.push_device(0, 'amplitudes', 20, 0, 10, 0)",
                "Msd.push_device(1, 'amplitudes', 20, 10, 10, 0)",
                'Msd.result_acf()',
                'Msd.close()',
                'Projection.close()'],
 'rouse-file-subset': ['Projection(3,2, 12x2, (<(2, 12) #2ea9fc7d31>, <(2, 12) #2ea9fc7d31>), dev=0)',
                       'Projection.reserve(8)',
                       'Projection.accumulate_traj(file, 2..9, 24..59,96..119)',
                       'Projection.device_result()',
                       'Msd(8, 1, 4, dev=0)',
                       "Msd.push_device(0, 'amplitudes', 10, 0, 3, 0)",
                       "Msd.push_device(1, 'amplitudes', 10, 3, 3, 0)",
                       "Msd.push_device(2, 'amplitudes', 10, 6, 2, 0)",
                       "Msd.push_device(3, 'amplitudes', 10, 8, 2, 0)",
                       'Msd.result_acf()',
                       'Msd.close()',
                       'Projection.close()'],
 'rouse-hbm32': ['Projection(10, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                 'Projection.reserve(10)',
                 'rows(0, 10)',
                 "Projection.accumulate_device('rows0+10', 120, 10, None)",
                 'Projection.device_result()',
                 'Msd(10, 1, 2, dev=0)',
                 "Msd.push_device(0, 'amplitudes', 20, 0, 10, 0)",
                 "Msd.push_device(1, 'amplitudes', 20, 10, 10, 0)",
                 'Msd.result_acf()',
                 'Msd.close()',
                 'Projection.close()'],
 'rouse-hbm32-frames': ['Projection(3,2, 12x2, (<(2, 12) #2ea9fc7d31>, <(2, 12) #2ea9fc7d31>), dev=0)',
                        'Projection.reserve(4)',
                        'to_host(0, 1)',
                        'to_host(2, 1)',
                        'to_host(3, 1)',
                        'to_host(7, 1)',
                        'Projection.accumulate(pos32[0,2..3,7 | 24..59,96..119])',
                        'Projection.device_result()',
                        'Msd(4, 1, 4, dev=0)',
                        "Msd.push_device(0, 'amplitudes', 10, 0, 3, 0)",
                        "Msd.push_device(1, 'amplitudes', 10, 3, 3, 0)",
                        "Msd.push_device(2, 'amplitudes', 10, 6, 2, 0)",
                        "Msd.push_device(3, 'amplitudes', 10, 8, 2, 0)",
                        'Msd.result_acf()',
                        'Msd.close()',
                        'Projection.close()'],
 'rouse-hbm32-subset': ['Projection(3,2, 12x2, (<(2, 12) #2ea9fc7d31>, <(2, 12) #2ea9fc7d31>), dev=0)',
                        'Projection.reserve(8)',
                        'rows(1, 8)',
                        "Projection.accumulate_device('rows1+8', 120, 8, 24..59,96..119)",
                        'Projection.device_result()',
                        'Msd(8, 1, 4, dev=0)',
                        "Msd.push_device(0, 'amplitudes', 10, 0, 3, 0)",
                        "Msd.push_device(1, 'amplitudes', 10, 3, 3, 0)",
                        "Msd.push_device(2, 'amplitudes', 10, 6, 2, 0)",
                        "Msd.push_device(3, 'amplitudes', 10, 8, 2, 0)",
                        'Msd.result_acf()',
                        'Msd.close()',
                        'Projection.close()'],
 'rouse-hbm64': ['Projection(10, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                 'Projection.reserve(10)',
                 'to_host(0, 10)',
                 'Projection.accumulate(pos64[0..9 | 0..119])',
                 'Projection.device_result()',
                 'Msd(10, 1, 2, dev=0)',
                 "Msd.push_device(0, 'amplitudes', 20, 0, 10, 0)",
                 "Msd.push_device(1, 'amplitudes', 20, 10, 10, 0)",
                 'Msd.result_acf()',
                 'Msd.close()',
                 'Projection.close()'],
 'rouse-memory': ['Projection(10, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                  'Projection.reserve(10)',
                  'Projection.accumulate(pos32[0..9 | 0..119])',
                  'Projection.device_result()',
                  'Msd(10, 1, 2, dev=0)',
                  "Msd.push_device(0, 'amplitudes', 20, 0, 10, 0)",
                  "Msd.push_device(1, 'amplitudes', 20, 10, 10, 0)",
                  'Msd.result_acf()',
                  'Msd.close()',
                  'Projection.close()'],
 'rouse-memory-gather': ['Projection(5x2, 12x2, (<(2, 12) #2ea9fc7d31>, <(2, 12) #2ea9fc7d31>), dev=0)',
                         'Projection.reserve(5)',
                         'Projection.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                         'Projection.device_result()',
                         'Msd(2, 2, 4, dev=0)',
                         "Msd.push_device(0, 'amplitudes', 20, 0, 5, 0)",
                         "Msd.push_device(1, 'amplitudes', 20, 5, 5, 0)",
                         "Msd.push_device(2, 'amplitudes', 20, 10, 5, 0)",
                         "Msd.push_device(3, 'amplitudes', 20, 15, 5, 0)",
                         'Msd.result_acf()',
                         'Msd.close()',
                         'Projection.close()'],
 'rouse-memory-no-fft': ['Projection(5, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                         'Projection.reserve(10)',
                         'Projection.accumulate(pos32[0..9 | 0..59])',
                         'Projection.result()',
                         'Projection.close()'],
 'rouse-memory-rank1': ['Projection(10, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                        'Projection.reserve(10)',
                        'Projection.accumulate(pos32[0..9 | 0..119])',
                        'Projection.device_result()',
                        'Msd(10, 1, 2, dev=0)',
                        "Msd.push_device(0, 'amplitudes', 20, 5, 5, 0)",
                        "Msd.push_device(1, 'amplitudes', 20, 15, 5, 0)",
                        'Msd.result_acf()',
                        'Msd.close()',
                        'Projection.close()'],
 'rouse-memory-residues-unwrap': ['Projection(10, 4, ([0.23097 0.0956709 -0.0956709 -0.23097 0.176777 -0.176777 '
                                  '-0.176777 0.176777]), dev=0)',
                                  'Projection.set_grouping(0..120/3, <(120,) #2a35702bbc>)',
                                  'Projection.set_unwrap([50 50 50], <(40, 3) #fb5db8ad72>)',
                                  'Projection.reserve(8)',
                                  'Projection.accumulate(pos32[2..9 | 0..119])',
                                  'Projection.device_result()',
                                  'Msd(8, 1, 2, dev=0)',
                                  "Msd.push_device(0, 'amplitudes', 20, 0, 10, 0)",
                                  "Msd.push_device(1, 'amplitudes', 20, 10, 10, 0)",
                                  'Msd.result_acf()',
                                  'Msd.close()',
                                  'Projection.close()'],
 'rouse-per-frame': ['Projection(3,2, 12x2, (<(2, 12) #2ea9fc7d31>, <(2, 12) #2ea9fc7d31>), dev=0)',
                     'Projection.reserve(10)',
                     'Projection.accumulate(pos32[0..9 | 24..59,96..119])',
                     'Projection.device_result()',
                     'Msd(10, 1, 4, dev=0)',
                     "Msd.push_device(0, 'amplitudes', 10, 0, 3, 0)",
                     "Msd.push_device(1, 'amplitudes', 10, 3, 3, 0)",
                     "Msd.push_device(2, 'amplitudes', 10, 6, 2, 0)",
                     "Msd.push_device(3, 'amplitudes', 10, 8, 2, 0)",
                     'Msd.result_acf()',
                     'Msd.close()',
                     'Projection.close()'],
 'rouse-per-frame-rank1': ['Projection(3, 12, (<(2, 12) #2ea9fc7d31>), dev=0)',
                           'Projection.reserve(10)',
                           'Projection.accumulate(pos32[0..9 | 24..59])',
                           'Projection.device_result()',
                           'Msd(10, 1, 2, dev=0)',
                           "Msd.push_device(0, 'amplitudes', 6, 2, 1, 0)",
                           "Msd.push_device(1, 'amplitudes', 6, 5, 1, 0)",
                           'Msd.result_acf()',
                           'Msd.close()',
                           'Projection.close()'],
 'vh-blocks': ['VanHove(1048576, [0 1.25 2.5 3.75 5], 0..1, dev=0, zero_dims=0)',
               'VanHove.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
               'VanHove.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
               'VanHove.result()',
               'VanHove.close()'],
 'vh-file': ['VanHove(120, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
             'VanHove.accumulate_traj(file, 0..5, None)',
             'VanHove.result()',
             'VanHove.close()'],
 'vh-file-subset': ['VanHove(60, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
                    'VanHove.accumulate_traj(file, 2..9, 30..89)',
                    'VanHove.result()',
                    'VanHove.close()'],
 'vh-hbm32': ['VanHove(120, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
              'rows(0, 10)',
              "VanHove.accumulate_device('rows0+10', 120, 10, None)",
              'VanHove.result()',
              'VanHove.close()'],
 'vh-hbm32-frames': ['VanHove(60, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
                     'to_host(0, 1)',
                     'to_host(2, 1)',
                     'to_host(4, 1)',
                     'to_host(6, 1)',
                     'VanHove.accumulate(pos32[0,2,4,6 | 30..89])',
                     'VanHove.result()',
                     'VanHove.close()'],
 'vh-hbm32-subset': ['VanHove(60, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
                     'rows(1, 8)',
                     "VanHove.accumulate_device('rows1+8', 120, 8, 30..89)",
                     'VanHove.result()',
                     'VanHove.close()'],
 'vh-hbm64': ['VanHove(120, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
              'to_host(0, 10)',
              'VanHove.accumulate(pos64[0..9 | 0..119])',
              'VanHove.result()',
              'VanHove.close()'],
 'vh-memory': ['VanHove(120, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
               'VanHove.accumulate(pos32[0..9 | 0..119])',
               'VanHove.result()',
               'VanHove.close()'],
 'vh-memory-gather': ['VanHove(60x2, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
                      'VanHove.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                      'VanHove.result()',
                      'VanHove.close()'],
 'vh-memory-lags-beyond': [],
 'vh-memory-unwrap-drop': ['VanHove(120, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=2)',
                           'VanHove.set_unwrap([50 50 50])',
                           'VanHove.accumulate(pos32[0..9 | 0..119])',
                           'VanHove.result()',
                           'VanHove.close()'],
 'vh-per-frame': ['VanHove(60, [0 1.25 2.5 3.75 5], 0..2, dev=0, zero_dims=0)',
                  'VanHove.accumulate(pos32[0..9 | 30..89])',
                  'VanHove.result()',
                  'VanHove.close()'],
 'vhd-blocks': ['DistinctVanHove(1048576, 1048576, [0 1.25 2.5 3.75 5], 0..1, [50 50 50], dev=0, origin_step=1, '
                'same=True, zero_dims=0)',
                'DistinctVanHove.accumulate(pos32<zero-stride (85, 1048576, 3)>)',
                'DistinctVanHove.accumulate(pos32<zero-stride (15, 1048576, 3)>)',
                'DistinctVanHove.result()',
                'DistinctVanHove.close()'],
 'vhd-file': ['DistinctVanHove(120, 120, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=True, '
              'zero_dims=0)',
              'DistinctVanHove.accumulate_traj(file, 0..5, None)',
              'DistinctVanHove.result()',
              'DistinctVanHove.close()'],
 'vhd-file-subset': ['DistinctVanHove(30, 30, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=False, '
                     'zero_dims=0)',
                     'DistinctVanHove.accumulate_traj(file, 2..9, 30..59,90..119)',
                     'DistinctVanHove.result()',
                     'DistinctVanHove.close()'],
 'vhd-hbm32': ['DistinctVanHove(120, 120, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=True, '
               'zero_dims=0)',
               'rows(0, 10)',
               "DistinctVanHove.accumulate_device('rows0+10', 120, 10, None)",
               'DistinctVanHove.result()',
               'DistinctVanHove.close()'],
 'vhd-hbm32-frames': ['DistinctVanHove(30, 30, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, '
                      'same=False, zero_dims=0)',
                      'to_host(0, 1)',
                      'to_host(2, 1)',
                      'to_host(4, 1)',
                      'to_host(6, 1)',
                      'DistinctVanHove.accumulate(pos32[0,2,4,6 | 30..59,90..119])',
                      'DistinctVanHove.result()',
                      'DistinctVanHove.close()'],
 'vhd-hbm32-subset': ['DistinctVanHove(30, 30, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, '
                      'same=False, zero_dims=0)',
                      'rows(1, 8)',
                      "DistinctVanHove.accumulate_device('rows1+8', 120, 8, 30..59,90..119)",
                      'DistinctVanHove.result()',
                      'DistinctVanHove.close()'],
 'vhd-hbm64': ['DistinctVanHove(120, 120, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=True, '
               'zero_dims=0)',
               'to_host(0, 10)',
               'DistinctVanHove.accumulate(pos64[0..9 | 0..119])',
               'DistinctVanHove.result()',
               'DistinctVanHove.close()'],
 'vhd-memory': ['DistinctVanHove(120, 120, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=True, '
                'zero_dims=0)',
                'DistinctVanHove.accumulate(pos32[0..9 | 0..119])',
                'DistinctVanHove.result()',
                'DistinctVanHove.close()'],
 'vhd-memory-gather': ['DistinctVanHove(60, 60, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, '
                       'same=False, zero_dims=0)',
                       'DistinctVanHove.accumulate(pos32[0,2,4,6,8 | 60..119,0..59])',
                       'DistinctVanHove.result()',
                       'DistinctVanHove.close()'],
 'vhd-memory-lags-beyond': [],
 'vhd-per-frame': ['DistinctVanHove(30, 30, [0 1.25 2.5 3.75 5], 0..2, [50 50 50], dev=0, origin_step=1, same=False, '
                   'zero_dims=0)',
                   'DistinctVanHove.accumulate(pos32[0..9 | 30..59,90..119])',
                   'DistinctVanHove.result()',
                   'DistinctVanHove.close()']})
