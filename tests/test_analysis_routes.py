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
from mdhelper_amd import _core
from mdhelper_amd.analysis import (EndToEndVector, IntermediateScatteringFunction, Onsager,
                                   RadialDistributionFunction, SingleChainStructureFactor, StructureFactor)

F, N, L = 10, 120, 50.0
BIG_N = 1 << 20          # particles of the zero-stride trajectories whose frames split into several blocks

_trace = []
_tokens = [0]


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
    monkeypatch.setattr(_core, "DeviceArray", DeviceArrayRecorder)
    monkeypatch.setattr(_core, "device_info", lambda dev=0: _record("device_info") or {"hbm_available_bytes": 1 << 40})
    monkeypatch.setattr(_core, "synchronize", lambda dev=0: _record("synchronize"))
    monkeypatch.setattr(_core, "correlate_device", _correlate)
    monkeypatch.setattr(mdhelper_amd.io.TrajectoryFile, "load_device",
                        lambda self, frames, d_out, dev=0, **kw: _record("file.load_device", (frames, d_out)))
    _trace.clear()
    _tokens[0] = 0


@pytest.fixture(autouse=True)
def recorders(monkeypatch):
    install_recorders(monkeypatch)
    yield
    _trace.clear()


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


BIG_FRAMES = {"rdf": 400, "sq": 100, "isf": 100, "scsf": 100, "e2e": 50}


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
