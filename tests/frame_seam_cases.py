"""
Cases of the slab-seam tests of the per-frame engines: shared by ``test_frame_seams_host.py`` (which checks on the CPU
that every case crosses the seam it names, with the plan queries ``X.slab_frames`` / ``_core.feed_slab_frames``, and
that the walk carries unwrap state across it) and ``test_gpu_frame_seams.py`` (which runs them).  Plain data and NumPy.

Two loops cut a call: the engine's own (``slab_frames`` frames per kernel launch: 32 768, or fewer where the scratch of
a frame is large) and, on the host and file routes, the staging feed (``feed_slab_frames``: 64 MiB of coordinates).

  family 1  F = 32 768 + 3 frames of 24 points: the frame-count limit of the engine's loop, on the host route (one
            feed slab) and on the device route through an index.  Every variant as one call, and as a first call of
            FIRST frames followed by the long one, so that the seam falls at frames_seen != 0 on rows that were copied
            when the row buffer grew (the seam is then FIRST frames later in the walk).
  family 2  5 592 points with a grouping and the unwrap / recentring: the scratch limits the slab to ~1 300 frames;
            F = slab + 3.  Device route: on the host route the feed cuts such frames into slabs shorter than the
            engine's, so that the engine's loop would run once per feed slab.
  family 3  5 592 rows, 2 001 frames from host memory (134 MB) or a file: feed slabs of 1000 / 1000 / 1 frames, the
            third reusing the staging set of the first; the engine's own slab is longer, so every seam is the feed's.

The positions are chains of bonded points whose centres random-walk in an orthorhombic box, stored wrapped as float32;
the chains of the recentring group of the Profile cases also drift steadily.  ``check_crossings`` asserts that the
image count of a coordinate changes exactly at every seam, and that the recentring group's centre changes its cell
there.
"""

from collections import namedtuple
from functools import lru_cache

import numpy as np

from mdhelper_amd import _core

LIMIT = 32768               # what no engine exceeds per launch (grid y); asserted against the plans by the host test
FIRST = 100                 # frames of the short first call of family 1
F1 = LIMIT + 3
FEED_ROWS, FEED_FRAMES = 5592, 2001
MAX_INPUT_BYTES = 136 << 20
MIN_MARGIN = 1e-3           # no image decision may hang on a last bit: | |d| - L / 2 | stays above this

# name -> (frames, chains per group, points per chain, box, step of a chain's centre per frame, seed)
WALKS = {"small": (FIRST + F1, (2, 2), (5, 7), (12.0, 14.0, 16.0), 0.6, 11),
         "big": (FEED_FRAMES, (699,), (8,), (50.0, 55.0, 60.0), 2.5, 5)}
PROFILE_SIZES = {"small": (10, 14), "big": (8, FEED_ROWS - 8)}       # group 0 is the recentring group
PROFILE_BINS = {"small": (4, 5, 3), "big": (2, 3, 2)}
SMALL_FRAME_ROWS = 37       # the larger frame the index of family 1 gathers from
VH_SIZES, VH_LAGS = (70, FEED_ROWS - 70), (0, 1, 3, 999, 1001)
VH_EDGES = np.linspace(0.0, 400.0, 41)
DIP_SIZES = (129, FEED_ROWS - 129)

Case = namedtuple("Case", "name engine family walk lo hi calls route grouped unwrap whole recenter per_frame index "
                          "reserve")


def _case(name, engine, family, walk, lo, hi, calls, route, *, grouped=False, unwrap=False, whole=False,
          recenter=False, per_frame=False, index=False, reserve=False):
    return Case(name, engine, family, walk, lo, hi, tuple(calls), route, grouped, unwrap, whole, recenter, per_frame,
                index, reserve)


# ------------------------------------------------------------------------------------------------ plans

def layout(c):
    """(n_chains, n_monomers) of the chain engines of a case."""
    _, n_chains, n_monomers, *_ = WALKS[c.walk]
    return list(n_chains), list(n_monomers)


def n_points(c):
    n_chains, n_monomers = layout(c)
    return int(np.dot(n_chains, n_monomers))


def atoms_per_point(c):
    """Molecules of two atoms on the small walk; of one atom (a grouping that only costs scratch) on the big one."""
    return (2 if c.walk == "small" else 1) if c.grouped else 1


def fed_rows(c):
    """Rows of a frame as the engine is given it (the larger frame on the index route)."""
    return SMALL_FRAME_ROWS if c.index else n_points(c) * atoms_per_point(c)


def engine_slab(c):
    """The engine's own slab from the library's plan query; None for the engines that have none."""
    n_chains, n_monomers = layout(c)
    if c.engine == "prof":
        return _core.ProfileEngine.slab_frames(n_points(c), grouped=c.grouped, recenter=c.recenter)
    if c.engine == "gyr":
        return _core.GyrationEngine.slab_frames(n_chains, n_monomers, grouped=c.grouped, unwrap=c.unwrap)
    if c.engine == "rouse":
        return _core.ChainProjectionEngine.slab_frames(n_chains, n_monomers, grouped=c.grouped, unwrap=c.unwrap)
    if c.engine == "msid":
        return _core.InternalDistanceEngine.slab_frames(n_chains, n_monomers, grouped=c.grouped, whole=c.whole,
                                                        unwrap=c.unwrap)
    return None


def feed_slab(c, n_frames):
    """Frames per staged slab of a call of n_frames frames; None on the device route."""
    return None if c.route == "device" else _core.feed_slab_frames(n_frames, fed_rows(c))


def cuts(c):
    """Every frame (row of the result) at which a kernel launch of the case begins: the calls, the feed slabs of each
    and the engine's slabs of those."""
    out, slab = [], engine_slab(c)
    for a, b in zip(c.calls[:-1], c.calls[1:]):
        feed = feed_slab(c, b - a) or b - a
        for f0 in range(a, b, feed):
            f1 = min(b, f0 + feed)
            out.extend(range(f0, f1, slab or f1 - f0))
    return out


def seams(c):
    """The cuts inside a call: what the library does to a call, not what the caller did."""
    return [f for f in cuts(c) if f not in c.calls]


def input_bytes(c):
    return 12 * fed_rows(c) * max(b - a for a, b in zip(c.calls[:-1], c.calls[1:]))


def split_calls(c):
    """Cut points of the comparison run: device calls of at most half the smaller slab, which cross no seam."""
    F = c.calls[-1]
    slabs = [s for s in (engine_slab(c), feed_slab(c, F)) if s]
    step = min(slabs) // 2
    return list(range(0, F, step)) + [F]


def checked_frames(c):
    """The frames compared with the definition: both ends and three around every seam."""
    F = c.calls[-1]
    return sorted({0, F - 1} | {f for s in seams(c) for f in (s - 1, s, s + 1) if f < F})


# ------------------------------------------------------------------------------------------------ the cases

def _family1():
    out = []
    one, two = (0, F1, (0, F1)), (0, FIRST + F1, (0, FIRST, FIRST + F1))

    def both(name, engine, route="host", **kw):
        for tag, (lo, hi, calls) in (("one call", one), ("two calls", two)):
            out.append(_case(f"1 {engine} {name}, {tag}", engine, 1, "small", lo, hi, calls, route, **kw))

    for engine in ("gyr", "rouse", "msid"):
        both("plain", engine)
        both("unwrap", engine, unwrap=True)
        both("grouped unwrap", engine, grouped=True, unwrap=True, reserve=engine == "rouse")
        both("index unwrap", engine, "device", index=True, unwrap=True)
    both("plain reserve", "rouse", reserve=True)
    both("whole", "msid", whole=True)
    both("grouped whole", "msid", grouped=True, whole=True)
    both("plain totals", "prof")
    both("recenter rows", "prof", recenter=True, per_frame=True)
    both("recenter totals", "prof", recenter=True)
    both("grouped recenter rows", "prof", grouped=True, recenter=True, per_frame=True)
    both("grouped totals", "prof", grouped=True)
    both("index rows", "prof", "device", index=True, per_frame=True)
    return out


def _family2():
    out = []
    for engine, kw in (("gyr", dict(unwrap=True)), ("rouse", dict(unwrap=True)), ("msid", dict(unwrap=True)),
                       ("prof", dict(recenter=True, per_frame=True))):
        probe = _case("", engine, 2, "big", 0, 0, (0, 0), "device", grouped=True, **kw)
        F = engine_slab(probe) + 3
        out.append(probe._replace(name=f"2 {engine} scratch-bound", hi=F, calls=(0, F)))
    return out


def _family3():
    F = FEED_FRAMES
    return [_case("3 gyr unwrap", "gyr", 3, "big", 0, F, (0, F), "host", unwrap=True),
            _case("3 prof recenter totals", "prof", 3, "big", 0, F, (0, F), "host", recenter=True),
            _case("3 rouse", "rouse", 3, "big", 0, F, (0, F), "host"),
            _case("3 msid", "msid", 3, "big", 0, F, (0, F), "host"),
            _case("3 dip unwrap", "dip", 3, "big", 0, F, (0, F), "host", unwrap=True),
            _case("3 vh unwrap", "vh", 3, "big", 0, F, (0, F), "host", unwrap=True),
            _case("3 gyr unwrap file", "gyr", 3, "big", 0, F, (0, F), "file", unwrap=True)]


FAMILY1, FAMILY2, FAMILY3 = _family1(), _family2(), _family3()
ALL_CASES = FAMILY1 + FAMILY2 + FAMILY3


# ------------------------------------------------------------------------------------------------ the walks

def make_whole(points, n_chains, n_monomers, dims):
    """float64[n, 3] of one frame with every chain made whole bond after bond from its first point (minimum image)."""
    out, lo = np.array(points, dtype=np.float64), 0
    dims = np.asarray(dims, dtype=np.float64)
    for M, N in zip(n_chains, n_monomers):
        x = out[lo:lo + M * N].reshape(M, N, 3)
        for n in range(1, N):
            d = x[:, n] - x[:, n - 1]
            x[:, n] -= np.round(d / dims) * dims
        lo += M * N
    return out


def _recentre_drifts(true, masses, dims, seam_frames, speed):
    """One drift per axis (length per frame, about `speed`) for the recentring group, the first len(masses) points:
    with it the group's centre at frames seam - 1 and seam lies at equal distances on either side of a face of the
    box, for the seam of that axis.  The centre is the one the engine forms: mass-weighted, of the points unwrapped
    from frame 0, whose own image counts are 0 (the drift leaves frame 0 alone)."""
    drifts, group, w = np.zeros(3), len(masses), masses / masses.sum()
    for axis, s in enumerate(seam_frames):
        L = dims[axis]
        x0, xa, xb = (true[f, :group, axis] for f in (0, s - 1, s))
        cell0 = np.floor(x0 / L) * L
        mid = (((xa - cell0) * w).sum() + ((xb - cell0) * w).sum()) / 2
        k = np.ceil((mid + speed * (s - 0.5)) / L)
        drifts[axis] = (k * L - mid) / (s - 0.5)
    return drifts


def recentre_seams(walk):
    """Absolute frames of the walk at which a Profile case with recentring has a seam: at most one per axis."""
    found = []
    for c in ALL_CASES:
        if c.walk == walk and c.engine == "prof" and c.recenter:
            found.extend(c.lo + s for s in seams(c))
    return sorted(set(found))


@lru_cache(maxsize=1)
def walk(name):
    """(points float32[F, n, 3] wrapped into the box, dims float64[3])."""
    F, n_chains, n_monomers, dims, step, seed = WALKS[name]
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims)
    parts = []
    for M, N in zip(n_chains, n_monomers):
        bonds = rng.normal(size=(M, N, 3))
        bonds /= np.linalg.norm(bonds, axis=-1, keepdims=True)
        chain = rng.uniform(0.0, dims, (M, 1, 3)) + np.cumsum(bonds, axis=1)
        centre = np.cumsum(rng.normal(0.0, step, (F, M, 1, 3)), axis=0)
        wiggle = rng.standard_normal((F, M, N, 3), dtype=np.float32) * np.float32(0.05)
        parts.append((chain[None] + centre + wiggle).reshape(F, M * N, 3))
    true = np.concatenate(parts, axis=1)
    at = recentre_seams(name)
    assert len(at) <= 3, at
    g = PROFILE_SIZES[name][0]
    drifts = _recentre_drifts(true, _point_masses(true.shape[1])[:g], dims, at, step / 2)
    true[:, :g] += np.arange(F)[:, None, None] * drifts
    points = np.mod(true, dims).astype(np.float32)
    points.setflags(write=False)
    return points, dims


def forget_walks():
    walk.cache_clear()


def _point_masses(n):
    return np.random.default_rng(17).uniform(1.0, 20.0, n)


def point_masses(c):
    """float64 masses of the points: the same for every case of a walk, grouped or not."""
    return _point_masses(n_points(c))


def masses_of(c):
    """float64 masses of the fed atoms: the points' own, or each split 3 : 1 between the two atoms of a molecule."""
    m = point_masses(c)
    return m if atoms_per_point(c) == 1 else np.stack((0.75 * m, 0.25 * m), axis=1).ravel()


def grouping(c):
    """(CSR offsets, atom masses) of the grouping of a grouped case."""
    return atoms_per_point(c) * np.arange(n_points(c) + 1), masses_of(c)


def index_of(c):
    """The rows of the larger frame that hold the points, in incoming order."""
    return np.random.default_rng(23).permutation(SMALL_FRAME_ROWS)[:n_points(c)].astype(np.int32)


def rows(c):
    """float32[F, fed_rows, 3]: the frames the case feeds.  Ungrouped: the wrapped points; two-atom molecules: atoms at
    fixed offsets about the wrapped point, not wrapped themselves; index route: the points scattered over a larger
    frame of other particles."""
    points, dims = walk(c.walk)
    if c.grouped and atoms_per_point(c) == 2:
        # 3 : 1 masses at -1 : 3 offsets (multiples of 1 / 1024): the centre stays on the point up to rounding
        off = np.round(np.random.default_rng(29).uniform(-0.1, 0.1, (points.shape[1], 1, 3)) * 1024) / 1024
        off = (off * np.array([-1.0, 3.0])[None, :, None]).astype(np.float32)
        return (points[c.lo:c.hi, :, None, :] + off[None]).reshape(c.hi - c.lo, -1, 3)
    if c.index:
        frame = (np.random.default_rng(31).random((len(points), SMALL_FRAME_ROWS, 3)) * dims).astype(np.float32)
        frame[:, index_of(c)] = points
        return frame[c.lo:c.hi]
    return points[c.lo:c.hi]


def centres(r, c):
    """float64[F, n_points, 3]: the points the engine works on, from fed rows r (selected frames of ``rows(c)``): the
    mass-weighted centres of a grouping, summed in row order and divided once; else the rows themselves."""
    if c.index:
        r = r[:, index_of(c)]
    r = r.astype(np.float64)
    if not c.grouped:
        return r
    size = atoms_per_point(c)
    m = masses_of(c).reshape(-1, size)
    acc, tot = np.zeros((len(r), m.shape[0], 3)), np.zeros(m.shape[0])
    for a in range(size):
        acc = acc + m[None, :, a, None] * r[:, a::size]
        tot = tot + m[:, a]
    return acc / tot[None, :, None]


def start_of(c):
    """float64[n_points, 3]: the points of the first frame with every chain whole, the `start` of the unwrap."""
    _, dims = walk(c.walk)
    return make_whole(centres(rows(c)[:1], c)[0], *layout(c), dims)


# ------------------------------------------------------------------------------------------------ what the walk must do

def crossed_at(points, dims, f):
    """bool[n, 3]: the image count of the coordinate changes between frames f - 1 and f (float64 points)."""
    return np.abs(points[f] - points[f - 1]) >= np.asarray(dims) / 2


def check_crossings(c):
    """A lost d_prev / d_image, or a `first` flag raised again, must change the result: at every seam of the case at
    least one coordinate changes its image count exactly there, for Profile recentring the group's centre (of the
    points unwrapped from the first frame) changes its cell there, and no image decision is closer than MIN_MARGIN
    to its threshold anywhere.  Returns the number of coordinates that cross, per seam."""
    _, dims = walk(c.walk)
    r = rows(c)
    counts = []
    for s in seams(c):
        pts = centres(r[s - 1:s + 1], c)
        counts.append(int(crossed_at(pts, dims, 1).sum()))
        assert counts[-1] >= 1, (c.name, s)
    pts = centres(r, c) if c.grouped or c.index else r       # float32 differences widen exactly when taken in float64
    d = np.abs(pts[1:].astype(np.float64) - pts[:-1])
    assert np.abs(d - dims / 2).min() > MIN_MARGIN, c.name
    if c.engine == "prof" and c.recenter:
        g = PROFILE_SIZES[c.walk][0]
        x = pts[:, :g].astype(np.float64)
        step = np.diff(x, axis=0)
        images = np.concatenate((np.zeros((1, g, 3)), -np.cumsum(np.sign(step) * (np.abs(step) >= dims / 2), axis=0)))
        m = point_masses(c)[:g]
        com = ((x + images * dims) * m[None, :, None]).sum(axis=1) / m.sum()
        cell = np.floor(com / dims)
        for s in seams(c):
            assert np.any(cell[s] != cell[s - 1]), (c.name, s)
    return counts
