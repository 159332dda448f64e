"""
Cases of the slab-limit tests of the ten engines that derive from ``_SlabbedFrameEngine`` (dip, vh, chi4, vhd, prs, hb,
clu, ang, ori, boo): shared by ``test_slab_limits_host.py`` (which checks on the CPU, with ``engine.plan()`` and
``_core.feed_slab_frames``, that every case crosses the seam it names and that its input makes a lost seam state
visible) and ``test_gpu_slab_limits.py`` (which runs them).  Plain data and NumPy; an engine handle is created only to
ask it for its plan, which needs no device (the dipole engine acquires its stream in create: its plan is restated here
and pinned against the library by the GPU module).

  family 1  F1 = 32 768 + 3 frames of 37 rows (24 + 13 for the two-set engines, a dozen water molecules for hb): the
            frame-count limit of a launch.  As one call of F1 frames from host memory (one feed slab), and as FIRST
            frames followed by F1 frames from HBM through an index into a frame of 45 rows.  Lags (0, 1, 3, 40): in
            the two-call form the ring of 40 + 32 768 frames is shorter than the 32 871 frames fed, so it wraps
            inside the second call.
  family 2  the history-bound slab: device route, F = plan()["slab_frames"] + 3, lags (0, 1, 3, 999).  5 592 points
            for vh, chi4 and ori; 600 + 8 rows for prs, clu, ang and boo; 333 water molecules of which 10 accept for
            hb; 4 096 groups for dip, whose slab is bounded by its tiles; 8 190 + 2 rows and every third frame an
            origin for vhd, whose ring takes 12 B a row but whose reference takes a pair's time.
  family 3  PairResidence, 3 + 5 points, 3 x 32 768 + 3 frames: more than 65 535 origins meet the second and the third
            slab, so the walk of the survival sums takes a second batch; with every second frame an origin it does not.
  family 4  VanHove with every point at rest: the counters of one wave receive 64 lanes x 32 768 frames in a launch.

The rows are points that random-walk in an orthorhombic box, stored wrapped as float32.  A few rows are scripted
around every seam of a case (``script``): a pair in contact throughout, a pair whose contact breaks exactly at the
seam, a pair in contact in the seam frame only, and a point that crosses a face of the box exactly at the seam.
"""

from collections import namedtuple
from functools import lru_cache

import numpy as np

import hydrogen_bond_cases as hbc
from frame_seam_cases import F1, FIRST, LIMIT, MIN_MARGIN, crossed_at      # noqa: F401  (the tests use them from here)
from mdhelper_amd import _core

HISTORY_BYTES = 256 << 20       # what the frames of a default slab take at most, in every one of the ten engines
WALK_ORIGINS = 65535            # origins per launch of the survival walk (PRS_WALK_ORIGINS)
SPLIT_SLAB, SPLIT_CALL = 1024, 1000     # the comparison run: the small-slab regime the engines' own modules pin

N, N1, N2 = 37, 24, 13
FRAME_ROWS = 45                 # the larger frame the index of family 1 gathers from
DIMS = np.array([12.0, 14.0, 16.0])
CUTOFF = 3.0
REACH = 20                      # frames a scripted contact stays broken, or a scripted point stays across the face
LAGS1, LAGS2 = (0, 1, 3, 40), (0, 1, 3, 999)
SEAMS1 = (LIMIT, FIRST + LIMIT)         # of the one-call and of the two-call form, in frames of the walk
VH_REACH = {"small": 30.0, "big": 400.0, "rest": 30.0}      # the last edge of the van Hove bins
VHD_EDGES = np.linspace(0.0, 6.0, 61)
CHI4_CUTOFFS = (1.0, 4.0, 30.0)
ANG_THRESHOLDS = np.linspace(1.0, -1.0, 19)
BOO_EDGES = np.linspace(0.0, 1.0, 51)
BOO_DEGREES = (4, 6)
HB_MOLECULES, HB_BOX, HB_DISTANCE, HB_ANGLE = 12, np.array([8.0, 9.0, 10.0]), 3.5, 120.0

BIG_ROWS, BIG_GROUPS, BIG_DIMS = 5592, (70, 5522), np.array([50.0, 55.0, 60.0])
# the lists of 600 centres bound the slab of the list engines; 8 partners keep a reference of all frames affordable
MID_N1, MID_N2, MID_DIMS = 600, 8, np.array([18.0, 20.0, 22.0])
MID_HB_MOLECULES, MID_HB_BOX = 333, np.array([30.0, 32.0, 34.0])
MID_HB_ACCEPTORS = 10           # oxygens that accept: the lists take bytes per hydrogen, the reference time per pair
DIP_GROUPS = (1,) * 4095 + (129,)       # 4 097 tiles of 24 B a frame
# distinct van Hove: 12 B a row of either set in the ring, but n1 * n2 pairs: a small second set keeps the reference
# cheap
# every third frame an origin: of the three frames behind the seam one ends an origin pair of every lag
WIDE_N1, WIDE_N2, WIDE_DIMS, WIDE_STEP = 8190, 2, np.array([40.0, 44.0, 48.0]), 3

REST_GROUPS, REST_LAGS = (65, 2 * 64 + 3), (0, 1, 40)
BATCH_N1, BATCH_N2, BATCH_FRAMES, BATCH_DIMS = 3, 5, 3 * LIMIT + 3, np.array([7.0, 8.0, 9.0])

LAG_ENGINES = ("vh", "chi4", "vhd", "prs", "hb", "ori")
LIST_ENGINES = ("prs", "hb", "clu", "ang", "boo")
UNWRAPPED = ("dip", "vh", "chi4")
STEPPED = ("chi4", "vhd", "prs", "hb")          # the engines that take an origin_step
ENGINES = ("dip", "vh", "chi4", "vhd", "prs", "hb", "clu", "ang", "ori", "boo")

Case = namedtuple("Case", "name engine family walk calls route index lags origin_step continuous bins")


def _case(name, engine, family, walk, calls, route, *, index=False, lags=(), origin_step=1, continuous=True, bins=201):
    return Case(name, engine, family, walk, tuple(calls), route, index, tuple(lags), origin_step, continuous, bins)


# ------------------------------------------------------------------------------------------------ the engines

def sizes_of(c):
    """Rows of a frame as the engine works on it."""
    if c.walk == "small":
        return 3 * HB_MOLECULES if c.engine == "hb" else N
    if c.walk == "big":
        return BIG_ROWS
    if c.walk == "mid":
        return 3 * MID_HB_MOLECULES if c.engine == "hb" else MID_N1 + MID_N2
    if c.walk == "dip":
        return sum(DIP_GROUPS)
    if c.walk == "rest":
        return sum(REST_GROUPS)
    if c.walk == "wide":
        return WIDE_N1 + WIDE_N2
    return BATCH_N1 + BATCH_N2


def dims_of(c):
    if c.engine == "hb":
        return HB_BOX if c.walk == "small" else MID_HB_BOX
    return {"small": DIMS, "big": BIG_DIMS, "mid": MID_DIMS, "dip": BIG_DIMS, "rest": DIMS, "batch": BATCH_DIMS,
            "wide": WIDE_DIMS}[c.walk]


def groups_of(c):
    """The group sizes of dip, vh, chi4 and ori; (n1, n2) of the two-set engines."""
    if c.walk == "small":
        return (N1, N2)
    if c.walk == "big":
        return BIG_GROUPS
    if c.walk == "mid":
        return (MID_N1, MID_N2)
    if c.walk == "dip":
        return DIP_GROUPS
    if c.walk == "rest":
        return REST_GROUPS
    if c.walk == "wide":
        return (WIDE_N1, WIDE_N2)
    return (BATCH_N1, BATCH_N2)


def vh_edges(c):
    return np.linspace(0.0, VH_REACH[c.walk], c.bins + 1)


def dip_charges(n):
    return np.random.default_rng(37).uniform(-1.0, 1.0, n)


def ori_pairs(n_rows):
    """Vector v points from row v to the next row: as many vectors as rows."""
    tail = np.arange(n_rows, dtype=np.int32)
    return np.stack((tail, (tail + 1) % n_rows), axis=1)


def max_neighbors(c):
    """8 for the origin batches; 16 for the small bond-order case, whose slab then stays the 32 768 frames of a launch;
    else the engines' default of 32."""
    if c.walk == "batch":
        return 8
    return 16 if c.engine == "boo" and c.walk == "small" else 32


def hb_tables(c):
    """(h_row, d_row, a_row) of a hydrogen-bond case: every hydrogen with its oxygen; every oxygen accepts in the small
    water, the first MID_HB_ACCEPTORS (the scripted molecules among them) in the history-bound one."""
    h_row, d_row, a_row = hbc.water_tables(sizes_of(c) // 3)
    return h_row, d_row, a_row if c.walk == "small" else a_row[:MID_HB_ACCEPTORS]


def make_engine(c, start=None):
    """A fresh engine of the case; ``start``: the first frame's points, for the dipole unwrap.  Only the dipole engine
    touches a device here."""
    dims, g = dims_of(c), groups_of(c)
    if c.engine == "dip":
        eng = _core.DipoleEngine(g, dip_charges(sum(g)))
        if start is not None:
            eng.set_unwrap(dims, start)
        return eng
    if c.engine == "vh":
        eng = _core.VanHoveEngine(g, vh_edges(c), c.lags)
        eng.set_unwrap(dims)
        return eng
    if c.engine == "chi4":
        eng = _core.FourPointEngine(g, CHI4_CUTOFFS, c.lags, origin_step=c.origin_step)
        eng.set_unwrap(dims)
        return eng
    if c.engine == "vhd":
        return _core.DistinctVanHoveEngine(g[0], g[1], VHD_EDGES, c.lags, dims, origin_step=c.origin_step)
    if c.engine == "prs":
        return _core.PairResidenceEngine(g[0], g[1], CUTOFF, c.lags, dims, origin_step=c.origin_step,
                                         max_neighbors=max_neighbors(c), continuous=c.continuous)
    if c.engine == "hb":
        n_mol = sizes_of(c) // 3
        return _core.HydrogenBondEngine(3 * n_mol, *hb_tables(c), HB_DISTANCE, hbc.cos_of(HB_ANGLE), c.lags,
                                        dims, origin_step=c.origin_step, max_neighbors=max_neighbors(c),
                                        continuous=c.continuous)
    if c.engine == "clu":
        species = np.repeat([0, 1], g).astype(np.int32)
        return _core.ClusterEngine(species, [[0.0, CUTOFF], [CUTOFF, 0.0]], dims, max_neighbors=max_neighbors(c))
    if c.engine == "ang":
        return _core.AngleEngine(g[0], [g[1]], CUTOFF, ANG_THRESHOLDS, dims, max_neighbors=max_neighbors(c))
    if c.engine == "ori":
        n = sizes_of(c)
        eng = _core.OrientationEngine(g, ori_pairs(n), n, c.lags)
        eng.set_box(dims)
        return eng
    return _core.BondOrderEngine(g[0], g[1], CUTOFF, BOO_DEGREES, BOO_EDGES, dims, max_neighbors=max_neighbors(c))


def frame_bytes(c):
    """What a frame takes of the 256 MiB, by the accounting written next to each engine's X_slab (csrc/mdx_*.hip,
    mdx_residence_device.hpp): the formula the host test pins ``plan()`` against."""
    g, n, nb = groups_of(c), sizes_of(c), max_neighbors(c)
    if c.engine == "dip":
        return 24 * sum(-(-k // _core.DipoleEngine.TILE) for k in g)    # one partial sum of 3 doubles per tile
    if c.engine in ("vh", "ori"):
        return 24 * n                                   # 3 doubles per point or vector in the ring
    if c.engine == "chi4":
        # the ring, and a uint32 per counter in the scratch
        return 24 * n + 4 * len(c.lags) * len(g) * len(CHI4_CUTOFFS)
    if c.engine == "vhd":
        return 12 * n                                   # 3 floats per row in the ring
    if c.engine == "prs":                               # gathered rows, len + list words, a mask word per row
        return 12 * n + (nb + 1) * g[0] * 4 + 8 * g[0]
    if c.engine == "hb":
        n_h = 2 * (n // 3)
        return 12 * n + (nb + 1) * n_h * 4 + 8 * n_h
    if c.engine == "clu":                               # gathered rows, len + list words, a label and a size per row
        return 12 * n + (nb + 1) * n * 4 + 8 * n
    if c.engine == "ang":                               # gathered rows, len + list words of the centres
        return 12 * n + (nb + 1) * g[0] * 4
    # boo: gathered rows, len + list words, q_lm of every degree (2 (l_max + 1) doubles a centre), the values
    D, l_max = len(BOO_DEGREES), max(BOO_DEGREES)
    return 12 * n + (nb + 1) * g[0] * 4 + 8 * D * 2 * (l_max + 1) * g[0] + 8 * D * 1 * g[0]


def default_slab(c):
    """The formula of every X_slab: 32 768 frames, or what 256 MiB hold of frames of ``frame_bytes``."""
    return min(LIMIT, max(1, HISTORY_BYTES // frame_bytes(c)))


@lru_cache(maxsize=None)
def plan(c):
    """``plan()`` of a fresh engine of the case, before its first frame.  The dipole engine's create acquires a
    stream, so its plan is the formula here (pinned against the library on the GPU)."""
    if c.engine == "dip":
        return {"slab_frames": default_slab(c), "ring_frames": 0}
    eng = make_engine(c)
    try:
        return eng.plan()
    finally:
        eng.close()


def fed_rows(c):
    return FRAME_ROWS if c.index else sizes_of(c)


def feed_slab(c, n_frames):
    return None if c.route == "device" else _core.feed_slab_frames(n_frames, fed_rows(c))


def cuts(c):
    """Every frame at which a kernel launch of the case begins: the calls, the feed slabs of each and the engine's
    slabs of those."""
    out, slab = [], plan(c)["slab_frames"]
    for a, b in zip(c.calls[:-1], c.calls[1:]):
        feed = feed_slab(c, b - a) or b - a
        for f0 in range(a, b, feed):
            out.extend(range(f0, min(b, f0 + feed), slab))
    return out


def seams(c):
    """The cuts inside a call: what the library does to a call, not what the caller did."""
    return [f for f in cuts(c) if f not in c.calls]


def split_calls(c):
    F = c.calls[-1]
    return list(range(0, F, SPLIT_CALL)) + [F]


def checked_frames(c):
    F = c.calls[-1]
    return sorted({0, F - 1} | {f for s in seams(c) for f in (s - 1, s, s + 1) if f < F})


def input_bytes(c):
    return 12 * fed_rows(c) * max(b - a for a, b in zip(c.calls[:-1], c.calls[1:]))


def walk_batches(c, f_lo, nf):
    """The launches of ``SurvivalWalk::walk`` for the new frames [f_lo, f_lo + nf): (first origin number, origins) of
    each, origin number o being frame o * origin_step."""
    step, lag = c.origin_step, max(c.lags)
    o_lo, o_hi = -(-max(0, f_lo - lag) // step), -(-(f_lo + nf) // step)
    return [(o, min(WALK_ORIGINS, o_hi - o)) for o in range(o_lo, o_hi, WALK_ORIGINS)]


# ------------------------------------------------------------------------------------------------ the cases

def _family1():
    out = []
    for engine in ENGINES:
        for step in (1, 3) if engine in STEPPED else (1,):
            for continuous in (True, False) if engine in ("prs", "hb") else (True,):
                lags = LAGS1 if engine in LAG_ENGINES else ()
                tag = f"{engine} step {step}" + ("" if continuous else " intermittent")
                out.append(_case(f"1 {tag}, one call", engine, 1, "small", (0, F1), "host", lags=lags,
                                 origin_step=step, continuous=continuous))
                out.append(_case(f"1 {tag}, two calls", engine, 1, "small", (0, FIRST, FIRST + F1), "device",
                                 index=True, lags=lags, origin_step=step, continuous=continuous))
    return out


def _family2():
    out = []
    for engine, walk in (("vh", "big"), ("chi4", "big"), ("ori", "big"), ("vhd", "wide"), ("prs", "mid"), ("hb", "mid"),
                         ("clu", "mid"), ("ang", "mid"), ("boo", "mid"), ("dip", "dip")):
        probe = _case("", engine, 2, walk, (0, 0), "device", lags=LAGS2 if engine in LAG_ENGINES else (),
                      origin_step=WIDE_STEP if engine == "vhd" else 1)
        F = plan(probe)["slab_frames"] + 3
        out.append(probe._replace(name=f"2 {engine} history-bound", calls=(0, F)))
    return out


def _family3():
    F = BATCH_FRAMES
    # continuous: every origin's thread walks the frames up to its longest lag one after the other (once none of its
    # contacts is alive a frame costs it little, but the loop runs on); 0.8 s a pass on an MI355X, so the case is in
    return [_case("3 prs two batches", "prs", 3, "batch", (0, F), "device", lags=(0, 1, 40000), continuous=False),
            _case("3 prs one batch of every second frame", "prs", 3, "batch", (0, F), "device", lags=(0, 1, 65000),
                  origin_step=2, continuous=False),
            _case("3 prs two batches, continuous", "prs", 3, "batch", (0, F), "device", lags=(0, 1, 40000))]


def _family4():
    return [_case(f"4 vh at rest, {bins} bins", "vh", 4, "rest", (0, F1), "device", lags=REST_LAGS, bins=bins)
            for bins in (201, 5000)]


FAMILY1, FAMILY2, FAMILY3, FAMILY4 = _family1(), _family2(), _family3(), _family4()
ALL_CASES = FAMILY1 + FAMILY2 + FAMILY3 + FAMILY4


# ------------------------------------------------------------------------------------------------ the rows

def scripted_seams(c):
    """The frames the rows of the case's walk are scripted around: both forms of family 1 share one walk."""
    return SEAMS1 if c.family == 1 else tuple(seams(c))


def _wrap(true, dims):
    wrapped = (true - np.floor(true / dims) * dims).astype(np.float32)
    wrapped[wrapped >= dims.astype(np.float32)] = 0.0      # float32 rounding at the upper face
    return wrapped


def script(true, dims, at, first2):
    """Overwrites rows of the unwrapped float64 walk ``true [F, n, 3]`` around the frames ``at``; set 2 begins at row
    ``first2``.  Row first2 sits 1.0 from row 0 in every frame (a contact that never breaks); row first2 + 1 sits 1.0
    from row 1 but CUTOFF + 2.5 from it in the REACH frames from every seam on (broken exactly at the seam); row
    first2 + 2 sits 1.0 from row 2 in the seam frame alone; rows first2 + 3, + 4 and + 5 sit 1.0 from rows 3, 4 and 6
    in those REACH frames alone (so that the contacts of the seam frame are not as many as those of the frame before);
    the x of row 5 jumps across the face of the box at the seam and back REACH frames later."""
    F = len(true)
    f = np.arange(F)
    broken = np.zeros(F, dtype=bool)
    for s in at:
        broken |= (f >= s) & (f < s + REACH)
    only = np.isin(f, at)
    near, far = np.array([1.0, 0.0, 0.0]), np.array([CUTOFF + 2.5, 0.0, 0.0])
    true[:, first2] = true[:, 0] + near
    true[:, first2 + 1] = true[:, 1] + np.where(broken[:, None], far, near)
    true[:, first2 + 2] = true[:, 2] + np.where(only[:, None], near, far)
    for a, b in ((3, 3), (4, 4), (6, 5)):
        true[:, first2 + b] = true[:, a] + np.where(broken[:, None], near, far)
    true[:, 5, 0] = np.where(broken, 0.25, dims[0] - 0.25)
    return true


def script_batch(true, at):
    """The rows of the 3 + 5 points of family 3 around the frames ``at``: row 3 sits 1.0 from row 0 in every frame, row
    4 sits 1.0 from row 1 but 4.2 along z from it in the REACH frames from every seam on, row 5 sits 1.0 from row 2 in
    those REACH frames alone, row 6 sits 1.0 on the other side of row 2 in the seam frame alone; row 7 walks freely."""
    F = len(true)
    f = np.arange(F)
    broken = np.zeros(F, dtype=bool)
    for s in at:
        broken |= (f >= s) & (f < s + REACH)
    only = np.isin(f, at)
    near, far = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 4.2])
    true[:, 3] = true[:, 0] + near
    true[:, 4] = true[:, 1] + np.where(broken[:, None], far, near)
    true[:, 5] = true[:, 2] + np.where(broken[:, None], near, far)
    true[:, 6] = true[:, 2] + np.where(only[:, None], -near, -far)
    return true


@lru_cache(maxsize=2)
def _wide_walk(n_frames):
    """float32 [F, 8 192, 3]: the points of the history-bound distinct van Hove case, each in uniform motion (a walk
    of 67 million steps would take longer to make than the case to run), made 1 024 rows at a time."""
    rng = np.random.default_rng(17)
    points = np.empty((n_frames, WIDE_N1 + WIDE_N2, 3), dtype=np.float32)
    f = np.arange(n_frames, dtype=np.float64)[:, None, None]
    for lo in range(0, points.shape[1], 1024):
        start, velocity = rng.uniform(0.0, WIDE_DIMS, (1, 1024, 3)), rng.normal(0.0, 0.05, (1, 1024, 3))
        points[:, lo:lo + 1024] = _wrap(start + velocity * f, WIDE_DIMS)
    points.setflags(write=False)
    return points


@lru_cache(maxsize=2)
def _walk(name, at, n_frames):
    """float32 [F, n, 3] wrapped into the box: the points of a walk, scripted around the frames ``at``."""
    n, dims, first2, step, seed = {"small": (N, DIMS, N1, 0.3, 11), "big": (BIG_ROWS, BIG_DIMS, BIG_GROUPS[0], 1.5, 5),
                                   "mid": (MID_N1 + MID_N2, MID_DIMS, MID_N1, 0.3, 8),
                                   "dip": (sum(DIP_GROUPS), BIG_DIMS, 64, 1.5, 9),
                                   "batch": (BATCH_N1 + BATCH_N2, BATCH_DIMS, BATCH_N1, 0.3, 14)}[name]
    rng = np.random.default_rng(seed)
    steps = rng.standard_normal((n_frames, n, 3), dtype=np.float32) * np.float32(step)
    true = rng.uniform(0.0, dims, (1, n, 3)) + np.cumsum(steps, axis=0, dtype=np.float64)
    del steps
    true = script_batch(true, at) if name == "batch" else script(true, dims, at, first2)
    points = _wrap(true, dims)
    points.setflags(write=False)
    return points


def script_water(points, dims, at):
    """Overwrites the molecules 0 ... 9 of the wrapped float32 water ``points [F, 3 n_mol, 3]`` around the frames
    ``at``.  The first hydrogen of molecule a = 0, 2, 4, 6, 8 points along x, and the oxygen of molecule a + 1 sits
    2.8 along x from the oxygen of a (a bond: r_DA = 2.8, angle 180 degrees) or 4.2 along y (none).  Molecules 0 and 1
    are bonded in every frame; 2 and 3 in every frame but the REACH frames from every seam on; 4 and 5 in the seam
    frame alone; 6 and 7, and 8 and 9, in those REACH frames alone.  No other pair of atoms of a scripted pair of
    molecules is bonded."""
    F = len(points)
    f = np.arange(F)
    broken = np.zeros(F, dtype=bool)
    for s in at:
        broken |= (f >= s) & (f < s + REACH)
    only = np.isin(f, at)
    near, far = np.array([2.8, 0.0, 0.0]), np.array([0.0, 4.2, 0.0])
    true = points.astype(np.float64)
    for a, bonded in ((0, np.ones(F, dtype=bool)), (2, ~broken), (4, only), (6, broken), (8, broken)):
        Oa = true[:, 3 * a]
        Ob = Oa + np.where(bonded[:, None], near, far)
        true[:, 3 * a + 1], true[:, 3 * a + 2] = Oa + [0.96, 0.0, 0.0], Oa + [-0.3, 0.9, 0.0]
        true[:, 3 * a + 3], true[:, 3 * a + 4], true[:, 3 * a + 5] = Ob, Ob + [0.5, 0.8, 0.0], Ob + [0.5, -0.8, 0.0]
    return _wrap(true, dims)


@lru_cache(maxsize=2)
def _water(name, at, n_frames):
    n_mol, dims, seed = {"small": (HB_MOLECULES, HB_BOX, 1), "mid": (MID_HB_MOLECULES, MID_HB_BOX, 4)}[name]
    points = script_water(hbc.water(seed, n_frames, n_mol, dims, step=0.05, turn=0.05), dims, at)
    points.setflags(write=False)
    return points


def forget_walks():
    _walk.cache_clear()
    _wide_walk.cache_clear()
    _water.cache_clear()


def points(c):
    """float32 [frames of the walk, rows, 3]: the rows the engine works on, every frame of the case's walk (the case
    feeds the first ``c.calls[-1]`` of them)."""
    F = FIRST + F1 if c.family == 1 else c.calls[-1]
    if c.walk == "rest":
        frame = np.random.default_rng(19).uniform(0.0, DIMS, (1, sum(REST_GROUPS), 3)).astype(np.float32)
        return np.broadcast_to(frame, (F,) + frame.shape[1:])
    if c.engine == "hb":
        return _water(c.walk, scripted_seams(c), F)
    if c.walk == "wide":
        return _wide_walk(F)
    return _walk(c.walk, scripted_seams(c), F)


def index_of(c):
    return np.random.default_rng(23).permutation(FRAME_ROWS)[:sizes_of(c)].astype(np.int32)


def rows(c, whole=False):
    """float32 [F, fed rows, 3]: the frames the case feeds (``whole``: every frame of its walk); on the index route
    the points scattered over a larger frame of other particles."""
    p = points(c)
    if c.index:
        frame = (np.random.default_rng(31).random((len(p), FRAME_ROWS, 3)) * dims_of(c)).astype(np.float32)
        frame[:, index_of(c)] = p
        p = frame
    return p if whole else p[:c.calls[-1]]


# ------------------------------------------------------------------------------------------------ restatements

def min_image(d, dims):
    dims = np.asarray(dims, dtype=np.float64)
    return d - dims * np.rint(d * (1.0 / dims))


def square(w):
    return (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]


def unwrapped(pos, dims, start=None):
    """float64 [F, n, 3]: the reference's unwrap, every frame at once.  A coordinate's image count after frame f is
    minus the sum of sign(d) over the frames up to f with |d| >= dims / 2, d = x - x_prev of the raw points: integers,
    so the order of that sum does not matter.  ``start``: x_prev before the first frame (else the first frame is its
    own start).  Also returns the smallest | |d| - dims / 2 |."""
    x = np.asarray(pos).astype(np.float64)
    dims = np.asarray(dims, dtype=np.float64)
    first = x[:1] if start is None else np.asarray(start, dtype=np.float64)[None]
    d = np.diff(np.concatenate((first, x)), axis=0)
    images = -np.cumsum(np.sign(d) * (np.abs(d) >= dims / 2), axis=0)
    return x + images * dims, float(np.abs(np.abs(d) - dims / 2).min())


def survival(h, lags, origin_step):
    """The survival sums of bool ``h [F, rows, partners]``, vectorised over the origins: a loop over the lags only.
    ``gone[f]`` is the first frame from f on in which the pair is not in contact, so the contact of origin f0 is alive
    in every frame up to f0 + lag iff gone[f0] > f0 + lag."""
    F = len(h)
    frames = np.arange(F).reshape((F,) + (1,) * (h.ndim - 1))
    gone = np.where(h, F, frames)
    gone = np.minimum.accumulate(gone[::-1], axis=0)[::-1]
    out = {key: np.zeros(len(lags), dtype=np.int64) for key in ("intermittent", "continuous", "origin_counts")}
    for k, lag in enumerate(lags):
        if lag >= F:
            continue
        o = slice(0, F - lag, origin_step)
        later = slice(lag, F, origin_step)
        out["origin_counts"][k] = h[o].sum()
        out["intermittent"][k] = (h[o] & h[later]).sum()
        out["continuous"][k] = (gone[o] > frames[o] + lag).sum()
    return out


def contact_matrix(pos, n1, dims, cutoff=CUTOFF, chunk=4096):
    """bool [F, n1, n2] of float32 pos [F, n1 + n2, 3]: ``test_gpu_residence.contact_matrix`` for every frame."""
    out = np.empty((len(pos), n1, pos.shape[1] - n1), dtype=bool)
    for lo in range(0, len(pos), chunk):
        x = pos[lo:lo + chunk].astype(np.float64)
        w = min_image(x[:, None, n1:] - x[:, :n1, None], dims)
        out[lo:lo + chunk] = square(w) <= np.float64(cutoff) * np.float64(cutoff)
    return out


def bond_matrix(pos, dims, chunk=4096, acceptors=None):
    """bool [F, n_h, n_a] of the water of ``hydrogen_bond_cases``: its ``frame_geometry`` and bond rule for every
    frame; ``acceptors``: the first oxygens alone accept."""
    n_mol = pos.shape[1] // 3
    h_row, d_row, a_row = hbc.water_tables(n_mol)
    a_row = a_row[:acceptors]
    own = a_row[None, :] == d_row[:, None]
    rc2, cos_max = np.float64(HB_DISTANCE) * np.float64(HB_DISTANCE), np.float64(hbc.cos_of(HB_ANGLE))
    out = np.empty((len(pos), len(h_row), len(a_row)), dtype=bool)
    for lo in range(0, len(pos), chunk):
        x = pos[lo:lo + chunk].astype(np.float64)
        H, D, A = x[:, h_row], x[:, d_row], x[:, a_row]
        r2 = square(min_image(A[:, None] - D[:, :, None], dims))
        hd = min_image(D - H, dims)[:, :, None]
        ha = min_image(A[:, None] - H[:, :, None], dims)
        dot = (hd[..., 0] * ha[..., 0] + hd[..., 1] * ha[..., 1]) + hd[..., 2] * ha[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = dot / np.sqrt(square(hd) * square(ha))
            out[lo:lo + chunk] = (r2 <= rc2) & ~own & (cos <= cos_max)
    return out


def restate_vh(pos, sizes, edges, lags, dims):
    """``test_gpu_vanhove.restate`` with a loop over the lags only: (counts, moments, accumulators, evaluations).  An
    accumulator takes its terms in frame order: ``numpy.cumsum`` along the frames adds them one after the other."""
    x, margin = unwrapped(pos, dims)
    assert margin > MIN_MARGIN
    F, n = x.shape[:2]
    n_bins = len(edges) - 1
    acc = np.zeros((len(lags), n, 2))
    counts = np.zeros((len(lags), len(sizes), n_bins), dtype=np.int64)
    evaluations = 0
    offs = np.concatenate(([0], np.cumsum(sizes)))
    for k, lag in enumerate(lags):
        if lag >= F:
            continue
        r2 = square(x[lag:] - x[:F - lag])
        acc[k, :, 0] = np.cumsum(r2, axis=0)[-1]
        acc[k, :, 1] = np.cumsum(r2 * r2, axis=0)[-1]
        evaluations += n * (F - lag)
        r = np.sqrt(r2)
        for g, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
            counts[k, g] = np.histogram(r[:, a:b], n_bins, (edges[0], edges[-1]))[0]
    moments = np.zeros((len(lags), len(sizes), 2))
    for g, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        s = np.zeros((len(lags), 2))
        for p in range(a, b):                           # a group's points in row order
            s = s + acc[:, p, :]
        moments[:, g] = s
    return counts, moments, acc, evaluations


def restate_chi4(pos, sizes, cutoffs, lags, dims, origin_step):
    """``test_gpu_four_point.restate`` with a loop over the lags only: all integers."""
    x, margin = unwrapped(pos, dims)
    assert margin > MIN_MARGIN
    F, n = x.shape[:2]
    a2 = np.asarray(cutoffs, dtype=np.float64) * np.asarray(cutoffs, dtype=np.float64)
    shape = (len(lags), len(sizes), len(a2))
    s1, s2 = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    origins = np.zeros(len(lags), dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(sizes)))
    for k, lag in enumerate(lags):
        if lag >= F:
            continue
        r2 = square(x[lag::origin_step][:len(range(0, F - lag, origin_step))] - x[0:F - lag:origin_step])
        origins[k] = len(r2)
        for g, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
            q = (r2[:, a:b, None] <= a2).sum(axis=1).astype(np.int64)
            s1[k, g], s2[k, g] = q.sum(axis=0), (q * q).sum(axis=0)
    return s1, s2, origins, n * int(origins.sum())


def restate_vhd(pos, n1, edges, lags, dims, origin_step, chunk=4096):
    """``test_gpu_vanhove_distinct.restate`` with a loop over the lags and chunks of origins."""
    x = np.asarray(pos)
    F, n2 = len(x), x.shape[1] - n1
    n_bins = len(edges) - 1
    counts = np.zeros((len(lags), n_bins), dtype=np.int64)
    n_origins = np.zeros(len(lags), dtype=np.int64)
    for k, lag in enumerate(lags):
        o = np.arange(0, max(F - lag, 0), origin_step)
        n_origins[k] = len(o)
        for lo in range(0, len(o), chunk):
            f0 = o[lo:lo + chunk]
            a, b = x[f0, :n1].astype(np.float64), x[f0 + lag, n1:].astype(np.float64)
            r = np.sqrt(square(min_image(b[:, None] - a[:, :, None], dims)))
            counts[k] += np.histogram(r, n_bins, (edges[0], edges[-1]))[0]
    return counts, n_origins, int(n_origins.sum()) * n1 * n2


def restate_ori(pos, sizes, pairs, lags, dims, tori):
    """``test_gpu_orientation.restate`` (module ``tori``) with a loop over the lags only: (vector accumulators,
    frame sums of every group, evaluations)."""
    u = tori.unit_vectors(pos, pairs, dims=dims)
    F, V = u.shape[:2]
    acc = np.zeros((len(lags), V, 2))
    evaluations = 0
    for k, lag in enumerate(lags):
        if lag >= F:
            continue
        a, b = u[lag:], u[:F - lag]
        c = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        acc[k, :, 0] = np.cumsum(c, axis=0)[-1]
        acc[k, :, 1] = np.cumsum((1.5 * (c * c)) - 0.5, axis=0)[-1]
        evaluations += V * (F - lag)
    frame_sums = np.zeros((F, len(sizes), 6))
    lo = 0
    for g, size in enumerate(sizes):
        total = np.zeros((F, 6))
        for t0 in range(lo, lo + size, tori.T):         # its tiles in tile order
            partial = np.zeros((F, 6))
            for v in range(t0, min(t0 + tori.T, lo + size)):        # a tile's vectors in row order
                partial = partial + np.stack([u[:, v, a] * u[:, v, b] for a, b in tori.PRODUCTS], axis=1)
            total = total + partial
        frame_sums[:, g] = total
        lo += size
    return acc, frame_sums, evaluations


def restate_ang(pos, n0, thresholds, dims, cutoff=CUTOFF, chunk=2048):
    """The counts [n_bins] and the degenerate triplets of ``test_gpu_angle.restate`` for one ligand group, every frame
    and centre at once: the cosine of every pair a < b of ligands, kept where both are neighbours of the centre."""
    t = np.asarray(thresholds, dtype=np.float64)
    counts, degenerate = np.zeros(len(t) - 1, dtype=np.int64), 0
    a, b = np.triu_indices(pos.shape[1] - n0, 1)
    for lo in range(0, len(pos), chunk):
        x = pos[lo:lo + chunk].astype(np.float64)
        w = min_image(x[:, None, n0:] - x[:, :n0, None], dims)
        r2 = square(w)
        near = r2 <= np.float64(cutoff) * np.float64(cutoff)
        both = near[..., a] & near[..., b]
        f, i, p = np.nonzero(both)
        wa, wb = w[f, i, a[p]], w[f, i, b[p]]
        dot = (wa[:, 0] * wb[:, 0] + wa[:, 1] * wb[:, 1]) + wa[:, 2] * wb[:, 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            cosine = dot / np.sqrt(r2[f, i, a[p]] * r2[f, i, b[p]])
        nan = np.isnan(cosine)
        degenerate += int(nan.sum())
        counts += np.bincount(np.searchsorted(-t[1:-1], -cosine[~nan], side="right"), minlength=len(t) - 1)
    return counts, degenerate


def seam_origins(c, s, lag):
    """The origins f0 (multiples of origin_step) whose frame pair (f0, f0 + lag) of the case reaches across the seam
    s: f0 < s <= f0 + lag < F; for lag 0 the origins behind the seam, s <= f0 < F."""
    F = c.calls[-1]
    lo, hi = (s, F) if lag == 0 else (max(0, s - lag), min(s, F - lag))
    return [f0 for f0 in range(-(-lo // c.origin_step) * c.origin_step, hi, c.origin_step)]
