"""
Wavevector sets, shapes and environments of the S(q) route tests: shared by ``test_sq_plan_host.py`` (which checks on
the CPU that every set plans to the kernel, row stride, block shape, split and slab it is meant for) and
``test_gpu_sq_routes.py`` (which runs them).  The sets were chosen with the plan query (``SqEngine.plan``).
"""

from collections import namedtuple

import numpy as np

import isf_cases as ic
from isf_cases import LENGTHS, SMALL_GRID, box_m, pairs_of  # noqa: F401
from oracle.fourier import grid_wavevectors

# the four density kernels of csrc/mdx_sq.hip in the normal mode, lowest first, and the environment that steps a
# lattice set down to each
ROUTES = ("general", "tables", "columns", "quads")
ENV = {"quads": {}, "columns": {"MDX_SQ_NO_QUADS": "1"}, "tables": {"MDX_SQ_NO_COLUMNS": "1"},
       "general": {"MDX_SQ_NO_LATTICE": "1"}}
SWITCHES = ("MDX_SQ_NO_LATTICE", "MDX_SQ_NO_COLUMNS", "MDX_SQ_NO_QUADS")
# single-chain mode: the plan's route 0 is sq_chain_sincos_kernel, 3 sq_chain_quads_kernel
CHAIN_ROUTES = {0: "chain-sincos", 3: "chain-quads"}

# q, m_max: as isf_cases.WaveSet; route / stride: what mdx_sq_create chooses WITHOUT any switch; lower: the routes
# below its own that the set can also take (a switch that finds the next form declined lands further down)
SqSet = namedtuple("SqSet", "name q m_max route stride lower")


def set_env(monkeypatch, env):
    """The stated environment of a case: the three switches cleared, then those of ``env`` (a route or a dict) set."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (ENV[env] if isinstance(env, str) else env).items():
        monkeypatch.setenv(name, value)


def routes_of(ws):
    """The routes a set can take and the environment of each: its own by default, those below it by a switch."""
    return [(ROUTES[ws.route], {})] + [(r, ENV[r]) for r in ws.lower]


def lattice_set(name, m, route, stride, lower, lengths=LENGTHS):
    m = np.asarray(m)
    return SqSet(name, ic._from_m(m, lengths), int(np.abs(m).max()), route, stride, tuple(lower))


def from_isf(ws, lower):
    """A set of the ISF cases: mdx_sq_create gives sq_quad_plan the arguments the ISF planner gives it, so the quad
    form and row stride are the same (test_sq_plan_host.py verifies that)."""
    return SqSet(ws.name, ws.q, ws.m_max, {2: 3, 0: 0}[ws.route], ws.stride, tuple(lower))


def random_set(name, n_q, seed, scale=2.5):
    """Off-lattice wavevectors: the general kernel without a switch.  ONE wavevector is always a lattice (m = 1 on
    every axis) that neither item builder takes: the tables by default, the general kernel by MDX_SQ_NO_LATTICE."""
    q = ic.random_set(name, n_q, seed, scale=scale).q
    return SqSet(name, q, 1, 1, 0, ("general",)) if n_q == 1 else SqSet(name, q, 0, 0, 0, ())


def _sparse(top, n, seed):
    """About n scattered triples of 0 .. top with m = 1 and m = top on every axis: no column holds four wavevectors
    and no quad block 60 % of its entries, so both item builders decline the set; sum R = 3 (top + 1)."""
    m = np.random.default_rng(seed).integers(0, top + 1, (n, 3))
    return np.unique(np.concatenate([m, [[1, 0, top], [0, top, 1], [top, 1, 0]]]), axis=0)


ALL_LOWER = ("columns", "tables", "general")
_B = {ws.name: ws for ws in ic.B_SETS}
_7 = box_m((-3, 4), (-3, 4), (-3, 4))

# ---- case A: wavevector-set shapes x routes
A_SETS = (
    # the six quad forms (isf_cases.B_SETS: regular strides 81, 65, 49, 33, 17 and general items)
    from_isf(_B["octant 8^3"], ALL_LOWER),
    # 63 wavevectors in 16 columns: one short of the columns builder's four per item, NO_QUADS lands on the tables
    from_isf(_B["4^3 without q = 0"], ("tables", "general")),
    from_isf(_B["12 x 4 x 8 grid"], ALL_LOWER),
    from_isf(_B["q_max sphere of the 12^3 octant"], ALL_LOWER),
    from_isf(_B["12^3 grid (three blocks)"], ALL_LOWER),
    from_isf(_B["2 x 8 x 24 grid"], ALL_LOWER),
    from_isf(_B["full 7^3 grid, m = -3 .. 3 (general items)"], ALL_LOWER),
    from_isf(_B["10^3 grid (general items, rows padded)"], ALL_LOWER),
    from_isf(_B["5 x 9 x 17 grid (general items, unequal axes)"], ALL_LOWER),
    # the quad planner declines these (fewer than 60 % of the accumulators used), sq_build_columns takes them: the
    # columns route by default — 43 items of at most 7 m_z (nz < 8) in a block of 64 threads, 225 in one of 256
    lattice_set("ragged columns of the 7^3 grid", ic._ragged(_7, 81, 0.6), 2, 0, ("tables", "general")),
    lattice_set("ragged columns of a 15 x 15 x 7 grid", ic._ragged(box_m((-7, 8), (-7, 8), (-3, 4)), 5, 0.6), 2, 0,
                ("tables", "general")),
    # both builders decline these: the tables route by default, with tiles of 64 particles and (sum R = 207) of 8
    lattice_set("sphere |q| < 0.5 of the 7^3 grid", ic._sphere(_7, LENGTHS, 0.4999), 1, 0, ("general",)),
    lattice_set("scattered triples up to m = 68", _sparse(68, 40, 3), 1, 0, ("general",)),
    # lattice-shaped sets the detector declines — no m = 1 on an axis; sum R = 210 > 208 (tables of fewer than 8
    # particles) — take the general kernel without any switch
    from_isf(_B["grid from m = 2"], ()),
    lattice_set("scattered triples up to m = 69", _sparse(69, 40, 3), 0, 0, ()),
)
A_GROUPS = ((333, 130), (5, 1))
A_FRAMES = 6

# ---- case B: wavevector-count edges of PAIR_Q = 64 (sq_pair_kernel) and SQ_QPB = 512 (the general and tables kernels)
B_SETS = tuple(random_set(f"{n} off-lattice wavevectors", n, 200 + n) for n in (1, 63, 64, 65, 511, 512, 513))
B_TABLES_SET = from_isf(_B["q_max sphere of the 12^3 octant"], ALL_LOWER)     # 828 wavevectors: two q-blocks of the tables
B_GROUPS, B_FRAMES = (70, 31), 5

# ---- case C: particle splits.  SMALL_GRID (63 wavevectors) cannot take the columns route — its 16 columns hold
# 63 < 4 x 16 wavevectors, sq_build_columns declines — so that route runs the same grid WITH q = 0 (64 wavevectors)
C_SET = from_isf(SMALL_GRID, ("tables", "general"))
C_COLUMNS_SET = lattice_set("4^3 grid (cubic)", box_m(4, 4, 4), 3, 65, ALL_LOWER, lengths=[33.0] * 3)
C_ROUTE_SETS = (("quads", C_SET), ("columns", C_COLUMNS_SET), ("tables", C_SET), ("general", C_SET))
C_CASES = (          # name, groups, mode, parts the plan must report, whether per = ceil(n / parts) leaves a remainder
    ("one group of 4096: 2 exact parts", (4096,), None, 2, False),
    ("one group of 4097: 2 parts, ragged", (4097,), None, 2, True),
    ("one group of 8195: 4 parts, the last shorter", (8195,), None, 4, True),
    ("groups of 4097, 3, 0 and 1", (4097, 3, 0, 1), "partial", 2, True),
)
C_FRAMES = 2

# ---- case D: slabs.  The 32^3 grid is also the quads set with ONE copy per item (n_sub = 1): the planner gives an
# item several copies unless the items fill whole blocks of 256, which takes about 8 000 wavevectors
D_FRAMES = 32771                      # the frame cap: 32 768 + 3
D_COLUMN = lattice_set("one column of 7 wavevectors", box_m(1, 1, 7), 2, 0, ("tables", "general"))
D_GROUPS = (2, 1)
D_BYTE_SET = SqSet("32^3 grid (the reference's default, meshgrid order)", grid_wavevectors([33.0] * 3, 32), 31, 3, 17,
                   ("general",))
D_BYTE_FRAMES, D_BYTE_SLAB = 1027, 1024
D_BYTE_CHECKED = np.unique(np.concatenate([[0, 1, 63, 64, 511, 512, 32767],
                                           np.random.default_rng(7).integers(0, 32768, 121)]))
D_CHAIN_POINTS, D_CHAIN_LENGTH = 4, 2
D_CHAIN_QUADS_SET = C_COLUMNS_SET

# ---- case E: single chains.  name, set, environment, chain route, regular stride.  Small sets: the reference of a
# case grows with chains x length x wavevectors, and the sincos kernel's tile is 1 024 particles
E_SIGNED = lattice_set("3 x 3 x 7 grid, m = -1 .. 1, -1 .. 1, -3 .. 3", box_m((-1, 2), (-1, 2), (-3, 4)), 3, 0, ALL_LOWER)
E_FORMS = (
    ("chain-quads regular", C_COLUMNS_SET, {}, 3, 81),
    ("chain-quads general items", E_SIGNED, {}, 3, 0),
    ("chain-sincos by switch", C_COLUMNS_SET, ENV["columns"], 0, 0),
    ("chain-sincos off-lattice", random_set("63 off-lattice wavevectors", 63, 263), {}, 0, 0),
)
E_TILES = {"chain-quads regular": 80, "chain-quads general items": 176}       # the planned table tiles
E_SINCOS_TILE = 1024                                                            # SQ_TILE, the sincos kernel's LDS stage
E_SPLITS = (         # name, chains, chain length, parts, chains per part
    ("3 chains of 1367", 3, 1367, 2, 2),
    ("8 chains of 1025", 8, 1025, 4, 2),
)
E_FRAMES = 2

# ---- case F: large coordinates
F_SET = lattice_set("grid up to m = 6", box_m(7, 7, 7), 3, 81, ALL_LOWER, lengths=[33.0] * 3)
F_RANDOM = random_set("65 off-lattice wavevectors", 65, 265, scale=3.0)

# ---- case H: a wavevector listed twice
_dup = np.concatenate([box_m(8, 8, 8), [[3, 2, 1]]])
H_TWICE = lattice_set("octant 8^3 with (3, 2, 1) twice", _dup, 3, 0, ALL_LOWER)
H_TWICE_AT = (int(np.flatnonzero((box_m(8, 8, 8) == [3, 2, 1]).all(axis=1))[0]), len(_dup) - 1)

NORMAL_SETS = A_SETS + B_SETS + (B_TABLES_SET, C_SET, C_COLUMNS_SET, D_COLUMN, D_BYTE_SET, E_SIGNED, F_SET, F_RANDOM,
                                 H_TWICE)


def walk(n_frames, n, length, seed, step=0.25, centre=None):
    """float32[F, n, 3]: a random walk, wrapped into the box, or unwrapped around ``centre``."""
    rng = np.random.default_rng(seed)
    steps = np.cumsum(rng.normal(0.0, step, (n_frames, n, 3)), axis=0)
    if centre is None:
        return np.mod(rng.uniform(0, length, (1, n, 3)) + steps, length).astype(np.float32)
    return (centre + rng.uniform(-length, length, (1, n, 3)) + steps).astype(np.float32)


def offsets_of(groups):
    return np.concatenate(([0], np.cumsum(groups))).astype(np.int64)
