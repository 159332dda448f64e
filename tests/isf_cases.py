"""
Wavevector sets, shapes and environments of the ISF route tests: shared by ``test_isf_plan_host.py`` (which checks on
the CPU that every set plans to the kernel it is meant for) and ``test_gpu_isf_routes.py`` (which runs them).
"""

from collections import namedtuple

import numpy as np

# the three kernel routes of csrc/mdx_isf.hip and the environment that selects each
ROUTES = ("general", "tables", "quads")
ENV = {"quads": {}, "tables": {"MDX_ISF_NO_QUADS": "1"}, "general": {"MDX_SQ_NO_LATTICE": "1"}}
SWITCHES = ("MDX_SQ_NO_LATTICE", "MDX_ISF_NO_QUADS")

LENGTHS = np.array([31.0, 29.5, 33.25])      # unequal box lengths: three different lattice bases

# q: float64[n_q, 3]; m_max: the largest |m| of a lattice set (0: off-lattice); route / stride: what the planner is
# meant to choose for it WITHOUT any switch (stride: row stride of the regular quad form, 0 otherwise)
WaveSet = namedtuple("WaveSet", "name q m_max route stride")


def set_env(monkeypatch, route_or_env):
    """The stated environment of a case: both switches cleared, then those of the route (or of a dict) set."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    env = ENV[route_or_env] if isinstance(route_or_env, str) else route_or_env
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def routes_of(ws):
    """The routes a set can take and the environment of each: its own by default, the ones below it by a switch."""
    default = ROUTES[ws.route]
    out = [(default, {})]
    if ws.route == 2:
        out.append(("tables", ENV["tables"]))
    if ws.route >= 1:
        out.append(("general", ENV["general"]))
    return out


def _from_m(m, lengths):
    return 2 * np.pi * np.asarray(m, dtype=np.float64) / np.asarray(lengths, dtype=np.float64)


def box_m(x, y, z):
    """Integer triples of a grid; an axis is a count n (m = 0 .. n - 1) or a (lo, hi) range (m = lo .. hi - 1)."""
    axes = [np.arange(*a) if isinstance(a, tuple) else np.arange(a) for a in (x, y, z)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)


def lattice_set(name, m, route, stride, lengths=LENGTHS):
    m = np.asarray(m)
    return WaveSet(name, _from_m(m, lengths), int(np.abs(m).max()), route, stride)


def random_set(name, n_q, seed, route=0, scale=2.5):
    """Off-lattice wavevectors: no common base per axis, so the lattice detection declines them."""
    rng = np.random.default_rng(seed)
    return WaveSet(name, rng.normal(0.0, scale, (n_q, 3)), 0, route, 0)


def _sphere(m, lengths, q_max):
    return m[np.linalg.norm(_from_m(m, lengths), axis=1) <= q_max]


def _ragged(m, seed, keep):
    return m[np.random.default_rng(seed).random(len(m)) < keep]


# ---- case B: wavevector-set shapes on the incoherent quads kernels.  The list of the S(q) sweep
# (test_sq_column_form_equals_lattice_and_general_kernels), with the sets that reach the remaining row strides
# chosen through the plan query: the planner takes the largest tile of {80, 64, 48, 32, 16} that fits 36 KB of
# tables of 3 R rows (R = the largest m + 1, rounded up to the 4 x 8 blocks) and is a multiple of the copies per item.
B_SETS = (
    lattice_set("octant 8^3", box_m(8, 8, 8), 2, 81),
    lattice_set("4^3 without q = 0", box_m(4, 4, 4)[1:], 2, 65),
    lattice_set("12 x 4 x 8 grid", box_m(12, 4, 8), 2, 49),
    lattice_set("q_max sphere of the 12^3 octant", _sphere(box_m(12, 12, 12), LENGTHS, 2.2), 2, 33),
    lattice_set("12^3 grid (three blocks)", box_m(12, 12, 12), 2, 33),
    lattice_set("2 x 8 x 24 grid", box_m(2, 8, 24), 2, 17),
    lattice_set("full 7^3 grid, m = -3 .. 3 (general items)", box_m((-3, 4), (-3, 4), (-3, 4)), 2, 0),
    lattice_set("10^3 grid (general items, rows padded)", box_m(10, 10, 10), 2, 0),
    lattice_set("5 x 9 x 17 grid (general items, unequal axes)", box_m(5, 9, 17), 2, 0),
    # the quad planner declines these (fewer than 60 % of the accumulators used): per-wavevector tables
    lattice_set("ragged columns of the 7^3 grid", _ragged(box_m((-3, 4), (-3, 4), (-3, 4)), 81, 0.6), 1, 0),
    lattice_set("sphere |q| < 0.5 of the 7^3 grid", _sphere(box_m((-3, 4), (-3, 4), (-3, 4)), LENGTHS, 0.4999), 1, 0),
    # no wavevector has m = 1, so the smallest component is not the base of its axis: the lattice detection
    # declines the set and it takes the general kernels without any switch
    lattice_set("grid from m = 2", box_m((2, 9), (2, 9), (2, 9)), 0, 0),
)
B_GROUPS = ((333, 130), (5, 1))
B_FRAMES, B_LAGS = 6, 4

# ---- case A: ring and chunk bookkeeping
A_SETS = (
    lattice_set("2^3 without q = 0", box_m(2, 2, 2)[1:], 1, 0, lengths=[33.0] * 3),     # 7 of 32 accumulators: tables
    random_set("7 off-lattice wavevectors", 7, 5),
    lattice_set("4^3 without q = 0 (cubic)", box_m(4, 4, 4)[1:], 2, 65, lengths=[33.0] * 3),   # the quads route
)
A_GROUPS, A_FRAMES = (5, 3), 23
A_LAGS = (1, 2, 5, 8, 30)
A_CUTS = (1, 1, 3, 7, 11)

# ---- case C: wavevector-count edges (one block of 512 wavevectors, one short of it, one over)
C_SETS = tuple(random_set(f"{n} off-lattice wavevectors", n, 100 + n, route=(1 if n == 1 else 0)) for n in (1, 511, 513))
C_GROUPS, C_FRAMES, C_LAGS = (70, 31), 5, 3

# ---- case D: particle splits with a ragged last part
SMALL_GRID = lattice_set("4^3 without q = 0 (cubic)", box_m(4, 4, 4)[1:], 2, 65, lengths=[33.0] * 3)
D_CASES = (          # name, groups, mode, rho parts the plan must report
    ("one group of 2049, total", (2049,), None, 2),
    ("one group of 4099, total", (4099,), None, 4),
    ("groups of 2049 and 700, partial", (2049, 700), "partial", 2),
)
D_FRAMES, D_LAGS = 7, 3

# ---- case F: large unwrapped coordinates
F_SET = lattice_set("grid up to m = 6", box_m(7, 7, 7), 2, 81, lengths=[33.0] * 3)

ALL_SETS = B_SETS + A_SETS + C_SETS + (SMALL_GRID, F_SET)


def pairs_of(n_groups, mode):
    """The reference's pair lists (structure.py:1459-1464)."""
    if mode == "partial":
        return tuple((j, k) for j in range(n_groups) for k in range(j, n_groups))
    if mode == "pair":
        return ((0, n_groups - 1),)
    return ((None, None),)
