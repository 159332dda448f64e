"""
Shapes, pushes, walks, lags and environments of the MSD route tests: shared by ``test_msd_plan_host.py`` (which checks
on the CPU that every case plans to the pass-A and pass-B kernel, head, super groups, split and parts it names, and
that the reference of every case is sensitive to the push's last coordinate series) and ``test_gpu_msd_routes.py``
(which runs them).  The expectations are written out here; the plan query (``MsdEngine.plan``) confirms them.
"""

from collections import namedtuple

import numpy as np

from oracle import correlation as oc

SWITCHES = ("MDX_MSD_ROCFFT", "MDX_MSD_TWO_PASS")
OWN, ROCFFT, TWO_PASS = {}, {"MDX_MSD_ROCFFT": "1"}, {"MDX_MSD_TWO_PASS": "1"}
PASS_A = ("rocfft", "single400", "cols400_fused", "cols_small_fused", "cols")
PASS_B = ("none", "tiny", "short", "mid", "rows512", "rows1024", "general")
EPS = 2.0 ** -52
C_MAX = 4096.0
# the constant of the bound |got - ref| <= C[route] * unit (unit_of) per pass-A/pass-B route: 8 x the largest ratio
# observed by test_gpu_msd_routes.py on an MI355X (the table in its docstring), rounded up to a power of two
ROUTE_C = {"rocfft/none": 8.0, "single400/none": 8.0, "cols400_fused/tiny": 4.0, "cols400_fused/short": 8.0,
           "cols400_fused/mid": 4.0, "cols400_fused/rows512": 4.0, "cols400_fused/rows1024": 8.0,
           "cols_small_fused/mid": 8.0, "cols_small_fused/rows512": 4.0, "cols_small_fused/rows1024": 8.0,
           "cols/rows512": 8.0, "cols/rows1024": 8.0}
STEP = 0.3          # standard deviation of a walk's steps
BOX = 33.0

# T_b range -> (n_fft, r1, r2, pass A, pass B) without a switch: the 18 own lengths
LENGTHS = (
    (1, 200, 400, 400, 1, "single400", "none"),
    (201, 400, 800, 400, 2, "single400", "none"),
    (401, 800, 1600, 400, 4, "single400", "none"),
    (801, 1600, 3200, 400, 8, "cols400_fused", "short"),
    (1601, 3200, 6400, 400, 16, "cols400_fused", "short"),
    (3201, 4096, 1 << 13, 64, 128, "cols_small_fused", "mid"),
    (4097, 6400, 12800, 400, 32, "cols400_fused", "short"),
    (6401, 8192, 1 << 14, 64, 256, "cols_small_fused", "mid"),
    (8193, 12800, 25600, 400, 64, "cols400_fused", "short"),
    (12801, 16384, 1 << 15, 64, 512, "cols_small_fused", "rows512"),
    (16385, 25600, 51200, 400, 128, "cols400_fused", "mid"),
    (25601, 32768, 1 << 16, 64, 1024, "cols_small_fused", "rows1024"),
    (32769, 51200, 102400, 400, 256, "cols400_fused", "mid"),
    (51201, 102400, 204800, 400, 512, "cols400_fused", "rows512"),
    (102401, 131072, 1 << 18, 512, 512, "cols", "rows512"),
    (131073, 204800, 409600, 400, 1024, "cols400_fused", "rows1024"),
    (204801, 262144, 1 << 19, 1024, 512, "cols", "rows512"),
    (262145, 524288, 1 << 20, 1024, 1024, "cols", "rows1024"),
)

Push = namedtuple("Push", "group first count zero_dims")
# pushes: what the case feeds (push_device, or push_device_f32 when f32); seed / centre: its walk; want: the plan
# fields of pushes[0] that the case is about (beside the route and the head, which route_of and expected_head state
# for every case)
Case = namedtuple("Case", "name t_block n_blocks n_total pushes env f32 seed centre want")


def set_env(monkeypatch, env):
    """The stated environment of a case: both switches cleared, then those of ``env`` set."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def own_length(t_block):
    for lo, hi, n_fft, r1, r2, a, b in LENGTHS:
        if lo <= t_block <= hi:
            return n_fft, r1, r2, a, b
    raise ValueError(t_block)


def route_of(case):
    """(n_fft, r1, r2, pass A, pass B) the case must plan to in its environment."""
    if "MDX_MSD_ROCFFT" in case.env:
        return {1: 2, 60: 128, 65: 144}[case.t_block], 0, 0, "rocfft", "none"
    n_fft, r1, r2, a, b = own_length(case.t_block)
    if "MDX_MSD_TWO_PASS" in case.env and r2 in (2, 4):
        return n_fft, r1, r2, "cols400_fused", "tiny"
    return n_fft, r1, r2, a, b


def expected_head(c, push):
    """Coordinates by which pass A enters the push early: rows of whole 128-byte lines (16 | 3 n_total), and only the
    kernels with the 400-point first factor — the single-pass one included — do it."""
    _, r1, _, a, _ = route_of(c)
    return 3 * push.first % 16 if r1 == 400 and 3 * c.n_total % 16 == 0 else 0


def route_name(case):
    return "/".join(route_of(case)[3:])


def n_groups(case):
    return 1 + max(p.group for p in case.pushes)


# A walk whose last series happens to end where it began (an end-to-end displacement of a few per cent of its
# expectation, in any block) says little at lag T_b - 1 and fails the sensitivity check of test_msd_plan_host.py: those
# shapes draw another walk.  (group letter, T_b, n_blocks, n_total) -> seed.
RESEEDED = {("A", 25601, 2, 16): 100, ("A", 102401, 1, 16): 101, ("A", 204801, 1, 16): 101, ("B", 4097, 2, 46): 100,
            ("B", 12801, 1, 46): 100, ("B", 25601, 1, 89): 100, ("C", 801, 2, 32): 100, ("C", 4097, 2, 32): 102,
            ("D", 3, 2048, 20): 102, ("D", 3, 2049, 20): 102, ("D", 801, 9, 20): 100, ("D", 801, 10, 20): 100,
            ("D", 801, 11, 20): 100, ("D", 3201, 62, 4): 101, ("D", 3201, 63, 4): 101, ("D", 3201, 64, 4): 101}


def case(name, t_block, n_blocks, n_total, pushes, env=OWN, f32=False, seed=1, centre=0.0, **want):
    seed = RESEEDED.get((name[0], t_block, n_blocks, n_total), seed)
    return Case(name, t_block, n_blocks, n_total, tuple(Push(*p) for p in pushes), env, f32, seed, centre, want)


# ------------------------------------------------------------------------------------------------ walks and lags
_WALKS = {}


def positions(c):
    """float64[T, n_total, 3] of the case, read-only and shared between the cases of one shape and seed: in every
    block a walk of steps N(0, 0.3) that starts within a few steps (N(0, 1)) of ``centre``.  Cases that push float32
    get values a float32 holds exactly, so that both entry points see the same numbers."""
    key = (c.t_block, c.n_blocks, c.n_total, c.seed, c.centre, c.f32)
    if key not in _WALKS:
        rng = np.random.default_rng([c.seed, c.t_block, c.n_total])
        steps = rng.normal(0.0, STEP, (c.n_blocks, c.t_block, c.n_total, 3))
        steps[:, 0] = rng.normal(0.0, 1.0, (c.n_blocks, c.n_total, 3)) + c.centre
        pos = np.cumsum(steps, axis=1).reshape(c.n_blocks * c.t_block, c.n_total, 3)
        if c.f32:
            pos = pos.astype(np.float32).astype(np.float64)
        pos.setflags(write=False)
        _WALKS[key] = pos
    return _WALKS[key]


def forget_walks():
    _WALKS.clear()


def lags_of(t_block):
    """All lags of blocks of up to 1 600 frames; else the lags around the kernels' row and tile boundaries (199 .. 201:
    the live rows of the 400-point factor, 4095 .. 8192: the carries of the finishing kernel's tiles), both ends, the
    middle and 16 seeded random ones."""
    if t_block <= 1600:
        return np.arange(t_block)
    fixed = {0, 1, 2, 3, 199, 200, 201, 4095, 4096, 4097, 8191, 8192, t_block // 2, t_block - 2, t_block - 1}
    rng = np.random.default_rng(t_block)
    return np.array(sorted({m for m in fixed if 0 <= m < t_block} | set(rng.integers(0, t_block, 16).tolist())))


def unit_of(n_fft, t_block, energy, lags):
    """``unit[b, l] = 2^-52 (1 + log2 n_fft) E[b] / (T_b - m_l)``, the rounding scale of ``msd``; ``result_acf`` has the
    same without the window count."""
    scale = EPS * (1.0 + np.log2(n_fft)) * np.asarray(energy, dtype=np.float64)[:, None]
    return scale / (t_block - np.asarray(lags))[None, :], np.broadcast_to(scale, (len(energy), len(lags)))


def tables_of(c, lags, cache, particles=None):
    """``oracle.correlation.msd_series_tables`` of the case's walk at ``lags``, over the first ``particles`` particles
    (default: those any push of the case reaches); computed once per walk and lag set."""
    n = particles or max(p.first + p.count for p in c.pushes)
    key = (c.t_block, c.n_blocks, c.n_total, c.seed, c.centre, c.f32, n, tuple(int(m) for m in lags))
    if key not in cache:
        t = oc.msd_series_tables(positions(c)[:, :n], c.t_block, c.n_blocks, lags)
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        cache[key] = t
    return cache[key]


# ------------------------------------------------------------------------------------------------ A: every shape
A_PUSHES = ((0, 0, 11, 0), (1, 5, 6, 0))
A_TOTAL = 16
A_SHORTEST = (1, 200, 201, 401, 801, 1601, 3201, 4097, 6401, 8193, 12801, 16385, 25601, 32769, 51201, 102401, 131073,
              204801, 262145)
A_LONGEST = (400, 800, 1600, 3200, 4096, 6400, 8192, 12800)


def _a(t_block, env=OWN, tag=""):
    n_fft = own_length(t_block)[0]
    # (group 1 starts at particle 5 of 16: 15 coordinates into a 128-byte line)
    return case(f"A T_b={t_block}{tag}", t_block, 2 if n_fft <= (1 << 16) else 1, A_TOTAL, A_PUSHES, env, seed=3)


A_CASES = [_a(t) for t in A_SHORTEST + A_LONGEST]
A_TWO_PASS = [_a(t, TWO_PASS, " two-pass") for t in (201, 401)]
A_ROCFFT = [_a(t, ROCFFT, " rocFFT") for t in (1, 60, 65)]

# ------------------------------------------------------------------------------------------------ B: particle counts
B_SHAPES = (150, 201, 401, 801, 4097, 16385, 3201)        # one per pass-A kernel; 16385: pair groups in fours
B_COUNTS = (1, 5, 11, 16, 43, 86)
B_SMALL_SHAPES = (6401, 12801, 25601)                      # the other three 64 x R2 shapes: 43 and 86 particles
B_NONFUSED = (102401, (1, 5, 6))                           # 512 x 512


def _b(t_block, count):
    n_fft, r1, r2, a, _ = own_length(t_block)
    pmul = 8 * (512 // r2 if r2 in (128, 256) else 1)
    p_pad = -(-(-(-3 * count // 2)) // pmul) * pmul
    fused = a in ("cols400_fused", "cols_small_fused")
    # the array holds three particles more than the push, which starts at the third: no whole lines, head 0
    return case(f"B T_b={t_block} n={count}", t_block, 2 if t_block < 12000 else 1, count + 3, ((0, 2, count, 0),),
                seed=5, n_elem=3 * count, p_pad=p_pad, super_groups=-(-p_pad // 64) if fused else 0)


B_CASES = ([_b(t, n) for t in B_SHAPES for n in B_COUNTS] + [_b(t, n) for t in B_SMALL_SHAPES for n in (43, 86)]
           + [_b(B_NONFUSED[0], n) for n in B_NONFUSED[1]])

# ------------------------------------------------------------------------------------------------ C: head
C_TOTAL = 32
C_SHAPES = (150, 201, 401, 801, 4097)          # single<1>, <2>, <4>, 400 x 8, 400 x 32 (pair-group-major Y)
C_ZERO_DIMS = (0, 1, 2, 4, 6)
C_FIRSTS = tuple(range(16))                    # head = 3 first mod 16: every value 0 .. 15
C_CONTROL_TOTAL = 37                           # 111 coordinates per frame: no whole lines
C_CONTROL_SMALL = 3201                         # 64 x 128: this pass A never enters early


def c_cases(t_block, zero_dims):
    """Every head on one shape with one mask: the range to the array's last particle, and one particle.  The values
    are float32's, and the GPU test pushes them through both entry points."""
    out = []
    for first in C_FIRSTS:
        for count in (C_TOTAL - first, 1):
            out.append(case(f"C T_b={t_block} zero={zero_dims} first={first} n={count}", t_block, 2, C_TOTAL,
                            ((0, first, count, zero_dims),), f32=True, seed=7, n_elem=3 * count + 3 * first % 16))
    return out


def compact_of(c):
    """The same particles pushed from a compact copy of their own: the array is the selection, head 0."""
    p = c.pushes[0]
    return c._replace(name=c.name + " compact", n_total=p.count, pushes=(Push(p.group, 0, p.count, p.zero_dims),),
                      want={"n_elem": 3 * p.count})


C_CASES = [c for t in C_SHAPES for z in C_ZERO_DIMS for c in c_cases(t, z)]
# controls: the same pushes plan head 0 where the rows are no whole lines, and on the 64 x 128 shape whatever `first` is
C_CONTROLS = ([case(f"C control T_b={t} of 37 first={f}", t, 2, C_CONTROL_TOTAL, ((0, f, C_CONTROL_TOTAL - f, 2),),
                    f32=True, seed=7, n_elem=3 * (C_CONTROL_TOTAL - f)) for t in C_SHAPES for f in (5, 11)]
              + [case(f"C control T_b={C_CONTROL_SMALL} first={f}", C_CONTROL_SMALL, 2, C_TOTAL, ((0, f, C_TOTAL - f, 2),),
                      f32=True, seed=7, n_elem=3 * (C_TOTAL - f)) for f in (1, 7, 15)])

# ------------------------------------------------------------------------------------------------ D: block counts
D_SINGLE = [case(f"D single B={b}", 3, b, 20, ((0, 0, 20, 0),), seed=11, split=s, p_pad=32)
            for b, s in ((1, 4), (33, 4), (2048, 1), (2049, 1))]      # 64 and 63 wanted, 4 pair groups; then 1
D_ROWS400 = [case(f"D 400x8 B={b}", 801, b, 20, ((0, 0, 20, 0),), seed=11, rows_parts=parts)
             for b, parts in ((1, 5), (9, 5), (10, 1), (11, 1))]
D_ROWS64 = [case(f"D 64x128 B={b}", 3201, b, 4, ((0, 0, 4, 0),), seed=11, rows_parts=parts)
            for b, parts in ((1, 32), (62, 4), (63, 1), (64, 1))]
# (400 x blocks >= 4 096 and 64 x blocks >= 4 096 take one part outright — 11 and 64 blocks; below that slots_split takes
# the first factor that fills >= 97 % of four rounds of 512 block slots, which is 1 again at 10 and at 63 blocks: the
# last block counts with several parts are 9 and 62)
D_CASES = D_SINGLE + D_ROWS400 + D_ROWS64

# ------------------------------------------------------------------------------------------------ E, F, G, I
FAMILY_SHAPES = (150, 801, 3201, 102401)       # single pass, 400 x R2, 64 x R2, not fused
E_UNION = [case(f"E T_b={t}", t, 2 if t < 12000 else 1, 20, ((0, 0, 20, 5),), seed=13) for t in FAMILY_SHAPES]
F_CASES = [case(f"F T_b={t}", t, 2 if t < 12000 else 1, 9, ((0, 1, 7, 0),), seed=17, centre=40 * BOX)
           for t in FAMILY_SHAPES]
G_SHAPES = (150, 201, 401, 801, 4097, 3201)    # every family that reads float32 where it lies
G_CASES = [case(f"G T_b={t}", t, 2, C_TOTAL, ((0, 3, 20, 2),), f32=True, seed=19) for t in G_SHAPES]   # head 9
I_CASE = case("I T_b=801", 801, 2, 12, ((0, 2, 9, 0),), seed=23)

SENSITIVITY_CASES = A_CASES + A_TWO_PASS + A_ROCFFT + B_CASES + C_CASES + C_CONTROLS + D_CASES + G_CASES
ALL_CASES = SENSITIVITY_CASES + E_UNION + F_CASES + [I_CASE]
