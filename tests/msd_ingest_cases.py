"""
Inputs and the definition for the tests of the MSD frame preparation (csrc/mdx_msd.hip: the segment-parallel unwrap,
the frame and molecule centres of mass, the three frame sources and the chunk / cut / frame-block bookkeeping of
``msd_push_frames`` and ``msd_system_com_frames``): shared by ``test_msd_ingest_host.py`` (CPU) and
``test_gpu_msd_ingest.py``.  Needs no GPU and no torch.

Lattice.  The box is L = (12.5, 16.0, 9.75) and every coordinate is an integer number of q = 2^-30; one lattice UNIT is
1/64 = 2^24 q.  float32 cases keep wrapped coordinates on whole units in [0, L); float64 cases add a per-particle
offset below one unit that is a multiple of q, so a path that narrowed to float32 would be off by many units.  Box
lengths, shifts, image flags and dyadic masses are integers as well, and every operation of the definition (difference,
comparison with L/2, image * L, sum, shift, floor(x / L) * L, division by a power of two) is exact in float64: any
summation order gives the same bits, and the tests compare with ``assert_array_equal``.

The reference is the definition in int64 (``unwrap_ref``, ``wrap_ref``, ``centre_ref``, ``molecule_centres_ref``):
d = x - x_old; 2 |d| >= L -> image -= sign(d); x_old = x; out = x + image L; then - shift; then wrap (x -= floor(x / L) L
only where x < 0 or x > L); then centres sum m x / sum m as exact rationals (``fractions``) or integers over a power-of-
two denominator.  ``test_msd_ingest_host.py`` shows that it equals ``algorithm.topology.unwrap`` / ``wrap`` and
``algorithm.molecule.center_of_mass`` in float64 bit for bit on every case's inputs.

Planted events.  ``lattice_walk`` scripts a few rows (``ROLES``) and fills the others with random walkers;
``events_of`` FINDS the events in any walk, and ``assert_claims`` checks that a case holds every event it claims.
"""

from collections import namedtuple
from fractions import Fraction

import numpy as np

Q_BITS = 30
UNIT = 1 << 24                                   # one lattice unit (1/64) in q = 2^-30
L_UNITS = np.array([800, 1024, 624], dtype=np.int64)          # L = (12.5, 16.0, 9.75) in units: all even
LQ = L_UNITS * UNIT                              # box lengths in q
BOX = L_UNITS / 64.0                             # float64 box lengths
SEG = 128                                        # UNWRAP_SEG of csrc/mdx_msd.hip
STAGE_DEFAULT = 64 << 20                         # bytes of staged frames per unwrap launch without the hook
HOOK = "MDX_MSD_STAGE_BYTES"
EPS = 2.0 ** -52

# scripted rows of a walk with at least N_SCRIPTED rows (smaller walks hold random walkers only)
ROLES = {"crosser": 0, "runner": 1, "still": 2, "tie": 3, "near": 4}
N_SCRIPTED = 7                                   # the five above, one random walker, the last row (a second runner)
RUNNER_V = np.array([37, -53, 29])               # units per frame, |v| < L/2 in every dimension


def to_float(xq, dtype=np.float64, bits=Q_BITS):
    """Integers in units of 2^-bits -> floats, exactly (asserted)."""
    xq = np.asarray(xq, dtype=np.int64)
    assert np.abs(xq).max(initial=0) < (1 << 53)
    out = np.ldexp(xq.astype(np.float64), -bits).astype(dtype)
    assert np.array_equal(np.ldexp(out.astype(np.float64), bits), xq), "not representable"
    return out


def default_cross_at(n_frames, boundaries=()):
    """Frames f whose pair f - 1 -> f the crosser crosses on: 0 -> 1, the last pair, 126 -> 127, 127 -> 128 and 128 -> 129
    (both sides of a segment boundary, on consecutive frames) and the pair that straddles every stated block boundary."""
    want = {1, n_frames - 1, SEG - 1, SEG, SEG + 1} | set(int(b) for b in boundaries)
    return tuple(sorted(f for f in want if 1 <= f < n_frames))


def block_boundaries(n_frames, block):
    return tuple(range(block, n_frames, block)) if block >= 1 else ()


def lattice_walk(n_frames, n_rows, seed, cross_at=None, f64=False):
    """int64[T, n, 3] wrapped coordinates in q, in [0, L).  Rows ``ROLES`` (walks of at least N_SCRIPTED rows) are
    scripted; row 85 (coordinates 255 .. 257: threads 255 / 0 / 1 of two blocks) is a second crosser when it exists;
    the last row of other walks is a second runner; everything else walks randomly with steps of up to 150 units,
    which crosses often."""
    T, n = int(n_frames), int(n_rows)
    rng = np.random.default_rng([seed, T, n])
    steps = rng.integers(-150, 151, (T, n, 3))
    steps[0] = rng.integers(0, L_UNITS, (n, 3))
    w = np.cumsum(steps, axis=0) % L_UNITS
    t = np.arange(T)
    if cross_at is None:
        cross_at = default_cross_at(T)
    if n >= N_SCRIPTED:
        hits = np.zeros(T, dtype=np.int64)
        hits[list(cross_at)] = 1
        parity = np.cumsum(hits) % 2
        crosser = np.where(parity[:, None] == 0, L_UNITS - 5, 3)        # L - 5 <-> 3: a true step of 8 units
        w[:, ROLES["crosser"]] = crosser
        if n > 85:
            w[:, 85] = np.where(parity[:, None] == 0, 3, L_UNITS - 5)  # the other way round
        w[:, ROLES["runner"]] = (np.array([11, 500, 77]) + t[:, None] * RUNNER_V) % L_UNITS
        if n - 1 != 85:
            w[:, n - 1] = (np.array([700, 20, 600]) - t[:, None] * RUNNER_V) % L_UNITS
        w[:, ROLES["still"]] = np.array([100, 200, 300]) + (t % 2)[:, None]
        half = L_UNITS // 2
        a = np.array([10, 10, 10])
        tie = np.where(((t >= T // 3) & (t < 2 * T // 3))[:, None], a + half, a)    # d = +L/2, later -L/2
        w[:, ROLES["tie"]] = tie
        fifth = t * 5 // max(T, 1)                                       # 0 .. 4
        near = np.where((fifth == 1)[:, None], a + half - 1, np.where((fifth == 3)[:, None], a + half + 1, a))
        w[:, ROLES["near"]] = near
    assert w.min() >= 0 and (w < L_UNITS).all()
    wq = w.astype(np.int64) * UNIT
    if f64:
        wq = wq + rng.integers(1, UNIT, (1, n, 1))      # below one unit: the coordinates stay in [0, L)
    return wq


# ------------------------------------------------------------------------------------------------ the definition
def image_steps(wq, lq=LQ):
    """int[T, n, 3]: the change of the image flag on the pair t - 1 -> t (0 at t = 0)."""
    d = np.diff(wq, axis=0, prepend=wq[:1])
    return np.where(2 * np.abs(d) >= lq, -np.sign(d), 0)


def unwrap_ref(wq, images0=None, unwrap=True, shift_q=None, lq=LQ):
    """The prepared block in q (or in the units of ``lq``): unwrapped from the flags ``images0`` (default 0) when
    ``unwrap``, then minus the per-frame ``shift_q[T, 3]``."""
    out = np.array(wq, dtype=np.int64)
    if unwrap:
        img = np.cumsum(image_steps(wq, lq), axis=0, dtype=np.int64)
        if images0 is not None:
            img = img + np.asarray(images0, dtype=np.int64)[None]
        out = out + img * lq
    if shift_q is not None:
        out = out - np.asarray(shift_q, dtype=np.int64)[:, None, :]
    return out


def unwrap_ref_serial(wq, images0=None):
    """The same walk frame by frame, as the definition is written (the check of ``unwrap_ref``'s cumulative sum)."""
    img = np.zeros(wq.shape[1:], dtype=np.int64) if images0 is None else np.array(images0, dtype=np.int64)
    out = np.empty_like(wq)
    old = wq[0]
    for t in range(wq.shape[0]):
        d = wq[t] - old
        crossed = 2 * np.abs(d) >= LQ
        img[crossed] -= np.sign(d[crossed])
        old = wq[t]
        out[t] = wq[t] + img * LQ
    return out


def wrap_ref(xq, lq=LQ):
    """x -= floor(x / L) L only where x < 0 or x > L (so L stays L), in integers."""
    xq = np.asarray(xq, dtype=np.int64)
    outside = (xq < 0) | (xq > lq)
    return np.where(outside, xq - (xq // lq) * lq, xq)


def centre_ref(xq, masses):
    """sum m x / sum m per frame of ``xq[T, n, 3]`` as exact rationals: object array [T, 3] of Fractions in q."""
    m = [Fraction(v) for v in np.asarray(masses, dtype=np.float64).tolist()]
    total = sum(m)
    out = np.empty(xq.shape[:1] + (3,), dtype=object)
    for t in range(xq.shape[0]):
        for k in range(3):
            out[t, k] = sum(mi * int(x) for mi, x in zip(m, xq[t, :, k].tolist()) if mi) / total
    return out


def centre_dyadic(xq, masses_int, extra_bits):
    """Integer masses whose total is 2^extra_bits: the centre in units of 2^-(Q_BITS + extra_bits), exactly."""
    m = np.asarray(masses_int, dtype=np.int64)
    assert int(m.sum()) == 1 << extra_bits
    return (xq * m[None, :, None]).sum(axis=1)


def fractions_to_float(fr, bits=Q_BITS):
    """Correctly rounded float64 of Fractions in units of 2^-bits."""
    return np.array([[float(v / (1 << bits)) for v in row] for row in fr], dtype=np.float64)


def molecule_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def molecule_centres_dyadic(xq, offsets, masses_int, extra_bits):
    """Every molecule's total is 2^extra_bits: centres int64[T, n_mol, 3] in units of 2^-(Q_BITS + extra_bits)."""
    m = np.asarray(masses_int, dtype=np.int64)
    out = np.empty((xq.shape[0], len(offsets) - 1, 3), dtype=np.int64)
    for g in range(len(offsets) - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        assert int(m[lo:hi].sum()) == 1 << extra_bits
        out[:, g] = (xq[:, lo:hi] * m[None, lo:hi, None]).sum(axis=1)
    return out


def molecule_centres_restated(x, offsets, masses):
    """What the molecule kernel promises for any masses: separate float64 multiply and add in row order from 0.0 and
    one division by the sequentially summed mass.  x: float64[T, n, 3] -> float64[T, n_mol, 3]."""
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(masses, dtype=np.float64)
    out = np.empty((x.shape[0], len(offsets) - 1, 3))
    for g in range(len(offsets) - 1):
        acc = np.zeros((x.shape[0], 3))
        total = np.float64(0.0)
        for a in range(int(offsets[g]), int(offsets[g + 1])):
            acc = acc + m[a] * x[:, a]
            total = total + m[a]
        out[:, g] = acc / total
    return out


# ------------------------------------------------------------------------------------------------ planted events
def events_of(wq, images0=None):
    """The events present in a walk: a set of names, ``("cross", f)`` for every pair f - 1 -> f some coordinate crosses
    on, and ``("row", name)`` facts about single rows."""
    found = set()
    d = np.diff(wq, axis=0, prepend=wq[:1])
    step = image_steps(wq)
    for k in range(3):
        dk = d[:, :, k]
        if (dk == LQ[k] // 2).any():
            found.add(f"tie+{k}")
        if (dk == -(LQ[k] // 2)).any():
            found.add(f"tie-{k}")
        if (np.abs(dk) == LQ[k] // 2 - UNIT).any():
            found.add(f"below{k}")
        if (np.abs(dk) == LQ[k] // 2 + UNIT).any():
            found.add(f"above{k}")
    # ties count, the displacement just below does not
    assert np.array_equal(step != 0, 2 * np.abs(d) >= LQ)
    for f in np.flatnonzero(step.any(axis=(1, 2))):
        found.add(("cross", int(f)))
    img = np.cumsum(step, axis=0)
    if images0 is not None:
        img = img + np.asarray(images0)[None]
    if np.abs(img).max(initial=0) >= 3:
        found.add("image3")
    if (~step.any(axis=(0, 2))).any():
        found.add("never")
    if wq.shape[0] >= 3 and ((step[1:-1] * step[2:]) == -1).any():
        found.add("flip")
    return found


def claims_of(n_frames, n_rows, cross_at=None):
    """What a walk of ``lattice_walk`` must hold, by its size."""
    T, n = int(n_frames), int(n_rows)
    claims = set()
    if n < N_SCRIPTED:
        return claims
    for f in (default_cross_at(T) if cross_at is None else cross_at):
        claims.add(("cross", int(f)))
    claims.add("never")
    if T >= 6:
        claims |= {f"{name}{k}" for name in ("tie+", "tie-", "below", "above") for k in range(3)}
    if T >= SEG + 2:
        claims |= {"flip", ("cross", SEG - 1), ("cross", SEG), ("cross", SEG + 1)}
    if T >= 100:
        claims.add("image3")
    if T >= 2:
        claims |= {("cross", 1), ("cross", T - 1)}
    return claims


def assert_claims(wq, claims, images0=None):
    missing = set(claims) - events_of(wq, images0)
    assert not missing, f"planted events missing: {sorted(map(str, missing))}"


# ------------------------------------------------------------------------------------------------ hook arithmetic
def ceil_div(a, b):
    return -(-a // b)


def frame_block(n_frames, n_rows, elem, stage_bytes=None, resident=False):
    """``msd_frame_block``: frames per unwrap launch."""
    most = 32768 * SEG if resident else (stage_bytes or STAGE_DEFAULT) // (3 * elem * n_rows)
    return max(1, min(n_frames, most))


def push_plan(n_frames, n_sel, elem, stage_bytes, offsets=None, resident=False):
    """``msd_push_frames`` under the hook: (chunk, cuts, frames per block)."""
    chunk = max(1, stage_bytes // (n_frames * 24))
    chunk = min(chunk, n_sel)
    chunk = ceil_div(n_sel, ceil_div(n_sel, chunk))
    cuts = [0]
    if offsets is not None:
        sizes = np.diff(offsets)
        chunk = max(chunk, int(sizes.max()))
        for m in range(len(sizes)):
            if offsets[m + 1] - cuts[-1] > chunk:
                cuts.append(int(offsets[m]))
        cuts.append(n_sel)
    else:
        cuts += list(range(chunk, n_sel, chunk)) + [n_sel]
    return chunk, cuts, frame_block(n_frames, chunk, elem, stage_bytes, resident)


# ------------------------------------------------------------------------------------------------ case families
FRAME_COUNTS = (1, 2, 127, 128, 129, 257, 300)     # frames per block of family A (the engine holds 1 or 3 blocks)
PARTICLE_COUNTS = (1, 85, 86, 171)                 # 3, 255, 258 and 513 coordinates: around the 256-thread blocks
N_BLOCKS = (1, 3)
DECOYS = 5                                         # rows of a frame that no index lists
B_FRAMES = 300
B_BLOCKS = (1, 127, 128, 129, 200)                 # frames per launch of family B
B_ROWS = 7                                         # family B through push_*: one-particle chunks (see b_stage_bytes)
C_ROWS, C_CHUNK = 86, 7
NATURAL_ROWS = 22400                               # 80 MB of float32 frames: blocks of 249 + 51 at the natural constant
G_SIZES = (1, 2, 3, 5, 1, 4) * 5 + (1, 5)          # 86 rows in 32 molecules; the largest holds 5
G_DYADIC = {1: (8,), 2: (3, 5), 3: (1, 2, 5), 4: (1, 3, 2, 2), 5: (3, 1, 1, 2, 1)}     # every molecule weighs 2^3
H_FRAMES = 65537


def b_stage_bytes(block, elem, n_rows=1):
    """The hook value that makes ``frame_block`` of ``n_rows`` rows equal ``block``.  Through ``msd_push_frames`` the
    same number is the chunk's budget: a block shorter than the series needs bytes < 3 elem rows T <= 24 rows T, so the
    chunk is ONE particle there (or, with a grouping, the largest molecule): frame blocks are plural in push_* only
    together with one-particle (one-molecule-sized) chunks.  ``msd_system_com_frames`` has no chunks."""
    return block * 3 * elem * n_rows


def index_kinds(n_rows, seed):
    """name -> (n_total, index or None) of the selections family A reads out of HBM-resident frames."""
    rng = np.random.default_rng([seed, n_rows])
    n_total = n_rows + DECOYS
    scattered = rng.permutation(n_total)[:n_rows]
    twice = scattered.copy()
    if n_rows >= N_SCRIPTED:
        twice[6] = twice[5]                      # a row listed twice (not a scripted one)
    else:
        twice = np.concatenate([twice, twice[:1]])
    return {"none": (n_rows, None), "contiguous": (n_total, np.arange(2, 2 + n_rows)),
            "scattered": (n_total, scattered), "twice": (n_total, twice)}


def scatter_rows(sel_q, n_total, index, seed):
    """int64[T, n_total, 3] whose rows ``index`` are ``sel_q``'s (a row listed twice keeps the later assignment: the
    truth of a selection is always ``frames[:, index]``) and whose other rows are decoys."""
    rng = np.random.default_rng([seed, n_total, 17])
    frames = rng.integers(0, L_UNITS, (sel_q.shape[0], n_total, 3)) * UNIT
    if index is None:
        return np.array(sel_q)
    frames[:, index] = sel_q
    return frames


def frame_lists(n_frames, seed):
    """(regular, irregular, frames in the file): the regular list takes the even file frames, the strictly increasing
    irregular one odd frames with gaps; every other frame of the file is a decoy."""
    rng = np.random.default_rng([seed, n_frames, 23])
    regular = 2 * np.arange(n_frames)
    slots = n_frames + max(2, n_frames // 8)
    irregular = 2 * np.sort(rng.choice(slots, n_frames, replace=False)) + 1
    return regular, irregular, 2 * slots + 1


def file_frames(sel_q, n_total, index, seed):
    """int64[F_file, n_total, 3] for a trajectory file: the walk at both frame lists, decoys elsewhere."""
    T = sel_q.shape[0]
    regular, irregular, n_file = frame_lists(T, seed)
    rng = np.random.default_rng([seed, n_total, 29])
    out = rng.integers(0, L_UNITS, (n_file, n_total, 3)) * UNIT
    walk = scatter_rows(sel_q, n_total, index, seed)
    out[regular] = walk
    out[irregular] = walk
    return out


def ingest_lags(t_block):
    """The lags observable (c) is compared at: both ends, the middle and eight seeded ones."""
    fixed = {0, 1, 2, 3, t_block // 2, t_block - 2, t_block - 1}
    rng = np.random.default_rng(t_block)
    return np.array(sorted({m for m in fixed if 0 <= m < t_block} | set(rng.integers(0, t_block, 8).tolist())))


def wrap_rows(n_frames):
    """int64[T, 6, 3] UNWRAPPED coordinates in q for the wrap tests: exactly 0, L, 2 L, -L, one unit below 0, one unit
    above L, constant in time."""
    rows = np.stack([0 * LQ, LQ, 2 * LQ, -LQ, 0 * LQ - UNIT, LQ + UNIT])
    return np.broadcast_to(rows[None], (n_frames, 6, 3)).copy()


def wrap_rows_wrapped():
    """(wrapped coordinates int64[6, 3] in q, image flags int[6, 3]) whose unwrapped values are ``wrap_rows``'s."""
    w = np.stack([0 * LQ, 0 * LQ, 0 * LQ, 0 * LQ, LQ - UNIT, 0 * LQ + UNIT])
    img = np.array([[0] * 3, [1] * 3, [2] * 3, [-1] * 3, [-1] * 3, [1] * 3])
    return w, img


def arbitrary_masses(n, seed):
    rng = np.random.default_rng([seed, n, 31])
    return rng.uniform(0.5, 40.0, n)


def dyadic_masses(n, seed, bits=10):
    """Integer masses that sum to 2^bits."""
    rng = np.random.default_rng([seed, n, 37])
    total = 1 << bits
    assert n <= total
    m = np.ones(n, dtype=np.int64)
    extra = rng.multinomial(total - n, np.full(n, 1.0 / n))
    return m + extra


def g_masses_dyadic():
    return np.concatenate([G_DYADIC[s] for s in G_SIZES]).astype(np.int64)


IngestCase = namedtuple("IngestCase", "name n_frames n_rows f64 seed cross_at images n_blocks", defaults=(1,))


def case_walk(c):
    """(wrapped walk in q, initial image flags or None) of a case."""
    wq = lattice_walk(c.n_frames, c.n_rows, c.seed, c.cross_at, c.f64)
    images0 = None
    if c.images:
        images0 = np.random.default_rng([c.seed, 41]).integers(-2, 3, (c.n_rows, 3))
    return wq, images0


def shift_of(c):
    """A shift that differs in every frame, in q: up to two box lengths."""
    rng = np.random.default_rng([c.seed, 47])
    return rng.integers(-2 * 1024, 2 * 1024, (c.n_frames, 3)) * UNIT


def a_case(frames, n_blocks, n_rows, f64):
    T = frames * n_blocks
    return IngestCase(f"A T={frames}x{n_blocks} n={n_rows} {'f64' if f64 else 'f32'}", T, n_rows, f64, 3, None, False,
                      n_blocks)


def natural_case():
    """22 400 rows x 300 frames of float32 from host memory WITHOUT the hook: blocks of 249 + 51 frames.  Kept in
    lattice units (int32) to stay small: (wrapped walk int32[T, n, 3] in units, summed unwrapped trajectory int64[T, 3]
    in units, the block)."""
    block = frame_block(B_FRAMES, NATURAL_ROWS, 4)
    rng = np.random.default_rng(43)
    steps = rng.integers(-150, 151, (B_FRAMES, NATURAL_ROWS, 3), dtype=np.int32)
    steps[0] = rng.integers(0, L_UNITS, (NATURAL_ROWS, 3))
    lu = L_UNITS.astype(np.int32)
    w = np.cumsum(steps, axis=0, dtype=np.int32) % lu
    del steps
    t = np.arange(B_FRAMES)
    for row, sign in ((0, 1), (NATURAL_ROWS - 1, -1)):          # cross on block - 1 -> block and nowhere else
        w[:, row] = np.where((t >= block)[:, None] == (sign > 0), 3, lu - 5)
    step = image_steps(w, lu)
    assert step[block, 0].all() and step[block, NATURAL_ROWS - 1].all() and not step[:block, 0].any()
    traj = (w.astype(np.int64) + np.cumsum(step, axis=0, dtype=np.int64) * L_UNITS).sum(axis=1)
    return w, traj, block


def b_case(block, n_rows, f64, images=True):
    cross = default_cross_at(B_FRAMES, block_boundaries(B_FRAMES, block))
    return IngestCase(f"B block={block} n={n_rows} {'f64' if f64 else 'f32'}", B_FRAMES, n_rows, f64, 5, cross, images)


def c_case(f64, images=True):
    return IngestCase(f"C n={C_ROWS} {'f64' if f64 else 'f32'}", B_FRAMES, C_ROWS, f64, 7, None, images)


A_CASES = [a_case(t, b, n, f64) for t in FRAME_COUNTS for b in N_BLOCKS for n in PARTICLE_COUNTS for f64 in (False, True)]
# (block, rows, float64): a block of ONE frame on few rows only: it is rows x 300 launches
B_PARAMS = ([(blk, B_ROWS, f64) for blk in B_BLOCKS for f64 in (False, True)]
            + [(blk, C_ROWS, f64) for blk in B_BLOCKS[1:] for f64 in (False, True)])
B_CASES = [b_case(*p) for p in B_PARAMS]
C_CASES = [c_case(False), c_case(True)]
G_CASE = IngestCase("G molecules", B_FRAMES, int(np.sum(G_SIZES)), False, 11,
                    default_cross_at(B_FRAMES, block_boundaries(B_FRAMES, 127)), False)
ALL_CASES = A_CASES + B_CASES + C_CASES + [G_CASE]
