"""
The LDS form of the cell-sorted pair kernel bins in 16.16 fixed point (``cell_fixed_q``): every case here plans to
that form (or, for one, to the global form that keeps the float position) and its counts must EQUAL those of
``oracle.cbind.c_radial_histogram``.

The inputs put pairs where the fixed-point value is at its limits: at distance 0 and below ``eta`` bin widths (negative
positions: the convert rounds down and the low half must come out high), exactly on bin edges and within ``eta`` of
both range ends, in bricks dense enough in on-edge pairs that a wave's list overflows and the unit is redone through
the shared mapping, at bin counts around 255 (where ``2^16 pos`` crosses 2^24 and its low bits fall off the float),
at every replica count (the address is ``bin * 4 R + base``, a multiply where a shift was), beyond the range of the
skipping step (the unconditional tail), in a small box at half its length (the straddling loops) and in a triclinic cell.
"""
import functools

import numpy as np
import pytest

from mdhelper_amd import _core
from oracle.cbind import c_radial_histogram
from test_rdf_fixed_bin_host import fixed_form, fma32

ORTHO = (30.0, 29.5, 31.0, 90.0, 90.0, 90.0)
SMALL = (12.0, 12.5, 12.25, 90.0, 90.0, 90.0)
TRI = (31.0, 28.5, 35.25, 75.0, 80.0, 110.0)


def _gas(rng, n, box):
    return (rng.random((n, 3)) * np.asarray(box[:3])).astype(np.float32)


def _eta_w(c):
    """eta of the frame in Angstrom, from the engine's own constants"""
    edges = np.linspace(c["rng"][0], c["rng"][1], c["bins"] + 1)
    k = _core.RdfEngine.filter_constants(edges, c["box"][:3], max(c["box"][:3]))
    return k["eta"] * (edges[1] - edges[0])


def _coincident(c, rng, pos):
    """64 sites with two particles each: a quarter at distance 0, the rest at 0.05 .. 1.9 eta bin widths"""
    ew = _eta_w(c)
    sites = pos[:64].copy()
    gap = np.where(np.arange(64) % 4 == 0, 0.0, np.linspace(0.05, 1.9, 64) * ew)
    pos[64:128] = sites
    pos[64:128, 0] += gap.astype(np.float32)


def _brick(c, rng, pos, origin=(4.0, 4.0, 4.0), side=8):
    """side^3 particles on a lattice whose constant is five bin widths of the (0, 6) / 60 range and a multiple of 2^-1:
    every coordinate and every difference is exact, and the pairs along the axes sit exactly on bin edges"""
    g = np.arange(side, dtype=np.float32) * np.float32(0.5)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin, dtype=np.float32)
    pos[:xyz.shape[0]] = xyz


def _range_ends(c, rng, pos):
    """dimers at r0 and r1 and within 0.2 eta bin widths of either, on both sides, along the three axes"""
    ew = _eta_w(c)
    r0, r1 = c["rng"]
    seps = [r + d * ew for r in ((r0, r1) if r0 > 0 else (r1,)) for d in (-0.6, -0.2, -0.01, 0.0, 0.01, 0.2, 0.6)]
    k = 0
    for sep in seps:
        for axis in range(3):
            pos[2 * k + 1] = pos[2 * k]
            pos[2 * k + 1, axis] += np.float32(sep)
            k += 1


def _nothing(c, rng, pos):
    pass


def _case(name, n=2048, n2=None, box=ORTHO, rng=(0.0, 6.0), bins=60, excl=None, frames=1, build=_nothing, plan=None,
          stats=()):
    base = {"family": 2, "gh": 0}
    base.update(plan or {})
    return dict(name=name, n=n, n2=n2, box=box, rng=rng, bins=bins, excl=excl, frames=frames, build=build, plan=base,
                stats=stats)


CASES = [
    _case("coincident and nearly coincident, r0 = 0", build=_coincident, frames=2, plan={"n_hist": 8, "lower": 0}),
    _case("coincident, 201 bins to 15 of 68.94", n=4096, box=(68.94, 68.94, 68.94, 90.0, 90.0, 90.0), rng=(0.0, 15.0),
          bins=201, build=_coincident, plan={"n_hist": 8, "skip": 1}),
    _case("brick on bin edges, self", build=_brick, stats=("exact",), plan={"skip": 1}),
    _case("brick on bin edges, self, exclusion (1, 1)", build=_brick, excl=(1, 1), frames=3, stats=("exact",)),
    _case("brick on bin edges, two groups", n2=3000, build=_brick, stats=("exact",), plan={"self": 0}),
    _case("brick on bin edges, range (3, 6)", rng=(3.0, 6.0), bins=30, build=_brick, excl=(1, 1), stats=("exact",),
          plan={"lower": 1}),
    _case("within eta of r1", build=_range_ends, excl=(1, 1), frames=2),
    _case("within eta of r0 and r1, range (3, 6)", rng=(3.0, 6.0), build=_range_ends, plan={"lower": 1}),
    _case("254 bins", bins=254, build=_range_ends, plan={"n_hist": 4}),
    _case("255 bins", bins=255, build=_coincident, plan={"n_hist": 4}),
    _case("256 bins", bins=256, build=_brick, excl=(1, 1), plan={"n_hist": 4}),
    _case("3000 bins, two replicas", bins=3000, build=_brick, plan={"n_hist": 2}),
    _case("5000 bins, one replica", bins=5000, build=_coincident, excl=(1, 1), plan={"n_hist": 1}),
    _case("5200 bins, global form", bins=5200, build=_brick, plan={"gh": 1, "n_hist": 0}),
    _case("range end beyond the skipping step", rng=(0.0, 10.0), bins=100, build=_brick, excl=(1, 1),
          plan={"skip": 0, "n_hist": 8}, stats=("exact",)),
    _case("small box, range to half its length", box=SMALL, rng=(0.0, 6.0), bins=60, build=_brick, excl=(1, 1),
          plan={"skip": 0}, stats=("exact", "general")),
    _case("small box, range (3, 6)", box=SMALL, rng=(3.0, 6.0), bins=127, build=_range_ends,
          plan={"skip": 0, "lower": 1}, stats=("general",)),
    _case("triclinic", box=TRI, rng=(0.0, 6.0), bins=60, build=_brick, excl=(1, 1), plan={"family": 4, "skip": 1},
          stats=("exact",)),
]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(c for c in CASES if c["name"] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    pos1 = np.stack([_gas(rng, c["n"], c["box"]) for _ in range(c["frames"])])
    pos2 = None if c["n2"] is None else np.stack([_gas(rng, c["n2"], c["box"]) for _ in range(c["frames"])])
    for f in range(c["frames"]):
        c["build"](c, rng, pos1[f])
        if pos2 is not None:   # the second group's brick stands five lattice constants from the first
            _brick(c, rng, pos2[f], origin=(6.5, 4.0, 4.0), side=6)
    boxes = np.tile(np.asarray(c["box"], dtype=np.float32), (c["frames"], 1))
    want = np.zeros(c["bins"], dtype=np.int64)
    for f in range(c["frames"]):
        c_radial_histogram(pos1[f], pos1[f] if pos2 is None else pos2[f], c["bins"], c["rng"], boxes[f],
                           exclusion=c["excl"], counts=want)
    for a in (pos1, pos2, boxes, want):
        if a is not None:
            a.setflags(write=False)
    return pos1, pos2, boxes, want


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case_plans_to_its_form(c):
    edges = np.linspace(c["rng"][0], c["rng"][1], c["bins"] + 1)
    p = _core.RdfEngine.plan(edges, c["excl"], "auto", c["n"], c["n2"], c["box"], c["frames"])
    assert {k: p[k] for k in c["plan"]} == c["plan"], p


def test_every_replica_count_of_the_lds_form_is_run():
    edges = lambda c: np.linspace(c["rng"][0], c["rng"][1], c["bins"] + 1)
    seen = {_core.RdfEngine.plan(edges(c), c["excl"], "auto", c["n"], c["n2"], c["box"], c["frames"])["n_hist"]
            for c in CASES if not c["plan"]["gh"]}
    assert seen == {1, 2, 4, 8}


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_counts_equal_the_oracle(c):
    pos1, pos2, boxes, want = _inputs(c["name"])
    assert want.sum() >= 1000
    edges = np.linspace(c["rng"][0], c["rng"][1], c["bins"] + 1)
    eng = _core.RdfEngine(edges, c["excl"], algo="auto")
    eng.accumulate(pos1, pos2, boxes)
    got, st = eng.counts(), eng.stats()
    eng.close()
    np.testing.assert_array_equal(got, want)
    assert st["cell_units"] > 0, st
    if "exact" in c["stats"]:
        assert st["pairs_exact"] > 0, st
    if "general" in c["stats"]:
        assert st["cell_units_general"] > 0, st


# ------------------------------------------------------------------------- the threshold of the low half, to the unit

TQ_BOX = (168.0, 168.0, 168.0, 90.0, 90.0, 90.0)
TQ_RANGE, TQ_BINS = (0.0, 6.0), 60


@functools.lru_cache(maxsize=None)
def _tq_dimers():
    """Two frames of 128 isolated dimers, 7 apart on the plane z = 0 of a 168 box, each along z from z = 0 (every
    coordinate and every difference exact, so the step's r2 is fl(s s)): in the first the fixed-point position of
    every dimer has the low half TQ - 1 (sure), in the second TQ (undecided) — for every float32 within 2 ulp of s, so
    that the rounding of s s and the one ulp of v_sqrt_f32 cannot move a dimer to the other side."""
    edges = np.linspace(*TQ_RANGE, TQ_BINS + 1)
    # eta depends on the largest |coordinate| of the batch, which the engine takes from the frames: the last column
    max_abs = 3.5 + 7.0 * 23
    k = _core.RdfEngine.filter_constants(edges, TQ_BOX[:3], max_abs)
    s = np.arange(np.float32(1.0).view(np.int32), np.float32(4.0).view(np.int32), dtype=np.int32).view(np.float32)
    qf = fma32(s, np.float32(k["iwq"]), np.float32(k["p0q"]))
    low = np.floor(qf.astype(np.float64)).astype(np.int64) & 0xFFFF
    site = np.arange(128)
    boxes = np.asarray([TQ_BOX], dtype=np.float32)
    frames = []
    for want_low in (k["tq"] - 1, k["tq"]):
        hit = low == want_low
        core = hit[4:] & hit[3:-1] & hit[2:-2] & hit[1:-3] & hit[:-4]        # s - 2 ulp .. s + 2 ulp
        idx = np.nonzero(core)[0] + 2
        assert idx.size >= 128, idx.size
        pos = np.zeros((1, 256, 3), dtype=np.float32)
        pos[0, 0::2, 0] = pos[0, 1::2, 0] = 3.5 + 7.0 * (site % 24)
        pos[0, 0::2, 1] = pos[0, 1::2, 1] = 3.5 + 7.0 * (site // 24)
        pos[0, 1::2, 2] = s[idx[np.linspace(0, idx.size - 1, 128).astype(int)]]
        assert float(np.abs(pos).max()) == max_abs
        frames.append((pos, c_radial_histogram(pos[0], pos[0], TQ_BINS, TQ_RANGE, boxes[0], exclusion=(1, 1))))
    return frames, boxes, k


def test_tq_dimers_are_what_they_claim():
    frames, boxes, k = _tq_dimers()
    for (pos, want), is_sure in zip(frames, (True, False)):
        assert want.sum() == 2 * 128                      # the dimers' own pairs and nothing else
        sure, _ = fixed_form(pos[0, 1::2, 2].copy(), k)
        assert np.all(sure == is_sure)


@pytest.mark.gpu
def test_low_half_equal_to_tq_is_undecided_and_one_below_is_sure():
    """`pairs_exact` counts the pairs the steps listed for the exact arithmetic (a pair of one diagonal tile is met
    from both sides and listed twice): none of the dimers whose low half is TQ - 1, every dimer whose low half is TQ.
    A threshold one too high lists none of the second frame, one too low all of the first."""
    frames, boxes, k = _tq_dimers()
    edges = np.linspace(*TQ_RANGE, TQ_BINS + 1)
    p = _core.RdfEngine.plan(edges, (1, 1), "auto", 256, None, TQ_BOX, 1)
    assert (p["family"], p["gh"], p["excl"]) == (2, 0, 1)
    listed = []
    for pos, want in frames:
        eng = _core.RdfEngine(edges, (1, 1), algo="auto")
        eng.accumulate(pos, None, boxes)
        got, st = eng.counts(), eng.stats()
        eng.close()
        np.testing.assert_array_equal(got, want)
        listed.append(st["pairs_exact"])
    assert listed[0] == 0 and 128 <= listed[1] <= 256, listed
