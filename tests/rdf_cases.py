"""
Inputs, environments and intended kernels of the RDF route tests: shared by ``test_rdf_plan_host.py`` (which checks on
the CPU that every case plans to the kernel family, template arguments and histogram form it states) and
``test_gpu_rdf_routes.py`` (which runs them against the fp64 oracle).  The cases were chosen with the plan query
(``RdfEngine.plan``); what each states is written down here from the selection rules, not read back from the plan.

Families of ``mdx_rdf.hip`` and their instantiations (56 in all):
  tile-exact / tile-filter   rdf_tile_kernel<MODE, IPT, PBC, EXCL, GH>                      2 x 2 x 2 x 2 x 2 = 32
  cell-ortho / tri-culled    rdf_cell_pair_kernel<EXCL, LOWER, MODE, TRI, SKIP>: EXCL x LOWER x
                             {skip, no-skip, global histogram, triclinic, triclinic global}     2 x 2 x 5 = 20
  tri-brute                  rdf_tri_tile_kernel<EXCL, GH>                                          2 x 2 =  4
"""

import zlib
from collections import namedtuple

import numpy as np

FAMILIES = ("tile-exact", "tile-filter", "cell-ortho", "tri-brute", "tri-culled")
SWITCHES = ("MDX_RDF_SLAB_BYTES", "MDX_RDF_TRI_BRUTE", "MDX_RDF_CHUNK_TILES", "MDX_RDF_SORT_BESIDE",
            "MDX_RDF_LDS_FLUSH_UNITS", "MDX_RDF_PIPE_MB")
BRUTE = {"MDX_RDF_TRI_BRUTE": "1"}

# unequal edges, so that an axis mix-up shows; 0.3 x the shortest is 7.098: a range end of 6 keeps the skipping step of
# the cell kernel, 9 (still below half the shortest edge) takes the unconditional tail
ORTHO = (24.17, 24.0, 23.66, 90.0, 90.0, 90.0)
# half the smallest cell height is above 6 * 1.02 + 1e-3: from 1 024 particles on, AUTO and CELL take the culled kernel
TRI = (31.0, 28.5, 35.25, 75.0, 80.0, 110.0)
# the a axis of the row lattice (family F): 64 sites 0.5 apart
TRI_ROWS = (32.0, 28.5, 35.25, 75.0, 80.0, 110.0)
RANGE, RANGE_LOWER, RANGE_NOSKIP, RANGE_NOSKIP_LOWER = (0.0, 6.0), (2.0, 6.0), (0.0, 9.0), (2.0, 9.0)

# largest bin count of every replica count; beyond the last: the global histogram (base + n_hist x 4 x bins against
# 64 KiB; the cell kernel also holds 8 replicas while 13 KiB suffice, and has one spare word per replica)
TILE256_STEPS = ((2559, 4), (3839, 2), (5119, 1))       # rdf_tile_kernel at IPT = 1, rdf_tri_tile_kernel
TILE512_STEPS = ((2389, 4), (3583, 2), (4778, 1))       # rdf_tile_kernel at IPT = 2
CELL_STEPS = ((229, 8), (2559, 4), (3839, 2), (5119, 1))
# first bin count whose dynamic LDS exceeds 48 KiB (4 replicas each)
TILE256_ATTR, TILE512_ATTR, CELL_48K = 1878, 1707, 1877
# bin counts that take 2 replicas, 1 replica and the global histogram in every family at once
FORM_BINS = {2: 3000, 1: 4500, 0: 5200}

# name; family: index into FAMILIES; n1, n2 (None: one set); frames; box (six numbers or None); bins, range, excl, algo,
# env; build: the construction of the positions (``positions``); plan: the plan fields the case is meant to reach;
# claims: what keeps it from passing vacuously — "ends" (first and last bin hold pairs), "exact" (pairs go through the
# exact re-evaluation), "general" (cell units on the per-pair image path), "culled" (fewer than half of the pairs are
# evaluated), "tiny" (one particle: exempt from the 1 000 pairs, the counts are known), "lattice" (the counts of the
# lattice pairs, those exactly at r0 and r1 among them, are known: ``lattice_counts``); repeats: runs on the GPU (3 where the order inside a cell differs from run to run and edge pairs exist)
Case = namedtuple("Case", "name group family n1 n2 frames box bins range excl algo env build plan claims repeats")


def n_hist_of(bins, steps):
    """(n_hist, gh) of a bin count by a family's table."""
    for top, n in steps:
        if bins <= top:
            return n, 0
    return 0, 1


def _steps(family, n1, n2):
    if family in (2, 4):
        return CELL_STEPS
    if family == 3:
        return TILE256_STEPS
    return TILE512_STEPS if max(n1, n2 or n1) >= 2048 else TILE256_STEPS


def case(group, name, family, n1, n2=None, *, box=ORTHO, bins=60, rng=RANGE, excl=(1, 1), algo=None, env=None,
         frames=2, build="gas+dimers", claims=("ends",), more=None):
    """A case and the plan it states, from the selection rules of mdx_rdf.hip."""
    fam = FAMILIES.index(family)
    algo = algo or {0: "exact", 1: "filter", 2: "cell", 3: "auto", 4: "auto"}[fam]
    n_hist, gh = n_hist_of(bins, _steps(fam, n1, n2))
    cellish = fam in (2, 4)
    plan = {"family": fam,
            "ipt": 2 if fam < 2 and max(n1, n2 or n1) >= 2048 else 1,
            "self": int(n2 is None and (excl is None or excl[0] == excl[1])),
            "excl": int(excl is not None), "pbc": int(box is not None),
            "lower": int(cellish and rng[0] > 0), "gh": gh, "n_hist": n_hist,
            "lazy_orig": int(fam == 2 and (excl is None or max(excl) <= 1))}
    if cellish and not gh:
        plan["skip"] = int(fam == 4 or rng[1] <= 0.3 * min(box[:3]))
    plan.update(more or {})
    claims = tuple(claims)
    if "dimers" in build and fam in (1, 2, 4) and "exact" not in claims:
        claims += ("exact",)        # separations swept through bin edges: the float32 filter cannot decide them
    repeats = 3 if cellish and "exact" in claims else 1
    return Case(f"{group}: {name}", group, fam, n1, n2, frames, box, bins, tuple(rng), excl, algo, dict(env or {}),
                build, plan, claims, repeats)


def set_env(monkeypatch, env):
    """The stated environment of a case: every switch of the RDF engine cleared, then those of ``env`` set."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def edges_of(c):
    return np.linspace(c.range[0], c.range[1], c.bins + 1)


def instantiation(plan):
    """The kernel instantiation a plan (a dict of plan fields) stands for."""
    fam = plan["family"]
    if fam < 2:
        return ("tile", ("exact", "filter")[fam], plan["ipt"], plan["pbc"], plan["excl"], plan["gh"])
    if fam == 3:
        return ("tri", plan["excl"], plan["gh"])
    form = ("tri-gh" if plan["gh"] else "tri") if fam == 4 else \
        ("gh" if plan["gh"] else ("skip" if plan["skip"] else "no-skip"))
    return ("cell", plan["excl"], plan["lower"], form)


ALL_INSTANTIATIONS = frozenset(
    [("tile", m, i, p, e, g) for m in ("exact", "filter") for i in (1, 2) for p in (0, 1) for e in (0, 1)
     for g in (0, 1)]
    + [("cell", e, lo, f) for e in (0, 1) for lo in (0, 1) for f in ("skip", "no-skip", "gh", "tri", "tri-gh")]
    + [("tri", e, g) for e in (0, 1) for g in (0, 1)])
# instantiations the selection code cannot produce, with the reason (none: all 56 are reached)
UNREACHABLE = {}

# ------------------------------------------------------------------------------------------------- positions

N_SWEEP = 8      # dimers per swept edge


def _dimer_separations(c):
    """Separations in the first and the last bin, and swept through the range ends and three interior edges."""
    e = edges_of(c)
    w = (c.range[1] - c.range[0]) / c.bins
    d = min(2e-4, 0.25 * w)
    r = [np.full(N_SWEEP, e[0] + 0.5 * w), np.full(N_SWEEP, e[-1] - 0.5 * w), np.linspace(e[-1] - d, e[-1] + d, N_SWEEP)]
    if c.range[0] > 0:
        r.append(np.linspace(e[0] - d, e[0] + d, N_SWEEP))
    for k in sorted({1, c.bins // 2, c.bins - 1} - {0, c.bins}):
        r.append(np.linspace(e[k] - d, e[k] + d, N_SWEEP))
    return np.concatenate(r)


def _lengths(c):
    return np.array(c.box[:3] if c.box is not None else ORTHO[:3])


def _gas(rng, n, L):
    return rng.uniform(0.0, 1.0, (n, 3)) * L


def _frame(c, rng):
    L = _lengths(c)
    n2 = c.n1 if c.n2 is None else c.n2
    if c.build == "gas":
        return _gas(rng, c.n1, L), (None if c.n2 is None else _gas(rng, n2, L))
    if c.build == "gas+dimers":
        r = _dimer_separations(c)
        u = rng.normal(size=(len(r), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        a = 0.2 * L + _gas(rng, len(r), 0.6 * L)
        b = a + u * r[:, None]
        if c.n2 is None:
            # a first, b last: no exclusion block of three rows holds both ends of a dimer
            assert c.n1 >= 2 * len(r) + 3
            return np.vstack((a, _gas(rng, c.n1 - 2 * len(r), L), b)), None
        assert c.n1 >= len(r) and n2 >= len(r) + 3
        return np.vstack((a, _gas(rng, c.n1 - len(r), L))), np.vstack((_gas(rng, n2 - len(r), L), b))
    if c.build == "coincident":
        # the last 50 rows lie exactly on the first 50: distinct particles at distance 0
        x = _gas(rng, c.n1 - 50, L)
        return np.vstack((x, x[:50])), None
    if c.build == "lattice":
        # simple cubic, spacing 1, filling the box: distances 1 and 2 are exact in float32 and equal r0 and r1
        side = round(c.n1 ** (1 / 3))
        assert side ** 3 == c.n1 and c.box[0] == c.box[1] == c.box[2] == side
        x = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        return rng.permutation(x), None
    if c.build == "rows":
        # rows along the a axis of a triclinic cell, sites one bin width (0.5) apart and periodic along a; the row
        # origins lie where the contract's wrap leaves them alone, so every separation inside a row is exact
        assert c.n1 % 64 == 0 and c.box[0] == 32.0
        rows = c.n1 // 64
        origin = np.column_stack((np.zeros(rows), rng.uniform(1.0, 20.0, rows), rng.uniform(1.0, 25.0, rows)))
        x = origin[:, None, :] + np.arange(64)[None, :, None] * np.array([0.5, 0.0, 0.0])
        return rng.permutation(x.reshape(-1, 3)), None
    raise ValueError(c.build)


def lattice_counts(c):
    """``(counts, exact)`` of the pairs a lattice construction puts into every bin by itself; ``exact``: nothing else
    lies in range.  Cubic lattice of spacing 1, range (1, 2), 4 bins: 6 neighbours at 1 = r0, 12 at sqrt 2, 8 at sqrt 3,
    6 at 2 = r1.  Rows of spacing 0.5, range (1, 4), 6 bins: two neighbours at every multiple of 0.5 from 1 = r0 to
    4 = r1, the last bin holding 3.5 and 4; other rows may come within range."""
    if c.build == "lattice":
        return np.array([6, 12, 8, 6]) * c.n1 * c.frames, True
    assert c.build == "rows"
    return np.array([2, 2, 2, 2, 2, 4]) * c.n1 * c.frames, False


def positions(c):
    """``(pos1, pos2 or None, boxes or None)``: float32[frames, n, 3] and float32[frames, 6], seeded by the name."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    p1, p2 = [], []
    for _ in range(c.frames):
        a, b = _frame(c, rng)
        if c.box is not None and c.box[3:] == (90.0, 90.0, 90.0) and c.build != "lattice":
            a, b = np.mod(a, _lengths(c)), (None if b is None else np.mod(b, _lengths(c)))
        p1.append(a)
        p2.append(b)
    pos1 = np.asarray(p1, dtype=np.float32)
    pos2 = None if c.n2 is None else np.asarray(p2, dtype=np.float32)
    boxes = None if c.box is None else np.tile(np.asarray(c.box, dtype=np.float32), (c.frames, 1))
    assert pos1.shape == (c.frames, c.n1, 3)
    return pos1, pos2, boxes


# ------------------------------------------------------------------------------------------------- the table

_SETUP = {"tile-filter": dict(n1=300), "tile-exact": dict(n1=300), "cell-ortho": dict(n1=300),
          "tri-brute": dict(n1=300, box=TRI), "tri-culled": dict(n1=1024, box=TRI)}


def _family_a():
    out = []
    sweeps = (("tile-filter", 300, ORTHO, TILE256_STEPS, TILE256_ATTR), ("tile-filter", 2048, ORTHO, TILE512_STEPS, TILE512_ATTR),
              ("cell-ortho", 300, ORTHO, CELL_STEPS, CELL_48K), ("tri-brute", 300, TRI, TILE256_STEPS, TILE256_ATTR),
              ("tri-culled", 1024, TRI, CELL_STEPS, CELL_48K))
    for family, n, box, steps, line in sweeps:
        bins = sorted({b for top, _ in steps for b in (top, top + 1)} | {line - 1, line})
        for b in bins:
            more = {}
            if family != "cell-ortho" and family != "tri-culled":
                rows = 512 if n >= 2048 and family != "tri-brute" else 256
                more["lds_attribute"] = int(16 * rows + 8 * (b + 1) + 4 * n_hist_of(b, steps)[0] * b > 48 * 1024)
            out.append(case("A", f"{family} N={n} {b} bins", family, n, box=box, bins=b, frames=1 if n >= 1024 else 2,
                            more=more))
    for b in (FORM_BINS[2], FORM_BINS[1]):
        out.append(case("A", f"tile-exact N=300 {b} bins", "tile-exact", 300, bins=b))
    # the replica-poor forms and the global histogram x sets x exclusion x lower range end
    for family in ("tile-filter", "cell-ortho", "tri-brute", "tri-culled"):
        s = _SETUP[family]
        for form, b in FORM_BINS.items():
            for two in (False, True):
                for excl in (None, (1, 1), (3, 3)):
                    for rng in (RANGE, RANGE_LOWER):
                        n2 = (400 if s["n1"] >= 1024 else 200) if two else None
                        name = f"{family} n_hist={form or 'GH'} {'two sets' if two else 'one set'} excl={excl} r0={rng[0]}"
                        out.append(case("A", name, family, s["n1"], n2, box=s.get("box", ORTHO), bins=b, rng=rng,
                                        excl=excl, frames=1 if s["n1"] >= 1024 else 2))
    return out


def _family_b():
    out = []
    for mode in ("tile-exact", "tile-filter"):
        for n in (300, 2048):
            for box in (None, ORTHO):
                for excl in (None, (1, 1)):
                    for b in (60, 5120):
                        out.append(case("B", f"{mode} N={n} {'pbc' if box else 'open'} excl={excl} {b} bins", mode, n,
                                        box=box, excl=excl, bins=b, frames=1 if n >= 2048 else 2))
    for excl in (None, (1, 1)):
        for lower in (False, True):
            for form, kw in (("skip", dict(rng=RANGE_LOWER if lower else RANGE)),
                             ("no-skip", dict(rng=RANGE_NOSKIP_LOWER if lower else RANGE_NOSKIP)),
                             ("gh", dict(rng=RANGE_LOWER if lower else RANGE, bins=5120)),
                             ("tri", dict(rng=RANGE_LOWER if lower else RANGE, box=TRI)),
                             ("tri-gh", dict(rng=RANGE_LOWER if lower else RANGE, box=TRI, bins=5120))):
                tri = "box" in kw
                # (300 particles in three i tiles that each span the box: with the range at 0.38 of the shortest edge
                # tile pairs straddle half a box and take the per-pair image path)
                claims = ("ends", "general") if form == "no-skip" and excl is None and not lower else ("ends",)
                out.append(case("B", f"cell {form} excl={excl} lower={int(lower)}", "tri-culled" if tri else "cell-ortho",
                                1024 if tri else 300, excl=excl, frames=1 if tri else 2, claims=claims, **kw))
    # orthorhombic culling itself: 7 000 particles in a cell seven range ends across
    out.append(case("B", "cell skip, culled: N=7000", "cell-ortho", 7000, box=(52.0, 47.5, 61.25, 90.0, 90.0, 90.0),
                    bins=201, rng=(0.0, 7.5), frames=1, claims=("ends", "culled")))
    for excl in (None, (1, 1)):
        for b in (60, 5120):
            out.append(case("B", f"tri-brute excl={excl} {b} bins", "tri-brute", 300, box=TRI, excl=excl, bins=b))
    return out


def _family_c():
    """One set, two different exclusions: `self` is false, and both copies are built from the same rows.  (With
    different exclusions one of them exceeds 1, so the cell route always materialises the sorted originals:
    lazy_orig = 1 cannot be reached here.)"""
    out = []
    routes = (("tile-exact", 300, ORTHO, None), ("tile-filter", 300, ORTHO, None), ("cell-ortho", 300, ORTHO, None),
              ("tri-brute", 300, TRI, None), ("tri-culled", 1024, TRI, None))
    for family, n, box, _ in routes:
        for excl, dn in (((2, 5), 0), ((1, 3), 0), ((2, 5), 1)):      # dn = 1: not a multiple of either exclusion
            out.append(case("C", f"{family} N={n + dn} excl={excl}", family, n + dn, box=box, excl=excl,
                            frames=1 if n >= 1024 else 2))
    for family in ("tile-filter", "cell-ortho"):
        out.append(case("C", f"{family} N=300 excl=(2, 500) larger than the set", family, 300, excl=(2, 500)))
    return out


def _family_d():
    out = []
    wide = dict(rng=RANGE_NOSKIP, build="gas", claims=())
    for n in (127, 128, 129, 255, 256, 257):
        for family in ("tile-exact", "tile-filter", "cell-ortho"):
            out.append(case("D", f"{family} N={n}", family, n, more={"n1_pad": -(-n // (128 if family == "cell-ortho" else 256))
                                                                      * (128 if family == "cell-ortho" else 256)}, **wide))
    for n in (2047, 2048, 2049):        # IPT 1 | 2; 2048 | 2049: 4 | 5 tiles of 512 rows for one set
        for family in ("tile-exact", "tile-filter", "cell-ortho"):
            T = 128 if family == "cell-ortho" else (512 if n >= 2048 else 256)
            more = {"n1_pad": -(-n // T) * T}
            if family != "cell-ortho":
                more.update(tiles1=-(-n // T), grid_x=-(-(-(-n // T)) // 4))
            out.append(case("D", f"{family} N={n}", family, n, frames=1, more=more, **wide))
    for n in (1023, 1024):              # AUTO on triclinic frames: brute force below 1 024 particles, culled from there
        out.append(case("D", f"triclinic auto N={n}", "tri-culled" if n >= 1024 else "tri-brute", n, box=TRI, frames=1,
                        build="gas", claims=()))
    for n in (1024, 1025):              # 4 | 5 tiles of 256 rows for one set: one | two blocks along x
        more = dict(tiles1=-(-n // 256), grid_x=-(-(-(-n // 256)) // 4))
        out.append(case("D", f"tile-filter N={n}", "tile-filter", n, frames=1, more=more, **wide))
        out.append(case("D", f"tri-brute N={n}", "tri-brute", n, box=TRI, env=BRUTE, frames=1, build="gas", claims=(),
                        more=more))
    # two sets, 8 | 9 j tiles: one | two blocks along x.  (At T = 256 the tile kernel cannot see 9 tiles: from 2 048
    # rows on it takes T = 512; the triclinic tile kernel always has T = 256.)
    for n2 in (4096, 4097):
        more = dict(tiles2=-(-n2 // 512), grid_x=-(-(-(-n2 // 512)) // 8))
        out.append(case("D", f"tile-filter 64 x {n2}", "tile-filter", 64, n2, frames=1, more=more, **wide))
    out.append(case("D", "tile-filter 64 x 2047", "tile-filter", 64, 2047, frames=1, more=dict(tiles2=8, grid_x=1), **wide))
    for n2 in (2048, 2049):
        more = dict(tiles2=-(-n2 // 256), grid_x=-(-(-(-n2 // 256)) // 8))
        out.append(case("D", f"tri-brute 64 x {n2}", "tri-brute", 64, n2, box=TRI, env=BRUTE, frames=1, build="gas",
                        claims=(), rng=RANGE_NOSKIP, more=more))
    # one particle against itself: without exclusion the pair (0, 0) at distance 0 per frame, with it nothing
    for family, box in (("tile-exact", ORTHO), ("tile-filter", ORTHO), ("tile-filter", None), ("cell-ortho", ORTHO),
                        ("tri-brute", TRI)):
        for excl in (None, (1, 1)):
            out.append(case("D", f"{family} N=1 {'pbc' if box else 'open'} excl={excl}", family, 1, box=box, excl=excl,
                            build="gas", claims=("tiny",)))
    far = dict(rng=(0.0, 11.5), build="gas", claims=(), frames=3)
    for family in ("tile-exact", "tile-filter", "cell-ortho"):
        out.append(case("D", f"{family} 1 x 2100", family, 1, 2100, **far))
        out.append(case("D", f"{family} 2100 x 1", family, 2100, 1, **far))
    return out


def _family_f():
    out = []
    cube = (8.0, 8.0, 8.0, 90.0, 90.0, 90.0)
    for family in ("tile-exact", "tile-filter", "cell-ortho"):
        out.append(case("F", f"{family} cubic lattice, r0 = 1 and r1 = 2 are lattice distances", family, 512, box=cube,
                        bins=4, rng=(1.0, 2.0), build="lattice", frames=1,
                        claims=("ends", "lattice") if family == "tile-exact" else ("ends", "lattice", "exact")))
    for family, n, env in (("tri-brute", 1024, BRUTE), ("tri-culled", 1024, {})):
        out.append(case("F", f"{family} rows one bin width apart along a", family, n, box=TRI_ROWS, bins=6, rng=(1.0, 4.0),
                        build="rows", frames=1, env=env,
                        claims=("ends", "lattice") + (("exact",) if family == "tri-culled" else ())))
    for family in FAMILIES:
        s = _SETUP[family]
        for excl in (None, (1, 1)):
            out.append(case("F", f"{family} coincident particles excl={excl}", family, s["n1"] + 50, box=s.get("box", ORTHO),
                            excl=excl, build="coincident", frames=1 if s["n1"] >= 1024 else 2, claims=()))
    return out


CASES = tuple(_family_a() + _family_b() + _family_c() + _family_d() + _family_f())
assert len({c.name for c in CASES}) == len(CASES)

# ---- family E: 32 769 frames (one past the slab and grid-z cap of every route) of 7 particles, a cell per frame
SEAM_FRAMES, SEAM_N, SEAM_BINS, SEAM_RANGE, SEAM_EXCL = 32769, 7, 50, (0.0, 4.0), (1, 1)
# The frames lie in device memory and go through ``accumulate_device``, so that the engine gets ONE run of 32 769 frames
# (the host-buffer entry point would stage it in pieces of its own, none longer than 16 384).  launches: the slabs the
# engine reports for the one-call form — two, 32 768 + 1; the cell route with the sort beside the pair kernel starts a
# run of several slabs with a quarter and a half slab (8 192 + 16 384 + 8 193), the serial route does not.
SeamCase = namedtuple("SeamCase", "name family algo tri env")
SEAM_CASES = (SeamCase("E: tile-exact", 0, "exact", False, {}), SeamCase("E: tile-filter", 1, "filter", False, {}),
              SeamCase("E: cell-ortho", 2, "cell", False, {}),
              SeamCase("E: cell-ortho, serial sort", 2, "cell", False, {"MDX_RDF_SORT_BESIDE": "0"}),
              SeamCase("E: tri-brute", 3, "auto", True, {}))


def seam_inputs(tri):
    """float32[32 769, 7, 3] positions and float32[32 769, 6] cells that change from frame to frame."""
    rng = np.random.default_rng(32769 + int(tri))
    f = np.arange(SEAM_FRAMES)
    L = 9.0 + 1.5 * np.sin(f * 0.37)[:, None] * np.array([1.0, 0.5, -0.7]) + np.array([0.0, 0.4, 0.9])
    angles = np.array([75.0, 80.0, 110.0] if tri else [90.0, 90.0, 90.0])
    boxes = np.concatenate((L, np.broadcast_to(angles, (SEAM_FRAMES, 3))), axis=1).astype(np.float32)
    pos = (rng.uniform(0.0, 1.0, (SEAM_FRAMES, SEAM_N, 3)) * L[:, None, :]).astype(np.float32)
    return pos, boxes


def ortho_restatement(pos, boxes, n_bins, rng, excl):
    """The orthorhombic contract (mdx_rdf.hip, oracle/c/rdf_oracle.c) for one set against itself, vectorised over the
    frames in float64: float32 difference, minimum image with the float32 reciprocal, rsq without contraction,
    min < d <= max, exclusion, numpy.histogram.  Summed over the frames."""
    n = pos.shape[1]
    fd = (pos[:, None, :, :] - pos[:, :, None, :]).astype(np.float64)          # [F, i, j, 3]: x_j - x_i in float32
    box = boxes[:, None, None, :3].astype(np.float64)
    inv = (1.0 / boxes[:, :3].astype(np.float64)).astype(np.float32).astype(np.float64)[:, None, None, :]
    s = inv * fd
    r = np.where(np.abs(s - np.trunc(s)) == 0.5, np.trunc(s) + np.sign(s), np.rint(s))     # C round()
    w = box * (s - r)
    d = np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])
    keep = (d <= rng[1]) & (d > rng[0] - 2.220446049250313e-16)
    if excl is not None:
        i = np.arange(n)
        keep &= (i[:, None] // excl[0] != i[None, :] // excl[1])[None]
    return np.histogram(d[keep], n_bins, rng)[0].astype(np.int64)
