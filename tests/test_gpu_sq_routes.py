"""
Every kernel route of the S(q) engine (csrc/mdx_sq.hip) against the fp64 definition of its outputs, at the edges of
its bookkeeping: wavevector-set shapes of every quad form, column and table shape, the 64- and 512-wavevector blocks,
particle splits with ragged and empty parts, the frame slab loop at both of its caps, the single-chain kernels and
their whole-chain splits, large coordinates, the entry points, the molecule stage, tolerance-free invariants and the
refusals.

Every case sets its stated environment (none, MDX_SQ_NO_QUADS=1, MDX_SQ_NO_COLUMNS=1 or MDX_SQ_NO_LATTICE=1), first
asserts through the plan query (``SqEngine.plan``, mdx_sq_plan) that this is the kernel, row stride, split and slab
it means to test, and compares the UN-NORMALISED result with ``oracle.fourier.ssf_definition_ref``.

Tolerance.  For every output element the reference also returns S = sum_f (n_j |rho_k| + n_k |rho_j|) (n: group
sizes; total mode 2 N |rho|; chains sum_f sum_c 2 n_c |rho_c|) and the tests assert

    |got - ref| <= C * 2^-52 * (1 + phi) * S

with phi = the largest |q . r| of the case, plus the largest |m| on the lattice routes (the tables are filled by a
recurrence of |m| complex products).  S = 0 (empty groups) therefore asks for exact zeros.  C is 8 x the largest
ratio observed over this module on an MI355X, rounded up to a power of two, and at most 4096; sums are formed in a
fixed order, so there is no run-to-run spread and the margin is for other inputs.  Route-against-route comparisons
use the same bound.

Observed |got - ref| / (2^-52 (1 + phi) S), largest over the module:

    route          ratio     C       from
    general        0.188     2       groups (5, 1) on the 12 x 4 x 8 grid, 6 frames (case A)
    tables         0.114     1       the same case
    columns        0.112     1       the same case
    quads          0.113     1       the same case
    chain-sincos   0.0079    0.125   one chain of 2 053 points at the 4^3 grid (case E)
    chain-quads    0.025     0.25    32 771 frames of two chains of 2 points at the 4^3 grid (case D)

(route against route at most 0.18: quads against general on the 12^3 grid, groups (5, 1).  The particle-split cases
stay below 0.1, the slab cases below 0.03.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sq_cases as sc  # noqa: E402
from mdhelper_amd import _core  # noqa: E402
from mdhelper_amd.io import TrajectoryFile  # noqa: E402
from oracle import fourier as of  # noqa: E402
from trajfiles import write_amber_netcdf  # noqa: E402

EPS = 2.0 ** -52
C_MAX = 4096.0
C = {"general": 2.0, "tables": 1.0, "columns": 1.0, "quads": 1.0, "chain-sincos": 0.125, "chain-quads": 0.25}
OBSERVED = {}            # route -> (largest ratio seen, the case that gave it)
LATTICE = {"tables", "columns", "quads", "chain-quads"}
TOTAL = ((None, None),)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    assert max(C.values()) <= C_MAX
    yield
    for route, (r, label) in sorted(OBSERVED.items()):
        print(f"\nSQ-RATIO {route:12s} {r:.4g} (C = {C[route]:g}) from {label}", end="")
    print()


def feed(eng, frames, cuts=None):
    """The frames whole, or cut into calls of ``cuts`` frames."""
    if cuts is None:
        eng.accumulate(frames)
        return
    assert sum(cuts) == len(frames)
    at = 0
    for c in cuts:
        eng.accumulate(frames[at:at + c])
        at += c


def engine(monkeypatch, ws, route, groups, pairs, n_frames, want=None):
    """An engine on ``route`` — after the plan query has confirmed that the set takes it in that environment for a
    call of ``n_frames`` frames (``want``: further plan fields the case is about)."""
    env = dict(sc.routes_of(ws))[route]
    sc.set_env(monkeypatch, env)
    p = _core.SqEngine.plan(ws.q, groups, n_frames)
    assert _core.SqEngine.ROUTES[p["route"]] == route, (ws.name, route, p)
    if not env:
        assert p["regular_stride"] == ws.stride, (ws.name, p)
    for key, value in (want or {}).items():
        assert p[key] == value, (ws.name, route, key, p)
    return _core.SqEngine(ws.q, groups, pairs)


def chain_engine(monkeypatch, ws, env, n_points, length, n_frames, want):
    """A single-chain engine after the plan query has confirmed the chain kernel (0 sincos, 3 quads) and ``want``."""
    sc.set_env(monkeypatch, env)
    p = _core.SqEngine.plan(ws.q, (n_points,), n_frames, length)
    for key, value in want.items():
        assert p[key] == value, (ws.name, key, p)
    eng = _core.SqEngine(ws.q, (n_points,), TOTAL)
    eng.set_chains(length)
    return eng, sc.CHAIN_ROUTES[p["route"]], p


def run(monkeypatch, ws, route, groups, pairs, frames, cuts=None, want=None):
    eng = engine(monkeypatch, ws, route, groups, pairs, max(cuts) if cuts else len(frames), want)
    try:
        feed(eng, frames, cuts)
        return eng.result()
    finally:
        eng.close()


def _ratio(got, want, scale, phi):
    """Largest |got - want| / (eps (1 + phi) S); where S = 0 the values must be equal."""
    unit = EPS * (1.0 + phi) * scale
    diff = np.abs(got - want)
    exact = unit == 0
    assert np.all(diff[exact] == 0), "nonzero where the definition gives an exact zero"
    return float((diff[~exact] / unit[~exact]).max(initial=0.0))


def check(label, route, ws, got, ref, other=None, other_route=None):
    """``got`` of ``route`` against the reference (or against another route's result, same bound)."""
    assert got.shape == ref["ssf"].shape, (label, got.shape)
    phi = ref["phi_max"] + (ws.m_max if {route, other_route or route} & LATTICE else 0)
    bound = max(C[route], C[other_route or route])
    r = _ratio(got, ref["ssf"] if other is None else other, ref["S"], phi)
    if other is None and r > OBSERVED.get(route, (-1.0, ""))[0]:
        OBSERVED[route] = (r, label)
    print(f"{label} | {route}{' vs ' + other_route if other_route else ''} | ratio {r:.4g}")
    assert r <= bound, (label, route, other_route, r)


_REFS = {}


def reference(key, frames, groups, pairs, q, chain_length=0):
    """Computed once per case and shared between the routes; never modified."""
    if key not in _REFS:
        ref = of.ssf_definition_ref(frames, sc.offsets_of(groups), pairs, q, chain_length)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("groups", sc.A_GROUPS, ids=str)
@pytest.mark.parametrize("ws", sc.A_SETS, ids=lambda ws: ws.name)
def test_a_set_shapes_on_every_route(ws, groups, monkeypatch):
    """Every quad form, both column block sizes, both table tiles and the detector's refusals, each on every route
    the set can take; groups that are no multiple of any tile, and smaller than one."""
    frames = sc.walk(sc.A_FRAMES, sum(groups), sc.LENGTHS, 11)
    pairs = sc.pairs_of(2, "partial")
    ref = reference(("A", ws.name, groups), frames, groups, pairs, ws.q)
    out = {}
    for route, _ in sc.routes_of(ws):
        out[route] = run(monkeypatch, ws, route, groups, pairs, frames)
        check(f"A {ws.name} {groups}", route, ws, out[route], ref)
    first = sc.ROUTES[ws.route]
    for route in ws.lower:
        check(f"A {ws.name} {groups}", first, ws, out[first], ref, other=out[route], other_route=route)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("ws", sc.B_SETS, ids=lambda ws: ws.name)
def test_b_wavevector_count_edges(ws, monkeypatch):
    """n_q of 1, 63, 64, 65 (the 64 wavevectors of a sq_pair_kernel block) and 511, 512, 513 (the 512 of a density
    block) on the general kernel; ONE wavevector is a lattice and takes the tables by default."""
    frames = sc.walk(sc.B_FRAMES, sum(sc.B_GROUPS), 33.0, 17)
    pairs = sc.pairs_of(2, "partial")
    ref = reference(("B", ws.name), frames, sc.B_GROUPS, pairs, ws.q)
    for route, _ in sc.routes_of(ws):
        want = {"blocks": -(-len(ws.q) // 512)}
        check(f"B {ws.name}", route, ws, run(monkeypatch, ws, route, sc.B_GROUPS, pairs, frames, want=want), ref)


def test_b_tables_with_two_wavevector_blocks(monkeypatch):
    ws = sc.B_TABLES_SET
    frames = sc.walk(sc.B_FRAMES, sum(sc.B_GROUPS), sc.LENGTHS, 19)
    pairs = sc.pairs_of(2, "partial")
    ref = reference("B tables", frames, sc.B_GROUPS, pairs, ws.q)
    got = run(monkeypatch, ws, "tables", sc.B_GROUPS, pairs, frames, want={"blocks": 2})
    check(f"B {ws.name}", "tables", ws, got, ref)


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("route_set", sc.C_ROUTE_SETS, ids=lambda rs: rs[0])
@pytest.mark.parametrize("case", sc.C_CASES, ids=lambda c: c[0])
def test_c_particle_splits(case, route_set, monkeypatch):
    """rho in 2 and 4 particle parts, summed in a fixed order by sq_pair_kernel: exact and ragged parts, a group
    smaller than the parts (2 + 1, 1 + 0) and an empty one beside the group that causes the split."""
    name, groups, mode, parts, ragged = case
    route, ws = route_set
    pairs = sc.pairs_of(len(groups), mode)
    assert (-(-max(groups) // parts) * parts != max(groups)) == ragged
    frames = sc.walk(sc.C_FRAMES, sum(groups), 33.0, 23)
    ref = reference(("C", name, ws.name), frames, groups, pairs, ws.q)
    got = run(monkeypatch, ws, route, groups, pairs, frames, want={"n_split": parts})
    check(f"C {name}", route, ws, got, ref)
    if len(groups) > 1:
        for p, (j, k) in enumerate(pairs):
            assert bool(got[p].any()) == (2 not in (j, k))          # the empty group's pairs: exact zeros


# ------------------------------------------------------------------------------------------------ D
def _resident(eng, frames):
    """All frames in HBM, one accumulate_device call: the engine's own slab loop cuts them."""
    d_frames = _core.DeviceArray.from_host(frames)
    try:
        eng.accumulate_device(d_frames.ptr, frames.shape[1], len(frames))
        eng.synchronize()
        return eng.result()
    finally:
        d_frames.free()
        eng.close()


@pytest.mark.parametrize("route", [r for r, _ in sc.routes_of(sc.D_COLUMN)])
def test_d_frame_cap_cuts_the_call_in_two_slabs(route, monkeypatch):
    """32 771 frames in one call: a slab of 32 768 and one of 3 — the second += into the sums and the frame offset of
    the second slab's positions."""
    ws, pairs = sc.D_COLUMN, sc.pairs_of(2, "partial")
    frames = sc.walk(sc.D_FRAMES, sum(sc.D_GROUPS), 33.0, 29)
    ref = reference("D frames", frames, sc.D_GROUPS, pairs, ws.q)
    eng = engine(monkeypatch, ws, route, sc.D_GROUPS, pairs, sc.D_FRAMES, {"slab_frames": 32768})
    check("D frame cap", route, ws, _resident(eng, frames), ref)
    # the second slab matters: without its three frames the result misses the bound by orders of magnitude
    short = reference("D frames, first slab", frames[:32768], sc.D_GROUPS, pairs, ws.q)
    assert _ratio(short["ssf"], ref["ssf"], ref["S"], ref["phi_max"]) > 1e6 * C_MAX


@pytest.mark.parametrize("route", [r for r, _ in sc.routes_of(sc.D_BYTE_SET)])
def test_d_byte_cap_cuts_the_call_in_two_slabs(route, monkeypatch):
    """32 768 wavevectors: 512 KiB of partial sums per frame, slabs of 1 024 frames; 1 027 frames of 2 particles.
    Also the quads kernel with ONE copy per item, in four blocks."""
    ws, groups = sc.D_BYTE_SET, (2,)
    frames = sc.walk(sc.D_BYTE_FRAMES, 2, 33.0, 31)
    at = sc.D_BYTE_CHECKED
    ref = reference("D bytes", frames, groups, TOTAL, ws.q[at])
    want = {"slab_frames": sc.D_BYTE_SLAB}
    if route == "quads":
        want.update(n_sub=1, blocks=4)
    got = _resident(engine(monkeypatch, ws, route, groups, TOTAL, sc.D_BYTE_FRAMES, want), frames)
    check("D byte cap", route, ws, got[:, at], ref)
    # every other element against plain float64, |rho|^2 = 2 + 2 cos(q . (r_1 - r_2)): errors of 1e-9 of the
    # largest value, far below what a slab error (three frames of 1 027 lost, or read at a wrong offset) makes
    d = frames[:, 0].astype(np.float64) - frames[:, 1].astype(np.float64)
    plain = np.zeros(len(ws.q))
    for f0 in range(0, len(d), 64):
        plain += (2.0 + 2.0 * np.cos(d[f0:f0 + 64] @ ws.q.T)).sum(axis=0)
    assert np.abs(got[0] - plain).max() <= 1e-9 * 4 * sc.D_BYTE_FRAMES


@pytest.mark.parametrize("ws, route", ((sc.D_COLUMN, 0), (sc.D_CHAIN_QUADS_SET, 3)), ids=("sincos", "quads"))
def test_d_frame_cap_in_chain_mode(ws, route, monkeypatch):
    n, length = sc.D_CHAIN_POINTS, sc.D_CHAIN_LENGTH
    frames = sc.walk(sc.D_FRAMES, n, 33.0, 37)
    ref = reference(("D chains", ws.name), frames, (n,), TOTAL, ws.q, length)
    eng, name, _ = chain_engine(monkeypatch, ws, {}, n, length, sc.D_FRAMES, {"route": route, "slab_frames": 32768})
    check("D frame cap, chains", name, ws, _resident(eng, frames), ref)


# ------------------------------------------------------------------------------------------------ E
def _prime_above(n):
    n += 1
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


@pytest.mark.parametrize("form", sc.E_FORMS, ids=lambda f: f[0])
def test_e_single_chains(form, monkeypatch):
    """Chain lengths around the planned tile t of each chain kernel — 1, t - 1, t, t + 1, a prime above 2 t, the
    whole system as one chain — and whole-chain splits: 3 chains in parts of 2 + 1, 8 chains in 4 parts."""
    name, ws, env, route, stride = form
    t = sc.E_TILES[name] if route == 3 else sc.E_SINCOS_TILE
    want = {"route": route, "regular_stride": stride, "tile": t}
    zero = np.flatnonzero(~ws.q.any(axis=1))
    cases = [(f"length {n}", 7 if n == 1 else 3, n, want) for n in (1, t - 1, t, t + 1, _prime_above(2 * t))]
    cases.append(("one chain", 1, 2 * t + 5, want))
    cases += [(label, n_chains, n, dict(want, n_split=parts, chains_per_part=per))
              for label, n_chains, n, parts, per in sc.E_SPLITS]
    for label, n_chains, length, plan_wants in cases:
        n = n_chains * length
        frames = sc.walk(sc.E_FRAMES, n + 3, sc.LENGTHS, 41 + length)              # three rows beyond the chains
        ref = reference(("E", ws.name, label, length), frames[:, :n], (n,), TOTAL, ws.q, length)
        eng, kernel, _ = chain_engine(monkeypatch, ws, env, n, length, sc.E_FRAMES, plan_wants)
        try:
            eng.accumulate(frames)
            got = eng.result()
        finally:
            eng.close()
        check(f"E {name}, {label}", kernel, ws, got, ref)
        # S_chain(q = 0) = F sum_c n_c^2, exactly
        assert np.array_equal(got[0, zero], np.full(len(zero), float(sc.E_FRAMES * n_chains * length ** 2)))


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("ws", (sc.F_SET, sc.F_RANDOM), ids=lambda ws: ws.name)
def test_f_large_unwrapped_coordinates(ws, monkeypatch):
    """An unwrapped walk 40 box lengths from the origin: phases of several thousand radians, grid up to m = 6."""
    groups = (150, 75)
    frames = sc.walk(3, sum(groups), 33.0, 43, step=0.4, centre=40 * 33.0)
    pairs = sc.pairs_of(2, "partial")
    ref = reference(("F", ws.name), frames, groups, pairs, ws.q)
    assert ref["phi_max"] > 4000.0
    out = {route: run(monkeypatch, ws, route, groups, pairs, frames) for route, _ in sc.routes_of(ws)}
    first = sc.ROUTES[ws.route]
    for route in out:
        check(f"F {ws.name}", route, ws, out[route], ref)
        if route != first:
            check(f"F {ws.name}", first, ws, out[first], ref, other=out[route], other_route=route)


# ------------------------------------------------------------------------------------------------ G
G_SET, G_GROUPS, G_CUTS = sc.C_COLUMNS_SET, (41, 22), (1, 1, 3, 7, 11)


@pytest.mark.parametrize("route", sc.ROUTES)
def test_g_entry_points(route, monkeypatch, tmp_path):
    """Host memory whole and in calls of (1, 1, 3, 7, 11) frames, HBM, and a trajectory file (once through a shuffled
    particle index), all with rows beyond the groups' span."""
    ws, groups, cuts = G_SET, G_GROUPS, G_CUTS
    n, extra = sum(groups), 7
    frames = sc.walk(sum(cuts), n, 33.0, 47)
    wide = np.concatenate([frames, sc.walk(sum(cuts), extra, 900.0, 53)], axis=1)       # n > n_total
    pairs = sc.pairs_of(2, "partial")
    ref = reference("G", frames, groups, pairs, ws.q)
    check("G host, whole", route, ws, run(monkeypatch, ws, route, groups, pairs, wide), ref)
    check("G host, cut", route, ws, run(monkeypatch, ws, route, groups, pairs, wide, cuts), ref)

    eng = engine(monkeypatch, ws, route, groups, pairs, len(wide))
    check("G device", route, ws, _resident(eng, wide), ref)

    # the file holds more particles in another order; the index picks the groups' rows back out of it
    rng = np.random.default_rng(59)
    n_file = n + extra
    index = rng.permutation(n_file)[:n].astype(np.int32)
    assert np.any(np.diff(index) < 0)
    stored = wide.copy()
    stored[:, index] = frames
    for name, data, idx in (("file", wide, None), ("file + index", stored, index)):
        path = tmp_path / (name.replace(" + ", "_") + ".nc")
        write_amber_netcdf(path, data, (33.0, 33.0, 33.0))
        t = TrajectoryFile(path)
        eng = engine(monkeypatch, ws, route, groups, pairs, len(data))
        try:
            eng.accumulate_traj(t, np.arange(len(data)), idx)
            check(f"G {name}", route, ws, eng.result(), ref)
        finally:
            eng.close()
            t.close()


@pytest.mark.parametrize("route", sc.ROUTES)
def test_g_molecule_stage(route, monkeypatch):
    """Molecules of 1 to 4 rows with unequal masses: the Fourier sums run over the float32 centres of mass."""
    ws, groups = G_SET, (29, 16)                        # molecules per group
    sizes = np.resize([1, 2, 3, 4], sum(groups) + 2)    # two molecules beyond the groups' span
    mol_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    masses = np.random.default_rng(61).uniform(1.0, 30.0, int(mol_offsets[-1]))
    atoms = sc.walk(9, int(mol_offsets[-1]), 33.0, 67)
    centres = of.molecule_centres_ref(atoms, mol_offsets, masses)
    pairs = sc.pairs_of(2, "partial")
    ref = reference("G molecules", centres, groups, pairs, ws.q)
    for cuts in (None, (2, 7)):
        eng = engine(monkeypatch, ws, route, groups, pairs, 9)
        try:
            eng.set_grouping(mol_offsets, masses)
            feed(eng, atoms, cuts)
            check(f"G molecules {cuts}", route, ws, eng.result(), ref)
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------ H
@pytest.mark.parametrize("route", sc.ROUTES)
def test_h_invariants_without_tolerance(route, monkeypatch):
    ws, groups, n_frames = G_SET, (333, 0, 130), 5
    frames = sc.walk(n_frames, sum(groups), 33.0, 71)
    pairs = ((0, 2), (2, 0), (0, 0), (1, 1), (0, 1), (1, 2), (2, 2))
    eng = engine(monkeypatch, ws, route, groups, pairs, n_frames)
    try:
        eng.accumulate(frames)
        first = eng.result()
        assert np.array_equal(first, eng.result())
        eng.reset()
        assert not eng.result().any()
        eng.accumulate(frames)
        assert np.array_equal(first, eng.result())                  # two runs of one engine: the same bits
    finally:
        eng.close()
    check("H pairs", route, ws, first, reference("H", frames, groups, pairs, ws.q))
    assert np.array_equal(first[0], first[1])                       # (2, 0) gives the bits of (0, 2)
    assert not first[3].any() and not first[4].any() and not first[5].any()       # the empty group's pairs
    zero = np.flatnonzero(~ws.q.any(axis=1))
    assert len(zero) == 1                                           # q = 0: F n_j n_k, twice that for j != k
    want = [2 * 333 * 130, 2 * 333 * 130, 333 * 333, 0, 0, 0, 130 * 130]
    assert np.array_equal(first[:, zero[0]], np.array(want, dtype=np.float64) * n_frames)
    # one group: the total mode gives the bits of the pair (0, 0)
    single = run(monkeypatch, ws, route, (463,), ((0, 0),), frames)
    total = run(monkeypatch, ws, route, (463,), TOTAL, frames)
    assert np.array_equal(single, total)


def test_h_a_wavevector_listed_twice(monkeypatch):
    """sq_build_quad_blocks declines a set that lists a wavevector twice: general quad items, where both copies are
    slots of their own — and get the same bits, on every route."""
    ws, groups = sc.H_TWICE, (70, 31)
    a, b = sc.H_TWICE_AT
    frames = sc.walk(4, sum(groups), sc.LENGTHS, 73)
    pairs = sc.pairs_of(2, "partial")
    ref = reference("H twice", frames, groups, pairs, ws.q)
    for route, _ in sc.routes_of(ws):
        got = run(monkeypatch, ws, route, groups, pairs, frames)
        check("H twice", route, ws, got, ref)
        assert np.array_equal(got[:, a], got[:, b]) and got[:, a].all()


# ------------------------------------------------------------------------------------------------ I
def test_i_refusals_leave_the_sums_unchanged(monkeypatch):
    """Argument checks that return before any launch: the library's invalid-value error, nothing accumulated."""
    ws = G_SET
    frames = sc.walk(4, 12, 33.0, 79)
    eng = engine(monkeypatch, ws, "quads", (12,), TOTAL, 2)
    try:
        with pytest.raises(ValueError, match="whole number of chains"):
            eng.set_chains(5)                                       # 12 points are no chains of 5
        eng.accumulate(frames[:2])
        before = eng.result()
        assert before.any()
        with pytest.raises(ValueError, match="before the first frame"):
            eng.set_chains(3)
        with pytest.raises(ValueError, match="the groups span"):
            eng.accumulate(frames[2:, :11])                         # fewer particles than the groups span
        d_frames = _core.DeviceArray.from_host(frames[2:, :11])
        with pytest.raises(ValueError, match="the groups span"):
            eng.accumulate_device(d_frames.ptr, 11, 2)
        d_frames.free()
        assert np.array_equal(before, eng.result())
        # the engine goes on as if nothing had happened — in the normal mode
        eng.accumulate(frames[2:])
        check("I continued", "quads", ws, eng.result(), reference("I", frames, (12,), TOTAL, ws.q))
    finally:
        eng.close()
    eng = engine(monkeypatch, ws, "quads", (7, 5), sc.pairs_of(2, "partial"), 2)
    try:
        with pytest.raises(ValueError, match="one group over all points"):
            eng.set_chains(3)
        eng.accumulate(frames[:2])
        check("I two groups", "quads", ws, eng.result(),
              reference("I two", frames[:2], (7, 5), sc.pairs_of(2, "partial"), ws.q))
    finally:
        eng.close()
