"""
Every kernel route of the ISF engine (csrc/mdx_isf.hip) against the fp64 definition of its outputs, at the edges of
its bookkeeping: ring and chunk arithmetic, wavevector-set shapes of every quad row stride, the 512-wavevector block,
ragged particle splits, pair lists and spans, large coordinates, the three entry points, the molecule stage,
tolerance-free invariants and the refusal of a changed row count.

Every case builds its engine under a stated environment (default, MDX_ISF_NO_QUADS=1 or MDX_SQ_NO_LATTICE=1), first
asserts through the plan query (``IsfEngine.plan``, mdx_isf_plan) that this is the kernel it means to test, and
compares the UN-NORMALISED results with ``oracle.fourier.isf_definition_ref``: no ring, extended precision.

Tolerance.  For every output element the reference also returns S — ``iisf``: slot size x frame pairs at the lag;
``cisf``: sum_f |rho_a(f - lag)| |rho_b(f)|, both orderings for a cross pair — and the tests assert

    |got - ref| <= C * 2^-52 * (1 + phi) * S

with phi = the largest |q . r| of the case, plus the largest |m| on the lattice routes (the tables are filled by a
recurrence of |m| complex products, each adding a rounding error to the one of the phase).  S = 0 (lags beyond the
frames, empty groups, slots without a diagonal pair) therefore asks for exact zeros.  C is 8 x the largest ratio
observed over this module on an MI355X, rounded up to a power of two; sums are formed in a fixed order, so there is
no run-to-run spread and the margin is for other inputs.  Route-against-route comparisons use the same bound.

Observed |got - ref| / (2^-52 (1 + phi) S), largest over the module:

    route     cisf     iisf      C
    general   5.19     0.23      64
    tables    1.84     0.21      16
    quads     1.80     0.057     16

(the largest: 23 frames of 8 particles at 7 off-lattice wavevectors; the lattice routes: a group of 5 and a group of
1 on the 12 x 4 x 8 grid; route against route at most 2.1)
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import isf_cases as ic  # noqa: E402
from mdhelper_amd import _core, _lib  # noqa: E402
from mdhelper_amd.io import TrajectoryFile  # noqa: E402
from oracle import fourier as of  # noqa: E402
from trajfiles import write_amber_netcdf  # noqa: E402

EPS = 2.0 ** -52
C = {"general": 64.0, "tables": 16.0, "quads": 16.0}        # <= 4096 each: see the docstring
OBSERVED = {}            # (route, "cisf" | "iisf") -> largest ratio seen


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for (route, what), r in sorted(OBSERVED.items()):
        print(f"\nISF-RATIO {route:8s} {what} {r:.4g} (C = {C[route]:g})", end="")
    print()


def walk(n_frames, n, length, seed, step=0.25, centre=None):
    """float32[F, n, 3]: a random walk, wrapped into the box, or unwrapped around ``centre``."""
    rng = np.random.default_rng(seed)
    steps = np.cumsum(rng.normal(0.0, step, (n_frames, n, 3)), axis=0)
    if centre is None:
        return np.mod(rng.uniform(0, length, (1, n, 3)) + steps, length).astype(np.float32)
    return (centre + rng.uniform(-length, length, (1, n, 3)) + steps).astype(np.float32)


def offsets_of(groups):
    return np.concatenate(([0], np.cumsum(groups))).astype(np.int64)


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


def engine(monkeypatch, ws, route, groups, pairs, n_lags, incoherent=True):
    """An engine on ``route`` — after the plan query has confirmed that the set takes it in that environment."""
    env = dict(ic.routes_of(ws))[route]
    ic.set_env(monkeypatch, env)
    p = _core.IsfEngine.plan(ws.q, groups, pairs, n_lags)
    assert _core.IsfEngine.ROUTES[p["route"]] == route, (ws.name, route, p)
    if route == "quads" and not env:
        assert p["regular_stride"] == ws.stride, (ws.name, p)
    return _core.IsfEngine(ws.q, groups, pairs, n_lags, incoherent)


def run(monkeypatch, ws, route, groups, pairs, n_lags, frames, cuts=None):
    eng = engine(monkeypatch, ws, route, groups, pairs, n_lags)
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
    """``got`` of ``route`` against the reference (or against another route's results, same bound)."""
    phi = ref["phi_max"] + (ws.m_max if {route, other_route or route} != {"general"} else 0)
    bound = max(C[route], C[other_route or route])
    for what, g, w in (("cisf", got[0], ref["cisf"] if other is None else other[0]),
                       ("iisf", got[1], ref["iisf"] if other is None else other[1])):
        if g is None:
            continue
        r = _ratio(g, w, ref["S_" + what], phi)
        if other is None:
            OBSERVED[(route, what)] = max(OBSERVED.get((route, what), 0.0), r)
        print(f"{label} | {route}{' vs ' + other_route if other_route else ''} | {what} ratio {r:.4g}")
        assert r <= bound, (label, route, other_route, what, r)


_REFS = {}


def reference(key, frames, groups, pairs, ws, n_lags):
    """Computed once per case and shared between the routes; never modified."""
    if key not in _REFS:
        ref = of.isf_definition_ref(frames, offsets_of(groups), pairs, ws.q, n_lags)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("n_lags", ic.A_LAGS)
def test_a_ring_and_chunk_bookkeeping(n_lags, monkeypatch):
    """Groups (5, 3), 23 frames, fed whole and in calls of (1, 1, 3, 7, 11) — with 5 lags the last call meets
    ring_slots - slot0 < n_lags at slot 7 of 10.  n_lags of 1, 2 and more than the frames; lags >= F exactly zero."""
    frames = walk(ic.A_FRAMES, sum(ic.A_GROUPS), 33.0, 3)
    pairs = ic.pairs_of(2, "partial")
    for ws in ic.A_SETS:
        ref = reference(("A", ws.name, n_lags), frames, ic.A_GROUPS, pairs, ws, n_lags)
        for route, _ in ic.routes_of(ws):
            whole = run(monkeypatch, ws, route, ic.A_GROUPS, pairs, n_lags, frames)
            cut = run(monkeypatch, ws, route, ic.A_GROUPS, pairs, n_lags, frames, ic.A_CUTS)
            for label, got in (("whole", whole), ("cut", cut)):
                check(f"A {ws.name} {n_lags} lags {label}", route, ws, got, ref)
                assert not got[0][ic.A_FRAMES:].any() and not got[1][ic.A_FRAMES:].any()
                assert got[0][:ic.A_FRAMES].any() and got[1][:ic.A_FRAMES].any()
    # total mode through the same feeds
    ws, pairs = ic.A_SETS[1], ic.pairs_of(2, None)
    ref = reference(("A total", n_lags), frames, ic.A_GROUPS, pairs, ws, n_lags)
    check(f"A total {n_lags} lags", "general", ws,
          run(monkeypatch, ws, "general", ic.A_GROUPS, pairs, n_lags, frames, ic.A_CUTS), ref)


@pytest.mark.parametrize("n_lags", (2, 5))
def test_a_coherent_only_engine(n_lags, monkeypatch):
    """Without the incoherent part the new frames go through the position stage, not the ring; result() with an
    iisf buffer is refused."""
    frames = walk(ic.A_FRAMES, sum(ic.A_GROUPS), 33.0, 3)
    pairs = ic.pairs_of(2, "partial")
    for ws in ic.A_SETS:
        ref = reference(("A", ws.name, n_lags), frames, ic.A_GROUPS, pairs, ws, n_lags)
        route = ic.ROUTES[ws.route]
        eng = engine(monkeypatch, ws, route, ic.A_GROUPS, pairs, n_lags, incoherent=False)
        try:
            feed(eng, frames, ic.A_CUTS)
            cisf, iisf = eng.result()
            assert iisf is None
            check(f"A coherent only {ws.name}", route, ws, (cisf, None), ref)
            buf = np.zeros((n_lags, 2, len(ws.q)))
            with pytest.raises(RuntimeError, match="without the incoherent part"):
                _lib.check(_lib.lib().mdx_isf_result(eng.handle, cisf.ctypes.data_as(ctypes.c_void_p),
                                                     buf.ctypes.data_as(ctypes.c_void_p)))
            assert not buf.any()
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("groups", ic.B_GROUPS, ids=str)
@pytest.mark.parametrize("ws", ic.B_SETS, ids=lambda ws: ws.name)
def test_b_wavevector_set_shapes(ws, groups, monkeypatch):
    """One set per reachable row stride of the regular quads kernel, general items, and the sets the planner sends
    to the tables and to the general kernels; groups that are no multiple of any tile, and smaller than one."""
    frames = walk(ic.B_FRAMES, sum(groups), ic.LENGTHS, 11)
    pairs = ic.pairs_of(2, "partial")
    ref = reference(("B", ws.name, groups), frames, groups, pairs, ws, ic.B_LAGS)
    out = {}
    for route, _ in ic.routes_of(ws):
        out[route] = run(monkeypatch, ws, route, groups, pairs, ic.B_LAGS, frames)
        check(f"B {ws.name} {groups}", route, ws, out[route], ref)
    first = ic.ROUTES[ws.route]
    for route in out:
        if route != first:
            check(f"B {ws.name} {groups}", first, ws, out[first], ref, other=out[route], other_route=route)


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("ws", ic.C_SETS, ids=lambda ws: ws.name)
def test_c_wavevector_count_edges(ws, monkeypatch):
    """n_q of 1, 511 and 513 on the general kernels (512 wavevectors per block).  Off-lattice sets of 511 and 513
    take them without a switch; ONE wavevector is always a lattice (m = 1 on every axis), so the planner gives it
    the tables: it runs there by default, and on the general kernels through MDX_SQ_NO_LATTICE."""
    frames = walk(ic.C_FRAMES, sum(ic.C_GROUPS), 33.0, 17)
    pairs = ic.pairs_of(2, "partial")
    ic.set_env(monkeypatch, {})
    assert _core.IsfEngine.plan(ws.q, ic.C_GROUPS, pairs, ic.C_LAGS)["route"] == (0 if len(ws.q) > 1 else 1)
    ws = ws._replace(m_max=1 if len(ws.q) == 1 else 0)
    ref = reference(("C", ws.name), frames, ic.C_GROUPS, pairs, ws, ic.C_LAGS)
    for route, _ in ic.routes_of(ws):
        check(f"C {ws.name}", route, ws, run(monkeypatch, ws, route, ic.C_GROUPS, pairs, ic.C_LAGS, frames), ref)


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("route", ic.ROUTES)
@pytest.mark.parametrize("case", ic.D_CASES, ids=lambda c: c[0])
def test_d_ragged_particle_splits(case, route, monkeypatch):
    """rho in 2 and 4 particle parts through the merge kernel, the incoherent sums in parts through the reduce
    kernel, the last part shorter than per = ceil(range / parts)."""
    name, groups, mode, rho_split = case
    ws, pairs = ic.SMALL_GRID, ic.pairs_of(len(groups), mode)
    frames = walk(ic.D_FRAMES, sum(groups), 33.0, 23)
    ic.set_env(monkeypatch, dict(ic.routes_of(ws))[route])
    p = _core.IsfEngine.plan(ws.q, groups, pairs, ic.D_LAGS)
    assert p["rho_split"] == rho_split and p["incoherent_split"] > 1, p
    biggest = max(groups) if mode else sum(groups)
    assert biggest % p["rho_split"] and biggest % p["incoherent_split"]
    ref = reference(("D", name), frames, groups, pairs, ws, ic.D_LAGS)
    check(f"D {name}", route, ws, run(monkeypatch, ws, route, groups, pairs, ic.D_LAGS, frames), ref)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("route", ic.ROUTES)
def test_e_pair_lists_and_spans(route, monkeypatch):
    ws, n_lags = ic.SMALL_GRID, 3
    groups = (37, 12, 21)
    frames = walk(6, sum(groups), 33.0, 29)

    # "pair" mode on three groups: no diagonal pair, every incoherent slot exactly zero
    pairs = ic.pairs_of(3, "pair")
    assert pairs == ((0, 2),)
    ref = reference("E pair", frames, groups, pairs, ws, n_lags)
    got = run(monkeypatch, ws, route, groups, pairs, n_lags, frames)
    check("E pair mode", route, ws, got, ref)
    assert got[1].shape == (n_lags, 3, len(ws.q)) and not got[1].any() and got[0].any()

    # a custom list: only the slot of group 1 is filled
    pairs = ((1, 1), (0, 2))
    ref = reference("E custom", frames, groups, pairs, ws, n_lags)
    got = run(monkeypatch, ws, route, groups, pairs, n_lags, frames)
    check("E custom list", route, ws, got, ref)
    assert not got[1][:, 0].any() and not got[1][:, 2].any() and got[1][:, 1].all()

    # an empty group between two others
    hollow, pairs = (37, 0, 21), ic.pairs_of(3, "partial")
    hollow_frames = frames[:, :sum(hollow)]
    ref = reference("E hollow", hollow_frames, hollow, pairs, ws, n_lags)
    got = run(monkeypatch, ws, route, hollow, pairs, n_lags, hollow_frames)
    check("E empty group", route, ws, got, ref)
    assert not got[1][:, 1].any() and got[1][:, 0].all() and got[1][:, 2].all()
    for p, (j, k) in enumerate(pairs):
        assert bool(got[0][:, p].any()) == (1 not in (j, k))

    # 7 rows beyond the groups' span, filled with other numbers: nothing changes, to the bit
    pairs = ic.pairs_of(3, "partial")
    plain = run(monkeypatch, ws, route, groups, pairs, n_lags, frames, (2, 4))
    wide = np.concatenate([frames, walk(6, 7, 900.0, 31)], axis=1)
    padded = run(monkeypatch, ws, route, groups, pairs, n_lags, wide, (2, 4))
    assert np.array_equal(plain[0], padded[0]) and np.array_equal(plain[1], padded[1])
    check("E rows beyond the span", route, ws, padded, reference("E partial", frames, groups, pairs, ws, n_lags))


# ------------------------------------------------------------------------------------------------ F
def test_f_large_unwrapped_coordinates(monkeypatch):
    """An unwrapped walk around 1500 in a box of 33: phases of order 10^3, grid up to m = 6."""
    ws, groups, n_lags = ic.F_SET, (150, 75), 4
    frames = walk(6, sum(groups), 33.0, 37, step=0.4, centre=1500.0)
    pairs = ic.pairs_of(2, "partial")
    ref = reference("F", frames, groups, pairs, ws, n_lags)
    assert ref["phi_max"] > 1000.0
    out = {route: run(monkeypatch, ws, route, groups, pairs, n_lags, frames) for route in ic.ROUTES}
    for route in ic.ROUTES:
        check("F", route, ws, out[route], ref)
    for route in ("tables", "general"):
        check("F", "quads", ws, out["quads"], ref, other=out[route], other_route=route)


# ------------------------------------------------------------------------------------------------ G
@pytest.mark.parametrize("route", ("quads", "general"))
def test_g_entry_points_agree_to_the_bit(route, monkeypatch, tmp_path):
    """Host memory, HBM and a trajectory file (once through a non-monotonic particle index) enter
    isf_accumulate_staged with the same chunks, and the sums are formed in a fixed order: bit-identical."""
    ws, groups, n_lags, cuts = ic.SMALL_GRID, (41, 22), 5, (3, 9, 8)
    n = sum(groups)
    frames = walk(sum(cuts), n, 33.0, 41)
    pairs = ic.pairs_of(2, "partial")
    ref = reference("G", frames, groups, pairs, ws, n_lags)
    starts = np.concatenate(([0], np.cumsum(cuts)))

    host = run(monkeypatch, ws, route, groups, pairs, n_lags, frames, cuts)
    check("G host", route, ws, host, ref)

    eng = engine(monkeypatch, ws, route, groups, pairs, n_lags)
    d_frames = _core.DeviceArray.from_host(frames)
    for a, c in zip(starts, cuts):
        eng.accumulate_device(d_frames.offset(int(a)), n, int(c))
    eng.synchronize()
    device = eng.result()
    eng.close()
    d_frames.free()

    # the file holds more particles in another order; the index picks the groups' rows back out of it
    rng = np.random.default_rng(43)
    n_file = n + 9
    index = rng.permutation(n_file)[:n].astype(np.int32)
    assert np.any(np.diff(index) < 0)
    stored = walk(sum(cuts), n_file, 33.0, 47)
    stored[:, index] = frames
    results = {}
    for name, data, idx in (("file", frames, None), ("file + index", stored, index)):
        path = tmp_path / (name.replace(" + ", "_") + ".nc")
        write_amber_netcdf(path, data, (33.0, 33.0, 33.0))
        t = TrajectoryFile(path)
        eng = engine(monkeypatch, ws, route, groups, pairs, n_lags)
        for a, c in zip(starts, cuts):
            eng.accumulate_traj(t, np.arange(a, a + c), idx)
        results[name] = eng.result()
        eng.close()
        t.close()
    for name, got in (("device", device), *results.items()):
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]), name


# ------------------------------------------------------------------------------------------------ H
@pytest.mark.parametrize("route", ("quads", "general"))
def test_h_molecule_stage_inside_the_chunk_loop(route, monkeypatch):
    """Molecules of 1, 2 and 5 atoms with unequal masses; 9 lags and 40 frames: the row stage is refilled chunk by
    chunk across ring wraps (18 slots)."""
    ws, n_lags, n_frames = ic.SMALL_GRID, 9, 40
    groups = (29, 16)                                   # molecules per group
    sizes = np.resize([1, 2, 5], sum(groups))
    mol_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    rng = np.random.default_rng(53)
    masses = rng.uniform(1.0, 30.0, int(mol_offsets[-1]))
    atoms = walk(n_frames, int(mol_offsets[-1]), 33.0, 59)
    centres = of.molecule_centres_ref(atoms, mol_offsets, masses)
    assert centres.dtype == np.float32 and centres.shape == (n_frames, sum(groups), 3)
    pairs = ic.pairs_of(2, "partial")
    ref = reference("H", centres, groups, pairs, ws, n_lags)
    for cuts in (None, (4, 13, 23)):
        eng = engine(monkeypatch, ws, route, groups, pairs, n_lags)
        try:
            eng.set_grouping(mol_offsets, masses)
            feed(eng, atoms, cuts)
            check(f"H {cuts}", route, ws, eng.result(), ref)
            with pytest.raises(ValueError, match="grouping was defined for"):     # the stage's own row-count check
                eng.accumulate(atoms[:1, :-1])
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------ I
@pytest.mark.parametrize("route", ic.ROUTES)
def test_i_invariants_without_tolerance(route, monkeypatch):
    ws, groups, n_lags, cuts = ic.SMALL_GRID, (333, 130), 4, (1, 5, 3)
    n_frames = sum(cuts)
    frames = walk(n_frames, sum(groups), 33.0, 61)
    for mode in ("partial", None):
        pairs = ic.pairs_of(2, mode)
        eng = engine(monkeypatch, ws, route, groups, pairs, n_lags)
        try:
            feed(eng, frames, cuts)
            first = eng.result()
            # lag 0: the displacement is 0, every table entry and every cosine is 1
            sizes = np.array(groups if mode else [sum(groups)], dtype=np.float64)
            assert np.array_equal(first[1][0], np.broadcast_to(sizes[:, None] * n_frames, first[1][0].shape))
            again = eng.result()
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
            eng.reset()
            zero = eng.result()
            assert not zero[0].any() and not zero[1].any()
            feed(eng, frames, cuts)
            second = eng.result()
            assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        finally:
            eng.close()
        # cisf[0] is the structure factor's sum over the frames (the SqEngine, default route)
        ic.set_env(monkeypatch, {})
        sq = _core.SqEngine(ws.q, groups, pairs)
        sq.accumulate(frames)
        ssf = sq.result()
        sq.close()
        ref = reference(("I", mode), frames, groups, pairs, ws, n_lags)
        check(f"I {mode}", route, ws, first, ref)
        phi = ref["phi_max"] + ws.m_max
        assert _ratio(first[0][0], ssf, ref["S_cisf"][0], phi) <= max(C.values())


# ------------------------------------------------------------------------------------------------ J
@pytest.mark.parametrize("incoherent", (True, False))
def test_j_changed_row_count_is_refused(incoherent, monkeypatch):
    """The position ring is laid out with the row count of the series: another count after the first frame is the
    library's invalid-value error (with or without the incoherent part — one rule), the frames accepted before it
    stay intact, and reset() starts a series that may have another count."""
    ws, groups, n_lags = ic.SMALL_GRID, (20, 9), 4
    n = sum(groups)
    frames = walk(9, n + 6, 33.0, 67)
    pairs = ic.pairs_of(2, "partial")
    eng = engine(monkeypatch, ws, "quads", groups, pairs, n_lags, incoherent)
    try:
        eng.accumulate(frames[:5, :n])
        before = eng.result()
        d_frames = _core.DeviceArray.from_host(frames[5:])
        for bad in (lambda: eng.accumulate(frames[5:]),                                   # more rows
                    lambda: eng.accumulate(frames[5:, :n + 1]),
                    lambda: eng.accumulate_device(d_frames.ptr, n + 6, 4)):
            with pytest.raises(ValueError, match="points per frame"):
                bad()
            after = eng.result()
            assert eng.stats()["frames"] == 5
            assert np.array_equal(before[0], after[0])
            assert after[1] is None if not incoherent else np.array_equal(before[1], after[1])
        d_frames.free()
        # the series goes on with the count it started with, as if nothing had happened
        eng.accumulate(frames[5:, :n])
        ref = reference("J", frames[:, :n], groups, pairs, ws, n_lags)
        check("J continued", "quads", ws, eng.result(), ref)
        # a new series may have another count: the extra rows lie beyond the groups' span
        eng.reset()
        eng.accumulate(frames)
        check("J after reset", "quads", ws, eng.result(), ref)
    finally:
        eng.close()
