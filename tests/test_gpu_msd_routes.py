"""
Every transform route of the MSD engine (csrc/mdx_msd.hip, csrc/mdx_msd_fft.hpp) against the windowed fp64 definition
of its outputs, at the edges of its bookkeeping: the 18 own transform lengths at their shortest and longest blocks, the
two-pass and rocFFT switches, particle counts around the pairs, pair groups and super groups, every head (a push that
pass A enters up to 15 coordinates early) crossed with every mask of dropped dimensions, the block counts at which the
single-pass grid and the parts of pass B change, tolerance-free invariants, far-from-origin walks, float32 frames read
in place and the refusals.  The cases are those of ``msd_cases.py``; ``test_msd_plan_host.py`` shows on the CPU what
they reach.

Every case sets its stated environment (none, MDX_MSD_TWO_PASS=1 or MDX_MSD_ROCFFT=1), first asserts through the plan
query (``MsdEngine.plan``, mdx_msd_plan) that this is the pass A, pass B, head, super-group count, split and part count
it means to test, then checks ``n_fft`` and ``transform`` of the live engine, and compares ``result()`` and
``result_acf()`` with ``oracle.correlation.msd_definition_ref`` in EVERY block and group, at every lag (blocks of up
to 1 600 frames) or at the lags of ``msd_cases.lags_of``.

Tolerance.  With E[g, b] = sum over the pushed particles, kept dimensions and frames of x^2,

    |msd - ref|        <= C[route] * unit,   unit[g, b, m] = 2^-52 (1 + log2 n_fft) E[g, b] / (T_b - m)
    |result_acf - ref| <= C[route] * 2^-52 (1 + log2 n_fft) E[g, b]

(the FFT correlation errs by a small multiple of eps log2 N |x|^2, the S_m recurrence cancels against 2 sum D = 2 E,
and both are divided by the window count), so E = 0 asks for exact zeros.  C is one number per pass-A/pass-B route: 8 x
the largest ratio observed over this module on an MI355X, rounded up to a power of two, and at most C_MAX = 4096.  The
sums are formed in a fixed order, so there is no run-to-run spread and the margin is for other inputs.  Route-against-
route comparisons (own against rocFFT, single pass against two passes, a head push against a compact copy of the same
particles, one push against two) use the same bound.  ``traj`` is held to |got - ref| <= (n - 1) 2^-52 A[t, k],
A = sum_p |x_pk(t)|, which holds for any order of n additions: nothing is measured there.

Observed |got - ref| / unit, largest over the module (msd and result_acf together):

    route                        ratio     C       from
    rocfft/none                  0.989     8       a block of ONE frame, n_fft = 2 (case A under MDX_MSD_ROCFFT=1)
    single400/none               0.629     8       T_b = 150, float32 frames, head 9, y dropped (case G)
    cols400_fused/tiny           0.484     4       T_b = 401 under MDX_MSD_TWO_PASS=1 (case A)
    cols400_fused/short          0.609     8       T_b = 801, first = 11 (head 1), 21 particles, y dropped (case C)
    cols400_fused/mid            0.330     4       T_b = 32 769 (case A)
    cols400_fused/rows512        0.390     4       T_b = 51 201 (case A)
    cols400_fused/rows1024       0.609     8       T_b = 131 073 (case A)
    cols_small_fused/mid         0.506     8       T_b = 3 201 in 63 blocks, 4 particles (case D)
    cols_small_fused/rows512     0.435     4       T_b = 12 801, 43 particles: two super groups (case B)
    cols_small_fused/rows1024    0.586     8       T_b = 25 601 (case A)
    cols/rows512                 0.653     8       T_b = 204 801 (case A)
    cols/rows1024                0.665     8       T_b = 262 145 (case A)

(route against route at most 0.65: a head push against the compact copy on the single-pass kernel, T_b = 150; own
against rocFFT 0.41, single pass against two passes 0.35, one push against two 0.26.  Nothing was found wrong.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import msd_cases as mc  # noqa: E402
from mdhelper_amd import _core  # noqa: E402
from oracle import correlation as oc  # noqa: E402

C_MAX = mc.C_MAX
C = mc.ROUTE_C              # one table for this module and test_gpu_msd_ingest.py
OBSERVED = {}            # route -> (largest ratio seen, the case that gave it)
PLAN = _core.MsdEngine.plan
PASS_A, PASS_B = _core.MsdEngine.PASS_A, _core.MsdEngine.PASS_B


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    assert max(C.values()) <= C_MAX
    yield
    for route, (r, label) in sorted(OBSERVED.items()):
        print(f"\nMSD-RATIO {route:26s} {r:.4g} (C = {C[route]:g}) from {label}", end="")
    print()
    mc.forget_walks()


@pytest.fixture
def hbm():
    """Uploads of a test, freed when it ends; every array must start on a 128-byte line (what the head needs)."""
    held = []

    def upload(arr):
        d = _core.DeviceArray.from_host(arr)
        held.append(d)
        assert d.ptr.value % 128 == 0
        return d

    yield upload
    for d in held:
        d.free()


@pytest.fixture(autouse=True)
def _drop_walks():
    """The walks are regenerated from their seeds; the (small) reference tables stay for the module."""
    yield
    mc.forget_walks()


_TABLES = {}


def reference(c, push, particles=None):
    """The definition for one push of the case; the per-series tables are computed once per walk and never modified."""
    lags = mc.lags_of(c.t_block)
    tables = mc.tables_of(c, lags, _TABLES, particles)
    ref = oc.msd_definition_ref(mc.positions(c), c.t_block, c.n_blocks, push.first, push.count, push.zero_dims, lags,
                                tables)
    ref["lags"], ref["n"] = lags, push.count
    return ref


def assert_plan(monkeypatch, c, elem_bytes=8):
    """The plan of every push of the case is what the tables say; returns the route name."""
    mc.set_env(monkeypatch, c.env)
    n_fft, r1, r2, a, b = mc.route_of(c)
    for i, push in enumerate(c.pushes):
        p = PLAN(c.t_block, c.n_blocks, c.n_total, push.first, push.count, elem_bytes)
        assert (p["n_fft"], p["r1"], p["r2"], PASS_A[p["pass_a"]], PASS_B[p["pass_b"]]) == (n_fft, r1, r2, a, b), (c.name, p)
        assert p["head"] == mc.expected_head(c, push) and p["n_elem"] == 3 * push.count + p["head"], (c.name, p)
        if i == 0:
            for key, value in c.want.items():
                assert p[key] == value, (c.name, key, p)
    return f"{a}/{b}"


def engine(monkeypatch, c, groups=None, elem_bytes=8):
    """An engine for the case in its environment, after the plan query and the live engine have confirmed the route."""
    route = assert_plan(monkeypatch, c, elem_bytes)
    n_fft, r1, r2, a, _ = mc.route_of(c)
    eng = _core.MsdEngine(c.t_block, c.n_blocks, groups or mc.n_groups(c))
    assert eng.n_fft == n_fft and eng.transform == (a != "rocfft", r1, r2), (c.name, eng.n_fft, eng.transform)
    assert eng.reads_f32 == (a not in ("rocfft", "cols"))
    return eng, route


def feed(eng, c, d_pos, f32=False, pushes=None):
    for p in pushes or c.pushes:
        (eng.push_device_f32 if f32 else eng.push_device)(p.group, d_pos.ptr, c.n_total, p.first, p.count, p.zero_dims)


def results(eng, lags):
    msd, traj = eng.result()
    return {"msd": msd[:, :, lags], "traj": traj, "acf": eng.result_acf()[:, :, lags]}


def run(monkeypatch, c, hbm, f32=False):
    eng, route = engine(monkeypatch, c, elem_bytes=4 if f32 else 8)
    try:
        pos = mc.positions(c)
        feed(eng, c, hbm(pos.astype(np.float32) if f32 else pos), f32)
        return results(eng, mc.lags_of(c.t_block)), route
    finally:
        eng.close()


def _ratio(got, want, unit):
    diff = np.abs(got - want)
    exact = unit == 0
    assert np.all(diff[exact] == 0), "nonzero where the definition gives an exact zero"
    return float((diff[~exact] / unit[~exact]).max(initial=0.0))


def check(label, route, c, got, ref, group=0, other=None, other_route=None, other_group=None):
    """Group ``group`` of ``got`` against the reference (or against group ``other_group`` of another run's results, same
    bound)."""
    n_fft = mc.route_of(c)[0]
    unit, unit_acf = mc.unit_of(n_fft, c.t_block, ref["E"], ref["lags"])
    at = group if other_group is None else other_group
    want = ref if other is None else {k: other[k][at] for k in ("msd", "acf", "traj")}
    r_msd = _ratio(got["msd"][group], want["msd"], unit)
    r_acf = _ratio(got["acf"][group], want["acf"], unit_acf)
    r = max(r_msd, r_acf)
    if other is None and r > OBSERVED.get(route, (-1.0, ""))[0]:
        OBSERVED[route] = (r, label)
    print(f"{label} g{group} | {route}{' vs ' + other_route if other_route else ''} | msd {r_msd:.4g} acf {r_acf:.4g}")
    assert r <= max(C[route], C[other_route or route]), (label, route, other_route, r_msd, r_acf)
    # the summed trajectories: any order of n additions (a comparison of two runs: each may be that far off)
    slack = (ref["n"] - 1) * mc.EPS * ref["A"] * (1 if other is None else 2)
    assert np.all(np.abs(got["traj"][group] - want["traj"]) <= slack), (label, "traj")
    for k in range(3):
        if not ref["A"][..., k].any():
            assert not got["traj"][group][..., k].any(), (label, "traj of a dropped dimension")


def check_case(label, route, c, got):
    """Every group of the case (one push each) in every block."""
    for push in c.pushes:
        check(label, route, c, got, reference(c, push), push.group)


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("c", mc.A_CASES, ids=lambda c: c.name)
def test_a_every_own_length(c, monkeypatch, hbm):
    """The 18 own lengths at their shortest block, those up to 25 600 points also at their longest: two groups of 11
    and 6 particles out of an array of 16 per frame, the second from particle 5."""
    got, route = run(monkeypatch, c, hbm)
    check_case(c.name, route, c, got)


@pytest.mark.parametrize("c", mc.A_TWO_PASS + mc.A_ROCFFT, ids=lambda c: c.name)
def test_a_switched_routes_and_route_against_route(c, monkeypatch, hbm):
    """The two-pass form of 800 and 1 600 points and the rocFFT pipeline (a block of one frame, a power-of-two length
    and one that is none), each against the definition and against the route the engine takes without the switch."""
    got, route = run(monkeypatch, c, hbm)
    check_case(c.name, route, c, got)
    plain = c._replace(env=mc.OWN)
    base, base_route = run(monkeypatch, plain, hbm)
    assert base_route != route
    for push in c.pushes:
        check(c.name, base_route, plain, base, reference(c, push), push.group, other=got, other_route=route)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("c", mc.B_CASES, ids=lambda c: c.name)
def test_b_particle_count_edges(c, monkeypatch, hbm):
    """1 particle (one live pair and a half-dead one), 5 and 11 (odd coordinate counts: the shifted last load), 16 (whole
    pair groups), 43 and 86 (two and three super groups, the last ragged) on one shape per pass-A kernel; the large
    counts on all four 64 x R2 shapes; 1, 5 and 6 on 512 x 512."""
    got, route = run(monkeypatch, c, hbm)
    check_case(c.name, route, c, got)


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("zero_dims", mc.C_ZERO_DIMS)
@pytest.mark.parametrize("t_block", mc.C_SHAPES)
def test_c_every_head_with_every_mask(t_block, zero_dims, monkeypatch, hbm):
    """first = 0 .. 15 of 32 particles per frame: pass A enters the push head = 3 first mod 16 coordinates early, which
    decides the dimension a coordinate belongs to and which coordinates pair up.  The range to the array's last
    particle and a single particle, float64 and float32, against the definition and against the same particles pushed
    from a compact copy (head 0)."""
    cases = mc.c_cases(t_block, zero_dims)
    pos = mc.positions(cases[0])
    d64, d32 = hbm(pos), hbm(pos.astype(np.float32))
    lags = mc.lags_of(t_block)
    eng, route = engine(monkeypatch, cases[0], groups=3)
    try:
        for c in cases:
            push = c.pushes[0]
            assert_plan(monkeypatch, c)
            assert_plan(monkeypatch, c, 4)
            assert_plan(monkeypatch, mc.compact_of(c))
            eng.reset()
            eng.push_device(0, d64.ptr, c.n_total, push.first, push.count, zero_dims)
            eng.push_device_f32(1, d32.ptr, c.n_total, push.first, push.count, zero_dims)
            compact = _core.DeviceArray.from_host(pos[:, push.first:push.first + push.count])
            assert compact.ptr.value % 128 == 0
            eng.push_device(2, compact.ptr, push.count, 0, push.count, zero_dims)
            got = results(eng, lags)
            compact.free()
            ref = reference(c, push, mc.C_TOTAL)
            check(c.name, route, c, got, ref, 0)
            check(c.name + " f32", route, c, got, ref, 1)
            assert np.array_equal(got["msd"][0], got["msd"][1]) and np.array_equal(got["traj"][0], got["traj"][1])
            check(c.name + " compact", route, c, got, ref, 2)
            check(c.name, route, c, got, ref, 0, other=got, other_route=route, other_group=2)
    finally:
        eng.close()


@pytest.mark.parametrize("c", mc.C_CONTROLS, ids=lambda c: c.name)
def test_c_controls_without_a_head(c, monkeypatch, hbm):
    """The pushes of case C where pass A must NOT enter early: 37 particles per frame (no whole lines) on the five
    shapes, and the 64 x 128 shape, whose pass A has no head; float64 and float32, y dropped."""
    assert c.pushes[0].first % 16 and mc.expected_head(c, c.pushes[0]) == 0
    wide, route = run(monkeypatch, c, hbm)
    narrow, _ = run(monkeypatch, c, hbm, f32=True)
    check_case(c.name, route, c, wide)
    assert all(np.array_equal(wide[k], narrow[k]) for k in wide)


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("c", mc.D_CASES, ids=lambda c: c.name)
def test_d_block_count_edges(c, monkeypatch, hbm):
    """The single-pass grid split by the pair groups (1 and 33 blocks) and by the blocks (2 048, 2 049); pass B of both
    fused families in several parts and in one, on either side of the block counts where that changes."""
    got, route = run(monkeypatch, c, hbm)
    check_case(c.name, route, c, got)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("c", mc.E_UNION, ids=lambda c: c.name)
def test_e_semantics_without_tolerance(c, monkeypatch, hbm):
    """Fixed-order sums: two runs give the same bits; reset() gives exact zeros and a re-run the same bits; a group
    never pushed stays zero; a push of no particles changes nothing; all dimensions dropped gives zeros; a dropped
    dimension's column of traj is exactly zero.  Within the bound: two pushes into one group equal one of the union."""
    push = c.pushes[0]
    lags = mc.lags_of(c.t_block)
    d_pos = hbm(mc.positions(c))
    eng, route = engine(monkeypatch, c, groups=4)
    try:
        feed(eng, c, d_pos)
        first = results(eng, lags)
        again = results(eng, lags)
        assert all(np.array_equal(first[k], again[k]) for k in first)           # reading the result changes nothing
        assert all(not first[k][1:].any() for k in first)                        # groups never pushed
        assert not first["traj"][0][..., 0].any() and not first["traj"][0][..., 2].any() and first["traj"][0].any()
        eng.push_device(0, d_pos.ptr, c.n_total, 3, 0, 0)                        # no particles
        eng.push_device(1, d_pos.ptr, c.n_total, 0, push.count, 7)               # no dimensions
        after = results(eng, lags)
        assert all(np.array_equal(first[k], after[k]) for k in first)
        eng.reset()
        zero = results(eng, lags)
        assert all(not zero[k].any() for k in zero)
        feed(eng, c, d_pos)
        rerun = results(eng, lags)
        assert all(np.array_equal(first[k], rerun[k]) for k in first)
        # the union in two pushes, cut inside a pair (7 particles = 21 coordinates), into another group
        cut = 7
        eng.push_device(2, d_pos.ptr, c.n_total, push.first, cut, push.zero_dims)
        eng.push_device(2, d_pos.ptr, c.n_total, push.first + cut, push.count - cut, push.zero_dims)
        both = results(eng, lags)
        ref = reference(c, push)
        check(c.name, route, c, both, ref, 0)
        check(c.name + " in two pushes", route, c, both, ref, 2)
        check(c.name, route, c, both, ref, 0, other=both, other_route=route, other_group=2)
    finally:
        eng.close()
    other = _core.MsdEngine(c.t_block, c.n_blocks, 4)
    try:
        feed(other, c, d_pos)
        fresh = results(other, lags)
        assert all(np.array_equal(first[k], fresh[k]) for k in first)            # another engine: the same bits
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("c", mc.F_CASES, ids=lambda c: c.name)
def test_f_walks_far_from_the_origin(c, monkeypatch, hbm):
    """An unwrapped walk centred 40 box lengths from the origin: E per frame is over 10^6 times the MSD of one step,
    and the same bound holds."""
    ref = reference(c, c.pushes[0])
    assert ref["lags"][1] == 1 and ref["E"].min() / c.t_block > 1e6 * ref["msd"][:, 1].max()
    got, route = run(monkeypatch, c, hbm)
    check_case(c.name, route, c, got)


# ------------------------------------------------------------------------------------------------ G
@pytest.mark.parametrize("c", mc.G_CASES, ids=lambda c: c.name)
def test_g_float32_frames_in_place(c, monkeypatch, hbm):
    """push_device_f32 with a head of 9 coordinates (where the family has one) and a dropped dimension: the definition
    of the widened data, and bit for bit what push_device gives for the widened array."""
    wide, route = run(monkeypatch, c, hbm)
    narrow, route32 = run(monkeypatch, c, hbm, f32=True)
    assert route == route32
    check_case(c.name, route, c, wide)
    check_case(c.name + " f32", route, c, narrow)
    assert all(np.array_equal(wide[k], narrow[k]) for k in wide)


# ------------------------------------------------------------------------------------------------ I
def test_i_refusals_leave_the_sums_unchanged(monkeypatch, hbm):
    c = mc.I_CASE
    push = c.pushes[0]
    lags = mc.lags_of(c.t_block)
    d_pos = hbm(mc.positions(c))
    eng, route = engine(monkeypatch, c, groups=2)
    try:
        eng.push_device(0, d_pos.ptr, c.n_total, push.first, 4, 0)
        before = results(eng, lags)
        for bad in ((0, c.n_total - 2, 3, 0), (0, -1, 2, 0), (0, 0, 2, 8), (2, 0, 2, 0), (-1, 0, 2, 0)):
            group, first, count, zero_dims = bad
            with pytest.raises(ValueError):
                eng.push_device(group, d_pos.ptr, c.n_total, first, count, zero_dims)
            with pytest.raises(ValueError):
                eng.push_device_f32(group, d_pos.ptr, c.n_total, first, count, zero_dims)
        after = results(eng, lags)
        assert all(np.array_equal(before[k], after[k]) for k in before)
        # the engine goes on: the rest of the push, and the whole is within the bound
        eng.push_device(0, d_pos.ptr, c.n_total, push.first + 4, push.count - 4, 0)
        check(c.name, route, c, results(eng, lags), reference(c, push), 0)
    finally:
        eng.close()
