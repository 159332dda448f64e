"""
``mdx_msd_plan`` on the CPU: every case of ``test_gpu_msd_routes.py`` (``msd_cases.py``) plans, in its environment, to
the pass-A and pass-B kernel, head, super groups, split and parts it names; the cases together reach every kernel the
engine can launch, all 16 heads, one, two and more super groups, one and several parts of pass B for both fused
families, single-pass grids limited by the pair groups and by the blocks, and both layouts of Y.  The reference of
every case is shown to be sensitive to the push's last coordinate series.  The query touches no device.
"""
import numpy as np
import pytest

import msd_cases as mc
from mdhelper_amd import _core
from oracle import correlation as oc

plan = _core.MsdEngine.plan
PASS_A, PASS_B = _core.MsdEngine.PASS_A, _core.MsdEngine.PASS_B


def plan_of(monkeypatch, c, push=None, elem_bytes=8):
    mc.set_env(monkeypatch, c.env)
    p = push or c.pushes[0]
    return plan(c.t_block, c.n_blocks, c.n_total, p.first, p.count, elem_bytes)


def test_kernels_are_named_as_the_library_numbers_them():
    assert PASS_A == mc.PASS_A and PASS_B == mc.PASS_B
    assert len(_core.MsdEngine.PLAN_FIELDS) == 16


def check_plan(monkeypatch, c):
    n_fft, r1, r2, a, b = mc.route_of(c)
    for i, push in enumerate(c.pushes):
        for elem_bytes in (8, 4) if c.f32 else (8,):
            p = plan_of(monkeypatch, c, push, elem_bytes)
            assert (p["n_fft"], p["r1"], p["r2"]) == (n_fft, r1, r2), (c.name, p)
            assert (PASS_A[p["pass_a"]], PASS_B[p["pass_b"]]) == (a, b), (c.name, p)
            assert p["own"] == (a != "rocfft") and p["single"] == (a == "single400"), (c.name, p)
            assert p["fused_sums"] == (a in ("single400", "cols400_fused", "cols_small_fused")), (c.name, p)
            assert p["reads_f32"] == p["fused_sums"]
            assert p["head"] == mc.expected_head(c, push), (c.name, p)
            assert p["n_elem"] == 3 * push.count + p["head"], (c.name, p)
            if i == 0:
                for key, value in c.want.items():
                    assert p[key] == value, (c.name, key, p)
    return plan_of(monkeypatch, c)


@pytest.mark.parametrize("c", mc.ALL_CASES, ids=lambda c: c.name)
def test_every_case_plans_to_what_it_names(c, monkeypatch):
    check_plan(monkeypatch, c)


def test_case_a_covers_the_eighteen_own_lengths_at_both_ends(monkeypatch):
    assert len(mc.LENGTHS) == 18
    shortest = {mc.own_length(t)[0]: t for t in mc.A_SHORTEST if t != 200}
    assert sorted(shortest) == sorted(row[2] for row in mc.LENGTHS)
    for lo, hi, n_fft, *_ in mc.LENGTHS:
        assert shortest[n_fft] == lo                                   # the shortest block of the length ...
        mc.set_env(monkeypatch, mc.OWN)
        if lo > 1:
            assert plan(lo - 1, 1, 16, 0, 11)["n_fft"] < n_fft          # ... one frame fewer takes the length before
        if n_fft <= 25600:
            assert hi in mc.A_LONGEST + (200,)                          # and the longest
            assert plan(hi + 1, 1, 16, 0, 11)["n_fft"] > n_fft
    # more than 524 288 frames: rocFFT without a switch
    assert plan(524289, 1, 16, 0, 11)["own"] == 0
    # rocFFT lengths: 1 frame, a power of two, and a length that is none
    assert [mc.route_of(c)[0] for c in mc.A_ROCFFT] == [2, 128, 144]


def test_the_cases_together_reach_every_kernel_and_edge(monkeypatch):
    plans = {c.name: check_plan(monkeypatch, c) for c in mc.ALL_CASES}
    assert {PASS_A[p["pass_a"]] for p in plans.values()} == set(PASS_A)
    # the general rows kernel is in the source but no length of the engine launches it: rows of 2 .. 1024 points all
    # have a kernel of their own (msdfft::pass_b_kernel), so the cases reach every pass B that can run
    assert {PASS_B[p["pass_b"]] for p in plans.values()} == set(PASS_B) - {"general"}
    mc.set_env(monkeypatch, mc.OWN)
    assert all(PASS_B[plan(row[0], 1, 16, 0, 11)["pass_b"]] != "general" for row in mc.LENGTHS)
    routes = {mc.route_name(c) for c in mc.ALL_CASES}
    assert routes == {"rocfft/none", "single400/none", "cols400_fused/tiny", "cols400_fused/short", "cols400_fused/mid",
                      "cols400_fused/rows512", "cols400_fused/rows1024", "cols_small_fused/mid",
                      "cols_small_fused/rows512", "cols_small_fused/rows1024", "cols/rows512", "cols/rows1024"}
    # every instantiation of the single-pass kernel and of the 400 x R2 and 64 x R2 pass A
    assert {p["r2"] for p in plans.values() if p["single"]} == {1, 2, 4}
    assert {p["r2"] for p in plans.values() if PASS_A[p["pass_a"]] == "cols400_fused"} == {2, 4} | {2 ** k for k in range(3, 11)}
    assert {p["r2"] for p in plans.values() if PASS_A[p["pass_a"]] == "cols_small_fused"} == {128, 256, 512, 1024}
    # all 16 heads, on each shape of case C, with every mask
    for t in mc.C_SHAPES:
        for z in mc.C_ZERO_DIMS:
            cases = mc.c_cases(t, z)
            assert {plans[c.name]["head"] for c in cases} == set(range(16))
            assert all(c.pushes[0].first + c.pushes[0].count == mc.C_TOTAL or c.pushes[0].count == 1 for c in cases)
            # odd and even n_elem: which coordinates pair up
            assert {plans[c.name]["n_elem"] % 2 for c in cases} == {0, 1}
    assert any(p["head"] and p["pg_major"] for p in plans.values())
    # ... and the same particles from a compact copy plan head 0
    for c in mc.C_CASES[::7]:
        assert check_plan(monkeypatch, mc.compact_of(c))["head"] == 0
    # super groups 1, 2 and >= 3 on both fused families, the last one ragged
    for family in ("cols400_fused", "cols_small_fused"):
        ps = [plans[c.name] for c in mc.B_CASES if mc.route_of(c)[3] == family]
        assert {min(p["super_groups"], 3) for p in ps} == {1, 2, 3}
        assert any(p["super_groups"] == 3 and p["p_pad"] % 64 for p in ps)
    small = [plans[c.name] for c in mc.B_CASES if mc.route_of(c)[3] == "cols_small_fused" and c.pushes[0].count >= 43]
    assert {p["r2"] for p in small} == {128, 256, 512, 1024} and all(p["super_groups"] >= 2 for p in small)
    # pair groups in fours (128-point rows) and in twos (256-point rows)
    assert plans["B T_b=16385 n=1"]["p_pad"] == 32 and plans["B T_b=6401 n=43"]["p_pad"] % 16 == 0
    # parts of pass B: one and several, for both fused families
    for cases in (mc.D_ROWS400, mc.D_ROWS64):
        parts = [plans[c.name]["rows_parts"] for c in cases]
        assert parts[-1] == 1 and parts[0] > 1 and parts[1] > 1, parts
    # the single-pass grid: 64 and 63 splits wanted, 4 pair groups there; 2 048 blocks and more: 1
    assert [plans[c.name]["split"] for c in mc.D_SINGLE] == [4, 4, 1, 1]
    assert plan(3, 33, 2000, 0, 2000)["split"] == 63 and plan(3, 1, 2000, 0, 2000)["split"] == 64
    assert {p["pg_major"] for p in plans.values() if p["own"] and not p["single"]} == {0, 1}


def test_controls_plan_no_head(monkeypatch):
    mc.set_env(monkeypatch, mc.OWN)
    for t in mc.C_SHAPES:
        for first in mc.C_FIRSTS:
            # 37 particles per frame: 111 coordinates, no whole lines
            assert plan(t, 2, mc.C_CONTROL_TOTAL, first, mc.C_CONTROL_TOTAL - first)["head"] == 0
            # an array that does not start on a line
            assert plan(t, 2, mc.C_TOTAL, first, 1, 8, False)["head"] == 0
    assert all(check_plan(monkeypatch, c)["head"] == 0 and c.pushes[0].first % 16 for c in mc.C_CONTROLS)
    for first in mc.C_FIRSTS:
        p = plan(mc.C_CONTROL_SMALL, 2, mc.C_TOTAL, first, mc.C_TOTAL - first)
        assert PASS_A[p["pass_a"]] == "cols_small_fused" and p["head"] == 0
    # MsdEngine.push stages the selection: the device side sees first = 0 of an array of `count` particles, whatever
    # the caller's range was — which is why the head cases go through push_device
    for t, count in ((70001, 16), (40000, 32), (50000, 48), (801, 32)):
        assert plan(t, 1, count, 0, count)["head"] == 0


def test_plan_follows_the_switches_and_refuses_bad_arguments(monkeypatch):
    mc.set_env(monkeypatch, mc.ROCFFT)
    for t in (1, 201, 801, 3201, 102401):
        p = plan(t, 1, 16, 0, 16)
        assert (p["own"], p["r1"], p["pass_a"], p["pass_b"], p["head"], p["p_pad"], p["split"]) == (0, 0, 0, 0, 0, 0, 0)
        assert p["n_elem"] == 48
        with pytest.raises(NotImplementedError):
            plan(t, 1, 16, 0, 16, 4)
    mc.set_env(monkeypatch, mc.TWO_PASS)
    assert plan(200, 1, 16, 0, 16)["single"] == 1                    # 400 points have no two-pass form
    assert plan(801, 1, 16, 0, 16)["pass_b"] == PASS_B.index("short")
    mc.set_env(monkeypatch, mc.OWN)
    with pytest.raises(NotImplementedError):
        plan(102401, 1, 16, 0, 16, 4)                               # 512 x 512 does not read float32
    for bad in ((0, 1, 16, 0, 16), (801, 0, 16, 0, 16), (801, 1, 16, 1, 16), (801, 1, 16, 0, 0), (801, 1, 16, -1, 4),
                (801, 1, 16, 0, 16, 2)):
        with pytest.raises(ValueError):
            plan(*bad)


# ------------------------------------------------------------------------------------------------ sensitivity
_TABLES = {}


def last_kept_series(push):
    """(particle, dimension) of the last coordinate series the push feeds: the last kept dimension of its last
    particle (a dropped dimension enters as zeros, and leaving zeros out changes nothing)."""
    return push.first + push.count - 1, max(k for k in range(3) if not (push.zero_dims >> k) & 1)


def weakest_ratio(c):
    """Smallest |full - without| / unit over the pushes, the blocks and lags 1 and T_b - 1 (T_b = 1: of the ACF)."""
    n_fft = mc.route_of(c)[0]
    lags = np.array(sorted({min(1, c.t_block - 1), c.t_block - 1}))
    tables = mc.tables_of(c, lags, _TABLES)
    weakest = np.inf
    for push in c.pushes:
        full = oc.msd_definition_ref(mc.positions(c), c.t_block, c.n_blocks, push.first, push.count, push.zero_dims,
                                     lags, tables)
        particle, k = last_kept_series(push)
        less = {key: (v.copy() if key in ("sq", "acf", "e") else v) for key, v in tables.items()}
        for key in ("sq", "acf"):
            less[key][:, particle, k, :] = 0
        less["e"][:, particle, k] = 0
        without = oc.msd_definition_ref(mc.positions(c), c.t_block, c.n_blocks, push.first, push.count,
                                        push.zero_dims, lags, less)
        unit, unit_acf = mc.unit_of(n_fft, c.t_block, full["E"], lags)
        if c.t_block == 1:
            assert np.all(full["msd"] == 0)
            ratio = np.abs(full["acf"] - without["acf"]) / unit_acf
        else:
            ratio = np.abs(full["msd"] - without["msd"]) / unit
        weakest = min(weakest, float(ratio.min()))
    return weakest


@pytest.mark.parametrize("c", mc.SENSITIVITY_CASES, ids=lambda c: c.name)
def test_the_reference_notices_one_missing_series(c):
    """The reference of the push with its last coordinate series left out differs from the full one, at lag 1 and at
    lag T_b - 1 in every block, by more than 1000 C_MAX units of the bound the GPU test asserts: no kernel that drops,
    doubles or misplaces a series can stay inside any C <= C_MAX.  A block of ONE frame has lag 0 only, where the MSD
    is 0 whatever is pushed: there the un-normalised ACF (= E) carries the check."""
    r = weakest_ratio(c)
    assert r > 1000 * mc.C_MAX, (c.name, r)
    if len(_TABLES) > 8:
        _TABLES.clear()
        mc.forget_walks()
