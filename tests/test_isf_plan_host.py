"""
``mdx_isf_plan`` on the CPU: every wavevector set of ``test_gpu_isf_routes.py`` plans to the kernel route the GPU test
means to run, the sets together reach every row stride of the regular quad form, and the particle-split cases
report the splits (with a ragged last part) they are there for.  The query touches no device.
"""
import numpy as np
import pytest

import isf_cases as ic
from mdhelper_amd import _core

plan = _core.IsfEngine.plan
PARTIAL2 = ic.pairs_of(2, "partial")
ic_route_keys = ("route", "regular_stride", "tile", "n_sub", "items_per_block", "blocks")


@pytest.mark.parametrize("ws", ic.ALL_SETS, ids=lambda ws: ws.name)
def test_every_set_plans_to_its_route(ws, monkeypatch):
    for route, env in ic.routes_of(ws):
        ic.set_env(monkeypatch, env)
        p = plan(ws.q, (333, 130), PARTIAL2, 4)
        assert _core.IsfEngine.ROUTES[p["route"]] == route, (ws.name, env, p)
        if not env:
            assert p["route"] == ws.route and p["regular_stride"] == ws.stride, (ws.name, p)
        if route != "quads":
            assert p["regular_stride"] == 0 and p["n_sub"] == 1
            assert p["blocks"] == -(-len(ws.q) // 512) and p["items_per_block"] == 512
            assert p["tile"] == 512 if route == "general" else 8 <= p["tile"] <= 64
        else:
            assert p["tile"] % p["n_sub"] == 0 and p["items_per_block"] * p["n_sub"] <= 256
            assert p["regular_stride"] in (0, p["tile"] + 1)


def test_the_sets_reach_every_row_stride(monkeypatch):
    ic.set_env(monkeypatch, {})
    strides = {plan(ws.q, ic.B_GROUPS[0], PARTIAL2, ic.B_LAGS)["regular_stride"] for ws in ic.B_SETS if ws.route == 2}
    assert strides == {0, 17, 33, 49, 65, 81}
    # ... for the small groups as well: the wavevectors alone decide the route
    for ws in ic.B_SETS:
        a, b = (plan(ws.q, g, PARTIAL2, ic.B_LAGS) for g in ic.B_GROUPS)
        assert [a[k] for k in ic_route_keys] == [b[k] for k in ic_route_keys]
    # at least one quads set needs more than one block of items
    assert any(plan(ws.q, ic.B_GROUPS[0], PARTIAL2, ic.B_LAGS)["blocks"] > 1 for ws in ic.B_SETS if ws.route == 2)


@pytest.mark.parametrize("case", ic.D_CASES, ids=lambda c: c[0])
def test_split_cases_report_ragged_splits(case, monkeypatch):
    _, groups, mode, rho_split = case
    pairs = ic.pairs_of(len(groups), mode)
    biggest = max(groups) if mode else sum(groups)
    for route, env in ic.routes_of(ic.SMALL_GRID):
        ic.set_env(monkeypatch, env)
        for n_new in (ic.D_LAGS, 1):          # a full chunk and the last frame of the feed
            p = plan(ic.SMALL_GRID.q, groups, pairs, ic.D_LAGS, n_new)
            assert _core.IsfEngine.ROUTES[p["route"]] == route
            assert p["rho_split"] == rho_split, (route, p)
            assert p["incoherent_split"] > 1, (route, p)
            # per = ceil(range / parts) does not divide the range: the last part is shorter
            for parts in (p["rho_split"], p["incoherent_split"]):
                assert -(-biggest // parts) * parts != biggest, (route, parts)
                assert -(-biggest // parts) * (parts - 1) < biggest      # ... but not empty


def test_plan_follows_the_switches_and_refuses_bad_arguments(monkeypatch):
    q = ic.SMALL_GRID.q
    ic.set_env(monkeypatch, {"MDX_SQ_NO_LATTICE": "1", "MDX_ISF_NO_QUADS": "1"})
    assert plan(q, (9,), ic.pairs_of(1, None), 3)["route"] == 0
    ic.set_env(monkeypatch, {})
    assert plan(q, (9,), ic.pairs_of(1, None), 3)["route"] == 2
    # pairs without a diagonal pair: no incoherent range to split
    assert plan(q, (5000, 10, 5000), ((0, 2),), 3)["incoherent_split"] == 1
    assert plan(q, (5000, 10, 5000), ((1, 1), (0, 2)), 3)["incoherent_split"] == 1
    assert plan(q, (5000, 10, 5000), ((0, 0), (0, 2)), 3)["incoherent_split"] > 1
    with pytest.raises(ValueError):
        plan(q, (9,), ic.pairs_of(1, None), 0)
    with pytest.raises(ValueError):
        plan(np.zeros((0, 3)), (9,), ic.pairs_of(1, None), 3)
