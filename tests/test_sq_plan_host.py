"""
``mdx_sq_plan`` on the CPU: every wavevector set of ``test_gpu_sq_routes.py`` plans to the kernel route the GPU test
means to run, in every environment it runs it in; the sets together reach every quad form, one and several copies
per item, several blocks, both column block sizes, both table tiles and both refusals of the lattice detector; the
split, slab and chain cases report the parts and slab lengths they are there for.  The query touches no device.
"""
import numpy as np
import pytest

import isf_cases as ic
import sq_cases as sc
from mdhelper_amd import _core

plan = _core.SqEngine.plan
ROUTES = _core.SqEngine.ROUTES
GROUPS = sc.A_GROUPS[0]
ROUTE_KEYS = ("route", "regular_stride", "tile", "n_sub", "items_per_block", "blocks", "threads")


def default_plan(monkeypatch, ws, groups=GROUPS, n_frames=sc.A_FRAMES, chain_length=0):
    sc.set_env(monkeypatch, {})
    return plan(ws.q, groups, n_frames, chain_length)


def test_routes_are_named_as_the_library_numbers_them():
    assert ROUTES == sc.ROUTES


@pytest.mark.parametrize("ws", sc.NORMAL_SETS, ids=lambda ws: ws.name)
def test_every_set_plans_to_its_routes(ws, monkeypatch):
    """Its own route by default, every route of ``lower`` under that route's switch."""
    taken = dict(sc.routes_of(ws))
    assert len(taken) == 1 + len(ws.lower)
    p = default_plan(monkeypatch, ws)
    assert p["route"] == ws.route and p["regular_stride"] == ws.stride, (ws.name, p)
    for route, env in taken.items():
        sc.set_env(monkeypatch, env)
        p = plan(ws.q, GROUPS, sc.A_FRAMES)
        assert ROUTES[p["route"]] == route, (ws.name, route, p)
        n_q = len(ws.q)
        if route in ("general", "tables"):
            assert p["threads"] == 256 and p["items_per_block"] == 512 and p["blocks"] == -(-n_q // 512)
            assert p["regular_stride"] == 0 and p["n_sub"] == 1
            assert p["tile"] == 1024 if route == "general" else 8 <= p["tile"] <= 64
        elif route == "columns":
            assert p["threads"] in (64, 128, 192, 256) and p["items_per_block"] == p["threads"]
            assert p["regular_stride"] == 0 and p["n_sub"] == 1 and 4 <= p["tile"] <= 64
        else:
            assert p["threads"] == 256 and p["tile"] % p["n_sub"] == 0 and p["items_per_block"] * p["n_sub"] <= 256
            assert p["regular_stride"] in (0, p["tile"] + 1)
        # the wavevectors alone decide the route: the small groups of case A get the same kernels
        small = plan(ws.q, sc.A_GROUPS[1], sc.A_FRAMES)
        assert [small[k] for k in ROUTE_KEYS] == [p[k] for k in ROUTE_KEYS]


def test_isf_sets_reach_the_same_quad_forms_here(monkeypatch):
    """mdx_sq_create and the ISF planner call sq_quad_plan with the same arguments: verified, not assumed."""
    for ws in ic.B_SETS:
        ic.set_env(monkeypatch, {})
        isf = _core.IsfEngine.plan(ws.q, ic.B_GROUPS[0], ic.pairs_of(2, "partial"), ic.B_LAGS)
        sq = default_plan(monkeypatch, ws)
        assert (sq["route"] == 3) == (isf["route"] == 2), ws.name
        if isf["route"] == 2:
            for key in ("regular_stride", "tile", "n_sub", "items_per_block", "blocks"):
                assert sq[key] == isf[key], (ws.name, key)
        else:
            assert (sq["route"] == 0) == (isf["route"] == 0), ws.name


def test_the_sets_together_reach_every_form(monkeypatch):
    plans = {ws.name: default_plan(monkeypatch, ws) for ws in sc.A_SETS}
    quads = [p for p in plans.values() if p["route"] == 3]
    assert {p["regular_stride"] for p in quads} == {0, 17, 33, 49, 65, 81}             # all six quad forms
    # several copies per item, and (the 32^3 grid of case D) one; more than one block
    assert any(p["n_sub"] >= 2 for p in quads) and default_plan(monkeypatch, sc.D_BYTE_SET)["n_sub"] == 1
    assert any(p["blocks"] > 1 and p["n_sub"] >= 2 for p in quads)
    # the columns route by default: the quad planner declines, sq_build_columns takes; blocks of 64 and of 256 threads
    columns = {name: p for name, p in plans.items() if p["route"] == 2}
    assert {64, 256} <= {p["threads"] for p in columns.values()}
    # ... and every column of the 7^3 sets holds at most 7 wavevectors: items of nz < 8
    assert "ragged columns of the 7^3 grid" in columns
    # the tables route by default: both builders decline; tiles of 64 and of 8 particles
    tables = [p for p in plans.values() if p["route"] == 1]
    assert {8, 64} <= {p["tile"] for p in tables}
    # lattice-shaped sets the detector declines: the general kernel without a switch
    declined = [ws for ws in sc.A_SETS if ws.route == 0 and ws.m_max > 0]
    assert len(declined) == 2 and all(plans[ws.name]["route"] == 0 for ws in declined)
    m = [np.rint(ws.q * sc.LENGTHS / (2 * np.pi)).astype(int) for ws in declined]
    assert not (m[0] == 1).any() and 3 * (m[0].max() - m[0].min() + 1) <= 208          # no m = 1 on any axis
    assert all((m[1] == 1).any(axis=0)) and 3 * (m[1].max() + 1) > 208                 # sum R > 208
    # every lattice set runs again on each lower route: the lower routes are reached by sets of every quad form
    for route in ("columns", "tables", "general"):
        assert {ws.stride for ws in sc.A_SETS if ws.route == 3 and route in ws.lower} >= {0, 17, 33, 49, 81}
    # the 63 wavevectors of the small grid are one short of what sq_build_columns takes: MDX_SQ_NO_QUADS lands on the
    # tables, and a test that called that run "columns" would compare the tables kernel with itself
    sc.set_env(monkeypatch, "columns")
    assert plan(sc.C_SET.q, GROUPS, sc.A_FRAMES)["route"] == 1 and "columns" not in sc.C_SET.lower
    assert plan(sc.C_COLUMNS_SET.q, GROUPS, sc.A_FRAMES)["route"] == 2
    # the tables route with two q-blocks (case B)
    sc.set_env(monkeypatch, "tables")
    p = plan(sc.B_TABLES_SET.q, sc.B_GROUPS, sc.B_FRAMES)
    assert p["route"] == 1 and p["blocks"] == 2
    # a wavevector listed twice: the regular quad form declines it, the general items take it (case H)
    p = default_plan(monkeypatch, sc.H_TWICE)
    assert p["route"] == 3 and p["regular_stride"] == 0
    a, b = sc.H_TWICE_AT
    assert a != b and np.array_equal(sc.H_TWICE.q[a], sc.H_TWICE.q[b])


@pytest.mark.parametrize("case", sc.C_CASES, ids=lambda c: c[0])
def test_split_cases_report_their_parts(case, monkeypatch):
    _, groups, mode, parts, ragged = case
    biggest = max(groups)
    for route, ws in sc.C_ROUTE_SETS:
        sc.set_env(monkeypatch, route)
        p = plan(ws.q, groups, sc.C_FRAMES)
        assert ROUTES[p["route"]] == route and p["n_split"] == parts, (route, p)
        assert p["slab_frames"] == sc.C_FRAMES
        per = -(-biggest // parts)
        assert (per * parts != biggest) == ragged
        assert per * (parts - 1) < biggest                     # the last part of the large group is not empty
    if len(groups) > 1:
        # per = ceil(3 / 2) = 2: the group of 3 splits 2 + 1; the group of 1 leaves an empty part, the empty group two
        assert [(-(-n // parts), n) for n in groups[1:]] == [(2, 3), (0, 0), (1, 1)]
    # one particle fewer than 4096 and the engine does not split at all: nothing in the suite reached n_split > 1
    sc.set_env(monkeypatch, {})
    assert plan(sc.C_SET.q, (4095,), sc.C_FRAMES)["n_split"] == 1
    assert plan(sc.C_SET.q, (4096,), 4096)["n_split"] == 1      # ... nor with many frames


def test_slab_cases_report_both_caps(monkeypatch):
    # the frame cap, on every route the one-column set can take, and in chain mode
    for route, env in sc.routes_of(sc.D_COLUMN):
        sc.set_env(monkeypatch, env)
        p = plan(sc.D_COLUMN.q, sc.D_GROUPS, sc.D_FRAMES)
        assert ROUTES[p["route"]] == route and p["slab_frames"] == 32768 < sc.D_FRAMES, (route, p)
        assert p["n_split"] == 1
    assert len(sc.D_COLUMN.q) == 7
    sc.set_env(monkeypatch, {})
    for ws, route in ((sc.D_COLUMN, 0), (sc.D_CHAIN_QUADS_SET, 3)):
        p = plan(ws.q, (sc.D_CHAIN_POINTS,), sc.D_FRAMES, sc.D_CHAIN_LENGTH)
        assert p["route"] == route and p["slab_frames"] == 32768 and p["n_split"] == 1, p
    # the byte cap: 32 768 wavevectors x 16 bytes = 512 KiB of partial sums per frame, 1 024 frames in 512 MiB
    for route, env in sc.routes_of(sc.D_BYTE_SET):
        sc.set_env(monkeypatch, env)
        p = plan(sc.D_BYTE_SET.q, (2,), sc.D_BYTE_FRAMES)
        assert ROUTES[p["route"]] == route and p["slab_frames"] == sc.D_BYTE_SLAB < sc.D_BYTE_FRAMES, (route, p)
        assert p["n_split"] == 1
    p = default_plan(monkeypatch, sc.D_BYTE_SET, (2,), sc.D_BYTE_FRAMES)
    assert p["n_sub"] == 1 and p["blocks"] > 1 and p["regular_stride"] == 17
    assert {0, 1, 63, 64, 511, 512, 32767} <= set(sc.D_BYTE_CHECKED.tolist()) and len(sc.D_BYTE_CHECKED) <= 128


def test_chain_cases_reach_both_kernels_and_their_splits(monkeypatch):
    for name, ws, env, route, stride in sc.E_FORMS:
        sc.set_env(monkeypatch, env)
        p = plan(ws.q, (4101,), sc.E_FRAMES, 1367)
        assert p["route"] == route and p["regular_stride"] == stride and p["n_sub"] == 1, (name, p)
        assert p["tile"] == (sc.E_TILES[name] if route == 3 else sc.E_SINCOS_TILE), (name, p)
        for _, n_chains, length, parts, per in sc.E_SPLITS:
            p = plan(ws.q, (n_chains * length,), sc.E_FRAMES, length)
            assert p["route"] == route and p["n_split"] == parts and p["chains_per_part"] == per, (name, p)
        # the whole system as one chain is never split
        assert plan(ws.q, (8200,), sc.E_FRAMES, 8200)["n_split"] == 1
    # 3 chains in parts of 2: the last part holds one chain
    assert sc.E_SPLITS[0][1] - sc.E_SPLITS[0][4] * (sc.E_SPLITS[0][3] - 1) == 1
    # a chain plan (one copy per item) never comes out differently from the normal plan: a set that takes the quads
    # in the normal mode takes them in chain mode, with the same item form — so the sincos kernel is reached by a
    # switch or by a set that no quad form takes, not by the cap on the copies
    for ws in sc.NORMAL_SETS:
        normal = default_plan(monkeypatch, ws)
        chain = default_plan(monkeypatch, ws, (8,), 2, 2)
        assert (chain["route"] == 3) == (normal["route"] == 3), ws.name
        if normal["route"] == 3:
            assert (chain["regular_stride"] == 0) == (normal["regular_stride"] == 0), ws.name


def test_plan_follows_the_switches_and_refuses_bad_arguments(monkeypatch):
    q = sc.C_COLUMNS_SET.q
    for route in sc.ROUTES:
        sc.set_env(monkeypatch, route)
        assert ROUTES[plan(q, (9,), 3)["route"]] == route
    sc.set_env(monkeypatch, {"MDX_SQ_NO_LATTICE": "1", "MDX_SQ_NO_QUADS": "1"})
    assert plan(q, (9,), 3)["route"] == 0
    sc.set_env(monkeypatch, {})
    with pytest.raises(ValueError):
        plan(q, (9,), 0)
    with pytest.raises(ValueError):
        plan(np.zeros((0, 3)), (9,), 3)
    with pytest.raises(ValueError):
        plan(q, (9,), 3, 2)             # 9 points are no whole number of chains of 2
    with pytest.raises(ValueError):
        plan(q, (6, 6), 3, 2)           # chain mode needs one group
