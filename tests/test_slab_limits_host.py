"""
The slab plans of the lag and pair engines on the CPU (``engine.plan()`` = ``mdx_X_plan``: the host arithmetic the
accumulate loops call too), and the cases of ``test_gpu_slab_limits.py`` (``slab_limit_cases.py``): every case has its
seam where its family says, its rows make a seam state that is lost, re-filled or raised again change a result, and
the vectorised restatements equal the engines' own modules' on the first 300 frames.  Nothing here touches a device;
the dipole engine, whose create acquires a stream, has its plan pinned by the GPU module.
"""
import numpy as np
import pytest

import hydrogen_bond_cases as hbc
import slab_limit_cases as sc
import test_gpu_angle as tang
import test_gpu_four_point as tchi4
import test_gpu_orientation as tori
import test_gpu_residence as tprs
import test_gpu_vanhove as tvh
import test_gpu_vanhove_distinct as tvhd
from mdhelper_amd import _core

MIB = 1 << 20


def one(family, engine, **kw):
    found = [c for c in family if c.engine == engine and all(getattr(c, k) == v for k, v in kw.items())]
    return found[0]


# ------------------------------------------------------------------------------------------------ the plan query

def history_bound_case(engine):
    return one(sc.FAMILY2, engine)


@pytest.mark.parametrize("engine", [e for e in sc.ENGINES if e != "dip"])
def test_plan_is_the_byte_accounting_of_the_engine(engine):
    """slab_frames = min(32 768, 256 MiB // bytes of a frame), the bytes as each engine's source states them
    (``slab_limit_cases.frame_bytes``); ring_frames = max(lags) + slab_frames for the lag engines, else 0; a slab that
    was asked for replaces the default in both, and 0 restores it."""
    tiny = one(sc.FAMILY1, engine)
    cases = [tiny] + ([history_bound_case(engine)] if history_bound_case(engine) else [])
    for c in cases:
        per_frame = sc.frame_bytes(c)
        want = min(sc.LIMIT, max(1, (256 * MIB) // per_frame))
        assert want == (sc.LIMIT if c is tiny else (256 * MIB) // per_frame)
        assert c is tiny or 1000 <= want <= 3200
        lag = max(c.lags) if engine in sc.LAG_ENGINES else None
        eng = sc.make_engine(c)
        try:
            assert eng.plan() == {"slab_frames": want, "ring_frames": 0 if lag is None else lag + want}
            eng.set_slab_frames(7)
            assert eng.plan() == {"slab_frames": 7, "ring_frames": 0 if lag is None else lag + 7}
            eng.set_slab_frames(sc.LIMIT)
            assert eng.plan() == {"slab_frames": sc.LIMIT, "ring_frames": 0 if lag is None else lag + sc.LIMIT}
            eng.set_slab_frames(0)
            assert eng.plan() == {"slab_frames": want, "ring_frames": 0 if lag is None else lag + want}
        finally:
            eng.close()


def test_plan_of_a_distinct_van_hove_history_of_8192_rows():
    """12 B a row in the ring: 256 MiB hold 2 730 frames of 8 192 rows."""
    eng = _core.DistinctVanHoveEngine(8000, 192, sc.VHD_EDGES, sc.LAGS2, sc.MID_DIMS)
    try:
        assert eng.plan() == {"slab_frames": (256 * MIB) // (12 * 8192), "ring_frames": 999 + 2730}
    finally:
        eng.close()


def test_plan_errors_need_no_device():
    from mdhelper_amd import _lib
    assert _lib.lib().mdx_vh_plan(None, None, None) != 0
    eng = sc.make_engine(one(sc.FAMILY1, "prs"))
    try:
        assert _lib.lib().mdx_prs_plan(eng.handle, None, None) != 0
    finally:
        eng.close()


def test_dipole_formula_of_the_cases():
    """What ``slab_limit_cases.plan`` takes for the dipole engine: 24 B per tile of 128 points of a group."""
    c = one(sc.FAMILY2, "dip")
    assert sc.frame_bytes(c) == 24 * (4095 + 2) and sc.plan(c) == {"slab_frames": 2730, "ring_frames": 0}
    assert sc.plan(one(sc.FAMILY1, "dip")) == {"slab_frames": sc.LIMIT, "ring_frames": 0}


# ------------------------------------------------------------------------------------------------ the seams

@pytest.mark.parametrize("c", sc.ALL_CASES, ids=lambda c: c.name)
def test_every_case_has_its_seam_where_its_family_says(c):
    F, p = c.calls[-1], sc.plan(c)
    slab, ring = p["slab_frames"], p["ring_frames"]
    lag = max(c.lags) if c.lags else 0
    assert ring == (lag + slab if c.engine in sc.LAG_ENGINES else 0)
    assert all(0 < s < F for s in sc.seams(c))
    if c.family == 1:
        assert slab == sc.LIMIT and F == c.calls[-2] + sc.F1 and sc.input_bytes(c) <= 20e6
        assert sc.seams(c) == [c.calls[-2] + sc.LIMIT] and c.calls[-2] in (0, sc.FIRST)
        assert sc.scripted_seams(c) == sc.SEAMS1 and sc.seams(c)[0] in sc.SEAMS1
        if c.route == "host":       # one feed slab: the seam is the engine's own
            assert sc.feed_slab(c, sc.F1) == sc.F1 and len(c.calls) == 2 and not c.index
        else:
            assert c.index and len(c.calls) == 3
        if c.engine in sc.LAG_ENGINES:
            assert c.lags == (0, 1, 3, 40) and ring == 32808
            # the two-call form feeds more frames than the ring holds: it wraps inside the second call
            assert (F > ring) == (len(c.calls) == 3) and (len(c.calls) == 2 or c.calls[1] < ring < F)
        assert c.origin_step in (1, 3) and sc.LIMIT % 3 != 0
    elif c.family == 2:
        # roughly 1 000 to 3 000 frames: the angle lists of 600 centres give 3 103
        assert c.route == "device" and 1000 <= slab <= 3200 and F == slab + 3 and sc.seams(c) == [slab]
        assert slab == (256 * MIB) // sc.frame_bytes(c)
        # 12 B a row bound the distinct van Hove slab only from 2 731 rows on: its input is twice the others'
        assert c.lags in ((), (0, 1, 3, 999)) and sc.input_bytes(c) <= (272 if c.engine == "vhd" else 136) * MIB
        assert c.origin_step == (3 if c.engine == "vhd" else 1)
    elif c.family == 3:
        assert slab == sc.LIMIT and F == 3 * sc.LIMIT + 3 and sc.seams(c) == [sc.LIMIT, 2 * sc.LIMIT, 3 * sc.LIMIT]
        assert sc.input_bytes(c) < 10e6
    else:
        assert slab == sc.LIMIT and F == sc.F1 and sc.seams(c) == [sc.LIMIT] and c.lags == (0, 1, 40)
        assert sc.groups_of(c) == (65, 2 * 64 + 3) and c.bins in (201, 5000)
    # the comparison run never reaches a default slab or an origin batch
    assert sc.SPLIT_CALL <= sc.SPLIT_SLAB < slab and lag + sc.SPLIT_SLAB <= sc.WALK_ORIGINS + 1 or c.family == 3


@pytest.mark.parametrize("c", [c for c in sc.ALL_CASES if c.lags], ids=lambda c: c.name)
def test_every_lag_has_an_origin_pair_across_every_seam(c):
    """A launch behind a seam that evaluates nothing would hide a ring or a frame base lost there.  For every seam s:
    lag 0 has an origin behind it (s <= f0 < next seam); every lag from origin_step on has an origin pair across it
    (f0 < s <= f0 + lag < F: the frames s - lag ... s - 1 hold a multiple of origin_step); a shorter lag (lag 1 of the
    cases with every third frame an origin, where frame s - 1 is no origin) has a pair that ends in the launch behind
    the seam.  So every launch of a case adds to the sums of every lag."""
    F = c.calls[-1]
    ends = sc.seams(c)[1:] + [F]
    for s, end in zip(sc.seams(c), ends):
        for lag in c.lags:
            found = sc.seam_origins(c, s, lag)
            assert all(f0 % c.origin_step == 0 and f0 + lag < F for f0 in found), (s, lag)
            assert all(s <= f0 for f0 in found) if lag == 0 else all(f0 < s <= f0 + lag for f0 in found)
            assert found or 0 < lag < c.origin_step, (s, lag)
            assert any(s <= f0 + lag < end for f0 in range(0, F - lag, c.origin_step)), (s, lag)
            if lag == 0:
                assert any(f0 < end for f0 in found), s


def test_seam_origins_sees_an_empty_tail():
    """The shape this check exists for: slab 2 730, 2 733 frames, every 16th frame an origin: no lag of (0, 1, 3, 999)
    has a pair that ends behind the seam."""
    c = one(sc.FAMILY2, "vhd")._replace(origin_step=16)
    assert sc.seams(c) == [2730]
    assert sc.seam_origins(c, 2730, 0) == [] and not any(f0 + 1 >= 2730 for f0 in sc.seam_origins(c, 2730, 1))
    for lag in c.lags:
        assert not any(2730 <= f0 + lag < 2733 for f0 in range(0, 2733 - lag, 16))


def test_the_table_holds_what_the_families_list():
    names = [c.name for c in sc.ALL_CASES]
    assert len(set(names)) == len(names)
    assert {c.engine for c in sc.FAMILY1} == set(sc.ENGINES)
    for engine in sc.ENGINES:
        mine = [c for c in sc.FAMILY1 if c.engine == engine]
        assert {len(c.calls) for c in mine} == {2, 3}
        assert {c.origin_step for c in mine} == ({1, 3} if engine in sc.STEPPED else {1})
        assert {c.continuous for c in mine} == ({True, False} if engine in ("prs", "hb") else {True})
    assert sorted(c.engine for c in sc.FAMILY2) == sorted(sc.ENGINES)
    wide = one(sc.FAMILY2, "vhd")
    assert sc.groups_of(wide) == (8190, 2) and sc.plan(wide) == {"slab_frames": 2730, "ring_frames": 3729}
    assert [(c.engine, c.continuous) for c in sc.FAMILY3] == [("prs", False), ("prs", False), ("prs", True)]
    assert [c.engine for c in sc.FAMILY4] == ["vh", "vh"]
    assert sc.N % 64 and sc.N1 % 64 and sc.N2 % 64 and sc.N == sc.N1 + sc.N2


def test_origin_batches_of_family_3():
    """The third slab of the first case meets 72 768 origins: a batch of 65 535 and one of 7 233.  Every second frame
    of the second case: 49 152 origins at most, one batch, though more frames lie within its longest lag."""
    two, single, continuous = sc.FAMILY3
    assert continuous == two._replace(name=continuous.name, continuous=True)
    assert two.lags == (0, 1, 40000) and two.origin_step == 1 and sc.plan(two)["ring_frames"] == 72768
    third = sc.cuts(two)[2]
    assert third == 65536 and sc.walk_batches(two, third, sc.LIMIT) == [(25536, 65535), (25536 + 65535, 7233)]
    assert sum(n for _, n in sc.walk_batches(two, third, sc.LIMIT)) == 72768 == 98304 - 25536
    # the second slab meets the 65 536 origins [0, 65 536): a second batch of one origin; the first and last slabs one
    assert sc.walk_batches(two, sc.LIMIT, sc.LIMIT) == [(0, 65535), (65535, 1)]
    assert [len(sc.walk_batches(two, f, n)) for f, n in ((0, sc.LIMIT), (3 * sc.LIMIT, 3))] == [1, 1]
    assert single.lags == (0, 1, 65000) and single.origin_step == 2
    assert sc.walk_batches(single, third, sc.LIMIT) == [(268, 48884)]       # the even frames of [536, 98 304)
    assert max(len(sc.walk_batches(single, f, min(sc.LIMIT, single.calls[-1] - f))) for f in sc.cuts(single)) == 1
    assert 98304 - 536 > sc.WALK_ORIGINS                    # as frames they would not fit one batch
    # the longest lags have origins before and after the slab whose walk takes two batches
    assert two.calls[-1] - 40000 > 2 * sc.LIMIT - 40000 > 0 and single.calls[-1] - 65000 > 0


# ------------------------------------------------------------------------------------------------ what the rows must do

SCRIPTED = 8        # the scripted rows are among the first 8 of either set (of the first 10 molecules of the water)


def check_lists(near, far, s, per_frame_0):
    """What the list engines' cases guarantee around the seam s.  near: bool [3, rows, partners] of the frames s - 1,
    s, s + 1; far: bool [w + 2, ...] of the scripted rows alone in the frames s - w ... s + 1, w = max_lag / 2 + 1;
    per_frame_0: the contacts of frame 0."""
    per_frame = near.sum(axis=(1, 2))
    assert per_frame.min() >= 1
    assert (near[0] != near[1]).any(axis=1).any() and (near[1] != near[2]).any(axis=1).any()
    assert np.logical_and.reduce(far, axis=0).sum() >= 1                    # a mask that must survive the seam
    assert (np.logical_and.reduce(far[:-2], axis=0) & ~far[-2]).sum() >= 1  # alive up to s - 1, broken exactly at s
    assert per_frame[1] != per_frame[0] and per_frame[1] != per_frame_0     # a slab-relative frame index shows


@pytest.mark.parametrize("walk", ["small", "mid"])
def test_contacts_around_the_seams(walk):
    seen = set()
    for c in [c for c in sc.FAMILY1 + sc.FAMILY2 if c.walk == walk and c.engine in ("prs", "clu", "ang", "boo")]:
        s, = sc.seams(c)
        if s in seen:                                   # the engines' cases share the rows
            continue
        seen.add(s)
        n1, dims, pts = sc.groups_of(c)[0], sc.dims_of(c), sc.points(c)
        w = (max(c.lags) if c.lags else 40) // 2 + 1
        near = sc.contact_matrix(pts[[s - 1, s, s + 1, 0]], n1, dims, chunk=1)
        rows = list(range(SCRIPTED)) + list(range(n1, n1 + SCRIPTED))
        far = sc.contact_matrix(pts[s - w:s + 2][:, rows], SCRIPTED, dims)
        check_lists(near[:3], far, s, near[3].sum())
        assert near.sum(axis=2).max() <= sc.max_neighbors(c)
        if walk == "mid":                               # every frame: no row of either set beyond the cap
            h = sc.contact_matrix(pts, n1, dims)
            assert max(h.sum(axis=2).max(), h.sum(axis=1).max()) <= sc.max_neighbors(c)
            assert h.sum(axis=(1, 2)).min() >= 1 and (h.sum(axis=2) >= 2).any()     # and a centre with a triplet
    if walk == "small":                                 # every frame of the small walk: no row beyond any cap
        h = sc.contact_matrix(pts, n1, dims)
        assert h.sum(axis=2).max() <= 16 and h.sum(axis=(1, 2)).min() >= 1
        assert seen == set(sc.SEAMS1)


def test_contacts_around_the_seams_of_the_origin_batches():
    """Family 3: all frames of 3 x 5 pairs.  Around each of the three seams the contact set changes, a contact breaks
    exactly there, and the contacts of the seam frame differ in number from those of the frame before and of frame 0;
    one contact lives through all frames, so through every seam and half of the longest lag before it."""
    c = sc.FAMILY3[0]
    assert all(sc.seams(k) == sc.seams(c) and sc.scripted_seams(k) == tuple(sc.seams(c)) for k in sc.FAMILY3)
    h = sc.contact_matrix(sc.points(c), sc.BATCH_N1, sc.BATCH_DIMS)
    per_frame = h.sum(axis=(1, 2))
    assert h.all(axis=0).sum() >= 1 and per_frame.min() >= 1 and h.sum(axis=2).max() <= sc.max_neighbors(c)
    for s in sc.seams(c):
        assert (h[s - 1] != h[s]).any() and (h[s] != h[s + 1]).any()
        assert (h[s - 20001:s].all(axis=0) & ~h[s]).sum() >= 1          # alive for half the longest lag, broken at s
        assert per_frame[s] != per_frame[s - 1] and per_frame[s] != per_frame[0]


def test_bonds_around_the_seams():
    for c in (one(sc.FAMILY1, "hb"), one(sc.FAMILY1, "hb", route="device"), one(sc.FAMILY2, "hb")):
        s, = sc.seams(c)
        dims, pts = sc.dims_of(c), sc.points(c)
        w = max(c.lags) // 2 + 1
        n_a = len(sc.hb_tables(c)[2])
        near = sc.bond_matrix(pts[[s - 1, s, s + 1, 0]], dims, chunk=1, acceptors=n_a)
        far = sc.bond_matrix(pts[s - w:s + 2][:, :30], dims)
        check_lists(near[:3], far, s, near[3].sum())
        assert near.sum(axis=2).max() <= sc.max_neighbors(c) and n_a >= 10      # the scripted molecules accept
    b = sc.bond_matrix(sc.points(one(sc.FAMILY1, "hb")), sc.HB_BOX)
    assert b.sum(axis=2).max() <= sc.max_neighbors(c) and b.sum(axis=(1, 2)).min() >= 1


@pytest.mark.parametrize("walk", ["small", "big", "dip"])
def test_image_counts_change_at_the_seams(walk):
    seen = set()
    for c in [c for c in sc.FAMILY1 + sc.FAMILY2 if c.walk == walk and c.engine in sc.UNWRAPPED]:
        key = (tuple(sc.seams(c)), c.calls[-1])
        if key in seen:
            continue
        seen.add(key)
        pts, dims = sc.points(c)[:c.calls[-1]], sc.dims_of(c)
        for s in sc.seams(c):
            assert sc.crossed_at(pts[s - 1:s + 1].astype(np.float64), dims, 1).sum() >= 1, (c.name, s)
        margin = min(float(np.abs(np.abs(np.diff(pts[lo:lo + 4097].astype(np.float64), axis=0)) - dims / 2).min())
                     for lo in range(0, len(pts) - 1, 4096))
        assert margin > sc.MIN_MARGIN, c.name


def test_per_frame_values_differ_around_the_seams():
    """Dipole rows: the scripted point carries a charge and jumps by a box length less half a unit at the seam."""
    for c in (one(sc.FAMILY1, "dip"), one(sc.FAMILY2, "dip")):
        pts = sc.points(c)
        q = sc.dip_charges(pts.shape[1])
        for s in sc.seams(c):
            m = (q[None, :, None] * pts[[0, s - 1, s]].astype(np.float64)).sum(axis=1)
            assert np.abs(m[2] - m[1]).max() > 1e-3 and np.abs(m[2] - m[0]).max() > 1e-3


def test_rest_case_is_at_rest():
    c = sc.FAMILY4[0]
    pts = sc.points(c)
    assert pts.shape == (sc.F1, 196, 3) and (pts == pts[0]).all()
    assert np.searchsorted(sc.vh_edges(c), 0.0, side="right") - 1 == 0      # a displacement of 0 counts in bin 0
    # a wave's counter takes 64 lanes x 32 768 frames in the first launch of lag 0: 2^21, as the source says
    assert 64 * sc.LIMIT == 1 << 21 and max(sc.groups_of(c)) > 64


# ------------------------------------------------------------------------------------------------ the restatements

HEAD = 300


def test_vectorised_van_hove_is_the_modules_own():
    c = one(sc.FAMILY1, "vh")
    pts, sizes = sc.points(c)[sc.LIMIT - 200:sc.LIMIT + 100], sc.groups_of(c)
    got = sc.restate_vh(pts, sizes, sc.vh_edges(c), c.lags, sc.DIMS)
    want = tvh.restate(pts, sizes, sc.vh_edges(c), c.lags, dims=sc.DIMS)
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    assert got[3] == want[3] and want[0].sum() > 0
    x, _ = sc.unwrapped(pts, sc.DIMS)
    np.testing.assert_array_equal(x, pts.astype(np.float64) + tvh.images_ref(pts, sc.DIMS) * sc.DIMS)
    assert tvh.images_ref(pts, sc.DIMS).any()


def test_vectorised_four_point_is_the_modules_own():
    for c in (one(sc.FAMILY1, "chi4", origin_step=1), one(sc.FAMILY1, "chi4", origin_step=3)):
        pts, sizes = sc.points(c)[:HEAD], sc.groups_of(c)
        got = sc.restate_chi4(pts, sizes, sc.CHI4_CUTOFFS, c.lags, sc.DIMS, c.origin_step)
        want = tchi4.restate(pts, sizes, sc.CHI4_CUTOFFS, c.lags, origin_step=c.origin_step, dims=sc.DIMS)
        for g, w in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(g, w)
        assert got[3] == want[3]


def test_vectorised_distinct_van_hove_is_the_modules_own():
    for c in (one(sc.FAMILY1, "vhd", origin_step=1), one(sc.FAMILY1, "vhd", origin_step=3)):
        pts = sc.points(c)[:HEAD]
        got = sc.restate_vhd(pts, sc.N1, sc.VHD_EDGES, c.lags, sc.DIMS, c.origin_step, chunk=64)
        want = tvhd.restate(pts[:, :sc.N1], pts[:, sc.N1:], sc.VHD_EDGES, c.lags, sc.DIMS, origin_step=c.origin_step)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert got[2] == want[2] and want[0].sum() > 0


def test_vectorised_survival_is_the_modules_own():
    for c in (one(sc.FAMILY1, "prs", origin_step=1), one(sc.FAMILY1, "prs", origin_step=3)):
        pts = sc.points(c)[sc.LIMIT - 200:sc.LIMIT + 100]
        h = sc.contact_matrix(pts, sc.N1, sc.DIMS, chunk=64)
        got = sc.survival(h, c.lags, c.origin_step)
        want = tprs.restate(pts[:, :sc.N1], pts[:, sc.N1:], sc.CUTOFF, c.lags, sc.DIMS, origin_step=c.origin_step)
        for key in tprs.KEYS:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        np.testing.assert_array_equal(h.sum(axis=(1, 2)), want["contacts"])
        assert 0 < want["continuous"][-1] < want["intermittent"][-1]
    # a lag that no origin reaches, and one that a single origin reaches
    got = sc.survival(h, (299, 300, 5000), 1)
    assert got["origin_counts"].tolist() == [int(h[0].sum()), 0, 0]


def test_vectorised_bonds_are_the_modules_own():
    c = one(sc.FAMILY1, "hb", origin_step=3)
    pts = sc.points(c)[sc.LIMIT - 200:sc.LIMIT + 100]
    b = sc.bond_matrix(pts, sc.HB_BOX, chunk=64)
    want = hbc.restate(pts, *hbc.water_tables(sc.HB_MOLECULES), sc.HB_DISTANCE, hbc.cos_of(sc.HB_ANGLE), c.lags,
                       sc.HB_BOX, origin_step=3, max_neighbors=sc.max_neighbors(c))
    np.testing.assert_array_equal(b, want["bond"])
    got = sc.survival(b, c.lags, 3)
    for key in hbc.KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert want["degenerate"] == 0 and 0 < want["continuous"][-1] < want["intermittent"][-1]
    # and with the first oxygens alone as acceptors, as in the history-bound case
    c = one(sc.FAMILY2, "hb")
    s, = sc.seams(c)
    pts, tables = sc.points(c)[s - 20:s + 3], sc.hb_tables(c)
    assert len(tables[2]) == sc.MID_HB_ACCEPTORS == 10 and len(tables[0]) == 666
    want = hbc.restate(pts, *tables, sc.HB_DISTANCE, hbc.cos_of(sc.HB_ANGLE), (0, 1, 3), sc.MID_HB_BOX,
                       max_neighbors=sc.max_neighbors(c))
    np.testing.assert_array_equal(sc.bond_matrix(pts, sc.MID_HB_BOX, chunk=8, acceptors=10), want["bond"])
    assert want["evaluations"] == len(pts) * (666 * 10 - 20) and want["bonds"].min() >= 1


def test_vectorised_orientation_is_the_modules_own():
    c = one(sc.FAMILY1, "ori")
    pts, sizes, pairs = sc.points(c)[:HEAD], sc.groups_of(c), sc.ori_pairs(sc.N)
    acc, frame_sums, evaluations = sc.restate_ori(pts, sizes, pairs, c.lags, sc.DIMS, tori)
    want = tori.restate(pts, sizes, pairs, c.lags, dims=sc.DIMS)
    np.testing.assert_array_equal(acc, want[1])
    np.testing.assert_array_equal(frame_sums, want[2])
    assert evaluations == want[3]


def test_vectorised_angles_are_the_modules_own():
    c = one(sc.FAMILY1, "ang")
    pts = sc.points(c)[sc.LIMIT - 200:sc.LIMIT + 100]
    counts, degenerate = sc.restate_ang(pts, sc.N1, sc.ANG_THRESHOLDS, sc.DIMS, chunk=64)
    want = tang.restate(pts, sc.N1, [sc.N2], sc.CUTOFF, sc.ANG_THRESHOLDS, sc.DIMS)
    np.testing.assert_array_equal(counts, want["counts"][0])
    assert degenerate == want["degenerate"][0] == 0 and counts.sum() == want["triplets"] > 0
