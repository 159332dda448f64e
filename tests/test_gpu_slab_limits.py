"""
The lag and pair engines at their default slab and launch limits: launches of 32 768 frames, the engine's own seam
inside one call, rings sized by default and their wrap, the origin batches of the survival walk and full wave counters
of the van Hove kernel.  The cases, and where ``engine.plan()`` puts their seams, are in ``slab_limit_cases.py``;
``test_slab_limits_host.py`` checks them on the CPU.

Every case is compared twice.

Split invariance, bit for bit: a second engine of the same configuration with ``set_slab_frames(1024)`` is given the
same frames by the device route in calls of 1 000 frames, the small-slab regime the engines' own modules pin; every
output of the two must be equal (``assert_array_equal``): these engines count in integers or add every float64
accumulator in frame order, which is what their own modules assert for splits into calls and slabs.

Definition: the sums that no frame owns against the float64 restatement of all frames (``slab_limit_cases.restate_*``,
proved equal to the modules' own restatements by the host test; the first group of the 5 592-point cases), per-frame
outputs at frame 0, the three frames around every seam and the last frame against the restatement of the engine's own
module, with that module's exactness rule or tolerance as it stands; ``stats()`` against the contract's counts.
"""
import numpy as np
import pytest

import bond_order_cases as bc
import slab_limit_cases as sc
import test_gpu_cluster as tclu
import test_gpu_dipole as tdip
import test_gpu_orientation as tori
from mdhelper_amd import _core

pytestmark = pytest.mark.gpu

STATS = ("frames", "evaluations", "max_row", "degenerate", "triplets", "bonds")


# ------------------------------------------------------------------------------------------------ the engines

def outputs(eng, c):
    """Every output of the engine, by name."""
    if c.engine == "dip":
        out = {"rows": eng.result()}
    elif c.engine == "vh":
        counts, moments = eng.result()
        out = {"counts": counts, "moments": moments, "point_moments": eng.point_moments()}
    elif c.engine == "chi4":
        out = dict(zip(("sums", "square_sums", "n_origins"), eng.result()))
    elif c.engine == "vhd":
        out = {"counts": eng.result()}
    elif c.engine == "prs":
        out = dict(eng.result(), contacts=eng.contacts())
    elif c.engine == "hb":
        out = dict(eng.result(), bonds_per_frame=eng.bonds(), **eng.geometry())
    elif c.engine == "clu":
        out = dict(eng.result(), **eng.frames())
    elif c.engine == "ang":
        out = eng.result()
    elif c.engine == "ori":
        out = {"sums": eng.result(), "vector_sums": eng.vector_sums(), "frame_sums": eng.frame_sums()}
    else:
        frames = eng.frames()
        out = dict(eng.result(), frame_sums=frames["sums"], counted=frames["counted"])
    stats = eng.stats()
    out.update({f"stats {key}": np.array(stats[key]) for key in STATS if key in stats})
    return out


def run(c, rows, d_rows, calls, route, *, slab=0, index=None, reslab=None):
    """The outputs of a fresh engine of the case given the frames in the calls `calls` by `route`; reslab = (call
    number, frames): the dipole engine's slab changed before that call."""
    start = sc.points(c)[0].astype(np.float64) if c.engine == "dip" else None
    eng = sc.make_engine(c, start)
    try:
        if slab:
            eng.set_slab_frames(slab)
        for k, (a, b) in enumerate(zip(calls[:-1], calls[1:])):
            if reslab and k == reslab[0]:
                eng.set_slab_frames(reslab[1])
            if route == "host":
                eng.accumulate(rows[a:b])
            else:
                eng.accumulate_device(d_rows.rows(a, b - a).ptr, d_rows.shape[1], b - a, index)
        eng.synchronize()
        assert eng.stats()["frames"] == calls[-1] - calls[0]
        return outputs(eng, c)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the definitions

def assert_equal(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def check_dip(c, got, frames):
    pts, dims, sizes = sc.points(c)[:c.calls[-1]], sc.dims_of(c), sc.groups_of(c)
    q = sc.dip_charges(pts.shape[1])
    images = tdip.unwrap_ref(pts, pts[0].astype(np.float64), dims)
    assert any(images[s].any() and (images[s] != images[s - 1]).any() for s in sc.seams(c))
    want, tol = tdip.sums_ref(tdip.terms_ref(pts[frames], q, images[frames], dims), sizes)
    tdip.assert_within(got["rows"][:, frames], want, tol)


def check_vh(c, got, frames):
    pts, sizes, F = sc.points(c)[:c.calls[-1]], sc.groups_of(c), c.calls[-1]
    if c.family == 4:
        # closed form: every displacement is 0, in bin 0, for every point and every frame pair of the lag
        want = np.zeros_like(got["counts"])
        for k, lag in enumerate(c.lags):
            want[k, :, 0] = [n * (F - lag) for n in sizes]
        assert_equal(got["counts"], want, "counts")
        assert not got["moments"].any() and not got["point_moments"].any()
        assert got["stats evaluations"] == sum(sizes) * sum(F - lag for lag in c.lags)
        return
    n = sum(sizes) if c.family == 1 else sizes[0]       # family 2: the first group, whose points are followed alone
    G = len(sizes) if c.family == 1 else 1
    counts, moments, acc, evaluations = sc.restate_vh(pts[:, :n], sizes[:G], sc.vh_edges(c), c.lags, sc.dims_of(c))
    assert_equal(got["counts"][:, :G], counts, "counts")
    assert_equal(got["moments"][:, :G], moments, "moments")
    assert_equal(got["point_moments"][:, :n], acc, "point moments")
    assert int(got["stats evaluations"]) * n == evaluations * sum(sizes)
    assert counts[-1].sum() > 0 and moments[-1].min() > 0


def check_chi4(c, got, frames):
    pts, sizes = sc.points(c)[:c.calls[-1]], sc.groups_of(c)
    n = sum(sizes) if c.family == 1 else sizes[0]
    G = len(sizes) if c.family == 1 else 1
    s1, s2, origins, evaluations = sc.restate_chi4(pts[:, :n], sizes[:G], sc.CHI4_CUTOFFS, c.lags, sc.dims_of(c),
                                                   c.origin_step)
    assert_equal(got["sums"][:, :G], s1, "sums")
    assert_equal(got["square_sums"][:, :G], s2, "square sums")
    assert_equal(got["n_origins"], origins, "origins")
    assert int(got["stats evaluations"]) * n == evaluations * sum(sizes)
    assert 0 < s1[1, 0, 0] < s1[1, 0, -1] and s1[-1, 0, -1] > 0     # the cutoffs separate the displacements


def check_vhd(c, got, frames):
    pts = sc.points(c)[:c.calls[-1]]
    counts, n_origins, evaluations = sc.restate_vhd(pts, sc.groups_of(c)[0], sc.VHD_EDGES, c.lags, sc.dims_of(c),
                                                    c.origin_step, chunk=4096 if c.family == 1 else 32)
    assert_equal(got["counts"], counts, "counts")
    assert got["stats evaluations"] == evaluations and counts[-1].sum() > 0


def check_survival(c, got, h):
    want = sc.survival(h, c.lags, c.origin_step)
    for key in ("intermittent", "origin_counts"):
        assert_equal(got[key], want[key], key)
    assert_equal(got["continuous"], want["continuous"] if c.continuous else np.zeros_like(want["continuous"]),
                 "continuous")
    assert 0 < want["intermittent"][-1] < want["origin_counts"][-1]
    if c.family == 1:       # a contact that lives through the longest lag, and one that does not
        assert 0 < want["continuous"][-1] < want["intermittent"][-1]


def check_prs(c, got, frames):
    F, (n1, n2), dims = c.calls[-1], sc.groups_of(c), sc.dims_of(c)
    pts = sc.points(c)[:F]
    assert got["stats evaluations"] == F * n1 * n2
    h = sc.contact_matrix(pts, n1, dims)
    assert_equal(got["contacts"], h.sum(axis=(1, 2)), "contacts")
    assert got["stats max_row"] == h.sum(axis=2).max() <= sc.max_neighbors(c)
    check_survival(c, got, h)


def check_hb(c, got, frames):
    F, dims = c.calls[-1], sc.dims_of(c)
    pts = sc.points(c)[:F]
    n_mol, n_a = pts.shape[1] // 3, len(sc.hb_tables(c)[2])
    # every accepting oxygen is the donor of its own two hydrogens: those pairs are not evaluated
    assert got["stats evaluations"] == F * (2 * n_mol * n_a - 2 * n_a) and got["stats degenerate"] == 0
    assert got["distance_counts"].sum() == got["cosine_counts"].sum() == got["bonds_per_frame"].sum()
    assert got["donated"].sum() == F * 2 * n_mol
    b = sc.bond_matrix(pts, dims, chunk=4096 if c.family == 1 else 256, acceptors=n_a)
    assert_equal(got["bonds_per_frame"], b.sum(axis=(1, 2)), "bonds")
    assert_equal(got["donated"], np.bincount(b.sum(axis=2).ravel(), minlength=sc.max_neighbors(c) + 1), "donated")
    assert got["stats max_row"] == b.sum(axis=2).max()
    check_survival(c, got, b)


def check_clu(c, got, frames):
    F, (n1, n2), dims = c.calls[-1], sc.groups_of(c), sc.dims_of(c)
    n = n1 + n2
    species = np.repeat([0, 1], (n1, n2))
    want = tclu.restate(sc.points(c)[frames], species, [[0.0, sc.CUTOFF], [sc.CUTOFF, 0.0]], dims)
    for key in ("bonds", "n_clusters", "largest", "sum_squares"):
        assert_equal(got[key][frames], want[key], key)
    assert got["stats evaluations"] == F * (n * (n - 1) // 2)
    # what follows from the definitions over all frames
    s = np.arange(n + 1)
    assert_equal(got["species_counts"].sum(axis=0), s * got["size_counts"], "species counts")
    assert got["size_counts"].sum() == got["n_clusters"].sum() and (s * got["size_counts"]).sum() == F * n
    assert (s * s * got["size_counts"]).sum() == got["sum_squares"].sum()
    # unlike pairs only: the bonds of a frame are the contacts of the residence cases, the rows those of either set
    h = sc.contact_matrix(sc.points(c)[:F], n1, dims)
    assert_equal(got["bonds"], h.sum(axis=(1, 2)), "bonds of every frame")
    assert got["stats max_row"] == max(h.sum(axis=2).max(), h.sum(axis=1).max()) <= sc.max_neighbors(c)


def check_ang(c, got, frames):
    F, (n1, n2) = c.calls[-1], sc.groups_of(c)
    assert got["stats evaluations"] == F * n1 * n2
    assert got["coordination"].sum() == F * n1
    assert got["counts"].sum() + got["degenerate"].sum() == got["stats triplets"] and not got["degenerate"].any()
    # the coordination and the triplets of all frames from the contacts of the residence cases
    rows = sc.contact_matrix(sc.points(c)[:F], n1, sc.dims_of(c)).sum(axis=2)
    assert_equal(got["coordination"][0], np.bincount(rows.ravel(), minlength=sc.max_neighbors(c) + 1), "coordination")
    assert got["stats triplets"] == (rows * (rows - 1) // 2).sum() and got["stats max_row"] == rows.max()
    counts, degenerate = sc.restate_ang(sc.points(c)[:F], n1, sc.ANG_THRESHOLDS, sc.dims_of(c))
    assert_equal(got["counts"][0], counts, "counts")
    assert degenerate == 0 and counts.sum() > 0


def check_ori(c, got, frames):
    F, sizes, dims = c.calls[-1], sc.groups_of(c), sc.dims_of(c)
    pts = sc.points(c)[:F]
    V = sum(sizes) if c.family == 1 else sizes[0]       # family 2: the vectors of the first group
    G = len(sizes) if c.family == 1 else 1
    acc, frame_sums, evaluations = sc.restate_ori(pts, sizes[:G], sc.ori_pairs(pts.shape[1])[:V], c.lags, dims, tori)
    assert_equal(got["vector_sums"][:, :V], acc, "vector sums")
    assert_equal(got["frame_sums"][:, :G], frame_sums, "frame sums")
    lo = 0
    for g, size in enumerate(sizes[:G]):
        s = np.zeros((len(c.lags), 2))
        for v in range(lo, lo + size):                  # a group's vectors in row order
            s = s + acc[:, v, :]
        assert_equal(got["sums"][:, g], s, "sums")
        lo += size
    assert int(got["stats evaluations"]) * V == evaluations * sum(sizes) and got["stats degenerate"] == 0


def check_boo(c, got, frames):
    F, (n1, n2), dims = c.calls[-1], sc.groups_of(c), sc.dims_of(c)
    want = bc.restate(sc.points(c)[frames], n1, n2, sc.CUTOFF, sc.BOO_DEGREES, sc.BOO_EDGES, dims,
                      max_neighbors=sc.max_neighbors(c))
    assert_equal(got["frame_sums"][frames], want["sums"], "frame sums")
    assert_equal(got["counted"][frames], want["counted"], "counted")
    assert got["stats evaluations"] == F * n1 * n2 and got["stats degenerate"] == 0
    assert got["coordination"].sum() == F * n1
    assert got["stats bonds"] == (got["coordination"] * np.arange(len(got["coordination"]))).sum()
    assert_equal(got["counts"].sum(axis=-1) + got["outside"], np.full(got["outside"].shape, got["counted"].sum()),
                 "counted values")
    rows = sc.contact_matrix(sc.points(c)[:F], n1, dims).sum(axis=2)
    assert_equal(got["coordination"], np.bincount(rows.ravel(), minlength=sc.max_neighbors(c) + 1), "coordination")
    assert_equal(got["counted"], (rows > 0).sum(axis=1), "counted of every frame")
    assert got["stats max_row"] == rows.max()


CHECKS = {"dip": check_dip, "vh": check_vh, "chi4": check_chi4, "vhd": check_vhd, "prs": check_prs, "hb": check_hb,
          "clu": check_clu, "ang": check_ang, "ori": check_ori, "boo": check_boo}


# ------------------------------------------------------------------------------------------------ the tests

@pytest.fixture(scope="module")
def device_rows():
    """The fed frames of a case's whole walk in HBM (the case's frames are the first ones), kept while consecutive
    cases feed the same array: {index: array} of one walk at a time."""
    held = {}

    def get(c, index):
        key = (c.walk, c.engine == "hb") + ((sc.scripted_seams(c), c.calls[-1]) if c.family == 2 else ())
        if held.get("key") != key:
            for d in held.pop("arrays", {}).values():
                d.free()
            held["key"], held["arrays"] = key, {}
        if index not in held["arrays"]:
            held["arrays"][index] = _core.DeviceArray.from_host(sc.rows(c._replace(index=index), whole=True))
        return held["arrays"][index]

    yield get
    for d in held.pop("arrays", {}).values():
        d.free()
    sc.forget_walks()


def test_the_dipole_plan_is_the_formula_of_the_cases():
    """The dipole engine's create acquires its stream, so its plan is pinned here and not by the host module: 24 B
    per tile of 128 points of a group, 256 MiB of tile sums, 32 768 frames at most."""
    for c in [c for c in sc.ALL_CASES if c.engine == "dip"]:
        eng = sc.make_engine(c)
        try:
            assert eng.plan() == sc.plan(c) == {"slab_frames": min(sc.LIMIT, (256 << 20) // sc.frame_bytes(c)),
                                                "ring_frames": 0}
            eng.set_slab_frames(7)
            assert eng.plan() == {"slab_frames": 7, "ring_frames": 0}
            eng.set_slab_frames(0)
            assert eng.plan() == sc.plan(c)
        finally:
            eng.close()


def test_a_sized_ring_limits_the_plan():
    """Once the first frame has sized the ring, the plan reports that ring, whatever slab the formula would give."""
    c = [c for c in sc.FAMILY1 if c.engine == "vhd"][0]
    eng = sc.make_engine(c)
    try:
        eng.set_slab_frames(5)
        eng.accumulate(sc.rows(c)[:3])
        assert eng.plan() == {"slab_frames": 5, "ring_frames": 45}
        eng.reset()
        eng.set_slab_frames(0)
        assert eng.plan() == {"slab_frames": sc.LIMIT, "ring_frames": 40 + sc.LIMIT}
    finally:
        eng.close()


@pytest.mark.parametrize("c", sc.ALL_CASES, ids=lambda c: c.name)
def test_slab_limit(c, device_rows):
    rows = sc.rows(c)
    assert rows.shape == (c.calls[-1], sc.fed_rows(c), 3) and rows.dtype == np.float32
    index = sc.index_of(c) if c.index else None
    got = run(c, rows, device_rows(c, c.index), c.calls, c.route, index=index)
    split = run(c, None, device_rows(c, False), sc.split_calls(c), "device", slab=sc.SPLIT_SLAB)
    assert got.keys() == split.keys()
    for key in got:
        assert_equal(got[key], split[key], key)
    if c.engine == "dip":   # the slab changed once in the middle of the run: the rows do not depend on it
        again = run(c, None, device_rows(c, False), sc.split_calls(c), "device", slab=sc.SPLIT_SLAB, reslab=(2, 333))
        assert_equal(got["rows"], again["rows"], "rows after a change of slab")
    assert got["stats frames"] == c.calls[-1]
    CHECKS[c.engine](c, got, sc.checked_frames(c))
