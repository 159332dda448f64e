"""
The per-frame engines across the seams of the two loops that cut a call: their own slab loop (``X_accumulate_rows``:
at most 32 768 frames, or what the scratch of a frame allows, per launch) and the staging feed of the host and file
routes (``mdx_frame_feed.hpp``: 64 MiB of coordinates per slab, two staging sets).  The cases, and where the plan
queries put their seams, are in ``frame_seam_cases.py``; ``test_frame_seams_host.py`` checks them on the CPU.

Every case is compared twice.

Split invariance, bit for bit: a second engine of the same configuration is given the same frames by the device route
in calls of at most half the smaller slab, which cross no seam; every output of the two must be equal
(``assert_array_equal``).  These engines compute each frame by itself or count in integers, which is what their own
modules assert for splits into calls.

Definition at the seam: frame 0, the three frames around every seam and the last frame against the float64
restatement of the engine's own module (``test_gpu_gyradius.py``, ``test_gpu_rouse.py``,
``test_gpu_internal_distances.py``, ``test_gpu_profile.py``, ``test_gpu_dipole.py``, ``test_gpu_vanhove.py``), with that
module's tolerance or exactness rule as it stands; accumulated Profile counts against the restatement of all frames;
the van Hove sums, which no frame owns, against the restatement of all frames of the first group.
"""
import numpy as np
import pytest

import frame_seam_cases as fc
import test_gpu_dipole as tdip
import test_gpu_gyradius as tgyr
import test_gpu_internal_distances as tmsid
import test_gpu_profile as tprof
import test_gpu_rouse as trouse
import test_gpu_vanhove as tvh
from mdhelper_amd import _core
from mdhelper_amd.io import TrajectoryFile

pytestmark = pytest.mark.gpu

ROUSE_MODES = (1, 2, 3)
AXES = (0, 1, 2)


def dip_charges():
    return np.random.default_rng(37).uniform(-1.0, 1.0, fc.FEED_ROWS)


def rouse_weights(c):
    return [trouse.rouse_weights(N, ROUSE_MODES) for N in fc.layout(c)[1]]


# ------------------------------------------------------------------------------------------------ the engines

def make_engine(c):
    _, dims = fc.walk(c.walk)
    n_chains, n_monomers = fc.layout(c)
    F = c.calls[-1]
    if c.engine == "gyr":
        eng = _core.GyrationEngine(n_chains, n_monomers, fc.point_masses(c))
    elif c.engine == "rouse":
        eng = _core.ChainProjectionEngine(n_chains, n_monomers, rouse_weights(c))
    elif c.engine == "msid":
        eng = _core.InternalDistanceEngine(n_chains, n_monomers)
    elif c.engine == "prof":
        eng = _core.ProfileEngine(fc.PROFILE_SIZES[c.walk], AXES, fc.PROFILE_BINS[c.walk], dims,
                                  per_frame=c.per_frame)
    elif c.engine == "dip":
        eng = _core.DipoleEngine(fc.DIP_SIZES, dip_charges())
    else:
        eng = _core.VanHoveEngine(fc.VH_SIZES, fc.VH_EDGES, fc.VH_LAGS)
    try:
        if c.grouped:
            eng.set_grouping(*fc.grouping(c))
        if c.unwrap:
            if c.engine == "vh":
                eng.set_unwrap(dims)
            else:
                eng.set_unwrap(dims, fc.start_of(c))
        if c.whole:
            eng.set_whole(dims)
        if c.recenter:
            eng.set_recenter(0, fc.point_masses(c)[:fc.PROFILE_SIZES[c.walk][0]])
        if c.reserve:
            eng.reserve(F)
    except Exception:
        eng.close()
        raise
    return eng


def outputs(eng, c):
    """Every output of the engine, as a list of arrays."""
    if c.engine == "prof":
        return eng.counts()
    if c.engine == "msid":
        return eng.result()
    if c.engine == "vh":
        counts, moments = eng.result()
        return [counts, moments, eng.point_moments(), np.array(eng.stats()["evaluations"])]
    return [eng.result()]


def run(c, rows, d_rows, cuts, route, tmp_path=None):
    """The outputs of a fresh engine of the case given the frames in the calls `cuts` by `route`."""
    index = fc.index_of(c) if c.index else None
    eng, traj, path = make_engine(c), None, None
    try:
        if route == "file":
            from trajfiles import write_dcd
            path = tmp_path / "seam.dcd"
            write_dcd(path, rows)
            traj = TrajectoryFile(path)
            assert traj.n_atoms == fc.fed_rows(c) and traj.n_frames == len(rows)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if route == "host":
                eng.accumulate(rows[a:b])
            elif route == "device":
                eng.accumulate_device(d_rows.rows(a, b - a).ptr, rows.shape[1], b - a, index)
            else:
                eng.accumulate_traj(traj, np.arange(a, b))
        eng.synchronize()
        assert eng.stats()["frames"] == cuts[-1]
        return outputs(eng, c)
    finally:
        eng.close()
        if traj is not None:
            traj.close()
        if path is not None:
            path.unlink(missing_ok=True)        # 134 MB that pytest would keep for three sessions


# ------------------------------------------------------------------------------------------------ the definitions

_POINTS = {}


def whole_walk(c):
    """The case with the frames of its whole walk: what the cached references are computed for."""
    F = fc.WALKS[c.walk][0]
    return c._replace(lo=0, hi=F, calls=(0, F), index=False)


def reference_points(c, what, compute):
    """float64 points of every frame of the case's walk (its frames are the first ones), computed once per engine,
    walk and grouping; references of the 134 MB walk are kept one at a time."""
    key = (c.engine, c.walk, c.grouped, what)
    if key not in _POINTS:
        if c.walk == "big":
            for k in [k for k in _POINTS if k[1] == "big"]:
                del _POINTS[k]
        w = whole_walk(c)
        _POINTS[key] = compute(w, fc.rows(w))
    return _POINTS[key]


def chain_points(c, mod):
    """The points the chain engines work on, all frames of the walk: the module's own centres and unwrap rule."""
    _, dims = fc.walk(c.walk)
    size = fc.atoms_per_point(c)

    def compute(w, rows):
        pts = mod.centres_ref(rows, size, fc.masses_of(w)) if w.grouped else rows.astype(np.float64)
        if not c.unwrap:
            return pts
        margin = []
        out = mod.unwrap_ref(pts, fc.start_of(w), dims, margin)
        assert min(margin) > fc.MIN_MARGIN
        return out

    return reference_points(c, "unwrap" if c.unwrap else "raw", compute)


def check_gyr(c, got, frames):
    pts = chain_points(c, tgyr)[frames]
    want = tgyr.radii_ref(pts, fc.point_masses(c), *fc.layout(c))
    np.testing.assert_allclose(got[0][:, frames], want, rtol=tgyr.RTOL, atol=0)


def check_rouse(c, got, frames):
    pts = chain_points(c, trouse)[frames]
    n_chains, n_monomers = fc.layout(c)
    want = trouse.amplitudes_ref(pts, n_chains, n_monomers, rouse_weights(c))
    np.testing.assert_allclose(got[0][frames], want, rtol=0, atol=trouse.atol_for(max(n_monomers), pts))


def check_msid(c, got, frames):
    _, dims = fc.walk(c.walk)
    n_chains, n_monomers = fc.layout(c)
    pts = chain_points(c, tmsid)[frames]
    if c.whole:
        margin, parts, lo = [], [], 0
        for M, N in zip(n_chains, n_monomers):
            parts.append(tmsid.whole_ref(pts[:, lo:lo + M * N], M, N, dims, margin))
            lo += M * N
        assert min(margin) > fc.MIN_MARGIN
        pts = np.concatenate(parts, axis=1)
    want = tmsid.internal_ref(pts, n_chains, n_monomers)
    for g, w, M, N in zip(got, want, n_chains, n_monomers):
        tmsid.check(g[frames], w, M, N)


def check_prof(c, got, frames):
    _, dims = fc.walk(c.walk)
    sizes, bins = fc.PROFILE_SIZES[c.walk], fc.PROFILE_BINS[c.walk]
    size = fc.atoms_per_point(c)

    def compute(w, rows):
        pts = tprof.centres_ref(rows, size, fc.masses_of(w)) if w.grouped else rows.astype(np.float64)
        if c.recenter:
            pts = tprof.recentre_ref(pts, dims, slice(0, sizes[0]), fc.point_masses(w)[:sizes[0]], dims / 2)
        return pts

    F = c.calls[-1]
    pts = reference_points(c, "recentred" if c.recenter else "raw", compute)[:F]
    exact = not (c.grouped or c.recenter)           # float32 coordinates binned as they are: no edge can be missed
    if c.per_frame:
        assert exact or tprof.edge_distance(pts[frames], AXES, bins, dims) > tprof.DELTA
        want = tprof.counts_ref(pts[frames], sizes, AXES, bins, dims, average=False)
        tprof.assert_counts([g[:, frames] for g in got], want)
        for g in got:       # and every group's points are counted once in every frame of the run
            np.testing.assert_array_equal(g.sum(axis=-1), np.repeat(np.array(sizes)[:, None], F, axis=1))
    else:
        assert exact or tprof.edge_distance(pts, AXES, bins, dims) > tprof.DELTA
        # the totals over all frames are the histogram of all frames' points: one long frame, group after group
        offs = np.concatenate(([0], np.cumsum(sizes)))
        long = np.concatenate([pts[:, a:b].reshape(1, -1, 3) for a, b in zip(offs[:-1], offs[1:])], axis=1)
        tprof.assert_counts(got, tprof.counts_ref(long, [F * s for s in sizes], AXES, bins, dims))


def check_dip(c, got, frames):
    _, dims = fc.walk(c.walk)
    q = dip_charges()
    images = reference_points(c, "images", lambda w, rows: tdip.unwrap_ref(rows, fc.start_of(w), dims))
    want, tol = tdip.sums_ref(tdip.terms_ref(fc.rows(c)[frames], q, images[frames], dims), fc.DIP_SIZES)
    tdip.assert_within(got[0][:, frames], want, tol)


def check_vh(c, got, frames):
    """No frame owns a van Hove sum: all frames of the first group, whose points the restatement follows alone."""
    _, dims = fc.walk(c.walk)
    n = fc.VH_SIZES[0]
    counts, moments, acc, evaluations = tvh.restate(fc.rows(c)[:, :n], [n], fc.VH_EDGES, fc.VH_LAGS, dims=dims)
    np.testing.assert_array_equal(got[0][:, :1], counts)
    np.testing.assert_array_equal(got[1][:, :1], moments)
    np.testing.assert_array_equal(got[2][:, :n], acc)
    assert int(got[3]) * n == evaluations * fc.FEED_ROWS
    assert counts[-1].sum() > 0 and moments[-1].min() > 0            # the longest lag has origins before both seams


CHECKS = {"gyr": check_gyr, "rouse": check_rouse, "msid": check_msid, "prof": check_prof, "dip": check_dip,
          "vh": check_vh}


# ------------------------------------------------------------------------------------------------ the tests

@pytest.fixture(scope="module")
def device_rows():
    """The fed frames of a case's whole walk in HBM (the case's frames are the first ones), kept while consecutive
    cases feed the same array."""
    held = {}

    def get(c):
        key = (c.walk, fc.atoms_per_point(c), c.index)
        if held.get("key") != key:
            if "d" in held:
                held.pop("d").free()
            held["key"], held["d"] = key, _core.DeviceArray.from_host(fc.rows(whole_walk(c)._replace(index=c.index)))
        return held["d"]

    yield get
    if "d" in held:
        held.pop("d").free()
    _POINTS.clear()
    fc.forget_walks()


@pytest.mark.parametrize("c", fc.ALL_CASES, ids=lambda c: c.name)
def test_seam(c, device_rows, tmp_path):
    rows = fc.rows(c)
    assert rows.shape == (c.calls[-1], fc.fed_rows(c), 3) and rows.dtype == np.float32
    d_rows = device_rows(c)
    got = run(c, rows, d_rows, c.calls, c.route, tmp_path)
    split = run(c, rows, d_rows, fc.split_calls(c), "device")
    assert len(got) == len(split)
    for g, s in zip(got, split):
        np.testing.assert_array_equal(g, s)
    CHECKS[c.engine](c, got, fc.checked_frames(c))
