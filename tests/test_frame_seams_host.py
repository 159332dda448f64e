"""
The slab plans of the per-frame engines on the CPU (``X.slab_frames`` = ``mdx_X_slab_frames``,
``_core.feed_slab_frames`` = ``mdx_feed_slab_frames``: host arithmetic the accumulate loops call too): every case of
``test_gpu_frame_seams.py`` (``frame_seam_cases.py``) has its seam where the table says, its walk carries unwrap state
across that seam, and its input stays within the byte bound.  The queries touch no device.
"""
import numpy as np
import pytest

import frame_seam_cases as fc
from mdhelper_amd import _core


@pytest.mark.parametrize("c", fc.ALL_CASES, ids=lambda c: c.name)
def test_every_case_has_its_seam_where_the_table_says(c):
    F = c.calls[-1]
    assert c.hi - c.lo == F and fc.input_bytes(c) <= fc.MAX_INPUT_BYTES
    slab = fc.engine_slab(c)
    if c.family == 1:
        # the frame-count limit, in one feed slab; the seam 32 768 frames into the long call
        assert slab == fc.LIMIT and F == c.calls[-2] + fc.LIMIT + 3
        assert fc.feed_slab(c, fc.F1) in (None, fc.F1)
        assert fc.seams(c) == [c.calls[-2] + fc.LIMIT]
        assert c.calls[-2] in (0, fc.FIRST)
    elif c.family == 2:
        # the scratch limits the slab; no feed on the way
        assert slab < fc.LIMIT and F == slab + 3 and c.route == "device" and c.grouped
        assert fc.seams(c) == [slab]
        assert fc.input_bytes(c) <= 128 << 20
    else:
        # at least three feed slabs, so that a staging set is used twice, none longer than the engine's own slab
        feed = fc.feed_slab(c, F)
        assert feed == 1000 and -(-F // feed) >= 3 and (slab is None or feed <= slab)
        assert fc.seams(c) == [1000, 2000]
        assert fc.input_bytes(c) > 128 << 20            # more than two staging sets of 64 MiB
    assert all(0 < f < F for f in fc.seams(c))
    # the comparison run crosses no seam: every call of it lies inside one launch of the case under test
    split = fc.split_calls(c)
    step = max(b - a for a, b in zip(split[:-1], split[1:]))
    assert 2 * step <= min(s for s in (slab, fc.feed_slab(c, F), F) if s)


def test_the_table_holds_what_the_issue_lists():
    names = [c.name for c in fc.ALL_CASES]
    assert len(set(names)) == len(names)
    by = {(c.family, c.engine) for c in fc.ALL_CASES}
    assert by == {(f, e) for f in (1, 2) for e in ("prof", "gyr", "rouse", "msid")} | \
        {(3, e) for e in ("prof", "gyr", "rouse", "msid", "dip", "vh")}
    one = [c for c in fc.FAMILY1 if len(c.calls) == 2]
    two = [c for c in fc.FAMILY1 if len(c.calls) == 3]
    assert [c._replace(name="", hi=0, calls=()) for c in one] == [c._replace(name="", hi=0, calls=()) for c in two]
    for engine in ("gyr", "rouse", "msid"):
        kinds = {(c.grouped, c.unwrap, c.whole, c.index) for c in one if c.engine == engine}
        assert {(False, False, False, False), (False, True, False, False), (True, True, False, False),
                (False, True, False, True)} <= kinds
    assert {(c.grouped, c.whole) for c in one if c.engine == "msid" and c.whole} == {(False, True), (True, True)}
    assert {c.reserve for c in one if c.engine == "rouse"} == {False, True}
    prof = [c for c in one if c.engine == "prof"]
    assert {(c.recenter, c.per_frame) for c in prof} >= {(True, True), (True, False), (False, False)}
    assert any(c.grouped for c in prof) and any(c.index and c.route == "device" for c in prof)
    assert [c.route for c in fc.FAMILY3].count("file") == 1
    assert all(c.recenter or c.grouped for c in fc.FAMILY2 if c.engine == "prof")
    # the lags of the van Hove case reach across both feed seams
    assert max(fc.VH_LAGS) > 1000 and 999 in fc.VH_LAGS


@pytest.mark.parametrize("c", fc.ALL_CASES, ids=lambda c: c.name)
def test_the_walk_carries_state_across_every_seam(c):
    counts = fc.check_crossings(c)
    assert len(counts) == len(fc.seams(c)) and min(counts) >= 1


def test_plans_against_the_worked_examples():
    gyr, prof = _core.GyrationEngine.slab_frames, _core.ProfileEngine.slab_frames
    rouse, msid = _core.ChainProjectionEngine.slab_frames, _core.InternalDistanceEngine.slab_frames
    # 1 024 chains x 8, one-atom molecules, unwrap: (256 MiB) / (32 * 1024 + 36 * 8192) = 819
    assert gyr([1024], [8], grouped=True, unwrap=True) == 819
    assert gyr([1024], [8]) == 8192 and gyr([3, 4], [5, 6]) == fc.LIMIT
    # plain atoms need no scratch at all, whatever their number
    assert prof(10 ** 8) == fc.LIMIT and prof(8192, grouped=True) == 1365 and prof(8192, recenter=True) == 2730
    assert rouse([10 ** 6], [100]) == fc.LIMIT and rouse([1024], [8], grouped=True, unwrap=True) == 910
    # more scratch, fewer frames, never fewer than one
    assert msid([1024], [8], whole=True) >= msid([1024], [8], grouped=True, unwrap=True) >= 1
    assert msid([1024], [8], whole=True) == msid([1024], [8], grouped=True)
    assert gyr([10 ** 4], [10 ** 4], grouped=True, unwrap=True) == 1
    # 64 MiB of rows, at least one frame, at most the call
    assert _core.feed_slab_frames(2001, 5592) == 1000 and _core.feed_slab_frames(10 ** 6, 5593) == 999
    assert _core.feed_slab_frames(7, 24) == 7 and _core.feed_slab_frames(5, 10 ** 8) == 1


def test_plans_refuse_bad_arguments():
    bad = [lambda: _core.feed_slab_frames(0, 10), lambda: _core.feed_slab_frames(10, 0),
           lambda: _core.ProfileEngine.slab_frames(0), lambda: _core.ProfileEngine.slab_frames(2 ** 31 // 3),
           lambda: _core.GyrationEngine.slab_frames([0], [5]), lambda: _core.GyrationEngine.slab_frames([2, 2], [5]),
           lambda: _core.GyrationEngine.slab_frames([], []),
           lambda: _core.ChainProjectionEngine.slab_frames([2 ** 20], [2 ** 20]),
           lambda: _core.ChainProjectionEngine.slab_frames([3], [0]),
           lambda: _core.InternalDistanceEngine.slab_frames([3], [1]),            # a chain needs a bond
           lambda: _core.InternalDistanceEngine.slab_frames([0], [4]),
           lambda: _core.InternalDistanceEngine.slab_frames([3], [4], whole=True, unwrap=True)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert np.isscalar(_core.InternalDistanceEngine.slab_frames([3], [2]))


@pytest.fixture(scope="module", autouse=True)
def _forget_the_walks():
    """The 134 MB walk is not kept for the rest of the session."""
    yield
    fc.forget_walks()
