"""
Every RDF kernel route against the fp64 contract: the cases of ``rdf_cases.py`` run through ``RdfEngine`` in their
stated environment, the plan is asserted, and the counts must EQUAL those of ``oracle.cbind.c_radial_histogram`` (the
fp64 restatement of the contract) summed over the frames — integers, no tolerance.  The conditions that keep a case
from passing vacuously are checked on the CPU against the oracle alone; the statistics a case claims, on the GPU.
"""
import functools

import numpy as np
import pytest

import rdf_cases as rc
from mdhelper_amd import _core
from oracle.cbind import c_radial_histogram, max_threads

OMP_THREADS = max_threads()     # the oracle keeps the thread count of its last call: the per-frame loops give it back


def _restore_threads():
    c_radial_histogram(np.zeros((1, 3)), np.zeros((1, 3)), 1, (0.0, 1.0), None, n_threads=OMP_THREADS)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(c for c in rc.CASES if c.name == name)
    pos1, pos2, boxes = rc.positions(c)
    want = np.zeros(c.bins, dtype=np.int64)
    for f in range(c.frames):
        c_radial_histogram(pos1[f], pos1[f] if pos2 is None else pos2[f], c.bins, c.range,
                           None if boxes is None else boxes[f], exclusion=c.excl, counts=want)
    for a in (pos1, pos2, boxes, want):
        if a is not None:
            a.setflags(write=False)
    return pos1, pos2, boxes, want


@pytest.mark.parametrize("group", sorted({c.group for c in rc.CASES}))
def test_no_case_is_vacuous(group):
    """At least 1 000 pairs binned, pairs in the first and the last bin wherever the case claims the range ends, and
    the lattice constructions' own pairs (those exactly at r0 and r1 among them) where the counts are known."""
    for c in (c for c in rc.CASES if c.group == group):
        want = _inputs(c.name)[3]
        if "tiny" in c.claims:
            assert c.n1 == 1 and c.n2 is None and want.sum() == want[0] == (c.frames if c.excl is None else 0), c.name
            continue
        assert want.sum() >= 1000, (c.name, int(want.sum()))
        if "lattice" in c.claims:
            counts, exact = rc.lattice_counts(c)
            assert np.array_equal(want, counts) if exact else np.all(want >= counts), (c.name, want, counts)
            assert counts[0] > 0 and counts[-1] > 0
        if "ends" in c.claims:
            assert want[0] > 0 and want[-1] > 0, (c.name, int(want[0]), int(want[-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.CASES, ids=lambda c: c.name)
def test_route(c, monkeypatch):
    pos1, pos2, boxes, want = _inputs(c.name)
    rc.set_env(monkeypatch, c.env)
    p = _core.RdfEngine.plan(rc.edges_of(c), c.excl, c.algo, c.n1, c.n2, c.box, c.frames)
    assert {k: p[k] for k in c.plan} == c.plan
    for _ in range(c.repeats):
        eng = _core.RdfEngine(rc.edges_of(c), c.excl, algo=c.algo)
        eng.accumulate(pos1, pos2, boxes)
        got, st, ran = eng.counts(), eng.stats(), eng.last_plan()
        eng.close()
        # what was launched is what was planned (the host route cuts a call into pieces of its own, each a run with
        # slabs of its own: the two slab fields describe the last piece, not the call)
        assert {k: v for k, v in ran.items() if k not in ("slab_frames", "n_slabs")} == \
            {k: v for k, v in p.items() if k not in ("slab_frames", "n_slabs")}
        assert np.array_equal(got, want), (np.nonzero(got - want)[0][:10], (got - want)[np.nonzero(got - want)[0][:10]])
        assert st["pairs_evaluated"] == c.frames * c.n1 * (c.n1 if c.n2 is None else c.n2)
        if "exact" in c.claims:
            assert st["pairs_exact"] > 0, st
        if "general" in c.claims:
            assert st["cell_units_general"] > 0, st
        if "culled" in c.claims:
            assert 0 < st["pairs_computed"] < st["pairs_evaluated"] / 2, st
        if c.family in (2, 4) and "tiny" not in c.claims:
            assert st["cell_units"] > 0, st


# ------------------------------------------------------------------------------------------- family E: frame seams

@functools.lru_cache(maxsize=None)
def _seam(tri):
    pos, boxes = rc.seam_inputs(tri)
    if tri:
        want = np.zeros(rc.SEAM_BINS, dtype=np.int64)
        for f in range(rc.SEAM_FRAMES):
            c_radial_histogram(pos[f], pos[f], rc.SEAM_BINS, rc.SEAM_RANGE, boxes[f], exclusion=rc.SEAM_EXCL,
                               n_threads=1, counts=want)
        _restore_threads()
    else:
        want = rc.ortho_restatement(pos, boxes, rc.SEAM_BINS, rc.SEAM_RANGE, rc.SEAM_EXCL)
    for a in (pos, boxes, want):
        a.setflags(write=False)
    return pos, boxes, want


def test_the_restatement_of_the_seam_cases_is_the_oracle():
    """The vectorised numpy restatement of the orthorhombic contract against the C oracle, frame by frame, on 64
    frames that include both sides of the seam; and the seam cases bin pairs in every frame around it."""
    pos, boxes, want = _seam(False)
    frames = np.r_[0:30, 32750:32769, 5000:5015]
    for f in frames:
        one = c_radial_histogram(pos[f], pos[f], rc.SEAM_BINS, rc.SEAM_RANGE, boxes[f], exclusion=rc.SEAM_EXCL, n_threads=1)
        assert np.array_equal(rc.ortho_restatement(pos[f:f + 1], boxes[f:f + 1], rc.SEAM_BINS, rc.SEAM_RANGE,
                                                   rc.SEAM_EXCL), one), f
    _restore_threads()
    assert np.array_equal(rc.ortho_restatement(pos[frames], boxes[frames], rc.SEAM_BINS, rc.SEAM_RANGE, rc.SEAM_EXCL),
                          sum(rc.ortho_restatement(pos[f:f + 1], boxes[f:f + 1], rc.SEAM_BINS, rc.SEAM_RANGE,
                                                   rc.SEAM_EXCL) for f in frames))
    assert want.sum() > 100000
    for tri in (False, True):
        pos, boxes, _ = _seam(tri)
        last = c_radial_histogram(pos[-1], pos[-1], rc.SEAM_BINS, rc.SEAM_RANGE, boxes[-1], exclusion=rc.SEAM_EXCL)
        assert last.sum() > 0 and len(np.unique(boxes[:, 0])) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True], ids=["one call", "32768 + 1"])
@pytest.mark.parametrize("c", rc.SEAM_CASES, ids=lambda c: c.name)
def test_frame_seam(c, split, monkeypatch):
    """32 769 frames resident on the device: one past the slab length and the grid-z cap of every route, as one run
    (the engine cuts it at frame 32 768 and reports the slabs) and as two calls cut at the seam."""
    pos, boxes, want = _seam(c.tri)
    rc.set_env(monkeypatch, c.env)
    edges = np.linspace(rc.SEAM_RANGE[0], rc.SEAM_RANGE[1], rc.SEAM_BINS + 1)
    p = _core.RdfEngine.plan(edges, rc.SEAM_EXCL, c.algo, rc.SEAM_N, None, boxes, rc.SEAM_FRAMES)
    assert (p["family"], p["slab_frames"], p["n_slabs"]) == (c.family, 32768, 2)
    d_pos, d_boxes = _core.DeviceArray.from_host(pos), _core.DeviceArray.from_host(boxes)
    d_pos1, d_boxes1 = _core.DeviceArray.from_host(pos[32768:]), _core.DeviceArray.from_host(boxes[32768:])
    eng = _core.RdfEngine(edges, rc.SEAM_EXCL, algo=c.algo)
    try:
        if split:
            eng.accumulate_device(d_pos.ptr, rc.SEAM_N, None, rc.SEAM_N, d_boxes.ptr, 32768)
            eng.accumulate_device(d_pos1.ptr, rc.SEAM_N, None, rc.SEAM_N, d_boxes1.ptr, 1)
        else:
            eng.accumulate_device(d_pos.ptr, rc.SEAM_N, None, rc.SEAM_N, d_boxes.ptr, rc.SEAM_FRAMES)
        got, st = eng.counts(), eng.stats()
    finally:
        eng.close()
        for a in (d_pos, d_boxes, d_pos1, d_boxes1):
            a.free()
    assert np.array_equal(got, want), np.nonzero(got - want)[0]
    assert st["pairs_evaluated"] == rc.SEAM_FRAMES * rc.SEAM_N ** 2
    # one pair launch per slab: 32 768 + 1 on every route, whether the engine cut the run or the caller did
    beside = not split and st["slabs_sorted_beside"] > 0
    assert st["launches"] == (3 if beside else 2), st
    if c.env:
        assert st["slabs_sorted_beside"] == 0
