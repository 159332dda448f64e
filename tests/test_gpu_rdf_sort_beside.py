"""
RDF cell path: the sort of slab k + 1 beside the pair kernel of slab k (mdx_rdf.hip::accumulate_cell with its
cell_sort_beside and cell_slabs, rdf_cell_sort_small_kernel): two sets of sorted copies, a side stream, packed 16-bit
cell counters.

Bin counts must equal the CPU oracle (``oracle.cbind.c_radial_histogram``) bit for bit, and
``stats()["slabs_sorted_beside"]`` says whether the overlapped route ran.  MDX_RDF_SLAB_BYTES shrinks the
slab (33 bytes per padded particle and frame) so that small inputs take several slabs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mdhelper_amd import _core  # noqa: E402
from mdhelper_amd._lib import check, lib  # noqa: E402
from oracle.cbind import c_radial_histogram  # noqa: E402

F_ALL, N1, N2 = 25, 3000, 1000
N1P, N2P = 3072, 1024            # padded to whole 128-particle tiles
RANGE, BINS = (0.5, 11.0), 90


def _edges(n_bins, rng):
    return np.linspace(rng[0], rng[1], n_bins + 1)


def _slab_bytes(frames, *padded):
    return str(frames * 33 * sum(padded))


@pytest.fixture(scope="module")
def walk():
    """25 frames of 3 000 + 1 000 particles, boxes changing per frame (the shapes of test_rdf_cell_many_slabs)."""
    rng = np.random.default_rng(77)
    Ls = (36 + 4 * rng.random((F_ALL, 3))).astype(np.float32)
    boxes = np.concatenate([Ls, np.full((F_ALL, 3), 90, np.float32)], axis=1)
    a = (rng.random((F_ALL, N1, 3)) * Ls[:, None, :]).astype(np.float32)
    b = (rng.random((F_ALL, N2, 3)) * Ls[:, None, :]).astype(np.float32)
    a[:, :200] += Ls[:, None, :] * np.array([2, -1, 1], dtype=np.float32)      # unwrapped images
    for arr in (a, b, boxes):
        arr.setflags(write=False)
    return a, b, boxes


@pytest.fixture(scope="module")
def want_self11(walk):
    """Per-frame oracle counts of the self histogram, exclusion (1, 1)."""
    a, _b, boxes = walk
    out = np.stack([c_radial_histogram(a[f], a[f], BINS, RANGE, boxes[f], exclusion=(1, 1)) for f in range(F_ALL)])
    out.setflags(write=False)
    return out


def _run(eng, calls):
    for args in calls:
        eng.accumulate(*args)
    got, st = eng.counts(), eng.stats()
    eng.close()
    return got, st


@pytest.mark.parametrize("kind", ["self_1_1", "self_4_4", "cross"])
def test_many_slabs_two_sets(monkeypatch, walk, want_self11, kind):
    """23 frames, three per slab: eight slabs over two accumulate calls (5 + 3), both sets in use, a last slab of
    two frames.  Exclusion (1, 1): no sorted originals; (4, 4): sorted originals; cross: two sorts per slab."""
    a, b, boxes = walk
    F = 23
    if kind == "cross":
        monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(3, N1P, N2P))
        want = sum(c_radial_histogram(a[f], b[f], BINS, RANGE, boxes[f]) for f in range(F))
        eng = _core.RdfEngine(_edges(BINS, RANGE), None, algo="cell")
        calls = [(a[:14], b[:14], boxes[:14]), (a[14:F], b[14:F], boxes[14:F])]
    else:
        monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(3, N1P))
        excl = (1, 1) if kind == "self_1_1" else (4, 4)
        want = want_self11[:F].sum(axis=0) if kind == "self_1_1" else \
            sum(c_radial_histogram(a[f], a[f], BINS, RANGE, boxes[f], exclusion=excl) for f in range(F))
        eng = _core.RdfEngine(_edges(BINS, RANGE), excl, algo="cell")
        calls = [(a[:14], None, boxes[:14]), (a[14:F], None, boxes[14:F])]
    got, st = _run(eng, calls)
    assert st["slabs_sorted_beside"] == 4 + 2, st      # every slab of a call but its first
    assert np.array_equal(got, want)


@pytest.mark.parametrize("frames,beside", [(6, 1), (7, 2), (3, 0), (1, 0)])
def test_slab_count_edges(monkeypatch, walk, want_self11, frames, beside):
    """Exactly two slabs, 2 * slab + 1 frames; one slab and a one-frame call take the serial route."""
    a, _b, boxes = walk
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(3, N1P))
    eng = _core.RdfEngine(_edges(BINS, RANGE), (1, 1), algo="cell")
    got, st = _run(eng, [(a[:frames], None, boxes[:frames])])
    assert st["slabs_sorted_beside"] == beside, st
    assert np.array_equal(got, want_self11[:frames].sum(axis=0))


def test_ramp_and_spread_launches(monkeypatch, walk, want_self11):
    """Eight frames per slab: the call ramps up through slabs of 2, 4, 8, 8 and 3 frames.  Launches of fewer than
    eight frames take the pair kernel's `spread` form beside a sort of eight, and the number of blocks left to the
    sort is scaled between slabs of different length."""
    a, _b, boxes = walk
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(8, N1P))
    eng = _core.RdfEngine(_edges(BINS, RANGE), (1, 1), algo="cell")
    got, st = _run(eng, [(a, None, boxes)])
    assert st["slabs_sorted_beside"] == 4, st
    assert np.array_equal(got, want_self11.sum(axis=0))


def test_join_caller_may_overwrite_after_synchronize(monkeypatch, walk, want_self11):
    """accumulate_device returns with work queued on both streams; after synchronize() the caller overwrites the
    trajectory in HBM, and the counts are still those of the frames that were there.  Then reset() and a second
    call on the same engine, on the frames now in place.

    What this does NOT cover: the explicit join at the exit of cell_slabs_forked.  On a successful call every kernel
    on the side stream is already followed by a pair kernel on the handle's stream that waits for it, so the counts
    here would be the same without the join; it matters on the error exits, which no test provokes."""
    a, _b, boxes = walk
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(3, N1P))
    F = 7
    d_traj = _core.DeviceArray.from_host(a[:F])
    d_boxes = _core.DeviceArray.from_host(boxes[:F])
    eng = _core.RdfEngine(_edges(BINS, RANGE), (1, 1), algo="cell")
    eng.accumulate_device(d_traj.ptr, N1, None, N1, d_boxes.ptr, F)
    eng.synchronize()
    other, other_boxes = np.ascontiguousarray(a[F:2 * F]), np.ascontiguousarray(boxes[F:2 * F])
    check(lib().mdx_memcpy_h2d(0, d_traj.ptr, _core._ptr(other), other.nbytes))
    check(lib().mdx_memcpy_h2d(0, d_boxes.ptr, _core._ptr(other_boxes), other_boxes.nbytes))
    got = eng.counts()
    assert eng.stats()["slabs_sorted_beside"] == 2
    assert np.array_equal(got, want_self11[:F].sum(axis=0))
    eng.reset()
    assert eng.stats()["slabs_sorted_beside"] == 0
    eng.accumulate_device(d_traj.ptr, N1, None, N1, d_boxes.ptr, F)
    got = eng.counts()
    st = eng.stats()
    eng.close()
    d_traj.free()
    d_boxes.free()
    assert st["slabs_sorted_beside"] == 2
    assert np.array_equal(got, want_self11[F:2 * F].sum(axis=0))


def test_dense_cells(monkeypatch):
    """6 000 particles, 95 % of them within 0.05 A of forty centres: a packed 16-bit counter holds hundreds."""
    rng = np.random.default_rng(3)
    F, n, L = 4, 6000, np.float32(40.0)
    dims = np.array([L, L, L, 90, 90, 90], dtype=np.float32)
    centres = rng.random((40, 3)) * L
    pos = rng.random((F, n, 3)) * L
    k = int(0.95 * n)
    pos[:, :k] = centres[rng.integers(0, 40, (F, k))] + rng.uniform(-0.05, 0.05, (F, k, 3)) / np.sqrt(3.0)
    pos = pos.astype(np.float32)
    want = sum(c_radial_histogram(pos[f], pos[f], 201, (0.0, 5.0), dims) for f in range(F))
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(2, 6016))
    eng = _core.RdfEngine(_edges(201, (0.0, 5.0)), None, algo="cell")
    got, st = _run(eng, [(pos, None, dims)])
    assert st["slabs_sorted_beside"] == 1, st
    assert np.array_equal(got, want)


def _hist_65k(n, monkeypatch, beside):
    rng = np.random.default_rng(11)
    F, L = 4, np.float32(200.0)
    dims = np.array([L, L, L, 90, 90, 90], dtype=np.float32)
    pos = (rng.random((F, n, 3)) * L).astype(np.float32)
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(2, 65536))
    if beside:
        monkeypatch.delenv("MDX_RDF_SORT_BESIDE", raising=False)
    else:
        monkeypatch.setenv("MDX_RDF_SORT_BESIDE", "0")
    eng = _core.RdfEngine(_edges(60, (0.0, 3.0)), (1, 1), algo="cell")
    return _run(eng, [(pos, None, dims)])


@pytest.mark.parametrize("n,beside", [(65535, 1), (65536, 0)])
def test_selection_guard(monkeypatch, n, beside):
    """Packed counters hold a set of at most 65 535 particles; one more takes the serial route.  (Reference: the
    serial route itself, the code of before — the CPU oracle is too slow at this size.)"""
    got, st = _hist_65k(n, monkeypatch, True)
    ref, st_ref = _hist_65k(n, monkeypatch, False)
    assert st["slabs_sorted_beside"] == beside, st
    assert st_ref["slabs_sorted_beside"] == 0
    assert got.sum() > 0
    assert np.array_equal(got, ref)


def test_switch(monkeypatch, walk, want_self11):
    """MDX_RDF_SORT_BESIDE=0: the serial route, same counts."""
    a, _b, boxes = walk
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", _slab_bytes(3, N1P))
    monkeypatch.setenv("MDX_RDF_SORT_BESIDE", "0")
    eng = _core.RdfEngine(_edges(BINS, RANGE), (1, 1), algo="cell")
    got, st = _run(eng, [(a[:14], None, boxes[:14])])
    assert st["slabs_sorted_beside"] == 0, st
    assert np.array_equal(got, want_self11[:14].sum(axis=0))
