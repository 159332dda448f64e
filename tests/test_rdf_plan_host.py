"""
``mdx_rdf_plan`` on the CPU: every case of ``test_gpu_rdf_routes.py`` plans to the kernel family, template arguments and
histogram form it states, in the environment it runs in; together the cases reach all 56 instantiations of the three
pair kernels; the replica counts step at the stated bin counts; the slab arithmetic of every route holds at its caps;
bad arguments and bin edges that ``numpy.linspace`` would not yield are refused before any device is touched.
"""
from ctypes import byref, c_void_p

import numpy as np
import pytest

import rdf_cases as rc
from mdhelper_amd import _core, _lib

plan = _core.RdfEngine.plan


def plan_of(c, monkeypatch):
    rc.set_env(monkeypatch, c.env)
    return plan(rc.edges_of(c), c.excl, c.algo, c.n1, c.n2, c.box, c.frames)


def test_families_are_named_as_the_library_numbers_them():
    assert _core.RdfEngine.FAMILIES == rc.FAMILIES


@pytest.mark.parametrize("group", sorted({c.group for c in rc.CASES}))
def test_every_case_plans_to_what_it_states(group, monkeypatch):
    wrong = []
    for c in (c for c in rc.CASES if c.group == group):
        p = plan_of(c, monkeypatch)
        bad = {k: (p[k], v) for k, v in c.plan.items() if p[k] != v}
        if bad:
            wrong.append((c.name, bad))
    assert not wrong, wrong


def test_the_cases_reach_every_instantiation(monkeypatch):
    reached = {rc.instantiation(plan_of(c, monkeypatch)) for c in rc.CASES}
    assert len(rc.ALL_INSTANTIATIONS) == 56
    assert reached <= rc.ALL_INSTANTIATIONS
    assert rc.ALL_INSTANTIATIONS - reached == set(rc.UNREACHABLE), sorted(rc.ALL_INSTANTIATIONS - reached, key=str)
    # the seam cases run four of them over 32 769 frames
    assert {c.family for c in rc.SEAM_CASES} == {0, 1, 2, 3}


@pytest.mark.parametrize("family, n, box, steps", [
    ("filter", 300, rc.ORTHO, rc.TILE256_STEPS), ("exact", 300, None, rc.TILE256_STEPS),
    ("filter", 2048, rc.ORTHO, rc.TILE512_STEPS), ("exact", 2049, None, rc.TILE512_STEPS),
    ("cell", 300, rc.ORTHO, rc.CELL_STEPS), ("auto", 300, rc.TRI, rc.TILE256_STEPS),
    ("auto", 1024, rc.TRI, rc.CELL_STEPS)], ids=str)
def test_replica_counts_step_where_stated(family, n, box, steps, monkeypatch):
    rc.set_env(monkeypatch, {})
    tops = [top for top, _ in steps]
    for bins in sorted({1, 2, 64, 65, 512, 20000} | {b for top in tops for b in (top - 1, top, top + 1, top + 2)}):
        p = plan(np.linspace(0.0, 6.0, bins + 1), (1, 1), family, n, None, box)
        assert (p["n_hist"], p["gh"]) == rc.n_hist_of(bins, steps), (bins, p)
        assert p["lds_bytes"] <= 64 * 1024
        cell = steps is rc.CELL_STEPS
        rows = 512 if steps is rc.TILE512_STEPS else 256
        want = 16 * rows if p["gh"] else 16 * rows + 8 * (bins + 1) + 4 * p["n_hist"] * (bins + 1 if cell else bins)
        assert p["lds_bytes"] == want, (bins, p)
        assert p["lds_attribute"] == (0 if cell else int(want > 48 * 1024)), (bins, p)


def test_the_48_kib_line(monkeypatch):
    rc.set_env(monkeypatch, {})
    for algo, n, box, line in (("filter", 300, rc.ORTHO, rc.TILE256_ATTR), ("filter", 2048, rc.ORTHO, rc.TILE512_ATTR),
                               ("cell", 300, rc.ORTHO, rc.CELL_48K), ("auto", 300, rc.TRI, rc.TILE256_ATTR)):
        below = plan(np.linspace(0.0, 6.0, line), (1, 1), algo, n, None, box)
        above = plan(np.linspace(0.0, 6.0, line + 1), (1, 1), algo, n, None, box)
        assert below["lds_bytes"] <= 48 * 1024 < above["lds_bytes"], (algo, n, below, above)
        assert (below["lds_attribute"], above["lds_attribute"]) == ((0, 0) if algo == "cell" else (0, 1))


def test_padding_tiles_and_grid(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 6.0, 61)
    for n, ipt in ((1, 1), (256, 1), (257, 1), (2047, 1), (2048, 2), (2049, 2)):
        p = plan(e, (1, 1), "filter", n, None, rc.ORTHO)
        T = 256 * ipt
        assert (p["ipt"], p["n1_pad"], p["tiles1"], p["chunk"]) == (ipt, -(-n // T) * T, -(-n // T), 4)
        assert p["grid_x"] == -(-p["tiles2"] // 4) and p["n2_pad"] == p["n1_pad"]
    p = plan(e, (1, 1), "filter", 5, 2300, rc.ORTHO)
    assert (p["ipt"], p["n1_pad"], p["n2_pad"], p["tiles1"], p["tiles2"], p["chunk"], p["grid_x"]) == \
        (2, 512, 2560, 1, 5, 8, 1)
    for n in (127, 128, 129):
        p = plan(e, (1, 1), "cell", n, None, rc.ORTHO)
        assert (p["n1_pad"], p["tiles1"], p["tiles2"]) == (-(-n // 128) * 128, -(-n // 128), -(-n // 128) * 2)
    # items of the cell kernel: a quarter of the j tiles (whole 64s of them) with the skipping step, 64 tiles without
    p = plan(e, (1, 1), "cell", 70000, None, (200.0, 200.0, 200.0, 90.0, 90.0, 90.0))
    assert (p["skip"], p["tiles2"], p["chunk"], p["grid_x"]) == (1, 1094, 320, 4)
    p = plan(np.linspace(0.0, 90.0, 61), (1, 1), "cell", 70000, None, (200.0, 200.0, 200.0, 90.0, 90.0, 90.0))
    assert (p["skip"], p["chunk"], p["grid_x"]) == (0, 64, 18)
    monkeypatch.setenv("MDX_RDF_CHUNK_TILES", "128")
    assert plan(e, (1, 1), "cell", 70000, None, (200.0,) * 3 + (90.0,) * 3)["grid_x"] == 9


def test_self_and_lazy_originals(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 6.0, 61)
    for excl, same, self_, lazy in ((None, True, 1, 1), ((1, 1), True, 1, 1), ((3, 3), True, 1, 0), ((2, 5), True, 0, 0),
                                    ((1, 3), True, 0, 0), ((1, 1), False, 0, 1), (None, False, 0, 1)):
        p = plan(e, excl, "cell", 300, None if same else 300, rc.ORTHO)
        assert (p["self"], p["lazy_orig"], p["excl"]) == (self_, lazy, int(excl is not None)), (excl, same, p)
    assert plan(e, None, "auto", 1024, None, rc.TRI)["lazy_orig"] == 0


def test_algorithm_resolution(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 6.0, 61)
    fam = lambda algo, n, box: rc.FAMILIES[plan(e, None, algo, n, None, box)["family"]]
    assert [fam(a, 300, rc.ORTHO) for a in ("auto", "exact", "filter", "cell")] == \
        ["cell-ortho", "tile-exact", "tile-filter", "cell-ortho"]
    assert [fam(a, 300, None) for a in ("auto", "exact", "filter", "cell")] == \
        ["tile-filter", "tile-exact", "tile-filter", "tile-filter"]
    assert [fam(a, 1024, rc.TRI) for a in ("auto", "exact", "filter", "cell")] == \
        ["tri-culled", "tri-brute", "tri-brute", "tri-culled"]
    assert fam("auto", 1023, rc.TRI) == "tri-brute"
    # the range must end below half the smallest cell height (with 2 % and 1e-3 to spare) in EVERY frame
    wide = np.linspace(0.0, 14.0, 61)
    assert plan(wide, None, "auto", 1024, None, rc.TRI)["family"] == 3
    boxes = np.tile(np.array(rc.TRI, dtype=np.float32), (5, 1))
    assert plan(e, None, "auto", 1024, None, boxes, 5)["family"] == 4
    boxes[3, :3] = (31.0, 12.0, 35.25)
    assert plan(e, None, "auto", 1024, None, boxes, 5)["family"] == 3
    monkeypatch.setenv("MDX_RDF_TRI_BRUTE", "1")
    assert fam("auto", 1024, rc.TRI) == "tri-brute"


def test_skip_follows_the_shortest_edge_of_the_run(monkeypatch):
    rc.set_env(monkeypatch, {})
    boxes = np.tile(np.array(rc.ORTHO, dtype=np.float32), (4, 1))
    e = np.linspace(0.0, 6.0, 61)
    assert plan(e, None, "cell", 300, None, boxes, 4)["skip"] == 1
    boxes[2, 1] = 19.9                                  # 0.3 x 19.9 < 6
    assert plan(e, None, "cell", 300, None, boxes, 4)["skip"] == 0


def test_slab_arithmetic(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 4.0, 51)
    # 32 768 frames are one slab on every route, 32 769 two
    for algo, box in (("exact", rc.ORTHO), ("filter", None), ("cell", rc.ORTHO), ("auto", rc.TRI)):
        for frames, slabs in ((32768, 1), (32769, 2), (65536, 2), (65537, 3)):
            p = plan(e, (1, 1), algo, 7, None, box, frames)
            assert (p["slab_frames"], p["n_slabs"]) == (32768, slabs), (algo, frames, p)
    # the culled triclinic kernel: 1 024 particles x 32 769 frames are planned, not run
    p = plan(e, (1, 1), "auto", 1024, None, rc.TRI, 32769)
    assert (p["family"], p["slab_frames"], p["n_slabs"]) == (4, 32768, 2)
    # brute-force routes: 1 GiB of packed float4 rows, both sets unless `self`
    p = plan(e, (1, 1), "filter", 100000, None, rc.ORTHO, 5000)
    assert (p["n1_pad"], p["slab_frames"], p["n_slabs"]) == (100352, 2 ** 30 // (16 * 100352), -(-5000 // 668))
    p = plan(e, (1, 1), "filter", 100000, 100000, rc.ORTHO, 5000)
    assert p["slab_frames"] == 2 ** 30 // (16 * 2 * 100352)
    # cell routes: 2.5 GiB at 33 bytes per padded row, whole rounds of 256 frames from 256 on
    p = plan(e, (1, 1), "cell", 32000, None, rc.ORTHO, 5000)
    raw = (5 << 29) // (33 * 32000)
    assert raw == 2542 and (p["slab_frames"], p["n_slabs"]) == (2304, 3)
    p = plan(e, (1, 1), "cell", 32000, 32000, rc.ORTHO, 5000)
    assert p["slab_frames"] == 1024                      # 1 271 frames fit
    p = plan(e, (1, 1), "cell", 400000, None, rc.ORTHO, 5000)
    assert p["slab_frames"] == (5 << 29) // (33 * 400000) == 203     # below 256: not rounded
    p = plan(e, (1, 1), "cell", 32000, None, rc.ORTHO, 100)
    assert (p["slab_frames"], p["n_slabs"]) == (100, 1)
    # MDX_RDF_SLAB_BYTES, on the cell routes only
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", str(33 * 384 * 300))
    p = plan(e, (1, 1), "cell", 300, None, rc.ORTHO, 1000)
    assert (p["slab_frames"], p["n_slabs"]) == (256, 4)
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", str(33 * 384 * 255))
    assert plan(e, (1, 1), "cell", 300, None, rc.ORTHO, 1000)["slab_frames"] == 255
    monkeypatch.setenv("MDX_RDF_SLAB_BYTES", "1")
    assert plan(e, (1, 1), "cell", 300, None, rc.ORTHO, 1000)["n_slabs"] == 1000
    assert plan(e, (1, 1), "auto", 1024, None, rc.TRI, 10)["slab_frames"] == 1
    assert plan(e, (1, 1), "filter", 300, None, rc.ORTHO, 1000)["slab_frames"] == 1000


def test_argument_errors(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 6.0, 61)
    with pytest.raises(ValueError, match="exclusion"):
        plan(e, (0, 2), "auto", 300)
    with pytest.raises(ValueError, match="exclusion"):
        plan(e, (-1, -1), "auto", 300)
    with pytest.raises(ValueError, match="bad size"):
        plan(e, None, "auto", 0)
    with pytest.raises(ValueError, match="bad size"):
        plan(e, None, "auto", 300, 0)
    with pytest.raises(ValueError, match="bad size"):
        plan(e, None, "auto", 300, None, None, 0)
    with pytest.raises(ValueError, match="too many"):
        plan(e, None, "auto", 2 ** 30)
    with pytest.raises(ValueError, match="n_bins"):
        plan(np.array([1.0]), None, "auto", 300)
    with pytest.raises(ValueError, match="positive"):
        plan(e, None, "auto", 300, None, (24.0, 0.0, 24.0, 90.0, 90.0, 90.0))
    with pytest.raises(ValueError, match="invalid cell"):
        plan(e, None, "auto", 300, None, (24.0, 24.0, 24.0, 90.0, 180.0, 60.0))
    with pytest.raises(ValueError, match="span a volume"):
        plan(e, None, "auto", 300, None, (24.0, 24.0, 24.0, 20.0, 20.0, 120.0))
    mixed = np.tile(np.array(rc.ORTHO, dtype=np.float32), (3, 1))
    mixed[2] = rc.TRI
    with pytest.raises(ValueError, match="frame 2: orthorhombic and triclinic"):
        plan(e, None, "auto", 300, None, mixed, 3)
    out = np.zeros(24, dtype=np.int64)
    assert _lib.lib().mdx_rdf_plan(60, None, 0, 0, 0, 300, 300, 1, None, 1, out.ctypes.data) == -1
    assert _lib.lib().mdx_rdf_plan(60, e.ctypes.data, 0, 0, 7, 300, 300, 1, None, 1, out.ctypes.data) == -1


# every (bins, range) the suite and analysis/structure.py hand to the engine through numpy.linspace, and ranges that
# strain the rounding: far from the origin, tiny, huge, not representable
LINSPACE = [(150, (0.0, 14.0)), (90, (0.5, 11.0)), (201, (0.0, 15.0)), (4, (0, 1)), (50, (0.0, 8.0)), (150, (0.0, 10.0)),
            (64, (0.0, 9.0)), (150, (0.0, 3.0)), (150, (2.5, 3.0)), (512, (2.9, 3.0)), (3, (0.0, 3.0)), (101, (0.0, 12.0)),
            (201, (0.0, 5.0)), (60, (0.0, 3.0)), (120, (0.0, 9.0)), (33, (1.5, 8.0)), (5000, (0.0, 12.0)),
            (20000, (0.0, 12.0)), (1, (0.0, 1.0)), (7, (0.1, 0.7)), (1000, (1e-3, 1.1e-3)), (999, (0.3, 1e6)),
            (2 ** 20, (0.0, np.pi)), (4097, (1 / 3, 1e3 / 7)), (100, (0.0, 1e-300)), (100, (1e300, 1.0000001e300))]


@pytest.mark.parametrize("bins, rng", LINSPACE, ids=str)
def test_linspace_edges_pass(bins, rng, monkeypatch):
    rc.set_env(monkeypatch, {})
    assert plan(np.linspace(rng[0], rng[1], bins + 1), None, "auto", 300)["family"] == 1


def test_linspace_edges_of_the_cases_pass(monkeypatch):
    rc.set_env(monkeypatch, {})
    for bins, rng in {(c.bins, c.range) for c in rc.CASES} | {(rc.SEAM_BINS, rc.SEAM_RANGE)}:
        plan(np.linspace(rng[0], rng[1], bins + 1), None, "auto", 300)
    # a half-open arange grid is within an ulp or two of linspace as well
    plan(np.arange(61) * 0.1, None, "auto", 300)


def _create_rc(edges, algo):
    """mdx_rdf_create itself: the edges are checked before the device is, so no device is needed for a refusal."""
    e = np.ascontiguousarray(edges, dtype=np.float64)
    h = c_void_p()
    code = _lib.lib().mdx_rdf_create(byref(h), 0, e.size - 1, e.ctypes.data, 0, 0, _lib.RDF_ALGO[algo])
    assert code != 0 and not h.value
    msg = _lib.lib().mdx_last_error()
    return code, msg.decode() if msg else ""


def _perturbed():
    e = np.linspace(0.0, 12.0, 102)
    e[40] = np.nextafter(e[40], np.inf) + 5 * np.spacing(12.0)
    return e


def _reversed_pair():
    e = np.linspace(0.0, 12.0, 102)
    e[[50, 51]] = e[[51, 50]]
    return e


@pytest.mark.parametrize("algo", ["auto", "exact", "filter", "cell"])
@pytest.mark.parametrize("edges, names", [
    (np.geomspace(1.0, 5.0, 11), r"edges\[1\]"), (_perturbed(), r"edges\[40\]"), (_reversed_pair(), r"edges\[50\]"),
    (np.linspace(0.0, 12.0, 102) ** 2 / 12.0, r"edges\[1\]"), (np.array([0.0, 1.0, 1.0, 3.0]), r"edges\[1\]")],
    ids=["geomspace", "one perturbed edge", "reversed pair", "quadratic", "repeated edge"])
def test_other_edges_are_refused_by_create_before_the_device(edges, names, algo):
    import re
    code, msg = _create_rc(edges, algo)
    assert code == -1 and re.search(names, msg), (code, msg)
    with pytest.raises(ValueError, match=names):
        plan(edges, None, algo, 300)
    with pytest.raises(ValueError, match=names):
        _core.radial_histogram_device(np.zeros((4, 3)), np.zeros((4, 3)), len(edges) - 1, edges, None)


def test_four_ulp_are_allowed_and_five_are_not(monkeypatch):
    rc.set_env(monkeypatch, {})
    e = np.linspace(0.0, 12.0, 97)              # 0.125 apart: the grid itself is exact
    ulp = np.spacing(12.0)
    for k in (1, 48, 95):
        ok, bad = e.copy(), e.copy()
        ok[k] += 4 * ulp
        bad[k] -= 5 * ulp
        assert ok[k] - e[k] == 4 * ulp and e[k] - bad[k] == 5 * ulp
        plan(ok, None, "auto", 300)
        with pytest.raises(ValueError, match=rf"edges\[{k}\]"):
            plan(bad, None, "auto", 300)
