"""
The frame preparation of the MSD engine (csrc/mdx_msd.hip: ``msd_image_delta_kernel``, ``msd_image_scan_kernel``,
``msd_unwrap_widen_kernel``, ``msd_frame_com_kernel``, ``msd_molecule_com_kernel``, the three ``FrameSource``s and the
chunk / cut / frame-block bookkeeping of ``msd_push_frames`` / ``msd_system_com_frames``) against its definition, on
``_core.MsdEngine`` directly.  Inputs lie on a dyadic lattice (``msd_ingest_cases.py``), so the definition is integer
arithmetic and every comparison of prepared coordinates is ``assert_array_equal``:

(a) ``result()[1]``, the summed trajectory, is bit-equal to the integer reference;
(b) ``system_com_*`` with one-hot masses returns ONE row's prepared coordinate at every frame, bit-equal: the first and
    the last row, the rows on threads 255 / 256 (84 and 85), the rows next to the chunk cuts and every scripted row;
(c) ``result()[0]`` and ``result_acf()`` agree with ``oracle.correlation.msd_definition_ref`` of the reference-prepared
    block within the bound and the per-route constants of ``test_gpu_msd_routes.py`` (``msd_cases.ROUTE_C``): the
    transform received the prepared block, not only the sums.

``MDX_MSD_STAGE_BYTES`` (test hook) makes small inputs run through several frame blocks, particle chunks and molecule
cuts; ``test_msd_ingest_host.py`` restates its arithmetic and shows what the exact comparison is sensitive to.  In
``msd_push_frames`` the hook is the chunk's budget AND the staged bytes, so frame blocks are plural there only with
one-particle chunks (or chunks raised to the largest molecule); ``msd_system_com_frames`` has blocks without chunks.

Which test catches which removal (each was removed in a copy of the library, all reads in bounds, and run):
    ``prev`` in the ``first_block == 0`` branch   test_b_frame_blocks (all), test_b_natural_constant, test_c_* (probes),
                                                  test_f_*[unwrap], test_g_*
    ``+ 3 * a0`` on the image flags               test_b_frame_blocks (all), test_c_particle_chunks
    ``+ a0`` on the index                         test_c_particle_chunks, test_b_frame_blocks (file source), test_g_molecules_dyadic
    ``+ 3 * f0`` on the shift                     test_b_frame_blocks (all)

J, ``cross()``: against the windowed definition in ``np.longdouble`` of the engine's own summed trajectories, within
C_X 2^-52 (1 + log2 n_fft) sqrt(E_i E_j) / (T_b - m).  Observed on an MI355X: a largest ratio of 0.576, so C_X = 8
(``C_X`` below); observable (c) over the whole module: 0.684 against C = 8 of single400/none (B, blocks of 128, 86
rows of float64 from host memory), 0.092 against C = 4 of cols400_fused/rows512 (H).

Found by G (one molecule per push): ``msd_molecule_com_kernel`` fused its multiply and add (``__dmul_rn`` / ``__dadd_rn``
are plain operators in HIP's headers), one ulp off the reference's ``bincount`` order in a fifth of the centres; fixed
in the kernel.  H: a grid of 65 537 rows is accepted and gives the reference's bits; nothing was batched.
"""
import zlib

import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

import msd_cases as mc  # noqa: E402
import msd_ingest_cases as mi  # noqa: E402
import trajfiles  # noqa: E402
from mdhelper_amd import _core  # noqa: E402
from mdhelper_amd.io import TrajectoryFile  # noqa: E402
from oracle import correlation as oc  # noqa: E402

# cross(): 8 x the largest |got - ref| / unit observed over test_j_cross on an MI355X, rounded up to a power of two.
# Observed 0.576 (T_b = 500, pair (1, 1), block 0; T_b = 4 097 stays below it)  ->  8 x 0.576 = 4.6  ->  C_X = 8.
C_X = 8.0
OBSERVED = {"cross": (0.0, ""), "msd": (0.0, "")}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for what, (r, label) in OBSERVED.items():
        print(f"\nMSD-INGEST-RATIO {what} {r:.4g} from {label}", end="")
    print()


@pytest.fixture
def hold():
    """Device arrays and files of a test, released when it ends."""
    held = []
    yield held
    for h in held:
        (h.free if hasattr(h, "free") else h.close)()


def dtype_of(f64):
    return np.float64 if f64 else np.float32


class Source:
    """One way a selection reaches the engine.  ``truth``: the selection's wrapped coordinates in q."""

    def __init__(self, name, truth, push, com):
        self.name, self.truth, self.push, self.com = name, truth, push, com


def host_source(wq, f64):
    x = mi.to_float(wq, dtype_of(f64))
    return Source("host", wq, lambda eng, g, **kw: eng.push_f32(g, x, **kw),
                  lambda eng, m, **kw: eng.system_com_f32(x, m, **kw))


def device_source(wq, f64, kind, seed, hold):
    n_total, index = mi.index_kinds(wq.shape[1], seed)[kind]
    frames = mi.scatter_rows(wq, n_total, index, seed)
    truth = frames if index is None else frames[:, index]
    d = _core.DeviceArray.from_host(mi.to_float(frames, dtype_of(f64)))
    hold.append(d)
    return Source(f"device {kind}", truth, lambda eng, g, **kw: eng.push_frames_device(g, d, n_total, index, **kw),
                  lambda eng, m, **kw: eng.system_com_device(d, n_total, index, m, **kw))


def file_sources(wq, seed, tmp_path, hold, formats=("nc", "dcd"), lists=("regular", "irregular"), tag=""):
    """The selection as scattered rows of a NetCDF / DCD file (float32), at a regular and an irregular frame list."""
    n_total, index = mi.index_kinds(wq.shape[1], seed)["scattered"]
    stored = mi.to_float(mi.file_frames(wq, n_total, index, seed), np.float32)
    regular, irregular, _ = mi.frame_lists(wq.shape[0], seed)
    out = []
    for fmt in formats:
        path = tmp_path / f"walk{tag}.{fmt}"
        if fmt == "nc":
            trajfiles.write_amber_netcdf(str(path), stored, lengths=mi.BOX)
        else:
            trajfiles.write_dcd(str(path), stored, unitcell=[*mi.BOX, 90.0, 90.0, 90.0])
        tf = TrajectoryFile(path)
        hold.append(tf)
        for which in lists:
            frames = regular if which == "regular" else irregular
            out.append(Source(f"{fmt} {which}", wq,
                              lambda eng, g, tf=tf, frames=frames, **kw: eng.push_traj(g, tf, frames, index, **kw),
                              lambda eng, m, tf=tf, frames=frames, **kw: eng.system_com_traj(tf, frames, index, m, **kw)))
    return out


def results(eng):
    msd, traj = eng.result()
    return msd, traj, eng.result_acf()


def _ratio(got, want, unit):
    diff = np.abs(got - want)
    exact = unit == 0
    assert np.all(diff[exact] == 0), "nonzero where the definition gives an exact zero"
    return float((diff[~exact] / unit[~exact]).max(initial=0.0))


_REFS = {}


def reference(prepared_q, t_block, n_blocks, zero_dims=0, bits=mi.Q_BITS):
    """Observables (a) and (c) of one push of the reference-prepared block ``prepared_q[T, n, 3]`` (in 2^-bits);
    computed once per block and never modified."""
    T = t_block * n_blocks
    prepared_q = np.ascontiguousarray(prepared_q[:T])
    key = (prepared_q.shape, zlib.crc32(prepared_q.tobytes()), t_block, n_blocks, zero_dims, bits)
    if key not in _REFS:
        lags = mi.ingest_lags(t_block)
        ref = oc.msd_definition_ref(mi.to_float(prepared_q, bits=bits), t_block, n_blocks, 0, prepared_q.shape[1],
                                    zero_dims, lags)
        keep = np.array([0 if (zero_dims >> k) & 1 else 1 for k in range(3)])
        ref["traj_exact"] = mi.to_float(prepared_q.sum(axis=1) * keep, bits=bits).reshape(n_blocks, t_block, 3)
        assert_array_equal(ref["traj"], ref["traj_exact"])
        ref["lags"] = lags
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def check_group(label, res, g, ref, t_block):
    msd, traj, acf = res
    assert_array_equal(traj[g], ref["traj_exact"], err_msg=f"{label}: traj")                      # (a)
    n_fft, _, _, a, b = mc.own_length(t_block)
    unit, unit_acf = mc.unit_of(n_fft, t_block, ref["E"], ref["lags"])
    r = max(_ratio(msd[g][:, ref["lags"]], ref["msd"], unit), _ratio(acf[g][:, ref["lags"]], ref["acf"], unit_acf))
    if r > OBSERVED["msd"][0]:
        OBSERVED["msd"] = (r, label)
    assert r <= mc.ROUTE_C[f"{a}/{b}"], (label, f"{a}/{b}", r)                                     # (c)


def one_hot(n, row):
    m = np.zeros(n)
    m[row] = 1.0
    return m


def probe_rows(n, cuts=()):
    """The first and the last row, the rows whose coordinates sit on threads 255 / 256, the scripted rows, and the
    first and last row of the stated chunks."""
    rows = {0, n - 1} | {r for r in (84, 85) if r < n}
    if n >= mi.N_SCRIPTED:
        rows |= set(mi.ROLES.values())
    for a in cuts:
        rows |= {r for r in (a - 1, a) if 0 <= r < n}
    return sorted(rows)


def check_probes(label, eng, src, prepared_q, rows, **kw):
    """(b): one-hot masses give one row's prepared coordinate at every frame."""
    n = src.truth.shape[1]
    for r in rows:
        got = src.com(eng, one_hot(n, r), **kw)
        assert_array_equal(got, mi.to_float(prepared_q[:, r]), err_msg=f"{label}: row {r}")


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("c", mi.A_CASES, ids=lambda c: c.name)
def test_a_every_source_and_element_type(c, tmp_path, hold, monkeypatch):
    """Host float32 / float64, HBM-resident frames with no index, a contiguous, a scattered and a twice-listing one,
    NetCDF and DCD files at a regular and an irregular frame list (float32 cases); 1 .. 300 frames per block in 1 and 3
    blocks; 1, 85, 86 and 171 particles; with and without unwrapping: (a), (b) and (c)."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    wq, _ = mi.case_walk(c)
    t_block = c.n_frames // c.n_blocks
    srcs = [host_source(wq, c.f64)] + [device_source(wq, c.f64, k, c.seed, hold)
                                       for k in ("none", "contiguous", "scattered", "twice")]
    if not c.f64:
        srcs += file_sources(wq, c.seed, tmp_path, hold)
    eng = _core.MsdEngine(t_block, c.n_blocks, 2 * len(srcs))
    try:
        for i, s in enumerate(srcs):
            s.push(eng, 2 * i, unwrap_dims=None)
            s.push(eng, 2 * i + 1, unwrap_dims=mi.BOX)
        res = results(eng)
        for i, s in enumerate(srcs):
            for u in (0, 1):
                ref = reference(mi.unwrap_ref(s.truth, unwrap=bool(u)), t_block, c.n_blocks)
                check_group(f"{c.name} {s.name} unwrap={u}", res, 2 * i + u, ref, t_block)
        for s in srcs:
            rows = probe_rows(s.truth.shape[1])
            check_probes(f"{c.name} {s.name}", eng, s, mi.unwrap_ref(s.truth), rows, unwrap_dims=mi.BOX)
            check_probes(f"{c.name} {s.name} raw", eng, s, s.truth, rows[:2])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("block,n_rows,f64", mi.B_PARAMS)
def test_b_frame_blocks(block, n_rows, f64, tmp_path, hold, monkeypatch):
    """300 frames prepared in blocks of 1, 127, 128, 129 and 200 frames from the staged sources (host memory, a file),
    with a shift that differs per frame and initial images, crossings planted on every pair that straddles a block:
    bit-equal to the single-block result and to the reference.  Through push_* the chunks are one particle wide (both
    plural); through system_com_* all rows are staged together."""
    c = mi.b_case(block, n_rows, f64)
    wq, images0 = mi.case_walk(c)
    T, elem = c.n_frames, 8 if f64 else 4
    shift_q = mi.shift_of(c)
    shift = mi.to_float(shift_q)
    srcs = [host_source(wq, f64)]
    if not f64:
        srcs += file_sources(wq, c.seed, tmp_path, hold, lists=("irregular",))
    stage = mi.b_stage_bytes(block, elem)
    chunk, cuts, blk = mi.push_plan(T, n_rows, elem, stage)
    assert (chunk, blk) == (1, block) and len(cuts) == n_rows + 1 and mi.ceil_div(T, blk) >= 2
    prepared = mi.unwrap_ref(wq, images0, shift_q=shift_q)
    ref = reference(prepared, T, 1)
    eng = _core.MsdEngine(T, 1, 2 * len(srcs))
    try:
        eng.set_initial_images(images0)
        for i, s in enumerate(srcs):
            monkeypatch.delenv(mi.HOOK, raising=False)
            s.push(eng, 2 * i, unwrap_dims=mi.BOX, shift=shift)
            monkeypatch.setenv(mi.HOOK, str(stage))
            s.push(eng, 2 * i + 1, unwrap_dims=mi.BOX, shift=shift)
        res = results(eng)
        for i, s in enumerate(srcs):
            check_group(f"{c.name} {s.name} one block", res, 2 * i, ref, T)
            check_group(f"{c.name} {s.name} blocks of {block}", res, 2 * i + 1, ref, T)
            assert_array_equal(res[1][2 * i], res[1][2 * i + 1])         # (the chunks reorder the sums of msd)
        # system_com_*: blocks of `block` frames of all rows (no shift there)
        stage_all = mi.b_stage_bytes(block, elem, n_rows)
        assert mi.frame_block(T, n_rows, elem, stage_all) == block
        monkeypatch.setenv(mi.HOOK, str(stage_all))
        unshifted = mi.unwrap_ref(wq, images0)
        for s in srcs:
            check_probes(f"{c.name} {s.name}", eng, s, unshifted, probe_rows(n_rows), unwrap_dims=mi.BOX)
    finally:
        eng.close()


def test_b_natural_constant(monkeypatch):
    """Without the hook: 22 400 particles x 300 frames of float32 from host memory are 80 MB and go through blocks of
    249 + 51 frames; the crossings planted on 248 -> 249 count."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    w, traj_units, block = mi.natural_case()
    assert block == 249
    x = (w.astype(np.float32) / np.float32(64.0))
    assert np.array_equal(x.astype(np.float64) * 64.0, w)
    eng = _core.MsdEngine(mi.B_FRAMES, 1, 1)
    try:
        eng.push_f32(0, x, unwrap_dims=mi.BOX)
        _, traj = eng.result(want_msd=False)
        assert_array_equal(traj[0, 0], traj_units.astype(np.float64) / 64.0)
        for row in (0, mi.NATURAL_ROWS - 1):
            got = eng.system_com_f32(x, one_hot(mi.NATURAL_ROWS, row), unwrap_dims=mi.BOX)
            want = mi.unwrap_ref(w[:, row:row + 1], lq=mi.L_UNITS)[:, 0]
            # it crossed: the stored coordinate jumps by L - 8 units, the unwrapped one moves by 8
            assert abs(w[-1, row] - w[0, row]).min() > 600 and abs(want[-1] - want[0]).max() == 8
            assert_array_equal(got, want / 64.0)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
def test_c_particle_chunks(f64, tmp_path, hold, monkeypatch):
    """86 particles in chunks of 7 (twelve and one of 2) on every source — host, HBM-resident with a scattered index,
    both files —, with initial images that differ per row and a shift; bit-equal to one chunk and to the reference."""
    c = mi.c_case(f64)
    wq, images0 = mi.case_walk(c)
    T, elem = c.n_frames, 8 if f64 else 4
    shift_q = mi.shift_of(c)
    shift = mi.to_float(shift_q)
    stage = mi.C_CHUNK * 24 * T
    srcs = [host_source(wq, f64), device_source(wq, f64, "scattered", c.seed, hold),
            device_source(wq, f64, "none", c.seed, hold)]
    if not f64:
        srcs += file_sources(wq, c.seed, tmp_path, hold, lists=("irregular",))
    for s in srcs:          # (files stage float32; resident frames are not staged)
        chunk, cuts, blk = mi.push_plan(T, c.n_rows, elem if s.name == "host" else 4, stage,
                                        resident=s.name.startswith("device"))
        assert chunk == mi.C_CHUNK and len(cuts) == 14 and blk == T
    ref = reference(mi.unwrap_ref(wq, images0, shift_q=shift_q), T, 1)
    eng = _core.MsdEngine(T, 1, 2 * len(srcs))
    try:
        eng.set_initial_images(images0)
        for i, s in enumerate(srcs):
            assert_array_equal(s.truth, wq)
            monkeypatch.delenv(mi.HOOK, raising=False)
            s.push(eng, 2 * i, unwrap_dims=mi.BOX, shift=shift)
            monkeypatch.setenv(mi.HOOK, str(stage))
            s.push(eng, 2 * i + 1, unwrap_dims=mi.BOX, shift=shift)
        res = results(eng)
        for i, s in enumerate(srcs):
            check_group(f"{c.name} {s.name} one chunk", res, 2 * i, ref, T)
            check_group(f"{c.name} {s.name} chunks of 7", res, 2 * i + 1, ref, T)
        # (b) at the first and the last row of every chunk
        unshifted = mi.unwrap_ref(wq, images0)
        for s in srcs[:2]:
            check_probes(f"{c.name} {s.name}", eng, s, unshifted, probe_rows(c.n_rows, cuts), unwrap_dims=mi.BOX)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
def test_d_initial_images(f64, hold, monkeypatch):
    """Flags in -2 .. 2: frame 0 already carries them, they continue through the segments, ``None`` clears them, and
    system_com_* starts from them too."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    c = mi.c_case(f64)
    wq, images0 = mi.case_walk(c)
    assert images0.min() == -2 and images0.max() == 2
    T = c.n_frames
    srcs = [host_source(wq, f64), device_source(wq, f64, "scattered", c.seed, hold)]
    eng = _core.MsdEngine(T, 1, 3 * len(srcs))
    try:
        for i, s in enumerate(srcs):
            s.push(eng, 3 * i, unwrap_dims=mi.BOX)                      # none set yet
            eng.set_initial_images(images0)
            s.push(eng, 3 * i + 1, unwrap_dims=mi.BOX)
            with_images = mi.unwrap_ref(wq, images0)
            check_probes(f"{c.name} {s.name} images", eng, s, with_images, probe_rows(c.n_rows), unwrap_dims=mi.BOX)
            # not unwrapped: the flags do not apply
            check_probes(f"{c.name} {s.name} raw", eng, s, wq, (0, 85))
            eng.set_initial_images(None)
            s.push(eng, 3 * i + 2, unwrap_dims=mi.BOX)
            check_probes(f"{c.name} {s.name} cleared", eng, s, mi.unwrap_ref(wq), (0, 1, 85), unwrap_dims=mi.BOX)
        res = results(eng)
        plain, flagged = reference(mi.unwrap_ref(wq), T, 1), reference(with_images, T, 1)
        first = mi.to_float((wq[0] + images0 * mi.LQ).sum(axis=0))
        assert_array_equal(flagged["traj_exact"][0, 0], first)
        for i, s in enumerate(srcs):
            check_group(f"{c.name} {s.name} before", res, 3 * i, plain, T)
            check_group(f"{c.name} {s.name} images", res, 3 * i + 1, flagged, T)
            check_group(f"{c.name} {s.name} cleared", res, 3 * i + 2, plain, T)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ E
def test_e_dropped_dimensions(hold, monkeypatch):
    """zero_dims 0, 1, 2, 4 and 6 after unwrapping: the dropped column of traj is exactly zero, the others unchanged."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    c = mi.a_case(129, 1, 86, False)
    wq, _ = mi.case_walk(c)
    masks = (0, 1, 2, 4, 6)
    srcs = [host_source(wq, False), device_source(wq, False, "scattered", c.seed, hold)]
    eng = _core.MsdEngine(c.n_frames, 1, len(masks) * len(srcs))
    try:
        for i, s in enumerate(srcs):
            for j, z in enumerate(masks):
                s.push(eng, len(masks) * i + j, unwrap_dims=mi.BOX, zero_dims=z)
        res = results(eng)
        prepared = mi.unwrap_ref(wq)
        for i, s in enumerate(srcs):
            for j, z in enumerate(masks):
                g = len(masks) * i + j
                check_group(f"{c.name} {s.name} zero_dims={z}", res, g, reference(prepared, c.n_frames, 1, z), c.n_frames)
                for k in range(3):
                    if (z >> k) & 1:
                        assert not res[1][g][..., k].any()
                    else:
                        assert_array_equal(res[1][g][..., k], res[1][len(masks) * i][..., k])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ F
F_FRAMES_CHECKED = (0, 1, 126, 127, 128, 129, 254, 299)


@pytest.mark.parametrize("mode", ("wrap", "unwrap", "both"))
@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
def test_f_system_centre_of_mass(f64, mode, tmp_path, hold, monkeypatch):
    """system_com_f32 (both element types), system_com_device and system_com_traj; one-hot and dyadic masses (total
    2^10) bit-equal, arbitrary masses within (n + 2) 2^-52 sum m |x| / M of the exact rational centre — n fused steps,
    the tree's additions are among them, the reciprocal and its product —; wrap alone, unwrap alone and both, on rows
    that sit exactly at 0, L, 2 L, -L and one unit outside; once in one block and once in blocks of 127 frames."""
    c = mi.b_case(127, mi.C_ROWS, f64)
    walk, _ = mi.case_walk(c)
    T = c.n_frames
    rows_w, rows_img = mi.wrap_rows_wrapped()
    if mode == "wrap":           # the unwrapped coordinates are the input, as stored
        raw = np.concatenate([mi.unwrap_ref(walk), mi.wrap_rows(T)], axis=1)
        prepared, images0 = raw, None
    else:
        raw = np.concatenate([walk, np.broadcast_to(rows_w[None], (T, 6, 3))], axis=1)
        images0 = np.concatenate([np.zeros((c.n_rows, 3), dtype=np.int64), rows_img])
        prepared = mi.unwrap_ref(raw, images0)
        assert_array_equal(prepared[:, c.n_rows:], mi.wrap_rows(T))
    final = mi.wrap_ref(prepared) if mode != "unwrap" else prepared
    n = raw.shape[1]
    kw = {"wrap": {"wrap_dims": mi.BOX}, "unwrap": {"unwrap_dims": mi.BOX},
          "both": {"unwrap_dims": mi.BOX, "wrap_dims": mi.BOX}}[mode]
    srcs = [host_source(raw, f64), device_source(raw, f64, "scattered", c.seed, hold)]
    if not f64:
        srcs += file_sources(raw, c.seed, tmp_path, hold, formats=("nc",), lists=("irregular",))
    dyadic = mi.dyadic_masses(n, c.seed)
    arbitrary = mi.arbitrary_masses(n, c.seed)
    want_dyadic = mi.to_float(mi.centre_dyadic(final, dyadic, 10), bits=mi.Q_BITS + 10)
    checked = list(F_FRAMES_CHECKED)
    want_arbitrary = mi.fractions_to_float(mi.centre_ref(final[checked], arbitrary))
    slack = (n + 2) * mi.EPS * (np.abs(mi.to_float(final[checked])) * arbitrary[None, :, None]).sum(axis=1) \
        / arbitrary.sum()
    eng = _core.MsdEngine(T, 1, 1)
    try:
        if images0 is not None:
            eng.set_initial_images(images0)
        for stage in (None, mi.b_stage_bytes(127, 8 if f64 else 4, n)):
            if stage is None:
                monkeypatch.delenv(mi.HOOK, raising=False)
            else:
                monkeypatch.setenv(mi.HOOK, str(stage))
            for s in srcs:
                label = f"F {mode} {s.name} stage={stage}"
                assert_array_equal(s.truth, raw)
                rows = [0, c.n_rows - 1] + list(range(c.n_rows, n))
                check_probes(label, eng, s, final, rows, **kw)
                assert_array_equal(s.com(eng, dyadic.astype(np.float64), **kw), want_dyadic, err_msg=label)
                got = s.com(eng, arbitrary, **kw)[checked]
                assert np.all(np.abs(got - want_arbitrary) <= slack), (label, np.abs(got - want_arbitrary).max())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ G
def _g_setup():
    c = mi.G_CASE
    wq, _ = mi.case_walk(c)
    return c, wq, mi.molecule_offsets(mi.G_SIZES), mi.shift_of(c)


def test_g_molecules_dyadic(tmp_path, hold, monkeypatch):
    """Molecules of 1, 2, 3, 5, 1, 4, ... rows that each weigh 2^3: traj is the exact sum of the centres minus the shift
    (subtracted from the centres), in one chunk and in chunks raised to the largest molecule — (1, 4) ends exactly on
    a cut, the last chunk holds one molecule — with blocks of 127 frames; the system centre of the wrapped molecule
    centres is exact too."""
    c, wq, offsets, shift_q = _g_setup()
    T, n_mol = c.n_frames, len(offsets) - 1
    masses = mi.g_masses_dyadic()
    prepared = mi.unwrap_ref(wq)
    centres = mi.molecule_centres_dyadic(prepared, offsets, masses, 3)                 # in 2^-33
    shifted = centres - 8 * shift_q[:, None, :]
    ref = reference(shifted, T, 1, bits=mi.Q_BITS + 3)
    wrapped = mi.wrap_ref(centres, 8 * mi.LQ)
    assert (wrapped != centres).any()
    want_com = mi.to_float(wrapped.sum(axis=1), bits=mi.Q_BITS + 3 + 5)               # 32 molecules of equal mass
    stage = mi.b_stage_bytes(127, 4, 5)
    chunk, cuts, blk = mi.push_plan(T, c.n_rows, 4, stage, offsets)
    assert (chunk, blk) == (5, 127) and cuts[-4:] == [75, 80, 81, 86]
    srcs = [host_source(wq, False), device_source(wq, False, "scattered", c.seed, hold)]
    srcs += file_sources(wq, c.seed, tmp_path, hold, formats=("dcd",), lists=("irregular",))
    eng = _core.MsdEngine(T, 1, 2 * len(srcs))
    try:
        eng.set_grouping(offsets, masses.astype(np.float64))
        for i, s in enumerate(srcs):
            for j, value in enumerate((None, stage)):
                if value is None:
                    monkeypatch.delenv(mi.HOOK, raising=False)
                else:
                    monkeypatch.setenv(mi.HOOK, str(value))
                s.push(eng, 2 * i + j, unwrap_dims=mi.BOX, shift=mi.to_float(shift_q))
                got = s.com(eng, np.ones(c.n_rows), unwrap_dims=mi.BOX, wrap_dims=mi.BOX)
                assert_array_equal(got, want_com, err_msg=f"G {s.name} stage={value}")
        res = results(eng)
        for g in range(2 * len(srcs)):
            check_group(f"G dyadic {srcs[g // 2].name} {'chunks' if g % 2 else 'one chunk'}", res, g, ref, T)
    finally:
        eng.close()


def test_g_molecules_arbitrary_masses(hold, monkeypatch):
    """Any masses: ONE molecule per push is bit-equal to the sequential float64 restatement (separate multiply and
    add in row order, one division, then the shift); many molecules: the restated centres summed, within
    (n - 1) 2^-52 sum |c| (any order of n - 1 additions)."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    c, wq, offsets, shift_q = _g_setup()
    T = c.n_frames
    x = mi.to_float(mi.unwrap_ref(wq))
    x32 = mi.to_float(wq, np.float32)
    masses = mi.arbitrary_masses(c.n_rows, c.seed)
    shift = mi.to_float(shift_q)
    sizes = (1, 2, 3, 5, 86)
    eng = _core.MsdEngine(T, 1, len(sizes) + 2)
    try:
        for g, k in enumerate(sizes):
            eng.set_grouping([0, k], masses[:k])
            eng.push_f32(g, np.ascontiguousarray(x32[:, :k]), unwrap_dims=mi.BOX, shift=shift if k == 3 else None)
        restated = mi.molecule_centres_restated(x, offsets, masses)
        for g, stage in ((len(sizes), None), (len(sizes) + 1, mi.b_stage_bytes(127, 4, 5))):
            if stage is not None:
                monkeypatch.setenv(mi.HOOK, str(stage))
            eng.set_grouping(offsets, masses)
            eng.push_f32(g, x32, unwrap_dims=mi.BOX, shift=shift)
        _, traj = eng.result(want_msd=False)
        for g, k in enumerate(sizes):
            want = mi.molecule_centres_restated(x[:, :k], np.array([0, k]), masses[:k])[:, 0]
            assert_array_equal(traj[g, 0], want - shift if k == 3 else want, err_msg=f"one molecule of {k}")
        many = restated - shift[:, None, :]
        slack = (many.shape[1] - 1) * mi.EPS * np.abs(many).sum(axis=1)
        for g in (len(sizes), len(sizes) + 1):
            assert np.all(np.abs(traj[g, 0] - many.sum(axis=1)) <= slack)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ H
def test_h_more_frames_than_a_grids_y_extent(monkeypatch):
    """2 molecules of 2 particles over 65 537 frames in one block: ``msd_molecule_com_kernel`` runs one grid row per
    frame, in both callers."""
    monkeypatch.delenv(mi.HOOK, raising=False)
    T = mi.H_FRAMES
    wq = mi.lattice_walk(T, 4, 13)
    offsets, masses = np.array([0, 2, 4]), np.array([1, 3, 2, 2])
    prepared = mi.unwrap_ref(wq)
    assert np.abs(prepared).max() > 3 * mi.LQ.max()
    centres = mi.molecule_centres_dyadic(prepared, offsets, masses, 2)                 # in 2^-32
    x = mi.to_float(wq, np.float32)
    eng = _core.MsdEngine(T, 1, 1)
    try:
        eng.set_grouping(offsets, masses.astype(np.float64))
        eng.push_f32(0, x, unwrap_dims=mi.BOX)
        check_group("H push_f32", results(eng), 0, reference(centres, T, 1, bits=mi.Q_BITS + 2), T)
        got = eng.system_com_f32(x, np.ones(4), unwrap_dims=mi.BOX)
        assert_array_equal(got, mi.to_float(centres.sum(axis=1), bits=mi.Q_BITS + 3))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ I
def test_i_refusals_leave_the_result_unchanged(tmp_path, hold, monkeypatch):
    monkeypatch.delenv(mi.HOOK, raising=False)
    c = mi.a_case(130, 1, 7, False)
    wq, _ = mi.case_walk(c)
    T, n = c.n_frames, c.n_rows
    x = mi.to_float(wq, np.float32)
    host = host_source(wq, False)
    dev = _core.DeviceArray.from_host(x)
    hold.append(dev)
    files = file_sources(wq, c.seed, tmp_path, hold, formats=("nc",), lists=("regular",))
    tf, regular = hold[-1], mi.frame_lists(T, c.seed)[0]
    n_file = tf.n_atoms
    eng = _core.MsdEngine(T, 1, 2)
    try:
        host.push(eng, 0, unwrap_dims=mi.BOX)
        before = results(eng)
        ones = np.ones(n)
        eng.set_initial_images(np.zeros((5, 3), dtype=np.int32))
        with pytest.raises(ValueError, match="initial image flags were set for 5 particles, 7 are staged"):
            host.push(eng, 0, unwrap_dims=mi.BOX)
        with pytest.raises(ValueError, match="initial image flags were set for 5 particles, 7 are staged"):
            host.com(eng, ones, unwrap_dims=mi.BOX)
        eng.set_initial_images(None)
        eng.set_grouping([0, 3, 6], np.ones(6))
        with pytest.raises(ValueError, match="7 particles given, the grouping was defined for 6"):
            host.push(eng, 0, unwrap_dims=mi.BOX)
        with pytest.raises(ValueError, match="7 particles given, the grouping was defined for 6"):
            host.com(eng, ones)
        eng.set_grouping(None, None)
        bad_box = np.array([12.5, 0.0, 9.75])
        for push in (host.push, files[0].push, lambda e, g, **kw: e.push_frames_device(g, dev, n, None, **kw)):
            with pytest.raises(ValueError, match="unwrapping needs positive box dimensions"):
                push(eng, 0, unwrap_dims=bad_box)
        for com in (host.com, files[0].com, lambda e, m, **kw: e.system_com_device(dev, n, None, m, **kw)):
            with pytest.raises(ValueError, match="unwrapping / wrapping needs positive box dimensions"):
                com(eng, ones, wrap_dims=bad_box)
            with pytest.raises(ValueError, match="unwrapping / wrapping needs positive box dimensions"):
                com(eng, ones, unwrap_dims=-mi.BOX)
            with pytest.raises(ValueError, match="the selection has no mass"):
                com(eng, np.zeros(n))
        with pytest.raises(ValueError, match=r"particle index 7 out of range \[0, 7\)"):
            eng.push_frames_device(0, dev, n, [0, 7])
        with pytest.raises(ValueError, match=r"particle index -1 out of range \[0, 7\)"):
            eng.system_com_device(dev, n, [-1, 2], np.ones(2))
        with pytest.raises(ValueError, match=rf"particle index {n_file} out of range \[0, {n_file}\)"):
            eng.push_traj(0, tf, regular, [1, n_file])
        with pytest.raises(ValueError, match=rf"particle index {n_file} out of range \[0, {n_file}\)"):
            eng.system_com_traj(tf, regular, [1, n_file], np.ones(2))
        with pytest.raises(ValueError, match="129 frames given, the engine needs 130"):
            eng.push_f32(0, x[:-1], unwrap_dims=mi.BOX)
        with pytest.raises(ValueError, match="129 frames given, the engine needs 130"):
            eng.push_frames_device(0, _core.DeviceArray.view(dev, (T - 1, n, 3)), n)
        with pytest.raises(ValueError, match="129 frames listed, the engine needs 130"):
            eng.push_traj(0, tf, regular[:-1])
        after = results(eng)
        for b, a in zip(before, after):
            assert_array_equal(a, b)
        # the engine goes on
        files[0].push(eng, 1, unwrap_dims=mi.BOX)
        ref = reference(mi.unwrap_ref(wq), T, 1)
        res = results(eng)
        check_group("I host", res, 0, ref, T)
        check_group("I file", res, 1, ref, T)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ J
def _cross_definition(a, b, lags):
    """mean_t (a(t + m) - a(t)) . (b(t + m) - b(t)) of two series [T_b, 3] in np.longdouble."""
    a, b = a.astype(np.longdouble), b.astype(np.longdouble)
    out = np.empty(len(lags), dtype=np.longdouble)
    for i, m in enumerate(lags):
        m = int(m)
        da, db = a[m:] - a[:len(a) - m], b[m:] - b[:len(b) - m]
        out[i] = (da * db).sum() / (len(a) - m)
    return out


@pytest.mark.parametrize("t_block", (1, 2, 500, 4097))
def test_j_cross(t_block, monkeypatch):
    """cross() of the summed trajectories of three groups (5, 1 and 7 particles) in 3 blocks against the windowed
    definition; 4 097 frames are two tiles of ``msd_finish_kernel`` (the carry).  (i, j) and (j, i) are bit-equal (both
    kernels are symmetric in the pair), and (i, i) of the one-particle group is ``result()`` of that group."""
    for name in mc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    n_blocks, sizes = 3, (5, 1, 7)
    rng = np.random.default_rng([t_block, 59])
    steps = rng.normal(0.0, mc.STEP, (n_blocks, t_block, sum(sizes), 3))
    steps[:, 0] = rng.normal(0.0, 1.0, (n_blocks, sum(sizes), 3))
    pos = np.cumsum(steps, axis=1).reshape(n_blocks * t_block, sum(sizes), 3)
    lags = mc.lags_of(t_block)
    eng = _core.MsdEngine(t_block, n_blocks, len(sizes))
    try:
        first = 0
        for g, k in enumerate(sizes):
            eng.push(g, pos, first, k)
            first += k
        msd, traj = eng.result()
        pairs = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (1, 1), (2, 2)]
        got = eng.cross(pairs)
        n_fft = eng.n_fft
    finally:
        eng.close()
    energy = (traj.astype(np.longdouble) ** 2).sum(axis=(2, 3)).astype(np.float64)            # [group, block]
    worst = 0.0
    for p, (i, j) in enumerate(pairs):
        assert_array_equal(got[p], got[pairs.index((j, i))])
        for b in range(n_blocks):
            want = _cross_definition(traj[i, b], traj[j, b], lags).astype(np.float64)
            unit = mi.EPS * (1.0 + np.log2(n_fft)) * np.sqrt(energy[i, b] * energy[j, b]) / (t_block - lags)
            r = _ratio(got[p, b, lags], want, unit)
            print(f"J T_b={t_block} pair {i, j} block {b}: {r:.4g}")
            if r > OBSERVED["cross"][0]:
                OBSERVED["cross"] = (r, f"T_b = {t_block}, pair {i, j}, block {b}")
            worst = max(worst, r)
    assert worst <= C_X, worst
    # the one-particle group: its summed trajectory is the particle's
    _, _, _, a, bb = mc.own_length(t_block)
    for b in range(n_blocks):
        unit = mi.EPS * (1.0 + np.log2(n_fft)) * energy[1, b] / (t_block - np.arange(t_block))
        assert np.all(np.abs(got[pairs.index((1, 1)), b] - msd[1, b]) <= (C_X + mc.ROUTE_C[f"{a}/{bb}"]) * unit)
