"""
What ``test_gpu_msd_ingest.py`` rests on, checked without a GPU: the integer reference of ``msd_ingest_cases.py`` is the
package's own float64 ``unwrap`` / ``wrap`` / ``center_of_mass`` bit for bit on every case's inputs; every case holds
the events it claims; the hook values cut the chunks, molecule cuts and frame blocks the cases name; and the exact
comparison sees each of the slips it is there for (a lost crossing, an image off by one for a segment, a chunk that
reads row a instead of row a + a0) as at least one box length, 624 lattice units, in the summed trajectory.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import msd_ingest_cases as mi
from mdhelper_amd.algorithm import molecule, topology

BOX_LENGTH = 624 * mi.UNIT          # the shortest box length in q


def floats(c, xq):
    """What the engine is fed, widened: float32 cases hold float32 values."""
    return mi.to_float(xq, np.float64 if c.f64 else np.float32).astype(np.float64)


def package_unwrap(x, images0):
    """``algorithm.topology.unwrap`` frame by frame with thresholds L / 2, as the analysis classes call it."""
    out = np.empty_like(x)
    old = x[0].copy()
    images = np.zeros(x.shape[1:], dtype=int) if images0 is None else np.array(images0, dtype=int)
    for t in range(x.shape[0]):
        frame = x[t].copy()
        topology.unwrap(frame, old, mi.BOX, thresholds=mi.BOX / 2, images=images)
        out[t] = frame
    return out


@pytest.mark.parametrize("c", mi.ALL_CASES, ids=lambda c: c.name)
def test_reference_is_the_packages_float64_and_the_events_are_there(c):
    wq, images0 = mi.case_walk(c)
    mi.assert_claims(wq, mi.claims_of(c.n_frames, c.n_rows, c.cross_at), images0)
    x = floats(c, wq)
    ref_q = mi.unwrap_ref(wq, images0)
    assert_array_equal(ref_q, mi.unwrap_ref_serial(wq, images0))
    unwrapped = package_unwrap(x, images0)
    assert_array_equal(unwrapped, mi.to_float(ref_q))
    assert_array_equal(topology.wrap(unwrapped, mi.BOX, in_place=False), mi.to_float(mi.wrap_ref(ref_q)))
    # the system centre with dyadic masses that sum to 2^10: a few frames, any summation order
    m = mi.dyadic_masses(c.n_rows, c.seed)
    frames = sorted({0, c.n_frames // 2, c.n_frames - 1})
    want = mi.to_float(mi.centre_dyadic(ref_q[frames], m, 10), bits=mi.Q_BITS + 10)
    for i, t in enumerate(frames):
        got = molecule.center_of_mass(masses=m.astype(float), positions=unwrapped[t])
        assert_array_equal(got, want[i])


def test_wrap_rows():
    """0 and L stay, 2 L and -L go to 0, one unit below 0 goes to L - 1 unit, one unit above L to one unit."""
    rows = mi.wrap_rows(2)
    want = np.stack([0 * mi.LQ, mi.LQ, 0 * mi.LQ, 0 * mi.LQ, mi.LQ - mi.UNIT, 0 * mi.LQ + mi.UNIT])
    assert_array_equal(mi.wrap_ref(rows)[0], want)
    assert_array_equal(topology.wrap(mi.to_float(rows[0]), mi.BOX, in_place=False), mi.to_float(want))
    w, img = mi.wrap_rows_wrapped()
    assert_array_equal(mi.unwrap_ref(w[None], img)[0], rows[0])
    assert (w >= 0).all() and (w < mi.LQ).all() and np.abs(img).max() <= 2


class _Residues:
    """The two attributes ``center_of_mass(group, "residues")`` reads."""

    def __init__(self, offsets, masses, positions):
        self.resindices = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        self.masses, self.positions = masses, positions


def test_molecule_centres_are_the_packages_bincount():
    c = mi.G_CASE
    wq, _ = mi.case_walk(c)
    offsets = mi.molecule_offsets(mi.G_SIZES)
    assert offsets[-1] == c.n_rows == 86 and len(offsets) - 1 == 32 and np.diff(offsets).max() == 5
    ref_q = mi.unwrap_ref(wq)
    x = mi.to_float(ref_q)
    dyadic = mi.g_masses_dyadic()
    arbitrary = mi.arbitrary_masses(c.n_rows, c.seed)
    exact = mi.to_float(mi.molecule_centres_dyadic(ref_q, offsets, dyadic, 3), bits=mi.Q_BITS + 3)
    restated_dyadic = mi.molecule_centres_restated(x, offsets, dyadic)
    restated = mi.molecule_centres_restated(x, offsets, arbitrary)
    assert_array_equal(restated_dyadic, exact)
    for t in (0, 127, 128, 299):
        assert_array_equal(molecule.center_of_mass(_Residues(offsets, dyadic.astype(float), x[t]), "residues"), exact[t])
        assert_array_equal(molecule.center_of_mass(_Residues(offsets, arbitrary, x[t]), "residues"), restated[t])
    # the exact rational centre of the arbitrary masses lies within n roundings of the restatement
    fr = mi.fractions_to_float(mi.centre_ref(ref_q[:2, :5], arbitrary[:5]))
    one = mi.molecule_centres_restated(x[:2, :5], np.array([0, 5]), arbitrary[:5])[:, 0]
    assert np.all(np.abs(fr - one) <= 7 * mi.EPS * np.abs(x[:2, :5]).max())


def test_natural_case_crosses_on_its_block_boundary():
    w, traj, block = mi.natural_case()
    assert block == 249 and mi.B_FRAMES - block == 51
    assert w.shape == (300, mi.NATURAL_ROWS, 3) and w.dtype == np.int32 and w.nbytes == 80_640_000
    # without the crossing on 248 -> 249 the two planted rows are one box length off from frame 249 on: they cross in
    # opposite directions, so look at one of them
    step = mi.image_steps(w[:, :1], mi.L_UNITS)
    assert step[block].all() and np.count_nonzero(step) == 3


# ------------------------------------------------------------------------------------------------ hook arithmetic
def test_hook_arithmetic():
    T = mi.B_FRAMES
    # 64 MiB hold 48 000 frames of 115 particles: without the hook every small series is one block
    assert mi.frame_block(T, 115, 4) == T and (64 << 20) // (12 * 115) >= 48000
    for elem in (4, 8):
        for block in mi.B_BLOCKS:
            # push_*: the hook is also the chunk's budget, and frame blocks are plural only with one-particle chunks
            for n in (mi.B_ROWS, mi.C_ROWS):
                chunk, cuts, blk = mi.push_plan(T, n, elem, mi.b_stage_bytes(block, elem))
                assert (chunk, blk) == (1, block) and cuts == list(range(n + 1))
                assert mi.ceil_div(T, blk) >= 2
            # system_com_*: no chunks
            assert mi.frame_block(T, mi.C_ROWS, elem, mi.b_stage_bytes(block, elem, mi.C_ROWS)) == block
        # a chunk never has several frame blocks unless it is one particle (or was raised to a molecule)
        for stage in (1, 100, 7199, 7200, 50400, 10 ** 6):
            chunk, _, blk = mi.push_plan(T, mi.C_ROWS, elem, stage)
            assert chunk == 1 or blk == T
    # family C: 86 particles in chunks of 7 (twelve of them and one of 2), one frame block
    chunk, cuts, blk = mi.push_plan(T, mi.C_ROWS, 4, mi.C_CHUNK * 24 * T)
    assert (chunk, blk) == (7, T) and cuts == list(range(0, 86, 7)) + [86] and len(cuts) == 14
    # molecules: a budget below the largest molecule is raised to it, and with it come several frame blocks
    offsets = mi.molecule_offsets(mi.G_SIZES)
    chunk, cuts, blk = mi.push_plan(T, 86, 4, mi.b_stage_bytes(127, 4, 5), offsets)
    assert (chunk, blk) == (5, 127)
    assert cuts[-4:] == [75, 80, 81, 86]        # (1, 4) ends exactly on a cut; one molecule; the last chunk: one of 5
    assert all(a in set(offsets.tolist()) for a in cuts) and max(np.diff(cuts)) == 5 and len(cuts) > 3
    # H: more frames than a grid's y extent in one block
    assert mi.frame_block(mi.H_FRAMES, 4, 4) == mi.H_FRAMES > 65535
    # resident frames are not staged: the hook leaves their blocks alone
    assert mi.frame_block(T, 86, 4, 12, resident=True) == T


# ------------------------------------------------------------------------------------------------ sensitivity
def _traj(prepared_q):
    return prepared_q.sum(axis=1)


def _moved(a, b):
    return int(np.abs(_traj(a) - _traj(b)).max())


def test_a_lost_crossing_moves_traj_by_a_box_length():
    c = mi.b_case(127, mi.C_ROWS, False)
    wq, images0 = mi.case_walk(c)
    ref = mi.unwrap_ref(wq, images0)
    for lost in (127, 128, 254, 299):
        assert lost in c.cross_at
        # what a block that starts at `lost` without the previous block's last frame would do
        step = mi.image_steps(wq)
        step[lost] = 0
        wrong = wq + (np.cumsum(step, axis=0) + images0[None]) * mi.LQ
        assert _moved(ref, wrong) >= BOX_LENGTH
        # one row alone (the one-hot probe): the crosser
        assert np.abs(ref[:, 0] - wrong[:, 0]).max() >= BOX_LENGTH


def test_an_image_off_by_one_for_a_segment_moves_traj_by_a_box_length():
    c = mi.c_case(True)
    wq, images0 = mi.case_walk(c)
    ref = mi.unwrap_ref(wq, images0)
    for row in (0, 5, 85):
        wrong = ref.copy()
        wrong[mi.SEG:2 * mi.SEG, row, 2] += mi.LQ[2]
        assert _moved(ref, wrong) >= BOX_LENGTH


def test_reading_row_a_instead_of_a_plus_a0_moves_traj_by_a_box_length():
    c = mi.c_case(False)
    wq, images0 = mi.case_walk(c)
    ref = mi.unwrap_ref(wq, images0)
    _, cuts, _ = mi.push_plan(c.n_frames, c.n_rows, 4, mi.C_CHUNK * 24 * c.n_frames)
    # image flags of rows [0, c) given to every chunk
    wrong_images = np.concatenate([images0[:hi - lo] for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _moved(ref, mi.unwrap_ref(wq, wrong_images)) >= BOX_LENGTH
    # index rows [0, c) read by every chunk
    n_total, index = mi.index_kinds(c.n_rows, c.seed)["scattered"]
    frames = mi.scatter_rows(wq, n_total, index, c.seed)
    assert_array_equal(frames[:, index], wq)
    wrong_index = np.concatenate([index[:hi - lo] for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _moved(ref, mi.unwrap_ref(frames[:, wrong_index], images0)) >= BOX_LENGTH
    # the shift of frames [0, nf) subtracted in every frame block
    shift = mi.shift_of(c)
    blocks = np.concatenate([np.arange(min(127, c.n_frames - f0)) for f0 in range(0, c.n_frames, 127)])
    assert _moved(mi.unwrap_ref(wq, images0, shift_q=shift), mi.unwrap_ref(wq, images0, shift_q=shift[blocks])) \
        >= BOX_LENGTH


def test_sources_hold_the_walk():
    """Every placement of a selection in wider frames and in a file gives the walk back."""
    c = mi.a_case(129, 1, 86, False)
    wq, _ = mi.case_walk(c)
    for name, (n_total, index) in mi.index_kinds(c.n_rows, c.seed).items():
        frames = mi.scatter_rows(wq, n_total, index, c.seed)
        truth = frames if index is None else frames[:, index]
        assert truth.shape[1] == c.n_rows and frames.shape[1] == n_total
        if name == "twice":
            assert index[5] == index[6] and not np.array_equal(truth, wq)
            truth[:, 5] = wq[:, 5]
        assert_array_equal(truth, wq)
        regular, irregular, n_file = mi.frame_lists(c.n_frames, c.seed)
        assert np.all(np.diff(irregular) > 0) and len(set(np.diff(irregular))) > 1 and irregular[-1] < n_file
        assert len(set(np.diff(regular))) == 1 and not set(regular) & set(irregular)
        stored = mi.file_frames(wq, n_total, index, c.seed)
        assert_array_equal(stored[regular], frames)
        assert_array_equal(stored[irregular], frames)
