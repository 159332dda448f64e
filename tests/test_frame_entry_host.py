"""
The C entry points the sixteen per-frame engines share (``csrc/mdx_frame_entry.hpp``) at their NULL checks, and on a
lazy handle that has not touched its device.  The return codes and texts are those of the hand-written entry points
these replaced, engine by engine: where those said "NULL argument" and where "NULL handle" is part of the ABI's
behaviour and is pinned here as it was, not unified.  Nothing here touches a device.
"""
import ctypes

import numpy as np
import pytest

from mdhelper_amd import _core, _lib

MDX_ERR_INVALID_VALUE = -1

ENGINES = ("prof", "gyr", "rouse", "msid", "dip", "vh", "vhd", "prs", "clu", "ang", "ori", "boo", "chi4", "hb", "dih",
           "sdf")
SLABBED = ("dip", "vh", "vhd", "prs", "clu", "ang", "ori", "boo", "chi4", "hb", "dih", "sdf")
RINGED = ("vh", "vhd", "prs", "ori", "chi4", "hb", "dih")

# what mdx_last_error() says after mdx_X_<name>(NULL, ...), for every engine ...
NULL_HANDLE_TEXT = {
    "accumulate": "NULL argument",
    "accumulate_device": "NULL argument",
    "accumulate_traj": "NULL handle",
    "enable_timing": "NULL handle",
    "synchronize": "NULL handle",
    "reset": "NULL handle",
    "set_slab_frames": "NULL handle",
}
# ... and after mdx_X_plan(NULL, ...): an engine with a ring checks its handle first, the others all three pointers
PLAN_NULL_HANDLE_TEXT = {
    "dip": "NULL argument", "vh": "NULL handle", "vhd": "NULL handle", "prs": "NULL handle", "clu": "NULL argument",
    "ang": "NULL argument", "ori": "NULL handle", "boo": "NULL argument", "chi4": "NULL handle", "hb": "NULL handle",
    "dih": "NULL handle", "sdf": "NULL argument",
}

CASES = [(x, name, text) for x in ENGINES for name, text in NULL_HANDLE_TEXT.items()
         if name != "set_slab_frames" or x in SLABBED] + [(x, "plan", PLAN_NULL_HANDLE_TEXT[x]) for x in SLABBED]


def last_error():
    return _lib.lib().mdx_last_error().decode()


def call_with_null_handle(fn, others):
    """fn(NULL, ...): the other pointers NULL too, or (``others``) valid, and every size 0."""
    sizes = (ctypes.c_int, ctypes.c_int64)
    words = np.zeros(8, dtype=np.int64)
    args = [0 if t in sizes else ctypes.cast(words.ctypes.data, t) if others else None for t in fn.argtypes]
    args[0] = None
    return fn(*args)


def test_the_tables_name_every_engine_once():
    assert len(set(ENGINES)) == 16 and set(SLABBED) <= set(ENGINES) and set(RINGED) <= set(SLABBED)
    assert set(PLAN_NULL_HANDLE_TEXT) == set(SLABBED)
    assert {x for x, text in PLAN_NULL_HANDLE_TEXT.items() if text == "NULL handle"} == set(RINGED)
    assert len(CASES) == 16 * 6 + 12 * 2
    for x in ENGINES:
        for name in ("set_slab_frames", "plan"):
            assert (f"mdx_{x}_{name}" in _lib.EXPORTS) == (x in SLABBED)


@pytest.mark.parametrize("others", [False, True], ids=["others_null", "others_valid"])
@pytest.mark.parametrize("engine,name,text", CASES, ids=[f"{x}_{name}" for x, name, _ in CASES])
def test_null_handle_is_an_invalid_value_in_the_words_of_the_engine(engine, name, text, others):
    fn = getattr(_lib.lib(), f"mdx_{engine}_{name}")
    assert call_with_null_handle(fn, others) == MDX_ERR_INVALID_VALUE
    assert last_error() == text


@pytest.mark.parametrize("engine", ENGINES)
def test_destroy_of_null_is_ok(engine):
    assert getattr(_lib.lib(), f"mdx_{engine}_destroy")(None) == _lib.MDX_OK


def make_vh():
    return _core.VanHoveEngine([3, 2], np.linspace(0.0, 2.0, 5), [0, 1, 3])


def make_sdf():
    # two three-atom molecules, each the other's partner group of one atom
    return _core.SpatialDistributionEngine(6, [0, 3], [1, 4], [2, 5], [0, 2], [0, 3], [0, 1], 0, 1.0, [4.0, 4.0, 4.0])


@pytest.mark.parametrize("make,ring", [(make_vh, 3), (make_sdf, None)], ids=["vh", "sdf"])
def test_a_lazy_handle_lives_and_dies_without_a_device(make, ring):
    """set_slab_frames, plan, enable_timing, reset, synchronize and destroy of a handle that never saw a frame:
    none has a device side to wait for, zero or release."""
    eng = make()
    fn = eng._fn
    h = eng.handle
    slab, frames = ctypes.c_int64(), ctypes.c_int64()
    assert fn("set_slab_frames")(h, 5) == _lib.MDX_OK
    assert fn("plan")(h, ctypes.byref(slab), ctypes.byref(frames)) == _lib.MDX_OK
    assert (slab.value, frames.value) == (5, 0 if ring is None else ring + 5)
    assert fn("enable_timing")(h, 1) == _lib.MDX_OK
    assert fn("reset")(h) == _lib.MDX_OK
    assert fn("synchronize")(h) == _lib.MDX_OK
    assert eng.stats()["frames"] == 0
    # argument errors of a live handle keep their words too
    assert fn("set_slab_frames")(h, -1) == MDX_ERR_INVALID_VALUE and last_error().startswith("frames must lie in [0, ")
    assert fn("plan")(h, None, None) == MDX_ERR_INVALID_VALUE and last_error() == "NULL argument"
    assert fn("accumulate")(h, None, 5, 1) == MDX_ERR_INVALID_VALUE and last_error() == "NULL argument"
    assert fn("accumulate_device")(h, None, 5, 1, None, 0) == MDX_ERR_INVALID_VALUE
    assert last_error() == "NULL argument"
    assert fn("accumulate_traj")(h, None, None, 0, None, 0) == MDX_ERR_INVALID_VALUE and last_error() == "NULL handle"
    assert fn("destroy")(h) == _lib.MDX_OK
    eng.handle = ctypes.c_void_p()      # close() has nothing left to destroy
