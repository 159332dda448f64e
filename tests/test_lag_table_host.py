"""
The lag lists the six lag engines refuse in ``create``, which needs no GPU (a handle touches its device with the first
frame): van Hove, four-point susceptibility, orientational relaxation, distinct van Hove, pair residence and hydrogen
bonds.  Every engine gets the same bad lists, and every refusal is compared word for word with the message the engine
gave before the engines shared their lag table (``LagTable`` in ``csrc/mdx_lag_history.hpp``); the caps and the words
about them differ per engine and are listed here as they stood.
"""
import ctypes

import numpy as np
import pytest

from mdhelper_amd import _lib

EDGES = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
DIMS = np.array([10.0, 11.0, 12.0])
ONE = np.array([2], dtype=np.int64)             # a group of two points
ONE_VECTOR = np.array([1], dtype=np.int64)      # a group of one vector
CUTOFFS = np.array([0.5, 1.0])
PAIR = np.array([0, 1], dtype=np.int32)
H_ROW, D_ROW, A_ROW = (np.array([k], dtype=np.int32) for k in range(3))

NONE = "lags must hold at least one lag"


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _creates(lib, h):
    """create(n_lags, lags, origin_step) of every lag engine, its other arguments good ones"""
    out = ctypes.byref(h)
    return {
        "vh": lambda n, lags, step: lib.mdx_vh_create(out, 0, 1, p(ONE), 4, p(EDGES), n, p(lags), 0),
        "chi4": lambda n, lags, step: lib.mdx_chi4_create(out, 0, 1, p(ONE), 2, p(CUTOFFS), n, p(lags), step, 0),
        "ori": lambda n, lags, step: lib.mdx_ori_create(out, 0, 1, p(ONE_VECTOR), 2, p(PAIR), n, p(lags), 0),
        "vhd": lambda n, lags, step: lib.mdx_vhd_create(out, 0, 2, 3, 0, 4, p(EDGES), n, p(lags), step, p(DIMS), 0),
        "prs": lambda n, lags, step: lib.mdx_prs_create(out, 0, 2, 3, 0, 2.0, n, p(lags), step, p(DIMS), 0, 32, 1),
        "hb": lambda n, lags, step: lib.mdx_hb_create(out, 0, 3, 1, p(H_ROW), p(D_ROW), 1, p(A_ROW), 2.0, -0.5, n,
                                                      p(lags), step, p(DIMS), 0, 32, 1),
    }


# engine: (its destroy, the most lags it takes, what it says to one more, whether it has an origin_step)
ENGINES = {
    "vh": ("mdx_vh_destroy", 1 << 24, NONE, False),
    "chi4": ("mdx_chi4_destroy", 1 << 16, "lags must hold at least one lag and at most 65536", True),
    "ori": ("mdx_ori_destroy", 1 << 24, NONE, False),
    "vhd": ("mdx_vhd_destroy", 65535, "at most 65535 lags", True),
    "prs": ("mdx_prs_destroy", (1 << 24) - 1, "at most 2^24 lags", True),
    "hb": ("mdx_hb_destroy", (1 << 24) - 1, "at most 2^24 lags", True),
}
NONE_SAID = {"vh": NONE, "chi4": "lags must hold at least one lag and at most 65536", "ori": NONE, "vhd": NONE,
             "prs": NONE, "hb": NONE}


@pytest.fixture(scope="module")
def long_lags():
    """0, 1, 2, ...: a good list of every length up to one more than the largest cap"""
    return np.arange((1 << 24) + 1, dtype=np.int64)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_create_refuses_bad_lags(engine, long_lags):
    lib, h = _lib.lib(), ctypes.c_void_p()
    create = _creates(lib, h)[engine]
    destroy, most, too_many, has_step = ENGINES[engine]
    i64 = lambda *v: np.array(v, dtype=np.int64)      # noqa: E731

    def refused(n, lags, step, message):
        rc = create(n, lags, step)
        said = lib.mdx_last_error().decode()
        assert rc == -1 and said == message, (engine, n, lags[:4], step, rc, said)

    # the other arguments are good ones: the same call with a good list makes a handle
    assert create(3, i64(0, 1, 3), 1) == 0, lib.mdx_last_error()
    assert getattr(lib, destroy)(h) == 0
    refused(0, i64(0), 1, NONE_SAID[engine])                            # empty
    refused(2, i64(-1, 0), 1, "lags must not be negative")              # negative first
    refused(3, i64(0, 2, 2), 1, "lags must be strictly increasing")     # equal neighbours
    refused(2, i64(3, 1), 1, "lags must be strictly increasing")        # decreasing
    refused(3, i64(0, 1, -2), 1, "lags must not be negative")           # negative behind good ones
    refused(most + 1, long_lags, 1, too_many)                           # one more than the engine takes
    if has_step:
        refused(3, i64(0, 1, 3), 0, "origin_step must be at least 1")
        refused(3, i64(0, 1, 3), -2, "origin_step must be at least 1")
    # the cap itself is a length the lag check accepts
    assert create(most, long_lags, 1) == 0, lib.mdx_last_error()
    assert getattr(lib, destroy)(h) == 0
