"""
The 16.16 fixed-point bin position of the cell-sorted pair kernel's LDS form against the float32 form it replaces, on
the CPU, with the engine's own constants (``mdx_rdf_filter_constants``).

Both forms are restated in NumPy with a correctly rounded float32 fma:

* float form (global-histogram steps, and every LDS step before the fixed-point one):
  ``pos = fl32(s inv_w + pos0)``, sure ``<=> fract(pos) < sure_w``, bin ``floor(pos)``;
* fixed-point form: ``q = floor(fl32(s IWQ + P0Q))`` as a 32-bit integer, sure ``<=> low16(q) < TQ``, bin
  ``high16(q)``.

``IWQ`` and ``P0Q`` are ``inv_w`` and ``pos0`` times 2^16, so the float the convert reads is ``2^16 pos`` to the bit and
``q = floor(2^16 pos)``: every pair the fixed-point form calls sure the float form calls sure, with the same bin, and
the pairs only the float form calls sure have ``fract(pos)`` in ``[TQ 2^-16, sure_w)`` — less than 2^-16 of a bin.

Samples: every float32 ``s`` within 64 ulp of the image of each bin edge and of each end of each sure window, and 10^6
random ones, uniform over the range (so that a share of samples is a share of bin width).
"""
import numpy as np
import pytest

from mdhelper_amd import _core

C2_BOX = 68.94
# name: (r0, r1, n_bins, box length)
CASES = {"C2": (0.0, 15.0, 201, C2_BOX), "range-3-6": (3.0, 6.0, 60, 30.0), "box-10": (0.0, 5.0, 100, 10.0)}
for _n in (1, 126, 127, 254, 255, 256, 2000):
    CASES[f"bins-{_n}"] = (0.0, 6.0, _n, 30.0)
    CASES[f"bins-{_n}-lower"] = (3.0, 6.0, _n, 30.0)


def fma32(a, b, c):
    """fl32(a b + c) of float32 arrays, one rounding: the product of two float32 values is exact in float64, its sum
    with c is split into a float64 head and its error (two-sum), and a head that is not exact is made odd, after which
    the rounding to float32 cannot land on a tie the error would have broken."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    hi = p + c
    v = hi - p
    lo = (p - (hi - v)) + (c - v)
    bits = hi.view(np.int64)
    fix = (lo != 0.0) & ((bits & 1) == 0)
    # (the neighbour of an even head is odd; hi == 0 with lo != 0 cannot happen: a sum that rounds to zero is exact)
    hi = np.where(fix, np.nextafter(hi, np.where(lo > 0.0, np.inf, -np.inf)), hi)
    return hi.astype(np.float32)


def constants(case):
    r0, r1, n_bins, L = CASES[case]
    edges = np.linspace(r0, r1, n_bins + 1)
    return edges, _core.RdfEngine.filter_constants(edges, [L, L, L], L)


def float_form(s, k):
    pos = fma32(s, np.float32(k["inv_w"]), np.float32(k["pos0"]))
    fl = np.floor(pos)
    fract = np.minimum(pos - fl, np.float32(1.0) - np.float32(2.0 ** -24))   # v_fract_f32 stays below 1
    return fract < np.float32(k["sure_w"]), fl.astype(np.int64)


def fixed_form(s, k):
    qf = fma32(s, np.float32(k["iwq"]), np.float32(k["p0q"]))
    assert np.all(np.abs(qf) < 2.0 ** 31)   # nowhere near the convert's saturation
    q = np.floor(qf.astype(np.float64)).astype(np.int64) & 0xFFFFFFFF
    high = q >> 16
    return (q & 0xFFFF) < k["tq"], np.where(high >= 0x8000, high - 0x10000, high)


def neighbours(centres):
    """every float32 within 64 ulp of the float32 nearest to each centre"""
    c = np.asarray(centres, dtype=np.float64).astype(np.float32)
    c = c[c > 0]
    out = c.view(np.int32)[:, None] + np.arange(-64, 65, dtype=np.int32)[None, :]
    out = out[out >= 0]
    return np.unique(out.astype(np.int32).view(np.float32))


def samples(case, edges, k):
    r0, r1, n_bins, _ = CASES[case]
    w = (r1 - r0) / n_bins
    eta = k["eta"]
    sets = [neighbours(edges)]
    if 2.0 * eta < 1.0:
        sets.append(neighbours(edges[:-1] + eta * w))           # fract(pos) = 0: a sure window opens
        sets.append(neighbours(edges[1:] - eta * w))            # fract(pos) = sure_w: it closes
        sets.append(neighbours(edges[:-1] + eta * w + (k["sure_w"] - k["tq"] / 65536.0) * w))
    near = np.concatenate(sets)
    rng = np.random.default_rng(17)
    rand = rng.uniform(r0, r1, 1_000_000).astype(np.float32)
    return near, rand


def window(s, k):
    """candidates only: the step classifies no other pair"""
    r2 = s * s
    return s[(r2 < np.float32(k["cand_hi"])) & (r2 >= np.float32(k["cand_lo"]))]


@pytest.mark.parametrize("case", sorted(CASES))
def test_constants_are_exact_scalings(case):
    _, k = constants(case)
    assert k["tq"] == min(max(int(np.floor(k["sure_w"] * 65536.0)), 0), 65535)
    if k["sure_w"] > 0:
        assert k["tq"] == int(np.floor(k["sure_w"] * 65536.0))
    assert k["iwq"] == k["inv_w"] * 65536.0 and k["p0q"] == k["pos0"] * 65536.0
    assert np.float32(k["sure_w"]) == np.float32(1.0) - np.float32(2.0) * np.float32(k["eta"])
    assert 0.0 < k["eta"] <= 1.0


@pytest.mark.parametrize("case", sorted(CASES))
def test_fixed_point_sure_is_float_sure_with_the_same_bin(case):
    edges, k = constants(case)
    near, rand = samples(case, edges, k)
    n_bins = CASES[case][2]
    for s in (window(near, k), window(rand, k)):
        sure_f, bin_f = float_form(s, k)
        sure_q, bin_q = fixed_form(s, k)
        assert not np.any(sure_q & ~sure_f), s[sure_q & ~sure_f][:8]
        assert np.array_equal(bin_q[sure_q], bin_f[sure_q])
        assert np.all((bin_q[sure_q] >= 0) & (bin_q[sure_q] <= n_bins))
        # what only the float form calls sure lies in [TQ 2^-16, sure_w) of its bin
        only = sure_f & ~sure_q
        pos = fma32(s[only], np.float32(k["inv_w"]), np.float32(k["pos0"])).astype(np.float64)
        assert np.all(pos - np.floor(pos) >= k["tq"] / 65536.0)
    # negative positions (a candidate has pos > -2 eta) are undecided in both forms
    s = window(near, k)
    neg = fma32(s, np.float32(k["inv_w"]), np.float32(k["pos0"])) < 0
    if 2.0 * k["eta"] < 1.0:
        assert not np.any(float_form(s[neg], k)[0]) and not np.any(fixed_form(s[neg], k)[0])


@pytest.mark.parametrize("case", sorted(CASES))
def test_undecided_share_grows_by_less_than_two_to_the_minus_15(case):
    edges, k = constants(case)
    _, rand = samples(case, edges, k)
    s = window(rand, k)
    und_f = np.count_nonzero(~float_form(s, k)[0])
    und_q = np.count_nonzero(~fixed_form(s, k)[0])
    print(f"{case}: undecided share {und_f / s.size:.6e} -> {und_q / s.size:.6e} (eta {k['eta']:.4e}, TQ {k['tq']})")
    assert und_f <= und_q <= und_f + s.size * 2.0 ** -15
