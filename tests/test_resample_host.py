"""CPU: the yardsticks of tests/test_gpu_resample.py, checked without a GPU.

  * the ratio matrix (tests/resample_comb.py) reaches every launch shape of mm_resample_banded_f32, as
    mm_resample_banded_shape -- the library's own host arithmetic -- reports it;
  * the impulse comb is a correct and complete probe: audio_io.banded_resample_numpy (the NumPy statement of the
    banded operator) reproduces the integer-indexed expectation exactly, and every tap of every copy of the period is
    visited; the same for the edge comb (impulses on the first and last sample);
  * the comb sees what the suite's noise comparison cannot: a table built from taps whose outer 5 % are zero.

Everything here is equality.
"""
import ctypes as C

import numpy as np
import pytest

import resample_comb as RC
from modulation_mfcc_amd import _lib
from modulation_mfcc_amd.audio_io import banded_resample_numpy, banded_tables

IDS = [RC.ratio_id(p) for p in RC.MATRIX]


def test_shape_query_validates_without_a_device():
    """mm_resample_banded_shape is host arithmetic: the argument rules of mm_resample_banded_f32, nothing written on
    failure, and the 1 / 3 tables' shape worked out by hand."""
    lib = _lib.load()
    tb = RC.tables(48000, 16000)["tabs"]
    assert (tb["F"], tb["S"], tb["NB"]) == (16, 48, 1)
    qt, pad, lds = C.c_int32(-7), C.c_int32(-7), C.c_size_t(77)
    good = (tb["F"], tb["S"], tb["NB"], tb["ksteps"], tb["win"])
    for bad in ((15, 48, 1), (16, 0, 1), (16, 48, 2), (16, 48, 1, 0), (16, 48, 1, tb["ksteps"] + 4),
                (16, 48, 1, tb["ksteps"], 4 * tb["ksteps"] - 1)):
        args = bad + good[len(bad):]
        assert lib.mm_resample_banded_shape(*args, C.byref(qt), C.byref(pad), C.byref(lds)) == _lib.MM_ERR_INVALID_ARG, bad
    assert lib.mm_resample_banded_shape(*good, None, C.byref(pad), C.byref(lds)) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_resample_banded_shape(*good, C.byref(qt), None, C.byref(lds)) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_resample_banded_shape(*good, C.byref(qt), C.byref(pad), None) == _lib.MM_ERR_INVALID_ARG
    assert (qt.value, pad.value, lds.value) == (-7, -7, 77)
    assert lib.mm_resample_banded_shape(*good, C.byref(qt), C.byref(pad), C.byref(lds)) == _lib.MM_OK
    # S = 48: periods q and q + 2 of a read share a bank (96 = 0 mod 32), eight to a bank -> padded; 16 * 8 periods of 48
    # samples + the window + 8, one pad word per 32 and one more
    fl = (16 * 8 - 1) * 48 + tb["win"] + 8
    assert (qt.value, pad.value, lds.value) == (8, 1, 4 * (fl + fl // 32 + 1))


def test_ratio_matrix_reaches_every_launch_shape():
    """QT 8 / 4 / 2 / 1, both pad values, every pipeline remainder G % 3, the period remainders F % 16 whose last block
    wraps into the next period, one-block and many-block periods, and ratios the matrix pipe refuses."""
    qts, pads, g3, f16, nbs = set(), set(), set(), set(), set()
    for pair in RC.MATRIX:
        tb = RC.tables(*pair)["tabs"]
        rc, qt, pad, lds = RC.shape_of(tb)
        assert rc == _lib.MM_OK, pair
        assert 0 < lds <= 160 * 1024
        qts.add(qt); pads.add(pad); g3.add(tb["ksteps"] // 8 % 3); f16.add(tb["F"] % 16); nbs.add(tb["NB"])
    assert qts == {8, 4, 2, 1}
    assert pads == {0, 1}
    assert g3 == {0, 1, 2}
    assert f16 >= {0, 3, 4, 8, 9, 14}
    assert 1 in nbs and max(nbs) >= 20
    assert len(RC.UNSUPPORTED) >= 1
    for pair in RC.UNSUPPORTED:
        rc, qt, pad, lds = RC.shape_of(RC.tables(*pair)["tabs"])
        assert (rc, qt, pad, lds) == (_lib.MM_ERR_UNSUPPORTED, -1, -1, 0), pair


@pytest.mark.parametrize("edge", [False, True], ids=["comb", "edge"])
@pytest.mark.parametrize("pair", RC.MATRIX, ids=IDS)
def test_comb_is_exact_and_complete(pair, edge):
    t = RC.tables(*pair)
    tb, L, h32 = t["tabs"], t["L"], t["h32"]
    x, want, tap = RC.comb(*pair, edge)
    assert len(x) <= 450000 and not np.signbit(want[want == 0]).any()
    got = banded_resample_numpy(x, tb, len(want))
    np.testing.assert_array_equal(got.astype(np.float32), want)         # (a) -- and nothing was rounded on the way
    np.testing.assert_array_equal(got, want.astype(np.float64))
    full = np.count_nonzero(h32) * tb["F"] // L
    assert (np.count_nonzero(h32) * tb["F"]) % L == 0
    if not edge:
        assert np.count_nonzero(want) == full                           # (b): every tap of every copy of the period
        assert np.count_nonzero(tap >= 0) == len(h32) * tb["F"] // L
        assert x[0] == 0 and x[-1] == 0
    else:
        # impulses on the first and the last sample; only what falls outside [0, n_out) is missing
        assert x[0] != 0 and x[-1] != 0
        # (half a response, len(h) / 2 M outputs, at either end)
        assert full - len(h32) // t["M"] - 2 <= np.count_nonzero(want) < full
        assert want[0] == x[0] * h32[t["half"]] and want[0] != 0


@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 16000)], ids=["48000to16000", "44100to16000"])
def test_comb_sees_a_table_with_its_outer_taps_zeroed(pair):
    """What the noise comparison at 2e-6 of the maximum lets through (1.0e-6 and 1.2e-6 with scipy on both sides, the
    outer 5 % of each half of the filter zeroed; it first fails at 8 %), the comb reports tap by tap: every mismatch
    is a zeroed tap, and every zeroed tap is a mismatch."""
    t = RC.tables(*pair)
    h32, L, M = t["h32"], t["L"], t["M"]
    cut = int(0.05 * t["half"])             # 5 % of each half of the symmetric filter, at either end
    hz = h32.astype(np.float64)
    hz[:cut] = 0.0
    hz[len(hz) - cut:] = 0.0
    tz = banded_tables(L, M, hz, t["half"])
    x, want, tap = RC.comb(*pair)
    got = banded_resample_numpy(x, tz, len(want)).astype(np.float32)
    bad = got != want
    assert bad.any()
    outer = (tap >= 0) & ((tap < cut) | (tap >= len(h32) - cut))
    np.testing.assert_array_equal(bad, outer & (want != 0))
    assert (got[bad] == 0).all()
