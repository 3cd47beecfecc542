"""Host side (no GPU) of the Lomb-Scargle modulation spectrum: the yardstick of tests/lomb_oracle.py admits the kernel's
one-pass algebra and refuses wrong ones, every fixture's bound stays under the ceiling, the fifth header and its ctypes
table, the refusals of the C entry before any launch, and the argument errors of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lomb_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, lomb

HEADER = os.path.join(ROOT, "include", "modmfcc_lomb.h")


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS, ids=O.combo_id)
@pytest.mark.parametrize("name", O.NAMES)
def test_every_bound_is_under_the_ceiling(name, combo):
    want, sp, b = O.reference(name, combo)
    assert O.FLOOR <= b <= O.CEILING and np.isfinite(want).all() and sp < O.CEILING / O.MARGIN
    t, x, f = O.fixture(name)
    v = ~np.isnan(x)
    assert v.sum() >= 37 and f.min() >= 2.0 / (len(t) / O.FS) * (1 - 1e-12) and f.max() <= 0.45 * O.FS


@pytest.mark.parametrize("combo", O.COMBOS, ids=O.combo_id)
@pytest.mark.parametrize("name", O.SHORT_NAMES)
def test_the_one_pass_algebra_passes(name, combo):
    t, x, f = O.fixture(name)
    O.check(O.one_pass(t, x, f, **O._kw(combo)), name, combo)


@pytest.mark.parametrize("combo", [O.COMBOS[0], (True, True, "amplitude")], ids=O.combo_id)
def test_the_one_pass_algebra_passes_on_the_long_row(combo):
    """(two of the twelve: NumPy takes a second a combination on 210 000 x 64)"""
    t, x, f = O.fixture("long")
    O.check(O.one_pass(t, x, f, **O._kw(combo)), "long", combo)


def test_the_recorded_long_reference_is_what_the_oracle_computes():
    """tests/golden/lomb/lomb_long.npz against a fresh evaluation of every 16th frequency of one combination (scipy's
    result at a frequency does not depend on the others but for the rounding of its matrix products)."""
    combo = (True, False, "amplitude")
    want, sp, _ = O.reference("long", combo)
    part, sp_part = O.compute_reference("long", combo, every=16)
    assert np.abs(part - want[::16]).max() <= 1e-13 * np.abs(want).max()
    # (spreads are relative to the largest value of their own grid: compared as absolute errors)
    assert sp_part * np.abs(part).max() <= 2.0 * sp * np.abs(want).max()


def test_it_catches_wrong_algebra():
    t, x, f = O.fixture("f0-gaps")
    for combo in O.COMBOS:
        want, _, b = O.reference("f0-gaps", combo)
        filled = np.where(np.isnan(x), np.nanmean(x), x)                         # gaps filled in instead of masked
        assert O.measure(O.one_pass(t, filled, f, **O._kw(combo)), want) > 1e3 * b
        assert O.measure(want * (1 + 1e-9), want) > b                             # a relative error of 1e-9
        got = want.copy()
        got[7] = np.nan
        assert O.measure(got, want) == np.inf
    fm = O.reference("f0-gaps", (True, False, "power"))
    assert O.measure(O.one_pass(t, x, f, floating_mean=False), fm[0]) > 1e3 * fm[2]        # the floating mean left out
    pc = O.reference("f0-gaps", (False, True, "power"))
    assert O.measure(O.one_pass(t, x, f), pc[0]) > 1e3 * pc[2]                             # precenter left out
    am = O.reference("f0-gaps", (False, False, "amplitude"))
    assert O.measure(np.conj(am[0]), am[0]) > 1e3 * am[2]                                  # the sign of b / tau


def test_longdouble_is_wider_and_the_combinations_are_twelve():
    assert np.finfo(np.longdouble).eps < 1e-18 and len(O.COMBOS) == 12 == len(set(O.COMBOS))
    assert (O.FLOOR, O.MARGIN, O.CEILING) == (1e-12, 16.0, 1e-10)


# ---- the fifth header ------------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_fifth_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_LOMB) and len(protos) == 3, set(protos) ^ set(_lib.PROTOTYPES_LOMB)
    assert not set(protos) & (set(_lib.PROTOTYPES) | set(_lib.PROTOTYPES_MODPSD) | set(_lib.PROTOTYPES_MODCSD)
                              | set(_lib.PROTOTYPES_SPLINE))
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_lomb.h but not exported"
        res, args = _lib.PROTOTYPES_LOMB[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    res, args = _lib.PROTOTYPES_LOMB["mm_lombscargle_f64"]
    assert args[-1] is C.c_void_p and res is C.c_int
    txt = open(HEADER).read()
    assert lib.mm_lomb_version() == int(re.search(r"#define MM_LOMB_VERSION (\d+)", txt).group(1)) == 100
    assert int(re.search(r"#define MM_LOMB_CHUNK (\d+)", txt).group(1)) == _lib.MM_LOMB_CHUNK == lomb.LOMB_CHUNK
    for name in ("PRECENTER", "FLOATING_MEAN", "POWER", "NORMALIZE", "AMPLITUDE"):
        m = re.search(rf"MM_LOMB_{name}\s*=\s*(\d+)(?:\s*<<\s*(\d+))?", txt)
        assert int(m.group(1)) << int(m.group(2) or 0) == getattr(_lib, "MM_LOMB_" + name), name
    assert lomb._NORMALIZE == {"power": _lib.MM_LOMB_POWER, "normalize": _lib.MM_LOMB_NORMALIZE,
                               "amplitude": _lib.MM_LOMB_AMPLITUDE}
    assert lib.mm_version() == 123                                           # nothing in the other headers changed


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_lomb\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_lomb\.h", mk, flags=re.M)
    assert '#include "mm_lomb.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in open(os.path.join(csrc, "mm_lomb.hip")).read()


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null, 256-byte aligned "pointer": every call below must return before it is looked at


def _call(x=P, rows=2, n=100, xs=100, lens=None, t=P, om=P, nf=5, flags=0, out=P, os_=5, im=None, ws=P, wb=1 << 40):
    return _lib.load().mm_lombscargle_f64(x, rows, n, xs, lens, t, om, nf, flags, out, os_, im, ws, wb, None)


@pytest.mark.parametrize("bad", [dict(x=None), dict(t=None), dict(om=None), dict(out=None), dict(rows=0), dict(rows=-1),
                                 dict(n=0), dict(nf=0), dict(nf=-3), dict(xs=99), dict(os_=4), dict(flags=16), dict(flags=-1),
                                 dict(flags=3 << 2), dict(flags=_lib.MM_LOMB_AMPLITUDE),
                                 dict(rows=(1 << 19) + 1), dict(n=(1 << 30) + 1, xs=(1 << 30) + 1),
                                 dict(nf=(1 << 20) + 1, os_=(1 << 20) + 1), dict(rows=1 << 19, nf=1 << 19, os_=1 << 19),
                                 dict(rows=1 << 19, n=1 << 22, xs=1 << 22),
                                 dict(rows=1 << 17, n=1 << 18, xs=1 << 18), dict(rows=1 << 16, nf=1 << 16, os_=1 << 16)])
def test_invalid_arguments_are_refused_before_any_launch(bad):
    assert _call(**bad) == _lib.MM_ERR_INVALID_ARG
    if set(bad) <= {"rows", "n", "nf", "xs", "os_"} and not set(bad) <= {"xs", "os_"}:
        d = dict(rows=2, n=100, nf=5)
        d.update({k: v for k, v in bad.items() if k in d})
        assert _lib.load().mm_lombscargle_workspace_bytes(d["rows"], d["n"], d["nf"]) == 0


@pytest.mark.parametrize("n", [1, 100, 512, 513, 5000])
def test_a_missing_misaligned_or_short_workspace_is_refused(n):
    need = _lib.load().mm_lombscargle_workspace_bytes(2, n, 5)
    assert need > 0 and need % 256 == 0
    for bad in (dict(wb=need - 1), dict(wb=0), dict(ws=None), dict(ws=P + 8), dict(ws=P + 128)):
        assert _call(n=n, xs=n, **bad) == _lib.MM_ERR_WORKSPACE
    assert _call(n=n, xs=n, flags=_lib.MM_LOMB_AMPLITUDE, wb=0) == _lib.MM_ERR_INVALID_ARG      # arguments first


def test_the_workspace_size():
    f = _lib.load().mm_lombscargle_workspace_bytes
    s = lomb.LOMB_CHUNK
    sizes = [f(3, n, 7) for n in (1, s - 1, s, s + 1, 2 * s, 2 * s + 1, 300001)]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert f(3, s, 7) == f(3, 1, 7) < 4 * 256 < f(3, s + 1, 7)              # one chunk: no partial sums
    assert f(3, s + 1, 7) >= 2 * 6 * 3 * 7 * 8                               # two chunks of six sums per (row, frequency)
    assert f(1, 1 << 30, 1) > 0 and f(1, (1 << 30) + 1, 1) == 0


# ---- Python, without a device -----------------------------------------------------------------------------------------------------
def test_the_names_are_exported():
    import modulation_mfcc_amd as M
    assert M.modulation_lombscargle_batch is lomb.modulation_lombscargle_batch
    assert M.modulation_lombscargle_ragged_batch is lomb.modulation_lombscargle_ragged_batch
    assert M.modulation_lombscargle_list is lomb.modulation_lombscargle_list


def test_argument_errors_are_scipys():
    import torch
    from scipy.signal import lombscargle
    x = torch.ones((2, 10), dtype=torch.float64)
    f = np.array([1.0, 2.0])
    calls = (lambda **kw: lomb.modulation_lombscargle_batch(x, 100.0, kw.pop("f", f), **kw),
             lambda **kw: lomb.modulation_lombscargle_ragged_batch(x, [10, 10], 100.0, kw.pop("f", f), **kw))
    for bad in (dict(normalize="psd"), dict(normalize=None), dict(normalize=2), dict(f=[]), dict(f=np.ones((2, 2))), dict(f=3.0)):
        with pytest.raises(ValueError) as ours:
            calls[0](**dict(bad))
        with pytest.raises(ValueError) as theirs:
            lombscargle(np.arange(10.0), np.ones(10), np.asarray(bad.get("f", f), dtype=np.float64) * 2 * np.pi,
                        normalize=bad.get("normalize", False))
        assert str(ours.value) == str(theirs.value)
        with pytest.raises(ValueError, match=re.escape(str(theirs.value))):
            calls[1](**dict(bad))
    for call in calls:                                       # valid arguments, host data: no host fallback
        with pytest.raises(TypeError, match="CUDA"):
            call()
        with pytest.raises(TypeError, match="CUDA"):
            call(normalize="amplitude", floating_mean=True, precenter=True)
    with pytest.raises(TypeError, match="CUDA"):
        lomb.modulation_lombscargle_list([x[0]], 100.0, f)
    assert lomb._flags(False, False, False) == 0 and lomb._flags(True, True, True) == 1 | 2 | _lib.MM_LOMB_NORMALIZE
    assert lomb._flags(False, "amplitude", True) == 2 | _lib.MM_LOMB_AMPLITUDE and lomb._flags(False, "power", False) == 0


def test_a_host_time_axis_must_be_finite_and_the_axis_cache_is_bounded():
    for bad in (np.nan, np.inf):
        t = np.arange(10) / 100.0
        t[7] = bad
        with pytest.raises(ValueError, match="finite at every index"):
            lomb._time_axis(t, 10, 100.0, "cpu")
    with pytest.raises(ValueError, match="equal non-zero length"):
        lomb._time_axis(np.arange(9.0), 10, 100.0, "cpu")
    lomb._axes.clear()
    for n in range(1, 40):
        lomb._time_axis(None, n, 100.0, "cpu")
    assert len(lomb._axes) == lomb._AXES_KEPT == 16 and (39, 100.0, "cpu") in lomb._axes
    lomb._axes.clear()


def test_the_launch_limits_are_the_headers():
    f = _lib.load().mm_lombscargle_workspace_bytes
    assert f(1 << 17, 1 << 17, 1) > 0 and f(1 << 17, (1 << 18) - 511, 1) == 0          # rows x chunks < 2^26
    assert f((1 << 16) - 1, 100, 1 << 16) > 0 and f(1 << 16, 100, 1 << 16) == 0         # rows x n_freq < 2^32
    txt = open(HEADER).read()
    assert "< 2^26" in txt and "rows * n_freq < 2^32" in txt


def test_the_default_axis_and_the_grid_are_the_oracles():
    assert np.array_equal(lomb.default_time_axis(1001, 100.0), O.time_axis(1001))
    f = O.grid(1001)
    assert np.array_equal(lomb._omega(f), 2.0 * np.pi * np.asarray(f, dtype=np.float64))
