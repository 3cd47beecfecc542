"""CPU: the ragged filters without a device -- the exported symbols, the routing of apply_filter_ragged_batch (which kernel
family a filter goes to, and the two cases that keep the loop over the distinct lengths), applyFilter's exceptions, scipy's
own ValueErrors with the row named before anything is launched, and the C entries' argument checks, which answer before
any launch.  A stand-in for a device tensor carries shape, type and strides; the leaves that would launch are recorded."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from modulation_mfcc_amd import _lib, calc, filters, ragged

ENTRIES = ("mm_sosfiltfilt_ragged_f64", "mm_sosfiltfilt_ragged_f32_f64", "mm_stencil_ragged_f64", "mm_fir_filtfilt_ragged_f64",
           "mm_fir_filtfilt_ragged_f32_f64", "mm_savgol_ragged_f64")


class FakeDeviceTensor:
    """What ragged.device_rows looks at, and nothing that could launch."""
    __module__ = "torch.fake"
    is_cuda = True
    device = "cuda:0"

    def __init__(self, rows, n_max, dtype=torch.float64, stride=None):
        self.shape, self.dtype, self._stride = (rows, n_max), dtype, (stride or n_max, 1)

    def dim(self):
        return 2

    def stride(self, k):
        return self._stride[k]

    def double(self):
        return FakeDeviceTensor(*self.shape, torch.float64)

    def float(self):
        return FakeDeviceTensor(*self.shape, torch.float32)


@pytest.fixture
def leaves(monkeypatch):
    """Every function behind apply_filter_ragged_batch that would touch the device, replaced by a recorder."""
    seen = []

    def rec(name):
        def f(x, *a, **k):
            seen.append((name, x.dtype, a, k))
            return x
        return f
    for name in ("sosfiltfilt_ragged_batch", "fir_filtfilt_ragged_batch", "savgol_ragged_batch", "_apply_filter_per_length"):
        monkeypatch.setattr(filters, name, rec(name))
    monkeypatch.setattr(calc, "apply_stencil_ragged", rec("apply_stencil_ragged"))
    monkeypatch.setattr(ragged, "counts_on_device", lambda lens, dev: lens)
    return seen


def test_exported_symbols():
    import modulation_mfcc_amd as M
    for name in ("sosfiltfilt_ragged_batch", "fir_filtfilt_ragged_batch", "savgol_ragged_batch", "apply_filter_ragged_batch",
                 "applyFilter_batch"):
        assert getattr(M, name) is getattr(filters, name)
    hdr = open(os.path.join(ROOT, "include", "modmfcc.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"\bsize_t mm_sosfiltfilt_ragged_workspace_bytes\(", hdr)
    assert _lib.MM_RAGGED_MAX_SEC == 4


LENS = [400, 350, 1000, 512]


@pytest.mark.parametrize("kw,dtype,leaf", [
    (dict(filt="iir", cutOff=[12]), torch.float64, "sosfiltfilt_ragged_batch"),
    (dict(filt="iir", cutOff=[12]), torch.float32, "sosfiltfilt_ragged_batch"),                  # float32 up to the kernel
    (dict(filt="iir", cutOff=[12], filtLen=8), torch.float64, "sosfiltfilt_ragged_batch"),      # four sections
    (dict(filt="iir", cutOff=[12], filtLen=9), torch.float64, "_apply_filter_per_length"),      # five: the loop stays
    (dict(filt="iir", cutOff=[3, 20], filtType="band", filtLen=6), torch.float64, "_apply_filter_per_length"),
    (dict(filt="fir", cutOff=[12], filtLen=6), torch.float64, "apply_stencil_ragged"),
    (dict(filt="fir", cutOff=[12], filtLen=8), torch.float64, "apply_stencil_ragged"),
    (dict(filt="fir", cutOff=[12], filtLen=9), torch.float64, "fir_filtfilt_ragged_batch"),
    (dict(filt="fir", cutOff=[12], filtLen=6), torch.float32, "_apply_filter_per_length"),      # float32, <= 8 taps: the loop
    (dict(filt="fir", cutOff=[12], filtLen=9), torch.float32, "fir_filtfilt_ragged_batch"),
    (dict(filt="fir", cutOff=[12], coeffs=np.ones(101) / 101), torch.float64, "fir_filtfilt_ragged_batch"),
    (dict(filt="sg", cutOff=[12], filtLen=7), torch.float64, "apply_stencil_ragged"),
    (dict(filt="sg", cutOff=[12], filtLen=16, polyOrd=2), torch.float32, "apply_stencil_ragged"),
    (dict(filt="sg", cutOff=[12], filtLen=17), torch.float64, "savgol_ragged_batch"),
    (dict(filt="sg", cutOff=[12], filtLen=101), torch.float32, "savgol_ragged_batch"),
])
def test_routing(kw, dtype, leaf, leaves):
    x = FakeDeviceTensor(len(LENS), max(LENS), dtype, stride=max(LENS) + 5)
    filters.apply_filter_ragged_batch(x, LENS, 100.0, **kw)
    assert [s[0] for s in leaves] == [leaf], leaves
    name, seen_dtype, args, kwargs = leaves[0]
    if leaf == "apply_stencil_ragged":
        assert seen_dtype == torch.float64                       # the banded operator takes float64 rows
        want = 3 * kw["filtLen"] + 1 if kw["filt"] == "fir" else 0
        assert kwargs.get("n_min", 0) == want                    # filtfilt's own minimum travels with the operator
    elif leaf != "_apply_filter_per_length":
        assert seen_dtype == dtype                               # the long kernels and the IIR rows take the caller's type


def test_apply_filter_exceptions(leaves):
    x = FakeDeviceTensor(len(LENS), max(LENS))
    f = filters.apply_filter_ragged_batch
    with pytest.raises(Exception, match="without specifying a cut Off freq"):
        f(x, LENS, 100.0, filt="iir", cutOff=None)
    with pytest.raises(Exception, match="among iir, fir and  sg"):
        f(x, LENS, 100.0, filt=None, cutOff=[12])
    with pytest.raises(Exception, match="filtType must be one among"):
        f(x, LENS, 100.0, cutOff=[12], filtType="notch")
    with pytest.raises(Exception, match="smaller than the half of the sampling freq"):
        f(x, LENS, 100.0, cutOff=[60])
    with pytest.raises(Exception, match=r"cutOff\[0\]<cutOff\[1\]"):
        f(x, LENS, 100.0, cutOff=[20, 3], filtType="band")
    with pytest.raises(Exception, match="only one or two cut off frequencies allowed"):
        f(x, LENS, 100.0, cutOff=[3, 20])
    with pytest.raises(Exception, match="sg .* filters can only be lowpass"):
        f(x, LENS, 100.0, filt="sg", cutOff=[3, 20], filtType="band")
    with pytest.raises(UnboundLocalError):
        f(x, LENS, 100.0, filt="median", cutOff=[12])
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        f(x, LENS, 100.0, filt="sg", cutOff=[12], filtLen=3, polyOrd=3)
    assert not leaves


def test_argument_errors(leaves):
    f = filters.apply_filter_ragged_batch
    with pytest.raises(TypeError, match="CUDA"):
        f(np.zeros((2, 100)), [100, 50], 100.0, cutOff=[12])
    with pytest.raises(TypeError, match="CUDA"):
        f(FakeDeviceTensor(2, 100, torch.int16), [100, 50], 100.0, cutOff=[12])
    x = FakeDeviceTensor(4, 1000)
    with pytest.raises(ValueError, match=r"lengths must have shape \(4,\)"):
        f(x, [400, 400, 400], 100.0, cutOff=[12])
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 1000\]"):
        f(x, [400, 0, 400, 400], 100.0, cutOff=[12])
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 1000\]"):
        f(x, [400, 1001, 400, 400], 100.0, cutOff=[12])
    with pytest.raises(TypeError, match="lengths must be integers"):
        f(x, [400.0, 400.0, 400.0, 400.0], 100.0, cutOff=[12])
    assert not leaves


def test_scipys_refusals_name_the_row(monkeypatch):
    """Host lengths scipy would refuse: scipy's text, the first such row and its length appended, before any launch."""
    monkeypatch.setattr(ragged, "counts_on_device", lambda lens, dev: pytest.fail("lengths were uploaded"))
    monkeypatch.setattr(calc, "apply_stencil_ragged", lambda *a, **k: pytest.fail("launched"))
    x = FakeDeviceTensor(4, 1000)
    f = filters.apply_filter_ragged_batch
    cases = [
        (dict(filt="iir", cutOff=[12]), 21, r"greater than padlen, which is 21\."),
        (dict(filt="iir", cutOff=[12], filtLen=5), 18, r"greater than padlen, which is 18\."),     # an odd order: ntaps 6
        (dict(filt="fir", cutOff=[12], filtLen=6), 18, r"greater than padlen, which is 18\."),
        (dict(filt="fir", cutOff=[12], filtLen=101), 303, r"greater than padlen, which is 303\."),
        (dict(filt="sg", cutOff=[12], filtLen=7), 6, r"window_length must be less than or equal to the size of x\."),
        (dict(filt="sg", cutOff=[12], filtLen=101), 100, r"window_length must be less than or equal to the size of x\."),
    ]
    for kw, short, text in cases:
        with pytest.raises(ValueError, match=text + rf" \(row 2 has {short} samples\)") as err:
            f(x, [1000, 400, short, short - 1 if short > 1 else 1], 100.0, **kw)
        assert isinstance(err.value, filters.RowRefused) and err.value.row == 2 and err.value.n == short
        assert re.search(text + "$", err.value.base)          # scipy's text on its own, for callers that name a clip instead
    # the three batch functions themselves
    sos = filters.iir_sos(100.0, cutOff=[12])
    with pytest.raises(filters.RowRefused, match=r"padlen, which is 21\. \(row 0 has 21 samples\)"):
        filters.sosfiltfilt_ragged_batch(x, [21, 400, 400, 1000], sos)
    with pytest.raises(filters.RowRefused, match=r"padlen, which is 27\. \(row 3 has 27 samples\)"):
        filters.fir_filtfilt_ragged_batch(x, [28, 400, 400, 27], np.ones(9) / 9)
    with pytest.raises(ValueError, match="at least two taps"):
        filters.fir_filtfilt_ragged_batch(x, [400] * 4, [1.0])
    with pytest.raises(ValueError, match="sos array must be shape"):
        filters.sosfiltfilt_ragged_batch(x, [400] * 4, np.ones((2, 5)))


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """MM_ERR_INVALID_ARG (-1) for every bad argument, MM_ERR_UNSUPPORTED (-2) for more than 4 sections, MM_ERR_WORKSPACE
    (-4) below the query; the pointers are never dereferenced."""
    import ctypes as C
    import scipy.signal
    lib = _lib.load()
    fake = 4096
    q = lib.mm_sosfiltfilt_ragged_workspace_bytes
    assert q(0, 100) == 0 and q(3, 0) == 0 and q(-1, 100) == 0
    need = int(q(3, 2000))
    assert 0 < need <= int(lib.mm_sosfiltfilt_workspace_bytes(3, 2000))
    s3, s5 = (np.ascontiguousarray(scipy.signal.butter(o, 0.1, output="sos")) for o in (6, 10))
    for fn in (lib.mm_sosfiltfilt_ragged_f64, lib.mm_sosfiltfilt_ragged_f32_f64):
        def call(x=fake, rows=3, n=2000, xs=2000, lens=fake, s=s3, ns=None, y=fake, ws=fake, wsb=need):
            return fn(x, rows, n, xs, lens, s.ctypes.data, s.shape[0] if ns is None else ns, y, ws, wsb, None)
        assert call(lens=None) == -1
        assert call(x=None) == -1 and call(y=None) == -1 and call(ws=None) == -1
        assert call(rows=0) == -1 and call(n=0) == -1 and call(xs=1999) == -1 and call(ns=0) == -1
        assert call(n=21, xs=21) == -1                        # not even the longest row exceeds padlen
        assert call(s=s5) == -2
        assert call(wsb=need - 1) == -4
    cs = calc._c_stencil(filters.fir_filtfilt_stencil(np.ones(6) / 6), 19)
    assert cs.reserved == 19
    st = lib.mm_stencil_ragged_f64
    assert st(C.byref(cs), fake, 3, 100, 100, None, fake, None) == -1
    assert st(None, fake, 3, 100, 100, fake, fake, None) == -1
    assert st(C.byref(cs), fake, 3, 100, 99, fake, fake, None) == -1
    assert st(C.byref(cs), fake, 3, 9, 100, fake, fake, None) == -1        # n_max below the operator's edge rows
    for fn in (lib.mm_fir_filtfilt_ragged_f64, lib.mm_fir_filtfilt_ragged_f32_f64):
        assert fn(fake, 1, 100, 100, None, fake, 9, fake, 100, None) == -1          # NULL lengths
        assert fn(None, 1, 100, 100, fake, fake, 9, fake, 100, None) == -1
        assert fn(fake, 1, 27, 27, fake, fake, 9, fake, 27, None) == -1             # n_max == 3 L
        assert fn(fake, 1, 100, 100, fake, fake, 1, fake, 100, None) == -1          # a single tap
        assert fn(fake, 2, 100, 99, fake, fake, 9, fake, 100, None) == -1
        assert fn(fake, 2, 100, 100, fake, fake, 9, fake, 99, None) == -1
    sg = lib.mm_savgol_ragged_f64
    assert sg(fake, 1, 100, 100, None, fake, fake, fake, 21, 4, fake, 100, None) == -1
    assert sg(None, 1, 100, 100, fake, fake, fake, fake, 21, 4, fake, 100, None) == -1
    assert sg(fake, 1, 100, 100, fake, fake, None, fake, 21, 4, fake, 100, None) == -1
    assert sg(fake, 1, 20, 20, fake, fake, fake, fake, 21, 4, fake, 20, None) == -1            # window > n_max
    assert sg(fake, 1, 100, 100, fake, fake, fake, fake, 21, 22, fake, 100, None) == -1
