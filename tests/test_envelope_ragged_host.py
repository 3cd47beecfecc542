"""CPU: the ragged amplitude envelopes without a device -- the exported names, the frame counts of the ragged RMS, the
power-of-two class of a clip length and the grouping of the rows by it (the leaf that would launch is recorded), and the C
entries' argument checks, which answer before any launch.  (The checks of mm_hilbert_envelope_ragged that need a handle --
a row stride below n_max, a workspace one byte short -- are in tests/test_gpu_envelope_ragged.py: a handle owns device
tables, so none exists without a device.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from modulation_mfcc_amd import _lib, batch, calc, mfcc, ragged

ENTRIES = ("mm_rms_ragged_f32", "mm_hilbert_ragged_create", "mm_hilbert_envelope_ragged")


def test_exported_names():
    import modulation_mfcc_amd as M
    for name in ("hilbert_envelope_ragged_batch", "amplitude_envelope_ragged_batch", "calculate_amplitude_envelope_batch"):
        assert getattr(M, name) is getattr(calc, name) and name in calc.__all__
    for name in ("rms_ragged_batch", "rms_ragged_frames"):
        assert getattr(M, name) is getattr(batch, name)
    assert M.get_amplitude_batch is mfcc.get_amplitude_batch and "get_amplitude_batch" in mfcc.__all__
    hdr = open(os.path.join(ROOT, "include", "modmfcc.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(rf"\bint {name}\(", hdr), name
    assert "mm_hilbert_ragged_workspace_bytes" in _lib.PROTOTYPES and hasattr(lib, "mm_hilbert_ragged_workspace_bytes")
    assert re.search(r"\bsize_t mm_hilbert_ragged_workspace_bytes\(", hdr)


def test_get_amplitude_batch_is_the_calc_function(monkeypatch):
    seen = []
    monkeypatch.setattr(calc, "calculate_amplitude_envelope_batch", lambda clips, sr, **kw: seen.append((clips, sr, kw)) or "r")
    assert mfcc.get_amplitude_batch(["c"], 16000, method="Hilb", hopLen=0.02) == "r"
    assert seen == [(["c"], 16000, dict(method="Hilb", hopLen=0.02))]


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("frame,hop", [(400, 80), (401, 80), (64, 1), (5000, 100), (1, 1)])
def test_rms_ragged_frames_agrees_with_the_library(frame, hop, center):
    lib = _lib.load()
    lens = np.array([1, 2, 63, 64, 65, 399, 400, 401, 402, 4999, 5000, 5001, 16000, 160000, 160001])
    got = batch.rms_ragged_frames(lens, frame, hop, center)
    assert got.dtype == np.int64
    for n, g in zip(lens, got):
        want = lib.mm_rms_num_frames(int(n), frame, hop, 1 if center else 0)
        assert g == max(want, 0), (n, g, want)          # (no frame: the library answers MM_ERR_INVALID_ARG, the helper 0)
    assert batch.rms_ragged_frames([], frame, hop, center).shape == (0,)


def test_power_of_two_class_of_a_length():
    f = calc.hilbert_ragged_fft_size
    assert [f(n) for n in (1, 2, 8)] == [16, 16, 16]
    assert f(9) == 32                                    # 2 * 9 - 1 = 17
    for k in range(4, 24):
        assert f(2 ** k) == 2 ** (k + 1)                 # 2^(k+1) - 1 fits
        assert f(2 ** k + 1) == 2 ** (k + 2)             # 2^(k+1) + 1 does not
    for n in (3, 100, 4097, 65537, 70001, 160000):
        M = f(n)
        assert M >= max(16, 2 * n - 1) and (M == 16 or M // 2 < 2 * n - 1) and M & (M - 1) == 0
    got = calc._hilbert_ragged_classes(np.array([9, 1, 4097, 8, 16, 4096]))
    assert [(M, idx.tolist()) for M, idx in got] == [(16, [1, 3]), (32, [0, 4]), (8192, [5]), (16384, [2])]


@pytest.fixture
def leaf(monkeypatch):
    """A CPU tensor stands in for the device batch; the one function that would launch is recorded and answers with its
    transform length in every column."""
    seen = []

    def rows(x2, lens_dev, M):
        seen.append((M, tuple(x2.shape), lens_dev.tolist()))
        return torch.full(x2.shape, float(M), dtype=x2.dtype)
    monkeypatch.setattr(ragged, "is_device_tensor", lambda x: isinstance(x, torch.Tensor))
    monkeypatch.setattr(calc, "_hilbert_ragged_rows", rows)
    return seen


def test_rows_are_grouped_by_class_with_host_lengths(leaf):
    lens = [4097, 1, 300, 8, 4096, 257, 9]
    x = torch.zeros((7, 5000), dtype=torch.float32)
    y = calc.hilbert_envelope_ragged_batch(x, lens)
    # one call per class, ascending, each on its own rows cut to the class's longest clip
    assert leaf == [(16, (2, 8), [1, 8]), (32, (1, 9), [9]), (1024, (2, 300), [300, 257]), (8192, (1, 4096), [4096]),
                    (16384, (1, 4097), [4097])]
    assert y.shape == (7, 5000) and y.dtype == torch.float32
    want = {0: (16384, 4097), 1: (16, 8), 2: (1024, 300), 3: (16, 8), 4: (8192, 4096), 5: (1024, 300), 6: (32, 9)}
    for b, (M, n_c) in want.items():
        assert (y[b, :n_c] == M).all() and (y[b, n_c:] == 0).all(), b


def test_one_class_that_fills_the_batch_goes_as_it_is(leaf):
    x = torch.zeros((3, 1000), dtype=torch.float64)
    calc.hilbert_envelope_ragged_batch(x, np.array([1000, 600, 513]))
    assert leaf == [(2048, (3, 1000), [1000, 600, 513])]


def test_one_class_in_a_wider_batch_is_cut_to_its_longest_clip(leaf):
    """M = 256 covers 128 samples, not the batch's 4096 columns: the leaf sees [rows, 120], the rest of the result is zero."""
    x = torch.ones((4, 4096), dtype=torch.float32)
    y = calc.hilbert_envelope_ragged_batch(x, [100, 100, 90, 120])
    assert leaf == [(256, (4, 120), [100, 100, 90, 120])]
    assert y.shape == (4, 4096) and (y[:, :120] == 256).all() and (y[:, 120:] == 0).all()
    leaf.clear()
    calc.hilbert_envelope_ragged_batch(torch.ones((2, 1000)), [70, 70])            # equal short clips in a wide buffer
    assert leaf == [(256, (2, 70), [70, 70])]
    for M, shape, _ in leaf:
        assert 2 * shape[1] - 1 <= M


def test_ragged_handles_stay_out_of_the_single_length_lru(monkeypatch):
    made = []
    monkeypatch.setattr(calc, "_HilbertPlan", lambda n, code, device, ragged=False: made.append((n, code, ragged)) or object())
    monkeypatch.setattr(calc, "_HILBERT_RAGGED_PLANS", {})
    before = dict(calc._HILBERT_PLANS)
    plans = [calc._hilbert_ragged_plan(1 << p, 0, "cuda:0") for p in range(4, 26)]          # every M there is
    assert [calc._hilbert_ragged_plan(1 << p, 0, "cuda:0") for p in range(4, 26)] == plans  # all kept: nothing rebuilt
    assert made == [((1 << p) // 2, 0, True) for p in range(4, 26)]
    assert dict(calc._HILBERT_PLANS) == before


def test_argument_errors(leaf):
    f = calc.hilbert_envelope_ragged_batch
    x = torch.zeros((3, 100), dtype=torch.float32)
    with pytest.raises(TypeError, match="float32 / float64"):
        f(x.half(), [100, 50, 1])
    with pytest.raises(TypeError, match="CUDA"):
        f(np.zeros((3, 100), np.float32), [100, 50, 1])
    with pytest.raises(ValueError, match=r"\[B, n_max\]"):
        f(x[0], [100])
    for bad in ([100, 0, 1], [100, 101, 1], [100, -5, 1]):
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 100\]"):
            f(x, bad)
    with pytest.raises(ValueError, match=r"lengths must have shape \(3,\)"):
        f(x, [100, 50])
    with pytest.raises(TypeError, match="lengths must be integers"):
        f(x, [100.0, 50.0, 1.0])
    assert not leaf


def test_batch_call_refuses_what_the_single_call_refuses():
    f = calc.calculate_amplitude_envelope_batch
    assert f([], 16000) == [] and f([], 16000, method="Hilb", outFilter="iir") == []
    with pytest.raises(NotImplementedError, match="Praat"):
        f([np.zeros(100, np.float32)], 16000, method="RMSpraat")
    with pytest.raises(UnboundLocalError, match="unknown amplitude method 'rms'"):
        f([np.zeros(100, np.float32)], 16000, method="rms")
    with pytest.raises(NotImplementedError, match="Praat"):
        calc.amplitude_envelope_ragged_batch(None, [1], 16000, method="RMSpraat")
    with pytest.raises(UnboundLocalError):
        calc.amplitude_envelope_ragged_batch(None, [1], 16000, method="hilb")


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """MM_ERR_INVALID_ARG (-1) for every bad argument; the pointers are never dereferenced."""
    lib = _lib.load()
    fake = 4096

    def rms(x=fake, batch_=3, n=2000, xs=2000, lens=fake, frame=400, hop=80, center=1, y=fake):
        return lib.mm_rms_ragged_f32(x, batch_, n, xs, lens, frame, hop, center, y, None)
    assert rms(x=None) == -1 and rms(lens=None) == -1 and rms(y=None) == -1
    assert rms(batch_=0) == -1 and rms(xs=1999) == -1 and rms(n=0, xs=0) == -1
    assert rms(frame=0) == -1 and rms(hop=0) == -1
    assert rms(n=399, xs=399, center=0) == -1                  # not even the longest clip has a frame

    h = C.c_void_p()
    create = lib.mm_hilbert_ragged_create
    assert create(100, 0, None) == -1
    assert create(0, 0, C.byref(h)) == -1 and create(-3, 1, C.byref(h)) == -1
    assert create((1 << 24) + 1, 0, C.byref(h)) == -1          # n_max > 2^24
    assert create(100, 2, C.byref(h)) == -1 and create(100, -1, C.byref(h)) == -1
    assert not h.value

    q = lib.mm_hilbert_ragged_workspace_bytes
    assert q(None, 3, 100) == 0

    def env(hh=None, x=fake, rows=3, n=100, xs=100, lens=fake, y=fake, ys=100, ws=fake, wsb=1 << 30):
        return lib.mm_hilbert_envelope_ragged(hh, x, rows, n, xs, lens, y, ys, ws, wsb, None)
    assert env() == -1                                          # no handle
    # the row count is looked at before the handle: 0 and 65536 are refused whatever else is passed
    assert env(hh=fake, rows=0) == -1 and env(hh=fake, rows=65536) == -1 and env(hh=fake, rows=-1) == -1
    assert env(hh=fake, rows=0, x=None, lens=None, y=None, ws=None) == -1
