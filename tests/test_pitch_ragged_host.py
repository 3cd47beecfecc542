"""CPU: the host side of the ragged pYIN path -- the frame counts, the new C symbols in the header and the binding, the
workspace query, the argument checks that fire before any launch, the validation of host lengths, and the signature of
get_f0_batch.  (The library loads without a GPU, as pitch.pyin_params shows.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import pyin_oracle as O
from modulation_mfcc_amd import _lib, get_f0, get_f0_batch, interp, pitch, pyin_ragged_frames
from modulation_mfcc_amd.plan import check_lengths

C5 = dict(frame_length=512, hop_length=40, fmin=100, fmax=500)
C5_SR = 8000
LENGTHS = [4000, 1, 39, 40, 80, 599, 600, 640, 3999]
LENGTHS_NC = [4000, 512, 551, 552, 511]
NEW = {"mm_pyin_ragged_workspace_bytes": 3, "mm_pyin_ragged_f32": 15, "mm_pyin_ragged_f64": 15,
       "mm_interp_nan_linear_ragged_f64": 8, "mm_interp_nan_ragged_f64": 11}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "modmfcc.h")


def _oracle_frames(n, center):
    return O.sizes(n, C5_SR, C5["fmin"], C5["fmax"], C5["frame_length"], None, C5["hop_length"], center=center)["n_frames"]


def test_frames_are_the_oracles_and_the_librarys():
    lib = _lib.load()
    got = pyin_ragged_frames(LENGTHS, 512, 40)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    assert got.tolist() == [101, 1, 1, 2, 3, 15, 16, 17, 100]
    assert got.tolist() == [_oracle_frames(n, True) for n in LENGTHS]
    nc = pyin_ragged_frames(LENGTHS_NC, 512, 40, center=False)
    assert nc.tolist() == [88, 1, 1, 2, 0]
    assert nc.tolist() == [max(_oracle_frames(n, False), 0) for n in LENGTHS_NC]
    for center, lens, want in ((True, LENGTHS, got), (False, LENGTHS_NC, nc)):
        p, _ = pitch.pyin_params(4000, C5_SR, center=center, **C5)
        assert [lib.mm_pyin_num_frames(C.byref(p), n) for n in lens] == want.tolist()
    # an odd frame_length pads frame_length // 2 each side
    p, _ = pitch.pyin_params(4000, C5_SR, frame_length=513, hop_length=40, fmin=100, fmax=500)
    assert pyin_ragged_frames([1, 41, 700], 513, 40).tolist() == [lib.mm_pyin_num_frames(C.byref(p), n) for n in (1, 41, 700)]


def test_symbols_are_in_the_header_and_prototyped():
    lib = _lib.load()
    with open(HEADER) as f:
        header = f.read()
    for name, n_args in NEW.items():
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/modmfcc.h"
        assert len(m.group(1).split(",")) == n_args


def test_ragged_workspace_is_the_padded_batchs():
    lib = _lib.load()
    p, _ = pitch.pyin_params(4000, C5_SR, **C5)
    for rows, n in ((1, 4000), (9, 4000), (7, 100000), (3, 1)):
        want = lib.mm_pyin_workspace_bytes(C.byref(p), rows, n)
        assert want > 0 and lib.mm_pyin_ragged_workspace_bytes(C.byref(p), rows, n) == want
    assert lib.mm_pyin_ragged_workspace_bytes(None, 1, 4000) == 0
    assert lib.mm_pyin_ragged_workspace_bytes(C.byref(p), 0, 4000) == 0
    assert lib.mm_pyin_ragged_workspace_bytes(C.byref(p), 1, 0) == 0
    q, _ = pitch.pyin_params(4000, C5_SR, center=False, **C5)
    assert lib.mm_pyin_ragged_workspace_bytes(C.byref(q), 2, 511) == 0          # T_max == 0
    bad, _ = pitch.pyin_params(4000, C5_SR, **C5)
    bad.hop_length = 0
    assert lib.mm_pyin_ragged_workspace_bytes(C.byref(bad), 1, 4000) == 0


def test_c_entries_check_their_arguments_before_any_launch():
    lib = _lib.load()
    p, _ = pitch.pyin_params(4000, C5_SR, **C5)
    buf = np.zeros(64)                         # never dereferenced: every call below is refused first
    d = buf.ctypes.data
    t = _lib.mm_pyin_tables(*([d] * 7))
    for fn in (lib.mm_pyin_ragged_f32, lib.mm_pyin_ragged_f64):
        ok = [C.byref(p), C.byref(t), d, 2, 4000, 4000, d, d, d, d, d, None, d, 1 << 40, None]
        for i, v in ((6, None), (2, None), (7, None), (12, None), (1, None), (3, 0), (4, 0), (5, 3999)):
            a = list(ok)
            a[i] = v
            assert fn(*a) == _lib.MM_ERR_INVALID_ARG, (fn, i)
        a = list(ok)
        a[13] = 16                                             # workspace too small
        assert fn(*a) == _lib.MM_ERR_WORKSPACE
    f = lib.mm_interp_nan_linear_ragged_f64
    assert f(d, 1, 64, 64, None, d, 64, None) == _lib.MM_ERR_INVALID_ARG            # NULL d_counts
    assert f(None, 1, 64, 64, d, d, 64, None) == _lib.MM_ERR_INVALID_ARG
    assert f(d, 1, 64, 63, d, d, 64, None) == _lib.MM_ERR_INVALID_ARG
    g = lib.mm_interp_nan_ragged_f64
    assert g(0, d, 1, 64, 64, None, d, 64, d, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert g(7, d, 1, 64, 64, d, d, 64, d, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG    # unknown kind
    assert g(0, d, 1, 64, 64, d, d, 63, d, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert g(0, d, 1, 64, 64, d, d, 64, d, 8, None) == _lib.MM_ERR_WORKSPACE


def test_host_lengths_are_validated():
    got = check_lengths(LENGTHS, 9, 4000)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == LENGTHS
    for bad in ([0, 4000], [4001, 1], [-1, 5]):
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 4000\]"):
            check_lengths(bad, 2, 4000)
    with pytest.raises(ValueError):
        check_lengths([4000], 2, 4000)
    with pytest.raises(TypeError):
        check_lengths([4000.0, 1.0], 2, 4000)
    # the ragged calls refuse anything but a device batch before they look at the lengths
    with pytest.raises(TypeError):
        pitch.pyin_ragged_batch(np.zeros((2, 4000), np.float32), [4000, 1], C5_SR, **C5)
    with pytest.raises(TypeError):
        interp.interp_nan_ragged_batch(np.zeros((2, 40)), [40, 1])


def test_get_f0_batch_carries_get_f0s_keywords_and_refusals():
    one, many = inspect.signature(get_f0), inspect.signature(get_f0_batch)
    a, b = list(one.parameters.values()), list(many.parameters.values())
    assert b[0].name == "clips"
    assert [(p.name, p.kind, p.default) for p in a[1:]] == [(p.name, p.kind, p.default) for p in b[1:]]
    y = [np.zeros(100), np.zeros(50)]
    with pytest.raises(NotImplementedError):
        get_f0_batch(y, 16000)                                  # the default method is Praat's, as in get_f0
    with pytest.raises(NotImplementedError):
        get_f0_batch(y, 16000, method="praatcc")
    with pytest.raises(UnboundLocalError):
        get_f0_batch(y, 16000, method="yin")
    with pytest.raises(Exception, match="Cannot filter f0 signal with gaps"):
        get_f0_batch(y, 16000, method="pyin", interpUnvoiced=None)
    for name in ("pyin_ragged_batch", "pyin_ragged_frames", "interp_nan_ragged_batch", "get_f0_batch"):
        assert name in pitch.__all__
    assert "interp_nan_ragged_batch" in interp.__all__
    keys = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind == inspect.Parameter.KEYWORD_ONLY]
    assert keys(pitch.pyin_ragged_batch) == keys(pitch.pyin_batch)
