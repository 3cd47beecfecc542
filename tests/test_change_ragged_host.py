"""CPU: the host side of the ragged MFCC-change tail -- the two C symbols, the checks of the C entry that need no plan,
validation of `frames`, the grouping helper and the signature of get_MFCCS_change_batch.
(A plan owns device tables and cannot be made without a GPU, so the checks behind a valid plan -- a bad diff_method, a short
workspace, MM_ERR_UNSUPPORTED for five sections and for a clip that does not fit LDS, the workspace query of a valid
shape -- run in tests/test_gpu_change_ragged.py::test_c_entry_checks_fire_before_any_launch, as those of mm_mfcc_ragged_f32
do in tests/test_gpu_ragged.py.)"""
import inspect

import numpy as np
import pytest
import scipy.signal
import torch

from modulation_mfcc_amd import _lib, get_MFCCS_change, get_MFCCS_change_batch
from modulation_mfcc_amd.plan import by_length, check_frames, sos_padlen

SOS = np.ascontiguousarray(scipy.signal.butter(6, 0.24, output="sos"))


def test_symbols_are_exported_and_prototyped():
    lib = _lib.load()
    for name in ("mm_change_ragged_workspace_bytes_for", "mm_mfcc_change_ragged_f64"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES["mm_mfcc_change_ragged_f64"][1]) == 15
    assert len(_lib.PROTOTYPES["mm_change_ragged_workspace_bytes_for"][1]) == 8
    assert lib.mm_version() == 123


def test_c_entry_rejects_a_null_plan_and_null_pointers():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)          # never dereferenced: the plan is checked before any pointer is used
    fr = np.ones(1, dtype=np.int64)
    p, s = buf.ctypes.data, SOS.ctypes.data
    f = lib.mm_mfcc_change_ragged_f64
    assert f(None, p, 1, 64, fr.ctypes.data, 1, 0, s, 3, s, 3, p, p, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert f(None, p, 1, 64, None, 1, 0, s, 3, s, 3, p, p, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG      # NULL d_frames
    assert f(None, None, 0, 0, None, 0, 0, None, 0, None, 0, None, None, 0, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_change_ragged_workspace_bytes_for(None, 4, 1001, 1, s, 3, s, 3) == 0


def test_padlen_is_scipys():
    for order in range(1, 9):
        sos = scipy.signal.butter(order, 0.24, output="sos")
        with pytest.raises(ValueError, match=f"padlen, which is {sos_padlen(sos)}\\."):
            scipy.signal.sosfiltfilt(sos, np.zeros(sos_padlen(sos)))
        scipy.signal.sosfiltfilt(sos, np.zeros(sos_padlen(sos) + 1))
    assert sos_padlen(SOS) == 21


def test_host_frames_are_validated():
    got = check_frames([22, 50, 76], 3, 76, 21)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [22, 50, 76]
    assert check_frames(torch.tensor([30, 40], dtype=torch.int32), 2, 40, 21).tolist() == [30, 40]
    assert check_frames(np.array([1, 2], dtype=np.uint8), 2, 2).tolist() == [1, 2]          # no filter: any length >= 1
    # scipy's own text for a clip sosfiltfilt refuses (T_b = padlen), with the first such clip named
    try:
        scipy.signal.sosfiltfilt(SOS, np.zeros(21))
    except ValueError as e:
        text = str(e)
    with pytest.raises(ValueError) as ei:
        check_frames([30, 21, 76, 5], 4, 76, 21)
    assert str(ei.value).startswith(text) and "clip 1 " in str(ei.value) and "21 frames" in str(ei.value)
    check_frames([30, 22, 76], 3, 76, 21)
    for bad in ([0, 50, 76], [22, 50, 77], [-3, 50, 76], [22, 50, 2 ** 40]):
        with pytest.raises(ValueError, match=r"frames must lie in \[1, 76\]"):
            check_frames(bad, 3, 76, 21)
    with pytest.raises(ValueError):
        check_frames([30, 40], 3, 76, 21)            # one per clip
    with pytest.raises(ValueError):
        check_frames(30, 1, 76, 21)
    for bad in ([30.0, 40.0], [True, True], ["30", "40"]):
        with pytest.raises(TypeError):
            check_frames(bad, 2, 76, 21)


def test_grouping_by_length():
    groups = by_length([30, 22, 30, 76, 22, 30])
    assert [T for T, _ in groups] == [22, 30, 76]
    assert [idx.tolist() for _, idx in groups] == [[1, 4], [0, 2, 5], [3]]
    assert all(idx.dtype == np.int64 for _, idx in groups)


def test_batch_signature_carries_the_reference_keywords():
    one, many = inspect.signature(get_MFCCS_change), inspect.signature(get_MFCCS_change_batch)
    a, b = list(one.parameters.values()), list(many.parameters.values())
    assert [p.kind for p in b[:2]] == [inspect.Parameter.POSITIONAL_ONLY] * 2 and b[1].name == "sigSr"
    assert [(p.name, p.kind, p.default) for p in a[2:]] == [(p.name, p.kind, p.default) for p in b[2:]]
    assert all(p.kind == inspect.Parameter.KEYWORD_ONLY for p in b[2:]) and len(b) == 18
    assert get_MFCCS_change_batch([], 10000) == []
