"""CPU: the host side of the ragged calls -- validation of `lengths`, pack_clips, and the C entry's checks that need no plan.
(A plan owns device tables, so the checks behind a valid plan -- batch < 1, a short workspace, the workspace query's
monotony -- run in tests/test_gpu_ragged.py.)"""
import numpy as np
import pytest
import torch

from modulation_mfcc_amd import _lib, pack_clips
from modulation_mfcc_amd.plan import check_lengths


def test_c_entry_rejects_a_null_plan_and_null_pointers():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)          # never dereferenced: the plan is checked first
    lens = np.ones(1, dtype=np.int64)
    p = buf.ctypes.data
    assert lib.mm_mfcc_ragged_f32(None, p, 1, 64, 64, lens.ctypes.data, p, None, p, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_mfcc_ragged_f32(None, None, 0, 0, 0, None, None, None, None, 0, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_ragged_workspace_bytes(None, 4, 16000) == 0


def test_host_lengths_are_validated():
    got = check_lengths([1, 5, 100], 3, 100)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [1, 5, 100]
    assert check_lengths(np.array([7, 8], dtype=np.uint8), 2, 8).dtype == np.int64
    assert check_lengths(torch.tensor([3, 4], dtype=torch.int32), 2, 4).tolist() == [3, 4]
    assert check_lengths((2,), 1, 2).tolist() == [2]
    for bad in ([0, 5, 100], [1, 5, 101], [-1, 5, 100], [1, 5, 2 ** 40]):
        with pytest.raises(ValueError):
            check_lengths(bad, 3, 100)
    with pytest.raises(ValueError):
        check_lengths([1, 2], 3, 100)               # one per clip
    with pytest.raises(ValueError):
        check_lengths([[1, 2, 3]], 3, 100)
    with pytest.raises(ValueError):
        check_lengths(5, 1, 100)                    # a scalar is not [1]
    for bad in ([1.0, 2.0, 3.0], [True, True, True], ["1", "2", "3"]):
        with pytest.raises(TypeError):
            check_lengths(bad, 3, 100)


def test_pack_clips_shapes_on_the_host():
    clips = [torch.arange(n, dtype=torch.float32) + 10 * i for i, n in enumerate((5, 1, 9, 3))]
    audio, lengths = pack_clips(clips)
    assert tuple(audio.shape) == (4, 9) and audio.dtype == torch.float32
    assert lengths.dtype == torch.int64 and lengths.device.type == "cpu" and lengths.tolist() == [5, 1, 9, 3]
    for b, c in enumerate(clips):
        assert torch.equal(audio[b, :c.shape[0]], c)
    assert check_lengths(lengths, 4, 9).tolist() == [5, 1, 9, 3]
    with pytest.raises(ValueError):
        pack_clips([])
    with pytest.raises(ValueError):
        pack_clips([torch.zeros(3), torch.zeros(0)])
    with pytest.raises(TypeError):
        pack_clips([torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(TypeError):
        pack_clips([torch.zeros(2, 3)])
    with pytest.raises(TypeError):
        pack_clips([np.zeros(3, dtype=np.float32)])
