"""CPU: modulation_mfcc_amd.ragged on its own -- the host rules of ragged batches that until now were only tested through
one caller each: the [rows, n_max] check and the row pitch, the two frame counts, the grouping, the refusals and the list
layer.  CPU tensors stand in for device ones where a function looks at nothing but shape, type and strides."""
import numpy as np
import pytest
import torch

from modulation_mfcc_amd import _lib, batch, calc, pitch, ragged
from modulation_mfcc_amd.plan import MfccConfig


@pytest.fixture
def cpu_rows(monkeypatch):
    """device_rows looks at the layout only: let a CPU tensor pass its device test."""
    monkeypatch.setattr(ragged, "is_device_tensor", lambda x: isinstance(x, torch.Tensor))


# every caller's parameters: (dtypes, type text, shape text, keywords)
CALLERS = {
    "filters": ((torch.float64, torch.float32), "x must be a float64 or float32 CUDA(HIP) tensor",
                "x must be [rows, n_max], at least one row and one column", {}),
    "hilbert": ((torch.float32, torch.float64), "x must be a float32 / float64 CUDA(HIP) tensor",
                "x must be [B, n_max], at least one row and one column", {}),
    "rms": ((torch.float32,), "audio must be a float32 CUDA(HIP) tensor", "audio must be [B, n_max]", dict(nonempty=False)),
    "pyin": ((torch.float32, torch.float64), "audio must be a CUDA(HIP) tensor [n] or [B, n]", "audio must be [n] or [B, n]",
             dict(widen=torch.float64, one_dim=True, nonempty=False)),
    "interp": ((torch.float64,), "interp_nan_ragged_batch takes a CUDA(HIP) tensor", "x must be [rows, n_max]",
               dict(widen=torch.float64, nonempty=False)),
}


def test_is_device_tensor():
    assert not ragged.is_device_tensor(torch.zeros(3)) and not ragged.is_device_tensor(np.zeros(3))
    assert not ragged.is_device_tensor([1, 2]) and not ragged.is_device_tensor(None)

    class Fake:
        __module__ = "torch.fake"
        is_cuda = True
    assert ragged.is_device_tensor(Fake())
    # a CPU tensor of counts is host data: validated, returned as numpy
    got = ragged.check_counts(torch.tensor([3, 4], dtype=torch.int32), 2, 4, None, "counts")
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [3, 4]


def test_row_pitch_and_copies(cpu_rows):
    dtypes, type_text, shape_text, kw = CALLERS["filters"]
    one = torch.zeros(100, dtype=torch.float64).as_strided((1, 100), (0, 1))             # a single row with stride 0: pitch n
    assert one.stride(0) == 0
    got = ragged.device_rows(one, dtypes, type_text, shape_text)
    assert got is one and ragged.row_pitch(got) == 100
    many = torch.arange(100, dtype=torch.float64).expand(3, 100)           # rows with stride 0 < n_max: copied
    got = ragged.device_rows(many, dtypes, type_text, shape_text)
    assert got is not many and got.stride() == (100, 1) and ragged.row_pitch(got) == 100 and torch.equal(got, many)
    overlap = torch.arange(200, dtype=torch.float64).as_strided((3, 100), (50, 1))      # 0 < stride < n_max: copied
    got = ragged.device_rows(overlap, dtypes, type_text, shape_text)
    assert got.stride() == (100, 1) and torch.equal(got, overlap)
    wide = torch.zeros((3, 177), dtype=torch.float32)[:, :100]             # a stride > n_max is kept as the view it is
    got = ragged.device_rows(wide, dtypes, type_text, shape_text)
    assert got is wide and ragged.row_pitch(got) == 177
    cols = torch.zeros((3, 200), dtype=torch.float32)[:, ::2]              # an inner stride: copied
    got = ragged.device_rows(cols, dtypes, type_text, shape_text)
    assert got.stride() == (100, 1)
    assert ragged.row_pitch(torch.zeros((1, 7))[:, :5]) == 5               # one row: n, whatever its stride says


@pytest.mark.parametrize("caller", list(CALLERS))
def test_each_callers_refusals(caller, cpu_rows):
    dtypes, type_text, shape_text, kw = CALLERS[caller]
    f = lambda x: ragged.device_rows(x, dtypes, type_text, shape_text, **kw)     # noqa: E731
    with pytest.raises(TypeError) as err:
        f(np.zeros((2, 10), dtype=np.float32))
    assert str(err.value) == type_text
    with pytest.raises(ValueError) as err:
        f(torch.zeros((2, 3, 4), dtype=dtypes[0]))
    assert str(err.value) == shape_text
    other = torch.zeros((2, 10), dtype=torch.int16)
    if "widen" in kw:                                                      # another type is converted, values intact
        other[1, 3] = -7
        got = f(other)
        assert got.dtype == torch.float64 and got[1, 3] == -7 and got.shape == (2, 10)
    else:
        with pytest.raises(TypeError) as err:
            f(other)
        assert str(err.value) == type_text
    row = torch.zeros(10, dtype=dtypes[0])
    if kw.get("one_dim"):
        assert f(row).shape == (1, 10)
    else:
        with pytest.raises(ValueError) as err:
            f(row)
        assert str(err.value) == shape_text
    empty = torch.zeros((0, 10), dtype=dtypes[0])
    if kw.get("nonempty", True):
        with pytest.raises(ValueError) as err:
            f(empty)
        assert str(err.value) == shape_text
    else:
        assert f(empty).shape == (0, 10)


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("frame,hop", [(400, 160), (513, 40), (7, 3)])
def test_centered_frames(frame, hop, center):
    lib = _lib.load()
    lens = [1, frame - 1, frame, frame + hop - 1, frame + hop]
    got = ragged.centered_frames(np.array(lens), frame, hop, center)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    t = torch.tensor(lens, dtype=torch.int64)
    same = ragged.centered_frames(t, frame, hop, center)                   # the CPU tensor stands in for the device one
    assert isinstance(same, torch.Tensor) and same.dtype == torch.int64 and same.tolist() == got.tolist()
    assert t.tolist() == lens                                              # the argument is not written to
    assert ragged.centered_frames(lens, frame, hop, center).tolist() == got.tolist()       # a list is host data
    for n, g in zip(lens, got):
        want = lib.mm_rms_num_frames(n, frame, hop, 1 if center else 0)
        assert g == max(want, 0), (n, g, want)                             # 0 where the library refuses
    assert ragged.centered_frames([0, -3], frame, hop, center).tolist() == [0, 0]
    assert batch.rms_ragged_frames is ragged.centered_frames and pitch.pyin_ragged_frames is ragged.centered_frames


@pytest.mark.parametrize("n_fft", [512, 400, 401])
def test_stft_frames(n_fft):
    hop = 160
    cfg = MfccConfig(sr=16000.0, n_fft=n_fft, win_length=n_fft, hop_length=hop, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
    lens = [1, hop - 1, hop, 3 * hop + 1]
    want = [cfg.num_frames(n) for n in lens]
    got = ragged.stft_frames(np.array(lens), n_fft, hop)
    assert got.dtype == np.int64 and got.tolist() == want
    t = torch.tensor(lens, dtype=torch.int64)
    assert ragged.stft_frames(t, n_fft, hop).tolist() == want and t.tolist() == lens


def test_group_rows():
    groups = ragged.group_rows([30, 22, 30, 76, 22, 30])
    assert [(T, idx.tolist()) for T, idx in groups] == [(22, [1, 4]), (30, [0, 2, 5]), (76, [3])]
    assert all(idx.dtype == np.int64 for _, idx in groups)
    got = ragged.group_rows([calc.hilbert_ragged_fft_size(n) for n in (9, 1, 4097, 8, 16, 4096)])
    assert [(M, idx.tolist()) for M, idx in got] == [(16, [1, 3]), (32, [0, 4]), (8192, [5]), (16384, [2])]


def test_refuse_short():
    lens = np.array([400, 21, 22, 5], dtype=np.int64)
    text = ragged.PADLEN_TEXT.format(21)
    with pytest.raises(ragged.RowRefused) as err:
        ragged.refuse_short(lens, 400, 22, text)
    assert str(err.value) == text + " (row 1 has 21 samples)" and (err.value.base, err.value.row, err.value.n) == (text, 1, 21)
    with pytest.raises(ValueError) as err:
        ragged.refuse_short(lens, 400, 22, text, "clip", "frames")
    assert str(err.value) == text + " (clip 1 has 21 frames)" and type(err.value) is ValueError
    with pytest.raises(ValueError) as err:
        ragged.refuse_short(lens, 400, 22, lambda n: f"a clip of {n} samples", "clip", None)
    assert str(err.value) == "a clip of 21 samples (clip 1)" and type(err.value) is ValueError
    ragged.refuse_short(lens, 400, 5, text)
    # counts that are not on the host (None stands in for a device tensor): only n_max is looked at
    ragged.refuse_short(None, 22, 22, text)
    with pytest.raises(ValueError) as err:
        ragged.refuse_short(None, 21, 22, text)
    assert str(err.value) == text and type(err.value) is ValueError


def test_split_pack_and_pack_clips():
    clips = [torch.arange(5, dtype=torch.float32), torch.arange(3, dtype=torch.float64),
             torch.tensor([-300, 7, 20000], dtype=torch.int16), torch.arange(5, dtype=torch.float32) + 10]
    f32, others = ragged.split_by_dtype(clips)
    assert f32 == [0, 3] and others == [1, 2]                              # the int16 clip goes with the float64 ones
    assert ragged.split_by_dtype([None, clips[1]]) == ([], [1])
    x, lengths = ragged.pack([clips[i] for i in others], torch.float64)
    assert x.dtype == torch.float64 and x.shape == (2, 3) and isinstance(lengths, np.ndarray) and lengths.dtype == np.int64
    assert lengths.tolist() == [3, 3] and x[1].tolist() == [-300.0, 7.0, 20000.0]          # converted on the copy, values intact
    groups = list(ragged.packed_groups(clips))
    assert [(idx, tuple(x.shape), x.dtype, lens.tolist()) for idx, x, lens in groups] == \
        [([0, 3], (2, 5), torch.float32, [5, 5]), ([1, 2], (2, 3), torch.float64, [3, 3])]
    assert [idx for idx, _, _ in ragged.packed_groups(clips[:1])] == [[0]]
    with pytest.raises(TypeError, match="pack_clips: every clip must be a 1-D float64 tensor"):
        batch.pack_clips([clips[1], clips[2]], torch.float64)              # pack_clips still refuses it
    audio, lens = batch.pack_clips([clips[0], clips[3][:2]])
    assert isinstance(lens, torch.Tensor) and lens.dtype == torch.int64 and lens.tolist() == [5, 2] and audio.shape == (2, 5)


def test_named_and_blame_clip():
    try:
        raise IndexError("index 0 is out of bounds")
    except IndexError as e:
        err = ragged.named(e, 4)
        assert type(err) is IndexError and str(err) == "index 0 is out of bounds (clip 4)" and err.__cause__ is e
        assert str(ragged.named(e, 2, "curve")) == "index 0 is out of bounds (curve 2)"
    fresh = ragged.named(TypeError("x must be float"), 1)
    assert type(fresh) is TypeError and str(fresh) == "x must be float (clip 1)" and fresh.__cause__ is None
    refused = ragged.RowRefused("scipy's text.", 2, 19)
    err = ragged.named(refused, 7)
    assert type(err) is ValueError and str(err) == "scipy's text. (clip 7)"

    def one(b):
        if b == 1:
            raise ValueError("too short")
    with pytest.raises(ValueError) as got:
        ragged.blame_clip(ValueError("the batch's"), one, [5, 8, 9])
    assert str(got.value) == "too short (clip 8)" and str(got.value.__cause__) == "too short"
    batch_error = ValueError("the batch's")
    with pytest.raises(ValueError) as got:
        ragged.blame_clip(batch_error, lambda b: None, [5, 8, 9])          # no clip alone reproduces it: unchanged
    assert got.value is batch_error
