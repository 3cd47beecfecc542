"""GPU (-m gpu): the batched loader -- mm_pcm_decode_ragged_f32 under audio_io.load_wav_batch, load_audio_batch over it
and the ragged resamplers, and get_MFCCS_change_batch on a list of paths -- against the per-file calls (load_wav,
load_audio, get_MFCCS_change_batch on the loaded tensors): equality of the bit patterns everywhere.

The WAVE files are written here with struct: 16-bit mono and stereo, 24-bit mono, float32 stereo, 8-bit with three
channels, float64 mono (and 32-bit stereo); 1, 7, 8, 9, 1000 and 4097 frames (4097: two 2048-frame chunks of the decode
kernel's 16-byte path and one frame of its sample-by-sample path); 44100 and 16000 Hz.
"""
import struct

import numpy as np
import pytest

import resample_comb as RC

pytestmark = pytest.mark.gpu

CHANGE = dict(outFiltCutOff=[12])      # the defaults; outFiltCutOff has none that applyFilter takes ([None])

# (name, kind, bits, channels, frames, rate)
FILES = (
    ("s16m", "int", 16, 1, 4097, 44100),
    ("s16s", "int", 16, 2, 1000, 44100),
    ("s24m", "int", 24, 1, 9, 16000),
    ("f32s", "float", 32, 2, 8, 44100),
    ("u8x3", "int", 8, 3, 7, 16000),
    ("f64m", "float", 64, 1, 1, 44100),
    ("s16s_long", "int", 16, 2, 4097, 16000),
    ("f32s_long", "float", 32, 2, 4097, 44100),
    ("f32m_long", "float", 32, 1, 2049, 16000),
    ("s32s", "int", 32, 2, 33, 44100),
)


def _write_wav(path, kind, bits, channels, frames, rate, seed):
    rng = np.random.default_rng(seed)
    n = frames * channels
    if kind == "float":
        data = rng.uniform(-1.0, 1.0, n).astype("<f4" if bits == 32 else "<f8").tobytes()
    elif bits == 8:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    elif bits == 24:
        v = rng.integers(-(1 << 23), 1 << 23, n, dtype=np.int64)
        v[:2] = (-(1 << 23), (1 << 23) - 1)[:min(2, n)]
        data = b"".join(struct.pack("<i", int(q))[:3] for q in v)
    else:
        lo, hi = -(1 << (bits - 1)), 1 << (bits - 1)
        v = rng.integers(lo, hi, n, dtype=np.int64)
        v[:2] = (lo, hi - 1)[:min(2, n)]
        data = v.astype("<i2" if bits == 16 else "<i4").tobytes()
    align = channels * bits // 8
    fmt = struct.pack("<IHHIIHH", 16, 3 if kind == "float" else 1, channels, rate, rate * align, align, bits)
    body = b"WAVE" + b"fmt " + fmt + b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavs")
    paths = []
    for i, (name, kind, bits, ch, frames, rate) in enumerate(FILES):
        p = str(d / f"{name}.wav")
        _write_wav(p, kind, bits, ch, frames, rate, 100 + i)
        paths.append(p)
    return paths


def _same_bits(got, want, what):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(RC.bits(got) != RC.bits(want))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:8].tolist())


def _zero_bits(t, what):
    assert not RC.bits(t.cpu().numpy()).any(), what


def test_files_cover_the_issue(wavs):
    assert {(k, b, c) for _, k, b, c, _, _ in FILES} >= {("int", 16, 1), ("int", 16, 2), ("int", 24, 1), ("float", 32, 2),
                                                         ("int", 8, 3), ("float", 64, 1)}
    assert {f for *_, f, _ in FILES} >= {1, 7, 8, 9, 1000, 4097} and {r for *_, r in FILES} == {44100, 16000}


def test_load_wav_batch_equals_load_wav(wavs, gpu):
    from modulation_mfcc_amd import load_wav, load_wav_batch
    x, lengths, rates, first_row = load_wav_batch(wavs, gpu)
    ch = [c for _, _, _, c, _, _ in FILES]
    assert first_row.tolist() == np.concatenate([[0], np.cumsum(ch)]).tolist()
    assert x.shape == (sum(ch), 4097) and x.dtype.is_floating_point and x.device == gpu
    assert lengths.dtype == np.int64 and lengths.tolist() == [f for _, _, _, c, f, _ in FILES for _ in range(c)]
    assert rates.tolist() == [float(r) for _, _, _, c, _, r in FILES for _ in range(c)]
    for i, p in enumerate(wavs):
        one, sr = load_wav(p, gpu)
        r0, r1 = int(first_row[i]), int(first_row[i + 1])
        assert sr == rates[r0] and one.shape == (r1 - r0, lengths[r0])
        _same_bits(x[r0:r1, :one.shape[1]], one, FILES[i])
        _zero_bits(x[r0:r1, one.shape[1]:], (FILES[i], "not +0.0 behind the frames"))
    # any subset and order, a single file
    x1, l1, _, f1 = load_wav_batch([wavs[4]], gpu)
    assert x1.shape == (3, 7) and f1.tolist() == [0, 3] and l1.tolist() == [7, 7, 7]
    _same_bits(x1, load_wav(wavs[4], gpu)[0], "one file")


@pytest.mark.parametrize("sr", [16000, 22050])
def test_load_audio_batch_equals_load_audio(wavs, sr, gpu):
    """sr = 16000: the 44.1 kHz files go through one ragged resample, the 16 kHz files are copied; sr = 22050: two
    ragged resamples (two source rates).  Every row is load_audio of its file, bit for bit, zeros behind."""
    from modulation_mfcc_amd import load_audio, load_audio_batch
    x, lengths, first_row = load_audio_batch(wavs, sr, channel=None, device=gpu)
    assert x.shape[0] == first_row[-1] == len(lengths) and lengths.dtype == np.int64
    for i, p in enumerate(wavs):
        one = load_audio(p, sr, gpu)
        r0, r1 = int(first_row[i]), int(first_row[i + 1])
        assert one.shape[0] == r1 - r0 and (lengths[r0:r1] == one.shape[1]).all(), (FILES[i], lengths[r0:r1], one.shape)
        _same_bits(x[r0:r1, :one.shape[1]], one, (FILES[i], sr))
        _zero_bits(x[r0:r1, one.shape[1]:], (FILES[i], sr, "behind the row"))
    assert x.shape[1] == lengths.max()
    # one channel per file, picked as get_MFCCS_change picks channelN: a mono file gives its only channel
    for k in (0, 1, -1):
        xk, lk = load_audio_batch(wavs, sr, channel=k, device=gpu)
        assert xk.shape[0] == len(wavs) == len(lk)
        for i, p in enumerate(wavs):
            one = load_audio(p, sr, gpu)
            row = one[0] if one.shape[0] == 1 else one[k]
            assert lk[i] == row.shape[0]
            _same_bits(xk[i, :lk[i]], row, (FILES[i], sr, k))
    with pytest.raises(IndexError, match=r"\(file 1\)"):
        load_audio_batch(wavs, sr, channel=2, device=gpu)               # the first stereo file has no channel 2


def test_load_audio_batch_keeps_the_rates(wavs, gpu):
    from modulation_mfcc_amd import load_audio_batch, load_wav_batch
    x, lengths, rates, first_row = load_audio_batch(wavs, None, channel=None, device=gpu)
    x0, l0, r0, f0 = load_wav_batch(wavs, gpu)
    _same_bits(x, x0, "sr None")
    assert lengths.tolist() == l0.tolist() and rates.tolist() == r0.tolist() and first_row.tolist() == f0.tolist()
    # one source rate, already the target: the decoded rows as they are
    same = [p for p, f in zip(wavs, FILES) if f[5] == 16000]
    x, lengths = load_audio_batch(same, 16000, device=gpu)
    assert x.shape == (len(same), 4097) and lengths.tolist() == [f[4] for f in FILES if f[5] == 16000]


def test_change_curves_of_paths_equal_those_of_loaded_clips(wavs, gpu):
    """get_MFCCS_change_batch on paths (one decode, one resample) against the same call on the list of load_audio tensors
    (a load per file, pack_clips): the same ragged launches on a batch with identical valid parts -- equal exactly."""
    from modulation_mfcc_amd import get_MFCCS_change_batch, load_audio
    paths = [p for p, f in zip(wavs, FILES) if f[4] >= 1000]
    assert len(paths) == 5
    for sr, channelN in ((16000, 0), (16000, 1), (10000, 0)):
        got = get_MFCCS_change_batch(paths, sr, channelN=channelN, **CHANGE)
        clips = [load_audio(p, sr, gpu) for p in paths]
        clips = [c[0] if c.shape[0] == 1 else c for c in clips]         # as get_MFCCS_change loads a path: a mono file is [n]
        want = get_MFCCS_change_batch(clips, sr, channelN=channelN, **CHANGE)
        assert len(got) == len(want) == len(paths)
        for (c, t), (wc, wt) in zip(got, want):
            assert c.shape == wc.shape and len(c) > 21
            np.testing.assert_array_equal(c, wc)
            np.testing.assert_array_equal(t, wt)
    # a mixed list keeps the per-clip route
    mixed = get_MFCCS_change_batch([paths[0], load_audio(paths[1], 16000, gpu)], 16000, **CHANGE)   # (a stereo tensor)
    both = get_MFCCS_change_batch(paths[:2], 16000, **CHANGE)
    for (c, _), (wc, _) in zip(mixed, both):
        np.testing.assert_array_equal(c, wc)


def test_refusals_name_the_file(wavs, tmp_path, gpu):
    from modulation_mfcc_amd import get_MFCCS_change_batch, load_audio_batch, load_wav_batch
    empty = str(tmp_path / "empty.wav")
    _write_wav(empty, "int", 16, 2, 0, 16000, 1)
    adpcm = str(tmp_path / "adpcm.wav")
    with open(adpcm, "wb") as f:
        body = b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 2, 1, 8000, 4000, 1, 4) + b"data" + struct.pack("<I", 2) + b"\x01\x00"
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    for call in (lambda ps: load_wav_batch(ps, gpu), lambda ps: load_audio_batch(ps, 16000, device=gpu),
                 lambda ps: get_MFCCS_change_batch(ps, 16000, **CHANGE)):
        with pytest.raises(ValueError, match=r"no frames \(file 2\)"):
            call([wavs[0], wavs[1], empty])
        with pytest.raises(ValueError, match=r"unsupported WAVE encoding .*\(file 1\)"):
            call([wavs[0], adpcm, empty])
