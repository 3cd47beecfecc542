"""CPU: the host arithmetic of the batched loader -- audio_io.plan_wav_batch (where each file's bytes and rows go), the
output lengths of resample_ragged_batch -- and the yardstick of the ragged resamplers' GPU file (tests/ragged_comb.py:
the exact answer to a PREFIX of the edge comb) against the NumPy statement of the banded operator.  No GPU is used."""
import numpy as np
import pytest

import ragged_comb as RG
import resample_comb as RC
from modulation_mfcc_amd import audio_io

BPS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 8}


def _hdr(fmt, channels, n_frames, sr=44100.0):
    kind, bits = {v: k for k, v in audio_io._FMT.items()}[fmt] if fmt in BPS else ("int", 12)
    return dict(sr=float(sr), channels=channels, bits=bits, kind=kind, fmt=fmt, data_offset=44,
                data_bytes=n_frames * channels * BPS.get(fmt, 0), n_frames=n_frames)


MIX = [(2, 1, 4097), (2, 2, 1000), (3, 1, 9), (5, 2, 8), (1, 3, 7), (6, 1, 1), (4, 2, 33), (3, 3, 5), (2, 1, 8)]


def test_plan_offsets_rows_and_table():
    pl = audio_io.plan_wav_batch([_hdr(*m) for m in MIX])
    B = len(MIX)
    off, nb = pl["offsets"], pl["nbytes"]
    assert off.dtype == np.int64 and off.shape == (B,) and off[0] == 0
    assert (off % 16 == 0).all()
    np.testing.assert_array_equal(nb, [n * c * BPS[f] for f, c, n in MIX])
    assert (off[1:] >= off[:-1] + nb[:-1]).all()                      # byte ranges in file order, none overlapping
    assert (off[1:] - (off[:-1] + nb[:-1]) < 16).all()                # ... and no more than the alignment between them
    assert pl["total_bytes"] >= off[-1] + nb[-1] and pl["total_bytes"] % 16 == 0
    # rows: every channel of every file, in file and channel order
    ch = np.array([c for _, c, _ in MIX])
    np.testing.assert_array_equal(pl["first_row"], np.concatenate([[0], np.cumsum(ch)]))
    np.testing.assert_array_equal(pl["row_file"], np.repeat(np.arange(B), ch))
    np.testing.assert_array_equal(pl["row_channel"], np.concatenate([np.arange(c) for c in ch]))
    np.testing.assert_array_equal(pl["frames"], [n for _, _, n in MIX])
    assert pl["n_max"] == 4097
    # the device table: one 32-byte record per file, the fields of mm_wav_rec in its order
    tab = pl["table"]
    assert tab.dtype == audio_io.WAV_REC and tab.dtype.itemsize == 32 and tab.shape == (B,)
    assert [tab.dtype.fields[k][1] for k in ("byte_offset", "n_frames", "fmt", "channels", "first_row")] == [0, 8, 16, 20, 24]
    np.testing.assert_array_equal(tab["byte_offset"], off)
    np.testing.assert_array_equal(tab["n_frames"], pl["frames"])
    np.testing.assert_array_equal(tab["fmt"], [f for f, _, _ in MIX])
    np.testing.assert_array_equal(tab["channels"], ch)
    np.testing.assert_array_equal(tab["first_row"], pl["first_row"][:-1])


def test_plan_of_one_file():
    pl = audio_io.plan_wav_batch([_hdr(2, 2, 5)])
    assert pl["total_bytes"] == 32 and list(pl["first_row"]) == [0, 2] and pl["n_max"] == 5


def test_plan_refusals_name_the_file():
    good = _hdr(2, 1, 10)
    with pytest.raises(ValueError, match=r"holds no frames \(file 2\)"):
        audio_io.plan_wav_batch([good, good, _hdr(2, 2, 0), _hdr(2, 1, 0)])
    with pytest.raises(ValueError, match=r"unsupported WAVE encoding .*\(file 1\)"):
        audio_io.plan_wav_batch([good, _hdr(7, 1, 10)])
    with pytest.raises(ValueError, match=r"unsupported WAVE encoding .*\(file 0\)"):
        audio_io.plan_wav_batch([_hdr(2, 0, 10)])
    with pytest.raises(ValueError, match="no files"):
        audio_io.plan_wav_batch([])


def test_read_wav_header_refusal_is_named_by_the_batch_loader(tmp_path):
    """load_wav_batch parses every header before it asks for the device: a file with an encoding read_wav_header refuses
    raises its error with the file's index, with or without a GPU."""
    import struct
    ok = tmp_path / "ok.wav"
    ok.write_bytes(b"RIFF" + struct.pack("<I", 38) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 8000, 16000, 2, 16) +
                   b"data" + struct.pack("<I", 2) + b"\x01\x00")
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFF" + struct.pack("<I", 38) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 2, 1, 8000, 4000, 1, 4) +
                    b"data" + struct.pack("<I", 2) + b"\x01\x00")          # format tag 2: ADPCM
    assert audio_io.read_wav_header(str(ok))["n_frames"] == 1
    with pytest.raises(ValueError, match=r"unsupported WAVE encoding \(format tag 2, 4 bits\) \(file 1\)"):
        audio_io.load_wav_batch([str(ok), str(bad)])


@pytest.mark.parametrize("pair", RG.PAIRS + ((48000, 250),), ids=RC.ratio_id)
def test_out_lengths_arithmetic(pair):
    """resample_out_lengths == -(-n L // M) in Python integers for n = 1 .. 2000 and around the n at which n L passes
    2^31 and 2^32 (int64 arithmetic: no wrap), on numpy arrays and on int64 tensors."""
    import torch
    L, M = audio_io.resample_ratio(*pair)
    ns = list(range(1, 2001))
    for edge in (1 << 31, 1 << 32, 1 << 40):
        ns += [edge // L + d for d in (-2, -1, 0, 1, 2, 3)]
    want = [-(-n * L // M) for n in ns]
    assert max(n * L for n in ns) > 1 << 31
    arr = np.array(ns, dtype=np.int64)
    got = audio_io.resample_out_lengths(arr, L, M)
    assert got.dtype == np.int64 and got.tolist() == want
    assert arr.tolist() == ns                                          # the argument is left as it was
    t = torch.from_numpy(arr)
    got_t = audio_io.resample_out_lengths(t, L, M)
    assert got_t.dtype == torch.int64 and got_t.tolist() == want and t.tolist() == ns


@pytest.mark.parametrize("pair", RG.PAIRS, ids=RC.ratio_id)
def test_extended_comb_is_the_edge_comb(pair):
    x, want, _ = RC.comb(*pair, True)
    np.testing.assert_array_equal(RC.bits(RG.edge_comb(pair, len(x))), RC.bits(x))
    np.testing.assert_array_equal(RC.bits(RG.prefix_want(pair, len(x))), RC.bits(want))


@pytest.mark.parametrize("pair", RG.PAIRS, ids=RC.ratio_id)
def test_row_lengths_cover_the_cases(pair):
    t = RC.tables(*pair)
    F = t["tabs"]["F"]
    ns, n_max, tile = RG.row_lengths(pair)
    outs = {RG.out_len(pair, n) for n in ns}
    assert ns[0] == 1 and ns[-1] == n_max and len(set(ns.tolist())) == len(ns)
    assert RG.out_len(pair, n_max) >= 3 * tile and RG.out_len(pair, ns[0]) + tile <= RG.out_len(pair, n_max)  # whole tiles empty
    if t["L"] <= t["M"]:                                               # every output count is reachable
        assert {1, 2, 3, F - 3, F, tile - 1, tile, tile + 1} <= outs
    else:                                                              # 3 / 1: multiples of 3 only
        assert {3, F - 3, F, tile, tile + 3} <= outs
    x = RG.edge_comb(pair, n_max)
    assert any(n < n_max and x[n] != 0 for n in ns), "no row is cut at an impulse"


@pytest.mark.parametrize("pair", RG.PAIRS, ids=RC.ratio_id)
def test_prefix_yardstick_agrees_with_the_banded_operator(pair):
    """For a few prefixes of the edge comb, the impulse-response yardstick equals audio_io.banded_resample_numpy of the
    prefix alone: every output holds at most one non-zero product, so the float64 operator is exact too."""
    t = RC.tables(*pair)
    ns, n_max, tile = RG.row_lengths(pair)
    x = RG.edge_comb(pair, n_max)
    W = RG.spacing(pair)
    some = [n for n in ns if n <= 4 * W + 2][:12] + [int(ns[len(ns) // 2])]
    assert any(x[n] != 0 for n in some if n < n_max)
    for n_b in some:
        n_out_b = RG.out_len(pair, n_b)
        want = RG.prefix_want(pair, n_b)
        got = audio_io.banded_resample_numpy(x[:n_b], t["tabs"], n_out_b)
        assert want.shape == got.shape == (n_out_b,)
        np.testing.assert_array_equal(got.astype(np.float32), want, err_msg=f"{pair} n_b {n_b}")
        assert not np.signbit(want).any() or (want[np.signbit(want)] != 0).all()       # no -0.0 in the yardstick
