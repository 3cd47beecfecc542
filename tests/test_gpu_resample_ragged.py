"""GPU (-m gpu): both sample-rate converters with a length per row -- mm_resample_banded_ragged_f32 (matrix pipe,
resample_mfma_kernel<PAD, VEC, true>) and mm_resample_ragged_f32 (resample_kernel<true>, float64 accumulation) -- and
audio_io.resample_ragged_batch over them.  Ratios of resample_comb.MATRIX: 48000 -> 16000 (QT 8, pad, NB 1), 44100 ->
16000 (QT 2), 16000 -> 48000 (upsampling, F % 16 = 14), 16000 -> 11025 (QT 1, pad, NB 28).

A  tap by tap          rows = prefixes of the edge comb (tests/ragged_comb.py; test_audio_batch_host.py checks the
                       yardstick on the CPU): n_out_b = 1, 2, 3, below F, F, a tile of 16 QT F outputs -1 / +0 / +1,
                       rows cut at an impulse, three tiles; behind a row the rest of the comb or NaN; aligned rows and
                       rows one float off at an odd pitch; device lengths (with 0, a negative value and n_max + 5,
                       which the kernels clamp) and host lengths: equality of the bit patterns, +0.0 behind every row
B  the single call     noise rows of 1, 300 and 20000 samples equal resample_batch of each row alone bit for bit; the
                       suite's 2e-6 of the maximum against scipy for the longest
C  guard bands         NaN sentinels before and behind the output and between its rows (y_stride > n_out_max)
D  items > workgroups  4 CUs + 76 rows of 64 samples with a length each; and rows of four tiles of which most are empty,
                       more items than resident workgroups: a workgroup stages again after an empty item
E  the fall-back       48000 -> 250: 'auto' is 'f64' bit for bit, 'mfma' raises, the banded entry refuses and writes nothing

The only tolerance in this file is B's 2e-6 (tests/test_gpu_resample.py: TOL); everything else is equality.
"""
import ctypes as C

import numpy as np
import pytest

import ragged_comb as RG
import resample_comb as RC
from modulation_mfcc_amd import _lib

pytestmark = pytest.mark.gpu

IDS = [RC.ratio_id(p) for p in RG.PAIRS]
TOL = 2e-6
GUARD = 32
METHODS = ["mfma", "f64"]


def _torch():
    import torch
    return torch


def _stream(gpu):
    return C.c_void_p(_torch().cuda.current_stream(gpu).cuda_stream)


def _rows_view(x2, aligned, gpu):
    """Host rows [rows, n] -> (holder, view [rows, n] on the device): `aligned` rows start on 16 bytes with a pitch that is
    a multiple of 4 (the VEC instantiations), otherwise one float off with an odd pitch.  NaN before, between and behind."""
    torch = _torch()
    rows, n = x2.shape
    pitch, off = ((n + 3) // 4 * 4 + 4, 0) if aligned else (n + 1 + n % 2, 1)
    buf = torch.full((off + rows * pitch + 8,), float("nan"), dtype=torch.float32, device=gpu)
    view = buf[off:off + rows * pitch].view(rows, pitch)[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x2, dtype=np.float32)).to(gpu))
    assert (view.data_ptr() % 16 == 0 and pitch % 4 == 0) == aligned and (aligned or pitch % 2 == 1)
    return buf, view


def _launch(method, pair, gpu, x_ptr, rows, n_max, pitch, d_lens, y_ptr, n_out_max, y_stride):
    """One call of mm_resample_banded_ragged_f32 ('mfma') or mm_resample_ragged_f32 ('f64') -> status."""
    from modulation_mfcc_amd import audio_io
    torch = _torch()
    lib = _lib.load()
    t = RC.tables(*pair)
    L, M = t["L"], t["M"]
    assert d_lens.dtype == torch.int64 and d_lens.is_cuda and d_lens.shape == (rows,)
    with torch.cuda.device(gpu):
        if method == "mfma":
            tb = audio_io._device_banded(L, M, gpu)
            return lib.mm_resample_banded_ragged_f32(x_ptr, rows, n_max, pitch, d_lens.data_ptr(), tb["d_atab"].data_ptr(),
                                                     tb["d_lo_off"].data_ptr(), tb["F"], tb["S"], tb["NB"], tb["ksteps"],
                                                     tb["lo_min"], tb["win"], y_ptr, n_out_max, y_stride, _stream(gpu))
        taps, tpp, half = audio_io._device_taps(L, M, gpu)
        return lib.mm_resample_ragged_f32(x_ptr, rows, n_max, pitch, d_lens.data_ptr(), taps.data_ptr(), L, M, tpp, half,
                                          y_ptr, n_out_max, y_stride, _stream(gpu))


def _same_bits(got, want, what):
    bad = np.argwhere(RC.bits(got) != RC.bits(want))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:8].tolist(), [float(got[tuple(i)]) for i in bad[:8]],
                               [float(want[tuple(i)]) for i in bad[:8]])


# ---- A: tap by tap ------------------------------------------------------------------------------------------------
_A = {}


def _case_a(pair):
    """(lengths as the kernels must take them [rows], the device lengths' raw values [rows], x rows [rows, n_max] with the
    comb behind every row, want [rows, n_out_max]) -- computed once per ratio, shared and read-only."""
    if pair not in _A:
        ns, n_max, _ = RG.row_lengths(pair)
        # three more rows whose DEVICE lengths are 0, negative and n_max + 5: clamped to 1, 1 and n_max
        eff = np.concatenate([ns, [1, 1, n_max]]).astype(np.int64)
        raw = np.concatenate([ns, [0, -7, n_max + 5]]).astype(np.int64)
        n_out_max = RG.out_len(pair, n_max)
        x = np.tile(RG.edge_comb(pair, n_max), (len(eff), 1))
        want = np.stack([RG.prefix_want(pair, n, n_out_max) for n in eff])
        for a in (eff, raw, x, want):
            a.setflags(write=False)
        _A[pair] = (eff, raw, x, want)
    return _A[pair]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("behind", ["comb", "nan"])
@pytest.mark.parametrize("pair", RG.PAIRS, ids=IDS)
def test_every_row_is_its_prefix_alone(pair, behind, method, gpu):
    """Row b of the output is a h[m M + half - p L] over the impulses at p < n_b for m < n_out_b and +0.0 from there to
    n_out_max, bit for bit (the output starts as NaN).  Behind n_b the input holds the rest of the comb -- rows are cut
    AT an impulse, and everywhere the next impulse is closer than the filter is long: reading it changes exact outputs
    -- or NaN, which reading turns into NaN.  Short rows leave the second and third tile of the launch wholly empty."""
    from modulation_mfcc_amd import resample_ragged_batch
    torch = _torch()
    eff, raw, x, want = _case_a(pair)
    rows, n_max = x.shape
    n_out_max = want.shape[1]
    xin = np.array(x)
    if behind == "nan":
        xin[np.arange(n_max)[None, :] >= eff[:, None]] = np.nan
    d_raw = torch.from_numpy(np.array(raw)).to(gpu)
    for aligned in (True, False):
        hold, view = _rows_view(xin, aligned, gpu)
        out = torch.full((rows, n_out_max), float("nan"), dtype=torch.float32, device=gpu)
        rc = _launch(method, pair, gpu, view.data_ptr(), rows, n_max, view.stride(0), d_raw, out.data_ptr(), n_out_max, n_out_max)
        assert rc == _lib.MM_OK
        _same_bits(out.cpu().numpy(), want, (pair, method, behind, f"VEC {int(aligned)}", "device lengths"))
        # the Python layer: device lengths (no read-back: out_lengths is a tensor of the clamped values' counts) ...
        y, ol = resample_ragged_batch(view, d_raw, *pair, method=method)
        assert torch.is_tensor(ol) and ol.is_cuda and ol.dtype == torch.int64
        assert ol.cpu().tolist() == [RG.out_len(pair, n) for n in eff]
        _same_bits(y.cpu().numpy(), want, (pair, method, behind, f"VEC {int(aligned)}", "resample_ragged_batch, device lengths"))
        # ... and host lengths without the longest rows: the call is cut to the longest row it has
        k = rows - 4                                    # the ascending rows but the longest: all shorter than n_max
        cut = int(eff[:k].max())
        assert cut == eff[k - 1] < n_max == eff[k]
        y, ol = resample_ragged_batch(view[:k], np.array(eff[:k]), *pair, method=method)
        assert isinstance(ol, np.ndarray) and ol.dtype == np.int64 and ol.tolist() == [RG.out_len(pair, n) for n in eff[:k]]
        assert y.shape == (k, RG.out_len(pair, cut))
        _same_bits(y.cpu().numpy(), want[:k, :y.shape[1]], (pair, method, behind, f"VEC {int(aligned)}", "host lengths"))
        assert not want[:k, y.shape[1]:].any()
        del hold


def test_host_lengths_are_validated(gpu):
    from modulation_mfcc_amd import resample_ragged_batch
    torch = _torch()
    x = torch.zeros((3, 50), dtype=torch.float32, device=gpu)
    for bad in ([1, 0, 5], [1, 2, 51], [1, 2], [1.0, 2.0, 3.0]):
        with pytest.raises((ValueError, TypeError)):
            resample_ragged_batch(x, bad, 48000, 16000)
    with pytest.raises(TypeError):
        resample_ragged_batch(x.double(), [1, 2, 3], 48000, 16000)
    with pytest.raises(TypeError):
        resample_ragged_batch(x, torch.tensor([1, 2, 3], dtype=torch.int32, device=gpu), 48000, 16000)
    with pytest.raises(ValueError, match="method"):
        resample_ragged_batch(x, [1, 2, 3], 48000, 16000, method="soxr")
    # equal rates: the valid parts, zeros behind them, NaN padding not carried over
    x[:] = float("nan")
    x[0, :1], x[1, :20], x[2, :50] = 1.0, 2.0, 3.0
    y, ol = resample_ragged_batch(x, [1, 20, 50], 16000, 16000)
    want = np.zeros((3, 50), dtype=np.float32)
    want[0, :1], want[1, :20], want[2, :50] = 1.0, 2.0, 3.0
    _same_bits(y.cpu().numpy(), want, "L == M")
    assert ol.tolist() == [1, 20, 50]


# ---- B: equals the single call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RG.PAIRS, ids=IDS)
def test_rows_equal_the_single_call(pair, gpu):
    import scipy.signal
    from modulation_mfcc_amd import resample_batch, resample_ragged_batch
    torch = _torch()
    t = RC.tables(*pair)
    lens = np.array([1, 300, 20000], dtype=np.int64)
    x = np.random.default_rng(23).standard_normal((3, 20000)).astype(np.float32)
    d = torch.from_numpy(x).to(gpu)
    want = scipy.signal.resample_poly(x[2].astype(np.float64), t["L"], t["M"], window=t["h32"].astype(np.float64) / t["L"])
    for method in METHODS:
        for lengths in (lens, torch.from_numpy(lens).to(gpu)):
            y, ol = resample_ragged_batch(d, lengths, *pair, method=method)
            y = y.cpu().numpy()
            assert y.shape == (3, RG.out_len(pair, 20000)) and [int(v) for v in ol] == [RG.out_len(pair, n) for n in lens]
            for b, n in enumerate(lens):
                one = resample_batch(d[b, :n], *pair, method=method).cpu().numpy()
                _same_bits(y[b, :len(one)], one, (pair, method, int(n)))
                assert not RC.bits(y[b, len(one):]).any(), (pair, method, int(n), "not +0.0 behind the row")
            err = np.abs(y[2] - want).max() / np.abs(want).max()
            print(f"B {RC.ratio_id(pair)} {method}: {err:.2e}")
            assert err <= TOL, (pair, method, err)


# ---- C: guard bands -----------------------------------------------------------------------------------------------
_GUARD_N = {
    (48000, 16000): (1, 4, 7, 10, 1000, 6155),
    (44100, 16000): (3, 300, 1000, 1003, 1006, 1009),
    (16000, 48000): (1, 2, 3, 4, 43, 1001),
    (16000, 11025): (2, 5, 10, 100, 641, 20001),
}


@pytest.mark.parametrize("pair", RG.PAIRS, ids=IDS)
def test_nothing_is_written_outside_the_rows(pair, gpu):
    """Three rows of lengths n_max, 1 and about n_max / 2 into an output whose rows are y_stride = n_out_max + 3 (and + 0)
    apart, NaN sentinels before, between and behind them, NaN behind every input row: the sentinels survive, the body is
    finite, +0.0 behind every row's own outputs."""
    torch = _torch()
    t = RC.tables(*pair)
    L, M = t["L"], t["M"]
    n_outs = [-(-n * L // M) for n in _GUARD_N[pair]]
    assert {v % 4 for v in n_outs} == {0, 1, 2, 3}
    rng = np.random.default_rng(5)
    for n_max, n_out_max in zip(_GUARD_N[pair], n_outs):
        lens = np.array([n_max, 1, max(1, n_max // 2)], dtype=np.int64)
        x = rng.standard_normal((3, n_max)).astype(np.float32)
        x[np.arange(n_max)[None, :] >= lens[:, None]] = np.nan
        d_lens = torch.from_numpy(lens).to(gpu)
        for method in METHODS:
            for gap in (3, 0):
                ys = n_out_max + gap
                xin = torch.from_numpy(x).to(gpu)
                u = (np.uint32(0x7FC00000) | (np.arange(3 * ys + 2 * GUARD, dtype=np.uint32) & np.uint32(0xFFFFF)))
                out = torch.from_numpy(u.view(np.float32).copy()).to(gpu)
                rc = _launch(method, pair, gpu, xin.data_ptr(), 3, n_max, n_max, d_lens, out.data_ptr() + 4 * GUARD, n_out_max, ys)
                assert rc == _lib.MM_OK
                got = out.cpu().numpy().view(np.uint32)
                what = (pair, n_max, method, gap)
                np.testing.assert_array_equal(got[:GUARD], u[:GUARD], err_msg=f"front sentinel {what}")
                np.testing.assert_array_equal(got[GUARD + 3 * ys - gap:], u[GUARD + 3 * ys - gap:], err_msg=f"back sentinel {what}")
                body = got[GUARD:GUARD + 3 * ys].reshape(3, ys)
                np.testing.assert_array_equal(body[:, n_out_max:], u[GUARD:GUARD + 3 * ys].reshape(3, ys)[:, n_out_max:],
                                              err_msg=f"sentinel between rows {what}")
                assert np.isfinite(body[:, :n_out_max].view(np.float32)).all(), what
                for b, n in enumerate(lens):
                    assert not body[b, -(-int(n) * L // M):n_out_max].any(), (what, b)


# ---- D: more items than workgroups --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pair", [(8000, 16000), (44100, 16000)], ids=["8000to16000", "44100to16000"])
def test_more_rows_than_resident_workgroups(pair, method, gpu):
    """rows = 4 CUs + 76 of 64 samples, one LDS tile per row, a length in 1 .. 64 and one impulse per row (before or behind
    the row's end): workgroups come round to a second and third item with another length."""
    from modulation_mfcc_amd import resample_ragged_batch
    torch = _torch()
    t = RC.tables(*pair)
    L, M, n = t["L"], t["M"], 64
    n_out = -(-n * L // M)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rows = 4 * cus + 76
    lens = 1 + (np.arange(rows, dtype=np.int64) * 37) % 64
    assert set(lens.tolist()) == set(range(1, 65))
    x = np.zeros((rows, n), dtype=np.float32)
    want = np.zeros((rows, n_out), dtype=np.float32)
    for r in range(rows):
        p, a = (r * 11) % 64, RC.amplitude(r)
        x[r, p] = a
        if p < lens[r]:
            n_out_r = -(-int(lens[r]) * L // M)
            RC.response(want[r, :n_out_r], np.full(n_out_r, -1, dtype=np.int64), t["h32"], L, M, t["half"], p, a)
    want[want == 0] = 0.0
    assert ((np.arange(rows) * 11) % 64 >= lens).sum() > rows // 8           # impulses behind their row's end
    for lengths in (lens, torch.from_numpy(lens).to(gpu)):
        got = resample_ragged_batch(torch.from_numpy(x).to(gpu), lengths, *pair, method=method)[0].cpu().numpy()
        assert got.shape == want.shape and np.count_nonzero(want) > rows // 2
        _same_bits(got, want, (pair, method))


@pytest.mark.parametrize("method", METHODS)
def test_staging_again_after_empty_items(method, gpu):
    """48000 -> 16000, rows of four tiles (2048 outputs each), CUs + 19 rows: more (row, tile) items than the 4 workgroups
    per CU of the launch, and with lengths spread over 1 .. n_max about half of the items are empty -- a workgroup that
    met an empty item (no barrier, no staging) stages its next tile into the LDS the last one used.  One impulse per
    tile and row, before or behind the row's end."""
    from modulation_mfcc_amd import resample_ragged_batch
    torch = _torch()
    pair = (48000, 16000)
    t = RC.tables(*pair)
    L, M = t["L"], t["M"]
    rc, qt, _, lds = RC.shape_of(t["tabs"])
    tile = 16 * qt * t["tabs"]["F"]
    n_max = 4 * tile * M // L
    n_out = -(-n_max * L // M)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rows = cus + 19
    assert rc == _lib.MM_OK and n_out == 4 * tile and rows * 4 > min(4, 163840 // lds) * cus
    lens = 1 + (np.arange(rows, dtype=np.int64) * 7919) % n_max
    lens[:3] = (1, n_max, tile * M // L)
    reach = -(-len(t["h32"]) // L) + 2
    x = np.zeros((rows, n_max), dtype=np.float32)
    want = np.zeros((rows, n_out), dtype=np.float32)
    empty = 0
    for r in range(rows):
        n_out_r = -(-int(lens[r]) * L // M)
        empty += (n_out - n_out_r) // tile
        tap = np.full(n_out_r, -1, dtype=np.int64)
        for k in range(4):
            p = k * (n_max // 4) + reach + (r * 53) % (n_max // 4 - 2 * reach)
            x[r, p] = RC.amplitude(r + k)
            if p < lens[r]:
                RC.response(want[r, :n_out_r], tap, t["h32"], L, M, t["half"], p, RC.amplitude(r + k))
    want[want == 0] = 0.0
    assert empty > rows
    got = resample_ragged_batch(torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu), *pair, method=method)[0].cpu().numpy()
    _same_bits(got, want, (pair, method))


# ---- E: the fall-back ---------------------------------------------------------------------------------------------
def test_ratio_beyond_the_lds_tile_falls_back(gpu):
    from modulation_mfcc_amd import audio_io, resample_batch, resample_ragged_batch
    torch = _torch()
    pair = (48000, 250)
    t = RC.tables(*pair)
    assert RC.shape_of(t["tabs"])[0] == _lib.MM_ERR_UNSUPPORTED
    n_max, lens = 50000, np.array([50000, 777, 1], dtype=np.int64)
    x = np.random.default_rng(11).standard_normal((3, n_max)).astype(np.float32)
    d = torch.from_numpy(x).to(gpu)
    d_lens = torch.from_numpy(lens).to(gpu)
    auto = resample_ragged_batch(d, d_lens, *pair, method="auto")[0].cpu().numpy()
    f64 = resample_ragged_batch(d, d_lens, *pair, method="f64")[0].cpu().numpy()
    _same_bits(auto, f64, "auto against f64")
    n_out_max = -(-n_max * t["L"] // t["M"])
    assert auto.shape == (3, n_out_max)
    for b, n in enumerate(lens):
        one = resample_batch(d[b, :n], *pair, method="f64").cpu().numpy()
        _same_bits(auto[b, :len(one)], one, ("single call", int(n)))
        assert not RC.bits(auto[b, len(one):]).any()
    with pytest.raises(NotImplementedError, match="mm_resample_banded_ragged_f32"):
        resample_ragged_batch(d, d_lens, *pair, method="mfma")
    u = (np.uint32(0x7FC00000) | (np.arange(3 * n_out_max + 2 * GUARD, dtype=np.uint32) & np.uint32(0xFFFFF)))
    out = torch.from_numpy(u.view(np.float32).copy()).to(gpu)
    rc = _launch("mfma", pair, gpu, d.data_ptr(), 3, n_max, n_max, d_lens, out.data_ptr() + 4 * GUARD, n_out_max, n_out_max)
    assert rc == _lib.MM_ERR_UNSUPPORTED
    torch.cuda.synchronize(gpu)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), u)


def test_entries_validate_on_the_host(gpu):
    """Bad arguments are refused before anything is launched: an output count that is not that of n_max, an output pitch
    below the output count, an input pitch below n_max."""
    torch = _torch()
    pair = (48000, 16000)
    x = torch.zeros((2, 300), dtype=torch.float32, device=gpu)
    y = torch.full((2, 100), float("nan"), dtype=torch.float32, device=gpu)
    d_lens = torch.tensor([300, 5], dtype=torch.int64, device=gpu)
    for method in METHODS:
        assert _launch(method, pair, gpu, x.data_ptr(), 2, 300, 300, d_lens, y.data_ptr(), 99, 100) == _lib.MM_ERR_INVALID_ARG
        assert _launch(method, pair, gpu, x.data_ptr(), 2, 300, 300, d_lens, y.data_ptr(), 100, 99) == _lib.MM_ERR_INVALID_ARG
        assert _launch(method, pair, gpu, x.data_ptr(), 2, 300, 299, d_lens, y.data_ptr(), 100, 100) == _lib.MM_ERR_INVALID_ARG
    torch.cuda.synchronize(gpu)
    assert torch.isnan(y).all()
