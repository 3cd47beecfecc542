"""GPU (-m gpu): the sample-rate converters of load_audio -- mm_resample_banded_f32 (matrix pipe, resample_mfma_kernel
<PAD, VEC> x 4, host-built operand tables) and mm_resample_f32 (resample_kernel, float64 accumulation, the fall-back) --
tap by tap, at every launch shape (the ratio matrix of tests/resample_comb.py; tests/test_resample_host.py asserts
through mm_resample_banded_shape that it holds QT 8 / 4 / 2 / 1, both pad values, every pipeline remainder and the
wrapping period remainders).

A  tap by tap          the impulse comb and the edge comb (resample_comb.py: exact in any arithmetic), both kernels,
                       16-byte aligned rows and rows one float off with an odd pitch: equality of the bit patterns
B  the check has teeth a table built from taps whose outer 5 % are zero passes the suite's noise comparison (2e-6 of
                       the maximum) and fails the comb, at the zeroed taps only
C  guard bands         NaN sentinels before and behind the output, NaN padding behind the input rows; n_out % 4 in
                       0 .. 3, odd n_out under several rows (unaligned rows: no 16-byte store), n_out < 4, n_out < F
D  items > workgroups  the grid-stride loop over (row, tile) items re-staging its LDS tile, four and two workgroups per CU
E  the fall-back       ratios whose tile exceeds the LDS: 'auto' is 'f64' bit for bit, 'mfma' raises, the entry point
                       returns MM_ERR_UNSUPPORTED and writes nothing
F  new ratios          the suite's noise comparison (2e-6 of the maximum, scipy.signal.resample_poly with the same
                       float32 taps) at the ratios it did not have

The only tolerance in this file is that 2e-6 (B, E, F: tests/test_gpu_parity.py, test_load_and_resample_on_device).

MEASURED (MI355X).  Wall time of the file: 3.7 s for its 67 cases (1.5 s of it device set-up; no case above 0.2 s).
F, max|got - want| / max|want| on the suite's noise (3 x 20000) and on two-row clips of 1 / 7 / 300 samples:

    in -> out        L / M      shape        mfma 20000  f64 20000   mfma 1 / 7 / 300            f64 1 / 7 / 300
    16000 -> 48000   3 / 1      QT 8         3.96e-07    4.62e-08    8.6e-09 1.4e-07 2.9e-07     8.6e-09 4.5e-08 3.4e-08
    16000 -> 12000   3 / 4      QT 8, pad    5.01e-07    3.51e-08    8.3e-09 6.7e-08 2.9e-07     8.3e-09 1.6e-08 4.0e-08
    22050 -> 10000   200 / 441  QT 2         4.94e-07    4.42e-08    2.1e-08 3.2e-08 2.0e-07     2.1e-08 2.4e-08 3.0e-08
    48000 -> 44100   147 / 160  QT 4, pad    4.69e-07    4.81e-08    3.1e-08 5.6e-08 2.3e-07     3.1e-08 2.5e-08 3.5e-08
    192000 -> 16000  1 / 12     QT 4, pad    1.06e-06    2.94e-08    2.0e-08 1.6e-08 2.0e-07     2.0e-08 6.3e-09 2.9e-08
    16000 -> 11025   441 / 640  QT 1, pad    3.35e-07    3.04e-08    3.7e-08 5.9e-08 3.1e-07     3.7e-08 3.1e-08 4.3e-08
    44100 -> 48000   160 / 147  QT 8         3.63e-07    3.07e-08    4.3e-08 7.7e-08 3.0e-07     4.3e-08 3.1e-08 3.6e-08

(1 / 12 sums 2251 taps per output in two float32 chains: the largest figure, half the bound.)
B, the same noise through the matrix-pipe kernel: 5.58e-07 (48 -> 16 kHz) and 4.65e-07 (44.1 -> 16 kHz) with the
library's table, 1.06e-06 and 1.25e-06 with the outer 5 % of each half of the filter zeroed -- both under 2e-6, while
the comb differs at every one of the 2 x 14 and 2 x 2066 zeroed taps, in each of their F / L outputs.  E: 'auto' against scipy 3.04e-08 (48000 -> 250) and
4.19e-08 (44100 -> 250).  A, C, D: equality.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_comb as RC
from modulation_mfcc_amd import _lib

pytestmark = pytest.mark.gpu

IDS = [RC.ratio_id(p) for p in RC.MATRIX]
TOL = 2e-6                       # test_load_and_resample_on_device's bound, times max |want|
GUARD = 32                       # sentinel floats on either side of an output


def _torch():
    import torch
    return torch


def _stream(gpu):
    return C.c_void_p(_torch().cuda.current_stream(gpu).cuda_stream)


def _sentinel(n, gpu, base=0):
    """n quiet NaNs with their position in the payload, as a float32 device tensor (and the same bits on the host)."""
    torch = _torch()
    u = (np.uint32(0x7FC00000) | ((np.arange(n, dtype=np.uint32) + np.uint32(base)) & np.uint32(0xFFFFF)))
    return torch.from_numpy(u.view(np.float32).copy()).to(gpu), u


def _rows_layout(x2, aligned, gpu):
    """Host rows [rows, n] -> (holder, data_ptr, pitch) on the device: `aligned` rows start on 16 bytes with a pitch that
    is a multiple of 4 (the VEC instantiations), otherwise one float off with an odd pitch (!VEC).  Whatever lies before,
    between and behind the rows is NaN: a kernel that read it as signal would poison its exact output."""
    torch = _torch()
    rows, n = x2.shape
    if aligned:
        pitch, off = (n + 3) // 4 * 4 + 4, 0
    else:
        pitch, off = n + 1 + n % 2, 1
    buf = torch.full((off + rows * pitch + 8,), float("nan"), dtype=torch.float32, device=gpu)
    view = buf[off:off + rows * pitch].view(rows, pitch)
    view[:, :n] = torch.from_numpy(np.array(x2, dtype=np.float32)).to(gpu)
    ptr = view.data_ptr()
    assert buf.data_ptr() % 16 == 0
    assert (ptr % 16 == 0 and pitch % 4 == 0) == aligned and (aligned or pitch % 2 == 1)
    return buf, ptr, pitch


def _launch(method, pair, gpu, x_ptr, rows, n, pitch, y_ptr, n_out, atab=None):
    """One call of mm_resample_banded_f32 ('mfma') or mm_resample_f32 ('f64') -> status."""
    from modulation_mfcc_amd import audio_io
    torch = _torch()
    lib = _lib.load()
    t = RC.tables(*pair)
    L, M = t["L"], t["M"]
    with torch.cuda.device(gpu):
        if method == "mfma":
            tb = audio_io._device_banded(L, M, gpu)
            d_atab = tb["d_atab"] if atab is None else atab
            return lib.mm_resample_banded_f32(x_ptr, rows, n, pitch, d_atab.data_ptr(), tb["d_lo_off"].data_ptr(), tb["F"],
                                              tb["S"], tb["NB"], tb["ksteps"], tb["lo_min"], tb["win"], y_ptr, n_out,
                                              _stream(gpu))
        taps, tpp, half = audio_io._device_taps(L, M, gpu)
        return lib.mm_resample_f32(x_ptr, rows, n, pitch, taps.data_ptr(), L, M, tpp, half, y_ptr, n_out, _stream(gpu))


def _run(method, pair, gpu, x2, aligned=True, atab=None):
    """Rows [rows, n] through one kernel -> float32 [rows, n_out]; the output starts as NaN."""
    torch = _torch()
    t = RC.tables(*pair)
    rows, n = x2.shape
    n_out = -(-n * t["L"] // t["M"])
    hold, ptr, pitch = _rows_layout(x2, aligned, gpu)
    out = torch.full((rows, n_out), float("nan"), dtype=torch.float32, device=gpu)
    assert _launch(method, pair, gpu, ptr, rows, n, pitch, out.data_ptr(), n_out, atab) == _lib.MM_OK
    got = out.cpu().numpy()
    del hold
    return got


# ---- A: tap by tap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mfma", "f64"])
@pytest.mark.parametrize("edge", [False, True], ids=["comb", "edge"])
@pytest.mark.parametrize("pair", RC.MATRIX, ids=IDS)
def test_every_tap_of_every_launch_shape(pair, edge, method, gpu):
    """The comb through the kernel equals a h[m M + half - p L] bit for bit (zeros are +0.0: both kernels start their
    sums at +0.0 and add +-0 products).  Two rows -- the comb and twice the comb -- so the pitch counts; once from
    aligned rows (resample_mfma_kernel<PAD, true>) and once from rows one float off with an odd pitch (<PAD, false>);
    PAD follows the ratio (resample_comb.MATRIX).  The combs span several LDS tiles of 16 QT periods (160 / 441: 5120
    outputs per tile, 141 k outputs), so every tile seam has taps on both sides."""
    x, want, _ = RC.comb(*pair, edge)
    rc, qt, pad, _ = RC.shape_of(RC.tables(*pair)["tabs"])
    assert rc == _lib.MM_OK and len(want) > 16 * qt * RC.tables(*pair)["tabs"]["F"]          # more than one tile
    x2 = np.stack([x, 2.0 * x])
    for aligned in (True, False):
        got = _run(method, pair, gpu, x2, aligned)
        for r, scale in enumerate((1.0, 2.0)):
            w = (np.float32(scale) * want).astype(np.float32)
            bad = np.flatnonzero(RC.bits(got[r]) != RC.bits(w))
            assert bad.size == 0, (pair, method, f"QT {qt} PAD {pad} VEC {int(aligned)}", r, bad.size, bad[:8], got[r][bad[:8]],
                                   w[bad[:8]])


# ---- B: the check has teeth ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _suite_noise():
    """The white noise of test_load_and_resample_on_device: the same generator, the same draws."""
    rng = np.random.default_rng(0)
    rng.uniform(-0.9, 0.9, (30001, 2))
    xs = rng.standard_normal((3, 20000)).astype(np.float32)
    xs.setflags(write=False)
    return xs


def _scipy(x2, pair):
    import scipy.signal
    t = RC.tables(*pair)
    return scipy.signal.resample_poly(np.asarray(x2, dtype=np.float64), t["L"], t["M"], axis=1,
                                      window=t["h32"].astype(np.float64) / t["L"])


@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 16000)], ids=["48000to16000", "44100to16000"])
def test_outer_taps_are_seen_by_the_comb_and_not_by_the_noise(pair, gpu):
    """The SAME kernel with an operand table built from taps whose outer 5 % on each side are zero (what a dropped last
    group of k-steps, a misplaced clamp or a truncated tap count amounts to): on the suite's noise it stays within the
    suite's 2e-6 of the maximum of the UNDOCTORED scipy result -- asserted, because it documents the gap --, on the comb
    it differs at every zeroed tap and nowhere else."""
    from modulation_mfcc_amd.audio_io import banded_tables
    torch = _torch()
    t = RC.tables(*pair)
    h32 = t["h32"]
    cut = int(0.05 * t["half"])             # 5 % of each half of the symmetric filter, at either end
    hz = h32.astype(np.float64)
    hz[:cut] = 0.0
    hz[len(hz) - cut:] = 0.0
    tz = banded_tables(t["L"], t["M"], hz, t["half"])
    for k in ("F", "S", "NB", "ksteps", "lo_min", "win"):
        assert tz[k] == t["tabs"][k]
    d_atab = torch.from_numpy(tz["atab"]).to(gpu)
    xs = _suite_noise()
    want_n = _scipy(xs, pair)
    scale = np.abs(want_n).max()
    e_good = np.abs(_run("mfma", pair, gpu, xs) - want_n).max() / scale
    e_doct = np.abs(_run("mfma", pair, gpu, xs, atab=d_atab) - want_n).max() / scale
    print(f"B {RC.ratio_id(pair)}: noise error {e_good:.2e} (library table), {e_doct:.2e} (outer 5 % zeroed)")
    assert e_good <= TOL
    assert e_doct <= TOL                    # the gap: the noise comparison cannot see the outer taps
    x, want, tap = RC.comb(*pair)
    got = _run("mfma", pair, gpu, x[None, :], atab=d_atab)[0]
    bad = RC.bits(got) != RC.bits(want)
    outer = (tap >= 0) & ((tap < cut) | (tap >= len(h32) - cut))
    assert bad.sum() > 0
    assert not (bad & ~outer).any()         # every mismatch lies at a zeroed tap
    np.testing.assert_array_equal(bad, outer & (want != 0))
    assert (RC.bits(got[bad]) == 0).all()


# ---- C: guard bands and padding -----------------------------------------------------------------------------------
_GUARD_N = {
    (48000, 16000): (1, 4, 7, 10, 13, 46, 47, 50, 53, 56, 1000, 6155),        # F = 16
    (44100, 16000): (3, 7, 300, 441, 1000, 1003, 1006, 1009, 30000),          # F = 160
    (16000, 48000): (1, 2, 3, 4, 5, 11, 43, 1001),                            # F = 30, upsampling
    (16000, 11025): (2, 5, 10, 100, 641, 1500, 20001),                        # F = 441, QT = 1
}


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("pair", sorted(_GUARD_N), ids=[RC.ratio_id(p) for p in sorted(_GUARD_N)])
def test_nothing_is_written_or_read_outside_the_rows(pair, rows, gpu):
    """Both entry points, output = rows n_out floats between two bands of NaN sentinels, input = [:, :n] of a buffer
    whose padding columns are NaN: the sentinels survive, the outputs are finite, and they do not depend on the pitch
    (p = pitch - n in 0 -- contiguous, nothing behind the rows --, 1, 3, 4).  With n_out odd and three rows the second
    row starts unaligned: the 16-byte store must fall back to scalar ones."""
    torch = _torch()
    t = RC.tables(*pair)
    L, M, F = t["L"], t["M"], t["tabs"]["F"]
    n_outs = [-(-n * L // M) for n in _GUARD_N[pair]]
    assert {v % 4 for v in n_outs} == {0, 1, 2, 3} and any(v % 2 for v in n_outs)
    assert any(v < 4 for v in n_outs) and any(4 <= v < F for v in n_outs) and any(v > F for v in n_outs)
    rng = np.random.default_rng(5)
    for n, n_out in zip(_GUARD_N[pair], n_outs):
        x = rng.standard_normal((rows, n)).astype(np.float32)
        for method in ("mfma", "f64"):
            first = None
            for p in (0, 1, 3, 4):
                xin = torch.full((rows, n + p), float("nan"), dtype=torch.float32, device=gpu)
                xin[:, :n] = torch.from_numpy(x).to(gpu)
                out, sent = _sentinel(rows * n_out + 2 * GUARD, gpu, base=n)
                y_ptr = out.data_ptr() + 4 * GUARD
                assert _launch(method, pair, gpu, xin.data_ptr(), rows, n, n + p, y_ptr, n_out) == _lib.MM_OK
                got = out.cpu().numpy().view(np.uint32)
                what = (pair, rows, n, method, p)
                np.testing.assert_array_equal(got[:GUARD], sent[:GUARD], err_msg=f"front sentinel {what}")
                np.testing.assert_array_equal(got[-GUARD:], sent[-GUARD:], err_msg=f"back sentinel {what}")
                body = got[GUARD:-GUARD]
                assert np.isfinite(body.view(np.float32)).all(), what
                if first is None:
                    first = body.copy()
                else:
                    np.testing.assert_array_equal(body, first, err_msg=f"pitch n + {p} against contiguous rows {what}")


# ---- D: more items than workgroups --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mfma", "f64"])
@pytest.mark.parametrize("pair,n", [((8000, 16000), 64), ((44100, 16000), 600)], ids=["8000to16000", "44100to16000"])
def test_more_rows_than_resident_workgroups(pair, n, method, gpu):
    """rows = 4 CUs + 76, one LDS tile per row: the grid (four workgroups per CU at 8 -> 16 kHz, two at 44.1 -> 16 kHz)
    is smaller than the item count, so workgroups come round to a second and third item and stage a new tile into the
    same LDS after the barrier.  One impulse per row at sample row % 64, amplitude +-2^k: exact taps per row."""
    from modulation_mfcc_amd import resample_batch
    torch = _torch()
    t = RC.tables(*pair)
    L, M = t["L"], t["M"]
    rc, qt, _, lds = RC.shape_of(t["tabs"])
    n_out = -(-n * L // M)
    assert rc == _lib.MM_OK and n_out <= 16 * qt * t["tabs"]["F"]                      # one tile per row
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rows = 4 * cus + 76
    assert rows > min(4, 163840 // lds) * cus
    x = np.zeros((rows, n), dtype=np.float32)
    want = np.zeros((rows, n_out), dtype=np.float32)
    tap = np.full(n_out, -1, dtype=np.int64)
    for r in range(rows):
        x[r, r % 64] = RC.amplitude(r)
        tap[:] = -1
        RC.response(want[r], tap, t["h32"], L, M, t["half"], r % 64, RC.amplitude(r))
    want[want == 0] = 0.0
    got = resample_batch(torch.from_numpy(x).to(gpu), *pair, method=method).cpu().numpy()
    assert got.shape == want.shape and np.count_nonzero(want) > rows
    bad = np.argwhere(RC.bits(got) != RC.bits(want))
    assert bad.shape[0] == 0, (pair, method, bad.shape[0], bad[:8])


# ---- E: the fall-back ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RC.UNSUPPORTED, ids=[RC.ratio_id(p) for p in RC.UNSUPPORTED])
def test_ratios_beyond_the_lds_tile_fall_back(pair, gpu):
    from modulation_mfcc_amd import audio_io, resample_batch
    torch = _torch()
    t = RC.tables(*pair)
    assert RC.shape_of(t["tabs"])[0] == _lib.MM_ERR_UNSUPPORTED
    x = np.random.default_rng(11).standard_normal((2, 200000)).astype(np.float32)
    d = torch.from_numpy(x).to(gpu)
    auto = resample_batch(d, *pair, method="auto").cpu().numpy()
    f64 = resample_batch(d, *pair, method="f64").cpu().numpy()
    np.testing.assert_array_equal(RC.bits(auto), RC.bits(f64))
    want = _scipy(x, pair)
    assert auto.shape == want.shape == (2, -(-200000 * t["L"] // t["M"]))
    err = np.abs(auto - want).max() / np.abs(want).max()
    print(f"E {RC.ratio_id(pair)}: {err:.2e}")
    assert err <= TOL
    with pytest.raises(NotImplementedError, match="mm_resample_banded_f32"):
        resample_batch(d, *pair, method="mfma")
    # the entry point itself: refused before anything is launched
    n_out = auto.shape[1]
    out, sent = _sentinel(2 * n_out + 2 * GUARD, gpu)
    tb = audio_io._device_banded(t["L"], t["M"], gpu)
    lib = _lib.load()
    with torch.cuda.device(gpu):
        rc = lib.mm_resample_banded_f32(d.data_ptr(), 2, 200000, 200000, tb["d_atab"].data_ptr(), tb["d_lo_off"].data_ptr(),
                                        tb["F"], tb["S"], tb["NB"], tb["ksteps"], tb["lo_min"], tb["win"],
                                        out.data_ptr() + 4 * GUARD, n_out, _stream(gpu))
    assert rc == _lib.MM_ERR_UNSUPPORTED
    torch.cuda.synchronize(gpu)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), sent)


# ---- F: new ratios against scipy ----------------------------------------------------------------------------------
_NEW = ((16000, 48000), (16000, 12000), (22050, 10000), (48000, 44100), (192000, 16000), (16000, 11025), (44100, 48000))


@pytest.mark.parametrize("pair", _NEW, ids=[RC.ratio_id(p) for p in _NEW])
def test_new_ratios_against_scipy(pair, gpu):
    """test_load_and_resample_on_device's comparison (scipy's polyphase arithmetic in float64 with the same float32
    taps, 2e-6 of the maximum) at the ratios of the matrix it does not run -- QT = 4 and QT = 1 among them -- on its
    noise and on clips shorter than the filter."""
    from modulation_mfcc_amd import resample_batch
    torch = _torch()
    t = RC.tables(*pair)
    rng = np.random.default_rng(17)
    for x in (_suite_noise(),) + tuple(rng.standard_normal((2, n)).astype(np.float32) for n in (1, 7, 300)):
        want = _scipy(x, pair)
        for method in ("mfma", "f64"):
            got = resample_batch(torch.from_numpy(np.array(x)).to(gpu), *pair, method=method).cpu().numpy()
            assert got.shape == want.shape == (x.shape[0], -(-x.shape[1] * t["L"] // t["M"]))
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
            print(f"F {RC.ratio_id(pair)} n={x.shape[1]} {method}: {err:.2e}")
            assert err <= TOL, (pair, x.shape[1], method, err)
