"""GPU (-m gpu): applyFilter's three filters with a length per curve -- mm_sosfiltfilt_ragged_f64 / _f32_f64,
mm_stencil_ragged_f64, mm_fir_filtfilt_ragged_f64 / _f32_f64 and mm_savgol_ragged_f64 through sosfiltfilt_ragged_batch,
fir_filtfilt_ragged_batch, savgol_ragged_batch, apply_filter_ragged_batch, applyFilter_batch, and their two callers,
tail.mfcc_change_ragged_device and get_f0_batch.

The criterion is exactness: row b of a ragged call equals the single-length call on x[b:b+1, :n_b] bit for bit
(torch.equal), and is +0.0 behind n_b.  The single-length calls are pinned to the long-double oracles by
tests/test_gpu_sos.py and tests/test_gpu_longfilt.py; test_against_the_oracles repeats that anchor on ragged rows, one
case per kernel family, with the bounds those files publish.

Inputs: sos_oracle.envelope_rows / longfilt_oracle.curve_rows in a padded batch whose row stride exceeds n_max, NaN
behind every row unless a test says otherwise.  Lengths sit where the kernels change path: the 1088-sample segments of
the IIR rows (n_ext = n + 2 padlen around 1, 2, 16 and 17 segments), the 2048-output tiles of the long filters."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import longfilt_oracle as LQ
import mfcc_oracle as MO
import pyin_oracle as PO
import sos_oracle as SQ
from modulation_mfcc_amd import (_lib, applyFilter, applyFilter_batch, apply_filter_ragged_batch, calc, filters,
                                 fir_filtfilt_batch, fir_filtfilt_ragged_batch, get_f0, get_f0_batch, pitch, savgol_batch,
                                 savgol_ragged_batch, sosfiltfilt_batch, sosfiltfilt_ragged_batch, tail)

pytestmark = pytest.mark.gpu

T = filters.LONGFILT_TILE
SEG = 1088                  # samples per segment of the IIR rows (MM_SEG_LEN of csrc/mm_sos_rows.hip.inc)
R_SOS, FLOOR_SOS = 16.0, 1e-15          # R_SWEEP of tests/test_gpu_sos.py and its floor
R_LONG, EPS = 32.0, 2.0 ** -52          # R_SWEEP, EPS of tests/test_gpu_longfilt.py


@functools.lru_cache(maxsize=None)
def _rows(seed, rows, n, dtype=np.float64, kind="curve"):
    make = LQ.curve_rows if kind == "curve" else SQ.envelope_rows
    x = make(np.random.default_rng(seed), rows, n, dtype)
    x.setflags(write=False)
    return x


def _packed(x, lens, gpu, fill=np.nan, extra=5, n_max=None):
    """x[b, :lens[b]] in a device view [rows, n_max] whose row stride is n_max + extra; behind every row: ``fill`` (a number,
    or 'next': the next row's samples times 7)."""
    n_max = int(max(lens)) if n_max is None else n_max
    buf = np.empty((len(lens), n_max + extra), dtype=x.dtype)
    for b, n in enumerate(lens):
        buf[b] = 7.0 * x[(b + 1) % len(lens), :n_max + extra] if isinstance(fill, str) else fill
        buf[b, :n] = x[b, :n]
    v = torch.from_numpy(buf).to(gpu)[:, :n_max]
    assert v.stride(0) == n_max + extra
    return v


def _check(got, single, xd, lens, rows=None, what=""):
    """Rows of the ragged result against ``single`` on the row alone: equal bits, +0.0 behind the row's length."""
    assert tuple(got.shape) == tuple(xd.shape) and got.is_cuda
    for b in (range(len(lens)) if rows is None else rows):
        n = int(lens[b])
        want = single(xd[b:b + 1, :n])
        assert want.shape == (1, n) and want.dtype == got.dtype, (what, b, want.dtype, got.dtype)
        assert not torch.isnan(want).any()
        assert torch.equal(got[b, :n], want[0]), \
            f"{what} row {b} n={n}: {int((got[b, :n] != want[0]).sum())} of {n} samples differ from the row alone"
        behind = got[b, n:]
        assert bool((behind == 0).all()) and not bool(torch.signbit(behind).any()), f"{what} row {b} n={n}: not +0.0 behind n_b"


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit-equality with the row alone
# ---------------------------------------------------------------------------------------------------------------------
def _sos(sections):
    """Butterworth low-pass at 2.4e-3 of Nyquist (12 Hz at 10 kHz, a point of test_gpu_sos.py's sweep): narrow enough that
    a segment's start state still carries 0.3 % (order 2) to 20 % (order 8) of the state 1088 samples earlier, so the scan
    over the segments is part of every output bit.  (At 0.05 of Nyquist the state has decayed below one ulp within a segment
    and any two segment scans agree.)"""
    sos = scipy.signal.butter(2 * sections, 2.4e-3, output="sos")
    assert sos.shape == (sections, 6)
    return sos


def _iir_lengths(sections, up_to_segments=18):
    pad = 3 * (2 * sections + 1)
    ext = [SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 16 * SEG - 1, 16 * SEG + 1, 17 * SEG + 1]
    return [pad + 1] + [e - 2 * pad for e in ext if e <= up_to_segments * SEG], pad


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("sections", [1, 2, 3, 4])
def test_iir_rows_equal_the_row_alone(sections, dtype, gpu):
    """Up to 8 rows: a wave per segment, the form a row alone takes; the lengths end one sample before, at and after a
    segment boundary, for 1, 2, 16 and 17 segments (the segment scan's lanes), and at padlen + 1."""
    sos = _sos(sections)
    lens, pad = _iir_lengths(sections)
    assert len(lens) == 8 and min(lens) == pad + 1
    x = _rows(10 + sections, len(lens), max(lens) + 5, dtype, "envelope")
    xd = _packed(x, lens, gpu)
    got = sosfiltfilt_ragged_batch(xd, lens, sos)
    assert got.dtype == torch.float64
    _check(got, lambda r: sosfiltfilt_batch(r, sos), xd, lens, what=f"iir {sections} sections {dtype.__name__}")


@pytest.mark.parametrize("sections", [1, 2, 3, 4])
def test_iir_130_rows_equal_the_row_alone(sections, gpu):
    """130 rows, where the single-length call switches to a workgroup per row.  A row alone runs a wave per segment, and the
    contract is bit-equality with the row alone, so the ragged call takes the workgroup form only where it is the same
    arithmetic: n_max + 2 padlen within ONE round of 16 segments (batch A: extended lengths up to 16 segments less a
    sample).  Batch B reaches 17 segments and a sample: a wave per segment at every row count.  Both against the single
    rows, at the boundary lengths and at two rows of random length; every row: zeros behind its length, no NaN."""
    sos = _sos(sections)
    single = lambda r: sosfiltfilt_batch(r, sos)                                     # noqa: E731
    for name, segs in (("A: one round", 16), ("B: two rounds", 18)):
        special, pad = _iir_lengths(sections, segs)
        rng = np.random.default_rng(sections)
        lens = list(rng.integers(pad + 1, max(special) + 1, 130))
        where = [0, 129] + list(range(7, 7 + 11 * (len(special) - 2), 11))
        for w, n in zip(where, special):
            lens[w] = n
        n_max = max(lens)
        assert (n_max + 2 * pad <= 16 * SEG) == (segs == 16)
        x = SQ.envelope_rows(np.random.default_rng(20 + sections), 130, n_max + 5)      # (19 MB: not kept)
        xd = _packed(x, lens, gpu)
        got = sosfiltfilt_ragged_batch(xd, lens, sos)
        _check(got, single, xd, lens, rows=where + [64, 65], what=f"iir {sections} sections, 130 rows, {name}")
        behind = torch.arange(n_max, device=gpu)[None, :] >= torch.tensor(lens, device=gpu)[:, None]
        assert bool((got[behind] == 0).all()) and not bool(torch.isnan(got).any())


FIR_L = [2, 8, 9, 64, 65, 101]


def _firwin(L):
    return scipy.signal.firwin(L, 0.24, window=("kaiser", 7.4))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", FIR_L)
def test_fir_rows_equal_the_row_alone(L, dtype, gpu):
    taps = _firwin(L)
    lens = [3 * L + 1, T - 1, T, T + 1, 2 * T + L]
    x = _rows(30 + L, len(lens), max(lens) + 5, dtype)
    xd = _packed(x, lens, gpu)
    got = fir_filtfilt_ragged_batch(xd, lens, taps)
    assert got.dtype == torch.float64
    _check(got, lambda r: fir_filtfilt_batch(r, taps), xd, lens, what=f"fir L={L} {dtype.__name__}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("W", [5, 16, 17, 18, 101])
def test_savgol_rows_equal_the_row_alone(W, dtype, gpu):
    """A row with n == W has both edge fits on one window (and, for an even W, no interior output at all)."""
    lens = [W, W + 1, T, T + 1, 2 * T + W]
    x = _rows(40 + W, len(lens), max(lens) + 5, dtype)
    xd = _packed(x, lens, gpu)
    for p in (2, 3):
        for deriv in (0, 1):
            got = savgol_ragged_batch(xd, lens, W, p, deriv=deriv, delta=0.005)
            assert got.dtype == xd.dtype                                        # float32 in, float32 out, as scipy
            _check(got, lambda r: savgol_batch(r, W, p, deriv=deriv, delta=0.005), xd, lens,
                   what=f"sg W={W} p={p} deriv={deriv} {dtype.__name__}")


APPLY_CASES = [dict(filt="iir", cutOff=[12]), dict(filt="iir", cutOff=[3, 20], filtType="band", filtLen=2),
               dict(filt="fir", cutOff=[12], filtLen=6), dict(filt="fir", cutOff=[12], filtLen=101),
               dict(filt="sg", cutOff=[12], filtLen=7), dict(filt="sg", cutOff=[12], filtLen=101),
               dict(filt="sg", cutOff=[12], filtLen=16, polyOrd=2)]
APPLY_LENS = [1001, 304, 650, 2 * T + 7, 512]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kw", APPLY_CASES, ids=[f"{k['filt']}{k.get('filtLen', 6)}{k.get('filtType', '')}" for k in APPLY_CASES])
def test_apply_filter_ragged_batch_equals_apply_filter(kw, dtype, gpu):
    """Every route of applyFilter for device curves: the IIR rows, the banded operator (6 taps, windows of 7 and 16), the
    long kernels (101), and -- float32 'fir' of 6 taps -- the per-length loop that stays."""
    x = _rows(50, len(APPLY_LENS), max(APPLY_LENS) + 5, dtype)
    xd = _packed(x, APPLY_LENS, gpu)
    got = apply_filter_ragged_batch(xd, APPLY_LENS, 100.0, **kw)
    _check(got, lambda r: applyFilter(r, 100.0, **kw), xd, APPLY_LENS, what=f"{kw} {dtype.__name__}")


def test_apply_filter_batch_on_a_mixed_list(gpu):
    x = _rows(51, 6, 900)
    curves = [x[0, :700], torch.from_numpy(x[1, :333].copy()).to(gpu), torch.from_numpy(x[2, :900].astype(np.float32)).to(gpu),
              x[3, :420].astype(np.float32), torch.from_numpy(x[4, :899].copy()).to(gpu),
              torch.from_numpy(x[5, :340].astype(np.float32)).to(gpu)]
    for kw in (dict(filt="iir", cutOff=[12]), dict(filt="fir", cutOff=[12], filtLen=101), dict(filt="sg", cutOff=[12], filtLen=7)):
        got = applyFilter_batch(curves, 100.0, **kw)
        assert isinstance(got, list) and len(got) == len(curves)
        for i, (c, g) in enumerate(zip(curves, got)):
            want = applyFilter(c, 100.0, **kw)
            assert type(g) is type(want) and g.dtype == want.dtype and g.shape == want.shape, (kw, i)
            if isinstance(c, torch.Tensor):
                assert g.is_cuda and torch.equal(g, want), (kw, i)
            else:
                np.testing.assert_array_equal(g, want, err_msg=f"{kw} curve {i}")
    assert applyFilter_batch([], 100.0, filt="iir", cutOff=[12]) == []
    with pytest.raises(ValueError, match=r"padlen, which is 303\. \(curve 1\)"):
        applyFilter_batch([curves[0], curves[1][:303]], 100.0, filt="fir", cutOff=[12], filtLen=101)


# ---------------------------------------------------------------------------------------------------------------------
# 2. row independence
# ---------------------------------------------------------------------------------------------------------------------
INDEP = {
    "iir": (lambda x, l: sosfiltfilt_ragged_batch(x, l, _sos(3)), 1500),
    "fir101": (lambda x, l: fir_filtfilt_ragged_batch(x, l, _firwin(101)), T + 9),
    "sg101": (lambda x, l: savgol_ragged_batch(x, l, 101, 3), T + 9),
    "fir6 (banded)": (lambda x, l: apply_filter_ragged_batch(x, l, 100.0, filt="fir", cutOff=[12], filtLen=6), 137),
    "sg7 (banded)": (lambda x, l: apply_filter_ragged_batch(x, l, 100.0, filt="sg", cutOff=[12], filtLen=7), 137),
}


@pytest.mark.parametrize("name", list(INDEP))
def test_row_independence(name, gpu):
    """The same row at the same n_b in batches of different neighbours, neighbour lengths and n_max, with NaN, zeros or
    another row's values behind n_b: equal bits; and the whole call again: equal bits."""
    run, n = INDEP[name]
    wide = 2 * n + 300
    x = _rows(60, 4, wide + 5)
    me = x[0]

    def batch(rows, lens, pos, fill, n_max):
        src = np.stack(rows)
        return run(_packed(src, lens, gpu, fill=fill, n_max=n_max), lens)[pos, :n].clone()
    a = batch([me, x[1], x[2]], [n, wide, 400], 0, np.nan, wide)
    b = batch([x[3], x[1], me], [n + 100, n + 150, n], 2, 0.0, n + 150)
    c = batch([x[2], me], [n, n], 1, "next", n)
    assert not torch.isnan(a).any()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a, batch([me, x[1], x[2]], [n, wide, 400], 0, np.nan, wide))


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the long-double oracles, one case per kernel family
# ---------------------------------------------------------------------------------------------------------------------
def test_against_the_oracles(gpu):
    """E = max|y - oracle| / max|oracle| per row, on the row's own samples; E_scipy is scipy's float64 result against the
    same oracle.  IIR: E <= 16 max(E_scipy, 1e-15); FIR and Savitzky-Golay: E <= 32 max(E_scipy, 2^-52)."""
    lens = [1500, 3 * 101 + 1, T + 1, 2 * T + 101, 777]
    x = _rows(70, len(lens), max(lens) + 5)
    xd = _packed(x, lens, gpu)
    sos, taps = _sos(3), _firwin(101)
    st6 = _firwin(6)
    fams = [
        ("iir", sosfiltfilt_ragged_batch(xd, lens, sos), lambda r: SQ.sosfiltfilt_ext_ld(sos, r),
         lambda r: scipy.signal.sosfiltfilt(sos, r), R_SOS, FLOOR_SOS),
        ("fir101", fir_filtfilt_ragged_batch(xd, lens, taps), lambda r: LQ.fir_filtfilt_ext_ld(taps, r),
         lambda r: scipy.signal.filtfilt(taps, 1, r), R_LONG, EPS),
        ("sg101", savgol_ragged_batch(xd, lens, 101, 3), lambda r: LQ.savgol_ext_ld(r, 101, 3),
         lambda r: scipy.signal.savgol_filter(r, 101, 3, mode="interp"), R_LONG, EPS),
        ("fir6 (banded)", apply_filter_ragged_batch(xd, lens, 100.0, filt="fir", cutOff=[12], filtLen=6),
         lambda r: LQ.fir_filtfilt_ext_ld(st6, r), lambda r: scipy.signal.filtfilt(st6, 1, r), R_LONG, EPS),
        ("sg7 (banded)", apply_filter_ragged_batch(xd, lens, 100.0, filt="sg", cutOff=[12], filtLen=7),
         lambda r: LQ.savgol_ext_ld(r, 7, 3), lambda r: scipy.signal.savgol_filter(r, 7, 3, mode="interp"), R_LONG, EPS),
    ]
    for name, got, oracle, sci, R, floor in fams:
        g = got.cpu().numpy()
        for b, n in enumerate(lens):
            ext = np.asarray(oracle(x[b, :n])).reshape(-1)
            e_ref, e_dev = SQ.rel_err(sci(x[b, :n]), ext), SQ.rel_err(g[b, :n], ext)
            print(f"{name} row {b} n={n}: E_scipy {e_ref:.2e} E_dev {e_dev:.2e} ratio {e_dev / max(e_ref, floor):.2f}")
            assert e_dev <= R * max(e_ref, floor), (name, b, n, e_ref, e_dev)


# ---------------------------------------------------------------------------------------------------------------------
# 4. device lengths
# ---------------------------------------------------------------------------------------------------------------------
DEV_CASES = {
    # name: (call, shortest row scipy takes, scipy's text)
    "iir": (lambda x, l: sosfiltfilt_ragged_batch(x, l, _sos(3)), 22, r"padlen, which is 21\."),
    "fir9": (lambda x, l: fir_filtfilt_ragged_batch(x, l, _firwin(9)), 28, r"padlen, which is 27\."),
    "sg21": (lambda x, l: savgol_ragged_batch(x, l, 21, 3), 21, r"window_length must be less than or equal to the size of x\."),
    "fir6 (banded)": (lambda x, l: apply_filter_ragged_batch(x, l, 100.0, filt="fir", cutOff=[12], filtLen=6), 19,
                      r"padlen, which is 18\."),
    "sg7 (banded)": (lambda x, l: apply_filter_ragged_batch(x, l, 100.0, filt="sg", cutOff=[12], filtLen=7), 7,
                     r"window_length must be less than or equal to the size of x\."),
}


@pytest.mark.parametrize("name", list(DEV_CASES))
def test_device_lengths(name, gpu):
    """An int64 device tensor goes through with no read-back: the same bits as host lengths.  0 and n_max + 5 are clamped
    to 1 and n_max; a row scipy refuses (one sample; one below the filter's minimum) comes out NaN in [0, n_b) and zero
    behind it, its neighbours stay right.  int32: TypeError.  The same lengths on the host: scipy's text, the row named."""
    run, least, text = DEV_CASES[name]
    n_max = 150
    dev_lens = [150, 0, 77, n_max + 5, least - 1, least]
    eff_lens = [150, 1, 77, n_max, least - 1, least]
    host_lens = [150, 40, 77, n_max, 40, least]              # valid stand-ins in the rows a host call refuses
    x = _rows(80, 6, n_max + 5)
    xd = _packed(x, eff_lens, gpu)
    dl = torch.tensor(dev_lens, dtype=torch.int64, device=gpu)
    with _no_read_back():
        got = run(xd, dl)
    host = run(xd, host_lens)
    for b in (0, 2, 3, 5):
        assert torch.equal(got[b], host[b]), (name, b)
        assert not torch.isnan(got[b]).any()
    for b in (1, 4):
        n = eff_lens[b]
        assert bool(torch.isnan(got[b, :n]).all()), (name, b)
        assert bool((got[b, n:] == 0).all()) and not bool(torch.signbit(got[b, n:]).any()), (name, b)
    with pytest.raises(TypeError):
        run(xd, dl.to(torch.int32))
    with pytest.raises(ValueError, match=text + r" \(row 1 has 1 samples\)") as err:
        run(xd, eff_lens)
    assert isinstance(err.value, filters.RowRefused) and err.value.row == 1


@contextlib.contextmanager
def _no_read_back():
    """Inside: any Tensor.cpu / .tolist / .item / .numpy raises (the lengths stay on the device)."""
    def refuse(*a, **k):
        raise AssertionError("a device tensor was read back")
    names = ("cpu", "tolist", "item", "numpy")
    own = {k: torch.Tensor.__dict__[k] for k in names if k in torch.Tensor.__dict__}
    for k in names:
        setattr(torch.Tensor, k, refuse)
    try:
        yield
    finally:
        for k in names:
            if k in own:
                setattr(torch.Tensor, k, own[k])
            else:
                delattr(torch.Tensor, k)             # (inherited from the C base class again)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the loops over the distinct lengths are gone
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _single_length_calls():
    """Records every call of the single-length filter functions, wherever a module holds them."""
    calls = []
    spots = [(filters, "sosfiltfilt_batch"), (filters, "fir_filtfilt_batch"), (filters, "savgol_batch"),
             (calc, "apply_stencil"), (filters, "applyFilter"), (pitch, "applyFilter"), (tail, "applyFilter"),
             (calc, "applyFilter")]
    saved = [(m, k, getattr(m, k)) for m, k in spots]

    def wrap(k, fn):
        def counted(*a, **kw):
            calls.append(k)
            return fn(*a, **kw)
        return counted
    for m, k, fn in saved:
        setattr(m, k, wrap(k, fn))
    try:
        yield calls
    finally:
        for m, k, fn in saved:
            setattr(m, k, fn)


F0_SR = 16000
F0_KW = {"iir": dict(outFilter="iir", outFiltCutOff=[10]), "fir": dict(outFilter="fir", outFiltCutOff=[10]),
         "sg": dict(outFilter="sg", outFiltCutOff=[10], outFiltLen=7)}


@pytest.mark.parametrize("filt", list(F0_KW))
def test_get_f0_batch_filters_in_one_ragged_call(filt, gpu):
    """Five clips, five frame counts: no single-length filter function is reached, and every curve equals get_f0 on the
    clip alone bit for bit."""
    g = [PO.synth("glide", F0_SR, s, np.float64, seed=i) for i, s in enumerate((0.6, 0.45, 0.5, 0.4, 0.55))]
    clips = [g[0], g[1], torch.from_numpy(g[2]).to(gpu), g[3], torch.from_numpy(g[4]).to(gpu)]
    kw = dict(method="pyin", interpUnvoiced="linear", **F0_KW[filt])
    with _single_length_calls() as calls:
        got = get_f0_batch(clips, F0_SR, **kw)
    assert not calls, calls
    assert len({len(t) for _, t in got}) == 5
    for i, (c, (f0, f0t)) in enumerate(zip(clips, got)):
        wf, wt = get_f0(c, F0_SR, **kw)
        np.testing.assert_array_equal(f0t, wt)
        if isinstance(c, torch.Tensor):
            assert f0.is_cuda and torch.equal(f0, wf), f"clip {i}"
        else:
            np.testing.assert_array_equal(f0, wf, err_msg=f"clip {i}")
            assert not np.isnan(f0).any()


C1 = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)


@pytest.mark.parametrize("kwargs", [dict(outFilter="fir", outFiltCutOff=[12]),
                                    dict(outFilter="sg", outFiltCutOff=[12], outFiltLen=7, outFiltPolyOrd=3),
                                    dict(outFilter="fir", outFiltCutOff=[12], outFiltLen=11)],
                         ids=["fir6", "sg7", "fir11"])
def test_change_tail_filters_in_one_ragged_call(kwargs, gpu):
    """tail.mfcc_change_ragged_device with a 'fir' / 'sg' output filter: no single-length filter function is reached, a
    device ``frames`` tensor is not read back, and every curve equals, bit for bit, what the loop it replaces gave:
    applyFilter on the clip's own stretch of the ragged curve.  (The curve BEFORE the output filter comes from the ragged
    change kernel, which differs from the single-length tail by rounding by design -- include/modmfcc.h,
    mm_mfcc_change_ragged_f64 -- so against mfcc_change_device on the clip alone the bound is that tail's 1e-10.)"""
    from modulation_mfcc_amd import MfccConfig, get_plan
    plan = get_plan(MfccConfig(**C1))
    Tm, frames = 300, [300, 40, 211, 64, 123]
    m = np.random.default_rng(3).standard_normal((len(frames), 13, Tm)).cumsum(axis=2).astype(np.float32)
    for b, n in enumerate(frames):
        m[b, :, n:] = np.nan
    md = torch.from_numpy(m).to(gpu)
    kw = dict(tStep=0.01, **kwargs)
    with _single_length_calls() as calls:
        host = tail.mfcc_change_ragged_device(plan, md, frames, **kw)
        fr = torch.tensor(frames, dtype=torch.int64, device=gpu)
        with _no_read_back():
            dev = tail.mfcc_change_ragged_device(plan, md, fr, **kw)
    assert not calls, calls
    assert torch.equal(host, dev)
    curve = plan.mfcc_change_ragged(md, frames, tail.design_lowpass(6, 12, 0.01), None, remove_first=True,
                                    diff_method="grad", out_filter=False)
    fkw = dict(filt=kwargs["outFilter"], cutOff=kwargs["outFiltCutOff"], filtLen=kwargs.get("outFiltLen", 6),
               polyOrd=kwargs.get("outFiltPolyOrd", 3))
    for b, n in enumerate(frames):
        assert torch.equal(host[b, :n], applyFilter(curve[b, :n], 100.0, **fkw)), f"clip {b}"
        assert bool((host[b, n:] == 0).all()) and not bool(torch.signbit(host[b, n:]).any())
        alone = tail.mfcc_change_device(plan, md[b:b + 1, :, :n].contiguous(), **kw)[0].cpu().numpy()
        want = MO.mfcc_change_tail(m[b, :, :n], **kw)
        for y in (alone, host[b, :n].cpu().numpy()):
            assert np.abs(y - want).max() <= 1e-10 * np.abs(want).max(), f"clip {b}"


def test_six_sections_keep_the_per_length_route(gpu):
    """A band-pass of order 6 has six sections: no ragged kernel (the time-major kernels are single-length), so
    apply_filter_ragged_batch filters per distinct length through applyFilter -- and is still right, with host and with
    device lengths.  The ragged entry itself refuses: MM_ERR_UNSUPPORTED."""
    lens = [400, 250, 400, 333]
    x = _rows(90, len(lens), 405)
    xd = _packed(x, lens, gpu)
    kw = dict(filt="iir", cutOff=[3, 20], filtType="band", filtLen=6)
    sos = filters.iir_sos(100.0, cutOff=[3, 20], filtLen=6, filtType="band")
    assert sos.shape == (6, 6)
    with _single_length_calls() as calls:
        got = apply_filter_ragged_batch(xd, lens, 100.0, **kw)
    assert calls.count("applyFilter") == 3 and calls.count("sosfiltfilt_batch") == 3, calls
    dev = apply_filter_ragged_batch(xd, torch.tensor(lens, dtype=torch.int64, device=gpu), 100.0, **kw)
    assert torch.equal(got, dev)
    g = got.cpu().numpy()
    for b, n in enumerate(lens):
        ext = SQ.sosfiltfilt_ext(sos, x[b, :n])
        e_ref, e_dev = SQ.rel_err(scipy.signal.sosfiltfilt(sos, x[b, :n]), ext), SQ.rel_err(g[b, :n], ext)
        assert e_dev <= R_SOS * max(e_ref, FLOOR_SOS), (b, e_ref, e_dev)
        assert (g[b, n:] == 0).all() and not np.signbit(g[b, n:]).any()
    with pytest.raises(NotImplementedError, match="mm_sosfiltfilt_ragged_f64"):
        sosfiltfilt_ragged_batch(xd, lens, sos)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C entries check before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_checks_fire_before_any_launch(gpu):
    """Behind valid device pointers: every refused call leaves the output's sentinel in place."""
    lib = _lib.load()
    rows, n = 3, 400
    x = torch.zeros((rows, n), dtype=torch.float64, device=gpu)
    xf = x.float()
    lens = torch.full((rows,), n, dtype=torch.int64, device=gpu)
    out = torch.full((rows, n), 7.0, dtype=torch.float64, device=gpu)
    tab = torch.zeros(4096, dtype=torch.float64, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    s3, s5 = (np.ascontiguousarray(scipy.signal.butter(o, 0.1, output="sos")) for o in (6, 10))
    need = int(lib.mm_sosfiltfilt_ragged_workspace_bytes(rows, n))
    assert 0 < need <= int(lib.mm_sosfiltfilt_workspace_bytes(rows, n))
    assert lib.mm_sosfiltfilt_ragged_workspace_bytes(0, n) == 0 and lib.mm_sosfiltfilt_ragged_workspace_bytes(rows, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    INV, UNS, WSP = _lib.MM_ERR_INVALID_ARG, _lib.MM_ERR_UNSUPPORTED, _lib.MM_ERR_WORKSPACE

    def sos(fn=lib.mm_sosfiltfilt_ragged_f64, src=x, nn=n, ln=lens.data_ptr(), s=s3, wsb=need):
        return fn(src.data_ptr(), rows, nn, n, ln, s.ctypes.data, s.shape[0], out.data_ptr(), ws.data_ptr(), wsb, st)
    for fn, src in ((lib.mm_sosfiltfilt_ragged_f64, x), (lib.mm_sosfiltfilt_ragged_f32_f64, xf)):
        assert sos(fn, src, ln=None) == INV
        assert sos(fn, src, s=s5) == UNS
        assert sos(fn, src, wsb=need - 1) == WSP
        assert sos(fn, src, nn=21) == INV                    # not even the longest row exceeds padlen
    cs = calc._c_stencil(filters.fir_filtfilt_stencil(_firwin(6)), 19)
    assert lib.mm_stencil_ragged_f64(C.byref(cs), x.data_ptr(), rows, n, n, None, out.data_ptr(), st) == INV
    assert lib.mm_stencil_ragged_f64(C.byref(cs), x.data_ptr(), rows, n, n - 1, lens.data_ptr(), out.data_ptr(), st) == INV
    for fn, src in ((lib.mm_fir_filtfilt_ragged_f64, x), (lib.mm_fir_filtfilt_ragged_f32_f64, xf)):
        assert fn(src.data_ptr(), rows, n, n, None, tab.data_ptr(), 9, out.data_ptr(), n, st) == INV
        assert fn(src.data_ptr(), rows, 27, n, lens.data_ptr(), tab.data_ptr(), 9, out.data_ptr(), n, st) == INV
    sg = lib.mm_savgol_ragged_f64
    assert sg(x.data_ptr(), rows, n, n, None, tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), 21, 4, out.data_ptr(), n, st) == INV
    assert sg(x.data_ptr(), rows, 20, n, lens.data_ptr(), tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), 21, 4, out.data_ptr(),
              n, st) == INV
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert sos() == _lib.MM_OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
