"""GPU (-m gpu): FIR filtfilt and Savitzky-Golay filters of any length on the device -- mm_fir_filtfilt_f64 / _f32_f64 and
mm_savgol_f64 (csrc/mm_longfilt.hip) through fir_filtfilt_batch, savgol_batch, applyFilter, get_velocity and the MFCC-change
tail -- against tests/longfilt_oracle.py, scipy restated in 80-bit long double.

A  FIR sweep      E_dev <= R * max(E_scipy, 2^-52) for every tap count x length x row count x dtype listed below
B  Savitzky-Golay sweep   the same rule: windows x orders x derivatives x lengths, float32 in and out
C  public paths   applyFilter / get_velocity / mfcc_change_device equal the batch functions exactly and never call scipy's
                  filters (the test that fails before this kernel existed); short filters still equal the stencil bit for bit
D  edges          scipy's ValueErrors, strided input, more basis polynomials than one round of the edge kernel, table cache

E = max|y - oracle| / max|oracle| over the checked rows (first and last); E_scipy is scipy's own float64 result on the same
rows.  Boundary lengths come from the kernel: T = filters.LONGFILT_TILE outputs per workgroup, C = filters.LONGFILT_CHUNK taps
per chunk (L = C/2 is the longest filter of one chunk, 2 L - 1 = C - 1 taps; L = C/2 + 1 the shortest of two).

MEASURED (MI355X), worst case per filter over n in {3L+1 | W, T-1, T, T+1, 2T+L | 2T+W}, 3 strided rows, plus 1 and 130 rows
at n = T+1:

    filter              float64: worst at     E_scipy     E_dev  ratio   float32: E_scipy     E_dev  ratio
    fir L=9 lowpass                n=4105    2.73e-16  3.64e-16   1.34            2.53e-16  3.43e-16   1.36
    fir L=16 lowpass             rows=130    2.30e-16  6.27e-16   2.72            1.97e-16  4.95e-16   2.23
    fir L=17 lowpass               n=2049    2.37e-16  5.64e-16   2.38            2.46e-16  4.30e-16   1.74
    fir L=17 highpass                n=52    5.14e-16  4.32e-16   0.84            5.89e-16  3.00e-16   0.51
    fir L=64 lowpass               n=2049    2.19e-16  1.07e-15   4.81            2.11e-16  9.52e-16   4.29
    fir L=65 lowpass             rows=130    2.67e-16  1.53e-15   5.72            2.48e-16  9.41e-16   3.79
    fir L=65 highpass               n=196    1.46e-15  8.97e-16   0.62            1.69e-15  1.08e-15   0.64
    fir L=101 lowpass            rows=130    3.78e-16  1.17e-15   3.08            3.17e-16  6.24e-16   1.97
    fir L=101 highpass           rows=130    4.15e-15  1.72e-15   0.41            1.25e-15  5.78e-16   0.46
    fir L=100 bandpass              n=301    3.82e-16  1.53e-15   4.00            6.57e-16  1.78e-15   2.71
    fir L=301 lowpass              n=4397    6.17e-16  1.58e-15   2.56            4.53e-16  1.21e-15   2.67
    fir L=301 bandpass             n=4397    1.64e-15  5.08e-15   3.10            4.04e-16  1.11e-15   2.74
    sg W=17 p=2            deriv=1 rows=1    1.86e-15  2.17e-15   1.16            3.16e-08  3.16e-08   1.00
    sg W=17 p=3            deriv=1 n=2048    7.32e-15  2.88e-15   0.39            3.16e-08  3.16e-08   1.00
    sg W=17 p=5            deriv=1 n=4113    4.18e-14  7.80e-15   0.19            3.14e-08  3.14e-08   1.00
    sg W=18 p=2              deriv=1 n=18    8.03e-16  3.69e-16   0.46            3.17e-08  3.17e-08   1.00
    sg W=18 p=3            deriv=1 rows=1    2.65e-15  2.13e-15   0.81            3.17e-08  3.17e-08   1.00
    sg W=18 p=5            deriv=1 n=2048    2.95e-14  1.89e-15   0.06            3.15e-08  3.15e-08   1.00
    sg W=64 p=2              deriv=1 n=64    1.67e-16  1.39e-16   0.63            3.25e-08  3.25e-08   1.00
    sg W=64 p=3            deriv=1 n=2047    1.95e-14  3.72e-15   0.19            3.25e-08  3.25e-08   1.00
    sg W=64 p=5              deriv=0 n=64    9.47e-14  2.66e-16   0.00            3.25e-08  3.25e-08   1.00
    sg W=101 p=2         deriv=1 rows=130    2.84e-14  3.97e-15   0.14            3.24e-08  3.24e-08   1.00
    sg W=101 p=3           deriv=1 n=2049    4.17e-15  1.62e-15   0.39            3.24e-08  3.24e-08   1.00
    sg W=101 p=5            deriv=0 n=101    5.12e-10  2.61e-16   0.00            4.75e-08  4.75e-08   1.00
    sg W=257 p=2         deriv=1 rows=130    7.99e-16  2.15e-15   2.69            3.43e-08  3.43e-08   1.00
    sg W=257 p=3           deriv=1 rows=1    1.91e-14  3.73e-15   0.20            3.43e-08  3.43e-08   1.00
    sg W=257 p=5            deriv=0 n=257    1.82e-08  2.72e-16   0.00            4.99e-08  4.99e-08   1.00

(Savitzky-Golay rows: the worst of deriv 0, 1, 2.)  Worst ratio 5.72 (fir L = 65 low-pass, 130 rows); R = 4 x 5.72 = 22.9, rounded
up to a power of two: 32.  A float32 Savitzky-Golay curve is one rounding to float32 (3e-8) in scipy and on the device alike.
scipy's own error over these cases: FIR 2e-16 .. 4e-15; Savitzky-Golay up to 5e-10 (W 101, p 5) and 1.8e-8 (W 257, p 5),
where the device stays at 1e-16 .. 8e-15.
"""
import functools

import numpy as np
import pytest
import scipy.signal

import mfcc_oracle as O
import longfilt_oracle as Q
from conftest import load_golden

pytestmark = pytest.mark.gpu

R_SWEEP = 32.0         # four times the worst measured ratio of sweeps A and B (table above), rounded up to a power of two
EPS = 2.0 ** -52


def _TC():
    from modulation_mfcc_amd import filters
    return filters.LONGFILT_TILE, filters.LONGFILT_CHUNK


T, C = _TC()


def _dev(x, gpu):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.flags.writeable else x.copy()).to(gpu)


def _strided(x, gpu):
    """The rows of x as a device view whose row stride is larger than n."""
    import torch
    xd = _dev(x, gpu)
    buf = torch.full((x.shape[0], x.shape[1] + 5), float("nan"), dtype=xd.dtype, device=gpu)
    buf[:, :x.shape[1]] = xd
    v = buf[:, :x.shape[1]]
    assert v.stride(0) == x.shape[1] + 5
    return v


def _firwin(L, kind):
    cut = [0.06, 0.3] if kind == "bandpass" else 0.24          # 12 Hz at a 100 Hz envelope rate
    return scipy.signal.firwin(L, cut, window=("kaiser", 7.4), pass_zero=kind)


@functools.lru_cache(maxsize=None)
def _rows(n, dtype=np.float64, rows=3):
    x = Q.curve_rows(np.random.default_rng(n + rows), rows, n, dtype)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# A. FIR sweep
# ---------------------------------------------------------------------------------------------------------------------
FIR_CASES = [(9, "lowpass"), (16, "lowpass"), (17, "lowpass"), (17, "highpass"), (C // 2, "lowpass"), (C // 2 + 1, "lowpass"),
             (C // 2 + 1, "highpass"), (101, "lowpass"), (101, "highpass"), (100, "bandpass"), (301, "lowpass"),
             (301, "bandpass")]


def fir_lengths(L):
    return [3 * L + 1, T - 1, T, T + 1, 2 * T + L]


def fir_measure(taps, x, gpu, strided=True):
    """(E_scipy, E_dev) on the first and last row of x."""
    from modulation_mfcc_amd import fir_filtfilt_batch
    sel = [0, x.shape[0] - 1]
    ext = Q.fir_filtfilt_ext_ld(taps, x[sel])
    got = fir_filtfilt_batch(_strided(x, gpu) if strided else _dev(x, gpu), taps)
    assert got.dtype.is_floating_point and got.element_size() == 8 and got.is_cuda and tuple(got.shape) == x.shape
    return Q.rel_err(scipy.signal.filtfilt(taps, 1, x[sel]), ext), Q.rel_err(got.cpu().numpy()[sel], ext)


def fir_points(L, kind):
    """Every (label, x, strided) of one filter: the length family on 3 strided rows, 1 and 130 rows, float32."""
    pts = [(f"n={n}", _rows(n), True) for n in fir_lengths(L)]
    pts.append(("rows=1", _rows(T + 1, rows=1), False))
    pts.append(("rows=130", _rows(T + 1, rows=130), False))
    pts.append(("f32", _rows(T + 1, np.float32), True))
    pts.append(("f32 n=3L+1", _rows(3 * L + 1, np.float32), False))
    return pts


@pytest.mark.parametrize("L,kind", FIR_CASES, ids=[f"L{L}-{k}" for L, k in FIR_CASES])
def test_fir_sweep(L, kind, gpu):
    taps = _firwin(L, kind)
    for label, x, strided in fir_points(L, kind):
        e_ref, e_dev = fir_measure(taps, x, gpu, strided)
        print(f"fir L={L} {kind} {label}: E_scipy {e_ref:.2e} E_dev {e_dev:.2e} ratio {e_dev / max(e_ref, EPS):.2f}")
        assert e_dev <= R_SWEEP * max(e_ref, EPS), (label, e_ref, e_dev)


# ---------------------------------------------------------------------------------------------------------------------
# B. Savitzky-Golay sweep
# ---------------------------------------------------------------------------------------------------------------------
SG_CASES = [(W, p) for W in (17, 18, 64, 101, 257) for p in (2, 3, 5)]
SG_SR = 200.0          # an articulograph channel


def sg_lengths(W):
    return [W, 3 * W + 1, T - 1, T, T + 1, 2 * T + W]


def sg_measure(x, W, p, deriv, delta, gpu, strided=True):
    from modulation_mfcc_amd import savgol_batch
    sel = [0, x.shape[0] - 1]
    ext = Q.savgol_ext_ld(x[sel], W, p, deriv, delta)
    got = savgol_batch(_strided(x, gpu) if strided else _dev(x, gpu), W, p, deriv=deriv, delta=delta)
    assert got.is_cuda and tuple(got.shape) == x.shape
    assert got.cpu().numpy().dtype == x.dtype                   # float32 in, float32 out, as scipy
    want = scipy.signal.savgol_filter(x[sel], W, p, deriv=deriv, delta=delta, mode="interp")
    return Q.rel_err(want, ext), Q.rel_err(got.cpu().numpy()[sel], ext)


def sg_points(W):
    pts = [(f"n={n}", _rows(n), True) for n in sg_lengths(W)]
    pts.append(("rows=1", _rows(T + 1, rows=1), False))
    pts.append(("rows=130", _rows(T + 1, rows=130), False))
    pts.append(("f32", _rows(T + 1, np.float32), True))
    pts.append(("f32 n=W", _rows(W, np.float32), False))
    return pts


@pytest.mark.parametrize("W,p", SG_CASES, ids=[f"W{W}-p{p}" for W, p in SG_CASES])
def test_savgol_sweep(W, p, gpu):
    for deriv in (0, 1, 2):
        for label, x, strided in sg_points(W):
            e_ref, e_dev = sg_measure(x, W, p, deriv, 1 / SG_SR, gpu, strided)
            print(f"sg W={W} p={p} deriv={deriv} {label}: E_scipy {e_ref:.2e} E_dev {e_dev:.2e} "
                  f"ratio {e_dev / max(e_ref, EPS):.2f}")
            assert e_dev <= R_SWEEP * max(e_ref, EPS), (deriv, label, e_ref, e_dev)


@pytest.mark.parametrize("W,p", [(21, 2), (101, 3)])
def test_get_velocity_sg_any_width(W, p, gpu):
    """get_velocity(method='sg') on a device tensor: the reference calls savgol_filter WITHOUT delta (script/calc.py:640), so
    the derivative is per sample whatever sr is -- savgol_batch(delta=1) exactly, and the ratio rule against the oracle."""
    from modulation_mfcc_amd import get_velocity, savgol_batch
    x = _rows(T + 1)
    d = _dev(x, gpu)
    for deriv in (0, 1, 2):
        got = get_velocity(d, SG_SR, deriv, "sg", W, 2, p)
        assert got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), savgol_batch(d, W, p, deriv=deriv, delta=1.0).cpu().numpy())
        ext = Q.savgol_ext_ld(x, W, p, deriv, 1.0)
        e_ref = Q.rel_err(scipy.signal.savgol_filter(x, W, p, deriv=deriv, axis=1, mode="interp"), ext)
        e_dev = Q.rel_err(got.cpu().numpy(), ext)
        print(f"get_velocity W={W} p={p} deriv={deriv}: E_scipy {e_ref:.2e} E_dev {e_dev:.2e}")
        assert e_dev <= R_SWEEP * max(e_ref, EPS)
    one = get_velocity(d[1], SG_SR, 1, "sg", W, 2, p)              # a single curve
    np.testing.assert_array_equal(one.cpu().numpy(), savgol_batch(d, W, p, deriv=1).cpu().numpy()[1])


# ---------------------------------------------------------------------------------------------------------------------
# C. public paths
# ---------------------------------------------------------------------------------------------------------------------
def _public_calls(d, d32):
    """name -> (call through the public function, the same through the batch function)."""
    from modulation_mfcc_amd import applyFilter, fir_filtfilt_batch, get_velocity, savgol_batch
    taps = scipy.signal.firwin(101, 12.0 / 50.0, window=("kaiser", 7.4), pass_zero="lowpass")
    band = scipy.signal.firwin(100, np.array([2.0, 20.0]) / 50.0, window=("kaiser", 7.4), pass_zero="bandpass")
    return {
        "fir101": (lambda: applyFilter(d, 100.0, filt="fir", cutOff=[12], filtLen=101), lambda: fir_filtfilt_batch(d, taps)),
        "fir100band": (lambda: applyFilter(d, 100.0, filt="fir", cutOff=[2, 20], filtLen=100, filtType="band"),
                       lambda: fir_filtfilt_batch(d, band)),
        "fir101_f32": (lambda: applyFilter(d32, 100.0, filt="fir", cutOff=[12], filtLen=101),
                       lambda: fir_filtfilt_batch(d32, taps)),
        "fir_coeffs": (lambda: applyFilter(d, 100.0, filt="fir", cutOff=[12], coeffs=taps[:33] * 2),
                       lambda: fir_filtfilt_batch(d, taps[:33] * 2)),
        "fir_1d": (lambda: applyFilter(d[1], 100.0, filt="fir", cutOff=[12], filtLen=101), lambda: fir_filtfilt_batch(d, taps)[1]),
        "sg51": (lambda: applyFilter(d, 100.0, filt="sg", cutOff=[12], filtLen=51, polyOrd=3), lambda: savgol_batch(d, 51, 3)),
        "sg51_f32": (lambda: applyFilter(d32, 100.0, filt="sg", cutOff=[12], filtLen=51, polyOrd=3),
                     lambda: savgol_batch(d32, 51, 3)),
        "velocity21": (lambda: get_velocity(d, 200.0, 1, "sg", 21, 2, 3), lambda: savgol_batch(d, 21, 3, deriv=1, delta=1.0)),
        "velocity21_f32": (lambda: get_velocity(d32, 200.0, 2, "sg", 21, 2, 2),
                           lambda: savgol_batch(d32, 21, 2, deriv=2, delta=1.0)),
    }


def test_public_paths_equal_the_batch_functions(gpu):
    import torch
    d, d32 = _dev(_rows(T + 1), gpu), _dev(_rows(T + 1, np.float32), gpu)
    for name, (public, batch) in _public_calls(d, d32).items():
        got, want = public(), batch()
        assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, name
        # a float32 curve: 'fir' returns float64 (scipy's filtfilt upcasts), 'sg' keeps float32 (savgol_filter does)
        assert got.dtype == (torch.float32 if name in ("sg51_f32", "velocity21_f32") else torch.float64), name
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=name)


def test_long_filters_stay_on_the_device(gpu, monkeypatch):
    """Before mm_longfilt.hip these calls copied the curves to the host and ran exactly these scipy functions."""
    from modulation_mfcc_amd import calc, filters

    def host(*a, **k):
        raise AssertionError("a device curve went through scipy on the host")
    monkeypatch.setattr(filters._sig, "filtfilt", host)
    monkeypatch.setattr(filters._sig, "savgol_filter", host)
    monkeypatch.setattr(calc, "savgol_filter", host)
    d, d32 = _dev(_rows(T + 1), gpu), _dev(_rows(T + 1, np.float32), gpu)
    for name, (public, _) in _public_calls(d, d32).items():
        y = public()
        assert y.is_cuda and bool(y.isfinite().all()), name


@pytest.mark.parametrize("form", ["clip", "time-major"])
def test_change_tail_long_fir(form, gpu):
    """mfcc_change_device(outFilter='fir', outFiltLen=101) on the refdefault_am golden MFCCs.  The fixture has 201 frames and
    101 taps need more than 303 (there scipy's padlen ValueError comes out, as on the host), so the filtered clips are the
    golden MFCCs followed by their mirror image: 402 frames."""
    from modulation_mfcc_amd import MfccConfig, fir_filtfilt_batch, get_plan, tail
    kw, _, exp = load_golden("refdefault_am")
    plan = get_plan(MfccConfig(**kw))
    mf = exp["mfcc"].astype(np.float32)
    long = np.concatenate([mf, mf[:, ::-1]], axis=1)
    m = _dev(np.stack([long, long[::-1].copy() * 0.5]), gpu)
    args = dict(tStep=0.005, outFilter="fir", outFiltCutOff=[12], outFiltLen=101)
    prev = plan.set_fuse_tail(form == "clip")
    try:
        got = tail.mfcc_change_device(plan, m, **args)
        change = plan.mfcc_change(m, tail.design_lowpass(6, 12, 0.005), None, remove_first=True, diff_method="grad",
                                  out_filter=False)
        with pytest.raises(ValueError, match="greater than padlen, which is 303"):
            tail.mfcc_change_device(plan, _dev(mf[None], gpu), **args)
    finally:
        plan.set_fuse_tail(prev)
    taps = scipy.signal.firwin(101, 12.0 / 100.0, window=("kaiser", 7.4), pass_zero="lowpass")
    np.testing.assert_array_equal(got.cpu().numpy(), fir_filtfilt_batch(change, taps).cpu().numpy())
    for i, mm in enumerate((long, long[::-1] * 0.5)):
        want = O.mfcc_change_tail(mm, **args)
        assert np.abs(got[i].cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()     # test_change_tail_on_device's bound


def test_short_filters_keep_the_stencil_bit_for_bit(gpu):
    """L <= 8 and W <= 16 never reach the new kernels: applyFilter's output is the banded operator's."""
    from modulation_mfcc_amd import applyFilter, calc, filters
    x = _rows(600)
    d = _dev(x, gpu)
    for L in (2, 6, 8):
        taps = scipy.signal.firwin(L, 0.24, window=("kaiser", 7.4))
        want = calc.apply_stencil(d, filters.fir_filtfilt_stencil(taps), 1).cpu().numpy()
        np.testing.assert_array_equal(applyFilter(d, 100.0, filt="fir", cutOff=[12], filtLen=L).cpu().numpy(), want)
        # the long kernel on the same taps agrees to rounding (it is not what applyFilter runs here)
        assert Q.rel_err(filters.fir_filtfilt_batch(d, taps).cpu().numpy(), want) <= 1e-14
    for W, p in ((5, 2), (6, 3), (16, 3)):
        st, passes = calc.velocity_stencil(1.0, 0, "sg", W, 2, p)
        want = calc.apply_stencil(d, st, passes).cpu().numpy()
        np.testing.assert_array_equal(applyFilter(d, 100.0, filt="sg", cutOff=[12], filtLen=W, polyOrd=p).cpu().numpy(), want)
        assert Q.rel_err(filters.savgol_batch(d, W, p).cpu().numpy(), want) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# D. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_scipy_value_errors_before_any_launch(gpu):
    from modulation_mfcc_amd import applyFilter, fir_filtfilt_batch, get_velocity, savgol_batch
    import torch
    for L in (9, 101):
        x = torch.zeros((2, 3 * L), dtype=torch.float64, device=gpu)
        for call in (lambda: fir_filtfilt_batch(x, _firwin(L, "lowpass")),
                     lambda: applyFilter(x, 100.0, filt="fir", cutOff=[12], filtLen=L),
                     lambda: applyFilter(x.float(), 100.0, filt="fir", cutOff=[12], filtLen=L)):
            with pytest.raises(ValueError, match=f"must be greater than padlen, which is {3 * L}"):
                call()
    x = torch.zeros((2, 100), dtype=torch.float64, device=gpu)
    for call in (lambda: savgol_batch(x, 101, 3), lambda: applyFilter(x, 100.0, filt="sg", cutOff=[12], filtLen=101),
                 lambda: get_velocity(x, 200.0, 1, "sg", 101, 2, 3)):
        with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
            call()
    for call in (lambda: savgol_batch(x, 21, 21), lambda: applyFilter(x, 100.0, filt="sg", cutOff=[12], filtLen=21, polyOrd=30)):
        with pytest.raises(ValueError, match="polyorder must be less than window_length"):
            call()
    with pytest.raises(ValueError):
        fir_filtfilt_batch(x, [1.0])
    with pytest.raises(ValueError):
        savgol_batch(torch.zeros((2, 3, 100), dtype=torch.float64, device=gpu), 21, 3)
    with pytest.raises(TypeError):
        fir_filtfilt_batch(x.to(torch.float16), _firwin(9, "lowpass"))


def test_strided_input_through_the_batch_functions(gpu):
    """Non-unit inner stride (every second sample of a wider tensor) and a transposed view: the same as a packed copy."""
    from modulation_mfcc_amd import fir_filtfilt_batch, savgol_batch
    big = _dev(_rows(2 * T + 2), gpu)
    taps = _firwin(C // 2 + 1, "lowpass")
    for view in (big[:, ::2], big.t().contiguous().t()[:, 3:T + 40]):
        assert view.stride(1) != 1
        np.testing.assert_array_equal(fir_filtfilt_batch(view, taps).cpu().numpy(),
                                      fir_filtfilt_batch(view.contiguous(), taps).cpu().numpy())
        np.testing.assert_array_equal(savgol_batch(view, 101, 3, deriv=1).cpu().numpy(),
                                      savgol_batch(view.contiguous(), 101, 3, deriv=1).cpu().numpy())


def test_savgol_more_basis_polynomials_than_one_round(gpu):
    """polyorder + 1 = 81 > 64: the edge kernel takes the basis in two rounds.  The polynomial of degree W - 1 through W
    samples interpolates them, so savgol_filter(deriv=0) is the identity -- edges and interior; 81 + 81 products of
    orthonormal coefficients per output in float64: within 1e-12 of the curve's maximum."""
    from modulation_mfcc_amd import savgol_batch
    for n in (81, 300):
        x = _rows(n)
        got = savgol_batch(_dev(x, gpu), 81, 80).cpu().numpy()
        assert Q.rel_err(got, x) <= 1e-12, Q.rel_err(got, x)


def test_table_cache_is_bounded(gpu):
    from modulation_mfcc_amd import filters, savgol_batch
    d = _dev(_rows(300), gpu)
    first = savgol_batch(d, 21, 2).cpu().numpy()
    for W in range(23, 23 + 2 * (filters.LONGFILT_MAX_TABLES + 2), 2):
        savgol_batch(d, W, 2)
    assert len(filters._LONG_TABLES) <= filters.LONGFILT_MAX_TABLES
    assert not any(k[:2] == ("sg", 21) for k in filters._LONG_TABLES)               # evicted, rebuilt on the next call
    np.testing.assert_array_equal(savgol_batch(d, 21, 2).cpu().numpy(), first)
