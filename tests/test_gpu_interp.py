"""GPU (-m gpu): interp_NAN's pchip / nearest / nearest-up / previous / next / zero / slinear kinds on the device
(mm_interp_nan_f64) and the articulograph reader's regrid (mm_regrid_linear_f32_f64), csrc/mm_interp.hip, against scipy
itself: the reference's recipes (script/calc.py:345-385 and :173-219) are restated here with scipy.interpolate directly.

Bounds: the kinds that copy values are compared exactly; pchip, slinear and the regrid within 1e-12 of the largest
expected magnitude (per column for the regrid), the bound of the linear kernel in test_gpu_pitch.py."""
import numpy as np
import pytest
import scipy.signal
import torch
from scipy import interpolate

import pyin_oracle as O
from test_interp_host import KINDS, write_pos
from modulation_mfcc_amd import (interp, get_f0, interp_NAN, interp_nan_batch, read_AG50x_arrays, velocity_batch,
                                 find_peaks_batch, peaks_to_list)

pytestmark = pytest.mark.gpu

S = interp.INTERP_SEGMENT
COPYING = ("nearest", "nearest-up", "previous", "next", "zero")
NAN = np.nan


def _dev(y, gpu):
    return torch.from_numpy(np.ascontiguousarray(y)).to(gpu)


def scipy_fill(x, method):
    """script/calc.py:345-385 with scipy: the end fix and PchipInterpolator(extrapolate=False) for 'pchip', otherwise
    interp1d(kind, fill_value='extrapolate') over the valid samples, evaluated at the NaN ones."""
    out = np.array(x, dtype=np.float64, copy=True)
    nans = np.isnan(out)
    if not nans.any():
        return out
    if method == "pchip":
        if nans[0]:
            out[0] = out[np.argwhere(~nans)[0, 0]]
        if nans[-1]:
            out[-1] = out[np.argwhere(~nans)[-1, 0]]
        nans = np.isnan(out)
        f = interpolate.PchipInterpolator(np.where(~nans)[0], out[~nans], extrapolate=False)
    else:
        f = interpolate.interp1d(np.where(~nans)[0], out[~nans], method, fill_value="extrapolate")
    out[nans] = f(np.where(nans)[0])
    return out


def check(got, want, method, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if method in COPYING:
        np.testing.assert_array_equal(got, want, err_msg=what)          # NaN positions included
    else:
        assert not np.isnan(want).any() and not np.isnan(got).any(), what
        err = np.abs(got - want).max()
        assert err <= 1e-12 * np.abs(want).max(), f"{what}: {method} max err {err:.3e}, max |want| {np.abs(want).max():.3e}"


def _nan_curve(n, lead, tail, seed=0):
    rng = np.random.default_rng(seed)
    x = 100 + np.cumsum(rng.standard_normal(n))
    x[rng.random(n) < 0.3] = np.nan
    x[:lead] = np.nan
    if tail:
        x[-tail:] = np.nan
    x[n // 3:n // 3 + 50] = np.nan
    return x


ENDS = [(0, 0), (7, 0), (0, 9), (13, 21)]
_curves = {}


def curves(lead, tail):
    """One single curve and five batch rows (different gap patterns) per end case, with scipy's answers, made once."""
    key = (lead, tail)
    if key not in _curves:
        rows = np.stack([_nan_curve(3001, lead, tail, seed=100 * s + lead + tail) for s in range(6)])
        _curves[key] = (rows, {m: np.stack([scipy_fill(r, m) for r in rows]) for m in KINDS})
    return _curves[key]


def test_device_tensor_never_goes_through_the_host(gpu, monkeypatch):
    x = _nan_curve(500, 3, 4)
    want = scipy_fill(x, "pchip")

    def boom(*a, **k):
        raise AssertionError("interp_NAN took a device tensor to the host")
    monkeypatch.setattr(interp, "_interp_nan_host", boom)
    for method in KINDS:
        got = interp_NAN(_dev(x, gpu), method)
        assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and got.dtype == torch.float64
    check(interp_NAN(_dev(x, gpu), "pchip"), want, "pchip")
    with pytest.raises(AssertionError):
        interp_NAN(_dev(x, gpu), "cubic")                    # the kinds that solve over all knots still do


@pytest.mark.parametrize("lead,tail", ENDS)
@pytest.mark.parametrize("method", KINDS)
def test_kinds_match_scipy(gpu, method, lead, tail):
    rows, want = curves(lead, tail)
    want = want[method]
    single = interp_NAN(_dev(rows[0], gpu), method)
    assert single.shape == (3001,)
    check(single, want[0], method, "single row")
    batch = interp_nan_batch(_dev(rows[1:], gpu), method)
    check(batch, want[1:], method, "batch")
    for r in range(1, 6):                                    # a row of a batch is that row alone, bit for bit
        alone = interp_nan_batch(_dev(rows[r], gpu), method)
        np.testing.assert_array_equal(batch[r - 1].cpu().numpy(), alone.cpu().numpy())
    valid = ~np.isnan(rows)
    np.testing.assert_array_equal(batch.cpu().numpy()[valid[1:]], rows[1:][valid[1:]])     # valid samples pass unchanged


def _border_rows():
    rng = np.random.default_rng(11)

    def base(n):
        return 50 + np.cumsum(rng.standard_normal(n))
    rows = {}
    for n in (S - 1, S, S + 1, 2 * S + 3):
        x = base(n)
        x[rng.random(n) < 0.4] = NAN
        rows[f"random n={n}"] = x
        x = base(n)
        x[rng.random(n) < 0.4] = NAN
        x[:3] = NAN
        x[-2:] = NAN
        rows[f"random, NaN ends, n={n}"] = x
    x = base(3 * S + 7)                                      # a run of S + 5 NaNs that swallows segment 1 whole
    x[S - 3:2 * S + 2] = NAN
    assert np.isnan(x).sum() == S + 5 and np.isnan(x[S:2 * S]).all()
    rows["run of S+5"] = x
    x = base(3 * S)                                          # a gap from the last sample of segment 0, one up to the
    x[S - 1:S + 4] = NAN                                     # first sample of segment 2
    x[2 * S - 4:2 * S + 1] = NAN
    rows["gaps at segment borders"] = x
    x = base(2 * S)                                          # one-sample gaps exactly on either side of a border
    x[S - 1] = NAN
    x[2 * S - 1] = NAN
    rows["gap is the last sample of a segment"] = x
    x = base(2 * S)
    x[S] = NAN
    x[0] = NAN
    rows["gap is the first sample of a segment"] = x
    x = np.full(2 * S + 3, NAN)                              # only two valid samples, both in the last segment
    x[2 * S] = 3.0
    x[2 * S + 2] = -1.0
    rows["two valid in the last segment"] = x
    x = np.full(2 * S + 3, NAN)                              # only the two end samples
    x[0] = -2.0
    x[-1] = 7.0
    rows["valid at 0 and n-1 only"] = x
    x = np.full(3 * S + 1, NAN)                              # three knots, one a segment: neighbours two segments away
    x[5] = 1.0
    x[S + S // 2] = 4.0
    x[3 * S] = 2.0
    rows["one knot per segment"] = x
    return rows


BORDER = _border_rows()


@pytest.mark.parametrize("method", KINDS)
def test_segment_borders(gpu, method):
    for name, x in BORDER.items():
        check(interp_nan_batch(_dev(x, gpu), method), scipy_fill(x, method), method, name)
    same = [x for x in BORDER.values() if len(x) == 2 * S + 3]          # rows of one length as one batch
    got = interp_nan_batch(_dev(np.stack(same), gpu), method)
    check(got, np.stack([scipy_fill(x, method) for x in same]), method, "batch of 2S+3")


def _patterns(n):
    vals = np.array([3.0, -1.5, 4.25, 0.5, 2.0])[:n]
    for bits in range(2 ** n):
        x = vals.copy()
        x[[(bits >> i) & 1 == 1 for i in range(n)]] = NAN
        yield x


@pytest.mark.parametrize("method", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_rows_every_nan_pattern(gpu, method, n):
    """Every NaN pattern of a row of n samples: one valid sample at the start, in the middle, at the end, two adjacent
    ones, no NaN at all -- and the rows scipy refuses, which must raise the same exception type here."""
    seen = 0
    for x in _patterns(n):
        try:
            want = scipy_fill(x, method)
        except Exception as e:                               # all NaN; one valid sample under slinear
            assert isinstance(e, (IndexError, ValueError))
            with pytest.raises(type(e)):
                interp_nan_batch(_dev(x, gpu), method)
            continue
        check(interp_nan_batch(_dev(x, gpu), method), want, method, str(x))
        seen += 1
    assert seen >= 2 ** n - 1 - (n if method == "slinear" else 0)


def test_pchip_shape_cases(gpu):
    cases = {
        "monotone run": [1.0, NAN, 2.0, NAN, NAN, 4.5, NAN, 5.0, NAN, NAN, NAN, 9.0],
        "local extremum": [1.0, NAN, 3.0, NAN, NAN, 5.0, NAN, NAN, 2.0, NAN, 1.0],
        "two equal neighbours": [1.0, NAN, 2.0, NAN, NAN, 2.0, NAN, 4.0, NAN, 4.0, NAN, 3.0],
        # first knot, h0 = h1 = 2, secants m0 = 1, m1 = 10: d = (6 m0 - 2 m1) / 4 < 0 has the other sign -> 0
        "edge: sign of d differs": [0.0, NAN, 2.0, NAN, 22.0, NAN, 23.0],
        # m0 = 1, m1 = -10: d = 6.5 > 3 m0 with secants of different sign -> 3 m0
        "edge: overshoot clipped": [0.0, NAN, 2.0, NAN, -18.0, NAN, -19.0],
        # the same two at the last knot
        "last edge: sign of d differs": [23.0, NAN, 22.0, NAN, 2.0, NAN, 0.0],
        "last edge: overshoot clipped": [-19.0, NAN, -18.0, NAN, 2.0, NAN, 0.0],
        "edge formula kept": [0.0, NAN, 2.0, NAN, 5.0, NAN, 9.0],
        "two knots": [NAN, 1.0, NAN, NAN, 4.0, NAN],
        "end fix makes flat ends": [NAN, NAN, 1.0, NAN, 3.0, NAN, 2.0, NAN, NAN],
    }
    for name, row in cases.items():
        x = np.array(row)
        check(interp_nan_batch(_dev(x, gpu), "pchip"), scipy_fill(x, "pchip"), "pchip", name)
    # the constructed edge cases do hit the corrections they are named for
    h0 = h1 = 2.0
    for m0, m1, expect in ((1.0, 10.0, 0.0), (1.0, -10.0, 3.0), (1.0, 1.5, 0.75)):
        d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
        d = 0.0 if np.sign(d) != np.sign(m0) else (3 * m0 if np.sign(m0) != np.sign(m1) and abs(d) > 3 * abs(m0) else d)
        assert d == expect
    got = interp_nan_batch(_dev(np.array(cases["local extremum"]), gpu), "pchip").cpu().numpy()
    assert got.max() == 5.0                                  # derivative 0 at the extremum: no overshoot
    got = interp_nan_batch(_dev(np.array(cases["two equal neighbours"]), gpu), "pchip").cpu().numpy()
    assert (got[2:6] == 2.0).all() and (got[7:10] == 4.0).all()


def test_nearest_ties(gpu):
    x = np.array([1.0, NAN, 3.0, NAN, NAN, NAN, 7.0, NAN, 9.0, NAN, NAN, NAN, NAN, NAN, 15.0, NAN])
    lo = interp_nan_batch(_dev(x, gpu), "nearest").cpu().numpy()
    up = interp_nan_batch(_dev(x, gpu), "nearest-up").cpu().numpy()
    np.testing.assert_array_equal(lo, [1, 1, 3, 3, 3, 7, 7, 7, 9, 9, 9, 9, 15, 15, 15, 15])
    np.testing.assert_array_equal(up, [1, 3, 3, 3, 7, 7, 7, 9, 9, 9, 9, 15, 15, 15, 15, 15])
    np.testing.assert_array_equal(lo, scipy_fill(x, "nearest"))
    np.testing.assert_array_equal(up, scipy_fill(x, "nearest-up"))
    x = np.full(2 * S + 1, NAN)                              # a tie in the middle of a gap of 2 S - 1 samples
    x[0], x[-1] = 1.0, 2.0
    assert interp_nan_batch(_dev(x, gpu), "nearest")[S].item() == 1.0
    assert interp_nan_batch(_dev(x, gpu), "nearest-up")[S].item() == 2.0


def test_errors(gpu):
    good = _nan_curve(40, 2, 2)
    rows = np.stack([good, np.full(40, NAN), good])
    with pytest.raises(IndexError):
        interp_NAN(_dev(rows, gpu), "pchip")
    with pytest.raises(IndexError):
        interp_nan_batch(_dev(rows[1], gpu), "pchip")
    for method in ("nearest", "nearest-up", "previous", "next", "zero", "slinear"):
        with pytest.raises(ValueError):
            interp_nan_batch(_dev(rows, gpu), method)
        with pytest.raises(ValueError):                      # what scipy raises for it
            scipy_fill(rows[1], method)
    one = np.full(40, NAN)
    one[17] = 2.0
    with pytest.raises(ValueError, match="at least 2 entries"):
        interp_nan_batch(_dev(np.stack([good, one]), gpu), "slinear")
    with pytest.raises(ValueError, match="at least 2 entries"):
        interp_NAN(_dev(one, gpu), "slinear")
    np.testing.assert_array_equal(interp_nan_batch(_dev(one, gpu), "zero").cpu().numpy(), np.full(40, 2.0))
    for method in ("quadratic", "cubic"):
        with pytest.raises(NotImplementedError):
            interp_nan_batch(_dev(good, gpu), method)
    with pytest.raises(ValueError):
        interp_nan_batch(_dev(good, gpu), "akima")
    with pytest.raises(ValueError):
        interp_nan_batch(_dev(np.zeros((2, 3, 4)), gpu), "pchip")
    got = interp_NAN(_dev(good, gpu), "cubic")               # still the host's result, on the device again
    assert got.device.type == "cuda"
    np.testing.assert_array_equal(got.cpu().numpy(), O.interp_NAN(good, "cubic"))
    np.testing.assert_array_equal(interp_nan_batch(_dev(good, gpu), "linear").cpu().numpy(), interp_NAN(good, "linear"))


@pytest.mark.parametrize("method", KINDS)
def test_dtypes_and_strides(gpu, method):
    rows = np.stack([_nan_curve(S + 77, 2, 5, seed=s) for s in range(3)])
    want = interp_nan_batch(_dev(rows, gpu), method)
    got32 = interp_nan_batch(_dev(rows.astype(np.float32), gpu), method)
    assert got32.dtype == torch.float32
    w32 = interp_nan_batch(_dev(rows.astype(np.float32).astype(np.float64), gpu), method).to(torch.float32)
    np.testing.assert_array_equal(got32.cpu().numpy(), w32.cpu().numpy())
    got16 = interp_nan_batch(_dev(rows, gpu).to(torch.bfloat16), method)
    assert got16.dtype == torch.bfloat16 and got16.shape == want.shape
    big = torch.full((3, S + 100), 7.0, dtype=torch.float64, device=gpu)           # a column slice: row stride > n
    big[:, 11:11 + S + 77] = _dev(rows, gpu)
    view = big[:, 11:11 + S + 77]
    assert not view.is_contiguous()
    np.testing.assert_array_equal(interp_nan_batch(view, method).cpu().numpy(), want.cpu().numpy())
    np.testing.assert_array_equal(interp_nan_batch(view[:, ::2], method).cpu().numpy(),
                                  interp_nan_batch(view[:, ::2].contiguous(), method).cpu().numpy())
    assert (big[:, :11] == 7.0).all() and (big[:, 11 + S + 77:] == 7.0).all()
    full = np.arange(12.0).reshape(3, 4)                      # nothing to fill
    np.testing.assert_array_equal(interp_nan_batch(_dev(full, gpu), method).cpu().numpy(), full)


def test_get_f0_pchip_end_to_end(gpu):
    sr = 16000
    y = O.synth("glide", sr, 2.0)
    kw = dict(interpUnvoiced="pchip", outFilter="iir", outFiltCutOff=[12])
    f0, f0t = get_f0(y, sr, method="pyin", **kw)
    wf, wt = O.get_f0(y, sr, **kw)
    assert isinstance(f0, np.ndarray) and f0.shape == wf.shape
    np.testing.assert_array_equal(f0t, wt)
    assert np.abs(f0 - wf).max() <= 1e-9 * np.abs(wf).max()
    d, dt = get_f0(_dev(y, gpu), sr, method="pyin", **kw)
    assert isinstance(d, torch.Tensor) and d.device.type == "cuda"
    np.testing.assert_array_equal(dt, f0t)
    np.testing.assert_array_equal(d.cpu().numpy(), f0)


# ---------------------------------------------------------------------------------------------------------------------
# read_AG50x: the .pos reader and the regrid
# ---------------------------------------------------------------------------------------------------------------------
def _pos_data(n, channels, seed):
    """Records that mix magnitudes: columns of 1e4 + noise, of 1e-3 noise and of plain noise side by side, and every
    fourth column alternating 1e4 + noise with 1e-3 noise from one record to the next, so that the float32 difference of
    two neighbouring samples rounds -- a float64 difference misses the bound."""
    rng = np.random.default_rng(seed)
    cols = 7 * channels
    kind = np.arange(cols) % 4
    walk = rng.standard_normal((n, cols)).cumsum(axis=0)
    data = np.where(kind == 0, 1e4 + walk, np.where(kind == 1, 1e-3 * walk, 30.0 * walk))
    odd = (np.arange(n) % 2 == 1)[:, None]
    data = np.where((kind == 3) & odd, 1e4 + walk, np.where(kind == 3, 1e-3 * walk, data))
    return data.astype(np.float32)


def scipy_read(data, channels, rate, target):
    """script/calc.py:173-219 from the records on: the reference's time axes and interp1d per channel and dimension."""
    pos = data.reshape(len(data), -1, 7)
    original_time = np.linspace(0, len(pos) / rate, len(pos))
    new_time = np.arange(0, original_time[-1], 1 / target)
    out = np.zeros((len(new_time), pos.shape[1], pos.shape[2]))
    for i in range(pos.shape[1]):
        for j in range(pos.shape[2]):
            out[:, i, j] = interpolate.interp1d(original_time, pos[:, i, j], kind="linear", fill_value="extrapolate")(new_time)
    return out, new_time


@pytest.mark.parametrize("target", [200, 1250, 250])
@pytest.mark.parametrize("n", [2, 3, 257])
@pytest.mark.parametrize("channels", [16, 8])
def test_read_ag50x_arrays_matches_interp1d(gpu, tmp_path, channels, n, target):
    data = _pos_data(n, channels, seed=n + channels)
    p = tmp_path / "rec.pos"
    write_pos(p, data, channels, 250)
    a = read_AG50x_arrays(p, target, device=gpu)
    want, wt = scipy_read(data, channels, 250, target)
    ema = a["ema"]
    assert isinstance(ema, torch.Tensor) and ema.device.type == "cuda" and ema.dtype == torch.float64
    assert tuple(ema.shape) == want.shape == (len(wt), channels, 7)
    np.testing.assert_array_equal(a["time"], wt)
    np.testing.assert_array_equal(a["channels"], np.arange(channels))
    assert a["dimensions"] == ["x", "z", "y", "phi", "theta", "rms", "extra"]
    assert a["attrs"] == dict(device="AG50x", duration=wt[-1], original_samplerate=250, resampled_samplerate=target)
    got = ema.cpu().numpy().reshape(len(wt), -1)
    want = want.reshape(len(wt), -1)
    err = np.abs(got - want).max(axis=0)
    bound = 1e-12 * np.abs(want).max(axis=0)
    assert (err <= bound).all(), f"worst column: err {err.max():.3e}, err / max|want| {np.max(err / np.abs(want).max(axis=0)):.3e}"
    if n == 257:                                             # the fixture does tell a float64 difference from a float32 one
        pos = data.astype(np.float64)
        t_in = np.linspace(0, n / 250, n)
        hi = np.clip(np.searchsorted(t_in, wt), 1, n - 1)
        f64 = (pos[hi] - pos[hi - 1]) / (t_in[hi] - t_in[hi - 1])[:, None] * (wt - t_in[hi - 1])[:, None] + pos[hi - 1]
        assert (np.abs(f64 - want).max(axis=0) > bound).any()


def test_read_ag50x_rejects_what_the_reference_rejects(gpu, tmp_path):
    p = tmp_path / "bad.pos"
    write_pos(p, np.zeros((4, 256)), 32, 250)
    with pytest.raises(ValueError):
        read_AG50x_arrays(p, device=gpu)
    write_pos(p, np.zeros((1, 56)), 8, 250)                  # one record: interp1d needs two
    with pytest.raises(ValueError):
        read_AG50x_arrays(p, device=gpu)


def test_read_ag50x_dataset(gpu, tmp_path):
    xr = pytest.importorskip("xarray")
    from modulation_mfcc_amd import read_AG50x
    data = _pos_data(50, 8, seed=1)
    p = tmp_path / "rec.pos"
    write_pos(p, data, 8, 250)
    ds = read_AG50x(p, 200)
    want, wt = scipy_read(data, 8, 250, 200)
    assert isinstance(ds, xr.Dataset) and ds["ema"].dims == ("time", "channels", "dimensions")
    np.testing.assert_array_equal(ds["time"].values, wt)
    assert list(ds["dimensions"].values) == ["x", "z", "y", "phi", "theta", "rms", "extra"]
    assert ds.attrs["device"] == "AG50x" and ds.attrs["original_samplerate"] == 250
    assert np.abs(ds["ema"].values - want).max() <= 1e-12 * np.abs(want).max()


def test_position_velocity_peak_chain_on_the_device(gpu, tmp_path):
    """What the file is read for (script/main.py:1310 on): a channel's z position -> velocity -> its peaks and troughs,
    all on the device, against numpy / scipy on the same regridded column."""
    n, channels = 700, 16
    rng = np.random.default_rng(4)
    data = _pos_data(n, channels, seed=2)
    t = np.arange(n) / 250
    data[:, 3 * 7 + 1] = (10 * np.sin(2 * np.pi * 3 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    p = tmp_path / "rec.pos"
    write_pos(p, data, channels, 250)
    a = read_AG50x_arrays(p, 200, device=gpu)
    z = a["ema"][:, 3, 1]
    zh = z.cpu().numpy()
    vel = velocity_batch(z.contiguous(), 200.0)
    np.testing.assert_array_equal(vel.cpu().numpy(), np.gradient(zh, 1 / 200.0))
    for negate in (False, True):
        idx, count = find_peaks_batch(vel, negate=negate)[:2]
        got = peaks_to_list(idx, count).cpu().numpy()
        want = scipy.signal.find_peaks(-vel.cpu().numpy() if negate else vel.cpu().numpy())[0]
        assert len(want) > 5
        np.testing.assert_array_equal(got, want)


def test_all_ten_methods_a_row_alone_in_a_batch_and_under_full_counts_are_the_same_bits(gpu):
    """Every method of the table on a [3, 1030] float64 batch (a segment border; two chunks of the spline solve) with gaps
    at both ends: interp_nan_batch / interp_nan_spline_batch of a row alone is the row inside the batch, and both are the
    ragged call with full counts, host and device, bit for bit.  (The comparisons with scipy are the tests above, in
    test_gpu_pitch.py and in test_gpu_spline.py.)"""
    from modulation_mfcc_amd import (interp_nan_ragged_batch, interp_nan_spline_batch, interp_nan_spline_ragged_batch)
    n = S + 6
    rows = np.stack([_nan_curve(n, 2 + s, 3 + 2 * s, seed=40 + s) for s in range(3)])
    assert np.isnan(rows[:, 0]).all() and np.isnan(rows[:, -1]).all()

    def same(a, b):                                           # (NaN for NaN: 'previous' and 'next' leave one end unfilled)
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64), b.view(torch.int64))
    x = _dev(rows, gpu)
    assert sorted(interp._METHODS) == sorted(("linear",) + tuple(KINDS) + ("quadratic", "cubic"))
    for method, m in interp._METHODS.items():
        alone, ragged = ((interp_nan_spline_batch, interp_nan_spline_ragged_batch) if m.family is interp._SPLINE else
                         (interp_nan_batch, interp_nan_ragged_batch))
        batch = alone(x, method)
        assert batch.shape == (3, n) and batch.dtype == torch.float64, method
        assert torch.equal(batch[~torch.isnan(x)], x[~torch.isnan(x)]), method
        for r in range(3):
            assert same(alone(x[r], method), batch[r]), (method, r)
        assert same(ragged(x, [n] * 3, method), batch), method
        assert same(ragged(x, torch.full((3,), n, dtype=torch.int64, device=gpu), method), batch), method
