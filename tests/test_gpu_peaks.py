"""GPU (-m gpu): find_peaks_batch / MinMaxFinder (csrc/mm_peaks.hip) against scipy.signal.find_peaks itself, the call the
reference's MinMaxFinder makes (script/calc.py:651-686).  Indices, counts and bases are compared with
assert_array_equal, heights / thresholds / prominences for exact equality: they are differences of the same float64
values, so there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from conftest import load_golden
from modulation_mfcc_amd import MfccConfig, MfccPlan, MinMaxFinder, _lib, butter_sos, find_peaks_batch, peaks_to_list
from modulation_mfcc_amd.calc import FIND_PEAKS_SEGMENT as S

pytestmark = pytest.mark.gpu

PROPS = {"height": ("peak_heights",), "threshold": ("left_thresholds", "right_thresholds"),
         "prominence": ("prominences", "left_bases", "right_bases")}


def _check(x, gpu, *, lo=None, hi=None, negate=False, tensor=None, **cond):
    """find_peaks_batch on the rows of x (numpy [rows, n]) == scipy.signal.find_peaks on every row (slice)."""
    import torch
    x = np.asarray(x)
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu) if tensor is None else tensor
    idx, count, props = find_peaks_batch(d, negate=negate, lo=lo, hi=hi, **cond)
    rows, n = x.shape
    cap = max(0, (n - 1) // 2)
    assert idx.dtype == torch.int32 and count.dtype == torch.int32 and tuple(idx.shape) == (rows, cap)
    assert sorted(props) == sorted(k for c in cond for k in PROPS[c])
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    props = {k: v.cpu().numpy() for k, v in props.items()}
    for r in range(rows):
        a = 0 if lo is None else int(np.broadcast_to(np.asarray(lo), (rows,))[r])
        b = n if hi is None else int(np.broadcast_to(np.asarray(hi), (rows,))[r])
        row = x[r, a:max(a, b)].astype(np.float64)
        want, wprops = scipy.signal.find_peaks(-row if negate else row, **cond)
        assert count[r] == len(want), (r, count[r], len(want))
        np.testing.assert_array_equal(idx[r, :count[r]], want, err_msg=f"row {r}")
        assert (idx[r, count[r]:] == -1).all()
        for k, v in wprops.items():
            got = props[k][r]
            assert tuple(got.shape) == (cap,)
            np.testing.assert_array_equal(got[:count[r]], v, err_msg=f"row {r} {k}")
            assert (got[count[r]:] == -1).all() if got.dtype.kind == "i" else np.isnan(got[count[r]:]).all()


@pytest.mark.parametrize("rows", [1, 3, 130])
def test_plateaus_and_compaction(rows, gpu):
    rng = np.random.default_rng(7 + rows)
    for n in (1, 2, 3, 63, 64, 65, S - 1, S, S + 1, 2 * S + 3):
        _check(rng.integers(0, 4, (rows, n)).astype(np.float64), gpu)


def _hand_rows():
    n = 2 * S + 40
    rows = {}
    base = np.zeros(n)
    r = base.copy(); r[S - 3:S + 9] = 1.0                    # straddles the boundary, midpoint in the next segment
    rows["straddle"] = r
    r = base.copy(); r[S - 2:2 * S + 5] = 2.0                # spans a whole segment
    rows["span"] = r
    r = base.copy(); r[:7] = 1.0; r[-9:] = 1.0; r[50] = 3.0  # plateaus touching each end are not peaks
    rows["ends"] = r
    rows["constant"] = np.full(n, 1.5)
    rows["rising"] = np.arange(n, dtype=np.float64)
    rows["falling"] = -np.arange(n, dtype=np.float64)
    rows["alternating"] = (np.arange(n) % 2).astype(np.float64)      # reaches cap = (n - 1) // 2
    r = base.copy(); r[10:20] = 1.0; r[14] = np.nan; r[S:S + 6] = 2.0; r[S + 6] = np.nan; r[300] = 1.0; r[299] = np.nan
    r[400] = 1.0; r[401] = np.nan; r[500] = 1.0
    rows["nan"] = r
    return rows


def test_hand_built_rows(gpu):
    rows = _hand_rows()
    assert len(scipy.signal.find_peaks(rows["straddle"])[0]) == 1 and scipy.signal.find_peaks(rows["straddle"])[0][0] >= S
    n = rows["alternating"].shape[0]
    assert len(scipy.signal.find_peaks(rows["alternating"])[0]) == (n - 1) // 2
    x = np.stack(list(rows.values()))
    _check(x, gpu)
    _check(x, gpu, negate=True)
    _check(x, gpu, prominence=0, threshold=0, height=(None, None))
    small = np.array([[1, np.nan, 1, 3, 1, 2, np.nan, 2, 1], [0, 1, 0, 1, 0, 1, 0, 0, 0]], dtype=np.float64)
    _check(small, gpu)
    _check(small[1:, :7], gpu)


def test_minima_dtype_and_stride(gpu):
    import torch
    rng = np.random.default_rng(11)
    x = np.round(rng.standard_normal((5, S + 77)), 1)
    _check(x, gpu, negate=True)
    _check(x, gpu, negate=True, height=0.5, threshold=(None, 1.0), prominence=(0.3, None))
    x32 = rng.standard_normal((4, 333)).astype(np.float32)
    _check(x32, gpu, prominence=0.1, height=0)
    big = torch.from_numpy(x).to(gpu)
    _check(x[:, 5:205], gpu, tensor=big[:, 5:205], prominence=0)            # row stride > n
    _check(x[1:2, 9:S], gpu, tensor=big[1:2, 9:S])
    one = find_peaks_batch(big[2], prominence=0)                            # 1-D in, 1-D out
    want, wp = scipy.signal.find_peaks(x[2], prominence=0)
    assert one[0].dim() == 1 and one[1].dim() == 0 and one[2]["prominences"].dim() == 1
    np.testing.assert_array_equal(peaks_to_list(one[0], one[1]).cpu().numpy(), want)
    np.testing.assert_array_equal(one[2]["left_bases"].cpu().numpy()[:len(want)], wp["left_bases"])
    lists = peaks_to_list(*find_peaks_batch(big)[:2])
    assert len(lists) == 5
    for r, got in enumerate(lists):
        np.testing.assert_array_equal(got.cpu().numpy(), scipy.signal.find_peaks(x[r])[0])


def test_sub_ranges(gpu):
    import torch
    rng = np.random.default_rng(13)
    n = 2 * S + 3
    x = rng.integers(0, 5, (8, n)).astype(np.float64)
    lo = np.array([0, 5, 100, 100, S - 1, S, 17, n - 2])
    hi = np.array([n, n - 5, 100, 102, S + 2, 2 * S + 1, 20, n])         # empty, 2-sample and 3-sample ranges among them
    _check(x, gpu, lo=lo, hi=hi)
    _check(x, gpu, lo=lo, hi=hi, negate=True, prominence=0, threshold=0, height=(None, 3))
    _check(x, gpu, lo=7)
    _check(x, gpu, hi=S)
    d = torch.from_numpy(x).to(gpu)
    a = find_peaks_batch(d, lo=torch.from_numpy(lo).to(gpu), hi=torch.from_numpy(hi).to(gpu).int(), prominence=1)
    b = find_peaks_batch(d, lo=lo, hi=hi, prominence=1)
    for u, v in zip((a[0], a[1], a[2]["right_bases"]), (b[0], b[1], b[2]["right_bases"])):
        assert torch.equal(u, v)


def test_more_rows_than_one_grid(gpu):
    """Rows beyond the grid's y limit (65 535) take further launches of every kernel: 65 541 rows of 9 samples, tiled
    from 61 distinct rows so that scipy runs once per distinct row."""
    import torch
    rng = np.random.default_rng(29)
    base = rng.integers(0, 3, (61, 9)).astype(np.float64)
    rows = 65541
    pick = np.arange(rows) % 61
    d = torch.from_numpy(base).to(gpu)[torch.from_numpy(pick).to(gpu)]
    idx, count, props = find_peaks_batch(d, prominence=0)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    prom, rb = props["prominences"].cpu().numpy(), props["right_bases"].cpu().numpy()
    for k in range(61):
        want, wp = scipy.signal.find_peaks(base[k], prominence=0)
        sel = pick == k
        assert (count[sel] == len(want)).all()
        assert (idx[sel, :len(want)] == want).all() and (idx[sel, len(want):] == -1).all()
        assert (prom[sel, :len(want)] == wp["prominences"]).all() and (rb[sel, :len(want)] == wp["right_bases"]).all()
    idx2, count2, _ = find_peaks_batch(d, negate=True)
    for k in range(61):
        want = scipy.signal.find_peaks(-base[k])[0]
        sel = pick == k
        assert (count2.cpu().numpy()[sel] == len(want)).all() and (idx2.cpu().numpy()[sel, :len(want)] == want).all()


def test_infinite_plateau_with_threshold(gpu):
    """inf - inf beside the midpoint of an infinite plateau is NaN: numpy's min / max propagate it, so scipy drops the peak
    as soon as one threshold bound is set and keeps it (with NaN thresholds) when both are open."""
    x = np.zeros((2, 40))
    x[0, 5:9] = np.inf; x[0, 20] = 1.0; x[0, 30:32] = np.inf
    x[1, 3] = np.inf; x[1, 10:13] = -1.0; x[1, 25:31] = np.inf
    with np.errstate(invalid="ignore"):
        for thr in (0, (None, 5.0), (0.5, None), (None, None)):
            _check(x, gpu, threshold=thr)
            _check(-x, gpu, negate=True, threshold=thr, height=(None, None))


def test_tensor_ranges_are_clamped(gpu):
    """lo / hi given as device tensors are clamped to 0 <= lo <= hi <= n on the device; heights and thresholds are read
    at the clamped positions too."""
    import torch
    rng = np.random.default_rng(31)
    n = 300
    x = np.round(rng.standard_normal((5, n)), 1)
    lo = np.array([-7, n + 4, 10, 50, -1])
    hi = np.array([n + 9, n + 5, 5, 120, 40])
    d = torch.from_numpy(x).to(gpu)
    idx, count, props = find_peaks_batch(d, lo=torch.from_numpy(lo).to(gpu), hi=torch.from_numpy(hi).to(gpu), height=(None, None),
                                         threshold=0, prominence=0)
    for r in range(5):
        a = min(max(lo[r], 0), n)
        b = min(max(hi[r], a), n)
        want, wp = scipy.signal.find_peaks(x[r, a:b], height=(None, None), threshold=0, prominence=0)
        assert int(count[r]) == len(want)
        np.testing.assert_array_equal(idx[r, :len(want)].cpu().numpy(), want)
        for k, v in wp.items():
            np.testing.assert_array_equal(props[k][r, :len(want)].cpu().numpy(), v, err_msg=k)
    assert int(count[0]) > 0 and int(count[3]) > 0 and int(count[1]) == 0 and int(count[2]) == 0


def _smooth(rng, rows, n):
    x = np.cumsum(rng.standard_normal((rows, n)), axis=1)
    k = np.hanning(9)
    return np.stack([np.convolve(r, k / k.sum(), mode="same") for r in x])


CONDS = [dict(height=0.0), dict(height=(None, 1.0)), dict(height=(-1.0, None)), dict(threshold=0.05),
         dict(threshold=(None, 0.5)), dict(threshold=(0.01, None)), dict(prominence=0.5), dict(prominence=(None, 2.0)),
         dict(prominence=(0.1, None)), dict(height=(-2.0, 3.0), threshold=(0.0, 1.0), prominence=(0.2, 5.0)),
         dict(prominence=(None, None))]


@pytest.mark.parametrize("cond", CONDS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_conditions(cond, gpu, peak_inputs):
    smooth, quant = peak_inputs
    _check(smooth, gpu, **cond)                 # tie-free bases
    _check(quant, gpu, **cond)                  # equal minima: the nearest one is the base
    _check(quant, gpu, negate=True, **cond)


@pytest.fixture(scope="module")
def peak_inputs():
    rng = np.random.default_rng(17)
    smooth = _smooth(rng, 6, S + 301)
    quant = np.round(_smooth(rng, 6, S + 301) * 2) / 2
    return smooth, quant


def test_rising_ramp_with_ripples(gpu):
    """Every left scan of the prominence pass runs to the row start (the stated O(n^2) worst case), n about 3 S."""
    n = 3 * S + 5
    t = np.arange(n, dtype=np.float64)
    x = np.stack([0.01 * t + np.where(t % 4 == 1, 0.5, 0.0), 0.01 * t + 0.3 * np.sin(t)])
    _check(x, gpu, prominence=0)
    _check(x, gpu, prominence=(0.2, None), height=1.0)
    _check(x[:, ::-1], gpu, prominence=0)


def _ref_minmax(x, y, interval, sign):
    """The reference's MinMaxFinder (script/calc.py:651-686), restated with scipy."""
    if interval is None:
        return [], []
    start, end = interval
    keep = [i for i, t in enumerate(x) if start <= t and t <= end]
    ts, vs = np.array([x[i] for i in keep]), np.array([y[i] for i in keep])
    peaks, _ = scipy.signal.find_peaks(sign * vs)
    if len(peaks) == 0:
        return [], []
    return ts[peaks], vs[peaks]


def test_minmaxfinder(gpu, capsys):
    import torch
    rng = np.random.default_rng(19)
    t = np.arange(700) * 0.005
    y = np.round(np.cumsum(rng.standard_normal(700)), 0)
    f = MinMaxFinder()
    for interval in ((0.5, 2.5), (0.0, 10.0), (1.0, 1.0), (0.5, 0.5075), (3.0, 2.0)):
        for name, sign in (("analyse_maximum", 1), ("analyse_minimum", -1)):
            wt, wv = _ref_minmax(t, y, interval, sign)
            for args in ((t, y), (list(t), list(y))):
                gt, gv = getattr(f, name)(*args, interval)
                if len(wt) == 0:
                    assert (gt, gv) == ([], [])
                    continue
                assert isinstance(gt, np.ndarray) and isinstance(gv, np.ndarray)
                np.testing.assert_array_equal(gt, wt)
                np.testing.assert_array_equal(gv, wv)
            dt, dv = getattr(f, name)(torch.from_numpy(t).to(gpu), torch.from_numpy(y).to(gpu), interval)
            if len(wt) == 0:
                assert (dt, dv) == ([], [])
                continue
            assert dt.is_cuda and dv.is_cuda
            np.testing.assert_array_equal(dt.cpu().numpy(), wt)
            np.testing.assert_array_equal(dv.cpu().numpy(), wv)
    ft, fv = f.find_in_interval(t, y, (0.5, 2.5))
    keep = (t >= 0.5) & (t <= 2.5)
    np.testing.assert_array_equal(ft, t[keep])
    np.testing.assert_array_equal(fv, y[keep])
    with pytest.raises(TypeError):
        f.find_in_interval(torch.from_numpy(t).to(gpu), y, (0.5, 2.5))
    capsys.readouterr()
    assert f.analyse_maximum(t, y, None) == ([], []) and f.analyse_minimum(t, y, None) == ([], [])
    assert capsys.readouterr().out == "No interval specified.\n" * 2
    assert f.analyse_maximum(t, np.arange(700.0), (0.5, 2.5)) == ([], [])           # an interval without peaks


def test_end_to_end_change_curve(gpu):
    """The change curve of a golden clip stays on the device from MfccPlan.mfcc_change into find_peaks_batch."""
    import torch
    kw, y, _ = load_golden("c1_am")
    plan = MfccPlan(MfccConfig(**kw))
    m = plan.mfcc(torch.from_numpy(np.stack([y, y[::-1].copy()])).to(gpu))
    sos = butter_sos(2, 0.2)
    curve = plan.mfcc_change(m, sos)
    assert curve.is_cuda and curve.dtype == torch.float64
    host = curve.cpu().numpy()
    for negate in (False, True):
        idx, count, props = find_peaks_batch(curve, negate=negate, prominence=0)
        for r, got in enumerate(peaks_to_list(idx, count)):
            want, wp = scipy.signal.find_peaks(-host[r] if negate else host[r], prominence=0)
            assert len(want) >= 1
            np.testing.assert_array_equal(got.cpu().numpy(), want)
            np.testing.assert_array_equal(props["prominences"][r, :len(want)].cpu().numpy(), wp["prominences"])


def test_arguments_and_capacity(gpu):
    import math
    import torch
    lib = _lib.load()
    rows, n, cap, pad = 3, 2 * S + 3, 5, 4
    x = np.random.default_rng(23).integers(0, 4, (rows, n)).astype(np.float64)
    d = torch.from_numpy(x).to(gpu)
    need = lib.mm_find_peaks_workspace_bytes(rows, n)
    assert need > 0 and lib.mm_find_peaks_workspace_bytes(0, n) == 0 and lib.mm_find_peaks_workspace_bytes(rows, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    o = _lib.mm_peaks_opts()
    for f in (o.height, o.threshold, o.prominence):
        f[0], f[1] = -math.inf, math.inf
    o.use_prominence = 1
    count = torch.full((rows + pad,), -7, dtype=torch.int32, device=gpu)
    idx = torch.full((rows * cap + pad,), -7, dtype=torch.int32, device=gpu)
    lb, rb = idx.clone(), idx.clone()
    prom = torch.full((rows * cap + pad,), -7.0, dtype=torch.float64, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(opts=o, x_ptr=d.data_ptr(), dtype=1, rows_=rows, n_=n, stride=n, cap_=cap, cnt=count.data_ptr(),
             ix=idx.data_ptr(), ws_bytes=need):
        return lib.mm_find_peaks(C.byref(opts), x_ptr, dtype, rows_, n_, stride, None, None, cap_, cnt, ix, prom.data_ptr(),
                                 lb.data_ptr(), rb.data_ptr(), ws.data_ptr(), ws_bytes, st)
    assert call(ws_bytes=need - 1) == _lib.MM_ERR_WORKSPACE
    for bad in (dict(x_ptr=None), dict(dtype=2), dict(rows_=0), dict(n_=0), dict(stride=n - 1), dict(cap_=-1),
                dict(cnt=None), dict(ix=None)):
        assert call(**bad) == _lib.MM_ERR_INVALID_ARG, bad
    nan_opts = _lib.mm_peaks_opts.from_buffer_copy(o)
    nan_opts.height[0] = math.nan
    assert call(opts=nan_opts) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_find_peaks(None, d.data_ptr(), 1, rows, n, n, None, None, cap, count.data_ptr(), idx.data_ptr(),
                             prom.data_ptr(), lb.data_ptr(), rb.data_ptr(), ws.data_ptr(), need, st) == _lib.MM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (count == -7).all() and (idx == -7).all() and (prom == -7).all()        # refused calls wrote nothing
    assert call() == _lib.MM_OK
    torch.cuda.synchronize()
    for r in range(rows):
        want, wp = scipy.signal.find_peaks(x[r], prominence=(None, None))
        assert len(want) > cap and int(count[r]) == len(want)                       # the true count
        sl = slice(r * cap, (r + 1) * cap)
        np.testing.assert_array_equal(idx[sl].cpu().numpy(), want[:cap])            # exactly cap entries
        np.testing.assert_array_equal(prom[sl].cpu().numpy(), wp["prominences"][:cap])
        np.testing.assert_array_equal(lb[sl].cpu().numpy(), wp["left_bases"][:cap])
        np.testing.assert_array_equal(rb[sl].cpu().numpy(), wp["right_bases"][:cap])
    for buf in (count[rows:], idx[rows * cap:], lb[rows * cap:], rb[rows * cap:], prom[rows * cap:]):
        assert (buf == -7).all()                                                    # the padding is untouched
    with pytest.raises(ValueError):
        find_peaks_batch(d, lo=-1)
    with pytest.raises(ValueError):
        find_peaks_batch(d, height=(1, 2, 3))
    with pytest.raises(ValueError):
        find_peaks_batch(d.reshape(1, rows, n))
