"""GPU (-m gpu): find_peaks_ex_batch / mm_find_peaks_ex (csrc/mm_peaks.hip: plateau_size, distance, wlen, width) against
scipy.signal.find_peaks on tie-free data and against ref_find_peaks (test_peaks_ex_host.py: scipy's pieces with the
stated tie rule of the distance condition) on data with tied heights.  Indices, counts and every property are compared
with assert_array_equal -- bit for bit, NaNs in the same places; there is no tolerance in this file."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import scipy.signal

from conftest import load_golden
from modulation_mfcc_amd import MfccConfig, MfccPlan, _lib, butter_sos, find_peaks_batch, find_peaks_ex_batch
from modulation_mfcc_amd.calc import FIND_PEAKS_SEGMENT as S
from test_peaks_ex_host import ref_find_peaks

pytestmark = pytest.mark.gpu

def _scipy(x, **kw):
    return scipy.signal.find_peaks(x, **kw)


def _check(x, gpu, oracle, *, lo=None, hi=None, negate=False, **cond):
    """find_peaks_ex_batch on the rows of x (numpy [rows, n]) == oracle(row or slice, **cond): peaks, the keys of the
    properties, their values and their padding.  Returns the number of peaks compared."""
    import torch
    x = np.asarray(x)
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    idx, count, props = find_peaks_ex_batch(d, negate=negate, lo=lo, hi=hi, **cond)
    rows, n = x.shape
    cap = max(0, (n - 1) // 2)
    assert idx.dtype == torch.int32 and count.dtype == torch.int32 and tuple(idx.shape) == (rows, cap)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    props = {k: v.cpu().numpy() for k, v in props.items()}
    total = 0
    for r in range(rows):
        a = 0 if lo is None else int(np.broadcast_to(np.asarray(lo), (rows,))[r])
        b = n if hi is None else int(np.broadcast_to(np.asarray(hi), (rows,))[r])
        row = x[r, a:max(a, b)].astype(np.float64)
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore", scipy.signal._peak_finding_utils.PeakPropertyWarning)
            want, wprops = oracle(-row if negate else row, **cond)
        what = f"row {r} {cond} lo={a} hi={b} negate={negate}"
        assert count[r] == len(want), (what, count[r], len(want))
        np.testing.assert_array_equal(idx[r, :count[r]], want, err_msg=what)
        assert (idx[r, count[r]:] == -1).all()
        assert sorted(props) == sorted(wprops), (what, sorted(props), sorted(wprops))
        for k, v in wprops.items():
            got = props[k][r]
            assert tuple(got.shape) == (cap,)
            assert got.dtype == (np.int32 if v.dtype.kind == "i" else np.float64), (k, got.dtype)
            np.testing.assert_array_equal(got[:count[r]], v, err_msg=f"{what} {k}")
            assert (got[count[r]:] == -1).all() if got.dtype.kind == "i" else np.isnan(got[count[r]:]).all()
        total += len(want)
    return total


def _same(a, b):
    """torch.equal, NaN padding included (doubles are compared as bit patterns)."""
    import torch
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _walk(seed, rows, n, dtype=np.float64):
    x = np.cumsum(np.random.default_rng(seed).standard_normal((rows, n)), axis=1).astype(dtype)
    assert all(len(np.unique(r)) == r.size for r in x)           # tie-free: scipy's distance selection is defined
    return x


def _ints(seed, rows, n, dtype=np.float64):
    return np.random.default_rng(seed).integers(0, 4, (rows, n)).astype(dtype)


def test_only_the_old_arguments(gpu):
    """With find_peaks_batch's arguments alone the result is find_peaks_batch's, output for output; so is that of the C
    entry with ext = NULL (and of a zeroed ext)."""
    import torch
    n = 2 * S + 3
    x = _ints(3, 4, n)
    d = torch.from_numpy(x).to(gpu)
    lo = torch.tensor([0, 5, S - 1, 100], device=gpu)
    hi = torch.tensor([n, n - 5, 2 * S + 1, 90], device=gpu, dtype=torch.int32)
    for negate in (False, True):
        for kw in (dict(prominence=0), dict(prominence=0, lo=lo, hi=hi), dict(prominence=(1, None), height=1, threshold=0, lo=lo),
                   dict(), dict(prominence=0, wlen=None, rel_height=0.7)):
            old = find_peaks_batch(d, negate=negate, **{k: v for k, v in kw.items() if k not in ("wlen", "rel_height")})
            new = find_peaks_ex_batch(d, negate=negate, **kw)
            assert _same(old[0], new[0]) and _same(old[1], new[1]) and sorted(old[2]) == sorted(new[2])
            assert all(_same(old[2][k], new[2][k]) for k in old[2])
    lib = _lib.load()
    old = find_peaks_batch(d, prominence=0, negate=True, lo=lo, hi=hi)
    rows, cap = 4, (n - 1) // 2
    o = _lib.mm_peaks_opts()
    for f in (o.height, o.threshold, o.prominence):
        f[0], f[1] = -math.inf, math.inf
    o.prominence[0] = 0.0
    o.negate = o.use_prominence = 1
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    lo32 = lo.int()
    zero = _lib.mm_peaks_ext()
    for ext in (None, C.byref(zero)):
        count = torch.zeros(rows, dtype=torch.int32, device=gpu)
        idx, lb, rb = (torch.zeros((rows, cap), dtype=torch.int32, device=gpu) for _ in range(3))
        prom = torch.zeros((rows, cap), dtype=torch.float64, device=gpu)
        need = lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), ext, rows, n)
        assert need == lib.mm_find_peaks_workspace_bytes(rows, n)
        ws = torch.empty(need, dtype=torch.uint8, device=gpu)
        out = _lib.mm_peaks_out(count.data_ptr(), idx.data_ptr(), prom.data_ptr(), lb.data_ptr(), rb.data_ptr())
        assert lib.mm_find_peaks_ex(C.byref(o), ext, d.data_ptr(), 1, rows, n, n, lo32.data_ptr(), hi.data_ptr(), cap,
                                    C.byref(out), ws.data_ptr(), need, st) == _lib.MM_OK
        assert _same(count, old[1]) and _same(idx, old[0]) and _same(prom, old[2]["prominences"])
        assert _same(lb, old[2]["left_bases"]) and _same(rb, old[2]["right_bases"])


ALONE = [dict(plateau_size=1), dict(plateau_size=(2, None)), dict(distance=4), dict(prominence=0, wlen=9), dict(width=1),
         dict(plateau_size=(None, 2), height=(None, None), threshold=(None, 4.0), distance=3, prominence=(0.5, None),
              width=(0.5, 40), wlen=31, rel_height=0.75)]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [3, 64, S - 1, S, S + 1, 2 * S + 3], ids=lambda n: f"n{n}")
def test_each_condition_and_all_six(n, rows, gpu):
    k = np.arange(rows)
    lo, hi = (k * n) // 7, n - (k[::-1] * n) // 5
    total = 0
    for dtype in (np.float64, np.float32):
        walk, ints = _walk(100 + n + rows, rows, n, dtype), _ints(200 + n + rows, rows, n, dtype)
        for cond in ALONE:
            for negate in (False, True):
                for rng in (dict(), dict(lo=lo, hi=hi)):
                    total += _check(walk, gpu, _scipy, negate=negate, **rng, **cond)
                    total += _check(ints, gpu, ref_find_peaks, negate=negate, **rng, **cond)
    assert total > 0 or n == 3


def test_plateau_size(gpu):
    n = 2 * S + 40
    x = _ints(5, 3, n)
    x[0, :7] = 5.0; x[0, -9:] = 5.0                  # plateaus touching each end of the row: not peaks
    x[0, S - 1:S + 1] = 6.0                          # a plateau of two across the sample pair S - 1 | S
    x[1, S - 3:S + 9] = 6.0                          # straddles the boundary, midpoint in the next segment
    x[1, 5] = 7.0
    x[2, S + 500:2 * S + 5] = 6.0                    # edges in different segments
    want = ref_find_peaks(x[0], plateau_size=2)
    at = list(want[0]).index(S - 1)
    assert (want[1]["left_edges"][at], want[1]["right_edges"][at]) == (S - 1, S)
    assert want[0][0] > 6 and want[0][-1] < n - 9
    for ps in (1, (2, None), (None, 3), (2.5, 4), (None, None), (12, 12), (500, None)):
        for negate in (False, True):
            _check(x, gpu, ref_find_peaks, plateau_size=ps, negate=negate)
        _check(x, gpu, ref_find_peaks, plateau_size=ps, lo=[3, S - 1, S + 501], hi=[n - 4, S + 8, n])
        _check(x, gpu, ref_find_peaks, plateau_size=ps, height=1, threshold=0, prominence=0)
    _check(x.astype(np.float32), gpu, ref_find_peaks, plateau_size=(None, 3))


@pytest.mark.parametrize("distance", [1, 2, 3.5, 7, 64, 65, 1500])
def test_distance(distance, gpu):
    """Windows of the distance selection that span no, one and two segment boundaries of the candidate list and of the
    row."""
    n = 3 * S + 5
    walk, ints = _walk(7, 3, n), _ints(9, 3, n)
    assert _check(walk, gpu, _scipy, distance=distance) > 3
    _check(walk, gpu, _scipy, distance=distance, negate=True, height=(None, None))
    _check(ints, gpu, ref_find_peaks, distance=distance)
    _check(ints, gpu, ref_find_peaks, distance=distance, negate=True, lo=[0, 9, S], hi=[n, n - 9, 2 * S + 1])
    _check(walk.astype(np.float32)[:, :S + 1], gpu, _scipy, distance=distance)


def test_distance_ramps_and_equal_peaks(gpu):
    """The worst case of the fixed point: on a rising ramp of 2050 peaks two samples apart, distance=3 lets every round
    decide two peaks, the highest and its neighbour (1025 rounds inside the one launch); the same ramp falling; a row of
    600 equal peaks, where the tie rule decides everything."""
    n = 4101
    up = np.zeros(n)
    up[1::2] = np.arange(1, 2051)
    x = np.stack([up, up[::-1]])
    assert len(scipy.signal.find_peaks(up)[0]) == 2050
    assert _check(x, gpu, _scipy, distance=3) == 2 * 1025
    _check(x, gpu, _scipy, distance=3, prominence=0, width=0)
    equal = np.tile([0.0, 1.0], 600)[None, :]
    for d in (3, 4):
        want = ref_find_peaks(equal[0], distance=d)[0]
        assert want[-1] == 1197 and (np.diff(want) == 4).all()            # the larger index has priority
        _check(equal, gpu, ref_find_peaks, distance=d)
        _check(equal, gpu, ref_find_peaks, distance=d, negate=True)


@pytest.mark.parametrize("wlen", [2, 3, 4, 4.2, 63, 64, 65, 129, 2 * S + 1, 10 ** 6])
def test_wlen(wlen, gpu):
    n = 2 * S + 3
    walk, ints = _walk(13, 3, n), _ints(15, 3, n)
    t = np.arange(n)
    slow = (np.sin(t / 150.0) + 0.01 * np.sin(t * 1.7))[None, :]          # scans that run to the end of the window
    for negate in (False, True):
        _check(walk, gpu, _scipy, prominence=0, wlen=wlen, negate=negate)
        _check(ints, gpu, ref_find_peaks, prominence=0, wlen=wlen, negate=negate)
        _check(slow, gpu, _scipy, prominence=0, wlen=wlen, negate=negate)
    # windows clipped by the slice, not by the row
    lo, hi = [40, S - 20, 700], [n - 40, S + 45, 900]
    _check(walk, gpu, _scipy, prominence=0, wlen=wlen, lo=lo, hi=hi)
    _check(ints, gpu, ref_find_peaks, prominence=(1, None), wlen=wlen, lo=lo, hi=hi)
    _check(walk.astype(np.float32), gpu, _scipy, prominence=(None, 2.0), wlen=wlen)


def _slow_sine(n):
    rng = np.random.default_rng(21)
    t = np.arange(n)
    x = np.stack([np.sin(t / 200.0) + 0.002 * rng.standard_normal(n), np.sin(t / 37.0) + 0.05 * rng.standard_normal(n),
                  np.sin(t / 700.0 + 0.1) + 0.001 * rng.standard_normal(n)])
    assert all(len(np.unique(r)) == r.size for r in x)
    return x


@pytest.mark.parametrize("rel_height", [0, 0.5, 1.0, 1.5])
def test_width(rel_height, gpu):
    n = 2 * S + 3
    slow, walk, ints = _slow_sine(n), _walk(23, 3, n), _ints(25, 3, n)
    # the scans run past 64, 128 and a segment boundary before they meet the bases
    lens, cross = [], False
    for r in slow:
        p, pr = scipy.signal.find_peaks(r, width=0, rel_height=1.0)
        lens += [p - pr["left_ips"], pr["right_ips"] - p]
        cross |= bool(((pr["left_ips"] < S) & (p > S)).any() or ((pr["right_ips"] > S) & (p < S)).any())
    lens = np.concatenate(lens)
    assert ((lens > 64) & (lens < 128)).any() and (lens > 128).any() and cross
    for width in (0, (1, None), (None, 30)):
        for negate in (False, True):
            _check(slow, gpu, _scipy, width=width, rel_height=rel_height, negate=negate)
            _check(ints, gpu, ref_find_peaks, width=width, rel_height=rel_height, negate=negate)
        _check(walk, gpu, _scipy, width=width, rel_height=rel_height, wlen=41)
        _check(walk, gpu, _scipy, width=width, rel_height=rel_height, wlen=300, prominence=1.0)
        _check(slow, gpu, _scipy, width=width, rel_height=rel_height, lo=[30, S - 7, 900], hi=[n - 30, 2 * S, 1700])
        _check(ints, gpu, ref_find_peaks, width=width, rel_height=rel_height, wlen=9, lo=[30, S - 7, 900], hi=[n - 30, 2 * S, 1700])
    _check(walk.astype(np.float32), gpu, _scipy, width=(2, 50), rel_height=rel_height)
    _check(slow.astype(np.float32), gpu, _scipy, width=0, rel_height=rel_height)


def test_width_with_infinities(gpu):
    """A +inf peak (infinite prominence; NaN height of evaluation at rel_height 0) and a -inf sample (an infinite
    prominence for every peak whose base it is): scipy's NaNs and infinities come out in the same places."""
    rng = np.random.default_rng(27)
    x = np.round(np.cumsum(rng.standard_normal((2, 400)), axis=1), 1)
    x[0, 100] = np.inf
    x[0, 250] = -np.inf
    x[1, 50:53] = np.inf
    x[1, 300] = -np.inf
    for rel_height in (0, 0.5, 1.0):
        for kw in (dict(width=0), dict(width=(None, None), prominence=0), dict(width=0, wlen=50), dict(width=(1, None))):
            _check(x, gpu, ref_find_peaks, rel_height=rel_height, **kw)
            _check(x, gpu, ref_find_peaks, rel_height=rel_height, negate=True, **kw)
    want = ref_find_peaks(x[0], width=(None, None), rel_height=0.5)[1]
    assert np.isinf(want["prominences"]).any() and not np.isfinite(want["width_heights"]).all()


def test_capacity_through_the_abi(gpu):
    import torch
    lib = _lib.load()
    rows, n, cap, pad = 3, 2 * S + 3, 5, 4
    x = _ints(23, rows, n)
    d = torch.from_numpy(x).to(gpu)
    o, e = _lib.mm_peaks_opts(), _lib.mm_peaks_ext()
    for f in (o.height, o.threshold, o.prominence, e.plateau_size, e.width):
        f[0], f[1] = -math.inf, math.inf
    o.use_prominence = 1
    e.plateau_size[1] = 3.0
    e.rel_height, e.distance, e.wlen = 0.5, 3, 21
    e.use_plateau_size = e.use_distance = e.use_width = 1
    cond = dict(plateau_size=(None, 3), distance=3, prominence=(None, None), width=(None, None), wlen=21)
    need = lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    count = torch.full((rows + pad,), -7, dtype=torch.int32, device=gpu)
    ints = {k: torch.full((rows * cap + pad,), -7, dtype=torch.int32, device=gpu)
            for k in ("idx", "lbase", "rbase", "plateau_sizes", "left_edges", "right_edges")}
    dbls = {k: torch.full((rows * cap + pad,), -7.0, dtype=torch.float64, device=gpu)
            for k in ("prom", "widths", "width_heights", "left_ips", "right_ips")}
    out = _lib.mm_peaks_out(count=count.data_ptr(), **{k: v.data_ptr() for k, v in {**ints, **dbls}.items()})
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(ext=e, ws_bytes=need, cap_=cap, out_=out):
        return lib.mm_find_peaks_ex(C.byref(o), C.byref(ext), d.data_ptr(), 1, rows, n, n, None, None, cap_, C.byref(out_),
                                    ws.data_ptr(), ws_bytes, st)
    assert call(ws_bytes=need - 1) == _lib.MM_ERR_WORKSPACE
    assert call(ws_bytes=lib.mm_find_peaks_workspace_bytes(rows, n)) == _lib.MM_ERR_WORKSPACE
    bad = _lib.mm_peaks_ext.from_buffer_copy(e)
    bad.wlen = 1
    assert call(ext=bad) == _lib.MM_ERR_INVALID_ARG
    assert call(cap_=-1) == _lib.MM_ERR_INVALID_ARG
    noprom = _lib.mm_peaks_out.from_buffer_copy(out)
    noprom.prom = None
    assert call(out_=noprom) == _lib.MM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (count == -7).all() and all((v == -7).all() for v in {**ints, **dbls}.values())     # refused calls wrote nothing
    assert call() == _lib.MM_OK
    torch.cuda.synchronize()
    names = {"idx": None, "prom": "prominences", "lbase": "left_bases", "rbase": "right_bases"}
    for r in range(rows):
        want, wp = ref_find_peaks(x[r], **cond)
        assert len(want) > cap and int(count[r]) == len(want)                       # the true count
        sl = slice(r * cap, (r + 1) * cap)
        for k, v in {**ints, **dbls}.items():
            w = want if k == "idx" else wp[names.get(k, k)]
            np.testing.assert_array_equal(v[sl].cpu().numpy(), w[:cap], err_msg=k)   # exactly cap entries
    assert (count[rows:] == -7).all()
    for v in {**ints, **dbls}.values():
        assert (v[rows * cap:] == -7).all()                                         # the padding is untouched


def test_more_rows_than_one_grid_staged(gpu):
    """Rows beyond the grid's y limit (65 535) take further launches of every stage kernel but the distance one, whose
    grid is the rows themselves: 65 541 rows of 9 samples, tiled from 61 distinct rows so that the oracle runs once per
    distinct row, under all four staged conditions at once.  Each of them alone drops candidates of these rows, and
    some but not all candidates survive the four together."""
    import torch
    base = np.random.default_rng(29).integers(0, 3, (61, 9)).astype(np.float64)
    rows, cap = 65541, 4
    pick = np.arange(rows) % 61
    cond = dict(plateau_size=(None, 2), distance=3, prominence=(None, 1), width=(None, 3), wlen=5)
    maxima = sum(len(ref_find_peaks(r)[0]) for r in base)
    dropped = [maxima - sum(len(ref_find_peaks(r, **{k: cond[k]})[0]) for r in base)
               for k in ("plateau_size", "distance", "prominence", "width")]
    assert maxima == 110 and dropped == [3, 19, 50, 3]
    # rows 65535 .. 65540, the second launch of each kernel, repeat the distinct rows 21 .. 26: some of their maxima
    # survive, so a wrong first row there shows
    assert list(pick[65535:]) == [21, 22, 23, 24, 25, 26]
    assert sum(len(ref_find_peaks(r)[0]) for r in base[21:27]) == 10
    assert [len(ref_find_peaks(r, **cond)[0]) for r in base[21:27]] == [1, 1, 1, 0, 1, 0]
    d = torch.from_numpy(base).to(gpu)[torch.from_numpy(pick).to(gpu)]
    idx, count, props = find_peaks_ex_batch(d, **cond)
    assert tuple(idx.shape) == (rows, cap) and len(props) == 10
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    props = {k: v.cpu().numpy() for k, v in props.items()}
    kept = empty = 0
    for k in range(61):
        want, wp = ref_find_peaks(base[k], **cond)
        m, sel = len(want), pick == k
        kept += m
        empty += m == 0
        assert (count[sel] == m).all()
        assert (idx[sel, :m] == want).all() and (idx[sel, m:] == -1).all()
        assert sorted(props) == sorted(wp)
        for name, v in wp.items():
            got = props[name][sel]
            if v.dtype.kind == "i":
                assert got.dtype == np.int32 and (got[:, :m] == v).all() and (got[:, m:] == -1).all(), name
            else:                                                  # doubles as bit patterns
                assert got.dtype == np.float64 and not np.isnan(v).any()
                assert (got[:, :m].view(np.int64) == v.astype(np.float64).view(np.int64)).all(), name
                assert np.isnan(got[:, m:]).all(), name
    assert 0 < kept < maxima and (kept, empty) == (63, 12)


def test_end_to_end_change_curve(gpu):
    """The change curve of a golden clip stays on the device from MfccPlan.mfcc_change into find_peaks_ex_batch."""
    import torch
    kw, y, _ = load_golden("c1_am")
    plan = MfccPlan(MfccConfig(**kw))
    m = plan.mfcc(torch.from_numpy(np.stack([y, y[::-1].copy()])).to(gpu))
    curve = plan.mfcc_change(m, butter_sos(2, 0.2))
    assert curve.is_cuda and curve.dtype == torch.float64
    host = curve.cpu().numpy()
    cond = dict(distance=5, width=1, prominence=0, wlen=41)
    idx, count, props = find_peaks_ex_batch(curve, **cond)
    assert all(v.is_cuda for v in (idx, count, *props.values()))
    for r in range(2):
        want, wp = scipy.signal.find_peaks(host[r], **cond)
        assert len(want) >= 1 and int(count[r]) == len(want)
        np.testing.assert_array_equal(idx[r, :len(want)].cpu().numpy(), want)
        assert sorted(props) == sorted(wp)
        for k, v in wp.items():
            np.testing.assert_array_equal(props[k][r, :len(want)].cpu().numpy(), v, err_msg=k)
