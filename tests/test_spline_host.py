"""CPU: the fourth header's symbols exported, bound and prototyped; the refusals of mm_interp_spline_f64 that come before
any launch; the workspace size; the Python refusals that need no device; the yardstick (tests/spline_oracle.py) on its own
fixtures -- a float64 NumPy emulation of the kernels' two systems passes it everywhere, five other interpolants do not."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.interpolate import CubicSpline, PchipInterpolator, make_interp_spline

import spline_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, interp

HEADER = os.path.join(ROOT, "include", "modmfcc_spline.h")


# ---- the fourth header --------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_fourth_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_SPLINE) and len(protos) == 3, set(protos) ^ set(_lib.PROTOTYPES_SPLINE)
    assert not set(protos) & (set(_lib.PROTOTYPES) | set(_lib.PROTOTYPES_MODPSD) | set(_lib.PROTOTYPES_MODCSD))
    assert len(_lib.PROTOTYPES_MODPSD) == 7 and len(_lib.PROTOTYPES_MODCSD) == 4
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_spline.h but not exported"
        res, args = _lib.PROTOTYPES_SPLINE[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert sorted(taking_stream) == ["mm_interp_spline_f64", "mm_interp_spline_ragged_f64"]
    assert lib.mm_version() == 123
    txt = open(HEADER).read()
    assert re.search(r"MM_SPLINE_QUADRATIC\s*=\s*2\s*,\s*MM_SPLINE_CUBIC\s*=\s*3", txt)
    assert (_lib.MM_SPLINE_QUADRATIC, _lib.MM_SPLINE_CUBIC) == (2, 3) and interp._SPLINE_KINDS == {"quadratic": 2, "cubic": 3}


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_spline\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_spline\.h", mk, flags=re.M)
    assert '#include "mm_spline.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()
    src = open(os.path.join(csrc, "mm_spline.hip")).read()
    assert f"kSpChunk = {interp.SPLINE_CHUNK};" in src and '#include "mm_interp_seg.hip.inc"' in src
    assert '#include "mm_interp_seg.hip.inc"' in open(os.path.join(csrc, "mm_interp.hip")).read()


# ---- refusals before any launch -------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null "pointer": every call below must return before it is looked at
MAXN = 0x7fffffff - 1024


def _single(kind=3, x=P, rows=2, n=100, xs=100, y=P, ys=100, ws=P, wb=1 << 40):
    return _lib.load().mm_interp_spline_f64(kind, x, rows, n, xs, y, ys, ws, wb, None)


def _ragged(kind=3, x=P, rows=2, n=100, xs=100, cnt=P, y=P, ys=100, ws=P, wb=1 << 40):
    return _lib.load().mm_interp_spline_ragged_f64(kind, x, rows, n, xs, cnt, y, ys, ws, wb, None)


@pytest.mark.parametrize("call", [_single, _ragged], ids=["single", "ragged"])
@pytest.mark.parametrize("bad", [dict(kind=0), dict(kind=1), dict(kind=4), dict(kind=-1), dict(x=None), dict(y=None),
                                 dict(ws=None), dict(rows=0), dict(rows=-1), dict(n=0), dict(xs=99), dict(ys=99),
                                 dict(n=MAXN + 1, xs=MAXN + 1, ys=MAXN + 1), dict(rows=1 << 31),
                                 dict(rows=1 << 22, n=1 << 20, xs=1 << 20, ys=1 << 20)])
def test_invalid_arguments_are_refused_before_any_launch(call, bad):
    assert call(**bad) == _lib.MM_ERR_INVALID_ARG
    if "kind" in bad or "rows" in bad or "n" in bad:
        d = dict(kind=3, rows=2, n=100)
        d.update({k: v for k, v in bad.items() if k in d})
        assert _lib.load().mm_interp_spline_workspace_bytes(d["kind"], d["rows"], d["n"]) == 0


def test_the_ragged_entry_needs_its_counts():
    assert _ragged(cnt=None) == _lib.MM_ERR_INVALID_ARG


@pytest.mark.parametrize("call", [_single, _ragged], ids=["single", "ragged"])
@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("n", [100, 1026, 1027, 5000])
def test_a_short_workspace_is_refused(call, kind, n):
    need = _lib.load().mm_interp_spline_workspace_bytes(kind, 2, n)
    assert need > 0
    assert call(kind=kind, n=n, xs=n, ys=n, wb=need - 1) == _lib.MM_ERR_WORKSPACE
    assert call(kind=kind, n=n, xs=n, ys=n, wb=0) == _lib.MM_ERR_WORKSPACE


def test_the_workspace_size_is_monotone_and_the_largest_n_has_one():
    f = _lib.load().mm_interp_spline_workspace_bytes
    for kind in (2, 3):
        sizes = [f(kind, 3, n) for n in (1, 2, 3, 40, 1023, 1024, 1025, 1026, 1027, 2048, 2050, 5000, 300001)]
        assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        rows = [f(kind, r, 1001) for r in (1, 2, 3, 64, 1024)]
        assert all(a < b for a, b in zip(rows, rows[1:])), rows
        assert f(kind, 1, MAXN) > 0 and f(kind, 1, MAXN + 1) == 0
        # a row of at most SPLINE_CHUNK unknowns (n - 2) needs no spikes: 20 bytes a sample and the small lists
        assert f(kind, 1, 1026) < 21 * 1026 + 4 * 256 < 36 * 1026 < f(kind, 1, 1027)


# ---- Python, without a device ---------------------------------------------------------------------------------------------------
def test_the_names_are_exported():
    import modulation_mfcc_amd as M
    assert M.interp_nan_spline_batch is interp.interp_nan_spline_batch
    assert M.interp_nan_spline_ragged_batch is interp.interp_nan_spline_ragged_batch
    assert interp.SPLINE_CHUNK == 1024 == O.S == interp.INTERP_SEGMENT
    assert interp._INTERP_HOST_KINDS == ("quadratic", "cubic")         # the old route keeps them


def test_python_refusals():
    import torch
    x = np.ones(10)
    for m in ("linear", "pchip", "slinear", "spline", ""):
        with pytest.raises(ValueError, match="'quadratic' or 'cubic'"):
            interp.interp_nan_spline_batch(x, m)
        with pytest.raises(ValueError, match="'quadratic' or 'cubic'"):
            interp.interp_nan_spline_ragged_batch(x, [10], m)
    for m in O.METHODS:
        for host in (x, torch.ones(10, dtype=torch.float64)):
            with pytest.raises(TypeError, match="CUDA"):
                interp.interp_nan_spline_batch(host, m)
            with pytest.raises(TypeError, match="CUDA"):
                interp.interp_nan_spline_ragged_batch(host.reshape(1, 10), [10], m)


def test_the_error_texts_are_scipys():
    for m in O.METHODS:
        k = O.DEGREE[m]
        for v in range(0, k + 1):
            x = np.full(50, np.nan)
            x[np.arange(v) * 7 + 3] = 1.0 + np.arange(v)
            with pytest.raises(ValueError) as e:
                O.recipe(x, m)
            with pytest.raises(ValueError) as mine:
                interp._spline_refuse(k, v)
            assert str(mine.value) == str(e.value), (m, v)
        interp._spline_refuse(k, k + 1)
        assert not np.isnan(O.recipe(O.chosen(50, k + 1), m)).any()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def _thomas(a, b, c, d):
    b, d = b.copy(), d.copy()
    for i in range(1, len(b)):
        w = a[i] / b[i - 1]
        b[i] -= w * c[i - 1]
        d[i] -= w * d[i - 1]
    x = np.empty(len(b))
    x[-1] = d[-1] / b[-1]
    for i in range(len(b) - 2, -1, -1):
        x[i] = (d[i] - c[i] * x[i + 1]) / b[i]
    return x


def emulate(x, method):
    """The kernels' formulation in float64 NumPy (csrc/mm_spline.hip's header), solved by an unpivoted Thomas sweep."""
    x = np.asarray(x, dtype=np.float64)
    valid = ~np.isnan(x)
    xi, y, t = np.where(valid)[0].astype(np.float64), x[valid], np.where(~valid)[0].astype(np.float64)
    K = len(xi)
    h = np.diff(xi)
    dl = np.diff(y) / h
    hl, hr, l, r = h[:-1], h[1:], dl[:-1], dl[1:]
    j = np.clip(np.searchsorted(xi, t, "right") - 1, 0, K - 2)
    out = x.copy()
    if method == "cubic":
        a, b, c, d = hl.copy(), 2 * (hl + hr), hr.copy(), 6 * (r - l)
        a[0], b[0], c[0], d[0] = 0, hl[0] + 2 * hr[0], hr[0] - hl[0], hr[0] * d[0] / (hl[0] + hr[0])
        c[-1], b[-1], a[-1], d[-1] = 0, hr[-1] + 2 * hl[-1], hl[-1] - hr[-1], hl[-1] * d[-1] / (hl[-1] + hr[-1])
        M = np.empty(K)
        M[1:-1] = _thomas(a, b, c, d)
        M[0] = M[1] + (M[1] - M[2]) * h[0] / h[1]
        M[-1] = M[-2] + (M[-2] - M[-3]) * h[-1] / h[-2]
        s0, s1, hh = t - xi[j], t - xi[j + 1], h[j]
        c3 = (M[j + 1] - M[j]) / (6 * hh)
        left = y[j] + s0 * (dl[j] - hh * (2 * M[j] + M[j + 1]) / 6 + s0 * (M[j] / 2 + s0 * c3))
        right = y[j + 1] + s1 * (dl[j] + hh * (2 * M[j + 1] + M[j]) / 6 + s1 * (M[j + 1] / 2 + s1 * c3))
        out[~valid] = np.where(np.abs(s0) <= np.abs(s1), left, right)
        return out
    first, last = np.arange(K - 2) == 0, np.arange(K - 2) == K - 3
    a, c = np.where(first, 0, 0.5 / hl), np.where(last, 0, 0.5 / hr)
    b = np.where(first, 1 / hl, 1.5 / hl) + np.where(last, 1 / hr, 1.5 / hr)
    d = np.where(first, l / hl, 2 * l / hl) + np.where(last, r / hr, 2 * r / hr)
    m = np.zeros(K + 1)
    m[1:K - 1] = _thomas(a, b, c, d)
    p = np.where(j == 0, 1, np.where(j == K - 2, K - 2, np.where(2 * t <= xi[j] + xi[j + 1], j, j + 1)))
    cp = np.where(p == K - 2, (dl[p] - m[p]) / h[p], (4 * dl[p] - 3 * m[p] - m[p + 1]) / (2 * h[p]))
    s = t - xi[p]
    out[~valid] = y[p] + s * (m[p] + s * cp)
    return out


HOST_NAMES = (["five-knot", "scatter30", "every-second", "sparse40", "alt-1-59", "alt-1-1-1-97", "single-nan", "four-knots",
               "f0-40-1-7", "f0-1023-7-7", "f0-1025-0-1", "knots-1025"])


@pytest.mark.parametrize("method", O.METHODS)
def test_an_unpivoted_float64_solve_of_the_kernels_systems_passes(method):
    worst = 0.0
    for name in HOST_NAMES + O.few_names(method):
        c, b, sp = O.check(emulate(O.fixture(name), method), name, method)
        assert b == 1e-12 or name == "five-knot", (name, b, sp)         # the floor decides on all but the five-knot fixture
        worst = max(worst, c / b)
    assert worst < 1 / 3                                                # the margin's factor of three


def test_the_five_knot_fixture_is_the_one_the_margin_comes_from():
    want, sp, b = O.reference("five-knot", "cubic")
    assert 1e-13 < sp < 1e-12 and b == 16 * sp
    assert O.reference("five-knot", "quadratic")[1] < 1e-12 / 16


def _swap(name, method, values):
    """scipy's row with the NaN samples taken from another interpolant."""
    x = O.fixture(name)
    got = O.reference(name, method)[0].copy()
    nan = np.isnan(x)
    got[nan] = values(np.where(~nan)[0].astype(np.float64), x[~nan], np.where(nan)[0].astype(np.float64))
    return got


@pytest.mark.parametrize("name", ["f0-1023-7-7", "sparse40", "five-knot"])
def test_it_catches_a_natural_spline_and_pchip_in_place_of_not_a_knot(name):
    for wrong in (lambda xi, yi, t: CubicSpline(xi, yi, bc_type="natural")(t), lambda xi, yi, t: PchipInterpolator(xi, yi, extrapolate=True)(t)):
        with pytest.raises(AssertionError, match="beyond the bound"):
            O.check(_swap(name, "cubic", wrong), name, "cubic")


@pytest.mark.parametrize("name", ["f0-1023-7-7", "sparse40", "five-knot"])
def test_it_catches_quadratic_knots_at_the_data_points(name):
    def wrong(xi, yi, t):
        knots = np.r_[[xi[0]] * 3, xi[2:-1], [xi[-1]] * 3]       # K - 3 interior knots, at data points
        return make_interp_spline(xi, yi, k=2, t=knots)(t)
    with pytest.raises(AssertionError, match="beyond the bound"):
        O.check(_swap(name, "quadratic", wrong), name, "quadratic")


@pytest.mark.parametrize("name", ["f0-1023-7-7", "sparse40", "five-knot"])
def test_it_catches_a_knot_list_shifted_by_one(name):
    def cubic(xi, yi, t):
        return make_interp_spline(xi, yi, k=3, t=np.r_[[xi[0]] * 4, xi[1:-3], [xi[-1]] * 4])(t)

    def quadratic(xi, yi, t):
        mid = (xi[1:] + xi[:-1]) / 2
        return make_interp_spline(xi, yi, k=2, t=np.r_[[xi[0]] * 3, mid[:-2], [xi[-1]] * 3])(t)
    for method, wrong in (("cubic", cubic), ("quadratic", quadratic)):
        with pytest.raises(AssertionError, match="beyond the bound"):
            O.check(_swap(name, method, wrong), name, method)


@pytest.mark.parametrize("method", O.METHODS)
@pytest.mark.parametrize("name", ["f0-1023-7-7", "f0-40-1-7", "five-knot"])
def test_it_catches_linear_extrapolation_at_the_ends(name, method):
    x = O.fixture(name)
    got = O.reference(name, method)[0].copy()
    idx = np.where(~np.isnan(x))[0]
    t = np.arange(len(x), dtype=np.float64)
    lo, hi = t < idx[0], t > idx[-1]
    got[lo] = x[idx[0]] + (x[idx[1]] - x[idx[0]]) / (idx[1] - idx[0]) * (t[lo] - idx[0])
    got[hi] = x[idx[-1]] + (x[idx[-1]] - x[idx[-2]]) / (idx[-1] - idx[-2]) * (t[hi] - idx[-1])
    with pytest.raises(AssertionError, match="beyond the bound"):
        O.check(got, name, method)


def test_it_catches_a_nan_and_a_changed_valid_sample():
    for method in O.METHODS:
        want = O.reference("scatter30", method)[0]
        got = want.copy()
        got[np.where(np.isnan(O.fixture("scatter30")))[0][3]] = np.nan
        with pytest.raises(AssertionError, match="beyond the bound"):
            O.check(got, "scatter30", method)
        got = want.copy()
        got[500] += 1e-9
        with pytest.raises(AssertionError, match="beyond the bound"):
            O.check(got, "scatter30", method)
        assert O.check(want, "scatter30", method)[0] == 0.0
