"""CPU: the surface of find_peaks_ex_batch -- signature, exports, scipy's argument errors, the checks mm_find_peaks_ex
makes before any launch -- and ``ref_find_peaks``, the restatement of scipy.signal.find_peaks that the GPU tests use as
their oracle on data with tied heights.  No GPU compute is called here."""
import ctypes as C
import inspect
import itertools
import math
import warnings

import numpy as np
import pytest
import scipy.signal

import modulation_mfcc_amd
from modulation_mfcc_amd import _lib, calc


def _select(prop, bounds):
    """scipy's _select_by_property for a number or a (min, max) pair."""
    pmin, pmax = bounds if isinstance(bounds, (tuple, list)) else (bounds, None)
    keep = np.ones(prop.size, dtype=bool)
    if pmin is not None:
        keep &= pmin <= prop
    if pmax is not None:
        keep &= prop <= pmax
    return keep


def select_by_distance(peaks, heights, distance):
    """scipy's _select_by_peak_distance with the tie rule of find_peaks_ex_batch: peaks are visited from the highest down,
    of equally high ones the LARGER index first (a stable argsort walked from its end); a visited peak that is still kept
    deletes every peak nearer than ``distance``."""
    keep = np.ones(len(peaks), dtype=bool)
    order = np.argsort(heights, kind="stable")
    for j in order[::-1]:
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < distance:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < len(peaks) and peaks[k] - peaks[j] < distance:
            keep[k] = False
            k += 1
    return keep


def ref_find_peaks(x, *, height=None, threshold=None, distance=None, prominence=None, width=None, wlen=None,
                   rel_height=0.5, plateau_size=None):
    """scipy.signal.find_peaks restated: scipy itself for plateau_size / height / threshold, ``select_by_distance``,
    scipy.signal.peak_prominences / peak_widths for the values, scipy's interval filters -- in scipy's order."""
    x = np.asarray(x, dtype=np.float64)
    first = {k: v for k, v in (("plateau_size", plateau_size), ("height", height), ("threshold", threshold))
             if v is not None}
    peaks, props = scipy.signal.find_peaks(x, **first)

    def cut(keep):
        nonlocal peaks, props
        peaks = peaks[keep]
        props = {k: v[keep] for k, v in props.items()}
    if distance is not None:
        cut(select_by_distance(peaks, x[peaks], math.ceil(distance)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", scipy.signal._peak_finding_utils.PeakPropertyWarning)
        if prominence is not None or width is not None:
            props.update(zip(("prominences", "left_bases", "right_bases"),
                             scipy.signal.peak_prominences(x, peaks, wlen=wlen)))
        if prominence is not None:
            cut(_select(props["prominences"], prominence))
        if width is not None:
            data = (props["prominences"], props["left_bases"], props["right_bases"])
            props.update(zip(("widths", "width_heights", "left_ips", "right_ips"),
                             scipy.signal.peak_widths(x, peaks, rel_height, data)))
            cut(_select(props["widths"], width))
    return peaks, props


def assert_same_peaks(got, want, what=""):
    """(peaks, props) pairs equal bit for bit: the same keys, NaNs in the same places."""
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what} peaks")
    assert sorted(got[1]) == sorted(want[1]), (what, sorted(got[1]), sorted(want[1]))
    for k, v in want[1].items():
        np.testing.assert_array_equal(got[1][k], v, err_msg=f"{what} {k}")


def test_signature_and_defaults():
    sig = inspect.signature(calc.find_peaks_ex_batch)
    assert list(sig.parameters) == ["x", "negate", "height", "threshold", "distance", "prominence", "width", "wlen",
                                    "rel_height", "plateau_size", "lo", "hi"]
    assert sig.parameters["x"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "x")
    assert sig.parameters["negate"].default is False and sig.parameters["rel_height"].default == 0.5
    assert all(sig.parameters[k].default is None for k in ("height", "threshold", "distance", "prominence", "width", "wlen",
                                                          "plateau_size", "lo", "hi"))
    assert "larger index" in calc.find_peaks_ex_batch.__doc__.lower()             # the tie rule is stated
    assert "find_peaks_ex_batch" in calc.find_peaks_batch.__doc__ and "not offered" not in calc.find_peaks_batch.__doc__


def test_exports():
    assert "find_peaks_ex_batch" in calc.__all__
    assert modulation_mfcc_amd.find_peaks_ex_batch is calc.find_peaks_ex_batch


X7 = np.array([0.0, 1.0, 0.0, 2.0, 0.0, 1.0, 0.0])


@pytest.mark.parametrize("kw", [dict(distance=0.5), dict(distance=0), dict(distance=-3), dict(prominence=0, wlen=1),
                                dict(prominence=0, wlen=0), dict(width=0, wlen=1.0), dict(width=0, wlen=-2),
                                dict(prominence=0, wlen=0.5), dict(width=0, rel_height=-1),
                                dict(width=(None, 3), rel_height=-0.001)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_argument_errors_are_scipys(kw):
    """The ValueErrors are raised before x is looked at, with the message scipy raises for the same arguments."""
    with pytest.raises(ValueError) as want:
        scipy.signal.find_peaks(X7, **kw)
    with pytest.raises(ValueError) as got:
        calc.find_peaks_ex_batch(X7, **kw)
    assert str(got.value) == str(want.value)


def test_arguments_scipy_accepts_are_accepted():
    """wlen is not looked at without prominence / width, rel_height not without width; per-sample arrays stay a
    TypeError; what is accepted then stops at the host array (TypeError), as find_peaks_batch does."""
    for kw in (dict(wlen=0), dict(wlen=1), dict(rel_height=-1), dict(prominence=0, rel_height=-1), dict(distance=1),
               dict(distance=2.5, plateau_size=(None, 3), width=(1, None), wlen=2.5, rel_height=0)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", scipy.signal._peak_finding_utils.PeakPropertyWarning)
            scipy.signal.find_peaks(X7, **kw)
        with pytest.raises(TypeError, match="CUDA"):
            calc.find_peaks_ex_batch(X7, **kw)
    for kw in (dict(plateau_size=np.ones(3)), dict(width=np.ones(3))):
        with pytest.raises(TypeError, match="per-sample"):
            calc.find_peaks_ex_batch(X7, **kw)
    with pytest.raises(ValueError):
        calc.find_peaks_ex_batch(X7, width=(1, 2, 3))


def _abi_structs():
    o, e = _lib.mm_peaks_opts(), _lib.mm_peaks_ext()
    for f in (o.height, o.threshold, o.prominence, e.plateau_size, e.width):
        f[0], f[1] = -math.inf, math.inf
    e.rel_height = 0.5
    return o, e


BAD_EXT = [("plateau_size_nan", lambda o, e: e.plateau_size.__setitem__(0, math.nan)),
           ("width_nan", lambda o, e: e.width.__setitem__(1, math.nan)),
           ("height_nan", lambda o, e: o.height.__setitem__(0, math.nan)),
           ("distance_0", lambda o, e: (setattr(e, "use_distance", 1), setattr(e, "distance", 0))),
           ("distance_neg", lambda o, e: (setattr(e, "use_distance", 1), setattr(e, "distance", -4))),
           ("wlen_1", lambda o, e: setattr(e, "wlen", 1)),
           ("rel_height_neg", lambda o, e: setattr(e, "rel_height", -0.25)),
           ("rel_height_nan", lambda o, e: setattr(e, "rel_height", math.nan))]


@pytest.mark.parametrize("name,spoil", BAD_EXT, ids=[b[0] for b in BAD_EXT])
def test_invalid_abi_calls(name, spoil):
    """mm_find_peaks_ex refuses these before any launch.  With null device pointers (which alone are refused too), and
    with stand-in addresses that the host never dereferences plus a workspace of 0 bytes: the argument checks come before
    the workspace check, so a sound call stops at MM_ERR_WORKSPACE and a spoilt one at MM_ERR_INVALID_ARG, neither
    touching a device."""
    lib = _lib.load()
    o, e = _abi_structs()
    e.use_width = e.use_plateau_size = 1
    e.use_distance, e.distance, e.wlen = 1, 3, 5
    rows, n, cap = 2, 64, 31
    null = _lib.mm_peaks_out()
    fake = _lib.mm_peaks_out(*([0x1000] * 12))

    def call(out, x, ws):
        return lib.mm_find_peaks_ex(C.byref(o), C.byref(e), x, 1, rows, n, n, None, None, cap, C.byref(out), ws, 0, None)
    assert lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n) > lib.mm_find_peaks_workspace_bytes(rows, n)
    assert call(fake, 0x1000, 0x1000) == _lib.MM_ERR_WORKSPACE
    spoil(o, e)
    assert call(null, None, None) == _lib.MM_ERR_INVALID_ARG
    assert call(fake, 0x1000, 0x1000) == _lib.MM_ERR_INVALID_ARG


def test_abi_workspace_and_required_outputs():
    lib = _lib.load()
    o, e = _abi_structs()
    rows, n = 3, 2051
    old = lib.mm_find_peaks_workspace_bytes(rows, n)
    assert lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), None, rows, n) == old         # ext NULL: mm_find_peaks
    assert lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n) == old   # no condition of ext used
    e.wlen = 9
    assert lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n) == old   # wlen without prominence
    e.use_distance, e.distance = 1, 2
    big = lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n)
    assert big >= old + rows * ((n - 1) // 2) * 44
    assert lib.mm_find_peaks_ex_workspace_bytes(None, C.byref(e), rows, n) == 0
    assert lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), 0, n) == 0
    # width needs the prominence triple
    e.use_width = 1
    out = _lib.mm_peaks_out(*([0x1000] * 12))
    out.lbase = None
    assert lib.mm_find_peaks_ex(C.byref(o), C.byref(e), 0x1000, 1, rows, n, n, None, None, 5, C.byref(out), 0x1000, 0,
                                None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_find_peaks_ex(C.byref(o), C.byref(e), 0x1000, 1, rows, n, n, None, None, 5, None, 0x1000, 0,
                                None) == _lib.MM_ERR_INVALID_ARG


def test_select_by_distance_tie_rule():
    peaks = np.arange(1, 1200, 2)
    ones = np.ones(len(peaks))
    assert peaks[select_by_distance(peaks, ones, 3)].tolist() == list(range(1199, 0, -4))[::-1]
    assert peaks[select_by_distance(peaks, ones, 2)].tolist() == peaks.tolist()
    assert select_by_distance(np.array([1, 3]), np.array([2.0, 1.0]), 3).tolist() == [True, False]


def _walks(seed, rows, n):
    return np.cumsum(np.random.default_rng(seed).standard_normal((rows, n)), axis=1)


GRID = {"plateau_size": [1, (None, 1), (2, None)], "height": [0.0, (-3.0, 8.0)], "threshold": [0.05, (None, 2.0)],
        "distance": [1, 2, 3.5, 40], "prominence": [0, 1.0, (0.5, 6.0)], "width": [0, (1, None), (None, 30), (2.5, 40)]}


def test_reference_restatement_equals_scipy():
    """On tie-free float data (seeded random walks) ref_find_peaks is scipy.signal.find_peaks, bit for bit and key for
    key: each condition alone over its grid, with wlen and rel_height, pairs of conditions, and all six together."""
    x = _walks(41, 4, 700)
    assert all(len(np.unique(r)) == r.size for r in x)
    calls = [{}]
    calls += [{k: v} for k, vs in GRID.items() for v in vs]
    calls += [dict(prominence=0, wlen=w) for w in (2, 3, 4.2, 65, 5000)]
    calls += [dict(width=0, rel_height=h, wlen=w) for h in (0, 0.5, 1.0, 1.5) for w in (None, 21)]
    calls += [{a: GRID[a][-1], b: GRID[b][0]} for a, b in itertools.combinations(GRID, 2)]
    calls += [dict(plateau_size=1, height=(-3.0, 8.0), threshold=0.05, distance=d, prominence=(0.5, 6.0), width=(1, 40),
                   wlen=w, rel_height=h) for d in (2, 7) for w in (None, 31) for h in (0.5, 1.0)]
    found = 0
    for kw in calls:
        for r in x:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", scipy.signal._peak_finding_utils.PeakPropertyWarning)
                want = scipy.signal.find_peaks(r, **kw)
            assert_same_peaks(ref_find_peaks(r, **kw), want, str(kw))
            found += len(want[0])
    assert found > 1000
