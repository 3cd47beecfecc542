"""CPU: the sixth header's symbols exported, bound and prototyped; the unit in both builds; the workspace size; the refusals
of mm_zoom2d_* that come before any launch; scipy's errors from the Python layer; the yardstick (tests/zoom_oracle.py) where
it is defined -- its long-double restatement against scipy on the shapes of tests/test_gpu_zoom.py, which do contain the
cval last column."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.ndimage

import zoom_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, zoom

HEADER = os.path.join(ROOT, "include", "modmfcc_zoom.h")
ENTRIES = ["mm_zoom2d_f32", "mm_zoom2d_f64", "mm_zoom2d_ragged_f32", "mm_zoom2d_ragged_f64"]


# ---- the sixth header ----------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_sixth_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_ZOOM) and len(protos) == 6, set(protos) ^ set(_lib.PROTOTYPES_ZOOM)
    assert not set(protos) & (set(_lib.PROTOTYPES) | set(_lib.PROTOTYPES_MODPSD) | set(_lib.PROTOTYPES_MODCSD)
                              | set(_lib.PROTOTYPES_SPLINE) | set(_lib.PROTOTYPES_LOMB))
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_zoom.h but not exported"
        res, args = _lib.PROTOTYPES_ZOOM[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert sorted(taking_stream) == ENTRIES
    txt = open(HEADER).read()
    assert lib.mm_zoom_version() == int(re.search(r"#define MM_ZOOM_VERSION (\d+)", txt).group(1)) == 100
    assert int(re.search(r"#define MM_ZOOM_SEGMENT (\d+)", txt).group(1)) == _lib.MM_ZOOM_SEGMENT == zoom.ZOOM_SEGMENT
    assert int(re.search(r"#define MM_ZOOM_MAX_TAPS (\d+)", txt).group(1)) == _lib.MM_ZOOM_MAX_TAPS == zoom.ZOOM_MAX_TAPS
    assert re.search(r"MM_ZOOM_CONSTANT\s*=\s*0\s*,\s*MM_ZOOM_MIRROR\s*=\s*1", txt)
    assert re.search(r"MM_ZOOM_PREFILTER\s*=\s*1\s*,\s*MM_ZOOM_DB\s*=\s*2\s*,\s*MM_ZOOM_FILTER_ONLY\s*=\s*4", txt)
    assert zoom._MODE_CODES == {"constant": _lib.MM_ZOOM_CONSTANT, "mirror": _lib.MM_ZOOM_MIRROR}
    assert (zoom._PREFILTER, zoom._DB, zoom._FILTER_ONLY) == (_lib.MM_ZOOM_PREFILTER, _lib.MM_ZOOM_DB, _lib.MM_ZOOM_FILTER_ONLY)
    assert lib.mm_version() == 123                                           # nothing in the other headers changed


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_zoom\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_zoom\.h", mk, flags=re.M)
    assert "Sixteen translation units" in mk and "#   mm_zoom.hip " in mk
    assert '#include "mm_zoom.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()
    src = open(os.path.join(csrc, "mm_zoom.hip")).read()
    assert "kZmSeg = MM_ZOOM_SEGMENT" in src and "#pragma clang fp contract(off)" in src


# ---- the workspace ---------------------------------------------------------------------------------------------------------------
def test_the_workspace_size_is_zero_for_bad_arguments_and_monotone():
    f = _lib.load().mm_zoom2d_workspace_bytes
    good = dict(order=4, images=3, h=129, w=300, ho=774, wo=1800)

    def size(**kw):
        d = dict(good, **kw)
        return f(d["order"], d["images"], d["h"], d["w"], d["ho"], d["wo"])
    assert size() > 0
    for bad in (dict(order=-1), dict(order=6), dict(images=0), dict(images=-2), dict(h=0), dict(w=0), dict(ho=0), dict(wo=0),
                dict(h=-5), dict(w=(1 << 30) + 1, h=1), dict(h=1 << 16, w=1 << 15), dict(ho=1 << 16, wo=1 << 15),
                dict(images=1 << 31), dict(images=1 << 20, ho=1 << 12, wo=1 << 12)):
        assert size(**bad) == 0, bad
    for order in range(6):
        ws = [size(order=order, w=w) for w in (1, 2, 59, 127, 128, 129, 300, 30001)]
        assert all(a > 0 for a in ws) and all(a <= b for a, b in zip(ws, ws[1:])), ws
        hs = [size(order=order, h=h) for h in (1, 2, 129, 257, 1025)]
        assert all(a <= b for a, b in zip(hs, hs[1:])) and hs[0] < hs[-1], hs
        bs = [size(order=order, images=b) for b in (1, 2, 64, 1024)]
        assert all(a < b for a, b in zip(bs, bs[1:])), bs
    # a float64 plane of the input per filtered stage: one for orders 0 and 1, two from order 2 on
    assert 129 * 300 * 3 * 8 <= size(order=1) < size(order=2) <= 2 * (129 * 300 * 3 * 8 + 256)
    assert size(ho=1, wo=1) == size(ho=5000, wo=5000)                      # the output is the caller's


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null, 256-byte aligned "pointer": every call below must return before it is looked at


def _single(f32=False, order=3, mode=0, cval=0.0, flags=1, x=P, b=2, h=10, w=20, xi=200, xr=20, ho=20, wo=40, y=P, yi=800,
            yr=40, ws=P, wb=1 << 40):
    fn = _lib.load().mm_zoom2d_f32 if f32 else _lib.load().mm_zoom2d_f64
    return fn(order, mode, cval, flags, x, b, h, w, xi, xr, ho, wo, y, yi, yr, ws, wb, None)


def _ragged(f32=False, order=3, mode=0, cval=0.0, flags=1, x=P, b=2, h=10, w=20, xi=200, xr=20, wd=P, zx=2.0, ho=20, wo=40,
            y=P, yi=800, yr=40, ws=P, wb=1 << 40):
    fn = _lib.load().mm_zoom2d_ragged_f32 if f32 else _lib.load().mm_zoom2d_ragged_f64
    return fn(order, mode, cval, flags, x, b, h, w, xi, xr, wd, zx, ho, wo, y, yi, yr, ws, wb, None)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("call", [_single, _ragged], ids=["single", "ragged"])
def test_bad_orders_modes_and_sizes_are_refused_before_any_launch(call, f32):
    for bad in (dict(order=-1), dict(order=6), dict(order=17), dict(mode=2), dict(mode=-1)):
        assert call(f32=f32, **bad) == _lib.MM_ERR_UNSUPPORTED, bad
    for bad in (dict(x=None), dict(y=None), dict(b=0), dict(b=-1), dict(h=0), dict(w=0), dict(ho=0), dict(wo=0), dict(h=-3),
                dict(xr=19), dict(yr=39), dict(xi=199), dict(yi=799), dict(flags=8), dict(flags=-1),
                dict(flags=1 | 4),                                            # filter only: the output has the input's size
                dict(h=1 << 16, w=1 << 15, xr=1 << 15, xi=1 << 31), dict(ho=1 << 16, wo=1 << 15, yr=1 << 15, yi=1 << 31),
                dict(b=1 << 31)):
        assert call(f32=f32, **bad) == _lib.MM_ERR_INVALID_ARG, bad
    assert call(f32=f32, flags=1 | 4, ho=10, wo=20, yi=200, yr=20, ws=None) == _lib.MM_ERR_WORKSPACE     # (admitted that far)
    need = _lib.load().mm_zoom2d_workspace_bytes(3, 2, 10, 20, 20, 40)
    assert need > 0
    for bad in (dict(ws=None), dict(wb=need - 1), dict(wb=0), dict(ws=P + 8)):
        assert call(f32=f32, **bad) == _lib.MM_ERR_WORKSPACE, bad


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_ragged_entry_needs_its_widths_and_a_positive_zoom(f32):
    assert _ragged(f32=f32, wd=None) == _lib.MM_ERR_INVALID_ARG
    for zx in (0.0, -1.0, float("nan"), float("inf")):
        assert _ragged(f32=f32, zx=zx) == _lib.MM_ERR_INVALID_ARG


# ---- Python, without a device ---------------------------------------------------------------------------------------------------
def test_the_names_are_exported():
    import modulation_mfcc_amd as M
    for name in ("zoom_batch", "zoom_ragged_batch", "spline_filter_batch", "spectrogram_image", "spectrogram_image_batch"):
        assert getattr(M, name) is getattr(zoom, name)
    assert zoom.ZOOM_MODES == O.MODES
    for n, z in ((5, 1.5), (8, 2.5), (59, 6), (129, 6), (7, 1.3), (10, 0.5), (63, 2.5)):
        assert zoom.zoom_output_size(n, z) == scipy.ndimage.zoom(np.zeros(n), z, order=0).shape[0] == O.out_size(n, z)
    assert zoom.zoom_output_size(5, 1.5) == 8                               # ties to even


def _raised(f):
    with pytest.raises(Exception) as e:
        f()
    return type(e.value), str(e.value)


def test_the_python_layer_raises_what_scipy_raises():
    x = np.ones((4, 5))
    for kw in (dict(zoom=(1, 2, 3)), dict(zoom=(2,)), dict(zoom=2, order=2.5), dict(zoom=2, order=3.0), dict(zoom=2, order=6),
               dict(zoom=2, order=-1), dict(zoom=2, order=7.5), dict(zoom=2, mode="foo"), dict(zoom=2, order="3")):
        want = _raised(lambda: scipy.ndimage.zoom(x, **kw))
        assert _raised(lambda: zoom.zoom_batch(x, **kw)) == want, (kw, want)
        kw = dict(kw)
        assert _raised(lambda: zoom.zoom_ragged_batch(x[None], [5], kw.pop("zoom"), **kw)) == want, (kw, want)
    for order in (0, 1, 6, -1, 1.5):
        want = _raised(lambda: scipy.ndimage.spline_filter(x, order=order))
        assert want == (RuntimeError, "spline order not supported")
        assert _raised(lambda: zoom.spline_filter_batch(x, order)) == want, order
    assert _raised(lambda: zoom.spline_filter_batch(x, 2.5))[0] is TypeError
    for mode in ("nearest", "reflect", "wrap", "grid-mirror", "grid-wrap", "grid-constant"):
        scipy.ndimage.zoom(x, 2, mode=mode)                                 # scipy has it
        with pytest.raises(NotImplementedError, match="'constant' and 'mirror'"):
            zoom.zoom_batch(x, 2, mode=mode)
    with pytest.raises(NotImplementedError, match="grid_mode"):
        zoom.zoom_batch(x, 2, grid_mode=True)
    # arguments scipy admits come as far as the device check
    import torch
    for host in (x, torch.ones(4, 5, dtype=torch.float64)):
        for f in (lambda: zoom.zoom_batch(host, 2), lambda: zoom.zoom_batch(host, (1.5, 2.5), order=np.int64(4), mode="mirror"),
                  lambda: zoom.spline_filter_batch(host, 5), lambda: zoom.spectrogram_image(host),
                  lambda: zoom.spectrogram_image_batch(host), lambda: zoom.zoom_ragged_batch(host, [5], 2)):
            with pytest.raises(TypeError, match="CUDA"):
                f()
    assert zoom.spectrogram_image(x, zoom_blur=False) is x
    doc = " ".join((zoom.__doc__ + zoom.zoom_batch.__doc__).split())
    assert "Finite inputs only" in doc and "every output whose taps touch" in doc
    assert "Finite inputs only" in open(HEADER).read()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def test_longdouble_is_wider_and_the_bound_is_the_familys():
    assert np.finfo(np.longdouble).eps < 1e-18 and (O.FLOOR, O.MARGIN, O.CEILING) == (1e-12, 16.0, 1e-10)
    assert O.bound_of(0.0) == 1e-12 and O.bound_of(1e-13) == 16e-13
    assert O.bound_of(0.0, np.float32, 100.0) == 1e-12 + float(np.spacing(np.float32(100.0))) / 100.0
    with pytest.raises(AssertionError, match="ill-conditioned"):
        O.bound_of(1e-11)


SHAPES = [((7, 59), 6), ((5, 129), 6), ((5, 8), (1.5, 2.5)), ((6, 63), 2.5), ((6, 64), 2.5), ((9, 11), 1.3), ((12, 10), 0.5),
          ((4, 5), 1.0), ((1, 7), 3), ((7, 1), 3), ((2, 2), 6), ((3, 3), 2), ((1, 1), 4)]


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("order", O.ORDERS)
def test_the_restatement_equals_scipy_on_the_test_shapes(order, mode):
    worst = 0.0
    for (h, w), z in SHAPES:
        for cval in (0.0, -7.5):
            x = O.image(h, w)
            exact, outside = O.restate(x, z, order, mode, cval)
            want = O.scipy_zoom(x, z, order, mode, cval)
            worst = max(worst, O.measure(exact.astype(np.float64), want))
            assert (want[outside] == cval).all()
            if cval != 0.0:
                assert ((want == cval) == outside).all(), "scipy returns cval exactly where the restatement says"
            # the yardstick admits scipy itself and the restatement rounded to float64
            O.check(want, x, z, order, mode, cval)
            O.check(exact.astype(np.float64), x, z, order, mode, cval)
    assert worst <= 1e-12, worst
    x = O.image(7, 59)
    a = O.restate(x, 6, order, mode, prefilter=False)[0].astype(np.float64)
    assert O.measure(a, O.scipy_zoom(x, 6, order, mode, prefilter=False)) <= 1e-12


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_the_restated_prefilter_equals_scipys(order):
    for h, w in ((7, 59), (129, 5), (1, 5), (5, 1), (2, 2), (3, 300), (2, 65)):
        x = O.image(h, w)
        want = scipy.ndimage.spline_filter(x, order=order, mode="mirror")
        assert O.measure(O.spline_filter2(x, order).astype(np.float64), want) <= 1e-12
        assert scipy.ndimage.spline_filter(x, order=order, mode="constant").tobytes() == want.tobytes()
        O.check_filter(want, x, order)


def test_the_shapes_contain_the_cval_last_column():
    """59 x 6 rounds one ulp past the last sample, 129 x 6 does not: the GPU tests cannot pass by never meeting the quirk."""
    for n, z, quirk in ((59, 6, True), (129, 6, False), (63, 2.5, True), (64, 2.5, True), (29, 3, True), (50, 3, True),
                        (101, 3, True)):
        outside = O.axis_plan(n, O.out_size(n, z), 4, "constant")[0]
        assert outside[:-1].sum() == 0 and bool(outside[-1]) == quirk, (n, z)
        assert not O.axis_plan(n, O.out_size(n, z), 4, "mirror")[0].any()
        got = scipy.ndimage.zoom(np.ones((3, n)), (1, z), order=4, cval=-7.5)
        assert (got[:, -1] == -7.5).all() == quirk and (got[:, :-1] != -7.5).all()


def test_it_catches_wrong_results():
    x = O.image(7, 59)
    want = O.scipy_zoom(x, 6, 4, cval=-7.5)
    for wrong in (O.scipy_zoom(x, 6, 3, cval=-7.5), O.scipy_zoom(x, 6, 4, cval=-7.5, prefilter=False),
                  O.scipy_zoom(x, 6, 4, "mirror", cval=-7.5), want * (1 + 1e-9)):
        with pytest.raises(AssertionError):
            O.check(wrong, x, 6, 4, cval=-7.5)
    got = want.copy()
    got[3, 5] = np.nan
    with pytest.raises(AssertionError, match="beyond the bound"):
        O.check(got, x, 6, 4, cval=-7.5)
    got = want.copy()
    got[:, -1] = np.nextafter(-7.5, 0)                                       # a last column that is cval but for one ulp
    with pytest.raises(AssertionError, match="bit for bit"):
        O.check(got, x, 6, 4, cval=-7.5)
    with pytest.raises(AssertionError):
        O.check(want.astype(np.float32), x, 6, 4, cval=-7.5)                # the dtype is part of the check
    assert O.check(want, x, 6, 4, cval=-7.5)[0] == 0.0
