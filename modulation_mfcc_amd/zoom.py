"""The B-spline zoom of 2-D feature images on the device (csrc/mm_zoom.hip, include/modmfcc_zoom.h).

    zoom_batch(x, zoom, order=3, mode='constant', cval=0.0, prefilter=True)  -> scipy.ndimage.zoom on the last two axes
    zoom_ragged_batch(x, widths, zoom, ...)                                  -> the same with a width per image
    spline_filter_batch(x, order)                                            -> scipy.ndimage.spline_filter(mode='mirror')
    spectrogram_image(spect_data, zoom_blur=True)                            -> script/praat_py_ui/spectrogram.py:70-71
    spectrogram_image_batch(power, zoom=6, order=4, db=True)                 -> the same with 10 log10 in front, batched

``x`` is a CUDA(HIP) tensor [H, W] or [B, H, W], float32 or float64; the result has its type and is scipy's within a few of
scipy's own roundings (the yardstick of tests/test_gpu_zoom.py), not bit for bit -- but where scipy returns ``cval`` the
result is ``cval`` exactly, the last row or column included when its coordinate rounds one ulp past the last sample (a
width of 59 at zoom 6).  All arithmetic is float64; a float32 result is the float64 result rounded once, as in scipy.

Finite inputs only.  In scipy ONE Inf or NaN sample (log10 of a zero) makes the whole image non-finite through the
prefilter's recursions.  Here the prefilter is applied as its impulse response, and the sample reaches its support (at most
88 samples each way) and no further: every output whose taps touch the sample is non-finite, nothing is promised about the
rest.  There is no host fallback.
"""
from __future__ import annotations

import operator

import numpy as np

from . import ragged

__all__ = ["zoom_batch", "zoom_ragged_batch", "spline_filter_batch", "spectrogram_image", "spectrogram_image_batch",
           "zoom_output_size", "ZOOM_SEGMENT", "ZOOM_MAX_TAPS", "ZOOM_MODES"]

ZOOM_SEGMENT = 128          # columns a workgroup of the horizontal prefilter owns (MM_ZOOM_SEGMENT of include/modmfcc_zoom.h)
ZOOM_MAX_TAPS = 80          # the longest one-sided impulse response of a prefilter (MM_ZOOM_MAX_TAPS)
ZOOM_MODES = ("constant", "mirror")
_MODE_CODES = {"constant": 0, "mirror": 1}                                   # MM_ZOOM_CONSTANT / MM_ZOOM_MIRROR
_SCIPY_MODES = ("nearest", "wrap", "reflect", "grid-mirror", "mirror", "constant", "grid-wrap", "grid-constant")
_PREFILTER, _DB, _FILTER_ONLY = 1, 2, 4                                      # MM_ZOOM_PREFILTER / _DB / _FILTER_ONLY

# scipy.ndimage's own texts
_MSG_ORDER = "spline order not supported"
_MSG_RANK = "sequence argument must have length equal to input rank"
_MSG_MODE = "boundary mode not supported"
_MSG_NEGATIVE = "negative dimensions are not allowed"


def _order(order, least=0):
    if order < least or order > 5:                                          # (a str raises Python's TypeError, as in scipy)
        raise RuntimeError(_MSG_ORDER)
    return operator.index(order)            # TypeError: 'float' object cannot be interpreted as an integer


def _mode(mode, grid_mode=False):
    if grid_mode:
        raise NotImplementedError("grid_mode=True is not built; grid_mode=False with mode 'constant' or 'mirror' is")
    if mode in _MODE_CODES:
        return _MODE_CODES[mode]
    if mode in _SCIPY_MODES:
        raise NotImplementedError(f"mode {mode!r} is not built: the modes built are 'constant' and 'mirror' ('nearest', "
                                  "'reflect', 'wrap' and the grid- modes initialise their prefilter in scipy's own way)")
    raise RuntimeError(_MSG_MODE)


def _zoom_pair(zoom):
    if isinstance(zoom, (str, bytes)) or not hasattr(zoom, "__iter__"):
        return zoom, zoom
    z = list(zoom)
    if len(z) != 2:
        raise RuntimeError(_MSG_RANK)
    return z[0], z[1]


def zoom_output_size(n, zoom):
    """scipy's output length of an axis of n samples: round(n * zoom), ties to even (5 x 1.5 -> 8)."""
    return int(round(n * zoom))


def _images(x, who):
    import torch
    if not ragged.is_device_tensor(x):
        raise TypeError(f"{who} takes a CUDA(HIP) tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who} takes float32 or float64 images, got {x.dtype}")
    if x.dim() not in (2, 3):
        raise ValueError(f"{who} takes an image [H, W] or a batch [B, H, W], got {tuple(x.shape)}")
    single = x.dim() == 2
    x3 = x.unsqueeze(0) if single else x
    if x3.shape[1] < 1 or x3.shape[2] < 1:
        raise ValueError(f"{who}: an image needs a row and a column, got {tuple(x.shape)}")
    b, h, w = x3.shape
    si, sr, sc = x3.stride()
    if (w > 1 and sc != 1) or (h > 1 and sr < w) or (b > 1 and si < (h - 1) * sr + w):
        x3 = x3.contiguous()
    return x3, single


def _strides(t):
    b, h, w = t.shape
    sr = t.stride(1) if h > 1 else w
    si = t.stride(0) if b > 1 else (h - 1) * sr + w
    return si, sr


def _run(x3, widths, zoom_x, order, mode, cval, flags, h_out, w_out):
    import torch
    from . import _lib
    b, h, w = x3.shape
    dev = x3.device
    out = torch.empty((b, h_out, w_out), dtype=x3.dtype, device=dev)
    if b == 0 or h_out == 0 or w_out == 0:
        return out
    need = int(_lib.load().mm_zoom2d_workspace_bytes(order, b, h, w, h_out, w_out))
    if need == 0:
        raise ValueError(f"zoom: {b} images of {h} x {w} to {h_out} x {w_out} are beyond the kernel's limits")
    ws = _lib.workspace(need, dev)
    si, sr = _strides(x3)
    form, per_image = ("", ()) if widths is None else ("_ragged", (widths.data_ptr(), float(zoom_x)))
    _lib.call(f"mm_zoom2d{form}_f32" if x3.dtype == torch.float32 else f"mm_zoom2d{form}_f64", dev,
              order, mode, float(cval), flags, x3.data_ptr(), b, h, w, si, sr, *per_image,
              h_out, w_out, out.data_ptr(), h_out * w_out, w_out, ws.data_ptr(), ws.numel())
    return out


def zoom_batch(x, zoom, order=3, mode="constant", cval=0.0, prefilter=True, *, grid_mode=False, db=False):
    """scipy.ndimage.zoom(x, zoom, order=, mode=, cval=, prefilter=) on the last two axes of a CUDA(HIP) tensor ``x``
    [H, W] or [B, H, W] (float32 or float64, any strides whose last is 1) -> [.., round(H zy), round(W zx)] of x's type.
    ``zoom``: a number or (zy, zx).  scipy's defaults and scipy's errors: RuntimeError for a ``zoom`` of another length, an
    order outside 0 .. 5 and a mode scipy does not know, TypeError for an order that is no integer.  Modes scipy has and
    this does not ('nearest', 'reflect', 'wrap', the grid- modes) and grid_mode=True raise NotImplementedError.
    ``db``: the samples are 10 log10(x) in float64 as they are loaded (the reference's ``10 * numpy.log10(values)``).
    Finite inputs only: a non-finite sample makes every output whose taps touch it non-finite, not the whole image as in
    scipy (the module's text).  Nothing is read back."""
    zy, zx = _zoom_pair(zoom)
    order = _order(order)
    code = _mode(mode, grid_mode)
    x3, single = _images(x, "zoom_batch")
    h_out, w_out = zoom_output_size(x3.shape[1], zy), zoom_output_size(x3.shape[2], zx)
    if h_out < 0 or w_out < 0:
        raise ValueError(_MSG_NEGATIVE)
    out = _run(x3, None, 1.0, order, code, cval, (_PREFILTER if prefilter else 0) | (_DB if db else 0), h_out, w_out)
    return out[0] if single else out


def zoom_ragged_batch(x, widths, zoom, order=3, mode="constant", cval=0.0, prefilter=True, *, grid_mode=False, db=False):
    """zoom_batch with a width per image: ``x`` [B, H, W_max] on the device, ``widths`` [B] (host integers, validated:
    ValueError outside [1, W_max]; or an int64 device tensor, clamped by the kernels and never read back) ->
    (y [B, round(H zy), W_out], the output widths).  Image b is zoom_batch(x[b, :, :widths[b]], ...) bit for bit in its
    first round(widths[b] zx) columns, +0.0 behind them; what x holds behind a width (NaN, another image) never matters.
    With host widths W_out is the widest result and the output widths are an int64 numpy array; with device widths W_out
    is round(W_max zx) and they are an int64 tensor on the device."""
    import torch
    zy, zx = _zoom_pair(zoom)
    order = _order(order)
    code = _mode(mode, grid_mode)
    x3, single = _images(x, "zoom_ragged_batch")
    if single:
        raise ValueError(f"zoom_ragged_batch takes a batch [B, H, W_max], got {tuple(x.shape)}")
    b, h, w = x3.shape
    lens = ragged.check_counts(widths, b, w, x3.device, "widths")
    zx = float(zx)
    h_out = zoom_output_size(h, zy)
    if h_out < 0 or zoom_output_size(w, zx) < 0:
        raise ValueError(_MSG_NEGATIVE)
    with torch.cuda.device(x3.device):
        if isinstance(lens, np.ndarray):
            w_outs = np.rint(lens.astype(np.float64) * zx).astype(np.int64)
            if b and int(w_outs.min()) < 1:
                i = int(np.argmin(w_outs))
                raise ValueError(f"zoom_ragged_batch: image {i} of {int(lens[i])} columns has no column at zoom {zx}")
            w_out = int(w_outs.max()) if b else 0
        else:
            w_out = zoom_output_size(w, zx)
            w_outs = torch.clamp(torch.round(torch.clamp(lens, 1, w).to(torch.float64) * zx), 1, max(w_out, 1)).to(torch.int64)
        cd = ragged.counts_on_device(lens, x3.device)
        out = _run(x3, cd, zx, order, code, cval, (_PREFILTER if prefilter else 0) | (_DB if db else 0), h_out, w_out)
    return out, w_outs


def spline_filter_batch(x, order=3):
    """The prefilter alone: scipy.ndimage.spline_filter(x, order, mode='mirror') on the last two axes of a CUDA(HIP) tensor
    [H, W] or [B, H, W] -> the B-spline coefficients, in x's type (orders 2 .. 5; scipy's RuntimeError otherwise)."""
    order = _order(order, least=2)
    x3, single = _images(x, "spline_filter_batch")
    out = _run(x3, None, 1.0, order, 0, 0.0, _PREFILTER | _FILTER_ONLY, x3.shape[1], x3.shape[2])
    return out[0] if single else out


def spectrogram_image(spect_data, zoom_blur=True):
    """script/praat_py_ui/spectrogram.py:70-71 on the device: ``scipy.ndimage.zoom(spect_data, 6, order=4)`` when
    ``zoom_blur``, the image as it is otherwise.  ``spect_data`` is the dB image [F, T] (or a batch [B, F, T])."""
    return zoom_batch(spect_data, 6, order=4) if zoom_blur else spect_data


def spectrogram_image_batch(power, zoom=6, order=4, db=True):
    """The viewer's image from a POWER spectrogram [F, T] or [B, F, T] (what pspec.praat_spectrogram_batch returns -- the
    reference's Sound.to_spectrogram; pspec.spectrogram_view is the whole chain -- or any strictly positive image):
    ``scipy.ndimage.zoom(10 * numpy.log10(power), zoom, order=order)`` with the dB step taken on load, in float64, without
    a pass of its own."""
    return zoom_batch(power, zoom, order=order, db=db)
