"""The Lomb-Scargle (least-squares) modulation spectrum of curves with holes, on the device (csrc/mm_lomb.hip,
include/modmfcc_lomb.h).

    modulation_lombscargle_batch(x, fs, f, ...)                  -> [rows, F] float64 (complex128 for 'amplitude')
    modulation_lombscargle_ragged_batch(x, lengths, fs, f, ...)  -> the same with a length per row
    modulation_lombscargle_list(curves, fs, f, ...)              -> a list, one spectrum per 1-D curve of any length

Row r's data points are its valid samples -- the non-NaN samples in front of its length -- at the times ``t`` of one
axis shared by the batch; the result is scipy.signal.lombscargle(t[valid], x[r, valid], 2 pi f, precenter=, normalize=,
floating_mean=) of scipy 1.15, within a few of scipy's own roundings (the yardstick of tests/test_gpu_lomb.py), not bit for bit.  Nothing is
filled in: an f0 curve that is NaN where the clip is unvoiced, or an articulograph channel with drop-outs, is analysed on
the samples it has.  There is no host fallback.
"""
from __future__ import annotations


import numpy as np

from . import ragged

__all__ = ["modulation_lombscargle_batch", "modulation_lombscargle_ragged_batch", "modulation_lombscargle_list",
           "LOMB_CHUNK"]

LOMB_CHUNK = 512            # samples a workgroup sums (MM_LOMB_CHUNK of include/modmfcc_lomb.h): longer rows are cut

# scipy.signal.lombscargle's own texts
_MSG_XY = "Parameters x, y, weights must be 1-D arrays of equal non-zero length!"
_MSG_FREQS = "Parameter freqs must be a 1-D array of non-zero length!"
_MSG_NORMALIZE = "Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'."
_NORMALIZE = {"power": 0 << 2, "normalize": 1 << 2, "amplitude": 2 << 2}        # MM_LOMB_POWER / _NORMALIZE / _AMPLITUDE

_axes = {}                  # (n_max, fs, device) -> the default time axis on the device, uploaded once; the last
_AXES_KEPT = 16             # sixteen are kept (a caller that sweeps n_max must not collect one tensor per length)
_grids = {}                 # (omega's bytes, device) -> omega on the device: a repeated grid is uploaded once, so that a
_GRIDS_KEPT = 16            # warmed call copies nothing from the host (it can be captured into a graph)


def _flags(precenter, normalize, floating_mean):
    if isinstance(normalize, (bool, np.bool_)):
        normalize = "normalize" if normalize else "power"
    if not isinstance(normalize, str) or normalize not in _NORMALIZE:
        raise ValueError(_MSG_NORMALIZE)
    return (1 if precenter else 0) | (2 if floating_mean else 0) | _NORMALIZE[normalize]


def _omega(f):
    """f in Hz -> (omega in rad/s, float64 on the host: the very array a caller would hand to scipy)."""
    f = np.asarray(f, dtype=np.float64)
    if not (f.ndim == 1 and f.size > 0):
        raise ValueError(_MSG_FREQS)
    return 2.0 * np.pi * f


def _grid_on_device(omega, dev):
    import torch
    key = (omega.tobytes(), str(dev))
    if key not in _grids:
        while len(_grids) >= _GRIDS_KEPT:
            _grids.pop(next(iter(_grids)))
        _grids[key] = torch.from_numpy(omega).to(dev)
    return _grids[key]


def default_time_axis(n_max, fs):
    """np.arange(n_max) / fs in float64: the reference's time axis of a curve sampled at fs."""
    return np.arange(int(n_max)) / fs


def _time_axis(t, n_max, fs, dev):
    import torch
    if t is None:
        key = (int(n_max), float(fs), str(dev))
        if key not in _axes:
            while len(_axes) >= _AXES_KEPT:
                _axes.pop(next(iter(_axes)))
            _axes[key] = torch.from_numpy(default_time_axis(n_max, float(fs))).to(dev)
        return _axes[key]
    if ragged.is_device_tensor(t):
        if t.dtype != torch.float64 or tuple(t.shape) != (int(n_max),):
            raise ValueError(_MSG_XY)
        return t.to(dev).contiguous()
    t = np.asarray(t, dtype=np.float64)
    if t.shape != (int(n_max),):
        raise ValueError(_MSG_XY)
    if not np.isfinite(t).all():
        raise ValueError("t must be finite at every index: the cosines of omega t are shared by the rows of the batch")
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def _rows(x, who):
    import torch
    if not ragged.is_device_tensor(x):
        raise TypeError(f"{who} takes a CUDA(HIP) tensor")
    if not x.is_floating_point():
        raise TypeError("x must be a floating-point tensor")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(_MSG_XY)
    xd = x if x.dtype == torch.float64 else x.double()
    if (xd.shape[1] > 1 and xd.stride(1) != 1) or (xd.shape[0] > 1 and xd.stride(0) < xd.shape[1]):
        xd = xd.contiguous()
    return xd


def _run(xd, cd, t, fs, f, precenter, normalize, floating_mean):
    import torch
    from . import _lib
    flags = _flags(precenter, normalize, floating_mean)
    omega = _omega(f)
    rows, n_max = xd.shape
    dev = xd.device
    with torch.cuda.device(dev):
        td = _time_axis(t, n_max, fs, dev)
        od = _grid_on_device(omega, dev)
        nf = omega.shape[0]
        amplitude = (flags & (3 << 2)) == _NORMALIZE["amplitude"]
        out = torch.empty((2 if amplitude else 1, rows, nf), dtype=torch.float64, device=dev)
        lib = _lib.load()
        need = int(lib.mm_lombscargle_workspace_bytes(rows, n_max, nf))
        if need == 0:
            raise ValueError(f"modulation_lombscargle: [{rows}, {n_max}] rows x {nf} frequencies is beyond the kernel's limits")
        ws = _lib.workspace(need, dev)
        _lib.call("mm_lombscargle_f64", dev, xd.data_ptr(), rows, n_max, ragged.row_pitch(xd),
                  None if cd is None else cd.data_ptr(), td.data_ptr(), od.data_ptr(), nf, flags, out[0].data_ptr(), nf,
                  out[1].data_ptr() if amplitude else None, ws.data_ptr(), ws.numel())
        return torch.complex(out[0], out[1]) if amplitude else out[0]


def modulation_lombscargle_batch(x, fs, f, *, t=None, precenter=False, normalize=False, floating_mean=False):
    """The Lomb-Scargle periodogram of every row of a CUDA(HIP) tensor ``x`` [rows, n] (float64; float32 rows are widened)
    at the frequencies ``f`` (Hz, a host array) -> [rows, len(f)] float64 on the device, complex128 for
    normalize='amplitude'.  The NaN samples of a row are no data points.  ``t``: the time axis of the n samples in
    seconds, any finite float64 axis of length n (a host array, checked: ValueError for a NaN or Inf; or a device tensor,
    not read back: a non-finite time there poisons every row, masked or not); the default, np.arange(n) / fs, is uploaded
    once per (n, fs, device).  precenter, normalize (False | 'power', True | 'normalize', 'amplitude') and floating_mean
    are scipy.signal.lombscargle's, and so are its ValueErrors for an empty ``f``, wrong shapes and an unknown
    normalize.  A row without a valid sample comes out NaN: nothing is read back."""
    _flags(precenter, normalize, floating_mean)             # scipy's argument errors come first, device or not
    _omega(f)
    xd = _rows(x, "modulation_lombscargle_batch")
    return _run(xd, None, t, fs, f, precenter, normalize, floating_mean)


def modulation_lombscargle_ragged_batch(x, lengths, fs, f, *, t=None, precenter=False, normalize=False,
                                        floating_mean=False):
    """modulation_lombscargle_batch with a length per row: ``x`` [rows, n_max] on the device, ``lengths`` [rows] (host
    integers, validated: ValueError outside [1, n_max]; or an int64 device tensor, clamped by the kernels).  Row b is
    modulation_lombscargle_batch(x[b:b + 1, :lengths[b]], ...) bit for bit; what x holds at or behind a row's length
    (NaN, Inf, another curve) never matters.  With host lengths a row without a valid sample raises scipy's ValueError
    with the row named (one read-back of the mask counts); with device lengths nothing is read back and such a row comes
    out NaN -- the convention of apply_filter_ragged_batch."""
    import torch
    _flags(precenter, normalize, floating_mean)
    _omega(f)
    xd = _rows(x, "modulation_lombscargle_ragged_batch")
    rows, n_max = xd.shape
    lens = ragged.check_lengths(lengths, rows, n_max, xd.device)
    with torch.cuda.device(xd.device):
        cd = ragged.counts_on_device(lens, xd.device)
        if isinstance(lens, np.ndarray):
            behind = torch.arange(n_max, device=xd.device)[None, :] >= cd[:, None]
            valid = (~(torch.isnan(xd) | behind)).sum(dim=1).cpu().numpy()
            ragged.refuse_short(valid, n_max, 1, _MSG_XY, "row", "valid samples")
        return _run(xd, cd, t, fs, f, precenter, normalize, floating_mean)


def modulation_lombscargle_list(curves, fs, f, /, **kw):
    """modulation_lombscargle_batch for a list of 1-D CUDA(HIP) curves of any lengths -> a list of [len(f)] tensors, each
    what the curve gives alone, bit for bit.  The curves form one padded float64 batch and run through
    modulation_lombscargle_ragged_batch: one call instead of one per distinct length.  ``t``, where given, covers the
    longest curve.  A curve without a valid sample raises scipy's ValueError with the curve's index appended."""
    import torch
    curves = list(curves)
    for i, c in enumerate(curves):
        if not ragged.is_device_tensor(c):
            raise TypeError(f"modulation_lombscargle_list takes CUDA(HIP) tensors (curve {i})")
        if c.dim() != 1:
            raise ValueError(f"curves must be [n] (curve {i})")
        if c.shape[0] < 1:
            raise ValueError(f"curves must not be empty (curve {i})")
    if not curves:
        return []
    x, lens = ragged.pack(curves, torch.float64)
    try:
        y = modulation_lombscargle_ragged_batch(x, lens, fs, f, **kw)
    except ragged.RowRefused as e:
        raise ragged.named(e, e.row, "curve")
    return [y[b] for b in range(len(curves))]
