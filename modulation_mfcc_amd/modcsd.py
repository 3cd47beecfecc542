"""The Welch cross spectrum and coherence on the device: ``scipy.signal.csd`` / ``scipy.signal.coherence`` (and
``scipy.signal.welch`` of either side) along the last axis of pairs of float32 rows -- an MFCC trajectory against the RMS
envelope, the MFCC-change curve against an articulator channel, two coefficients against each other -- in one launch
(mm_modcsd_f32, include/modmfcc_modcsd.h; csrc/mm_modcsd.hip).

    modulation_cross_spectra_batch(x, y, fs, ...)   -> (f, Pxx, Pyy, Pxy complex64, Cxy)
    modulation_csd_batch(x, y, fs, ...)             -> (f, Pxy)         conj(X) Y, as scipy
    modulation_coherence_batch(x, y, fs, ...)       -> (f, Cxy)         no ``scaling``, as scipy
    ..._ragged_batch(x, y, lengths, fs, ...)        the same with one length per pair

``x`` is [..., n] ([rows, n_max] for the ragged calls).  ``y`` has the shape of ``x``, or fewer rows: [m, n] with m dividing
the rows of ``x``; pair r is then row r of x with row r // (rows / m) of y -- the 13 trajectories of a clip against the clip's
one envelope with no copy.  Parameters, defaults, refusals and the frequency grid are those of modpsd.py (``nfft`` defaults to
the smallest power of two >= ``nperseg``), but ``nfft`` ends at 2048 (NotImplementedError beyond).  A pair has one length.

Every pair's bits are the same in any batch: alone, among other pairs, with y shared or materialised, padded or not.  The
coherence never exceeds 1 and is exactly 1 for a pair with a single segment (wherever it is not 0 / 0 = NaN).  Pxx / Pyy are
within the yardstick of modulation_psd_batch but not its bits (that kernel squares in float32).
"""
from __future__ import annotations

from . import modpsd, ragged

__all__ = ["modulation_cross_spectra_batch", "modulation_csd_batch", "modulation_coherence_batch",
           "modulation_cross_spectra_ragged_batch", "modulation_csd_ragged_batch", "modulation_coherence_ragged_batch",
           "y_group"]

NFFT_MAX = 2048
_TYPE_TEXT = "x and y must be float32 CUDA(HIP) tensors"
_ALL, _CSD, _COH = (True, True, True, True), (False, False, True, False), (False, False, False, True)


def y_group(x_rows, y_rows):
    """How many rows of x share one row of y: x_rows / y_rows, ValueError unless y_rows divides x_rows.  Host arithmetic."""
    x_rows, y_rows = int(x_rows), int(y_rows)
    if x_rows == 0 and y_rows == 0:
        return 1
    if y_rows < 1 or x_rows % y_rows:
        raise ValueError(f"y has {y_rows} rows, x has {x_rows}: y must have as many rows as x or a divisor of them")
    return max(1, x_rows // y_rows)


def _spec(fs, window, nperseg, noverlap, nfft, detrend, scaling):
    """modpsd._Spec (its refusals, its defaults), refused beyond nfft 2048 with the limit named."""
    import ctypes as C
    from . import _lib
    spec = modpsd._Spec(fs, window, nperseg, noverlap, nfft, detrend, scaling)
    _lib.check(_lib.load().mm_modcsd_check(C.byref(spec.c)), f"modulation_csd: nfft = {spec.nfft} (a power of two in "
               f"[{modpsd.NFFT_MIN}, {NFFT_MAX}] is built: four float64 sums per bin and lane)")
    return spec


def _check_pair(x, y):
    import torch
    for t in (x, y):
        if not (ragged.is_device_tensor(t) and t.dtype == torch.float32):
            raise TypeError(_TYPE_TEXT)
    if x.device != y.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}")


def _rows(t, n):
    """[..., n] -> [rows, n] with unit inner stride and a row pitch >= n (a copy only where the layout has neither)."""
    t2 = t if t.dim() == 2 else t.reshape(-1, n)
    if (n > 1 and t2.stride(1) != 1) or (t2.shape[0] > 1 and t2.stride(0) < n):
        t2 = t2.contiguous()
    return t2


def _run(spec, x2, y2, group, lens_dev, want):
    """mm_modcsd_f32 on x2 [rows, n], y2 [rows / group, n] on the current stream -> [Pxx, Pyy, Pxy, Cxy], None for an
    output ``want`` does not ask for (its pointer is NULL: not computed, not stored)."""
    import torch
    from . import _lib
    lib = _lib.load()
    rows, n = x2.shape
    dev = x2.device
    shapes = ((rows, spec.bins), (rows, spec.bins), (rows, spec.bins, 2), (rows, spec.bins))
    outs = [torch.empty(s, dtype=torch.float32, device=dev) if w else None for s, w in zip(shapes, want)]
    if rows:
        plan = modpsd._modpsd_plan(spec, dev)
        need = int(lib.mm_modcsd_workspace_bytes(plan.h, rows, n))
        ws = _lib.workspace(need, dev) if need else None
        _lib.call("mm_modcsd_f32", dev, plan.h, x2.data_ptr(), rows, n, ragged.row_pitch(x2), y2.data_ptr(),
                  ragged.row_pitch(y2), group, None if lens_dev is None else lens_dev.data_ptr(),
                  *[None if o is None else o.data_ptr() for o in outs], spec.bins, None if ws is None else ws.data_ptr(), need)
    if outs[2] is not None:
        outs[2] = torch.view_as_complex(outs[2])
    return outs


def _single(x, y, fs, want, window, nperseg, noverlap, nfft, detrend, scaling):
    _check_pair(x, y)
    if x.dim() < 1 or y.dim() < 1:
        raise ValueError("x and y must be [..., n]")
    spec = _spec(fs, window, nperseg, noverlap, nfft, detrend, scaling)
    n = x.shape[-1]
    if y.shape[-1] != n:
        raise ValueError(f"x has {n} samples per row, y has {y.shape[-1]}")
    if n < spec.nperseg:
        raise ValueError(modpsd.SHORT_TEXT.format(spec.nperseg, n))
    lead = tuple(x.shape[:-1])
    x2, y2 = _rows(x, n), _rows(y, n)
    group = y_group(x2.shape[0], y2.shape[0])
    return spec.freqs(), [None if o is None else o.reshape(lead + (spec.bins,))
                          for o in _run(spec, x2, y2, group, None, want)]


def _ragged(x, y, lengths, fs, want, window, nperseg, noverlap, nfft, detrend, scaling):
    import torch
    x2 = ragged.device_rows(x, (torch.float32,), _TYPE_TEXT, "x must be [rows, n_max]")
    y2 = ragged.device_rows(y, (torch.float32,), _TYPE_TEXT, "y must be [rows, n_max] or [rows // g, n_max]")
    _check_pair(x2, y2)
    rows, n = x2.shape
    if y2.shape[1] != n:
        raise ValueError(f"x has {n} samples per row, y has {y2.shape[1]}")
    group = y_group(rows, y2.shape[0])
    spec = _spec(fs, window, nperseg, noverlap, nfft, detrend, scaling)
    lens = ragged.check_lengths(lengths, rows, n, x2.device)
    ragged.refuse_short(lens, n, spec.nperseg, lambda short: modpsd.SHORT_TEXT.format(spec.nperseg, short))
    with torch.cuda.device(x2.device):
        lens_dev = ragged.counts_on_device(lens, x2.device)
    return spec.freqs(), _run(spec, x2, y2, group, lens_dev, want)


def modulation_cross_spectra_batch(x, y, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant",
                                   scaling="density"):
    """Both auto spectra, the cross spectrum and the magnitude-squared coherence of pairs of float32 CUDA(HIP) rows in
    one launch -> ``(f, Pxx, Pyy, Pxy, Cxy)``: ``f`` the numpy float64 frequencies rfftfreq(nfft, 1 / fs); ``Pxx``,
    ``Pyy`` (scipy.signal.welch of either side) and ``Cxy`` (scipy.signal.coherence) float32 [..., nfft / 2 + 1], ``Pxy``
    (scipy.signal.csd: conj(X) Y) complex64.  ``x`` [..., n]; ``y`` of the same shape or [m, n], m dividing the rows of x
    (the module text).  The keywords are those of modulation_psd_batch; nfft <= 2048.  On the current stream; nothing is
    read back."""
    f, o = _single(x, y, fs, _ALL, window, nperseg, noverlap, nfft, detrend, scaling)
    return (f,) + tuple(o)


def modulation_csd_batch(x, y, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant",
                         scaling="density"):
    """``scipy.signal.csd(x, y, fs, ...)`` of pairs of rows -> ``(f, Pxy complex64)``: the Pxy of
    modulation_cross_spectra_batch bit for bit; the other three are not computed."""
    f, o = _single(x, y, fs, _CSD, window, nperseg, noverlap, nfft, detrend, scaling)
    return f, o[2]


def modulation_coherence_batch(x, y, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant"):
    """``scipy.signal.coherence(x, y, fs, ...)`` of pairs of rows -> ``(f, Cxy float32)``: the Cxy of
    modulation_cross_spectra_batch bit for bit (NaN where either side has no power in a bin: scipy's 0 / 0)."""
    f, o = _single(x, y, fs, _COH, window, nperseg, noverlap, nfft, detrend, "density")
    return f, o[3]


def modulation_cross_spectra_ragged_batch(x, y, lengths, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None,
                                          detrend="constant", scaling="density"):
    """modulation_cross_spectra_batch for pairs of different lengths in one padded batch: ``x`` [rows, n_max] and ``y``
    [rows, n_max] or [rows // g, n_max] float32 on the device (rows may be strided) and one valid sample count per PAIR.
    Pair b is modulation_cross_spectra_batch(x[b, :lengths[b]], y[b // g, :lengths[b]]) bit for bit on one frequency grid;
    what lies behind a pair's length never matters.

    ``lengths``: host integers (validated: ValueError outside [1, n_max] and for a pair shorter than nperseg, the row
    named) or an int64 device tensor (no read-back: clamped into [1, n_max] on the device, a pair shorter than nperseg
    comes out NaN in every output)."""
    f, o = _ragged(x, y, lengths, fs, _ALL, window, nperseg, noverlap, nfft, detrend, scaling)
    return (f,) + tuple(o)


def modulation_csd_ragged_batch(x, y, lengths, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None,
                                detrend="constant", scaling="density"):
    """modulation_csd_batch with one length per pair (modulation_cross_spectra_ragged_batch) -> ``(f, Pxy)``."""
    f, o = _ragged(x, y, lengths, fs, _CSD, window, nperseg, noverlap, nfft, detrend, scaling)
    return f, o[2]


def modulation_coherence_ragged_batch(x, y, lengths, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None,
                                      detrend="constant"):
    """modulation_coherence_batch with one length per pair (modulation_cross_spectra_ragged_batch) -> ``(f, Cxy)``."""
    f, o = _ragged(x, y, lengths, fs, _COH, window, nperseg, noverlap, nfft, detrend, "density")
    return f, o[3]
