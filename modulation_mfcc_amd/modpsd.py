"""The Welch modulation power spectrum on the device: ``scipy.signal.welch`` along the last axis of float32 rows -- MFCC
trajectories, RMS envelopes, any curve the package produces -- averaged, detrended, windowed and scaled, on a frequency
grid that depends on ``fs`` and ``nfft`` alone (mm_modpsd_f32, include/modmfcc_modpsd.h; csrc/mm_modpsd.hip).

    modulation_psd_batch(x, fs, ...)                  [..., n]        -> (f [nfft/2+1] numpy float64, Pxx [..., nfft/2+1])
    modulation_psd_ragged_batch(x, lengths, fs, ...)  [rows, n_max]   -> the same with one length per row

Two deliberate differences from scipy:

* the default ``nfft`` is the smallest power of two in [32, 4096] that is >= ``nperseg`` (scipy: ``nperseg``); the result
  equals scipy's when scipy is called with that ``nfft``.  Other values of ``nfft`` are not built (NotImplementedError);
* a row shorter than ``nperseg`` is refused (scipy shrinks ``nperseg`` and warns): ValueError from the single-length call
  and from the ragged call with host lengths (the row named), a NaN row with device lengths, which are never read back.

``average`` is 'mean'.  Every row's bits are the same in any batch: alone, among other rows, padded or not.
"""
from __future__ import annotations

import collections

import numpy as np

from . import ragged

__all__ = ["modulation_psd_batch", "modulation_psd_ragged_batch", "modpsd_nfft", "modpsd_segments"]

NFFT_MIN, NFFT_MAX = 32, 4096
_DETREND = {False: 0, None: 0, "constant": 1, "linear": 2}
_SCALING = {"density": 0, "spectrum": 1}
SHORT_TEXT = "nperseg = {0} is greater than the input length = {1}; a shorter row has no segment (scipy would shrink nperseg)"

_PLANS = collections.OrderedDict()      # (parameters, window bytes, device) -> _ModpsdPlan, least recently used first
MODPSD_MAX_PLANS = 32                   # a handle owns 64 KiB of twiddles and nfft window values


def modpsd_nfft(nperseg):
    """The default transform length: the smallest power of two in [32, 4096] that is >= nperseg."""
    return max(NFFT_MIN, 1 << (int(nperseg) - 1).bit_length())


class _Spec:
    """The validated parameters of a call: scipy's errors where scipy has one, the float32 window, the C struct."""

    def __init__(self, fs, window, nperseg, noverlap, nfft, detrend, scaling):
        from . import _lib
        if isinstance(nperseg, bool) or int(nperseg) != nperseg or int(nperseg) < 1:
            raise ValueError("nperseg must be a positive integer")
        nperseg = int(nperseg)
        noverlap = nperseg // 2 if noverlap is None else int(noverlap)
        if noverlap >= nperseg:
            raise ValueError("noverlap must be less than nperseg.")
        if noverlap < 0:
            raise ValueError("noverlap must be a nonnegative integer")
        nfft = modpsd_nfft(nperseg) if nfft is None else int(nfft)
        if nfft < nperseg:
            raise ValueError("nfft must be greater than or equal to nperseg.")
        if isinstance(detrend, np.bool_):
            detrend = bool(detrend)
        if not isinstance(detrend, (str, bool, type(None))) or detrend not in _DETREND or detrend is True:
            raise ValueError(f"detrend must be False, 'constant' or 'linear', got {detrend!r}")
        if scaling not in _SCALING:
            raise ValueError(f"Unknown scaling: {scaling!r}")
        fs = float(fs)
        if not (fs > 0 and np.isfinite(fs)):
            raise ValueError("fs must be positive and finite")
        if isinstance(window, (str, tuple)):
            from scipy.signal import get_window
            win = get_window(window, nperseg)
        else:
            win = np.asarray(window.detach().cpu().numpy() if type(window).__module__.startswith("torch") else window)
            if win.ndim != 1:
                raise ValueError("window must be 1-D")
            if win.shape[0] != nperseg:
                raise ValueError("value specified for nperseg is different from length of window")
        self.window = np.ascontiguousarray(win, dtype=np.float32)
        if not np.isfinite(self.window).all():
            raise ValueError("window must be finite")
        w64 = self.window.astype(np.float64)
        if (w64 * w64).sum() == 0 or (scaling == "spectrum" and w64.sum() == 0):
            raise ValueError(f"window sums to zero: no {scaling!r} scaling")
        self.fs, self.nperseg, self.noverlap, self.nfft = fs, nperseg, noverlap, nfft
        self.c = _lib.mm_modpsd_params(fs, nperseg, noverlap, nfft, _DETREND[detrend], _SCALING[scaling])
        import ctypes as C
        _lib.check(_lib.load().mm_modpsd_check(C.byref(self.c)), f"modulation_psd: nfft = {nfft} (a power of two in "
                   f"[{NFFT_MIN}, {NFFT_MAX}] is built)")
        self.bins = nfft // 2 + 1
        self.key = (fs, nperseg, noverlap, nfft, _DETREND[detrend], _SCALING[scaling], self.window.tobytes())

    def freqs(self):
        return np.fft.rfftfreq(self.nfft, 1.0 / self.fs)


def modpsd_segments(n, nperseg=256, noverlap=None):
    """Segments Welch's method takes from a row of ``n`` samples: (n - noverlap) // (nperseg - noverlap), 0 for
    n < nperseg.  Host arithmetic (no GPU needed); an array of lengths gives an int64 array."""
    nperseg = int(nperseg)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if nperseg < 1 or not 0 <= noverlap < nperseg:
        raise ValueError("need nperseg >= 1 and 0 <= noverlap < nperseg")
    n = np.asarray(n, dtype=np.int64)
    k = np.where(n < nperseg, 0, (n - noverlap) // (nperseg - noverlap))
    return int(k) if k.ndim == 0 else k


class _ModpsdPlan:
    """Owner of one mm_modpsd handle (window and twiddle tables of one parameter set on one device)."""

    def __init__(self, spec, device):
        import ctypes as C
        import torch
        from . import _lib
        self._lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(self._lib.mm_modpsd_create(C.byref(spec.c), spec.window.ctypes.data, C.byref(h)), "mm_modpsd_create")
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._lib.mm_modpsd_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _modpsd_plan(spec, device):
    """The cached mm_modpsd handle of (parameters, window bytes, device) -- LRU of MODPSD_MAX_PLANS."""
    key = spec.key + (str(device),)
    if key in _PLANS:
        _PLANS.move_to_end(key)
    else:
        import torch
        while len(_PLANS) >= MODPSD_MAX_PLANS:
            _, old = _PLANS.popitem(last=False)
            torch.cuda.synchronize(device)                    # nothing in flight may still read the tables
            del old
        _PLANS[key] = _ModpsdPlan(spec, device)
    return _PLANS[key]


def _run(spec, x2, lens_dev):
    """mm_modpsd_f32 on x2 [rows, n_max] (unit inner stride) on the current stream -> Pxx [rows, bins] float32."""
    import torch
    from . import _lib
    lib = _lib.load()
    rows, n = x2.shape
    dev = x2.device
    out = torch.empty((rows, spec.bins), dtype=torch.float32, device=dev)
    if rows == 0:
        return out
    plan = _modpsd_plan(spec, dev)
    need = int(lib.mm_modpsd_workspace_bytes(plan.h, rows, n))
    ws = _lib.workspace(need, dev) if need else None
    _lib.call("mm_modpsd_f32", dev, plan.h, x2.data_ptr(), rows, n, ragged.row_pitch(x2),
              None if lens_dev is None else lens_dev.data_ptr(), out.data_ptr(), spec.bins,
              None if ws is None else ws.data_ptr(), need)
    return out


_TYPE_TEXT = "x must be a float32 CUDA(HIP) tensor"


def modulation_psd_batch(x, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant",
                         scaling="density"):
    """``scipy.signal.welch(x, fs, window, nperseg, noverlap, nfft, detrend, scaling=scaling, axis=-1)`` of a float32
    CUDA(HIP) tensor [..., n] (unit inner stride; anything else is copied) -> ``(f, Pxx)``: ``f`` the numpy float64
    frequencies rfftfreq(nfft, 1 / fs), ``Pxx`` a float32 device tensor [..., nfft / 2 + 1].  On the current stream;
    nothing is read back.

    ``window``: a name or tuple for scipy.signal.get_window (periodic), or ``nperseg`` values; ``noverlap`` defaults to
    nperseg // 2, ``nfft`` to the smallest power of two in [32, 4096] >= nperseg (NOT scipy's nperseg: the module text);
    ``detrend`` False, 'constant' or 'linear'; ``scaling`` 'density' (V^2 / Hz) or 'spectrum' (V^2).  ValueError for
    n < nperseg (scipy would shrink nperseg), TypeError for float64 or host input."""
    import torch
    if not (ragged.is_device_tensor(x) and x.dtype == torch.float32):
        raise TypeError(_TYPE_TEXT)
    if x.dim() < 1:
        raise ValueError("x must be [..., n]")
    spec = _Spec(fs, window, nperseg, noverlap, nfft, detrend, scaling)
    n = x.shape[-1]
    if n < spec.nperseg:
        raise ValueError(SHORT_TEXT.format(spec.nperseg, n))
    lead = tuple(x.shape[:-1])
    if x.dim() == 2:
        x2 = ragged.device_rows(x, (torch.float32,), _TYPE_TEXT, "x must be [..., n]", nonempty=False)
    else:
        x2 = x.reshape(-1, n)
        if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
    return spec.freqs(), _run(spec, x2, None).reshape(lead + (spec.bins,))


def modulation_psd_ragged_batch(x, lengths, fs, *, window="hann", nperseg=256, noverlap=None, nfft=None,
                                detrend="constant", scaling="density"):
    """modulation_psd_batch for rows of different lengths in one padded batch: ``x`` [rows, n_max] float32 on the device
    (rows may be strided) and one valid sample count per row -> ``(f, Pxx [rows, nfft / 2 + 1])``.  Row b is
    modulation_psd_batch(x[b, :lengths[b]]) bit for bit: its own segment count, one frequency grid for all rows; what the
    padding holds (zeros, NaN, another row) never matters.

    ``lengths``: host integers (validated: ValueError outside [1, n_max] and for a row shorter than nperseg, the row
    named) or an int64 device tensor (no read-back: the kernel clamps it into [1, n_max], a row shorter than nperseg
    comes out NaN)."""
    import torch
    x2 = ragged.device_rows(x, (torch.float32,), _TYPE_TEXT, "x must be [rows, n_max]")
    rows, n = x2.shape
    spec = _Spec(fs, window, nperseg, noverlap, nfft, detrend, scaling)
    lens = ragged.check_lengths(lengths, rows, n, x2.device)
    ragged.refuse_short(lens, n, spec.nperseg, lambda short: SHORT_TEXT.format(spec.nperseg, short))
    with torch.cuda.device(x2.device):
        lens_dev = ragged.counts_on_device(lens, x2.device)
    return spec.freqs(), _run(spec, x2, lens_dev)
