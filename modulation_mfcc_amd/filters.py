"""``applyFilter`` -- shared by the reference's script/mfcc.py:29-135 and script/calc.py:23-129
(the two copies are identical in behaviour).  Filter DESIGN (butter, firwin, savgol_coeffs) is scipy on the
host exactly as in the reference.  numpy input is filtered by the reference's own scipy calls; float64 curves
that live on the GPU are filtered there (mm_sosfiltfilt_f64; mm_stencil_f64 for FIR filters up to 8 taps and
Savitzky-Golay windows up to 16 samples, mm_fir_filtfilt_f64 / mm_savgol_f64 for every longer one) -- SURVEY.md 8(f) row N1.
A padded batch of device curves with a length per curve goes through apply_filter_ragged_batch (the mm_*_ragged_* entries:
every row what applyFilter gives for the row alone, in the launches of one call); applyFilter_batch takes a list of curves.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
from scipy import signal as _sig

from . import ragged
from .ragged import RowRefused  # noqa: F401  (callers catch it here)

_KINDS = ("bandpass", "lowpass", "highpass")

_MSG_NO_CUTOFF = "Cannot apply filter without specifying a cut Off freq. (CutOff is None)."
_MSG_NO_FILT = ("Cannot apply filter without specifying a filter method among iir, fir and  sg "
                "(filt is None).")
_MSG_KIND = "filtType must be one among: lowpass, highpass, bandpass. Partial matches allowed."
_MSG_NYQ = ("Cut off frequencies must be smaller than the half of the sampling freq. of the signal "
            "submitted to the filter")
_MSG_ORDER = "If two cut off freqs are provided: cutOff[0]<cutOff[1]"
_MSG_COUNT = ("only one or two cut off frequencies allowed. If two freqs are provided, filtType "
              "must be bandpass")
_MSG_SG = "sg (savitsky Golay) filters can only be lowpass (one cutOff freq allowed)"


def _resolve_kind(prefix):
    for kind in _KINDS:           # reference order: first match in (bandpass, lowpass, highpass)
        try:
            if kind.startswith(prefix):
                return kind
        except TypeError:
            break
    raise Exception(_MSG_KIND)


def _band_edges(cut, sr, kind):
    n = len(cut)
    if not ((n == 1 and kind in ("lowpass", "highpass")) or (n == 2 and kind == "bandpass")):
        raise Exception(_MSG_COUNT)
    return np.asarray(cut, dtype=float) / (sr / 2)


def _validate(filt, cutOff, filtType, sr):
    if filt is None or cutOff is None:
        raise Exception(_MSG_NO_CUTOFF if cutOff is None else _MSG_NO_FILT)
    kind = _resolve_kind(filtType)
    if any((sr / 2) <= np.array(cutOff)):
        raise Exception(_MSG_NYQ)
    if len(cutOff) > 0 and any(np.diff(cutOff) <= 0):
        raise Exception(_MSG_ORDER)
    return kind


@functools.lru_cache(maxsize=64)
def _iir_sos_cached(sr, cut, filtLen, kind):
    sos = _sig.butter(filtLen, _band_edges(list(cut), sr, kind), btype=kind, output="sos")
    return sos


def _iir_design(sr, cutOff, filtLen, kind):
    """The Butterworth design of applyFilter(filt='iir'), kept per argument set -- but ONLY for arguments the cache key
    represents exactly: an integral order (int / np.integer, not bool) and numeric cut-offs.  Anything else (filtLen =
    6.5, a string, ...) goes straight to the reference's own scipy.signal.butter call, so scipy's validation and message
    apply ('Filter order must be a nonnegative integer') instead of a silently truncated order."""
    if isinstance(filtLen, (int, np.integer)) and not isinstance(filtLen, (bool, np.bool_)):
        try:
            return _iir_sos_cached(float(sr), tuple(float(c) for c in cutOff), int(filtLen), kind)
        except (TypeError, ValueError):
            pass
    return _sig.butter(filtLen, _band_edges(cutOff, sr, kind), btype=kind, output="sos")


def iir_sos(sr, *, cutOff, filtLen=6, filtType="low"):
    """The Butterworth sections applyFilter(filt='iir') would use (same checks, same exceptions); the design is
    kept per argument set (host arithmetic, scipy.signal.butter)."""
    kind = _validate("iir", cutOff, filtType, sr)
    return np.array(_iir_design(sr, cutOff, filtLen, kind))


def sos_sections(sos):
    """The float64 [n_sections, 6] array of an SOS argument, or scipy's own ValueError (signal._filter_design._validate_sos:
    same conditions, same messages) -- a flat vector of 6 k numbers, or sections scaled so that a0 != 1, are refused as
    scipy.signal.sosfiltfilt refuses them, before anything is launched.  More sections than the kernels take
    (_lib.MM_MAX_SEC) is the library's limit, not scipy's: MMError."""
    from . import _lib
    s = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    if s.ndim != 2:
        raise ValueError("sos array must be 2D")
    if s.shape[1] != 6:
        raise ValueError("sos array must be shape (n_sections, 6)")
    if not (s[:, 3] == 1).all():
        raise ValueError("sos[:, 3] should be all ones")
    if s.shape[0] > _lib.MM_MAX_SEC:
        raise _lib.MMError(_lib.MM_ERR_UNSUPPORTED, f"{s.shape[0]} second-order sections: the device filters take at most "
                                                    f"{_lib.MM_MAX_SEC}")
    return np.ascontiguousarray(s)


def sosfiltfilt_batch(x, sos):
    """scipy.signal.sosfiltfilt(sos, x) along the last axis of a float64 or float32 CUDA(HIP) tensor [rows, n] (or [n])
    on the device (mm_sosfiltfilt_f64 / _f32_f64): the recursion of applyFilter(filt='iir') for a whole batch of
    curves; float64 result, as scipy returns for either input type."""
    import torch
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float64, torch.float32)):
        raise TypeError("x must be a float64 or float32 CUDA(HIP) tensor")
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [rows, n]")
    s = sos_sections(sos)
    if x2.shape[1] <= ragged.sos_padlen(s):   # scipy.signal.sosfiltfilt's own check and message
        raise ValueError(ragged.PADLEN_TEXT.format(ragged.sos_padlen(s)))
    out = _sosfiltfilt(x2, x2.stride(0), s)
    return out[0] if squeeze else out


def _f64_entry(x2, stem, d_lens):
    """The name of a filter entry for rows of x2's type, single-length or ragged: float32 rows (librosa's RMS envelope ...)
    go to the _f32_f64 entries, which form the odd extension in float32 before they upcast, as scipy does; the result is
    float64 either way."""
    import torch
    return stem + ("" if d_lens is None else "_ragged") + ("_f64" if x2.dtype == torch.float64 else "_f32_f64")


def _sosfiltfilt(x2, pitch, s, d_lens=None):
    """mm_sosfiltfilt_f64 / _f32_f64 (``d_lens`` None) or their _ragged twins on checked rows -> float64 [rows, n]."""
    import torch
    from . import _lib
    rows, n = x2.shape
    sizer = "mm_sosfiltfilt_workspace_bytes" if d_lens is None else "mm_sosfiltfilt_ragged_workspace_bytes"
    out = torch.empty((rows, n), dtype=torch.float64, device=x2.device)
    ws = _lib.workspace(getattr(_lib.load(), sizer)(rows, n), x2.device)
    _lib.call(_f64_entry(x2, "mm_sosfiltfilt", d_lens), x2.device, x2.data_ptr(), rows, n, pitch, *ragged.lens_arg(d_lens),
              s.ctypes.data, s.shape[0], out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def fir_filtfilt_stencil(taps):
    """scipy.signal.filtfilt(taps, 1, x) -- the 'fir' branch of applyFilter (script/mfcc.py:113-126) -- as the
    banded operator mm_stencil_f64 applies.  filtfilt pads x by an odd extension of 3 * len(taps) samples, runs
    the filter forwards and backwards from lfilter_zi states and crops the padding; for an FIR filter the two
    start-up transients (len(taps) - 1 samples each) lie inside the cropped padding, so every kept output is
    the correlation of the extended signal with h = taps (*) reversed taps.  Inside that is the symmetric stencil
    h; the first / last len(taps) - 1 outputs fold the taps that reach the extension x_ext[-m] = 2 x[0] - x[m]
    back onto the signal.  Raises NotImplementedError when it does not fit the C struct (more than 8 taps; or a single tap,
    which scipy rejects)."""
    from . import _lib
    b = np.asarray(taps, dtype=np.float64).ravel()
    L = len(b)
    if L < 2 or 2 * L - 1 > _lib.MM_ST_MAXW or L - 1 > _lib.MM_ST_MAXE:     # one tap: scipy's lfilter_zi raises
        raise NotImplementedError("FIR filter too long (or too short) for the device stencil")
    h = np.convolve(b, b[::-1])                      # h[d + L - 1], d = -(L-1) .. L-1 (symmetric)
    half = L - 1
    ew = 2 * half
    el = np.zeros((half, ew))
    for i in range(half):
        for d in range(-half, half + 1):
            j = i + d
            if j >= 0:
                el[i, j] += h[d + half]
            else:                                    # odd extension about x[0]
                el[i, 0] += 2.0 * h[d + half]
                el[i, -j] -= h[d + half]
    er = el[::-1, ::-1]                              # the same fold about x[n - 1]
    return dict(off=list(range(-half, half + 1)), c=[float(v) for v in h], den_c=1.0, n_edge=half, edge_w=ew,
                el=el.tolist(), er=np.ascontiguousarray(er).tolist(), den_e=1.0)


LONGFILT_TILE = 2048        # outputs per workgroup of the long-filter kernel (kLfTile of csrc/mm_longfilt.hip)
LONGFILT_CHUNK = 128        # taps per chunk: each chunk is staged and summed on its own (kLfChunk)
LONGFILT_MAX_TABLES = 16    # device tables kept (a 1001-tap FIR is 16 kB, a 1001 x 5 Savitzky-Golay set 60 kB)

_LONG_TABLES = collections.OrderedDict()    # (kind, arguments ..., device) -> device tables, least recently used first


def _device_tables(key, dev, build):
    """The float64 device tables of one argument set on one device (LRU of LONGFILT_MAX_TABLES sets); ``build`` returns
    the host arrays."""
    import torch
    key = key + (str(dev),)
    if key in _LONG_TABLES:
        _LONG_TABLES.move_to_end(key)
    else:
        while len(_LONG_TABLES) >= LONGFILT_MAX_TABLES:
            torch.cuda.synchronize(dev)          # nothing in flight may still read the evicted tables
            _LONG_TABLES.popitem(last=False)
        _LONG_TABLES[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in build())
    return _LONG_TABLES[key]


def fir_filtfilt_taps(taps):
    """h = taps (*) reversed taps, the 2 L - 1 correlation taps of scipy.signal.filtfilt(taps, 1, x) on the odd-extended
    signal (see fir_filtfilt_stencil), h[k] on x_ext[i - (L - 1) + k]: formed in long double, rounded once."""
    b = np.asarray(taps, dtype=np.float64).ravel().astype(np.longdouble)
    return np.convolve(b, b[::-1]).astype(np.float64)


def _savgol_basis(window, polyorder, deriv, pos):
    """The polynomials of degree <= polyorder that are orthonormal over the window positions 0 .. window - 1:
    (phi [polyorder + 1][window], their values there; dphi [polyorder + 1][len(pos)], their deriv-th derivatives with respect
    to the position at ``pos``), in long double.  phi_{k+1} is t phi_k orthogonalised (twice) against phi_0 .. phi_k on
    the abscissa scaled to [-1, 1] and normalised; the derivatives follow the same linear steps, (t phi_k)^(m) =
    t phi_k^(m) + m phi_k^(m-1) -- no power basis, no least-squares solve: the fit of degree p through samples x is
    sum_q (phi_q . x) phi_q."""
    LD = np.longdouble
    s = LD(2) / LD(window - 1) if window > 1 else LD(1)
    mid = LD(window - 1) / LD(2)
    t = (np.arange(window).astype(LD) - mid) * s
    te = (np.asarray(pos, dtype=np.float64).astype(LD) - mid) * s
    phi = np.zeros((polyorder + 1, window), dtype=LD)
    d = np.zeros((deriv + 1, polyorder + 1, len(te)), dtype=LD)        # d[m][q]: m-th derivative of polynomial q at te
    phi[0] = 1 / np.sqrt(LD(window))
    d[0, 0] = phi[0, 0]
    for k in range(polyorder):
        v = t * phi[k]
        dv = te * d[:, k]
        dv[1:] += np.arange(1, deriv + 1).astype(LD)[:, None] * d[:-1, k]
        for _ in range(2):
            r = phi[:k + 1] @ v
            v = v - r @ phi[:k + 1]
            dv = dv - np.einsum("q,mqe->me", r, d[:, :k + 1])
        norm = np.sqrt((v * v).sum())
        phi[k + 1] = v / norm
        d[:, k + 1] = dv / norm
    return phi, d[deriv] * s ** deriv


def savgol_tables(window_length, polyorder, deriv=0, delta=1.0):
    """The three float64 tables of mm_savgol_f64 for scipy.signal.savgol_filter(x, window_length, polyorder, deriv, delta,
    mode='interp'), built in long double and rounded once:
        c [W]              interior taps as a correlation, savgol_coeffs(W, p, deriv, delta)[::-1]: c[k] on
                           x[i - (W - 1) // 2 + k] (the fit evaluated at the window's centre (W - 1) / 2, which for an
                           even window lies between two samples: scipy's centring)
        Q [p + 1][W]       an orthonormal basis of the polynomials of degree <= p on the window
        P [2][W // 2][p + 1]   the basis' deriv-th derivatives / delta^deriv at positions 0 .. W // 2 - 1 (the first outputs,
                           fitted to x[:W]) and at W - W // 2 .. W - 1 (the last ones, fitted to x[-W:])
    The fit's coefficients are a = Q x[window], the edge outputs P a.  Raises scipy's own ValueErrors."""
    from scipy.signal import savgol_coeffs
    W, p, deriv = int(window_length), int(polyorder), int(deriv)
    savgol_coeffs(W, p, deriv=deriv, delta=delta)          # scipy's argument checks, scipy's messages
    if deriv < 0:
        raise ValueError("deriv must be a nonnegative integer")
    half = W // 2
    pos = np.concatenate(([(W - 1) / 2.0], np.arange(half), np.arange(W - half, W)))
    phi, dphi = _savgol_basis(W, p, deriv, pos)
    dphi = dphi / np.longdouble(delta) ** deriv
    c = (dphi[:, 0][:, None] * phi).sum(axis=0)
    P = np.ascontiguousarray(dphi[:, 1:].T).reshape(2, half, p + 1)
    return c.astype(np.float64), phi.astype(np.float64), P.astype(np.float64)


def _fir_filtfilt(x2, b, d_lens=None):
    """mm_fir_filtfilt_f64 / _f32_f64 (``d_lens`` None) or their _ragged twins on checked rows -> float64 [rows, n]."""
    import torch
    from . import _lib
    rows, n = x2.shape
    out = torch.empty((rows, n), dtype=torch.float64, device=x2.device)
    if rows:
        (h,) = _device_tables(("fir", b.tobytes()), x2.device, lambda: (fir_filtfilt_taps(b),))
        _lib.call(_f64_entry(x2, "mm_fir_filtfilt", d_lens), x2.device, x2.data_ptr(), rows, n, ragged.row_pitch(x2),
                  *ragged.lens_arg(d_lens), h.data_ptr(), len(b), out.data_ptr(), n)
    return out


def _savgol(x2, tables, W, p, was_f32, d_lens=None):
    """mm_savgol_f64 (``d_lens`` None) or mm_savgol_ragged_f64 on checked float64 rows -> [rows, n], float32 again for rows
    that were float32 (filtered in float64, rounded once)."""
    import torch
    from . import _lib
    rows, n = x2.shape
    c, q, pe = tables
    out = torch.empty((rows, n), dtype=torch.float64, device=x2.device)
    if rows:
        _lib.call("mm_savgol_f64" if d_lens is None else "mm_savgol_ragged_f64", x2.device, x2.data_ptr(), rows, n,
                  ragged.row_pitch(x2), *ragged.lens_arg(d_lens), c.data_ptr(), q.data_ptr(), pe.data_ptr(), W, p + 1,
                  out.data_ptr(), n)
    return out.float() if was_f32 else out


def fir_filtfilt_batch(x, taps):
    """scipy.signal.filtfilt(taps, 1, x) along the last axis of a float64 or float32 CUDA(HIP) tensor [rows, n] (or [n])
    on the device, for ANY number of taps L >= 2 (mm_fir_filtfilt_f64 / _f32_f64): the correlation of the odd-extended rows
    with the 2 L - 1 taps of fir_filtfilt_taps.  Rows may be strided (row stride >= n).  float64 result, as scipy returns
    for either input type; a float32 row's extension is formed in float32, as scipy forms it.  n <= 3 L raises scipy's
    ValueError."""
    import torch
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float64, torch.float32)):
        raise TypeError("x must be a float64 or float32 CUDA(HIP) tensor")
    b = np.asarray(taps, dtype=np.float64).ravel()
    L = len(b)
    if L < 2:
        raise ValueError("fir_filtfilt_batch needs at least two taps")
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [rows, n]", pitched=True)
    if x2.shape[1] <= 3 * L:      # scipy.signal.filtfilt's own check and message
        raise ValueError(ragged.PADLEN_TEXT.format(3 * L))
    out = _fir_filtfilt(x2, b)
    return out[0] if squeeze else out


def savgol_batch(x, window_length, polyorder, deriv=0, delta=1.0):
    """scipy.signal.savgol_filter(x, window_length, polyorder, deriv=deriv, delta=delta, mode='interp') along the last axis
    of a float64 or float32 CUDA(HIP) tensor [rows, n] (or [n]) on the device, for ANY window_length <= n (mm_savgol_f64,
    tables: savgol_tables).  Rows may be strided.  A float32 tensor comes back float32, filtered in float64 and rounded
    once, as scipy does.  Bad arguments raise scipy's ValueErrors."""
    import torch
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float64, torch.float32)):
        raise TypeError("x must be a float64 or float32 CUDA(HIP) tensor")
    W, p, deriv, delta = int(window_length), int(polyorder), int(deriv), float(delta)
    tables = _device_tables(("sg", W, p, deriv, delta), x.device, lambda: savgol_tables(W, p, deriv, delta))
    was_f32 = x.dtype == torch.float32
    x2, squeeze = ragged.batch_rows(x.double() if was_f32 else x, "x must be [n] or [rows, n]", pitched=True)
    if W > x2.shape[1]:           # scipy.signal.savgol_filter's own check and message
        raise ValueError(ragged.SG_WINDOW_TEXT)
    out = _savgol(x2, tables, W, p, was_f32)
    return out[0] if squeeze else out


def _stencil_rows(x, st):
    from .calc import apply_stencil
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [rows, n]")
    y = apply_stencil(x2, st, 1)
    return y[0] if squeeze else y


def _apply_filter_device(x, sr, kind, *, filt, cutOff, filtLen, polyOrd, coeffs):
    """applyFilter for float64 CUDA(HIP) curves ([n] or [rows, n], along the last axis): 'iir' through
    mm_sosfiltfilt_f64, 'sg' and 'fir' through the banded-operator kernel (mm_stencil_f64) where the filter fits its C
    struct (Savitzky-Golay windows up to 16 samples, FIR filters up to 8 taps: results unchanged), longer ones through
    savgol_batch / fir_filtfilt_batch.  Only what scipy itself rejects (a single FIR tap) still goes to the reference's
    own scipy call on the host, for its exception."""
    import torch
    was_f32 = x.dtype == torch.float32
    x_in = x                                # (the float32 entry points and scipy below get the caller's own type)
    if filt == "iir" and was_f32:
        pass                                # float32 curves keep their type up to the kernel (odd extension in float32)
    elif x.dtype != torch.float64:
        x = x.double()                      # scipy filters in float64 whatever the input type
    if filt == "iir":
        if coeffs is not None:
            sos = np.asarray(coeffs)
        else:                               # the design (host, ~0.15 ms) is kept per argument set: the device filter of
            _band_edges(cutOff, sr, kind)   # 1024 envelope rows takes less than designing it (count check first)
            sos = _iir_design(sr, cutOff, filtLen, kind)
        return sosfiltfilt_batch(x, sos)
    if filt == "sg":
        if len(cutOff) != 1:
            raise Exception(_MSG_SG)
        from .calc import velocity_batch
        y = velocity_batch(x, 1.0, 0, "sg", filtLen, 2, polyOrd)       # (any window: the stencil, beyond it savgol_batch)
        # scipy.signal.savgol_filter keeps a float32 curve float32 (it correlates in double and rounds once): so here
        return y.float() if was_f32 else y
    if filt == "fir":
        taps = np.asarray(coeffs) if coeffs is not None else \
            _sig.firwin(filtLen, _band_edges(cutOff, sr, kind), window=("kaiser", 7.4), pass_zero=kind)
        try:
            st = fir_filtfilt_stencil(taps)
        except NotImplementedError:
            st = None
        if st is not None:
            pad = 3 * len(taps)
            if x.shape[-1] <= pad:             # scipy.signal.filtfilt's own check and message
                raise ValueError(ragged.PADLEN_TEXT.format(pad))
            if was_f32:
                # scipy forms the odd extension of a float32 curve in float32 before lfilter upcasts (as sosfiltfilt does):
                # extend explicitly in float32, run the operator over the extended curve (its own edge rows then only touch
                # samples that are cropped again: pad > taps - 1), crop
                xi = x_in if x_in.dim() == 2 else x_in.unsqueeze(0)
                n = xi.shape[1]
                ext = torch.cat((2 * xi[:, :1] - xi[:, 1:pad + 1].flip(1), xi, 2 * xi[:, -1:] - xi[:, n - pad - 1:n - 1].flip(1)), dim=1)
                y = _stencil_rows(ext.double(), st)[:, pad:pad + n]
                return y[0] if x_in.dim() == 1 else y
            return _stencil_rows(x, st)
        if np.size(taps) >= 2:                 # more than 8 taps: the long kernel (float32 rows through _f32_f64)
            return fir_filtfilt_batch(x_in if was_f32 else x, taps)
        # a single tap: scipy's own call, for scipy's own exception
        y = applyFilter(x_in.cpu().numpy(), sr, filt=filt, cutOff=cutOff, filtLen=filtLen,
                        filtType=kind[:-4], polyOrd=polyOrd, coeffs=coeffs)
        return torch.from_numpy(np.ascontiguousarray(y)).to(x.device)
    raise UnboundLocalError(f"applyFilter: unknown filt {filt!r} (expected 'iir', 'fir' or 'sg')")


# ---- ragged batches: a padded batch [rows, n_max] and a length per row -------------------------------------------------
# Row b of every function below equals the single-length function on x[b:b+1, :n_b] bit for bit in its first n_b columns
# and is +0.0 behind them; the columns of x at and behind n_b are never read (NaN, Inf, another row's data).  The launches
# are those of the single-length call at n_max; device lengths are not read back.


def _ragged_args(x, lengths):
    """The common argument checks: (x as ragged.device_rows returns it, lengths as ragged.check_lengths does)."""
    import torch
    x = ragged.device_rows(x, (torch.float64, torch.float32), "x must be a float64 or float32 CUDA(HIP) tensor",
                           "x must be [rows, n_max], at least one row and one column")
    return x, ragged.check_lengths(lengths, x.shape[0], x.shape[1], x.device)


def sosfiltfilt_ragged_batch(x, lengths, sos):
    """sosfiltfilt_batch with a length per row (mm_sosfiltfilt_ragged_f64 / _f32_f64): x float64 or float32 [rows, n_max]
    on the device (rows may be strided), ``lengths`` host integers or an int64 device tensor [rows] -> float64
    [rows, n_max].  Both odd extensions are formed about the row's own ends, the backward pass starts at the row's own
    end.  Host lengths at or below scipy's padlen raise scipy's ValueError with the row named; device lengths go through
    without a read-back (clamped into [1, n_max]; such a row comes out NaN before its length).  Up to 4 sections (more:
    NotImplementedError, the library's MM_ERR_UNSUPPORTED -- apply_filter_ragged_batch filters those per distinct length)."""
    x2, lens = _ragged_args(x, lengths)
    s = sos_sections(sos)
    padlen = ragged.sos_padlen(s)
    ragged.refuse_short(lens, x2.shape[1], padlen + 1, ragged.PADLEN_TEXT.format(padlen))
    return _sosfiltfilt(x2, ragged.row_pitch(x2), s, ragged.counts_on_device(lens, x.device))


def fir_filtfilt_ragged_batch(x, lengths, taps):
    """fir_filtfilt_batch with a length per row (mm_fir_filtfilt_ragged_f64 / _f32_f64), any number of taps L >= 2: x
    float64 or float32 [rows, n_max] on the device, ``lengths`` as for sosfiltfilt_ragged_batch -> float64 [rows, n_max].
    The odd extension is staged about the row's own ends (a float32 row's in float32).  Host lengths <= 3 L raise scipy's
    ValueError with the row named; such a row comes out NaN with device lengths."""
    x2, lens = _ragged_args(x, lengths)
    b = np.asarray(taps, dtype=np.float64).ravel()
    L = len(b)
    if L < 2:
        raise ValueError("fir_filtfilt_ragged_batch needs at least two taps")
    ragged.refuse_short(lens, x2.shape[1], 3 * L + 1, ragged.PADLEN_TEXT.format(3 * L))
    return _fir_filtfilt(x2, b, ragged.counts_on_device(lens, x.device))


def savgol_ragged_batch(x, lengths, window_length, polyorder, deriv=0, delta=1.0):
    """savgol_batch with a length per row (mm_savgol_ragged_f64), any window_length: x float64 or float32 [rows, n_max] on
    the device, ``lengths`` as for sosfiltfilt_ragged_batch -> [rows, n_max], float64, or float32 for a float32 x (filtered
    in float64, rounded once).  The edge polynomials are fitted to the row's own first and last window.  Host lengths below
    the window raise scipy's ValueError with the row named; such a row comes out NaN with device lengths."""
    import torch
    x2, lens = _ragged_args(x, lengths)
    W, p, deriv, delta = int(window_length), int(polyorder), int(deriv), float(delta)
    ragged.refuse_short(lens, x2.shape[1], W, ragged.SG_WINDOW_TEXT)
    tables = _device_tables(("sg", W, p, deriv, delta), x.device, lambda: savgol_tables(W, p, deriv, delta))
    was_f32 = x2.dtype == torch.float32
    if was_f32:
        x2 = x2.double()        # (the padding converts with the rows; it is never read)
    return _savgol(x2, tables, W, p, was_f32, ragged.counts_on_device(lens, x.device))


def _apply_filter_per_length(x, lens, sr, kw):
    """The per-length route of apply_filter_ragged_batch: applyFilter on every group of rows of one length (device lengths
    are read back first) -> float64 [rows, n_max], zeros behind each row's length.  Host lengths scipy refuses raise its
    ValueError with the row named; with device lengths such a row comes out NaN, as in the ragged kernels."""
    import torch
    on_host = isinstance(lens, np.ndarray)
    if not on_host:
        lens = lens.clamp(1, x.shape[1]).cpu().numpy()
    out = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for n, idx in ragged.group_rows(lens):
        ii = torch.from_numpy(idx).to(x.device)
        try:
            out[ii, :n] = applyFilter(x[ii, :n], sr, **kw)
        except ValueError as e:
            if on_host:
                raise RowRefused(str(e), idx[0], n) from e
            out[ii, :n] = float("nan")
    return out


def apply_filter_ragged_batch(x, lengths, sr, /, *, filt: str = "iir", cutOff=[None], filtLen: int = 6,
                              filtType: str = "low", polyOrd: int = 3, coeffs=None):
    """``applyFilter`` for a padded batch of device curves with a length per row: x float64 or float32 [rows, n_max] on the
    device (rows may be strided), ``lengths`` host integers or an int64 device tensor [rows] -> [rows, n_max]; row b holds
    ``applyFilter(x[b, :n_b], sr, ...)`` bit for bit in its first n_b columns and +0.0 behind them, in one ragged call: the
    launches of ONE single-length call at n_max, whatever the number of distinct lengths.  The columns of x at and behind
    n_b are never read.  float64 result, except 'sg' on float32 curves, which comes back float32, as applyFilter returns it.

    The routing is applyFilter's for device curves: 'iir' -> sosfiltfilt_ragged_batch; 'sg' and 'fir' through the banded
    operator (mm_stencil_ragged_f64) where they fit its struct (windows up to 16 samples, up to 8 taps), through
    savgol_ragged_batch / fir_filtfilt_ragged_batch beyond.  It raises applyFilter's exceptions for the same bad
    arguments.  Host lengths that scipy refuses raise scipy's ValueError with the row named (RowRefused) before any launch;
    device lengths are not read back, and such a row comes out NaN before its length.

    Two cases have no ragged kernel and keep the loop over the distinct lengths (applyFilter per group of rows of one
    length, device lengths read back first; same layout of the result): a float32 'fir' filter of at most 8 taps (its
    float32 odd extension is formed in torch around the banded operator), and 'iir' filters of more than 4 sections
    (time-major kernels)."""
    import torch
    from . import _lib
    kind = _validate(filt, cutOff, filtType, sr)
    kw = dict(filt=filt, cutOff=cutOff, filtLen=filtLen, filtType=filtType, polyOrd=polyOrd, coeffs=coeffs)
    x2, lens = _ragged_args(x, lengths)
    n_max = x2.shape[1]
    was_f32 = x2.dtype == torch.float32
    if filt == "iir":
        if coeffs is not None:
            sos = np.asarray(coeffs)
        else:
            _band_edges(cutOff, sr, kind)
            sos = _iir_design(sr, cutOff, filtLen, kind)
        if sos_sections(sos).shape[0] > _lib.MM_RAGGED_MAX_SEC:
            return _apply_filter_per_length(x2, lens, sr, kw)
        return sosfiltfilt_ragged_batch(x2, lens, sos)
    if filt == "sg":
        if len(cutOff) != 1:
            raise Exception(_MSG_SG)
        from .calc import apply_stencil_ragged, velocity_stencil
        try:
            st, _ = velocity_stencil(1.0, 0, "sg", filtLen, 2, polyOrd)
        except NotImplementedError:
            return savgol_ragged_batch(x2, lens, filtLen, polyOrd, deriv=0, delta=1.0)
        ragged.refuse_short(lens, n_max, len(st["c"]), ragged.SG_WINDOW_TEXT)
        y = apply_stencil_ragged(x2.double() if was_f32 else x2, ragged.counts_on_device(lens, x.device), st)
        return y.float() if was_f32 else y
    if filt == "fir":
        taps = np.asarray(coeffs) if coeffs is not None else \
            _sig.firwin(filtLen, _band_edges(cutOff, sr, kind), window=("kaiser", 7.4), pass_zero=kind)
        try:
            st = fir_filtfilt_stencil(taps)
        except NotImplementedError:
            st = None
        if st is not None:
            if was_f32:
                return _apply_filter_per_length(x2, lens, sr, kw)
            from .calc import apply_stencil_ragged
            pad = 3 * len(taps)
            ragged.refuse_short(lens, n_max, pad + 1, ragged.PADLEN_TEXT.format(pad))
            return apply_stencil_ragged(x2, ragged.counts_on_device(lens, x.device), st, n_min=pad + 1)
        if np.size(taps) >= 2:
            return fir_filtfilt_ragged_batch(x2, lens, taps)
        return _apply_filter_per_length(x2, lens, sr, kw)       # a single tap: scipy's own exception, through applyFilter
    raise UnboundLocalError(f"applyFilter: unknown filt {filt!r} (expected 'iir', 'fir' or 'sg')")


def applyFilter_batch(curves, sr, /, **kw):
    """``applyFilter`` for a list of 1-D curves of any lengths -> a list, each entry what ``applyFilter(curve, sr, **kw)``
    returns for the curve alone, bit for bit.  A numpy curve is filtered by the reference's own scipy call on the host, as
    applyFilter filters it, and comes back numpy.  The CUDA(HIP) curves form one padded batch per type (float32; float64
    and everything else, which applyFilter widens) and run through apply_filter_ragged_batch: one ragged call each instead
    of one call per distinct length.  A curve scipy refuses raises scipy's ValueError with the curve's index appended."""
    curves = list(curves)
    out = [None] * len(curves)
    on_device = [ragged.is_device_tensor(c) for c in curves]
    for i, c in enumerate(curves):
        if on_device[i] and c.dim() != 1:
            raise ValueError(f"curves must be [n] (curve {i})")
        if not on_device[i]:
            try:
                out[i] = applyFilter(c, sr, **kw)
            except ValueError as e:
                raise ragged.named(e, i, "curve")
    for idx, x, lens in ragged.packed_groups([c if d else None for c, d in zip(curves, on_device)]):
        if int(lens.min()) < 1:
            raise ValueError(f"curves must not be empty (curve {idx[int(lens.argmin())]})")
        try:
            y = apply_filter_ragged_batch(x, lens, sr, **kw)
        except RowRefused as e:
            raise ragged.named(e, idx[e.row], "curve")
        for b, i in enumerate(idx):
            out[i] = y[b, :lens[b]].clone()
    return out


def applyFilter(x, sr, /, *, filt: str = "iir", cutOff=[None], filtLen: int = 6,
                filtType: str = "low", polyOrd: int = 3, coeffs=None):
    """Zero-phase low / high / band-pass of ``x`` (sampled at ``sr`` Hz).

    filt      'iir' Butterworth of order ``filtLen`` (sosfiltfilt), 'fir' Kaiser(7.4) window of
              ``filtLen`` taps (filtfilt), 'sg' Savitzky-Golay window ``filtLen`` / order ``polyOrd``
    cutOff    one frequency (low/high-pass) or two increasing ones (band-pass), in Hz
    filtType  'low' | 'high' | 'band' (prefix match, as in the reference)
    coeffs    optional ready-made coefficients: SOS array for 'iir', taps for 'fir'.  (The
              reference accepts the argument but then dies on an unbound name; here it works.)

    Raises the reference's bare ``Exception`` messages for the same bad arguments.
    """
    kind = _validate(filt, cutOff, filtType, sr)
    if ragged.is_device_tensor(x):       # a batch of curves that lives on the GPU stays there
        return _apply_filter_device(x, sr, kind, filt=filt, cutOff=cutOff, filtLen=filtLen, polyOrd=polyOrd, coeffs=coeffs)

    if filt == "iir":
        sos = np.asarray(coeffs) if coeffs is not None else \
            _sig.butter(filtLen, _band_edges(cutOff, sr, kind), btype=kind, output="sos")
        return _sig.sosfiltfilt(sos, x)
    if filt == "fir":
        taps = np.asarray(coeffs) if coeffs is not None else \
            _sig.firwin(filtLen, _band_edges(cutOff, sr, kind), window=("kaiser", 7.4), pass_zero=kind)
        return _sig.filtfilt(taps, 1, x)
    if filt == "sg":
        if len(cutOff) != 1:
            raise Exception(_MSG_SG)
        return _sig.savgol_filter(x, filtLen, polyOrd, deriv=0, mode="interp")
    # unknown method: the reference falls through to `return y` with y never assigned
    raise UnboundLocalError(f"applyFilter: unknown filt {filt!r} (expected 'iir', 'fir' or 'sg')")
