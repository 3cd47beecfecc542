"""Drop-in for the part of the reference's ``script/calc.py`` that touches the MFCC path.

script/calc.py holds no MFCC arithmetic; what the north star names as the
drop-in surface is ``applyFilter`` (script/calc.py:23-129), ``get_velocity`` (:593-650, applied by
the UI to the MFCC-change curve, script/main.py:668-713) and the RMS / Hilbert amplitude envelope
(:221-343), the pYIN branch of ``get_f0`` with its ``interp_NAN`` (:345-592; modulation_mfcc_amd.pitch, .interp) and
``MinMaxFinder`` (:651-686: the peaks and troughs of a drawn curve, scipy.signal.find_peaks on the device --
``find_peaks_batch`` for [rows, n] device curves, ``find_peaks_ex_batch`` with scipy's remaining conditions).  Praat-backed
functions (f0 by 'praatac' / 'praatcc', formants, RMSpraat) are out of scope.  ``read_AG50x`` (:173-219), the
articulograph reader whose data that chain runs on, is modulation_mfcc_amd.ema.
"""
from __future__ import annotations

import numpy as np
from scipy.signal import savgol_filter

from . import ragged
from .filters import applyFilter
from .interp import interp_NAN, interp_nan_batch, interp_nan_ragged_batch  # noqa: F401
from .pitch import get_f0, get_f0_batch  # noqa: F401
from .ema import read_AG50x, read_AG50x_arrays, read_pos_header  # noqa: F401

__all__ = ["applyFilter", "get_f0", "get_f0_batch", "interp_NAN", "interp_nan_batch", "interp_nan_ragged_batch",
           "read_AG50x", "read_AG50x_arrays", "read_pos_header",
           "get_velocity", "calculate_amplitude_envelope", "velocity_stencil", "velocity_batch", "apply_stencil",
           "hilbert_envelope_batch", "amplitude_envelope_batch", "hilbert_envelope_ragged_batch",
           "amplitude_envelope_ragged_batch", "calculate_amplitude_envelope_batch", "find_peaks_batch", "find_peaks_ex_batch",
           "peaks_to_list", "MinMaxFinder"]


import collections

_HILBERT_PLANS = collections.OrderedDict()     # (n, dtype, device) -> _HilbertPlan, least recently used first
HILBERT_MAX_PLANS = 8           # every clip length has its own tables (a Bluestein length: ~13 n complex values)
HILBERT_WS_BYTES = 4 << 30      # workspace bound of one mm_hilbert_envelope call: batches are cut to fit


class _HilbertPlan:
    """Owner of one mm_hilbert handle (constant chirp / twiddle tables of one clip length on one device)."""

    def __init__(self, n, dtype_code, device, ragged=False):
        import ctypes as C
        import torch
        from . import _lib
        self._lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(device):
            if ragged:       # n: the longest clip of the transform length the handle is for
                _lib.check(self._lib.mm_hilbert_ragged_create(n, dtype_code, C.byref(h)), "mm_hilbert_ragged_create")
            else:
                _lib.check(self._lib.mm_hilbert_create(n, dtype_code, C.byref(h)), "mm_hilbert_create")
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._lib.mm_hilbert_destroy(self.h)
                self.h = None
        except Exception:
            pass


_HILBERT_RAGGED_PLANS = {}      # (M, dtype, device) -> _HilbertPlan of the ragged envelope: twiddle tables only (16 M / 1024 +
                                # 16 KiB bytes), at most 22 transform lengths -- kept, never evicted


def _hilbert_ragged_plan(M, code, device):
    """The mm_hilbert handle of the ragged envelope for the transform length M (mm_hilbert_ragged_create at the longest
    clip M takes, M / 2), kept per (M, dtype code, device) apart from the single-length plans' LRU."""
    key = (int(M), int(code), str(device))
    if key not in _HILBERT_RAGGED_PLANS:
        _HILBERT_RAGGED_PLANS[key] = _HilbertPlan(int(M) // 2, int(code), device, ragged=True)
    return _HILBERT_RAGGED_PLANS[key]


def _hilbert_plan(n, code, device):
    """The cached mm_hilbert handle of (length, dtype code, device) -- LRU of HILBERT_MAX_PLANS lengths."""
    key = (int(n), int(code), str(device))
    if key in _HILBERT_PLANS:
        _HILBERT_PLANS.move_to_end(key)
    else:
        import torch
        while len(_HILBERT_PLANS) >= HILBERT_MAX_PLANS:      # files of many different lengths: bounded table memory
            _, old = _HILBERT_PLANS.popitem(last=False)
            torch.cuda.synchronize(device)                    # nothing in flight may still read the tables
            del old
        _HILBERT_PLANS[key] = _HilbertPlan(int(n), int(code), device)
    return _HILBERT_PLANS[key]


def rfft_rows_long(x, n_fft, out=None):
    """np.fft.rfft(x, n_fft, axis=-1) of float32 device rows [R, T] (T <= n_fft, n_fft even and 2 / 3 / 5 / 7-smooth, in
    practice a power of two) -> complex64 [R, n_fft / 2 + 1]: the library's Stockham FFT in global memory
    (mm_hilbert_rfft_f32) -- the trajectory rFFT (row A8) of clips with more than 8192 frames, e.g. one recording at the
    reference's default 1 ms step (script/mfcc.py:296).  Rows are taken in chunks that bound the workspace."""
    import torch
    from . import _lib
    if not (ragged.is_device_tensor(x) and x.dtype == torch.float32 and x.dim() == 2):
        raise TypeError("x must be a float32 CUDA(HIP) tensor [rows, T]")
    if x.stride(1) != 1:
        x = x.contiguous()
    rows, T = x.shape
    n_fft = int(n_fft)
    if T < 1 or T > n_fft:
        raise ValueError("need 1 <= T <= n_fft")
    if out is None:
        out = torch.empty((rows, n_fft // 2 + 1), dtype=torch.complex64, device=x.device)
    plan = _hilbert_plan(n_fft, 0, x.device)
    lib = _lib.load()
    per_row = int(lib.mm_hilbert_rfft_workspace_bytes(plan.h, 1))
    chunk = int(max(1, min(rows, 65535, HILBERT_WS_BYTES // max(per_row, 1))))
    _lib.call_chunked("mm_hilbert_rfft_f32", x.device, rows, chunk,
                      lambda r0, r: (plan.h, x[r0:].data_ptr(), r, x.stride(0), T, out[r0:].data_ptr()),
                      lambda r: lib.mm_hilbert_rfft_workspace_bytes(plan.h, r))
    return out


def hilbert_envelope_batch(x):
    """|scipy.signal.hilbert(x)| along the last axis of a CUDA(HIP) tensor ([n] or [B, n], float32 or float64)
    on the device, in scipy's arithmetic: DFT of length N = len(x) in the input's precision, negative
    frequencies zeroed / positive ones doubled, inverse DFT, magnitude (script/calc.py:286).

    N is the clip length, an arbitrary integer: lengths of the form 2^a 3^b 5^c 7^d (160 000 = 2^8 * 5^4 for a 10 s
    clip, 441 000, 480 000 ...) are transformed directly by the library's mixed-radix Stockham FFT, any other length
    through Bluestein's chirp-z identity over a power-of-two FFT (mm_hilbert_envelope, csrc/mm_hilbert.hip.inc);
    the constant tables of a length are built once and kept (LRU of HILBERT_MAX_PLANS lengths)."""
    import torch
    from . import _lib
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float32, torch.float64)):
        raise TypeError("x must be a float32 / float64 CUDA(HIP) tensor")
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [B, n]")
    rows, n = x2.shape
    out = torch.empty((rows, n), dtype=x.dtype, device=x.device)
    if n == 0 or rows == 0:
        return out[0] if squeeze else out
    code = 0 if x.dtype == torch.float32 else 1
    plan = _hilbert_plan(n, code, x.device)
    lib = _lib.load()
    # two clips share one complex transform: calls of an even number of clips, sized by what a PAIR needs
    per_pair = int(lib.mm_hilbert_workspace_bytes(plan.h, 2))
    chunk = max(1, min(rows, 65534, 2 * (HILBERT_WS_BYTES // per_pair)))
    _lib.call_chunked("mm_hilbert_envelope", x.device, rows, chunk,
                      lambda r0, r: (plan.h, x2[r0:].data_ptr(), r, x2.stride(0), out[r0:].data_ptr(), n),
                      lambda r: lib.mm_hilbert_workspace_bytes(plan.h, r))
    return out[0] if squeeze else out


def hilbert_ragged_fft_size(n):
    """The power-of-two transform length of a clip of ``n`` samples in the ragged envelope: M = 2^p >= max(16, 2 n - 1)."""
    return max(16, 1 << (2 * int(n) - 2).bit_length())


def _hilbert_ragged_classes(lens):
    """Host lengths [B] -> [(M, int64 index array of the rows whose own transform length is M)], ascending M."""
    return ragged.group_rows([hilbert_ragged_fft_size(n) for n in lens])


def _hilbert_ragged_rows(x2, lens_dev, M):
    """mm_hilbert_envelope_ragged on x2 [rows, n_max] (unit inner stride) with device lengths, through the transform length
    ``M`` >= 2 n_max - 1 -> [rows, n_max]; the rows are cut into calls of at most HILBERT_WS_BYTES of workspace."""
    import torch
    from . import _lib
    rows, n = x2.shape
    code = 0 if x2.dtype == torch.float32 else 1
    plan = _hilbert_ragged_plan(M, code, x2.device)
    lib = _lib.load()
    out = torch.empty((rows, n), dtype=x2.dtype, device=x2.device)
    per_row = int(lib.mm_hilbert_ragged_workspace_bytes(plan.h, 1, n))
    chunk = int(max(1, min(rows, 65535, HILBERT_WS_BYTES // max(per_row, 1))))
    _lib.call_chunked("mm_hilbert_envelope_ragged", x2.device, rows, chunk,
                      lambda r0, r: (plan.h, x2[r0:].data_ptr(), r, n, ragged.row_pitch(x2), lens_dev[r0:].data_ptr(),
                                     out[r0:].data_ptr(), n),
                      lambda r: lib.mm_hilbert_ragged_workspace_bytes(plan.h, r, n))
    return out


def hilbert_envelope_ragged_batch(x, lengths):
    """hilbert_envelope_batch for clips of different lengths in one padded batch: ``x`` [B, n_max] (float32 or float64 on the
    device, rows may be strided) and one valid sample count per clip -> [B, n_max] of the same type.  Row b holds
    |scipy.signal.hilbert(x[b, :n_b])| -- the DFT at the clip's OWN length -- in its first n_b columns and +0.0 behind them;
    what the padding of ``x`` holds never matters, and a NaN or an infinity inside a clip makes that row NaN and no other.

    Every clip goes through Bluestein's identity with its own chirp over a shared power-of-two FFT (mm_hilbert_envelope_
    ragged): no tables per length; the handle of a transform length M (its twiddle tables) is kept for good.
    ``lengths``: host integers (validated: ValueError outside [1, n_max]) -- the rows are then grouped by their own M =
    2^p >= max(16, 2 n_b - 1), one ragged call per class, so a short clip does not pay for a long neighbour's transform and
    a row's result depends on its own length only -- or an int64 device tensor (no read-back; the kernels clamp it; one class,
    that of n_max).  Calls are cut to HILBERT_WS_BYTES of workspace.

    The clips are transformed as they are, without hilbert_envelope_batch's per-clip power-of-two scaling (that serves its
    pairing): the unnormalised transforms reach max(envelope) n_b M, so a float32 clip stays finite where scipy does only
    while that product is below 3.4e38 -- amplitudes up to about 1e27 at ten seconds of 16 kHz, 6e23 at 2^24 samples."""
    import torch
    x = ragged.device_rows(x, (torch.float32, torch.float64), "x must be a float32 / float64 CUDA(HIP) tensor",
                           "x must be [B, n_max], at least one row and one column")
    B, n_max = x.shape
    lens = ragged.check_lengths(lengths, B, n_max, x.device)
    if not isinstance(lens, np.ndarray):
        return _hilbert_ragged_rows(x, lens, hilbert_ragged_fft_size(n_max))
    out = None
    for M, idx in _hilbert_ragged_classes(lens):
        n_c = int(lens[idx].max())              # the class's calls are cut to its longest clip: M covers n_c, not n_max
        lens_c = ragged.counts_on_device(lens[idx], x.device)
        if len(idx) == B and n_c == n_max:      # one class that fills the batch: as it is, no gather
            return _hilbert_ragged_rows(x, lens_c, M)
        if out is None:
            out = torch.zeros((B, n_max), dtype=x.dtype, device=x.device)
        if len(idx) == B:
            out[:, :n_c] = _hilbert_ragged_rows(x[:, :n_c], lens_c, M)
        else:
            ii = torch.from_numpy(idx).to(x.device)
            out[ii, :n_c] = _hilbert_ragged_rows(x[ii, :n_c], lens_c, M)
    return out


def amplitude_envelope_ragged_batch(x, lengths, sr, *, method: str = "RMS", winLen: float = 0.1, hopLen: float = 0.01,
                                    center: bool = True):
    """amplitude_envelope_batch for a padded batch with a length per clip: ``x`` [B, n_max] on the device, ``lengths`` host
    integers or an int64 device tensor -> (env [B, n_out_max], out_lengths, sample rate of the envelope).  Row b holds what
    amplitude_envelope_batch gives for x[b, :lengths[b]] alone in its first out_lengths[b] columns ('RMS': bit for bit,
    batch.rms_ragged_batch; 'Hilb': hilbert_envelope_ragged_batch) and +0.0 behind them.  ``out_lengths`` is a numpy array
    for host lengths and a device tensor for device lengths (the clamped lengths for 'Hilb', the frame counts for 'RMS')."""
    from .batch import rms_ragged_batch

    def seen():     # the lengths as the kernels see them: device lengths clamped, with no read-back
        return lengths.clamp(1, x.shape[1]) if ragged.is_device_tensor(lengths) else np.asarray(lengths, dtype=np.int64)
    if method == "Hilb":
        env = hilbert_envelope_ragged_batch(x, lengths)
        return env, seen(), 1 / hopLen                    # the reference's rate quirk, as in amplitude_envelope_batch
    if method == "RMS":
        import torch
        xf = x if x.dtype == torch.float32 else x.float()
        frame, hop = int(winLen * sr), int(hopLen * sr)
        env = rms_ragged_batch(xf, lengths, frame, hop, center)
        return env, ragged.centered_frames(seen(), frame, hop, center), 1 / hopLen
    _envelope_method(method)        # neither: its refusal


def amplitude_envelope_batch(x, sr, *, method: str = "RMS", winLen: float = 0.1, hopLen: float = 0.01,
                             center: bool = True):
    """The envelope of calculate_amplitude_envelope (script/calc.py:284-343, before its output filter) for a
    batch of clips on the device: [B, n] (or [n]) CUDA(HIP) tensor -> ([B, n_out], sample rate of the envelope).
    'RMS' = librosa.feature.rms(frame_length=int(winLen*sr), hop_length=int(hopLen*sr), center, pad_mode=
    'constant') through mm_rms_f32, 'Hilb' = |hilbert(x)| (hilbert_envelope_batch)."""
    from .batch import rms_batch
    if method == "Hilb":
        return hilbert_envelope_batch(x), 1 / hopLen      # the reference's rate quirk, see below
    if method == "RMS":
        import torch
        xf = x if x.dtype == torch.float32 else x.float()
        squeeze = xf.dim() == 1
        env = rms_batch(xf, int(winLen * sr), int(hopLen * sr), center)
        return (env[0] if squeeze else env), 1 / hopLen
    _envelope_method(method)        # neither: its refusal


def _envelope_method(method):
    """The refusals of calculate_amplitude_envelope and its list form."""
    if method == "RMSpraat":
        raise NotImplementedError("method='RMSpraat' calls Praat through parselmouth; not part of this build")
    if method not in ("Hilb", "RMS"):
        raise UnboundLocalError(f"unknown amplitude method {method!r}")   # reference: `amp` unbound


def _envelope_signal(x, method):
    """The signal of calculate_amplitude_envelope and its list form on the device: a CUDA(HIP) tensor as it is, a host
    signal in the precision the reference computes it in -- librosa.feature.rms / scipy.signal.hilbert keep float32 input
    in single precision, anything else in double."""
    if ragged.is_device_tensor(x):
        return x
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("modulation_mfcc_amd needs an AMD GPU (gfx950); there is no CPU fallback")
    xa = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(xa, dtype=np.float32 if (method == "RMS" or xa.dtype == np.float32)
                                                 else np.float64)).cuda()


def calculate_amplitude_envelope(x, sr, /, *, method: str = "RMS", winLen: float = 0.1,
                                 hopLen: float = 0.01, center: bool = True, outFilter=None,
                                 outFiltType: str = "low", outFiltCutOff=[12], outFiltLen: int = 6,
                                 outFiltPolyOrd: int = 3):
    """script/calc.py:221-343.  'RMS' and 'Hilb'; 'RMSpraat' needs Praat (out of scope).

    The envelope is computed on the GPU (framewise RMS: mm_rms_f32; Hilbert: device FFT).  A numpy signal
    returns numpy arrays like the reference (its output filter, a short per-frame curve, then runs through the
    reference's own scipy calls on the host); a CUDA(HIP) tensor ([n] or a batch [B, n]) returns device tensors and
    is filtered on the device too (applyFilter's device branch)."""
    _envelope_method(method)
    on_device = ragged.is_device_tensor(x)
    xd = _envelope_signal(x, method)
    env, env_sr = amplitude_envelope_batch(xd, sr, method=method, winLen=winLen, hopLen=hopLen, center=center)
    # the reference tests method != 'hilb' (lower case), so 'Hilb' ALSO gets hop-spaced time stamps
    # and the 1/hopLen rate for its output filter (script/calc.py:333-337); kept as is.
    times = np.arange(env.shape[-1]) * hopLen
    if not on_device:
        env = env.cpu().numpy()
    if outFilter is not None:
        env = applyFilter(env, env_sr, filt=outFilter, filtType=outFiltType, cutOff=outFiltCutOff,
                          filtLen=outFiltLen, polyOrd=outFiltPolyOrd)
    return env, times


def calculate_amplitude_envelope_batch(clips, sr, /, *, method: str = "RMS", winLen: float = 0.1, hopLen: float = 0.01,
                                       center: bool = True, outFilter=None, outFiltType: str = "low", outFiltCutOff=[12],
                                       outFiltLen: int = 6, outFiltPolyOrd: int = 3):
    """``calculate_amplitude_envelope`` for a list of clips of any lengths ([n] each, numpy or CUDA(HIP) tensors) -> a list of
    ``(amp, ampT)``, one per clip, each what the single call returns for that clip: numpy ``amp`` for a numpy clip, a device
    tensor for a device clip, ``ampT = np.arange(len(amp)) * hopLen`` for both methods (the reference's 'hilb' quirk).

    The clips are packed (batch.pack_clips) and run through amplitude_envelope_ragged_batch: 'RMS' as one float32 batch,
    'Hilb' as one batch of its float32 clips and one of the others (float64), each clip in the precision it has alone.
    ``outFilter`` is ONE filters.apply_filter_ragged_batch on the padded envelopes at the rate 1 / hopLen -- for numpy clips
    too, whose single call filters with scipy on the host (equal to rounding) -- and one copy brings the numpy results back.
    A clip the single call refuses raises that call's exception with the clip's index appended."""
    _envelope_method(method)
    import torch
    from .batch import pack_clips
    from .filters import apply_filter_ragged_batch
    clips = list(clips)
    on_device = [ragged.is_device_tensor(c) for c in clips]
    sigs = [_envelope_signal(c, method) for c in clips]
    for i, c in enumerate(sigs):
        if method == "RMS":
            sigs[i] = c = c if c.dtype == torch.float32 else c.float()
        elif c.dtype not in (torch.float32, torch.float64):
            raise ragged.named(TypeError("x must be a float32 / float64 CUDA(HIP) tensor"), i)
        if c.dim() != 1 or c.shape[0] < 1:
            raise ragged.named(ValueError("every clip must be [n] with at least one sample"), i)
    kw = dict(method=method, winLen=winLen, hopLen=hopLen, center=center)
    out = [None] * len(clips)
    for idx in ragged.split_by_dtype(sigs):
        if not idx:
            continue
        x, lengths = pack_clips([sigs[i] for i in idx], sigs[idx[0]].dtype)
        try:
            env, out_len, env_sr = amplitude_envelope_ragged_batch(x, lengths.numpy(), sr, **kw)
        except ValueError as e:
            ragged.blame_clip(e, lambda b: amplitude_envelope_batch(sigs[idx[b]], sr, **kw), idx)
        if outFilter is not None:
            try:
                env = apply_filter_ragged_batch(env, out_len, env_sr, filt=outFilter, filtType=outFiltType,
                                                cutOff=outFiltCutOff, filtLen=outFiltLen, polyOrd=outFiltPolyOrd)
            except ragged.RowRefused as e:                        # (an envelope too short for the filter)
                raise ragged.named(e, idx[e.row])
        host = None if all(on_device[i] for i in idx) else env.cpu().numpy()
        for b, i in enumerate(idx):
            n = int(out_len[b])
            out[i] = (env[b, :n].clone() if on_device[i] else host[b, :n].copy(), np.arange(n) * hopLen)
    return out


def _findiff_first_axis(x, h, order, acc):
    """Central finite differences of accuracy ``acc`` with one-sided stencils at the edges --
    the behaviour of findiff.FinDiff(0, h, order, acc=acc) used at script/calc.py:636."""
    x = np.asarray(x, dtype=float)
    n = x.shape[0]
    half = (order + 1) // 2 - 1 + acc // 2        # central stencil half-width
    width_edge = order + acc                      # one-sided stencil points

    def weights(offsets):
        offsets = np.asarray(offsets, dtype=float)
        m = len(offsets)
        A = np.vander(offsets, m, increasing=True).T
        rhs = np.zeros(m)
        rhs[order] = float(np.prod(np.arange(1, order + 1)))
        return np.linalg.solve(A, rhs)

    if n < max(2 * half + 1, width_edge):
        raise ValueError("signal too short for the requested finite-difference stencil")
    out = np.empty_like(x)
    c_off = np.arange(-half, half + 1)
    c_w = weights(c_off)
    for i in range(n):
        if i < half:
            off = np.arange(0, width_edge)
        elif i >= n - half:
            off = np.arange(-(width_edge - 1), 1)
        else:
            off = None
        if off is None:
            out[i] = np.tensordot(c_w, x[i + c_off], axes=(0, 0))
        else:
            out[i] = np.tensordot(weights(off), x[i + off], axes=(0, 0))
    return out / h ** order


def _fd_weights(offsets, order):
    """Finite-difference weights of the ``order``-th derivative on integer ``offsets`` (unit spacing)."""
    offsets = np.asarray(offsets, dtype=float)
    m = len(offsets)
    A = np.vander(offsets, m, increasing=True).T
    rhs = np.zeros(m)
    rhs[order] = float(np.prod(np.arange(1, order + 1)))
    return np.linalg.solve(A, rhs)


def velocity_stencil(sr: float, difference: int = 1, method: str = "gradient", width: int = 3,
                     accOrder: int = 2, polyOrder: int = 2):
    """The derivative of get_velocity (script/calc.py:593-650) as the banded operator mm_stencil_f64 applies:
    (stencil dict, passes).  'gradient' is ONE first-derivative stencil applied ``difference`` times, exactly
    as the reference loops np.gradient.  Raises NotImplementedError when the stencil does not fit the C
    struct (windows wider than 16 samples, edge zones longer than 8): velocity_batch then runs 'sg' through
    filters.savgol_batch (any window, on the device); only 'finDiff' beyond the struct uses the host path."""
    from . import _lib
    W, E = _lib.MM_ST_MAXW, _lib.MM_ST_MAXE
    if method == "gradient":
        h = 1 / sr      # np.gradient(x, h): (x[i+1] - x[i-1]) / (2 h) inside, first-order differences at the ends
        return dict(off=[-1, 1], c=[-1.0, 1.0], den_c=2.0 * h, n_edge=1, edge_w=2,
                    el=[[-1.0, 1.0]], er=[[-1.0, 1.0]], den_e=h), int(difference)
    if method == "sg":
        from scipy.signal import savgol_coeffs
        width, polyOrder, difference = int(width), int(polyOrder), int(difference)
        half = width // 2
        if width > W or half > E:
            raise NotImplementedError("Savitzky-Golay window too wide for the device stencil")
        conv = savgol_coeffs(width, polyOrder, deriv=difference, delta=1.0)    # taps of scipy's convolve1d
        c = conv[::-1]                                                         # as a correlation: x[i - half + k]
        # mode='interp': the first / last half samples come from the polynomial fitted to the first / last
        # window (scipy.signal._savitzky_golay._fit_edge); linear in the window -> fit unit vectors
        t = np.arange(width)
        pc = np.polyfit(t, np.eye(width), polyOrder)                           # [polyOrder + 1, width]
        for _ in range(difference):
            pc = pc[:-1] * np.arange(pc.shape[0] - 1, 0, -1)[:, None] if pc.shape[0] > 1 else np.zeros((1, width))
        el = [[float(np.polyval(pc[:, j], i)) for j in range(width)] for i in range(half)]
        er = [[float(np.polyval(pc[:, j], width - half + i)) for j in range(width)] for i in range(half)]
        # scipy's convolve1d puts an even kernel's centre at width // 2: as a correlation the taps sit on
        # x[i - (width - 1) // 2 .. i + width // 2] (odd width: -half .. half; width 6, the reference's default
        # outFiltLen: -2 .. 3)
        off = list(range(-((width - 1) // 2), width // 2 + 1))
        assert len(off) == len(c) == width
        return dict(off=off, c=[float(v) for v in c], den_c=1.0, n_edge=half, edge_w=width,
                    el=el, er=er, den_e=1.0), 1
    if method == "finDiff":
        order, acc = int(difference), int(accOrder)
        half = (order + 1) // 2 - 1 + acc // 2
        we = order + acc
        ew = half - 1 + we if half > 0 else we
        if 2 * half + 1 > W or ew > W or half > E:
            raise NotImplementedError("finite-difference stencil too wide for the device stencil")
        c_off = list(range(-half, half + 1))
        el = [[0.0] * ew for _ in range(half)]
        er = [[0.0] * ew for _ in range(half)]
        for i in range(half):
            w = _fd_weights(np.arange(0, we), order)             # forward stencil on samples i .. i + we - 1
            for k in range(we):
                el[i][i + k] = float(w[k])
            # output n - half + i: backward stencil on samples i' - (we - 1) .. i', as positions in the last ew
            w = _fd_weights(np.arange(-(we - 1), 1), order)
            pos = ew - half + i
            for k in range(we):
                er[i][pos - (we - 1) + k] = float(w[k])
        h = 1 / sr
        return dict(off=c_off, c=[float(v) for v in _fd_weights(c_off, order)], den_c=h ** order, n_edge=half,
                    edge_w=ew, el=el, er=er, den_e=h ** order), 1
    raise ValueError("Méthode inconnue. Utilisez 'gradient', 'sg' ou 'finDiff'.")


def _c_stencil(st, n_min: int = 0):
    """The C struct mm_stencil of a stencil dict; ``n_min`` (the ragged entry only) is the shortest row the caller takes."""
    from . import _lib
    cs = _lib.mm_stencil()
    if len(st["off"]) != len(st["c"]):
        raise ValueError("stencil: one offset per tap")
    cs.n_c, cs.n_edge, cs.edge_w, cs.reserved = len(st["c"]), st["n_edge"], st["edge_w"], int(n_min)
    for k, (o, c) in enumerate(zip(st["off"], st["c"])):
        cs.off[k], cs.c[k] = o, c
    for i in range(st["n_edge"]):
        for j in range(st["edge_w"]):
            cs.el[i][j], cs.er[i][j] = st["el"][i][j], st["er"][i][j]
    cs.den_c, cs.den_e = st["den_c"], st["den_e"]
    return cs


def apply_stencil_ragged(x2, lens_dev, st, n_min: int = 0):
    """The banded operator ``st`` once along the last axis of a float64 CUDA(HIP) tensor [rows, n_max] with unit inner
    stride, a length per row (``lens_dev``: int64 device tensor [rows]; mm_stencil_ragged_f64): row b equals
    apply_stencil on x2[b:b+1, :n_b] bit for bit in its first n_b columns and is +0.0 behind them; nothing at or behind n_b
    is read.  A row shorter than the operator takes (or than ``n_min``) comes out NaN."""
    return _stencil(x2, _c_stencil(st, n_min), lens_dev)


def _stencil(x2, cs, d_lens=None):
    """One pass of the C stencil ``cs``: mm_stencil_f64 (``d_lens`` None) or mm_stencil_ragged_f64 -> float64 [rows, n]."""
    import ctypes as C
    import torch
    from . import _lib
    rows, n = x2.shape
    out = torch.empty((rows, n), dtype=torch.float64, device=x2.device)
    _lib.call("mm_stencil_f64" if d_lens is None else "mm_stencil_ragged_f64", x2.device, C.byref(cs), x2.data_ptr(), rows, n,
              ragged.row_pitch(x2), *ragged.lens_arg(d_lens), out.data_ptr())
    return out


def apply_stencil(x2, st, passes: int = 1):
    """Run the banded operator ``st`` (dict: off, c, den_c, n_edge, edge_w, el, er, den_e -- the fields of the C
    struct mm_stencil) ``passes`` times along the last axis of a float64 CUDA(HIP) tensor [rows, n] with unit
    inner stride (mm_stencil_f64)."""
    cs = _c_stencil(st)
    src = x2
    for _ in range(passes):
        src = _stencil(src, cs)
    return src


def velocity_batch(x, sr: float, difference: int = 1, method: str = "gradient", width: int = 3,
                   accOrder: int = 2, polyOrder: int = 2):
    """get_velocity along the LAST axis of a float64 CUDA(HIP) tensor [rows, n] (or [n]) on the device
    (mm_stencil_f64; row N2) -- e.g. on the [B, T] output of MfccPlan.mfcc_change.  'gradient' equals
    np.gradient(x, 1/sr) bit for bit, 'sg' / 'finDiff' agree with scipy / findiff to float64 round-off; 'sg' windows of
    more than 16 samples run through filters.savgol_batch (mm_savgol_f64), any width up to the row's length.  A float32
    tensor (an RMS envelope) comes back float32 for 'gradient' / 'sg', as numpy / scipy return it, to float32 round-off."""
    import torch
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float64, torch.float32)):
        raise TypeError("x must be a float64 (or float32) CUDA(HIP) tensor")
    if x.dtype == torch.float32:
        # numpy / scipy keep a float32 curve float32 for 'gradient' and 'sg' (np.gradient in float32 arithmetic,
        # savgol_filter in double, rounded once); here: float64 on the device, rounded once -- equal to float32 round-off
        y = velocity_batch(x.double(), sr, difference, method, width, accOrder, polyOrder)
        return y.float() if method in ("gradient", "sg") else y
    try:
        st, passes = velocity_stencil(sr, difference, method, width, accOrder, polyOrder)
    except NotImplementedError:
        if method != "sg":
            raise
        from .filters import savgol_batch       # windows beyond the stencil: mm_savgol_f64 (delta 1, as the reference calls it)
        return savgol_batch(x, width, polyOrder, deriv=difference, delta=1.0)
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [rows, n]")
    rows, n = x2.shape
    if method == "sg" and n < len(st["c"]):       # scipy.signal.savgol_filter's own check and message
        raise ValueError(ragged.SG_WINDOW_TEXT)
    if n < max(2 * st["n_edge"], st["edge_w"]):
        raise ValueError("signal too short for the requested finite-difference stencil")
    src = apply_stencil(x2, st, passes)
    return src[0] if squeeze else src


def get_velocity(x: np.ndarray, sr: float, difference: int = 1, method: str = "gradient",
                 width: int = 3, accOrder: int = 2, polyOrder: int = 2):
    """First or second derivative of ``x`` (sampled at ``sr``) -- script/calc.py:593-650.

    method 'gradient' (np.gradient, repeated ``difference`` times), 'sg' (Savitzky-Golay with
    ``width`` points and polynomial order ``polyOrder``) or 'finDiff' (finite-difference stencils
    of accuracy ``accOrder``).  Unknown methods raise the reference's ValueError.

    A float64 CUDA(HIP) tensor (a curve, or [rows, n] curves along the last axis) is differentiated on
    the device (``velocity_batch``: 'gradient', 'sg' of any width, 'finDiff' stencils that fit mm_stencil; a wider
    'finDiff' stencil makes the round trip through the host); numpy input keeps the reference's host arithmetic.
    """
    if ragged.is_device_tensor(x):
        if method not in ("gradient", "sg", "finDiff"):
            raise ValueError("Méthode inconnue. Utilisez 'gradient', 'sg' ou 'finDiff'.")
        try:
            return velocity_batch(x, sr, difference, method, width, accOrder, polyOrder)
        except NotImplementedError:
            import torch
            y = get_velocity(x.cpu().numpy().T, sr, difference, method, width, accOrder, polyOrder)
            return torch.from_numpy(np.ascontiguousarray(np.asarray(y).T)).to(x.device)
    if method == "finDiff":
        return _findiff_first_axis(x, 1 / sr, difference, accOrder)
    if method == "sg":
        return savgol_filter(x, width, polyOrder, deriv=difference, axis=0, mode="interp")
    if method == "gradient":
        for _ in range(difference):
            x = np.gradient(x, 1 / sr)
        return x
    raise ValueError("Méthode inconnue. Utilisez 'gradient', 'sg' ou 'finDiff'.")


FIND_PEAKS_SEGMENT = 1024       # samples per workgroup of the peak kernels (csrc/mm_peaks.hip: kPkThreads * kPkPer)


def _peak_interval(name, v):
    """scipy's _unpack_condition_args for scalar bounds: a number is the minimum, a pair is (min, max), None an open side."""
    import math
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name} must be a number or a (min, max) pair")
        vmin, vmax = v
    else:
        vmin, vmax = v, None
    out = []
    for b, open_side in ((vmin, -math.inf), (vmax, math.inf)):
        if b is None:
            out.append(open_side)
            continue
        if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name}: bounds must be real numbers or None (per-sample arrays are not supported)")
        if math.isnan(float(b)):
            raise ValueError(f"{name}: bounds must not be NaN")
        out.append(float(b))
    return out


def _peak_range(name, v, rows, n, device):
    """lo / hi of find_peaks_batch as an int32 device tensor [rows] (None stays None)."""
    import torch
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.dtype not in (torch.int32, torch.int64) or v.numel() != rows:
            raise TypeError(f"{name} must be an int32 / int64 tensor with one entry per row")
        return v.reshape(rows).to(device=device, dtype=torch.int32).contiguous()
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name} must be an integer, a sequence of integers or an integer tensor")
    a = np.broadcast_to(a.astype(np.int64), (rows,)) if a.ndim == 0 else a.astype(np.int64).reshape(-1)
    if a.shape != (rows,):
        raise ValueError(f"{name} must have one entry per row")
    if (a < 0).any() or (a > n).any():
        raise ValueError(f"{name} must lie in [0, n]")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def find_peaks_batch(x, *, negate=False, height=None, threshold=None, prominence=None, lo=None, hi=None):
    """scipy.signal.find_peaks along the LAST axis of a float64 / float32 CUDA(HIP) tensor [rows, n] (or [n]) on the
    device (mm_find_peaks) -- e.g. on the [B, T] output of MfccPlan.mfcc_change, velocity_batch or pyin_batch.

    Returns ``(idx, count, props)``, all on the device, nothing synchronised: ``idx`` int32 [rows, cap] holds each row's
    peak indices ascending, padded with -1, ``count`` int32 [rows] their number, ``cap = max(0, (n - 1) // 2)`` the most a
    row can have.  Indices, bases and prominences equal scipy's bit for bit (float32 input is promoted to float64 per
    element, as scipy does).

    ``negate=True`` finds the peaks of ``-x`` (the troughs) without a negated copy; heights, thresholds and prominences
    are then those of ``-x``, as ``find_peaks(-x, ...)`` returns them.  ``height``, ``threshold`` and ``prominence`` are
    a minimum, or ``(min, max)`` with ``None`` for an open side, applied in scipy's order; ``props`` holds
    ``peak_heights``, ``left_thresholds`` / ``right_thresholds``, ``prominences`` / ``left_bases`` / ``right_bases``,
    each exactly when scipy returns it, shaped like ``idx`` (NaN / -1 beyond the count).  ``lo`` / ``hi`` (an integer, one
    per row, or an integer tensor; tensors are clamped to 0 <= lo <= hi <= n on the device) restrict row r to
    ``x[r, lo:hi]``: the result is scipy's on that slice, indices relative to ``lo``.  ``distance``, ``width``, ``wlen``
    and ``plateau_size`` are those of ``find_peaks_ex_batch``, of which this function is the subset that needs no
    candidate stages.  A 1-D input gives 1-D outputs."""
    return _find_peaks(x, negate, height, threshold, prominence, lo, hi, None)


def find_peaks_ex_batch(x, *, negate=False, height=None, threshold=None, distance=None, prominence=None, width=None,
                        wlen=None, rel_height=0.5, plateau_size=None, lo=None, hi=None):
    """``find_peaks_batch`` with every condition of scipy.signal.find_peaks (mm_find_peaks_ex): input, ``(idx, count,
    props)``, ``negate``, ``lo`` / ``hi``, the 1-D squeeze and the TypeErrors are those of ``find_peaks_batch``; with only
    its arguments the same kernels run.

    The conditions are applied in scipy's order -- ``plateau_size``, ``height``, ``threshold``, ``distance``,
    ``prominence``, ``width`` -- and ``props`` holds exactly the keys scipy returns for the same arguments, shaped like
    ``idx``: ``plateau_sizes`` / ``left_edges`` / ``right_edges`` (int32, -1 beyond the count), ``peak_heights``,
    ``left_thresholds`` / ``right_thresholds``, ``prominences`` / ``left_bases`` / ``right_bases`` (with ``width`` alone
    too), ``widths`` / ``width_heights`` / ``left_ips`` / ``right_ips`` (float64, NaN beyond the count; positions relative
    to ``lo``).  Every value equals scipy's bit for bit.

    ``plateau_size`` and ``width`` are a minimum or ``(min, max)`` with ``None`` for an open side.  ``distance`` is a real
    number >= 1, used as ``ceil(distance)``.  ``wlen`` is looked at only when ``prominence`` or ``width`` is given, as in
    scipy: ``None`` is no window, a value > 1 is used as ``ceil(wlen)``, the window being ``[p - wlen // 2, p + wlen // 2]``
    clipped to the row (to ``x[r, lo:hi]``).  ``rel_height`` >= 0 is that of scipy.signal.peak_widths.  scipy's
    PeakPropertyWarning is not emitted.

    Tied heights under ``distance``: scipy ranks the peaks with an unstable ``np.argsort``, so which of two equally high
    peaks nearer than ``distance`` survives is not defined there.  Here the peak with the LARGER index has priority (a
    stable argsort walked from its end)."""
    import math
    ext = {"plateau_size": None, "distance": 0, "width": None, "wlen": 0, "rel_height": float(rel_height)}
    if plateau_size is not None:
        ext["plateau_size"] = _peak_interval("plateau_size", plateau_size)
    if distance is not None:
        if isinstance(distance, bool) or not isinstance(distance, (int, float, np.integer, np.floating)):
            raise TypeError("distance must be a real number")
        if not distance >= 1:
            raise ValueError("`distance` must be greater or equal to 1")
        ext["distance"] = min(int(math.ceil(distance)), 0x7fffffff)
    if width is not None:
        ext["width"] = _peak_interval("width", width)
    if prominence is not None or width is not None:
        if wlen is not None:
            if isinstance(wlen, bool) or not isinstance(wlen, (int, float, np.integer, np.floating)):
                raise TypeError("wlen must be a real number")
            if not 1 < wlen:
                raise ValueError(f"`wlen` must be larger than 1, was {wlen}")
            ext["wlen"] = min(int(wlen) if isinstance(wlen, (int, np.integer)) else int(math.ceil(wlen)), 0x7fffffff)
        if width is not None and rel_height < 0:
            raise ValueError("`rel_height` must be greater or equal to 0.0")
    if not ext["rel_height"] >= 0:
        ext["rel_height"] = 0.0                                 # unused without width; the C entry refuses it always
    return _find_peaks(x, negate, height, threshold, prominence, lo, hi, ext)


def _find_peaks(x, negate, height, threshold, prominence, lo, hi, ext):
    """find_peaks_batch (ext None: mm_find_peaks) and find_peaks_ex_batch (ext: the checked extra conditions)."""
    import ctypes as C
    import math
    import torch
    from . import _lib
    if not (ragged.is_device_tensor(x) and x.dtype in (torch.float64, torch.float32)):
        raise TypeError("x must be a float64 (or float32) CUDA(HIP) tensor")
    x2, squeeze = ragged.batch_rows(x, "x must be [n] or [rows, n]", pitched=True)
    o = _lib.mm_peaks_opts()
    o.negate = 1 if negate else 0
    for name, v, field in (("height", height, o.height), ("threshold", threshold, o.threshold),
                           ("prominence", prominence, o.prominence)):
        field[0], field[1] = _peak_interval(name, v) if v is not None else (-math.inf, math.inf)
        setattr(o, "use_" + name, 0 if v is None else 1)
    rows, n = x2.shape
    dev = x2.device
    d_lo, d_hi = _peak_range("lo", lo, rows, n, dev), _peak_range("hi", hi, rows, n, dev)
    cap = max(0, (n - 1) // 2)
    idx = torch.empty((rows, cap), dtype=torch.int32, device=dev)
    count = torch.zeros((rows,), dtype=torch.int32, device=dev)
    props = {}
    prom = lb = rb = None
    f64 = lambda: torch.empty((rows, cap), dtype=torch.float64, device=dev)     # noqa: E731
    i32 = lambda: torch.empty((rows, cap), dtype=torch.int32, device=dev)       # noqa: E731
    plateau = ext is not None and ext["plateau_size"] is not None
    widths = ext is not None and ext["width"] is not None
    if prominence is not None or widths:
        prom, lb, rb = f64(), i32(), i32()
    wout = [f64() for _ in range(4)] if widths else [None] * 4
    pout = [i32() for _ in range(3)] if plateau else [None] * 3
    if rows > 0 and n > 0:
        lib = _lib.load()
        stride = ragged.row_pitch(x2)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        dtype = 0 if x2.dtype == torch.float32 else 1
        if ext is None:
            ws = _lib.workspace(lib.mm_find_peaks_workspace_bytes(rows, n), dev)
            _lib.call("mm_find_peaks", dev, C.byref(o), x2.data_ptr(), dtype, rows, n, stride, ptr(d_lo), ptr(d_hi), cap,
                      count.data_ptr(), ptr(idx), ptr(prom), ptr(lb), ptr(rb), ws.data_ptr(), ws.numel())
        else:
            e = _lib.mm_peaks_ext()
            for name, use in (("plateau_size", plateau), ("width", widths)):
                field = getattr(e, name)
                field[0], field[1] = ext[name] if use else (-math.inf, math.inf)
                setattr(e, "use_" + name, 1 if use else 0)
            e.rel_height, e.wlen = ext["rel_height"], ext["wlen"]
            e.distance, e.use_distance = ext["distance"], 1 if ext["distance"] else 0
            out = _lib.mm_peaks_out(count.data_ptr(), ptr(idx), ptr(prom), ptr(lb), ptr(rb), *(ptr(t) for t in wout + pout))
            ws = _lib.workspace(lib.mm_find_peaks_ex_workspace_bytes(C.byref(o), C.byref(e), rows, n), dev)
            _lib.call("mm_find_peaks_ex", dev, C.byref(o), C.byref(e), x2.data_ptr(), dtype, rows, n, stride, ptr(d_lo),
                      ptr(d_hi), cap, C.byref(out), ws.data_ptr(), ws.numel())
    if plateau:
        props["plateau_sizes"], props["left_edges"], props["right_edges"] = pout
    if height is not None or threshold is not None:
        # x[p], x[p] - x[p -+ 1]: gathers of the input at the indices the kernel returned, the same float64 differences
        ok = idx >= 0
        at = idx.long().clamp_(min=0)
        if d_lo is not None:
            at += d_lo.long().clamp_(0, n)[:, None]            # the kernel's clamp of a tensor lo
        nan = torch.full((), math.nan, dtype=torch.float64, device=dev)

        def val(off):
            v = x2.gather(1, (at + off).clamp_(0, max(n - 1, 0))).double() if cap else x2.new_empty((rows, 0)).double()
            return -v if negate else v
        if height is not None:
            props["peak_heights"] = torch.where(ok, val(0), nan)
        if threshold is not None:
            props["left_thresholds"] = torch.where(ok, val(0) - val(-1), nan)
            props["right_thresholds"] = torch.where(ok, val(0) - val(1), nan)
    if prom is not None:
        props["prominences"], props["left_bases"], props["right_bases"] = prom, lb, rb
    if widths:
        props["widths"], props["width_heights"], props["left_ips"], props["right_ips"] = wout
    if squeeze:
        return idx[0], count[0], {k: v[0] for k, v in props.items()}
    return idx, count, props


def peaks_to_list(idx, count):
    """``(idx, count)`` of find_peaks_batch -> a list with one int32 device tensor per row, trimmed to its count (a 1-D
    pair gives one tensor).  Copies ``count`` to the host: this SYNCHRONISES the device once."""
    if idx.dim() == 1:
        return idx[:int(count.item())]
    return [idx[r, :c] for r, c in enumerate(count.tolist())]


class MinMaxFinder:
    """script/calc.py:651-686: the minima / maxima of a drawn curve inside a time interval.  The peak search
    (scipy.signal.find_peaks(values) / find_peaks(-values)) runs on the device (find_peaks_batch).  numpy / list input is
    masked on the host as the reference does and returns numpy arrays; CUDA(HIP) tensors for ``x`` and ``y`` are masked
    on the device and return device tensors.  There is no CPU fallback."""

    def find_in_interval(self, times, values, interval):
        """The samples whose time lies in ``start <= t <= end``: ``(times, values)`` as numpy arrays for host input, as
        device tensors when both are CUDA(HIP) tensors.  One device tensor beside host data is a TypeError."""
        start, end = interval
        on_device = ragged.is_device_tensor(times), ragged.is_device_tensor(values)
        if any(on_device):
            if not all(on_device):
                raise TypeError("times and values must both be host data or both CUDA(HIP) tensors")
            keep = (times >= start) & (times <= end)
            return times[keep], values[keep]
        t, v = np.asarray(times), np.asarray(values)
        m = min(t.shape[0], v.shape[0]) if t.ndim and v.ndim else 0     # pairs, as far as the shorter one goes
        t, v = t[:m], v[:m]
        keep = (t >= start) & (t <= end) if m else np.zeros(0, dtype=bool)
        return t[keep], v[keep]

    def _analyse(self, x, y, interval, negate):
        if interval is None:
            print("No interval specified.")
            return [], []
        import torch
        interval_times, interval_values = self.find_in_interval(x, y, interval)
        on_device = ragged.is_device_tensor(interval_values)
        if on_device:
            d = interval_values if interval_values.dtype in (torch.float32, torch.float64) else interval_values.double()
        else:
            if not torch.cuda.is_available():
                raise RuntimeError("modulation_mfcc_amd needs an AMD GPU (gfx950); there is no CPU fallback")
            if interval_values.size == 0:
                return [], []
            # scipy.signal.find_peaks converts its argument to float64
            d = torch.from_numpy(np.ascontiguousarray(interval_values, dtype=np.float64)).cuda()
        if d.numel() == 0:
            return [], []
        peaks = peaks_to_list(*find_peaks_batch(d.reshape(-1), negate=negate)[:2])
        if len(peaks) == 0:
            return [], []
        if on_device:
            peaks = peaks.long()
            return interval_times[peaks], interval_values[peaks]
        peaks = peaks.cpu().numpy()
        return interval_times[peaks], interval_values[peaks]

    def analyse_minimum(self, x, y, interval):
        return self._analyse(x, y, interval, True)

    def analyse_maximum(self, x, y, interval):
        return self._analyse(x, y, interval, False)
