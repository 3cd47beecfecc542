"""Praat's spectrogram on the device (csrc/mm_pspec.hip, include/modmfcc_pspec.h): the first step of
the viewer's picture, script/praat_py_ui/parselmouth_calc.py:31-39.

    praat_spectrogram_params(n, sr, **kw)               -> the framing arithmetic of Sound.to_spectrogram (numpy, no GPU)
    praat_spectrogram_batch(audio, sr, **kw)            -> (times, freqs, power [.., F, T])
    praat_spectrogram_ragged_batch(audio, lengths, ..)  -> (frames, t1, freqs, power [rows, F, T_max]), a length per clip
    praat_spectrogram_list(clips, sr, **kw)             -> [(times, freqs, power [F, T_b])] for clips of any lengths
    Parselmouth(path).get_sound() / .get_spectrogram()  -> the reference's wrapper, its dataclasses and field names
    spectrogram_view(path_or_audio, sr, zoom_blur)      -> (x_grid, y_grid, the viewer's image): the whole chain on the device

``**kw`` are parselmouth's keywords and defaults: window_length=0.005, maximum_frequency=5000.0, time_step=0.002,
frequency_step=20.0, window_shape='GAUSSIAN' (or SQUARE, HAMMING, BARTLETT, WELCH, HANNING); the two oversampling limits
are 8, as in parselmouth.  What is computed is the algorithm of Praat's Sound_to_Spectrogram as DESIGN.md section 19 states
it; the yardstick is a float64 restatement of that statement (tests/test_gpu_pspec.py).  parselmouth itself is not
available where this package is tested, so parity with Praat's own numbers is NOT pinned (INTEGRATION.md has the recipe to
compare).  The framing is host arithmetic in float64, the frames' first samples go to the device as a table; the device
windows, transforms (float32 for float32 sounds, float64 for float64), squares, averages over the channels and sums the
bands.  There is no host fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from dataclasses import dataclass, field

import numpy as np

from . import ragged

__all__ = ["praat_spectrogram_params", "praat_spectrogram_batch", "praat_spectrogram_ragged_batch",
           "praat_spectrogram_list", "PraatSpectrogramParams", "Parselmouth", "Sound", "Spectrogram", "spectrogram_view",
           "WINDOW_SHAPES", "MAX_NFFT", "MAX_CHANNELS"]

WINDOW_SHAPES = ("SQUARE", "HAMMING", "BARTLETT", "WELCH", "HANNING", "GAUSSIAN")
MAX_NFFT = 4096              # MM_PSPEC_MAX_NFFT of include/modmfcc_pspec.h
MAX_CHANNELS = 8             # MM_PSPEC_MAX_CHANNELS
_OVERSAMPLING = 8.0          # parselmouth's maximum_time_oversampling and maximum_frequency_oversampling
_DB = 1                      # MM_PSPEC_DB

_MSG_WINDOW = "analysis window too short: less than one sample pair ({0} samples of {1} s in a window of {2} s)"
_MSG_SHORT = "sound shorter than the analysis window: {0} samples are {1} s, the window takes {2} s"
_MSG_BANDS = "no frequency band: maximum_frequency {0} Hz is below the frequency step {1} Hz"
_MSG_SHAPE = "unknown window_shape {0!r}: the shapes are " + ", ".join(WINDOW_SHAPES)
_MSG_NFFT = ("a transform of {0} points is not built (the limit is {1}): window_length {2} s at {3} Hz with a frequency "
             "step of {4} Hz")


@dataclass(frozen=True)
class PraatSpectrogramParams:
    """The quantities of DESIGN.md section 19 for a sound of ``n`` samples at ``sr``: ``nw`` window samples of ``window``
    (float64), ``n_frames`` frames whose first samples (0-based) are ``starts``, frame k centred at ``t1 + k time_step``;
    ``n_freqs`` bands of ``bw`` bins of an ``nfft``-point transform, band j centred at ``y1 + j frequency_step``;
    ``scale`` = 1 / sum(window^2) / bw.  ``time_step`` and ``frequency_step`` are the ones in effect, not the keywords."""
    n: int
    sr: float
    dx: float
    x1: float
    window_length: float
    window_shape: str
    physical_length: float
    nw: int
    half: int
    n_frames: int
    t1: float
    time_step: float
    maximum_frequency: float
    n_freqs: int
    nfft: int
    bw: int
    bin_hz: float
    frequency_step: float
    y1: float
    scale: float
    window: np.ndarray = field(repr=False, compare=False)
    starts: np.ndarray = field(repr=False, compare=False)

    @property
    def times(self):
        return self.t1 + np.arange(self.n_frames, dtype=np.float64) * self.time_step

    @property
    def freqs(self):
        return self.y1 + np.arange(self.n_freqs, dtype=np.float64) * self.frequency_step

    @property
    def x_grid(self):
        return self.t1 - self.time_step / 2 + np.arange(self.n_frames + 1, dtype=np.float64) * self.time_step

    @property
    def y_grid(self):
        return self.y1 - self.frequency_step / 2 + np.arange(self.n_freqs + 1, dtype=np.float64) * self.frequency_step

    @property
    def hops(self):
        """The distinct distances between the first samples of consecutive frames, ascending."""
        return sorted(set(np.diff(self.starts).tolist()))


def praat_window(shape, nw, nspw):
    """The window of ``nw`` samples for a physical window of ``nspw`` = physical_length / dx samples (not an integer),
    float64: Praat's formulas, sample i = 1 .. nw."""
    i = np.arange(1, nw + 1, dtype=np.float64)
    if shape == "GAUSSIAN":
        ph = (i - 0.5 * (nw + 1)) / nspw
        edge = math.exp(-12.0)
        return (np.exp(-48.0 * ph * ph) - edge) / (1.0 - edge)
    ph = i / nspw
    if shape == "SQUARE":
        return np.ones(nw, dtype=np.float64)
    if shape == "HAMMING":
        return 0.54 - 0.46 * np.cos(2.0 * np.pi * ph)
    if shape == "BARTLETT":
        return 1.0 - np.abs(2.0 * ph - 1.0)
    if shape == "WELCH":
        return 1.0 - (2.0 * ph - 1.0) ** 2
    if shape == "HANNING":
        return 0.5 * (1.0 - np.cos(2.0 * np.pi * ph))
    raise ValueError(_MSG_SHAPE.format(shape))


def praat_spectrogram_params(n, sr, window_length=0.005, maximum_frequency=5000.0, time_step=0.002, frequency_step=20.0,
                             window_shape="GAUSSIAN"):
    """The framing arithmetic of Sound.to_spectrogram for ``n`` samples at ``sr`` Hz, float64, in Praat's order (DESIGN.md
    section 19) -> PraatSpectrogramParams (its arrays read-only: the last geometries are kept).  numpy only.  ValueError: a
    window of less than one sample pair, a sound shorter than the window, no frequency band, an unknown shape;
    NotImplementedError: a transform above 4096 points."""
    return _params(int(n), float(sr), float(window_length), float(maximum_frequency), float(time_step), float(frequency_step),
                   window_shape)


@functools.lru_cache(maxsize=256)
def _params(n, sr, window_length, maximum_frequency, time_step, frequency_step, window_shape):
    """The framing arithmetic of Sound.to_spectrogram for ``n`` samples at ``sr`` Hz, float64, in Praat's order (DESIGN.md
    section 19), once per argument list."""
    shape = window_shape.upper() if isinstance(window_shape, str) else window_shape
    if shape not in WINDOW_SHAPES:
        raise ValueError(_MSG_SHAPE.format(window_shape))
    if not (sr > 0.0 and math.isfinite(sr)) or not (window_length > 0.0 and math.isfinite(window_length)):
        raise ValueError(f"sr and window_length must be positive, got {sr} and {window_length}")
    dx = 1.0 / sr
    x1 = 0.5 * dx
    nyquist = 0.5 / dx
    phys = 2.0 * window_length if shape == "GAUSSIAN" else window_length
    eff_t = window_length / math.sqrt(math.pi)
    eff_f = 1.0 / eff_t
    ts = max(float(time_step), eff_t / _OVERSAMPLING)
    fs = max(float(frequency_step), eff_f / _OVERSAMPLING)
    dur = dx * n
    nw0 = int(math.floor(phys / dx))
    half = nw0 // 2 - 1
    if half < 1:
        raise ValueError(_MSG_WINDOW.format(nw0, dx, phys))
    nw = 2 * half
    if phys > dur:
        raise ValueError(_MSG_SHORT.format(n, dur, phys))
    T = 1 + int(math.floor((dur - phys) / ts))
    t1 = x1 + 0.5 * ((n - 1) * dx - (T - 1) * ts)
    fmax = float(maximum_frequency)
    if fmax <= 0.0 or fmax > nyquist:
        fmax = nyquist
    F = int(math.floor(fmax / fs))
    if F < 1:
        raise ValueError(_MSG_BANDS.format(fmax, fs))
    nfft = 1
    while nfft < nw or nfft < 2 * F * (nyquist / fmax):
        nfft *= 2
    if nfft > MAX_NFFT:
        raise NotImplementedError(_MSG_NFFT.format(nfft, MAX_NFFT, window_length, sr, fs))
    bw = max(1, int(math.floor(fs * dx * nfft)))
    bin_hz = 1.0 / (dx * nfft)
    fs = bw * bin_hz
    F = int(math.floor(fmax / fs))
    if F < 1:
        raise ValueError(_MSG_BANDS.format(fmax, fs))
    y1 = 0.5 * (fs - bin_hz)
    window = praat_window(shape, nw, phys / dx)
    scale = 1.0 / float(np.sum(window * window)) / bw
    t = t1 + np.arange(T, dtype=np.float64) * ts
    left = np.floor((t - x1) / dx).astype(np.int64) + 1                  # 1-based, as in Praat
    starts = left - half                                                   # 0-based first sample: left + 1 - half - 1
    if int(starts.min()) < 0 or int(starts.max()) + nw > n or F * bw > nfft // 2:
        raise ValueError(f"frames out of range: first samples {int(starts.min())} .. {int(starts.max())}, a window of {nw} "
                         f"samples, a sound of {n}")                     # (not reachable for a finite sound: a guard)
    starts = starts.astype(np.int32)
    window.setflags(write=False)
    starts.setflags(write=False)
    return PraatSpectrogramParams(n=n, sr=sr, dx=dx, x1=x1, window_length=window_length, window_shape=shape,
                                  physical_length=phys, nw=nw, half=half, n_frames=T, t1=t1, time_step=ts,
                                  maximum_frequency=fmax, n_freqs=F, nfft=nfft, bw=bw, bin_hz=bin_hz, frequency_step=fs,
                                  y1=y1, scale=scale, window=window, starts=starts)


# ---- the device side --------------------------------------------------------------------------------------------------------
def _sounds(audio, who, batch_only=False):
    """audio [n], [rows, n] or [rows, channels, n] -> ([rows, channels, n] with a unit last stride, a channel stride >= n
    and a row stride >= channels * channel stride -- a copy where the layout is another --, the leading shape)."""
    import torch
    if not ragged.is_device_tensor(audio):
        raise TypeError(f"{who} takes a CUDA(HIP) tensor")
    if audio.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who} takes float32 or float64 sounds, got {audio.dtype}")
    if audio.dim() not in ((2, 3) if batch_only else (1, 2, 3)):
        raise ValueError(f"{who} takes " + ("" if batch_only else "[n], ") + f"[rows, n] or [rows, channels, n], got "
                         f"{tuple(audio.shape)}")
    lead = tuple(audio.shape[:-1]) if audio.dim() < 3 else (audio.shape[0],)
    x = audio.reshape(1, 1, -1) if audio.dim() == 1 else audio.unsqueeze(1) if audio.dim() == 2 else audio
    rows, ch, n = x.shape
    if rows < 1 or ch < 1 or n < 1:
        raise ValueError(f"{who}: a sound needs a row, a channel and a sample, got {tuple(audio.shape)}")
    if ch > MAX_CHANNELS:
        raise NotImplementedError(f"{who}: {ch} channels, the limit is {MAX_CHANNELS}")
    sr_, sc, sn = x.stride()
    if (n > 1 and sn != 1) or (ch > 1 and sc < n) or (rows > 1 and sr_ < (ch * sc if ch > 1 else n)):
        x = x.contiguous()
    return x, lead


def _strides(x):
    rows, ch, n = x.shape
    sc = x.stride(1) if ch > 1 else n
    sr_ = x.stride(0) if rows > 1 else ch * sc
    return sr_, sc


_PLANS = {}                  # (device, dtype, channels, geometry, lengths) -> (mm_pspec_params, window, table) on the device
_PLANS_MAX = 64


def _plan(x, p, lens, table):
    """The host's share of a call, made once per geometry: the parameter struct with the tiles' span, the window in x's type
    and the table of first samples on x's device.  ``lens``: None for the one table of ``p`` for every row, the tuple of
    the clips' lengths for a table row per clip (with ``p`` -- the rate and the keywords -- they determine the table);
    ``table()`` builds the host table [rows, t_max] when the geometry is new.  A geometry that has been seen builds and
    uploads nothing (a captured call must not).  A new one waits once for its upload, so that any stream may read the
    tables later -- and, where it takes the place of the oldest of _PLANS_MAX, for the device first: a kernel on any
    stream may still be reading the tables that go."""
    import torch
    ch, dev = x.shape[1], x.device
    key = (str(dev), x.dtype, ch, p, lens)
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= _PLANS_MAX:
            torch.cuda.synchronize(dev)
            _PLANS.pop(next(iter(_PLANS)))
        host = table()
        c = _c_params(p, ch, _span(host, p.nw, _tile_frames(p, ch)), 0)
        w = p.window.astype(np.float32 if x.dtype == torch.float32 else np.float64)
        plan = _PLANS[key] = (c, torch.from_numpy(w).to(dev), torch.from_numpy(np.array(host, dtype=np.int32)).to(dev))
        torch.cuda.current_stream(dev).synchronize()
    return plan


def _tile_frames(p, channels):
    from . import _lib
    c = _c_params(p, channels, 0, 0)
    tile = int(_lib.load().mm_pspec_tile_frames(C.byref(c)))
    if tile < 1:
        _lib.check(tile, "mm_pspec_tile_frames")
    return tile


def _c_params(p, channels, span, flags):
    from . import _lib
    return _lib.mm_pspec_params(scale=p.scale, nw=p.nw, nfft=p.nfft, bw=p.bw, n_freqs=p.n_freqs, channels=channels,
                                span=max(0, min(int(span), 1 << 30)), flags=flags, reserved=0)


def _span(starts, nw, tile):
    """Samples from the first sample of a tile's first frame to the last of its last frame, the largest over the tiles of
    the rows of ``starts`` [rows, T_max] (-1 behind a row's frames)."""
    span = 0
    for row in np.atleast_2d(starts):
        s = row[row >= 0]
        if s.size:
            first = s[::tile]
            last = s[np.minimum(np.arange(tile - 1, s.size + tile - 1, tile), s.size - 1)]
            span = max(span, int((last - first).max()) + nw)
    return span


def _launch(x, p, lens, table, t_max, db):
    """mm_pspec_f32 / _f64 on x [rows, channels, n_max] with the plan of (p, lens, table) -> [rows, F, t_max] of x's type."""
    import torch
    from . import _lib
    rows, ch, n_max = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        c, d_w, d_s = _plan(x, p, lens, table)
        if bool(c.flags) != bool(db):
            c = _c_params(p, ch, c.span, _DB if db else 0)
        out = torch.empty((rows, p.n_freqs, t_max), dtype=x.dtype, device=dev)
        sr_, sc = _strides(x)
        _lib.call("mm_pspec_f32" if x.dtype == torch.float32 else "mm_pspec_f64", dev, C.byref(c), x.data_ptr(), rows, n_max,
                  sr_, sc, d_w.data_ptr(), d_s.data_ptr(), t_max, 0 if lens is None else t_max, out.data_ptr(),
                  p.n_freqs * t_max, t_max)
    return out


def praat_spectrogram_batch(audio, sr, *, db=False, **kw):
    """Sound.to_spectrogram(**kw).values for every sound of ``audio``: a CUDA(HIP) tensor [n], [rows, n] or
    [rows, channels, n], float32 or float64, any strides whose last is 1 -> (times float64 numpy [T], freqs float64 numpy
    [F], power [.., F, T] on the device, of audio's type: Pa^2 / Hz, T fastest).  Several channels: the mean of the
    channels' powers, as in Praat.  ``db``: 10 log10 of the power, taken in float64 before the one rounding (-inf where a
    band holds no power).  Refusals come before any launch (praat_spectrogram_params).  Nothing is read back."""
    x, lead = _sounds(audio, "praat_spectrogram_batch")
    p = praat_spectrogram_params(x.shape[2], sr, **kw)
    out = _launch(x, p, None, lambda: p.starts[None, :], p.n_frames, db)
    return p.times, p.freqs, out.reshape(lead + (p.n_freqs, p.n_frames))


def _ragged_params(lens, sr, kw, name):
    """One PraatSpectrogramParams per length (equal lengths share one); a refusal names its clip through ``name(b)``."""
    by_len, ps = {}, []
    for b, n in enumerate(lens.tolist()):
        if n not in by_len:
            try:
                by_len[n] = praat_spectrogram_params(n, sr, **kw)
            except (ValueError, NotImplementedError) as e:
                raise ragged.named(e, name(b))
        ps.append(by_len[n])
    return ps


def _ragged(x, lens, sr, kw, db, name):
    ps = _ragged_params(lens, sr, kw, name)
    p0 = ps[0]          # window, transform and bands depend on sr and the keywords alone; frames and t1 on the length
    frames = np.array([p.n_frames for p in ps], dtype=np.int64)
    t_max = int(frames.max())

    def table():
        starts = np.full((len(ps), t_max), -1, dtype=np.int32)
        for b, p in enumerate(ps):
            starts[b, :p.n_frames] = p.starts
        return starts
    out = _launch(x, p0, tuple(lens.tolist()), table, t_max, db)
    return frames, np.array([p.t1 for p in ps], dtype=np.float64), p0, out


def praat_spectrogram_ragged_batch(audio, lengths, sr, *, db=False, **kw):
    """praat_spectrogram_batch with a length per clip: ``audio`` [rows, n_max] or [rows, channels, n_max] on the device,
    ``lengths`` [rows] HOST integers in [1, n_max] -> (frames int64 numpy [rows], t1 float64 numpy [rows], freqs float64
    numpy [F], power [rows, F, max(frames)]).  Clip b has frames[b] frames, frame k centred at t1[b] + k time_step, and
    its image is praat_spectrogram_batch(audio[b, ..., :lengths[b]]) bit for bit in its first frames[b] columns, +0.0
    behind them; what ``audio`` holds behind a length never matters.  A clip the single call refuses is refused here with
    its index, before any launch.  An int64 device tensor of lengths raises NotImplementedError: the frame table -- how
    many frames a clip has and where each starts -- is host arithmetic in float64."""
    if ragged.is_device_tensor(lengths):
        raise NotImplementedError("praat_spectrogram_ragged_batch takes host lengths: the frame table (the frame count of a "
                                  "clip, its centring and the first sample of every frame) is float64 arithmetic on the "
                                  "host, and reading device lengths back would wait for the stream")
    x, _ = _sounds(audio, "praat_spectrogram_ragged_batch", batch_only=True)
    lens = ragged.check_lengths(lengths, x.shape[0], x.shape[2])
    frames, t1, p0, out = _ragged(x, lens, sr, kw, db, lambda b: b)
    return frames, t1, p0.freqs, out


def praat_spectrogram_list(clips, sr, *, db=False, **kw):
    """1-D CUDA(HIP) tensors of any lengths (float32 clips in one batch, the others as float64 in another) ->
    [(times, freqs, power [F, T_b])] in the clips' order, each what praat_spectrogram_batch gives for the clip alone.  A
    refusal names the clip by its place in ``clips``."""
    clips = list(clips)
    for i, s in enumerate(clips):
        if not ragged.is_device_tensor(s) or s.dim() != 1 or s.shape[0] < 1:
            raise ragged.named(ValueError("praat_spectrogram_list takes 1-D CUDA(HIP) tensors with a sample at the least"), i)
    out = [None] * len(clips)
    for idx, x, lens in ragged.packed_groups(clips):
        frames, t1, p0, y = _ragged(x.unsqueeze(1), lens, sr, kw, db, lambda b: idx[b])
        for b, i in enumerate(idx):
            T = int(frames[b])
            out[i] = (t1[b] + np.arange(T, dtype=np.float64) * p0.time_step, p0.freqs, y[b, :, :T])
    return out


# ---- the reference's wrapper (script/praat_py_ui/parselmouth_calc.py) -----------------------------------------------------------
@dataclass
class Sound:
    timestamps: list = field(default_factory=list)
    # Shape (channels, len(amplitudes))
    amplitudes: list = field(default_factory=list)
    sample_rate: int = 44100


@dataclass
class Spectrogram:
    timestamps: list = field(default_factory=list)
    frequencies: list = field(default_factory=list)
    data_matrix: list = field(default_factory=list)


class Parselmouth:
    """The reference's ``Parselmouth(filepath)``: the WAVE file at its own rate with all its channels, on the device.
    ``get_sound()`` -> Sound(xs float64 numpy [n], values [channels, n] on the device, the rate); ``get_spectrogram()`` ->
    Spectrogram(x_grid, y_grid float64 numpy, 10 log10(values) [F, T] on the device)."""

    def __init__(self, filepath, device=None):
        from .audio_io import load_wav
        self._values, self._sr = load_wav(os.fspath(filepath), device)

    def get_sound(self):
        n = self._values.shape[1]
        dx = 1.0 / float(self._sr)
        return Sound(0.5 * dx + np.arange(n, dtype=np.float64) * dx, self._values, self._sr)

    def get_spectrogram(self, **kw):
        x = self._values.unsqueeze(0)
        p = praat_spectrogram_params(x.shape[2], self._sr, **kw)
        _, _, db = praat_spectrogram_batch(x, self._sr, db=True, **kw)
        return Spectrogram(p.x_grid, p.y_grid, db[0])


def spectrogram_view(path_or_audio, sr=None, zoom_blur=True, **kw):
    """The viewer's picture, script/praat_py_ui/spectrogram.py:60-71, on the device: Sound.to_spectrogram, 10 log10 and
    scipy.ndimage.zoom(.., 6, order=4) -> (x_grid, y_grid, image).  ``path_or_audio``: a WAVE file (its own rate, all
    channels) or a CUDA(HIP) tensor [n] or [channels, n] with ``sr``.  The power goes straight to zoom_batch(.., 6,
    order=4, db=True), which takes the logarithm as it loads: no pass in between; without ``zoom_blur`` the image is the dB
    image itself."""
    from .zoom import zoom_batch
    if ragged.is_device_tensor(path_or_audio):
        if sr is None:
            raise ValueError("spectrogram_view of a tensor needs its sampling rate")
        x = path_or_audio
        if x.dim() not in (1, 2):
            raise ValueError(f"spectrogram_view takes one sound [n] or [channels, n], got {tuple(x.shape)}")
        x = x.reshape(1, 1, -1) if x.dim() == 1 else x.unsqueeze(0)
    else:
        from .audio_io import load_wav
        values, file_sr = load_wav(os.fspath(path_or_audio))
        x, sr = values.unsqueeze(0), file_sr
    p = praat_spectrogram_params(x.shape[2], sr, **kw)
    _, _, img = praat_spectrogram_batch(x, sr, db=not zoom_blur, **kw)
    return p.x_grid, p.y_grid, (zoom_batch(img[0], 6, order=4, db=True) if zoom_blur else img[0])
