"""Praat's intensity contour on the device (csrc/mm_pint.hip, include/modmfcc_pint.h): the
``sound.to_intensity()`` / ``intensities.get_value(time)`` of script/calc.py:131-170 and the ``call(xObj, "To Intensity",
minPitch, step, 1)`` that ends the 'RMSpraat' amplitude method (script/calc.py:292-324, script/mfcc.py:214-233).

    praat_intensity_params(n, sr, **kw)                 -> the framing arithmetic of Sound_to_Intensity (numpy, no GPU)
    praat_intensity_batch(audio, sr, **kw)              -> (times, intensity [.., T])
    praat_intensity_ragged_batch(audio, lengths, ..)    -> (frames, t1, intensity [rows, T_max]), a length per clip
    praat_intensity_list(clips, sr, **kw)               -> [(times, intensity [T_b])] for clips of any lengths
    to_intensity(sound_or_audio, sr, ..)                -> Intensity, with .get_value(time, interpolation)
    praat_rms_envelope(x, sr, min_pitch, hopLen, ..)    -> (amp, ampT): the tail of 'RMSpraat' for a given pitch floor

``**kw`` are parselmouth's keywords and defaults: minimum_pitch=100.0, time_step=None (0.8 / minimum_pitch),
subtract_mean=True.  What is computed is the algorithm of Praat's Sound_to_Intensity as DESIGN.md section 20 states it;
the yardstick is a float64 restatement of that statement (tests/test_gpu_pint.py).  parselmouth itself is not available
where this package is tested, so parity with Praat's own digits is NOT pinned (INTEGRATION.md has the recipe to compare).
The framing and the window are host arithmetic in float64, the frames' centre samples go to the device as a table; the
device sums in float64 whatever the samples' type.  ``calculate_amplitude_envelope(method='RMSpraat')`` itself still raises:
its pitch floor comes from Praat's pitch tracker.  There is no host fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from . import ragged
from .pspec import Sound, _sounds, _strides

__all__ = ["praat_intensity_params", "praat_intensity_batch", "praat_intensity_ragged_batch", "praat_intensity_list",
           "PraatIntensityParams", "Intensity", "to_intensity", "praat_rms_envelope", "bessel_i0", "MAX_HALF", "MAX_CHANNELS",
           "INTERPOLATIONS"]

MAX_HALF = 16384             # MM_PINT_MAX_HALF of include/modmfcc_pint.h
MAX_CHANNELS = 8             # MM_PINT_MAX_CHANNELS
_LINEAR, _KEEP_MEAN = 1, 2   # MM_PINT_LINEAR, MM_PINT_KEEP_MEAN
INTERPOLATIONS = {"nearest": 0, "linear": 1, "cubic": 2}

_MSG_SHORT = "sound shorter than the analysis window: {0} samples are {1} s, the window takes {2} s"
_MSG_HALF = "a window of {0} samples on either side is not built (the limit is {1}): minimum_pitch {2} Hz at {3} Hz"


def bessel_i0(x):
    """Praat's NUMbessel_i0_f: Abramowitz & Stegun 9.8.1 / 9.8.2, float64, elementwise (|error| below 2e-7 relative)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    small = x < 3.75
    t = np.where(small, x / 3.75, 0.0)
    t = t * t
    lo = 1.0 + t * (3.5156229 + t * (3.0899424 + t * (1.2067492 + t * (0.2659732 + t * (0.0360768 + t * 0.0045813)))))
    xs = np.where(small, 3.75, x)
    t = 3.75 / xs
    hi = np.exp(xs) / np.sqrt(xs) * (0.39894228 + t * (0.01328592 + t * (0.00225319 + t * (-0.00157565 + t * (0.00916281 + t * (
        -0.02057706 + t * (0.02635537 + t * (-0.01647633 + t * 0.00392377))))))))
    return np.where(small, lo, hi)


@dataclass(frozen=True)
class PraatIntensityParams:
    """The quantities of DESIGN.md section 20 for a sound of ``n`` samples at ``sr``: ``hw`` taps on either side, ``W`` =
    2 hw + 1 taps of ``window`` (float64), ``T`` frames whose centre samples (0-based) are ``centres``, frame k at ``t1 + k
    time_step``.  ``time_step`` is the one in effect, not the keyword."""
    n: int
    sr: float
    dx: float
    x1: float
    minimum_pitch: float
    subtract_mean: bool
    physical_length: float
    hw: int
    W: int
    T: int
    t1: float
    time_step: float
    window: np.ndarray = field(repr=False, compare=False)
    centres: np.ndarray = field(repr=False, compare=False)

    @property
    def n_frames(self):
        return self.T

    @property
    def times(self):
        return self.t1 + np.arange(self.T, dtype=np.float64) * self.time_step

    @property
    def hops(self):
        """The distinct distances between the centre samples of consecutive frames, ascending."""
        return sorted(set(np.diff(self.centres).tolist()))


def praat_intensity_params(n, sr, minimum_pitch=100.0, time_step=None, subtract_mean=True):
    """The framing arithmetic of Sound.to_intensity for ``n`` samples at ``sr`` Hz, float64, in the order of DESIGN.md
    section 20 -> PraatIntensityParams (its arrays read-only: the last geometries are kept).  numpy only.  ValueError: a
    sound shorter than the window, a rate or pitch floor that is not positive; NotImplementedError: hw above 16384."""
    ts = 0.0 if time_step is None else float(time_step)
    return _params(int(n), float(sr), float(minimum_pitch), ts, bool(subtract_mean))


def _geometry(sr, minimum_pitch, time_step):
    """(dx, x1, phys, hw, dt): what does not depend on the sound's length."""
    if not (sr > 0.0 and math.isfinite(sr)) or not (minimum_pitch > 0.0 and math.isfinite(minimum_pitch)):
        raise ValueError(f"sr and minimum_pitch must be positive, got {sr} and {minimum_pitch}")
    dx = 1.0 / sr
    x1 = dx / 2
    phys = 6.4 / minimum_pitch
    dt = time_step if time_step > 0.0 else 0.8 / minimum_pitch
    if not math.isfinite(dt):
        raise ValueError(f"time_step must be finite, got {time_step}")
    hw = int(math.floor(0.5 * phys / dx))
    if hw < 1:
        raise ValueError(f"analysis window too short: {phys} s is less than two samples of {dx} s")
    if hw > MAX_HALF:
        raise NotImplementedError(_MSG_HALF.format(hw, MAX_HALF, minimum_pitch, sr))
    return dx, x1, phys, hw, dt


def _window(hw, dx, phys):
    i = np.arange(-hw, hw + 1, dtype=np.float64)
    u = dx * i / (0.5 * phys)
    root = 1.0 - u * u
    root[root < 0.0] = 0.0
    w = bessel_i0((2.0 * np.pi * np.pi + 0.5) * np.sqrt(root))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=256)
def _params(n, sr, minimum_pitch, time_step, subtract_mean):
    dx, x1, phys, hw, dt = _geometry(sr, minimum_pitch, time_step)
    dur = n * dx
    if phys > dur:
        raise ValueError(_MSG_SHORT.format(n, dur, phys))
    T = int(math.floor((dur - phys) / dt)) + 1
    t1 = x1 - dx / 2 + dur / 2 - T * dt / 2 + dt / 2
    t = t1 + np.arange(T, dtype=np.float64) * dt
    c = np.floor((t - x1) / dx + 0.5).astype(np.int64)
    if T >= 2 ** 31 or int(c.min()) < 0 or int(c.max()) >= n:
        raise ValueError(f"frames out of range: centre samples {int(c.min())} .. {int(c.max())}, a sound of {n}")   # (a guard)
    c = c.astype(np.int32)
    c.setflags(write=False)
    return PraatIntensityParams(n=n, sr=sr, dx=dx, x1=x1, minimum_pitch=minimum_pitch, subtract_mean=subtract_mean,
                                physical_length=phys, hw=hw, W=2 * hw + 1, T=T, t1=t1, time_step=dt,
                                window=_window(hw, dx, phys), centres=c)


# ---- the device side --------------------------------------------------------------------------------------------------------
_PLANS = {}                  # (device, channels, geometry, lengths) -> (mm_pint_params, window, table) on the device
_PLANS_MAX = 64


def _c_params(p, channels, span, linear):
    from . import _lib
    flags = (_LINEAR if linear else 0) | (0 if p.subtract_mean else _KEEP_MEAN)
    return _lib.mm_pint_params(hw=p.hw, channels=channels, span=max(0, min(int(span), 1 << 30)), flags=flags, reserved=0)


def _tile_frames(p, channels):
    from . import _lib
    c = _c_params(p, channels, 0, False)
    tile = int(_lib.load().mm_pint_tile_frames(C.byref(c)))
    if tile < 1:
        _lib.check(tile, "mm_pint_tile_frames")
    return tile


def _span(centres, W, tile):
    """Samples from the first sample of a tile's first frame to the last of its last frame, the largest over the tiles of
    the rows of ``centres`` [rows, T_max] (-1 behind a row's frames)."""
    span = 0
    for row in np.atleast_2d(centres):
        s = row[row >= 0]
        if s.size:
            first = s[::tile]
            last = s[np.minimum(np.arange(tile - 1, s.size + tile - 1, tile), s.size - 1)]
            span = max(span, int((last - first).max()) + W)
    return span


def _plan(x, p, lens, table):
    """The host's share of a call, made once per geometry: the parameter struct with the tiles' span, the window and the
    table of centre samples on x's device.  ``lens``: None for the one table of ``p`` for every row, the tuple of the
    clips' lengths for a table row per clip; ``table()`` builds the host table [rows, t_max] when the geometry is new.  A
    geometry that has been seen builds and uploads nothing (a captured call must not).  A new one waits once for its upload
    -- and, where it takes the place of the oldest of _PLANS_MAX, for the device first: a kernel on any stream may still
    be reading the tables that go."""
    import torch
    ch, dev = x.shape[1], x.device
    key = (str(dev), ch, p, lens)
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= _PLANS_MAX:
            torch.cuda.synchronize(dev)
            _PLANS.pop(next(iter(_PLANS)))
        host = table()
        c = _c_params(p, ch, _span(host, p.W, _tile_frames(p, ch)), False)
        plan = _PLANS[key] = (c, torch.from_numpy(np.array(p.window)).to(dev),
                              torch.from_numpy(np.array(host, dtype=np.int32)).to(dev))
        torch.cuda.current_stream(dev).synchronize()
    return plan


def _entry(x, c, d_w, d_c, table_rows, d_len, t_max):
    """mm_pint_f32 / _f64 on x [rows, channels, n_max] -> [rows, t_max] float64."""
    import torch
    from . import _lib
    rows, ch, n_max = x.shape
    out = torch.empty((rows, t_max), dtype=torch.float64, device=x.device)
    sr_, sc = _strides(x)
    _lib.call("mm_pint_f32" if x.dtype == torch.float32 else "mm_pint_f64", x.device, C.byref(c), x.data_ptr(), rows, n_max,
              sr_, sc, d_w.data_ptr(), d_c.data_ptr(), t_max, t_max if table_rows else 0,
              None if d_len is None else d_len.data_ptr(), out.data_ptr(), t_max)
    return out


def _launch(x, p, lens, table, t_max, db):
    import torch
    with torch.cuda.device(x.device):
        c, d_w, d_c = _plan(x, p, lens, table)
        if bool(c.flags & _LINEAR) != (not db):
            c = _c_params(p, x.shape[1], c.span, not db)
        d_len = None if lens is None else ragged.counts_on_device(np.array(lens, dtype=np.int64), x.device)
        return _entry(x, c, d_w, d_c, lens is not None, d_len, t_max)


def praat_intensity_batch(audio, sr, *, db=True, **kw):
    """Sound.to_intensity(**kw).values for every sound of ``audio``: a CUDA(HIP) tensor [n], [rows, n] or
    [rows, channels, n], float32 or float64, any strides whose last is 1 -> (times float64 numpy [T], intensity [.., T]
    float64 on the device: dB re 4e-10 Pa^2, -300 for a frame without power; with ``db=False`` the power in Pa^2).
    Several channels: the mean of the channels' powers, as in Praat.  Refusals come before any launch.  Nothing is read
    back."""
    x, lead = _sounds(audio, "praat_intensity_batch")
    p = praat_intensity_params(x.shape[2], sr, **kw)
    out = _launch(x, p, None, lambda: p.centres[None, :], p.T, db)
    return p.times, out.reshape(lead + (p.T,))


def _ragged_params(lens, sr, kw, name, noun="row"):
    """One PraatIntensityParams per length (equal lengths share one); a refusal names its row or clip, ``name(b)``."""
    by_len, ps = {}, []
    for b, n in enumerate(lens.tolist()):
        if n not in by_len:
            try:
                by_len[n] = praat_intensity_params(n, sr, **kw)
            except (ValueError, NotImplementedError) as e:
                raise ragged.named(e, name(b), noun)
        ps.append(by_len[n])
    return ps


def _ragged(x, lens, sr, kw, db, name, noun="row"):
    ps = _ragged_params(lens, sr, kw, name, noun)
    frames = np.array([p.T for p in ps], dtype=np.int64)
    t_max = int(frames.max())

    def table():
        centres = np.full((len(ps), t_max), -1, dtype=np.int32)
        for b, p in enumerate(ps):
            centres[b, :p.T] = p.centres
        return centres
    out = _launch(x, ps[0], tuple(lens.tolist()), table, t_max, db)
    return frames, np.array([p.t1 for p in ps], dtype=np.float64), ps[0], out


def _ragged_device(x, d_len, sr, kw, db):
    """Lengths on the device, never read back: the frame table is the arithmetic of _params in torch float64 on the device
    (the same IEEE operations in the same order), sized for n_max; a row shorter than the window comes out NaN."""
    import torch
    rows, ch, n_max = x.shape
    p = praat_intensity_params(n_max, sr, **kw)               # the window, and the most frames a row can have
    dx, x1, phys, dt, dev = p.dx, p.x1, p.physical_length, p.time_step, x.device
    with torch.cuda.device(dev):
        n = d_len.clamp(1, n_max).to(torch.float64)
        dur = n * dx
        ok = ~(phys > dur)
        # (a tensor divided by a Python number is multiplied by its reciprocal on the device: divide by tensors)
        dt_t, dx_t = torch.full_like(dur[:1], dt), torch.full_like(dur[:1], dx)
        T = torch.where(ok, torch.floor((dur - phys) / dt_t) + 1, torch.zeros_like(dur))
        t1 = x1 - dx / 2 + dur / 2 - T * dt / 2 + dt / 2
        k = torch.arange(p.T, dtype=torch.float64, device=dev)
        t = t1[:, None] + k[None, :] * dt
        centre = torch.floor((t - x1) / dx_t + 0.5)
        centre = torch.where(k[None, :] < T[:, None], centre, torch.full_like(centre, -1.0)).to(torch.int32)
        # every frame from memory would be correct too; the span of the longest row's tiles sizes the staged copy
        c = _c_params(p, ch, _span(p.centres[None, :], p.W, _tile_frames(p, ch)), not db)
        _, d_w, _ = _plan(x, p, None, lambda: p.centres[None, :])
        out = _entry(x, c, d_w, centre, True, d_len, p.T)
        out = torch.where(ok[:, None], out, torch.full_like(out, float("nan")))
    return T.to(torch.int64), t1, out


def praat_intensity_ragged_batch(audio, lengths, sr, *, db=True, **kw):
    """praat_intensity_batch with a length per clip: ``audio`` [rows, n_max] or [rows, channels, n_max] on the device,
    ``lengths`` [rows] in [1, n_max] -> (frames [rows], t1 [rows], intensity [rows, T_max] float64).  Clip b has frames[b]
    frames, frame k at t1[b] + k time_step, and its contour is praat_intensity_batch(audio[b, ..., :lengths[b]]) bit for
    bit in its first frames[b] values, +0.0 behind them; what ``audio`` holds behind a length is never read.  Host lengths:
    frames and t1 are numpy, T_max = max(frames), and a clip shorter than the window is refused with its row, before any
    launch.  An int64 device tensor of lengths is never read back: frames and t1 are device tensors, T_max is the frame
    count of n_max samples, and a clip shorter than the window is a row of NaN with frames 0."""
    x, _ = _sounds(audio, "praat_intensity_ragged_batch", batch_only=True)
    lens = ragged.check_lengths(lengths, x.shape[0], x.shape[2], x.device)
    if ragged.is_device_tensor(lens):
        return _ragged_device(x, lens, sr, kw, db)
    frames, t1, _, out = _ragged(x, lens, sr, kw, db, lambda b: b)
    return frames, t1, out


def praat_intensity_list(clips, sr, *, db=True, **kw):
    """1-D CUDA(HIP) tensors of any lengths (float32 clips in one batch, the others as float64 in another) ->
    [(times, intensity [T_b])] in the clips' order, each what praat_intensity_batch gives for the clip alone.  A refusal
    names the clip by its place in ``clips``."""
    clips = list(clips)
    for i, s in enumerate(clips):
        if not ragged.is_device_tensor(s) or s.dim() != 1 or s.shape[0] < 1:
            raise ragged.named(ValueError("praat_intensity_list takes 1-D CUDA(HIP) tensors with a sample at the least"), i)
    out = [None] * len(clips)
    for idx, x, lens in ragged.packed_groups(clips):
        frames, t1, p0, y = _ragged(x.unsqueeze(1), lens, sr, kw, db, lambda b: idx[b], "clip")
        for b, i in enumerate(idx):
            T = int(frames[b])
            out[i] = (t1[b] + np.arange(T, dtype=np.float64) * p0.time_step, y[b, :T])
    return out


# ---- parselmouth's object ------------------------------------------------------------------------------------------------------
def _lookup(values, frames, t1, time_step, times, depth):
    """mm_pint_value_f64: values [rows, T_max] float64 on the device, ``times`` a float64 device tensor [q] -> [rows, q]."""
    import torch
    from . import _lib
    dev = values.device
    rows, t_max = values.shape
    q = times.shape[0]
    out = torch.empty((rows, q), dtype=torch.float64, device=dev)
    if q:
        _lib.call("mm_pint_value_f64", dev, values.data_ptr(), rows, t_max, ragged.row_pitch(values),
                  None if frames is None else frames.data_ptr(), t1.data_ptr(), C.c_double(time_step), times.data_ptr(), q, 0,
                  depth, out.data_ptr(), q)
    return out


@dataclass
class Intensity:
    """parselmouth's Intensity, on the device: ``values`` [1, T] float64 (dB), frame k at ``t1 + k time_step``."""
    values: object
    t1: float
    time_step: float
    n_frames: int
    xmin: float
    xmax: float

    def xs(self):
        return self.t1 + np.arange(self.n_frames, dtype=np.float64) * self.time_step

    def get_time_step(self):
        return self.time_step

    def get_value(self, time, interpolation="cubic"):
        """The contour at ``time`` (seconds): Vector_getValueAtX, 'nearest', 'linear' or 'cubic' (parselmouth's default);
        NaN more than half a step outside the frames.  A scalar gives a float (one read-back), a numpy array or sequence
        a numpy array, a CUDA(HIP) tensor a tensor on the device with nothing read back."""
        import torch
        key = interpolation.lower() if isinstance(interpolation, str) else interpolation
        if key not in INTERPOLATIONS:
            raise ValueError(f"unknown interpolation {interpolation!r}: 'nearest', 'linear' or 'cubic'")
        dev = self.values.device
        on_device = ragged.is_device_tensor(time)
        with torch.cuda.device(dev):
            if on_device:
                shape, q = tuple(time.shape), time.to(torch.float64).reshape(-1).contiguous()
            else:
                host = np.asarray(time, dtype=np.float64)
                shape, q = host.shape, torch.from_numpy(np.ascontiguousarray(host.reshape(-1))).to(dev)
            t1 = torch.full((1,), self.t1, dtype=torch.float64, device=dev)
            out = _lookup(self.values.reshape(1, -1), None, t1, self.time_step, q, INTERPOLATIONS[key]).reshape(shape)
        if on_device:
            return out
        return float(out.item()) if shape == () else out.cpu().numpy()


def to_intensity(sound_or_audio, sr=None, minimum_pitch=100.0, time_step=None, subtract_mean=True):
    """``Sound.to_intensity(minimum_pitch, time_step, subtract_mean)`` -> Intensity.  ``sound_or_audio``: a Sound of
    modulation_mfcc_amd.pspec (its rate is taken), a CUDA(HIP) tensor [n] or [channels, n], or a numpy array of those
    shapes (uploaded as float64) with ``sr``."""
    import torch
    x = sound_or_audio
    if isinstance(x, Sound):
        x, sr = x.amplitudes, x.sample_rate
    if sr is None:
        raise ValueError("to_intensity of samples needs their sampling rate")
    if not ragged.is_device_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(ragged.gpu())
    if x.dim() not in (1, 2):
        raise ValueError(f"to_intensity takes one sound [n] or [channels, n], got {tuple(x.shape)}")
    x = x.reshape(1, 1, -1) if x.dim() == 1 else x.unsqueeze(0)
    p = praat_intensity_params(x.shape[2], sr, minimum_pitch, time_step, subtract_mean)
    _, y = praat_intensity_batch(x, sr, minimum_pitch=minimum_pitch, time_step=time_step, subtract_mean=subtract_mean)
    return Intensity(values=y, t1=p.t1, time_step=p.time_step, n_frames=p.T, xmin=0.0, xmax=p.n * p.dx)


def praat_rms_envelope(x, sr, min_pitch, hopLen=0.01, outFilter=None, outFiltType="low", outFiltCutOff=[12], outFiltLen=6,
                       outFiltPolyOrd=3):
    """The tail of the reference's 'RMSpraat' amplitude method (script/calc.py:311-343) for a pitch floor the caller
    supplies -- the lowest f0 of the clip, from pyin_batch for instance; the reference takes it from Praat's pitch tracker,
    which this package does not have.  ``min_pitch`` > 120: to_intensity(min_pitch, hopLen); otherwise
    to_intensity(120, 1 / sr), a frame per sample.  -> (amp, ampT): the dB values flattened (a device tensor for a device
    signal, numpy for a numpy one), ``ampT = arange(len(amp)) / ampSr`` with ampSr = 1 / the contour's time step; with
    ``outFilter`` amp goes through applyFilter at ampSr."""
    from .filters import applyFilter
    on_device = ragged.is_device_tensor(x)
    if float(min_pitch) > 120:
        inten = to_intensity(x, sr, float(min_pitch), hopLen, True)
    else:
        inten = to_intensity(x, sr, 120.0, 1.0 / sr, True)
    amp_sr = 1 / inten.get_time_step()
    amp = inten.values.flatten()
    amp_t = np.arange(amp.shape[0]) / amp_sr
    if not on_device:
        amp = amp.cpu().numpy()
    if outFilter is not None:
        amp = applyFilter(amp, amp_sr, filt=outFilter, filtType=outFiltType, cutOff=outFiltCutOff, filtLen=outFiltLen,
                          polyOrd=outFiltPolyOrd)
    return amp, amp_t
