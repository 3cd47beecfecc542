"""The yardstick of the Praat-style spectrogram (modulation_mfcc_amd/pspec.py, csrc/mm_pspec.hip): DESIGN.md section 19
restated three times, independently of the package.

  spectrogram(x, sr, dtype=float64)   the definition in numpy of ``dtype`` with scipy.fft.rfft (which keeps float32)
  spectrogram_dft(x, sr)              the same frames through a direct DFT in long double (transforms up to 1024 points)
  geometry(n, sr)                     the framing arithmetic (float64, Praat's order)

error(P, P_ref) = max |P - P_ref| / max P_ref over a clip's image.  The bounds:
  float64 entry   max(1e-12, 16 r64), r64 the float64 restatement's own error against the long-double one on that case
                  (0 where the direct DFT is not taken: transforms above 1024 points, the long clips)
  float32 entry   max(16 r32, 8 float32 spacings of the maximum), r32 the float32 restatement's error against the float64 one
parselmouth is not installed where this runs: parity with Praat's own numbers is not pinned by this file.
"""
import math

import numpy as np
import scipy.fft

SHAPES = ("SQUARE", "HAMMING", "BARTLETT", "WELCH", "HANNING", "GAUSSIAN")
DEFAULTS = dict(window_length=0.005, maximum_frequency=5000.0, time_step=0.002, frequency_step=20.0, window_shape="GAUSSIAN")
NARROW = dict(window_length=0.03, frequency_step=100.0)
DFT_MAX_NFFT = 1024
DFT_MAX_WORK = 2.5e7          # frames x window samples x bins of a direct DFT


def window(shape, nw, nspw):
    i = np.arange(1, nw + 1, dtype=np.float64)
    if shape == "GAUSSIAN":
        imid = 0.5 * (nw + 1)
        ph = (i - imid) / nspw
        return (np.exp(-48.0 * ph * ph) - math.exp(-12.0)) / (1.0 - math.exp(-12.0))
    ph = i / nspw
    return {"SQUARE": lambda: np.ones(nw), "HAMMING": lambda: 0.54 - 0.46 * np.cos(2 * np.pi * ph),
            "BARTLETT": lambda: 1.0 - np.abs(2.0 * ph - 1.0), "WELCH": lambda: 1.0 - (2.0 * ph - 1.0) ** 2,
            "HANNING": lambda: 0.5 * (1.0 - np.cos(2 * np.pi * ph))}[shape]()


def geometry(n, sr, **kw):
    """DESIGN.md section 19, line by line -> dict; ValueError where Praat refuses."""
    k = dict(DEFAULTS, **kw)
    wl, shape = k["window_length"], k["window_shape"]
    if shape not in SHAPES:
        raise ValueError("shape")
    dx = 1.0 / sr
    x1 = 0.5 * dx
    nyquist = 0.5 / dx
    phys = 2 * wl if shape == "GAUSSIAN" else wl
    eff_t = wl / math.sqrt(math.pi)
    eff_f = 1 / eff_t
    ts = max(k["time_step"], eff_t / 8)
    fs = max(k["frequency_step"], eff_f / 8)
    dur = dx * n
    nw = math.floor(phys / dx)
    half = nw // 2 - 1
    nw = 2 * half
    if nw < 1:
        raise ValueError("window")
    if phys > dur:
        raise ValueError("short")
    T = 1 + math.floor((dur - phys) / ts)
    t1 = x1 + 0.5 * ((n - 1) * dx - (T - 1) * ts)
    fmax = k["maximum_frequency"]
    if fmax <= 0 or fmax > nyquist:
        fmax = nyquist
    F = math.floor(fmax / fs)
    if F < 1:
        raise ValueError("bands")
    nfft = 1
    while nfft < nw or nfft < 2 * F * (nyquist / fmax):
        nfft *= 2
    bw = max(1, math.floor(fs * dx * nfft))
    bin_hz = 1 / (dx * nfft)
    fs = bw * bin_hz
    F = math.floor(fmax / fs)
    y1 = 0.5 * (fs - bin_hz)
    w = window(shape, nw, phys / dx)
    scale = 1 / np.sum(w * w) / bw
    starts = []
    for j in range(T):
        t = t1 + j * ts
        left = math.floor((t - x1) / dx) + 1
        starts.append(left + 1 - half - 1)
    return dict(n=n, sr=sr, dx=dx, x1=x1, nw=nw, half=half, T=T, t1=t1, ts=ts, fmax=fmax, F=F, nfft=nfft, bw=bw, bin_hz=bin_hz,
                fs=fs, y1=y1, w=w, scale=scale, starts=np.array(starts, dtype=np.int64),
                times=t1 + np.arange(T) * ts, freqs=y1 + np.arange(F) * fs,
                x_grid=t1 - ts / 2 + np.arange(T + 1) * ts, y_grid=y1 - fs / 2 + np.arange(F + 1) * fs)


def _frames(x, g, dtype):
    """x [C, n] -> the windowed frames [C, T, nw] of ``dtype``."""
    x = np.atleast_2d(np.asarray(x)).astype(dtype)
    idx = g["starts"][:, None] + np.arange(g["nw"])[None, :]
    return x[:, idx] * g["w"].astype(dtype)[None, None, :]


def spectrogram(x, sr, dtype=np.float64, **kw):
    """x [n] or [channels, n] -> [F, T] of ``dtype``: every step of the definition in ``dtype``."""
    x = np.atleast_2d(np.asarray(x))
    g = geometry(x.shape[1], sr, **kw)
    X = scipy.fft.rfft(_frames(x, g, dtype), n=g["nfft"], axis=-1)
    assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    P = (X.real * X.real + X.imag * X.imag)[..., :g["nfft"] // 2]         # the Nyquist bin is never used
    P = P.mean(axis=0, dtype=dtype)                                       # [T, nfft / 2]
    F, bw = g["F"], g["bw"]
    out = dtype(g["scale"]) * P[:, :F * bw].reshape(g["T"], F, bw).sum(axis=2, dtype=dtype)
    assert out.dtype == dtype
    return np.ascontiguousarray(out.T)


def has_dft(g):
    return g["nfft"] <= DFT_MAX_NFFT and g["T"] * g["nw"] * g["F"] * g["bw"] <= DFT_MAX_WORK


def spectrogram_dft(x, sr, **kw):
    """The same frames through a direct DFT in long double, bins below F bw only -> [F, T] long double."""
    L = np.longdouble
    x = np.atleast_2d(np.asarray(x))
    g = geometry(x.shape[1], sr, **kw)
    assert has_dft(g)
    fr = _frames(x, g, np.float64).astype(L)                               # (the products are float64's, as in the definition)
    nb = g["F"] * g["bw"]
    two_pi = 8 * np.arctan(L(1))
    nk = (np.arange(g["nw"])[:, None] * np.arange(nb)[None, :]) % g["nfft"]
    ang = two_pi * nk.astype(L) / L(g["nfft"])
    c, s = np.cos(ang), np.sin(ang)
    re, im = fr @ c, fr @ s                                               # [C, T, nb]
    P = (re * re + im * im).mean(axis=0)
    out = L(g["scale"]) * P.reshape(g["T"], g["F"], g["bw"]).sum(axis=2)
    return np.ascontiguousarray(out.T)


def error(P, ref):
    ref = np.asarray(ref)
    m = np.abs(ref).max()
    return float(np.abs(np.asarray(P).astype(ref.dtype) - ref).max() / m)


_REFS = {}


def references(x, sr, **kw):
    """(P64, r64, r32) of a clip, computed once per clip (by its bytes) and left unchanged."""
    x = np.asarray(x)
    key = (x.tobytes(), x.shape, x.dtype.str, sr, tuple(sorted(kw.items())))
    if key not in _REFS:
        x64 = x.astype(np.float64)
        P64 = spectrogram(x64, sr, np.float64, **kw)
        g = geometry(np.atleast_2d(x).shape[1], sr, **kw)
        r64 = error(P64, spectrogram_dft(x64, sr, **kw)) if has_dft(g) else 0.0
        r32 = error(spectrogram(x.astype(np.float32), sr, np.float32, **kw), P64)
        P64.setflags(write=False)
        _REFS[key] = (P64, r64, r32)
    return _REFS[key]


def bound(P64, r64, r32, dtype):
    if dtype == np.float64:
        return max(1e-12, 16 * r64)
    m = np.float32(P64.max())
    return max(16 * r32, 8 * float(np.spacing(m)) / float(m))


def check(got, x, sr, what="", **kw):
    """``got`` [F, T] in the type of ``x``, against the float64 restatement within the entry's bound; prints the figures."""
    x = np.asarray(x)
    P64, r64, r32 = references(x, sr, **kw)
    assert got.shape == P64.shape and got.dtype == x.dtype, (what, got.shape, P64.shape, got.dtype)
    assert np.isfinite(got).all(), what
    e, b = error(got, P64), bound(P64, r64, r32, x.dtype.type)
    print(f"pspec {what or ''} {x.dtype.name} sr {sr} n {x.shape[-1]} {kw or ''}: error {e:.3e}, bound {b:.3e} "
          f"(r64 {r64:.2e}, r32 {r32:.2e})")
    assert e <= b, (what, e, b)
    return e, b


def noise(seed, n, channels=None, dtype=np.float32, amp=0.1):
    """White noise plus a tone: every band holds power."""
    r = np.random.default_rng(seed)
    shape = (n,) if channels is None else (channels, n)
    x = amp * r.standard_normal(shape) + 0.05 * np.sin(2 * np.pi * 0.031 * np.arange(n) + seed)
    return x.astype(dtype)
