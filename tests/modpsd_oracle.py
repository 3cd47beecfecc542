"""The yardstick of the Welch modulation power spectrum (modulation_psd_batch; include/modmfcc_modpsd.h), built like
tests/modspec_oracle.py, whose fixed rows (cases) and EPS it uses.

Reference: scipy.signal.welch in float64 on the float32 rows with the float32-rounded window.  Powers are compared as
amplitudes, A = sqrt(P_ref / (s d_k)) and G = sqrt(got / (s d_k)) -- the root-mean-square over the row's segments of |X_k| --
so that the measure is that of a float32 FFT:

    c[r, k] = |G - A| / (2^-24 (A + log2(nfft) N_r)),    N_r^2 = mean over the row's segments of (||w x_seg||^2 + ||w trend_seg||^2)

A pays for rounding the stored value, log2(nfft) N_r is the propagated-error term of a float32 FFT of nfft points, and the
trend (the float64 mean or least-squares line the detrend removes; zero for detrend=False) makes a large offset, or an impulse
under a zero of the taper, pay with the row's own magnitude: what is subtracted was rounded to float32 at that size.  Without
the trend term the measure is infinite for an impulse at sample 0 under a Hann window.  Any got < 0 is an error outright; a
row of zeros must come back as exact zeros.

The bound of every test is  c.max() <= MARGIN * max(C_ref, 1),  C_ref the largest c an independent float32 transform
reaches on the same rows with the same parameters: scipy.fft.rfft (pocketfft, complex64) of the float32 windowed segments,
squared and averaged in float64 (psd32).  It is computed here, on the host, never from the code under test.  (welch itself
on float32 input is no such reference: its float32 mean loses up to c ~ 200 at many segments.)

Nothing in the package imports this module.
"""
from __future__ import annotations

import numpy as np

from modspec_oracle import EPS, ROW_ZERO, cases, take  # noqa: F401

MARGIN = 4.0


class Params:
    """One parameter set: the float32 window, the scale factor s, the per-bin factor d."""

    def __init__(self, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", scaling="density"):
        from scipy.signal import get_window
        self.fs, self.nperseg = float(fs), int(nperseg)
        self.noverlap = self.nperseg // 2 if noverlap is None else int(noverlap)
        self.nfft = max(32, 1 << (self.nperseg - 1).bit_length()) if nfft is None else int(nfft)
        self.detrend, self.scaling = detrend, scaling
        self.window_arg = window
        w = get_window(window, self.nperseg) if isinstance(window, (str, tuple)) else np.asarray(window)
        self.w = np.ascontiguousarray(w, dtype=np.float32)
        w64 = self.w.astype(np.float64)
        self.s = 1.0 / (self.fs * (w64 * w64).sum()) if scaling == "density" else 1.0 / w64.sum() ** 2
        self.d = np.full(self.nfft // 2 + 1, 2.0)
        self.d[0] = self.d[-1] = 1.0
        self.step = self.nperseg - self.noverlap
        self.bins = self.nfft // 2 + 1

    def kwargs(self):
        """The keywords of modulation_psd_batch (the window as it was given here: a name, a tuple or an array)."""
        return dict(window=self.window_arg, nperseg=self.nperseg, noverlap=self.noverlap, nfft=self.nfft, detrend=self.detrend,
                    scaling=self.scaling)

    def key(self):
        return (self.fs, self.nperseg, self.noverlap, self.nfft, self.detrend, self.scaling, self.w.tobytes())

    def num_segments(self, n):
        return 0 if n < self.nperseg else (int(n) - self.noverlap) // self.step


def welch64(x, p):
    """(f, P): scipy.signal.welch in float64 on the float32 rows."""
    from scipy.signal import welch
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-1] >= p.nperseg, (x.dtype, x.shape, p.nperseg)
    return welch(x.astype(np.float64), fs=p.fs, window=p.w, nperseg=p.nperseg, noverlap=p.noverlap, nfft=p.nfft,
                 detrend=p.detrend, return_onesided=True, scaling=p.scaling, axis=-1, average="mean")


def segments(x, p):
    """float64 [rows, K, nperseg]: the row's segments, starting at i * step."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    K = p.num_segments(x.shape[-1])
    assert K >= 1
    v = np.lib.stride_tricks.sliding_window_view(x, p.nperseg, axis=-1)[:, ::p.step][:, :K]
    assert v.shape[1] == K
    return v


def trend(seg, p):
    """The float64 trend the detrend removes from every segment (zeros for detrend=False)."""
    from scipy.signal import detrend as sdetrend
    if p.detrend is False or p.detrend is None:
        return np.zeros_like(seg)
    return seg - sdetrend(seg, axis=-1, type=p.detrend)


def row_norm(x, p):
    """N_r [rows, 1]."""
    seg = segments(x, p)
    w = p.w.astype(np.float64)
    e = ((w * seg) ** 2).sum(axis=-1) + ((w * trend(seg, p)) ** 2).sum(axis=-1)
    return np.sqrt(e.mean(axis=-1))[:, None]


def psd32(x, p):
    """The independent float32 transform: float64 detrend, rounded to float32, times the float32 window in float32,
    scipy.fft.rfft in complex64, |.|^2 and the mean over segments in float64, scaled -> float64 [rows, bins]."""
    from scipy import fft as sfft
    seg = segments(x, p)
    y = (seg - trend(seg, p)).astype(np.float32) * p.w
    assert y.dtype == np.float32
    X = sfft.rfft(y, n=p.nfft, axis=-1)
    assert X.dtype == np.complex64
    P = (X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2).mean(axis=1)
    return P * (p.s * p.d)


def bin_error(got, x, p):
    """c[r, k]; inf where a zero row did not come back as zeros or a value is NaN; AssertionError for a negative power."""
    x = np.atleast_2d(np.asarray(x))
    got = np.asarray(got, dtype=np.float64).reshape(x.shape[0], p.bins)
    assert not (got < 0).any(), "negative power"
    _, P = welch64(x, p)
    A = np.sqrt(P / (p.s * p.d))
    G = np.sqrt(got / (p.s * p.d))
    den = EPS * (A + np.log2(p.nfft) * row_norm(x, p))
    err = np.abs(G - A)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, c)


def rows_for(p, T):
    """The fixed rows [16, T] of modspec_oracle.cases for these parameters (cosines on bins of max(nfft, T) points)."""
    return cases(max(p.nfft, int(T)), int(T))


_C_REF = {}


def c_ref(p, T):
    """The largest c of the independent float32 transform on rows_for(p, T) (kept per parameter set and T)."""
    k = (p.key(), int(T))
    if k not in _C_REF:
        x = rows_for(p, T)
        _C_REF[k] = float(bin_error(psd32(x, p), x, p).max())
    return _C_REF[k]


def tolerance(p, T, margin=None):
    return (MARGIN if margin is None else margin) * max(c_ref(p, T), 1.0)


def check(got, x, p, what="", margin=None):
    """Asserts bin_error(got, x, p) <= tolerance(p, T) on every row (x: rows of rows_for(p, T), in any selection);
    returns the largest c."""
    x = np.atleast_2d(np.asarray(x))
    c = bin_error(got, x, p)
    tol = tolerance(p, x.shape[-1], margin)
    per_row = c.max(axis=-1)
    bad = np.flatnonzero(~(per_row <= tol))
    assert bad.size == 0, (f"{what}: nperseg {p.nperseg} nfft {p.nfft} noverlap {p.noverlap} detrend {p.detrend} {p.scaling} "
                           f"T {x.shape[-1]}: {bad.size} of {per_row.size} rows beyond c = {tol:.2f} "
                           f"(C_ref {c_ref(p, x.shape[-1]):.2f}); worst row {int(per_row.argmax())} c = {per_row.max():.2f}, "
                           f"first rows {bad[:8].tolist()}")
    return float(per_row.max())
