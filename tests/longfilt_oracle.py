"""``scipy.signal.filtfilt(b, 1, x)`` and ``scipy.signal.savgol_filter(..., mode='interp')`` restated in ``np.longdouble``
-- the yardstick of the device's long FIR / Savitzky-Golay filters, in the manner of tests/sos_oracle.py: with it scipy's
own float64 error becomes a measurable quantity, the unit of the ratio rule in tests/test_gpu_longfilt.py.

FIR.  filtfilt pads by the odd extension of 3 L samples (formed in the input's OWN type: a float32 curve is extended in
float32 arithmetic, then widened), filters forwards and backwards from lfilter_zi states and crops.  For an FIR filter
both start-up transients (L - 1 samples) lie inside the cropped padding, so every kept output is exactly

    y[i] = sum_k h[k] ext[3 L + i - (L - 1) + k],   h = b (*) reversed b   (2 L - 1 taps)

which is what is summed here, h and the sum in the 64-bit-mantissa type.

Savitzky-Golay.  The least-squares polynomial of degree p over a window of W samples, by ORTHOGONALISATION (twice-applied
modified Gram-Schmidt of the monomials on the abscissa scaled to [-1, 1], V = Q R) where scipy solves raw-power
least-squares systems (lstsq for the taps, polyfit at the edges): the weight row of "deriv-th derivative of the fit at window position u" is
w(u) = Q R^-T d(u), d(u)_k = k! / (k - deriv)! u^(k - deriv) (scaled).  Interior output i is w((W - 1) / 2) on
x[i - (W - 1) // 2 ...] -- scipy's savgol_coeffs evaluates an even window's fit at the half-sample centre and convolve1d
puts that kernel's origin at W // 2, which is this alignment (calc.velocity_stencil documents the same rule) -- for i in
[W // 2, n - W // 2); the first / last W // 2 outputs are w(i) on x[:W] and w(W - W // 2 + i) on x[-W:].

Nothing in the package imports this module.

    fir_filtfilt_ext_ld(taps, x)                        [n] or [rows, n] -> np.longdouble
    savgol_weights_ld(W, p, deriv, delta, pos)          [len(pos)][W] weight rows (np.longdouble)
    savgol_ext_ld(x, W, p, deriv=0, delta=1.0)          [n] or [rows, n] -> np.longdouble
    rel_err(a, ref)                                     max|a - ref| / max|ref|
"""
from __future__ import annotations

import numpy as np

from sos_oracle import LD, odd_ext, rel_err  # noqa: F401  (the same extended type, the same guard on its precision)


def fir_filtfilt_ext_ld(taps, x):
    b = np.asarray(taps, dtype=np.float64).ravel()
    L = len(b)
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    edge = 3 * L
    if x.shape[-1] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    ext = odd_ext(x, edge)                              # float32 stays float32 here, as in scipy
    bl = b.astype(LD)
    h = np.zeros(2 * L - 1, dtype=LD)
    for i in range(L):                                  # h[d + L - 1] = sum_i b[i] b[i - d]
        for j in range(L):
            h[i - j + L - 1] += bl[i] * bl[j]
    rows = ext.reshape(-1, ext.shape[-1]).astype(LD)
    n = x.shape[-1]
    out = np.zeros((rows.shape[0], n), dtype=LD)
    first = edge - (L - 1)
    for k in range(2 * L - 1):
        out += h[k] * rows[:, first + k:first + k + n]
    return out.reshape(x.shape)


def _qr_ld(V):
    """V = Q R by modified Gram-Schmidt, every column orthogonalised twice, in long double."""
    m, k = V.shape
    Q = np.array(V, dtype=LD)
    R = np.zeros((k, k), dtype=LD)
    for j in range(k):
        for _ in range(2):
            for i in range(j):
                r = (Q[:, i] * Q[:, j]).sum()
                R[i, j] += r
                Q[:, j] = Q[:, j] - r * Q[:, i]
        R[j, j] = np.sqrt((Q[:, j] * Q[:, j]).sum())
        Q[:, j] = Q[:, j] / R[j, j]
    return Q, R


def savgol_weights_ld(W, p, deriv, delta, pos):
    W, p, deriv = int(W), int(p), int(deriv)
    if p >= W:
        raise ValueError("polyorder must be less than window_length.")
    s = LD(2) / LD(W - 1) if W > 1 else LD(1)
    mid = LD(W - 1) / LD(2)
    t = (np.arange(W).astype(LD) - mid) * s
    V = np.stack([t ** k for k in range(p + 1)], axis=1)
    Q, R = _qr_ld(V)
    rows = []
    for u in np.asarray(pos, dtype=np.float64):
        tu = (LD(u) - mid) * s
        d = np.zeros(p + 1, dtype=LD)
        for k in range(deriv, p + 1):
            f = LD(1)
            for m in range(k - deriv + 1, k + 1):
                f *= m
            d[k] = f * tu ** (k - deriv)
        z = np.zeros(p + 1, dtype=LD)                   # R^T z = d: forward substitution
        for i in range(p + 1):
            z[i] = (d[i] - (R[:i, i] * z[:i]).sum()) / R[i, i]
        rows.append((Q * z[None, :]).sum(axis=1) * (s / LD(delta)) ** deriv)
    return np.array(rows, dtype=LD).reshape(len(rows), W)


def savgol_ext_ld(x, W, p, deriv=0, delta=1.0):
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    W = int(W)
    n = x.shape[-1]
    half = W // 2
    pos = np.concatenate(([(W - 1) / 2.0], np.arange(half), np.arange(W - half, W)))
    w = savgol_weights_ld(W, p, deriv, delta, pos)
    if W > n:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    rows = x.reshape(-1, n).astype(LD)
    out = np.zeros(rows.shape, dtype=LD)
    m = n - 2 * half                                    # interior outputs [half, n - half)
    if m > 0:
        first = half - (W - 1) // 2
        for k in range(W):
            out[:, half:n - half] += w[0, k] * rows[:, first + k:first + k + m]
    if half:
        out[:, :half] = (w[1:1 + half][None, :, :] * rows[:, None, :W]).sum(axis=2)
        out[:, n - half:] = (w[1 + half:][None, :, :] * rows[:, None, n - W:]).sum(axis=2)
    return out.reshape(x.shape)


def curve_rows(rng, rows, n, dtype=np.float64):
    """|random walk| + noise (the shape of an envelope or an articulograph channel: a large slow part, a small fast one)."""
    return (np.abs(rng.standard_normal((rows, n)).cumsum(axis=1)) + rng.standard_normal((rows, n))).astype(dtype)
