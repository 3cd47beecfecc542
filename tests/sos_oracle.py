"""``scipy.signal.sosfiltfilt`` (default padtype / padlen) restated sequentially in ``np.longdouble`` -- the yardstick of
the device IIR filter where scipy's own float64 rounding is no longer negligible (poles within 1e-3 of the unit circle).

The steps are scipy's (signal/_filter_design.py, _signaltools.py): the padlen rule, the odd extension (formed in the
input's own type: a float32 curve is extended in float32 arithmetic, then upcast), ``sosfilt_zi`` with its running gain,
the direct-form-II-transposed recursion forwards, the same over the reversed result, the crop.  Everything after the
extension -- the zi solve included -- is carried in the 64-bit-mantissa extended type, so what is left against the exact
result of the given float64 coefficients is ~1e-19 times the conditioning, three orders below scipy's float64.

Nothing in the package imports this module.

    sosfiltfilt_ext(sos, x)   [n] or [rows, n] -> float64 (rounded once from the extended result)
    padlen_of(sos)            scipy's edge length 3 * ntaps
    rel_err(a, ref)           max|a - ref| / max|ref|
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
# an x87 80-bit (or wider) long double is what makes this a yardstick; a platform where longdouble is float64 must
# fail here, not pass with a reference no better than the code under test
assert np.finfo(LD).eps < 1e-18, "sos_oracle needs an extended-precision np.longdouble (eps < 1e-18)"


def check_sos(sos):
    """scipy's _validate_sos: the same two ValueErrors, float64 [n_sections, 6] back."""
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    if sos.ndim != 2:
        raise ValueError("sos array must be 2D")
    if sos.shape[1] != 6:
        raise ValueError("sos array must be shape (n_sections, 6)")
    if not (sos[:, 3] == 1).all():
        raise ValueError("sos[:, 3] should be all ones")
    return sos


def padlen_of(sos):
    sos = check_sos(sos)
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def odd_ext(x, n):
    """scipy.signal._arraytools.odd_ext along the last axis, in x's own dtype."""
    x = np.asarray(x)
    left = 2 * x[..., :1] - x[..., n:0:-1]
    right = 2 * x[..., -1:] - x[..., -2:-(n + 2):-1]
    return np.concatenate((left, x, right), axis=-1)


def sosfilt_zi_ext(sos):
    """sosfilt_zi: per section the steady state of a unit step (lfilter_zi: (I - companion(a)^T) zi = b[1:] - a[1:] b0),
    scaled by the gain of the sections before it."""
    zi = []
    scale = LD(1)
    for b0, b1, b2, _, a1, a2 in ([LD(v) for v in row] for row in sos):
        B0, B1 = b1 - a1 * b0, b2 - a2 * b0
        z0 = (B0 + B1) / (LD(1) + a1 + a2)
        zi.append((scale * z0, scale * (B1 - a2 * z0)))
        scale *= (b0 + b1 + b2) / (LD(1) + a1 + a2)
    return zi


def _sosfilt_row(sos_ld, zi, seq):
    """One pass over a list of longdouble samples (in place), scalar arithmetic.  Every section starts from zi * the
    FIRST INPUT sample, as scipy's zi * x_0 does: the running gain is already inside zi."""
    first = seq[0]
    for (b0, b1, b2, a1, a2), (zi0, zi1) in zip(sos_ld, zi):
        z0, z1 = zi0 * first, zi1 * first
        for i, x in enumerate(seq):
            y = b0 * x + z0
            z0 = b1 * x - a1 * y + z1
            z1 = b2 * x - a2 * y
            seq[i] = y
    return seq


def sosfiltfilt_ext_ld(sos, x):
    """The extended-precision result itself (np.longdouble), [n] or [rows, n]."""
    sos = check_sos(sos)
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    edge = padlen_of(sos)
    if x.shape[-1] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    ext = odd_ext(x, edge)                          # float32 stays float32 here, as in scipy
    sos_ld = [tuple(LD(v) for v in (r[0], r[1], r[2], r[4], r[5])) for r in sos]
    zi = sosfilt_zi_ext(sos)
    rows = ext.reshape(-1, ext.shape[-1])
    out = np.empty((rows.shape[0], x.shape[-1]), dtype=LD)
    for r, row in enumerate(rows):
        seq = [LD(v) for v in row]
        _sosfilt_row(sos_ld, zi, seq)
        seq.reverse()
        _sosfilt_row(sos_ld, zi, seq)
        seq.reverse()
        out[r] = seq[edge:len(seq) - edge]
    return out.reshape(x.shape)


def sosfiltfilt_ext(sos, x):
    return sosfiltfilt_ext_ld(sos, x).astype(np.float64)


def rel_err(a, ref):
    a = np.asarray(a, dtype=LD)
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def envelope_rows(rng, rows, n, dtype=np.float64):
    """|random walk| + noise: the shape of an amplitude envelope (large slow part, small fast part)."""
    return (np.abs(rng.standard_normal((rows, n)).cumsum(axis=1)) + rng.standard_normal((rows, n))).astype(dtype)


def foreign_designs():
    """Sections no Butterworth design produces: zeros on the unit circle at arbitrary angles (b2 != 0, b1 != +-2 b0),
    a high-pass FIRST section (the running gain of sosfilt_zi becomes 0 for every later one), first-order sections
    with b2 == 0 and a2 == 0 in unequal numbers (the padlen rule takes the smaller count), a pure gain."""
    from scipy import signal as S
    return {
        "ellip6_low": S.ellip(6, 0.5, 60, 0.05, output="sos"),
        "ellip3_high": S.ellip(3, 1, 40, 0.2, "high", output="sos"),
        "cheby1_5_high": S.cheby1(5, 1, 0.1, "high", output="sos"),
        "cheby2_8_low": S.cheby2(8, 60, 0.1, output="sos"),
        "cheby2_4_band": S.cheby2(4, 40, [0.1, 0.3], "band", output="sos"),
        "bessel2_band": S.bessel(2, [0.01, 0.05], "band", output="sos"),
        "notch": S.tf2sos(*S.iirnotch(0.1, 30)),
        "peak": S.tf2sos(*S.iirpeak(0.2, 10)),
        "b2zero_a2zero": np.array([[1, 1, 0, 1, -0.5, 0.2], [1, 0.3, 0.1, 1, -0.4, 0]], dtype=np.float64),
        "two_b2zero": np.array([[1, 1, 0, 1, -0.5, 0.2], [1, -1, 0, 1, -0.3, 0.1]], dtype=np.float64),
        "gain_half": np.array([[0.5, 0, 0, 1, 0, 0]], dtype=np.float64),
    }
