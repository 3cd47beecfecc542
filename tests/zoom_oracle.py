"""The yardstick of the spline zoom (zoom_batch, mm_zoom2d_f32 / _f64): scipy.ndimage.zoom itself, the measure and its
bound, and a restatement of scipy's prefilter and evaluation in NumPy for tests/test_zoom_host.py and
tests/test_gpu_zoom.py.

  want     scipy.ndimage.zoom(x, zoom, order=, mode=, cval=, prefilter=) on the last two axes, in the input's dtype.
  c        max|got - want| / max|want| over the image (a NaN or an infinity where scipy has a number is an error of any
           size).
  bound    max(1e-12, 16 * spread), at most 1e-10 (asserted).  spread is scipy's own rounding on the case: scipy against
           `restate` in np.longdouble -- the same prefilter recursion (poles, gain, whole-sample-symmetric initialisation)
           and the same evaluation (coordinate, start index, mirrored taps, cardinal B-spline weights) -- relative to
           max|want|.  For a float32 result one float32 spacing of max|want| is added: scipy rounds its float64 result once.
  cval     where scipy returns cval (constant mode: the coordinate outside [0, n - 1], which the last row or column is
           when (n_out - 1) * step rounds one ulp past n - 1) the result must be cval bit for bit; those positions are
           compared against scipy alone.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.ndimage

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: no yardstick for scipy's rounding"

FLOOR, MARGIN, CEILING = 1e-12, 16.0, 1e-10
MODES = ("constant", "mirror")
ORDERS = (0, 1, 2, 3, 4, 5)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def poles(order, dt=np.longdouble):
    s = lambda v: np.sqrt(dt(v))
    if order == 2:
        return [s(8) - 3]
    if order == 3:
        return [s(3) - 2]
    if order == 4:
        return [s(664 - s(438976)) + s(304) - 19, s(664 + s(438976)) - s(304) - 19]
    if order == 5:
        return [s(dt(67.5) - s(dt(4436.25))) + s(dt(26.25)) - dt(6.5), s(dt(67.5) + s(dt(4436.25))) - s(dt(26.25)) - dt(6.5)]
    return []


def spline_filter_axis(a, order, axis, dt=np.longdouble):
    """scipy's spline_filter1d(mode='mirror') along one axis, in the type dt: the gain, then per pole the causal pass from
    the whole-sample-symmetric initial value and the anticausal pass."""
    c = np.moveaxis(np.array(a, dtype=dt), axis, 0).copy()
    n = c.shape[0]
    if order < 2 or n == 1:
        return np.moveaxis(c, 0, axis)
    ps = poles(order, dt)
    gain = dt(1)
    for z in ps:
        gain *= (1 - z) * (1 - 1 / z)
    c *= gain
    for z in ps:
        zn = z ** (n - 1)
        c0 = c[0] + zn * c[n - 1]
        zi = z
        for i in range(1, n - 1):
            c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
            zi = zi * z
        c[0] = c0 / (1 - zn * zn)
        for i in range(1, n):
            c[i] += z * c[i - 1]
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def spline_filter2(x, order, dt=np.longdouble):
    return spline_filter_axis(spline_filter_axis(x, order, -2, dt), order, -1, dt)


def bspline(order, x):
    """The centred cardinal B-spline of degree `order` at the distances x >= 0 (an array, its type kept)."""
    dt = x.dtype.type
    out = np.zeros_like(x)
    if order == 1:
        m = x < 1
        out[m] = 1 - x[m]
    elif order == 2:
        m = x < 0.5
        out[m] = dt(0.75) - x[m] * x[m]
        m = (x >= 0.5) & (x < 1.5)
        t = dt(1.5) - x[m]
        out[m] = t * t / 2
    elif order == 3:
        m = x < 1
        out[m] = (x[m] * x[m] * (x[m] - 2) * 3 + 4) / 6
        m = (x >= 1) & (x < 2)
        t = 2 - x[m]
        out[m] = t * t * t / 6
    elif order == 4:
        m = x < 0.5
        t = x[m] * x[m]
        out[m] = t * (t / 4 - dt(0.625)) + dt(115) / 192
        m = (x >= 0.5) & (x < 1.5)
        t = x[m]
        out[m] = t * (t * (t * (dt(5) / 6 - t / 6) - dt(1.25)) + dt(5) / 24) + dt(55) / 96
        m = (x >= 1.5) & (x < 2.5)
        t = x[m] - dt(2.5)
        t = t * t
        out[m] = t * t / 24
    elif order == 5:
        m = x < 1
        t = x[m]
        q = t * t
        out[m] = q * (q * (dt(0.25) - t / 12) - dt(0.5)) + dt(11) / 20
        m = (x >= 1) & (x < 2)
        t = x[m]
        out[m] = t * (t * (t * (t * (t / 24 - dt(0.375)) + dt(1.25)) - dt(1.75)) + dt(0.625)) + dt(17) / 40
        m = (x >= 2) & (x < 3)
        t = 3 - x[m]
        q = t * t
        out[m] = t * q * q / 120
    else:
        raise ValueError(order)
    return out


def out_size(n, zoom):
    return int(round(n * zoom))


def step(n, n_out):
    return np.float64(n - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(1.0)


def axis_plan(n, n_out, order, mode, dt=np.longdouble):
    """-> (outside [n_out] bool, taps [n_out, order + 1] mirrored indices, weights [n_out, order + 1] of type dt)."""
    z = step(n, n_out)
    cc = np.arange(n_out, dtype=np.float64) * z                    # one float64 multiply
    outside = ((cc < 0) | (cc > n - 1)) if mode == "constant" else np.zeros(n_out, dtype=bool)
    if order == 0:
        start = np.floor(cc + 0.5).astype(np.int64)
        w = np.ones((n_out, 1), dtype=dt)
    else:
        start = (np.floor(cc + 0.5) if order % 2 == 0 else np.floor(cc)).astype(np.int64) - order // 2
        taps = start[:, None] + np.arange(order + 1)[None, :]
        w = bspline(order, np.abs(cc.astype(dt)[:, None] - taps.astype(dt)))
    taps = start[:, None] + np.arange(order + 1 if order else 1)[None, :]
    if n == 1:
        taps = np.zeros_like(taps)
    else:
        p = 2 * n - 2
        taps = np.mod(taps, p)
        taps = np.where(taps >= n, p - taps, taps)
    return outside, taps, w


def restate(x, zoom, order, mode="constant", cval=0.0, prefilter=True, dt=np.longdouble):
    """scipy.ndimage.zoom on a 2-D image restated: -> (result of type dt, outside mask)."""
    x = np.asarray(x)
    zy, zx = (zoom, zoom) if np.isscalar(zoom) else zoom
    h, w = x.shape
    ho, wo = out_size(h, zy), out_size(w, zx)
    c = spline_filter2(x, order, dt) if prefilter and order > 1 else np.array(x, dtype=dt)
    oy, ty, wy = axis_plan(h, ho, order, mode, dt)
    ox, tx, wx = axis_plan(w, wo, order, mode, dt)
    rows = np.zeros((ho, w), dtype=dt)
    for b in range(ty.shape[1]):
        rows += wy[:, b, None] * c[ty[:, b], :]
    out = np.zeros((ho, wo), dtype=dt)
    for a in range(tx.shape[1]):
        out += rows[:, tx[:, a]] * wx[None, :, a]
    outside = oy[:, None] | ox[None, :]
    out[outside] = dt(cval)
    return out, outside


# ---- the measure ---------------------------------------------------------------------------------------------------------------
def scipy_zoom(x, zoom, order, mode="constant", cval=0.0, prefilter=True):
    return scipy.ndimage.zoom(np.asarray(x), zoom, order=order, mode=mode, cval=cval, prefilter=prefilter)


def measure(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    d[~np.isfinite(got)] = np.inf
    return float(d.max() / max(np.abs(want).max(), 1e-300))


def spread_of(want64, exact):
    return float(np.abs(exact - want64.astype(np.longdouble)).max() / max(np.abs(want64).max(), 1e-300))


def bound_of(sp, dtype=np.float64, scale=1.0):
    b = max(FLOOR, MARGIN * sp)
    assert b <= CEILING, f"bound {b:.3e} beyond {CEILING:g}: the case is too ill-conditioned to be a test"
    if np.dtype(dtype) == np.float32:
        b += float(np.spacing(np.float32(scale))) / max(scale, 1e-300)
    return b


def reference(x, zoom, order, mode="constant", cval=0.0, prefilter=True):
    """(want in x's dtype, outside mask, bound) of one image: scipy's result, where it is cval, and the bound from scipy's
    own rounding (scipy on the float64 input against the long-double restatement)."""
    x = np.asarray(x)
    want = scipy_zoom(x, zoom, order, mode, cval, prefilter)
    want64 = want if x.dtype == np.float64 else scipy_zoom(x.astype(np.float64), zoom, order, mode, cval, prefilter)
    exact, outside = restate(x.astype(np.float64), zoom, order, mode, cval, prefilter)
    sp = spread_of(want64, exact)
    return want, outside, bound_of(sp, x.dtype, float(np.abs(want64).max())), sp


def check(got, x, zoom, order, mode="constant", cval=0.0, prefilter=True, what=""):
    """Assert c <= bound, the dtype, the shape, and cval bit for bit where scipy returns it; -> (c, bound, spread)."""
    want, outside, b, sp = reference(x, zoom, order, mode, cval, prefilter)
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    c = measure(got, want)
    tag = what or f"{x.shape} x {zoom} order {order} {mode} cval {cval}"
    print(f"zoom {tag}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}, cval positions {int(outside.sum())}")
    assert c <= b, f"{tag}: c = {c:.3e} beyond the bound {b:.3e} (spread {sp:.3e})"
    if outside.any():
        assert (want[outside] == want.dtype.type(cval)).all(), "scipy itself has no cval where the restatement expects it"
        assert got[outside].tobytes() == want[outside].tobytes(), f"{tag}: the cval positions are not cval bit for bit"
    return c, b, sp


def check_filter(got, x, order, what=""):
    """The prefilter alone against scipy.ndimage.spline_filter(mode='mirror') on the last two axes."""
    x = np.asarray(x)
    want = scipy.ndimage.spline_filter(x, order=order, mode="mirror", output=x.dtype)
    want64 = scipy.ndimage.spline_filter(x.astype(np.float64), order=order, mode="mirror")
    sp = spread_of(want64, spline_filter2(x.astype(np.float64), order))
    b = bound_of(sp, x.dtype, float(np.abs(want64).max()))
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape
    c = measure(got, want)
    print(f"spline_filter {what or x.shape} order {order}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}")
    assert c <= b, f"spline_filter {what or x.shape} order {order}: c = {c:.3e} beyond the bound {b:.3e}"
    return c, b, sp


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    import zlib
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


@functools.lru_cache(maxsize=None)
def _image(h, w, key):
    a = _rng("image", h, w, key).standard_normal((h, w))
    a.setflags(write=False)
    return a


def image(h, w, key=0, dtype=np.float64):
    """A unit-variance image (the hardest content for the prefilter: no smoothness to lean on); read-only."""
    a = _image(h, w, key)
    return a if dtype == np.float64 else a.astype(dtype)


@functools.lru_cache(maxsize=None)
def power(h, w, key=0):
    """A strictly positive power image with the dynamic range of a speech spectrogram (about 90 dB)."""
    r = _rng("power", h, w, key)
    f, t = np.arange(h)[:, None], np.arange(w)[None, :]
    db = -30.0 - 40.0 * f / h + 20.0 * np.sin(t / 17.0 + f / 9.0) + 6.0 * r.standard_normal((h, w))
    p = 10.0 ** (db / 10.0)
    p.setflags(write=False)
    return p
