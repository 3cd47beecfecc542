"""The yardstick of Praat's intensity contour (modulation_mfcc_amd/pint.py, csrc/mm_pint.hip): DESIGN.md section 20 restated
independently of the package.

  geometry(n, sr, **kw)            the framing arithmetic and the window (float64, the statement's order)
  intensity(x, sr, **kw)           the definition in numpy float64 -> P [T] in Pa^2 (level() gives dB)
  intensity_ld(x, sr, **kw)        the same in np.longdouble with plain ascending sums (cumsum, no pairwise blocks)
  frames(x, n, hw, w, centres)     both of them for any list of centre samples (the clipped windows of the C ABI tests)
  value(y, t1, dt, t, depth)       Vector_getValueAtX at depth 0, 1, 2 in the type of ``y`` (float64 or long double)

error: per frame, |P - P_ref| / P_ref, the maximum over the frames (a frame without power must be 0 exactly).  The bound of
the device's float64 result: max(1e-12, 16 r64), r64 the float64 restatement's own error against the long-double one on
that case -- the project's convention (tests/pspec_oracle.py).  The lookup: 16 x the float64 restatement's error against the
long-double one, at least 1e-12 of the contour's range.
parselmouth is not installed where this runs: parity with Praat's own digits is not pinned by this file.
"""
import math

import numpy as np

L = np.longdouble
DEFAULTS = dict(minimum_pitch=100.0, time_step=None, subtract_mean=True)


def bessel_i0(x):
    """Abramowitz & Stegun 9.8.1 / 9.8.2 for one float."""
    ax = abs(x)
    if ax < 3.75:
        t = (x / 3.75) ** 2
        return 1.0 + t * (3.5156229 + t * (3.0899424 + t * (1.2067492 + t * (0.2659732 + t * (0.0360768 + t * 0.0045813)))))
    t = 3.75 / ax
    return math.exp(ax) / math.sqrt(ax) * (0.39894228 + t * (0.01328592 + t * (0.00225319 + t * (-0.00157565 + t * (
        0.00916281 + t * (-0.02057706 + t * (0.02635537 + t * (-0.01647633 + t * 0.00392377))))))))


def window(hw, dx, phys):
    out = np.empty(2 * hw + 1, dtype=np.float64)
    for i in range(-hw, hw + 1):
        u = dx * i / (0.5 * phys)
        out[i + hw] = bessel_i0((2 * math.pi ** 2 + 0.5) * math.sqrt(max(0.0, 1 - u * u)))
    return out


def geometry(n, sr, **kw):
    """DESIGN.md section 20, line by line -> dict; ValueError where Praat refuses."""
    k = dict(DEFAULTS, **kw)
    dx = 1.0 / sr
    x1 = dx / 2
    phys = 6.4 / k["minimum_pitch"]
    dt = k["time_step"] if k["time_step"] is not None and k["time_step"] > 0 else 0.8 / k["minimum_pitch"]
    hw = math.floor(0.5 * phys / dx)
    dur = n * dx
    if phys > dur:
        raise ValueError("short")
    T = math.floor((dur - phys) / dt) + 1
    t1 = x1 - dx / 2 + dur / 2 - T * dt / 2 + dt / 2
    centres = np.array([math.floor((t1 + j * dt - x1) / dx + 0.5) for j in range(T)], dtype=np.int64)
    return dict(n=n, sr=sr, dx=dx, x1=x1, phys=phys, dt=dt, hw=hw, W=2 * hw + 1, T=T, t1=t1, centres=centres,
                w=window(hw, dx, phys), subtract_mean=k["subtract_mean"], times=t1 + np.arange(T) * dt)


def frames(x, n, hw, w, centres, subtract_mean=True, dtype=np.float64):
    """x [channels, >= n] -> P [len(centres)] of ``dtype`` for a sound of ``n`` samples; a centre outside [0, n) gives 0."""
    x = np.atleast_2d(np.asarray(x))
    ld = dtype is L
    out = np.zeros(len(centres), dtype=dtype)
    wd = np.asarray(w).astype(dtype)
    for k, c in enumerate(np.asarray(centres).tolist()):
        if c < 0 or c >= n:
            continue
        lo, hi = max(0, c - hw), min(n - 1, c + hw)
        ww = wd[lo - c + hw:hi - c + hw + 1]
        sxw, sw = dtype(0), dtype(0)
        for ch in range(x.shape[0]):
            seg = x[ch, lo:hi + 1].astype(dtype)
            if ld:
                m = np.cumsum(seg)[-1] / L(seg.size) if subtract_mean else L(0)
                d = seg - m
                sxw = sxw + np.cumsum(d * d * ww)[-1]
                sw = sw + np.cumsum(ww)[-1]
            else:
                m = seg.mean() if subtract_mean else 0.0
                d = seg - m
                sxw += np.sum(d * d * ww)
                sw += np.sum(ww)
        out[k] = sxw / sw
    return out


def intensity(x, sr, **kw):
    x = np.atleast_2d(np.asarray(x))
    g = geometry(x.shape[1], sr, **kw)
    return frames(x, g["n"], g["hw"], g["w"], g["centres"], g["subtract_mean"], np.float64)


def intensity_ld(x, sr, **kw):
    x = np.atleast_2d(np.asarray(x))
    g = geometry(x.shape[1], sr, **kw)
    return frames(x, g["n"], g["hw"], g["w"], g["centres"], g["subtract_mean"], L)


def level(P):
    """Pa^2 -> dB re 4e-10, -300 below 4e-40, float64."""
    P = np.asarray(P, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(P < 4e-40, -300.0, 10.0 * np.log10(np.maximum(P, 1e-300) / 4e-10))


def error(P, ref):
    """The largest per-frame relative error; inf where a frame without power is not 0 exactly."""
    P, ref = np.asarray(P), np.asarray(ref)
    assert P.shape == ref.shape, (P.shape, ref.shape)
    zero = ref == 0
    if (P[zero] != 0).any() or not np.isfinite(P.astype(np.float64)).all():
        return float("inf")
    if zero.all():
        return 0.0
    return float(np.max(np.abs(P[~zero].astype(ref.dtype) - ref[~zero]) / ref[~zero]))


_REFS = {}


def references(x, sr, **kw):
    """(P64, r64) of a clip, computed once per clip (by its bytes) and left unchanged."""
    x = np.asarray(x)
    key = (x.tobytes(), x.shape, x.dtype.str, sr, tuple(sorted(kw.items())))
    if key not in _REFS:
        x64 = x.astype(np.float64)
        P64 = intensity(x64, sr, **kw)
        r64 = error(P64, intensity_ld(x64, sr, **kw))
        P64.setflags(write=False)
        _REFS[key] = (P64, r64)
    return _REFS[key]


def bound(r64):
    return max(1e-12, 16 * r64)


def check(got, x, sr, what="", **kw):
    """``got`` [T] float64 (Pa^2) against the float64 restatement of ``x`` (whatever its type: the samples are widened)
    within the bound; prints the figures."""
    P64, r64 = references(x, sr, **kw)
    got = np.asarray(got)
    assert got.shape == P64.shape and got.dtype == np.float64, (what, got.shape, P64.shape, got.dtype)
    e, b = error(got, P64), bound(r64)
    print(f"pint {what} {np.asarray(x).dtype.name} sr {sr} shape {np.asarray(x).shape} {kw or ''}: error {e:.3e}, bound {b:.3e} "
          f"(r64 {r64:.2e})")
    assert e <= b, (what, e, b)
    return e, b


def check_frames(got, x, n, hw, w, centres, what="", subtract_mean=True):
    """The same for any centre list (clipped windows)."""
    P64 = frames(x, n, hw, w, centres, subtract_mean, np.float64)
    r64 = error(P64, frames(x, n, hw, w, centres, subtract_mean, L))
    e, b = error(np.asarray(got), P64), bound(r64)
    print(f"pint {what} centres {list(centres)[:6]}..: error {e:.3e}, bound {b:.3e} (r64 {r64:.2e})")
    assert e <= b, (what, e, b)
    return e, b


# ---- the lookup ---------------------------------------------------------------------------------------------------------------
DEPTHS = {"nearest": 0, "linear": 1, "cubic": 2}


def value(y, t1, dt, t, depth):
    """Vector_getValueAtX over NUM_interpolate_sinc at depth 0, 1, 2, in the type of ``y``; NaN outside the domain."""
    y = np.asarray(y)
    F = y.dtype.type
    T = y.shape[0]
    t1, dt, t = F(t1), F(dt), F(t)
    lo = t1 - dt / 2
    if not (t >= lo and t <= lo + T * dt):
        return F("nan")
    s = (t - t1) / dt
    if s <= 0:
        return y[0]
    if s >= T - 1:
        return y[T - 1]
    a = int(np.floor(s))
    b = a + 1
    if s == a:
        return y[a]
    depth = min(depth, a + 1, T - 1 - a)
    if depth <= 0:
        return y[int(np.floor(s + F(0.5)))]
    if depth == 1:
        return y[a] + (s - a) * (y[b] - y[a])
    dl, dr = (y[b] - y[a - 1]) / 2, (y[b + 1] - y[a]) / 2
    fl, fr = s - a, b - s
    return y[a] * fr + y[b] * fl - fl * fr * (F(0.5) * (dr - dl) + (fl - F(0.5)) * (dl + dr - 2 * (y[b] - y[a])))


def check_values(got, y, t1, dt, times, depth, what=""):
    """``got`` [q] float64 against value() in float64; NaN exactly where the restatement has it."""
    y = np.asarray(y, dtype=np.float64)
    want = np.array([value(y, t1, dt, t, depth) for t in times], dtype=np.float64)
    ld = np.array([value(y.astype(L), t1, dt, t, depth) for t in times], dtype=L)
    got = np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    rng = float(y.max() - y.min()) or float(np.abs(y).max()) or 1.0
    r = float(np.max(np.abs(want[ok].astype(L) - ld[ok]))) if ok.any() else 0.0
    e = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    b = max(16 * r, 1e-12 * rng)
    print(f"pint value {what} depth {depth} T {y.shape[0]} q {len(times)}: error {e:.3e}, bound {b:.3e} (r {r:.2e})")
    assert e <= b, (what, e, b)
    return e, b


def noise(seed, n, channels=None, dtype=np.float32, amp=0.1):
    """White noise plus a tone."""
    r = np.random.default_rng(seed)
    shape = (n,) if channels is None else (channels, n)
    x = amp * r.standard_normal(shape) + 0.05 * np.sin(2 * np.pi * 0.031 * np.arange(n) + seed)
    return x.astype(dtype)
