"""The yardstick of the Lomb-Scargle modulation spectrum (modulation_lombscargle_batch, mm_lombscargle_f64): scipy on the
valid samples of a row, the measure and its bound, the one-pass algebra of the kernel in NumPy, and the fixtures of
tests/test_lomb_host.py and tests/test_gpu_lomb.py.

  want     scipy.signal.lombscargle(t[valid], x[valid], 2 pi f, precenter=, normalize=, floating_mean=), valid = the
           non-NaN samples in front of the row's length (scipy 1.15; a warning about the legacy keyword is silenced).
  c        max|got - want| / max|want| over the row's frequencies (complex magnitudes for 'amplitude'); a NaN or an
           infinity where scipy has a number is an error of any size.
  bound    max(1e-12, 16 * spread), at most 1e-10 (asserted: an ill-conditioned fixture cannot widen it silently).
           spread is scipy's own rounding: scipy against its own formulas, statement by statement, evaluated in
           np.longdouble on the same float64 inputs (t, y, omega are the float64 values; everything after them -- the
           products omega t, the cosines, the sums, tau, the second pass -- is longdouble), relative to max|want|.

Where scipy's own spread leaves the ceiling, and fixtures therefore do not go: frequencies far below 1 / T with the
floating mean (6e-11 .. 6e-7), the Nyquist frequency of an integer grid in 'amplitude' mode (SS clamps, b is noise /
epsneg), rows of three valid samples with the floating mean (1e-8).  Accuracy fixtures stay on grids inside
[2 / T, 0.45 fs] with at least 37 valid samples; f = 0 and three-sample rows have cases of their own (check_row(...,
lift_ceiling=True)).
"""
from __future__ import annotations

import functools
import itertools
import os
import warnings

import numpy as np
from scipy.signal import lombscargle

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: no yardstick for scipy's rounding"

FLOOR, MARGIN, CEILING = 1e-12, 16.0, 1e-10
FS = 100.0
NORMALIZE = ("power", "normalize", "amplitude")
COMBOS = list(itertools.product((False, True), (False, True), NORMALIZE))      # (floating_mean, precenter, normalize)
LD = np.longdouble


def combo_id(combo):
    fm, pc, norm = combo
    return f"{'fm' if fm else 'nofm'}-{'pc' if pc else 'nopc'}-{norm}"


def valid_of(x, length=None):
    x = np.asarray(x, dtype=np.float64)
    v = ~np.isnan(x)
    if length is not None:
        v[int(length):] = False
    return v


def recipe(t, x, f, *, floating_mean=False, precenter=False, normalize="power", length=None):
    """scipy on the valid samples of one row; f in Hz (raises what scipy raises)."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    v = valid_of(x, length)
    omega = 2.0 * np.pi * np.asarray(f, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.atleast_1d(lombscargle(t[v], x[v].copy(), omega, precenter=precenter, normalize=normalize,
                                         floating_mean=floating_mean))


def _finish(K, Y, YY, C, S, YC, YS, CC, SS, tau, floating_mean, normalize, one, eps):
    """scipy's statements behind the second pass, in the type of the arguments."""
    if floating_mean:
        YC = YC - Y * C
        YS = YS - Y * S
        CC = CC - C * C
        SS = SS - S * S
    CC = np.where(CC < eps, eps, CC)
    SS = np.where(SS < eps, eps, SS)
    a = YC / CC
    b = YS / SS
    p = 2 * one * (a * YC + b * YS)
    if normalize == "power":
        return p * (one * K / 4)
    if normalize == "normalize":
        if floating_mean:
            YY = YY - Y * Y
        return p * (one / 2 / YY)
    return (a + 1j * b) * (np.cos(tau) + 1j * np.sin(tau))


def exact(t, x, f, *, floating_mean=False, precenter=False, normalize="power", length=None, block=8):
    """scipy's formulas in np.longdouble on the same float64 inputs, a block of frequencies at a time."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    v = valid_of(x, length)
    tl, yl = t[v].astype(LD)[:, None], x[v].astype(LD)[:, None]
    omega = (2.0 * np.pi * np.asarray(f, dtype=np.float64)).astype(LD)
    K = tl.shape[0]
    one = LD(1)
    w = one / LD(K)
    if precenter:
        yl = yl - yl.sum() * w
    Y = (yl * w).sum()
    YY = (yl * yl * w).sum()
    eps = LD(np.finfo(np.float64).epsneg)
    out = []
    for k0 in range(0, omega.shape[0], block):
        wt = omega[None, k0:k0 + block] * tl
        cw, sw = np.cos(wt), np.sin(wt)
        CC = (cw * cw).sum(axis=0) * w
        SS = one - CC
        CS = (cw * sw).sum(axis=0) * w
        if floating_mean:
            C, S = cw.sum(axis=0) * w, sw.sum(axis=0) * w
            CC, SS, CS = CC - C * C, SS - S * S, CS - C * S
        tau = np.arctan2(2 * CS, CC - SS) / 2
        wt = wt - tau[None, :]
        cw, sw = np.cos(wt), np.sin(wt)
        YC, YS = (yl * cw).sum(axis=0) * w, (yl * sw).sum(axis=0) * w
        CC = (cw * cw).sum(axis=0) * w
        SS = one - CC
        C, S = cw.sum(axis=0) * w, sw.sum(axis=0) * w
        out.append(_finish(LD(K), Y, YY, C, S, YC, YS, CC, SS, tau, floating_mean, normalize, one, eps))
    return np.concatenate(out)


def one_pass(t, x, f, *, floating_mean=False, precenter=False, normalize="power", length=None):
    """The kernel's algebra in float64 NumPy: one pass of sums over the valid samples (cos, sin, cos^2, cos sin, y cos,
    y sin; y, y^2 per row), the first and second moments rotated by tau in the epilogue.  Summation is by ``@`` -- not the
    device's tile order."""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    v = valid_of(x, length)
    tv, y = t[v], x[v].copy()
    omega = 2.0 * np.pi * np.asarray(f, dtype=np.float64)
    K = float(tv.shape[0])
    w = 1.0 / K
    if precenter:
        y = y - y.sum() / K
    wt = tv[:, None] * omega[None, :]
    cw, sw = np.cos(wt), np.sin(wt)
    m = np.ones_like(tv)
    C0, S0, CC0, CS0 = (m @ cw) * w, (m @ sw) * w, (m @ (cw * cw)) * w, (m @ (cw * sw)) * w
    YC0, YS0 = (y @ cw) * w, (y @ sw) * w
    Y, YY = y.sum() * w, (y @ y) * w
    SS0 = 1.0 - CC0
    cca, ssa, csa = CC0, SS0, CS0
    if floating_mean:
        cca, ssa, csa = CC0 - C0 * C0, SS0 - S0 * S0, CS0 - C0 * S0
    tau = 0.5 * np.arctan2(2.0 * csa, cca - ssa)
    c, s = np.cos(tau), np.sin(tau)
    YC, YS = YC0 * c + YS0 * s, YS0 * c - YC0 * s
    CC = (c * c) * CC0 + (2.0 * c * s) * CS0 + (s * s) * SS0
    SS = 1.0 - CC
    C, S = C0 * c + S0 * s, S0 * c - C0 * s
    return _finish(K, Y, YY, C, S, YC, YS, CC, SS, tau, floating_mean, normalize, 1.0, np.finfo(np.float64).epsneg)


def measure(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = np.isfinite(want)                        # (where scipy itself has no number, nothing is asked)
    if not ok.any():
        return 0.0
    d = np.abs(got - want).astype(np.float64)
    d[~np.isfinite(got)] = np.inf
    return float(d[ok].max() / np.abs(want[ok]).max())


def spread_of(want, ex):
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float(np.abs(ex - want.astype(ex.dtype))[ok].max() / np.abs(want[ok]).max())


def bound_of(sp, lift_ceiling=False):
    b = max(FLOOR, MARGIN * sp)
    assert lift_ceiling or b <= CEILING, f"bound {b:.3e} beyond {CEILING:g}: the fixture is too ill-conditioned to be a test"
    return b


def _kw(combo):
    fm, pc, norm = combo
    return dict(floating_mean=fm, precenter=pc, normalize=norm)


GOLDEN_LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lomb", "lomb_long.npz")


@functools.lru_cache(maxsize=None)
def _golden_long():
    """scipy's results and spreads of the "long" fixture for the twelve combinations, recorded: scipy takes 3 s a call
    on its 210 000 valid samples, the longdouble evaluation 8 s.  ``python tests/lomb_oracle.py`` writes the file into
    tests/golden/lomb/ (a folder of its own: the .npz files of tests/golden itself are the MFCC vectors);
    tests/test_lomb_host.py recomputes a part of it."""
    z = np.load(GOLDEN_LONG)
    assert z["combos"].tolist() == [combo_id(c) for c in COMBOS]
    return {c: (z["want"][i], float(z["spread"][i])) for i, c in enumerate(COMBOS)}


def compute_reference(name, combo, every=1):
    """(want, spread) from scratch; every: only each `every`-th frequency of the fixture's grid."""
    t, x, f = fixture(name)
    f = f[::every]
    want = recipe(t, x, f, **_kw(combo))
    return want, spread_of(want, exact(t, x, f, **_kw(combo)))


@functools.lru_cache(maxsize=None)
def reference(name, combo):
    """(want, spread, bound) of a named fixture: computed once, shared, never modified (the array is read-only)."""
    if name == "long":
        want, sp = _golden_long()[combo]
        want = want.copy() if combo[2] == "amplitude" else np.ascontiguousarray(want.real)
    else:
        want, sp = compute_reference(name, combo)
    want.setflags(write=False)
    return want, sp, bound_of(sp)


def check(got, name, combo, what=""):
    """Assert c <= bound for a named fixture; -> (c, bound, spread)."""
    want, sp, b = reference(name, combo)
    c = measure(got, want)
    print(f"lomb {what or name} {combo_id(combo)}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}")
    assert c <= b, f"{what or name} {combo_id(combo)}: c = {c:.3e} beyond the bound {b:.3e} (spread {sp:.3e})"
    return c, b, sp


def check_row(got, t, x, f, combo, what="row", length=None, lift_ceiling=False):
    """The same for a row that is no named fixture.  lift_ceiling: the bound stays 16 x spread but may pass 1e-10 -- only
    for the f = 0 and three-sample cases with the floating mean, where scipy's own spread does."""
    want = recipe(t, x, f, length=length, **_kw(combo))
    sp = spread_of(want, exact(t, x, f, length=length, **_kw(combo)))
    b = bound_of(sp, lift_ceiling)
    c = measure(got, want)
    print(f"lomb {what} {combo_id(combo)}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}")
    assert c <= b, f"{what} {combo_id(combo)}: c = {c:.3e} beyond the bound {b:.3e} (spread {sp:.3e})"
    return c, b, sp


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def _rng(*key):
    import zlib
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


def time_axis(n, fs=FS):
    return np.arange(n) / fs


def grid(n, fs=FS, count=160, top=None):
    """`count` frequencies from 2 / T to 0.45 fs (or `top` Hz), T = n / fs."""
    return np.linspace(2.0 / (n / fs), 0.45 * fs if top is None else top, count)


def f0_curve(n, key, fs=FS):
    """An f0-like curve in Hz: a slow declination, a 4 Hz and a 1.3 Hz modulation, jitter."""
    r = _rng("f0", key)
    t = time_axis(n, fs)
    return (150.0 - 2.0 * (t % 10.0) + 18.0 * np.sin(2 * np.pi * 4.0 * t + 0.4) + 9.0 * np.sin(2 * np.pi * 1.3 * t + 1.0)
            + 1.5 * r.standard_normal(n))


GAPS_12 = ((0, 9), (40, 31), (120, 25), (199, 30), (287, 18), (350, 33), (441, 12), (500, 41), (610, 22), (700, 27),
           (820, 19), (984, 17))                        # (start, count): twelve unvoiced stretches, 284 samples of 1001


def with_gaps(x, gaps):
    x = x.copy()
    for a, c in gaps:
        x[a:a + c] = np.nan
    return x


NAMES = ("f0-gaps", "f0-full", "scatter37", "long")
SHORT_NAMES = NAMES[:3]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(t, x, f in Hz) of a named fixture, read-only."""
    if name in ("f0-gaps", "f0-full"):
        n = 1001
        x = f0_curve(n, 1)
        if name == "f0-gaps":
            x = with_gaps(x, GAPS_12)
            assert int((~np.isnan(x)).sum()) == 717
        f = grid(n)
    elif name == "scatter37":
        n = 1001
        full = f0_curve(n, 2)
        x = np.full(n, np.nan)
        keep = np.sort(_rng("scatter").choice(n, size=37, replace=False))
        x[keep] = full[keep]
        f = grid(n)
    elif name == "long":
        n = 300001
        r = _rng("long-mask")
        f = grid(n, count=64, top=40.0)
        tt = time_axis(n)                  # an articulograph-like channel (mm): small mean, slow and syllabic movement, both
        # on frequencies of the grid -- between them max|want| is a side lobe and scipy's rounding of omega t (1e-10 rad at
        # t = 3000 s) a large part of it: the spread leaves the ceiling
        x = (4.0 + 8.0 * np.sin(2 * np.pi * f[5] * tt + 0.3) + 5.0 * np.sin(2 * np.pi * f[1] * tt + 2.0)
             + 0.5 * _rng("long").standard_normal(n))
        starts = r.integers(0, n - 400, size=300)
        for a, c in zip(starts, r.integers(40, 400, size=300)):
            x[a:a + c] = np.nan
        extra = np.flatnonzero(~np.isnan(x))
        drop = int(round(extra.size - 0.7 * n))
        assert drop > 0, "the stretches alone already leave fewer than 70 % valid"
        x[r.choice(extra, size=drop, replace=False)] = np.nan
        assert abs((~np.isnan(x)).sum() / n - 0.7) < 1e-3
    else:
        raise KeyError(name)
    t = time_axis(n)
    for a in (t, x, f):
        a.setflags(write=False)
    return t, x, f


if __name__ == "__main__":          # records tests/golden/lomb/lomb_long.npz (minutes)
    rows = [compute_reference("long", c) for c in COMBOS]
    for c, (w, sp) in zip(COMBOS, rows):
        print(combo_id(c), f"spread {sp:.3e}, bound {bound_of(sp):.3e}", flush=True)
    os.makedirs(os.path.dirname(GOLDEN_LONG), exist_ok=True)
    np.savez(GOLDEN_LONG, combos=np.array([combo_id(c) for c in COMBOS]), want=np.stack([w.astype(np.complex128) for w, _ in rows]),
             spread=np.array([sp for _, sp in rows]))
