"""The yardstick of the spline gap filling (interp_nan_spline_batch, mm_interp_spline_f64): the reference's recipe restated
with scipy, the measure and its bound, and the fixtures of tests/test_spline_host.py and tests/test_gpu_spline.py.

  want     script/calc.py:379 restated: interp1d(valid indices, valid values, kind, fill_value="extrapolate") at the NaN
           indices, the valid samples kept.
  c        max|got - want| / max|want| over the row.
  bound    max(1e-12, 16 * spread), at most 1e-10 (asserted: an ill-conditioned input cannot widen it silently).
           1e-12 is the bound of this kernel family (linear and pchip in tests/test_gpu_interp.py).  spread is scipy's own
           rounding: scipy's result against the same collocation system (BSpline.design_matrix on scipy's knot vector)
           solved by np.linalg.solve with iterative refinement in np.longdouble and evaluated in np.longdouble (the design
           matrix of the query points times the refined coefficients), relative to max|want|.  The margin 16: a NumPy
           emulation of two unpivoted float64 forms of the same interpolants stood at most 4.8 x spread from scipy (the
           five-knot fixture: spread 2.95e-13, condition 1.8e5, the moment form at 1.42e-12); 16 leaves a factor of three.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg
from scipy.interpolate import BSpline, interp1d, make_interp_spline

assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: no yardstick for scipy's rounding"

METHODS = ("quadratic", "cubic")
DEGREE = {"quadratic": 2, "cubic": 3}
FLOOR, MARGIN, CEILING = 1e-12, 16.0, 1e-10
S = 1024                    # interp.INTERP_SEGMENT = interp.SPLINE_CHUNK


def recipe(x, method):
    """The reference's interp_NAN for one curve and one of the two methods (raises what scipy raises)."""
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    nans = np.isnan(x)
    if nans.sum() == 0:
        return out
    f = interp1d(np.where(~nans)[0], x[~nans], method, fill_value="extrapolate")
    out[nans] = f(np.where(nans)[0])
    return out


def spread(x, method):
    """scipy's own rounding on this row, relative to max|want|."""
    x = np.asarray(x, dtype=np.float64)
    k = DEGREE[method]
    valid = ~np.isnan(x)
    xi, yi, tq = np.where(valid)[0].astype(np.float64), x[valid], np.where(~valid)[0].astype(np.float64)
    want = recipe(x, method)
    t = make_interp_spline(xi, yi, k=k).t
    A = BSpline.design_matrix(xi, t, k).toarray()
    Al, yl = A.astype(np.longdouble), yi.astype(np.longdouble)
    lu = scipy.linalg.lu_factor(A)                # np.linalg.solve's factorisation, made once for the refinement
    c = scipy.linalg.lu_solve(lu, yi).astype(np.longdouble)
    for _ in range(4):
        c = c + scipy.linalg.lu_solve(lu, (yl - Al @ c).astype(np.float64)).astype(np.longdouble)
    assert float(np.abs(yl - Al @ c).max()) <= 1e-17 * float((np.abs(Al) @ np.abs(c)).max()), "refinement did not converge"
    Q = BSpline.design_matrix(tq, t, k, extrapolate=True).toarray().astype(np.longdouble)
    exact = Q @ c
    return float(np.abs(exact - want[~valid].astype(np.longdouble)).max() / np.abs(want).max())


def measure(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    d[~np.isfinite(got)] = np.inf                 # a NaN or an infinity where scipy has a number is an error of any size
    return float(d.max() / np.abs(want).max())


def bound_of(sp):
    b = max(FLOOR, MARGIN * sp)
    assert b <= CEILING, f"bound {b:.3e} beyond {CEILING:g}: the fixture is too ill-conditioned to be a test"
    return b


@functools.lru_cache(maxsize=None)
def reference(name, method):
    """(want, spread, bound) of a named fixture: computed once, shared, never modified (the array is read-only)."""
    x = fixture(name)
    want = recipe(x, method)
    want.setflags(write=False)
    sp = spread(x, method)
    return want, sp, bound_of(sp)


def check(got, name, method, what=""):
    """Assert c <= bound for a named fixture; -> (c, bound, spread)."""
    want, sp, b = reference(name, method)
    c = measure(got, want)
    print(f"spline {what or name} {method}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}")
    assert c <= b, f"{what or name} {method}: c = {c:.3e} beyond the bound {b:.3e} (spread {sp:.3e})"
    return c, b, sp


def check_row(got, x, method, what="row"):
    """The same for a row that is no named fixture."""
    want = recipe(x, method)
    sp = spread(x, method)
    b = bound_of(sp)
    c = measure(got, want)
    print(f"spline {what} {method}: c = {c:.3e}, bound = {b:.3e}, spread = {sp:.3e}")
    assert c <= b, f"{what} {method}: c = {c:.3e} beyond the bound {b:.3e} (spread {sp:.3e})"
    return c, b, sp


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def _rng(*key):
    import zlib
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


def curve(n, key):
    """An f0-like curve: 110 .. 215 Hz, slow movement plus jitter."""
    r = _rng("curve", key)
    t = np.arange(n)
    return 160.0 + 45.0 * np.sin(t / 37.0 + r.uniform(0, 6)) + 8.0 * np.sin(t / 5.3) + r.standard_normal(n)


def ends(x, lead, tail):
    x = x.copy()
    if lead:
        x[:lead] = np.nan
    if tail:
        x[len(x) - tail:] = np.nan
    return x


def f0_like(n, key=0, lead=0, tail=0):
    """Voiced runs of 1-80 samples, gaps of 1-60 (a tenth of both in a row of fewer than 200 samples); the first, the
    last and samples 8 .. 12 are valid: lead / tail alone decide the ends, and no row is too sparse for a cubic."""
    r = _rng("f0", n, key)
    c = curve(n, ("f0", key))
    x = c.copy()
    run_hi, gap_hi = (81, 61) if n >= 200 else (9, 7)
    i = 0
    while i < n:
        i += int(r.integers(1, run_hi))
        g = int(r.integers(1, gap_hi))
        x[i:i + g] = np.nan
        i += g
    x[0], x[n - 1] = c[0], c[n - 1]
    x[8:13] = c[8:13]                             # five valid samples behind any lead
    assert np.isnan(x).any()
    return ends(x, lead, tail)


def spaced(n, steps, key=0):
    """Valid samples at the running sum of `steps`, repeated; NaN between them."""
    c = curve(n, ("spaced", steps, key))
    x = np.full(n, np.nan)
    p, k = 0, 0
    while p < n:
        x[p] = c[p]
        p += steps[k % len(steps)]
        k += 1
    return x


def chosen(n, K, key=0):
    """Exactly K valid samples, scattered over n."""
    r = _rng("chosen", n, K, key)
    c = curve(n, ("chosen", K, key))
    x = np.full(n, np.nan)
    idx = np.sort(r.choice(n, size=K, replace=False))
    x[idx] = c[idx]
    return x


def knots(K, key=0):
    """A row with exactly K valid samples: every ninth sample of the rest is a NaN, the row begins and ends with one."""
    n = K + K // 8 + 2
    x = np.full(n, np.nan)
    keep = np.ones(n, dtype=bool)
    keep[0] = keep[n - 1] = False
    keep[np.arange(K // 8) * 9 + 4] = False
    assert keep.sum() == K, (K, keep.sum())
    x[keep] = curve(n, ("knots", K, key))[keep]
    return x


def _five():
    x = np.full(1001, np.nan)
    x[[3, 500, 501, 502, 990]] = [1.0, 2.0, -1.0, 5.0, 3.0]
    return x


def _scatter30(n=1001):
    x = curve(n, "scatter30")
    x[_rng("scatter30").choice(n, size=30, replace=False)] = np.nan
    return x


def _every_second(n=1001):
    x = curve(n, "second")
    x[1::2] = np.nan
    return x


def _swallow():
    x = f0_like(3 * S + 5, key=5)
    x[S - 10:2 * S + 10] = np.nan
    return x


def _single():
    x = curve(1001, "single")
    x[417] = np.nan
    return x


LENGTHS = (40, S - 1, S, S + 1, 2 * S + 77, 3 * S + 5)
ENDS = ((0, 0), (1, 0), (0, 7), (7, 1))        # leading / trailing NaN runs of 0, 1 and 7 samples
# the chunks hold S unknowns, two fewer than knots: S + 2 knots are the last single chunk, 2 S + 2 the last pair
KNOT_COUNTS = (S - 1, S, S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2, 2 * S + 3)

_FIXTURES = {
    "five-knot": _five,
    "scatter30": _scatter30,
    "every-second": _every_second,
    "sparse40": lambda: chosen(1001, 40),
    "alt-1-59": lambda: spaced(1001, (1, 59)),
    "alt-1-1-1-97": lambda: spaced(1001, (1, 1, 1, 97)),
    "swallow": _swallow,
    "single-nan": _single,
    "three-chunks": lambda: knots(2 * S + 300, key=3),
    "four-knots": lambda: chosen(700, 4, key=4),
}
for _n in LENGTHS:
    for _l, _t in ENDS + ((7, 7), (1, 7), (0, 1)):
        _FIXTURES[f"f0-{_n}-{_l}-{_t}"] = functools.partial(f0_like, _n, 0, _l, _t)
for _k in KNOT_COUNTS:
    _FIXTURES[f"knots-{_k}"] = functools.partial(knots, _k)
for _m in METHODS:
    for _d in (1, 2):
        _FIXTURES[f"few-{_m}-{_d}"] = functools.partial(chosen, 1001, DEGREE[_m] + _d, ("few", _m))

# what the GPU tests measure and docs/experiments.md lists (the f0 rows: one per length, and the end runs at 1001-like S - 1)
MEASURED = (["five-knot", "scatter30", "every-second", "sparse40", "alt-1-59", "alt-1-1-1-97", "swallow", "single-nan",
             "three-chunks"] + [f"knots-{k}" for k in KNOT_COUNTS])


@functools.lru_cache(maxsize=None)
def _fixture(name):
    x = _FIXTURES[name]()
    x.setflags(write=False)
    return x


def fixture(name):
    return _fixture(name)


def few_names(method):
    return [f"few-{method}-1", f"few-{method}-2"]
