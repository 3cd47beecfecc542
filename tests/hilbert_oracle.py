"""The yardstick of the Hilbert envelope |scipy.signal.hilbert(x)| (csrc/mm_hilbert.hip.inc): a reference in the next higher
precision, a per-sample error measure normalised per row, the same measure of independent host envelopes in the clips' own
precision (the kernels get a fixed margin over them), the fixed input rows, and the rule that says which kernel instantiations
a call reaches.

    c[r, t] = |got[r, t] - want[r, t]| / (eps (|want[r, t]| + L sigma_r)),     L = 2 log2(n),  eps = 2^-24 | 2^-53

|want| pays for rounding the stored value (two clips per transform: see below).  L sigma_r is the propagated error of the two n-point transforms of an envelope:
each of the log2(n) radix-2 levels of a transform (wider radices do several levels at once) adds a relative eps to values
whose root-mean-square over the samples is sigma_r, and forward + inverse make 2 log2(n) levels.  sigma_r follows from the
algorithm:

    one clip per transform (a single row, the ragged call, scipy):        sigma_r = rms(x_r)
    two clips per transform (every other call of the batched envelope):   sigma_r = 2^e_r hypot(rms(a'), rms(b'))

with a' and b' the two clips of the pair after their exact scaling by a power of two into [0.5, 1) (max |x| = f 2^e) and
2^e_r row r's own scale back: the complex sequence a' + i b' is what is transformed, so both clips carry the rounding noise
of the pair's norm.  The partner of row r is row r ^ 1 of the same library call; a missing, all-zero or non-finite partner
contributes nothing (the kernel keeps it out of the pair).  A row of zeros must come back as exact zeros, a row with a NaN or
an infinity as NaN throughout -- and its partner within its bound.

The stored value of a pair.  With one clip per transform the value that is rounded last is the complex sample whose
magnitude is stored, hence |want|.  With two clips the transform ends on  zz[t] = (a'[t] - H(b')[t]) + i (H(a')[t] + b'[t])  and
the envelopes come from  H(a') = Im zz - b',  H(b') = a' - Re zz:  the rounding of zz[t] is relative to |zz[t]| <= |z_a'[t]| +
|z_b'[t]|, the sum of BOTH scaled envelopes at that sample, and the differences pass it on in full -- where clip a has an
impulse and clip b is silent, H(b') is the difference of two values of the impulse's size.  So for a row r with partner p

    c[r, t] = |got - want| / (eps (|want_r[t]| + 2^(e_r - e_p) |want_p[t]| + L sigma_r))

(the partner's reference envelope brought to row r's scale; nothing is added for a row without a partner).  Found on the
device: the unit impulse at n / 2 beside the one at n / 3, float64, n = 131072, was 6 eps off at t = n / 3 -- three units in
the last place of the 0.5 that a'[t] and Re zz[t] both hold there -- which the first form of the measure read as c = 45 against
C_ref = 7.5; scipy's own float32 pair shows the same sample (c = 15 in the first form).

The bound of every row:  c[r].max() <= MARGIN * max(C_ref[r], 1),  MARGIN = modspec_oracle.MARGIN (two bits: another
factorisation, table twiddles, another FMA contraction).  C_ref[r] is the same measure of a HOST envelope in the clip's own
precision on that very case row -- computed here from scipy's same-precision FFT, never from the code under test:

    direct lengths, one clip        |scipy.signal.hilbert(x)|               (complex64 for float32 clips)
    direct lengths, two clips       the pair a' + i b' through scipy.fft in the clips' precision
    chirp lengths, ragged call      bluestein_analytic below: the chirp identity X[k] = w[k] sum_j (x[j] w[j]) conj(w[k - j]),
                                    w[k] = exp(-i pi k^2 / n), as a circular convolution of length M = 2^p >= 2 n - 1; chirp in
                                    float64, rounded once; transforms of length M by scipy in the clips' precision

Nothing in the package imports this module.

    envelope_hi(x)                  the reference: float64 for float32 clips, np.longdouble for float64 clips
    envelope_dft(x)                 the same from a direct O(n^2) long-double DFT (confirms envelope_hi for small n)
    spectrum_mask(n)                1 at bin 0 (and n / 2 for even n), 2 below n / 2, 0 above
    rows_for(n, dtype)              the case rows [16 | 18, n];  take(x, rows) cycles through them (modspec_oracle.take)
    pair_scale(x), sigma(x, paired) the power-of-two scales and sigma_r
    errors(got, want, sig, n, dt)   c[r, t]
    reference(n, dtype)             cached: rows, want, C_ref per form ("single", "paired")
    check(got, x, idx, ...)         asserts the bound per row, returns (largest c, its C_ref, its bound)
    passes(n), features(...)        the pass plan and the kernel instantiations of one call
    ENVELOPE_LENGTHS, FORWARD_LENGTHS, BLUESTEIN_LENGTHS, RAGGED_M      what the GPU tests run (test_hilbert_host.py asserts
                                    that they reach every feature any length up to LIMIT reaches)
"""
from __future__ import annotations

import functools

import numpy as np

import modspec_oracle as MO

LD = np.longdouble
MARGIN = MO.MARGIN
EPS = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
ROW_LOUD, ROW_QUIET, ROW_MEAN1E4, ROW_ZERO = MO.ROW_LOUD, MO.ROW_QUIET, MO.ROW_MEAN1E4, MO.ROW_ZERO
ROW_1E30, ROW_1EM30 = 16, 17                      # float32 only
LIMIT = 200000                                    # the coverage condition looks at every smooth length up to here


def _hi(dtype):
    return np.float64 if np.dtype(dtype) == np.float32 else LD


def _ctype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def spectrum_mask(n):
    """scipy.signal.hilbert's weights, written out: 1 at bin 0 and at n / 2 for even n, 2 below n / 2, 0 above."""
    n = int(n)
    h = np.zeros(n)
    h[0] = 1.0
    if n % 2 == 0:
        h[n // 2] = 1.0
        h[1:n // 2] = 2.0
    else:
        h[1:(n + 1) // 2] = 2.0
    return h


def envelope_hi(x):
    """|hilbert(x)| along the last axis in the next higher precision (scipy.fft keeps long double: complex256 here)."""
    from scipy import fft as sfft
    assert np.finfo(LD).eps < 1e-18, "envelope_hi needs an extended-precision np.longdouble (eps < 1e-18)"
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    hi = _hi(x.dtype)
    X = sfft.fft(x.astype(hi), axis=-1)
    assert X.dtype == (np.complex128 if hi is np.float64 else np.clongdouble), X.dtype
    z = sfft.ifft(X * spectrum_mask(x.shape[-1]).astype(hi), axis=-1)
    assert z.dtype == X.dtype
    return np.abs(z)


def envelope_dft(x):
    """The same envelope from a direct O(n^2) DFT and inverse DFT in np.longdouble, the angles reduced in integers."""
    assert np.finfo(LD).eps < 1e-18, "envelope_dft needs an extended-precision np.longdouble (eps < 1e-18)"
    x = np.atleast_2d(np.asarray(x)).astype(LD)
    n = x.shape[-1]
    k = np.arange(n, dtype=np.int64)
    ang = ((k[:, None] * k[None, :]) % n).astype(LD) * (2 * np.arctan2(LD(0), LD(-1)) / LD(n))
    C, S = np.cos(ang), np.sin(ang)
    h = spectrum_mask(n).astype(LD)
    Xr, Xi = (x @ C) * h, -(x @ S) * h                   # X[k] = sum x[t] exp(-i ang)
    zr, zi = (Xr @ C - Xi @ S) / LD(n), (Xr @ S + Xi @ C) / LD(n)
    return np.sqrt(zr * zr + zi * zi)


# ---- the case rows ----

def rows_for(n, dtype):
    """The fixed rows of an envelope of n samples: modspec_oracle.cases(n_even, n) -- trajectories, a constant, noise at 1e3 and
    1e-6 side by side, impulses, cosines on bins 1, n / 4, n / 2 - 1, n / 2, zeros -- and for float32 noise at 1e30 and 1e-30.
    n < 4: explicit rows in the same places."""
    n = int(n)
    dtype = np.dtype(dtype)
    if n < 4:
        base = np.array([1.0, -2.0, 0.75])[:n]
        alt = np.array([1.0, -1.0, 1.0])[:n]
        first = np.array([1.0, 0.0, 0.0])[:n]
        last = np.array([0.0, 0.0, 1.0])[3 - n:]
        rows = [base, base + 1, 100 + base, np.full(n, 37.25), 1e3 * base[::-1], 1e-6 * base, 1e4 + base,
                first, last, first, last, alt, 3 * alt, -base, 0.5 * alt + 0.25, np.zeros(n)]
        x = np.stack(rows)
    else:
        x = MO.cases(n + (n & 1), n).astype(np.float64)
    assert x.shape == (MO.N_CASES, n)
    if dtype == np.float32:
        rng = np.random.default_rng([7, n])
        noise = rng.standard_normal((2, n))
        x = np.concatenate([x, noise * np.array([[1e30], [1e-30]])])
    x = x.astype(dtype)
    x.setflags(write=False)
    return x


def take_index(count, n_rows, start=ROW_LOUD):
    return (start + np.arange(int(count))) % int(n_rows)


def take(x, count, start=ROW_LOUD):
    """(rows, their case indices): `count` rows of the case set cycling from the loud noise row, as modspec_oracle.take."""
    idx = take_index(count, x.shape[0], start)
    got = MO.take(x, count, start)
    assert np.array_equal(got, x[idx])
    return got, idx


# ---- the measure ----

def pair_scale(x):
    """(down, up, kind) per row as hb_rowscale_kernel documents them: max |x| = f 2^e, f in [0.5, 1) -> 2^-e, 2^e; a row of
    zeros: up 0; a row with a NaN or an infinity: down 0, up NaN.  kind: 0 finite, 1 zero, 2 non-finite."""
    x = np.asarray(x)
    lo = -100 if x.dtype == np.float32 else -900
    down = np.ones(x.shape[0])
    up = np.ones(x.shape[0])
    kind = np.zeros(x.shape[0], dtype=np.int64)
    for r in range(x.shape[0]):
        if not np.isfinite(x[r]).all():
            down[r], up[r], kind[r] = 0.0, np.nan, 2
            continue
        m = float(np.abs(x[r]).max())
        if m == 0:
            up[r], kind[r] = 0.0, 1
            continue
        e = max(int(np.frexp(m)[1]), lo)
        down[r], up[r] = np.ldexp(1.0, -e), np.ldexp(1.0, e)
    return down, up, kind


def _rms(v):
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt((v * v).mean(axis=-1))


def sigma(x, paired):
    """sigma_r of every row of one library call (float64)."""
    x = np.asarray(x)
    if not paired:
        with np.errstate(invalid="ignore", over="ignore"):
            return _rms(x)
    down, up, kind = pair_scale(x)
    out = np.zeros(x.shape[0])
    for r in range(x.shape[0]):
        if kind[r] != 0:
            out[r] = 0.0 if kind[r] == 1 else np.nan
            continue
        own = _rms(x[r].astype(np.float64) * down[r])
        p = r ^ 1
        other = _rms(x[p].astype(np.float64) * down[p]) if p < x.shape[0] and kind[p] == 0 else 0.0
        out[r] = up[r] * np.hypot(own, other)
    return out


def stored(x, want, paired):
    """The magnitude whose rounding the stored value pays for, per sample: |want| where a clip has a transform to itself; in a
    pair the magnitude of the pair's complex sample at row r's scale, at most |want_r| + 2^(e_r - e_p) |want_p| (see the head of
    this file).  `want`: the reference envelopes of the rows of the call."""
    out = np.abs(want)
    if not paired:
        return out
    out = out.copy()
    down, up, kind = pair_scale(x)
    for r in range(x.shape[0]):
        p = r ^ 1
        if kind[r] == 0 and p < x.shape[0] and kind[p] == 0:
            out[r] += out.dtype.type(up[r] * down[p]) * np.abs(want[p])
    return out


def errors(got, want, sig, n, dtype, stored_scale=None):
    """c[r, t]; inf where the denominator is zero and the error is not, and wherever `got` is not finite.  `stored_scale`:
    stored(x, want, paired), |want| if left out."""
    hi = _hi(dtype)
    got = np.asarray(got)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    L = 2.0 * np.log2(n) if n > 1 else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(hi) - want.astype(hi))
        first = np.abs(want) if stored_scale is None else stored_scale
        den = hi(EPS[np.dtype(dtype)]) * (first.astype(hi) + hi(L) * np.asarray(sig, dtype=hi)[:, None])
        ok = den > 0
        c = np.where(ok, err / np.where(ok, den, 1), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(c), c, np.inf).astype(np.float64)


# ---- host envelopes in the clips' own precision ----

def scipy_fft(ctype):
    from scipy import fft as sfft

    def fft(a):
        out = sfft.fft(np.ascontiguousarray(a, dtype=ctype), axis=-1)
        assert out.dtype == ctype, out.dtype
        return out
    return fft


def direct_analytic(z, fft, mask=None):
    """x + i H(x) of the complex rows z by an n-point transform `fft` in z's precision; the inverse is
    conj(fft(conj(.))) / n."""
    n = z.shape[-1]
    rt = z.real.dtype
    h = (spectrum_mask(n) if mask is None else mask).astype(rt)
    return np.conj(fft(np.conj(fft(z) * h))) / rt.type(n)


@functools.lru_cache(maxsize=4)
def chirp(n, M):
    """(w [n], b [M]) in float64: w[k] = exp(-i pi k^2 / n) with k^2 reduced mod 2 n in integers, b the wrapped conjugate."""
    k = np.arange(n, dtype=np.int64)
    ang = np.pi * ((k * k) % (2 * n)).astype(np.float64) / n
    w = np.cos(ang) - 1j * np.sin(ang)
    b = np.zeros(M, dtype=np.complex128)
    b[:n] = np.conj(w)
    b[M - n + 1:] = np.conj(w[1:][::-1])
    return w, b


@functools.lru_cache(maxsize=4)
def _chirp_spectrum(n, M):
    return np.fft.fft(chirp(n, M)[1])


def chirp_fft_size(n):
    return max(16, 1 << max(2 * int(n) - 2, 0).bit_length())


def bluestein_analytic(z, fft, M, mask=None, chirp_dtype=None, bhat_in_precision=False):
    """direct_analytic through the chirp identity: every n-point transform as a circular convolution of length M with the
    chirp, the M-point transforms by `fft`.  The chirp is computed in float64 and rounded once (through `chirp_dtype` first, if
    given: a mutant); its spectrum in float64 and rounded once, or (`bhat_in_precision`, the ragged call) by `fft` itself."""
    n = z.shape[-1]
    ct, rt = z.dtype, z.real.dtype
    assert M >= 2 * n - 1
    w64, b64 = chirp(n, M)
    if chirp_dtype is not None:
        w64, b64 = w64.astype(chirp_dtype).astype(np.complex128), b64.astype(chirp_dtype).astype(np.complex128)
    w = w64.astype(ct)
    bhat = fft(b64.astype(ct)) if bhat_in_precision or chirp_dtype is not None else _chirp_spectrum(n, M).astype(ct)
    h = (spectrum_mask(n) if mask is None else mask).astype(rt)

    def dft(v):
        a = np.zeros(v.shape[:-1] + (M,), dtype=ct)
        a[..., :n] = v * w
        conv = np.conj(fft(np.conj(fft(a) * bhat))) / rt.type(M)
        return conv[..., :n] * w
    return np.conj(dft(np.conj(dft(z) * h))) / rt.type(n)


def single_envelope(x, analytic):
    """|analytic(x)| of real rows, one clip per transform."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(analytic(x.astype(_ctype(x.dtype)))).astype(x.dtype)


def paired_envelope(x, analytic, scaled=True):
    """The envelopes of the rows of one call, two clips per transform as the kernel header describes it: rows 2 p and 2 p + 1
    scaled by their powers of two, a' + i b' transformed, H(a) = Im - b', H(b) = a' - Re.  `scaled=False`: a mutant."""
    x = np.asarray(x)
    rt = x.dtype
    down, up, kind = pair_scale(x)
    if not scaled:
        down, up = np.where(kind == 0, 1.0, down), np.where(kind == 0, 1.0, up)
    rows = x.shape[0]
    xs = np.where((kind == 0)[:, None], x, 0).astype(rt) * down.astype(rt)[:, None]
    if rows % 2:
        xs = np.concatenate([xs, np.zeros((1, x.shape[1]), dtype=rt)])
    a, b = xs[0::2], xs[1::2]
    zz = analytic((a + 1j * b).astype(_ctype(rt)))
    ha, hb = zz.imag - b, a - zz.real
    env = np.empty_like(xs)
    env[0::2] = np.sqrt(a * a + ha * ha)
    env[1::2] = np.sqrt(b * b + hb * hb)
    with np.errstate(invalid="ignore"):
        return (env[:rows] * up.astype(rt)[:, None]).astype(rt)


def host_analytic(n, dtype, ragged_M=None):
    """The transform the host envelopes of length n are built on: scipy's, directly or through the chirp identity."""
    fft = scipy_fft(_ctype(dtype))
    if ragged_M is not None:
        return lambda z: bluestein_analytic(z, fft, ragged_M, bhat_in_precision=True)
    plan = passes(n)
    if plan["bluestein"]:
        return lambda z: bluestein_analytic(z, fft, plan["M"])
    return lambda z: direct_analytic(z, fft)


# ---- the reference of a length, cached ----

class Reference:
    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.plan = passes(self.n)
        self.rows = rows_for(self.n, self.dtype)
        self.want = envelope_hi(self.rows)
        self._c_ref = {}

    def c_ref(self, form):
        """C_ref per case row.  "single": one clip per transform.  "paired": the larger of the row beside its neighbour
        (row r ^ 1 of the case set, which is what take() puts beside it) and the row without a partner."""
        if form in self._c_ref:
            return self._c_ref[form]
        x, n, dt = self.rows, self.n, self.dtype
        if n == 1:
            c = np.zeros(x.shape[0])
        elif form == "single":
            if self.plan["bluestein"]:
                env = single_envelope(x, host_analytic(n, dt))
            else:
                from scipy.signal import hilbert
                z = hilbert(x, axis=-1)
                assert z.dtype == _ctype(dt), z.dtype
                env = np.abs(z).astype(dt)
            c = errors(env, self.want, sigma(x, False), n, dt).max(-1)
        else:
            assert form == "paired"
            an = host_analytic(n, dt)
            c = errors(paired_envelope(x, an), self.want, sigma(x, True), n, dt, stored(x, self.want, True)).max(-1)
            alone = np.zeros((2 * x.shape[0], n), dtype=dt)      # every row without a partner (a row of zeros is kept out)
            alone[0::2] = x
            c = np.maximum(c, errors(paired_envelope(alone, an)[0::2], self.want, sigma(alone, True)[0::2], n, dt).max(-1))
        c.setflags(write=False)
        self._c_ref[form] = c
        return c


@functools.lru_cache(maxsize=4)
def _reference(n, dtype):
    return Reference(n, dtype)


def reference(n, dtype):
    return _reference(int(n), np.dtype(dtype))


def bound(c_ref):
    return MARGIN * np.maximum(c_ref, 1.0)


def check(got, x, idx, n, dtype, paired, what="", margin=None):
    """The rows `x` of ONE library call (case rows `idx`; -1: a row that holds a NaN or an infinity) and what the call
    returned: every finite row within its bound, every zero row exact zeros, every non-finite row NaN throughout.
    Returns (c, C_ref, bound) of the row that comes closest to its bound."""
    ref = reference(n, dtype)
    x, got, idx = np.asarray(x), np.asarray(got), np.asarray(idx)
    assert got.shape == x.shape and got.dtype == ref.dtype, (got.shape, x.shape, got.dtype)
    form = "paired" if paired else "single"
    finite = np.isfinite(x).all(-1)
    assert (finite == (idx >= 0)).all()
    assert np.array_equal(x[finite], ref.rows[idx[finite]])
    if paired:                       # C_ref was computed for the partner take() gives, or none
        down, up, kind = pair_scale(x)
        for r in np.flatnonzero(finite):
            p = r ^ 1
            assert p >= x.shape[0] or kind[p] != 0 or idx[p] == (idx[r] ^ 1), (what, r, idx[r], idx[p])
    for r in np.flatnonzero(~finite):
        assert np.isnan(got[r]).all(), f"{what}: row {r} holds a NaN or an infinity and did not come back as NaN throughout"
    fin = np.flatnonzero(finite)
    if fin.size == 0:
        return 0.0, 0.0, float(bound(0.0))
    want = ref.want[idx[fin]]
    sig = sigma(x, paired)[fin]
    want_all = np.zeros(x.shape, dtype=ref.want.dtype)
    want_all[fin] = want
    c = errors(got[fin], want, sig, n, dtype, stored(x, want_all, paired)[fin]).max(-1)
    zero = ~x[fin].any(-1)
    assert (got[fin][zero] == 0).all(), f"{what}: a row of zeros did not come back as exact zeros"
    cr = ref.c_ref(form)[idx[fin]]
    assert np.isfinite(cr).all(), f"{what}: no host yardstick for case rows {idx[fin][~np.isfinite(cr)].tolist()} as {form}"
    tol = (MARGIN if margin is None else margin) * np.maximum(cr, 1.0)
    bad = np.flatnonzero(~(c <= tol))
    worst = int(np.argmax(c / tol))
    assert bad.size == 0, (f"{what}: n {n} {ref.dtype} {form}: {bad.size} of {fin.size} rows beyond their bound; worst: call row "
                           f"{int(fin[worst])} (case row {int(idx[fin[worst]])}) c = {c[worst]:.2f} > {tol[worst]:.2f} "
                           f"(C_ref {cr[worst]:.2f}); rows {fin[bad][:8].tolist()} c {np.round(c[bad][:8], 2).tolist()}")
    return float(c[worst]), float(cr[worst]), float(tol[worst])


def check_clip(got, x, M, what="", margin=None):
    """One clip of the ragged call (its valid samples `x`, what came back for them, the call's transform length M): the
    single-clip sigma, C_ref from the chirp identity at M with the chirp spectrum taken in the clip's precision."""
    x, got = np.asarray(x), np.asarray(got)
    n, dt = x.shape[-1], x.dtype
    x2, got2 = x[None, :], got[None, :]
    want = envelope_hi(x2)
    sig = sigma(x2, False)
    c = float(errors(got2, want, sig, n, dt).max())
    if not x.any():
        assert (got == 0).all(), f"{what}: a clip of zeros did not come back as exact zeros"
    if n == 1:
        cr = 0.0
    else:
        cr = float(errors(single_envelope(x2, host_analytic(n, dt, ragged_M=M)), want, sig, n, dt).max())
    tol = (MARGIN if margin is None else margin) * max(cr, 1.0)
    assert c <= tol, f"{what}: n {n} {dt} M {M}: c = {c:.2f} > {tol:.2f} (C_ref {cr:.2f})"
    return c, cr, tol


# ---- the plan rule ----

def _smooth_counts(n):
    cnt = []
    for p in (2, 3, 5, 7):
        k = 0
        while n % p == 0:
            n //= p
            k += 1
        cnt.append(k)
    return cnt, n


def _radices(cnt):
    """hb_set_passes: fused radix-16 pairs (256), radix 16, the rest of the twos; per odd prime the fused radix-25 pair (625),
    squares, the prime."""
    cnt = list(cnt)
    out = []
    while cnt[0] >= 8:
        out.append(256)
        cnt[0] -= 8
    while cnt[0] >= 4:
        out.append(16)
        cnt[0] -= 4
    if cnt[0]:
        out.append(1 << cnt[0])
    for i, p in ((1, 3), (2, 5), (3, 7)):
        if p == 5:
            while cnt[i] >= 4:
                out.append(625)
                cnt[i] -= 4
        while cnt[i] >= 2:
            out.append(p * p)
            cnt[i] -= 2
        if cnt[i]:
            out.append(p)
    return out


def passes(n, ragged=False):
    """mm_hilbert_create / mm_hilbert_ragged_create: {"bluestein", "M", "radix"} of a clip length (ragged: of the longest clip)."""
    n = int(n)
    cnt, rest = _smooth_counts(n)
    bluestein = ragged or rest != 1
    M = n
    if bluestein:
        M = chirp_fft_size(n)
        cnt = [M.bit_length() - 1, 0, 0, 0]
    return {"bluestein": bluestein, "M": M, "radix": _radices(cnt)}


def _fuse_c(R, dtype):
    return (32 if R == 256 else 10) // (2 if np.dtype(dtype) == np.float64 else 1)


def _pass_feature(R, M, Ns, dtype, in_mode, out_mode, paired, rg, mid=False):
    fused = R in (256, 625)
    if mid:
        kernel = "mid2" if fused else "mid"
        pos = "Ns1" if M // R == 1 else "twiddled"
    else:
        kernel = "pass2" if fused else "pass"
        if Ns == 1:
            pos = "Ns1"
        elif not fused and R <= 16 and Ns <= 128 and 128 % Ns == 0:
            pos = "lds"
        else:
            pos = "strided"
    if fused:
        C = _fuse_c(R, dtype)
        partial = (M // R) % C != 0
    else:
        partial = (M // R) % 128 != 0
    # two clips per transform shows only where clips are read or the envelope is stored
    shows = in_mode in ("real", "real_chirp") or out_mode == "envelope"
    return (kernel, R, pos, "partial" if partial else "full", in_mode, out_mode, ("paired" if paired else "single") if shows else "-",
            np.dtype(dtype).name, "ragged" if rg else "dense")


def _fft_features(radix, M, dtype, in_mode, out_mode, paired, rg):
    out, Ns = [], 1
    for i, R in enumerate(radix):
        out.append(_pass_feature(R, M, Ns, dtype, in_mode if i == 0 else "complex",
                                 out_mode if i + 1 == len(radix) else "complex", paired, rg))
        Ns *= R
    return out


def features(n, rows, call, dtype=np.float32):
    """The kernel instantiations one call reaches, as a set of (kernel, radix, position, last workgroup, in-mode, out-mode,
    pairing, dtype, dense | ragged).  call: "envelope" (mm_hilbert_envelope of `rows` clips of n samples), "rfft"
    (mm_hilbert_rfft_f32 at n points) or "ragged" (mm_hilbert_envelope_ragged, n the longest clip)."""
    n, rows = int(n), int(rows)
    if call == "ragged":
        plan = passes(n, ragged=True)
        M, radix = plan["M"], plan["radix"]
        out = _fft_features(radix, M, dtype, "complex", "complex", False, True)      # the chirps' spectra (dense kernels)
        out = [f[:8] + ("dense",) for f in out]
        for im, om in (("real_chirp", "mul_conj"), ("complex", "bluestein_mid"), ("complex", "mul_conj"), ("complex", "envelope")):
            out += _fft_features(radix, M, dtype, im, om, False, True)
        return set(out)
    plan = passes(n)
    M, radix = plan["M"], plan["radix"]
    if call == "rfft":
        assert not plan["bluestein"] and n % 2 == 0 and np.dtype(dtype) == np.float32
        return set(_fft_features(radix, M, dtype, "real", "half", False, False))
    assert call == "envelope"
    paired = rows > 1 and len(radix) > 0
    if not radix:
        return {("abs", 1, "-", "-", "real", "envelope", "single", np.dtype(dtype).name, "dense")}
    out = []
    if plan["bluestein"]:
        for im, om in (("real_chirp", "mul_conj"), ("complex", "bluestein_mid"), ("complex", "mul_conj"), ("complex", "envelope")):
            out += _fft_features(radix, M, dtype, im, om, paired, False)
        return set(out)
    P, Ns = len(radix), 1
    for i in range(P - 1):
        out.append(_pass_feature(radix[i], M, Ns, dtype, "real" if i == 0 else "complex", "complex", paired, False))
        Ns *= radix[i]
    out.append(_pass_feature(radix[P - 1], M, Ns, dtype, "real" if P == 1 else "complex", "envelope" if P == 1 else "complex",
                             paired, False, mid=True))
    Ns = radix[P - 1]
    for i in range(P - 2, -1, -1):
        out.append(_pass_feature(radix[i], M, Ns, dtype, "complex", "envelope" if i == 0 else "complex", paired, False))
        Ns *= radix[i]
    return set(out)


def smooth_lengths(limit=LIMIT):
    out = []
    a = 1
    while a <= limit:
        b = a
        while b <= limit:
            c = b
            while c <= limit:
                d = c
                while d <= limit:
                    out.append(d)
                    d *= 7
                c *= 5
            b *= 3
        a *= 2
    return sorted(out)


def bluestein_length(M, smallest):
    """A length that is not 2-3-5-7-smooth and goes through chirp transforms of length M: the smallest above M / 4 or the
    largest with 2 n - 1 <= M."""
    n = M // 4 + 1 if smallest else M // 2
    while True:
        if _smooth_counts(n)[1] != 1:
            assert chirp_fft_size(n) == M, (n, M)
            return n
        n += 1 if smallest else -1


ENVELOPE_ROWS = (1, 2, 5, 37)
# greedy covers over smooth_lengths() (tools of this file: test_hilbert_host.greedy_cover), recomputed with features() above
ENVELOPE_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 24, 25, 32, 35, 49, 64, 81, 125, 128, 256, 343, 625, 750, 1024, 2048, 3072, 3125,
                    4096, 4375, 6250, 8192, 8750, 9600, 18432, 30240, 31360, 40000, 43904, 46875, 48020, 53760, 65536, 131072,
                    144000)
FORWARD_LENGTHS = (2, 4, 8, 14, 16, 18, 32, 54, 64, 96, 128, 162, 256, 320, 384, 640, 896, 1024, 1152, 1250, 1500, 2048, 4096, 8750,
                   9600, 13824, 16000, 17010, 18432, 31250, 31360, 43904, 65536, 81920, 96040, 120960, 131072)
BLUESTEIN_LENGTHS = tuple(bluestein_length(1 << p, smallest=(p % 2 == 1)) for p in range(5, 20))
LONG_CASES = (441000, bluestein_length(1 << 19, smallest=False))      # passes 8 9 25 5 49, and another length at M = 2^19
RAGGED_M = tuple(1 << p for p in (4, 5, 6, 7, 8, 10, 11, 12, 13, 16, 17))
