"""The yardstick of the Welch cross spectrum and coherence (modulation_cross_spectra_batch; include/modmfcc_modcsd.h), built
on tests/modpsd_oracle.py: its Params, segments, trend, row_norm, EPS, MARGIN and fixed rows.

Reference: scipy.signal.csd and scipy.signal.coherence in float64 on the float32 rows with the float32-rounded window.

Pairs (pairs_for): the 16 fixed rows of rows_for(p, T), each with itself, with the next row, with a copy of itself delayed
by 3 samples and with the zero row: 64 pairs.

Pxy is compared on the unscaled cross amplitude, A = Pxy_ref / (s d_k) and G = got / (s d_k) -- the mean over the pair's
segments of conj(X_k) Y_k.  With Ax, Ay the root-mean-square over the segments of |X_k|, |Y_k| (from scipy.signal.welch in
float64) and Nx, Ny the row norms of modpsd_oracle.row_norm:

    c[r, k] = |G - A| / (2^-24 (Ax Ay + log2(nfft) (Ax Ny + Ay Nx)))

the float32-FFT error of a mean of products: a transform error dX_i of size 2^-24 log2(nfft) Nx meets Y_i, and by
Cauchy-Schwarz |mean conj(dX_i) Y_i| <= rms |dX| rms |Y|; Ax Ay pays for rounding the stored value.  Where the denominator is
0 only an exact 0 is right (c = inf otherwise).

The bound is  c.max() <= MARGIN * max(C_ref, 1),  C_ref the largest c of an independent float32 pipeline on the same pairs
with the same parameters (spectra32: the detrended, windowed float32 segments through scipy.fft.rfft in complex64, products
and mean in float64).  It is computed here, on the host, never from the code under test.  Pxx and Pyy go through
modpsd_oracle.check as it stands.

That measure is first order in 2^-24, and a cross spectrum has bins where the first order vanishes: where BOTH sides have no
true amplitude (bin 0 after a detrend; the bins beside a cosine that sits on a bin; the bins of an impulse under a zero of
the taper) the float32 transforms still hold their rounding noise dX_i, dY_i, and conj(dX_i) dY_i does not average to nothing
when y is x itself.  There the reference pipeline reaches c = 60 .. 2.5e7 on five of the fifteen parameter sets below and inf
on one (Ax = Ay = 0 exactly at bin 0: boxcar, constant detrend), so that MARGIN * C_ref binds nothing on those sets.  Every
check is therefore made TWICE, and both must hold:

    cross_error   the measure above, as it stands, with its own C_ref (vacuous where C_ref is inf);
    cross_error2  the same with the second-order term in the denominator,
                      2^-24 (Ax Ay + L (Ax Ny + Ay Nx) + MARGIN 2^-24 L^2 Nx Ny),   L = log2(nfft),
                  |mean conj(dX_i) dY_i| <= rms |dX| rms |dY| by the same Cauchy-Schwarz step.  The factor MARGIN in it:
                  modpsd_oracle.check admits a transform whose noise in an empty bin is MARGIN 2^-24 L N (c = MARGIN at
                  A = 0); two such transforms give MARGIN^2 (2^-24 L)^2 Nx Ny, which is c2 = MARGIN here, the bound at
                  C_ref <= 1.  Without the factor a transform that passes on both sides could fail in the product.  Its
                  C_ref stays below 8 on every set (tests/test_modcsd_host.py asserts that, and that it is finite on every
                  pair and bin).

The added term is MARGIN 2^-24 L Nx Ny / (Ax Ny + Ay Nx) of the first-order one: below 1e-4 wherever either side has a
thousandth of its row norm in the bin, so the second check asks what the first asks wherever the first asks anything.

Coherence against scipy is measured as the plain difference |C - C_ref64| on pairs that carry power in every bin
(coherence_pairs: white noise plus a shared white component, delayed on one side), bounded by MARGIN x the largest
difference of the same float32 pipeline, its coherence rounded to the float32 the device returns.

_GPU_SETS (gpu_set(i)) is the list of parameter sets tests/test_gpu_modcsd.py runs against this yardstick; tests/test_modcsd_host.py
walks the same list on the host, so that no pair and no bin of it can be excluded unseen.

Nothing in the package imports this module.
"""
from __future__ import annotations

import numpy as np

import modpsd_oracle as P
from modpsd_oracle import EPS, MARGIN, Params, row_norm, rows_for, segments, trend  # noqa: F401

FS = 200.0
KINDS = ("self", "next", "delayed", "zero")
DELAY = 3


def length_for(nperseg, noverlap, K):
    """A row length with exactly K segments, half a step beyond the last one."""
    step = nperseg - noverlap
    return nperseg + (K - 1) * step + (step - 1) // 2


def _set(nperseg, nfft, noverlap, K, detrend, scaling, window):
    noverlap = nperseg // 2 if noverlap is None else noverlap
    w = np.kaiser(nperseg, 7.4) if window == "array" else window
    p = Params(FS, w, nperseg, noverlap, nfft, detrend, scaling)
    T = length_for(nperseg, noverlap, K)
    assert p.num_segments(T) == K
    return p, T


# (nperseg, nfft, noverlap (None: the default nperseg // 2), segments per row, detrend, scaling, window)
_GPU_SETS = [
    (32, 32, None, 1, "constant", "density", "hann"),          # fewer points than lanes
    (32, 32, 31, 33, "linear", "spectrum", "hann"),            # hop 1; two chunks
    (31, 32, 0, 5, False, "density", "array"),                 # odd, zero-padded
    (64, 64, None, 65, "constant", "density", "hann"),         # as many points as lanes; three chunks
    (64, 64, 63, 4, "linear", "density", "boxcar"),            # hop 1; one segment per wave
    (64, 64, 0, 32, False, "spectrum", "hann"),                # a full chunk
    (128, 128, None, 33, "linear", "spectrum", "array"),
    (128, 128, 0, 1, "constant", "density", "hann"),
    (255, 256, None, 5, "constant", "density", "hann"),        # the wave remainder
    (1024, 1024, None, 4, "linear", "density", "hann"),
    (1024, 1024, 0, 33, "constant", "spectrum", "boxcar"),
    (1200, 2048, None, 5, "constant", "density", "array"),
    (2048, 2048, None, 1, False, "density", "hann"),
    (2048, 2048, 0, 4, "linear", "spectrum", "hann"),
    (2048, 2048, None, 33, "constant", "density", "hann"),     # the finish kernel at 1025 bins
]
GPU_SET_IDS = [f"{s[0]}in{s[1]}-nov{s[2]}-K{s[3]}-{s[4]}-{s[5]}-{s[6]}" for s in _GPU_SETS]


def gpu_set(i):
    """(Params, T) of entry i of the list."""
    return _set(*_GPU_SETS[i])


N_GPU_SETS = len(_GPU_SETS)
# the sets on which white noise has power in every bin: all but a detrend under a boxcar window, which leaves bin 0 with none
COH_SETS = [i for i, s in enumerate(_GPU_SETS) if not (s[6] == "boxcar" and s[4])]


# ---- the pairs ----------------------------------------------------------------------------------------------------------
def delayed(x, d=DELAY):
    y = np.zeros_like(x)
    y[..., d:] = x[..., :x.shape[-1] - d]
    return y


_PAIRS = {}


def pairs_for(p, T):
    """(x [64, T], y [64, T]) float32, read-only: rows_for(p, T) four times, against KINDS."""
    k = (max(p.nfft, int(T)), int(T))
    if k not in _PAIRS:
        r = rows_for(p, T)
        x = np.concatenate([r, r, r, r])
        y = np.concatenate([r, np.roll(r, -1, axis=0), delayed(r), np.zeros_like(r)])
        x.setflags(write=False)
        y.setflags(write=False)
        _PAIRS[k] = (x, y)
    return _PAIRS[k]


def coherence_pairs(T, pairs=16, seed=7):
    """(x, y) float32 [pairs, T]: independent white noise on either side plus a shared white component of weight
    0.1 .. 3, delayed by the pair's index on the y side: every bin carries power on both sides, the coherence runs from
    near 0 to near 1."""
    g = np.random.default_rng([seed, int(T)])
    shared = g.standard_normal((pairs, T + pairs))
    wgt = np.geomspace(0.1, 3.0, pairs)[:, None]
    x = g.standard_normal((pairs, T)) + wgt * shared[:, pairs:]
    y = g.standard_normal((pairs, T)) + wgt * np.stack([shared[i, pairs - i:pairs - i + T] for i in range(pairs)])
    return x.astype(np.float32), y.astype(np.float32)


# ---- the references -------------------------------------------------------------------------------------------------------
def _kw(p):
    return dict(fs=p.fs, window=p.w, nperseg=p.nperseg, noverlap=p.noverlap, nfft=p.nfft, detrend=p.detrend, axis=-1)


def csd64(x, y, p):
    """(f, Pxy complex128): scipy.signal.csd in float64 on the float32 rows."""
    from scipy.signal import csd
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == y.shape and x.shape[-1] >= p.nperseg
    return csd(x.astype(np.float64), y.astype(np.float64), return_onesided=True, scaling=p.scaling, average="mean", **_kw(p))


def coherence64(x, y, p):
    """(f, Cxy float64): scipy.signal.coherence in float64 on the float32 rows; NaN where scipy divides 0 by 0."""
    from scipy.signal import coherence
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == y.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        return coherence(x.astype(np.float64), y.astype(np.float64), **_kw(p))


def _transform32(x, p):
    from scipy import fft as sfft
    seg = segments(x, p)
    v = (seg - trend(seg, p)).astype(np.float32) * p.w
    assert v.dtype == np.float32
    X = sfft.rfft(v, n=p.nfft, axis=-1)
    assert X.dtype == np.complex64
    return X.astype(np.complex128)              # exact


def spectra32(x, y, p):
    """The independent float32 pipeline -> (Pxx, Pyy, Pxy, Cxy): float64 detrend rounded to float32, the float32 window,
    scipy.fft.rfft in complex64, products and the mean over segments in float64; Pxx, Pyy, Pxy scaled, in float64; Cxy
    from the unscaled means, rounded to float32 (the type the device returns)."""
    X, Y = _transform32(x, p), _transform32(y, p)
    sxx, syy, sxy = (np.abs(X) ** 2).mean(axis=1), (np.abs(Y) ** 2).mean(axis=1), (np.conj(X) * Y).mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        coh = (np.abs(sxy) ** 2 / (sxx * syy)).astype(np.float32)
    f = p.s * p.d
    return sxx * f, syy * f, sxy * f, coh


# ---- the measure of Pxy -----------------------------------------------------------------------------------------------------
def denominators(x, y, p):
    """The denominators of c and c2 [pairs, bins]."""
    sd = p.s * p.d
    Ax, Ay = np.sqrt(P.welch64(x, p)[1] / sd), np.sqrt(P.welch64(y, p)[1] / sd)
    Nx, Ny = row_norm(x, p), row_norm(y, p)
    L = np.log2(p.nfft)
    first = EPS * (Ax * Ay + L * (Ax * Ny + Ay * Nx))
    return first, first + MARGIN * EPS * EPS * L * L * Nx * Ny


def cross_errors(got, x, y, p):
    """(c, c2) [pairs, bins] each (the module text); inf where an exact 0 was due and did not come, or where a value is
    NaN."""
    x, y = np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y))
    got = np.asarray(got, dtype=np.complex128).reshape(x.shape[0], p.bins)
    sd = p.s * p.d
    err = np.abs(got / sd - csd64(x, y, p)[1] / sd)
    out = []
    for den in denominators(x, y, p):
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
        out.append(np.where(np.isnan(err), np.inf, c))
    return tuple(out)


def cross_error(got, x, y, p):
    return cross_errors(got, x, y, p)[0]


def cross_error2(got, x, y, p):
    return cross_errors(got, x, y, p)[1]


_C_REF = {}


def c_ref(p, T, second_order=False):
    """The largest c (c2) of the independent float32 pipeline on pairs_for(p, T) (kept per parameter set and T)."""
    k = (p.key(), int(T))
    if k not in _C_REF:
        x, y = pairs_for(p, T)
        _C_REF[k] = tuple(float(c.max()) for c in cross_errors(spectra32(x, y, p)[2], x, y, p))
    return _C_REF[k][1 if second_order else 0]


def tolerance(p, T, second_order=False, margin=None):
    return (MARGIN if margin is None else margin) * max(c_ref(p, T, second_order), 1.0)


def check_pxy(got, x, y, p, what="", margin=None, measures=(False, True)):
    """Asserts cross_error <= tolerance and cross_error2 <= its tolerance on every pair (pairs of pairs_for(p, T), in any
    selection; ``measures``: (False,) the first alone, (True,) the second alone); returns the largest c of each."""
    x, y = np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(y))
    worst = []
    cs = cross_errors(got, x, y, p)
    for second in measures:
        c = cs[1 if second else 0]
        tol = tolerance(p, x.shape[-1], bool(second), margin)
        per_row = c.max(axis=-1)
        bad = np.flatnonzero(~(per_row <= tol))
        assert bad.size == 0, (f"{what}: Pxy ({'second' if second else 'first'}-order measure), nperseg {p.nperseg} nfft {p.nfft} "
                               f"noverlap {p.noverlap} detrend {p.detrend} {p.scaling} T {x.shape[-1]}: {bad.size} of "
                               f"{per_row.size} pairs beyond c = {tol:.2f} (C_ref {c_ref(p, x.shape[-1], bool(second)):.2f}); "
                               f"worst pair {int(per_row.argmax())} c = {per_row.max():.2f}, first pairs {bad[:8].tolist()}")
        worst.append(float(per_row.max()))
    return tuple(worst)


# ---- the measure of the coherence against scipy ------------------------------------------------------------------------------
def coherence_error(got, x, y, p):
    """|got - scipy.signal.coherence| [pairs, bins]; inf where either is NaN (coherence_pairs have no such bin)."""
    ref = coherence64(x, y, p)[1]
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref)
    return np.where(np.isnan(err), np.inf, err)


def coherence_ref_error(x, y, p):
    """The largest coherence_error of the float32 pipeline on these pairs."""
    return float(coherence_error(spectra32(x, y, p)[3], x, y, p).max())
