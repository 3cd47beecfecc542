"""The yardstick of the modulation spectrum (row A8: the rFFT of every MFCC trajectory, zero-padded to n points): a float64
reference of the rows the device actually transformed, a per-bin error measure normalised per row, the same measure of an
independent float32 FFT (scipy's pocketfft) the kernels get a fixed margin over, and the fixed input rows.

    c[r, k] = |got[r, k] - X[r, k]| / (2^-24 (|X[r, k]| + log2(n) ||x_r||_2))

|X_k| pays for rounding the stored value, log2(n) ||x||_2 is the propagated-error term of a float32 FFT of n points (every
one of the log2 n passes adds a relative 2^-24 to values whose root-mean-square over the bins is ||x||_2).  Both terms are
the ROW's own: a quiet row beside a loud one is held to its own norm, a bin far below the row's DC bin to the row's norm and
not to the DC bin's magnitude.  A row of zeros must come back as exact zeros.

The bound of every test is  c.max() <= MARGIN * max(C_ref(n), 1)  with C_ref(n) the largest c scipy's float32 transform
reaches over the whole case set at that n: computed here, on the host, from the reference and never from the code under test.
MARGIN = 4 (two bits) covers another factorisation (radix-16 register passes), table twiddles and another FMA contraction.

Nothing in the package imports this module.

    rfft64(x, n)           np.fft.rfft of the float32 rows in float64
    dft_longdouble(x, n)   direct O(n^2) DFT in np.longdouble (confirms rfft64 for small n)
    bin_error(got, x, n)   c[r, k] above (inf where a zero row did not come back as zeros)
    ref_c(x, n)            bin_error of scipy.fft.rfft on the zero-padded float32 rows
    cases(n, T)            the fixed rows [16, T] float32;  take(x, rows, start) cycles through them
    c_ref(n), tolerance(n) C_ref(n) over cases(n, T) for T in edge_lengths(n), and MARGIN * max(C_ref(n), 1)
    check(got, x, n, what) asserts the bound per row, returns c.max()
"""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
MARGIN = 4.0
EPS = 2.0 ** -24
N_CASES = 16
# rows of cases(): a 1e-6-scaled noise row lies directly between a 1e3-scaled one and a mean-1e4 trajectory
ROW_LOUD, ROW_QUIET, ROW_MEAN1E4, ROW_ZERO = 4, 5, 6, 15


def rfft64(x, n):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-1] <= n, (x.dtype, x.shape, n)
    return np.fft.rfft(x.astype(np.float64), n=int(n), axis=-1)


def dft_longdouble(x, n):
    """X[r, k] = sum_t x[r, t] exp(-2 pi i k t / n), k = 0 .. n / 2: every term formed and summed in np.longdouble, the
    angle reduced exactly (k t mod n in integers) before it is scaled."""
    assert np.finfo(LD).eps < 1e-18, "dft_longdouble needs an extended-precision np.longdouble (eps < 1e-18)"
    x = np.atleast_2d(np.asarray(x)).astype(LD)
    T = x.shape[-1]
    k = np.arange(n // 2 + 1, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    ang = ((k * t) % n).astype(LD) * (2 * np.arctan2(LD(0), LD(-1)) / LD(n))       # 2 pi (k t mod n) / n
    re = x @ np.cos(ang).T
    im = -(x @ np.sin(ang).T)
    return re + 1j * im


def bin_error(got, x, n):
    x = np.asarray(x)
    X = rfft64(x, n)
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == X.shape, (got.shape, X.shape)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))
    den = EPS * (np.abs(X) + np.log2(n) * norm)
    err = np.abs(got - X)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, c)


def rfft32(x, n):
    """scipy's float32 transform of the zero-padded rows -> complex64."""
    from scipy import fft as sfft
    x = np.asarray(x)
    assert x.dtype == np.float32
    pad = np.zeros(x.shape[:-1] + (int(n),), dtype=np.float32)
    pad[..., :x.shape[-1]] = x
    out = sfft.rfft(pad, axis=-1)
    assert out.dtype == np.complex64
    return out


def ref_c(x, n):
    return bin_error(rfft32(x, n), x, n)


def cases(n, T, seed=0):
    """[16, T] float32.  Rows 0-2, 6: trajectory-like (mean + 4 Hz AM at a 100 Hz frame rate + noise, sigma ~ 1) with means
    0, 1, 100, 1e4; 3: a constant; 4, 5: noise scaled 1e3 and 1e-6; 7-10: unit impulses at 0, T // 3, T // 2, T - 1;
    11-14: cosines centred on bins 1, n / 4, n / 2 - 1, n / 2; 15: zeros."""
    n, T = int(n), int(T)
    assert 1 <= T <= n
    rng = np.random.default_rng([seed, n, T])
    t = np.arange(T, dtype=np.float64)

    def traj(mean):
        return mean + np.cos(2 * np.pi * 0.04 * t + rng.uniform(0, 2 * np.pi)) + 0.5 * rng.standard_normal(T)

    rows = [traj(0.0), traj(1.0), traj(100.0), np.full(T, 37.25),
            1e3 * rng.standard_normal(T), 1e-6 * rng.standard_normal(T), traj(1e4)]
    for pos in (0, T // 3, T // 2, T - 1):
        e = np.zeros(T)
        e[pos] = 1.0
        rows.append(e)
    for k in (1, n // 4, n // 2 - 1, n // 2):
        rows.append(np.cos(2 * np.pi * ((k * np.arange(T, dtype=np.int64)) % n) / n))
    rows.append(np.zeros(T))
    x = np.stack(rows).astype(np.float32)
    assert x.shape == (N_CASES, T)
    x.setflags(write=False)
    return x


def take(x, rows, start=ROW_LOUD):
    """`rows` rows of the case set, cycling from `start`: one row is the loud noise row, five end on two impulses with the
    quiet row between its loud neighbours, 37 go through the set twice and a bit."""
    return np.ascontiguousarray(x[(start + np.arange(int(rows))) % x.shape[0]])


def edge_lengths(n):
    return tuple(sorted(T for T in {1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n} if 1 <= T <= n))


@functools.lru_cache(maxsize=None)
def c_ref(n):
    return float(max(ref_c(cases(n, T), n).max() for T in edge_lengths(n)))


def tolerance(n, margin=None):
    return (MARGIN if margin is None else margin) * max(c_ref(int(n)), 1.0)


def check(got, x, n, what="", margin=None):
    """Asserts bin_error(got, x, n) <= tolerance(n) on every row; returns the largest c."""
    c = bin_error(got, x, n)
    tol = tolerance(n, margin)
    per_row = c.reshape(-1, c.shape[-1]).max(axis=-1)
    bad = np.flatnonzero(~(per_row <= tol))
    assert bad.size == 0, (f"{what}: n {n}: {bad.size} of {per_row.size} rows beyond c = {tol:.2f} "
                           f"(C_ref {c_ref(int(n)):.2f}); worst row {int(per_row.argmax())} c = {per_row.max():.2f}, "
                           f"first rows {bad[:8].tolist()}")
    return float(per_row.max())
