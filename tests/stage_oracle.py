"""The yardstick of the STFT power and log-mel stages (rows A1-A5: centre pad, frame, pre-emphasis, window, rFFT, |.|^2, mel,
10 log10): a float64 reference built from the oracle's own pieces, a per-bin and a per-filter error measure normalised by the
FRAME's own norm, the same measures of a float32 host pipeline (scipy's pocketfft) the kernels get a fixed margin over, and the
fixed case clips.  Host only; nothing in the package imports this module.  MARGIN and EPS are modspec_oracle's.

Reference, for one float32 clip y and a configuration (a dict of MfccConfig / OracleConfig keywords):

    f[t, :] = float64(O.frame_signal(y, n_fft, hop, preemph)) * O.hann_window_padded(win_length, n_fft)
    X = np.fft.rfft(f)            ||f_t|| the 2-norm of frame t           W = float64(O.mel_filterbank(...))

Per-frame floor -- |X| pays for rounding the stored value, log2(n_fft) ||f_t|| is the propagated error of a float32 FFT, as in
modspec_oracle; both are the FRAME's own, so a quiet frame beside a loud one, or a bin 50 dB under the frame's peak, is held
to that frame and not to the clip's maximum:

    e[t, k] = 2^-24 (|X[t, k]| + log2(n_fft) ||f_t||)

Power, measured in AMPLITUDE (in power the ratio is squared at the bins that lie under the floor, and an honest float32
pipeline then spreads over two decades):

    c_A[t, k] = | sqrt(P_got[t, k]) - |X[t, k]| | / e[t, k]

A frame of zeros must come back as exact zeros (c = inf otherwise); a NaN or a negative power is c = inf.

Log-mel -- the floor carried through the mel sum and the logarithm:

    mel = |X|^2 @ W.T        d_P = e (2 |X| + e)        d_mel = d_P @ W.T + 2^-24 mel
    fl = max(mel, amin)      L = 10 log10(fl)           d_L = (10 / ln 10) d_mel / fl + 2 * 2^-24 |L|
    c_L[t, m] = | lm_got[m, t] - L[t, m] | / d_L[t, m]

The second term of d_L is the float32 storage of a dB value plus one unit in the last place of the logarithm; empty filters
and silent frames sit on the amin floor and are held to that term alone.

The bound of every test is  c.max() <= MARGIN * max(C_ref, 1), per measure, with C_ref the largest c the float32 host pipeline
(float32 frame x float32 window, scipy.fft.rfft in float32, re^2 + im^2, float32 einsum with W, float32 10 log10(max(amin, .)))
reaches over the whole case set of the configuration, every length of lengths(cfg) included: computed here, on the host, cached
per configuration, never from the code under test.

    cases(n, cfg)                  the fixed clips [14, n] float32 (rows below)
    lengths(cfg)                   the clip lengths of a configuration: one frame, a partial tile, 63 / 64 / 65 / 66 frames
    aligned_lengths(cfg)           the same rounded up to multiples of 4 (extra cases for kernels with an alignment gate)
    reference(cfg, n)              Ref(A, e, L, dL) of cases(n, cfg), cached;  reference_of(y, cfg) for other clips
    host_pipeline(y, cfg, ...)     the float32 pipeline -> (P [B, T, bins], lm [B, n_mels, T]); window / W / frames replaceable
    power_error(P, ref)            c_A [B, T, bins];   logmel_error(lm, ref)   c_L [B, T, n_mels]
    c_ref(cfg), bounds(cfg)        (C_A, C_L) of the host pipeline and MARGIN * max(., 1) of each
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import mfcc_oracle as O
from modspec_oracle import EPS, MARGIN

N_CASES = 14
# rows of cases(): the 1e-6-scaled noise lies between the 1e3-scaled one and the first tone; the impulse at n - 1 lies
# directly before the one at 0 (a pre-emphasis carry across rows lands on a sample that is 1 and must stay 1)
ROW_AM, ROW_LOUD, ROW_QUIET, ROW_TONE0, ROW_IMP_LAST, ROW_IMP_FIRST, ROW_STEP, ROW_CONST, ROW_ZERO = 0, 1, 2, 3, 7, 8, 11, 12, 13

Ref = namedtuple("Ref", "A e L dL")      # |X| and its floor [B, T, bins]; log-mel and its floor [B, T, n_mels]


def key(cfg):
    return tuple(sorted(cfg.items()))


def tone_bins(n_fft):
    return (1, n_fft // 4, n_fft // 2 - 1, n_fft // 8 + 3)


def impulse_positions(n):
    return (n - 1, 0, min(1, n - 1), n // 3)


def cases(n, cfg, seed=0):
    """[14, n] float32.  0: O.synth_clip(1, n, sr, 'am'); 1, 2: noise scaled 1e3 and 1e-6; 3-6: cosines exactly on bins 1,
    n_fft / 4, n_fft / 2 - 1, n_fft / 8 + 3 of the frame (phase reduced as (k t) mod n_fft); 7-10: unit impulses at n - 1, 0,
    min(1, n - 1), n / 3 (every frame holding one has P[k] = w[i]^2 at every k); 11: noise, first half x 1e3, second half
    x 1e-4; 12: the constant 0.75; 13: zeros."""
    n, n_fft = int(n), int(cfg["n_fft"])
    rng = np.random.default_rng([seed, n, n_fft])
    rows = [O.synth_clip(1, n, cfg["sr"], "am").astype(np.float64),
            1e3 * rng.standard_normal(n), 1e-6 * rng.standard_normal(n)]
    t = np.arange(n, dtype=np.int64)
    for k in tone_bins(n_fft):
        rows.append(np.cos(2 * np.pi * ((k * t) % n_fft) / n_fft))
    for pos in impulse_positions(n):
        imp = np.zeros(n)
        imp[pos] = 1.0
        rows.append(imp)
    step = rng.standard_normal(n)
    step[:n // 2] *= 1e3
    step[n // 2:] *= 1e-4
    rows += [step, np.full(n, 0.75), np.zeros(n)]
    x = np.stack(rows).astype(np.float32)
    assert x.shape == (N_CASES, n)
    x.setflags(write=False)
    return x


def lengths(cfg):
    """n_fft <= 2048: one frame (1, 3), a partial tile (n_fft / 2 + 1), 63 / 64 / 65 / 66 frames; beyond: three short ones."""
    n_fft, hop = int(cfg["n_fft"]), int(cfg["hop_length"])
    if n_fft <= 2048:
        return tuple(sorted({1, 3, n_fft // 2 + 1, 63 * hop - 1, 63 * hop, 64 * hop, 65 * hop + 7}))
    return tuple(sorted({1, n_fft // 2 + 1, 8 * hop + 7}))


def aligned_lengths(cfg):
    """lengths(cfg) from 3 on, rounded up to a multiple of 4: what a kernel with an alignment gate (rows at 16 bytes, n % 4 == 0)
    accepts.  They are extra cases held to the bound of lengths(cfg); C_ref is not taken over them."""
    return tuple(sorted({(n + 3) & ~3 for n in lengths(cfg) if n >= 3} - set(lengths(cfg))))


def window64(cfg):
    return O.hann_window_padded(int(cfg["win_length"]), int(cfg["n_fft"]))


def mel_weights(cfg):
    """O.mel_filterbank: float32 values [n_mels, bins]."""
    return O.mel_filterbank(cfg["sr"], int(cfg["n_fft"]), int(cfg["n_mels"]), cfg["fmin"], cfg["fmax"])


def frames_of(y, cfg):
    """[B, T, n_fft] float32: O.frame_signal of every row of y (pre-emphasis in float32, zero centre padding)."""
    y = np.atleast_2d(np.asarray(y))
    assert y.dtype == np.float32
    return np.stack([O.frame_signal(r, int(cfg["n_fft"]), int(cfg["hop_length"]), cfg.get("preemph", 0.0)) for r in y])


def reference_of(y, cfg):
    n_fft = int(cfg["n_fft"])
    amin = float(cfg.get("amin", 1e-10))
    f = frames_of(y, cfg).astype(np.float64) * window64(cfg)
    A = np.abs(np.fft.rfft(f, axis=-1))
    e = EPS * (A + np.log2(n_fft) * np.sqrt((f ** 2).sum(-1, keepdims=True)))
    W = mel_weights(cfg).astype(np.float64)
    mel = (A * A) @ W.T
    d_mel = (e * (2 * A + e)) @ W.T + EPS * mel
    fl = np.maximum(mel, amin)
    L = 10.0 * np.log10(fl)
    dL = (10.0 / np.log(10.0)) * d_mel / fl + 2 * EPS * np.abs(L)
    return Ref(A, e, L, dL)


@functools.lru_cache(maxsize=16)      # a test touches one configuration, at most 13 lengths
def _reference(k, n):
    return reference_of(cases(n, dict(k)), dict(k))


def reference(cfg, n):
    return _reference(key(cfg), int(n))


def _ratio(err, den):
    """err / den; where the floor is 0 (a frame of zeros) the value must be exact; NaN counts as inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, c)


def power_error(P, ref):
    P = np.asarray(P).astype(np.float64)
    assert P.shape == ref.A.shape, (P.shape, ref.A.shape)
    with np.errstate(invalid="ignore"):
        return _ratio(np.abs(np.sqrt(P) - ref.A), ref.e)


def logmel_error(lm, ref):
    """lm as the plan returns it: [B, n_mels, T]."""
    lm = np.swapaxes(np.asarray(lm).astype(np.float64), -1, -2)
    assert lm.shape == ref.L.shape, (lm.shape, ref.L.shape)
    return _ratio(np.abs(lm - ref.L), ref.dL)


def host_power(fr, win):
    """float32 frames [B, T, n_fft] x float32 window -> scipy.fft.rfft (float32) -> re^2 + im^2, float32."""
    from scipy import fft as sfft
    x = (fr.astype(np.float32) * win.astype(np.float32)).astype(np.float32)
    S = sfft.rfft(x, axis=-1)
    assert S.dtype == np.complex64
    return (S.real * S.real + S.imag * S.imag).astype(np.float32)


def host_logmel(P, W, amin=1e-10):
    """float32 einsum with W, float32 10 log10(max(amin, .)) -> [B, n_mels, T]."""
    mel = np.einsum("btf,mf->bmt", P.astype(np.float32), W.astype(np.float32), optimize=True).astype(np.float32)
    return (np.float32(10.0) * np.log10(np.maximum(np.float32(amin), mel))).astype(np.float32)


def host_pipeline(y, cfg, window=None, W=None, frames=None):
    """(P [B, T, bins], lm [B, n_mels, T]) of the float32 host pipeline; the mutants of test_stage_host replace a piece."""
    fr = frames_of(y, cfg) if frames is None else frames
    P = host_power(fr, window64(cfg) if window is None else window)
    return P, host_logmel(P, mel_weights(cfg) if W is None else W, cfg.get("amin", 1e-10))


@functools.lru_cache(maxsize=16)
def _host(k, n):
    return host_pipeline(cases(n, dict(k)), dict(k))


def host(cfg, n):
    """host_pipeline of cases(n, cfg), cached."""
    return _host(key(cfg), int(n))


@functools.lru_cache(maxsize=None)
def _c_ref(k):
    cfg = dict(k)
    cA = cL = 0.0
    for n in lengths(cfg):
        P, lm = host(cfg, n)
        ref = reference(cfg, n)
        cA = max(cA, float(power_error(P, ref).max()))
        cL = max(cL, float(logmel_error(lm, ref).max()))
    return cA, cL


def c_ref(cfg):
    """(C_A, C_L): the largest c_A and c_L of the float32 host pipeline over cases(n, cfg), n in lengths(cfg)."""
    return _c_ref(key(cfg))


def bounds(cfg, margin=None):
    m = MARGIN if margin is None else margin
    cA, cL = c_ref(cfg)
    return m * max(cA, 1.0), m * max(cL, 1.0)
