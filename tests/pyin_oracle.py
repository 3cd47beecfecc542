"""NumPy / scipy restatement of librosa 0.10's ``pyin`` (core/pitch.py, sequence.py) and of the reference's
``get_f0(method='pyin')`` / ``interp_NAN`` (script/calc.py:345-592) -- the test oracle of the pitch path.

librosa is not a dependency of this project; this module restates its arithmetic step by step ("Pitch"),
including the dtype flow of numpy < 2 (float64 FFT, input-dtype energy terms).  Nothing in the package imports it.

    pyin_dense      steps 1-8 with librosa's dense (2 n_bins)^2 Viterbi
    viterbi_banded  the banded decode of the device kernel (in-band sources + one out-of-band candidate)
    get_f0          the reference's get_f0 / interp_NAN with scipy's own interpolators and filters
"""
from __future__ import annotations

import math

import numpy as np
import scipy.signal
import scipy.stats
from scipy import interpolate

TINY = np.finfo(np.float64).tiny


# ---------------------------------------------------------------------------------------------------------------------
# sizes and tables
# ---------------------------------------------------------------------------------------------------------------------
def sizes(n, sr, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, resolution=0.1,
          max_transition_rate=35.92, center=True):
    if win_length is None:
        win_length = frame_length // 2
    if hop_length is None:
        hop_length = frame_length // 4
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)
    nbps = int(np.ceil(1.0 / resolution))
    n_bins = int(np.floor(12 * nbps * np.log2(fmax / fmin))) + 1
    width = round(max_transition_rate * 12 * hop_length / sr) * nbps + 1
    n_pad = n + (2 * (frame_length // 2) if center else 0)
    n_frames = 1 + (n_pad - frame_length) // hop_length
    return dict(win_length=win_length, hop_length=hop_length, min_period=min_period, max_period=max_period,
                nbps=nbps, n_bins=n_bins, width=width, n_frames=n_frames)


def beta_probs(n_thresholds=100, beta_parameters=(2, 18)):
    thresholds = np.linspace(0, 1, n_thresholds + 1)
    beta_cdf = scipy.stats.beta.cdf(thresholds, beta_parameters[0], beta_parameters[1])
    return thresholds, np.diff(beta_cdf)


def transition_local(n_states, width):
    """librosa.sequence.transition_local(n_states, width, window='triangle', wrap=False), literally."""
    transition = np.zeros((n_states, n_states), dtype=np.float64)
    for i in range(n_states):
        w = scipy.signal.get_window("triangle", width, fftbins=False)
        lpad = (n_states - width) // 2
        if lpad < 0:
            raise ValueError(f"target size ({n_states}) must be at least input size ({width})")
        trans_row = np.pad(w, (lpad, n_states - width - lpad), mode="constant")
        trans_row = np.roll(trans_row, n_states // 2 + i + 1)
        trans_row[min(n_states, i + width // 2 + 1):] = 0
        trans_row[:max(0, i - width // 2)] = 0
        transition[i] = trans_row
    transition /= transition.sum(axis=1, keepdims=True)
    return transition


def transition_full(n_bins, width, switch_prob):
    """np.kron(transition_loop(2, 1 - switch_prob), transition_local(...))."""
    p = 1 - switch_prob
    t_switch = np.empty((2, 2))
    t_switch[:] = (1 - p) / 1
    t_switch[0, 0] = p
    t_switch[1, 1] = p
    return np.kron(t_switch, transition_local(n_bins, width))


# ---------------------------------------------------------------------------------------------------------------------
# steps 1-6
# ---------------------------------------------------------------------------------------------------------------------
def frames(y, frame_length, hop_length, center=True, pad_mode="constant"):
    if center:
        y = np.pad(y, (frame_length // 2, frame_length // 2), mode=pad_mode)
    n_frames = 1 + (len(y) - frame_length) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n_frames)[:, None]
    return y[idx]                                           # [n_frames, frame_length], input dtype


def cmnd(y_frames, frame_length, win_length, min_period, max_period):
    """_cumulative_mean_normalized_difference on [n_frames, frame_length] frames -> [n_frames, P] float64."""
    yf = y_frames.astype(np.float64)                        # numpy < 2: the FFT is float64 for any input
    a = np.fft.rfft(yf, frame_length, axis=-1)
    b = np.fft.rfft(yf[:, win_length:0:-1], frame_length, axis=-1)
    acf = np.fft.irfft(a * b, frame_length, axis=-1)[:, win_length:]
    acf[np.abs(acf) < 1e-6] = 0
    energy = np.cumsum(y_frames ** 2, axis=-1)              # input dtype, sequential
    energy = energy[:, win_length:] - energy[:, :-win_length]
    energy[np.abs(energy) < 1e-6] = 0
    yin = energy[:, :1] + energy - 2 * acf                  # float32 + float32, then promoted
    num = yin[:, min_period:max_period + 1]
    tau = np.arange(1, max_period + 1)
    cummean = np.cumsum(yin[:, 1:max_period + 1], axis=-1) / tau
    den = cummean[:, min_period - 1:max_period]
    return num / (den + TINY)


def parabolic_shifts(x):
    """librosa 0.10 _parabolic_interpolation along the last axis."""
    shifts = np.zeros_like(x)
    xm, x0, xp = x[:, :-2], x[:, 1:-1], x[:, 2:]
    a = xp + xm - 2 * x0
    b = (xp - xm) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(np.abs(b) >= np.abs(a), 0.0, -b / a)
    shifts[:, 1:-1] = s
    return shifts


def localmin(x):
    m = np.zeros(len(x), dtype=bool)
    m[1:-1] = (x[1:-1] < x[:-2]) & (x[1:-1] <= x[2:])
    m[-1] = x[-1] < x[-2]
    return m


def observations(yin, shifts, sr, fmin, thresholds, bprobs, boltzmann_parameter, no_trough_prob, min_period,
                 n_bins, nbps):
    """__pyin_helper -> (observation_probs [2 n_bins, T], voiced_prob [T])."""
    yin_probs = np.zeros_like(yin.T)                        # [P, T]
    for i, fr in enumerate(yin):
        is_trough = localmin(fr)
        is_trough[0] = fr[0] < fr[1]
        (idx,) = np.nonzero(is_trough)
        if len(idx) == 0:
            continue
        h = fr[idx]
        below = np.less.outer(h, thresholds[1:])
        pos = np.cumsum(below, axis=0) - 1
        n_tr = np.count_nonzero(below, axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            prior = scipy.stats.boltzmann.pmf(pos, boltzmann_parameter, n_tr)
        prior[~below] = 0
        probs = prior.dot(bprobs)
        gmin = np.argmin(h)
        n_below_min = np.count_nonzero(~below[gmin, :])
        probs[gmin] += no_trough_prob * np.sum(bprobs[:n_below_min])
        yin_probs[idx, i] = probs
    period, frame = np.nonzero(yin_probs)
    cand = min_period + period
    cand = cand + shifts.T[period, frame]
    f0c = sr / cand
    bins = 12 * nbps * np.log2(f0c / fmin)
    bins = np.clip(np.round(bins), 0, n_bins).astype(int)
    obs = np.zeros((2 * n_bins, yin.shape[0]))
    obs[bins, frame] = yin_probs[period, frame]
    vp = np.clip(np.sum(obs[:n_bins, :], axis=0), 0, 1)
    obs[n_bins:, :] = (1 - vp[None, :]) / n_bins
    return obs, vp


# ---------------------------------------------------------------------------------------------------------------------
# step 8
# ---------------------------------------------------------------------------------------------------------------------
def viterbi_dense(obs, transition, p_init):
    """librosa.sequence.viterbi (_viterbi): float64 log space, argmax ties to the lowest index."""
    log_trans = np.log(transition + TINY)
    log_prob = np.log(obs + TINY).T                         # [T, S]
    log_p_init = np.log(p_init + TINY)
    T, S = log_prob.shape
    value = np.empty((T, S))
    ptr = np.zeros((T, S), dtype=np.int64)
    value[0] = log_prob[0] + log_p_init
    lt_T = log_trans.T
    for t in range(1, T):
        trans_out = value[t - 1] + lt_T                     # [j, k]
        p = np.argmax(trans_out, axis=1)
        ptr[t] = p
        value[t] = log_prob[t] + trans_out[np.arange(S), p]
    states = np.empty(T, dtype=np.int64)
    states[-1] = np.argmax(value[-1])
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def banded_tables(transition, n_bins):
    """(H, same [n_bins][2H+1], cross [n_bins][2H+1]): log(A + tiny) of the sources k = j - H + d of target j, within the
    same voicing half and across it (the full matrix is kron(t_switch, T): both halves have the same band)."""
    T = transition[:n_bins, :n_bins]
    k, j = np.nonzero(T)
    H = int(np.abs(k - j).max()) if len(k) else 0
    la = np.log(transition + TINY)
    W = 2 * H + 1
    same = np.full((n_bins, W), -np.inf)
    cross = np.full((n_bins, W), -np.inf)
    for jj in range(n_bins):
        for d in range(W):
            kk = jj - H + d
            if 0 <= kk < n_bins:
                same[jj, d] = la[kk, jj]
                cross[jj, d] = la[n_bins + kk, jj]
    return H, same, cross


def viterbi_banded(obs, transition, p_init, n_bins):
    """The device kernel's decode, stated in NumPy: for target j only the 2 (2H+1) in-band sources are scanned; every
    other source k has log(A + tiny) = log(tiny) exactly, so the best of them is the source that maximises
    fl(value[k] + log(tiny)) at its lowest index g (rounding is monotone: that is the maximum of value, and g is the
    lowest index whose rounded sum equals it).  When g lies outside j's band it joins the scan as one more candidate;
    candidates are ordered by (value desc, index asc) -- the dense argmax."""
    H, same, cross = banded_tables(transition, n_bins)
    W = 2 * H + 1
    LT = np.log(TINY)
    log_prob = np.log(obs + TINY).T
    T, S = log_prob.shape
    # per target state j: source indices [S, 2W] (voiced band, then unvoiced band) and their log-transitions
    jb = np.arange(S) % n_bins
    half = np.arange(S) // n_bins
    kk = jb[:, None] - H + np.arange(W)[None, :]
    ok = (kk >= 0) & (kk < n_bins)
    src = np.concatenate([np.where(ok, kk, 0), np.where(ok, n_bins + kk, 0)], axis=1)
    tv = np.where((half == 0)[:, None], same[jb], cross[jb])     # voiced sources
    tu = np.where((half == 1)[:, None], same[jb], cross[jb])     # unvoiced sources
    tab = np.concatenate([np.where(ok, tv, -np.inf), np.where(ok, tu, -np.inf)], axis=1)
    valid = np.concatenate([ok, ok], axis=1)
    lo, hi = np.maximum(jb - H, 0), np.minimum(jb + H, n_bins - 1)
    big = np.iinfo(np.int64).max
    value = log_prob[0] + np.log(p_init + TINY)
    ptr = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        key = value + LT
        g = int(np.argmax(key))
        cand = np.where(valid, value[src] + tab, -np.inf)
        gb = g % n_bins
        gout = (gb < lo) | (gb > hi)
        cg = np.where(gout, key[g], -np.inf)
        best = np.maximum(cand.max(axis=1), cg)
        bi = np.where(valid & (cand == best[:, None]), src, big).min(axis=1)
        bi = np.where(gout & (cg == best), np.minimum(bi, g), bi)
        ptr[t] = bi
        value = log_prob[t] + best
    states = np.empty(T, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


# ---------------------------------------------------------------------------------------------------------------------
# pyin
# ---------------------------------------------------------------------------------------------------------------------
def pyin_stages(y, *, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
                beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
                switch_prob=0.01, no_trough_prob=0.01, center=True, pad_mode="constant"):
    z = sizes(len(y), sr, fmin, fmax, frame_length, win_length, hop_length, resolution, max_transition_rate, center)
    yf = frames(np.asarray(y), frame_length, z["hop_length"], center, pad_mode)
    yin = cmnd(yf, frame_length, z["win_length"], z["min_period"], z["max_period"])
    sh = parabolic_shifts(yin)
    thr, bp = beta_probs(n_thresholds, beta_parameters)
    obs, vp = observations(yin, sh, sr, fmin, thr, bp, boltzmann_parameter, no_trough_prob, z["min_period"],
                           z["n_bins"], z["nbps"])
    A = transition_full(z["n_bins"], z["width"], switch_prob)
    p_init = np.zeros(2 * z["n_bins"])
    p_init[z["n_bins"]:] = 1 / z["n_bins"]
    return dict(sizes=z, cmnd=yin, obs=obs, voiced_prob=vp, A=A, p_init=p_init)


def finish(states, st, fmin, fill_na=np.nan):
    z = st["sizes"]
    n_bins, nbps = z["n_bins"], z["nbps"]
    freqs = fmin * 2 ** (np.arange(n_bins) / (12 * nbps))
    f0 = freqs[states % n_bins]
    voiced = states < n_bins
    if fill_na is not None:
        f0[~voiced] = fill_na
    return f0, voiced, st["voiced_prob"]


def pyin_dense(y, *, fmin, fmax, sr=22050, fill_na=np.nan, return_states=False, **kw):
    st = pyin_stages(y, fmin=fmin, fmax=fmax, sr=sr, **kw)
    states = viterbi_dense(st["obs"], st["A"], st["p_init"])
    out = finish(states, st, fmin, fill_na)
    return (out + (states,)) if return_states else out


def pyin_banded(y, *, fmin, fmax, sr=22050, fill_na=np.nan, return_states=False, **kw):
    st = pyin_stages(y, fmin=fmin, fmax=fmax, sr=sr, **kw)
    states = viterbi_banded(st["obs"], st["A"], st["p_init"], st["sizes"]["n_bins"])
    out = finish(states, st, fmin, fill_na)
    return (out + (states,)) if return_states else out


# ---------------------------------------------------------------------------------------------------------------------
# get_f0 / interp_NAN (script/calc.py:345-592, method='pyin')
# ---------------------------------------------------------------------------------------------------------------------
def interp_NAN(X, method="linear"):
    newX = np.array(X, copy=True)
    mynans = np.isnan(newX)
    if np.sum(mynans) == 0:
        return newX
    justnans = np.empty(np.size(X))
    justnans[:] = np.nan
    if method == "pchip":
        if np.argwhere(mynans)[0] == 0:
            newX[0] = newX[np.argwhere(np.isnan(newX) == 0)[0]]
        if np.argwhere(mynans)[-1] == len(X) - 1:
            newX[-1] = newX[np.argwhere(np.isnan(newX) == 0)[-1]]
        mynans = np.isnan(newX)
        f = interpolate.PchipInterpolator(np.where(mynans == 0)[0], newX[mynans == 0], extrapolate=False)
    else:
        f = interpolate.interp1d(np.where(mynans == 0)[0], newX[mynans == 0], method, fill_value="extrapolate")
    justnans[mynans] = f(np.squeeze(np.where(mynans)))
    newX[mynans] = justnans[mynans]
    return newX


def _lowpass(x, sr, cut, order):
    sos = scipy.signal.butter(order, cut / (sr / 2), btype="low", output="sos")
    return scipy.signal.sosfiltfilt(sos, x)


def get_f0(x, sr, hopSize=0.01, minPitch=75, maxPitch=600, interpUnvoiced="linear", outFilter="iir",
           outFiltCutOff=(12,), outFiltLen=6, outFiltPolyOrd=3, minMaxQuant=None, banded=False, **pyin_kw):
    """get_f0(method='pyin') with a low-pass 'iir' or 'sg' output filter (the reference's own scipy calls)."""
    run = pyin_banded if banded else pyin_dense
    hop_length = int(hopSize * sr)
    f0, _, _ = run(x, fmin=minPitch, fmax=maxPitch, sr=sr, hop_length=hop_length, **pyin_kw)
    if minMaxQuant is not None:
        v = f0[np.isnan(f0) == 0]
        q = np.quantile(v, [minMaxQuant[0], minMaxQuant[1]])
        f0, _, _ = run(x, fmin=q[0], fmax=q[1], sr=sr, hop_length=hop_length, **pyin_kw)
    f0t = np.arange(len(f0)) * hopSize
    if interpUnvoiced is not None:
        f0 = interp_NAN(f0, interpUnvoiced)
    if outFilter == "iir":
        f0 = _lowpass(f0, 1 / hopSize, outFiltCutOff[0], outFiltLen)
    elif outFilter == "sg":
        f0 = scipy.signal.savgol_filter(f0, outFiltLen, outFiltPolyOrd, deriv=0, mode="interp")
    return f0, f0t


# ---------------------------------------------------------------------------------------------------------------------
# deterministic test signals
# ---------------------------------------------------------------------------------------------------------------------
def synth(kind, sr, seconds, dtype=np.float64, seed=0):
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    rng = np.random.default_rng(seed)
    if kind == "glide":                                     # 110 -> 330 Hz, 5 Hz vibrato, silent gaps, light noise
        f = 110 * 3 ** (t / seconds) * (1 + 0.01 * np.sin(2 * np.pi * 5 * t))
        ph = 2 * np.pi * np.cumsum(f) / sr
        y = sum((0.5 / k) * np.sin(k * ph) for k in (1, 2, 3, 4))
        gate = ((t % 0.6) < 0.45).astype(float)
        y = y * gate + 0.003 * rng.standard_normal(n)
    elif kind.startswith("sine"):                           # sine200, sine50, sine800
        y = 0.5 * np.sin(2 * np.pi * float(kind[4:]) * t)
    elif kind == "noise":
        y = 0.3 * rng.standard_normal(n)
    elif kind == "silence":
        y = np.zeros(n)
    elif kind == "fade":                                    # 220 Hz tone fading far below the 1e-6 cuts
        y = 0.5 * np.sin(2 * np.pi * 220 * t) * np.exp(-t * 12.0 / seconds * math.log(10))
    else:
        raise ValueError(kind)
    return y.astype(dtype)
