"""pYIN f0 tracking on the GPU: librosa.pyin as the reference's ``get_f0(method='pyin')`` calls it
(script/calc.py:386-592), and its ``interp_NAN`` (:345-385).

    pyin_batch(audio [B, n] | [n] device tensor, sr, fmin=, fmax=, ...)  -> (f0, voiced_flag, voiced_prob) on the device
    pyin_ragged_batch(audio [B, n_max], lengths [B], sr, ...)             -> the same with a length per clip (+ frames [B])
    get_f0_batch(clips, sr, method='pyin', ...)                           -> [(f0, f0t), ...]: get_f0 of a list of clips
    pyin(y, fmin=, fmax=, sr=22050, ...)                                  -> librosa.pyin's signature: numpy in, numpy out
    interp_NAN(X, method='linear')                                        -> 'linear' on the device, other kinds via scipy
    interp_nan_spline_batch(x, 'quadratic' | 'cubic')                     -> scipy's spline gap filling on the device
    get_f0(x, sr, method='pyin', ...)                                     -> (f0, f0t), the reference's signature

The device path is three kernels (csrc/mm_pitch.hip): the cumulative-mean-normalised difference of every frame, the
trough probabilities and pitch-bin candidates of every frame, and a banded Viterbi decode per clip.  Every constant
table is built here with numpy / scipy exactly as librosa builds it (the beta and Boltzmann distributions, the
transition matrix of librosa.sequence), so the device never re-derives a special function.  The Praat methods
('praatac' / 'praatcc') call Praat through parselmouth and are not part of this package.
"""
from __future__ import annotations

import collections
import ctypes as C
import inspect

import numpy as np
import scipy.signal
import scipy.stats
from scipy import interpolate

from . import ragged
from .filters import applyFilter, apply_filter_ragged_batch

__all__ = ["pyin_batch", "pyin_ragged_batch", "pyin_ragged_frames", "pyin", "interp_NAN", "interp_nan_batch",
           "interp_nan_ragged_batch", "interp_nan_spline_batch", "interp_nan_spline_ragged_batch", "get_f0", "get_f0_batch", "pyin_sizes", "beta_tables", "boltzmann_table",
           "transition_matrix", "banded_log_transitions", "pitch_freqs", "pyin_params", "pyin_cmnd", "pyin_records"]

TINY = np.finfo(np.float64).tiny
PYIN_WS_BYTES = 512 << 20      # scratch bound of one device call (back-pointers + per-frame records): batches are cut to fit


# ---------------------------------------------------------------------------------------------------------------------
# host tables (no GPU needed)
# ---------------------------------------------------------------------------------------------------------------------
def pyin_sizes(n, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, resolution=0.1,
               max_transition_rate=35.92, center=True):
    """The derived sizes of one librosa.pyin call: frames, lag range, pitch bins, transition width."""
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
    n_frames = 1 + (n_pad - frame_length) // hop_length if n_pad >= frame_length else 0
    return dict(win_length=int(win_length), hop_length=int(hop_length), min_period=min_period,
                max_period=max_period, nbps=nbps, n_bins=n_bins, width=int(width), n_frames=int(n_frames))


def beta_tables(n_thresholds=100, beta_parameters=(2, 18)):
    """(thresholds [n + 1], beta_probs [n], beta_cum [n + 1]): librosa's threshold grid, the beta distribution's mass
    between thresholds, and np.sum(beta_probs[:k]) for every k (the no-trough bonus of the global minimum)."""
    thresholds = np.linspace(0, 1, n_thresholds + 1)
    beta_cdf = scipy.stats.beta.cdf(thresholds, beta_parameters[0], beta_parameters[1])
    beta_probs = np.diff(beta_cdf)
    beta_cum = np.array([np.sum(beta_probs[:k]) for k in range(n_thresholds + 1)])
    return thresholds, beta_probs, beta_cum


def max_troughs(min_period, max_period):
    """Trough slots per frame: troughs of a CMND row are at least two lags apart."""
    return (max_period - min_period + 2) // 2 + 1


def boltzmann_table(R, boltzmann_parameter=2):
    """[R + 1][R]: entry [N][k] = scipy.stats.boltzmann.pmf(k, boltzmann_parameter, N) for k < N (0 elsewhere)."""
    tab = np.zeros((R + 1, R))
    N = np.arange(1, R + 1)[:, None]
    k = np.arange(R)[None, :]
    NN, KK = np.broadcast_arrays(N, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = scipy.stats.boltzmann.pmf(KK, boltzmann_parameter, NN)
    tab[1:] = np.where(KK < NN, v, 0.0)
    return tab


def _transition_local(n_states, width):
    # librosa.sequence.transition_local(n_states, width, window='triangle', wrap=False), line for line
    transition = np.zeros((n_states, n_states), dtype=np.float64)
    for i in range(n_states):
        w = scipy.signal.get_window("triangle", width, fftbins=False)
        lpad = (n_states - width) // 2
        if lpad < 0:
            raise ValueError(f"pyin: transition width {width} exceeds the {n_states} pitch bins of fmin..fmax "
                             "(librosa.util.pad_center raises the same)")
        trans_row = np.pad(w, (lpad, n_states - width - lpad), mode="constant")
        trans_row = np.roll(trans_row, n_states // 2 + i + 1)
        trans_row[min(n_states, i + width // 2 + 1):] = 0
        trans_row[:max(0, i - width // 2)] = 0
        transition[i] = trans_row
    transition /= transition.sum(axis=1, keepdims=True)
    return transition


def transition_matrix(n_bins, width, switch_prob=0.01):
    """The dense [2 n_bins]^2 transition of librosa.pyin: np.kron(transition_loop(2, 1 - switch_prob),
    transition_local(n_bins, width, window='triangle', wrap=False))."""
    p = 1 - switch_prob
    t_switch = np.empty((2, 2))
    t_switch[:] = (1 - p) / 1          # transition_loop: off-diagonal (1 - prob) / (n_states - 1)
    t_switch[0, 0] = p
    t_switch[1, 1] = p
    return np.kron(t_switch, _transition_local(n_bins, width))


def banded_log_transitions(n_bins, width, switch_prob=0.01):
    """(H, same [n_bins][2H+1], cross [n_bins][2H+1]): log(A + tiny) of source bin j - H + d into target bin j, within one
    voicing half and across the halves, taken from the dense matrix itself (so bitwise librosa's values); H is the
    widest |source - target| with a nonzero transition.  Entries of sources outside [0, n_bins) are -inf (never read)."""
    A = transition_matrix(n_bins, width, switch_prob)
    T = A[:n_bins, :n_bins]
    k, j = np.nonzero(T)
    H = int(np.abs(k - j).max()) if len(k) else 0
    la = np.log(A + TINY)
    W = 2 * H + 1
    kk = np.arange(n_bins)[:, None] - H + np.arange(W)[None, :]
    ok = (kk >= 0) & (kk < n_bins)
    kc = np.where(ok, kk, 0)
    jj = np.broadcast_to(np.arange(n_bins)[:, None], kk.shape)
    same = np.where(ok, la[kc, jj], -np.inf)
    cross = np.where(ok, la[n_bins + kc, jj], -np.inf)
    return H, np.ascontiguousarray(same), np.ascontiguousarray(cross)


def pitch_freqs(fmin, n_bins, nbps):
    return fmin * 2 ** (np.arange(n_bins) / (12 * nbps))


def _check_params(sr, fmin, fmax, frame_length, win_length):
    if fmin is None or fmax is None:
        raise ValueError('both "fmin" and "fmax" must be provided')
    if fmin >= fmax:
        raise ValueError(f"fmin={fmin} must be less than fmax={fmax}")
    if fmax > sr / 2:
        raise ValueError(f"fmax={fmax} must not exceed the Nyquist frequency sr/2={sr / 2}")
    if win_length >= frame_length:
        raise ValueError(f"win_length={win_length} must be less than frame_length={frame_length}")


def pyin_params(n, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
                resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan,
                center=True):
    """(mm_pyin_params, sizes dict) of one call, validated by the library (mm_pyin_check; no GPU needed).  Raises
    ValueError for librosa's parameter errors, NotImplementedError beyond the kernels' limits."""
    from . import _lib
    wl = frame_length // 2 if win_length is None else win_length
    _check_params(sr, fmin, fmax, frame_length, wl)
    z = pyin_sizes(n, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                   hop_length=hop_length, resolution=resolution, max_transition_rate=max_transition_rate, center=center)
    p = _lib.mm_pyin_params()
    p.sr, p.fmin, p.fmax = float(sr), float(fmin), float(fmax)
    p.no_trough_prob = float(no_trough_prob)
    p.log_tiny = float(np.log(TINY))
    p.fill_na = float(np.nan if fill_na is None else fill_na)
    p.log_p_init[0] = float(np.log(0.0 + TINY))
    p.log_p_init[1] = float(np.log(1 / z["n_bins"] + TINY))
    p.frame_length, p.win_length, p.hop_length = int(frame_length), z["win_length"], z["hop_length"]
    p.center = 1 if center else 0
    p.min_period, p.max_period = z["min_period"], z["max_period"]
    p.n_thresholds, p.nbps, p.n_bins = int(n_thresholds), z["nbps"], z["n_bins"]
    p.band_h = (z["width"] - 1) // 2
    p.max_troughs = max_troughs(z["min_period"], z["max_period"])
    _lib.check(_lib.load().mm_pyin_check(C.byref(p)), "pyin parameters")
    return p, z


# ---------------------------------------------------------------------------------------------------------------------
# device tables (cached per parameter set and device)
# ---------------------------------------------------------------------------------------------------------------------
_TABLES = collections.OrderedDict()
MAX_TABLES = 16


class _Tables:
    def __init__(self, key, device):
        import torch
        from . import _lib
        (fmin, n_bins, nbps, width, switch_prob, n_thr, beta_parameters, boltz, R) = key
        thr, bp, bc = beta_tables(n_thr, beta_parameters)
        H, same, cross = banded_log_transitions(n_bins, width, switch_prob)
        self.H = H
        arrs = dict(thresholds=thr, beta_probs=bp, beta_cum=bc, boltzmann=boltzmann_table(R, boltz),
                    log_same=same, log_cross=cross, freqs=pitch_freqs(fmin, n_bins, nbps))
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device) for k, v in arrs.items()}
        t = _lib.mm_pyin_tables()
        for k, v in self.dev.items():
            setattr(t, k, v.data_ptr())
        self.c = t


def _tables(p, z, switch_prob, beta_parameters, boltzmann_parameter, device):
    key = (float(p.fmin), z["n_bins"], z["nbps"], z["width"], float(switch_prob), int(p.n_thresholds),
           tuple(float(b) for b in beta_parameters), boltzmann_parameter, int(p.max_troughs))
    dk = (key, str(device))
    if dk in _TABLES:
        _TABLES.move_to_end(dk)
    else:
        import torch
        while len(_TABLES) >= MAX_TABLES:
            _TABLES.popitem(last=False)
            torch.cuda.synchronize(device)
        _TABLES[dk] = _Tables(key, device)
    return _TABLES[dk]


def _as_signal(audio):
    """Device rows [B, n] in the type the kernels take: float32 stays float32 (librosa's energy terms then run in
    float32), everything else becomes float64 (integer PCM keeps its values) -> (rows, whether audio was [n])."""
    import torch
    x = ragged.device_rows(audio, (torch.float32, torch.float64), "audio must be a CUDA(HIP) tensor [n] or [B, n]",
                           "audio must be [n] or [B, n]", widen=torch.float64, one_dim=True, nonempty=False)
    return x, audio.dim() == 1


_TORCH_PAD = {"reflect": "reflect", "edge": "replicate", "wrap": "circular"}


def _pad_center(x, frame_length, pad_mode):
    """np.pad(x, frame_length // 2, mode=pad_mode) of every row of [B, n], on the device."""
    import torch
    if pad_mode not in _TORCH_PAD:
        raise NotImplementedError(f"pad_mode={pad_mode!r}: the device path pads 'constant', 'reflect', 'edge', 'wrap'")
    h = frame_length // 2
    return torch.nn.functional.pad(x.unsqueeze(1), (h, h), mode=_TORCH_PAD[pad_mode]).squeeze(1).contiguous()


def pyin_batch(audio, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
               beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
               switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan, center=True, pad_mode="constant",
               return_states=False):
    """librosa.pyin on every row of a device batch -> (f0 float64, voiced_flag bool, voiced_prob float64), each
    [B, n_frames] (or [n_frames] for a [n] input), on the input's device.  ``return_states`` adds the decoded Viterbi
    states (int32; state < n_bins is voiced).  Batches are cut so that one call's scratch stays within PYIN_WS_BYTES."""
    import torch
    from . import _lib
    x, squeeze = _as_signal(audio)
    if center and pad_mode != "constant":
        x = _pad_center(x, frame_length, pad_mode)
        center = False
    B, n = x.shape
    p, z = pyin_params(n, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                       hop_length=hop_length, n_thresholds=n_thresholds, resolution=resolution,
                       max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob,
                       fill_na=fill_na, center=center)
    T = z["n_frames"]
    if T < 1:
        raise ValueError(f"pyin: a signal of {n} samples is shorter than frame_length={frame_length}")
    lib = _lib.load()
    tabs = _tables(p, z, switch_prob, beta_parameters, boltzmann_parameter, x.device)
    p.band_h = tabs.H
    dev = x.device
    f0 = torch.empty((B, T), dtype=torch.float64, device=dev)
    voiced = torch.empty((B, T), dtype=torch.uint8, device=dev)
    vprob = torch.empty((B, T), dtype=torch.float64, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    rows = B
    while rows > 1 and lib.mm_pyin_workspace_bytes(C.byref(p), rows, n) > PYIN_WS_BYTES:
        rows = max(1, min(rows - 1, rows * PYIN_WS_BYTES // lib.mm_pyin_workspace_bytes(C.byref(p), rows, n)))
    ws = torch.empty(int(lib.mm_pyin_workspace_bytes(C.byref(p), rows, n)), dtype=torch.uint8, device=dev)
    fn, name = (lib.mm_pyin_f32, "mm_pyin_f32") if x.dtype == torch.float32 else (lib.mm_pyin_f64, "mm_pyin_f64")
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for r0 in range(0, B, rows):
            r = min(rows, B - r0)
            _lib.check(fn(C.byref(p), C.byref(tabs.c), x[r0].data_ptr(), r, n, ragged.row_pitch(x), f0[r0].data_ptr(),
                          voiced[r0].data_ptr(), vprob[r0].data_ptr(), states[r0].data_ptr(), ws.data_ptr(), ws.numel(),
                          stream), name)
    if fill_na is None:                 # librosa keeps the decoded bin's frequency on unvoiced frames
        f0 = tabs.dev["freqs"][(states % z["n_bins"]).long()]
    out = (f0, voiced.bool(), vprob) + ((states,) if return_states else ())
    return tuple(o[0] for o in out) if squeeze else out


pyin_ragged_frames = ragged.centered_frames     # frames of clips of ``lengths`` samples: mm_pyin_num_frames per clip

_MSG_SHORT = "pyin: a signal of {} samples is shorter than frame_length={}"


def pyin_ragged_batch(audio, lengths, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None,
                      n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1,
                      max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan, center=True,
                      pad_mode="constant", return_states=False):
    """pyin_batch for clips of different lengths in one padded batch: ``audio`` [B, n_max] (float32 or float64 on the
    device, any row pitch >= n_max) and one valid sample count per clip -> (f0, voiced_flag, voiced_prob, frames), each
    [B, T_max] but ``frames`` (int64 [B] on the device), and the states under ``return_states``.  Row b holds, in the
    columns [0, frames[b]), exactly what pyin_batch returns for audio[b, :lengths[b]] alone -- its own centre padding, its
    own last frame, its own decode -- and zeros behind them; what the padding of ``audio`` holds never matters.

    ``lengths``: host integers (validated: ValueError outside [1, n_max], and pyin_batch's ValueError with the clip's index
    for a clip without a frame) or an int64 device tensor (no read-back; the kernels clamp it, and a clip without a frame
    gets an all-zero row and frames[b] == 0).  ``center=True`` with another ``pad_mode`` than 'constant' needs host
    lengths: every clip is padded alone and the batch is packed again.  The scratch follows T_max, not the sum of the
    clips' frames; batches are cut to PYIN_WS_BYTES as in pyin_batch."""
    import torch
    from . import _lib
    x, _ = _as_signal(audio)
    if audio.dim() != 2:
        raise ValueError("audio must be [B, n_max]")
    B, n = x.shape
    lens = ragged.check_lengths(lengths, B, n, x.device)
    on_host = isinstance(lens, np.ndarray)
    if center and pad_mode != "constant":
        if not on_host:
            raise ValueError(f"pad_mode={pad_mode!r} pads every clip on its own: lengths must be host values")
        h = frame_length // 2
        padded = torch.empty((B, n + 2 * h), dtype=x.dtype, device=x.device)
        for b in range(B):
            padded[b, :int(lens[b]) + 2 * h] = _pad_center(x[b:b + 1, :int(lens[b])], frame_length, pad_mode)[0]
        x, n, lens, center = padded, n + 2 * h, lens + 2 * h, False
    p, z = pyin_params(n, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                       hop_length=hop_length, n_thresholds=n_thresholds, resolution=resolution,
                       max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob,
                       fill_na=fill_na, center=center)
    T = z["n_frames"]
    if T < 1:
        raise ValueError(_MSG_SHORT.format(n, frame_length))
    ragged.refuse_short(lens, n, 1 if center else frame_length, lambda short: _MSG_SHORT.format(short, frame_length), "clip", None)
    lib = _lib.load()
    dev = x.device
    tabs = _tables(p, z, switch_prob, beta_parameters, boltzmann_parameter, dev)
    p.band_h = tabs.H
    f0 = torch.empty((B, T), dtype=torch.float64, device=dev)
    voiced = torch.empty((B, T), dtype=torch.uint8, device=dev)
    vprob = torch.empty((B, T), dtype=torch.float64, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    frames = torch.empty(B, dtype=torch.int64, device=dev)
    need = lib.mm_pyin_ragged_workspace_bytes
    rows = B
    while rows > 1 and need(C.byref(p), rows, n) > PYIN_WS_BYTES:
        rows = max(1, min(rows - 1, rows * PYIN_WS_BYTES // need(C.byref(p), rows, n)))
    ws = torch.empty(int(need(C.byref(p), rows, n)), dtype=torch.uint8, device=dev)
    f32 = x.dtype == torch.float32
    name = "mm_pyin_ragged_f32" if f32 else "mm_pyin_ragged_f64"
    with torch.cuda.device(dev):
        lens_dev = ragged.counts_on_device(lens, dev)       # (on the current stream)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for r0 in range(0, B, rows):
            r = min(rows, B - r0)
            fn = lib.mm_pyin_ragged_f32 if f32 else lib.mm_pyin_ragged_f64
            _lib.check(fn(C.byref(p), C.byref(tabs.c), x[r0].data_ptr(), r, n, ragged.row_pitch(x), lens_dev[r0:].data_ptr(),
                          f0[r0].data_ptr(), voiced[r0].data_ptr(), vprob[r0].data_ptr(), states[r0].data_ptr(),
                          frames[r0:].data_ptr(), ws.data_ptr(), ws.numel(), stream), name)
    if fill_na is None:                 # librosa keeps the decoded bin's frequency on unvoiced frames: of real frames only
        live = torch.arange(T, device=dev)[None, :] < frames[:, None]
        f0 = tabs.dev["freqs"][(states % z["n_bins"]).long()] * live
    return (f0, voiced.bool(), vprob, frames) + ((states,) if return_states else ())


def pyin_cmnd(audio, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, center=True):
    """Stage: the cumulative-mean-normalised difference rows [B, n_frames, max_period - min_period + 1] (float64) of
    a device batch (mm_pyin_cmnd; zero padding when centred)."""
    import torch
    from . import _lib
    x, squeeze = _as_signal(audio)
    B, n = x.shape
    p, z = pyin_params(n, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                       hop_length=hop_length, center=center)
    out = torch.empty((B, z["n_frames"], z["max_period"] - z["min_period"] + 1), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mm_pyin_cmnd(C.byref(p), x.data_ptr(), 0 if x.dtype == torch.float32 else 1, B, n,
                                            ragged.row_pitch(x), out.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "mm_pyin_cmnd")
    return out[0] if squeeze else out


def pyin_records(cmnd, sr, *, fmin, fmax, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
                 beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
                 switch_prob=0.01, no_trough_prob=0.01):
    """Stage: CMND rows [n_frames, P] (pyin_cmnd of one row) -> the per-frame observation records of mm_pyin_candidates:
    (count [T] int32, bins [T, max_troughs] int32, probs [T, max_troughs] float64, voiced_prob [T] float64)."""
    import torch
    from . import _lib
    T = cmnd.shape[0]
    p, z = pyin_params(frame_length, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                       hop_length=hop_length, n_thresholds=n_thresholds, resolution=resolution,
                       max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob)
    tabs = _tables(p, z, switch_prob, beta_parameters, boltzmann_parameter, cmnd.device)
    p.band_h = tabs.H
    R = p.max_troughs
    c = cmnd.contiguous()
    dev = c.device
    count = torch.zeros(T, dtype=torch.int32, device=dev)
    bins = torch.zeros((T, R), dtype=torch.int32, device=dev)
    probs = torch.zeros((T, R), dtype=torch.float64, device=dev)
    vp = torch.empty(T, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mm_pyin_candidates(C.byref(p), C.byref(tabs.c), c.data_ptr(), T, count.data_ptr(),
                                                  bins.data_ptr(), probs.data_ptr(), vp.data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "mm_pyin_candidates")
    return count, bins, probs, vp


def _gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("modulation_mfcc_amd needs an AMD GPU (gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device_signal(y):
    """numpy -> device tensor: float32 and float64 keep their type, integer PCM (and anything else) becomes float64."""
    import torch
    a = np.asarray(y)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(_gpu())


def pyin(y, *, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100,
         beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01,
         no_trough_prob=0.01, fill_na=np.nan, center=True, pad_mode="constant"):
    """librosa.pyin's signature and defaults: a 1-D (or [B, n]) numpy signal -> numpy (f0, voiced_flag, voiced_prob),
    computed on the GPU."""
    out = pyin_batch(_to_device_signal(y), sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                     hop_length=hop_length, n_thresholds=n_thresholds, beta_parameters=beta_parameters,
                     boltzmann_parameter=boltzmann_parameter, resolution=resolution,
                     max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob,
                     fill_na=fill_na, center=center, pad_mode=pad_mode)
    return tuple(o.cpu().numpy() for o in out)


# ---------------------------------------------------------------------------------------------------------------------
# interp_NAN / get_f0 (script/calc.py:345-592)
# ---------------------------------------------------------------------------------------------------------------------
def _interp_linear_device(X):
    import torch
    from . import _lib
    squeeze = X.dim() == 1
    x = X.unsqueeze(0) if squeeze else X
    if x.dim() != 2:
        raise ValueError("X must be [n] or [rows, n]")
    xd = x.to(torch.float64).contiguous()
    valid = (~torch.isnan(xd)).sum(dim=1)
    if bool((valid < 2).any()):         # scipy.interpolate.interp1d needs two points
        raise ValueError("x and y arrays must have at least 2 entries")
    y = torch.empty_like(xd)
    rows, n = xd.shape
    with torch.cuda.device(xd.device):
        _lib.check(_lib.load().mm_interp_nan_linear_f64(xd.data_ptr(), rows, n, n, y.data_ptr(), n,
                                                         C.c_void_p(torch.cuda.current_stream(xd.device).cuda_stream)),
                   "mm_interp_nan_linear_f64")
    y = y.to(X.dtype)
    return y[0] if squeeze else y


def _interp_nan_host(X, method):
    # script/calc.py:345-385 as written
    import copy
    newX = copy.copy(X)
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


INTERP_SEGMENT = 1024       # samples per workgroup of the segmented interp_NAN kernels (kIpSeg of csrc/mm_interp.hip)
# interp_NAN methods of mm_interp_nan_f64 (MM_INTERP_* of include/modmfcc.h)
_INTERP_KINDS = {"pchip": 0, "nearest": 1, "nearest-up": 2, "previous": 3, "next": 4, "zero": 5, "slinear": 6}
_INTERP_HOST_KINDS = ("quadratic", "cubic")     # a banded solve over all knots: scipy on the host


def _interp_kind_device(X, method):
    import torch
    from . import _lib
    kind = _INTERP_KINDS[method]
    squeeze = X.dim() == 1
    x = X.unsqueeze(0) if squeeze else X
    if x.dim() != 2:
        raise ValueError("X must be [n] or [rows, n]")
    if not x.is_floating_point():
        raise TypeError("X must be a floating-point tensor")
    rows, n = x.shape
    if rows == 0 or n == 0:
        return X.clone()
    xd = x.to(torch.float64)
    if xd.stride(1) != 1 or xd.stride(0) < n:
        xd = xd.contiguous()
    fewest = int((~torch.isnan(xd)).sum(dim=1).min())   # the one read-back: what scipy would raise for
    if fewest == n:
        return X.clone()
    if method == "slinear" and fewest < 2:
        raise ValueError("x and y arrays must have at least 2 entries")
    if fewest < 1:
        if method == "pchip":                            # the reference's np.argwhere(...)[0] of an empty array
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        raise ValueError("cannot reshape array of size 0 into shape (0,newaxis)")     # scipy interp1d of empty x
    y = torch.empty((rows, n), dtype=torch.float64, device=xd.device)
    lib = _lib.load()
    with torch.cuda.device(xd.device):
        ws = torch.empty(int(lib.mm_interp_nan_workspace_bytes(kind, rows, n)), dtype=torch.uint8, device=xd.device)
        _lib.check(lib.mm_interp_nan_f64(kind, xd.data_ptr(), rows, n, xd.stride(0), y.data_ptr(), n, ws.data_ptr(),
                                         ws.numel(), C.c_void_p(torch.cuda.current_stream(xd.device).cuda_stream)),
                   "mm_interp_nan_f64")
    y = y.to(X.dtype)
    return y[0] if squeeze else y


def interp_nan_batch(x, method: str = "linear"):
    """interp_NAN along the last axis of a CUDA(HIP) tensor [n] or [rows, n] of any float dtype, on the device only:
    computed in float64 and cast back.  ``method``: 'linear' (mm_interp_nan_linear_f64) or one of 'pchip', 'nearest',
    'nearest-up', 'previous', 'next', 'zero', 'slinear' (mm_interp_nan_f64; rows are cut into segments of INTERP_SEGMENT
    samples, one workgroup each).  'quadratic' and 'cubic' need a solve over all knots: NotImplementedError here
    (interp_NAN runs them through scipy on the host); any other name is a ValueError.  Rows with too few valid samples
    raise what the reference raises (interp_NAN's doc string), after one read-back of the smallest count."""
    if not ragged.is_device_tensor(x):
        raise TypeError("interp_nan_batch takes a CUDA(HIP) tensor; interp_NAN also takes numpy curves")
    if method == "linear":
        return _interp_linear_device(x)
    if method in _INTERP_KINDS:
        return _interp_kind_device(x, method)
    if method in _INTERP_HOST_KINDS:
        raise NotImplementedError(f"method={method!r} needs a banded solve over all knots; not on the device")
    raise ValueError(f"interp_nan_batch: unknown method {method!r}")


def interp_nan_ragged_batch(x, counts, method: str = "linear"):
    """interp_nan_batch with a count per row: ``x`` [rows, n_max] on the device, ``counts`` [rows] (host integers,
    validated: ValueError outside [1, n_max]; or an int64 device tensor, clamped by the kernels) -> [rows, n_max] of x's
    dtype.  Row b holds interp_nan_batch(x[b, :counts[b]], method) in the columns [0, counts[b]) and zeros behind them;
    what x holds behind a row's count never matters.  The methods and the errors are interp_nan_batch's, the errors taken
    from the smallest number of valid samples below a row's count, in one read-back."""
    import torch
    from . import _lib
    xd = ragged.device_rows(x, (torch.float64,), "interp_nan_ragged_batch takes a CUDA(HIP) tensor", "x must be [rows, n_max]",
                            widen=torch.float64, nonempty=False)
    if method != "linear" and method not in _INTERP_KINDS:
        if method in _INTERP_HOST_KINDS:
            raise NotImplementedError(f"method={method!r} needs a banded solve over all knots; not on the device")
        raise ValueError(f"interp_nan_ragged_batch: unknown method {method!r}")
    if not x.is_floating_point():
        raise TypeError("x must be a floating-point tensor")
    rows, n = x.shape
    if rows == 0 or n == 0:
        return x.clone()
    dev = x.device
    cnt = ragged.check_counts(counts, rows, n, dev, "counts")
    pitch_ = ragged.row_pitch(xd)
    with torch.cuda.device(dev):
        cd = ragged.counts_on_device(cnt, dev)
        c = cd.clamp(1, n)
        valid = ((~torch.isnan(xd)) & (torch.arange(n, device=dev)[None, :] < c[:, None])).sum(dim=1)
        if method == "linear":                              # scipy.interpolate.interp1d needs two points, NaN or not
            if int(valid.min()) < 2:
                raise ValueError("x and y arrays must have at least 2 entries")
        else:                                               # a row without a NaN below its count is returned as it is
            fewest = int(torch.where(valid < c, valid, torch.full_like(valid, 2)).min())
            if method == "slinear" and fewest < 2:
                raise ValueError("x and y arrays must have at least 2 entries")
            if fewest < 1:
                if method == "pchip":
                    raise IndexError("index 0 is out of bounds for axis 0 with size 0")
                raise ValueError("cannot reshape array of size 0 into shape (0,newaxis)")
        y = torch.empty((rows, n), dtype=torch.float64, device=dev)
        lib = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if method == "linear":
            _lib.check(lib.mm_interp_nan_linear_ragged_f64(xd.data_ptr(), rows, n, pitch_, cd.data_ptr(), y.data_ptr(), n,
                                                           stream), "mm_interp_nan_linear_ragged_f64")
        else:
            kind = _INTERP_KINDS[method]
            ws = torch.empty(int(lib.mm_interp_nan_workspace_bytes(kind, rows, n)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mm_interp_nan_ragged_f64(kind, xd.data_ptr(), rows, n, pitch_, cd.data_ptr(), y.data_ptr(), n,
                                                    ws.data_ptr(), ws.numel(), stream), "mm_interp_nan_ragged_f64")
    return y.to(x.dtype)


SPLINE_CHUNK = 1024         # knots per workgroup of the spline solve (kSpChunk of csrc/mm_spline.hip): longer rows are cut
# interp_NAN methods of mm_interp_spline_f64 (MM_SPLINE_* of include/modmfcc_spline.h): the kind is the spline's degree
_SPLINE_KINDS = {"quadratic": 2, "cubic": 3}
_MSG_SPLINE_FEW = "The number of derivatives at boundaries does not match: expected {}, got 0+0"   # make_interp_spline's


def _spline_kind(method, who):
    if method not in _SPLINE_KINDS:
        raise ValueError(f"{who}: method must be 'quadratic' or 'cubic', got {method!r}")
    return _SPLINE_KINDS[method]


def _spline_refuse(kind, fewest):
    """scipy's ValueError for the row with the fewest valid samples among the rows that have a NaN."""
    if fewest < 1:
        raise ValueError("cannot reshape array of size 0 into shape (0,newaxis)")          # scipy interp1d of empty x
    if fewest <= kind:
        raise ValueError(_MSG_SPLINE_FEW.format(kind + 1 - fewest))


def interp_nan_spline_batch(x, method: str = "cubic"):
    """interp_NAN's 'quadratic' and 'cubic' kinds along the last axis of a CUDA(HIP) tensor [n] or [rows, n] of any float
    dtype, on the device only (mm_interp_spline_f64): computed in float64 and cast back.  scipy's
    interp1d(valid indices, valid values, method, fill_value='extrapolate') at the NaN samples -- the not-a-knot cubic
    spline, the quadratic spline with its knots at the midpoints -- within a few of scipy's own roundings, not bit for
    bit; samples before the first and behind the last valid one are extrapolated with the end pieces.  The valid samples
    of a row are compacted by rank, the tridiagonal system of a row is solved in LDS, in chunks of SPLINE_CHUNK knots
    for a longer row.  A row without a NaN is returned as it is; a row with a NaN and fewer than 3 ('quadratic') or 4
    ('cubic') valid samples raises scipy's ValueError, after one read-back of the smallest count.  Another method name
    is a ValueError, a host array a TypeError.  interp_NAN and interp_nan_batch do not route here."""
    import torch
    from . import _lib
    kind = _spline_kind(method, "interp_nan_spline_batch")
    if not ragged.is_device_tensor(x):
        raise TypeError("interp_nan_spline_batch takes a CUDA(HIP) tensor")
    squeeze = x.dim() == 1
    xs = x.unsqueeze(0) if squeeze else x
    if xs.dim() != 2:
        raise ValueError("x must be [n] or [rows, n]")
    if not xs.is_floating_point():
        raise TypeError("x must be a floating-point tensor")
    rows, n = xs.shape
    if rows == 0 or n == 0:
        return x.clone()
    xd = xs.to(torch.float64)
    if xd.stride(1) != 1 or xd.stride(0) < n:
        xd = xd.contiguous()
    fewest = int((~torch.isnan(xd)).sum(dim=1).min())   # the one read-back: what scipy would raise for
    if fewest == n:
        return x.clone()
    _spline_refuse(kind, fewest)
    y = torch.empty((rows, n), dtype=torch.float64, device=xd.device)
    lib = _lib.load()
    with torch.cuda.device(xd.device):
        ws = torch.empty(int(lib.mm_interp_spline_workspace_bytes(kind, rows, n)), dtype=torch.uint8, device=xd.device)
        _lib.check(lib.mm_interp_spline_f64(kind, xd.data_ptr(), rows, n, ragged.row_pitch(xd), y.data_ptr(), n, ws.data_ptr(),
                                            ws.numel(), C.c_void_p(torch.cuda.current_stream(xd.device).cuda_stream)),
                   "mm_interp_spline_f64")
    y = y.to(x.dtype)
    return y[0] if squeeze else y


def interp_nan_spline_ragged_batch(x, counts, method: str = "cubic"):
    """interp_nan_spline_batch with a count per row: ``x`` [rows, n_max] on the device, ``counts`` [rows] (host integers,
    validated: ValueError outside [1, n_max]; or an int64 device tensor, clamped by the kernels) -> [rows, n_max] of x's
    dtype.  Row b holds interp_nan_spline_batch(x[b, :counts[b]], method) in the columns [0, counts[b]), bit for bit, and
    zeros behind them; what x holds behind a row's count never matters.  The errors are interp_nan_spline_batch's, taken
    from the smallest number of valid samples below a row's count, in one read-back."""
    import torch
    from . import _lib
    kind = _spline_kind(method, "interp_nan_spline_ragged_batch")
    xd = ragged.device_rows(x, (torch.float64,), "interp_nan_spline_ragged_batch takes a CUDA(HIP) tensor",
                            "x must be [rows, n_max]", widen=torch.float64, nonempty=False)
    if not x.is_floating_point():
        raise TypeError("x must be a floating-point tensor")
    rows, n = x.shape
    if rows == 0 or n == 0:
        return x.clone()
    dev = x.device
    cnt = ragged.check_counts(counts, rows, n, dev, "counts")
    with torch.cuda.device(dev):
        cd = ragged.counts_on_device(cnt, dev)
        c = cd.clamp(1, n)
        valid = ((~torch.isnan(xd)) & (torch.arange(n, device=dev)[None, :] < c[:, None])).sum(dim=1)
        # a row without a NaN below its count is returned as it is, however few samples it has
        _spline_refuse(kind, int(torch.where(valid < c, valid, torch.full_like(valid, kind + 1)).min()))
        y = torch.empty((rows, n), dtype=torch.float64, device=dev)
        lib = _lib.load()
        ws = torch.empty(int(lib.mm_interp_spline_workspace_bytes(kind, rows, n)), dtype=torch.uint8, device=dev)
        _lib.check(lib.mm_interp_spline_ragged_f64(kind, xd.data_ptr(), rows, n, ragged.row_pitch(xd), cd.data_ptr(),
                                                   y.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "mm_interp_spline_ragged_f64")
    return y.to(x.dtype)


def interp_NAN(X, method: str = "linear"):
    """script/calc.py:345-385: NaN samples of a curve filled by interpolation.  'linear' (scipy interp1d, extrapolated at
    the ends) runs on the device (mm_interp_nan_linear_f64) for numpy curves and CUDA(HIP) tensors ([n] or [rows, n]).
    A CUDA(HIP) tensor stays on the device for 'pchip' (PchipInterpolator after the reference's end fix), 'nearest',
    'nearest-up', 'previous', 'next', 'zero' and 'slinear' too (interp_nan_batch, mm_interp_nan_f64); only 'quadratic' and
    'cubic', which solve a banded system over all knots, take a device tensor through scipy on the host and back.  A
    numpy curve with any method but 'linear' runs the reference's own scipy calls.  On the device a row without a valid
    sample raises IndexError under 'pchip' and scipy's ValueError for empty input otherwise; 'linear' and 'slinear' need
    two valid samples (ValueError)."""
    if method == "linear":
        if ragged.is_device_tensor(X):
            return _interp_linear_device(X)
        a = np.asarray(X)
        if np.sum(np.isnan(a)) == 0:
            return a.copy()
        import torch
        y = _interp_linear_device(torch.from_numpy(np.ascontiguousarray(a)).to(_gpu()))
        return y.cpu().numpy()
    if ragged.is_device_tensor(X):
        if method in _INTERP_KINDS:
            return _interp_kind_device(X, method)
        import torch
        rows = X.cpu().numpy()
        out = _interp_nan_host(rows, method) if rows.ndim == 1 else np.stack([_interp_nan_host(r, method) for r in rows])
        return torch.from_numpy(np.ascontiguousarray(out)).to(X.device)
    return _interp_nan_host(X, method)


_MSG_GAPS = inspect.cleandoc("""Post processing filters should be applied (outFiltes is not None) \
        but unvoiced regions are not interpolated (interpUnvoiced is None).
        Cannot filter f0 signal with gaps due to unvoiced regions""")


def _pyin_keywords(a):
    """The arguments of get_f0 / get_f0_batch (their locals()) -> the keywords of their pyin_batch / pyin_ragged_batch
    calls, after get_f0's refusals."""
    if (a["interpUnvoiced"] is None) & (a["outFilter"] is not None):
        raise Exception(_MSG_GAPS)
    if a["method"] in ("praatac", "praatcc"):
        raise NotImplementedError(f"method={a['method']!r} calls Praat through parselmouth; not part of this build")
    if a["method"] != "pyin":
        raise UnboundLocalError(f"get_f0: unknown method {a['method']!r}")     # reference: f0 unbound
    return dict(sr=a["sr"], frame_length=a["pyinframe_length"], win_length=a["pyinwin_length"],
                hop_length=int(a["hopSize"] * a["sr"]), n_thresholds=a["n_thresholds"], beta_parameters=a["beta_parameters"],
                boltzmann_parameter=a["boltzmann_parameter"], resolution=a["resolution"],
                max_transition_rate=a["max_transition_rate"], switch_prob=a["switch_prob"],
                no_trough_prob=a["no_trough_prob"], fill_na=a["pyinfill_na"], center=a["pyincenter"], pad_mode=a["pyinpad_mode"])


def get_f0(x, sr: float, method: str = "praatac", hopSize: float = 0.01, minPitch: float = 75, maxPitch: float = 600,
           interpUnvoiced="linear", outFilter="iir", outFiltType: str = "low", outFiltCutOff=[None],
           outFiltLen: int = 6, outFiltPolyOrd: int = 3, minMaxQuant=None, maxCandNum: int = 15,
           veryAccurate: bool = False, silenceThresh: float = 0.03, voicingThresh: float = 0.45,
           octaveCost: float = 0.01, octaveJumpCost: float = 0.35, voicedUnvoicedCost: float = 0.14,
           pyinframe_length: int = 2048, pyinwin_length: int = None, n_thresholds: int = 100,
           beta_parameters: tuple = (2, 18), boltzmann_parameter: int = 2, resolution: float = 0.1,
           max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01,
           pyinfill_na: float = np.nan, pyincenter: bool = True, pyinpad_mode: str = "constant"):
    """script/calc.py:386-592 -> (f0, f0t).  method='pyin' runs librosa.pyin's arithmetic on the GPU (pyin_batch), the
    minMaxQuant second pass with its quantiles taken on the host as the reference does, then interp_NAN and applyFilter.
    The curve stays on the device between them for interpUnvoiced 'linear', 'pchip', 'nearest', 'nearest-up', 'previous',
    'next', 'zero' and 'slinear' (interp_NAN); 'quadratic' and 'cubic' go through scipy on the host.
    A numpy signal returns numpy arrays; a CUDA(HIP) tensor [n] returns f0 as a device tensor (filtered on the device)
    and f0t as numpy, like calculate_amplitude_envelope.  'praatac' / 'praatcc' call Praat (parselmouth): not part of
    this package."""
    kw = _pyin_keywords(locals())
    on_device = ragged.is_device_tensor(x)
    xd = x if on_device else _to_device_signal(x)
    f0, _voiced, _vprob = pyin_batch(xd, fmin=minPitch, fmax=maxPitch, **kw)
    if minMaxQuant is not None:
        h = f0.cpu().numpy()
        h = h[np.isnan(h) == 0]
        quants = np.quantile(h, [minMaxQuant[0], minMaxQuant[1]])
        f0, _voiced, _vprob = pyin_batch(xd, fmin=quants[0], fmax=quants[1], **kw)
    f0t = np.arange(f0.shape[-1]) * hopSize
    if interpUnvoiced is not None:
        f0 = interp_NAN(f0, interpUnvoiced)
    if outFilter is not None:
        f0 = applyFilter(f0, 1 / hopSize, filt=outFilter, cutOff=outFiltCutOff, filtLen=outFiltLen, filtType=outFiltType,
                         polyOrd=outFiltPolyOrd)
    if not on_device:
        f0 = f0.cpu().numpy()
    return f0, f0t


def get_f0_batch(clips, sr: float, method: str = "praatac", hopSize: float = 0.01, minPitch: float = 75,
                 maxPitch: float = 600, interpUnvoiced="linear", outFilter="iir", outFiltType: str = "low",
                 outFiltCutOff=[None], outFiltLen: int = 6, outFiltPolyOrd: int = 3, minMaxQuant=None, maxCandNum: int = 15,
                 veryAccurate: bool = False, silenceThresh: float = 0.03, voicingThresh: float = 0.45,
                 octaveCost: float = 0.01, octaveJumpCost: float = 0.35, voicedUnvoicedCost: float = 0.14,
                 pyinframe_length: int = 2048, pyinwin_length: int = None, n_thresholds: int = 100,
                 beta_parameters: tuple = (2, 18), boltzmann_parameter: int = 2, resolution: float = 0.1,
                 max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01,
                 pyinfill_na: float = np.nan, pyincenter: bool = True, pyinpad_mode: str = "constant"):
    """``get_f0`` for a list of clips of any lengths -> a list of ``(f0, f0t)``, one per clip, each what ``get_f0`` returns
    for that clip alone: a numpy pair for a numpy clip, a device tensor and a numpy ``f0t`` for a CUDA(HIP) clip [n].

    The float32 clips and the others (float64; integer PCM becomes float64) form one padded batch each, so every clip keeps
    the precision it has alone, and run through pyin_ragged_batch.  ``interpUnvoiced`` runs ragged on the device
    (interp_nan_ragged_batch; 'quadratic' and 'cubic' per clip through scipy, as interp_NAN does).  ``outFilter`` is
    ONE ragged call on the padded curves with their frame counts (filters.apply_filter_ragged_batch: every row what
    applyFilter gives for the row alone, bit for bit; only 'iir' filters of more than 4 sections, which have no ragged
    kernel, still loop over the distinct frame counts there).  ``minMaxQuant``: the first pass
    is ragged; the second has its own fmin / fmax, and with them its own pitch bins and transition band, per clip, so it
    runs pyin_batch clip by clip.  The errors are get_f0's, with the clip's index appended where one clip is at fault."""
    kw = _pyin_keywords(locals())
    clips = list(clips)
    on_device = [ragged.is_device_tensor(c) for c in clips]
    sigs = [c if d else _to_device_signal(c) for c, d in zip(clips, on_device)]
    for i, s in enumerate(sigs):
        if s.dim() != 1:
            raise ragged.named(ValueError("audio must be [n]"), i)
        if s.shape[0] < 1 or pyin_ragged_frames([s.shape[0]], pyinframe_length, max(kw["hop_length"], 1), pyincenter)[0] < 1:
            raise ragged.named(ValueError(_MSG_SHORT.format(s.shape[0], pyinframe_length)), i)
    out = [None] * len(clips)
    for idx, audio, lengths in ragged.packed_groups(sigs):      # (integer PCM: converted to float64 on the copy)
        f0 = pyin_ragged_batch(audio, lengths, fmin=minPitch, fmax=maxPitch, **kw)[0]
        frames = pyin_ragged_frames(lengths, pyinframe_length, kw["hop_length"], pyincenter)
        if minMaxQuant is not None:
            first = f0.cpu().numpy()
            for b, i in enumerate(idx):
                h = first[b, :frames[b]]
                h = h[np.isnan(h) == 0]
                try:
                    quants = np.quantile(h, [minMaxQuant[0], minMaxQuant[1]])
                    f0[b, :frames[b]] = pyin_batch(audio[b, :lengths[b]], fmin=quants[0], fmax=quants[1], **kw)[0]
                except (ValueError, IndexError, NotImplementedError) as e:
                    raise ragged.named(e, i)
        if interpUnvoiced is not None:
            if interpUnvoiced == "linear" or interpUnvoiced in _INTERP_KINDS:
                try:
                    f0 = interp_nan_ragged_batch(f0, frames, interpUnvoiced)
                except (ValueError, IndexError) as e:
                    ragged.blame_clip(e, lambda b: interp_NAN(f0[b, :frames[b]], interpUnvoiced), idx)
            else:
                for b, i in enumerate(idx):
                    try:
                        f0[b, :frames[b]] = interp_NAN(f0[b, :frames[b]], interpUnvoiced)
                    except (ValueError, IndexError) as e:
                        raise ragged.named(e, i)
        if outFilter is not None:
            try:
                f0 = apply_filter_ragged_batch(f0, frames, 1 / hopSize, filt=outFilter, cutOff=outFiltCutOff,
                                               filtLen=outFiltLen, filtType=outFiltType, polyOrd=outFiltPolyOrd)
            except ragged.RowRefused as e:                                # (too few frames for the filter)
                raise ragged.named(e, idx[e.row])
        for b, i in enumerate(idx):
            f = f0[b, :frames[b]]
            out[i] = (f.clone() if on_device[i] else f.cpu().numpy(), np.arange(int(frames[b])) * hopSize)
    return out
