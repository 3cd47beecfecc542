"""pYIN f0 tracking on the GPU: librosa.pyin as the reference's ``get_f0(method='pyin')`` calls it
(script/calc.py:386-592).

    pyin_batch(audio [B, n] | [n] device tensor, sr, fmin=, fmax=, ...)  -> (f0, voiced_flag, voiced_prob) on the device
    pyin_ragged_batch(audio [B, n_max], lengths [B], sr, ...)             -> the same with a length per clip (+ frames [B])
    get_f0_batch(clips, sr, method='pyin', ...)                           -> [(f0, f0t), ...]: get_f0 of a list of clips
    pyin(y, fmin=, fmax=, sr=22050, ...)                                  -> librosa.pyin's signature: numpy in, numpy out
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

from . import ragged
from .filters import applyFilter, apply_filter_ragged_batch
from .interp import _INTERP_KINDS, interp_NAN, interp_nan_ragged_batch
# gap filling lived in this module before interp.py: its names stay importable from here
from .interp import (INTERP_SEGMENT, SPLINE_CHUNK, _INTERP_HOST_KINDS, _SPLINE_KINDS, _interp_nan_host,  # noqa: F401
                     _spline_refuse, interp_nan_batch, interp_nan_spline_batch, interp_nan_spline_ragged_batch)

__all__ = ["pyin_batch", "pyin_ragged_batch", "pyin_ragged_frames", "pyin", "interp_NAN", "interp_nan_batch",
           "interp_nan_ragged_batch", "interp_nan_spline_batch", "interp_nan_spline_ragged_batch", "get_f0", "get_f0_batch",
           "pyin_sizes", "beta_tables", "boltzmann_table", "transition_matrix", "banded_log_transitions", "pitch_freqs",
           "pyin_params", "pyin_cmnd", "pyin_records"]

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
    x, squeeze = _as_signal(audio)
    if center and pad_mode != "constant":
        x = _pad_center(x, frame_length, pad_mode)
        center = False
    B, n = x.shape
    p, z = pyin_params(n, sr, fmin=fmin, fmax=fmax, frame_length=frame_length, win_length=win_length,
                       hop_length=hop_length, n_thresholds=n_thresholds, resolution=resolution,
                       max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob,
                       fill_na=fill_na, center=center)
    if z["n_frames"] < 1:
        raise ValueError(f"pyin: a signal of {n} samples is shorter than frame_length={frame_length}")
    tabs, f0, voiced, vprob, states, _ = _pyin(x, p, z, switch_prob, beta_parameters, boltzmann_parameter)
    if fill_na is None:                 # librosa keeps the decoded bin's frequency on unvoiced frames
        f0 = tabs.dev["freqs"][(states % z["n_bins"]).long()]
    out = (f0, voiced.bool(), vprob) + ((states,) if return_states else ())
    return tuple(o[0] for o in out) if squeeze else out


def _pyin(x, p, z, switch_prob, beta_parameters, boltzmann_parameter, d_lens=None):
    """mm_pyin_f32 / _f64 (``d_lens`` None) or their _ragged twins on checked rows [B, n] with validated parameters, in
    calls whose scratch stays within PYIN_WS_BYTES -> (the device tables, f0, voiced uint8, voiced_prob, states, each
    [B, n_frames], and the ragged entries' frames [B], else None)."""
    import torch
    from . import _lib
    lib = _lib.load()
    B, n = x.shape
    T, dev = z["n_frames"], x.device
    tabs = _tables(p, z, switch_prob, beta_parameters, boltzmann_parameter, dev)
    p.band_h = tabs.H
    f0 = torch.empty((B, T), dtype=torch.float64, device=dev)
    voiced = torch.empty((B, T), dtype=torch.uint8, device=dev)
    vprob = torch.empty((B, T), dtype=torch.float64, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    frames = None if d_lens is None else torch.empty(B, dtype=torch.int64, device=dev)
    form = "" if d_lens is None else "_ragged"
    need = getattr(lib, f"mm_pyin{form}_workspace_bytes")
    rows = B
    while rows > 1 and need(C.byref(p), rows, n) > PYIN_WS_BYTES:
        rows = max(1, min(rows - 1, rows * PYIN_WS_BYTES // need(C.byref(p), rows, n)))
    pitch = ragged.row_pitch(x)

    def args(r0, r):
        lens, counted = ((), ()) if d_lens is None else ((d_lens[r0:].data_ptr(),), (frames[r0:].data_ptr(),))
        return (C.byref(p), C.byref(tabs.c), x[r0].data_ptr(), r, n, pitch, *lens, f0[r0].data_ptr(), voiced[r0].data_ptr(),
                vprob[r0].data_ptr(), states[r0].data_ptr(), *counted)
    _lib.call_chunked(f"mm_pyin{form}_f32" if x.dtype == torch.float32 else f"mm_pyin{form}_f64", dev, B, rows, args,
                      lambda r: need(C.byref(p), r, n))
    return tabs, f0, voiced, vprob, states, frames


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
    if z["n_frames"] < 1:
        raise ValueError(_MSG_SHORT.format(n, frame_length))
    ragged.refuse_short(lens, n, 1 if center else frame_length, lambda short: _MSG_SHORT.format(short, frame_length), "clip", None)
    tabs, f0, voiced, vprob, states, frames = _pyin(x, p, z, switch_prob, beta_parameters, boltzmann_parameter,
                                                    ragged.counts_on_device(lens, x.device))
    if fill_na is None:                 # librosa keeps the decoded bin's frequency on unvoiced frames: of real frames only
        live = torch.arange(z["n_frames"], device=x.device)[None, :] < frames[:, None]
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
    _lib.call("mm_pyin_cmnd", x.device, C.byref(p), x.data_ptr(), 0 if x.dtype == torch.float32 else 1, B, n,
              ragged.row_pitch(x), out.data_ptr())
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
    _lib.call("mm_pyin_candidates", dev, C.byref(p), C.byref(tabs.c), c.data_ptr(), T, count.data_ptr(), bins.data_ptr(),
              probs.data_ptr(), vp.data_ptr())
    return count, bins, probs, vp


def _to_device_signal(y):
    """numpy -> device tensor: float32 and float64 keep their type, integer PCM (and anything else) becomes float64."""
    import torch
    a = np.asarray(y)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(ragged.gpu())


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
# get_f0 (script/calc.py:386-592)
# ---------------------------------------------------------------------------------------------------------------------
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
