"""Drop-in for the numeric functions of the reference's ``script/mfcc.py``.

Same names, argument meaning, positional-only / keyword-only split, return values and error
behaviour as the reference (script/mfcc.py:29-39, 262-264, 291-311), so the Qt UI's call sites
(script/main.py:750-769, 1049-1066) work unchanged after ``from modulation_mfcc_amd.mfcc import
get_MFCCS_change, load_channel``.  The librosa.feature.mfcc call at script/mfcc.py:387 is replaced
by the HIP path (``MfccPlan.mfcc`` -> libmodmfcc.so); there is no CPU fallback for it.

Host side, as in the reference: filter DESIGN (scipy.signal.butter / firwin) and the 'fir' branch of
applyFilter (a scipy call in the reference too).  The MFCC-change tail (script/mfcc.py:392-427) is in
``tail.py``, the input side (WAVE decode + resampling, script/mfcc.py:284,373) in ``audio_io.py``.
"""
from __future__ import annotations

import numpy as np

from . import filters as _filters
from . import tail as _tail
from .plan import MfccConfig, get_plan

__all__ = ["applyFilter", "get_amplitude", "get_amplitude_batch", "load_channel", "get_MFCCS_change", "get_MFCCS_change_batch", "mfcc_array"]

applyFilter = _filters.applyFilter


def _load_audio_device(path, sr):
    """librosa.load(path, sr=sr, mono=False) (script/mfcc.py:284,373) for WAVE files, on the device: float32
    CUDA(HIP) tensor, [n] for a mono file and [channels, n] otherwise -- RIFF header parsed on the host, PCM
    decode and sample-rate conversion by the kernels of row N4 (modulation_mfcc_amd/audio_io.py, which also
    states how the resampler relates to librosa's soxr_hq)."""
    from .audio_io import load_audio
    x = load_audio(path, sr)
    return x[0] if x.shape[0] == 1 else x


def _load_audio(path, sr):
    """Same, as the numpy array the reference's callers get."""
    return _load_audio_device(path, sr).cpu().numpy()


def load_channel(file_path: str, signal_sample_rate: float = 10_000, channel_nb: int = 0):
    """script/mfcc.py:262-289: every channel of the file at ``signal_sample_rate`` (the reference
    ignores ``channel_nb`` as well -- its channel pick is commented out)."""
    return _load_audio(file_path, signal_sample_rate)


def mfcc_array(y, cfg: MfccConfig) -> np.ndarray:
    """One clip through the HIP path: numpy [n] -> float32 [n_mfcc, T] (== librosa.feature.mfcc)."""
    import torch
    y = np.ascontiguousarray(np.asarray(y), dtype=np.float32)
    if y.ndim != 1:
        raise ValueError("expected a 1-D signal")
    plan = get_plan(cfg)
    d = torch.from_numpy(y).to(plan.device)
    return plan.mfcc(d)[0].cpu().numpy()


def get_amplitude(x, sr, /, *, method: str = "RMS", winLen: float = 0.1, hopLen: float = 0.01,
                  center: bool = True, outFilter=None, outFiltType: str = "low",
                  outFiltCutOff=[12], outFiltLen: int = 6, outFiltPolyOrd: int = 3):
    """script/mfcc.py:137-259 -- same function as calc.calculate_amplitude_envelope."""
    from .calc import calculate_amplitude_envelope
    return calculate_amplitude_envelope(x, sr, method=method, winLen=winLen, hopLen=hopLen,
                                        center=center, outFilter=outFilter, outFiltType=outFiltType,
                                        outFiltCutOff=outFiltCutOff, outFiltLen=outFiltLen,
                                        outFiltPolyOrd=outFiltPolyOrd)


def get_amplitude_batch(clips, sr, /, **kw):
    """get_amplitude for a list of clips of any lengths -- same function as calc.calculate_amplitude_envelope_batch."""
    from .calc import calculate_amplitude_envelope_batch
    return calculate_amplitude_envelope_batch(clips, sr, **kw)


def _signal_row(clip, sigSr, channelN, device=None):
    """The signal of get_MFCCS_change and its list form: a path is loaded on the device (it never leaves the GPU), a
    [channels, n] array gives its channel ``channelN``; with ``device`` the row is brought there as the float32 [n] the
    MFCC kernels take (arrays of any float dtype are cast)."""
    signal = _load_audio_device(clip, sigSr) if isinstance(clip, str) else clip
    if signal.ndim > 1:
        signal = signal[channelN, :]
    if device is None:
        return signal
    import torch
    if isinstance(signal, torch.Tensor):
        y = signal.to(device=device, dtype=torch.float32)
    else:
        y = torch.from_numpy(np.ascontiguousarray(np.asarray(signal), dtype=np.float32)).to(device)
    if y.dim() != 1:
        raise ValueError("expected a 1-D signal")
    return y


def get_MFCCS_change(audioIn, sigSr, /, *, channelN: int = 0, tStep: float = 0.001,
                     winLen: float = 0.025, n_mfcc: int = 13, n_fft: int = 512, minFreq: int = 100,
                     maxFreq: int = 10000, removeFirst: int = 1, filtCutoff: int = 12,
                     filtOrd: int = 6, diffMethod: str = "grad", outFilter: str = "iir",
                     outFiltType: str = "low", outFiltCutOff=[None], outFiltLen: int = 6,
                     outFiltPolyOrd: int = 3):
    """Amount of change in the MFCCs over time -- script/mfcc.py:291-427.

    ``audioIn`` is a path or an array ([n] or [channels, n]); returns ``(totChange, T)``: the
    change curve and the time anchor of every frame, as the reference does.  The MFCCs come from
    the HIP kernels (float32 arithmetic; arrays of any float dtype are cast to float32).
    """
    signal = _signal_row(audioIn, sigSr, channelN)
    cfg = MfccConfig.from_reference_call(sigSr, tStep=tStep, winLen=winLen, n_mfcc=n_mfcc,
                                         n_fft=n_fft, minFreq=minFreq, maxFreq=maxFreq)
    if _tail.device_path_applies(diffMethod, outFilter):
        plan = get_plan(cfg)
        coeffs_dev = plan.mfcc(_signal_row(signal, sigSr, channelN, plan.device))
        anchors = _tail.time_anchors(coeffs_dev.shape[2], tStep, winLen)
        change = _tail.mfcc_change_device(plan, coeffs_dev, tStep=tStep, removeFirst=removeFirst,
                                          filtCutoff=filtCutoff, filtOrd=filtOrd, diffMethod=diffMethod,
                                          outFilter=outFilter,
                                          outFiltType=outFiltType, outFiltCutOff=outFiltCutOff,
                                          outFiltLen=outFiltLen, outFiltPolyOrd=outFiltPolyOrd)[0].cpu().numpy()
        return change, anchors
    coeffs = mfcc_array(signal.cpu().numpy() if hasattr(signal, "is_cuda") else signal, cfg)
    anchors = _tail.time_anchors(coeffs.shape[1], tStep, winLen)
    change = _tail.mfcc_change(coeffs, tStep=tStep, removeFirst=removeFirst, filtCutoff=filtCutoff,
                               filtOrd=filtOrd, diffMethod=diffMethod, outFilter=outFilter,
                               outFiltType=outFiltType, outFiltCutOff=outFiltCutOff,
                               outFiltLen=outFiltLen, outFiltPolyOrd=outFiltPolyOrd)
    return change, anchors


def get_MFCCS_change_batch(clips, sigSr, /, *, channelN: int = 0, tStep: float = 0.001,
                           winLen: float = 0.025, n_mfcc: int = 13, n_fft: int = 512, minFreq: int = 100,
                           maxFreq: int = 10000, removeFirst: int = 1, filtCutoff: int = 12,
                           filtOrd: int = 6, diffMethod: str = "grad", outFilter: str = "iir",
                           outFiltType: str = "low", outFiltCutOff=[None], outFiltLen: int = 6,
                           outFiltPolyOrd: int = 3):
    """``get_MFCCS_change`` for a list of clips of any lengths -> a list of ``(totChange, T)`` numpy pairs, one per clip,
    each what ``get_MFCCS_change`` returns for that clip alone (its own last frame, its own time anchors).

    ``clips``: paths, arrays or device tensors ([n] or [channels, n]; ``channelN`` picks as in the single call).  The
    clips are packed into one padded batch (``pack_clips``; a list of paths only is decoded and resampled as one batch by
    ``audio_io.load_audio_batch``) and run through the ragged MFCC and the ragged change tail in
    a few launches (``mfcc_change_ragged_batch``); one copy brings the curves back.  A clip with too few frames for the
    filters raises scipy's ValueError, as the single call does, with the clip's index in the message.
    """
    kw = dict(channelN=channelN, tStep=tStep, winLen=winLen, n_mfcc=n_mfcc, n_fft=n_fft, minFreq=minFreq, maxFreq=maxFreq,
              removeFirst=removeFirst, filtCutoff=filtCutoff, filtOrd=filtOrd, diffMethod=diffMethod, outFilter=outFilter,
              outFiltType=outFiltType, outFiltCutOff=outFiltCutOff, outFiltLen=outFiltLen, outFiltPolyOrd=outFiltPolyOrd)
    clips = list(clips)
    if not _tail.device_path_applies(diffMethod, outFilter) or not clips:
        return [get_MFCCS_change(c, sigSr, **kw) for c in clips]       # (an output filter applyFilter refuses: its own error)
    from .batch import mfcc_change_ragged_batch, pack_clips
    cfg = MfccConfig.from_reference_call(sigSr, tStep=tStep, winLen=winLen, n_mfcc=n_mfcc,
                                         n_fft=n_fft, minFreq=minFreq, maxFreq=maxFreq)
    plan = get_plan(cfg)
    if all(isinstance(c, str) for c in clips):
        # a list of files: one decode launch and one ragged resample per source rate instead of a load per file; the
        # rows are bit for bit those of the route below (audio_io.load_audio_batch)
        import torch
        from .audio_io import load_audio_batch
        audio, lengths = load_audio_batch(clips, sigSr, channel=channelN, device=plan.device)
        lengths = torch.from_numpy(lengths)
    else:
        audio, lengths = pack_clips([_signal_row(c, sigSr, channelN, plan.device) for c in clips])
    change, _ =mfcc_change_ragged_batch(audio, lengths, cfg, tStep=tStep, removeFirst=removeFirst, filtCutoff=filtCutoff,
                                         filtOrd=filtOrd, diffMethod=diffMethod, outFilter=outFilter,
                                         outFiltType=outFiltType, outFiltCutOff=outFiltCutOff, outFiltLen=outFiltLen,
                                         outFiltPolyOrd=outFiltPolyOrd)
    change = change.cpu().numpy()
    frames = [cfg.num_frames(int(n)) for n in lengths]
    return [(change[b, :T].copy(), _tail.time_anchors(T, tStep, winLen)) for b, T in enumerate(frames)]
