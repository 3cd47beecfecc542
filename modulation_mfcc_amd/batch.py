"""Batched entry points (new in the build; the reference processes one clip per call from the
GUI thread, script/main.py:750-769).  All tensors are float32 / complex64 on the GPU.
"""
from __future__ import annotations

from . import ragged
from .plan import MfccConfig, get_plan


def mfcc_batch(audio, cfg: MfccConfig, out=None):
    """[B, n] device tensor -> MFCC [B, n_mfcc, T]; per clip identical to librosa.feature.mfcc
    as called at script/mfcc.py:387."""
    return get_plan(cfg).mfcc(audio, out=out)


def modspec_batch(mfcc, cfg: MfccConfig, out=None):
    """[B, n_mfcc, T] -> complex64 [B, n_mfcc, n_mod/2+1]: rFFT of every coefficient trajectory,
    zero-padded to n_mod (build-defined)."""
    return get_plan(cfg).modspec(mfcc, out=out)


def mfcc_modspec_batch(audio, cfg: MfccConfig, mfcc_out=None, mod_out=None):
    """The whole hot path: MFCC and its modulation spectrum."""
    return get_plan(cfg).mfcc_modspec(audio, out=mfcc_out, out_mod=mod_out)     # one launch where the plan can


def mfcc_ragged_batch(audio, lengths, cfg: MfccConfig, out=None):
    """Padded batch [B, n_max] + one length per clip -> (MFCC [B, n_mfcc, T_max], frames [B]): every clip's MFCC as
    mfcc_batch gives it for that clip alone in the columns [0, frames[b]), zeros behind them; what the padding holds
    (zeros, NaN, another clip) never matters.  See MfccPlan.mfcc_ragged."""
    return get_plan(cfg).mfcc_ragged(audio, lengths, out=out)


def mfcc_modspec_ragged_batch(audio, lengths, cfg: MfccConfig, mfcc_out=None, mod_out=None):
    """mfcc_ragged_batch and the modulation spectrum of every clip's own frames on the batch's one modulation-frequency
    axis -> (MFCC, spectrum complex64 [B, n_mfcc, n_mod/2+1], frames)."""
    return get_plan(cfg).mfcc_modspec_ragged(audio, lengths, out=mfcc_out, out_mod=mod_out)


def mfcc_modpsd_batch(audio, cfg: MfccConfig, **welch):
    """[B, n] device tensor -> (MFCC [B, n_mfcc, T], f [bins] numpy, Pxx [B, n_mfcc, bins]): the MFCC and the Welch modulation
    power spectrum of every coefficient trajectory (scipy.signal.welch at fs = sr / hop_length; the keywords of
    modpsd.modulation_psd_batch).  See MfccPlan.mfcc_modpsd."""
    return get_plan(cfg).mfcc_modpsd(audio, **welch)


def mfcc_modpsd_ragged_batch(audio, lengths, cfg: MfccConfig, **welch):
    """mfcc_modpsd_batch for a padded batch [B, n_max] + one length per clip: every clip's spectrum is that of the clip
    alone, all on one frequency grid."""
    return get_plan(cfg).mfcc_modpsd(audio, lengths, **welch)


def mfcc_modcsd_batch(audio, ref, cfg: MfccConfig, **welch):
    """[B, n] device tensor and one reference curve per clip on the frame grid, ``ref`` [B, T] (e.g. rms_batch at the
    configuration's hop) -> (MFCC [B, n_mfcc, T], f [bins] numpy, Pxx, Pyy, Pxy complex64, Cxy, each [B, n_mfcc, bins]): the
    Welch auto spectra, cross spectrum and coherence of every coefficient trajectory against its clip's curve
    (scipy.signal.welch / csd / coherence at fs = sr / hop_length; the keywords of
    modcsd.modulation_cross_spectra_batch).  See MfccPlan.mfcc_modcsd."""
    return get_plan(cfg).mfcc_modcsd(audio, ref, **welch)


def mfcc_modcsd_ragged_batch(audio, ref, lengths, cfg: MfccConfig, **welch):
    """mfcc_modcsd_batch for a padded batch [B, n_max] + one length per clip: every clip's spectra are those of the clip
    alone, all on one frequency grid."""
    return get_plan(cfg).mfcc_modcsd(audio, ref, lengths, **welch)


def mfcc_change_ragged_batch(audio, lengths, cfg: MfccConfig, *, tStep=None, **tail):
    """Padded batch [B, n_max] + one length per clip -> (change [B, T_max] float64, frames [B] int64 on the device): the
    amount-of-change curve of every clip as get_MFCCS_change computes it for that clip alone, in the columns
    [0, frames[b]), zeros behind them.  mfcc_ragged_batch followed by the ragged change tail
    (tail.mfcc_change_ragged_device, whose keywords -- removeFirst, filtCutoff, filtOrd, diffMethod, outFilter, ... -- pass
    through; tStep defaults to the configuration's hop_length / sr); nothing leaves the device.  Host `lengths` are
    validated on the host: a clip with too few frames for the filters raises scipy's ValueError (device lengths: NaN)."""
    from . import tail as _tail
    plan = get_plan(cfg)
    if tStep is None:
        tStep = cfg.hop_length / cfg.sr
    mfcc, frames = plan.mfcc_ragged(audio, lengths)
    fr = frames
    if not ragged.is_device_tensor(lengths):        # host lengths: host frame counts, validated by the tail
        fr = ragged.stft_frames(lengths, cfg.n_fft, cfg.hop_length)
    return _tail.mfcc_change_ragged_device(plan, mfcc, fr, tStep=tStep, **tail), frames


def pack_clips(clips, dtype=None):
    """A list of 1-D float32 tensors (one device) -> (audio [B, n_max] on that device, lengths int64 [B] on the host) for
    the ragged calls.  The padding behind each clip is left as allocated: the ragged calls never read it into a result.
    ``dtype``: another type the clips all have (torch.float64: the double-precision Hilbert envelope)."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    clips = list(clips)
    if not clips:
        raise ValueError("pack_clips: no clips")
    for c in clips:
        if not (isinstance(c, torch.Tensor) and c.dtype == dtype and c.dim() == 1):
            raise TypeError(f"pack_clips: every clip must be a 1-D {str(dtype).replace('torch.', '')} tensor")
        if c.device != clips[0].device:
            raise ValueError(f"pack_clips: clips on {clips[0].device} and {c.device}")
        if c.shape[0] < 1:
            raise ValueError("pack_clips: empty clip")
    audio, lengths = ragged.pack(clips, dtype)
    return audio, torch.from_numpy(lengths)


def rfft_batch(rows, n: int, cfg: MfccConfig = None, out=None):
    """Stage-isolated batched rFFT (the kernel the '% HBM roofline (rFFT)' metric is quoted on)."""
    return get_plan(cfg or MfccConfig()).rfft(rows, n, out=out)


def _rms(audio, pitch, frame_length, hop_length, center, n_out, d_lens=None):
    """mm_rms_f32 (``d_lens`` None) or mm_rms_ragged_f32 on checked rows [B, n] -> [B, n_out] float32."""
    import torch
    from . import _lib
    B, n = audio.shape
    out = torch.empty((B, n_out), dtype=torch.float32, device=audio.device)
    _lib.call("mm_rms_f32" if d_lens is None else "mm_rms_ragged_f32", audio.device, audio.data_ptr(), B, n, pitch,
              *ragged.lens_arg(d_lens), frame_length, hop_length, center, out.data_ptr())
    return out


def _rms_frames(n, frame_length, hop_length, center):
    from . import _lib
    n_out = _lib.load().mm_rms_num_frames(n, frame_length, hop_length, center)
    if n_out < 0:
        _lib.check(int(n_out), "mm_rms_num_frames")
    return n_out


def rms_batch(audio, frame_length: int, hop_length: int, center: bool = True):
    """Framewise RMS on the device (row N3): [B, n] float32 CUDA(HIP) tensor -> [B, n_out], equal to
    librosa.feature.rms(y, frame_length=..., hop_length=..., center=..., pad_mode='constant') per
    clip (script/calc.py:331)."""
    import torch
    if not (ragged.is_device_tensor(audio) and audio.dtype == torch.float32):
        raise TypeError("audio must be a float32 CUDA(HIP) tensor")
    audio, _ = ragged.batch_rows(audio, "audio must be [n] or [B, n]")
    frame_length, hop_length, center = int(frame_length), int(hop_length), 1 if center else 0
    n_out = _rms_frames(audio.shape[1], frame_length, hop_length, center)
    return _rms(audio, audio.stride(0), frame_length, hop_length, center, n_out)


rms_ragged_frames = ragged.centered_frames      # RMS frames of clips of ``lengths`` samples: mm_rms_num_frames per clip


def rms_ragged_batch(audio, lengths, frame_length: int, hop_length: int, center: bool = True):
    """rms_batch for clips of different lengths in one padded batch (mm_rms_ragged_f32): ``audio`` [B, n_max] float32 on the
    device and one valid sample count per clip -> [B, t_max] float32, t_max the frames of n_max.  Row b holds, in its first
    rms_ragged_frames(lengths[b]) columns, rms_batch(audio[b, :lengths[b]]) bit for bit -- the clip's own centre padding,
    zeros for everything behind its end -- and +0.0 behind them; what the padding of ``audio`` holds never matters.

    ``lengths``: host integers (validated: ValueError outside [1, n_max], and for a clip shorter than the frame without
    centring, the clip named) or an int64 device tensor (no read-back; the kernels clamp it, and a clip without a frame gets
    a NaN row).  One launch, that of n_max."""
    import torch
    audio = ragged.device_rows(audio, (torch.float32,), "audio must be a float32 CUDA(HIP) tensor", "audio must be [B, n_max]",
                               nonempty=False)
    B, n = audio.shape
    lens = ragged.check_lengths(lengths, B, n, audio.device)
    frame_length, hop_length, center = int(frame_length), int(hop_length), 1 if center else 0
    t_max = _rms_frames(n, frame_length, hop_length, center)
    ragged.refuse_short(lens, n, 1 if center else frame_length,
                        lambda short: f"rms: a clip of {short} samples is shorter than frame_length={frame_length}", "clip", None)
    return _rms(audio, ragged.row_pitch(audio), frame_length, hop_length, center, t_max,
                ragged.counts_on_device(lens, audio.device))
