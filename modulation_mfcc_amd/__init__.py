"""modulation_mfcc_amd -- MI355X-native MFCC + modulation-spectrum extractor.

Drop-in for the numeric hot path of aaron-randreth/modulation-mfcc (script/mfcc.py,
script/calc.py); Python host code over hand-written gfx950 HIP kernels (libmodmfcc.so, C ABI in
include/modmfcc.h).  torch is used for device buffers, streams and torch.distributed only.
"""
from .plan import MfccConfig, MfccPlan, get_plan, butter_sos  # noqa: F401
from .batch import mfcc_batch, modspec_batch, mfcc_modspec_batch, rfft_batch, rms_batch  # noqa: F401
from .batch import mfcc_ragged_batch, mfcc_modspec_ragged_batch, mfcc_change_ragged_batch, pack_clips  # noqa: F401
from .batch import rms_ragged_batch, rms_ragged_frames  # noqa: F401
from .batch import mfcc_modpsd_batch, mfcc_modpsd_ragged_batch  # noqa: F401
from .modpsd import modulation_psd_batch, modulation_psd_ragged_batch, modpsd_nfft, modpsd_segments  # noqa: F401
from .batch import mfcc_modcsd_batch, mfcc_modcsd_ragged_batch  # noqa: F401
from .modcsd import modulation_cross_spectra_batch, modulation_csd_batch, modulation_coherence_batch  # noqa: F401
from .modcsd import (modulation_cross_spectra_ragged_batch, modulation_csd_ragged_batch,  # noqa: F401
                     modulation_coherence_ragged_batch)
from .mfcc import get_MFCCS_change, get_MFCCS_change_batch, load_channel, applyFilter, get_amplitude  # noqa: F401
from .mfcc import get_amplitude_batch  # noqa: F401
from .calc import (get_velocity, calculate_amplitude_envelope, velocity_batch, amplitude_envelope_batch,  # noqa: F401
                   hilbert_envelope_batch, hilbert_envelope_ragged_batch, amplitude_envelope_ragged_batch,
                   calculate_amplitude_envelope_batch, find_peaks_batch, find_peaks_ex_batch,
                   peaks_to_list, MinMaxFinder)
from .filters import sosfiltfilt_batch, fir_filtfilt_batch, savgol_batch  # noqa: F401
from .filters import (sosfiltfilt_ragged_batch, fir_filtfilt_ragged_batch, savgol_ragged_batch,  # noqa: F401
                      apply_filter_ragged_batch, applyFilter_batch)
from .audio_io import load_audio, load_wav, resample_batch  # noqa: F401
from .audio_io import plan_wav_batch, load_wav_batch, resample_ragged_batch, load_audio_batch  # noqa: F401
from .pitch import pyin_batch, pyin, get_f0  # noqa: F401
from .pitch import pyin_ragged_batch, pyin_ragged_frames, get_f0_batch  # noqa: F401
from .interp import interp_NAN, interp_nan_batch, interp_nan_ragged_batch  # noqa: F401
from .interp import interp_nan_spline_batch, interp_nan_spline_ragged_batch  # noqa: F401
from .lomb import modulation_lombscargle_batch, modulation_lombscargle_ragged_batch, modulation_lombscargle_list  # noqa: F401
from .zoom import (zoom_batch, zoom_ragged_batch, spline_filter_batch, spectrogram_image,  # noqa: F401
                   spectrogram_image_batch)
from .pspec import (praat_spectrogram_params, praat_spectrogram_batch, praat_spectrogram_ragged_batch,  # noqa: F401
                    praat_spectrogram_list, Parselmouth, Sound, Spectrogram, spectrogram_view)
from .pint import (praat_intensity_params, praat_intensity_batch, praat_intensity_ragged_batch,  # noqa: F401
                   praat_intensity_list, Intensity, to_intensity, praat_rms_envelope)
from .ema import read_AG50x, read_AG50x_arrays, read_pos_header  # noqa: F401

__version__ = "0.2.0"
