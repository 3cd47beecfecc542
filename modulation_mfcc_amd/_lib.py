"""ctypes binding of libmodmfcc.so (include/modmfcc.h and, for the Welch modulation power spectrum, include/modmfcc_modpsd.h;
for the Welch cross spectrum and coherence, include/modmfcc_modcsd.h; for the quadratic and cubic spline gap filling,
include/modmfcc_spline.h; for the Lomb-Scargle periodogram of rows with holes, include/modmfcc_lomb.h; for the B-spline zoom
of 2-D feature images, include/modmfcc_zoom.h; for the Praat-style spectrogram, include/modmfcc_pspec.h; for Praat's
intensity contour, include/modmfcc_pint.h).

There is NO CPU fallback: when the shared library cannot be loaded, or a plan cannot be created
because no MI355X is visible, the calls raise.  Build the library with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C modulation_mfcc_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MODMFCC_LIB: load another build of the library (development: ablation / stamp builds made by tools/*.sh
# go to their own files instead of overwriting the product library)
LIB_PATH = os.environ.get("MODMFCC_LIB") or os.path.join(_HERE, "libmodmfcc.so")

MM_OK = 0
MM_ERR_INVALID_ARG = -1
MM_ERR_UNSUPPORTED = -2
MM_ERR_HIP = -3
MM_ERR_WORKSPACE = -4
MM_ERR_ALLOC = -5

STAGES = ("logmel", "dct", "modspec", "rfft", "power", "change", "init", "reserved")
MM_NUM_STAGES = 8


class mm_config(C.Structure):
    _fields_ = [
        ("sr", C.c_double),
        ("n_fft", C.c_int32),
        ("win_length", C.c_int32),
        ("hop_length", C.c_int32),
        ("n_mels", C.c_int32),
        ("n_mfcc", C.c_int32),
        ("fmin", C.c_double),
        ("fmax", C.c_double),
        ("preemph", C.c_float),
        ("top_db", C.c_float),
        ("amin", C.c_float),
        ("center", C.c_int32),
        ("n_mod_fft", C.c_int32),
    ]


MM_ST_MAXW, MM_ST_MAXE = 16, 8


class mm_stencil(C.Structure):
    _fields_ = [
        ("n_c", C.c_int32), ("n_edge", C.c_int32), ("edge_w", C.c_int32), ("reserved", C.c_int32),
        ("off", C.c_int32 * MM_ST_MAXW),
        ("c", C.c_double * MM_ST_MAXW),
        ("el", (C.c_double * MM_ST_MAXW) * MM_ST_MAXE),
        ("er", (C.c_double * MM_ST_MAXW) * MM_ST_MAXE),
        ("den_c", C.c_double), ("den_e", C.c_double),
    ]


class mm_pyin_params(C.Structure):
    _fields_ = [
        ("sr", C.c_double), ("fmin", C.c_double), ("fmax", C.c_double),
        ("no_trough_prob", C.c_double), ("log_tiny", C.c_double), ("fill_na", C.c_double),
        ("log_p_init", C.c_double * 2),
        ("frame_length", C.c_int32), ("win_length", C.c_int32), ("hop_length", C.c_int32), ("center", C.c_int32),
        ("min_period", C.c_int32), ("max_period", C.c_int32), ("n_thresholds", C.c_int32), ("nbps", C.c_int32),
        ("n_bins", C.c_int32), ("band_h", C.c_int32), ("max_troughs", C.c_int32), ("reserved", C.c_int32),
    ]


class mm_pyin_tables(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("thresholds", "beta_probs", "beta_cum", "boltzmann", "log_same", "log_cross",
                                           "freqs")]


class mm_peaks_opts(C.Structure):
    _fields_ = [
        ("height", C.c_double * 2), ("threshold", C.c_double * 2), ("prominence", C.c_double * 2),
        ("negate", C.c_int32), ("use_height", C.c_int32), ("use_threshold", C.c_int32), ("use_prominence", C.c_int32),
    ]


class mm_peaks_ext(C.Structure):
    _fields_ = [
        ("plateau_size", C.c_double * 2), ("width", C.c_double * 2), ("rel_height", C.c_double),
        ("distance", C.c_int32), ("wlen", C.c_int32), ("use_plateau_size", C.c_int32), ("use_distance", C.c_int32),
        ("use_width", C.c_int32),
    ]


class mm_peaks_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("count", "idx", "prom", "lbase", "rbase", "widths", "width_heights", "left_ips",
                                           "right_ips", "plateau_sizes", "left_edges", "right_edges")]


MM_MAX_SEC = 16            # sections per SOS filter (mm_change.hip.inc)
MM_RAGGED_MAX_SEC = 4      # sections the ragged IIR entries take (the segmented rows; mm_sos_rows.hip.inc)


class MMError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: {detail}" if detail else what)


_vp = C.c_void_p
_i64 = C.c_int64
_cfgp = C.POINTER(mm_config)
_pyp = C.POINTER(mm_pyin_params)
_pyt = C.POINTER(mm_pyin_tables)

# name -> (restype, argtypes); every symbol include/modmfcc.h declares
PROTOTYPES = {
    "mm_version": (C.c_int, []),
    "mm_strerror": (C.c_char_p, [C.c_int]),
    "mm_last_hip_error": (C.c_char_p, []),
    "mm_config_default": (C.c_int, [_cfgp]),
    "mm_config_validate": (C.c_int, [_cfgp]),
    "mm_num_frames": (_i64, [_cfgp, _i64]),
    "mm_num_bins": (C.c_int32, [_cfgp]),
    "mm_mod_fft_len": (C.c_int32, [_cfgp, _i64]),
    "mm_build_window": (C.c_int, [_cfgp, _vp]),
    "mm_build_mel": (C.c_int, [_cfgp, _vp]),
    "mm_build_dct": (C.c_int, [_cfgp, _vp]),
    "mm_build_mel_sweep": (C.c_int, [_cfgp, C.c_int, _vp, _vp, _vp, _vp]),
    "mm_build_mel_runs": (C.c_int, [_cfgp, C.c_int, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "mm_build_mel_runs_shared": (C.c_int, [_cfgp, C.c_int, C.c_int, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "mm_build_butter_sos": (C.c_int, [C.c_int, C.c_double, _vp]),
    "mm_plan_create": (C.c_int, [_cfgp, C.POINTER(_vp)]),
    "mm_plan_destroy": (C.c_int, [_vp]),
    "mm_plan_config": (C.c_int, [_vp, _cfgp]),
    "mm_plan_kernel_path": (C.c_int, [_vp]),
    "mm_plan_fused_dct": (C.c_int, [_vp]),
    "mm_plan_set_fuse_dct": (C.c_int, [_vp, C.c_int]),
    "mm_plan_fused_tail": (C.c_int, [_vp, _i64, _i64]),
    "mm_plan_shared_runs": (C.c_int, [_vp]),
    "mm_plan_set_shared_runs": (C.c_int, [_vp, C.c_int]),
    "mm_plan_set_fuse_tail": (C.c_int, [_vp, C.c_int]),
    "mm_mfcc_modspec_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_plan_force_generic": (C.c_int, [_vp, C.c_int]),
    "mm_plan_set_variant": (C.c_int, [_vp, C.c_int]),
    "mm_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_mfcc_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    "mm_logmel_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "mm_stft_power_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "mm_rfft_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, C.c_int32, _vp, _vp]),
    "mm_modspec_f32": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "mm_ragged_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_mfcc_ragged_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_mfcc_change_f64": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int32, C.c_int32, _vp, C.c_int32, _vp,
                                     C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_sosfiltfilt_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_sosfiltfilt_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "mm_sosfiltfilt_f32_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_stencil_f64": (C.c_int, [C.POINTER(mm_stencil), _vp, _i64, _i64, _i64, _vp, _vp]),
    "mm_fir_filtfilt_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, _vp, _i64, _vp]),
    "mm_fir_filtfilt_f32_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, _vp, _i64, _vp]),
    "mm_savgol_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _i64, _vp]),
    "mm_sosfiltfilt_ragged_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "mm_sosfiltfilt_ragged_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_sosfiltfilt_ragged_f32_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_stencil_ragged_f64": (C.c_int, [C.POINTER(mm_stencil), _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "mm_fir_filtfilt_ragged_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, _vp, _i64, _vp]),
    "mm_fir_filtfilt_ragged_f32_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, _vp, _i64, _vp]),
    "mm_savgol_ragged_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _i64, _vp]),
    "mm_change_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_change_workspace_bytes_for": (C.c_size_t, [_vp, _i64, _i64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32]),
    "mm_change_ragged_workspace_bytes_for": (C.c_size_t, [_vp, _i64, _i64, C.c_int32, _vp, C.c_int32, _vp, C.c_int32]),
    "mm_mfcc_change_ragged_f64": (C.c_int, [_vp, _vp, _i64, _i64, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp,
                                            C.c_int32, _vp, _vp, C.c_size_t, _vp]),
    "mm_rms_num_frames": (_i64, [_i64, C.c_int32, C.c_int32, C.c_int32]),
    "mm_rms_f32": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "mm_rms_ragged_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "mm_hilbert_ragged_create": (C.c_int, [_i64, C.c_int32, C.POINTER(_vp)]),
    "mm_hilbert_ragged_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_hilbert_envelope_ragged": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, C.c_size_t, _vp]),
    "mm_hilbert_create": (C.c_int, [_i64, C.c_int32, C.POINTER(_vp)]),
    "mm_hilbert_destroy": (None, [_vp]),
    "mm_hilbert_fft_size": (_i64, [_vp]),
    "mm_hilbert_workspace_bytes": (C.c_size_t, [_vp, _i64]),
    "mm_hilbert_envelope": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, C.c_size_t, _vp]),
    "mm_hilbert_rfft_workspace_bytes": (C.c_size_t, [_vp, _i64]),
    "mm_hilbert_rfft_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    "mm_pcm_decode_f32": (C.c_int, [_vp, C.c_int32, C.c_int32, _i64, _vp, _i64, _vp]),
    "mm_resample_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, C.c_int32, C.c_int32, C.c_int32, _i64, _vp, _i64, _vp]),
    "mm_resample_banded_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, _vp, _i64, _vp]),
    "mm_resample_banded_shape": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "mm_pcm_decode_ragged_f32": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    "mm_resample_ragged_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _i64, _vp, _i64,
                                        _i64, _vp]),
    "mm_resample_banded_ragged_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_int32, _vp, _i64, _i64, _vp]),
    "mm_devcopy_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "mm_pyin_check": (C.c_int, [_pyp]),
    "mm_pyin_num_frames": (_i64, [_pyp, _i64]),
    "mm_pyin_cmnd": (C.c_int, [_pyp, _vp, C.c_int32, _i64, _i64, _i64, _vp, _vp]),
    "mm_pyin_candidates": (C.c_int, [_pyp, _pyt, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "mm_pyin_decode_workspace_bytes": (C.c_size_t, [_pyp, _i64, _i64]),
    "mm_pyin_decode": (C.c_int, [_pyp, _pyt, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_pyin_workspace_bytes": (C.c_size_t, [_pyp, _i64, _i64]),
    "mm_pyin_f32": (C.c_int, [_pyp, _pyt, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_pyin_f64": (C.c_int, [_pyp, _pyt, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_pyin_ragged_workspace_bytes": (C.c_size_t, [_pyp, _i64, _i64]),
    "mm_pyin_ragged_f32": (C.c_int, [_pyp, _pyt, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_pyin_ragged_f64": (C.c_int, [_pyp, _pyt, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_interp_nan_linear_ragged_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    "mm_interp_nan_ragged_f64": (C.c_int, [C.c_int32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, C.c_size_t, _vp]),
    "mm_interp_nan_linear_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "mm_interp_nan_workspace_bytes": (C.c_size_t, [C.c_int32, _i64, _i64]),
    "mm_interp_nan_f64": (C.c_int, [C.c_int32, _vp, _i64, _i64, _i64, _vp, _i64, _vp, C.c_size_t, _vp]),
    "mm_regrid_linear_f32_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "mm_find_peaks_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "mm_find_peaks": (C.c_int, [C.POINTER(mm_peaks_opts), _vp, C.c_int32, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp,
                                _vp, _vp, _vp, C.c_size_t, _vp]),
    "mm_find_peaks_ex_workspace_bytes": (C.c_size_t, [C.POINTER(mm_peaks_opts), C.POINTER(mm_peaks_ext), _i64, _i64]),
    "mm_find_peaks_ex": (C.c_int, [C.POINTER(mm_peaks_opts), C.POINTER(mm_peaks_ext), _vp, C.c_int32, _i64, _i64, _i64, _vp,
                                   _vp, _i64, C.POINTER(mm_peaks_out), _vp, C.c_size_t, _vp]),
    "mm_timing_enable": (C.c_int, [_vp, C.c_int]),
    "mm_timing_read": (C.c_int, [_vp, _vp, _vp]),
}


class mm_modpsd_params(C.Structure):
    _fields_ = [
        ("fs", C.c_double),
        ("nperseg", C.c_int32), ("noverlap", C.c_int32), ("nfft", C.c_int32),
        ("detrend", C.c_int32), ("scaling", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


_mpp = C.POINTER(mm_modpsd_params)

# name -> (restype, argtypes); every symbol include/modmfcc_modpsd.h declares (the second header: the Welch modulation
# power spectrum, versioned by mm_modpsd_version apart from mm_version)
PROTOTYPES_MODPSD = {
    "mm_modpsd_version": (C.c_int, []),
    "mm_modpsd_check": (C.c_int, [_mpp]),
    "mm_modpsd_num_segments": (_i64, [_mpp, _i64]),
    "mm_modpsd_create": (C.c_int, [_mpp, _vp, C.POINTER(_vp)]),
    "mm_modpsd_destroy": (None, [_vp]),
    "mm_modpsd_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_modpsd_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, C.c_size_t, _vp]),
}

# every symbol include/modmfcc_modcsd.h declares (the third header: the Welch cross spectrum and coherence, on the handle of
# the second header; versioned by mm_modcsd_version)
PROTOTYPES_MODCSD = {
    "mm_modcsd_version": (C.c_int, []),
    "mm_modcsd_check": (C.c_int, [_mpp]),
    "mm_modcsd_workspace_bytes": (C.c_size_t, [_vp, _i64, _i64]),
    "mm_modcsd_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, C.c_size_t,
                                _vp]),
}

# every symbol include/modmfcc_spline.h declares (the fourth header: interp_NAN's 'quadratic' and 'cubic' kinds)
MM_SPLINE_QUADRATIC, MM_SPLINE_CUBIC = 2, 3
PROTOTYPES_SPLINE = {
    "mm_interp_spline_workspace_bytes": (C.c_size_t, [C.c_int32, _i64, _i64]),
    "mm_interp_spline_f64": (C.c_int, [C.c_int32, _vp, _i64, _i64, _i64, _vp, _i64, _vp, C.c_size_t, _vp]),
    "mm_interp_spline_ragged_f64": (C.c_int, [C.c_int32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, C.c_size_t, _vp]),
}

# every symbol include/modmfcc_lomb.h declares (the fifth header: the Lomb-Scargle periodogram of rows with holes)
MM_LOMB_PRECENTER, MM_LOMB_FLOATING_MEAN = 1, 2
MM_LOMB_POWER, MM_LOMB_NORMALIZE, MM_LOMB_AMPLITUDE = 0 << 2, 1 << 2, 2 << 2
MM_LOMB_CHUNK = 512
PROTOTYPES_LOMB = {
    "mm_lomb_version": (C.c_int, []),
    "mm_lombscargle_workspace_bytes": (C.c_size_t, [_i64, _i64, _i64]),
    "mm_lombscargle_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.c_int32, _vp, _i64, _vp, _vp, C.c_size_t,
                                     _vp]),
}

# every symbol include/modmfcc_zoom.h declares (the sixth header: the B-spline zoom of 2-D feature images)
MM_ZOOM_CONSTANT, MM_ZOOM_MIRROR = 0, 1
MM_ZOOM_PREFILTER, MM_ZOOM_DB, MM_ZOOM_FILTER_ONLY = 1, 2, 4
MM_ZOOM_SEGMENT, MM_ZOOM_MAX_TAPS = 128, 80
_zoom_args = [C.c_int32, C.c_int32, C.c_double, C.c_int32, _vp, _i64, _i64, _i64, _i64, _i64]
_zoom_out = [_i64, _i64, _vp, _i64, _i64, _vp, C.c_size_t, _vp]
PROTOTYPES_ZOOM = {
    "mm_zoom_version": (C.c_int, []),
    "mm_zoom2d_workspace_bytes": (C.c_size_t, [C.c_int32, _i64, _i64, _i64, _i64, _i64]),
    "mm_zoom2d_f32": (C.c_int, _zoom_args + _zoom_out),
    "mm_zoom2d_f64": (C.c_int, _zoom_args + _zoom_out),
    "mm_zoom2d_ragged_f32": (C.c_int, _zoom_args + [_vp, C.c_double] + _zoom_out),
    "mm_zoom2d_ragged_f64": (C.c_int, _zoom_args + [_vp, C.c_double] + _zoom_out),
}



class mm_pspec_params(C.Structure):
    _fields_ = [
        ("scale", C.c_double),
        ("nw", C.c_int32), ("nfft", C.c_int32), ("bw", C.c_int32), ("n_freqs", C.c_int32), ("channels", C.c_int32),
        ("span", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


# every symbol include/modmfcc_pspec.h declares (the seventh header: the Praat-style spectrogram; no entry takes a workspace)
MM_PSPEC_MAX_NFFT, MM_PSPEC_MAX_CHANNELS, MM_PSPEC_DB = 4096, 8, 1
_psp = C.POINTER(mm_pspec_params)
_pspec_args = [_psp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp]
PROTOTYPES_PSPEC = {
    "mm_pspec_version": (C.c_int, []),
    "mm_pspec_check": (C.c_int, [_psp]),
    "mm_pspec_tile_frames": (C.c_int32, [_psp]),
    "mm_pspec_f32": (C.c_int, _pspec_args),
    "mm_pspec_f64": (C.c_int, _pspec_args),
}



class mm_pint_params(C.Structure):
    _fields_ = [("hw", C.c_int32), ("channels", C.c_int32), ("span", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/modmfcc_pint.h declares (the eighth header: Praat's intensity contour; no entry takes a workspace)
MM_PINT_MAX_HALF, MM_PINT_MAX_CHANNELS = 16384, 8
MM_PINT_LINEAR, MM_PINT_KEEP_MEAN = 1, 2
MM_PINT_NEAREST, MM_PINT_LINEAR_INTERP, MM_PINT_CUBIC = 0, 1, 2
_pip = C.POINTER(mm_pint_params)
_pint_args = [_pip, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]
PROTOTYPES_PINT = {
    "mm_pint_version": (C.c_int, []),
    "mm_pint_check": (C.c_int, [_pip]),
    "mm_pint_tile_frames": (C.c_int32, [_pip]),
    "mm_pint_f32": (C.c_int, _pint_args),
    "mm_pint_f64": (C.c_int, _pint_args),
    "mm_pint_value_f64": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.c_double, _vp, _i64, _i64, C.c_int32, _vp, _i64, _vp]),
}

_lib = None
_torch = None       # the torch module, bound by load(): call() and workspace() look nothing up per call


def load():
    """Load libmodmfcc.so (once).  Raises ImportError -- never falls back to a CPU path."""
    global _lib, _torch
    if _lib is not None:
        return _lib
    # torch FIRST: its wheel bundles the HIP runtime (torch/lib/libamdhip64.so), libmodmfcc.so was linked against
    # /opt/rocm's.  Whichever is loaded first serves both (same SONAME); loaded the other way round the process
    # ends up with two runtimes and the second one finds no device ("hipGetDevice failed").
    try:
        import torch
        _torch = torch
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`make -C modulation_mfcc_amd/csrc` (needs hipcc, --offload-arch=gfx950). "
            "modulation_mfcc_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for table in (PROTOTYPES, PROTOTYPES_MODPSD, PROTOTYPES_MODCSD, PROTOTYPES_SPLINE, PROTOTYPES_LOMB, PROTOTYPES_ZOOM,
                  PROTOTYPES_PSPEC, PROTOTYPES_PINT):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError when the .so is stale
            fn.restype = res
            fn.argtypes = args
    if lib.mm_version() < 121:
        raise ImportError("libmodmfcc.so is older than the Python binding; rebuild it")
    _lib = lib
    return lib


def check(status, what):
    if status == MM_OK:
        return
    lib = load()
    msg = lib.mm_strerror(int(status)).decode()
    detail = lib.mm_last_hip_error().decode() if status == MM_ERR_HIP else ""
    if status == MM_ERR_INVALID_ARG:
        raise ValueError(f"{what}: {msg}")
    if status == MM_ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise MMError(status, f"{what}: {msg}", detail)


# ---- compute calls: every entry whose last parameter is ``void* stream`` goes through call() ----------------------------
def torch_stream(dev=None):
    """torch's current stream of ``dev`` (None: of the current device), read now -- the package's one such read."""
    if _torch is None:
        load()
    return _torch.cuda.current_stream(dev)


def call(name, dev, *args, ok=()):
    """The compute entry ``name`` with ``args`` and, as its last argument, the current stream of ``dev``, read at call time
    inside the device guard of ``dev`` (a tensor's device need not be the current one); the status goes through check().
    A failure status listed in ``ok`` is returned unchecked: MM_ERR_UNSUPPORTED where the caller has another route.  The
    entry is looked up on the loaded library at every call (an attribute ctypes caches)."""
    lib = _lib or load()
    with _torch.cuda.device(dev):
        rc = getattr(lib, name)(*args, C.c_void_p(torch_stream(dev).cuda_stream))
    if rc != MM_OK and rc not in ok:
        check(rc, name)
    return rc


def workspace(nbytes, dev):
    """``nbytes`` of scratch on ``dev`` for the calls of one function (a uint8 tensor; pointer and numel() go to the entry)."""
    load()
    return _torch.empty(int(nbytes), dtype=_torch.uint8, device=dev)


def call_chunked(name, dev, rows, chunk, args, ws_bytes=None):
    """The entry ``name`` over ``rows`` rows in calls of at most ``chunk``: ``args(r0, r)`` gives the arguments of the call
    for the rows r0 .. r0 + r - 1.  With ``ws_bytes``, a function of the rows of one call, one workspace sized for ``chunk``
    rows serves every call, appended to its arguments as (pointer, bytes)."""
    tail = ()
    if ws_bytes is not None:
        ws = workspace(ws_bytes(chunk), dev)
        tail = (ws.data_ptr(), ws.numel())
    for r0 in range(0, rows, chunk):
        call(name, dev, *args(r0, min(chunk, rows - r0)), *tail)
