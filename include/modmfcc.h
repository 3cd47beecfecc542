/*
 * modmfcc.h -- C ABI of libmodmfcc.so: MI355X (gfx950) MFCC + modulation-spectrum extractor.
 *
 * The reference (aaron-randreth/modulation-mfcc) is pure Python and has no FFI; the
 * interface each entry point replaces is therefore a Python call site:
 *
 *   mm_mfcc_f32            <- librosa.feature.mfcc(y, sr, n_mfcc, win_length, hop_length,
 *                             n_fft, fmin, fmax) as called at script/mfcc.py:387
 *                             (rows A1-A6 of SURVEY.md section 8(a)), batched over clips
 *   mm_num_frames          <- frame count implied by that call, used at script/mfcc.py:390
 *   mm_logmel_f32          <- the melspectrogram + 10*log10 half of the same call (stage test)
 *   mm_stft_power_f32      <- the stft + |.|^2 half of the same call (stage test / roofline)
 *   mm_rfft_f32            <- the batched rFFT stage in isolation (np.fft.rfft rows; the
 *                             "% HBM roofline (rFFT)" metric of BASELINE.json)
 *   mm_modspec_f32         <- row A8: rFFT over every coefficient's time trajectory
 *                             (build-defined; no reference site)
 *   mm_mfcc_ragged_f32     <- the same MFCC (and row A8) for a padded batch with one length per clip, each clip as if
 *                             it were called alone (build-defined; no reference site)
 *   mm_mfcc_change_f64     <- script/mfcc.py:392-427 (drop c0, Butterworth sosfiltfilt,
 *                             gradient or Savitzky-Golay derivative, norm, output filter) -- row N1
 *   mm_mfcc_change_ragged_f64 <- the same tail for the result of mm_mfcc_ragged_f32: one frame count per clip, each
 *                             clip's curve as if it were called alone (build-defined; no reference site)
 *   mm_sosfiltfilt_f64     <- applyFilter(filt='iir') (script/mfcc.py:29-135): scipy sosfiltfilt on a batch
 *   mm_stencil_f64         <- get_velocity (script/calc.py:593-650): np.gradient / savgol_filter /
 *                             findiff derivative of a curve -- row N2
 *   mm_fir_filtfilt_f64,
 *   mm_savgol_f64          <- applyFilter(filt='fir' | 'sg') and get_velocity(method='sg') with filters of any length:
 *                             scipy filtfilt(b, 1, x) / savgol_filter(mode='interp') on a batch
 *   mm_sosfiltfilt_ragged_f64, mm_stencil_ragged_f64,
 *   mm_fir_filtfilt_ragged_f64,
 *   mm_savgol_ragged_f64   <- the four filters above on a padded batch with one length per curve, each curve filtered as
 *                             if it were called alone, bit for bit (build-defined; no reference site)
 *   mm_rms_ragged_f32,
 *   mm_hilbert_envelope_ragged <- the two envelopes below for a padded batch with one length per clip
 *   mm_rms_f32,
 *   mm_hilbert_envelope    <- calculate_amplitude_envelope (script/calc.py:284-343): librosa.feature.rms /
 *                             |scipy.signal.hilbert| -- row N3
 *   mm_pcm_decode_ragged_f32, mm_resample_ragged_f32,
 *   mm_resample_banded_ragged_f32 <- the loader below for a list of files: one decode launch for all of them, both
 *                             resamplers with one length per row (build-defined; no reference site)
 *   mm_pcm_decode_f32,
 *   mm_resample_f32        <- librosa.load(path, sr=sigSr, mono=False) (script/mfcc.py:284,373) -- row N4
 *   mm_find_peaks,
 *   mm_find_peaks_ex       <- MinMaxFinder (script/calc.py:651-686; script/main.py:1546-1613):
 *                             scipy.signal.find_peaks(y) / find_peaks(-y) on a batch of curves
 *   mm_build_window/mel/dct<- scipy.signal.get_window('hann'), librosa.filters.mel,
 *                             scipy.fftpack.dct(type=2, norm='ortho') constant tables
 *
 * Contract:
 *   - plain pointers and sizes only; every data/workspace pointer is DEVICE memory owned by
 *     the caller (e.g. torch tensor.data_ptr()); the plan owns only constant device tables;
 *   - every compute call is asynchronous on the caller's hipStream_t (passed as void*), does
 *     no allocation and no synchronisation (graph-capture safe);
 *   - functions return MM_OK (0) or a negative mm_status; nothing throws, nothing exits;
 *   - a plan is bound to the device current at creation.  Its constant tables never change after mm_plan_create;
 *     the few SET-UP calls that do change plan state -- mm_plan_set_variant, mm_plan_set_fuse_dct,
 *     mm_plan_set_fuse_tail, mm_plan_force_generic, mm_timing_enable / mm_timing_read -- are unsynchronised
 *     host-side switches: call them from the thread that owns the plan, between compute calls, never while another
 *     thread is inside a compute call on the same plan.  A plan that is only computed with (no set-up calls, timing
 *     off) may be shared by threads that each pass their own buffers, workspace and stream.
 */
#ifndef MODMFCC_H
#define MODMFCC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_VERSION 123 /* 0.3.3 */

typedef enum mm_status {
  MM_OK = 0,
  MM_ERR_INVALID_ARG = -1,  /* NULL pointer, non-positive size, fmax <= fmin ...              */
  MM_ERR_UNSUPPORTED = -2,  /* n_fft > 8192, center == 0, n_mod_fft not a power of two ...    */
  MM_ERR_HIP = -3,          /* a HIP runtime call failed (see mm_last_hip_error)              */
  MM_ERR_WORKSPACE = -4,    /* workspace smaller than mm_workspace_bytes()                    */
  MM_ERR_ALLOC = -5
} mm_status;

/* POD configuration; mirrors the keyword arguments of the librosa call at script/mfcc.py:387
 * plus the build's extensions (n_mels, preemph, top_db, amin, n_mod_fft). */
typedef struct mm_config {
  double sr;          /* sample rate in Hz (sigSr)                                            */
  int32_t n_fft;      /* FFT length: ANY integer 2..8192 (librosa: any n_fft >= win_length)   */
  int32_t win_length; /* int(winLen*sigSr), 1..n_fft                                          */
  int32_t hop_length; /* int(tStep*sigSr), >= 1                                               */
  int32_t n_mels;     /* librosa default 128; 1..256                                          */
  int32_t n_mfcc;     /* 1..n_mels                                                            */
  double fmin;        /* minFreq                                                              */
  double fmax;        /* maxFreq (may exceed Nyquist: empty filters, as the reference does)   */
  float preemph;      /* 0 = off (reference behaviour); y[n] - a*y[n-1]                       */
  float top_db;       /* 80; < 0 disables the per-clip clamp                                  */
  float amin;         /* 1e-10                                                                */
  int32_t center;     /* must be 1 (librosa center=True, pad_mode='constant')                 */
  int32_t n_mod_fft;  /* trajectory rFFT length; 0 = next power of two >= n_frames (> 8192: mm_hilbert_rfft_f32) */
} mm_config;

typedef struct mm_plan mm_plan;

/* kernels whose device time mm_timing_read() reports */
enum {
  MM_STAGE_LOGMEL = 0,   /* fused frame+window+rFFT+power+mel+log (+per-clip max)             */
  MM_STAGE_DCT = 1,      /* top_db clamp + DCT-II                                             */
  MM_STAGE_MODSPEC = 2,  /* trajectory rFFT                                                   */
  MM_STAGE_RFFT = 3,     /* stage-isolated batched rFFT                                       */
  MM_STAGE_POWER = 4,    /* fused frame+window+rFFT+power                                     */
  MM_STAGE_CHANGE = 5,   /* MFCC-change tail                                                  */
  MM_STAGE_INIT = 6,     /* clip-max reset                                                    */
  MM_NUM_STAGES = 8
};

int mm_version(void);
const char* mm_strerror(int status);
const char* mm_last_hip_error(void);

/* ---- host-only helpers (no GPU needed) ------------------------------------------------ */
int mm_config_default(mm_config* cfg);                           /* reference defaults      */
int mm_config_validate(const mm_config* cfg);
int64_t mm_num_frames(const mm_config* cfg, int64_t n_samples);  /* 1 + (n_samples + 2 (n_fft / 2) - n_fft) / hop: 1 + n_samples / hop for even n_fft */
int32_t mm_num_bins(const mm_config* cfg);                       /* n_fft/2 + 1             */
int32_t mm_mod_fft_len(const mm_config* cfg, int64_t n_frames);  /* resolved n_mod_fft      */
int mm_build_window(const mm_config* cfg, float* out /*[n_fft]*/);
int mm_build_mel(const mm_config* cfg, float* out /*[n_mels][n_fft/2+1]*/);
int mm_build_dct(const mm_config* cfg, float* out /*[n_mfcc][n_mels]*/);
/* Sweep form of the mel matrix used by the lane<->frame kernels (host-only, for tests): bin k
 * feeds filter d[k] with weight wlo[k] and filter d[k]+1 with weight whi[k]; part = per-wave
 * {k_begin, k_end, m_begin, m_end}.  Returns MM_ERR_UNSUPPORTED if the matrix has another shape. */
int mm_build_mel_sweep(const mm_config* cfg, int n_waves, float* wlo /*[n_bins]*/,
                       float* whi /*[n_bins]*/, int32_t* d /*[n_bins]*/, int32_t* part /*[n_waves][4]*/);
/* Run form of the same sweep, exactly as the fused kernel reads it from LDS (host-only, for tests):
 * hdr [n_runs][4] = {first bin (multiple of 4), n_groups, first group, filter d}; grp [n_groups][8] =
 * {weight in filter d x4, weight in filter d+1 x4}; part [n_waves][4] = {run_begin, run_end, m_begin,
 * m_end}.  counts[0] = n_runs, counts[1] = n_groups.  Capacities are in runs / groups. */
int mm_build_mel_runs(const mm_config* cfg, int n_waves, int32_t* hdr, int32_t hdr_cap, float* grp,
                      int32_t grp_cap, int32_t* part, int32_t* counts);
/* The "shared runs" form of that table, which the fused launches of the staged-sample kernel walk where the plan has
 * two log-mel tiles and no empty filter (host-only, for tests): every run d = -1 .. n_mels-1 appears ONCE.  The first part
 * with a filter starts at run m_begin-1, every other one at run m_begin; the last run of a part that has a successor
 * keeps both weights, and its second sum is handed to the successor.  part[w][3] = m_end | 1 << 16 (the part's first
 * filter takes its rising half from the part before) | 1 << 17 (its last run hands over).  weighted = 1 (n_waves 16
 * only): the cuts of the fused plan, whose four DCT waves get half-size parts; 0: the cuts of mm_build_mel_runs. */
int mm_build_mel_runs_shared(const mm_config* cfg, int n_waves, int weighted, int32_t* hdr, int32_t hdr_cap, float* grp,
                             int32_t grp_cap, int32_t* part, int32_t* counts);
/* Butterworth low-pass as second-order sections, scipy.signal.butter(order, wn, 'low',
 * output='sos') layout [n_sections][6]; returns the number of sections or a negative status. */
int mm_build_butter_sos(int order, double wn, double* sos /*[(order+1)/2][6]*/);

/* ---- plan ----------------------------------------------------------------------------- */
int mm_plan_create(const mm_config* cfg, mm_plan** out);
int mm_plan_destroy(mm_plan* plan);
int mm_plan_config(const mm_plan* plan, mm_config* out);
/* Which fused kernel a log-mel / MFCC call of this plan runs on, for a regular call (aligned rows,
 * n_samples >= 4): 0 = generic LDS radix-2; 1 = register radix-16, 8 waves per workgroup; 2 = register
 * radix-16, 16 waves, direct loads (n_fft 512, even hop, no pre-emphasis); 3 = register radix-16
 * wave-per-frame-group kernel (n_fft 1024 / 2048, and what is left of n_fft 512); 4 = variant 2 with the
 * tile's samples staged through LDS (hop <= 252; any hop parity, row alignment and length, optional
 * pre-emphasis); 5 = 12-wave kernel with the mel contraction (and for n_mfcc <= 16 the DCT-II) on the
 * matrix pipe, 48-frame double-buffered power tiles (n_fft 512, hop <= 170 at 40 mel: the tables must fit
 * the 160 KB of LDS) -- opt-in (mm_plan_set_variant): measured slower than variant 4, see DESIGN.md.  n_fft 64 / 128 / 256 plans use the n_fft 512
 * variants too (frames zero-padded to 512 points: same power at every (512/n_fft)-th bin).  6 = the any-length
 * kernel: every n_fft that is not a power of two in [32, 4096] -- 400, 600, 1000, 1536, a prime, 8192, 16 -- as a
 * mixed-radix (2 / 3 / 5 / 7) Stockham FFT in LDS, Bluestein's chirp-z transform for lengths with other prime factors
 * (such a plan has this one kernel: variants and force_generic do not apply). */
int mm_plan_kernel_path(const mm_plan* plan);
/* 1 if mm_mfcc_f32 of this plan applies the DCT-II inside the log-mel kernel (variants 4 and 5: the DCT
 * of the unclamped rows, followed by a fix-up launch that redoes only the clips whose minimum lies more
 * than top_db under their maximum), 0 if it runs the separate clamp + DCT kernel. */
int mm_plan_fused_dct(const mm_plan* plan);
/* on = 0: always run the separate clamp + DCT kernel (A/B measurements, cross-checks); returns the
 * previous setting.  Default on. */
int mm_plan_set_fuse_dct(mm_plan* plan, int on);
/* mm_mfcc_modspec_f32 in ONE launch (whole clips per workgroup: the clip maximum / minimum never leave it, the
 * clamp fix-up and the trajectory rFFT of the workgroup's clips run at the end of the tile kernel)?  1 when the
 * n_fft 512 staged-sample kernel with its fused DCT takes the call, the trajectory length is 512 or 1024 and
 * `batch` clips spread over the compute units within 4 % (at most 32 per workgroup); 0 = the separate launches.
 * mm_plan_set_fuse_tail(plan, 0) pins the separate launches (A/B measurements, cross-checks; returns the previous
 * setting; default on = 1).  2 widens clip mode to 2048-point trajectories (1025 .. 2048 frames per clip: the 2048-point
 * transform at the end of the launch) and to mm_mfcc_f32 on plans with empty mel filters (their add inside the launch):
 * faster when no clip clamps, slower when a few do (one workgroup pays a clip's whole fix-up) -- see DESIGN.md 4.3.  The same switch selects the device form of mm_mfcc_change_f64 (on: the clip-resident
 * single launch; off: the time-major launches). */
int mm_plan_fused_tail(const mm_plan* plan, int64_t batch, int64_t n_samples);
int mm_plan_set_fuse_tail(mm_plan* plan, int on);
/* Shared mel runs in the fused launches of the staged-sample kernel: mm_plan_shared_runs() = 1 when a
 * regular fused call of this plan walks every mel run once (two log-mel tiles, no empty filters, an instantiation for the
 * plan's hop), 0 when it walks the overlapping runs of mm_build_mel_runs.  The results are bit for bit the same.
 * mm_plan_set_shared_runs(plan, 0) pins the overlapping runs (A/B measurements, cross-checks); returns the previous
 * setting; default on. */
int mm_plan_shared_runs(const mm_plan* plan);
int mm_plan_set_shared_runs(mm_plan* plan, int on);
/* force the generic kernels (debug / cross-check); returns previous value */
int mm_plan_force_generic(mm_plan* plan, int on);
/* pin one of the variants above (1..5) for the calls it can take, 0 = automatic choice; returns the
 * previous setting.  Results of all variants agree within float32 round-off (tests/test_gpu_parity.py);
 * this is how the tests and tools/ab.sh select a kernel -- the library reads no environment variable. */
int mm_plan_set_variant(mm_plan* plan, int variant);
size_t mm_workspace_bytes(const mm_plan* plan, int64_t batch, int64_t n_samples);

/* ---- compute (device pointers, async on `stream`) ---------------------------------------
 * d_audio : float32 [batch][audio_stride], n_samples valid per clip
 * d_mfcc  : float32 [batch][n_mfcc][n_frames]   (coefficient-major, librosa layout)          */
int mm_mfcc_f32(mm_plan* plan, const float* d_audio, int64_t batch, int64_t n_samples,
                int64_t audio_stride, float* d_mfcc, void* d_workspace, size_t ws_bytes,
                void* stream);

/* d_logmel : float32 [batch][n_mels][n_frames], 10*log10(max(amin, mel)) BEFORE the clamp;
 * d_clipmax: float32 [batch], per-clip maximum of d_logmel                                   */
int mm_logmel_f32(mm_plan* plan, const float* d_audio, int64_t batch, int64_t n_samples,
                  int64_t audio_stride, float* d_logmel, float* d_clipmax, void* stream);

/* d_power : float32 [batch][n_frames][n_fft/2+1] (frame-major)                               */
int mm_stft_power_f32(mm_plan* plan, const float* d_audio, int64_t batch, int64_t n_samples,
                      int64_t audio_stride, float* d_power, void* stream);

/* rows of `in_len` (<= n, zero padded) real samples -> complex64 [rows][n/2+1] interleaved;
 * n a power of two in [32, 8192].                                                             */
int mm_rfft_f32(mm_plan* plan, const float* d_in, int64_t rows, int64_t in_len,
                int64_t in_stride, int32_t n, float* d_out, void* stream);

/* d_mfcc [batch][n_mfcc][n_frames] -> complex64 [batch][n_mfcc][n_mod/2+1]                   */
int mm_modspec_f32(mm_plan* plan, const float* d_mfcc, int64_t batch, int64_t n_frames,
                   float* d_modspec, void* stream);

/* Rows A1-A6 + A8 in one call: d_mfcc as mm_mfcc_f32 (bit for bit), d_modspec as mm_modspec_f32 of it (to
 * float32 round-off: the in-kernel transform is a second instantiation of the same code); one kernel launch
 * where mm_plan_fused_tail() says so, the two calls' launches otherwise.  Workspace: mm_workspace_bytes(). */
int mm_mfcc_modspec_f32(mm_plan* plan, const float* d_audio, int64_t batch, int64_t n_samples,
                        int64_t audio_stride, float* d_mfcc, float* d_modspec, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* Ragged batches (csrc/mm_ragged.hip; no reference site: the reference takes one clip per call): a padded batch
 * d_audio [batch][audio_stride] with n_samples = the longest clip and d_lengths (DEVICE, int64 [batch]) the valid
 * samples of every clip.  With T_b = mm_num_frames(lengths[b]) and T_max = mm_num_frames(n_samples):
 *   d_mfcc [batch][n_mfcc][T_max]: columns [0, T_b) = the MFCC of clip b ALONE as mm_mfcc_f32 defines it (its own centre
 *     padding at its own end, the top_db maximum over its own n_mels x T_b values), columns [T_b, T_max) = 0.0f;
 *   d_modspec (may be NULL) complex64 [batch][n_mfcc][n_mod / 2 + 1], n_mod = mm_mod_fft_len(T_max): mm_modspec_f32 of
 *     d_mfcc, i.e. the rFFT of every clip's own T_b columns zero-padded to the batch's n_mod.
 * Samples at and beyond lengths[b] never enter a result, whatever they hold (NaN, Inf, another clip's audio); a row's
 * result does not depend on the other rows (bit for bit, for one n_samples).  A length outside [1, n_samples] is clamped
 * into it on the device: a wrong row, never an access out of bounds.  Every plan and kernel path; asynchronous on
 * `stream`, no allocation, no synchronisation.  The launches: the plan's unclamped log-mel (mm_logmel_f32) over the
 * batch as it lies, the same over one short patch row per clip that redoes the few frames reaching past the clip's end,
 * a per-clip maximum, clamp + DCT-II, and the trajectory rFFT.  MM_ERR_UNSUPPORTED when d_modspec is
 * given and n_mod > 8192 (pass NULL and transform d_mfcc with mm_hilbert_rfft_f32), and for a plan with |preemph| > 1 (the
 * patch row continues a clip with preemph^k y[L - 1], which must not grow); MM_ERR_INVALID_ARG / MM_ERR_WORKSPACE
 * as mm_mfcc_f32.  Workspace: mm_ragged_workspace_bytes() (0 for invalid arguments). */
size_t mm_ragged_workspace_bytes(const mm_plan* plan, int64_t batch, int64_t n_samples);
int mm_mfcc_ragged_f32(mm_plan* plan, const float* d_audio, int64_t batch, int64_t n_samples, int64_t audio_stride,
                       const int64_t* d_lengths, float* d_mfcc, float* d_modspec, void* d_workspace, size_t ws_bytes,
                       void* stream);

/* MFCC-change tail (script/mfcc.py:392-427, outFilter 'iir' low-pass or None): d_mfcc [batch][n_mfcc]
 * [n_frames] f32 -> d_change [batch][n_frames] f64.  diff_method 0 = np.gradient (diffMethod='grad',
 * script/mfcc.py:405-407), 1 = savgol_filter(x, 3, 2, deriv=1, mode='interp') (any other diffMethod,
 * script/mfcc.py:409-412; needs n_frames >= 3).
 * sos1/sos2: HOST pointers to [n_sec][6] Butterworth sections (first / output filter).
 * Float64 recursion with fused multiply-adds (5 operations per section and sample), the odd extension of the float32
 * MFCC rows formed in float32 as scipy does on a float32 array: within ~1e-11 of scipy (tests: 1e-9 of the curve's maximum).
 * Three device forms, the same arithmetic per sample (they differ by rounding, ~1e-13 relative at most):
 *   - clip-resident (default for both filters <= 4 sections and clips up to ~5000 frames): one launch, a workgroup per clip, the clip's rows and the curve
 *     in LDS (rows in groups when they do not fit at once), the filters time-parallel over 64 chunks per row;
 *     of the workspace only ~10 KB of filter tables are used;
 *   - segmented rows (clips so long that LDS holds less than a quarter of their rows at once, about 5000 frames at
 *     12 rows -- one recording at the reference's default 1 ms step is 10 001 frames per ten seconds): both filters
 *     through the kernels of
 *     mm_sosfiltfilt_f64 (a wave per 1088 samples of a row), the derivative + norm between them;
 *   - time-major (more than 4 sections, and after mm_plan_set_fuse_tail(plan, 0)): eight launches over a float64
 *     workspace of [frames][rows of all clips].                                                */
int mm_mfcc_change_f64(mm_plan* plan, const float* d_mfcc, int64_t batch, int64_t n_frames,
                       int32_t remove_first, int32_t diff_method, const double* sos1, int32_t n_sec1,
                       const double* sos2, int32_t n_sec2, double* d_change,
                       void* d_workspace, size_t ws_bytes, void* stream);
/* Workspace: mm_change_workspace_bytes_for() = what the form THIS call takes needs (same arguments as the call: a few KB
 * for the clip-resident form, ~2 x rows x frames doubles for the other two); mm_change_workspace_bytes() = the upper
 * bound over all forms and filters, for callers that size their buffer before they know the filters.  The call checks
 * ws_bytes against the former. */
size_t mm_change_workspace_bytes(const mm_plan* plan, int64_t batch, int64_t n_frames);
size_t mm_change_workspace_bytes_for(const mm_plan* plan, int64_t batch, int64_t n_frames, int32_t remove_first,
                                     const double* sos1, int32_t n_sec1, const double* sos2, int32_t n_sec2);

/* The same tail for a ragged batch (no reference site: the reference takes one clip per call): d_mfcc [batch][n_mfcc]
 * [n_frames_max] f32 and d_frames (DEVICE, int64 [batch]) as mm_mfcc_ragged_f32 writes / its caller derives them ->
 * d_change [batch][n_frames_max] f64.  With T_b = d_frames[b]:
 *   columns [0, T_b) = mm_mfcc_change_f64 on d_mfcc[b][:][0 .. T_b) ALONE: both odd extensions formed about frame T_b - 1
 *     (the MFCC rows' in float32), the one-sided derivative at T_b - 1, the norm, the second filter;
 *   columns [T_b, n_frames_max) = +0.0.
 * MFCC columns at and behind T_b never enter a result, whatever they hold (NaN, Inf): the kernel loads T_b columns of a row.
 * A row's result depends on its own data, T_b and n_frames_max only (bit for bit reproducible for one n_frames_max; against
 * the single-length call it differs by rounding, ~1e-13 relative: the filters' chunk length follows n_frames_max).
 * d_frames[b] outside [1, n_frames_max] is clamped into it on the device.  A clip scipy refuses, T_b <= the larger padding
 * length, comes out NaN in [0, T_b): never an access out of bounds.  One launch of the clip-resident kernel (plus the
 * table uploads), a workgroup per clip, shaped on the host for n_frames_max; no allocation, no synchronisation,
 * asynchronous on `stream`.  mm_plan_set_fuse_tail() does not affect it.
 * MM_ERR_UNSUPPORTED, before any launch, where the clip-resident form does not reach: a filter of more than 4 sections, or
 * n_frames_max so long that one row and the curve do not fit LDS (about 10 000 frames) -- run mm_mfcc_change_f64 per
 * distinct length then.  MM_ERR_INVALID_ARG as mm_mfcc_change_f64 (checked against n_frames_max) and for d_frames == NULL;
 * MM_ERR_WORKSPACE below mm_change_ragged_workspace_bytes_for() (the filter tables, a few KB; 0 for invalid arguments). */
size_t mm_change_ragged_workspace_bytes_for(const mm_plan* plan, int64_t batch, int64_t n_frames_max, int32_t remove_first,
                                            const double* sos1, int32_t n_sec1, const double* sos2, int32_t n_sec2);
int mm_mfcc_change_ragged_f64(mm_plan* plan, const float* d_mfcc, int64_t batch, int64_t n_frames_max,
                              const int64_t* d_frames, int32_t remove_first, int32_t diff_method,
                              const double* sos1, int32_t n_sec1, const double* sos2, int32_t n_sec2,
                              double* d_change, void* d_workspace, size_t ws_bytes, void* stream);

/* Zero-phase IIR filter of float64 curves: scipy.signal.sosfiltfilt(sos, x) with its defaults (odd
 * extension by 3 * ntaps samples, sosfilt_zi initial state), i.e. the 'iir' branch of applyFilter
 * (script/mfcc.py:29-135, script/calc.py:23-129) on a batch.  d_x [rows][x_stride] -> d_y [rows][n];
 * sos: HOST pointer to [n_sec][6] sections; n must exceed the padding length.  Needs no plan.
 * Up to 4 sections (Butterworth order <= 8): rows of any length in segments of 64 x 17 samples, a wave per segment,
 * the recursion closed over chunk / segment / row levels (three launches per direction, 24 bytes of traffic per
 * sample and direction; from 128 rows on a workgroup walks a row, sixteen segments per round: one launch per direction,
 * 16 bytes per sample: 256 rows x 160 000 samples in 0.39 ms); more sections: a lane per row, eight chunks.
 * Differs from scipy's sequential recursion by rounding only. */
int mm_sosfiltfilt_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* sos,
                       int32_t n_sec, double* d_y, void* d_workspace, size_t ws_bytes, void* stream);
size_t mm_sosfiltfilt_workspace_bytes(int64_t rows, int64_t n);
/* The same for FLOAT32 rows (librosa's RMS envelope, MFCC rows): scipy.signal.sosfiltfilt forms the odd extension
 * `2 x[0] - x[k]` in the array's own type before its recursion upcasts, so the padded samples of a float32 curve are
 * rounded to float32 -- this entry point does exactly that (the float64 entry point on an upcast copy differs from
 * scipy's result on the float32 array by ~3e-9).  Same workspace. */
int mm_sosfiltfilt_f32_f64(const float* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* sos,
                           int32_t n_sec, double* d_y, void* d_workspace, size_t ws_bytes, void* stream);

/* Derivative transforms of get_velocity (script/calc.py:593-650; row N2) as ONE banded linear operator
 * along time on float64 rows: interior output i = (sum_k c[k] x[i + off[k]]) / den_c; the n_edge first
 * outputs = (el[i] . x[0 .. edge_w)) / den_e, the n_edge last ones = (er[i] . x[n - edge_w .. n)) / den_e.
 * np.gradient (n_c 2, off {-1, +1}, c {-1, 1}, den_c 2h; one edge row {-1, 1}, den_e h) comes out bit for
 * bit; Savitzky-Golay (mode='interp') and the findiff stencils to float64 round-off.  The host builds the
 * taps (modulation_mfcc_amd/calc.py: velocity_stencil).  d_x [rows][x_stride] -> d_y [rows][n], n >=
 * max(2 n_edge, edge_w, spread of off).  Needs no plan. */
#define MM_ST_MAXW 16
#define MM_ST_MAXE 8
typedef struct mm_stencil {
  int32_t n_c, n_edge, edge_w, reserved;
  int32_t off[MM_ST_MAXW];
  double c[MM_ST_MAXW];
  double el[MM_ST_MAXE][MM_ST_MAXW];
  double er[MM_ST_MAXE][MM_ST_MAXW];
  double den_c, den_e;
} mm_stencil;
int mm_stencil_f64(const mm_stencil* st, const double* d_x, int64_t rows, int64_t n, int64_t x_stride,
                   double* d_y, void* stream);

/* FIR filters and Savitzky-Golay windows of ANY length (csrc/mm_longfilt.hip): what mm_stencil does not hold.  Tables are
 * DEVICE pointers, built on the host (modulation_mfcc_amd/filters.py: fir_filtfilt_taps, savgol_tables).  d_x
 * [rows][x_stride] -> d_y [rows][y_stride], float64 out; d_y must not overlap d_x.  A workgroup computes 2048 consecutive
 * outputs of a row, the taps in chunks of 128 (each chunk summed on its own, then the chunk sums).  No plan, no workspace.
 * 256 rows x 160 000 samples: 101 FIR taps 0.51 ms, a Savitzky-Golay window of 101 samples 0.34 ms.
 *
 * mm_fir_filtfilt_f64: scipy.signal.filtfilt(b, 1, x) with its defaults for n_taps = len(b) >= 2 taps, n > 3 n_taps -- the
 * 'fir' branch of applyFilter (script/mfcc.py:113-126).  Both start-up transients of filtfilt lie in the cropped padding,
 * so every output is the correlation of the odd-extended row (2 x[0] - x[m] before, 2 x[n-1] - x[n-1-m] after it; formed
 * while the samples are staged) with d_h [2 n_taps - 1] = b (*) reversed b.  Differs from scipy's two sequential passes by
 * rounding only.  mm_fir_filtfilt_f32_f64: the same for FLOAT32 rows, the extension formed in float32 and then widened, as
 * scipy forms it on a float32 array (cf. mm_sosfiltfilt_f32_f64).
 *
 * mm_savgol_f64: scipy.signal.savgol_filter(x, window, polyorder, deriv, delta, mode='interp'), window <= n.  Outputs
 * [window / 2, n - window / 2) are the correlation with d_c [window] = savgol_coeffs(...)[::-1] on x[i - (window - 1) / 2
 * ...] (an even window is centred as scipy's convolve1d centres it).  The first and last window / 2 outputs come from the
 * polynomial fitted to the first / last window: a = Q x[window] with d_q [n_basis][window] an orthonormal basis of the
 * polynomials of degree < n_basis = polyorder + 1 on the window, then y = P a with d_p [2][window / 2][n_basis] the basis'
 * deriv-th derivatives (delta folded in) at the first, then at the last window / 2 positions.  d_q / d_p may be NULL when
 * window == 1.
 *
 * MM_ERR_INVALID_ARG before any launch: NULL pointers, rows < 1, n <= 3 n_taps or n_taps < 2, window > n or < 1, n_basis
 * outside [1, window], strides < n, more than 2^31 - 1 tiles. */
int mm_fir_filtfilt_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_h, int32_t n_taps,
                        double* d_y, int64_t y_stride, void* stream);
int mm_fir_filtfilt_f32_f64(const float* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_h, int32_t n_taps,
                            double* d_y, int64_t y_stride, void* stream);
int mm_savgol_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_c, const double* d_q,
                  const double* d_p, int32_t window, int32_t n_basis, double* d_y, int64_t y_stride, void* stream);

/* The filters above for a ragged batch (no reference site: the reference filters one curve per call): the arguments of
 * the single-length entry point with n read as n_max, the longest row, and d_lens (DEVICE, int64 [rows]), one length per
 * row, the convention of d_frames of mm_mfcc_change_ragged_f64.  d_y is [rows][n_max] ([rows][y_stride] for the FIR and
 * Savitzky-Golay entries).  With n_b = d_lens[b], clamped on the device into [1, n_max]:
 *   columns [0, n_b) of row b = BIT FOR BIT what the single-length entry point writes for d_x[b][0 .. n_b) alone (rows = 1,
 *     n = n_b): both odd extensions about the row's own first and last sample (in float32 for the _f32_f64 entries), the
 *     backward IIR pass from the row's own end, the Savitzky-Golay edge fits on the row's own first and last window, the
 *     stencil's right edge rows at n_b;
 *   columns [n_b, n_max) = +0.0.
 * Nothing at or behind n_b is loaded, whatever it holds (NaN, Inf, another row's data), and nothing outside
 * [rows][x_stride] is touched.  A row scipy would refuse -- n_b <= padlen (sosfiltfilt), n_b <= 3 n_taps (FIR), window > n_b
 * (Savitzky-Golay), n_b < max(2 n_edge, edge_w) (stencil) -- comes out NaN in [0, n_b) and zero behind it; its neighbours
 * are not affected.  The launches are those of the single-length call at n_max, shaped on the host: no allocation, no
 * synchronisation, no read-back of the lengths, asynchronous on `stream`.
 * mm_sosfiltfilt_ragged_*: up to 4 sections (more: MM_ERR_UNSUPPORTED before any launch -- filter per distinct length with
 * mm_sosfiltfilt_f64 then), on the segmented rows: segments anchored at the row's own start (forward) and end (backward),
 * segments behind the row's extended length exit.  A row alone runs a wave per segment; so does the ragged call, except
 * from 128 rows on when n_max + 2 padlen <= 16 x 1088, where a workgroup walks each row in ONE round of sixteen segments,
 * which is the same arithmetic operation for operation (a second round would carry a differently rounded state).
 * mm_stencil_ragged_f64 reads st->reserved as the shortest row the CALLER takes where that exceeds the operator's own
 * minimum (filtfilt as a banded operator: 3 n_taps + 1); shorter rows come out NaN.  mm_stencil_f64 ignores the field.
 * Workspace: mm_sosfiltfilt_ragged_workspace_bytes(rows, n_max) (0 for invalid arguments); MM_ERR_WORKSPACE below it.
 * MM_ERR_INVALID_ARG as the single-length entries (checked against n_max), and for d_lens == NULL. */
size_t mm_sosfiltfilt_ragged_workspace_bytes(int64_t rows, int64_t n_max);
int mm_sosfiltfilt_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                              const double* sos, int32_t n_sec, double* d_y, void* d_workspace, size_t ws_bytes,
                              void* stream);
int mm_sosfiltfilt_ragged_f32_f64(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                                  const double* sos, int32_t n_sec, double* d_y, void* d_workspace, size_t ws_bytes,
                                  void* stream);
int mm_stencil_ragged_f64(const mm_stencil* st, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                          const int64_t* d_lens, double* d_y, void* stream);
int mm_fir_filtfilt_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                               const double* d_h, int32_t n_taps, double* d_y, int64_t y_stride, void* stream);
int mm_fir_filtfilt_ragged_f32_f64(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                                   const double* d_h, int32_t n_taps, double* d_y, int64_t y_stride, void* stream);
int mm_savgol_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                         const double* d_c, const double* d_q, const double* d_p, int32_t window, int32_t n_basis,
                         double* d_y, int64_t y_stride, void* stream);

/* Framewise RMS (row N3): librosa.feature.rms(y, frame_length, hop_length, center, pad_mode=
 * 'constant') as called at script/calc.py:331 / script/mfcc.py:247.  d_audio [batch][audio_stride]
 * -> d_rms [batch][n_out], n_out = 1 + (n_samples + 2*(center ? frame_length/2 : 0) - frame_length)
 * / hop_length.  Needs no plan. */
int64_t mm_rms_num_frames(int64_t n_samples, int32_t frame_length, int32_t hop_length, int32_t center);
int mm_rms_f32(const float* d_audio, int64_t batch, int64_t n_samples, int64_t audio_stride,
               int32_t frame_length, int32_t hop_length, int32_t center, float* d_rms, void* stream);
/* The same for a ragged batch (no reference site: the reference takes one clip per call): d_audio [batch][audio_stride]
 * padded to n_max samples and d_lens (DEVICE, int64 [batch]), the valid samples of each clip, clamped by the kernels into
 * [1, n_max] -> d_rms [batch][t_max], t_max = mm_rms_num_frames(n_max, ...).  Row b holds the T_b = mm_rms_num_frames(n_b,
 * ...) frames of audio[b, :n_b] -- its own centre padding, zeros for everything at or behind n_b, which is never read --
 * bit for bit what mm_rms_f32 gives for that clip alone (the same kernels, the same summation order), and +0.0 in
 * [T_b, t_max).  Without centring a clip shorter than frame_length has no frame: its row is NaN.  The launch is that of
 * n_max, whatever the lengths. */
int mm_rms_ragged_f32(const float* d_audio, int64_t batch, int64_t n_max, int64_t audio_stride, const int64_t* d_lens,
                      int32_t frame_length, int32_t hop_length, int32_t center, float* d_rms, void* stream);

/* Hilbert envelope (row N3): np.abs(scipy.signal.hilbert(x)) as called at script/calc.py:286 -- the DFT of the
 * clip at its own length n (any integer 1 .. 2^24), negative frequencies zeroed, positive ones doubled, the
 * inverse DFT, the magnitude -- for a batch of clips of one length.  A length of the form 2^a 3^b 5^c 7^d (>= 16:
 * sample counts such as 160 000, 441 000, 480 000) is transformed DIRECTLY by the library's mixed-radix Stockham FFT
 * (radix 16 / 8 / 4 / 2 / 9 / 3 / 25 / 5 / 49 / 7 passes, pairs of radix-16 or radix-25 passes fused into one
 * launch): mm_hilbert_fft_size() == n.  Any other length goes through Bluestein's chirp-z identity over a
 * power-of-two FFT of mm_hilbert_fft_size() = M >= 2n - 1 points.  Transforms run in the clips' own precision like
 * scipy (dtype 0: float32 / complex64, 1: float64 / complex128).
 * Two clips share one complex transform (clip 2r in the real part, 2r + 1 in the imaginary part: the spectrum mask is
 * linear, so the masked inverse transform returns (a - H b) + i (H a + b), and with a and b at hand both analytic
 * signals follow); each clip is scaled by a power of two first (exact), so a quiet clip next to a loud one keeps its
 * own relative accuracy, and a clip of zeros comes out as zeros.  A call with a single clip transforms it alone.
 * mm_hilbert_create allocates and fills the constant device tables on the current device (and synchronises);
 * mm_hilbert_envelope is asynchronous on `stream`: d_x [rows][x_stride] -> d_env [rows][env_stride], rows <=
 * 65535 per call, workspace = mm_hilbert_workspace_bytes(rows) = two [ceil(rows / 2)][fft_size] complex buffers and the
 * clips' scale factors -- size it with that call, not from n (fft_size is n on the direct path, M on the Bluestein
 * path). */
typedef struct mm_hilbert mm_hilbert;
int mm_hilbert_create(int64_t n, int32_t dtype, mm_hilbert** out);
void mm_hilbert_destroy(mm_hilbert* h);
int64_t mm_hilbert_fft_size(const mm_hilbert* h);
size_t mm_hilbert_workspace_bytes(const mm_hilbert* h, int64_t rows);
int mm_hilbert_envelope(mm_hilbert* h, const void* d_x, int64_t rows, int64_t x_stride, void* d_env,
                        int64_t env_stride, void* d_workspace, size_t ws_bytes, void* stream);
/* The Hilbert envelope of a ragged batch (no reference site: the reference takes one clip per call): d_x [rows][x_stride]
 * padded to n_max samples and d_lens (DEVICE, int64 [rows]), clamped by the kernels into [1, n_max] -> d_env [rows]
 * [env_stride]: row b holds |scipy.signal.hilbert(x[b, :n_b])| in [0, n_b) and +0.0 in [n_b, n_max).  scipy's DFT runs at
 * the clip's own length, so every row goes through Bluestein's identity with its OWN chirp exp(-i pi k^2 / n_b) over one
 * shared power-of-two FFT: mm_hilbert_ragged_create(n_max, dtype) fixes M = 2^p >= max(16, 2 n_max - 1) (mm_hilbert_
 * fft_size) and owns the twiddle tables of M only, so one handle serves every call whose n_max it covers (2 n_max - 1 <=
 * M), whatever the lengths.  Per call: the rows' chirps and wrapped chirps (integers k^2 mod 2 n_b, sincospi in float64,
 * rounded once), their spectra by one batched FFT in the clips' precision, then the four transforms of the chirp branch
 * of mm_hilbert_envelope with one clip per transform (two clips could share one only if they shared a chirp).  Nothing at
 * or behind n_b is read; a NaN or an infinity inside a clip makes that row NaN in [0, n_b) and touches no other row.
 * The clips are transformed unscaled (mm_hilbert_envelope's power-of-two scaling serves its pairing): the unnormalised
 * transforms reach max(envelope) n_b M, so a float32 clip stays finite where scipy does only while that product is below
 * 3.4e38: amplitudes up to about 1e27 at 160 000 samples (M = 2^19), 6e23 at 2^24 samples; float64: no practical limit.
 * Asynchronous on `stream`, no allocation, rows <= 65535; workspace = mm_hilbert_ragged_workspace_bytes(h, rows, n_max) =
 * three [rows][M] complex buffers, the [rows][n_max] chirps and a flag per row (0 for invalid arguments; MM_ERR_WORKSPACE
 * below it).  A ragged handle is not taken by mm_hilbert_envelope / mm_hilbert_rfft_f32, nor the other way round. */
int mm_hilbert_ragged_create(int64_t n_max, int32_t dtype, mm_hilbert** out);
size_t mm_hilbert_ragged_workspace_bytes(const mm_hilbert* h, int64_t rows, int64_t n_max);
int mm_hilbert_envelope_ragged(mm_hilbert* h, const void* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                               const int64_t* d_lens, void* d_env, int64_t env_stride, void* d_workspace, size_t ws_bytes,
                               void* stream);
/* rFFT of real float32 rows zero-padded to the plan's length n (a plan of dtype 0 whose length is even and 2 / 3 / 5 / 7-
 * smooth, i.e. mm_hilbert_fft_size() == n): d_x [rows][x_stride] with n_valid <= n samples each -> d_out complex64
 * [rows][n / 2 + 1] -- the trajectory rFFT (np.fft.rfft(mfcc, n, axis=-1), row A8 of the hot path) for clips with more
 * than 8192 frames, which mm_modspec_f32 does not take: one recording at the reference's default 1 ms step
 * (script/mfcc.py:296) is 10 001 frames per ten seconds.  rows <= 65535 per call; asynchronous on `stream`. */
size_t mm_hilbert_rfft_workspace_bytes(const mm_hilbert* h, int64_t rows);
int mm_hilbert_rfft_f32(mm_hilbert* h, const float* d_x, int64_t rows, int64_t x_stride, int64_t n_valid, float* d_out,
                        void* d_ws, size_t ws_bytes, void* stream);

/* Input side (row N4): what librosa.load(path, sr=sigSr, mono=False) does before the hot path
 * (script/mfcc.py:284,373).
 * mm_pcm_decode_f32: interleaved little-endian PCM frames (device copy of a WAV data chunk) -> planar
 *   float32 [channels][out_stride]; fmt 1 = u8, 2 = s16, 3 = packed s24, 4 = s32, 5 = f32, 6 = f64; scaled to
 *   [-1, 1) as libsndfile does.
 * mm_resample_f32: rational-ratio (L / M) polyphase FIR sample-rate conversion, zero-phase, n_out =
 *   ceil(n_in * L / M) as librosa.resample returns; d_taps = DEVICE pointer to the low-pass taps (DC gain L) in
 *   OUTPUT-phase order, records of four: taps[j / 4][t][j % 4] = h[ph_t + j * L] with ph_t = (t * M + half_len)
 *   mod L the polyphase branch of the t-th output of a period (taps_per_phase a multiple of 4, zero padded; 16-byte
 *   aligned), half_len = (len(h) - 1) / 2; rows <= 65535.  The host
 *   designs h (modulation_mfcc_amd/audio_io.py: a Kaiser-windowed sinc of soxr-HQ class: pass band to 0.913 of
 *   the lower Nyquist, > 120 dB stop band); the reference's resampler is soxr_hq, whose coefficients are not
 *   public API, so outputs agree with it to the quality of both filters, not bit for bit. */
int mm_pcm_decode_f32(const void* d_raw, int32_t fmt, int32_t channels, int64_t n_frames, float* d_out,
                      int64_t out_stride, void* stream);
int mm_resample_f32(const float* d_x, int64_t rows, int64_t n_in, int64_t x_stride, const float* d_taps,
                    int32_t L, int32_t M, int32_t taps_per_phase, int64_t half_len, float* d_y, int64_t n_out,
                    void* stream);
/* mm_resample_banded_f32: the same conversion as a banded GEMM on the matrix pipe (v_mfma_f32_16x16x4_f32: exact float32
 *   products, float32 accumulation in tap order; measured within 8e-7 of full scale of the float64 accumulation of mm_resample_f32) -- the
 *   default of audio_io.resample_batch.  Outputs m = q F + 16 b + r (F >= 16 a multiple of L: a period of outputs with
 *   the same taps; b < NB = ceil(F / 16); r < 16, 16 b + r < F) read the window x[q S + lo_min + lo_off[b] + k], S = F M / L, k < 4 ksteps, through
 *   d_atab [NB][ksteps / 4][64][4] (16-byte aligned; ksteps a multiple of 8): entry (b, ks / 4, lane, ks % 4) = the tap
 *   of row r = lane % 16 at window sample k = 32 (ks / 8) + KOFF[lane / 16] + ks % 8, KOFF = {0, 16, 8, 24} (zero
 *   outside the row's taps_per_phase taps); win = max_b lo_off[b] + 4 ksteps.  The host builds both tables
 *   (audio_io.banded_tables).  Returns MM_ERR_UNSUPPORTED when one tile of 16 periods does not fit the LDS
 *   (S + win > ~40 k samples): use mm_resample_f32 then. */
int mm_resample_banded_f32(const float* d_x, int64_t rows, int64_t n_in, int64_t x_stride, const float* d_atab,
                           const int32_t* d_lo_off, int32_t F, int32_t S, int32_t NB, int32_t ksteps, int32_t lo_min,
                           int32_t win, float* d_y, int64_t n_out, void* stream);
/* mm_resample_banded_shape: the launch shape mm_resample_banded_f32 would use for these tables -- *qt = periods per LDS
 *   tile / 16 (8, 4, 2 or 1), *pad = 1 when the tile carries one pad word per 32 (strides S that put the 16 periods of
 *   a read on few banks), *lds_bytes = the tile.  Host arithmetic only: no HIP call, no device needed; both entries
 *   go through the same helper.  MM_OK, MM_ERR_UNSUPPORTED (the tile of 16 periods exceeds the LDS: nothing is written)
 *   or MM_ERR_INVALID_ARG (NULL outputs, F < 16, S < 1, NB != ceil(F / 16), ksteps no positive multiple of 8,
 *   win < 4 ksteps). */
int mm_resample_banded_shape(int32_t F, int32_t S, int32_t NB, int32_t ksteps, int32_t win, int32_t* qt, int32_t* pad,
                             size_t* lds_bytes);

/* The input side for a LIST of files (audio_io.load_audio_batch): a padded batch with one length per row.
 *
 * mm_pcm_decode_ragged_f32: d_raw = ONE device buffer of raw_bytes bytes holding the data chunks of n_files files,
 *   d_recs = one mm_wav_rec per file (device): the byte offset of the file's data in d_raw (a multiple of 16 lets the
 *   16-bit / float32 mono and stereo files take 16-byte loads; any offset decodes), its frame count, the format code
 *   of mm_pcm_decode_f32, its channel count and the output row of its first channel.  ONE launch, whatever the mix of
 *   formats and channel counts: channel c of a file goes to row first_row + c of d_out [out_rows][out_stride], planar
 *   float32, every value bit for bit what mm_pcm_decode_f32 writes; columns [n_frames, max_frames) of those rows are
 *   +0.0 (no memset needed), columns beyond max_frames are not written.  No byte outside [byte_offset, byte_offset +
 *   n_frames * channels * bytes per sample) is read; a record whose range leaves the buffer, whose format is not 1 .. 6
 *   or whose frame count is negative decodes as an empty file (zeros), one whose rows leave [0, out_rows) is skipped.
 *   Frames beyond max_frames are cut.  Rows must not be shared between records.
 * mm_resample_ragged_f32 / mm_resample_banded_ragged_f32: mm_resample_f32 / mm_resample_banded_f32 with one length per
 *   row: d_lens [rows] int64 (device).  Row b holds n_b = clamp(d_lens[b], 1, n_max) samples and gets n_out_b =
 *   ceil(n_b L / M) outputs (64-bit arithmetic; the banded entry computes it as ceil(n_b F / S), the same number):
 *   columns [0, n_out_b) of output row b are bit for bit what the single-length entry writes for x[b, :n_b] alone,
 *   columns [n_out_b, n_out_max) are +0.0.  n_out_max must be ceil(n_max L / M) (MM_ERR_INVALID_ARG otherwise), y_stride
 *   >= n_out_max is the output's row pitch.  Nothing at or behind x[b, n_b] is read, nothing outside [0, n_out_max) of
 *   a row is written.  Tables, the rows <= 65535 limit of the float64 kernel and MM_ERR_UNSUPPORTED of the banded one
 *   (nothing is written then) as in the single-length entries.  The launch shape is that of n_max: a tile of the
 *   banded kernel that lies wholly behind a row's outputs stages and multiplies nothing and stores its zeros. */
typedef struct mm_wav_rec {
  int64_t byte_offset; /* of the file's first frame in d_raw */
  int64_t n_frames;
  int32_t fmt;         /* 1 = u8, 2 = s16, 3 = packed s24, 4 = s32, 5 = f32, 6 = f64 */
  int32_t channels;
  int64_t first_row;   /* output row of channel 0 */
} mm_wav_rec;
int mm_pcm_decode_ragged_f32(const void* d_raw, int64_t raw_bytes, const mm_wav_rec* d_recs, int64_t n_files,
                             int64_t max_frames, float* d_out, int64_t out_rows, int64_t out_stride, void* stream);
int mm_resample_ragged_f32(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                           const float* d_taps, int32_t L, int32_t M, int32_t taps_per_phase, int64_t half_len,
                           float* d_y, int64_t n_out_max, int64_t y_stride, void* stream);
int mm_resample_banded_ragged_f32(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                                  const float* d_atab, const int32_t* d_lo_off, int32_t F, int32_t S, int32_t NB,
                                  int32_t ksteps, int32_t lo_min, int32_t win, float* d_y, int64_t n_out_max,
                                  int64_t y_stride, void* stream);

/* Measurement aid: float4 grid-stride device-to-device copy of n_floats (a multiple of 4; 16-byte
 * aligned pointers) on `stream` -- the practical HBM ceiling bench.py quotes beside the stage-isolated
 * rFFT figure.  No reference counterpart. */
int mm_devcopy_f32(const float* d_src, float* d_dst, int64_t n_floats, void* stream);

/* ---- pYIN f0 tracking (get_f0(method='pyin'), script/calc.py:386-592: librosa.pyin) ---------------- */
/* Parameters of one pyin call.  The host (modulation_mfcc_amd/pitch.py) derives every field with numpy, as librosa
 * does: min_period = max(floor(sr / fmax), 1), max_period = min(ceil(sr / fmin), frame_length - win_length - 1),
 * nbps = ceil(1 / resolution), n_bins = floor(12 nbps log2(fmax / fmin)) + 1, band_h = half-width of the
 * transition band, max_troughs >= (max_period - min_period + 2) / 2 + 1 (trough slots per frame record),
 * log_tiny = log(float64 tiny), log_p_init = {log(0 + tiny), log(1 / n_bins + tiny)}. */
typedef struct mm_pyin_params {
  double sr, fmin, fmax;
  double no_trough_prob;
  double log_tiny;
  double fill_na;          /* f0 of unvoiced frames (NaN by default)                                   */
  double log_p_init[2];    /* voiced, unvoiced                                                         */
  int32_t frame_length, win_length, hop_length;
  int32_t center;          /* 1: frame_length / 2 zeros each side (pad_mode='constant'); 0: no padding */
  int32_t min_period, max_period, n_thresholds, nbps;
  int32_t n_bins, band_h, max_troughs, reserved;
} mm_pyin_params;

/* Constant float64 tables, DEVICE pointers, built on the host with scipy / numpy. */
typedef struct mm_pyin_tables {
  const double* thresholds;  /* [n_thresholds + 1] linspace(0, 1)                                        */
  const double* beta_probs;  /* [n_thresholds] diff(beta.cdf(thresholds, *beta_parameters))             */
  const double* beta_cum;    /* [n_thresholds + 1] np.sum(beta_probs[:k])                                */
  const double* boltzmann;   /* [max_troughs + 1][max_troughs] boltzmann.pmf(k, lambda, N) at [N][k]     */
  const double* log_same;    /* [n_bins][2 band_h + 1] log(A + tiny) of source j - band_h + d, same voicing */
  const double* log_cross;   /* [n_bins][2 band_h + 1] the same across voicing                           */
  const double* freqs;       /* [n_bins] fmin 2 ** (k / (12 nbps))                                       */
} mm_pyin_tables;

/* MM_OK, MM_ERR_INVALID_ARG (fmin >= fmax, fmax > sr / 2, win_length >= frame_length,
 * max_period < min_period + 2, inconsistent derived fields) or MM_ERR_UNSUPPORTED (beyond the kernels' LDS:
 * max_troughs > 512, n_bins > ~800, win_length + max_period > ~8 k).  Host only. */
int mm_pyin_check(const mm_pyin_params* p);
/* 1 + (n + 2 (frame_length / 2) center - frame_length) / hop_length; 0 when the clip is too short. */
int64_t mm_pyin_num_frames(const mm_pyin_params* p, int64_t n);
/* Stage: the cumulative-mean-normalised difference rows of rows x n signals (dtype 0 = float32, 1 = float64;
 * [rows][x_stride]) -> d_cmnd float64 [rows][n_frames][max_period - min_period + 1]. */
int mm_pyin_cmnd(const mm_pyin_params* p, const void* d_x, int32_t dtype, int64_t rows, int64_t n, int64_t x_stride,
                 double* d_cmnd, void* stream);
/* Stage: CMND rows of `frames` frames -> per-frame records: d_count [frames], d_bins / d_probs [frames][max_troughs]
 * (the observation's nonzero voiced bins, ascending lag = descending bin, duplicates resolved as librosa assigns them)
 * and d_voiced_prob [frames]. */
int mm_pyin_candidates(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_cmnd, int64_t frames,
                       int32_t* d_count, int32_t* d_bins, double* d_probs, double* d_voiced_prob, void* stream);
/* Stage: banded Viterbi decode of rows x n_frames records -> d_states int32, d_f0 float64, d_voiced uint8
 * [rows][n_frames]; workspace = the int16 back-pointers. */
size_t mm_pyin_decode_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n_frames);
int mm_pyin_decode(const mm_pyin_params* p, const mm_pyin_tables* t, const int32_t* d_count, const int32_t* d_bins,
                   const double* d_probs, const double* d_voiced_prob, int64_t rows, int64_t n_frames, int32_t* d_states,
                   double* d_f0, uint8_t* d_voiced, void* d_ws, size_t ws_bytes, void* stream);
/* Whole path, signal -> (f0, voiced_flag, voiced_prob, states) per [rows][n_frames]; workspace from
 * mm_pyin_workspace_bytes (back-pointers + records of every frame, CMND scratch of at most 16 k frames). */
size_t mm_pyin_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n);
int mm_pyin_f32(const mm_pyin_params* p, const mm_pyin_tables* t, const float* d_x, int64_t rows, int64_t n,
                int64_t x_stride, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob, int32_t* d_states, void* d_ws,
                size_t ws_bytes, void* stream);
int mm_pyin_f64(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_x, int64_t rows, int64_t n,
                int64_t x_stride, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob, int32_t* d_states, void* d_ws,
                size_t ws_bytes, void* stream);
/* The whole path for clips of different lengths in one padded batch d_x [rows][x_stride >= n_max].  d_lengths: DEVICE
 * int64 [rows], the valid samples of each row, clamped by the kernels into [1, n_max] (as mm_mfcc_ragged_f32 does).  Row b
 * is computed as the clip of its first n_b samples alone: its own centre padding, its own last frame; the samples at and
 * behind n_b never enter a result, whatever they hold.  The outputs keep the padded frame space [rows][T_max], T_max =
 * mm_pyin_num_frames(p, n_max): row b holds T_b = mm_pyin_num_frames(p, n_b) frames (0 when center is off and n_b <
 * frame_length) and zeros in [T_b, T_max) of all four outputs.  d_frames: DEVICE int64 [rows], receives T_b; may be NULL.
 * The workspace follows T_max, not sum T_b: mm_pyin_ragged_workspace_bytes equals mm_pyin_workspace_bytes at n_max.
 * Nothing is allocated, nothing synchronises.  MM_ERR_INVALID_ARG: NULL d_lengths, and every case of mm_pyin_f32
 * (T_max < 1 among them); MM_ERR_WORKSPACE before any launch. */
size_t mm_pyin_ragged_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n_max);
int mm_pyin_ragged_f32(const mm_pyin_params* p, const mm_pyin_tables* t, const float* d_x, int64_t rows, int64_t n_max,
                       int64_t x_stride, const int64_t* d_lengths, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob,
                       int32_t* d_states, int64_t* d_frames, void* d_ws, size_t ws_bytes, void* stream);
int mm_pyin_ragged_f64(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_x, int64_t rows, int64_t n_max,
                       int64_t x_stride, const int64_t* d_lengths, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob,
                       int32_t* d_states, int64_t* d_frames, void* d_ws, size_t ws_bytes, void* stream);
/* interp_NAN(method='linear') (script/calc.py:345-385) of float64 rows: NaN samples get scipy interp1d's linear
 * interpolation between their valid neighbours, extrapolated from the first / last two valid samples at the ends.
 * Rows with fewer than two valid samples are copied unchanged (scipy raises; the host checks). d_y may equal d_x
 * only when the strides are equal. */
int mm_interp_nan_linear_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y, int64_t y_stride,
                             void* stream);
/* interp_NAN for the other kinds that need no solve over all knots (csrc/mm_interp.hip).  Valid samples are copied
 * through; a NaN sample i with the valid neighbours k1 < i < k2 gets
 *   PCHIP       the reference's end fix (a NaN first / last sample becomes a knot with the first / last valid value),
 *               then scipy's PchipInterpolator over the knots: weighted harmonic mean derivatives inside, the three-point
 *               formula with its two sign corrections at the end knots, the straight line for two knots;
 *   NEAREST / NEAREST_UP   the value of the closer of k1, k2, a tie going to k1 / to k2; the end value outside the knots;
 *   PREVIOUS / NEXT        the value at k1 / at k2, NaN where there is none (before the first / after the last valid sample);
 *   ZERO        PREVIOUS, but the first valid value before the first valid sample;
 *   SLINEAR     the straight line through k1 and k2, through the first / last two valid samples outside them
 * as scipy.interpolate.interp1d(kind, fill_value='extrapolate') does.  Rows are independent, n <= 2^31 - 1025.  A row with
 * no valid sample (SLINEAR: fewer than two) is copied unchanged: scipy raises, the host checks.  d_y may equal d_x when
 * the strides are equal.  Workspace: 32 bytes per segment of 1024 samples and 16 per row.  MM_ERR_INVALID_ARG (unknown
 * kind, NULL pointers, rows / n < 1, strides < n) or MM_ERR_WORKSPACE before any launch. */
enum {
  MM_INTERP_PCHIP = 0, MM_INTERP_NEAREST = 1, MM_INTERP_NEAREST_UP = 2, MM_INTERP_PREVIOUS = 3, MM_INTERP_NEXT = 4,
  MM_INTERP_ZERO = 5, MM_INTERP_SLINEAR = 6
};
size_t mm_interp_nan_workspace_bytes(int32_t kind, int64_t rows, int64_t n);
int mm_interp_nan_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y,
                      int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream);
/* Both interp_NAN entries with a count per row: d_counts, DEVICE int64 [rows], clamped by the kernels into [1, n_max].
 * Row b is the curve of its first c_b samples: a sample is valid when it is not NaN and its index is below c_b, "the last
 * sample" (the pchip end fix, the extrapolation from the last two valid samples, NEXT behind the last valid one) is
 * c_b - 1, and columns [c_b, n_max) of d_y are written as 0.  A row with too few valid samples below c_b is copied
 * unchanged in [0, c_b).  Workspace of the second: mm_interp_nan_workspace_bytes(kind, rows, n_max).  MM_ERR_INVALID_ARG
 * for NULL d_counts and the cases of the entries above; MM_ERR_WORKSPACE before any launch. */
int mm_interp_nan_linear_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                                    const int64_t* d_counts, double* d_y, int64_t y_stride, void* stream);
int mm_interp_nan_ragged_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                             const int64_t* d_counts, double* d_y, int64_t y_stride, void* d_ws, size_t ws_bytes,
                             void* stream);
/* The regrid of read_AG50x (script/calc.py:173-219): d_out[j][c] = scipy interp1d(t_in, y[:, c], 'linear')(t_out[j]) for
 * the float32 samples d_y [n][y_stride] (time-major, cols <= y_stride interleaved columns) -> float64 d_out [m][out_stride].
 * Per output time the index is scipy's: the first i with t_in[i] >= t (binary search of d_t_in, ascending), clipped to
 * [1, n - 1]; the two samples are subtracted in float32, divided by the float64 step t_in[i] - t_in[i - 1], and
 * slope * (t - t_in[i - 1]) + y[i - 1] is taken in float64 -- scipy's arithmetic for a float32 y.  Times outside t_in
 * extrapolate from the end interval.  MM_ERR_INVALID_ARG: NULL pointers, n < 2, cols or m < 1, strides < cols. */
int mm_regrid_linear_f32_f64(const float* d_y, int64_t n, int64_t cols, int64_t y_stride, const double* d_t_in,
                             const double* d_t_out, int64_t m, double* d_out, int64_t out_stride, void* stream);

/* ---- peaks and troughs (MinMaxFinder, script/calc.py:651-686: scipy.signal.find_peaks) --------------- */
/* Conditions of one call, each an interval [min, max] with -INFINITY / +INFINITY for an open side (scipy's None:
 * that side is not tested); an interval counts only when its use_ flag is set.  negate: the peaks of -x (troughs). */
typedef struct mm_peaks_opts {
  double height[2];        /* x[p] (of -x when negate)                                                  */
  double threshold[2];     /* min(x[p] - x[p-1], x[p] - x[p+1]) >= [0], max(...) <= [1]; NaN propagates  */
  double prominence[2];    /* scipy's peak_prominences with wlen=None                                   */
  int32_t negate, use_height, use_threshold, use_prominence;
} mm_peaks_opts;

/* scipy.signal.find_peaks of rows x n curves (dtype 0 = float32, promoted per element, 1 = float64; [rows][x_stride],
 * x_stride >= n), conditions applied in scipy's order: height, threshold, prominence.  d_lo / d_hi (int32 [rows],
 * either may be NULL = 0 / n; clamped to 0 <= lo <= hi <= n) restrict row r to the slice x[lo:hi]: indices and bases
 * are relative to lo, the slice's ends are never peaks, the prominence scan stays inside it.
 * d_count [rows] = the TRUE number of peaks; d_idx [rows][cap] = their plateau midpoints, ascending, -1 beyond
 * min(count, cap) (peaks beyond cap are dropped, never written).  cap = (n - 1) / 2 always suffices.  With
 * use_prominence, d_prom (NaN-padded), d_lbase, d_rbase [rows][cap] are written too (NULL otherwise).
 * Workspace: segment counts and the candidate list of the prominence pass (20 bytes per possible peak).
 * MM_ERR_INVALID_ARG (NULL pointers, rows / n < 1, x_stride < n, NaN bounds) or MM_ERR_WORKSPACE before any launch. */
size_t mm_find_peaks_workspace_bytes(int64_t rows, int64_t n);
int mm_find_peaks(const mm_peaks_opts* opts, const void* d_x, int32_t dtype, int64_t rows, int64_t n, int64_t x_stride,
                  const int32_t* d_lo, const int32_t* d_hi, int64_t cap, int32_t* d_count, int32_t* d_idx, double* d_prom,
                  int32_t* d_lbase, int32_t* d_rbase, void* d_ws, size_t ws_bytes, void* stream);

/* The remaining conditions of scipy.signal.find_peaks, beside mm_peaks_opts: plateau_size and width are intervals like
 * the others, distance is scipy's ceil(distance) >= 1, wlen its ceil(wlen) >= 2 (<= 0: no window) and is looked at only
 * when the prominence is computed, rel_height >= 0 that of peak_widths.  A zeroed struct asks for nothing. */
typedef struct mm_peaks_ext {
  double plateau_size[2];  /* right_edge - left_edge + 1                                                 */
  double width[2];         /* scipy's peak_widths at rel_height, prominences taken inside wlen           */
  double rel_height;
  int32_t distance, wlen, use_plateau_size, use_distance, use_width;
} mm_peaks_ext;

/* Device outputs of mm_find_peaks_ex: count [rows], every other array [rows][cap], padded like d_idx (integers -1,
 * doubles NaN).  NULL = not wanted, except count and (cap > 0) idx; prom, lbase and rbase are required when
 * use_prominence or use_width is set.  An array of a condition that is not used is left untouched. */
typedef struct mm_peaks_out {
  int32_t* count;
  int32_t* idx;
  double* prom;
  int32_t* lbase;
  int32_t* rbase;
  double* widths;
  double* width_heights;
  double* left_ips;
  double* right_ips;
  int32_t* plateau_sizes;
  int32_t* left_edges;
  int32_t* right_edges;
} mm_peaks_out;

/* mm_find_peaks with every condition of scipy.signal.find_peaks, applied in its order: plateau_size, height, threshold,
 * distance, prominence, width.  ext == NULL, or an ext that uses none of its conditions, is mm_find_peaks itself: the
 * same kernels and the same workspace.  Otherwise the conditions run as stages over the candidate list of the workspace
 * (64 bytes per possible peak): distance is scipy's greedy selection (of two equally high peaks nearer than distance the
 * one with the LARGER index survives -- scipy leaves that to an unstable sort), all its rounds in one launch; the
 * prominence window is [p - wlen / 2, p + wlen / 2] clipped to the slice; widths, width heights and interpolated
 * positions (relative to lo) equal scipy's peak_widths bit for bit.  Status codes, the true count beyond cap and the
 * checks before any launch are those of mm_find_peaks; a NaN bound, use_distance with distance < 1, wlen == 1 or
 * rel_height < 0 is MM_ERR_INVALID_ARG as well. */
size_t mm_find_peaks_ex_workspace_bytes(const mm_peaks_opts* opts, const mm_peaks_ext* ext, int64_t rows, int64_t n);
int mm_find_peaks_ex(const mm_peaks_opts* opts, const mm_peaks_ext* ext, const void* d_x, int32_t dtype, int64_t rows,
                     int64_t n, int64_t x_stride, const int32_t* d_lo, const int32_t* d_hi, int64_t cap,
                     const mm_peaks_out* out, void* d_ws, size_t ws_bytes, void* stream);

/* ---- per-kernel device timing (hipEvents on the launch stream) ------------------------- */
/* on = 0: off; 1: every stage; otherwise a mask with bit (MM_STAGE_x + 1) set for each stage to time
 * (two hipEventRecord per timed launch: timing fewer stages perturbs the stream less). */
int mm_timing_enable(mm_plan* plan, int on);
/* synchronises the recorded events; ms_sum[s]/count[s] = average launch duration of stage s;
 * resets the accumulators. Arrays of MM_NUM_STAGES. */
int mm_timing_read(mm_plan* plan, double* ms_sum, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* MODMFCC_H */
