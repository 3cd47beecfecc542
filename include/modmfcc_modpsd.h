/*
 * modmfcc_modpsd.h -- second header of libmodmfcc.so: the Welch modulation power spectrum.
 *
 *   mm_modpsd_f32  <- scipy.signal.welch(x, fs, window, nperseg, noverlap, nfft, detrend, return_onesided=True, scaling,
 *                     axis=-1, average='mean') on a batch of float32 rows (MFCC trajectories, RMS envelopes, any curve),
 *                     with one length per row where the caller has one (build-defined; no reference site)
 *
 * The contract is that of modmfcc.h: device pointers owned by the caller, asynchronous on the caller's stream, no
 * allocation and no synchronisation in a compute call (graph-capture safe), MM_OK or a negative mm_status.  The handle owns
 * constant device tables only (window, twiddles) and is bound to the device current at creation; one handle may be used by
 * several threads, each with its own buffers, workspace and stream.
 *
 * Semantics.  step = nperseg - noverlap; a row of n samples has K = (n - noverlap) / step segments (integer division) that
 * start at i * step; nothing behind the last full segment is used, nothing is padded.  Each segment is detrended (0: not,
 * 1: its mean subtracted, 2: its least-squares line subtracted -- both in float64, the result rounded to float32),
 * multiplied by the window, zero-padded to nfft and transformed;
 *     P[k] = s * d[k] * mean_i |X_i[k]|^2,   s = 1 / (fs * sum w^2) ('density')  or  1 / (sum w)^2 ('spectrum'),
 *     d[k] = 2 except at k = 0 and k = nfft / 2,   k = 0 .. nfft / 2   at the frequencies k * fs / nfft.
 * The mean over segments is accumulated in float64, in an order that depends on the segment's index within its row only:
 * a row's result does not change with the batch it is computed in.
 *
 * Limits: nfft a power of two in [32, 4096]; 1 <= nperseg <= nfft; 0 <= noverlap < nperseg; detrend 0 / 1 / 2; scaling
 * 0 / 1; fs > 0 and finite.  A row shorter than nperseg has no segment: its result is NaN (scipy would shrink nperseg).
 */
#ifndef MODMFCC_MODPSD_H
#define MODMFCC_MODPSD_H

#include "modmfcc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mm_modpsd_params {
  double fs;
  int32_t nperseg, noverlap, nfft;
  int32_t detrend;      /* 0 none, 1 constant, 2 linear */
  int32_t scaling;      /* 0 density, 1 spectrum */
  int32_t reserved[3];  /* 0 */
} mm_modpsd_params;

typedef struct mm_modpsd mm_modpsd;

int mm_modpsd_version(void); /* 1 */

/* MM_OK, MM_ERR_INVALID_ARG (a value that is never valid) or MM_ERR_UNSUPPORTED (an nfft this build has no kernel for) */
int mm_modpsd_check(const mm_modpsd_params* p);

/* segments of a row of n samples; 0 for n < nperseg; MM_ERR_INVALID_ARG for invalid parameters */
int64_t mm_modpsd_num_segments(const mm_modpsd_params* p, int64_t n);

/* window_host: nperseg float32 values on the HOST.  MM_ERR_INVALID_ARG for a window with a non-finite value, with
 * sum w^2 = 0, or with sum w = 0 under 'spectrum'. */
int mm_modpsd_create(const mm_modpsd_params* p, const float* window_host, mm_modpsd** out);
void mm_modpsd_destroy(mm_modpsd* h);

/* Bytes of workspace mm_modpsd_f32 needs for `rows` rows of up to n_max samples (0 where a row of n_max samples has at
 * most MM_MODPSD_CHUNK segments: one launch, no workspace; also 0 for invalid arguments). */
size_t mm_modpsd_workspace_bytes(const mm_modpsd* h, int64_t rows, int64_t n_max);

#define MM_MODPSD_CHUNK 32 /* segments per workgroup: segment i of a row belongs to chunk i / 32, wave i % 4 of it */

/* d_x [rows][x_stride] float32, x_stride >= n_max; d_lens: int64 [rows] on the device, clamped into [1, n_max] there, or
 * NULL (every row has n_max samples; n_max < nperseg is then MM_ERR_INVALID_ARG); d_psd [rows][psd_stride] float32,
 * psd_stride >= nfft / 2 + 1, nothing behind the nfft / 2 + 1 values of a row is written.  d_ws: 8-byte aligned, may be
 * NULL when mm_modpsd_workspace_bytes is 0.  One launch, two where a row may have more than MM_MODPSD_CHUNK segments. */
int mm_modpsd_f32(const mm_modpsd* h, const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                  const int64_t* d_lens, float* d_psd, int64_t psd_stride, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
