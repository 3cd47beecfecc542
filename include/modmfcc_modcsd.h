/*
 * modmfcc_modcsd.h -- third header of libmodmfcc.so: the Welch cross spectrum and coherence of pairs of rows.
 *
 *   mm_modcsd_f32  <- scipy.signal.csd(x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided=True, scaling,
 *                     axis=-1, average='mean'), scipy.signal.coherence of the same arguments and scipy.signal.welch of
 *                     either side, on a batch of pairs of float32 rows with one length per pair, in one launch
 *                     (build-defined; no reference site)
 *
 * The handle is that of the second header (mm_modpsd_create / mm_modpsd_destroy: window, twiddles, scale, parameters); the
 * contract is that of the other two headers: device pointers owned by the caller, asynchronous on the caller's stream, no
 * allocation and no synchronisation in the compute call (graph-capture safe), MM_OK or a negative mm_status; one handle may
 * be used by several threads, each with its own buffers, workspace and stream.
 *
 * Pairs.  Pair r is row r of x with row r / y_group of y (integer division, y_group >= 1): with y_group = 13 the thirteen
 * trajectories of a clip share the clip's one envelope row and nothing is copied.  The pair has ONE length,
 * clamp(d_lens[r], 1, n_max), or n_max when d_lens is NULL; exactly x[r][0 : len) and y[r / y_group][0 : len) are read.
 *
 * Semantics.  Segments, detrend (float64, rounded to float32), window, zero padding and the frequency grid are those of
 * modmfcc_modpsd.h, word for word, applied to both sides.  With X_i, Y_i the float32 transforms of segment i of either side
 * (one complex transform of w x + i w y, split into the two), s and d[k] as in modmfcc_modpsd.h, K the segment count:
 *     Pxx[k] = s d[k] mean_i |X_i[k]|^2        Pyy[k] = s d[k] mean_i |Y_i[k]|^2
 *     Pxy[k] = s d[k] mean_i conj(X_i[k]) Y_i[k]                                   (scipy's convention: conjugate on x)
 *     coh[k] = |sum_i conj(X_i[k]) Y_i[k]|^2 / (sum_i |X_i[k]|^2  sum_i |Y_i[k]|^2)
 * Before the transform either side of a segment is scaled by a power of two to a norm in [1, 2), and the power is undone in
 * float64 behind it (both exact): the float32 rounding error of each side is relative to that side, however loud the other
 * one is.  A side that is all zeros in a segment contributes exact zeros to Pxx / Pyy / Pxy.
 * The products of a segment are formed in float64 from the float32 X_i, Y_i (exact: 24 x 24 bits) and the sums over the
 * segments are float64, in an order that depends on the segment's index within its row only: a pair's bits do not change
 * with the batch it is computed in, with y_group, or with what lies behind its length.  The coherence is taken from the
 * float64 sums before they are scaled or rounded: it never exceeds 1.0f, it is exactly 1.0f wherever it is defined for a
 * pair with one segment, and it is NaN where the denominator is 0 (scipy's 0 / 0).  A pair without a segment
 * (len < nperseg) is NaN in every output, both parts of Pxy included.
 *
 * Pxx and Pyy of this entry need NOT equal mm_modpsd_f32 bit for bit: that entry squares in float32 and transforms a
 * packed real row; both are within the same bound of scipy.signal.welch.
 *
 * Limits: those of modmfcc_modpsd.h, but nfft a power of two in [32, 2048]: a lane holds four float64 sums per bin.
 */
#ifndef MODMFCC_MODCSD_H
#define MODMFCC_MODCSD_H

#include "modmfcc_modpsd.h"

#ifdef __cplusplus
extern "C" {
#endif

int mm_modcsd_version(void); /* 1 */

/* as mm_modpsd_check; MM_ERR_UNSUPPORTED also for nfft = 4096 */
int mm_modcsd_check(const mm_modpsd_params* p);

/* Bytes of workspace mm_modcsd_f32 needs for `rows` pairs of up to n_max samples (0 where a row of n_max samples has at
 * most MM_MODPSD_CHUNK segments, for a handle mm_modcsd_check refuses and for invalid arguments). */
size_t mm_modcsd_workspace_bytes(const mm_modpsd* h, int64_t rows, int64_t n_max);

/* d_x [rows][x_stride] and d_y [ceil(rows / y_group)][y_stride] float32, both strides >= n_max; d_lens: int64 [rows] on the
 * device, clamped into [1, n_max] there, or NULL (every pair has n_max samples; n_max < nperseg is then
 * MM_ERR_INVALID_ARG).  d_pxx, d_pyy, d_coh [rows][out_stride] float32 and d_pxy [rows][out_stride][2] float32 (re, im),
 * out_stride >= nfft / 2 + 1 in bins for all four; nothing behind the nfft / 2 + 1 bins of a row is written.  Any of the
 * four may be NULL (not computed); all four NULL is MM_ERR_INVALID_ARG.  d_ws: 8-byte aligned, may be NULL when
 * mm_modcsd_workspace_bytes is 0.  A handle with nfft = 4096 is MM_ERR_UNSUPPORTED.  One launch, two where a row may have
 * more than MM_MODPSD_CHUNK segments. */
int mm_modcsd_f32(const mm_modpsd* h, const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const float* d_y,
                  int64_t y_stride, int64_t y_group, const int64_t* d_lens, float* d_pxx, float* d_pyy, float* d_pxy,
                  float* d_coh, int64_t out_stride, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
