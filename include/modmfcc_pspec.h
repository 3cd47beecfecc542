/*
 * modmfcc_pspec.h -- seventh header of libmodmfcc.so: the Praat-style spectrogram of sounds on the device.
 *
 *   mm_pspec_f32 / _f64  <- script/praat_py_ui/parselmouth_calc.py:31-39, Sound.to_spectrogram(): the power in bands of
 *                           short Gaussian-windowed (or other) frames whose centres need not lie on the sample grid
 *
 * The contract is that of the other side headers: device pointers owned by the caller, asynchronous on the caller's
 * stream, no allocation and no synchronisation (graph-capture safe), MM_OK or a negative mm_status; every refusal comes
 * before the first launch.  The entries take no workspace.
 *
 * The host does the framing arithmetic (modulation_mfcc_amd/pspec.py): the window of nw samples, the
 * transform length nfft, the band width bw in bins, the band count n_freqs, the scale 1 / (sum w^2) / bw and, per row, the
 * first sample of every frame.  The device does, per listed frame k of row r with s = d_start[r][k]:
 *   X        = the real transform of x[r][c][s .. s + nw) * d_w, zero-filled to nfft, per channel c, in the entry's type
 *   P[b]     = sum over the channels of |X[b]|^2, b < n_freqs * bw (the bins behind are never formed), in float64
 *   y[r][j][k] = (sum of P[j bw .. (j + 1) bw), ascending) / channels * scale, in float64, rounded once to the entry's type;
 *                with MM_PSPEC_DB 10 log10 of it, in float64, rounded once (-inf for a band without power: a silent frame)
 * An entry with s < 0 or s + nw > n_max -- the -1 behind a row's last frame, or a table the caller got wrong -- reads
 * nothing and writes +0.0 in every band (with MM_PSPEC_DB too: no frame, no level).  All of d_y[r][j][0 .. t_max) is
 * written.
 *
 * What is read: only samples of [s, s + nw) of a listed frame reach a result.  The workgroup's staged copy reads MORE of
 * the row than that -- every sample from the lowest first sample of a tile's valid entries on, up to `span` samples and
 * never at or behind n_max: the gaps between frames that are out of order and, in a ragged batch, what lies behind the
 * clip's own length up to n_max.  Those values are loaded and never used (NaN there changes no bit); every index of
 * [0, n_max) of every row and channel must therefore be readable memory.
 *
 * A row's result depends on its own samples and table entries only: not on the batch, the strides, the row's index or on
 * what lies behind its length.  A frame's values are the same whether its samples came through the workgroup's staged copy
 * or straight from memory.
 *
 * Limits: 32 <= nfft <= 4096, a power of two; 2 <= nw <= nfft; 1 <= bw; 1 <= n_freqs; n_freqs * bw <= nfft / 2;
 * 1 <= channels <= 8 (MM_ERR_UNSUPPORTED otherwise); scale finite and > 0; 0 <= span; no flag but MM_PSPEC_DB; 1 <= rows, 1 <= t_max,
 * nw <= n_max < 2^31 - 4096; rows * ceil(t_max / tile) < 2^31; x_channel_stride >= n_max, x_row_stride >= channels *
 * x_channel_stride or (rows == 1) anything, y_band_stride >= t_max, y_row_stride >= n_freqs * y_band_stride,
 * start_row_stride 0 (one table for all rows) or >= t_max.
 */
#ifndef MODMFCC_PSPEC_H
#define MODMFCC_PSPEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_PSPEC_VERSION 100
#define MM_PSPEC_MAX_NFFT 4096
#define MM_PSPEC_MAX_CHANNELS 8

enum { MM_PSPEC_DB = 1 };                                                             /* flags */

typedef struct mm_pspec_params {
  double scale;        /* 1 / (sum of the squared window) / bw */
  int32_t nw;          /* samples of the window, even */
  int32_t nfft;        /* transform length */
  int32_t bw;          /* bins per band */
  int32_t n_freqs;     /* bands */
  int32_t channels;
  int32_t span;        /* samples from the first sample of a tile's first frame to the last of its last frame, the largest
                          over the tiles: what a workgroup copies to LDS once (capped by the kernel; frames that do not
                          fit are read from memory, 0 reads every frame from memory) */
  int32_t flags;       /* 0 or MM_PSPEC_DB */
  int32_t reserved;    /* 0 */
} mm_pspec_params;

int mm_pspec_version(void);

/* MM_OK, MM_ERR_INVALID_ARG or MM_ERR_UNSUPPORTED for the limits above that concern p alone */
int mm_pspec_check(const mm_pspec_params* p);

/* consecutive frames of a row that one workgroup owns (a power of two; tile t holds frames t * tile .. ); < 0: the status
 * of mm_pspec_check */
int32_t mm_pspec_tile_frames(const mm_pspec_params* p);

/* d_x [rows][channels][n_max] (strides in elements), d_w [nw] in the entry's type, d_start int32 [rows or 1][t_max]
 * -> d_y [rows][n_freqs][t_max] */
int mm_pspec_f32(const mm_pspec_params* p, const float* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                 int64_t x_channel_stride, const float* d_w, const int32_t* d_start, int64_t t_max,
                 int64_t start_row_stride, float* d_y, int64_t y_row_stride, int64_t y_band_stride, void* stream);
int mm_pspec_f64(const mm_pspec_params* p, const double* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                 int64_t x_channel_stride, const double* d_w, const int32_t* d_start, int64_t t_max,
                 int64_t start_row_stride, double* d_y, int64_t y_row_stride, int64_t y_band_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
