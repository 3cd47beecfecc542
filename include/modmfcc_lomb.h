/*
 * modmfcc_lomb.h -- fifth header of libmodmfcc.so: the Lomb-Scargle (least-squares) modulation spectrum of curves with
 * holes, on the device.
 *
 *   mm_lombscargle_f64  <- (no reference site) scipy.signal.lombscargle(t[valid], x[r, valid], omega, precenter=,
 *                          normalize=, floating_mean=) of scipy 1.15 for every row r of a batch of float64 rows, where
 *                          `valid` are the non-NaN samples in front of the row's length: f0 curves that are NaN where the
 *                          clip is unvoiced, articulograph channels that are NaN where a sensor dropped out
 *
 * The contract is that of the other four headers: device pointers owned by the caller, asynchronous on the caller's
 * stream, no allocation and no synchronisation (graph-capture safe), MM_OK or a negative mm_status; every refusal comes
 * before the first launch and leaves the outputs untouched.
 *
 * Semantics (scipy 1.15, the generalised periodogram of Zechmeister & Kuerster).  The data points of row r are its valid
 * samples (t_j, x[r][j]); the weights are uniform, 1 / K_r with K_r the number of valid samples.  Per frequency: the tau
 * rotation that removes CS, CC and SS clamped to epsneg (2^-53), a = YC / CC, b = YS / SS, pgram = 2 (a YC + b YS), then
 *   MM_LOMB_POWER      pgram K_r / 4                      (normalize=False | 'power')
 *   MM_LOMB_NORMALIZE  pgram 0.5 / YY                     (normalize=True | 'normalize')
 *   MM_LOMB_AMPLITUDE  (a + i b) exp(i tau), real part to d_out, imaginary part to d_out_im   ('amplitude')
 * MM_LOMB_PRECENTER subtracts the mean of the row's valid samples first; MM_LOMB_FLOATING_MEAN fits an offset per
 * frequency (C, S, Y terms), both as scipy has them.  The arithmetic is float64 but not scipy's order of operations: the
 * sums of cos, sin, cos^2, cos sin, y cos, y sin over the valid samples are taken in one pass and rotated by tau
 * algebraically, so a result is within a few of scipy's own roundings of it, not equal bit for bit.
 *
 * Masking.  A sample that is NaN, or at or behind the row's length, contributes an exact zero whatever it holds (its
 * operand is selected, never multiplied).  An Inf in front of the length poisons its own row only.  A row without a
 * valid sample gets NaN in every output.  d_lengths: int64 [rows] on the device, clamped into [1, n_max] on the device;
 * NULL: every row has n_max samples.
 *
 * A row's result depends on its own samples, d_t and d_omega only: the samples are summed in chunks of
 * MM_LOMB_CHUNK, the chunks in ascending order, so a row has the same bits alone, anywhere in any batch, and with any
 * n_max and any contents behind its length.
 *
 * Limits: 1 <= rows <= 2^19, 1 <= n_max <= 2^30, 1 <= n_freq <= 2^20, rows * ceil(n_max / MM_LOMB_CHUNK) < 2^26,
 * rows * n_freq < 2^32 (a launch takes fewer than 2^32 threads), strides >= n_max resp. n_freq.  d_t and d_omega must be finite at EVERY index: the
 * cosines are generated for the batch, not per row, so a NaN or Inf time poisons every row, the rows that mask that sample
 * included.
 */
#ifndef MODMFCC_LOMB_H
#define MODMFCC_LOMB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_LOMB_VERSION 100 /* 1.0.0 */
#define MM_LOMB_CHUNK 512   /* samples a workgroup sums; longer rows go through the workspace and a finish kernel */

enum {
  MM_LOMB_PRECENTER = 1,
  MM_LOMB_FLOATING_MEAN = 2,
  MM_LOMB_POWER = 0 << 2,       /* the normalisation: bits 2-3 of flags */
  MM_LOMB_NORMALIZE = 1 << 2,
  MM_LOMB_AMPLITUDE = 2 << 2
};

int mm_lomb_version(void);

/* Bytes of workspace for `rows` rows of up to n_max samples at n_freq frequencies; 0 for invalid arguments. */
size_t mm_lombscargle_workspace_bytes(int64_t rows, int64_t n_max, int64_t n_freq);

/* d_x [rows][x_stride] float64, d_lengths int64 [rows] or NULL, d_t [n_max] float64 (seconds), d_omega [n_freq] float64
 * (rad/s) -> d_out [rows][out_stride] float64; d_out_im [rows][out_stride] float64 for MM_LOMB_AMPLITUDE (required
 * then, ignored otherwise).  d_ws: 256-byte aligned, ws_bytes >= the size above (MM_ERR_WORKSPACE for a NULL,
 * misaligned or short workspace).  MM_ERR_INVALID_ARG: NULL pointers, sizes outside the limits, short strides, unknown
 * flag bits, MM_LOMB_AMPLITUDE without d_out_im. */
int mm_lombscargle_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lengths,
                       const double* d_t, const double* d_omega, int64_t n_freq, int32_t flags, double* d_out,
                       int64_t out_stride, double* d_out_im, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
