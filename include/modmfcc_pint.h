/*
 * modmfcc_pint.h -- eighth header of libmodmfcc.so: Praat's intensity contour of sounds on the device.
 *
 *   mm_pint_f32 / _f64   <- script/calc.py:131-170 and :292-324, script/mfcc.py:214-233: Sound.to_intensity() and
 *                           call(sound, "To Intensity", minimum_pitch, time_step, subtract_mean): the mean-centred power
 *                           under a Kaiser-like window, one value per frame, frames the host lists by their centre sample
 *   mm_pint_value_f64    <- Intensity.get_value(time): Vector_getValueAtX at depth 0, 1 and 2
 *
 * The contract is that of the other side headers: device pointers owned by the caller, asynchronous on the caller's
 * stream, no allocation and no synchronisation (graph-capture safe), MM_OK or a negative mm_status; every refusal comes
 * before the first launch.  The entries take no workspace.
 *
 * The host does the framing arithmetic (modulation_mfcc_amd/pint.py): the half width hw, the window
 * w[-hw .. hw] (d_w[i + hw], float64 whatever the samples' type) and, per row, the centre sample of every frame.  The
 * device does, per listed frame k of row r with c = d_centre[r][k] and len = the row's length (d_len[r] clamped to
 * [0, n_max]; n_max where d_len is NULL), all of it in float64:
 *   l = max(0, c - hw), r = min(len - 1, c + hw)
 *   per channel:  m = (sum of x[l .. r]) / (r - l + 1), or 0 with MM_PINT_KEEP_MEAN
 *                 sxw += sum over j = l .. r of (x[j] - m)^2 w[j - c]
 *   sw = sum over j = l .. r of w[j - c];   P = sxw / (sw * channels)
 *   d_y[r][k] = P < 4e-40 ? -300 : 10 log10(P / 4e-10);  with MM_PINT_LINEAR, P itself
 * Every sum is taken in the order DESIGN.md section 20 states, a function of c, l, r and hw alone.
 * An entry with c < 0 or c >= len -- the -1 behind a row's last frame, or a table the caller got wrong -- reads nothing
 * and writes +0.0.  All of d_y[r][0 .. t_max) is written.  Nothing at or behind a row's length is read.
 *
 * A row's result depends on its own samples, length and table entries only: not on the batch, the strides, the row's
 * index, the entry's place in the table or on whether a frame's samples came through the workgroup's staged copy.
 *
 * Limits: 1 <= hw <= MM_PINT_MAX_HALF, 1 <= channels <= MM_PINT_MAX_CHANNELS (MM_ERR_UNSUPPORTED above them), 0 <= span,
 * no flag but MM_PINT_LINEAR | MM_PINT_KEEP_MEAN, reserved 0; 1 <= rows, 1 <= t_max < 2^31, 1 <= n_max < 2^31 - 2^15;
 * rows * ceil(t_max / tile) < 2^31; x_channel_stride >= n_max, x_row_stride >= channels * x_channel_stride or (rows == 1)
 * anything, y_row_stride >= t_max, centre_row_stride 0 (one table for all rows) or >= t_max.
 */
#ifndef MODMFCC_PINT_H
#define MODMFCC_PINT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_PINT_VERSION 100
#define MM_PINT_MAX_HALF 16384
#define MM_PINT_MAX_CHANNELS 8

enum { MM_PINT_LINEAR = 1, MM_PINT_KEEP_MEAN = 2 };                                   /* flags */
enum { MM_PINT_NEAREST = 0, MM_PINT_LINEAR_INTERP = 1, MM_PINT_CUBIC = 2 };           /* depth of mm_pint_value_f64 */

typedef struct mm_pint_params {
  int32_t hw;          /* taps on either side of a frame's centre sample: the window has 2 hw + 1 */
  int32_t channels;
  int32_t span;        /* samples from the first sample of a tile's first frame to the last of its last frame, the largest
                          over the tiles: sizes what a workgroup copies to LDS (capped by the kernel; frames that do not
                          lie in the copy are read from memory, 0 reads every frame from memory) */
  int32_t flags;       /* MM_PINT_LINEAR: Pa^2 instead of dB; MM_PINT_KEEP_MEAN: subtract_mean=False */
  int32_t reserved;    /* 0 */
} mm_pint_params;

int mm_pint_version(void);

/* MM_OK, MM_ERR_INVALID_ARG or MM_ERR_UNSUPPORTED for the limits above that concern p alone */
int mm_pint_check(const mm_pint_params* p);

/* consecutive table entries of a row that one workgroup owns (a power of two; tile t holds entries t * tile .. ); < 0: the
 * status of mm_pint_check */
int32_t mm_pint_tile_frames(const mm_pint_params* p);

/* d_x [rows][channels][n_max] (strides in elements), d_w [2 hw + 1] float64, d_centre int32 [rows or 1][t_max], d_len
 * int64 [rows] or NULL -> d_y [rows][t_max] float64 */
int mm_pint_f32(const mm_pint_params* p, const float* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                int64_t x_channel_stride, const double* d_w, const int32_t* d_centre, int64_t t_max,
                int64_t centre_row_stride, const int64_t* d_len, double* d_y, int64_t y_row_stride, void* stream);
int mm_pint_f64(const mm_pint_params* p, const double* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                int64_t x_channel_stride, const double* d_w, const int32_t* d_centre, int64_t t_max,
                int64_t centre_row_stride, const int64_t* d_len, double* d_y, int64_t y_row_stride, void* stream);

/* The contour's value at times: d_y [rows][t_max], row r holding d_frames[r] values (NULL: t_max; clamped to [0, t_max])
 * at d_t1[r] + k time_step; d_q [rows or 1][n_q] query times (q_row_stride 0: one list for all rows, or >= n_q) ->
 * d_out [rows][n_q].  NaN outside [t1 - dt / 2, t1 - dt / 2 + T dt] and for a row without a frame. */
int mm_pint_value_f64(const double* d_y, int64_t rows, int64_t t_max, int64_t y_row_stride, const int64_t* d_frames,
                      const double* d_t1, double time_step, const double* d_q, int64_t n_q, int64_t q_row_stride,
                      int32_t depth, double* d_out, int64_t out_row_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
