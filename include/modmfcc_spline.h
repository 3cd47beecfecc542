/*
 * modmfcc_spline.h -- fourth header of libmodmfcc.so: interp_NAN's 'quadratic' and 'cubic' kinds on the device.
 *
 *   mm_interp_spline_f64  <- script/calc.py:379, interp1d(valid_indices, valid_values, kind, fill_value="extrapolate")
 *                            evaluated at the NaN indices, kind in ('quadratic', 'cubic'), on a batch of float64 rows
 *
 * The contract is that of mm_interp_nan_f64 / mm_interp_nan_ragged_f64 (include/modmfcc.h): device pointers owned by the
 * caller, asynchronous on the caller's stream, no allocation and no synchronisation (graph-capture safe), MM_OK or a
 * negative mm_status; every refusal comes before the first launch.
 *
 * Semantics (scipy 1.15).  The valid (non-NaN) samples of a row are the data points (x_j, y_j), j < K, x_j their indices.
 *   MM_SPLINE_CUBIC      make_interp_spline(k=3): the C2 cubic spline with not-a-knot conditions at x_1 and x_{K-2}
 *                        (interior knots x[2:-2]); K = 4 is one cubic.
 *   MM_SPLINE_QUADRATIC  make_interp_spline(k=2): the C1 quadratic spline whose interior knots are the midpoints
 *                        (x_i + x_{i+1}) / 2, i = 1 .. K-3 (the first and the last midpoint are no knots); K = 3 is one
 *                        parabola.
 * NaN samples before x_0 and behind x_{K-1} are extrapolated with the end pieces.  Valid samples are copied through.  A row
 * without a NaN, and a row with fewer than kind + 1 valid samples, is copied through as it is (the Python layer raises
 * scipy's error for the latter).  Either interpolant is unique; the arithmetic is float64 without contraction, but not
 * scipy's order of operations: the result is within a few of scipy's own roundings of it, not equal bit for bit.
 *
 * A row's result depends on its own samples only: not on the batch, on n_max, or on what lies behind its count.
 *
 * Ragged form: row r has clamp(d_counts[r], 1, n_max) samples; the columns behind them are written as +0.0 and never read
 * as samples.
 *
 * Limits: 1 <= rows, 1 <= n <= 2^31 - 1 - 1024 (indices are int32), rows * ceil(n / 1024) < 2^31, strides >= n.
 */
#ifndef MODMFCC_SPLINE_H
#define MODMFCC_SPLINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MM_SPLINE_QUADRATIC = 2, MM_SPLINE_CUBIC = 3 };

/* Bytes of workspace for `rows` rows of up to n samples; 0 for invalid arguments. */
size_t mm_interp_spline_workspace_bytes(int32_t kind, int64_t rows, int64_t n);

/* d_x [rows][x_stride] -> d_y [rows][y_stride], float64; d_ws: 256-byte aligned, ws_bytes >= the size above
 * (MM_ERR_WORKSPACE otherwise). */
int mm_interp_spline_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride,
                         double* d_y, int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream);

/* the same with a sample count per row: d_counts int64 [rows] on the device */
int mm_interp_spline_ragged_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                                const int64_t* d_counts, double* d_y, int64_t y_stride,
                                void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
