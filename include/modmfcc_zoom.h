/*
 * modmfcc_zoom.h -- sixth header of libmodmfcc.so: the B-spline zoom of 2-D feature images on the device.
 *
 *   mm_zoom2d_f32 / _f64  <- script/praat_py_ui/spectrogram.py:70-71, scipy.ndimage.zoom(spect_data, 6, order=4) on
 *                            10 * numpy.log10(spectrogram.values); any order 0 .. 5, any zoom per axis, on a batch of images
 *
 * The contract is that of include/modmfcc_spline.h and include/modmfcc_lomb.h: device pointers owned by the caller,
 * asynchronous on the caller's stream, no allocation and no synchronisation (graph-capture safe), MM_OK or a negative
 * mm_status; every refusal comes before the first launch.
 *
 * Semantics (scipy 1.15): scipy.ndimage.zoom(x, zoom, order, mode, cval, prefilter, grid_mode=False) on the last two axes.
 *   sizes      the caller gives h_out and w_out (scipy: round(n * zoom), ties to even); the step of an axis is
 *              z = (n - 1) / (n_out - 1) in float64, 1 when n_out == 1.
 *   prefilter  orders 2 .. 5, both modes: the exact spline filter of the whole-sample-symmetric ("mirror") extension --
 *              scipy.ndimage.spline_filter(mode='mirror'), which is what scipy applies in mode 'constant' too -- down the
 *              columns, then along the rows.  It is applied as the filter's own two-sided impulse response, cut where a
 *              tap falls below 2^-68 of the centre tap (at most 80 samples each way), on the mirrored samples: no serial
 *              pass over an axis.  An axis of length 1 is left as it is.
 *   evaluation output index j has the coordinate cc = j * z (one float64 multiply).  MM_ZOOM_CONSTANT: cc < 0 or cc > n - 1
 *              gives cval for that whole output row or column -- also where (n_out - 1) * z rounds one ulp past n - 1
 *              (n = 59 at zoom 6), as in scipy.  Otherwise the taps are start .. start + order with
 *              start = floor(cc + 0.5) - order / 2 (even orders), floor(cc) - order / 2 (odd orders); a tap outside
 *              [0, n - 1] is mirrored with the period 2 n - 2 in both modes; the weights are the centred cardinal
 *              B-spline of the order at cc - tap.  Order 0 is the sample at floor(cc + 0.5).
 *   types      all arithmetic is float64 without contraction; a float32 result is the float64 result rounded once.
 *   MM_ZOOM_DB the samples are 10 * log10(x) in float64 as they are loaded (the reference's dB step).
 * The result is within a few of scipy's own roundings of scipy's, not equal bit for bit; the cval positions are equal
 * bit for bit.
 *
 * Finite inputs only.  In scipy ONE Inf or NaN sample makes the whole image non-finite through the filter's recursions;
 * here it reaches the filter's support (at most 88 samples each way) and no further: every output whose taps touch the
 * sample is non-finite, the rest of the image is what it would be for a finite sample there, or non-finite.
 *
 * An image's result depends on its own samples and sizes only: not on the batch, on the strides, or (ragged form) on what
 * lies behind its width.
 *
 * Ragged form: image b has w_b = clamp(d_widths[b], 1, w) columns, w_out_b = clamp(rint(w_b * zoom_x), 1, w_out) output
 * columns and its own horizontal step; the output columns behind w_out_b are written as +0.0, the input behind w_b is
 * never read.  h and h_out are common.
 *
 * Limits: 1 <= images; 1 <= h, w, h_out, w_out <= 2^30; h * w < 2^31 and h_out * w_out < 2^31 (indices are int32 within
 * an image); images * ceil(h / 2) * ceil(w / 128) < 2^31 and images * ceil(h_out / 32) * ceil(w_out / 256) < 2^31; row
 * strides >= the width, image strides >= (rows - 1) * row stride + width; MM_ZOOM_FILTER_ONLY needs h_out == h and
 * w_out == w.  Orders outside 0 .. 5 and modes other than the two: MM_ERR_UNSUPPORTED.
 */
#ifndef MODMFCC_ZOOM_H
#define MODMFCC_ZOOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ZOOM_VERSION 100
#define MM_ZOOM_SEGMENT 128        /* columns a workgroup of the horizontal prefilter owns, per row */
#define MM_ZOOM_MAX_TAPS 80        /* the longest one-sided impulse response of a prefilter (order 5: 56) */

enum { MM_ZOOM_CONSTANT = 0, MM_ZOOM_MIRROR = 1 };                                   /* mode */
enum { MM_ZOOM_PREFILTER = 1, MM_ZOOM_DB = 2, MM_ZOOM_FILTER_ONLY = 4 };            /* flags */

int mm_zoom_version(void);

/* Bytes of workspace for `images` images of h x w samples zoomed to h_out x w_out; 0 for invalid arguments. */
size_t mm_zoom2d_workspace_bytes(int32_t order, int64_t images, int64_t h, int64_t w, int64_t h_out, int64_t w_out);

/* d_x [images][h][w] (strides in elements) -> d_y [images][h_out][w_out]; d_ws: 256-byte aligned, ws_bytes >= the size
 * above (MM_ERR_WORKSPACE otherwise).  MM_ZOOM_FILTER_ONLY stops behind the prefilter: d_y holds the spline
 * coefficients, scipy.ndimage.spline_filter(x, order, mode='mirror'). */
int mm_zoom2d_f32(int32_t order, int32_t mode, double cval, int32_t flags, const float* d_x, int64_t images, int64_t h,
                  int64_t w, int64_t x_image_stride, int64_t x_row_stride, int64_t h_out, int64_t w_out, float* d_y,
                  int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream);
int mm_zoom2d_f64(int32_t order, int32_t mode, double cval, int32_t flags, const double* d_x, int64_t images, int64_t h,
                  int64_t w, int64_t x_image_stride, int64_t x_row_stride, int64_t h_out, int64_t w_out, double* d_y,
                  int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream);

/* the same with a width per image: d_widths int64 [images] on the device, zoom_x the horizontal zoom factor */
int mm_zoom2d_ragged_f32(int32_t order, int32_t mode, double cval, int32_t flags, const float* d_x, int64_t images,
                         int64_t h, int64_t w_max, int64_t x_image_stride, int64_t x_row_stride,
                         const int64_t* d_widths, double zoom_x, int64_t h_out, int64_t w_out, float* d_y,
                         int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream);
int mm_zoom2d_ragged_f64(int32_t order, int32_t mode, double cval, int32_t flags, const double* d_x, int64_t images,
                         int64_t h, int64_t w_max, int64_t x_image_stride, int64_t x_row_stride,
                         const int64_t* d_widths, double zoom_x, int64_t h_out, int64_t w_out, double* d_y,
                         int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
