// libmodmfcc: FIR filtfilt and Savitzky-Golay filters of ANY length on float64 rows -- the 'fir' and 'sg' branches of
// applyFilter (script/mfcc.py:113-133) and get_velocity(method='sg') (script/calc.py:640) beyond what the banded operator
// mm_stencil_f64 holds (8 taps, windows of 16).  gfx950 only.  The kernels:
//   longcorr_kernel<T, EXT>   y[r][i] = sum_k h[k] xe[i + off0 + k] for i in [i_lo, i_hi), direct form.  A workgroup owns a
//                       tile of kLfTile consecutive outputs of one row and takes the taps in chunks of kLfChunk: per chunk
//                       it stages the kLfTile + kLfChunk samples the chunk reaches in LDS (neither the tap count nor the
//                       row has to fit), each lane keeps kLfPer consecutive outputs and a sliding window of kLfPer samples
//                       in registers, so one 8-byte LDS read feeds kLfPer multiply-adds; the tap is wave-uniform.  Every
//                       chunk is summed on its own and the chunk sums are added.  EXT: xe is scipy's odd extension, formed
//                       while staging in the input's own type T (2 x[0] - x[m], 2 x[n-1] - x[n-1-m]); otherwise xe = x.
//   sg_edge_kernel      the first and last W / 2 outputs of savgol_filter(mode='interp'): the polynomial fitted to the
//                       first / last window, as a = Q x[window] (p + 1 dot products over an orthonormal basis, a wave
//                       each) and y = P a (a thread per output).
#include "mm_common.h"

namespace {

constexpr int kLfThreads = 256;
constexpr int kLfPer = 8;                               // consecutive outputs per lane = samples in its register window
constexpr int kLfTile = kLfThreads * kLfPer;            // outputs per workgroup (filters.LONGFILT_TILE)
constexpr int kLfChunk = 128;                           // taps per chunk (filters.LONGFILT_CHUNK); a multiple of kLfPer
constexpr int kLfStage = kLfTile + kLfChunk;            // staged samples per chunk (the last window refill included)
// Lane l reads sample 8 l + o: 64 bytes apart, ds_read_b64 would put the 32 lanes of a group on 4 of the 32 bank pairs.
// One pad slot after every 8 samples makes the lane stride 9 slots (odd): the 32 lanes of a group hit 32 bank pairs.
constexpr int kLfSlots = kLfStage + kLfStage / kLfPer;  // 19 584 bytes: eight workgroups per CU
constexpr int kSgQ = 64;                                // basis polynomials per round of sg_edge_kernel

static_assert(kLfPer == 8 && kLfChunk % kLfPer == 0 && kLfStage % kLfPer == 0, "window rotation is written for 8");

__device__ __forceinline__ int lf_slot(int p) { return p + (p >> 3); }

// sample g of the (extended) row; 0 where neither the row nor the extension reaches (only outputs beyond i_hi read those)
template <typename T, bool EXT>
__device__ __forceinline__ double lf_sample(const T* __restrict__ xr, int64_t n, int64_t g) {
#pragma clang fp contract(off)
  if (g >= 0 && g < n) return (double)xr[g];
  if constexpr (EXT) {
    if (g < 0) {
      if (-g >= n) return 0.0;
      const T e = (T)2 * xr[0] - xr[-g];                // in T: scipy's odd_ext runs before lfilter upcasts
      return (double)e;
    }
    const int64_t m = g - (n - 1);
    if (m >= n) return 0.0;
    const T e = (T)2 * xr[n - 1] - xr[n - 1 - m];
    return (double)e;
  }
  return 0.0;
}

// RAGGED: a length per row (lens, DEVICE int64 [rows], clamped into [1, n]); n and i_hi are then those of the longest row,
// which shape the grid, and a row's own outputs end n - i_hi before ITS end, as the longest row's do.  Outputs of the
// tile at or behind the row's length become +0.0 (a tile without any output of the row's stages nothing), those of a row
// shorter than n_min -- one scipy refuses -- NaN before its length; the outputs between the row's last one and its length
// (the Savitzky-Golay edge) are sg_edge_kernel's.  Nothing at or behind the row's length is loaded: the staging reads
// through lf_sample with the row's own length.  The tiles start at the row's start and the chunks do not depend on the
// length: an output is summed in the order the row alone gives it.
template <typename T, bool EXT, bool RAGGED>
__global__ __launch_bounds__(kLfThreads) void longcorr_kernel(const T* __restrict__ x, int64_t n, int64_t x_stride,
                                                              const double* __restrict__ h, int32_t n_taps, int64_t off0,
                                                              int64_t i_lo, int64_t i_hi, int32_t tiles,
                                                              double* __restrict__ y, int64_t y_stride,
                                                              const int64_t* __restrict__ lens, int64_t n_min) {
  __shared__ double s[kLfSlots];
  const int64_t row = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const T* xr = x + row * x_stride;
  const int64_t i0 = i_lo + tile * kLfTile;             // first output of the tile
  const int lane = threadIdx.x;
  const int64_t i_end = i_hi;                           // RAGGED: where the zeros behind a shorter row end
  if constexpr (RAGGED) {
    const int64_t nb = lens[row], back = n - i_hi;
    n = nb < 1 ? 1 : (nb > n ? n : nb);                 // the row's own length from here on (uniform over the workgroup)
    i_hi = n - back;
    const bool bad = n < n_min;
    if (bad || i0 >= i_hi) {                            // no output of the row's in this tile: before any barrier
      double* yr = y + row * y_stride;
      const int64_t i = i0 + (int64_t)kLfPer * lane;
#pragma unroll
      for (int j = 0; j < kLfPer; ++j) {
        if (i + j < i_end) {
          if (i + j >= n) yr[i + j] = 0.0;
          else if (bad) yr[i + j] = __builtin_nan("");
        }
      }
      return;
    }
  }
  const double* sp = s + (kLfPer + 1) * lane;           // slot of sample kLfPer * lane
  double total[kLfPer];
#pragma unroll
  for (int j = 0; j < kLfPer; ++j) total[j] = 0.0;

#pragma unroll 1
  for (int32_t c0 = 0; c0 < n_taps; c0 += kLfChunk) {
    const int nc = min(kLfChunk, n_taps - c0);
    const int64_t g0 = i0 + off0 + c0;                  // staged sample p is xe[g0 + p]
    for (int p = lane; p < kLfStage; p += kLfThreads) s[lf_slot(p)] = lf_sample<T, EXT>(xr, n, g0 + p);
    __syncthreads();
    const double* hc = h + c0;
    double acc[kLfPer], w[kLfPer];
#pragma unroll
    for (int j = 0; j < kLfPer; ++j) { acc[j] = 0.0; w[j] = sp[j]; }
    // tap k0 + kk multiplies samples 8 l + k0 + kk + j: the window rotates in place, w[kk] is refilled with sample
    // 8 l + k0 + kk + 8 (slot: one group of 9 further) once tap k0 + kk has used it
    int k0 = 0;
#pragma unroll 1
    for (; k0 + kLfPer <= nc; k0 += kLfPer) {
      const double* sn = sp + (kLfPer + 1) * (k0 / kLfPer + 1);
#pragma unroll
      for (int kk = 0; kk < kLfPer; ++kk) {
        const double hk = hc[k0 + kk];                  // wave-uniform
#pragma unroll
        for (int j = 0; j < kLfPer; ++j) acc[j] = __builtin_fma(hk, w[(kk + j) & (kLfPer - 1)], acc[j]);
        w[kk] = sn[kk];
      }
    }
    if (k0 < nc) {                                      // the last 1 .. 7 taps of the filter (uniform)
      const double* sn = sp + (kLfPer + 1) * (k0 / kLfPer + 1);
#pragma unroll
      for (int kk = 0; kk < kLfPer - 1; ++kk) {
        if (k0 + kk < nc) {
          const double hk = hc[k0 + kk];
#pragma unroll
          for (int j = 0; j < kLfPer; ++j) acc[j] = __builtin_fma(hk, w[(kk + j) & (kLfPer - 1)], acc[j]);
          w[kk] = sn[kk];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kLfPer; ++j) total[j] += acc[j];
    __syncthreads();
  }

  double* yr = y + row * y_stride;
  const int64_t i = i0 + (int64_t)kLfPer * lane;
#pragma unroll
  for (int j = 0; j < kLfPer; ++j) {
    if (i + j < i_hi) yr[i + j] = total[j];
    else if constexpr (RAGGED) {
      if (i + j >= n && i + j < i_end) yr[i + j] = 0.0;
    }
  }
}

// block = (row, side): side 0 the first W / 2 outputs from x[0 .. W), side 1 the last W / 2 from x[n - W .. n)
// RAGGED: side 1 fits x[n_b - W .. n_b) of the row's own length n_b and writes the W / 2 outputs before it, then the zeros
// that longcorr_kernel's range [W / 2, n - W / 2) leaves: [max(n_b, n - W / 2), n).  A row with n_b < W (scipy refuses it)
// gets NaN before n_b and zeros behind it in the same two stretches, [0, W / 2) and [n - W / 2, n), and loads nothing.
template <bool RAGGED>
__global__ __launch_bounds__(kLfThreads) void sg_edge_kernel(const double* __restrict__ x, int64_t n, int64_t x_stride,
                                                             const double* __restrict__ q_tab, const double* __restrict__ p_tab,
                                                             int32_t W, int32_t p1, double* __restrict__ y, int64_t y_stride,
                                                             const int64_t* __restrict__ lens) {
  __shared__ double s_a[kSgQ];
  const int64_t row = blockIdx.x >> 1;
  const int side = blockIdx.x & 1;
  const int half = W / 2;
  if constexpr (RAGGED) {
    const int64_t nb = lens[row], n_max = n;
    n = nb < 1 ? 1 : (nb > n_max ? n_max : nb);         // the row's own length from here on (uniform over the workgroup)
    double* yr = y + row * y_stride;
    if (n < W) {                                        // before any barrier
      const int64_t lo = side ? (n_max - half > half ? n_max - half : half) : 0, hi = side ? n_max : half;
      for (int64_t i = lo + threadIdx.x; i < hi; i += kLfThreads) yr[i] = i < n ? __builtin_nan("") : 0.0;
      return;
    }
    if (side)
      for (int64_t i = (n > n_max - half ? n : n_max - half) + threadIdx.x; i < n_max; i += kLfThreads) yr[i] = 0.0;
  }
  const double* xw = x + row * x_stride + (side ? n - W : 0);
  double* yo = y + row * y_stride + (side ? n - half : 0);
  const double* ps = p_tab + (int64_t)side * half * p1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll 1
  for (int q0 = 0; q0 < p1; q0 += kSgQ) {               // (more than kSgQ basis polynomials: rounds; y carries the sum)
    const int nq = min(kSgQ, p1 - q0);
    for (int q = wave; q < nq; q += kLfThreads / 64) {
      const double* qr = q_tab + (int64_t)(q0 + q) * W;
      double a = 0.0;
      for (int w = lane; w < W; w += 64) a = __builtin_fma(qr[w], xw[w], a);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (lane == 0) s_a[q] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < half; i += kLfThreads) {
      const double* pr = ps + (int64_t)i * p1 + q0;
      double v = q0 ? yo[i] : 0.0;
      for (int q = 0; q < nq; ++q) v = __builtin_fma(pr[q], s_a[q], v);
      yo[i] = v;
    }
    __syncthreads();
  }
}

// grid of longcorr_kernel for `outputs` outputs per row; 0 when it does not fit a 31-bit block index
int64_t lf_tiles(int64_t rows, int64_t outputs) {
  const int64_t tiles = (outputs + kLfTile - 1) / kLfTile;
  return tiles > 0x7fffffff || rows * tiles > 0x7fffffff ? 0 : tiles;
}

// d_lens (DEVICE int64 [rows], or null): the ragged form, n the longest row's length
template <typename T>
int lf_fir_filtfilt(const T* d_x, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_lens, const double* d_h,
                    int32_t n_taps, double* d_y, int64_t y_stride, void* stream) {
  if (!d_x || !d_h || !d_y || rows < 1 || rows > 0x7fffffff || n_taps < 2 || n_taps > (1 << 29) || n <= 3 * (int64_t)n_taps ||
      x_stride < n || y_stride < n)
    return MM_ERR_INVALID_ARG;
  const int64_t tiles = lf_tiles(rows, n);
  if (!tiles) return MM_ERR_INVALID_ARG;
  if (d_lens)
    hipLaunchKernelGGL((longcorr_kernel<T, true, true>), dim3((unsigned)(rows * tiles)), dim3(kLfThreads), 0, (hipStream_t)stream,
                       d_x, n, x_stride, d_h, 2 * n_taps - 1, -(int64_t)(n_taps - 1), (int64_t)0, n, (int32_t)tiles, d_y, y_stride,
                       d_lens, 3 * (int64_t)n_taps + 1);
  else
    hipLaunchKernelGGL((longcorr_kernel<T, true, false>), dim3((unsigned)(rows * tiles)), dim3(kLfThreads), 0, (hipStream_t)stream,
                       d_x, n, x_stride, d_h, 2 * n_taps - 1, -(int64_t)(n_taps - 1), (int64_t)0, n, (int32_t)tiles, d_y, y_stride,
                       d_lens, (int64_t)0);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

int lf_savgol(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_lens, const double* d_c,
              const double* d_q, const double* d_p, int32_t window, int32_t n_basis, double* d_y, int64_t y_stride, void* stream) {
  if (!d_x || !d_c || !d_y || rows < 1 || rows > 0x3fffffff || window < 1 || window > n || n_basis < 1 || n_basis > window ||
      x_stride < n || y_stride < n)
    return MM_ERR_INVALID_ARG;
  const int32_t half = window / 2;
  if (half > 0 && (!d_q || !d_p)) return MM_ERR_INVALID_ARG;
  const int64_t i_lo = half, i_hi = n - half;           // window == n, even: no interior output at all
  hipStream_t st = (hipStream_t)stream;
  if (i_hi > i_lo) {
    const int64_t tiles = lf_tiles(rows, i_hi - i_lo);
    if (!tiles) return MM_ERR_INVALID_ARG;
    if (d_lens)
      hipLaunchKernelGGL((longcorr_kernel<double, false, true>), dim3((unsigned)(rows * tiles)), dim3(kLfThreads), 0, st, d_x, n,
                         x_stride, d_c, window, -(int64_t)((window - 1) / 2), i_lo, i_hi, (int32_t)tiles, d_y, y_stride, d_lens,
                         (int64_t)window);
    else
      hipLaunchKernelGGL((longcorr_kernel<double, false, false>), dim3((unsigned)(rows * tiles)), dim3(kLfThreads), 0, st, d_x, n,
                         x_stride, d_c, window, -(int64_t)((window - 1) / 2), i_lo, i_hi, (int32_t)tiles, d_y, y_stride, d_lens,
                         (int64_t)0);
    HIP_TRY(hipGetLastError());
  }
  if (half > 0) {
    if (d_lens)
      hipLaunchKernelGGL(sg_edge_kernel<true>, dim3((unsigned)(2 * rows)), dim3(kLfThreads), 0, st, d_x, n, x_stride, d_q, d_p,
                         window, n_basis, d_y, y_stride, d_lens);
    else
      hipLaunchKernelGGL(sg_edge_kernel<false>, dim3((unsigned)(2 * rows)), dim3(kLfThreads), 0, st, d_x, n, x_stride, d_q, d_p,
                         window, n_basis, d_y, y_stride, d_lens);
    HIP_TRY(hipGetLastError());
  }
  return MM_OK;
}

}  // namespace

extern "C" {

int mm_fir_filtfilt_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_h, int32_t n_taps,
                        double* d_y, int64_t y_stride, void* stream) {
  return lf_fir_filtfilt(d_x, rows, n, x_stride, nullptr, d_h, n_taps, d_y, y_stride, stream);
}

int mm_fir_filtfilt_f32_f64(const float* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_h, int32_t n_taps,
                            double* d_y, int64_t y_stride, void* stream) {
  return lf_fir_filtfilt(d_x, rows, n, x_stride, nullptr, d_h, n_taps, d_y, y_stride, stream);
}

int mm_fir_filtfilt_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                               const double* d_h, int32_t n_taps, double* d_y, int64_t y_stride, void* stream) {
  if (!d_lens) return MM_ERR_INVALID_ARG;
  return lf_fir_filtfilt(d_x, rows, n_max, x_stride, d_lens, d_h, n_taps, d_y, y_stride, stream);
}

int mm_fir_filtfilt_ragged_f32_f64(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                                   const double* d_h, int32_t n_taps, double* d_y, int64_t y_stride, void* stream) {
  if (!d_lens) return MM_ERR_INVALID_ARG;
  return lf_fir_filtfilt(d_x, rows, n_max, x_stride, d_lens, d_h, n_taps, d_y, y_stride, stream);
}

int mm_savgol_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* d_c, const double* d_q,
                  const double* d_p, int32_t window, int32_t n_basis, double* d_y, int64_t y_stride, void* stream) {
  return lf_savgol(d_x, rows, n, x_stride, nullptr, d_c, d_q, d_p, window, n_basis, d_y, y_stride, stream);
}

int mm_savgol_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                         const double* d_c, const double* d_q, const double* d_p, int32_t window, int32_t n_basis, double* d_y,
                         int64_t y_stride, void* stream) {
  if (!d_lens) return MM_ERR_INVALID_ARG;
  return lf_savgol(d_x, rows, n_max, x_stride, d_lens, d_c, d_q, d_p, window, n_basis, d_y, y_stride, stream);
}

}  // extern "C"
