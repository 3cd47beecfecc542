// mm_zoom.hip -- the B-spline zoom of 2-D feature images (include/modmfcc_zoom.h): scipy.ndimage.zoom of scipy 1.15 on the
// last two axes of a batch, orders 0 .. 5, modes 'constant' and 'mirror', in float64.  DESIGN.md section 17.
//
// The prefilter of an order is a cascade of first-order recursions, forwards and backwards, over the whole-sample-symmetric
// extension of a line.  Its poles are small (the largest, of order 5, is -0.4306), so its two-sided impulse response
// g[|k|] falls below 2^-68 of g[0] within 56 samples: the filter is applied as that response on the mirrored samples,
//     c[i] = sum over k = -R .. R of g[|k|] s[mirror(i + k)],
// ascending in k, one fused multiply-add a tap.  No sample waits for another, a line needs no serial pass, and an output
// depends on its own line alone.  The response is computed on the host in long double (the recursions run on an impulse)
// and travels in the kernel arguments; a workgroup copies it into LDS, where its index is wave-uniform (a broadcast read).
//
// Kernels (no atomics), at most three launches a call:
//   zm_filter_v_kernel  a thread per column and kZmVB consecutive rows: the loads are coalesced along the row, a loaded
//                       sample feeds kZmVB sums.  It also is the load stage: float32 or float64 in, 10 log10 on load,
//                       float64 out -- with R = 0 (orders 0 and 1, prefilter off, h = 1) a conversion.
//   zm_filter_h_kernel  a workgroup per 8 rows x MM_ZOOM_SEGMENT columns: the segments and R mirrored samples either side
//                       in LDS (lane-consecutive 8-byte reads: no bank conflict), a thread per column and 4 rows, so
//                       that a tap read feeds four sums.
//   zm_eval_kernel      a workgroup per 32 x 256 output tile, a thread per output column.  The column's start index,
//                       mirrored taps and weights live in its registers for the whole tile, the rows' in LDS.  The
//                       horizontal pass of the coefficient rows the tile needs goes into LDS (16 rows at a time: any
//                       shrink factor fits, a row of outputs needs at most order + 1), the vertical pass into a
//                       register, and every store is a full row of the tile: 1 KiB (float32) or 2 KiB contiguous.
// Everything that forms a coordinate, a comparison or a weight is compiled without contraction.
#include "mm_common.h"
#include "../../include/modmfcc_zoom.h"

namespace {

constexpr int kZmThreads = 256;
constexpr int kZmSeg = MM_ZOOM_SEGMENT;          // columns of a horizontal prefilter segment
constexpr int kZmTapMax = MM_ZOOM_MAX_TAPS;      // R <= kZmTapMax
constexpr int kZmVB = 8;                         // rows a thread of the vertical prefilter owns
constexpr int kZmHR = 4;                         // rows a thread of the horizontal prefilter owns
constexpr int kZmTileW = 256, kZmTileH = 32;     // the evaluation's output tile
constexpr int kZmPatchRows = 16;                 // coefficient rows (after the horizontal pass) resident in LDS
static_assert(kZmThreads == 2 * kZmSeg && kZmThreads == kZmTileW && kZmTileH <= kZmThreads, "thread maps");

struct ZmTaps {
  int r, reserved;
  double g[kZmTapMax + kZmVB];                   // g[|k|], +0.0 behind r
};

__device__ __forceinline__ int zm_mirror(int i, int n) {      // whole-sample-symmetric, period 2 n - 2 (n <= 2^30)
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

__device__ __forceinline__ int zm_width(const int64_t* __restrict__ widths, int64_t b, int w) {
  if (!widths) return w;
  const int64_t v = widths[b];
  return v < 1 ? 1 : (v > w ? w : (int)v);
}

template <typename T>
__device__ __forceinline__ double zm_load(const T* __restrict__ p, int db) {
#pragma clang fp contract(off)
  const double v = (double)*p;
  return db ? 10.0 * log10(v) : v;
}

template <typename T>
__global__ __launch_bounds__(kZmThreads) void zm_filter_v_kernel(const T* __restrict__ x, int64_t x_img, int64_t x_row, int h,
                                                                 int w, const int64_t* __restrict__ widths, ZmTaps taps, int db,
                                                                 double* __restrict__ out, int tiles_x, int tiles_y) {
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  const int64_t b = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - b * tiles);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  __shared__ double sg[kZmTapMax + kZmVB + 1];
  for (int i = threadIdx.x; i <= kZmTapMax + kZmVB; i += kZmThreads) sg[i] = i < kZmTapMax + kZmVB ? taps.g[i] : 0.0;
  __syncthreads();
  const int col = tx * kZmThreads + threadIdx.x;
  if (col >= zm_width(widths, b, w)) return;                     // (no barrier behind this point)
  const int y0 = ty * kZmVB;
  const T* __restrict__ xi = x + b * x_img + col;
  double* __restrict__ o = out + b * h * (int64_t)w + col;
  const int R = h == 1 ? 0 : taps.r;
  if (R == 0) {                                                  // a conversion: the sample's bits, -0.0 included
#pragma unroll
    for (int k = 0; k < kZmVB; ++k)
      if (y0 + k < h) o[(int64_t)(y0 + k) * w] = zm_load(xi + (int64_t)(y0 + k) * x_row, db);
    return;
  }
  // row y0 + k takes sample y0 - R + s with the tap g[|s - R - k|]: the taps of the kZmVB rows are a window that moves
  // by one a step (|s - R - k| <= R + kZmVB: a zero tap behind R changes no sum)
  double acc[kZmVB], tp[kZmVB];
#pragma unroll
  for (int k = 0; k < kZmVB; ++k) {
    acc[k] = 0.0;
    tp[k] = sg[R + k];
  }
  for (int s = 0; s < kZmVB + 2 * R; ++s) {
    const int yy = zm_mirror(y0 - R + s, h);                     // (wave-uniform)
    const double v = zm_load(xi + (int64_t)yy * x_row, db);
#pragma unroll
    for (int k = 0; k < kZmVB; ++k) acc[k] = __builtin_fma(tp[k], v, acc[k]);
#pragma unroll
    for (int k = kZmVB - 1; k > 0; --k) tp[k] = tp[k - 1];
    const int d = s + 1 - R;
    tp[0] = sg[d < 0 ? -d : d];
  }
#pragma unroll
  for (int k = 0; k < kZmVB; ++k)
    if (y0 + k < h) o[(int64_t)(y0 + k) * w] = acc[k];
}

// a [images][h][w] float64 -> out (the second plane of the workspace, or the caller's output for MM_ZOOM_FILTER_ONLY:
// then the columns behind a ragged width up to zero_w are written as +0.0)
template <typename TO>
__global__ __launch_bounds__(kZmThreads) void zm_filter_h_kernel(const double* __restrict__ a, int h, int w,
                                                                 const int64_t* __restrict__ widths, ZmTaps taps,
                                                                 TO* __restrict__ out, int64_t o_img, int64_t o_row, int zero_w,
                                                                 int tiles_x, int tiles_y) {
  __shared__ double seg[2 * kZmHR][kZmSeg + 2 * kZmTapMax];
  __shared__ double sg[kZmTapMax + 1];
  if (threadIdx.x <= kZmTapMax) sg[threadIdx.x] = taps.g[threadIdx.x];
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  const int64_t b = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - b * tiles);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int half = threadIdx.x / kZmSeg, lx = threadIdx.x - half * kZmSeg;
  const int row0 = (ty * 2 + half) * kZmHR, x0 = tx * kZmSeg;      // this thread's kZmHR rows (the same in a wave)
  const int wb = zm_width(widths, b, w);
  const int R = wb == 1 ? 0 : taps.r;
  if (x0 < wb) {
#pragma unroll
    for (int q = 0; q < kZmHR; ++q) {
      const int row = row0 + q < h ? row0 + q : h - 1;             // (a row behind the image: the last one again, not stored)
      const double* __restrict__ ar = a + (b * h + row) * (int64_t)w;
      for (int i = lx; i < kZmSeg + 2 * R; i += kZmSeg) seg[half * kZmHR + q][i] = ar[zm_mirror(x0 - R + i, wb)];
    }
  }
  __syncthreads();
  const int xo = x0 + lx;
  TO* __restrict__ o = out + b * o_img + (int64_t)row0 * o_row + xo;
  if (xo < wb) {
    double acc[kZmHR];
#pragma unroll
    for (int q = 0; q < kZmHR; ++q) acc[q] = seg[half * kZmHR + q][lx + R];
    if (R > 0) {
#pragma unroll
      for (int q = 0; q < kZmHR; ++q) acc[q] = 0.0;
      for (int k = 0; k <= 2 * R; ++k) {                           // a tap read feeds kZmHR rows
        const double g = sg[k < R ? R - k : k - R];
#pragma unroll
        for (int q = 0; q < kZmHR; ++q) acc[q] = __builtin_fma(g, seg[half * kZmHR + q][lx + k], acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kZmHR; ++q)
      if (row0 + q < h) o[(int64_t)q * o_row] = (TO)acc[q];
  } else if (xo < zero_w) {
#pragma unroll
    for (int q = 0; q < kZmHR; ++q)
      if (row0 + q < h) o[(int64_t)q * o_row] = (TO)0.0;
  }
}

// the centred cardinal B-spline of degree ORDER at the distance x >= 0
template <int ORDER>
__device__ __forceinline__ double zm_bspline(double x) {
#pragma clang fp contract(off)
  if (ORDER == 1) return x < 1.0 ? 1.0 - x : 0.0;
  if (ORDER == 2) {
    if (x < 0.5) return 0.75 - x * x;
    if (x < 1.5) {
      const double t = 1.5 - x;
      return t * t / 2.0;
    }
    return 0.0;
  }
  if (ORDER == 3) {
    if (x < 1.0) return (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0;
    if (x < 2.0) {
      const double t = 2.0 - x;
      return t * t * t / 6.0;
    }
    return 0.0;
  }
  if (ORDER == 4) {
    if (x < 0.5) {
      const double t = x * x;
      return t * (t / 4.0 - 0.625) + 115.0 / 192.0;
    }
    if (x < 1.5) return x * (x * (x * (5.0 / 6.0 - x / 6.0) - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
    if (x < 2.5) {
      double t = x - 2.5;
      t = t * t;
      return t * t / 24.0;
    }
    return 0.0;
  }
  if (ORDER == 5) {
    if (x < 1.0) {
      const double q = x * x;
      return q * (q * (0.25 - x / 12.0) - 0.5) + 11.0 / 20.0;
    }
    if (x < 2.0) return x * (x * (x * (x * (x / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 17.0 / 40.0;
    if (x < 3.0) {
      const double t = 3.0 - x, q = t * t;
      return t * q * q / 120.0;
    }
    return 0.0;
  }
  return 1.0;
}

// output index j of an axis of n samples with the step z: the first tap, whether scipy returns cval, the weights
template <int ORDER>
__device__ __forceinline__ void zm_axis(int j, double z, int n, int mode, int& start, bool& outside, double (&wt)[ORDER + 1]) {
#pragma clang fp contract(off)
  const double cc = (double)j * z;                               // one float64 multiply, contracted into nothing
  outside = mode == MM_ZOOM_CONSTANT && (cc < 0.0 || cc > (double)(n - 1));
  if (ORDER == 0) {
    start = (int)floor(cc + 0.5);
    wt[0] = 1.0;
    return;
  }
  start = (int)floor((ORDER & 1) ? cc : cc + 0.5) - ORDER / 2;
#pragma unroll
  for (int a = 0; a <= ORDER; ++a) wt[a] = zm_bspline<ORDER>(fabs(cc - (double)(start + a)));
}

template <typename T, int ORDER>
__global__ __launch_bounds__(kZmThreads) void zm_eval_kernel(const double* __restrict__ c, int h, int w,
                                                             const int64_t* __restrict__ widths, double zoom_x, double zy,
                                                             double zx, int mode, double cval, T* __restrict__ out, int64_t o_img,
                                                             int64_t o_row, int h_out, int w_out, int tiles_x, int tiles_y) {
#pragma clang fp contract(off)
  constexpr int K1 = ORDER + 1;
  __shared__ double hrow[kZmPatchRows][kZmTileW];
  __shared__ double swy[kZmTileH][K1];
  __shared__ int ssy[kZmTileH], sfy[kZmTileH];
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  const int64_t b = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - b * tiles);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int tid = threadIdx.x;

  int wb = w, wob = w_out;
  double zxb = zx;
  if (widths) {                                                  // the image's own width, output width and step
    wb = zm_width(widths, b, w);
    const double r = rint((double)wb * zoom_x);
    wob = r < 1.0 ? 1 : (r > (double)w_out ? w_out : (int)r);
    zxb = wob > 1 ? (double)(wb - 1) / (double)(wob - 1) : 1.0;
  }
  const int j = tx * kZmTileW + tid;
  const bool live = j < wob;
  double wxv[K1];
  int ix[K1];
  bool ox = false;
#pragma unroll
  for (int a = 0; a < K1; ++a) {
    wxv[a] = 0.0;
    ix[a] = 0;
  }
  if (live) {
    int start;
    zm_axis<ORDER>(j, zxb, wb, mode, start, ox, wxv);
#pragma unroll
    for (int a = 0; a < K1; ++a) ix[a] = zm_mirror(start + a, wb);
  }
  const int jy0 = ty * kZmTileH;
  const int th = h_out - jy0 < kZmTileH ? h_out - jy0 : kZmTileH;
  if (tid < th) {
    int start;
    bool oy;
    double wv[K1];
    zm_axis<ORDER>(jy0 + tid, zy, h, mode, start, oy, wv);
    ssy[tid] = start;
    sfy[tid] = oy ? 1 : 0;
#pragma unroll
    for (int a = 0; a < K1; ++a) swy[tid][a] = wv[a];
  }
  __syncthreads();

  const double* __restrict__ cb = c + b * h * (int64_t)w;
  T* __restrict__ ob = out + b * o_img + j;
  const T cv = (T)cval;
  for (int yb = 0; yb < th;) {
    // the rows yb .. ye - 1 whose taps fit into the resident coefficient rows (the starts ascend with the row; one row
    // always fits); everything here is the same in every thread
    const int r0 = ssy[yb];
    int ye = yb + 1;
    while (ye < th && ssy[ye] + K1 - r0 <= kZmPatchRows) ++ye;
    const int span = ssy[ye - 1] + K1 - r0;
    if (live && !ox) {
      for (int r = 0; r < span; ++r) {
        const double* __restrict__ p = cb + (int64_t)zm_mirror(r0 + r, h) * w;
        double acc = wxv[0] * p[ix[0]];
#pragma unroll
        for (int a = 1; a < K1; ++a) acc = __builtin_fma(wxv[a], p[ix[a]], acc);
        hrow[r][tid] = acc;
      }
    }
    __syncthreads();
    if (j < w_out) {
      int held = -1;                                             // the resident rows in hv: rows of one start share them
      double hv[K1];
#pragma unroll
      for (int a = 0; a < K1; ++a) hv[a] = 0.0;
      for (int y = yb; y < ye; ++y) {
        T v = (T)0.0;                                            // (behind a ragged image's output width)
        if (live) {
          v = cv;
          if (!ox && !sfy[y]) {
            const int base = ssy[y] - r0;
            if (base != held) {                                  // (the same in every thread)
#pragma unroll
              for (int a = 0; a < K1; ++a) hv[a] = hrow[base + a][tid];
              held = base;
            }
            double acc = swy[y][0] * hv[0];
#pragma unroll
            for (int a = 1; a < K1; ++a) acc = __builtin_fma(swy[y][a], hv[a], acc);
            v = (T)acc;
          }
        }
        ob[(int64_t)(jy0 + y) * o_row] = v;
      }
    }
    __syncthreads();                                             // before the resident rows are replaced
    yb = ye;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// The prefilter's impulse response: scipy's recursions (ni_splines.c: gain, then per pole the causal and the anticausal
// pass) on an impulse far from both ends, in long double.
void zm_taps(int order, ZmTaps& t) {
  t.r = 0;
  t.reserved = 0;
  for (double& v : t.g) v = 0.0;
  t.g[0] = 1.0;
  long double pole[2];
  int np = 0;
  if (order == 2) pole[np++] = sqrtl(8.0L) - 3.0L;
  if (order == 3) pole[np++] = sqrtl(3.0L) - 2.0L;
  if (order == 4) {
    pole[np++] = sqrtl(664.0L - sqrtl(438976.0L)) + sqrtl(304.0L) - 19.0L;
    pole[np++] = sqrtl(664.0L + sqrtl(438976.0L)) - sqrtl(304.0L) - 19.0L;
  }
  if (order == 5) {
    pole[np++] = sqrtl(67.5L - sqrtl(4436.25L)) + sqrtl(26.25L) - 6.5L;
    pole[np++] = sqrtl(67.5L + sqrtl(4436.25L)) - sqrtl(26.25L) - 6.5L;
  }
  if (np == 0) return;
  constexpr int L = 4 * kZmTapMax, N = 2 * L + 1;
  std::vector<long double> c(N, 0.0L);
  long double gain = 1.0L;
  for (int p = 0; p < np; ++p) gain *= (1.0L - pole[p]) * (1.0L - 1.0L / pole[p]);
  c[L] = gain;
  for (int p = 0; p < np; ++p) {
    const long double z = pole[p];
    for (int i = 1; i < N; ++i) c[i] += z * c[i - 1];
    c[N - 1] = (z * c[N - 2] + c[N - 1]) * z / (z * z - 1.0L);
    for (int i = N - 2; i >= 0; --i) c[i] = z * (c[i + 1] - c[i]);
  }
  int r = 0;
  for (int k = 0; k <= kZmTapMax; ++k)
    if (fabsl(c[L + k]) > ldexpl(fabsl(c[L]), -68)) r = k;
  t.r = r;
  for (int k = 0; k <= r; ++k) t.g[k] = (double)c[L + k];
}

bool zm_shape_ok(int64_t images, int64_t h, int64_t w, int64_t h_out, int64_t w_out) {
  const int64_t top = (int64_t)1 << 30, lim = (int64_t)1 << 31;
  if (images < 1 || images >= lim || h < 1 || w < 1 || h_out < 1 || w_out < 1 || h > top || w > top || h_out > top || w_out > top)
    return false;
  if (h * w >= lim || h_out * w_out >= lim) return false;
  const int64_t th = ((h + 1) / 2) * ((w + kZmSeg - 1) / kZmSeg);
  const int64_t te = ((h_out + kZmTileH - 1) / kZmTileH) * ((w_out + kZmTileW - 1) / kZmTileW);
  return images * th < lim && images * te < lim;                 // (factors below 2^31 each: no overflow)
}

size_t zm_plane_bytes(int64_t images, int64_t h, int64_t w) { return align_up((size_t)images * h * w * sizeof(double), 256); }

template <typename T, int ORDER>
void zm_launch_eval(hipStream_t st, unsigned grid, const double* c, int h, int w, const int64_t* widths, double zoom_x, double zy,
                    double zx, int mode, double cval, T* out, int64_t o_img, int64_t o_row, int h_out, int w_out, int tiles_x,
                    int tiles_y) {
  hipLaunchKernelGGL((zm_eval_kernel<T, ORDER>), dim3(grid), dim3(kZmThreads), 0, st, c, h, w, widths, zoom_x, zy, zx, mode, cval,
                     out, o_img, o_row, h_out, w_out, tiles_x, tiles_y);
}

template <typename T>
int zm_run(int32_t order, int32_t mode, double cval, int32_t flags, const T* d_x, int64_t images, int64_t h, int64_t w,
           int64_t x_img, int64_t x_row, const int64_t* d_widths, bool ragged, double zoom_x, int64_t h_out, int64_t w_out,
           T* d_y, int64_t y_img, int64_t y_row, void* d_ws, size_t ws_bytes, void* stream) {
  if (order < 0 || order > 5 || (mode != MM_ZOOM_CONSTANT && mode != MM_ZOOM_MIRROR)) return MM_ERR_UNSUPPORTED;
  const bool only = (flags & MM_ZOOM_FILTER_ONLY) != 0;
  if (!zm_shape_ok(images, h, w, h_out, w_out) || !d_x || !d_y || (flags & ~7) || (ragged && !d_widths) ||
      (ragged && !(zoom_x > 0.0 && zoom_x < 1e300)) || (only && (h_out != h || w_out != w)) ||
      (h > 1 && x_row < w) || (h_out > 1 && y_row < w_out) || x_row < 0 || y_row < 0 ||
      (images > 1 && (x_img < (h - 1) * x_row + w || y_img < (h_out - 1) * y_row + w_out)) || x_img < 0 || y_img < 0)
    return MM_ERR_INVALID_ARG;
  if (!d_ws || ((uintptr_t)d_ws & 255) || ws_bytes < mm_zoom2d_workspace_bytes(order, images, h, w, h_out, w_out))
    return MM_ERR_WORKSPACE;
  const bool filter = (flags & MM_ZOOM_PREFILTER) && order >= 2;
  ZmTaps taps;
  zm_taps(filter ? order : 0, taps);
  double* plane_a = (double*)d_ws;
  double* plane_b = (double*)((char*)d_ws + zm_plane_bytes(images, h, w));
  hipStream_t st = (hipStream_t)stream;
  const int hi = (int)h, wi = (int)w;
  {
    const int tx = (wi + kZmThreads - 1) / kZmThreads, ty = (hi + kZmVB - 1) / kZmVB;
    hipLaunchKernelGGL((zm_filter_v_kernel<T>), dim3((unsigned)(images * tx * ty)), dim3(kZmThreads), 0, st, d_x, x_img, x_row, hi,
                       wi, d_widths, taps, (flags & MM_ZOOM_DB) ? 1 : 0, plane_a, tx, ty);
    HIP_TRY(hipGetLastError());
  }
  const double* coeff = plane_a;
  if (filter || only) {
    const int tx = (wi + kZmSeg - 1) / kZmSeg, ty = (hi + 2 * kZmHR - 1) / (2 * kZmHR);
    const unsigned grid = (unsigned)(images * tx * ty);
    if (only)
      hipLaunchKernelGGL((zm_filter_h_kernel<T>), dim3(grid), dim3(kZmThreads), 0, st, (const double*)plane_a, hi, wi, d_widths,
                         taps, d_y, y_img, y_row, wi, tx, ty);
    else
      hipLaunchKernelGGL((zm_filter_h_kernel<double>), dim3(grid), dim3(kZmThreads), 0, st, (const double*)plane_a, hi, wi,
                         d_widths, taps, plane_b, h * w, w, 0, tx, ty);
    HIP_TRY(hipGetLastError());
    if (only) return MM_OK;
    coeff = plane_b;
  }
  const int ho = (int)h_out, wo = (int)w_out;
  const int tx = (wo + kZmTileW - 1) / kZmTileW, ty = (ho + kZmTileH - 1) / kZmTileH;
  const unsigned grid = (unsigned)(images * tx * ty);
  const double zy = ho > 1 ? (double)(hi - 1) / (double)(ho - 1) : 1.0;
  const double zx = wo > 1 ? (double)(wi - 1) / (double)(wo - 1) : 1.0;
#define ZM_EVAL(O)                                                                                                             \
  case O:                                                                                                                      \
    zm_launch_eval<T, O>(st, grid, coeff, hi, wi, d_widths, zoom_x, zy, zx, mode, cval, d_y, y_img, y_row, ho, wo, tx, ty);       \
    break;
  switch (order) {
    ZM_EVAL(0) ZM_EVAL(1) ZM_EVAL(2) ZM_EVAL(3) ZM_EVAL(4) ZM_EVAL(5)
  }
#undef ZM_EVAL
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // namespace

extern "C" {

int mm_zoom_version(void) { return MM_ZOOM_VERSION; }

size_t mm_zoom2d_workspace_bytes(int32_t order, int64_t images, int64_t h, int64_t w, int64_t h_out, int64_t w_out) {
  if (order < 0 || order > 5 || !zm_shape_ok(images, h, w, h_out, w_out)) return 0;
  return (order >= 2 ? 2 : 1) * zm_plane_bytes(images, h, w);
}

int mm_zoom2d_f32(int32_t order, int32_t mode, double cval, int32_t flags, const float* d_x, int64_t images, int64_t h,
                  int64_t w, int64_t x_image_stride, int64_t x_row_stride, int64_t h_out, int64_t w_out, float* d_y,
                  int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return zm_run<float>(order, mode, cval, flags, d_x, images, h, w, x_image_stride, x_row_stride, nullptr, false, 1.0, h_out,
                       w_out, d_y, y_image_stride, y_row_stride, d_ws, ws_bytes, stream);
}

int mm_zoom2d_f64(int32_t order, int32_t mode, double cval, int32_t flags, const double* d_x, int64_t images, int64_t h,
                  int64_t w, int64_t x_image_stride, int64_t x_row_stride, int64_t h_out, int64_t w_out, double* d_y,
                  int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return zm_run<double>(order, mode, cval, flags, d_x, images, h, w, x_image_stride, x_row_stride, nullptr, false, 1.0, h_out,
                        w_out, d_y, y_image_stride, y_row_stride, d_ws, ws_bytes, stream);
}

int mm_zoom2d_ragged_f32(int32_t order, int32_t mode, double cval, int32_t flags, const float* d_x, int64_t images,
                         int64_t h, int64_t w_max, int64_t x_image_stride, int64_t x_row_stride,
                         const int64_t* d_widths, double zoom_x, int64_t h_out, int64_t w_out, float* d_y,
                         int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return zm_run<float>(order, mode, cval, flags, d_x, images, h, w_max, x_image_stride, x_row_stride, d_widths, true, zoom_x,
                       h_out, w_out, d_y, y_image_stride, y_row_stride, d_ws, ws_bytes, stream);
}

int mm_zoom2d_ragged_f64(int32_t order, int32_t mode, double cval, int32_t flags, const double* d_x, int64_t images,
                         int64_t h, int64_t w_max, int64_t x_image_stride, int64_t x_row_stride,
                         const int64_t* d_widths, double zoom_x, int64_t h_out, int64_t w_out, double* d_y,
                         int64_t y_image_stride, int64_t y_row_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return zm_run<double>(order, mode, cval, flags, d_x, images, h, w_max, x_image_stride, x_row_stride, d_widths, true, zoom_x,
                        h_out, w_out, d_y, y_image_stride, y_row_stride, d_ws, ws_bytes, stream);
}

}  // extern "C"
