// Praat-style spectrogram (include/modmfcc_pspec.h): band powers of short windowed frames whose
// first samples the host lists per row.
//
//   pspec_kernel<T, LOG2N>  one workgroup per (row, tile of mm_pspec_tile_frames consecutive frames).
//     front      every wave reads the tile's table entries and finds the lowest valid first sample; the workgroup copies
//                the samples from there on, `span` per channel, to LDS ONCE (consecutive frames overlap by about 80 %) and
//                builds its own twiddle table there (sincospi in float64, rounded once to T).  A wave cuts its frames out of
//                the copy at the table's offsets; a frame that does not lie in the copy is read from memory -- the same
//                values either way.
//     transform  per frame and channel: window, the packed real transform in the wave's LDS buffer (wave_cfft_lds +
//                real_split of mm_common.h, in T), |X|^2 added to float64 accumulators for the bins below n_freqs * bw only.
//     back       the accumulators go to the wave's buffer as float64; a lane per band adds its bw bins in ascending order,
//                divides by the channels, scales, rounds once to T and writes out[band][frame] of the workgroup's tile in
//                LDS; after a barrier a store instruction writes consecutive FRAMES of one band.
//
// Which wave transforms a frame does not matter: a frame's arithmetic is a function of its samples and of p alone, so a
// row's bits do not depend on the batch, the strides or the row's index.  A table entry is used only if 0 <= s and
// s + nw <= n_max; every other entry yields +0.0 and no read.
#include "mm_common.h"
#include "../../include/modmfcc_pspec.h"

#define PSPEC_MIN_LOG2N 5
#define PSPEC_MAX_LOG2N 12

namespace {

template <class T> struct PspecCplx;
template <> struct PspecCplx<float> { using type = float2; };
template <> struct PspecCplx<double> { using type = double2; };

// The shape of a transform length: what one workgroup holds.  (The same for both types but for the waves of the float64
// 4096-point transform, whose four buffers of 32 KiB would leave no room for the rest.)
struct PspecShape { int log2n, waves, tile_base, stage_cap, out_cap; };

PspecShape pspec_shape(int log2n, size_t elem) {
  const int nfft = 1 << log2n;
  PspecShape s;
  s.log2n = log2n;
  s.waves = (elem == 8 && log2n == 12) ? 2 : 4;                                   // PSPEC_WAVES
  s.tile_base = log2n <= 10 ? 32 : 16;                                            // frames per tile at the most
  s.stage_cap = log2n <= 10 ? std::max(4 * nfft, 2048) : log2n == 11 ? 2 * nfft : nfft;   // staged samples, all channels
  s.out_cap = log2n <= 10 ? 8192 : log2n == 11 ? 4096 : 2048;                     // values of the output tile
  return s;
}

int pspec_tile(const mm_pspec_params& p) {
  const PspecShape s = pspec_shape(ilog2(p.nfft), 8);
  int tile = s.tile_base;
  while (tile > 1 && (int64_t)tile * p.n_freqs > s.out_cap) tile >>= 1;
  return tile;
}

template <class T>
struct PspecArgs {
  const T* x;
  const T* w;
  const int32_t* start;
  T* y;
  int64_t n_max, x_row, x_chan, t_max, start_row, y_row, y_band;
  double scale;
  int nw, bw, n_freqs, channels, tile, tiles, span, db;    // span: staged samples per channel (0: none)
};

// waves of a workgroup: pspec_shape's, at compile time
#define PSPEC_WAVES(T, LOG2N) ((sizeof(T) == 8 && (LOG2N) == 12) ? 2 : 4)

template <class T, int LOG2N>
__global__ __launch_bounds__(64 * PSPEC_WAVES(T, LOG2N)) void pspec_kernel(PspecArgs<T> a) {
  using C2 = typename PspecCplx<T>::type;
  constexpr int WAVES = PSPEC_WAVES(T, LOG2N);
  constexpr int NFFT = 1 << LOG2N, NC = NFFT / 2, LOG2NC = LOG2N - 1;
  constexpr int NP = NC >= 64 ? NC / 64 : 1;           // sample pairs per lane
  constexpr int NA = NC / 128 + 1;                     // bin pairs (k, NC - k), k = lane + 64 i <= NC / 2, per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // LDS: [WAVES] transform buffers of NC complex | NC twiddles | the staged samples | the output tile [n_freqs][tile + 1]
  C2* zs = reinterpret_cast<C2*>(smem);
  C2* z = zs + (size_t)wave * NC;
  C2* tw = zs + (size_t)WAVES * NC;
  T* stage = reinterpret_cast<T*>(tw + NC);
  T* otile = stage + (size_t)a.span * a.channels;
  const int opitch = a.tile + 1;

  const int64_t row = blockIdx.x / a.tiles;
  const int64_t k0 = (int64_t)(blockIdx.x % a.tiles) * a.tile;
  const int32_t* tab = a.start + row * a.start_row + k0;
  const T* xr = a.x + row * a.x_row;
  const int nbins = a.n_freqs * a.bw;

  // the tile's entries, one per lane (tile <= 32): the lowest valid first sample, in every wave alike
  int s_mine = -1;
  if (lane < a.tile && k0 + lane < a.t_max) {
    const int s = tab[lane];
    if (s >= 0 && (int64_t)s + a.nw <= a.n_max) s_mine = s;
  }
  int s_min = s_mine < 0 ? 0x7FFFFFFF : s_mine;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s_min = min(s_min, __shfl_xor(s_min, o, 64));
  const bool any = s_min != 0x7FFFFFFF;                // (workgroup-uniform)

  if (any) {
    for (int k = threadIdx.x; k < NC; k += 64 * WAVES) {
      double sn, cs;
      sincospi(-2.0 * (double)k / (double)NFFT, &sn, &cs);
      tw[k] = mm_cplx((T)cs, (T)sn);
    }
    for (int c = 0; c < a.channels; ++c) {
      const T* xc = xr + c * a.x_chan + s_min;
      T* sc = stage + (size_t)c * a.span;
      for (int i = threadIdx.x; i < a.span; i += 64 * WAVES)
        if ((int64_t)s_min + i < a.n_max) sc[i] = xc[i];
    }
  }
  __syncthreads();

  for (int f = wave; f < a.tile; f += WAVES) {         // (wave-uniform)
    const int s = __shfl(s_mine, f, 64);
    if (s < 0) {
      for (int j = lane; j < a.n_freqs; j += 64) otile[j * opitch + f] = (T)0;      // (in dB too: no frame, no level)
      continue;
    }
    const bool staged = s - s_min + a.nw <= a.span;
    double accA[NA], accB[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) accA[i] = accB[i] = 0.0;
    for (int c = 0; c < a.channels; ++c) {
      // (two calls, not one pointer chosen between LDS and memory: each loop keeps its address space)
      auto fill = [&](const T* src) {
#pragma unroll 4
        for (int i = 0; i < NP; ++i) {
          const int n = lane + 64 * i, j = 2 * n;
          if (n < NC) {
            const T y0 = j < a.nw ? src[j] * a.w[j] : (T)0, y1 = j + 1 < a.nw ? src[j + 1] * a.w[j + 1] : (T)0;
            z[__brev((unsigned)n) >> (32 - LOG2NC)] = mm_cplx(y0, y1);
          }
        }
      };
      if (staged) fill(stage + (size_t)c * a.span + (s - s_min));
      else fill(xr + c * a.x_chan + s);
      wave_lds_sync();
      wave_cfft_lds(z, LOG2NC, tw, lane, NFFT);
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int k = lane + 64 * i;
        if (k <= NC / 2 && (k < nbins || NC - k < nbins)) {      // the bins behind the last band are never formed
          C2 xa, xb;
          real_split(z, k, NC, tw, 1, xa, xb);
          accA[i] += (double)(xa.x * xa.x + xa.y * xa.y);
          accB[i] += (double)(xb.x * xb.x + xb.y * xb.y);
        }
      }
      wave_lds_sync();
    }
    // the powers of the bins below nbins (<= NC) as float64 over the wave's buffer (NC float64 fit in NC complex of T)
    double* pd = reinterpret_cast<double*>(z);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) {
        if (k < nbins) pd[k] = accA[i];
        if (NC - k != k && NC - k < nbins) pd[NC - k] = accB[i];
      }
    }
    wave_lds_sync();
    const double inv_c = 1.0 / (double)a.channels;     // (exact for 1, 2, 4, 8 channels; one rounding otherwise)
    for (int j = lane; j < a.n_freqs; j += 64) {
      const double* q = pd + (size_t)j * a.bw;
      double sum = q[0];
      for (int b = 1; b < a.bw; ++b) sum += q[b];
      const double v = a.channels == 1 ? sum * a.scale : sum * inv_c * a.scale;
      otile[j * opitch + f] = (T)(a.db ? 10.0 * log10(v) : v);
    }
    wave_lds_sync();
  }
  __syncthreads();

  // out[row][band][k0 .. k0 + tile): consecutive threads write consecutive frames of one band
  T* yr = a.y + row * a.y_row + k0;
  const int64_t left = a.t_max - k0;
  const int valid = left < a.tile ? (int)left : a.tile;
  for (int i = threadIdx.x; i < a.n_freqs * a.tile; i += 64 * WAVES) {
    const int j = i / a.tile, f = i - j * a.tile;      // (tile is a power of two)
    if (f < valid) yr[j * a.y_band + f] = otile[j * opitch + f];
  }
}

template <class T>
using PspecKernel = void (*)(PspecArgs<T>);

template <class T>
PspecKernel<T> pspec_kernel_of(int log2n) {
  switch (log2n) {
    case 5: return pspec_kernel<T, 5>;
    case 6: return pspec_kernel<T, 6>;
    case 7: return pspec_kernel<T, 7>;
    case 8: return pspec_kernel<T, 8>;
    case 9: return pspec_kernel<T, 9>;
    case 10: return pspec_kernel<T, 10>;
    case 11: return pspec_kernel<T, 11>;
    case 12: return pspec_kernel<T, 12>;
  }
  return nullptr;
}

template <class T>
int pspec_launch(const PspecArgs<T>& a, const PspecShape& s, int64_t blocks, size_t lds, hipStream_t st) {
  static PerDeviceOnce once;
  const int rc = per_device_once(once, "pspec_kernel", [] {
    for (int l = PSPEC_MIN_LOG2N; l <= PSPEC_MAX_LOG2N; ++l)
      if (hipFuncSetAttribute((const void*)pspec_kernel_of<T>(l), hipFuncAttributeMaxDynamicSharedMemorySize,
                              MM_LM_LDS_MAX) != hipSuccess)
        return false;
    return true;
  });
  if (rc) return rc;
  const auto kernel = pspec_kernel_of<T>(s.log2n);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * s.waves), lds, st, a);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

template <class T>
int pspec_run(const mm_pspec_params* p, const T* d_x, int64_t rows, int64_t n_max, int64_t x_row, int64_t x_chan, const T* d_w,
              const int32_t* d_start, int64_t t_max, int64_t start_row, T* d_y, int64_t y_row, int64_t y_band, void* stream) {
  const int rc = mm_pspec_check(p);
  if (rc != MM_OK) return rc;
  if (!d_x || !d_w || !d_start || !d_y || rows < 1 || t_max < 1 || n_max < p->nw) return MM_ERR_INVALID_ARG;
  if (n_max >= 0x7FFFFFFFll - MM_PSPEC_MAX_NFFT || t_max > 0x7FFFFFFFll) return MM_ERR_INVALID_ARG;
  if (x_chan < n_max || (rows > 1 && x_row < (int64_t)p->channels * x_chan)) return MM_ERR_INVALID_ARG;
  if (y_band < t_max || y_row < (int64_t)p->n_freqs * y_band) return MM_ERR_INVALID_ARG;
  if (start_row != 0 && start_row < t_max) return MM_ERR_INVALID_ARG;
  const int log2n = ilog2(p->nfft);
  const PspecShape s = pspec_shape(log2n, sizeof(T));
  const int tile = pspec_tile(*p);
  const int64_t tiles = (t_max + tile - 1) / tile;
  if (rows > 0x7FFFFFFFll / tiles) return MM_ERR_INVALID_ARG;
  // what a workgroup stages per channel: the tile's span where all channels fit, their share of the buffer otherwise
  // (at least a window, or nothing: the frames behind it are read from memory)
  int span = std::min<int64_t>(std::min<int64_t>(p->span, n_max), s.stage_cap / p->channels);
  if (span < p->nw) span = 0;
  const int nc = p->nfft / 2;
  const size_t lds = ((size_t)s.waves * nc + nc) * 2 * sizeof(T) +
                     ((size_t)span * p->channels + (size_t)p->n_freqs * (tile + 1)) * sizeof(T);
  if (lds > MM_LM_LDS_MAX) return MM_ERR_UNSUPPORTED;
  const PspecArgs<T> a = {d_x, d_w, d_start, d_y, n_max, x_row, x_chan, t_max, start_row, y_row, y_band, p->scale,
                          p->nw, p->bw, p->n_freqs, p->channels, tile, (int)tiles, span, p->flags & MM_PSPEC_DB};
  return pspec_launch<T>(a, s, rows * tiles, lds, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int mm_pspec_version(void) { return MM_PSPEC_VERSION; }

int mm_pspec_check(const mm_pspec_params* p) {
  if (!p) return MM_ERR_INVALID_ARG;
  if (p->nw < 2 || p->nfft < 1 || p->bw < 1 || p->n_freqs < 1 || p->channels < 1 || p->span < 0) return MM_ERR_INVALID_ARG;
  if (!(p->scale > 0.0) || !std::isfinite(p->scale) || (p->flags & ~MM_PSPEC_DB) || p->reserved) return MM_ERR_INVALID_ARG;
  if (p->nfft < (1 << PSPEC_MIN_LOG2N) || p->nfft > MM_PSPEC_MAX_NFFT || (p->nfft & (p->nfft - 1))) return MM_ERR_UNSUPPORTED;
  if (p->nw > p->nfft || p->channels > MM_PSPEC_MAX_CHANNELS) return MM_ERR_UNSUPPORTED;
  if ((int64_t)p->n_freqs * p->bw > p->nfft / 2) return MM_ERR_INVALID_ARG;
  return MM_OK;
}

int32_t mm_pspec_tile_frames(const mm_pspec_params* p) {
  const int rc = mm_pspec_check(p);
  return rc != MM_OK ? rc : pspec_tile(*p);
}

int mm_pspec_f32(const mm_pspec_params* p, const float* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                 int64_t x_channel_stride, const float* d_w, const int32_t* d_start, int64_t t_max,
                 int64_t start_row_stride, float* d_y, int64_t y_row_stride, int64_t y_band_stride, void* stream) {
  return pspec_run<float>(p, d_x, rows, n_max, x_row_stride, x_channel_stride, d_w, d_start, t_max, start_row_stride, d_y,
                          y_row_stride, y_band_stride, stream);
}

int mm_pspec_f64(const mm_pspec_params* p, const double* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                 int64_t x_channel_stride, const double* d_w, const int32_t* d_start, int64_t t_max,
                 int64_t start_row_stride, double* d_y, int64_t y_row_stride, int64_t y_band_stride, void* stream) {
  return pspec_run<double>(p, d_x, rows, n_max, x_row_stride, x_channel_stride, d_w, d_start, t_max, start_row_stride, d_y,
                           y_row_stride, y_band_stride, stream);
}

}  // extern "C"
