// Welch cross spectrum and coherence (include/modmfcc_modcsd.h): scipy.signal.csd / coherence / welch along pairs of float32
// rows, a length per pair, on the handle of mm_modpsd.hip.
//
//   modcsd_kernel<LOG2N>   one workgroup (4 waves) per (pair, chunk of MM_MODPSD_CHUNK = 32 segments); segment i of a pair
//                          belongs to chunk i / 32 and, inside it, to wave i % 4, which takes its segments in ascending
//                          order -- the plan of modpsd_kernel.  A wave reads both sides of its segment for the detrend
//                          statistics (float64 sums over the wave) and again, from the cache, to subtract the trends in
//                          float64, writes z = w x + i w y bit-reversed into its LDS buffer, brings either side to a norm
//                          in [1, 2) by a power of two (exact; a quiet side must not carry a loud side's rounding error)
//                          and transforms the nfft complex points there (mcsd_cfft_lds: float64 butterflies, float32 points).  Lane l then holds
//                          the bins k = l + 64 i <= nfft / 2, the powers of two undone in float64:
//                              X[k] = (Z[k] + conj Z[N - k]) / 2        Y[k] = (Z[k] - conj Z[N - k]) / 2i
//                          (the halving is exact) and adds |X|^2, |Y|^2, Re and Im of conj(X) Y -- products of float32
//                          values formed in float64, exact -- to four float64 accumulators per bin.  The four waves' sums
//                          meet through LDS as (w0 + w1) + (w2 + w3), one accumulator kind at a time.  A batch whose pairs
//                          have one chunk each ends here: coherence from the sums, scale, round, store.  Otherwise every
//                          chunk stores its float64 sums to the workspace and
//   modcsd_finish_kernel   adds a pair's chunks in ascending order and does the same.
//
// Which wave adds which segment in which order is a function of the segment's index alone, the chunk sums are added in
// ascending order whichever kernel does it, and the two kernels finish a bin with the same function (explicit fma: no
// contraction the compiler could choose differently in either): a pair's bits do not depend on rows, n_max, y_group or
// the other pairs.  No atomics.  A pair without a segment is NaN.
#include "mm_common.h"
#include "../../include/modmfcc_modcsd.h"
#include "mm_welch.hip.inc"

#define MCSD_MIN_LOG2N 5
#define MCSD_MAX_LOG2N 11       // 17 bins x 4 float64 sums = 136 VGPRs per lane; nfft 4096 would need 264

struct ModcsdArgs {
  const float* x;
  const float* y;
  const int64_t* lens;
  const float* window;
  const float2* tw;
  float* pxx;            // any of the four may be nullptr
  float* pyy;
  float* pxy;            // [rows][out_stride][2]
  float* coh;
  double* part;          // [rows][max_chunks][4][bins] chunk sums, or nullptr: one chunk per pair, finished directly
  int64_t n_max, x_stride, y_stride, y_group, out_stride, max_chunks;
  double scale;
  int nperseg, step, noverlap, detrend;
};

// bin k of a pair from its float64 sums over the K segments: sxx = sum |X|^2, syy = sum |Y|^2, (sre, sim) = sum conj(X) Y
__device__ __forceinline__ void mcsd_finish_bin(const ModcsdArgs& p, int64_t row, int k, int nh, double sxx, double syy,
                                                double sre, double sim, int64_t K) {
  const double d = (k == 0 || k == nh) ? 1.0 : 2.0;
  const double f = p.scale * d / (double)K;
  const int64_t o = row * p.out_stride + k;
  if (p.pxx) p.pxx[o] = (float)(sxx * f);
  if (p.pyy) p.pyy[o] = (float)(syy * f);
  if (p.pxy) {
    p.pxy[2 * o] = (float)(sre * f);
    p.pxy[2 * o + 1] = (float)(sim * f);
  }
  if (p.coh) p.coh[o] = (float)(fma(sre, sre, sim * sim) / (sxx * syy));     // 0 / 0 = NaN, as scipy's
}

__device__ __forceinline__ void mcsd_nan_bin(const ModcsdArgs& p, int64_t row, int k) {
  const float nan = __builtin_nanf("");
  const int64_t o = row * p.out_stride + k;
  if (p.pxx) p.pxx[o] = nan;
  if (p.pyy) p.pyy[o] = nan;
  if (p.pxy) { p.pxy[2 * o] = nan; p.pxy[2 * o + 1] = nan; }
  if (p.coh) p.coh[o] = nan;
}

// floor(log2(sqrt(ss))) of a side's energy; 0 (no scaling) for a side without energy and for one that is not finite
__device__ __forceinline__ int mcsd_half_exponent(double ss) {
  if (!(ss > 0.0) || !(ss < __builtin_huge_val())) return 0;
  return ilogb(ss) >> 1;
}

// wave_cfft_lds of mm_common.h (in-place radix-2 DIT over a wave-private LDS buffer, input bit-reversed) with every butterfly
// evaluated in float64 -- the float32 points and twiddles are exact in it, w b is rounded once -- and each stored component
// rounded to float32 once.  Where neither side of a pair has a true amplitude the cross spectrum is the PRODUCT of the two
// sides' transform noise: the float32 butterflies (three roundings per component) left 6 x the reference's there.
__device__ __forceinline__ void mcsd_cfft_lds(float2* z, int log2n, const float2* __restrict__ tw, int lane) {
  const int n = 1 << log2n;
  for (int s = 1; s <= log2n; ++s) {
    const int half = 1 << (s - 1);
    const int tw_stride = MM_TW_N >> s;
    for (int j = lane; j < (n >> 1); j += 64) {
      const int pos = j & (half - 1);
      const int i0 = ((j >> (s - 1)) << s) + pos;
      const int i1 = i0 + half;
      const float2 w = tw[pos * tw_stride];
      const float2 a = z[i0], b = z[i1];
      const double wr = w.x, wi = w.y, br = b.x, bi = b.y;
      const double tr = fma(wr, br, -(wi * bi)), ti = fma(wr, bi, wi * br);      // (the inner products are exact)
      z[i0] = make_float2((float)((double)a.x + tr), (float)((double)a.y + ti));
      z[i1] = make_float2((float)((double)a.x - tr), (float)((double)a.y - ti));
    }
    wave_lds_sync();
  }
}

template <int LOG2N>
__global__ __launch_bounds__(64 * MPSD_WAVES) void modcsd_kernel(ModcsdArgs p) {
  constexpr int N = 1 << LOG2N;                        // complex points of the transform
  constexpr int NH = N / 2;                            // bins 0 .. NH
  constexpr int NP = N >= 64 ? N / 64 : 1;             // samples of either side per lane
  constexpr int NB = NH / 64 + 1;                      // bins k = lane + 64 i <= NH per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float2* z = reinterpret_cast<float2*>(smem) + (size_t)wave * N;

  const int64_t row = blockIdx.x / p.max_chunks, chunk = blockIdx.x % p.max_chunks;
  const int64_t len = mpsd_row_len(p.lens, row, p.n_max);
  const int64_t K = mpsd_segments(len, p.nperseg, p.noverlap, p.step);
  const int64_t seg0 = chunk * MM_MODPSD_CHUNK;
  if (K == 0) {                                        // (workgroup-uniform)
    if (!p.part && chunk == 0)
      for (int k = threadIdx.x; k <= NH; k += 64 * MPSD_WAVES) mcsd_nan_bin(p, row, k);
    return;
  }
  if (seg0 >= K) return;                               // (workgroup-uniform)
  const int n_seg = (int)(K - seg0 < MM_MODPSD_CHUNK ? K - seg0 : MM_MODPSD_CHUNK);
  const float* ax = p.x + row * p.x_stride;
  const float* ay = p.y + (row / p.y_group) * p.y_stride;
  const double centre = 0.5 * (double)(p.nperseg - 1);
  // sum (j - centre)^2 = n (n^2 - 1) / 12
  const double sxx = (double)p.nperseg * ((double)p.nperseg * (double)p.nperseg - 1.0) / 12.0;

  double acc[4][NB];                                   // |X|^2, |Y|^2, Re conj(X) Y, Im conj(X) Y
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[q][i] = 0.0;

  for (int s = wave; s < n_seg; s += MPSD_WAVES) {     // (wave-uniform)
    const float* xs = ax + (seg0 + s) * (int64_t)p.step;   // samples xs[0 .. nperseg), ys[0 .. nperseg): all below len
    const float* ys = ay + (seg0 + s) * (int64_t)p.step;
    // as in modpsd_kernel the segment is read once for the detrend statistics and once more (from the cache) to be
    // transformed
    double mx = 0.0, my = 0.0, slx = 0.0, sly = 0.0;
    if (p.detrend) {
      double s0x = 0.0, s1x = 0.0, s0y = 0.0, s1y = 0.0;
#pragma unroll 4
      for (int i = 0; i < NP; ++i) {
        const int j = lane + 64 * i;
        const double x0 = j < p.nperseg ? (double)xs[j] : 0.0, y0 = j < p.nperseg ? (double)ys[j] : 0.0;
        s0x += x0;
        s0y += y0;
        if (p.detrend == 2) {
          s1x += ((double)j - centre) * x0;
          s1y += ((double)j - centre) * y0;
        }
      }
      mx = mpsd_wave_sum(s0x) / (double)p.nperseg;
      my = mpsd_wave_sum(s0y) / (double)p.nperseg;
      if (p.detrend == 2 && p.nperseg > 1) {
        slx = mpsd_wave_sum(s1x) / sxx;
        sly = mpsd_wave_sum(s1y) / sxx;
      }
    }
    double ssx = 0.0, ssy = 0.0;                       // the energy either side puts into the transform
#pragma unroll 4
    for (int i = 0; i < NP; ++i) {
      const int j = lane + 64 * i;
      if (j < N) {
        float x0 = 0.0f, y0 = 0.0f;
        if (j < p.nperseg) {
          x0 = xs[j];
          y0 = ys[j];
          if (p.detrend) {
            const double tj = (double)j - centre;
            x0 = (float)((double)x0 - (mx + slx * tj));
            y0 = (float)((double)y0 - (my + sly * tj));
          }
        }
        const float w = p.window[j];
        const float vx = x0 * w, vy = y0 * w;
        ssx = fma((double)vx, (double)vx, ssx);
        ssy = fma((double)vy, (double)vy, ssy);
        z[__brev((unsigned)j) >> (32 - LOG2N)] = make_float2(vx, vy);
      }
    }
    // The float32 transform's rounding error in X and in Y is that of the whole of z: a quiet side beside a loud one would
    // carry the loud one's error.  Either side is therefore brought to a norm in [1, 2) by a power of two -- exact, and
    // undone exactly on the float64 side of the split -- before the transform.  (Each lane rescales the points it wrote.)
    ssx = mpsd_wave_sum(ssx);
    ssy = mpsd_wave_sum(ssy);
    const int hx = mcsd_half_exponent(ssx), hy = mcsd_half_exponent(ssy);       // (wave-uniform)
    if (hx | hy) {
      const double dx = ldexp(1.0, -hx), dy = ldexp(1.0, -hy);
#pragma unroll 4
      for (int i = 0; i < NP; ++i) {
        const int j = lane + 64 * i;
        if (j < N) {
          float2* q = z + (__brev((unsigned)j) >> (32 - LOG2N));
          const float2 v = *q;
          *q = make_float2((float)((double)v.x * dx), (float)((double)v.y * dy));
        }
      }
    }
    // A side of zeros takes the factor 0: what the transform's rounding carries over from the other side (Z[k] and
    // conj Z[N - k] of a real row differ in their last bits) must not become a power of the zero row.  (NaN != 0.)
    const double ux = ssx == 0.0 ? 0.0 : ldexp(1.0, hx), uy = ssy == 0.0 ? 0.0 : ldexp(1.0, hy);
    wave_lds_sync();
    mcsd_cfft_lds(z, LOG2N, p.tw, lane);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = lane + 64 * i;
      if (k <= NH) {
        const float2 a = z[k], b = z[(N - k) & (N - 1)];
        const double xr = (double)(0.5f * (a.x + b.x)) * ux, xi = (double)(0.5f * (a.y - b.y)) * ux;
        const double yr = (double)(0.5f * (a.y + b.y)) * uy, yi = (double)(0.5f * (b.x - a.x)) * uy;
        acc[0][i] += fma(xr, xr, xi * xi);
        acc[1][i] += fma(yr, yr, yi * yi);
        acc[2][i] += fma(xr, yr, xi * yi);
        acc[3][i] += fma(xr, yi, -(xi * yr));
      }
    }
    wave_lds_sync();
  }

  // (w0 + w1) + (w2 + w3) through LDS, one accumulator kind at a time: the odd waves hand theirs to the even ones, then
  // wave 2 to wave 0.  The two slots of NH + 1 float64 lie over the transform buffers of other waves: a barrier in front
  // of each hand-off.
  double* ex = reinterpret_cast<double*>(smem);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const bool gives = round == 0 ? (wave & 1) : wave == 2;
      const bool takes = round == 0 ? !(wave & 1) : wave == 0;
      double* slot = ex + (size_t)(round == 0 ? (wave >> 1) : 0) * (NH + 1);
      __syncthreads();
      if (gives) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int k = lane + 64 * i;
          if (k <= NH) slot[k] = acc[q][i];
        }
      }
      __syncthreads();
      if (takes) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int k = lane + 64 * i;
          if (k <= NH) acc[q][i] += slot[k];
        }
      }
    }
  }
  if (wave != 0) return;
  if (p.part) {
    double* o = p.part + (row * p.max_chunks + chunk) * (int64_t)(4 * (NH + 1));
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int k = lane + 64 * i;
        if (k <= NH) o[q * (NH + 1) + k] = acc[q][i];
      }
  } else {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = lane + 64 * i;
      if (k <= NH) mcsd_finish_bin(p, row, k, NH, acc[0][i], acc[1][i], acc[2][i], acc[3][i], K);
    }
  }
}

// ceil(bins / 256) workgroups per pair: a thread per bin adds the pair's chunk sums in ascending order
static __global__ __launch_bounds__(256) void modcsd_finish_kernel(ModcsdArgs p, int nh) {
  const int per_row = (nh + 1 + 255) / 256;
  const int k = (int)(blockIdx.x % per_row) * 256 + threadIdx.x;
  if (k > nh) return;
  const int64_t row = blockIdx.x / per_row;
  const int64_t K = mpsd_segments(mpsd_row_len(p.lens, row, p.n_max), p.nperseg, p.noverlap, p.step);
  if (K == 0) { mcsd_nan_bin(p, row, k); return; }
  const int64_t chunks = (K + MM_MODPSD_CHUNK - 1) / MM_MODPSD_CHUNK;
  const int64_t bins = nh + 1;
  const double* q = p.part + row * p.max_chunks * (4 * bins) + k;
  double s[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) s[a] = q[a * bins];
  for (int64_t c = 1; c < chunks; ++c) {
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] += q[c * (4 * bins) + a * bins];
  }
  mcsd_finish_bin(p, row, k, nh, s[0], s[1], s[2], s[3], K);
}

using ModcsdKernel = void (*)(ModcsdArgs);
static ModcsdKernel mcsd_kernel_of(int log2n) {
  switch (log2n) {
    case 5: return modcsd_kernel<5>;
    case 6: return modcsd_kernel<6>;
    case 7: return modcsd_kernel<7>;
    case 8: return modcsd_kernel<8>;
    case 9: return modcsd_kernel<9>;
    case 10: return modcsd_kernel<10>;
    case 11: return modcsd_kernel<11>;
  }
  return nullptr;
}

extern "C" {

int mm_modcsd_version(void) { return 1; }

int mm_modcsd_check(const mm_modpsd_params* p) {
  const int rc = mm_modpsd_check(p);
  if (rc != MM_OK) return rc;
  if (p->nfft < (1 << MCSD_MIN_LOG2N) || p->nfft > (1 << MCSD_MAX_LOG2N)) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

size_t mm_modcsd_workspace_bytes(const mm_modpsd* h, int64_t rows, int64_t n_max) {
  if (!h || rows < 1 || n_max < 1 || mm_modcsd_check(&h->p) != MM_OK) return 0;
  const int64_t chunks = mpsd_max_chunks(h, n_max);
  if (chunks <= 1) return 0;
  return (size_t)rows * (size_t)chunks * 4 * (size_t)(h->p.nfft / 2 + 1) * sizeof(double);
}

int mm_modcsd_f32(const mm_modpsd* h, const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const float* d_y,
                  int64_t y_stride, int64_t y_group, const int64_t* d_lens, float* d_pxx, float* d_pyy, float* d_pxy,
                  float* d_coh, int64_t out_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_x || !d_y || rows < 1 || n_max < 1 || x_stride < n_max || y_stride < n_max || y_group < 1)
    return MM_ERR_INVALID_ARG;
  if (!d_pxx && !d_pyy && !d_pxy && !d_coh) return MM_ERR_INVALID_ARG;
  const int rc = mm_modcsd_check(&h->p);
  if (rc != MM_OK) return rc;
  const int nh = h->p.nfft / 2;
  if (out_stride < nh + 1) return MM_ERR_INVALID_ARG;
  if (!d_lens && n_max < h->p.nperseg) return MM_ERR_INVALID_ARG;
  const int64_t chunks = mpsd_max_chunks(h, n_max);
  const size_t need = mm_modcsd_workspace_bytes(h, rows, n_max);
  if (need && (!d_ws || ((uintptr_t)d_ws & 7))) return MM_ERR_INVALID_ARG;
  if (ws_bytes < need) return MM_ERR_WORKSPACE;
  const int64_t finish_per_row = (nh + 1 + 255) / 256;
  if (rows > 0x7FFFFFFF / chunks || rows > 0x7FFFFFFF / finish_per_row) return MM_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  ModcsdArgs a;
  a.x = d_x; a.y = d_y; a.lens = d_lens; a.window = h->d_window; a.tw = h->d_tw;
  a.pxx = d_pxx; a.pyy = d_pyy; a.pxy = d_pxy; a.coh = d_coh;
  a.part = chunks > 1 ? (double*)d_ws : nullptr;
  a.n_max = n_max; a.x_stride = x_stride; a.y_stride = y_stride; a.y_group = y_group; a.out_stride = out_stride;
  a.max_chunks = chunks;
  a.scale = h->scale;
  a.nperseg = h->p.nperseg; a.step = h->p.nperseg - h->p.noverlap; a.noverlap = h->p.noverlap; a.detrend = h->p.detrend;
  // LDS: the four transform buffers, 8 nfft bytes each (64 KiB at nfft 2048); the two hand-off slots of nfft / 2 + 1
  // float64 lie over them
  const size_t lds = (size_t)MPSD_WAVES * h->p.nfft * sizeof(float2);
  hipLaunchKernelGGL(mcsd_kernel_of(h->log2n), dim3((unsigned)(rows * chunks)), dim3(64 * MPSD_WAVES), lds, st, a);
  if (chunks > 1)
    hipLaunchKernelGGL(modcsd_finish_kernel, dim3((unsigned)(rows * finish_per_row)), dim3(256), 0, st, a, nh);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
