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
// the other pairs.  No atomics.  A pair without a segment is NaN.  The plan, the trend, the hand-off, the chunk sum, the
// shared refusals and the launch are mm_welch.hip.inc's: the code modpsd_kernel and mm_modpsd_f32 run.
#include "mm_common.h"
#include "../../include/modmfcc_modcsd.h"
#include "mm_welch.hip.inc"

#define MCSD_MIN_LOG2N 5
#define MCSD_MAX_LOG2N 11       // 17 bins x 4 float64 sums = 136 VGPRs per lane; nfft 4096 would need 264

struct ModcsdArgs {
  WelchArgs w;           // part: [rows][max_chunks][4][bins]
  const float* x;
  const float* y;
  float* pxx;            // any of the four may be nullptr
  float* pyy;
  float* pxy;            // [rows][out_stride][2]
  float* coh;
  int64_t x_stride, y_stride, y_group, out_stride;
};

// bin k of a pair from its float64 sums over the K segments: sxx = sum |X|^2, syy = sum |Y|^2, (sre, sim) = sum conj(X) Y
__device__ __forceinline__ void mcsd_finish_bin(const ModcsdArgs& p, int64_t row, int k, int nh, double sxx, double syy,
                                                double sre, double sim, int64_t K) {
  const double d = (k == 0 || k == nh) ? 1.0 : 2.0;
  const double f = p.w.scale * d / (double)K;
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

  const WelchArgs& w = p.w;
  const WelchPlan g = welch_plan(w, blockIdx.x);
  if (g.state == WELCH_NAN && !w.part && g.chunk == 0)
    for (int k = threadIdx.x; k <= NH; k += 64 * MPSD_WAVES) mcsd_nan_bin(p, g.row, k);
  if (g.state != WELCH_WORK) return;                   // (workgroup-uniform)
  const float* ax = p.x + g.row * p.x_stride;
  const float* ay = p.y + (g.row / p.y_group) * p.y_stride;
  const WelchDetrend d = welch_detrend(w.nperseg);

  double acc[4][NB];                                   // |X|^2, |Y|^2, Re conj(X) Y, Im conj(X) Y
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[q][i] = 0.0;

  for (int s = wave; s < g.n_seg; s += MPSD_WAVES) {   // (wave-uniform)
    const float* xs = ax + (g.seg0 + s) * (int64_t)w.step; // samples xs[0 .. nperseg), ys[0 .. nperseg): all below len
    const float* ys = ay + (g.seg0 + s) * (int64_t)w.step;
    // as in modpsd_kernel the segment is read once for the detrend statistics and once more (from the cache) to be
    // transformed
    WelchTrend tx = {0.0, 0.0}, ty = {0.0, 0.0};
    if (w.detrend) {
      double s0x = 0.0, s1x = 0.0, s0y = 0.0, s1y = 0.0;
#pragma unroll 4
      for (int i = 0; i < NP; ++i) {
        const int j = lane + 64 * i;
        const double x0 = j < w.nperseg ? (double)xs[j] : 0.0, y0 = j < w.nperseg ? (double)ys[j] : 0.0;
        s0x += x0;
        s0y += y0;
        if (w.detrend == 2) {
          s1x += ((double)j - d.centre) * x0;
          s1y += ((double)j - d.centre) * y0;
        }
      }
      tx.mean = welch_mean(s0x, w);
      ty.mean = welch_mean(s0y, w);
      tx.slope = welch_slope(s1x, w, d);
      ty.slope = welch_slope(s1y, w, d);
    }
    double ssx = 0.0, ssy = 0.0;                       // the energy either side puts into the transform
#pragma unroll 4
    for (int i = 0; i < NP; ++i) {
      const int j = lane + 64 * i;
      if (j < N) {
        float x0 = 0.0f, y0 = 0.0f;
        if (j < w.nperseg) {
          x0 = xs[j];
          y0 = ys[j];
          if (w.detrend) {
            x0 = welch_subtract(x0, j, tx, d);
            y0 = welch_subtract(y0, j, ty, d);
          }
        }
        const float wj = w.window[j];
        const float vx = x0 * wj, vy = y0 * wj;
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
    mcsd_cfft_lds(z, LOG2N, w.tw, lane);
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

  // every (bin, accumulator of kind q) of this lane
  auto kind = [&](int q, auto f) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = lane + 64 * i;
      if (k <= NH) f(k, acc[q][i]);
    }
  };
  // the four waves' sums meet one kind at a time: two slots of NH + 1 float64 are all that lies over the transform buffers
#pragma unroll
  for (int q = 0; q < 4; ++q) welch_handoff(reinterpret_cast<double*>(smem), NH + 1, wave, [&](auto f) { kind(q, f); });
  if (wave != 0) return;
  if (w.part) {
    double* o = w.part + (g.row * w.max_chunks + g.chunk) * (int64_t)(4 * (NH + 1));
#pragma unroll
    for (int q = 0; q < 4; ++q) kind(q, [&](int k, double& sum) { o[q * (NH + 1) + k] = sum; });
  } else {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = lane + 64 * i;
      if (k <= NH) mcsd_finish_bin(p, g.row, k, NH, acc[0][i], acc[1][i], acc[2][i], acc[3][i], g.K);
    }
  }
}

// ceil(bins / 256) workgroups per pair: a thread per bin adds the pair's chunk sums in ascending order
static __global__ __launch_bounds__(256) void modcsd_finish_kernel(ModcsdArgs p, int nh) {
  const WelchFinish f = welch_finish_plan(p.w, nh);
  if (f.state == WELCH_IDLE) return;
  if (f.state == WELCH_NAN) { mcsd_nan_bin(p, f.row, f.k); return; }
  const int64_t bins = nh + 1;
  const double* q = p.w.part + f.row * p.w.max_chunks * (4 * bins) + f.k;
  double s[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) s[a] = welch_chunk_sum(q + a * bins, f.chunks, 4 * bins);
  mcsd_finish_bin(p, f.row, f.k, nh, s[0], s[1], s[2], s[3], f.K);
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
  return h && mm_modcsd_check(&h->p) == MM_OK ? welch_workspace_bytes(h, rows, n_max, 4) : 0;
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
  const WelchLaunch l = welch_launch_plan(h, rows, n_max, nh + 1, 4, d_lens, d_ws, ws_bytes);
  if (l.rc != MM_OK) return l.rc;
  const ModcsdArgs a = {welch_args(h, d_lens, n_max, l.chunks, d_ws), d_x, d_y, d_pxx, d_pyy, d_pxy, d_coh,
                        x_stride, y_stride, y_group, out_stride};
  // LDS: the four transform buffers, 8 nfft bytes each (64 KiB at nfft 2048); the two hand-off slots of nfft / 2 + 1
  // float64 lie over them
  const size_t lds = (size_t)MPSD_WAVES * h->p.nfft * sizeof(float2);
  return welch_launch(mcsd_kernel_of(h->log2n), modcsd_finish_kernel, a, l, rows, nh + 1, lds, stream);
}

}  // extern "C"
