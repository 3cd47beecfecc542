// Welch modulation power spectrum (include/modmfcc_modpsd.h): scipy.signal.welch along float32 rows, a length per row.
//
//   modpsd_kernel<LOG2N>   one workgroup (4 waves) per (row, chunk of MM_MODPSD_CHUNK = 32 segments).  Segment i of a row
//                          belongs to chunk i / 32 and, inside it, to wave i % 4, which takes its segments in ascending
//                          order.  A wave reads its segment for the detrend statistics (float64 sums over the wave) and again,
//                          from the cache, to subtract the trend in float64, writes the windowed values bit-reversed into
//                          its LDS buffer, transforms them there (the packed real transform of rfft_generic_kernel:
//                          wave_cfft_lds + real_split of mm_common.h) and adds |X[k]|^2 to float64 accumulators its lanes
//                          hold for their bins.  The four waves' sums meet through LDS as (w0 + w1) + (w2 + w3).  A batch
//                          whose rows have one chunk each ends here: scale, round, store.  Otherwise every chunk stores
//                          its float64 sums to the workspace and
//   modpsd_finish_kernel   adds a row's chunks in ascending order, scales, rounds and stores.
//
// Which wave adds which segment in which order is a function of the segment's index alone, and the chunk sums are added in
// ascending order whichever kernel does it (one chunk: the sum is that chunk's): a row's bits do not depend on rows, n_max
// or the other rows.  No atomics.  A row without a segment (shorter than nperseg) is NaN.  That plan (welch_plan), the
// trend, the hand-off (welch_handoff) and the chunk sum are mm_welch.hip.inc's, one copy for this unit and mm_modcsd.hip;
// the order in which a lane adds up its samples and squares its bins is this kernel's own.
#include "mm_common.h"
#include "../../include/modmfcc_modpsd.h"
#include "mm_welch.hip.inc"   // shared with mm_modcsd.hip: handle, workgroup plan, detrend, hand-off, chunk sum, launch

#define MPSD_MIN_LOG2N 5
#define MPSD_MAX_LOG2N 12

struct ModpsdArgs {
  WelchArgs w;           // part: [rows][max_chunks][bins]
  const float* x;
  float* psd;
  int64_t x_stride, psd_stride;
};

// P[k] of a row from the float64 sum over its K segments
__device__ __forceinline__ float mpsd_value(double sum, int k, int nc, double scale, int64_t K) {
  const double d = (k == 0 || k == nc) ? 1.0 : 2.0;
  return (float)(sum * (scale * d / (double)K));
}

template <int LOG2N>
__global__ __launch_bounds__(64 * MPSD_WAVES) void modpsd_kernel(ModpsdArgs p) {
  constexpr int NC = 1 << (LOG2N - 1);                 // complex points of the packed transform; bins 0 .. NC
  constexpr int LOG2NC = LOG2N - 1;
  constexpr int NP = NC >= 64 ? NC / 64 : 1;           // sample pairs per lane
  constexpr int NA = NC / 128 + 1;                     // bin pairs (k, NC - k), k = lane + 64 i <= NC / 2, per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float2* z = reinterpret_cast<float2*>(smem) + (size_t)wave * NC;

  const WelchArgs& w = p.w;
  const WelchPlan g = welch_plan(w, blockIdx.x);
  float* out = p.psd + g.row * p.psd_stride;
  if (g.state == WELCH_NAN && !w.part && g.chunk == 0)
    for (int k = threadIdx.x; k <= NC; k += 64 * MPSD_WAVES) out[k] = __builtin_nanf("");
  if (g.state != WELCH_WORK) return;                   // (workgroup-uniform)
  const float* a = p.x + g.row * p.x_stride;
  const int tw_stride = MM_TW_N >> LOG2N;
  const WelchDetrend d = welch_detrend(w.nperseg);

  double accA[NA], accB[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) accA[i] = accB[i] = 0.0;

  for (int s = wave; s < g.n_seg; s += MPSD_WAVES) {   // (wave-uniform)
    const float* as = a + (g.seg0 + s) * (int64_t)w.step;  // samples as[0 .. nperseg): all below len
    // the segment is read once for the detrend statistics and once more (from the cache) to be transformed: held in
    // registers between the two, the 64 samples per lane of nfft 4096 would spill beside the accumulators
    WelchTrend t = {0.0, 0.0};
    if (w.detrend) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
      for (int i = 0; i < NP; ++i) {
        const int j = 2 * (lane + 64 * i);
        const double x0 = j < w.nperseg ? (double)as[j] : 0.0, x1 = j + 1 < w.nperseg ? (double)as[j + 1] : 0.0;
        s0 += x0 + x1;
        if (w.detrend == 2) s1 += ((double)j - d.centre) * x0 + ((double)(j + 1) - d.centre) * x1;
      }
      t = {welch_mean(s0, w), welch_slope(s1, w, d)};
    }
#pragma unroll 4
    for (int i = 0; i < NP; ++i) {
      const int n = lane + 64 * i, j = 2 * n;
      if (n < NC) {
        float y0 = j < w.nperseg ? as[j] : 0.0f, y1 = j + 1 < w.nperseg ? as[j + 1] : 0.0f;
        if (w.detrend) {
          y0 = j < w.nperseg ? welch_subtract(y0, j, t, d) : 0.0f;
          y1 = j + 1 < w.nperseg ? welch_subtract(y1, j + 1, t, d) : 0.0f;
        }
        z[__brev((unsigned)n) >> (32 - LOG2NC)] = make_float2(y0 * w.window[j], y1 * w.window[j + 1]);
      }
    }
    wave_lds_sync();
    wave_cfft_lds(z, LOG2NC, w.tw, lane);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) {
        float2 xa, xb;
        real_split(z, k, NC, w.tw, tw_stride, xa, xb);
        accA[i] += (double)(xa.x * xa.x + xa.y * xa.y);
        accB[i] += (double)(xb.x * xb.x + xb.y * xb.y);
      }
    }
    wave_lds_sync();
  }

  // every (bin, accumulator) of this lane, in the order of the stores: k = NC - k = NC / 2 ends as accB's
  auto bins = [&](auto f) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) { f(k, accA[i]); f(NC - k, accB[i]); }
    }
  };
  welch_handoff(reinterpret_cast<double*>(smem), NC + 1, wave, bins);
  if (wave != 0) return;
  if (w.part) {
    double* o = w.part + (g.row * w.max_chunks + g.chunk) * (int64_t)(NC + 1);
    bins([o](int k, double& sum) { o[k] = sum; });
  } else {
    bins([&](int k, double& sum) { out[k] = mpsd_value(sum, k, NC, w.scale, g.K); });
  }
}

// ceil(bins / 256) workgroups per row: a thread per bin adds the row's chunk sums in ascending order
static __global__ __launch_bounds__(256) void modpsd_finish_kernel(ModpsdArgs p, int nc) {
  const WelchFinish f = welch_finish_plan(p.w, nc);
  if (f.state == WELCH_IDLE) return;
  float* out = p.psd + f.row * p.psd_stride;
  if (f.state == WELCH_NAN) { out[f.k] = __builtin_nanf(""); return; }
  const double* q = p.w.part + f.row * p.w.max_chunks * (int64_t)(nc + 1) + f.k;
  out[f.k] = mpsd_value(welch_chunk_sum(q, f.chunks, nc + 1), f.k, nc, p.w.scale, f.K);
}

using ModpsdKernel = void (*)(ModpsdArgs);
static ModpsdKernel mpsd_kernel_of(int log2n) {
  switch (log2n) {
    case 5: return modpsd_kernel<5>;
    case 6: return modpsd_kernel<6>;
    case 7: return modpsd_kernel<7>;
    case 8: return modpsd_kernel<8>;
    case 9: return modpsd_kernel<9>;
    case 10: return modpsd_kernel<10>;
    case 11: return modpsd_kernel<11>;
    case 12: return modpsd_kernel<12>;
  }
  return nullptr;
}

extern "C" {

int mm_modpsd_version(void) { return 1; }

int mm_modpsd_check(const mm_modpsd_params* p) {
  if (!p) return MM_ERR_INVALID_ARG;
  if (!(p->fs > 0.0) || !std::isfinite(p->fs)) return MM_ERR_INVALID_ARG;
  if (p->nperseg < 1 || p->noverlap < 0 || p->noverlap >= p->nperseg || p->nfft < p->nperseg) return MM_ERR_INVALID_ARG;
  if (p->detrend < 0 || p->detrend > 2 || p->scaling < 0 || p->scaling > 1) return MM_ERR_INVALID_ARG;
  if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return MM_ERR_INVALID_ARG;
  if (p->nfft < (1 << MPSD_MIN_LOG2N) || p->nfft > (1 << MPSD_MAX_LOG2N) || (p->nfft & (p->nfft - 1))) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

int64_t mm_modpsd_num_segments(const mm_modpsd_params* p, int64_t n) {
  const int rc = mm_modpsd_check(p);
  if (rc != MM_OK && rc != MM_ERR_UNSUPPORTED) return rc;     // (the count does not depend on nfft)
  return n < 0 ? MM_ERR_INVALID_ARG : mpsd_host_segments(*p, n);
}

void mm_modpsd_destroy(mm_modpsd* h) {
  if (!h) return;
  if (h->d_window) (void)hipFree(h->d_window);
  if (h->d_tw) (void)hipFree(h->d_tw);
  delete h;
}

int mm_modpsd_create(const mm_modpsd_params* p, const float* window_host, mm_modpsd** out) {
  if (!out) return MM_ERR_INVALID_ARG;
  *out = nullptr;
  const int rc = mm_modpsd_check(p);
  if (rc != MM_OK) return rc;
  if (!window_host) return MM_ERR_INVALID_ARG;
  double sw = 0.0, sww = 0.0;
  for (int j = 0; j < p->nperseg; ++j) {
    if (!std::isfinite(window_host[j])) return MM_ERR_INVALID_ARG;
    sw += (double)window_host[j];
    sww += (double)window_host[j] * (double)window_host[j];
  }
  if (sww == 0.0 || (p->scaling == 1 && sw == 0.0)) return MM_ERR_INVALID_ARG;
  mm_modpsd* h = new (std::nothrow) mm_modpsd();
  if (!h) return MM_ERR_ALLOC;
  h->p = *p;
  h->log2n = ilog2(p->nfft);
  h->scale = p->scaling == 1 ? 1.0 / (sw * sw) : 1.0 / (p->fs * sww);
  h->d_window = nullptr;
  h->d_tw = nullptr;
  auto fail = [&](int code) { mm_modpsd_destroy(h); return code; };
  if (hipGetDevice(&h->device) != hipSuccess) { g_hip_err = "hipGetDevice failed"; return fail(MM_ERR_HIP); }
  std::vector<float> win((size_t)p->nfft, 0.0f), tw((size_t)2 * MM_TW_N);
  std::copy(window_host, window_host + p->nperseg, win.begin());
  mm::build_twiddles(MM_TW_N, tw.data());
  if (hipMalloc(&h->d_window, win.size() * sizeof(float)) != hipSuccess || hipMalloc(&h->d_tw, tw.size() * sizeof(float)) != hipSuccess)
    return fail(MM_ERR_ALLOC);
  if (hipMemcpy(h->d_window, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    g_hip_err = "hipMemcpy of the modpsd tables failed";
    return fail(MM_ERR_HIP);
  }
  *out = h;
  return MM_OK;
}

size_t mm_modpsd_workspace_bytes(const mm_modpsd* h, int64_t rows, int64_t n_max) {
  return welch_workspace_bytes(h, rows, n_max, 1);
}

int mm_modpsd_f32(const mm_modpsd* h, const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                  float* d_psd, int64_t psd_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_x || !d_psd || rows < 1 || n_max < 1 || x_stride < n_max) return MM_ERR_INVALID_ARG;
  const int nc = h->p.nfft / 2;
  if (psd_stride < nc + 1) return MM_ERR_INVALID_ARG;
  const WelchLaunch l = welch_launch_plan(h, rows, n_max, nc + 1, 1, d_lens, d_ws, ws_bytes);
  if (l.rc != MM_OK) return l.rc;
  const ModpsdArgs a = {welch_args(h, d_lens, n_max, l.chunks, d_ws), d_x, d_psd, x_stride, psd_stride};
  // LDS: the four transform buffers, 8 nc bytes each (64 KiB at nfft 4096); the two hand-off buffers of (nc + 1) float64
  // lie over them
  const size_t lds = std::max((size_t)MPSD_WAVES * nc * sizeof(float2), (size_t)2 * (nc + 1) * sizeof(double));
  return welch_launch(mpsd_kernel_of(h->log2n), modpsd_finish_kernel, a, l, rows, nc + 1, lds, stream);
}

}  // extern "C"
