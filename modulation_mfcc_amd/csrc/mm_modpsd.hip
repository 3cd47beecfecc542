// Welch modulation power spectrum (include/modmfcc_modpsd.h): scipy.signal.welch along float32 rows, a length per row.
//
//   modpsd_kernel<LOG2N>   one workgroup (4 waves) per (row, chunk of MM_MODPSD_CHUNK = 32 segments).  Segment i of a row
//                          belongs to chunk i / 32 and, inside it, to wave i % 4, which takes its segments in ascending
//                          order.  A wave reads its segment for the detrend statistics (float64 sums over the wave) and again,
//                          from the cache, to subtract the trend in float64, writes the windowed values bit-reversed into
//                          its LDS buffer,
//                          transforms them there (the packed real transform of rfft_generic_kernel: wave_cfft_lds +
//                          real_split of mm_common.h) and adds |X[k]|^2 to float64 accumulators its lanes hold for their
//                          bins.  The four waves' sums meet through LDS as (w0 + w1) + (w2 + w3).  A batch whose rows
//                          have one chunk each ends here: scale, round, store.  Otherwise every chunk stores its float64
//                          sums to the workspace and
//   modpsd_finish_kernel   adds a row's chunks in ascending order, scales, rounds and stores.
//
// Which wave adds which segment in which order is a function of the segment's index alone, and the chunk sums are added in
// ascending order whichever kernel does it (one chunk: the sum is that chunk's): a row's bits do not depend on rows, n_max
// or the other rows.  No atomics.  A row without a segment (shorter than nperseg) is NaN.
#include "mm_common.h"
#include "../../include/modmfcc_modpsd.h"
#include "mm_welch.hip.inc"   // the handle, row length, segment count, wave sum, chunk count: shared with mm_modcsd.hip

#define MPSD_MIN_LOG2N 5
#define MPSD_MAX_LOG2N 12

struct ModpsdArgs {
  const float* x;
  const int64_t* lens;
  const float* window;
  const float2* tw;
  float* psd;
  double* part;          // [rows][max_chunks][bins] chunk sums, or nullptr: one chunk per row, stored directly
  int64_t n_max, x_stride, psd_stride, max_chunks;
  double scale;
  int nperseg, step, noverlap, detrend;
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

  const int64_t row = blockIdx.x / p.max_chunks, chunk = blockIdx.x % p.max_chunks;
  const int64_t len = mpsd_row_len(p.lens, row, p.n_max);
  const int64_t K = mpsd_segments(len, p.nperseg, p.noverlap, p.step);
  const int64_t seg0 = chunk * MM_MODPSD_CHUNK;
  float* out = p.psd + row * p.psd_stride;
  if (K == 0) {                                        // (workgroup-uniform)
    if (!p.part && chunk == 0)
      for (int k = threadIdx.x; k <= NC; k += 64 * MPSD_WAVES) out[k] = __builtin_nanf("");
    return;
  }
  if (seg0 >= K) return;                               // (workgroup-uniform)
  const int n_seg = (int)(K - seg0 < MM_MODPSD_CHUNK ? K - seg0 : MM_MODPSD_CHUNK);
  const float* a = p.x + row * p.x_stride;
  const int tw_stride = MM_TW_N >> LOG2N;
  const double centre = 0.5 * (double)(p.nperseg - 1);
  // sum (j - centre)^2 = n (n^2 - 1) / 12
  const double sxx = (double)p.nperseg * ((double)p.nperseg * (double)p.nperseg - 1.0) / 12.0;

  double accA[NA], accB[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) accA[i] = accB[i] = 0.0;

  for (int s = wave; s < n_seg; s += MPSD_WAVES) {     // (wave-uniform)
    const float* as = a + (seg0 + s) * (int64_t)p.step;  // samples as[0 .. nperseg): all below len
    // the segment is read once for the detrend statistics and once more (from the cache) to be transformed: held in
    // registers between the two, the 64 samples per lane of nfft 4096 would spill beside the accumulators
    double mean = 0.0, slope = 0.0;
    if (p.detrend) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
      for (int i = 0; i < NP; ++i) {
        const int j = 2 * (lane + 64 * i);
        const double x0 = j < p.nperseg ? (double)as[j] : 0.0, x1 = j + 1 < p.nperseg ? (double)as[j + 1] : 0.0;
        s0 += x0 + x1;
        if (p.detrend == 2) s1 += ((double)j - centre) * x0 + ((double)(j + 1) - centre) * x1;
      }
      mean = mpsd_wave_sum(s0) / (double)p.nperseg;
      if (p.detrend == 2 && p.nperseg > 1) slope = mpsd_wave_sum(s1) / sxx;
    }
#pragma unroll 4
    for (int i = 0; i < NP; ++i) {
      const int n = lane + 64 * i, j = 2 * n;
      if (n < NC) {
        float y0 = j < p.nperseg ? as[j] : 0.0f, y1 = j + 1 < p.nperseg ? as[j + 1] : 0.0f;
        if (p.detrend) {
          y0 = j < p.nperseg ? (float)((double)y0 - (mean + slope * ((double)j - centre))) : 0.0f;
          y1 = j + 1 < p.nperseg ? (float)((double)y1 - (mean + slope * ((double)(j + 1) - centre))) : 0.0f;
        }
        z[__brev((unsigned)n) >> (32 - LOG2NC)] = make_float2(y0 * p.window[j], y1 * p.window[j + 1]);
      }
    }
    wave_lds_sync();
    wave_cfft_lds(z, LOG2NC, p.tw, lane);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) {
        float2 xa, xb;
        real_split(z, k, NC, p.tw, tw_stride, xa, xb);
        accA[i] += (double)(xa.x * xa.x + xa.y * xa.y);
        accB[i] += (double)(xb.x * xb.x + xb.y * xb.y);
      }
    }
    wave_lds_sync();
  }

  // (w0 + w1) + (w2 + w3) through LDS: the odd waves hand theirs to the even ones, then wave 2 to wave 0.  The buffers
  // lie over the transform buffers of other waves: a barrier in front of each hand-off.
  double* ex = reinterpret_cast<double*>(smem);
  for (int round = 0; round < 2; ++round) {
    const bool gives = round == 0 ? (wave & 1) : wave == 2;
    const bool takes = round == 0 ? !(wave & 1) : wave == 0;
    double* slot = ex + (size_t)(round == 0 ? (wave >> 1) : 0) * (NC + 1);
    __syncthreads();
    if (gives) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int k = lane + 64 * i;
        if (k <= NC / 2) { slot[k] = accA[i]; slot[NC - k] = accB[i]; }
      }
    }
    __syncthreads();
    if (takes) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int k = lane + 64 * i;
        if (k <= NC / 2) { accA[i] += slot[k]; accB[i] += slot[NC - k]; }
      }
    }
  }
  if (wave != 0) return;
  if (p.part) {
    double* o = p.part + (row * p.max_chunks + chunk) * (int64_t)(NC + 1);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) { o[k] = accA[i]; o[NC - k] = accB[i]; }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int k = lane + 64 * i;
      if (k <= NC / 2) {
        out[k] = mpsd_value(accA[i], k, NC, p.scale, K);
        out[NC - k] = mpsd_value(accB[i], NC - k, NC, p.scale, K);
      }
    }
  }
}

// ceil(bins / 256) workgroups per row: a thread per bin adds the row's chunk sums in ascending order
static __global__ __launch_bounds__(256) void modpsd_finish_kernel(ModpsdArgs p, int nc) {
  const int per_row = (nc + 1 + 255) / 256;
  const int k = (int)(blockIdx.x % per_row) * 256 + threadIdx.x;
  if (k > nc) return;
  const int64_t row = blockIdx.x / per_row;
  const int64_t K = mpsd_segments(mpsd_row_len(p.lens, row, p.n_max), p.nperseg, p.noverlap, p.step);
  float* out = p.psd + row * p.psd_stride;
  if (K == 0) { out[k] = __builtin_nanf(""); return; }
  const int64_t chunks = (K + MM_MODPSD_CHUNK - 1) / MM_MODPSD_CHUNK;
  const double* q = p.part + row * p.max_chunks * (int64_t)(nc + 1) + k;
  double sum = q[0];
  for (int64_t c = 1; c < chunks; ++c) sum += q[c * (int64_t)(nc + 1)];
  out[k] = mpsd_value(sum, k, nc, p.scale, K);
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
  if (!h || rows < 1 || n_max < 1) return 0;
  const int64_t chunks = mpsd_max_chunks(h, n_max);
  if (chunks <= 1) return 0;
  return (size_t)rows * (size_t)chunks * (size_t)(h->p.nfft / 2 + 1) * sizeof(double);
}

int mm_modpsd_f32(const mm_modpsd* h, const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                  float* d_psd, int64_t psd_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_x || !d_psd || rows < 1 || n_max < 1 || x_stride < n_max) return MM_ERR_INVALID_ARG;
  const int nc = h->p.nfft / 2;
  if (psd_stride < nc + 1) return MM_ERR_INVALID_ARG;
  if (!d_lens && n_max < h->p.nperseg) return MM_ERR_INVALID_ARG;
  const int64_t chunks = mpsd_max_chunks(h, n_max);
  const size_t need = mm_modpsd_workspace_bytes(h, rows, n_max);
  if (need && (!d_ws || ((uintptr_t)d_ws & 7))) return MM_ERR_INVALID_ARG;
  if (ws_bytes < need) return MM_ERR_WORKSPACE;
  const int64_t finish_per_row = (nc + 1 + 255) / 256;
  if (rows > 0x7FFFFFFF / chunks || rows > 0x7FFFFFFF / finish_per_row) return MM_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  ModpsdArgs a;
  a.x = d_x; a.lens = d_lens; a.window = h->d_window; a.tw = h->d_tw; a.psd = d_psd;
  a.part = chunks > 1 ? (double*)d_ws : nullptr;
  a.n_max = n_max; a.x_stride = x_stride; a.psd_stride = psd_stride; a.max_chunks = chunks;
  a.scale = h->scale;
  a.nperseg = h->p.nperseg; a.step = h->p.nperseg - h->p.noverlap; a.noverlap = h->p.noverlap; a.detrend = h->p.detrend;
  // LDS: the four transform buffers, 8 nc bytes each (64 KiB at nfft 4096); the two hand-off buffers of (nc + 1) float64
  // lie over them
  const size_t lds = std::max((size_t)MPSD_WAVES * nc * sizeof(float2), (size_t)2 * (nc + 1) * sizeof(double));
  hipLaunchKernelGGL(mpsd_kernel_of(h->log2n), dim3((unsigned)(rows * chunks)), dim3(64 * MPSD_WAVES), lds, st, a);
  if (chunks > 1)
    hipLaunchKernelGGL(modpsd_finish_kernel, dim3((unsigned)(rows * finish_per_row)), dim3(256), 0, st, a, nc);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
