// What the two Welch units share (mm_modpsd.hip: include/modmfcc_modpsd.h; mm_modcsd.hip: include/modmfcc_modcsd.h): the
// handle, a row's length and segment count, the float64 wave sum of the detrend statistics, the host-side chunk count.
// Included by both units and, through them, twice by the single-translation-unit build: guarded.
#ifndef MM_WELCH_HIP_INC
#define MM_WELCH_HIP_INC

#define MPSD_WAVES 4

struct mm_modpsd {
  mm_modpsd_params p;
  int device;
  int log2n;
  double scale;          // 1 / (fs sum w^2) or 1 / (sum w)^2
  float* d_window;       // [nfft], zeros behind nperseg
  float2* d_tw;          // [MM_TW_N] exp(-2 pi i k / MM_TW_N)
};

__device__ __forceinline__ int64_t mpsd_row_len(const int64_t* lens, int64_t row, int64_t n_max) {
  if (!lens) return n_max;
  const int64_t l = lens[row];
  return l < 1 ? 1 : (l > n_max ? n_max : l);
}

__device__ __forceinline__ int64_t mpsd_segments(int64_t len, int nperseg, int noverlap, int step) {
  return len < nperseg ? 0 : (len - noverlap) / step;
}

__device__ __forceinline__ double mpsd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static int64_t mpsd_host_segments(const mm_modpsd_params& p, int64_t n) {
  return n < p.nperseg ? 0 : (n - p.noverlap) / (p.nperseg - p.noverlap);
}

static int64_t mpsd_max_chunks(const mm_modpsd* h, int64_t n_max) {
  const int64_t K = mpsd_host_segments(h->p, n_max);
  return K < 1 ? 1 : (K + MM_MODPSD_CHUNK - 1) / MM_MODPSD_CHUNK;
}

#endif
