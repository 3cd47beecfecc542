// What the two Welch units share (mm_modpsd.hip: include/modmfcc_modpsd.h; mm_modcsd.hip: include/modmfcc_modcsd.h): the
// handle and everything "a row's bits never depend on the batch" rests on, once.  Device: WelchArgs, welch_plan (workgroup
// -> row, chunk, segments), the detrend constants, mean, slope and subtraction, welch_handoff ((w0 + w1) + (w2 + w3)),
// welch_finish_plan and welch_chunk_sum.  Host: welch_workspace_bytes, welch_launch_plan (the shared refusals and the
// grids), welch_args, welch_launch.  Included by both units and, through them, twice by the single-translation-unit build.
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

// the kernel arguments of either unit; each keeps its own pointers and strides beside them
struct WelchArgs {
  const int64_t* lens;
  const float* window;
  const float2* tw;
  double* part;          // [rows][max_chunks][sums per bin][bins] chunk sums, or nullptr: one chunk per row, finished directly
  int64_t n_max, max_chunks;
  double scale;
  int nperseg, step, noverlap, detrend;
};

// segments of a row: its length clamped into [1, n_max]; 0 for a row shorter than nperseg
__device__ __forceinline__ int64_t welch_segments(const WelchArgs& w, int64_t row) {
  const int64_t l = w.lens ? w.lens[row] : w.n_max, len = l < 1 ? 1 : (l > w.n_max ? w.n_max : l);
  return len < w.nperseg ? 0 : (len - w.noverlap) / w.step;
}

__device__ __forceinline__ double mpsd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// no segment (a NaN row) / a chunk beyond the row's last, or a thread beyond the last bin / work
enum WelchState { WELCH_NAN, WELCH_IDLE, WELCH_WORK };

// Workgroup `block` of the main kernels takes segments seg0 .. seg0 + n_seg of `row`; wave v of it the segments seg0 + v,
// seg0 + v + MPSD_WAVES, ... in ascending order.  (Workgroup-uniform.)
struct WelchPlan { WelchState state; int64_t row, chunk, K, seg0; int n_seg; };

__device__ __forceinline__ WelchPlan welch_plan(const WelchArgs& w, unsigned block) {
  WelchPlan g;
  g.row = block / w.max_chunks; g.chunk = block % w.max_chunks;
  g.K = welch_segments(w, g.row);
  g.seg0 = g.chunk * MM_MODPSD_CHUNK;
  g.n_seg = (int)(g.K - g.seg0 < MM_MODPSD_CHUNK ? g.K - g.seg0 : MM_MODPSD_CHUNK);
  g.state = g.K == 0 ? WELCH_NAN : g.seg0 >= g.K ? WELCH_IDLE : WELCH_WORK;
  return g;
}

// The detrend of a segment x[0 .. nperseg): the centre of j and sxx = sum (j - centre)^2 = n (n^2 - 1) / 12; mean and slope
// from the lanes' shares of s0 = sum x[j] and s1 = sum (j - centre) x[j], which each kernel adds up in its own order;
// sample j without its trend.
struct WelchDetrend { double centre, sxx; };
struct WelchTrend { double mean, slope; };

__device__ __forceinline__ WelchDetrend welch_detrend(int nperseg) {
  return {0.5 * (double)(nperseg - 1), (double)nperseg * ((double)nperseg * (double)nperseg - 1.0) / 12.0};
}

// (two functions, not one per side: the cross kernel starts the wave sums and divisions of both sides' means together,
// ahead of the slopes' branch -- with a side's mean and slope in one call its calls cost 0.7 %: docs/experiments.md)
__device__ __forceinline__ double welch_mean(double s0, const WelchArgs& w) { return mpsd_wave_sum(s0) / (double)w.nperseg; }

__device__ __forceinline__ double welch_slope(double s1, const WelchArgs& w, const WelchDetrend& d) {
  return w.detrend == 2 && w.nperseg > 1 ? mpsd_wave_sum(s1) / d.sxx : 0.0;
}

__device__ __forceinline__ float welch_subtract(float v, int j, const WelchTrend& t, const WelchDetrend& d) {
  return (float)((double)v - (t.mean + t.slope * ((double)j - d.centre)));
}

// (w0 + w1) + (w2 + w3) of the four waves' float64 accumulators through two slots of `bins` float64 at `ex`: the odd waves
// hand theirs to the even ones, then wave 2 to wave 0.  `walk(f)` calls f(k, a) for every bin k and accumulator a (a
// register: the walk unrolls) of the calling lane.  The slots lie over the transform buffers of other waves: a barrier
// in front of each hand-off.
template <class Walk>
__device__ __forceinline__ void welch_handoff(double* ex, int bins, int wave, Walk walk) {
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const bool gives = round == 0 ? (wave & 1) : wave == 2;
    const bool takes = round == 0 ? !(wave & 1) : wave == 0;
    double* slot = ex + (size_t)(round == 0 ? (wave >> 1) : 0) * bins;
    __syncthreads();
    if (gives) walk([slot](int k, double& a) { slot[k] = a; });
    __syncthreads();
    if (takes) walk([slot](int k, double& a) { a += slot[k]; });
  }
}

// Thread -> (bin k, row) of the finish kernels: ceil(bins / 256) workgroups of 256 threads per row; nc is the last bin
struct WelchFinish { WelchState state; int k; int64_t row, K, chunks; };

__device__ __forceinline__ WelchFinish welch_finish_plan(const WelchArgs& w, int nc) {
  const int per_row = (nc + 1 + 255) / 256;
  WelchFinish f = {WELCH_IDLE, (int)(blockIdx.x % per_row) * 256 + (int)threadIdx.x, 0, 0, 0};
  if (f.k > nc) return f;
  f.row = blockIdx.x / per_row;
  f.K = welch_segments(w, f.row);
  f.chunks = (f.K + MM_MODPSD_CHUNK - 1) / MM_MODPSD_CHUNK;
  f.state = f.K == 0 ? WELCH_NAN : WELCH_WORK;
  return f;
}

// q[0] + q[stride] + ... over a row's chunks, ascending
__device__ __forceinline__ double welch_chunk_sum(const double* q, int64_t chunks, int64_t stride) {
  double sum = q[0];
  for (int64_t c = 1; c < chunks; ++c) sum += q[c * stride];
  return sum;
}

static int64_t mpsd_host_segments(const mm_modpsd_params& p, int64_t n) {
  return n < p.nperseg ? 0 : (n - p.noverlap) / (p.nperseg - p.noverlap);
}

static int64_t mpsd_max_chunks(const mm_modpsd* h, int64_t n_max) {
  const int64_t K = mpsd_host_segments(h->p, n_max);
  return K < 1 ? 1 : (K + MM_MODPSD_CHUNK - 1) / MM_MODPSD_CHUNK;
}

// bytes of the chunk sums (sums_per_bin float64 per bin); 0 where every row has one chunk
static size_t welch_workspace_bytes(const mm_modpsd* h, int64_t rows, int64_t n_max, int sums_per_bin) {
  if (!h || rows < 1 || n_max < 1) return 0;
  const int64_t chunks = mpsd_max_chunks(h, n_max);
  return chunks <= 1 ? 0 : (size_t)rows * (size_t)chunks * sums_per_bin * (size_t)(h->p.nfft / 2 + 1) * sizeof(double);
}

// what a compute entry refuses after its own arguments, in this order, and the grids of its launches
struct WelchLaunch { int rc; int64_t chunks, finish_per_row; };

static WelchLaunch welch_launch_plan(const mm_modpsd* h, int64_t rows, int64_t n_max, int bins, int sums_per_bin,
                                     const int64_t* d_lens, const void* d_ws, size_t ws_bytes) {
  WelchLaunch l = {MM_OK, mpsd_max_chunks(h, n_max), (bins + 255) / 256};
  const size_t need = welch_workspace_bytes(h, rows, n_max, sums_per_bin);
  if (!d_lens && n_max < h->p.nperseg) l.rc = MM_ERR_INVALID_ARG;
  else if (need && (!d_ws || ((uintptr_t)d_ws & 7))) l.rc = MM_ERR_INVALID_ARG;
  else if (ws_bytes < need) l.rc = MM_ERR_WORKSPACE;
  else if (rows > 0x7FFFFFFF / l.chunks || rows > 0x7FFFFFFF / l.finish_per_row) l.rc = MM_ERR_UNSUPPORTED;
  return l;
}

static WelchArgs welch_args(const mm_modpsd* h, const int64_t* d_lens, int64_t n_max, int64_t chunks, void* d_ws) {
  const mm_modpsd_params& p = h->p;
  return {d_lens, h->d_window, h->d_tw, chunks > 1 ? (double*)d_ws : nullptr, n_max, chunks, h->scale,
          p.nperseg, p.nperseg - p.noverlap, p.noverlap, p.detrend};
}

// the main kernel on a workgroup per (row, chunk) with `lds` bytes, then -- more than one chunk -- the finish kernel
template <class Args>
static int welch_launch(void (*kernel)(Args), void (*finish)(Args, int), const Args& a, const WelchLaunch& l, int64_t rows,
                        int bins, size_t lds, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(rows * l.chunks)), dim3(64 * MPSD_WAVES), lds, st, a);
  if (l.chunks > 1)
    hipLaunchKernelGGL(finish, dim3((unsigned)(rows * l.finish_per_row)), dim3(256), 0, st, a, bins - 1);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

#endif
