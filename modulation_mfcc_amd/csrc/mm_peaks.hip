// libmodmfcc: peak / trough detection on batches of curves -- scipy.signal.find_peaks(y) / find_peaks(-y) as the
// reference's MinMaxFinder calls it (script/calc.py:651-686, script/main.py:1546-1613), with the height, threshold and
// prominence (wlen=None) conditions.  gfx950 only.  The kernels ("Peaks"):
//   pk_count_kernel   rising edges of a segment that resolve to a peak and pass height / threshold -> count per segment
//   pk_scan_kernel    exclusive scan of a row's segment counts; the row's total; -1 fill of the unused index slots
//   pk_write_kernel   the same test again, plateau midpoints written at scan offset + rank (ballot / popcount)
//   pk_prom_kernel    one wave per candidate: prominence and bases, 64 samples a step
//   pk_ccount_kernel / pk_cwrite_kernel   the candidates the prominence interval keeps, compacted the same way
// Every comparison is a plain IEEE one (NaN compares false, as in scipy's Cython loops); values are float64 throughout
// (float32 input is promoted per element, exactly), so indices, bases and prominences equal scipy's bit for bit.
#include "mm_common.h"

namespace {

constexpr int kPkThreads = 256;
constexpr int kPkWaves = kPkThreads / 64;
constexpr int kPkPer = 4;                               // samples per thread, strided by the workgroup
constexpr int kPkSeg = kPkThreads * kPkPer;             // samples (or candidates) per segment = workgroup
constexpr int kPkPromWaves = 4;
constexpr unsigned kPkMaxGridY = 65535;
constexpr unsigned kPkPromMaxGridX = 4096;

__device__ __forceinline__ uint64_t pk_lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

struct PkArgs {
  const void* x;
  int64_t x_stride;
  const int32_t* lo;        // nullable
  const int32_t* hi;        // nullable
  int32_t n, nseg;
  int32_t row0;             // first row of this launch (rows beyond the grid's y limit take further launches)
  int32_t negate, use_height, use_threshold;
  double hmin, hmax, tmin, tmax;
};

// one row's samples as scipy sees them: float64, negated for troughs, restricted to [lo, hi)
template <class T>
struct PkRow {
  const T* p;
  int32_t lo, hi;
  bool neg;
  __device__ __forceinline__ PkRow(const PkArgs& a, int64_t row) {
    p = (const T*)a.x + row * a.x_stride;
    int32_t l = a.lo ? a.lo[row] : 0, h = a.hi ? a.hi[row] : a.n;
    l = min(max(l, 0), a.n);
    h = min(max(h, l), a.n);
    lo = l; hi = h; neg = a.negate != 0;
  }
  __device__ __forceinline__ double at(int32_t i) const {
    const double v = (double)p[i];
    return neg ? -v : v;
  }
};

// An open side (the +-inf the host passes for None) is not tested at all, as scipy skips it.
__device__ __forceinline__ bool pk_in(double v, double vmin, double vmax) {
  return (vmin == -INFINITY || vmin <= v) && (vmax == INFINITY || v <= vmax);
}

// scipy's _local_maxima_1d at sample i (absolute; lo < i < hi - 1): -1, or the plateau midpoint when i is the rising edge
// of a plateau whose first different sample is lower.  Then height and threshold, scipy's order and arithmetic.
template <class T>
__device__ __forceinline__ int32_t pk_peak_at(const PkArgs& a, const PkRow<T>& r, int32_t i) {
  if (i <= r.lo || i >= r.hi - 1) return -1;
  const double v = r.at(i);
  if (!(r.at(i - 1) < v)) return -1;
  int32_t j = i + 1;
  const int32_t last = r.hi - 1;
  while (j < last && r.at(j) == v) ++j;            // the lane walks its plateau alone
  if (!(r.at(j) < v)) return -1;
  const int32_t mid = (int32_t)(((int64_t)i + (j - 1)) / 2);
  if (a.use_height && !pk_in(v, a.hmin, a.hmax)) return -1;
  if (a.use_threshold) {
    const double dl = v - r.at(mid - 1), dr = v - r.at(mid + 1);
    // np.min / np.max of the pair, NaN propagating as numpy's do (inf - inf beside an infinite plateau): a NaN then
    // fails every bound that is set, so scipy drops the peak unless both sides are open
    const bool un = dl != dl || dr != dr;
    const double dmin = un ? NAN : (dl < dr ? dl : dr), dmax = un ? NAN : (dl > dr ? dl : dr);
    if (!((a.tmin == -INFINITY || a.tmin <= dmin) && (a.tmax == INFINITY || dmax <= a.tmax))) return -1;
  }
  return mid - r.lo;
}

template <class T>
__global__ __launch_bounds__(kPkThreads) void pk_count_kernel(PkArgs a, int32_t* __restrict__ segcount) {
  __shared__ int s_w[kPkWaves];
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  int cnt = 0;                                       // wave-uniform
  if (base < r.hi && base + kPkSeg > r.lo) {
#pragma unroll
    for (int k = 0; k < kPkPer; ++k) {
      const int64_t i = base + k * kPkThreads + threadIdx.x;
      const bool pk = i < a.n && pk_peak_at<T>(a, r, (int32_t)i) >= 0;
      cnt += __popcll(__ballot(pk));
    }
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kPkWaves; ++w) t += s_w[w];
    segcount[row * a.nseg + blockIdx.x] = t;
  }
}

// exclusive prefix over the workgroup's 256 values (v of thread t -> sum of v of threads < t); total in *tot
__device__ __forceinline__ int pk_block_exscan(int v, int* s_w, int* tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < kPkWaves; ++q) {
    const int c = s_w[q];
    if (q < w) before += c;
    all += c;
  }
  *tot = all;
  return before + inc - v;
}

// A workgroup per row: segcount[row][0 .. nseg) becomes its exclusive prefix, total[row] the sum; idx[row][min(total,
// cap) .. cap) is filled with -1, as are the bases, the prominences with NaN (fill == nullptr: the candidate pass, whose
// consumers read only below the count).
__global__ __launch_bounds__(kPkThreads) void pk_scan_kernel(int32_t* __restrict__ segcount, int32_t nseg,
                                                             int32_t* __restrict__ total, int32_t* __restrict__ fill,
                                                             int32_t* __restrict__ fill_lb, int32_t* __restrict__ fill_rb,
                                                             double* __restrict__ fill_prom, int64_t cap) {
  __shared__ int s_w[kPkWaves];
  const int64_t row = blockIdx.x;
  int32_t* sc = segcount + row * nseg;
  const int32_t L = (nseg + kPkThreads - 1) / kPkThreads;
  const int32_t b = min(nseg, (int32_t)threadIdx.x * L), e = min(nseg, b + L);
  int sum = 0;
  for (int32_t s = b; s < e; ++s) sum += sc[s];
  int tot = 0;
  int run = pk_block_exscan(sum, s_w, &tot);
  for (int32_t s = b; s < e; ++s) {
    const int c = sc[s];
    sc[s] = run;
    run += c;
  }
  if (threadIdx.x == 0) total[row] = tot;
  if (fill) {
    for (int64_t k = min<int64_t>(tot, cap) + threadIdx.x; k < cap; k += kPkThreads) {
      fill[row * cap + k] = -1;
      if (fill_lb) { fill_lb[row * cap + k] = -1; fill_rb[row * cap + k] = -1; fill_prom[row * cap + k] = NAN; }
    }
  }
}

// rank of this thread's hit of round k among the segment's hits: rounds, then waves, then lanes -- ascending samples
__device__ __forceinline__ int pk_rank(const uint64_t (&m)[kPkPer], int k, int (*s_c)[kPkWaves]) {
  const int w = threadIdx.x >> 6;
  int before = 0;
#pragma unroll
  for (int kk = 0; kk < kPkPer; ++kk)
#pragma unroll
    for (int q = 0; q < kPkWaves; ++q)
      if (kk < k || (kk == k && q < w)) before += s_c[kk][q];
  return before + __popcll(m[k] & pk_lanemask_lt());
}

template <class T>
__global__ __launch_bounds__(kPkThreads) void pk_write_kernel(PkArgs a, const int32_t* __restrict__ segoff,
                                                              int32_t* __restrict__ idx, int64_t cap) {
  __shared__ int s_c[kPkPer][kPkWaves];
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  if (!(base < r.hi && base + kPkSeg > r.lo)) return;          // (workgroup-uniform)
  int32_t mid[kPkPer];
  uint64_t m[kPkPer];
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    const int64_t i = base + k * kPkThreads + threadIdx.x;
    mid[k] = i < a.n ? pk_peak_at<T>(a, r, (int32_t)i) : -1;
    m[k] = __ballot(mid[k] >= 0);
    if ((threadIdx.x & 63) == 0) s_c[k][threadIdx.x >> 6] = __popcll(m[k]);
  }
  __syncthreads();
  const int64_t off = segoff[row * a.nseg + blockIdx.x];
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    if (mid[k] >= 0) {
      const int64_t pos = off + pk_rank(m, k, s_c);
      if (pos < cap) idx[row * cap + pos] = mid[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// prominence (scipy's _peak_prominences, wlen=None): a wave per candidate.  Each step looks at the next 64 samples away
// from the peak; the first lane whose sample is above the peak, NaN or outside the row ends the scan (ballot), the lanes
// before it take part in a (value, distance) min-reduction in which an equal value nearer the peak wins; a step's
// minimum replaces the running one only when strictly lower -- together scipy's "first reached with <".
// ---------------------------------------------------------------------------------------------------------------------
struct PkPromArgs {
  const int32_t* ccount;    // [rows] candidates per row
  const int32_t* cidx;      // [rows][ccap] ascending, relative to lo
  double* cprom;            // [rows][ccap]
  int32_t* clb;             // [rows][ccap]; -1 where the prominence interval drops the candidate
  int32_t* crb;
  int64_t ccap;
  double pmin, pmax;
};

template <class T, int DIR>
__device__ __forceinline__ void pk_scan_side(const PkRow<T>& r, int32_t p, double vp, double& best, int32_t& base) {
  const int lane = threadIdx.x & 63;
  best = vp; base = p;
  for (int64_t step = 0;; step += 64) {
    const int64_t i = (int64_t)p + DIR * (step + 1 + lane);
    const bool inside = DIR < 0 ? i >= r.lo : i < r.hi;
    const double v = inside ? r.at((int32_t)i) : 0.0;
    const bool stop = !inside || !(v <= vp);
    const uint64_t sm = __ballot(stop);
    const int first = sm ? __ffsll((unsigned long long)sm) - 1 : 64;
    double bv = lane < first ? v : INFINITY;
    int bl = lane < first ? lane : 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const int ol = __shfl_xor(bl, o, 64);
      if (ov < bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
    }
    if (bl < 64 && bv < best) { best = bv; base = (int32_t)((int64_t)p + DIR * (step + 1 + bl)); }
    if (sm) break;
  }
}

template <class T>
__global__ __launch_bounds__(64 * kPkPromWaves) void pk_prom_kernel(PkArgs a, PkPromArgs q) {
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  const int w = threadIdx.x >> 6;
  for (int64_t c = (int64_t)blockIdx.x * kPkPromWaves + w; c < nc; c += (int64_t)gridDim.x * kPkPromWaves) {
    const int32_t p = q.cidx[row * q.ccap + c] + r.lo;
    const double vp = r.at(p);
    double lmin, rmin;
    int32_t lb, rb;
    pk_scan_side<T, -1>(r, p, vp, lmin, lb);
    pk_scan_side<T, 1>(r, p, vp, rmin, rb);
    const double prom = vp - (lmin > rmin ? lmin : rmin);
    const bool keep = pk_in(prom, q.pmin, q.pmax);
    if ((threadIdx.x & 63) == 0) {
      q.cprom[row * q.ccap + c] = prom;
      q.clb[row * q.ccap + c] = keep ? lb - r.lo : -1;
      q.crb[row * q.ccap + c] = rb - r.lo;
    }
  }
}

__global__ __launch_bounds__(kPkThreads) void pk_ccount_kernel(PkPromArgs q, int32_t row0, int32_t ncseg,
                                                               int32_t* __restrict__ segcount) {
  __shared__ int s_w[kPkWaves];
  const int64_t row = (int64_t)row0 + blockIdx.y;
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  int cnt = 0;
  if (base < nc) {
#pragma unroll
    for (int k = 0; k < kPkPer; ++k) {
      const int64_t c = base + k * kPkThreads + threadIdx.x;
      cnt += __popcll(__ballot(c < nc && q.clb[row * q.ccap + c] >= 0));
    }
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kPkWaves; ++w) t += s_w[w];
    segcount[row * ncseg + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kPkThreads) void pk_cwrite_kernel(PkPromArgs q, int32_t row0, int32_t ncseg,
                                                               const int32_t* __restrict__ segoff,
                                                               int32_t* __restrict__ idx, double* __restrict__ prom,
                                                               int32_t* __restrict__ lb, int32_t* __restrict__ rb,
                                                               int64_t cap) {
  __shared__ int s_c[kPkPer][kPkWaves];
  const int64_t row = (int64_t)row0 + blockIdx.y;
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  if (base >= nc) return;                                      // (workgroup-uniform)
  bool keep[kPkPer];
  uint64_t m[kPkPer];
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    const int64_t c = base + k * kPkThreads + threadIdx.x;
    keep[k] = c < nc && q.clb[row * q.ccap + c] >= 0;
    m[k] = __ballot(keep[k]);
    if ((threadIdx.x & 63) == 0) s_c[k][threadIdx.x >> 6] = __popcll(m[k]);
  }
  __syncthreads();
  const int64_t off = segoff[row * ncseg + blockIdx.x];
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    if (keep[k]) {
      const int64_t pos = off + pk_rank(m, k, s_c);
      if (pos < cap) {
        const int64_t c = row * q.ccap + base + k * kPkThreads + threadIdx.x;
        idx[row * cap + pos] = q.cidx[c];
        prom[row * cap + pos] = q.cprom[c];
        lb[row * cap + pos] = q.clb[c];
        rb[row * cap + pos] = q.crb[c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
constexpr int64_t kPkMaxN = 0x7fffffff - 2 * kPkSeg;           // 32-bit sample indices, segment arithmetic included

size_t pk_align(size_t v) { return (v + 255) / 256 * 256; }
int64_t pk_max_peaks(int64_t n) { return n < 3 ? 0 : (n - 1) / 2; }
int64_t pk_segs(int64_t n) { return std::max<int64_t>(1, (n + kPkSeg - 1) / kPkSeg); }

struct PkWs {
  int32_t *segcount, *ccount, *cidx, *clb, *crb, *csegcount;
  double* cprom;
  size_t bytes;
};

PkWs pk_carve(void* d_ws, int64_t rows, int64_t n) {
  const size_t ccap = (size_t)pk_max_peaks(n), R = (size_t)rows;
  char* w = (char*)d_ws;
  size_t o = 0;
  PkWs s;
  s.segcount = (int32_t*)(w + o);  o += pk_align(R * (size_t)pk_segs(n) * sizeof(int32_t));
  s.ccount = (int32_t*)(w + o);    o += pk_align(R * sizeof(int32_t));
  s.csegcount = (int32_t*)(w + o); o += pk_align(R * (size_t)pk_segs((int64_t)ccap) * sizeof(int32_t));
  s.cprom = (double*)(w + o);      o += pk_align(R * ccap * sizeof(double));
  s.cidx = (int32_t*)(w + o);      o += pk_align(R * ccap * sizeof(int32_t));
  s.clb = (int32_t*)(w + o);       o += pk_align(R * ccap * sizeof(int32_t));
  s.crb = (int32_t*)(w + o);       o += pk_align(R * ccap * sizeof(int32_t));
  s.bytes = o;
  return s;
}

template <class T>
int pk_run(const mm_peaks_opts* o, PkArgs a, int64_t rows, int64_t cap, int32_t* d_count, int32_t* d_idx, double* d_prom,
           int32_t* d_lb, int32_t* d_rb, const PkWs& ws, hipStream_t st) {
  const bool prom = o->use_prominence != 0;
  const int64_t ccap = pk_max_peaks(a.n);
  const int32_t ncseg = (int32_t)pk_segs(ccap);
  PkPromArgs q;
  q.ccount = ws.ccount; q.cidx = ws.cidx; q.cprom = ws.cprom; q.clb = ws.clb; q.crb = ws.crb; q.ccap = ccap;
  q.pmin = o->prominence[0]; q.pmax = o->prominence[1];
  // without prominence the first compaction writes the outputs; with it, the candidate list of the workspace
  int32_t* idx1 = prom ? ws.cidx : d_idx;
  const int64_t cap1 = prom ? ccap : cap;
  for (int64_t r0 = 0; r0 < rows; r0 += kPkMaxGridY) {
    a.row0 = (int32_t)r0;
    const unsigned ry = (unsigned)std::min<int64_t>(rows - r0, kPkMaxGridY);
    hipLaunchKernelGGL(pk_count_kernel<T>, dim3((unsigned)a.nseg, ry), dim3(kPkThreads), 0, st, a, ws.segcount);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)rows), dim3(kPkThreads), 0, st, ws.segcount, a.nseg,
                     prom ? ws.ccount : d_count, prom ? (int32_t*)nullptr : d_idx, (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, cap);
  HIP_TRY(hipGetLastError());
  if (cap1 > 0) {
    for (int64_t r0 = 0; r0 < rows; r0 += kPkMaxGridY) {
      a.row0 = (int32_t)r0;
      const unsigned ry = (unsigned)std::min<int64_t>(rows - r0, kPkMaxGridY);
      hipLaunchKernelGGL(pk_write_kernel<T>, dim3((unsigned)a.nseg, ry), dim3(kPkThreads), 0, st, a, ws.segcount, idx1, cap1);
      HIP_TRY(hipGetLastError());
    }
  }
  if (!prom) return MM_OK;
  if (ccap > 0) {
    const unsigned gx = (unsigned)std::min<int64_t>((ccap + kPkPromWaves - 1) / kPkPromWaves, kPkPromMaxGridX);
    for (int64_t r0 = 0; r0 < rows; r0 += kPkMaxGridY) {
      a.row0 = (int32_t)r0;
      const unsigned ry = (unsigned)std::min<int64_t>(rows - r0, kPkMaxGridY);
      hipLaunchKernelGGL(pk_prom_kernel<T>, dim3(gx, ry), dim3(64 * kPkPromWaves), 0, st, a, q);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(pk_ccount_kernel, dim3((unsigned)ncseg, ry), dim3(kPkThreads), 0, st, q, (int32_t)r0, ncseg,
                         ws.csegcount);
      HIP_TRY(hipGetLastError());
    }
  } else {
    HIP_TRY(hipMemsetAsync(ws.csegcount, 0, (size_t)rows * ncseg * sizeof(int32_t), st));
  }
  hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)rows), dim3(kPkThreads), 0, st, ws.csegcount, ncseg, d_count, d_idx,
                     d_lb, d_rb, d_prom, cap);
  HIP_TRY(hipGetLastError());
  if (cap > 0 && ccap > 0) {
    for (int64_t r0 = 0; r0 < rows; r0 += kPkMaxGridY) {
      const unsigned ry = (unsigned)std::min<int64_t>(rows - r0, kPkMaxGridY);
      hipLaunchKernelGGL(pk_cwrite_kernel, dim3((unsigned)ncseg, ry), dim3(kPkThreads), 0, st, q, (int32_t)r0, ncseg,
                         ws.csegcount, d_idx, d_prom, d_lb, d_rb, cap);
      HIP_TRY(hipGetLastError());
    }
  }
  return MM_OK;
}

bool pk_interval_ok(const double (&v)[2]) { return !std::isnan(v[0]) && !std::isnan(v[1]); }

}  // namespace

extern "C" {

size_t mm_find_peaks_workspace_bytes(int64_t rows, int64_t n) {
  if (rows < 1 || rows > 0x7fffffff || n < 1 || n > kPkMaxN) return 0;
  return pk_carve(nullptr, rows, n).bytes;
}

int mm_find_peaks(const mm_peaks_opts* opts, const void* d_x, int32_t dtype, int64_t rows, int64_t n, int64_t x_stride,
                  const int32_t* d_lo, const int32_t* d_hi, int64_t cap, int32_t* d_count, int32_t* d_idx, double* d_prom,
                  int32_t* d_lbase, int32_t* d_rbase, void* d_ws, size_t ws_bytes, void* stream) {
  if (!opts || !d_x || !d_count || !d_ws || (dtype != 0 && dtype != 1)) return MM_ERR_INVALID_ARG;
  if (rows < 1 || rows > 0x7fffffff || n < 1 || n > kPkMaxN || x_stride < n || cap < 0 || cap > kPkMaxN)
    return MM_ERR_INVALID_ARG;
  if (cap > 0 && !d_idx) return MM_ERR_INVALID_ARG;
  if (!pk_interval_ok(opts->height) || !pk_interval_ok(opts->threshold) || !pk_interval_ok(opts->prominence))
    return MM_ERR_INVALID_ARG;
  if (opts->use_prominence && cap > 0 && (!d_prom || !d_lbase || !d_rbase)) return MM_ERR_INVALID_ARG;
  const PkWs ws = pk_carve(d_ws, rows, n);
  if (ws_bytes < ws.bytes) return MM_ERR_WORKSPACE;
  PkArgs a;
  a.x = d_x; a.x_stride = x_stride; a.lo = d_lo; a.hi = d_hi; a.n = (int32_t)n; a.nseg = (int32_t)pk_segs(n); a.row0 = 0;
  a.negate = opts->negate != 0; a.use_height = opts->use_height != 0; a.use_threshold = opts->use_threshold != 0;
  a.hmin = opts->height[0]; a.hmax = opts->height[1]; a.tmin = opts->threshold[0]; a.tmax = opts->threshold[1];
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) return pk_run<float>(opts, a, rows, cap, d_count, d_idx, d_prom, d_lbase, d_rbase, ws, st);
  return pk_run<double>(opts, a, rows, cap, d_count, d_idx, d_prom, d_lbase, d_rbase, ws, st);
}

}  // extern "C"
