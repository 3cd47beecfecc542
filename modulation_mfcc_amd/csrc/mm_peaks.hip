// libmodmfcc: peak / trough detection on batches of curves -- scipy.signal.find_peaks(y) / find_peaks(-y) as the
// reference's MinMaxFinder calls it (script/calc.py:651-686, script/main.py:1546-1613), with the height, threshold and
// prominence (wlen=None) conditions.  gfx950 only.  The kernels ("Peaks"):
//   pk_count_kernel   rising edges of a segment that resolve to a peak and pass height / threshold -> count per segment
//   pk_scan_kernel    exclusive scan of a row's segment counts; the row's total; -1 fill of the unused index slots
//   pk_write_kernel   the same test again, plateau midpoints written at scan offset + rank (ballot / popcount)
//   pk_prom_kernel <T, false>   one wave per candidate: prominence and bases, 64 samples a step; a drop is left base -1
//   pk_ccount_kernel / pk_cwrite_kernel   the candidates a keep array (here the left bases) keeps, compacted the same way
// mm_find_peaks_ex adds plateau_size, distance, wlen and width as stages over the candidate list of the workspace, each
// clearing a candidate's keep flag, and the same compaction on that flag at the end (one driver, pk_run, for both):
//   pk_count / pk_write <T, true>   the plateau's edges beside its midpoint, plateau_size filtered with height / threshold
//   pk_distance_kernel    a workgroup per row: scipy's greedy selection as a fixed point, every round inside the launch
//   pk_prom_kernel <T, true>    a wave per kept candidate: prominence inside wlen, then scipy's peak_widths at rel_height
//   pk_ccount_kernel / pk_cwrite_kernel   the kept candidates and every property the caller asked for
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
  int32_t use_plateau;      // read by the <T, true> kernels only
  double psmin, psmax;
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
// of a plateau whose first different sample is lower.  Then height and threshold, scipy's order and arithmetic.  EX: the
// plateau's edges (relative to lo) come back too -- the lane that owns the rising edge has walked to the falling one,
// across segment boundaries as well -- and plateau_size is tested first.
template <class T, bool EX>
__device__ __forceinline__ int32_t pk_peak_at(const PkArgs& a, const PkRow<T>& r, int32_t i, int32_t& le, int32_t& re) {
  if (i <= r.lo || i >= r.hi - 1) return -1;
  const double v = r.at(i);
  if (!(r.at(i - 1) < v)) return -1;
  int32_t j = i + 1;
  const int32_t last = r.hi - 1;
  while (j < last && r.at(j) == v) ++j;            // the lane walks its plateau alone
  if (!(r.at(j) < v)) return -1;
  const int32_t mid = (int32_t)(((int64_t)i + (j - 1)) / 2);
  if (EX) {
    le = i - r.lo; re = j - 1 - r.lo;
    if (a.use_plateau && !pk_in((double)(j - i), a.psmin, a.psmax)) return -1;
  }
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

// The count of segment blockIdx.x: the number of its elements i (kPkPer rounds of kPkThreads) for which hit(i) holds goes
// to *dst.  A segment outside [lo, hi) (workgroup-uniform) has nothing to test.
// (The callables of this helper and of pk_seg_compact capture kernel arguments by value: captured by reference they
// cost registers and about a tenth more instructions; docs/experiments.md, "One driver for the peak search".)
template <class Hit>
__device__ __forceinline__ void pk_seg_count(int32_t lo, int32_t hi, int32_t* dst, Hit hit) {
  __shared__ int s_w[kPkWaves];
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  int cnt = 0;                                       // wave-uniform
  if (base < hi && base + kPkSeg > lo) {
#pragma unroll
    for (int k = 0; k < kPkPer; ++k) cnt += __popcll(__ballot(hit(base + k * kPkThreads + threadIdx.x)));
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kPkWaves; ++w) t += s_w[w];
    *dst = t;
  }
}

template <class T, bool EX>
__global__ __launch_bounds__(kPkThreads) void pk_count_kernel(PkArgs a, int32_t* __restrict__ segcount) {
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  pk_seg_count(r.lo, r.hi, segcount + row * a.nseg + blockIdx.x, [=](int64_t i) {
    int32_t le, re;
    return i < a.n && pk_peak_at<T, EX>(a, r, (int32_t)i, le, re) >= 0;
  });
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

// the output arrays whose unused slots a scan pads: i[0] the indices, then bases and edges; prominences and widths
struct PkFill {
  int32_t* i[6];
  double* d[5];
};

// A workgroup per row: segcount[row][0 .. nseg) becomes its exclusive prefix, total[row] the sum; every array of f that
// is not NULL is filled over [row][min(total, cap) .. cap), integers with -1, doubles with NaN (f.i[0] == nullptr: the
// candidate pass, whose consumers read only below the count).
__global__ __launch_bounds__(kPkThreads) void pk_scan_kernel(int32_t* __restrict__ segcount, int32_t nseg,
                                                             int32_t* __restrict__ total, PkFill f, int64_t cap) {
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
  if (f.i[0]) {
    for (int64_t k = min<int64_t>(tot, cap) + threadIdx.x; k < cap; k += kPkThreads) {
#pragma unroll
      for (int u = 0; u < 6; ++u)
        if (f.i[u]) f.i[u][row * cap + k] = -1;
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (f.d[u]) f.d[u][row * cap + k] = NAN;
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

// EX: the candidate's edges and its keep flag (1) go to the workspace beside the midpoint
struct PkEdges {
  int32_t *le, *re, *keep;
};

// The compaction of segment blockIdx.x (every thread of the workgroup calls it): hit(k, i) says whether element i, this
// thread's of round k, stays; the ones that stay take the positions *segoff + rank, ascending, and emit(k, i, pos) writes
// one whose position is below cap.
template <class Hit, class Emit>
__device__ __forceinline__ void pk_seg_compact(const int32_t* segoff, int64_t cap, Hit hit, Emit emit) {
  __shared__ int s_c[kPkPer][kPkWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kPkSeg + threadIdx.x;
  bool h[kPkPer];
  uint64_t m[kPkPer];
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    h[k] = hit(k, i0 + k * kPkThreads);
    m[k] = __ballot(h[k]);
    if ((threadIdx.x & 63) == 0) s_c[k][threadIdx.x >> 6] = __popcll(m[k]);
  }
  __syncthreads();
  const int64_t off = *segoff;
#pragma unroll
  for (int k = 0; k < kPkPer; ++k) {
    if (h[k]) {
      const int64_t pos = off + pk_rank(m, k, s_c);
      if (pos < cap) emit(k, i0 + k * kPkThreads, pos);
    }
  }
}

template <class T, bool EX>
__global__ __launch_bounds__(kPkThreads) void pk_write_kernel(PkArgs a, const int32_t* __restrict__ segoff,
                                                              int32_t* __restrict__ idx, int64_t cap, PkEdges e) {
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  const int64_t base = (int64_t)blockIdx.x * kPkSeg;
  if (!(base < r.hi && base + kPkSeg > r.lo)) return;          // (workgroup-uniform)
  int32_t mid[kPkPer], le[kPkPer], re[kPkPer];
  pk_seg_compact(
      segoff + row * a.nseg + blockIdx.x, cap,
      [=, &mid, &le, &re](int k, int64_t i) {
        mid[k] = i < a.n ? pk_peak_at<T, EX>(a, r, (int32_t)i, le[k], re[k]) : -1;
        return mid[k] >= 0;
      },
      [=, &mid, &le, &re](int k, int64_t, int64_t pos) {
        idx[row * cap + pos] = mid[k];
        if (EX) { e.le[row * cap + pos] = le[k]; e.re[row * cap + pos] = re[k]; e.keep[row * cap + pos] = 1; }
      });
}

// The candidate list of the workspace.  A candidate keeps the slot the first compaction gave it.  mm_find_peaks has the
// first row of arrays only and drops a candidate by a left base of -1; the stages of mm_find_peaks_ex drop one by setting
// its keep flag to -1, later stages skip it.  Either way the last compaction removes it.
struct PkCand {
  int32_t* ccount;                                  // [rows] candidates per row
  int64_t ccap;
  int32_t *idx, *lb, *rb;                           // [rows][ccap]; idx ascending, relative to lo
  double* prom;
  int32_t *keep, *le, *re;                          // the stages only (NULL otherwise)
  double *w, *wh, *lip, *rip;                       // wh holds the heights while the distance stage runs
};

// ---------------------------------------------------------------------------------------------------------------------
// prominence (scipy's _peak_prominences): a wave per candidate.  Each step looks at the next 64 samples away
// from the peak; the first lane whose sample is above the peak, NaN or outside the row ends the scan (ballot), the lanes
// before it take part in a (value, distance) min-reduction in which an equal value nearer the peak wins; a step's
// minimum replaces the running one only when strictly lower -- together scipy's "first reached with <".
// ---------------------------------------------------------------------------------------------------------------------
// lim: the last sample of the scan (inclusive): the row's (slice's) end, or the end of scipy's wlen window
template <class T, int DIR>
__device__ __forceinline__ void pk_scan_side(const PkRow<T>& r, int32_t p, int32_t lim, double vp, double& best,
                                             int32_t& base) {
  const int lane = threadIdx.x & 63;
  best = vp; base = p;
  for (int64_t step = 0;; step += 64) {
    const int64_t i = (int64_t)p + DIR * (step + 1 + lane);
    const bool inside = DIR < 0 ? i >= lim : i <= lim;
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

// scipy's _peak_widths on one side: from the peak towards its base, the first sample that is the base itself or not above
// the evaluation height h; 64 samples a step, the first stopping lane decides (the lane at the peak itself included)
template <class T, int DIR>
__device__ __forceinline__ int32_t pk_cross_side(const PkRow<T>& r, int32_t p, int32_t base, double h) {
  const int lane = threadIdx.x & 63;
  for (int64_t step = 0;; step += 64) {
    const int64_t i = (int64_t)p + DIR * (step + lane);
    const bool inside = DIR < 0 ? i > base : i < base;
    const double v = inside ? r.at((int32_t)i) : 0.0;
    const uint64_t sm = __ballot(!inside || !(h < v));
    if (sm) return (int32_t)((int64_t)p + DIR * (step + __ffsll((unsigned long long)sm) - 1));
  }
}

// pmin, pmax last and the kernel's PkCand behind them, ccap second in it: what the <T, false> kernel reads is then one
// 64-byte stretch of the kernel arguments.  On a batch a wave of that kernel lives for one candidate, and with the
// arguments scattered over six loads it took 1.3 % longer (docs/experiments.md, "One driver for the peak search").
struct PkPromOpts {
  double wmin, wmax, rel_height;                    // EX only, as wlen and use_width
  int32_t wlen, use_width;
  double pmin, pmax;
};

// A wave per candidate: the prominence, its bases and its interval.  EX = false: every candidate, the whole slice, and a
// candidate the interval drops gets the left base -1.  EX = true: the kept candidates, inside scipy's wlen window
// ([p - wlen / 2, p + wlen / 2] clipped to the slice; wlen < 2: the slice), then -- for the survivors -- scipy's
// peak_widths, operation for operation in float64 with contraction off (an fma in h or the interpolation changes the
// last bit), and the width interval; a drop clears the keep flag.
template <class T, bool EX>
__global__ __launch_bounds__(64 * kPkPromWaves) void pk_prom_kernel(PkArgs a, PkPromOpts o, PkCand q) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)a.row0 + blockIdx.y;
  const PkRow<T> r(a, row);
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  const int w = threadIdx.x >> 6;
  for (int64_t c = (int64_t)blockIdx.x * kPkPromWaves + w; c < nc; c += (int64_t)gridDim.x * kPkPromWaves) {
    const int64_t at = row * q.ccap + c;
    if constexpr (EX) {
      if (q.keep[at] < 0) continue;                   // (wave-uniform)
    }
    const int32_t p = q.idx[at] + r.lo;
    const double vp = r.at(p);
    int32_t wl = r.lo, wr = r.hi - 1;
    if constexpr (EX) {
      if (o.wlen >= 2) {
        wl = max(wl, p - o.wlen / 2);
        wr = (int32_t)min<int64_t>(wr, (int64_t)p + o.wlen / 2);
      }
    }
    double lmin, rmin;
    int32_t lb, rb;
    pk_scan_side<T, -1>(r, p, wl, vp, lmin, lb);
    pk_scan_side<T, 1>(r, p, wr, vp, rmin, rb);
    const double prom = vp - (lmin > rmin ? lmin : rmin);
    bool keep = pk_in(prom, o.pmin, o.pmax);
    if constexpr (EX) {
      double width = 0.0, h = 0.0, lip = 0.0, rip = 0.0;
      if (keep && o.use_width) {
        h = vp - prom * o.rel_height;                 // two roundings (contract off), as the host compiler gives scipy
        const int32_t il = pk_cross_side<T, -1>(r, p, lb, h), ir = pk_cross_side<T, 1>(r, p, rb, h);
        const double xl = r.at(il), xr = r.at(ir);
        lip = (double)(il - r.lo);
        if (xl < h) lip += (h - xl) / (r.at(il + 1) - xl);
        rip = (double)(ir - r.lo);
        if (xr < h) rip -= (h - xr) / (r.at(ir - 1) - xr);
        width = rip - lip;
        keep = pk_in(width, o.wmin, o.wmax);
      }
      if ((threadIdx.x & 63) == 0) {
        q.prom[at] = prom; q.lb[at] = lb - r.lo; q.rb[at] = rb - r.lo;
        if (o.use_width) { q.w[at] = width; q.wh[at] = h; q.lip[at] = lip; q.rip[at] = rip; }
        if (!keep) q.keep[at] = -1;
      }
    } else if ((threadIdx.x & 63) == 0) {
      q.prom[at] = prom; q.lb[at] = keep ? lb - r.lo : -1; q.rb[at] = rb - r.lo;
    }
  }
}

// keep [rows][ccap]: a candidate stays when its entry is >= 0 (the left bases of mm_find_peaks, or the stages' flags)
__global__ __launch_bounds__(kPkThreads) void pk_ccount_kernel(const int32_t* __restrict__ ccount,
                                                               const int32_t* __restrict__ keep, int64_t ccap,
                                                               int32_t row0, int32_t ncseg,
                                                               int32_t* __restrict__ segcount) {
  const int64_t row = (int64_t)row0 + blockIdx.y;
  const int32_t nc = (int32_t)min<int64_t>(ccount[row], ccap);
  pk_seg_count(0, nc, segcount + row * ncseg + blockIdx.x,
               [=](int64_t c) { return c < nc && keep[row * ccap + c] >= 0; });
}

// the candidates keep keeps, and each property whose output pointer is not NULL, at scan offset + rank
__global__ __launch_bounds__(kPkThreads) void pk_cwrite_kernel(PkCand q, const int32_t* __restrict__ keep, int32_t row0,
                                                               int32_t ncseg, const int32_t* __restrict__ segoff,
                                                               mm_peaks_out out, int64_t cap) {
  const int64_t row = (int64_t)row0 + blockIdx.y;
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  if ((int64_t)blockIdx.x * kPkSeg >= nc) return;              // (workgroup-uniform)
  pk_seg_compact(
      segoff + row * ncseg + blockIdx.x, cap,
      [=](int, int64_t i) { return i < nc && keep[row * q.ccap + i] >= 0; },
      [=](int, int64_t i, int64_t pos) {
        const int64_t c = row * q.ccap + i, d = row * cap + pos;
        out.idx[d] = q.idx[c];
        if (out.prom) { out.prom[d] = q.prom[c]; out.lbase[d] = q.lb[c]; out.rbase[d] = q.rb[c]; }
        if (out.widths) out.widths[d] = q.w[c];
        if (out.width_heights) out.width_heights[d] = q.wh[c];
        if (out.left_ips) out.left_ips[d] = q.lip[c];
        if (out.right_ips) out.right_ips[d] = q.rip[c];
        if (out.plateau_sizes) out.plateau_sizes[d] = q.re[c] - q.le[c] + 1;
        if (out.left_edges) out.left_edges[d] = q.le[c];
        if (out.right_edges) out.right_edges[d] = q.re[c];
      });
}

constexpr int kPkDistThreads = 1024;

__device__ __forceinline__ int32_t pk_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void pk_st(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// scipy's _select_by_peak_distance (the highest peak first, each survivor deleting what is nearer than distance) as a
// fixed point, a workgroup per row, all rounds in this launch.  Priority is (height, index): of two equally high peaks
// the one with the larger index goes first, which is a stable argsort walked from its end.  keep: 0 undecided, -1
// deleted, k >= 1 kept in round k.  Round k: an undecided peak with no undecided neighbour of higher priority nearer
// than distance becomes kept (a peak marked k in this very pass still counts as undecided for its neighbours); after
// the barrier the peaks kept in round k delete their undecided neighbours.  The highest undecided peak of a row is
// always kept, so there are at most as many rounds as peaks (a ramp of peaks under a distance that reaches one
// neighbour needs half as many); typical curves need a handful.
template <class T>
__global__ __launch_bounds__(kPkDistThreads) void pk_distance_kernel(PkArgs a, PkCand q, int32_t distance) {
  const int64_t row = blockIdx.x;
  const PkRow<T> r(a, row);
  const int32_t nc = (int32_t)min<int64_t>(q.ccount[row], q.ccap);
  const int32_t* pos = q.idx + row * q.ccap;
  double* h = q.wh + row * q.ccap;
  int32_t* keep = q.keep + row * q.ccap;
  for (int32_t c = threadIdx.x; c < nc; c += kPkDistThreads) {
    h[c] = r.at(pos[c] + r.lo);
    pk_st(keep + c, 0);
  }
  __syncthreads();
  for (int32_t round = 1; round <= nc + 1; ++round) {
    int open = 0;
    for (int32_t c = threadIdx.x; c < nc; c += kPkDistThreads) {
      if (pk_ld(keep + c) != 0) continue;
      open = 1;
      const int32_t pc = pos[c];
      const double hc = h[c];
      bool top = true;
      for (int32_t j = c - 1; top && j >= 0 && pc - pos[j] < distance; --j) {
        const int32_t s = pk_ld(keep + j);
        if ((s == 0 || s == round) && h[j] > hc) top = false;
      }
      for (int32_t j = c + 1; top && j < nc && pos[j] - pc < distance; ++j) {
        const int32_t s = pk_ld(keep + j);
        if ((s == 0 || s == round) && h[j] >= hc) top = false;
      }
      if (top) pk_st(keep + c, round);
    }
    if (!__syncthreads_or(open)) break;
    for (int32_t c = threadIdx.x; c < nc; c += kPkDistThreads) {
      if (pk_ld(keep + c) != round) continue;
      const int32_t pc = pos[c];
      for (int32_t j = c - 1; j >= 0 && pc - pos[j] < distance; --j)
        if (pk_ld(keep + j) == 0) pk_st(keep + j, -1);
      for (int32_t j = c + 1; j < nc && pos[j] - pc < distance; ++j)
        if (pk_ld(keep + j) == 0) pk_st(keep + j, -1);
    }
    __syncthreads();
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
  int32_t *segcount, *csegcount;
  PkCand q;                               // the arrays of the stages are NULL unless ex
  size_t bytes;
};

PkWs pk_carve(void* d_ws, int64_t rows, int64_t n, bool ex) {
  const size_t ccap = (size_t)pk_max_peaks(n), R = (size_t)rows;
  PkWs s = {};
  size_t o = 0;
  auto take = [&](size_t bytes) {
    void* p = (char*)d_ws + o;
    o += pk_align(bytes);
    return p;
  };
  s.segcount = (int32_t*)take(R * (size_t)pk_segs(n) * sizeof(int32_t));
  s.q.ccount = (int32_t*)take(R * sizeof(int32_t));
  s.csegcount = (int32_t*)take(R * (size_t)pk_segs((int64_t)ccap) * sizeof(int32_t));
  const size_t di = R * ccap * sizeof(int32_t), dd = R * ccap * sizeof(double);
  s.q.prom = (double*)take(dd);
  s.q.idx = (int32_t*)take(di);
  s.q.lb = (int32_t*)take(di);
  s.q.rb = (int32_t*)take(di);
  if (ex) {
    s.q.w = (double*)take(dd);
    s.q.wh = (double*)take(dd);
    s.q.lip = (double*)take(dd);
    s.q.rip = (double*)take(dd);
    s.q.keep = (int32_t*)take(di);
    s.q.le = (int32_t*)take(di);
    s.q.re = (int32_t*)take(di);
  }
  s.q.ccap = (int64_t)ccap;
  s.bytes = o;
  return s;
}

// launch(r0, ry) for every chunk of at most kPkMaxGridY rows: r0 is the chunk's first row, ry the grid's y extent
template <class F>
hipError_t pk_rows(int64_t rows, F launch) {
  for (int64_t r0 = 0; r0 < rows; r0 += kPkMaxGridY) {
    launch((int32_t)r0, (unsigned)std::min<int64_t>(rows - r0, kPkMaxGridY));
    if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  }
  return hipSuccess;
}

bool pk_interval_ok(const double (&v)[2]) { return !std::isnan(v[0]) && !std::isnan(v[1]); }

// count, scan, first compaction, [distance], [prominence (+ widths)], candidate count, scan, final compaction.  e is read
// only when staged; out holds the arrays of the conditions that run and NULL for the others.
template <class T>
int pk_run(const mm_peaks_opts* o, const mm_peaks_ext* e, bool staged, const PkArgs& a0, int64_t rows, int64_t cap,
           const mm_peaks_out& out, const PkWs& ws, hipStream_t st) {
  const bool need_prom = o->use_prominence != 0 || (staged && e->use_width != 0);
  // with neither stages nor prominence the first compaction writes the outputs; otherwise the candidate list
  const bool direct = !staged && !need_prom;
  const PkCand& q = ws.q;
  const int32_t ncseg = (int32_t)pk_segs(q.ccap);
  const int32_t* keep = staged ? q.keep : q.lb;
  const unsigned gseg = (unsigned)a0.nseg, gcseg = (unsigned)ncseg;
  const dim3 thr(kPkThreads);
  PkPromOpts po = {};
  po.pmin = o->use_prominence ? o->prominence[0] : -INFINITY; po.pmax = o->use_prominence ? o->prominence[1] : INFINITY;
  if (staged) {
    po.wmin = e->width[0]; po.wmax = e->width[1]; po.rel_height = e->rel_height;
    po.wlen = e->wlen; po.use_width = e->use_width != 0;
  }
  PkFill f1 = {}, f = {};
  f1.i[0] = direct ? out.idx : nullptr;
  f.i[0] = out.idx; f.i[1] = out.lbase; f.i[2] = out.rbase; f.i[3] = out.plateau_sizes; f.i[4] = out.left_edges;
  f.i[5] = out.right_edges;
  f.d[0] = out.prom; f.d[1] = out.widths; f.d[2] = out.width_heights; f.d[3] = out.left_ips; f.d[4] = out.right_ips;

  const auto from = [&](int32_t r0) {                // the kernel arguments of the chunk that starts at row r0
    PkArgs a = a0;
    a.row0 = r0;
    return a;
  };
  const auto count = staged ? pk_count_kernel<T, true> : pk_count_kernel<T, false>;
  HIP_TRY(pk_rows(rows, [&](int32_t r0, unsigned ry) {
    hipLaunchKernelGGL(count, dim3(gseg, ry), thr, 0, st, from(r0), ws.segcount);
  }));
  hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)rows), thr, 0, st, ws.segcount, a0.nseg,
                     direct ? out.count : q.ccount, f1, cap);
  HIP_TRY(hipGetLastError());
  const int64_t cap1 = direct ? cap : q.ccap;
  if (cap1 > 0) {
    const auto write = staged ? pk_write_kernel<T, true> : pk_write_kernel<T, false>;
    HIP_TRY(pk_rows(rows, [&](int32_t r0, unsigned ry) {
      hipLaunchKernelGGL(write, dim3(gseg, ry), thr, 0, st, from(r0), ws.segcount, direct ? out.idx : q.idx, cap1,
                         PkEdges{q.le, q.re, q.keep});
    }));
  }
  if (direct) return MM_OK;
  if (q.ccap > 0) {
    if (staged && e->use_distance) {
      hipLaunchKernelGGL(pk_distance_kernel<T>, dim3((unsigned)rows), dim3(kPkDistThreads), 0, st, from(0), q,
                         e->distance);
      HIP_TRY(hipGetLastError());
    }
    const auto prom = staged ? pk_prom_kernel<T, true> : pk_prom_kernel<T, false>;
    const unsigned gx = (unsigned)std::min<int64_t>((q.ccap + kPkPromWaves - 1) / kPkPromWaves, kPkPromMaxGridX);
    HIP_TRY(pk_rows(rows, [&](int32_t r0, unsigned ry) {
      if (need_prom) hipLaunchKernelGGL(prom, dim3(gx, ry), dim3(64 * kPkPromWaves), 0, st, from(r0), po, q);
      hipLaunchKernelGGL(pk_ccount_kernel, dim3(gcseg, ry), thr, 0, st, q.ccount, keep, q.ccap, r0, ncseg,
                         ws.csegcount);
    }));
  } else {
    fill_words(ws.csegcount, 0u, (int64_t)rows * ncseg, st);
  }
  hipLaunchKernelGGL(pk_scan_kernel, dim3((unsigned)rows), thr, 0, st, ws.csegcount, ncseg, out.count, f, cap);
  HIP_TRY(hipGetLastError());
  if (cap > 0 && q.ccap > 0) {
    HIP_TRY(pk_rows(rows, [&](int32_t r0, unsigned ry) {
      hipLaunchKernelGGL(pk_cwrite_kernel, dim3(gcseg, ry), thr, 0, st, q, keep, r0, ncseg, ws.csegcount, out, cap);
    }));
  }
  return MM_OK;
}

// whether a call needs the stages (and their workspace), or is one that mm_find_peaks answers with its own kernels
bool pk_is_ex(const mm_peaks_opts* o, const mm_peaks_ext* e) {
  return e && (e->use_plateau_size || e->use_distance || e->use_width || (e->wlen > 0 && o->use_prominence));
}

bool pk_shape_ok(int64_t rows, int64_t n) { return rows >= 1 && rows <= 0x7fffffff && n >= 1 && n <= kPkMaxN; }

// every check, then the one driver
int pk_find(const mm_peaks_opts* opts, const mm_peaks_ext* ext, const void* d_x, int32_t dtype, int64_t rows, int64_t n,
            int64_t x_stride, const int32_t* d_lo, const int32_t* d_hi, int64_t cap, const mm_peaks_out* outp, void* d_ws,
            size_t ws_bytes, void* stream) {
  if (!opts || !d_x || !outp || !outp->count || !d_ws || (dtype != 0 && dtype != 1)) return MM_ERR_INVALID_ARG;
  if (!pk_shape_ok(rows, n) || x_stride < n || cap < 0 || cap > kPkMaxN) return MM_ERR_INVALID_ARG;
  mm_peaks_out out = *outp;
  if (cap > 0 && !out.idx) return MM_ERR_INVALID_ARG;
  if (!pk_interval_ok(opts->height) || !pk_interval_ok(opts->threshold) || !pk_interval_ok(opts->prominence))
    return MM_ERR_INVALID_ARG;
  if (ext) {
    if (!pk_interval_ok(ext->plateau_size) || !pk_interval_ok(ext->width) || !(ext->rel_height >= 0.0))
      return MM_ERR_INVALID_ARG;
    if ((ext->use_distance && ext->distance < 1) || ext->wlen == 1) return MM_ERR_INVALID_ARG;
  }
  const bool ex = pk_is_ex(opts, ext);
  const bool need_prom = opts->use_prominence || (ex && ext->use_width);
  if (need_prom && cap > 0 && (!out.prom || !out.lbase || !out.rbase)) return MM_ERR_INVALID_ARG;
  const PkWs ws = pk_carve(d_ws, rows, n, ex);
  if (ws_bytes < ws.bytes) return MM_ERR_WORKSPACE;
  // a property of a stage that does not run is not written
  if (!need_prom) { out.prom = nullptr; out.lbase = out.rbase = nullptr; }
  if (!ex || !ext->use_width) { out.widths = out.width_heights = nullptr; out.left_ips = out.right_ips = nullptr; }
  if (!ex || !ext->use_plateau_size) { out.plateau_sizes = nullptr; out.left_edges = out.right_edges = nullptr; }
  PkArgs a;
  a.x = d_x; a.x_stride = x_stride; a.lo = d_lo; a.hi = d_hi; a.n = (int32_t)n; a.nseg = (int32_t)pk_segs(n); a.row0 = 0;
  a.negate = opts->negate != 0; a.use_height = opts->use_height != 0; a.use_threshold = opts->use_threshold != 0;
  a.hmin = opts->height[0]; a.hmax = opts->height[1]; a.tmin = opts->threshold[0]; a.tmax = opts->threshold[1];
  a.use_plateau = ex && ext->use_plateau_size != 0;
  a.psmin = ex ? ext->plateau_size[0] : -INFINITY; a.psmax = ex ? ext->plateau_size[1] : INFINITY;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) return pk_run<float>(opts, ext, ex, a, rows, cap, out, ws, st);
  return pk_run<double>(opts, ext, ex, a, rows, cap, out, ws, st);
}

}  // namespace

extern "C" {

size_t mm_find_peaks_workspace_bytes(int64_t rows, int64_t n) {
  if (!pk_shape_ok(rows, n)) return 0;
  return pk_carve(nullptr, rows, n, false).bytes;
}

size_t mm_find_peaks_ex_workspace_bytes(const mm_peaks_opts* opts, const mm_peaks_ext* ext, int64_t rows, int64_t n) {
  if (!opts || !pk_shape_ok(rows, n)) return 0;
  return pk_carve(nullptr, rows, n, pk_is_ex(opts, ext)).bytes;
}

int mm_find_peaks(const mm_peaks_opts* opts, const void* d_x, int32_t dtype, int64_t rows, int64_t n, int64_t x_stride,
                  const int32_t* d_lo, const int32_t* d_hi, int64_t cap, int32_t* d_count, int32_t* d_idx, double* d_prom,
                  int32_t* d_lbase, int32_t* d_rbase, void* d_ws, size_t ws_bytes, void* stream) {
  mm_peaks_out out = {};
  out.count = d_count; out.idx = d_idx; out.prom = d_prom; out.lbase = d_lbase; out.rbase = d_rbase;
  return pk_find(opts, nullptr, d_x, dtype, rows, n, x_stride, d_lo, d_hi, cap, &out, d_ws, ws_bytes, stream);
}

int mm_find_peaks_ex(const mm_peaks_opts* opts, const mm_peaks_ext* ext, const void* d_x, int32_t dtype, int64_t rows,
                     int64_t n, int64_t x_stride, const int32_t* d_lo, const int32_t* d_hi, int64_t cap,
                     const mm_peaks_out* out, void* d_ws, size_t ws_bytes, void* stream) {
  return pk_find(opts, ext, d_x, dtype, rows, n, x_stride, d_lo, d_hi, cap, out, d_ws, ws_bytes, stream);
}

}  // extern "C"
