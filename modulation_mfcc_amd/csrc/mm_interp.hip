// libmodmfcc: the two places where the reference's script/calc.py calls scipy.interpolate.  gfx950 only.
//   interp_NAN (script/calc.py:345-385) for the kinds that need no solve over all knots: linear, pchip (PchipInterpolator
//   after the reference's end fix), nearest, nearest-up, previous, next, zero and slinear (interp1d,
//   fill_value='extrapolate').  ('quadratic' and 'cubic' are mm_spline.hip.)
//   read_AG50x (script/calc.py:173-219): interp1d(t_in, float32 column, 'linear') of every column of a .pos file.
// The kernels:
//   interp_linear_kernel   'linear': a workgroup per row, a thread per contiguous piece of it
//   ip_summary_kernel   a workgroup per segment of kIpSeg samples: the validity of its samples as sixteen wave ballots,
//                       from them the first two and the last two valid samples of the segment
//   ip_scan_kernel      a wave per row: the last two valid samples before and the first two after every segment (a scan of
//                       the summaries with "the nearer pair wins"), and the first / last two of the whole row
//   ip_eval_kernel<K>   a workgroup per segment again: lanes read adjacent samples, a NaN sample finds its neighbouring
//                       valid samples in the ballots of its own segment, beyond it in the scan's result, and evaluates
//   regrid_linear_kernel   a thread per output element, lanes along the interleaved columns: binary search of the input
//                       times (scipy's searchsorted index), then scipy's float32 / float64 arithmetic
// Valid samples are copied through.  The float64 arithmetic is written without contraction (no fused multiply-add), in
// scipy's order of operations.
#include "mm_common.h"

#include "mm_interp_seg.hip.inc"

namespace {

struct IpPair { int32_t a, b; };                        // the nearest and the second nearest valid sample, -1 = none

// the two nearest of a farther and a nearer set
__device__ __forceinline__ IpPair ip_comb(IpPair far, IpPair near) {
  if (near.a < 0) return far;
  if (near.b < 0) return IpPair{near.a, far.a};
  return near;
}

__global__ __launch_bounds__(kIpThreads) void ip_summary_kernel(const double* __restrict__ x, int64_t n_max,
                                                                int64_t x_stride, const int64_t* __restrict__ counts,
                                                                int32_t nseg, int4* __restrict__ summary) {
  __shared__ uint64_t s_m[kIpWords];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int64_t base = seg * kIpSeg;
  const int64_t n = ip_row_count(counts, row, n_max);
  double v[kIpPer];
  ip_load_segment(x + row * x_stride, n, base, v, s_m);
  if (threadIdx.x == 0) {
    int4 s = make_int4(-1, -1, -1, -1);                 // first, second, last, last but one
    // the searches exclude the index they start from: local samples 0 and kIpSeg - 1 are looked at by hand
    const int a = (s_m[0] & 1ull) ? 0 : ip_seg_next(s_m, 0);
    if (a >= 0) {
      s.x = (int32_t)(base + a);
      const int b = ip_seg_next(s_m, a);
      if (b >= 0) s.y = (int32_t)(base + b);
      const int z = (s_m[kIpWords - 1] >> 63) ? kIpSeg - 1 : ip_seg_prev(s_m, kIpSeg - 1);
      s.z = (int32_t)(base + z);
      const int y = ip_seg_prev(s_m, z);
      if (y >= 0) s.w = (int32_t)(base + y);
    }
    summary[blockIdx.x] = s;
  }
}

// carry[row][seg] = {last, last but one valid sample before the segment, first, second valid sample after it};
// rowinfo[row] = {first, second, last but one, last valid sample of the row}
__global__ __launch_bounds__(64) void ip_scan_kernel(const int4* __restrict__ summary, int32_t nseg, int4* __restrict__ carry,
                                                     int4* __restrict__ rowinfo) {
  const int64_t row = blockIdx.x;
  const int4* sm = summary + row * nseg;
  int4* cr = carry + row * nseg;
  const int lane = threadIdx.x;
  IpPair run_f{-1, -1}, run_b{-1, -1};
  for (int32_t c = 0; c < nseg; c += 64) {
    const int32_t sf = c + lane, sb = nseg - 1 - sf;    // forward and backward position of this lane
    const bool on = sf < nseg;
    IpPair f{-1, -1}, b{-1, -1};
    if (on) {
      const int4 u = sm[sf], w = sm[sb];
      f = IpPair{u.z, u.w};
      b = IpPair{w.x, w.y};
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const IpPair pf{__shfl_up(f.a, o, 64), __shfl_up(f.b, o, 64)};
      const IpPair pb{__shfl_up(b.a, o, 64), __shfl_up(b.b, o, 64)};
      if (lane >= o) { f = ip_comb(pf, f); b = ip_comb(pb, b); }
    }
    IpPair ef{__shfl_up(f.a, 1, 64), __shfl_up(f.b, 1, 64)}, eb{__shfl_up(b.a, 1, 64), __shfl_up(b.b, 1, 64)};
    if (lane == 0) { ef = IpPair{-1, -1}; eb = IpPair{-1, -1}; }
    ef = ip_comb(run_f, ef);
    eb = ip_comb(run_b, eb);
    if (on) {                                           // two lanes write the halves of one entry when sf == sb': plain ints
      int32_t* pf = (int32_t*)(cr + sf);
      int32_t* pb = (int32_t*)(cr + sb);
      pf[0] = ef.a; pf[1] = ef.b;
      pb[2] = eb.a; pb[3] = eb.b;
    }
    run_f = ip_comb(run_f, IpPair{__shfl(f.a, 63, 64), __shfl(f.b, 63, 64)});
    run_b = ip_comb(run_b, IpPair{__shfl(b.a, 63, 64), __shfl(b.b, 63, 64)});
  }
  if (lane == 0) rowinfo[row] = make_int4(run_b.a, run_b.b, run_f.b, run_f.a);
}

__device__ __forceinline__ double ip_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// scipy's PchipInterpolator._edge_case: the one-sided three-point estimate with its two shape corrections
__device__ __forceinline__ double ip_pchip_edge(double h0, double h1, double m0, double m1) {
#pragma clang fp contract(off)
  const double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
  if (ip_sign(d) != ip_sign(m0)) return 0.0;
  if (ip_sign(m0) != ip_sign(m1) && fabs(d) > 3.0 * fabs(m0)) return 3.0 * m0;
  return d;
}

// the weighted harmonic mean of the secant slopes left (hl, ml) and right (hr, mr) of an interior knot
__device__ __forceinline__ double ip_pchip_inner(double hl, double hr, double ml, double mr) {
#pragma clang fp contract(off)
  if (ip_sign(ml) != ip_sign(mr) || ml == 0.0 || mr == 0.0) return 0.0;
  const double w1 = 2.0 * hr + hl, w2 = hr + 2.0 * hl;
  const double whmean = (w1 / ml + w2 / mr) / (w1 + w2);
  return 1.0 / whmean;
}

enum { IP_PCHIP = 0, IP_NEAREST, IP_NEAREST_UP, IP_PREVIOUS, IP_NEXT, IP_ZERO, IP_SLINEAR, IP_KINDS };

template <int KIND>
__global__ __launch_bounds__(kIpThreads) void ip_eval_kernel(const double* __restrict__ x, int64_t n_max, int64_t x_stride,
                                                             const int64_t* __restrict__ counts, double* __restrict__ y,
                                                             int64_t y_stride, int32_t nseg,
                                                             const int4* __restrict__ carry,
                                                             const int4* __restrict__ rowinfo) {
#pragma clang fp contract(off)
  __shared__ uint64_t s_m[kIpWords];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int64_t base = seg * kIpSeg;
  const int64_t n = ip_row_count(counts, row, n_max);         // "the last sample" below is n - 1 of this row
  const double* xr = x + row * x_stride;
  double* yr = y + row * y_stride;
  double v[kIpPer];
  ip_load_segment(xr, n, base, v, s_m);
  const int4 cr = carry[blockIdx.x];
  const int4 ri = rowinfo[row];
  const int64_t F1 = ri.x, F2 = ri.y, L2 = ri.z, L1 = ri.w;
  const int64_t need2 = KIND == IP_SLINEAR ? F2 : F1;   // fewer valid samples than the kind needs: copied (the host raises)

  // the valid sample before / after sample k, k in this segment or the nearest valid one outside it
  auto prev_valid = [&](int64_t k) -> int64_t {
    if (k < base) return cr.y;
    const int l = ip_seg_prev(s_m, (int)(k - base));
    return l >= 0 ? base + l : (int64_t)cr.x;
  };
  auto next_valid = [&](int64_t k) -> int64_t {
    if (k >= base + kIpSeg) return cr.w;
    const int l = ip_seg_next(s_m, (int)(k - base));
    return l >= 0 ? base + l : (int64_t)cr.z;
  };

#pragma unroll
  for (int k = 0; k < kIpPer; ++k) {
    const int64_t i = base + k * kIpThreads + threadIdx.x;
    if (i >= n) {
      if (i < n_max) yr[i] = 0.0;                             // behind the row's count
      continue;
    }
    if (v[k] == v[k] || need2 < 0) { yr[i] = v[k]; continue; }
    const int64_t k1 = prev_valid(i), k2 = next_valid(i);
    double r;
    if constexpr (KIND == IP_NEAREST || KIND == IP_NEAREST_UP) {
      bool right;
      if (k1 < 0) right = true;
      else if (k2 < 0) right = false;
      else right = KIND == IP_NEAREST ? (k2 - i < i - k1) : (k2 - i <= i - k1);
      r = xr[right ? k2 : k1];
    } else if constexpr (KIND == IP_PREVIOUS) {
      r = k1 < 0 ? NAN : xr[k1];
    } else if constexpr (KIND == IP_NEXT) {
      r = k2 < 0 ? NAN : xr[k2];
    } else if constexpr (KIND == IP_ZERO) {
      r = xr[k1 < 0 ? F1 : k1];
    } else if constexpr (KIND == IP_SLINEAR) {
      int64_t lo, hi;
      if (k1 < 0) { lo = F1; hi = F2; }
      else if (k2 < 0) { lo = L2; hi = L1; }
      else { lo = k1; hi = k2; }
      const double ylo = xr[lo], yhi = xr[hi];
      const double slope = (yhi - ylo) / ((double)hi - (double)lo);
      r = slope * ((double)i - (double)lo) + ylo;
    } else {
      // pchip: the reference's end fix makes samples 0 and n - 1 knots (with the first / last valid value) when they are NaN
      auto val = [&](int64_t q) -> double { return xr[q < F1 ? F1 : (q > L1 ? L1 : q)]; };
      if (i == 0 || i == n - 1) {
        r = val(i);
      } else {
        const int64_t q1 = k1 < 0 ? 0 : k1, q2 = k2 < 0 ? n - 1 : k2;
        int64_t q0 = -1, q3 = -1;                       // the knot before q1, the knot after q2
        if (q1 > 0) { q0 = prev_valid(q1); if (q0 < 0) q0 = 0; }
        if (q2 < n - 1) { q3 = next_valid(q2); if (q3 < 0) q3 = n - 1; }
        const double y1 = val(q1), y2 = val(q2);
        const double h = (double)q2 - (double)q1;
        const double m = (y2 - y1) / h;
        double h0 = 0.0, m0 = 0.0, h3 = 0.0, m3 = 0.0;
        if (q0 >= 0) { h0 = (double)q1 - (double)q0; m0 = (y1 - val(q0)) / h0; }
        if (q3 >= 0) { h3 = (double)q3 - (double)q2; m3 = (val(q3) - y2) / h3; }
        double d1, d2;
        if (q0 < 0) d1 = q3 < 0 ? m : ip_pchip_edge(h, h3, m, m3);
        else d1 = ip_pchip_inner(h0, h, m0, m);
        if (q3 < 0) d2 = q0 < 0 ? m : ip_pchip_edge(h, h0, m, m0);
        else d2 = ip_pchip_inner(h, h3, m, m3);
        // CubicHermiteSpline's power-basis coefficients, PPoly's evaluation: c3 + c2 s + c1 s^2 + c0 s^3
        const double t = (d1 + d2 - 2.0 * m) / h;
        const double c0 = t / h, c1 = (m - d1) / h - t;
        const double s = (double)i - (double)q1;
        double z = s;
        r = y1 + d1 * z;
        z *= s;
        r = r + c1 * z;
        z *= s;
        r = r + c0 * z;
      }
    }
    yr[i] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// interp_NAN(method='linear'): scipy.interpolate.interp1d(valid idx, valid values, 'linear', fill_value='extrapolate')
// at the NaN positions -- slope = (y_hi - y_lo) / (x_hi - x_lo), y = slope * (x - x_lo) + y_lo with (lo, hi) the
// neighbouring valid samples inside, the first two / last two valid samples beyond the ends.  A workgroup per row;
// thread t walks the contiguous segment t, with the valid neighbours of its segment from a scan of per-segment ends.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kInterpThreads = 256;

// counts (or nullptr): row b is the curve of its first c_b = clamp(counts[b], 1, n_max) samples -- whatever lies behind
// is no sample of it, and columns [c_b, n_max) of the output are 0.
__global__ __launch_bounds__(kInterpThreads) void interp_linear_kernel(const double* __restrict__ x, int64_t n_max,
                                                                       int64_t stride, const int64_t* __restrict__ counts,
                                                                       double* __restrict__ y, int64_t y_stride) {
#pragma clang fp contract(off)
  __shared__ int64_t s_first[kInterpThreads][2], s_last[kInterpThreads][2];
  __shared__ int64_t s_ends[4];
  const double* xr = x + blockIdx.x * stride;
  double* yr = y + blockIdx.x * y_stride;
  const int t = threadIdx.x;
  const int64_t n = counts ? min<int64_t>(max<int64_t>(counts[blockIdx.x], 1), n_max) : n_max;
  for (int64_t i = n + t; i < n_max; i += kInterpThreads) yr[i] = 0.0;
  const int64_t L = (n + kInterpThreads - 1) / kInterpThreads;
  const int64_t b = min<int64_t>(n, t * L), e = min<int64_t>(n, b + L);
  int64_t f1 = -1, f2 = -1, l1 = -1, l2 = -1;     // first two / last two valid samples of the segment
  for (int64_t i = b; i < e; ++i) {
    if (!isnan(xr[i])) {
      if (f1 < 0) f1 = i; else if (f2 < 0) f2 = i;
      l2 = l1; l1 = i;
    }
  }
  s_first[t][0] = f1; s_first[t][1] = f2; s_last[t][0] = l1; s_last[t][1] = l2;
  __syncthreads();
  if (t == 0) {
    int64_t a0 = -1, a1 = -1, z0 = -1, z1 = -1;
    for (int s = 0; s < kInterpThreads && a1 < 0; ++s)
      for (int q = 0; q < 2; ++q) {
        const int64_t v = s_first[s][q];
        if (v >= 0 && a1 < 0) { if (a0 < 0) a0 = v; else if (v != a0) a1 = v; }
      }
    for (int s = kInterpThreads - 1; s >= 0 && z1 < 0; --s)
      for (int q = 0; q < 2; ++q) {
        const int64_t v = s_last[s][q];
        if (v >= 0 && z1 < 0) { if (z0 < 0) z0 = v; else if (v != z0) z1 = v; }
      }
    s_ends[0] = a0; s_ends[1] = a1; s_ends[2] = z1; s_ends[3] = z0;
  }
  __syncthreads();
  const int64_t a0 = s_ends[0], a1 = s_ends[1], z1 = s_ends[2], z0 = s_ends[3];
  if (a1 < 0) {                                   // fewer than two valid samples: scipy raises; the host checks first
    for (int64_t i = b; i < e; ++i) yr[i] = xr[i];
    return;
  }
  int64_t p = -1;                                 // last valid sample before the segment
  for (int s = t - 1; s >= 0 && p < 0; --s) p = s_last[s][0];
  int64_t q = -1;                                 // next valid sample at or after i (searched once per NaN run)
  for (int64_t i = b; i < e; ++i) {
    const double v = xr[i];
    if (!isnan(v)) { yr[i] = v; p = i; continue; }
    if (q <= i) {
      q = -1;
      for (int64_t k = i + 1; k < e && q < 0; ++k) if (!isnan(xr[k])) q = k;
      for (int s = t + 1; s < kInterpThreads && q < 0; ++s) q = s_first[s][0];
      if (q < 0) q = n;                           // none: extrapolation from the last two
    }
    int64_t lo_i, hi_i;
    if (p < 0) { lo_i = a0; hi_i = a1; }
    else if (q >= n) { lo_i = z1; hi_i = z0; }
    else { lo_i = p; hi_i = q; }
    const double ylo = xr[lo_i], yhi = xr[hi_i];
    const double slope = (yhi - ylo) / ((double)hi_i - (double)lo_i);
    yr[i] = slope * ((double)i - (double)lo_i) + ylo;
  }
}

// out[j][c] = interp1d(t_in, y[:, c], 'linear')(t_out[j]) with y float32: scipy's searchsorted index clipped to [1, n - 1],
// the float32 difference of the two samples over the float64 step, slope * (t - t_lo) + y_lo in float64
__global__ __launch_bounds__(kIpThreads) void regrid_linear_kernel(const float* __restrict__ yv, int64_t n, int64_t cols,
                                                                   int64_t y_stride, const double* __restrict__ t_in,
                                                                   const double* __restrict__ t_out, int64_t m,
                                                                   double* __restrict__ out, int64_t out_stride) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * kIpThreads + threadIdx.x;
  if (e >= m * cols) return;
  const int64_t j = e / cols, c = e - j * cols;
  const double t = t_out[j];
  int64_t lo = 0, hi = n;                               // first index with t_in[index] >= t
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (t_in[mid] < t) lo = mid + 1; else hi = mid;
  }
  const int64_t ih = lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo), il = ih - 1;
  const double t_lo = t_in[il], t_hi = t_in[ih];
  const float y_lo = yv[il * y_stride + c], y_hi = yv[ih * y_stride + c];
  const float dy = y_hi - y_lo;
  const double slope = (double)dy / (t_hi - t_lo);
  out[j * out_stride + c] = slope * (t - t_lo) + (double)y_lo;
}

template <int KIND>
void ip_launch_eval(unsigned blocks, hipStream_t st, const double* d_x, int64_t n, int64_t x_stride, const int64_t* d_counts,
                    double* d_y, int64_t y_stride, int32_t nseg, const int4* carry, const int4* rowinfo) {
  hipLaunchKernelGGL(ip_eval_kernel<KIND>, dim3(blocks), dim3(kIpThreads), 0, st, d_x, n, x_stride, d_counts, d_y, y_stride,
                     nseg, carry, rowinfo);
}

int ip_run(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_counts, double* d_y,
           int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (kind < 0 || kind >= IP_KINDS || !ip_shape_ok(rows, n) || !d_x || !d_y || !d_ws || x_stride < n || y_stride < n)
    return MM_ERR_INVALID_ARG;
  const int64_t nseg = ip_nseg(n);
  if (ws_bytes < mm_interp_nan_workspace_bytes(kind, rows, n)) return MM_ERR_WORKSPACE;
  char* w = (char*)d_ws;
  int4* summary = (int4*)w;  w += ip_align((size_t)rows * nseg * sizeof(int4));
  int4* carry = (int4*)w;    w += ip_align((size_t)rows * nseg * sizeof(int4));
  int4* rowinfo = (int4*)w;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(rows * nseg);
  hipLaunchKernelGGL(ip_summary_kernel, dim3(blocks), dim3(kIpThreads), 0, st, d_x, n, x_stride, d_counts, (int32_t)nseg,
                     summary);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ip_scan_kernel, dim3((unsigned)rows), dim3(64), 0, st, summary, (int32_t)nseg, carry, rowinfo);
  HIP_TRY(hipGetLastError());
#define IP_EVAL(K) ip_launch_eval<K>(blocks, st, d_x, n, x_stride, d_counts, d_y, y_stride, (int32_t)nseg, carry, rowinfo)
  switch (kind) {
    case IP_PCHIP:      IP_EVAL(IP_PCHIP); break;
    case IP_NEAREST:    IP_EVAL(IP_NEAREST); break;
    case IP_NEAREST_UP: IP_EVAL(IP_NEAREST_UP); break;
    case IP_PREVIOUS:   IP_EVAL(IP_PREVIOUS); break;
    case IP_NEXT:       IP_EVAL(IP_NEXT); break;
    case IP_ZERO:       IP_EVAL(IP_ZERO); break;
    default:            IP_EVAL(IP_SLINEAR); break;
  }
#undef IP_EVAL
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // namespace

extern "C" {

size_t mm_interp_nan_workspace_bytes(int32_t kind, int64_t rows, int64_t n) {
  if (kind < 0 || kind >= IP_KINDS || !ip_shape_ok(rows, n)) return 0;
  const int64_t nseg = ip_nseg(n);
  return 2 * ip_align((size_t)rows * nseg * sizeof(int4)) + ip_align((size_t)rows * sizeof(int4));
}

int mm_interp_nan_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y,
                      int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return ip_run(kind, d_x, rows, n, x_stride, nullptr, d_y, y_stride, d_ws, ws_bytes, stream);
}

int mm_interp_nan_ragged_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                             const int64_t* d_counts, double* d_y, int64_t y_stride, void* d_ws, size_t ws_bytes,
                             void* stream) {
  if (!d_counts) return MM_ERR_INVALID_ARG;
  return ip_run(kind, d_x, rows, n_max, x_stride, d_counts, d_y, y_stride, d_ws, ws_bytes, stream);
}

int mm_interp_nan_linear_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y, int64_t y_stride,
                             void* stream) {
  if (!d_x || !d_y || rows < 1 || rows > 0x7fffffff || n < 1 || x_stride < n || y_stride < n) return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(interp_linear_kernel, dim3((unsigned)rows), dim3(kInterpThreads), 0, (hipStream_t)stream, d_x, n,
                     x_stride, (const int64_t*)nullptr, d_y, y_stride);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

int mm_interp_nan_linear_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                                    const int64_t* d_counts, double* d_y, int64_t y_stride, void* stream) {
  if (!d_x || !d_y || !d_counts || rows < 1 || rows > 0x7fffffff || n_max < 1 || x_stride < n_max || y_stride < n_max)
    return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(interp_linear_kernel, dim3((unsigned)rows), dim3(kInterpThreads), 0, (hipStream_t)stream, d_x, n_max,
                     x_stride, d_counts, d_y, y_stride);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

int mm_regrid_linear_f32_f64(const float* d_y, int64_t n, int64_t cols, int64_t y_stride, const double* d_t_in,
                             const double* d_t_out, int64_t m, double* d_out, int64_t out_stride, void* stream) {
  if (!d_y || !d_t_in || !d_t_out || !d_out || n < 2 || cols < 1 || y_stride < cols || m < 1 || out_stride < cols)
    return MM_ERR_INVALID_ARG;
  if (m > ((int64_t)0x7fffffff * kIpThreads) / cols) return MM_ERR_INVALID_ARG;
  const int64_t blocks = (m * cols + kIpThreads - 1) / kIpThreads;
  hipLaunchKernelGGL(regrid_linear_kernel, dim3((unsigned)blocks), dim3(kIpThreads), 0, (hipStream_t)stream, d_y, n, cols,
                     y_stride, d_t_in, d_t_out, m, d_out, out_stride);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
