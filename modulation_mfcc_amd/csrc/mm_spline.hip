// libmodmfcc: interp_NAN's 'quadratic' and 'cubic' kinds (script/calc.py:379, scipy.interpolate.interp1d -> make_interp_spline
// with k = 2 / 3), the two that need a solve over all valid samples of a row.  gfx950 only; its C ABI is in
// include/modmfcc_spline.h.  float64 throughout, compiled without contraction.  DESIGN.md section 15.
//
// The valid samples of a row are the data points (x_j, y_j), j < K; h_j = x_{j+1} - x_j, dl_j = (y_{j+1} - y_j) / h_j.
// Either spline is written with one unknown per interior data point j = 1 .. K-2 and a tridiagonal, strictly diagonally
// dominant system (unpivoted elimination is stable):
//   cubic      the second derivatives M_j:  h_{j-1} M_{j-1} + 2 (h_{j-1} + h_j) M_j + h_j M_{j+1} = 6 (dl_j - dl_{j-1}),
//              the not-a-knot conditions (M_1 - M_0) / h_0 = (M_2 - M_1) / h_1 and its mirror image folded into rows 1
//              and K-2:  (h_0 + 2 h_1) M_1 + (h_1 - h_0) M_2 = 6 (dl_1 - dl_0) h_1 / (h_0 + h_1)
//   quadratic  the first derivatives m_j.  The piece around x_j is  y_j + m_j s + c_j s^2,  s = t - x_j; it ends at the
//              midpoints to either side (the knots of scipy's k = 2 spline), the pieces of x_1 and x_{K-2} reach over x_0 /
//              x_{K-1}.  Continuity of value and slope at the midpoint of interval j gives c_j and c_{j+1} from m_j, m_{j+1};
//              that both intervals beside x_j give the same c_j is the equation
//                 m_{j-1} / h_{j-1} + 3 m_j (1 / h_{j-1} + 1 / h_j) + m_{j+1} / h_j = 4 (dl_{j-1} / h_{j-1} + dl_j / h_j)
//              (halved below); an end interval has no knot: its side of the row is  m_j / h = dl / h.
// The kernels:
//   sp_count_kernel     a workgroup per segment of kIpSeg samples: the number of valid samples of the segment
//   sp_scan_kernel      a wave per row: the exclusive scan of these numbers (the rank of a segment's first valid sample), K
//   sp_knots_kernel     a workgroup per segment: every valid sample's rank from the scan and the segment's ballots, its
//                       index and value to the compacted lists
//   sp_solve_kernel     a workgroup per chunk of kSpChunk unknowns: builds the chunk's rows of the system and solves them by
//                       parallel cyclic reduction in LDS.  A row of one chunk is done.  With more chunks the coupling to the
//                       neighbouring chunks is cut and three right-hand sides are solved at once: the chunk's own and the
//                       two spikes (the response to the last unknown before and the first one behind the chunk)
//   sp_reduce_kernel    a wave per row with more than one chunk: the 2 x 2 block tridiagonal system of the unknowns beside
//                       the chunk borders (forward elimination and back-substitution over the borders, the coefficients
//                       staged 64 borders at a time by the wave)
//   sp_back_kernel      a workgroup per chunk: own solution minus the spikes times the two neighbouring unknowns
//   sp_eval_kernel      a workgroup per segment: a NaN sample's interval is the rank of its previous valid sample, clamped
//                       into the first / last interval (extrapolation); evaluates the piece
// Chunks are cut by rank, not by position: a row's arithmetic depends on its own samples only.
#include "mm_common.h"
#include "../../include/modmfcc_spline.h"

#include "mm_interp_seg.hip.inc"

namespace {

constexpr int kSpChunk = 1024;                          // unknowns per chunk = workgroup (interp.SPLINE_CHUNK)
constexpr int kSpPer = kSpChunk / kIpThreads;           // rows of the system per thread
static_assert(kSpChunk <= kIpSeg, "the chunks of a row must not outnumber its segments (grid limit)");

// does the row get a spline?  K valid samples of cnt: at least kind + 1 of them and a NaN to fill
__device__ __forceinline__ bool sp_fills(int kind, int32_t K, int64_t cnt) { return K > kind && K < cnt; }

__global__ __launch_bounds__(kIpThreads) void sp_count_kernel(const double* __restrict__ x, int64_t n_max, int64_t x_stride,
                                                              const int64_t* __restrict__ counts, int32_t nseg,
                                                              int32_t* __restrict__ segoff) {
  __shared__ uint64_t s_m[kIpWords];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int64_t n = ip_row_count(counts, row, n_max);
  double v[kIpPer];
  ip_load_segment(x + row * x_stride, n, seg * kIpSeg, v, s_m);
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kIpWords; ++w) c += __popcll(s_m[w]);
    segoff[blockIdx.x] = c;
  }
}

// in place: the number of valid samples of every segment -> the number before it; rowK[row] = the number in the row
__global__ __launch_bounds__(64) void sp_scan_kernel(int32_t* __restrict__ segoff, int32_t nseg, int32_t* __restrict__ rowK) {
  const int64_t row = blockIdx.x;
  int32_t* so = segoff + row * nseg;
  const int lane = threadIdx.x;
  int32_t run = 0;
  for (int32_t c = 0; c < nseg; c += 64) {
    const int32_t s = c + lane;
    const int32_t own = s < nseg ? so[s] : 0;
    int32_t incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t p = __shfl_up(incl, o, 64);
      if (lane >= o) incl += p;
    }
    if (s < nseg) so[s] = run + incl - own;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) rowK[row] = run;
}

// the number of valid samples of the segment before local index l; s_pre[w] = the number before ballot w
__device__ __forceinline__ int sp_seg_rank(const uint64_t* s_m, const int32_t* s_pre, int l) {
  return s_pre[l >> 6] + __popcll(s_m[l >> 6] & ((1ull << (l & 63)) - 1ull));
}
__device__ __forceinline__ void sp_word_prefix(const uint64_t* s_m, int32_t* s_pre) {
  if (threadIdx.x < kIpWords) {
    int c = 0;
    for (int w = 0; w < (int)threadIdx.x; ++w) c += __popcll(s_m[w]);
    s_pre[threadIdx.x] = c;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kIpThreads) void sp_knots_kernel(int kind, const double* __restrict__ x, int64_t n_max,
                                                              int64_t x_stride, const int64_t* __restrict__ counts,
                                                              int32_t nseg, const int32_t* __restrict__ segoff,
                                                              const int32_t* __restrict__ rowK, int32_t* __restrict__ kpos,
                                                              double* __restrict__ kval) {
  __shared__ uint64_t s_m[kIpWords];
  __shared__ int32_t s_pre[kIpWords];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int64_t base = seg * kIpSeg;
  const int64_t n = ip_row_count(counts, row, n_max);
  if (!sp_fills(kind, rowK[row], n)) return;            // (uniform over the workgroup)
  double v[kIpPer];
  ip_load_segment(x + row * x_stride, n, base, v, s_m);
  sp_word_prefix(s_m, s_pre);
  const int64_t off = row * n_max + segoff[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kIpPer; ++k) {
    const int l = k * kIpThreads + threadIdx.x;
    if (v[k] == v[k]) {                                 // rank < K <= n <= n_max: inside the row's part of the lists
      const int64_t r = off + sp_seg_rank(s_m, s_pre, l);
      kpos[r] = (int32_t)(base + l);
      kval[r] = v[k];
    }
  }
}

// Row j (1 <= j <= K-2) of the system: lo x_{j-1} + di x_j + up x_{j+1} = rh
template <int KIND>
__device__ __forceinline__ void sp_system_row(const int32_t* __restrict__ pos, const double* __restrict__ val, int32_t j,
                                              int32_t K, double& lo, double& di, double& up, double& rh) {
#pragma clang fp contract(off)
  const double hl = (double)(pos[j] - pos[j - 1]), hr = (double)(pos[j + 1] - pos[j]);
  const double y = val[j];
  const double dl = (y - val[j - 1]) / hl, dr = (val[j + 1] - y) / hr;
  if constexpr (KIND == MM_SPLINE_CUBIC) {
    lo = hl; di = 2.0 * (hl + hr); up = hr; rh = 6.0 * (dr - dl);
    if (j == 1) { lo = 0.0; di = hl + 2.0 * hr; up = hr - hl; rh = hr * rh / (hl + hr); }
    else if (j == K - 2) { up = 0.0; di = hr + 2.0 * hl; lo = hl - hr; rh = hl * rh / (hl + hr); }
  } else {
    double bl, br, rl, rr;
    if (j == 1) { lo = 0.0; bl = 1.0 / hl; rl = dl / hl; }
    else { lo = 0.5 / hl; bl = 1.5 / hl; rl = 2.0 * dl / hl; }
    if (j == K - 2) { up = 0.0; br = 1.0 / hr; rr = dr / hr; }
    else { up = 0.5 / hr; br = 1.5 / hr; rr = 2.0 * dr / hr; }
    di = bl + br;
    rh = rl + rr;
  }
}

// A workgroup per chunk.  MULTI: rows may have more than one chunk (three right-hand sides); otherwise every row is one chunk.
template <int KIND, bool MULTI>
__global__ __launch_bounds__(kIpThreads) void sp_solve_kernel(int64_t n_max, const int64_t* __restrict__ counts, int32_t nchunk,
                                                              const int32_t* __restrict__ rowK,
                                                              const int32_t* __restrict__ kpos, const double* __restrict__ kval,
                                                              double* __restrict__ sol, double* __restrict__ spl,
                                                              double* __restrict__ spr) {
#pragma clang fp contract(off)
  constexpr int NR = MULTI ? 3 : 1;                     // right-hand sides
  __shared__ double s_a[kSpChunk], s_b[kSpChunk], s_c[kSpChunk], s_d[NR][kSpChunk];
  const int64_t row = blockIdx.x / nchunk;
  const int32_t chunk = blockIdx.x % nchunk;
  const int32_t K = rowK[row];
  if (!sp_fills(KIND, K, ip_row_count(counts, row, n_max))) return;
  const int32_t U = K - 2, u0 = chunk * kSpChunk;       // the unknowns of the row, the first one of this chunk
  if (u0 >= U) return;
  const int32_t m = min(U - u0, kSpChunk);
  const int32_t* pos = kpos + row * n_max;
  const double* val = kval + row * n_max;

  double a[kSpPer], b[kSpPer], c[kSpPer], d[NR][kSpPer];
#pragma unroll
  for (int q = 0; q < kSpPer; ++q) {
    const int r = q * kIpThreads + threadIdx.x;
    a[q] = 0.0; b[q] = 1.0; c[q] = 0.0;                 // behind the chunk's unknowns: identity rows
#pragma unroll
    for (int e = 0; e < NR; ++e) d[e][q] = 0.0;
    if (r < m) {
      sp_system_row<KIND>(pos, val, u0 + r + 1, K, a[q], b[q], c[q], d[0][q]);
      if constexpr (MULTI) {                            // cut the coupling to the neighbouring chunks: the spikes' right-hand sides
        if (r == 0) { d[1][q] = a[q]; a[q] = 0.0; }
        if (r == m - 1) { d[2][q] = c[q]; c[q] = 0.0; }
      }
    }
  }
  // parallel cyclic reduction: after the step of stride s, row i couples to rows i - 2 s and i + 2 s only
  for (int s = 1; s < m; s <<= 1) {
#pragma unroll
    for (int q = 0; q < kSpPer; ++q) {
      const int r = q * kIpThreads + threadIdx.x;
      s_a[r] = a[q]; s_b[r] = b[q]; s_c[r] = c[q];
#pragma unroll
      for (int e = 0; e < NR; ++e) s_d[e][r] = d[e][q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSpPer; ++q) {
      const int r = q * kIpThreads + threadIdx.x;
      const int p = r - s, t = r + s;
      double k1 = 0.0, k2 = 0.0, na = 0.0, nc = 0.0;
      if (p >= 0) {
        k1 = a[q] / s_b[p];
        na = -(s_a[p] * k1);
        b[q] = b[q] - s_c[p] * k1;
#pragma unroll
        for (int e = 0; e < NR; ++e) d[e][q] = d[e][q] - s_d[e][p] * k1;
      }
      if (t < kSpChunk) {
        k2 = c[q] / s_b[t];
        nc = -(s_c[t] * k2);
        b[q] = b[q] - s_a[t] * k2;
#pragma unroll
        for (int e = 0; e < NR; ++e) d[e][q] = d[e][q] - s_d[e][t] * k2;
      }
      a[q] = na; c[q] = nc;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kSpPer; ++q) {
    const int r = q * kIpThreads + threadIdx.x;
    if (r < m) {
      const int64_t o = row * n_max + u0 + r + 1;       // indexed by data point: <= K - 2
      sol[o] = d[0][q] / b[q];
      if constexpr (MULTI) { spl[o] = d[1][q] / b[q]; spr[o] = d[2][q] / b[q]; }
    }
  }
}

// The unknowns beside the border k (between chunk k-1 and chunk k, k = 1 .. nch-1) are z_k = (l, f): the last one of chunk
// k-1 and the first one of chunk k.  With v, w, u the chunk's own solution and its left / right spike at these two places:
//    l + wl l' + ul f = vl     (l' = the l of border k-1)            f + wf l + uf f'' = vf     (f'' = the f of border k+1)
// a block tridiagonal system whose diagonal blocks stay [[1, p], [q, 1]] under elimination.  red[row][k] = (p, g) of the
// eliminated first equation; ext[row][chunk] = (the unknown before the chunk, the unknown behind it), 0 outside the row.
__global__ __launch_bounds__(64) void sp_reduce_kernel(int kind, int64_t n_max, const int64_t* __restrict__ counts,
                                                       int32_t nchunk, const int32_t* __restrict__ rowK,
                                                       const double* __restrict__ sol, const double* __restrict__ spl,
                                                       const double* __restrict__ spr, double2* __restrict__ red,
                                                       double2* __restrict__ ext) {
#pragma clang fp contract(off)
  __shared__ double s_v[2][64], s_w[2][64], s_u[2][64], s_p[64], s_g[64];
  const int64_t row = blockIdx.x;
  const int32_t K = rowK[row];
  if (!sp_fills(kind, K, ip_row_count(counts, row, n_max))) return;
  const int32_t nch = (K - 2 + kSpChunk - 1) / kSpChunk;
  if (nch < 2) return;
  const int lane = threadIdx.x;
  const double* v = sol + row * n_max;
  const double* w = spl + row * n_max;
  const double* u = spr + row * n_max;
  double2* rd = red + (int64_t)row * nchunk;
  double2* ex = ext + (int64_t)row * nchunk;
  // side 0 = the last unknown of chunk k-1 (data point k * kSpChunk), side 1 = the first one of chunk k (the next)
  auto stage = [&](int32_t k) {
    if (k >= 1 && k < nch) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int64_t o = (int64_t)k * kSpChunk + e;
        s_v[e][lane] = v[o]; s_w[e][lane] = w[o]; s_u[e][lane] = u[o];
      }
    }
  };
  double p_prev = 0.0, g_prev = 0.0, q_prev = 0.0, vf_prev = 0.0, uf_prev = 0.0;
  for (int32_t k0 = 1; k0 < nch; k0 += 64) {            // forward
    stage(k0 + lane);
    wave_lds_sync();
    if (lane == 0) {
      const int cnt = min(64, nch - k0);
      for (int i = 0; i < cnt; ++i) {
        double p = s_u[0][i], g = s_v[0][i];
        if (k0 + i > 1) {                               // eliminate the l of the border before
          const double t = s_w[0][i] / (1.0 - p_prev * q_prev);
          g = g - t * (g_prev - p_prev * vf_prev);
          p = p + t * p_prev * uf_prev;
        }
        s_p[i] = p; s_g[i] = g;
        p_prev = p; g_prev = g; q_prev = s_w[1][i]; vf_prev = s_v[1][i]; uf_prev = s_u[1][i];
      }
    }
    wave_lds_sync();
    if (k0 + lane < nch) rd[k0 + lane] = make_double2(s_p[lane], s_g[lane]);
    wave_lds_sync();
  }
  double f_next = 0.0;                                  // the f of the border behind (none behind the last)
  const int32_t last0 = 1 + ((nch - 2) / 64) * 64;
  for (int32_t k0 = last0; k0 >= 1; k0 -= 64) {         // backward
    stage(k0 + lane);
    if (k0 + lane < nch) { const double2 t = rd[k0 + lane]; s_p[lane] = t.x; s_g[lane] = t.y; }
    wave_lds_sync();
    if (lane == 0) {
      const int cnt = min(64, nch - k0);
      for (int i = cnt - 1; i >= 0; --i) {
        const double p = s_p[i], q = s_w[1][i];
        const double r0 = s_g[i], r1 = s_v[1][i] - s_u[1][i] * f_next;
        const double det = 1.0 - p * q;
        const double l = (r0 - p * r1) / det, f = (r1 - q * r0) / det;
        s_p[i] = l; s_g[i] = f;                         // reused: the border's two unknowns
        f_next = f;
      }
    }
    wave_lds_sync();
    // chunk c has border c before it (its l) and border c + 1 behind it (its f): two plain doubles per entry
    if (k0 + lane < nch) {
      double* e0 = (double*)(ex + k0 + lane);
      double* e1 = (double*)(ex + k0 + lane - 1);
      e0[0] = s_p[lane];
      e1[1] = s_g[lane];
    }
    wave_lds_sync();
  }
  if (lane == 0) { ((double*)ex)[0] = 0.0; ((double*)(ex + nch - 1))[1] = 0.0; }
}

__global__ __launch_bounds__(kIpThreads) void sp_back_kernel(int kind, int64_t n_max, const int64_t* __restrict__ counts,
                                                             int32_t nchunk, const int32_t* __restrict__ rowK,
                                                             double* __restrict__ sol, const double* __restrict__ spl,
                                                             const double* __restrict__ spr,
                                                             const double2* __restrict__ ext) {
#pragma clang fp contract(off)
  const int64_t row = blockIdx.x / nchunk;
  const int32_t chunk = blockIdx.x % nchunk;
  const int32_t K = rowK[row];
  if (!sp_fills(kind, K, ip_row_count(counts, row, n_max))) return;
  const int32_t U = K - 2, u0 = chunk * kSpChunk;
  if (U <= kSpChunk || u0 >= U) return;                 // a row of one chunk is solved already
  const int32_t m = min(U - u0, kSpChunk);
  const double2 e = ext[(int64_t)row * nchunk + chunk];
#pragma unroll
  for (int q = 0; q < kSpPer; ++q) {
    const int r = q * kIpThreads + threadIdx.x;
    if (r < m) {
      const int64_t o = row * n_max + u0 + r + 1;
      sol[o] = (sol[o] - spl[o] * e.x) - spr[o] * e.y;
    }
  }
}

// the second derivative at data point j: the solution, at the two ends the not-a-knot condition
__device__ __forceinline__ double sp_moment(const int32_t* __restrict__ pos, const double* __restrict__ M, int32_t j, int32_t K) {
#pragma clang fp contract(off)
  if (j == 0) {
    const double h0 = (double)(pos[1] - pos[0]), h1 = (double)(pos[2] - pos[1]);
    const double m1 = M[1];
    return m1 + (m1 - M[2]) * h0 / h1;
  }
  if (j == K - 1) {
    const double hl = (double)(pos[K - 1] - pos[K - 2]), hm = (double)(pos[K - 2] - pos[K - 3]);
    const double m1 = M[K - 2];
    return m1 + (m1 - M[K - 3]) * hl / hm;
  }
  return M[j];
}

template <int KIND>
__global__ __launch_bounds__(kIpThreads) void sp_eval_kernel(const double* __restrict__ x, int64_t n_max, int64_t x_stride,
                                                             const int64_t* __restrict__ counts, double* __restrict__ y,
                                                             int64_t y_stride, int32_t nseg,
                                                             const int32_t* __restrict__ segoff,
                                                             const int32_t* __restrict__ rowK,
                                                             const int32_t* __restrict__ kpos, const double* __restrict__ kval,
                                                             const double* __restrict__ sol) {
#pragma clang fp contract(off)
  __shared__ uint64_t s_m[kIpWords];
  __shared__ int32_t s_pre[kIpWords];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int64_t base = seg * kIpSeg;
  const int64_t n = ip_row_count(counts, row, n_max);
  double* yr = y + row * y_stride;
  double v[kIpPer];
  ip_load_segment(x + row * x_stride, n, base, v, s_m);
  sp_word_prefix(s_m, s_pre);
  const int32_t K = rowK[row];
  const bool fills = sp_fills(KIND, K, n);              // otherwise copied (too few valid samples: the host raises)
  const int32_t before = segoff[blockIdx.x];
  const int32_t* pos = kpos + row * n_max;
  const double* val = kval + row * n_max;
  const double* S = sol + row * n_max;
#pragma unroll
  for (int k = 0; k < kIpPer; ++k) {
    const int l = k * kIpThreads + threadIdx.x;
    const int64_t i = base + l;
    if (i >= n) {
      if (i < n_max) yr[i] = 0.0;                       // behind the row's count
      continue;
    }
    if (v[k] == v[k] || !fills) { yr[i] = v[k]; continue; }
    // the interval [x_j, x_{j+1}] the sample lies in; the first / last one for a sample outside the data
    const int32_t j = min(max(before + sp_seg_rank(s_m, s_pre, l) - 1, 0), K - 2);
    const int32_t x0 = pos[j], x1 = pos[j + 1];
    const double h = (double)(x1 - x0);
    double r;
    if constexpr (KIND == MM_SPLINE_CUBIC) {
      const double y0 = val[j], y1 = val[j + 1];
      const double M0 = sp_moment(pos, S, j, K), M1 = sp_moment(pos, S, j + 1, K);
      const double dl = (y1 - y0) / h;
      const double c3 = (M1 - M0) / (6.0 * h);
      const double s0 = (double)(i - x0), s1 = (double)(i - x1);
      if (fabs(s0) <= fabs(s1)) {                       // expanded about the nearer end of the interval
        const double c1 = dl - h * (2.0 * M0 + M1) / 6.0;
        r = y0 + s0 * (c1 + s0 * (M0 / 2.0 + s0 * c3));
      } else {
        const double c1 = dl + h * (2.0 * M1 + M0) / 6.0;
        r = y1 + s1 * (c1 + s1 * (M1 / 2.0 + s1 * c3));
      }
    } else {
      int32_t p;                                        // the data point whose piece holds the sample
      if (j == 0) p = 1;
      else if (j == K - 2) p = K - 2;
      else p = 2 * i <= (int64_t)x0 + x1 ? j : j + 1;
      const int32_t xp = pos[p];
      const double g = (double)(pos[p + 1] - xp);
      const double yp = val[p], mp = S[p];
      const double dp = (val[p + 1] - yp) / g;
      const double cp = p == K - 2 ? (dp - mp) / g : (4.0 * dp - 3.0 * mp - S[p + 1]) / (2.0 * g);
      const double s = (double)(i - xp);
      r = yp + s * (mp + s * cp);
    }
    yr[i] = r;
  }
}

int64_t sp_nchunk(int64_t n) { return (std::max<int64_t>(n - 2, 1) + kSpChunk - 1) / kSpChunk; }

bool sp_shape_ok(int32_t kind, int64_t rows, int64_t n) {
  return (kind == MM_SPLINE_QUADRATIC || kind == MM_SPLINE_CUBIC) && ip_shape_ok(rows, n);
}

template <int KIND, bool MULTI>
void sp_launch_solve(unsigned blocks, hipStream_t st, int64_t n, const int64_t* d_counts, int32_t nchunk, const int32_t* rowK,
                     const int32_t* kpos, const double* kval, double* sol, double* spl, double* spr) {
  hipLaunchKernelGGL((sp_solve_kernel<KIND, MULTI>), dim3(blocks), dim3(kIpThreads), 0, st, n, d_counts, nchunk, rowK, kpos,
                     kval, sol, spl, spr);
}

int sp_run(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_counts, double* d_y,
           int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (!sp_shape_ok(kind, rows, n) || !d_x || !d_y || !d_ws || x_stride < n || y_stride < n) return MM_ERR_INVALID_ARG;
  if (ws_bytes < mm_interp_spline_workspace_bytes(kind, rows, n)) return MM_ERR_WORKSPACE;
  const int64_t nseg = ip_nseg(n), nchunk = sp_nchunk(n);
  const bool multi = nchunk > 1;
  const size_t cells = (size_t)rows * (size_t)n;
  char* w = (char*)d_ws;
  int32_t* segoff = (int32_t*)w;  w += ip_align((size_t)rows * nseg * sizeof(int32_t));
  int32_t* rowK = (int32_t*)w;    w += ip_align((size_t)rows * sizeof(int32_t));
  int32_t* kpos = (int32_t*)w;    w += ip_align(cells * sizeof(int32_t));
  double* kval = (double*)w;      w += ip_align(cells * sizeof(double));
  double* sol = (double*)w;       w += ip_align(cells * sizeof(double));
  double *spl = nullptr, *spr = nullptr;
  double2 *red = nullptr, *ext = nullptr;
  if (multi) {
    spl = (double*)w;             w += ip_align(cells * sizeof(double));
    spr = (double*)w;             w += ip_align(cells * sizeof(double));
    red = (double2*)w;            w += ip_align((size_t)rows * nchunk * sizeof(double2));
    ext = (double2*)w;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned seg_blocks = (unsigned)(rows * nseg), chunk_blocks = (unsigned)(rows * nchunk);
  hipLaunchKernelGGL(sp_count_kernel, dim3(seg_blocks), dim3(kIpThreads), 0, st, d_x, n, x_stride, d_counts, (int32_t)nseg,
                     segoff);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sp_scan_kernel, dim3((unsigned)rows), dim3(64), 0, st, segoff, (int32_t)nseg, rowK);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(sp_knots_kernel, dim3(seg_blocks), dim3(kIpThreads), 0, st, (int)kind, d_x, n, x_stride, d_counts,
                     (int32_t)nseg, segoff, rowK, kpos, kval);
  HIP_TRY(hipGetLastError());
#define SP_SOLVE(K, M) sp_launch_solve<K, M>(chunk_blocks, st, n, d_counts, (int32_t)nchunk, rowK, kpos, kval, sol, spl, spr)
  if (kind == MM_SPLINE_CUBIC) { if (multi) SP_SOLVE(MM_SPLINE_CUBIC, true); else SP_SOLVE(MM_SPLINE_CUBIC, false); }
  else { if (multi) SP_SOLVE(MM_SPLINE_QUADRATIC, true); else SP_SOLVE(MM_SPLINE_QUADRATIC, false); }
#undef SP_SOLVE
  HIP_TRY(hipGetLastError());
  if (multi) {
    hipLaunchKernelGGL(sp_reduce_kernel, dim3((unsigned)rows), dim3(64), 0, st, (int)kind, n, d_counts, (int32_t)nchunk, rowK,
                       sol, spl, spr, red, ext);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sp_back_kernel, dim3(chunk_blocks), dim3(kIpThreads), 0, st, (int)kind, n, d_counts, (int32_t)nchunk,
                       rowK, sol, spl, spr, ext);
    HIP_TRY(hipGetLastError());
  }
  if (kind == MM_SPLINE_CUBIC)
    hipLaunchKernelGGL(sp_eval_kernel<MM_SPLINE_CUBIC>, dim3(seg_blocks), dim3(kIpThreads), 0, st, d_x, n, x_stride, d_counts,
                       d_y, y_stride, (int32_t)nseg, segoff, rowK, kpos, kval, sol);
  else
    hipLaunchKernelGGL(sp_eval_kernel<MM_SPLINE_QUADRATIC>, dim3(seg_blocks), dim3(kIpThreads), 0, st, d_x, n, x_stride,
                       d_counts, d_y, y_stride, (int32_t)nseg, segoff, rowK, kpos, kval, sol);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // namespace

extern "C" {

size_t mm_interp_spline_workspace_bytes(int32_t kind, int64_t rows, int64_t n) {
  if (!sp_shape_ok(kind, rows, n)) return 0;
  const int64_t nseg = ip_nseg(n), nchunk = sp_nchunk(n);
  const size_t cells = (size_t)rows * (size_t)n;
  size_t b = ip_align((size_t)rows * nseg * sizeof(int32_t)) + ip_align((size_t)rows * sizeof(int32_t)) +
             ip_align(cells * sizeof(int32_t)) + 2 * ip_align(cells * sizeof(double));
  if (nchunk > 1) b += 2 * ip_align(cells * sizeof(double)) + 2 * ip_align((size_t)rows * nchunk * sizeof(double2));
  return b;
}

int mm_interp_spline_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y,
                         int64_t y_stride, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_run(kind, d_x, rows, n, x_stride, nullptr, d_y, y_stride, d_ws, ws_bytes, stream);
}

int mm_interp_spline_ragged_f64(int32_t kind, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                                const int64_t* d_counts, double* d_y, int64_t y_stride, void* d_ws, size_t ws_bytes,
                                void* stream) {
  if (!d_counts) return MM_ERR_INVALID_ARG;
  return sp_run(kind, d_x, rows, n_max, x_stride, d_counts, d_y, y_stride, d_ws, ws_bytes, stream);
}

}  // extern "C"
