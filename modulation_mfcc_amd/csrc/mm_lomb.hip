// mm_lomb.hip -- the Lomb-Scargle (least-squares) modulation spectrum of curves with holes (include/modmfcc_lomb.h):
// scipy.signal.lombscargle of scipy 1.15 on the valid (non-NaN, in front of the length) samples of every row of a batch,
// in float64.  DESIGN.md section 16.
//
// The cosines and sines of omega_k t_j belong to the time axis and the frequency grid, not to the row; the row owns its
// mask m_rj and its values.  So the sums of a batch are six matrix products [rows x samples] . [samples x frequencies]:
//     C = m . cos    S = m . sin    CC = m . cos^2    CS = m . (cos sin)    YC = (m y) . cos    YS = (m y) . sin
// whose right-hand sides are generated on the fly and whose left-hand sides are two selected operands per sample.  They
// run on v_mfma_f64_16x16x4_f64: a wave owns 16 frequencies and kLsRowTiles tiles of 16 rows, a lane generates ONE
// (sample, frequency) pair per step of 4 samples (lane l: sample l >> 4, frequency l & 15 -- the B operand) and loads one
// (row, sample) pair per row tile (row l & 15, sample l >> 4 -- the A operand); four generated values feed six
// accumulations per row tile.  The accumulator of the float64 instruction is NOT laid out like the float32 ones:
// register i of lane l holds row (l >> 4) + 4 i, column l & 15.
//
// Kernels (no atomics, no LDS, no barrier):
//   ls_stat_kernel   a wave per (row, chunk of kLsChunk samples): the count of valid samples, sum y and sum y^2 (of y - mean
//                    in a second pass when MM_LOMB_PRECENTER is set, after ls_mean_kernel added the row's chunks)
//   ls_main_kernel   a workgroup of 4 waves per (chunk, 16 kLsRowTiles rows, 64 frequencies); with one chunk it runs the
//                    epilogue on its sums, otherwise it stores them
//   ls_finish_kernel a thread per (row, frequency): the chunks in ascending order, then the same epilogue
// Summation order: inside a chunk by the sample index alone (steps of 4 from the chunk's start; a masked sample adds a
// zero, which changes no sum), then the chunks ascending -- a chunk behind a row's length holds +0.0 and changes
// nothing.  So a row's bits do not depend on rows, on its place in a tile, on n_max or on the other rows.  The epilogue
// is compiled without contraction so that its two copies (main, finish) round alike.
#include "mm_common.h"
#include "../../include/modmfcc_lomb.h"

#ifndef MM_LOMB_ROW_TILES
#define MM_LOMB_ROW_TILES 1     // tiles of 16 rows a wave carries: trig per product against 6 x 8 accumulator VGPRs a tile
#endif                          // (1, 2 and 4 were timed, 1 is the fastest at every timed shape: docs/experiments.md)

namespace {

constexpr int kLsChunk = MM_LOMB_CHUNK;
constexpr int kLsRowTiles = MM_LOMB_ROW_TILES;
constexpr int kLsThreads = 256;                 // 4 waves
constexpr int kLsFreqTile = 64;                 // 16 frequencies a wave
constexpr int kLsSums = 6;                      // C, S, CC, CS, YC, YS
static_assert(kLsChunk % 64 == 0, "ls_stat_kernel strides a chunk by the wave");
static_assert(kLsRowTiles == 1 || kLsRowTiles == 2 || kLsRowTiles == 4, "row tiles a wave");

typedef double ls_f64x4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

__device__ __forceinline__ int64_t ls_row_len(const int64_t* __restrict__ lengths, int64_t row, int64_t n_max) {
  if (!lengths) return n_max;
  const int64_t l = lengths[row];
  return l < 1 ? 1 : (l > n_max ? n_max : l);
}

__device__ __forceinline__ double ls_wave_sum(double v) {      // fixed tree: the same order for every row
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// stat [rows][nchunks][3]: valid count, sum (y - mean), sum (y - mean)^2 of the chunk; mean: nullptr = 0
__global__ __launch_bounds__(kLsThreads) void ls_stat_kernel(const double* __restrict__ x, int64_t rows, int64_t n_max,
                                                              int64_t x_stride, const int64_t* __restrict__ lengths,
                                                              int64_t nchunks, const double* __restrict__ mean,
                                                              double* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * (kLsThreads / 64) + (threadIdx.x >> 6);
  if (gw >= rows * nchunks) return;
  const int64_t row = gw / nchunks, chunk = gw - row * nchunks;
  const int64_t len = ls_row_len(lengths, row, n_max);
  const double mu = mean ? mean[row] : 0.0;
  const double* __restrict__ xr = x + row * x_stride;
  double k = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int u = 0; u < kLsChunk / 64; ++u) {
    const int64_t j = chunk * kLsChunk + u * 64 + lane;
    if (j < len) {
      const double v = xr[j];
      if (v == v) {
        const double d = v - mu;
        k += 1.0;
        s1 += d;
        s2 = __builtin_fma(d, d, s2);
      }
    }
  }
  k = ls_wave_sum(k);
  s1 = ls_wave_sum(s1);
  s2 = ls_wave_sum(s2);
  if (lane == 0) {
    double* o = stat + gw * 3;
    o[0] = k;
    o[1] = s1;
    o[2] = s2;
  }
}

// the chunks of a row in ascending order: count and sums
__device__ __forceinline__ void ls_row_stat(const double* __restrict__ stat, int64_t row, int64_t nchunks, double& K,
                                            double& sy, double& syy) {
  const double* p = stat + row * nchunks * 3;
  K = p[0];
  sy = p[1];
  syy = p[2];
  for (int64_t c = 1; c < nchunks; ++c) {
    K += p[3 * c];
    sy += p[3 * c + 1];
    syy += p[3 * c + 2];
  }
}

__global__ __launch_bounds__(kLsThreads) void ls_mean_kernel(const double* __restrict__ stat, int64_t rows, int64_t nchunks,
                                                              double* __restrict__ mean) {
  const int64_t row = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
  if (row >= rows) return;
  double K, sy, syy;
  ls_row_stat(stat, row, nchunks, K, sy, syy);
  mean[row] = sy / K;        // (NaN for a row without a valid sample: that row is NaN anyway)
}

// scipy's lombscargle from the raw sums q = {sum cos, sum sin, sum cos^2, sum cos sin, sum y cos, sum y sin} over the K
// valid samples, sy = sum y, syy = sum y^2: the second pass of scipy (cos and sin of omega t - tau) is the rotation of the
// first and second moments by tau.
__device__ __forceinline__ void ls_epilogue(double K, double sy, double syy, const double (&q)[kLsSums], int flags,
                                            double* __restrict__ out, double* __restrict__ out_im) {
#pragma clang fp contract(off)
  const int norm = flags & (3 << 2);
  if (!(K >= 1.0)) {
    *out = __builtin_nan("");
    if (norm == MM_LOMB_AMPLITUDE) *out_im = __builtin_nan("");
    return;
  }
  const bool fm = (flags & MM_LOMB_FLOATING_MEAN) != 0;
  const double w = 1.0 / K;
  const double C0 = q[0] * w, S0 = q[1] * w, CC0 = q[2] * w, CS0 = q[3] * w, YC0 = q[4] * w, YS0 = q[5] * w;
  const double SS0 = 1.0 - CC0, Y = sy * w;
  double cca = CC0, ssa = SS0, csa = CS0;
  if (fm) {
    cca -= C0 * C0;
    ssa -= S0 * S0;
    csa -= C0 * S0;
  }
  const double tau = 0.5 * atan2(2.0 * csa, cca - ssa);
  double s, c;
  sincos(tau, &s, &c);
  double YC = YC0 * c + YS0 * s;
  double YS = YS0 * c - YC0 * s;
  double CC = (c * c) * CC0 + (2.0 * c * s) * CS0 + (s * s) * SS0;
  double SS = 1.0 - CC;
  if (fm) {
    const double Cr = C0 * c + S0 * s, Sr = S0 * c - C0 * s;
    YC -= Y * Cr;
    YS -= Y * Sr;
    CC -= Cr * Cr;
    SS -= Sr * Sr;
  }
  const double epsneg = 1.1102230246251565e-16;      // np.finfo(np.float64).epsneg
  if (CC < epsneg) CC = epsneg;
  if (SS < epsneg) SS = epsneg;
  const double a = YC / CC, b = YS / SS;
  double p = 2.0 * (a * YC + b * YS);
  if (norm == MM_LOMB_POWER) {
    *out = p * (K / 4.0);
  } else if (norm == MM_LOMB_NORMALIZE) {
    double YY = syy * w;
    if (fm) YY -= Y * Y;
    *out = p * (0.5 / YY);
  } else {
    *out = a * c - b * s;
    *out_im = a * s + b * c;
  }
}

// part [nchunks][6][rows][n_freq]
template <int NRT, bool DIRECT>
__global__ __launch_bounds__(kLsThreads) void ls_main_kernel(const double* __restrict__ x, int64_t rows, int64_t n_max,
                                                              int64_t x_stride, const int64_t* __restrict__ lengths,
                                                              const double* __restrict__ t, const double* __restrict__ omega,
                                                              int64_t n_freq, int flags, const double* __restrict__ mean,
                                                              const double* __restrict__ stat, double* __restrict__ part,
                                                              double* __restrict__ out, int64_t out_stride,
                                                              double* __restrict__ out_im) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = blockIdx.x;
  const int64_t f0 = ((int64_t)blockIdx.z * (kLsFreqTile / 16) + wave) * 16;
  if (f0 >= n_freq) return;                                      // (wave-uniform; the kernel has no barrier)
  const int64_t r0 = (int64_t)blockIdx.y * (16 * NRT);
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t fb = f0 + lo;
  const double om = omega[fb < n_freq ? fb : n_freq - 1];

  const double* xr[NRT];
  int64_t len[NRT];
  double mu[NRT];
#pragma unroll
  for (int i = 0; i < NRT; ++i) {
    const int64_t r = r0 + 16 * i + lo;
    const bool ok = r < rows;
    const int64_t rr = ok ? r : rows - 1;
    xr[i] = x + rr * x_stride;
    len[i] = ok ? ls_row_len(lengths, rr, n_max) : 0;            // a row behind the batch: every sample masked
    mu[i] = mean ? mean[rr] : 0.0;
  }

  ls_f64x4 acc[NRT][kLsSums];
#pragma unroll
  for (int i = 0; i < NRT; ++i)
#pragma unroll
    for (int k = 0; k < kLsSums; ++k) acc[i][k] = ls_f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t j0 = chunk * kLsChunk;
  // the longest row of the wave's tiles ends the walk: the samples behind it are masked for every row and add zeros, so
  // stopping there changes no bit (a chunk behind all 16 NRT lengths does no step and stores +0.0)
  int64_t longest = len[0];
#pragma unroll
  for (int i = 1; i < NRT; ++i) longest = len[i] > longest ? len[i] : longest;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const int64_t other = __shfl_xor(longest, o, 64);
    longest = other > longest ? other : longest;
  }
  longest = __shfl(longest, 0, 64);                              // (all four groups of 16 lanes hold it; one value a wave)
  int64_t j1 = j0 + kLsChunk < n_max ? j0 + kLsChunk : n_max;
  if (longest < j1) j1 = longest;
  // the loads of a step are issued one step ahead of their use (a workgroup has few waves to hide them behind)
  double tj = j0 + hi < n_max ? t[j0 + hi] : 0.0;
  double v[NRT];
#pragma unroll
  for (int i = 0; i < NRT; ++i) {
    v[i] = __builtin_nan("");
    if (j0 + hi < len[i]) v[i] = xr[i][j0 + hi];
  }
#pragma unroll 2
  for (int64_t jb = j0; jb < j1; jb += 4) {
    const int64_t jn = jb + 4 + hi;
    double tn = 0.0, vn[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) vn[i] = __builtin_nan("");
    if (jb + 4 < j1) {                                           // (wave-uniform)
      if (jn < n_max) tn = t[jn];
#pragma unroll
      for (int i = 0; i < NRT; ++i)
        if (jn < len[i]) vn[i] = xr[i][jn];
    }
    double s, c;
    sincos(om * tj, &s, &c);                                     // the float64 product of the two inputs, as scipy forms it
    const double cc = c * c, cs = c * s;
#pragma unroll
    for (int i = 0; i < NRT; ++i) {
      const bool valid = v[i] == v[i];                           // (a sample at or behind the length was never loaded: NaN)
      const double m = valid ? 1.0 : 0.0;
      const double my = valid ? v[i] - mu[i] : 0.0;              // selected, never NaN * 0
      acc[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(m, c, acc[i][0], 0, 0, 0);
      acc[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(m, s, acc[i][1], 0, 0, 0);
      acc[i][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(m, cc, acc[i][2], 0, 0, 0);
      acc[i][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(m, cs, acc[i][3], 0, 0, 0);
      acc[i][4] = __builtin_amdgcn_mfma_f64_16x16x4f64(my, c, acc[i][4], 0, 0, 0);
      acc[i][5] = __builtin_amdgcn_mfma_f64_16x16x4f64(my, s, acc[i][5], 0, 0, 0);
    }
    tj = tn;
#pragma unroll
    for (int i = 0; i < NRT; ++i) v[i] = vn[i];
  }

  if (fb >= n_freq) return;
#pragma unroll
  for (int i = 0; i < NRT; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t r = r0 + 16 * i + hi + 4 * g;                // C/D layout of the float64 MFMA
      if (r >= rows) continue;
      if (DIRECT) {
        const double q[kLsSums] = {acc[i][0][g], acc[i][1][g], acc[i][2][g], acc[i][3][g], acc[i][4][g], acc[i][5][g]};
        ls_epilogue(stat[r * 3], stat[r * 3 + 1], stat[r * 3 + 2], q, flags, out + r * out_stride + fb,
                    out_im ? out_im + r * out_stride + fb : nullptr);
      } else {
#pragma unroll
        for (int k = 0; k < kLsSums; ++k) part[((chunk * kLsSums + k) * rows + r) * n_freq + fb] = acc[i][k][g];
      }
    }
}

__global__ __launch_bounds__(kLsThreads) void ls_finish_kernel(const double* __restrict__ part, const double* __restrict__ stat,
                                                                int64_t rows, int64_t n_freq, int64_t nchunks, int flags,
                                                                double* __restrict__ out, int64_t out_stride,
                                                                double* __restrict__ out_im) {
  const int64_t idx = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
  if (idx >= rows * n_freq) return;
  const int64_t r = idx / n_freq, f = idx - r * n_freq;
  const int64_t plane = rows * n_freq;
  const double* p = part + idx;
  double q[kLsSums];
#pragma unroll
  for (int k = 0; k < kLsSums; ++k) q[k] = p[k * plane];
#pragma unroll 4      // (16 was timed: five times slower, docs/experiments.md)
  for (int64_t c = 1; c < nchunks; ++c) {                        // ascending, every sum on its own
#pragma unroll
    for (int k = 0; k < kLsSums; ++k) q[k] += p[(c * kLsSums + k) * plane];
  }
  double K, sy, syy;
  ls_row_stat(stat, r, nchunks, K, sy, syy);
  ls_epilogue(K, sy, syy, q, flags, out + r * out_stride + f, out_im ? out_im + r * out_stride + f : nullptr);
}

bool ls_shape_ok(int64_t rows, int64_t n_max, int64_t n_freq) {
  if (rows < 1 || rows > ((int64_t)1 << 19) || n_max < 1 || n_max > ((int64_t)1 << 30) || n_freq < 1 ||
      n_freq > ((int64_t)1 << 20))
    return false;
  const int64_t nchunks = (n_max + kLsChunk - 1) / kLsChunk;
  // a launch takes fewer than 2^32 threads a dimension: 64 threads per (row, chunk) in ls_stat_kernel, one per (row, frequency)
  // in ls_finish_kernel -- refused here, before any launch
  return rows * nchunks < ((int64_t)1 << 26) && rows * n_freq < ((int64_t)1 << 32);
}

}  // namespace

extern "C" {

int mm_lomb_version(void) { return MM_LOMB_VERSION; }

size_t mm_lombscargle_workspace_bytes(int64_t rows, int64_t n_max, int64_t n_freq) {
  if (!ls_shape_ok(rows, n_max, n_freq)) return 0;
  const int64_t nchunks = (n_max + kLsChunk - 1) / kLsChunk;
  size_t b = align_up((size_t)rows * nchunks * 3 * sizeof(double), 256) + align_up((size_t)rows * sizeof(double), 256);
  if (nchunks > 1) b += align_up((size_t)nchunks * kLsSums * rows * n_freq * sizeof(double), 256);
  return b;
}

int mm_lombscargle_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lengths,
                       const double* d_t, const double* d_omega, int64_t n_freq, int32_t flags, double* d_out,
                       int64_t out_stride, double* d_out_im, void* d_ws, size_t ws_bytes, void* stream) {
  const int norm = flags & (3 << 2);
  if (!ls_shape_ok(rows, n_max, n_freq) || !d_x || !d_t || !d_omega || !d_out || x_stride < n_max || out_stride < n_freq ||
      (flags & ~15) || norm > MM_LOMB_AMPLITUDE || (norm == MM_LOMB_AMPLITUDE && !d_out_im))
    return MM_ERR_INVALID_ARG;
  if (!d_ws || ((uintptr_t)d_ws & 255) || ws_bytes < mm_lombscargle_workspace_bytes(rows, n_max, n_freq))
    return MM_ERR_WORKSPACE;
  const int64_t nchunks = (n_max + kLsChunk - 1) / kLsChunk;
  char* w = (char*)d_ws;
  double* stat = (double*)w;  w += align_up((size_t)rows * nchunks * 3 * sizeof(double), 256);
  double* mean = (double*)w;  w += align_up((size_t)rows * sizeof(double), 256);
  double* part = nchunks > 1 ? (double*)w : nullptr;
  double* out_im = norm == MM_LOMB_AMPLITUDE ? d_out_im : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const unsigned stat_blocks = (unsigned)((rows * nchunks + kLsThreads / 64 - 1) / (kLsThreads / 64));
  const bool centre = (flags & MM_LOMB_PRECENTER) != 0;
  hipLaunchKernelGGL(ls_stat_kernel, dim3(stat_blocks), dim3(kLsThreads), 0, st, d_x, rows, n_max, x_stride, d_lengths, nchunks,
                     (const double*)nullptr, stat);
  HIP_TRY(hipGetLastError());
  if (centre) {
    hipLaunchKernelGGL(ls_mean_kernel, dim3((unsigned)((rows + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st, stat, rows,
                       nchunks, mean);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ls_stat_kernel, dim3(stat_blocks), dim3(kLsThreads), 0, st, d_x, rows, n_max, x_stride, d_lengths,
                       nchunks, (const double*)mean, stat);
    HIP_TRY(hipGetLastError());
  }
  const dim3 grid((unsigned)nchunks, (unsigned)((rows + 16 * kLsRowTiles - 1) / (16 * kLsRowTiles)),
                  (unsigned)((n_freq + kLsFreqTile - 1) / kLsFreqTile));
  const double* mean_in = centre ? mean : nullptr;
  if (nchunks == 1)
    hipLaunchKernelGGL((ls_main_kernel<kLsRowTiles, true>), grid, dim3(kLsThreads), 0, st, d_x, rows, n_max, x_stride, d_lengths,
                       d_t, d_omega, n_freq, (int)flags, mean_in, (const double*)stat, part, d_out, out_stride, out_im);
  else
    hipLaunchKernelGGL((ls_main_kernel<kLsRowTiles, false>), grid, dim3(kLsThreads), 0, st, d_x, rows, n_max, x_stride, d_lengths,
                       d_t, d_omega, n_freq, (int)flags, mean_in, (const double*)stat, part, d_out, out_stride, out_im);
  HIP_TRY(hipGetLastError());
  if (nchunks > 1) {
    hipLaunchKernelGGL(ls_finish_kernel, dim3((unsigned)((rows * n_freq + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads), 0, st,
                       (const double*)part, (const double*)stat, rows, n_freq, nchunks, (int)flags, d_out, out_stride, out_im);
    HIP_TRY(hipGetLastError());
  }
  return MM_OK;
}

}  // extern "C"
