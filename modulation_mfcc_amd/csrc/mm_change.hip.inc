#pragma once
// The reference's MFCC-change tail (script/mfcc.py:392-427) on the device, float64 like scipy (which
// upcasts):  drop c0 -> sosfiltfilt(sos1) per coefficient row -> np.gradient along time ->
// sqrt(sum_rows d^2) / n_rows -> sosfiltfilt(sos2).  SURVEY.md 8(f) row N1.  Three device forms (change_form(), mm_tail.hip):
// the clip-resident kernel of mm_change_clip.hip.inc, and the two this file holds the derivative + norm kernels of.
//
// TIME-MAJOR (mm_sos_tm.hip.inc; row r = clip * n_rows + coefficient is the fast index of the workspace):
//   tm_pack_kernel      mfcc f32 [B][n_mfcc][T] -> ws1 f64 [T + 2 p1][Rp]
//   chg_pad_kernel      odd extension of ws1 (in float32 arithmetic: odd_ext_f32)
//   chg_sos_kernel<NS>  (or its chunked form) in place over ws1
//   chg_norm_kernel     gradient + norm over the clip's rows -> ws2 f64 [T + 2 p2][Bp] (lane = clip)
//   chg_pad_kernel      odd extension of ws2
//   chg_sos_kernel<NS>  the output filter on ws2
//   tm_unpack_kernel    ws2 -> out f64 [B][T]
//
// Measured at 1024 clips x 12 rows x 1001 frames: 0.24 ms (sequential recursions on 192 and then 16 waves: 0.41 ms;
// time-parallel chunks: 0.27; derivative + norm with unit-stride reads: 0.24); (the one-block-per-clip predecessor -- 12
// busy lanes per clip, recursion state in scratch memory -- took 3.2 ms).
//
// SEGMENTED ROWS (mm_sos_rows.hip.inc): launch_chg_segmented below.
struct ChangeParams {
  const float* mfcc;   // [B][n_mfcc][T]
  int64_t n_frames, batch;
  int n_mfcc, first_row, n_rows;
  int p1, p2;          // padlen of the two filters
  int sg;              // differentiator: 0 = np.gradient, 1 = savgol_filter(x, 3, 2, deriv=1, mode='interp')
  int64_t R, Rp, Bp;   // rows = batch * n_rows; both padded to multiples of 64
  double* ws1;         // [T + 2 p1][Rp]
  double* ws2;         // [T + 2 p2][Bp]
  double* out;         // [B][T]
};

// The derivative at the first / last sample of a row: np.gradient's first-order difference, or (sg) the derivative of
// the parabola through the three end samples (Savitzky-Golay mode='interp'); x(0) x(1) x(2) = those samples in time
// order.  Interior: both differentiators are (x[t+1] - x[t-1]) / 2 (the Savitzky-Golay window 3, order 2, deriv 1
// coefficients are [1/2, 0, -1/2])
template <class F>
__device__ __forceinline__ double chg_end_deriv(bool first, int sg, F x) {
  return first ? (sg ? (-3.0 * x(0) + 4.0 * x(1) - x(2)) / 2.0 : x(1) - x(0))
               : (sg ? (3.0 * x(2) - 4.0 * x(1) + x(0)) / 2.0 : x(2) - x(1));
}

// np.gradient along time (central, one-sided at the ends), norm over the clip's rows
// One block = 64 clips at one time step: the squared derivatives of all their rows are formed with unit-stride reads
// of the time-major buffer (thread <-> column) and parked in LDS, then thread <-> clip adds its rows in row order
// (the same sum, term by term, as one thread walking the rows of its clip at a 96-byte stride between lanes did).
#define MM_CHG_MAXROWS 64
__global__ __launch_bounds__(256) void chg_norm_kernel(ChangeParams p) {
  __shared__ double sq[64 * MM_CHG_MAXROWS];
  const int64_t T = p.n_frames;
  const int64_t b0 = (int64_t)blockIdx.y * 64, t = blockIdx.x;
  const int64_t c0 = b0 * p.n_rows;
  const int count = 64 * p.n_rows;
  const double* f = p.ws1 + (int64_t)p.p1 * p.Rp;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int64_t col = c0 + e;
    double d = 0.0;
    if (col < p.R) {
      if (T == 1) d = 0.0;
      else if (t == 0) d = chg_end_deriv(true, p.sg, [&](int i) { return f[i * p.Rp + col]; });
      else if (t == T - 1) d = chg_end_deriv(false, p.sg, [&](int i) { return f[(T - 3 + i) * p.Rp + col]; });
      else d = (f[(t + 1) * p.Rp + col] - f[(t - 1) * p.Rp + col]) / 2.0;
    }
    sq[e] = d * d;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int64_t b = b0 + threadIdx.x;
    double acc = 0.0;
    if (b < p.batch) {
      for (int r = 0; r < p.n_rows; ++r) acc += sq[threadIdx.x * p.n_rows + r];
      acc = sqrt(acc) / (double)p.n_rows;
    }
    if (b < p.Bp) p.ws2[(p.p2 + t) * p.Bp + b] = acc;
  }
}

// More than MM_CHG_MAXROWS rows per clip: one thread per (time step, clip) walks the clip's rows.
__global__ __launch_bounds__(256) void chg_norm_rows_kernel(ChangeParams p) {
  const int64_t T = p.n_frames;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= T * p.Bp) return;
  const int64_t b = idx % p.Bp, t = idx / p.Bp;
  double acc = 0.0;
  if (b < p.batch) {
    const double* f = p.ws1 + (int64_t)p.p1 * p.Rp + b * p.n_rows;
    for (int r = 0; r < p.n_rows; ++r) {
      double d;
      if (T == 1) d = 0.0;
      else if (t == 0) d = chg_end_deriv(true, p.sg, [&](int i) { return f[i * p.Rp + r]; });
      else if (t == T - 1) d = chg_end_deriv(false, p.sg, [&](int i) { return f[(T - 3 + i) * p.Rp + r]; });
      else d = (f[(t + 1) * p.Rp + r] - f[(t - 1) * p.Rp + r]) / 2.0;
      acc += d * d;
    }
    acc = sqrt(acc) / (double)p.n_rows;
  }
  p.ws2[(p.p2 + t) * p.Bp + b] = acc;
}

// ---- the MFCC-change tail on the segmented rows: one long recording (the reference's own call: a whole file, tStep
// 1 ms -> 10 001 frames per ten seconds) or a few long clips, where neither a workgroup per clip nor a lane per row
// fills the chip.  rows filter (float32 MFCC rows in, float64 rows out) -> derivative + norm -> curve filter.
__global__ __launch_bounds__(256) void chg_norm_rowmajor_kernel(const double* __restrict__ f, int64_t batch, int n_rows,
                                                                int64_t T, int sg, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * T) return;
  const int64_t b = idx / T, t = idx - b * T;
  const double* fr = f + b * n_rows * T;
  double acc = 0.0;
  if (t > 0 && t < T - 1) {
#pragma unroll 4
    for (int r = 0; r < n_rows; ++r) {
      const double d = (fr[r * T + t + 1] - fr[r * T + t - 1]) / 2.0;
      acc += d * d;
    }
  } else {
    const int64_t e = t == 0 ? 0 : T - 3;                  // (T > padlen >= 6)
    for (int r = 0; r < n_rows; ++r) {
      const double x[3] = {fr[r * T + e], fr[r * T + e + 1], fr[r * T + e + 2]};
      const double d = chg_end_deriv(t == 0, sg, [&](int i) { return x[i]; });
      acc += d * d;
    }
  }
  out[idx] = sqrt(acc) / (double)n_rows;
}

// doubles: rows filter's workspace | filtered rows [R][T] | curve [B][T] | curve filter's workspace
static size_t chg_seg_workspace_doubles(int64_t batch, int n_rows, int64_t T, int pad1, int pad2) {
  return seg_workspace_doubles(batch * n_rows, T, pad1) + (size_t)(batch * n_rows * T) + (size_t)(batch * T) +
         seg_workspace_doubles(batch, T, pad2);
}

static int launch_chg_segmented(const ChangeParams& q, const SosFilt& f1, const SosFilt& f2, double* ws, hipStream_t st) {
  const int64_t R = q.batch * q.n_rows, T = q.n_frames;
  double* ws1 = ws;
  double* rows_out = ws1 + seg_workspace_doubles(R, T, f1.padlen);
  double* curve = rows_out + R * T;
  double* ws2 = curve + q.batch * T;
  SegSrc s1 = {nullptr, 0, q.mfcc, q.n_mfcc, q.first_row, q.n_rows};
  int rc = launch_sos_rows_any(f1, s1, R, T, rows_out, ws1, st);
  if (rc) return rc;
  if ((q.batch * T + 255) / 256 > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  double* norm_out = f2.n_sec > 0 ? curve : q.out;
  hipLaunchKernelGGL(chg_norm_rowmajor_kernel, dim3((unsigned)((q.batch * T + 255) / 256)), dim3(256), 0, st, rows_out, q.batch,
                     q.n_rows, T, q.sg, norm_out);
  if (f2.n_sec > 0) {
    SegSrc s2 = {curve, T, nullptr, 0, 0, 0};
    rc = launch_sos_rows_any(f2, s2, q.batch, T, q.out, ws2, st);
  }
  return rc;
}
