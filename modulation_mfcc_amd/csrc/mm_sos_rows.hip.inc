#pragma once
// mm_sosfiltfilt_f64 on [rows][n] float64 curves of ANY length, time-parallel over the whole chip: the 'iir' branch of
// applyFilter (script/mfcc.py:29-135, script/calc.py:23-129) on a batch of curves -- amplitude envelopes at the audio rate
// (method 'Hilb': 160 000 samples per ten-second clip, script/calc.py:284-343), RMS envelopes, MFCC-change curves.
//
// The time-major kernels of mm_sos_tm.hip.inc give a row to a lane and cut it into 8 chunks: 256 envelopes of 160 000
// samples keep 32 waves busy on a chip that holds 4096 (10 ms, 65 GB/s).  Here a row is cut into SEGMENTS of 64 chunks x
// 17 samples, a wave per segment with the segment in LDS (coalesced loads along time, lane = chunk), and the linear
// recursion is closed over three levels (chunk, segment, row) with the tables and the lane scan of mm_sos.hip.inc:
//
//   per direction
//   1 sos_seg_state_kernel   wave = (row, segment): S(k) = sum_i W[i] x[k][i] per chunk (end state from zero state), then
//                            the scan over the 64 lanes with the powers of Phi: the last lane holds the END STATE the
//                            SEGMENT reaches from zero state                                     -> seg_S [rows][n_seg]
//   2 sos_seg_scan_kernel    wave = row: start states of the segments, Z(s + 1) = Phi^64 Z(s) + S(s), Z(0) = zi * first
//                            sample: the same scan over lanes = segments, 64 at a time           -> seg_Z [rows][n_seg]
//   3 sos_seg_apply_kernel   wave = (row, segment): S(k) again, the scan seeded with Z(segment), the recursion over every
//                            chunk from its true start state, outputs stored along time
//   (rows of one segment: step 3 alone, seeded with zi * first sample)
//
// The forward direction reads x with scipy's odd extension formed on the fly and writes the padded row-major workspace;
// the reverse direction reads that and writes y without the padding.  Traffic: 3 x 8 bytes per sample and direction.
// Differs from scipy's sequential recursion by rounding only (the Phi products), like the other time-parallel forms.
//
// RG (mm_sosfiltfilt_ragged_*): a length per row.  SegSource reads the row's n_b once per wave and works on the row's own
// n_ext_b = n_b + 2 pad and segment count: forward segments are anchored at the row's start, backward ones at its own end,
// waves behind the row's segments exit (wave-uniform; these kernels have no workgroup barrier), and the backward pass's
// waves share the +0.0 of the columns behind n_b.  The segments, the lanes and the scans are those of the row filtered
// alone, so the result is too, bit for bit; a row scipy refuses (n_b <= pad) is not loaded at all and comes out NaN.
// RG = false compiles to the single-length kernels as they were.
#define MM_SEG_CH 17             // samples per chunk (odd: the chunks of a segment start in different LDS banks)
#define MM_SEG_LEN (64 * MM_SEG_CH)
#define MM_SEG_WAVES 4            // segments per workgroup (8.7 KB of LDS each)
#define MM_SEG_JT 13              // powers Phi^(2^j), j < 13: 6 for the chunks of a segment, 6 for 64 segments, 1 carry

template <int NS, bool RG>
struct SegArgs {
  SosCoef<NS> f;
  const double* tab;             // W [MM_SEG_CH][2 NS] | P [MM_SEG_JT][packed lower block triangle, by columns]
  const double* x;               // forward: the caller's rows [rows][x_stride] ...
  int64_t x_stride;
  const float* xf;               // ... or (not null) float32 rows: n_mfcc > 0: MFCC rows [clips][n_mfcc][n], row r =
  int n_mfcc, first_row, n_rows; //     clip r / n_rows, coefficient first_row + r % n_rows (the change tail's first
                                 //     filter); n_mfcc == 0: plain rows [rows][x_stride].  Float32 rows get their odd
                                 //     extension in float32 arithmetic, as scipy forms it (odd_ext_f32)
  double* ws;                    // padded rows [rows][ws_stride]: forward output, reverse input
  int64_t ws_stride;
  double* y;                     // reverse: output [rows][n]
  double* seg_S;                 // [rows][n_seg][2 NS]
  double* seg_Z;                 // [rows][n_seg][2 NS]
  int64_t rows, n, n_ext;        // n_ext = n + 2 pad
  int n_seg, pad, reverse;
  const int64_t* lens;           // ragged (not null): a length per row, DEVICE int64 [rows]; n, n_ext and n_seg are then
                                 //     those of the longest row the launch is shaped for, y is [rows][n]
};

// sample p (pass order) of the extended row -- forward: scipy's odd extension of x; reverse: the workspace from its end
template <int NS, bool RG>
struct SegSource {
  const double* base;
  const float* basef;            // float32 source (forward pass of the change tail), else null
  double e0, e1;                 // x[0], x[n - 1] (forward)
  int64_t n, n_ext;              // the row's own length and extended length
  int pad, reverse;
  int n_seg;                     // segments of the row; 0: a ragged row scipy refuses (n <= pad), nothing of it is loaded
  __device__ __forceinline__ SegSource(const SegArgs<NS, RG>& a, int64_t row) {
    n = a.n; n_ext = a.n_ext; n_seg = a.n_seg;
    pad = a.pad; reverse = a.reverse; basef = nullptr; base = nullptr;
    if constexpr (RG) {          // the row's own length, clamped: one scalar load per wave (the row is wave-uniform)
      const int64_t nb = a.lens[row];
      n = nb < 1 ? 1 : (nb > a.n ? a.n : nb);
      n_ext = n + 2 * (int64_t)pad;
      n_seg = n > pad ? (int)((n_ext + MM_SEG_LEN - 1) / MM_SEG_LEN) : 0;
    }
    if (reverse) { base = a.ws + row * a.ws_stride; e0 = e1 = 0.0; }
    else if (a.xf) {
      if (a.n_mfcc > 0) basef = mfcc_row(a.xf, a.n_mfcc, a.first_row, a.n_rows, a.n, row);
      else basef = a.xf + row * a.x_stride;
      e0 = (double)basef[0]; e1 = (double)basef[n - 1];
    } else { base = a.x + row * a.x_stride; e0 = base[0]; e1 = base[n - 1]; }
  }
  // one unconditional load per sample (clamped index), the extension by a select
  __device__ __forceinline__ double at(int64_t p) const {
    const bool in = p < n_ext;
    const int64_t t = in ? p : n_ext - 1;
    if (reverse) {
      const double v = base[n_ext - 1 - t];
      return in ? v : 0.0;
    }
    const int64_t i = t < pad ? pad - t : (t < pad + n ? t - pad : 2 * n - 2 + pad - t);
    double r;
    if (basef) {
      const float vf = basef[i];
      r = t < pad ? (double)(2.0f * (float)e0 - vf) : (t < pad + n ? (double)vf : (double)(2.0f * (float)e1 - vf));
    } else {
      const double v = base[i];
      r = t < pad ? 2.0 * e0 - v : (t < pad + n ? v : 2.0 * e1 - v);
    }
    return in ? r : 0.0;
  }
};

// a segment that touches neither the extension nor the row's end (all but two or three per row) ...
template <int NS, bool RG>
__device__ __forceinline__ bool seg_inner(const SegSource<NS, RG>& src, int64_t p0) {
  return src.reverse ? p0 + MM_SEG_LEN <= src.n_ext : (p0 >= src.pad && p0 + MM_SEG_LEN <= src.pad + src.n);
}
// ... is loaded from one address per lane, the 17 loads at immediate offsets
template <int NS, bool RG>
__device__ __forceinline__ void seg_inner_loads(const SegSource<NS, RG>& src, int64_t p0, int lane, double (&v)[MM_SEG_CH]) {
  if (src.reverse) {
    // ascending addresses over ascending lanes (v[m] = pass position MM_SEG_LEN - 1 - lane - 64 m: the puts below mirror)
    const double* q = src.base + (src.n_ext - p0 - MM_SEG_LEN + lane);
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) v[m] = q[64 * m];
  } else if (src.basef) {
    const float* q = src.basef + (p0 - src.pad + lane);
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) v[m] = (double)q[64 * m];
  } else {
    const double* q = src.base + (p0 - src.pad + lane);
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) v[m] = q[64 * m];
  }
}

template <int NS, bool RG>
__device__ __forceinline__ void seg_load(const SegSource<NS, RG>& src, int64_t p0, double* slab, int lane) {
  double v[MM_SEG_CH];
  const bool inner = seg_inner<NS, RG>(src, p0);
  if (inner) seg_inner_loads<NS, RG>(src, p0, lane, v);
  else {
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) v[m] = src.at(p0 + lane + 64 * m);
  }
  if (inner && src.reverse) {
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) slab[MM_SEG_LEN - 1 - lane - 64 * m] = v[m];
  } else {
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) slab[lane + 64 * m] = v[m];
  }
}

// seg_load in two halves for sos_row_stream_kernel: the loads of a segment issued into registers a round ahead
// (seg_fetch: only an inner segment), the slab written when its turn comes
template <int NS, bool RG>
__device__ __forceinline__ bool seg_fetch(const SegSource<NS, RG>& src, int64_t p0, int lane, double (&v)[MM_SEG_CH]) {
  const bool inner = seg_inner<NS, RG>(src, p0);
  if (inner) seg_inner_loads<NS, RG>(src, p0, lane, v);
  return inner;
}

template <int NS, bool RG>
__device__ __forceinline__ void seg_put(const SegSource<NS, RG>& src, int64_t p0, double* slab, int lane, const double (&v)[MM_SEG_CH],
                                        bool fetched) {
  if (fetched && src.reverse) {
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) slab[MM_SEG_LEN - 1 - lane - 64 * m] = v[m];
  } else if (fetched) {
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) slab[lane + 64 * m] = v[m];
  } else {
#pragma unroll 1
    for (int m = 0; m < MM_SEG_CH; ++m) slab[lane + 64 * m] = src.at(p0 + lane + 64 * m);
  }
}

// S = sum_i W[i] x[i] over the lane's chunk (W through the scalar cache)
template <int NS>
__device__ __forceinline__ void seg_weighted_sum(const double* q, const MM_CONST double* W, double (&Z)[2 * NS]) {
  constexpr int S2 = 2 * NS;
#pragma unroll
  for (int a = 0; a < S2; ++a) Z[a] = 0.0;
#pragma unroll
  for (int i = 0; i < MM_SEG_CH; ++i) {
    const double x = q[i];
#pragma unroll
    for (int a = 0; a < S2; ++a) Z[a] = fma(W[i * S2 + a], x, Z[a]);
  }
}

// Z <- M Z for one packed matrix
template <int NS>
__device__ __forceinline__ void seg_matvec(double (&Z)[2 * NS], const MM_CONST double* Pj) {
  constexpr int S2 = 2 * NS;
  double o[S2];
#pragma unroll
  for (int a = 0; a < S2; ++a) o[a] = 0.0;
#pragma unroll
  for (int b = 0; b < S2; ++b) {
    const int base = sos_tri_col(NS, b);
#pragma unroll
    for (int a = (b & ~1); a < S2; ++a) o[a] = fma(Pj[base + a - (b & ~1)], Z[b], o[a]);
  }
#pragma unroll
  for (int a = 0; a < S2; ++a) Z[a] = o[a];
}

template <int NS, bool RG>
__global__ __launch_bounds__(64 * MM_SEG_WAVES) void sos_seg_state_kernel(SegArgs<NS, RG> a) {
  extern __shared__ double seg_lds[];
  constexpr int S2 = 2 * NS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nsm1 = a.n_seg - 1;                            // the last segment's end state is never used
  const int64_t item = (int64_t)blockIdx.x * MM_SEG_WAVES + wave;
  if (item >= a.rows * nsm1) return;                       // wave-uniform; the kernel has no workgroup barrier
  const int64_t row = item / nsm1;
  const int seg = (int)(item - row * nsm1);
  double* slab = seg_lds + wave * MM_SEG_LEN;
  const MM_CONST double* W = (const MM_CONST double*)a.tab;
  const MM_CONST double* P = W + MM_SEG_CH * S2;
  const SegSource<NS, RG> src(a, row);
  if (RG && seg >= src.n_seg - 1) return;                  // ragged: behind the row's own segments (wave-uniform)
  seg_load<NS, RG>(src, (int64_t)seg * MM_SEG_LEN, slab, lane);
  wave_lds_sync();
  double Z[S2];
  seg_weighted_sum<NS>(slab + lane * MM_SEG_CH, W, Z);
  sos_lane_scan<NS, 6>(Z, P, 0, 6, lane, lane);
  if (lane == 63) {
    double* o = a.seg_S + (row * a.n_seg + seg) * S2;
#pragma unroll
    for (int c = 0; c < S2; ++c) o[c] = Z[c];
  }
}

template <int NS, bool RG>
__global__ __launch_bounds__(64 * MM_SEG_WAVES) void sos_seg_scan_kernel(SegArgs<NS, RG> a) {
  constexpr int S2 = 2 * NS, TRI = 2 * NS * (NS + 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * MM_SEG_WAVES + wave;
  if (row >= a.rows) return;
  const MM_CONST double* P = (const MM_CONST double*)a.tab + MM_SEG_CH * S2;
  const SegSource<NS, RG> src(a, row);
  const int n_seg = src.n_seg;                             // the row's own (ragged: at most a.n_seg, which strides S and Z)
  if (RG && n_seg <= 1) return;                            // ragged: one segment starts from zi * first sample, as a row alone
  const double x0 = src.at(0);
  double carry[S2];                                        // start state of segment `base`
#pragma unroll
  for (int s = 0; s < NS; ++s) { carry[2 * s] = a.f.zi[s][0] * x0; carry[2 * s + 1] = a.f.zi[s][1] * x0; }
  const double* S = a.seg_S + row * a.n_seg * S2;
  double* Zo = a.seg_Z + row * a.n_seg * S2;
#pragma unroll 1
  for (int base = 0; base < n_seg; base += 64) {
    const int s = base + lane;
    // u(0) = carry, u(i) = S(base + i - 1)
    double Z[S2];
    const bool have = lane > 0 && s - 1 < n_seg - 1;
#pragma unroll
    for (int c = 0; c < S2; ++c) Z[c] = lane == 0 ? carry[c] : (have ? S[(int64_t)(s - 1) * S2 + c] : 0.0);
    sos_lane_scan<NS, 6>(Z, P, 6, 6, lane, lane);
    if (s < n_seg) {
#pragma unroll
      for (int c = 0; c < S2; ++c) Zo[(int64_t)s * S2 + c] = Z[c];
    }
    if (base + 64 < n_seg) {                               // next round: Z(base + 64) = Phi^64 Z(base + 63) + S(base + 63)
      double nx[S2];
#pragma unroll
      for (int c = 0; c < S2; ++c) nx[c] = Z[c];
      seg_matvec<NS>(nx, P + 6 * TRI);
#pragma unroll
      for (int c = 0; c < S2; ++c) {
        nx[c] += S[(int64_t)(base + 63) * S2 + c];         // (every lane reads it; lane 63's value is the one used)
        carry[c] = lane_from(63 << 2, nx[c]);
      }
    }
  }
}

// the filtered segment, slab -> global memory along time: forward -> the padded workspace; reverse -> y without the padding
template <int NS, bool RG>
__device__ __forceinline__ void seg_store(const SegArgs<NS, RG>& a, const SegSource<NS, RG>& src, int64_t row, int64_t p0,
                                          const double* slab, int lane) {
  const int64_t n = RG ? src.n : a.n, n_ext = RG ? src.n_ext : a.n_ext;      // the row's own (y rows are a.n apart)
  if (!a.reverse && p0 + MM_SEG_LEN <= n_ext) {
    double* o = a.ws + row * a.ws_stride + p0 + lane;
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) o[64 * m] = slab[lane + 64 * m];
  } else if (a.reverse && n_ext - 1 - a.pad - p0 < n && n_ext - a.pad - p0 - MM_SEG_LEN >= 0) {
    double* o = a.y + row * a.n + (n_ext - a.pad - p0 - MM_SEG_LEN + lane);          // ascending addresses over ascending lanes
#pragma unroll
    for (int m = 0; m < MM_SEG_CH; ++m) o[64 * m] = slab[MM_SEG_LEN - 1 - lane - 64 * m];
  } else
#pragma unroll
  for (int m = 0; m < MM_SEG_CH; ++m) {
    const int64_t p = p0 + lane + 64 * m;
    if (p < n_ext) {
      const double v = slab[lane + 64 * m];
      if (!a.reverse) a.ws[row * a.ws_stride + p] = v;
      else {
        const int64_t t = n_ext - 1 - p - a.pad;
        if (t >= 0 && t < n) a.y[row * a.n + t] = v;
      }
    }
  }
}

// ragged, reverse pass: columns [first, first + count) of y's row that lie at or behind the row's own length become +0.0,
// and NaN before it where scipy refuses the row (n <= pad: nothing of the row was loaded or filtered)
template <int NS, bool RG>
__device__ __forceinline__ void seg_fill(const SegArgs<NS, RG>& a, const SegSource<NS, RG>& src, int64_t row, int64_t first,
                                         int64_t count, int lane, int stride) {
  double* yr = a.y + row * a.n;
  const int64_t end = first + count < a.n ? first + count : a.n;
  for (int64_t j = first + lane; j < end; j += stride) {
    if (j >= src.n) yr[j] = 0.0;
    else if (src.n_seg == 0) yr[j] = __builtin_nan("");
  }
}

template <int NS, bool RG>
__global__ __launch_bounds__(64 * MM_SEG_WAVES) void sos_seg_apply_kernel(SegArgs<NS, RG> a) {
  extern __shared__ double seg_lds[];
  constexpr int S2 = 2 * NS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * MM_SEG_WAVES + wave;
  if (item >= a.rows * a.n_seg) return;
  const int64_t row = item / a.n_seg;
  const int seg = (int)(item - row * a.n_seg);
  double* slab = seg_lds + wave * MM_SEG_LEN;
  const MM_CONST double* W = (const MM_CONST double*)a.tab;
  const MM_CONST double* P = W + MM_SEG_CH * S2;
  const SegSource<NS, RG> src(a, row);
  const int64_t p0 = (int64_t)seg * MM_SEG_LEN;
  // ragged, reverse pass: the launch's segments share the zeros (and NaN) of the row between them, MM_SEG_LEN columns each
  if (RG && a.reverse) seg_fill<NS, RG>(a, src, row, p0, MM_SEG_LEN, lane, 64);
  if (RG && seg >= src.n_seg) return;                      // ragged: behind the row's own segments (wave-uniform)
  seg_load<NS, RG>(src, p0, slab, lane);
  wave_lds_sync();
  double* q = slab + lane * MM_SEG_CH;
  double Z[S2];
  seg_weighted_sum<NS>(q, W, Z);                           // (samples behind the row's end are zeros; their sums are unused)
  // u(0) = the segment's start state, u(k) = S(k - 1)
  {
    double z0[S2];
    if (src.n_seg == 1) {
      const double x0 = slab[0];
#pragma unroll
      for (int s = 0; s < NS; ++s) { z0[2 * s] = a.f.zi[s][0] * x0; z0[2 * s + 1] = a.f.zi[s][1] * x0; }
    } else {
      const double* zs = a.seg_Z + (row * a.n_seg + seg) * S2;
#pragma unroll
      for (int c = 0; c < S2; ++c) z0[c] = zs[c];
    }
    const int from = (lane - 1) << 2;
#pragma unroll
    for (int c = 0; c < S2; ++c) {
      const double up = lane_from(from, Z[c]);
      Z[c] = lane == 0 ? z0[c] : up;
    }
  }
  sos_lane_scan<NS, 6>(Z, P, 0, 6, lane, lane);
  {
    double z0[NS], z1[NS], v[MM_SEG_CH];
#pragma unroll
    for (int s = 0; s < NS; ++s) { z0[s] = Z[2 * s]; z1[s] = Z[2 * s + 1]; }
#pragma unroll
    for (int i = 0; i < MM_SEG_CH; ++i) v[i] = q[i];
#pragma unroll
    for (int i = 0; i < MM_SEG_CH; ++i) v[i] = sos_step<NS>(a.f, v[i], z0, z1);   // (past `len`: on zeros, never stored)
#pragma unroll
    for (int i = 0; i < MM_SEG_CH; ++i) q[i] = v[i];
  }
  wave_lds_sync();
  seg_store<NS, RG>(a, src, row, p0, slab, lane);
}

// A ROW PER WORKGROUP (batches of at least MM_ROW_MIN rows): the three launches above read every sample twice per
// direction (once for the segments' end states, once to filter) because a segment's start state depends on every
// segment before it.  Here the 16 waves of a workgroup walk ONE row, 16 segments per round, and the dependence is
// closed inside the round: every wave forms its segment's end state from zero state (weighted sums + scan, as
// sos_seg_state_kernel), a barrier, wave 0 scans the 16 end states behind the carry of the round before
// (sos_seg_scan_kernel's step: lanes = segments), a barrier, every wave filters its segment from its true start
// state (sos_seg_apply_kernel).  One read and one write per sample and direction, no segment states in memory; the
// next round's samples are loaded while this one computes.
#define MM_ROW_WAVES 16
#define MM_ROW_MIN 128
template <int NS, bool RG>
__global__ __launch_bounds__(64 * MM_ROW_WAVES) void sos_row_stream_kernel(SegArgs<NS, RG> a) {
  extern __shared__ double seg_lds[];
  __shared__ double segS[2][MM_ROW_WAVES][2 * MM_SCAN_MAX_SEC];
  __shared__ double segZ[MM_ROW_WAVES][2 * MM_SCAN_MAX_SEC];
  constexpr int S2 = 2 * NS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x;
  double* slab = seg_lds + wave * MM_SEG_LEN;
  double* q = slab + lane * MM_SEG_CH;
  const MM_CONST double* W = (const MM_CONST double*)a.tab;
  const MM_CONST double* P = W + MM_SEG_CH * S2;
  const SegSource<NS, RG> src(a, row);
  const int n_seg = src.n_seg;                             // the row's own: uniform over the workgroup, like every barrier below
  __shared__ double carry[2 * MM_SCAN_MAX_SEC];                 // start state of segment `base` (wave 0 reads and writes it)
  if (threadIdx.x == 0 && (!RG || n_seg > 0)) {
    const double x0 = src.at(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) { carry[2 * s] = a.f.zi[s][0] * x0; carry[2 * s + 1] = a.f.zi[s][1] * x0; }
  }
  // ragged, reverse pass: the zeros (and NaN) of the row, shared among the workgroup's threads
  if (RG && a.reverse) seg_fill<NS, RG>(a, src, row, 0, a.n, threadIdx.x, 64 * MM_ROW_WAVES);
  double v[MM_SEG_CH];
  bool fetched = wave < n_seg ? seg_fetch<NS, RG>(src, (int64_t)wave * MM_SEG_LEN, lane, v) : false;
  MM_STAMP_BEGIN(10)
#pragma unroll 1
  for (int base = 0, r = 0; base < n_seg; base += MM_ROW_WAVES, ++r) {
    const int seg = base + wave;
    const bool live = seg < n_seg;                         // wave-uniform
    const int64_t p0 = (int64_t)seg * MM_SEG_LEN;
    double S[S2];
    if (live) {
      seg_put<NS, RG>(src, p0, slab, lane, v, fetched);
      wave_lds_sync();
      MM_STAMP_AT(0)
      if (seg + MM_ROW_WAVES < n_seg) fetched = seg_fetch<NS, RG>(src, p0 + (int64_t)MM_ROW_WAVES * MM_SEG_LEN, lane, v);
      seg_weighted_sum<NS>(q, W, S);
      MM_STAMP_AT(1)
      double V[S2];
#pragma unroll
      for (int c = 0; c < S2; ++c) V[c] = S[c];
      sos_lane_scan<NS, 6>(V, P, 0, 6, lane, lane);              // lane 63: the end state the segment reaches from zero state
      if (lane == 63) {
#pragma unroll
        for (int c = 0; c < S2; ++c) segS[r & 1][wave][c] = V[c];
      }
    }
    MM_STAMP_AT(2)
    __syncthreads();
    MM_STAMP_AT(3)
    if (wave == 0) {
      // lanes = segments of the round: u(0) = carry, u(i) = end state of segment base + i - 1; lane i then holds the start
      // state of segment base + i, lane 16 the next round's carry (end states of waves without a segment are stale
      // values that only reach lanes behind the row's last segment)
      double Z[S2];
#pragma unroll
      for (int c = 0; c < S2; ++c) Z[c] = lane == 0 ? carry[c] : (lane <= MM_ROW_WAVES ? segS[r & 1][lane - 1 < 0 ? 0 : lane - 1][c] : 0.0);
      sos_lane_scan<NS, 6>(Z, P, 6, 6, lane, lane);
      if (lane < MM_ROW_WAVES) {
#pragma unroll
        for (int c = 0; c < S2; ++c) segZ[lane][c] = Z[c];
      }
      if (lane == MM_ROW_WAVES) {
#pragma unroll
        for (int c = 0; c < S2; ++c) carry[c] = Z[c];
      }
    }
    MM_STAMP_AT(4)
    __syncthreads();
    MM_STAMP_AT(5)
    if (live) {
      double Z[S2];
      const int from = (lane - 1) << 2;
#pragma unroll
      for (int c = 0; c < S2; ++c) {
        const double up = lane_from(from, S[c]);
        Z[c] = lane == 0 ? segZ[wave][c] : up;
      }
      sos_lane_scan<NS, 6>(Z, P, 0, 6, lane, lane);
      MM_STAMP_AT(6)
      {
        double z0[NS], z1[NS], y[MM_SEG_CH];
#pragma unroll
        for (int s = 0; s < NS; ++s) { z0[s] = Z[2 * s]; z1[s] = Z[2 * s + 1]; }
#pragma unroll
        for (int i = 0; i < MM_SEG_CH; ++i) y[i] = q[i];
#pragma unroll
        for (int i = 0; i < MM_SEG_CH; ++i) y[i] = sos_step<NS>(a.f, y[i], z0, z1);
#pragma unroll
        for (int i = 0; i < MM_SEG_CH; ++i) q[i] = y[i];
      }
      wave_lds_sync();
      MM_STAMP_AT(7)
      seg_store<NS, RG>(a, src, row, p0, slab, lane);
      wave_lds_sync();                                     // (the stores have read the slab before the next round's put)
      MM_STAMP_AT(8)
    }
  }
  MM_STAMP_END_BLK(10, gridDim.x - 1)
}
// ---- host side ----
template <int NS>
static void seg_tables(const SosCoef<NS>& c, std::vector<double>& tab) {
  constexpr int S2 = 2 * NS, TRI = 2 * NS * (NS + 1);
  tab.assign((size_t)MM_SEG_CH * S2 + (size_t)MM_SEG_JT * TRI, 0.0);
  sos_scan_tables<NS>(c, MM_SEG_CH, MM_SEG_JT, tab.data(), tab.data() + (size_t)MM_SEG_CH * S2);
}

static int64_t seg_count(int64_t n_ext) { return (n_ext + MM_SEG_LEN - 1) / MM_SEG_LEN; }
static int64_t seg_ws_stride(int64_t n_ext) { return (n_ext + 1) & ~(int64_t)1; }
// doubles of workspace: table | seg_S | seg_Z | padded rows
static size_t seg_workspace_doubles(int64_t rows, int64_t n, int pad) {
  const int64_t n_ext = n + 2 * (int64_t)pad;
  return (size_t)(1024 + 2 * rows * seg_count(n_ext) * 2 * MM_SCAN_MAX_SEC + rows * seg_ws_stride(n_ext));
}

struct SegSrc {                  // where the forward pass reads: float64 rows, or float32 MFCC rows of clips
  const double* x; int64_t x_stride;
  const float* xf; int n_mfcc, first_row, n_rows;
};

// lens (DEVICE int64 [rows], or null): the ragged form -- n is then the longest row's length, which shapes every launch
template <int NS, bool RG>
static int launch_sos_rows(const SosFilt& f, const SegSrc& src, int64_t rows, int64_t n, double* d_y, double* ws,
                           hipStream_t st, const int64_t* lens) {
  constexpr int S2 = 2 * NS;
  SegArgs<NS, RG> a;
  sos_coef_of<NS>(f, &a.f);
  std::vector<double> tab;
  seg_tables<NS>(a.f, tab);
  if (tab.size() > 1024) return MM_ERR_UNSUPPORTED;
  a.rows = rows; a.n = n; a.pad = f.padlen; a.n_ext = n + 2 * (int64_t)f.padlen;
  const int64_t nseg = seg_count(a.n_ext);
  if (nseg > 0x7FFFFFFF || (rows * nseg + MM_SEG_WAVES - 1) / MM_SEG_WAVES > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  a.n_seg = (int)nseg;
  a.tab = ws;
  a.seg_S = ws + 1024;
  a.seg_Z = a.seg_S + rows * nseg * S2;
  a.ws = ws + 1024 + 2 * rows * nseg * 2 * MM_SCAN_MAX_SEC;
  a.ws_stride = seg_ws_stride(a.n_ext);
  a.x = src.x; a.x_stride = src.x_stride; a.xf = src.xf; a.n_mfcc = src.n_mfcc; a.first_row = src.first_row;
  a.n_rows = src.n_rows; a.y = d_y; a.lens = lens;
  sos_tab_upload(tab, ws, st);
  // a workgroup per row: one read + one write per sample.  Ragged rows only up to one round of segments: within a round the
  // workgroup's scan over segments is the wave-per-segment form's, operation for operation, and a ragged row equals the row
  // filtered alone (which takes that form) bit for bit; the carry into a second round is rounded differently
  if (rows >= MM_ROW_MIN && nseg > 1 && rows <= 0x7FFFFFFF && (!RG || nseg <= MM_ROW_WAVES)) {
    static PerDeviceOnce attr_once;
    const size_t rlds = (size_t)MM_ROW_WAVES * MM_SEG_LEN * sizeof(double);
    {
      const int rc = per_device_once(attr_once, "sos_row_stream_kernel", [] {
        return hipFuncSetAttribute((const void*)sos_row_stream_kernel<NS, RG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds) == hipSuccess;
      });
      if (rc) return rc;
    }
    for (int pass = 0; pass < 2; ++pass) {
      a.reverse = pass;
      hipLaunchKernelGGL((sos_row_stream_kernel<NS, RG>), dim3((unsigned)rows), dim3(64 * MM_ROW_WAVES), rlds, st, a);
    }
    return MM_OK;
  }
  const size_t lds = (size_t)MM_SEG_WAVES * MM_SEG_LEN * sizeof(double);
  const dim3 blk(64 * MM_SEG_WAVES);
  for (int pass = 0; pass < 2; ++pass) {
    a.reverse = pass;
    if (nseg > 1) {
      const int64_t items = rows * (nseg - 1);
      hipLaunchKernelGGL((sos_seg_state_kernel<NS, RG>), dim3((unsigned)((items + MM_SEG_WAVES - 1) / MM_SEG_WAVES)), blk, lds, st, a);
      hipLaunchKernelGGL((sos_seg_scan_kernel<NS, RG>), dim3((unsigned)((rows + MM_SEG_WAVES - 1) / MM_SEG_WAVES)), blk, 0, st, a);
    }
    hipLaunchKernelGGL((sos_seg_apply_kernel<NS, RG>), dim3((unsigned)((rows * nseg + MM_SEG_WAVES - 1) / MM_SEG_WAVES)), blk, lds, st, a);
  }
  return MM_OK;
}

static int launch_sos_rows_any(const SosFilt& f, const SegSrc& src, int64_t rows, int64_t n, double* d_y, double* ws,
                               hipStream_t st, const int64_t* lens = nullptr) {
  return with_scan_sections(f.n_sec, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    return lens ? launch_sos_rows<NS, true>(f, src, rows, n, d_y, ws, st, lens)
                : launch_sos_rows<NS, false>(f, src, rows, n, d_y, ws, st, nullptr);
  });
}
