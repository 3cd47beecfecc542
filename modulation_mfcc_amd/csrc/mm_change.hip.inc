#pragma once
// The reference's MFCC-change tail (script/mfcc.py:392-427) on the device, float64 like scipy (which
// upcasts):  drop c0 -> sosfiltfilt(sos1) per coefficient row -> np.gradient along time ->
// sqrt(sum_rows d^2) / n_rows -> sosfiltfilt(sos2).  SURVEY.md 8(f) row N1.
//
// sosfiltfilt = scipy.signal.sosfiltfilt defaults: odd extension by padlen = 3*ntaps samples,
// steady-state initial conditions sosfilt_zi(sos) scaled by the first sample of each pass, forward
// pass, reversed pass, strip the padding.  The IIR recursion is sequential in time and independent
// per row, so ONE LANE OWNS ONE ROW and the rows of the whole batch run side by side:
//
//   chg_pack_kernel     mfcc f32 [B][n_mfcc][T] -> ws1 f64 [T + 2 p1][Rp], TIME-MAJOR (row r =
//                       clip * n_rows + coefficient is the fast index: every access of the
//                       recursion below is one coalesced 512-byte line per wave), odd extension included
//   chg_sos_kernel<NS>  in-place forward + reverse pass over ws1; sections unrolled (coefficients and
//                       the 2*NS state words live in registers), samples fetched 8 time steps ahead
//   chg_norm_kernel     gradient + norm over the clip's rows -> ws2 f64 [T + 2 p2][Bp] (lane = clip)
//   chg_pad_kernel      odd extension of ws2
//   chg_sos_kernel<NS>  the output filter on ws2
//   chg_unpack_kernel   ws2 -> out f64 [B][T]
//
// Measured at 1024 clips x 12 rows x 1001 frames: 0.24 ms (sequential recursions on 192 and then 16 waves: 0.41 ms;
// time-parallel chunks: 0.27; derivative + norm with unit-stride reads: 0.24); (the one-block-per-clip predecessor -- 12
// busy lanes per clip, recursion state in scratch memory -- took 3.2 ms).
#define MM_MAX_SEC 16

struct SosFilt {
  double c[MM_MAX_SEC][6];   // b0 b1 b2 a0 a1 a2 (a0 = 1); sections beyond n_sec are the identity
  double zi[MM_MAX_SEC][2];  // sosfilt_zi
  int n_sec, padlen;
};

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

// value i of the odd extension (by p samples on both sides) of x[0..T)
template <class F>
__device__ __forceinline__ double odd_ext(F x, int64_t i, int p, int64_t T) {
  if (i < p) return 2.0 * x(0) - x(p - i);
  if (i < p + T) return x(i - p);
  return 2.0 * x(T - 1) - x(T - 2 - (i - p - T));
}
// The same for rows that are float32 in the reference (librosa's MFCCs and RMS envelopes): scipy.signal.sosfiltfilt
// forms the extension `2 * x[0] - x[k]` in the array's own type BEFORE the recursion upcasts, i.e. the padded samples
// are rounded to float32.  Formed in float64 instead, the filtered rows move by 3e-9 and the change curve (a
// derivative of them) by 1e-7 of its maximum -- with this, the tail equals scipy's to ~1e-12.
template <class F>
__device__ __forceinline__ double odd_ext_f32(F x, int64_t i, int p, int64_t T) {
  if (i < p) return (double)(2.0f * (float)x(0) - (float)x(p - i));
  if (i < p + T) return x(i - p);
  return (double)(2.0f * (float)x(T - 1) - (float)x(T - 2 - (i - p - T)));
}

// 64 rows x 64 time steps per block through an LDS tile: reads coalesced along time, writes along rows
__global__ __launch_bounds__(256) void chg_pack_kernel(ChangeParams p) {
  __shared__ float tile[64][65];
  const int64_t T = p.n_frames;
  const int64_t r0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t r = r0 + rr, t = t0 + tx;
    float v = 0.0f;
    if (r < p.R && t < T) {
      const int64_t b = r / p.n_rows, c = r - b * p.n_rows;
      v = p.mfcc[(b * p.n_mfcc + p.first_row + c) * T + t];
    }
    tile[rr][tx] = v;
  }
  __syncthreads();
  for (int tt = ty; tt < 64; tt += 4) {
    const int64_t t = t0 + tt;
    if (t < T) p.ws1[(p.p1 + t) * p.Rp + r0 + tx] = (double)tile[tx][tt];
  }
}

// odd extension of a time-major buffer [T + 2 pad][W]: one thread per (padding sample, column)
// f32: the interior holds float32 values (see odd_ext_f32)
__global__ __launch_bounds__(256) void chg_pad_kernel(double* ws, int64_t T, int pad, int64_t W, int f32) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * (int64_t)pad * W) return;
  const int64_t col = idx % W, j = idx / W;                 // j in [0, 2 pad)
  const int64_t i = j < pad ? j : T + j;                    // position in the extended sequence
  auto x = [&](int64_t t) { return ws[(pad + t) * W + col]; };
  ws[i * W + col] = f32 ? odd_ext_f32(x, i, pad, T) : odd_ext(x, i, pad, T);
}

template <int NS>
struct SosCoef {
  double c[NS][5];     // b0 b1 b2 a1 a2
  double zi[NS][2];
};

// One sample through the cascade (transposed direct form II, scipy's sosfilt recursion) in 5 float64 operations per
// section, every multiply-add fused -- the dependent chain of this recursion is what bounds the filter kernels:
//   y = b0 x + z0;   z0' = b1 x + (z1 - a1 y);   z1' = b2 x - a2 y
template <int NS>
__device__ __forceinline__ double sos_step(const SosCoef<NS>& f, double x, double (&z0)[NS], double (&z1)[NS]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double y = fma(f.c[s][0], x, z0[s]);
    z0[s] = fma(f.c[s][1], x, fma(-f.c[s][3], y, z1[s]));
    z1[s] = fma(f.c[s][2], x, -(f.c[s][4] * y));
    x = y;
  }
  return x;
}

// forward + reverse pass, in place, over the time-major buffer ws[n][W]; lane = column
template <int NS>
__global__ __launch_bounds__(64) void chg_sos_kernel(double* ws, int64_t n, int64_t W, SosCoef<NS> f) {
  constexpr int U = 8;
  const int64_t col = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double* w = ws + col;
  double z0[NS], z1[NS];
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t first = pass ? n - 1 : 0;
    const int64_t step = pass ? -W : W;
    double* q = w + first * W;
    const double x0 = *q;
#pragma unroll
    for (int s = 0; s < NS; ++s) { z0[s] = f.zi[s][0] * x0; z1[s] = f.zi[s][1] * x0; }
    int64_t i = 0;
    // blocks of U samples, the NEXT block's loads in flight while this one runs through the sections (one wave per
    // SIMD here: nothing else hides the ~1 us a load takes -- without the prefetch a block cost its latency again)
    double v[U], nv[U];
    if (n >= U) {
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = q[u * step];
    }
    for (; i + U <= n; i += U) {
      const bool more = i + 2 * U <= n;
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) nv[u] = q[(U + u) * step];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = sos_step<NS>(f, v[u], z0, z1);
#pragma unroll
      for (int u = 0; u < U; ++u) q[u * step] = v[u];
      q += U * step;
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = nv[u];
      }
    }
    for (; i < n; ++i) {
      *q = sos_step<NS>(f, *q, z0, z1);
      q += step;
    }
  }
}

// Time-parallel form of the same recursion (used for n >= MM_SOS_CHUNK_MIN): the sequence is cut into K chunks and
// the K waves of a workgroup take one each, all on the same 64 columns.  The cascade is linear in (state, input), so
//   state at the end of a chunk = (state reached from ZERO state) + Phi * (state at its start),
// Phi = the 2 NS x 2 NS transition of one full chunk with zero input (host: sos_chunk_phi).  Per direction:
//   A  every wave runs its chunk from zero state, keeps only the final state            (no stores)
//   B  the start states follow by the chain Z(k+1) = Zzs(k) + Phi Z(k), Z(0) = zi * first sample (every wave
//      forms its own prefix of the chain from the LDS copies of the Zzs)
//   C  every wave runs its chunk again from its true start state and stores the outputs (in place)
// Twice the arithmetic of chg_sos_kernel on K times the waves: the sequential kernel keeps one wave per SIMD busy on a
// fifth of the SIMDs and is bound by its own dependent double-precision chain.  Differs from it by rounding only
// (the Phi products): ~1e-14 relative.
#define MM_SOS_K 8
#define MM_SOS_CHUNK_MIN 256
template <int NS>
struct SosChunk {
  SosCoef<NS> f;
  double phi[2 * NS][2 * NS];    // state order: z0[0], z1[0], z0[1], z1[1], ...
  int64_t chunk;                 // samples per full chunk
};

template <int NS>
__global__ __launch_bounds__(64 * MM_SOS_K) void chg_sos_chunk_kernel(double* ws, int64_t n, int64_t W, SosChunk<NS> g) {
  constexpr int U = 8;
  __shared__ double zs[MM_SOS_K][2 * NS][64];
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  double* w = ws + col;
  const int64_t i0 = (int64_t)k * g.chunk;
  const int64_t len = i0 >= n ? 0 : (n - i0 < g.chunk ? n - i0 : g.chunk);
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t step = pass ? -W : W;
    double* q0 = w + (pass ? n - 1 - i0 : i0) * W;          // this chunk's first sample in pass order
    double z0[NS], z1[NS];
    // ---- A: zero-state run, final state only
#pragma unroll
    for (int s = 0; s < NS; ++s) { z0[s] = 0.0; z1[s] = 0.0; }
    {
      const double* q = q0;
      int64_t i = 0;
      for (; i + U <= len; i += U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = q[u * step];
#pragma unroll
        for (int u = 0; u < U; ++u) (void)sos_step<NS>(g.f, v[u], z0, z1);
        q += U * step;
      }
      for (; i < len; ++i) { (void)sos_step<NS>(g.f, *q, z0, z1); q += step; }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) { zs[k][2 * s][lane] = z0[s]; zs[k][2 * s + 1][lane] = z1[s]; }
    const double x0 = w[(pass ? n - 1 : 0) * W];            // first sample of the pass: scales the start state
    __syncthreads();
    // ---- B: Z(k) from the chain over the chunks before this one
    double Z[2 * NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { Z[2 * s] = g.f.zi[s][0] * x0; Z[2 * s + 1] = g.f.zi[s][1] * x0; }
#pragma unroll 1
    for (int kk = 0; kk < k; ++kk) {
      double Zn[2 * NS];
#pragma unroll
      for (int a = 0; a < 2 * NS; ++a) {
        double acc = zs[kk][a][lane];
#pragma unroll
        for (int b = 0; b < 2 * NS; ++b) acc = fma(g.phi[a][b], Z[b], acc);
        Zn[a] = acc;
      }
#pragma unroll
      for (int a = 0; a < 2 * NS; ++a) Z[a] = Zn[a];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) { z0[s] = Z[2 * s]; z1[s] = Z[2 * s + 1]; }
    // ---- C: the chunk again from its true start state, outputs in place
    {
      double* q = q0;
      int64_t i = 0;
      for (; i + U <= len; i += U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = q[u * step];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = sos_step<NS>(g.f, v[u], z0, z1);
#pragma unroll
        for (int u = 0; u < U; ++u) q[u * step] = v[u];
        q += U * step;
      }
      for (; i < len; ++i) { *q = sos_step<NS>(g.f, *q, z0, z1); q += step; }
    }
    __syncthreads();                                         // the reverse pass reads what every chunk stored
  }
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
      // interior: both differentiators are (x[t+1] - x[t-1]) / 2 (the Savitzky-Golay window 3, order 2,
      // deriv 1 coefficients are [1/2, 0, -1/2]); ends: np.gradient's first-order difference, or the
      // derivative of the parabola through the three end samples (mode='interp')
      if (T == 1) d = 0.0;
      else if (t == 0) d = p.sg ? (-3.0 * f[col] + 4.0 * f[p.Rp + col] - f[2 * p.Rp + col]) / 2.0 : f[p.Rp + col] - f[col];
      else if (t == T - 1)
        d = p.sg ? (3.0 * f[(T - 1) * p.Rp + col] - 4.0 * f[(T - 2) * p.Rp + col] + f[(T - 3) * p.Rp + col]) / 2.0
                 : f[(T - 1) * p.Rp + col] - f[(T - 2) * p.Rp + col];
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
      else if (t == 0) d = p.sg ? (-3.0 * f[r] + 4.0 * f[p.Rp + r] - f[2 * p.Rp + r]) / 2.0 : f[p.Rp + r] - f[r];
      else if (t == T - 1)
        d = p.sg ? (3.0 * f[(T - 1) * p.Rp + r] - 4.0 * f[(T - 2) * p.Rp + r] + f[(T - 3) * p.Rp + r]) / 2.0
                 : f[(T - 1) * p.Rp + r] - f[(T - 2) * p.Rp + r];
      else d = (f[(t + 1) * p.Rp + r] - f[(t - 1) * p.Rp + r]) / 2.0;
      acc += d * d;
    }
    acc = sqrt(acc) / (double)p.n_rows;
  }
  p.ws2[(p.p2 + t) * p.Bp + b] = acc;
}

__global__ __launch_bounds__(256) void chg_unpack_kernel(ChangeParams p) {
  __shared__ double tile[64][65];
  const int64_t T = p.n_frames;
  const int64_t b0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int tt = ty; tt < 64; tt += 4) {
    const int64_t t = t0 + tt;
    tile[tt][tx] = (t < T) ? p.ws2[(p.p2 + t) * p.Bp + b0 + tx] : 0.0;
  }
  __syncthreads();
  for (int bb = ty; bb < 64; bb += 4) {
    const int64_t b = b0 + bb, t = t0 + tx;
    if (b < p.batch && t < T) p.out[b * T + t] = tile[tx][bb];
  }
}

// Generic row form of the same filter: [rows][n] float64 curves <-> the time-major workspace [n + 2 pad][Wp]
// (mm_sosfiltfilt_f64: applyFilter(filt='iir') of script/mfcc.py:29-135 / script/calc.py:23-129 on a batch of
// curves, e.g. amplitude envelopes or MFCC-change curves).
template <typename TIn>
__global__ __launch_bounds__(256) void sos_rows_pack_kernel(const TIn* __restrict__ x, int64_t rows, int64_t n,
                                                            int64_t x_stride, int pad, int64_t Wp, double* __restrict__ ws) {
  __shared__ double tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t r = r0 + rr, t = t0 + tx;
    tile[rr][tx] = (r < rows && t < n) ? (double)x[r * x_stride + t] : 0.0;
  }
  __syncthreads();
  for (int tt = ty; tt < 64; tt += 4) {
    const int64_t t = t0 + tt;
    if (t < n) ws[(pad + t) * Wp + r0 + tx] = tile[tx][tt];
  }
}

__global__ __launch_bounds__(256) void sos_rows_unpack_kernel(const double* __restrict__ ws, int64_t rows, int64_t n, int pad,
                                                              int64_t Wp, double* __restrict__ y) {
  __shared__ double tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int tt = ty; tt < 64; tt += 4) {
    const int64_t t = t0 + tt;
    tile[tt][tx] = (t < n) ? ws[(pad + t) * Wp + r0 + tx] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t r = r0 + rr, t = t0 + tx;
    if (r < rows && t < n) y[r * n + t] = tile[tx][rr];
  }
}

// Phi of the time-parallel form: the state the cascade reaches after one full chunk of zero input, per unit start state
template <int NS>
static void sos_chunk_phi(const SosCoef<NS>& c, int64_t chunk, double (&phi)[2 * NS][2 * NS]) {
  for (int b = 0; b < 2 * NS; ++b) {
    double z0[NS], z1[NS];
    for (int s2 = 0; s2 < NS; ++s2) { z0[s2] = 0.0; z1[s2] = 0.0; }
    (b & 1 ? z1 : z0)[b >> 1] = 1.0;
    for (int64_t i = 0; i < chunk; ++i) {
      double x = 0.0;
      for (int s2 = 0; s2 < NS; ++s2) {
        const double y = c.c[s2][0] * x + z0[s2];
        z0[s2] = c.c[s2][1] * x - c.c[s2][3] * y + z1[s2];
        z1[s2] = c.c[s2][2] * x - c.c[s2][4] * y;
        x = y;
      }
    }
    for (int s2 = 0; s2 < NS; ++s2) { phi[2 * s2][b] = z0[s2]; phi[2 * s2 + 1][b] = z1[s2]; }
  }
}

// ---- host side: pick the section count (identity sections pad up to an instantiated size) ----
template <int NS>
static void launch_sos(const SosFilt& f, double* ws, int64_t n, int64_t W, hipStream_t st) {
  SosCoef<NS> c;
  for (int s = 0; s < NS; ++s) {
    if (s < f.n_sec) {
      c.c[s][0] = f.c[s][0]; c.c[s][1] = f.c[s][1]; c.c[s][2] = f.c[s][2]; c.c[s][3] = f.c[s][4]; c.c[s][4] = f.c[s][5];
      c.zi[s][0] = f.zi[s][0]; c.zi[s][1] = f.zi[s][1];
    } else {   // identity section: y = 1*x + 0 exactly, state stays 0
      c.c[s][0] = 1.0; c.c[s][1] = c.c[s][2] = c.c[s][3] = c.c[s][4] = 0.0;
      c.zi[s][0] = c.zi[s][1] = 0.0;
    }
  }
  if constexpr (NS <= 4) if (n >= MM_SOS_CHUNK_MIN) {      // (more sections: LDS and kernel-argument size)
    SosChunk<NS> g;
    g.f = c;
    g.chunk = (n + MM_SOS_K - 1) / MM_SOS_K;
    sos_chunk_phi<NS>(c, g.chunk, g.phi);
    hipLaunchKernelGGL((chg_sos_chunk_kernel<NS>), dim3((unsigned)(W / 64)), dim3(64 * MM_SOS_K), 0, st, ws, n, W, g);
    return;
  }
  hipLaunchKernelGGL((chg_sos_kernel<NS>), dim3((unsigned)(W / 64)), dim3(64), 0, st, ws, n, W, c);
}

static void launch_sos_any(const SosFilt& f, double* ws, int64_t n, int64_t W, hipStream_t st) {
  if (f.n_sec <= 1) launch_sos<1>(f, ws, n, W, st);
  else if (f.n_sec == 2) launch_sos<2>(f, ws, n, W, st);
  else if (f.n_sec == 3) launch_sos<3>(f, ws, n, W, st);
  else if (f.n_sec == 4) launch_sos<4>(f, ws, n, W, st);
  else if (f.n_sec <= 6) launch_sos<6>(f, ws, n, W, st);
  else if (f.n_sec <= 8) launch_sos<8>(f, ws, n, W, st);
  else launch_sos<MM_MAX_SEC>(f, ws, n, W, st);
}


// ------------------------------------------------------------------------------------------
// Banded linear operator along time on [rows][n] float64 rows -- the derivative transforms of
// get_velocity (script/calc.py:593-650; SURVEY.md 8(f) row N2): np.gradient (repeated), Savitzky-Golay
// derivative with mode='interp' (interior = correlation with savgol_coeffs, first / last half-window
// samples = derivative of the polynomial fitted to the first / last window), findiff central stencils
// with one-sided stencils at the ends.  All of them are: interior y[i] = (sum_k c[k] x[i + off[k]]) /
// den_c, and for the n_edge first / last outputs a dense row over the first / last edge_w inputs.
// One thread per output sample; the taps travel in the kernel argument.
// ------------------------------------------------------------------------------------------
// RAGGED: a length per row (lens, DEVICE int64 [rows], clamped into [1, n_max]); the right edge rows sit at the row's own
// end, nothing at or behind it is loaded, the columns behind it become +0.0, and a row too short for the operator NaN.
template <bool RAGGED>
__global__ __launch_bounds__(256) void stencil_kernel(mm_stencil st, const double* __restrict__ x, int64_t rows,
                                                      int64_t n_max, int64_t in_stride, const int64_t* __restrict__ lens,
                                                      double* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * n_max) return;
  const int64_t r = idx / n_max, i = idx - r * n_max;
  int64_t n = n_max;
  if constexpr (RAGGED) {
    const int64_t nb = lens[r];
    n = nb < 1 ? 1 : (nb > n_max ? n_max : nb);
    if (i >= n) { y[idx] = 0.0; return; }
    // (st.reserved: the caller's own minimum, e.g. filtfilt's 3 n_taps + 1, where it exceeds the operator's)
    if (n < 2 * (int64_t)st.n_edge || n < st.edge_w || n < st.reserved) { y[idx] = __builtin_nan(""); return; }
  }
  const double* xr = x + r * in_stride;
  double acc = 0.0, den;
  if (i < st.n_edge) {
    for (int j = 0; j < st.edge_w; ++j) acc = fma(st.el[i][j], xr[j], acc);
    den = st.den_e;
  } else if (i >= n - st.n_edge) {
    const int e = (int)(i - (n - st.n_edge));
    for (int j = 0; j < st.edge_w; ++j) acc = fma(st.er[e][j], xr[n - st.edge_w + j], acc);
    den = st.den_e;
  } else {
    for (int k = 0; k < st.n_c; ++k) acc = fma(st.c[k], xr[i + st.off[k]], acc);
    den = st.den_c;
  }
  y[idx] = acc / den;
}
