#pragma once
// sosfiltfilt on a TIME-MAJOR float64 workspace [n + 2 pad][W]: the form of filters of more than MM_SCAN_MAX_SEC sections
// (mm_sosfiltfilt_f64) and of the change tail after mm_plan_set_fuse_tail(plan, 0) (mm_change.hip.inc).  The IIR recursion
// is sequential in time and independent per row, so ONE LANE OWNS ONE ROW and the rows of the whole batch run side by side:
//
//   tm_pack_kernel      rows [rows][n] (float64, float32, or the MFCC rows of clips) -> ws f64 [n + 2 pad][W], the row the
//                       fast index: every access of the recursion below is one coalesced 512-byte line per wave
//   chg_pad_kernel      odd extension of ws
//   chg_sos_kernel<NS>  in-place forward + reverse pass over ws; sections unrolled (coefficients and
//                       the 2*NS state words live in registers), samples fetched 8 time steps ahead
//   tm_unpack_kernel    ws -> rows f64 [rows][n]

// Row sources of tm_pack_kernel: where row r starts, and the type its samples cross the LDS tile in
template <typename TIn>
struct PlainRows {               // [rows][stride]: applyFilter(filt='iir') of script/mfcc.py:29-135 / script/calc.py:23-129 on
  typedef double tile_t;         // a batch of curves, e.g. amplitude envelopes or MFCC-change curves
  const TIn* x; int64_t stride;
  __device__ __forceinline__ const TIn* row(int64_t r) const { return x + r * stride; }
};
struct MfccRows {                // the change tail's first filter (mfcc_row)
  typedef float tile_t;
  const float* mfcc; int n_mfcc, first_row, n_rows; int64_t T;
  __device__ __forceinline__ const float* row(int64_t r) const { return mfcc_row(mfcc, n_mfcc, first_row, n_rows, T, r); }
};

// 64 rows x 64 time steps per block through an LDS tile: reads coalesced along time, writes along rows
template <class Src>
__global__ __launch_bounds__(256) void tm_pack_kernel(Src src, int64_t rows, int64_t n, int pad, int64_t Wp, double* __restrict__ ws) {
  __shared__ typename Src::tile_t tile[64][65];
  const int64_t r0 = (int64_t)blockIdx.x * 64, t0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t r = r0 + rr, t = t0 + tx;
    tile[rr][tx] = (r < rows && t < n) ? (typename Src::tile_t)src.row(r)[t] : 0;
  }
  __syncthreads();
  for (int tt = ty; tt < 64; tt += 4) {
    const int64_t t = t0 + tt;
    if (t < n) ws[(pad + t) * Wp + r0 + tx] = (double)tile[tx][tt];
  }
}

__global__ __launch_bounds__(256) void tm_unpack_kernel(const double* __restrict__ ws, int64_t rows, int64_t n, int pad,
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
  sos_coef_of<NS>(f, &c);
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
