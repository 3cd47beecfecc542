#pragma once
// The MFCC-change tail of mm_change.hip.inc as ONE launch with the clip resident in LDS (SURVEY.md 8(f) row N1;
// script/mfcc.py:392-427).  The time-major form streams a float64 workspace of (T + 2 pad) x rows through HBM six
// times (pack, pad, two filter directions, norm, ...: ~600 MB at 1024 clips x 12 rows x 1001 frames, 8 launches,
// 0.24 ms); here a workgroup owns a clip, reads its 48 KB of float32 MFCCs once and writes 8 KB of float64 curve:
//
//   rows [G][n1] f64 in LDS  <- mfcc rows of the clip (cast), odd extension by p1 on both sides
//   sosfiltfilt(sos1)           in place, time-parallel: thread = (row, chunk), K1 <= 64 chunks per row
//   curve [n2] f64 in LDS    <- sqrt(sum_rows d^2) / n_rows, d = np.gradient / Savitzky-Golay(3, 2) along time;
//                               summed in row order like chg_norm_kernel (groups of G rows when the clip's rows
//                               do not fit LDS at once: longer clips still take this path, G rows at a time)
//   sosfiltfilt(sos2)           the same routine on the one curve, K2 chunks
//   out [T] f64              <- curve
//
// One direction of the filter on a sequence cut into K chunks of `chunk` samples (the cascade is linear in (state,
// input), see chg_sos_chunk_kernel):
//   A  the state a chunk reaches from ZERO state is a weighted sum of its inputs, S = sum_i W[i] x[i], W[i] = the state
//      left `chunk - 1 - i` steps after a unit sample: 2 NS independent multiply-adds per sample instead of the
//      recursion's dependent chain of 7 NS operations (measured: 130 cycles per sample for the recursion at one wave
//      per SIMD).  W is the same for every chunk (the last chunk's end state is never used) and is read from LDS
//      at a wave-uniform address.
//   B  start states Z(k) = sum_{i<=k} Phi^(k-i) u(i), u(0) = zi * first sample, u(i) = S(i-1): a Hillis-Steele scan
//      over the chunks, step j adds Phi^(2^j) times the value 2^j chunks back (log2 K steps of one 2NS x 2NS
//      matrix-vector product; the sequential chain of chg_sos_chunk_kernel costs K of them on the last chunk).
//      K is a power of two <= 64 and the chunks of a sequence are consecutive lanes of ONE wave, so the values
//      travel by lane shuffles: no LDS buffer, no barrier (with an LDS buffer and two barriers a step cost ~1000
//      cycles, and the two scans were a third of the kernel): sos_lane_scan, mm_sos.hip.inc
//   C  every thread runs the recursion over its chunk from Z(k) and stores the outputs in place
// W and the powers of Phi come from the host through the first bytes of the caller's workspace (sos_scan_tables,
// uploaded by sos_tab_upload).
//
// Differs from the time-major kernels and from scipy's sequential recursion by rounding only (~1e-14 relative).
// Taken when both filters have <= MM_SCAN_MAX_SEC sections and one row (plus the curve) fits LDS; otherwise
// mm_mfcc_change_f64 keeps the time-major kernels.
#define MM_CLIP_MAXTHREADS 1024   // rows resident x chunks per row, rounded up to waves
#define MM_CLIP_LDS_MAX (160 * 1024)
#define MM_CLIP_KMAX 64           // chunks per sequence: a power of two, one wave holds a sequence's chunks
#define MM_CLIP_JMAX 6            // log2 of it
#define MM_CLIP_LU 16             // row loads in flight per thread

template <int NS>
struct ClipFilt {
  SosCoef<NS> f;
  int chunk, K, J;               // samples per chunk, chunks per sequence, scan steps = ceil(log2 K)
  int offW, offP;                // W [chunk][2 NS] and P [J][packed lower block triangle, by columns] in the table, in doubles
};

template <int NS>
struct ChgClipArgs {
  ClipFilt<NS> f1, f2;
  const double* tab;             // clip_tables, in the caller's workspace
  int tab_n;
  int n1, n2;                    // extended lengths T + 2 p1, T + 2 p2
  int pitch;                     // doubles between rows in LDS (>= n1)
  int G;                         // rows resident at once
  int has2;
  const int64_t* frames;         // ragged form only: [batch] valid frames per clip (device)
};

// forward + reverse pass in place over n_seq sequences of n samples at X + r * pitch; thread = (sequence, chunk),
// g.K a power of two <= 64.  tab: clip_tables (global memory, read through the scalar cache).  Every thread of the
// block must call it (barriers inside); ends with a barrier.
template <int NS>
__device__ __forceinline__ void clip_filtfilt(double* X, int pitch, int n, int n_seq, const ClipFilt<NS>& g,
                                              const MM_CONST double* tab MM_STAMP_FWD_DECL) {
  constexpr int U = 4, S2 = 2 * NS;
  const int task = threadIdx.x;
  const bool on = task < n_seq * g.K;
  const int r = on ? task >> g.J : 0, k = task & (g.K - 1);
  double* w = X + r * pitch;
  const int i0 = k * g.chunk;
  const int len = (!on || i0 >= n) ? 0 : (n - i0 < g.chunk ? n - i0 : g.chunk);
  const bool full = len == g.chunk;
  const MM_CONST double* W = tab + g.offW;      // wave-uniform addresses: scalar loads, operands in SGPRs
  const MM_CONST double* P = tab + g.offP;
  // a wave without a task only meets the barriers (the curve has one wave of tasks: the others would run A and B
  // on nothing and take issue slots from it)
  const bool wave_on = __builtin_amdgcn_readfirstlane(task) < n_seq * g.K;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (!wave_on) { __syncthreads(); continue; }
    const int step = pass ? -1 : 1;
    double* q0 = w + (pass ? n - 1 - i0 : i0);
    // ---- A: end state from zero state = sum_i W[i] x[i] (threads without a full chunk read one address, weight it,
    //         and nobody uses their sum)
    double Z[S2];
#pragma unroll
    for (int a = 0; a < S2; ++a) Z[a] = 0.0;
    {
      const double* q = full ? q0 : X;
      const int st = full ? step : 0;
#pragma unroll 4
      for (int i = 0; i < g.chunk; ++i) {
        const double x = q[i * st];
#pragma unroll
        for (int a = 0; a < S2; ++a) Z[a] = fma(W[i * S2 + a], x, Z[a]);
      }
    }
    MM_STAMP_REL(0)
    // ---- B: u(0) = zi * first sample, u(k) = S(k - 1); inclusive scan over the K lanes of the sequence
    //         (a lane without a source inside its sequence reads some other lane and ignores it)
    {
      const double x0 = w[pass ? n - 1 : 0];
      const int src = ((int)(threadIdx.x & 63) - 1) << 2;
#pragma unroll
      for (int a = 0; a < S2; ++a) {
        const double up = lane_from(src, Z[a]);
        Z[a] = k == 0 ? g.f.zi[a >> 1][a & 1] * x0 : up;
      }
    }
    sos_lane_scan<NS>(Z, P, 0, g.J, (int)(threadIdx.x & 63), k);
    MM_STAMP_REL(1)
    // ---- C: the recursion over the chunk from its start state, outputs in place (A read this chunk only: no barrier)
    {
      double z0[NS], z1[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) { z0[s] = Z[2 * s]; z1[s] = Z[2 * s + 1]; }
      double* q = q0;
      int i = 0;
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
    __syncthreads();                                 // the other direction cuts the sequence at other places
    MM_STAMP_REL(2)
  }
}

// RAG: the ragged form (mm_mfcc_change_ragged_f64).  p.n_frames is then the batch's T_max -- the row stride of mfcc and
// out, and what the host sized a.pitch, the chunk tables, K1 / K2, G and the LDS for -- and the workgroup works on its own
// T = frames[b] clamped into [1, T_max]: it loads T columns of every row, forms both odd extensions about frame T - 1,
// differentiates one-sidedly there and filters sequences of T + 2 pad samples (the chunks behind them have length 0:
// clip_filtfilt never uses the sum of a chunk that is not full).  Columns [T, T_max) of out are +0.0; a clip scipy
// refuses (T <= a padding length) gets NaN in [0, T).  Nothing behind column T of a row is ever loaded.
template <int NS, bool RAG>
__global__ __launch_bounds__(MM_CLIP_MAXTHREADS) void chg_clip_kernel(ChangeParams p, ChgClipArgs<NS> a) {
  extern __shared__ double clip_lds[];
  double* X = clip_lds;                                   // [G][pitch]
  double* C = X + (((size_t)a.G * a.pitch + 1) & ~(size_t)1);   // [n2]
  const MM_CONST double* tab = (const MM_CONST double*)a.tab;
  const int Tmax = (int)p.n_frames, tid = threadIdx.x, nthr = blockDim.x;
  const int64_t b = blockIdx.x;
  const double rows_d = (double)p.n_rows;
  int T = Tmax, n1 = a.n1, n2 = a.n2;
  if constexpr (RAG) {
    const int64_t v = a.frames[b];                        // one value per workgroup: every branch on T is uniform
    T = v < 1 ? 1 : (v > (int64_t)Tmax ? Tmax : (int)v);
    n1 = T + 2 * p.p1; n2 = T + 2 * p.p2;
    double* out = p.out + b * (int64_t)Tmax;
    const bool too_short = T <= (p.p1 > p.p2 ? p.p1 : p.p2);
    for (int t = tid; t < Tmax; t += nthr)
      if (t >= T) out[t] = 0.0; else if (too_short) out[t] = __builtin_nan("");
    if (too_short) return;                                // (before the first barrier, the whole workgroup)
  }
  MM_STAMP_BEGIN(12)
  for (int r0 = 0; r0 < p.n_rows; r0 += a.G) {
    const int g = p.n_rows - r0 < a.G ? p.n_rows - r0 : a.G;
    if constexpr (RAG) {
      // T columns of g rows that lie T_max apart: a wave per row, MM_CLIP_LU loads in flight per thread.  The row is
      // wave-uniform, so no (row, column) has to be found before a load can go: the flat walk below with the index found
      // first put that arithmetic in front of the loads instead of under them (measured: +15 % on this section, the
      // whole launch 0.109 ms against 0.104 ms single-length at 1024 x 12 x 1001; this form: 0.100 ms)
      const float* src = p.mfcc + (b * p.n_mfcc + p.first_row + r0) * (int64_t)Tmax;
      const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6, lane = tid & 63, n_waves = nthr >> 6;
      for (int r = wave; r < g; r += n_waves) {
        const float* row = src + (int64_t)r * Tmax;
        double* xr = X + r * a.pitch + p.p1;
        for (int t0 = lane; t0 < T; t0 += 64 * MM_CLIP_LU) {
          float v[MM_CLIP_LU];
#pragma unroll
          for (int u = 0; u < MM_CLIP_LU; ++u) {     // clamped index: no branch around a load, all in flight together
            const int t = t0 + 64 * u;
            v[u] = row[t < T ? t : T - 1];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < MM_CLIP_LU; ++u) {
            const int t = t0 + 64 * u;
            if (t < T) xr[t] = (double)v[u];
          }
        }
      }
    } else {
      // the g rows are one contiguous run of g * T floats; MM_CLIP_LU loads in flight per thread
      const float* src = p.mfcc + (b * p.n_mfcc + p.first_row + r0) * (int64_t)T;
      const int total = g * T;
      const float rT = 1.0f / (float)T;
      for (int e0 = tid; e0 < total; e0 += nthr * MM_CLIP_LU) {
        float v[MM_CLIP_LU];
#pragma unroll
        for (int u = 0; u < MM_CLIP_LU; ++u) {       // clamped index: no branch around a load, all in flight together
          const int e = e0 + u * nthr;
          v[u] = src[e < total ? e : total - 1];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < MM_CLIP_LU; ++u) {
          const int e = e0 + u * nthr;
          int r = (int)((float)e * rT);
          int t = e - r * T;
          if (t < 0) { --r; t += T; } else if (t >= T) { ++r; t -= T; }
          if (e < total) X[r * a.pitch + p.p1 + t] = (double)v[u];
        }
      }
    }
    __syncthreads();
    MM_STAMP_AT(0)
    for (int e = tid; e < 2 * p.p1 * g; e += nthr) {
      const int r = e / (2 * p.p1), j = e - r * 2 * p.p1;
      double* w = X + r * a.pitch;
      const int i = j < p.p1 ? j : T + j;
      auto x = [&](int64_t t) { return w[p.p1 + t]; };
      w[i] = odd_ext_f32(x, (int64_t)i, p.p1, (int64_t)T);          // the MFCC rows are float32: see odd_ext_f32
    }
    __syncthreads();
    MM_STAMP_AT(1)
    clip_filtfilt<NS>(X, a.pitch, n1, g, a.f1, tab MM_STAMP_FWD(2));
    // derivative along time, squared, added to the curve in row order.  Interior: both differentiators are
    // (x[t+1] - x[t-1]) / 2 (see chg_norm_kernel); the two end samples are left to two threads below.
    const bool last = r0 + g >= p.n_rows;
    for (int t = tid; t < T; t += nthr) {
      double acc = r0 ? C[p.p2 + t] : 0.0;
      const double* f = X + p.p1;
      if (t > 0 && t < T - 1) {
#pragma unroll 4
        for (int r = 0; r < g; ++r) {
          const double d = (f[r * a.pitch + t + 1] - f[r * a.pitch + t - 1]) / 2.0;
          acc += d * d;
        }
      } else {
        // first / last sample (T > padlen >= 6): np.gradient's one-sided difference, or the derivative of the
        // parabola through the three end samples (chg_end_deriv)
        const double* fe = f + (t == 0 ? 0 : T - 3);
#pragma unroll 4
        for (int r = 0; r < g; ++r) {
          const double x[3] = {fe[r * a.pitch], fe[r * a.pitch + 1], fe[r * a.pitch + 2]};
          const double d = chg_end_deriv(t == 0, p.sg, [&](int i) { return x[i]; });
          acc += d * d;
        }
      }
      C[p.p2 + t] = last ? sqrt(acc) / rows_d : acc;
    }
    __syncthreads();
    MM_STAMP_AT(5)
  }
  if (a.has2) {
    for (int j = tid; j < 2 * p.p2; j += nthr) {
      const int i = j < p.p2 ? j : T + j;
      auto x = [&](int64_t t) { return C[p.p2 + t]; };
      C[i] = odd_ext(x, (int64_t)i, p.p2, (int64_t)T);
    }
    __syncthreads();
    MM_STAMP_AT(6)
    clip_filtfilt<NS>(C, 0, n2, 1, a.f2, tab MM_STAMP_FWD(7));
  }
  double* out = p.out + b * (int64_t)Tmax;
  for (int t = tid; t < T; t += nthr) out[t] = C[p.p2 + t];
  MM_STAMP_AT(10)
  MM_STAMP_END_BLK(12, gridDim.x - 1)      // a late workgroup: the first ones also pay the cold misses of the tables
}

// ---- host side ----
// chunk length, scan depth and the two tables of one filter, appended to `tab`
template <int NS>
static void clip_filt_of(const SosFilt& f, int n, int K, ClipFilt<NS>* g, std::vector<double>& tab) {
  constexpr int S2 = 2 * NS, TRI = 2 * NS * (NS + 1);
  sos_coef_of<NS>(f, &g->f);
  g->K = K;
  g->chunk = ((n + K - 1) / K) | 1;          // odd: the chunks of a row start in different LDS banks
  g->J = 0;
  while ((1 << g->J) < K) ++g->J;            // (K is a power of two)
  const int J = std::max(g->J, 1);
  g->offW = (int)tab.size();
  g->offP = g->offW + g->chunk * S2;
  tab.resize((size_t)g->offP + (size_t)J * TRI);
  sos_scan_tables<NS>(g->f, g->chunk, J, tab.data() + g->offW, tab.data() + g->offP);
}

struct ClipShape { int G, K1, K2, pitch, threads; size_t lds; int64_t tab_n; };

// rows resident at once (in `groups` equal groups), chunk counts and workgroup size under an LDS budget; G = 0: no room
static ClipShape clip_shape_under(int n_rows, int64_t n1, int64_t n2, int64_t lds_max, int* groups) {
  ClipShape s;
  constexpr int64_t S2 = 2 * MM_SCAN_MAX_SEC;
  s.pitch = (int)(n1 | 1);
  s.K2 = MM_CLIP_KMAX;
  const int64_t room = lds_max / 8 - ((n2 + 1) & ~(int64_t)1) - 1;
  int64_t G = room > 0 ? room / s.pitch : 0;
  G = std::min<int64_t>(G, std::min<int64_t>(n_rows, MM_CLIP_MAXTHREADS / 2));
  s.G = (int)G; s.K1 = 0; s.lds = 0; s.tab_n = 0; s.threads = 0; *groups = 0;
  if (G < 1) return s;
  // equal groups (13 rows that fit 12 at a time: 7 + 6, not 12 + 1), the most chunks per row the workgroup takes
  *groups = (int)((n_rows + G - 1) / G);
  G = (n_rows + *groups - 1) / *groups;
  s.G = (int)G;
  s.K1 = MM_CLIP_KMAX;
  while (s.K1 > 1 && G * s.K1 > MM_CLIP_MAXTHREADS) s.K1 >>= 1;
  s.threads = (int)std::max<int64_t>((G * s.K1 + 63) / 64 * 64, s.K2);
  s.lds = (size_t)(((G * s.pitch + 1) & ~(int64_t)1) + ((n2 + 1) & ~(int64_t)1)) * 8;
  // upper bound of the table (MM_SCAN_MAX_SEC sections, deepest scan): what the workspace must hold
  s.tab_n = (((n1 + s.K1 - 1) / s.K1 | 1) + ((n2 + s.K2 - 1) / s.K2 | 1)) * S2 + 2 * MM_CLIP_JMAX * S2 * S2;
  return s;
}

// Half the LDS (two clips in flight per CU: the phases of one cover the latencies of the other, measured -9 % at
// 12 rows x 1001 frames) when that costs at most two groups of rows; otherwise as many rows at once as fit.
static ClipShape clip_shape(int n_rows, int64_t n1, int64_t n2) {
  int groups = 0;
  ClipShape s = clip_shape_under(n_rows, n1, n2, MM_CLIP_LDS_MAX / 2, &groups);
  if (s.G >= 1 && groups <= 2) return s;
  return clip_shape_under(n_rows, n1, n2, MM_CLIP_LDS_MAX, &groups);
}

// frames: the ragged form's lengths (q.n_frames, n1, n2 and s are then those of the batch's T_max)
template <int NS, bool RAG = false>
static int launch_chg_clip(const ChangeParams& q, const SosFilt& f1, const SosFilt& f2, const ClipShape& s, int64_t n1,
                           int64_t n2, double* d_tab, hipStream_t st, const int64_t* frames = nullptr) {
  static PerDeviceOnce attr_once;
  {
    const int rc = per_device_once(attr_once, "chg_clip_kernel", [] {
      return hipFuncSetAttribute((const void*)chg_clip_kernel<NS, RAG>, hipFuncAttributeMaxDynamicSharedMemorySize, MM_CLIP_LDS_MAX) == hipSuccess;
    });
    if (rc) return rc;
  }
  ChgClipArgs<NS> a;
  a.n1 = (int)n1; a.n2 = (int)n2; a.pitch = s.pitch; a.G = s.G; a.has2 = f2.n_sec > 0; a.frames = frames;
  std::vector<double> tab;
  tab.reserve((size_t)s.tab_n);
  clip_filt_of<NS>(f1, (int)n1, s.K1, &a.f1, tab);
  // the reference's default call filters rows and curve with the same Butterworth: one table (and one upload launch) then
  if (f2.n_sec == f1.n_sec && n2 == n1 && s.K2 == s.K1 && memcmp(f2.c, f1.c, sizeof(f1.c[0]) * f1.n_sec) == 0 &&
      memcmp(f2.zi, f1.zi, sizeof(f1.zi[0]) * f1.n_sec) == 0)
    a.f2 = a.f1;
  else
    clip_filt_of<NS>(f2, (int)n2, s.K2, &a.f2, tab);
  if ((int64_t)tab.size() > s.tab_n) return MM_ERR_WORKSPACE;     // (cannot happen: tab_n is the bound the caller's workspace was checked against)
  a.tab = d_tab; a.tab_n = (int)tab.size();
  sos_tab_upload(tab, d_tab, st);
  hipLaunchKernelGGL((chg_clip_kernel<NS, RAG>), dim3((unsigned)q.batch), dim3((unsigned)s.threads), s.lds, st, q, a);
  return MM_OK;
}
