// libmodmfcc: pYIN f0 tracking (librosa.pyin as get_f0(method='pyin') calls it, script/calc.py:386-592).  gfx950 only.
// Three kernels make the path ("Pitch"):
//   pyin_cmnd_kernel   frames -> cumulative-mean-normalised difference rows (float64; the energy terms in the input type)
//   pyin_cand_kernel   CMND row -> troughs, threshold / Boltzmann probabilities, pitch-bin candidates (a wave per frame)
//   pyin_viterbi_kernel candidates -> banded Viterbi over the 2 n_bins states (a workgroup per clip) + backtrack
// The host builds every constant table (modulation_mfcc_amd/pitch.py: scipy's beta / Boltzmann distributions, the
// transition matrix of librosa.sequence with numpy's own operations); the device never re-derives them.
#include "mm_common.h"

// numpy neither fuses a product into a sum nor re-associates: every square and sum below is computed
// as written (hipcc would otherwise contract y * y + c into an fma).  The autocorrelation, which numpy takes through a
// float64 FFT, uses explicit fma (rounding at 1e-16 relative either way).
#pragma clang fp contract(off)

namespace {

constexpr double kTiny = 2.2250738585072014e-308;       // np.finfo(np.float64).tiny
constexpr int kCmndThreads = 256;
constexpr int kAcfLags = 8;                             // lags per autocorrelation work item (sliding register window)
constexpr int kCandWaves = 4;
constexpr int kMaxChunks = 8;                           // trough slots per wave: 64 * kMaxChunks
constexpr int kVitThreads = 1024;
constexpr size_t kLdsMax = 64 * 1024;
constexpr int64_t kCmndChunkFrames = 16384;             // frames per CMND scratch chunk of the whole-path entry

__device__ __forceinline__ uint64_t lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// A length per row (the ragged entry points).  Row b has n_b = clamp(lens[b], 1, n_max) samples and T_b =
// mm_pyin_num_frames(p, n_b) frames inside the padded [rows][T_max] frame space; T_b is 0 when an uncentred row is shorter
// than a frame.  lens == nullptr: every row has n_max samples (every other entry point).
struct RowLens { const int64_t* lens; int64_t n_max; int frame_length; int hop; int pad2; };

__device__ __forceinline__ int64_t row_samples(const RowLens& r, int64_t row) {
  return min<int64_t>(max<int64_t>(r.lens[row], 1), r.n_max);
}
__device__ __forceinline__ int64_t row_frames(const RowLens& r, int64_t row) {
  const int64_t padded = row_samples(r, row) + r.pad2;
  return padded < r.frame_length ? 0 : 1 + (padded - r.frame_length) / r.hop;
}

template <class T> __device__ __forceinline__ T small_cut();
template <> __device__ __forceinline__ float small_cut<float>() { return 1e-6f; }
template <> __device__ __forceinline__ double small_cut<double>() { return 1e-6; }

// ---------------------------------------------------------------------------------------------------------------------
// CMND: a workgroup per F consecutive frames of one row.  The (F - 1) hop + win + max_period + 1 samples the frames
// read are staged once in LDS as float64 (exact for float32 input).  Lanes 0..F-1 then run numpy's sequential
// cumsum(y ** 2) of their frame in the input type (one lane per frame: 1.2 k dependent adds at the defaults), the whole
// workgroup the autocorrelation lags (kAcfLags per work item), and lanes 0..F-1 the sequential float64 cumulative mean.
// en[f][tau] holds, in turn: c_tau (the running sum), (T)(energy[0] + energy[tau]), d[tau], cmnd[tau].
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kCmndThreads) void pyin_cmnd_kernel(const T* __restrict__ x, int64_t n, int64_t x_stride,
                                                                 int64_t n_frames, int64_t tiles_per_row, int64_t tile0,
                                                                 int64_t frame0, int64_t frame_end, int F, int hop,
                                                                 int pad, int win, int min_p, int max_p, int span,
                                                                 RowLens rl, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double pyin_lds[];
  const int P1 = max_p + 1;
  double* ys = pyin_lds;                         // [span + kAcfLags]
  double* en = pyin_lds + span + kAcfLags;       // [F][P1]
  const int64_t tile = tile0 + blockIdx.x;
  const int64_t row = tile / tiles_per_row;
  const int64_t t0 = (tile - row * tiles_per_row) * F;
  int64_t nv = n, Tv = n_frames;                 // valid samples and frames of this row
  if (rl.lens) {
    nv = row_samples(rl, row);
    Tv = row_frames(rl, row);
    if (t0 >= Tv) return;                        // a tile of dead frames: uniform over the workgroup, ahead of every barrier
  }
  const int nf = (int)min<int64_t>((int64_t)F, Tv - t0);
  const T* xr = x + row * x_stride;
  const int64_t g0 = t0 * hop - pad;
  for (int i = threadIdx.x; i < span + kAcfLags; i += blockDim.x) {
    const int64_t g = g0 + i;
    ys[i] = (i < span && g >= 0 && g < nv) ? (double)xr[g] : 0.0;
  }
  __syncthreads();
  const int f = threadIdx.x;
  if (f < nf) {
    const double* y = ys + f * hop;
    double* e = en + f * P1;
    const T cut = small_cut<T>();
    T c = T(0), e0 = T(0);
    const int last = win + max_p;
    for (int j = 0; j <= last; ++j) {
      const T v = (T)y[j];
      c = c + v * v;
      if (j <= max_p) e[j] = (double)c;
      if (j >= win) {
        const int tau = j - win;
        T d = c - (T)e[tau];
        if (fabs(d) < cut) d = T(0);
        if (tau == 0) e0 = d;
        e[tau] = (double)(T)(e0 + d);
      }
    }
  }
  __syncthreads();
  const int nblk = (max_p + kAcfLags - 1) / kAcfLags;
  for (int w = threadIdx.x; w < nf * nblk; w += blockDim.x) {
    const int ff = w / nblk, tau0 = 1 + (w - ff * nblk) * kAcfLags;
    const double* y = ys + ff * hop;
    double acc[kAcfLags], win_[kAcfLags];
#pragma unroll
    for (int m = 0; m < kAcfLags; ++m) { acc[m] = 0.0; win_[m] = y[1 + tau0 + m]; }
    for (int j = 1; j <= win; ++j) {
      const double yj = y[j];
#pragma unroll
      for (int m = 0; m < kAcfLags; ++m) acc[m] = fma(yj, win_[m], acc[m]);
#pragma unroll
      for (int m = 0; m < kAcfLags - 1; ++m) win_[m] = win_[m + 1];
      win_[kAcfLags - 1] = y[j + 1 + tau0 + kAcfLags - 1];   // <= span + kAcfLags - 1 (zero tail)
    }
    double* e = en + ff * P1;
#pragma unroll
    for (int m = 0; m < kAcfLags; ++m) {
      const int tau = tau0 + m;
      if (tau <= max_p) {
        const double a = fabs(acc[m]) < 1e-6 ? 0.0 : acc[m];
        e[tau] = e[tau] - 2.0 * a;
      }
    }
  }
  __syncthreads();
  if (f < nf) {
    double* e = en + f * P1;
    double cs = 0.0;
    for (int tau = 1; tau <= max_p; ++tau) {
      const double d = e[tau];
      cs = cs + d;
      e[tau] = d / (cs / (double)tau + kTiny);
    }
  }
  __syncthreads();
  const int P = max_p - min_p + 1;
  const int64_t fr0 = row * n_frames + t0;       // flat frame index
  for (int i = threadIdx.x; i < nf * P; i += blockDim.x) {
    const int ff = i / P, k = i - ff * P;
    const int64_t fr = fr0 + ff;
    if (fr >= frame0 && fr < frame_end) out[(fr - frame0) * P + k] = en[ff * P1 + min_p + k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Candidates: a wave per frame.  Troughs are compacted in ascending-lag order into LDS; slot s of the wave's list is
// handled by lane s % 64 in chunk s / 64.  For each threshold k (ascending) a ballot of the troughs whose first
// threshold index k0 equals k gives, with mbcnt, every trough's Boltzmann position and the count n_k -- no per-frame
// prior matrix.  Then the global-minimum bonus, the candidate bins, librosa's duplicate rule (the later lag wins) and
// voiced_prob as numpy sums a column (ascending bin).
// ---------------------------------------------------------------------------------------------------------------------
struct CandArgs {
  const double* cmnd; int64_t frames; int P; int min_p; int n_thr; int R; int n_bins; int nbps;
  double sr, fmin, ntp;
  const double* thr; const double* beta; const double* beta_cum; const double* boltz;
  int32_t* count; int32_t* bins; double* probs; double* vp;
  RowLens rl; int64_t frame0, T_max;             // ragged: this launch starts at flat frame frame0 of [rows][T_max]
};

__global__ __launch_bounds__(64 * kCandWaves) void pyin_cand_kernel(CandArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pyin_lds[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int R = a.R;
  double* s_h = pyin_lds + wv * (2 * R);         // trough heights [R], then candidate probs [R]
  double* s_p = s_h + R;
  int* s_i = (int*)(pyin_lds + kCandWaves * 2 * R) + wv * (2 * R);   // trough lags [R], candidate bins [R]
  int* s_b = s_i + R;
  const int64_t fr = (int64_t)blockIdx.x * kCandWaves + wv;
  const bool live = fr < a.frames;
  // a frame behind its row's T_b has no CMND row (the scratch keeps whatever an earlier chunk left): count 0, voiced_prob 0
  bool rd = live;
  if (rd && a.rl.lens) {
    const int64_t gf = a.frame0 + fr, row = gf / a.T_max;
    rd = gf - row * a.T_max < row_frames(a.rl, row);
  }
  const int P = a.P;
  const double* x = a.cmnd + (rd ? fr : 0) * P;
  // 1. troughs (util.localmin with is_trough[0] = x[0] < x[1])
  int nt = 0;
  if (rd) {
    for (int base = 0; base < P; base += 64) {
      const int i = base + lane;
      bool tr = false;
      double xi = 0.0;
      if (i < P) {
        xi = x[i];
        if (i == 0) tr = xi < x[1];
        else if (i == P - 1) tr = xi < x[i - 1];
        else tr = xi < x[i - 1] && xi <= x[i + 1];
      }
      const uint64_t m = __ballot(tr);
      if (tr) {
        const int s = nt + __popcll(m & lanemask_lt());
        s_h[s] = xi;
        s_i[s] = i;
      }
      nt += __popcll(m);
    }
  }
  __syncthreads();
  // 2. probabilities of the troughs
  const int nc = (nt + 63) >> 6;
  double h[kMaxChunks], pr[kMaxChunks];
  int k0[kMaxChunks], pos[kMaxChunks];
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    const int s = c * 64 + lane;
    h[c] = 0.0; pr[c] = 0.0; pos[c] = 0; k0[c] = a.n_thr;
    if (c < nc && s < nt) {
      h[c] = s_h[s];
      int lo = 0, hi = a.n_thr;                    // k0 = #{m in 1..n_thr : !(h < thr[m])}
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (h[c] < a.thr[mid + 1]) hi = mid; else lo = mid + 1;
      }
      k0[c] = lo;
    }
  }
  if (nt > 0) {
    int N = 0;
    for (int k = 0; k < a.n_thr; ++k) {
      uint64_t m[kMaxChunks];
      int tot = 0;
#pragma unroll
      for (int c = 0; c < kMaxChunks; ++c) { m[c] = c < nc ? __ballot(k0[c] == k) : 0ull; tot += __popcll(m[c]); }
      if (tot == 0 && N == 0) continue;            // no trough below this threshold yet
      N += tot;
      const double bk = a.beta[k];
      const double* bz = a.boltz + (int64_t)N * R;
      int before = 0;
#pragma unroll
      for (int c = 0; c < kMaxChunks; ++c) {
        if (c < nc) {
          pos[c] += before + __popcll(m[c] & lanemask_lt());
          before += __popcll(m[c]);
          if (k0[c] <= k) pr[c] = pr[c] + bz[pos[c]] * bk;
        }
      }
    }
    // global minimum (np.argmin: first occurrence) takes no_trough_prob * sum(beta[:k0])
    double bh = INFINITY;
    int bs = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      const int s = c * 64 + lane;
      if (c < nc && s < nt && (h[c] < bh || (h[c] == bh && s < bs))) { bh = h[c]; bs = s; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double oh = __shfl_xor(bh, o, 64);
      const int os = __shfl_xor(bs, o, 64);
      if (oh < bh || (oh == bh && os < bs)) { bh = oh; bs = os; }
    }
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c)
      if (c < nc && c * 64 + lane == bs) pr[c] = pr[c] + a.ntp * a.beta_cum[k0[c]];
  }
  // 3. candidates: troughs with a nonzero probability, ascending lag -> pitch bins
  int ncand = 0;
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    if (c < nc) {
      const int s = c * 64 + lane;
      const bool on = s < nt && pr[c] != 0.0;
      int bin = 0;
      if (on) {
        const int i = s_i[s];
        double sh = 0.0;
        if (i > 0 && i < P - 1) {
          const double xm = x[i - 1], x0 = x[i], xp = x[i + 1];
          const double aa = xp + xm - 2.0 * x0;
          const double bb = (xp - xm) / 2.0;
          sh = fabs(bb) >= fabs(aa) ? 0.0 : -bb / aa;
        }
        const double period = (double)(a.min_p + i) + sh;
        const double f0 = a.sr / period;
        double bf = rint((double)(12 * a.nbps) * log2(f0 / a.fmin));
        bf = fmin(fmax(bf, 0.0), (double)a.n_bins);
        bin = (int)bf;
      }
      const uint64_t m = __ballot(on);
      if (on) {
        const int o = ncand + __popcll(m & lanemask_lt());
        s_b[o] = bin;
        s_p[o] = pr[c];
      }
      ncand += __popcll(m);
    }
  }
  __syncthreads();
  // 4. librosa's assignment: on a duplicate bin the later lag wins; bin n_bins is the first unvoiced row (overwritten)
  int nk = 0;
  for (int base = 0; base < ncand; base += 64) {
    const int o = base + lane;
    bool keep = false;
    int b = 0;
    double p = 0.0;
    if (o < ncand) {
      b = s_b[o]; p = s_p[o];
      keep = b < a.n_bins && (o == ncand - 1 || s_b[o + 1] != b);
    }
    const uint64_t m = __ballot(keep);
    if (keep) {
      const int q = nk + __popcll(m & lanemask_lt());
      a.bins[fr * R + q] = b;
      a.probs[fr * R + q] = p;
    }
    nk += __popcll(m);
  }
  if (live && lane == 0) {
    a.count[fr] = nk;
    // np.sum(obs[:n_bins], axis=0): a sequential column sum, ascending bin = descending lag
    double v = 0.0;
    for (int o = ncand - 1; o >= 0; --o) {
      const int b = s_b[o];
      if (b < a.n_bins && (o == ncand - 1 || s_b[o + 1] != b)) v = v + s_p[o];
    }
    a.vp[fr] = fmin(fmax(v, 0.0), 1.0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Viterbi: a workgroup per row, state j of 2 n_bins on thread j (and j + blockDim ...).  value rows double-buffered in
// LDS, log-observation rows triple-buffered (frame t is read while frame t + 1 gets its candidates and frame t + 2 its
// defaults), one barrier per frame.
//
// Dense equivalence.  librosa scans every source k for target j: value[k] + log(A[k, j] + tiny).  Outside the band
// A[k, j] == 0 (the band of transition_local, in both voicing halves of the kron), so those sources all add the same
// LT = log(tiny).  Let g be the lowest index maximising key[k] = fl(value[k] + LT).  Because rounding is monotone,
// key[g] = fl(max value + LT) >= key[k] for every k, and every k < g has key[k] < key[g].
//   * g outside j's band: among the out-of-band sources the dense argmax meets (key[g], g) first -- its largest sum
//     at its lowest index -- so adding that one candidate to the in-band scan reproduces the dense choice under the
//     (value desc, index asc) order.
//   * g inside j's band: its in-band sum fl(value[g] + log(A[g, j] + tiny)) >= key[g] since log(A + tiny) >= LT.
//     Every out-of-band k has key[k] <= key[g]; if equal, k > g.  So no out-of-band source beats the in-band
//     maximum, and on a tie an in-band index <= g wins.  Leaving them all out changes nothing.
// (g is the plain argmax of value whenever value + LT rounds injectively near the maximum -- nearly always; the key
// form also covers values a rounding step apart.)
// ---------------------------------------------------------------------------------------------------------------------
struct VitArgs {
  const int32_t* count; const int32_t* bins; const double* probs; const double* vp;
  int64_t T; int R; int n_bins; int H;
  double LT; double lp_voiced; double lp_unvoiced; double fill_na;
  const double* same; const double* cross; const double* freqs;
  int16_t* ptr; int32_t* states; double* f0; uint8_t* voiced;
  RowLens rl; double* vp_tail; int64_t* frames;  // ragged: T is T_max, the row runs its own T_b; frames[row] = T_b (or NULL)
};

__device__ __forceinline__ void vit_reduce(double& v, int& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

__device__ __forceinline__ void vit_obs_defaults(const VitArgs& a, double* lo, int64_t fr, int S) {
  const double lu = log((1.0 - a.vp[fr]) / (double)a.n_bins + kTiny);
  for (int j = threadIdx.x; j < S; j += blockDim.x) lo[j] = j < a.n_bins ? a.LT : lu;
}

__device__ __forceinline__ void vit_obs_cands(const VitArgs& a, double* lo, int64_t fr) {
  const int nk = a.count[fr];
  for (int q = threadIdx.x; q < nk; q += blockDim.x) lo[a.bins[fr * a.R + q]] = log(a.probs[fr * a.R + q] + kTiny);
}

// ragged rows: zeros in [T, TM) of every output
__device__ __forceinline__ void vit_zero_tail(const VitArgs& a, int64_t f0i, int64_t T, int64_t TM) {
  for (int64_t t = T + threadIdx.x; t < TM; t += blockDim.x) {
    a.f0[f0i + t] = 0.0;
    a.voiced[f0i + t] = 0;
    a.vp_tail[f0i + t] = 0.0;
    a.states[f0i + t] = 0;
  }
}

__global__ __launch_bounds__(kVitThreads) void pyin_viterbi_kernel(VitArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pyin_lds[];
  const int nb = a.n_bins, S = 2 * nb, H = a.H, W = 2 * H + 1;
  double* val = pyin_lds;                   // [2][S]
  double* lob = pyin_lds + 2 * S;           // [3][S]
  double* red_v = lob + 3 * S;              // [2][16]
  int* red_i = (int*)(red_v + 32);          // [2][16]
  const int64_t row = blockIdx.x, TM = a.T;
  const int64_t T = a.rl.lens ? row_frames(a.rl, row) : TM;     // every prefetch below stops at T: a dead frame's record
  const int64_t f0i = row * TM;                                 // may hold any bin index
  int16_t* ptr = a.ptr + row * TM * S;
  if (a.rl.lens) {
    if (a.frames && threadIdx.x == 0) a.frames[row] = T;
    vit_zero_tail(a, f0i, T, TM);
    if (T == 0) return;                                         // uniform over the workgroup, ahead of every barrier
  }
  const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
  // frame 0 (and the candidates of frame 1, defaults of frame 1)
  vit_obs_defaults(a, lob, f0i, S);
  if (T > 1) vit_obs_defaults(a, lob + S, f0i + 1, S);
  __syncthreads();
  vit_obs_cands(a, lob, f0i);
  if (T > 1) vit_obs_cands(a, lob + S, f0i + 1);
  __syncthreads();
  {
    double kv = -INFINITY; int ki = 0x7fffffff;
    for (int j = threadIdx.x; j < S; j += blockDim.x) {
      const double v = lob[j] + (j < nb ? a.lp_voiced : a.lp_unvoiced);
      val[j] = v;
      const double key = v + a.LT;
      if (key > kv || (key == kv && j < ki)) { kv = key; ki = j; }
    }
    vit_reduce(kv, ki);
    if (lane == 0) { red_v[wv] = kv; red_i[wv] = ki; }
    if (T > 2) vit_obs_defaults(a, lob + 2 * S, f0i + 2, S);
  }
  __syncthreads();
  for (int64_t t = 1; t < T; ++t) {
    const int pb = (int)((t - 1) & 1), cb = (int)(t & 1);
    const double* vp = val + pb * S;
    double* vc = val + cb * S;
    const double* lo = lob + (t % 3) * S;
    // g: lowest index of the largest fl(value + LT) of frame t - 1
    double gv = red_v[pb * 16]; int g = red_i[pb * 16];
    for (int w = 1; w < nw; ++w) {
      const double ov = red_v[pb * 16 + w]; const int oi = red_i[pb * 16 + w];
      if (ov > gv || (ov == gv && oi < g)) { gv = ov; g = oi; }
    }
    const int gb = g < nb ? g : g - nb;
    double kv = -INFINITY; int ki = 0x7fffffff;
    for (int j = threadIdx.x; j < S; j += blockDim.x) {
      const int jb = j < nb ? j : j - nb;
      const bool uv = j >= nb;
      const int k_lo = max(jb - H, 0), k_hi = min(jb + H, nb - 1);
      const double* tv = (uv ? a.cross : a.same) + (int64_t)jb * W + (H - jb);   // indexed by source bin k
      const double* tu = (uv ? a.same : a.cross) + (int64_t)jb * W + (H - jb);
      double best = -INFINITY; int bi = 0x7fffffff;
      for (int k = k_lo; k <= k_hi; ++k) {                 // voiced sources, ascending
        const double c = vp[k] + tv[k];
        if (c > best) { best = c; bi = k; }
      }
      for (int k = k_lo; k <= k_hi; ++k) {                 // unvoiced sources, ascending
        const double c = vp[nb + k] + tu[k];
        if (c > best) { best = c; bi = nb + k; }
      }
      if (gb < k_lo || gb > k_hi) {
        if (gv > best || (gv == best && g < bi)) { best = gv; bi = g; }
      }
      ptr[t * S + j] = (int16_t)bi;
      const double v = lo[j] + best;
      vc[j] = v;
      const double key = v + a.LT;
      if (key > kv || (key == kv && j < ki)) { kv = key; ki = j; }
    }
    vit_reduce(kv, ki);
    if (lane == 0) { red_v[cb * 16 + wv] = kv; red_i[cb * 16 + wv] = ki; }
    if (t + 1 < T) vit_obs_cands(a, lob + ((t + 1) % 3) * S, f0i + t + 1);
    if (t + 2 < T) vit_obs_defaults(a, lob + ((t + 2) % 3) * S, f0i + t + 2, S);
    __syncthreads();
  }
  // last state: np.argmax(value[-1]) (plain values, lowest index)
  {
    const double* vl = val + ((T - 1) & 1) * S;
    double kv = -INFINITY; int ki = 0x7fffffff;
    for (int j = threadIdx.x; j < S; j += blockDim.x)
      if (vl[j] > kv || (vl[j] == kv && j < ki)) { kv = vl[j]; ki = j; }
    vit_reduce(kv, ki);
    if (lane == 0) { red_v[wv] = kv; red_i[wv] = ki; }
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    double gv = red_v[0]; int s = red_i[0];
    for (int w = 1; w < nw; ++w)
      if (red_v[w] > gv || (red_v[w] == gv && red_i[w] < s)) { gv = red_v[w]; s = red_i[w]; }
    for (int64_t t = T - 1; t >= 0; --t) {
      a.states[f0i + t] = s;
      const bool on = s < nb;
      a.voiced[f0i + t] = on ? 1 : 0;
      a.f0[f0i + t] = on ? a.freqs[s] : a.fill_na;
      if (t > 0) s = ptr[t * S + s];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int cmnd_tile_frames(const mm_pyin_params* p, int* span_out, size_t* lds_out) {
  const int P1 = p->max_period + 1;
  const int base = p->win_length + p->max_period + 1;
  for (int F = 16; F >= 1; --F) {
    const int span = (F - 1) * p->hop_length + base;
    const size_t lds = sizeof(double) * ((size_t)span + kAcfLags + (size_t)F * P1);
    if (lds <= kLdsMax) { *span_out = span; *lds_out = lds; return F; }
  }
  return 0;
}

int64_t n_lags(const mm_pyin_params* p) { return p->max_period - p->min_period + 1; }

size_t vit_lds(const mm_pyin_params* p) { return sizeof(double) * (5 * 2 * (size_t)p->n_bins + 32) + sizeof(int) * 32; }

size_t records_bytes(const mm_pyin_params* p, int64_t frames) {
  return (size_t)frames * (size_t)p->max_troughs * (sizeof(int32_t) + sizeof(double)) +
         (size_t)frames * (sizeof(int32_t) + sizeof(double));
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

RowLens row_lens(const mm_pyin_params* p, const int64_t* d_lens, int64_t n_max) {
  return RowLens{d_lens, n_max, p->frame_length, p->hop_length, p->center ? 2 * (p->frame_length / 2) : 0};
}

template <class T>
int launch_cmnd(const mm_pyin_params* p, const T* d_x, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_lens,
                int64_t frame0, int64_t frame_end, double* d_out, hipStream_t st) {
  int span = 0;
  size_t lds = 0;
  const int F = cmnd_tile_frames(p, &span, &lds);
  const int64_t nT = mm_pyin_num_frames(p, n);
  const int64_t tpr = (nT + F - 1) / F;
  // tiles covering flat frames [frame0, frame_end)
  const int64_t r0 = frame0 / nT, r1 = (frame_end - 1) / nT;
  const int64_t tile0 = r0 * tpr + (frame0 - r0 * nT) / F;
  const int64_t tile1 = r1 * tpr + (frame_end - 1 - r1 * nT) / F + 1;
  (void)rows;
  static PerDeviceOnce once;
  int rc = per_device_once(once, "pyin_cmnd_kernel", [] {
    return hipFuncSetAttribute((const void*)pyin_cmnd_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) == hipSuccess;
  });
  if (rc) return rc;
  for (int64_t tb = tile0; tb < tile1; tb += 1 << 30) {
    const int64_t nt = std::min<int64_t>(tile1 - tb, 1 << 30);
    hipLaunchKernelGGL(pyin_cmnd_kernel<T>, dim3((unsigned)nt), dim3(kCmndThreads), lds, st, d_x, n, x_stride, nT, tpr, tb,
                       frame0, frame_end, F, p->hop_length, p->center ? p->frame_length / 2 : 0, p->win_length,
                       p->min_period, p->max_period, span, row_lens(p, d_lens, n), d_out);
    HIP_TRY(hipGetLastError());
  }
  return MM_OK;
}

int launch_cand(const mm_pyin_params* p, const mm_pyin_tables* tb, const double* d_cmnd, int64_t frames, int32_t* d_count,
                int32_t* d_bins, double* d_probs, double* d_vp, const int64_t* d_lens, int64_t n_max, int64_t frame0,
                hipStream_t st) {
  CandArgs a;
  a.rl = row_lens(p, d_lens, n_max); a.frame0 = frame0; a.T_max = d_lens ? mm_pyin_num_frames(p, n_max) : 1;
  a.cmnd = d_cmnd; a.frames = frames; a.P = (int)n_lags(p); a.min_p = p->min_period; a.n_thr = p->n_thresholds;
  a.R = p->max_troughs; a.n_bins = p->n_bins; a.nbps = p->nbps; a.sr = p->sr; a.fmin = p->fmin; a.ntp = p->no_trough_prob;
  a.thr = tb->thresholds; a.beta = tb->beta_probs; a.beta_cum = tb->beta_cum; a.boltz = tb->boltzmann;
  a.count = d_count; a.bins = d_bins; a.probs = d_probs; a.vp = d_vp;
  const size_t lds = (size_t)kCandWaves * 2 * a.R * (sizeof(double) + sizeof(int));
  static PerDeviceOnce once;
  int rc = per_device_once(once, "pyin_cand_kernel", [] {
    return hipFuncSetAttribute((const void*)pyin_cand_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) == hipSuccess;
  });
  if (rc) return rc;
  const int64_t blocks = (frames + kCandWaves - 1) / kCandWaves;
  if (blocks > 0x7fffffff) return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pyin_cand_kernel, dim3((unsigned)blocks), dim3(64 * kCandWaves), lds, st, a);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

int launch_vit(const mm_pyin_params* p, const mm_pyin_tables* tb, const int32_t* d_count, const int32_t* d_bins,
               const double* d_probs, double* d_vp, int64_t rows, int64_t T, int32_t* d_states, double* d_f0,
               uint8_t* d_voiced, int16_t* d_ptr, const int64_t* d_lens, int64_t n_max, int64_t* d_frames, hipStream_t st) {
  VitArgs a;
  a.rl = row_lens(p, d_lens, n_max); a.vp_tail = d_vp; a.frames = d_frames;
  a.count = d_count; a.bins = d_bins; a.probs = d_probs; a.vp = d_vp; a.T = T; a.R = p->max_troughs; a.n_bins = p->n_bins;
  a.H = p->band_h; a.LT = p->log_tiny; a.lp_voiced = p->log_p_init[0]; a.lp_unvoiced = p->log_p_init[1];
  a.fill_na = p->fill_na; a.same = tb->log_same; a.cross = tb->log_cross; a.freqs = tb->freqs;
  a.ptr = d_ptr; a.states = d_states; a.f0 = d_f0; a.voiced = d_voiced;
  static PerDeviceOnce once;
  int rc = per_device_once(once, "pyin_viterbi_kernel", [] {
    return hipFuncSetAttribute((const void*)pyin_viterbi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) == hipSuccess;
  });
  if (rc) return rc;
  const int S = 2 * p->n_bins;
  const int threads = std::min(kVitThreads, (S + 63) / 64 * 64);
  hipLaunchKernelGGL(pyin_viterbi_kernel, dim3((unsigned)rows), dim3(threads), vit_lds(p), st, a);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

bool tables_ok(const mm_pyin_tables* t) {
  return t && t->thresholds && t->beta_probs && t->beta_cum && t->boltzmann && t->log_same && t->log_cross && t->freqs;
}

template <class T>
int pyin_whole(const mm_pyin_params* p, const mm_pyin_tables* tb, const T* d_x, int64_t rows, int64_t n, int64_t x_stride,
               bool ragged, const int64_t* d_lens, int64_t* d_frames, double* d_f0, uint8_t* d_voiced, double* d_vp,
               int32_t* d_states, void* d_ws, size_t ws_bytes, void* stream) {
  int rc = mm_pyin_check(p);
  if (rc) return rc;
  if (ragged && !d_lens) return MM_ERR_INVALID_ARG;
  if (!tables_ok(tb) || !d_x || !d_f0 || !d_voiced || !d_vp || !d_states || !d_ws || rows < 1 || rows > 0x7fffffff ||
      n < 1 || x_stride < n)
    return MM_ERR_INVALID_ARG;
  const int64_t nT = mm_pyin_num_frames(p, n);
  if (nT < 1) return MM_ERR_INVALID_ARG;
  if (ws_bytes < mm_pyin_workspace_bytes(p, rows, n)) return MM_ERR_WORKSPACE;
  const int64_t frames = rows * nT, R = p->max_troughs;
  char* w = (char*)d_ws;
  int16_t* ptr = (int16_t*)w;              w += align256((size_t)frames * 2 * p->n_bins * sizeof(int16_t));
  int32_t* count = (int32_t*)w;            w += align256((size_t)frames * sizeof(int32_t));
  int32_t* bins = (int32_t*)w;             w += align256((size_t)frames * R * sizeof(int32_t));
  double* probs = (double*)w;              w += align256((size_t)frames * R * sizeof(double));
  double* cmnd = (double*)w;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunk = std::min<int64_t>(frames, kCmndChunkFrames);
  for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
    const int64_t f1 = std::min(frames, f0 + chunk);
    rc = launch_cmnd<T>(p, d_x, rows, n, x_stride, d_lens, f0, f1, cmnd, st);
    if (rc) return rc;
    rc = launch_cand(p, tb, cmnd, f1 - f0, count + f0, bins + f0 * R, probs + f0 * R, d_vp + f0, d_lens, n, f0, st);
    if (rc) return rc;
  }
  return launch_vit(p, tb, count, bins, probs, d_vp, rows, nT, d_states, d_f0, d_voiced, ptr, d_lens, n, d_frames, st);
}

}  // namespace

extern "C" {

int mm_pyin_check(const mm_pyin_params* p) {
  if (!p) return MM_ERR_INVALID_ARG;
  if (!(p->sr > 0) || !(p->fmin > 0) || !(p->fmin < p->fmax) || p->fmax > p->sr / 2) return MM_ERR_INVALID_ARG;
  if (p->frame_length < 3 || p->win_length < 1 || p->win_length >= p->frame_length || p->hop_length < 1)
    return MM_ERR_INVALID_ARG;
  if (p->min_period < 1 || p->max_period > p->frame_length - p->win_length - 1 || p->max_period < p->min_period + 2)
    return MM_ERR_INVALID_ARG;
  if (p->n_thresholds < 1 || p->nbps < 1 || p->n_bins < 1 || p->band_h < 0 || p->center < 0 || p->center > 1)
    return MM_ERR_INVALID_ARG;
  if (p->max_troughs < (p->max_period - p->min_period + 2) / 2 + 1) return MM_ERR_INVALID_ARG;
  // device limits: trough slots of a wave, LDS of the candidate / Viterbi / CMND kernels, 16-bit back-pointers
  if (p->max_troughs > 64 * kMaxChunks) return MM_ERR_UNSUPPORTED;
  if ((size_t)kCandWaves * 2 * p->max_troughs * (sizeof(double) + sizeof(int)) > kLdsMax) return MM_ERR_UNSUPPORTED;
  if (vit_lds(p) > kLdsMax || 2 * p->n_bins > 32767) return MM_ERR_UNSUPPORTED;
  int span = 0;
  size_t lds = 0;
  if (cmnd_tile_frames(p, &span, &lds) < 1) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

int64_t mm_pyin_num_frames(const mm_pyin_params* p, int64_t n) {
  if (!p || n < 1 || p->hop_length < 1) return 0;
  const int64_t padded = n + (p->center ? 2 * (int64_t)(p->frame_length / 2) : 0);
  if (padded < p->frame_length) return 0;
  return 1 + (padded - p->frame_length) / p->hop_length;
}

size_t mm_pyin_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n) {
  if (mm_pyin_check(p) || rows < 1) return 0;
  const int64_t frames = rows * mm_pyin_num_frames(p, n);
  if (frames < 1) return 0;
  const int64_t R = p->max_troughs;
  return align256((size_t)frames * 2 * p->n_bins * sizeof(int16_t)) + align256((size_t)frames * sizeof(int32_t)) +
         align256((size_t)frames * R * sizeof(int32_t)) + align256((size_t)frames * R * sizeof(double)) +
         (size_t)std::min<int64_t>(frames, kCmndChunkFrames) * n_lags(p) * sizeof(double);
}

int mm_pyin_cmnd(const mm_pyin_params* p, const void* d_x, int32_t dtype, int64_t rows, int64_t n, int64_t x_stride,
                 double* d_cmnd, void* stream) {
  int rc = mm_pyin_check(p);
  if (rc) return rc;
  if (!d_x || !d_cmnd || rows < 1 || n < 1 || x_stride < n || (dtype != 0 && dtype != 1)) return MM_ERR_INVALID_ARG;
  const int64_t T = mm_pyin_num_frames(p, n);
  if (T < 1) return MM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) return launch_cmnd<float>(p, (const float*)d_x, rows, n, x_stride, nullptr, 0, rows * T, d_cmnd, st);
  return launch_cmnd<double>(p, (const double*)d_x, rows, n, x_stride, nullptr, 0, rows * T, d_cmnd, st);
}

int mm_pyin_candidates(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_cmnd, int64_t frames,
                       int32_t* d_count, int32_t* d_bins, double* d_probs, double* d_voiced_prob, void* stream) {
  int rc = mm_pyin_check(p);
  if (rc) return rc;
  if (!tables_ok(t) || !d_cmnd || frames < 1 || !d_count || !d_bins || !d_probs || !d_voiced_prob) return MM_ERR_INVALID_ARG;
  return launch_cand(p, t, d_cmnd, frames, d_count, d_bins, d_probs, d_voiced_prob, nullptr, 0, 0, (hipStream_t)stream);
}

size_t mm_pyin_decode_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n_frames) {
  if (mm_pyin_check(p) || rows < 1 || n_frames < 1) return 0;
  return (size_t)rows * n_frames * 2 * p->n_bins * sizeof(int16_t);
}

int mm_pyin_decode(const mm_pyin_params* p, const mm_pyin_tables* t, const int32_t* d_count, const int32_t* d_bins,
                   const double* d_probs, const double* d_voiced_prob, int64_t rows, int64_t n_frames, int32_t* d_states,
                   double* d_f0, uint8_t* d_voiced, void* d_ws, size_t ws_bytes, void* stream) {
  int rc = mm_pyin_check(p);
  if (rc) return rc;
  if (!tables_ok(t) || !d_count || !d_bins || !d_probs || !d_voiced_prob || rows < 1 || rows > 0x7fffffff || n_frames < 1 ||
      !d_states || !d_f0 || !d_voiced || !d_ws)
    return MM_ERR_INVALID_ARG;
  if (ws_bytes < mm_pyin_decode_workspace_bytes(p, rows, n_frames)) return MM_ERR_WORKSPACE;
  return launch_vit(p, t, d_count, d_bins, d_probs, const_cast<double*>(d_voiced_prob), rows, n_frames, d_states, d_f0,
                    d_voiced, (int16_t*)d_ws, nullptr, 0, nullptr, (hipStream_t)stream);
}

int mm_pyin_f32(const mm_pyin_params* p, const mm_pyin_tables* t, const float* d_x, int64_t rows, int64_t n,
                int64_t x_stride, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob, int32_t* d_states, void* d_ws,
                size_t ws_bytes, void* stream) {
  return pyin_whole<float>(p, t, d_x, rows, n, x_stride, false, nullptr, nullptr, d_f0, d_voiced, d_voiced_prob, d_states,
                           d_ws, ws_bytes, stream);
}

int mm_pyin_f64(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_x, int64_t rows, int64_t n,
                int64_t x_stride, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob, int32_t* d_states, void* d_ws,
                size_t ws_bytes, void* stream) {
  return pyin_whole<double>(p, t, d_x, rows, n, x_stride, false, nullptr, nullptr, d_f0, d_voiced, d_voiced_prob, d_states,
                            d_ws, ws_bytes, stream);
}

size_t mm_pyin_ragged_workspace_bytes(const mm_pyin_params* p, int64_t rows, int64_t n_max) {
  return mm_pyin_workspace_bytes(p, rows, n_max);           // the frame space is [rows][T_max]
}

int mm_pyin_ragged_f32(const mm_pyin_params* p, const mm_pyin_tables* t, const float* d_x, int64_t rows, int64_t n_max,
                       int64_t x_stride, const int64_t* d_lengths, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob,
                       int32_t* d_states, int64_t* d_frames, void* d_ws, size_t ws_bytes, void* stream) {
  return pyin_whole<float>(p, t, d_x, rows, n_max, x_stride, true, d_lengths, d_frames, d_f0, d_voiced, d_voiced_prob,
                           d_states, d_ws, ws_bytes, stream);
}

int mm_pyin_ragged_f64(const mm_pyin_params* p, const mm_pyin_tables* t, const double* d_x, int64_t rows, int64_t n_max,
                       int64_t x_stride, const int64_t* d_lengths, double* d_f0, uint8_t* d_voiced, double* d_voiced_prob,
                       int32_t* d_states, int64_t* d_frames, void* d_ws, size_t ws_bytes, void* stream) {
  return pyin_whole<double>(p, t, d_x, rows, n_max, x_stride, true, d_lengths, d_frames, d_f0, d_voiced, d_voiced_prob,
                            d_states, d_ws, ws_bytes, stream);
}

}  // extern "C"
