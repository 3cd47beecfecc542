#pragma once
// Hilbert envelope |scipy.signal.hilbert(x)| of whole clips (SURVEY.md 8(f) row N3; script/calc.py:286).
// Included by mm_side.hip.
//
// scipy transforms the clip at its OWN length n (an arbitrary integer: 160 000 = 2^8 * 5^4 for a 10 s clip),
// zeroes the negative frequencies, doubles the positive ones and transforms back.  Here both length-n DFTs
// are Bluestein chirp-z transforms: with w[k] = exp(-i pi k^2 / n),
//
//     X[k] = w[k] * sum_j (x[j] w[j]) * conj(w[k - j])
//
// is a linear convolution, evaluated as a circular one of length M = 2^p >= 2n - 1 with power-of-two FFTs.
// Lengths whose only prime factors are 2, 3, 5 and 7 -- sample counts like 160 000 = 2^8 5^4, 480 000, 441 000 --
// skip the chirps: the FFT below takes them directly (M = n), a tenth of the Bluestein traffic.  The FFT is a
// Stockham autosort transform in global memory: one pass per radix (16, 8 / 4 / 2, 9, 3, 25, 5, 49, 7; pairs of
// radix-16 or radix-25 passes fused into one launch, hb_pass2_kernel), each thread one radix-R butterfly in registers --
//
//     pass with radix R after passes of total radix Ns:   j in [0, M/R),  k = j mod Ns
//         v[t] = in[j + t M/R] * W_(Ns R)^(k t),   V = DFT_R(v),   out[(j - k) R + k + u Ns] = V[u]
//
// -- reads are unit-stride across threads; writes are runs of Ns points (the first pass, Ns = 1, goes through an
// LDS transpose so that its stores are unit-stride too; radix <= 16, and so does every pass whose Ns divides the
// workgroup).  Twiddles W_M^e come from two float64 tables (e = 1024 hi + lo: one complex product), built on the
// device with sincospi: two exact values per butterfly, the rest from short products of them.  Only the FORWARD transform exists: every inverse is
// conj(FFT(conj(.))), with the conjugations folded into the pointwise kernels between the transforms.
// Everything is templated on the scalar type: float32 clips are transformed in complex64, float64 ones in
// complex128, as scipy does; the chirp spectrum is always computed in float64 and rounded once.
//
// TWO CLIPS PER COMPLEX TRANSFORM.  The clips are real: clip a goes into the real part and clip b into the imaginary
// part of one complex sequence.  The spectrum mask is linear, so the masked inverse transform of FFT(a + i b) is
// z_a + i z_b with z = x + i H(x) the analytic signals: its real part is a - H(b), its imaginary part H(a) + b, and
// with a and b at hand (re-read by the last pass) H(a) = Im - b, H(b) = a - Re -- both envelopes from one forward and
// one inverse transform, half the passes' traffic and arithmetic per clip.  The rounding noise of a pair is relative
// to the larger of its two clips, so each clip is first scaled by a power of two (exact) that brings its maximum
// into [0.5, 1): a per-row maximum (hb_rowmax_kernel, one read of the input) costs an eighth of what the pairing saves.
//
// The pointwise steps between the transforms (chirp products, the spectrum mask, the magnitude) ride on the
// first / last pass of the neighbouring transform (HbIo), so the traffic per clip is that of the passes alone:
// (2 direct or 4 Bluestein transforms) x passes x 2 x M x sizeof(complex) -- HBM-bound streaming kernels.
//
// A LENGTH PER CLIP (mm_hilbert_envelope_ragged).  Clips of different lengths cannot share a mixed-radix plan, but they
// share the chirp identity: one M = 2^p >= 2 n_max - 1 for all rows, each row with its own chirp exp(-i pi k^2 / n_b) and
// chirp spectrum, both written per call (hb_chirp_ragged_kernel + one batched FFT in the clips' precision).  The passes
// are the RG = true instantiations of the same kernels: hb_row_setup loads the row's n, w, bhat and scale once per
// workgroup.  One clip per transform -- two clips could share one only if they shared a chirp.
//
// SHARED PIECES.  Device, as MACROS (below: MM_HB_...): FUSED_ITEM (the XCD-ordered (row, c) of the two fused kernels),
// TWIDDLE_DFT (twiddle + DFT of all four pass kernels), COLUMN_POWERS / EXCHANGE / STAGE_B (the rest of the radix-R^2
// butterfly: hb_pass2_kernel once, hb_mid2_kernel twice), STORE_RUN2 / STORE_RUN (the staged stores of the fused / the
// single-radix kernels); as a function hb_chirp_phase (both chirp kernels).  Host: hb_with_radix (every launch of the four
// pass kernels, dense and ragged), hb_fused_grid, hb_chirp_envelope (the four chirp transforms of mm_hilbert_envelope and
// mm_hilbert_envelope_ragged).  Macros, because an inlined function around these pieces is optimised on its own first: with
// a complex product inside, the operands of the sum of two products in hb_mul come out in the other order and the backend
// contracts the other product into the FMA (the last bit of the results changes); without one, the integer code and the
// register allocation of the kernel still move (docs/experiments.md, "Hilbert FFT: shared pieces").

#include <type_traits>

#include "mm_hb_math.h"

#define MM_HB_THREADS 128
#define MM_HB_TWLO 1024

__device__ __forceinline__ hb_c<double> hb_twiddle(const hb_c<double>* __restrict__ lo, const hb_c<double>* __restrict__ hi,
                                                   int64_t e) {
  return hb_mul(hi[e >> 10], lo[e & (MM_HB_TWLO - 1)]);
}

// What the first pass of a transform reads and the last one writes: the pointwise steps between the
// transforms of an envelope (chirp products, spectrum mask, conjugations, magnitude) ride on the passes.
enum { HB_IN_COMPLEX = 0, HB_IN_REAL = 1, HB_IN_REAL_CHIRP = 2 };
enum { HB_OUT_COMPLEX = 0, HB_OUT_ENVELOPE = 1, HB_OUT_MASK_CONJ = 2, HB_OUT_BLUESTEIN_MID = 3, HB_OUT_MUL_CONJ = 4,
       HB_OUT_HALF = 5 };       // bins 0 .. M / 2 of a real row's spectrum to io.half (mm_hilbert_rfft)
template <typename T>
struct HbIo {
  const T* x;               // HB_IN_REAL*: the clips [rows][x_stride], n valid samples each (zero beyond)
  int64_t x_stride;
  const hb_c<T>* w;         // chirp exp(-i pi k^2 / n), k < n
  const hb_c<T>* bhat;      // HB_OUT_MUL_CONJ: V -> conj(V bhat[m])
  T* env;                   // HB_OUT_ENVELOPE: |V[m]| * scale, m < n
  int64_t env_stride;
  int64_t n;
  T scale;
  int in_mode, out_mode;
  int64_t x_rows;           // real clips
  const T* down;            // not null: TWO clips per transformed row (2 r in the real part, 2 r + 1 in the imaginary
  const T* up;              //   part), each scaled by down[clip] = 2^-e on the way in and by up[clip] = 2^e on the way out
  T da, db, ua, ub;         // the workgroup's row: down / up of its two clips (hb_row_setup; the kernels' own copy)
  hb_c<T>* half;            // HB_OUT_HALF: [rows][half_stride] complex, bins m <= half_bins - 1 of every row
  int64_t half_stride, half_bins;
  // ragged kernels (RG) only -- a length, a chirp and a chirp spectrum per row (hb_row_setup<T, true>):
  const int64_t* lens;      //   [rows] valid samples of each clip, clamped into [1, n_max]; n, w, bhat and scale above are then
  int64_t n_max;            //   the workgroup's row's: w [rows][n_max], bhat [rows][M]
  const int* bad;           //   [rows] not 0: the clip holds a NaN or an infinity, its envelope is NaN
};

template <typename T, bool RG = false>
__device__ __forceinline__ void hb_row_setup(HbIo<T>& io, int64_t row, int64_t M) {
  if constexpr (RG) {
    // one clip per transformed row, each with its own length, chirp and chirp spectrum: uniform per workgroup, loaded once
    const int64_t len = io.lens[row];
    const int64_t n = len < 1 ? 1 : (len > io.n_max ? io.n_max : len);
    io.n = n;
    io.w += row * io.n_max;
    io.bhat += row * M;
    if (io.out_mode == HB_OUT_ENVELOPE) io.scale = io.bad[row] ? (T)NAN : (T)(1.0 / ((double)M * (double)n));
    return;
  }
  if (!io.down) return;
  io.da = io.down[2 * row]; io.ua = io.up[2 * row];
  const bool two = 2 * row + 1 < io.x_rows;
  io.db = two ? io.down[2 * row + 1] : (T)0;
  io.ub = two ? io.up[2 * row + 1] : (T)0;
}

// the pair of real samples (scaled) that transformed row `row` carries at index idx
template <typename T>
__device__ __forceinline__ hb_c<T> hb_pair(const HbIo<T>& io, int64_t row, int64_t idx) {
  hb_c<T> r;
  const int64_t ra = 2 * row, rb = 2 * row + 1 < io.x_rows ? 2 * row + 1 : ra;      // (no partner: db = 0)
  r.x = io.x[ra * io.x_stride + idx] * io.da;
  r.y = io.x[rb * io.x_stride + idx] * io.db;
  // (down = 0 marks a clip with non-finite samples, or the missing partner of an odd clip count: zeros, not NaN * 0)
  if (io.da == (T)0) r.x = (T)0;
  if (io.db == (T)0) r.y = (T)0;
  return r;
}

// scipy.signal.hilbert's spectrum weights: 1, 2 .. 2, (1 at n/2 for even n,) 0 .. 0
template <typename T>
__device__ __forceinline__ T hb_mask(int64_t k, int64_t n) {
  return (k == 0 || 2 * k == n) ? (T)1 : (k < (n + 1) / 2 ? (T)2 : (T)0);
}

template <typename T>
__device__ __forceinline__ hb_c<T> hb_load(const HbIo<T>& io, const hb_c<T>* __restrict__ src, int64_t row, int64_t idx) {
  if (io.in_mode == HB_IN_COMPLEX) return src[idx];
  hb_c<T> r;
  r.x = (T)0; r.y = (T)0;
  if (idx < io.n) {
    if (io.down) {
      r = hb_pair<T>(io, row, idx);
      if (io.in_mode == HB_IN_REAL_CHIRP) r = hb_mul(r, io.w[idx]);
    } else {
      const T v = io.x[row * io.x_stride + idx];
      if (io.in_mode == HB_IN_REAL_CHIRP) { r.x = v * io.w[idx].x; r.y = v * io.w[idx].y; } else r.x = v;
    }
  }
  return r;
}

template <typename T, bool RG = false>
__device__ __forceinline__ void hb_store(const HbIo<T>& io, hb_c<T>* __restrict__ dst, int64_t row, int64_t m, hb_c<T> V) {
  switch (io.out_mode) {
    case HB_OUT_COMPLEX: dst[m] = V; break;
    case HB_OUT_ENVELOPE:
      if (m < io.n && !io.down) {       // one clip per transform: |z| = |V| scale
        T mag;
        if constexpr (sizeof(T) == 4) mag = hypotf(V.x, V.y); else mag = hypot(V.x, V.y);
        io.env[row * io.env_stride + m] = mag * io.scale;
      } else if (m < io.n) {
        // V = conj(z) / scale (direct lengths) or z w[m] / scale (chirp transforms: the last chirp product is still due),
        // z = z_a + i z_b = (a - H b) + i (H a + b) on the scaled clips
        hb_c<T> z;
        if (io.w) { hb_c<T> wc = io.w[m]; wc.y = -wc.y; z = hb_mul(wc, V); } else { z.x = V.x; z.y = -V.y; }
        z.x *= io.scale; z.y *= io.scale;
        const hb_c<T> ab = hb_pair<T>(io, row, m);
        const T ha = z.y - ab.y, hb = ab.x - z.x;
        // (the scaled clips lie in [-1, 1]: a plain square root neither overflows nor underflows where it matters)
        io.env[2 * row * io.env_stride + m] = sqrt(ab.x * ab.x + ha * ha) * io.ua;
        if (2 * row + 1 < io.x_rows) io.env[(2 * row + 1) * io.env_stride + m] = sqrt(ab.y * ab.y + hb * hb) * io.ub;
      } else if constexpr (RG) {
        if (m < io.n_max) io.env[row * io.env_stride + m] = (T)0;       // behind the clip's end: +0.0
      }
      break;
    case HB_OUT_HALF:
      if (m < io.half_bins) io.half[row * io.half_stride + m] = V;
      break;
    case HB_OUT_MASK_CONJ: {            // direct lengths, between the two transforms: conj(X h)
      const T h = hb_mask<T>(m, io.n);
      V.x *= h; V.y *= -h;
      dst[m] = V;
      break;
    }
    case HB_OUT_BLUESTEIN_MID: {
      // V = FFT_M(conj(A Bhat)) -> X[k] = w[k] conj(V[k]) / M -> Y = X h[k] -> the input of the second chirp
      // transform, which evaluates DFT_n(conj(Y)): conj(Y[k]) w[k], zero beyond n
      hb_c<T> r;
      r.x = (T)0; r.y = (T)0;
      if (m < io.n) {
        const hb_c<T> w = io.w[m];
        const T h = hb_mask<T>(m, io.n) * io.scale;
        V.y = -V.y;
        hb_c<T> X = hb_mul(w, V);
        X.x *= h; X.y *= -h;
        r = hb_mul(X, w);
      }
      dst[m] = r;
      break;
    }
    default: {                          // HB_OUT_MUL_CONJ: the input of the forward transform that stands in for an inverse
      hb_c<T> r = hb_mul(V, io.bhat[m]);
      r.y = -r.y;
      dst[m] = r;
    }
  }
}

// w[t] = W_M^(e t), t = 1 .. N - 1, as short products of two exact table values (see hb_pass_kernel); w[0] unused.
template <typename T, int N>
__device__ __forceinline__ void hb_twiddle_powers(const hb_c<double>* __restrict__ lo, const hb_c<double>* __restrict__ hi,
                                                  int64_t e, hb_c<T> (&w)[N]) {
  constexpr int B = N <= 4 ? N : (N == 9 ? 3 : (N == 25 ? 5 : (N == 49 ? 7 : 4)));
  constexpr int NH = (N + B - 1) / B;
  hb_c<T> wl[B], wh[NH];
  {
    const hb_c<double> a = hb_twiddle(lo, hi, e);
    wl[1].x = (T)a.x; wl[1].y = (T)a.y;
  }
#pragma unroll
  for (int i = 2; i < B; ++i) wl[i] = (i & 1) ? hb_mul(wl[i - 1], wl[1]) : hb_mul(wl[i / 2], wl[i / 2]);
  if constexpr (NH > 1) {
    const hb_c<double> a = hb_twiddle(lo, hi, e * B);
    wh[1].x = (T)a.x; wh[1].y = (T)a.y;
#pragma unroll
    for (int i = 2; i < NH; ++i) wh[i] = (i & 1) ? hb_mul(wh[i - 1], wh[1]) : hb_mul(wh[i / 2], wh[i / 2]);
  }
#pragma unroll
  for (int t = 1; t < N; ++t) {
    const int th = t / B, tl = t % B;
    w[t] = th == 0 ? wl[tl] : (tl == 0 ? wh[th] : hb_mul(wh[th], wl[tl]));
  }
}

// Two Stockham passes of the same radix R fused into one launch: a radix-R^2 butterfly computed by R threads --
//   inputs   in[c + t nbC],  t = tB + R tA,  nbC = M / R^2,  c in [0, nbC),  k = c mod Ns
//   stage A  thread tB: v[tA] * W_(Ns R)^(k tA), DFT-R over tA -> a[u];  * W_(Ns R^2)^(k tB) * W_(R^2)^(tB u)
//   exchange through LDS (R x R per butterfly)
//   stage B  thread u: DFT-R over tB -> b[v];  out[(c - k) R^2 + k + (u + v R) Ns]
// -- i.e. the passes (R, Ns) and (R, Ns R) without the round trip through global memory between them.  A workgroup
// takes C consecutive c (thread = x C + c_local: unit-stride loads and stores of C points).
#ifndef MM_HB_C16
#define MM_HB_C16 32     // butterflies per workgroup of the fused radix-16 pair (float; double: half): the run length of its
#endif                   // strided loads / stores -- 32 complex = 256 B, 32 envelope floats = one 128-byte line
template <typename T, int R> struct HbFuse {
  static constexpr int C = (R == 16 ? MM_HB_C16 : 10) / (sizeof(T) == 8 ? 2 : 1);
  static constexpr int THREADS = C * R;
  static constexpr int PITCH = R * (R + 1) + 1;       // LDS points per butterfly: R columns of R + 1, one more between butterflies
};

// The shared pieces of the two fused kernels are MACROS, not functions, on purpose: an inlined function is optimised on its
// own first, and that changes which product of a complex multiplication the compiler contracts into an FMA (the last bit
// of the results) and the register allocation (docs/experiments.md, "Hilbert FFT: shared pieces").  The text below compiles
// exactly as if it stood in the kernel.  They use the kernels' own names: T, R, C, RC, PITCH, tile, cl, x, nbC, n_rows, live,
// lo, hi, io, dst, row, c.
//
// MM_HB_FUSED_ITEM: declares the thread's `row` and `c`; returns from the kernel in the workgroups that pad the grid
// (hb_fused_grid rounds up to 8).  XCD-aware block order: workgroups go round-robin to the 8 XCDs, and blocks with
// neighbouring c share cache lines (C = 10: 80-byte segments) -- so XCD x takes a contiguous eighth of the (row, c-block)
// list, and neighbours meet in one L2 instead of fetching the shared lines into two.
#define MM_HB_FUSED_ITEM                                                      \
  const int64_t nblk = (nbC + C - 1) / C;                                     \
  const int64_t per = (int64_t)gridDim.x / 8;                                 \
  const int64_t L = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;         \
  if (L >= nblk * n_rows) return;                                             \
  const int64_t row = L / nblk;                                               \
  const int64_t c = (L - row * nblk) * C + cl;

// MM_HB_TWIDDLE_DFT(V, TW, E), inside `if (live)`, all four pass kernels: V[t] *= W_M^(E t) if TW (the passes in front left
// Ns > 1; E is evaluated only then), then the DFT of V (output u at V[hb_perm<R>(u)]).
// W_(Ns R)^(k t) = W_M^(E t), t < R: two exact values from the float64 tables -- W^E and W^(B E) -- rounded to T, their
// first powers by squaring / one more product, and w[t] = (W^(B E))^(t / B) * (W^E)^(t % B): at most four roundings per
// twiddle, four table reads per butterfly instead of two per point.  (The whole chain in float64 cost the float32 passes
// 10 % of their time; one long float32 chain 4x the error.)  E t < M for t < R.
#define MM_HB_TWIDDLE_DFT(V, TW, E)                                           \
  if (TW) {                                                                   \
    hb_c<T> w[R];                                                             \
    hb_twiddle_powers<T, R>(lo, hi, (E), w);                                  \
    _Pragma("unroll") for (int t = 1; t < R; ++t) V[t] = hb_mul(V[t], w[t]);  \
  }                                                                           \
  hb_dft<T, R>(V);

// MM_HB_COLUMN_POWERS, inside `if (live)`: declares wu[u] = W_M^(tB nbC u) = W_(R^2)^(tB u), tB = x, for MM_HB_EXCHANGE.
// Computed by every butterfly: kept live across the two of hb_mid2_kernel the powers cost 2 R registers.
#define MM_HB_COLUMN_POWERS                                                   \
  hb_c<T> wu[R];                                                              \
  if (x > 0) hb_twiddle_powers<T, R>(lo, hi, (int64_t)x * nbC, wu);

// MM_HB_EXCHANGE(V, TW, E_OUT), behind the two above: stage A's outputs * W_(R^2)^(tB u), and if TW * W_M^(E_OUT) =
// W_(Ns R^2)^(k tB) (one table value), into the thread's row of the butterfly's LDS tile.
#define MM_HB_EXCHANGE(V, TW, E_OUT)                                          \
  hb_c<T> outer;                                                              \
  outer.x = (T)1; outer.y = (T)0;                                             \
  if ((TW) && x > 0) {                                                        \
    const hb_c<double> a = hb_twiddle(lo, hi, (E_OUT));                       \
    outer.x = (T)a.x; outer.y = (T)a.y;                                       \
  }                                                                           \
  hb_c<T>* wr = tile + cl * PITCH + x;                                        \
  _Pragma("unroll") for (int u = 0; u < R; ++u) {                             \
    hb_c<T> a = V[hb_perm<R>(u)];                                             \
    if (x > 0) {                                                              \
      if (u > 0) a = hb_mul(a, wu[u]);                                        \
      if (TW) a = hb_mul(a, outer);                                           \
    }                                                                         \
    wr[u * (R + 1)] = a;                                                      \
  }

// MM_HB_STAGE_B(B), inside `if (live)` behind the barrier: declares B, the thread's column of the exchange, and transforms it
// (output vv at B[hb_perm<R>(vv)]).
#define MM_HB_STAGE_B(B)                                                      \
  hb_c<T> B[R];                                                               \
  const hb_c<T>* rd = tile + cl * PITCH + x * (R + 1);                        \
  _Pragma("unroll") for (int tB = 0; tB < R; ++tB) B[tB] = rd[tB];            \
  hb_dft<T, R>(B);

// MM_HB_STORE_RUN2(RG, B): butterfly c fills out[c R^2 .. (c + 1) R^2), i.e. the workgroup one contiguous run (Ns = 1) -- B
// (natural order) back through LDS (slot x + vv R of butterfly cl), then unit-stride stores.  Two barriers, the first one for
// the threads that still read their column of the tile; every thread of the workgroup comes here.
#define MM_HB_STORE_RUN2(RG, B)                                               \
  __syncthreads();                                                            \
  if (live) {                                                                 \
    _Pragma("unroll") for (int vv = 0; vv < R; ++vv) tile[cl * PITCH + x + vv * R] = B[vv]; \
  }                                                                           \
  __syncthreads();                                                            \
  const int64_t c0 = c - cl;                                                  \
  const int n_live = (int)(nbC - c0 < C ? nbC - c0 : C);                      \
  for (int e = threadIdx.x; e < n_live * RC; e += C * R)                      \
    hb_store<T, RG>(io, dst, row, c0 * RC + e, tile[(e / RC) * PITCH + (e % RC)]);

template <typename T, int R, bool RG = false>
__global__ __launch_bounds__((HbFuse<T, R>::THREADS)) void hb_pass2_kernel(const hb_c<T>* __restrict__ in, hb_c<T>* __restrict__ out,
                                                                        int64_t M, int64_t Ns, int64_t n_rows,
                                                                        const hb_c<double>* __restrict__ lo,
                                                                        const hb_c<double>* __restrict__ hi, HbIo<T> io) {
  constexpr int C = HbFuse<T, R>::C, RC = R * R, PITCH = HbFuse<T, R>::PITCH;
  __shared__ hb_c<T> tile[C * PITCH];
  const int64_t nbC = M / RC;
  const int cl = threadIdx.x % C, x = threadIdx.x / C;          // x: tB in stage A, u in stage B
  MM_HB_FUSED_ITEM
  const hb_c<T>* src = in + row * M;
  hb_c<T>* dst = out + row * M;
  hb_row_setup<T, RG>(io, row, M);
  const bool live = c < nbC;
  const int64_t k = live ? (int64_t)((uint32_t)c % (uint32_t)Ns) : 0;
  if (live) {
    hb_c<T> v[R];
#pragma unroll
    for (int tA = 0; tA < R; ++tA) v[tA] = hb_load(io, src, row, c + (x + (int64_t)R * tA) * nbC);
    MM_HB_TWIDDLE_DFT(v, Ns > 1, k * (M / (Ns * R)))
    MM_HB_COLUMN_POWERS
    MM_HB_EXCHANGE(v, Ns > 1, k * x * (nbC / Ns))
  }
  __syncthreads();
  hb_c<T> b_keep[R];                      // natural order, for the first pass's staged stores
  if (live) {
    MM_HB_STAGE_B(b)
#pragma unroll
    for (int vv = 0; vv < R; ++vv) b_keep[vv] = b[hb_perm<R>(vv)];
    if (Ns > 1) {
      const int64_t m0 = (c - k) * RC + k + (int64_t)x * Ns;
#pragma unroll
      for (int vv = 0; vv < R; ++vv) hb_store<T, RG>(io, dst, row, m0 + (int64_t)vv * R * Ns, b[hb_perm<R>(vv)]);
    }
  }
  if (Ns == 1) {                          // the first pass
    MM_HB_STORE_RUN2(RG, b_keep)
  }
}

// The MIDDLE of an envelope of a directly transformed length, in one launch: the forward transform's LAST pass, the
// spectrum mask (+ conjugation: the inverse is a forward transform of the conjugate) and the inverse transform's FIRST pass.
// The forward transform is decimation in time as everywhere here; the inverse runs its passes in the OPPOSITE radix order,
// so its first pass has the forward's last radix and Ns = 1 -- and then both butterflies work on the same points:
//   forward last pass, radix R^2, Ns = nbC = M / R^2:   butterfly c writes   X[c + nbC t],  t = u + R v
//   inverse first pass, radix R^2, Ns = 1:              butterfly c reads  in[c + nbC t],   t = tB + R tA
// with the forward's output (u, v) exactly where the inverse's stage A wants its input (tB, tA): thread u holds v[tA].
// The masked spectrum never goes to memory: one read + one write of the rows instead of two of each (256 x 160 000
// float32 clips: 1.80 -> 1.47 GB per envelope, one launch less).  Fused radix-16 / radix-25 pairs (hb_pass2_kernel's
// butterfly, twice, with the LDS tile reused); io.in_mode / io.out_mode as in the single passes (a transform of ONE such
// pass loads the clips and stores the envelope here).
template <typename T, int R>
__global__ __launch_bounds__((HbFuse<T, R>::THREADS)) void hb_mid2_kernel(const hb_c<T>* __restrict__ in, hb_c<T>* __restrict__ out,
                                                                       int64_t M, int64_t n_rows,
                                                                       const hb_c<double>* __restrict__ lo,
                                                                       const hb_c<double>* __restrict__ hi, HbIo<T> io) {
  constexpr int C = HbFuse<T, R>::C, RC = R * R, PITCH = HbFuse<T, R>::PITCH;
  __shared__ hb_c<T> tile[C * PITCH];
  const int64_t nbC = M / RC;                                   // = Ns of the forward's last pass
  const int cl = threadIdx.x % C, x = threadIdx.x / C;
  MM_HB_FUSED_ITEM
  const hb_c<T>* src = in + row * M;
  hb_c<T>* dst = out + row * M;
  hb_row_setup<T>(io, row, M);
  const bool live = c < nbC;
  // ---- forward, last pass (Ns = nbC, so k = c): W_(Ns R)^(k tA) = W_M^(k R tA), W_(Ns R^2)^(k tB) = W_M^(k tB) ----
  if (live) {
    MM_HB_COLUMN_POWERS
    hb_c<T> v[R];
#pragma unroll
    for (int tA = 0; tA < R; ++tA) v[tA] = hb_load(io, src, row, c + (x + (int64_t)R * tA) * nbC);
    MM_HB_TWIDDLE_DFT(v, nbC > 1, c * R)
    MM_HB_EXCHANGE(v, nbC > 1, c * x)
  }
  __syncthreads();
  hb_c<T> v2[R];                                                // thread u: X[c + nbC (u + R v)], masked and conjugated
  if (live) {
    MM_HB_STAGE_B(b)
#pragma unroll
    for (int vv = 0; vv < R; ++vv) {
      hb_c<T> V = b[hb_perm<R>(vv)];
      const T hm = hb_mask<T>(c + nbC * (int64_t)(x + R * vv), io.n);
      V.x *= hm; V.y *= -hm;
      v2[vv] = V;
    }
  }
  __syncthreads();                                              // every thread has read its column of the tile
  // ---- inverse, first pass (Ns = 1: no twiddles in front, W_(R^2)^(tB u) behind stage A) ----
  if (live) {
    MM_HB_COLUMN_POWERS
    MM_HB_TWIDDLE_DFT(v2, false, 0)
    MM_HB_EXCHANGE(v2, false, 0)
  }
  __syncthreads();
  hb_c<T> b_keep[R];
  if (live) {
    MM_HB_STAGE_B(b)
#pragma unroll
    for (int vv = 0; vv < R; ++vv) b_keep[vv] = b[hb_perm<R>(vv)];
  }
  MM_HB_STORE_RUN2(false, b_keep)
}

// MM_HB_STORE_RUN(RG, V, NS): a single-radix kernel's staged store (radix <= 16) where the workgroup's 128 butterflies cover
// ONE contiguous run -- runs of NS consecutive butterflies fill one contiguous block of NS R outputs each (NS divides the
// workgroup; NS = 1: every butterfly its own R outputs).  Through LDS (slot p of the run at p + p / R: conflict-free for
// NS = 1 as for NS >= 16), then unit-stride stores.  One barrier; every thread of the workgroup comes here.  A macro for the
// reason given at MM_HB_FUSED_ITEM; uses the kernels' T, R, tile, live, nb, io, dst, row.
#define MM_HB_STORE_RUN(RG, V, NS)                                            \
  if (live) {                                                                 \
    const int jl = threadIdx.x, ns = (int)(NS);                               \
    const int p0 = (jl / ns) * ns * R + jl % ns;                              \
    _Pragma("unroll") for (int u = 0; u < R; ++u) {                           \
      const int pp = p0 + u * ns;                                             \
      tile[pp + pp / R] = V[hb_perm<R>(u)];                                   \
    }                                                                         \
  }                                                                           \
  __syncthreads();                                                            \
  const int64_t j0 = (int64_t)blockIdx.x * MM_HB_THREADS;                     \
  const int64_t cnt = (nb - j0 < MM_HB_THREADS ? nb - j0 : MM_HB_THREADS) * R; \
  for (int64_t e = threadIdx.x; e < cnt; e += MM_HB_THREADS)                  \
    hb_store<T, RG>(io, dst, row, j0 * R + e, tile[e + e / R]);

// The same for a single radix (one thread per butterfly: the forward's outputs ARE the inverse's inputs, in registers).
template <typename T, int R>
__global__ __launch_bounds__(MM_HB_THREADS) void hb_mid_kernel(const hb_c<T>* __restrict__ in, hb_c<T>* __restrict__ out,
                                                               int64_t M, const hb_c<double>* __restrict__ lo,
                                                               const hb_c<double>* __restrict__ hi, HbIo<T> io) {
  constexpr bool kTile = R <= 16;
  __shared__ hb_c<T> tile[kTile ? MM_HB_THREADS * (R + 1) : 1];
  const int64_t nb = M / R;                                 // butterflies per row = Ns of the forward's last pass
  const int64_t j = (int64_t)blockIdx.x * MM_HB_THREADS + threadIdx.x;
  const int64_t row = blockIdx.y;
  const hb_c<T>* src = in + row * M;
  hb_c<T>* dst = out + row * M;
  hb_row_setup<T>(io, row, M);
  const bool live = j < nb;
  hb_c<T> v[R], v2[R];
  if (live) {
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = hb_load(io, src, row, j + t * nb);
    MM_HB_TWIDDLE_DFT(v, nb > 1, j)                         // k = j, W_(Ns R)^(k t) = W_M^(j t)
#pragma unroll
    for (int u = 0; u < R; ++u) {                           // X[j + nb u] -> the inverse's input t = u
      hb_c<T> V = v[hb_perm<R>(u)];
      const T hm = hb_mask<T>(j + nb * (int64_t)u, io.n);
      V.x *= hm; V.y *= -hm;
      v2[u] = V;
    }
    hb_dft<T, R>(v2);
  }
  if (kTile) {
    MM_HB_STORE_RUN(false, v2, 1)
  } else if (live) {
#pragma unroll
    for (int u = 0; u < R; ++u) hb_store(io, dst, row, j * R + u, v2[hb_perm<R>(u)]);
  }
}

// One Stockham pass over rows of M complex points (see the header).  grid = (ceil(M / R / 128), rows).
template <typename T, int R, bool RG = false>
__global__ __launch_bounds__(MM_HB_THREADS) void hb_pass_kernel(const hb_c<T>* __restrict__ in, hb_c<T>* __restrict__ out,
                                                                int64_t M, int64_t Ns, const hb_c<double>* __restrict__ lo,
                                                                const hb_c<double>* __restrict__ hi, HbIo<T> io) {
  constexpr bool kTile = R <= 16;            // first pass through an LDS transpose (wider radices: strided stores)
  __shared__ hb_c<T> tile[kTile ? MM_HB_THREADS * (R + 1) : 1];
  const int64_t nb = M / R;                                 // butterflies per row
  const int64_t j = (int64_t)blockIdx.x * MM_HB_THREADS + threadIdx.x;
  const int64_t row = blockIdx.y;
  const hb_c<T>* src = in + row * M;
  hb_c<T>* dst = out + row * M;
  hb_row_setup<T, RG>(io, row, M);
  const bool live = j < nb;
  hb_c<T> v[R];
  if (live) {
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = hb_load(io, src, row, j + t * nb);
    MM_HB_TWIDDLE_DFT(v, Ns > 1, (int64_t)((uint32_t)j % (uint32_t)Ns) * (M / (Ns * R)))      // k = j mod Ns; M <= 2^25
  }
  if (kTile && Ns <= MM_HB_THREADS && MM_HB_THREADS % Ns == 0) {
    MM_HB_STORE_RUN(RG, v, Ns)
  } else if (live) {
    const int64_t k = (int64_t)((uint32_t)j % (uint32_t)Ns);
    const int64_t m0 = (j - k) * R + k;
#pragma unroll
    for (int u = 0; u < R; ++u) hb_store<T, RG>(io, dst, row, m0 + u * Ns, v[hb_perm<R>(u)]);
  }
}

// the textual pieces belong to the four kernels above and to nothing else
#undef MM_HB_FUSED_ITEM
#undef MM_HB_TWIDDLE_DFT
#undef MM_HB_COLUMN_POWERS
#undef MM_HB_EXCHANGE
#undef MM_HB_STAGE_B
#undef MM_HB_STORE_RUN2
#undef MM_HB_STORE_RUN

// W_M^e tables in float64: lo[e] = W_M^e (e < min(M, 1024)), hi[a] = W_M^(1024 a) (a < ceil(M / 1024))
__global__ __launch_bounds__(256) void hb_tables_kernel(hb_c<double>* __restrict__ lo, hb_c<double>* __restrict__ hi,
                                                        int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_lo = M < MM_HB_TWLO ? M : MM_HB_TWLO, n_hi = (M + MM_HB_TWLO - 1) / MM_HB_TWLO;
  if (i < n_lo) {
    double s, c;
    sincospi(-2.0 * (double)i / (double)M, &s, &c);
    lo[i].x = c; lo[i].y = s;
  }
  if (i < n_hi) {
    double s, c;
    sincospi(-2.0 * (double)(i * MM_HB_TWLO) / (double)M, &s, &c);
    hi[i].x = c; hi[i].y = s;
  }
}

// b[k] = exp(+i pi k^2 / n) for |k| < n (wrapped into [0, M)), 0 elsewhere: the chirp whose spectrum multiplies
// every Bluestein product.  k^2 is reduced mod 2n in integers, so the phase is exact to float64 rounding.
__device__ __forceinline__ hb_c<double> hb_chirp_phase(int64_t i, int64_t n, int64_t M) {
  const int64_t k = i < n ? i : (M - i < n ? M - i : -1);
  hb_c<double> r;
  r.x = 0.0; r.y = 0.0;
  if (k >= 0) {
    const unsigned long long q = ((unsigned long long)k * (unsigned long long)k) % (unsigned long long)(2 * n);
    sincospi((double)q / (double)n, &r.y, &r.x);
  }
  return r;
}

__global__ __launch_bounds__(256) void hb_chirp_kernel(hb_c<double>* __restrict__ b, int64_t n, int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  b[i] = hb_chirp_phase(i, n, M);
}

// The same chirp for every row of a ragged batch, each at its own length n = lens[row] (clamped into [1, n_max]), rounded
// once to the clips' precision: b [rows][M] (the wrapped chirp, whose spectrum one batched hb_fft then takes) and
// w [rows][n_max] = conj(b[k]), k < n.  On the way the clip is looked through once: a NaN or an infinity in [0, n) sets
// bad[row] (zeroed by the caller), and the envelope store then writes NaN for that row.  scipy returns NaN for the WHOLE of
// such a row; the transforms alone do not (an infinity leaves infinities behind: hypot(inf, NaN) = inf), hence the flag.
// grid = (ceil(M / 256), rows).
template <typename T>
__global__ __launch_bounds__(256) void hb_chirp_ragged_kernel(const T* __restrict__ x, int64_t x_stride,
                                                              const int64_t* __restrict__ lens, int64_t n_max, int64_t M,
                                                              hb_c<T>* __restrict__ w, hb_c<T>* __restrict__ b,
                                                              int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = blockIdx.y;
  if (i >= M) return;
  const int64_t len = lens[row];
  const int64_t n = len < 1 ? 1 : (len > n_max ? n_max : len);
  const hb_c<double> ph = hb_chirp_phase(i, n, M);
  hb_c<T> r;
  r.x = (T)ph.x; r.y = (T)ph.y;
  b[row * M + i] = r;
  if (i < n) {
    r.y = -r.y;
    w[row * n_max + i] = r;
    const T v = x[row * x_stride + i];
    if (!((v < (T)0 ? -v : v) < (T)INFINITY)) atomicOr(bad + row, 1);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void hb_convert_kernel(const hb_c<double>* __restrict__ in, hb_c<T>* __restrict__ out,
                                                         int64_t count, int conj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  out[i].x = (T)in[i].x;
  out[i].y = (T)(conj ? -in[i].y : in[i].y);
}

// n == 1: the envelope of a single sample is its magnitude
template <typename T>
__global__ __launch_bounds__(256) void hb_abs_kernel(const T* __restrict__ x, int64_t x_stride, int64_t rows,
                                                     T* __restrict__ env, int64_t env_stride) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < rows) env[r * env_stride] = x[r * x_stride] < (T)0 ? -x[r * x_stride] : x[r * x_stride];
}

// max |x| per clip in two steps: P workgroups per clip leave partial maxima (no atomics: a few hundred of them on one
// address serialise in L2, 110 us for 256 clips), hb_rowscale_kernel folds them.  grid = (P, clips).
template <typename T>
__global__ __launch_bounds__(256) void hb_rowmax_kernel(const T* __restrict__ x, int64_t x_stride, int64_t n, T* __restrict__ part) {
  __shared__ T wmax[4];
  const int64_t row = blockIdx.y;
  const T* xr = x + row * x_stride;
  T m = (T)0;
  for (int64_t i0 = (int64_t)blockIdx.x * 4096 + threadIdx.x; i0 < n; i0 += (int64_t)gridDim.x * 4096) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int64_t i = i0 + 256 * u;
      const T v = xr[i < n ? i : n - 1];
      const T a = v < (T)0 ? -v : v;
      m = (a > m || a != a) ? a : m;                        // a NaN sticks (and switches the scaling off)
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const T o = __shfl_xor(m, d);
    m = (o > m || o != o) ? o : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) { const T o = wmax[w]; m = (o > m || o != o) ? o : m; }
    part[row * gridDim.x + blockIdx.x] = m;
  }
}

// down[r] = 2^-e, up[r] = 2^e with max|x_r| = f 2^e, f in [0.5, 1) (exact scalings).  A clip of zeros comes out as zeros
// (up = 0: without that it would carry its partner's rounding noise); non-finite clips are not scaled.
template <typename T>
__global__ __launch_bounds__(256) void hb_rowscale_kernel(const T* __restrict__ part, int P, int64_t rows, T* __restrict__ down,
                                                          T* __restrict__ up) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  T m = (T)0;
  for (int i = 0; i < P; ++i) { const T o = part[r * P + i]; m = (o > m || o != o) ? o : m; }
  T d = (T)1, u = (T)1;
  if (m == (T)0) u = (T)0;
  else if (!(m < (T)INFINITY)) {
    // a clip with a NaN or an infinity: scipy.signal.hilbert returns NaN for the whole row -- and for that row ONLY.  It
    // is kept out of its pair (down = 0: hb_pair substitutes zeros) and its envelope comes out as NaN (up = NaN).
    d = (T)0; u = (T)NAN;
  } else if (m > (T)0) {
    int e;
    if constexpr (sizeof(T) == 4) { (void)frexpf(m, &e); e = e < -100 ? -100 : e; d = ldexpf(1.0f, -e); u = ldexpf(1.0f, e); }
    else { (void)frexp(m, &e); e = e < -900 ? -900 : e; d = ldexp(1.0, -e); u = ldexp(1.0, e); }
  }
  down[r] = d; up[r] = u;
}

// ---- host side ----
struct mm_hilbert {
  int64_t n, M;
  int dtype;                       // 0 float32, 1 float64
  bool bluestein;
  bool ragged;                     // mm_hilbert_ragged_create: n = the longest clip any call may bring, tables only (no w, bhat)
  int n_pass;
  int radix[32];
  int device;
  void* w;                         // [n] chirp exp(-i pi k^2 / n)       (Bluestein only)
  void* bhat;                      // [M] FFT_M of the wrapped conjugate chirp
  void* lo;                        // twiddle tables, float64 for both precisions
  void* hi;
};

// The one radix -> instantiation table: f(the kernel's radix as a std::integral_constant, whether it is a fused pair) for
// the pass radix R of a plan (256 / 625: two passes of radix 16 / 25 fused).  RG, a ragged batch: M is a power of two, so
// radix 256, 16, 8, 4 or 2 only -- no ragged kernel of another radix is instantiated.
template <bool RG, typename F>
static void hb_with_radix(int R, F&& f) {
#define MM_HB_CASE(RR, KR, FUSED) \
  case RR: f(std::integral_constant<int, KR>{}, std::integral_constant<bool, FUSED>{}); return;
  if constexpr (!RG) {
    switch (R) {
      MM_HB_CASE(625, 25, true)
      MM_HB_CASE(49, 49, false) MM_HB_CASE(25, 25, false) MM_HB_CASE(9, 9, false) MM_HB_CASE(7, 7, false)
      MM_HB_CASE(5, 5, false) MM_HB_CASE(3, 3, false)
    }
  }
  switch (R) {
    MM_HB_CASE(256, 16, true) MM_HB_CASE(16, 16, false) MM_HB_CASE(8, 8, false) MM_HB_CASE(4, 4, false)
    default: f(std::integral_constant<int, 2>{}, std::false_type{});
  }
#undef MM_HB_CASE
}

// the XCD-ordered grid of a fused kernel: C butterflies of R^2 points per workgroup, rounded up to the 8 XCDs (MM_HB_FUSED_ITEM)
template <typename T, int R>
static dim3 hb_fused_grid(int64_t M, int64_t rows) {
  constexpr int C = HbFuse<T, R>::C;
  const int64_t total = ((M / (R * R) + C - 1) / C) * rows;
  return dim3((unsigned)((total + 7) / 8 * 8));
}

static dim3 hb_single_grid(int64_t M, int R, int64_t rows) {
  return dim3((unsigned)((M / R + MM_HB_THREADS - 1) / MM_HB_THREADS), (unsigned)rows);
}

template <typename T, bool RG = false>
static void hb_launch_pass(int R, const hb_c<T>* in, hb_c<T>* out, int64_t M, int64_t Ns, int64_t rows,
                           const hb_c<double>* lo, const hb_c<double>* hi, const HbIo<T>& io, hipStream_t st) {
  hb_with_radix<RG>(R, [&](auto radix, auto fused) {
    constexpr int KR = decltype(radix)::value;
    if constexpr (decltype(fused)::value) {
      const dim3 grid = hb_fused_grid<T, KR>(M, rows), block(HbFuse<T, KR>::THREADS);
      hipLaunchKernelGGL((hb_pass2_kernel<T, KR, RG>), grid, block, 0, st, in, out, M, Ns, rows, lo, hi, io);
    } else {
      hipLaunchKernelGGL((hb_pass_kernel<T, KR, RG>), hb_single_grid(M, KR, rows), dim3(MM_HB_THREADS), 0, st, in, out, M, Ns, lo,
                         hi, io);
    }
  });
}

// the fused middle of a directly transformed envelope (hb_mid2_kernel / hb_mid_kernel) for the pass radix R
template <typename T>
static void hb_launch_mid(int R, const hb_c<T>* in, hb_c<T>* out, int64_t M, int64_t rows, const hb_c<double>* lo,
                          const hb_c<double>* hi, const HbIo<T>& io, hipStream_t st) {
  hb_with_radix<false>(R, [&](auto radix, auto fused) {
    constexpr int KR = decltype(radix)::value;
    if constexpr (decltype(fused)::value) {
      const dim3 grid = hb_fused_grid<T, KR>(M, rows), block(HbFuse<T, KR>::THREADS);
      hipLaunchKernelGGL((hb_mid2_kernel<T, KR>), grid, block, 0, st, in, out, M, rows, lo, hi, io);
    } else {
      hipLaunchKernelGGL((hb_mid_kernel<T, KR>), hb_single_grid(M, KR, rows), dim3(MM_HB_THREADS), 0, st, in, out, M, lo, hi, io);
    }
  });
}

// forward FFT of `rows` rows of M points: *cur holds the input and, on return, the output; *other is scratch.
// io.in_mode applies to the first pass, io.out_mode to the last one (n_pass >= 1).
// `reversed`: the passes in the opposite radix order (any order is a valid Stockham factorisation) -- what the last
// pass writes decides how well its pointwise step coalesces: the fused radix-16 pair stores runs of 16 points, the
// fused radix-25 pair runs of 10.
template <typename T, bool RG = false>
static void hb_fft(const mm_hilbert* h, hb_c<T>** cur, hb_c<T>** other, int64_t rows, const hb_c<double>* lo,
                   const hb_c<double>* hi, const HbIo<T>& io, hipStream_t st, bool reversed = false) {
  int64_t Ns = 1;
  for (int i = 0; i < h->n_pass; ++i) {
    HbIo<T> q = io;
    if (i > 0) q.in_mode = HB_IN_COMPLEX;
    if (i + 1 < h->n_pass) q.out_mode = HB_OUT_COMPLEX;
    const int R = h->radix[reversed ? h->n_pass - 1 - i : i];
    hb_launch_pass<T, RG>(R, *cur, *other, h->M, Ns, rows, lo, hi, q, st);
    Ns *= R;
    std::swap(*cur, *other);
  }
}

// The envelope through chirps, four transforms: chirp transform 1: (x w) -> FFT -> * Bhat -> inverse FFT (as a forward one
// of the conjugate) -> * w / M; mask; chirp transform 2 of conj(Y) the same way; magnitude.  io: the clips, the chirp, its
// spectrum, the envelope and n (RG: n_max, every row's own n, w, bhat and scale 1 / (M n_b) by hb_row_setup).
template <typename T, bool RG>
static void hb_chirp_envelope(const mm_hilbert* h, hb_c<T>** cur, hb_c<T>** other, int64_t rows, const hb_c<double>* lo,
                              const hb_c<double>* hi, HbIo<T> io, hipStream_t st) {
  io.in_mode = HB_IN_REAL_CHIRP; io.out_mode = HB_OUT_MUL_CONJ;
  hb_fft<T, RG>(h, cur, other, rows, lo, hi, io, st);
  io.in_mode = HB_IN_COMPLEX; io.out_mode = HB_OUT_BLUESTEIN_MID; io.scale = (T)(1.0 / (double)h->M);
  hb_fft<T, RG>(h, cur, other, rows, lo, hi, io, st);
  io.out_mode = HB_OUT_MUL_CONJ;
  hb_fft<T, RG>(h, cur, other, rows, lo, hi, io, st);
  // (RG: io.n is n_max and this scale a placeholder -- hb_row_setup<T, true> writes the row's 1 / (M n_b) over it)
  io.out_mode = HB_OUT_ENVELOPE; io.scale = (T)(1.0 / ((double)h->M * (double)io.n));
  hb_fft<T, RG>(h, cur, other, rows, lo, hi, io, st);
}

static void hb_free(mm_hilbert* h) {
  if (!h) return;
  if (h->w) (void)hipFree(h->w);
  if (h->bhat) (void)hipFree(h->bhat);
  if (h->lo) (void)hipFree(h->lo);
  if (h->hi) (void)hipFree(h->hi);
  delete h;
}

#define MM_HB_MAX_N ((int64_t)1 << 24)
#define MM_HB_MAXPART 4096        // partial maxima of hb_rowmax_kernel: about 2048 workgroups over all clips

// the passes of M = 2^cnt[0] 3^cnt[1] 5^cnt[2] 7^cnt[3]
static void hb_set_passes(mm_hilbert* h, int cnt[4]) {
  const int primes[4] = {2, 3, 5, 7};
  h->n_pass = 0;
  for (; cnt[0] >= 8; cnt[0] -= 8) h->radix[h->n_pass++] = 256;    // two radix-16 passes fused (hb_pass2_kernel)
  for (; cnt[0] >= 4; cnt[0] -= 4) h->radix[h->n_pass++] = 16;     // the widest power-of-two butterflies first
  if (cnt[0]) h->radix[h->n_pass++] = 1 << cnt[0];
  for (int i = 1; i < 4; ++i) {
    if (primes[i] == 5)
      for (; cnt[i] >= 4; cnt[i] -= 4) h->radix[h->n_pass++] = 625;  // two radix-25 passes fused
    for (; cnt[i] >= 2; cnt[i] -= 2) h->radix[h->n_pass++] = primes[i] * primes[i];
    if (cnt[i]) h->radix[h->n_pass++] = primes[i];
  }
}

// the twiddle tables of h->M on the current device: allocated, the kernel that fills them enqueued on `st`
static int hb_make_tables(mm_hilbert* h, hipStream_t st) {
  if (hipGetDevice(&h->device) != hipSuccess) return MM_ERR_HIP;
  const int64_t M = h->M;
  const int64_t n_lo = M < MM_HB_TWLO ? M : MM_HB_TWLO, n_hi = (M + MM_HB_TWLO - 1) / MM_HB_TWLO;
  if (hipMalloc(&h->lo, n_lo * sizeof(hb_c<double>)) != hipSuccess || hipMalloc(&h->hi, n_hi * sizeof(hb_c<double>)) != hipSuccess)
    return MM_ERR_ALLOC;
  const int64_t nt = n_lo > n_hi ? n_lo : n_hi;
  hipLaunchKernelGGL(hb_tables_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, (hb_c<double>*)h->lo,
                     (hb_c<double>*)h->hi, M);
  return MM_OK;
}

// the power-of-two transform length of a clip of n samples through chirps: M = 2^p >= max(16, 2 n - 1)
static int64_t hb_chirp_fft_size(int64_t n, int* log2_out) {
  int64_t M = 16;
  int p = 4;
  while (M < 2 * n - 1) { M *= 2; ++p; }
  if (log2_out) *log2_out = p;
  return M;
}

extern "C" {

int mm_hilbert_create(int64_t n, int32_t dtype, mm_hilbert** out) {
  if (!out || n < 1 || n > MM_HB_MAX_N || dtype < 0 || dtype > 1) return MM_ERR_INVALID_ARG;
  *out = nullptr;
  mm_hilbert* h = new (std::nothrow) mm_hilbert();
  if (!h) return MM_ERR_ALLOC;
  h->n = n; h->dtype = dtype; h->w = h->bhat = h->lo = h->hi = nullptr;
  // n = 2^a 3^b 5^c 7^d: transformed directly; anything else through chirps and M = 2^p >= 2n - 1
  int64_t rest = n;
  int cnt[4] = {0, 0, 0, 0};
  const int primes[4] = {2, 3, 5, 7};
  for (int i = 0; i < 4; ++i)
    while (rest % primes[i] == 0) { rest /= primes[i]; ++cnt[i]; }
  h->bluestein = rest != 1;
  int64_t M = n;
  if (h->bluestein) {
    cnt[1] = cnt[2] = cnt[3] = 0;
    M = hb_chirp_fft_size(n, &cnt[0]);
  }
  h->M = M;
  hb_set_passes(h, cnt);
  const size_t esz = dtype ? sizeof(hb_c<double>) : sizeof(hb_c<float>);
  hb_c<double>*b0 = nullptr, *b1 = nullptr;
  auto fail = [&](int rc) {
    if (b0) (void)hipFree(b0);
    if (b1) (void)hipFree(b1);
    hb_free(h);
    return rc;
  };
  hipStream_t st = nullptr;
  {
    const int rc = hb_make_tables(h, st);
    if (rc != MM_OK) return fail(rc);
  }
  hb_c<double>*lo_d = (hb_c<double>*)h->lo, *hi_d = (hb_c<double>*)h->hi;
  if (h->bluestein) {
    if (hipMalloc(&b0, M * sizeof(hb_c<double>)) != hipSuccess || hipMalloc(&b1, M * sizeof(hb_c<double>)) != hipSuccess ||
        hipMalloc(&h->w, n * esz) != hipSuccess || hipMalloc(&h->bhat, M * esz) != hipSuccess)
      return fail(MM_ERR_ALLOC);
    const dim3 gm((unsigned)((M + 255) / 256)), gn((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(hb_chirp_kernel, gm, dim3(256), 0, st, b0, n, M);
    // w[k] = conj(b[k]), k < n
    if (dtype) hipLaunchKernelGGL(hb_convert_kernel<double>, gn, dim3(256), 0, st, b0, (hb_c<double>*)h->w, n, 1);
    else hipLaunchKernelGGL(hb_convert_kernel<float>, gn, dim3(256), 0, st, b0, (hb_c<float>*)h->w, n, 1);
    hb_c<double>*cur = b0, *other = b1;
    HbIo<double> plain = {};
    hb_fft<double>(h, &cur, &other, 1, lo_d, hi_d, plain, st);
    if (dtype) hipLaunchKernelGGL(hb_convert_kernel<double>, gm, dim3(256), 0, st, cur, (hb_c<double>*)h->bhat, M, 0);
    else hipLaunchKernelGGL(hb_convert_kernel<float>, gm, dim3(256), 0, st, cur, (hb_c<float>*)h->bhat, M, 0);
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(MM_ERR_HIP);
  if (b0) (void)hipFree(b0);
  if (b1) (void)hipFree(b1);
  *out = h;
  return MM_OK;
}

// The handle of the ragged envelope: the transform length M of clips of up to n_max samples and its twiddle tables,
// nothing that belongs to one length (every call brings its rows' chirps, mm_hilbert_envelope_ragged).
int mm_hilbert_ragged_create(int64_t n_max, int32_t dtype, mm_hilbert** out) {
  if (!out || n_max < 1 || n_max > MM_HB_MAX_N || dtype < 0 || dtype > 1) return MM_ERR_INVALID_ARG;
  *out = nullptr;
  mm_hilbert* h = new (std::nothrow) mm_hilbert();
  if (!h) return MM_ERR_ALLOC;
  h->dtype = dtype; h->bluestein = true; h->ragged = true;
  int cnt[4] = {0, 0, 0, 0};
  h->M = hb_chirp_fft_size(n_max, &cnt[0]);
  h->n = h->M / 2;                   // every clip this M takes: 2 n - 1 <= M
  hb_set_passes(h, cnt);
  hipStream_t st = nullptr;
  int rc = hb_make_tables(h, st);
  if (rc == MM_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) rc = MM_ERR_HIP;
  if (rc != MM_OK) { hb_free(h); return rc; }
  *out = h;
  return MM_OK;
}

void mm_hilbert_destroy(mm_hilbert* h) { hb_free(h); }

int64_t mm_hilbert_fft_size(const mm_hilbert* h) { return h ? h->M : MM_ERR_INVALID_ARG; }

size_t mm_hilbert_workspace_bytes(const mm_hilbert* h, int64_t rows) {
  if (!h || rows < 1 || h->ragged) return 0;
  // two [pairs of clips][fft_size] complex buffers + the clips' maxima and scale factors
  const size_t pairs = (size_t)((rows + 1) / 2);
  return (size_t)2 * pairs * (size_t)h->M * (h->dtype ? sizeof(hb_c<double>) : sizeof(hb_c<float>)) + ((size_t)rows * 3 + MM_HB_MAXPART) * 8 + 256;
}

}  // extern "C"

template <typename T>
static int hb_envelope(const mm_hilbert* h, const T* d_x, int64_t rows, int64_t x_stride, T* d_env, int64_t env_stride,
                       void* d_ws, hipStream_t st) {
  const int64_t n = h->n, M = h->M;
  const int64_t x_rows = rows;
  const bool paired = x_rows > 1 && h->n_pass > 0;          // (one recording: nothing to pair it with)
  if (paired) rows = (x_rows + 1) / 2;                      // transformed rows: two clips each
  hb_c<T>* cur = (hb_c<T>*)d_ws;
  hb_c<T>* other = cur + rows * M;
  T* rowmax = (T*)(other + rows * M);
  const hb_c<double>*lo = (const hb_c<double>*)h->lo, *hi = (const hb_c<double>*)h->hi;
  HbIo<T> io = {};
  io.x = d_x; io.x_stride = x_stride; io.w = (const hb_c<T>*)h->w; io.bhat = (const hb_c<T>*)h->bhat;
  io.env = d_env; io.env_stride = env_stride; io.n = n; io.x_rows = x_rows;
  if (paired) {
    T* part = rowmax + 2 * x_rows;                          // [x_rows][P]
    int64_t P = std::max<int64_t>(1, std::min<int64_t>((n + 4095) / 4096, 2048 / x_rows));
    if (P * x_rows > MM_HB_MAXPART) P = std::max<int64_t>(1, MM_HB_MAXPART / x_rows);
    hipLaunchKernelGGL(hb_rowmax_kernel<T>, dim3((unsigned)P, (unsigned)x_rows), dim3(256), 0, st, d_x, x_stride, n, part);
    hipLaunchKernelGGL(hb_rowscale_kernel<T>, dim3((unsigned)((x_rows + 255) / 256)), dim3(256), 0, st, part, (int)P, x_rows,
                       rowmax, rowmax + x_rows);
    io.down = rowmax; io.up = rowmax + x_rows;
  }
  if (h->n_pass == 0) {          // n == 1: the envelope of one sample is its magnitude
    hipLaunchKernelGGL(hb_abs_kernel<T>, dim3((unsigned)((x_rows + 255) / 256)), dim3(256), 0, st, d_x, x_stride, x_rows, d_env,
                       env_stride);
  } else if (h->bluestein) {
    hb_chirp_envelope<T, false>(h, &cur, &other, rows, lo, hi, io, st);
  } else {
    // forward passes 0 .. P-2 | the fused middle: forward pass P-1, mask, inverse pass P-1 (hb_mid*_kernel) | inverse passes
    // P-2 .. 0 (the inverse in the opposite radix order: any order is a valid Stockham factorisation); the clips ride in
    // on the first launch, the envelope (two float rows read, two written per point) out on the last
    const int P = h->n_pass;
    int64_t Ns = 1;
    for (int i = 0; i + 1 < P; ++i) {
      HbIo<T> q = io;
      q.in_mode = i == 0 ? HB_IN_REAL : HB_IN_COMPLEX; q.out_mode = HB_OUT_COMPLEX;
      hb_launch_pass<T>(h->radix[i], cur, other, M, Ns, rows, lo, hi, q, st);
      Ns *= h->radix[i];
      std::swap(cur, other);
    }
    {
      HbIo<T> q = io;
      q.in_mode = P == 1 ? HB_IN_REAL : HB_IN_COMPLEX;
      q.out_mode = P == 1 ? HB_OUT_ENVELOPE : HB_OUT_COMPLEX; q.scale = (T)(1.0 / (double)n);
      hb_launch_mid<T>(h->radix[P - 1], cur, other, M, rows, lo, hi, q, st);
      std::swap(cur, other);
    }
    Ns = h->radix[P - 1];
    for (int i = P - 2; i >= 0; --i) {
      HbIo<T> q = io;
      q.in_mode = HB_IN_COMPLEX; q.out_mode = i == 0 ? HB_OUT_ENVELOPE : HB_OUT_COMPLEX; q.scale = (T)(1.0 / (double)n);
      hb_launch_pass<T>(h->radix[i], cur, other, M, Ns, rows, lo, hi, q, st);
      Ns *= h->radix[i];
      std::swap(cur, other);
    }
  }
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

extern "C" int mm_hilbert_envelope(mm_hilbert* h, const void* d_x, int64_t rows, int64_t x_stride, void* d_env,
                                   int64_t env_stride, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_x || !d_env || !d_ws || rows < 1 || rows > 65535 || h->ragged || x_stride < h->n || env_stride < h->n)
    return MM_ERR_INVALID_ARG;
  if (ws_bytes < mm_hilbert_workspace_bytes(h, rows)) return MM_ERR_WORKSPACE;
  if ((h->M + 255) / 256 > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  return h->dtype ? hb_envelope<double>(h, (const double*)d_x, rows, x_stride, (double*)d_env, env_stride, d_ws, st)
                  : hb_envelope<float>(h, (const float*)d_x, rows, x_stride, (float*)d_env, env_stride, d_ws, st);
}

// ---- a ragged batch: a length per clip ----
// Workspace: bad [rows] int | w [rows][n_max] | three [rows][M] complex buffers (the chirps' spectra and the two the passes
// alternate between), each part on a 256-byte boundary.
static size_t hb_ragged_align(size_t b) { return (b + 255) / 256 * 256; }

extern "C" size_t mm_hilbert_ragged_workspace_bytes(const mm_hilbert* h, int64_t rows, int64_t n_max) {
  if (!h || !h->ragged || rows < 1 || n_max < 1 || n_max > h->n) return 0;
  const size_t esz = h->dtype ? sizeof(hb_c<double>) : sizeof(hb_c<float>);
  return hb_ragged_align((size_t)rows * sizeof(int)) + hb_ragged_align((size_t)rows * (size_t)n_max * esz) +
         (size_t)3 * hb_ragged_align((size_t)rows * (size_t)h->M * esz);
}

template <typename T>
static int hb_envelope_ragged(const mm_hilbert* h, const T* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                              const int64_t* d_lens, T* d_env, int64_t env_stride, void* d_ws, hipStream_t st) {
  const int64_t M = h->M;
  char* p = (char*)d_ws;
  int* bad = (int*)p;
  p += hb_ragged_align((size_t)rows * sizeof(int));
  hb_c<T>* w = (hb_c<T>*)p;
  p += hb_ragged_align((size_t)rows * (size_t)n_max * sizeof(hb_c<T>));
  const size_t buf = hb_ragged_align((size_t)rows * (size_t)M * sizeof(hb_c<T>));
  hb_c<T>* bhat = (hb_c<T>*)p;
  hb_c<T>* spare = (hb_c<T>*)(p + buf);
  hb_c<T>* third = (hb_c<T>*)(p + 2 * buf);
  const hb_c<double>*lo = (const hb_c<double>*)h->lo, *hi = (const hb_c<double>*)h->hi;
  fill_words(bad, 0u, rows, st);
  // every row's chirp at its own length, and the chirps' spectra: one batched transform in the clips' precision
  hipLaunchKernelGGL(hb_chirp_ragged_kernel<T>, dim3((unsigned)((M + 255) / 256), (unsigned)rows), dim3(256), 0, st, d_x, x_stride,
                     d_lens, n_max, M, w, bhat, bad);
  HbIo<T> plain = {};
  hb_fft<T>(h, &bhat, &spare, rows, lo, hi, plain, st);
  // the four transforms of hb_envelope's chirp branch, one clip per row, n / w / bhat / scale the row's own
  hb_c<T>*cur = spare, *other = third;
  HbIo<T> io = {};
  io.x = d_x; io.x_stride = x_stride; io.w = w; io.bhat = bhat; io.env = d_env; io.env_stride = env_stride;
  io.n = n_max; io.n_max = n_max; io.x_rows = rows; io.lens = d_lens; io.bad = bad;
  hb_chirp_envelope<T, true>(h, &cur, &other, rows, lo, hi, io, st);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

extern "C" int mm_hilbert_envelope_ragged(mm_hilbert* h, const void* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                                          const int64_t* d_lens, void* d_env, int64_t env_stride, void* d_ws, size_t ws_bytes,
                                          void* stream) {
  if (rows < 1 || rows > 65535 || !h || !d_x || !d_lens || !d_env || !d_ws) return MM_ERR_INVALID_ARG;
  if (!h->ragged || n_max < 1 || n_max > h->n || x_stride < n_max || env_stride < n_max) return MM_ERR_INVALID_ARG;
  if (ws_bytes < mm_hilbert_ragged_workspace_bytes(h, rows, n_max)) return MM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  return h->dtype ? hb_envelope_ragged<double>(h, (const double*)d_x, rows, n_max, x_stride, d_lens, (double*)d_env, env_stride,
                                               d_ws, st)
                  : hb_envelope_ragged<float>(h, (const float*)d_x, rows, n_max, x_stride, d_lens, (float*)d_env, env_stride,
                                              d_ws, st);
}

// rFFT of real float32 rows, zero-padded to the plan's length: the forward transform alone (the rows ride in on the first
// pass, bins 0 .. n / 2 out on the last) -- the trajectory rFFT (row A8) of clips with more than 8192 frames, e.g. one
// recording at the reference's default 1 ms step (script/mfcc.py:296: 10 001 frames per ten seconds).
extern "C" size_t mm_hilbert_rfft_workspace_bytes(const mm_hilbert* h, int64_t rows) {
  if (!h || rows < 1) return 0;
  return (size_t)2 * (size_t)rows * (size_t)h->M * sizeof(hb_c<float>) + 256;
}

extern "C" int mm_hilbert_rfft_f32(mm_hilbert* h, const float* d_x, int64_t rows, int64_t x_stride, int64_t n_valid,
                                   float* d_out, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_x || !d_out || !d_ws || rows < 1 || rows > 65535 || n_valid < 1 || n_valid > h->n || x_stride < n_valid)
    return MM_ERR_INVALID_ARG;
  if (h->dtype != 0 || h->bluestein || h->n_pass < 1 || (h->M & 1)) return MM_ERR_UNSUPPORTED;     // float32, a direct even length
  if (ws_bytes < mm_hilbert_rfft_workspace_bytes(h, rows)) return MM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hb_c<float>* cur = (hb_c<float>*)d_ws;
  hb_c<float>* other = cur + rows * h->M;
  HbIo<float> io = {};
  io.x = d_x; io.x_stride = x_stride; io.n = n_valid; io.x_rows = rows;
  io.in_mode = HB_IN_REAL; io.out_mode = HB_OUT_HALF;
  io.half = (hb_c<float>*)d_out; io.half_bins = h->M / 2 + 1; io.half_stride = io.half_bins;
  hb_fft<float>(h, &cur, &other, rows, (const hb_c<double>*)h->lo, (const hb_c<double>*)h->hi, io, st);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

