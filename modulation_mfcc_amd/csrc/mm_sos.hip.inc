#pragma once
// What every device form of scipy.signal.sosfiltfilt in mm_tail.hip shares (the time-major kernels of mm_sos_tm.hip.inc,
// the segmented rows of mm_sos_rows.hip.inc, the clip-resident change tail of mm_change_clip.hip.inc): the filter as the
// host holds it and as a kernel takes it, one step of the cascade, scipy's odd extension, and for the time-parallel
// forms the tables, the scan over lanes and the table upload.
//
// sosfiltfilt = scipy.signal.sosfiltfilt defaults: odd extension by padlen = 3*ntaps samples,
// steady-state initial conditions sosfilt_zi(sos) scaled by the first sample of each pass, forward
// pass, reversed pass, strip the padding.
#include <cfloat>
#include <type_traits>
#define MM_MAX_SEC 16
#define MM_SCAN_MAX_SEC 4         // most sections of any time-parallel form (the scans below); more: the time-major kernels
#define MM_CONST __attribute__((address_space(4)))
#define MM_TAB_PIECE 480          // doubles per upload launch (3.8 KB of kernel argument: under the 4 KB a launch may carry)

struct SosFilt {
  double c[MM_MAX_SEC][6];   // b0 b1 b2 a0 a1 a2 (a0 = 1); sections beyond n_sec are the identity
  double zi[MM_MAX_SEC][2];  // sosfilt_zi
  int n_sec, padlen;
};

template <int NS>
struct SosCoef {
  double c[NS][5];     // b0 b1 b2 a1 a2
  double zi[NS][2];
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

// Row r of float32 MFCCs [clips][n_mfcc][T] as the change tail filters them: clip r / n_rows, coefficient first_row + r % n_rows
__device__ __forceinline__ const float* mfcc_row(const float* mfcc, int n_mfcc, int first_row, int n_rows, int64_t T, int64_t r) {
  const int64_t b = r / n_rows, c = r - b * n_rows;
  return mfcc + (b * n_mfcc + first_row + c) * T;
}

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

// v of the lane whose byte address (4 * lane) is given; a negative address wraps inside the wave
__device__ __forceinline__ double lane_from(int byte_addr, double v) {
  const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(v));
  return __hiloint2double(hi, lo);
}

// Phi and its powers are block lower triangular (a section's state never reaches the sections before it): column b
// holds rows 2 * (b / 2) .. 2 NS - 1 only, TRI = 2 NS (NS + 1) numbers instead of 4 NS^2, stored by columns.
// Where column b starts in the packed matrix = the numbers of the columns before b
constexpr int sos_tri_col(int NS, int b) { return (b >> 1) * 2 * (2 * NS - (b >> 1) + 1) + (b & 1) * (2 * NS - (b & ~1)); }

// Inclusive scan over sequences of 2^J consecutive lanes of one wave: Z(k) <- sum_{i <= k} M^(k - i) Z(i), M^(2^j) = P[j0 + j], j < J,
// a Hillis-Steele scan whose step j adds M^(2^j) times the value 2^j places back.  lane: the thread's lane in its wave,
// k: its place in its sequence.  Raw ds_bpermute (byte address of the source lane): lanes without a source d lanes back
// inside their sequence read some other lane and ignore it.  JC: J where it is a constant (0: only known when the kernel
// runs) -- the compiler needs the bound inside this function to know 2^j small and fold `k >= d` into the subtraction
template <int NS, int JC = 0>
__device__ __forceinline__ void sos_lane_scan(double (&Z)[2 * NS], const MM_CONST double* P, int j0, int J, int lane, int k) {
  constexpr int S2 = 2 * NS, TRI = 2 * NS * (NS + 1);
#pragma unroll 1
  for (int j = 0; j < (JC ? JC : J); ++j) {
    const int d = 1 << j;
    double pr[S2], Pm[TRI];
    const MM_CONST double* Pj = P + (j0 + j) * TRI;
#pragma unroll
    for (int e = 0; e < TRI; ++e) Pm[e] = Pj[e];             // the whole matrix in one round trip of the scalar cache
    const int src = (lane - d) << 2;
#pragma unroll
    for (int b = 0; b < S2; ++b) pr[b] = lane_from(src, Z[b]);
    if (k >= d) {
#pragma unroll
      for (int b = 0; b < S2; ++b) {               // column by column: independent accumulators
        const int base = sos_tri_col(NS, b);
#pragma unroll
        for (int a = (b & ~1); a < S2; ++a) Z[a] = fma(Pm[base + a - (b & ~1)], pr[b], Z[a]);
      }
    }
  }
}

struct TabPiece { int n, off; double v[MM_TAB_PIECE]; };
__global__ __launch_bounds__(MM_TAB_PIECE) void sos_tab_upload_kernel(double* dst, TabPiece c) {
  if ((int)threadIdx.x < c.n) dst[c.off + threadIdx.x] = c.v[threadIdx.x];
}

// ---- host side ----
// a host table into device memory by kernel-argument copies: asynchronous, stateless, graph-capture safe like every compute call
static void sos_tab_upload(const std::vector<double>& tab, double* d_tab, hipStream_t st) {
  for (size_t off = 0; off < tab.size(); off += MM_TAB_PIECE) {
    TabPiece c;
    c.n = (int)std::min<size_t>(MM_TAB_PIECE, tab.size() - off);
    c.off = (int)off;
    memcpy(c.v, tab.data() + off, sizeof(double) * (size_t)c.n);
    hipLaunchKernelGGL(sos_tab_upload_kernel, dim3(1), dim3(MM_TAB_PIECE), 0, st, d_tab, c);
  }
}

// scipy.signal.sosfilt_zi + the padlen rule of sosfiltfilt, host side
static int make_sosfilt(const double* sos, int n_sec, SosFilt* f) {
  if (n_sec < 0 || n_sec > MM_MAX_SEC || (n_sec > 0 && !sos)) return MM_ERR_INVALID_ARG;
  f->n_sec = n_sec;
  f->padlen = 0;
  if (n_sec == 0) return MM_OK;
  double scale = 1.0;
  int zb = 0, za = 0;
  for (int s = 0; s < n_sec; ++s) {
    const double* r = sos + 6 * s;
    if (r[3] == 0.0) return MM_ERR_INVALID_ARG;
    double b0 = r[0] / r[3], b1 = r[1] / r[3], b2 = r[2] / r[3], a1 = r[4] / r[3], a2 = r[5] / r[3];
    f->c[s][0] = b0; f->c[s][1] = b1; f->c[s][2] = b2; f->c[s][3] = 1.0; f->c[s][4] = a1; f->c[s][5] = a2;
    // lfilter_zi: (I - companion(a)^T) zi = b[1:] - a[1:] b0
    const double B0 = b1 - a1 * b0, B1 = b2 - a2 * b0;
    const double den = 1.0 + a1 + a2;
    const double z0 = (B0 + B1) / den;
    f->zi[s][0] = scale * z0;
    f->zi[s][1] = scale * (B1 - a2 * z0);
    scale *= (b0 + b1 + b2) / (1.0 + a1 + a2);
    if (r[2] == 0.0) ++zb;
    if (r[5] == 0.0) ++za;
  }
  const int ntaps = 2 * n_sec + 1 - (zb < za ? zb : za);
  f->padlen = 3 * ntaps;
  return MM_OK;
}

// the filter as a kernel of NS sections takes it: identity sections pad up to an instantiated size
template <int NS>
static void sos_coef_of(const SosFilt& f, SosCoef<NS>* c) {
  for (int s = 0; s < NS; ++s) {
    if (s < f.n_sec) {
      c->c[s][0] = f.c[s][0]; c->c[s][1] = f.c[s][1]; c->c[s][2] = f.c[s][2]; c->c[s][3] = f.c[s][4]; c->c[s][4] = f.c[s][5];
      c->zi[s][0] = f.zi[s][0]; c->zi[s][1] = f.zi[s][1];
    } else {   // identity section: y = 1*x + 0 exactly, state stays 0
      c->c[s][0] = 1.0; c->c[s][1] = c->c[s][2] = c->c[s][3] = c->c[s][4] = 0.0;
      c->zi[s][0] = c->zi[s][1] = 0.0;
    }
  }
}

// f(std::integral_constant<int, NS>) for the instantiation of the time-parallel forms that takes n_sec sections: 2, 3 or 4
template <class F>
static int with_scan_sections(int n_sec, F f) {
  static_assert(MM_SCAN_MAX_SEC == 4, "one instantiation per section count up to MM_SCAN_MAX_SEC");
  return n_sec <= 2 ? f(std::integral_constant<int, 2>()) : n_sec == 3 ? f(std::integral_constant<int, 3>())
                                                                      : f(std::integral_constant<int, 4>());
}

// The two tables the scans of mm_change_clip.hip.inc and of mm_sos_rows.hip.inc close the recursion with, for chunks of `chunk` samples:
//   W[chunk - 1 - m] = the state m zero-input steps after a unit sample                       [chunk][2 NS]
//   P[j] = Phi^(2^j), j < J; Phi = the transition of one chunk with zero input, stored by columns, rows 2 * (b / 2) .. only
// Built in the host's extended precision (x87 long double, 64-bit mantissa) and rounded ONCE when stored.  The powers
// come from repeated squaring, and with the poles within 1e-3 of the unit circle the entries of Phi^k are large against
// what they add up to: squared in double, a 12 Hz low-pass at 48 kHz (wn = 5e-4) came out 2e-8 of its maximum away from
// the exact result, a thousand times scipy's own rounding; with exact-to-the-last-bit tables what is left is the
// device's double arithmetic, which is scipy's (docs/experiments.md, "The IIR filter near the unit circle").
#if !defined(__HIP_DEVICE_COMPILE__)
static_assert(LDBL_MANT_DIG >= 64, "the scan tables need an extended-precision long double on the host");
#endif
template <int NS>
static void sos_scan_tables(const SosCoef<NS>& f, int chunk, int J, double* W, double* P) {
  typedef long double xreal;
  constexpr int S2 = 2 * NS;
  xreal c[NS][5];
  for (int s = 0; s < NS; ++s) for (int k = 0; k < 5; ++k) c[s][k] = (xreal)f.c[s][k];
  // one step of the cascade (direct form II transposed) on input x
  auto step = [&](xreal x, xreal (&z0)[NS], xreal (&z1)[NS]) {
    for (int s = 0; s < NS; ++s) {
      const xreal y = c[s][0] * x + z0[s];
      z0[s] = c[s][1] * x - c[s][3] * y + z1[s];
      z1[s] = c[s][2] * x - c[s][4] * y;
      x = y;
    }
  };
  {
    xreal z0[NS], z1[NS];
    for (int s = 0; s < NS; ++s) { z0[s] = 0; z1[s] = 0; }
    for (int m = 0; m < chunk; ++m) {
      step(m == 0 ? (xreal)1 : (xreal)0, z0, z1);
      double* Wm = W + (size_t)(chunk - 1 - m) * S2;
      for (int s = 0; s < NS; ++s) { Wm[2 * s] = (double)z0[s]; Wm[2 * s + 1] = (double)z1[s]; }
    }
  }
  xreal A[S2][S2], B[S2][S2];
  for (int b = 0; b < S2; ++b) {
    xreal z0[NS], z1[NS];
    for (int s = 0; s < NS; ++s) { z0[s] = 0; z1[s] = 0; }
    (b & 1 ? z1 : z0)[b >> 1] = 1;
    for (int i = 0; i < chunk; ++i) step(0, z0, z1);
    for (int s = 0; s < NS; ++s) { A[2 * s][b] = z0[s]; A[2 * s + 1][b] = z1[s]; }
  }
  constexpr int TRI = 2 * NS * (NS + 1);
  for (int j = 0; j < J; ++j) {
    double* Pj = P + (size_t)j * TRI;
    int e = 0;
    for (int b = 0; b < S2; ++b) for (int a = (b & ~1); a < S2; ++a) Pj[e++] = (double)A[a][b];
    for (int a = 0; a < S2; ++a) for (int b = 0; b < S2; ++b) {
      xreal acc = 0;
      for (int k = 0; k < S2; ++k) acc += A[a][k] * A[k][b];
      B[a][b] = acc;
    }
    for (int a = 0; a < S2; ++a) for (int b = 0; b < S2; ++b) A[a][b] = B[a][b];
  }
}
