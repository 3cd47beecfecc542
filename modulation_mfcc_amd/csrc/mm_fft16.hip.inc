#pragma once
// Register radix-16 FFT core for gfx950 and the kernels built on it.  Included by mm_api.hip and mm_logmel16s.hip.
//
// A real row of n = 512*R samples (R = 1, 2) is packed into nc = 256*R complex points
// z[m] = x[2m] + i x[2m+1] and transformed by 16*R lanes that hold 16 complex values each:
//
//   stage 1   lane q holds z[16R*n1 + q], n1 = 0..15  -> DFT-16 in registers -> * W_nc^(q*k1)
//   exchange  16x16R transpose through a wave-private, padded LDS buffer (ds_write_b64 /
//             ds_read_b64, conflict-free; LDS ops of one wave execute in order: no barrier)
//   stage 2   R = 1: DFT-16 over n2 in registers                -> Z[k1 + 16*k2]
//             R = 2: lane (k1, p) does the DFT-16 of the n2 = 2m+p half, * W_32^(p*j), then one
//                    radix-2 butterfly with lane^1 through DPP quad_perm       -> Z[k1 + 16*(j+16p)]
//   split     real-FFT split X[k], X[nc-k] from Z[k] and conj Z[nc-k]; the partner value lives
//             in lane (16-k1)%16 (and p^1), register 15-j: R = 1 two DPP moves per float (row_mirror,
//             row_ror:1 -- the VALU, not the LDS pipe), R = 2 one ds_bpermute per float
//
// One wave processes 4/R rows at a time.  All register arrays are indexed by compile-time
// constants only (full unrolling), so everything stays in VGPRs.

namespace f16 {

__device__ __forceinline__ constexpr int P16(int k) { return 4 * (k & 3) + (k >> 2); }

__device__ __forceinline__ float2 cmulf(float2 a, float2 w) {
  return make_float2(fmaf(-a.y, w.y, a.x * w.x), fmaf(a.y, w.x, a.x * w.y));
}

__device__ __forceinline__ void radix4(float2& v0, float2& v1, float2& v2, float2& v3) {
  const float2 t0 = make_float2(v0.x + v2.x, v0.y + v2.y);
  const float2 t1 = make_float2(v0.x - v2.x, v0.y - v2.y);
  const float2 t2 = make_float2(v1.x + v3.x, v1.y + v3.y);
  const float2 t3 = make_float2(v1.x - v3.x, v1.y - v3.y);
  v0 = make_float2(t0.x + t2.x, t0.y + t2.y);
  v2 = make_float2(t0.x - t2.x, t0.y - t2.y);
  v1 = make_float2(t1.x + t3.y, t1.y - t3.x);
  v3 = make_float2(t1.x - t3.y, t1.y + t3.x);
}

// forward DFT-16 in place; output X[k] ends up at x[P16(k)]
__device__ __forceinline__ void dft16(float2 (&x)[16]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) radix4(x[b], x[4 + b], x[8 + b], x[12 + b]);
  const float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
  x[5] = cmulf(x[5], make_float2(C1, -S1));                               // W16^1
  x[6] = make_float2((x[6].x + x[6].y) * H, (x[6].y - x[6].x) * H);       // W16^2
  x[7] = cmulf(x[7], make_float2(S1, -C1));                               // W16^3
  x[9] = make_float2((x[9].x + x[9].y) * H, (x[9].y - x[9].x) * H);       // W16^2
  x[10] = make_float2(x[10].y, -x[10].x);                                 // W16^4 = -i
  x[11] = make_float2((x[11].y - x[11].x) * H, -(x[11].x + x[11].y) * H); // W16^6
  x[13] = cmulf(x[13], make_float2(S1, -C1));                             // W16^3
  x[14] = make_float2((x[14].y - x[14].x) * H, -(x[14].x + x[14].y) * H); // W16^6
  x[15] = cmulf(x[15], make_float2(-C1, S1));                             // W16^9
#pragma unroll
  for (int c = 0; c < 4; ++c) radix4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
}

// dft16 when x[0 .. Z-1] and x[16-Z .. 15] are zero on entry (Z <= 7: a window that covers the middle of the frame only --
// the reference's dialog lets the user type n_fft while winLen stays 25 ms: 250 samples in 2048 leave pairs 7 and 8).
// The zeros are followed through BOTH radix-4 passes with compile-time flags: a butterfly drops the additions of its zero
// inputs (0 + v = v, 0 - v = -v, v -+ 0 = v: what the full pass computes, up to where the compiler contracts the window
// product into a first-pass addition: 1 - 2 ulp against the unpruned kernel), a column whose four inputs are all zero is
// zero and is skipped by its twiddle and by the second pass.  The zero inputs are not read.
template <bool Z0, bool Z1, bool Z2, bool Z3>
__device__ __forceinline__ void radix4_f(float2& v0, float2& v1, float2& v2, float2& v3) {
  if constexpr (Z0 && Z1 && Z2 && Z3) return;                 // a zero column: nothing to compute, nothing is read later
  constexpr bool ZA = Z0 && Z2, ZB = Z1 && Z3;                // t0 = t1 = 0 / t2 = t3 = 0
  float2 t0, t1, t2, t3;
  if constexpr (!ZA) {
    t0 = Z0 ? v2 : (Z2 ? v0 : make_float2(v0.x + v2.x, v0.y + v2.y));
    t1 = Z0 ? make_float2(-v2.x, -v2.y) : (Z2 ? v0 : make_float2(v0.x - v2.x, v0.y - v2.y));
  }
  if constexpr (!ZB) {
    t2 = Z1 ? v3 : (Z3 ? v1 : make_float2(v1.x + v3.x, v1.y + v3.y));
    t3 = Z1 ? make_float2(-v3.x, -v3.y) : (Z3 ? v1 : make_float2(v1.x - v3.x, v1.y - v3.y));
  }
  if constexpr (ZA) {
    v0 = t2; v2 = make_float2(-t2.x, -t2.y);
    v1 = make_float2(t3.y, -t3.x); v3 = make_float2(-t3.y, t3.x);
  } else if constexpr (ZB) {
    v0 = t0; v2 = t0; v1 = t1; v3 = t1;
  } else {
    v0 = make_float2(t0.x + t2.x, t0.y + t2.y);
    v2 = make_float2(t0.x - t2.x, t0.y - t2.y);
    v1 = make_float2(t1.x + t3.y, t1.y - t3.x);
    v3 = make_float2(t1.x - t3.y, t1.y + t3.x);
  }
}

template <int Z>
__device__ __forceinline__ void dft16_z(float2 (&x)[16]) {
  static_assert(Z >= 1 && Z <= 7, "zero pairs per end");
#define MM_ZF(i) ((i) < Z || (i) >= 16 - Z)
#define MM_CZ(b) (MM_ZF(b) && MM_ZF(4 + (b)) && MM_ZF(8 + (b)) && MM_ZF(12 + (b)))      // column b is zero after the first pass
  radix4_f<MM_ZF(0), MM_ZF(4), MM_ZF(8), MM_ZF(12)>(x[0], x[4], x[8], x[12]);
  radix4_f<MM_ZF(1), MM_ZF(5), MM_ZF(9), MM_ZF(13)>(x[1], x[5], x[9], x[13]);
  radix4_f<MM_ZF(2), MM_ZF(6), MM_ZF(10), MM_ZF(14)>(x[2], x[6], x[10], x[14]);
  radix4_f<MM_ZF(3), MM_ZF(7), MM_ZF(11), MM_ZF(15)>(x[3], x[7], x[11], x[15]);
  const float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
  if constexpr (!MM_CZ(1)) {
    x[5] = cmulf(x[5], make_float2(C1, -S1));                               // W16^1
    x[9] = make_float2((x[9].x + x[9].y) * H, (x[9].y - x[9].x) * H);       // W16^2
    x[13] = cmulf(x[13], make_float2(S1, -C1));                             // W16^3
  }
  if constexpr (!MM_CZ(2)) {
    x[6] = make_float2((x[6].x + x[6].y) * H, (x[6].y - x[6].x) * H);       // W16^2
    x[10] = make_float2(x[10].y, -x[10].x);                                 // W16^4 = -i
    x[14] = make_float2((x[14].y - x[14].x) * H, -(x[14].x + x[14].y) * H); // W16^6
  }
  if constexpr (!MM_CZ(3)) {
    x[7] = cmulf(x[7], make_float2(S1, -C1));                               // W16^3
    x[11] = make_float2((x[11].y - x[11].x) * H, -(x[11].x + x[11].y) * H); // W16^6
    x[15] = cmulf(x[15], make_float2(-C1, S1));                             // W16^9
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    radix4_f<MM_CZ(0), MM_CZ(1), MM_CZ(2), MM_CZ(3)>(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
#undef MM_CZ
#undef MM_ZF
}

// The same transform when x[0..3] and x[12..15] are zero on entry (a window of at most half the frame, centred: a lane's
// first and last four stage-1 inputs lie outside it): the first radix-4 pass takes (0, a, c, 0) -> a + c, -i a - c, c - a,
// i a - c -- eight additions per butterfly instead of sixteen: what the full pass makes of the zeros, up to the compiler's
// multiply-add contraction of the window products (1 - 2 ulp against the unpruned kernel).  Only x[4..11] are read.
__device__ __forceinline__ void dft16_mid8(float2 (&x)[16]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float2 a = x[4 + b], c = x[8 + b];
    x[b] = make_float2(c.x + a.x, c.y + a.y);
    x[4 + b] = make_float2(-c.x + a.y, -c.y - a.x);
    x[8 + b] = make_float2(c.x - a.x, c.y - a.y);
    x[12 + b] = make_float2(-c.x - a.y, -c.y + a.x);
  }
  const float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
  x[5] = cmulf(x[5], make_float2(C1, -S1));                               // W16^1
  x[6] = make_float2((x[6].x + x[6].y) * H, (x[6].y - x[6].x) * H);       // W16^2
  x[7] = cmulf(x[7], make_float2(S1, -C1));                               // W16^3
  x[9] = make_float2((x[9].x + x[9].y) * H, (x[9].y - x[9].x) * H);       // W16^2
  x[10] = make_float2(x[10].y, -x[10].x);                                 // W16^4 = -i
  x[11] = make_float2((x[11].y - x[11].x) * H, -(x[11].x + x[11].y) * H); // W16^6
  x[13] = cmulf(x[13], make_float2(S1, -C1));                             // W16^3
  x[14] = make_float2((x[14].y - x[14].x) * H, -(x[14].x + x[14].y) * H); // W16^6
  x[15] = cmulf(x[15], make_float2(-C1, S1));                             // W16^9
#pragma unroll
  for (int c = 0; c < 4; ++c) radix4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
}

template <int R>
struct Geo {
  static constexpr int LPR = 16 * R;          // lanes per row
  static constexpr int ROWS = 4 / R;          // rows per wave
  static constexpr int NC = 256 * R;          // complex points
  static constexpr int S = (R == 1) ? 18 : 34;  // padded LDS row pitch (complex), 16-B aligned rows
  static constexpr int ROWC = 16 * S;         // complex slots per row
  static constexpr int WAVE_C = ROWS * ROWC;  // complex slots per wave (1152 / 1088)
};

// per-lane constants, loaded once per kernel
template <int R>
struct LaneTw {
  float2 tw1[15];  // W_nc^(q*k1), k1 = 1..15
  float2 tw2[15];  // R = 2: p ? W_32^j : 1, j = 1..15
  float2 wp[9];    // 0.5 * (-i) * W_n^k, k = k1 + 16*(j + 16p), j = 0..8
};

template <int R>
__device__ __forceinline__ void load_lane_tw(LaneTw<R>& t, const float2* __restrict__ tw, int q) {
  constexpr int NC = Geo<R>::NC;
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) t.tw1[k1 - 1] = tw[(q * k1) * (MM_TW_N / NC)];
  const int k1 = (R == 1) ? q : (q >> 1);
  const int p = (R == 1) ? 0 : (q & 1);
  if (R == 2) {
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      const float2 w = tw[j * (MM_TW_N / 32)];
      t.tw2[j - 1] = p ? w : make_float2(1.0f, 0.0f);
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const float2 w = tw[(k1 + 16 * (j + 16 * p)) * (MM_TW_N / (2 * NC))];
    t.wp[j] = make_float2(0.5f * w.y, -0.5f * w.x);
  }
}

__device__ __forceinline__ float dpp_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}

// x[n1] = z[16R*n1 + q] on entry.  On exit x[P16(j)] = Z[k1 + 16*(j + 16p)].
// ex = this wave's LDS exchange buffer, row = lane / LPR, q = lane % LPR.
template <int R>
__device__ __forceinline__ void cfft(float2 (&x)[16], const LaneTw<R>& t, float2* ex, int row, int q) {
  typedef Geo<R> G;
  dft16(x);
  float2* wr = ex + row * G::ROWC + q;
  wr[0] = x[P16(0)];
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) wr[k1 * G::S] = cmulf(x[P16(k1)], t.tw1[k1 - 1]);
  wave_lds_sync();
  if (R == 1) {
    // 128 contiguous, 16-byte aligned bytes per lane: 8 x ds_read_b128, conflict-free at pitch 18
    const float4* rd = reinterpret_cast<const float4*>(ex + row * G::ROWC + q * G::S);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 v = rd[i];
      x[2 * i] = make_float2(v.x, v.y);
      x[2 * i + 1] = make_float2(v.z, v.w);
    }
  } else {
    const float2* rd = ex + row * G::ROWC + (q >> 1) * G::S + (q & 1);
#pragma unroll
    for (int m = 0; m < 16; ++m) x[m] = rd[2 * m];
  }
  wave_lds_sync();
  dft16(x);
  if (R == 2) {
    const float s = (q & 1) ? -1.0f : 1.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float2 g = x[P16(j)];
      if (j) g = cmulf(g, t.tw2[j - 1]);
      x[P16(j)] = make_float2(fmaf(s, g.x, dpp_xor1(g.x)), fmaf(s, g.y, dpp_xor1(g.y)));
    }
  }
}

// Value of lane (16 - q) % 16 of the same 16-lane row: reflection about lane 0 = row_mirror
// (q -> 15 - q) followed by a rotation by one lane.  Two DPP moves on the VALU instead of one
// ds_bpermute through the LDS pipe (which is the busier of the two in the fused kernels).
__device__ __forceinline__ float dpp_neg_lane16(float v) {
  const int m = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true);   // row_mirror
  return __int_as_float(__builtin_amdgcn_update_dpp(0, m, 0x121, 0xf, 0xf, true));         // row_ror:1
}

// Fetch the split partners: b[j] = Z[nc - k_j] for j = 0..8 (j = 8 only meaningful for k1 == 0).
template <int R>
__device__ __forceinline__ void fetch_partners(const float2 (&x)[16], float2 (&b)[9], int lane, int q) {
  constexpr int LPR = Geo<R>::LPR;
  const int k1 = (R == 1) ? q : (q >> 1);
  const int src_q = (R == 1) ? ((16 - k1) & 15) : ((((16 - k1) & 15) << 1) | ((q & 1) ^ 1));
  const int src = (lane & ~(LPR - 1)) | src_q;
  const bool z = (k1 == 0);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = 15 - j;                                       // partner register for k1 != 0
    const float2 a0 = x[P16(i)], a1 = x[P16((i + 1) & 15)];     // k1 == 0 lanes expose reg i+1
    const float qx = z ? a1.x : a0.x, qy = z ? a1.y : a0.y;
    if (R == 1) b[j] = make_float2(dpp_neg_lane16(qx), dpp_neg_lane16(qy));
    else b[j] = make_float2(__shfl(qx, src, 64), __shfl(qy, src, 64));
  }
  if (z) b[0] = x[P16(0)];
  if (R == 1) b[8] = make_float2(dpp_neg_lane16(x[P16(8)].x), dpp_neg_lane16(x[P16(8)].y));
  else b[8] = make_float2(__shfl(x[P16(8)].x, src, 64), __shfl(x[P16(8)].y, src, 64));
}

// X[k] and X[nc-k] from a = Z[k], b = Z[nc-k], wp = 0.5*(-i)*W_n^k
__device__ __forceinline__ void split_pair(float2 a, float2 b, float2 wp, float2& xa, float2& xb) {
  const float2 u = make_float2(a.x + b.x, a.y - b.y);   // a + conj b
  const float2 d = make_float2(a.x - b.x, a.y + b.y);   // a - conj b
  const float2 v = cmulf(d, wp);
  xa = make_float2(fmaf(0.5f, u.x, v.x), fmaf(0.5f, u.y, v.y));
  xb = make_float2(fmaf(0.5f, u.x, -v.x), fmaf(-0.5f, u.y, v.y));
}

}  // namespace f16

#ifndef MM_RFFT_WAVES_PER_SIMD
#define MM_RFFT_WAVES_PER_SIMD 2   // measured: 2 waves/SIMD 5.2-5.4 TB/s, 3: 5.0, 4: 4.7 (spills).  A variant
                                   // with 16-byte global accesses staged through LDS reached 5.05 TB/s:
                                   // access width is not what limits this kernel.
#endif
// ------------------------------------------------------------------------------------------
// Stage-isolated batched rFFT, n = 512 (R=1) or 1024 (R=2).  FAST: rows are 8-byte aligned and
// in_len == n (two-float loads, no masks); otherwise masked scalar loads (zero padding).
// ------------------------------------------------------------------------------------------
template <int R, bool FAST>
__global__ __launch_bounds__(256, MM_RFFT_WAVES_PER_SIMD) void rfft16_kernel(RfftParams p) {
  typedef f16::Geo<R> G;
  __shared__ __attribute__((aligned(16))) float2 ex_all[4 * G::WAVE_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane & (G::LPR - 1), row = lane / G::LPR;
  float2* ex = ex_all + wave * G::WAVE_C;
  f16::LaneTw<R> t;
  f16::load_lane_tw<R>(t, p.tw, q);
  const int k1 = (R == 1) ? q : (q >> 1);
  const int pp = (R == 1) ? 0 : (q & 1);
  const int64_t n_groups = (p.rows + G::ROWS - 1) / G::ROWS;

  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_groups; g += (int64_t)gridDim.x * 4) {
    const int64_t r = g * G::ROWS + row;
    const int64_t rl = r < p.rows ? r : p.rows - 1;
    const float* a = p.in + rl * p.in_stride;
    float2 x[16];
    if (FAST) {
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1)
        x[n1] = *reinterpret_cast<const float2*>(a + 2 * (G::LPR * n1 + q));
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int e = 2 * (G::LPR * n1 + q);
        x[n1].x = (e < p.in_len) ? a[e] : 0.0f;
        x[n1].y = (e + 1 < p.in_len) ? a[e + 1] : 0.0f;
      }
    }
    f16::cfft<R>(x, t, ex, row, q);
    float2 b[9];
    f16::fetch_partners<R>(x, b, lane, q);
    if (r < p.rows) {
      float2* o = reinterpret_cast<float2*>(p.out) + r * (G::NC + 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k1 + 16 * (j + 16 * pp);
        float2 xa, xb;
        f16::split_pair(x[f16::P16(j)], b[j], t.wp[j], xa, xb);
        o[k] = xa;
        o[G::NC - k] = xb;
      }
      if (k1 == 0) {
        float2 xa, xb;
        f16::split_pair(x[f16::P16(8)], b[8], t.wp[8], xa, xb);
        o[16 * (8 + 16 * pp)] = xa;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// logmel512_kernel: fused frame + Hann + rFFT-512 + |.|^2 (+ mel + 10 log10 + per-clip max), the
// 8-wave / 256-VGPR variant (mm_logmel16w.hip.inc holds the default 16-wave variant; this one is
// used when the mel run table does not fit beside the 16-wave kernel's LDS tiles, or with MM_PATH=1).
//
// One 512-thread workgroup per CU walks 64-frame tiles of the clips (persistent, static stride).
//   phase A  each wave transforms 2 x 4 frames (16 lanes per frame, f16::cfft<1>); the frame
//            samples come straight from global memory as 8-byte loads issued ONE ITEM AHEAD into a
//            second register set (every sample is fetched n_fft/hop times, but from L1/L2: the 32
//            frames the 8 waves work on span ~22 KB), the window comes from LDS, and the power row
//            goes to the LDS tile P[64][260]
//   phase B  lane <-> frame: the 8 waves split the mel filters; each walks its run table (bins that
//            share one "falling" filter d), one ds_read_b128 of the power row + two broadcast
//            ds_read_b128 of weights + 8 FMA per aligned 4-bin group, and emits
//            10*log10(max(amin, mel)) coalesced over frames when a filter is complete
// MODE 0 stores the power tile instead of phase B (stage test / fused-STFT roofline).
// LDS: 64*260*4 (P) + 8*9216 (exchange) + 2 KB window + run table -> one workgroup per CU.
// ------------------------------------------------------------------------------------------
struct Logmel512Params {
  const float* audio;
  int64_t batch, n_samples, stride, n_frames, tiles_per_clip, n_tiles;
  int hop, n_mels;
  float amin, db_offset, preemph;
  const float* window;    // [512]
  const float2* tw;
  const float4* mel_tab;  // run headers [n_runs] (int4 bits) followed by groups [n_groups][2]
  int n_runs, n_tab16;    // n_tab16 = n_runs + 2 * n_groups (16-byte units)
  const int* wave_part;   // [n_waves][4] = {run_begin, run_end, m_begin, m_end}
  const float* lane_tab;  // 16-wave kernel: [16][84] per-lane window / twiddle record
  float* out_logmel;      // [B][n_mels][T]
  int* clip_key;          // [B]
  float* out_power;       // MODE 0: [B][T][257]
  // fused (unclamped) DCT of the staged-sample kernel (mm_logmel16s.hip.inc); out_mfcc == nullptr: off
  float* out_mfcc;        // [B][n_mfcc][T]
  int* key_nmin;          // [B] keys of -(clip min), or nullptr
  const float* dct_a;     // [dct_kb][dct_nk][64] A operands: dct[16 kb + (l & 15)][4 s + (l >> 4)]
  int n_mfcc, dct_nk, dct_kb, lt_rows;
  int lt_b2;              // row offset of the second log-mel buffer: lt_rows, or 0 when there is only one (MM_S16F_SINGLE)
  unsigned lt_off, dcta_off;          // LDS byte offsets: log-mel tile (double buffered unless lt_single), A operands
  unsigned long long dct_roles;       // nibble w: frame block (0..3) whose DCT wave w computes, 0xF = none
  // dct_flags bit 0 (MM_S16F_SINGLE): ONE log-mel tile (a 128-filter bank does not fit twice): the DCT of tile i runs at
  // the top of tile i + 1's phase A instead of under its phase B.
  // bit 1 (MM_S16F_SKIP): filters without a single weight ("empty": fmax above Nyquist -- the reference's own default
  // call has 26 of 128 -- or mel bands narrower than a bin) always read 10 log10(amin): the run table flags them (bit 16
  // of a header's first word), phase B neither computes nor stores them, they take no part in the clip minimum, and
  // their share of the DCT is analytic: E[k] L0 in the accumulators' start values (E[k] = sum over empty m of
  // dct[k][m]; E follows the A operands in dct_a and in LDS, then one bit per filter "is empty" as 8 x u32) + E[k]
  // max(0, thr - L0) added to the clip's rows once thr is known.
  int dct_flags;
  // fused tail of the staged-sample kernel (clip mode; out_mod == nullptr: off): a workgroup owns WHOLE clips,
  // keeps their maximum / minimum itself (no keys, no atomics), redoes the DCT of a clip that clamps and
  // transforms the finished clip's coefficient trajectories (row A8)
  float2* out_mod;        // [B][n_mfcc][n_mod / 2 + 1]
  const float* dct_t;     // [n_mels][dct_kp] transposed DCT rows of the clamp fix-up
  int n_mod, dct_kp;
  float top_db;
  unsigned red_off;       // LDS byte offset of the per-wave clip max / min slots [2][16][2]
};

#define MM_S16F_SINGLE 1
#define MM_S16F_SKIP 2
#define MM_S16F_HALFWIN 8  // the window (in its 512-point frame) is zero outside samples [128, 384): pruned first stage
#define MM_LM_PITCH 260                      // power-row pitch (floats): 16-B aligned rows, b128 reads
#define MM_LM_P_FLOATS (64 * MM_LM_PITCH)
#define MM_LM_EX_OFF (MM_LM_P_FLOATS * 4)
#define MM_LM_WIN_OFF (MM_LM_EX_OFF + 8 * f16::Geo<1>::WAVE_C * 8)
#define MM_LM_TAB_OFF (MM_LM_WIN_OFF + 512 * 4)

#include "mm_tile512.hip.inc"                // what the five tile kernels share

struct LmItem {      // wave-uniform description of one phase-A item (4 frames of this wave)
  const float* a;    // clip base
  int64_t t_first;   // first frame of the 4
  bool live;         // tile < n_tiles
  bool interior;     // every sample of the whole tile is inside the clip: unmasked 8-byte loads
};

__device__ __forceinline__ LmItem lm_item(const Logmel512Params& p, int64_t tile, int it, int wave) {
  LmItem m;
  m.live = tile < p.n_tiles;
  const int64_t b = m.live ? tile / p.tiles_per_clip : 0;
  const int64_t t0 = m.live ? (tile - b * p.tiles_per_clip) * 64 : 0;
  m.a = p.audio + b * p.stride;
  m.interior = m.live && (t0 * p.hop - 256 >= 0) && ((t0 + 63) * p.hop + 255 < p.n_samples) &&
               (t0 + 63 < p.n_frames);
  m.t_first = t0 + 32 * it + 4 * wave;
  return m;
}

// Same, from an already decomposed tile index (b = clip, tl = tile within the clip): the persistent
// loops step (b, tl) incrementally -- a 64-bit tile / tiles_per_clip costs ~140 scalar instructions
// and the scalar ALU is shared by the whole CU.
__device__ __forceinline__ LmItem lm_item_bt(const Logmel512Params& p, bool live, int b, int tl, int it,
                                             int wave) {
  LmItem m;
  m.live = live;
  const int t0 = live ? tl * 64 : 0;
  m.a = p.audio + (int64_t)(live ? b : 0) * p.stride;
  m.interior = live && (t0 * p.hop - 256 >= 0) && ((int64_t)(t0 + 63) * p.hop + 255 < p.n_samples) &&
               (t0 + 63 < p.n_frames);
  m.t_first = t0 + 32 * it + 4 * wave;
  return m;
}

// Issue the global loads of an item into x (consumed one item later).  Branch-free on purpose (a
// conditional load makes the compiler merge "loaded" and "old" registers at the join and wait for
// the data right there): every lane loads the 8-byte pair at its sample index CLAMPED into the
// clip, so edge items (clip start / end, frames past the last one) are prefetched like interior
// ones and only get their out-of-range elements zeroed when they are consumed (lm_mask_edge).
__device__ __forceinline__ void lm_prefetch(float2 (&x)[16], const Logmel512Params& p, const LmItem& m,
                                            int row, int q) {
  const int base = (int)((m.t_first + row) * p.hop) - 256 + 2 * q;   // even; may be < 0 or >= n
  const int hi = ((int)p.n_samples & ~1) - 2;                          // last aligned pair of the clip
  int off[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) off[n1] = min(max(base + 32 * n1, 0), hi);
  __builtin_amdgcn_sched_barrier(0);   // pin the loads HERE: the scheduler otherwise sinks them to
#pragma unroll                         // their first use to save registers and the prefetch is lost
  for (int n1 = 0; n1 < 16; ++n1) x[n1] = *reinterpret_cast<const float2*>(m.a + off[n1]);
  __builtin_amdgcn_sched_barrier(0);
}

// Zero what lies outside the clip (centre padding) or belongs to a frame >= n_frames.
__device__ __forceinline__ void lm_mask_edge(float2 (&x)[16], const Logmel512Params& p, const LmItem& m,
                                             int row, int q) {
  const int64_t tt = m.t_first + row;
  const bool fv = m.live && tt < p.n_frames;
  const int base = (int)(tt * p.hop) - 256 + 2 * q;
  const int n = (int)p.n_samples;
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const int i0 = base + 32 * n1;
    const bool ok = fv && i0 >= 0 && i0 + 1 < n;     // the whole pair is inside: keep the load
    float vx = ok ? x[n1].x : 0.0f, vy = ok ? x[n1].y : 0.0f;
    if ((n & 1) && fv && i0 == n - 1) vx = m.a[i0];  // odd-length clip: its last sample has no pair
    x[n1] = make_float2(vx, vy);
  }
}

// Window, transform and store the power rows of one item.
__device__ __forceinline__ void lm_compute_item(float2 (&x)[16], const Logmel512Params& p,
                                                const LmItem& m, const float2* winq,
                                                const f16::LaneTw<1>& t, float2* ex, float* P, int it,
                                                int wave, int row, int q, int lane) {
  if (!m.interior) lm_mask_edge(x, p, m, row, q);
  // window from LDS (winq = table + q): keeps 32 VGPRs free for the prefetched item
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const float2 w = winq[16 * n1];
    x[n1].x *= w.x; x[n1].y *= w.y;
  }
  f16::cfft<1>(x, t, ex, row, q);
  float2 pb[9];
  f16::fetch_partners<1>(x, pb, lane, q);
  float pw[17];
  tile512_split_power(x, pb, t.wp, pw);
  tile512_store_power_row<false>(P + (32 * it + 4 * wave + row) * MM_LM_PITCH, q, pw);
}

template <int MODE>
__global__ __launch_bounds__(512) void logmel512_kernel(Logmel512Params p) {
  typedef f16::Geo<1> G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float2* ex = reinterpret_cast<float2*>(smem + MM_LM_EX_OFF) + wave * G::WAVE_C;
  const int q = lane & 15, row = lane >> 4;

  f16::LaneTw<1> t;
  f16::load_lane_tw<1>(t, p.tw, q);
  {
    float* wl = reinterpret_cast<float*>(smem + MM_LM_WIN_OFF);
    wl[threadIdx.x] = p.window[threadIdx.x];
  }
  for (int i = threadIdx.x; i < p.n_tab16; i += 512)   // mel run table -> LDS (broadcast b128 reads)
    reinterpret_cast<float4*>(smem + MM_LM_TAB_OFF)[i] = p.mel_tab[i];
  if (threadIdx.x < 64 * 3)                            // zero the 3 pad columns of every power row
    P[(threadIdx.x / 3) * MM_LM_PITCH + 257 + threadIdx.x % 3] = 0.0f;
  const float2* win = reinterpret_cast<const float2*>(smem + MM_LM_WIN_OFF) + q;
  __syncthreads();

  const int run0 = p.wave_part[wave * 4 + 0], run1 = p.wave_part[wave * 4 + 1];
  const int m0 = p.wave_part[wave * 4 + 2];

  float2 xa[16], xb[16];
  LmItem ia = lm_item(p, blockIdx.x, 0, wave), ib;
  lm_prefetch(xa, p, ia, row, q);

  for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
    const int64_t b = tile / p.tiles_per_clip;
    const int64_t t0 = (tile - b * p.tiles_per_clip) * 64;
    // ---------------- phase A ----------------
    ib = lm_item(p, tile, 1, wave);
    lm_prefetch(xb, p, ib, row, q);
    lm_compute_item(xa, p, ia, win, t, ex, P, 0, wave, row, q, lane);
    ia = lm_item(p, tile + gridDim.x, 0, wave);               // next tile, consumed after phase B
    lm_prefetch(xa, p, ia, row, q);
    lm_compute_item(xb, p, ib, win, t, ex, P, 1, wave, row, q, lane);
    wg_barrier_lds();
    // ---------------- phase B ----------------
    if (MODE == 0) {
      tile512_store_power_tile(p.out_power, P, MM_LM_PITCH, b, t0, p.n_frames, wave, 8, lane);
    } else {
      const bool valid = (t0 + lane) < p.n_frames;
      float* o = p.out_logmel + (b * p.n_mels) * p.n_frames + t0 + lane;
      const float* pl = P + lane * MM_LM_PITCH;
      const float4* hdr = reinterpret_cast<const float4*>(smem + MM_LM_TAB_OFF);
      const float4* grp = hdr + p.n_runs;
      float vmax = -INFINITY, carry = 0.0f;
      float4 h = hdr[run0];
      for (int r = run0; r < run1; ++r) {
        const Tile512Run rh = tile512_run_header(h);
        if (r + 1 < run1) h = hdr[r + 1];
        float sa = 0.0f, sb = 0.0f;
        tile512_group_dot<2>(reinterpret_cast<const float4*>(pl + rh.k4), grp + 2 * rh.go, rh.ng, sa, sb);
        if (rh.dd >= m0) {   // filter dd is complete: rising half from the previous run + falling half
          const float db = tile512_db(fmaxf(p.amin, carry + sa), p.db_offset);
          if (valid) {
            o[(int64_t)rh.dd * p.n_frames] = db;
            vmax = fmaxf(vmax, db);
          }
        }
        carry = sb;
      }
      vmax = wave_max(vmax);
      if (lane == 0 && vmax > -INFINITY) atomicMax(p.clip_key + b, float_key(vmax));
    }
    wg_barrier_lds();
  }
}
