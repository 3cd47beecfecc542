#pragma once
// Shared device pieces of the n_fft = 512 tile kernels: logmel512_kernel (W8, mm_fft16.hip.inc), logmel512w_kernel (W16,
// mm_logmel16w.hip.inc), logmel512h_kernel (H16, mm_logmel16h.hip.inc), logmel512s_kernel (S16, mm_logmel16s.hip.inc) and
// logmel12m_kernel (M12, mm_logmel12m.hip.inc).  The five are the same arithmetic with different occupancy and staging
// trades (tests/test_gpu_parity.py asserts bit-identical rows between them): what they share is said once, here.
// W8, W16 and H16 are written with these pieces.  S16 takes the record offsets, the split-twiddle read and the MODE 0 tile
// store, M12 the staging fix-up and the dB conversion; the rest of those two is their own code: with the shared form their
// registers change (M12) or the same-box A/B came out slower (S16; docs/experiments.md, "S16 over the shared tile pieces").
// Included by mm_fft16.hip.inc behind namespace f16, which everything below builds on.

// ---- lane record (one per lane q, pitch MM_W16_LT_PITCH floats in LDS): window pairs | stage-1 twiddles | split twiddles ----
#define MM_LT_WIN 0       // w[32 n1 + 2 q + {0, 1}], n1 = 0..15
#define MM_LT_TW 32       // W_256^(q k1), k1 = 1..15
#define MM_LT_WP 64       // 0.5 (-i) W_512^k, k = q + 16 j, j = 0..7

// float4 I0 .. I1 - 1 of a record section as complex pairs v[2 i], v[2 i + 1] (ds_read_b128, conflict-free at the pitch)
template <int I0, int I1, int N>
__device__ __forceinline__ void tile512_read_rec(float2 (&v)[N], const float* sec) {
  static_assert(0 <= I0 && 2 * I1 <= N, "record section");
  const float4* s4 = reinterpret_cast<const float4*>(sec);
#pragma unroll
  for (int i = I0; i < I1; ++i) {
    const float4 t = s4[i];
    v[2 * i] = make_float2(t.x, t.y);
    v[2 * i + 1] = make_float2(t.z, t.w);
  }
}
__device__ __forceinline__ void tile512_read_wp(float2 (&wp)[8], const float* rec) { tile512_read_rec<0, 4>(wp, rec + MM_LT_WP); }

// x[n1] *= window pair n1
__device__ __forceinline__ void tile512_window(float2 (&x)[16], const float* rec) {
  float2 w[16];
  tile512_read_rec<0, 8>(w, rec + MM_LT_WIN);
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) { x[n1].x *= w[n1].x; x[n1].y *= w[n1].y; }
}

// The stage-1 multiply X[k1] *= W_256^(q k1), k1 = 1..15 (X[k1] sits at x[P16(k1)]); tw = that section of the lane record
__device__ __forceinline__ void tile512_twiddle(float2 (&x)[16], const float* tw) {
  float2 w[16];
  tile512_read_rec<0, 8>(w, tw);
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1) x[f16::P16(k1)] = f16::cmulf(x[f16::P16(k1)], w[k1 - 1]);
}

// ---- the 16x16 exchange between the two DFT-16 stages ----
// A layout type holds a lane's write and read addresses: store(h) puts h[k1] at element (k1, n2 = q) of the lane's frame,
// load(h) fetches elements (k1 = q, n2 = 0..15) as four b128.
//
// Swizzled, inside the wave's OWN four power rows (`rows` = the first of them; the rows are written only after the
// exchange): element (k1, n2) of frame `row` at row*256 + k1*16 + (n2 ^ 4*((k1 >> 2) & 3)), one ds_write_b32 per element.
struct Tile512ExSwz {
  float* wq[4];
  const float4* rq[4];
  __device__ __forceinline__ Tile512ExSwz(float* rows, int row, int q) {
    float* exw = rows + row * 256;
    const int sq = (q >> 2) & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wq[i] = exw + (q ^ (4 * i));
      rq[i] = reinterpret_cast<const float4*>(exw + q * 16 + 4 * (i ^ sq));
    }
  }
  __device__ __forceinline__ void store(const float (&h)[16]) const {
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) wq[k1 >> 2][k1 * 16] = h[k1];
  }
  __device__ __forceinline__ float4 load(int i) const { return *rq[i]; }
};

// Wave-private buffer `buf`, row pitch 20 floats: b128 reads conflict-free, b32 writes 2-way = free.
struct Tile512ExP20 {
  float* wr;
  const float4* rd;
  __device__ __forceinline__ Tile512ExP20(float* buf, int row, int q)
      : wr(buf + row * 320 + q), rd(reinterpret_cast<const float4*>(buf + row * 320 + q * 20)) {}
  __device__ __forceinline__ void store(const float (&h)[16]) const {
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) wr[k1 * 20] = h[k1];
  }
  __device__ __forceinline__ float4 load(int i) const { return rd[i]; }
};

// In two halves (re, then im: the imaginary parts stay in stage-1 order x[P16(k1)].y meanwhile).  LDS operations of one
// wave execute in order, so wave_lds_sync() only keeps the compiler from moving accesses across the hand-over.
template <class EX>
__device__ __forceinline__ void tile512_exchange(float2 (&x)[16], const EX& ex) {
  float h[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) h[k1] = x[f16::P16(k1)].x;
  ex.store(h);
  wave_lds_sync();
  {
    const float4 v0 = ex.load(0), v1 = ex.load(1), v2 = ex.load(2), v3 = ex.load(3);
    x[0].x = v0.x; x[1].x = v0.y; x[2].x = v0.z; x[3].x = v0.w;
    x[4].x = v1.x; x[5].x = v1.y; x[6].x = v1.z; x[7].x = v1.w;
    x[8].x = v2.x; x[9].x = v2.y; x[10].x = v2.z; x[11].x = v2.w;
    x[12].x = v3.x; x[13].x = v3.y; x[14].x = v3.z; x[15].x = v3.w;
  }
  wave_lds_sync();
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) h[k1] = x[f16::P16(k1)].y;
  ex.store(h);
  wave_lds_sync();
  {
    const float4 v0 = ex.load(0), v1 = ex.load(1), v2 = ex.load(2), v3 = ex.load(3);
    x[0].y = v0.x; x[1].y = v0.y; x[2].y = v0.z; x[3].y = v0.w;
    x[4].y = v1.x; x[5].y = v1.y; x[6].y = v1.z; x[7].y = v1.w;
    x[8].y = v2.x; x[9].y = v2.y; x[10].y = v2.z; x[11].y = v2.w;
    x[12].y = v3.x; x[13].y = v3.y; x[14].y = v3.z; x[15].y = v3.w;
  }
  wave_lds_sync();
}

// ---- real split and power row ----
// Lane q of a frame holds Z[q + 16 j] at x[P16(j)]; pb = the split partners (f16::fetch_partners<1>), wp = the split
// twiddles.  pw[2 j] = |X[q + 16 j]|^2, pw[2 j + 1] = |X[256 - q - 16 j]|^2, pw[16] = |X[128]|^2 (lane q = 0's).
template <int NW>
__device__ __forceinline__ void tile512_split_power(const float2 (&x)[16], const float2 (&pb)[9], const float2 (&wp)[NW],
                                                    float (&pw)[17]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float2 xa, xb;
    f16::split_pair(x[f16::P16(j)], pb[j], wp[j], xa, xb);
    pw[2 * j] = fmaf(xa.x, xa.x, xa.y * xa.y);
    pw[2 * j + 1] = fmaf(xb.x, xb.x, xb.y * xb.y);
  }
  const float2 zm = x[f16::P16(8)];
  pw[16] = fmaf(zm.x, zm.x, zm.y * zm.y);
}

// pr = the frame's power row.  ZERO_PAD: the exchange of the frame ran over the row's pad bins 257..259 (Tile512ExSwz), which phase B reads as zeros.
template <bool ZERO_PAD>
__device__ __forceinline__ void tile512_store_power_row(float* pr, int q, const float (&pw)[17]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    pr[q + 16 * j] = pw[2 * j];
    pr[256 - q - 16 * j] = pw[2 * j + 1];
  }
  if (q == 0) {
    pr[128] = pw[16];
    if (ZERO_PAD) { pr[257] = 0.0f; pr[258] = 0.0f; pr[259] = 0.0f; }
  }
}

// MODE 0: the 64 power rows of tile (clip b, first frame t0) to out_power[b][t][257], a row per wave and pass
template <class I>
__device__ __forceinline__ void tile512_store_power_tile(float* out_power, const float* P, int pitch, I b, I t0,
                                                         int64_t n_frames, int wave, int n_waves, int lane) {
  for (int r = wave; r < 64; r += n_waves) {
    if (t0 + r < n_frames) {
      float* o = out_power + (((int64_t)b * n_frames) + t0 + r) * 257;
      const float* src = P + r * pitch;
      for (int k = lane; k < 257; k += 64) o[k] = src[k];
    }
  }
}

// ---- the mel run walk (phase B, lane <-> frame) ----
// A run = the bins that share one "falling" filter dd: header {first bin k4 (a multiple of 4), 4-bin groups ng, offset
// of its weight groups go, dd} as int bits in a float4, wave-uniform.  (The skip_empty tables of S16, MM_S16F_SKIP, also
// carry "filter dd has no weights" in bit 16 of the first word; S16 has its own decode; this one returns the word whole.)
struct Tile512Run { int k4, ng, go, dd; };
__device__ __forceinline__ Tile512Run tile512_run_header(const float4& h) {
  Tile512Run r;
  r.k4 = __builtin_amdgcn_readfirstlane(__float_as_int(h.x));
  r.ng = __builtin_amdgcn_readfirstlane(__float_as_int(h.y));
  r.go = __builtin_amdgcn_readfirstlane(__float_as_int(h.z));
  r.dd = __builtin_amdgcn_readfirstlane(__float_as_int(h.w));
  return r;
}

// The inner group dot: per aligned 4-bin group one b128 of the lane's power row (pp) and two broadcast b128 of weights,
// (wlo, whi) of bins 0,1 | 2,3, WS float4 apart from group to group -> sa (falling filter), sb (rising: the next run's carry).
template <int WS>
__device__ __forceinline__ void tile512_group_dot(const float4* pp, const float4* gw, int ng, float& sa, float& sb) {
#pragma unroll 2
  for (int g = 0; g < ng; ++g) {
    const float4 pv = pp[g];
    const float4 wa = gw[WS * g], wb = gw[WS * g + 1];
    sa = fmaf(wa.x, pv.x, sa); sb = fmaf(wa.y, pv.x, sb);
    sa = fmaf(wa.z, pv.y, sa); sb = fmaf(wa.w, pv.y, sb);
    sa = fmaf(wb.x, pv.z, sa); sb = fmaf(wb.y, pv.z, sb);
    sa = fmaf(wb.z, pv.w, sa); sb = fmaf(wb.w, pv.w, sb);
  }
}

// 10 log10(v) - db_offset of an energy already clamped to amin
__device__ __forceinline__ float tile512_db(float clamped, float db_offset) {
  return 3.0102999566398120f * __builtin_amdgcn_logf(clamped) - db_offset;
}

// ---- staging: one loaded four-sample group on its way to the LDS sample buffer ----
// v = the group loaded for samples s0 .. s0 + 3 of a clip of n samples, from an address clamped into the clip.
// UNAL (rows that are not 16-byte aligned, or n % 4 != 0): the one group that straddles the clip end was loaded
// k = s0 - (n - 4) samples early and is re-aligned; otherwise groups never straddle a clip edge.
// PRE: pre-emphasis y[n] - a y[n-1], prev = y[s0 - 1] (y[-1] := 0): the product rounded to float32, then subtracted
// (no fma) -- the float32 arithmetic of the definition.  Last, everything outside the clip is zeroed.
template <bool PRE, bool UNAL>
__device__ __forceinline__ float4 tile512_stage_fix(float4 v, int s0, int n, float prev, float preemph) {
  const bool ok = s0 >= 0 && s0 < n;
  if (UNAL) {
    const int k = s0 - (n - 4);
    if (k > 0) {
      const float4 l = v;
      v.x = k == 1 ? l.y : (k == 2 ? l.z : l.w);
      v.y = k == 1 ? l.z : l.w;        // k >= 2: past the end unless k == 2 -> masked below
      v.z = l.w;
    }
  }
  if (PRE) {
    const float pv = s0 > 0 ? prev : 0.0f;
    const float4 r = v;
    v.x = r.x - __fmul_rn(preemph, pv); v.y = r.y - __fmul_rn(preemph, r.x);
    v.z = r.z - __fmul_rn(preemph, r.y); v.w = r.w - __fmul_rn(preemph, r.z);
  }
  if (UNAL) {
    v.x = ok ? v.x : 0.0f; v.y = (ok && s0 + 1 < n) ? v.y : 0.0f;
    v.z = (ok && s0 + 2 < n) ? v.z : 0.0f; v.w = (ok && s0 + 3 < n) ? v.w : 0.0f;
  } else {
    v.x = ok ? v.x : 0.0f; v.y = ok ? v.y : 0.0f; v.z = ok ? v.z : 0.0f; v.w = ok ? v.w : 0.0f;
  }
  return v;
}
