#pragma once
// logmel_wpf_kernel<R, MODE>: "wave per frame group" fused frame + Hann + rFFT + |.|^2 + mel + log
// for n_fft = 512*R, R = 1, 2, 4 (the generalisation of the n_fft = 2048 kernel).  A wave owns
// F = 4/R consecutive frames of one clip from samples to log-mel rows; nothing is shared between
// waves, so there is NO workgroup barrier in the loop and the LDS footprint per wave (~10 KB) does
// not depend on n_fft: one power row of n_fft 2048 is 4.1 KB, which rules out the 64-frame LDS
// tile of the n_fft = 512 tile kernels (BASELINE configs[3], the "LDS pressure" case).
//
// Per frame NC = 256*R complex points z[m] = x[2m] + i x[2m+1] on L = 16*R lanes x 16 registers:
//   stage 1  lane ll (= n2) holds z[L*n1 + ll]: DFT-16 over n1, * W_NC^(ll*k1)
//   xchg A   16 x L transpose through LDS, re then im; A[k1][n2 = R*m + p] is written p-major so that
//            lane (k1, p) = lane R*k1 + p reads its 16 values with 4 x ds_read_b128
//   stage 2  DFT-16 over m -> F_p[j], * W_L^(p*j)
//   xchg B   (R > 1) R x 16 transpose inside each k1 group: lane (k1, u) gets G_p[(16/R)u + r]
//   stage 3  (R > 1) 16/R radix-R butterflies over p -> Z[k1 + 16*j + 256*d]
//   split    Z to LDS in natural order (re, then im; padded so the b32 writes are conflict-free);
//            lane ll forms the pairs k = ll + L*i, NC - k, i = 0..7
//   mel      power row in LDS with one pad word per 16 bins; lane ll sweeps ITS 16 bins (weights,
//            first filter index and "filter finished" flags of those bins are per-lane constants
//            in registers); every filter gets its value from three single-writer LDS slots (the
//            lane in which its run ends; the pre-summed group of lanes whose sweep ends inside its
//            run, for the falling and for the rising half) -- plain stores, no LDS atomics; then
//            lane <-> filter: add the three slots, log, max, one contiguous row store [b][t][n_mels]
// Per workgroup one table of per-lane constants (window, twiddles: 116 floats per lane of a frame).
#include "mm_wpf_core.hip.inc"

// PRE: pre-emphasis y[n] - a*y[n-1] (y[-1] := 0) on the frame loads: one more 4-byte load per pair
// W16: sixteen waves per workgroup (four per SIMD, 128 registers) instead of twelve (168): the sweep's 34 per-lane mel
// weights are read from an LDS table instead of held in registers, and the power row lies OVER the exchange / Z-staging
// buffer (every read of Z is through before the first power value is written) -- 6 KB of LDS per wave instead of 10.5.
#define MM_WPF_ML_PITCH 38      // floats per lane of the LDS mel table: (wlo, whi) x 17 | d_start | bits | pad (b64 reads conflict-free)
// Z: the window's zero pairs at both ends of a lane's register set (wpf_stages): their loads, clamps and products are left out
// NI < 8 (R > 1, MODE 1): the mel bank's highest bin with a weight lies below NC / 2 (fmax < sr / 4: BASELINE configs[3] has
// 10 kHz at 48 kHz) -> a lane forms only its first NI split pairs (bins ll + L i, i < NI) and none of the mirror bins NC - k;
// the power row's other entries keep the zeros they were given at the start.  (Compile-time: as wave-uniform run-time
// tests the same pruning cost 8 - 11 spilled registers.)
template <int R, int MODE, bool PRE, bool W16 = false, int Z = 0, int NI = 8>
__global__ __launch_bounds__((W16 || NI < 8) ? 1024 : 768) void logmel_wpf_kernel(WpfParams p) {
  typedef WpfGeo<R> G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* ltab = reinterpret_cast<float*>(smem);
  for (int i = threadIdx.x; i < G::L * MM_WPF_LT_PITCH; i += blockDim.x) ltab[i] = p.lane_tab[i];
  float* mtab = ltab + G::L * MM_WPF_LT_PITCH;          // W16: mel weights of the L lanes, (wlo, whi) interleaved
  if (W16)
    for (int i = threadIdx.x; i < G::L * 34; i += blockDim.x) {
      const int l = i / 34, e = i - l * 34, j = e >> 1;
      mtab[l * MM_WPF_ML_PITCH + e] = p.mel_lane[l * 36 + ((e & 1) ? 17 + j : j)];
    }
  // (NI < 8: the power row ends at bin NC / 2 - 1 -- MM_WPF_PBUF_HALF floats per wave instead of G::PBUF; with the ~120 registers of these
  // instantiations that is what lets SIXTEEN waves share a CU: the host picks the wave count by the LDS it leaves)
  constexpr int PBUF = (NI < 8 && R >= 2) ? MM_WPF_PBUF_HALF : G::PBUF;      // (R = 2: two frames' rows of 274 floats)
  const int ps_stride = W16 ? G::XBUF / G::F : ((NI < 8 && R >= 2) ? MM_WPF_PBUF_HALF / G::F : G::PS);   // floats between the power rows of a wave's frames
  const int wave_floats = G::XBUF + (W16 ? 0 : PBUF) + G::F * 3 * p.macc_stride;
  float* xbuf = ltab + G::L * MM_WPF_LT_PITCH + (W16 ? G::L * MM_WPF_ML_PITCH : 0) + wave * wave_floats;
  float* pbuf = W16 ? xbuf : xbuf + G::XBUF;
  float* mbuf = xbuf + G::XBUF + (W16 ? 0 : PBUF);
  for (int i = lane; i < (W16 ? G::XBUF : PBUF) + G::F * 3 * p.macc_stride; i += 64) (W16 ? xbuf : pbuf)[i] = 0.0f;
  __syncthreads();
  const int fw = lane / G::L, ll = lane % G::L;         // frame within the wave, lane within the frame
  const float* lt = ltab + ll * MM_WPF_LT_PITCH;
  const int k1 = ll / R, pq = ll % R;                   // stage-2 role (k1, p); stage-3 role (k1, u = pq)
  float* xf = xbuf + fw * G::XS;                        // this frame's exchange area
  float* zf = xbuf + fw * G::ZS;                        // this frame's Z-half area (same buffer, later)
  float* prow = pbuf + fw * ps_stride;
  float* macc = mbuf + fw * 3 * p.macc_stride;   // three slots per filter, see the mel phase

  // NI < 8: the bank ends below bin 512, the sweep's slices are EIGHT bins per lane (64 lanes cover bins 0 .. 511) with eight
  // slots; otherwise sixteen bins and a seventeenth slot for bin NC (the host builds the per-lane tables to match)
  constexpr int NSLOT = (NI < 8 && R >= 2) ? 8 : 17;
  // stage 3 through DPP butterflies instead of the second LDS exchange: on the full kernel within 1 % either way
  // (MM_WPF_DPPB, off); on the half-band instantiations -- sixteen waves, the LDS pipe their limit -- 3.7 % faster
  constexpr bool DPPB = MM_WPF_DPPB || (NI < 8 && R >= 2);
  float wlo[W16 ? 1 : NSLOT], whi[W16 ? 1 : NSLOT];
  if (!W16) {
    const float* ml = p.mel_lane + ll * 36;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) { wlo[W16 ? 0 : i] = ml[i]; whi[W16 ? 0 : i] = ml[17 + i]; }
  }
  const float2* mlw = reinterpret_cast<const float2*>(mtab + ll * MM_WPF_ML_PITCH);     // W16: (wlo, whi)[17]
  const int d_start = __float_as_int(p.mel_lane[ll * 36 + 34]);       // >= -1
  const unsigned flush_bits = (unsigned)__float_as_int(p.mel_lane[ll * 36 + 35]);   // bit i: advance before slot i

  // frame groups (F consecutive frames of one clip) are split evenly over the waves of the grid
  const int64_t n_waves = (int64_t)gridDim.x * p.waves_per_wg;
  const int64_t wid = (int64_t)blockIdx.x * p.waves_per_wg + wave;
  const int64_t g_begin = wid * p.total_groups / n_waves;
  const int64_t g_end = (wid + 1) * p.total_groups / n_waves;
  if (g_begin >= g_end) return;
  int64_t b = g_begin / p.groups_per_clip;
  int64_t gt = g_begin - b * p.groups_per_clip;         // group index within the clip
  float vmax = -INFINITY;
  const int n = (int)p.n_samples;
  const int hi = n - 2;                                  // last pair that is completely inside the clip

  float2 x[16];
  float xp[PRE ? 16 : 1];     // PRE: the sample before each pair
  auto prefetch = [&](int64_t bb, int64_t gg) {
    const float* a = p.audio + bb * p.stride;
    const int base = (int)((gg * G::F + fw) * p.hop) - G::NC + 2 * ll;
    // unsigned 32-bit byte offsets from the wave-uniform clip base: global_load saddr + voffset form,
    // no 64-bit address arithmetic per load
    // a group whose frames lie completely inside the clip (all but the first / last few of a clip) needs no clamping:
    // one per-lane byte offset, the sixteen loads at immediate offsets from it (the clamped form costs four vector
    // instructions per load: 64 of the ~930 per frame)
    const bool inside = !PRE && (gg * G::F * p.hop - G::NC >= 0) && ((gg * G::F + G::F - 1) * p.hop + G::NC - 1 < n);   // wave-uniform
    unsigned off[16];
    if (inside) {
#pragma unroll
      for (int n1 = Z; n1 < 16 - Z; ++n1) off[n1] = 4u * (unsigned)(base + 2 * G::L * n1);
    } else {
      // (the clamps hang on a value defined by a volatile statement of this arm: otherwise the compiler evaluates all
      // sixteen AHEAD of the branch, for every group -- 64 integer instructions per frame that only edge groups need)
      int bo = base;
      asm volatile("; edge group: clamped offsets" : "+v"(bo));
#pragma unroll
      for (int n1 = Z; n1 < 16 - Z; ++n1) off[n1] = 4u * (unsigned)min(max(bo + 2 * G::L * n1, 0), hi);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n1 = Z; n1 < 16 - Z; ++n1)
      {   // 8-byte load at a 4-byte aligned address (rows of odd pitch / odd lead): global memory takes it
        const MmFloat2U t = *reinterpret_cast<const MmFloat2U*>(reinterpret_cast<const char*>(a) + off[n1]);
        x[n1] = make_float2(t.x, t.y);
      }
    if (PRE) {
#pragma unroll
      for (int n1 = Z; n1 < 16 - Z; ++n1)
        xp[n1] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a) + (off[n1] >= 4u ? off[n1] - 4u : 0u));
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  prefetch(b, gt);

  for (int64_t g = g_begin; g < g_end; ++g) {
    const float* a = p.audio + b * p.stride;
    const int64_t t_first = gt * G::F;
    const int64_t t = t_first + fw;                      // this lane's frame
    const bool fvalid = t < p.n_frames;
    if (PRE) {
      const int base = (int)(t * p.hop) - G::NC + 2 * ll;
#pragma unroll
      for (int n1 = Z; n1 < 16 - Z; ++n1) {
        const float pv = (base + 2 * G::L * n1 > 0) ? xp[n1] : 0.0f;
        x[n1] = make_float2(x[n1].x - __fmul_rn(p.preemph, pv), x[n1].y - __fmul_rn(p.preemph, x[n1].x));   // no fma
      }
    }
    // ---- zero what lies outside the clip (centre padding) ----
    {
      const bool edge = (t_first * p.hop - G::NC < 0) || ((t_first + G::F - 1) * p.hop + G::NC - 1 >= n);
      if (edge) {   // wave-uniform
        const int base = (int)(t * p.hop) - G::NC + 2 * ll;
#pragma unroll
        for (int n1 = Z; n1 < 16 - Z; ++n1) {
          const int i0 = base + 2 * G::L * n1;
          const bool ok = i0 >= 0 && i0 + 1 < n;
          float vx = ok ? x[n1].x : 0.0f, vy = ok ? x[n1].y : 0.0f;
          // pairs that straddle a clip edge (odd hop: i0 may be -1; odd length or odd i0: n - 1)
          if (i0 == n - 1) vx = PRE ? a[i0] - __fmul_rn(p.preemph, a[i0 - 1]) : a[i0];
          if (i0 == -1) vy = a[0];
          x[n1] = make_float2(vx, vy);
        }
      }
    }
    wpf_stages<R, true, DPPB, Z>(x, lt, xf, ll, k1, pq);
    int64_t nb = b, ngt = gt + 1;
    if (ngt == p.groups_per_clip) { ngt = 0; ++nb; }
    const bool more = g + 1 < g_end;
    if (R == 1) {
      // ---- R = 1: x[P16(k2)] = Z[ll + 16*k2]; the split partners come through ds_bpermute (as in
      //      the tile kernels), no Z staging ----
      float2 pb[9];
      f16::fetch_partners<1>(x, pb, lane, ll);
      float2 wp[8];
      {
        const float4* s4 = reinterpret_cast<const float4*>(lt + 96);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 v = s4[i]; wp[2 * i] = make_float2(v.x, v.y); wp[2 * i + 1] = make_float2(v.z, v.w); }
      }
      float pw[17];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float2 xa, xb;
        f16::split_pair(x[f16::P16(j)], pb[j], wp[j], xa, xb);
        pw[2 * j] = fmaf(xa.x, xa.x, xa.y * xa.y);
        pw[2 * j + 1] = fmaf(xb.x, xb.x, xb.y * xb.y);
      }
      {
        const float2 zm = x[f16::P16(8)];
        pw[16] = fmaf(zm.x, zm.x, zm.y * zm.y);
      }
      prefetch(more ? nb : b, more ? ngt : gt);      // x is free now
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ka = ll + 16 * j, kb = 256 - ka;
        prow[ka + (ka >> 4)] = pw[2 * j];
        prow[kb + (kb >> 4)] = pw[2 * j + 1];
      }
      if (ll == 0) prow[128 + 8] = pw[16];
    } else {
    // ---- Z to LDS in natural order, re then im; lane ll picks up its pairs k = ll + L*i, NC - k ----
    float ar[8], br[8], ai[8], bi[8], mr = 0.0f, mi = 0.0f;
    constexpr int ni = NI;                                  // pairs this configuration's mel bank reads
    constexpr bool hb = NI < 8;                             // ... and nothing from bin NC / 2 up
    {
#pragma unroll
      for (int v = 0; v < 16; ++v)       // register slot v holds Z[wpf_zk(v)] (the layout depends on how stage 3 ran)
        zf[wpf_zidx<R, DPPB>(wpf_zk<R, DPPB>(k1, pq, v))] = x[wpf_zreg<R, DPPB>(v)].x;
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < ni) {
          const int k = ll + G::L * i, kp = (G::NC - k) & (G::NC - 1);
          ar[i] = zf[wpf_zidx<R, DPPB>(k)];
          br[i] = zf[wpf_zidx<R, DPPB>(kp)];
        }
      }
      if (!hb) mr = zf[wpf_zidx<R, DPPB>(G::NC / 2)];
      wave_lds_sync();
#pragma unroll
      for (int v = 0; v < 16; ++v)
        zf[wpf_zidx<R, DPPB>(wpf_zk<R, DPPB>(k1, pq, v))] = x[wpf_zreg<R, DPPB>(v)].y;
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < ni) {
          const int k = ll + G::L * i, kp = (G::NC - k) & (G::NC - 1);
          ai[i] = zf[wpf_zidx<R, DPPB>(k)];
          bi[i] = zf[wpf_zidx<R, DPPB>(kp)];
        }
      }
      if (!hb) mi = zf[wpf_zidx<R, DPPB>(G::NC / 2)];
    }
    wave_lds_sync();
    // ---- next group's samples (x is free now) ----
    prefetch(more ? nb : b, more ? ngt : gt);
    // ---- real split -> power row (padded index k + (k >> 4)) ----
    {
      float2 wp[8];
      {
        const float4* s4 = reinterpret_cast<const float4*>(lt + 96);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 v = s4[i]; wp[2 * i] = make_float2(v.x, v.y); wp[2 * i + 1] = make_float2(v.z, v.w); }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < ni) {
          const int k = ll + G::L * i;
          float2 xa, xb;
          f16::split_pair(make_float2(ar[i], ai[i]), make_float2(br[i], bi[i]), wp[i], xa, xb);
          const int ka = k, kb = G::NC - k;
          prow[ka + (ka >> 4)] = fmaf(xa.x, xa.x, xa.y * xa.y);
          if (!hb) prow[kb + (kb >> 4)] = fmaf(xb.x, xb.x, xb.y * xb.y);
        }
      }
      if (ll == 0 && !hb) prow[G::NC / 2 + G::NC / 32] = fmaf(mr, mr, mi * mi);
    }
    }
    wave_lds_sync();
    if (MODE == 0) {
#pragma unroll 1
      for (int f = 0; f < G::F; ++f) {
        if (t_first + f < p.n_frames) {
          float* o = p.out_power + (b * p.n_frames + t_first + f) * (G::NC + 1);
          const float* src = pbuf + f * ps_stride;
          for (int k = lane; k <= G::NC; k += 64) o[k] = src[k + (k >> 4)];
        }
      }
    } else {
      // ---- mel sweep over this lane's 17 slots (slot 16 = bin NC, weights 0 except the last lane) ----
      // Filter d's value lives at slot d + 1 of a slot row of n_mels + 2 floats (macc_stride >= that): d runs from -1 (bins
      // under the first filter's peak) to n_mels - 1 and d + 1 to n_mels, so NO store needs a bounds test -- slots 0 and
      // n_mels + 1 collect what belongs to no filter and are never read.  The flush ("run d ends before slot i": store A,
      // A <- Bc, Bc <- 0, next filter) is per-lane data, not control flow: lanes that do not flush at slot i store to a
      // dummy slot and keep their sums through selects -- 8 vector instructions per slot instead of a divergent branch
      // around 10 with its exec-mask bookkeeping (the sweep was a fifth of the kernel's vector instructions).
      float A = 0.0f, Bc = 0.0f;
      // (padded power row: bin k at k + (k >> 4); an eight-bin slice starts at 8 ll + (ll >> 1))
      const float* pl = NSLOT == 8 ? prow + 8 * ll + (ll >> 1) : prow + 17 * ll;
      const float plast = NSLOT == 8 ? 0.0f : prow[G::NC + G::NC / 16];
      MM_LDS float* ms = (MM_LDS float*)macc;
      MM_LDS float* dptr = ms + (d_start + 1);                  // slot of the current falling filter
      MM_LDS float* const dummy = ms + p.macc_stride - 1;       // slot row 0's last pad word: never read
      unsigned fb = flush_bits;
      asm volatile("" : "+v"(fb));      // opaque per frame: hoisted out of the frame loop the seventeen bit tests are
                                        // seventeen more live registers in a kernel at its cap (14 spills)
#pragma unroll
      for (int i = 0; i < NSLOT; ++i) {
        const bool fl = (fb >> i) & 1u;
        *(fl ? dptr : dummy) = A;                              // slot row 0: the one lane in which run d ends
        A = fl ? Bc : A;
        Bc = fl ? 0.0f : Bc;
        dptr += fl ? 1 : 0;
        const float pv = (i < 16) ? pl[i] : plast;
        const float2 wv = W16 ? mlw[i] : make_float2(wlo[W16 ? 0 : i], whi[W16 ? 0 : i]);
        A = fmaf(wv.x, pv, A);
        Bc = fmaf(wv.y, pv, Bc);
        // (the kernel sits at its 168-register cap: keep the scheduler from hoisting all seventeen power reads to the top)
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      // Every filter receives exactly three kinds of contribution, each from ONE lane, so plain stores
      // into three slot rows replace LDS atomics (a ds_add_f32 costs ~100+ cycles, a wave-wide one onto a
      // handful of addresses far more: the atomics were 0.68 of this kernel's 2.78 ms at C4):
      //   row 0  the sum a lane holds when run d ENDS inside it (above),
      //   row 1  what is left in A when the sweep ends (filter d): neighbouring lanes end in the same
      //          run, so these contiguous groups are summed in registers first (DPP wave_shr:1, one
      //          lane at a time, fixed order) and the group's last lane stores,
      //   row 2  the same for Bc (filter d + 1).
      // WHICH slots are written depends on the tables alone, not on the frame: every written slot is overwritten by
      // the next frame, every other one keeps the zero it was initialised with -- nothing is cleared between frames.
      {
        const int dist = (int)(flush_bits >> 20) & 15;
        float tA = A, tB = Bc;
        for (int k = 1; k <= p.group_max; ++k) {
          tA = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(tA), 0x138, 0xf, 0xf, true));   // wave_shr:1
          tB = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(tB), 0x138, 0xf, 0xf, true));
          A += (dist >= k) ? tA : 0.0f;
          Bc += (dist >= k) ? tB : 0.0f;
        }
        if ((flush_bits >> 24) & 1u) {
          dptr[p.macc_stride] = A;
          dptr[2 * p.macc_stride + 1] = Bc;
        }
      }
      wave_lds_sync();
#pragma unroll 1
      for (int f = 0; f < G::F; ++f) {
        const bool fv = t_first + f < p.n_frames;       // wave-uniform
        const float* mrow = mbuf + f * 3 * p.macc_stride + 1;
        float* o = p.out_logmel + b * p.sB + (t_first + f) * p.sT;
        for (int m = lane; m < p.n_mels; m += 64) {
          const float v = mrow[m] + mrow[p.macc_stride + m] + mrow[2 * p.macc_stride + m];
          if (fv) {
            const float db = 3.0102999566398120f * __builtin_amdgcn_logf(fmaxf(p.amin, v)) - p.db_offset;
            o[(int64_t)m * p.sM] = db;
            vmax = fmaxf(vmax, db);
          }
        }
      }
      if (!more || nb != b) {   // clip finished (or this wave's range ends): publish the maximum
        vmax = wave_max(vmax);
        if (lane == 0 && vmax > -INFINITY) atomicMax(p.clip_key + b, float_key(vmax));
        vmax = -INFINITY;
      }
    }
    (void)fvalid;
    wave_lds_sync();
    b = nb; gt = ngt;
  }
}

// Stage-isolated batched rFFT for n = 512*R on the same transform (wpf_stages): one wave per F = 4/R
// rows, no window; R = 4 (n = 2048) is the size the register radix-16 kernel of mm_fft16.hip.inc
// does not cover.  FAST: in_len == n, even row pitch, 8-byte aligned base (two-float loads, no
// masks); otherwise masked scalar loads (zero padding).  The next row group's samples are loaded
// while the current one is split and stored.
#ifndef MM_RFFT2K_WAVES_PER_SIMD
#define MM_RFFT2K_WAVES_PER_SIMD 3
#endif
template <int R, bool FAST>
__global__ __launch_bounds__(512, MM_RFFT2K_WAVES_PER_SIMD) void rfft_wpf_kernel(RfftParams p, const float* __restrict__ lane_tab) {
  typedef WpfGeo<R> G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* ltab = reinterpret_cast<float*>(smem);
  for (int i = threadIdx.x; i < G::L * MM_WPF_LT_PITCH; i += blockDim.x) ltab[i] = lane_tab[i];
  float* xbuf = ltab + G::L * MM_WPF_LT_PITCH + wave * G::XBUF;
  __syncthreads();
  const int fw = lane / G::L, ll = lane % G::L;
  const float* lt = ltab + ll * MM_WPF_LT_PITCH;
  const int k1 = ll / R, pq = ll % R;
  float* xf = xbuf + fw * G::XS;
  float* zf = xbuf + fw * G::ZS;
  const int64_t n_groups = (p.rows + G::F - 1) / G::F;
  const int64_t gstride = (int64_t)gridDim.x * 8;

  float2 x[16];
  auto fetch = [&](int64_t g) {
    int64_t r = g * G::F + fw;
    r = r < p.rows ? r : p.rows - 1;
    const float* a = p.in + r * p.in_stride;
    if (FAST) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) x[n1] = *reinterpret_cast<const float2*>(a + 2 * (G::L * n1 + ll));
      __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int e = 2 * (G::L * n1 + ll);
        x[n1].x = (e < p.in_len) ? a[e] : 0.0f;
        x[n1].y = (e + 1 < p.in_len) ? a[e + 1] : 0.0f;
      }
    }
  };
  int64_t g = (int64_t)blockIdx.x * 8 + wave;
  if (g >= n_groups) return;
  fetch(g);
  for (; g < n_groups; g += gstride) {
    wpf_stages<R, false>(x, lt, xf, ll, k1, pq);
    float ar[8], br[8], ai[8], bi[8], mr, mi;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int r = v / R, d = v % R;
      const int k = (R == 1) ? (k1 + 16 * v) : (k1 + 16 * ((16 / R) * pq + r) + 256 * d);
      zf[G::zidx(k)] = (R == 1) ? x[f16::P16(v)].x : x[v].x;
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = ll + G::L * i, kp = (G::NC - k) & (G::NC - 1);
      ar[i] = zf[G::zidx(k)];
      br[i] = zf[G::zidx(kp)];
    }
    mr = zf[G::zidx(G::NC / 2)];
    wave_lds_sync();
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int r = v / R, d = v % R;
      const int k = (R == 1) ? (k1 + 16 * v) : (k1 + 16 * ((16 / R) * pq + r) + 256 * d);
      zf[G::zidx(k)] = (R == 1) ? x[f16::P16(v)].y : x[v].y;
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = ll + G::L * i, kp = (G::NC - k) & (G::NC - 1);
      ai[i] = zf[G::zidx(k)];
      bi[i] = zf[G::zidx(kp)];
    }
    mi = zf[G::zidx(G::NC / 2)];
    wave_lds_sync();
    const int64_t row = g * G::F + fw;
    if (g + gstride < n_groups) fetch(g + gstride);      // x is free now
    if (row < p.rows) {
      float2* o = reinterpret_cast<float2*>(p.out) + row * (G::NC + 1);
      float2 wp[8];
      {
        const float4* s4 = reinterpret_cast<const float4*>(lt + 96);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 v = s4[i]; wp[2 * i] = make_float2(v.x, v.y); wp[2 * i + 1] = make_float2(v.z, v.w); }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = ll + G::L * i;
        float2 xa, xb;
        f16::split_pair(make_float2(ar[i], ai[i]), make_float2(br[i], bi[i]), wp[i], xa, xb);
        o[k] = xa;
        o[G::NC - k] = xb;
      }
      if (ll == 0) o[G::NC / 2] = make_float2(mr, -mi);
    }
  }
}

// Clamp + DCT-II for FRAME-MAJOR log-mel rows [B][T][n_mels] (the layout logmel_wpf_kernel writes):
// a 64-frame tile goes through LDS so that both the row reads and the [b][k][t] writes are coalesced.
// KB = coefficients per wave and pass: the four waves of a workgroup split the n_mfcc rows, so KB is
// chosen as ceil(n_mfcc / 4) rounded up to an instantiated size (40 MFCC: KB = 10, every wave busy,
// no padded rows -- this kernel is VALU-bound at C4: 80 x 40 MACs per frame).
template <int KB>
__global__ __launch_bounds__(256) void dct_clamp_fm_kernel(const float* __restrict__ logmel,
                                                            const int* __restrict__ clip_key,
                                                            const float* __restrict__ dct_t, float* __restrict__ out,
                                                            int64_t n_frames, int n_mels, int n_mfcc, int kp,
                                                            float top_db) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);   // [64][n_mels + 1]
  const int64_t bpc = (n_frames + 63) / 64;
  const int64_t b = blockIdx.x / bpc;
  const int64_t t0 = (blockIdx.x % bpc) * 64;
  const int nf = (int)((n_frames - t0) < 64 ? (n_frames - t0) : 64);
  const float thr = top_db >= 0.0f ? key_float(clip_key[b]) - top_db : -INFINITY;
  const float* src = logmel + (b * n_frames + t0) * n_mels;
  const int pitch = n_mels + 1;
  for (int fr = threadIdx.x >> 6; fr < nf; fr += 4)          // one wave per row: coalesced, no division
    for (int m = threadIdx.x & 63; m < n_mels; m += 64)
      tile[fr * pitch + m] = fmaxf(src[fr * n_mels + m], thr);
  __syncthreads();
  // thread = (frame lane, coefficient group): 4 groups of 64 lanes, group g handles k0 = 16*g, +64 ...
  const int fl = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: DCT rows come via s_load
  if (fl >= nf) return;
  const float* row = tile + fl * pitch;
  for (int k0 = g * KB; k0 < n_mfcc; k0 += 4 * KB) {
    float acc[KB];
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) acc[kk] = 0.0f;
#pragma unroll 4
    for (int m = 0; m < n_mels; ++m) {
      const float xv = row[m];
      const float* dd = dct_t + (size_t)m * kp + k0;
#pragma unroll
      for (int kk = 0; kk < KB; ++kk) acc[kk] = fmaf(dd[kk], xv, acc[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < KB; ++kk)
      if (k0 + kk < n_mfcc) out[(b * n_mfcc + k0 + kk) * n_frames + t0 + fl] = acc[kk];
  }
}

// Matrix-pipe form of the same clamp + DCT, a WAVE per 16-frame tile: D[16 coefficients x 16 frames] += DCT[16 x 4
// filters] * L[4 filters x 16 frames] with v_mfma_f32_16x16x4_f32 (exact f32, 32 cycles, 1024 MACs), 20 steps x 3
// coefficient blocks for 80 mel / 40 MFCC (at BASELINE configs[3] the VALU kernel above spends 0.26 ms on those MACs: a
// sixth of the FP32 rate).  A 64-frame tile per workgroup runs load -> barrier -> clamp into LDS -> barrier -> MFMA ->
// store as one serial chain (measured 0.18 ms at configs[3]: 2.7 TB/s where the 492 MB it moves would take 0.08 ms);
// here a wave owns its tile end to end -- wave-private LDS tile [16][pitch] with an odd pitch (the B operand reads --
// lane (frame j, kc) reads filter 4 s + kc -- are conflict-free but for one lane pair), no workgroup barrier in the
// loop -- and requests the NEXT tile's rows (five 16-byte loads per lane at 80 mel: 20 VGPRs, where prefetching a
// 64-frame tile had cost 24 more and an occupancy step) before it multiplies the current one, so the sixteen waves of a
// CU overlap their phases freely.  A operands [kbn][nk][64] (dct_a_operands) in LDS, once per workgroup.
// (First version: 0.18 ms like the 64-frame kernel.  Counters: 7.7 vector instructions per MFMA -- the run-time step
// index of the operand batches (`min(s0 + i, nk - 1)`, zero selects) made every LDS address a computed one, and on
// gfx950 vector instructions add to the f32 MFMA's time.  Now the step count is padded to a multiple of the batch CH on
// the host (zero A operands, tile pitch widened so that the padded reads stay inside the row) and every operand read
// is base + immediate offset.)
// U = 16-byte loads per lane and tile (16 frames x n_mels floats over 64 lanes: 5 at 80 mel, at most 8 = 128 mel);
// SPLIT = n_mels is not a multiple of 4 (a group of four floats can straddle two frames).
template <int CH, int MM_DCTW_U, bool SPLIT>
__global__ __launch_bounds__(256, 4) void dct_clamp_fm_wave_kernel(const float* __restrict__ logmel,
                                                                 const int* __restrict__ clip_key,
                                                                 const float* __restrict__ dct_a /*[kbn][nk][64]*/,
                                                                 float* __restrict__ out, int64_t n_frames, int64_t n_items,
                                                                 int n_mels, int n_mfcc, int nk, int kbn, float top_db) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int pitch = (4 * nk) | 1;                     // >= n_mels, odd
  float* At = reinterpret_cast<float*>(smem);         // [kbn][nk][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* Lw = At + kbn * nk * 64 + wave * 16 * pitch; // this wave's tile
  const int j = lane & 15, g = lane >> 4;
  for (int i = threadIdx.x; i < kbn * nk * 64; i += 256) At[i] = dct_a[i];
  for (int i = lane; i < 16 * pitch; i += 64) Lw[i] = 0.0f;       // filters past n_mels stay zero
  __syncthreads();
  const int64_t tpc = (n_frames + 15) / 16;
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  const int per_tile = 16 * n_mels;                   // floats of a full tile (contiguous in the frame-major workspace)
  // where this lane's u-th group of four floats lands in the tile (the same for every tile)
  int dst[MM_DCTW_U];
#pragma unroll
  for (int u = 0; u < MM_DCTW_U; ++u) {
    const int e = 4 * (lane + 64 * u);
    const int fr = e / n_mels;
    dst[u] = fr * pitch + (e - fr * n_mels);
  }
  constexpr bool rows_split = SPLIT;
  MmFloat4U v[MM_DCTW_U];
  auto request = [&](int64_t it) {
    const int64_t b = it / tpc, t0 = (it - b * tpc) * 16;
    const int nf = (int)((n_frames - t0) < 16 ? (n_frames - t0) : 16);
    const float* src = logmel + (b * n_frames + t0) * n_mels;
    const int total = nf * n_mels;
#pragma unroll
    for (int u = 0; u < MM_DCTW_U; ++u) {
      const int e = 4 * (lane + 64 * u);
      if (e + 3 < total) v[u] = *reinterpret_cast<const MmFloat4U*>(src + e);
      else if (e < per_tile) {
        v[u].x = e < total ? src[e] : 0.0f; v[u].y = e + 1 < total ? src[e + 1] : 0.0f;
        v[u].z = e + 2 < total ? src[e + 2] : 0.0f; v[u].w = e + 3 < total ? src[e + 3] : 0.0f;
      }
    }
  };
  int64_t it = (int64_t)blockIdx.x * 4 + wave;
  if (it < n_items) request(it);
  for (; it < n_items; it += n_waves) {
    const int64_t b = it / tpc, t0 = (it - b * tpc) * 16;
    const float thr = top_db >= 0.0f ? key_float(clip_key[b]) - top_db : -INFINITY;
    // clamp into the tile (rows past the clip's end were loaded as zeros: their columns are not stored)
#pragma unroll
    for (int u = 0; u < MM_DCTW_U; ++u) {
      const int e = 4 * (lane + 64 * u);
      if (e < per_tile) {
        const float q4[4] = {fmaxf(v[u].x, thr), fmaxf(v[u].y, thr), fmaxf(v[u].z, thr), fmaxf(v[u].w, thr)};
        if (!rows_split) {
          Lw[dst[u]] = q4[0]; Lw[dst[u] + 1] = q4[1]; Lw[dst[u] + 2] = q4[2]; Lw[dst[u] + 3] = q4[3];
        } else {
          int fr = e / n_mels, m = e - fr * n_mels;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (e + c < per_tile) Lw[fr * pitch + m] = q4[c];
            if (++m == n_mels) { m = 0; ++fr; }
          }
        }
      }
    }
    wave_lds_sync();
    if (it + n_waves < n_items) request(it + n_waves);           // in flight during the MFMAs below
    const int64_t t = t0 + j;
    const float* Ap = At + lane;                       // nk is a multiple of CH (host): [kbn][nk][64]
    for (int kb = 0; kb < kbn; ++kb) {
      const float* Bp = Lw + j * pitch + g;
      mm_f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int s0 = 0; s0 < nk; s0 += CH) {
        float av[CH], bv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          av[i] = Ap[i * 64];
          bv[i] = Bp[4 * i];
        }
        Ap += CH * 64; Bp += 4 * CH;
#pragma unroll
        for (int i = 0; i < CH; i += 2) {
          a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i + 1], bv[i + 1], a1, 0, 0, 0);
        }
      }
      if (t < n_frames) {
        float* o = out + (b * n_mfcc + 16 * kb + 4 * g) * n_frames + t;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * kb + 4 * g + r < n_mfcc) o[(int64_t)r * n_frames] = a0[r] + a1[r];
      }
    }
    wave_lds_sync();                                   // the tile's reads are done before the next clamp overwrites it
  }
}

// ---- host side of dct_clamp_fm_kernel: pick KB = ceil(n_mfcc / 4) rounded up to {4, 8, 10, 12, 16} ----
static bool set_dct_fm_attr(int bytes) {
  if (hipFuncSetAttribute((const void*)dct_clamp_fm_wave_kernel<10, 5, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536) != hipSuccess ||
      hipFuncSetAttribute((const void*)dct_clamp_fm_wave_kernel<10, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536) != hipSuccess ||
      hipFuncSetAttribute((const void*)dct_clamp_fm_wave_kernel<8, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536) != hipSuccess)
    return false;
  const void* fn[5] = {(const void*)dct_clamp_fm_kernel<4>, (const void*)dct_clamp_fm_kernel<8>,
                       (const void*)dct_clamp_fm_kernel<10>, (const void*)dct_clamp_fm_kernel<12>,
                       (const void*)dct_clamp_fm_kernel<16>};
  for (int i = 0; i < 5; ++i)
    if (hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  return true;
}

static void launch_dct_fm(dim3 grid, size_t lds, hipStream_t st, const float* logmel, const int* keys, const float* dct_t,
                          float* out, int64_t T, int n_mels, int n_mfcc, int kp, float top_db) {
  const int kb = (n_mfcc + 3) / 4;
#define MM_DCT_FM(KB) hipLaunchKernelGGL((dct_clamp_fm_kernel<KB>), grid, dim3(256), lds, st, logmel, keys, dct_t, out, T, n_mels, n_mfcc, kp, top_db)
  if (kb <= 4) MM_DCT_FM(4);
  else if (kb <= 8) MM_DCT_FM(8);
  else if (kb <= 10) MM_DCT_FM(10);
  else if (kb <= 12) MM_DCT_FM(12);
  else MM_DCT_FM(16);
#undef MM_DCT_FM
}
