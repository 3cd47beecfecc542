#pragma once
// (included by mm_logmel16s.hip, its own translation unit: 124 instantiations)
// logmel512s_kernel<MODE, NR>: the 16-wave fused n_fft = 512 kernel of mm_logmel16w.hip.inc with the
// tile's samples STAGED through LDS.  Measured on the direct-load variant (compile-time ablations, s_memtime
// stamps in tools/stamps.py): its 16 x 8-byte global loads per item -- every sample is fetched
// n_fft/hop = 3.2 times through the vector-memory pipe, 256 load instructions per tile and CU, ~60
// cycles of issue each -- cost 0.09 of its 0.51 ms.  Here
//
//   * the 63*hop + 512 samples a 64-frame tile touches are loaded ONCE, as 16-byte loads (NR per
//     lane, NR*1024 four-sample groups per tile) issued at the top of the previous tile's phase A;
//     they are zero-masked (centre padding, clip end) and written to the LDS sample buffer S right
//     behind the barrier that ends every wave's reads of the previous tile's samples;
//   * phase A reads its 16 complex points per lane from S with 16 x ds_read_b64 (one address
//     register, immediate offsets): no clamping, no edge masks, no 64-bit address arithmetic;
//   * the 16x16 exchange between the DFT-16 stages no longer has its own 80 KB: it runs inside the
//     wave's OWN four power rows of P (they are written only after the exchange); NR 3 / 4: one
//     ds_write_addtid_b32 per register (2 LDS cycles, a ds_write_b32 costs 4), 64-float blocks at
//     mm_s16_xb offsets that keep the b128 reads conflict-free.
//
// Requirements (checked by choose_kernel, which otherwise falls back to the direct-load kernel, or to the
// generic one for odd hops / pre-emphasis, which only this kernel of the n_fft = 512 family handles):
// n_samples >= 4, 63*hop + 512 <= NR*4096 (16-byte aligned rows and n_samples % 4 == 0 take the plain
// instantiation, anything else UNAL).
// LDS: P 68,608 (NR 3 / 4, pitch 268) or 66,560 (NR 1 / 2) | S NR*16,384 | lane records 5,376 | mel run table.
// PRE: pre-emphasis y[n] - a*y[n-1] (y[-1] := 0; the optional extension of this build, float32)
// applied while the samples are staged -- one extra 4-byte load per 16-byte group for y[s0 - 1].
// ODD: odd hop (odd frames start at 4-byte aligned samples only: two b32 LDS reads per point).
// UNAL: audio rows that are not 16-byte aligned, or a length that is not a multiple of 4: the 16-byte
// loads are issued at 4-byte aligned addresses (global memory takes them) and the one group per clip
// that straddles the clip end is re-aligned from its clamped load.

// Clip mode: the trajectory rFFT (row A8) of one finished clip inside the tile kernel -- the arithmetic of
// rfft16_kernel<R, false> (n_mod = 512 R), with the twiddles fetched where they are used instead of held in
// registers for a whole launch.  The first MM_S16_FIN_WAVES waves take the coefficient rows (4 / R per wave and
// pass); their exchange buffers lie over the power tile, which is dead between two tiles.
struct S16Fin {               // what the finalisation of a clip needs, passed by value (a real call, see below)
  const float* logmel;        // [B][n_mels][T]
  float* mfcc;                // [B][n_mfcc][T]
  float2* mod;                // [B][n_mfcc][n_mod / 2 + 1]
  const float2* tw;
  const float* dct_t;
  int n_frames, n_mels, n_mfcc, dct_kp, n_mod;
  float top_db;
  // MM_S16F_SKIP (Logmel512Params::dct_flags): the empty filters' rows were never stored; L0 = their constant value,
  // dct_e = E[16 kb] followed by the "is empty" bits (8 x u32), nullptr when the plan skips nothing
  float L0;
  const float* dct_e;
};

// Inside a called function pointers are generic ("flat") unless told otherwise: a flat load may alias LDS, so the
// compiler would drain every load before the next LDS store.  Everything below therefore goes through pointers
// with explicit address spaces (1 = global, 3 = LDS) and native vector types.
// Twiddles of the in-kernel trajectory rFFT, written to LDS once per launch: per lane q of a row (16 R lanes) a
// record of 24 complex values -- W_nc^(q i), i = 1..15, then 0.5 (-i) W_n^k for the lane's nine split pairs --
// followed (R = 2) by W_32^j, j = 1..15.  6264 bytes for n_mod = 1024.
template <int R>
__device__ __forceinline__ void s16_fin_fill_tab(const float2* tw_generic, MM_LDS mm_v2f* tab) {
  typedef f16::Geo<R> G;
  const MM_GLOBAL mm_v2f* tw = (const MM_GLOBAL mm_v2f*)tw_generic;
  for (int idx = threadIdx.x; idx < G::LPR * MM_S16_FIN_REC + 15; idx += 1024) {
    mm_v2f v;
    if (idx < G::LPR * MM_S16_FIN_REC) {
      const int q = idx / MM_S16_FIN_REC, e = idx - q * MM_S16_FIN_REC;
      if (e < 15) {
        v = tw[(q * (e + 1)) * (MM_TW_N / G::NC)];
      } else {
        const int j = e - 15, k1 = (R == 1) ? q : (q >> 1), pp = (R == 1) ? 0 : (q & 1);
        const mm_v2f w = tw[(k1 + 16 * (j + 16 * pp)) * (MM_TW_N / (2 * G::NC))];
        v = (mm_v2f){0.5f * w.y, -0.5f * w.x};
      }
    } else {
      v = tw[(idx - G::LPR * MM_S16_FIN_REC + 1) * (MM_TW_N / 32)];
    }
    tab[idx] = v;
  }
}

// A called function receives its arguments in VGPRs; the descriptor words must be PROVABLY wave-uniform, or every
// buffer operation is wrapped in a waterfall loop.
__device__ __forceinline__ void* mm_uniform_ptr(const void* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (void*)(((unsigned long long)hi << 32) | lo);
}

template <int R>
__device__ __forceinline__ void s16_fin_modspec(const S16Fin& f, int c0, int n_clips, int wave, int lane, MM_LDS float* P,
                                                const MM_LDS mm_v2f* tab) {
  typedef f16::Geo<R> G;
  const int q = lane & (G::LPR - 1), row = lane / G::LPR;
  MM_LDS mm_v2f* ex = reinterpret_cast<MM_LDS mm_v2f*>(P) + wave * G::WAVE_C;
  const MM_LDS mm_v2f* rec = tab + q * MM_S16_FIN_REC;      // this lane's twiddle record (s16_fin_fill_tab)
  const int k1 = (R == 1) ? q : (q >> 1);
  const int pp = (R == 1) ? 0 : (q & 1);
  const int n_items = (f.n_mfcc + G::ROWS - 1) / G::ROWS;
  const int T = f.n_frames;
  // the clip's MFCC rows, the twiddle table, the clip's spectrum rows
  // this workgroup's clips c0 .. c0 + n_clips - 1: their MFCC rows and their spectrum rows (each one descriptor)
  const int n_rows = __builtin_amdgcn_readfirstlane(f.n_mfcc * n_clips);
  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
      mm_uniform_ptr(f.mfcc + (int64_t)c0 * f.n_mfcc * T), 0, n_rows * __builtin_amdgcn_readfirstlane(T) * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(
      mm_uniform_ptr(f.mod + (int64_t)c0 * f.n_mfcc * (G::NC + 1)), 0, n_rows * (G::NC + 1) * 8, 0x00020000);
  MM_FIN_STAMP_BEGIN
  for (int it = wave; it < n_items * n_clips; it += 16) {
    const int cl = it / n_items, g = it - cl * n_items;       // clip (local), row group
    const int rr = g * G::ROWS + row;                         // row within the clip
    const bool live = rr < f.n_mfcc;
    const int r = cl * f.n_mfcc + (live ? rr : f.n_mfcc - 1); // row within the workgroup's block of rows
    const int rl = r;
    // samples e, e + 1 of the row, e = 2 (LPR n1 + q): unconditional loads (past the row they read the next row,
    // past the clip zeros), zeros selected afterwards
    const int in_off = (rl * T + 2 * q) * 4;
    float2 x[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) x[n1] = mm_buf_f32x2(r_in, in_off + 8 * G::LPR * n1);   // 4-byte aligned pairs
    mm_v2f t1[15];                           // W_nc^(q i): read while the samples are in flight
#pragma unroll
    for (int i = 0; i < 15; ++i) t1[i] = rec[i];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      const int e = 2 * (G::LPR * n1 + q);
      x[n1].x = e < T ? x[n1].x : 0.0f;
      x[n1].y = e + 1 < T ? x[n1].y : 0.0f;
    }
    MM_FIN_STAMP(0)
    f16::dft16(x);
    MM_LDS mm_v2f* wr = ex + row * G::ROWC + q;
    wr[0] = (mm_v2f){x[f16::P16(0)].x, x[f16::P16(0)].y};
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      const float2 v = f16::cmulf(x[f16::P16(i)], make_float2(t1[i - 1].x, t1[i - 1].y));
      wr[i * G::S] = (mm_v2f){v.x, v.y};
    }
    wave_lds_sync();
    if (R == 1) {
      const MM_LDS mm_v4f* rd = reinterpret_cast<const MM_LDS mm_v4f*>(ex + row * G::ROWC + q * G::S);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const mm_v4f v = rd[i];
        x[2 * i] = make_float2(v.x, v.y);
        x[2 * i + 1] = make_float2(v.z, v.w);
      }
    } else {
      const MM_LDS mm_v2f* rd = ex + row * G::ROWC + (q >> 1) * G::S + (q & 1);
#pragma unroll
      for (int m = 0; m < 16; ++m) { const mm_v2f v = rd[2 * m]; x[m] = make_float2(v.x, v.y); }
    }
    wave_lds_sync();
    MM_FIN_STAMP(1)
    mm_v2f t2[15];                           // W_32^j (R = 2), read before the second DFT-16 needs them
    if (R == 2) {
#pragma unroll
      for (int j = 0; j < 15; ++j) t2[j] = tab[G::LPR * MM_S16_FIN_REC + j];
      __builtin_amdgcn_sched_barrier(0);
    }
    f16::dft16(x);
    if (R == 2) {
      const float s = pp ? -1.0f : 1.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float2 v = x[f16::P16(j)];
        if (j) {
          const mm_v2f w = t2[j - 1];
          v = f16::cmulf(v, pp ? make_float2(w.x, w.y) : make_float2(1.0f, 0.0f));
        }
        x[f16::P16(j)] = make_float2(fmaf(s, v.x, f16::dpp_xor1(v.x)), fmaf(s, v.y, f16::dpp_xor1(v.y)));
      }
    }
    MM_FIN_STAMP(2)
    mm_v2f wpv[9];                           // 0.5 (-i) W_n^k, k = k1 + 16 (j + 16 p)
#pragma unroll
    for (int j = 0; j < 9; ++j) wpv[j] = rec[15 + j];
    __builtin_amdgcn_sched_barrier(0);
    float2 b[9];
    f16::fetch_partners<R>(x, b, lane, q);
    if (live) {
      const int out_off = (r * (G::NC + 1) + k1 + 256 * pp) * 8;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        if (j == 8 && k1 != 0) break;
        const int k = k1 + 16 * (j + 16 * pp);
        float2 xa, xb;
        f16::split_pair(x[f16::P16(j)], b[j], make_float2(wpv[j].x, wpv[j].y), xa, xb);
        __builtin_amdgcn_raw_buffer_store_b64((mm_v2u){__float_as_uint(xa.x), __float_as_uint(xa.y)}, r_out,
                                              out_off + 128 * j, 0, 0);
        if (j < 8)
          __builtin_amdgcn_raw_buffer_store_b64((mm_v2u){__float_as_uint(xb.x), __float_as_uint(xb.y)}, r_out,
                                                (r * (G::NC + 1) + G::NC - k) * 8, 0, 0);
      }
    }
    MM_FIN_STAMP(3)
  }
}

// Clip mode: the tail of the workgroup's clips, run ONCE at the end of the launch by a called function (inlined, its
// hundred live registers push the tile loop's own values out of the 128 VGPRs a 16-wave workgroup has; called from
// inside the loop, even a small wrapper left a scratch reload in every tile iteration).  By then every LDS tile is
// dead: the sixteen waves all take row groups (two rows of a clip per wave and pass), each with its own exchange
// buffer, and the twiddle table is written where the staging buffer was.
//
// s16_fix_clip: the clamped DCT of a clip with values under max - top_db (the arithmetic of dct_fixup_kernel: the
// correction of mm_clamp_corr added to the stored rows); all 1024 threads.
__device__ __attribute__((noinline)) void s16_fix_clip(S16Fin f, int c, float thr, bool stage) {
  // The DCT table [n_mels][kp] goes to the bottom of the LDS first (the tiles are dead; the extreme slots lie behind
  // everything the loop used): read from global memory here it would be vector loads per filter and frame -- this
  // function also stores to global memory, so the compiler cannot use the scalar cache.
  extern __shared__ __attribute__((aligned(16))) char fix_smem[];
  MM_LDS float* dl = (MM_LDS float*)fix_smem;
  if (stage) {           // workgroup-uniform: the first clip of this workgroup that clamps
    const MM_GLOBAL float* dct_t = (const MM_GLOBAL float*)f.dct_t;
    for (int i = threadIdx.x; i < f.n_mels * f.dct_kp; i += 1024) dl[i] = dct_t[i];
    __syncthreads();
  }
  const MM_GLOBAL unsigned* ebits = f.dct_e ? (const MM_GLOBAL unsigned*)(f.dct_e + 16 * ((f.n_mfcc + 15) / 16)) : nullptr;
  const MM_GLOBAL float* dct_e = (const MM_GLOBAL float*)f.dct_e;
  const float d0 = f.dct_e ? fmaxf(thr - f.L0, 0.0f) : 0.0f;        // the empty filters all read L0
  // the clip's log-mel rows through a buffer descriptor: lane offset 4 t, the row offset in a scalar register -- no
  // 64-bit address per load, so thirty-two of them fit the 128 registers of this workgroup
  const int row_bytes = __builtin_amdgcn_readfirstlane(f.n_frames) * 4;
  const __amdgpu_buffer_rsrc_t r_lm = __builtin_amdgcn_make_buffer_rsrc(
      mm_uniform_ptr(f.logmel + (int64_t)c * f.n_mels * f.n_frames), 0, __builtin_amdgcn_readfirstlane(f.n_mels) * row_bytes, 0x00020000);
#pragma unroll 1
  for (int t = threadIdx.x; t < f.n_frames; t += 1024) {
    MM_GLOBAL float* o = (MM_GLOBAL float*)f.mfcc + (int64_t)c * f.n_mfcc * f.n_frames + t;
#pragma unroll 1
    for (int k0 = 0; k0 < f.n_mfcc; k0 += MM_DCT_KB) {
      float acc[MM_DCT_KB];
#pragma unroll
      for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = 0.0f;
      bool touched = mm_clamp_corr(
          acc, f.n_mels, thr,
          [&](int m) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_lm, 4 * t, __builtin_amdgcn_readfirstlane(m) * row_bytes, 0)); },
          [&](int m0) { return ebits ? ebits[m0 >> 5] : 0u; },
          [&](int m, auto fn) {
            const MM_LDS mm_v4f* d = (const MM_LDS mm_v4f*)(dl + m * f.dct_kp + k0);
#pragma unroll
            for (int q4 = 0; q4 < MM_DCT_KB / 4; ++q4) {
              const mm_v4f dv = d[q4];
              fn(4 * q4, dv.x); fn(4 * q4 + 1, dv.y); fn(4 * q4 + 2, dv.z); fn(4 * q4 + 3, dv.w);
            }
          });
      if (d0 > 0.0f) {
#pragma unroll
        for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = __builtin_fmaf(dct_e[k0 + kk], d0, acc[kk]);
        touched = true;
      }
      if (touched) {
#pragma unroll
        for (int kk = 0; kk < MM_DCT_KB; ++kk)
          if (k0 + kk < f.n_mfcc) o[(int64_t)(k0 + kk) * f.n_frames] = o[(int64_t)(k0 + kk) * f.n_frames] + acc[kk];
      }
    }
  }
}

// skip_empty, a clip that does not clamp but whose threshold lies above L0: the empty filters' clamped value is thr, the
// accumulators started from E[k] L0 -> E[k] (thr - L0) is added to every element of the clip's rows (the arithmetic of
// dct_fixup_kernel's add branch: one explicit fmaf per element).  deltas[clip] = thr - L0, or 0 for a clip that needs
// nothing (or took the fix-up, which includes the empty filters' share).  All sixteen waves, a row each: 2048 elements
// per pass through a buffer descriptor (sixteen 8-byte loads in flight, 4-byte stores under the row's bound).
__device__ __attribute__((noinline)) void s16_add_rows(S16Fin f, int c0, int n_clips, unsigned delta_off) {
  extern __shared__ __attribute__((aligned(16))) char add_smem[];
  const float* deltas = reinterpret_cast<const float*>(add_smem + delta_off);
  const int ll = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = f.n_frames;
  const int n_rows = __builtin_amdgcn_readfirstlane(f.n_mfcc * n_clips);
  const MM_GLOBAL float* dct_e = (const MM_GLOBAL float*)f.dct_e;
#pragma unroll 1
  for (int r = wave; r < n_rows; r += 16) {
    const int cl = r / f.n_mfcc, k = r - cl * f.n_mfcc;
    const float delta = deltas[cl];
    if (delta == 0.0f) continue;          // (wave-uniform)
    const float ek = dct_e[k];
    // one descriptor per row: offsets stay far below 2^31 whatever the clip length, and a load past the row returns zero
    const __amdgpu_buffer_rsrc_t r_io = __builtin_amdgcn_make_buffer_rsrc(
        mm_uniform_ptr(f.mfcc + ((int64_t)c0 * f.n_mfcc + r) * T), 0, __builtin_amdgcn_readfirstlane(T) * 4, 0x00020000);
#pragma unroll 1
    for (int e0 = 0; e0 < T; e0 += 2048) {
      float2 x[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) x[n1] = mm_buf_f32x2(r_io, (e0 + 2 * (64 * n1 + ll)) * 4);
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int off = (e0 + 2 * (64 * n1 + ll)) * 4;       // (stores past the row's bound are dropped by the descriptor)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_fmaf(ek, delta, x[n1].x)), r_io, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_fmaf(ek, delta, x[n1].y)), r_io, off + 4, 0, 0);
      }
    }
  }
}

// n_mod = 2048 (1025 .. 2048 frames per clip: the reference's own default call on ten seconds is 2001): the trajectory rFFT
// on the wave-per-row transform of rfft_wpf_kernel<4> (mm_wpf_core.hip.inc: 1024 complex points on 64 lanes x 16
// registers, two LDS exchanges) -- every wave takes rows of the workgroup's clips; f.tw carries that kernel's lane table
// (116 floats per lane), copied to the bottom of the LDS, the waves' exchange buffers (4.5 KB each) behind it.
static_assert(MM_S16_FIN2K_BYTES == (64 * MM_WPF_LT_PITCH + 16 * WpfGeo<4>::XBUF) * 4, "LDS of the 2048-point tail (mm_s16.h)");
__device__ __attribute__((noinline)) void s16_fin_modspec_2k(S16Fin f, int c0, int n_clips, unsigned delta_off) {
  typedef WpfGeo<4> G;
  extern __shared__ __attribute__((aligned(16))) char fin2k_smem[];
  float* ltab = reinterpret_cast<float*>(fin2k_smem);
  // per clip: E[k] * this is still to be added (0xFFFFFFFF: the plan has no empty filters, nothing was written)
  const bool has_deltas = delta_off != 0xFFFFFFFFu;
  const float* deltas = reinterpret_cast<const float*>(fin2k_smem + (has_deltas ? delta_off : 0u));
  const int ll = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const MM_GLOBAL float* gt = (const MM_GLOBAL float*)f.tw;
    for (int i = threadIdx.x; i < G::L * MM_WPF_LT_PITCH; i += 1024) ltab[i] = gt[i];
  }
  __syncthreads();
  const float* lt = ltab + ll * MM_WPF_LT_PITCH;
  float* xf = ltab + G::L * MM_WPF_LT_PITCH + wave * G::XBUF;
  float* zf = xf;
  const int k1 = ll / 4, pq = ll % 4;
  const int T = f.n_frames;
  const int n_rows = __builtin_amdgcn_readfirstlane(f.n_mfcc * n_clips);
  // this workgroup's clips: their MFCC rows and their spectrum rows, one buffer descriptor each (32-bit offsets; a read
  // past the last row returns zero)
  const __amdgpu_buffer_rsrc_t r_io = __builtin_amdgcn_make_buffer_rsrc(
      mm_uniform_ptr(f.mfcc + (int64_t)c0 * f.n_mfcc * T), 0, n_rows * __builtin_amdgcn_readfirstlane(T) * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(
      mm_uniform_ptr(f.mod + (int64_t)c0 * f.n_mfcc * (G::NC + 1)), 0, n_rows * (G::NC + 1) * 8, 0x00020000);
  const MM_GLOBAL float* dct_e = (const MM_GLOBAL float*)f.dct_e;
#pragma unroll 1
  for (int r = wave; r < n_rows; r += 16) {
    // samples e, e + 1 of the row, e = 2 (64 n1 + ll): unconditional loads (past the row they read the next row), zeros
    // selected afterwards
    const int in_off = (r * T + 2 * ll) * 4;
    float2 x[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) x[n1] = mm_buf_f32x2(r_io, in_off + 8 * G::L * n1);       // 4-byte aligned pairs
    const int cl = r / f.n_mfcc, k = r - cl * f.n_mfcc;
    const float delta = has_deltas ? deltas[cl] : 0.0f;
    if (delta != 0.0f) {                  // (wave-uniform) the empty filters' share of a clip that does not clamp: the
      const float ek = dct_e[k];          // arithmetic of dct_fixup_kernel's add branch, stored back to the MFCC row
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int e = 2 * (G::L * n1 + ll);
        x[n1].x = __builtin_fmaf(ek, delta, x[n1].x);
        x[n1].y = __builtin_fmaf(ek, delta, x[n1].y);
        if (e < T) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x[n1].x), r_io, in_off + 8 * G::L * n1, 0, 0);
        if (e + 1 < T) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x[n1].y), r_io, in_off + 8 * G::L * n1 + 4, 0, 0);
      }
    }
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
      const int e = 2 * (G::L * n1 + ll);
      x[n1].x = e < T ? x[n1].x : 0.0f;
      x[n1].y = e + 1 < T ? x[n1].y : 0.0f;
    }
    wpf_stages<4, false>(x, lt, xf, ll, k1, pq);
    // split: Z through LDS in natural order (re, then im), lane ll forms the pairs k = ll + 64 i, 1024 - k
    float ar[8], br[8], ai[8], bi[8], mr, mi;
#pragma unroll
    for (int v = 0; v < 16; ++v) zf[G::zidx(k1 + 16 * (4 * pq + v / 4) + 256 * (v % 4))] = x[v].x;
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = ll + G::L * i, kp = (G::NC - kk) & (G::NC - 1);
      ar[i] = zf[G::zidx(kk)];
      br[i] = zf[G::zidx(kp)];
    }
    mr = zf[G::zidx(G::NC / 2)];
    wave_lds_sync();
#pragma unroll
    for (int v = 0; v < 16; ++v) zf[G::zidx(k1 + 16 * (4 * pq + v / 4) + 256 * (v % 4))] = x[v].y;
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = ll + G::L * i, kp = (G::NC - kk) & (G::NC - 1);
      ai[i] = zf[G::zidx(kk)];
      bi[i] = zf[G::zidx(kp)];
    }
    mi = zf[G::zidx(G::NC / 2)];
    wave_lds_sync();
    float2 wp[8];
    {
      const float4* s4 = reinterpret_cast<const float4*>(lt + 96);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float4 v = s4[i]; wp[2 * i] = make_float2(v.x, v.y); wp[2 * i + 1] = make_float2(v.z, v.w); }
    }
    const int out_off = r * (G::NC + 1) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = ll + G::L * i;
      float2 xa, xb;
      f16::split_pair(make_float2(ar[i], ai[i]), make_float2(br[i], bi[i]), wp[i], xa, xb);
      __builtin_amdgcn_raw_buffer_store_b64((mm_v2u){__float_as_uint(xa.x), __float_as_uint(xa.y)}, r_out, out_off + 8 * kk, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b64((mm_v2u){__float_as_uint(xb.x), __float_as_uint(xb.y)}, r_out,
                                            out_off + 8 * (G::NC - kk), 0, 0);
    }
    if (ll == 0)
      __builtin_amdgcn_raw_buffer_store_b64((mm_v2u){__float_as_uint(mr), __float_as_uint(-mi)}, r_out, out_off + 8 * (G::NC / 2), 0, 0);
  }
}

// LDS map of the tail: exchange buffers [0, 16 * WAVE_C * 8) over the power tile and the staging buffer, the twiddle
// table behind them (the launch allocates at least that much); the extreme slots red[clip][wave] (red_off, behind
// everything the loop used) are read first and may be overwritten afterwards.
__device__ __attribute__((noinline)) void s16_finalize_all(S16Fin f, int c0, int n_clips, unsigned red_off, int clips_max) {
  extern __shared__ __attribute__((aligned(16))) char fin_smem[];        // the kernel's dynamic LDS
  MM_LDS char* lds = (MM_LDS char*)fin_smem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // per-clip "still to add" factors of the empty filters: behind the extreme slots of the launch's largest workgroup,
  // and (n_mod 2048) behind the 2048-point tail's buffers -- MM_S16_DELTA_OFF, the host sizes the LDS with the same macro
  const unsigned delta_off = MM_S16_DELTA_OFF(red_off, clips_max, f.n_mod);
  __syncthreads();                       // every MFCC row of the workgroup's clips is stored; the tiles are dead
  bool adds = false;
  if (f.top_db >= 0.0f) {
    const MM_LDS mm_v2f* red = reinterpret_cast<const MM_LDS mm_v2f*>(lds + red_off);
    bool any = false, fixed = false;
#pragma unroll 1
    for (int cl = 0; cl < n_clips; ++cl) {
      float mx = -INFINITY, mn = INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const mm_v2f v = red[cl * 16 + i];
        mx = fmaxf(mx, v.x);
        mn = fminf(mn, v.y);
      }
      const float thr = mx - f.top_db;
      float delta = 0.0f;
      if (mn < thr) {                    // workgroup-uniform
        s16_fix_clip(f, c0 + cl, thr, !fixed);
        any = true; fixed = true;
      } else if (f.dct_e && thr > f.L0) {
        delta = thr - f.L0;
        adds = true;
      }
      if (f.dct_e && threadIdx.x == 0) *reinterpret_cast<MM_LDS float*>(lds + delta_off + 4 * cl) = delta;
    }
    if (any) __syncthreads();            // the corrected rows are what the transform reads
  }
  wg_barrier_lds();                      // every wave has read the extreme slots: the table may lie over them
  if (f.n_mod == 2048) {                 // the 2048-point tail adds while it reads the rows
    s16_fin_modspec_2k(f, c0, n_clips, (f.dct_e && f.top_db >= 0.0f) ? delta_off : 0xFFFFFFFFu);
    return;
  }
  if (adds) {                            // (workgroup-uniform)
    s16_add_rows(f, c0, n_clips, delta_off);
    __syncthreads();
  }
  if (f.n_mod == 0) return;              // clip mode without a modulation spectrum (mm_mfcc_f32 on a plan with empty filters)
  MM_LDS mm_v2f* tab = reinterpret_cast<MM_LDS mm_v2f*>(lds + MM_S16_FIN_TAB_OFF);
  if (f.n_mod == 1024) s16_fin_fill_tab<2>(f.tw, tab); else s16_fin_fill_tab<1>(f.tw, tab);
  wg_barrier_lds();
  if (f.n_mod == 1024) s16_fin_modspec<2>(f, c0, n_clips, wave, lane, (MM_LDS float*)lds, tab);
  else s16_fin_modspec<1>(f, c0, n_clips, wave, lane, (MM_LDS float*)lds, tab);
}

// One half (re or im) of the 16x16 exchange: v[k1] of every lane to the wave's area at mm_s16_xb(k1) + lane, sixteen
// ds_write_addtid_b32 (address M0[15:0] + offset + 4 lane; m0v = the area's LDS byte address, below 64 KB: mm_s16.h).
// M0 is reserved by the compiler and not preserved around inline assembly: saved, set and restored inside the
// statement; the s_nop is the wait state an SALU write of M0 needs before an add-TID LDS instruction.  The LDS
// operations of one wave execute in order: the reads behind the caller's wave_lds_sync() see these stores, and nothing
// here returns data the compiler would have to count.
__device__ __forceinline__ void s16_ex_store(unsigned m0v, const float (&v)[16]) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "ds_write_addtid_b32 %3 offset:%c19\n\t"
      "ds_write_addtid_b32 %4 offset:%c20\n\t"
      "ds_write_addtid_b32 %5 offset:%c21\n\t"
      "ds_write_addtid_b32 %6 offset:%c22\n\t"
      "ds_write_addtid_b32 %7 offset:%c23\n\t"
      "ds_write_addtid_b32 %8 offset:%c24\n\t"
      "ds_write_addtid_b32 %9 offset:%c25\n\t"
      "ds_write_addtid_b32 %10 offset:%c26\n\t"
      "ds_write_addtid_b32 %11 offset:%c27\n\t"
      "ds_write_addtid_b32 %12 offset:%c28\n\t"
      "ds_write_addtid_b32 %13 offset:%c29\n\t"
      "ds_write_addtid_b32 %14 offset:%c30\n\t"
      "ds_write_addtid_b32 %15 offset:%c31\n\t"
      "ds_write_addtid_b32 %16 offset:%c32\n\t"
      "ds_write_addtid_b32 %17 offset:%c33\n\t"
      "ds_write_addtid_b32 %18 offset:%c34\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "s"(m0v), "i"(0),
        "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]),
        "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]),
        "i"(4 * mm_s16_xb(0)), "i"(4 * mm_s16_xb(1)), "i"(4 * mm_s16_xb(2)), "i"(4 * mm_s16_xb(3)),
        "i"(4 * mm_s16_xb(4)), "i"(4 * mm_s16_xb(5)), "i"(4 * mm_s16_xb(6)), "i"(4 * mm_s16_xb(7)),
        "i"(4 * mm_s16_xb(8)), "i"(4 * mm_s16_xb(9)), "i"(4 * mm_s16_xb(10)), "i"(4 * mm_s16_xb(11)),
        "i"(4 * mm_s16_xb(12)), "i"(4 * mm_s16_xb(13)), "i"(4 * mm_s16_xb(14)), "i"(4 * mm_s16_xb(15))
      : "memory");
}

// From mm_tile512.hip.inc this kernel takes the lane-record offsets, the split-twiddle read and the MODE 0 tile store; the
// rest of phase A and the mel walk stay on its own code (docs/experiments.md, "S16 over the shared tile pieces").
#ifndef MM_S16_SH_PRIO
#define MM_S16_SH_PRIO 3
#endif
// SH ("shared runs", mm::build_mel_runs_shared; fused launches with two log-mel tiles only): every mel run is walked by
// ONE wave.  The wave whose last run ends at a part boundary leaves that run's second sum -- the rising half of the next
// part's first filter -- in the filter's own row of the current log-mel tile, in front of the end-of-tile barrier; the
// wave that owns the filter keeps its falling half in a register through phase B and finishes it right behind that
// barrier (same sum, same operand order as the walk's own `carry + sa`).  The per-clip extremes follow the finishing step.
template <int MODE, int NR, bool PRE, bool ODD, bool UNAL, bool XA, bool SH>
__global__ __launch_bounds__(1024) void logmel512s_kernel(Logmel512Params p) {
  static_assert(!XA || NR >= 3, "the addtid exchange exists for NR 3 / 4 only");
  static_assert(!SH || MODE != 0, "shared runs belong to the fused launches");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = reinterpret_cast<float*>(smem);
  float* S = reinterpret_cast<float*>(smem + MM_S16_S_OFF(XA));
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 15, row = lane >> 4;
  const float* lt = reinterpret_cast<const float*>(smem + MM_S16_LT_OFF(NR, XA)) + q * MM_W16_LT_PITCH;

  for (int i = threadIdx.x; i < 16 * MM_W16_LT_PITCH; i += 1024)
    reinterpret_cast<float*>(smem + MM_S16_LT_OFF(NR, XA))[i] = p.lane_tab[i];
  if (threadIdx.x < 64 * 3) P[(threadIdx.x / 3) * MM_S16_PITCH(XA) + 257 + threadIdx.x % 3] = 0.0f;

  for (int i = threadIdx.x; i < p.n_tab16; i += 1024)
    reinterpret_cast<float4*>(smem + MM_S16_TAB_OFF(NR, XA))[i] = p.mel_tab[i];
  const int run0 = p.wave_part[wave * 4 + 0], run1 = p.wave_part[wave * 4 + 1];
  const int m0 = p.wave_part[wave * 4 + 2];
  // SH: m_end | MM_RUNS_CONSUMER | MM_RUNS_PRODUCER of this wave's part (wave-uniform)
  const int m1f = SH ? __builtin_amdgcn_readfirstlane(p.wave_part[wave * 4 + 3]) : 0;
  // Fused DCT (MODE 1, p.out_mfcc): phase B also leaves its log-mel values in an LDS tile Lt[m][frame]
  // (double buffered, pitch 80 floats) and four "DCT waves" -- they walk half-size mel parts -- turn the
  // PREVIOUS tile's Lt into MFCC rows at the end of their phase B: D[16 coefficients x 16 frames] +=
  // DCT[16 x 4 filters] * Lt[4 filters x 16 frames] on v_mfma_f32_16x16x4_f32 (10 steps for 40 mel; exact f32).
  // The rows are the DCT of the UNCLAMPED log-mel values: dct_fixup_kernel redoes the clips that clamp.
  const bool fused = MODE == 2 || (MODE == 1 && p.out_mfcc != nullptr);      // MODE 2: clip mode, always fused
  float* Lt = reinterpret_cast<float*>(smem + p.lt_off);
  const int role = fused ? (int)((p.dct_roles >> (4 * wave)) & 15) : 15;
  const bool lt_single = fused && p.lt_b2 == 0;       // one log-mel tile: the DCT waves work at the top of phase A
  // (NR <= 2 only -- hop <= 121, where such windows live: in the NR 3 / 4 instantiations the second code path costs
  // registers the 128-VGPR budget does not have: 8 - 13 spills in the BASELINE kernels)
  const bool halfwin = NR <= 2 && (p.dct_flags & MM_S16F_HALFWIN) != 0;
  if (fused) {
    for (int i = threadIdx.x; i < (p.lt_b2 + p.lt_rows) * 80; i += 1024) Lt[i] = 0.0f;
    for (int i = threadIdx.x; i < p.dct_kb * p.dct_nk * 64 + 16 * p.dct_kb; i += 1024)      // A operands | E[k]
      reinterpret_cast<float*>(smem + p.dcta_off)[i] = p.dct_a[i];
  }
  float vmin = INFINITY;
  int pb = 0, pt0 = 0;          // clip and first frame of the previous tile
  bool has_prev = false;
  auto dct_tile = [&](const float* Lp, int cb, int ct0) {
    int ln = lane;                      // opaque copy: the addresses below are recomputed here instead of being
    asm volatile("" : "+v"(ln));        // hoisted out of the tile loop (the kernel sits at its 128-VGPR cap)
    const int j = ln & 15, g = ln >> 4;
    const int t = ct0 + 16 * role + j;
    const float* A = reinterpret_cast<const float*>(smem + p.dcta_off) + ln;
    const float* Bp = Lp + g * 80 + 16 * role + j;
    for (int kb = 0; kb < p.dct_kb; ++kb) {
      mm_f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = {0.0f, 0.0f, 0.0f, 0.0f};
      {                                   // the empty filters' share: E[16 kb + 4 g + r] L0 (E behind the A operands; zeros
                                          // when the plan skips no filter)
        const float4 e4 = *reinterpret_cast<const float4*>(A + (p.dct_kb * p.dct_nk * 64 + 16 * kb + 4 * g - ln));
        const float l0 = mm_empty_level(p.amin, p.db_offset);
        a0[0] = e4.x * l0; a0[1] = e4.y * l0; a0[2] = e4.z * l0; a0[3] = e4.w * l0;
      }
      if (p.dct_nk == 10) {
        // 40 mel (BASELINE configs[1] / [2]): exactly ten steps -- every operand read is base + immediate offset, no
        // step clamp, no zero select (the run-time step index of the general form below costs ~5 vector instructions
        // per MFMA, and on gfx950 those add to the f32 MFMA's time)
        const float* Ak = A + kb * 640;
        float av[10], bv[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          av[i] = Ak[i * 64];
          bv[i] = Bp[i * 320];
        }
#pragma unroll
        for (int i = 0; i < 10; i += 2) {
          a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i + 1], bv[i + 1], a1, 0, 0, 0);
        }
      } else
      // operands of MM_S16F_CH steps fetched together (an LDS read returns after several hundred cycles while the
      // other twelve waves walk their mel parts), then the MFMAs; steps past dct_nk re-read the last one
      // and multiply by zero
      // (whole batches, then the rest in pairs: a batch padded with zero products would cost 32 cycles of the SIMD's vector
      // issue per padding step -- 26 steps were 36 matrix instructions)
      {
        int s0 = 0;
        for (; s0 + MM_S16F_CH <= p.dct_nk; s0 += MM_S16F_CH) {
          float av[MM_S16F_CH], bv[MM_S16F_CH];
#pragma unroll
          for (int i = 0; i < MM_S16F_CH; ++i) {
            av[i] = A[(kb * p.dct_nk + s0 + i) * 64];
            bv[i] = Bp[(s0 + i) * 320];
          }
#pragma unroll
          for (int i = 0; i < MM_S16F_CH; i += 2) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i + 1], bv[i + 1], a1, 0, 0, 0);
          }
        }
        for (; s0 < p.dct_nk; s0 += 4) {          // at most MM_S16F_CH - 1 steps left: four at a time, the last ones times zero
          float av[4], bv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int s = min(s0 + i, p.dct_nk - 1);
            av[i] = s0 + i < p.dct_nk ? A[(kb * p.dct_nk + s) * 64] : 0.0f;
            bv[i] = Bp[s * 320];
          }
          a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], a1, 0, 0, 0);
          if (s0 + 2 < p.dct_nk) {                // (wave-uniform)
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], a1, 0, 0, 0);
          }
        }
      }
      if (t < p.n_frames) {
        float* o = p.out_mfcc + ((int64_t)cb * p.n_mfcc + 16 * kb + 4 * g) * p.n_frames + t;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * kb + 4 * g + r < p.n_mfcc) o[(int64_t)r * p.n_frames] = a0[r] + a1[r];
      }
    }
  };

  const int tpc = (int)p.tiles_per_clip;
  constexpr bool clip_mode = MODE == 2;          // whole clips per workgroup, fused tail (its own instantiation:
                                                 // the MODE 1 kernels are exactly what they were without it)
  const int tile_begin = clip_mode ? (int)((int64_t)blockIdx.x * p.batch / gridDim.x) * tpc
                                   : (int)((int64_t)blockIdx.x * p.n_tiles / gridDim.x);
  const int tile_end = clip_mode ? (int)((int64_t)(blockIdx.x + 1) * p.batch / gridDim.x) * tpc
                                 : (int)((int64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x);
  const int n = (int)p.n_samples;
  float vmax = -INFINITY;
  int b = tile_begin / tpc, tl = tile_begin - b * tpc;
  int nb = b, ntl = tl;

  // exchange area = this wave's own four power rows.  XA (1068 of the rows' 1072 floats): register
  // k1 of the 64 lanes goes out as ONE ds_write_addtid_b32 (lane l at mm_s16_xb(k1) + l: no address VGPR, 2 LDS cycles
  // where a ds_write_b32 costs 4), so element (k1, n2) of frame `row` lives at mm_s16_xb(k1) + 16 row + n2: lane q
  // writes column n2 = q of every k1 and reads block k1 = q of its frame as four b128 (conflict-free: mm_s16.h).
  // NR 1 / 2: element (k1, n2) of frame `row` at row*256 + k1*16 + (n2 ^ 4*((k1 >> 2) & 3)), ds_write_b32 per element.
  constexpr bool addtid = XA;
  float* exw = P + 4 * wave * MM_S16_PITCH(XA) + (addtid ? mm_s16_xb(q) + 16 * row : row * 256);
  const unsigned exm0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(MM_LDS float*)(P + 4 * wave * MM_S16_PITCH(XA)));
  float* wq0 = exw + (q ^ 0);
  float* wq1 = exw + (q ^ 4);
  float* wq2 = exw + (q ^ 8);
  float* wq3 = exw + (q ^ 12);
  const int sq = addtid ? 0 : (q >> 2) & 3;
  const int rq = addtid ? 0 : q * 16;
  const float4* rq0 = reinterpret_cast<const float4*>(exw + rq + 4 * (0 ^ sq));
  const float4* rq1 = reinterpret_cast<const float4*>(exw + rq + 4 * (1 ^ sq));
  const float4* rq2 = reinterpret_cast<const float4*>(exw + rq + 4 * (2 ^ sq));
  const float4* rq3 = reinterpret_cast<const float4*>(exw + rq + 4 * (3 ^ sq));
  // this lane's 16 points of its frame: S[(4*wave + row)*hop + 2q + 32*n1]
  const float* sxf = S + (4 * wave + row) * p.hop + 2 * q;
  const float2* sx = reinterpret_cast<const float2*>(sxf);
  constexpr bool hop_odd = ODD;      // odd hop: odd frames start at 4-byte aligned samples only -> two b32 reads

  // the four-sample groups this thread stages: g = tid + 1024*j (clamped loads, masked on store)
  float4 sreg[NR];
  float sprev[PRE ? NR : 1];
  auto stage_interior = [&](int ttl) -> bool {
    const int base = ttl * 64 * p.hop - 256;
    return base >= 0 && base + NR * 4096 <= n;
  };
  auto stage_load = [&](int bb, int ttl) {
    const float* a = p.audio + (int64_t)bb * p.stride;
    const int first = ttl * 64 * p.hop - 256 + 4 * (int)threadIdx.x;
    int off[NR];
    // a tile whose whole staging window lies inside the clip (all but the first and the last one or two of a clip) needs
    // neither the address clamps here nor the zero masks in stage_store: wave-uniform test
    if (stage_interior(ttl)) {
#pragma unroll
      for (int j = 0; j < NR; ++j) off[j] = first + 4096 * j;
    } else {
#pragma unroll
      for (int j = 0; j < NR; ++j) off[j] = min(max(first + 4096 * j, 0), n - 4);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if (UNAL) {
        const MmFloat4U t = *reinterpret_cast<const MmFloat4U*>(a + off[j]);
        sreg[j] = make_float4(t.x, t.y, t.z, t.w);
      } else {
        sreg[j] = *reinterpret_cast<const float4*>(a + off[j]);
      }
    }
    if (PRE) {
#pragma unroll
      for (int j = 0; j < NR; ++j) sprev[j] = a[min(max(first + 4096 * j - 1, 0), n - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_store = [&](int ttl) {
    const int first = ttl * 64 * p.hop - 256 + 4 * (int)threadIdx.x;
    if (!PRE && stage_interior(ttl)) {          // nothing to mask, nothing to re-align: the loaded groups as they are
#pragma unroll
      for (int j = 0; j < NR; ++j) reinterpret_cast<float4*>(S)[threadIdx.x + 1024 * j] = sreg[j];
      return;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int s0 = first + 4096 * j;
      const bool ok = s0 >= 0 && s0 < n;       // !UNAL: groups never straddle a clip edge (n % 4 == 0)
      float4 v = sreg[j];
      if (UNAL) {      // the group that straddles the clip end was loaded k samples early (address clamped to n - 4)
        const int k = s0 - (n - 4);
        if (k > 0) {
          const float4 l = v;
          v.x = k == 1 ? l.y : (k == 2 ? l.z : l.w);
          v.y = k == 1 ? l.z : l.w;        // k >= 2: past the end unless k == 2 -> masked below
          v.z = l.w;
        }
      }
      if (PRE) {
        const float pv = s0 > 0 ? sprev[j] : 0.0f;
        const float4 r = v;
        // product rounded to float32, then subtracted (no fma): the float32 arithmetic of the definition
        v.x = r.x - __fmul_rn(p.preemph, pv); v.y = r.y - __fmul_rn(p.preemph, r.x);
        v.z = r.z - __fmul_rn(p.preemph, r.y); v.w = r.w - __fmul_rn(p.preemph, r.z);
      }
      if (UNAL) {
        v.x = ok ? v.x : 0.0f; v.y = (ok && s0 + 1 < n) ? v.y : 0.0f;
        v.z = (ok && s0 + 2 < n) ? v.z : 0.0f; v.w = (ok && s0 + 3 < n) ? v.w : 0.0f;
      } else {
        v.x = ok ? v.x : 0.0f; v.y = ok ? v.y : 0.0f; v.z = ok ? v.z : 0.0f; v.w = ok ? v.w : 0.0f;
      }
      reinterpret_cast<float4*>(S)[threadIdx.x + 1024 * j] = v;
    }
  };
  if (tile_begin < tile_end) {
    stage_load(b, tl);
    stage_store(tl);
  }
  __syncthreads();
  // the split partners come through DPP, which leaves ~40 VGPRs under the 128 of 4 waves/SIMD: the split twiddles stay
  // in registers for the whole launch (every ds_read_b128 of a per-lane constant costs the LDS pipe ~6 cycles per item)
  float2 wp[8];
  tile512_read_wp(wp, lt);

  MM_STAMP_BEGIN(16)
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int t0 = tl * 64;
    MM_STAMP_AT(9)
    if (++ntl == tpc) { ntl = 0; ++nb; }
    const bool more = tile + 1 < tile_end;
    // next tile's samples: issued first, in flight during phase A (no other vector-memory traffic
    // there, so the wait before they are written to S after the barrier is for these loads only)
    stage_load(more ? nb : b, more ? ntl : tl);
    MM_STAMP_AT(11)
    // ---------------- phase A: one item (4 frames) per wave ----------------
    // (a wave whose four frames all lie behind the clip's last frame -- the tail of a clip's last tile -- skips its
    // item: nobody stores what phase B makes of those frames' stale power rows)
    if (t0 + 4 * wave < (int)p.n_frames) {
    float2 x[16];
    if (halfwin) {     // wave-uniform: a window of at most 256 samples, centred -- a lane's pairs n1 = 4 .. 11 only
      // (the reference's default call: 250 samples in 512; also every plan whose n_fft <= 256 rides on this kernel)
      if (hop_odd) {
#pragma unroll
        for (int n1 = 4; n1 < 12; ++n1) x[n1] = make_float2(sxf[32 * n1], sxf[32 * n1 + 1]);
      } else {
#pragma unroll
        for (int n1 = 4; n1 < 12; ++n1) x[n1] = sx[16 * n1];
      }
      const float4* w4 = reinterpret_cast<const float4*>(lt) + 2;        // window values of pairs 4 .. 11
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 t = w4[i];
        x[4 + 2 * i].x *= t.x; x[4 + 2 * i].y *= t.y;
        x[5 + 2 * i].x *= t.z; x[5 + 2 * i].y *= t.w;
      }
      MM_STAMP_AT(0)
      f16::dft16_mid8(x);
    } else {
    if (hop_odd) {     // wave-uniform
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) x[n1] = make_float2(sxf[32 * n1], sxf[32 * n1 + 1]);
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) x[n1] = sx[16 * n1];
    }
    {
      float2 w[16];
      tile512_read_rec<0, 8>(w, lt);                       // window
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) { x[n1].x *= w[n1].x; x[n1].y *= w[n1].y; }
    }
    MM_STAMP_AT(0)
    f16::dft16(x);
    }
    MM_STAMP_AT(1)
    {
      // W_256^(q*k1), k1 = 1..15, from the lane record
      float2 w[16];
      const float4* t4 = reinterpret_cast<const float4*>(lt + MM_LT_TW);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 t = t4[i];
        w[2 * i] = make_float2(t.x, t.y);
        w[2 * i + 1] = make_float2(t.z, t.w);
      }
#pragma unroll
      for (int k1 = 1; k1 < 16; ++k1)
        x[f16::P16(k1)] = f16::cmulf(x[f16::P16(k1)], w[k1 - 1]);
    }
    MM_STAMP_AT(2)
    {
#define MM_S16_WR(k1, val)                                                                         \
  (((k1) >> 2) == 0 ? wq0 : ((k1) >> 2) == 1 ? wq1 : ((k1) >> 2) == 2 ? wq2 : wq3)[(k1) * 16] = (val)
      {
        float re[16];
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) re[k1] = x[f16::P16(k1)].x;
        if constexpr (addtid) {
          s16_ex_store(exm0, re);
        } else {
#pragma unroll
          for (int k1 = 0; k1 < 16; ++k1) MM_S16_WR(k1, re[k1]);
        }
      }
      wave_lds_sync();
      {
        const float4 v0 = *rq0, v1 = *rq1, v2 = *rq2, v3 = *rq3;
        x[0].x = v0.x; x[1].x = v0.y; x[2].x = v0.z; x[3].x = v0.w;
        x[4].x = v1.x; x[5].x = v1.y; x[6].x = v1.z; x[7].x = v1.w;
        x[8].x = v2.x; x[9].x = v2.y; x[10].x = v2.z; x[11].x = v2.w;
        x[12].x = v3.x; x[13].x = v3.y; x[14].x = v3.z; x[15].x = v3.w;
      }
      wave_lds_sync();
      float im[16];
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) im[k1] = x[f16::P16(k1)].y;
      if constexpr (addtid) {
        s16_ex_store(exm0, im);
      } else {
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) MM_S16_WR(k1, im[k1]);
      }
      wave_lds_sync();
      {
        const float4 v0 = *rq0, v1 = *rq1, v2 = *rq2, v3 = *rq3;
        x[0].y = v0.x; x[1].y = v0.y; x[2].y = v0.z; x[3].y = v0.w;
        x[4].y = v1.x; x[5].y = v1.y; x[6].y = v1.z; x[7].y = v1.w;
        x[8].y = v2.x; x[9].y = v2.y; x[10].y = v2.z; x[11].y = v2.w;
        x[12].y = v3.x; x[13].y = v3.y; x[14].y = v3.z; x[15].y = v3.w;
      }
      wave_lds_sync();
#undef MM_S16_WR
    }
    MM_STAMP_AT(10)
    f16::dft16(x);
    MM_STAMP_AT(3)
    {
      float2 pb[9];
      f16::fetch_partners<1>(x, pb, lane, q);
      float* pr = P + (4 * wave + row) * MM_S16_PITCH(XA);
      // every lane of the frame has finished reading the exchange area (in-order LDS, one wave)
      // before any of its power values is written over it
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
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pr[q + 16 * j] = pw[2 * j];
        pr[256 - q - 16 * j] = pw[2 * j + 1];
      }
      if (q == 0) {
        pr[128] = pw[16];
        pr[257] = 0.0f; pr[258] = 0.0f; pr[259] = 0.0f;   // pad bins: the exchange of the next frame ran over them
      }
    }
    }
    MM_STAMP_AT(4)
    // The DCT waves turn the previous tile's log-mel rows into MFCC rows: with two log-mel tiles at the top of phase B
    // (their LDS round trips then overlap the other waves' walks instead of sitting alone in front of the barrier); with
    // ONE tile (lt_single) before the barrier that opens phase B -- phase B overwrites the rows.  One call site.
    if (!lt_single) {
      wg_barrier_lds();
      MM_STAMP_AT(6)
      // every wave is past its phase-A reads of S: the next tile's samples go in
      stage_store(more ? ntl : tl);
    }
    if (MODE != 0 && role < 4 && has_prev) dct_tile(Lt + (((tile & 1) ^ 1) * p.lt_b2) * 80, pb, pt0);
    if (lt_single) {
      wg_barrier_lds();
      stage_store(more ? ntl : tl);
    }
    MM_STAMP_AT(5)
    // ---------------- phase B ----------------
    float held = 0.0f;          // SH: the falling half of filter m0, from the walk to the finishing step
    if (MODE == 0) {
      tile512_store_power_tile(p.out_power, P, MM_S16_PITCH(XA), b, t0, p.n_frames, wave, 16, lane);
    } else {
      const bool valid = (t0 + lane) < p.n_frames;
      float* o = p.out_logmel + ((int64_t)b * p.n_mels + m0) * p.n_frames + t0 + lane;
      const float* pl = P + lane * MM_S16_PITCH(XA);
      const float4* hdr = reinterpret_cast<const float4*>(smem + MM_S16_TAB_OFF(NR, XA));
      const float4* grp = hdr + p.n_runs;
      float carry = 0.0f;
      if (run0 < run1) {
        float4 h = hdr[run0];
        for (int r = run0; r < run1; ++r) {
          const int k4e = __builtin_amdgcn_readfirstlane(__float_as_int(h.x));
          const int k4 = k4e & 0xFFFF;
          const bool empty_d = (k4e >> 16) & 1;     // skip_empty tables only: filter dd has no weights
          const int ng = __builtin_amdgcn_readfirstlane(__float_as_int(h.y));
          const int go = __builtin_amdgcn_readfirstlane(__float_as_int(h.z));
          const int dd = __builtin_amdgcn_readfirstlane(__float_as_int(h.w));
          if (r + 1 < run1) h = hdr[r + 1];
          const float4* pp = reinterpret_cast<const float4*>(pl + k4);
          // the weights sit at wave-uniform addresses beyond the 64 KB an LDS instruction's offset field reaches; read
          // through an opaque VGPR pointer they cost one address add per loop iteration instead of a v_mov per read
          const MM_LDS mm_v4f* gw = (const MM_LDS mm_v4f*)(grp + 2 * go);
          asm volatile("" : "+v"(gw));
          float sa = 0.0f, sb = 0.0f;
          MM_STAMP_AT(12)
#pragma unroll 2
          for (int g = 0; g < ng; ++g) {
            const float4 pv = pp[g];
            const mm_v4f wa = gw[2 * g], wb = gw[2 * g + 1];   // (wlo, whi) of bins 0,1 | 2,3
            sa = fmaf(wa.x, pv.x, sa); sb = fmaf(wa.y, pv.x, sb);
            sa = fmaf(wa.z, pv.y, sa); sb = fmaf(wa.w, pv.y, sb);
            sa = fmaf(wb.x, pv.z, sa); sb = fmaf(wb.y, pv.z, sb);
            sa = fmaf(wb.z, pv.w, sa); sb = fmaf(wb.w, pv.w, sb);
          }
          MM_STAMP_AT(13)
          // what this run contributes to the clip's extremes: a quiet NaN (which loses in v_max / v_min) unless it emits
          // a live filter -- frames behind the clip's end (its last tile) and filters without weights stay out.  The two
          // updates sit on the common path: in one arm of the branch they cost a register copy on every edge.
          float dbm = __builtin_nanf("");
          if (SH && (m1f & MM_RUNS_CONSUMER) && r == run0) {      // (wave-uniform) filter m0: finished behind the barrier
            held = sa;
            o += p.n_frames;
          } else if (dd >= m0) {
            if (!empty_d) {                  // (an empty filter is neither computed nor stored: MM_S16F_SKIP)
              const float v = carry + sa;
              const float db = 3.0102999566398120f * __builtin_amdgcn_logf(mm_max_raw_s(v, p.amin)) - p.db_offset;
              if (valid && p.out_logmel) *o = db;
              dbm = valid ? db : dbm;
              if (fused) Lt[((tile & 1) * p.lt_b2 + dd) * 80 + lane] = db;      // (lt_b2 = 0: one buffer)
            }
            o += p.n_frames;
          }
          mm_max_acc(vmax, dbm);
          mm_min_acc(vmin, dbm);
          carry = sb;
          MM_STAMP_AT(14)
        }
        // the hand-over: row m_end of this tile's buffer, which nobody reads before its owner has finished the filter
        if (SH && (m1f & MM_RUNS_PRODUCER)) Lt[((tile & 1) * p.lt_b2 + (m1f & 0xFFFF)) * 80 + lane] = carry;
      }
      const bool clip_done = (tile + 1 == tile_end) || (ntl == 0);
      if (clip_done && !SH) {   // wave-uniform
        vmax = wave_max(vmax);
        if (p.key_nmin || clip_mode) vmin = wave_min(vmin);
        if (clip_mode) {
          if (lane == 0)
            reinterpret_cast<float2*>(smem + p.red_off)[(b - tile_begin / tpc) * 16 + wave] = make_float2(vmax, vmin);
        } else if (lane == 0 && vmax > -INFINITY) {
          atomicMax(p.clip_key + b, float_key(vmax));
          if (p.key_nmin) atomicMax(p.key_nmin + b, float_key(-vmin));
        }
        vmax = -INFINITY; vmin = INFINITY;
      }
    }
    MM_STAMP_AT(7)
    wg_barrier_lds();
    MM_STAMP_AT(8)
    if constexpr (SH) {
      // The finishing step of filter m0 of the tile just walked: the part before this one has left the filter's rising
      // half in its row of that tile's buffer.  Nothing of phase A is live here, and the DCT waves read the row behind the
      // next mid-tile barrier (behind the barrier after the loop for the launch's last tile).
      // (raised priority: a short dependent chain, which would otherwise queue behind the older waves' phase A)
      const bool valid = (t0 + lane) < p.n_frames;
      __builtin_amdgcn_s_setprio(MM_S16_SH_PRIO);
      if (m1f & MM_RUNS_CONSUMER) {      // (wave-uniform)
        float* lr = Lt + ((tile & 1) * p.lt_b2 + m0) * 80 + lane;
        const float v = *lr + held;
        const float db = 3.0102999566398120f * __builtin_amdgcn_logf(mm_max_raw_s(v, p.amin)) - p.db_offset;
        if (valid && p.out_logmel) p.out_logmel[((int64_t)b * p.n_mels + m0) * p.n_frames + t0 + lane] = db;
        *lr = db;
        const float dbm = valid ? db : __builtin_nanf("");
        mm_max_acc(vmax, dbm);
        mm_min_acc(vmin, dbm);
      }
      // the clip's extremes, now that its last tile's boundary filters are in (the walk's own block, above, otherwise)
      if ((tile + 1 == tile_end) || (ntl == 0)) {   // wave-uniform
        vmax = wave_max(vmax);
        if (p.key_nmin || clip_mode) vmin = wave_min(vmin);
        if (clip_mode) {
          if (lane == 0)
            reinterpret_cast<float2*>(smem + p.red_off)[(b - tile_begin / tpc) * 16 + wave] = make_float2(vmax, vmin);
        } else if (lane == 0 && vmax > -INFINITY) {
          atomicMax(p.clip_key + b, float_key(vmax));
          if (p.key_nmin) atomicMax(p.key_nmin + b, float_key(-vmin));
        }
        vmax = -INFINITY; vmin = INFINITY;
      }
      __builtin_amdgcn_s_setprio(0);
    }
    pb = b; pt0 = t0; has_prev = true;
    b = nb; tl = ntl;
  }
  // the last tile's log-mel values are complete behind the loop's final barrier (SH: behind its finishing step)
  if (SH) wg_barrier_lds();
  if (role < 4 && has_prev) dct_tile(Lt + (((tile_end - 1) & 1) * p.lt_b2) * 80, pb, pt0);
  if (clip_mode && has_prev) {           // the tail of this workgroup's clips (s16_finalize_all)
    S16Fin f;
    f.logmel = p.out_logmel; f.mfcc = p.out_mfcc; f.mod = p.out_mod; f.tw = p.tw; f.dct_t = p.dct_t;
    f.n_frames = (int)p.n_frames; f.n_mels = p.n_mels; f.n_mfcc = p.n_mfcc; f.dct_kp = p.dct_kp; f.n_mod = p.n_mod;
    f.top_db = p.top_db;
    f.dct_e = (p.dct_flags & MM_S16F_SKIP) ? p.dct_a + p.dct_kb * p.dct_nk * 64 : nullptr;
    f.L0 = mm_empty_level(p.amin, p.db_offset);
    s16_finalize_all(f, tile_begin / tpc, (tile_end - tile_begin) / tpc, p.red_off,
                     (int)((p.batch + gridDim.x - 1) / gridDim.x));
  }
  MM_STAMP_END(16)
}

// ---- host side: the instantiations, listed once.  MODE 0/1/2 x NR 3/4 x PRE x ODD x UNAL x XA = 96; NR 1/2 -- short
// hops, e.g. the reference's own 10 kHz default with hop 50: 14.6 KB of samples per tile instead of 48 KB of LDS --
// without PRE or XA (plans with pre-emphasis never ask for NR 1 / 2: setup_tile512): 24.  SH (shared mel runs): MODE 1 / 2
// x NR 3 / 4 with XA, without PRE / ODD / UNAL: 4 -- the regular calls of the long-hop plans (BASELINE configs[1] / [2]);
// every other call walks the overlapping runs (s16_has_shared tells the launcher which table to pass).
// key = sh << 8 | mode << 6 | (nr - 1) << 4 | xa << 3 | pre << 2 | odd << 1 | unal; a key without an instantiation holds nullptr ----
using S16Kernel = void (*)(Logmel512Params);
#define MM_S16_KEYS 448
template <int KEY>
static constexpr S16Kernel s16_entry() {
  constexpr int MODE = (KEY >> 6) & 3, NR = ((KEY >> 4) & 3) + 1;
  constexpr bool XA = (KEY & 8) != 0, PRE = (KEY & 4) != 0, ODD = (KEY & 2) != 0, UNAL = (KEY & 1) != 0, SH = (KEY & 256) != 0;
  if constexpr (MODE == 3 || (NR < 3 && (XA || PRE))) return nullptr;
  else if constexpr (SH && (MODE == 0 || NR < 3 || !XA || PRE || ODD || UNAL)) return nullptr;
  else return logmel512s_kernel<MODE, NR, PRE, ODD, UNAL, XA, SH>;
}
template <int... KEY>
static S16Kernel s16_lookup(int key, std::integer_sequence<int, KEY...>) {
  static constexpr S16Kernel table[] = {s16_entry<KEY>()...};
  return table[key];
}
static S16Kernel s16_kernel(int key) { return s16_lookup(key, std::make_integer_sequence<int, MM_S16_KEYS>()); }

static int s16_key(int mode, int nr, bool xa, bool pre, bool odd, bool unal, bool sh) {
  nr = nr >= 1 && nr <= 3 ? nr : 4;
  if (nr < 3) { xa = false; pre = false; }
  return (sh ? 256 : 0) | mode << 6 | (nr - 1) << 4 | (xa ? 8 : 0) | (pre ? 4 : 0) | (odd ? 2 : 0) | (unal ? 1 : 0);
}

bool s16_has_shared(int nr, bool xa, bool pre, bool odd, bool unal) {
  return s16_kernel(s16_key(1, nr, xa, pre, odd, unal, true)) != nullptr;
}

void launch_s16(int mode, int nr, bool xa, bool pre, bool odd, bool unal, bool sh, dim3 grid, size_t lds, hipStream_t st,
                const Logmel512Params& q) {
  if (mode == 1 && q.out_mod != nullptr) mode = 2;        // clip mode (fused tail); 2 may also be asked for directly (n_mod 0)
  mode = mode == 0 || mode == 1 ? mode : 2;
  hipLaunchKernelGGL(s16_kernel(s16_key(mode, nr, xa, pre, odd, unal, sh)), grid, dim3(1024), lds, st, q);
}

bool set_s16_attr(int bytes) {
  for (int key = 0; key < MM_S16_KEYS; ++key)
    if (s16_kernel(key) &&
        hipFuncSetAttribute((const void*)s16_kernel(key), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
      return false;
  return true;
}
