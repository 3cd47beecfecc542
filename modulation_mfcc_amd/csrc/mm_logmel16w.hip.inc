#pragma once
// logmel512w_kernel: the 16-wave variant of the fused n_fft = 512 kernel (mm_fft16.hip.inc has the
// 8-wave one).  Same arithmetic, different occupancy trade:
//
//   * 1024 threads = 16 waves = 4 waves per SIMD (<= 128 VGPRs): LDS / bpermute / global latency is
//     hidden by the other three waves of the SIMD instead of by a second register set;
//   * every wave transforms ONE item (4 frames) per 64-frame tile; the next tile's samples are
//     loaded into the (dead) x registers right after the power rows are written, so the mel phase
//     and its two barriers are the prefetch distance;
//   * per-lane constants (window, stage-1 twiddles, split twiddles) live in one LDS record per
//     lane q (pitch 84 floats -> conflict-free ds_read_b128), not in registers;
//   * the 16x16 transpose between the two DFT-16 stages is done in two halves (re, then im)
//     through a 5 KB wave-private buffer: 16 x ds_write_b32 + 4 x ds_read_b128 per half
//     (row pitch 20 floats: b128 reads conflict-free, b32 writes 2-way = free).
//
// LDS: P 64x260x4 = 66,560 | exchange 16 x 5,120 = 81,920 | lane records 5,376 | mel run table.
#define MM_W16_EX_FLOATS (4 * 320)
#define MM_W16_EX_OFF (MM_LM_P_FLOATS * 4)
#define MM_W16_LT_OFF (MM_W16_EX_OFF + 16 * MM_W16_EX_FLOATS * 4)
#define MM_W16_LT_PITCH 84
#define MM_W16_TAB_OFF (MM_W16_LT_OFF + 16 * MM_W16_LT_PITCH * 4)


template <int MODE>
__global__ __launch_bounds__(1024) void logmel512w_kernel(Logmel512Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* exf = reinterpret_cast<float*>(smem + MM_W16_EX_OFF) + wave * MM_W16_EX_FLOATS;
  const int q = lane & 15, row = lane >> 4;
  const float* lt = reinterpret_cast<const float*>(smem + MM_W16_LT_OFF) + q * MM_W16_LT_PITCH;
  const Tile512ExP20 ex(exf, row, q);

  for (int i = threadIdx.x; i < 16 * MM_W16_LT_PITCH; i += 1024)
    reinterpret_cast<float*>(smem + MM_W16_LT_OFF)[i] = p.lane_tab[i];
  for (int i = threadIdx.x; i < p.n_tab16; i += 1024)
    reinterpret_cast<float4*>(smem + MM_W16_TAB_OFF)[i] = p.mel_tab[i];
  if (threadIdx.x < 64 * 3) P[(threadIdx.x / 3) * MM_LM_PITCH + 257 + threadIdx.x % 3] = 0.0f;

  const int run0 = p.wave_part[wave * 4 + 0], run1 = p.wave_part[wave * 4 + 1];
  const int m0 = p.wave_part[wave * 4 + 2];

  // contiguous tile range per workgroup: the per-clip maximum is then reduced and published once
  // per clip (every tiles_per_clip tiles) instead of once per tile
  const int tile_begin = (int)((int64_t)blockIdx.x * p.n_tiles / gridDim.x);
  const int tile_end = (int)((int64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x);
  const int tpc = (int)p.tiles_per_clip;
  float vmax = -INFINITY;
  // (b, tl) = clip and tile-within-clip of the current tile, (nb, ntl) of the next one: stepped
  // incrementally (a 64-bit tile / tiles_per_clip is ~140 scalar instructions per wave per tile)
  int b = tile_begin / tpc, tl = tile_begin - b * tpc;
  int nb = b, ntl = tl;

  float2 x[16];
  LmItem item = lm_item_bt(p, tile_begin < tile_end, b, tl, 0, wave);
  lm_prefetch(x, p, item, row, q);
  __syncthreads();

  MM_STAMP_BEGIN(11)
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int t0 = tl * 64;
    MM_STAMP_AT(9)
    if (++ntl == tpc) { ntl = 0; ++nb; }
    // ---------------- phase A: one item per wave ----------------
    if (!item.interior) lm_mask_edge(x, p, item, row, q);
    tile512_window(x, lt);
    MM_STAMP_AT(0)
    f16::dft16(x);
    MM_STAMP_AT(1)
    tile512_twiddle(x, lt + MM_LT_TW);
    MM_STAMP_AT(2)
    tile512_exchange(x, ex);
    MM_STAMP_AT(10)
    f16::dft16(x);
    MM_STAMP_AT(3)
    {
      float2 pb[9], wp[8];
      f16::fetch_partners<1>(x, pb, lane, q);
      tile512_read_wp(wp, lt);
      float pw[17];
      tile512_split_power(x, pb, wp, pw);
      tile512_store_power_row<false>(P + (4 * wave + row) * MM_LM_PITCH, q, pw);
    }
    MM_STAMP_AT(4)
    // next tile's samples: in flight during the mel phase
    item = lm_item_bt(p, tile + 1 < tile_end, nb, ntl, 0, wave);
    lm_prefetch(x, p, item, row, q);
    MM_STAMP_AT(5)
    wg_barrier_lds();
    MM_STAMP_AT(6)
    // ---------------- phase B ----------------
    if (MODE == 0) {
      tile512_store_power_tile(p.out_power, P, MM_LM_PITCH, b, t0, p.n_frames, wave, 16, lane);
    } else {
      const bool valid = (t0 + lane) < p.n_frames;
      // filters are emitted in increasing order starting at m0: a running row pointer
      float* o = p.out_logmel + ((int64_t)b * p.n_mels + m0) * p.n_frames + t0 + lane;
      const float* pl = P + lane * MM_LM_PITCH;
      const float4* hdr = reinterpret_cast<const float4*>(smem + MM_W16_TAB_OFF);
      const float4* grp = hdr + p.n_runs;
      float carry = 0.0f;
      if (run0 < run1) {
        float4 h = hdr[run0];
        for (int r = run0; r < run1; ++r) {
          const Tile512Run rh = tile512_run_header(h);
          if (r + 1 < run1) h = hdr[r + 1];
          float sa = 0.0f, sb = 0.0f;
          tile512_group_dot<2>(reinterpret_cast<const float4*>(pl + rh.k4), grp + 2 * rh.go, rh.ng, sa, sb);
          if (rh.dd >= m0) {
            const float db = tile512_db(fmaxf(p.amin, carry + sa), p.db_offset);
            if (valid) {
              *o = db;
              vmax = fmaxf(vmax, db);
            }
            o += p.n_frames;
          }
          carry = sb;
        }
      }
      const bool clip_done = (tile + 1 == tile_end) || (ntl == 0);
      if (clip_done) {   // wave-uniform
        vmax = wave_max(vmax);
        if (lane == 0 && vmax > -INFINITY) atomicMax(p.clip_key + b, float_key(vmax));
        vmax = -INFINITY;
      }
    }
    MM_STAMP_AT(7)
    wg_barrier_lds();
    MM_STAMP_AT(8)
    b = nb; tl = ntl;
  }
  MM_STAMP_END(11)
}
