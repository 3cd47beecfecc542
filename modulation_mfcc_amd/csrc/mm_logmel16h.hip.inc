#pragma once
// logmel512h_kernel: the structural experiment VERDICT r2 #4 asked for -- the staged-sample n_fft = 512 kernel
// (mm_logmel16s.hip.inc) on 32-FRAME tiles with 8-wave workgroups, TWO workgroups per CU.  Included by mm_api.hip.
//
// Why: in the 16-wave kernel all four waves of a SIMD sit in the same phase between two workgroup barriers (phase A:
// the transforms, VALU-bound with LDS round trips; phase B: the mel walk, LDS-bound with little VALU), and the SIMD
// retires one VALU instruction per 4.4 cycles -- the rate ONE wave reaches alone.  Two independent workgroups per CU
// drift apart: one can walk its mel table while the other transforms, and a barrier of one is filled by the other.
// Round 1 tried 32-frame tiles with half-empty mel lanes (lane <-> frame leaves 32 of 64 lanes idle in phase B) and
// lost.  Here a wave walks TWO parts of the run table at once: lanes 0-31 (frames 0-31, part 2w) and lanes 32-63
// (frames 0-31 again, part 2w + 1) -- the per-run overhead (header decode, log, store) is paid once per PAIR of runs,
// the group loop runs to the longer of the two (the shorter one's weight list is zero-padded by the host, its window
// shifted so that it stays inside the power row).  Per CU and 64 frames the instruction count equals the 16-wave
// kernel's; what changes is that the two halves of the CU are no longer phase-locked.
//
// Opt-in (mm_plan_set_variant(plan, 7)): log-mel rows + clip keys only (the DCT runs as the separate kernel), plain
// aligned rows, even hop <= 181, no pre-emphasis.  LDS per workgroup: P 32 x 260 x 4 = 33,280 | S 3 x 8,192 | lane
// records 5,376 | pair table -> two workgroups per CU.
#define MM_H16_P_FLOATS (32 * MM_LM_PITCH)
#define MM_H16_S_OFF (MM_H16_P_FLOATS * 4)
#define MM_H16_NR 3
#define MM_H16_LT_OFF (MM_H16_S_OFF + MM_H16_NR * 8192)
#define MM_H16_TAB_OFF (MM_H16_LT_OFF + 16 * MM_W16_LT_PITCH * 4)

struct Logmel512hParams {
  const float* audio;
  int64_t batch, n_samples, stride, n_frames, tiles_per_clip, n_tiles;
  int hop, n_mels;
  float amin, db_offset;
  const float* lane_tab;      // [16][84]
  const float4* pair_tab;     // pair headers [n_pairs][2] (int bits) followed by groups [..][4]
  int n_pairs, n_tab16;
  const int* wave_part;       // [8][4] = {pair_begin, pair_end, m0 of half 0, m0 of half 1}
  float* out_logmel;          // [B][n_mels][T]
  int* clip_key;              // [B]
  int* key_nmin;              // [B] or nullptr
};

__global__ __launch_bounds__(512, 4) void logmel512h_kernel(Logmel512hParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = reinterpret_cast<float*>(smem);
  float* S = reinterpret_cast<float*>(smem + MM_H16_S_OFF);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 15, row = lane >> 4;
  const float* lt = reinterpret_cast<const float*>(smem + MM_H16_LT_OFF) + q * MM_W16_LT_PITCH;

  for (int i = threadIdx.x; i < 16 * MM_W16_LT_PITCH; i += 512)
    reinterpret_cast<float*>(smem + MM_H16_LT_OFF)[i] = p.lane_tab[i];
  if (threadIdx.x < 32 * 3) P[(threadIdx.x / 3) * MM_LM_PITCH + 257 + threadIdx.x % 3] = 0.0f;
  for (int i = threadIdx.x; i < p.n_tab16; i += 512)
    reinterpret_cast<float4*>(smem + MM_H16_TAB_OFF)[i] = p.pair_tab[i];
  const int pr0 = p.wave_part[wave * 4 + 0], pr1 = p.wave_part[wave * 4 + 1];
  const int m0A = p.wave_part[wave * 4 + 2], m0B = p.wave_part[wave * 4 + 3];

  const int tpc = (int)p.tiles_per_clip;
  const int tile_begin = (int)((int64_t)blockIdx.x * p.n_tiles / gridDim.x);
  const int tile_end = (int)((int64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x);
  const int n = (int)p.n_samples;
  float vmax = -INFINITY, vmin = INFINITY;
  int b = tile_begin / tpc, tl = tile_begin - b * tpc;
  int nb = b, ntl = tl;

  const Tile512ExSwz ex(P + 4 * wave * MM_LM_PITCH, row, q);   // exchange area = this wave's own four power rows
  const float2* sx = reinterpret_cast<const float2*>(S + (4 * wave + row) * p.hop + 2 * q);

  float4 sreg[MM_H16_NR];
  auto stage_load = [&](int bb, int ttl) {
    const float* a = p.audio + (int64_t)bb * p.stride;
    const int first = ttl * 32 * p.hop - 256 + 4 * (int)threadIdx.x;
    int off[MM_H16_NR];
#pragma unroll
    for (int j = 0; j < MM_H16_NR; ++j) off[j] = min(max(first + 2048 * j, 0), n - 4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < MM_H16_NR; ++j) sreg[j] = *reinterpret_cast<const float4*>(a + off[j]);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_store = [&](int ttl) {
    const int first = ttl * 32 * p.hop - 256 + 4 * (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < MM_H16_NR; ++j) {
      const int s0 = first + 2048 * j;
      // (n % 4 == 0: groups never straddle a clip edge)
      reinterpret_cast<float4*>(S)[threadIdx.x + 512 * j] = tile512_stage_fix<false, false>(sreg[j], s0, n, 0.0f, 0.0f);
    }
  };
  if (tile_begin < tile_end) {
    stage_load(b, tl);
    stage_store(tl);
  }
  __syncthreads();
  float2 wp[8];                               // split twiddles: registers for the whole launch
  tile512_read_wp(wp, lt);
  const int fr = lane & 31, hh = lane >> 5;   // phase B: frame within the tile, half (part 2w / 2w + 1)
  const int m0h = hh ? m0B : m0A;

  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int t0 = tl * 32;
    if (++ntl == tpc) { ntl = 0; ++nb; }
    const bool more = tile + 1 < tile_end;
    stage_load(more ? nb : b, more ? ntl : tl);
    // ---------------- phase A: one item (4 frames) per wave ----------------
    if (t0 + 4 * wave < (int)p.n_frames) {
      float2 x[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) x[n1] = sx[16 * n1];
      tile512_window(x, lt);
      f16::dft16(x);
      tile512_twiddle(x, lt + MM_LT_TW);
      tile512_exchange(x, ex);
      f16::dft16(x);
      {
        float2 pb[9];
        f16::fetch_partners<1>(x, pb, lane, q);
        float pw[17];
        tile512_split_power(x, pb, wp, pw);
        tile512_store_power_row<true>(P + (4 * wave + row) * MM_LM_PITCH, q, pw);
      }
    }
    wg_barrier_lds();
    stage_store(more ? ntl : tl);
    // ---------------- phase B: two parts of the run table per wave, one per 32-lane half ----------------
    {
      const bool valid = (t0 + fr) < p.n_frames;
      float* obase = p.out_logmel + (int64_t)b * p.n_mels * p.n_frames + t0 + fr;
      const float* pl = P + fr * MM_LM_PITCH;
      const float4* hdr = reinterpret_cast<const float4*>(smem + MM_H16_TAB_OFF);
      const float4* grp = hdr + 2 * p.n_pairs;
      float carry = 0.0f;
      if (pr0 < pr1) {
        float4 h0 = hdr[2 * pr0], h1 = hdr[2 * pr0 + 1];
        for (int r = pr0; r < pr1; ++r) {
          const int k4 = __float_as_int(hh ? h0.y : h0.x);
          const int ng = __builtin_amdgcn_readfirstlane(__float_as_int(h0.z));
          const int go = __builtin_amdgcn_readfirstlane(__float_as_int(h0.w));
          const int dd = __float_as_int(hh ? h1.y : h1.x);
          if (r + 1 < pr1) { h0 = hdr[2 * r + 2]; h1 = hdr[2 * r + 3]; }
          const float4* pp = reinterpret_cast<const float4*>(pl + k4);
          const float4* gw = grp + 4 * go + 2 * hh;
          float sa = 0.0f, sb = 0.0f;
          tile512_group_dot<4>(pp, gw, ng, sa, sb);
          if (dd >= m0h) {
            const float db = tile512_db(fmaxf(p.amin, carry + sa), p.db_offset);
            if (valid) {
              obase[(int64_t)dd * p.n_frames] = db;
              vmax = fmaxf(vmax, db);
              vmin = fminf(vmin, db);
            }
          }
          carry = sb;
        }
      }
      const bool clip_done = (tile + 1 == tile_end) || (ntl == 0);
      if (clip_done) {   // wave-uniform
        vmax = wave_max(vmax);
        if (p.key_nmin) vmin = wave_min(vmin);
        if (lane == 0 && vmax > -INFINITY) {
          atomicMax(p.clip_key + b, float_key(vmax));
          if (p.key_nmin) atomicMax(p.key_nmin + b, float_key(-vmin));
        }
        vmax = -INFINITY; vmin = INFINITY;
      }
    }
    wg_barrier_lds();
    b = nb; tl = ntl;
  }
}

// ---- host side: the pair table from the 16-part run table ---------------------------------------------------
struct H16Tables {
  std::vector<float> tab;      // pair headers [n_pairs][8] (int bits) | groups [n_groups][16]
  std::vector<int> part;       // [8][4]
  int n_pairs = 0;
};

// r16: run table of 16 parts (mm::build_mel_runs, groups as {wlo x4, whi x4}).  Wave w walks parts 2w (lanes 0-31)
// and 2w + 1 (lanes 32-63) in lockstep: pair r = (run r of part 2w, run r of part 2w + 1); the shorter run's groups
// are zero-padded to the longer one's count and its window start moved down so that it ends inside the 260-float
// power row; a part with fewer runs gets empty runs (dd far below every m0: never stored).
static void build_h16_tables(const mm::MelRuns& r16, H16Tables* out) {
  std::vector<int> hdr;
  std::vector<float> grp;
  out->part.assign(32, 0);
  std::vector<double> cost(8, 0.0);
  std::vector<int> pbeg(8), pend(8);
  for (int w = 0; w < 8; ++w) {
    const int a0 = r16.part[(2 * w) * 4 + 0], a1 = r16.part[(2 * w) * 4 + 1];
    const int b0 = r16.part[(2 * w + 1) * 4 + 0], b1 = r16.part[(2 * w + 1) * 4 + 1];
    const int n_pr = std::max(a1 - a0, b1 - b0);
    pbeg[w] = (int)(hdr.size() / 8);
    for (int r = 0; r < n_pr; ++r) {
      const int ra = r < a1 - a0 ? a0 + r : -1, rb = r < b1 - b0 ? b0 + r : -1;
      const int nga = ra >= 0 ? r16.hdr[4 * ra + 1] : 0, ngb = rb >= 0 ? r16.hdr[4 * rb + 1] : 0;
      const int ng = std::max(nga, ngb);
      const int go = (int)(grp.size() / 16);
      int k4[2], dd[2];
      std::vector<float> g16((size_t)ng * 16, 0.0f);
      for (int h = 0; h < 2; ++h) {
        const int rr = h ? rb : ra, ngh = h ? ngb : nga;
        k4[h] = 0; dd[h] = -(1 << 20);
        if (rr < 0) continue;
        const int k = r16.hdr[4 * rr + 0], gsrc = r16.hdr[4 * rr + 2];
        dd[h] = r16.hdr[4 * rr + 3];
        const int kk = std::min(k, 260 - 4 * ng);            // the window [kk, kk + 4 ng) stays inside the row
        const int shift = (k - kk) / 4;
        k4[h] = kk;
        for (int g = 0; g < ngh; ++g) {
          const float* src = &r16.grp[(size_t)(gsrc + g) * 8];   // {wlo x4, whi x4}
          float* dst = &g16[(size_t)(g + shift) * 16 + 8 * h];
          const float t[8] = {src[0], src[4], src[1], src[5], src[2], src[6], src[3], src[7]};   // (wlo_i, whi_i) pairs
          std::memcpy(dst, t, sizeof t);
        }
      }
      hdr.push_back(k4[0]); hdr.push_back(k4[1]); hdr.push_back(ng); hdr.push_back(go);
      hdr.push_back(dd[0]); hdr.push_back(dd[1]); hdr.push_back(0); hdr.push_back(0);
      grp.insert(grp.end(), g16.begin(), g16.end());
      cost[w] += 58.0 + 8.5 * ng;
    }
    pend[w] = (int)(hdr.size() / 8);
  }
  // wave v sits on SIMD v % 4: heaviest pair-part first onto the least loaded SIMD (two waves per SIMD)
  std::vector<int> order(8);
  for (int i = 0; i < 8; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b] || (cost[a] == cost[b] && a < b); });
  double load[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (int i = 0; i < 8; ++i) {
    const int w = order[i];
    int best = -1;
    for (int sd = 0; sd < 4; ++sd)
      if (cnt[sd] < 2 && (best < 0 || load[sd] < load[best])) best = sd;
    const int wave = best + 4 * cnt[best];
    out->part[wave * 4 + 0] = pbeg[w]; out->part[wave * 4 + 1] = pend[w];
    out->part[wave * 4 + 2] = r16.part[(2 * w) * 4 + 2]; out->part[wave * 4 + 3] = r16.part[(2 * w + 1) * 4 + 2];
    load[best] += cost[w]; ++cnt[best];
  }
  out->n_pairs = (int)(hdr.size() / 8);
  out->tab.resize(hdr.size() + grp.size());
  std::memcpy(out->tab.data(), hdr.data(), hdr.size() * 4);
  std::memcpy(out->tab.data() + hdr.size(), grp.data(), grp.size() * 4);
}
