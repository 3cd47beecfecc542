#pragma once
// logmel12m_kernel<NR, PRE, ODD, UNAL>: the fused n_fft = 512 kernel with the mel contraction (and, for
// n_mfcc <= 16, the DCT-II) on the MATRIX pipe.  gfx950 only.
//
// Why (profiles/r01c_sq_counters.md, VERDICT r1): the lane<->frame mel walk of logmel512s_kernel is
// 0.12 of its 0.42 ms, a third of its ds_read_b128 and pure VALU issue, sitting between two workgroup
// barriers -- and VALU issue is what bounds the transforms.  v_mfma_f32_16x16x4_f32 is exact f32 (a
// k-ordered fmaf chain) at the VALU's FLOP rate on a pipe the FFT does not use, and the Slaney mel
// matrix is banded: a block of 16 filters touches one contiguous bin range, so
// D[16 filters x 16 frames] += W[16 x 4 bins] * P[4 bins x 16 frames] over that range costs ~70 MFMAs per
// 16 frames (40 mel) instead of ~300 dense.  Run as a phase of its own that is 2.6 k matrix-pipe cycles
// per 64 frames against the walk's 4.1 k: the gain comes from running it UNDER the transforms.
//
// Geometry: 1024 threads = 16 waves.  Waves 0..11 transform (one item = 4 frames each: tile = 48 frames = 3
// MFMA column blocks of 16 frames), waves 12..15 -- one per SIMD -- do nothing but the mel units of the
// PREVIOUS tile: the power tile P is DOUBLE BUFFERED (2 x 48 x 260 floats), the transforms of tile i
// write P[i & 1] while the mel waves read P[(i - 1) & 1].  (A first version had 12 waves that each ran
// a share of the mel units between the stages of their transform: the units cannot be balanced over
// 12 waves -- 32 / 26 / 12 MFMAs -- and with one barrier pair per tile every wave waits for the
// slowest; 0.54 ms.  tools/stamps_m12.py.)
//
//   barrier A   P[prev] complete, samples S(i) staged
//   waves 0-11  read their 16 complex points of tile i from S
//   barrier B   (all S reads done -> S may be overwritten)
//   all waves   issue the LDS-DMA of tile i+1's samples (2 x 1 KiB per wave)
//   waves 0-11  window, DFT-16, twiddles, 16x16 exchange inside their own rows of P[i & 1], DFT-16, real
//               split, power rows;   waves 12-15: mel units of tile i-1 from P[(i - 1) & 1]
//   all waves   vmcnt(0): their pieces of S(i+1) have landed
//
// Mel unit (f, mb) = frame block f (16 frames) x filter block mb (16 filters): host-built list per mel
// wave (build_m12_tables: balanced by MFMA count, the units of one frame block adjacent).  Per 8-bin
// step one ds_read_b64 of the weights (A operand, lane (i, kc): W[16 mb + i][kb + 8 s + 2 kc + {0,1}])
// and one conflict-free ds_read_b64 of the power rows (B operand, lane (j, kc): P[16 f + j][same bins];
// pitch 260 = 4 mod 64) feed two MFMAs on two accumulators (the 40-cycle dependent latency of one chain
// would otherwise cap the pipe at 80 %).  The accumulator's lane layout D[4 g + r][j] IS the B layout of
// a following MFMA that contracts over the filter index, so 10 log10 max(amin, .) is applied in place
// and the DCT-II of the block is four more MFMAs (A operand: DCT[k][16 mb + 4 g + r]), chained over the
// wave's units of the frame block; the partial MFCC tile goes to an LDS slot and the LAST wave of the
// frame block to arrive (LDS counter; the LDS executes a CU's operations in issue order, so its
// partners' slots are complete) adds the slots in fixed order and stores [b][k][t] -- deterministic, no
// float atomics.
//
// The DCT is taken of the UNCLAMPED log-mel rows: exact whenever no value of the clip lies more than
// top_db under the clip maximum (then max(L, max - top_db) = L everywhere).  The kernel therefore also
// publishes the clip MINIMUM, always stores the log-mel rows, and dct_fixup_kernel recomputes the clamped
// DCT only for the clips with min < max - top_db (none in audio with a noise floor; all of them, at the
// old two-kernel cost, for clips with digital silence).
//
// LDS: P 2 x 49,920 | S 4 x (47 hop + 512) | window 2 KB | stage-1 twiddle records 2.3 KB | A table |
// DCT table 1 KB per filter block | partial slots 1 KB each | counters: 160,016 B at hop 160 / 40 mel.
#define MM_M12_TF 48
#define MM_M12_FW 12            // transform waves
#define MM_M12_THREADS 1024
#define MM_M12_PITCH 260
#define MM_M12_PBUF (MM_M12_TF * MM_M12_PITCH)
#define MM_M12_S_OFF (2 * MM_M12_PBUF * 4)
#define MM_M12_CH 4             // mel steps fetched ahead
#define MM_M12_TW_PITCH 36      // floats per lane record of stage-1 twiddles (9 x 16 B: conflict-free b128)

struct Logmel12mParams {
  const float* audio;
  int64_t batch, n_samples, stride, n_frames, tiles_per_clip, n_tiles;
  int hop, n_mels, n_mfcc, nb;       // nb = filter blocks of 16
  float amin, db_offset, preemph;
  const float* lane_tab;             // [16][84] window | W_256^(q k1) | split twiddles (global; read once)
  const float* window;               // [512] (centred Hann; n_fft < 512 plans: centred in 512)
  const float2* a_tab;               // per filter block: [steps][4][rows] float2 (rows = filters of the block)
  int n_a2;                          // float2 entries
  const float* dct_tab;              // [nb][4][64]
  // the mel units live in the kernel argument segment: a wave-uniform, dynamically indexed read of it is
  // a scalar load (from ordinary global memory the compiler must use vector loads -- the kernel also
  // stores to global memory -- and those queue behind the sample loads in vmcnt order)
  int4 units[MM_M12_MW * MM_M12_UMAX];   // {filter block | rows << 8 | frame block << 16 | slot << 20 | flush << 31,
                                         //  table offset (float2), first bin, steps}
  int n_units[8];                    // [4] units per mel wave, then [3] = first slot | slots << 8 per frame block
  float* out_logmel;                 // [B][n_mels][T] or nullptr
  float* out_mfcc;                   // [B][n_mfcc][T] (unclamped DCT) or nullptr
  int* key_max;                      // [B] order-preserving keys of the clip max (atomicMax)
  int* key_nmin;                     // [B] keys of -(clip min) (atomicMax) or nullptr
  int s_floats;                      // 47 hop + 512 rounded up to 256 (whole 1 KiB LDS-DMA pieces)
  const float* zeros;                // >= 16 zero bytes in global memory: source of the padding groups
  unsigned win_off, tw_off, a_off, dct_off, part_off, cnt_off; // LDS byte offsets
};

// LDS-DMA of 16 bytes per lane: LDS destination = wave-uniform byte address in M0 + 16 * lane, source address
// per lane.  M0 is compiler-reserved: saved and restored inside the statement.  (Inline asm: with the builtin
// hipcc orders every later LDS access behind the DMA with vmcnt(0), i.e. each wave would sit out the HBM
// latency of its own prefetch.)
__device__ __forceinline__ void glds16_asm(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

template <int NR, bool PRE, bool ODD, bool UNAL>
__global__ __launch_bounds__(MM_M12_THREADS) void logmel12m_kernel(Logmel12mParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Pb = reinterpret_cast<float*>(smem);
  float* S = reinterpret_cast<float*>(smem + MM_M12_S_OFF);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // ---- constant tables -> LDS ----
  if (threadIdx.x < 512) reinterpret_cast<float*>(smem + p.win_off)[threadIdx.x] = p.window[threadIdx.x];
  for (int i = threadIdx.x; i < 16 * 32; i += MM_M12_THREADS)       // stage-1 twiddles: floats 32..61 of a lane record
    reinterpret_cast<float*>(smem + p.tw_off)[(i >> 5) * MM_M12_TW_PITCH + (i & 31)] = p.lane_tab[(i >> 5) * MM_W16_LT_PITCH + 32 + (i & 31)];
  for (int i = threadIdx.x; i < p.n_a2; i += MM_M12_THREADS)
    reinterpret_cast<float2*>(smem + p.a_off)[i] = p.a_tab[i];
  for (int i = threadIdx.x; i < p.nb * 256; i += MM_M12_THREADS)
    reinterpret_cast<float*>(smem + p.dct_off)[i] = p.dct_tab[i];
  if (threadIdx.x < 2 * MM_M12_TF * 3) {
    const int r = threadIdx.x / 3;
    Pb[r * MM_M12_PITCH + 257 + threadIdx.x % 3] = 0.0f;
  }
  if (threadIdx.x < 4) reinterpret_cast<int*>(smem + p.cnt_off)[threadIdx.x] = 0;

  const int tile_begin = (int)((int64_t)blockIdx.x * p.n_tiles / gridDim.x);
  const int tile_end = (int)((int64_t)(blockIdx.x + 1) * p.n_tiles / gridDim.x);
  const int tpc = (int)p.tiles_per_clip;
  const int n = (int)p.n_samples;
  int b = tile_begin / tpc, tl = tile_begin - b * tpc;   // tile being transformed
  int nb = b, ntl = tl;                                  // the one after it

  // ---- staging of a tile's samples ----
  // Plain instantiation (16-byte aligned rows, n % 4 == 0, no pre-emphasis): 1 KiB pieces go straight from
  // global memory into S by LDS-DMA (piece = wave + 16 j; the SOURCE address is per lane, so a group outside
  // the clip reads the 16 zero bytes of p.zeros) -- no staging registers, no ds_write pass.  Issued right
  // behind barrier B, drained (vmcnt) before barrier A.  Otherwise: 16-byte loads into registers (group g =
  // tid + 1024 j), written to S before barrier A.
  constexpr bool DMA = !PRE && !UNAL;
  const unsigned s_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + MM_M12_S_OFF;
  auto stage_dma = [&](int bb, int ttl) {
    const float* a = p.audio + (int64_t)bb * p.stride;
    const int first = ttl * MM_M12_TF * p.hop - 256;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int wbase = 256 * (wave + 16 * j);                     // first float of this wave's 1 KiB piece
      const int s0 = first + wbase + 4 * lane;
      const float* src = (s0 >= 0 && s0 < n) ? a + s0 : p.zeros;
      if (wbase < p.s_floats) glds16_asm(src, s_lds + 4u * (unsigned)wbase);
    }
  };
  float4 sreg[DMA ? 1 : NR];
  float sprev[PRE ? NR : 1];
  auto stage_load = [&](int bb, int ttl) {
    const float* a = p.audio + (int64_t)bb * p.stride;
    const int first = ttl * MM_M12_TF * p.hop - 256 + 4 * (int)threadIdx.x;
    int off[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) off[j] = min(max(first + 4 * MM_M12_THREADS * j, 0), n - 4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if (UNAL) {
        const MmFloat4U t = *reinterpret_cast<const MmFloat4U*>(a + off[j]);
        sreg[DMA ? 0 : j] = make_float4(t.x, t.y, t.z, t.w);
      } else {
        sreg[DMA ? 0 : j] = *reinterpret_cast<const float4*>(a + off[j]);
      }
    }
    if (PRE) {
#pragma unroll
      for (int j = 0; j < NR; ++j) sprev[j] = a[min(max(first + 4 * MM_M12_THREADS * j - 1, 0), n - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_store = [&](int ttl) {
    const int first = ttl * MM_M12_TF * p.hop - 256 + 4 * (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int gi = 4 * ((int)threadIdx.x + MM_M12_THREADS * j);
      const int s0 = first + 4 * MM_M12_THREADS * j;
      const float4 v = tile512_stage_fix<PRE, UNAL>(sreg[DMA ? 0 : j], s0, n, sprev[PRE ? j : 0], p.preemph);
      if (gi < p.s_floats) *reinterpret_cast<float4*>(S + gi) = v;
    }
  };

  if (tile_begin < tile_end) {
    if (DMA) {
      stage_dma(b, tl);
    } else {
      stage_load(b, tl);
      stage_store(tl);
    }
  }
  if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMA is invisible to the compiler's counters
  __syncthreads();

  MM_STAMP_BEGIN(12)

  if (wave < MM_M12_FW) {
    // =============================== transform waves ===============================
    const int q = lane & 15, row = lane >> 4;
    float2 wp[8];                                        // split twiddles: registers for the whole launch
    {
      const float4* r4 = reinterpret_cast<const float4*>(p.lane_tab + q * MM_W16_LT_PITCH + 64);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 t = r4[i];
        wp[2 * i] = make_float2(t.x, t.y);
        wp[2 * i + 1] = make_float2(t.z, t.w);
      }
    }
    const float2* wl = reinterpret_cast<const float2*>(smem + p.win_off) + q;   // window pairs w[32 n1 + 2 q + {0, 1}]
    const float4* twl = reinterpret_cast<const float4*>(smem + p.tw_off + q * MM_M12_TW_PITCH * 4);
    const float* sxf = S + (4 * wave + row) * p.hop + 2 * q;
    const float2* sx = reinterpret_cast<const float2*>(sxf);
    for (int it = tile_begin; it <= tile_end; ++it) {
      const bool has_fft = it < tile_end;
      const bool more = it + 1 < tile_end;
      float* Pc = Pb + (it & 1) * MM_M12_PBUF;
      float2 x[16];
      if (has_fft) {
        if (ODD) {
#pragma unroll
          for (int n1 = 0; n1 < 16; ++n1) x[n1] = make_float2(sxf[32 * n1], sxf[32 * n1 + 1]);
        } else {
#pragma unroll
          for (int n1 = 0; n1 < 16; ++n1) x[n1] = sx[16 * n1];
        }
      }
      wg_barrier_lds();                                  // barrier B: every wave holds its samples
      MM_STAMP_AT(0)
      if (has_fft) { if (++ntl == tpc) { ntl = 0; ++nb; } }
      if (more) { if (DMA) stage_dma(nb, ntl); else stage_load(nb, ntl); }
      MM_STAMP_AT(1)
      if (has_fft) {
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) { const float2 w = wl[16 * n1]; x[n1].x *= w.x; x[n1].y *= w.y; }
        f16::dft16(x);
        {
          float2 w[16];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float4 t = twl[i];
            w[2 * i] = make_float2(t.x, t.y);
            w[2 * i + 1] = make_float2(t.z, t.w);
          }
#pragma unroll
          for (int k1 = 1; k1 < 16; ++k1) x[f16::P16(k1)] = f16::cmulf(x[f16::P16(k1)], w[k1 - 1]);
        }
        MM_STAMP_AT(3)
        // 16x16 exchange inside this wave's own four power rows of the CURRENT buffer (see logmel512s_kernel)
        float* exw = Pc + 4 * wave * MM_M12_PITCH + row * 256;
        float* wq0 = exw + (q ^ 0);
        float* wq1 = exw + (q ^ 4);
        float* wq2 = exw + (q ^ 8);
        float* wq3 = exw + (q ^ 12);
        const int sq = (q >> 2) & 3;
        const float4* rq0 = reinterpret_cast<const float4*>(exw + q * 16 + 4 * (0 ^ sq));
        const float4* rq1 = reinterpret_cast<const float4*>(exw + q * 16 + 4 * (1 ^ sq));
        const float4* rq2 = reinterpret_cast<const float4*>(exw + q * 16 + 4 * (2 ^ sq));
        const float4* rq3 = reinterpret_cast<const float4*>(exw + q * 16 + 4 * (3 ^ sq));
#define MM_M12_WR(k1, val)                                                                         \
  (((k1) >> 2) == 0 ? wq0 : ((k1) >> 2) == 1 ? wq1 : ((k1) >> 2) == 2 ? wq2 : wq3)[(k1) * 16] = (val)
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) MM_M12_WR(k1, x[f16::P16(k1)].x);
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
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) MM_M12_WR(k1, im[k1]);
        wave_lds_sync();
        {
          const float4 v0 = *rq0, v1 = *rq1, v2 = *rq2, v3 = *rq3;
          x[0].y = v0.x; x[1].y = v0.y; x[2].y = v0.z; x[3].y = v0.w;
          x[4].y = v1.x; x[5].y = v1.y; x[6].y = v1.z; x[7].y = v1.w;
          x[8].y = v2.x; x[9].y = v2.y; x[10].y = v2.z; x[11].y = v2.w;
          x[12].y = v3.x; x[13].y = v3.y; x[14].y = v3.z; x[15].y = v3.w;
        }
        wave_lds_sync();
#undef MM_M12_WR
        MM_STAMP_AT(5)
        f16::dft16(x);
        float2 pb[9];
        f16::fetch_partners<1>(x, pb, lane, q);
        float* pr = Pc + (4 * wave + row) * MM_M12_PITCH;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          float2 xa, xb;
          f16::split_pair(x[f16::P16(jj)], pb[jj], wp[jj], xa, xb);
          pr[q + 16 * jj] = fmaf(xa.x, xa.x, xa.y * xa.y);
          pr[256 - q - 16 * jj] = fmaf(xb.x, xb.x, xb.y * xb.y);
        }
        if (q == 0) {
          const float2 zm = x[f16::P16(8)];
          pr[128] = fmaf(zm.x, zm.x, zm.y * zm.y);
          pr[257] = 0.0f; pr[258] = 0.0f; pr[259] = 0.0f;   // pad bins: the exchange of the next frame ran over them
        }
      }
      MM_STAMP_AT(7)
      if (more && !DMA) stage_store(ntl);
      if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of S(i+1) have landed
      MM_STAMP_AT(8)
      wg_barrier_lds();                                  // barrier A
      MM_STAMP_AT(9)
      b = nb; tl = ntl;
    }
  } else {
    // ================================== mel waves ==================================
    const int mw = wave - MM_M12_FW;
    const int T = (int)p.n_frames;
    // the mel waves are the youngest wave of their SIMD: without a raised priority the three transform
    // waves take every issue slot (arbitration is by priority, then age) and the mel units only start
    // once the transforms wait at the barrier
    __builtin_amdgcn_s_setprio(3);
    const float2* A = reinterpret_cast<const float2*>(smem + p.a_off);
    const float* Dt = reinterpret_cast<const float*>(smem + p.dct_off);
    float* part = reinterpret_cast<float*>(smem + p.part_off);
    int* cnt = reinterpret_cast<int*>(smem + p.cnt_off);
    const int nu = p.n_units[mw];
    const int4* my_units = p.units + mw * MM_M12_UMAX;   // kernarg segment
    const int j = lane & 15, g = lane >> 4;
    int mb_clip = b, mtl = tl;                           // tile whose mel units run (the previous one)
    float vmax = -INFINITY, vmin = INFINITY;
    for (int it = tile_begin; it <= tile_end; ++it) {
      const bool has_fft = it < tile_end, has_mel = it > tile_begin;
      const bool more = it + 1 < tile_end;
      const float* Pp = Pb + ((it & 1) ^ 1) * MM_M12_PBUF;
      wg_barrier_lds();                                  // barrier B
      MM_STAMP_AT(0)
      if (has_fft) { if (++ntl == tpc) { ntl = 0; ++nb; } }
      if (more) { if (DMA) stage_dma(nb, ntl); else stage_load(nb, ntl); }
      MM_STAMP_AT(1)
      if (has_mel) {
        mm_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int u = 0; u < nu; ++u) {
          const int4 un = my_units[u];                   // wave-uniform: scalar load
          const int mblk = un.x & 255, nv = (un.x >> 8) & 255, fblk = (un.x >> 16) & 15, slot = (un.x >> 20) & 255;
          const bool flush = un.x < 0;
          const int n8 = un.w;
          const int t = mtl * MM_M12_TF + fblk * 16 + j;
          const bool tv = t < T;
          // A operand rows: only the nv existing filters of the block are stored; the other lanes read a
          // duplicate and use zero
          const bool arow = j < nv;
          const float2* at = A + un.y + g * nv + (arow ? j : 0);
          const float2* pr = reinterpret_cast<const float2*>(Pp + (fblk * 16 + j) * MM_M12_PITCH + 2 * g + un.z);
          // The LDS is busy with the twelve transform waves (a read comes back after several hundred cycles),
          // so the operands are fetched a whole chunk of MM_M12_CH steps ahead: while the 2 CH MFMAs of one
          // chunk run, the 2 CH ds_read_b64 of the next are in flight.  Steps past n8 re-read the last step
          // and multiply by zero.
          float dA[4];
          if (p.out_mfcc) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dA[r] = Dt[(mblk * 4 + r) * 64 + lane];
          }
          mm_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
          if (n8 > 0) {
            float2 a[MM_M12_CH], bq[MM_M12_CH];
#pragma unroll
            for (int i = 0; i < MM_M12_CH; ++i) {
              const int s = min(i, n8 - 1);
              a[i] = at[s * 4 * nv]; bq[i] = pr[s * 4];
            }
            for (int s0 = 0; s0 < n8; s0 += MM_M12_CH) {
              float2 an[MM_M12_CH], bn[MM_M12_CH];
#pragma unroll
              for (int i = 0; i < MM_M12_CH; ++i) {
                const int s = min(s0 + MM_M12_CH + i, n8 - 1);
                an[i] = at[s * 4 * nv]; bn[i] = pr[s * 4];
              }
#pragma unroll
              for (int i = 0; i < MM_M12_CH; ++i) {
                const bool live = arow && (s0 + i < n8);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(live ? a[i].x : 0.0f, bq[i].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(live ? a[i].y : 0.0f, bq[i].y, acc1, 0, 0, 0);
              }
#pragma unroll
              for (int i = 0; i < MM_M12_CH; ++i) { a[i] = an[i]; bq[i] = bn[i]; }
            }
          }
          MM_STAMP_AT(2)
          float L[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mblk * 16 + 4 * g + r;
            const float v = acc0[r] + acc1[r];
            L[r] = tile512_db(fmaxf(p.amin, v), p.db_offset);
            if (tv && m < p.n_mels) {
              if (p.out_logmel) p.out_logmel[((int64_t)mb_clip * p.n_mels + m) * T + t] = L[r];
              vmax = fmaxf(vmax, L[r]);
              vmin = fminf(vmin, L[r]);
            }
          }
          MM_STAMP_AT(3)
          if (p.out_mfcc) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(dA[r], L[r], c, 0, 0, 0);
            if (flush) {                                 // last unit of this wave for frame block fblk
              *reinterpret_cast<float4*>(part + (slot * 64 + lane) * 4) = make_float4(c[0], c[1], c[2], c[3]);
              c = mm_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
              // arrival ticket: the LDS executes the operations of a CU in issue order, so when the ticket of
              // the last wave of this frame block is granted every partner's slot is already written
              const int slot0 = p.n_units[4 + fblk] & 255, n_slots = p.n_units[4 + fblk] >> 8;
              wave_lds_sync();
              int old = 0;
              if (lane == 0) old = __hip_atomic_fetch_add(cnt + fblk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              old = __builtin_amdgcn_readfirstlane(old);
              wave_lds_sync();
              MM_STAMP_AT(4)
              if (old == n_slots - 1) {
                float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 1
                for (int sl = 0; sl < n_slots; ++sl) {   // fixed order: deterministic
                  const float4 v = *reinterpret_cast<const float4*>(part + ((slot0 + sl) * 64 + lane) * 4);
                  sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
                }
                if (lane == 0) cnt[fblk] = 0;
                if (tv) {
                  float* o = p.out_mfcc + ((int64_t)mb_clip * p.n_mfcc + 4 * g) * T + t;
                  if (4 * g + 0 < p.n_mfcc) o[0] = sum.x;
                  if (4 * g + 1 < p.n_mfcc) o[(int64_t)T] = sum.y;
                  if (4 * g + 2 < p.n_mfcc) o[(int64_t)2 * T] = sum.z;
                  if (4 * g + 3 < p.n_mfcc) o[(int64_t)3 * T] = sum.w;
                }
              }
            }
          }
        }
        MM_STAMP_AT(5)
        if (nu > 0 && (!has_fft || mtl == tpc - 1)) {    // clip finished (for this workgroup): publish min / max
          vmax = wave_max(vmax);
          vmin = wave_min(vmin);
          if (lane == 0 && vmax > -INFINITY) {
            atomicMax(p.key_max + mb_clip, float_key(vmax));
            if (p.key_nmin) atomicMax(p.key_nmin + mb_clip, float_key(-vmin));
          }
          vmax = -INFINITY; vmin = INFINITY;
        }
      }
      MM_STAMP_AT(7)
      if (more && !DMA) stage_store(ntl);
      if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      MM_STAMP_AT(8)
      wg_barrier_lds();                                  // barrier A
      MM_STAMP_AT(9)
      mb_clip = b; mtl = tl;
      b = nb; tl = ntl;
    }
  }
  MM_STAMP_END(12)
}

// Clamped DCT for the clips the fused kernel could not finish: min < max - top_db -- the stored unclamped DCT plus the
// correction of the values under the threshold (mm_clamp_corr, mm_common.h); every other block leaves at once.
// skip_empty (the staged-sample kernel's analytic treatment of filters without weights, Logmel512Params): such a
// filter's row was never stored -- its value is the constant L0 -- and a clip that does NOT clamp still gets
// E[k] (thr - L0) added when thr > L0 (the fused DCT started its accumulators from E[k] L0): one add per element, the
// arithmetic of s16_add_rows / s16_fin_modspec_2k (clip mode).
__global__ __launch_bounds__(256) void dct_fixup_kernel(const float* __restrict__ logmel,
                                                         const int* __restrict__ key_max,
                                                         const int* __restrict__ key_nmin,
                                                         const float* __restrict__ dct_t /*[n_mels][KP]*/,
                                                         float* __restrict__ out, int64_t n_frames,
                                                         int n_mels, int n_mfcc, int kp, float top_db,
                                                         const float* __restrict__ dct_e /* E[16 kb] | bits, or nullptr */,
                                                         float amin, float db_offset) {
  const int64_t bpc = (n_frames + 255) / 256;
  const int64_t b = blockIdx.x / bpc;
  const float mx = key_float(key_max[b]), mn = -key_float(key_nmin[b]);
  const float thr = mx - top_db;
  const float L0 = mm_empty_level(amin, db_offset);
  const bool clamp = mn < thr;
  const bool skip_empty = dct_e != nullptr;
  const unsigned* ebits = skip_empty ? reinterpret_cast<const unsigned*>(dct_e + 16 * ((n_mfcc + 15) / 16)) : nullptr;
  if (!clamp && !(skip_empty && thr > L0)) return;   // nothing under the threshold: the unclamped DCT is the result
  const int64_t t = (blockIdx.x % bpc) * 256 + threadIdx.x;
  if (t >= n_frames) return;
  float* o = out + b * n_mfcc * n_frames + t;
  if (!clamp) {
    // one fmaf per element; the rows' values are requested sixteen at a time (a dependent load - fma - store chain per
    // coefficient ran at 2 TB/s: 0.10 ms for the reference default's 2 049 024 frames x 13)
    const float delta = thr - L0;
    for (int k0 = 0; k0 < n_mfcc; k0 += 16) {
      float v[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) v[kk] = o[(int64_t)min(k0 + kk, n_mfcc - 1) * n_frames];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
        if (k0 + kk < n_mfcc) o[(int64_t)(k0 + kk) * n_frames] = __builtin_fmaf(dct_e[k0 + kk], delta, v[kk]);
    }
    return;
  }
  // a clip that clamps: the correction of mm_clamp_corr on top of the stored (unclamped) DCT
  const float* lm = logmel + b * n_mels * n_frames + t;
  const float d0 = skip_empty ? fmaxf(thr - L0, 0.0f) : 0.0f;       // the empty filters all read L0
  for (int k0 = 0; k0 < n_mfcc; k0 += MM_DCT_KB) {
    float acc[MM_DCT_KB];
#pragma unroll
    for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = 0.0f;
    bool touched = mm_clamp_corr(
        acc, n_mels, thr, [&](int m) { return lm[(int64_t)m * n_frames]; },
        [&](int m0) { return skip_empty ? ebits[m0 >> 5] : 0u; },
        [&](int m, auto f) {
          const float* d = dct_t + (size_t)m * kp + k0;
#pragma unroll
          for (int kk = 0; kk < MM_DCT_KB; ++kk) f(kk, d[kk]);
        });
    if (d0 > 0.0f) {
#pragma unroll
      for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = __builtin_fmaf(dct_e[k0 + kk], d0, acc[kk]);
      touched = true;
    }
    if (touched) {
#pragma unroll
      for (int kk = 0; kk < MM_DCT_KB; ++kk)
        if (k0 + kk < n_mfcc) o[(int64_t)(k0 + kk) * n_frames] = o[(int64_t)(k0 + kk) * n_frames] + acc[kk];
    }
  }
}

// ---- host side ----
struct M12Tables {
  std::vector<float> a_tab;     // per filter block [steps][4][rows][2]
  std::vector<float> dct_tab;   // [nb][4][64]
  std::vector<int> units;       // [4][UMAX][4]
  std::vector<int> n_units;     // [4] units per mel wave, then [3] first slot | slots << 8 (+1 pad)
  int nb, n_slots;
};

// mel: [n_mels][257] (n_fft 512, or a smaller n_fft embedded at every E-th bin); dct: [n_mfcc][n_mels]
static bool build_m12_tables(const mm_config& c, const float* mel, const float* dct, M12Tables* o) {
  const int NB = (c.n_mels + 15) / 16;
  if (3 * NB > MM_M12_MW * MM_M12_UMAX) return false;
  o->nb = NB;
  o->a_tab.clear();
  std::vector<int> first_off(NB), kb(NB), n8(NB), rows(NB);
  for (int mb = 0; mb < NB; ++mb) {
    int lo = 257, hi = 0;
    for (int i = 0; i < 16; ++i) {
      const int m = mb * 16 + i;
      if (m >= c.n_mels) break;
      for (int k = 0; k < 257; ++k)
        if (mel[(size_t)m * 257 + k] != 0.0f) { lo = std::min(lo, k); hi = std::max(hi, k + 1); }
    }
    const int nv = std::min(16, c.n_mels - mb * 16);
    rows[mb] = nv;
    first_off[mb] = (int)(o->a_tab.size() / 2);
    if (hi <= lo) { kb[mb] = 0; n8[mb] = 0; continue; }   // empty block (filters above Nyquist): amin rows
    int k0 = lo & ~1;
    int ns = (hi - k0 + 7) / 8;
    if (k0 + 8 * ns > MM_M12_PITCH) k0 = MM_M12_PITCH - 8 * ns;   // stay inside the row (pads are zero)
    if (k0 < 0) return false;
    kb[mb] = k0; n8[mb] = ns;
    for (int s = 0; s < ns; ++s)
      for (int kc = 0; kc < 4; ++kc)
        for (int i = 0; i < nv; ++i) {
          const int m = mb * 16 + i;
          for (int e = 0; e < 2; ++e) {
            const int k = k0 + 8 * s + 2 * kc + e;
            o->a_tab.push_back(k < 257 ? mel[(size_t)m * 257 + k] : 0.0f);
          }
        }
  }
  o->dct_tab.assign((size_t)NB * 4 * 64, 0.0f);
  if (c.n_mfcc <= 16)
    for (int mb = 0; mb < NB; ++mb)
      for (int r = 0; r < 4; ++r)
        for (int l = 0; l < 64; ++l) {
          const int i = l & 15, kc = l >> 4, m = mb * 16 + 4 * kc + r;
          if (i < c.n_mfcc && m < c.n_mels) o->dct_tab[((size_t)mb * 4 + r) * 64 + l] = dct[(size_t)i * c.n_mels + m];
        }
  // units (frame block f, filter block) -> the four mel waves: heaviest first onto the least loaded wave
  // (ties: a wave that already holds units of f, so that its DCT chain covers them with one partial slot)
  struct U { int f, mb, cost; };
  std::vector<U> us;
  for (int f = 0; f < 3; ++f)
    for (int mb = 0; mb < NB; ++mb) us.push_back({f, mb, 2 * n8[mb] + 8});
  std::stable_sort(us.begin(), us.end(), [](const U& a, const U& b) { return a.cost > b.cost; });
  int load[MM_M12_MW] = {0, 0, 0, 0};
  std::vector<std::vector<U>> mine(MM_M12_MW);
  for (const U& u : us) {
    int best = -1;
    for (int w = 0; w < MM_M12_MW; ++w) {
      if ((int)mine[w].size() >= MM_M12_UMAX) continue;
      bool has_f = false, best_has_f = false;
      for (const U& v : mine[w]) has_f |= v.f == u.f;
      if (best >= 0) for (const U& v : mine[best]) best_has_f |= v.f == u.f;
      if (best < 0 || load[w] < load[best] || (load[w] == load[best] && has_f && !best_has_f)) best = w;
    }
    if (best < 0) return false;
    mine[best].push_back(u);
    load[best] += u.cost;
  }
  o->units.assign(MM_M12_MW * MM_M12_UMAX * 4, 0);
  o->n_units.assign(8, 0);
  // partial slots: one per (frame block, contributing wave), numbered frame block by frame block
  int slot_of[3][MM_M12_MW], slot = 0;
  for (int f = 0; f < 3; ++f) {
    const int first = slot;
    for (int w = 0; w < MM_M12_MW; ++w) {
      bool has = false;
      for (const U& v : mine[w]) has |= v.f == f;
      slot_of[f][w] = has ? slot++ : -1;
    }
    o->n_units[4 + f] = first | ((slot - first) << 8);
  }
  o->n_slots = slot;
  for (int w = 0; w < MM_M12_MW; ++w) {
    std::stable_sort(mine[w].begin(), mine[w].end(), [](const U& a, const U& b) { return a.f < b.f || (a.f == b.f && a.mb < b.mb); });
    o->n_units[w] = (int)mine[w].size();
    for (size_t i = 0; i < mine[w].size(); ++i) {
      const U& u = mine[w][i];
      const bool flush = i + 1 == mine[w].size() || mine[w][i + 1].f != u.f;
      int* d = &o->units[((size_t)w * MM_M12_UMAX + i) * 4];
      d[0] = (int)((unsigned)u.mb | ((unsigned)rows[u.mb] << 8) | ((unsigned)u.f << 16) | ((unsigned)slot_of[u.f][w] << 20) |
                   (flush ? 0x80000000u : 0u));
      d[1] = first_off[u.mb]; d[2] = kb[u.mb]; d[3] = n8[u.mb];
    }
  }
  return true;
}

// ---- the instantiations, listed once: key = (nr - 1) << 3 | pre << 2 | odd << 1 | unal, NR 1 .. 3 ----
using M12Kernel = void (*)(Logmel12mParams);
#define MM_M12_KEYS 24
template <int KEY>
static constexpr M12Kernel m12_entry() {
  return logmel12m_kernel<(KEY >> 3) + 1, (KEY & 4) != 0, (KEY & 2) != 0, (KEY & 1) != 0>;
}
template <int... KEY>
static M12Kernel m12_lookup(int key, std::integer_sequence<int, KEY...>) {
  static constexpr M12Kernel table[] = {m12_entry<KEY>()...};
  return table[key];
}
static M12Kernel m12_kernel(int key) { return m12_lookup(key, std::make_integer_sequence<int, MM_M12_KEYS>()); }

static void launch_m12(int nr, bool pre, bool odd, bool unal, dim3 grid, size_t lds, hipStream_t st,
                       const Logmel12mParams& q) {
  nr = nr <= 1 ? 1 : nr == 2 ? 2 : 3;
  const int key = (nr - 1) << 3 | (pre ? 4 : 0) | (odd ? 2 : 0) | (unal ? 1 : 0);
  hipLaunchKernelGGL(m12_kernel(key), grid, dim3(MM_M12_THREADS), lds, st, q);
}

static bool set_m12_attr(int bytes) {
  for (int key = 0; key < MM_M12_KEYS; ++key)
    if (hipFuncSetAttribute((const void*)m12_kernel(key), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
      return false;
  return true;
}
