#pragma once
// Sample-rate conversion on the matrix pipe (SURVEY.md 8(f) row N4: librosa.load(path, sr=sigSr) resamples every file
// the UI opens, script/mfcc.py:284,373).  Included by mm_side.hip.
//
// The rational-ratio polyphase FIR  y[m] = sum_j h[ph_m + j L] x[ih_m - j]  (t = m M + c, ih = t div L, ph = t mod L)
// is a BANDED GEMM: outputs m = q F + 16 b + r (F = c L >= 16, a multiple of L chosen by the host: outputs F apart share their taps; b = block of 16
// consecutive outputs inside a period of F, r < 16) read the input window x[q S + lo_b + k], S = F M / L, k < K, through
// taps that depend on (b, r, k) only --
//
//     Y_b[r][q] = sum_k A_b[r][k] * X_b[k][q],     A_b[r][k] = h[ph0(16 b + r) + (ih0(16 b + r) - lo_b - k) L],
//                                                  X_b[k][q] = x[q S + lo_b + k]
//
// -- i.e. D[16 x 16] += A[16 x 4] B[4 x 16] with v_mfma_f32_16x16x4_f32: exact float32 products, float32 accumulation
// (a k-ordered fmaf chain per output), at the vector pipe's FLOP rate with NO vector instruction per multiply-add.
// The band (K = taps per output + the 15 M / L samples the 16 rows of a block slide by) costs 8 % of zero work at
// 160 / 441.  A operands: a table in MFMA lane order built by the host (modulation_mfcc_amd/audio_io.py), streamed from
// L2 (one coalesced 256-byte load per MFMA); B operands: the clip's samples staged ONCE per tile of 16 QT periods in
// LDS (zero-filled outside the clip: no edge cases in the loop), one ds_read_b32 per MFMA -- lane (k = l / 16, q = l %
// 16) reads tile[q S + k]; for strides S that are multiples of 8 the tile is padded by one word per 32 (PAD) so that the
// 16 periods of a read do not share a bank.  A wave owns (block, period-tile) units of an item (clip, 16 QT periods);
// the D tile's four registers are four consecutive outputs: 16-byte stores.
struct RsmParams {
  const float* x;
  int64_t rows, n_in, x_stride;
  const float* atab;            // [NB][ksteps / 4][64][4]: lane l's taps of four consecutive k-steps in one 16-byte record
  const int* lo_off;            // [NB]: lo_b - lo_min
  int F, S, NB, ksteps, lo_min, QT, tile_floats;
  float* y;
  int64_t n_out, tiles_per_row, n_items;
  const int64_t* lens;          // RAGGED: [rows] valid samples per row (device), clamped into [1, n_in] by the kernel
  int64_t y_stride;             // RAGGED: output row pitch >= n_out (the uniform entry's rows are n_out apart)
};

// PAD: one pad word per 32 in the LDS tile (strides S that put the 16 periods of a read on few banks);
// VEC: rows are 16-byte aligned (base pointer and pitch): the tile starts at a multiple of four samples and is staged
// with 16-byte loads.
// RAGGED (mm_resample_banded_ragged_f32): row b holds n_b = clamp(lens[b], 1, n_in) samples and gets n_out_b =
// ceil(n_b F / S) (= ceil(n_b L / M): F / S is L / M) outputs, +0.0 behind them up to n_out.  n_b takes the place of
// n_in in the staging bounds -- the tile geometry (q0, g0) does not depend on it, so the outputs are those of the row
// called alone --; it is read once per item through `row`, which derives from blockIdx.x and the item counter alone:
// a scalar load, the same value in every wave, so the branch around the two barriers of an item is taken by the whole
// workgroup or by none of it.  A tile wholly behind n_out_b stages nothing, multiplies nothing and stores zeros; in
// the last tile with outputs, a unit wholly behind n_out_b skips its multiplies.
template <bool PAD, bool VEC, bool RAGGED = false>
__global__ __launch_bounds__(256) void resample_mfma_kernel(RsmParams p) {
  extern __shared__ __attribute__((aligned(16))) float rsm_xs[];
  float* xs = rsm_xs;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: unit, block and A addresses live in SGPRs
  const int n = lane & 15, kq = lane >> 4;
  // K order inside a group of 32 samples (8 k-steps): lane quarter kq owns the 8 CONSECUTIVE samples koff + 0 .. 7,
  // koff = 0 / 16 / 8 / 24 -- the two quarters of a 32-lane half are 16 words apart, so for every odd period stride S
  // the 32 addresses of a read fall on 32 different banks ({S q mod 32, q < 16} and its shift by 16 are complementary);
  // the A table is stored in the same order (audio_io.banded_tables).
  const int koff = ((kq & 1) << 4) | ((kq & 2) << 2);
  const int periods = 16 * p.QT;
  const int n_units = p.NB * p.QT;
  for (int64_t item = blockIdx.x; item < p.n_items; item += gridDim.x) {
    const int64_t row = item / p.tiles_per_row;
    int64_t tile = item - row * p.tiles_per_row;
    if (RAGGED) {
      // rotate the row's tiles by a hash of the row: workgroups land on the CUs round-robin, and with tile = item mod
      // tiles_per_row a CU would meet the same tile of every row -- the CUs with the first tiles, which no row leaves
      // empty, would do all the work.  A rotation per row: every (row, tile) still belongs to exactly one item.
      tile = (tile + (int64_t)(((uint32_t)row * 2654435761u) >> 8)) % p.tiles_per_row;
    }
    const int64_t q0 = tile * periods;
    const float* xr = p.x + row * p.x_stride;
    int64_t n_in = p.n_in, n_out_row = p.n_out;
    if (RAGGED) {
      const int64_t len = p.lens[row];
      n_in = len < 1 ? 1 : (len > p.n_in ? p.n_in : len);
      n_out_row = (n_in * p.F + p.S - 1) / p.S;
      const int64_t m0 = q0 * p.F;
      if (m0 >= n_out_row) {                            // workgroup-uniform: no barrier is skipped by a part of it
        const int64_t m1 = m0 + (int64_t)periods * p.F < p.n_out ? m0 + (int64_t)periods * p.F : p.n_out;
        float* yr = p.y + row * p.y_stride;
        for (int64_t m = m0 + threadIdx.x; m < m1; m += 256) yr[m] = 0.0f;
        continue;
      }
    }
    int64_t g0 = q0 * (int64_t)p.S + p.lo_min;
    const int sh = VEC ? (int)(g0 & 3) : 0;                // tile word i holds x[g0 + i] with g0 a multiple of 4
    g0 -= sh;
    __syncthreads();                                    // every wave is done reading the previous tile
    if (VEC) {
      // every load of the tile in flight at once (up to 16 x 16 bytes per thread), zero outside the clip
      const int n4 = (p.tile_floats + 3 + 3) >> 2;
      for (int c0 = threadIdx.x; c0 < n4; c0 += 16 * 256) {
        float4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int c = c0 + 256 * u;
          const int64_t gi = g0 + 4 * (int64_t)c;
          v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (c < n4) {
            if (gi >= 0 && gi + 3 < n_in) {
              v[u] = *reinterpret_cast<const float4*>(xr + gi);
            } else if (gi + 3 >= 0 && gi < n_in) {      // the vector straddles an end of the clip
              v[u].x = (gi >= 0 && gi < n_in) ? xr[gi] : 0.0f;
              v[u].y = (gi + 1 >= 0 && gi + 1 < n_in) ? xr[gi + 1] : 0.0f;
              v[u].z = (gi + 2 >= 0 && gi + 2 < n_in) ? xr[gi + 2] : 0.0f;
              v[u].w = (gi + 3 >= 0 && gi + 3 < n_in) ? xr[gi + 3] : 0.0f;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int c = c0 + 256 * u;
          if (c < n4) {
            if (PAD) {
              const int i = 4 * c;
              xs[i + (i >> 5)] = v[u].x; xs[i + 1 + ((i + 1) >> 5)] = v[u].y;
              xs[i + 2 + ((i + 2) >> 5)] = v[u].z; xs[i + 3 + ((i + 3) >> 5)] = v[u].w;
            } else {
              reinterpret_cast<float4*>(xs)[c] = v[u];
            }
          }
        }
      }
    } else {
      for (int i0 = threadIdx.x; i0 < p.tile_floats; i0 += 32 * 256) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const int i = i0 + 256 * u;
          const int64_t gi = g0 + i;
          v[u] = (i < p.tile_floats && gi >= 0 && gi < n_in) ? xr[gi] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const int i = i0 + 256 * u;
          if (i < p.tile_floats) xs[PAD ? i + (i >> 5) : i] = v[u];
        }
      }
    }
    __syncthreads();
    for (int u = wave; u < n_units; u += 4) {
      const int b = u / p.QT, qt = u - b * p.QT;
      // A operands: [b][group of 8 k-steps][2][lane][4] -- two 16-byte loads per lane and group, through a buffer
      // descriptor: wave-uniform base, the group's offset in an SGPR (soffset), the lane's 16 bytes a constant VGPR, the
      // second half an immediate -- NO vector instruction per load (plain pointers cost a 64-bit vector add per group,
      // and vector instructions add to the f32 MFMA's time)
      const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(p.atab) + (size_t)b * p.ksteps * 64, 0, p.ksteps * 256, 0x00020000);
      const int a_voff = lane * 16;
      const int i0 = (qt * 16 + n) * p.S + p.lo_off[b] + koff + sh;
      const char* xb = reinterpret_cast<const char*>(xs) + 4 * i0;        // !PAD: group g's eight samples at xb + 128 g
      // two accumulator chains (even / odd k-steps): a 16x16x4 MFMA issues every 32 cycles but its result is ready
      // after 40, and two half-length fmaf chains round less than one
      mm_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
      const int G = p.ksteps >> 3;                     // the host pads ksteps to a multiple of 8
      mm_v4f al[3], ah[3];
      float bb[3][8];
      auto load_ab = [&](int g, int set) {
        g = g < G ? g : G - 1;                         // past the end: re-request the last group (no tail code)
        al[set] = __builtin_bit_cast(mm_v4f, __builtin_amdgcn_raw_buffer_load_b128(ra, a_voff, g * 2048, 0));
        ah[set] = __builtin_bit_cast(mm_v4f, __builtin_amdgcn_raw_buffer_load_b128(ra, a_voff + 1024, g * 2048, 0));
        if (PAD) {
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const int i = i0 + 32 * g + s;
            bb[set][s] = xs[i + (i >> 5)];
          }
        } else {
          const float* xg = reinterpret_cast<const float*>(xb + (g << 7));      // one vector add per group
#pragma unroll
          for (int s = 0; s < 8; ++s) bb[set][s] = xg[s];
        }
      };
      auto mfma8 = [&](int set) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(al[set].x, bb[set][0], acc, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(al[set].y, bb[set][1], acc1, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(al[set].z, bb[set][2], acc, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(al[set].w, bb[set][3], acc1, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[set].x, bb[set][4], acc, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[set].y, bb[set][5], acc1, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[set].z, bb[set][6], acc, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[set].w, bb[set][7], acc1, 0, 0, 0);
      };
      // Software pipeline over three register sets: the operands of group g + 2 are requested BEFORE the eight MFMAs
      // of group g issue -- 512 cycles of this wave's matrix work (twice that with the SIMD's second wave) cover the
      // L2 round trip of the A loads and the LDS reads; the sched_barriers keep the compiler from sinking the
      // requests back to their uses.
      // RAGGED: a unit whose first output lies behind the row's last one only stores zeros (wave-uniform; no barrier
      // inside the unit loop)
      if (!RAGGED || (q0 + qt * 16) * (int64_t)p.F + 16 * b < n_out_row) {
        load_ab(0, 0);
        load_ab(1, 1);
        for (int g = 0; g < G; g += 3) {
          load_ab(g + 2, 2);
          __builtin_amdgcn_sched_barrier(0);
          mfma8(0);
          __builtin_amdgcn_sched_barrier(0);
          if (g + 1 < G) {
            load_ab(g + 3, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(1);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (g + 2 < G) {
            load_ab(g + 4, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma8(2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        acc += acc1;
      }
      // D[i = 4 kq + v][j = n]: four consecutive outputs of period q0 + 16 qt + n; rows past the period's F outputs
      // (the last block of a period that is not a multiple of 16) belong to the next period's first block
      const int r0 = 16 * b + 4 * kq;
      const int64_t m = (q0 + qt * 16 + n) * (int64_t)p.F + r0;
      float* yo = p.y + row * (RAGGED ? p.y_stride : p.n_out) + m;
      if (RAGGED) {                                     // +0.0 behind the row's own outputs
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (m + v >= n_out_row) acc[v] = 0.0f;
      }
      if (r0 + 3 < p.F && m + 3 < p.n_out && ((reinterpret_cast<uintptr_t>(yo) & 15) == 0)) {
        *reinterpret_cast<float4*>(yo) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (r0 + v < p.F && m + v < p.n_out) yo[v] = acc[v];
      }
    }
  }
}
