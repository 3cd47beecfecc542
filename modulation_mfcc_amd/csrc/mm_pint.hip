// Praat's intensity contour (include/modmfcc_pint.h): the mean-centred, window-weighted power of
// frames whose centre samples the host lists per row; and the value lookup of the contour.
//
//   pint_kernel<T>   one workgroup of 256 threads per (row, tile of PINT_TILE consecutive table entries).  The threads form
//                    16 GROUPS of PINT_S = 16 lanes.  A frame is always summed by one group, in ONE order:
//                      the 2 hw + 1 taps are cut into 16 consecutive chunks (the first (2 hw + 1) % 16 one tap longer);
//                      lane s adds its chunk's terms in ascending order from 0.0 (terms outside [l, r] are skipped);
//                      the 16 partial sums are added by the butterfly lane ^ 8, ^ 4, ^ 2, ^ 1.
//                    That holds for the samples' sum (the mean), the weighted squares (continued through the channels) and
//                    the window's sum; it is a function of hw, c, l and r alone.
//     sub-sweeps     the tile is worked in sub-sweeps of `sub` entries (16 .. 128, from p->span: as many as the staged copy
//                    holds).  Per sub-sweep the workgroup copies the samples from the lowest window start on to LDS once, as
//                    float64; a group owns sub / 16 consecutive entries.
//     dense path     a group whose 8 entries lie within 8 consecutive samples (time_step = 1 / sr), unclipped and staged,
//                    keeps the 8 frames centred at c0 .. c0 + 7 in registers; an entry takes the frame of its centre: a lane walks its chunk once, each sample it reads serves 8 frames, the taps slide
//                    through a register window.  4 float64 operations per tap and frame, 1 / 8 LDS read of each kind.
//     frame path     every other frame: the group walks the frame alone, from the staged copy or, where the frame does not
//                    lie in it (or nothing is staged), from memory -- the same operations in the same order either way.
//   pint_value_kernel   a thread per query time.
#include "mm_common.h"
#include "../../include/modmfcc_pint.h"

#define PINT_S 16          // lanes of a group = chunks of a frame
#define PINT_R 8           // frames a group holds in registers on the dense path
#define PINT_GROUPS 16     // groups of a workgroup
#define PINT_TILE 128      // table entries of a workgroup = PINT_GROUPS * PINT_R
#define PINT_PAD 16        // slack behind the staged samples and taps: the dense path's last block reads (and drops) up to 2 R - 2
#define PINT_LDS_MAX 98304 // what a workgroup may take of the CU's 160 KiB

namespace {

template <class T>
struct PintArgs {
  const T* x;
  const double* w;
  const int32_t* centre;
  const int64_t* len;
  double* y;
  int64_t n_max, x_row, x_chan, t_max, centre_row, y_row;
  int hw, channels, tiles, sub, cap, w_lds, linear, keep_mean;   // cap: staged samples per channel (0: none); w_lds: taps in LDS
};

__device__ __forceinline__ double pint_group_sum(double v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

__device__ __forceinline__ double pint_level(double P, int linear) {
  return linear ? P : (P < 4e-40 ? -300.0 : 10.0 * log10(P / 4e-10));
}

// One block of R steps of the dense path: step t = t0 + u reads the lane's sample t and tap t; frame r takes tap t - r.
// MEAN: acc[r] += x.  Otherwise acc[r] = fma((x - m[r])^2, tap, acc[r]).  PRED: only taps 0 <= t - r < lc count.
template <bool PRED, bool MEAN>
__device__ __forceinline__ void pint_block(const double* xs, const double* ws, int t0, int lc, const double (&m)[PINT_R],
                                           double (&acc)[PINT_R], double (&wr)[PINT_R]) {
#pragma unroll
  for (int u = 0; u < PINT_R; ++u) {
    const double x = xs[t0 + u];
    if (!MEAN) wr[u] = ws[t0 + u];
#pragma unroll
    for (int r = 0; r < PINT_R; ++r) {
      double v;
      if (MEAN) {
        v = acc[r] + x;
      } else {
        const double d = x - m[r];
        v = fma(d * d, wr[(u - r + PINT_R) % PINT_R], acc[r]);
      }
      if (PRED) {
        const int i = t0 + u - r;
        acc[r] = (i >= 0 && i < lc) ? v : acc[r];
      } else {
        acc[r] = v;
      }
    }
  }
}

template <bool MEAN>
__device__ __forceinline__ void pint_dense_pass(const double* xs, const double* ws, int q, int lc, const double (&m)[PINT_R],
                                                double (&acc)[PINT_R]) {
  double wr[PINT_R];
#pragma unroll
  for (int r = 0; r < PINT_R; ++r) wr[r] = 0.0;
  // steps 0 .. q + R - 1 at the most (lc <= q + 1); blocks 1 .. with b R + R - 1 <= q - 1 need no predicate
  const int blocks = (q + PINT_R) / PINT_R + 1;
  const int full_end = q / PINT_R;                     // blocks [1, full_end) are full
  pint_block<true, MEAN>(xs, ws, 0, lc, m, acc, wr);
  int b = 1;
  for (; b < full_end; ++b) pint_block<false, MEAN>(xs, ws, b * PINT_R, lc, m, acc, wr);
  for (; b < blocks; ++b) pint_block<true, MEAN>(xs, ws, b * PINT_R, lc, m, acc, wr);
}

// The frame path: the lane's chunk [i0, i1) of taps (already cut to [l, r]) of one frame and one channel.
template <class XS>
__device__ __forceinline__ double pint_chunk_mean(XS xs, int i0, int i1) {
  double a = 0.0;
  for (int i = i0; i < i1; ++i) a = a + (double)xs[i];
  return a;
}
template <class XS, class WS>
__device__ __forceinline__ double pint_chunk_power(XS xs, WS ws, int i0, int i1, double m, double a) {
  for (int i = i0; i < i1; ++i) {
    const double d = (double)xs[i] - m;
    a = fma(d * d, ws[i], a);
  }
  return a;
}
template <class WS>
__device__ __forceinline__ double pint_chunk_weight(WS ws, int i0, int i1) {
  double a = 0.0;
  for (int i = i0; i < i1; ++i) a = a + ws[i];
  return a;
}

template <class T>
__global__ __launch_bounds__(PINT_S* PINT_GROUPS) void pint_kernel(PintArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int32_t cent[PINT_TILE];
  // LDS: the taps [w_lds + PAD] | the staged samples [channels][cap + PAD]
  double* wl = reinterpret_cast<double*>(smem);
  double* stage = wl + (a.w_lds ? a.w_lds + PINT_PAD : 0);
  const int pitch = a.cap + PINT_PAD;
  const int tid = threadIdx.x, s = tid & (PINT_S - 1), g = tid / PINT_S;
  const int64_t row = blockIdx.x / a.tiles;
  const int64_t k0 = (int64_t)(blockIdx.x % a.tiles) * PINT_TILE;
  const T* xr = a.x + row * a.x_row;
  double* yr = a.y + row * a.y_row;
  int64_t len64 = a.len ? a.len[row] : a.n_max;
  len64 = len64 < 0 ? 0 : len64 > a.n_max ? a.n_max : len64;
  const int len = (int)len64;
  const int hw = a.hw, W = 2 * hw + 1;
  const int q = W / PINT_S, rem = W % PINT_S;
  const int cs = s * q + (s < rem ? s : rem), lc = q + (s < rem ? 1 : 0);    // the lane's chunk: taps [cs, cs + lc)

  if (tid < PINT_TILE) {
    int c = -1;
    if (k0 + tid < a.t_max) {
      c = a.centre[row * a.centre_row + k0 + tid];
      if (c < 0 || c >= len) c = -1;
    }
    cent[tid] = c;
  }
  for (int i = tid; i < a.w_lds; i += PINT_S * PINT_GROUPS) wl[i] = a.w[i];
  __syncthreads();

  // the window's sum of an unclipped frame, in the frame's order (the dense path's frames are unclipped)
  double sw_full = 0.0;
  if (a.w_lds) sw_full = pint_group_sum(pint_chunk_weight(wl, cs, cs + lc));
  const double nch = (double)a.channels;

  const int per = a.sub / PINT_GROUPS;
  for (int e0 = 0; e0 < PINT_TILE && k0 + e0 < a.t_max; e0 += a.sub) {
    // the sub-sweep's staged copy: from the lowest window start on, at most cap samples, never at or behind len
    int cmin = 0x7FFFFFFF;
    for (int e = 0; e < a.sub; ++e) {
      const int c = cent[e0 + e];
      if (c >= 0 && c < cmin) cmin = c;
    }
    int s0 = 0, staged = 0;
    if (cmin != 0x7FFFFFFF && a.cap > 0) {              // (workgroup-uniform)
      s0 = cmin - hw < 0 ? 0 : cmin - hw;
      staged = len - s0 < a.cap ? len - s0 : a.cap;
      for (int ch = 0; ch < a.channels; ++ch) {
        const T* xc = xr + ch * a.x_chan + s0;
        double* sc = stage + (size_t)ch * pitch;
        for (int i = tid; i < staged; i += PINT_S * PINT_GROUPS) sc[i] = (double)xc[i];
      }
    }
    __syncthreads();

    const int eg = e0 + g * per;                        // the group's first entry
    bool dense = per == PINT_R && a.w_lds != 0;
    int c0 = 0;
    if (dense) {
      // eight valid entries, the lowest centre c0: the eight frames centred at c0 .. c0 + 7 are computed, an entry takes the
      // frame of its centre (a table of a frame per sample repeats or skips a centre where the framing's rounding falls
      // on a tie); an entry whose centre lies further on goes through the frame path below
      c0 = cent[eg];
#pragma unroll
      for (int r = 1; r < PINT_R; ++r) {
        const int c = cent[eg + r];
        dense = dense && c >= 0;
        c0 = c < c0 ? c : c0;
      }
      int near = 0;
#pragma unroll
      for (int r = 0; r < PINT_R; ++r) near += (unsigned)(cent[eg + r] - c0) < (unsigned)PINT_R;
      dense = dense && near >= PINT_R - 2;
      dense = dense && c0 >= 0 && c0 - hw >= s0 && c0 + PINT_R - 1 + hw <= len - 1 && c0 + PINT_R - 1 + hw - s0 < staged;
    }
    if (dense) {                                        // (group-uniform; four groups of a wave may differ)
      double acc[PINT_R], m[PINT_R];
#pragma unroll
      for (int r = 0; r < PINT_R; ++r) acc[r] = m[r] = 0.0;
      const int base = c0 - hw - s0 + cs;
      for (int ch = 0; ch < a.channels; ++ch) {
        const double* xs = stage + (size_t)ch * pitch + base;
        if (!a.keep_mean) {
          double sum[PINT_R];
#pragma unroll
          for (int r = 0; r < PINT_R; ++r) sum[r] = 0.0;
          pint_dense_pass<true>(xs, wl + cs, q, lc, m, sum);
#pragma unroll
          for (int r = 0; r < PINT_R; ++r) m[r] = pint_group_sum(sum[r]) / (double)W;
        }
        pint_dense_pass<false>(xs, wl + cs, q, lc, m, acc);
      }
      const int mine = s < PINT_R ? cent[eg + s] - c0 : -1;      // lane s < 8 stores entry s: the frame of its centre
      double out = 0.0;
#pragma unroll
      for (int r = 0; r < PINT_R; ++r) {
        const double P = pint_group_sum(acc[r]) / (sw_full * nch);
        if (mine == r) out = pint_level(P, a.linear);
      }
      if ((unsigned)mine < (unsigned)PINT_R) yr[k0 + eg + s] = out;
    }
    {
      for (int f = 0; f < per; ++f) {
        const int64_t k = k0 + eg + f;
        if (k >= a.t_max) break;
        const int c = cent[eg + f];
        if (dense && (unsigned)(c - c0) < (unsigned)PINT_R) continue;     // (stored above)
        if (c < 0) {
          if (s == 0) yr[k] = 0.0;
          continue;
        }
        const int l = c - hw < 0 ? 0 : c - hw, r = c + hw > len - 1 ? len - 1 : c + hw;
        // the lane's taps, cut to [l, r]: tap i is sample c - hw + i
        int i0 = cs, i1 = cs + lc;
        if (i0 < l - (c - hw)) i0 = l - (c - hw);
        if (i1 > r - (c - hw) + 1) i1 = r - (c - hw) + 1;
        const bool in_lds = staged > 0 && l >= s0 && r - s0 < staged;      // (group-uniform)
        const bool clipped = r - l + 1 != W;
        double acc = 0.0, sw;
        const double count = (double)(r - l + 1);
        // (two address spaces, two loops each: no pointer chosen between LDS and memory)
        if (a.w_lds) {
          sw = clipped ? pint_group_sum(pint_chunk_weight(wl, i0, i1)) : sw_full;
        } else {
          sw = pint_group_sum(pint_chunk_weight(a.w, i0, i1));
        }
        for (int ch = 0; ch < a.channels; ++ch) {
          double m = 0.0;
          if (in_lds) {
            const double* xs = stage + (size_t)ch * pitch + (c - hw - s0);   // (may point before the copy: indexed from i0 on)
            if (!a.keep_mean) m = pint_group_sum(pint_chunk_mean(xs, i0, i1)) / count;
            acc = a.w_lds ? pint_chunk_power(xs, (const double*)wl, i0, i1, m, acc) : pint_chunk_power(xs, a.w, i0, i1, m, acc);
          } else {
            const T* xs = xr + ch * a.x_chan + (c - hw);
            if (!a.keep_mean) m = pint_group_sum(pint_chunk_mean(xs, i0, i1)) / count;
            acc = a.w_lds ? pint_chunk_power(xs, (const double*)wl, i0, i1, m, acc) : pint_chunk_power(xs, a.w, i0, i1, m, acc);
          }
        }
        const double P = pint_group_sum(acc) / (sw * nch);
        if (s == 0) yr[k] = pint_level(P, a.linear);
      }
    }
    __syncthreads();                                    // the next sub-sweep overwrites the copy
  }
}

struct PintValueArgs {
  const double* y;
  const int64_t* frames;
  const double* t1;
  const double* q;
  double* out;
  int64_t rows, t_max, y_row, n_q, q_row, out_row;
  double dt;
  int depth;
};

__global__ __launch_bounds__(256) void pint_value_kernel(PintValueArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.rows * a.n_q) return;
  const int64_t row = i / a.n_q, j = i - row * a.n_q;
  int64_t T = a.frames ? a.frames[row] : a.t_max;
  T = T < 0 ? 0 : T > a.t_max ? a.t_max : T;
  const double* y = a.y + row * a.y_row;
  const double t = a.q[row * a.q_row + j], t1 = a.t1[row], dt = a.dt;
  double v = __builtin_nan("");
  const double lo = t1 - dt / 2;
  if (T >= 1 && t >= lo && t <= lo + (double)T * dt) {       // (false for a NaN time)
    const double sx = (t - t1) / dt;
    if (sx <= 0.0) {
      v = y[0];
    } else if (sx >= (double)(T - 1)) {
      v = y[T - 1];
    } else {
      const int64_t ia = (int64_t)floor(sx), ib = ia + 1;
      if (sx == (double)ia) {
        v = y[ia];
      } else {
        int64_t depth = a.depth;
        if (depth > ia + 1) depth = ia + 1;
        if (depth > T - 1 - ia) depth = T - 1 - ia;
        if (depth <= 0) {
          v = y[(int64_t)floor(sx + 0.5)];
        } else if (depth == 1) {
          v = y[ia] + (sx - (double)ia) * (y[ib] - y[ia]);
        } else {
          const double yl = y[ia], yr = y[ib];
          const double dl = 0.5 * (yr - y[ia - 1]), dr = 0.5 * (y[ib + 1] - yl);
          const double fl = sx - (double)ia, fr = (double)ib - sx;
          v = yl * fr + yr * fl - fl * fr * (0.5 * (dr - dl) + (fl - 0.5) * (dl + dr - 2.0 * (yr - yl)));
        }
      }
    }
  }
  a.out[row * a.out_row + j] = v;
}

template <class T>
int pint_run(const mm_pint_params* p, const T* d_x, int64_t rows, int64_t n_max, int64_t x_row, int64_t x_chan,
             const double* d_w, const int32_t* d_centre, int64_t t_max, int64_t centre_row, const int64_t* d_len, double* d_y,
             int64_t y_row, void* stream) {
  const int rc = mm_pint_check(p);
  if (rc != MM_OK) return rc;
  if (!d_x || !d_w || !d_centre || !d_y || rows < 1 || t_max < 1 || n_max < 1) return MM_ERR_INVALID_ARG;
  if (n_max >= 0x7FFFFFFFll - 32768 || t_max >= 0x7FFFFFFFll) return MM_ERR_INVALID_ARG;
  if (x_chan < n_max || (rows > 1 && x_row < (int64_t)p->channels * x_chan)) return MM_ERR_INVALID_ARG;
  if (y_row < t_max || (centre_row != 0 && centre_row < t_max)) return MM_ERR_INVALID_ARG;
  const int64_t tiles = (t_max + PINT_TILE - 1) / PINT_TILE;
  if (rows > 0x7FFFFFFFll / tiles) return MM_ERR_INVALID_ARG;
  // LDS: the taps where they leave room for a window of samples per channel; then the largest sub-sweep whose span --
  // the tile's, in proportion -- fits, or a window's worth at the least (frames outside the copy read from memory)
  const int64_t W = 2 * (int64_t)p->hw + 1, doubles = PINT_LDS_MAX / 8;
  int w_lds = 0, sub = PINT_GROUPS, cap = 0;
  if (W + PINT_PAD + (W + PINT_PAD) * p->channels <= doubles) {
    w_lds = (int)W;
    const int64_t room = (doubles - (W + PINT_PAD)) / p->channels - PINT_PAD;
    const int64_t span = std::min<int64_t>(std::max<int64_t>(p->span, W), n_max);
    sub = PINT_TILE;
    while (sub > PINT_GROUPS && (span - W) * sub / PINT_TILE + W > room) sub >>= 1;
    cap = p->span > 0 ? (int)std::min<int64_t>((span - W) * sub / PINT_TILE + W, room) : 0;
    if (cap > 0 && cap < std::min<int64_t>(W, n_max)) cap = 0;
  }
  const size_t lds = ((w_lds ? (size_t)w_lds + PINT_PAD : 0) + (size_t)p->channels * ((size_t)cap + PINT_PAD)) * sizeof(double);
  static PerDeviceOnce once;
  const int orc = per_device_once(once, "pint_kernel", [] {
    return hipFuncSetAttribute((const void*)pint_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, PINT_LDS_MAX) ==
           hipSuccess;
  });
  if (orc) return orc;
  const PintArgs<T> a = {d_x, d_w, d_centre, d_len, d_y, n_max, x_row, x_chan, t_max, centre_row, y_row, p->hw, p->channels,
                         (int)tiles, sub, cap, w_lds, p->flags & MM_PINT_LINEAR, p->flags & MM_PINT_KEEP_MEAN};
  hipLaunchKernelGGL(pint_kernel<T>, dim3((unsigned)(rows * tiles)), dim3(PINT_S * PINT_GROUPS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // namespace

extern "C" {

int mm_pint_version(void) { return MM_PINT_VERSION; }

int mm_pint_check(const mm_pint_params* p) {
  if (!p) return MM_ERR_INVALID_ARG;
  if (p->hw < 1 || p->channels < 1 || p->span < 0) return MM_ERR_INVALID_ARG;
  if ((p->flags & ~(MM_PINT_LINEAR | MM_PINT_KEEP_MEAN)) || p->reserved) return MM_ERR_INVALID_ARG;
  if (p->hw > MM_PINT_MAX_HALF || p->channels > MM_PINT_MAX_CHANNELS) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

int32_t mm_pint_tile_frames(const mm_pint_params* p) {
  const int rc = mm_pint_check(p);
  return rc != MM_OK ? rc : PINT_TILE;
}

int mm_pint_f32(const mm_pint_params* p, const float* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                int64_t x_channel_stride, const double* d_w, const int32_t* d_centre, int64_t t_max,
                int64_t centre_row_stride, const int64_t* d_len, double* d_y, int64_t y_row_stride, void* stream) {
  return pint_run<float>(p, d_x, rows, n_max, x_row_stride, x_channel_stride, d_w, d_centre, t_max, centre_row_stride, d_len,
                         d_y, y_row_stride, stream);
}

int mm_pint_f64(const mm_pint_params* p, const double* d_x, int64_t rows, int64_t n_max, int64_t x_row_stride,
                int64_t x_channel_stride, const double* d_w, const int32_t* d_centre, int64_t t_max,
                int64_t centre_row_stride, const int64_t* d_len, double* d_y, int64_t y_row_stride, void* stream) {
  return pint_run<double>(p, d_x, rows, n_max, x_row_stride, x_channel_stride, d_w, d_centre, t_max, centre_row_stride, d_len,
                          d_y, y_row_stride, stream);
}

int mm_pint_value_f64(const double* d_y, int64_t rows, int64_t t_max, int64_t y_row_stride, const int64_t* d_frames,
                      const double* d_t1, double time_step, const double* d_q, int64_t n_q, int64_t q_row_stride,
                      int32_t depth, double* d_out, int64_t out_row_stride, void* stream) {
  if (!d_y || !d_t1 || !d_q || !d_out || rows < 1 || t_max < 1 || n_q < 1) return MM_ERR_INVALID_ARG;
  if (y_row_stride < t_max || out_row_stride < n_q || (q_row_stride != 0 && q_row_stride < n_q)) return MM_ERR_INVALID_ARG;
  if (!(time_step > 0.0) || !std::isfinite(time_step) || depth < MM_PINT_NEAREST || depth > MM_PINT_CUBIC) return MM_ERR_INVALID_ARG;
  if (rows > 0x7FFFFFFFll * 256 / n_q) return MM_ERR_INVALID_ARG;
  const PintValueArgs a = {d_y, d_frames, d_t1, d_q, d_out, rows, t_max, y_row_stride, n_q, q_row_stride, out_row_stride,
                           time_step, depth};
  const int64_t blocks = (rows * n_q + 255) / 256;
  hipLaunchKernelGGL(pint_value_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
