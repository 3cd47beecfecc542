// Ragged batches: MFCC (and modulation spectrum) of a padded batch [B][n_max] with one length per clip, every clip's
// result equal to what that clip gives alone.  gfx950 (MI355X / CDNA4) only.  DESIGN.md section 12.
//
// The path is built from the stage entries that exist (mm_logmel_f32, mm_modspec_f32) and four small kernels:
//   main pass   mm_logmel_f32 on the caller's audio as it lies: every frame whose whole span ends at or before the clip's
//               length is right already; the others ("edge frames", a handful per clip) hold whatever the padding gave
//   ragged_gather_kernel    per clip a short row [a_b, L_b) + zeros into the workspace, a_b a multiple of the hop
//   patch pass  mm_logmel_f32 on those rows [B][n_patch]
//   ragged_scatter_kernel   the patch's columns over the edge columns of the main log-mel
//   ragged_max_kernel       per-clip maximum over the n_mels x T_b valid values (an ordered-key atomicMax per workgroup)
//   ragged_clamp_dct_kernel top_db clamp + DCT-II with T_b per clip, 0.0f stored for t >= T_b
//   mm_modspec_f32 over the result when the spectrum is asked for (the zero fill IS the transform's zero padding)
#include "mm_common.h"
#include "mm_plan.h"

namespace {

// Frame geometry of a plan, one value set per call (host), and the per-clip quantities every kernel derives from it.
// Frame t reads the samples [t hop - pl, t hop + pr): the n_fft points of the frame -- or the 512 points the embedded
// n_fft 64 / 128 / 256 plans transform (their window is zero outside the frame, but 0 * NaN is NaN).
struct RaggedGeo {
  int64_t n_samples, t_max;
  int hop, pr, odd;      // odd = n_fft - 2 (n_fft / 2): what an odd n_fft consumes beyond its centre padding
  int guard;             // patch frames in front of the first edge frame: ceil((pl + (preemph ? 1 : 0)) / hop)
  int n_patch, t_patch;  // samples / frames of a patch row
};

struct RaggedClip {
  int64_t len;           // lengths[b] clamped into [1, n_samples]
  int64_t t_b;           // frames of the clip alone
  int64_t t_e;           // first edge frame: the first t with t hop + pr > len (t_e <= t_b)
  int64_t t_a;           // clip frame of patch frame 0; the patch row starts at sample t_a hop
};

__device__ __forceinline__ RaggedClip ragged_clip(const RaggedGeo& g, const int64_t* __restrict__ lengths, int64_t b) {
  RaggedClip c;
  int64_t len = lengths[b];
  len = len < 1 ? 1 : (len > g.n_samples ? g.n_samples : len);
  c.len = len;
  c.t_b = 1 + (len - g.odd) / g.hop;
  c.t_e = len >= g.pr ? (len - g.pr) / g.hop + 1 : 0;
  if (c.t_e > c.t_b) c.t_e = c.t_b;
  c.t_a = c.t_e > g.guard ? c.t_e - g.guard : 0;
  return c;
}

// patch[b][i] = audio[b][a_b + i] for a_b + i < L_b; behind the clip 0 -- with pre-emphasis the sequence v_0 = y[L_b - 1],
// v_k = rn(pre v_{k-1}) instead: the log-mel kernels form y[n] - rn(pre y[n-1]) on the row they are given, and the clip alone
// ends in zeros AFTER its pre-emphasis; on this tail every such difference is exactly 0 (a plain zero fill would put
// -pre y[L_b - 1] behind the clip's last sample).
__global__ __launch_bounds__(256) void ragged_gather_kernel(RaggedGeo g, const float* __restrict__ audio, int64_t stride,
                                                             const int64_t* __restrict__ lengths, float* __restrict__ patch,
                                                             float preemph) {
  const int chunks = (g.n_patch + 255) / 256;
  const int64_t b = blockIdx.x / chunks;
  const int i = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (i >= g.n_patch) return;
  const RaggedClip c = ragged_clip(g, lengths, b);
  const int64_t src = c.t_a * g.hop + i;
  float v = 0.0f;
  if (src < c.len) {
    v = audio[b * stride + src];
  } else if (preemph != 0.0f) {
    v = audio[b * stride + c.len - 1];
    for (int64_t k = src - c.len; k >= 0 && v != 0.0f; --k) v = __fmul_rn(preemph, v);
  }
  patch[b * g.n_patch + i] = v;
}

// logmel[b][m][t_a + t'] = patch_logmel[b][m][t'] for the edge frames t_e <= t_a + t' < t_b; a workgroup per clip
__global__ __launch_bounds__(256) void ragged_scatter_kernel(RaggedGeo g, const int64_t* __restrict__ lengths,
                                                              const float* __restrict__ patch_lm, float* __restrict__ logmel,
                                                              int n_mels) {
  const int64_t b = blockIdx.x;
  const RaggedClip c = ragged_clip(g, lengths, b);
  const int first = (int)(c.t_e - c.t_a);
  const int64_t avail = c.t_b - c.t_a;
  const int end = avail < g.t_patch ? (int)avail : g.t_patch;
  const int w = end - first;
  if (w <= 0) return;
  for (int e = threadIdx.x; e < n_mels * w; e += 256) {
    const int m = e / w, tp = first + (e - m * w);
    logmel[(b * n_mels + m) * g.t_max + c.t_a + tp] = patch_lm[(b * n_mels + m) * g.t_patch + tp];
  }
}

// key[b] = max over m < n_mels, t < t_b of logmel[b][m][t] as an ordered key (key[] preset to the lowest key).
// A workgroup takes MM_RAGGED_MAX_FRAMES frames of one clip: lane <-> frame, so every row read is coalesced.
#define MM_RAGGED_MAX_FRAMES 512
__global__ __launch_bounds__(256) void ragged_max_kernel(RaggedGeo g, const int64_t* __restrict__ lengths,
                                                          const float* __restrict__ logmel, int n_mels, int* __restrict__ key) {
  __shared__ float part[4];
  const int64_t chunks = (g.t_max + MM_RAGGED_MAX_FRAMES - 1) / MM_RAGGED_MAX_FRAMES;
  const int64_t b = blockIdx.x / chunks;
  const RaggedClip c = ragged_clip(g, lengths, b);
  const int64_t t0 = (blockIdx.x % chunks) * MM_RAGGED_MAX_FRAMES;
  if (t0 >= c.t_b) return;                                     // (workgroup-uniform)
  const int64_t t1 = t0 + MM_RAGGED_MAX_FRAMES < c.t_b ? t0 + MM_RAGGED_MAX_FRAMES : c.t_b;
  const float* lm = logmel + b * n_mels * g.t_max;
  float v = -INFINITY;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
    const float* col = lm + t;
    int m = 0;
    for (; m + 8 <= n_mels; m += 8) {                          // eight rows' loads in flight
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = col[(int64_t)(m + j) * g.t_max];
#pragma unroll
      for (int j = 0; j < 8; ++j) v = fmaxf(v, x[j]);
    }
    for (; m < n_mels; ++m) v = fmaxf(v, col[(int64_t)m * g.t_max]);
  }
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    if (v > -INFINITY) atomicMax(key + b, float_key(v));
  }
}

// dct_clamp_kernel (mm_api.hip) with the frame count read per clip: lane <-> frame, the DCT row wave-uniform; the
// columns t >= t_b of the [B][n_mfcc][t_max] output get 0.0f.
__global__ __launch_bounds__(256) void ragged_clamp_dct_kernel(RaggedGeo g, const int64_t* __restrict__ lengths,
                                                                const float* __restrict__ logmel, const int* __restrict__ key,
                                                                const float* __restrict__ dct_t /*[n_mels][KP]*/,
                                                                float* __restrict__ out, int n_mels, int n_mfcc, int kp,
                                                                float top_db) {
  const int64_t bpc = (g.t_max + 255) / 256;
  const int64_t b = blockIdx.x / bpc;
  const int64_t t = (blockIdx.x % bpc) * 256 + threadIdx.x;
  if (t >= g.t_max) return;
  const RaggedClip c = ragged_clip(g, lengths, b);
  float* o = out + b * n_mfcc * g.t_max + t;
  if (t >= c.t_b) {
    for (int k = 0; k < n_mfcc; ++k) o[(int64_t)k * g.t_max] = 0.0f;
    return;
  }
  const float thr = top_db >= 0.0f ? key_float(key[b]) - top_db : -INFINITY;
  const float* lm = logmel + b * n_mels * g.t_max + t;
  for (int k0 = 0; k0 < n_mfcc; k0 += MM_DCT_KB) {
    float acc[MM_DCT_KB];
#pragma unroll
    for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = 0.0f;
#pragma unroll 4
    for (int m = 0; m < n_mels; ++m) {
      const float x = fmaxf(lm[(int64_t)m * g.t_max], thr);
      const float* d = dct_t + (size_t)m * kp + k0;
#pragma unroll
      for (int kk = 0; kk < MM_DCT_KB; ++kk) acc[kk] = fmaf(d[kk], x, acc[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < MM_DCT_KB; ++kk)
      if (k0 + kk < n_mfcc) o[(int64_t)(k0 + kk) * g.t_max] = acc[kk];
  }
}

// The geometry of a call.  The patch row is as long as the longest stretch [a_b, L_b) any clip can have, and has as many
// frames as guard + the most edge frames a clip can have ("The edge patch", derives both bounds).
RaggedGeo ragged_geo(const mm_plan* p, int64_t n_samples) {
  const mm_config& c = p->cfg;
  RaggedGeo g;
  const bool embedded = p->embed.factor > 1;                   // n_fft 64 / 128 / 256 transformed as 512 points
  const int pl = embedded ? 256 : c.n_fft / 2, pr = embedded ? 256 : c.n_fft - c.n_fft / 2;
  g.n_samples = n_samples;
  g.t_max = mm_num_frames(&c, n_samples);
  g.hop = c.hop_length;
  g.pr = pr;
  g.odd = c.n_fft - 2 * (c.n_fft / 2);
  g.guard = (pl + (c.preemph != 0.0f ? 1 : 0) + g.hop - 1) / g.hop;
  const int64_t edge_max = (pr - g.odd) / g.hop + 1;
  const int64_t by_frames = (edge_max + g.guard - 1) * g.hop + g.odd, by_samples = (int64_t)pr + (int64_t)g.guard * g.hop;
  g.n_patch = (int)((std::max(by_frames, by_samples) + 3) / 4 * 4);   // (>= 4 and a multiple of 4: the plan's regular kernel takes it)
  g.t_patch = (int)mm_num_frames(&c, g.n_patch);
  return g;
}

// Workspace: main log-mel [B][n_mels][t_max] | patch rows [B][n_patch] | patch log-mel [B][n_mels][t_patch] |
// the log-mel entry's clip maxima [B] (not used) | max keys [B]
struct RaggedWs { size_t logmel, patch, patch_lm, clipmax, key, total; };
RaggedWs ragged_ws(const mm_plan* p, const RaggedGeo& g, int64_t batch) {
  RaggedWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
  w.logmel = take((size_t)batch * p->cfg.n_mels * g.t_max * 4);
  w.patch = take((size_t)batch * g.n_patch * 4);
  w.patch_lm = take((size_t)batch * p->cfg.n_mels * g.t_patch * 4);
  w.clipmax = take((size_t)batch * 4);
  w.key = take((size_t)batch * 4);
  w.total = off;
  return w;
}

}  // namespace

extern "C" {

size_t mm_ragged_workspace_bytes(const mm_plan* p, int64_t batch, int64_t n_samples) {
  if (!p || batch < 1 || n_samples < 1 || n_samples > MM_MAX_SAMPLES) return 0;
  return ragged_ws(p, ragged_geo(p, n_samples), batch).total;
}

int mm_mfcc_ragged_f32(mm_plan* p, const float* d_audio, int64_t batch, int64_t n_samples, int64_t stride,
                       const int64_t* d_lengths, float* d_mfcc, float* d_modspec, void* d_ws, size_t ws_bytes, void* stream) {
  if (!p || !d_audio || !d_lengths || !d_mfcc || !d_ws || batch < 1 || n_samples < 1 || stride < n_samples ||
      n_samples > MM_MAX_SAMPLES)
    return MM_ERR_INVALID_ARG;
  if (!(std::fabs(p->cfg.preemph) <= 1.0f)) return MM_ERR_UNSUPPORTED;   // the gather kernel's tail pre^k y[L - 1] must not grow
  const RaggedGeo g = ragged_geo(p, n_samples);
  const RaggedWs w = ragged_ws(p, g, batch);
  if (ws_bytes < w.total) return MM_ERR_WORKSPACE;
  if (d_modspec) {
    const int n_mod = mm_mod_fft_len(&p->cfg, g.t_max);
    if (n_mod < 0) return n_mod;
    if (n_mod > 8192) return MM_ERR_UNSUPPORTED;               // longer trajectories: mm_hilbert_rfft_f32 on d_mfcc
  }
  const int64_t bpc = (g.t_max + 255) / 256, max_chunks = (g.t_max + MM_RAGGED_MAX_FRAMES - 1) / MM_RAGGED_MAX_FRAMES;
  const int64_t patch_chunks = (g.n_patch + 255) / 256;
  if (batch * bpc > 0x7FFFFFFF || batch * patch_chunks > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;   // (grid limit; max_chunks <= bpc)
  hipStream_t st = (hipStream_t)stream;
  const mm_config& c = p->cfg;
  char* ws = (char*)d_ws;
  float *logmel = (float*)(ws + w.logmel), *patch = (float*)(ws + w.patch), *patch_lm = (float*)(ws + w.patch_lm);
  float* clipmax = (float*)(ws + w.clipmax);
  int* key = (int*)(ws + w.key);

  // main pass on the audio as it lies, then the patch rows through the same entry
  int rc = mm_logmel_f32(p, d_audio, batch, n_samples, stride, logmel, clipmax, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(ragged_gather_kernel, dim3((unsigned)(batch * patch_chunks)), dim3(256), 0, st, g,
                     d_audio, stride, d_lengths, patch, c.preemph);
  HIP_TRY(hipGetLastError());
  rc = mm_logmel_f32(p, patch, batch, g.n_patch, g.n_patch, patch_lm, clipmax, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(ragged_scatter_kernel, dim3((unsigned)batch), dim3(256), 0, st, g, d_lengths, patch_lm, logmel, c.n_mels);
  HIP_TRY(hipGetLastError());
  {
    StageTimer tm(p, MM_STAGE_DCT, st);
    if (c.top_db >= 0.0f) {
      fill_words(key, MM_KEY_UNSET, batch, st);
      hipLaunchKernelGGL(ragged_max_kernel, dim3((unsigned)(batch * max_chunks)), dim3(256), 0, st, g, d_lengths, logmel,
                         c.n_mels, key);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ragged_clamp_dct_kernel, dim3((unsigned)(batch * bpc)), dim3(256), 0, st, g, d_lengths, logmel, key,
                       p->base.d_dct_t, d_mfcc, c.n_mels, c.n_mfcc, p->kp, c.top_db);
    HIP_TRY(hipGetLastError());
  }
  if (d_modspec) return mm_modspec_f32(p, d_mfcc, batch, g.t_max, d_modspec, stream);
  return MM_OK;
}

}  // extern "C"
