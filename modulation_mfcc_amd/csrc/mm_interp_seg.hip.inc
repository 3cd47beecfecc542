// What the segmented NaN-interpolation units share (mm_interp.hip, mm_spline.hip): the segment size, the load of a
// segment with its validity ballots, the sample count of a row, the search of the ballots for a valid neighbour; on the
// host the workspace alignment, the segment count and the shape limit.
#pragma once

namespace {

constexpr int kIpThreads = 256;
constexpr int kIpPer = 4;                               // samples per thread, strided by the workgroup
constexpr int kIpSeg = kIpThreads * kIpPer;             // samples per segment = workgroup (interp.INTERP_SEGMENT)
constexpr int kIpWords = kIpSeg / 64;                   // ballots per segment
constexpr int64_t kIpMaxN = 0x7fffffff - kIpSeg;        // indices are int32, the segment's end included

// The segment's samples of this thread (NaN beyond the row's end) and the validity ballots of the whole segment in LDS.
__device__ __forceinline__ void ip_load_segment(const double* __restrict__ xr, int64_t n, int64_t base, double (&v)[kIpPer],
                                                uint64_t* s_m) {
#pragma unroll
  for (int k = 0; k < kIpPer; ++k) {
    const int64_t i = base + k * kIpThreads + threadIdx.x;
    v[k] = i < n ? xr[i] : NAN;
    const uint64_t m = __ballot(v[k] == v[k]);
    if ((threadIdx.x & 63) == 0) s_m[k * (kIpThreads / 64) + (threadIdx.x >> 6)] = m;
  }
  __syncthreads();
}

// The samples of a row: all n_max of it, or its first clamp(counts[row], 1, n_max) (the ragged entry point).  What lies
// behind the count is no sample: never valid, never an end of the curve, and written as 0.
__device__ __forceinline__ int64_t ip_row_count(const int64_t* __restrict__ counts, int64_t row, int64_t n_max) {
  return counts ? min<int64_t>(max<int64_t>(counts[row], 1), n_max) : n_max;
}

// last valid sample of the segment before local index j / first one after it; -1 when there is none
__device__ __forceinline__ int ip_seg_prev(const uint64_t* s_m, int j) {
  int w = j >> 6;
  uint64_t bits = s_m[w] & ((1ull << (j & 63)) - 1ull);
  while (bits == 0 && w > 0) bits = s_m[--w];
  return bits ? (w << 6) + 63 - __clzll((long long)bits) : -1;
}
__device__ __forceinline__ int ip_seg_next(const uint64_t* s_m, int j) {
  int w = j >> 6;
  const int b = j & 63;
  uint64_t bits = b == 63 ? 0ull : s_m[w] & (~0ull << (b + 1));
  while (bits == 0 && w < kIpWords - 1) bits = s_m[++w];
  return bits ? (w << 6) + __ffsll((unsigned long long)bits) - 1 : -1;
}

// host: a workspace part's size (parts start on 256 bytes), the segments of a row, and the shapes the units take -- rows
// and rows x segments are grid sizes, a sample's index is an int32
size_t ip_align(size_t v) { return (v + 255) / 256 * 256; }
int64_t ip_nseg(int64_t n) { return (n + kIpSeg - 1) / kIpSeg; }
bool ip_shape_ok(int64_t rows, int64_t n) {
  return rows >= 1 && rows <= 0x7fffffff && n >= 1 && n <= kIpMaxN && rows * ip_nseg(n) <= 0x7fffffff;
}

}  // namespace
