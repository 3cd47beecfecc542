#pragma once
// ------------------------------------------------------------------------------------------
// Banded linear operator along time on [rows][n] float64 rows -- the derivative transforms of
// get_velocity (script/calc.py:593-650; SURVEY.md 8(f) row N2): np.gradient (repeated), Savitzky-Golay
// derivative with mode='interp' (interior = correlation with savgol_coeffs, first / last half-window
// samples = derivative of the polynomial fitted to the first / last window), findiff central stencils
// with one-sided stencils at the ends.  All of them are: interior y[i] = (sum_k c[k] x[i + off[k]]) /
// den_c, and for the n_edge first / last outputs a dense row over the first / last edge_w inputs.
// One thread per output sample; the taps travel in the kernel argument.
// ------------------------------------------------------------------------------------------
// RAGGED: a length per row (lens, DEVICE int64 [rows], clamped into [1, n_max]); the right edge rows sit at the row's own
// end, nothing at or behind it is loaded, the columns behind it become +0.0, and a row too short for the operator NaN.
template <bool RAGGED>
__global__ __launch_bounds__(256) void stencil_kernel(mm_stencil st, const double* __restrict__ x, int64_t rows,
                                                      int64_t n_max, int64_t in_stride, const int64_t* __restrict__ lens,
                                                      double* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * n_max) return;
  const int64_t r = idx / n_max, i = idx - r * n_max;
  int64_t n = n_max;
  if constexpr (RAGGED) {
    const int64_t nb = lens[r];
    n = nb < 1 ? 1 : (nb > n_max ? n_max : nb);
    if (i >= n) { y[idx] = 0.0; return; }
    // (st.reserved: the caller's own minimum, e.g. filtfilt's 3 n_taps + 1, where it exceeds the operator's)
    if (n < 2 * (int64_t)st.n_edge || n < st.edge_w || n < st.reserved) { y[idx] = __builtin_nan(""); return; }
  }
  const double* xr = x + r * in_stride;
  double acc = 0.0, den;
  if (i < st.n_edge) {
    for (int j = 0; j < st.edge_w; ++j) acc = fma(st.el[i][j], xr[j], acc);
    den = st.den_e;
  } else if (i >= n - st.n_edge) {
    const int e = (int)(i - (n - st.n_edge));
    for (int j = 0; j < st.edge_w; ++j) acc = fma(st.er[e][j], xr[n - st.edge_w + j], acc);
    den = st.den_e;
  } else {
    for (int k = 0; k < st.n_c; ++k) acc = fma(st.c[k], xr[i + st.off[k]], acc);
    den = st.den_c;
  }
  y[idx] = acc / den;
}

// d_lens (DEVICE int64 [rows], or null): the ragged form, n the longest row's length
static int stencil_impl(const mm_stencil* st, const double* d_x, int64_t rows, int64_t n, int64_t x_stride,
                        const int64_t* d_lens, double* d_y, void* stream) {
  if (!st || !d_x || !d_y || rows < 1 || n < 1 || x_stride < n) return MM_ERR_INVALID_ARG;
  if (st->n_c < 1 || st->n_c > MM_ST_MAXW || st->n_edge < 0 || st->n_edge > MM_ST_MAXE || st->edge_w < 0 ||
      st->edge_w > MM_ST_MAXW || (st->n_edge > 0 && st->edge_w < 1) || st->den_c == 0.0 ||
      (st->n_edge > 0 && st->den_e == 0.0))
    return MM_ERR_INVALID_ARG;
  int lo = 0, hi = 0;
  for (int k = 0; k < st->n_c; ++k) { lo = std::min(lo, st->off[k]); hi = std::max(hi, st->off[k]); }
  // every interior output must find its taps inside the row, the edge rows their inputs
  if (n < 2 * (int64_t)st->n_edge || n < st->edge_w || -lo > st->n_edge || hi > st->n_edge) return MM_ERR_INVALID_ARG;
  const int64_t total = rows * n;
  if ((total + 255) / 256 > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  if (d_lens)
    hipLaunchKernelGGL(stencil_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *st,
                       d_x, rows, n, x_stride, d_lens, d_y);
  else
    hipLaunchKernelGGL(stencil_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *st,
                       d_x, rows, n, x_stride, d_lens, d_y);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}
