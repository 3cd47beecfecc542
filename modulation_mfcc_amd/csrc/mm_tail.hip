// libmodmfcc: the rows after the MFCCs (SURVEY.md 8(f) N1, N2 and the 'iir' filter of N3) -- the MFCC-change tail of
// script/mfcc.py:392-427 in its three device forms, scipy.signal.sosfiltfilt on batches of curves, the banded stencil
// operator behind get_velocity (script/calc.py:593-650) and the 'sg' / 'fir' output filters.  gfx950 only.
#include "mm_common.h"
#include "mm_plan.h"

#include "mm_sos.hip.inc"           // the filter, the cascade step, the tables / lane scan / upload of the time-parallel forms
#include "mm_sos_tm.hip.inc"        // sosfiltfilt on a time-major workspace (any section count)
#include "mm_sos_rows.hip.inc"      // sosfiltfilt on segmented rows (up to MM_SCAN_MAX_SEC sections)
#include "mm_change.hip.inc"        // the change tail: derivative + norm kernels, the segmented form
#include "mm_change_clip.hip.inc"   // the change tail as one clip-resident launch
#include "mm_stencil.hip.inc"       // the banded stencil

static int change_pads(int n_sec1, const double* sos1, int n_sec2, const double* sos2, SosFilt* f1, SosFilt* f2) {
  int rc = make_sosfilt(sos1, n_sec1, f1);
  if (rc) return rc;
  if (n_sec1 < 1) return MM_ERR_INVALID_ARG;
  return make_sosfilt(sos2, n_sec2, f2);
}

static int64_t round64(int64_t v) { return (v + 63) / 64 * 64; }

// Which of the three device forms a change-tail call takes, and the workspace (in doubles) THAT form needs -- one
// routine for the size query and for the call, so the two cannot disagree.
enum { MM_CHG_TIME_MAJOR = 0, MM_CHG_CLIP = 1, MM_CHG_SEGMENTED = 2 };
struct ChgForm { int form; size_t need; ClipShape cs; };
static ChgForm change_form(const mm_plan* p, int64_t batch, int64_t n_frames, int n_rows, const SosFilt& f1, const SosFilt& f2) {
  ChgForm r;
  const int64_t p1 = f1.padlen, p2 = f2.n_sec > 0 ? f2.padlen : 0;
  const int64_t n1 = n_frames + 2 * p1, n2 = n_frames + 2 * p2;
  r.cs = clip_shape(n_rows, n1, n2);
  const bool small_sec = f1.n_sec <= MM_SCAN_MAX_SEC && f2.n_sec <= MM_SCAN_MAX_SEC;
  // Long clips (one recording at a 1 ms step is 10 001 frames per ten seconds): the clip form holds fewer and fewer rows
  // at once and walks its groups one after the other -- from five groups on (about 5000 frames at 12 rows) a wave per
  // 1088 samples of a row (mm_sos_rows.hip.inc) is faster at every clip count (tools/chg_forms.py: 8001 frames 0.80 ms
  // against 0.11 - 0.45 ms for 1 - 256 clips; 4001 frames, three groups: 0.12 against 0.11 - 0.27 ms)
  bool few_long = r.cs.G >= 1 && (n_rows + r.cs.G - 1) / r.cs.G > 4;
#ifdef MM_DEV
  if (const char* e = getenv("MM_CHG_FORM")) few_long = e[0] == 's';      // side build only: A/B of the two forms (tools/chg_forms.py)
#endif
  if (!p->user.no_fuse_tail && small_sec && (r.cs.G < 1 || few_long)) {
    r.form = MM_CHG_SEGMENTED;
    r.need = chg_seg_workspace_doubles(batch, n_rows, n_frames, (int)p1, (int)p2);
  } else if (!p->user.no_fuse_tail && small_sec && r.cs.G >= 1) {
    r.form = MM_CHG_CLIP;
    r.need = (size_t)r.cs.tab_n;        // filter tables only (a few KB): the clip lives in LDS
  } else {
    r.form = MM_CHG_TIME_MAJOR;         // two time-major buffers [T + 2 pad][columns padded to 64]
    r.need = (size_t)n1 * (size_t)round64(batch * n_rows) + (size_t)n2 * (size_t)round64(batch);
  }
  return r;
}

// ---- ragged batches: one frame count per clip (include/modmfcc.h) ----
// The clip-resident kernel alone, shaped for the longest clip: chunk tables, K1 / K2, row groups and LDS follow from
// n_frames_max, a workgroup reads its own length.  No other form: more than MM_SCAN_MAX_SEC sections or a clip whose single row
// does not fit LDS is MM_ERR_UNSUPPORTED, whatever mm_plan_set_fuse_tail() says.
static bool change_ragged_shape(int n_rows, int64_t n_frames_max, const SosFilt& f1, const SosFilt& f2, ClipShape* cs) {
  const int64_t p1 = f1.padlen, p2 = f2.n_sec > 0 ? f2.padlen : 0;
  *cs = clip_shape(n_rows, n_frames_max + 2 * p1, n_frames_max + 2 * p2);
  return f1.n_sec <= MM_SCAN_MAX_SEC && f2.n_sec <= MM_SCAN_MAX_SEC && cs->G >= 1;
}

// Both change entries: the arguments checked, the two filters made and ChangeParams filled for batch clips of n_frames
// (ragged: the longest clip's); q.ws2 is left to the time-major form
static int change_setup(const mm_plan* p, const float* d_mfcc, int64_t batch, int64_t n_frames, int32_t remove_first,
                        int32_t diff_method, const double* sos1, int32_t n_sec1, const double* sos2, int32_t n_sec2,
                        double* d_change, void* d_ws, SosFilt* f1, SosFilt* f2, ChangeParams* q) {
  if (!p || !d_mfcc || !d_change || !d_ws || batch < 1 || n_frames < 1) return MM_ERR_INVALID_ARG;
  if (diff_method < 0 || diff_method > 1 || (diff_method == 1 && n_frames < 3)) return MM_ERR_INVALID_ARG;
  if (remove_first < 0 || remove_first >= p->cfg.n_mfcc) return MM_ERR_INVALID_ARG;
  if (batch > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  const int rc = change_pads(n_sec1, sos1, n_sec2, sos2, f1, f2);
  if (rc) return rc;
  // scipy: "The length of the input vector x must be greater than padlen" (ragged: what the host can know -- not even
  // the longest clip is one scipy takes; a shorter one comes out NaN, on the device)
  if (n_frames <= f1->padlen || n_frames <= f2->padlen) return MM_ERR_INVALID_ARG;
  q->mfcc = d_mfcc; q->n_frames = n_frames; q->batch = batch; q->n_mfcc = p->cfg.n_mfcc;
  q->first_row = remove_first ? 1 : 0; q->n_rows = q->n_mfcc - q->first_row;
  q->p1 = f1->padlen; q->p2 = f2->n_sec > 0 ? f2->padlen : 0; q->sg = diff_method;
  q->R = batch * q->n_rows; q->Rp = round64(q->R); q->Bp = round64(batch);
  q->ws1 = (double*)d_ws; q->ws2 = nullptr; q->out = d_change;
  return MM_OK;
}

static size_t sosfiltfilt_workspace_doubles(int64_t rows, int64_t n, bool ragged) {
  const size_t sg = seg_workspace_doubles(rows, n, 3 * (2 * MM_SCAN_MAX_SEC + 1));
  if (ragged) return sg;                                  // the segmented rows only
  // the larger of the two device forms: time-major [n + 2 pad][rows padded to 64] | segmented rows (mm_sos_rows.hip.inc)
  return std::max((size_t)(n + 2 * 3 * (2 * MM_MAX_SEC + 1)) * (size_t)round64(rows), sg);
}

// d_x (float64 rows) or d_xf (float32 rows: odd extension in float32 arithmetic, see odd_ext_f32)
// d_lens (DEVICE int64 [rows], or null): the ragged form, n the longest row's length
static int sosfiltfilt_impl(const double* d_x, const float* d_xf, int64_t rows, int64_t n, int64_t x_stride, const int64_t* d_lens,
                            const double* sos, int32_t n_sec, double* d_y, void* d_ws, size_t ws_bytes, void* stream) {
  if ((!d_x && !d_xf) || !d_y || !d_ws || rows < 1 || n < 1 || x_stride < n || n_sec < 1) return MM_ERR_INVALID_ARG;
  SosFilt f;
  int rc = make_sosfilt(sos, n_sec, &f);
  if (rc) return rc;
  if (d_lens && f.n_sec > MM_SCAN_MAX_SEC) return MM_ERR_UNSUPPORTED;    // the time-major kernels stay single-length
  // scipy: "The length of the input vector x must be greater than padlen" (ragged: what the host can know -- not even
  // the longest row is one scipy takes; a shorter one comes out NaN, on the device)
  if (n <= f.padlen) return MM_ERR_INVALID_ARG;
  if (ws_bytes < sosfiltfilt_workspace_doubles(rows, n, d_lens != nullptr) * sizeof(double)) return MM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (f.n_sec <= MM_SCAN_MAX_SEC) {     // segmented rows: a wave per 1088 samples of a row, any length
    const SegSrc src = {d_x, x_stride, d_xf, 0, 0, 0};
    rc = launch_sos_rows_any(f, src, rows, n, d_y, (double*)d_ws, st, d_lens);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MM_OK;
  }
  const int64_t Wp = round64(rows), tb = (n + 63) / 64;
  if (tb > 65535 || Wp / 64 > 0x7FFFFFFF || 2 * (int64_t)f.padlen * Wp / 256 + 1 > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  double* ws = (double*)d_ws;
  const dim3 grid((unsigned)(Wp / 64), (unsigned)tb);
  if (d_xf)
    hipLaunchKernelGGL((tm_pack_kernel<PlainRows<float>>), grid, dim3(256), 0, st, PlainRows<float>{d_xf, x_stride}, rows, n,
                       f.padlen, Wp, ws);
  else
    hipLaunchKernelGGL((tm_pack_kernel<PlainRows<double>>), grid, dim3(256), 0, st, PlainRows<double>{d_x, x_stride}, rows, n,
                       f.padlen, Wp, ws);
  hipLaunchKernelGGL(chg_pad_kernel, dim3((unsigned)((2 * (int64_t)f.padlen * Wp + 255) / 256)), dim3(256), 0, st, ws, n,
                     f.padlen, Wp, d_xf ? 1 : 0);
  launch_sos_any(f, ws, n + 2 * f.padlen, Wp, st);
  hipLaunchKernelGGL(tm_unpack_kernel, grid, dim3(256), 0, st, ws, rows, n, f.padlen, Wp, d_y);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

extern "C" {

// Upper bound over the three forms and every filter of up to MM_MAX_SEC sections (a caller that does not know its
// filters yet); mm_change_workspace_bytes_for() sizes the form a given call takes.
size_t mm_change_workspace_bytes(const mm_plan* p, int64_t batch, int64_t n_frames) {
  if (!p || batch < 1 || n_frames < 1) return 0;
  // two time-major buffers [T + 2 pad][columns padded to 64]; worst-case padding 3 * (2 * MM_MAX_SEC + 1)
  const int64_t padmax = 3 * (2 * MM_MAX_SEC + 1);
  const int64_t n = n_frames + 2 * padmax;
  const size_t tm = (size_t)n * (size_t)(round64(batch * p->cfg.n_mfcc) + round64(batch));
  // ... or the segmented rows' buffers (mm_sos_rows.hip.inc), whichever is larger
  const int pads = 3 * (2 * MM_SCAN_MAX_SEC + 1);
  const size_t sg = chg_seg_workspace_doubles(batch, p->cfg.n_mfcc, n_frames, pads, pads);
  return std::max(tm, sg) * sizeof(double);
}

size_t mm_change_workspace_bytes_for(const mm_plan* p, int64_t batch, int64_t n_frames, int32_t remove_first, const double* sos1,
                                     int32_t n_sec1, const double* sos2, int32_t n_sec2) {
  if (!p || batch < 1 || n_frames < 1 || remove_first < 0 || remove_first >= p->cfg.n_mfcc) return 0;
  SosFilt f1, f2;
  if (change_pads(n_sec1, sos1, n_sec2, sos2, &f1, &f2)) return 0;
  const int n_rows = p->cfg.n_mfcc - (remove_first ? 1 : 0);
  return std::max<size_t>(change_form(p, batch, n_frames, n_rows, f1, f2).need, 1) * sizeof(double);
}

int mm_mfcc_change_f64(mm_plan* p, const float* d_mfcc, int64_t batch, int64_t n_frames,
                       int32_t remove_first, int32_t diff_method, const double* sos1, int32_t n_sec1, const double* sos2,
                       int32_t n_sec2, double* d_change, void* d_ws, size_t ws_bytes, void* stream) {
  SosFilt f1, f2;
  ChangeParams q;
  int rc = change_setup(p, d_mfcc, batch, n_frames, remove_first, diff_method, sos1, n_sec1, sos2, n_sec2, d_change, d_ws, &f1, &f2, &q);
  if (rc) return rc;
  const int64_t n1 = n_frames + 2 * q.p1, n2 = n_frames + 2 * q.p2;
  // the workspace of the form that runs (mm_change_workspace_bytes_for); mm_change_workspace_bytes is the bound over all forms
  const ChgForm cf = change_form(p, batch, n_frames, q.n_rows, f1, f2);
  if (ws_bytes < cf.need * sizeof(double)) return MM_ERR_WORKSPACE;
  q.ws2 = q.ws1 + n1 * q.Rp;
  const int64_t tblocks = (n_frames + 63) / 64;
  if (tblocks > 65535 || 2 * (int64_t)q.p1 * q.Rp / 256 + 1 > 0x7FFFFFFF || n_frames * q.Bp / 256 + 1 > 0x7FFFFFFF ||
      q.Bp / 64 > 65535 || n_frames > 0x7FFFFFFF)
    return MM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  StageTimer tm(p, MM_STAGE_CHANGE, st);
  if (cf.form == MM_CHG_SEGMENTED) {       // mm_sos_rows.hip.inc: a wave per 1088 samples of a row
    rc = launch_chg_segmented(q, f1, f2, q.ws1, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MM_OK;
  }
  if (cf.form == MM_CHG_CLIP) {            // mm_change_clip.hip.inc: one launch, no workspace traffic
    rc = with_scan_sections(std::max(f1.n_sec, f2.n_sec), [&](auto ns) {
      return launch_chg_clip<decltype(ns)::value>(q, f1, f2, cf.cs, n1, n2, q.ws1, st);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MM_OK;
  }
  const dim3 rows_grid((unsigned)(q.Rp / 64), (unsigned)tblocks), curve_grid((unsigned)(q.Bp / 64), (unsigned)tblocks);
  hipLaunchKernelGGL(tm_pack_kernel<MfccRows>, rows_grid, dim3(256), 0, st,
                     MfccRows{q.mfcc, q.n_mfcc, q.first_row, q.n_rows, n_frames}, q.R, n_frames, q.p1, q.Rp, q.ws1);
  hipLaunchKernelGGL(chg_pad_kernel, dim3((unsigned)((2 * (int64_t)q.p1 * q.Rp + 255) / 256)), dim3(256), 0, st,
                     q.ws1, n_frames, q.p1, q.Rp, 1);
  launch_sos_any(f1, q.ws1, n1, q.Rp, st);
  if (q.n_rows <= MM_CHG_MAXROWS)
    hipLaunchKernelGGL(chg_norm_kernel, dim3((unsigned)n_frames, (unsigned)(q.Bp / 64)), dim3(256), 0, st, q);
  else
    hipLaunchKernelGGL(chg_norm_rows_kernel, dim3((unsigned)((n_frames * q.Bp + 255) / 256)), dim3(256), 0, st, q);
  if (f2.n_sec > 0) {
    hipLaunchKernelGGL(chg_pad_kernel, dim3((unsigned)((2 * (int64_t)q.p2 * q.Bp + 255) / 256)), dim3(256), 0, st,
                       q.ws2, n_frames, q.p2, q.Bp, 0);
    launch_sos_any(f2, q.ws2, n2, q.Bp, st);
  }
  hipLaunchKernelGGL(tm_unpack_kernel, curve_grid, dim3(256), 0, st, q.ws2, batch, n_frames, q.p2, q.Bp, q.out);
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

size_t mm_change_ragged_workspace_bytes_for(const mm_plan* p, int64_t batch, int64_t n_frames_max, int32_t remove_first,
                                            const double* sos1, int32_t n_sec1, const double* sos2, int32_t n_sec2) {
  if (!p || batch < 1 || n_frames_max < 1 || n_frames_max > 0x7FFFFFFF || remove_first < 0 || remove_first >= p->cfg.n_mfcc)
    return 0;
  SosFilt f1, f2;
  if (change_pads(n_sec1, sos1, n_sec2, sos2, &f1, &f2)) return 0;
  ClipShape cs;
  // (a call the ragged entry answers with MM_ERR_UNSUPPORTED needs nothing: one double, so that a caller has a buffer to pass)
  const bool ok = change_ragged_shape(p->cfg.n_mfcc - (remove_first ? 1 : 0), n_frames_max, f1, f2, &cs);
  return std::max<size_t>(ok ? (size_t)cs.tab_n : 0, 1) * sizeof(double);
}

int mm_mfcc_change_ragged_f64(mm_plan* p, const float* d_mfcc, int64_t batch, int64_t n_frames_max, const int64_t* d_frames,
                              int32_t remove_first, int32_t diff_method, const double* sos1, int32_t n_sec1,
                              const double* sos2, int32_t n_sec2, double* d_change, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_frames || n_frames_max > 0x7FFFFFFF) return MM_ERR_INVALID_ARG;
  SosFilt f1, f2;
  ChangeParams q;
  int rc = change_setup(p, d_mfcc, batch, n_frames_max, remove_first, diff_method, sos1, n_sec1, sos2, n_sec2, d_change, d_ws, &f1, &f2, &q);
  if (rc) return rc;
  ClipShape cs;
  if (!change_ragged_shape(q.n_rows, n_frames_max, f1, f2, &cs)) return MM_ERR_UNSUPPORTED;
  if (ws_bytes < (size_t)cs.tab_n * sizeof(double)) return MM_ERR_WORKSPACE;
  const int64_t n1 = n_frames_max + 2 * q.p1, n2 = n_frames_max + 2 * q.p2;
  hipStream_t st = (hipStream_t)stream;
  StageTimer tm(p, MM_STAGE_CHANGE, st);
  rc = with_scan_sections(std::max(f1.n_sec, f2.n_sec), [&](auto ns) {
    return launch_chg_clip<decltype(ns)::value, true>(q, f1, f2, cs, n1, n2, q.ws1, st, d_frames);
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return MM_OK;
}

size_t mm_sosfiltfilt_workspace_bytes(int64_t rows, int64_t n) {
  return rows < 1 || n < 1 ? 0 : sosfiltfilt_workspace_doubles(rows, n, false) * sizeof(double);
}

int mm_sosfiltfilt_f64(const double* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* sos, int32_t n_sec,
                       double* d_y, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x) return MM_ERR_INVALID_ARG;
  return sosfiltfilt_impl(d_x, nullptr, rows, n, x_stride, nullptr, sos, n_sec, d_y, d_ws, ws_bytes, stream);
}

int mm_sosfiltfilt_f32_f64(const float* d_x, int64_t rows, int64_t n, int64_t x_stride, const double* sos, int32_t n_sec,
                           double* d_y, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x) return MM_ERR_INVALID_ARG;
  return sosfiltfilt_impl(nullptr, d_x, rows, n, x_stride, nullptr, sos, n_sec, d_y, d_ws, ws_bytes, stream);
}

int mm_stencil_f64(const mm_stencil* st, const double* d_x, int64_t rows, int64_t n, int64_t x_stride, double* d_y,
                   void* stream) {
  return stencil_impl(st, d_x, rows, n, x_stride, nullptr, d_y, stream);
}

int mm_stencil_ragged_f64(const mm_stencil* st, const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride,
                          const int64_t* d_lens, double* d_y, void* stream) {
  if (!d_lens) return MM_ERR_INVALID_ARG;
  return stencil_impl(st, d_x, rows, n_max, x_stride, d_lens, d_y, stream);
}

size_t mm_sosfiltfilt_ragged_workspace_bytes(int64_t rows, int64_t n_max) {
  return rows < 1 || n_max < 1 ? 0 : sosfiltfilt_workspace_doubles(rows, n_max, true) * sizeof(double);
}

int mm_sosfiltfilt_ragged_f64(const double* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                              const double* sos, int32_t n_sec, double* d_y, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x || !d_lens) return MM_ERR_INVALID_ARG;
  return sosfiltfilt_impl(d_x, nullptr, rows, n_max, x_stride, d_lens, sos, n_sec, d_y, d_ws, ws_bytes, stream);
}

int mm_sosfiltfilt_ragged_f32_f64(const float* d_x, int64_t rows, int64_t n_max, int64_t x_stride, const int64_t* d_lens,
                                  const double* sos, int32_t n_sec, double* d_y, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_x || !d_lens) return MM_ERR_INVALID_ARG;
  return sosfiltfilt_impl(nullptr, d_x, rows, n_max, x_stride, d_lens, sos, n_sec, d_y, d_ws, ws_bytes, stream);
}

}  // extern "C"
