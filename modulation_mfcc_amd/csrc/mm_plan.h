// struct mm_plan (the MFCC plan behind include/modmfcc.h) and the per-stage event timer: shared by mm_api.hip (which
// creates and runs plans) and mm_tail.hip (whose change tail reads the plan's configuration and timing state).
#pragma once
#include "mm_common.h"

// any-length STFT (mm_anyfft.hip.inc): host-side description of the transform of an n_fft that is not a power of two
struct AnyPlan {
  int nn = 0, packed = 0, n_pass = 0, radix[16] = {0}, M = 0, log2M = 0, tpf = 64;
  unsigned grp_bytes = 0, b_off = 0, p_off = 0;
  float2 *d_tw = nullptr, *d_split = nullptr, *d_chirp = nullptr, *d_bhat = nullptr;
  // LDSTAB: packed constant tables (window | tw | split | chirp | mel_w | mel_start | mel_len | mel_off)
  float* d_tabpack = nullptr;
  int tab_floats = 0, o_tw = 0, o_split = 0, o_chirp = 0, o_melw = 0, o_mstart = 0, o_mlen = 0, o_moff = 0;
  bool lds_tab = false;
  bool ok = false;
  int fb = 0;                    // > 0: the batched kernel (stft_anyb_kernel) with this many frames per wave at once
  int reg2 = 0, reg2_r2 = 0;     // > 0: the two-stage register kernel (mm_reg2.hip), nn = reg2 x reg2_r2
  unsigned fb_grp_bytes = 0;     // its LDS bytes per wave: two buffers of fb x nn complex points
};

// 12-wave matrix-pipe variant (mm_logmel12m.hip.inc): unit lists kept in the plan
#define MM_M12_MW 4             // mel waves
#define MM_M12_UMAX 12          // units per mel wave

#define MM_MAX_TIMED 16384
#define MM_MAX_SAMPLES (((int64_t)1 << 29) - 8192)

// Plan state, one part per kernel family (filled by the set-up functions of mm_plan_create, read by the launchers of
// launch_stft).  A family whose `ok` stays false is not used.  The plan owns every device table: upload() records each
// allocation and the destructor frees them.
struct mm_plan {
  mm_config cfg{};
  int device = 0;
  int n_bins = 0, log2nc = 0, kp = 0;
  float db_offset = 0.0f;
  int num_cus = 256;

  struct Base {                    // generic STFT, clamp + DCT, rFFT: every plan has these tables
    float *d_window = nullptr, *d_mel_w = nullptr, *d_dct_t = nullptr;   // d_dct_t: [n_mels][kp]
    float2* d_tw = nullptr;
    int *d_mel_start = nullptr, *d_mel_len = nullptr, *d_mel_off = nullptr;
  } base;
  // n_fft < 512 embedded in the 512-point kernels: the window centred in 512, factor 512 / n_fft (else 1)
  struct Embed { float* d_window = nullptr; int factor = 1; } embed;
  struct W8 {                      // logmel512_kernel: mel run table (headers + groups) and wave parts
    bool ok = false; float* d_tab = nullptr; int* d_part = nullptr;
    int n_runs = 0, n_tab16 = 0; size_t lds_bytes = 0;
  } w8;
  struct W16 {                     // logmel512w_kernel: its own 16-way run table + per-lane records
    bool ok = false; float *d_tab = nullptr, *d_lane_tab = nullptr; int* d_part = nullptr;
    int n_runs = 0, n_tab16 = 0; size_t lds_bytes = 0;
  } w16;
  struct H16 {                     // 32-frame-tile / two-workgroup experiment (mm_logmel16h.hip.inc)
    bool ok = false; float* d_tab = nullptr; int* d_part = nullptr;
    int n_pairs = 0, n_tab16 = 0; size_t lds_bytes = 0;
  } h16;
  struct S16 {                     // staged-sample variant (mm_logmel16s.hip.inc), on the W16 tables
    int nr = 0;                    // 16-byte groups per thread and tile (0: not usable)
    bool xa = false;               // its ds_write_addtid_b32 exchange (NR 3 / 4, when the plan's LDS layout allows: mm_s16.h)
    bool halfwin = false;          // the 512-point window is zero outside [128, 384): the kernel prunes its first stage
    size_t lds_bytes = 0;
  } s16;
  struct S16F {                    // the staged-sample variant with the (unclamped) DCT fused in: its own run table (four
    bool ok = false;               // half-size parts for the DCT waves), DCT A operands, LDS layout
    float *d_tab = nullptr, *d_dcta = nullptr; int* d_part = nullptr;
    int n_runs = 0, n_tab16 = 0, lt_rows = 0, nk = 0, kb = 0;
    int flags = 0;                 // Logmel512Params::dct_flags (MM_S16F_SINGLE | MM_S16F_SKIP)
    unsigned lt_off = 0, dcta_off = 0, red_off = 0;   // red_off: clip mode's per-wave clip max / min slots
    unsigned long long roles = 0; size_t lds_bytes = 0;
    struct Shared {                // the same plan on the shared-runs table (mm::build_mel_runs_shared): two log-mel tiles and
      bool ok = false;             // no empty filters only; DCT operands, flags and row counts are those above
      float* d_tab = nullptr; int* d_part = nullptr;
      int n_runs = 0, n_tab16 = 0;
      unsigned lt_off = 0, dcta_off = 0, red_off = 0;
      unsigned long long roles = 0; size_t lds_bytes = 0;
    } sh;
  } s16f;
  struct M12 {                     // 12-wave MFMA-mel variant (mm_logmel12m.hip.inc)
    bool ok = false, fused_dct = false;
    float *d_a = nullptr, *d_dct = nullptr, *d_zeros = nullptr;
    int units[MM_M12_MW * MM_M12_UMAX * 4] = {}, n_units[8] = {};
    int nb = 0, nr = 0, s_floats = 0, n_a2 = 0;
    unsigned win_off = 0, tw_off = 0, a_off = 0, dct_off = 0, part_off = 0, cnt_off = 0;
    size_t lds_bytes = 0;
  } m12;
  struct Wpf {                     // wave-per-frame-group kernel (n_fft 512 / 1024 / 2048)
    bool ok = false; float *d_lane_tab = nullptr, *d_mel_lane = nullptr;
    int r = 0, waves = 0, group_max = 0; size_t lds_bytes = 0;
    bool w16 = false; size_t lds16 = 0;         // sixteen-wave form (W16): whether it applies, its LDS bytes
    bool half = false; int pairs = 0;           // the mel bank reads no bin >= NC / 2: split pairs the kernel forms (NI)
    int waves_half = 0; size_t lds_half = 0;    // launch geometry of the half-band instantiations (up to sixteen waves)
    int z = 0;                     // 3 / 5 / 6 / 7: the window is zero for a lane's first and last Z pairs (logmel_wpf_kernel<.., Z>)
  } wpf;
  struct DctFm {                   // clamp + DCT of the frame-major rows on the matrix pipe
    float* d_wave_a = nullptr;     // A operands [kb][wave_nk][64] of dct_clamp_fm_wave_kernel<CH>, steps padded to a multiple
                                   // of CH with zeros (nullptr: VALU kernel)
    int kb = 0, wave_nk = 0, ch = 0;
  } dctfm;
  struct Rf2k { bool ok = false; float* d_lane_tab = nullptr; } rf2k;   // rfft_wpf_kernel<4> (stage-isolated rFFT, n = 2048)
  AnyPlan any;                     // any-length STFT (mm_anyfft.hip.inc): n_fft that is not a power of two in [32, 4096]

  struct Switches {
    int variant = 0;               // mm_plan_set_variant: 0 = automatic
    int force_generic = 0;         // mm_plan_force_generic
    int no_fuse = 0;               // mm_plan_set_fuse_dct(0): always run the separate clamp + DCT kernel
    int no_fuse_tail = 0;          // mm_plan_set_fuse_tail(0): mm_mfcc_modspec_f32 always runs its separate launches
    int no_shared_runs = 0;        // mm_plan_set_shared_runs(0): fused launches walk the overlapping runs (A/B, cross-checks)
    int fuse_tail_wide = 0;        // mm_plan_set_fuse_tail(2): clip mode also for 2048-point trajectories and for mm_mfcc_f32 (empty filters)
  } user;
  struct Timing {
    int on = 0, ev_used = 0;
    std::vector<hipEvent_t> ev_pool;   // pairs
    std::vector<int> ev_stage;
    double t_sum[MM_NUM_STAGES] = {};
    int64_t t_cnt[MM_NUM_STAGES] = {};
  } timing;

  mm_plan() = default;
  mm_plan(const mm_plan&) = delete; mm_plan& operator=(const mm_plan&) = delete;
  ~mm_plan() { for (void* d : owned) (void)hipFree(d); }
  // device copy of a host table; the allocation is recorded before the copy, so a failed copy does not leak
  template <class T>
  int upload(T** dst, const void* src, size_t bytes) {
    HIP_TRY(hipMalloc((void**)dst, bytes));
    owned.push_back(*dst);
    HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return MM_OK;
  }

 private:
  std::vector<void*> owned;
};

namespace {

struct StageTimer {
  mm_plan* p;
  hipStream_t s;
  int idx;
  StageTimer(mm_plan* plan, int stage, hipStream_t stream) : p(plan), s(stream), idx(-1) {
    mm_plan::Timing& t = p->timing;
    if (!t.on || t.ev_used >= MM_MAX_TIMED) return;
    if (t.on != 1 && !((t.on >> (stage + 1)) & 1)) return;   // stage mask
    if ((size_t)(2 * t.ev_used + 1) >= t.ev_pool.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      t.ev_pool.push_back(a);
      t.ev_pool.push_back(b);
    }
    idx = t.ev_used++;
    t.ev_stage.resize(t.ev_used);
    t.ev_stage[idx] = stage;
    (void)hipEventRecord(t.ev_pool[2 * idx], s);
  }
  ~StageTimer() {
    if (idx >= 0) (void)hipEventRecord(p->timing.ev_pool[2 * idx + 1], s);
  }
};

}  // namespace
