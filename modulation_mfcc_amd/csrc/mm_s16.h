// The staged-sample n_fft = 512 kernel (mm_logmel16s.hip.inc) is its own translation unit (124 instantiations): this
// header carries what the plan / dispatch code in mm_api.hip needs from it -- the LDS layout and the launch wrappers.
#pragma once
#include "mm_common.h"

// Power rows of this kernel.  XA instantiations (NR 3 / 4 only: long hops, BASELINE configs[1] / [2] / [4]) write the
// 16x16 exchange with ds_write_addtid_b32 and need pitch 268 (4 rows = 1072 >= the 1068 floats of mm_s16_xb's blocks;
// 268 = 4 x 67, 67 odd: phase B's lane-per-frame b128 reads stay conflict-free): 2 KB more LDS.  The others keep the
// ds_write_b32 exchange at pitch 260: NR 1 / 2 (the reference default, NR 1, ran 2.5 % slower with it) and every plan
// whose fused-DCT layout only fits without those 2 KB (setup_tile512 / setup_s16f in mm_api.hip: mm_plan::S16::xa).
#define MM_S16_XA_PITCH 268
#define MM_S16_PITCH(XA) ((XA) ? MM_S16_XA_PITCH : MM_LM_PITCH)
#define MM_S16_S_OFF(XA) (64 * MM_S16_PITCH(XA) * 4)
// 16x16 exchange (ds_write_addtid_b32: lane l of register k1 at mm_s16_xb(k1) + l).  Lane (row, q) reads block q,
// its frame's 16 floats at mm_s16_xb(q) + 16 row, as four b128 in chunk order; those reads are conflict-free when, in
// every b128 lane group, the sixteen lanes' 16-byte slots (mm_s16_xb(q) / 4 + 4 row) mod 16 differ: the blocks of
// q in {0..3, 12..15} and those of q in {4..11} each take slots {0..3, 8..11} once (tests/test_s16_layout.py).
// Block j = 0..15 lies at 64 j + 4 s_j, s_j = 0,0,1,1,2,2,3,3,8,8,9,9,..: 1068 floats.
__host__ __device__ constexpr int mm_s16_xb(int k1) {
  const int m = k1 < 4 ? k1 : (k1 >= 12 ? k1 - 8 : k1 - 4), j = 2 * m + ((k1 >= 4 && k1 < 12) ? 1 : 0);
  return 64 * j + 4 * ((m & 3) + 8 * (m >> 2));
}
// the layout tests/test_s16_layout.py models: these sixteen offsets, the area inside four rows, and every wave's area
// starting below 64 KB (an add-TID store's address is M0[15:0] + offset + 4 lane)
static_assert(mm_s16_xb(0) == 0 && mm_s16_xb(1) == 132 && mm_s16_xb(2) == 264 && mm_s16_xb(3) == 396 &&
              mm_s16_xb(4) == 64 && mm_s16_xb(5) == 196 && mm_s16_xb(6) == 328 && mm_s16_xb(7) == 460 &&
              mm_s16_xb(8) == 608 && mm_s16_xb(9) == 740 && mm_s16_xb(10) == 872 && mm_s16_xb(11) == 1004 &&
              mm_s16_xb(12) == 544 && mm_s16_xb(13) == 676 && mm_s16_xb(14) == 808 && mm_s16_xb(15) == 940,
              "exchange block offsets (tests/test_s16_layout.py)");
static_assert(1068 <= 4 * MM_S16_XA_PITCH && 15 * 4 * MM_S16_XA_PITCH * 4 < 65536, "exchange area of the XA layout");
#ifndef MM_S16F_CH
#define MM_S16F_CH 12     // DCT steps (4 filters each) whose operands are fetched together
#endif
#ifndef MM_S16F_W
#define MM_S16F_W 0.5     // mel share of a DCT wave relative to the other waves
#endif
// cuts of the shared-runs table (mm::build_mel_sweep's filter_cost = lead_cost): a run costs the walk ~58 instructions, a
// 4-bin group ~8.5 (balance_parts_over_simds), i.e. a filter weighs as much as ~27 bins
#ifndef MM_S16F_SH_FC
#define MM_S16F_SH_FC 27.0
#endif
#define MM_S16_LT_OFF(NR, XA) (MM_S16_S_OFF(XA) + (NR) * 16384)
#define MM_S16_TAB_OFF(NR, XA) (MM_S16_LT_OFF(NR, XA) + 16 * MM_W16_LT_PITCH * 4)

#define MM_S16_CPW_MAX 32         // clip mode: at most this many clips per workgroup (extreme slots in LDS, 128 B each)
#define MM_S16_FIN_REC 24
#define MM_S16_FIN_TAB_BYTES ((32 * MM_S16_FIN_REC + 15) * 8)
#define MM_S16_FIN_TAB_OFF (16 * 9216)
// clip mode, plans with empty filters: the per-clip add factors (a float per clip of the workgroup) lie behind the extreme
// slots of the launch's largest workgroup (clips_max x 128 B) and, at n_mod 2048, behind the 2048-point tail's buffers
#define MM_S16_DELTA_OFF(red_off, clips_max, n_mod)                                                             \
  (((n_mod) == 2048 && (red_off) + (clips_max) * 128 < MM_S16_FIN2K_BYTES) ? MM_S16_FIN2K_BYTES : (red_off) + (clips_max) * 128)
#define MM_S16_FIN2K_BYTES 103424   // n_mod 2048: lane table of the 2048-point transform (64 x 116 floats) + 16 x 4.5 KB exchange buffers

struct Logmel512Params;
// mode 0 power rows | 1 log-mel (+ fused DCT) | (1 with q.out_mod set ->) 2 clip mode; nr = 16-byte staging groups per thread;
// xa (nr 3 / 4 only): the ds_write_addtid_b32 exchange at pitch MM_S16_PITCH(true); sh: q carries a shared-runs table
// (mm::build_mel_runs_shared) -- only where s16_has_shared() says the instantiation exists
void launch_s16(int mode, int nr, bool xa, bool pre, bool odd, bool unal, bool sh, dim3 grid, size_t lds, hipStream_t st,
                const Logmel512Params& q);
bool s16_has_shared(int nr, bool xa, bool pre, bool odd, bool unal);
bool set_s16_attr(int bytes);       // hipFuncAttributeMaxDynamicSharedMemorySize on every instantiation (current device)
