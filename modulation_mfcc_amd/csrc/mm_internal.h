// Internal declarations shared by mm_tables.cpp (host tables) and the .hip translation units (device code + C ABI).
#ifndef MM_INTERNAL_H
#define MM_INTERNAL_H

#include <vector>

#include "../../include/modmfcc.h"

namespace mm {

struct MelCsr {
  std::vector<int> start, len, off;  // per filter: first bin, run length, offset into w
  std::vector<float> w;
};

// Sweep form of the mel matrix for the lane<->frame kernels: every bin k feeds at most the
// "falling" filter d[k] (weight wlo) and the "rising" filter d[k]+1 (weight whi), d monotone.
struct MelSweep {
  std::vector<float> wlo, whi;
  std::vector<int> d;
  std::vector<int> part;  // [n_waves][4] = {k_begin, k_end, m_begin, m_end}
};
// weights (optional, [n_waves]): relative share of the sweep cost each wave should get (default: equal).  The cost of a
// part is its bins + filter_cost per filter; lead_cost is charged once, to the first part (its run -1 in the shared form).
bool build_mel_sweep(const mm_config& c, const float* dense, int n_waves, MelSweep* out, const double* weights = nullptr,
                     double filter_cost = 6.0, double lead_cost = 0.0);

// Run form of the sweep for the fused kernel's phase B.  A "run" is the set of bins with one value
// of d; per wave the runs d = m_begin-1 .. m_end-1 are listed in order.  Bins are handled in
// aligned groups of 4 (one ds_read_b128 of the power row); weights outside the run are zero.
struct MelRuns {
  std::vector<int> hdr;     // [n_runs][4] = {first bin (multiple of 4), n_groups, first group, d}
  std::vector<float> grp;   // [n_groups][8] = {wlo x4, whi x4}
  std::vector<int> part;    // [n_waves][4] = {run_begin, run_end, m_begin, m_end}
};
void build_mel_runs(const mm_config& c, const MelSweep& sw, int n_waves, MelRuns* out);
// "Shared runs": every run d = -1 .. n_mels-1 is listed ONCE.  The first part with a filter starts at run m_begin-1 as
// above; every other one starts at run m_begin, and the rising half of its first filter (run m_begin-1) comes from the
// part before it, whose last run keeps both weights: its second sum is handed over.  part[w][3] = m_end | flags.
#define MM_RUNS_CONSUMER (1 << 16)       // the part's first filter takes its rising half from the part before
#define MM_RUNS_PRODUCER (1 << 17)       // the part's last run hands its second sum (filter m_end's rising half) over
void build_mel_runs_shared(const mm_config& c, const MelSweep& sw, int n_waves, MelRuns* out);

int validate(const mm_config* c);
void build_window(const mm_config& c, float* out);
void build_mel(const mm_config& c, float* out);
void build_dct(const mm_config& c, float* out);
void build_twiddles(int n, float* out);
int build_butter_sos(int order, double wn, double* sos);
void build_mel_csr(const mm_config& c, const float* dense, MelCsr* csr);

}  // namespace mm
#endif
