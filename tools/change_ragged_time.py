"""Ragged MFCC-change tail timing (GPU box): 1024 clips x 13 MFCC, T_b drawn uniformly from [200, 1001] (seed 0), the
reference's default filters (order-6 Butterworth at 12 Hz twice, 10 ms step).  Timed with device events around the whole
Python call, the candidates alternating in one process; the results are compared before anything is timed.
    (a) MfccPlan.mfcc_change_ragged: one launch with a length per clip
    (b) what was the only correct route before it: one mfcc_change per distinct length, scattered into a zeroed output
    (c) the single-length mfcc_change at T = 1001 on the same batch (wrong for the shorter clips, more arithmetic: the
        launch the ragged kernel was derived from)
    (d) the ragged call with every T_b = 1001 against (c): the cost of the length-awareness itself
Every figure is a whole call (workspace allocation, table uploads and the kernel), which is what a user pays.
    python tools/change_ragged_time.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    import torch
    from modulation_mfcc_amd import MfccConfig, get_plan, tail
    from modulation_mfcc_amd.plan import by_length
    dev = torch.device("cuda", 0)
    plan = get_plan(MfccConfig(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0))
    B, Tm = 1024, 1001
    rng = np.random.default_rng(0)
    frames = rng.integers(200, Tm + 1, B).astype(np.int64)
    frames[0] = Tm
    m = rng.standard_normal((B, 13, Tm)).cumsum(axis=2).astype(np.float32)
    for b, T in enumerate(frames):
        m[b, :, T:] = 0.0
    d = torch.from_numpy(m).to(dev)
    sos = tail.design_lowpass(6, 12, 0.01)
    fr_dev = torch.from_numpy(frames).to(dev)
    full_dev = torch.full((B,), Tm, dtype=torch.int64, device=dev)
    groups = [(T, torch.from_numpy(idx).to(dev)) for T, idx in by_length(frames)]

    def ragged():
        return plan.mfcc_change_ragged(d, fr_dev, sos, sos)

    def per_length():
        out = torch.zeros((B, Tm), dtype=torch.float64, device=dev)
        for T, ii in groups:
            out[ii, :T] = plan.mfcc_change(d[ii, :, :T], sos, sos)
        return out

    def single():
        return plan.mfcc_change(d, sos, sos)

    def ragged_full():
        return plan.mfcc_change_ragged(d, full_dev, sos, sos)

    # results first: (a) against (b) clip by clip, (d) against (c)
    a, b_, c, e = ragged(), per_length(), single(), ragged_full()
    scale = b_.abs().amax(dim=1, keepdim=True)
    err_ab = float(((a - b_).abs() / scale).max())
    err_dc = float(((e - c).abs() / c.abs().amax(dim=1, keepdim=True)).max())
    short = torch.from_numpy(frames < Tm).to(dev)
    err_cb = float((((c - b_).abs() * (b_ != 0)) / scale)[short].max())
    assert err_ab <= 1e-10 and err_dc <= 1e-10, (err_ab, err_dc)
    print(f"{B} clips x 12 rows, T_b in [{frames.min()}, {frames.max()}] ({len(groups)} distinct lengths, mean {frames.mean():.0f}), T_max {Tm}")
    print(f"    max difference / clip maximum: ragged vs per-length {err_ab:.1e}; ragged(all 1001) vs single-length {err_dc:.1e}; "
          f"single-length on the padded batch vs per-length, shorter clips {err_cb:.1e}", flush=True)

    def one_ms(fn):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        return s.elapsed_time(t)

    def stats(t):
        t = sorted(t)
        return f"{t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}; {len(t)} calls)"

    fns = {"(a) ragged, one launch": ragged, "(c) single-length T=1001": single, "(d) ragged, every T_b=1001": ragged_full,
           "(b) one call per distinct length": per_length}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for rep in range(10):                       # alternating: 30 calls each of (a), (c), (d), then one of (b)
        for _ in range(30):
            for k in list(fns)[:3]:
                t[k].append(one_ms(fns[k]))
        t["(b) one call per distinct length"].append(one_ms(per_length))
    for k in fns:
        print(f"    {k}: {stats(t[k])}", flush=True)
    # 20 calls between two events: the host runs ahead of the device, so this is the larger of host and device time per call
    for k in list(fns)[:3]:
        per = []
        for _ in range(10):
            s, u = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                fns[k]()
            u.record()
            torch.cuda.synchronize()
            per.append(s.elapsed_time(u) / 20)
        print(f"    {k}, 20 calls back to back, per call: {stats(per)}", flush=True)
    # the launches alone (table uploads + kernel): the library's own events around them, alternating rounds of 20 calls
    dev_ms = {k: [] for k in list(fns)[:3]}
    plan.timing_enable(True, stages=["change"])
    plan.timing_read()
    for rep in range(10):
        for k in dev_ms:
            for _ in range(20):
                fns[k]()
            ms, n = plan.timing_read()["change"]
            dev_ms[k].append(ms / n)
    plan.timing_enable(False)
    for k in dev_ms:
        print(f"    {k}, launches only (library events), per call: {stats(dev_ms[k])}", flush=True)


if __name__ == "__main__":
    main()
