"""Peak-search timing (GPU box): find_peaks_batch on [1024, 1001] float64 change-like curves (the headline batch) and on one
[1, 300001] curve (a five-minute recording at the 1 ms step), each bare and with prominence=0, timed with device events
behind warm-ups; beside them the copy to the host plus a Python loop of scipy.signal.find_peaks over the same rows.
    python tools/peaks_time.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.signal


def curves(rows, n, seed):
    """Smooth positive curves with the look of an MFCC change: low-passed noise, a few peaks per hundred samples."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n + 24))
    k = np.hanning(25)
    k /= k.sum()
    return np.abs(np.stack([np.convolve(r, k, mode="valid") for r in x]))


def main():
    import torch
    from modulation_mfcc_amd import find_peaks_batch
    dev = torch.device("cuda", 0)

    def dev_ms(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for a, b in ev)
        return t[len(t) // 2], t[0], t[-1]

    def host_ms(d, kw, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = d.cpu().numpy()
            out = [scipy.signal.find_peaks(r, **kw) for r in h]
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2], len(out)

    for rows, n in ((1024, 1001), (1, 300001)):
        x = curves(rows, n, rows)
        d = torch.from_numpy(x).to(dev)
        peaks = sum(len(scipy.signal.find_peaks(r)[0]) for r in x)
        for kw in ({}, {"prominence": 0}):
            idx, count, _ = find_peaks_batch(d, **kw)
            assert int(count.sum()) == peaks
            med, lo, hi = dev_ms(lambda: find_peaks_batch(d, **kw), 20, 200)
            cpu, _ = host_ms(d, kw, 5)
            print(f"[{rows}, {n}] float64, {peaks} peaks, {kw or 'no conditions'}: find_peaks_batch {med:.3f} ms "
                  f"(min {lo:.3f}, max {hi:.3f}; 200 calls);  copy + scipy loop {cpu:.2f} ms", flush=True)


if __name__ == "__main__":
    main()
