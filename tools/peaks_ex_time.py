"""Timing of the staged peak search (GPU box): find_peaks_ex_batch(distance=5, prominence=0, width=1) on [1024, 2001]
float64 change-like curves and on one [1, 300001] row, the distance worst case (the 4101-sample ramp, distance=3), and the
old-arguments-only path -- find_peaks_batch(prominence=0) beside find_peaks_ex_batch(prominence=0) -- each with device
events, 3 warm-ups and 20 timed calls (median, min, max); beside them the copy to the host plus a scipy loop.
    python tools/peaks_ex_time.py                      # everything, of this tree
    python tools/peaks_ex_time.py --tree DIR           # the package of another checkout (one without find_peaks_ex_batch,
                                                       # e.g. the parent commit, times find_peaks_batch alone)
    python tools/peaks_ex_time.py --one batch|ex       # ONE call of the old-arguments path, for a kernel trace"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.signal

from peaks_time import curves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--one", choices=("batch", "ex"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import modulation_mfcc_amd as M
    dev = torch.device("cuda", 0)
    ex = getattr(M, "find_peaks_ex_batch", None)
    print(f"package: {os.path.dirname(M.__file__)} ({'with' if ex else 'without'} find_peaks_ex_batch)", flush=True)

    if args.one:
        d = torch.from_numpy(curves(1024, 2001, 1024)).to(dev)
        torch.cuda.synchronize()
        (M.find_peaks_batch if args.one == "batch" else ex)(d, prominence=0)
        torch.cuda.synchronize()
        return

    def dev_ms(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for a, b in ev)
        return f"{t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}; {args.reps} calls)"

    def host_ms(d, kw, reps=3):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = [scipy.signal.find_peaks(r, **kw) for r in d.cpu().numpy()]
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2], sum(len(p) for p, _ in out)

    full = dict(distance=5, prominence=0, width=1)
    for rows, n in ((1024, 2001), (1, 300001)):
        x = curves(rows, n, rows)
        d = torch.from_numpy(x).to(dev)
        tag = f"[{rows}, {n}] float64"
        for rep in range(2):            # the old path twice, the two functions alternating: the spread between repeats
            print(f"{tag} find_peaks_batch(prominence=0) #{rep}: {dev_ms(lambda: M.find_peaks_batch(d, prominence=0))}", flush=True)
            if ex:
                print(f"{tag} find_peaks_ex_batch(prominence=0) #{rep}: {dev_ms(lambda: ex(d, prominence=0))}", flush=True)
        if ex:
            cpu, peaks = host_ms(d, full)
            assert int(ex(d, **full)[1].sum()) == peaks
            print(f"{tag} find_peaks_ex_batch(distance=5, prominence=0, width=1), {peaks} peaks: {dev_ms(lambda: ex(d, **full))};  "
                  f"copy + scipy loop {cpu:.2f} ms", flush=True)
            for kw in (dict(distance=5), dict(prominence=0, wlen=41), dict(plateau_size=1)):
                print(f"{tag} find_peaks_ex_batch({kw}): {dev_ms(lambda: ex(d, **kw))}", flush=True)
    if ex:
        ramp = np.zeros((1, 4101))
        ramp[0, 1::2] = np.arange(1, 2051)
        d = torch.from_numpy(ramp).to(dev)
        cpu, peaks = host_ms(d, dict(distance=3))
        assert int(ex(d, distance=3)[1].sum()) == peaks == 1025
        print(f"ramp [1, 4101], distance=3 (1025 rounds in one launch), {peaks} peaks: {dev_ms(lambda: ex(d, distance=3))};  "
              f"copy + scipy {cpu:.2f} ms", flush=True)


if __name__ == "__main__":
    main()
