"""Spline gap filling timing (GPU box): interp_nan_spline_batch / interp_nan_spline_ragged_batch (mm_interp_spline_f64) against
the route they replace -- the curves copied to the host, scipy's interp1d row by row (interp._interp_nan_host, unchanged),
the result copied back: what interp_NAN(device tensor, 'quadratic' | 'cubic') does -- and against
interp_nan_batch(..., 'pchip') as the floor, on [1024, 1001] float64 f0-like rows, on the same rows ragged at 200 .. 1001
samples, and on [1, 300001].  Every call is timed whole with device events (the wrappers' one read-back included),
warmed, repeated, the median printed with the extremes; device and host calls alternate in one process; the results are
compared before anything is timed.
    python tools/spline_time.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from interp_time import f0_like


def host_round_trip(X, method, counts=None):
    import torch
    from modulation_mfcc_amd import interp
    rows = X.cpu().numpy()
    if counts is None:
        out = np.stack([interp._interp_nan_host(r, method) for r in rows])
    else:
        out = np.zeros_like(rows)
        for b, c in enumerate(counts):
            out[b, :c] = interp._interp_nan_host(rows[b, :c], method)
    return torch.from_numpy(np.ascontiguousarray(out)).to(X.device)


def main():
    import torch
    from modulation_mfcc_amd import (interp_nan_batch, interp_nan_ragged_batch, interp_nan_spline_batch,
                                     interp_nan_spline_ragged_batch)
    dev = torch.device("cuda", 0)

    def one_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(t):
        t = sorted(t)
        return f"{t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}; {len(t)} calls)"

    for rows, n, ragged, host_reps in ((1024, 1001, False, 3), (1024, 1001, True, 3), (1, 300001, False, 5)):
        x = f0_like(rows, n, rows)
        counts = None
        if ragged:
            counts = np.linspace(200, n, rows).astype(np.int64)
            for b, c in enumerate(counts):
                x[b, c - 1] = 150.0                       # (a valid last sample, as in the even rows of the full batch)
        d = torch.from_numpy(x).to(dev)
        cd = None if counts is None else torch.from_numpy(counts).to(dev)
        shape = f"[{rows}, {n}]" + (" ragged at 200 .. 1001" if ragged else "")
        print(f"{shape} float64, {int(np.isnan(x).sum())} NaN samples", flush=True)
        for method in ("quadratic", "cubic"):
            if ragged:
                fns = {"device": lambda: interp_nan_spline_ragged_batch(d, cd, method),
                       "host round trip": lambda: host_round_trip(d, method, counts)}
            else:
                fns = {"device": lambda: interp_nan_spline_batch(d, method), "host round trip": lambda: host_round_trip(d, method)}
            got, want = fns["device"]().cpu().numpy(), fns["host round trip"]().cpu().numpy()
            err = max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got, want))
            assert err <= 1e-10, err
            for fn in fns.values():                               # warm-up: code objects, scipy imports, allocator
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in fns}
            for rep in range(host_reps):                          # alternating: 40 device calls, then one host call
                t["device"] += [one_ms(fns["device"]) for _ in range(40)]
                t["host round trip"].append(one_ms(fns["host round trip"]))
            print(f"  {method}: largest difference device / host, relative to the row's maximum: {err:.1e}", flush=True)
            for k in fns:
                print(f"    {k} {method}: {stats(t[k])}", flush=True)
        floor = (lambda: interp_nan_ragged_batch(d, cd, "pchip")) if ragged else (lambda: interp_nan_batch(d, "pchip"))
        for _ in range(3):
            floor()
        print(f"    device pchip (the floor): {stats([one_ms(floor) for _ in range(100)])}", flush=True)


if __name__ == "__main__":
    main()
