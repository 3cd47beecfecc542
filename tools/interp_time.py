"""interp_NAN timing (GPU box): interp_NAN(device tensor, 'pchip') on the device (mm_interp_nan_f64) against the host
round trip it replaces -- the curve copied to the host, scipy's PchipInterpolator row by row in a Python loop
(interp._interp_nan_host, unchanged), the result copied back -- on [1024, 1000] float64 (a batch of ten-second f0 curves at
the 10 ms step) and on [1, 300001] (a five-minute recording at the 1 ms step).  Both are timed with device events around
the whole call, alternating in one process; the results are compared before anything is timed.  'linear' and 'nearest'
are timed on the device beside them.
    python tools/interp_time.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def f0_like(rows, n, seed):
    """f0-like curves: a slow random walk around 150 Hz with unvoiced gaps (NaN runs of 5 .. 40 samples, a third of the
    samples), NaN at both ends of every other row."""
    rng = np.random.default_rng(seed)
    x = 150 + np.cumsum(rng.standard_normal((rows, n)), axis=1) * 0.3
    for r in range(rows):
        i = int(rng.integers(0, 30))
        while i < n:
            g = int(rng.integers(5, 41))
            x[r, i:i + g] = np.nan
            i += g + int(rng.integers(10, 81))
        if r % 2:
            x[r, :3] = np.nan
            x[r, -4:] = np.nan
        else:
            x[r, 0] = x[r, -1] = 150.0
    return x


def host_round_trip(X, method):
    """What interp_NAN did with a device tensor for every method but 'linear' before mm_interp_nan_f64 existed."""
    import torch
    from modulation_mfcc_amd import interp
    rows = X.cpu().numpy()
    out = interp._interp_nan_host(rows, method) if rows.ndim == 1 else np.stack([interp._interp_nan_host(r, method) for r in rows])
    return torch.from_numpy(np.ascontiguousarray(out)).to(X.device)


def main():
    import torch
    from modulation_mfcc_amd import interp_NAN
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

    for rows, n, host_reps in ((1024, 1000, 5), (1, 300001, 10)):
        x = f0_like(rows, n, rows)
        d = torch.from_numpy(x).to(dev)
        d1 = d if rows > 1 else d[0]
        got, want = interp_NAN(d1, "pchip").cpu().numpy(), host_round_trip(d1, "pchip").cpu().numpy()
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-12, err
        fns = {"device pchip": lambda: interp_NAN(d1, "pchip"), "host round trip pchip": lambda: host_round_trip(d1, "pchip")}
        for fn in fns.values():                               # warm-up: code objects, scipy imports, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for rep in range(host_reps):                          # alternating: 40 device calls, then one host call
            t["device pchip"] += [one_ms(fns["device pchip"]) for _ in range(40)]
            t["host round trip pchip"].append(one_ms(fns["host round trip pchip"]))
        print(f"[{rows}, {n}] float64, {int(np.isnan(x).sum())} NaN samples, max rel. difference device / host {err:.1e}", flush=True)
        for k in fns:
            print(f"    {k}: {stats(t[k])}", flush=True)
        for method in ("linear", "nearest"):
            for _ in range(3):
                interp_NAN(d1, method)
            print(f"    device {method}: {stats([one_ms(lambda: interp_NAN(d1, method)) for _ in range(100)])}", flush=True)


if __name__ == "__main__":
    main()
