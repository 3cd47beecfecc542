"""Long FIR / Savitzky-Golay filter timing (GPU box): applyFilter on device curves with filters beyond the banded stencil,
    fir101   applyFilter(x, 100.0, filt='fir', cutOff=[12], filtLen=101)              x [256, 160000] float64
    sg101    applyFilter(x, 100.0, filt='sg', cutOff=[12], filtLen=101, polyOrd=3)    the same rows
    fir501   applyFilter(x, 100.0, filt='fir', cutOff=[12], filtLen=501)              x [300001] float64 (one long curve)
on the device (mm_fir_filtfilt_f64 / mm_savgol_f64) against the host round trip these calls made before those kernels
existed: the curves copied to the host, the reference's scipy call (filtfilt / savgol_filter, one core), the result copied
back.  Device events around the whole call, warm-up first, the two alternating in one process, median over the repeats; the
results are compared before anything is timed.  A torch.nn.functional.conv1d float64 row (the 201-tap correlation of fir101
without its extension) stands beside them where the backend offers it.
    python tools/longfilt_time.py [--root TREE] [--host-reps N] [--conv1d]
--root TREE imports the package from another checkout (the parent commit: there applyFilter IS the round trip)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def curves(rows, n, seed):
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal((rows, n)).cumsum(axis=1)) + rng.standard_normal((rows, n))


def host_round_trip(x, sr, **kw):
    """What applyFilter did with a device tensor for filters beyond the stencil: scipy on the host, copied both ways."""
    import torch
    from modulation_mfcc_amd import applyFilter
    y = applyFilter(x.cpu().numpy(), sr, **kw)
    return torch.from_numpy(np.ascontiguousarray(y)).to(x.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=20)
    ap.add_argument("--conv1d", action="store_true", help="also time the backend's float64 conv1d on the fir101 rows")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import applyFilter
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
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

    big = torch.from_numpy(curves(256, 160000, 1)).to(dev)
    one = torch.from_numpy(curves(1, 300001, 2)[0]).to(dev)
    cases = (("fir101", big, 100.0, dict(filt="fir", cutOff=[12], filtLen=101)),
             ("sg101", big, 100.0, dict(filt="sg", cutOff=[12], filtLen=101, polyOrd=3)),
             ("fir501", one, 100.0, dict(filt="fir", cutOff=[12], filtLen=501)))
    for name, x, sr, kw in cases:
        fns = {"applyFilter(device tensor)": lambda: applyFilter(x, sr, **kw), "host round trip": lambda: host_round_trip(x, sr, **kw)}
        got, want = (fn() for fn in fns.values())                 # (also the first call of each: code objects, tables)
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 1e-9, err                                   # the host's own error at 101 samples, order 3 is ~1e-11
        for _ in range(2):
            fns["applyFilter(device tensor)"]()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.host_reps):                           # alternating
            t["applyFilter(device tensor)"] += [one_ms(fns["applyFilter(device tensor)"]) for _ in range(args.device_reps)]
            t["host round trip"].append(one_ms(fns["host round trip"]))
        print(f"{name}: {tuple(x.shape)} float64, {kw}; max rel. difference {err:.1e}", flush=True)
        for k in fns:
            print(f"    {k}: {stats(t[k])}", flush=True)

    if not args.conv1d:
        return
    # the interior of fir101 as a float64 convolution of the backend: 256 x 160 000 outputs x 201 taps
    import scipy.signal
    b = scipy.signal.firwin(101, 12.0 / 50.0, window=("kaiser", 7.4))
    h = torch.from_numpy(np.convolve(b, b[::-1])).to(dev)[None, None, :]
    try:
        f = lambda: torch.nn.functional.conv1d(big[:, None, :], h, padding=100)      # noqa: E731
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        print(f"conv1d float64 [256, 1, 160000] x 201 taps: {stats([one_ms(f) for _ in range(10)])}", flush=True)
    except Exception as e:      # noqa: BLE001  (no float64 convolution in this backend: a missing row, not a failure)
        print(f"conv1d float64: not available here ({type(e).__name__}: {str(e).splitlines()[0][:100]})", flush=True)


if __name__ == "__main__":
    main()
