"""Lomb-Scargle timing (GPU box): modulation_lombscargle_batch / _ragged_batch (mm_lombscargle_f64) against
  (a) the route without it: the rows copied to the host, scipy.signal.lombscargle on the valid samples row by row, the
      result copied back;
  (b) a float64 torch composition on the device: cos / sin of the outer product t x omega, one matmul per sum with the mask
      as a factor, the same epilogue elementwise -- the honest competitor,
on [1024, 1001] f0-like rows (a third NaN) x 200 frequencies, the same rows ragged at 200 .. 1001 samples, and one row of
300 001 samples (70 % valid) x 64 frequencies; floating_mean=True, normalize='power'.  Every call is timed whole with
device events, warmed, repeated, the median printed with the extremes; the results are compared before anything is timed.
    python tools/lomb_time.py                 the three shapes, the three routes
    python tools/lomb_time.py --device-only   a few device calls per shape (for rocprofv3 --kernel-trace --stats -- python ...)
MODMFCC_LIB selects a side build of the library (make OBJDIR=build_rt4 OUT=../libmodmfcc_rt4.so
EXTRA=-DMM_LOMB_ROW_TILES=4): the row tiles a wave carries."""
import os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from interp_time import f0_like

KW = dict(floating_mean=True, normalize="power")


def host_route(X, t, f, counts=None):
    import torch
    from scipy.signal import lombscargle
    rows = X.cpu().numpy()
    omega = 2.0 * np.pi * f
    out = np.empty((rows.shape[0], f.shape[0]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b, r in enumerate(rows):
            v = ~np.isnan(r)
            if counts is not None:
                v[counts[b]:] = False
            out[b] = lombscargle(t[v], r[v], omega, **KW)
    return torch.from_numpy(out).to(X.device)


def torch_route(X, td, od, cd=None):
    """The one-pass sums as six float64 matmuls, the mask as a factor; floating mean, 'power'."""
    import torch
    m = ~torch.isnan(X)
    if cd is not None:
        m &= torch.arange(X.shape[1], device=X.device)[None, :] < cd[:, None]
    y = torch.where(m, X, torch.zeros((), dtype=X.dtype, device=X.device))
    m = m.to(torch.float64)
    ang = td[:, None] * od[None, :]
    cw, sw = torch.cos(ang), torch.sin(ang)
    K = m.sum(dim=1, keepdim=True)
    w = 1.0 / K
    C0, S0, CC0, CS0 = (m @ cw) * w, (m @ sw) * w, (m @ (cw * cw)) * w, (m @ (cw * sw)) * w
    YC0, YS0, Y = (y @ cw) * w, (y @ sw) * w, y.sum(dim=1, keepdim=True) * w
    SS0 = 1.0 - CC0
    tau = 0.5 * torch.atan2(2.0 * (CS0 - C0 * S0), (CC0 - C0 * C0) - (SS0 - S0 * S0))
    c, s = torch.cos(tau), torch.sin(tau)
    Cr, Sr = C0 * c + S0 * s, S0 * c - C0 * s
    YC, YS = YC0 * c + YS0 * s - Y * Cr, YS0 * c - YC0 * s - Y * Sr
    CC = (c * c) * CC0 + (2.0 * c * s) * CS0 + (s * s) * SS0
    SS = (1.0 - CC - Sr * Sr).clamp_min(2.0 ** -53)
    CC = (CC - Cr * Cr).clamp_min(2.0 ** -53)
    return 2.0 * (YC * YC / CC + YS * YS / SS) * (K / 4.0)


def long_row(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 100.0
    x = 4.0 + 8.0 * np.sin(2 * np.pi * 3.1 * t) + 0.5 * rng.standard_normal(n)
    x[rng.random(n) < 0.3] = np.nan
    return x[None, :]


def main():
    import torch
    from modulation_mfcc_amd import _lib, modulation_lombscargle_batch, modulation_lombscargle_ragged_batch
    device_only = "--device-only" in sys.argv
    dev = torch.device("cuda", 0)
    print(f"library: {_lib.LIB_PATH}", flush=True)

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

    fs = 100.0
    for rows, n, nf, ragged in ((1024, 1001, 200, False), (1024, 1001, 200, True), (1, 300001, 64, False)):
        x = f0_like(rows, n, rows) if rows > 1 else long_row(n, 7)
        counts = None
        if ragged:
            counts = np.linspace(200, n, rows).astype(np.int64)
            x[:, 0] = 150.0
        t = np.arange(n) / fs
        f = np.linspace(2.0 / (n / fs), 0.45 * fs if rows > 1 else 40.0, nf)
        d, td, od = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(2.0 * np.pi * f).to(dev)
        cd = None if counts is None else torch.from_numpy(counts).to(dev)
        shape = f"[{rows}, {n}] x {nf} frequencies" + (" ragged at 200 .. 1001" if ragged else "")
        print(f"{shape}, float64, {int(np.isnan(x).sum())} NaN samples", flush=True)
        device = (lambda: modulation_lombscargle_ragged_batch(d, cd, fs, f, **KW)) if ragged else \
            (lambda: modulation_lombscargle_batch(d, fs, f, **KW))
        if device_only:
            for _ in range(5):
                device()
            torch.cuda.synchronize()
            continue
        fns = {"device": device, "torch float64 composition": lambda: torch_route(d, td, od, cd),
               "host round trip (scipy per row)": lambda: host_route(d, t, f, counts)}
        got = {k: fn().cpu().numpy() for k, fn in fns.items()}
        want = got["host round trip (scipy per row)"]
        for k in ("device", "torch float64 composition"):
            err = max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got[k], want))
            print(f"  {k}: largest difference from scipy, relative to the row's maximum: {err:.1e}", flush=True)
            assert err <= 1e-9, err
        for k in ("device", "torch float64 composition"):
            for _ in range(3):
                fns[k]()
        torch.cuda.synchronize()
        tm = {k: [] for k in fns}
        for rep in range(3):                                   # alternating: 20 calls of each device route, then (once) the host
            tm["device"] += [one_ms(fns["device"]) for _ in range(20)]
            tm["torch float64 composition"] += [one_ms(fns["torch float64 composition"]) for _ in range(20)]
        tm["host round trip (scipy per row)"].append(one_ms(fns["host round trip (scipy per row)"]))
        for k in fns:
            print(f"    {k}: {stats(tm[k])}", flush=True)
        valid = float((~np.isnan(x)).sum()) if counts is None else float(sum((~np.isnan(x[b, :c])).sum() for b, c in enumerate(counts)))
        dense = 12.0 * rows * n * nf                               # six products, 2 flop each, masked samples included
        print(f"    contraction: {dense / 1e9:.2f} GFLOP dense ({12.0 * valid * nf / 1e9:.2f} on valid samples)", flush=True)


if __name__ == "__main__":
    main()
