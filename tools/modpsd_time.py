"""Welch modulation power spectrum timing (GPU box): three routes to scipy.signal.welch of float32 trajectories that are
already on the device, in one process.
    (a)  modulation_psd_batch / modulation_psd_ragged_batch (mm_modpsd_f32: one launch, two for more than 32 segments)
    (b)  the only route before it: the trajectories copied to the host and scipy.signal.welch there (the copy included)
    (c)  a torch composition on the device: unfold, detrend, window, torch.fft.rfft, |.|^2, mean over the segments
on two workloads:
    'batch'      1024 clips x 13 trajectories x 1001 frames at fs 200, nperseg 256 (Hann, half overlap, constant detrend), and
                 the same batch ragged at 200 .. 1001 frames ((a) only: (b) and (c) have no ragged form but a loop)
    'recording'  one 13 x 300 001 recording at fs 1000, nperseg 1024
Device events around each call (the host route: a host clock around copy + welch), warm-up first, median over the repeats;
(a) and (c) are compared with (b) before anything is timed.
    python tools/modpsd_time.py [--root TREE] [--clips B] [--reps N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import scipy.signal
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import modulation_psd_batch, modulation_psd_ragged_batch
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        ts = sorted(ts)
        return f"{ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls)"

    def timed(fn, clock=event_ms, reps=args.reps, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        return stats([clock(fn) for _ in range(reps)])

    def torch_welch(x, fs, nperseg):
        """Route (c): Hann, half overlap, constant detrend, 'density', nfft = nperseg."""
        w = torch.hann_window(nperseg, periodic=True, device=x.device, dtype=torch.float32)
        seg = x.unfold(-1, nperseg, nperseg // 2)                       # [rows, K, nperseg] view
        seg = (seg - seg.mean(dim=-1, keepdim=True)) * w
        P = torch.fft.rfft(seg, dim=-1).abs().square().mean(dim=-2)
        P = P * (1.0 / (fs * float((w.double() ** 2).sum())))
        P[..., 1:-1] *= 2
        return P

    def host_welch(x, fs, nperseg):
        """Route (b)."""
        return scipy.signal.welch(x.cpu().numpy(), fs=fs, nperseg=nperseg, axis=-1)[1]

    def workload(name, rows, n, fs, nperseg, host_reps):
        g = torch.Generator(device=dev).manual_seed(0)
        t = torch.arange(n, device=dev, dtype=torch.float32) / fs
        x = 20.0 + torch.sin(2 * np.pi * 4.0 * t) + 0.5 * torch.randn((rows, n), device=dev, generator=g)
        kw = dict(nperseg=nperseg)
        ref = host_welch(x, fs, nperseg)
        for what, got in (("(a)", modulation_psd_batch(x, fs, **kw)[1]), ("(c)", torch_welch(x, fs, nperseg))):
            err = float(np.abs(got.cpu().numpy() - ref).max() / ref.max())
            print(f"'{name}': {what} differs from (b) by {err:.1e} of the largest value", flush=True)
            assert err <= 1e-5, err
        print(f"'{name}': {rows} rows x {n} samples, fs {fs}, nperseg {nperseg}, "
              f"{(n - nperseg // 2) // (nperseg - nperseg // 2)} segments per row", flush=True)
        print(f"    (a) modulation_psd_batch:                 {timed(lambda: modulation_psd_batch(x, fs, **kw))}", flush=True)
        print(f"    (b) copy to the host + scipy.signal.welch: {timed(lambda: host_welch(x, fs, nperseg), wall_ms, host_reps, 1)}",
              flush=True)
        print(f"    (c) torch unfold / rfft / mean:            {timed(lambda: torch_welch(x, fs, nperseg))}", flush=True)
        return x

    x = workload("batch", args.clips * 13, 1001, 200.0, 256, 3)
    rng = np.random.default_rng(1)
    lens = rng.integers(200, 1002, size=x.shape[0]).astype(np.int64)
    lens[0] = 1001
    lens_dev = torch.from_numpy(lens).to(dev)
    P = modulation_psd_ragged_batch(x, lens_dev, 200.0, nperseg=256)[1]
    for b in (0, 1, 2, x.shape[0] - 1):
        if lens[b] >= 256:
            assert torch.equal(P[b:b + 1], modulation_psd_batch(x[b:b + 1, :int(lens[b])], 200.0, nperseg=256)[1]), b
    print(f"'batch' ragged at {lens.min()} .. {lens.max()} frames ({int((lens < 256).sum())} rows below nperseg: NaN), "
          f"sampled rows equal the rows alone bit for bit", flush=True)
    print(f"    (a) modulation_psd_ragged_batch, device lengths: "
          f"{timed(lambda: modulation_psd_ragged_batch(x, lens_dev, 200.0, nperseg=256))}", flush=True)
    del x, P
    workload("recording", 13, 300001, 1000.0, 1024, 5)


if __name__ == "__main__":
    main()
